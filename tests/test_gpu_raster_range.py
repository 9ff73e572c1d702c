"""Range mode of the HIP rasterizer (tt_rast_range_*, tt_aa_range_*; raster.rasterize(pos (V,4), tri, ranges=...)):
several meshes in one call must give, image by image, the bits of instance mode on the image's own sub-mesh; the
float64 oracle of the contract (tests/raster_reference.py) per image; interpolate / antialias forward; the gradient of
an antialias(interpolate(...)) loss to the shared vertex buffer and attributes; argument errors."""
import math
import os
import sys

import pytest
import torch

from triplaneturbo_amd import ops, raster, synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
H = W = 32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def perspective(fovy_deg, aspect, near=0.1, far=1000.0):
    t = math.tan(math.radians(fovy_deg) / 2)
    P = torch.zeros(4, 4)
    P[0, 0], P[1, 1] = 1 / (t * aspect), -1 / t
    P[2, 2], P[2, 3], P[3, 2] = -(far + near) / (far - near), -2 * far * near / (far - near), -1
    return P


def random_mvp(gen):
    """one perspective camera looking at the origin from a seeded random direction and distance"""
    az, el, rel = (torch.rand(3, generator=gen) * torch.tensor([360.0, 50.0, 0.5]) + torch.tensor([0.0, -25.0, 0.8])).tolist()
    _, _, c2w, _ = synthetic.make_cameras(1, H, W, fovy_deg=60.0, rel_distance=rel, elevation_deg=el, azimuth_start_deg=az)
    return (perspective(60.0, W / H)[None] @ torch.inverse(c2w))[0]


def clip(v, mvp):
    return torch.cat([v, torch.ones(v.shape[0], 1, dtype=v.dtype)], -1) @ mvp.t().to(v.dtype)


def octahedron():
    v = 0.6 * torch.tensor([[1.0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    t = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    return v, t.int()


def icosphere():
    """an icosahedron subdivided once: 42 vertices, 80 triangles"""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1),
         (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [list(map(float, x)) for x in v]
    mid = {}

    def m(a, b):
        key = (min(a, b), max(a, b))
        if key not in mid:
            mid[key] = len(v)
            v.append([(x + y) / 2 for x, y in zip(v[a], v[b])])
        return mid[key]

    out = []
    for a, b, c in f:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    vt = torch.tensor(v)
    return 0.55 * vt / vt.norm(dim=1, keepdim=True), torch.tensor(out, dtype=torch.int32)


def mc_sphere(dev):
    """marching cubes of a sphere on a 16^3 grid; more than 1024 triangles so that the scan of the slots' pixel
    counts spans more than one TT_XSCAN_SPAN block (20^3 if the 16^3 mesh were smaller)"""
    for res in (16, 20):
        x = torch.linspace(-1, 1, res, device=dev)
        g = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), -1)
        v, t = ops.marching_cubes(g.norm(dim=-1) - 0.8)
        if t.shape[0] > 1024:
            break
    assert t.shape[0] > 1024, t.shape
    return ((v * 2 - 1) * 0.7).cpu(), t.cpu().int()


class Scene:
    """three meshes under their own cameras, packed; image b of a range-mode call shows `pieces[b]`"""

    def __init__(self, dev, ranges_of):
        gen = torch.Generator().manual_seed(20)
        meshes = [octahedron(), icosphere(), mc_sphere(dev)]
        self.pos = [clip(v, random_mvp(gen)).float() for v, _ in meshes]   # CPU (V_i,4)
        self.tri = [t for _, t in meshes]
        self.attr = [torch.randn(v.shape[0], 3, generator=gen) for v, _ in meshes]
        pk = raster.pack_ranges(self.pos, self.tri)
        self.t_ofs, self.v_ofs = pk.tri_offsets, pk.vertex_offsets
        self.tri_cat, self.n_tri = pk.tri, pk.tri.shape[0]
        self.ranges = torch.tensor(ranges_of(pk.tri_offsets, [t.shape[0] for t in self.tri]), dtype=torch.int32)
        self.color = torch.rand(self.ranges.shape[0], H, W, 3, generator=gen)
        self.wts = torch.randn(self.ranges.shape[0], H, W, 3, generator=gen)

    def piece(self, b):
        """(pos (V,4), tri (T,3) with indices into it, attr (V,3), mesh number or None) of image b: the image's mesh
        with its own local indices, or, for a range over several meshes, the packed buffers and the range's rows"""
        first, count = self.ranges[b].tolist()
        for i, t0 in enumerate(self.t_ofs):
            if first == t0 and count == self.tri[i].shape[0]:
                return self.pos[i], self.tri[i], self.attr[i], i
        return torch.cat(self.pos), self.tri_cat[first:first + count], torch.cat(self.attr), None


def five_images(t_ofs, n):  # mc, octahedron, nothing, icosphere, octahedron again: scrambled, repeated, count = 0
    return [[t_ofs[2], n[2]], [t_ofs[0], n[0]], [5, 0], [t_ofs[1], n[1]], [t_ofs[0], n[0]]]


def two_meshes_in_one(t_ofs, n):  # the sixth variant: image 1's range covers the octahedron and the icosphere
    return [[t_ofs[2], n[2]], [t_ofs[0], n[0] + n[1]], [0, 0], [t_ofs[1], n[1]], [t_ofs[0], n[0]]]


@pytest.fixture(scope="module", params=[five_images, two_meshes_in_one], ids=["five_images", "two_meshes_in_one"])
def case(request, dev):
    """the scene, its range-mode rast and, per image, the instance-mode rast of the image's sub-mesh (computed once)"""
    s = Scene(dev, request.param)
    pos, tri = torch.cat(s.pos).to(dev), s.tri_cat.to(dev)
    rast = raster.rasterize(pos, tri, (H, W), ranges=s.ranges)
    inst = []
    for b in range(s.ranges.shape[0]):
        p, t, _, _ = s.piece(b)
        inst.append(raster.rasterize(p[None].to(dev), t.to(dev), (H, W)))
    return s, pos, tri, rast, inst


def test_rasterize_equals_instance_mode_bitwise(case):
    s, pos, tri, rast, inst = case
    assert rast.shape == (5, H, W, 4)
    for b, (first, count) in enumerate(s.ranges.tolist()):
        ids = rast[b, ..., 3]
        want = inst[b][0]
        assert torch.equal(rast[b, ..., :3], want[..., :3]), b  # u, v, z/w: the same bits
        assert torch.equal(torch.where(ids > 0, ids - first, ids), want[..., 3]), b  # global id = first + local id
        if count == 0:
            assert rast[b].abs().max() == 0
        else:
            assert (ids > 0).float().mean() > 0.05, b
            assert ids[ids > 0].min() >= first + 1 and ids.max() <= first + count
    assert torch.equal(rast, raster.rasterize(pos, tri, (H, W), ranges=s.ranges))  # bit-identical launches


def test_rasterize_matches_oracle(case):
    """the comparison rule of tests/test_gpu_raster.py::test_rasterize_matches_oracle_and_repeats_bitwise (_check_rast):
    under 1e-3 of the pixels ambiguous, equal ids and (u, v, z/w) within 1e-5 on the others"""
    s, _, _, rast, _ = case
    refs, ambs, got = [], [], rast.cpu().double()
    for b, (first, count) in enumerate(s.ranges.tolist()):
        p, t, _, _ = s.piece(b)
        ref, amb = R.rasterize(p.double()[None], t, H, W)
        refs.append(ref[0])
        ambs.append(amb[0])
        got[b, ..., 3] = torch.where(got[b, ..., 3] > 0, got[b, ..., 3] - first, got[b, ..., 3])
    ref, amb = torch.stack(refs), torch.stack(ambs)
    ok = ~amb
    assert amb.float().mean() < 1e-3, amb.float().mean()
    assert torch.equal(got[..., 3][ok], ref[..., 3][ok]), (got[..., 3][ok] != ref[..., 3][ok]).sum()
    assert (got[..., :3][ok] - ref[..., :3][ok]).abs().max() <= 1e-5


def test_interpolate_and_antialias_equal_instance_mode_bitwise(case, dev):
    s, pos, tri, rast, inst = case
    feat = raster.interpolate(torch.cat(s.attr).to(dev), rast, tri)  # 2-D attr
    color = s.color.to(dev)
    aa = raster.antialias(color, rast, pos, tri)
    assert feat.shape == (5, H, W, 3) and aa.shape == (5, H, W, 3)
    for b in range(5):
        p, t, a, _ = s.piece(b)
        assert torch.equal(feat[b:b + 1], raster.interpolate(a[None].to(dev), inst[b], t.to(dev))), b
        assert torch.equal(aa[b:b + 1], raster.antialias(color[b:b + 1], inst[b], p[None].to(dev), t.to(dev))), b
    assert (aa != color).any()
    # the table assembled by pack_ranges, through the context
    pk = raster.pack_ranges([x.to(dev) for x in s.pos], [x.to(dev) for x in s.tri],
                            [raster.edge_topology(t.to(dev), p.shape[0]) for p, t in zip(s.pos, s.tri)])
    ctx = raster.RasterizerContext("cuda", dev)
    assert torch.equal(ctx.antialias(color, rast, pk.pos, pk.tri, topology=pk.topology), aa)
    assert torch.equal(ctx.antialias(color, rast, pk.pos, pk.tri), aa)
    assert torch.equal(ctx.rasterize(pk.pos, pk.tri, (H, W), ranges=s.ranges)[0], rast)


def _dilate(amb):
    a = amb.clone()
    a[:, 1:] |= amb[:, :-1]
    a[:, :-1] |= amb[:, 1:]
    a[:, :, 1:] |= amb[:, :, :-1]
    a[:, :, :-1] |= amb[:, :, 1:]
    return a


def test_loss_backward_to_pos_and_attr(dev):
    """One loss over antialias(interpolate(attr, rast, tri), rast, pos, tri) of the five images; the octahedron is shown
    by two images (its gradient is their sum), one image is empty.  Bars of tests/test_gpu_raster.py:
    test_end_to_end_loss_backward_to_v_pos (output within 1e-4 on the certain pixels, gradient within 1e-4 relative)
    and the two backward-oracle tests (1e-4 relative)."""
    s = Scene(dev, five_images)
    # float64 restatement, image by image on the image's mesh; a mesh shown twice is the same leaf twice
    pos64 = [p.double().requires_grad_(True) for p in s.pos]
    attr64 = [a.double().requires_grad_(True) for a in s.attr]
    loss64, outs64, keeps = 0.0, [], []
    for b in range(5):
        _, t, _, i = s.piece(b)
        if i is None or t.shape[0] == 0:
            outs64.append(torch.zeros(H, W, 3, dtype=torch.float64))
            keeps.append(torch.ones(H, W, dtype=torch.bool))
            continue
        r64, amb = R.rasterize(pos64[i][None], t, H, W)
        keep = ~_dilate(_dilate(amb))[0]
        out = R.antialias(R.interpolate(attr64[i][None], r64, t), r64.detach(), pos64[i][None], t)[0]
        loss64 = loss64 + (out * (s.wts[b].double() * keep[..., None])).sum()
        outs64.append(out.detach())
        keeps.append(keep)
    loss64.backward()
    keep = torch.stack(keeps)
    assert (~keep).float().mean() < 0.02

    ctx = raster.RasterizerContext("cuda", dev)
    pos = [p.to(dev).requires_grad_(True) for p in s.pos]
    attr = [a.to(dev).requires_grad_(True) for a in s.attr]
    pk = raster.pack_ranges(pos, [t.to(dev) for t in s.tri])
    rast, _ = ctx.rasterize(pk.pos, pk.tri, (H, W), ranges=s.ranges)
    img, _ = ctx.interpolate(torch.cat(attr), rast, pk.tri)
    out = ctx.antialias(img, rast, pk.pos, pk.tri)
    (out * (s.wts * keep[..., None]).to(dev)).sum().backward()

    assert (out.detach().cpu().double() - torch.stack(outs64))[keep].abs().max() < 1e-4
    assert out[2].abs().max() == 0  # the empty image
    for i in range(3):
        assert pos[i].grad.shape == pos[i].shape and attr[i].grad.shape == attr[i].shape
        assert pos64[i].grad.norm() > 0 and attr64[i].grad.norm() > 0
        assert (pos[i].grad.cpu().double() - pos64[i].grad).norm() <= 1e-4 * pos64[i].grad.norm(), i
        assert (attr[i].grad.cpu().double() - attr64[i].grad).norm() <= 1e-4 * attr64[i].grad.norm(), i


def test_argument_errors(dev):
    pos = torch.zeros(6, 4, device=dev)
    tri = octahedron()[1].to(dev)
    launches = []
    real = raster._launch
    raster._launch = lambda *a, **k: launches.append(a[0])
    try:
        for bad in (torch.tensor([[0, 8], [4, 5]], dtype=torch.int32),   # first + count > T
                    torch.tensor([[-1, 2]], dtype=torch.int32),          # negative first
                    torch.tensor([[0, 8]], dtype=torch.int32).to(dev),   # on the GPU
                    torch.tensor([[0, 8]], dtype=torch.int64)):          # int64
            with pytest.raises(ValueError):
                raster.rasterize(pos, tri, (H, W), ranges=bad)
        with pytest.raises(ValueError, match=r"ranges\[1\]"):  # names the offending row
            raster.rasterize(pos, tri, (H, W), ranges=torch.tensor([[0, 8], [4, 5]], dtype=torch.int32))
        with pytest.raises(ValueError):  # ranges with a 3-D pos
            raster.rasterize(pos[None], tri, (H, W), ranges=torch.tensor([[0, 8]], dtype=torch.int32))
        with pytest.raises(ValueError):  # a 2-D pos without ranges
            raster.rasterize(pos, tri, (H, W))
    finally:
        raster._launch = real
    assert launches == []
