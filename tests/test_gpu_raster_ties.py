"""The HIP rasterizer's coverage at exact and near ties (csrc/tt_raster_cover.h: canonical edge order, double-float
residuals, the tie rule, the per-edge choice between the screen-space and the homogeneous form; the depth key of
tt_raster.hip), on the lattice scenes of tests/raster_lattice.py.  No pixel is masked out anywhere in this file.

  1  partition: every triangle rasterized alone (range mode, one triangle per image); the images' coverage must sum to
     exactly 1 on every pixel of the mesh, and an ordinary rasterize of the whole list must show that single owner
  2  exact scenes (every fp32 operation on the way to a decision is exact) against the float64 oracle on every pixel:
     ids, (u, v, z/w), antialias, and the gradients of both
  3  a shared edge between a triangle with every w > 0 and one with a vertex behind the camera
  4  depth ties go to the smaller id, in instance and range mode, and -0 ties with +0
  5  the UV atlas's overlap guard (tt_uv_overlap) counts the same meshes the same way
Tolerances are those of tests/test_gpu_raster.py: ids exact, (u, v, z/w) 1e-5, antialias 1e-4, gradients 1e-4
relative in norm."""
import functools
import os
import sys

import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, raster

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_lattice as L  # noqa: E402
import raster_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64

LATTICES = [(16, 16, 2, "one"), (16, 8, 2, "pow2"), (16, 16, 2, "rand"), (12, 20, 2, "rand"), (16, 16, 1, "rand"),
            (24, 24, 3, "rand")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _each(dev, pos, tri, H, W):
    """(T,H,W,4) on the CPU: triangle t alone in image t, one range-mode call"""
    ranges = torch.tensor([(t, 1) for t in range(tri.shape[0])], dtype=torch.int32)
    return raster.rasterize(pos.to(dev), tri.to(dev), (H, W), ranges=ranges).cpu()


def _whole(dev, pos, tri, H, W):
    return raster.rasterize(pos[None].to(dev), tri.to(dev), (H, W))[0].cpu()


def _check_single_owner(dev, pos, tri, H, W, each, count):
    """where exactly one triangle covers the pixel alone, the whole mesh shows that triangle, with the same bits"""
    whole = _whole(dev, pos, tri, H, W)
    owner = (each[..., 3] > 0).float().argmax(0)
    one = count == 1
    assert torch.equal(whole[..., 3][one], (owner + 1).float()[one])
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    assert torch.equal(whole[..., :3][one], each[owner, yy, xx, :3][one])
    assert torch.equal(whole[..., 3] > 0, count > 0)


@functools.lru_cache(maxsize=None)
def _exact_scene(name):
    """(pos, tri, H, W, oracle rast (H,W,4), oracle amb (H,W), oracle per-triangle coverage count (H,W)), computed once"""
    if name == "centre_grid":
        pos, tri, H, W = L.centre_grid(16, 2) + (16, 16)
    elif name == "fan":
        pos, tri, H, W = L.fan(16, 8) + (16, 16)
    elif name == "lattice_one":
        pos, tri, H, W = L.lattice_grid(16, 16, 2, "one", 0) + (16, 16)
    elif name == "lattice_pow2":
        pos, tri, H, W = L.lattice_grid(16, 8, 2, "pow2", 0) + (16, 8)
    elif name.startswith("square_"):
        pos, tri, H, W = L.square(16, name == "square_centres") + (16, 16)
    else:  # split_<N>_<flip>
        _, n, flip = name.split("_")
        pos, tri, H, W = L.split_quad(flip == "1") + (int(n), int(n))
    ref, amb = R.rasterize(pos[None].double(), tri, H, W)
    count = torch.zeros(H, W, dtype=torch.long)
    for t in range(tri.shape[0]):
        count += (R.rasterize(pos[None].double(), tri[t:t + 1], H, W)[0][0, ..., 3] > 0).long()
    return pos, tri, H, W, ref[0].detach(), amb[0], count


# ---------------------------------------------------------------------------------------------------------------
# 1  partition


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("case", LATTICES, ids=lambda c: "%dx%d_k%d_%s" % c)
def test_lattice_is_partitioned(dev, case, seed):
    H, W, k, mode = case
    pos, tri = L.lattice_grid(H, W, k, mode, seed)
    each = _each(dev, pos, tri, H, W)
    count = (each[..., 3] > 0).sum(0)
    print("pixels covered 0 times:", int((count == 0).sum()), " more than once:", int((count > 1).sum()))
    assert torch.equal(count, torch.ones(H, W, dtype=count.dtype))
    ids = each[..., 3]
    assert ((ids == 0) | (ids == torch.arange(1, tri.shape[0] + 1).float()[:, None, None])).all()  # global ids
    _check_single_owner(dev, pos, tri, H, W, each, count)


@pytest.mark.parametrize("name", ["centre_grid", "fan"])
def test_exact_mesh_is_partitioned_inside_and_on_its_outline(dev, name):
    pos, tri, H, W, _, _, want = _exact_scene(name)
    assert want.max() == 1 and want.sum() >= 100  # the oracle's own 0/1 mask of the mesh, outline included
    each = _each(dev, pos, tri, H, W)
    count = (each[..., 3] > 0).sum(0)
    print("pixels that differ from the outline mask:", int((count != want).sum()))
    assert torch.equal(count, want)
    _check_single_owner(dev, pos, tri, H, W, each, count)


# ---------------------------------------------------------------------------------------------------------------
# 2  exact scenes against the oracle, every pixel

EXACT = ["centre_grid", "fan", "lattice_one", "lattice_pow2", "split_8_0", "split_8_1", "split_16_0", "split_16_1"]


@pytest.mark.parametrize("name", EXACT)
def test_exact_scene_matches_oracle_on_every_pixel(dev, name):
    pos, tri, H, W, ref, amb, _ = _exact_scene(name)
    assert amb.any()  # the scene does have ties
    rast = _whole(dev, pos, tri, H, W).double()
    print("ids that differ:", int((rast[..., 3] != ref[..., 3]).sum()), " max |(u, v, z/w) - oracle|:",
          float((rast[..., :3] - ref[..., :3]).abs().max()))
    assert torch.equal(rast[..., 3], ref[..., 3])
    assert (rast[..., :3] - ref[..., :3]).abs().max() <= 1e-5


@pytest.mark.parametrize("name", ["centre_grid", "fan", "lattice_pow2"])
def test_exact_scene_rasterize_backward_matches_oracle(dev, name):
    pos, tri, H, W, _, _, _ = _exact_scene(name)
    wts = torch.randn(1, H, W, 2, generator=torch.Generator().manual_seed(3))  # not masked
    p = pos[None].to(dev).requires_grad_(True)
    rast = raster.rasterize(p, tri.to(dev), (H, W))
    (rast[..., :2] * wts.to(dev)).sum().backward()
    p64 = pos[None].double().requires_grad_(True)
    (R.rasterize(p64, tri, H, W)[0][..., :2] * wts.double()).sum().backward()
    err = (p.grad.cpu().double() - p64.grad).norm() / p64.grad.norm()
    print("relative gradient error:", float(err))
    assert p64.grad.norm() > 0
    assert err <= 1e-4
    assert p.grad[..., 2].abs().max() == 0


@pytest.mark.parametrize("name", ["square_centres", "square_corners", "fan"])
def test_exact_scene_antialias_matches_oracle(dev, name):
    pos, tri, H, W, ref, _, _ = _exact_scene(name)
    rast = raster.rasterize(pos[None].to(dev), tri.to(dev), (H, W)).detach()
    assert torch.equal(rast[0, ..., 3].cpu().double(), ref[..., 3])
    g = torch.Generator().manual_seed(11)
    color = torch.rand(1, H, W, 3, generator=g)
    wts = torch.randn(1, H, W, 3, generator=g)
    c = color.to(dev).requires_grad_(True)
    p = pos[None].to(dev).requires_grad_(True)
    out = raster.antialias(c, rast, p, tri.to(dev))
    (out * wts.to(dev)).sum().backward()
    c64 = color.double().requires_grad_(True)
    p64 = pos[None].double().requires_grad_(True)
    want = R.antialias(c64, rast.cpu().double(), p64, tri)
    (want * wts.double()).sum().backward()
    e_out = (out.detach().cpu().double() - want.detach()).abs().max()
    e_c = (c.grad.cpu().double() - c64.grad).norm() / c64.grad.norm()
    e_p = (p.grad.cpu().double() - p64.grad).norm() / p64.grad.norm()
    print("max |out - oracle|:", float(e_out), " relative gradient errors (color, pos):", float(e_c), float(e_p))
    # square_centres blends; the two outlines on pixel corners cross every pair at s = 0.5 exactly, where the blend
    # weight |0.5 - s| is 0 and only its derivative is not: the output is the input, the gradient to pos is not zero
    assert bool((want.detach() != color.double()).any()) == (name == "square_centres")
    assert p64.grad.norm() > 0 and c64.grad.norm() > 0
    assert e_out <= 1e-4
    assert e_c <= 1e-4
    assert e_p <= 1e-4


# ---------------------------------------------------------------------------------------------------------------
# 3  a shared edge between a screen-path and a homogeneous-path triangle


def mixed_edge_violations(dev, W, d, seeds=range(8)):
    """(on-edge pixels checked, those whose two coverages do not sum to 1): the seeds' pairs in one range-mode call"""
    scenes = [L.mixed_edge(W, d, seed) for seed in seeds]
    pk = raster.pack_ranges([s[0] for s in scenes], [s[1] for s in scenes])
    each = _each(dev, pk.pos, pk.tri, W, W)
    cov = (each[..., 3] > 0).long()
    checked = bad = 0
    for i, (_, _, pix) in enumerate(scenes):
        assert cov[2 * i].sum() > 10 and cov[2 * i + 1].sum() > 10  # both triangles are on screen
        s = (cov[2 * i] + cov[2 * i + 1])[pix[:, 1], pix[:, 0]]
        checked += len(pix)
        bad += int((s != 1).sum())
    return checked, bad


@pytest.mark.parametrize("d", [(1, 3), (3, 1), (1, 1), (3, 5)], ids=lambda d: "d%d_%d" % d)
@pytest.mark.parametrize("W", [32, 64])
def test_mixed_path_shared_edge_is_covered_once(dev, W, d):
    checked, bad = mixed_edge_violations(dev, W, d)
    print("on-edge pixels:", checked, " covered 0 or 2 times:", bad)
    assert checked >= 16
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------
# 4  depth ties


def _quad_of(tri, ids):
    """0 / 1: the quad (vertices 0..3 / 4..7) of the triangle shown by each covered pixel; -1 where empty"""
    q = (tri.long()[(ids.long() - 1).clamp(min=0), 0] >= 4).long()
    return torch.where(ids > 0, q, torch.full_like(q, -1))


def depth_tie_winners(dev, signed_zero):
    """per list order (first quad first / second quad first): the quad shown by every pixel, in instance mode and in
    range mode with both quads in one image; and the rasts"""
    N = 16
    pos, tri = L.coincident_quads(N, signed_zero)
    out = {}
    for order, t in (("ab", tri), ("ba", tri[[2, 3, 0, 1]].contiguous())):
        inst = _whole(dev, pos, t, N, N)
        assert torch.equal(inst, _whole(dev, pos, t, N, N))  # bit-identical launches
        ranges = torch.tensor([[2, 2], [0, 4], [0, 2]], dtype=torch.int32)
        rng = raster.rasterize(pos.to(dev), t.to(dev), (N, N), ranges=ranges).cpu()
        rev = raster.rasterize(pos.to(dev), t.to(dev), (N, N), ranges=ranges.flip(0).contiguous()).cpu()
        assert torch.equal(rng, rev.flip(0))  # the order of the ranges changes nothing
        assert torch.equal(rng[1], inst)       # both quads in one image: the instance-mode picture, global ids
        assert torch.equal(rng[0, ..., 3] > 0, inst[..., 3] > 0) and rng[0, ..., 3].max() == 4
        out[order] = (_quad_of(t, inst[..., 3]), inst)
    return out


@pytest.mark.parametrize("signed_zero", [False, True], ids=["z_quarter", "z_signed_zero"])
def test_depth_tie_goes_to_the_smaller_id(dev, signed_zero):
    got = depth_tie_winners(dev, signed_zero)
    for order, first in (("ab", 0), ("ba", 1)):
        q, inst = got[order]
        covered = q >= 0
        print(order, "covered:", int(covered.sum()), " pixels not won by the quad listed first:",
              int((q[covered] != first).sum()))
        assert covered.sum() == 12 * 12
        assert (q[covered] == first).all()          # the quad listed first holds the smaller ids
        assert inst[..., 3].max() == 2              # and it is its two triangles that show
        if signed_zero:
            assert (inst[..., 2] == 0).all() and not torch.signbit(inst[..., 2]).any()  # the stored depth is +0
    if signed_zero:  # the same winners as at z = 0.25, pixel by pixel
        ref = depth_tie_winners(dev, False)
        for order in ("ab", "ba"):
            assert torch.equal(got[order][1][..., 3], ref[order][1][..., 3])
            assert torch.equal(got[order][1][..., :2], ref[order][1][..., :2])


# ---------------------------------------------------------------------------------------------------------------
# 5  the overlap guard on the same meshes


def _overlap(dev, v_tex, t_tex, N):
    lib = tt._lib.load()
    Vt, T = v_tex.shape[0], t_tex.shape[0]
    v_tex, t_tex = v_tex.to(dev).contiguous(), t_tex.to(dev).contiguous()
    flags = torch.full((T,), 7, device=dev, dtype=torch.uint8)
    tot = torch.full((4,), -1, device=dev, dtype=torch.int32)
    ws = torch.empty(int(lib.tt_uv_workspace_bytes(Vt, T, N)), device=dev, dtype=torch.uint8)
    tt._lib.check(lib.tt_uv_overlap(ops._ptr(v_tex), ops._ptr(t_tex), Vt, Vt, T, N, ops._ptr(ws), ops._ptr(flags),
                                    ops._ptr(tot), ops._stream()), "overlap")
    return flags.cpu(), tot.cpu()


@pytest.mark.parametrize("name", ["lattice_one", "centre_grid"])
def test_overlap_guard_counts_like_the_rasterizer(dev, name):
    pos, tri, H, W, _, _, _ = _exact_scene(name)
    N = H
    assert H == W and (pos[:, 3] == 1).all()
    v_tex = (pos[:, :2] + 1) / 2  # exact: dyadic
    each = _each(dev, pos, tri, N, N)
    covered = int(((each[..., 3] > 0).sum(0) > 0).sum())
    flags, tot = _overlap(dev, v_tex, tri, N)
    print("flagged faces:", int(tot[0]), " covered texels:", int(tot[1]), " rasterizer:", covered)
    assert tot[0] == 0 and tot[1] == covered and covered == (256 if name == "lattice_one" else 144)
    assert (flags == 0).all()
    # one triangle again under a new face index: exactly the two coincident faces are flagged
    f = 5
    assert (each[f, ..., 3] > 0).any()
    flags, tot = _overlap(dev, v_tex, torch.cat([tri, tri[f:f + 1]]), N)
    want = torch.zeros(tri.shape[0] + 1, dtype=torch.uint8)
    want[f] = want[-1] = 1
    assert tot[0] == 2 and tot[1] == covered
    assert torch.equal(flags, want)
