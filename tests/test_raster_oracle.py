"""The float64 raster oracle (tests/raster_reference.py) against first principles, without a GPU: its gradients
against central finite differences, exact single coverage of a split quad, the perimeter property of the antialias,
and near-plane clipping against an independent per-pixel solve; and on the tie scenes of tests/raster_lattice.py, what
tests/test_gpu_raster_ties.py asks of the kernel: the oracle itself covers every pixel of the exact scenes once and
gives a depth tie to the smaller id."""
import pytest
import torch

import raster_lattice as L
import raster_reference as R

F64 = torch.float64


def _quad(x0, x1, y0, y1, z=0.0, w=1.0):
    """an axis-aligned NDC rectangle as two triangles sharing the diagonal (vertex 0 - vertex 2)"""
    pos = torch.tensor([[x0, y0, z, 1.0], [x1, y0, z, 1.0], [x1, y1, z, 1.0], [x0, y1, z, 1.0]], dtype=F64)
    pos[:, :3] *= w
    pos[:, 3] = w
    tri = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    return pos[None], tri


def _scene(seed=0, B=2, T=6, V=12):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(B, V, 4, generator=g, dtype=F64) * 1.6 - 0.8
    pos[..., 2] = pos[..., 2] * 0.5
    pos[..., 3] = 1.0 + 0.3 * torch.rand(B, V, generator=g, dtype=F64)
    pos[..., :3] *= pos[..., 3:4]
    tri = torch.stack([torch.randperm(V, generator=g)[:3] for _ in range(T)]).int()
    return pos, tri


def _fd(fn, x, eps=1e-6):
    g = torch.zeros_like(x)
    flat = x.view(-1)
    for i in range(flat.numel()):
        old = flat[i].item()
        flat[i] = old + eps
        fp = fn().item()
        flat[i] = old - eps
        fm = fn().item()
        flat[i] = old
        g.view(-1)[i] = (fp - fm) / (2 * eps)
    return g


def test_rasterize_uv_gradient_matches_finite_differences():
    pos, tri = _scene(1)
    H = W = 12
    rast, amb = R.rasterize(pos, tri, H, W)
    wts = torch.randn(rast.shape[:3] + (2,), dtype=F64, generator=torch.Generator().manual_seed(2))
    p = pos.clone().requires_grad_(True)
    (R.rasterize(p, tri, H, W)[0][..., :2] * wts).sum().backward()
    ids0 = rast[..., 3].clone()

    def f():
        r, _ = R.rasterize(pos, tri, H, W)
        assert torch.equal(r[..., 3], ids0)  # the step is too small to change visibility
        return (r[..., :2] * wts).sum()

    fd = _fd(f, pos)
    assert (ids0 > 0).sum() > 20
    assert torch.allclose(p.grad, fd, rtol=1e-5, atol=1e-6), (p.grad - fd).abs().max()
    assert p.grad[..., 2].abs().max() == 0  # u, v do not depend on clip z


def test_interpolate_gradients_match_finite_differences():
    pos, tri = _scene(3)
    rast, _ = R.rasterize(pos, tri, 10, 10)
    rast = rast.detach()
    g = torch.Generator().manual_seed(4)
    for A in (2, 1):
        attr = torch.randn(A, pos.shape[1], 3, generator=g, dtype=F64)
        wts = torch.randn(2, 10, 10, 3, generator=g, dtype=F64)
        a = attr.clone().requires_grad_(True)
        r = rast.clone().requires_grad_(True)
        (R.interpolate(a, r, tri) * wts).sum().backward()
        fd_a = _fd(lambda: (R.interpolate(attr, rast, tri) * wts).sum(), attr)
        fd_r = _fd(lambda: (R.interpolate(attr, rast, tri) * wts).sum(), rast)
        assert torch.allclose(a.grad, fd_a, atol=1e-7)
        assert torch.allclose(r.grad[..., :2], fd_r[..., :2], atol=1e-7)


def test_antialias_gradients_match_finite_differences():
    pos, tri = _scene(5, B=1, T=5)
    H = W = 14
    rast, _ = R.rasterize(pos, tri, H, W)
    rast = rast.detach()
    g = torch.Generator().manual_seed(6)
    color = torch.rand(1, H, W, 3, generator=g, dtype=F64)
    wts = torch.randn(1, H, W, 3, generator=g, dtype=F64)
    c = color.clone().requires_grad_(True)
    p = pos.clone().requires_grad_(True)
    out = R.antialias(c, rast, p, tri)
    assert (out - color).abs().sum() > 0  # some silhouette pixels were blended
    (out * wts).sum().backward()
    fd_c = _fd(lambda: (R.antialias(color, rast, pos, tri) * wts).sum(), color)
    fd_p = _fd(lambda: (R.antialias(color, rast, pos, tri) * wts).sum(), pos)
    assert torch.allclose(c.grad, fd_c, atol=1e-7)
    assert torch.allclose(p.grad, fd_p, rtol=1e-5, atol=1e-6), (p.grad - fd_p).abs().max()
    assert p.grad.abs().sum() > 0


def test_split_quad_is_covered_exactly_once():
    # the diagonal of [-1,1]^2 passes exactly through pixel centres of a square image: the tie rule decides them
    for H in (8, 9, 16):
        pos, tri = _quad(-1.0, 1.0, -1.0, 1.0)
        count = torch.zeros(H, H, dtype=torch.long)
        for t in range(2):
            r, _ = R.rasterize(pos, tri[t:t + 1], H, H)
            count += (r[0, ..., 3] > 0).long()
        assert count.min() == 1 and count.max() == 1
        r, _ = R.rasterize(pos, tri, H, H)
        assert (r[0, ..., 3] > 0).all()
        # and either triangle order / winding gives the same single coverage
        r2, _ = R.rasterize(pos, tri[:, [0, 2, 1]], H, H)
        assert (r2[0, ..., 3] > 0).all()


def test_antialiased_opacity_moves_with_the_perimeter():
    H = W = 48
    L = 20  # square side in pixels
    def ndc(px, N):  # pixel coordinate -> NDC (pixel centre px samples (2 px + 1) / N - 1)
        return (2 * px + 1) / N - 1

    def total(delta):
        x0, y0 = 10.3, 12.6
        pos, tri = _quad(ndc(x0, W), ndc(x0 + L + delta, W), ndc(y0, H), ndc(y0 + L, H), w=1.3)
        rast, _ = R.rasterize(pos, tri, H, W)
        mask = (rast[..., 3:] > 0).to(F64)
        return R.antialias(mask, rast, pos, tri).sum().item()

    base = total(0.0)
    assert abs(base - L * L) <= 1.0
    for delta in (0.2, 0.37, 0.81, 1.45):
        assert abs(total(delta) - base - L * delta) <= 1.0, (delta, total(delta) - base)


def test_near_plane_fragments_are_dropped():
    # one triangle whose z/w crosses -1 (the near plane) and another that straddles w = 0
    H = W = 24
    pos = torch.tensor([[[-0.8, -0.8, -1.5, 1.0], [0.9, -0.6, 0.5, 1.0], [0.0, 0.9, 0.2, 1.0],
                         [-0.5, 0.5, 0.0, 0.5], [0.5, 0.5, 0.0, -0.5], [0.0, -0.5, 0.0, 1.0]]], dtype=F64)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rast, _ = R.rasterize(pos, tri, H, W)
    X, Y = R.pixel_ndc(H, W)
    v = pos[0, :3][:, [0, 1, 3]]  # rows (x, y, w)
    n_in = n_cut = 0
    for py in range(H):
        for px in range(W):
            # independent solve for b (3) and s: sum_k b_k v_k = s (X, Y, 1), sum b = 1 (s = the interpolated w)
            M = torch.zeros(4, 4, dtype=F64)
            M[:3, :3] = v.T
            M[:3, 3] = -torch.tensor([X[px], Y[py], 1.0], dtype=F64)
            M[3, :3] = 1.0
            sol = torch.linalg.solve(M, torch.tensor([0, 0, 0, 1.0], dtype=F64))
            b, s = sol[:3], sol[3]
            inside = bool((b >= 0).all()) and s > 0
            zw = float((b * pos[0, :3, 2]).sum() / (b * pos[0, :3, 3]).sum()) if inside else 0.0
            want = inside and -1 <= zw <= 1
            got = rast[0, py, px, 3] > 0
            assert got == want, (px, py, zw)
            n_in += inside
            n_cut += inside and zw < -1
            if want:
                assert abs(rast[0, py, px, 2] - zw) < 1e-9
    assert n_in > 50 and n_cut > 5  # the scene does exercise the clip
    # the triangle with one vertex at w < 0: only the part with interpolated w > 0 is rasterized
    tri2 = torch.tensor([[3, 4, 5]], dtype=torch.int32)
    rast2, _ = R.rasterize(pos, tri2, H, W)
    v2 = pos[0, 3:6][:, [0, 1, 3]]
    for py in range(0, H, 3):
        for px in range(0, W, 3):
            M = torch.zeros(4, 4, dtype=F64)
            M[:3, :3] = v2.T
            M[:3, 3] = -torch.tensor([X[px], Y[py], 1.0], dtype=F64)
            M[3, :3] = 1.0
            sol = torch.linalg.solve(M, torch.tensor([0, 0, 0, 1.0], dtype=F64))
            b, s = sol[:3], sol[3]
            want = bool((b >= 0).all()) and s > 0  # s = the interpolated w: in front of the camera
            assert (rast2[0, py, px, 3] > 0) == want


def _count(pos, tri, H, W):
    """(H,W) how many triangles, each rasterized alone, cover the pixel; and the whole mesh's ids"""
    count = torch.zeros(H, W, dtype=torch.long)
    for t in range(tri.shape[0]):
        count += (R.rasterize(pos[None].double(), tri[t:t + 1], H, W)[0][0, ..., 3] > 0).long()
    whole, amb = R.rasterize(pos[None].double(), tri, H, W)
    return count, whole[0, ..., 3], amb[0]


@pytest.mark.parametrize("case", [(16, 16, 2, "one", 0), (16, 16, 2, "one", 1), (16, 8, 2, "pow2", 0),
                                  (16, 8, 2, "pow2", 1), (8, 8, 1, "pow2", 2), (16, 16, 4, "one", 3)])
def test_exact_lattice_is_partitioned_by_the_oracle(case):
    H, W = case[:2]
    pos, tri = L.lattice_grid(*case)
    assert tri.shape[0] == 2 * (H // case[2]) * (W // case[2]) and len(set(map(tuple, tri.sort(1).values.tolist()))) == tri.shape[0]
    count, ids, amb = _count(pos, tri, H, W)
    assert amb.any()  # the diagonals do run through pixel centres
    assert count.min() == 1 and count.max() == 1
    assert (ids > 0).all()


@pytest.mark.parametrize("name", ["centre_grid", "fan"])
def test_exact_mesh_is_partitioned_by_the_oracle_inside_and_on_its_outline(name):
    N = 16
    pos, tri = L.centre_grid(N, 2) if name == "centre_grid" else L.fan(N, 8)
    count, ids, amb = _count(pos, tri, N, N)
    assert amb.any()
    assert count.max() == 1 and torch.equal(count > 0, ids > 0)
    c = torch.arange(N) + 0.5  # pixel centres; both outlines are the square 2 .. 14 (centre_grid: 2.5 .. 14.5)
    lo, hi = (2.5, 14.5) if name == "centre_grid" else (2.0, 14.0)
    inside = ((c > lo) & (c < hi))[:, None] & ((c > lo) & (c < hi))[None, :]
    outside = ~(((c >= lo) & (c <= hi))[:, None] & ((c >= lo) & (c <= hi))[None, :])
    assert (count[inside] == 1).all() and (count[outside] == 0).all()
    if name == "centre_grid":  # on the outline: the tie rule gives the mesh its low-x and low-y sides, not the others
        assert (~inside & ~outside).any()
        assert count[2, 3] == 1 and count[3, 2] == 1 and count[14, 3] == 0 and count[3, 14] == 0


def test_rand_lattice_tiles_the_image_away_from_its_edges():
    # x = fl(X w) is inexact: the oracle is no reference on the diagonals' pixel centres (the partition property is
    # the kernel's whole assertion there); away from them the builder's mesh covers every pixel once
    pos, tri = L.lattice_grid(12, 20, 2, "rand", 0)
    w = pos[:, 3]
    assert ((w >= 0.5) & (w < 2)).all() and (torch.frexp(w)[0] * 2 ** 24 % 2 ** 12 != 0).any()  # non-dyadic
    count, ids, amb = _count(pos, tri, 12, 20)
    assert amb.any() and (~amb).sum() > 100
    assert (count[~amb] == 1).all()


@pytest.mark.parametrize("W,d", [(32, (1, 3)), (32, (3, 1)), (64, (1, 1)), (64, (3, 5))])
def test_mixed_edge_scene_is_what_it_says(W, d):
    for seed in range(8):
        pos, tri, pix = L.mixed_edge(W, d, seed)
        p = pos.double()
        n_front = [(p[t.long(), 3] > 0).sum().item() for t in tri]
        assert sorted(n_front) == [2, 3]  # one triangle in front, one with a vertex behind the camera
        shared = sorted(set(tri[0].tolist()) & set(tri[1].tolist()))
        assert len(shared) == 2 and (p[shared, 3] > 0).all()
        a, b = (p[i, :2] / p[i, 3:4] for i in shared)
        X, Y = R.pixel_ndc(W, W)
        c = torch.stack([X[pix[:, 0]], Y[pix[:, 1]]], -1)
        cross = (b - a)[0] * (c - a)[:, 1] - (b - a)[1] * (c - a)[:, 0]
        assert cross.abs().max() < 1e-6  # the returned pixel centres lie on the edge, up to the rounding of x = fl(X w)
        s = ((c - a) * (b - a)).sum(-1) / ((b - a) ** 2).sum()
        assert ((s > 0) & (s < 1)).all() and len(pix) >= 2
        count, _, amb = _count(pos, tri, W, W)
        assert amb[pix[:, 1], pix[:, 0]].all()  # the oracle is no reference there
        assert (count[~amb] <= 1).all()  # the visible parts lie on opposite sides of the edge
        for k in range(len(pix)):  # and meet along it: around an on-edge centre both triangles show
            y0, x0 = max(pix[k, 1] - 1, 0), max(pix[k, 0] - 1, 0)
            near = [(R.rasterize(pos[None].double(), tri[t:t + 1], W, W)[0][0, y0:y0 + 3, x0:x0 + 3, 3] > 0).any() for t in (0, 1)]
            assert all(near)
            if k == 1:
                break


@pytest.mark.parametrize("signed_zero", [False, True])
def test_oracle_gives_a_depth_tie_to_the_smaller_id(signed_zero):
    N = 16
    pos, tri = L.coincident_quads(N, signed_zero)
    if signed_zero:
        assert not torch.signbit(pos[:4, 2]).any() and torch.signbit(pos[4:, 2]).all() and (pos[:, 2] == 0).all()
    for t, first in ((tri, 0), (tri[[2, 3, 0, 1]], 4)):
        r, amb = R.rasterize(pos[None].double(), t, N, N)
        ids = r[0, ..., 3]
        assert (ids > 0).sum() == 12 * 12 and amb[0][ids > 0].all()  # every covered pixel is a depth tie
        assert ids.max() == 2  # the two triangles listed first
        assert (t.long()[ids[ids > 0].long() - 1, 0] // 4 * 4 == first).all()
        alone, _ = R.rasterize(pos[None].double(), t[2:], N, N)  # the quad listed second covers the same pixels
        assert torch.equal(alone[0, ..., 3] > 0, ids > 0)
