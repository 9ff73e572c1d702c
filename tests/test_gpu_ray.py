"""HIP ray casting (tt_ray_*; ops.mesh_ray_cast, mesh_ray_occluded, ray_mesh_depth, mesh_ambient_occlusion,
bake_ambient_occlusion; Mesh.ray_cast / occluded / ambient_occlusion; the exporter's map_Ka and the viewer's "ao" mode)
against the float64 Moeller-Trumbore reference and the fp32 restatements of tests/ray_reference.py.

Scale of a ray: s = (L + |o|_inf) / |d|, L the mesh's largest absolute coordinate.  The bar on t is 1e-6 s: the fp32 numpy
restatement of the pair shows 1.2e-7 (tetra), 1.7e-7 (cube), 1.5e-7 (lattice) and 2.4e-7 s (sphere24) against float64 on the
2 000 committed rays of each mesh.  The bar on the reconstructed hit point |sum b_k v_k - (o + t d)|_inf is four times
what that restatement shows on the test's own clean rays, in units of L + |o|_inf: it shows 6.8e-8 (tetra), 1.6e-7 (cube),
1.4e-7 (lattice) and 1.0e-7 (sphere24), so the bars are 2.7e-7 / 6.2e-7 / 5.5e-7 / 4.2e-7; the test computes them from the
restatement, never from the GPU's answer.  A ray is "unclean" when the float64 answer hangs on a margin below eta = 1e-4
(ray_reference.classify); the committed random sets hold 0, 1, 0 and 0 such rays of 2 000."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, export, ops, viewer
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_reference as R  # noqa: E402
from test_gpu_simplify import _exporter, _exporter_modules  # noqa: E402,F401  (the exporter test's small geometry)

pytestmark = pytest.mark.gpu
INF = float("inf")
GRIDS = (2, 3, 6, 7, 33, None)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_GRIDS = {}


def grid(name, dev, G=None):
    """The TriangleGrid of a mesh of ray_reference at grid G, built once."""
    if (name, G) not in _GRIDS:
        v, tri = R.mesh(name)
        _GRIDS[name, G] = ops.TriangleGrid(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev), grid=G)
    return _GRIDS[name, G]


def cast(o, d, tg, **kw):
    dev = tg.v_pos.device
    return ops.mesh_ray_cast(torch.from_numpy(np.ascontiguousarray(o)).to(dev),
                             torch.from_numpy(np.ascontiguousarray(d)).to(dev), tg, **kw)


def cast_np(o, d, tg, **kw):
    t, face, bary = cast(o, d, tg, **kw)
    return t.cpu().numpy(), face.cpu().numpy(), bary.cpu().numpy()


def same(x, y):
    return all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b) for a, b in zip(x, y))


def check_unclean(c, rows, t, face):
    """An unclean ray's answer is a valid hit or a near miss of the reference: a reported face is met by the ray within
    eta of its boundary at the reported t; a reported miss has no hit well inside a face and well inside [0, t_max]."""
    for i in rows:
        es = R.ETA * c["s"][i]
        if face[i] >= 0:
            assert c["B"][i, face[i]] >= -2 * R.ETA and abs(t[i] - c["T"][i, face[i]]) <= es, i
        else:
            with np.errstate(invalid="ignore"):
                assert not ((c["B"][i] > R.ETA) & (c["T"][i] > es)).any(), i


# ---- a. against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tetra", "cube", "lattice", "sphere24"])
def test_against_float64(name, dev):
    v, tri = R.mesh(name)
    o, d, c = R.case(name)
    tg = grid(name, dev)
    t, face, bary = cast_np(o, d, tg)
    clean = ~c["unclean"]
    assert c["unclean"].mean() <= 0.01
    assert np.array_equal(face[clean], c["face"][clean])
    m = clean & (face >= 0)
    err = np.abs(t[m].astype(np.float64) - c["t"][m]) / c["s"][m]
    rt, rf, rb = R.restated(name)
    point_bar = 4 * R.point_residual(o, d, v, tri, rt, rf, rb)[clean & (rf >= 0)].max()
    res = R.point_residual(o, d, v, tri, t, face, bary)[m]
    print(f"{name}: {m.sum()} clean hits, t error {err.max():.3g} s (bar 1e-6), hit point {res.max():.3g} "
          f"(bar {point_bar:.3g})")
    # the pair runs without contraction, every operation rounded on its own: the restatement's bits, unclean rays included
    assert np.array_equal(face, rf) and np.array_equal(t.view(np.uint32), rt.view(np.uint32))
    assert np.array_equal(bary.view(np.uint32), rb.view(np.uint32))
    assert (err <= R.T_BAR).all()
    assert (bary[m] >= 0).all() and (np.abs(bary[m].astype(np.float64).sum(1) - 1) <= 1e-6).all()
    assert (res <= point_bar).all()
    miss = face < 0
    assert np.isposinf(t[miss]).all() and (bary[miss] == 0).all() and (face[miss] == -1).all()
    check_unclean(c, np.nonzero(~clean)[0], t, face)

    # rows that cannot be served: a NaN row in the middle of a wave, an inf row and a zero direction at the end
    o2, d2 = np.concatenate([o, o[:2]]), np.concatenate([d, d[:2]])
    o2[1000, 1] = np.nan
    d2[-2, 0] = np.inf
    d2[-1] = 0
    t2, f2, b2 = cast_np(o2, d2, tg)
    bad = np.array([1000, len(o), len(o) + 1])
    assert np.isnan(t2[bad]).all() and (f2[bad] == -1).all() and (b2[bad] == 0).all()
    keep = np.setdiff1d(np.arange(len(o)), bad)
    assert np.array_equal(t2[keep].view(np.uint32), t[keep].view(np.uint32))
    assert np.array_equal(f2[keep], face[keep]) and np.array_equal(b2[keep].view(np.uint32), bary[keep].view(np.uint32))
    occ = ops.mesh_ray_occluded(torch.from_numpy(o2).to(dev), torch.from_numpy(d2).to(dev), tg).cpu().numpy()
    assert not occ[bad].any() and np.array_equal(occ[keep], face[keep] >= 0)


@pytest.mark.parametrize("name", ["tetra", "cube", "lattice"])
def test_t_max(name, dev):
    """One t_max per call, in the middle of the hits: a ray whose nearest hit is beyond it misses (or reports a farther
    face never); the answer is the reference's with that t_max."""
    v, tri = R.mesh(name)
    o, d, c0 = R.case(name)
    tm = float(np.float32(np.median(c0["t"][c0["face"] >= 0])))
    c = R.classify(o, d, v, tri, t_max=tm)
    t, face, _ = cast_np(o, d, grid(name, dev), t_max=tm)
    clean = ~c["unclean"]
    assert c["unclean"].mean() <= 0.01
    beyond = clean & (c0["face"] >= 0) & (c0["t"] > tm)
    assert beyond.sum() > 50 and (face[beyond] == -1).all() and np.isposinf(t[beyond]).all()
    assert np.array_equal(face[clean], c["face"][clean])
    assert (t[face >= 0] <= np.float32(tm)).all()
    occ = ops.mesh_ray_occluded(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev), grid(name, dev), t_max=tm)
    assert np.array_equal(occ.cpu().numpy(), face >= 0)


@pytest.mark.parametrize("name", ["tetra", "cube", "lattice", "sphere24"])
def test_two_sided(name, dev):
    """The same ray reversed, from a point behind the hit face and in front of the next one, reports the same face."""
    v, tri = R.mesh(name)
    o, d, c = R.case(name)
    rows = np.nonzero(~c["unclean"] & (c["face"] >= 0))[0][:300]
    with np.errstate(invalid="ignore"):
        later = np.where((c["B"][rows] >= 0) & (c["T"][rows] > c["t"][rows, None]), c["T"][rows], np.inf).min(1)
    tm = np.minimum(0.5 * (c["t"][rows] + later), c["t"][rows] + 0.25 * c["s"][rows])
    o2 = (o[rows].astype(np.float64) + tm[:, None] * d[rows].astype(np.float64)).astype(np.float32)
    d2 = -d[rows]
    c2 = R.classify(o2, d2, v, tri)
    t2, f2, _ = cast_np(o2, d2, grid(name, dev))
    ok = ~c2["unclean"]
    assert ok.sum() > 0.9 * len(rows)
    assert np.array_equal(f2[ok], c["face"][rows][ok])


# ---- b. independence, bit for bit ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "sphere24"])
def test_independent_of_grid_order_and_launch(name, dev):
    o1, d1 = R.random_rays(500, 21)
    o2, d2 = R.special_rays(name)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    base = ops.mesh_ray_cast(to, td, grid(name, dev, 1))
    assert int((base[1] >= 0).sum()) > len(o) // 2 and int((base[1] < 0).sum()) > 50
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(o))).to(dev)
    for G in GRIDS:
        tg = grid(name, dev, G)
        for cell_order in (False, True):
            assert same(ops.mesh_ray_cast(to, td, tg, cell_order=cell_order), base), (name, G, cell_order)
        got = ops.mesh_ray_cast(to[perm].contiguous(), td[perm].contiguous(), tg)
        assert same(got, [x[perm] for x in base]), (name, G)
        assert torch.equal(ops.mesh_ray_occluded(to, td, tg), base[1] >= 0), (name, G)
    for _ in range(3):
        assert same(ops.mesh_ray_cast(to, td, grid(name, dev)), base)
    # the kernel's pair is the restatement's, operation by operation: the face it reports is the restatement's
    hit, t, _ = R.pair_f32(o, d, *R.mesh(name))
    bt, bf = R.brute_f32(hit, t)
    assert np.array_equal(base[1].cpu().numpy(), bf) and np.array_equal(base[0].cpu().numpy().view(np.uint32),
                                                                           bt.view(np.uint32))
    m = Mesh(grid(name, dev).v_pos, grid(name, dev).t_pos_idx)
    assert same(m.ray_cast(to, td), base) and torch.equal(m.occluded(to, td), base[1] >= 0)


# ---- c. watertight ----------------------------------------------------------------------------------------------
def test_watertight_sphere(dev):
    """From an origin inside sphere24 one ray at every vertex and one at every edge midpoint, targets in fp32: every ray
    hits, at the reference's nearest t (barycentrics >= -1e-6 there) within the bar."""
    v, tri = R.mesh("sphere24")
    o, d = R.aimed_rays(v, tri, np.array([[0.05, -0.03, 0.02]], np.float32))
    assert len(o) == len(v) + len(R.edges(tri))
    t, face, bary = cast_np(o, d, grid("sphere24", dev))
    assert int((face >= 0).sum()) == len(o)
    T, B = R.moller_trumbore(o, d, v, tri)
    with np.errstate(invalid="ignore"):
        ref = np.where((B >= -1e-6) & (T >= 0), T, np.inf).min(1)
    err = np.abs(t.astype(np.float64) - ref) / R.scale(o, d, v)
    print(f"watertight: {len(o)} rays, t error {err.max():.3g} s")
    assert (err <= R.T_BAR).all()
    for G in (1, 7, 33):
        assert same(cast(o, d, grid("sphere24", dev, G)), cast(o, d, grid("sphere24", dev)))


def test_watertight_quad_edge(dev):
    v, tri = R.mesh("quad")
    s = np.linspace(-1, 1, 257).astype(np.float32)[1:-1]
    target = np.stack([s, s, np.zeros_like(s)], 1)  # points of the shared edge, vertex 0 to vertex 2
    origins = np.array([[0.3, -0.2, 1.0], [-0.7, 0.9, -2.0], [0.0, 0.0, 0.5], [5.0, 4.0, 3.0]], np.float32)
    o = np.repeat(origins, len(s), 0)
    d = (np.tile(target, (len(origins), 1)) - o).astype(np.float32)
    o = np.concatenate([o, target + np.array([0, 0, 1], np.float32)])  # and straight down onto the edge
    d = np.concatenate([d, np.tile(np.array([[0, 0, -2]], np.float32), (len(s), 1))])
    for G in (None, 1, 5):
        t, face, bary = cast_np(o, d, grid("quad", dev, G))
        assert ((face == 0) | (face == 1)).all()
        assert np.isfinite(t).all() and (bary >= 0).all()
    assert np.array_equal(t[-len(s):], np.full(len(s), 0.5, np.float32))


# ---- d. degenerate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["degenerate", "point"])
def test_faces_without_area_never_hit(name, dev):
    v, tri = R.mesh(name)
    o1, d1 = R.random_rays(500, 5)
    o2, d2 = R.aimed_rays(v, tri, R.SIXTH_ORIGINS)
    o3 = np.array([[0.5, 0, -1], [1.5, 0, 2], [0.25, 0.25, -0.75], [0.25, 0.25, 0.25]], np.float32)
    d3 = np.array([[0, 0, 1], [0, 0, -1], [0, 0, 1], [1, 0, 0]], np.float32)
    o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3])
    for G in (None, 1, 4):
        t, face, bary = cast_np(o, d, grid(name, dev, G))
        assert (face == -1).all() and np.isposinf(t).all() and (bary == 0).all()
        assert not ops.mesh_ray_occluded(torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev),
                                         grid(name, dev, G)).any()
    p = torch.from_numpy(o[:64]).to(dev)
    ao = ops.mesh_ambient_occlusion(p, torch.from_numpy(d[:64]).to(dev), grid(name, dev), max_distance=INF, bias=0.0)
    assert torch.equal(ao, torch.ones_like(ao))


def test_bad_arguments(dev):
    tg = grid("tetra", dev)
    o = torch.zeros(4, 3, device=dev)
    d = torch.ones(4, 3, device=dev)
    for kw in ({"t_max": -1.0}, {"t_max": float("nan")}, {"t_max": "far"}):
        with pytest.raises(ValueError):
            ops.mesh_ray_cast(o, d, tg, **kw)
        with pytest.raises(ValueError):
            ops.mesh_ray_occluded(o, d, tg, **kw)
    with pytest.raises(ValueError):
        ops.mesh_ray_cast(o, d[:3], tg)
    with pytest.raises(ValueError):
        ops.mesh_ray_cast(o[:, :2], d[:, :2], tg)
    with pytest.raises(TypeError):
        ops.mesh_ray_cast(o.double(), d, tg)
    with pytest.raises(TypeError):
        ops.mesh_ray_cast(o, d, (tg.v_pos, tg.t_pos_idx))
    with pytest.raises(RuntimeError):
        ops.mesh_ray_cast(o.cpu(), d, tg)
    for K in (0, 1025):
        with pytest.raises(ValueError):
            ops.mesh_ambient_occlusion(o, d, tg, n_rays=K)
    with pytest.raises(ValueError):
        ops.mesh_ambient_occlusion(o, d, tg, max_distance=-1.0)
    with pytest.raises(ValueError):
        ops.mesh_ambient_occlusion(o, d, tg, bias=float("inf"))
    with pytest.raises(ValueError):
        Mesh(tg.v_pos, tg.t_pos_idx).ambient_occlusion(points=o)
    # the C entry points themselves: TT_ERR_BAD_ARG before any launch
    out = (torch.empty(4, device=dev), torch.empty(4, device=dev, dtype=torch.int32), torch.empty(4, 3, device=dev))
    g = (tg.records, tg.cell_ptr, tg.cell_tri, tg.n_faces, tg.M, tg.G, *tg.lo, tg.ext, tg.h, tg.inv_h)
    bad_grids = [g[:3] + (0,) + g[4:], g[:4] + (0,) + g[5:], g[:5] + (0,) + g[6:], g[:5] + (257,) + g[6:],
                 g[:9] + (-1.0,) + g[10:], g[:6] + (float("nan"),) + g[7:]]
    for bg in bad_grids:
        with pytest.raises(RuntimeError, match="tt_ray_cast failed"):
            ops._launch("tt_ray_cast", o, d, None, 4, INF, *bg, *out)
    for n, tm in ((-1, INF), (4, -1.0), (4, float("nan"))):
        with pytest.raises(RuntimeError, match="tt_ray_cast failed"):
            ops._launch("tt_ray_cast", o, d, None, n, tm, *g, *out)
    with pytest.raises(RuntimeError, match="tt_ray_cast failed"):
        ops._launch("tt_ray_cast", o, None, None, 4, INF, *g, *out)
    hit = torch.empty(4, device=dev, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="tt_ray_any failed"):
        ops._launch("tt_ray_any", o, d, None, 4, INF, *g, None)
    hits = torch.empty(4, device=dev, dtype=torch.int32)
    table = ops.ao_directions(4).to(dev)
    for K, bias, md in ((0, 0.0, 1.0), (1025, 0.0, 1.0), (4, float("nan"), 1.0), (4, 0.0, -1.0)):
        with pytest.raises(RuntimeError, match="tt_ray_ao failed"):
            ops._launch("tt_ray_ao", o, d, table, 4, K, bias, md, *g, hits)
    ops._launch("tt_ray_cast", None, None, None, 0, INF, *g, None, None, None)  # N = 0 does nothing
    ops._launch("tt_ray_any", None, None, None, 0, INF, *g, None)
    ops._launch("tt_ray_ao", None, None, None, 0, 4, 0.0, 1.0, *g, None)
    e = torch.zeros(0, 3, device=dev)
    assert ops.mesh_ray_cast(e, e, tg)[0].numel() == 0 and ops.mesh_ray_occluded(e, e, tg).numel() == 0


# ---- e. seams -----------------------------------------------------------------------------------------------------
def test_launch_sizes(dev):
    o, d, _ = R.case("lattice")
    tg = grid("lattice", dev)
    full = cast(o, d, tg)
    for N in (1, 63, 64, 65, 257, 1025):
        assert same(cast(o[:N], d[:N], tg), [x[:N] for x in full]), N
        assert same(cast(o[-N:], d[-N:], tg, cell_order=True), [x[-N:] for x in full]), N


# ---- f. gradient --------------------------------------------------------------------------------------------------
def _plane_grads(o, d, v, idx, w, dtype):
    """Gradients of sum_i w_i t'_i, t' = n.(a - o) / n.d, n = (b - a) x (c - a), on the CPU in `dtype`."""
    o, d, v = (torch.tensor(x, dtype=dtype, requires_grad=True) for x in (o, d, v))
    a, b, c = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    n = torch.linalg.cross(b - a, c - a)
    t = (n * (a - o)).sum(-1) / (n * d).sum(-1)
    (t * torch.tensor(w, dtype=dtype)).sum().backward()
    return t.detach().numpy(), [x.grad.numpy().astype(np.float64) for x in (o, d, v)]


@pytest.mark.parametrize("name", ["tetra", "sphere24"])
def test_depth_gradient(name, dev):
    """ops.ray_mesh_depth: the value is the kernel's t; the gradients w.r.t. origins, dirs and v_pos are those of the
    plane formula with the face fixed, taken by float64 autograd on the CPU.  Tolerance: the same formula evaluated by
    CPU autograd in float32 deviates from the float64 one by some e per tensor (rounding of the formula itself, the
    conditioning of grazing rays included); the GPU runs that formula in float32 with another order of the scatter sums
    into v_pos, so the bar is 8 e + 1e-6 max |g|.  Rows that miss, and rows that cannot be served, have zero gradient."""
    v, tri = R.mesh(name)
    o, d, c = R.case(name)
    o, d = o[:600].copy(), d[:600].copy()
    d[7] = 0  # a row that cannot be served
    tg = grid(name, dev)
    to = torch.from_numpy(o).to(dev).requires_grad_()
    td = torch.from_numpy(d).to(dev).requires_grad_()
    tv = torch.from_numpy(v).to(dev).requires_grad_()
    t = ops.ray_mesh_depth(to, td, tv, torch.from_numpy(tri).to(dev), tg=tg)
    t0, face, _ = ops.mesh_ray_cast(to, td, tg)
    assert same([t.detach()], [t0])
    face = face.cpu().numpy()
    hit = (face >= 0) & ~c["unclean"][:600]
    hit[7] = False
    assert hit.sum() > 80 and (face < 0).sum() > 80
    w = np.random.default_rng(5).uniform(0.5, 1.5, 600).astype(np.float32)
    t.backward(torch.from_numpy(w).to(dev))  # every row takes part: the rows that miss must add nothing
    got = [x.grad.cpu().numpy().astype(np.float64) for x in (to, td, tv)]
    assert all(np.isfinite(g).all() for g in got)
    rows = np.nonzero(face >= 0)[0]
    idx = torch.from_numpy(tri[face[rows]].astype(np.int64))
    t64, ref = _plane_grads(o[rows], d[rows], v, idx, w[rows], torch.float64)
    _, f32 = _plane_grads(o[rows], d[rows], v, idx, w[rows], torch.float32)
    assert (np.abs(t64 - t.detach().cpu().numpy()[rows]) <= R.T_BAR * c["s"][rows])[hit[rows]].all()
    full = [np.zeros_like(got[0]), np.zeros_like(got[1]), ref[2]]
    full[0][rows], full[1][rows] = ref[0], ref[1]
    e32 = [np.zeros_like(got[0]), np.zeros_like(got[1]), f32[2]]
    e32[0][rows], e32[1][rows] = f32[0], f32[1]
    for k, what in enumerate(("origins", "dirs", "v_pos")):
        e = np.abs(e32[k] - full[k]).max()
        bar = 8 * e + 1e-6 * np.abs(full[k]).max()
        err = np.abs(got[k] - full[k]).max()
        print(f"{name} d/d{what}: error {err:.3g}, float32 restatement {e:.3g}, bar {bar:.3g}, max |g| "
              f"{np.abs(full[k]).max():.3g}")
        assert err <= bar, what
    miss = face < 0
    assert (got[0][miss] == 0).all() and (got[1][miss] == 0).all()
    assert np.isnan(t.detach().cpu().numpy()[7]) and np.isposinf(t.detach().cpu().numpy()[miss & (np.arange(600) != 7)]).all()


# ---- g. ambient occlusion -----------------------------------------------------------------------------------------
def test_ao_exact_cases(dev):
    fv, ft = R.quad(size=4.0, z=0.0)
    floor = ops.TriangleGrid(torch.from_numpy(fv).to(dev), torch.from_numpy(ft).to(dev))
    p = torch.tensor(np.random.default_rng(1).uniform(-3, 3, (200, 3)) * [1, 1, 0], dtype=torch.float32, device=dev)
    up = torch.tensor([[0.0, 0.0, 2.5]], device=dev).expand(200, 3).contiguous()
    ao = ops.mesh_ambient_occlusion(p, up, floor, n_rays=64)
    assert torch.equal(ao, torch.ones_like(ao))  # nothing above a lone floor
    tg = grid("cube", dev)
    c = torch.zeros(6, 3, device=dev)
    n = torch.tensor([[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -1, 0], [0, 0, 1e-3], [0.3, -0.4, -5]], device=dev)
    ao = ops.mesh_ambient_occlusion(c, n, tg, n_rays=64, max_distance=2.0, bias=0.0)
    assert torch.equal(ao, torch.zeros_like(ao))  # closed in: every ray from the centre hits the cube
    bad_p = torch.tensor([[float("nan"), 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, float("inf")]], device=dev)
    bad_n = torch.tensor([[0, 0, 1], [0, 0, 0], [0, float("nan"), 1], [0, 0, 1.0]], device=dev)
    assert torch.isnan(ops.mesh_ambient_occlusion(bad_p, bad_n, tg)).all()
    assert (ops.mesh_ao_hits(bad_p, bad_n, tg) == -1).all()
    assert ops.mesh_ambient_occlusion(c[:0], n[:0], tg).numel() == 0


@functools.lru_cache(maxsize=None)
def ao_case(name):
    """300 surface points (every other normal turned inward, so that the closed sphere is not all open), the defaults of
    ops.mesh_ambient_occlusion, the float64 reference."""
    v, tri = R.mesh(name)
    p, n = R.surface_points(v, tri, 300, 3)
    n[1::2] *= -1
    diag = float(np.linalg.norm(v.max(0).astype(np.float64) - v.min(0)))
    hits, unclean = R.ao_reference(p, n, R.ao_directions(64), 1e-3 * diag, 0.25 * diag, v, tri)
    return p, n, diag, hits, unclean


@pytest.mark.parametrize("name", ["sphere24", "lattice"])
def test_ao_against_float64(name, dev):
    p, n, diag, ref, unclean = ao_case(name)
    assert unclean.sum() <= 0.02 * 300 * 64
    assert 0.05 < ref.mean() / 64 < 0.95
    tp, tn = torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev)
    base = ops.mesh_ao_hits(tp, tn, grid(name, dev, 1))
    got = base.cpu().numpy()
    print(f"{name}: mean ao {1 - got.mean() / 64:.4f}, reference {1 - ref.mean() / 64:.4f}, "
          f"{(got != ref).sum()} of 300 points differ, {unclean.sum()} unclean rays")
    assert (np.abs(got - ref) <= unclean).all()
    ao = ops.mesh_ambient_occlusion(tp, tn, grid(name, dev))
    assert torch.equal(ao, 1.0 - base.float() / 64.0)
    # independent of the grid and of the order of the points, repeatable, bit for bit
    perm = torch.from_numpy(np.random.default_rng(2).permutation(300)).to(dev)
    for G in GRIDS:
        tg = grid(name, dev, G)
        assert torch.equal(ops.mesh_ao_hits(tp, tn, tg), base), G
        assert torch.equal(ops.mesh_ao_hits(tp[perm].contiguous(), tn[perm].contiguous(), tg), base[perm]), G
    assert torch.equal(ops.mesh_ao_hits(tp, tn, grid(name, dev)), base)
    m = Mesh(grid(name, dev).v_pos, grid(name, dev).t_pos_idx)
    assert torch.equal(m.ambient_occlusion(tp, tn), ao)
    per_vertex = m.ambient_occlusion()
    assert per_vertex.shape == (m.v_pos.shape[0],) and bool(((per_vertex >= 0) & (per_vertex <= 1)).all())


@pytest.mark.parametrize("K", [1, 63, 64, 65])
def test_ao_counts_the_occluded_rays(K, dev):
    """hits[i] = the number of the point's K rays, built on the host in fp32 as the kernel builds them, that
    mesh_ray_occluded calls hit; rays the float64 reference calls unclean excepted."""
    v, tri = R.mesh("lattice")
    p, n = ao_case("lattice")[:2]
    p, n = p[:100], n[:100]
    bias, md = 0.004, 0.6
    table = R.ao_directions(K)
    o, d = R.ao_rays_f32(p, n, table, bias)
    tg = grid("lattice", dev)
    occ = ops.mesh_ray_occluded(torch.from_numpy(o.reshape(-1, 3).copy()).to(dev),
                                torch.from_numpy(d.reshape(-1, 3).copy()).to(dev), tg, t_max=md)
    per_ray = occ.reshape(100, K).sum(1).cpu().numpy()
    hits = ops.mesh_ao_hits(torch.from_numpy(p).to(dev), torch.from_numpy(n).to(dev), tg, n_rays=K, max_distance=md,
                            bias=bias).cpu().numpy()
    _, unclean = R.ao_reference(p, n, table, bias, md, v, tri)
    print(f"K={K}: {(hits != per_ray).sum()} of 100 points differ from the per-ray count")
    assert (np.abs(hits - per_ray) <= unclean).all()
    assert hits.min() >= 0 and hits.max() <= K


# ---- h. export ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modules(dev):
    return _exporter_modules(dev)


def test_exporter_ambient_occlusion(modules, tmp_path):
    r, g, m, b, cache = modules
    N = 256
    cfg = {"save_uv": True, "texture_size": N, "texture_format": "png"}
    exp = _exporter(modules, cfg)
    assert exp.bake_ambient_occlusion is False and exp.ao_rays == 64 and exp.ao_distance is None
    exp.simplify_grid = 24
    (before,) = exp(cache)
    exp.bake_ambient_occlusion = False
    (unset,) = exp(cache)
    assert set(unset.params) == set(before.params) and "map_Ka" not in unset.params
    for k, x in before.params.items():
        if torch.is_tensor(x):
            assert torch.equal(x, unset.params[k]), k
    exp.bake_ambient_occlusion = True
    exp.ao_rays = 32
    (out,) = exp(cache)
    assert set(out.params) == set(before.params) | {"map_Ka"}
    for k, x in before.params.items():
        if torch.is_tensor(x):
            assert torch.equal(x, out.params[k]), k
    ka, mesh = out.params["map_Ka"], out.params["mesh"]
    assert tuple(ka.shape) == (N, N, 1) and ka.dtype == torch.float32
    assert bool(((ka >= 0) & (ka <= 1)).all())
    ref, info = ops.bake_ambient_occlusion(mesh, N, n_rays=32)
    texel = info["texel"]
    assert info["n_covered"] == texel.numel() > N * N // 4
    assert torch.equal(ka.reshape(-1)[texel], ref.reshape(-1)[texel])
    assert torch.equal(ref.reshape(-1)[texel], 1.0 - info["hits"].float() / 32.0)
    assert abs(info["mean"] - float(ref.reshape(-1)[texel].mean())) < 1e-6
    assert torch.equal(exp.ao_info["hits"], info["hits"])
    assert 0.2 < info["mean"] < 1.0 and int((info["hits"] > 0).sum()) > 0  # a blobby shape: some of it is occluded
    hole = torch.ones(N * N, dtype=torch.bool, device=ka.device)
    hole[texel] = False
    assert torch.equal(ref.reshape(-1)[hole], torch.ones_like(ref.reshape(-1)[hole]))

    files = export.save_obj(str(tmp_path / out.save_name), **out.params)
    assert str(tmp_path / "texture_ao.png") in files
    assert "map_Ka texture_ao.png\n" in open(tmp_path / "model.mtl").read()
    back = viewer.load_ao_map(str(tmp_path / "model.obj"), device=ka.device)
    assert tuple(back.shape) == (N, N, 1) and float((back - ka).abs().max()) <= 1.0 / 255.0
    loaded, kd = viewer.load_obj(str(tmp_path / "model.obj"), device=ka.device)
    with torch.no_grad():
        plain = viewer.turntable(loaded, kd, n_views=2, height=96, width=96)
        shaded = viewer.turntable(loaded, kd, n_views=2, height=96, width=96, map_Ka=back)
        alone = viewer.turntable(loaded, kd, n_views=2, height=96, width=96, mode="ao", map_Ka=back)
    assert plain.shape == shaded.shape == alone.shape == (2, 96, 96, 3)
    assert bool((shaded <= plain + 1e-6).all()) and float((plain - shaded).abs().max()) > 0.02
    assert torch.equal(alone[..., 0], alone[..., 1]) and float((alone - plain).abs().max()) > 0.02
    with pytest.raises(ValueError):
        viewer.turntable(loaded, kd, n_views=1, height=32, width=32, mode="ao")
    assert viewer.load_ao_map(str(tmp_path / "model.obj")) is not None
    os.makedirs(tmp_path / "plain")
    export.save_obj(str(tmp_path / "plain" / "model.obj"), **before.params)
    assert viewer.load_ao_map(str(tmp_path / "plain" / "model.obj")) is None
    assert not os.path.exists(tmp_path / "plain" / "texture_ao.png")
