"""HIP point-to-mesh distance (tt_dist_*; ops.TriangleGrid, mesh_closest_point, point_mesh_distance2,
mesh_surface_samples; Mesh.closest_point / distance_to / simplify(max_error=); the exporter's simplify_max_error)
against the float64 restatement tests/distance_reference.py.

The bar of every distance comparison is 4e-6 * max(L_mesh, |p|_inf), L_mesh the mesh's largest absolute coordinate: an
fp32 numpy restatement of the Voronoi formulation measured 1.05e-6 against float64 on 2 700 points x 1 024 jittered
sphere triangles with coordinates <= 1, the GPU differs from that by FMA contraction only, the bar is about 4x that.
The deviations the GPU shows are printed by each test and recorded in profiles/mesh_distance.json: at most 0.046 of the
bar on an MI355X (torus32), a reported face at most 4.7e-8 farther than the float64 nearest."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import ops
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import simplify_reference as S  # noqa: E402
from test_gpu_simplify import _exporter, _exporter_modules  # noqa: E402,F401  (the exporter test's small geometry)

pytestmark = pytest.mark.gpu
REL = 4e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def mesh_np(name):
    hand_built = {"two_clusters": D.two_clusters, "spanning": D.spanning, "one_octant": D.one_octant}
    v, t = hand_built[name]() if name in hand_built else S.source_mesh(name)
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(t, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def case(name):
    """(points float32, float64 distance, float64 pair matrix) of a mesh, computed once; at most about 4 M pairs."""
    v, t = mesh_np(name)
    pts = D.query_points(v, t)
    if len(pts) * len(t) > 5_000_000:  # torus32: fewer uniform points, the on-surface ones kept
        pts = np.concatenate([pts[:100], pts[1500:]])
    M = D.pair_matrix(pts, v, t)
    return pts, M.min(1)[0].sqrt().numpy(), M.numpy()


def gpu(name, dev):
    v, t = mesh_np(name)
    return torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)


def bar(pts, v):
    return REL * np.maximum(np.abs(v).max(), np.abs(pts.astype(np.float64)).max(1))


def check_rows(pts, v, t, d_ref, M, d2, face, bary, what):
    """The contract of test (a) on finite rows; returns the largest error in units of the bar."""
    d2, face, bary = d2.cpu().numpy().astype(np.float64), face.cpu().numpy(), bary.cpu().numpy().astype(np.float64)
    b = bar(pts, v)
    assert np.isfinite(d2).all() and (d2 >= 0).all()
    err = np.abs(np.sqrt(d2) - d_ref)
    assert (face >= 0).all() and (face < len(t)).all()
    d_face = np.sqrt(M[np.arange(len(pts)), face]) if M is not None else D.distance_to_faces(pts, v, t, face)
    excess = d_face - d_ref
    closest = (bary[:, :, None] * v.astype(np.float64)[t[face]]).sum(1)
    d_bary = np.linalg.norm(pts.astype(np.float64) - closest, axis=1)
    print(f"{what}: N {len(pts)} T {len(t)}  max |d - ref| = {err.max():.3e} ({(err / b).max():.3f} of the bar), "
          f"face excess {excess.max():.3e}, |bary sum - 1| {np.abs(bary.sum(1) - 1).max():.2e}, "
          f"| |p - c(bary)| - d | {np.abs(d_bary - np.sqrt(d2)).max():.3e}, faces != float64 argmin "
          f"{(face != (M.argmin(1) if M is not None else face)).mean():.3f}")
    assert (err <= b).all(), f"worst {(err / b).max():.2f} of the bar at point {pts[(err / b).argmax()]}"
    assert (excess <= b).all()
    assert (bary >= 0).all() and (np.abs(bary.sum(1) - 1) <= 1e-6).all()
    assert (np.abs(d_bary - np.sqrt(d2)) <= b).all()
    return (err / b).max()


# ---- a. against float64 brute force ----
@pytest.mark.parametrize("name", ["sphere24", "torus32", "hand", "triangle", "two_clusters", "spanning"])
def test_matches_float64_brute_force(dev, name):
    v, t = mesh_np(name)
    pts, d_ref, M = case(name)
    bad = np.array([[0.1, np.nan, 0.2], [np.inf, 0.0, 0.0], [0.3, 0.1, -np.inf]], np.float32)
    allp = np.concatenate([pts[:700], bad[:1], pts[700:], bad[1:]])  # NaN in the middle of a wave, inf rows at the end
    tg = ops.TriangleGrid(*gpu(name, dev))
    assert tg.G == D.default_grid(len(t)) and tg.cell_ptr[-1].item() == tg.M == tg.cell_tri.shape[0]
    d2, face, bary = ops.mesh_closest_point(torch.from_numpy(allp).to(dev), tg)
    assert d2.dtype == torch.float32 and face.dtype == torch.int32 and bary.dtype == torch.float32
    rows = torch.tensor([700, len(allp) - 2, len(allp) - 1], device=dev)
    assert torch.isnan(d2[rows]).all() and (face[rows] == -1).all() and (bary[rows] == 0).all()
    keep = torch.ones(len(allp), dtype=torch.bool, device=dev)
    keep[rows] = False
    check_rows(pts, v, t, d_ref, M, d2[keep], face[keep], bary[keep], name)
    # the other rows of the launch are unaffected by the rows that are not finite
    clean = ops.mesh_closest_point(torch.from_numpy(pts).to(dev), tg)
    for x, y in zip((d2, face, bary), clean):
        assert torch.equal(x[keep], y)


# ---- b. independence, bit for bit ----
@pytest.mark.parametrize("name", ["sphere24", "two_clusters", "spanning"])
def test_answer_is_independent_of_grid_order_and_launch(dev, name):
    v, t = mesh_np(name)
    pts, d_ref, M = case(name)
    if name == "two_clusters":  # 64 points on the mid-plane between the clusters: ~16 rings at G = 33, near-ties
        rng = np.random.default_rng(21)
        mid = np.concatenate([np.zeros((64, 1)), rng.uniform(-0.3, 0.3, (64, 2))], 1).astype(np.float32)
        pts = np.concatenate([pts, mid])
    vg, tgpu = gpu(name, dev)
    p = torch.from_numpy(pts).to(dev)
    base = ops.mesh_closest_point(p, ops.TriangleGrid(vg, tgpu, grid=1))  # brute force through the same kernel
    assert (base[1] >= 0).all()
    for G in (2, 7, 33, None):
        tg = ops.TriangleGrid(vg, tgpu, grid=G)
        for cell_order in (False, True):
            got = ops.mesh_closest_point(p, tg, cell_order=cell_order)
            for x, y, what in zip(got, base, ("d2", "face", "bary")):
                assert torch.equal(x, y), f"{what} differs at G={tg.G} cell_order={cell_order}: " \
                                          f"{int((x != y).reshape(len(pts), -1).any(1).sum())} rows"
    perm = torch.from_numpy(np.random.default_rng(22).permutation(len(pts))).to(dev)
    for cell_order in (False, True):
        got = ops.mesh_closest_point(p[perm], tg, cell_order=cell_order)
        for x, y in zip(got, base):
            assert torch.equal(x, y[perm])
    for _ in range(3):
        for x, y in zip(ops.mesh_closest_point(p, tg), base):
            assert torch.equal(x, y)
    if name == "two_clusters":
        check_rows(pts, v, t, np.sqrt(D.pair_matrix(pts, v, t).min(1)[0].numpy()), None, *base, "two_clusters + mid-plane")


# ---- c. seams ----
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1025])
def test_point_counts_around_the_wave_and_block_size(dev, N):
    v, t = mesh_np("sphere24")
    pts, d_ref, M = case("sphere24")
    sel = np.arange(N) * 2 % len(pts)
    tg = ops.TriangleGrid(*gpu("sphere24", dev))
    for cell_order in (False, True):
        got = ops.mesh_closest_point(torch.from_numpy(pts[sel]).to(dev), tg, cell_order=cell_order)
        check_rows(pts[sel], v, t, d_ref[sel], M[sel], *got, f"N={N}")
    empty = ops.mesh_closest_point(torch.zeros(0, 3, device=dev), tg)
    assert [x.shape[0] for x in empty] == [0, 0, 0]


def test_every_triangle_in_one_cell(dev):
    v, t = mesh_np("one_octant")
    pts = D.query_points(v, t)
    M = D.pair_matrix(pts, v, t)
    tg = ops.TriangleGrid(*gpu("one_octant", dev), grid=2)
    ptr = tg.cell_ptr.cpu().numpy()
    assert (np.diff(ptr) > 0).sum() == 1 and tg.M == len(t)  # one occupied cell, which holds every triangle
    got = ops.mesh_closest_point(torch.from_numpy(pts).to(dev), tg)
    check_rows(pts, v, t, M.min(1)[0].sqrt().numpy(), M.numpy(), *got, "one_octant G=2")


def test_a_mesh_without_extent_and_bad_arguments(dev):
    v = torch.full((3, 3), 0.25, device=dev)
    tri = torch.tensor([[0, 1, 2]], device=dev, dtype=torch.int32)
    tg = ops.TriangleGrid(v, tri, grid=4)
    p = torch.tensor([[0.25, 0.25, 0.25], [1.25, 0.25, 0.25]], device=dev)
    d2, face, bary = ops.mesh_closest_point(p, tg)
    assert d2.tolist() == [0.0, 1.0] and face.tolist() == [0, 0] and torch.allclose(bary.sum(1), torch.ones(2, device=dev))
    with pytest.raises(ValueError):
        ops.TriangleGrid(v, tri + 1)  # an index outside [0, V)
    with pytest.raises(ValueError):
        ops.TriangleGrid(v * float("nan"), tri)
    with pytest.raises(ValueError):
        ops.TriangleGrid(v, tri[:0])
    with pytest.raises(ValueError):
        ops.mesh_closest_point(torch.zeros(4, 2, device=dev), tg)


# ---- d. backward ----
def test_backward_matches_float64_autograd_with_the_face_fixed(dev):
    v, t = mesh_np("sphere24")
    rng = np.random.default_rng(31)
    pts = rng.uniform(-0.9, 0.9, (3000, 3)).astype(np.float32)
    wts = rng.uniform(-1, 1, 3000).astype(np.float32)
    vg, tgpu = gpu("sphere24", dev)
    p = torch.from_numpy(pts).to(dev).requires_grad_(True)
    vv = vg.clone().requires_grad_(True)
    tg = ops.TriangleGrid(vg, tgpu)
    d2 = ops.point_mesh_distance2(p, vv, tgpu, tg)
    (torch.from_numpy(wts).to(dev) * d2).sum().backward()
    face = ops.mesh_closest_point(p.detach(), tg)[1].cpu().numpy()
    assert torch.equal(d2.detach(), ops.mesh_closest_point(p.detach(), tg)[0])
    P = torch.tensor(pts, dtype=torch.float64, requires_grad=True)
    V = torch.tensor(v, dtype=torch.float64, requires_grad=True)
    corner = [V[torch.from_numpy(t[face, k].astype(np.int64))] for k in range(3)]
    (torch.tensor(wts, dtype=torch.float64) * D.closest_point(P, *corner)[0]).sum().backward()
    for name, got, want in (("grad_points", p.grad, P.grad), ("grad_v_pos", vv.grad, V.grad)):
        err = (got.cpu().double() - want).abs().max().item() / want.abs().max().item()
        print(f"{name}: max |got - float64| = {err:.3e} of the gradient's max-abs; "
              f"most points on one vertex {np.bincount(t[face].reshape(-1)).max()}")
        assert err <= 1e-4
    # a grid built inside the call, points alone requiring grad, and a row that is not finite
    q = torch.from_numpy(np.concatenate([pts[:5], [[np.nan, 0, 0]]]).astype(np.float32)).to(dev).requires_grad_(True)
    out = ops.point_mesh_distance2(q, vg, tgpu)
    out[:5].sum().backward()
    assert torch.isnan(out[5]) and torch.equal(q.grad[5], torch.zeros(3, device=dev))
    assert torch.allclose(q.grad[:5], p.grad[:5] / torch.from_numpy(wts[:5]).to(dev)[:, None], rtol=1e-5, atol=1e-7)


# ---- e. sampler ----
@pytest.mark.parametrize("name,spacing", [("sphere24", 0.05), ("sphere24", 0.0133), ("hand", 0.021)])
def test_sampler_matches_the_restatement(dev, name, spacing):
    v, t = mesh_np(name)
    ks, ratio = D.face_k(v, t, spacing)
    assert np.abs(ratio - np.round(ratio)).min() > 1e-4, "spacing too close to an integer division of an edge"
    want_p, want_f = D.surface_samples(v, t, spacing)
    pts, face = ops.mesh_surface_samples(*gpu(name, dev), spacing)
    assert pts.dtype == torch.float32 and face.dtype == torch.int32
    assert pts.shape == (len(want_p), 3) and np.array_equal(face.cpu().numpy(), want_f)
    err = np.abs(pts.cpu().numpy().astype(np.float64) - want_p).max()
    print(f"{name} spacing {spacing}: S {len(want_p)}, k {ks.min()}..{ks.max()}, max |p - ref| = {err:.3e}")
    assert err <= 1e-6 * np.abs(v).max()


def test_sampler_refuses_too_many_samples_before_allocating(dev):
    vg, tgpu = gpu("sphere24", dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(ValueError, match="spacing"):
        ops.mesh_surface_samples(vg, tgpu, 1e-5)  # ~1e11 samples
    assert torch.cuda.max_memory_allocated() - before < 1 << 20


# ---- f. distance_to ----
def _subset_max(samples, mesh, extra, seed):
    """float64 one-sided maximum over a fixed 2 000-sample subset plus `extra` (the GPU's argmax sample), and the
    float64 distance of `extra` alone."""
    s = samples.cpu().numpy()
    pick = np.random.default_rng(seed).permutation(len(s))[:2000]
    pts = np.concatenate([s[pick], np.asarray(extra, np.float32)[None]])
    d = np.sqrt(D.pair_matrix(pts, mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy()).min(1)[0].numpy())
    return d.max(), d[-1]


def test_distance_to_against_float64(dev):
    full = Mesh(*gpu("sphere24", dev))
    low = full.simplify(grid=8)
    L = np.abs(mesh_np("sphere24")[0]).max()
    res = low.distance_to(full)
    diag = max(float((m.v_pos.amax(0) - m.v_pos.amin(0)).norm()) for m in (low, full))
    assert res["spacing"] == pytest.approx(diag / 200, rel=1e-6)
    for side, src, dst, seed in (("a_to_b", low, full, 41), ("b_to_a", full, low, 42)):
        samples = ops.mesh_surface_samples(src.v_pos, src.t_pos_idx, res["spacing"])[0]
        sub_max, at_argmax = _subset_max(samples, dst, res[side]["argmax_point"], seed)
        print(f"{side}: S {len(samples)} max {res[side]['max']:.5f} mean {res[side]['mean']:.5f} rms "
              f"{res[side]['rms']:.5f}; float64 at the argmax sample {at_argmax:.5f}, over the subset {sub_max:.5f}")
        assert abs(res[side]["max"] - at_argmax) <= REL * L  # the reported maximum is the distance of a real sample
        assert sub_max <= res[side]["max"] + REL * L         # ... and no sample of the subset lies farther
        assert (samples == torch.tensor(res[side]["argmax_point"], device=dev)).all(1).any()
        assert 0 < res[side]["mean"] <= res[side]["rms"] <= res[side]["max"]
    assert res["hausdorff"] == max(res["a_to_b"]["max"], res["b_to_a"]["max"])
    assert res["n_samples"][0] > 0 and res["n_samples"][1] > 0
    swapped = full.distance_to(low)
    assert swapped["a_to_b"] == res["b_to_a"] and swapped["b_to_a"] == res["a_to_b"]
    assert swapped["hausdorff"] == res["hausdorff"] and swapped["n_samples"] == res["n_samples"][::-1]
    same = full.distance_to(full)
    print(f"self distance {same['hausdorff']:.3e} (bar {REL * L:.3e})")
    assert same["hausdorff"] <= REL * L
    d2, face, bary = full.closest_point(full.v_pos[:10])
    assert (d2 <= (REL * L) ** 2).all() and face.dtype == torch.int32 and bary.shape == (10, 3)


# ---- g. simplify(max_error=) ----
@pytest.fixture(scope="module")
def torus_runs(dev):
    full = Mesh(*gpu("torus32", dev))
    full.add_extra("tag", 7)
    return full, {e: full.simplify(max_error=e) for e in (0.1, 0.025)}


@pytest.mark.parametrize("budget", [0.1, 0.025])
def test_simplify_max_error_meets_the_budget(dev, torus_runs, budget):
    full, runs = torus_runs
    low = runs[budget]
    info = low.extras["simplify"]
    err = info["error"]
    assert low is not full and 0 < low.t_pos_idx.shape[0] < full.t_pos_idx.shape[0]
    assert sorted(info) == ["cell", "error", "grid", "n_clusters", "vertex_map"] and low.extras["tag"] == 7
    assert "simplify" not in full.extras
    assert err["max_error"] == budget and err["spacing"] == budget / 4
    assert err["hausdorff"] + err["spacing"] <= budget
    again = full.simplify(grid=info["grid"])
    assert torch.equal(again.v_pos, low.v_pos) and torch.equal(again.t_pos_idx, low.t_pos_idx)
    for side, src, dst, seed in (("a_to_b", low, full, 51), ("b_to_a", full, low, 52)):
        samples = ops.mesh_surface_samples(src.v_pos, src.t_pos_idx, err["spacing"])[0]
        sub_max, at_argmax = _subset_max(samples, dst, err[side]["argmax_point"], seed)
        print(f"budget {budget} grid {info['grid']} T {full.t_pos_idx.shape[0]} -> {low.t_pos_idx.shape[0]} {side}: "
              f"max {err[side]['max']:.5f}, float64 subset max {sub_max:.5f}")
        assert sub_max <= budget and sub_max <= err[side]["max"] + REL


def test_simplify_max_error_tighter_budget_keeps_more_faces(torus_runs):
    full, runs = torus_runs
    assert runs[0.025].t_pos_idx.shape[0] >= runs[0.1].t_pos_idx.shape[0]
    assert runs[0.025].extras["simplify"]["grid"] >= runs[0.1].extras["simplify"]["grid"]


def test_other_simplify_modes_are_unchanged(dev, torus_runs):
    full, _ = torus_runs
    by_grid = full.simplify(grid=12)
    want = ops.mesh_simplify(full.v_pos, full.t_pos_idx, 12)
    assert torch.equal(by_grid.v_pos, want[0]) and torch.equal(by_grid.t_pos_idx, want[1])
    by_faces = full.simplify(target_faces=600)
    want = ops.mesh_simplify(full.v_pos, full.t_pos_idx, by_faces.extras["simplify"]["grid"])
    assert torch.equal(by_faces.v_pos, want[0]) and torch.equal(by_faces.t_pos_idx, want[1])
    assert 0 < by_faces.t_pos_idx.shape[0] <= 600
    for m in (by_grid, by_faces):
        assert sorted(m.extras["simplify"]) == ["cell", "grid", "n_clusters", "vertex_map"]
    with pytest.raises(ValueError, match="samples"):
        full.simplify(max_error=1e-7)


@pytest.fixture(scope="module")
def modules(dev):
    return _exporter_modules(dev)


def test_exporter_simplify_max_error(modules):
    r, g, m, b, cache = modules
    cfg = {"fmt": "obj"}
    with torch.no_grad():
        full = r.isosurface(cache)[0]
    cell = 2.0 * float(g.cfg.radius) / 64  # one isosurface cell (resolution 64)
    exp = _exporter(modules, cfg)
    assert exp.simplify_max_error is None
    exp.simplify_max_error = 2 * cell
    (out,) = exp(cache)
    mesh = out.params["mesh"]
    err = mesh.extras["simplify"]["error"]
    print(f"exporter max_error {2 * cell:.4f}: T {full.t_pos_idx.shape[0]} -> {mesh.t_pos_idx.shape[0]}, grid "
          f"{mesh.extras['simplify']['grid']}, hausdorff {err['hausdorff']:.5f}")
    assert 0 < mesh.t_pos_idx.shape[0] < full.t_pos_idx.shape[0]
    assert err["hausdorff"] + err["spacing"] <= 2 * cell == err["max_error"]
    assert exp._bake_max_step(mesh) == mesh.extras["simplify"]["cell"]
    exp.simplify_max_error = None
    (plain,) = exp(cache)
    (fresh,) = _exporter(modules, cfg)(cache)
    for key in ("v_pos", "t_pos_idx", "v_rgb"):
        assert torch.equal(getattr(plain.params["mesh"], key), getattr(fresh.params["mesh"], key))
    assert torch.equal(plain.params["mesh"].t_pos_idx, full.t_pos_idx)
    assert "simplify" not in plain.params["mesh"].extras
