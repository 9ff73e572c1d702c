"""Point-to-mesh distance without a GPU: the library's surface, the argument checks of Mesh.simplify(max_error=) and the
exporter, and the float64 restatement (tests/distance_reference.py) itself -- against closed-form cases, against
Ericson's formulation, its mirror of the kernel's ring search against brute force, and the sampler's covering property."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import simplify_reference as S  # noqa: E402

ENTRY_POINTS = ["tt_dist_workspace_bytes", "tt_dist_build_count", "tt_dist_build_fill", "tt_dist_keys", "tt_dist_query",
                "tt_dist_bwd", "tt_dist_sample_workspace_bytes", "tt_dist_sample_count", "tt_dist_sample_emit"]


def test_library_surface():
    assert "tt_dist.hip" in _lib.SOURCES
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_dist_")) == sorted(ENTRY_POINTS)
    assert _lib._expected_abi() == 17
    assert _lib.TT_DIST_MAX_GRID == 256
    assert _lib.TT_DIST_MAX_SAMPLES == 2 ** 26
    assert [ops.dist_default_grid(t) for t in (1, 64, 65, 1772, 10 ** 6, 10 ** 7)] == [1, 1, 2, 6, 125, 256]
    assert [D.default_grid(t) for t in (1, 64, 65, 1772, 10 ** 6, 10 ** 7)] == [1, 1, 2, 6, 125, 256]


def _cpu_mesh():
    v, tri = S.single_triangle()
    return Mesh(torch.from_numpy(v), torch.from_numpy(tri))


def test_simplify_max_error_argument_errors_need_no_gpu():
    mesh = _cpu_mesh()
    with pytest.raises(ValueError):
        mesh.simplify(grid=4, max_error=0.1)
    with pytest.raises(ValueError):
        mesh.simplify(target_faces=10, max_error=0.1)
    with pytest.raises(ValueError):
        mesh.simplify(grid=4, target_faces=10, max_error=0.1)
    with pytest.raises(ValueError):
        mesh.simplify()
    for bad in (0, -1, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError):
            mesh.simplify(max_error=bad)
    for v, t in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)),
                 (torch.rand(5, 3), torch.zeros(0, 3, dtype=torch.int32))):
        empty = Mesh(v, t)
        assert empty.simplify(max_error=0.1) is empty


def test_exporter_refuses_two_simplify_attributes():
    exp = __import__("triplaneturbo_amd").find("multiprompt-mesh-exporter")({}, geometry=None, material=None,
                                                                            background=None)
    assert exp.simplify_max_error is None
    for two in (("simplify_grid", 8, "simplify_max_error", 0.1), ("simplify_target_faces", 100, "simplify_max_error", 0.1),
                ("simplify_grid", 8, "simplify_target_faces", 100)):
        exp.simplify_grid = exp.simplify_target_faces = exp.simplify_max_error = None
        setattr(exp, two[0], two[1])
        setattr(exp, two[2], two[3])
        with pytest.raises(ValueError, match="at most one"):
            exp(torch.zeros(1))


def test_ops_argument_errors_need_no_gpu():
    v, tri = (torch.from_numpy(x) for x in S.single_triangle())
    for g in (0, 257, -3):
        with pytest.raises(ValueError):
            ops.TriangleGrid(v, tri, grid=g)
    with pytest.raises(TypeError):
        ops.TriangleGrid(v, tri, grid=2.0)
    for sp in (0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            ops.mesh_surface_samples(v, tri, sp)
    with pytest.raises(RuntimeError):
        ops.TriangleGrid(v, tri)  # no CPU path
    with pytest.raises(RuntimeError):
        ops.mesh_surface_samples(v, tri, 0.1)
    with pytest.raises(TypeError):
        ops.mesh_closest_point(torch.zeros(4, 3), None)


# ---- the restatement against closed forms ----
A, B, C = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
REGIONS = [  # point, distance, barycentrics
    ("face", [0.25, 0.25, 1.0], 1.0, [0.5, 0.25, 0.25]),
    ("vertex a", [-1.0, -1.0, 0.0], np.sqrt(2.0), [1, 0, 0]),
    ("vertex b", [2.0, -0.2, 0.0], np.sqrt(1.04), [0, 1, 0]),
    ("vertex c", [-0.2, 2.0, 0.0], np.sqrt(1.04), [0, 0, 1]),
    ("edge ab", [0.5, -1.0, 0.5], np.sqrt(1.25), [0.5, 0.5, 0]),
    ("edge ac", [-1.0, 0.5, 0.5], np.sqrt(1.25), [0.5, 0, 0.5]),
    ("edge bc", [1.0, 1.0, 0.5], np.sqrt(0.75), [0, 0.5, 0.5]),
]


def _one(p, a, b, c):
    d2, bary = D.closest_point(*(torch.as_tensor(np.asarray(x, np.float64)) for x in (p, a, b, c)))
    return float(d2.sqrt()), bary.numpy()


@pytest.mark.parametrize("name,p,dist,bary", REGIONS)
def test_restatement_in_each_voronoi_region(name, p, dist, bary):
    d, b = _one(p, A, B, C)
    assert abs(d - dist) <= 1e-14 and np.abs(b - np.asarray(bary, np.float64)).max() <= 1e-14
    assert abs(np.sqrt(D.ericson(np.asarray(p), A, B, C)) - dist) <= 1e-14


def test_restatement_on_degenerate_triangles():
    p = np.array([1.5, 1.0, 0.0])
    far = np.array([2.0, 0.0, 0.0])
    cases = [((A, A, far), 1.0),                      # two equal vertices: the segment a-c
             ((A, far, far), 1.0), ((far, A, far), 1.0),
             ((A, A, A), np.sqrt(3.25)),              # three equal vertices: a point
             ((A, far, B), 1.0), ((B, A, far), 1.0)]  # collinear: the union of the segments is [0, 2] on the x axis
    for (a, b, c), want in cases:
        d, bary = _one(p, a, b, c)
        assert np.isfinite(d) and np.isfinite(bary).all()
        assert abs(d - want) <= 1e-14
        assert bary.min() >= 0 and abs(bary.sum() - 1) <= 1e-14


def test_restatement_agrees_with_ericson_on_random_pairs():
    rng = np.random.default_rng(5)
    P = rng.uniform(-1.5, 1.5, (200, 1, 3))
    T = rng.uniform(-1, 1, (1, 200, 3, 3))
    P, T = np.broadcast_to(P, (200, 200, 3)), np.broadcast_to(T, (200, 200, 3, 3))
    mine = D.closest_point(*(torch.as_tensor(np.ascontiguousarray(x)) for x in (P, T[..., 0, :], T[..., 1, :], T[..., 2, :])))[0]
    book = D.ericson(P, T[..., 0, :], T[..., 1, :], T[..., 2, :])
    assert np.abs(np.sqrt(mine.numpy()) - np.sqrt(book)).max() <= 1e-12


# ---- the ring search and its stopping rule ----
@pytest.fixture(scope="module")
def search_case():
    rng = np.random.default_rng(6)
    centres = rng.uniform(-0.8, 0.8, (190, 1, 3))
    v = (centres + rng.uniform(-0.2, 0.2, (190, 3, 3))).reshape(-1, 3).astype(np.float32)
    tri = np.arange(570, dtype=np.int32).reshape(190, 3)
    tri = np.concatenate([tri, tri[:10]])  # ten faces twice: equal distance, the smaller index must win
    lo = v.min(0)
    ext = (v.max(0) - lo).max()
    edges = [lo + ext * np.float32(k) / np.float32(g) for g in (2, 5) for k in range(g + 1)]  # exactly on cell boundaries
    pts = np.concatenate([rng.uniform(-1.5, 1.5, (120, 3)),
                          np.stack([edges[i % len(edges)] for i in range(40)]),
                          v[rng.permutation(len(v))[:40]]]).astype(np.float32)
    pts[120:140, 1] = rng.uniform(-1, 1, 20)  # boundary in x and z only
    return pts, v, tri, D.pair_matrix(pts, v, tri).numpy()


@pytest.mark.parametrize("G", [1, 2, 5])
def test_ring_search_equals_brute_force_exactly(search_case, G):
    pts, v, tri, M = search_case
    assert pts.shape == (200, 3) and tri.shape == (200, 3)
    d2, face = D.grid_search(pts, v, tri, G, M)
    assert np.array_equal(d2, M.min(1))
    assert np.array_equal(face, M.argmin(1))  # numpy's argmin is the first, i.e. the smallest, index
    assert (M[:, :10] == M[:, 190:]).all() and (face < 190).all()  # the duplicated faces tie; the smaller index wins


def test_stopping_one_ring_early_would_be_caught(search_case):
    """The mirror with the bound loosened by one ring (r + 1 in place of r) gives a wrong answer on this set: the case
    can tell a sound stopping rule from an unsound one."""
    pts, v, tri, M = search_case
    G = 5
    lo, ext, h, inv_h = D.box(v, G)
    p3 = v[tri]
    c0, c1 = D.cell(p3.min(1), lo, inv_h, G), D.cell(p3.max(1), lo, inv_h, G)
    wrong = 0
    for i, p in enumerate(pts):
        q = np.minimum(np.maximum(p, lo), lo + ext)
        c = D.cell(q, lo, inv_h, G)
        best = np.inf
        for r in range(G):
            near = ((c0 <= c + r) & (c1 >= c - r)).all(1)
            best = M[i, near].min() if near.any() else np.inf
            if best < ((p - q).astype(np.float64) ** 2).sum() + ((r + 1) * float(h)) ** 2:
                break
        wrong += best != M[i].min()
    assert wrong > 0


# ---- the sampler ----
def test_sampler_counts_and_covering():
    v, tri = D.two_clusters()
    spacing = 0.031
    ks, ratio = D.face_k(v, tri, spacing)
    assert np.abs(ratio - np.round(ratio)).min() > 1e-4
    pts, face = D.surface_samples(v, tri, spacing)
    assert np.array_equal(np.bincount(face, minlength=len(tri)), (ks + 1) * (ks + 2) // 2)
    assert np.array_equal(face, np.sort(face))
    # the first and last sample of a face are its corners a and c
    first = np.concatenate([[0], np.cumsum((ks + 1) * (ks + 2) // 2)[:-1]])
    assert np.array_equal(pts[first], v.astype(np.float64)[tri[:, 0]])
    rng = np.random.default_rng(7)
    f = rng.integers(0, len(tri), 2000)
    b = rng.dirichlet([1, 1, 1], 2000)
    surf = (b[:, :, None] * v.astype(np.float64)[tri[f]]).sum(1)
    gap = np.array([np.sqrt(((pts[face == fi] - s) ** 2).sum(1).min()) for fi, s in zip(f, surf)])
    print(f"sampler: S = {len(pts)}, largest gap to the face's own samples {gap.max() / spacing:.3f} spacing")
    assert gap.max() <= spacing
