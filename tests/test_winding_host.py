"""Winding number without a GPU: the library's surface, the argument checks of the wrappers, the OBJ reader, and the
float64 restatement (tests/winding_reference.py) itself -- closed surfaces, the zero cases, the tree's ranges, the
(l, m) walk, and the cap on the points its comparisons leave out."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops, shape, viewer
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_reference as S  # noqa: E402
import winding_reference as W  # noqa: E402

ENTRY_POINTS = ["tt_wind_node_count", "tt_wind_face_keys", "tt_wind_build", "tt_wind_point_keys", "tt_wind_exact",
                "tt_wind_fast"]


def test_library_surface():
    assert "tt_wind.hip" in _lib.SOURCES
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_wind_")) == sorted(ENTRY_POINTS)
    assert _lib.TT_WIND_MAX_LEVELS == 6
    sizes = (1, 6, 7, 24, 25, 96, 97, 1772, 3040, 6144, 6145, 27_748, 84_460, 473_060, 10 ** 8)
    assert [ops.wind_default_levels(t) for t in sizes] == [W.default_levels(t) for t in sizes] \
        == [0, 0, 1, 1, 2, 2, 3, 5, 5, 5, 6, 6, 6, 6, 6]


def test_argument_errors_need_no_gpu():
    v, tri = (torch.from_numpy(x) for x in S.single_triangle())
    pts = torch.zeros(4, 3)
    for levels in (-1, 7, 100):
        with pytest.raises(ValueError):
            ops.WindingTree(v, tri, levels=levels)
    for levels in (2.0, True, "3"):
        with pytest.raises(TypeError):
            ops.WindingTree(v, tri, levels=levels)
    for beta in (0, -1.0, float("nan"), "2", True):
        with pytest.raises(ValueError):
            ops.mesh_winding_number(pts, v, tri, beta=beta)
        with pytest.raises(ValueError):
            ops.mesh_signed_distance(pts, v, tri, beta=beta)
    with pytest.raises(RuntimeError):
        ops.WindingTree(v, tri)  # no CPU path
    with pytest.raises(RuntimeError):
        ops.mesh_winding_number(pts, v, tri)
    with pytest.raises(RuntimeError):
        ops.mesh_contains(pts, v, tri, exact=True)
    with pytest.raises(RuntimeError):
        ops.mesh_signed_distance(pts, v, tri)
    with pytest.raises(RuntimeError):
        Mesh(v, tri).contains(pts)
    with pytest.raises(TypeError):
        ops.mesh_winding_number(pts, None)
    with pytest.raises(TypeError):
        ops.mesh_winding_number(pts, v)  # v_pos without t_pos_idx
    with pytest.raises(RuntimeError):
        shape.MeshOBJ(*S.single_triangle()).winding_number(pts)  # the query decides the device


# ---- the restatement ----
def _probe_points(v):
    rng = np.random.default_rng(3)
    lo, ext, _ = W.box(v, 0)
    return lo.astype(np.float64) + rng.uniform(-0.2, 1.2, (400, 3)) * float(ext)


def _inside_sphere24(p):
    return np.linalg.norm(p, axis=1)


@pytest.mark.parametrize("name", ["sphere24", "torus32"])
def test_closed_surfaces_give_one_inside_zero_outside(name):
    v, t = W.mesh(name)
    p = _probe_points(v)
    w = W.exact(p, v, t)
    side = np.round(w)
    assert np.abs(w - side).max() <= 1e-9 and set(side.astype(int)) == {0, 1}
    if name == "sphere24":  # the extractor's sphere: 1 well inside its radius, 0 well outside
        r = np.linalg.norm(v.astype(np.float64), axis=1)
        d = np.linalg.norm(p, axis=1)
        assert (side[d < 0.95 * r.min()] == 1).all() and (side[d > 1.05 * r.max()] == 0).all()
    flipped = W.exact(p, v, t[:, ::-1])
    assert np.abs(flipped + side).max() <= 1e-9


def test_zero_cases():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    in_plane = np.array([[0.25, 0.25, 0.0], [3.0, -2.0, 0.0], [0.5, 0.5, 0.0], [-0.0, -1.0, -0.0]])  # inside, outside, on an edge
    for dtype in (np.float64, np.float32):
        assert (W.solid_angle(in_plane, a, b, c, dtype) == 0).all()
        p = np.array([[0.3, 0.2, 0.7], [0.5, 0.0, -0.0]])
        assert (W.solid_angle(p, a, b, b, dtype) == 0).all() and (W.solid_angle(p, a, a, a, dtype) == 0).all()
        # collinear, distinct vertices: num is rounding noise, not a zero; the angle stays noise while den > 0
        assert np.abs(W.solid_angle(p, a, b, 0.5 * (a + b), dtype)).max() <= 1e-6
    # just off the plane: a half space, negative on the side the normal (+z) points to
    above = W.solid_angle(np.array([0.2, 0.2, 1e-9]), a, b, c)
    assert abs(above + 2 * np.pi) <= 1e-6 and abs(W.solid_angle(np.array([0.2, 0.2, -1e-9]), a, b, c) - 2 * np.pi) <= 1e-6


@pytest.mark.parametrize("name,L", [("sphere24", 3), ("hand", 1), ("two_clusters", 2)])
def test_beta_inf_equals_the_exact_sum(name, L):
    pts, w, _, _ = W.case(name)
    wf, _ = W.fast(W.tree(name, L), pts[:300], np.inf)
    assert np.abs(wf - w[:300]).max() <= 1e-12
    assert abs(W.fast_one(W.tree(name, L), pts[7], np.inf) - w[7]) <= 1e-12


@pytest.mark.parametrize("L", [0, 1, 3])
def test_walk_with_every_node_near_visits_every_leaf_once_in_morton_order(L):
    visited = list(W.walk(L, lambda l, m: True))
    assert [m for l, m in visited if l == L] == list(range(8 ** L))
    assert len(visited) == (8 ** (L + 1) - 1) // 7 and len(set(visited)) == len(visited)
    # nothing near: the root alone; one path near: the siblings of the path
    assert list(W.walk(L, lambda l, m: False)) == [(0, 0)]
    if L == 3:
        path = list(W.walk(L, lambda l, m: m == 0))
        assert path == ([(0, 0), (1, 0), (2, 0)] + [(3, m) for m in range(8)] + [(2, m) for m in range(1, 8)]
                        + [(1, m) for m in range(1, 8)])


@pytest.mark.parametrize("name,L", [("sphere24", 3), ("torus32", 2), ("hand", 2), ("spanning", 1)])
def test_node_ranges_are_contiguous_unions_of_the_children(name, L):
    tr = W.tree(name, L)
    v, t = W.mesh(name)
    keys = W.face_keys(v, t, L)[tr.order]
    assert (np.diff(keys) >= 0).all() and tr.leaf_ptr[-1] == len(t)
    same = np.diff(keys) == 0
    assert (np.diff(tr.order)[same] > 0).all()  # (key, face) order
    for l in range(L + 1):
        lv = tr.levels[l]
        shift = 3 * (L - l)
        for m in range(8 ** l):
            rows = np.flatnonzero(keys >> shift == m)
            assert lv["end"][m] - lv["begin"][m] == len(rows)
            assert len(rows) == 0 or (rows[0] == lv["begin"][m] and rows[-1] == lv["end"][m] - 1)
            assert (lv["r"][m] < 0) == (len(rows) == 0)
        if l < L:
            ch = tr.levels[l + 1]
            assert np.array_equal(lv["begin"], ch["begin"][0::8]) and np.array_equal(lv["end"], ch["end"][7::8])
            assert np.array_equal(ch["begin"][1:], ch["end"][:-1])
    root = tr.levels[0]
    tri64 = v.astype(np.float64)[t]
    n_all = 0.5 * np.cross(tri64[:, 1] - tri64[:, 0], tri64[:, 2] - tri64[:, 0])
    assert np.abs(root["N"][0] - n_all.sum(0)).max() <= 1e-12
    assert np.linalg.norm(tri64.reshape(-1, 3) - root["c"][0], axis=1).max() <= root["r"][0] + 1e-12  # r bounds the faces


@pytest.mark.parametrize("name", W.MESHES)
def test_points_left_out_stay_within_their_caps(name):
    pts, w, away, _ = W.case(name)
    print(f"{name}: {len(pts)} points, {(~away).sum()} closer than {W.NEAR_SURFACE} extents to the surface")
    assert len(pts) * len(W.mesh(name)[1]) <= 6_000_000
    assert (~away).mean() <= 0.01
    for L in (0, 1, 3):  # the depths of test (d) of tests/test_gpu_winding.py
        for beta in (2.0, 3.0):
            _, margin, err = W.fast_case(name, L, beta)
            print(f"   L {L} beta {beta}: method error {err:.3e}, margin <= 1e-4 for {(margin <= 1e-4).mean():.4f}")
            assert (margin <= 1e-4).mean() <= 0.05


def test_own_atan2_accuracy():
    """The fp32 mirror of the kernel's wind_atan2 against float64 arctan2 over every octant, 17 decades of magnitude, the
    reduction threshold tan(pi/8), the diagonal and the negative x axis: 2.85 ulp at most (numpy's own float32 arctan2
    shows 3.3 on the same set), mean 0.39.  The bar: Cephes' atanf polynomial (peak relative error 1.9e-7, 1.6 ulp),
    half an ulp each for the quotient and the two octant subtractions: 3.1."""
    rng = np.random.default_rng(1)
    n = 1_000_000
    ang, r = rng.uniform(-np.pi, np.pi, n), np.exp(rng.uniform(-20, 20, n))
    k = rng.uniform(0.1, 10, 50_000).astype(np.float32)
    wiggle = (1 + rng.uniform(-1e-6, 1e-6, len(k))).astype(np.float32)
    y = np.concatenate([(r * np.sin(ang)).astype(np.float32), k * np.float32(0.41421356) * wiggle, k, k * np.float32(1e-20)])
    x = np.concatenate([(r * np.cos(ang)).astype(np.float32), k, k * wiggle, -k])
    y, x = y[y != 0], x[y != 0]
    ref = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(W.atan2_f32(y, x).astype(np.float64) - ref) / ulp
    print(f"wind_atan2 (fp32 mirror): max {err.max():.2f} ulp, mean {err.mean():.2f}; numpy float32 arctan2: "
          f"{(np.abs(np.arctan2(y, x).astype(np.float64) - ref) / ulp).max():.2f}")
    assert err.max() <= 3.1
    with np.errstate(invalid="ignore"):
        assert np.isnan(W.atan2_f32(np.float32(np.inf), np.float32(np.inf)))  # the pair turns this NaN into 0


# ---- the OBJ reader ----
def test_obj_reader_accepts_the_four_face_forms_and_a_quad(tmp_path):
    path = tmp_path / "forms.obj"
    path.write_text("# a comment\nmtllib none.mtl\nv 0 0 0\nv 1 0 0 0.5 0.5 0.5\nv 1 1 0\nv 0 1 0\nv 0 0 1\n"
                    "vt 0 0\nvt 1 0\nvt 1 1\nvn 0 0 1\n"
                    "f 1 2 3\nf 1/1 3/2 4/3\nf 1/1/1 2/2/1 5/3/1\nf 2//1 3//1 5//1\nf 1 2 3 4\nf -1 -2 -3\n\ng tail\n")
    v, f = viewer.read_obj_geometry(str(path))
    assert v.shape == (5, 3) and v.dtype == np.float64 and f.dtype == np.int64
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [0, 1, 2], [0, 2, 3], [4, 3, 2]]
    (tmp_path / "bad.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n")
    with pytest.raises(ValueError):
        viewer.read_obj_geometry(str(tmp_path / "bad.obj"))
    (tmp_path / "two.obj").write_text("v 0 0 0\nv 1 0 0\nf 1 2\n")
    with pytest.raises(ValueError):
        viewer.read_obj_geometry(str(tmp_path / "two.obj"))
    loss = shape.ShapeLoss(str(path))  # a file without usable vt / a quad loads; no GPU until the first query
    assert loss.sketchshape.v.shape == (5, 3) and abs(np.linalg.norm(loss.sketchshape.v, axis=1).max() - 0.7) <= 1e-12
    assert np.allclose(loss.sketchshape.v, W.shape_loss_mesh(v), atol=1e-15)
