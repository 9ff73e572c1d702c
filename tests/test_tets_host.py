"""Marching tetrahedra without a GPU: the C ABI's surface and argument validation, the Kuhn grid generator, the numpy
oracle of the contract (tests/mt_reference.py) against the reference helper's recorded results
(tests/golden/reference_tets.npz, written by tests/golden/make_golden_tets.py), and the torch-only parts of
MarchingTetrahedraHelper and the mesh renderer's "mt" configuration."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import _lib, ops
from triplaneturbo_amd import isosurface as I

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_reference as MC  # noqa: E402  (mesh checks)
import mt_reference as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("sphere9", "jitter5", "zeros7")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_tets.npz")))


def test_entry_point_surface():
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_mt_")) == [
        "tt_mt_bwd", "tt_mt_count", "tt_mt_emit", "tt_mt_workspace_bytes"]
    assert "tt_tets.hip" in _lib.SOURCES
    assert _lib.TT_ABI_VERSION == 17


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)  # never dereferenced: validation fails first
    big = (1 << 28) + 1
    for ne, nt in ((0, 5), (5, 0), (-1, 5), (5, -1), (big, 5), (5, big)):
        assert lib.tt_mt_workspace_bytes(ne, nt) == -1
        assert lib.tt_mt_count(one, one, one, ne, nt, one, one, null) == -1
        assert lib.tt_mt_emit(one, one, one, one, ne, nt, one, one, one, null) == -1
        assert lib.tt_mt_bwd(one, one, one, one, one, 4, ne, nt, one, one, one, one, null) == -1
    # crossing flag + case byte + two int32 prefixes
    assert lib.tt_mt_workspace_bytes(1000, 700) >= 1000 + 700 + 4 * 1700
    assert lib.tt_mt_workspace_bytes(1 << 28, 1 << 28) > 0
    for k in range(5):  # level, edges, tets, workspace, totals
        args = [one, one, one, 9, 6, one, one]
        args[k if k < 3 else k + 2] = null
        assert lib.tt_mt_count(*args, null) == -1
    for k in range(7):  # pos, level, edges, tet_edge, workspace, v_pos, t_pos_idx
        args = [one, one, one, one, 9, 6, one, one, one]
        args[k if k < 4 else k + 2] = null
        assert lib.tt_mt_emit(*args, null) == -1
    for k in range(9):  # pos, level, edges, vert_ptr, vert_col, workspace, grad_v, grad_level, grad_pos
        args = [one, one, one, one, one, 4, 9, 6, one, one, one, one]
        args[k if k < 5 else k + 3] = null
        assert lib.tt_mt_bwd(*args, null) == -1
    for nv in (0, -3, big):
        assert lib.tt_mt_bwd(one, one, one, one, one, nv, 9, 6, one, one, one, one, null) == -1


def test_marching_tets_refuses_cpu_tensors():
    v, t = I.kuhn_tet_grid(3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.TetGrid(v, t)
    with pytest.raises(TypeError, match="TetGrid"):
        ops.marching_tets(v, torch.zeros(27), None)


@pytest.mark.parametrize("R", [2, 3, 6])
def test_kuhn_tet_grid(R):
    v, t = I.kuhn_tet_grid(R)
    assert v.dtype == torch.float32 and t.dtype == torch.int64
    assert torch.equal(v, I.DiffMarchingCubeHelper(R).grid_vertices)  # the marching-cubes grid, in its order
    assert t.shape == (6 * (R - 1) ** 3, 4) and t.min() == 0 and t.max() == R ** 3 - 1
    p = v.double()[t]
    det = torch.linalg.det(torch.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], p[:, 3] - p[:, 0]], dim=1))
    assert (det > 0).all()
    assert abs(det.sum().item() / 6 - 1.0) < 1e-12  # the tets tile the unit cube
    # conforming: every interior triangular face belongs to two tets, every boundary face to one
    faces = torch.sort(t[:, [[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]]].reshape(-1, 3), dim=1)[0]
    _, counts = torch.unique(faces, dim=0, return_counts=True)
    assert counts.max() == 2 and (counts == 1).sum() == 6 * 2 * (R - 1) ** 2


def test_surface_on_the_kuhn_grid_is_closed_and_faces_outward():
    """with the reference's triangle table, positively oriented tets give a closed, consistently oriented surface
    whose normals point toward level > 0"""
    v, t = I.kuhn_tet_grid(9)
    v = v.numpy()
    level = np.linalg.norm(v - 0.5, axis=1) - 0.33
    mt = M.marching_tets(v, level, t.numpy())
    assert len(mt.t_pos_idx) > 200
    assert MC.euler_characteristic(mt.v_pos, mt.t_pos_idx) == 2
    assert MC.unmatched_directed_edges(mt.t_pos_idx, len(mt.v_pos)) == []  # every edge once in each direction
    # outward = toward level > 0; the distance is convex along an edge, so every vertex lies inside the sphere
    ball = 4 / 3 * np.pi * 0.33 ** 3
    assert 0.85 * ball < MC.signed_volume(mt.v_pos, mt.t_pos_idx) < ball


@pytest.mark.parametrize("case", CASES)
def test_the_oracle_reproduces_the_reference_helper(golden, case):
    g = {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "_")}
    R = int(g["resolution"])
    tb = M.tet_tables(g["indices"], len(g["vertices"]))
    assert np.array_equal(tb.edges, g["all_edges"])
    assert np.array_equal(tb.edges[tb.tet_edge].reshape(-1, 12),
                          np.sort(g["indices"][:, M.BASE_EDGES].reshape(-1, 6, 2), axis=2).reshape(-1, 12))
    for v in range(0, len(g["vertices"]), 37):  # a CSR row = the edges that hold the vertex, ascending
        assert np.array_equal(tb.vert_col[tb.vert_ptr[v]:tb.vert_ptr[v + 1]], np.nonzero((tb.edges == v).any(1))[0])
    plain = M.marching_tets(g["vertices"], g["level"], g["indices"], tb)
    assert np.array_equal(plain.t_pos_idx, g["t_pos_idx"]) and plain.t_pos_idx.dtype == np.int32
    assert plain.v_pos.tobytes() == g["v_pos"].tobytes()  # bit for bit
    # the helper's deformation: range / resolution * tanh, in fp32
    grid = (torch.from_numpy(g["vertices"]) + 1.0 / R * torch.tanh(torch.from_numpy(g["deformation"]))).numpy()
    deformed = M.marching_tets(grid, g["level"], g["indices"], tb)
    assert np.array_equal(deformed.t_pos_idx, g["t_pos_idx_def"])
    assert deformed.v_pos.tobytes() == g["v_pos_def"].tobytes()
    # the gradient formulas of the contract are the reference's autograd
    g_level, g_pos = M.backward(plain, g["vertices"], g["level"], g["W"])
    assert np.abs(g_level - g["g64_level"][:, 0]).max() <= 1e-9 * np.abs(g_level).max()
    if case == "zeros7":
        assert (g["level"] == 0).sum() > 20  # exact zeros are unoccupied ends of crossing edges
    assert np.abs(g["level"][plain.a, 0] - g["level"][plain.b, 0]).min() >= 1e-3


def test_helper_attributes_without_a_gpu(tmp_path):
    h = I.MarchingTetrahedraHelper(6, point_range=(0, 1))
    v, t = I.kuhn_tet_grid(6)
    assert torch.equal(h.grid_vertices, v) and torch.equal(h.indices, t) and h.points_range == (0, 1)
    x = torch.randn(7, 3, requires_grad=True)
    n = h.normalize_grid_deformation(x)
    assert torch.equal(n, 1.0 / 6 * torch.tanh(x)) and n.requires_grad
    # the empty-field fix-up sets: on the lattice, the reference's (the two outer layers, the vertex (R//2,)*3)
    for R in (5, 6, 16):
        h = I.MarchingTetrahedraHelper(R)
        m = torch.zeros([R] * 3, dtype=torch.bool)
        for a in range(3):
            m.transpose(0, a)[:2] = True
            m.transpose(0, a)[-2:] = True
        assert torch.equal(h.border_indices, torch.nonzero(m.reshape(-1)))
        c = R // 2
        assert h.center_indices.tolist() == [[c * R * R + c * R + c]]
    # a file in the reference's format loads unchanged; a grid that is no lattice gets its sets by position
    I.write_tet_grid(str(tmp_path / "6_tets.npz"), 6)
    f = I.MarchingTetrahedraHelper(6, str(tmp_path / "6_tets.npz"))
    assert torch.equal(f.grid_vertices, v) and torch.equal(f.indices, t)
    keep = torch.arange(216) % 7 != 3  # drop vertices: Nv != R^3
    np.savez(tmp_path / "odd.npz", vertices=v[keep].numpy() * 2 - 1, indices=np.zeros((1, 4), dtype=np.int64))
    o = I.MarchingTetrahedraHelper(6, str(tmp_path / "odd.npz"))
    full = I.MarchingTetrahedraHelper(6)
    renumber = torch.cumsum(keep, 0) - 1
    want = renumber[full.border_indices[:, 0][keep[full.border_indices[:, 0]]]]
    assert torch.equal(o.border_indices[:, 0], want)
    centre = o.grid_vertices[o.center_indices[0, 0]]
    # the lattice's centre vertex (0.2, 0.2, 0.2) is among the dropped ones: a neighbour one cell (0.4) away stands in
    assert not keep[3 * 36 + 3 * 6 + 3] and (centre - 0.2).abs().sum() <= 0.4 + 1e-6


def test_renderer_mt_configuration(tmp_path):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    g = tt.find(t["geometry_type"])(t["geometry"])
    m = tt.find(t["material_type"])(t["material"])
    b = tt.find(t["background_type"])(t["background"])
    cfg = dict(s["renderer"], isosurface_method="mt", isosurface_resolution=8)
    with pytest.raises(NotImplementedError, match="tet_grid=.*load/tets/8_tets.npz|load/tets/8_tets.npz.*tet_grid="):
        tt.find(s["renderer_type"])(cfg, geometry=g, material=m, background=b)
    with pytest.raises(NotImplementedError, match="mc-cpu"):
        tt.find(s["renderer_type"])(dict(cfg, isosurface_method="mc-cpu"), geometry=g, material=m, background=b)
    I.write_tet_grid(str(tmp_path / "8_tets.npz"), 8)
    r = tt.find(s["renderer_type"])(cfg, geometry=g, material=m, background=b, tet_grid=tmp_path / "8_tets.npz")
    assert isinstance(r.isosurface_helper, I.MarchingTetrahedraHelper) and g.isosurface == r.isosurface
    d = tt.find(s["renderer_type"])(dict(cfg, isosurface_method="diffmc"), geometry=g, material=m, background=b)
    assert torch.equal(r.border_indices, d.border_indices) and torch.equal(r.center_indices, d.center_indices)
