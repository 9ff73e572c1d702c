"""Mesh simplification without a GPU: the library's surface (sources, symbols, ABI version), the argument checks of
Mesh.simplify, and the invariants of the contract's numpy restatement (tests/simplify_reference.py) on marching-cubes
meshes: Euler characteristic, closedness, orientation, the face reduction, the sqrt(3) h bound, and the dedupe rule on
a hand-built case."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_reference as MC  # noqa: E402
import mesh_reference as M  # noqa: E402
import simplify_reference as S  # noqa: E402

ENTRY_POINTS = ["tt_simplify_workspace_bytes", "tt_simplify_keys", "tt_simplify_ranks", "tt_simplify_pairs",
                "tt_simplify_solve", "tt_simplify_faces", "tt_simplify_emit_count", "tt_simplify_emit"]


def test_library_surface():
    assert "tt_simplify.hip" in _lib.SOURCES
    for name in ENTRY_POINTS:
        assert name in _lib.SYMBOLS
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_simplify_")) == sorted(ENTRY_POINTS)
    assert _lib._expected_abi() == 17
    assert (_lib.TT_SIMPLIFY_MIN_GRID, _lib.TT_SIMPLIFY_MAX_GRID) == (2, 1024)
    assert _lib.TT_SIMPLIFY_MAX_CLUSTERS == S.MAX_CLUSTERS == 2 ** 21 - 1


def _cpu_mesh():
    v, tri = S.single_triangle()
    return Mesh(torch.from_numpy(v), torch.from_numpy(tri))


def test_simplify_argument_errors_need_no_gpu():
    mesh = _cpu_mesh()
    with pytest.raises(ValueError):
        mesh.simplify()
    with pytest.raises(ValueError):
        mesh.simplify(grid=8, target_faces=100)
    with pytest.raises(ValueError):
        mesh.simplify(grid=1)
    with pytest.raises(ValueError):
        mesh.simplify(grid=1025)
    with pytest.raises(ValueError):
        mesh.simplify(target_faces=0)


def test_empty_mesh_comes_back_as_itself():
    for v, t in ((torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)),
                 (torch.rand(5, 3), torch.zeros(0, 3, dtype=torch.int32))):
        mesh = Mesh(v, t)
        assert mesh.simplify(grid=4) is mesh
        assert mesh.simplify(target_faces=10) is mesh


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name, level in (("sphere24", M.sphere_field(24)), ("torus32", M.torus_field(32)),
                        ("blobs32", M.blobs_field(32))):
        mc = MC.marching_cubes(level)
        out[name] = (mc.v_pos * 2 - 1, mc.t_pos_idx)
    return out


CASES = [("sphere24", 4), ("sphere24", 8), ("sphere24", 12), ("torus32", 12), ("torus32", 16), ("blobs32", 8)]


@pytest.fixture(scope="module")
def results(meshes):
    return {(name, g): S.simplify(*meshes[name], g) for name, g in CASES}


@pytest.mark.parametrize("name,grid", [c for c in CASES if c[0] != "blobs32"])
def test_topology_is_preserved(meshes, results, name, grid):
    v, tri = meshes[name]
    v2, t2, info = results[(name, grid)]
    assert MC.euler_characteristic(v2, t2) == (2 if name == "sphere24" else 0)
    assert MC.unmatched_directed_edges(t2, len(v2)) == []
    assert len(t2) <= (0.65 if name == "sphere24" else 0.4) * len(tri)
    assert t2.dtype == np.int32 and v2.dtype == np.float32
    assert sorted(set(t2.reshape(-1).tolist())) == list(range(len(v2)))  # dense: every output vertex is referenced
    if name == "sphere24":  # every face outward with respect to the sphere's centre (0 after the map to [-1, 1])
        p = v2.astype(np.float64)[t2]
        n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        assert ((n * p.mean(1)).sum(1) > 0).all()


@pytest.mark.parametrize("name,grid", CASES)
def test_vertices_stay_in_their_cells(meshes, results, name, grid):
    v, tri = meshes[name]
    v2, t2, info = results[(name, grid)]
    h, vmap = info["cell"], info["vertex_map"]
    kept = vmap >= 0
    moved = np.linalg.norm(v2.astype(np.float64)[vmap[kept]] - v.astype(np.float64)[kept], axis=1)
    print(f"{name} G={grid}: V {len(v)} -> {len(v2)}, T {len(tri)} -> {len(t2)}, max move {moved.max() / h:.3f} h")
    assert moved.max() <= np.sqrt(3.0) * h
    off = np.abs(v2.astype(np.float64) - info["centre"].astype(np.float64))
    assert off.max() <= 0.5 * h * (1 + 1e-6)  # float32 rounding of centre + x
    if name == "blobs32":  # clusters that lose every face: the vertex compaction is not the identity
        assert info["n_clusters"] > len(v2) and (~kept).any()


def test_dedupe_keeps_the_first_of_equal_rotated_triples_and_both_orientations():
    v, tri = S.dedupe_case()
    v2, t2, info = S.simplify(v, tri, 3)
    assert info["cell"] == 1.0 and info["n_clusters"] == 4
    rank = info["rank"]
    A, B, C = rank[0], rank[2], rank[4]
    assert (rank[1], rank[3], rank[5], rank[6]) == (A, B, C, A) and A < C < B
    assert t2.tolist() == [[A, B, C], [A, C, B]]  # the corner cluster (3,3,3) is the last rank: no renumbering shift
    assert info["vertex_map"].tolist() == [A, A, B, B, C, C, A, -1]


def test_single_triangle_and_flat_mesh():
    v, tri = S.single_triangle()
    v2, t2, info = S.simplify(v, tri, 2)
    assert t2.tolist() == [[0, 2, 1]] and len(v2) == 3  # ranks follow the cell keys: (0,1,0) before (1,0,0)
    same = S.simplify(np.zeros((3, 3), np.float32), tri, 4)  # no extent: the mesh as it is
    assert same[2]["unchanged"] and same[1].tolist() == tri.tolist()
