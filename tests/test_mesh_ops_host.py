"""Mesh regularisers and outlier removal without a GPU: the numpy oracle (tests/mesh_reference.py) against the
reference's own Mesh (tests/golden/reference_mesh_ops.npz, make_golden_mesh_ops.py), the C ABI's argument checks,
the ops' refusal of CPU tensors, the threestudio Mesh API's names and signatures, and the tables of the shared
face-edge sort (ops.sort_face_edges) against plain-Python grouping."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops, raster
from triplaneturbo_amd import isosurface as I

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mesh_reference as M  # noqa: E402
import uv_reference as U  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "reference_mesh_ops.npz"))
NAMES = sorted({k.rsplit("_v_pos", 1)[0] for k in GOLDEN.files if k.endswith("_v_pos")})


def test_golden_holds_the_expected_meshes():
    assert NAMES == ["blobs33", "hand", "sphere17", "torus24"]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_the_reference_mesh(name):
    v, t = GOLDEN[f"{name}_v_pos"], GOLDEN[f"{name}_t_pos_idx"]
    assert np.array_equal(M.edges(t), GOLDEN[f"{name}_edges"])
    for loss_name, fn in (("laplacian", M.laplacian), ("normal_consistency", M.normal_consistency)):
        loss, grad = fn(v, t)
        want, want_g = float(GOLDEN[f"{name}_{loss_name}"]), GOLDEN[f"{name}_{loss_name}_grad"]
        assert abs(loss - want) <= 1e-6 * abs(want), (loss_name, loss, want)
        assert np.abs(grad - want_g).max() <= 1e-6 * np.abs(want_g).max(), loss_name


def test_oracle_components_of_the_hand_mesh():
    v, t = M.hand_mesh()
    assert M.face_components(t).tolist() == [0, 0, 0, 0, 4, 4, 6, 7, 7]
    v2, t2 = M.remove_small_components(v, t, 2)  # drops the lone degenerate face 6 and the unreferenced vertex 10
    assert t2.tolist() == t[[0, 1, 2, 3, 4, 5, 7, 8]].tolist() and np.array_equal(v2, v[:10])
    v4, t4 = M.remove_small_components(v, t, 3)  # the tetrahedron and its vertices 0-3 only
    assert t4.tolist() == t[:4].tolist() and np.array_equal(v4, v[:4])
    v3, t3 = M.remove_small_components(v, t, 0.75)  # int(4 * 0.75) = 3: the tetrahedron alone
    assert t3.tolist() == t[:4].tolist() and np.array_equal(v3, v[:4])


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)  # never dereferenced: validation fails first
    big = (1 << 28) + 1
    assert lib.tt_mesh_workspace_bytes(-1, 4) == -1
    assert lib.tt_mesh_workspace_bytes(4, -1) == -1
    assert lib.tt_mesh_workspace_bytes(big, 4) == -1
    assert lib.tt_mesh_workspace_bytes(0, 0) >= 0
    assert lib.tt_mesh_workspace_bytes(1000, 2000) >= 4 * 2000 * 2 + 12 * 1000
    assert lib.tt_mesh_components(null, 5, 4, one, one, null) == -1  # pairs missing
    assert lib.tt_mesh_components(one, 5, 4, null, one, null) == -1  # workspace missing
    assert lib.tt_mesh_components(one, 5, 4, one, null, null) == -1  # labels missing
    assert lib.tt_mesh_components(one, -1, 4, one, one, null) == -1
    assert lib.tt_mesh_components(null, 0, 0, one, null, null) == 0  # no faces: nothing to do, no launch
    assert lib.tt_mesh_compact_count(one, one, 4, 0, 0, 0.0, 1, one, one, null) == -1  # T = 0
    assert lib.tt_mesh_compact_count(null, one, 4, 2, 0, 0.0, 1, one, one, null) == -1
    assert lib.tt_mesh_compact_count(one, one, 4, 2, 2, 0.0, 1, one, one, null) == -1  # unknown mode
    assert lib.tt_mesh_compact_count(one, one, 4, 2, 1, float("nan"), 0, one, one, null) == -1
    assert lib.tt_mesh_compact_count(one, one, 4, 2, 0, 0.0, 1, one, null, null) == -1
    assert lib.tt_mesh_compact_emit(one, one, 4, 2, one, one, null, null) == -1
    assert lib.tt_mesh_compact_emit(null, one, 4, 2, one, one, one, null) == -1
    assert lib.tt_mesh_laplacian_fwd(one, null, one, 4, 2, one, one, null) == -1
    assert lib.tt_mesh_laplacian_fwd(one, one, one, 4, 2, one, null, null) == -1
    assert lib.tt_mesh_laplacian_bwd(one, one, one, 4, 2, null, one, one, null) == -1
    assert lib.tt_mesh_laplacian_bwd(one, one, one, 4, 2, one, one, null, null) == -1
    assert lib.tt_mesh_nc_fwd(one, one, 4, 2, 7, one, one, null) == -1  # E > 3T
    assert lib.tt_mesh_nc_fwd(one, null, 4, 2, 6, one, one, null) == -1
    assert lib.tt_mesh_nc_bwd(one, one, one, 4, 6, null, one, null) == -1
    assert lib.tt_mesh_nc_bwd(one, null, one, 4, 6, one, one, null) == -1  # nbr_ptr missing
    assert lib.tt_mesh_nc_bwd(null, one, null, 4, 6, one, one, null) == -1  # v_nrm missing
    assert lib.tt_mesh_laplacian_bwd(null, null, null, 0, 0, one, one, null, null) == 0  # V = 0: nothing to do
    assert lib.tt_mesh_nc_bwd(null, null, null, 0, 0, one, null, null) == 0


def test_ops_refuse_cpu_tensors():
    v = torch.zeros(4, 3)
    t = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mesh_topology(t, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        I.Mesh(v, t).laplacian()
    with pytest.raises(RuntimeError, match="no CPU path"):
        I.Mesh(v, t).edges
    with pytest.raises(RuntimeError, match="no CPU path"):
        I.Mesh(v, t).remove_outlier(0.5)


def _random_tri(n_vert, n_tri, seed):
    return torch.randint(0, n_vert, (n_tri, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


@pytest.mark.parametrize("tri, n_vert", [(torch.from_numpy(M.hand_mesh()[1]), 11), (_random_tri(5, 40, 0), 5),
                                         (_random_tri(5, 40, 1), 5), (_random_tri(7, 5, 2), 7),
                                         (_random_tri(7, 5, 3), 7)])
def test_shared_sort_groups_the_face_edges_like_a_dictionary(tri, n_vert):
    T = tri.shape[0]
    groups = {}  # unordered vertex pair -> its face edges 3f + k, ascending
    for fe in range(3 * T):
        a, b = int(tri[fe // 3, fe % 3]), int(tri[fe // 3, (fe % 3 + 1) % 3])
        groups.setdefault((min(a, b), max(a, b)), []).append(fe)
    srt = ops.sort_face_edges(tri, n_vert)
    edge_ofs, edge_tri = srt.antialias_tables()
    assert edge_ofs.dtype == edge_tri.dtype == torch.int32
    assert tuple(edge_ofs.shape) == (3 * T, 2) and tuple(edge_tri.shape) == (3 * T,)
    for pair, members in groups.items():
        firsts = {int(edge_ofs[fe, 0]) for fe in members}
        assert len(firsts) == 1, pair  # one group per pair ...
        first = firsts.pop()
        assert all(int(edge_ofs[fe, 1]) == len(members) for fe in members), pair  # ... of the right size ...
        # ... that lists the triangles of exactly these face edges, in ascending face-edge order (stable sort)
        assert edge_tri[first:first + len(members)].tolist() == [fe // 3 for fe in members], pair
    assert len({int(edge_ofs[m[0], 0]) for m in groups.values()}) == len(groups)  # distinct pairs, distinct groups
    assert srt.edges().tolist() == sorted(map(list, groups))
    for got, want in zip(raster.edge_topology(tri, n_vert), (edge_ofs, edge_tri)):
        assert torch.equal(got, want)


def test_shared_sort_gives_the_hand_mesh_its_edges_and_face_pairs():
    tri = M.hand_mesh()[1]
    srt = ops.sort_face_edges(torch.from_numpy(tri), 11)
    assert np.array_equal(srt.edges().numpy(), M.edges(tri))
    pairs = srt.face_pairs()
    assert pairs.dtype == torch.int32 and np.array_equal(pairs.numpy(), U.face_pairs(tri))
    # five tetrahedron edges (its sixth, (1,2), has three users), (2,4) of the strip 4-5 and (7,8) of the strip 7-8;
    # (6,7) has three users too: twice the degenerate face 6, once face 7
    assert len(pairs) == 7


def test_mesh_has_the_threestudio_api():
    sig = {n: list(inspect.signature(getattr(I.Mesh, n)).parameters) for n in
           ("normal_consistency", "laplacian", "remove_outlier", "set_vertex_color")}
    assert sig == {"normal_consistency": ["self"], "laplacian": ["self"],
                   "remove_outlier": ["self", "outlier_n_faces_threshold"], "set_vertex_color": ["self", "v_rgb"]}
    for prop in ("requires_grad", "edges", "v_nrm", "v_rgb"):
        assert isinstance(inspect.getattr_static(I.Mesh, prop), property), prop


def test_requires_grad_and_vertex_colour_need_no_gpu():
    v = torch.zeros(4, 3, requires_grad=True)
    t = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    m = I.Mesh(v, t, note=1)
    assert m.requires_grad
    assert m.remove_outlier(0.5) is m  # differentiable: returned unchanged before any GPU work
    rgb = torch.ones(4, 3)
    m.set_vertex_color(rgb)
    assert m.v_rgb is rgb
    with pytest.raises(AssertionError):
        m.set_vertex_color(torch.ones(3, 3))
    empty = I.Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32))
    assert empty.remove_outlier(0.01) is empty
