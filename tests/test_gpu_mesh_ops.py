"""The tt_mesh_* kernels behind Mesh.edges / normal_consistency() / laplacian() / remove_outlier() against the
reference's own Mesh (tests/golden/reference_mesh_ops.npz: edges, both losses and their gradients, computed in float64
by make_golden_mesh_ops.py) and the numpy oracle tests/mesh_reference.py.

remove_outlier has no golden: the reference runs it with trimesh, which is not available here.  Its oracle is the
contract of include/tt_abi.h ("mesh regularisers and outlier removal") as tests/mesh_reference.py implements it:
faces joined by an edge that exactly two face edges use, components with >= threshold faces kept, vertices and faces
in their original order."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, raster
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, Mesh, isosurface

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mc_reference as MC  # noqa: E402
import mesh_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = np.load(os.path.join(HERE, "golden", "reference_mesh_ops.npz"))
NAMES = sorted({k.rsplit("_v_pos", 1)[0] for k in GOLDEN.files if k.endswith("_v_pos")})
LOSSES = ("laplacian", "normal_consistency")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mesh(v, t, dev, grad=False, idx_dtype=torch.int32):
    vp = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(dev).requires_grad_(grad)
    return Mesh(vp, torch.from_numpy(np.asarray(t, dtype=np.int64)).to(dev, idx_dtype).reshape(-1, 3))


def _loss_and_grad(v, t, loss_name, dev):
    m = _mesh(v, t, dev, grad=True)
    loss = getattr(m, loss_name)()
    loss.backward()
    return loss.detach(), m.v_pos.grad


def _sphere16(dev):
    v, t = ops.marching_cubes(torch.from_numpy(M.sphere_field(16)).to(dev))
    return Mesh(v, t)


@pytest.mark.parametrize("which", ["hand", "sphere16"])
def test_topology_antialias_tables_are_edge_topology(dev, which):
    """Mesh.topology's antialias tables are raster.edge_topology's: values, dtype, shape and contiguity"""
    mesh = _mesh(*M.hand_mesh(), dev) if which == "hand" else _sphere16(dev)
    got = mesh.topology.antialias_tables
    want = raster.edge_topology(mesh.t_pos_idx.int(), mesh.v_pos.shape[0])
    assert want[0].shape[0] == 3 * mesh.t_pos_idx.shape[0] > 0
    for g, w in zip(got, want):
        assert torch.equal(g, w) and g.dtype == w.dtype == torch.int32
        assert g.is_contiguous() and w.is_contiguous()
    assert mesh.topology.antialias_tables is got  # derived once and kept


def test_one_face_edge_sort_serves_every_consumer(dev, monkeypatch):
    """torch.sort calls of a mesh that is rendered and regularised: the shared face-edge sort, and the neighbour
    CSR's once the Laplacian asks for it (three before the antialias tables moved into MeshTopology)"""
    mesh = _sphere16(dev)
    assert not mesh.requires_grad and mesh.t_pos_idx.shape[0] > 0
    calls = []
    real_sort = torch.sort

    def counting_sort(*args, **kwargs):
        calls.append(1)
        return real_sort(*args, **kwargs)

    monkeypatch.setattr(torch, "sort", counting_sort)
    mesh.topology.antialias_tables
    assert len(calls) == 1
    mesh.laplacian()
    assert len(calls) == 2
    mesh.normal_consistency()
    mesh.edges
    assert mesh.remove_outlier(0.01) is not mesh
    mesh.topology.antialias_tables
    assert len(calls) == 2


@pytest.mark.parametrize("name", NAMES)
def test_edges_match_the_reference(dev, name):
    v, t = GOLDEN[f"{name}_v_pos"], GOLDEN[f"{name}_t_pos_idx"]
    want = GOLDEN[f"{name}_edges"]
    assert np.array_equal(want, M.edges(t))
    for dt in (torch.int32, torch.int64):
        e = _mesh(v, t, dev, idx_dtype=dt).edges
        assert e.dtype == dt and np.array_equal(e.cpu().numpy(), want)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("loss_name", LOSSES)
def test_losses_and_gradients_match_the_reference(dev, name, loss_name):
    v, t = GOLDEN[f"{name}_v_pos"], GOLDEN[f"{name}_t_pos_idx"]
    loss, grad = _loss_and_grad(v, t, loss_name, dev)
    want, want_g = float(GOLDEN[f"{name}_{loss_name}"]), GOLDEN[f"{name}_{loss_name}_grad"]
    o_loss, o_grad = (M.laplacian if loss_name == "laplacian" else M.normal_consistency)(v, t)
    for ref, ref_g in ((want, want_g), (o_loss, o_grad)):
        assert abs(loss.item() - ref) <= 1e-5 * abs(ref), (loss.item(), ref)
        err = np.abs(grad.cpu().numpy().astype(np.float64) - ref_g).max()
        assert err <= 1e-4 * np.abs(ref_g).max(), (err, np.abs(ref_g).max())


@pytest.mark.parametrize("loss_name", LOSSES)
def test_loss_gradient_against_the_normals_oracle(dev, loss_name):
    """the HIP backward w.r.t. v_nrm alone (normal consistency) / v_pos (Laplacian) against float64"""
    v, t = GOLDEN["blobs33_v_pos"], GOLDEN["blobs33_t_pos_idx"]
    m = _mesh(v, t, dev)
    x = (m.v_nrm if loss_name == "normal_consistency" else m.v_pos).detach().clone().requires_grad_(True)
    fn = ops.mesh_normal_consistency_loss if loss_name == "normal_consistency" else ops.mesh_laplacian_loss
    (fn(x, m.topology) * 3.0).backward()
    x64 = x.detach().cpu().numpy()
    _, want = (M.normal_consistency_of_normals if loss_name == "normal_consistency" else M.laplacian)(x64, t)
    assert np.abs(x.grad.cpu().numpy() - 3.0 * want).max() <= 1e-4 * np.abs(3.0 * want).max()


@pytest.mark.parametrize("loss_name", LOSSES)
def test_launches_are_bit_identical(dev, loss_name):
    """the HIP forward and backward on a fixed input (v_pos for the Laplacian, v_nrm for normal consistency).  The
    vertex normals themselves come from Mesh._compute_vertex_normal, whose torch scatter_add_ is not bit-reproducible
    on the GPU, so the normal-consistency gradient w.r.t. v_pos is only as repeatable as that."""
    v, t = GOLDEN["blobs33_v_pos"], GOLDEN["blobs33_t_pos_idx"]
    m = _mesh(v, t, dev)
    x0 = (m.v_nrm if loss_name == "normal_consistency" else m.v_pos).detach().clone()
    fn = ops.mesh_normal_consistency_loss if loss_name == "normal_consistency" else ops.mesh_laplacian_loss
    runs = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        loss = fn(x, m.topology)
        loss.backward()
        runs.append((loss.detach(), x.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_empty_and_faceless_losses_follow_torch_mean(dev):
    m = _mesh(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int64), dev, grad=True)
    assert m.edges.shape == (0, 2)
    lap = m.laplacian()
    assert lap.item() == 0.0  # every r_i = 0, V = 3
    lap.backward()
    assert torch.equal(m.v_pos.grad, torch.zeros_like(m.v_pos))
    assert torch.isnan(ops.mesh_normal_consistency_loss(m.v_nrm.detach(), m.topology))  # mean over no edges


def _check_remove(v, t, thr, dev, idx_dtype=torch.int32):
    m = _mesh(v, t, dev, idx_dtype=idx_dtype)
    m.add_extra("tag", 5)
    out = m.remove_outlier(thr)
    want_v, want_t = M.remove_small_components(v, t, thr)
    assert out is not m and out.extras == {"tag": 5}
    assert out.t_pos_idx.dtype == idx_dtype and out.v_pos.dtype == torch.float32
    assert np.array_equal(out.v_pos.cpu().numpy(), want_v)
    assert np.array_equal(out.t_pos_idx.cpu().numpy(), np.asarray(want_t).reshape(-1, 3))
    return out


@pytest.fixture(scope="module")
def blobs():
    mc = MC.marching_cubes(M.blobs_field(48))
    return mc.v_pos, mc.t_pos_idx.astype(np.int64)


def test_components_match_the_oracle(dev, blobs):
    v, t = blobs
    m = _mesh(v, t, dev)
    labels = ops.mesh_face_components(m.topology).cpu().numpy()
    want = M.face_components(t)
    assert np.array_equal(labels, want)
    assert len(np.unique(want)) == 5


def test_remove_outlier_matches_the_oracle(dev, blobs):
    v, t = blobs
    sizes = np.sort(np.bincount(M.face_components(t)))[::-1]
    sizes = sizes[sizes > 0]
    n_all = len(t)
    out = _check_remove(v, t, 0.1, dev)  # the two spheres stay, the blobs go
    assert 0 < out.t_pos_idx.shape[0] < n_all
    _check_remove(v, t, int(sizes[2]) + 1, dev, idx_dtype=torch.int64)  # int threshold
    out = _check_remove(v, t, 0, dev)  # keeps everything
    assert out.t_pos_idx.shape[0] == n_all and out.v_pos.shape[0] == len(v)
    out = _check_remove(v, t, 1.0, dev)  # only the largest
    assert out.t_pos_idx.shape[0] == sizes[0]
    out = _check_remove(v, t, int(sizes[0]) + 1, dev)  # nothing
    assert out.t_pos_idx.shape == (0, 3) and out.v_pos.shape == (0, 3)


@pytest.mark.parametrize("thr", [1, 2, 3, 0.75, 0.5, 0.0])
def test_remove_outlier_on_the_non_manifold_hand_mesh(dev, thr):
    v, t = M.hand_mesh()
    _check_remove(v, t, thr, dev)


def test_remove_outlier_edge_cases(dev):
    empty = _mesh(np.zeros((4, 3), np.float32), np.zeros((0, 3), np.int64), dev)
    assert empty.remove_outlier(0.01) is empty
    v, t = M.hand_mesh()
    m = _mesh(v, t, dev, grad=True)
    assert m.remove_outlier(0.5) is m


def test_remove_outlier_of_a_cut_sheet_crosses_the_scan_seam_in_both_counters(dev):
    """520 x 520 sheet without the faces of cell row 3: components of 3114 and 534570 faces.  remove_outlier(0.5) drops
    the small one, which sits first, so every surviving id shifts; V' = 268320 and T' = 534570 both exceed the 262144
    items (1024 blocks of 256) that one chunk of the block-total scan covers."""
    n = 520
    v, t = M.sheet(n)
    t = t[t.min(1) // n != 3]
    out = _check_remove(v, t, 0.5, dev)
    assert tuple(out.v_pos.shape) == (268320, 3) and tuple(out.t_pos_idx.shape) == (534570, 3)


def _mesh_renderer(dev):
    s = json.load(open(os.path.join(HERE, "golden", "reference_mesh_renderer_config.json")))
    tc = json.load(open(os.path.join(HERE, "golden", "reference_training_config.json")))
    g = tt.find(tc["geometry_type"])(tc["geometry"]).to(dev)
    m = tt.find(tc["material_type"])(tc["material"]).to(dev)
    b = tt.find(tc["background_type"])(tc["background"]).to(dev)
    r = tt.find(s["renderer_type"])(s["renderer"], geometry=g, material=m, background=b).to(dev)
    return r


def test_regularisers_through_the_mesh_renderer(dev):
    from test_gpu_mesh_renderer import _cameras
    P, n_view, H, W = 2, 2, 64, 64
    torch.manual_seed(0)
    r = _mesh_renderer(dev)
    assert r.cfg.isosurface_resolution == 128
    r.train()
    r.update_step(0, 100)
    cam = _cameras(P * n_view, H, W, dev)
    cache = (torch.randn(P, 6, 32, 64, 64, device=dev) * 0.3).requires_grad_(True)
    out = r(cam["mvp_mtx"], cam["camera_positions"], cam["light_positions"], H, W, space_cache=cache,
            text_embed=torch.randn(P, 1024, device=dev), rays_d_rasterize=cam["rays_d_rasterize"],
            camera_distances=cam["camera_distances"], c2w=cam["c2w"])
    # the reference system's loop (multiprompt_dual_renderer_multistep_generator.py:716-757)
    loss = 0.0
    for mesh in out["mesh"]:
        assert mesh.requires_grad and mesh.t_pos_idx.shape[0] > 0
        loss += mesh.normal_consistency() + mesh.laplacian()
    assert torch.isfinite(loss)
    loss.backward()
    assert cache.grad is not None and torch.isfinite(cache.grad).all() and cache.grad.abs().sum() > 0
    with torch.no_grad():
        meshes = r.isosurface(cache)
    for mesh in meshes:
        assert not mesh.requires_grad
        clean = mesh.remove_outlier(0.01)
        v, t = mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy()
        want_v, want_t = M.remove_small_components(v, t, 0.01)
        cv, ct = clean.v_pos.cpu().numpy(), clean.t_pos_idx.cpu().numpy()
        assert np.array_equal(cv, want_v) and np.array_equal(ct, want_t)
        assert ct.size == 0 or (ct.min() >= 0 and ct.max() < len(cv))
        faces_in = {tuple(map(tuple, f)) for f in v[t].tolist()}
        assert all(tuple(map(tuple, f)) in faces_in for f in cv[ct].tolist())  # a subset of the input's faces


def test_remove_outlier_160_through_isosurface(dev):
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    with torch.no_grad():
        (mesh,) = isosurface(cache, g.forward_field, helper)
    v, t = mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy()
    labels = ops.mesh_face_components(mesh.topology).cpu().numpy()
    assert np.array_equal(labels, M.face_components(t))
    for thr in (0.01, 0.5):
        clean = mesh.remove_outlier(thr)
        want_v, want_t = M.remove_small_components(v, t, thr)
        assert np.array_equal(clean.v_pos.cpu().numpy(), want_v)
        assert np.array_equal(clean.t_pos_idx.cpu().numpy(), want_t)


def _csr_by_loop(pairs, n_rows):
    rows = [[] for _ in range(n_rows)]
    for r, c in pairs:
        rows[r].append(c)
    ptr = np.cumsum([0] + [len(r) for r in rows]).tolist()
    return ptr, [c for r in rows for c in sorted(r)]


def test_shared_csr_builder_and_validators_on_the_smallest_meshes(dev):
    """ops._csr behind MeshTopology.nbr_*, TetGrid.vert_* and mesh_tangents' group -> corner table, and the shared index
    checks, at the smallest shapes that reach every branch: a tetrahedron, the same with a degenerate face (a self
    pair), the R = 3 Kuhn lattice and a two-triangle quad cut along its diagonal in UV space."""
    from triplaneturbo_amd.isosurface import kuhn_tet_grid
    tet = torch.tensor([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
    for tri in (tet, torch.cat([tet, torch.tensor([[0, 0, 1]])])):
        a, b = ops.MeshTopology(tri.to(dev, torch.int32), 4), ops.MeshTopology(tri.to(dev), 4)
        edges = a.edges.cpu().tolist()
        assert ([0, 0] in edges) == (len(tri) == 5) and b.edges.dtype == torch.int64
        want = _csr_by_loop(edges + [e[::-1] for e in edges], 4)
        for topo in (a, b):
            assert topo.nbr_ptr.dtype == topo.nbr_col.dtype == torch.int32
            assert (topo.nbr_ptr.tolist(), topo.nbr_col.tolist()) == want
    v, t = kuhn_tet_grid(3)
    grid = ops.TetGrid(v.to(dev), t.to(dev))
    edges = grid.edges.cpu().tolist()
    want = _csr_by_loop([(a_, e) for e, (a_, _) in enumerate(edges)] + [(b_, e) for e, (_, b_) in enumerate(edges)], 27)
    assert (grid.vert_ptr.tolist(), grid.vert_col.tolist()) == want and grid.vert_col.dtype == torch.int32
    assert torch.equal(ops.TetGrid(v.to(dev), t.to(dev, torch.int32)).vert_col, grid.vert_col)

    v_pos = torch.tensor([[0., 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], device=dev)
    v_nrm = torch.tensor([[0., 0, 1]], device=dev).repeat(4, 1)
    quad = torch.tensor([[0, 1, 2], [0, 2, 3]], device=dev, dtype=torch.int32)
    v_tex = torch.tensor([[0., 0], [.4, 0], [.4, .4], [.5, .1], [.9, .5], [.5, .5]], device=dev)  # Vt = 6: a seam
    t_tex = torch.tensor([[0, 1, 2], [3, 4, 5]], device=dev)
    got = ops.mesh_tangents(v_pos, quad, v_tex, t_tex, v_nrm, group="tex")
    key = t_tex.reshape(-1).long()  # the table as it was built before ops._csr: a stable sort by the row alone
    corner = torch.sort(key, stable=True)[1].int().contiguous()
    ptr = torch.zeros(7, device=dev, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(key, minlength=6), 0)
    want = torch.empty_like(got)
    ops._launch("tt_bake_tangents", v_pos, quad, v_tex, t_tex.int(), v_nrm, ptr.int(), corner, 4, 6, 2,
                ops._BAKE_GROUPS["tex"], want)
    assert got.shape == (6, 3) and torch.equal(got, want) and torch.isfinite(got).all()
    assert torch.equal(got, ops.mesh_tangents(v_pos, quad.long(), v_tex, t_tex.int(), v_nrm, group="tex"))

    rast, field = torch.zeros(2, 2, 4, device=dev), torch.zeros(2, 2, 3, device=dev)
    users = {"MeshTopology": lambda x: ops.MeshTopology(x, 4), "mesh_simplify": lambda x: ops.mesh_simplify(v_pos, x, 4),
             "mesh_tangents": lambda x: ops.mesh_tangents(v_pos, x, v_tex, t_tex, v_nrm),
             "bake_encode": lambda x: ops.bake_encode(rast, v_nrm, x, got, t_tex, field)}
    for name, fn in users.items():
        for bad in (quad.short(), quad.float(), quad[:, :2], quad.reshape(-1)):
            with pytest.raises(TypeError, match="int32 / int64"):
                fn(bad)
        if name != "bake_encode":  # (its kernel reads the ids of covered texels only: no range check, as before)
            for bad in (quad + 2, quad - 1):
                with pytest.raises(ValueError, match="outside"):
                    fn(bad)
    for bad in (t.to(dev, torch.int16), t.to(dev).float(), t.to(dev)[:, :3]):
        with pytest.raises(TypeError, match="int32 / int64"):
            ops.TetGrid(v.to(dev), bad)
    with pytest.raises(ValueError, match="outside"):
        ops.TetGrid(v.to(dev)[:-1], t.to(dev))
