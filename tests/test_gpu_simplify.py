"""HIP mesh simplification (tt_simplify_*; ops.mesh_simplify, Mesh.simplify, the exporter's simplify_grid) against the
contract's numpy restatement (tests/simplify_reference.py): faces, vertex_map and cluster count must be equal, positions
within 1e-3 h (the regularised 3x3 system has a condition number of at most 1 + 1/lam ~ 1e3, the fp32 sums carry ~1e-6
relative error, |x| <= h; measured on an MI355X: at most 2.0e-5 h on these cases, 4.4e-5 h on 160^3 meshes,
profiles/simplify.json).  Then determinism, the target_faces bisection, detached positions, and the exporter's bake and
files on the simplified mesh."""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, viewer
from triplaneturbo_amd.export import save_obj
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def reference(name, grid):
    return S.simplify(*S.source_mesh(name), grid)


def gpu_mesh(name, dev):
    v, tri = S.source_mesh(name)
    return Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(tri)).to(dev).int())


@pytest.mark.parametrize("name,grid", S.CASES)
def test_matches_the_restatement(dev, name, grid):
    mesh = gpu_mesh(name, dev)
    v_ref, t_ref, i_ref = reference(name, grid)
    v2, t2, info = ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, grid)
    assert t2.dtype == torch.int32 and v2.dtype == torch.float32 and info["vertex_map"].dtype == torch.int32
    assert info["grid"] == grid and info["cell"] == i_ref["cell"] and info["n_clusters"] == i_ref["n_clusters"]
    assert np.array_equal(info["vertex_map"].cpu().numpy(), i_ref["vertex_map"])
    assert np.array_equal(t2.cpu().numpy(), t_ref)
    assert tuple(v2.shape) == v_ref.shape
    dev_h = np.abs(v2.cpu().numpy().astype(np.float64) - v_ref.astype(np.float64)).max() / info["cell"]
    print(f"{name} G={grid}: V' {len(v_ref)} T' {len(t_ref)} clusters {info['n_clusters']} max |v' - ref| = {dev_h:.3e} h")
    assert dev_h <= 1e-3
    if name == "blobs32":
        assert info["n_clusters"] > v2.shape[0]
    if name == "dedupe":
        assert t2.tolist() == [[0, 2, 1], [0, 1, 2]]  # [[A,B,C],[A,C,B]] with ranks A = 0, C = 1, B = 2


def test_heightfield_crosses_the_scan_seam_in_both_counters(dev):
    """A 520 x 520 heightfield with unreferenced vertices spliced into the middle of the vertex array, grid 1024:
    309029 clusters of which 270400 are marked, 538722 kept faces.  Both counters exceed the 262144 items that one chunk
    of the block-total scan covers, and the cluster compaction is not the identity.  Faces, vertex_map and cluster
    count must equal the restatement's; positions are held to the contract's own bound (a mapped vertex and its output
    vertex share a cell: at most sqrt(3) h apart), the deviation from the restatement is printed."""
    import mesh_reference as M
    n = 520
    v, t = M.sheet(n)
    rng = np.random.default_rng(0)
    x, y = v[:, 0].reshape(n, n), v[:, 1].reshape(n, n)
    noise = rng.uniform(-0.3, 0.3, (n, n)).astype(np.float32)
    v[:, 2] = (np.float32(40) * np.sin(x / np.float32(23)) * np.cos(y / np.float32(17)) + noise).reshape(-1)
    loose = v[::7].copy()  # referenced by no face
    loose[:, 2] += 100
    mid = n * n // 2
    v = np.concatenate([v[:mid], loose, v[mid:]])
    t = np.where(t >= mid, t + len(loose), t).astype(np.int32)
    v_ref, t_ref, i_ref = S.simplify(v, t, 1024)
    assert i_ref["n_clusters"] == 309029 and int((i_ref["vertex_map"] == -1).sum()) == 38629
    assert v_ref.shape == (270400, 3) and t_ref.shape == (538722, 3)
    v2, t2, info = ops.mesh_simplify(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), 1024)
    assert info["n_clusters"] == i_ref["n_clusters"]
    vmap = info["vertex_map"].cpu().numpy()
    assert np.array_equal(vmap, i_ref["vertex_map"])
    assert np.array_equal(t2.cpu().numpy(), t_ref)
    assert tuple(v2.shape) == v_ref.shape
    got = v2.cpu().numpy().astype(np.float64)
    print(f"heightfield G=1024: max |v' - ref| = {np.abs(got - v_ref.astype(np.float64)).max() / info['cell']:.3e} h")
    mapped = vmap >= 0
    dist = np.linalg.norm(v[mapped].astype(np.float64) - got[vmap[mapped]], axis=1)
    print(f"heightfield G=1024: max |v - v'[vertex_map]| = {dist.max() / info['cell']:.4f} h")
    assert dist.max() <= np.sqrt(3.0) * info["cell"]


def test_two_calls_are_bit_identical(dev):
    mesh = gpu_mesh("sphere32", dev)
    a = ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, 8)
    b = ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, 8)
    assert a[1].shape[0] > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2]["vertex_map"], b[2]["vertex_map"])


def test_out_of_range_arguments_raise_before_gpu_work(dev):
    mesh = gpu_mesh("triangle", dev)
    for g in (1, 1025):
        with pytest.raises(ValueError):
            ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, g)
    with pytest.raises(ValueError):
        ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, 4, lam=-1.0)
    with pytest.raises(ValueError):
        ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx + 1, 4)  # an index outside [0, V)
    flat = Mesh(torch.zeros(3, 3, device=dev), mesh.t_pos_idx)
    assert flat.simplify(grid=4) is flat  # no extent


def test_target_faces_picks_the_largest_grid_that_fits(dev):
    mesh = gpu_mesh("sphere32", dev)
    mesh.add_extra("tag", 7)
    low = mesh.simplify(target_faces=300)
    assert 0 < low.t_pos_idx.shape[0] <= 300
    g = low.extras["simplify"]["grid"]
    assert low.extras["tag"] == 7 and "simplify" not in mesh.extras
    assert low.extras["simplify"]["cell"] > 0
    again = mesh.simplify(grid=g)
    assert torch.equal(low.v_pos, again.v_pos) and torch.equal(low.t_pos_idx, again.t_pos_idx)
    assert g == 256 or mesh.simplify(grid=g + 1).t_pos_idx.shape[0] > 300
    # a target below what grid 2 gives: the grid-2 result
    tiny = mesh.simplify(target_faces=1)
    assert tiny.extras["simplify"]["grid"] == 2
    assert torch.equal(tiny.t_pos_idx, mesh.simplify(grid=2).t_pos_idx)


def test_positions_that_require_grad_are_detached(dev):
    mesh = gpu_mesh("sphere24", dev)
    hot = Mesh(mesh.v_pos.clone().requires_grad_(True), mesh.t_pos_idx)
    a, b = hot.simplify(grid=8), mesh.simplify(grid=8)
    assert not a.requires_grad and not a.v_pos.requires_grad
    assert torch.equal(a.v_pos, b.v_pos) and torch.equal(a.t_pos_idx, b.t_pos_idx)


# ---- the exporter on the simplified mesh (the set-up of tests/test_gpu_export.py::_exporter_modules) ----
def _exporter_modules(dev, resolution=64):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    r = tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=resolution), geometry=g, material=m,
                                    background=b).to(dev)
    # a smooth scene: planes drawn at 8^2 and upsampled
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    return r, g, m, b, cache


@pytest.fixture(scope="module")
def modules(dev):
    return _exporter_modules(dev)


def _exporter(modules, cfg):
    r, g, m, b, cache = modules
    return tt.find("multiprompt-mesh-exporter")(cfg, geometry=g, material=m, background=b)


def test_exporter_bakes_the_simplified_mesh(modules, tmp_path):
    r, g, m, b, cache = modules
    N = 512
    cfg = {"save_uv": True, "texture_size": N, "texture_format": "png"}
    exp = _exporter(modules, cfg)
    assert exp.simplify_grid is None and exp.simplify_target_faces is None
    exp.simplify_grid = 24
    (out,) = exp(cache)
    mesh, kd = out.params["mesh"], out.params["map_Kd"]
    with torch.no_grad():
        full = r.isosurface(cache)[0]
    want = full.simplify(grid=24)
    assert torch.equal(mesh.v_pos, want.v_pos) and torch.equal(mesh.t_pos_idx, want.t_pos_idx)
    assert 0 < mesh.t_pos_idx.shape[0] < full.t_pos_idx.shape[0]
    assert mesh.extras["simplify"]["grid"] == 24
    assert kd.shape == (N, N, 3) and kd.min() >= 0 and kd.max() <= 1
    # bake: every covered texel = material.export(geometry.export(p)), p recomputed in torch from the UV triangle
    uv4 = torch.cat((mesh.v_tex * 2 - 1, torch.zeros_like(mesh.v_tex[:, :1]), torch.ones_like(mesh.v_tex[:, :1])), -1)
    rast = tt.raster.rasterize(uv4[None], mesh.t_tex_idx, N)[0]
    cov = rast[..., 3] > 0
    assert cov.any()
    tid = rast[..., 3][cov].long() - 1
    py, px = torch.nonzero(cov, as_tuple=True)
    c = torch.stack([(px.double() + 0.5) / N, (py.double() + 0.5) / N], -1)
    T3 = mesh.v_tex.double()[mesh.t_tex_idx.long()[tid]]
    d = (T3[:, 1, 0] - T3[:, 0, 0]) * (T3[:, 2, 1] - T3[:, 0, 1]) - (T3[:, 1, 1] - T3[:, 0, 1]) * (T3[:, 2, 0] - T3[:, 0, 0])
    b1 = ((c[:, 0] - T3[:, 0, 0]) * (T3[:, 2, 1] - T3[:, 0, 1]) - (c[:, 1] - T3[:, 0, 1]) * (T3[:, 2, 0] - T3[:, 0, 0])) / d
    b2 = ((T3[:, 1, 0] - T3[:, 0, 0]) * (c[:, 1] - T3[:, 0, 1]) - (T3[:, 1, 1] - T3[:, 0, 1]) * (c[:, 0] - T3[:, 0, 0])) / d
    P3 = mesh.v_pos.double()[mesh.t_pos_idx.long()[tid]]
    p = (1 - b1 - b2)[:, None] * P3[:, 0] + b1[:, None] * P3[:, 1] + b2[:, None] * P3[:, 2]
    with torch.no_grad():
        albedo = m.export(**g.export(points=p.float(), space_cache=cache[:1]))["albedo"]
    err = (kd[cov] - albedo).abs().max().item()
    print(f"bake on the simplified mesh: T {full.t_pos_idx.shape[0]} -> {mesh.t_pos_idx.shape[0]}, max error {err:.2e}")
    assert err <= 1e-5
    # files: the OBJ round-trips the face count through the viewer's loader
    paths = save_obj(str(tmp_path / out.save_name), **out.params)
    assert sorted(os.path.basename(x) for x in paths) == ["model.mtl", "model.obj", "texture_kd.png"]
    loaded, tex = viewer.load_obj(str(tmp_path / "model.obj"), device=mesh.v_pos.device)
    assert loaded.t_pos_idx.shape[0] == mesh.t_pos_idx.shape[0] and tex is not None
    # both attributes None: bit for bit the output of an untouched exporter
    exp.simplify_grid = None
    (plain,) = exp(cache)
    (fresh,) = _exporter(modules, cfg)(cache)
    for key in ("v_pos", "t_pos_idx", "v_tex", "t_tex_idx"):
        assert torch.equal(getattr(plain.params["mesh"], key), getattr(fresh.params["mesh"], key))
    assert torch.equal(plain.params["mesh"].t_pos_idx, full.t_pos_idx)
    assert torch.equal(plain.params["map_Kd"], fresh.params["map_Kd"])


def test_exporter_obj_format_colours_the_simplified_vertices(modules):
    r, g, m, b, cache = modules
    exp = _exporter(modules, {"fmt": "obj"})
    exp.simplify_grid = 24
    (out,) = exp(cache)
    mesh = out.params["mesh"]
    with torch.no_grad():
        want = r.isosurface(cache)[0].simplify(grid=24)
    assert out.params["save_vertex_color"] is True
    assert mesh.v_pos.shape == want.v_pos.shape and mesh.v_rgb.shape == mesh.v_pos.shape
    assert mesh.v_rgb.min() >= 0 and mesh.v_rgb.max() <= 1
