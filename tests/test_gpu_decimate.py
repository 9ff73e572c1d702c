"""HIP mesh decimation (tt_decimate_*; ops.mesh_decimate, Mesh.decimate, the exporter's decimate_target_faces) against
the contract's numpy restatement and trace checker (tests/decimate_reference.py): every collapse the GPU applied must be
valid by the restated rules, the collapses of a round must have disjoint closed neighbourhoods, points and costs must
agree with the restatement (1e-5 x the bounding-box diagonal; rel 1e-3 + 1e-12 diag^2), and replaying the trace must
reproduce vertices, faces and vertex_map exactly.  Then topology (edge-face counts, Euler characteristic, components),
locked vertices, the compaction's second-level seam, determinism, argument errors and the exporter."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def run(dev, v, t, target, **kw):
    """ops.mesh_decimate with a trace on numpy input: (v', t', vertex_map, info, trace), all numpy."""
    v2, t2, info = ops.mesh_decimate(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), target,
                                     return_trace=True, **kw)
    assert v2.dtype == torch.float32 and t2.dtype == torch.int32 and info["vertex_map"].dtype == torch.int32
    assert info["target_faces"] == target and len(info["trace"]) == info["n_rounds"]
    trace = [tuple(x.cpu().numpy() for x in r) for r in info["trace"]]
    assert all(e.dtype == np.int32 and x.dtype == np.float32 for e, x, _ in trace)
    return v2.cpu().numpy(), t2.cpu().numpy(), info["vertex_map"].cpu().numpy(), info, trace


def test_icosphere_keeps_the_sphere(dev):
    v, t = R.icosphere(3)
    assert len(t) == 1280
    v2, t2, vm, info, trace = run(dev, v, t, 200)
    R.check_trace(v, t, trace, 200, final=(v2, t2, vm))
    print(f"icosphere 1280 -> {len(t2)} in {info['n_rounds']} rounds")
    assert R.manifold_stats(t2) == (True, 2, 1)
    assert 199 <= len(t2) <= 200 and not info["stalled"] and not info["unchanged"] and info["n_locked"] == 0
    assert vm.min() >= 0 and set(vm.tolist()) == set(range(len(v2)))


def test_torus_keeps_its_handle_and_selection_stays_parallel(dev):
    v, t = R.torus(32, 16)
    assert len(t) == 1024
    v2, t2, vm, info, trace = run(dev, v, t, 128)
    R.check_trace(v, t, trace, 128, final=(v2, t2, vm))
    print(f"torus 1024 -> {len(t2)} in {info['n_rounds']} rounds")
    assert R.manifold_stats(t2) == (True, 0, 1)
    assert 127 <= len(t2) <= 128
    assert info["n_rounds"] <= 128


def test_noisy_sphere_flips_no_face(dev):
    v, t = R.icosphere(4, noise=0.03, seed=0)
    assert len(t) == 5120
    would_flip = R.round_edges(v, t, R.vertex_quadrics(v, t))[3]
    print(f"noisy sphere: the flip test rejects {int(would_flip.sum())} collapses of the input that every other rule accepts")
    assert would_flip.any()  # the guard is exercised on this input
    v2, t2, vm, info, trace = run(dev, v, t, 500)
    R.check_trace(v, t, trace, 500, final=(v2, t2, vm))  # every collapse within the flip bound
    print(f"noisy sphere 5120 -> {len(t2)} in {info['n_rounds']} rounds")
    assert R.manifold_stats(t2) == (True, 2, 1) and 499 <= len(t2) <= 500


def test_tetrahedron_and_octahedron(dev):
    v, t = R.tetrahedron()
    tv, tt_ = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev)
    v2, t2, info = ops.mesh_decimate(tv, tt_, 4)  # 4 faces, the smallest target there is: nothing to do
    assert info["unchanged"] and info["n_rounds"] == 0 and v2.data_ptr() == tv.data_ptr() and t2 is tt_
    # the tetrahedron refuses to collapse: two of them in one mesh, 8 faces for a target of 4, stall at once
    v8, t8 = np.concatenate([v, v + 4]), np.concatenate([t, t + 4])
    v2, t2, vm, info, trace = run(dev, v8, t8, 4)
    assert info["stalled"] and info["unchanged"] and info["n_rounds"] == 0 and trace == []
    assert np.array_equal(v2, v8) and np.array_equal(t2, t8) and np.array_equal(vm, np.arange(8))
    R.check_trace(v8, t8, trace, 4, final=(v2, t2, vm), stalled=True)
    # the octahedron: whatever it ends with is a closed manifold sphere, and `stalled` says why it ended
    v, t = R.octahedron()
    v2, t2, vm, info, trace = run(dev, v, t, 4)
    R.check_trace(v, t, trace, 4, final=(v2, t2, vm), stalled=info["stalled"])
    assert R.manifold_stats(t2) == (True, 2, 1) and 4 <= len(t2) <= 8
    assert info["stalled"] == (len(t2) > 4)


def test_open_height_field_keeps_its_boundary(dev):
    n = 17
    v, t = R.height_field(n)
    v2, t2, vm, info, trace = run(dev, v, t, 64)
    R.check_trace(v, t, trace, 64, final=(v2, t2, vm), stalled=info["stalled"])
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    boundary = np.flatnonzero(((i == 0) | (i == n - 1) | (j == 0) | (j == n - 1)).reshape(-1))
    assert len(boundary) == 64 == info["n_locked"]
    assert (vm[boundary] >= 0).all() and len(set(vm[boundary].tolist())) == 64
    assert np.array_equal(v2[vm[boundary]].view(np.uint32), v[boundary].view(np.uint32))
    assert len(t2) < len(t) // 2  # the interior is decimated
    print(f"height field 512 -> {len(t2)} in {info['n_rounds']} rounds, stalled {info['stalled']}")
    e = np.sort(np.concatenate([t2[:, [0, 1]], t2[:, [1, 2]], t2[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    on_boundary = np.isin(ue, vm[boundary]).all(1) & (cnt == 1)
    assert (cnt[~on_boundary] == 2).all() and int(on_boundary.sum()) == 64  # the 64 boundary edges, all others two faces


def test_non_manifold_edge_locks_its_vertices(dev):
    v, t = R.two_tetrahedra_sharing_an_edge()
    v2, t2, vm, info, trace = run(dev, v, t, 4)
    locked = np.flatnonzero(R.Topology(t, len(v)).locked)
    assert info["n_locked"] == len(locked) == 2
    assert np.array_equal(v2[vm[locked]].view(np.uint32), v[locked].view(np.uint32))
    R.check_trace(v, t, trace, 4, final=(v2, t2, vm), stalled=info["stalled"])


def test_one_round_across_the_compaction_seam(dev):
    """364 x 364 height field, 263 538 faces: the faces span more than the 262 144 items one chunk of the compaction's
    second-level scan covers.  One round; faces and vertex_map must equal the replay of the traced collapses."""
    v, t = R.height_field(364, amp=0.02, fx=40.0, fy=37.0)
    assert len(t) == 263538 > 262144
    v2, t2, vm, info, trace = run(dev, v, t, 1000, max_rounds=1)
    assert info["n_rounds"] == 1 and len(trace) == 1 and not info["stalled"]
    k = len(trace[0][0])
    print(f"seam: one round kept {k} collapses, {len(t)} -> {len(t2)} faces")
    assert k >= 1000 and len(t2) == len(t) - 2 * k
    assert t2.max() == len(v2) - 1 == len(v) - k - 1
    R.check_trace(v, t, trace, 1000, final=(v2, t2, vm), validate=False)
    sample = [(trace[0][0][::97], trace[0][1][::97], trace[0][2][::97])]  # every 97th collapse against the rules
    R.check_trace(v, t, sample, 1000)


def test_two_calls_are_bit_identical(dev):
    v, t = R.icosphere(3, noise=0.02, seed=1)
    a, b = run(dev, v, t, 300), run(dev, v, t, 300)
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    assert a[3]["n_rounds"] == b[3]["n_rounds"] > 1
    for ra, rb in zip(a[4], b[4]):
        assert all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(ra, rb))


def test_argument_errors_and_detached_positions(dev):
    v, t = (torch.from_numpy(x).to(dev) for x in R.icosphere(1))
    for bad in (3, 0, -5):
        with pytest.raises(ValueError, match="target_faces"):
            ops.mesh_decimate(v, t, bad)
    for bad in (20.0, "20", None, True):
        with pytest.raises(TypeError, match="target_faces"):
            ops.mesh_decimate(v, t, bad)
    with pytest.raises(ValueError, match="finite"):
        ops.mesh_decimate(torch.where(torch.arange(len(v), device=dev)[:, None] == 3, float("nan"), v), t, 20)
    with pytest.raises(ValueError, match="index outside"):
        ops.mesh_decimate(v, t + 1, 20)
    with pytest.raises(TypeError):
        ops.mesh_decimate(v.double(), t, 20)
    with pytest.raises(ValueError, match="max_rounds"):
        ops.mesh_decimate(v, t, 20, max_rounds=-1)
    empty = ops.mesh_decimate(v, t[:0], 20)
    assert empty[2]["unchanged"] and empty[1].shape == (0, 3)
    small = ops.mesh_decimate(v, t, 80)  # no more faces than the target
    assert small[2]["unchanged"] and small[0].data_ptr() == v.data_ptr() and small[1] is t
    hot = Mesh(v.clone().requires_grad_(True), t)
    hot.add_extra("tag", 7)
    a, b = hot.decimate(20), Mesh(v, t).decimate(20)
    assert not a.v_pos.requires_grad and torch.equal(a.v_pos, b.v_pos) and torch.equal(a.t_pos_idx, b.t_pos_idx)
    assert a.extras["tag"] == 7 and "decimate" not in hot.extras
    assert a.extras["decimate"]["target_faces"] == 20 and 19 <= a.t_pos_idx.shape[0] <= 20
    t64 = ops.mesh_decimate(v, t.long(), 20)  # int64 faces go in, int32 faces come out
    assert t64[1].dtype == torch.int32 and torch.equal(t64[1], b.t_pos_idx)


# ---- the exporter on the decimated mesh (the set-up of tests/test_gpu_simplify.py::_exporter_modules) ----
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


def test_exporter_bakes_the_decimated_mesh(dev):
    r, g, m, b, cache = _exporter_modules(dev)
    N, target = 256, 1500
    cfg = {"save_uv": True, "texture_size": N, "texture_format": "png"}
    make = lambda: tt.find("multiprompt-mesh-exporter")(cfg, geometry=g, material=m, background=b)
    exp = make()
    assert exp.decimate_target_faces is None
    exp.decimate_target_faces = target
    exp.bake_normal_map = exp.bake_ambient_occlusion = True
    (out,) = exp(cache)
    mesh = out.params["mesh"]
    with torch.no_grad():
        full = r.isosurface(cache)[0]
    want = full.decimate(target)
    assert full.t_pos_idx.shape[0] > target
    assert torch.equal(mesh.v_pos, want.v_pos) and torch.equal(mesh.t_pos_idx, want.t_pos_idx)
    info = mesh.extras["decimate"]
    print(f"exporter: {full.t_pos_idx.shape[0]} -> {mesh.t_pos_idx.shape[0]} faces in {info['n_rounds']} rounds, "
          f"stalled {info['stalled']}, locked {info['n_locked']}")
    assert mesh.t_pos_idx.shape[0] < full.t_pos_idx.shape[0] and not info["unchanged"]
    assert info["stalled"] or mesh.t_pos_idx.shape[0] <= target
    closed_in = R.manifold_stats(full.t_pos_idx.cpu().numpy())
    if closed_in[0]:  # a closed input: same Euler characteristic and components, the budget met
        assert R.manifold_stats(mesh.t_pos_idx.cpu().numpy()) == closed_in
    for key in ("map_Kd", "map_Bump", "map_Ka"):
        img = out.params[key]
        assert img.shape[:2] == (N, N) and bool(torch.isfinite(img).all()), key
    assert out.params["map_Kd"].shape == (N, N, 3)
    exp.simplify_grid = 24
    with pytest.raises(ValueError, match="decimate_target_faces"):
        exp(cache)
    # unset: bit for bit the output of an exporter that never had the attribute set
    exp.simplify_grid = exp.decimate_target_faces = None
    exp.bake_normal_map = exp.bake_ambient_occlusion = False
    (plain,) = exp(cache)
    (fresh,) = make()(cache)
    for key in ("v_pos", "t_pos_idx", "v_tex", "t_tex_idx"):
        assert torch.equal(getattr(plain.params["mesh"], key), getattr(fresh.params["mesh"], key))
    assert torch.equal(plain.params["mesh"].t_pos_idx, full.t_pos_idx)
    assert torch.equal(plain.params["map_Kd"], fresh.params["map_Kd"])
