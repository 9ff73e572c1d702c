"""Conformal UV charts on the GPU (tt_uv_lscm_*; ops.uv_flatten_lscm, ops.uv_atlas(method="lscm"), Mesh.unwrap_uv,
exporter.uv_method): the solver against the dense float64 reference (tests/uv_lscm_reference.py), its failure flags,
the atlas invariants of tests/test_gpu_export.py with the conformal map in place of the projection, the quality the
feature is for, the exact fallback, determinism, and the exporter end to end."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, raster, synthetic, viewer
from triplaneturbo_amd.export import save_obj
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_lscm_reference as L  # noqa: E402
import uv_reference as U  # noqa: E402
from test_isosurface_oracle import sphere, torus, two_spheres  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.3
MESHES = ["sphere", "torus", "two_spheres"]
# |uv_gpu - uv_ref| / chart extent: 10 x the maximum measured over the cases below (tools/time_uv_atlas.py records it in
# profiles/uv_lscm.json), and never above one texel of a chart that spans 1024
SOLVER_CAP = 1e-3


def solver_bound():
    rec = json.load(open(os.path.join(ROOT, "profiles", "uv_lscm.json")))["solver_vs_reference"]
    return min(10.0 * float(rec["max_rel_err"]), SOLVER_CAP)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def small_meshes(dev):
    def mc(level):
        v, t = ops.marching_cubes(torch.from_numpy(level).to(dev))
        return Mesh(v * 2 - 1, t)
    return {"sphere": mc(sphere(48)), "torus": mc(torus(40)), "two_spheres": mc(two_spheres(40))}


@pytest.fixture(scope="module")
def atlases(small_meshes):
    """both atlases of every small mesh at N = 256, pad 2, computed once"""
    out = {}
    for name, m in small_meshes.items():
        out[name] = {k: ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 256, 2, method=k) for k in ("axis", "lscm")}
    return out


def run_solver_case(v, tri, chart, dev):
    uv, t_tex, info = ops.uv_flatten_lscm(torch.from_numpy(v).to(dev), torch.from_numpy(tri).int().to(dev),
                                          torch.from_numpy(chart).int().to(dev))
    ref = L.flatten(v, tri, chart, TAU)
    assert np.array_equal(t_tex.cpu().numpy(), ref["t_tex"])
    assert np.array_equal(info["chart_ids"].cpu().numpy(), ref["chart_ids"])
    assert np.array_equal(info["pins"].cpu().numpy(), ref["pins"])
    assert not ref["fallback"].any() and not info["fallback"].any()
    assert uv.dtype == torch.float64 and info["iterations"] >= int(info["chart_iterations"].max()) > 0
    assert (info["residual"] <= 1e-8).all()
    err = L.solver_error(uv.cpu().numpy(), ref)
    k, rot = info["scale"].cpu().numpy(), info["rotation"].cpu().numpy()
    assert np.abs(k / ref["scale"] - 1).max() <= 1e-5
    # (a chart as wide as it is high has no principal axis to speak of: the final coordinates are compared, not angles)
    final = info["uv_final"].double().cpu().numpy()
    c, s = np.cos(rot)[ref["vchart_dense"]], np.sin(rot)[ref["vchart_dense"]]
    kk = k[ref["vchart_dense"]]
    raw = uv.cpu().numpy()
    want = np.stack([kk * (c * raw[:, 0] - s * raw[:, 1]), kk * (s * raw[:, 0] + c * raw[:, 1])], 1)
    assert np.abs(final - want).max() <= 1e-6 * max(np.abs(want).max(), 1e-30)
    return err


@pytest.mark.parametrize("name", ["flat_patch", "half_cylinder", "one_triangle", "two_triangles", "shared_vertices"])
def test_solver_matches_the_reference_on_explicit_charts(dev, name):
    err = run_solver_case(*L.explicit_cases()[name], dev)
    print(f"{name}: max |uv - uv_ref| / extent = {err:.3e} (bound {solver_bound():.3e})")
    assert err <= solver_bound()


@pytest.mark.parametrize("name", MESHES)
def test_solver_matches_the_reference_on_axis_charts(dev, small_meshes, atlases, name):
    m = small_meshes[name]
    chart = atlases[name]["axis"][2]["chart"]
    err = run_solver_case(m.v_pos.cpu().numpy(), m.t_pos_idx.cpu().numpy().astype(np.int64),
                          chart.cpu().numpy().astype(np.int64), dev)
    print(f"{name}: max |uv - uv_ref| / extent = {err:.3e} (bound {solver_bound():.3e})")
    assert err <= solver_bound()


def test_failure_flags(dev, small_meshes):
    # a chart of zero-area faces only (collinear; all in one point) next to a good one
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5], [0, 1, 0]], dtype=torch.float32, device=dev)
    tri = torch.tensor([[0, 1, 2], [3, 3, 3], [0, 1, 4]], dtype=torch.int32, device=dev)
    uv, t_tex, info = ops.uv_flatten_lscm(v, tri, torch.tensor([0, 1, 2], dtype=torch.int32, device=dev))
    assert info["fallback"].tolist() == [True, True, False]
    assert torch.isfinite(uv).all()
    ref = L.flatten(v.cpu().numpy(), tri.cpu().numpy().astype(np.int64), np.array([0, 1, 2]), TAU)
    assert ref["fallback"].tolist() == [True, True, False]
    # a closed sphere as ONE chart: two pins on a closed surface cannot keep every face within [tau, 1/tau]
    m = small_meshes["sphere"]
    T = m.t_pos_idx.shape[0]
    uv, t_tex, info = ops.uv_flatten_lscm(m.v_pos, m.t_pos_idx, torch.zeros(T, dtype=torch.int32, device=dev))
    print(f"closed sphere as one chart: {info['iterations']} iterations, residual {float(info['residual'][0]):.2e}")
    assert info["fallback"].tolist() == [True] and info["charts"] == 1
    assert float(info["residual"][0]) <= 1e-8  # it converged: the acceptance test rejected it, not the iteration limit
    # no iteration: nothing converges
    uv, t_tex, info = ops.uv_flatten_lscm(v, tri, torch.tensor([0, 1, 2], dtype=torch.int32, device=dev), max_iters=0)
    assert info["fallback"].all() and info["iterations"] == 0 and int(info["chart_iterations"].max()) == 0


def _invariants(mesh, v_tex, t_tex, info, N, pad):
    """tests/test_gpu_export.py's _invariants with the conformal map in place of the projection on accepted charts"""
    ls = info["lscm"]
    vt = v_tex.double().cpu()
    assert vt.min() >= 0 and vt.max() <= 1
    tri = mesh.t_pos_idx.long().cpu()
    tt_ = t_tex.long().cpu()
    v = mesh.v_pos.double().cpu()
    lab = info["labels"].long().cpu()
    chart = info["chart"].long().cpu()
    box = info["chart_box"].double()
    off = info["offsets"].double()
    s = info["scale"]
    fb = ls["fallback"].cpu()
    pair = torch.stack([tt_.reshape(-1), tri.reshape(-1)], 1).unique(dim=0)
    assert len(pair) == len(vt) and torch.equal(pair[:, 0], torch.arange(len(vt)))
    # accepted charts: texel UV = offset + pad + 0.5 + s (R_c k_c raw - min); fallback charts: the projection
    raw = ls["uv"].cpu()[tt_]  # (T,3,2)
    k, rot = ls["scale"].cpu()[chart][:, None], ls["rotation"].cpu()[chart][:, None]
    fu = k * (torch.cos(rot) * raw[..., 0] - torch.sin(rot) * raw[..., 1])
    fv = k * (torch.sin(rot) * raw[..., 0] + torch.cos(rot) * raw[..., 1])
    ax = torch.tensor(U.AXES)
    cu, cv = ax[lab][:, 0], ax[lab][:, 1]
    P = v[tri]
    pu = P.gather(2, cu[:, None, None].expand(-1, 3, 1))[..., 0]
    pv = P.gather(2, cv[:, None, None].expand(-1, 3, 1))[..., 0]
    f = fb[chart][:, None]
    qu, qv = torch.where(f, pu, fu), torch.where(f, pv, fv)
    Uw = off[chart, 0][:, None] + pad + 0.5 + (qu - box[chart, 0][:, None]) * s
    Vw = off[chart, 1][:, None] + pad + 0.5 + (qv - box[chart, 1][:, None]) * s
    got = vt[tt_] * N
    assert (got[..., 0] - Uw).abs().max() <= 2e-3 and (got[..., 1] - Vw).abs().max() <= 2e-3
    # signed UV area positive and within [tau, 1/tau] s^2 (3-D area) on faces whose area is far above float rounding
    e1, e2 = got[:, 1] - got[:, 0], got[:, 2] - got[:, 0]
    area_uv = 0.5 * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    area_3d = 0.5 * torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).norm(dim=-1) * s * s
    big = area_3d > 1e-3
    assert big.float().mean() > 0.5
    assert (area_uv[big] > 0).all()
    assert (area_uv[big] >= TAU * area_3d[big] * (1 - 1e-3) - 1e-4).all()
    assert (area_uv[big] <= area_3d[big] / TAU * (1 + 1e-3) + 1e-4).all()
    # chart texel boxes inside the texture and disjoint
    occ = torch.zeros(N, N, dtype=torch.int32)
    w = box[:, 2:] - box[:, :2]
    for c in range(info["charts"]):
        x0, y0 = int(off[c, 0]), int(off[c, 1])
        bw = int(np.ceil(float(w[c, 0]) * s)) + 2 * pad + 1
        bh = int(np.ceil(float(w[c, 1]) * s)) + 2 * pad + 1
        assert x0 >= 0 and y0 >= 0 and x0 + bw <= N and y0 + bh <= N
        occ[y0:y0 + bh, x0:x0 + bw] += 1
    assert occ.max() == 1
    lo, hi = got.amin(1), got.amax(1)
    assert (lo[:, 0] >= off[chart, 0] + pad + 0.5 - 2e-3).all() and (lo[:, 1] >= off[chart, 1] + pad + 0.5 - 2e-3).all()
    assert (hi[:, 0] <= off[chart, 0] + pad + 0.5 + w[chart, 0] * s + 2e-3).all()
    assert (hi[:, 1] <= off[chart, 1] + pad + 0.5 + w[chart, 1] * s + 2e-3).all()
    # zero texel centres are covered twice (a fresh count by the overlap kernel)
    lib_flags = torch.empty(len(tri), device=v_tex.device, dtype=torch.uint8)
    tot = torch.empty(4, device=v_tex.device, dtype=torch.int32)
    lib = tt._lib.load()
    ws = torch.empty(int(lib.tt_uv_workspace_bytes(mesh.v_pos.shape[0], len(tri), N)), device=v_tex.device,
                     dtype=torch.uint8)
    tt._lib.check(lib.tt_uv_overlap(ops._ptr(v_tex), ops._ptr(t_tex), len(vt), mesh.v_pos.shape[0], len(tri), N,
                                    ops._ptr(ws), ops._ptr(lib_flags), ops._ptr(tot), ops._stream()), "overlap")
    assert int(tot[0]) == 0


@pytest.mark.parametrize("name", MESHES)
def test_atlas_invariants(small_meshes, atlases, name):
    v_tex, t_tex, info = atlases[name]["lscm"]
    _invariants(small_meshes[name], v_tex, t_tex, info, 256, 2)
    axis = atlases[name]["axis"][2]
    assert torch.equal(info["labels"], axis["labels"])
    chart0 = axis["chart"] if axis["overlap_rounds"] == 0 else None
    if chart0 is None:  # the axis path's first-round charts: its labels' components without singletons
        m = small_meshes[name]
        tri = m.t_pos_idx.cpu().numpy().astype(np.int64)
        chart0 = torch.from_numpy(U.charts(tri, U.face_pairs(tri), axis["labels"].cpu().numpy())).to(v_tex.device)
    assert torch.equal(info["lscm"]["chart_round0"].long(), chart0.long())
    assert set(info["lscm"]) >= {"uv", "iterations", "residual", "pins", "fallback", "rotation", "scale"}
    C = info["charts"]
    assert info["lscm"]["uv"].dtype == torch.float64 and info["lscm"]["uv"].shape == (v_tex.shape[0], 2)
    assert info["lscm"]["fallback"].dtype == torch.bool
    for key, shape in (("residual", (C,)), ("pins", (C, 2)), ("fallback", (C,)), ("rotation", (C,)), ("scale", (C,))):
        assert tuple(info["lscm"][key].shape) == shape, key


@pytest.mark.parametrize("name", MESHES)
def test_conformal_charts_are_less_stretched(small_meshes, atlases, name):
    m = small_meshes[name]
    v, tri = m.v_pos.cpu().numpy(), m.t_pos_idx.cpu().numpy().astype(np.int64)
    v_tex, t_tex, info = atlases[name]["lscm"]
    assert int(info["lscm"]["fallback"].sum()) == 0 and info["overlap_rounds"] == 0
    a_tex, a_idx, _ = atlases[name]["axis"]
    lscm = L.mean_anisotropy(v, tri, v_tex.cpu().numpy(), t_tex.cpu().numpy())
    axis = L.mean_anisotropy(v, tri, a_tex.cpu().numpy(), a_idx.cpu().numpy())
    print(f"{name}: area-weighted mean sigma1/sigma2 lscm {lscm:.4f} axis {axis:.4f}, "
          f"{info['lscm']['iterations']} iterations, {info['charts']} charts")
    assert lscm < axis


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_fallback_is_the_axis_atlas_bit_for_bit(small_meshes, atlases, name):
    m = small_meshes[name]
    v_tex, t_tex, info = ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 256, 2, method="lscm", lscm_max_iters=0)
    assert info["lscm"]["fallback"].all()
    a_tex, a_idx, a_info = atlases[name]["axis"]
    assert torch.equal(v_tex, a_tex) and torch.equal(t_tex, a_idx)
    assert torch.equal(info["chart_box"], a_info["chart_box"]) and info["scale"] == a_info["scale"]


def test_two_calls_are_bit_identical(small_meshes, atlases):
    m = small_meshes["torus"]
    a = atlases["torus"]["lscm"]
    b = ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 256, 2, method="lscm")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[2]["lscm"]["uv"], b[2]["lscm"]["uv"])
    assert torch.equal(a[2]["lscm"]["residual"], b[2]["lscm"]["residual"])


def test_mesh_unwrap_uv_takes_the_method(small_meshes, atlases):
    src = small_meshes["sphere"]
    m = Mesh(src.v_pos, src.t_pos_idx)
    m.unwrap_uv(texture_size=256, method="lscm")
    assert "lscm" in m.uv_info and torch.equal(m.v_tex, atlases["sphere"]["lscm"][0])
    m.unwrap_uv(texture_size=256)
    assert "lscm" not in m.uv_info and torch.equal(m.v_tex, atlases["sphere"]["axis"][0])
    with pytest.raises(NotImplementedError):
        m.unwrap_uv({"max_iterations": 2}, method="lscm")


# ---- the exporter ------------------------------------------------------------------------------------------------
N_TEX, SIZE, FOVY = 512, 128, 40.0


@pytest.fixture(scope="module")
def exporter(dev):
    """the exporter scene of tests/test_gpu_textured_render.py, restated"""
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=64), geometry=g, material=m,
                                background=b).to(dev)
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    exp = tt.find("multiprompt-mesh-exporter")({"save_uv": True, "texture_size": N_TEX, "texture_format": "png"},
                                               geometry=g, material=m, background=b)
    return exp, g, m, cache


def test_exporter_lscm_render_matches_the_decoded_field(exporter, dev, tmp_path):
    """bake, fill, save_obj, load_obj, render: tests/test_gpu_textured_render.py's check of the baked texture against
    the field decoded at the same surface points, with its bar (mean absolute difference <= 0.02)"""
    exp, g, m, cache = exporter
    exp.uv_method = "lscm"
    try:
        (out,) = exp(cache)
    finally:
        exp.uv_method = None
    info = out.params["mesh"].uv_info
    assert "lscm" in info and int((~info["lscm"]["fallback"]).sum()) > 0
    save_obj(str(tmp_path / out.save_name), **out.params)
    mesh, kd = viewer.load_obj(str(tmp_path / out.save_name), device=dev)
    _, _, c2w, _ = synthetic.make_cameras(2, SIZE, SIZE, fovy_deg=FOVY)
    mvp = (viewer.get_projection_matrix(FOVY, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    ctx = raster.RasterizerContext("cuda", dev)
    with torch.no_grad():
        img = viewer.render_textured(mesh, kd, mvp, SIZE, SIZE, ssaa=1, antialias=False, ctx=ctx)
        rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), mesh.t_pos_idx, (SIZE, SIZE))
        cov = rast[..., 3] > 0
        p, _ = ctx.interpolate(mesh.v_pos[None], rast, mesh.t_pos_idx)
        want = m.export(**g.export(points=p[cov], space_cache=cache[:1]))["albedo"]
    assert (cov.flatten(1).sum(1) > 0.05 * SIZE * SIZE).all()
    err = (img[cov] - want).abs().flatten().double()
    print(f"lscm bake vs decode at {int(cov.sum())} covered pixels: mean {err.mean().item():.4f} "
          f"max {err.max().item():.4f}; {info['charts']} charts, {int(info['lscm']['fallback'].sum())} fallbacks")
    assert err.mean().item() <= 0.02


def test_exporter_lscm_normal_map(exporter):
    exp, g, m, cache = exporter
    exp.uv_method, exp.bake_normal_map = "lscm", True
    try:
        (out,) = exp(cache)
    finally:
        exp.uv_method, exp.bake_normal_map = None, False
    bump, mesh = out.params["map_Bump"], out.params["mesh"]
    rast = ops.uv_rasterize(mesh.v_tex, mesh.t_tex_idx, N_TEX)
    cov = rast[..., 3] > 0
    assert int(cov.sum()) == exp.bake_info["n_covered"] > 10000
    n = bump[cov] * 2 - 1
    assert torch.isfinite(bump).all() and (n.norm(dim=-1) - 1).abs().max().item() <= 1e-4


def test_exporter_unset_is_the_axis_export_bit_for_bit(exporter):
    exp, g, m, cache = exporter
    assert exp.uv_method is None
    (a,) = exp(cache)
    exp.uv_method = "axis"
    try:
        (b,) = exp(cache)
    finally:
        exp.uv_method = None
    assert set(a.params) == set(b.params)
    for key in ("v_pos", "t_pos_idx", "v_tex", "t_tex_idx"):
        assert torch.equal(getattr(a.params["mesh"], key), getattr(b.params["mesh"], key)), key
    assert torch.equal(a.params["map_Kd"], b.params["map_Kd"])
    assert "lscm" not in a.params["mesh"].uv_info and "lscm" not in b.params["mesh"].uv_info
