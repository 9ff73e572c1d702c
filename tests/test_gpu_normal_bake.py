"""The tangent-space normal-map bake (tt_bake_project / tt_bake_encode; ops.bake_normal_map, the exporter's
bake_normal_map switch, viewer.load_normal_map and mode "normal_map") on the exporter scene of tests/test_gpu_export.py:
64^2 planes, isosurface_resolution 64, simplify_grid 16, a 256^2 texture.  The kernels against the float64 restatement
(tests/tangent_reference.py) on the GPU's own inputs, the projection's bounds, the OBJ / MTL / PNG round trip, what the
map is for (the rendered normals get closer to the field's than the low-poly mesh's own), and that nothing changes
while the switch is unset."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, raster, viewer
from triplaneturbo_amd.export import read_png, save_obj
from triplaneturbo_amd.isosurface import Mesh, obj_uv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import tangent_reference as TR  # noqa: E402
from test_gpu_export import _exporter_modules  # noqa: E402
from time_normal_bake import normal_errors  # noqa: E402

pytestmark = pytest.mark.gpu
N, GRID, STEPS = 256, 16, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def scene(dev):
    """the exporter run three times in this order: switch unset (before any bake in the process), set, unset again"""
    r, g, m, b, cache = _exporter_modules(dev)
    exp = tt.find("multiprompt-mesh-exporter")({"save_uv": True, "texture_size": N, "texture_format": "png"},
                                               geometry=g, material=m, background=b)
    assert exp.bake_normal_map is False and exp.bake_project_steps == 2
    exp.simplify_grid = GRID
    (before,) = exp(cache)
    exp.bake_normal_map = True
    (baked,) = exp(cache)
    info = exp.bake_info
    exp.bake_normal_map = False
    (after,) = exp(cache)
    mesh = baked.params["mesh"]

    def field(p):
        with torch.no_grad():
            out = g.forward(p[None], cache[:1], output_normal=True)
        return out["sdf"], out["sdf_grad"]

    rast = ops.uv_rasterize(mesh.v_tex, mesh.t_tex_idx, N)
    pos0 = raster.interpolate(mesh.v_pos[None], rast[None], mesh.t_pos_idx.int())[0].reshape(-1, 3)
    return dict(before=before, baked=baked, after=after, info=info, mesh=mesh, field=field, rast=rast,
                pts0=pos0[info["texel"]].contiguous(), cell=mesh.extras["simplify"]["cell"])


def test_switch_unset_changes_nothing_and_set_keeps_the_colour(scene):
    b, k, a = scene["before"].params, scene["baked"].params, scene["after"].params
    assert b["map_Bump"] is None and a["map_Bump"] is None
    for x in (k, a):
        assert torch.equal(x["map_Kd"], b["map_Kd"])
        assert torch.equal(x["mesh"].v_tex, b["mesh"].v_tex) and torch.equal(x["mesh"].t_tex_idx, b["mesh"].t_tex_idx)
        assert torch.equal(x["mesh"].v_pos, b["mesh"].v_pos)
    assert set(k) == set(b)
    bump = k["map_Bump"]
    assert bump.shape == (N, N, 3) and bump.dtype == torch.float32 and 0 <= bump.min() and bump.max() <= 1
    info = scene["info"]
    print({x: info[x] for x in ("n_covered", "n_backfacing", "mean_abs_sdf_before", "mean_abs_sdf_after")})
    assert info["n_covered"] == int((scene["rast"][..., 3] > 0).sum()) == len(info["texel"]) > 10000
    assert info["n_backfacing"] < 0.01 * info["n_covered"]


def test_encode_matches_the_restatement(scene):
    mesh, rast, info = scene["mesh"], scene["rast"], scene["info"]
    field = torch.zeros(N * N, 3, device=rast.device)
    field[info["texel"]] = info["sdf_grad"]
    got, counts = ops.bake_encode(rast, mesh.v_nrm, mesh.t_pos_idx, mesh.v_tng_tex, mesh.t_tex_idx,
                                  field.reshape(N, N, 3))
    want, cov, back = TR.encode(*(x.cpu().numpy() for x in (rast, mesh.v_nrm, mesh.t_pos_idx, mesh.v_tng_tex,
                                                            mesh.t_tex_idx, field.reshape(N, N, 3))))
    g = got.cpu().numpy()
    err = np.abs(g.astype(np.float64) - want)[cov].max()
    print(f"encode: max error {err:.2e} over {cov.sum()} covered texels, {back.sum()} back-facing")
    assert err <= 1e-5
    assert np.array_equal(g[~cov], np.broadcast_to(np.float32([0.5, 0.5, 1.0]), g[~cov].shape))
    n_cov, n_back = counts.tolist()
    assert n_cov == cov.sum() == info["n_covered"]
    near = cov & (np.abs(want[..., 2] - 0.5) <= 1e-5)  # m.n within rounding of 0: either count is right
    assert abs(n_back - back.sum()) <= near.sum() and n_back == info["n_backfacing"]
    # the exporter's map is this map, filled; covered texels come back bit for bit
    bump = scene["baked"].params["map_Bump"]
    c = torch.from_numpy(cov).to(bump.device)
    assert torch.equal(bump[c], got[c])
    again, _ = ops.bake_normal_map(mesh, scene["field"], N, project_steps=STEPS, rast=rast)
    assert torch.equal(again, got)  # bit-identical from run to run


def test_projection_step_and_bounds(scene):
    mesh, info, field, cell = scene["mesh"], scene["info"], scene["field"], scene["cell"]
    p0 = scene["pts0"]
    sdf, grad = field(p0)
    for max_step in (cell, cell / 64):  # the limit idle, and the limit biting on most points
        got = ops.bake_project_step(p0.clone(), sdf, grad, max_step).cpu().numpy().astype(np.float64)
        want = TR.project_step(p0.cpu().numpy(), sdf.cpu().numpy(), grad.cpu().numpy(), max_step)
        rel = np.abs(got - want).max() / np.abs(want).max()
        moved = np.linalg.norm(want - p0.cpu().numpy(), axis=1)
        print(f"max_step {max_step:.4f}: relative error {rel:.2e}, {(moved > 0.999 * max_step).mean():.2f} at the limit")
        assert rel <= 1e-6
    mask = torch.arange(len(p0), device=p0.device) % 3 == 0
    got = ops.bake_project_step(p0.clone(), sdf, grad, cell, mask=mask)
    assert torch.equal(got[~mask], p0[~mask]) and not torch.equal(got[mask], p0[mask])
    # K steps move a point by at most K max_step
    disp = (info["points"].double() - p0.double()).norm(dim=1).max().item()
    print(f"displacement after {STEPS} steps: {disp:.4f} (max_step {cell:.4f}); mean |sdf| "
          f"{info['mean_abs_sdf_before']:.3e} -> {info['mean_abs_sdf_after']:.3e}")
    assert disp <= STEPS * cell * (1 + 1e-6)
    assert info["mean_abs_sdf_after"] < info["mean_abs_sdf_before"]
    small = cell / 64
    _, i2 = ops.bake_normal_map(mesh, field, N, project_steps=STEPS, max_step=small, rast=scene["rast"])
    d2 = (i2["points"].double() - p0.double()).norm(dim=1).max().item()
    # (the positions are stored in fp32: each step adds up to sqrt(3) / 2 ulp of a coordinate below 2)
    assert d2 <= STEPS * (small * (1 + 1e-6) + 3 ** 0.5 * 2.0 ** -24)
    assert i2["mean_abs_sdf_after"] < i2["mean_abs_sdf_before"]


def test_zero_steps_samples_the_unprojected_points(scene):
    mesh, rast, info = scene["mesh"], scene["rast"], scene["info"]
    got, i0 = ops.bake_normal_map(mesh, scene["field"], N, project_steps=0, rast=rast)
    assert torch.equal(i0["points"], scene["pts0"]) and torch.equal(i0["texel"], info["texel"])
    assert i0["mean_abs_sdf_after"] == i0["mean_abs_sdf_before"]
    field = torch.zeros(N * N, 3, device=rast.device)
    field[info["texel"]] = scene["field"](scene["pts0"])[1].reshape(-1, 3)
    want, _ = ops.bake_encode(rast, mesh.v_nrm, mesh.t_pos_idx, mesh.v_tng_tex, mesh.t_tex_idx, field.reshape(N, N, 3))
    assert torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.bake_normal_map(mesh, scene["field"], N, project_steps=-1, rast=rast)
    with pytest.raises(ValueError):
        ops.bake_normal_map(Mesh(mesh.v_pos, mesh.t_pos_idx), scene["field"], N)  # not simplified: max_step is needed


@pytest.fixture(scope="module")
def round_trip(scene, dev, tmp_path_factory):
    """export -> save_obj (PNG) -> load_obj + load_normal_map, two 128^2 views of the loaded mesh, and every covered
    pixel's UV moved to a covered texel centre: the pixel gets the barycentrics the bake's own UV rasterisation has at
    the nearest texel centre, where that texel lies in the pixel's face.  There the bake queried `want`."""
    d = tmp_path_factory.mktemp("round_trip")
    out, info = scene["baked"], scene["info"]
    paths = save_obj(str(d / out.save_name), **out.params)
    mesh, map_kd = viewer.load_obj(str(d / "model.obj"), device=dev)
    png = viewer.load_normal_map(str(d / "model.obj"), device=dev)
    size = 128
    ctx = raster.RasterizerContext("cuda", dev)
    _, _, c2w, _ = tt.synthetic.make_cameras(2, size, size, fovy_deg=40.0, elevation_deg=15.0)
    mvp = (viewer.get_projection_matrix(40.0, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), mesh.t_pos_idx, (size, size))
    cov = rast[..., 3] > 0
    uv = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)[0]
    tx = (uv[..., 0] * N).floor().clamp(0, N - 1).long()
    ty = (uv[..., 1] * N).floor().clamp(0, N - 1).long()
    at = scene["rast"][ty, tx]  # the bake's rasterisation at those texels
    same = cov & (at[..., 3] == rast[..., 3])
    moved = torch.where(same[..., None], torch.cat([at[..., :2], rast[..., 2:]], -1), torch.zeros_like(rast))
    queried = torch.zeros(N * N, 3, device=dev)
    queried[info["texel"]] = F.normalize(info["sdf_grad"], dim=-1)
    return dict(dir=d, paths=paths, mesh=mesh, map_kd=map_kd, png=png, bump=out.params["map_Bump"], ctx=ctx, mvp=mvp,
                size=size, rast=rast, cov=cov, same=same, moved=moved, want=queried[(ty * N + tx)[same]])


def test_round_trip_through_the_files(scene, round_trip, dev):
    rt = round_trip
    d, mesh, bump, ctx, mvp, size, rast, cov = (rt[k] for k in ("dir", "mesh", "bump", "ctx", "mvp", "size", "rast", "cov"))
    assert sorted(os.path.basename(p) for p in rt["paths"]) == ["model.mtl", "model.obj", "texture_kd.png",
                                                                "texture_nrm.png"]
    assert "map_Bump texture_nrm.png" in open(d / "model.mtl").read()
    assert rt["png"].shape == bump.shape and (rt["png"] - bump).abs().max().item() <= 1.0 / 255.0
    assert np.array_equal(read_png(str(d / "texture_nrm.png")), (bump.cpu().numpy() * 255.0).astype(np.uint8))
    baked_mesh = scene["baked"].params["mesh"]
    assert (mesh.v_pos - baked_mesh.v_pos).abs().max().item() <= 1e-6
    # mode "normal_map" is (world normal + 1) / 2 over the background
    kw = dict(antialias=False, ctx=ctx)
    img = viewer.render_textured(mesh, rt["map_kd"], mvp, size, size, mode="normal_map", map_Bump=bump,
                                 filter_mode="nearest", **kw)
    n_img = viewer.world_normal_from_map(mesh, rast, bump, filter_mode="nearest", ctx=ctx)
    assert (img[cov] - (n_img[cov] + 1) / 2).abs().max().item() <= 1e-6 and (img[~cov] == 1).all()
    # with the mesh in memory (the UVs the bake saw) the rebuilt normal is the queried one
    assert rt["same"].float().sum() > 0.5 * cov.float().sum()
    got = viewer.world_normal_from_map(baked_mesh, rt["moved"], bump, filter_mode="nearest", ctx=ctx)[rt["same"]]
    err_mem = (got - rt["want"]).abs().max().item()
    print(f"round trip, mesh in memory: max |rebuilt - queried| = {err_mem:.2e} over {int(rt['same'].sum())} pixels")
    assert err_mem <= 1e-5
    # "rgb" is what it was without the two new arguments, and shaded with them
    plain = viewer.render_textured(mesh, rt["map_kd"], mvp, size, size, **kw)
    light = torch.tensor([0.3, -0.5, 0.8])
    lit = viewer.render_textured(mesh, rt["map_kd"], mvp, size, size, map_Bump=bump, light_dir=light, **kw)
    assert torch.equal(plain, viewer.render_textured(mesh, rt["map_kd"], mvp, size, size, map_Bump=bump, **kw))
    n_lin = viewer.world_normal_from_map(mesh, rast, bump, ctx=ctx)
    shade = (n_lin * F.normalize(light, dim=0).to(dev)).sum(-1, keepdim=True).clamp_min(0)
    assert (lit[cov] - (plain * shade)[cov]).abs().max().item() <= 1e-6 and (lit <= plain + 1e-6).all()


def test_round_trip_rebuilds_the_queried_normal_from_the_loaded_mesh(scene, round_trip):
    """The same comparison with the mesh load_obj returns, float map, nearest filtering, bound 1e-5.

    save_obj writes `vt u (1 - v)` with `1 - v` rounded to float32 (tests/test_export_host.py pins that text), so
    load_obj's v_tex is up to 2^-25 from the exporter's.  The simplified mesh has UV triangles well under a texel wide,
    whose tangents amplify that by 1 / (UV edge length): built on v_tex itself, the loaded mesh's tangents were 1.96e-5
    from the ones the map was encoded in and this comparison read 1.23e-5.  Mesh.v_tng_tex is therefore built on
    isosurface.obj_uv(v_tex), the UVs as the file carries them, which both meshes share exactly.  (Their v_nrm still
    differ by an ulp, the order of scatter_add's float atomics, so the two v_tng_tex are compared on one v_nrm.)"""
    rt = round_trip
    mesh, baked_mesh = rt["mesh"], scene["baked"].params["mesh"]
    got = viewer.world_normal_from_map(mesh, rt["moved"], rt["bump"], filter_mode="nearest", ctx=rt["ctx"])[rt["same"]]
    err = (got - rt["want"]).abs().max().item()
    d_uv = (mesh.v_tex - baked_mesh.v_tex).abs().max().item()
    d_tng = (mesh.v_tng_tex - baked_mesh.v_tng_tex).abs().max().item()
    print(f"round trip, loaded mesh: max |rebuilt - queried| = {err:.2e} over {int(rt['same'].sum())} pixels; the files "
          f"move v_tex by {d_uv:.2e} and v_tng_tex by {d_tng:.2e}")
    assert err <= 1e-5
    assert 0 < d_uv <= 2.0 ** -25 and torch.equal(mesh.v_tex, obj_uv(baked_mesh.v_tex))
    assert torch.equal(baked_mesh.v_tng_tex, ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx,
                                                               baked_mesh.v_nrm, "tex"))


def test_the_map_brings_the_normals_closer_to_the_field(scene):
    """what the map is for: over the interior covered pixels of two 128^2 views, the mean angle to the field's normal at
    the projected surface point is smaller with the map than with the low-poly mesh's own normals.  No ratio is
    asserted: none can be derived, and one read off the code under test would be circular.  (tools/time_normal_bake.py
    records both figures for the 160^3 scenes in profiles/normal_bake.json.)"""
    bump = scene["baked"].params["map_Bump"]
    e_map, e_low, pixels = normal_errors(scene["mesh"], bump, scene["field"], scene["cell"], size=128, n_views=2,
                                         project_steps=STEPS)
    print(f"mean angle to the field normal over {pixels} pixels: {e_map:.3f} deg with the map, {e_low:.3f} deg without")
    assert pixels > 2000
    assert e_map < e_low


def test_cli_writes_the_bump_views(scene, tmp_path):
    out = scene["baked"]
    save_obj(str(tmp_path / out.save_name), **out.params)
    viewer.main([str(tmp_path / "model.obj"), "--out", str(tmp_path / "views"), "--num_views", "2", "--size", "64",
                 "--ssaa", "1", "--bump"])
    assert sorted(os.listdir(tmp_path / "views")) == ["bump_0.png", "bump_1.png", "rgb_0.png", "rgb_1.png"]
    img = read_png(str(tmp_path / "views" / "bump_0.png"))
    assert img.shape == (64, 64, 3) and (img != 255).any()
    # an OBJ whose MTL names no normal map: --bump writes nothing extra
    plain = scene["before"]
    os.makedirs(tmp_path / "plain")
    save_obj(str(tmp_path / "plain" / plain.save_name), **plain.params)
    assert viewer.load_normal_map(str(tmp_path / "plain" / "model.obj")) is None
    viewer.main([str(tmp_path / "plain" / "model.obj"), "--out", str(tmp_path / "plain" / "views"), "--num_views", "1",
                 "--size", "32", "--ssaa", "1", "--bump"])
    assert os.listdir(tmp_path / "plain" / "views") == ["rgb_0.png"]
