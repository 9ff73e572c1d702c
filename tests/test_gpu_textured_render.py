"""The exported asset seen the way a consumer sees it: export a scene with the `multiprompt-mesh-exporter`, write it
with save_obj, read it back with viewer.load_obj and render it with viewer.render_textured (rasterize the mesh,
interpolate v_tex through t_tex_idx, sample map_Kd) -- against the float64 restatement of the sampler at the same UVs,
against decoding the field at the same surface points, and through the gradients, the turntable and the CLI."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import raster, synthetic, viewer
from triplaneturbo_amd.export import read_png, save_obj
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TEX, SIZE, FOVY = 512, 128, 40.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _exporter_modules(dev, resolution=64):
    """the exporter scene of tests/test_gpu_export.py, restated: two prompts, smooth 64^2 planes upsampled from 8^2"""
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=resolution), geometry=g, material=m,
                                background=b).to(dev)
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    return g, m, b, cache


@pytest.fixture(scope="module")
def scene(dev, tmp_path_factory):
    """export -> save_obj -> load_obj, the G-buffer of two views and their render, computed once"""
    g, m, b, cache = _exporter_modules(dev)
    exp = tt.find("multiprompt-mesh-exporter")({"save_uv": True, "texture_size": N_TEX, "texture_format": "png"},
                                               geometry=g, material=m, background=b)
    (out,) = exp(cache)
    d = tmp_path_factory.mktemp("export")
    save_obj(str(d / out.save_name), **out.params)
    mesh, kd = viewer.load_obj(str(d / out.save_name), device=dev)
    _, _, c2w, _ = synthetic.make_cameras(2, SIZE, SIZE, fovy_deg=FOVY)
    mvp = (viewer.get_projection_matrix(FOVY, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    ctx = raster.RasterizerContext("cuda", dev)
    with torch.no_grad():
        img = viewer.render_textured(mesh, kd, mvp, SIZE, SIZE, ssaa=1, antialias=False, ctx=ctx)
        rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), mesh.t_pos_idx, (SIZE, SIZE))
        uv, _ = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)
    return dict(g=g, m=m, cache=cache, obj=str(d / out.save_name), mesh=mesh, kd=kd, mvp=mvp, ctx=ctx, img=img,
                rast=rast, uv=uv, covered=rast[..., 3] > 0)


def test_loaded_asset_is_the_exported_one(scene):
    mesh, kd = scene["mesh"], scene["kd"]
    assert kd.shape == (N_TEX, N_TEX, 3) and kd.min() >= 0 and kd.max() <= 1
    assert mesh.t_tex_idx.shape == mesh.t_pos_idx.shape and mesh.v_tex.min() >= 0 and mesh.v_tex.max() <= 1
    assert scene["img"].shape == (2, SIZE, SIZE, 3)
    n = scene["covered"].flatten(1).sum(1)
    assert (n > 0.05 * SIZE * SIZE).all(), n  # both views see the object
    assert (scene["img"][~scene["covered"]] == 1.0).all()  # the background, untouched without antialiasing


def test_render_equals_the_restatement_at_the_same_uv(scene):
    """covered pixels of the render = the float64 restatement sampling the same map at the same (interpolated) uv;
    1e-5 max|tex| with max|tex| <= 1 (u TW - 0.5 is exact in fp32 for TW = 512: only the weight products round)"""
    cov = scene["covered"].cpu()
    want = TR.texture(scene["kd"][None].cpu(), scene["uv"].cpu(), "linear", "clamp")
    err = (scene["img"].cpu().double() - want)[cov].abs().max().item()
    print(f"render vs restatement at {int(cov.sum())} covered pixels: max {err:.2e}")
    assert err <= 1e-5


def test_baked_texture_equals_the_decoded_field_at_the_surface(scene):
    """at covered pixels: decode material.export(geometry.export(p)) at p = interpolate(v_pos).  Mean absolute
    difference <= 0.02, the bar of tests/test_gpu_export.py for texture vs decode; p99 and max are decided by chart
    seams (a pixel whose taps reach into the padding) and are printed, not asserted."""
    mesh, cov = scene["mesh"], scene["covered"]
    with torch.no_grad():
        p, _ = scene["ctx"].interpolate(mesh.v_pos[None], scene["rast"], mesh.t_pos_idx)
        want = scene["m"].export(**scene["g"].export(points=p[cov], space_cache=scene["cache"][:1]))["albedo"]
    err = (scene["img"][cov] - want).abs().flatten().double()
    mean, p99, mx = err.mean().item(), torch.quantile(err, 0.99).item(), err.max().item()
    print(f"bake vs decode at {int(cov.sum())} covered pixels: mean {mean:.4f} p99 {p99:.4f} max {mx:.4f}")
    assert mean <= 0.02


def test_gradient_to_the_texture(scene):
    """loss = sum(rgb mask) before the background lerp: every covered pixel hands out weights that sum to 1 per
    channel (clamp), so grad map_Kd sums to 3 n_covered; texels outside every pixel's four taps get exactly 0"""
    kd = scene["kd"].clone().requires_grad_(True)
    uv, cov = scene["uv"], scene["covered"]
    rgb = raster.texture(kd[None], uv, boundary_mode="clamp")
    (rgb * cov[..., None].float()).sum().backward()
    n_cov = int(cov.sum())
    assert abs(kd.grad.double().sum().item() - 3 * n_cov) <= 1e-5 * 3 * n_cov
    x = (uv[cov].double().cpu() * N_TEX - 0.5).floor().long()
    touched = torch.zeros(N_TEX, N_TEX, dtype=torch.bool)
    for dy in (0, 1):
        for dx in (0, 1):
            touched[(x[:, 1] + dy).clamp(0, N_TEX - 1), (x[:, 0] + dx).clamp(0, N_TEX - 1)] = True
    grad = kd.grad.cpu()
    assert torch.count_nonzero(grad[~touched]) == 0
    assert (grad[touched].abs().sum(-1) > 0).float().mean() > 0.9  # (a tap with weight exactly 0 receives nothing)


def test_gradient_to_the_vertices(scene):
    src = scene["mesh"]
    mesh = Mesh(src.v_pos.clone().requires_grad_(True), src.t_pos_idx)
    mesh._v_tex, mesh._t_tex_idx = src.v_tex, src.t_tex_idx
    viewer.render_textured(mesh, scene["kd"], scene["mvp"], SIZE, SIZE, ctx=scene["ctx"]).sum().backward()
    assert torch.isfinite(mesh.v_pos.grad).all() and torch.count_nonzero(mesh.v_pos.grad) > 0


def test_normal_mode_and_supersampling(scene):
    with torch.no_grad():
        nrm = viewer.render_textured(scene["mesh"], None, scene["mvp"], SIZE, SIZE, mode="normal", ssaa=2)
    assert nrm.shape == (2, SIZE, SIZE, 3) and nrm.min() >= 0 and nrm.max() <= 1
    inside = F.avg_pool2d(scene["covered"][:, None].float(), 3, 1, 1)[:, 0] == 1  # away from the silhouette
    n = nrm[inside] * 2 - 1
    assert (n.norm(dim=-1) - 1).abs().mean() < 0.05  # the average of 2 x 2 unit normals, nearly unit on a smooth surface


def test_turntable(scene):
    with torch.no_grad():
        imgs = viewer.turntable(scene["mesh"], scene["kd"], n_views=4, height=SIZE, width=SIZE)
    assert imgs.shape == (4, SIZE, SIZE, 3) and imgs.min() >= 0 and imgs.max() <= 1
    assert ((imgs < 1).flatten(1).sum(1) > 0.02 * SIZE * SIZE * 3).all()  # every view has covered pixels


def test_cli_writes_the_turntable_pngs(scene, tmp_path):
    out = tmp_path / "views"
    r = subprocess.run([sys.executable, "-m", "triplaneturbo_amd.viewer", scene["obj"], "--out", str(out), "--size", "96",
                        "--ssaa", "2", "--normal"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(out)) == sorted([f"{k}_{i}.png" for k in ("rgb", "normal") for i in range(4)])
    for i in range(4):
        img = read_png(str(out / f"rgb_{i}.png"))
        assert img.shape == (96, 96, 3) and (img < 255).any()
