"""Dev tool: HIP-event times of texture sampling (tt_tex_fwd / tt_tex_bwd, raster.texture) on render-shaped inputs, and
the bake-vs-decode error of a textured render of an exported scene -> profiles/texture.json.

  minify    4 x 512^2 pixels sample a 1024^2 x 3 map at the UVs of the bench mesh's atlas (the random-plane scene of
            tools/time_mesh_ops.py at 128^3, four turntable views): neighbouring pixels land texels apart
  magnify   the same pixels and UVs on a 64^2 x 3 map: many pixels share a texel (same-address atomics in the backward)

Uncovered pixels carry uv = 0 and grad_out = 0, as in a masked render.  Per case: forward and backward (grad_tex and
grad_uv) medians over --iters launches after --warmup, the forward's achieved bytes/s over the bytes it must move
(uv in, out out, the map once) against the HBM peak, and the backward's atomic adds per second (non-zero terms, 4 bytes
each) against the chip-wide float-atomic rate.  There is no bar: these are the first measurements of these kernels.

usage: python tools/time_texture.py [--iters 30] [--warmup 5] [--out profiles/texture.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import raster, synthetic, viewer  # noqa: E402
from triplaneturbo_amd.export import save_obj  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface  # noqa: E402

HBM_PEAK = 8.0e12     # bytes/s, MI355X spec
ATOMIC_RATE = 1.3e12  # bytes/s of fp32 atomic adds, chip-wide (measured: profiles/r06_atomic_bench.txt)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def bench_uv(dev, size=512, n_views=4):
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    with torch.no_grad():
        (mesh,) = isosurface(cache, g.forward_field, DiffMarchingCubeHelper(128).to(dev))
        mesh.unwrap_uv(texture_size=2048)  # the noise surface's ~55k charts do not fit 1024^2; the UVs are in [0, 1]
        _, _, c2w, _ = synthetic.make_cameras(n_views, size, size, fovy_deg=40.0)
        mvp = (viewer.get_projection_matrix(40.0, 1.0)[None] @ torch.inverse(c2w)).to(dev)
        ctx = raster.RasterizerContext("cuda", dev)
        rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), mesh.t_pos_idx, (size, size))
        uv, _ = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)
    return uv.contiguous(), (rast[..., 3:] > 0).float()


def measure(uv, mask, n_tex, iters, warmup):
    dev = uv.device
    B, H, W, _ = uv.shape
    tex = torch.rand(1, n_tex, n_tex, 3, device=dev)
    g_out = torch.randn(B, H, W, 3, device=dev) * mask
    tex_g, uv_g = tex.clone().requires_grad_(True), uv.clone().requires_grad_(True)
    out = raster.texture(tex_g, uv_g, boundary_mode="clamp")

    def bwd():
        torch.autograd.grad(out, (tex_g, uv_g), g_out, retain_graph=True)

    fwd_ms = timed(lambda: raster.texture(tex, uv, boundary_mode="clamp"), iters, warmup)
    bwd_ms = timed(bwd, iters, warmup)
    fwd_bytes = B * H * W * (8 + 12) + tex.numel() * 4
    n_atomics = int(mask.sum().item()) * 4 * 3  # upper bound: four taps x three channels per covered pixel
    return {"texture": [n_tex, n_tex, 3], "pixels": [B, H, W], "covered_fraction": round(mask.mean().item(), 4),
            "fwd_ms": round(fwd_ms, 5), "bwd_ms": round(bwd_ms, 5),
            "fwd_min_bytes": fwd_bytes, "fwd_bytes_per_s": round(fwd_bytes / (fwd_ms * 1e-3), 0),
            "fwd_fraction_of_hbm_peak": round(fwd_bytes / (fwd_ms * 1e-3) / HBM_PEAK, 4),
            "bwd_atomic_adds": n_atomics, "bwd_atomic_adds_per_s": round(n_atomics / (bwd_ms * 1e-3), 0),
            "bwd_fraction_of_atomic_rate": round(4 * n_atomics / (bwd_ms * 1e-3) / ATOMIC_RATE, 4)}


def bake_vs_decode(dev, tmp):
    """the scene of tests/test_gpu_textured_render.py: export at 512^2, save, load, render two 128^2 views without
    antialiasing, decode the field at the covered pixels' surface points"""
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=64), geometry=g, material=m, background=b).to(dev)
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    exp = tt.find("multiprompt-mesh-exporter")({"save_uv": True, "texture_size": 512, "texture_format": "png"},
                                               geometry=g, material=m, background=b)
    (out,) = exp(cache)
    save_obj(os.path.join(tmp, out.save_name), **out.params)
    mesh, kd = viewer.load_obj(os.path.join(tmp, out.save_name), device=dev)
    _, _, c2w, _ = synthetic.make_cameras(2, 128, 128, fovy_deg=40.0)
    mvp = (viewer.get_projection_matrix(40.0, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    ctx = raster.RasterizerContext("cuda", dev)
    with torch.no_grad():
        img = viewer.render_textured(mesh, kd, mvp, 128, 128, antialias=False, ctx=ctx)
        rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), mesh.t_pos_idx, (128, 128))
        cov = rast[..., 3] > 0
        p, _ = ctx.interpolate(mesh.v_pos[None], rast, mesh.t_pos_idx)
        want = m.export(**g.export(points=p[cov], space_cache=cache[:1]))["albedo"]
    err = (img[cov] - want).abs().flatten().double()
    return {"scene": "two prompts, 64^2 planes upsampled from 8^2, isosurface 64^3, map_Kd 512^2 PNG, 2 views at 128^2",
            "covered_pixels": int(cov.sum()), "mean_abs": round(err.mean().item(), 5),
            "p99_abs": round(torch.quantile(err, 0.99).item(), 5), "max_abs": round(err.max().item(), 5)}


def main():
    import tempfile
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    uv, mask = bench_uv(dev)
    res = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "statistic": "median of per-iteration HIP-event times, ms (backward = grad_tex + grad_uv, one launch + memset)",
           "backward_scatter": "plain fp32 atomic adds, no same-texel pre-reduction",
           "hbm_peak_bytes_per_s": HBM_PEAK, "atomic_rate_bytes_per_s": ATOMIC_RATE, "cases": {}}
    for name, n_tex in (("minify", 1024), ("magnify", 64)):
        res["cases"][name] = measure(uv, mask, n_tex, a.iters, a.warmup)
        print(name, json.dumps(res["cases"][name]))
    with tempfile.TemporaryDirectory() as tmp:
        res["bake_vs_decode"] = bake_vs_decode(dev, tmp)
    print("bake_vs_decode", json.dumps(res["bake_vs_decode"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
