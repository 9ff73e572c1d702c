"""Dev tool: latency of the HIP rasterizer (tt_rast_*, tt_interp_*, tt_aa_*; triplaneturbo_amd.raster) and of the
mesh renderer `generative-space-mesh-rasterize-renderer` at the training shape: 8 prompts x 4 views at 512^2, 128^3
marching cubes on the deformable grid, random planes, the hashgrid background (the reference config's renderer block).
HIP events, warm-up and repeats.  Each raster op forward and backward is timed on prompt 0's mesh and its 4 views;
the renderer's forward and forward + backward on all 8 prompts.  Per-kernel durations: run it under
`rocprofv3 --kernel-trace --stats` (profiles/mesh_render_512.json).

--batch-prompts times the renderer with `batch_prompts = True` (all prompts through one set of range-mode launches).

usage: python tools/time_mesh_render.py [--reps 20] [--batch-prompts] [--out profiles/mesh_render_512.json]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import raster, synthetic  # noqa: E402


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def perspective(fovy_deg, aspect, near=0.1, far=1000.0):
    t = math.tan(math.radians(fovy_deg) / 2)
    P = torch.zeros(4, 4)
    P[0, 0], P[1, 1] = 1 / (t * aspect), -1 / t
    P[2, 2], P[2, 3], P[3, 2] = -(far + near) / (far - near), -2 * far * near / (far - near), -1
    return P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--prompts", type=int, default=8)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--batch-prompts", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    rcfg = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    torch.manual_seed(0)
    g = tt.find(cfg["geometry_type"])(cfg["geometry"]).to(dev)
    m = tt.find(cfg["material_type"])(cfg["material"]).to(dev)
    b = tt.find(cfg["background_type"])(cfg["background"]).to(dev)
    r = tt.find(rcfg["renderer_type"])(rcfg["renderer"], geometry=g, material=m, background=b).to(dev)
    r.train()
    r.batch_prompts = a.batch_prompts
    P, NV, H = a.prompts, a.views, a.res
    rays_o, rays_d, c2w, dist = synthetic.make_cameras(P * NV, H, H, fovy_deg=60.0)
    mvp = (perspective(60.0, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    cpos = c2w[:, :3, 3].to(dev)
    cache = (torch.randn(P, 6, 32, 64, 64, device=dev) * 0.3).requires_grad_(True)
    text = torch.randn(P, 1024, device=dev)
    kw = dict(space_cache=cache, text_embed=text, rays_d_rasterize=rays_d.to(dev), camera_distances=dist.to(dev),
              c2w=c2w.to(dev))

    res = {"prompts": P, "views_per_prompt": NV, "height": H, "width": H,
           "isosurface_resolution": r.cfg.isosurface_resolution, "deformable_grid": True,
           "batch_prompts": bool(a.batch_prompts)}
    # the raster ops on prompt 0's mesh and views
    with torch.no_grad():
        mesh = r.isosurface(cache)[0]
    v = mesh.v_pos.detach()
    tri = mesh.t_pos_idx
    res["n_vert"], res["n_tri"] = int(v.shape[0]), int(tri.shape[0])
    pos = r.ctx.vertex_transform(v, mvp[:NV]).contiguous().requires_grad_(True)
    topo = mesh.topology.antialias_tables
    res["edge_topology"] = timed(  # the bare-tensor function: one sort, no validation
        lambda: raster.edge_topology(tri, v.shape[0]), a.reps)
    res["rasterize_fwd"] = timed(lambda: raster.rasterize(pos, tri, (H, H)), a.reps)
    rast = raster.rasterize(pos, tri, (H, H))
    res["covered_fraction"] = float((rast[..., 3] > 0).float().mean())
    g_r = torch.randn_like(rast)
    res["rasterize_bwd"] = timed(lambda: torch.autograd.grad(rast, pos, g_r, retain_graph=True), a.reps)
    attr = pos.detach()
    res["interpolate_fwd_C4"] = timed(lambda: raster.interpolate(attr, rast.detach(), tri), a.reps)
    attr_r = attr.clone().requires_grad_(True)
    rr = rast.detach().clone().requires_grad_(True)
    out_i = raster.interpolate(attr_r, rr, tri)
    g_i = torch.randn_like(out_i)
    res["interpolate_bwd_C4"] = timed(lambda: torch.autograd.grad(out_i, [attr_r, rr], g_i, retain_graph=True), a.reps)
    col = torch.rand(NV, H, H, 3, device=dev, requires_grad=True)
    res["antialias_fwd_C3"] = timed(lambda: raster.antialias(col, rast.detach(), pos, tri, topo), a.reps)
    out_a = raster.antialias(col, rast.detach(), pos, tri, topo)
    g_a = torch.randn_like(out_a)
    res["antialias_bwd_C3"] = timed(lambda: torch.autograd.grad(out_a, [col, pos], g_a, retain_graph=True), a.reps)

    # the renderer, all prompts
    def fwd():
        return r(mvp, cpos, cpos, H, H, **kw)

    def fwd_bwd():
        out = fwd()
        loss = out["comp_rgb"].mean() + out["opacity"].mean() + out["disparity"].mean() + \
            out["comp_normal_cam_vis"].mean() + sum(x.mean() for x in out["sdf"]) + \
            sum(x.square().mean() for x in out["sdf_grad"])
        loss.backward()

    reps = max(3, a.reps // 4)
    res["renderer_fwd"] = timed(fwd, reps, warmup=1)
    res["renderer_fwd_bwd"] = timed(fwd_bwd, reps, warmup=1)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
