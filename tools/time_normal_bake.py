"""Dev tool: the normal-map bake (tangents + projection + encode, ops.mesh_tangents / ops.bake_normal_map) on the 160^3
scenes of tools/time_export.py simplified to grid 64, at 1024^2, next to the existing colour bake (geometry.export +
material.export over the same texels) from the same run: HIP-event medians over --reps after one warm-up, the launches'
own times, the covered / back-facing texel counts and the |sdf| the projection leaves.  Also what the map is for
(`normal_errors`, shared with tests/test_gpu_normal_bake.py): the mean angle between the field's normal at the surface
and (a) the viewer's "normal_map" render, (b) its "normal" render of the low-poly mesh alone.

usage: python tools/time_normal_bake.py [--reps 10] [--out profiles/normal_bake.json]"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import ops, raster, synthetic, viewer  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface  # noqa: E402
from time_export import timed  # noqa: E402

GRID, SIZE = 64, 1024


@torch.no_grad()
def normal_errors(mesh, map_bump, field_fn, max_step, size=128, n_views=2, project_steps=2):
    """(e_map, e_low, pixels): over the interior covered pixels (covered, and so are their four neighbours) of n_views
    turntable views at size^2 without antialiasing, the mean angle in degrees between the field's unit normal at the
    pixel's surface point pulled onto the iso-surface (project_steps bounded Newton steps of at most max_step) and the
    viewer's mode "normal_map" (e_map) / mode "normal" (e_low).  field_fn(points (M,3)) -> (sdf, sdf_grad)."""
    dev = mesh.v_pos.device
    ctx = raster.RasterizerContext("cuda", dev)
    _, _, c2w, _ = synthetic.make_cameras(n_views, size, size, fovy_deg=40.0, elevation_deg=15.0)
    mvp = (viewer.get_projection_matrix(40.0, 1.0)[None] @ torch.inverse(c2w)).to(dev)
    kw = dict(antialias=False, ctx=ctx)
    img_map = viewer.render_textured(mesh, None, mvp, size, size, mode="normal_map", map_Bump=map_bump, **kw)
    img_low = viewer.render_textured(mesh, None, mvp, size, size, mode="normal", **kw)
    tri = mesh.t_pos_idx.int()
    rast, _ = ctx.rasterize(ctx.vertex_transform(mesh.v_pos, mvp), tri, (size, size))
    cov = rast[..., 3] > 0
    inner = cov.clone()
    inner[:, 1:] &= cov[:, :-1]
    inner[:, :-1] &= cov[:, 1:]
    inner[:, :, 1:] &= cov[:, :, :-1]
    inner[:, :, :-1] &= cov[:, :, 1:]
    inner[:, 0] = inner[:, -1] = False
    inner[:, :, 0] = inner[:, :, -1] = False
    pts = ctx.interpolate(mesh.v_pos[None], rast, tri)[0][inner].contiguous()
    for _ in range(project_steps):
        sdf, g = field_fn(pts)
        ops.bake_project_step(pts, sdf, g, max_step)
    ref = F.normalize(field_fn(pts)[1].reshape(-1, 3).float(), dim=-1)

    def angle(img):
        n = F.normalize(img[inner] * 2.0 - 1.0, dim=-1)
        return math.degrees(float(torch.acos((n * ref).sum(-1).clamp(-1.0, 1.0)).double().mean()))

    return angle(img_map), angle(img_low), int(inner.sum())


def measure(g, m, cache, helper, reps):
    (full,) = isosurface(cache, g.forward_field, helper)
    mesh = full.simplify(grid=GRID)
    res = {"full": {"V": int(full.v_pos.shape[0]), "T": int(full.t_pos_idx.shape[0])}, "grid": GRID,
           "cell": mesh.extras["simplify"]["cell"], "V": int(mesh.v_pos.shape[0]), "T": int(mesh.t_pos_idx.shape[0])}
    try:
        mesh.unwrap_uv(texture_size=SIZE)
    except RuntimeError as e:  # too many charts for the texture: reported, not timed
        res["error"] = str(e)
        return res
    ctx = raster.RasterizerContext()
    rast = ops.uv_rasterize(mesh.v_tex, mesh.t_tex_idx, SIZE)

    def field(p):
        out = g.forward(p[None], cache, output_normal=True)
        return out["sdf"], out["sdf_grad"]

    def colour_bake():
        gb_pos, _ = ctx.interpolate_one(mesh.v_pos, rast[None], mesh.t_pos_idx)
        return m.export(**g.export(points=gb_pos[0], space_cache=cache))["albedo"]

    def tangents():
        return ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm, "tex")

    t_tng, _ = timed(tangents, reps)
    t_bake, (bump, info) = timed(lambda: ops.bake_normal_map(mesh, field, SIZE, rast=rast), reps)
    t_kd, _ = timed(colour_bake, reps)
    t_fill, filled = timed(lambda: ops.texture_fill(bump, rast[..., 3] > 0), reps)
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    for _ in range(reps):
        tangents()
        ops.bake_normal_map(mesh, field, SIZE, rast=rast)
    ops.set_kernel_timer(None)
    launches = {k: v[0] for k, v in timer.summary(median=True).items() if k.startswith("bake_")}
    e_map, e_low, pixels = normal_errors(mesh, filled, field, mesh.extras["simplify"]["cell"], size=512)
    res.update(texture_size=SIZE, tangents_ms=t_tng, project_encode_ms=t_bake, normal_bake_ms=t_tng + t_bake,
               colour_bake_ms=t_kd, fill_ms=t_fill, launch_ms=launches,
               **{k: info[k] for k in ("n_covered", "n_backfacing", "mean_abs_sdf_before", "mean_abs_sdf_after")},
               mean_angle_deg={"normal_map": e_map, "low_poly": e_low, "pixels": pixels, "views": "2 x 512^2"})
    print(f"T {res['full']['T']} -> {res['T']}: tangents {t_tng:.2f} ms, projection + encode {t_bake:.2f} ms "
          f"(3 field queries), colour bake {t_kd:.2f} ms, fill {t_fill:.2f} ms; |sdf| {info['mean_abs_sdf_before']:.2e} "
          f"-> {info['mean_abs_sdf_after']:.2e}; back-facing {info['n_backfacing']} of {info['n_covered']}; "
          f"mean angle {e_map:.2f} deg with the map, {e_low:.2f} deg without")
    return res


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    m = tt.find("no-material")({}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms", "scenes": {}}
    for scene, c in (("bench_random_planes_160", cache), ("smooth_planes_160", smooth)):
        print(f"## {scene}")
        out["scenes"][scene] = measure(g, m, c, helper, a.reps)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
