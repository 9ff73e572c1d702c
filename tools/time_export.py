"""Dev tool: HIP-event times of the textured export's stages on the bench scene (random planes, the exporter's 160^3
marching-cubes helper) and on a smooth one (the planes drawn at 8^2 and upsampled): isosurface, UV atlas (ops.uv_atlas: labels, charts, host packing, emit, overlap guard), bake
(UV rasterize + position interpolate + geometry.export + material.export) and fill (ops.texture_fill), at 1024^2 and
2048^2, with the chart count, density, fill ratio and overlap rounds.  Medians over --reps after one warm-up.

usage: python tools/time_export.py [--reps 10] [--out profiles/export_160.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import ops, raster  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2], out


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
    # and a smooth object: the same planes drawn at 8^2 and upsampled (the bench scene's noise surface is the worst case)
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


def measure(g, m, cache, helper, reps):
    t_iso, meshes = timed(lambda: isosurface(cache, g.forward_field, helper), reps)
    mesh = meshes[0]
    ctx = raster.RasterizerContext()
    res = {"V": int(mesh.v_pos.shape[0]), "T": int(mesh.t_pos_idx.shape[0]), "isosurface_ms": t_iso, "sizes": {}}
    topo = mesh.topology
    for N in (1024, 2048):
        try:
            t_atlas, (v_tex, t_tex, info) = timed(lambda: ops.uv_atlas(mesh.v_pos, mesh.t_pos_idx, topo, N, 2), reps)
        except RuntimeError as e:  # too many charts for the texture: reported, not timed
            res["sizes"][N] = {"error": str(e)}
            continue

        def bake():
            uv = v_tex * 2.0 - 1.0
            uv4 = torch.cat((uv, torch.zeros_like(uv[..., :1]), torch.ones_like(uv[..., :1])), -1)
            rast, _ = ctx.rasterize_one(uv4, t_tex, (N, N))
            gb_pos, _ = ctx.interpolate_one(mesh.v_pos, rast[None], mesh.t_pos_idx)
            alb = m.export(**g.export(points=gb_pos[0], space_cache=cache))["albedo"]
            return alb, rast[..., 3] > 0

        t_bake, (alb, mask) = timed(bake, reps)
        t_fill, _ = timed(lambda: ops.texture_fill(alb, mask), reps)
        res["sizes"][N] = {"atlas_ms": t_atlas, "bake_ms": t_bake, "fill_ms": t_fill,
                           "atlas_bake_fill_ms": t_atlas + t_bake + t_fill, "charts": info["charts"],
                           "texels_per_unit": info["scale"], "fill_ratio": info["fill_ratio"],
                           "overlap_rounds": info["overlap_rounds"], "uv_vertices": int(v_tex.shape[0])}
    print("| size | atlas ms | bake ms | fill ms | total ms | charts | fill ratio | overlap rounds |")
    print("|---|---|---|---|---|---|---|---|")
    for N, r in res["sizes"].items():
        if "error" in r:
            print(f"| {N}^2 | {r['error']} |")
            continue
        print(f"| {N}^2 | {r['atlas_ms']:.2f} | {r['bake_ms']:.2f} | {r['fill_ms']:.2f} | {r['atlas_bake_fill_ms']:.2f} "
              f"| {r['charts']} | {r['fill_ratio']:.3f} | {r['overlap_rounds']} |")
    print(f"mesh V={res['V']} T={res['T']}, isosurface {t_iso:.2f} ms")
    return res


if __name__ == "__main__":
    main()
