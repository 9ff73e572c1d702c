"""Dev tool: ops.mesh_sdf_grid on the smooth 160^3 mesh of profiles/mesh_distance.json (random planes drawn at 8^2 and
upsampled, about 84 k faces) and on its decimate(20000), at R = 128 and 256, band = 3: HIP-event time of the whole
call (grid and tree built before), split by launch label into scatter (candidates: tt_sdfgrid_scatter / _corners),
distance (tt_dist_query on the candidates), winding (tt_wind_fast on them) and finish -- next to the same grid by the
composition it replaces, mesh.signed_distance on all R^3 corners in chunks, on the same box.  Medians over --reps
after one warm-up.  A first measurement: neither side had been timed before, so the ratio is recorded, not judged.

usage: python tools/time_sdf_grid.py [--reps 3] [--out profiles/mesh_sdf_grid.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import ops  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface  # noqa: E402
from time_export import timed  # noqa: E402

RESOLUTIONS, BAND, CHUNK = (128, 256), 3.0, 1 << 21
PARTS = {"sdfgrid_scatter": "scatter", "sdfgrid_corners": "scatter", "dist_query": "distance", "wind_fast": "winding",
         "sdfgrid_finish": "finish"}


def composition(mesh, info, R):
    """the clamped signed distance of every corner by the existing queries, in chunks of CHUNK points"""
    idx = torch.stack(torch.meshgrid(*[torch.arange(R, device=mesh.v_pos.device)] * 3, indexing="ij"), -1)
    P = (info["lo"] + idx.float() * info["h"]).view(-1, 3)
    out = torch.cat([mesh.signed_distance(P[i:i + CHUNK]) for i in range(0, P.shape[0], CHUNK)])
    return out.clamp(-info["tau"], info["tau"]).view(R, R, R)


def measure(mesh, reps):
    mesh.triangle_grid, mesh.winding_tree  # built once, outside every timing
    res = {"T": int(mesh.t_pos_idx.shape[0]), "V": int(mesh.v_pos.shape[0]), "resolutions": {}}
    for R in RESOLUTIONS:
        t, (level, info) = timed(lambda: mesh.sdf_grid(R, BAND), reps)
        parts = {}
        for _ in range(reps):
            timer = ops.KernelTimer()
            ops.set_kernel_timer(timer)
            mesh.sdf_grid(R, BAND)
            ops.set_kernel_timer(None)
            run = {}
            for label, (ms, n) in timer.summary().items():
                run[PARTS.get(label, label)] = run.get(PARTS.get(label, label), 0.0) + ms * n
            for k, v in run.items():
                parts.setdefault(k, []).append(v)
        parts = {k: sorted(v)[len(v) // 2] for k, v in parts.items()}
        tc, ref = timed(lambda: composition(mesh, info, R), reps)
        row = {"ms": t, "parts_ms": parts, "band_corners": info["band_corners"], "candidates": info["candidates"],
               "corners": R ** 3, "composition_ms": tc, "composition_over_grid": tc / t,
               "equal_to_composition": bool(torch.equal(level, ref))}
        res["resolutions"][R] = row
        print(f"R {R}: sdf_grid {t:.2f} ms ({', '.join(f'{k} {v:.2f}' for k, v in parts.items())}), "
              f"{info['band_corners']} band corners of {R ** 3}; composition {tc:.2f} ms = {tc / t:.1f} x; "
              f"equal {row['equal_to_composition']}")
    return res


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
    (mesh,) = isosurface(smooth, g.forward_field, DiffMarchingCubeHelper(160).to(dev))
    out = {"device": torch.cuda.get_device_name(0), "band": BAND,
           "statistic": f"median of {a.reps} HIP-event times of whole calls, ms; parts: sums of their launches",
           "meshes": {}}
    for name, m in (("smooth_planes_160", mesh), ("smooth_planes_160_decimate_20000", mesh.decimate(20000))):
        print(f"## {name}")
        out["meshes"][name] = measure(m, a.reps)
        if a.out:  # what is measured so far survives a later failure
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
