"""Dev tool: the UV atlas (ops.uv_atlas) with method "axis" and "lscm" on the two 160^3 meshes of
profiles/mesh_decimate.json (random planes, the bench scene; and the same planes drawn at 8^2 and upsampled) at 2048^2,
and on the smooth scene's decimate(20000) result at 1024^2: HIP-event time of the whole call, CG iterations, charts and
how many fell back, overlap rounds, fill_ratio, and the per-face stretch of the atlas (area-weighted mean, p95 and max of
sigma1 / sigma2; p5 and p95 of the area ratio normalised by its area-weighted mean) by tests/uv_lscm_reference.py.
Before that, the solver against the dense float64 reference on the charts of tests/test_gpu_uv_lscm.py: the maximum
|uv - uv_ref| / chart extent, which that test takes its bound from ("solver_vs_reference").  Medians over --reps after
one warm-up.

usage: python tools/time_uv_atlas.py [--reps 3] [--out profiles/uv_lscm.json] [--solver-only]"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import _lib, ops  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, Mesh, isosurface  # noqa: E402
import uv_lscm_reference as L  # noqa: E402
from test_isosurface_oracle import sphere, torus, two_spheres  # noqa: E402
from time_export import timed  # noqa: E402


def solver_vs_reference(dev):
    cases = dict(L.explicit_cases())
    for name, level in (("sphere", sphere(48)), ("torus", torus(40)), ("two_spheres", two_spheres(40))):
        v, t = ops.marching_cubes(torch.from_numpy(level).to(dev))
        m = Mesh(v * 2 - 1, t)
        chart = ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 256, 2)[2]["chart"]
        cases[name] = (m.v_pos.cpu().numpy(), m.t_pos_idx.cpu().numpy().astype(np.int64),
                       chart.cpu().numpy().astype(np.int64))
    res = {}
    for name, (v, tri, chart) in cases.items():
        uv, _, info = ops.uv_flatten_lscm(torch.from_numpy(v).to(dev), torch.from_numpy(tri).int().to(dev),
                                          torch.from_numpy(chart).int().to(dev))
        ref = L.flatten(v, tri, chart)
        res[name] = {"rel_err": L.solver_error(uv.cpu().numpy(), ref), "charts": int(info["charts"]),
                     "largest_chart_vertices": int(np.bincount(ref["vchart_dense"]).max()),
                     "iterations": int(info["iterations"]), "fallbacks_gpu": int(info["fallback"].sum()),
                     "fallbacks_reference": int(ref["fallback"].sum())}
        print(f"solver vs reference, {name}: {res[name]}")
    return {"tol": _lib.TT_UV_LSCM_DEFAULT_TOL, "criterion": "max over charts of max |uv - uv_ref| / UV extent of the chart",
            "max_rel_err": max(r["rel_err"] for r in res.values()), "cases": res}


def stretch_stats(mesh, v_tex, t_tex):
    s1, s2, ratio, A = L.stretch(mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy(), v_tex.cpu().numpy(),
                                 t_tex.cpu().numpy())
    ok = (A > 0) & (s2 > 0)
    an, w, r = s1[ok] / s2[ok], A[ok], ratio[ok]
    r = r / ((w * r).sum() / w.sum())
    return {"anisotropy_mean": float((w * an).sum() / w.sum()), "anisotropy_p95": float(np.quantile(an, 0.95)),
            "anisotropy_max": float(an.max()), "area_ratio_p5": float(np.quantile(r, 0.05)),
            "area_ratio_p95": float(np.quantile(r, 0.95)), "flipped_faces": int((ratio[A > 0] <= 0).sum())}


def measure(mesh, N, reps):
    res = {"V": int(mesh.v_pos.shape[0]), "T": int(mesh.t_pos_idx.shape[0]), "texture_size": N}
    for method in ops.UV_METHODS:
        try:
            ms, (v_tex, t_tex, info) = timed(lambda: ops.uv_atlas(mesh.v_pos, mesh.t_pos_idx, mesh.topology, N, 2,
                                                                  method=method), reps)
        except RuntimeError as e:  # (too many charts for N)
            res[method] = {"error": str(e)}
            print(f"{method}: {e}")
            continue
        row = {"ms": ms, "charts": info["charts"], "overlap_rounds": info["overlap_rounds"],
               "fill_ratio": info["fill_ratio"], **stretch_stats(mesh, v_tex, t_tex)}
        if method == "lscm":
            ls = info["lscm"]
            row.update(cg_iterations=int(ls["iterations"]), fallbacks=int(ls["fallback"].sum()),
                       largest_chart_iterations=int(ls["chart_iterations"].max()))
        res[method] = row
        print(f"{method} at {N}^2: {row}")
    return res


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--solver-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "constants": {k: getattr(_lib, k) for k in ("TT_UV_LSCM_TILE", "TT_UV_LSCM_CHECK_EVERY",
                                                       "TT_UV_LSCM_DEFAULT_TOL", "TT_UV_LSCM_DEFAULT_MAX_ITERS")}}

    def save():  # what is measured so far survives a later failure
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(out, open(a.out, "w"), indent=1)

    out["solver_vs_reference"] = solver_vs_reference(dev)
    save()
    if not a.solver_only:
        torch.manual_seed(0)
        g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
        cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
        low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
        smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256)
        helper = DiffMarchingCubeHelper(160).to(dev)
        out["scenes"] = {}
        for scene, c in (("smooth_planes_160", smooth.to(dev)), ("bench_random_planes_160", cache)):
            print(f"## {scene}")
            (mesh,) = isosurface(c, g.forward_field, helper)
            out["scenes"][scene] = measure(mesh, 2048, a.reps)
            save()
            if scene == "smooth_planes_160":
                print("## smooth_planes_160, decimate(20000)")
                out["scenes"]["smooth_planes_160_decimate_20000"] = measure(mesh.decimate(20000), 1024, a.reps)
                save()
    print(json.dumps(out))
    save()


if __name__ == "__main__":
    main()
