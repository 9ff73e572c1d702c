"""Dev tool: the winding-number kernels (ops.WindingTree, mesh_winding_number exact / fast) on the two 160^3 scenes of
tools/time_simplify.py -- the bench mesh (random planes, 473 k faces) and the smooth scene (84 k faces) -- on the smooth
scene's grid-64 simplification (28 k faces) and on two meshes of the tests (torus32, 3 040 faces; sphere24, 1 772), each
with 100 k points near the surface and 100 k uniform in 1.1 x the box.  Per mesh: tree build time, exact and fast query time (with and without the
cell-order sort), a sweep of the tree depth L, the fast answer's deviation from the exact one at beta 2 and 3 and how
many points change side of 0.5, and -- the yardstick, there being no parent-commit time for a new capability -- the same
sum as a chunked torch brute force in fp32 on the same GPU (the expression of tests/winding_reference.py) on a subset
of the points, with the per-point ratio.  And, on the cases of tests/test_gpu_winding.py, the GPU's deviation from the
float64 restatement in units of that file's bar next to the restatement's own method error (CPU, float64).  Medians over
--reps after one warm-up.

usage: python tools/time_mesh_winding.py [--reps 5] [--out profiles/mesh_winding.json]"""
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
import winding_reference as W  # noqa: E402
from time_export import timed  # noqa: E402
from time_mesh_distance import make_points  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])

BAR = 1.7e-5  # tests/test_gpu_winding.py
BRUTE_POINTS = 2000
BRUTE_PAIRS = 4_000_000  # pairs per chunk of the torch brute force


def brute_force(points, mesh):
    """sum over the triangles of 2 atan2(num, den) / 4 pi, fp32 on the GPU, in chunks of points"""
    tri = mesh.t_pos_idx.long()
    A, B, C = (mesh.v_pos[tri[:, k]][None] for k in range(3))
    step = max(1, BRUTE_PAIRS // tri.shape[0])
    out = []
    for i in range(0, points.shape[0], step):
        p = points[i:i + step, None, :]
        a, b, c = A - p, B - p, C - p
        num = (a * torch.linalg.cross(b, c)).sum(-1)
        la, lb, lc = a.norm(dim=-1), b.norm(dim=-1), c.norm(dim=-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        out.append(torch.where(num == 0, torch.zeros_like(num), 2 * torch.atan2(num, den)).double().sum(1))
    return (torch.cat(out) / (4 * np.pi)).float()


def measure(mesh, reps):
    T = int(mesh.t_pos_idx.shape[0])
    t_build, tree = timed(lambda: ops.WindingTree(mesh.v_pos, mesh.t_pos_idx), reps)
    res = {"V": int(mesh.v_pos.shape[0]), "T": T, "default_levels": tree.L, "build_ms": t_build, "loads": {},
           "level_sweep_fast_ms": {}}
    pts = make_points(mesh, 100_000, 5)
    exact = {}
    for load, p in pts.items():
        t_exact, exact[load] = timed(lambda: ops.mesh_winding_number(p, tree, exact=True), max(reps // 3, 1))
        r = {"exact_ms": t_exact}
        for beta in (2.0, 3.0):
            t_fast, w = timed(lambda: ops.mesh_winding_number(p, tree, beta=beta), reps)
            dev = (w - exact[load]).abs()
            r[f"fast_beta{beta:g}_ms"] = t_fast
            r[f"fast_beta{beta:g}_max_abs_deviation"] = float(dev.max())
            r[f"fast_beta{beta:g}_mean_abs_deviation"] = float(dev.mean())
            r[f"fast_beta{beta:g}_points_changing_side"] = int(((w > 0.5) != (exact[load] > 0.5)).sum())
        r["fast_beta2_cell_order_ms"] = timed(lambda: ops.mesh_winding_number(p, tree, cell_order=True), reps)[0]
        r["exact_over_fast_beta2"] = t_exact / r["fast_beta2_ms"]
        res["loads"][load] = r
        print(f"  {load}: {r}")
    for L in range(max(W.default_levels(T) - 3, 0), ops._lib.TT_WIND_MAX_LEVELS + 1):
        t_b, t2 = timed(lambda: ops.WindingTree(mesh.v_pos, mesh.t_pos_idx, levels=L), max(reps // 3, 1))
        occupied = int((t2.level(L)[:, 3] >= 0).sum())
        row = {"build_ms": t_b, "occupied_leaves": occupied, "faces_per_occupied_leaf": T / max(occupied, 1)}
        for load, p in pts.items():
            t_fast, w = timed(lambda: ops.mesh_winding_number(p, t2), reps)
            row[f"{load}_ms"] = t_fast
            row[f"{load}_max_abs_deviation"] = float((w - exact[load]).abs().max())
        res["level_sweep_fast_ms"][str(L)] = row
        print(f"  L={L}: {row}")
    sub = pts["near_surface"][:BRUTE_POINTS].contiguous()
    t_brute, w_brute = timed(lambda: brute_force(sub, mesh), max(reps // 3, 1))
    per_point_brute = t_brute / BRUTE_POINTS
    res["torch_brute_force_fp32"] = {
        "points": BRUTE_POINTS, "ms": t_brute, "ms_per_1k_points": 1e3 * per_point_brute,
        "exact_ms_per_1k_points_at_100k": res["loads"]["near_surface"]["exact_ms"] / 100,
        "fast_ms_per_1k_points_at_100k": res["loads"]["near_surface"]["fast_beta2_ms"] / 100,
        "brute_over_exact_per_point": per_point_brute / (res["loads"]["near_surface"]["exact_ms"] / 100_000),
        "brute_over_fast_per_point": per_point_brute / (res["loads"]["near_surface"]["fast_beta2_ms"] / 100_000),
        "max_abs_difference_to_exact": float((w_brute - exact["near_surface"][:BRUTE_POINTS]).abs().max())}
    print(f"  build {t_build:.3f} ms, brute force {res['torch_brute_force_fp32']}")
    return res


def deviations_on_test_cases(dev):
    """the GPU against the float64 restatement on the cases of tests/test_gpu_winding.py"""
    out = {}
    for name in W.MESHES:
        v, t = W.mesh(name)
        pts, w, away, _ = W.case(name)
        vg, tg, p = torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(pts).to(dev)
        got = ops.mesh_winding_number(p, vg, tg, exact=True).double().cpu().numpy()
        row = {"N": len(pts), "T": len(t), "points_closer_than_1e-3_extents": float((~away).mean()),
               "exact_max_abs_error": float(np.abs(got - w)[away].max()),
               "exact_max_error_over_bar": float(np.abs(got - w)[away].max() / BAR), "fast": {}}
        for L in sorted({1, W.default_levels(len(t))}):
            tree = ops.WindingTree(vg, tg, levels=L)
            for beta in (2.0, 3.0):
                wf, margin, method_err = W.fast_case(name, L, beta)
                g = ops.mesh_winding_number(p, tree, beta=beta).double().cpu().numpy()
                sure = (margin > 1e-4) & away
                row["fast"][f"L{L}_beta{beta:g}"] = {
                    "method_error_float64_restatement": method_err,
                    "gpu_max_abs_deviation_from_exact": float(np.abs(g - w)[away].max()),
                    "gpu_vs_restatement_over_bar": float(np.abs(g - wf)[sure].max() / BAR),
                    "points_with_margin_below_1e-4_or_near": float((~sure).mean())}
        out[name] = row
        print(f"{name}: {row}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "default_levels_rule": "the smallest L with 6 * 4^L >= T, at most 6", "bar": BAR, "scenes": {}}
    with torch.no_grad():
        out["test_cases"] = deviations_on_test_cases(dev)
        out["worst_exact_error_over_bar"] = max(c["exact_max_error_over_bar"] for c in out["test_cases"].values())
        g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
        low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
        smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
        cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
        helper = DiffMarchingCubeHelper(160).to(dev)
        (bench,) = isosurface(cache, g.forward_field, helper)
        (full,) = isosurface(smooth, g.forward_field, helper)
        bench, full = Mesh(bench.v_pos.detach(), bench.t_pos_idx), Mesh(full.v_pos.detach(), full.t_pos_idx)
        small = {n: Mesh(*(torch.from_numpy(x).to(dev) for x in W.mesh(n))) for n in ("torus32", "sphere24")}
        for name, mesh in (("bench_random_planes_160", bench), ("smooth_planes_160", full),
                           ("smooth_planes_160_grid64", full.simplify(grid=64)), *small.items()):
            print(f"## {name}")
            out["scenes"][name] = measure(mesh, a.reps)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
