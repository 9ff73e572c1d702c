"""Dev tool: latency of the marching-cubes mesh extraction (tt_mc_*, triplaneturbo_amd.isosurface) at the exporter's
resolution on one random sphere-biased cache (as tests/test_gpu_baseline_configs.py::test_config4_...), with HIP events,
warm-up and repeats.  Reports the count launch (k_mc_classify + k_compact2_blocks), the 8-byte read-back, the emit, the
backward, the extraction end to end (ops.marching_cubes forward) and isosurface() + colorize_mesh() for one prompt, and
a bytes roofline of the kernels (algorithmic bytes from the shapes and V / T over the kernel time, against the HBM peak).
Per-kernel durations of the two count kernels: run it under `rocprofv3 --kernel-trace --stats`.

usage: python tools/time_isosurface.py [--res 160] [--reps 50] [--out profiles/isosurface_160.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import _lib, ops  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, colorize_mesh, isosurface  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])

HBM_PEAK = 8.0e12      # MI355X HBM3E, spec
HBM_MEASURED = 6.29e12  # float4 copy


def timed(fn, reps, warmup=5):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=160)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    R = a.res
    helper = DiffMarchingCubeHelper(R).to(dev)
    pts = helper.grid_vertices.to(dev) * 2 - 1
    with torch.no_grad():
        sdf, deform = g.forward_field(pts[None], cache)
    level = sdf.reshape(R, R, R).contiguous()
    deform = deform.reshape(R, R, R, 3).contiguous()
    ws = torch.empty(_lib.load().tt_mc_workspace_bytes(R), device=dev, dtype=torch.uint8)
    totals = torch.empty(2, device=dev, dtype=torch.int32)
    count = lambda: ops._launch("tt_mc_count", level, R, 0.0, ws, totals)  # noqa: E731
    count()
    V, T = (int(x) for x in totals.cpu())
    v_pos = torch.empty(V, 3, device=dev)
    t_pos = torch.empty(T, 3, device=dev, dtype=torch.int32)
    g_v = torch.randn(V, 3, device=dev)
    g_level = torch.empty_like(level)
    g_def = torch.empty_like(deform)
    emit = lambda: ops._launch("tt_mc_emit", level, deform, R, 0.0, ws, v_pos, t_pos)  # noqa: E731
    bwd = lambda: ops._launch("tt_mc_bwd", level, deform, R, 0.0, ws, g_v, g_level, g_def)  # noqa: E731
    res = {"res": R, "n_points": R ** 3, "n_vert": V, "n_tri": T, "deformation": True,
           "workspace_bytes": int(ws.numel())}
    res["count_classify_scan"] = timed(count, a.reps)
    res["readback_8B"] = timed(lambda: totals.cpu(), a.reps)
    res["emit"] = timed(emit, a.reps)
    res["bwd"] = timed(bwd, a.reps)
    res["extract_end_to_end"] = timed(lambda: ops.marching_cubes(level, deform, 0.0), a.reps)
    with torch.no_grad():
        res["isosurface_plus_colorize_1_prompt"] = timed(
            lambda: colorize_mesh(cache, g.export, isosurface(cache, g.forward_field, helper), torch.sigmoid),
            max(5, a.reps // 5), warmup=2)
    N, nblk = R ** 3, (R ** 3 + 255) // 256
    byts = {
        # level read, mask + case + in-block offsets written, block totals; block scan
        "count_classify_scan": 4 * N + N + N + 4 * N + 4 * nblk + 4 * nblk + 8 * nblk,
        # masks, cases, offsets, level, deformation read; v_pos, t_pos_idx written
        "emit": N + N + 4 * N + 8 * nblk + 4 * N + 12 * N + 12 * V + 12 * T,
        # level, mask, offsets, deformation, grad_v read; grad_level, grad_deformation written
        "bwd": 4 * N + N + 4 * N + 8 * nblk + 12 * N + 12 * V + 4 * N + 12 * N,
    }
    res["roofline"] = {k: {"bytes": b, "gbps": b / (res[k]["median_ms"] * 1e-3) / 1e9,
                           "frac_hbm_peak": b / (res[k]["median_ms"] * 1e-3) / HBM_PEAK,
                           "frac_hbm_measured": b / (res[k]["median_ms"] * 1e-3) / HBM_MEASURED}
                       for k, b in byts.items()}
    res["kernels_ms"] = res["count_classify_scan"]["median_ms"] + res["emit"]["median_ms"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
