"""Dev tool: mesh decimation (ops.mesh_decimate) on the two 160^3 meshes of profiles/mesh_distance.json (random planes,
the bench scene; and the same planes drawn at 8^2 and upsampled) at target_faces 20 000 and 5 000: HIP-event time of
the whole call, rounds, the share of that time spent in torch.sort, the launches' medians, the faces each method
actually produced, whether the result is a closed manifold (every edge two faces; Euler characteristic and components
where the mesh is small enough to count them on the host) and Mesh.distance_to the original -- next to the same numbers
for Mesh.simplify(target_faces=) at the same budget.  Then a sweep of TT_DECIMATE_QUANTILE x TT_DECIMATE_SELECT_PASSES
on the smaller mesh (the wrapper reads both through _lib at call time, so the sweep needs no rebuild).  Medians over
--reps after one warm-up.

usage: python tools/time_decimate.py [--reps 3] [--out profiles/mesh_decimate.json]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import _lib, ops  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, Mesh, isosurface  # noqa: E402
import decimate_reference as R  # noqa: E402
from time_export import timed  # noqa: E402

TARGETS = (20000, 5000)


def topology(mesh):
    """edge-face counts on the device; Euler characteristic and components on the host for a small mesh"""
    tri = mesh.t_pos_idx
    counts = ops.sort_face_edges(tri, mesh.v_pos.shape[0]).counts
    res = {"T": int(tri.shape[0]), "V": int(mesh.v_pos.shape[0]), "edges": int(counts.shape[0]),
           "edges_with_two_faces": int((counts == 2).sum()), "closed_manifold_edges": bool((counts == 2).all())}
    if tri.shape[0] <= 30000:
        _, res["euler_characteristic"], res["components"] = R.manifold_stats(tri.cpu().numpy())
    else:
        res["euler_characteristic"] = res["V"] - res["edges"] + res["T"]  # every vertex of these meshes is referenced
    return res


def distance(low, full):
    d = low.distance_to(full)
    return {"hausdorff": float(d["hausdorff"]), "rms_low_to_full": float(d["a_to_b"]["rms"]),
            "rms_full_to_low": float(d["b_to_a"]["rms"]), "spacing": float(d["spacing"])}


def sort_share(mesh, target):
    """ms inside torch.sort / ms of the whole call, one run with events around every sort"""
    real, spans = torch.sort, []

    def timed_sort(*a, **k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real(*a, **k)
        e1.record()
        spans.append((e0, e1))
        return out

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.sort = timed_sort
    try:
        a.record()
        ops.mesh_decimate(mesh.v_pos, mesh.t_pos_idx, target)
        b.record()
    finally:
        torch.sort = real
    torch.cuda.synchronize()
    total, sorts = a.elapsed_time(b), sum(x.elapsed_time(y) for x, y in spans)
    return {"total_ms": total, "sort_ms": sorts, "n_sorts": len(spans), "share": sorts / total}


def measure(mesh, reps):
    res = {"input": topology(mesh), "targets": {}}
    for target in TARGETS:
        t, (v2, t2, info) = timed(lambda: ops.mesh_decimate(mesh.v_pos, mesh.t_pos_idx, target), reps)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        ops.mesh_decimate(mesh.v_pos, mesh.t_pos_idx, target)
        ops.set_kernel_timer(None)
        launches = {k: {"median_ms": v[0], "launches": v[1]} for k, v in timer.summary(median=True).items()}
        low = Mesh(v2, t2)
        dec = {"ms": t, "n_rounds": info["n_rounds"], "stalled": info["stalled"], "n_locked": info["n_locked"],
               "torch_sort": sort_share(mesh, target), "launches": launches, **topology(low), **distance(low, mesh)}
        ts, simp = timed(lambda: mesh.simplify(target_faces=target), reps)
        clu = {"ms": ts, "grid": simp.extras["simplify"]["grid"], **topology(simp), **distance(simp, mesh)}
        res["targets"][target] = {"decimate": dec, "simplify_target_faces": clu}
        print(f"target {target}: decimate {t:.1f} ms, {info['n_rounds']} rounds, T {dec['T']}, closed "
              f"{dec['closed_manifold_edges']}, chi {dec.get('euler_characteristic')}, hausdorff {dec['hausdorff']:.5f}, "
              f"rms {dec['rms_low_to_full']:.5f} / {dec['rms_full_to_low']:.5f}, sort share "
              f"{dec['torch_sort']['share']:.2f} | simplify {ts:.1f} ms, T {clu['T']}, closed "
              f"{clu['closed_manifold_edges']}, hausdorff {clu['hausdorff']:.5f}, rms {clu['rms_low_to_full']:.5f} / "
              f"{clu['rms_full_to_low']:.5f}")
    return res


def sweep(mesh, target, reps):
    rows, keep = [], (_lib.TT_DECIMATE_QUANTILE, _lib.TT_DECIMATE_SELECT_PASSES)
    try:
        for q in (0.1, 0.25, 0.5, 0.75):
            for p in (1, 2, 3):
                _lib.TT_DECIMATE_QUANTILE, _lib.TT_DECIMATE_SELECT_PASSES = q, p
                t, (v2, t2, info) = timed(lambda: ops.mesh_decimate(mesh.v_pos, mesh.t_pos_idx, target), reps)
                d = distance(Mesh(v2, t2), mesh)
                rows.append({"quantile": q, "passes": p, "ms": t, "n_rounds": info["n_rounds"], "T": int(t2.shape[0]),
                             "hausdorff": d["hausdorff"], "rms_low_to_full": d["rms_low_to_full"]})
                print(f"quantile {q} passes {p}: {t:.1f} ms, {info['n_rounds']} rounds, hausdorff {d['hausdorff']:.5f}")
    finally:
        _lib.TT_DECIMATE_QUANTILE, _lib.TT_DECIMATE_SELECT_PASSES = keep
    return rows


@torch.no_grad()
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "constants": {"TT_DECIMATE_QUANTILE": _lib.TT_DECIMATE_QUANTILE,
                         "TT_DECIMATE_SELECT_PASSES": _lib.TT_DECIMATE_SELECT_PASSES}, "scenes": {}}
    meshes = {}
    for scene, c in (("smooth_planes_160", smooth), ("bench_random_planes_160", cache)):
        print(f"## {scene}")
        (mesh,) = isosurface(c, g.forward_field, helper)
        meshes[scene] = mesh
        out["scenes"][scene] = measure(mesh, a.reps)
        if a.out:  # what is measured so far survives a later failure
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(out, open(a.out, "w"), indent=1)
    print("## sweep, smooth_planes_160 -> 5000")
    out["sweep_smooth_planes_160_target_5000"] = sweep(meshes["smooth_planes_160"], 5000, a.reps)
    print(json.dumps(out))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
