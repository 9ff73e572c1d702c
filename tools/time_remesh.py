"""Dev tool: isotropic remeshing (ops.mesh_remesh) on the two 160^3 meshes of profiles/mesh_decimate.json (the same
planes drawn at 8^2 and upsampled; random planes, the bench scene) at two edge lengths: L from target_faces 20 000
(Mesh.remesh's estimate) and L = 1.0 x the mean edge.  HIP-event time of the whole call, the rounds of every phase and
iteration, the share of that time spent in torch.sort, the launches' medians, the figures of the issue's table for
input and output (share of short edges, long edges, minimum angles, valence deviation), whether the result is a closed
manifold, Mesh.distance_to the input -- and, for comparison, Mesh.decimate to the face count remeshing produced.
Nothing is asserted: there is nothing to compare a time against yet.  Medians over --reps after one warm-up.

usage: python tools/time_remesh.py [--reps 3] [--out profiles/mesh_remesh.json]"""
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
import remesh_reference as R  # noqa: E402
from time_decimate import distance, topology  # noqa: E402
from time_export import timed  # noqa: E402

TARGET_FACES = 20000


def quality(mesh, L):
    return R.quality(mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy(), L)


def sort_share(mesh, L):
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
        ops.mesh_remesh(mesh.v_pos, mesh.t_pos_idx, L)
        b.record()
    finally:
        torch.sort = real
    torch.cuda.synchronize()
    total, sorts = a.elapsed_time(b), sum(x.elapsed_time(y) for x, y in spans)
    return {"total_ms": total, "sort_ms": sorts, "n_sorts": len(spans), "share": sorts / total}


def measure(mesh, reps):
    mean_edge = R.mean_edge(mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy())
    p = mesh.v_pos[mesh.t_pos_idx.long()].double()
    area = 0.5 * float(torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1).norm(dim=-1).sum())
    res = {"input": dict(topology(mesh), mean_edge=mean_edge, area=area), "runs": {}}
    for name, L in ((f"target_faces_{TARGET_FACES}", ops.remesh_edge_length(area, TARGET_FACES)),
                    ("mean_edge_x1.0", mean_edge)):
        t, (v2, t2, info) = timed(lambda: ops.mesh_remesh(mesh.v_pos, mesh.t_pos_idx, L), reps)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        ops.mesh_remesh(mesh.v_pos, mesh.t_pos_idx, L)
        ops.set_kernel_timer(None)
        launches = {k: {"median_ms": v[0], "launches": v[1]} for k, v in timer.summary(median=True).items()}
        out = Mesh(v2, t2)
        run = {"edge_length": L, "L_over_mean_edge": L / mean_edge, "ms": t, "rounds": info["rounds"],
               "max_rounds": max(max(r.values()) for r in info["rounds"]), "split_passes": info["split_passes"],
               "n_split": info["n_split"], "n_collapsed": info["n_collapsed"], "n_flipped": info["n_flipped"],
               "n_reverted": info["n_reverted"], "n_locked": info["n_locked"], "split_capped": info["split_capped"],
               "rounds_capped": info["rounds_capped"], "torch_sort": sort_share(mesh, L), "launches": launches,
               "quality_in": quality(mesh, L), "quality_out": quality(out, L), **topology(out), **distance(out, mesh)}
        T = int(t2.shape[0])
        td, dec = timed(lambda: mesh.decimate(max(T, _lib.TT_DECIMATE_MIN_FACES)), reps)
        run["decimate_to_the_same_faces"] = {"ms": td, "n_rounds": dec.extras["decimate"]["n_rounds"],
                                             "stalled": dec.extras["decimate"]["stalled"], **topology(dec),
                                             "quality": quality(dec, L), **distance(dec, mesh)}
        res["runs"][name] = run
        qi, qo = run["quality_in"], run["quality_out"]
        print(f"{name}: L {L:.5f} ({L / mean_edge:.2f} x mean edge), {t:.1f} ms, rounds {info['rounds']}, "
              f"T {res['input']['T']} -> {T}, closed {run['closed_manifold_edges']}, short share "
              f"{qi['short_share']:.3f} -> {qo['short_share']:.3f}, long {qi['n_long']} -> {qo['n_long']}, min angle "
              f"{qi['min_angle_mean']:.1f} -> {qo['min_angle_mean']:.1f}, p5 {qi['min_angle_p5']:.1f} -> "
              f"{qo['min_angle_p5']:.1f}, valence {qi['valence_dev']:.2f} -> {qo['valence_dev']:.2f}, hausdorff "
              f"{run['hausdorff']:.5f}, sort share {run['torch_sort']['share']:.2f} | decimate {td:.1f} ms, T "
              f"{run['decimate_to_the_same_faces']['T']}, min angle "
              f"{run['decimate_to_the_same_faces']['quality']['min_angle_mean']:.1f}")
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
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "constants": {"TT_REMESH_MAX_ROUNDS": _lib.TT_REMESH_MAX_ROUNDS,
                         "TT_REMESH_MAX_SPLIT_PASSES": _lib.TT_REMESH_MAX_SPLIT_PASSES,
                         "TT_REMESH_DEFAULT_ITERATIONS": _lib.TT_REMESH_DEFAULT_ITERATIONS}, "scenes": {}}
    for scene, c in (("smooth_planes_160", smooth), ("bench_random_planes_160", cache)):
        print(f"## {scene}")
        (mesh,) = isosurface(c, g.forward_field, helper)
        out["scenes"][scene] = measure(mesh, a.reps)
        if a.out:  # what is measured so far survives a later failure
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
