"""Dev tool: mesh simplification (ops.mesh_simplify) on the 160^3 scenes of tools/time_export.py (random planes, the
bench scene; and the same planes drawn at 8^2 and upsampled) at grids 32 / 64 / 128: HIP-event time of the whole call
and of its launches, vertex / face / cluster counts, and the UV atlas (ops.uv_atlas at 2048^2: time, charts, seams =
face pairs whose faces lie in different charts) of the mesh before and after.  Also the measured position deviation from
the float64 restatement (tests/simplify_reference.py), in units of the cell side h, on the cases of
tests/test_gpu_simplify.py and on the 160^3 scenes, where faces and vertex_map must be equal.  Medians over --reps after
one warm-up.

usage: python tools/time_simplify.py [--reps 10] [--out profiles/simplify.json]"""
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
import simplify_reference as S  # noqa: E402
from time_export import timed  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])

GRIDS = (32, 64, 128)
ATLAS = 2048


def deviation(mesh, grid):
    """max |v' - v'_ref| / h against the float64 restatement; faces, vertex_map and cluster count must be equal"""
    v2, t2, info = ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, grid)
    v_ref, t_ref, i_ref = S.simplify(mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy(), grid)
    same = (np.array_equal(t2.cpu().numpy(), t_ref) and info["n_clusters"] == i_ref["n_clusters"] and
            np.array_equal(info["vertex_map"].cpu().numpy(), i_ref["vertex_map"]))
    dev = float(np.abs(v2.cpu().numpy().astype(np.float64) - v_ref).max() / info["cell"]) if same and len(v_ref) else None
    return {"faces_and_map_equal": bool(same), "max_position_deviation_h": dev}


def atlas(mesh, reps):
    topo = mesh.topology
    try:
        t, (v_tex, t_tex, info) = timed(lambda: ops.uv_atlas(mesh.v_pos, mesh.t_pos_idx, topo, ATLAS, 2), reps)
    except RuntimeError as e:  # too many charts for the texture: reported, not timed
        return {"error": str(e)}
    pairs = topo.face_pairs.long()
    chart = info["chart"]
    seams = int((chart[pairs[:, 0]] != chart[pairs[:, 1]]).sum()) if len(pairs) else 0
    return {"uv_atlas_ms": t, "charts": info["charts"], "seams": seams, "fill_ratio": info["fill_ratio"],
            "overlap_rounds": info["overlap_rounds"]}


def measure(mesh, reps):
    res = {"V": int(mesh.v_pos.shape[0]), "T": int(mesh.t_pos_idx.shape[0]), "atlas_2048": atlas(mesh, reps),
           "grids": {}}
    for G in GRIDS:
        t, (v2, t2, info) = timed(lambda: ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, G), reps)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        for _ in range(reps):
            ops.mesh_simplify(mesh.v_pos, mesh.t_pos_idx, G)
        ops.set_kernel_timer(None)
        low = Mesh(v2, t2)
        r = {"simplify_ms": t, "launch_ms": {k: v[0] for k, v in timer.summary(median=True).items()},
             "V": int(v2.shape[0]), "T": int(t2.shape[0]), "clusters": info["n_clusters"], "cell": info["cell"],
             "atlas_2048": atlas(low, reps), **deviation(mesh, G)}
        res["grids"][G] = r
        a = r["atlas_2048"]
        print(f"G={G}: {t:.2f} ms, T {res['T']} -> {r['T']}, atlas "
              f"{a.get('uv_atlas_ms', float('nan')):.2f} ms charts {a.get('charts')} seams {a.get('seams')}, "
              f"deviation {r['max_position_deviation_h']} h, equal {r['faces_and_map_equal']}")
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
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "position_bar_h": 1e-3, "scenes": {}, "test_cases": {}}
    # the cases of tests/test_gpu_simplify.py
    worst = 0.0
    for name, G in S.CASES:
        v, tri = S.source_mesh(name)
        d = deviation(Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(np.asarray(tri)).to(dev).int()), G)
        out["test_cases"][f"{name}_G{G}"] = d
        worst = max(worst, d["max_position_deviation_h"] or 0.0)
        print(f"{name} G={G}: {d}")
    for scene, c in (("bench_random_planes_160", cache), ("smooth_planes_160", smooth)):
        print(f"## {scene}")
        (mesh,) = isosurface(c, g.forward_field, helper)
        out["scenes"][scene] = measure(mesh, a.reps)
        worst = max([worst] + [r["max_position_deviation_h"] or 0.0 for r in out["scenes"][scene]["grids"].values()])
    out["worst_position_deviation_h"] = worst
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
