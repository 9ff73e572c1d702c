"""Dev tool: the point-to-mesh distance kernels (ops.TriangleGrid, mesh_closest_point, point_mesh_distance2,
Mesh.simplify(max_error=)) on the smooth 160^3 scene of tools/time_normal_bake.py (planes drawn at 8^2 and upsampled) and
its grid-64 simplification.  Per mesh: grid build time, M / T, query time for 100 k and 1 M points (uniform in 1.1 x the
bounding box, and jittered surface samples, timed apart) with and without the cell-order sort, a sweep of G around the
default rule, backward time, and -- the yardstick, there being no parent-commit time for a new kernel -- the same query
as a chunked torch brute force in fp32 on the same GPU (the expression of tests/distance_reference.py) on a subset of
the points, with the per-point ratio.  On the full mesh also simplify(max_error = 2 isosurface cells) next to
simplify(target_faces = the face count it arrived at).  And the deviations from the float64 restatement on the cases of
tests/test_gpu_mesh_distance.py, in units of that file's bar 4e-6 * max(L_mesh, |p|_inf).  Medians over --reps after
one warm-up.

usage: python tools/time_mesh_distance.py [--reps 10] [--out profiles/mesh_distance.json]"""
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
import distance_reference as D  # noqa: E402
import simplify_reference as S  # noqa: E402
from time_export import timed  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])

BRUTE_POINTS = 2000
BRUTE_PAIRS = 4_000_000  # pairs per chunk of the torch brute force


def brute_force(points, mesh):
    """min over the triangles of the restatement's d2, fp32 on the GPU, in chunks of points"""
    tri = mesh.t_pos_idx.long()
    A, B, C = (mesh.v_pos[tri[:, k]][None] for k in range(3))
    step = max(1, BRUTE_PAIRS // tri.shape[0])
    return torch.cat([D.closest_point(points[i:i + step, None, :], A, B, C)[0].min(1)[0]
                      for i in range(0, points.shape[0], step)])


def make_points(mesh, n, seed):
    """{load: (n,3)}: "uniform" in 1.1 x the bounding box (most of it empty space, far from the surface) and
    "near_surface", surface samples jittered by 1 % of the diagonal (what distance_to and a surface loss send)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    lo, hi = mesh.v_pos.amin(0), mesh.v_pos.amax(0)
    mid, half = 0.5 * (lo + hi), 0.55 * (hi - lo)
    uni = mid + half * (torch.rand(n, 3, generator=g).to(lo.device) * 2 - 1)
    diag = float((hi - lo).norm())
    s = ops.mesh_surface_samples(mesh.v_pos, mesh.t_pos_idx, diag / 400)[0]
    pick = torch.randint(0, s.shape[0], (n,), generator=g).to(lo.device)
    near = s[pick] + 0.01 * diag * torch.randn(n, 3, generator=g).to(lo.device)
    return {"uniform": uni.contiguous(), "near_surface": near.contiguous()}


def measure(mesh, reps):
    T = int(mesh.t_pos_idx.shape[0])
    t_build, tg = timed(lambda: ops.TriangleGrid(mesh.v_pos, mesh.t_pos_idx), reps)
    res = {"V": int(mesh.v_pos.shape[0]), "T": T, "default_grid": tg.G, "build_ms": t_build, "M": tg.M,
           "M_over_T": tg.M / T, "query": {}, "grid_sweep_100k_ms": {}}
    pts = {n: make_points(mesh, n, 5) for n in (100_000, 1_000_000)}
    for n, loads in pts.items():
        r = {}
        for load, p in loads.items():
            if load == "uniform" and n > 100_000:  # seconds per launch: the 100 k figure says it all
                continue
            for name, order in (("plain", False), ("cell_order", True)):
                r[f"{load}_{name}_ms"] = timed(lambda: ops.mesh_closest_point(p, tg, cell_order=order), reps)[0]
        res["query"][str(n)] = r
        print(f"  query {n}: {r}")
    for G in sorted({max(tg.G // 2, 1), tg.G, min(2 * tg.G, 256), min(4 * tg.G, 256)}):
        g2 = ops.TriangleGrid(mesh.v_pos, mesh.t_pos_idx, grid=G)
        res["grid_sweep_100k_ms"][str(G)] = dict(
            {f"{load}_ms": timed(lambda: ops.mesh_closest_point(p, g2), reps)[0] for load, p in pts[100_000].items()},
            M_over_T=g2.M / T)
    print(f"  sweep: {res['grid_sweep_100k_ms']}")
    p = pts[100_000]["near_surface"]
    # backward through point_mesh_distance2 (the forward query excluded: timed around .backward())
    q = p.clone().requires_grad_(True)
    v = mesh.v_pos.clone().requires_grad_(True)

    def bwd():
        with torch.enable_grad():
            loss = ops.point_mesh_distance2(q, v, mesh.t_pos_idx, tg).sum()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        loss.backward()
        b.record()
        torch.cuda.synchronize()
        q.grad = v.grad = None
        return a.elapsed_time(b)

    bwd()
    res["backward_100k_ms"] = sorted(bwd() for _ in range(reps))[reps // 2]
    # the yardstick
    sub = p[:BRUTE_POINTS].contiguous()
    t_brute, d_brute = timed(lambda: brute_force(sub, mesh), max(reps // 3, 1))
    d_grid = ops.mesh_closest_point(sub, tg)[0]
    per_point_brute = t_brute / BRUTE_POINTS
    per_point_grid = res["query"]["100000"]["near_surface_plain_ms"] / 100_000
    res["torch_brute_force_fp32"] = {
        "points": BRUTE_POINTS, "ms": t_brute, "ms_per_1k_points": 1e3 * per_point_brute,
        "grid_query_ms_per_1k_points_at_100k": 1e3 * per_point_grid,
        "brute_over_grid_per_point": per_point_brute / per_point_grid,
        "max_abs_d_difference": float((d_brute.sqrt() - d_grid.sqrt()).abs().max())}
    print(f"  build {t_build:.3f} ms, M/T {tg.M / T:.2f}, backward {res['backward_100k_ms']:.3f} ms, brute force "
          f"{res['torch_brute_force_fp32']}")
    return res


def test_case_deviations(dev):
    """max |d - float64| in units of the tests' bar, on the meshes and points of tests/test_gpu_mesh_distance.py"""
    out = {}
    for name in ("sphere24", "torus32", "hand", "triangle", "two_clusters", "spanning", "one_octant"):
        hand_built = {"two_clusters": D.two_clusters, "spanning": D.spanning, "one_octant": D.one_octant}
        v, t = hand_built[name]() if name in hand_built else S.source_mesh(name)
        v, t = np.asarray(v, np.float32), np.asarray(t, np.int32)
        pts = D.query_points(v, t)
        if len(pts) * len(t) > 5_000_000:
            pts = np.concatenate([pts[:100], pts[1500:]])
        M = D.pair_matrix(pts, v, t).numpy()
        tg = ops.TriangleGrid(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev))
        d2, face, _ = ops.mesh_closest_point(torch.from_numpy(pts).to(dev), tg)
        d = d2.sqrt().double().cpu().numpy()
        ref = np.sqrt(M.min(1))
        bar = 4e-6 * np.maximum(np.abs(v).max(), np.abs(pts.astype(np.float64)).max(1))
        excess = np.sqrt(M[np.arange(len(pts)), face.cpu().numpy()]) - ref
        out[name] = {"N": len(pts), "T": len(t), "G": tg.G, "max_abs_error": float(np.abs(d - ref).max()),
                     "max_error_over_bar": float((np.abs(d - ref) / bar).max()), "max_face_excess": float(excess.max()),
                     "faces_differing_from_float64_argmin": float((face.cpu().numpy() != M.argmin(1)).mean())}
        print(f"{name}: {out[name]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "default_grid_rule": "clamp(ceil(sqrt(T) / 8), 1, 256)", "bar": "4e-6 * max(L_mesh, |p|_inf)", "scenes": {}}
    with torch.no_grad():
        out["test_cases"] = test_case_deviations(dev)
        out["worst_error_over_bar"] = max(c["max_error_over_bar"] for c in out["test_cases"].values())
        g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
        low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
        smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
        (full,) = isosurface(smooth, g.forward_field, DiffMarchingCubeHelper(160).to(dev))
        full = Mesh(full.v_pos.detach(), full.t_pos_idx)
        simp = full.simplify(grid=64)
        for name, mesh in (("smooth_planes_160", full), ("smooth_planes_160_grid64", simp)):
            print(f"## {name}")
            out["scenes"][name] = measure(mesh, a.reps)
        # simplify by deviation next to simplify by face count, on the full mesh
        cell = 2.0 * float(g.cfg.radius) / 160
        t_err, by_err = timed(lambda: full.simplify(max_error=2 * cell), max(a.reps // 3, 1))
        n_faces = int(by_err.t_pos_idx.shape[0])
        t_cnt, by_cnt = timed(lambda: full.simplify(target_faces=n_faces), max(a.reps // 3, 1))
        err = by_err.extras["simplify"]["error"]
        out["simplify_max_error"] = {
            "max_error": 2 * cell, "isosurface_cell": cell, "total_ms": t_err, "grid": by_err.extras["simplify"]["grid"],
            "T": n_faces, "hausdorff": err["hausdorff"], "spacing": err["spacing"], "n_samples": list(err["n_samples"]),
            "a_to_b": {k: err["a_to_b"][k] for k in ("max", "mean", "rms")},
            "b_to_a": {k: err["b_to_a"][k] for k in ("max", "mean", "rms")},
            "simplify_target_faces_same_count_ms": t_cnt, "target_faces_grid": by_cnt.extras["simplify"]["grid"]}
        print(f"simplify: {out['simplify_max_error']}")
    faster = all(s["torch_brute_force_fp32"]["brute_over_grid_per_point"] > 1 for s in out["scenes"].values())
    out["grid_query_faster_than_brute_force_at_T_ge_10k"] = bool(faster)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
