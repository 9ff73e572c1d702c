"""Dev tool: the ray-casting kernels (ops.mesh_ray_cast, mesh_ray_occluded, mesh_ambient_occlusion) on the two 160^3
scenes of tools/time_simplify.py -- the bench mesh (random planes, 473 k faces) and the smooth scene (84 k faces).  Per
mesh: closest hit and any hit for 100 k camera-like rays (four pinhole cameras around the object, 158^2 pixels each),
with and without the cell-order sort; the ambient-occlusion kernel for 100 k surface points at K = 64 with the default
ray length and bias; the sweep of the grid over sqrt(T) / 8, / 4, / 2 for both loads (the mesh keeps ONE grid, the
distance query's sqrt(T) / 8, whatever the sweep prefers for rays: the record says which it prefers); and -- the
yardstick, there being no parent-commit time for a new capability -- the same closest hit as a chunked torch brute force
(Moeller-Trumbore, fp32, on the same GPU) and through the kernel at G = 1, both on a subset of the rays, with the
per-ray ratios.  And, on the cases of tests/test_gpu_ray.py, the GPU's deviation from the float64 reference in units of
that file's bar.  Medians over --reps after one warm-up.

usage: python tools/time_mesh_ray.py [--reps 5] [--out profiles/mesh_raycast.json]"""
import argparse
import json
import math
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
import ray_reference as R  # noqa: E402
from time_export import timed  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])

BRUTE_RAYS = 2000
BRUTE_PAIRS = 4_000_000  # pairs per chunk of the torch brute force
K = 64


def brute_force(o, d, mesh):
    """nearest t >= 0 over the triangles, Moeller-Trumbore in fp32 on the GPU, in chunks of rays; inf for a miss"""
    tri = mesh.t_pos_idx.long()
    a, b, c = (mesh.v_pos[tri[:, k]][None] for k in range(3))
    e1, e2 = b - a, c - a
    step = max(1, BRUTE_PAIRS // tri.shape[0])
    out = []
    for i in range(0, o.shape[0], step):
        oo, dd = o[i:i + step, None, :], d[i:i + step, None, :]
        p = torch.linalg.cross(dd.expand(-1, e2.shape[1], -1), e2.expand(dd.shape[0], -1, -1))
        det = (e1 * p).sum(-1)
        s = oo - a
        u = (s * p).sum(-1) / det
        q = torch.linalg.cross(s, e1.expand(s.shape[0], -1, -1))
        v = (dd * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
        ok = (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)
        out.append(torch.where(ok, t, torch.full_like(t, float("inf"))).min(1)[0])
    return torch.cat(out)


def camera_rays(mesh, n_side=158, n_cams=4):
    """(origins, dirs) of n_cams pinhole cameras on a circle of 1.5 bounding-box diagonals about the centre, 40 degrees"""
    lo, hi = mesh.v_pos.amin(0), mesh.v_pos.amax(0)
    mid, diag = 0.5 * (lo + hi), float((hi - lo).norm())
    dev = mid.device
    half = math.tan(math.radians(20.0))
    px = (torch.arange(n_side, device=dev, dtype=torch.float32) + 0.5) / n_side * 2 - 1
    yy, xx = torch.meshgrid(px, px, indexing="ij")
    o, d = [], []
    for k in range(n_cams):
        az = 2 * math.pi * k / n_cams + 0.3
        eye = mid + 1.5 * diag * torch.tensor([math.cos(az) * 0.95, math.sin(az) * 0.95, 0.3], device=dev)
        fwd = F.normalize(mid - eye, dim=0)
        right = F.normalize(torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], device=dev)), dim=0)
        up = torch.linalg.cross(right, fwd)
        dirs = fwd[None, None] + half * (xx[..., None] * right + yy[..., None] * up)
        o.append(eye.expand(n_side * n_side, 3))
        d.append(dirs.reshape(-1, 3))
    return torch.cat(o).contiguous(), torch.cat(d).contiguous()


def surface_points(mesh, n, seed):
    """n surface samples with their face normals (unnormalised)"""
    lo, hi = mesh.v_pos.amin(0), mesh.v_pos.amax(0)
    s, face = ops.mesh_surface_samples(mesh.v_pos, mesh.t_pos_idx, float((hi - lo).norm()) / 400)
    pick = torch.randint(0, s.shape[0], (n,), generator=torch.Generator().manual_seed(seed)).to(s.device)
    fv = mesh.v_pos[mesh.t_pos_idx[face[pick].long()].long()]
    nrm = torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    keep = nrm.abs().amax(-1) > 0
    return s[pick][keep].contiguous(), nrm[keep].contiguous()


def measure(mesh, reps):
    T = int(mesh.t_pos_idx.shape[0])
    t_build, tg = timed(lambda: ops.TriangleGrid(mesh.v_pos, mesh.t_pos_idx), reps)
    res = {"V": int(mesh.v_pos.shape[0]), "T": T, "default_grid": tg.G, "build_ms": t_build, "M_over_T": tg.M / T}
    o, d = camera_rays(mesh)
    p, n = surface_points(mesh, 100_000, 5)
    t_cast, (t, face, _) = timed(lambda: ops.mesh_ray_cast(o, d, tg), reps)
    res["camera_rays"] = {"N": int(o.shape[0]), "hit_fraction": float((face >= 0).float().mean()),
                          "closest_hit_ms": t_cast,
                          "closest_hit_cell_order_ms": timed(lambda: ops.mesh_ray_cast(o, d, tg, cell_order=True), reps)[0],
                          "any_hit_ms": timed(lambda: ops.mesh_ray_occluded(o, d, tg), reps)[0]}
    t_ao, ao = timed(lambda: ops.mesh_ambient_occlusion(p, n, tg, n_rays=K), reps)
    res["ambient_occlusion"] = {"N": int(p.shape[0]), "K": K, "rays": int(p.shape[0]) * K, "mean_ao": float(ao.mean()),
                                "ms": t_ao, "M_rays_per_s": p.shape[0] * K / t_ao / 1e3}
    print(f"  {res}")
    res["grid_sweep"] = {}
    for div in (8, 4, 2):
        G = int(min(max(math.ceil(math.sqrt(T) / div), 1), ops._lib.TT_DIST_MAX_GRID))
        t_b, g2 = timed(lambda: ops.TriangleGrid(mesh.v_pos, mesh.t_pos_idx, grid=G), max(reps // 3, 1))
        t_c, got = timed(lambda: ops.mesh_ray_cast(o, d, g2), reps)
        t_a, ao2 = timed(lambda: ops.mesh_ambient_occlusion(p, n, g2, n_rays=K), reps)
        row = {"grid": G, "build_ms": t_b, "M_over_T": g2.M / T, "closest_hit_ms": t_c, "ambient_occlusion_ms": t_a,
               "equal_to_default_grid": bool(torch.equal(got[1], face) and torch.equal(got[0], t) and
                                             torch.equal(ao2, ao))}
        res["grid_sweep"][f"sqrt(T)/{div}"] = row
        print(f"  sqrt(T)/{div}: {row}")
    best = min(res["grid_sweep"].items(), key=lambda kv: kv[1]["closest_hit_ms"])[0]
    best_ao = min(res["grid_sweep"].items(), key=lambda kv: kv[1]["ambient_occlusion_ms"])[0]
    res["grid_the_sweep_prefers"] = {"closest_hit": best, "ambient_occlusion": best_ao,
                                     "grid_kept": "sqrt(T)/8, the distance query's: one grid per mesh"}
    sub = torch.randperm(o.shape[0], generator=torch.Generator().manual_seed(1))[:BRUTE_RAYS].to(o.device)
    so, sd = o[sub].contiguous(), d[sub].contiguous()
    t_brute, tb = timed(lambda: brute_force(so, sd, mesh), max(reps // 3, 1))
    g1 = ops.TriangleGrid(mesh.v_pos, mesh.t_pos_idx, grid=1)
    t_g1, got1 = timed(lambda: ops.mesh_ray_cast(so, sd, g1), max(reps // 3, 1))
    both = torch.isfinite(tb) & (face[sub] >= 0)
    res["yardsticks"] = {
        "rays": BRUTE_RAYS, "torch_brute_force_fp32_ms": t_brute, "kernel_grid1_ms": t_g1,
        "grid_ms_per_1k_rays_at_100k": t_cast / (o.shape[0] / 1000),
        "brute_over_grid_per_ray": (t_brute / BRUTE_RAYS) / (t_cast / o.shape[0]),
        "grid1_over_grid_per_ray": (t_g1 / BRUTE_RAYS) / (t_cast / o.shape[0]),
        "grid1_equal_to_grid": bool(torch.equal(got1[1], face[sub]) and torch.equal(got1[0], t[sub])),
        "rays_hit_by_both": int(both.sum()),
        "max_rel_t_difference_to_brute": float(((tb - t[sub]).abs() / t[sub])[both].max()) if bool(both.any()) else None}
    print(f"  yardsticks: {res['yardsticks']}")
    return res


def deviations_on_test_cases(dev):
    """the GPU against the float64 reference on the committed rays of tests/test_gpu_ray.py, in units of its bars"""
    out = {}
    for name in ("tetra", "cube", "lattice", "sphere24"):
        v, tri = R.mesh(name)
        o, d, c = R.case(name)
        tg = ops.TriangleGrid(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev))
        t, face, bary = (x.cpu().numpy() for x in ops.mesh_ray_cast(torch.from_numpy(o).to(dev),
                                                                    torch.from_numpy(d).to(dev), tg))
        rt, rf, rb = R.restated(name)
        m = ~c["unclean"] & (face >= 0)
        out[name] = {"rays": len(o), "T": len(tri), "unclean": int(c["unclean"].sum()), "clean_hits": int(m.sum()),
                     "faces_equal_on_clean_rays": bool(np.array_equal(face[~c["unclean"]], c["face"][~c["unclean"]])),
                     "max_t_error_over_bar": float((np.abs(t[m].astype(np.float64) - c["t"][m]) / c["s"][m]).max() / R.T_BAR),
                     "restatement_max_t_error_over_bar": float(
                         (np.abs(rt[m].astype(np.float64) - c["t"][m]) / c["s"][m]).max() / R.T_BAR),
                     "max_hit_point_residual": float(R.point_residual(o, d, v, tri, t, face, bary)[m].max()),
                     "restatement_max_hit_point_residual": float(R.point_residual(o, d, v, tri, rt, rf, rb)[m].max()),
                     "bitwise_equal_to_fp32_restatement": bool(np.array_equal(t.view(np.uint32), rt.view(np.uint32)) and
                                                               np.array_equal(face, rf))}
        print(f"{name}: {out[name]}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    out = {"device": torch.cuda.get_device_name(0), "statistic": f"median of {a.reps} HIP-event times, ms",
           "grid_rule": "clamp(ceil(sqrt(T) / 8), 1, 256), the TriangleGrid's one grid", "t_bar": "1e-6 (L + |o|_inf) / |d|",
           "scenes": {}}
    with torch.no_grad():
        out["test_cases"] = deviations_on_test_cases(dev)
        g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
        low = torch.randn(1, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
        smooth = F.interpolate(low, size=(256, 256), mode="bilinear", align_corners=True).reshape(1, 6, 32, 256, 256).to(dev)
        cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
        helper = DiffMarchingCubeHelper(160).to(dev)
        (bench,) = isosurface(cache, g.forward_field, helper)
        (full,) = isosurface(smooth, g.forward_field, helper)
        bench, full = Mesh(bench.v_pos.detach(), bench.t_pos_idx), Mesh(full.v_pos.detach(), full.t_pos_idx)
        for name, mesh in (("smooth_planes_160", full), ("bench_random_planes_160", bench)):
            print(f"## {name}")
            out["scenes"][name] = measure(mesh, a.reps)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
