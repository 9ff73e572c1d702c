"""Dev tool: latency of the marching-tetrahedra mesh extraction (tt_mt_*, ops.TetGrid / ops.marching_tets) on the Kuhn
lattices of the training (128) and export (160) resolutions, on the sdf / deformation of one random sphere-biased cache
(as tools/time_isosurface.py), with HIP events, warm-up and repeats.  Per resolution it reports the one-off table build
(ops.TetGrid), the count launch (k_mt_classify + 2 x k_compact2_blocks), the 12-byte read-back, the emit, the backward,
the extraction end to end (ops.marching_tets forward + backward of sum(W * v_pos)), a bytes roofline of the three
entries (compulsory bytes from the shapes and V / T over the kernel time, against the measured copy ceiling), and two
baselines on the same GPU and field:
  torch_restatement   the reference algorithm (threestudio/models/isosurface.py:231-301) restated in torch: per call a
                      torch.unique(dim=0) over the six edges of every surface tet and the gather / mask / cat chain;
                      forward + autograd backward.  Its faces must equal the HIP faces (checked here).
  marching_cubes      ops.marching_cubes forward + backward on the same level and deformation at the same R.

usage: python tools/time_tets.py [--res 128 160] [--reps 30] [--out profiles/mt_isosurface.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import _lib, ops  # noqa: E402
from triplaneturbo_amd.isosurface import MarchingTetrahedraHelper, kuhn_tet_grid  # noqa: E402

HBM_MEASURED = 6.29e12  # float4 copy (tools/time_isosurface.py)

_BASE = [0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3]
_TABLE = [[-1] * 6, [1, 0, 2, -1, -1, -1], [4, 0, 3, -1, -1, -1], [1, 4, 2, 1, 3, 4], [3, 1, 5, -1, -1, -1],
          [2, 3, 0, 2, 5, 3], [1, 4, 0, 1, 5, 4], [4, 2, 5, -1, -1, -1], [4, 5, 2, -1, -1, -1], [4, 1, 0, 4, 5, 1],
          [3, 2, 0, 3, 5, 2], [1, 3, 5, -1, -1, -1], [4, 1, 2, 4, 3, 1], [3, 0, 4, -1, -1, -1], [2, 0, 1, -1, -1, -1],
          [-1] * 6]
_COUNT = [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]


def timed(fn, reps, warmup=3):
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


def torch_restatement(pos, level, tets, table, count):
    """The reference's per-call algorithm in torch ops: surface tets, their sorted edges, unique(dim=0), the crossing
    edges' interpolation, faces through the inverse map."""
    occ = level > 0
    occ4 = occ[tets]
    n_occ = occ4.sum(1)
    surface = (n_occ > 0) & (n_occ < 4)
    pairs = torch.sort(tets[surface][:, _BASE].reshape(-1, 2), dim=1)[0]
    uniq, inverse = torch.unique(pairs, dim=0, return_inverse=True)
    cross = occ[uniq].sum(1) == 1
    vertex_of = torch.full((uniq.shape[0],), -1, dtype=torch.long, device=pos.device)
    vertex_of[cross] = torch.arange(int(cross.sum()), device=pos.device)
    ids = vertex_of[inverse].reshape(-1, 6)
    a, b = uniq[cross].unbind(1)
    sa, sb = level[a], level[b]
    den = sa - sb
    v_pos = pos[a] * (-sb / den)[:, None] + pos[b] * (sa / den)[:, None]
    case = (occ4[surface] * torch.tensor([1, 2, 4, 8], device=pos.device)).sum(1)
    n_tri = count[case]
    one, two = n_tri == 1, n_tri == 2
    faces = torch.cat([torch.gather(ids[one], 1, table[case[one]][:, :3]),
                       torch.gather(ids[two], 1, table[case[two]]).reshape(-1, 3)])
    return v_pos, faces


def measure(R, reps, dev, g, cache):
    res = {"res": R}
    vertices, indices = kuhn_tet_grid(R)
    vertices, indices = vertices.to(dev), indices.to(dev)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    grid = ops.TetGrid(vertices, indices)
    b.record()
    torch.cuda.synchronize()
    res["tables_build_once_ms"] = a.elapsed_time(b)
    Nv, Ne, Nt = grid.n_vertices, grid.n_edges, grid.n_tets
    helper = MarchingTetrahedraHelper(R, tet_grid=grid).to(dev)
    with torch.no_grad():
        sdf, deform = g.forward_field((vertices * 2 - 1)[None], cache)
        level = sdf.reshape(Nv).contiguous()
        pos = (vertices + helper.normalize_grid_deformation(deform[0])).contiguous()
    ws = torch.empty(_lib.load().tt_mt_workspace_bytes(Ne, Nt), device=dev, dtype=torch.uint8)
    totals = torch.empty(3, device=dev, dtype=torch.int32)
    count = lambda: ops._launch("tt_mt_count", level, grid.edges, grid.tets, Ne, Nt, ws, totals)  # noqa: E731
    count()
    V, T1, T2 = (int(x) for x in totals.cpu())
    F = T1 + 2 * T2
    v_pos = torch.empty(V, 3, device=dev)
    t_pos = torch.empty(F, 3, device=dev, dtype=torch.int32)
    g_v = torch.randn(V, 3, device=dev)
    g_level, g_pos = torch.empty_like(level), torch.empty_like(pos)
    emit = lambda: ops._launch("tt_mt_emit", pos, level, grid.edges, grid.tet_edge, Ne, Nt, ws, v_pos,  # noqa: E731
                               t_pos)
    bwd = lambda: ops._launch("tt_mt_bwd", pos, level, grid.edges, grid.vert_ptr, grid.vert_col, Nv, Ne,  # noqa: E731
                              Nt, ws, g_v, g_level, g_pos)
    res.update(n_vertices=Nv, n_edges=Ne, n_tets=Nt, n_vert=V, n_tri=F, n_one_tri_tets=T1, n_two_tri_tets=T2,
               workspace_bytes=int(ws.numel()),
               table_bytes=sum(int(x.numel() * x.element_size()) for x in
                               (grid.tets, grid.edges, grid.tet_edge, grid.vert_ptr, grid.vert_col)))
    res["count_classify_scan"] = timed(count, reps)
    res["readback_12B"] = timed(lambda: totals.cpu(), reps)
    res["emit"] = timed(emit, reps)
    res["bwd"] = timed(bwd, reps)

    def fwd_bwd(extract):
        p, lv = pos.clone().requires_grad_(True), level.clone().requires_grad_(True)
        v, t = extract(p, lv)
        (v * g_v).sum().backward()
        return v, t

    res["extract_fwd_bwd"] = timed(lambda: fwd_bwd(lambda p, lv: ops.marching_tets(p, lv, grid)), reps)
    table = torch.tensor(_TABLE, device=dev)
    cnt = torch.tensor(_COUNT, device=dev)
    tets64 = indices.long()
    base = lambda p, lv: torch_restatement(p, lv, tets64, table, cnt)  # noqa: E731
    v_ref, t_ref = fwd_bwd(base)
    v_hip, t_hip = fwd_bwd(lambda p, lv: ops.marching_tets(p, lv, grid))
    assert torch.equal(t_ref.int(), t_hip), "the torch restatement and the HIP extraction disagree on the faces"
    res["max_abs_v_pos_vs_torch_restatement"] = (v_ref - v_hip).abs().max().item()
    res["torch_restatement_fwd_bwd"] = timed(lambda: fwd_bwd(base), max(5, reps // 3), warmup=2)
    lv3, df3 = level.reshape(R, R, R), deform[0].reshape(R, R, R, 3).contiguous()

    def mc():
        a_, b_ = lv3.clone().requires_grad_(True), df3.clone().requires_grad_(True)
        v, _ = ops.marching_cubes(a_, b_, 0.0)
        (v * v.detach()).sum().backward()

    res["marching_cubes_fwd_bwd"] = timed(mc, reps)
    nblk = (Ne + 255) // 256 + (Nt + 255) // 256
    surf = T1 + T2
    byts = {
        # edges, tets, level read; crossing flags, cases, in-block offsets, block totals written; the block scans
        "count_classify_scan": 8 * Ne + 16 * Nt + 4 * Nv + Ne + Nt + 4 * (Ne + Nt) + 4 * nblk + 12 * nblk,
        # flags and cases read; per crossing edge its offset, ends, two levels, two positions, the vertex written; per
        # surface tet its offset and six edge rows, per face three vertex offsets and the row written
        "emit": Ne + Nt + 8 * nblk + (4 + 8 + 8 + 24 + 12) * V + (4 + 24) * surf + (12 + 12) * F,
        # the CSR and a flag per incidence; per crossing incidence its offset, ends, two levels, two positions and the
        # vertex gradient; grad_level and grad_pos written
        "bwd": 4 * Nv + 4 * 2 * Ne + 2 * Ne + (4 + 8 + 8 + 24 + 12) * 2 * V + 16 * Nv,
    }
    res["roofline"] = {k: {"bytes": n, "gbps": n / (res[k]["median_ms"] * 1e-3) / 1e9,
                           "frac_copy_ceiling": n / (res[k]["median_ms"] * 1e-3) / HBM_MEASURED}
                       for k, n in byts.items()}
    res["speedup_vs_torch_restatement"] = (res["torch_restatement_fwd_bwd"]["median_ms"]
                                           / res["extract_fwd_bwd"]["median_ms"])
    res["ratio_to_marching_cubes"] = res["extract_fwd_bwd"]["median_ms"] / res["marching_cubes_fwd_bwd"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[128, 160])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    out = {"copy_ceiling_bytes_per_s": HBM_MEASURED, "grids": [measure(R, a.reps, dev, g, cache) for R in a.res]}
    line = json.dumps(out, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
