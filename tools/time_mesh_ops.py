"""Dev tool: HIP-event times of the mesh regularisers and outlier removal (tt_mesh_*) on the two meshes the package
makes, next to a torch restatement of the reference's formulation on the same GPU -> profiles/mesh_ops.json.

  renderer_128  generative-space-mesh-rasterize-renderer's isosurface at 128^3 (training config geometry)
  export_160    isosurface() at 160^3 (the exporter's resolution)

Per mesh: the topology build (torch sorts, once per mesh; MeshTopology's lazily derived face pairs, neighbour CSR and
workspace are touched inside the timed function, so the figure is both sorts and every tt_mesh_* table),
per-kernel-launch times (ops.KernelTimer labels),
end-to-end times of laplacian / normal consistency forward and forward+backward and of remove_outlier, and the
reference formulation restated in torch (threestudio/models/mesh.py: COO unique + coalesce + sparse mm for the
Laplacian, cosine_similarity over gathered edge normals; remove_outlier has no GPU counterpart in the reference).
Medians over --iters iterations after --warmup.

usage: python tools/time_mesh_ops.py [--iters 30] [--warmup 5] [--out profiles/mesh_ops.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import triplaneturbo_amd as tt  # noqa: E402
from triplaneturbo_amd import _lib, ops  # noqa: E402
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, Mesh, isosurface  # noqa: E402

if os.environ.get("TT_LIB_VARIANT"):  # dev A/B of an experiment build (tools/build_variants.py)
    _lib.use_variant(os.environ["TT_LIB_VARIANT"])


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def ref_laplacian(v_pos, t_pos_idx):
    """threestudio Mesh._laplacian_uniform + laplacian(), restated"""
    faces = t_pos_idx.long()
    V = v_pos.shape[0]
    with torch.no_grad():
        ii, jj = faces[:, [1, 2, 0]].flatten(), faces[:, [2, 0, 1]].flatten()
        adj = torch.stack([torch.cat([ii, jj]), torch.cat([jj, ii])], dim=0).unique(dim=1)
        vals = torch.ones(adj.shape[1]).to(v_pos)
        idx = torch.cat((adj, torch.stack((adj[0], adj[0]), dim=0)), dim=1)
        L = torch.sparse_coo_tensor(idx, torch.cat((-vals, vals)), (V, V)).coalesce()
    return L.mm(v_pos).norm(dim=1).mean()


def ref_edges(t_pos_idx):
    e = torch.cat([t_pos_idx[:, [0, 1]], t_pos_idx[:, [1, 2]], t_pos_idx[:, [2, 0]]], dim=0)
    return torch.unique(e.sort()[0], dim=0)


def ref_normal_consistency(v_nrm, edges):
    n = v_nrm[edges.long()]
    return (1.0 - torch.cosine_similarity(n[:, 0], n[:, 1], dim=-1)).mean()


def renderer_mesh(dev):
    tc = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    torch.manual_seed(0)
    g = tt.find(tc["geometry_type"])(tc["geometry"]).to(dev)
    m = tt.find(tc["material_type"])(tc["material"]).to(dev)
    b = tt.find(tc["background_type"])(tc["background"]).to(dev)
    r = tt.find(s["renderer_type"])(s["renderer"], geometry=g, material=m, background=b).to(dev)
    cache = torch.randn(1, 6, 32, 64, 64, device=dev) * 0.3
    with torch.no_grad():
        (mesh,) = r.isosurface(cache)
    return mesh, r.cfg.isosurface_resolution


def export_mesh(dev):
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    with torch.no_grad():
        (mesh,) = isosurface(cache, g.forward_field, DiffMarchingCubeHelper(160).to(dev))
    return mesh, 160


def measure(mesh, iters, warmup):
    v0, t = mesh.v_pos.detach(), mesh.t_pos_idx
    res = {"V": int(v0.shape[0]), "T": int(t.shape[0])}

    def build():  # MeshTopology derives these on first use: touch them, so the figure stays the whole build
        topo = ops.mesh_topology(t, v0.shape[0])
        return topo.face_pairs, topo.nbr_ptr, topo.ws

    res["topology_build_ms"] = timed(build, iters, warmup)
    topo = ops.mesh_topology(t, v0.shape[0])
    res["E"] = topo.n_edges
    v = v0.clone().requires_grad_(True)
    nrm = Mesh(v0, t).v_nrm.detach().clone().requires_grad_(True)

    def lap_fb():
        ops.mesh_laplacian_loss(v, topo).backward()

    def nc_fb():
        ops.mesh_normal_consistency_loss(nrm, topo).backward()

    def remove():
        ops.mesh_remove_small_components(v0, t, 0.01, topo)

    hip = {"laplacian_fwd_ms": timed(lambda: ops.mesh_laplacian_loss(v0, topo), iters, warmup),
           "laplacian_fwd_bwd_ms": timed(lap_fb, iters, warmup),
           "normal_consistency_fwd_ms": timed(lambda: ops.mesh_normal_consistency_loss(nrm.detach(), topo), iters,
                                              warmup),
           "normal_consistency_fwd_bwd_ms": timed(nc_fb, iters, warmup),
           "remove_outlier_0.01_ms": timed(remove, iters, warmup)}
    kt = ops.KernelTimer()
    ops.set_kernel_timer(kt)
    for _ in range(iters):
        lap_fb()
        nc_fb()
        remove()
    ops.set_kernel_timer(None)
    hip["per_launch_median_ms"] = {k: round(ms, 5) for k, (ms, n) in kt.summary(median=True).items()}
    res["hip"] = hip

    vr = v0.clone().requires_grad_(True)
    nr = nrm.detach().clone().requires_grad_(True)
    edges = ref_edges(t)

    def rl_fb():
        ref_laplacian(vr, t).backward()

    def rn_fb():
        ref_normal_consistency(nr, edges).backward()

    res["torch_reference_formulation"] = {
        "laplacian_fwd_ms": timed(lambda: ref_laplacian(v0, t), iters, warmup),
        "laplacian_fwd_bwd_ms": timed(rl_fb, iters, warmup),
        "edges_ms": timed(lambda: ref_edges(t), iters, warmup),
        "normal_consistency_fwd_ms (edges given)": timed(lambda: ref_normal_consistency(nr.detach(), edges), iters,
                                                         warmup),
        "normal_consistency_fwd_bwd_ms (edges given)": timed(rn_fb, iters, warmup)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ops.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup,
           "statistic": "median of per-iteration HIP-event times, ms", "meshes": {}}
    for name, make in (("renderer_128", renderer_mesh), ("export_160", export_mesh)):
        mesh, R = make(dev)
        out["meshes"][name] = dict(resolution=R, **measure(mesh, a.iters, a.warmup))
        print(name, json.dumps(out["meshes"][name]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
