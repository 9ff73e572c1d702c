"""Golden vectors of the reference's marching tetrahedra (run ONCE, on the CPU, next to a reference checkout).

    python tests/golden/make_golden_tets.py REFERENCE_CHECKOUT     ->  tests/golden/reference_tets.npz

Imports threestudio/models/isosurface.py (MarchingTetrahedraHelper :126-327) and threestudio/models/mesh.py from the
checkout, with the annotation stubs of make_golden_renderer.py for the packages they import but do not compute with,
and RUNS the helper on three small grids.  Nothing of the reference is copied: only DATA is written -- the inputs made
here and the reference's results.  Per case `c` the file holds
    c_resolution, c_vertices (Nv,3) f32, c_indices (Nt,4) i64, c_level (Nv,1) f32, c_deformation (Nv,3) f32 (the raw
    offsets that go through normalize_grid_deformation), c_W (V,3) f64
    c_all_edges (Ne,2) i64, c_v_pos / c_t_pos_idx (without deformation), c_v_pos_def / c_t_pos_idx_def (with it)
    c_g64_level, c_g64_level_def, c_g64_deformation and the same with g32: d sum(W * v_pos) / d (level, deformation)
    from the helper run in float64 / float32 (level alone for the run without deformation)
The cases: a noisy sphere on the 9^3 Kuhn lattice; a jittered 5^3 grid with its vertices relabelled and its tets and
their corners shuffled; a 7^3 field quantised to quarters so that it holds exact zeros.  Every crossing edge of every
case has |s_a - s_b| >= 1e-3 (asserted here), so the gradients are well conditioned in fp32."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from triplaneturbo_amd.isosurface import kuhn_tet_grid  # noqa: E402  (torch only: no GPU, no library)


def _reference_helper_class(ref):
    import importlib
    import make_golden_renderer as G
    G.REF = ref
    G._install_stubs()
    return importlib.import_module("threestudio.models.isosurface").MarchingTetrahedraHelper


def _cases():
    rng = np.random.default_rng(20)
    out = {}
    v, t = kuhn_tet_grid(9)
    v, t = v.numpy(), t.numpy()
    level = np.linalg.norm(v - 0.5, axis=1) - 0.31 + 0.03 * rng.standard_normal(len(v))
    out["sphere9"] = (9, v, t, level)

    v, t = kuhn_tet_grid(5)
    v, t = v.numpy().copy(), t.numpy().copy()
    v += rng.uniform(-0.06, 0.06, v.shape).astype(np.float32)
    relabel = rng.permutation(len(v))  # old id -> new id
    v2 = np.empty_like(v)
    v2[relabel] = v
    t = relabel[t][rng.permutation(len(t))]
    t = np.take_along_axis(t, np.argsort(rng.random(t.shape), axis=1), axis=1)  # corners of every tet shuffled
    level = np.sin(5.0 * v2[:, 0]) * np.cos(4.0 * v2[:, 1]) + v2[:, 2] - 0.5 + 0.05 * rng.standard_normal(len(v2))
    out["jitter5"] = (5, v2, t, level)

    v, t = kuhn_tet_grid(7)
    v, t = v.numpy(), t.numpy()
    f = np.linalg.norm((v - 0.5) * np.array([1.0, 1.3, 0.8]), axis=1) - 0.3 + 0.1 * np.sin(9.0 * v[:, 0])
    level = np.round(f * 4.0) / 4.0
    out["zeros7"] = (7, v, t, level)
    return {k: (r, v.astype(np.float32), t.astype(np.int64), lv.astype(np.float32).reshape(-1, 1))
            for k, (r, v, t, lv) in out.items()}


def main():
    Helper = _reference_helper_class(os.path.abspath(sys.argv[1]))
    import mt_reference as M
    res = {}
    rng = np.random.default_rng(21)
    for name, (R, vertices, indices, level) in _cases().items():
        deformation = (0.5 * rng.standard_normal(vertices.shape)).astype(np.float32)
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "tets.npz")
            np.savez(path, vertices=vertices, indices=indices)
            helper = Helper(R, path)
        lv, df = torch.from_numpy(level), torch.from_numpy(deformation)
        with torch.no_grad():
            plain, deformed = helper(lv.clone()), helper(lv.clone(), df)
        V = plain.v_pos.shape[0]
        assert V > 50 and deformed.v_pos.shape[0] == V and torch.equal(plain.t_pos_idx, deformed.t_pos_idx)
        W = rng.standard_normal((V, 3))
        res.update({f"{name}_resolution": np.asarray(R), f"{name}_vertices": vertices, f"{name}_indices": indices,
                    f"{name}_level": level, f"{name}_deformation": deformation, f"{name}_W": W,
                    f"{name}_all_edges": helper.all_edges.numpy(),
                    f"{name}_v_pos": plain.v_pos.numpy(), f"{name}_t_pos_idx": plain.t_pos_idx.numpy(),
                    f"{name}_v_pos_def": deformed.v_pos.numpy(), f"{name}_t_pos_idx_def": deformed.t_pos_idx.numpy()})
        # the conditioning the gradient tests rely on, on the oracle's crossing edges (= the reference's: pinned by
        # tests/test_tets_host.py)
        mt = M.marching_tets(vertices, level, indices)
        gap = np.abs(level[mt.a, 0] - level[mt.b, 0]).min()
        assert gap >= 1e-3, (name, gap)
        n_zero = int((level == 0).sum())
        for tag, dt in (("g64", torch.float64), ("g32", torch.float32)):
            h = helper.to(dt)  # the vertex buffer follows; the index buffers stay int64
            a = lv.to(dt).requires_grad_(True)
            (h(a).v_pos * torch.from_numpy(W).to(dt)).sum().backward()
            res[f"{name}_{tag}_level"] = a.grad.numpy()
            a, b = lv.to(dt).requires_grad_(True), df.to(dt).requires_grad_(True)
            (h(a, b).v_pos * torch.from_numpy(W).to(dt)).sum().backward()
            res[f"{name}_{tag}_level_def"], res[f"{name}_{tag}_deformation"] = a.grad.numpy(), b.grad.numpy()
        print(f"{name}: Nv {len(vertices)} Nt {len(indices)} Ne {len(res[name + '_all_edges'])} V {V} "
              f"T {plain.t_pos_idx.shape[0]} exact zeros {n_zero} min |s_a - s_b| {gap:.3g}")
    out = os.path.join(HERE, "reference_tets.npz")
    np.savez_compressed(out, **res)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
