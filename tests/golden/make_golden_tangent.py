"""Golden vectors of the reference's vertex tangents (run once, on the CPU, against a reference checkout).

    python tests/golden/make_golden_tangent.py REFERENCE_CHECKOUT   ->  tests/golden/reference_mesh_tangent.npz

Imports threestudio/models/mesh.py from the checkout (nothing is copied) with make_golden_renderer's import stubs, as
make_golden_mesh_ops.py does, and RUNS Mesh._compute_vertex_tangent (:162-205, through _compute_vertex_normal) in
float64 on the CPU for the marching-cubes meshes sphere17, torus24 and blobs33 (tests/mesh_reference.py fields through
tests/mc_reference.py).  The UVs are data made here: tests/uv_reference.py's atlas at N = 128, padding 2
(tangent_reference.atlas).  The reference's result must be finite everywhere on these meshes (asserted): the golden
holds no NaN the restatement would have to special-case.

Only DATA is written: input meshes, UVs and the reference's tangents.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(HERE, "reference_mesh_tangent.npz")

import mc_reference as MC  # noqa: E402
import mesh_reference as M  # noqa: E402
import tangent_reference as TR  # noqa: E402

N, PAD = 128, 2


def main(ref):
    import make_golden_renderer as R
    R.REF = os.path.abspath(ref)
    R._install_stubs()
    Mesh = importlib.import_module("threestudio.models.mesh").Mesh
    torch.set_num_threads(1)
    data = {"texture_size": np.int64(N), "padding": np.int64(PAD)}
    for name, field in (("sphere17", M.sphere_field(17)), ("torus24", M.torus_field(24)),
                        ("blobs33", M.blobs_field(33))):
        mc = MC.marching_cubes(field)
        v, t = mc.v_pos.astype(np.float32), mc.t_pos_idx.astype(np.int64)
        v_tex, t_tex = TR.atlas(v, t, N, PAD)
        mesh = Mesh(torch.tensor(v, dtype=torch.float64), torch.as_tensor(t))
        mesh._v_tex, mesh._t_tex_idx = torch.tensor(v_tex, dtype=torch.float64), torch.as_tensor(t_tex)
        tng = mesh._compute_vertex_tangent().numpy().copy()
        assert np.isfinite(tng).all(), f"{name}: the reference's tangents are not finite"
        data[f"{name}_v_pos"], data[f"{name}_t_pos_idx"] = v, t.astype(np.int32)
        data[f"{name}_v_tex"], data[f"{name}_t_tex_idx"] = v_tex, t_tex.astype(np.int32)
        data[f"{name}_v_tng"] = tng
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
