"""Golden vectors of the reference's Mesh regularisers (run once, on the CPU, against a reference checkout).

    python tests/golden/make_golden_mesh_ops.py REFERENCE_CHECKOUT   ->  tests/golden/reference_mesh_ops.npz

Imports threestudio/models/mesh.py from the checkout (nothing is copied) with make_golden_renderer's import stubs for
absent packages (they carry no arithmetic) and RUNS, in float64 on the CPU, for each input mesh:

  Mesh.edges (_compute_edges :255-267), Mesh.normal_consistency() (:269-274, through _compute_vertex_normal :134-160),
  Mesh.laplacian() (:276-308, the sparse COO matrix), and backward() of each loss to v_pos.

The inputs are data made here: tests/mc_reference.py meshes of analytic fields (R <= 33) and mesh_reference's
hand-built mesh (degenerate face, unreferenced vertex, non-manifold edge, several components).  remove_outlier is not
pinned: the reference runs it with trimesh, which is not available; tests/mesh_reference.py is its oracle.

Only DATA is written: input meshes and the reference's outputs.
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
OUT = os.path.join(HERE, "reference_mesh_ops.npz")

import mc_reference as MC  # noqa: E402
import mesh_reference as M  # noqa: E402


def input_meshes():
    """name -> (v_pos float32 (V,3), t_pos_idx int64 (T,3))"""
    out = {}
    for name, field in (("sphere17", M.sphere_field(17)), ("torus24", M.torus_field(24)),
                        ("blobs33", M.blobs_field(33))):
        mc = MC.marching_cubes(field)
        out[name] = (mc.v_pos.astype(np.float32), mc.t_pos_idx.astype(np.int64))
    out["hand"] = M.hand_mesh()
    return out


def main(ref):
    import make_golden_renderer as R
    R.REF = os.path.abspath(ref)
    R._install_stubs()
    Mesh = importlib.import_module("threestudio.models.mesh").Mesh
    torch.set_num_threads(1)
    data = {}
    for name, (v, t) in input_meshes().items():
        data[f"{name}_v_pos"] = v
        data[f"{name}_t_pos_idx"] = t
        for loss_name in ("normal_consistency", "laplacian"):
            vp = torch.tensor(v, dtype=torch.float64, requires_grad=True)
            mesh = Mesh(vp, torch.as_tensor(t))
            loss = getattr(mesh, loss_name)()
            loss.backward()
            data[f"{name}_{loss_name}"] = np.float64(loss.item())
            data[f"{name}_{loss_name}_grad"] = vp.grad.numpy().copy()
            data[f"{name}_edges"] = mesh.edges.numpy().copy()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): " + ", ".join(sorted({k.split('_')[0] for k in data})))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
