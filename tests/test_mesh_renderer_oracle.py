"""The CPU-only half of the mesh renderer's oracle (tests/mesh_renderer_reference.py): the scene the GPU tests run is
closed, inside the box, visibly deformed and meets the suite's ambiguity cap on the float64 restatement alone (the
float32 oracle field stands in for the HIP one), and the float32 restatement is the float64 one within the bar the GPU
tests hold the kernels to."""
import numpy as np
import pytest
import torch

import mc_reference as M
import mesh_reference as MR
import mesh_renderer_reference as X
from parity import TOL_VS_FP32, rel


@pytest.fixture(scope="module")
def runs():
    sc = X.scene()
    with torch.no_grad():
        sdf, deform = X.field(X.leaves(sc, torch.float32, "solid"), torch.float32)
    topo = X.topology_fields(sdf, deform)
    r64 = X.restate(sc, torch.float64, topo)
    r32 = X.restate(sc, torch.float32, topo)
    return sc, topo, r32, r64


def test_vertex_normals_torch_is_the_numpy_oracle(runs):
    _, _, _, r64 = runs
    v, tri = r64.meshes[0]
    assert np.abs(MR.vertex_normals_torch(v.detach(), tri).numpy() - MR.vertex_normals(v.detach().numpy(), tri)).max() < 1e-12


def test_scene_exercises_every_stage_and_meets_the_ambiguity_cap(runs):
    sc, topo, r32, r64 = runs
    cell = 2.0 / (X.RES - 1)
    for p, (sdf, deform) in enumerate(topo):
        mc = M.marching_cubes(sdf, deform, 0.0)
        assert len(mc.t_pos_idx) > 500
        assert M.unmatched_directed_edges(mc.t_pos_idx, len(mc.v_pos)) == []  # closed
        v = r64.meshes[p][0].detach()
        assert v.abs().max() < 1 - 4 * cell  # well inside the [-1, 1] box
        on_edge = np.unique(np.concatenate([mc.p0, mc.p1]))
        d = np.abs(deform.reshape(-1, 3)[on_edge])  # grid-cell units, at the grid points that carry the surface
        assert 0.02 < d.mean() < 0.25 and d.max() < 1.0, (d.mean(), d.max())
    frac = r64.ambiguous.float().mean().item()
    print(f"ambiguous pixel fraction {frac:.2e}")
    assert frac < 1e-3
    covered = r64.covered.float().mean(dim=(1, 2))
    assert (covered > 0.1).all() and (covered < 0.5).all(), covered  # every view shows its mesh and a background
    keep, margins = X.keep_mask(r64, r32)
    print(f"kept pixel fraction {keep.float().mean().item():.3f}, kink margins {margins}")
    assert keep.float().mean() > 0.5  # most pixels carry weight
    assert torch.equal(r32.ids[keep], r64.ids[keep])
    assert not torch.equal(r64.ids[:X.N_VIEW], r64.ids[X.N_VIEW:])  # the prompts differ


def test_opacity_alone_reaches_only_the_geometry(runs):
    """The restatement's silhouette gradient: a loss on the antialiased opacity reaches the geometry planes, the sdf
    net and the deformation net (antialias -> clip positions -> marching cubes -> field) and is exactly zero, or
    absent, on the texture planes, the feature net and the background."""
    sc, _, r32, r64 = runs
    keep, _ = X.keep_mask(r64, r32)
    _, g = X.gradients(r64, sc, keep, keys=("opacity",), point_terms=False, retain_graph=True)
    reached = [n for n in X.GEO_NAMES if not n.startswith("feat")]
    assert all(n in g and g[n].abs().sum() > 0 for n in reached), list(g)
    assert g["space_cache"][:, :3].abs().sum() > 0 and g["space_cache"][:, 3:].abs().max() == 0
    assert all(g[n].abs().max() == 0 for n in g if n not in reached)


def test_float32_restatement_against_float64(runs):
    """The bar the GPU tests hold the kernels to against the float32 restatement (parity.TOL_VS_FP32) only means
    something on a scene where the float32 restatement itself is that close to the exact math."""
    sc, _, r32, r64 = runs
    keep, _ = X.keep_mask(r64, r32)
    l64, g64 = X.gradients(r64, sc, keep)
    l32, g32 = X.gradients(r32, sc, keep)
    for k in X.IMAGE_KEYS:
        err = (r32.out[k].double() - r64.out[k])[keep].abs().max().item()
        print(f"{k}: float32 vs float64 max abs {err:.2e}")
        assert err < 1e-4, (k, err)  # images of order 1; 1e-4 is what test_gpu_raster.py asks of an antialiased image
    assert set(g64) == set(X.GEO_NAMES + X.BG_NAMES)
    for n in g64:
        e = rel(g32[n], g64[n])
        print(f"grad {n}: float32 vs float64 {e:.2e}, norm {g64[n].norm().item():.3e}")
        assert g64[n].norm() > 0 and e <= TOL_VS_FP32, (n, e)
