"""HIP marching tetrahedra (tt_mt_*, ops.TetGrid / ops.marching_tets, isosurface.MarchingTetrahedraHelper) against
the reference helper's recorded results (tests/golden/reference_tets.npz) and the numpy oracle of the contract
(tests/mt_reference.py): identical faces, positions within 2e-6, the compaction's block and chunk seams, gradients
against the reference's float64 autograd, bit-repeatable launches, edge cases, and the mesh renderer's "mt" path."""
import json
import os
import sys

import numpy as np
import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops
from triplaneturbo_amd.isosurface import MarchingTetrahedraHelper, kuhn_tet_grid

from parity import check_outputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mt_reference as M  # noqa: E402
from test_gpu_mesh_renderer import _cameras  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POS_TOL = 2e-6  # the marching-cubes bar (tests/test_gpu_isosurface.py)
CASES = ("sphere9", "jitter5", "zeros7")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "reference_tets.npz")))


def _case(golden, case):
    return {k[len(case) + 1:]: v for k, v in golden.items() if k.startswith(case + "_")}


def _helper(g, dev):
    grid = ops.TetGrid(torch.from_numpy(g["vertices"]).to(dev), torch.from_numpy(g["indices"]).to(dev))
    return MarchingTetrahedraHelper(int(g["resolution"]), tet_grid=grid).to(dev)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_def", [False, True])
def test_forward_matches_the_reference_helper(dev, golden, case, with_def):
    g = _case(golden, case)
    helper = _helper(g, dev)
    level = torch.from_numpy(g["level"]).to(dev)
    deformation = torch.from_numpy(g["deformation"]).to(dev) if with_def else None
    mesh = helper(level, deformation)
    sfx = "_def" if with_def else ""
    assert mesh.t_pos_idx.dtype == torch.int32 and mesh.v_pos.dtype == torch.float32
    assert np.array_equal(mesh.t_pos_idx.cpu().numpy(), g["t_pos_idx" + sfx])
    err = np.abs(mesh.v_pos.cpu().numpy() - g["v_pos" + sfx]).max()
    print(f"{case} def={with_def}: max |v_pos - reference| = {err:.3g}, bit-equal "
          f"{mesh.v_pos.cpu().numpy().tobytes() == g['v_pos' + sfx].tobytes()}")
    assert err <= POS_TOL
    assert np.array_equal(helper.all_edges.cpu().numpy(), g["all_edges"]) and helper.all_edges.dtype == torch.int64
    # the reference's extras
    assert mesh.extras["tet_edges"] is helper.all_edges and mesh.extras["grid_level"] is level
    assert mesh.extras["grid_deformation"] is deformation
    want = helper.grid_vertices if not with_def else helper.grid_vertices + helper.normalize_grid_deformation(deformation)
    assert torch.equal(mesh.extras["grid_vertices"], want)


def _hip(vertices, indices, level, dev, grid=None):
    grid = grid or ops.TetGrid(torch.from_numpy(vertices).to(dev), torch.from_numpy(indices).to(dev))
    v, t = ops.marching_tets(grid.vertices, torch.from_numpy(level).to(dev), grid)
    return v.cpu().numpy(), t.cpu().numpy(), grid


def _check_against_oracle(vertices, indices, level, dev):
    want = M.marching_tets(vertices, level, indices)
    v, t, grid = _hip(vertices, indices, level, dev)
    tb = want.tables
    assert np.array_equal(grid.edges.cpu().numpy(), tb.edges) and np.array_equal(grid.tet_edge.cpu().numpy(), tb.tet_edge)
    assert np.array_equal(grid.vert_ptr.cpu().numpy(), tb.vert_ptr)
    assert np.array_equal(grid.vert_col.cpu().numpy(), tb.vert_col)
    assert np.array_equal(t, want.t_pos_idx)
    assert v.shape == want.v_pos.shape and np.abs(v - want.v_pos).max() <= POS_TOL
    return want, tb


def test_compaction_block_seam(dev):
    """Two blocks per compaction, the second one partial: between 256 and 512 items for every counter, i.e. edges (491)
    and tets (300).  No cubic Kuhn lattice has both counts in that range (4^3: 279 edges, 162 tets; 5^3: 604, 384), so
    the grid is the first 300 tets of the 5^3 lattice.  Then a whole 7^3 lattice: several blocks, different numbers of
    them for edges and tets, both last blocks partial."""
    v, t = (x.numpy() for x in kuhn_tet_grid(5))
    t = t[:300]
    rng = np.random.default_rng(3)
    want, tb = _check_against_oracle(v, t, rng.standard_normal(len(v)).astype(np.float32), dev)
    assert 256 < len(tb.edges) < 512 and 256 < len(t) < 512 and len(want.v_pos) > 100
    v, t = (x.numpy() for x in kuhn_tet_grid(7))
    want, tb = _check_against_oracle(v, t, rng.standard_normal(len(v)).astype(np.float32), dev)
    assert len(tb.edges) // 256 != len(t) // 256 and len(tb.edges) % 256 and len(t) % 256 and len(want.v_pos) > 256


def test_compaction_chunk_seam(dev):
    """R = 37: 279 936 tets are more than one 1024 x 256 chunk of the second scan level"""
    v, t = (x.numpy() for x in kuhn_tet_grid(37))
    assert len(t) == 279936 > 1024 * 256
    rng = np.random.default_rng(4)
    level = (np.sin(11.0 * v[:, 0]) * np.cos(9.0 * v[:, 1]) + v[:, 2] - 0.5
             + 0.2 * rng.standard_normal(len(v))).astype(np.float32)
    want, _ = _check_against_oracle(v, t, level, dev)
    assert len(want.t_pos_idx) > 100000


def _grads(helper, level, deformation, W):
    level = level.clone().requires_grad_(True)
    deformation = None if deformation is None else deformation.clone().requires_grad_(True)
    mesh = helper(level, deformation)
    (mesh.v_pos * W).sum().backward()
    return mesh, level.grad, None if deformation is None else deformation.grad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("with_def", [False, True])
def test_backward_against_the_reference_float64(dev, golden, case, with_def):
    g = _case(golden, case)
    helper = _helper(g, dev)
    level = torch.from_numpy(g["level"]).to(dev)
    deformation = torch.from_numpy(g["deformation"]).to(dev) if with_def else None
    W = torch.from_numpy(g["W"]).float().to(dev)
    _, g_level, g_def = _grads(helper, level, deformation, W)
    sfx = "_level_def" if with_def else "_level"
    got = {"grad_level": g_level.cpu()}
    o32, o64 = ({"grad_level": torch.from_numpy(g[tag + sfx])} for tag in ("g32", "g64"))
    if with_def:
        got["grad_deformation"] = g_def.cpu()
        o32["grad_deformation"] = torch.from_numpy(g["g32_deformation"])
        o64["grad_deformation"] = torch.from_numpy(g["g64_deformation"])
    mt = M.marching_tets(g["vertices"], g["level"], g["indices"])
    assert np.abs(g["level"][mt.a, 0] - g["level"][mt.b, 0]).min() >= 1e-3  # the conditioning the bar assumes
    check_outputs(f"marching tets backward {case} def={with_def}", got, o32, o64, tuple(got))
    on_edge = np.zeros(len(g["vertices"]), dtype=bool)
    on_edge[mt.a] = True
    on_edge[mt.b] = True
    off = torch.from_numpy(~on_edge)
    assert off.any() and (g_level.cpu().reshape(-1)[off] == 0).all()
    if with_def:
        assert (g_def.cpu()[off] == 0).all()
    # the op itself: grad_pos is dense with exact zeros off the crossing edges
    pos = helper.grid_vertices.clone().requires_grad_(True)
    v, _ = ops.marching_tets(pos, level, helper.tet_grid)
    (v * W).sum().backward()
    # (an end at level 0 has weight w = 0 / D: a zero row on a crossing edge is legitimate)
    assert (pos.grad.cpu()[off] == 0).all() and (pos.grad.cpu()[~off] != 0).any()


def test_launches_are_bit_repeatable(dev):
    v, t = kuhn_tet_grid(20)
    grid = ops.TetGrid(v.to(dev), t.to(dev))
    gen = torch.Generator().manual_seed(5)
    level = torch.randn(len(v), generator=gen).to(dev)
    pos = (v + 0.01 * torch.randn(v.shape, generator=gen)).to(dev)

    def run():
        p, lv = pos.clone().requires_grad_(True), level.clone().requires_grad_(True)
        vp, tp = ops.marching_tets(p, lv, grid)
        W = torch.randn(vp.shape, generator=torch.Generator().manual_seed(6)).to(dev)
        (vp * W).sum().backward()
        return vp.detach(), tp, lv.grad, p.grad

    a, b = run(), run()
    assert a[0].shape[0] > 10000
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_edge_cases(dev):
    v, t = kuhn_tet_grid(6)
    grid = ops.TetGrid(v.to(dev), t.to(dev))
    for sign in (1.0, -1.0):  # no level set: empty outputs, a zero backward
        lv = (sign * torch.ones(len(v), 1, device=dev)).requires_grad_(True)
        pos = v.to(dev).requires_grad_(True)
        vp, tp = ops.marching_tets(pos, lv, grid)
        assert vp.shape == (0, 3) and tp.shape == (0, 3) and tp.dtype == torch.int32
        vp.sum().backward()
        assert lv.grad.shape == lv.shape and (lv.grad == 0).all() and (pos.grad == 0).all()
    # NaN levels are unoccupied: the oracle's faces, NaN positions where an edge ends in one
    level = np.random.default_rng(7).standard_normal(len(v)).astype(np.float32)
    level[::11] = np.nan
    want = M.marching_tets(v.numpy(), level, t.numpy())
    got_v, got_t, _ = _hip(v.numpy(), t.numpy(), level, dev, grid)
    assert np.array_equal(got_t, want.t_pos_idx) and np.isnan(want.v_pos).any()
    assert np.array_equal(np.isnan(got_v), np.isnan(want.v_pos))
    assert np.abs(np.nan_to_num(got_v) - np.nan_to_num(want.v_pos)).max() <= POS_TOL
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.marching_tets(v, torch.zeros(len(v), device=dev), grid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.marching_tets(v.to(dev), torch.zeros(len(v)), grid)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.TetGrid(v.to(dev), t)
    for bad in (len(v), -1):
        t_bad = t.clone()
        t_bad[17, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            ops.TetGrid(v.to(dev), t_bad.to(dev))
    with pytest.raises(ValueError, match="one value per grid vertex"):
        ops.marching_tets(v.to(dev), torch.zeros(len(v) - 1, device=dev), grid)


# ---------------------------------------------------------------------------------------------------------------
def _renderer(dev, zero_weights=False, geo_over=None, **rend_over):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=True, **(geo_over or {}))).to(dev)
    if zero_weights:
        with torch.no_grad():
            for net in (g.sdf_network, g.feature_network, g.deformation_network):
                for w in net.parameters():
                    w.zero_()
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    R = 16
    grid = ops.TetGrid(*(x.to(dev) for x in kuhn_tet_grid(R)))
    cfg = dict(s["renderer"], isosurface_method="mt", isosurface_resolution=R, enable_bg_rays=False,
               sdf_grad_shrink=1.0, def_grad_shrink=1.0, **rend_over)
    r = tt.find(s["renderer_type"])(cfg, geometry=g, material=m, background=b, tet_grid=grid).to(dev)
    return r, g, grid


def _render(r, cache, dev, H=32, W=32, n_view=2):
    cam = _cameras(n_view, H, W, dev)
    return r(cam["mvp_mtx"], cam["camera_positions"], cam["light_positions"], H, W, space_cache=cache,
             text_embed=torch.zeros(1, 1024, device=dev), camera_distances=cam["camera_distances"], c2w=cam["c2w"])


def test_mesh_renderer_mt_path(dev):
    r, g, grid = _renderer(dev)
    r.train()
    helper = r.isosurface_helper
    assert isinstance(helper, MarchingTetrahedraHelper) and helper.tet_grid is grid
    cache = (torch.randn(1, 6, 32, 32, 32, generator=torch.Generator().manual_seed(9)) * 0.5).to(dev)
    cache.requires_grad_(True)
    out = _render(r, cache, dev)
    assert out["comp_rgb"].shape == (2, 32, 32, 3) and len(out["mesh"]) == 1
    mesh = out["mesh"][0]
    # the mesh is the helper applied to the field on the helper's grid, mapped to [-1, 1]
    points = helper.grid_vertices * 2 - 1
    sdf, deformation = g.forward_field(points[None], cache)  # under autograd, as the renderer calls it
    assert (sdf > 0).any() and (sdf < 0).any()
    want = helper(sdf[0].detach(), deformation[0].detach())
    assert mesh.t_pos_idx.shape[0] > 100 and torch.equal(mesh.t_pos_idx, want.t_pos_idx)
    assert torch.equal(mesh.v_pos, want.v_pos * 2 - 1)
    assert not hasattr(r, "isosurface_helper_1") and set(mesh.extras) >= {"grid_vertices", "tet_edges", "grid_level"}
    loss = out["comp_rgb"].square().mean() + mesh.laplacian()
    loss.backward()
    params = {"space_cache": cache, "sdf_network": next(g.sdf_network.parameters()),
              "deformation_network": next(g.deformation_network.parameters())}
    for name, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name


def test_mesh_renderer_mt_empty_field_takes_the_fix_up_path(dev):
    r, g, _ = _renderer(dev, zero_weights=True, geo_over={"sdf_bias_params": -0.1}, allow_empty_flag=True)
    r.train()
    cache = torch.randn(1, 6, 32, 32, 32, device=dev).requires_grad_(True)
    out = _render(r, cache, dev)
    mesh = out["mesh"][0]
    assert mesh.t_pos_idx.shape[0] > 0 and mesh.v_pos.shape[0] > 0  # the InstantMesh fix-up made a surface
    assert not r.empty_flag  # consumed by the forward
    for k in ("opacity", "disparity", "comp_rgb", "comp_normal_cam_vis"):
        assert torch.isfinite(out[k]).all() and not out[k].requires_grad, k  # detached (allow_empty_flag)
