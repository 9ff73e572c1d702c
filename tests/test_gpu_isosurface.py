"""HIP marching cubes (tt_mc_*, ops.marching_cubes, triplaneturbo_amd.isosurface) against the numpy oracle of the
contract (tests/mc_reference.py): identical topology and vertex count, positions within 2e-6, bit-repeatable launches,
gradients against a float64 re-implementation, edge cases, and the full 160^3 text -> mesh path through the geometry
plugin (isosurface() + colorize_mesh(), mesh_exporter.py:78-183)."""
import os
import sys

import numpy as np
import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, colorize_mesh, isosurface

from parity import check_outputs

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_reference as M  # noqa: E402
from test_isosurface_oracle import sphere, torus, two_spheres  # noqa: E402

pytestmark = pytest.mark.gpu
POS_TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _random(R, seed):
    return np.random.default_rng(seed).standard_normal((R, R, R)).astype(np.float32)


FIELDS = {
    "sphere33": lambda: sphere(33),
    "sphere64": lambda: sphere(64),
    "torus33": lambda: torus(33),
    "two_spheres64": lambda: two_spheres(64),
    "random17": lambda: _random(17, 0),
    "r2": lambda: np.array([[[-1, 1], [1, 1]], [[1, 1], [1, -0.5]]], dtype=np.float32),
}


def _deform(R, seed):
    return np.random.default_rng(seed).uniform(-0.4, 0.4, (R, R, R, 3)).astype(np.float32)


def _hip(level, deform, iso, dev):
    lv = torch.from_numpy(level).to(dev)
    d = None if deform is None else torch.from_numpy(deform).to(dev)
    v, t = ops.marching_cubes(lv, d, iso)
    return v.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", sorted(FIELDS))
@pytest.mark.parametrize("with_def", [False, True])
@pytest.mark.parametrize("iso", [0.0, 0.05])
def test_hip_matches_the_oracle(dev, name, with_def, iso):
    level = FIELDS[name]()
    R = level.shape[0]
    deform = _deform(R, 1) if with_def else None
    want = M.marching_cubes(level, deform, iso)
    v, t = _hip(level, deform, iso, dev)
    assert t.dtype == np.int32 and v.dtype == np.float32
    assert len(v) == len(want.v_pos) > 0
    assert np.array_equal(t, want.t_pos_idx)
    assert np.abs(v - want.v_pos).max() <= POS_TOL
    if with_def:
        v0, t0 = _hip(level, None, iso, dev)
        vz, tz = _hip(level, np.zeros_like(deform), iso, dev)
        assert np.array_equal(v0, vz) and np.array_equal(t0, tz)  # zero deformation == none, bit for bit


def _run(level, deform, iso, W, dev):
    lv = torch.from_numpy(level).to(dev).requires_grad_(True)
    d = None if deform is None else torch.from_numpy(deform).to(dev).requires_grad_(True)
    v, t = ops.marching_cubes(lv, d, iso)
    (v * W.to(dev)).sum().backward()
    return v.detach().cpu(), t.cpu(), lv.grad.cpu(), None if d is None else d.grad.cpu()


def test_launches_are_bit_repeatable(dev):
    level, deform = _random(48, 2), _deform(48, 3)
    V = len(M.marching_cubes(level, deform, 0.1).v_pos)
    W = torch.randn(V, 3, generator=torch.Generator().manual_seed(0))
    a = _run(level, deform, 0.1, W, dev)
    b = _run(level, deform, 0.1, W, dev)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name,with_def,iso", [("sphere33", False, 0.0), ("sphere33", True, 0.05),
                                               ("torus33", True, 0.0), ("random17", True, 0.1)])
def test_backward_against_float64(dev, name, with_def, iso):
    level = FIELDS[name]()
    R = level.shape[0]
    deform = _deform(R, 4) if with_def else None
    mc = M.marching_cubes(level, deform, iso)
    W = torch.randn(len(mc.v_pos), 3, generator=torch.Generator().manual_seed(1))
    _, _, g_level, g_def = _run(level, deform, iso, W, dev)

    def ref(dtype):
        lv = torch.from_numpy(level).to(dtype).requires_grad_(True)
        d = None if deform is None else torch.from_numpy(deform).to(dtype).requires_grad_(True)
        v = M.vertex_positions_torch(mc, lv, d, iso)
        (v * W.to(dtype)).sum().backward()
        out = {"grad_level": lv.grad}
        if d is not None:
            out["grad_deformation"] = d.grad
        return out

    got = {"grad_level": g_level}
    if with_def:
        got["grad_deformation"] = g_def
    check_outputs(f"marching cubes backward {name} def={with_def} iso={iso}", got, ref(torch.float32),
                  ref(torch.float64), tuple(got))
    on_edge = np.zeros(R ** 3, dtype=bool)
    on_edge[mc.p0] = True
    on_edge[mc.p1] = True
    assert (g_level.reshape(-1)[torch.from_numpy(~on_edge)] == 0).all()
    if with_def:
        assert (g_def.reshape(-1, 3)[torch.from_numpy(~on_edge)] == 0).all()


def test_edge_cases(dev):
    v, t = ops.marching_cubes(torch.ones(20, 20, 20, device=dev), None, 0.0)
    assert v.shape == (0, 3) and t.shape == (0, 3)
    lv = torch.ones(20, 20, 20, device=dev, requires_grad=True)
    v, _ = ops.marching_cubes(lv, None, 0.0)
    v.sum().backward()  # an empty mesh still back-propagates (zeros)
    assert (lv.grad == 0).all()
    for R in (1, 513):
        with pytest.raises(RuntimeError, match="tt_mc_workspace_bytes failed: bad argument"):
            ops.marching_cubes(torch.zeros(R, R, R, device=dev), None, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.marching_cubes(torch.zeros(4, 4, 4), None, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.marching_cubes(torch.zeros(4, 4, 4, device=dev), torch.zeros(4, 4, 4, 3), 0.0)


def _geometry(dev):
    torch.manual_seed(0)
    return tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)


def test_isosurface_and_colours_160_through_the_plugin(dev):
    g = _geometry(dev)
    cache = (torch.randn(2, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    helper = DiffMarchingCubeHelper(160).to(dev)
    with torch.no_grad():
        meshes = isosurface(cache, g.forward_field, helper)
        meshes = colorize_mesh(cache, g.export, meshes, torch.sigmoid)
        pts = helper.grid_vertices.to(dev) * 2 - 1
        sdf, deform = g.forward_field(pts[None].expand(2, -1, -1), cache)
    assert len(meshes) == 2
    for b, mesh in enumerate(meshes):
        want = M.marching_cubes(sdf[b].reshape(160, 160, 160).cpu().numpy(),
                                deform[b].reshape(160, 160, 160, 3).cpu().numpy(), 0.0)
        assert len(want.t_pos_idx) > 10000
        assert np.array_equal(mesh.t_pos_idx.cpu().numpy(), want.t_pos_idx)
        v_want = torch.from_numpy(want.v_pos).to(dev) * 2 - 1  # the same mapping to [-1, 1] (scale_tensor)
        assert (mesh.v_pos - v_want).abs().max().item() <= 2 * POS_TOL
        rgb = mesh.v_rgb
        assert rgb.shape == (len(want.v_pos), 3) and torch.isfinite(rgb).all()
        sel = torch.arange(0, len(want.v_pos), max(1, len(want.v_pos) // 1024), device=dev)[:1024]
        with torch.no_grad():
            col = torch.sigmoid(g.export(v_want[sel][None], cache[b:b + 1])["features"][0])
        assert (rgb[sel] - col).abs().max().item() <= 1e-5
        assert mesh.v_nrm.shape == mesh.v_pos.shape and torch.isfinite(mesh.v_nrm).all()


def test_field_without_a_level_set_falls_back_to_the_unit_sphere(dev):
    helper = DiffMarchingCubeHelper(48).to(dev)
    cache = torch.zeros(1, 6, 32, 8, 8, device=dev)
    field = lambda pts, c: (torch.ones(pts.shape[0], pts.shape[1], 1, device=dev), None)  # noqa: E731
    (mesh,) = isosurface(cache, field, helper)
    r = mesh.v_pos.norm(dim=-1)
    assert len(mesh.v_pos) > 1000 and (r - 1).abs().max().item() < 2.0 / 47


def test_gradient_reaches_the_space_cache_and_the_deformation_net(dev):
    g = _geometry(dev)
    cache = (torch.randn(1, 6, 32, 64, 64, generator=torch.Generator().manual_seed(9)) * 0.5).to(dev)
    cache.requires_grad_(True)
    helper = DiffMarchingCubeHelper(64).to(dev)
    (mesh,) = isosurface(cache, g.forward_field, helper)
    assert mesh.v_pos.requires_grad and len(mesh.v_pos) > 1000
    W = torch.randn(mesh.v_pos.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    (mesh.v_pos * W).sum().backward()
    for name, grad in [("space_cache", cache.grad)] + [
            (f"deformation_network.{i}", w.grad) for i, w in enumerate(g.deformation_network.weights())]:
        assert grad is not None and torch.isfinite(grad).all() and grad.abs().sum() > 0, name
    assert all(w.grad is not None and w.grad.abs().sum() > 0 for w in g.sdf_network.weights())
