"""Marching cubes without a GPU: the C ABI validates its arguments before any HIP call, the op refuses CPU tensors, and
the torch-only parts of triplaneturbo_amd.isosurface (grid, normals, colouring loop) behave like the reference's."""
import ctypes
import os
import re

import pytest
import torch

from triplaneturbo_amd import _lib, ops
from triplaneturbo_amd import isosurface as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(8)  # never dereferenced: validation fails first
    hdr = open(os.path.join(ROOT, "include", "tt_abi.h")).read()
    assert int(re.search(r"#define\s+TT_MC_MAX_RES\s+(\d+)", hdr).group(1)) == 512
    for bad in (-1, 0, 1, 513, 1 << 20):
        assert lib.tt_mc_workspace_bytes(bad) == -1
        assert lib.tt_mc_count(one, bad, 0.0, one, one, null) == -1
        assert lib.tt_mc_emit(one, null, bad, 0.0, one, one, one, null) == -1
        assert lib.tt_mc_bwd(one, null, bad, 0.0, one, one, one, null, null) == -1
    for R in (2, 17, 160, 512):
        assert lib.tt_mc_workspace_bytes(R) >= 6 * R ** 3  # masks, cases, int32 offsets per point
    assert lib.tt_mc_count(null, 8, 0.0, one, one, null) == -1
    assert lib.tt_mc_count(one, 8, 0.0, null, one, null) == -1
    assert lib.tt_mc_count(one, 8, 0.0, one, null, null) == -1
    assert lib.tt_mc_emit(one, null, 8, 0.0, one, null, one, null) == -1
    assert lib.tt_mc_emit(one, null, 8, 0.0, one, one, null, null) == -1
    # deformation and its gradient go together
    assert lib.tt_mc_bwd(one, one, 8, 0.0, one, one, one, null, null) == -1
    assert lib.tt_mc_bwd(one, null, 8, 0.0, one, one, one, one, null) == -1
    assert lib.tt_mc_bwd(one, null, 8, 0.0, one, null, one, null, null) == -1


def test_marching_cubes_refuses_cpu_tensors_and_bad_shapes():
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.marching_cubes(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match=r"\(R,R,R\)"):
        ops.marching_cubes(torch.zeros(4, 4, 5))


def test_grid_vertices_are_the_reference_grid():
    for rng in ((0, 1), (-1, 1)):
        h = I.DiffMarchingCubeHelper(7, rng)
        x = torch.linspace(*rng, 7)
        g = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), -1).reshape(-1, 3)
        assert torch.equal(h.grid_vertices, g * (rng[1] - rng[0]) + rng[0])
        assert h.grid_vertices is h.grid_vertices and h.grid_vertices.device.type == "cpu"
    # level.view(R,R,R)[i,j,k] is grid point i*R*R + j*R + k: x = i, y = j, z = k
    h = I.DiffMarchingCubeHelper(5)
    assert torch.equal(h.grid_vertices.view(5, 5, 5, 3)[1, 2, 3], torch.tensor([0.25, 0.5, 0.75]))


def test_vertex_normals_of_an_outward_tetrahedron():
    v = torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    t = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)
    m = I.Mesh(v, t)
    n = m.v_nrm
    assert torch.allclose(n.norm(dim=-1), torch.ones(4))
    assert ((n * (v - v.mean(0))).sum(-1) > 0).all()
    assert m.v_rgb is None


def test_colorize_mesh_slices_the_cache_per_mesh():
    seen = []

    def export(points, cache):
        seen.append((points.shape, cache.shape, cache[0, 0, 0, 0, 0].item()))
        return {"features": points * 2}

    cache = torch.arange(3.0).view(3, 1, 1, 1, 1).expand(3, 6, 2, 2, 2)
    meshes = [I.Mesh(torch.rand(n, 3), torch.zeros(0, 3, dtype=torch.int32)) for n in (4, 5, 6)]
    out = I.colorize_mesh(cache, export, meshes, torch.sigmoid)
    assert out is meshes
    assert [s[2] for s in seen] == [0.0, 1.0, 2.0] and [s[0] for s in seen] == [(1, 4, 3), (1, 5, 3), (1, 6, 3)]
    for m in meshes:
        assert torch.equal(m.v_rgb, torch.sigmoid(m.v_pos * 2))
