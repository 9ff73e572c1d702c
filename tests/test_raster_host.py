"""Rasterizer and mesh renderer without a GPU: the C ABI validates its arguments before any HIP call, the ops refuse
CPU tensors, and the reference's mesh-renderer config block instantiates `generative-space-mesh-rasterize-renderer`."""
import ctypes
import json
import os
import re

import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import _lib, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first
    hdr = open(os.path.join(ROOT, "include", "tt_abi.h")).read()
    assert re.search(r"#define\s+TT_RAST_MAX_TRIS\s+\(1 << 24\)", hdr)
    big = 1 << 24
    for B, T, H, W in ((0, 4, 8, 8), (1, -1, 8, 8), (1, 4, 0, 8), (1, 4, 8, 0), (1, 4, -3, 8), (1, big, 8, 8)):
        assert lib.tt_rast_workspace_bytes(B, T, H, W) == -1
        assert lib.tt_rast_fwd(one, one, B, 3, T, H, W, one, one, null) == -1
        assert lib.tt_rast_bwd(one, one, one, one, B, 3, T, H, W, one, null) == -1
        assert lib.tt_interp_fwd(one, 1, one, one, B, 3, T, H, W, 2, one, null) == -1
        assert lib.tt_interp_bwd(one, 1, one, one, one, B, 3, T, H, W, 2, one, one, null) == -1
        assert lib.tt_aa_fwd(one, one, one, one, one, one, B, 3, T, H, W, 2, one, null) == -1
        assert lib.tt_aa_bwd(one, one, one, one, one, one, one, B, 3, T, H, W, 2, one, one, null) == -1
    assert lib.tt_rast_workspace_bytes(4, big - 1, 512, 512) >= 8 * 4 * 512 * 512  # the depth keys
    assert lib.tt_rast_workspace_bytes(1, 0, 1, 1) > 0
    # null pointers where the count they are indexed by is positive
    assert lib.tt_rast_fwd(null, one, 1, 3, 1, 8, 8, one, one, null) == -1
    assert lib.tt_rast_fwd(one, null, 1, 3, 1, 8, 8, one, one, null) == -1
    assert lib.tt_rast_fwd(one, one, 1, 3, 1, 8, 8, null, one, null) == -1
    assert lib.tt_rast_fwd(one, one, 1, 3, 1, 8, 8, one, null, null) == -1
    assert lib.tt_rast_bwd(one, one, null, one, 1, 3, 1, 8, 8, one, null) == -1
    assert lib.tt_rast_bwd(one, one, one, one, 1, 3, 1, 8, 8, null, null) == -1
    # C < 1, attribute batch neither 1 nor B, both interpolate gradients null
    assert lib.tt_interp_fwd(one, 1, one, one, 2, 3, 1, 8, 8, 0, one, null) == -1
    assert lib.tt_interp_fwd(one, 3, one, one, 2, 3, 1, 8, 8, 2, one, null) == -1
    assert lib.tt_interp_fwd(one, 1, null, one, 2, 3, 1, 8, 8, 2, one, null) == -1
    assert lib.tt_interp_bwd(one, 1, one, one, one, 2, 3, 1, 8, 8, 2, null, null, null) == -1
    assert lib.tt_aa_fwd(one, one, one, one, null, one, 1, 3, 1, 8, 8, 2, one, null) == -1
    assert lib.tt_aa_fwd(one, one, one, one, one, null, 1, 3, 1, 8, 8, 2, one, null) == -1
    assert lib.tt_aa_fwd(one, one, one, one, one, one, 1, 3, 1, 8, 8, 0, one, null) == -1
    assert lib.tt_aa_bwd(one, one, one, one, one, one, null, 1, 3, 1, 8, 8, 2, one, one, null) == -1
    assert lib.tt_aa_bwd(one, one, one, one, one, one, one, 1, 3, 1, 8, 8, 2, null, one, null) == -1


def test_ops_refuse_cpu_tensors():
    pos = torch.zeros(1, 3, 4)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    rast = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.rasterize(pos, tri, (4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.interpolate(torch.zeros(1, 3, 2), rast, tri)
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.antialias(torch.zeros(1, 4, 4, 3), rast, pos, tri)
    ctx = raster.RasterizerContext("cuda", None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ctx.rasterize(pos, tri, (4, 4))
    with pytest.raises(NotImplementedError):
        raster.interpolate(torch.zeros(1, 3, 2), rast, tri, rast_db=rast)


def test_edge_topology_groups_shared_edges():
    # two triangles sharing edge (0, 2), one dangling triangle
    tri = torch.tensor([[0, 1, 2], [0, 2, 3], [4, 5, 6]], dtype=torch.int32)
    ofs, etri = raster.edge_topology(tri, 7)
    assert ofs.shape == (9, 2) and etri.shape == (9,)
    for t in range(3):
        for k in range(3):
            a, b = int(tri[t, k]), int(tri[t, (k + 1) % 3])
            first, cnt = (int(x) for x in ofs[3 * t + k])
            members = sorted(int(x) for x in etri[first:first + cnt])
            want = sorted(u for u in range(3) if {a, b} <= set(tri[u].tolist()))
            assert members == want, (t, k, members, want)


def test_vertex_transform_matches_the_reference_formula():
    ctx = raster.RasterizerContext("gl", None)  # context_type is accepted and ignored
    g = torch.Generator().manual_seed(0)
    v = torch.randn(5, 3, generator=g)
    mvp = torch.randn(2, 4, 4, generator=g)
    out = ctx.vertex_transform(v, mvp)
    ref = torch.einsum("bij,nj->bni", mvp, torch.cat([v, torch.ones(5, 1)], -1))
    assert torch.allclose(out, ref, atol=1e-5)


def test_reference_mesh_renderer_config_loads():
    """configs/TriplaneTurbo_v1.yaml's `renderer` block (tests/golden/reference_mesh_renderer_config.json, written by
    make_golden_mesh_renderer_config.py) instantiates the mesh renderer with every key it sets."""
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    g = tt.find(t["geometry_type"])(t["geometry"])
    m = tt.find(t["material_type"])(t["material"])
    b = tt.find(t["background_type"])(t["background"])
    r = tt.find(s["renderer_type"])(s["renderer"], geometry=g, material=m, background=b)
    assert type(r).__name__ == "GenerativeSpaceMeshRasterizeRenderer"
    assert r.cfg.isosurface_method == "diffmc" and r.cfg.enable_bg_rays and not r.cfg.allow_empty_flag
    assert r.cfg.isosurface_resolution == 128 and r.cfg.normal_direction == "camera"
    assert g.isosurface == r.isosurface
    r.update_step(0, 10)
    assert r.sdf_grad_shrink == 0.001 and r.def_grad_shrink == 0.001
    assert r.center_indices.shape == (1, 1) and r.border_indices.shape[0] == 128 ** 3 - 124 ** 3
    with pytest.raises(NotImplementedError):
        tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_method="mt"), geometry=g, material=m, background=b)
    with pytest.raises(NotImplementedError):
        tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_remove_outliers=True), geometry=g, material=m,
                                    background=b)
    with pytest.raises(KeyError):
        tt.find(s["renderer_type"])(dict(s["renderer"], not_a_key=1), geometry=g, material=m, background=b)
