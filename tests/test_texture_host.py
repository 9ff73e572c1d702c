"""Texture sampling and the textured viewer, the parts that need no GPU: the additive C-ABI entries, raster.texture's
argument handling, the float64 restatement (tests/texture_reference.py) pinned to torch's grid_sample, and
viewer.load_obj as the inverse of export.save_obj."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from triplaneturbo_amd import _lib, raster
from triplaneturbo_amd.export import read_png, save_obj
from triplaneturbo_amd.isosurface import Mesh
from triplaneturbo_amd.viewer import load_obj

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def test_header_declares_the_texture_entries_and_keeps_its_version():
    text = open(os.path.join(ROOT, "include", "tt_abi.h")).read()
    lib = ctypes.CDLL(_lib.build())
    for name in ("tt_tex_fwd", "tt_tex_bwd"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)
    assert int(re.search(r"^#define TT_ABI_VERSION (\d+)", text, re.M).group(1)) == 17
    protos, defines = _lib._parse_abi()
    assert len(protos["tt_tex_bwd"][1]) == len(protos["tt_tex_fwd"][1]) + 2  # + grad_out, two outputs for one
    assert (defines["TT_TEX_FILTER_NEAREST"], defines["TT_TEX_FILTER_LINEAR"]) == (0, 1)
    assert (defines["TT_TEX_BOUNDARY_WRAP"], defines["TT_TEX_BOUNDARY_CLAMP"], defines["TT_TEX_BOUNDARY_ZERO"]) == (0, 1, 2)
    assert "tt_texture.hip" in _lib.SOURCES


def test_texture_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.texture(torch.rand(1, 4, 4, 3), torch.rand(1, 2, 2, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        raster.RasterizerContext().texture(torch.rand(1, 4, 4, 3), torch.rand(1, 2, 2, 2), boundary_mode="clamp")


@pytest.mark.parametrize("kw,named", [
    (dict(filter_mode="linear-mipmap-nearest"), "linear-mipmap-nearest"),
    (dict(filter_mode="linear-mipmap-linear"), "linear-mipmap-linear"),
    (dict(boundary_mode="cube"), "cube"),
    (dict(uv_da=torch.zeros(1, 2, 2, 4)), "uv_da"),
    (dict(mip_level_bias=torch.zeros(1, 2, 2)), "mip_level_bias"),
    (dict(mip=[torch.zeros(1, 2, 2, 3)]), "mip"),
    (dict(max_mip_level=2), "max_mip_level")])
def test_unsupported_options_raise_and_name_themselves(kw, named):
    with pytest.raises(NotImplementedError, match=re.escape(named)):
        raster.texture(torch.rand(1, 4, 4, 3), torch.rand(1, 2, 2, 2), **kw)


def test_unknown_modes_and_keywords_are_errors():
    tex, uv = torch.rand(1, 4, 4, 3), torch.rand(1, 2, 2, 2)
    with pytest.raises(ValueError, match="filter_mode"):
        raster.texture(tex, uv, filter_mode="cubic")
    with pytest.raises(ValueError, match="boundary_mode"):
        raster.texture(tex, uv, boundary_mode="mirror")
    with pytest.raises(TypeError, match="bogus"):
        raster.texture(tex, uv, bogus=1)


# ---------------- the restatement against grid_sample ----------------
def _case(shape, B, seed):
    g = torch.Generator().manual_seed(seed)
    tex = torch.randn(*shape, generator=g, dtype=F64)
    uv = torch.rand(B, 6, 5, 2, generator=g, dtype=F64) * 4.0 - 1.5
    return tex, uv


def _grid_sample(tex, uv, mode, padding_mode):
    """tex (N,TH,TW,C), uv (B,H,W,2) in texture coordinates -> (B,H,W,C): align_corners=False puts pixel centres at
    (i + 0.5) / size, the texel-centre convention of the contract; grid = 2 uv - 1"""
    B = uv.shape[0]
    img = tex.permute(0, 3, 1, 2).expand(B, -1, -1, -1)
    return F.grid_sample(img, uv * 2 - 1, mode=mode, padding_mode=padding_mode, align_corners=False).permute(0, 2, 3, 1)


CASES = [((1, 5, 7, 3), 2, 0), ((2, 4, 4, 1), 2, 1)]


@pytest.mark.parametrize("shape,B,seed", CASES)
@pytest.mark.parametrize("bnd,padding", [("clamp", "border"), ("zero", "zeros")])
def test_restatement_linear_equals_grid_sample(shape, B, seed, bnd, padding):
    tex, uv = _case(shape, B, seed)
    assert (TR.texture(tex, uv, "linear", bnd) - _grid_sample(tex, uv, "bilinear", padding)).abs().max() <= 1e-12


@pytest.mark.parametrize("shape,B,seed", CASES)
@pytest.mark.parametrize("bnd,padding", [("clamp", "border"), ("zero", "zeros")])
def test_restatement_nearest_equals_grid_sample(shape, B, seed, bnd, padding):
    """grid_sample rounds x = u TW - 0.5 to the nearest integer, which is floor(u TW) away from ties (random UVs)"""
    tex, uv = _case(shape, B, seed)
    assert (TR.texture(tex, uv, "nearest", bnd) - _grid_sample(tex, uv, "nearest", padding)).abs().max() <= 1e-12


@pytest.mark.parametrize("shape,B,seed", CASES)
def test_restatement_linear_wrap_equals_sampling_a_periodically_padded_copy(shape, B, seed):
    tex, uv = _case(shape, B, seed)
    N, TH, TW, C = tex.shape
    pad = 2
    padded = tex[:, torch.arange(-pad, TH + pad) % TH][:, :, torch.arange(-pad, TW + pad) % TW]
    # the same sample inside the copy: x reduced to one period, shifted by the padding, in the copy's coordinates
    size = torch.tensor([TW, TH], dtype=F64)
    x = torch.remainder(uv * size - 0.5, size)
    uv_padded = (x + pad + 0.5) / (size + 2 * pad)
    want = _grid_sample(padded, uv_padded, "bilinear", "zeros")  # no tap reaches the copy's border
    assert (TR.texture(tex, uv, "linear", "wrap") - want).abs().max() <= 1e-12


def test_restatement_gives_zero_and_no_gradient_at_non_finite_uv():
    tex, uv = _case((1, 5, 7, 3), 2, 0)
    uv[0, 0, 0, 0] = float("nan")
    uv[1, 2, 3, 1] = float("-inf")
    tex.requires_grad_(True)
    uv.requires_grad_(True)
    out = TR.texture(tex, uv, "linear", "wrap")
    out.sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(uv.grad).all() and torch.isfinite(tex.grad).all()
    assert torch.count_nonzero(out[0, 0, 0]) == 0 and torch.count_nonzero(out[1, 2, 3]) == 0
    assert torch.count_nonzero(uv.grad[0, 0, 0]) == 0 and torch.count_nonzero(uv.grad[1, 2, 3]) == 0
    assert abs(tex.grad.sum().item() - 3 * (2 * 6 * 5 - 2)) <= 1e-9


# ---------------- load_obj(save_obj(...)) ----------------
def test_load_obj_reads_back_what_save_obj_writes(tmp_path):
    g = torch.Generator().manual_seed(5)
    v_pos = torch.randn(4, 3, generator=g)
    mesh = Mesh(v_pos, torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32))
    mesh._v_tex = torch.rand(5, 2, generator=g)
    mesh._t_tex_idx = torch.tensor([[0, 1, 2], [4, 1, 3]], dtype=torch.int32)
    mesh.set_vertex_color(torch.rand(4, 3, generator=g))
    kd = torch.rand(4, 4, 3, generator=g)
    paths = save_obj(str(tmp_path / "model.obj"), mesh, save_mat=True, save_normal=True, save_uv=True,
                     save_vertex_color=True, map_Kd=kd, map_format="png")
    assert sorted(os.path.basename(p) for p in paths) == ["model.mtl", "model.obj", "texture_kd.png"]
    got, got_kd = load_obj(str(tmp_path / "model.obj"))
    assert got.t_pos_idx.dtype == torch.int32 and torch.equal(got.t_pos_idx, mesh.t_pos_idx)
    assert got.t_tex_idx.dtype == torch.int32 and torch.equal(got.t_tex_idx, mesh.t_tex_idx)
    # save_obj prints the shortest decimal that identifies each float32, which reads back to the same float32 ...
    assert got.v_pos.dtype == torch.float32 and torch.equal(got.v_pos, mesh.v_pos)
    assert torch.equal(got.v_rgb, mesh.v_rgb)
    assert torch.equal(got.v_tex[:, 0], mesh.v_tex[:, 0])
    # ... and writes v as 1 - v: one rounding of a number below 1 on the way out, one on the way back (2^-25 each)
    assert (got.v_tex[:, 1].double() - mesh.v_tex[:, 1].double()).abs().max() <= 2.0 ** -24
    img = read_png(str(tmp_path / "texture_kd.png"))
    assert got_kd.dtype == torch.float32 and got_kd.shape == (4, 4, 3)
    assert torch.equal(got_kd, torch.from_numpy(img).float() / 255.0)
    assert np.array_equal(img, (kd.numpy() * 255.0).astype(np.uint8))


def test_load_obj_without_material_or_uvs(tmp_path):
    mesh = Mesh(torch.rand(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
    save_obj(str(tmp_path / "plain.obj"), mesh)
    got, kd = load_obj(str(tmp_path / "plain.obj"))
    assert kd is None and got.v_rgb is None and got._v_tex is None
    assert torch.equal(got.v_pos, mesh.v_pos) and torch.equal(got.t_pos_idx, mesh.t_pos_idx)
