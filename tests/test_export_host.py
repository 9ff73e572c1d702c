"""Textured mesh export without a GPU: the `multiprompt-mesh-exporter` registry entry and its Config, the UV-atlas /
texture-fill C ABI's argument checks, the host shelf packing (tt_uv_pack) against tests/uv_reference.py,
NoMaterial.export, and save_obj's OBJ / MTL / PNG output in the reference's line formats."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import _lib
from triplaneturbo_amd.export import ExporterOutput, png_bytes, read_png, save_obj

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_reference as U  # noqa: E402

# multiprompt_mesh_exporter.py:19-30 + threestudio/models/exporters/base.py:20-21
REFERENCE_CONFIG = {"save_video": False, "fmt": "obj-mtl", "save_name": "model", "save_normal": False,
                    "save_uv": False, "save_texture": True, "texture_size": 1024, "texture_format": "jpg",
                    "xatlas_chart_options": {}, "xatlas_pack_options": {}, "context_type": "cuda"}


def test_registry_name_and_config_match_the_reference():
    import dataclasses
    cls = tt.find("multiprompt-mesh-exporter")
    cfg = cls.Config()
    assert {f.name for f in dataclasses.fields(cfg)} == set(REFERENCE_CONFIG)
    assert dataclasses.asdict(cfg) == REFERENCE_CONFIG
    assert [f.name for f in dataclasses.fields(ExporterOutput)] == ["save_name", "save_type", "params"]
    with pytest.raises(KeyError):
        cls({"no_such_key": 1}, geometry=None, material=None, background=None)


def test_uv_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first
    for V, T, N in ((-1, 4, 64), (8, -1, 64), (8, 4, 0), (8, 4, 16385), (8, 1 << 24, 64)):
        assert lib.tt_uv_workspace_bytes(V, T, N) == -1
        assert lib.tt_uv_labels(one, one, one, V, T, 0, 8, 0.3, N, one, one, null) == -1
        assert lib.tt_uv_charts(one, one, one, one, null, V, T, 0, N, one, one, one, one, null) == -1
        assert lib.tt_uv_emit_count(one, one, V, T, N, one, one, null) == -1
        assert lib.tt_uv_emit(one, one, one, one, one, one, 1, 1.0, V, T, N, 2, one, one, one, null) == -1
        assert lib.tt_uv_overlap(one, one, 3, V, T, N, one, one, one, null) == -1
    assert lib.tt_uv_workspace_bytes(8, 4, 64) >= 4 * 64 * 64
    assert lib.tt_uv_workspace_bytes(0, 0, 1) > 0
    # labels: too many pairs, bad rounds / tau, null pointers
    assert lib.tt_uv_labels(one, one, one, 8, 4, 7, 8, 0.3, 64, one, one, null) == -1
    assert lib.tt_uv_labels(one, one, null, 8, 4, 2, 8, 0.3, 64, one, one, null) == -1
    assert lib.tt_uv_labels(one, one, one, 8, 4, 2, -1, 0.3, 64, one, one, null) == -1
    for tau in (0.0, -0.1, 0.6, float("nan")):
        assert lib.tt_uv_labels(one, one, one, 8, 4, 2, 8, tau, 64, one, one, null) == -1
    assert lib.tt_uv_labels(null, one, one, 8, 4, 2, 8, 0.3, 64, one, one, null) == -1
    assert lib.tt_uv_labels(one, one, one, 8, 4, 2, 8, 0.3, 64, null, one, null) == -1
    assert lib.tt_uv_charts(one, one, one, null, null, 8, 4, 2, 64, one, one, one, one, null) == -1
    assert lib.tt_uv_charts(one, one, one, one, null, 8, 4, 2, 64, one, one, one, null, null) == -1
    assert lib.tt_uv_emit(one, one, one, one, one, one, 5, 1.0, 8, 4, 64, 2, one, one, one, null) == -1  # C > T
    assert lib.tt_uv_emit(one, one, one, one, one, one, 1, -1.0, 8, 4, 64, 2, one, one, one, null) == -1
    assert lib.tt_uv_emit(one, one, one, one, one, one, 1, 1.0, 8, 4, 64, -1, one, one, one, null) == -1
    assert lib.tt_uv_emit(one, one, one, one, one, null, 1, 1.0, 8, 4, 64, 2, one, one, one, null) == -1
    assert lib.tt_uv_overlap(one, one, 13, 8, 4, 64, one, one, one, null) == -1  # Vt > 3T
    assert lib.tt_uv_overlap(one, one, 3, 8, 4, 64, one, null, one, null) == -1
    # fill
    for H, W, C in ((0, 4, 3), (4, 0, 3), (4, 4, 0), (4, 4, 65), (16385, 4, 3)):
        assert lib.tt_tex_fill(one, one, H, W, C, one, one, null) == -1
    assert lib.tt_tex_fill_workspace_bytes(0, 4) == -1
    assert lib.tt_tex_fill_workspace_bytes(4, 4) >= 2 * 4 * 16
    assert lib.tt_tex_fill(null, one, 4, 4, 3, one, one, null) == -1
    assert lib.tt_tex_fill(one, null, 4, 4, 3, one, one, null) == -1
    assert lib.tt_tex_fill(one, one, 4, 4, 3, null, one, null) == -1
    # pack (host memory)
    box = np.zeros((2, 4), np.float32)
    off = np.zeros((2, 2), np.int32)
    sc = np.zeros(1, np.float32)
    P = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.tt_uv_pack(P(box), 0, 64, 2, P(off), P(sc)) == -1
    assert lib.tt_uv_pack(P(box), 2, 0, 2, P(off), P(sc)) == -1
    assert lib.tt_uv_pack(P(box), 2, 64, -1, P(off), P(sc)) == -1
    assert lib.tt_uv_pack(null, 2, 64, 2, P(off), P(sc)) == -1
    bad = np.array([[1, 0, 0, 1]], np.float32)  # umax < umin
    assert lib.tt_uv_pack(P(bad), 1, 64, 2, P(off), P(sc)) == -1


def _pack(box, N, pad):
    lib = _lib.load()
    box = np.ascontiguousarray(box, np.float32)
    off = np.zeros((len(box), 2), np.int32)
    sc = np.zeros(1, np.float32)
    st = lib.tt_uv_pack(ctypes.c_void_p(box.ctypes.data), len(box), N, pad, ctypes.c_void_p(off.ctypes.data),
                        ctypes.c_void_p(sc.ctypes.data))
    return st, off, float(sc[0])


@pytest.mark.parametrize("seed,C,N,pad", [(0, 1, 64, 2), (1, 7, 256, 2), (2, 40, 512, 3), (3, 300, 1024, 2),
                                          (4, 25, 128, 0)])
def test_shelf_packing_matches_the_restatement_and_boxes_are_disjoint(seed, C, N, pad):
    rng = np.random.default_rng(seed)
    lo = rng.uniform(-1, 1, (C, 2))
    size = rng.uniform(0, 0.5, (C, 2)) ** 2
    size[rng.random(C) < 0.1] = 0.0  # point charts (singleton zero-area faces)
    box = np.concatenate([lo, lo + size], 1).astype(np.float32)
    st, off, s = _pack(box, N, pad)
    assert st == 0
    want_off, want_s = U.pack(box, N, pad)
    assert s == want_s and np.array_equal(off, want_off)
    # every box inside the texture, pairwise disjoint; the density is within the bisection's precision of the next
    occ = np.zeros((N, N), np.int32)
    wh = box[:, 2:].astype(np.float64) - box[:, :2].astype(np.float64)
    for c in range(C):
        bw, bh = (int(np.ceil(x * s)) + 2 * pad + 1 for x in wh[c])
        assert off[c, 0] >= 0 and off[c, 1] >= 0 and off[c, 0] + bw <= N and off[c, 1] + bh <= N
        occ[off[c, 1]:off[c, 1] + bh, off[c, 0]:off[c, 0] + bw] += 1
    assert occ.max() == 1
    hi = float(np.float32(s * (1 + 2 * U.REL_PREC)))
    assert U._shelf(list(wh[:, 0]), list(wh[:, 1]), s, N, pad) is not None
    assert s > 0 and hi > s


def test_packing_too_many_charts_is_unsupported():
    box = np.zeros((5000, 4), np.float32)
    box[:, 2:] = 0.01
    st, _, _ = _pack(box, 64, 2)
    assert st == -2


def test_no_material_export_clamps_and_slices():
    m = tt.find("no-material")({})
    f = torch.tensor([[-20.0, 0.0, 20.0], [3.0, -3.0, 0.5]])
    out = m.export(f, points=None)
    assert set(out) == {"albedo"}
    want = (torch.sigmoid(f) * 1.002 - 0.001).clamp(0, 1)
    assert torch.equal(out["albedo"], want)
    assert out["albedo"].min() == 0.0 and out["albedo"].max() == 1.0


class _M(SimpleNamespace):
    pass


def test_save_obj_writes_the_reference_line_formats(tmp_path):
    v_pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5], [0.25, 0.5, 1.0]])
    t_pos_idx = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    v_tex = torch.tensor([[0.1, 0.2], [0.9, 0.2], [0.1, 0.75], [0.5, 0.5]])
    t_tex_idx = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    v_nrm = torch.tensor([[0.0, 0.0, 1.0]] * 4)
    mesh = _M(v_pos=v_pos, t_pos_idx=t_pos_idx, v_tex=v_tex, t_tex_idx=t_tex_idx, v_nrm=v_nrm, v_rgb=None)
    rng = np.random.default_rng(0)
    tex = torch.from_numpy(rng.uniform(-0.2, 1.2, (6, 5, 3)).astype(np.float32))
    paths = save_obj(str(tmp_path / "model"), mesh, save_mat=True, save_normal=True, save_uv=True, map_Kd=tex,
                     map_format="png")
    assert paths == [str(tmp_path / "model.mtl"), str(tmp_path / "texture_kd.png"), str(tmp_path / "model.obj")]
    lines = open(tmp_path / "model.obj").read().splitlines()
    assert lines[:3] == ["mtllib model.mtl", "g object", "usemtl default"]
    vp = v_pos.numpy()
    assert lines[3:7] == [f"v {p[0]} {p[1]} {p[2]}" for p in vp]
    assert lines[7:11] == [f"vn {n[0]} {n[1]} {n[2]}" for n in v_nrm.numpy()]
    assert lines[11:15] == [f"vt {t[0]} {1.0 - t[1]}" for t in v_tex.numpy()]
    assert lines[15:] == ["f 1/1/1 2/2/2 3/3/3", "f 1/1/1 3/3/3 4/4/4"]
    assert open(tmp_path / "model.mtl").read() == "newmtl default\nKa 0.0 0.0 0.0\nmap_Kd texture_kd.png\nKs 0.0 0.0 0.0\n"
    want = (np.clip(tex.numpy(), 0, 1) * 255.0).astype(np.uint8)
    assert np.array_equal(read_png(str(tmp_path / "texture_kd.png")), want)
    # without uv / normals / material: "f a// b// c//", vertex colours on the v lines, Kd in the MTL
    mesh.v_rgb = torch.tensor([[1.0, 0.5, 0.25]] * 4)
    save_obj(str(tmp_path / "plain.obj"), mesh, save_vertex_color=True)
    lines = open(tmp_path / "plain.obj").read().splitlines()
    assert lines[0] == f"v {vp[0][0]} {vp[0][1]} {vp[0][2]} 1.0 0.5 0.25"
    assert lines[-1] == "f 1// 3// 4//"
    save_obj(str(tmp_path / "nomap.obj"), mesh, save_mat=True)
    assert "Kd 1.0 1.0 1.0" in open(tmp_path / "nomap.mtl").read()


def test_png_round_trip_every_channel_count(tmp_path):
    rng = np.random.default_rng(1)
    for shape in ((7, 9), (7, 9, 1), (7, 9, 3), (7, 9, 4), (1, 1, 3)):
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        p = tmp_path / "x.png"
        p.write_bytes(png_bytes(img))
        back = read_png(str(p))
        assert np.array_equal(back.reshape(img.shape), img)


def test_save_texture_without_save_uv_asserts_like_the_reference():
    exporter = tt.find("multiprompt-mesh-exporter")({"save_uv": False, "save_texture": True}, geometry=None,
                                                    material=None, background=None)
    mesh = _M(v_pos=None, t_pos_idx=None)
    with pytest.raises(AssertionError, match="save_uv must be True when save_texture is True"):
        exporter.export_obj_with_mtl(mesh, None)


def test_exporter_without_an_isosurface_raises_clearly():
    exporter = tt.find("multiprompt-mesh-exporter")({}, geometry=SimpleNamespace(), material=None, background=None)
    with pytest.raises(RuntimeError, match="isosurface"):
        exporter(torch.zeros(1))


def test_unwrap_uv_refuses_other_xatlas_options():
    from triplaneturbo_amd.isosurface import Mesh
    m = Mesh(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="max_iterations"):
        m.unwrap_uv({"max_iterations": 2}, {})
    with pytest.raises(NotImplementedError, match="bruteForce"):
        m.unwrap_uv({}, {"padding": 2, "bruteForce": True})
