"""Tangents and the normal-map encode without a GPU: the contract's float64 restatement (tests/tangent_reference.py)
against the reference's own Mesh._compute_vertex_tangent (tests/golden/reference_mesh_tangent.npz), the conditioning
the GPU test's bound rests on, the degenerate rule, encode -> decode, the bitangent's direction, and the library's
surface (header section, symbols, argument checks that run before any HIP call)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_reference as M  # noqa: E402
import tangent_reference as TR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sphere17", "torus24", "blobs33")
ENTRY_POINTS = ["tt_bake_tangents", "tt_bake_project", "tt_bake_encode"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_mesh_tangent.npz"))


def _mesh(golden, name):
    v, t = golden[f"{name}_v_pos"], golden[f"{name}_t_pos_idx"]
    return v, t, golden[f"{name}_v_tex"], golden[f"{name}_t_tex_idx"], M.vertex_normals(v, t)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(golden, name):
    v, t, vt, tt_, nrm = _mesh(golden, name)
    want = golden[f"{name}_v_tng"]
    assert np.isfinite(want).all()
    got, st = TR.tangents(v, t, vt, tt_, nrm, "pos", with_stats=True)
    err = np.abs(got - want).max()
    print(f"{name}: max |restatement - reference| = {err:.2e}")
    assert err <= 1e-12
    assert not st["degenerate"].any()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("group", ["pos", "tex"])
def test_no_group_is_ill_conditioned(golden, name, group):
    """what the GPU test's 1e-5 rests on: no cancellation in the sum (|sum tang| / sum |tang| >= 0.1) or in the
    Gram-Schmidt step (|t - (t.n) n| >= 0.1), so fp32 rounding is amplified by at most ~10 x each"""
    v, t, vt, tt_, nrm = _mesh(golden, name)
    out, st = TR.tangents(v, t, vt, tt_, nrm, group, with_stats=True)
    print(f"{name} {group}: cond >= {st['cond'].min():.3f}, perp >= {st['perp'].min():.3f}, clamped {st['clamped']}")
    assert st["cond"].min() >= 0.1 and st["perp"].min() >= 0.1
    assert np.abs(np.linalg.norm(out, axis=1) - 1).max() <= 1e-12
    n = nrm if group == "pos" else None
    if n is not None:
        assert np.abs((out * n).sum(1)).max() <= 1e-12
    if name == "blobs33":
        assert st["clamped"] == 13  # faces on the denom clamp


def test_degenerate_rule_on_the_hand_mesh():
    v, t = M.hand_mesh()
    vt, tt_ = TR.atlas(v, t, 128, 2)
    nrm = M.vertex_normals(v, t)
    for group in ("pos", "tex"):
        out, st = TR.tangents(v, t, vt, tt_, nrm, group, with_stats=True)
        assert np.isfinite(out).all()
        assert np.abs(np.linalg.norm(out, axis=1) - 1).max() <= 1e-12
        if group == "pos":
            assert st["degenerate"][10]  # the unreferenced vertex
            assert np.abs((out * nrm).sum(1)).max() <= 1e-12
            assert np.allclose(out[10], TR.perp(nrm[10]))
    for n in ([0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8], [1 / 3 ** 0.5] * 3, [-0.2, 0.9, (1 - 0.85) ** 0.5]):
        p = TR.perp(n)
        assert abs(p @ p - 1) <= 1e-12 and abs(p @ np.asarray(n)) <= 1e-12
    assert np.array_equal(TR.perp([1 / 3 ** 0.5] * 3)[1:] < 0, [True, True])  # ties take the first axis: x


def _random_rast(T, H, W, seed):
    rng = np.random.RandomState(seed)
    u = rng.uniform(0, 1, (H, W))
    w = rng.uniform(0, 1, (H, W)) * (1 - u)
    fid = rng.randint(1, T + 1, (H, W)).astype(np.float64)
    fid[rng.uniform(size=(H, W)) < 0.1] = 0.0  # uncovered
    fid[0, 0] = T + 1.0  # not a face: uncovered too
    return np.stack([u, w, np.zeros((H, W)), fid], -1)


def test_encode_decode_is_the_identity(golden):
    v, t, vt, tt_, nrm = _mesh(golden, "torus24")
    tng = TR.tangents(v, t, vt, tt_, nrm, "tex")
    rast = _random_rast(len(t), 24, 24, 5)
    m = np.random.RandomState(6).normal(size=(24, 24, 3)) * 3.0
    img, cov, back = TR.encode(rast, nrm, t, tng, tt_, m)
    assert cov.sum() > 400 and (~cov).sum() > 0 and back.sum() > 0
    assert np.array_equal(img[~cov], np.broadcast_to([0.5, 0.5, 1.0], img[~cov].shape))
    assert img.min() >= -1e-12 and img.max() <= 1 + 1e-12
    _, th, bh, nh = TR.frames(rast, nrm, t, tng, tt_)
    mh = m / np.linalg.norm(m, axis=-1, keepdims=True)
    assert np.abs(TR.decode(img, th, bh, nh) - mh)[cov].max() <= 1e-12
    # the frame is orthonormal and right-handed as (t^, n^, b^): b^ = t^ x n^
    for a, b in ((th, bh), (th, nh), (bh, nh)):
        assert np.abs((a * b).sum(-1))[cov].max() <= 1e-12
    assert np.abs(np.cross(th, nh) - bh)[cov].max() <= 1e-12


def test_bitangent_points_along_increasing_obj_v():
    """a skewed two-triangle quad P(u, v) = O + u A + v B with its UVs = (u, v), positively oriented as the atlas makes
    them: save_obj writes vt = (u, 1 - v), so the OBJ's v grows along -B, and that is where b^ = t^ x n^ points"""
    O, A, B = np.array([0.1, -0.2, 0.3]), np.array([1.0, 0.2, 0.1]), np.array([-0.1, 1.0, 0.3])
    uv = np.array([[0.2, 0.2], [0.8, 0.2], [0.8, 0.7], [0.2, 0.7]], np.float32)
    v = (O + uv[:, :1].astype(np.float64) * A + uv[:, 1:].astype(np.float64) * B).astype(np.float32)
    t = np.array([[0, 1, 2], [0, 2, 3]])
    nrm = M.vertex_normals(v, t)
    assert (nrm @ np.cross(A, B) > 0).all()  # dP/du x dP/dv is parallel to +n: positive UV area
    tng = TR.tangents(v, t, uv, t, nrm, "tex")
    assert (tng @ A > 0.9 * np.linalg.norm(A)).all()  # t^ follows dP/du
    rast = np.array([[[0.3, 0.3, 0.0, 1.0], [0.2, 0.5, 0.0, 2.0]]])
    cov, th, bh, nh = TR.frames(rast, nrm, t, tng, t)
    assert cov.all()
    d_obj_v = -(B - (B @ nh[0, 0]) * nh[0, 0])  # dP / d(OBJ v), in the face's plane
    for b in bh[0]:
        assert b @ d_obj_v > 0.9 * np.linalg.norm(d_obj_v)
    # a field normal tilted towards increasing OBJ v has a green channel above 0.5
    img, _, _ = TR.encode(rast, nrm, t, tng, t, np.broadcast_to(nh[0, 0] + 0.3 * d_obj_v, (1, 2, 3)))
    assert (img[..., 1] > 0.55).all() and (img[..., 2] > 0.9).all()


def test_obj_uv_is_what_the_files_carry(golden, tmp_path):
    """Mesh.v_tng_tex is built on obj_uv(v_tex), so that the exporter's mesh and the one load_obj returns build their
    tangents on the same UVs: save_obj -> load_obj turns v_tex into exactly obj_uv(v_tex), obj_uv changes nothing on a
    second pass, and it moves v by at most 2^-25 (half an ulp of 1 - v) and u not at all"""
    from triplaneturbo_amd import viewer
    from triplaneturbo_amd.export import save_obj
    from triplaneturbo_amd.isosurface import Mesh, obj_uv
    rng = np.random.RandomState(3)
    edge = np.float32([[0.0, 0.0], [1.0, 1.0], [0.5, 0.5], [0.25, 2.0 ** -25], [0.75, 1 - 2.0 ** -24], [0.1, 1e-9]])
    for name, vt in (("torus24", golden["torus24_v_tex"]),
                     ("random", np.concatenate([edge, rng.uniform(0, 1, (500, 2)).astype(np.float32),
                                                (rng.uniform(0, 1, (500, 2)) ** 8).astype(np.float32)]))):
        vt = torch.from_numpy(np.ascontiguousarray(vt, np.float32))
        idx = (torch.arange(3 * (len(vt) // 3), dtype=torch.int32) % len(vt)).reshape(-1, 3)
        mesh = Mesh(torch.from_numpy(rng.normal(size=(len(vt), 3)).astype(np.float32)), idx)
        mesh._v_tex, mesh._t_tex_idx = vt, idx
        save_obj(str(tmp_path / name), mesh, save_uv=True)
        loaded, _ = viewer.load_obj(str(tmp_path / f"{name}.obj"))
        q = obj_uv(vt)
        assert q.dtype == torch.float32 and q.is_contiguous() and not q.requires_grad
        assert torch.equal(loaded.v_tex, q) and torch.equal(obj_uv(q), q)
        assert torch.equal(loaded.v_pos, mesh.v_pos) and torch.equal(loaded.t_tex_idx, idx)
        assert torch.equal(q[:, 0], vt[:, 0]) and (q[:, 1].double() - vt[:, 1].double()).abs().max() <= 2.0 ** -25
        assert name != "random" or not torch.equal(q, vt)  # and the files do move some v


def test_library_surface():
    assert "tt_bake.hip" in _lib.SOURCES
    text = open(os.path.join(ROOT, "include", "tt_abi.h")).read()
    assert "tangents and normal-map baking (tt_bake.hip)" in text
    protos = re.findall(r"^int (tt_bake_\w+)\(", text, re.M)
    assert sorted(protos) == sorted(ENTRY_POINTS)
    for name in protos:
        assert name in _lib.SYMBOLS
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_bake_")) == sorted(ENTRY_POINTS)
    assert (_lib.TT_BAKE_GROUP_POS, _lib.TT_BAKE_GROUP_TEX) == (0, 1)
    for rule in ("degenerate", "project", "encode", "b^ = t^ x n^"):
        assert rule in text.split("tangents and normal-map baking (tt_bake.hip)")[1]


def test_argument_checks_run_before_any_hip_call():
    lib = _lib.load()
    bad = _lib.TT_ERR_BAD_ARG if hasattr(_lib, "TT_ERR_BAD_ARG") else -1
    assert lib.tt_bake_tangents(None, None, None, None, None, None, None, 4, 4, 2, 7, None, None) == bad  # group
    assert lib.tt_bake_tangents(None, None, None, None, None, None, None, 4, 4, 2, 0, None, None) == bad  # null
    assert lib.tt_bake_tangents(None, None, None, None, None, None, None, 0, 0, 0, 0, None, None) == 0  # nothing to do
    assert lib.tt_bake_project(None, None, None, None, -1, 0.1, None) == bad
    assert lib.tt_bake_project(None, None, None, None, 8, -0.1, None) == bad
    assert lib.tt_bake_project(None, None, None, None, 8, float("nan"), None) == bad
    assert lib.tt_bake_project(None, None, None, None, 8, 0.1, None) == bad  # null
    assert lib.tt_bake_project(None, None, None, None, 0, 0.1, None) == 0
    assert lib.tt_bake_encode(None, None, None, None, None, None, 4, 4, 2, 8, 8, None, None, None) == bad
    assert lib.tt_bake_encode(None, None, None, None, None, None, 0, 4, 2, 0, 0, None, None, None) == bad  # T > 0, V = 0


def test_python_argument_errors_need_no_gpu():
    z3, z2, i3 = torch.zeros(3, 3), torch.zeros(3, 2), torch.zeros(1, 3, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.mesh_tangents(z3, i3, z2, i3, z3, group="face")
    with pytest.raises(RuntimeError):
        ops.mesh_tangents(z3, i3, z2, i3, z3)  # no CPU path
    from triplaneturbo_amd import viewer
    with pytest.raises(ValueError):
        viewer.render_textured(None, None, None, 8, 8, mode="bump")
    exp_cls = __import__("triplaneturbo_amd").find("multiprompt-mesh-exporter")
    exp = exp_cls({}, geometry=None, material=None, background=None)
    assert exp.bake_normal_map is False and exp.bake_project_steps == 2
