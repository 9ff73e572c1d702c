"""HIP vertex tangents (tt_bake_tangents; ops.mesh_tangents, Mesh.v_tng / v_tng_tex) against the contract's float64
restatement (tests/tangent_reference.py) and the reference's own tangents (tests/golden/reference_mesh_tangent.npz).

The bound, 1e-5 on every component of every group with nothing excluded: the kernel adds a handful of fp32 face tangents
per group and normalises twice; tests/test_tangent_host.py shows that no group of these meshes cancels by more than 10 x
in the sum or in the Gram-Schmidt step, and an fp32 restatement of the same sums stays within 6.4e-7 of the float64 one
on all twelve cases, so 1e-5 leaves 15 x over fp32 rounding."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import ops
from triplaneturbo_amd.isosurface import Mesh, obj_uv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_reference as M  # noqa: E402
import tangent_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sphere17", "torus24", "blobs33")
TOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_mesh_tangent.npz"))


@pytest.fixture(scope="module")
def cases(dev, golden):
    """(name, N) -> the mesh on the GPU with its HIP atlas at N^2, padding 2, and the float64 restatement of both
    groupings from the GPU's own v_nrm and UVs (computed once, shared by the tests below)"""
    out = {}
    for name in NAMES:
        v = torch.from_numpy(golden[f"{name}_v_pos"]).to(dev)
        t = torch.from_numpy(golden[f"{name}_t_pos_idx"]).to(dev)
        for N in (128, 256):
            mesh = Mesh(v, t)
            mesh.unwrap_uv(xatlas_pack_options={"padding": 2}, texture_size=N)
            args = [x.cpu().numpy() for x in (mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm)]
            out[name, N] = (mesh, {g: TR.tangents(*args, g) for g in ("pos", "tex")})
    return out


@pytest.mark.parametrize("group", ["pos", "tex"])
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("name", NAMES)
def test_tangents_match_the_restatement(cases, name, N, group):
    mesh, want = cases[name, N]
    got = ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm, group)
    assert got.shape == want[group].shape and got.dtype == torch.float32 and not got.requires_grad
    err = np.abs(got.cpu().numpy().astype(np.float64) - want[group]).max()
    print(f"{name} N={N} {group}: max error {err:.2e} over {len(want[group])} groups")
    assert err <= TOL
    again = ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm, group)
    assert torch.equal(got, again)  # bit-identical from run to run
    if group == "pos":
        assert torch.equal(mesh.v_tng, got)
    else:  # the property is the same call on the UVs as an OBJ file carries them (isosurface.obj_uv)
        assert torch.equal(mesh.v_tng_tex, ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, obj_uv(mesh.v_tex),
                                                             mesh.t_tex_idx, mesh.v_nrm, "tex"))


@pytest.mark.parametrize("name", NAMES)
def test_v_tng_equals_the_reference(dev, golden, name):
    """Mesh.v_tng against threestudio's _compute_vertex_tangent (float64), on the inputs the reference saw: the golden's
    positions and UVs (set the way viewer.load_obj sets them).  The UVs are an input of the comparison, not a detail:
    a sliver face's tangent amplifies an ulp of its UVs, and a face on the denom clamp changes weight with the atlas's
    scale.  The float64 restatement itself, fed the restated atlas at 1024^2 instead of 128^2, is 1.2e-5 from this golden
    on torus24 and 5e-2 on blobs33 (13 clamped faces)."""
    mesh = Mesh(torch.from_numpy(golden[f"{name}_v_pos"]).to(dev), torch.from_numpy(golden[f"{name}_t_pos_idx"]).to(dev))
    mesh._v_tex = torch.from_numpy(golden[f"{name}_v_tex"]).to(dev)
    mesh._t_tex_idx = torch.from_numpy(golden[f"{name}_t_tex_idx"]).to(dev)
    err = np.abs(mesh.v_tng.cpu().numpy().astype(np.float64) - golden[f"{name}_v_tng"]).max()
    print(f"{name}: max |v_tng - reference| = {err:.2e}")
    assert err <= TOL


def test_v_tng_unwraps_on_first_use_and_never_requires_grad(dev, golden):
    hot = torch.from_numpy(golden["sphere17_v_pos"]).to(dev).requires_grad_(True)
    mesh = Mesh(hot, torch.from_numpy(golden["sphere17_t_pos_idx"]).to(dev))
    assert mesh._v_tex is None and mesh.v_nrm.requires_grad
    tng = mesh.v_tng
    assert mesh._v_tex is not None and tng.shape == hot.shape and not tng.requires_grad
    assert mesh.v_tng_tex.shape == (mesh.v_tex.shape[0], 3) and not mesh.v_tng_tex.requires_grad
    assert torch.equal(tng, ops.mesh_tangents(mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm))
    mesh.unwrap_uv(texture_size=128)  # new UVs: the tangents are rebuilt from them
    assert mesh._v_tng is None and mesh._v_tng_tex is None
    assert mesh.v_tng_tex.shape == (mesh.v_tex.shape[0], 3)


def test_hand_mesh_gives_finite_unit_tangents(dev):
    v, t = M.hand_mesh()
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev).int())
    mesh.unwrap_uv(texture_size=128)
    nrm = mesh.v_nrm.cpu().numpy().astype(np.float64)
    for group, got in (("pos", mesh.v_tng), ("tex", mesh.v_tng_tex)):
        g = got.cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all()
        assert np.abs(np.linalg.norm(g, axis=1) - 1).max() <= TOL
        vt = mesh.v_tex if group == "pos" else obj_uv(mesh.v_tex)
        want = TR.tangents(v, t, vt.cpu().numpy(), mesh.t_tex_idx.cpu().numpy(), nrm, group)
        assert np.abs(g - want).max() <= TOL
    g = mesh.v_tng.cpu().numpy().astype(np.float64)
    assert np.abs((g * nrm).sum(1)).max() <= TOL
    assert np.abs(g[10] - TR.perp(nrm[10])).max() <= TOL  # the unreferenced vertex: the fixed perpendicular


def test_argument_errors(dev):
    v, t = M.hand_mesh()
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev).int())
    a = (mesh.v_pos, mesh.t_pos_idx, mesh.v_tex, mesh.t_tex_idx, mesh.v_nrm)
    with pytest.raises(ValueError):
        ops.mesh_tangents(*a, group="face")
    with pytest.raises(ValueError):
        ops.mesh_tangents(a[0], a[1] + 5, *a[2:])  # an index outside [0, V)
    with pytest.raises(ValueError):
        ops.mesh_tangents(a[0], a[1], a[2], a[3][:-1], a[4])
    empty = ops.mesh_tangents(a[0], a[1][:0], a[2], a[3][:0], a[4])  # no faces: every vertex takes the fixed perpendicular
    assert empty.shape == a[0].shape and torch.isfinite(empty).all()
