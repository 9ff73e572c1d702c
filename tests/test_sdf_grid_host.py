"""Mesh to SDF grid without a GPU: the numpy restatement (tests/sdf_grid_reference.py) held to the conditions the GPU
tests put on Mesh.solidify, the C ABI's argument checks, the Python-side argument errors and the ABI surface."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sdf_grid_reference as S  # noqa: E402

ENTRY_POINTS = ["tt_sdfgrid_workspace_bytes", "tt_sdfgrid_scatter", "tt_sdfgrid_corners", "tt_sdfgrid_finish"]


def test_abi_surface_and_version():
    assert _lib.TT_ABI_VERSION == 17  # new symbols only
    assert "tt_dist.hip" in _lib.SOURCES  # the kernels live with the closest-point routine they share
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_sdfgrid_")) == sorted(ENTRY_POINTS)
    assert (_lib.TT_SDFGRID_MAX_RES, _lib.TT_SDFGRID_MAX_BAND) == (512, 16)
    lib = _lib.load()
    assert lib.tt_abi_version() == 17


def test_c_abi_rejects_bad_arguments_without_touching_the_gpu():
    lib = _lib.load()
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(256)  # never dereferenced: validation fails first
    nan, inf = float("nan"), float("inf")
    for R, T in ((1, 4), (513, 4), (-3, 4), (32, 0), (32, -1), (32, (1 << 28) + 1)):
        assert lib.tt_sdfgrid_workspace_bytes(R, T) == -1
        assert lib.tt_sdfgrid_scatter(one, T, R, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, one, one, null) == -1
        assert lib.tt_sdfgrid_corners(R, T, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, one, 1, one, one, null) == -1
        assert lib.tt_sdfgrid_finish(R, T, 0.3, 0.3, one, one, one, one, one, 1, one, one, null) == -1
    assert lib.tt_sdfgrid_workspace_bytes(32, 100) >= 12 * 32 ** 3 + 8 * 101
    # h, tau, sign_tau: not finite, not positive, sign_tau below tau, a band beyond TT_SDFGRID_MAX_BAND + 1 cells
    for h, tau, sign_tau in ((0.0, 0.3, 0.3), (-0.1, 0.3, 0.3), (nan, 0.3, 0.3), (inf, 0.3, 0.3), (0.1, 0.0, 0.3),
                             (0.1, -0.3, 0.3), (0.1, nan, 0.3), (0.1, 0.3, 0.2), (0.1, 0.3, nan), (0.1, 0.3, inf),
                             (0.1, 1.0, 1.8)):
        assert lib.tt_sdfgrid_scatter(one, 4, 32, 0.0, 0.0, 0.0, h, tau, sign_tau, one, one, null) == -1
        assert lib.tt_sdfgrid_corners(32, 4, 0.0, 0.0, 0.0, h, tau, sign_tau, one, 1, one, one, null) == -1
    for tau, sign_tau in ((0.0, 0.3), (nan, 0.3), (0.3, 0.2), (0.3, nan)):
        assert lib.tt_sdfgrid_finish(32, 4, tau, sign_tau, one, one, one, one, one, 1, one, one, null) == -1
    for lo in ((nan, 0.0, 0.0), (0.0, inf, 0.0), (0.0, 0.0, -inf)):
        assert lib.tt_sdfgrid_scatter(one, 4, 32, *lo, 0.1, 0.3, 0.3, one, one, null) == -1
        assert lib.tt_sdfgrid_corners(32, 4, *lo, 0.1, 0.3, 0.3, one, 1, one, one, null) == -1
    # null pointers, n_cand out of range
    for args in ((null, one, one), (one, null, one), (one, one, null)):
        assert lib.tt_sdfgrid_scatter(args[0], 4, 32, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, args[1], args[2], null) == -1
        assert lib.tt_sdfgrid_corners(32, 4, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, args[0], 1, args[1], args[2], null) == -1
    for n_cand in (-1, 32 ** 3 + 1):
        assert lib.tt_sdfgrid_corners(32, 4, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, one, n_cand, one, one, null) == -1
        assert lib.tt_sdfgrid_finish(32, 4, 0.3, 0.3, one, one, one, one, one, n_cand, one, one, null) == -1
    assert lib.tt_sdfgrid_corners(32, 4, 0.0, 0.0, 0.0, 0.1, 0.3, 0.3, null, 0, null, null, null) == 0  # nothing to do
    for hole in range(7):  # workspace, corner, d2, nearest, winding | level, face
        a = [null if i == hole else one for i in range(7)]
        assert lib.tt_sdfgrid_finish(32, 4, 0.3, 0.3, *a[:5], 1, *a[5:], null) == -1


def test_python_argument_errors_come_before_any_tensor_is_touched():
    v = torch.zeros(3, 3)  # CPU tensors: only the argument checks can run
    t = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    for R in (1, 513, 0):
        with pytest.raises(ValueError, match="resolution"):
            ops.mesh_sdf_grid(v, t, R)
    with pytest.raises(TypeError):
        ops.mesh_sdf_grid(v, t, 32.0)
    for band in (0.0, -1.0, 16.5, float("nan"), "3", True):
        with pytest.raises(ValueError, match="band"):
            ops.mesh_sdf_grid(v, t, 64, band=band)
    # bounds=None needs R >= 2 * (ceil(band) + 1) + 2; explicit bounds do not
    for R, band in ((9, 3.0), (7, 2.0), (5, 0.5), (11, 3.5)):
        with pytest.raises(ValueError, match="leaves no room"):
            ops.mesh_sdf_grid(v, t, R, band=band)
        with pytest.raises(ValueError, match="leaves no room"):
            Mesh(v, t).sdf_grid(R, band=band)
        with pytest.raises(RuntimeError, match="must live on the GPU"):  # past the argument checks
            ops.mesh_sdf_grid(v, t, R, band=band, bounds=((0.0, 0.0, 0.0), 1.0))
    for bounds in (((0.0, 0.0), 1.0), ((0.0, 0.0, 0.0), 0.0), ((0.0, 0.0, float("nan")), 1.0), (1.0,), "box",
                   ((0.0, 0.0, 0.0), float("inf"))):
        with pytest.raises(ValueError, match="bounds"):
            ops.mesh_sdf_grid(v, t, 32, bounds=bounds)
    with pytest.raises(ValueError, match="beta"):
        ops.mesh_sdf_grid(v, t, 32, beta=0.0)
    # CPU tensors: the project's one answer for every op
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.mesh_sdf_grid(v, t, 32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        Mesh(v, t).solidify(32)
    m = Mesh(v, t)
    with pytest.raises(ValueError, match="band >= 1"):  # tau - h < 0: no offset fits, not even 0
        m.solidify(32, band=0.5)
    for offset in (float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="offset"):
            m.solidify(32, offset=offset)
    with pytest.raises(ValueError, match="project"):
        m.solidify(32, offset=0.01, project=True)
    with pytest.raises(ValueError, match="leaves no room"):
        m.solidify(9)


def test_default_bounds_leave_the_margin_and_match_the_restatement():
    rng = np.random.default_rng(0)
    for R, band in ((10, 3.0), (20, 2.0), (33, 0.5), (33, 3.5), (128, 3.0), (512, 16.0)):
        box_lo = rng.uniform(-2, 2, 3).astype(np.float32)
        box_hi = box_lo + rng.uniform(0.1, 3, 3).astype(np.float32)
        lo, h = ops.sdf_grid_bounds(box_lo, box_hi, R, band)
        lo_ref, h_ref = S.default_bounds(np.stack([box_lo, box_hi]), R, band)
        assert lo.dtype == np.float32 and np.array_equal(lo, lo_ref) and h == h_ref
        m = int(np.ceil(band)) + 1
        hi = lo.astype(np.float64) + float(h) * (R - 1)
        assert ((box_lo - lo.astype(np.float64)) / float(h) >= m - 1e-2).all()
        assert ((hi - box_hi) / float(h) >= m - 1e-2).all()
    with pytest.raises(ValueError, match="no extent"):
        ops.sdf_grid_bounds(np.zeros(3), np.zeros(3), 32, 3.0)


def test_far_sign_rule_of_the_restatement():
    R = 6
    sign_mask = np.zeros((R, R, R), bool)
    inside = np.zeros((R, R, R), bool)
    sign_mask[0, 0, [1, 3]] = True
    inside[0, 0, 1] = True      # row (0,0): + | - own | - carried | + own | + carried ...
    sign_mask[1, 2, 4] = True
    inside[1, 2, 4] = True      # row (1,2): + until 4, then -
    s = S.far_sign(sign_mask, inside, R)
    assert s[0, 0].tolist() == [1, -1, -1, 1, 1, 1]
    assert s[1, 2].tolist() == [1, 1, 1, 1, -1, -1]
    assert (s[2] == 1).all()  # no sign corner in a row: +


@pytest.fixture(scope="module")
def solids():
    """The restatement's solidify at R = 20, band = 2 on the three closed meshes, once."""
    out = {}
    for name in S.FIELDS:
        v, t = S.mesh(name)
        out[name] = (v, t, S.solidify(v, t, 20, band=2.0))
    return out


@pytest.mark.parametrize("name", list(S.FIELDS))
def test_restatement_meets_the_closed_input_conditions(solids, name):
    src_v, src_t, (v, t, info) = solids[name]
    assert info["components_dropped"] == 0
    S.check_closed_input(name, v, t, src_v, src_t, float(info["h"]))
    # the band is what the field says it is: corners nearer than tau, and the level is the clamped signed distance
    level, gi = S.sdf_grid(src_v, src_t, 20, 2.0)
    assert gi["band_corners"] == int(gi["band"].sum()) > 0
    assert (np.abs(level[~gi["band"]]) == float(gi["tau"])).all() and (np.abs(level[gi["band"]]) < float(gi["tau"])).all()
    assert (gi["face"][gi["band"]] >= 0).all() and (gi["face"][~gi["band"]] == -1).all()
    # closed input: the far sign is the true sign (exact winding number of every corner)
    P = S.corners(gi["lo"], gi["h"], 20).reshape(-1, 3)
    inside = S.W.exact(P, src_v, src_t) > 0.5
    assert np.array_equal(level.reshape(-1) < 0, inside)


def test_restatement_merges_overlapping_spheres():
    meshes = [S.analytic_sphere(c, r) for c, r in S.OVERLAP]
    v, t, info = S.solidify(*S.concat(*meshes), 20, band=2.0)
    sd = np.stack([S.signed_distance_to_mesh(v, *m) for m in meshes], -1)
    S.check_overlap(v, t, sd, float(info["h"]))


def test_restatement_drops_the_cavity_wall_and_keeps_it_on_request():
    src = S.sphere_with_cavity()
    c, r_out, r_in = S.NESTED
    v, t, info = S.solidify(*src, 20, band=2.0)
    h = float(info["h"])
    assert info["components_dropped"] == 1
    assert S.is_closed(t, len(v)) and S.n_components(v, t) == 1
    assert np.abs(S.distance_to_mesh(v, *S.analytic_sphere(c, r_out))).max() <= h * (1 + 1e-4)
    v2, t2, info2 = S.solidify(*src, 20, band=2.0, keep_cavities=True)
    assert info2["components_dropped"] == 0
    assert S.is_closed(t2, len(v2)) and S.n_components(v2, t2) == 2


def test_restatement_offsets_the_sphere():
    v_src, t_src = S.analytic_sphere((0.5, 0.5, 0.5), 0.33)
    _, gi = S.sdf_grid(v_src, t_src, 20, 3.0)
    h = float(gi["h"])
    v, t, _ = S.solidify(v_src, t_src, 20, band=3.0, offset=2 * h)
    assert S.is_closed(t, len(v))
    radius = np.linalg.norm(v.astype(np.float64) - 0.5, axis=-1)
    assert np.abs(radius - (0.33 + 2 * h)).max() <= h
    with pytest.raises(ValueError):
        S.solidify(v_src, t_src, 20, band=3.0, offset=2.01 * h)
