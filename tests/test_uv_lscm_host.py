"""The conformal-chart reference (tests/uv_lscm_reference.py) on shapes whose answer is known, and the host side of
uv_atlas(method=...): no GPU.  A developable chart has E = 0, so its conformal map is an isometry: every UV edge as
long as its 3-D edge."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import _lib, ops
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_lscm_reference as L  # noqa: E402

ENTRY_POINTS = ["tt_uv_lscm_workspace_bytes", "tt_uv_lscm_table_ints", "tt_uv_lscm_index", "tt_uv_lscm_setup",
                "tt_uv_lscm_iterate", "tt_uv_lscm_finish", "tt_uv_lscm_emit"]


def _edge_lengths(P, tri):
    return np.concatenate([np.linalg.norm(P[tri[:, (k + 1) % 3]] - P[tri[:, k]], axis=1) for k in range(3)])


@pytest.mark.parametrize("shape", [L.flat_patch, L.half_cylinder])
def test_a_developable_chart_is_flattened_isometrically(shape):
    v, tri = shape()
    out = L.flatten(v, tri, np.zeros(len(tri), np.int64))
    assert not out["fallback"].any()
    assert out["energy"][0] <= 1e-20 * L.frames(v, tri)[3].sum()
    want = _edge_lengths(v.astype(np.float64), tri)
    got = _edge_lengths(out["uv_final"], out["t_tex"])
    assert np.abs(got / want - 1).max() <= 1e-8
    s1, s2, ratio, _ = L.stretch(v, tri, out["uv_final"], out["t_tex"])
    # (at sigma1 = sigma2 the closed form takes the root of a difference that is 0 up to rounding: sqrt(2^-52) = 1.5e-8)
    assert np.abs(s1 - 1).max() <= 1e-7 and np.abs(s2 - 1).max() <= 1e-7 and np.abs(ratio - 1).max() <= 1e-8
    # the principal axis lies along u: no covariance between u and v, and u the wider side
    d = out["uv_final"] - out["uv_final"].mean(0)
    assert abs((d[:, 0] * d[:, 1]).sum()) <= 1e-9 * (d ** 2).sum()
    assert (d[:, 0] ** 2).sum() >= (d[:, 1] ** 2).sum()


def test_the_flat_patch_needs_no_scale():
    """pins as far apart in UV as in space: on a flat chart the raw solution is the isometry already"""
    v, tri = L.flat_patch()
    out = L.flatten(v, tri, np.zeros(len(tri), np.int64))
    assert abs(out["scale"][0] - 1) <= 1e-9
    assert np.abs(_edge_lengths(out["uv"], out["t_tex"]) / _edge_lengths(v.astype(np.float64), tri) - 1).max() <= 1e-8


def test_a_single_triangle_comes_back_congruent():
    v = np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.5], [0.4, 0.8, -0.2]], np.float32)
    tri = np.array([[0, 1, 2]])
    out = L.flatten(v, tri, np.zeros(1, np.int64))
    assert not out["fallback"][0] and abs(out["scale"][0] - 1) <= 1e-12
    assert np.abs(_edge_lengths(out["uv"], out["t_tex"]) - _edge_lengths(v.astype(np.float64), tri)).max() <= 1e-12
    assert L.uv_areas(out["uv"], out["t_tex"])[0] > 0
    # the pins: the vertex farthest from the box centre, then the one farthest from it, at (0,0) and (d, 0)
    p0, p1 = out["pins"][0]
    assert np.array_equal(out["uv"][p0], [0, 0]) and out["uv"][p1, 1] == 0
    assert abs(out["uv"][p1, 0] - np.linalg.norm(v[p1].astype(np.float64) - v[p0])) <= 1e-15


def test_degenerate_charts_fall_back_in_the_reference():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5]], np.float32)
    out = L.flatten(v, np.array([[0, 1, 2], [3, 3, 3]]), np.array([0, 1]))  # a collinear face; a face in one point
    assert out["fallback"].tolist() == [True, True]


def test_uv_vertices_are_numbered_by_first_corner():
    tri = np.array([[0, 1, 2], [2, 1, 3], [3, 1, 4]])
    t_tex, vmesh, vchart = L.uv_vertices(tri, np.array([5, 2, 5]))
    assert t_tex.tolist() == [[0, 1, 2], [3, 4, 5], [6, 1, 7]]
    assert vmesh.tolist() == [0, 1, 2, 2, 1, 3, 3, 4] and vchart.tolist() == [5, 5, 5, 2, 2, 2, 5, 5]


def test_unknown_method_is_a_value_error():
    v, t = torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="nonsense"):
        ops.uv_atlas(v, t, method="nonsense")
    with pytest.raises(ValueError, match="nonsense"):
        Mesh(v, t).unwrap_uv(method="nonsense")
    assert ops.uv_method(None) == "axis" and ops.uv_method("axis") == "axis" and ops.uv_method("lscm") == "lscm"
    assert ops.UV_METHODS == ("axis", "lscm")


def test_abi_surface():
    assert "tt_uv_lscm.hip" in _lib.SOURCES
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("tt_uv_lscm_")) == sorted(ENTRY_POINTS)
    assert _lib.TT_ABI_VERSION == 17
    assert _lib.TT_UV_LSCM_TILE == 256 and _lib.TT_UV_LSCM_TILE % 64 == 0
    assert _lib.TT_UV_LSCM_DEFAULT_TOL == 1e-8 and ops.UV_LSCM_DEFAULT_MAX_ITERS == _lib.TT_UV_LSCM_DEFAULT_MAX_ITERS
    header = open(os.path.join(_lib.INCLUDE, "tt_abi.h")).read()
    assert "conformal UV charts (tt_uv_lscm.hip" in header
    assert _lib._PROTOS["tt_uv_lscm_iterate"][1][6] is _lib.ctypes.c_double  # tol travels as a double


def test_exporter_has_the_attribute_and_defaults_to_axis():
    import inspect

    from triplaneturbo_amd import export
    assert "self.uv_method: Optional[str] = None" in inspect.getsource(export)
    for fn in (Mesh.unwrap_uv, Mesh._unwrap_uv, ops.uv_atlas):
        assert inspect.signature(fn).parameters["method"].default == "axis"
