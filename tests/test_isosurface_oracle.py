"""The numpy marching-cubes oracle (tests/mc_reference.py) on analytic fields, checked with properties that do not use
the case table: closed and consistently oriented surfaces, Euler characteristics, enclosed volume, normals, components,
open boundaries only on the box faces.  (The GPU tests then compare the HIP kernels with this oracle exactly.)"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_reference as M  # noqa: E402


def grid(R):
    x = np.linspace(0.0, 1.0, R)
    return np.stack(np.meshgrid(x, x, x, indexing="ij"), -1)


def sphere(R, c=(0.5, 0.5, 0.5), r=0.33):
    return (np.linalg.norm(grid(R) - np.array(c), axis=-1) - r).astype(np.float32)


def torus(R, big=0.28, small=0.1):
    p = grid(R) - 0.5
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - big
    return (np.sqrt(q ** 2 + p[..., 2] ** 2) - small).astype(np.float32)


def two_spheres(R):
    return np.minimum(sphere(R, (0.3, 0.5, 0.5), 0.15), sphere(R, (0.72, 0.5, 0.5), 0.15)).astype(np.float32)


def closed_once(tri, n_vert):
    """every directed edge appears exactly once and its reverse exactly once"""
    d = M.directed_edges(tri)
    keys = M.edge_key(d, n_vert)
    rev = M.edge_key(d[:, ::-1], n_vert)
    return len(np.unique(keys)) == len(keys) and np.array_equal(np.sort(keys), np.sort(rev))


@pytest.mark.parametrize("R", [33, 64])
def test_sphere_closed_genus0_volume_and_outward_normals(R):
    r = 0.33
    mc = M.marching_cubes(sphere(R, r=r))
    v, t = mc.v_pos, mc.t_pos_idx
    assert len(t) > 0 and np.isfinite(v).all()
    assert closed_once(t, len(v))
    assert M.euler_characteristic(v, t) == 2
    vol = M.signed_volume(v, t)
    exact = 4.0 / 3.0 * math.pi * r ** 3
    assert vol > 0
    if R == 64:
        assert abs(vol - exact) / exact < 0.01, (vol, exact)
    w = v[t.astype(np.int64)].astype(np.float64)
    n = np.cross(w[:, 1] - w[:, 0], w[:, 2] - w[:, 0])
    out = np.einsum("ij,ij->i", n, w.mean(1) - 0.5)
    assert (out > 0).all()
    # vertices on the sphere up to the linear interpolation error
    assert np.abs(np.linalg.norm(v - 0.5, axis=-1) - r).max() < 1.0 / (R - 1)


@pytest.mark.parametrize("R", [33, 64])
def test_torus_euler_characteristic_zero(R):
    mc = M.marching_cubes(torus(R))
    assert closed_once(mc.t_pos_idx, len(mc.v_pos))
    assert M.euler_characteristic(mc.v_pos, mc.t_pos_idx) == 0
    assert M.signed_volume(mc.v_pos, mc.t_pos_idx) > 0


@pytest.mark.parametrize("R", [33, 64])
def test_two_disjoint_spheres(R):
    mc = M.marching_cubes(two_spheres(R))
    assert closed_once(mc.t_pos_idx, len(mc.v_pos))
    assert M.connected_components(len(mc.v_pos), mc.t_pos_idx) == 2
    assert M.euler_characteristic(mc.v_pos, mc.t_pos_idx) == 4


def _on_box_face(mc, vid):
    """(V, 6) bool: the vertex's edge lies on box face (axis, side)"""
    R = mc.res
    p0 = np.stack(np.unravel_index(mc.p0[vid], (R, R, R)), -1)
    ax = mc.axis[vid]
    out = np.zeros((len(vid), 6), dtype=bool)
    for c in range(3):
        off = ax != c
        out[:, 2 * c] = off & (p0[:, c] == 0)
        out[:, 2 * c + 1] = off & (p0[:, c] == R - 1)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_field_is_open_only_on_the_box_faces(seed):
    level = np.random.default_rng(seed).standard_normal((17, 17, 17)).astype(np.float32)
    mc = M.marching_cubes(level, isovalue=0.1)
    t = mc.t_pos_idx.astype(np.int64)
    assert len(t) > 1000
    bad = M.unmatched_directed_edges(t, len(mc.v_pos))
    assert bad, "a random field crosses the box faces"
    e = np.array(bad)
    u, v = e // len(mc.v_pos), e % len(mc.v_pos)
    fu, fv = _on_box_face(mc, u), _on_box_face(mc, v)
    assert (fu & fv).any(1).all(), "an open edge inside the box"


def test_random_field_away_from_the_box_is_closed():
    level = np.random.default_rng(3).standard_normal((17, 17, 17)).astype(np.float32)
    level[[0, -1]] = 1.0
    level[:, [0, -1]] = 1.0
    level[:, :, [0, -1]] = 1.0
    mc = M.marching_cubes(level)
    assert len(mc.t_pos_idx) > 500
    assert not M.unmatched_directed_edges(mc.t_pos_idx, len(mc.v_pos))


def test_values_exactly_at_the_isovalue():
    rng = np.random.default_rng(4)
    level = rng.integers(-1, 2, size=(20, 20, 20)).astype(np.float32)
    level[[0, -1]] = 1.0
    level[:, [0, -1]] = 1.0
    level[:, :, [0, -1]] = 1.0
    assert (level == 0).sum() > 1000
    mc = M.marching_cubes(level, isovalue=0.0)
    assert len(mc.t_pos_idx) > 0 and np.isfinite(mc.v_pos).all()
    assert not M.unmatched_directed_edges(mc.t_pos_idx, len(mc.v_pos))
    # a level exactly at the isovalue is outside: the vertex of an edge ending there sits on that grid point
    flat = level.reshape(-1)
    at = flat[mc.p1] == 0
    assert at.sum() > 100
    p1 = np.stack(np.unravel_index(mc.p1[at], level.shape), -1)
    assert np.abs(mc.v_pos[at] * 19 - p1).max() < 1e-5


def test_deformation_moves_vertices_by_the_interpolated_offset():
    R = 17
    lv = sphere(R)
    d = np.random.default_rng(5).uniform(-0.3, 0.3, (R, R, R, 3)).astype(np.float32)
    a = M.marching_cubes(lv)
    b = M.marching_cubes(lv, d)
    z = M.marching_cubes(lv, np.zeros_like(d))
    assert np.array_equal(a.t_pos_idx, b.t_pos_idx)
    assert np.array_equal(a.v_pos, z.v_pos)  # a zero deformation is exactly no deformation
    flat = lv.reshape(-1)
    t = (0 - flat[a.p0]) / (flat[a.p1] - flat[a.p0])
    dd = d.reshape(-1, 3)
    want = a.v_pos.astype(np.float64) + ((1 - t)[:, None] * dd[a.p0] + t[:, None] * dd[a.p1]) / (R - 1)
    assert np.abs(b.v_pos - want).max() < 1e-6
