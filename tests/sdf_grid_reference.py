"""numpy restatement of the mesh-to-SDF-grid contract (include/tt_abi.h, "mesh to SDF grid") and of Mesh.solidify, from
the float64 pair distance of tests/distance_reference.py, the exact winding sum of tests/winding_reference.py and the
marching-cubes oracle of tests/mc_reference.py: the corners, the band, the sign corners, the far-sign rule along the
last axis, the components and their signed volumes.  Nothing here knows the kernel's scatter.  Besides: the meshes of
tests/test_sdf_grid_host.py and tests/test_gpu_sdf_grid.py and the conditions both put on a solidified mesh."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import mc_reference as M  # noqa: E402
import test_isosurface_oracle as ISO  # noqa: E402
import winding_reference as W  # noqa: E402

F32 = np.float32
SIGN_BAND = 1.0 + 2.0 ** -10  # cells: corners nearer than this evaluate their own winding number


# ---------------------------------------------------------------------------------------------------------------
# meshes: marching cubes of analytic fields on [0,1]^3 (outward oriented, closed), at most 32^3
FIELDS = {"sphere": ISO.sphere, "torus": ISO.torus, "two_spheres": ISO.two_spheres}
GENUS_SUM = {"sphere": (1, 2), "torus": (1, 0), "two_spheres": (2, 4)}  # (components, Euler characteristic)


def mesh(name, res=16):
    mc = M.marching_cubes(FIELDS[name](res))
    return mc.v_pos.astype(F32), mc.t_pos_idx.astype(np.int32)


def analytic_sphere(c, r, res=16):
    mc = M.marching_cubes(ISO.sphere(res, c, r))
    return mc.v_pos.astype(F32), mc.t_pos_idx.astype(np.int32)


def concat(*meshes):
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(v)
        ts.append(t + base)
        base += len(v)
    return np.concatenate(vs).astype(F32), np.concatenate(ts).astype(np.int32)


OVERLAP = (((0.4, 0.5, 0.5), 0.2), ((0.6, 0.5, 0.5), 0.2))  # two analytic spheres, centres 0.2 apart
NESTED = ((0.5, 0.5, 0.5), 0.33, 0.15)  # centre, outer radius, radius of the inward-oriented inner sphere


def overlapping_spheres(res=16):
    return concat(*(analytic_sphere(c, r, res) for c, r in OVERLAP))


def sphere_with_cavity(res=16):
    c, r_out, r_in = NESTED
    v, t = analytic_sphere(c, r_in, res)
    return concat(analytic_sphere(c, r_out, res), (v, t[:, ::-1].copy()))


# ---------------------------------------------------------------------------------------------------------------
# the grid
def default_bounds(v_pos, R, band):
    """(lo (3,) fp32, h fp32): the cube about the box's centre in which the largest extent spans R - 1 - 2 m cells,
    m = ceil(band) + 1 (h carries a relative 2^-20)."""
    lo, hi = v_pos.min(0).astype(np.float64), v_pos.max(0).astype(np.float64)
    m = int(np.ceil(band)) + 1
    h = (hi - lo).max() * (1.0 + 2.0 ** -20) / (R - 1 - 2 * m)
    return ((lo + hi) * 0.5 - h * (R - 1) * 0.5).astype(F32), F32(h)


def corners(lo, h, R):
    """(R,R,R,3) fp32: lo + idx * h, the product and the sum each rounded to fp32."""
    idx = np.stack(np.meshgrid(*[np.arange(R, dtype=F32)] * 3, indexing="ij"), -1)
    return (np.asarray(lo, F32) + (idx * F32(h)).astype(F32)).astype(F32)


def far_sign(sign_mask, inside, R):
    """(R,R,R) +-1: a sign corner's own sign; elsewhere that of the nearest sign corner below it along the last axis
    in its (i, j) row, + when there is none."""
    out = np.ones((R, R, R))
    for k in range(R):
        prev = out[:, :, k - 1] if k else np.ones((R, R))
        out[:, :, k] = np.where(sign_mask[:, :, k], np.where(inside[:, :, k], -1.0, 1.0), prev)
    return out


def sdf_grid(v_pos, t_pos_idx, R, band, bounds=None):
    """The contract in float64: level (R,R,R), and {lo, h, tau, face, band (mask), band_corners}."""
    lo, h = default_bounds(v_pos, R, band) if bounds is None else (np.asarray(bounds[0], F32),
                                                                   F32(bounds[1]) / F32(R - 1))
    tau, sign_tau = F32(band) * h, F32(max(band, SIGN_BAND)) * h
    P = corners(lo, h, R).reshape(-1, 3)
    d2 = D.pair_matrix(P, v_pos, t_pos_idx)
    best, face = d2.min(1)
    d = best.sqrt().numpy().reshape(R, R, R)
    band_mask, sign_mask = d < float(tau), d < float(sign_tau)
    inside = np.zeros(R ** 3, bool)
    inside[sign_mask.reshape(-1)] = W.exact(P[sign_mask.reshape(-1)], v_pos, t_pos_idx) > 0.5
    sgn = far_sign(sign_mask, inside.reshape(R, R, R), R)
    level = sgn * np.where(band_mask, d, float(tau))
    return level, {"lo": lo, "h": h, "tau": tau, "band": band_mask,
                   "face": np.where(band_mask, face.numpy().reshape(R, R, R), -1), "band_corners": int(band_mask.sum())}


def face_components(n_vert, tri):
    """(T,) component label of every face (faces joined through shared vertices)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components as cc
    d = M.directed_edges(tri)
    g = sp.coo_matrix((np.ones(len(d)), (d[:, 0], d[:, 1])), shape=(n_vert, n_vert))
    return cc(g, directed=False)[1][np.asarray(tri, np.int64)[:, 0]]


def solidify(v_pos, t_pos_idx, R, band=3.0, offset=0.0, keep_cavities=False):
    """(v, t, info): sdf_grid, marching cubes at `offset`, the vertices back through lo and h, components, and unless
    keep_cavities every component of negative signed volume dropped."""
    level, info = sdf_grid(v_pos, t_pos_idx, R, band)
    h, tau = float(info["h"]), float(info["tau"])
    if abs(offset) > tau - h:
        raise ValueError("offset beyond tau - h")
    mc = M.marching_cubes(level.astype(F32), isovalue=offset)
    v, t = mc.v_pos.astype(np.float64) * ((R - 1) * h) + info["lo"].astype(np.float64), mc.t_pos_idx
    dropped = 0
    if len(t) and not keep_cavities:
        comp = face_components(len(v), t)
        keep = np.ones(len(t), bool)
        for c in np.unique(comp):
            if M.signed_volume(v, t[comp == c]) < 0:
                keep[comp == c] = False
                dropped += 1
        t = t[keep]
        used = np.zeros(len(v), bool)
        used[t.reshape(-1)] = True
        v, t = v[used], (np.cumsum(used) - 1)[t]
    return v.astype(F32), t.astype(np.int32), dict(info, components_dropped=dropped)


# ---------------------------------------------------------------------------------------------------------------
# the conditions on a solidified mesh (numpy arrays in, whoever made them)
def is_closed(t, n_vert):
    return len(t) > 0 and ISO.closed_once(np.asarray(t), n_vert)


def n_components(v, t):
    return len(np.unique(face_components(len(v), np.asarray(t))))


def distance_to_mesh(points, v_pos, t_pos_idx):
    """float64 distance of every point to the mesh."""
    return D.pair_matrix(points, v_pos, t_pos_idx).min(1)[0].sqrt().numpy()


def check_closed_input(name, v, t, src_v, src_t, h):
    comps, chi = GENUS_SUM[name]
    assert is_closed(t, len(v)), name
    assert n_components(v, t) == comps, name
    assert M.euler_characteristic(v, t) == chi, name
    assert M.signed_volume(v, t) > 0, name  # outward
    assert distance_to_mesh(v, src_v, src_t).max() <= h * (1 + 1e-4), name


def signed_distance_to_mesh(points, v_pos, t_pos_idx):
    """float64: negative where the exact winding number is above 1/2."""
    d = distance_to_mesh(points, v_pos, t_pos_idx)
    return np.where(W.exact(points, v_pos, t_pos_idx) > 0.5, -d, d)


def check_overlap(v, t, sd, h):
    """One closed component of genus 0; with sd (n, 2) the signed distance of every vertex to each of the two sphere
    meshes: within h of one sphere and not deeper than h inside the other."""
    assert is_closed(t, len(v)) and n_components(v, t) == 1 and M.euler_characteristic(v, t) == 2
    sd = np.asarray(sd, np.float64)
    assert (np.abs(sd).min(-1) <= h * (1 + 1e-4)).all(), np.abs(sd).min(-1).max() / h
    assert (sd >= -h * (1 + 1e-4)).all(), sd.min() / h
