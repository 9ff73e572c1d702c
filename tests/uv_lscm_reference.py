"""numpy float64 restatement of the conformal-chart contract (include/tt_abi.h, "conformal UV charts") for small meshes:
the UV vertices of a face -> chart assignment, the per-face frames, the matrix of the energy E assembled per chart and
solved densely with the two pins (np.linalg.lstsq: no iteration, so "converged" always holds here), then normalise,
orient and accept, and the per-face stretch (singular values of the UV Jacobian, area ratios) of any UV map.  Written
from the contract; the GPU solver is compared against `flatten`."""
import numpy as np


def uv_vertices(tri, chart):
    """(t_tex (T,3), vmesh (Vt,), vchart (Vt,)): one UV vertex per distinct (chart, vertex) pair, numbered in order of
    the pair's first corner 3f + k"""
    tri = np.asarray(tri, np.int64)
    ids, vmesh, vchart = {}, [], []
    t_tex = np.zeros(tri.shape, np.int64)
    for q in range(tri.size):
        f, k = divmod(q, 3)
        key = (int(chart[f]), int(tri[f, k]))
        if key not in ids:
            ids[key] = len(vmesh)
            vmesh.append(key[1])
            vchart.append(key[0])
        t_tex[f, k] = ids[key]
    return t_tex, np.array(vmesh, np.int64), np.array(vchart, np.int64)


def frames(v, tri):
    """per face: x1, x2, y2 of p0 = (0,0), p1 = (x1,0), p2 = (x2,y2) in the frame oriented by (p1-p0) x (p2-p0), the
    area A, and W (T,3,2) with grad u = (1 / 2A) sum_k u_k W_k; zeros for a zero-area face"""
    v = np.asarray(v, np.float32).astype(np.float64)
    tri = np.asarray(tri, np.int64)
    p0, p1, p2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    live = nn > 0
    l1 = np.sqrt((e1 * e1).sum(1))
    safe = np.where(live, l1, 1.0)
    x1 = np.where(live, l1, 0.0)
    x2 = np.where(live, (e2 * e1).sum(1) / safe, 0.0)
    y2 = np.where(live, np.sqrt(nn) / safe, 0.0)
    A = np.where(live, 0.5 * np.sqrt(nn), 0.0)
    z = np.zeros_like(x1)
    X = np.stack([z, x1, x2], 1)
    Y = np.stack([z, z, y2], 1)
    W = np.stack([Y[:, [1, 2, 0]] - Y[:, [2, 0, 1]], X[:, [2, 0, 1]] - X[:, [1, 2, 0]]], axis=2)
    return x1, x2, y2, A, W


def _farthest(P, centre):
    d = P - centre
    return int(np.argmax((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))  # first maximum: smallest id


def pins(v32, members, vmesh):
    """(p0, p1, distance) of a chart whose UV vertices are `members` (ascending); distance 0: every vertex coincides"""
    P32 = np.asarray(v32, np.float32)[vmesh[members]]
    P = P32.astype(np.float64)
    centre = 0.5 * (P32.min(0).astype(np.float64) + P32.max(0).astype(np.float64))
    a = _farthest(P, centre)
    b = _farthest(P, P[a])
    return int(members[a]), int(members[b]), float(np.sqrt(((P[b] - P[a]) ** 2).sum()))


def energy_matrix(t_tex_c, A, W, local):
    """M (2F, 2n) of one chart with E = |M x|^2, x = (u_0 .. u_{n-1}, v_0 .. v_{n-1}) over the chart's n UV vertices:
    the rows of face f are (sum_k v_k W_k - J sum_k u_k W_k) / (2 sqrt(A_f)), J = rotation by +90 degrees"""
    F, n = len(t_tex_c), len(local)
    M = np.zeros((2 * F, 2 * n))
    for i in range(F):
        if not A[i] > 0:
            continue
        s = 0.5 / np.sqrt(A[i])
        for k in range(3):
            j = local[int(t_tex_c[i, k])]
            wx, wy = W[i, k]
            M[2 * i, j] += s * wy       # -J (a, b) = (b, -a)
            M[2 * i, n + j] += s * wx
            M[2 * i + 1, j] += -s * wx
            M[2 * i + 1, n + j] += s * wy
    return M


def uv_areas(uv, t_tex):
    P = np.asarray(uv, np.float64)[t_tex]
    return 0.5 * ((P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0]))


def flatten(v, tri, chart, tau=0.3):
    """steps 2-8 of the contract.  Returns a dict: uv (Vt,2) the raw solution, t_tex (T,3), chart_ids (C,) sorted, and
    per chart pins (C,2), fallback (C,) bool, scale, rotation (C,), plus uv_final (Vt,2) = k R(rotation) uv of the
    accepted charts (zeros elsewhere) and energy (C,), E at the solution"""
    v32 = np.asarray(v, np.float32)
    tri = np.asarray(tri, np.int64)
    chart = np.asarray(chart, np.int64)
    tau = float(np.float32(tau))
    t_tex, vmesh, vchart = uv_vertices(tri, chart)
    _, _, _, A, W = frames(v32, tri)
    ids = np.unique(chart)
    C, Vt = len(ids), len(vmesh)
    uv = np.zeros((Vt, 2))
    final = np.zeros((Vt, 2))
    out = {"pins": np.zeros((C, 2), np.int64), "fallback": np.zeros(C, bool), "scale": np.ones(C),
           "rotation": np.zeros(C), "energy": np.zeros(C)}
    for ci, cid in enumerate(ids):
        faces = np.nonzero(chart == cid)[0]
        members = np.nonzero(vchart == cid)[0]
        local = {int(m): j for j, m in enumerate(members)}
        n = len(members)
        a, b, dist = pins(v32, members, vmesh)
        out["pins"][ci] = (a, b)
        if not dist > 0 or a == b:
            out["fallback"][ci] = True
            continue
        M = energy_matrix(t_tex[faces], A[faces], W[faces], local)
        x = np.zeros(2 * n)
        x[local[b]] = dist
        fixed = np.array([local[a], local[b], n + local[a], n + local[b]])
        free = np.setdiff1d(np.arange(2 * n), fixed)
        if len(free):
            x[free] = np.linalg.lstsq(M[:, free], -M[:, fixed] @ x[fixed], rcond=None)[0]
        out["energy"][ci] = float(((M @ x) ** 2).sum())
        uv[members, 0], uv[members, 1] = x[:n], x[n:]
        live = A[faces] > 0
        auv = uv_areas(uv, t_tex[faces])
        s_uv, s_3d = auv[live].sum(), A[faces][live].sum()
        if not (s_uv > 0 and s_3d > 0 and np.isfinite(s_3d / s_uv)):
            out["fallback"][ci] = True
            continue
        k = np.sqrt(s_3d / s_uv)
        d = uv[members] - uv[members].mean(0)
        theta = 0.5 * np.arctan2(2.0 * (d[:, 0] * d[:, 1]).sum(), (d[:, 0] ** 2).sum() - (d[:, 1] ** 2).sum())
        ratio = k * k * auv[live] / A[faces][live]
        if not ((auv[live] > 0).all() and (ratio >= tau).all() and (ratio <= 1.0 / tau).all()):
            out["fallback"][ci] = True
            continue
        c, s = np.cos(theta), np.sin(theta)
        final[members, 0] = k * (c * uv[members, 0] + s * uv[members, 1])
        final[members, 1] = k * (c * uv[members, 1] - s * uv[members, 0])
        out["scale"][ci], out["rotation"][ci] = k, -theta
    out.update(uv=uv, uv_final=final, t_tex=t_tex, chart_ids=ids, vchart=vchart, vmesh=vmesh,
               vchart_dense=np.searchsorted(ids, vchart))  # (the index of a UV vertex's chart into the (C,) arrays)
    return out


def stretch(v, tri, uv, t_tex):
    """per face of a UV map: (sigma1 >= sigma2, the singular values of the Jacobian of (u, v) in the face's isometric
    frame; ratio = UV area / A; A).  NaN on zero-area faces."""
    _, _, _, A, W = frames(v, tri)
    P = np.asarray(uv, np.float64)[np.asarray(t_tex, np.int64)]  # (T,3,2)
    with np.errstate(divide="ignore", invalid="ignore"):
        gu = (P[:, :, 0, None] * W).sum(1) / (2 * A[:, None])
        gv = (P[:, :, 1, None] * W).sum(1) / (2 * A[:, None])
        a, b, c, d = gu[:, 0], gu[:, 1], gv[:, 0], gv[:, 1]
        s = a * a + b * b + c * c + d * d
        det = a * d - b * c
        disc = np.sqrt(np.maximum(s * s - 4 * det * det, 0.0))
        s1, s2 = np.sqrt(0.5 * (s + disc)), np.sqrt(np.maximum(0.5 * (s - disc), 0.0))
        ratio = uv_areas(uv, np.asarray(t_tex, np.int64)) / A
    return s1, s2, ratio, A


def mean_anisotropy(v, tri, uv, t_tex):
    """area-weighted mean of sigma1 / sigma2 over the faces with positive area"""
    s1, s2, _, A = stretch(v, tri, uv, t_tex)
    ok = (A > 0) & (s2 > 0)
    return float((A[ok] * s1[ok] / s2[ok]).sum() / A[ok].sum())


# ---- the developable test shapes -------------------------------------------------------------------------------
def grid_patch(nx, ny, fn=None):
    """(v (nx*ny,3) float32, tri) of a regular nx x ny vertex grid over [0,1]^2, mapped by fn(x, y) -> (X, Y, Z)"""
    xs, ys = np.meshgrid(np.linspace(0, 1, nx), np.linspace(0, 1, ny), indexing="ij")
    x, y = xs.reshape(-1), ys.reshape(-1)
    P = np.stack(fn(x, y) if fn else (x, y, np.zeros_like(x)), 1).astype(np.float32)
    tri = []
    for i in range(nx - 1):
        for j in range(ny - 1):
            a, b, c, d = i * ny + j, (i + 1) * ny + j, (i + 1) * ny + j + 1, i * ny + j + 1
            tri += [(a, b, c), (a, c, d)]
    return P, np.array(tri, np.int64)


def flat_patch():
    """a flat 9 x 9 vertex patch, tilted out of the axis planes"""
    return grid_patch(9, 9, lambda x, y: (x + 0.25 * y, 0.8 * y - 0.1 * x, 0.3 * x + 0.5 * y))


def half_cylinder():
    """a 16 x 8 strip bent over half a cylinder of radius 0.5"""
    return grid_patch(16, 8, lambda x, y: (0.5 * np.cos(np.pi * x), 0.5 * np.sin(np.pi * x), 1.3 * y))


def explicit_cases():
    """name -> (v float32, tri, chart): the explicit charts of the solver test"""
    fv, ft = flat_patch()
    cv, ct = half_cylinder()
    one = (np.array([[0.1, 0.2, 0.3], [0.9, 0.1, 0.5], [0.4, 0.8, -0.2]], np.float32), np.array([[0, 1, 2]]))
    two = (np.array([[0, 0, 0], [1, 0, 0.1], [1.1, 1, 0], [0, 0.9, 0.6]], np.float32), np.array([[0, 1, 2], [0, 2, 3]]))
    half = (np.arange(len(ft)) >= len(ft) // 2).astype(np.int64) * 7 + 3  # ids 3 and 10: the cut shares a row of vertices
    return {"flat_patch": (fv, ft, np.zeros(len(ft), np.int64)), "half_cylinder": (cv, ct, np.zeros(len(ct), np.int64)),
            "one_triangle": (*one, np.zeros(1, np.int64)), "two_triangles": (*two, np.zeros(2, np.int64)),
            "shared_vertices": (fv, ft, half)}


def solver_error(uv, ref):
    """max over the charts of max |uv - uv_ref| / (the chart's UV extent)"""
    worst = 0.0
    for cid in ref["chart_ids"]:
        m = ref["vchart"] == cid
        extent = float((ref["uv"][m].max(0) - ref["uv"][m].min(0)).max())
        worst = max(worst, float(np.abs(uv[m] - ref["uv"][m]).max()) / extent)
    return worst
