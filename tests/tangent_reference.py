"""float64 numpy restatement of the contract "tangents and normal-map baking" (include/tt_abi.h): per-face tangents,
their sums per position vertex / per UV vertex, the degenerate rule, the projection step, and the normal-map encode and
its inverse.  Written from the contract; inputs are taken as given (fp32 values widened), every operation is float64."""
import numpy as np

TINY_SQ = 1e-20
PERP_SQ = 1e-12


def atlas(v, tri, N=128, pad=2):
    """(v_tex (Vt,2) float32, t_tex_idx (T,3) int64) of tests/uv_reference.py: labels, charts, boxes, packing, UVs"""
    import uv_reference as U
    tri = np.asarray(tri, np.int64)
    pairs = U.face_pairs(tri)
    lab = U.labels(v, tri, pairs)
    chart = U.charts(tri, pairs, lab)
    box = U.chart_boxes(v, tri, lab, chart)
    off, s = U.pack(box, N, pad)
    return U.emit(np.asarray(v, np.float32), tri, lab, chart, box, off, s, N, pad)


def perp(n):
    """the fixed unit vector perpendicular to unit n (3,): e_a - n_a n normalised, a = the first axis of smallest |n_a|"""
    n = np.asarray(n, np.float64)
    a = int(np.argmin(np.abs(n)))  # argmin takes the first of equal values
    q = -n[a] * n
    q[a] += 1.0
    qq = q @ q
    if not (np.isfinite(qq) and qq > 0.25):
        return np.array([1.0, 0.0, 0.0])
    return q / np.sqrt(qq)


def face_tangents(v_pos, t_pos_idx, v_tex, t_tex_idx):
    v, uv = np.asarray(v_pos, np.float64), np.asarray(v_tex, np.float64)
    tp, tt = np.asarray(t_pos_idx, np.int64), np.asarray(t_tex_idx, np.int64)
    pe1, pe2 = v[tp[:, 1]] - v[tp[:, 0]], v[tp[:, 2]] - v[tp[:, 0]]
    e1, e2 = uv[tt[:, 1]] - uv[tt[:, 0]], uv[tt[:, 2]] - uv[tt[:, 0]]
    denom = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = np.where(denom > 0, np.maximum(denom, 1e-6), np.minimum(denom, -1e-6))
    return (pe1 * e2[:, 1:2] - pe2 * e1[:, 1:2]) / d[:, None], denom


def tangents(v_pos, t_pos_idx, v_tex, t_tex_idx, v_nrm, group="pos", with_stats=False):
    """(G,3) unit tangents, G = V ("pos") or Vt ("tex"); with_stats also {"cond": |sum tang| / sum |tang| per group,
    "perp": |t - (t.n) n| per group, "degenerate": bool per group, "clamped": faces with |denom| < 1e-6}"""
    tp, tt = np.asarray(t_pos_idx, np.int64), np.asarray(t_tex_idx, np.int64)
    nrm = np.asarray(v_nrm, np.float64)
    tang, denom = face_tangents(v_pos, tp, v_tex, tt)
    V, Vt, T = len(nrm), len(v_tex), len(tp)
    key = (tt if group == "tex" else tp).reshape(-1)
    G = Vt if group == "tex" else V
    s = np.zeros((G, 3))
    absum = np.zeros(G)
    first = np.full(G, -1, np.int64)  # the position vertex of a group's smallest corner id
    for c in range(3 * T):  # ascending corner id
        g = key[c]
        s[g] += tang[c // 3]
        absum[g] += np.linalg.norm(tang[c // 3])
        if first[g] < 0:
            first[g] = tp.reshape(-1)[c]
    out = np.zeros((G, 3))
    cond, pr, deg = np.zeros(G), np.zeros(G), np.zeros(G, bool)
    for g in range(G):
        if group == "tex":
            n = nrm[first[g]] if first[g] >= 0 else np.array([0.0, 0.0, 1.0])
        else:
            n = nrm[g]
        ss = s[g] @ s[g]
        r = None
        if first[g] >= 0 and np.isfinite(ss) and ss > TINY_SQ:
            t = s[g] / np.sqrt(ss)
            r = t - (t @ n) * n
            rr = r @ r
            cond[g] = np.sqrt(ss) / absum[g] if absum[g] > 0 else 0.0
            pr[g] = np.sqrt(rr) if np.isfinite(rr) else 0.0
            if not (np.isfinite(rr) and rr > PERP_SQ):
                r = None
        if r is None:
            deg[g] = True
            out[g] = perp(n)
        else:
            out[g] = r / np.sqrt(r @ r)
    if with_stats:
        return out, {"cond": cond, "perp": pr, "degenerate": deg, "clamped": int((np.abs(denom) < 1e-6).sum())}
    return out


def project_step(p, sdf, g, max_step):
    """one bounded Newton step: p - c g, c = clamp(sdf / max(g.g, 1e-12), -1, 1) scaled so that |c g| <= max_step"""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    sdf = np.asarray(sdf, np.float64).reshape(-1)
    gg = (g * g).sum(1)
    a = np.clip(sdf / np.maximum(gg, 1e-12), -1.0, 1.0)
    ln = np.abs(a) * np.sqrt(gg)
    c = np.where(ln > max_step, a * (max_step / np.where(ln > 0, ln, 1.0)), a)
    ok = np.isfinite(np.abs(sdf) + gg)
    return np.where(ok[:, None], p - c[:, None] * g, p)


def _unit(x, fallback):
    xx = (x * x).sum(-1, keepdims=True)
    ok = np.isfinite(xx) & (xx > TINY_SQ)
    return np.where(ok, x / np.sqrt(np.where(ok, xx, 1.0)), fallback)


def frames(rast, v_nrm, t_pos_idx, tng_tex, t_tex_idx):
    """(covered (H,W) bool, t^, b^, n^ (H,W,3)) of the texels of rast (H,W,4) = (u, v, z/w, face + 1)"""
    rast = np.asarray(rast, np.float64)
    tp, tt = np.asarray(t_pos_idx, np.int64), np.asarray(t_tex_idx, np.int64)
    T = len(tp)
    fid = rast[..., 3].astype(np.int64) - 1
    cov = (fid >= 0) & (fid < T)
    f = np.where(cov, fid, 0)
    u, v = rast[..., 0:1], rast[..., 1:2]
    w2 = 1.0 - u - v

    def interp(attr, tri):
        a = np.asarray(attr, np.float64)
        return (u * a[tri[f, 0]] + v * a[tri[f, 1]]) + w2 * a[tri[f, 2]]

    n, t = interp(v_nrm, tp), interp(tng_tex, tt)
    nh = _unit(n, np.array([0.0, 0.0, 1.0]))
    q = t - (t * nh).sum(-1, keepdims=True) * nh
    fb = np.apply_along_axis(perp, -1, nh) if T else np.zeros_like(nh)
    th = _unit(q, fb)
    bh = np.cross(th, nh)
    return cov, th, bh, nh


def encode(rast, v_nrm, t_pos_idx, tng_tex, t_tex_idx, field_nrm):
    """(map (H,W,3), covered (H,W), back-facing (H,W)): 0.5 + 0.5 (m^.t^, m^.b^, m^.n^), (0.5, 0.5, 1) uncovered"""
    cov, th, bh, nh = frames(rast, v_nrm, t_pos_idx, tng_tex, t_tex_idx)
    mh = _unit(np.asarray(field_nrm, np.float64), nh)
    x = np.stack([(mh * th).sum(-1), (mh * bh).sum(-1), (mh * nh).sum(-1)], -1)
    out = np.where(cov[..., None], 0.5 + 0.5 * x, np.array([0.5, 0.5, 1.0]))
    return out, cov, cov & ~(x[..., 2] > 0)


def decode(img, th, bh, nh):
    """the world normal a map value stands for in the frame (t^, b^, n^): the inverse of encode"""
    x = 2.0 * np.asarray(img, np.float64) - 1.0
    n = x[..., 0:1] * th + x[..., 1:2] * bh + x[..., 2:3] * nh
    return n / np.maximum(np.linalg.norm(n, axis=-1, keepdims=True), 1e-300)
