"""Test-only float64 torch restatement of the rasterize / interpolate / antialias contract (include/tt_abi.h,
"rasterize / interpolate / antialias").  Brute force: every triangle against every pixel centre.  The antialias is
built from differentiable torch ops, so autograd supplies the reference gradients; rasterize's (u, v) likewise."""
import torch

F64 = torch.float64


def pixel_ndc(H, W, device="cpu"):
    X = (2 * torch.arange(W, dtype=F64, device=device) + 1) / W - 1
    Y = (2 * torch.arange(H, dtype=F64, device=device) + 1) / H - 1
    return X, Y


def _cross(a, b):
    return torch.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _edges(v, idx):
    """v (Tc,3,3) homogeneous 2-D (x, y, w), idx (Tc,3) vertex indices -> canonical normals n (Tc,3,3) (edge k opposite
    vertex k, lower index first), signs sg (Tc,3) (true-edge sign times sign(D)), sign(D) (Tc,), D (Tc,)"""
    D = (_cross(v[:, 0], v[:, 1]) * v[:, 2]).sum(-1)
    sd = torch.sign(D)
    ns, sgs = [], []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        fwd = idx[:, i] < idx[:, j]
        vi, vj = v[:, i], v[:, j]
        lo = torch.where(fwd[:, None], vi, vj)
        hi = torch.where(fwd[:, None], vj, vi)
        ns.append(_cross(lo, hi))
        sgs.append(torch.where(fwd, sd, -sd))
    return torch.stack(ns, 1), torch.stack(sgs, 1), sd, D


def rasterize(pos, tri, H, W, chunk=512, margin=1e-5):
    """pos (B,V,4), tri (T,3) -> rast (B,H,W,4) float64 (differentiable w.r.t. pos through u, v) and ambiguous
    (B,H,W) bool: pixels whose visibility is within `margin` of changing (a candidate near an edge, the near / far
    plane or a depth tie)."""
    pos = pos.to(F64)
    B, V, _ = pos.shape
    T = tri.shape[0]
    X, Y = pixel_ndc(H, W, pos.device)
    Pxy = torch.stack(torch.meshgrid(Y, X, indexing="ij")[::-1], -1).reshape(-1, 2)  # (HW, 2) = (X, Y)
    npix = H * W
    rasts, ambs = [], []
    tri = tri.long()
    if T == 0:
        return torch.zeros(B, H, W, 4, dtype=F64), torch.zeros(B, H, W, dtype=torch.bool)
    for b in range(B):
        best_z = torch.full((npix,), float("inf"), dtype=F64)
        best_t = torch.full((npix,), -1, dtype=torch.long)
        second_z = torch.full((npix,), float("inf"), dtype=F64)
        near_z = torch.full((npix,), float("inf"), dtype=F64)  # smallest z/w among uncertain candidates
        for c0 in range(0, T, chunk):
            tc = tri[c0:c0 + chunk]
            ok_idx = ((tc >= 0) & (tc < V)).all(1) & (tc[:, 0] != tc[:, 1]) & (tc[:, 1] != tc[:, 2]) & (
                tc[:, 0] != tc[:, 2])
            tcc = tc.clamp(0, max(V - 1, 0))
            pv = pos[b][tcc].detach()  # (Tc,3,4)
            v = pv[..., [0, 1, 3]]
            n, sg, sd, D = _edges(v, tcc)
            c = n[..., 0, None] * Pxy[None, None, :, 0] + n[..., 1, None] * Pxy[None, None, :, 1] + n[..., 2, None]
            te = sg[..., None] * c  # (Tc,3,HW)
            gx, gy = sg * n[..., 0], sg * n[..., 1]
            own = (gx > 0) | ((gx == 0) & (gy > 0))
            inside = ((te > 0) | ((te == 0) & own[..., None])).all(1)
            ssum = te.sum(1)
            den = (te * pv[..., 3, None]).sum(1)
            num = (te * pv[..., 2, None]).sum(1)
            zw = num / den.where(den != 0, torch.ones_like(den))
            valid = ok_idx[:, None] & (D != 0)[:, None] & (ssum > 0) & (den > 0)
            cov = valid & inside & (zw >= -1) & (zw <= 1)
            # uncertain: a barycentric or |z/w| - 1 within margin of the boundary
            bary = te / ssum.where(ssum > 0, torch.ones_like(ssum))[:, None]
            near_edge = bary.min(1).values.abs() < margin
            near_clip = ((zw.abs() - 1).abs() < margin)
            unsure = valid & (bary.min(1).values > -margin) & (zw >= -1 - margin) & (zw <= 1 + margin) & (
                near_edge | near_clip)
            z_c = torch.where(cov, zw, torch.full_like(zw, float("inf")))
            ids = torch.arange(c0, c0 + tc.shape[0])[:, None].expand_as(z_c)
            # chunk min by (z, id): z first, then the smallest id among equal z
            zmin = z_c.min(0).values
            tmin = torch.where(z_c == zmin[None], ids, torch.full_like(ids, T + 1)).min(0).values
            # second smallest z in the chunk (for depth ties)
            z2 = torch.where((z_c == zmin[None]) & (ids == tmin[None]), torch.full_like(z_c, float("inf")), z_c)
            z2 = z2.min(0).values
            better = (zmin < best_z) | ((zmin == best_z) & (tmin < best_t)) & torch.isfinite(zmin)
            second_z = torch.where(better, torch.minimum(best_z, z2), torch.minimum(second_z, zmin))
            best_t = torch.where(better, tmin, best_t)
            best_z = torch.where(better, zmin, best_z)
            near_z = torch.minimum(near_z, torch.where(unsure, zw, torch.full_like(zw, float("inf"))).min(0).values)
        covered = best_t >= 0
        tol = margin * (best_z.abs().where(covered, torch.zeros_like(best_z)) + 1)
        amb = (torch.isfinite(near_z) & (near_z <= torch.where(covered, best_z + tol, torch.full_like(best_z, float("inf"))))) | (
            covered & (second_z - best_z <= tol))
        # differentiable (u, v, z/w) of the winners
        t = best_t.clamp(min=0)
        pv = pos[b][tri[t].clamp(0, max(V - 1, 0))]  # (HW,3,4), with grad
        v = pv[..., [0, 1, 3]]
        p = torch.cat([Pxy, torch.ones(npix, 1, dtype=F64)], -1)
        e = torch.stack([(_cross(v[:, (k + 1) % 3], v[:, (k + 2) % 3]) * p).sum(-1) for k in range(3)], -1)
        s = e.sum(-1, keepdim=True)
        bc = e / s
        zw = (e * pv[..., 2]).sum(-1) / (e * pv[..., 3]).sum(-1)
        r = torch.stack([bc[:, 0], bc[:, 1], zw, (best_t + 1).to(F64)], -1)
        r = torch.where(covered[:, None], r, torch.zeros_like(r))
        rasts.append(r.reshape(H, W, 4))
        ambs.append(amb.reshape(H, W))
    return torch.stack(rasts), torch.stack(ambs)


def interpolate(attr, rast, tri):
    """attr (A,V,C), A = B or 1; rast (B,H,W,4) -> (B,H,W,C); differentiable w.r.t. attr and rast[..., :2]."""
    B, H, W, _ = rast.shape
    ids = rast[..., 3].round().long()
    t = (ids - 1).clamp(min=0)
    idx = tri.long()[t]  # (B,H,W,3)
    a = attr.to(F64).expand(B, -1, -1)
    gat = torch.stack([torch.gather(a, 1, idx[..., k].reshape(B, -1, 1).expand(-1, -1, a.shape[2])) for k in range(3)])
    gat = gat.reshape(3, B, H, W, -1)
    u, v = rast[..., 0:1].to(F64), rast[..., 1:2].to(F64)
    out = u * gat[0] + v * gat[1] + (1 - u - v) * gat[2]
    return torch.where((ids > 0)[..., None], out, torch.zeros_like(out))


def orientation(pos, tri):
    """(B,T) sign of det[[x,y,w]_0..2]"""
    v = pos.detach().to(F64)[:, tri.long()][..., [0, 1, 3]]  # (B,T,3,3)
    return torch.sign((_cross(v[..., 0, :], v[..., 1, :]) * v[..., 2, :]).sum(-1))


def silhouette(pos, tri):
    """(B,T,3) bool: edge k (vertices k, (k+1)%3) of t is a silhouette edge in view b"""
    B = pos.shape[0]
    T = tri.shape[0]
    o = orientation(pos, tri)
    groups = {}
    tl = tri.tolist()
    for t, (a, b_, c) in enumerate(tl):
        for k, (p, q) in enumerate(((a, b_), (b_, c), (c, a))):
            groups.setdefault((min(p, q), max(p, q)), []).append((t, k))
    sil = torch.zeros(B, T, 3, dtype=torch.bool)
    for members in groups.values():
        for t, k in members:
            others = [u for u, _ in members if u != t]
            if not others:
                sil[:, t, k] = True
            else:
                sil[:, t, k] = ((o[:, others] * o[:, t:t + 1]) < 0).any(1)
    return sil


def antialias(color, rast, pos, tri):
    """color (B,H,W,C), rast (B,H,W,4) (visibility input, no gradient), pos (B,V,4) -> (B,H,W,C) float64,
    differentiable w.r.t. color and pos."""
    B, H, W, C = color.shape
    color = color.to(F64)
    pos = pos.to(F64)
    tri = tri.long()
    sil = silhouette(pos, tri)
    ids = rast[..., 3].round().long()
    zw = rast[..., 2].to(F64)
    out = color.reshape(-1, C).clone()
    flat = color.reshape(-1, C)
    bidx = torch.arange(B)[:, None, None]
    for horiz in (True, False):
        if horiz:
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W - 1), indexing="ij")
            fy, fx, sy, sx = yy, xx, yy, xx + 1
        else:
            yy, xx = torch.meshgrid(torch.arange(H - 1), torch.arange(W), indexing="ij")
            fy, fx, sy, sx = yy, xx, yy + 1, xx
        fy, fx, sy, sx = (a[None].expand(B, -1, -1) for a in (fy, fx, sy, sx))
        bb = bidx.expand_as(fy)
        idf, ids_ = ids[bb, fy, fx], ids[bb, sy, sx]
        diff = idf != ids_
        inf = float("inf")
        kf = torch.where(idf > 0, zw[bb, fy, fx], torch.full_like(zw[bb, fy, fx], inf))
        ks = torch.where(ids_ > 0, zw[bb, sy, sx], torch.full_like(kf, inf))
        a_first = (kf < ks) | ((kf == ks) & (idf < ids_) & (idf > 0))
        t = torch.where(a_first, idf, ids_) - 1
        sel = diff & (t >= 0)
        bb, fy, fx, sy, sx, t, a_first = (x[sel] for x in (bb, fy, fx, sy, sx, t, a_first))
        if bb.numel() == 0:
            continue
        al = torch.where(a_first, fx if horiz else fy, sx if horiz else sy).to(F64)
        dirn = torch.where(a_first, 1.0, -1.0).to(F64)
        q0 = (fy if horiz else fx).to(F64)
        best = torch.full(bb.shape, inf, dtype=F64)
        for k in range(3):
            e0 = pos[bb, tri[t, k]]
            e1 = pos[bb, tri[t, (k + 1) % 3]]
            li, pi = (0, 1) if horiz else (1, 0)
            Nl, Np = (W, H) if horiz else (H, W)
            l0 = (e0[:, li] / e0[:, 3] + 1) * Nl / 2 - 0.5
            l1 = (e1[:, li] / e1[:, 3] + 1) * Nl / 2 - 0.5
            p0 = (e0[:, pi] / e0[:, 3] + 1) * Np / 2 - 0.5
            p1 = (e1[:, pi] / e1[:, 3] + 1) * Np / 2 - 0.5
            cross = (p0 > q0) != (p1 > q0)
            dp = torch.where(cross, p1 - p0, torch.ones_like(p1))
            r = (q0 - p0) / dp
            s = (l0 + r * (l1 - l0) - al) * dirn
            ok = cross & (e0[:, 3] > 0) & (e1[:, 3] > 0) & sil[bb, t, k] & (s >= 0) & (s < 1)
            best = torch.where(ok & (s < best), s, best)
        has = torch.isfinite(best)
        s = best[has]
        bb, fy, fx, sy, sx, a_first = (x[has] for x in (bb, fy, fx, sy, sx, a_first))
        pf = (bb * H + fy) * W + fx
        ps = (bb * H + sy) * W + sx
        pa = torch.where(a_first, pf, ps)
        pb = torch.where(a_first, ps, pf)
        lt = s < 0.5
        m = torch.where(lt, pa, pb)
        o = torch.where(lt, pb, pa)
        alpha = torch.where(lt, 0.5 - s, s - 0.5)
        out = out.index_put((m,), alpha[:, None] * (flat[o] - flat[m]), accumulate=True)
    return out.reshape(B, H, W, C)
