"""Float64 torch restatement of the texture-sampling contract (include/tt_abi.h, "texture sampling"), test-only.
Written with differentiable torch ops, so autograd gives the reference gradients w.r.t. tex and uv.

    texture(tex, uv, filter_mode, boundary_mode) -> (B,H,W,C)     tex (N,TH,TW,C), N = B or 1; uv (B,H,W,2)

u runs along the width, v along the height, texel (i, j) has its centre at ((i + 0.5) / TW, (j + 0.5) / TH).  A pixel
with a non-finite uv component gives 0 and no gradient."""
import torch

F64 = torch.float64


def _axis(u, n, linear, boundary):
    """taps (2 index tensors, long, inside [0, n)) and their weights (2 float64 tensors, differentiable in u)"""
    x = u * n - 0.5 if linear else u * n
    x0 = torch.floor(x.detach())
    f = (x - x0) if linear else torch.zeros_like(x)
    taps = [x0, x0 + 1] if linear else [x0]
    weights = [1 - f, f] if linear else [1 + 0 * x]  # nearest: constant in u, so autograd gives grad_uv = 0
    idx, w = [], []
    for t, wt in zip(taps, weights):
        t = t.long()
        if boundary == "wrap":
            i = torch.remainder(t, n)
        elif boundary == "clamp":
            i = t.clamp(0, n - 1)
        elif boundary == "zero":
            inside = (t >= 0) & (t <= n - 1)
            i = t.clamp(0, n - 1)
            wt = wt * inside.to(wt.dtype)
        else:
            raise ValueError(boundary)
        idx.append(i)
        w.append(wt)
    return idx, w


def texture(tex, uv, filter_mode="linear", boundary_mode="wrap"):
    tex, uv = tex.to(F64), uv.to(F64)
    N, TH, TW, C = tex.shape
    B, H, W, _ = uv.shape
    assert N in (1, B)
    linear = {"linear": True, "nearest": False}[filter_mode]
    finite = torch.isfinite(uv).all(-1)
    uv = torch.where(finite[..., None], uv, torch.zeros_like(uv))  # no gradient flows to the replaced pixels
    xi, xw = _axis(uv[..., 0], TW, linear, boundary_mode)
    yi, yw = _axis(uv[..., 1], TH, linear, boundary_mode)
    n = torch.arange(B)[:, None, None].expand(B, H, W) if N == B else torch.zeros(B, H, W, dtype=torch.long)
    out = torch.zeros(B, H, W, C, dtype=F64)
    for j, wy in zip(yi, yw):
        for i, wx in zip(xi, xw):
            out = out + (wy * wx)[..., None] * tex[n, j, i]
    return out * finite[..., None].to(F64)
