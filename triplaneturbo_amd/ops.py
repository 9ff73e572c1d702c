"""Torch-facing wrappers over the C ABI (include/tt_abi.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; all arithmetic of the hot path
happens in libtt_hip.so.  Tensors must be CUDA(=HIP) fp32; there is no CPU fallback (a CPU tensor raises).
"""
from __future__ import annotations

import ctypes
import dataclasses
from dataclasses import dataclass
from functools import cached_property
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

Tensor = torch.Tensor


class KernelTimer:
    """Optional per-launch timing with HIP events on torch's current stream (the stream every kernel of this
    package is launched on).  bench.py uses it to report the dominant kernel's average duration."""

    def __init__(self):
        self.events = []  # (label, start, end)

    def summary(self, median: bool = False):
        """label -> (mean or median duration in ms, number of launches)"""
        torch.cuda.synchronize()
        acc = {}
        for label, a, b in self.events:
            acc.setdefault(label, []).append(a.elapsed_time(b))
        mid = (lambda v: sorted(v)[len(v) // 2]) if median else (lambda v: sum(v) / len(v))
        return {k: (mid(v), len(v)) for k, v in acc.items()}


_TIMER: Optional[KernelTimer] = None


def set_kernel_timer(t: Optional[KernelTimer]) -> None:
    global _TIMER
    _TIMER = t


class _timed:
    def __init__(self, label):
        self.label = label

    def __enter__(self):
        if _TIMER is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if _TIMER is not None:
            self.b.record()
            _TIMER.events.append((self.label, self.a, self.b))
        return False


def _ptr(t: Optional[Tensor]) -> ctypes.c_void_p:
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t.data_ptr())


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _contig(t: Optional[Tensor]) -> Optional[Tensor]:
    return None if t is None else t.contiguous()


def _launch(name: str, *args, label: Optional[str] = None) -> None:
    """One status-returning GPU entry point of the library on torch's current stream: lib.<name>(*args, stream), a
    non-zero status raised as RuntimeError("<name> failed: ...").  A tensor goes in as its data pointer; the argtypes
    load() bound from the header convert the rest (None -> null pointer, a ctypes.Structure -> its address, Python
    numbers) and refuse anything else.  `args` holds every tensor (a `.contiguous()` temporary included) until the call
    has returned.  `label`: the KernelTimer label the launch is timed under, when a timer is installed."""
    fn = getattr(_lib.load(), name)
    ptrs = [a.data_ptr() if isinstance(a, Tensor) else a for a in args]
    if label is None:
        status = fn(*ptrs, _stream())
    else:
        with _timed(label):
            status = fn(*ptrs, _stream())
    _lib.check(status, name)


def _workspace(name: str, *dims: int, device) -> Tensor:
    """The uint8 workspace of the size lib.<name>(*dims) asks for (a tt_*_workspace_bytes query; negative = error)."""
    nbytes = int(getattr(_lib.load(), name)(*dims))
    _lib.check(min(nbytes, 0), name)
    return torch.empty(nbytes, device=device, dtype=torch.uint8)


def _chk_gpu(t: Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (triplaneturbo_amd has no CPU path)")
    if t.device.index != torch.cuda.current_device():
        # the kernels run on the current device's current stream (one process per GPU): a tensor of another GPU
        # would be a wild pointer there
        raise RuntimeError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}; "
                           f"call torch.cuda.set_device (one process per GPU)")


def _chk(t: Tensor, name: str, shape: Optional[Sequence[Optional[int]]] = None, dtype=torch.float32) -> Tensor:
    """`t` as a kernel argument: a `dtype` tensor on the current GPU, made contiguous; `shape` with None for any size."""
    _chk_gpu(t, name)
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if shape is not None and (t.dim() != len(shape) or any(e not in (None, n) for e, n in zip(shape, t.shape))):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {str(tuple(shape)).replace('None', '*')}")
    return t.contiguous()


def _chk_index(t: Tensor, name: str, width: int, rows: Optional[int] = None) -> Tensor:
    """An index table of the mesh stage: (N, width) int32 / int64 on the current GPU, N = `rows` when given.  Its values
    are checked with _minmax (one read-back, the caller's) and _chk_range."""
    _chk_gpu(t, name)
    if t.dtype not in (torch.int32, torch.int64) or t.dim() != 2 or t.shape[1] != width:
        raise TypeError(f"{name} must be (N,{width}) int32 / int64, got {tuple(t.shape)} {t.dtype}")
    if rows is not None and t.shape[0] != rows:
        raise ValueError(f"{name} has {t.shape[0]} rows, expected {rows}")
    return t


def _minmax(*tables: Tensor) -> Tensor:
    """(min, max) of every table, as one tensor on their device: (0, -1), in range for every n, for an empty table."""
    return torch.stack([x for t in tables for x in (t.aminmax() if t.numel() else t.new_tensor([0, -1]).unbind())])


def _chk_range(name: str, lo: int, hi: int, n: int) -> None:
    if lo < 0 or hi >= n:
        raise ValueError(f"{name} holds an index outside [0, {n})")


def _mesh_box(v_pos: Tensor, t_pos_idx: Tensor) -> Tuple[np.ndarray, np.ndarray, np.float32]:
    """The bounding box of a mesh in fp32, (lo (3,), hi (3,), ext = the largest of the three extents hi - lo), from ONE
    read-back that also carries the index range (every value exact in double).  ValueError for an index outside
    [0, V) or a position that is not finite (an extent that overflows fp32 included)."""
    box = torch.cat([v_pos.amin(0).double(), v_pos.amax(0).double(), _minmax(t_pos_idx).double()]).cpu()
    _chk_range("t_pos_idx", int(box[6]), int(box[7]), v_pos.shape[0])
    lo, hi = box[:3].float().numpy(), box[3:6].float().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        ext = (hi - lo).max()  # IEEE fp32, as on the device
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and np.isfinite(ext)):
        raise ValueError("v_pos holds a value that is not finite")
    return lo, hi, ext


def _chk_size(what: str, **counts: int) -> None:
    if max(counts.values()) > _lib.TT_MESH_MAX_ITEMS:
        sizes = ", ".join(f"{k}={v}" for k, v in counts.items())
        raise ValueError(f"{what}: {sizes} (limit TT_MESH_MAX_ITEMS = {_lib.TT_MESH_MAX_ITEMS})")


def _csr(row: Tensor, col: Optional[Tensor], n_rows: int, n_cols: int) -> Tuple[Tensor, Tensor]:
    """The pairs (row[i], col[i]) (int64, any device; row < n_rows, col < n_cols) as a CSR table: ptr (n_rows + 1) int32
    and col int32 sorted by (row, col), from one stable sort of row * n_cols + col.  With n_rows <= TT_MESH_MAX_ITEMS =
    2^28 and n_cols <= 3 * 2^28 (the corners of that many faces) the key stays below 2^58.  col = None is col[i] = i:
    the stable sort of the rows alone is that order already (0.05 ms of 0.25 for mesh_tangents at 28 k faces)."""
    order = torch.sort(row if col is None else torch.add(col, row, alpha=max(n_cols, 1)), stable=True)[1]
    out = (order if col is None else col[order]).int().contiguous()  # (queued before the row count, which syncs)
    ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=row.device)
    ptr[1:] = torch.cumsum(torch.bincount(row, minlength=n_rows), 0)
    return ptr.int().contiguous(), out


def _weights_struct(sdf_w: Sequence[Tensor], net2_w: Optional[Sequence[Tensor]], net2: str = "feat v",
                    net2_in: int = 96):
    """tt_mlp_weights of the sdf net and a second net (net2_in -> 64 -> 64 -> 3) in v1..v3: the feature net, or
    query_field's deformation net ("def d", 32 inputs)."""
    sw = [_chk(sdf_w[0], "sdf w1", (64, 32)), _chk(sdf_w[1], "sdf w2", (64, 64)), _chk(sdf_w[2], "sdf w3", (1, 64))]
    fw: List[Optional[Tensor]] = [None, None, None]
    if net2_w is not None:
        fw = [_chk(net2_w[0], net2 + "1", (64, net2_in)), _chk(net2_w[1], net2 + "2", (64, 64)),
              _chk(net2_w[2], net2 + "3", (3, 64))]
    st = _lib.MlpWeights(*[_ptr(t) for t in sw + fw])
    return st, sw + fw  # keep tensors alive


@dataclass
class RenderConfig:
    """Scalar knobs of GenerativeSpaceSDFVolumeRenderer that reach the kernels (reference renderer :40-71)."""
    radius: float = 1.0
    sdf_bias_radius: float = 0.5
    inv_std: float = 100.0
    cos_anneal_ratio: float = 1.0
    rgb_grad_shrink: float = 1.0
    tile_sb: int = 0  # consecutive samples of a ray per kernel tile (performance knob): 0 = default (2), 8 importance
    grad_copies: int = 1  # privatised copies of the plane-gradient buffer in the backward (performance knob)
    tile_chunk: int = 0  # samples of a ray block per work item (performance knob); 0 = automatic
    # precision of the MLP products (include/tt_abi.h): None / "split3" = fp32-grade three-piece products on the fp16 pipe
    # (default: the reference's precision, networks.py:91-97), "f32" = the fp32-input MFMA (A/B reference), "split2" /
    # "fast" = the two-piece fast mode of rounds 2-4 (~2^-21.5 per product).  exact_f32=True is the old spelling of "f32".
    precision: Optional[str] = None
    exact_f32: bool = False
    # TT_R_VOLSDF: alpha = |dists| x VolSDF density instead of the NeuS alpha (neus_volume_renderer.py:19-23,:95-96)
    use_volsdf: bool = False

    @property
    def prec(self) -> str:
        return _lib.resolve_precision(self.precision, self.exact_f32)
    # OPT-IN approximation of the backward (0 = exact): skip 32-sample tiles whose upstream gradients are all below the
    # threshold (tt_render_cfg.skip_eps_tex / skip_eps_geo in include/tt_abi.h; error measured in tests/test_gpu_skip.py)
    skip_eps_tex: float = 0.0
    skip_eps_geo: float = 0.0
    # trainable variance (reference class default, renderer :53,82): a 0-dim CUDA tensor holding inv_std (e.g.
    # exp(10 p).clamp(1e-6, 1e6)).  The kernels read it from the device (tt_render_cfg.inv_std_dev: no host read-back,
    # legal under stream capture) and, when it requires grad, render_samples returns d loss / d inv_std through autograd.
    # None = the host float `inv_std` above.
    inv_std_t: Optional[Tensor] = None
    # measurement hook (tt_render_cfg.stats): a zero-filled CUDA int64 tensor (3, 4); rows = forward / geometry backward /
    # texture backward decode kernel, columns = tile steps visited, tile steps executed, in-bounds (plane, sample) pairs,
    # reserved.  bench.py reads `live_tile_frac` from it; None = off
    stats: Optional[Tensor] = None
    # the differentiable render's forward also writes the sign mask of the sdf net's last hidden layer and its geometry
    # backward reads it (tt_render_fwd_h2mask / tt_render_bwd_geo_h2mask); False = the backward recomputes the layer for
    # its signs (tt_render_fwd / tt_render_bwd_geo: the A/B reference of the mask path)
    fwd_mask: bool = True
    # with fwd_mask: the forward saves the sign mask of the FIRST hidden layer as well (8 more bytes per sample) and the
    # geometry backward forms v = m1 . (W1 u) from one W1 product (tt_render_fwd_masks / tt_render_bwd_geo_masks); False =
    # the h2-only pair above (the A/B reference of the one-product form).  No effect without fwd_mask.
    fwd_mask_h1: bool = True


def sign_mask_bits(words: Tensor) -> Tensor:
    """(n, 2) int32 sign-mask words of tt_render_fwd_h2mask / tt_render_fwd_masks -> (n, 64) bool.  Element e of the hidden
    vector sits in dword (e >> 2) & 1 at bit (e & 3) + 4 (e >> 3): the kernels' register layout (include/tt_abi.h)."""
    if words.ndim != 2 or words.shape[1] != 2:
        raise ValueError(f"sign-mask words: expected (n, 2), got {tuple(words.shape)}")
    w = words.to(torch.int64) & 0xFFFFFFFF
    e = torch.arange(64, device=words.device)
    return ((w[:, (e >> 2) & 1] >> ((e & 3) + 4 * (e >> 3))[None, :]) & 1).bool()


def sign_mask_words(bits: Tensor) -> Tensor:
    """Inverse of sign_mask_bits: (n, 64) bool -> (n, 2) int32 words."""
    if bits.ndim != 2 or bits.shape[1] != 64:
        raise ValueError(f"sign-mask bits: expected (n, 64), got {tuple(bits.shape)}")
    e = torch.arange(64, device=bits.device)
    contrib = bits.to(torch.int64) << ((e & 3) + 4 * (e >> 3))[None, :]
    w = torch.stack([contrib[:, ((e >> 2) & 1) == d].sum(dim=1) for d in (0, 1)], dim=1)
    return torch.where(w >= 1 << 31, w - (1 << 32), w).to(torch.int32)


def planes_pack(space_cache: Tensor) -> Tensor:
    """(P,6,32,H,W) generator output -> (P,6,H,W,32) channels-last, rotate_planes 'v1' folded in."""
    space_cache = _chk(space_cache, "space_cache", (None, 6, 32, None, None))
    P, _, _, H, W = space_cache.shape
    out = torch.empty((P, 6, H, W, 32), device=space_cache.device, dtype=torch.float32)
    _launch("tt_planes_pack", space_cache, out, P, H, W)
    return out


def planes_unpack_grad(grad_packed: Tensor) -> Tensor:
    """(P,6,H,W,32) or privatised (copies,P,6,H,W,32) packed gradients -> (P,6,32,H,W), copies summed."""
    grad_packed = _chk(grad_packed, "grad_packed")
    copies = grad_packed.shape[0] if grad_packed.ndim == 6 else 1
    P, _, H, W, _ = grad_packed.shape[-5:]
    out = torch.empty((P, 6, 32, H, W), device=grad_packed.device, dtype=torch.float32)
    _launch("tt_planes_unpack_grad", grad_packed, out, P, H, W, copies)
    return out


class _PackPlanesFn(torch.autograd.Function):
    """tt_planes_pack as a differentiable op: its backward is tt_planes_unpack_grad (the exact transpose)."""

    @staticmethod
    def forward(ctx, space_cache):
        return planes_pack(space_cache)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_packed):
        return planes_unpack_grad(grad_packed.contiguous())


def pack_planes(space_cache: Tensor) -> Tensor:
    """Differentiable planes_pack.  A caller that renders the same cache several times (PatchRenderer: global + patch,
    plus the sampler's proposal pass) packs ONCE and hands `packed=` to render_samples / decode_rays: the packed
    gradients of all renders are summed by autograd and unpacked once (the reference re-materialises a rotated copy
    of the whole cache on every geometry call, few_step...:212-239)."""
    return _PackPlanesFn.apply(space_cache)


def query_points(packed: Tensor, sdf_w: Sequence[Tensor], feat_w: Optional[Sequence[Tensor]], points: Tensor,
                 views_per_prompt: int = 1, radius: float = 1.0, sdf_bias_radius: float = 0.5,
                 need_normal: bool = True, need_features: bool = True, exact_f32: bool = False,
                 precision: Optional[str] = None):
    """Per-point decode (no grad). points (B,N,3) -> sdf (B*N,1), sdf_grad (B*N,3)|None, features (B*N,3)|None."""
    packed = _chk(packed, "packed")
    points = _chk(points, "points")
    B, N, _ = points.shape
    P, _, H, W, _ = packed.shape
    wst, keep = _weights_struct(sdf_w, feat_w if need_features else None)
    dev = points.device
    sdf = torch.empty((B * N, 1), device=dev, dtype=torch.float32)
    grad = torch.empty((B * N, 3), device=dev, dtype=torch.float32) if need_normal else None
    feat = torch.empty((B * N, 3), device=dev, dtype=torch.float32) if need_features else None
    flags = (_lib.TT_Q_NORMAL if need_normal else 0) | (_lib.TT_Q_TEX if need_features else 0) | _lib.q_flag(
        _lib.resolve_precision(precision, exact_f32))
    _launch("tt_query_points", packed, wst, points, B, N, P, views_per_prompt, H, W, radius, sdf_bias_radius, flags,
            sdf, grad, feat, label="tt_query_points")
    return sdf, grad, feat


def query_field(packed: Tensor, sdf_w: Sequence[Tensor], deform_w: Sequence[Tensor], points: Tensor,
                views_per_prompt: int = 1, radius: float = 1.0, sdf_bias_radius: float = 0.5, exact_f32: bool = False,
                precision: Optional[str] = None):
    """sdf (B*N,1) and deformation (B*N,3) from the geometry planes (forward_field)."""
    packed = _chk(packed, "packed")
    points = _chk(points, "points")
    B, N, _ = points.shape
    P, _, H, W, _ = packed.shape
    wst, keep = _weights_struct(sdf_w, deform_w, "def d", 32)
    sdf = torch.empty((B * N, 1), device=points.device, dtype=torch.float32)
    deform = torch.empty((B * N, 3), device=points.device, dtype=torch.float32)
    _launch("tt_query_field", packed, wst, points, B, N, P, views_per_prompt, H, W, radius, sdf_bias_radius,
            _lib.q_flag(_lib.resolve_precision(precision, exact_f32)), sdf, deform, label="tt_query_field")
    return sdf, deform


class _QueryPointsFn(torch.autograd.Function):
    """Differentiable per-point decode (geometry.forward in training, few_step...:273-351): forward =
    tt_planes_pack + tt_query_points, backward = tt_points_bwd_geo (sdf and, through the second-order chain,
    sdf_grad) + tt_points_bwd_tex (features) + tt_planes_unpack_grad, and tt_points_bwd_x for the query points.
    Differentiable inputs: space_cache, the six MLP matrices and the points (the reference keeps `points` in the
    graph: the raster renderer decodes positions interpolated from mesh vertices,
    generative_space_mesh_rasterize_renderer.py:307-331)."""

    @staticmethod
    def forward(ctx, space_cache, w1, w2, w3, v1, v2, v3, points, views_per_prompt, radius, sdf_bias_radius,
                need_normal, prec):
        ctx.set_materialize_grads(False)
        packed = planes_pack(space_cache)
        sdf, grad, feat = query_points(packed, (w1, w2, w3), (v1, v2, v3), points, views_per_prompt, radius,
                                       sdf_bias_radius, need_normal=need_normal, need_features=True,
                                       precision=prec)
        ctx.save_for_backward(packed, w1, w2, w3, v1, v2, v3, points)
        ctx.meta = (views_per_prompt, radius, sdf_bias_radius, _lib.q_flag(prec))
        if grad is None:
            grad = sdf.new_zeros((sdf.shape[0], 3))
            ctx.mark_non_differentiable(grad)
        return sdf, grad, feat

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sdf, g_grad, g_feat):
        packed, w1, w2, w3, v1, v2, v3, points = ctx.saved_tensors
        vpp, radius, bias_r, qf = ctx.meta
        B, N, _ = points.shape
        P, _, H, W, _ = packed.shape
        wst, keep = _weights_struct((w1, w2, w3), (v1, v2, v3))
        g_sdf, g_grad, g_feat = _contig(g_sdf), _contig(g_grad), _contig(g_feat)
        gw = [None] * 6
        g_cache = None
        if any(ctx.needs_input_grad[:7]):
            grad_packed = torch.zeros_like(packed)
            gw = [torch.zeros_like(t) for t in (w1, w2, w3, v1, v2, v3)]
            gst = _grads_struct(gw)
            if g_sdf is not None or g_grad is not None:
                ws = torch.empty((B * N, 4), device=packed.device, dtype=torch.float32)
                _launch("tt_points_bwd_geo", packed, wst, points, B, N, P, vpp, H, W, radius, bias_r, qf, g_sdf, g_grad,
                        ws, grad_packed, gst)
            if g_feat is not None:
                _launch("tt_points_bwd_tex", packed, wst, points, B, N, P, vpp, H, W, radius, 3, qf, g_feat,
                        grad_packed, gst)
            g_cache = planes_unpack_grad(grad_packed) if ctx.needs_input_grad[0] else None
        g_points = None
        if ctx.needs_input_grad[7]:
            g_points = torch.empty_like(points)
            _launch("tt_points_bwd_x", packed, wst, points, B, N, P, vpp, H, W, radius, qf, g_sdf, g_grad, g_feat,
                    g_points)
        return (g_cache, *gw, g_points, None, None, None, None, None)


def query_points_grad(space_cache: Tensor, sdf_w: Sequence[Tensor], feat_w: Sequence[Tensor], points: Tensor,
                      views_per_prompt: int = 1, radius: float = 1.0, sdf_bias_radius: float = 0.5,
                      need_normal: bool = True, exact_f32: bool = False, precision: Optional[str] = None):
    """Differentiable per-point decode: sdf (B*N,1), sdf_grad (B*N,3) (zeros, non-differentiable, when
    need_normal is False), features (B*N,3); autograd-connected to space_cache, the six MLP matrices and -- when
    `points` requires grad -- the points.  precision / exact_f32: the mode of the forward and every backward kernel."""
    return _QueryPointsFn.apply(space_cache, sdf_w[0], sdf_w[1], sdf_w[2], feat_w[0], feat_w[1], feat_w[2],
                                _chk(points, "points"), int(views_per_prompt), float(radius), float(sdf_bias_radius),
                                bool(need_normal), _lib.resolve_precision(precision, bool(exact_f32)))


class _QueryFieldFn(torch.autograd.Function):
    """Differentiable implicit-field query (forward_field in training, few_step...:375-394; caller
    generative_space_mesh_rasterize_renderer.py:428-452): forward = tt_query_field, backward = tt_points_bwd_geo for
    the sdf head + tt_points_bwd_tex on the geometry planes for the deformation head (a 32->64->64->3 net on the SUM
    of the three planes is a 96->64->64->3 net with first-layer matrix [U1 U1 U1] on their concatenation)."""

    @staticmethod
    def forward(ctx, space_cache, w1, w2, w3, d1, d2, d3, points, views_per_prompt, radius, sdf_bias_radius,
                prec):
        ctx.set_materialize_grads(False)
        packed = planes_pack(space_cache)
        sdf, deform = query_field(packed, (w1, w2, w3), (d1, d2, d3), points, views_per_prompt, radius,
                                  sdf_bias_radius, precision=prec)
        ctx.save_for_backward(packed, w1, w2, w3, d1, d2, d3, points)
        ctx.meta = (views_per_prompt, radius, sdf_bias_radius, _lib.q_flag(prec))
        return sdf, deform

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sdf, g_def):
        packed, w1, w2, w3, d1, d2, d3, points = ctx.saved_tensors
        vpp, radius, bias_r, qf = ctx.meta
        B, N, _ = points.shape
        P, _, H, W, _ = packed.shape
        d1x3 = d1.repeat(1, 3).contiguous()  # (64, 96) = [U1 U1 U1]
        keep = [w1.contiguous(), w2.contiguous(), w3.contiguous(), d1x3, d2.contiguous(), d3.contiguous()]
        wst = _lib.MlpWeights(*[_ptr(t) for t in keep])  # `keep` holds the contiguous copies until the launches
        grad_packed = torch.zeros_like(packed)
        gw = [torch.zeros_like(t) for t in (w1, w2, w3, d1x3, d2, d3)]
        gst = _grads_struct(gw)
        if g_sdf is not None:
            ws = torch.empty((B * N, 4), device=packed.device, dtype=torch.float32)
            _launch("tt_points_bwd_geo", packed, wst, points, B, N, P, vpp, H, W, radius, bias_r, qf,
                    g_sdf.contiguous(), None, ws, grad_packed, gst)
        if g_def is not None:
            _launch("tt_points_bwd_tex", packed, wst, points, B, N, P, vpp, H, W, radius, 0, qf, g_def.contiguous(),
                    grad_packed, gst)
        gw[3] = gw[3].view(64, 3, 32).sum(dim=1)
        g_cache = planes_unpack_grad(grad_packed) if ctx.needs_input_grad[0] else None
        return (g_cache, *gw, None, None, None, None, None)


def query_field_grad(space_cache: Tensor, sdf_w: Sequence[Tensor], deform_w: Sequence[Tensor], points: Tensor,
                     views_per_prompt: int = 1, radius: float = 1.0, sdf_bias_radius: float = 0.5,
                     exact_f32: bool = False, precision: Optional[str] = None):
    """Differentiable field query: sdf (B*N,1), deformation (B*N,3); autograd-connected to space_cache, the sdf net
    and the deformation net."""
    return _QueryFieldFn.apply(space_cache, sdf_w[0], sdf_w[1], sdf_w[2], deform_w[0], deform_w[1], deform_w[2],
                               _chk(points, "points"), int(views_per_prompt), float(radius), float(sdf_bias_radius),
                               _lib.resolve_precision(precision, bool(exact_f32)))


def _inv_std_args(rc: RenderConfig):
    """(host inv_std clamped like LearnedVariance.forward, renderer :34-35; device pointer of rc.inv_std_t or None).  ONE
    place validates the device scalar -- CUDA, fp32, current device, one element -- for every wrapper that hands it to a
    kernel (a CPU / fp64 / other-GPU tensor would be a wild pointer there)."""
    inv_std = min(max(float(rc.inv_std), 1.0e-6), 1.0e6)
    if rc.inv_std_t is None:
        return inv_std, None
    t = _chk(rc.inv_std_t, "inv_std_t")
    if t.numel() != 1:
        raise ValueError("inv_std_t must hold one float")
    if t.data_ptr() != rc.inv_std_t.data_ptr():
        raise ValueError("inv_std_t must be a contiguous float32 CUDA tensor (the kernels read it in place)")
    return inv_std, t.data_ptr()  # (the tensor is kept alive by `rc`, which the callers hold across the launch)


def _make_cfg(packed: Tensor, n_rays: int, rays_per_view: int, n_samples: int, rc: RenderConfig,
              per_sample: bool, image_w: int = 0, stats_row: int = 0) -> "_lib.RenderCfg":
    P, _, H, W, _ = packed.shape
    n_views = n_rays // rays_per_view
    if n_views * rays_per_view != n_rays or n_views % P != 0:
        raise ValueError(f"n_rays={n_rays} is not views*rays_per_view with views a multiple of P={P}")
    inv_std, inv_std_dev = _inv_std_args(rc)
    stats = None
    if rc.stats is not None:
        if rc.stats.dtype != torch.int64 or not rc.stats.is_cuda or tuple(rc.stats.shape) != (3, 4):
            raise ValueError("stats must be a CUDA int64 tensor of shape (3, 4)")
        stats = rc.stats.data_ptr() + 32 * stats_row
    return _lib.RenderCfg(P, n_views // P, H, W, rays_per_view, n_samples, n_rays, rc.radius, rc.sdf_bias_radius,
                          inv_std, rc.cos_anneal_ratio, rc.rgb_grad_shrink,
                          (_lib.TT_R_PER_SAMPLE if per_sample else 0) | _lib.r_flag(rc.prec) |
                          (_lib.TT_R_VOLSDF if rc.use_volsdf else 0),
                          image_w if (image_w > 0 and rays_per_view % image_w == 0) else 0, int(rc.tile_sb),
                          max(1, int(rc.grad_copies)), max(0, int(rc.tile_chunk)), max(0.0, float(rc.skip_eps_tex)),
                          max(0.0, float(rc.skip_eps_geo)), inv_std_dev, stats)


def _ray_args(packed: Tensor, rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor):
    """The checked planes, rays (n_rays,3) and intervals (n_rays,S) of an entry point that walks rays."""
    packed = _chk(packed, "packed")
    rays_o, rays_d = _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d")
    t_starts, t_ends = _chk(t_starts, "t_starts"), _chk(t_ends, "t_ends")
    n_rays, S = t_starts.shape
    if rays_o.shape != (n_rays, 3) or rays_d.shape != (n_rays, 3) or t_ends.shape != (n_rays, S):
        raise ValueError("ray / interval shapes disagree")
    return packed, rays_o, rays_d, t_starts, t_ends


def _ray_outputs(n_rays: int, device, S: Optional[int] = None) -> dict:
    """Uninitialised per-ray outputs of the march and, given S, its per-sample weights / trans, in the order the
    entry points take them."""
    f32 = dict(device=device, dtype=torch.float32)
    out = {"opacity": torch.empty((n_rays, 1), **f32), "depth": torch.empty((n_rays, 1), **f32),
           "rgb_fg": torch.empty((n_rays, 3), **f32), "z_variance": torch.empty((n_rays, 1), **f32),
           "normal_acc": torch.empty((n_rays, 3), **f32)}
    if S is not None:
        out.update(weights=torch.empty((n_rays * S, 1), **f32), trans=torch.empty((n_rays * S, 1), **f32))
    return out


def render_forward_raw(packed: Tensor, sdf_w: Sequence[Tensor], feat_w: Sequence[Tensor], rays_o: Tensor,
                       rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, rays_per_view: int, rc: RenderConfig,
                       per_sample: bool = True, image_w: int = 0, h2_mask: Union[bool, Tensor] = False,
                       h1_mask: Union[bool, Tensor] = False):
    """One tt_render_fwd call (decode kernel + march kernel).  rays_* (n_rays,3); t_* (n_rays,S); image_w = width
    of each view's ray image (enables 8x4 pixel tiles).  Returns a dict of raw kernel outputs.  h2_mask=True (or the
    int32 buffer to write): the tt_render_fwd_h2mask form, which also returns "h2_mask" (n_rays*S, 2) int32, the saved
    state of tt_render_bwd_geo_h2mask.  h1_mask=True (or the buffer; needs h2_mask): the tt_render_fwd_masks form, which
    returns "h1_mask" in the same shape and layout too, the saved state of tt_render_bwd_geo_masks."""
    if h1_mask is not False and h2_mask is False:
        raise ValueError("h1_mask needs h2_mask (tt_render_fwd_masks writes both)")
    packed, rays_o, rays_d, t_starts, t_ends = _ray_args(packed, rays_o, rays_d, t_starts, t_ends)
    n_rays, S = t_starts.shape
    cfg = _make_cfg(packed, n_rays, rays_per_view, S, rc, per_sample, image_w)
    wst, keep = _weights_struct(sdf_w, feat_w)
    f32 = dict(device=packed.device, dtype=torch.float32)
    out = _ray_outputs(n_rays, packed.device, S)
    # per-sample decode results: outputs in training, inter-kernel workspace always
    out.update(sdf=torch.empty((n_rays * S, 1), **f32), sdf_grad=torch.empty((n_rays * S, 3), **f32),
               features=torch.empty((n_rays * S, 3), **f32))
    if h2_mask is not False:
        if h2_mask is True:
            h2_mask = torch.empty((n_rays * S, 2), device=packed.device, dtype=torch.int32)
        out["h2_mask"] = _chk(h2_mask, "h2_mask", (n_rays * S, 2), torch.int32)
        if out["h2_mask"].data_ptr() != h2_mask.data_ptr():
            raise ValueError("h2_mask must be contiguous (the kernel writes it in place)")
    if h1_mask is not False:
        if h1_mask is True:
            h1_mask = torch.empty((n_rays * S, 2), device=packed.device, dtype=torch.int32)
        out["h1_mask"] = _chk(h1_mask, "h1_mask", (n_rays * S, 2), torch.int32)
        if out["h1_mask"].data_ptr() != h1_mask.data_ptr():
            raise ValueError("h1_mask must be contiguous (the kernel writes it in place)")
        _launch("tt_render_fwd_masks", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg, *out.values(),
                label="tt_render_fwd")
    elif h2_mask is not False:
        _launch("tt_render_fwd_h2mask", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg, *out.values(),
                label="tt_render_fwd")
    else:
        _launch("tt_render_fwd", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg, *out.values(),
                label="tt_render_fwd")
    return out


@torch.no_grad()
def render_eval_raw(packed: Tensor, sdf_w: Sequence[Tensor], feat_w: Sequence[Tensor], rays_o: Tensor, rays_d: Tensor,
                    t_starts: Tensor, t_ends: Tensor, rays_per_view: int, rc: RenderConfig, image_w: int = 0,
                    transmittance_eps: float = 0.0, weight_eps: float = 0.0, stats: Optional[Tensor] = None):
    """tt_render_eval: the per-ray outputs of render_forward_raw (opacity, depth, rgb_fg, z_variance, normal_acc) from
    the fused decode + march kernel, no per-sample tensors, no autograd.  transmittance_eps / weight_eps > 0 switch
    on early termination / texture-decode skipping (error < transmittance_eps + S * weight_eps per ray); `stats` (2 x
    int64 on the device, zero-filled by the caller) receives the number of geometry / texture tile steps decoded."""
    packed, rays_o, rays_d, t_starts, t_ends = _ray_args(packed, rays_o, rays_d, t_starts, t_ends)
    n_rays, S = t_starts.shape
    cfg = _make_cfg(packed, n_rays, rays_per_view, S, rc, False, image_w)
    wst, keep = _weights_struct(sdf_w, feat_w)
    out = _ray_outputs(n_rays, packed.device)
    if stats is not None and (stats.dtype != torch.int64 or stats.numel() < 2 or not stats.is_cuda):
        raise ValueError("stats must be a CUDA int64 tensor with 2 elements")
    _launch("tt_render_eval", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg, float(transmittance_eps),
            float(weight_eps), *out.values(), stats, label="tt_render_eval")
    return out


def _placement(name: str) -> int:
    if name not in _lib.PLACEMENTS:
        raise ValueError(f"placement must be one of {sorted(_lib.PLACEMENTS)}, got {name!r}")
    return _lib.PLACEMENTS[name]


@torch.no_grad()
def sample_uniform(n_rays: int, n_samples: int, near: float, far: float, device, jitter: Optional[Tensor] = None,
                   placement: str = "tt"):
    """tt_sample_uniform: level-0 intervals (n_rays, n_samples); jitter (n_rays, n_samples+1) U[0,1) => stratified;
    placement: "tt" | "center" (enum tt_sample_placement, include/tt_abi.h)."""
    device = torch.device(device)
    place = _placement(placement)
    if device.type != "cuda":
        raise RuntimeError("triplaneturbo_amd samplers run on the GPU only (no CPU fallback)")
    f32 = dict(device=device, dtype=torch.float32)
    ts, te = torch.empty((n_rays, n_samples), **f32), torch.empty((n_rays, n_samples), **f32)
    if jitter is not None:
        jitter = _chk(jitter, "jitter")
        if jitter.shape != (n_rays, n_samples + 1):
            raise ValueError("jitter must be (n_rays, n_samples + 1)")
    with torch.cuda.device(device):  # (the launch takes `device`'s current stream)
        _launch("tt_sample_uniform", n_rays, n_samples, float(near), float(far), jitter, place, ts, te)
    return ts, te


@torch.no_grad()
def sample_importance(t_starts: Tensor, t_ends: Tensor, sdf: Tensor, n_fine: int, inv_std: float,
                      render_step_size: float, u_jitter: Optional[Tensor] = None, placement: str = "tt",
                      inv_std_t: Optional[Tensor] = None, use_volsdf: bool = False):
    """tt_sample_importance: proposal intervals (n_rays, K) + sdf at their mid-points -> (n_rays, K + n_fine + 1)
    intervals (proposal edges merged with n_fine + 1 inverse-CDF edges placed per `placement`).  inv_std_t: a 0-dim
    CUDA tensor that replaces the host float (trainable variance).  use_volsdf: the proposal density is the VolSDF
    density (renderer :286-287) instead of the fixed-step NeuS density (:288-297)."""
    place = _placement(placement) | (_lib.TT_PLACE_VOLSDF if use_volsdf else 0)
    if inv_std_t is not None:
        inv_std_t = _chk(inv_std_t.detach(), "inv_std_t")
    t_starts, t_ends, sdf = _chk(t_starts, "t_starts"), _chk(t_ends, "t_ends"), _chk(sdf, "sdf")
    n_rays, K = t_starts.shape
    if t_ends.shape != (n_rays, K) or sdf.numel() != n_rays * K:
        raise ValueError("proposal intervals / sdf shapes disagree")
    if u_jitter is not None:
        u_jitter = _chk(u_jitter, "u_jitter")
        if u_jitter.shape != (n_rays, n_fine + 1):
            raise ValueError("u_jitter must be (n_rays, n_fine + 1)")
    f32 = dict(device=t_starts.device, dtype=torch.float32)
    M = K + n_fine + 1
    ots, ote = torch.empty((n_rays, M), **f32), torch.empty((n_rays, M), **f32)
    _launch("tt_sample_importance", t_starts, t_ends, sdf, n_rays, K, int(n_fine), float(inv_std), inv_std_t,
            float(render_step_size), u_jitter, place, ots, ote, label="tt_sample_importance")
    return ots, ote


def _march_cfg(rc: RenderConfig, n_rays: int, S: int) -> "_lib.RenderCfg":
    """tt_render_cfg of the march entry points: no planes, one view of n_rays rays."""
    inv_std, inv_std_dev = _inv_std_args(rc)
    return _lib.RenderCfg(n_prompts=1, views_per_prompt=1, plane_h=1, plane_w=1, rays_per_view=n_rays, n_samples=S,
                          n_rays=n_rays, radius=rc.radius, sdf_bias_radius=rc.sdf_bias_radius, inv_std=inv_std,
                          cos_anneal_ratio=rc.cos_anneal_ratio, rgb_grad_shrink=rc.rgb_grad_shrink,
                          flags=_lib.TT_R_VOLSDF if rc.use_volsdf else 0, image_w=0,
                          tile_sb=0, grad_copies=1, tile_chunk=0, inv_std_dev=inv_std_dev)


@torch.no_grad()
def march_forward_raw(rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, sdf: Tensor, sdf_grad: Tensor,
                      features: Tensor, rc: RenderConfig, out: Optional[dict] = None):
    """The ray march alone (tt_march_fwd): NeuS alpha, transmittance, weights and the five accumulations, on
    per-sample sdf (n_rays*S,1), sdf_grad (.,3), features (.,3) already decoded.  No grad (the differentiable path is
    render_samples).  `out` may hold preallocated result tensors (bench: re-time the march on live buffers)."""
    rays_d, t_starts, t_ends = _chk(rays_d, "rays_d"), _chk(t_starts, "t_starts"), _chk(t_ends, "t_ends")
    sdf, sdf_grad, features = _chk(sdf, "sdf"), _chk(sdf_grad, "sdf_grad"), _chk(features, "features")
    n_rays, S = t_starts.shape
    if sdf.numel() != n_rays * S or sdf_grad.numel() != 3 * n_rays * S or features.numel() != 3 * n_rays * S:
        raise ValueError("per-sample tensors do not match (n_rays, S)")
    cfg = _march_cfg(rc, n_rays, S)
    if out is None:
        out = _ray_outputs(n_rays, rays_d.device, S)
    _launch("tt_march_fwd", rays_d, t_starts, t_ends, cfg, sdf, sdf_grad, features, out["opacity"], out["depth"],
            out["rgb_fg"], out["z_variance"], out["normal_acc"], out["weights"], out["trans"], label="tt_march_fwd")
    return out


@torch.no_grad()
def march_backward_raw(rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, fwd: dict, sdf: Tensor, sdf_grad: Tensor,
                       features: Tensor, rc: RenderConfig, g_opacity=None, g_depth=None, g_rgb_fg=None,
                       g_z_variance=None, g_normal_acc=None, g_weights=None, g_sdf=None, g_sdf_grad=None,
                       out: Optional[Tensor] = None, g_inv_std_rays: Optional[Tensor] = None):
    """tt_march_bwd: (n_rays*S, 4) = (d/d sdf, d/d sdf_grad) from upstream gradients of the march outputs; `fwd` is
    the dict march_forward_raw / render_forward_raw returned (opacity, depth, trans).  g_inv_std_rays (n_rays), if
    given, receives d loss / d inv_std per ray."""
    n_rays, S = t_starts.shape
    cfg = _march_cfg(rc, n_rays, S)
    if out is None:
        out = torch.empty((n_rays * S, 4), device=rays_d.device, dtype=torch.float32)
    gs = [_contig(t)
          for t in (g_opacity, g_depth, g_rgb_fg, g_z_variance, g_normal_acc, g_weights, g_sdf, g_sdf_grad)]
    _launch("tt_march_bwd", rays_d, t_starts, t_ends, cfg, fwd["opacity"], fwd["depth"], fwd["trans"], sdf, sdf_grad,
            features, *gs, g_inv_std_rays, out, label="tt_march_bwd")
    return out


def _zeros_like_flat(tensors: Sequence[Tensor]) -> List[Tensor]:
    """zeros_like for a list of tensors as views of one buffer (one fill kernel instead of one per tensor)"""
    sizes = [t.numel() for t in tensors]
    flat = torch.zeros(sum(sizes), device=tensors[0].device, dtype=tensors[0].dtype)
    out, ofs = [], 0
    for t, n in zip(tensors, sizes):
        out.append(flat[ofs:ofs + n].view_as(t))
        ofs += n
    return out


def _grads_struct(tensors: Sequence[Tensor]):
    return _lib.MlpWeights(*[_ptr(t) for t in tensors])  # same layout as tt_mlp_grads (6 pointers)


def _both_masks(rc: RenderConfig) -> bool:
    """The differentiable render saves the h1 sign mask next to the h2 one: the fp32-MFMA kernel has no use for it (its
    geometry backward stays on the h2-only path), so that mode does not pay for the word."""
    return bool(rc.fwd_mask and rc.fwd_mask_h1 and rc.prec != "f32")


class _TriplaneRenderFn(torch.autograd.Function):
    """Differentiable fused render on packed planes.  forward = tt_render_fwd; backward = tt_render_bwd_geo +
    tt_render_bwd_tex.  Differentiable inputs: the packed planes (see pack_planes) and the six MLP weights (sample
    positions are constants: the reference's sampler runs under no_grad, estimators.py:22)."""

    @staticmethod
    def forward(ctx, packed, w1, w2, w3, v1, v2, v3, rays_o, rays_d, t_starts, t_ends, rays_per_view, rc,
                image_w, inv_std_t=None):
        # inv_std_t: rc.inv_std_t again, as an autograd INPUT (trainable variance: its gradient is returned below)
        need_grad = any(ctx.needs_input_grad[:7]) or ctx.needs_input_grad[14]
        if inv_std_t is not None:  # keep a graph-free alias on ctx (same storage), not the autograd input itself
            rc = dataclasses.replace(rc, inv_std_t=inv_std_t.detach())
        ctx.set_materialize_grads(False)  # unused outputs (e.g. `features`, `weights`) reach backward as None, not as
        #                                    100 MB of zeros the kernels would have to read
        raw = render_forward_raw(packed, (w1, w2, w3), (v1, v2, v3), rays_o, rays_d, t_starts, t_ends, rays_per_view,
                                 rc, per_sample=True, image_w=image_w, h2_mask=need_grad and rc.fwd_mask,
                                 h1_mask=need_grad and _both_masks(rc))
        ctx.rays_per_view = rays_per_view
        ctx.rc = rc
        ctx.image_w = image_w
        ctx.inv_std_shape = None if inv_std_t is None else tuple(inv_std_t.shape)
        if need_grad:
            ctx.save_for_backward(packed, w1, w2, w3, v1, v2, v3, rays_o, rays_d, t_starts, t_ends, raw["opacity"],
                                  raw["depth"], raw["trans"], raw["weights"], raw["features"], raw["sdf"],
                                  raw["sdf_grad"], *([raw["h2_mask"]] if rc.fwd_mask else []),
                                  *([raw["h1_mask"]] if _both_masks(rc) else []))
        ctx.mark_non_differentiable(raw["trans"])
        return (raw["opacity"], raw["depth"], raw["rgb_fg"], raw["z_variance"], raw["normal_acc"], raw["weights"],
                raw["sdf"], raw["sdf_grad"], raw["features"], raw["trans"])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_op, g_depth, g_rgb, g_zvar, g_nacc, g_weights, g_sdf, g_sdf_grad, g_features, _g_trans):
        (packed, w1, w2, w3, v1, v2, v3, rays_o, rays_d, t_starts, t_ends, opacity, depth, trans, weights,
         features, sdf, sdf_grad) = ctx.saved_tensors[:18]
        masks = ctx.saved_tensors[18:]  # the forward's h2 sign mask [and h1 sign mask], or nothing: rc.fwd_mask[_h1]
        n_rays, S = t_starts.shape
        cfg = _make_cfg(packed, n_rays, ctx.rays_per_view, S, ctx.rc, True, ctx.image_w, stats_row=1)
        cfg_tex = _make_cfg(packed, n_rays, ctx.rays_per_view, S, ctx.rc, True, ctx.image_w, stats_row=2)
        workspace = torch.empty((n_rays * S, 4), device=packed.device, dtype=torch.float32)
        wst, keep = _weights_struct((w1, w2, w3), (v1, v2, v3))
        copies = max(1, int(ctx.rc.grad_copies))
        grad_packed = torch.zeros((copies,) + tuple(packed.shape), device=packed.device, dtype=torch.float32)
        gw = _zeros_like_flat((w1, w2, w3, v1, v2, v3))  # six views of ONE zero-filled buffer: one fill launch
        gst = _grads_struct(gw)

        g_op, g_depth, g_rgb, g_zvar, g_nacc, g_weights, g_sdf, g_sdf_grad, g_features = (
            _contig(t) for t in (g_op, g_depth, g_rgb, g_zvar, g_nacc, g_weights, g_sdf, g_sdf_grad, g_features))
        g_k_rays = None
        if ctx.needs_input_grad[14]:  # d loss / d inv_std, one partial per ray (summed below in a fixed order)
            g_k_rays = torch.empty((n_rays,), device=packed.device, dtype=torch.float32)
        _launch(("tt_render_bwd_geo", "tt_render_bwd_geo_h2mask", "tt_render_bwd_geo_masks")[len(masks)], packed, wst, rays_o, rays_d, t_starts,
                t_ends, cfg, opacity, depth, trans, sdf, sdf_grad, features, g_op, g_depth, g_rgb, g_zvar, g_nacc,
                g_weights, g_sdf, g_sdf_grad, g_k_rays, workspace, grad_packed, gst, *masks, label="tt_render_bwd_geo")
        _launch("tt_render_bwd_tex", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg_tex, weights, features, g_rgb,
                g_features, grad_packed, gst, label="tt_render_bwd_tex")
        g_packed = None
        if ctx.needs_input_grad[0]:
            g_packed = grad_packed[0] if copies == 1 else grad_packed.sum(dim=0)
        g_inv_std = None
        if g_k_rays is not None:
            g_inv_std = g_k_rays.double().sum().float().reshape(ctx.inv_std_shape)
        return (g_packed, *gw, None, None, None, None, None, None, None, g_inv_std)


def render_samples(space_cache: Optional[Tensor], sdf_w: Sequence[Tensor], feat_w: Sequence[Tensor], rays_o: Tensor,
                   rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, rays_per_view: int, rc: RenderConfig,
                   image_w: int = 0, packed: Optional[Tensor] = None):
    """Differentiable render for explicit sample intervals.  Returns a dict of per-ray accumulators and
    per-sample tensors (autograd-connected to space_cache and the MLP weights).  `packed` = pack_planes(space_cache)
    made by the caller (then space_cache is not looked at)."""
    names = ("opacity", "depth", "rgb_fg", "z_variance", "normal_acc", "weights", "sdf", "sdf_grad", "features",
             "trans")
    if packed is None:
        packed = pack_planes(space_cache)
    outs = _TriplaneRenderFn.apply(packed, sdf_w[0], sdf_w[1], sdf_w[2], feat_w[0], feat_w[1], feat_w[2],
                                   rays_o.contiguous(), rays_d.contiguous(), t_starts.contiguous(),
                                   t_ends.contiguous(), rays_per_view, rc, int(image_w), rc.inv_std_t)
    return dict(zip(names, outs))


@torch.no_grad()
def decode_rays(packed: Tensor, sdf_w: Sequence[Tensor], feat_w: Optional[Sequence[Tensor]], rays_o: Tensor,
                rays_d: Tensor, t_starts: Tensor, t_ends: Tensor, rays_per_view: int, rc: RenderConfig,
                need_normal: bool = False, need_features: bool = False, image_w: int = 0):
    """Per-sample decode along rays without the march (no grad): sdf (n_rays,S), optionally sdf_grad (n_rays,S,3)
    and features (n_rays,S,3).  The sampler's proposal pass uses the sdf-only form."""
    packed, rays_o, rays_d, t_starts, t_ends = _ray_args(packed, rays_o, rays_d, t_starts, t_ends)
    n_rays, S = t_starts.shape
    cfg = _make_cfg(packed, n_rays, rays_per_view, S, rc, False, image_w)
    wst, keep = _weights_struct(sdf_w, feat_w if need_features else None)
    f32 = dict(device=packed.device, dtype=torch.float32)
    sdf = torch.empty((n_rays, S), **f32)
    grad = torch.empty((n_rays, S, 3), **f32) if need_normal else None
    feat = torch.empty((n_rays, S, 3), **f32) if need_features else None
    flags = (_lib.TT_Q_NORMAL if need_normal else 0) | (_lib.TT_Q_TEX if need_features else 0)
    _launch("tt_decode_rays", packed, wst, rays_o, rays_d, t_starts, t_ends, cfg, flags, sdf, grad, feat,
            label="tt_decode_rays")
    return sdf, grad, feat


class _PatchCompositeFn(torch.autograd.Function):
    """tt_patch_composite_fwd / _bwd: bilinear upsample of the low-resolution global render + paste of the patch
    (patch_renderer.py:74-88) as one kernel each way."""

    @staticmethod
    def forward(ctx, low, patch, py, px, H, W, detach_low):
        low, patch = _chk(low, "low"), _chk(patch, "patch")
        B, h, w, C = low.shape
        PS = patch.shape[1]
        if patch.shape != (B, PS, PS, C):
            raise ValueError(f"patch {tuple(patch.shape)} does not match low {tuple(low.shape)}")
        out = torch.empty((B, H, W, C), device=low.device, dtype=torch.float32)
        _launch("tt_patch_composite_fwd", low, patch, out, B, h, w, H, W, C, PS, py, px)
        ctx.meta = (B, h, w, H, W, C, PS, py, px, detach_low)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        B, h, w, H, W, C, PS, py, px, detach_low = ctx.meta
        want_low = ctx.needs_input_grad[0] and not detach_low
        g_low = torch.empty((B, h, w, C), device=g_out.device, dtype=torch.float32) if want_low else None
        g_patch = torch.empty((B, PS, PS, C), device=g_out.device, dtype=torch.float32)
        _launch("tt_patch_composite_bwd", g_out.contiguous(), g_low, g_patch, B, h, w, H, W, C, PS, py, px)
        return g_low, (g_patch if ctx.needs_input_grad[1] else None), None, None, None, None, None


def patch_composite(low: Tensor, patch: Tensor, py: int, px: int, H: int, W: int, detach_low: bool = False) -> Tensor:
    """(B,h,w,C) low-resolution image upsampled bilinearly (align_corners=False) to (B,H,W,C) with `patch`
    (B,PS,PS,C) pasted at rows py.., columns px..; differentiable w.r.t. both (low: unless detach_low)."""
    return _PatchCompositeFn.apply(low, patch, int(py), int(px), int(H), int(W), bool(detach_low))


_COMPOSITE_MODES = {"world": 0, "camera": 1, "front": 2}


class _CompositeFn(torch.autograd.Function):
    """tt_composite_fwd / _bwd: the renderer's per-ray composite (renderer :433-530) as one kernel each way.
    Differentiable inputs: opacity, depth, rgb_fg, normal_acc and the background colour (a learned background,
    background.py); the cameras are constants."""

    @staticmethod
    def forward(ctx, opacity, depth, rgb_fg, normal_acc, bg, cam_dist, c2w, rays_per_view, mode, view_group):
        opacity, depth = _chk(opacity, "opacity"), _chk(depth, "depth")
        rgb_fg, normal_acc = _chk(rgb_fg, "rgb_fg"), _chk(normal_acc, "normal_acc")
        bg, cam_dist = _chk(bg, "bg_color"), _chk(cam_dist, "camera_distances")
        n = opacity.numel()
        if rays_per_view <= 0 or n % rays_per_view != 0:
            raise ValueError(f"n_rays={n} is not a multiple of rays_per_view={rays_per_view}")
        views = n // rays_per_view
        if cam_dist.numel() != views:  # (composite() already expanded a 1-element tensor)
            raise ValueError(f"camera_distances has {cam_dist.numel()} elements, expected one per view ({views})")
        if c2w is None:
            if mode != 0:
                raise ValueError("c2w is required for normal_direction 'camera' / 'front' (renderer :478-530)")
        else:
            c2w = _chk(c2w, "c2w", (views, 4, 4))
        if view_group <= 0 or views % view_group != 0:
            raise ValueError(f"view_group={view_group} does not divide the number of views ({views})")
        bg_stride = 0 if bg.numel() == 3 else 3
        if bg_stride and bg.numel() != 3 * n:
            raise ValueError("bg_color must have 3 or 3 * n_rays elements")
        f32 = dict(device=opacity.device, dtype=torch.float32)
        comp_rgb, comp_normal = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
        disparity = torch.empty((n, 1), **f32)
        vis = torch.empty((n, 3), **f32) if mode == 1 else None
        vis_white = torch.empty((n, 3), **f32) if mode != 0 else None
        _launch("tt_composite_fwd", opacity, depth, rgb_fg, normal_acc, bg, bg_stride, cam_dist, c2w, n, rays_per_view,
                mode, view_group, comp_rgb, disparity, comp_normal, vis, vis_white)
        ctx.save_for_backward(opacity, depth, rgb_fg, normal_acc, bg, cam_dist, *(() if c2w is None else (c2w,)))
        ctx.meta = (n, bg_stride, rays_per_view, mode, view_group)
        ctx.set_materialize_grads(False)
        dummy = comp_rgb.new_zeros(0)
        outs = (comp_rgb, disparity, comp_normal, vis if vis is not None else dummy,
                vis_white if vis_white is not None else dummy)
        return outs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_disp, g_cn, g_vis, g_visw):
        opacity, depth, rgb_fg, normal_acc, bg, cam_dist, *rest = ctx.saved_tensors
        c2w = rest[0] if rest else None
        n, bg_stride, rays_per_view, mode, view_group = ctx.meta
        g_rgb, g_disp, g_cn, g_vis, g_visw = (  # an empty gradient counts as an absent one
            _contig(t) if t is not None and t.numel() else None for t in (g_rgb, g_disp, g_cn, g_vis, g_visw))
        f32 = dict(device=opacity.device, dtype=torch.float32)
        g_op, g_dep = torch.empty((n, 1), **f32), torch.empty((n, 1), **f32)
        g_fg, g_na = torch.empty((n, 3), **f32), torch.empty((n, 3), **f32)
        g_bg = torch.empty((n, 3), **f32) if ctx.needs_input_grad[4] else None
        _launch("tt_composite_bwd", opacity, depth, rgb_fg, normal_acc, bg, bg_stride, cam_dist, c2w, n, rays_per_view,
                mode, view_group, g_rgb, g_disp, g_cn, g_vis, g_visw, g_op, g_dep, g_fg, g_na, g_bg)
        if g_bg is not None:
            g_bg = g_bg.sum(dim=0).view_as(bg) if bg_stride == 0 else g_bg.view_as(bg)
        return g_op, g_dep, g_fg, g_na, g_bg, None, None, None, None, None


def composite(opacity: Tensor, depth: Tensor, rgb_fg: Tensor, normal_acc: Tensor, bg_color: Tensor,
              camera_distances: Tensor, c2w: Optional[Tensor], rays_per_view: int, normal_direction: str = "camera",
              view_group: int = 1):
    """Per-ray composite of the renderer (renderer :433-530): returns comp_rgb (n,3), disparity (n,1), comp_normal
    (n,3), comp_normal_cam_vis (n,3) | None, comp_normal_cam_vis_white (n,3) | None.
    camera_distances: one per view, or a single element that is broadcast (as it broadcasts in the reference's
    `camera_distances.reshape(-1,1,1,1)` arithmetic); c2w (views,4,4), may be None for normal_direction 'world'."""
    mode = _COMPOSITE_MODES[normal_direction]
    views = opacity.numel() // max(int(rays_per_view), 1)
    camera_distances = camera_distances.reshape(-1).float()
    if camera_distances.numel() == 1 and views > 1:
        camera_distances = camera_distances.expand(views)
    camera_distances = camera_distances.contiguous()
    if c2w is not None:
        c2w = c2w.float().contiguous()
    rgb, disp, cn, vis, visw = _CompositeFn.apply(opacity, depth, rgb_fg, normal_acc, bg_color, camera_distances, c2w,
                                                  int(rays_per_view), mode, int(view_group))
    return rgb, disp, cn, (vis if mode == 1 else None), (visw if mode != 0 else None)


class _EikonalFn(torch.autograd.Function):
    """tt_eikonal_fwd / _bwd: mean((||sdf_grad|| - 1)^2) in one pass each way."""

    @staticmethod
    def forward(ctx, sdf_grad):
        g = _chk(sdf_grad, "sdf_grad", (None, 3))
        loss = torch.empty((), device=g.device, dtype=torch.float32)
        _launch("tt_eikonal_fwd", g, g.shape[0], loss)
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        g, = ctx.saved_tensors
        out = torch.empty_like(g)
        _launch("tt_eikonal_bwd", g, g_loss.contiguous().float(), g.shape[0], out)
        return out


def eikonal_loss(sdf_grad: Tensor) -> Tensor:
    """mean((||sdf_grad||_2 - 1)^2) over the samples (the training loop's eikonal regulariser,
    multiprompt_dual_renderer_multistep_generator.py:696-699) as one HIP kernel each way; sdf_grad (n,3) is the
    renderer's `out["sdf_grad"]`.  Equal to `((torch.linalg.norm(g, ord=2, dim=-1) - 1.0) ** 2).mean()`."""
    return _EikonalFn.apply(sdf_grad)


class _MarchingCubesFn(torch.autograd.Function):
    """Marching cubes with a backward pass (tt_mc_*, include/tt_abi.h "marching cubes"): the `diso.DiffMC` call of
    DiffMarchingCubeHelper.forward (mesh_exporter.py:65-75).  Forward = count, one 8-byte read-back, allocate, emit;
    the workspace (crossing masks + vertex offsets) stays in ctx for the backward gather tt_mc_bwd."""

    @staticmethod
    def forward(ctx, level, deformation, isovalue):
        R = level.shape[0]
        ws = _workspace("tt_mc_workspace_bytes", R, device=level.device)
        totals = torch.empty(2, device=level.device, dtype=torch.int32)
        _launch("tt_mc_count", level, R, isovalue, ws, totals)
        n_vert, n_tri = (int(x) for x in totals.cpu())
        v_pos = torch.empty((n_vert, 3), device=level.device, dtype=torch.float32)
        t_pos_idx = torch.empty((n_tri, 3), device=level.device, dtype=torch.int32)
        if n_vert > 0:
            _launch("tt_mc_emit", level, deformation, R, isovalue, ws, v_pos, t_pos_idx)
        ctx.save_for_backward(level, deformation, ws)
        ctx.isovalue = isovalue
        ctx.mark_non_differentiable(t_pos_idx)
        return v_pos, t_pos_idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_v, g_t):
        level, deformation, ws = ctx.saved_tensors
        if g_v is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        R = level.shape[0]
        g_level = torch.empty_like(level)
        g_def = torch.empty_like(deformation) if deformation is not None else None
        if g_v.shape[0] == 0:
            g_level.zero_()
            if g_def is not None:
                g_def.zero_()
        else:
            _launch("tt_mc_bwd", level, deformation, R, ctx.isovalue, ws, g_v.contiguous(), g_level, g_def)
        return (g_level if ctx.needs_input_grad[0] else None,
                g_def if ctx.needs_input_grad[1] else None, None)


def marching_cubes(level: Tensor, deformation: Optional[Tensor] = None, isovalue: float = 0.0) -> Tuple[Tensor, Tensor]:
    """Isosurface of `level` (R,R,R) at `isovalue`, optionally on a grid deformed by `deformation` (R,R,R,3, grid-cell
    units): v_pos (V,3) fp32 in [0,1]^3 (plus deformation / (R-1)), t_pos_idx (T,3) int32.  Differentiable w.r.t.
    level and deformation (through v_pos).  Contract: include/tt_abi.h, "marching cubes"."""
    if level.dim() != 3 or not (level.shape[0] == level.shape[1] == level.shape[2]):
        raise ValueError(f"level must be (R,R,R), got {tuple(level.shape)}")
    R = level.shape[0]
    level = _chk(level, "level")
    if deformation is not None:
        deformation = _chk(deformation, "deformation", (R, R, R, 3))
    return _MarchingCubesFn.apply(level, deformation, float(isovalue))


_TET_BASE_EDGES = (0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3)  # isosurface.py:175: the six edges of a tet, as corner pairs


class TetGrid:
    """The static tables of a tetrahedral grid for ops.marching_tets (include/tt_abi.h "marching tetrahedra"), built
    once with one torch.unique and one stable sort on the grid's device (plumbing; it syncs):
      vertices    (Nv,3) fp32, tets (Nt,4) int32: the grid as given
      edges       (Ne,2) int32: the unique vertex pairs (a < b) of the six base edges of every tet, lexicographic: the
                  reference helper's all_edges (threestudio/models/isosurface.py:206-219)
      tet_edge    (Nt,6) int32: the row of `edges` of each base edge of each tet
      vert_ptr    (Nv+1) int32, vert_col (2 Ne) int32: vertex -> incident rows of `edges`, each row ascending
    The constructor validates what the kernels trust: indices inside [0, Nv), counts within TT_MESH_MAX_ITEMS."""

    def __init__(self, vertices: Tensor, indices: Tensor):
        self.vertices = _chk(vertices, "vertices", (None, 3))
        indices = _chk_index(indices, "indices", 4)
        Nv, Nt = int(vertices.shape[0]), int(indices.shape[0])
        if Nv < 1 or Nt < 1:
            raise ValueError(f"a tet grid needs a vertex and a tet: Nv={Nv}, Nt={Nt}")
        _chk_size("tet grid too large for tt_mt_*", Nv=Nv, Nt=Nt)
        _chk_range("indices", *_minmax(indices).tolist(), Nv)  # one read-back
        self.n_vertices, self.n_tets = Nv, Nt
        self.tets = indices.int().contiguous()
        pairs = indices.long()[:, list(_TET_BASE_EDGES)].reshape(-1, 2)
        key = torch.add(pairs.amax(1), pairs.amin(1), alpha=Nv)
        uniq, inverse = torch.unique(key, return_inverse=True)  # sorted: lexicographic in (a, b)
        self.edges = torch.stack([uniq // Nv, uniq % Nv], dim=1).int().contiguous()
        self.tet_edge = inverse.reshape(Nt, 6).int().contiguous()
        Ne = self.n_edges = int(uniq.shape[0])
        _chk_size("tet grid too large for tt_mt_*", Ne=Ne)
        ends = self.edges.long().t().reshape(-1)  # the a ends, then the b ends
        self.vert_ptr, self.vert_col = _csr(ends, torch.arange(Ne, device=ends.device).repeat(2), Nv, Ne)


class _MarchingTetsFn(torch.autograd.Function):
    """Marching tetrahedra with a backward pass (tt_mt_*, include/tt_abi.h "marching tetrahedra"):
    MarchingTetrahedraHelper._forward (threestudio/models/isosurface.py:231-301).  Forward = count, one 12-byte
    read-back, allocate, emit; the workspace (crossing flags + vertex offsets) stays in ctx for the gather tt_mt_bwd."""

    @staticmethod
    def forward(ctx, pos, level, grid):
        dev = level.device
        ws = _workspace("tt_mt_workspace_bytes", grid.n_edges, grid.n_tets, device=dev)
        totals = torch.empty(3, device=dev, dtype=torch.int32)
        _launch("tt_mt_count", level, grid.edges, grid.tets, grid.n_edges, grid.n_tets, ws, totals)
        n_vert, n_one, n_two = (int(x) for x in totals.cpu())
        v_pos = torch.empty((n_vert, 3), device=dev, dtype=torch.float32)
        t_pos_idx = torch.empty((n_one + 2 * n_two, 3), device=dev, dtype=torch.int32)
        if n_vert > 0:
            _launch("tt_mt_emit", pos, level, grid.edges, grid.tet_edge, grid.n_edges, grid.n_tets, ws, v_pos,
                    t_pos_idx)
        ctx.save_for_backward(pos, level, ws)
        ctx.grid = grid
        ctx.mark_non_differentiable(t_pos_idx)
        return v_pos, t_pos_idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_v, g_t):
        pos, level, ws = ctx.saved_tensors
        grid = ctx.grid
        if g_v is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        g_level, g_pos = torch.empty_like(level), torch.empty_like(pos)
        if g_v.shape[0] == 0:
            g_level.zero_()
            g_pos.zero_()
        else:
            _launch("tt_mt_bwd", pos, level, grid.edges, grid.vert_ptr, grid.vert_col, grid.n_vertices, grid.n_edges,
                    grid.n_tets, ws, g_v.contiguous(), g_level, g_pos)
        return (g_pos if ctx.needs_input_grad[0] else None, g_level if ctx.needs_input_grad[1] else None, None)


def marching_tets(pos: Tensor, level: Tensor, grid: TetGrid) -> Tuple[Tensor, Tensor]:
    """The surface level = 0 of a field on a tet grid: `pos` (Nv,3) the (deformed) grid vertices, `level` (Nv) or
    (Nv,1), `grid` the TetGrid of the topology.  Returns v_pos (V,3) fp32 and t_pos_idx (T,3) int32, vertices and faces
    in the reference helper's order; differentiable w.r.t. level and pos (through v_pos).  Contract: include/tt_abi.h,
    "marching tetrahedra"."""
    if not isinstance(grid, TetGrid):
        raise TypeError("grid must be an ops.TetGrid")
    Nv = grid.n_vertices
    if not isinstance(level, torch.Tensor) or level.numel() != Nv:
        raise ValueError(f"level must hold one value per grid vertex ({Nv})")
    pos = _chk(pos, "pos", (Nv, 3))
    level = _chk(level.reshape(Nv), "level")
    if pos.device != grid.tets.device:
        raise RuntimeError(f"pos lives on {pos.device}, the tet grid on {grid.tets.device}")
    return _MarchingTetsFn.apply(pos, level, grid)


class FaceEdgeSort(NamedTuple):
    """sort_face_edges' result, all int64: sorted position p holds face edge perm[p] = 3f + k (vertices k, (k+1) % 3
    of face f) and lies in group inverse[p]; group g has the key uniq[g] = min(a,b) * base + max(a,b), counts[g] face
    edges and the first position starts[g].  Every connectivity table of a mesh is derived from these."""
    perm: Tensor
    uniq: Tensor
    inverse: Tensor
    counts: Tensor
    starts: Tensor
    base: int

    def edges(self) -> Tensor:  # (E,2) int64: the unique sorted vertex pairs, lexicographic, self pairs included
        return torch.stack([self.uniq // self.base, self.uniq % self.base], dim=1)

    def face_pairs(self) -> Tensor:  # (P,2) int32: the two faces of every edge that exactly two face edges use
        two = self.starts[self.counts == 2]
        return torch.stack([self.perm[two] // 3, self.perm[two + 1] // 3], dim=1).int().contiguous()

    def antialias_tables(self) -> Tuple[Tensor, Tensor]:  # raster.edge_topology's (edge_ofs, edge_tri)
        ofs = torch.empty((self.perm.shape[0], 2), dtype=torch.int32, device=self.perm.device)
        ofs[self.perm, 0] = self.starts[self.inverse].int()
        ofs[self.perm, 1] = self.counts[self.inverse].int()
        return ofs.contiguous(), (self.perm // 3).int().contiguous()


def sort_face_edges(tri: Tensor, n_vertices: int) -> FaceEdgeSort:
    """The face edges of tri (T,3) grouped by their unordered vertex pair: one stable torch.sort and one
    unique_consecutive of the key min(a,b) * max(n_vertices,1) + max(a,b) over face edge 3f + k (plumbing; it syncs).
    Any device, CPU included, and no validation."""
    base = max(int(n_vertices), 1)
    a = tri.long()
    b = a[:, [1, 2, 0]]
    key = torch.add(torch.maximum(a, b), torch.minimum(a, b), alpha=base).reshape(-1)
    skey, perm = torch.sort(key, stable=True)
    uniq, inverse, counts = torch.unique_consecutive(skey, return_inverse=True, return_counts=True)
    return FaceEdgeSort(perm, uniq, inverse, counts, torch.cumsum(counts, 0) - counts, base)


class MeshTopology:
    """The one connectivity object of a mesh (Mesh.topology), from t_pos_idx alone: what the tt_mesh_* and tt_uv_*
    kernels and antialias need (include/tt_abi.h).  The constructor validates and runs sort_face_edges once:
      tri         (T,3) int32
      edges       (E,2), dtype of t_pos_idx: the unique sorted face edges in lexicographic order, self pairs included
                  (threestudio Mesh._compute_edges); edges_i32 is its int32 copy
    Derived from that sort on first use and kept, so a consumer pays for its own tables only:
      face_pairs  (P,2) int32: the two faces of every edge that exactly two face edges use
      nbr_ptr     (V+1) int32, nbr_col (2E) int32: vertex -> neighbour CSR, each row ascending (the second sort)
      ws          the device workspace every tt_mesh_* entry point of this mesh shares
      antialias_tables  (edge_ofs (3T,2), edge_tri (3T)) int32, as raster.edge_topology(tri, V) returns them"""

    def __init__(self, t_pos_idx: Tensor, n_vertices: int):
        t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
        V, T = int(n_vertices), int(t_pos_idx.shape[0])
        _chk_size("mesh too large for tt_mesh_*", V=V, T=T)
        self.n_vertices, self.n_faces = V, T
        _chk_range("t_pos_idx", *(_minmax(t_pos_idx).tolist() if T > 0 else (0, -1)), V)  # one read-back
        self.tri = t_pos_idx.int().contiguous()
        self._sort = sort_face_edges(t_pos_idx, V)
        self.edges = self._sort.edges().to(t_pos_idx.dtype).contiguous()
        self.edges_i32 = self.edges if self.edges.dtype == torch.int32 else self.edges.int().contiguous()

    @property
    def n_edges(self) -> int:
        return self.edges.shape[0]

    @cached_property
    def face_pairs(self) -> Tensor:
        return self._sort.face_pairs()

    @cached_property
    def antialias_tables(self) -> Tuple[Tensor, Tensor]:
        return self._sort.antialias_tables()

    @cached_property
    def _nbr(self) -> Tuple[Tensor, Tensor]:
        # both directions of every unique edge, sorted by (row, column): a second stable sort
        e0, e1 = self.edges.long().unbind(1)
        return _csr(torch.cat([e0, e1]), torch.cat([e1, e0]), self.n_vertices, self.n_vertices)

    nbr_ptr = property(lambda self: self._nbr[0])
    nbr_col = property(lambda self: self._nbr[1])

    @cached_property
    def ws(self) -> Tensor:
        return _workspace("tt_mesh_workspace_bytes", self.n_vertices, self.n_faces, device=self.tri.device)


def mesh_topology(t_pos_idx: Tensor, n_vertices: int) -> MeshTopology:
    return MeshTopology(t_pos_idx, n_vertices)


class _MeshLaplacianFn(torch.autograd.Function):
    """tt_mesh_laplacian_fwd / _bwd: threestudio Mesh.laplacian() (uniform Laplacian, mean row norm)."""

    @staticmethod
    def forward(ctx, v_pos, topo):
        loss = torch.empty((), device=v_pos.device, dtype=torch.float32)
        _launch("tt_mesh_laplacian_fwd", v_pos, topo.nbr_ptr, topo.nbr_col, topo.n_vertices, topo.n_faces, topo.ws, loss,
                label="mesh_laplacian_fwd")
        ctx.save_for_backward(v_pos)
        ctx.topo = topo
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        v_pos, = ctx.saved_tensors
        topo = ctx.topo
        g = torch.empty_like(v_pos)
        _launch("tt_mesh_laplacian_bwd", v_pos, topo.nbr_ptr, topo.nbr_col, topo.n_vertices, topo.n_faces,
                g_loss.contiguous().float(), topo.ws, g, label="mesh_laplacian_bwd")
        return g, None


def mesh_laplacian_loss(v_pos: Tensor, topo: MeshTopology) -> Tensor:
    """(1/V) sum_i |sum_{j in N(i), j != i} (v_i - v_j)|: threestudio Mesh.laplacian() (mesh.py:282-288) as HIP
    kernels, differentiable w.r.t. v_pos (V,3) fp32.  No host round trip, no allocation beyond the outputs."""
    return _MeshLaplacianFn.apply(_chk(v_pos, "v_pos", (topo.n_vertices, 3)), topo)


class _MeshNormalConsistencyFn(torch.autograd.Function):
    """tt_mesh_nc_fwd / _bwd: threestudio Mesh.normal_consistency() w.r.t. the vertex normals."""

    @staticmethod
    def forward(ctx, v_nrm, topo):
        loss = torch.empty((), device=v_nrm.device, dtype=torch.float32)
        _launch("tt_mesh_nc_fwd", v_nrm, topo.edges_i32, topo.n_vertices, topo.n_faces, topo.n_edges, topo.ws, loss,
                label="mesh_nc_fwd")
        ctx.save_for_backward(v_nrm)
        ctx.topo = topo
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        v_nrm, = ctx.saved_tensors
        topo = ctx.topo
        g = torch.empty_like(v_nrm)
        _launch("tt_mesh_nc_bwd", v_nrm, topo.nbr_ptr, topo.nbr_col, topo.n_vertices, topo.n_edges,
                g_loss.contiguous().float(), g, label="mesh_nc_bwd")
        return g, None


def mesh_normal_consistency_loss(v_nrm: Tensor, topo: MeshTopology) -> Tensor:
    """mean over the mesh edges (a,b) of 1 - cosine_similarity(n_a, n_b, eps=1e-8): threestudio
    Mesh.normal_consistency() (mesh.py:269-274) as HIP kernels, differentiable w.r.t. v_nrm (V,3) fp32 (the caller's
    autograd carries it on to v_pos)."""
    return _MeshNormalConsistencyFn.apply(_chk(v_nrm, "v_nrm", (topo.n_vertices, 3)), topo)


def mesh_face_components(topo: MeshTopology) -> Tensor:
    """(T,) int32 connected-component label per face: the smallest face index of its component (faces joined by an
    edge that exactly two face edges use).  Leaves the per-component face counts in topo.ws."""
    labels = torch.empty(topo.n_faces, device=topo.tri.device, dtype=torch.int32)
    _launch("tt_mesh_components", topo.face_pairs, topo.face_pairs.shape[0], topo.n_faces, topo.ws, labels,
            label="mesh_components")
    return labels


@torch.no_grad()
def mesh_remove_small_components(v_pos: Tensor, t_pos_idx: Tensor, threshold, topo: MeshTopology
                                 ) -> Tuple[Tensor, Tensor]:
    """Drop the connected components with fewer than `threshold` faces (threestudio Mesh.remove_outlier's rule: a
    float threshold t means int(largest component's faces * t), an int is used as given; components with
    faces >= threshold stay) and the vertices no kept face references.  Kept vertices and faces keep their original
    order; faces are renumbered.  Returns (v_pos', t_pos_idx') with t_pos_idx's dtype; a mesh without faces comes
    back as it is.  One 8-byte read-back."""
    v_pos = _chk(v_pos, "v_pos", (topo.n_vertices, 3))
    if t_pos_idx.shape != topo.tri.shape:
        raise ValueError(f"t_pos_idx {tuple(t_pos_idx.shape)} is not the topology's {tuple(topo.tri.shape)}")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise TypeError(f"threshold must be an int or a float, got {type(threshold).__name__}")
    if topo.n_faces == 0:
        return v_pos, t_pos_idx
    frac_mode = isinstance(threshold, float)
    if frac_mode and threshold != threshold:
        raise ValueError("threshold is NaN")
    thr_int = 0 if frac_mode else max(min(int(threshold), 1 << 62), -(1 << 62))
    frac = max(min(float(threshold), 1e300), -1e300) if frac_mode else 0.0
    V, T = topo.n_vertices, topo.n_faces
    labels = mesh_face_components(topo)
    totals = torch.empty(2, device=v_pos.device, dtype=torch.int32)
    _launch("tt_mesh_compact_count", topo.tri, labels, V, T, int(frac_mode), frac, thr_int, topo.ws, totals,
            label="mesh_compact_count")
    n_vert, n_tri = (int(x) for x in totals.cpu())
    v_out = torch.empty((n_vert, 3), device=v_pos.device, dtype=torch.float32)
    t_out = torch.empty((n_tri, 3), device=v_pos.device, dtype=torch.int32)
    if n_tri > 0:
        _launch("tt_mesh_compact_emit", v_pos, topo.tri, V, T, topo.ws, v_out, t_out, label="mesh_compact_emit")
    return v_out, t_out.to(t_pos_idx.dtype)


# ---------------------------------------------------------------------------------------------------------------
# UV atlas and texture fill (include/tt_abi.h, "UV atlas and texture fill"): the exporter's xatlas / cv2.inpaint
UV_DEFAULT_ROUNDS, UV_DEFAULT_TAU = _lib.TT_UV_DEFAULT_ROUNDS, _lib.TT_UV_DEFAULT_TAU
UV_MAX_OVERLAP_ROUNDS = _lib.TT_UV_MAX_OVERLAP_ROUNDS
UV_METHODS = ("axis", "lscm")
UV_LSCM_DEFAULT_TOL, UV_LSCM_DEFAULT_MAX_ITERS = _lib.TT_UV_LSCM_DEFAULT_TOL, _lib.TT_UV_LSCM_DEFAULT_MAX_ITERS


def uv_method(method: Optional[str]) -> str:
    """The canonical name of an atlas flattening: None means "axis"; anything but UV_METHODS is a ValueError."""
    name = "axis" if method is None else method
    if name not in UV_METHODS:
        raise ValueError(f"unknown UV method {method!r}: one of {UV_METHODS}")
    return name


def _lscm_tables(tri: Tensor, chart: Tensor, t_tex_idx: Tensor, Vt: int, C: int) -> Tuple[Tensor, int]:
    """The int32 `tables` of tt_uv_lscm_* (include/tt_abi.h, "conformal UV charts": the UV vertices in chart order, the
    corner CSR on them, the charts' vertex ranges and their tiles) and the tile count: two stable torch sorts and one
    read-back (plumbing)."""
    dev, T, tile = tri.device, tri.shape[0], _lib.TT_UV_LSCM_TILE
    i64 = dict(device=dev, dtype=torch.int64)
    tt = t_tex_idx.reshape(-1).long()
    # chart and mesh vertex of every UV vertex (all corners of one (chart, vertex) pair write the same value)
    vchart_u, vmesh_u = torch.empty(Vt, **i64), torch.empty(Vt, **i64)
    vchart_u[tt] = chart.long().repeat_interleave(3)
    vmesh_u[tt] = tri.reshape(-1).long()
    vchart, vperm = torch.sort(vchart_u, stable=True)
    spos = torch.empty(Vt, **i64)
    spos[vperm] = torch.arange(Vt, **i64)
    fc = spos[tt]
    cptr, ccol = _csr(fc, None, Vt, 3 * T)
    n = torch.bincount(vchart, minlength=C)
    vptr, tptr = torch.zeros(C + 1, **i64), torch.zeros(C + 1, **i64)
    vptr[1:] = torch.cumsum(n, 0)
    n_tile = (n + (tile - 1)) // tile
    tptr[1:] = torch.cumsum(n_tile, 0)
    NT = int(tptr[-1].item())
    tchart = torch.repeat_interleave(torch.arange(C, **i64), n_tile)
    tbegin = vptr[tchart] + tile * (torch.arange(NT, **i64) - tptr[tchart])
    tables = torch.cat([fc, ccol.long(), vmesh_u[vperm], vchart, vperm, cptr.long(), vptr, tptr, tchart, tbegin])
    return tables.int().contiguous(), NT


def _lscm_flatten(v_pos: Tensor, tri: Tensor, chart: Tensor, t_tex_idx: Tensor, Vt: int, C: int,
                  chart_box: Optional[Tensor], tau: float, tol: float, max_iters: int) -> dict:
    """tt_uv_lscm_setup / _iterate / _finish on dense chart ids 0..C-1 and their UV vertices (t_tex_idx, Vt): the
    conformal map of every chart and which charts keep it.  The solver's state is read back once every
    TT_UV_LSCM_CHECK_EVERY iterations (4 bytes: the charts still iterating)."""
    dev, V, T = v_pos.device, v_pos.shape[0], tri.shape[0]
    tables, NT = _lscm_tables(tri, chart, t_tex_idx, Vt, C)
    if tables.numel() != int(_lib.load().tt_uv_lscm_table_ints(T, Vt, C, NT)):
        raise RuntimeError("uv lscm: the tables do not have the layout of include/tt_abi.h")
    ws = _workspace("tt_uv_lscm_workspace_bytes", T, Vt, C, NT, device=dev)
    totals = torch.empty(4, device=dev, dtype=torch.int32)
    with _timed("uv_lscm_solve"):
        _launch("tt_uv_lscm_setup", v_pos, tables, V, T, Vt, C, NT, ws)
        it = 0
        while it < max_iters:
            n = min(_lib.TT_UV_LSCM_CHECK_EVERY, max_iters - it)
            _launch("tt_uv_lscm_iterate", tables, T, Vt, C, NT, n, float(tol), ws, totals)
            it += n
            if int(totals[0].item()) == 0:
                break
        f64 = dict(device=dev, dtype=torch.float64)
        out = {"uv": torch.empty((Vt, 2), **f64), "uv_final": torch.empty((Vt, 2), device=dev),
               "box": torch.empty((C, 4), device=dev), "fallback": torch.empty(C, device=dev, dtype=torch.uint8),
               "pins": torch.empty((C, 2), device=dev, dtype=torch.int32),
               "chart_iterations": torch.empty(C, device=dev, dtype=torch.int32), "residual": torch.empty(C, **f64),
               "rotation": torch.empty(C, **f64), "scale": torch.empty(C, **f64)}
        _launch("tt_uv_lscm_finish", tables, chart_box, T, Vt, C, NT, float(tau), ws, out["uv"], out["uv_final"],
                out["box"], out["fallback"], out["pins"], out["chart_iterations"], out["residual"], out["rotation"],
                out["scale"])
    out["fallback"] = out["fallback"].bool()
    out["iterations"] = it
    return out


def _chk_lscm_args(tau: float, tol: float, max_iters: int) -> Tuple[float, float, int]:
    if not (0.0 < float(tau) <= _lib.TT_UV_MAX_TAU):
        raise ValueError(f"tau must lie in (0, {_lib.TT_UV_MAX_TAU}], got {tau}")
    if not (0.0 <= float(tol) < 1.0):
        raise ValueError(f"lscm tolerance must lie in [0, 1), got {tol}")
    if isinstance(max_iters, bool) or int(max_iters) != max_iters or max_iters < 0:
        raise ValueError(f"lscm max_iters must be an integer >= 0, got {max_iters}")
    return float(tau), float(tol), int(max_iters)


@torch.no_grad()
def uv_flatten_lscm(v_pos: Tensor, t_pos_idx: Tensor, chart: Tensor, tol: float = UV_LSCM_DEFAULT_TOL,
                    max_iters: int = UV_LSCM_DEFAULT_MAX_ITERS, tau: float = UV_DEFAULT_TAU
                    ) -> Tuple[Tensor, Tensor, dict]:
    """The least-squares conformal map of every chart of a face -> chart assignment (`chart` (T,) int32: a chart is the
    set of faces with one id), the solver of uv_atlas(method="lscm") on its own (include/tt_abi.h, "conformal UV
    charts").  Returns uv (Vt,2) fp64, the raw solution with the chart's two pins at (0,0) and (|p1 - p0|, 0); t_tex_idx
    (T,3) int32, one UV vertex per distinct (chart, vertex) pair in order of its first corner; and info, whose (C,)
    entries follow the sorted chart ids info["chart_ids"]: fallback (bool: the chart did not converge within max_iters
    to |r| <= tol |b|, is degenerate, flips a face or stretches one beyond [tau, 1/tau] in area), pins (C,2),
    iterations, chart_iterations, residual, rotation, scale, uv_final (Vt,2) fp32 (scaled to the 3-D area, principal
    axis along u; zeros for fallback charts) and box (C,4).  Nothing raises for a chart that fails.  Bit-identical from
    call to call."""
    tau, tol, max_iters = _chk_lscm_args(tau, tol, max_iters)
    v_pos = _chk(v_pos.detach(), "v_pos", (None, 3))
    V = v_pos.shape[0]
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    T = t_pos_idx.shape[0]
    _chk_size("mesh too large for tt_uv_lscm_*", V=V, T=T)
    chart = _chk(chart, "chart", (T,), dtype=torch.int32)
    dev = v_pos.device
    i32 = dict(device=dev, dtype=torch.int32)
    if T == 0:
        return (torch.zeros((0, 2), device=dev, dtype=torch.float64), torch.zeros((0, 3), **i32),
                {"charts": 0, "iterations": 0})
    _chk_range("t_pos_idx", *_minmax(t_pos_idx).tolist(), V)  # one read-back
    tri = t_pos_idx.int().contiguous()
    ids, dense = torch.unique(chart, return_inverse=True)
    dense, C = dense.int().contiguous(), int(ids.shape[0])
    ws = _workspace("tt_uv_workspace_bytes", V, T, 1, device=dev)
    totals = torch.empty(4, **i32)
    _launch("tt_uv_emit_count", tri, dense, V, T, 1, ws, totals)
    Vt = int(totals[0].item())
    t_tex_idx = torch.empty((T, 3), **i32)
    _launch("tt_uv_lscm_index", V, T, 1, ws, t_tex_idx)
    info = _lscm_flatten(v_pos, tri, dense, t_tex_idx, Vt, C, None, tau, tol, max_iters)
    info.update(charts=C, chart_ids=ids)
    return info["uv"], t_tex_idx, info


@torch.no_grad()
def uv_atlas(v_pos: Tensor, t_pos_idx: Tensor, topology: Optional[MeshTopology] = None, texture_size: int = 1024,
             padding: int = 2, rounds: int = UV_DEFAULT_ROUNDS, tau: float = UV_DEFAULT_TAU,
             max_overlap_rounds: int = UV_MAX_OVERLAP_ROUNDS, method: Optional[str] = "axis",
             lscm_tol: float = UV_LSCM_DEFAULT_TOL, lscm_max_iters: int = UV_LSCM_DEFAULT_MAX_ITERS
             ) -> Tuple[Tensor, Tensor, dict]:
    """Axis-projection UV atlas of a mesh for a texture_size^2 texture with `padding` texels around every chart:
    v_tex (Vt,2) fp32 in [0,1], t_tex_idx (T,3) int32 (face f of t_pos_idx), and info = {charts, scale (texels per
    world unit), fill_ratio (covered texel centres / N^2), overlap_rounds, labels, chart, chart_box, offsets,
    singleton}.  Labels and charts on the GPU (tt_uv_labels / tt_uv_charts), shelf packing on the host (tt_uv_pack,
    one read-back of the chart boxes), UVs (tt_uv_emit_count / tt_uv_emit), then the overlap guard (tt_uv_overlap):
    faces on a texel centre that two UV triangles cover become singleton charts and the atlas is redone; after
    max_overlap_rounds such rounds every face of a chart that still overlaps becomes a singleton.  Bit-identical from
    call to call.

    method="lscm" flattens the same charts by a least-squares conformal map instead (include/tt_abi.h, "conformal UV
    charts"; _lscm_flatten, re-solved in every overlap round): each chart is scaled to its 3-D area and turned with its
    principal axis along u before packing; a chart that does not converge within lscm_max_iters to lscm_tol, flips a
    face or changes a face's area by more than [tau, 1/tau] keeps its axis projection.  info["lscm"] then holds, for
    the last round: uv (Vt,2) fp64 (the raw solution), uv_final, iterations, chart_iterations, residual (C,), pins
    (C,2), fallback (C,) bool, rotation, scale (C,), and chart_round0, the charts before the overlap guard."""
    method = uv_method(method)
    lscm = method == "lscm"
    if lscm:
        tau, lscm_tol, lscm_max_iters = _chk_lscm_args(tau, lscm_tol, lscm_max_iters)
    v_pos = _chk(v_pos.detach(), "v_pos", (None, 3))
    V = v_pos.shape[0]
    topo = topology if topology is not None else mesh_topology(t_pos_idx, V)
    if topo.n_vertices != V or tuple(topo.tri.shape) != tuple(t_pos_idx.shape):
        raise ValueError("topology was built for another mesh")
    T, N, pad = topo.n_faces, int(texture_size), int(padding)
    dev = v_pos.device
    ws = _workspace("tt_uv_workspace_bytes", V, T, N, device=dev)
    i32 = dict(device=dev, dtype=torch.int32)
    info = {"charts": 0, "scale": 0.0, "fill_ratio": 0.0, "overlap_rounds": 0, "texture_size": N, "padding": pad}
    if T == 0:
        return torch.zeros((0, 2), device=dev), torch.zeros((0, 3), **i32), info
    tri, pairs = topo.tri, topo.face_pairs
    P = pairs.shape[0]
    labels = torch.empty(T, **i32)
    _launch("tt_uv_labels", v_pos, tri, pairs, V, T, P, int(rounds), float(tau), N, ws, labels, label="uv_labels")
    singleton = torch.zeros(T, device=dev, dtype=torch.uint8)
    flags = torch.empty(T, device=dev, dtype=torch.uint8)
    chart = torch.empty(T, **i32)
    box = torch.empty((T, 4), device=dev, dtype=torch.float32)
    totals = torch.empty(4, **i32)
    r = 0
    while True:
        _launch("tt_uv_charts", v_pos, tri, pairs, labels, singleton, V, T, P, N, ws, chart, box, totals,
                label="uv_charts")
        C = int(totals[0].item())
        if lscm:  # the conformal maps come before the packing: their boxes are what is packed
            _launch("tt_uv_emit_count", tri, chart, V, T, N, ws, totals)
            Vt = int(totals[0].item())
            t_tex_idx = torch.empty((T, 3), **i32)
            _launch("tt_uv_lscm_index", V, T, N, ws, t_tex_idx)
            sol = _lscm_flatten(v_pos, tri, chart, t_tex_idx, Vt, C, box, tau, lscm_tol, lscm_max_iters)
            if r == 0:
                sol_chart0 = chart.clone()
        pbox = sol["box"] if lscm else box  # (C,4) / (T,4): rows 0..C-1 are the charts' boxes
        box_h = pbox[:C].cpu()
        off_h = torch.empty((C, 2), dtype=torch.int32)
        scale_h = torch.zeros(1, dtype=torch.float32)
        st = _lib.load().tt_uv_pack(_ptr(box_h), C, N, pad, _ptr(off_h), _ptr(scale_h))  # on the host: no stream
        if st == _lib.TT_ERR_UNSUPPORTED:
            raise RuntimeError(f"uv_atlas: {C} charts do not fit a {N}^2 atlas with padding {pad} (every chart box is at "
                               f"least {2 * pad + 1}^2 texels): use a larger texture_size or a smaller padding")
        _lib.check(st, "tt_uv_pack")
        offsets = off_h.to(dev)
        scale = float(scale_h[0])
        with _timed("uv_emit"):
            if lscm:
                v_tex = torch.empty((Vt, 2), device=dev, dtype=torch.float32)
                _launch("tt_uv_lscm_emit", v_pos, tri, labels, chart, t_tex_idx, sol["uv_final"],
                        sol["fallback"].to(torch.uint8), pbox, offsets, C, scale, V, T, Vt, N, pad, v_tex)
            else:
                _launch("tt_uv_emit_count", tri, chart, V, T, N, ws, totals)
                Vt = int(totals[0].item())
                v_tex = torch.empty((Vt, 2), device=dev, dtype=torch.float32)
                t_tex_idx = torch.empty((T, 3), **i32)
                _launch("tt_uv_emit", v_pos, tri, labels, chart, box, offsets, C, scale, V, T, N, pad, ws, v_tex,
                        t_tex_idx)
        _launch("tt_uv_overlap", v_tex, t_tex_idx, Vt, V, T, N, ws, flags, totals, label="uv_overlap")
        n_flagged, n_covered = (int(x) for x in totals[:2].cpu())
        if n_flagged == 0:
            break
        if r < max_overlap_rounds:
            singleton |= flags
        else:  # every face of a chart that still overlaps: singleton charts sit in disjoint boxes and cannot overlap
            hit = torch.zeros(C, device=dev, dtype=torch.bool)
            hit[chart[flags.bool()].long()] = True
            singleton |= hit[chart.long()].to(torch.uint8)
        r += 1  # a flagged face is never a singleton: every round adds singletons, so the loop ends
    info.update(charts=C, scale=scale, fill_ratio=n_covered / float(N * N), overlap_rounds=r, labels=labels,
                chart=chart, chart_box=box_h, offsets=off_h, singleton=singleton)
    if lscm:
        info["lscm"] = dict(sol, chart_round0=sol_chart0)
    return v_tex, t_tex_idx, info


@torch.no_grad()
def texture_fill(img: Tensor, mask: Tensor) -> Tensor:
    """img (H,W,C) fp32 with every texel where mask (H,W) bool is False replaced by the texel value at the nearest
    True texel (jump flooding, tt_tex_fill); True texels come back bit for bit.  The exporter's stand-in for
    cv2.inpaint(TELEA) (multiprompt_mesh_exporter.py:96-107).  A (H,W) image is filled as one channel."""
    squeeze = img.dim() == 2
    x = _chk((img[..., None] if squeeze else img).detach(), "img", (None, None, None))  # (H,W) came in as (H,W,1)
    H, W, C = x.shape
    if not isinstance(mask, torch.Tensor) or not mask.is_cuda or tuple(mask.shape) != (H, W):
        raise ValueError(f"mask must be a GPU tensor of shape {(H, W)}")
    m = (mask != 0).to(torch.uint8).contiguous()
    ws = _workspace("tt_tex_fill_workspace_bytes", H, W, device=x.device)
    out = torch.empty_like(x)
    _launch("tt_tex_fill", x, m, H, W, C, ws, out, label="tex_fill")
    return out[..., 0] if squeeze else out


# ---------------------------------------------------------------------------------------------------------------
# mesh simplification (include/tt_abi.h, "mesh simplification"): vertex clustering with quadric-error placement
SIMPLIFY_DEFAULT_LAM = 1e-3


def _simplify_unchanged(v_pos: Tensor, t_pos_idx: Tensor, grid: int, cell: float) -> Tuple[Tensor, Tensor, dict]:
    V = v_pos.shape[0]
    info = {"grid": grid, "cell": cell, "n_clusters": V, "unchanged": True,
            "vertex_map": torch.arange(V, device=v_pos.device, dtype=torch.int32)}
    return v_pos, t_pos_idx, info


@torch.no_grad()
def mesh_simplify(v_pos: Tensor, t_pos_idx: Tensor, grid: int, lam: float = SIMPLIFY_DEFAULT_LAM
                  ) -> Tuple[Tensor, Tensor, dict]:
    """Vertex clustering on a grid^3 lattice over the mesh's bounding cube, one output vertex per occupied cell placed
    by its quadric (regularised towards the mean of the cell's vertices with weight lam, clamped to the cell); faces
    that collapse are dropped and duplicates of a surviving face removed (tt_simplify_*; three stable torch sorts and
    three small read-backs).  Returns v_pos' (V',3) fp32, t_pos_idx' (T',3) int32 and info = {grid, cell (the cell
    side h), n_clusters, vertex_map (V,) int32: the output vertex of each input vertex's cluster, -1 if dropped,
    unchanged}.  Every input vertex lies within sqrt(3) h of its output vertex; bit-identical from call to call.  A
    mesh without vertices, faces or extent comes back as it is (unchanged = True).  The output need not be manifold or
    free of self-intersections.  Positions are detached; the result never requires grad."""
    if isinstance(grid, bool) or not isinstance(grid, int):
        raise TypeError(f"grid must be an int, got {type(grid).__name__}")
    if not _lib.TT_SIMPLIFY_MIN_GRID <= grid <= _lib.TT_SIMPLIFY_MAX_GRID:
        raise ValueError(f"grid must be in [{_lib.TT_SIMPLIFY_MIN_GRID}, {_lib.TT_SIMPLIFY_MAX_GRID}], got {grid}")
    lam = float(lam)
    if not 0.0 <= lam <= 1e300:
        raise ValueError(f"lam must be a finite number >= 0, got {lam}")
    if (isinstance(v_pos, Tensor) and isinstance(t_pos_idx, Tensor) and v_pos.shape[1:] == t_pos_idx.shape[1:] == (3,)
            and t_pos_idx.dtype in (torch.int32, torch.int64) and 0 in (v_pos.shape[0], t_pos_idx.shape[0])):
        return _simplify_unchanged(v_pos.detach(), t_pos_idx, grid, 0.0)  # an empty mesh, wherever it lives
    v_pos = _chk(v_pos, "v_pos", (None, 3)).detach()
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    V, T, dev = v_pos.shape[0], t_pos_idx.shape[0], v_pos.device
    _chk_size("mesh too large for tt_simplify_*", V=V, T=T)
    lo, _, ext = _mesh_box(v_pos, t_pos_idx)  # the box in fp32; the two divisions below in IEEE fp32 on the host
    if ext == 0:
        return _simplify_unchanged(v_pos, t_pos_idx, grid, 0.0)
    h, inv_h = ext / np.float32(grid), np.float32(grid) / ext
    if not (np.isfinite(inv_h) and h > 0):
        raise ValueError(f"the mesh's extent {float(ext)} is too small for grid {grid} in fp32")
    lo3 = [float(x) for x in lo]
    h, inv_h = float(h), float(inv_h)
    tri = t_pos_idx.int().contiguous()
    ws = _workspace("tt_simplify_workspace_bytes", V, T, device=dev)
    i32 = dict(device=dev, dtype=torch.int32)
    i64 = dict(device=dev, dtype=torch.int64)
    totals = torch.empty(2, **i32)
    keys = torch.empty(V, **i64)
    _launch("tt_simplify_keys", v_pos, V, grid, *lo3, inv_h, keys, label="simplify_keys")
    skeys, perm = torch.sort(keys, stable=True)
    rank = torch.empty(V, **i32)
    _launch("tt_simplify_ranks", skeys, perm, V, T, grid, ws, rank, totals, label="simplify_ranks")
    C = int(totals[0].item())
    if C > _lib.TT_SIMPLIFY_MAX_CLUSTERS:
        raise ValueError(f"grid {grid} gives {C} clusters, more than {_lib.TT_SIMPLIFY_MAX_CLUSTERS}: use a coarser grid")
    pkeys = torch.empty(3 * T, **i64)
    _launch("tt_simplify_pairs", tri, rank, V, T, C, ws, pkeys, label="simplify_pairs")
    spkeys = torch.sort(pkeys, stable=True)[0]
    cpos = torch.empty((C, 3), device=dev, dtype=torch.float32)
    _launch("tt_simplify_solve", v_pos, tri, spkeys, perm, V, T, C, grid, *lo3, h, lam, ws, cpos,
            label="simplify_solve")
    fkeys = torch.empty(T, **i64)
    _launch("tt_simplify_faces", tri, rank, V, T, C, fkeys, label="simplify_faces")
    sfkeys, fperm = torch.sort(fkeys, stable=True)
    _launch("tt_simplify_emit_count", sfkeys, fperm, tri, rank, V, T, C, ws, totals, label="simplify_emit_count")
    n_vert, n_tri = (int(x) for x in totals.cpu())
    v_out = torch.empty((n_vert, 3), device=dev, dtype=torch.float32)
    t_out = torch.empty((n_tri, 3), **i32)
    vertex_map = torch.full((V,), -1, **i32)
    if n_tri > 0:
        _launch("tt_simplify_emit", cpos, tri, rank, V, T, C, ws, v_out, t_out, vertex_map, label="simplify_emit")
    return v_out, t_out, {"grid": grid, "cell": h, "n_clusters": C, "vertex_map": vertex_map, "unchanged": False}


# ---------------------------------------------------------------------------------------------------------------
# mesh decimation (include/tt_abi.h, "mesh decimation"): manifold-preserving parallel quadric edge collapse
def _decimate_unchanged(v_pos: Tensor, t_pos_idx: Tensor, target_faces: int, stalled: bool = False, n_locked: int = 0,
                        return_trace: bool = False) -> Tuple[Tensor, Tensor, dict]:
    V = v_pos.shape[0]
    info = {"target_faces": target_faces, "n_rounds": 0, "stalled": stalled, "n_locked": n_locked, "unchanged": True,
            "vertex_map": torch.arange(V, device=v_pos.device, dtype=torch.int32)}
    if return_trace:
        info["trace"] = []
    return v_pos, t_pos_idx, info


@torch.no_grad()
def mesh_decimate(v_pos: Tensor, t_pos_idx: Tensor, target_faces: int, max_rounds: Optional[int] = None,
                  return_trace: bool = False) -> Tuple[Tensor, Tensor, dict]:
    """Edge-collapse decimation to at most target_faces faces that keeps a closed 2-manifold a closed 2-manifold of the
    same genus and flips no face: rounds of quadric edge collapses whose closed neighbourhoods are pairwise disjoint
    (tt_decimate_*; per round one face-edge sort, two CSR sorts, one sort of the costs and four small read-backs).
    Vertices on a boundary or a non-manifold edge are locked: they never move or merge.  Returns v_pos' (V',3) fp32,
    t_pos_idx' (T',3) int32 and info = {target_faces, n_rounds (rounds that collapsed something), stalled (a round
    found no valid collapse before the target was reached), n_locked (locked vertices of the input), vertex_map (V,)
    int32: the output vertex each input vertex ended in, -1 for one no face referenced, unchanged}; with return_trace
    info["trace"] holds one (edges (k,2) int32, xopt (k,3) fp32, cost_bits (k,) int64) per round: the collapses b -> a it
    applied.  A closed manifold that does not stall ends with target_faces - 1 or target_faces faces.  A mesh that is
    empty, has no more than target_faces faces or admits no collapse comes back as it is (unchanged = True).
    Bit-identical from call to call.  Positions are detached; the result never requires grad."""
    if isinstance(target_faces, bool) or not isinstance(target_faces, int):
        raise TypeError(f"target_faces must be an int, got {type(target_faces).__name__}")
    if target_faces < _lib.TT_DECIMATE_MIN_FACES:
        raise ValueError(f"target_faces must be at least {_lib.TT_DECIMATE_MIN_FACES}, got {target_faces}")
    if max_rounds is None:
        max_rounds = _lib.TT_DECIMATE_DEFAULT_ROUNDS
    elif isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or max_rounds < 0:
        raise ValueError(f"max_rounds must be a non-negative int, got {max_rounds!r}")
    if (isinstance(v_pos, Tensor) and isinstance(t_pos_idx, Tensor) and v_pos.shape[1:] == t_pos_idx.shape[1:] == (3,)
            and t_pos_idx.dtype in (torch.int32, torch.int64) and 0 in (v_pos.shape[0], t_pos_idx.shape[0])):
        return _decimate_unchanged(v_pos.detach(), t_pos_idx, target_faces, return_trace=return_trace)  # an empty mesh
    v_pos = _chk(v_pos, "v_pos", (None, 3)).detach()
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    V, T, dev = v_pos.shape[0], t_pos_idx.shape[0], v_pos.device
    _chk_size("mesh too large for tt_decimate_*", V=V, T=T)
    chk = torch.cat([torch.isfinite(v_pos).all().reshape(1).long(), _minmax(t_pos_idx).long()]).tolist()  # one read-back
    _chk_range("t_pos_idx", chk[1], chk[2], V)
    if not chk[0]:
        raise ValueError("v_pos holds a value that is not finite")
    if T <= target_faces:
        return _decimate_unchanged(v_pos, t_pos_idx, target_faces, return_trace=return_trace)
    i32 = dict(device=dev, dtype=torch.int32)
    u8 = dict(device=dev, dtype=torch.uint8)
    ws = _workspace("tt_decimate_workspace_bytes", V, T, device=dev)
    pos = v_pos.clone()
    bufs = [t_pos_idx.int().contiguous().clone(), torch.empty((T, 3), **i32)]  # the live faces, written back and forth
    tri, cur = bufs[0], 0
    vf_ptr, vf_col = _csr(tri.reshape(-1).long(), None, V, 3 * T)
    quadrics = torch.empty((V, 10), device=dev, dtype=torch.float64)
    _launch("tt_decimate_quadrics", pos, tri, vf_ptr, vf_col, V, T, quadrics, label="decimate_quadrics")
    root, remap = torch.arange(V, **i32), torch.arange(V, **i32)
    locked, taken = torch.empty(V, **u8), torch.empty(V, **u8)
    owner = torch.empty(V, device=dev, dtype=torch.int64)
    totals = torch.empty(2, **i32)
    trace, stalled, n_locked, rnd = [], False, 0, 0
    while T > target_faces and rnd < max_rounds:
        fe = sort_face_edges(tri, V)
        e0, e1 = fe.uniq // fe.base, fe.uniq % fe.base
        E = int(e0.shape[0])
        edges = torch.stack([e0, e1], dim=1).int().contiguous()
        nbr_ptr, nbr_col = _csr(torch.cat([e0, e1]), torch.cat([e1, e0]), V, V)
        if rnd > 0:
            vf_ptr, vf_col = _csr(tri.reshape(-1).long(), None, V, 3 * T)
        _launch("tt_decimate_lock", edges, fe.counts.int().contiguous(), V, E, locked, label="decimate_lock")
        cost_bits, xopt = torch.empty(E, **i32), torch.empty((E, 3), device=dev, dtype=torch.float32)
        _launch("tt_decimate_edges", pos, quadrics, tri, edges, nbr_ptr, nbr_col, vf_ptr, vf_col, locked, V, T, E,
                cost_bits, xopt, label="decimate_edges")
        # the threshold stays on the device: the cost bits at rank floor(quantile * n_valid) of the valid edges
        cb = cost_bits.long() & 0xffffffff
        n_valid = (cb != 0xffffffff).sum()
        rank = (n_valid.double() * _lib.TT_DECIMATE_QUANTILE).floor().long().clamp(max=E - 1)
        tau = torch.sort(cb)[0].gather(0, rank.reshape(1)).contiguous()
        state = torch.empty(E, **u8)
        taken.zero_()
        for p in range(_lib.TT_DECIMATE_SELECT_PASSES):
            owner.fill_(-1)
            _launch("tt_decimate_mark", edges, nbr_ptr, nbr_col, cost_bits, tau, V, T, E, rnd, p, state, taken, owner,
                    label="decimate_mark")
            _launch("tt_decimate_select", edges, nbr_ptr, nbr_col, V, T, E, rnd, state, taken, owner,
                    label="decimate_select")
        selected = state == 2
        n_valid, n_selected, n_lock = torch.stack([n_valid, selected.sum(), locked.sum()]).tolist()  # one read-back
        if rnd == 0:
            n_locked = n_lock
        if n_valid == 0 or n_selected == 0:
            stalled = True
            break
        need = (T - target_faces + 1) // 2
        kept = selected.nonzero().reshape(-1)  # ascending edge index
        if n_selected > need:  # the `need` smallest by (cost bits, edge index)
            kept = torch.sort(kept[torch.sort(cb[kept], stable=True)[1][:need]])[0]
        K = int(kept.shape[0])
        k_edges, k_xopt = edges[kept].contiguous(), xopt[kept].contiguous()
        out = bufs[1 - cur]
        _launch("tt_decimate_apply", k_edges, k_xopt, tri, V, T, K, ws, pos, quadrics, remap, root, out, totals,
                label="decimate_apply")
        T = int(totals[1].item())
        cur = 1 - cur
        tri = bufs[cur][:T]
        rnd += 1
        if return_trace:
            trace.append((k_edges, k_xopt, cb[kept]))
    if rnd == 0:
        return _decimate_unchanged(v_pos, t_pos_idx, target_faces, stalled, n_locked, return_trace)
    _launch("tt_decimate_emit_count", tri, V, T, ws, totals, label="decimate_emit_count")
    n_vert = int(totals[0].item())
    v_out = torch.empty((n_vert, 3), device=dev, dtype=torch.float32)
    t_out = torch.empty((T, 3), **i32)
    vertex_map = torch.empty(V, **i32)
    _launch("tt_decimate_emit", pos, tri, root, V, T, ws, v_out, t_out, vertex_map, label="decimate_emit")
    info = {"target_faces": target_faces, "n_rounds": rnd, "stalled": stalled, "n_locked": n_locked,
            "vertex_map": vertex_map, "unchanged": False}
    if return_trace:
        info["trace"] = trace
    return v_out, t_out, info


# ---------------------------------------------------------------------------------------------------------------
# isotropic remeshing (include/tt_abi.h, "isotropic remeshing"): split, collapse, flip, relax on the input's surface
def remesh_thresholds(edge_length: float) -> Tuple[float, float]:
    """(hi2, lo2) of the contract: the fp32 squares of (float)(4/3 L) and (float)(4/5 L)."""
    h, l = np.float32((4.0 / 3.0) * edge_length), np.float32(0.8 * edge_length)
    return float(np.float32(h * h)), float(np.float32(l * l))


def remesh_edge_length(area: float, target_faces: int) -> float:
    """The edge length at which equilateral triangles cover `area` with target_faces faces: sqrt(4 A / (sqrt 3 N))."""
    return float(np.sqrt(4.0 * area / (np.sqrt(3.0) * target_faces)))


class _RemeshTopology:
    """The topology of one pass or round of ops.mesh_remesh (host plumbing, as ops.mesh_decimate's): the unique edges
    with their counts from one face-edge sort; on demand the neighbour CSR and the locked vertices (`nbr`), the
    vertex -> face CSR (`vf`), the unique edge of every face edge (`face_edge`) and the two face edges of every
    two-face edge (`edge_fe`)."""

    def __init__(self, tri: Tensor, V: int, nbr: bool = False, vf: bool = False, face_edge: bool = False,
                 edge_fe: bool = False):
        with _timed("remesh_topology"):
            fe = sort_face_edges(tri, V)
            e0, e1 = fe.uniq // fe.base, fe.uniq % fe.base
            self.E = int(e0.shape[0])
            self.edges = torch.stack([e0, e1], dim=1).int().contiguous()
            self.counts = fe.counts.int().contiguous()
            if nbr:
                self.nbr_ptr, self.nbr_col = _csr(torch.cat([e0, e1]), torch.cat([e1, e0]), V, V)
            if vf:
                self.vf_ptr, self.vf_col = _csr(tri.reshape(-1).long(), None, V, 3 * tri.shape[0])
            if face_edge:
                self.face_edge = torch.empty(fe.perm.shape[0], device=tri.device, dtype=torch.int32)
                self.face_edge[fe.perm] = fe.inverse.int()
            if edge_fe:
                self.edge_fe = torch.full((self.E, 2), -1, device=tri.device, dtype=torch.int32)
                two = fe.counts == 2
                first = fe.starts[two]
                self.edge_fe[two] = torch.stack([fe.perm[first], fe.perm[first + 1]], dim=1).int()
        if nbr:
            self.locked = torch.empty(V, device=tri.device, dtype=torch.uint8)
            _launch("tt_decimate_lock", self.edges, self.counts, V, self.E, self.locked, label="remesh_lock")


@torch.no_grad()
def mesh_remesh(v_pos: Tensor, t_pos_idx: Tensor, edge_length: float, iterations: Optional[int] = None,
                return_trace: bool = False) -> Tuple[Tensor, Tensor, dict]:
    """Isotropic remeshing towards edge length `edge_length` on the surface of the input mesh (tt_remesh_*; Botsch and
    Kobbelt): `iterations` (default TT_REMESH_DEFAULT_ITERATIONS) times split the edges longer than 4/3 L, collapse the
    edges shorter than 4/5 L to their midpoint, flip edges towards valence 6 and move every vertex tangentially and
    back onto the input surface (ops.mesh_closest_point on a TriangleGrid of the input); then one more split.
    Collapses and flips run in rounds of operations with disjoint neighbourhoods, chosen by hashed integer priorities
    (per round one face-edge sort, the CSR sorts and one read-back).  Vertices on a boundary or a non-manifold edge are
    locked: they never move or merge.  A closed 2-manifold stays one with the same Euler characteristic and
    components, no operation flips a face, and unless info["split_capped"] no edge of the result is longer than
    4/3 L.  NOT guaranteed: a lower bound on edge length (blocked collapses remain), sharp features, and the vertices
    of the closing split lie on chords of the surface, not on it.  Nothing is differentiable.

    Returns v_pos' (V',3) fp32, t_pos_idx' (T',3) int32 and info = {edge_length, iterations, n_split, n_collapsed,
    n_flipped, n_reverted (lists: one entry per iteration, n_split one more for the closing split), n_locked (locked
    vertices of the input), split_capped, rounds_capped (a phase ended at TT_REMESH_MAX_SPLIT_PASSES /
    TT_REMESH_MAX_ROUNDS), rounds (one dict {collapse, flip} per iteration) and split_passes (one count per split phase):
    the rounds and passes that changed something, source_face (V',) int32 and source_bary
    (V',3) fp32: the closest point of the input mesh to every output vertex, unchanged}; with return_trace
    info["trace"] holds the ordered records ("split", edges (k,2) int32), ("collapse", edges (k,2) int32, xopt (k,3)
    fp32), ("flip", edges (k,2) int32, cd (k,2) int32) and ("move", positions (V,3) fp32, reverted (V,) uint8).  An
    empty mesh, or one that no operation changes, comes back as it is (unchanged = True).  Bit-identical from call to
    call.  Positions are detached; the result never requires grad."""
    if iterations is None:
        iterations = _lib.TT_REMESH_DEFAULT_ITERATIONS
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise TypeError(f"iterations must be an int, got {type(iterations).__name__}")
    if iterations < 0:
        raise ValueError(f"iterations must not be negative, got {iterations}")
    if isinstance(edge_length, bool) or not isinstance(edge_length, (int, float)):
        raise TypeError(f"edge_length must be a number, got {type(edge_length).__name__}")
    edge_length = float(edge_length)
    hi2, lo2 = remesh_thresholds(edge_length) if np.isfinite(edge_length) else (0.0, 0.0)
    if not (edge_length > 0.0 and 0.0 < lo2 and hi2 < float("inf")):
        raise ValueError(f"edge_length must be finite and positive (its square in fp32 too), got {edge_length!r}")
    info = {"edge_length": edge_length, "iterations": iterations, "n_split": [], "n_collapsed": [], "n_flipped": [],
            "n_reverted": [], "n_locked": 0, "split_capped": False, "rounds_capped": False, "rounds": [],
            "split_passes": [], "unchanged": True}
    trace: list = []  # filled with return_trace only

    def record(*rec) -> None:
        if return_trace:
            trace.append(rec)

    if return_trace:
        info["trace"] = trace
    if (isinstance(v_pos, Tensor) and isinstance(t_pos_idx, Tensor) and v_pos.shape[1:] == t_pos_idx.shape[1:] == (3,)
            and t_pos_idx.dtype in (torch.int32, torch.int64) and 0 in (v_pos.shape[0], t_pos_idx.shape[0])):
        n = v_pos.shape[0]  # an empty mesh
        info["source_face"] = torch.full((n,), -1, device=v_pos.device, dtype=torch.int32)
        info["source_bary"] = torch.zeros((n, 3), device=v_pos.device, dtype=torch.float32)
        return v_pos.detach(), t_pos_idx, info
    v_pos = _chk(v_pos, "v_pos", (None, 3)).detach()
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    dev = v_pos.device
    _chk_size("mesh too large for tt_remesh_*", V=v_pos.shape[0], T=t_pos_idx.shape[0])
    chk = torch.cat([torch.isfinite(v_pos).all().reshape(1).long(), _minmax(t_pos_idx).long()]).tolist()  # one read-back
    _chk_range("t_pos_idx", chk[1], chk[2], v_pos.shape[0])
    if not chk[0]:
        raise ValueError("v_pos holds a value that is not finite")
    i32 = dict(device=dev, dtype=torch.int32)
    u8 = dict(device=dev, dtype=torch.uint8)
    f32 = dict(device=dev, dtype=torch.float32)
    pos, tri = v_pos.clone(), t_pos_idx.int().contiguous().clone()
    tg = TriangleGrid(v_pos, tri)  # the input surface: every move is pulled back onto it
    totals, count = torch.empty(2, **i32), torch.empty(1, **i32)
    tau = torch.zeros(1, device=dev, dtype=torch.int64)  # tt_decimate_mark's threshold: every candidate is eligible
    info["n_locked"] = int(_RemeshTopology(tri, pos.shape[0], nbr=True).locked.sum().item())

    def split_phase() -> None:
        nonlocal pos, tri
        n = 0
        for p in range(_lib.TT_REMESH_MAX_SPLIT_PASSES + 1):
            V, T = pos.shape[0], tri.shape[0]
            tp = _RemeshTopology(tri, V, face_edge=True)
            ws = _workspace("tt_remesh_workspace_bytes", T, tp.E, device=dev)
            _launch("tt_remesh_split_count", pos, tp.edges, tp.face_edge, V, T, tp.E, hi2, ws, totals,
                    label="remesh_split_count")
            M, Tn = totals.tolist()  # the pass's read-back
            if M == 0:
                break
            if p == _lib.TT_REMESH_MAX_SPLIT_PASSES:
                info["split_capped"] = True
                break
            _chk_size("mesh too large for tt_remesh_* after a split pass: use a larger edge_length", V=V + M, T=Tn)
            v_new, marked = torch.empty((M, 3), **f32), torch.empty((M, 2), **i32)
            t_out = torch.empty((Tn, 3), **i32)
            _launch("tt_remesh_split_emit", pos, tri, tp.edges, tp.face_edge, V, T, tp.E, M, Tn, ws, v_new, marked,
                    t_out, label="remesh_split_emit")
            pos, tri = torch.cat([pos, v_new]), t_out
            record("split", marked)
            n += M
        info["n_split"].append(n)
        info["split_passes"].append(p)

    def collapse_phase() -> int:
        nonlocal tri
        V, n = pos.shape[0], 0
        taken, owner = torch.empty(V, **u8), torch.empty(V, device=dev, dtype=torch.int64)
        quadrics = torch.zeros((V, 10), device=dev, dtype=torch.float64)  # tt_decimate_apply sums them; never read here
        remap, root = torch.arange(V, **i32), torch.arange(V, **i32)
        for rnd in range(_lib.TT_REMESH_MAX_ROUNDS + 1):
            T = tri.shape[0]
            tp = _RemeshTopology(tri, V, nbr=True, vf=True)
            E = tp.E
            cost_bits, xopt, state = torch.empty(E, **i32), torch.empty((E, 3), **f32), torch.empty(E, **u8)
            _launch("tt_remesh_collapse_candidates", pos, tri, tp.edges, tp.nbr_ptr, tp.nbr_col, tp.vf_ptr, tp.vf_col,
                    tp.locked, V, T, E, hi2, lo2, cost_bits, xopt, label="remesh_collapse_candidates")
            taken.zero_()
            owner.fill_(-1)
            _launch("tt_decimate_mark", tp.edges, tp.nbr_ptr, tp.nbr_col, cost_bits, tau, V, T, E, rnd, 0, state, taken,
                    owner, label="remesh_collapse_mark")
            _launch("tt_decimate_select", tp.edges, tp.nbr_ptr, tp.nbr_col, V, T, E, rnd, state, taken, owner,
                    label="remesh_collapse_select")
            kept = (state == 2).nonzero().reshape(-1)  # ascending edge index; the round's read-back
            K = int(kept.shape[0])
            if K == 0:
                return rnd
            if rnd == _lib.TT_REMESH_MAX_ROUNDS:
                info["rounds_capped"] = True
                return rnd
            k_edges, k_xopt = tp.edges[kept].contiguous(), xopt[kept].contiguous()
            ws = _workspace("tt_decimate_workspace_bytes", V, T, device=dev)
            out = torch.empty((T, 3), **i32)
            _launch("tt_decimate_apply", k_edges, k_xopt, tri, V, T, K, ws, pos, quadrics, remap, root, out, totals,
                    label="remesh_collapse_apply")
            tri = out[:int(totals[1].item())]
            record("collapse", k_edges, k_xopt)
            info["n_collapsed"][-1] += K
        raise AssertionError("unreachable")

    def flip_phase() -> int:
        V, T = pos.shape[0], tri.shape[0]
        owner = torch.empty(V, device=dev, dtype=torch.int64)
        for rnd in range(_lib.TT_REMESH_MAX_ROUNDS + 1):
            tp = _RemeshTopology(tri, V, nbr=True, edge_fe=True)
            E = tp.E
            state, cd, faces = torch.empty(E, **u8), torch.empty((E, 2), **i32), torch.empty((E, 2), **i32)
            _launch("tt_remesh_flip_select", pos, tri, tp.edges, tp.edge_fe, tp.nbr_ptr, tp.nbr_col, tp.locked, V, T, E,
                    hi2, rnd, state, cd, faces, owner, label="remesh_flip_select")
            kept = (state == 2).nonzero().reshape(-1)  # the round's read-back
            K = int(kept.shape[0])
            if K == 0:
                return rnd
            if rnd == _lib.TT_REMESH_MAX_ROUNDS:
                info["rounds_capped"] = True
                return rnd
            _launch("tt_remesh_flip_apply", tp.edges, cd, faces, state, V, T, E, tri, label="remesh_flip_apply")
            record("flip", tp.edges[kept].contiguous(), cd[kept].contiguous())
            info["n_flipped"][-1] += K
        raise AssertionError("unreachable")

    def move_phase() -> None:
        nonlocal pos
        V, T = pos.shape[0], tri.shape[0]
        tp = _RemeshTopology(tri, V, nbr=True, vf=True)
        q, movable, new = torch.empty((V, 3), **f32), torch.empty(V, **u8), torch.empty((V, 3), **f32)
        _launch("tt_remesh_relax", pos, tri, tp.nbr_ptr, tp.nbr_col, tp.vf_ptr, tp.vf_col, tp.locked, V, T, tp.E, q,
                movable, label="remesh_relax")
        _, face, bary = mesh_closest_point(q, tg)
        _launch("tt_remesh_place", pos, face, bary, tg.v_pos, tg.t_pos_idx, movable, V, tg.v_pos.shape[0], tg.n_faces,
                new, label="remesh_place")
        rev, cur = [torch.zeros(V, **u8), torch.empty(V, **u8)], 0
        while True:  # the reverted set only grows: at most V steps, in practice one or two
            _launch("tt_remesh_fold_flag", pos, new, tri, rev[cur], V, T, rev[1 - cur], count, label="remesh_fold_flag")
            if int(count.item()) == 0:
                break
            cur = 1 - cur
        _launch("tt_remesh_revert", pos, rev[cur], V, new, label="remesh_revert")
        info["n_reverted"].append(int(rev[cur].sum().item()))
        pos = new
        if return_trace:  # a copy: the next collapse round writes into pos
            record("move", new.clone(), rev[cur])

    for _ in range(iterations):
        split_phase()
        info["n_collapsed"].append(0)
        info["n_flipped"].append(0)
        info["rounds"].append({"collapse": collapse_phase(), "flip": flip_phase()})
        move_phase()
    split_phase()
    changed = sum(info["n_split"]) + sum(info["n_collapsed"]) + sum(info["n_flipped"]) > 0
    if not changed and bool(torch.equal(pos, v_pos)):
        v_out, t_out = v_pos, t_pos_idx
    else:
        V, T = pos.shape[0], tri.shape[0]
        ws = _workspace("tt_decimate_workspace_bytes", V, T, device=dev)
        _launch("tt_decimate_emit_count", tri, V, T, ws, totals, label="remesh_emit_count")
        v_out = torch.empty((int(totals[0].item()), 3), **f32)
        t_out = torch.empty((T, 3), **i32)
        _launch("tt_decimate_emit", pos, tri, torch.arange(V, **i32), V, T, ws, v_out, t_out, torch.empty(V, **i32),
                label="remesh_emit")
        info["unchanged"] = False
    _, info["source_face"], info["source_bary"] = mesh_closest_point(v_out, tg)
    return v_out, t_out, info


# ---------------------------------------------------------------------------------------------------------------
# point-to-mesh distance (include/tt_abi.h, "point-to-mesh distance"): closest point on a triangle mesh, surface samples
def dist_default_grid(n_faces: int) -> int:
    """The grid a TriangleGrid takes when the caller names none: clamp(ceil(sqrt(T) / 8), 1, TT_DIST_MAX_GRID), about two (cell, triangle) pairs
    per triangle; the fastest of the grids measured on both loads of profiles/mesh_distance.json."""
    return int(min(max(int(np.ceil(np.sqrt(float(n_faces)) / 8.0)), 1), _lib.TT_DIST_MAX_GRID))


def _chk_mesh(v_pos: Tensor, t_pos_idx: Tensor, what: str) -> Tuple[Tensor, Tensor]:
    """A mesh as the tt_dist_* kernels take it: v_pos (V,3) fp32 detached, t_pos_idx (T,3) int32, V, T >= 1 and within
    TT_MESH_MAX_ITEMS.  The index range and the positions' finiteness are the caller's one read-back."""
    v_pos = _chk(v_pos, "v_pos", (None, 3)).detach()
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    if v_pos.shape[0] < 1 or t_pos_idx.shape[0] < 1:
        raise ValueError(f"{what}: the mesh needs at least one vertex and one face, got V={v_pos.shape[0]}, "
                         f"T={t_pos_idx.shape[0]}")
    _chk_size(f"mesh too large for {what}", V=v_pos.shape[0], T=t_pos_idx.shape[0])
    return v_pos, t_pos_idx.int().contiguous()


class TriangleGrid:
    """The uniform grid of a triangle mesh for ops.mesh_closest_point / ops.point_mesh_distance2, built once per mesh
    (tt_dist_build_count / _fill; one 8-byte read-back for the number of (cell, triangle) pairs): 48-byte triangle
    records, the cell -> triangle CSR (cell_ptr, cell_tri), the cube (lo, ext, h, inv_h) and G; keeps the detached
    v_pos and the int32 t_pos_idx it was built from.  grid=None takes dist_default_grid(T); grid=1 is brute force.
    The answer of a query does not depend on the grid, only its cost does."""

    def __init__(self, v_pos: Tensor, t_pos_idx: Tensor, grid: Optional[int] = None):
        if grid is not None:
            if isinstance(grid, bool) or not isinstance(grid, int):
                raise TypeError(f"grid must be an int or None, got {type(grid).__name__}")
            if not 1 <= grid <= _lib.TT_DIST_MAX_GRID:
                raise ValueError(f"grid must be in [1, {_lib.TT_DIST_MAX_GRID}], got {grid}")
        self.v_pos, self.t_pos_idx = _chk_mesh(v_pos, t_pos_idx, "tt_dist_*")
        V, T, dev = self.v_pos.shape[0], self.t_pos_idx.shape[0], self.v_pos.device
        G = dist_default_grid(T) if grid is None else grid
        _chk_size("grid too large for tt_dist_*", cells=G ** 3 + 1)
        lo, hi, ext = self._box = _mesh_box(self.v_pos, self.t_pos_idx)
        h, inv_h = ext / np.float32(G), (np.float32(G) / ext if ext > 0 else np.float32(0))
        if not np.isfinite(inv_h) or (ext > 0 and not h > 0):
            raise ValueError(f"the mesh's extent {float(ext)} is too small for grid {G} in fp32")
        self.G, self.lo, self.ext, self.h, self.inv_h = G, [float(x) for x in lo], float(ext), float(h), float(inv_h)
        ws = _workspace("tt_dist_workspace_bytes", G, device=dev)
        self.records = torch.empty((T, 3, 4), device=dev, dtype=torch.float32)
        self.cell_ptr = torch.empty(G ** 3 + 1, device=dev, dtype=torch.int32)
        total = torch.empty(1, device=dev, dtype=torch.int64)
        _launch("tt_dist_build_count", self.v_pos, self.t_pos_idx, V, T, *_box_args(self), ws, self.records,
                self.cell_ptr, total, label="dist_build_count")
        self.M = int(total.item())
        _chk_size(f"grid {G} gives too many (cell, triangle) pairs for tt_dist_*: use a coarser grid", M=self.M)
        self.cell_tri = torch.empty(self.M, device=dev, dtype=torch.int32)
        _launch("tt_dist_build_fill", self.records, T, *_box_args(self), ws, self.cell_ptr, self.M, self.cell_tri,
                label="dist_build_fill")

    @property
    def n_faces(self) -> int:
        return self.t_pos_idx.shape[0]


def _box_args(tg: TriangleGrid) -> tuple:  # the cube as tt_dist_build_* and tt_dist_keys take it
    return (tg.G, *tg.lo, tg.ext, tg.inv_h)


def _grid_args(tg: TriangleGrid) -> tuple:  # the built grid as tt_dist_query and tt_ray_* take it
    return (tg.records, tg.cell_ptr, tg.cell_tri, tg.n_faces, tg.M, tg.G, *tg.lo, tg.ext, tg.h, tg.inv_h)


def _chk_built(given, cls, name: str):
    if not isinstance(given, cls):
        raise TypeError(f"{name} must be a {cls.__name__}, got {type(given).__name__}")
    return given


def _given_or_built(given, cls, name: str, v_pos: Tensor, t_pos_idx: Tensor):
    """`given` (a TriangleGrid / WindingTree the caller built for this mesh) or, for None, a new cls(v_pos, t_pos_idx)."""
    if given is None:
        return cls(v_pos, t_pos_idx)
    if _chk_built(given, cls, name).v_pos.shape != v_pos.shape:
        raise ValueError(f"{name} was built for {given.v_pos.shape[0]} vertices, v_pos has {v_pos.shape[0]}")
    return given


def _cell_order(points: Tensor, tg: TriangleGrid) -> Tensor:
    """The `order` of tt_dist_query / tt_ray_cast: `points` (N,3), N >= 1, by cell key (tt_dist_keys, one stable sort)."""
    keys = torch.empty(points.shape[0], device=points.device, dtype=torch.int64)
    _launch("tt_dist_keys", points, points.shape[0], *_box_args(tg), keys, label="dist_keys")
    return torch.sort(keys, stable=True)[1]


@torch.no_grad()
def mesh_closest_point(points: Tensor, tg: TriangleGrid, cell_order: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """The closest point of the mesh in `tg` to every row of points (N,3) fp32 (tt_dist_query): d2 (N,) fp32 the squared
    distance, face (N,) int32 the lexicographic minimum of (d2, face) over all triangles (equal distance: the smaller
    face index), bary (N,3) fp32 with the closest point = sum_k bary[k] v_pos[t_pos_idx[face, k]].  Exact, and bit for
    bit independent of the grid, the order of the points and the launch.  A row with a coordinate that is not finite
    gives (NaN, -1, 0).  cell_order=True serves the points in the order of their cell key (tt_dist_keys, one stable
    torch.sort) and writes the rows back in the caller's order: the same answer, a different memory access pattern."""
    _chk_built(tg, TriangleGrid, "tg")
    points = _chk(points, "points", (None, 3)).detach()
    N, dev = points.shape[0], points.device
    _chk_size("too many points for tt_dist_query", N=N)
    d2 = torch.empty(N, device=dev, dtype=torch.float32)
    face = torch.empty(N, device=dev, dtype=torch.int32)
    bary = torch.empty((N, 3), device=dev, dtype=torch.float32)
    if N == 0:
        return d2, face, bary
    order = _cell_order(points, tg) if cell_order else None
    _launch("tt_dist_query", points, order, N, *_grid_args(tg), d2, face, bary, label="dist_query")
    return d2, face, bary


class _PointMeshDistance2Fn(torch.autograd.Function):
    """d2 of ops.mesh_closest_point with the backward tt_dist_bwd: the nearest face and its barycentrics are fixed
    (envelope theorem), d(d2)/dp = 2 (p - c), d(d2)/dv_k = -2 b_k (p - c)."""

    @staticmethod
    def forward(ctx, points, v_pos, tg):
        d2, face, bary = mesh_closest_point(points, tg)
        ctx.save_for_backward(points.detach(), v_pos.detach(), face, bary)
        ctx.tri = tg.t_pos_idx
        return d2

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_d2):
        points, v_pos, face, bary = ctx.saved_tensors
        need_p, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_d2 is None or not (need_p or need_v):
            return None, None, None
        N, V, T = points.shape[0], v_pos.shape[0], ctx.tri.shape[0]
        g_p = torch.empty_like(points) if need_p else None
        g_v = torch.zeros_like(v_pos) if need_v else None
        if N > 0:
            _launch("tt_dist_bwd", points, v_pos, ctx.tri, face, bary, g_d2.contiguous(), N, V, T, g_p, g_v,
                    label="dist_bwd")
        return g_p, g_v, None


def point_mesh_distance2(points: Tensor, v_pos: Tensor, t_pos_idx: Tensor, tg: Optional[TriangleGrid] = None) -> Tensor:
    """Squared distance d2 (N,) of every row of points (N,3) to the mesh (v_pos, t_pos_idx), differentiable w.r.t.
    points and v_pos (the nearest face fixed).  `tg`: a TriangleGrid of the same mesh to reuse; else one is built here
    from the detached positions.  A point that is not finite gives NaN and no gradient."""
    points = _chk(points, "points", (None, 3))
    v_pos = _chk(v_pos, "v_pos", (None, 3))
    tg = _given_or_built(tg, TriangleGrid, "tg", v_pos, t_pos_idx)
    return _PointMeshDistance2Fn.apply(points, v_pos, tg)


def _chk_spacing(spacing) -> float:
    try:
        spacing = float(spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be a finite positive number, got {spacing!r}") from None
    if not 0.0 < spacing < float("inf"):
        raise ValueError(f"spacing must be a finite positive number, got {spacing!r}")
    return spacing


@torch.no_grad()
def mesh_surface_samples(v_pos: Tensor, t_pos_idx: Tensor, spacing: float) -> Tuple[Tensor, Tensor]:
    """A deterministic sample set of the surface with every surface point within `spacing` of a sample
    (tt_dist_sample_*): face f with longest edge L_f gets the (k+1)(k+2)/2 lattice points of k = max(1, ceil(L_f /
    spacing)) subdivisions, face-major.  points (S,3) fp32, face (S,) int32.  More than TT_DIST_MAX_SAMPLES samples is a
    ValueError raised before they are allocated.  Shared edges and vertices are sampled more than once."""
    spacing = _chk_spacing(spacing)
    v_pos, tri = _chk_mesh(v_pos, t_pos_idx, "tt_dist_sample_*")
    V, T, dev = v_pos.shape[0], tri.shape[0], v_pos.device
    ws = _workspace("tt_dist_sample_workspace_bytes", T, device=dev)
    offs = torch.empty(T + 1, device=dev, dtype=torch.int64)
    _launch("tt_dist_sample_count", v_pos, tri, V, T, spacing, ws, offs, label="dist_sample_count")
    lo, hi, S = (int(x) for x in torch.cat([_minmax(tri).long(), offs[T:]]).cpu())  # one read-back
    _chk_range("t_pos_idx", lo, hi, V)
    if S > _lib.TT_DIST_MAX_SAMPLES:
        raise ValueError(f"spacing {spacing} needs S = {S} samples or more, above TT_DIST_MAX_SAMPLES = "
                         f"{_lib.TT_DIST_MAX_SAMPLES}: use a larger spacing")
    points = torch.empty((S, 3), device=dev, dtype=torch.float32)
    face = torch.empty(S, device=dev, dtype=torch.int32)
    _launch("tt_dist_sample_emit", v_pos, tri, offs, V, T, spacing, S, points, face, label="dist_sample_emit")
    return points, face


@torch.no_grad()
def one_sided_distance(samples: Tensor, tg: TriangleGrid) -> dict:
    """{max, mean, rms, argmax_point} of the distance from `samples` (S,3) to the mesh in `tg`, over the samples as
    they are (not area-weighted); one read-back."""
    d = mesh_closest_point(samples, tg)[0].sqrt()
    i = torch.argmax(d)
    row = torch.cat([d[i].reshape(1), d.mean().reshape(1), (d * d).mean().sqrt().reshape(1), samples[i]]).double().cpu()
    return {"max": float(row[0]), "mean": float(row[1]), "rms": float(row[2]),
            "argmax_point": tuple(float(x) for x in row[3:6])}


# ---------------------------------------------------------------------------------------------------------------
# winding number (include/tt_abi.h, "winding number"): inside test, signed distance
def wind_default_levels(n_faces: int) -> int:
    """The octree depth a WindingTree takes when the caller names none: the smallest L with 6 * 4^L >= T, at most
    TT_WIND_MAX_LEVELS -- clamp(ceil(log4(T / 6)), 0, 6), about two faces per occupied leaf.  The fastest depth of the
    sweep in profiles/mesh_winding.json on every mesh measured (1.8 k to 473 k faces): the walk is bound by its
    dependent node loads and a leaf's pair loop, so deeper wins until leaves hold a face or two."""
    return next((L for L in range(_lib.TT_WIND_MAX_LEVELS) if 6 * 4 ** L >= n_faces), _lib.TT_WIND_MAX_LEVELS)


def _chk_beta(beta) -> float:
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not beta > 0:  # NaN fails the comparison
        raise ValueError(f"beta must be a positive number, got {beta!r}")
    return float(beta)


class WindingTree:
    """The dipole octree of a triangle mesh for ops.mesh_winding_number / mesh_contains / mesh_signed_distance, built
    once per mesh (tt_wind_face_keys, one stable sort, tt_wind_build; one read-back for the box and the index range):
    `records` (T,3,4) in face order (the exact sum), `sorted_records` in (Morton key, face) order with `face_order`
    (T,) int32 the face of every sorted row, `leaf_ptr` (8^L + 1) int32, `nodes` (n_nodes, 8) fp32 = N, r, c, A per
    node (r = -1: empty), level l from row (8^l - 1) / 7 on.  levels=None takes wind_default_levels(T); levels=0 is a
    root whose one leaf holds every face.  Keeps the detached v_pos and the int32 t_pos_idx it was built from."""

    def __init__(self, v_pos: Tensor, t_pos_idx: Tensor, levels: Optional[int] = None):
        if levels is not None:
            if isinstance(levels, bool) or not isinstance(levels, int):
                raise TypeError(f"levels must be an int or None, got {type(levels).__name__}")
            if not 0 <= levels <= _lib.TT_WIND_MAX_LEVELS:
                raise ValueError(f"levels must be in [0, {_lib.TT_WIND_MAX_LEVELS}], got {levels}")
        self.v_pos, self.t_pos_idx = _chk_mesh(v_pos, t_pos_idx, "tt_wind_*")
        V, T, dev = self.v_pos.shape[0], self.t_pos_idx.shape[0], self.v_pos.device
        L = wind_default_levels(T) if levels is None else levels
        lo, _, ext = _mesh_box(self.v_pos, self.t_pos_idx)
        inv_h = np.float32(1 << L) / ext if ext > 0 else np.float32(0)
        if not np.isfinite(inv_h):
            raise ValueError(f"the mesh's extent {float(ext)} is too small for {L} levels in fp32")
        self.L, self.lo, self.ext, self.inv_h = L, [float(x) for x in lo], float(ext), float(inv_h)
        self.records = torch.empty((T, 3, 4), device=dev, dtype=torch.float32)
        keys = torch.empty(T, device=dev, dtype=torch.int64)
        _launch("tt_wind_face_keys", self.v_pos, self.t_pos_idx, V, T, L, *self.lo, self.ext, self.inv_h, self.records,
                keys, label="wind_face_keys")
        self.leaf_ptr, self.face_order = _csr(keys, None, 8 ** L, T)
        self.sorted_records = self.records if L == 0 else self.records[self.face_order.long()].contiguous()
        self.nodes = torch.empty((int(_lib.load().tt_wind_node_count(L)), 8), device=dev, dtype=torch.float32)
        _launch("tt_wind_build", self.sorted_records, self.leaf_ptr, T, L, self.nodes, label="wind_build")

    @property
    def n_faces(self) -> int:
        return self.t_pos_idx.shape[0]

    def level(self, l: int) -> Tensor:
        """The (8^l, 8) rows of level l of the node table."""
        base = (8 ** l - 1) // 7
        return self.nodes[base:base + 8 ** l]

    def node_ranges(self, l: int) -> Tensor:
        """(8^l, 2) int32: the range of sorted faces under every node of level l."""
        ptr = self.leaf_ptr[::8 ** (self.L - l)]
        return torch.stack([ptr[:-1], ptr[1:]], 1)


def _wind_records(v_pos: Tensor, t_pos_idx: Tensor) -> Tensor:
    """The (T,3,4) records of a mesh in face order, which is all the exact sum reads: tt_wind_face_keys with a box
    without extent (every key 0, dropped); one read-back for the index range.  No sort, no node table."""
    v_pos, tri = _chk_mesh(v_pos, t_pos_idx, "tt_wind_*")
    V, T = v_pos.shape[0], tri.shape[0]
    lo, hi = (int(x) for x in _minmax(tri).cpu())
    _chk_range("t_pos_idx", lo, hi, V)
    records = torch.empty((T, 3, 4), device=v_pos.device, dtype=torch.float32)
    _launch("tt_wind_face_keys", v_pos, tri, V, T, 0, 0.0, 0.0, 0.0, 0.0, 0.0, records,
            torch.empty(T, device=v_pos.device, dtype=torch.int64), label="wind_face_keys")
    return records


def _wind_tree(v_pos_or_tree, t_pos_idx, levels: Optional[int] = None) -> WindingTree:
    if isinstance(v_pos_or_tree, WindingTree):
        if t_pos_idx is not None:
            raise ValueError("t_pos_idx goes with v_pos, not with a WindingTree")
        return v_pos_or_tree
    if not isinstance(v_pos_or_tree, torch.Tensor):
        raise TypeError(f"expected v_pos or a WindingTree, got {type(v_pos_or_tree).__name__}")
    if t_pos_idx is None:
        raise TypeError("v_pos needs t_pos_idx")
    return WindingTree(v_pos_or_tree, t_pos_idx, levels)


@torch.no_grad()
def mesh_winding_number(points: Tensor, v_pos_or_tree, t_pos_idx: Optional[Tensor] = None, beta: float = 2.0,
                        exact: bool = False, cell_order: bool = False) -> Tensor:
    """The generalized winding number w (N,) fp32 of the mesh about every row of points (N,3) fp32: 1 inside and 0
    outside an outward-oriented closed surface.  `v_pos_or_tree`: a WindingTree to reuse, or v_pos with t_pos_idx (a tree
    is built here; for exact=True only the face records, no tree).  exact=True sums every face (tt_wind_exact): bit for bit independent
    of the launch and the order of the points.  Otherwise the tree's dipole approximation (tt_wind_fast): nodes
    farther than beta bounding radii contribute N . (c - p) / (4 pi |c - p|^3); for a given (levels, beta) as
    independent.  cell_order=True serves the points in the order of their leaf cell (tt_wind_point_keys, one stable
    sort): the same bits.  A row with a coordinate that is not finite gives NaN."""
    beta = _chk_beta(beta)
    if exact and isinstance(v_pos_or_tree, torch.Tensor) and t_pos_idx is not None:
        tree, records = None, _wind_records(v_pos_or_tree, t_pos_idx)
    else:
        tree = _wind_tree(v_pos_or_tree, t_pos_idx)
        records = tree.records
    points = _chk(points, "points", (None, 3)).detach()
    N, dev = points.shape[0], points.device
    _chk_size("too many points for tt_wind_*", N=N)
    w = torch.empty(N, device=dev, dtype=torch.float32)
    if N == 0:
        return w
    if exact:
        _launch("tt_wind_exact", points, N, records, records.shape[0], w, label="wind_exact")
        return w
    order = None
    if cell_order:
        keys = torch.empty(N, device=dev, dtype=torch.int64)
        _launch("tt_wind_point_keys", points, N, tree.L, *tree.lo, tree.ext, tree.inv_h, keys, label="wind_point_keys")
        order = torch.sort(keys, stable=True)[1]
    _launch("tt_wind_fast", points, order, N, tree.sorted_records, tree.leaf_ptr, tree.nodes, tree.n_faces, tree.L,
            beta, w, label="wind_fast")
    return w


def mesh_contains(points: Tensor, v_pos_or_tree, t_pos_idx: Optional[Tensor] = None, beta: float = 2.0,
                  exact: bool = False, cell_order: bool = False) -> Tensor:
    """(N,) bool: w > 0.5 of ops.mesh_winding_number (a row that is not finite: False)."""
    return mesh_winding_number(points, v_pos_or_tree, t_pos_idx, beta, exact, cell_order) > 0.5


class _SignedRootFn(torch.autograd.Function):
    """sign * sqrt(d2) with the sign fixed; the gradient w.r.t. d2 is sign / (2 d), and exactly 0 where d == 0 (so the
    chain through d(d2)/dp = 2 (p - c) gives sign (p - c) / d, never inf)."""

    @staticmethod
    def forward(ctx, d2, sign):
        d = d2.sqrt()
        ctx.save_for_backward(d, sign)
        return sign * d

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        d, sign = ctx.saved_tensors
        return torch.where(d > 0, g * sign / (2 * d), torch.zeros_like(d)), None


def mesh_signed_distance(points: Tensor, v_pos: Tensor, t_pos_idx: Tensor, tg: Optional[TriangleGrid] = None,
                         tree: Optional[WindingTree] = None, beta: float = 2.0) -> Tensor:
    """Signed distance (N,) of every row of points (N,3) to the mesh, in the field's convention (negative inside):
    sign * sqrt(d2) with d2 of ops.point_mesh_distance2 and sign = -1 where ops.mesh_winding_number > 0.5, else +1.
    Differentiable w.r.t. points and v_pos with the sign and the nearest face fixed: the gradient w.r.t. a point is
    sign (p - c) / d, and exactly 0 where d == 0.  `tg`, `tree`: a TriangleGrid / WindingTree of the same mesh to
    reuse.  A point that is not finite gives NaN."""
    beta = _chk_beta(beta)
    points = _chk(points, "points", (None, 3))
    v_pos = _chk(v_pos, "v_pos", (None, 3))
    tree = _given_or_built(tree, WindingTree, "tree", v_pos, t_pos_idx)
    d2 = point_mesh_distance2(points, v_pos, t_pos_idx, tg)
    inside = mesh_winding_number(points, tree, beta=beta) > 0.5
    sign = torch.where(inside, -torch.ones_like(d2), torch.ones_like(d2)).detach()
    return _SignedRootFn.apply(d2, sign)


# ---------------------------------------------------------------------------------------------------------------
# mesh to SDF grid (include/tt_abi.h, "mesh to SDF grid"): the clamped signed distance on a regular grid
SDFGRID_SIGN_BAND = 1.0 + 2.0 ** -10  # cells: corners nearer than this carry their own sign even in a narrower band


def _chk_sdf_grid_args(resolution, band, default_bounds: bool) -> Tuple[int, float]:
    """(R, band) of ops.mesh_sdf_grid, checked before any tensor is looked at."""
    if isinstance(resolution, bool) or not isinstance(resolution, int):
        raise TypeError(f"resolution must be an int, got {type(resolution).__name__}")
    if not 2 <= resolution <= _lib.TT_SDFGRID_MAX_RES:
        raise ValueError(f"resolution must be in [2, {_lib.TT_SDFGRID_MAX_RES}], got {resolution}")
    if isinstance(band, bool) or not isinstance(band, (int, float)) or not 0 < band <= _lib.TT_SDFGRID_MAX_BAND:
        raise ValueError(f"band must be in (0, {_lib.TT_SDFGRID_MAX_BAND}] grid cells, got {band!r}")
    need = 2 * (int(np.ceil(band)) + 1) + 2
    if default_bounds and resolution < need:
        raise ValueError(f"resolution {resolution} leaves no room for band {band} around the mesh: "
                         f"bounds=None needs resolution >= 2 * (ceil(band) + 1) + 2 = {need}")
    return resolution, float(band)


def sdf_grid_bounds(box_lo, box_hi, resolution: int, band: float) -> Tuple[np.ndarray, np.float32]:
    """(lo (3,) fp32, h fp32) of the default grid of ops.mesh_sdf_grid: the cube about the centre of the box (box_lo,
    box_hi) in which the box's largest extent spans R - 1 - 2 m cells, m = ceil(band) + 1, so that at least m cells
    lie between the box and every face of the grid (h carries a relative 2^-20 on top against its own rounding)."""
    lo, hi = np.asarray(box_lo, np.float64), np.asarray(box_hi, np.float64)
    m = int(np.ceil(band)) + 1
    ext = float((hi - lo).max())
    if not ext > 0.0:
        raise ValueError("the mesh has no extent: give bounds=(lo, side)")
    h = ext * (1.0 + 2.0 ** -20) / (resolution - 1 - 2 * m)
    return ((lo + hi) * 0.5 - h * (resolution - 1) * 0.5).astype(np.float32), np.float32(h)


@torch.no_grad()
def mesh_sdf_grid(v_pos: Tensor, t_pos_idx: Tensor, resolution: int, band: float = 3.0, bounds=None,
                  tg: Optional[TriangleGrid] = None, tree: Optional[WindingTree] = None, beta: float = 2.0
                  ) -> Tuple[Tensor, dict]:
    """The signed distance of the mesh on a regular grid, clamped to a band: level (R,R,R) fp32 in the layout
    ops.marching_cubes reads, negative inside, and info = {lo (3,) fp32 tensor, h, tau (Python floats holding fp32
    values), face (R,R,R) int32, band_corners, sign_corners, candidates}.  NOT differentiable.  (tt_sdfgrid_*; include/tt_abi.h,
    "mesh to SDF grid".)

    Corner (i,j,k) is the fp32 point lo + (i,j,k) * h, a product then a sum, each rounded: torch's values for
    lo + idx.float() * h.  bounds=(lo, side): the cube from lo (three numbers) with h = side / (R - 1) in fp32.
    bounds=None: the cube about the mesh's bounding box with at least ceil(band) + 1 cells between the box and every
    grid face (sdf_grid_bounds), which needs R >= 2 * (ceil(band) + 1) + 2.

    With tau = band * h in fp32, a corner with d = sqrt(d2) < tau is a band corner: d2 and info["face"] are
    ops.mesh_closest_point's there, bit for bit: a scatter kernel (triangles to the corners of their grown boxes,
    integer atomics) finds the corners near the surface, and the closest-point query itself runs on those alone --
    the same device function inlined into the scatter differs from the query in the last bit.  level =
    sgn * d with sgn = -1 where ops.mesh_winding_number(..., beta) > 0.5, else +1 -- the rule of
    ops.mesh_signed_distance.  Every other corner has level = +-tau and face = -1.  Its sign is that of the nearest
    SIGN corner below it along the last axis in its (i,j) row, + when there is none; the sign corners are the corners
    with d < max(band, 1 + 2^-10) * h, which evaluate their own winding number.  For band >= 1 + 2^-10 they are the
    band corners; a narrower band alone could not tell the inside of a closed mesh, because the first corner behind a
    crossing (d <= h) need not be in it.  For a closed input level == mesh.signed_distance(corners).clamp(-tau, tau)
    at every corner.  An open input is closed along w = 1/2 where sign corners see it, and rows keep the sign they
    last saw.  The result does not depend on the order of the triangles or the launch (integer atomics only).

    `tg`, `tree`: a TriangleGrid / WindingTree of the same mesh to reuse.  R <= TT_SDFGRID_MAX_RES, 0 < band <=
    TT_SDFGRID_MAX_BAND; a vertex that is not finite is a ValueError (as for TriangleGrid).  Read-backs: the box (when
    a grid is built here), the number of candidates, the two counts of info (band_corners, sign_corners; `candidates`
    is what the scatter selected)."""
    R, band = _chk_sdf_grid_args(resolution, band, bounds is None)
    beta = _chk_beta(beta)
    if bounds is not None:
        try:
            b_lo, side = bounds
            b_lo = np.asarray([float(x) for x in b_lo], np.float32)
            side = np.float32(float(side))
        except (TypeError, ValueError):
            raise ValueError(f"bounds must be (lo, side) with three numbers and a number, got {bounds!r}") from None
        if b_lo.shape != (3,) or not np.isfinite(b_lo).all() or not (np.isfinite(side) and side > 0):
            raise ValueError(f"bounds must be (lo, side) with finite lo (3) and side > 0, got {bounds!r}")
    v_pos = _chk(v_pos, "v_pos", (None, 3)).detach()
    tg = _given_or_built(tg, TriangleGrid, "tg", v_pos, t_pos_idx)
    tree = _given_or_built(tree, WindingTree, "tree", v_pos, t_pos_idx)
    dev, T = v_pos.device, tg.n_faces
    if bounds is None:
        lo, h = sdf_grid_bounds(tg._box[0], tg._box[1], R, band)
    else:
        lo, h = b_lo, side / np.float32(R - 1)
    tau, sign_tau = np.float32(band) * h, np.float32(max(band, SDFGRID_SIGN_BAND)) * h
    if not (np.isfinite(h) and h > 0 and tau > 0 and np.isfinite(sign_tau)):
        raise ValueError(f"the grid step {float(h)} is not usable in fp32")
    geo = (*(float(x) for x in lo), float(h), float(tau), float(sign_tau))
    ws = _workspace("tt_sdfgrid_workspace_bytes", R, T, device=dev)
    counts = torch.empty(2, device=dev, dtype=torch.int32)
    _launch("tt_sdfgrid_scatter", tg.records, T, R, *geo, ws, counts, label="sdfgrid_scatter")
    n_cand = int(counts[1].item())
    corner = torch.empty(n_cand, device=dev, dtype=torch.int32)
    points = torch.empty((n_cand, 3), device=dev, dtype=torch.float32)
    _launch("tt_sdfgrid_corners", R, T, *geo, ws, n_cand, corner, points, label="sdfgrid_corners")
    d2, nearest, _ = mesh_closest_point(points, tg)
    w = mesh_winding_number(points, tree, beta=beta)
    level = torch.empty((R, R, R), device=dev, dtype=torch.float32)
    face = torch.empty((R, R, R), device=dev, dtype=torch.int32)
    _launch("tt_sdfgrid_finish", R, T, float(tau), float(sign_tau), ws, corner, d2, nearest, w, n_cand, level, face,
            label="sdfgrid_finish")
    d = d2.sqrt()
    n_band, n_sign = (int(x) for x in torch.stack([(d < float(tau)).sum(), (d < float(sign_tau)).sum()]).cpu())
    return level, {"lo": torch.from_numpy(lo.copy()).to(dev), "h": float(h), "tau": float(tau), "face": face,
                   "band_corners": n_band, "sign_corners": n_sign, "candidates": n_cand}


# ---------------------------------------------------------------------------------------------------------------
# ray casting (include/tt_abi.h, "ray casting"): closest hit, any hit, depth with a gradient, ambient occlusion
def _chk_t_max(t_max, name: str = "t_max") -> float:
    try:
        t_max = float(t_max)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number >= 0 (inf allowed), got {t_max!r}") from None
    if not t_max >= 0.0:
        raise ValueError(f"{name} must be a number >= 0 (inf allowed), got {t_max!r}")
    return t_max


def _chk_rays(origins: Tensor, dirs: Tensor, tg, what: str) -> Tuple[Tensor, Tensor]:
    _chk_built(tg, TriangleGrid, "tg")
    origins = _chk(origins, "origins", (None, 3)).detach()
    dirs = _chk(dirs, "dirs", (origins.shape[0], 3)).detach()
    _chk_size(f"too many rays for {what}", N=origins.shape[0])
    return origins, dirs


@torch.no_grad()
def mesh_ray_cast(origins: Tensor, dirs: Tensor, tg: TriangleGrid, t_max: float = float("inf"),
                  cell_order: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """The closest hit of every ray origins[i] + t dirs[i] (both (N,3) fp32; dirs of any non-zero length, t in units of
    dirs) with the mesh in `tg`, 0 <= t <= t_max (tt_ray_cast): t (N,) fp32, face (N,) int32, bary (N,3) fp32 with the
    hit point = sum_k bary[k] v_pos[t_pos_idx[face, k]].  The answer is the lexicographic minimum of (t, face) over all
    triangles of a watertight pair test (both sides of a face are hit), bit for bit independent of the grid, the order
    of the rays and the launch.  A miss is (inf, -1, 0); a row that is not finite or has a zero direction (NaN, -1, 0).
    cell_order=True serves the rays in the order of their origins' cell keys: the same answer."""
    origins, dirs = _chk_rays(origins, dirs, tg, "tt_ray_cast")
    t_max = _chk_t_max(t_max)
    N, dev = origins.shape[0], origins.device
    t = torch.empty(N, device=dev, dtype=torch.float32)
    face = torch.empty(N, device=dev, dtype=torch.int32)
    bary = torch.empty((N, 3), device=dev, dtype=torch.float32)
    if N == 0:
        return t, face, bary
    order = _cell_order(origins, tg) if cell_order else None
    _launch("tt_ray_cast", origins, dirs, order, N, t_max, *_grid_args(tg), t, face, bary, label="ray_cast")
    return t, face, bary


@torch.no_grad()
def mesh_ray_occluded(origins: Tensor, dirs: Tensor, tg: TriangleGrid, t_max: float = float("inf")) -> Tensor:
    """(N,) bool: whether ray i hits any triangle of the mesh in `tg` at 0 <= t <= t_max (tt_ray_any: the walk of
    mesh_ray_cast, left at the first hit).  Equal to mesh_ray_cast(...).face >= 0; a row that is not finite is False."""
    origins, dirs = _chk_rays(origins, dirs, tg, "tt_ray_any")
    t_max = _chk_t_max(t_max)
    N = origins.shape[0]
    hit = torch.empty(N, device=origins.device, dtype=torch.uint8)
    if N > 0:
        _launch("tt_ray_any", origins, dirs, None, N, t_max, *_grid_args(tg), hit, label="ray_any")
    return hit != 0


def ray_mesh_depth(origins: Tensor, dirs: Tensor, v_pos: Tensor, t_pos_idx: Tensor, tg: Optional[TriangleGrid] = None,
                   t_max: float = float("inf")) -> Tensor:
    """t (N,) of mesh_ray_cast against the mesh (v_pos, t_pos_idx), differentiable w.r.t. origins, dirs and v_pos with
    the hit face fixed: the value is the kernel's t; the gradient is that of the plane formula t' = n.(a - o) / n.d,
    n = (b - a) x (c - a), recomputed in torch on the gathered rows (t + (t' - t'.detach())).  Rows that miss are inf
    with zero gradient.  `tg`: a TriangleGrid of the same mesh to reuse."""
    origins = _chk(origins, "origins", (None, 3))
    dirs = _chk(dirs, "dirs", (origins.shape[0], 3))
    v_pos = _chk(v_pos, "v_pos", (None, 3))
    tg = _given_or_built(tg, TriangleGrid, "tg", v_pos, t_pos_idx)
    t, face, _ = mesh_ray_cast(origins, dirs, tg, t_max)
    hit = face >= 0
    idx = tg.t_pos_idx[face.clamp(min=0).long()].long()
    a, b, c = v_pos[idx[:, 0]], v_pos[idx[:, 1]], v_pos[idx[:, 2]]
    n = torch.linalg.cross(b - a, c - a)
    den = (n * dirs).sum(-1)
    tp = (n * (a - origins)).sum(-1) / torch.where(hit, den, torch.ones_like(den))
    return torch.where(hit, t + (tp - tp.detach()), t)


def ao_directions(K: int) -> Tensor:
    """The K local directions of the ambient-occlusion rays, (K,3) fp32 on the CPU: cosine weighted about +z, the same
    for every point.  u1 = (k + 0.5) / K, u2 = the base-2 radical inverse of k, r = sqrt(u1), phi = 2 pi u2, direction
    (r cos phi, r sin phi, sqrt(1 - u1)); numpy float64, rounded once."""
    if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= _lib.TT_RAY_MAX_DIRS:
        raise ValueError(f"the number of rays must be an int in [1, {_lib.TT_RAY_MAX_DIRS}], got {K!r}")
    k = np.arange(K, dtype=np.int64)
    u1 = (k.astype(np.float64) + 0.5) / K
    u2, f, n = np.zeros(K), 0.5, k.copy()
    while n.any():
        u2 += f * (n & 1)
        n >>= 1
        f *= 0.5
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    return torch.from_numpy(np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u1)], 1).astype(np.float32))


def _tg_diagonal(tg: TriangleGrid) -> float:
    """The bounding-box diagonal of the mesh in `tg` from the box its constructor read: fp32 extents, normed in double."""
    lo, hi, _ = tg._box
    return float(np.sqrt(np.sum((hi - lo).astype(np.float64) ** 2)))


@torch.no_grad()
def mesh_ao_hits(points: Tensor, normals: Tensor, tg: TriangleGrid, n_rays: int = 64,
                 max_distance: Optional[float] = None, bias: Optional[float] = None) -> Tensor:
    """hits (N,) int32 of tt_ray_ao: how many of the n_rays rays of ao_directions about normals[i], started at
    points[i] + bias n^, hit the mesh in `tg` within max_distance; -1 for a point or normal that is not finite or a zero
    normal.  Defaults as mesh_ambient_occlusion."""
    _chk_built(tg, TriangleGrid, "tg")
    points = _chk(points, "points", (None, 3)).detach()
    normals = _chk(normals, "normals", (points.shape[0], 3)).detach()
    N, dev = points.shape[0], points.device
    _chk_size("too many points for tt_ray_ao", N=N)
    table = ao_directions(n_rays).to(dev)
    max_distance = _chk_t_max(0.25 * _tg_diagonal(tg) if max_distance is None else max_distance, "max_distance")
    bias = float(1e-3 * _tg_diagonal(tg) if bias is None else bias)
    if not abs(bias) <= 3.0e38:
        raise ValueError(f"bias must be finite, got {bias}")
    hits = torch.empty(N, device=dev, dtype=torch.int32)
    if N > 0:
        _launch("tt_ray_ao", points, normals, table, N, n_rays, bias, max_distance, *_grid_args(tg), hits,
                label="ray_ao")
    return hits


@torch.no_grad()
def mesh_ambient_occlusion(points: Tensor, normals: Tensor, tg: TriangleGrid, n_rays: int = 64,
                           max_distance: Optional[float] = None, bias: Optional[float] = None) -> Tensor:
    """Ambient occlusion (N,) fp32 = 1 - hits / n_rays of points (N,3) with normals (N,3) (any non-zero length) against
    the mesh in `tg` (tt_ray_ao): 1 means open, 0 closed in; cosine-weighted rays (ao_directions) about the normal in the
    frame of Duff et al., started bias off the point, max_distance long.  Defaults: max_distance = 0.25 and bias = 1e-3
    of the mesh's bounding-box diagonal.  A row that is not finite or has a zero normal gives NaN.  Bit for bit
    independent of the grid and the order of the points."""
    hits = mesh_ao_hits(points, normals, tg, n_rays, max_distance, bias)
    ao = 1.0 - hits.float() / float(n_rays)
    return torch.where(hits < 0, torch.full_like(ao, float("nan")), ao)


@torch.no_grad()
def bake_ambient_occlusion(mesh, texture_size: int, n_rays: int = 64, max_distance: Optional[float] = None,
                           bias: Optional[float] = None, rast: Optional[Tensor] = None,
                           occluder: Optional[TriangleGrid] = None) -> Tuple[Tensor, dict]:
    """The ambient-occlusion map (N,N,1) fp32 in [0,1] of `mesh` (a Mesh with UVs): per covered texel of the UV
    rasterisation `rast` (N,N,4) (computed as the exporter does when None) the point interpolated from v_pos and the
    normal interpolated from v_nrm -- flipped to the side of the face's geometric normal where the two disagree, the
    geometric normal itself where the interpolated one vanishes -- go through mesh_ambient_occlusion against `occluder`
    (default mesh.triangle_grid).  Uncovered texels, and texels whose face has no normal at all, are 1: fill them with
    texture_fill.  info = {n_covered, mean (over the covered texels), texel (M,) int64: their flat ids, hits (M,) int32}."""
    from . import raster  # (raster imports this module)
    N = int(texture_size)
    if rast is None:
        rast = uv_rasterize(mesh.v_tex, mesh.t_tex_idx, N)
    rast = _chk(rast, "rast", (N, N, 4))
    tg = mesh.triangle_grid if occluder is None else occluder
    tri = mesh.t_pos_idx.int()
    T = tri.shape[0]
    tid = rast[..., 3].reshape(-1)
    texel = torch.nonzero((tid >= 1) & (tid <= T)).reshape(-1)
    v_pos = mesh.v_pos.detach().float()
    pos = raster.interpolate(v_pos[None], rast[None], tri)[0].reshape(-1, 3)[texel].contiguous()
    nrm = raster.interpolate(mesh.v_nrm.detach().float()[None], rast[None], tri)[0].reshape(-1, 3)[texel]
    fv = v_pos[tri[(tid[texel] - 1).long()].long()]  # (M,3,3)
    geo = torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0])
    nrm = torch.where(((nrm * geo).sum(-1) < 0)[:, None], -nrm, nrm)
    nrm = torch.where((nrm.abs().amax(-1) > 0)[:, None], nrm, geo).contiguous()
    hits = mesh_ao_hits(pos, nrm, tg, n_rays, max_distance, bias)
    ao = torch.where(hits < 0, torch.ones_like(pos[:, 0]), 1.0 - hits.float() / float(n_rays))
    out = torch.ones(N * N, device=rast.device, dtype=torch.float32)
    out[texel] = ao
    mean = float(ao.mean()) if ao.numel() else 1.0
    return out.reshape(N, N, 1), {"n_covered": int(texel.numel()), "mean": mean, "texel": texel, "hits": hits}


# ---------------------------------------------------------------------------------------------------------------
# tangents and normal-map baking (include/tt_abi.h, "tangents and normal-map baking")
_BAKE_GROUPS = {"pos": _lib.TT_BAKE_GROUP_POS, "tex": _lib.TT_BAKE_GROUP_TEX}


@torch.no_grad()
def mesh_tangents(v_pos: Tensor, t_pos_idx: Tensor, v_tex: Tensor, t_tex_idx: Tensor, v_nrm: Tensor,
                  group: str = "pos") -> Tensor:
    """Unit tangents of a UV-mapped mesh, perpendicular to the normals (tt_bake_tangents): the reference's per-face
    tangent (threestudio/models/mesh.py:162-205) summed over the corners of a group, normalised and Gram-Schmidt
    against the group's normal.  group="pos": one per position vertex, (V,3), the reference's Mesh.v_tng;
    group="tex": one per UV vertex, (Vt,3), with the normal of the UV vertex's position vertex -- tangents that split at
    chart seams, what the normal-map bake and the viewer use.  A group without a usable tangent (no corner, a zero sum,
    a tangent parallel to the normal) gets a fixed unit vector perpendicular to its normal where the reference yields
    NaN.  The group -> corner CSR is one stable sort here; each group's corners are added in ascending corner id, so the
    result is bit-identical from call to call.  Inputs are detached; the result never requires grad."""
    if group not in _BAKE_GROUPS:
        raise ValueError(f"group must be 'pos' or 'tex', got {group!r}")
    v_pos = _chk(v_pos.detach(), "v_pos", (None, 3))
    V, dev = v_pos.shape[0], v_pos.device
    v_nrm = _chk(v_nrm.detach(), "v_nrm", (V, 3))
    v_tex = _chk(v_tex.detach(), "v_tex", (None, 2))
    Vt = v_tex.shape[0]
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    T = t_pos_idx.shape[0]
    t_tex_idx = _chk_index(t_tex_idx, "t_tex_idx", 3, T)
    _chk_size("mesh too large for tt_bake_tangents", V=V, Vt=Vt, T=T)
    G = Vt if group == "tex" else V
    out = torch.empty((G, 3), device=dev, dtype=torch.float32)
    if G == 0:
        return out
    if T > 0:
        rng = _minmax(t_pos_idx, t_tex_idx).tolist()  # one read-back
        _chk_range("t_pos_idx", *rng[:2], V)
        _chk_range("t_tex_idx", *rng[2:], Vt)
    key = (t_tex_idx if group == "tex" else t_pos_idx).reshape(-1).long()
    ptr, corner = _csr(key, None, G, 3 * T)  # corner ids 3f + k by (group, corner id)
    _launch("tt_bake_tangents", v_pos, t_pos_idx.int().contiguous(), v_tex, t_tex_idx.int().contiguous(), v_nrm,
            ptr, corner, V, Vt, T, _BAKE_GROUPS[group], out, label="bake_tangents")
    return out


@torch.no_grad()
def bake_project_step(points: Tensor, sdf: Tensor, sdf_grad: Tensor, max_step: float,
                      mask: Optional[Tensor] = None) -> Tensor:
    """One bounded Newton step of `points` (M,3) towards the iso-surface, in place (tt_bake_project): p -= c g with
    c = clamp(sdf / max(|g|^2, 1e-12), -1, 1), scaled down so that the step is no longer than max_step.  sdf (M) or
    (M,1) and sdf_grad (M,3) are the field's values at the points; a point with mask (M) == 0 stays.  Returns points."""
    points = _chk(points, "points", (None, 3))
    M = points.shape[0]
    sdf = _chk(sdf.detach().reshape(-1), "sdf", (M,))
    sdf_grad = _chk(sdf_grad.detach().reshape(-1, 3), "sdf_grad", (M, 3))
    max_step = float(max_step)
    if not 0.0 <= max_step <= 3.0e38:
        raise ValueError(f"max_step must be a finite number >= 0, got {max_step}")
    m = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.numel() != M:
            raise ValueError(f"mask must be a GPU tensor of {M} elements")
        m = (mask.reshape(-1) != 0).to(torch.uint8).contiguous()
    _launch("tt_bake_project", points, sdf, sdf_grad, m, M, max_step, label="bake_project")
    return points


@torch.no_grad()
def bake_encode(rast: Tensor, v_nrm: Tensor, t_pos_idx: Tensor, tng_tex: Tensor, t_tex_idx: Tensor,
                field_nrm: Tensor) -> Tuple[Tensor, Tensor]:
    """The tangent-space normal map of one UV-space rasterisation (tt_bake_encode): per covered texel of rast (H,W,4)
    the field normal field_nrm (H,W,3) (any length; normalised inside) in the frame (t^, b^ = t^ x n^, n^) interpolated
    from tng_tex (Vt,3) and v_nrm (V,3), as 0.5 + 0.5 x; uncovered texels are (0.5, 0.5, 1).  Returns (map (H,W,3),
    counts (2,) int32 on the device = covered texels, covered texels whose field normal points into the face)."""
    rast = _chk(rast, "rast", (None, None, 4))
    H, W = rast.shape[:2]
    v_nrm = _chk(v_nrm.detach(), "v_nrm", (None, 3))
    tng_tex = _chk(tng_tex.detach(), "tng_tex", (None, 3))
    field_nrm = _chk(field_nrm.detach(), "field_nrm", (H, W, 3))
    t_pos_idx = _chk_index(t_pos_idx, "t_pos_idx", 3)
    T = t_pos_idx.shape[0]
    t_tex_idx = _chk_index(t_tex_idx, "t_tex_idx", 3, T)
    out = torch.empty((H, W, 3), device=rast.device, dtype=torch.float32)
    counts = torch.empty(2, device=rast.device, dtype=torch.int32)
    _launch("tt_bake_encode", rast, v_nrm, t_pos_idx.int().contiguous(), tng_tex, t_tex_idx.int().contiguous(),
            field_nrm, v_nrm.shape[0], tng_tex.shape[0], T, H, W, out, counts, label="bake_encode")
    return out, counts


def uv_rasterize(v_tex: Tensor, t_tex_idx: Tensor, texture_size: int) -> Tensor:
    """rast (N,N,4) of the UV triangles over the N^2 texel centres, exactly as the exporter rasterises them: clip
    position (2u - 1, 2v - 1, 0, 1)."""
    from . import raster  # (raster imports this module)
    uv_clip = v_tex * 2.0 - 1.0
    uv_clip4 = torch.cat((uv_clip, torch.zeros_like(uv_clip[..., 0:1]), torch.ones_like(uv_clip[..., 0:1])), dim=-1)
    N = int(texture_size)
    return raster.rasterize(uv_clip4[None].float(), t_tex_idx.int(), (N, N))[0]


@torch.no_grad()
def bake_normal_map(mesh, normal_fn, texture_size: int, project_steps: int = 2, max_step: Optional[float] = None,
                    rast: Optional[Tensor] = None) -> Tuple[Tensor, dict]:
    """Tangent-space normal map (N,N,3) fp32 in [0,1] of `mesh` (a Mesh with UVs) from an analytic field:
    normal_fn(points (M,3)) -> (sdf (M,1), sdf_grad (M,3)).  Per covered texel of the UV rasterisation `rast` (N,N,4)
    (computed as the exporter does when None): the surface point interpolated from v_pos is pulled onto the field's
    iso-surface by `project_steps` bounded Newton steps (tt_bake_project, each at most max_step long: a texel of a
    simplified mesh lies up to sqrt(3) cells off the surface), the field's gradient there is normalised and written in
    the frame (t^, b^ = t^ x n^, n^) interpolated from mesh.v_tng_tex and mesh.v_nrm (tt_bake_encode; green = increasing
    OBJ v).  Uncovered texels are (0.5, 0.5, 1): fill them with texture_fill.  Only covered texels are queried
    (project_steps + 1 queries).  max_step defaults to extras["simplify"]["cell"] of a simplified mesh and must be given
    otherwise.  info = {n_covered, n_backfacing (field normal pointing into the face; stored as computed),
    mean_abs_sdf_before, mean_abs_sdf_after (|sdf| at the queried points before / after the projection), points (M,3):
    the projected points, texel (M,) int64: their flat texel ids, sdf_grad (M,3): the gradient the map encodes}.
    Nothing here is differentiable."""
    from . import raster  # (raster imports this module)
    N, steps = int(texture_size), int(project_steps)
    if steps < 0:
        raise ValueError(f"project_steps must be >= 0, got {project_steps}")
    if max_step is None:
        simp = mesh.extras.get("simplify") if hasattr(mesh, "extras") else None
        if simp is None:
            raise ValueError("max_step must be given for a mesh that was not simplified (no extras['simplify'])")
        max_step = float(simp["cell"])
    if rast is None:
        rast = uv_rasterize(mesh.v_tex, mesh.t_tex_idx, N)
    rast = _chk(rast, "rast", (N, N, 4))
    T = mesh.t_pos_idx.shape[0]
    tid = rast[..., 3].reshape(-1)
    texel = torch.nonzero((tid >= 1) & (tid <= T)).reshape(-1)
    pos = raster.interpolate(mesh.v_pos.detach().float()[None], rast[None], mesh.t_pos_idx.int())[0].reshape(-1, 3)
    pts = pos[texel].contiguous()
    M = pts.shape[0]

    def query(p):
        sdf, grad = normal_fn(p)
        return sdf.detach().float().reshape(-1), grad.detach().float().reshape(-1, 3)

    field = torch.zeros((N * N, 3), device=rast.device, dtype=torch.float32)
    before = after = 0.0
    grad = torch.zeros((0, 3), device=rast.device)
    if M > 0:
        sdf, grad = query(pts)
        before_t = sdf.abs().mean()
        for k in range(steps):
            if k > 0:
                sdf, grad = query(pts)
            bake_project_step(pts, sdf, grad, max_step)
        if steps > 0:
            sdf, grad = query(pts)
        before, after = (float(x) for x in torch.stack([before_t, sdf.abs().mean()]).cpu())
        field[texel] = grad
    out, counts = bake_encode(rast, mesh.v_nrm, mesh.t_pos_idx, mesh.v_tng_tex, mesh.t_tex_idx, field.reshape(N, N, 3))
    n_cov, n_back = (int(x) for x in counts.cpu())
    return out, {"n_covered": n_cov, "n_backfacing": n_back, "mean_abs_sdf_before": before, "mean_abs_sdf_after": after,
                 "points": pts, "texel": texel, "sdf_grad": grad}
