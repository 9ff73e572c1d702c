"""CPU ORACLE (test infrastructure, NOT product code).

Pure-torch restatement of TriplaneTurbo's differentiable triplane volume
renderer hot path.  It exists so that the HIP path in ``triplaneturbo_amd`` can
be checked; only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import it.  The product path never routes through it.

Parity status
-------------
* plane sampling, MLP decode, first-order normals: PINNED against the importable reference
  functions (``tests/golden/make_golden.py`` imports ``/root/reference/triplaneturbo_executable`` in the build
  container and dumps ``tests/golden/reference_ops.npz``; ``tests/test_oracle_golden.py`` replays them).
* NeuS alpha, rgb_grad_shrink (+ its C() schedule), NoMaterial, compositing, disparity, camera-space normal maps,
  training extras, proposal density, render_step_size, and the GRADIENTS of the G6 loss through all of that (rows
  a14-a16, a19-a21), plus the PatchRenderer composite (a22): PINNED against the reference's OWN renderer classes --
  ``tests/golden/make_golden_renderer.py`` imports neus_volume_renderer.py, generative_space_sdf_volume_renderer.py,
  patch_renderer.py, no_material.py and the threestudio utils from /root/reference and RUNS them (fp64 + fp32, forward
  + autograd backward) on the inputs of render_small.npz -> ``tests/golden/reference_renderer.npz``;
  ``tests/test_oracle_reference_renderer.py`` checks this file against those vectors (fp64: 1e-15, bit-equal loss),
  ``tests/test_gpu_backward.py::test_backward_small_golden`` checks the HIP path against them directly.
* second-order terms: the reference's own double backward is CUDA-only; through the reference renderer run above the
  second-order path is exercised with THIS file's gather-based bilinear op underneath (itself checked against
  ``F.grid_sample`` and by fp64 ``gradcheck``/``gradgradcheck``).
* ray marching (nerfacc v0.5.2 ``render_weight_from_alpha`` / ``accumulate_along_rays`` / ``importance_sampling``,
  rows a4, a17, a18): nerfacc is an un-vendored third-party CUDA dependency (requirements.txt:5) and the reference has
  no tests for it => **parity unpinned** at that boundary only; the restatement follows nerfacc's published semantics
  and the reference's call sites (the golden run above injects an index_add_/segmented-product restatement of the two
  volrend functions, written independently of the dense one below, and an estimator that returns fixed intervals).

* background hash encoding: tiny-cuda-nn (README.md:74, requirements.txt:6 --
  an un-vendored, UNPINNED git master dependency with no ROCm build) provides
  ``HashGrid``; ``hashgrid_*`` below restate its published algorithm (Mueller
  et al. 2022 + tcnn ``grid.h``: per-level scale/resolution, dense vs hashed
  index, trilinear interpolation) in fp32 => **parity unpinned** there too
  (tcnn itself computes this op in fp16).

Every function cites the reference file:line it follows (paths relative to
/root/reference).  All functions are dtype-generic (fp32 follows the
reference's op order; fp64 is used as the "exact" arbiter).
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor

# --------------------------------------------------------------------------
# A SECOND fp32 evaluation order (round 5): the same math, different rounding
# --------------------------------------------------------------------------
# fp32 arithmetic does not define ONE answer for this renderer: NeuS alpha is a ratio of nearly equal sigmoids scaled by
# inv_std = 100, and comp_normal normalises an accumulated normal that can nearly cancel, so in ill-conditioned scenes two
# correct fp32 evaluations that merely add in a different order -- or use a different, equally valid fp32 sigmoid -- differ
# by 1e-4 ... 1e-2 in the gradients.  To MEASURE that sensitivity per case (instead of inferring it from the distance to
# fp64), the decode and the march can be evaluated in two more documented ways:
#   alt_order(1)
#   * nn.Linear (vanilla_mlp): the K input channels in REVERSED order, accumulated in blocks of 8 (block partial sums
#     first, blocks added last-to-first) -- the reference / default order is torch's GEMM over k = 0 .. K-1;
#   * bilinear blend (grid_sample_gather): corners se, sw, ne, nw instead of nw, ne, sw, se;
#   * v1 plane sum (sample_from_planes): planes 2, 1, 0 instead of 0, 1, 2;
#   * accumulate_along_rays (render): samples far-to-near instead of near-to-far;
#   * the logistic function (get_alpha, proposal_density, sigmoid_mipnerf): evaluated in fp64 and rounded to fp32 -- a
#     CORRECTLY ROUNDED fp32 sigmoid -- instead of torch's fp32 kernel (a vectorised exp with ~1 ulp error): the difference
#     between two valid fp32 implementations of the same function, and the one that matters most, because NeuS alpha
#     subtracts two nearly equal logistics.
#   * F.normalize (per-sample normal, comp_normal): x * rsqrt(max(|x|^2, eps^2)) with |x|^2 summed z-first;
#   * the sphere bias |x| with the squares summed z-first.
#   alt_order(2)
#   * F.normalize: x * (1 / max(|x|, eps)) -- reciprocal-multiply instead of the division;
#   * nn.Linear: channels in natural order, blocks of 16, block partial sums added first-to-last;
#   * corners ne, nw, se, sw;  planes (0 + 2) + 1;  samples accumulated in two halves (near half + far half);
#   * the logistic function in its two-branch fp32 form: 1 / (1 + exp(-x)) for x >= 0, exp(x) / (1 + exp(x)) for x < 0.
#   alt_order(3)
#   * nn.Linear: blocks of 4 channels, even blocks first, then the odd ones;  corners sw, nw, se, ne;  planes (1 + 2) + 0;
#     samples accumulated in chunks of 8 (chunk sums added near-to-far);
#   * the correctly rounded logistic (as level 1);  F.normalize as x / sqrt(|x|^2) with |x|^2 = x^2 + (y^2 + z^2);
#   * the sample position o + d t with ONE rounding (evaluated in fp64 and rounded: what a fused multiply-add gives) instead
#     of a rounded product followed by a rounded sum -- the sample coordinates are where fp32 rounding enters the geometry side.
#   alt_order(2) and (3) also
#   * render_weight_from_alpha: the transmittance as the step-by-step recurrence T_{i+1} = T_i (1 - alpha_i) instead of
#     torch.cumprod -- same forward values; autograd's backward is then the reverse recurrence, where cumprod's backward
#     divides by (1 - alpha_i) and loses digits when an alpha sits next to 1 (use_volsdf: alpha is not clipped).
# Same operations, same operands, same dtype: the pairwise distances of the three fp32 evaluations are the order /
# implementation sensitivity of the fp32 math itself on that scene, and tests/parity.py asks of the HIP path
#     |hip - fp32| <= max(1e-4, 1.5 x the largest of those distances).
_ALT_ORDER = 0


@contextlib.contextmanager
def alt_order(level=1):
    """Evaluate every sum / logistic of the decode and the march in alternative way `level` (0 / False = the default order,
    True = 1)."""
    global _ALT_ORDER
    prev, _ALT_ORDER = _ALT_ORDER, int(level)
    try:
        yield
    finally:
        _ALT_ORDER = prev


def _sigmoid(x: Tensor) -> Tensor:
    """torch.sigmoid(x) -- or, under alt_order() on fp32 input, another valid fp32 logistic (see above)."""
    if _ALT_ORDER in (1, 3) and x.dtype == torch.float32:
        return torch.sigmoid(x.double()).float()
    if _ALT_ORDER == 2:
        e = torch.exp(-x.abs())
        return torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    return torch.sigmoid(x)


def _normalize(x: Tensor, eps: float = 1e-12) -> Tensor:
    """F.normalize(x, dim=-1) -- or, under alt_order(), one of two other valid fp32 forms (see above)."""
    if _ALT_ORDER == 1:
        n2 = (x[..., 2:3] ** 2 + x[..., 1:2] ** 2) + x[..., 0:1] ** 2
        return x * torch.rsqrt(n2.clamp_min(eps * eps))
    if _ALT_ORDER == 2:
        return x * (1.0 / torch.linalg.norm(x, dim=-1, keepdim=True).clamp_min(eps))
    if _ALT_ORDER == 3:
        n2 = x[..., 0:1] ** 2 + (x[..., 1:2] ** 2 + x[..., 2:3] ** 2)
        return x / n2.sqrt().clamp_min(eps)
    return F.normalize(x, dim=-1, eps=eps)


def _norm3(x: Tensor) -> Tensor:
    """|x| of (..., 3) with keepdim, as (x ** 2).sum(-1).sqrt() -- under alt_order(1) with the squares summed z-first."""
    if _ALT_ORDER == 1:
        return ((x[..., 2:3] ** 2 + x[..., 1:2] ** 2) + x[..., 0:1] ** 2).sqrt()
    return (x ** 2).sum(dim=-1, keepdim=True).sqrt()


def _linear(x: Tensor, w: Tensor) -> Tensor:
    """F.linear(x, w) -- or, under alt_order(), the same product with the channels reversed and accumulated in blocks of 8."""
    if not _ALT_ORDER:
        return F.linear(x, w)
    K = w.shape[1]
    out = None
    if _ALT_ORDER == 1:
        for k1 in range(K, 0, -8):  # reversed channels, blocks of 8 last-to-first
            k0 = max(k1 - 8, 0)
            part = F.linear(x[..., k0:k1].flip(-1), w[:, k0:k1].flip(-1))
            out = part if out is None else out + part
    elif _ALT_ORDER == 2:
        for k0 in range(0, K, 16):  # natural order, blocks of 16 first-to-last
            part = F.linear(x[..., k0:k0 + 16], w[:, k0:k0 + 16])
            out = part if out is None else out + part
    else:
        for k0 in list(range(0, K, 8)) + list(range(4, K, 8)):  # blocks of 4: the even ones, then the odd ones
            part = F.linear(x[..., k0:k0 + 4], w[:, k0:k0 + 4])
            out = part if out is None else out + part
    return out


# --------------------------------------------------------------------------
# plane re-orientation, projection, bilinear sampling
# --------------------------------------------------------------------------
def rotate_planes_v1(space_cache: Tensor) -> Tensor:
    """custom/triplaneturbo/models/geometry/few_step_triplane_dual_stable_diffusion.py:212-225

    space_cache (B, 6, C, H, W) -> re-oriented copy.  Planes 0,3: transpose;
    planes 1,4: rot180; planes 2,5: rot90 clockwise.
    """
    out = torch.zeros_like(space_cache)
    out[:, 0::3] = torch.transpose(space_cache[:, 0::3], 3, 4)
    out[:, 1::3] = torch.rot90(space_cache[:, 1::3], k=2, dims=(3, 4))
    out[:, 2::3] = torch.rot90(space_cache[:, 2::3], k=-1, dims=(3, 4))
    return out


def project_onto_planes(coordinates: Tensor) -> Tensor:
    """custom/triplaneturbo/models/geometry/utils.py:46-63,111-125

    The reference multiplies by inverses of three permutation matrices; the
    products are exact, so the projection is a component selection:
    plane0 -> (x, y), plane1 -> (x, z), plane2 -> (z, y).
    coordinates (N, M, 3) -> (N, 3, M, 2)
    """
    x, y, z = coordinates.unbind(-1)
    return torch.stack(
        [torch.stack([x, y], -1), torch.stack([x, z], -1), torch.stack([z, y], -1)],
        dim=1,
    )


def bilinear_corners(grid: Tensor, H: int, W: int, padding_mode: str = "zeros", align_corners: bool = False):
    """ATen GridSampler index math (aten/src/ATen/native/cuda/GridSampler.cuh:23-31, GridSampler.h
    grid_sampler_unnormalize / clip_coordinates; gridsample_cuda.cu:87-129 uses the same formulas).  The renderer
    path uses the defaults (zeros padding, align_corners=False); "border" clips the pixel coordinate to
    [0, size-1] (gradient 0 outside), align_corners=True maps -1/+1 to the centres of the corner pixels.

    grid (..., 2) with [...,0] -> W axis.  Returns a list of 4 corners
    (iy, ix, weight, in_bounds) in the order nw, ne, sw, se.
    """
    gx, gy = grid[..., 0], grid[..., 1]
    if align_corners:
        ix = ((gx + 1) / 2) * (W - 1)
        iy = ((gy + 1) / 2) * (H - 1)
    else:
        ix = ((gx + 1) * W - 1) / 2
        iy = ((gy + 1) * H - 1) / 2
    if padding_mode == "border":
        # (clip_coordinates_set_grad: the gradient is 0 for ip <= 0 and ip >= size-1; torch.clamp's own backward lets
        # it through AT the two bounds, so the clipped branch is cut off the graph.  Same values.)
        ix = torch.where((ix > 0) & (ix < W - 1), ix, ix.detach().clamp(0, W - 1))
        iy = torch.where((iy > 0) & (iy < H - 1), iy, iy.detach().clamp(0, H - 1))
    elif padding_mode != "zeros":
        raise ValueError(padding_mode)
    ix_nw = torch.floor(ix)
    iy_nw = torch.floor(iy)
    ix_ne, iy_ne = ix_nw + 1, iy_nw
    ix_sw, iy_sw = ix_nw, iy_nw + 1
    ix_se, iy_se = ix_nw + 1, iy_nw + 1
    nw = (ix_se - ix) * (iy_se - iy)
    ne = (ix - ix_sw) * (iy_sw - iy)
    sw = (ix_ne - ix) * (iy - iy_ne)
    se = (ix - ix_nw) * (iy - iy_nw)
    corners = []
    for cx, cy, w in ((ix_nw, iy_nw, nw), (ix_ne, iy_ne, ne), (ix_sw, iy_sw, sw), (ix_se, iy_se, se)):
        inb = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
        corners.append((cy, cx, w, inb))
    return corners


def grid_sample_gather(inp: Tensor, grid: Tensor, padding_mode: str = "zeros", align_corners: bool = False) -> Tensor:
    """Gather-based restatement of F.grid_sample(mode='bilinear', padding_mode, align_corners); the renderer uses
    padding_mode='zeros', align_corners=False (custom/triplaneturbo/models/geometry/utils.py:21-24).

    Built from differentiable indexing so that autograd provides first AND
    second order derivatives on CPU (stock torch has no double backward for
    aten::grid_sampler_2d_backward; the reference needs its CUDA extension
    gridsample_cuda.cu for that).

    inp (N, C, H, W), grid (N, M, 2) -> (N, M, C)
    """
    N, C, H, W = inp.shape
    flat = inp.permute(0, 2, 3, 1).reshape(N, H * W, C)
    out = None
    corners = bilinear_corners(grid, H, W, padding_mode, align_corners)
    if _ALT_ORDER == 1:
        corners = corners[::-1]
    elif _ALT_ORDER == 2:
        corners = [corners[1], corners[0], corners[3], corners[2]]
    elif _ALT_ORDER == 3:
        corners = [corners[2], corners[0], corners[3], corners[1]]
    for cy, cx, w, inb in corners:
        idx = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long()  # (N, M)
        val = torch.gather(flat, 1, idx[..., None].expand(-1, -1, C))
        val = val * inb[..., None].to(inp.dtype)
        term = val * w[..., None]
        out = term if out is None else out + term
    return out


def sample_from_planes(plane_features: Tensor, coordinates: Tensor, interpolate_feat: str,
                       box_warp: float = 2.0) -> Tensor:
    """custom/triplaneturbo/models/geometry/utils.py:127-145 (v1 = sum, v2 = concat).

    plane_features (N, 3, C, H, W) (already re-oriented), coordinates (N, M, 3).
    """
    N, n_planes, C, H, W = plane_features.shape
    M = coordinates.shape[1]
    coordinates = (2 / box_warp) * coordinates
    proj = project_onto_planes(coordinates).reshape(N * n_planes, M, 2)
    feats = grid_sample_gather(plane_features.reshape(N * n_planes, C, H, W), proj)
    feats = feats.reshape(N, n_planes, M, C)
    if interpolate_feat in (None, "v1"):
        if _ALT_ORDER == 1:
            return (feats[:, 2] + feats[:, 1]) + feats[:, 0]
        if _ALT_ORDER == 2:
            return (feats[:, 0] + feats[:, 2]) + feats[:, 1]
        if _ALT_ORDER == 3:
            return (feats[:, 1] + feats[:, 2]) + feats[:, 0]
        return feats.sum(dim=1)
    elif interpolate_feat == "v2":
        return feats.permute(0, 2, 1, 3).reshape(N, M, n_planes * C)
    raise ValueError(interpolate_feat)


# --------------------------------------------------------------------------
# MLP, activations
# --------------------------------------------------------------------------
def vanilla_mlp(x: Tensor, weights: Sequence[Tensor]) -> Tensor:
    """threestudio/models/networks.py:67-104 -- Linear(bias=False)+ReLU, no output activation."""
    for i, w in enumerate(weights):
        x = _linear(x, w)
        if i + 1 < len(weights):
            x = torch.relu(x)
    return x


def sigmoid_mipnerf(x: Tensor) -> Tensor:
    """threestudio/utils/ops.py:118-119"""
    return _sigmoid(x) * (1 + 2 * 0.001) - 0.001


def scale_tensor(dat: Tensor, inp_scale, tgt_scale) -> Tensor:
    """threestudio/utils/ops.py:27-38"""
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    dat = dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]
    return dat


# --------------------------------------------------------------------------
# geometry decode (per point)
# --------------------------------------------------------------------------
def geometry_forward(points: Tensor, space_cache: Tensor, sdf_weights: Sequence[Tensor],
                     feat_weights: Sequence[Tensor], radius: float = 1.0,
                     sdf_bias_radius: float = 0.5, output_normal: bool = True,
                     create_graph: bool = False) -> Dict[str, Tensor]:
    """few_step_triplane_dual_stable_diffusion.py:273-351 (+ :131-154, :198-271).

    points (B, N, 3) in world units; space_cache (B, 6, C, H, W) as produced by
    the generator (NOT yet re-oriented).  Returns tensors shaped (B*N, .).
    """
    B, N, _ = points.shape
    if output_normal and not points.requires_grad:
        points = points.detach().requires_grad_(True)  # few_step...:283-286
    with (torch.enable_grad() if output_normal else contextlib.nullcontext()):
        points_unscaled = points
        pts = scale_tensor(points, (-radius, radius), (-1, 1))  # contract_to_unisphere_custom, utils.py:31-43
        rot = rotate_planes_v1(space_cache)
        enc_geo = sample_from_planes(rot[:, 0:3], pts, "v1")
        enc_tex = sample_from_planes(rot[:, 3:6], pts, "v2")
        sdf_orig = vanilla_mlp(enc_geo, sdf_weights).view(B, N, 1)
        sdf_bias = _norm3(points_unscaled) - sdf_bias_radius
        sdf = sdf_orig + sdf_bias
        features = vanilla_mlp(enc_tex, feat_weights).view(B, N, -1)
        out = {
            "sdf": sdf.reshape(B * N, 1),
            "sdf_orig": sdf_orig.reshape(B * N, 1),
            "features": features.reshape(B * N, -1),
            "enc_geo": enc_geo.reshape(B * N, -1),
            "enc_tex": enc_tex.reshape(B * N, -1),
        }
        if output_normal:
            sdf_grad = torch.autograd.grad(sdf, points_unscaled, grad_outputs=torch.ones_like(sdf),
                                           create_graph=create_graph)[0]
            normal = _normalize(sdf_grad)
            if not create_graph:
                sdf_grad, normal = sdf_grad.detach(), normal.detach()
            out.update(normal=normal.reshape(B * N, 3), shading_normal=normal.reshape(B * N, 3),
                       sdf_grad=sdf_grad.reshape(B * N, 3))
    return out


# --------------------------------------------------------------------------
# NeuS alpha + ray marching
# --------------------------------------------------------------------------
def volsdf_density(sdf: Tensor, inv_std) -> Tensor:
    """threestudio/models/renderers/neus_volume_renderer.py:19-23: the VolSDF Laplace-cdf density, inv_std clamped to [0, 80]."""
    inv_std = torch.as_tensor(inv_std, dtype=sdf.dtype).clamp(0.0, 80.0)
    beta = 1 / inv_std
    alpha = inv_std
    return alpha * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / beta))


def get_alpha(sdf: Tensor, normal: Tensor, dirs: Tensor, dists: Tensor, inv_std: float,
              cos_anneal_ratio: float = 1.0, use_volsdf: bool = False) -> Tensor:
    """threestudio/models/renderers/neus_volume_renderer.py:93-117 (use_volsdf=True: :95-96, alpha = |dists| x density,
    NOT clipped, independent of the normal)."""
    if use_volsdf:
        return torch.abs(dists.detach()) * volsdf_density(sdf, inv_std)
    true_cos = (dirs * normal).sum(-1, keepdim=True)
    iter_cos = -(F.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio)
                 + F.relu(-true_cos) * cos_anneal_ratio)
    estimated_next_sdf = sdf + iter_cos * dists * 0.5
    estimated_prev_sdf = sdf - iter_cos * dists * 0.5
    prev_cdf = _sigmoid(estimated_prev_sdf * inv_std)
    next_cdf = _sigmoid(estimated_next_sdf * inv_std)
    p = prev_cdf - next_cdf
    c = prev_cdf
    return ((p + 1e-5) / (c + 1e-5)).clip(0.0, 1.0)


def proposal_density(sdf: Tensor, inv_std: float, render_step_size: float, use_volsdf: bool = False) -> Tensor:
    """generative_space_sdf_volume_renderer.py:286-297 (fixed-step NeuS density of the proposal pass; use_volsdf: :286-287)."""
    if use_volsdf:
        return volsdf_density(sdf, inv_std)
    estimated_next_sdf = sdf - render_step_size * 0.5
    estimated_prev_sdf = sdf + render_step_size * 0.5
    prev_cdf = _sigmoid(estimated_prev_sdf * inv_std)
    next_cdf = _sigmoid(estimated_next_sdf * inv_std)
    p = prev_cdf - next_cdf
    c = prev_cdf
    alpha = ((p + 1e-5) / (c + 1e-5)).clip(0.0, 1.0)
    return alpha / render_step_size


def render_weight_from_alpha(alpha: Tensor) -> Tuple[Tensor, Tensor]:
    """nerfacc v0.5.2 render_weight_from_alpha on a dense (n_rays, S) layout
    (call site generative_space_sdf_volume_renderer.py:408-412):
    trans_i = prod_{j<i}(1-alpha_j), w_i = alpha_i * trans_i.  [parity unpinned]
    """
    one_minus = 1.0 - alpha
    if _ALT_ORDER >= 2:
        # alternative evaluations 2 / 3: the recurrence T_0 = 1, T_{i+1} = T_i (1 - alpha_i) step by step.  Same forward
        # values; autograd's backward is then the reverse recurrence itself, where torch.cumprod's backward forms
        # reverse_cumsum(grad * out) / input -- a division by (1 - alpha_i) that loses digits when an alpha sits next to 1
        # (use_volsdf: alpha is not clipped and crosses 1 continuously; NeuS alpha saturates AT 1, which cumprod treats apart)
        cols = [torch.ones_like(alpha[:, 0])]
        for i in range(alpha.shape[1] - 1):
            cols.append(cols[-1] * one_minus[:, i])
        trans = torch.stack(cols, dim=1)
        return alpha * trans, trans
    trans = torch.cumprod(
        torch.cat([torch.ones_like(alpha[:, :1]), one_minus[:, :-1]], dim=1), dim=1)
    return alpha * trans, trans


def render(space_cache: Tensor, sdf_weights: Sequence[Tensor], feat_weights: Sequence[Tensor],
           rays_o: Tensor, rays_d: Tensor, t_starts: Tensor, t_ends: Tensor,
           bg_color: Tensor, camera_distances: Tensor, c2w: Tensor,
           inv_std: float = 100.0, radius: float = 1.0, sdf_bias_radius: float = 0.5,
           cos_anneal_ratio: float = 1.0, rgb_grad_shrink: float = 1.0,
           create_graph: bool = True, training: bool = True, use_volsdf: bool = False) -> Dict[str, Tensor]:
    """GenerativeSpaceSDFVolumeRenderer._forward for explicit sample intervals
    (generative_space_sdf_volume_renderer.py:214-238, 326-546).

    space_cache (P, 6, C, H, W); rays_o/rays_d (B, Hh, Ww, 3) with B = P*n_view
    (view b uses prompt b // n_view, = the repeat_interleave of :120-143);
    t_starts/t_ends (B*Hh*Ww, S); bg_color (3,) or (B*Hh*Ww, 3) or (B,Hh,Ww,3).
    """
    B, Hh, Ww, _ = rays_o.shape
    P = space_cache.shape[0]
    n_view = B // P
    n_rays = B * Hh * Ww
    S = t_starts.shape[1]
    ro = rays_o.reshape(-1, 3)
    rd = rays_d.reshape(-1, 3)
    cache = space_cache.repeat_interleave(n_view, dim=0) if n_view > 1 else space_cache

    # :333-339
    t_positions = ((t_starts + t_ends) / 2.0).reshape(-1, 1)
    t_intervals = (t_ends - t_starts).reshape(-1, 1)
    ray_indices = torch.arange(n_rays).unsqueeze(-1).expand(-1, S).reshape(-1)
    t_origins = ro[ray_indices]
    t_dirs = rd[ray_indices]
    if _ALT_ORDER == 3 and t_positions.dtype == torch.float32:  # one rounding, as a fused multiply-add
        positions = (t_origins.double() + t_dirs.double() * t_positions.double()).float()
    else:
        positions = t_origins + t_dirs * t_positions

    geo = geometry_forward(positions.reshape(B, -1, 3), cache, sdf_weights, feat_weights,
                           radius=radius, sdf_bias_radius=sdf_bias_radius,
                           output_normal=True, create_graph=create_graph)
    rgb_fg_all = sigmoid_mipnerf(geo["features"])  # no_material.py:41-54
    if rgb_grad_shrink != 1.0:  # :397-400
        rgb_fg_all = rgb_grad_shrink * rgb_fg_all + (1.0 - rgb_grad_shrink) * rgb_fg_all.detach()

    alpha = get_alpha(geo["sdf"], geo["normal"], t_dirs, t_intervals, inv_std, cos_anneal_ratio, use_volsdf)
    weights2d, trans2d = render_weight_from_alpha(alpha.reshape(n_rays, S))
    weights = weights2d.reshape(-1, 1)

    def accumulate(values: Optional[Tensor]) -> Tensor:
        # nerfacc.accumulate_along_rays (call sites :414-431, :467-472)
        src = weights if values is None else weights * values
        src = src.reshape(n_rays, S, -1)
        if _ALT_ORDER == 1:  # far-to-near, one sample at a time
            acc = src[:, S - 1]
            for k in range(S - 2, -1, -1):
                acc = acc + src[:, k]
            return acc
        if _ALT_ORDER == 2 and S > 1:  # near half + far half
            return src[:, :S // 2].sum(dim=1) + src[:, S // 2:].sum(dim=1)
        if _ALT_ORDER == 3:  # chunks of 8 samples, chunk sums added near-to-far
            acc = None
            for k0 in range(0, S, 8):
                part = src[:, k0:k0 + 8].sum(dim=1)
                acc = part if acc is None else acc + part
            return acc
        return src.sum(dim=1)

    opacity = accumulate(None)
    depth = accumulate(t_positions)
    comp_rgb_fg = accumulate(rgb_fg_all)
    t_depth = depth[ray_indices]
    z_variance = accumulate((t_positions - t_depth) ** 2)

    bg = bg_color
    if bg.ndim == 1:
        bg = bg[None, :].expand(n_rays, -1)
    bg = bg.reshape(n_rays, -1)
    comp_rgb = comp_rgb_fg + bg * (1.0 - opacity)

    out = {
        "comp_rgb": comp_rgb.view(B, Hh, Ww, -1),
        "comp_rgb_fg": comp_rgb_fg.view(B, Hh, Ww, -1),
        "comp_rgb_bg": bg.reshape(B, Hh, Ww, -1),
        "opacity": opacity.view(B, Hh, Ww, 1),
        "depth": depth.view(B, Hh, Ww, 1),
        "z_variance": z_variance.view(B, Hh, Ww, 1),
    }
    # :452-462 (disparity, RichDreamer convention)
    cd = camera_distances.reshape(-1, 1, 1, 1)
    far = cd + math.sqrt(3.0)
    near = cd - math.sqrt(3.0)
    disparity_tmp = out["depth"] * out["opacity"] + (1.0 - out["opacity"]) * far
    out["disparity"] = torch.clamp((far - disparity_tmp) / (far - near), 0.0, 1.0)

    # :466-505 (normal_direction == "camera")
    normal_acc = accumulate(geo["normal"])
    out["normal_acc"] = normal_acc  # un-normalised sum_i w_i n_i (what tt_render_fwd returns)
    comp_normal = _normalize(normal_acc)
    out["comp_normal"] = comp_normal.view(B, Hh, Ww, 3)
    bg_normal = 0.5 * torch.ones_like(comp_normal)
    bg_normal[:, 2] = 1.0
    bg_normal_white = torch.ones_like(comp_normal)
    w2c = torch.inverse(c2w)
    rot = w2c[:, :3, :3]
    comp_normal_cam = comp_normal.view(B, -1, 3) @ rot.permute(0, 2, 1)
    flip_x = torch.eye(3, dtype=comp_normal.dtype)
    flip_x[0, 0] = -1
    comp_normal_cam = (comp_normal_cam @ flip_x[None]).view(-1, 3)
    out["comp_normal_cam_vis"] = ((comp_normal_cam + 1.0) / 2.0 * opacity + (1 - opacity) * bg_normal).view(B, Hh, Ww, 3)
    out["comp_normal_cam_vis_white"] = ((comp_normal_cam + 1.0) / 2.0 * opacity + (1 - opacity) * bg_normal_white).view(B, Hh, Ww, 3)

    if training:  # :532-545
        out.update(weights=weights, t_points=t_positions, t_intervals=t_intervals, t_dirs=t_dirs,
                   ray_indices=ray_indices, points=positions, alpha=alpha, trans=trans2d.reshape(-1, 1),
                   sdf=geo["sdf"], sdf_orig=geo["sdf_orig"], features=geo["features"],
                   normal=geo["normal"], shading_normal=geo["shading_normal"],
                   sdf_grad=geo["sdf_grad"], inv_std=torch.as_tensor(inv_std))
    return out


# --------------------------------------------------------------------------
# background: multiresolution hash encoding (tiny-cuda-nn HashGrid) + hypernet MLP
# --------------------------------------------------------------------------
HASH_PRIMES = (1, 2654435761, 805459861)


def hashgrid_levels(n_levels: int = 8, log2_hashmap_size: int = 19, base_resolution: int = 4,
                    per_level_scale: float = 1.8114473285278132):
    """Per-level (offset, size, scale, resolution) of tcnn's GridEncoding (3-D, GridType::Hash):
    scale_l = exp2(l * log2(per_level_scale)) * base_resolution - 1 (tcnn evaluates this with fp32 libm calls; here
    and in tt_hashgrid.hip it is evaluated in double from the fp32 per_level_scale and rounded once to fp32, so that
    it is libm-independent), resolution_l = ceil(scale_l) + 1,
    size_l = min(next_multiple(resolution_l^3, 8), 2^log2_hashmap_size); offsets are the running sum.
    (defaults = multi_prompt_neural_environment_hashgrid_map_background.py:25-34)"""
    import numpy as np
    levels, offset = [], 0
    l2 = math.log2(float(np.float32(per_level_scale)))
    for l in range(n_levels):
        scale = np.float32(2.0 ** (l * l2) * base_resolution - 1.0)
        res = int(math.ceil(float(scale))) + 1
        size = min((res ** 3 + 7) // 8 * 8, 1 << log2_hashmap_size) if res ** 3 < 2 ** 31 else 1 << log2_hashmap_size
        levels.append((offset, size, float(scale), res))
        offset += size
    return levels, offset


def hashgrid_encode(x: Tensor, params: Tensor, n_levels: int = 8, n_features: int = 2, log2_hashmap_size: int = 19,
                    base_resolution: int = 4, per_level_scale: float = 1.8114473285278132) -> Tensor:
    """tcnn kernel_grid (Linear interpolation): x (N,3) in [0,1]; params flat (total*F,) level-major, entry-major,
    feature-minor; returns (N, n_levels*F).  Per level: pos = scale*x + 0.5, cell = floor(pos), frac = pos - cell;
    corner index = dense x + y*res + z*res^2 when res^3 fits the level, else XOR of coord*prime (uint32), then
    % size; weights = prod(frac or 1-frac)."""
    levels, total = hashgrid_levels(n_levels, log2_hashmap_size, base_resolution, per_level_scale)
    assert params.numel() == total * n_features
    table = params.reshape(total, n_features)
    outs = []
    for (offset, size, scale, res) in levels:
        pos = x * scale + 0.5
        cell = torch.floor(pos)
        frac = pos - cell
        cell = cell.to(torch.int64)
        dense = res ** 3 <= size
        acc = 0
        for corner in range(8):
            w = 1
            idx3 = []
            for d in range(3):
                if corner & (1 << d):
                    w = w * frac[:, d]
                    idx3.append(cell[:, d] + 1)
                else:
                    w = w * (1 - frac[:, d])
                    idx3.append(cell[:, d])
            if dense:
                index = idx3[0] + idx3[1] * res + idx3[2] * res * res
            else:
                index = (idx3[0] * HASH_PRIMES[0]) & 0xFFFFFFFF
                index = index ^ ((idx3[1] * HASH_PRIMES[1]) & 0xFFFFFFFF)
                index = index ^ ((idx3[2] * HASH_PRIMES[2]) & 0xFFFFFFFF)
            index = index % size
            acc = acc + w[:, None] * table[offset + index]
        outs.append(acc)
    return torch.cat(outs, dim=1)


def hypernet_background(dirs: Tensor, text_embed: Tensor, grid_params: Tensor, hyper: Sequence[Tensor],
                        color_activation: str = "sigmoid-mipnerf", grid_cfg: Optional[dict] = None) -> Tensor:
    """MultipromptNeuralHashgridEnvironmentMapBackground.forward
    (multi_prompt_neural_environment_hashgrid_map_background.py:88-124) with LinearHyperNetwork
    (geometry/hypernetwork.py:18-100, n_hidden_layers = 1): hyper = (W0 (64,c_dim), ln_w, ln_b, W1 (n_out,64), b1).
    dirs (B,H,W,3) unit vectors; text_embed (P,c_dim), B a multiple of P."""
    B, Hh, Ww, _ = dirs.shape
    W0, ln_w, ln_b, W1, b1 = hyper
    h = F.silu(F.layer_norm(F.linear(text_embed, W0), (W0.shape[0],), ln_w, ln_b))
    out = F.linear(h, W1, b1)
    enc_dim = (grid_cfg or {}).get("n_levels", 8) * (grid_cfg or {}).get("n_features", 2)
    P = text_embed.shape[0]
    m1 = out[:, :enc_dim * 64].reshape(P, enc_dim, 64)  # out_dims {"bg_weights": [enc, 64, 3]}
    m2 = out[:, enc_dim * 64:enc_dim * 64 + 64 * 3].reshape(P, 64, 3)
    enc = hashgrid_encode(((dirs + 1.0) / 2.0).reshape(-1, 3), grid_params, **(grid_cfg or {}))
    enc = enc.reshape(B, Hh * Ww, enc_dim)
    nv = B // P
    x = torch.relu(torch.bmm(enc, m1.repeat_interleave(nv, dim=0)))
    x = torch.bmm(x, m2.repeat_interleave(nv, dim=0)).reshape(B, Hh, Ww, 3)
    if color_activation == "sigmoid-mipnerf":
        return sigmoid_mipnerf(x)
    if color_activation == "sigmoid":
        return torch.sigmoid(x)
    raise ValueError(color_activation)


# --------------------------------------------------------------------------
# samplers
# --------------------------------------------------------------------------
def placement_u(n: int, placement: str = "tt", jitter: Optional[Tensor] = None, dtype=torch.float32,
                level0: bool = False) -> Tensor:
    """cdf-space positions u_j, j = 0..n, of the n + 1 edges of one sampling level (1, n+1) or, jittered, (R, n+1).
    [parity unpinned: nerfacc v0.5.2's pdf.cu is unavailable, so the convention is an explicit contract, enum
    tt_sample_placement in include/tt_abi.h]
      "tt"     u_j = j / n; jitter: level 0 moves interior edges by (U - 0.5) / n, the fine level adds U / n, clamped
      "center" u_j = (j + 0.5) / (n + 1); jitter: (j + U_j) / (n + 1)"""
    j = torch.arange(n + 1, dtype=dtype)[None, :]
    if placement == "center":
        return (j + (0.5 if jitter is None else jitter.to(dtype))) / (n + 1)
    if placement != "tt":
        raise ValueError(placement)
    u = torch.linspace(0.0, 1.0, n + 1, dtype=dtype)[None, :]
    if jitter is None:
        return u
    if level0:
        interior = ((j > 0) & (j < n)).to(dtype)
        return u + interior * (jitter.to(dtype) - 0.5) / n
    return (u + jitter.to(dtype) / n).clamp(0.0, 1.0)


def uniform_intervals(n_rays: int, n_samples: int, near: float, far: float, dtype=torch.float32,
                      placement: str = "tt", jitter: Optional[Tensor] = None):
    """Level-0 of ImportanceEstimator.sampling (threestudio/models/estimators.py:61-79, 104-118): n_samples
    intervals on [near, far] from the uniform cdf; with the default placement and no jitter
    t_k = near + (far-near) * k / n_samples."""
    s = placement_u(n_samples, placement, jitter, dtype, level0=True)
    t = s * far + (1 - s) * near  # _transform_stot "uniform"
    t = t.expand(n_rays, -1)
    return t[:, :-1].contiguous(), t[:, 1:].contiguous()


def importance_resample(t_edges: Tensor, cdfs: Tensor, n: int, placement: str = "tt",
                        jitter: Optional[Tensor] = None) -> Tensor:
    """Inverse-CDF placement of n+1 edges, following nerfacc v0.5.2
    pdf.importance_sampling semantics for a dense batch: u_k (placement_u)
    mapped through the piecewise-linear CDF.
    [parity unpinned: nerfacc's exact u convention lives in its pdf.cu]

    t_edges (R, K+1) increasing, cdfs (R, K+1) non-decreasing in [0,1].
    """
    R = t_edges.shape[0]
    u = placement_u(n, placement, jitter, t_edges.dtype).expand(R, -1).contiguous()
    idx = torch.searchsorted(cdfs.contiguous(), u, right=True)
    lo = (idx - 1).clamp(0, cdfs.shape[1] - 1)
    hi = idx.clamp(0, cdfs.shape[1] - 1)
    c_lo, c_hi = cdfs.gather(1, lo), cdfs.gather(1, hi)
    t_lo, t_hi = t_edges.gather(1, lo), t_edges.gather(1, hi)
    denom = c_hi - c_lo
    frac = torch.where(denom > 0, (u - c_lo) / torch.where(denom > 0, denom, torch.ones_like(denom)),
                       torch.zeros_like(denom))
    return t_lo + frac.clamp(0, 1) * (t_hi - t_lo)


def importance_sampling(sdf_fn, n_rays: int, n_prop: int, n_fine: int, near: float, far: float,
                        inv_std: float, render_step_size: float, dtype=torch.float32, placement: str = "tt",
                        jitter0: Optional[Tensor] = None, jitter1: Optional[Tensor] = None):
    """ImportanceEstimator.sampling, one proposal level
    (threestudio/models/estimators.py:22-101; prop_sigma_fn =
    generative_space_sdf_volume_renderer.py:243-299).  jitter0 (n_rays, n_prop+1) / jitter1 (n_rays, n_fine+1):
    the U[0,1) draws of the two levels (None = stratified=False).

    sdf_fn(t_starts, t_ends) -> sdf (n_rays, n_prop) evaluated at interval mid-points.
    Returns t_starts, t_ends (n_rays, n_prop + n_fine + 1).
    """
    ts, te = uniform_intervals(n_rays, n_prop, near, far, dtype, placement, jitter0)
    t_vals = torch.cat([ts, te[:, -1:]], dim=1)
    sdf = sdf_fn(ts, te)
    sigma = proposal_density(sdf, inv_std, render_step_size)
    # nerfacc.render_transmittance_from_density: exp(-exclusive_cumsum(sigma * dt))
    sd = sigma * (te - ts)
    excl = torch.cumsum(torch.cat([torch.zeros_like(sd[:, :1]), sd[:, :-1]], dim=1), dim=1)
    trans = torch.exp(-excl)
    cdfs = 1.0 - torch.cat([trans, torch.zeros_like(trans[:, :1])], dim=1)
    t_fine = importance_resample(t_vals, cdfs, n_fine, placement, jitter1)
    t_all, _ = torch.sort(torch.cat([t_vals, t_fine], dim=1), dim=1)
    return t_all[:, :-1].contiguous(), t_all[:, 1:].contiguous()


# --------------------------------------------------------------------------
# the reference's native op: second-order grid_sample (K1)
# --------------------------------------------------------------------------
def grid_sample_2d_grad2(grad2_grad_input: Tensor, grad2_grad_grid: Tensor, grad_output: Tensor,
                         inp: Tensor, grid: Tensor):
    """Restatement of gridsample_cuda.cu:27-210 / gridsample_cuda.cpp:26-37
    (``grad2_2d``; zeros padding, align_corners=False) obtained by
    differentiating the restated bilinear op twice with autograd.

    inp (N,C,H,W), grid (N,Ho,Wo,2), grad_output (N,C,Ho,Wo),
    grad2_grad_input like inp, grad2_grad_grid like grid.
    Returns (grad_grad_output, grad_input, grad_grid).
    """
    N, C, H, W = inp.shape
    Ho, Wo = grid.shape[1:3]
    inp_ = inp.detach().requires_grad_(True)
    grid_ = grid.detach().requires_grad_(True)
    go_ = grad_output.detach().requires_grad_(True)
    out = grid_sample_gather(inp_, grid_.reshape(N, Ho * Wo, 2))  # (N, M, C)
    out = out.permute(0, 2, 1).reshape(N, C, Ho, Wo)
    g_inp, g_grid = torch.autograd.grad(out, (inp_, grid_), go_, create_graph=True)
    scalar = (g_inp * grad2_grad_input).sum() + (g_grid * grad2_grad_grid).sum()
    ggo, gi, gg = torch.autograd.grad(scalar, (go_, inp_, grid_), allow_unused=True)
    gi = torch.zeros_like(inp) if gi is None else gi
    gg = torch.zeros_like(grid) if gg is None else gg
    return ggo, gi, gg


# --------------------------------------------------------------------------
# cameras (synthetic inputs; reference training distribution)
# --------------------------------------------------------------------------
def make_cameras(n_view: int, height: int, width: int, fovy_deg: float = 60.0,
                 rel_distance: float = 0.9, elevation_deg: float = 15.0,
                 azimuth_start_deg: float = 0.0, dtype=torch.float32):
    """custom/triplaneturbo/data/*v2.py:251-359 + threestudio/utils/ops.py:194-231,301-347.
    Returns rays_o, rays_d (n_view, H, W, 3), c2w (n_view,4,4), camera_distances (n_view,)."""
    fovy = torch.full((n_view,), fovy_deg * math.pi / 180, dtype=dtype)
    az = (azimuth_start_deg + 360.0 / n_view * torch.arange(n_view, dtype=dtype)) * math.pi / 180
    el = torch.full((n_view,), elevation_deg * math.pi / 180, dtype=dtype)
    cam_d = rel_distance / torch.tan(0.5 * fovy)
    pos = torch.stack([cam_d * torch.cos(el) * torch.cos(az), cam_d * torch.cos(el) * torch.sin(az),
                       cam_d * torch.sin(el)], dim=-1)
    center = torch.zeros_like(pos)
    up = torch.tensor([0, 0, 1], dtype=dtype)[None].repeat(n_view, 1)
    lookat = F.normalize(center - pos, dim=-1)
    right = F.normalize(torch.linalg.cross(lookat, up), dim=-1)
    up = F.normalize(torch.linalg.cross(right, lookat), dim=-1)
    c2w3x4 = torch.cat([torch.stack([right, up, -lookat], dim=-1), pos[:, :, None]], dim=-1)
    c2w = torch.cat([c2w3x4, torch.zeros_like(c2w3x4[:, :1])], dim=1)
    c2w[:, 3, 3] = 1.0
    focal = 0.5 * height / torch.tan(0.5 * fovy)
    i, j = torch.meshgrid(torch.arange(width, dtype=dtype) + 0.5, torch.arange(height, dtype=dtype) + 0.5,
                          indexing="xy")
    dirs = torch.stack([(i - width / 2), -(j - height / 2), -torch.ones_like(i)], -1)
    dirs = dirs[None].repeat(n_view, 1, 1, 1)
    dirs[..., :2] = dirs[..., :2] / focal[:, None, None, None]
    rays_d = (dirs[:, :, :, None, :] * c2w[:, None, None, :3, :3]).sum(-1)
    rays_o = c2w[:, None, None, :3, 3].expand(rays_d.shape).contiguous()
    rays_d = F.normalize(rays_d, dim=-1)
    return rays_o, rays_d, c2w, cam_d


def init_mlp_weights(dims: Sequence[int], gen: torch.Generator, dtype=torch.float32) -> List[Tensor]:
    """nn.Linear default init (kaiming_uniform(a=sqrt(5)) => U(-1/sqrt(fan_in), 1/sqrt(fan_in))), bias-free."""
    ws = []
    for din, dout in zip(dims[:-1], dims[1:]):
        bound = 1.0 / math.sqrt(din)
        ws.append(((torch.rand(dout, din, generator=gen, dtype=torch.float64) * 2 - 1) * bound).to(dtype))
    return ws


def synthetic_loss(out: Dict[str, Tensor], proj: Dict[str, Tensor], lambda_sparsity: float = 1.0,
                   lambda_eikonal: float = 1.0, sample_mask: Optional[Tensor] = None) -> Tensor:
    """Fixed scalar loss of SURVEY.md G6: seeded random projections of the image-space outputs
    + sparsity (multiprompt_dual_renderer_multistep_generator.py:635) + eikonal (:696-699).
    sample_mask (N,) of 0/1 (the fuzz only): samples that leave the eikonal mean (their term counts as 0)."""
    loss = 0.0
    for k, p in proj.items():
        loss = loss + (out[k] * p).sum()
    loss = loss + lambda_sparsity * (out["opacity"] ** 2 + 0.01).sqrt().mean()
    eik = (torch.linalg.norm(out["sdf_grad"], ord=2, dim=-1) - 1.0) ** 2
    if sample_mask is not None:
        eik = eik * sample_mask.to(eik.dtype).to(eik.device).reshape(eik.shape)
    loss = loss + lambda_eikonal * eik.mean()
    return loss
