"""Shared by the ray-march tests (CPU only): the oracle march built from the oracle's own pieces, two input families that
keep a ray alive up to a chosen sample, and the element-wise bars measured from the oracle's fp32 evaluations.

The march (tt_march.hip) walks a ray 64 samples per pass; the forward's running transmittance and the backward's
reverse-scan carry link the passes.  Noise inputs make every ray opaque inside the first pass, so everything a later
pass computes is below any absolute bar.  The families here put the surface where the hand-over happens:

  late(S)   one ray per crossing index c: transparent (alpha ~ 1e-5) up to sample c, the surface ON a pass seam
            (c in {1, S-2, S-1} and {b-2 .. b+1} for every multiple b of 64), plus one empty ray.
  edges(S)  hand-built, exactly representable rays: cos(normal, ray) exactly 0 / -1 / +1, zero-length intervals,
            sdf == 0, a saturated sample (alpha == 1, T == 0 after it), features +-100.

march() is the oracle's math from O._normalize, O.get_alpha, O.render_weight_from_alpha and O.sigmoid_mipnerf, so that
O.alt_order(1 .. 3) gives three more valid fp32 evaluations of it (other logistic, other normalisation, the
transmittance recurrence, other summation orders).  inv_std is one leaf PER RAY: the loss separates per ray, so autograd
returns d loss / d inv_std per ray.

allowance(): e32_ray = the largest error against float64 of any of the four fp32 evaluations on that ray (over the
elements of the population named).  RTOL_ELEM, ATOL_ELEM: tests/parity.py.

  output / population                          bar of an element                                 e32_ray, max|ref| over
  weights, trans                               max(4 e32_ray, 2e-6)                              the ray's samples
  opacity .. normal_acc                        max(4 e32_ray, 2e-6)   (use_volsdf: 2e-6 x        the ray's elements
                                               max(1, max|ref|), the rule of its older test)
  ws, rows with a non-zero sdf_grad ("live")   max(4 e32_ray, RTOL |ref| + ATOL max|ref|)        those rows
  ws, zero-sdf_grad rows, sdf_grad columns     the same                                          the zero-sdf_grad rows,
      ("eps": gradient x 1e12, F.normalize eps)                                                  all four columns
  ws, zero-sdf_grad rows, d/d sdf column       the same                                          the live rows and these
      ("eps_sdf": carries no 1e12)                                                               elements
  g_inv_std_rays                               max(4 e32_ray, RTOL |ref| + ATOL max|ref|)        the ray / all rays

The issue's two row populations are "live" and "eps".  "eps_sdf" splits the d/d sdf column off the second: measured by
the bar of the 1e12-scaled columns beside it, it would not be checked at all; its bar is never wider than that one."""
import functools

import torch

from oracle import cpu_ref as O
from parity import ATOL_ELEM, RTOL_ELEM

S_LIST = (7, 64, 65, 128, 129, 193, 256, 257, 300)
EDGE_S = (7, 65, 129, 257, 300)  # one size per kernel form, ragged last pass, + the 2-pass form at its seam
INV_STD, RATIO = 40.0, 0.3
# use_volsdf: inv_std ~ 0.5 x S / (t range), so that alpha = |dt| x density stays of order one (above 1 on some samples:
# not clipped), the regime the switch is usable in
VOLSDF_INV_STD = {7: 1.0, 64: 8.0, 65: 9.0, 128: 18.0, 129: 18.0, 193: 27.0, 256: 36.0, 257: 36.0, 300: 43.0}
VOLSDF_ABOVE_CLAMP = (65, 95.0)  # one extra case above the clamp at 80: d / d inv_std is exactly 0 there
RAY_KEYS = ("opacity", "depth", "rgb_fg", "z_variance", "normal_acc")
FWD_KEYS = RAY_KEYS + ("weights", "trans")
UP_KEYS = RAY_KEYS + ("weights",)
PREFIX_S = (63, 64, 65, 128, 129, 256, 257)


def form_of(S):
    return "reg1" if S <= 64 else "reg2" if S <= 128 else "reg4" if S <= 256 else "stream"


# 7 + S, except where that draw misses the coverage condition of tests/test_march_reference_host.py: a last pass of ONE sample
# (S = 129, 257) needs an interval long enough to hold a quarter of the ray's weight on its own
SEEDS = {129: 4136, 257: 16264}


def seed_of(S):
    return SEEDS.get(S, 7 + S)


def crossings(S):
    c = {1, S - 2, S - 1}
    for b in range(64, S + 2, 64):
        c |= {b - 2, b - 1, b, b + 1}
    return sorted(i for i in c if 0 < i < S)


def late(S, seed=None):
    """(rd, ts, te, sdf, sdf_grad, feat) in float32 and the crossing index of each ray (-1: the empty ray)."""
    cs = crossings(S)
    n = len(cs) + 1
    g = torch.Generator().manual_seed(seed_of(S) if seed is None else seed)
    rd = O._normalize(torch.randn(n, 3, generator=g))
    edges = torch.sort(torch.rand(n, S + 1, generator=g) * 3.5 + 0.1, dim=1).values
    ts, te = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    tm, dt = ((ts + te) / 2).double(), (te - ts).double()
    u = torch.rand(n, S, generator=g).double()
    c = torch.tensor(cs)
    r = torch.arange(n - 1)
    sdf = tm[r, c].unsqueeze(1) - tm[:-1] + 0.3 * dt[r, c].unsqueeze(1) * (u[:-1] - 0.5)
    sdf = torch.cat([sdf, 0.5 + 0.1 * u[-1:]], dim=0).float().reshape(-1, 1)
    ridx = torch.arange(n).repeat_interleave(S)
    sdf_grad = -rd[ridx] * (0.8 + 0.4 * torch.rand(n * S, 1, generator=g)) + 0.3 * torch.randn(n * S, 3, generator=g)
    sdf_grad[::17] = 0.0  # F.normalize eps branch
    feat = torch.randn(n * S, 3, generator=g) * 2
    return (rd, ts, te, sdf, sdf_grad, feat), cs + [-1]


EDGE_RAYS = ("cos0", "cos-1", "cos+1", "dt0", "sdf0", "saturated", "feat100")


def edges(S):
    """Seven rays along rd = (0, 0, 1) on the grid t = 0.5 + i / 64; every input is a small dyadic number.  Returns the
    float32 inputs and the index of the saturated sample of ray 5."""
    n, h = len(EDGE_RAYS), 1.0 / 64
    c0 = S // 2
    sat = 64 if S > 65 else S // 2  # the saturated sample: the first of the second pass where there is one
    i = torch.arange(S, dtype=torch.float32)
    rd = torch.tensor([[0.0, 0.0, 1.0]]).repeat(n, 1)
    step = torch.ones(n, S)
    for j in {1, c0, min(64, S - 1)}:
        step[3, j] = 0.0  # te == ts
    e = 0.5 + h * torch.cat([torch.zeros(n, 1), torch.cumsum(step, dim=1)], dim=1)
    ts, te = e[:, :-1].contiguous(), e[:, 1:].contiguous()
    # crosses zero a quarter step before sample c0 and levels off 8 steps inside: deeper, 1 - alpha falls to ~1e-13 without
    # reaching 0 and cumprod's backward (the primary evaluation) divides by it -- exact saturation is ray 5's business.
    # (The quarter step keeps every logistic argument, sdf +- ic dt / 2, away from exactly 0: alt_order(2)'s two-branch
    # logistic goes through |x|, whose autograd derivative at 0 is 0, so that evaluation is not valid there.  sdf == 0 is
    # ray 4, where the interval ends are +- dt / 2.)
    sdf = ((c0 - i - 0.25) * h).clamp_min(-8.25 * h).repeat(n, 1)
    sdf[4] = 0.0
    sdf[5] = torch.where(i < sat, 10.0, -10.0)  # sigmoid(-400) = 0 in fp32: alpha clips to exactly 1 at sample `sat`
    grad = torch.tensor([[0.0, 0.0, -3.0]]).repeat(n, 1)
    grad[0] = torch.tensor([0.0, 2.0, 0.0])  # cos = 0: the kink of relu(-cos)
    grad[2] = torch.tensor([0.0, 0.0, 0.5])  # cos = +1: the kink of relu(0.5 - 0.5 cos)
    sdf_grad = grad.repeat_interleave(S, dim=0)
    feat = (((torch.arange(n * S * 3) % 5).float() - 2.0) * 0.5).reshape(n, S, 3)
    feat[6] = torch.where((torch.arange(S * 3) % 2 == 0).reshape(S, 3), 100.0, -100.0)
    return (rd, ts, te, sdf.reshape(-1, 1).contiguous(), sdf_grad.contiguous(), feat.reshape(-1, 3).contiguous()), sat


def _accumulate(src, n_rays, S):
    """nerfacc.accumulate_along_rays on the dense layout, in the summation order of the oracle's current evaluation."""
    src = src.reshape(n_rays, S, -1)
    lv = O._ALT_ORDER
    if lv == 1:  # far-to-near, one sample at a time
        acc = src[:, S - 1]
        for k in range(S - 2, -1, -1):
            acc = acc + src[:, k]
        return acc
    if lv == 2 and S > 1:  # near half + far half
        return src[:, :S // 2].sum(dim=1) + src[:, S // 2:].sum(dim=1)
    if lv == 3:  # chunks of 8 samples, chunk sums added near-to-far
        acc = None
        for k0 in range(0, S, 8):
            part = src[:, k0:k0 + 8].sum(dim=1)
            acc = part if acc is None else acc + part
        return acc
    return src.sum(dim=1)


def march(x, inv_std_samples, ratio=RATIO, use_volsdf=False):
    """The march boundary on per-sample sdf / sdf_grad / features; inv_std_samples (n_rays S, 1): one value per sample."""
    rd, ts, te, sdf, sdf_grad, feat = x
    n_rays, S = ts.shape
    tm = ((ts + te) / 2.0).reshape(-1, 1)
    dt = (te - ts).reshape(-1, 1)
    ridx = torch.arange(n_rays).repeat_interleave(S)
    normal = O._normalize(sdf_grad)
    alpha = O.get_alpha(sdf, normal, rd[ridx], dt, inv_std_samples, ratio, use_volsdf)
    w2, tr2 = O.render_weight_from_alpha(alpha.reshape(n_rays, S))
    w = w2.reshape(-1, 1)
    acc = lambda v: _accumulate(w if v is None else w * v, n_rays, S)  # noqa: E731
    depth = acc(tm)
    return {"opacity": acc(None), "depth": depth, "rgb_fg": acc(O.sigmoid_mipnerf(feat)),
            "z_variance": acc((tm - depth[ridx]) ** 2), "normal_acc": acc(normal), "weights": w,
            "trans": tr2.reshape(-1, 1)}


def upstream(x32):
    """One fixed set of upstream gradients for every output but trans (float32 values)."""
    n_rays, S = x32[1].shape
    g = torch.Generator().manual_seed(5)
    shape = {"opacity": (n_rays, 1), "depth": (n_rays, 1), "rgb_fg": (n_rays, 3), "z_variance": (n_rays, 1),
             "normal_acc": (n_rays, 3), "weights": (n_rays * S, 1)}
    return {k: torch.randn(shape[k], generator=g) for k in UP_KEYS}


def evaluate(x32, dtype, level, inv_std, use_volsdf=False, ups=None):
    """Forward outputs, the backward rows `ws` (n S, 4) = (d/d sdf, d/d sdf_grad), `gk` (n,) = d loss / d inv_std per
    ray and `gk_samples` (n S, 1), each sample's share of it (inv_std is a leaf per sample; the loss separates per ray, so
    a ray's shares add up to its gradient), of the oracle's evaluation `level` (0: primary, 1 .. 3: O.alt_order) in
    `dtype`, as float64 tensors.  The inputs are copied: x32 stays plain data."""
    x = [t.detach().clone().to(dtype) for t in x32]
    for t in x[3:5]:
        t.requires_grad_(True)
    n_rays, S = x[1].shape
    k = torch.full((n_rays * S, 1), float(inv_std), dtype=dtype, requires_grad=True)
    ups = upstream(x32) if ups is None else ups
    with O.alt_order(level):
        o = march(x, k, use_volsdf=use_volsdf)
        loss = sum((o[n] * ups[n].to(dtype)).sum() for n in UP_KEYS)
        gs, gg, gk = torch.autograd.grad(loss, [x[3], x[4], k])
    res = {n: v.detach().double() for n, v in o.items()}
    res["ws"] = torch.cat([gs, gg], dim=1).double()
    res["gk"] = gk.reshape(n_rays, S).sum(dim=1).double()  # summed in `dtype`, as autograd sums into a per-ray leaf
    res["gk_samples"] = gk.double()
    return res


def logistic_argument(x32, inv_std, ratio=RATIO):
    """The larger of the two NeuS logistic arguments (estimated sdf at the interval's ends x inv_std) per sample (n S,)."""
    rd, ts, te, sdf, sdf_grad, _ = [t.detach().double() for t in x32]
    n_rays, S = ts.shape
    cos = (rd.repeat_interleave(S, dim=0) * O._normalize(sdf_grad)).sum(-1, keepdim=True)
    ic = torch.relu(-cos * 0.5 + 0.5) * (1.0 - ratio) + torch.relu(-cos) * ratio
    return ((sdf + ic * (te - ts).reshape(-1, 1) * 0.5) * inv_std).reshape(-1)


def _populations(x32):
    """The backward-row populations as (elements the bar applies to, elements its e32_ray and max|ref| come from)."""
    zero = (x32[4] == 0).all(dim=1, keepdim=True)
    col0 = torch.tensor([[True, False, False, False]])
    live, eps = (~zero).expand(-1, 4), zero.expand(-1, 4)
    return {"live": (live, live), "eps": (eps & ~col0, eps), "eps_sdf": (eps & col0, live | (eps & col0))}


def _e32_ray(key, ref64, evals32, n_rays, mask=None):
    """Per ray, the largest error against float64 of any fp32 evaluation (over the elements of `mask`).  An evaluation
    without a value on an element does not vote there: alt_order(3) normalises as x / sqrt(|x|^2), whose autograd
    derivative at x = 0 is 0 / 0 -- the sdf_grad columns of the zero-sdf_grad rows."""
    e = torch.stack([torch.nan_to_num((ev[key] - ref64[key]).abs(), nan=0.0) for ev in evals32]).amax(dim=0)
    return (e if mask is None else e * mask).reshape(n_rays, -1).amax(dim=1)


def _forward_bars(key, ref64, evals32, ray_index, n_rays, scale_floor):
    ref = ref64[key]
    floor = 2e-6 * (max(1.0, ref.abs().max().item()) if scale_floor and key in RAY_KEYS else 1.0)
    per_ray = (4 * _e32_ray(key, ref64, evals32, n_rays)).clamp_min(floor)
    return (per_ray[ray_index] if key in ("weights", "trans") else per_ray).reshape(-1, 1).expand_as(ref).clone()


def _elem_bars(key, ref64, evals32, n_rays, mask=None):
    """max(4 e32_ray, RTOL_ELEM |ref| + ATOL_ELEM max|ref|) per ray (one row per ray), statistics over `mask`."""
    ref = ref64[key].reshape(n_rays, -1)
    top = (ref.abs() if mask is None else ref.abs() * mask.reshape(n_rays, -1)).max()
    return torch.maximum(4 * _e32_ray(key, ref64, evals32, n_rays, mask).reshape(-1, 1), RTOL_ELEM * ref.abs() + ATOL_ELEM * top)


def allowance(ref64, evals32, ray_index, populations=None, scale_floor=False):
    """The bar of every element of every output (a dict of tensors shaped like ref64's): the table of the module docstring."""
    n_rays = int(ray_index.max()) + 1
    bars = {key: _forward_bars(key, ref64, evals32, ray_index, n_rays, scale_floor) for key in FWD_KEYS}
    ref = ref64["ws"]
    everything = torch.ones_like(ref, dtype=torch.bool)
    bars["ws"] = torch.zeros_like(ref)
    for applies_to, stats in (populations or {"all": (everything, everything)}).values():
        if applies_to.any():
            bars["ws"] = torch.where(applies_to, _elem_bars("ws", ref64, evals32, n_rays, stats).reshape(ref.shape), bars["ws"])
    bars["gk"] = _elem_bars("gk", ref64, evals32, n_rays).reshape(-1)
    return bars


def ratios(got, ref64, bars):
    """error / allowance per element (0 / 0 = 0: an exact value under a zero bar passes)."""
    e = (got.double().reshape(ref64.shape) - ref64).abs()
    r = e / bars
    return torch.where(e == 0, torch.zeros_like(r), r)


class Case:
    """Inputs, float64 reference, the four fp32 evaluations and the bars of one (family, S, use_volsdf[, inv_std])."""

    def __init__(self, family, S, use_volsdf=False, inv_std=None):
        self.family, self.S, self.use_volsdf = family, S, use_volsdf
        self.sat = None
        if family == "late":
            self.x32, self.crossing = late(S)
        else:
            self.x32, self.sat = edges(S)
        self.n_rays = self.x32[1].shape[0]
        self.inv_std = inv_std if inv_std is not None else VOLSDF_INV_STD[S] if use_volsdf else INV_STD
        self.mode = "neus" if not use_volsdf else "volsdf" if inv_std is None else f"volsdf{inv_std:g}"
        self.ray_index = torch.arange(self.n_rays).repeat_interleave(S)
        self.ups = upstream(self.x32)
        # edges: the recurrence form (cumprod's backward divides by 1 - alpha = 0 on the saturated ray)
        self.ref64 = evaluate(self.x32, torch.float64, 0 if family == "late" else 3, self.inv_std, use_volsdf, self.ups)
        self.evals32 = [evaluate(self.x32, torch.float32, lv, self.inv_std, use_volsdf, self.ups) for lv in range(4)]
        self.populations = _populations(self.x32)
        self.bars = self.bars_from(self.evals32)

    def bars_from(self, evals32):
        return allowance(self.ref64, evals32, self.ray_index, self.populations, scale_floor=self.use_volsdf)

    def where(self, key, flat_index):
        """ray / sample / pass of an element of output `key`."""
        per_ray = key in RAY_KEYS + ("gk",)
        ncol = self.ref64[key].numel() // (self.n_rays if per_ray else self.n_rays * self.S)
        row, col = divmod(flat_index, ncol)
        ray, s = (row, None) if per_ray else divmod(row, self.S)
        tag = self.crossing[ray] if self.family == "late" else EDGE_RAYS[ray]
        at = "" if per_ray else f" sample {s} pass {s // 64} lane {s % 64}"
        return f"ray {ray} (crossing {tag}){at} col {col}"

    def worst(self, key, got, rays=None):
        """(largest error / allowance, description of where) of `got` against the reference; rays: a subset."""
        ref, bars = self.ref64[key], self.bars[key]
        if rays is not None:
            rows = rays if key in RAY_KEYS + ("gk",) else (rays.reshape(-1, 1) * self.S + torch.arange(self.S)).reshape(-1)
            ref, bars = ref[rows], bars[rows]
        r = ratios(got, ref, bars).reshape(-1)
        r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
        i = int(r.argmax())
        if rays is not None:  # back to an index into the whole tensor
            ncol = r.numel() // rows.numel()
            i = int(rows[i // ncol]) * ncol + i % ncol
        return float(r.max()), self.where(key, i)

    def check(self, key, got, rays=None, tag="hip"):
        worst, at = self.worst(key, got, rays)
        print(f"march {self.family} S={self.S} {form_of(self.S)} {self.mode} {key}: "
              f"{tag} error/allowance {worst:.3f} at {at}")
        assert worst <= 1.0, (self.family, self.S, key, worst, at)
        return worst


@functools.lru_cache(maxsize=None)
def case(family, S, use_volsdf=False, inv_std=None):
    return Case(family, S, use_volsdf, inv_std)


def coverage(S, ref64, x32):
    """Per 64-sample pass of the float64 reference: the largest T at the pass's first sample, the largest weight mass
    inside the pass over the rays with T >= 0.5 there, and the pass's largest |ws| over the tensor's."""
    n_rays = ref64["opacity"].shape[0]
    T = ref64["trans"].reshape(n_rays, S)
    w = ref64["weights"].reshape(n_rays, S)
    ws = ref64["ws"].abs().reshape(n_rays, S, 4)
    live = ~(x32[4] == 0).all(dim=1).reshape(n_rays, S, 1)  # not the 1e12-scaled rows: they would set the tensor's maximum
    ws = (ws * live).amax(dim=2)
    rows = []
    for b in range(0, S, 64):
        mass = w[:, b:b + 64].sum(dim=1)
        alive = T[:, b] >= 0.5
        rows.append({"pass": b // 64, "T_start": float(T[:, b].max()),
                     "mass": float((mass * alive).max()), "ws_frac": float(ws[:, b:b + 64].max() / ws.max())})
    return rows
