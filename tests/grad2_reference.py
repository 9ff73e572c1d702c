"""CPU reference of the grid-sample double backward (`grad2_2d`, tt_grad2.hip) and the constructed grids its tests use.

reference()      the op by its definition: autograd, twice, through oracle.cpu_ref.grid_sample_gather, in any dtype
                 (float64 is the target, float32 the yardstick of what float32 arithmetic can do).
contributions()  per element of grad_input, from the float64 weights: k, the number of in-bounds taps that land on it,
                 and S_abs, the sum of |t_k go| over them (t_k = dw_k/dx tx + dw_k/dy ty): what the error of a sum
                 accumulated in a narrow format is bounded by.
build_grid()     sample points constructed in pixel space as ip = j + o with an integer j from a named class and
                 o in [0.02, 0.98] ([0.06, 0.94] for half), mapped back through the inverse unnormalisation in float64
                 and rounded to the test dtype.  o is drawn one rounding error inside the [0.01, 0.99] ([0.05, 0.95])
                 that the tests rely on, so no point sits within rounding of a tap boundary, where the second
                 derivative jumps; near_distance() measures what the rounded grid really keeps.  Nothing is filtered.

Classes of j, per axis (taps j and j + 1, `size` texels):
  in        both taps in bounds (size >= 2)
  lo / hi   straddling the low / high border: one tap in bounds, one out
  out-1, out+1, out-3, out+3   fully outside by 1 / by 3 texels
  -1e4, +1e4, -1e30, +1e30     the grid coordinate itself at that value (half: +-1e30 saturates to +-65504, the
                               largest finite half; an infinite coordinate is the non-finite case, tested on its own)
  b0 / b1   border padding only: ip = 0 / ip = size-1 exactly (clip gradient 0 there, ATen's <= / >=), where the grid
            value that gives it is exact in the dtype
With align_corners and size == 1 every finite coordinate unnormalises to ip = 0 (mult = 0): the classes then only
vary the grid value."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import cpu_ref as O  # noqa: E402

MODES = [("zeros", False), ("zeros", True), ("border", False), ("border", True)]
# (N, C, H, W, Ho, Wo): the smallest shapes at which each path of the kernel exists
SHAPES = [(1, 1, 1, 1, 1, 7),  # single texel
          (2, 3, 3, 5, 1, 64),  # odd W, odd H*W, C = 3
          (1, 5, 1, 4, 3, 11),  # H = 1, 2-D grid, C = 5
          (2, 2, 4, 1, 1, 33),  # W = 1
          (3, 4, 7, 9, 1, 33),  # the known-answer shape
          (2, 1, 2, 3, 1, 300)]  # N*M = 600: tail of the third block, batch boundary inside a block
STRIDE_SHAPE = (1, 1, 2, 3, 1, 4096 * 256 + 257)  # past the 4096-block cap: the grid-stride loop, and contention
STRIDE_MODES = [("zeros", False), ("border", True)]
CONTENTION_SHAPE = (1, 2, 3, 5, 1, 4096)  # every point in one cell: 4096 packed-half adds per texel
WRAPPER_SHAPE = (2, 3, 3, 5, 3, 11)  # the autograd wrapper's second-order graph, a true 2-D grid
GRADGRAD_SHAPE = (1, 2, 3, 4, 2, 3)  # torch.autograd.gradgradcheck
DTYPES = {"float32": torch.float32, "float64": torch.float64, "float16": torch.float16}
HALF_MAX = 65504.0

INSIDE = ("in",)
STRADDLE = ("lo", "hi")
NEAR_OUT = ("out-1", "out+1", "out-3", "out+3")
FAR_OUT = ("-1e4", "+1e4", "-1e30", "+1e30")
OUTSIDE = NEAR_OUT + FAR_OUT
EXACT = ("b0", "b1")
_FAR = {"-1e4": -1e4, "+1e4": 1e4, "-1e30": -1e30, "+1e30": 1e30}
CLASSES = INSIDE + STRADDLE + OUTSIDE + EXACT


def among(ids, names):
    """Bool mask: which of the class ids (as build_grid returns them) belong to one of `names`."""
    return torch.isin(ids, torch.tensor([CLASSES.index(c) for c in names], dtype=torch.long))


def names(ids):
    """The set of class names that occur among the class ids."""
    return {CLASSES[i] for i in torch.unique(ids).tolist()}


def margin(dtype):
    """The distance from an integer pixel coordinate that build_grid() promises after rounding to `dtype`."""
    return 0.05 if dtype == torch.float16 else 0.01


def unnormalize(g, size, align_corners):
    """ATen grid_sampler_unnormalize, before any clip (float64 in, float64 out)."""
    if align_corners:
        return ((g + 1) / 2) * (size - 1)
    return ((g + 1) * size - 1) / 2


def normalize(ip, size, align_corners):
    """The inverse of unnormalize in float64.  With align_corners and size == 1 there is none (every g gives ip = 0):
    the other convention's inverse then merely spreads the grid values."""
    if align_corners and size > 1:
        return 2 * ip / (size - 1) - 1
    return (2 * ip + 1) / size - 1


def _round(g, dtype):
    if dtype == torch.float16:
        g = g.clamp(-HALF_MAX, HALF_MAX)
    return g.to(dtype).double()


def axis_classes(size, padding_mode, align_corners, dtype):
    """The classes that exist for an axis of `size` texels, in the order build_grid() deals them out."""
    names = list(STRADDLE + NEAR_OUT + FAR_OUT)
    if size >= 2:
        names.insert(0, "in")
    if padding_mode == "border":
        for name, ip in (("b0", 0.0), ("b1", float(size - 1))):
            g = _round(torch.tensor(normalize(ip, size, align_corners), dtype=torch.float64), dtype)
            # exact in the dtype, and exact in the float32 the kernel computes half in
            if float(unnormalize(g, size, align_corners)) == ip and \
                    float(unnormalize(g.float(), size, align_corners)) == ip:
                names.append(name)
    return names


def grid_args(shape):
    """How build_grid() is called for the shapes above that do not take every class in equal shares."""
    no_kink = INSIDE + STRADDLE + OUTSIDE
    if shape == STRIDE_SHAPE:  # mostly in bounds, so that each of the 6 texels collects well over 100,000 adds
        return dict(p_first=0.6)
    if shape == CONTENTION_SHAPE:
        return dict(x_classes=INSIDE, y_classes=INSIDE, cell=(2, 1))
    if shape == GRADGRAD_SHAPE:  # finite differences: not on the clip's kink
        return dict(x_classes=no_kink, y_classes=no_kink)
    return {}


def _axis(ids, size, align_corners, dtype, gen, j_cell=None):
    """One coordinate per class id of `ids`, float64 holding values of `dtype`; j_cell fixes the j of class "in"."""
    P = len(ids)
    lo = margin(dtype) + 0.01
    o = lo + (1 - 2 * lo) * torch.rand(P, generator=gen, dtype=torch.float64)
    j_in = torch.randint(0, max(size - 1, 1), (P,), generator=gen).double()
    if j_cell is not None:
        j_in = torch.full_like(j_in, float(j_cell))
    base = {"lo": -1, "hi": size - 1, "out-1": -2, "out+1": size, "out-3": -4, "out+3": size + 2}
    j = torch.tensor([float(base.get(c, 0)) for c in CLASSES], dtype=torch.float64)[ids]
    ip = torch.where(ids == CLASSES.index("in"), j_in, j) + o
    ip = torch.where(ids == CLASSES.index("b0"), torch.zeros_like(ip), ip)
    ip = torch.where(ids == CLASSES.index("b1"), torch.full_like(ip, float(size - 1)), ip)
    g = normalize(ip, size, align_corners)
    for c, v in _FAR.items():
        g = torch.where(ids == CLASSES.index(c), torch.full_like(g, v), g)
    return _round(g, dtype)


def build_grid(N, H, W, Ho, Wo, padding_mode, align_corners, dtype, seed=0, x_classes=None, y_classes=None,
               either=None, p_first=None, cell=None):
    """(grid (N,Ho,Wo,2) float64 holding values of `dtype`, the x classes, the y classes), the classes as (P,) ids into
    CLASSES in point order (n, ho, wo); see among() and names().  The first points walk the diagonal of the class
    table (both axes in the same class), the rest draw a class per axis at random; `p_first` gives the first class of
    each axis that probability instead of an equal share.  x_classes / y_classes restrict the classes of an axis.  either=(names): every point has a class of `names`
    on at least one axis (which one alternates), e.g. OUTSIDE: every point fully outside.  cell=(jx, jy) puts every
    point of class "in" into that one cell."""
    gen = torch.Generator().manual_seed(seed)
    P = N * Ho * Wo
    out = []
    for axis, (size, allowed) in enumerate(((W, x_classes), (H, y_classes))):
        avail = [c for c in axis_classes(size, padding_mode, align_corners, dtype) if allowed is None or c in allowed]
        if p_first is None:
            pick = torch.randint(0, len(avail), (P,), generator=gen)
        else:
            rest = torch.randint(1, max(len(avail), 2), (P,), generator=gen).clamp(max=len(avail) - 1)
            pick = torch.where(torch.rand(P, generator=gen) < p_first, torch.zeros(P, dtype=torch.long), rest)
        pick[:min(P, len(avail))] = torch.arange(min(P, len(avail)))
        if either is not None:
            forced = torch.tensor([i for i, c in enumerate(avail) if c in either], dtype=torch.long)
            sel = torch.nonzero(torch.arange(P) % 2 == axis).reshape(-1)
            pick[sel] = forced[torch.arange(len(sel)) % len(forced)]
        out.append(torch.tensor([CLASSES.index(c) for c in avail], dtype=torch.long)[pick])
    gx = _axis(out[0], W, align_corners, dtype, gen, None if cell is None else cell[0])
    gy = _axis(out[1], H, align_corners, dtype, gen, None if cell is None else cell[1])
    return torch.stack([gx, gy], -1).reshape(N, Ho, Wo, 2), out[0], out[1]


def near_distance(grid, H, W, align_corners):
    """min over the coordinates of `grid` that lie within 5 texels of the image of |ip - nearest integer|, the pixel
    coordinate from float64 unnormalisation of the (rounded) grid values; inf when there is none.  An axis with
    align_corners and size == 1 has ip = 0 identically and d ip / d g = 0: no tap boundary can be crossed there."""
    best = float("inf")
    for axis, size in ((0, W), (1, H)):
        if align_corners and size == 1:
            continue
        ip = unnormalize(grid[..., axis].double().reshape(-1), size, align_corners)
        ip = ip[(ip > -5) & (ip < size + 4)]
        if ip.numel():
            best = min(best, float((ip - torch.round(ip)).abs().min()))
    return best


def sample(inp, grid, padding_mode, align_corners):
    """The oracle's bilinear sampling in the op's layout: inp (N,C,H,W), grid (N,Ho,Wo,2) -> (N,C,Ho,Wo)."""
    N, C = inp.shape[:2]
    Ho, Wo = grid.shape[1:3]
    out = O.grid_sample_gather(inp, grid.reshape(N, Ho * Wo, 2), padding_mode, align_corners)  # (N, M, C)
    return out.permute(0, 2, 1).reshape(N, C, Ho, Wo)


def first_backward(go, inp, grid, padding_mode, align_corners, create_graph=False):
    """(grad_input, grad_grid) of the sampling: what aten::grid_sampler_2d_backward computes."""
    inp = inp if inp.requires_grad else inp.detach().requires_grad_(True)
    grid = grid if grid.requires_grad else grid.detach().requires_grad_(True)
    out = sample(inp, grid, padding_mode, align_corners)
    return torch.autograd.grad(out, (inp, grid), grad_outputs=go, create_graph=create_graph)


def reference(g2i, g2g, go, inp, grid, padding_mode, align_corners, dtype=torch.float64):
    """(grad_grad_output, grad_input, grad_grid) of grad2_2d by its definition, evaluated in `dtype`:
    out = gather(inp, grid); (gi1, gg1) = grad(out, (inp, grid), go, create_graph); L = <gi1, g2i> + <gg1, g2g>;
    the outputs are grad(L, (go, inp, grid)).  padding_mode "zeros" / "border" or 0 / 1."""
    if not isinstance(padding_mode, str):
        padding_mode = ("zeros", "border")[int(padding_mode)]
    g2i, g2g = g2i.detach().to(dtype), g2g.detach().to(dtype)
    go, inp, grid = (t.detach().to(dtype).requires_grad_(True) for t in (go, inp, grid))
    gi1, gg1 = first_backward(go, inp, grid, padding_mode, align_corners, create_graph=True)
    L = (gi1 * g2i).sum() + (gg1 * g2g).sum()
    ggo, gi, gg = torch.autograd.grad(L, (go, inp, grid), allow_unused=True)
    gi = torch.zeros_like(inp) if gi is None else gi
    gg = torch.zeros_like(grid) if gg is None else gg
    return ggo.detach(), gi.detach(), gg.detach()


def contributions(g2g, go, grid, shape, padding_mode, align_corners):
    """(k, S_abs), each shaped like grad_input = `shape` (N,C,H,W), from the float64 weights: grad_input[n,c,texel] is
    the sum over the points of batch n and their in-bounds taps on that texel of t_k go[n,c,point], with
    t_k = dw_k/dgx g2g.x + dw_k/dgy g2g.y.  k counts those terms, S_abs sums their absolute values."""
    if not isinstance(padding_mode, str):
        padding_mode = ("zeros", "border")[int(padding_mode)]
    N, C, H, W = shape
    g = grid.detach().double().reshape(N, -1, 2).requires_grad_(True)
    tg = g2g.detach().double().reshape(N, -1, 2)
    go = go.detach().double().reshape(N, C, -1)
    k = torch.zeros(N, H * W, dtype=torch.float64)
    s_abs = torch.zeros(N, C, H * W, dtype=torch.float64)
    for cy, cx, w, inb in O.bilinear_corners(g, H, W, padding_mode, align_corners):
        (dw,) = torch.autograd.grad((w * inb.double()).sum(), g, retain_graph=True)
        t = (dw * tg).sum(-1)  # (N, M)
        idx = (cy.detach().clamp(0, H - 1) * W + cx.detach().clamp(0, W - 1)).long()
        k.scatter_add_(1, idx, inb.double())
        term = (t[:, None, :] * go).abs() * inb.double()[:, None, :]
        s_abs.scatter_add_(2, idx[:, None, :].expand(-1, C, -1), term)
    return k[:, None, :].expand(-1, C, -1).reshape(N, C, H, W).clone(), s_abs.reshape(N, C, H, W)


def operands(shape, grid, dtype, seed=0):
    """Random (g2i, g2g, go, inp) for `shape` = (N,C,H,W,Ho,Wo) and `grid`, float64 holding values of `dtype`."""
    N, C, H, W, Ho, Wo = shape
    gen = torch.Generator().manual_seed(1000 + seed)
    mk = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).to(dtype).double()  # noqa: E731
    return mk(N, C, H, W), mk(N, Ho, Wo, 2), mk(N, C, Ho, Wo), mk(N, C, H, W)


def error32(ops, grid, padding_mode, align_corners, want):
    """e_ref32 per output: max |float32 evaluation - float64 evaluation| of the reference on the same operands."""
    got = reference(*ops, grid, padding_mode, align_corners, torch.float32)
    return [float((a.double() - b).abs().max()) for a, b in zip(got, want)]


def bar32(e_ref32, want):
    """The float32 bar of one output, max-abs: 4x what the float32 reference loses, or 4 ulp of the largest value."""
    return max(4 * e_ref32, 2.0 ** -22 * float(want.abs().max()))


@functools.lru_cache(maxsize=None)
def case(shape, padding_mode, align_corners, dtype_name, seed=0, **how):
    """One test case, computed once per session and shared: dict with grid, ops = (g2i, g2g, go, inp) (float64 holding
    values of the dtype), want (float64 reference), e32 (e_ref32 per output; None for float64), k and S_abs."""
    dtype = DTYPES[dtype_name]
    N, C, H, W, Ho, Wo = shape
    how = how or grid_args(shape)
    grid, xc, yc = build_grid(N, H, W, Ho, Wo, padding_mode, align_corners, dtype, seed, **how)
    ops = operands(shape, grid, dtype, seed)
    want = reference(*ops, grid, padding_mode, align_corners, torch.float64)
    e32 = None if dtype == torch.float64 else error32(ops, grid, padding_mode, align_corners, want)
    k, s_abs = contributions(ops[1], ops[2], grid, (N, C, H, W), padding_mode, align_corners)
    return dict(grid=grid, ops=ops, want=want, e32=e32, k=k, s_abs=s_abs, x_classes=xc, y_classes=yc)
