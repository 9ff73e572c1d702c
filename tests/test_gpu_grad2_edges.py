"""tt_grad2.hip (the drop-in for the reference's `grad2_2d`) element by element against its definition, at its edges.

The reference is tests/grad2_reference.py: autograd twice through the gather-based oracle, float64 for the target and
float32 for the yardstick, on constructed points that keep their distance from the tap boundaries (checked on the host,
tests/test_grad2_reference_host.py, where the reference also meets finite differences and the known-answer file).

Bars, per output, max-abs over elements:
  float64  1e-12 max|want|
  float32  max(4 e_ref32, 2^-22 max|want|), e_ref32 = what the float32 evaluation of the reference loses
  float16  operands rounded to half first (the reference consumes those values in float64).  grad_grad_output and
           grad_grid are computed in float32 and rounded once on store: 2^-11 |want| + the float32 bar, per element.
           grad_input takes one half rounding per contribution and one per atomic add: (k + 2) 2^-11 S_abs + the
           float32 bar, per element, with k and S_abs from the reference.
Every case prints e_hip and e_ref32 (pytest -s; profiles/grad2_edges.txt holds one such printout)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad2_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("ggo", "gi", "gg")
PAD = {"zeros": 0, "border": 1}
EDGE_SHAPE = R.SHAPES[1]  # (2,3,3,5,1,64): odd W, odd H*W


@pytest.fixture(scope="module")
def gsg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from triplaneturbo_amd import grid_sample_gradfix
    return grid_sample_gradfix


def _gpu(c, dtype):
    """(g2i, g2g, go, inp, grid) of a case on the GPU in `dtype` (the case holds values of that dtype already)."""
    return [t.to(dtype).cuda() for t in (*c["ops"], c["grid"])]


def _bars(want, e32, k, s_abs, dtype):
    """The three bars: a float for float64 / float32, a per-element tensor for half."""
    if dtype == torch.float64:
        return [1e-12 * float(w.abs().max()) for w in want]
    b32 = [R.bar32(e, w) for e, w in zip(e32, want)]
    if dtype == torch.float32:
        return b32
    u = 2.0 ** -11
    return [u * want[0].abs() + b32[0], (k + 2) * u * s_abs + b32[1], u * want[2].abs() + b32[2]]


def _check(label, got, want, e32, bars, rows=None):
    """Print e_hip / e_ref32 per output, then hold every element (of the point rows `rows`, a bool mask over the
    points (N,Ho,Wo), where given) to its bar."""
    bad = []
    for i, name in enumerate(NAMES):
        err = (got[i].detach().cpu().double() - want[i]).abs()
        bar = bars[i] if torch.is_tensor(bars[i]) else torch.full_like(err, bars[i])
        if rows is not None and name != "gi":
            m = rows[:, None].expand_as(err) if name == "ggo" else rows[..., None].expand_as(err)
            err, bar = err[m], bar[m]
        e_ref = "-" if e32 is None else f"{e32[i]:.3e}"
        print(f"grad2 {label} {name}: e_hip={float(err.max()):.3e} e_ref32={e_ref} bar={float(bar.max()):.3e} "
              f"max|want|={float(want[i].abs().max()):.3e}")
        if not bool((err <= bar).all()):
            bad.append((name, float(err.max()), float((err - bar).max())))
    assert not bad, (label, bad)


def _case_check(gsg, shape, padding_mode, align_corners, dtype_name, **how):
    dtype = R.DTYPES[dtype_name]
    c = R.case(shape, padding_mode, align_corners, dtype_name, **how)
    got = gsg.grad2_2d(*_gpu(c, dtype), PAD[padding_mode], align_corners)
    assert all(g.dtype == dtype for g in got)
    label = f"{'x'.join(map(str, shape))} {padding_mode} align={int(align_corners)} {dtype_name}"
    _check(label, got, c["want"], c["e32"], _bars(c["want"], c["e32"], c["k"], c["s_abs"], dtype))
    return c, got


# ---- every shape x padding x align_corners x dtype, all three outputs ----
@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_matches_reference(gsg, shape, padding_mode, align_corners, dtype_name):
    c, got = _case_check(gsg, shape, padding_mode, align_corners, dtype_name)
    N, C, H, W, Ho, Wo = shape
    assert got[0].shape == (N, C, Ho, Wo) and got[1].shape == (N, C, H, W) and got[2].shape == (N, Ho, Wo, 2)
    # the grid really holds what the shape is there for
    classes = R.names(c["x_classes"]) | R.names(c["y_classes"])
    assert {"lo", "hi", "out-1", "out+1"} <= classes and (W < 2 or "in" in R.names(c["x_classes"]))


# ---- exact assertions ----
@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("align_corners", [False, True])
def test_zeros_padding_fully_outside_is_exactly_zero(gsg, align_corners, dtype_name):
    """Every point has all four taps out of bounds (by 1, by 3, at +-1e4, at +-1e30): the flags zero every coefficient,
    the clamped tap indices still address valid texels, and everything written is 0."""
    dtype = R.DTYPES[dtype_name]
    c = R.case(EDGE_SHAPE, "zeros", align_corners, dtype_name, either=R.OUTSIDE)
    assert set(R.OUTSIDE) <= R.names(c["x_classes"]) | R.names(c["y_classes"])
    assert bool((R.among(c["x_classes"], R.OUTSIDE) | R.among(c["y_classes"], R.OUTSIDE)).all())
    assert all(float(w.abs().max()) == 0 for w in c["want"])
    for g, name in zip(gsg.grad2_2d(*_gpu(c, dtype), 0, align_corners), NAMES):
        assert bool((g == 0).all()), name


@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("align_corners", [False, True])
def test_border_padding_clipped_on_both_axes(gsg, align_corners, dtype_name):
    """Every point clipped on both axes: the clip gradient is 0, so the point's grad_grid row is exactly 0 and it adds
    nothing to grad_input; its weights are exactly 1 and 0, so in float32 / float64 grad_grad_output is the
    grad2_grad_input texel at the clamped corner, bit for bit."""
    dtype = R.DTYPES[dtype_name]
    N, C, H, W, Ho, Wo = EDGE_SHAPE
    c = R.case(EDGE_SHAPE, "border", align_corners, dtype_name, x_classes=R.OUTSIDE, y_classes=R.OUTSIDE)
    g2i, g2g, go, inp, grid = _gpu(c, dtype)
    ggo, gi, gg = gsg.grad2_2d(g2i, g2g, go, inp, grid, 1, align_corners)
    assert bool((gg == 0).all()) and bool((gi == 0).all())
    if dtype != torch.float16:
        ix = torch.where(grid[..., 0] < 0, 0, W - 1).reshape(N, -1)  # (N, M) clamped corner
        iy = torch.where(grid[..., 1] < 0, 0, H - 1).reshape(N, -1)
        idx = (iy * W + ix)[:, None, :].expand(-1, C, -1)
        want = torch.gather(g2i.reshape(N, C, H * W), 2, idx).reshape(N, C, Ho, Wo)
        assert torch.equal(ggo, want)
        assert torch.equal(ggo.cpu().double(), c["want"][0])  # and that is what the reference says, too


@pytest.mark.parametrize("dtype_name", list(R.DTYPES))
@pytest.mark.parametrize("padding_mode,align_corners", [("zeros", False), ("zeros", True)])
def test_outside_batch_next_to_an_ordinary_batch(gsg, padding_mode, align_corners, dtype_name):
    """Batch 1's points all lie fully outside, batch 0's are ordinary: batch 1's grad_input planes stay exactly 0 (a
    point row that indexed the wrong batch would land there), and everything still meets the reference."""
    dtype = R.DTYPES[dtype_name]
    N, C, H, W, Ho, Wo = EDGE_SHAPE
    c0 = R.case(EDGE_SHAPE, padding_mode, align_corners, dtype_name)
    c1 = R.case(EDGE_SHAPE, padding_mode, align_corners, dtype_name, either=R.OUTSIDE)
    grid = torch.cat([c0["grid"][:1], c1["grid"][1:]])
    ops = c0["ops"]
    want = R.reference(*ops, grid, padding_mode, align_corners)
    e32 = None if dtype == torch.float64 else R.error32(ops, grid, padding_mode, align_corners, want)
    k, s_abs = R.contributions(ops[1], ops[2], grid, (N, C, H, W), padding_mode, align_corners)
    got = gsg.grad2_2d(*[t.to(dtype).cuda() for t in (*ops, grid)], PAD[padding_mode], align_corners)
    assert bool((got[1][1] == 0).all()) and bool((got[0][1] == 0).all()) and bool((got[2][1] == 0).all())
    assert float(got[1][0].abs().max()) > 0
    _check(f"outside-batch {padding_mode} align={int(align_corners)} {dtype_name}", got, want, e32,
           _bars(want, e32, k, s_abs, dtype))


# ---- the grid-stride loop (more than 4096 blocks of 256 points), which is also the float32 contention case ----
@pytest.mark.parametrize("padding_mode,align_corners", R.STRIDE_MODES)
def test_grid_stride_loop_and_float32_contention(gsg, padding_mode, align_corners):
    """M = 4096 * 256 + 257 points on a 2 x 3 image.  grad_grad_output and grad_grid: the float32 bar over all points.
    grad_input: each texel collects well over 100,000 float32 atomic adds in an order nobody controls; (k + 8) 2^-24
    S_abs per element is the worst-case bound of k float32 additions in any order (plus the products' own roundings).
    At this k that is wider than grad_input itself: the float64 run below is what sees a single point."""
    c = R.case(R.STRIDE_SHAPE, padding_mode, align_corners, "float32")
    assert float(c["k"].min()) > 100000
    got = gsg.grad2_2d(*_gpu(c, torch.float32), PAD[padding_mode], align_corners)
    b32 = [R.bar32(e, w) for e, w in zip(c["e32"], c["want"])]
    bars = [b32[0], (c["k"] + 8) * 2.0 ** -24 * c["s_abs"], b32[2]]
    _check(f"grid-stride {padding_mode} align={int(align_corners)} float32", got, c["want"], c["e32"], bars)


@pytest.mark.parametrize("padding_mode,align_corners", R.STRIDE_MODES)
def test_grid_stride_loop_float64(gsg, padding_mode, align_corners):
    """The same points in float64, all three outputs at the float64 bar.  The worst-case float32 bar above is wider
    than grad_input itself at this k; 1e-12 max|want| is some 1e9 times below one point's contribution (~0.3), so a
    point that the loop visits twice or not at all shows here.  (Rounding: ~2^-53 sqrt(k) |partial sum| ~ 5e-11 for
    sums of this size in a random order, a few percent of the bar.)"""
    c = R.case(R.STRIDE_SHAPE, padding_mode, align_corners, "float64")
    got = gsg.grad2_2d(*_gpu(c, torch.float64), PAD[padding_mode], align_corners)
    _check(f"grid-stride {padding_mode} align={int(align_corners)} float64", got, c["want"], None,
           _bars(c["want"], None, c["k"], c["s_abs"], torch.float64))


@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_half_contention_in_one_cell(gsg, padding_mode, align_corners):
    """4096 points in one cell: 4096 packed-half atomic adds on each of its four texels, per channel."""
    c, got = _case_check(gsg, R.CONTENTION_SHAPE, padding_mode, align_corners, "float16")
    assert sorted(c["k"][0, 0].reshape(-1).tolist())[-4:] == [4096.0] * 4 and float(c["k"].sum()) == 2 * 4 * 4096


# ---- the odd-address branch of the packed-half atomic, at the ends of the tensor ----
@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_half_grad_input_at_an_odd_element_offset(gsg, padding_mode, align_corners):
    """grad_input as a view one half past a 4-byte boundary, between two guard elements: the first element is then the
    HIGH half of its aligned pair (whose low half is a guard) and the last one the LOW half of its pair.  The result
    meets the same bar as at an even offset, equals it within the bar, and both guards keep their value."""
    import triplaneturbo_amd as tt
    from triplaneturbo_amd import ops as tops
    N, C, H, W, Ho, Wo = EDGE_SHAPE
    c = R.case(EDGE_SHAPE, padding_mode, align_corners, "float16")
    g2i, g2g, go, inp, grid = _gpu(c, torch.float16)
    even = gsg.grad2_2d(g2i, g2g, go, inp, grid, PAD[padding_mode], align_corners)
    buf = torch.zeros(1 + N * C * H * W + 1, dtype=torch.float16, device="cuda")
    buf[0] = buf[-1] = 0.5
    gi = buf[1:-1]
    assert gi.data_ptr() % 4 == 2 and even[1].data_ptr() % 4 == 0
    ggo, gg = torch.empty_like(go), torch.empty_like(grid)
    lib = tt._lib.load()
    p = tops._ptr
    tt._lib.check(lib.tt_grid_sample_2d_grad2_typed(
        tt._lib.TT_DTYPE_F16, p(g2i), p(g2g), p(go), p(inp), p(grid), N, C, H, W, Ho * Wo, PAD[padding_mode],
        int(align_corners), p(ggo), p(gi), p(gg), tops._stream()), "grad2 at an odd offset")
    torch.cuda.synchronize()
    assert float(buf[0]) == 0.5 and float(buf[-1]) == 0.5
    bars = _bars(c["want"], c["e32"], c["k"], c["s_abs"], torch.float16)
    got = (ggo, gi.reshape(N, C, H, W), gg)
    _check(f"odd-offset {padding_mode} align={int(align_corners)} float16", got, c["want"], c["e32"], bars)
    assert torch.equal(ggo, even[0]) and torch.equal(gg, even[2])
    assert bool(((got[1].cpu().double() - even[1].cpu().double()).abs() <= bars[1]).all())


# ---- non-finite grid coordinates ----
@pytest.mark.parametrize("dtype_name", ["float32", "float16"])
@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_non_finite_coordinates_are_inert(gsg, padding_mode, align_corners, dtype_name):
    """Three points get (nan, 0.3), (0.2, -inf), (inf, 0.6).  Their grad_grad_output and grad_grid rows are exactly 0
    (the contract raster.texture has for non-finite UVs), and every other row and ALL of grad_input equal the reference
    in which those three points contribute nothing (their grad_output and grad2_grad_grid rows set to 0; points do not
    interact otherwise)."""
    dtype = R.DTYPES[dtype_name]
    N, C, H, W, Ho, Wo = EDGE_SHAPE
    c = R.case(EDGE_SHAPE, padding_mode, align_corners, dtype_name)
    where = [(0, 0, 0), (0, 0, 17), (1, 0, 3)]  # (n, ho, wo); the first one is an inside point
    values = [(float("nan"), 0.3), (0.2, float("-inf")), (float("inf"), 0.6)]
    g2i, g2g, go, inp = c["ops"]
    g2g_ref, go_ref, grid_bad = g2g.clone(), go.clone(), c["grid"].clone()
    dead = torch.zeros(N, Ho, Wo, dtype=torch.bool)
    for (n, ho, wo), v in zip(where, values):
        g2g_ref[n, ho, wo] = 0
        go_ref[n, :, ho, wo] = 0
        grid_bad[n, ho, wo] = torch.tensor(v, dtype=torch.float64)
        dead[n, ho, wo] = True
    ops_ref = (g2i, g2g_ref, go_ref, inp)
    want = R.reference(*ops_ref, c["grid"], padding_mode, align_corners)
    e32 = R.error32(ops_ref, c["grid"], padding_mode, align_corners, want)
    k, s_abs = R.contributions(g2g_ref, go_ref, c["grid"], (N, C, H, W), padding_mode, align_corners)
    got = gsg.grad2_2d(*[t.to(dtype).cuda() for t in (g2i, g2g, go, inp, grid_bad)], PAD[padding_mode], align_corners)
    ggo, gi, gg = (g.cpu() for g in got)
    assert bool((ggo[dead[:, None].expand_as(ggo)] == 0).all()) and bool((gg[dead] == 0).all())
    assert bool(torch.isfinite(gi).all())
    _check(f"non-finite {padding_mode} align={int(align_corners)} {dtype_name}", got, want, e32,
           _bars(want, e32, k, s_abs, dtype), rows=~dead)


# ---- the autograd wrapper ----
@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_gradgradcheck(gsg, padding_mode, align_corners):
    """torch's own numerical second-order check of grid_sample_2d in float64 on constructed points: the leg on the GPU
    that does not go through the oracle.  (nondet_tol: grad_input is summed with atomics.)"""
    N, C, H, W, Ho, Wo = R.GRADGRAD_SHAPE
    c = R.case(R.GRADGRAD_SHAPE, padding_mode, align_corners, "float64")
    inp = c["ops"][3].cuda().requires_grad_(True)
    grid = c["grid"].cuda().requires_grad_(True)
    assert torch.autograd.gradgradcheck(lambda a, b: gsg.grid_sample_2d(a, b, padding_mode, align_corners), (inp, grid),
                                        eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=1e-12)


def _second_order(f, inp, grid, w, r, variant):
    """The second-order graph of test_gpu_grad2.py (a gradient of the sample as part of the loss) with only some of
    the operands requiring grad.  variant "input": input (and the weights w, so that grad_grad_output is not trivially
    absent) -- grad2_grad_grid arrives as None; "grid": the grid alone -- grad2_grad_input arrives as None;
    "noncontig": both, the grid a permuted view of a (N,2,Ho,Wo) leaf."""
    grad = torch.autograd.grad
    if variant == "input":
        inp, w = inp.clone().requires_grad_(True), w.clone().requires_grad_(True)
        out = f(inp, grid)
        (g1,) = grad((out * w).sum(), inp, create_graph=True)
        loss = (g1.double() * r).sum() + (out.double() ** 2).sum()
        return grad(loss, (inp, w))
    if variant == "grid":
        grid = grid.clone().requires_grad_(True)
        out = f(inp, grid)
        (g1,) = grad((out * w).sum(), grid, create_graph=True)
        loss = (g1.double() ** 2).sum() + out.double().sum()
        return grad(loss, (grid,))
    inp = inp.clone().requires_grad_(True)
    base = grid.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    view = base.permute(0, 2, 3, 1)
    assert not view.is_contiguous()
    out = f(inp, view)
    (g1,) = grad((out * w).sum(), view, create_graph=True)
    loss = (g1.double() ** 2).sum() + out.double().sum()
    return grad(loss, (inp, base))


@pytest.mark.parametrize("variant", ["input", "grid", "noncontig"])
@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_wrapper_partial_requires_grad_and_views(gsg, padding_mode, align_corners, variant):
    c = R.case(R.WRAPPER_SHAPE, padding_mode, align_corners, "float32")
    r, _, w, inp = c["ops"]
    grid = c["grid"]

    def oracle(a, b):
        return R.sample(a, b, padding_mode, align_corners)

    want = [g.detach() for g in _second_order(oracle, inp, grid, w, r, variant)]
    w32 = _second_order(oracle, inp.float(), grid.float(), w.float(), r, variant)
    got = _second_order(lambda a, b: gsg.grid_sample_2d(a, b, padding_mode, align_corners), inp.float().cuda(),
                        grid.float().cuda(), w.float().cuda(), r.cuda(), variant)
    for i, (g, w64, g32) in enumerate(zip(got, want, w32)):
        assert g.dtype == torch.float32 and g.shape == w64.shape
        e_hip = float((g.cpu().double() - w64).abs().max())
        e_ref32 = float((g32.double() - w64).abs().max())
        print(f"grad2 wrapper {variant} {padding_mode} align={int(align_corners)} out{i}: e_hip={e_hip:.3e} "
              f"e_ref32={e_ref32:.3e} max|want|={float(w64.abs().max()):.3e}")
        assert float(w64.abs().max()) > 0
        assert e_hip <= R.bar32(e_ref32, w64), (variant, i, e_hip, e_ref32)


# ---- argument errors: before any launch ----
def test_argument_errors(gsg):
    N, C, H, W, Ho, Wo = 2, 3, 3, 5, 2, 4
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device="cuda")  # noqa: E731
    g2i, g2g, go, inp, grid = z(N, C, H, W), z(N, Ho, Wo, 2), z(N, C, Ho, Wo), z(N, C, H, W), z(N, Ho, Wo, 2)
    gsg.grad2_2d(g2i, g2g, go, inp, grid, 0, False)
    with pytest.raises(ValueError, match="grid"):  # grid.shape[0] != N
        gsg.grad2_2d(g2i, z(N + 1, Ho, Wo, 2), go, inp, z(N + 1, Ho, Wo, 2), 0, False)
    with pytest.raises(ValueError, match="grid"):  # grid.shape[-1] != 2
        gsg.grad2_2d(g2i, z(N, Ho, Wo, 3), go, inp, z(N, Ho, Wo, 3), 0, False)
    for bad in ((N, C, Ho, Wo + 1), (N, C + 1, Ho, Wo), (N, C, Ho * Wo), (N, C, Wo, Ho)):
        with pytest.raises(ValueError, match="grad_output"):
            gsg.grad2_2d(g2i, g2g, z(*bad), inp, grid, 0, False)
    with pytest.raises(ValueError, match="input"):  # a 3-D input
        gsg.grad2_2d(z(C, H, W), g2g, go, z(C, H, W), grid, 0, False)
    with pytest.raises(ValueError, match="grad2_grad_input"):
        gsg.grad2_2d(z(N, C, H, W + 1), g2g, go, inp, grid, 0, False)
    with pytest.raises(ValueError, match="grad2_grad_grid"):
        gsg.grad2_2d(g2i, z(N, Ho, Wo + 1, 2), go, inp, grid, 0, False)
    with pytest.raises(TypeError):  # mixed dtypes stay a TypeError
        gsg.grad2_2d(g2i, g2g, go.double(), inp, grid, 0, False)
    with pytest.raises(TypeError):
        gsg.grad2_2d(g2i, g2g, go, inp, grid.half(), 0, False)
