"""HIP texture sampling (tt_tex_fwd / tt_tex_bwd, raster.texture) against the float64 restatement of the contract
(tests/texture_reference.py) on the smallest shapes that can go wrong: odd sizes with one texture shared by three
images, a batched texture, a single texel, C = 1 .. 4 (every vector width), both filters x three boundary modes.

Inputs are constructed, not filtered.  `uv_rand` holds random UVs in [-1.5, 2.5] (half of them in [0, 1]) built as
(k + o) / (2 n) with an integer k and o in [0.004, 0.996], so that every coordinate is at least 2e-3 texel from a
texel edge (where nearest is discontinuous) and from a texel centre (where grad_uv is), plus one NaN, one +inf and one
-inf pixel.  `uv_exact` holds texel centres, texel edges and u, v in {0, 1} (exactly representable for the
power-of-two sizes) and is compared where the function is continuous there: the linear forward and grad_tex.

Tolerances: with |uv| <= 2.5 and sizes <= 8, u TW - 0.5 carries at most about 1.2e-6 of fp32 rounding and so do the
weights: forward within 1e-5 max|tex|, grad_tex within 1e-5 max|grad_tex_ref|, grad_uv within 1e-5 TW max|tex|
max|grad_out|."""
import functools
import os
import sys

import pytest
import torch

from triplaneturbo_amd import raster

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_reference as TR  # noqa: E402

pytestmark = pytest.mark.gpu
H, W = 6, 5
CASES = {"5x7x3_shared": ((1, 5, 7, 3), 3), "4x4x1_batched": ((2, 4, 4, 1), 2), "1x1x2_texel": ((1, 1, 1, 2), 2),
         "8x8x4": ((1, 8, 8, 4), 1)}
FILTERS = ["nearest", "linear"]
BOUNDARIES = ["wrap", "clamp", "zero"]
NONFINITE = [((0, 0, 0), (float("nan"), 0.3)), ((-1, 1, 1), (0.2, float("-inf"))), ((0, 2, 3), (float("inf"), 0.6))]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _rand_axis(g, shape, n):
    k = torch.randint(-3 * n, 5 * n, shape, generator=g)
    inside = torch.rand(shape, generator=g) < 0.5  # half of the coordinates in [0, 1]: in range for "zero", too
    k = torch.where(inside, torch.randint(0, 2 * n, shape, generator=g), k).double()
    o = 0.004 + 0.992 * torch.rand(shape, generator=g, dtype=torch.float64)
    return (k + o) / (2 * n)


def _exact_axis(n):
    centres = [(i + 0.5) / n for i in range(-n, 2 * n)]
    edges = [i / n for i in range(-n, 2 * n + 1)]
    return torch.tensor([0.0, 1.0] + centres + edges, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    (N, TH, TW, C), B = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    tex = torch.randn(N, TH, TW, C, generator=g)
    uv_rand = torch.stack([_rand_axis(g, (B, H, W), TW), _rand_axis(g, (B, H, W), TH)], -1).float()
    for (b, y, x), val in NONFINITE:
        uv_rand[b, y, x] = torch.tensor(val)
    eu, ev = _exact_axis(TW), _exact_axis(TH)
    k = torch.arange(B * H * W)
    uv_exact = torch.stack([eu[k % len(eu)], ev[(7 * k + k // len(eu)) % len(ev)]], -1)
    uv_exact[:4] = torch.tensor([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=torch.float64)
    uv_exact = uv_exact.reshape(B, H, W, 2).float()
    g_out = torch.randn(B, H, W, C, generator=g)
    return tex, uv_rand, uv_exact, g_out


@functools.lru_cache(maxsize=None)
def _reference(name, which, filt, bnd):
    """(out, grad_tex, grad_uv) of the restatement in float64, computed once per combination"""
    tex, uv_rand, uv_exact, g_out = _inputs(name)
    t = tex.double().requires_grad_(True)
    u = (uv_rand if which == "rand" else uv_exact).double().requires_grad_(True)
    out = TR.texture(t, u, filt, bnd)
    out.backward(g_out.double())
    return out.detach(), t.grad, u.grad


def _hip(dev, tex, uv, g_out, filt, bnd):
    t = tex.to(dev).requires_grad_(True)
    u = uv.to(dev).requires_grad_(True)
    out = raster.texture(t, u, filter_mode=filt, boundary_mode=bnd)
    out.backward(g_out.to(dev))
    return out.detach().cpu().double(), t.grad.cpu().double(), u.grad.cpu().double()


@pytest.mark.parametrize("bnd", BOUNDARIES)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(dev, name, filt, bnd):
    tex, uv_rand, uv_exact, g_out = _inputs(name)
    TW = tex.shape[2]
    tmax, gmax = tex.abs().max().item(), g_out.abs().max().item()
    out, g_tex, g_uv = _hip(dev, tex, uv_rand, g_out, filt, bnd)
    r_out, r_tex, r_uv = _reference(name, "rand", filt, bnd)
    e_out = (out - r_out).abs().max().item()
    e_tex = (g_tex - r_tex).abs().max().item()
    e_uv = (g_uv - r_uv).abs().max().item()
    print(f"{name} {filt} {bnd} rand: out {e_out:.2e} / {1e-5 * tmax:.2e}  grad_tex {e_tex:.2e} / "
          f"{1e-5 * r_tex.abs().max().item():.2e}  grad_uv {e_uv:.2e} / {1e-5 * TW * tmax * gmax:.2e}")
    assert e_out <= 1e-5 * tmax
    assert e_tex <= 1e-5 * r_tex.abs().max().item()
    assert e_uv <= 1e-5 * TW * tmax * gmax
    if filt == "nearest":
        assert torch.count_nonzero(g_uv) == 0
    for (b, y, x), _ in NONFINITE:  # exactly zero, not just close
        assert torch.count_nonzero(out[b, y, x]) == 0 and torch.count_nonzero(g_uv[b, y, x]) == 0
    if filt == "linear":  # texel centres, texel edges, u, v in {0, 1}: continuous for the forward and grad_tex
        out, g_tex, _ = _hip(dev, tex, uv_exact, g_out, filt, bnd)
        r_out, r_tex, _ = _reference(name, "exact", filt, bnd)
        e_out = (out - r_out).abs().max().item()
        e_tex = (g_tex - r_tex).abs().max().item()
        print(f"{name} {filt} {bnd} exact: out {e_out:.2e}  grad_tex {e_tex:.2e} / {1e-5 * r_tex.abs().max().item():.2e}")
        assert e_out <= 1e-5 * tmax
        assert e_tex <= 1e-5 * r_tex.abs().max().item()


@pytest.mark.parametrize("filt", FILTERS)
def test_only_one_input_requires_grad(dev, filt):
    """the grad_tex = NULL and grad_uv = NULL paths of tt_tex_bwd give what the full backward gives"""
    tex, uv_rand, _, g_out = _inputs("5x7x3_shared")
    _, r_tex, r_uv = _reference("5x7x3_shared", "rand", filt, "wrap")
    t = tex.to(dev).requires_grad_(True)
    raster.texture(t, uv_rand.to(dev), filter_mode=filt).backward(g_out.to(dev))
    assert (t.grad.cpu().double() - r_tex).abs().max() <= 1e-5 * r_tex.abs().max()
    u = uv_rand.to(dev).requires_grad_(True)
    raster.texture(tex.to(dev), u, filter_mode=filt).backward(g_out.to(dev))
    assert (u.grad.cpu().double() - r_uv).abs().max() <= 1e-5 * 7 * tex.abs().max() * g_out.abs().max()


def test_no_pixels_gives_an_empty_tensor(dev):
    tex = torch.randn(1, 5, 7, 3, device=dev, requires_grad=True)
    for shape in ((0, 6, 5, 2), (2, 0, 5, 2), (2, 6, 0, 2)):
        out = raster.texture(tex, torch.zeros(shape, device=dev))
        assert out.shape == shape[:3] + (3,) and out.numel() == 0
    out.sum().backward()  # the backward entry still writes every element of grad_tex
    assert torch.count_nonzero(tex.grad) == 0


def test_forward_and_grad_uv_are_bit_identical_across_launches(dev):
    tex, uv_rand, _, g_out = _inputs("8x8x4")
    a = _hip(dev, tex, uv_rand, g_out, "linear", "wrap")
    b = _hip(dev, tex, uv_rand, g_out, "linear", "wrap")
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


@pytest.mark.parametrize("bnd", ["clamp", "wrap"])
@pytest.mark.parametrize("name", list(CASES))
def test_linear_weights_sum_to_one(dev, name, bnd):
    """grad_out = 1 at finite uv: every pixel hands out weights that sum to 1 per channel, so grad_tex sums to
    B H W C (each texel receives a handful of terms: 1e-5 relative is far above fp32 summation error)"""
    tex, _, uv_exact, g_out = _inputs(name)
    _, g_tex, _ = _hip(dev, tex, uv_exact, torch.ones_like(g_out), "linear", bnd)
    assert abs(g_tex.sum().item() - g_out.numel()) <= 1e-5 * g_out.numel()
