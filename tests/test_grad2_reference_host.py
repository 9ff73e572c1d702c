"""The CPU reference of the grid-sample double backward (tests/grad2_reference.py) checked without a GPU: it replays
the known-answer file, agrees with central finite differences of the first backward (the leg that does not go through
autograd's double backward), and its constructed grids keep their distance from the tap boundaries in every dtype."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad2_reference as R  # noqa: E402


def test_reference_replays_known_answers(golden_dir):
    k = {n: torch.from_numpy(v) for n, v in np.load(os.path.join(golden_dir, "grad2_kat.npz")).items()}
    got = R.reference(k["g2i"], k["g2g"], k["go"], k["inp"], k["grid"], "zeros", False, torch.float64)
    for g, name in zip(got, ("ggo", "gi", "gg")):
        err = float((g - k[name]).abs().max())
        assert err <= 1e-12 * float(k[name].abs().max()), (name, err)


def test_border_clip_gradient_is_zero_at_the_bounds():
    """ATen's clip_coordinates_set_grad uses <= and >=: at ip = 0 and ip = size-1 exactly the first backward's
    grad_grid is 0 under border padding (torch.grid_sample itself agrees)."""
    inp = torch.randn(1, 2, 3, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    grid = torch.tensor([[[[-1.0, -1.0], [1.0, 1.0], [-1.0, 0.3], [0.2, 1.0]]]], dtype=torch.float64)
    go = torch.ones(1, 2, 1, 4, dtype=torch.float64)
    _, gg = R.first_backward(go, inp, grid, "border", True)
    g = grid.clone().requires_grad_(True)
    torch.nn.functional.grid_sample(inp, g, mode="bilinear", padding_mode="border", align_corners=True).sum().backward()
    assert torch.equal(gg[0, 0, :2], torch.zeros(2, 2, dtype=torch.float64))
    assert gg[0, 0, 2, 0] == 0 and gg[0, 0, 3, 1] == 0 and gg[0, 0, 2, 1] != 0 and gg[0, 0, 3, 0] != 0
    torch.testing.assert_close(gg, g.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("padding_mode,align_corners", R.MODES)
def test_reference_matches_finite_differences(padding_mode, align_corners):
    """L = <gi1, g2i> + <gg1, g2g> with (gi1, gg1) the first backward; the reference's three outputs are dL/d(go, inp,
    grid), here by central differences element by element.  L is linear in go and inp and bilinear in a point's two
    coordinates between tap boundaries, so the O(h^2) term vanishes and rounding (~1e-16 |L| / h) is what is left.
    Constructed points of every class but the exact-border ones, which sit on the clip's kink by construction."""
    N, C, H, W, Ho, Wo = 1, 2, 3, 4, 3, 4
    no_kink = R.INSIDE + R.STRADDLE + R.OUTSIDE
    grid, xc, yc = R.build_grid(N, H, W, Ho, Wo, padding_mode, align_corners, torch.float64, seed=7,
                                x_classes=no_kink, y_classes=no_kink)
    assert R.names(xc) == set(no_kink) and R.names(yc) == set(no_kink)
    g2i, g2g, go, inp = R.operands((N, C, H, W, Ho, Wo), grid, torch.float64, seed=7)
    want = R.reference(g2i, g2g, go, inp, grid, padding_mode, align_corners, torch.float64)

    def L(go_, inp_, grid_):
        gi1, gg1 = R.first_backward(go_, inp_, grid_, padding_mode, align_corners)
        return float((gi1 * g2i).sum() + (gg1 * g2g).sum())

    h = 1e-5
    args = [go, inp, grid]
    for which, w in enumerate(want):
        fd = torch.zeros_like(w).reshape(-1)
        for e in range(fd.numel()):
            lo = [a.clone() for a in args]
            hi = [a.clone() for a in args]
            lo[which].reshape(-1)[e] -= h
            hi[which].reshape(-1)[e] += h
            fd[e] = (L(*hi) - L(*lo)) / (2 * h)
        err = float((fd.reshape(w.shape) - w).abs().max())
        assert float(w.abs().max()) > 0
        assert err <= 1e-7 * float(w.abs().max()), (which, err)


def _grids():
    for shape in R.SHAPES + [R.STRIDE_SHAPE, R.CONTENTION_SHAPE, R.WRAPPER_SHAPE, R.GRADGRAD_SHAPE]:
        for padding_mode, align_corners in R.MODES:
            for name in R.DTYPES:
                unused = name == "float16" or (padding_mode, align_corners) not in R.STRIDE_MODES
                if shape == R.STRIDE_SHAPE and unused:  # (that case runs in float32 and float64, in two modes)
                    continue
                yield shape, padding_mode, align_corners, name


@pytest.mark.parametrize("shape,padding_mode,align_corners,dtype_name", list(_grids()))
def test_constructed_grids_keep_their_distance(shape, padding_mode, align_corners, dtype_name):
    """After rounding to the dtype every coordinate near the image is still margin(dtype) from an integer pixel
    coordinate, the far classes are still far, and every value is finite."""
    dtype = R.DTYPES[dtype_name]
    N, C, H, W, Ho, Wo = shape
    grid, xc, yc = R.build_grid(N, H, W, Ho, Wo, padding_mode, align_corners, dtype, **R.grid_args(shape))
    assert torch.equal(grid.to(dtype).double(), grid) and bool(torch.isfinite(grid).all())
    exact = torch.stack([R.among(xc, R.EXACT), R.among(yc, R.EXACT)], -1).reshape(grid.shape)
    far = torch.stack([R.among(xc, R.FAR_OUT), R.among(yc, R.FAR_OUT)], -1).reshape(grid.shape)
    assert bool((grid[far].abs() >= 9000).all())
    for axis, size in ((0, W), (1, H)):
        ip = R.unnormalize(grid[..., axis], size, align_corners)
        assert bool(((ip[exact[..., axis]] == 0) | (ip[exact[..., axis]] == size - 1)).all())
    kept = torch.where(exact, torch.full_like(grid, 1e4), grid)  # (an exact-border point sits ON a tap, on purpose)
    assert R.near_distance(kept, H, W, align_corners) >= R.margin(dtype)
