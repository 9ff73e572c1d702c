"""The geometry backward takes dW2 and dw3 of the sdf net from ONE accumulator (csrc/tt_backward.hip, "row-scaling
identity"):  D = sum_samples m2 v^T,  dW2_ij = w3_i D_ij,  dw3_i = sum_j W2_ij D_ij.  These tests pin what that form
could get wrong: output weights that are exactly zero or tiny (no division anywhere: the row of dW2 is exactly 0, dw3_i
is not), ragged tiles, the kernel-end flush across waves and workgroups (waves that popped nothing included), and the
per-point entry tt_points_bwd_geo, which runs the same kernel.  No case masks out rays."""
import os

import pytest
import torch

from oracle import cpu_ref as O

from parity import PRECISIONS, check_grads, rel  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = (("comp_rgb", 3), ("opacity", 1), ("depth", 1), ("z_variance", 1), ("disparity", 1), ("comp_normal", 3),
        ("comp_normal_cam_vis", 3))
ZERO_ROWS = list(range(0, 64, 4))   # 16 output weights exactly 0
TINY_ROWS = list(range(1, 64, 8))   # 8 output weights +-1e-30
GEO_NAMES = ["space_cache", "sdf.w1", "sdf.w2", "sdf.w3"]


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from triplaneturbo_amd import functional, ops
    return ops, functional


def _w3_with_zeros(w3):
    w3 = w3.clone()
    w3[0, ZERO_ROWS] = 0.0
    w3[0, TINY_ROWS] = torch.tensor([1e-30, -1e-30] * (len(TINY_ROWS) // 2))
    return w3


def _scene(P, R, n_view, Hh, Ww, S, seed):
    g = torch.Generator().manual_seed(seed)
    cache = torch.randn(P, 6, 32, R, R, generator=g) * 0.5
    sw = O.init_mlp_weights([32, 64, 64, 1], g)
    sw = [sw[0], sw[1], _w3_with_zeros(sw[2])]
    fw = O.init_mlp_weights([96, 64, 64, 3], g)
    ro, rd, c2w, cd = O.make_cameras(P * n_view, Hh, Ww)
    ts, te = O.uniform_intervals(P * n_view * Hh * Ww, S, 0.3, 3.2)
    proj = {n: torch.randn(P * n_view, Hh, Ww, c, generator=g) for n, c in KEYS}
    return cache, sw, fw, ro, rd, ts, te, torch.ones(3), cd, c2w, proj


RCK = dict(inv_std=100.0, rgb_grad_shrink=0.7, cos_anneal_ratio=1.0)
_ORACLE = {}


def _oracle(key):
    """fp32 and fp64 oracle gradients (planes + sdf net) of the scene `key`, evaluated once per module."""
    if key not in _ORACLE:
        cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = _scene(*key)

        def run(d):
            c = cache.to(d).requires_grad_(True)
            sws = [w.to(d).requires_grad_(True) for w in sw]
            out = O.render(c, sws, [w.to(d) for w in fw], ro.to(d), rd.to(d), ts.to(d), te.to(d), bg.to(d), cd.to(d),
                           c2w.to(d), **RCK)
            return list(torch.autograd.grad(O.synthetic_loss(out, {k: v.to(d) for k, v in proj.items()}), [c] + sws))
        _ORACLE[key] = (run(torch.float32), run(torch.float64))
    return _ORACLE[key]


def _hip(mods, key, **rc_kwargs):
    ops, functional = mods
    cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = _scene(*key)
    dev = "cuda"
    c = cache.to(dev).requires_grad_(True)
    sws = [w.to(dev).requires_grad_(True) for w in sw]
    out = functional.volume_render(c, sws, [w.to(dev) for w in fw], ro.to(dev), rd.to(dev), ts.to(dev), te.to(dev),
                                   bg.to(dev), cd.to(dev), c2w.to(dev), ops.RenderConfig(**RCK, **rc_kwargs), training=True)
    loss = O.synthetic_loss(out, {k: v.to(dev) for k, v in proj.items()})
    return [t.cpu() for t in torch.autograd.grad(loss, [c] + sws)]


def _check_zero_rows(dw2, dw3, dw3_32, dw3_64):
    """Rows with w3_i = 0: dW2's row is exactly 0 (w3_i x D), dw3_i is not and meets the bars of tests/parity.py on the
    sub-vector (1e-4 against the fp32 oracle; as close to fp64 as the fp32 oracle is, x3, or 1e-4)."""
    assert dw2[ZERO_ROWS].abs().max().item() == 0.0
    a, b32, b64 = dw3.reshape(-1)[ZERO_ROWS], dw3_32.reshape(-1)[ZERO_ROWS], dw3_64.reshape(-1)[ZERO_ROWS]
    e32, e64, e3264 = rel(a, b32), rel(a, b64), rel(b32, b64)
    print(f"dw3 on the {len(ZERO_ROWS)} rows with w3 = 0: hip_vs_fp32 {e32:.3g} hip_vs_fp64 {e64:.3g} fp32_vs_fp64 {e3264:.3g}")
    assert (a != 0).all() and (b64 != 0).all()
    assert e32 <= 1e-4, e32
    assert e64 <= max(1e-4, 3 * e3264), (e64, e3264)


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "test_gpu_geo_w3").split("::")[-1].split(" ")[0]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_and_tiny_output_weights(mods, precision):
    key = (1, 32, 1, 8, 8, 32, 71)
    g = _hip(mods, key, precision=precision)
    g32, g64 = _oracle(key)
    rows = check_grads(_case(), g, g32, g64, names=GEO_NAMES)
    print({n: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for n, r in rows.items()})
    _check_zero_rows(g[2], g[3], g32[3], g64[3])


@pytest.mark.parametrize("sb", [1, 2, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_tiles(mods, sb, precision):
    """2 prompts x 2 views of 5 x 7 rays x 45 samples: invalid lanes in a tile, tiles that straddle prompts."""
    key = (2, 32, 2, 5, 7, 45, 72)
    g = _hip(mods, key, precision=precision, tile_sb=sb)
    g32, g64 = _oracle(key)
    rows = check_grads(_case(), g[1:], g32[1:], g64[1:], names=GEO_NAMES[1:])
    print({n: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for n, r in rows.items()})
    _check_zero_rows(g[2], g[3], g32[3], g64[3])


@pytest.mark.parametrize("Hh,Ww,S", [(64, 64, 64),  # more work items than the 1 024 wave slots
                                     (8, 8, 32)])   # almost every wave pops nothing and flushes zeros
def test_flush_sums_over_waves_and_workgroups(mods, Hh, Ww, S):
    """sdf.w2 / sdf.w3 of one launch = the sum of two launches over the two halves of the image run under another tiling
    (tile_chunk, tile_sb).  Allowed: 3 x the difference of two runs of the full launch (float-atomic order)."""
    ops, functional = mods
    g = torch.Generator().manual_seed(73)
    R = 64
    cache = (torch.randn(1, 6, 32, R, R, generator=g) * 0.5).cuda()
    sw = [w.cuda() for w in O.init_mlp_weights([32, 64, 64, 1], g)]
    fw = [w.cuda() for w in O.init_mlp_weights([96, 64, 64, 3], g)]
    ro, rd, c2w, cd = O.make_cameras(1, Hh, Ww)
    ro, rd = ro.reshape(-1, 3).cuda(), rd.reshape(-1, 3).cuda()
    n_rays = Hh * Ww
    ts, te = [t.cuda() for t in O.uniform_intervals(n_rays, S, 0.3, 3.2)]
    pr = torch.randn(n_rays, 3, generator=g).cuda()

    def grads(lo, hi, **rc_kwargs):
        sws = [w.clone().requires_grad_(True) for w in sw]
        r = ops.render_samples(cache, sws, fw, ro[lo:hi], rd[lo:hi], ts[lo:hi], te[lo:hi], hi - lo,
                               ops.RenderConfig(**rc_kwargs), image_w=Ww)
        loss = (r["rgb_fg"] * pr[lo:hi]).sum() + r["opacity"].sum() + ((r["sdf_grad"].norm(dim=-1) - 1) ** 2).sum()
        return [t.double() for t in torch.autograd.grad(loss, sws[1:])]

    full, again = grads(0, n_rays), grads(0, n_rays)
    top, bottom = grads(0, n_rays // 2, tile_chunk=7, tile_sb=4), grads(n_rays // 2, n_rays, tile_chunk=7, tile_sb=4)
    for n, a, b, y, z in zip(("sdf.w2", "sdf.w3"), full, again, top, bottom):
        noise, diff = rel(b, a), rel(y + z, a)
        print(f"{n}: run-to-run {noise:.3g}, halves vs full {diff:.3g}")
        assert a.abs().max().item() > 0
        assert diff <= 3 * noise, (n, diff, noise)


_POINTS_ORACLE = {}


@pytest.mark.parametrize("upstream", ["sdf", "sdf_grad", "both"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_points_backward(mods, upstream, precision):
    """tt_points_bwd_geo on 300 points (not a multiple of 32), w3 with zeros, against autograd through the oracle's
    geometry_forward.  Bar as in tests/test_gpu_points_backward.py: as close to fp64 as the fp32 oracle is (x3) or 1e-4."""
    ops, functional = mods
    gen = torch.Generator().manual_seed(74)
    R, N = 32, 300
    cache = torch.randn(1, 6, 32, R, R, generator=gen) * 0.5
    sw = O.init_mlp_weights([32, 64, 64, 1], gen)
    sw = [sw[0], sw[1], _w3_with_zeros(sw[2])]
    fw = O.init_mlp_weights([96, 64, 64, 3], gen)
    pts = torch.rand(1, N, 3, generator=gen) * 2.2 - 1.1  # some outside the box (zeros padding)
    proj = {"sdf": torch.randn(N, 1, generator=gen), "sdf_grad": torch.randn(N, 3, generator=gen)}
    keys = ("sdf", "sdf_grad") if upstream == "both" else (upstream,)

    if upstream not in _POINTS_ORACLE:
        def oracle(dt):
            c = cache.to(dt).requires_grad_(True)
            ws = [w.to(dt).requires_grad_(True) for w in sw]
            o = O.geometry_forward(pts.to(dt), c, ws, [w.to(dt) for w in fw], output_normal=True, create_graph=True)
            return list(torch.autograd.grad(sum((o[k] * proj[k].to(dt)).sum() for k in keys), [c] + ws))
        _POINTS_ORACLE[upstream] = (oracle(torch.float32), oracle(torch.float64))
    g32, g64 = _POINTS_ORACLE[upstream]
    dev = "cuda"
    c = cache.to(dev).requires_grad_(True)
    ws = [w.to(dev).requires_grad_(True) for w in sw]
    sdf, sdf_grad, _ = ops.query_points_grad(c, ws, [w.to(dev) for w in fw], pts.to(dev), precision=precision)
    out = {"sdf": sdf, "sdf_grad": sdf_grad}
    g = [t.cpu() for t in torch.autograd.grad(sum((out[k] * proj[k].to(dev)).sum() for k in keys), [c] + ws)]
    for n, a, b32, b64 in zip(GEO_NAMES, g, g32, g64):
        e_hip, e_cpu = rel(a, b64), rel(b32, b64)
        print(f"{n}: hip_vs_fp64 {e_hip:.3g} fp32_vs_fp64 {e_cpu:.3g} hip_vs_fp32 {rel(a, b32):.3g}")
        assert e_hip <= max(1e-4, 3 * e_cpu), (n, e_hip, e_cpu)
    _check_zero_rows(g[2], g[3], g32[3], g64[3])
