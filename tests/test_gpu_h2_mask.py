"""Geometry backward with the forward's h2 sign mask (tt_render_fwd_h2mask / tt_render_bwd_geo_h2mask) and a1 as the mask
product C^T m2, C = diag(w3) W2 (csrc/tt_backward.hip).  What these forms could get wrong and the existing tests do not
look at: the content and layout of the mask words, the words of skipped tile steps, lanes that read another sample's word,
the image of C with zero / tiny / badly scaled factors, and the per-point entry (mask product only, no forward mask).

Scene: 2 prompts x 1 view of 7 x 5 rays x 13 samples on 16 x 16 planes, intervals 0.3 .. 3.2 (rays enter and leave the
cube: skipped and single-plane tile steps), w3 with 16 exact zeros and 8 entries of +-1e-30.  No case masks out rays."""
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
P, R, HH, WW, S, SEED = 2, 16, 7, 5, 13, 10
RCK = dict(inv_std=100.0, rgb_grad_shrink=0.7, cos_anneal_ratio=1.0)


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from triplaneturbo_amd import functional, ops
    return ops, functional


def _scene(scaled=False, far=3.2):
    g = torch.Generator().manual_seed(SEED)
    cache = torch.randn(P, 6, 32, R, R, generator=g) * 0.5
    sw = O.init_mlp_weights([32, 64, 64, 1], g)
    w3 = sw[2].clone()
    w3[0, ZERO_ROWS] = 0.0
    w3[0, TINY_ROWS] = torch.tensor([1e-30, -1e-30] * (len(TINY_ROWS) // 2))
    sw = [sw[0], sw[1] * 1e-6, w3 * 3e5] if scaled else [sw[0], sw[1], w3]
    fw = O.init_mlp_weights([96, 64, 64, 3], g)
    ro, rd, c2w, cd = O.make_cameras(P, HH, WW)
    ts, te = O.uniform_intervals(P * HH * WW, S, 0.3, far)
    proj = {n: torch.randn(P, HH, WW, c, generator=g) for n, c in KEYS}
    return cache, sw, fw, ro, rd, ts, te, torch.ones(3), cd, c2w, proj


_ORACLE = {}


def _oracle(scaled=False):
    """fp32 and fp64 oracle gradients (planes + sdf net), evaluated once per scene and module."""
    if scaled not in _ORACLE:
        cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = _scene(scaled)

        def run(d):
            c = cache.to(d).requires_grad_(True)
            sws = [w.to(d).requires_grad_(True) for w in sw]
            out = O.render(c, sws, [w.to(d) for w in fw], ro.to(d), rd.to(d), ts.to(d), te.to(d), bg.to(d), cd.to(d),
                           c2w.to(d), **RCK)
            return list(torch.autograd.grad(O.synthetic_loss(out, {k: v.to(d) for k, v in proj.items()}), [c] + sws))
        _ORACLE[scaled] = (run(torch.float32), run(torch.float64))
    return _ORACLE[scaled]


def _hip(mods, scaled=False, **rc_kwargs):
    ops, functional = mods
    cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = _scene(scaled)
    dev = "cuda"
    c = cache.to(dev).requires_grad_(True)
    sws = [w.to(dev).requires_grad_(True) for w in sw]
    out = functional.volume_render(c, sws, [w.to(dev) for w in fw], ro.to(dev), rd.to(dev), ts.to(dev), te.to(dev),
                                   bg.to(dev), cd.to(dev), c2w.to(dev), ops.RenderConfig(**RCK, **rc_kwargs), training=True)
    loss = O.synthetic_loss(out, {k: v.to(dev) for k, v in proj.items()})
    return [t.cpu() for t in torch.autograd.grad(loss, [c] + sws)]


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "test_gpu_h2_mask").split("::")[-1].split(" ")[0]


_MASK_REF = {}


def _mask_reference(far):
    """float64: z = W2 relu(W1 f) per sample (n, 64) with f from the oracle's plane sampling, the per-entry exclusion
    threshold 1e-5 ||W2_i||_1 max |h1|, and the samples that lie clearly outside every plane's bilinear support."""
    if far not in _MASK_REF:
        cache, sw, fw, ro, rd, ts, te = [t.double() if torch.is_tensor(t) else [w.double() for w in t]
                                         for t in _scene(far=far)[:7]]
        n_rays = P * HH * WW
        tm = ((ts + te) / 2.0).reshape(n_rays, S, 1)
        pos = ro.reshape(n_rays, 1, 3) + rd.reshape(n_rays, 1, 3) * tm
        geo = O.geometry_forward(pos.reshape(P, HH * WW * S, 3), cache, sw, fw, output_normal=False)
        f = geo["enc_geo"]  # (n, 32)
        h1 = torch.relu(f @ sw[0].T)
        z = h1 @ sw[1].T
        thr = 1e-5 * sw[1].abs().sum(dim=1)[None, :] * h1.abs().max(dim=1, keepdim=True).values
        # a plane has no in-bounds texel once one of its two coordinates is beyond the bilinear support; every plane is out
        # when two of the three coordinates are (radius 1: plane coordinates = positions)
        outside = pos.reshape(-1, 3).abs().sort(dim=1).values[:, 1] > 1.0 + 2.0 / R
        assert (f[outside] == 0).all()
        _MASK_REF[far] = (z, thr, outside)
    return _MASK_REF[far]


# far = 3.2 is the scene of the other tests; there every sample still has one plane with an in-bounds texel (single-plane
# tile steps, none skipped).  far = 6.4 adds samples outside every plane and tile steps that are skipped altogether.
@pytest.mark.parametrize("far", [3.2, 6.4])
@pytest.mark.parametrize("sb", [2, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mask_content_against_float64(mods, sb, precision, far):
    """Every valid sample's 64 bits against z > 0 in float64.  Left out: entries with |z_i| <= 1e-5 ||W2_i||_1 max |h1|
    where h1 is not all zero (their share is capped at 1e-3; on the CPU the float64 reference against its own fp32
    evaluation leaves out about 2e-4); a sample with h1 = 0 has z = 0 exactly and all of its bits must be 0.  The buffer is
    pre-filled with 0xFFFFFFFF: a sample nobody wrote, and a skipped tile step that left the fill value, both show."""
    ops, functional = mods
    cache, sw, fw, ro, rd, ts, te = _scene(far=far)[:7]
    z, thr, outside = _mask_reference(far)
    n = P * HH * WW * S
    buf = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    raw = ops.render_forward_raw(ops.planes_pack(cache.cuda()), [w.cuda() for w in sw], [w.cuda() for w in fw],
                                 ro.reshape(-1, 3).cuda(), rd.reshape(-1, 3).cuda(), ts.cuda(), te.cuda(), HH * WW,
                                 ops.RenderConfig(**RCK, precision=precision, tile_sb=sb), image_w=WW, h2_mask=buf)
    assert raw["h2_mask"].data_ptr() == buf.data_ptr()
    words = buf.cpu().to(torch.int64) & 0xFFFFFFFF  # (n, 2)
    # element e of h2 <-> dword (e >> 2) & 1, bit (e & 3) + 4 (e >> 3)   (register layout LIDX, csrc/tt_device.h)
    e = torch.arange(64)
    bits = (words[:, (e >> 2) & 1] >> ((e & 3) + 4 * (e >> 3))[None, :]) & 1  # (n, 64)
    keep = (z.abs() > thr) | (thr == 0)
    left_out = 1.0 - keep.double().mean().item()
    wrong = ((bits == 1) != (z > 0)) & keep
    print(f"{_case()}: left out {left_out:.3g} of {keep.numel()} entries, wrong bits {int(wrong.sum())}, "
          f"samples outside every plane {int(outside.sum())} of {n}, fill words left {int((words == 0xFFFFFFFF).sum())}")
    assert not outside.all() and (outside.any() or far == 3.2)
    assert left_out <= 1e-3, left_out
    assert not wrong.any(), wrong.nonzero()[:8]
    assert (words[outside] == 0).all()
    assert not (words == 0xFFFFFFFF).any()


@pytest.mark.parametrize("sb", [2, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mask_path_against_recompute_path(mods, sb, precision):
    g32, g64 = _oracle()
    g_mask = _hip(mods, precision=precision, tile_sb=sb, fwd_mask=True)
    g_rec = _hip(mods, precision=precision, tile_sb=sb, fwd_mask=False)
    for tag, g in (("mask", g_mask), ("recompute", g_rec)):
        rows = check_grads(f"{_case()}[{tag}]", g, g32, g64, names=GEO_NAMES)
        print(tag, {k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})
    print("mask vs recompute:", {k: rel(a, b) for k, a, b in zip(GEO_NAMES, g_mask, g_rec)})


@pytest.mark.parametrize("scaled", [False, True], ids=["zero_and_tiny_w3", "w2_1e-6_w3_3e5"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_c_image(mods, scaled, precision):
    """C = diag(w3) W2 with 16 zero rows and 8 rows of +-1e-30, and with W2 x 1e-6, w3 x 3e5: the image is normalised on the
    products, rows of zero w3 contribute exact zeros to a1, and their rows of dW2 = w3_i D_i are exactly 0."""
    g32, g64 = _oracle(scaled)
    g = _hip(mods, scaled, precision=precision)
    rows = check_grads(_case(), g, g32, g64, names=GEO_NAMES)
    print({k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})
    assert g[2][ZERO_ROWS].abs().max().item() == 0.0
    assert g[2].abs().max().item() > 0.0


def test_points_backward_mask_product(mods):
    """tt_points_bwd_geo runs the same kernel without a forward mask: the mask product alone, on 300 points (not a multiple
    of 32), through check_grads."""
    ops, functional = mods
    gen = torch.Generator().manual_seed(SEED + 1)
    N = 300
    cache, sw, fw = _scene()[:3]
    pts = torch.rand(P, N, 3, generator=gen) * 2.2 - 1.1  # some outside the box (zeros padding)
    proj = {"sdf": torch.randn(P * N, 1, generator=gen), "sdf_grad": torch.randn(P * N, 3, generator=gen)}

    def oracle(dt):
        c = cache.to(dt).requires_grad_(True)
        ws = [w.to(dt).requires_grad_(True) for w in sw]
        o = O.geometry_forward(pts.to(dt), c, ws, [w.to(dt) for w in fw], output_normal=True, create_graph=True)
        return list(torch.autograd.grad(sum((o[k] * proj[k].to(dt)).sum() for k in proj), [c] + ws))
    g32, g64 = oracle(torch.float32), oracle(torch.float64)
    dev = "cuda"
    c = cache.to(dev).requires_grad_(True)
    ws = [w.to(dev).requires_grad_(True) for w in sw]
    sdf, sdf_grad, _ = ops.query_points_grad(c, ws, [w.to(dev) for w in fw], pts.to(dev))
    out = {"sdf": sdf, "sdf_grad": sdf_grad}
    g = [t.cpu() for t in torch.autograd.grad(sum((out[k] * proj[k].to(dev)).sum() for k in proj), [c] + ws)]
    rows = check_grads(_case(), g, g32, g64, names=GEO_NAMES)
    print({k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})
    assert g[2][ZERO_ROWS].abs().max().item() == 0.0
