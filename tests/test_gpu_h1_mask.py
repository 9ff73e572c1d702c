"""Geometry backward with BOTH sign masks from the forward (tt_render_fwd_masks / tt_render_bwd_geo_masks) and the one-product
form v = m1 . (W1 u) (csrc/tt_backward.hip).  What the form could get wrong: the content and layout of the h1 mask words, the
words of skipped tile steps, lanes that read another sample's word (ragged tiles, clamped prefetch), the u-only gather, and v
with zero / tiny / badly scaled output weights.  Scene: tests/h1_mask_scene.py (the one of tests/test_gpu_h2_mask.py)."""
import os

import pytest
import torch

from oracle import cpu_ref as O

from h1_mask_scene import GEO_NAMES, HH, P, RCK, S, WW, ZERO_ROWS, h1_reference, oracle, scene
from parity import PRECISIONS, TOL_VS_FP32, check_grads, rel  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from triplaneturbo_amd import functional, ops
    return ops, functional


def _hip(mods, scaled=False, **rc_kwargs):
    ops, functional = mods
    cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = scene(scaled)
    dev = "cuda"
    c = cache.to(dev).requires_grad_(True)
    sws = [w.to(dev).requires_grad_(True) for w in sw]
    out = functional.volume_render(c, sws, [w.to(dev) for w in fw], ro.to(dev), rd.to(dev), ts.to(dev), te.to(dev),
                                   bg.to(dev), cd.to(dev), c2w.to(dev), ops.RenderConfig(**RCK, **rc_kwargs), training=True)
    loss = O.synthetic_loss(out, {k: v.to(dev) for k, v in proj.items()})
    return [t.cpu() for t in torch.autograd.grad(loss, [c] + sws)]


def _case():
    return os.environ.get("PYTEST_CURRENT_TEST", "test_gpu_h1_mask").split("::")[-1].split(" ")[0]


def _report(rows):
    print({k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})


# far = 3.2: every sample still has one plane with an in-bounds texel (single-plane tile steps, none skipped); far = 6.4 adds
# samples outside every plane and tile steps that are skipped altogether.
@pytest.mark.parametrize("far", [3.2, 6.4])
@pytest.mark.parametrize("sb", [2, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_h1_mask_content_against_float64(mods, sb, precision, far):
    """Every valid sample's 64 bits of h1_mask against z = W1 f > 0 in float64.  Left out: entries with |z_i| <= 1e-5 ||W1_i||_1
    max |f| (their share is capped at 1e-3; tests/test_h1_mask_host.py: the reference leaves out 8.6e-5 / 3.4e-5 and its own fp32
    evaluation has no wrong bit among the rest); a sample with f = 0 has z = 0 exactly and all of its bits must be 0.  Both
    buffers are pre-filled with 0xFFFFFFFF: a sample nobody wrote, and a skipped tile step that left the fill value, both show.
    The h2 words of the same launch are those of tt_render_fwd_h2mask, bit for bit."""
    ops, functional = mods
    cache, sw, fw, ro, rd, ts, te = scene(far=far)[:7]
    z, thr, outside = h1_reference(far)
    n = P * HH * WW * S
    rc = ops.RenderConfig(**RCK, precision=precision, tile_sb=sb)
    args = (ops.planes_pack(cache.cuda()), [w.cuda() for w in sw], [w.cuda() for w in fw], ro.reshape(-1, 3).cuda(),
            rd.reshape(-1, 3).cuda(), ts.cuda(), te.cuda(), HH * WW, rc)
    buf1 = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    buf2 = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    raw = ops.render_forward_raw(*args, image_w=WW, h2_mask=buf2, h1_mask=buf1)
    assert raw["h1_mask"].data_ptr() == buf1.data_ptr() and raw["h2_mask"].data_ptr() == buf2.data_ptr()
    h2_only = ops.render_forward_raw(*args, image_w=WW, h2_mask=True)
    assert torch.equal(h2_only["h2_mask"], buf2)
    for k in ("opacity", "depth", "rgb_fg", "sdf", "sdf_grad", "features", "weights"):
        assert torch.equal(h2_only[k], raw[k]), k
    bits = ops.sign_mask_bits(buf1.cpu())  # (n, 64)
    words = buf1.cpu().to(torch.int64) & 0xFFFFFFFF
    keep = (z.abs() > thr) | (thr == 0)
    left_out = 1.0 - keep.double().mean().item()
    wrong = (bits != (z > 0)) & keep
    print(f"{_case()}: left out {left_out:.3g} of {keep.numel()} entries, wrong bits {int(wrong.sum())}, "
          f"samples outside every plane {int(outside.sum())} of {n}, fill words left {int((words == 0xFFFFFFFF).sum())}")
    assert not outside.all() and (outside.any() or far == 3.2)
    assert left_out <= 1e-3, left_out
    assert not wrong.any(), wrong.nonzero()[:8]
    assert (words[outside] == 0).all()
    assert not (words == 0xFFFFFFFF).any()


@pytest.mark.parametrize("sb", [2, 8])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_product_path_against_oracles(mods, sb, precision):
    """Gradients of the new path against the fp32 and fp64 oracles (tests/parity.py), both tile shapes, every precision (the
    fp32-MFMA mode ignores the h1 mask).  Printed: the distance to the h2-only path and to the recompute path."""
    g32, g64 = oracle()
    g_new = _hip(mods, precision=precision, tile_sb=sb)
    g_h2 = _hip(mods, precision=precision, tile_sb=sb, fwd_mask_h1=False)
    g_rec = _hip(mods, precision=precision, tile_sb=sb, fwd_mask=False)
    _report(check_grads(_case(), g_new, g32, g64, names=GEO_NAMES))
    print("one product vs h2-only:", {k: rel(a, b) for k, a, b in zip(GEO_NAMES, g_new, g_h2)})
    print("one product vs recompute:", {k: rel(a, b) for k, a, b in zip(GEO_NAMES, g_new, g_rec)})


@pytest.mark.parametrize("scaled", [False, True], ids=["zero_and_tiny_w3", "w2_1e-6_w3_3e5"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_zero_tiny_and_scaled_w3(mods, scaled, precision):
    """w3 with 16 zero rows and 8 rows of +-1e-30, and with W2 x 1e-6, w3 x 3e5: rows of zero w3 give exactly 0 in dW2 = w3_i D_i."""
    g32, g64 = oracle(scaled)
    g = _hip(mods, scaled, precision=precision)
    _report(check_grads(_case(), g, g32, g64, names=GEO_NAMES))
    assert g[2][ZERO_ROWS].abs().max().item() == 0.0
    assert g[2].abs().max().item() > 0.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_mixed_tile_steps_and_stats(mods, precision):
    """far = 3.2 with one sample per lane group (tile_sb = 1): a work item's tile steps alternate between one live plane (the
    ray outside the cube along one axis) and three; the same launch again with the work accounting compiled in (STATS)."""
    ops, functional = mods
    g32, g64 = oracle()
    g = _hip(mods, precision=precision, tile_sb=1)
    _report(check_grads(_case() + "[plain]", g, g32, g64, names=GEO_NAMES))
    st = torch.zeros(3, 4, dtype=torch.int64, device="cuda")
    g_st = _hip(mods, precision=precision, tile_sb=1, stats=st)
    _report(check_grads(_case() + "[stats]", g_st, g32, g64, names=GEO_NAMES))
    visited, executed, _, single = st.cpu().tolist()[1]  # the geometry backward's row
    print("geometry backward tile steps: visited", visited, "executed", executed, "single-plane", single)
    assert 0 < single < executed <= visited
    for k, a, b in zip(GEO_NAMES, g, g_st):
        assert rel(a, b) <= TOL_VS_FP32, k  # the bar between two fp32 evaluations of one gradient (tests/parity.py)
