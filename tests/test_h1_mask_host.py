"""The identity behind the one-product geometry backward (csrc/tt_backward.hip, "One W1 product"), on the CPU in float64:
with m1, m2 the sign masks of h1 = relu(W1 f), h2 = relu(W2 h1) and u = sbar f + J gbar,

    D = sum_samples m2 (m1 . W1 u)^T,    dW2_ij = w3_i D_ij,    dw3_i = sum_j W2_ij D_ij,    dW1 = sum_samples a1 u^T

equal autograd's gradients of the full render loss (second-order chain through sdf_grad included), rows of zero and +-1e-30
w3 included.  Also: the sign-mask bit layout helpers of ops.py, the additive ABI entries, and what the float64 mask reference
of tests/test_gpu_h1_mask.py leaves out."""
import ctypes

import pytest
import torch

from oracle import cpu_ref as O

from h1_mask_scene import HH, P, RCK, S, WW, ZERO_ROWS, TINY_ROWS, h1_reference, scene


def _upstreams_and_grads(scaled):
    """float64: f, u = sbar f + J gbar per sample from autograd's upstreams of sdf and sdf_grad, and autograd's dW1, dW2, dw3."""
    d = torch.float64
    cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = scene(scaled)
    c = cache.to(d)
    sws = [w.to(d).requires_grad_(True) for w in sw]
    out = O.render(c, sws, [w.to(d) for w in fw], ro.to(d), rd.to(d), ts.to(d), te.to(d), bg.to(d), cd.to(d), c2w.to(d),
                   **RCK)
    loss = O.synthetic_loss(out, {k: v.to(d) for k, v in proj.items()})
    # upstream of sdf; of sdf_grad directly (eikonal term) and through normal = normalize(sdf_grad) (alpha, comp_normal)
    sbar, g_direct, nbar = torch.autograd.grad(loss, [out["sdf"], out["sdf_grad"], out["normal"]], retain_graph=True)
    dW1, dW2, dw3 = torch.autograd.grad(loss, sws)
    sg = out["sdf_grad"].detach().requires_grad_(True)
    gbar = g_direct + torch.autograd.grad(O._normalize(sg), sg, nbar)[0]
    # f and J gbar (J = d f / d x: a Jacobian-vector product by double backward) at the render's sample positions
    pos = out["points"].detach().reshape(P, HH * WW * S, 3).requires_grad_(True)
    f = O.sample_from_planes(O.rotate_planes_v1(c)[:, 0:3], pos, "v1")  # radius 1: plane coordinates = positions
    cot = torch.zeros_like(f, requires_grad=True)
    jt = torch.autograd.grad(f, pos, cot, create_graph=True)[0]
    jg = torch.autograd.grad(jt, cot, gbar.reshape(P, -1, 3))[0]
    f = f.detach().reshape(-1, 32)
    u = sbar * f + jg.reshape(-1, 32)
    return [w.detach() for w in sws], f, u, (dW1, dW2, dw3)


@pytest.mark.parametrize("scaled", [False, True], ids=["zero_and_tiny_w3", "w2_1e-6_w3_3e5"])
def test_one_product_identity_against_autograd(scaled):
    (W1, W2, w3), f, u, (dW1, dW2, dw3) = _upstreams_and_grads(scaled)
    z1 = f @ W1.T
    m1 = (z1 > 0).double()
    m2 = ((torch.relu(z1) @ W2.T) > 0).double()
    v = m1 * (u @ W1.T)
    D = m2.T @ v  # D_ij = sum_samples m2_i v_j
    my_dW2 = w3[0][:, None] * D
    my_dw3 = (W2 * D).sum(dim=1)[None, :]
    a1 = m1 * ((m2 * w3) @ W2)
    my_dW1 = a1.T @ u
    for name, a, b in (("dW1", my_dW1, dW1), ("dW2", my_dW2, dW2), ("dw3", my_dw3, dw3)):
        err = ((a - b).norm() / b.norm()).item()
        print(name, "relative difference to autograd", err)
        assert b.norm().item() > 0 and err <= 1e-11, (name, err)  # float64, sums of ~900 samples in another order
    assert (my_dW2[ZERO_ROWS] == 0).all() and (dW2[ZERO_ROWS] == 0).all()
    assert my_dW2[TINY_ROWS].abs().max().item() > 0


def test_bit_layout_helpers():
    from triplaneturbo_amd import ops
    # include/tt_abi.h: bit r of dword 2*sample + hi is element (r & 3) + 8 (r >> 2) + 4 hi
    for hi in (0, 1):
        for r in range(32):
            words = torch.zeros(3, 2, dtype=torch.int32)
            words[1, hi] = ctypes.c_int32(1 << r).value
            bits = ops.sign_mask_bits(words)
            assert bits.shape == (3, 64) and bits.dtype == torch.bool
            assert bits.nonzero().tolist() == [[1, (r & 3) + 8 * (r >> 2) + 4 * hi]]
    g = torch.Generator().manual_seed(3)
    bits = torch.rand(50, 64, generator=g) > 0.5
    bits[0], bits[1] = True, False
    words = ops.sign_mask_words(bits)
    assert words.dtype == torch.int32 and words[0].tolist() == [-1, -1] and words[1].tolist() == [0, 0]
    assert (ops.sign_mask_bits(words) == bits).all()
    with pytest.raises(ValueError):
        ops.sign_mask_bits(torch.zeros(4, 3, dtype=torch.int32))


def test_entries_are_additive():
    from triplaneturbo_amd import _lib, ops
    protos = _lib._PROTOS
    for base, ext in (("tt_render_fwd_h2mask", "tt_render_fwd_masks"), ("tt_render_bwd_geo_h2mask", "tt_render_bwd_geo_masks")):
        # the h2-mask entry's arguments with the h1 mask pointer in front of the stream
        assert protos[ext][0] is protos[base][0]
        assert protos[ext][1] == protos[base][1][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    rc = ops.RenderConfig()
    assert rc.fwd_mask is True and rc.fwd_mask_h1 is True
    assert ops.RenderConfig(fwd_mask_h1=False).fwd_mask is True
    assert ops.RenderConfig(fwd_mask=False).fwd_mask is False


@pytest.mark.parametrize("far", [3.2, 6.4])
def test_mask_reference_exclusions(far):
    """What the float64 reference of the GPU mask test leaves out (cap there: 1e-3), and that an fp32 evaluation of the same
    math has no wrong bit among the kept entries."""
    z, thr, outside = h1_reference(far)
    z32 = h1_reference(far, torch.float32)[0]
    keep = (z.abs() > thr) | (thr == 0)
    left_out = 1.0 - keep.double().mean().item()
    wrong = ((z32 > 0) != (z > 0)) & keep
    print(f"far {far}: left out {left_out:.3g} of {keep.numel()} entries, fp32 wrong bits {int(wrong.sum())}, "
          f"samples outside every plane {int(outside.sum())}")
    assert left_out <= 1e-3
    assert not wrong.any()
    assert (z[outside] == 0).all() and not outside.all()
