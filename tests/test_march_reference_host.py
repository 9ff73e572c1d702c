"""Conditions on the INPUTS of the element-wise ray-march tests (tests/march_reference.py), checked on the CPU against the
float64 reference alone: the `late` family keeps a ray alive into every 64-sample pass and puts weight and gradient mass
there, the bars built from the fp32 evaluations are not degenerate, the noise inputs of the older march test do not
meet the coverage condition (which is why the family exists), and every `edges` ray has a finite reference."""
import math

import pytest
import torch

import march_reference as M
from parity import ATOL_ELEM, RTOL_ELEM

SATURATED_X = math.log(31.0)  # 1 - logistic(x) < 2^-5
PRIMARY_WS_CAP = 4.0
PRIMARY_GK_CAP = 4.0
PRIMARY_GK_FLOOR_CAP = 32.0


@pytest.mark.parametrize("use_volsdf", [False, True], ids=["neus", "volsdf"])
@pytest.mark.parametrize("S", M.S_LIST)
def test_late_family_reaches_every_pass(S, use_volsdf):
    """Every pass has a ray with T >= 0.5 at the pass's first sample and weight mass >= 0.25 inside the pass, and the
    pass's largest |ws| (rows with a non-zero sdf_grad) is >= 0.1 of the tensor's."""
    c = M.case("late", S, use_volsdf)
    assert c.n_rays <= 21 and c.n_rays == len(M.crossings(S)) + 1
    for row in M.coverage(S, c.ref64, c.x32):
        print(f"coverage late S={S} {'volsdf' if use_volsdf else 'neus'} pass {row['pass']}: T_start {row['T_start']:.3f} "
              f"mass {row['mass']:.3f} ws_frac {row['ws_frac']:.3f}")
        assert row["mass"] >= 0.25, (S, row)  # (mass counts only rays with T >= 0.5 at the pass's first sample)
        assert row["ws_frac"] >= 0.1, (S, row)


@pytest.mark.parametrize("S", [65, 193, 256, 300])
def test_noise_inputs_do_not_reach_the_later_passes(S):
    """The inputs of test_march_forward_and_backward_match_oracle: past the first pass no ray is alive, so a wrong
    hand-over between passes changes nothing above that test's floor of 2e-6."""
    from test_gpu_march import _inputs  # the function that test runs (importing it needs no GPU)
    x32 = _inputs(37, S, 100 + S, torch.float32)
    ref = M.evaluate(x32, torch.float64, 0, M.INV_STD)
    rows = M.coverage(S, ref, x32)
    print([(r["pass"], f"{r['T_start']:.1e}", f"{r['mass']:.1e}") for r in rows])
    assert all(r["mass"] < 0.25 for r in rows[1:]), rows
    assert all(r["T_start"] < 0.5 for r in rows[1:]), rows
    assert all(r["T_start"] <= 2e-6 for r in rows[3:]), rows  # at or below that test's floor from the fourth pass on
    if S == 65:
        assert rows[1]["T_start"] <= 2e-6, rows  # and so is the one-sample second pass


@pytest.mark.parametrize("family,S,use_volsdf", [("late", S, v) for S in M.S_LIST for v in (False, True)]
                         + [("edges", S, False) for S in M.EDGE_S])  # (edges: the cosine kinks and the clip are NeuS's)
def test_the_yardstick_is_not_degenerate(family, S, use_volsdf):
    """Each fp32 evaluation, measured with the allowance built from the OTHER three, stays <= 0.5 of it: no bar rests on
    one outlying evaluation, and none is so tight that a valid fp32 evaluation would miss it.

    Asserted as stated for every output and evaluation but the BACKWARD of the primary evaluation under NeuS, where it
    holds on part of the elements only.  torch.sigmoid's fp32 backward is s (1 - s) with s rounded to fp32: an absolute
    error of 2^-25 in 1 - s, where the other three form the derivative to fp32 RELATIVE precision (1, 3: the logistic
    in float64; 2: from exp(-|x|)).  The HIP kernel forms sA (1 - sA) in fp32 as the primary does, so the bars keep the
    primary's vote; what is asserted for it instead:
      ws   <= 0.5 on every sample whose logistic is not saturated (1 - s >= 2^-5: the larger logistic argument
           x <= ln 31; beyond, 1 - s has lost 5 or more of its 24 bits), all populations.  On the saturated samples
           <= PRIMARY_WS_CAP (measured: 2.2, zero-sdf_grad rows of S = 65; 0.94 on edges).
      gk   a ray's gradient is the sum of its samples' shares.  The error of the shares of the unsaturated samples stays
           <= 0.5 of the ray's bar on every ray whose bar is not the ATOL floor (|gk| >= ATOL / RTOL = 1e-2 of the
           largest).  The whole gradient stays <= PRIMARY_GK_CAP there (measured 1.9, S = 300) and
           <= PRIMARY_GK_FLOOR_CAP on the floor rays (measured 15.9, S = 128: the empty ray, whose gradient is 1.6e-5
           of the largest -- 4.0e-7 against 0.0254 -- and which the primary computes as 0; other floor rays are sums of
           shares 1e3 times their size).
    The caps are twice the measured figures: a yardstick that drifts past them fails here."""
    c = M.case(family, S, use_volsdf)
    exempt = not use_volsdf
    saturated = M.logistic_argument(c.x32, c.inv_std) > SATURATED_X if exempt else None
    for lv in range(4):
        bars = c.bars_from([e for j, e in enumerate(c.evals32) if j != lv])
        for key in M.FWD_KEYS + ("ws", "gk"):
            r = M.ratios(c.evals32[lv][key], c.ref64[key], bars[key])
            if lv == 3 and key == "ws":  # x / sqrt(|x|^2) has no autograd derivative at x = 0: no value, no vote there
                assert torch.equal(torch.isnan(r), c.populations["eps"][0]), (family, S)
                r = torch.nan_to_num(r, nan=0.0)
            assert torch.isfinite(r).all(), (family, S, lv, key)
            print(f"yardstick {family} S={S} {'volsdf' if use_volsdf else 'neus'} {key}: fp32 evaluation {lv} "
                  f"error/allowance(other three) {float(r.max()):.3f}")
            if not (lv == 0 and exempt and key in ("ws", "gk")):
                assert float(r.max()) <= 0.5, (family, S, lv, key, float(r.max()))
            elif key == "ws":
                sat = saturated.reshape(-1, 1).expand(-1, 4)
                plain, capped = float((r * ~sat).max()), float((r * sat).max())
                print(f"yardstick {family} S={S} neus ws: primary, unsaturated samples {plain:.3f}, saturated {capped:.3f}")
                assert plain <= 0.5 and capped <= PRIMARY_WS_CAP, (family, S, plain, capped)
            else:
                ref = c.ref64["gk"].abs()
                floor = ref < ATOL_ELEM / RTOL_ELEM * ref.max()
                d = (c.evals32[0]["gk_samples"] - c.ref64["gk_samples"]).reshape(-1) * ~saturated
                shares = d.reshape(c.n_rays, S).sum(dim=1).abs() / bars["gk"]
                plain, capped, at_floor = float((shares * ~floor).max()), float((r * ~floor).max()), float((r * floor).max())
                print(f"yardstick {family} S={S} neus gk: primary, unsaturated shares {plain:.3f}, whole {capped:.3f}, "
                      f"rays at the ATOL floor ({int(floor.sum())} of {c.n_rays}) {at_floor:.3f}")
                assert plain <= 0.5 and capped <= PRIMARY_GK_CAP and at_floor <= PRIMARY_GK_FLOOR_CAP, (family, S)


@pytest.mark.parametrize("S", M.EDGE_S)
def test_edges_rays_have_a_finite_reference(S):
    """Every hand-built ray has a finite float64 reference, the primary (cumprod) and recurrence forms agree on it, and
    the saturated ray is saturated: alpha == 1 at its sample, T == 0 and zero gradient rows after it."""
    c = M.case("edges", S)
    for key, v in c.ref64.items():
        assert torch.isfinite(v).all(), (S, key)
    prim = M.evaluate(c.x32, torch.float64, 0, c.inv_std, ups=c.ups)
    for key, v in c.ref64.items():
        assert torch.isfinite(prim[key]).all(), (S, key)
        scale = v.abs().reshape(c.n_rays, -1).amax(dim=1).clamp_min(1e-6 * v.abs().max())
        d = ((prim[key] - v).abs().reshape(c.n_rays, -1).amax(dim=1) / scale).max().item()
        assert d <= 1e-9, (S, key, d)  # per ray, relative to the ray's largest value (the saturated ray's d / d inv_std
        #                                is ~1e-169: relative to 1e-6 of the tensor's largest there)
    ray = M.EDGE_RAYS.index("saturated")
    T = c.ref64["trans"].reshape(c.n_rays, S)[ray]
    w = c.ref64["weights"].reshape(c.n_rays, S)[ray]
    ws = c.ref64["ws"].reshape(c.n_rays, S, 4)[ray]
    assert T[c.sat] > 0.99 and w[c.sat] == T[c.sat]  # alpha == 1 there, the ray alive up to it
    assert (T[c.sat + 1:] == 0).all() and (w[c.sat + 1:] == 0).all() and (ws[c.sat + 1:] == 0).all()
    # the inputs are small dyadic numbers (multiples of 1 / 256): exact in every format, and so are the three cosines
    for t in c.x32:
        assert torch.equal(t, (t.double() * 256).round().div(256).float())
