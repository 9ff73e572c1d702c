"""The ray march alone (tt_march_fwd / tt_march_bwd, the nerfacc boundary: NeuS alpha -> render_weight_from_alpha ->
accumulate_along_rays x5) against the oracle on given per-sample sdf / sdf_grad / features.  S covers every kernel
variant: all passes of a ray held in registers (S <= 64, <= 128, <= 256) and the streaming form (S > 256), with
ragged last passes.  Backward = autograd of the oracle in fp64 (tolerance: as close as the fp32 oracle, x4).

The noise inputs of the first test make every ray opaque within a few dozen samples, so what the later passes compute
-- and the two values that link the passes, the forward's running transmittance and the backward's reverse-scan carry --
lies below its bars.  The `late` family (tests/march_reference.py) is there for that hand-over: one ray per crossing
index, transparent up to a surface that sits on a pass seam (samples b-2 .. b+1 of every multiple b of 64, the second
and the last two samples), so that every pass of every kernel form starts on a live ray and carries weight and gradient
mass; tests/test_march_reference_host.py checks that on the CPU.  The `edges` family adds hand-built rays at the kinks:
cos exactly 0 / -1 / +1, zero-length intervals, sdf == 0, a saturated sample, features +-100.  Both are compared element
by element -- forward, backward rows and the per-ray d loss / d inv_std -- with bars measured per ray from the oracle's
four fp32 evaluations; the forms are tied to each other bit for bit by the prefix property, and the optional upstream
gradients and the g_sdf / g_sdf_grad pass-through are compared with their explicit forms."""
import pytest
import torch
import torch.nn.functional as F

import march_reference as M
from oracle import cpu_ref as O

pytestmark = pytest.mark.gpu


def _inputs(n_rays, S, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    rd = F.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
    edges = torch.sort(torch.rand(n_rays, S + 1, generator=g) * 3.5 + 0.1, dim=1).values
    ts, te = edges[:, :-1].contiguous(), edges[:, 1:].contiguous()
    sdf = torch.randn(n_rays * S, 1, generator=g) * 0.05
    sdf_grad = torch.randn(n_rays * S, 3, generator=g)
    sdf_grad[::17] = 0.0  # F.normalize eps branch
    feat = torch.randn(n_rays * S, 3, generator=g) * 2
    return [t.to(dtype) for t in (rd, ts, te, sdf, sdf_grad, feat)]


def _oracle_march(rd, ts, te, sdf, sdf_grad, feat, inv_std, ratio):
    n_rays, S = ts.shape
    tm = ((ts + te) / 2.0).reshape(-1, 1)
    dt = (te - ts).reshape(-1, 1)
    ridx = torch.arange(n_rays).unsqueeze(-1).expand(-1, S).reshape(-1)
    normal = F.normalize(sdf_grad, dim=-1)
    alpha = O.get_alpha(sdf, normal, rd[ridx], dt, inv_std, ratio)
    w2, tr2 = O.render_weight_from_alpha(alpha.reshape(n_rays, S))
    w = w2.reshape(-1, 1)
    acc = lambda v: (w if v is None else w * v).reshape(n_rays, S, -1).sum(dim=1)
    depth = acc(tm)
    return {"opacity": acc(None), "depth": depth, "rgb_fg": acc(O.sigmoid_mipnerf(feat)),
            "z_variance": acc((tm - depth[ridx]) ** 2), "normal_acc": acc(normal), "weights": w,
            "trans": tr2.reshape(-1, 1)}


@pytest.mark.parametrize("S", [7, 64, 65, 128, 193, 256, 300])
def test_march_forward_and_backward_match_oracle(S):
    from triplaneturbo_amd import ops
    n_rays, inv_std, ratio = 37, 40.0, 0.3
    rc = ops.RenderConfig(inv_std=inv_std, cos_anneal_ratio=ratio)
    x32 = _inputs(n_rays, S, 100 + S, torch.float32)
    dev = [t.cuda() for t in x32]
    out = ops.march_forward_raw(dev[0], dev[1], dev[2], dev[3], dev[4], dev[5], rc)

    ref = {}
    for dt in (torch.float32, torch.float64):
        x = [t.to(dt) for t in x32]
        for t in x[3:]:
            t.requires_grad_(True)
        o = _oracle_march(*x, inv_std, ratio)
        g = torch.Generator().manual_seed(5)
        ups = {k: torch.randn(v.shape, generator=g).to(dt) for k, v in o.items() if k != "trans"}
        loss = sum((o[k] * ups[k]).sum() for k in ups)
        grads = torch.autograd.grad(loss, x[3:5])
        ref[dt] = (o, ups, grads)
    o32, _, g32 = ref[torch.float32]
    o64, ups, g64 = ref[torch.float64]
    for k in o64:
        e_hip = (out[k].cpu().double() - o64[k].detach()).abs().max().item()
        e_cpu = (o32[k].detach().double() - o64[k].detach()).abs().max().item()
        assert e_hip <= max(4 * e_cpu, 2e-6), (k, S, e_hip, e_cpu)

    u = {k: v.float().cuda() for k, v in ups.items()}
    ws = ops.march_backward_raw(dev[0], dev[1], dev[2], out, dev[3], dev[4], dev[5], rc, g_opacity=u["opacity"],
                                g_depth=u["depth"], g_rgb_fg=u["rgb_fg"], g_z_variance=u["z_variance"],
                                g_normal_acc=u["normal_acc"], g_weights=u["weights"])
    got = ws.cpu().double()
    want = torch.cat([g64[0], g64[1]], dim=1)
    want32 = torch.cat([g32[0], g32[1]], dim=1).double()
    live = torch.ones(n_rays * S, dtype=torch.bool)
    live[::17] = False  # zero sdf_grad: d normalize / d g = 1/eps there (1e12), compare separately in relative terms
    rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
    assert rel(got[live], want[live]) <= max(1e-4, 3 * rel(want32[live], want[live])), S
    assert rel(got[~live], want[~live]) <= max(1e-4, 3 * rel(want32[~live], want[~live])), S


def test_march_equals_the_fused_forward():
    """tt_render_fwd = decode kernel + the same march kernel: feeding its per-sample outputs back through tt_march_fwd
    reproduces its per-ray outputs bit for bit."""
    from triplaneturbo_amd import ops
    g = torch.Generator().manual_seed(3)
    P, R, Hh, Ww, S = 1, 32, 6, 5, 70
    cache = (torch.randn(P, 6, 32, R, R, generator=g) * 0.5).cuda()
    sw = [w.cuda() for w in O.init_mlp_weights([32, 64, 64, 1], g)]
    fw = [w.cuda() for w in O.init_mlp_weights([96, 64, 64, 3], g)]
    ro, rd, _, _ = O.make_cameras(1, Hh, Ww)
    ro, rd = ro.reshape(-1, 3).cuda(), rd.reshape(-1, 3).cuda()
    ts, te = O.uniform_intervals(Hh * Ww, S, 0.3, 3.2)
    ts, te = ts.cuda(), te.cuda()
    rc = ops.RenderConfig(inv_std=50.0)
    full = ops.render_forward_raw(ops.planes_pack(cache), sw, fw, ro, rd, ts, te, Hh * Ww, rc, image_w=Ww)
    again = ops.march_forward_raw(rd, ts, te, full["sdf"], full["sdf_grad"], full["features"], rc)
    for k in again:
        assert torch.equal(again[k], full[k]), k


# ------------------------------------------------------------------ the pass hand-over: late surfaces, element-wise bars
G_NAMES = ("g_opacity", "g_depth", "g_rgb_fg", "g_z_variance", "g_normal_acc", "g_weights")


def _subset(c, rays=None, S=None):
    """The inputs and upstream gradients of case `c` for some of its rays and its first S samples (device tensors)."""
    rays = torch.arange(c.n_rays) if rays is None else rays
    S = c.S if S is None else S
    per_sample = lambda t: t.reshape(c.n_rays, c.S, -1)[rays, :S].reshape(len(rays) * S, -1).contiguous().cuda()  # noqa: E731
    x = c.x32
    dev = [x[0][rays].contiguous().cuda(), x[1][rays, :S].contiguous().cuda(), x[2][rays, :S].contiguous().cuda(),
           per_sample(x[3]), per_sample(x[4]), per_sample(x[5])]
    ups = {"g_" + k: (per_sample(v) if k == "weights" else v[rays].contiguous().cuda()) for k, v in c.ups.items()}
    return dev, ups


def hip_march(c, rays=None, S=None, backward=True, **override):
    """tt_march_fwd (+ tt_march_bwd with the case's upstream gradients; override: g_* = None / a tensor) on case `c`."""
    from triplaneturbo_amd import ops
    rc = ops.RenderConfig(inv_std=c.inv_std, cos_anneal_ratio=M.RATIO, use_volsdf=c.use_volsdf)
    dev, ups = _subset(c, rays, S)
    out = dict(ops.march_forward_raw(*dev, rc))
    if backward:
        gk = torch.zeros(dev[1].shape[0], device="cuda")
        ups.update(override)
        out["ws"] = ops.march_backward_raw(dev[0], dev[1], dev[2], out, dev[3], dev[4], dev[5], rc, g_inv_std_rays=gk, **ups)
        out["gk"] = gk
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def check_case(c):
    """Every element of the forward, the backward rows and g_inv_std_rays within its allowance: all rays in one launch
    (the ray count of a family is what it is: 5, 9, 13, 17 rays leave a block of the grid ragged), then one ray alone."""
    got = hip_march(c)
    for key in M.FWD_KEYS + ("ws", "gk"):
        c.check(key, got[key])
    if c.use_volsdf and c.inv_std > 80.0:
        assert not got["gk"].any() and not c.ref64["gk"].any()  # above the clamp: exactly 0
    one = torch.tensor([c.n_rays // 2])
    alone = hip_march(c, rays=one)
    for key in M.FWD_KEYS + ("ws", "gk"):
        c.check(key, alone[key], rays=one, tag="hip, 1 ray")
        rows = one if key in M.RAY_KEYS + ("gk",) else torch.arange(c.S) + int(one) * c.S
        assert torch.equal(alone[key].reshape(len(rows), -1), got[key].reshape(-1, alone[key].numel() // len(rows))[rows]), key


@pytest.mark.parametrize("S", M.S_LIST)
def test_march_late_surfaces_meet_the_elementwise_allowance(S):
    check_case(M.case("late", S))


@pytest.mark.parametrize("S", M.EDGE_S)
def test_march_edge_rays_meet_the_allowance_and_saturate_exactly(S):
    c = M.case("edges", S)
    check_case(c)
    got = hip_march(c)
    ray = M.EDGE_RAYS.index("saturated")
    after = slice(c.sat + 1, None)
    T, w = got["trans"].reshape(c.n_rays, S)[ray], got["weights"].reshape(c.n_rays, S)[ray]
    assert T[c.sat] > 0.99 and w[c.sat] == T[c.sat]  # alpha clipped to exactly 1 on a live ray
    assert (T[after] == 0).all() and (w[after] == 0).all()
    assert (got["ws"].reshape(c.n_rays, S, 4)[ray, after] == 0).all()


def test_march_prefix_of_a_ray_is_bit_identical_in_every_form():
    """The forward's data moves only from lower lanes and earlier passes, so the first S' samples of a ray march to the
    same weights and transmittances whatever follows them -- whichever kernel form S' selects.  This ties the three
    register forms and the streaming form to each other at every seam."""
    c = M.case("late", 300)
    full = hip_march(c, backward=False)
    for Sp in M.PREFIX_S:
        part = hip_march(c, S=Sp, backward=False)
        for key in ("weights", "trans"):
            want = full[key].reshape(c.n_rays, c.S)[:, :Sp]
            got = part[key].reshape(c.n_rays, Sp)
            diff = (got != want).nonzero()
            assert diff.numel() == 0, (key, Sp, M.form_of(Sp), "first differing (ray, sample)", diff[0].tolist(),
                                       float(got[tuple(diff[0])]), float(want[tuple(diff[0])]))


@pytest.mark.parametrize("S", [129, 300])
def test_march_optional_upstream_gradients_and_pass_through(S):
    """Each upstream gradient given as None equals the run with a zero tensor bit for bit, and g_sdf / g_sdf_grad pass
    through the march boundary as one fp32 add on top of the rows computed without them."""
    c = M.case("late", S)
    _, ups = _subset(c)
    g = torch.Generator().manual_seed(11)
    extra = {"g_sdf": torch.randn(c.n_rays * S, 1, generator=g).cuda(),
             "g_sdf_grad": torch.randn(c.n_rays * S, 3, generator=g).cuda()}
    base = hip_march(c, **extra)
    for name in G_NAMES + ("g_sdf", "g_sdf_grad"):
        like = ups.get(name, extra.get(name))
        none = hip_march(c, **{**extra, name: None})
        zero = hip_march(c, **{**extra, name: torch.zeros_like(like)})
        for key in ("ws", "gk"):
            assert torch.equal(none[key], zero[key]), (name, key)
        assert not torch.equal(none["ws"], base["ws"]), name  # the gradient does reach the rows
    without = hip_march(c)
    assert torch.equal(without["ws"], hip_march(c, g_sdf=None, g_sdf_grad=None)["ws"])
    assert torch.equal(base["ws"], without["ws"] + torch.cat([extra["g_sdf"], extra["g_sdf_grad"]], dim=1).cpu())
    assert torch.equal(base["gk"], without["gk"])
