"""The single-plane path of the three decode kernels (tt_device.h, "plane mask of a tile step").

A tile step in which exactly ONE plane has an in-bounds texel -- the samples have left the cube along one axis, so only the
plane that does not use that axis still sees them -- runs the live plane's share of `V1 e` and that plane's gradient scatter
alone (scatter_one_plane); every other plane mask takes the general code.  The ray bundles here are built by hand so that
a test knows which path its tile steps take, and tt_render_cfg.stats[3] (executed tile steps that took the single-plane
path) says whether they did.  Forward outputs and every gradient are held against the CPU oracle with the bars of
tests/parity.py; rays with a sample on a ReLU kink leave the loss as in the fuzz (parity.kink_free_rays).

Every case was first run through the oracle alone (fp32 and fp64): the fp32 oracle meets the plain 1e-4 bar against fp64 on
every gradient of every case below, and the kink mask takes out at most 5 % of a case's rays (SEEDS: the seeds kept)."""
import math

import pytest
import torch

from oracle import cpu_ref as O

from parity import PRECISIONS, check_outputs, kink_free_rays
from test_gpu_backward import KEYS, _check, _hip_grads, _oracle_grads, mods  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

RCK = dict(inv_std=40.0, rgb_grad_shrink=0.7, cos_anneal_ratio=1.0)
LIVE_PLANE = {0: 2, 1: 1, 2: 0}  # axis the samples have left the cube along -> the plane that does not use it
SEEDS = {"axis": (13, 124, 213), "mixed": 24, "enter": 33, "crowded": 41}


def _frame(n_view):
    """Some valid camera frames: the renderer only uses them for the camera-space normal image and the depth range."""
    _, _, c2w, cd = O.make_cameras(n_view, 4, 4)
    return c2w, cd


def _scene(P, R, seed):
    g = torch.Generator().manual_seed(seed)
    cache = torch.randn(P, 6, 32, R, R, generator=g) * 0.5
    sw = O.init_mlp_weights([32, 64, 64, 1], g)
    fw = O.init_mlp_weights([96, 64, 64, 3], g)
    return g, cache, sw, fw


def _rays_out_along(axis_of_ray, g, n_view, Hh, Ww):
    """axis_of_ray: (n_view, Hh, Ww) int tensor.  Origin at +-1.5 on that axis (outside the radius-1 cube), the other two
    coordinates in [-0.6, 0.6]; unit direction inside the plane orthogonal to the axis: the ray never re-enters."""
    o = (torch.rand(n_view, Hh, Ww, 3, generator=g) * 2 - 1) * 0.6
    d = torch.randn(n_view, Hh, Ww, 3, generator=g)
    sign = torch.where(torch.rand(n_view, Hh, Ww, generator=g) < 0.5, -1.5, 1.5)
    idx = axis_of_ray.unsqueeze(-1)
    o.scatter_(-1, idx, sign.unsqueeze(-1))
    d.scatter_(-1, idx, torch.zeros(n_view, Hh, Ww, 1))
    return o, torch.nn.functional.normalize(d, dim=-1)


def case_axis_out(axis):
    R, S = ((16, 19), (40, 32), (16, 32))[axis]
    P, n_view, Hh, Ww = 1, 2, 4, 8
    g, cache, sw, fw = _scene(P, R, SEEDS["axis"][axis])
    ro, rd = _rays_out_along(torch.full((n_view, Hh, Ww), axis), g, n_view, Hh, Ww)
    ts, te = O.uniform_intervals(n_view * Hh * Ww, S, 0.0, 0.8)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=n_view, g=g)


def case_mixed():
    """Half the rays of every tile out along x, half out along y (pixel columns alternate; a tile is a 4x4 pixel block x 2
    samples): planes 2 and 1 are both live in every executed tile step -- a mask with two bits, the general path."""
    P, n_view, Hh, Ww, R, S = 1, 2, 4, 8, 16, 19
    g, cache, sw, fw = _scene(P, R, SEEDS["mixed"])
    axis = (torch.arange(Ww) % 2).expand(n_view, Hh, Ww).contiguous()
    ro, rd = _rays_out_along(axis, g, n_view, Hh, Ww)
    ts, te = O.uniform_intervals(n_view * Hh * Ww, S, 0.0, 0.8)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=n_view, g=g)


def case_entering():
    """Ordinary camera rays from outside the cube through it: single-plane steps on the way in and out, full steps inside.
    2 prompts x 2 views of 5x7 rays: ragged tiles, tiles that straddle prompts."""
    P, n_view, Hh, Ww, R, S = 2, 2, 5, 7, 16, 19
    g, cache, sw, fw = _scene(P, R, SEEDS["enter"])
    ro, rd, c2w, cd = O.make_cameras(P * n_view, Hh, Ww)
    ts, te = O.uniform_intervals(P * n_view * Hh * Ww, S, 0.3, 3.2)
    # The loss leaves the two normal images out: normalising the accumulated normal of a ray that crosses the whole cube
    # in 19 samples is ill-conditioned at the 1e-3 level (the fp32 oracle against fp64, every seed tried), far above the
    # bar.  The normal chain still carries gradient through the eikonal term of the loss.
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=n_view, g=g, c2w=c2w, cd=cd,
                loss_keys=KEYS[:5])


def case_crowded():
    """32 parallel rays, out along z, spread over the 40x40 plane 0 so that the 2x2 texel footprints of a tile (tile_sb = 1:
    the 32 rays at one sample index) are pairwise disjoint and distinct in the scatter's 16x16 torus table: 128 distinct
    texels per plane-tile, n > 64 -> the second 64-row pass inside scatter_one_plane."""
    P, n_view, Hh, Ww, R, S = 1, 1, 4, 8, 40, 19
    g, cache, sw, fw = _scene(P, R, SEEDS["crowded"])
    k = torch.arange(32)
    r, q = k % 8, k // 8
    bx = r + 8 * (r % 2)                    # 2x2 texel block of the ray: (bx % 8, by % 8) pairwise distinct
    by = q + 4 * ((r // 2) % 2) + 8 * (q % 2)
    ix, iy = 2.0 * bx + 0.5, 2.0 * by + 0.5  # between the block's texels
    x, y = (2 * ix + 1) / R - 1, (2 * iy + 1) / R - 1
    ro = torch.stack([x, y, torch.full_like(x, 1.5)], -1).reshape(1, Hh, Ww, 3).float()
    rd = torch.tensor([-1.0, -1.0, 0.0]).div(math.sqrt(2.0)).expand(1, Hh, Ww, 3).contiguous()
    ts, te = O.uniform_intervals(32, S, 0.0, 0.8)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=n_view, g=g)


_CASES = {}


def prepared(name, build):
    """The case's inputs, its kink mask and its oracle evaluations (fp32, fp64): computed once, shared by every test."""
    if name not in _CASES:
        c = build()
        B, Hh, Ww, _ = c["ro"].shape
        S = c["ts"].shape[1]
        if "c2w" not in c:
            c["c2w"], c["cd"] = _frame(B)
        c["bg"] = torch.ones(3)
        keep = kink_free_rays(c["cache"], c["sw"], c["fw"], c["ro"], c["rd"], c["ts"], c["te"], c["n_view"])
        keep &= kink_free_rays(c["cache"], c["sw"], c["fw"], c["ro"], c["rd"], c["ts"], c["te"], c["n_view"], net="feature")
        c["keep"] = keep
        c["proj"] = {n: torch.randn(B, Hh, Ww, ch, generator=c["g"]) * keep.view(B, Hh, Ww, 1).float()
                     for n, ch in c.get("loss_keys", KEYS)}
        c["smask"] = keep.view(-1, 1).expand(-1, S).reshape(-1).float()
        a = (c["cache"], c["sw"], c["fw"], c["ro"], c["rd"], c["ts"], c["te"], c["bg"], c["cd"], c["c2w"], c["proj"], RCK)
        c["o32"] = _oracle_grads(torch.float32, *a, sample_mask=c["smask"])
        c["o64"] = _oracle_grads(torch.float64, *a, sample_mask=c["smask"])
        _CASES[name] = c
    return _CASES[name]


def run_hip(mods, c, **knobs):
    stats = torch.zeros((3, 4), dtype=torch.int64, device="cuda")
    out, loss, grads = _hip_grads(mods, c["cache"], c["sw"], c["fw"], c["ro"], c["rd"], c["ts"], c["te"], c["bg"], c["cd"],
                                  c["c2w"], c["proj"], dict(RCK, stats=stats, **knobs), sample_mask=c["smask"])
    return out, loss, grads, stats.cpu().tolist()


def check_against_oracle(case, c, out, loss, grads):
    (o32, l32, g32), (o64, l64, g64) = c["o32"], c["o64"]
    B, Hh, Ww, _ = c["ro"].shape
    km = c["keep"].view(B, Hh, Ww, 1)
    img = [k for k, _ in KEYS]
    masked = lambda o: {k: o[k].detach().cpu().reshape(B, Hh, Ww, -1) * km.to(o[k].dtype) for k in img}  # noqa: E731
    print(check_outputs(case + " [images]", masked(out), masked(o32), masked(o64), img))
    per_sample = ("sdf", "features")
    print(check_outputs(case + " [samples]", out, o32, o64, per_sample))
    assert abs(loss - l64) <= max(4 * abs(l32 - l64), 1e-5 * abs(l64)), (case, loss, l32, l64)
    print(_check(grads, g32, g64))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_axis_out_takes_the_single_plane_path(mods, axis, precision):
    """Every ray stays outside the cube along one axis: every executed tile step has exactly one live plane (2, 1, 0 for
    x, y, z), in all three kernels; the two dead planes' texels receive exactly zero."""
    c = prepared(f"axis{axis}", lambda: case_axis_out(axis))
    out, loss, grads, st = run_hip(mods, c, precision=precision)
    print("stats", st)
    for r in range(3):
        assert st[r][1] > 0 and st[r][3] == st[r][1], (r, st)
    check_against_oracle(f"single_plane axis {axis} [{precision}]", c, out, loss, grads)
    g_planes, g64 = grads[0], c["o64"][2][0]
    live = LIVE_PLANE[axis]
    for p in range(3):
        for half in (0, 3):  # geometry planes 0..2, texture planes 3..5
            if p == live:
                assert float(g64[:, half + p].abs().max()) > 0 and float(g_planes[:, half + p].abs().max()) > 0
            else:
                assert float(g64[:, half + p].abs().max()) == 0.0  # (the oracle agrees on which planes are dead)
                assert float(g_planes[:, half + p].abs().max()) == 0.0, (axis, half + p)


def test_two_live_planes_take_the_general_path(mods):
    c = prepared("mixed", case_mixed)
    out, loss, grads, st = run_hip(mods, c)
    print("stats", st)
    for r in range(3):
        assert st[r][1] > 0 and st[r][3] == 0, (r, st)
    check_against_oracle("single_plane mixed bundle", c, out, loss, grads)
    assert float(grads[0][:, 0].abs().max()) == 0.0 and float(grads[0][:, 3].abs().max()) == 0.0  # plane 0 uses x and y


@pytest.mark.parametrize("chunk", [1, 5])
@pytest.mark.parametrize("sb", [1, 2, 8])
def test_items_that_alternate_between_the_two_paths(mods, sb, chunk):
    """Rays entering and leaving the cube: work items whose tile steps alternate between scatter_one_plane and
    scatter_planes -- each must leave the scatter matrix, the texel table and the dummy tags clean for the other."""
    c = prepared("enter", case_entering)
    out, loss, grads, st = run_hip(mods, c, tile_sb=sb, tile_chunk=chunk)
    print("stats", st)
    for r in range(3):
        assert 0 < st[r][3] < st[r][1], (r, st)  # both paths ran
    check_against_oracle(f"single_plane entering sb{sb} chunk{chunk}", c, out, loss, grads)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_crowded_single_plane_tile_takes_the_second_scatter_pass(mods, precision):
    c = prepared("crowded", case_crowded)
    out, loss, grads, st = run_hip(mods, c, tile_sb=1, precision=precision)
    print("stats", st)
    for r in range(3):
        assert st[r][1] > 0 and st[r][3] == st[r][1], (r, st)
    check_against_oracle(f"single_plane crowded [{precision}]", c, out, loss, grads)
