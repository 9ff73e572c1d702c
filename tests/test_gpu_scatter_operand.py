"""The B operand of the plane-gradient scatter's combine GEMM, taken from the registers of the backward kernels' last
product (tt_backward_common.h: sc2_regs_b, sc2_col, the factor tables; tt_mfma16.h: SWAP).

The geometry backward forms q^T = (W1^T a1)^T by exchanging the MFMA's two arguments and feeds it to G = M Q of all three
planes from registers; the samples' power-of-two factors travel through a 32-float table per plane, the columns of M are
permuted to match, and the [sample][33] rows of Q are written only for a plane that has a lost reference.  The cases below
are built by hand so that a test knows which of these paths its tile steps take; where the property is geometric (distinct
texels of a plane-tile, collisions in the scatter's 16 x 16 torus table) it is computed here from the sample positions and
asserted, so a case cannot silently stop covering its path.  Shapes are small: 32 - 49 rays, 5 - 8 samples, planes 16 x 16
to 64 x 64; a tile is the 32 rays of a 4 x 8 view at one sample index (tile_sb = 1) unless a test says otherwise.

Every gradient is held against oracle.cpu_ref (fp32 and fp64) under the bars of tests/parity.py, in all three precision
modes, through the entries that take the forward's h2 mask and through the ones that recompute it.  The two entries differ
in where the sign mask comes from and in float-atomic order only; each is within TOL_VS_FP32 of the fp32 oracle, so they are
asserted to lie within 2 x TOL_VS_FP32 of each other (triangle inequality) and the measured distance is printed.

Every case was first run through the oracle alone (SEEDS: the seeds kept): on every gradient the fp32 oracle is within 7e-6
of fp64, within 2e-6 of its own alternative summation order (oracle.cpu_ref.alt_order) and meets the element-wise bar of
tests/parity.py against fp64 on every element of the small matrices -- the ray-marched cases leave the
two normal images out of the loss for that, see case_inside -- and the kink mask (parity.kink_free_rays) takes out at most
10 % of a case's rays."""
import pytest
import torch

from oracle import cpu_ref as O

from parity import PRECISIONS, TOL_VS_FP32, check_grads, rel
from test_gpu_backward import KEYS, NAMES, _check, mods  # noqa: F401  (fixture)
from test_gpu_single_plane import RCK, _rays_out_along, _scene, prepared

pytestmark = pytest.mark.gpu

SEEDS = {"dense": 3, "n33": 3, "n65": 7, "sparse": 6, "ragged": 1, "axis": 3, "cross": 7, "points": 23}
PLANE_AXES = ((0, 1), (0, 2), (2, 1))  # (u, v) of planes 0..2: (x, y), (x, z), (z, y)


def case_inside(name, R, spread, n_view=1, Hh=4, Ww=8, S=6, **extra):
    """Parallel rays inside the cube: origins within spread / 2 of a centre, 0.2 long -- all three planes are live in every
    tile step, and the 32 points of a tile keep their mutual offsets from sample to sample, so `spread` alone sets how many
    distinct texels a tile touches on an R x R plane (its footprint is at most spread / 2 * R + 2 texels wide)."""
    g, cache, sw, fw = _scene(1, R, SEEDS[name])
    centre = (torch.rand(3, generator=g) - 0.5) * 0.4
    ro = centre + (torch.rand(n_view, Hh, Ww, 3, generator=g) - 0.5) * spread
    rd = torch.nn.functional.normalize(torch.randn(3, generator=g), dim=-1).expand(n_view, Hh, Ww, 3).contiguous()
    ts, te = O.uniform_intervals(n_view * Hh * Ww, S, 0.0, 0.2)
    # (the loss leaves the two normal images out, as test_gpu_single_plane.case_entering does: over rays this short, or this
    # far apart, the normalised accumulated normal is ill-conditioned -- the fp32 oracle itself moves by 1e-4 .. 1e-3 with
    # its summation order; the normal chain still carries gradient through sdf_grad)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=n_view, g=g, loss_keys=KEYS[:5], **extra)


def case_axis():
    """32 rays outside the cube along x: plane 2 alone is live in every executed tile step."""
    g, cache, sw, fw = _scene(1, 16, SEEDS["axis"])
    ro, rd = _rays_out_along(torch.zeros((1, 4, 8), dtype=torch.long), g, 1, 4, 8)
    ts, te = O.uniform_intervals(32, 8, 0.0, 0.8)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=1, g=g)


def case_crossing():
    """35 parallel rays (a ragged second tile) that enter the cube along +x: the samples at x = -1.9 .. -1.1 see plane 2
    (z, y) alone, the ones at x = -0.9 .. -0.5 all three -- with tile_sb = 1, 2, 4 a work item runs single-plane tile steps
    first and three-plane ones after them."""
    g, cache, sw, fw = _scene(1, 16, SEEDS["cross"])
    ro = torch.cat([torch.full((1, 5, 7, 1), -2.0), (torch.rand(1, 5, 7, 2, generator=g) - 0.5) * 0.8], -1)
    rd = torch.tensor([1.0, 0.0, 0.0]).expand(1, 5, 7, 3).contiguous()
    ts, te = O.uniform_intervals(35, 8, 0.0, 1.6)
    return dict(cache=cache, sw=sw, fw=fw, ro=ro, rd=rd, ts=ts, te=te, n_view=1, g=g, loss_keys=KEYS[:5])


CASES = {
    "dense": lambda: case_inside("dense", 16, 0.4),                     # at most 5 x 5 texels: n <= 32
    "n33": lambda: case_inside("n33", 32, 0.4),                         # at most 8 x 8 texels: 32 < n <= 64
    "n65": lambda: case_inside("n65", 64, 0.44),                        # at most 16 x 16 texels: n > 64, no collision
    "sparse": lambda: case_inside("sparse", 64, 1.3, n_view=2),         # ~42 texels wide: table collisions, two tiles
    "ragged": lambda: case_inside("ragged", 16, 0.4, Hh=5, Ww=7, S=5),  # 35 rays: 29 invalid lanes in the second tile
    "axis": case_axis,
    "cross": case_crossing,
}


def plane_tile_stats(c):
    """Per plane-tile (view, sample index, plane; the tile of tile_sb = 1 on a 4 x 8 view): (occupied entries of the 16 x 16
    torus table = rows of M, distinct texels that lose their entry to another texel)."""
    B, Hh, Ww, _ = c["ro"].shape
    assert Hh * Ww == 32
    R = c["cache"].shape[-1]
    tm = ((c["ts"] + c["te"]) * 0.5).double()
    pts = c["ro"].reshape(-1, 1, 3).double() + c["rd"].reshape(-1, 1, 3).double() * tm[..., None]
    out = []
    for b in range(B):
        for s in range(tm.shape[1]):
            p = pts[32 * b:32 * b + 32, s]
            for ua, va in PLANE_AXES:
                x0 = torch.floor(((p[:, ua] + 1) * R - 1) / 2).long().tolist()
                y0 = torch.floor(((p[:, va] + 1) * R - 1) / 2).long().tolist()
                texels = {(x + dx, y + dy) for x, y in zip(x0, y0) for dx in (0, 1) for dy in (0, 1)
                          if 0 <= x + dx < R and 0 <= y + dy < R}
                entries = {(x & 15, y & 15) for x, y in texels}
                out.append((len(entries), len(texels) - len(entries)))
    return out


def run(mods, c, scale=1.0, stats=False, **knobs):
    """Gradients of `scale` x the case's loss through the HIP path, divided by `scale` again (float64)."""
    ops, functional = mods
    dev = "cuda"
    st = torch.zeros((3, 4), dtype=torch.int64, device=dev) if stats else None
    cache = c["cache"].to(dev).requires_grad_(True)
    sws = [w.to(dev).requires_grad_(True) for w in c["sw"]]
    fws = [w.to(dev).requires_grad_(True) for w in c["fw"]]
    rc = ops.RenderConfig(**dict(RCK, **({"stats": st} if stats else {}), **knobs))
    out = functional.volume_render(cache, sws, fws, c["ro"].to(dev), c["rd"].to(dev), c["ts"].to(dev), c["te"].to(dev),
                                   c["bg"].to(dev), c["cd"].to(dev), c["c2w"].to(dev), rc, training=True)
    loss = O.synthetic_loss(out, {k: v.to(dev) for k, v in c["proj"].items()}, sample_mask=c["smask"]) * scale
    grads = [g.cpu().double() / scale for g in torch.autograd.grad(loss, [cache] + sws + fws)]
    for n, g in zip(NAMES, grads):
        assert torch.isfinite(g).all(), n
    return grads, (st.cpu().tolist() if stats else None)


def check_both_entries(mods, name, precision, **knobs):
    """The case through the h2-mask entries and through the recompute entries: each against the oracle, and against each
    other."""
    c = prepared("scatter_operand_" + name, CASES[name])
    assert float(c["keep"].float().mean()) >= 0.9, name
    g32, g64 = c["o32"][2], c["o64"][2]
    got = {}
    for tag, fwd_mask in (("mask", True), ("recompute", False)):
        got[tag], _ = run(mods, c, precision=precision, fwd_mask=fwd_mask, **knobs)
        rows = _check(got[tag], g32, g64)
        print(name, precision, tag, {k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})
    d = {n: rel(a, b) for n, a, b in zip(NAMES, got["mask"], got["recompute"])}
    print(name, precision, "mask vs recompute", d)
    for n, v in d.items():
        assert v <= 2 * TOL_VS_FP32, (name, n, v)
    return c


@pytest.mark.parametrize("precision", PRECISIONS)
def test_three_live_planes(mods, precision):
    """Every tile step scatters all three planes from the one q^T / the three tiles of ebar^T; n <= 32 rows per plane-tile."""
    c = check_both_entries(mods, "dense", precision, tile_sb=1)
    assert max(n for n, _ in plane_tile_stats(c)) <= 32
    _, st = run(mods, c, stats=True, precision=precision, tile_sb=1)
    for r in range(3):
        assert st[r][1] > 0 and st[r][3] == 0, (r, st)  # executed tile steps, none on the single-plane path


@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_plane_steps(mods, precision):
    c = check_both_entries(mods, "axis", precision, tile_sb=1)
    _, st = run(mods, c, stats=True, precision=precision, tile_sb=1)
    for r in range(3):
        assert st[r][1] > 0 and st[r][3] == st[r][1], (r, st)  # every executed tile step took scatter_one_plane


@pytest.mark.parametrize("sb", [1, 2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_items_that_alternate_between_the_two_paths(mods, precision, sb):
    """scatter_one_plane and scatter_planes inside one work item: each must leave M, the texel table and the factor tables
    fit for the other."""
    c = check_both_entries(mods, "cross", precision, tile_sb=sb, tile_chunk=4)
    _, st = run(mods, c, stats=True, precision=precision, tile_sb=sb, tile_chunk=4)
    for r in range(3):
        assert 0 < st[r][3] < st[r][1], (r, st)  # both paths ran


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_than_32_distinct_texels(mods, precision):
    """The second row tile of M (rows 32..63) is read and multiplied."""
    c = check_both_entries(mods, "n33", precision, tile_sb=1)
    stats = plane_tile_stats(c)
    assert any(32 < n <= 64 for n, _ in stats) and max(n for n, _ in stats) <= 64, stats
    assert all(lost == 0 for _, lost in stats), stats


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_than_64_distinct_texels(mods, precision):
    """The second 64-row pass: M is refilled with the rows of ranks 64.., the B operand in registers is used again."""
    c = check_both_entries(mods, "n65", precision, tile_sb=1)
    stats = plane_tile_stats(c)
    assert any(n > 64 for n, _ in stats), stats
    assert all(lost == 0 for _, lost in stats), stats


@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_table_collisions_stage_the_lost_rows(mods, precision, copies):
    """Rays spread over ~45 texels of a 64 x 64 plane: texels that collide in the 16 x 16 torus table lose their entry and go
    through scatter_lost, which reads the [sample][33] rows of Q -- written from the registers only then."""
    c = check_both_entries(mods, "sparse", precision, tile_sb=1, grad_copies=copies)
    stats = plane_tile_stats(c)
    assert sum(lost > 0 for _, lost in stats) >= len(stats) // 2, stats  # most plane-tiles have lost references
    assert any(n > 64 for n, _ in stats), stats                            # ... and some the second pass as well


@pytest.mark.parametrize("sb", [2, 4])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_ragged_tiles(mods, precision, sb):
    """35 rays, 5 samples: the second tile has 3 valid rays, and the last tile step of a ray runs past the chunk."""
    check_both_entries(mods, "ragged", precision, tile_sb=sb)


@pytest.mark.parametrize("log2_scale", [-70, 45])
@pytest.mark.parametrize("name", ["dense", "sparse"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_upstream_gradients_of_any_scale(mods, precision, name, log2_scale):
    """The factor table holds (deferred factor of the product) x (inverse of the sample's coefficient normalisation): with the
    loss scaled by 2^-70 or 2^45 both move by as many binades, and the scaled-back gradients must still meet the oracle's
    bars -- with three live planes, and on the lost-reference path."""
    c = prepared("scatter_operand_" + name, CASES[name])
    g, _ = run(mods, c, scale=2.0 ** log2_scale, precision=precision, tile_sb=1)
    rows = _check(g, c["o32"][2], c["o64"][2])
    print(name, precision, log2_scale, {k: (r["hip_vs_fp32"], r["hip_vs_fp64"]) for k, r in rows.items()})


_POINTS = {}


def _points_case():
    """50 query points on 32 x 32 planes (a full tile and a ragged one; some points outside the cube): a tile of random
    points touches ~100 distinct texels per plane, so the per-point entries take the second pass and the lost-reference
    path."""
    if not _POINTS:
        gen = torch.Generator().manual_seed(SEEDS["points"])
        cache = torch.randn(1, 6, 32, 32, 32, generator=gen) * 0.5
        sw = O.init_mlp_weights([32, 64, 64, 1], gen)
        fw = O.init_mlp_weights([96, 64, 64, 3], gen)
        pts = torch.rand(1, 50, 3, generator=gen) * 2.2 - 1.1
        keys = ("sdf", "features", "sdf_grad", "normal")
        proj = {k: torch.randn(50, 1 if k == "sdf" else 3, generator=gen) for k in keys}

        def oracle(dt):
            c = cache.to(dt).requires_grad_(True)
            ws = [w.to(dt).requires_grad_(True) for w in sw + fw]
            o = O.geometry_forward(pts.to(dt), c, ws[:3], ws[3:], output_normal=True, create_graph=True)
            return list(torch.autograd.grad(sum((o[k] * proj[k].to(dt)).sum() for k in keys), [c] + ws))
        _POINTS.update(cache=cache, sw=sw, fw=fw, pts=pts, proj=proj, g32=oracle(torch.float32), g64=oracle(torch.float64))
    return _POINTS


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_point_entries(precision):
    """tt_points_bwd_geo / tt_points_bwd_tex: the same two kernels on "rays" of one sample."""
    import triplaneturbo_amd as tt
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    p = _points_case()
    dev = torch.device("cuda", 0)
    geo = tt.find("few-step-triplane-dual-stable-diffusion")({}).to(dev)
    geo.precision = precision
    with torch.no_grad():
        for dst, src in zip(list(geo.sdf_network.weights()) + list(geo.feature_network.weights()), p["sw"] + p["fw"]):
            dst.copy_(src.to(dev))
    c = p["cache"].to(dev).requires_grad_(True)
    out = geo(p["pts"].to(dev), c, output_normal=True)
    loss = sum((out[k].reshape(50, -1) * p["proj"][k].to(dev)).sum() for k in p["proj"])
    params = [c] + list(geo.sdf_network.weights()) + list(geo.feature_network.weights())
    g_hip = [t.cpu() for t in torch.autograd.grad(loss, params)]
    rows = check_grads(f"scatter_operand points [{precision}]", g_hip, p["g32"], p["g64"])
    print(precision, {k: (r["hip_vs_fp32"], r["hip_vs_fp64"], r["fp32_vs_fp64"]) for k, r in rows.items()})
