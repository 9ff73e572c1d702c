"""Scene and float64 reference shared by tests/test_h1_mask_host.py and tests/test_gpu_h1_mask.py: the small scene of
tests/test_gpu_h2_mask.py (2 prompts x 1 view of 7 x 5 rays x 13 samples on 16 x 16 planes, intervals 0.3 .. far, w3 with 16
exact zeros and 8 entries of +-1e-30; 70 rays and an odd S: ragged tiles and a clamped prefetch)."""
import torch

from oracle import cpu_ref as O

KEYS = (("comp_rgb", 3), ("opacity", 1), ("depth", 1), ("z_variance", 1), ("disparity", 1), ("comp_normal", 3),
        ("comp_normal_cam_vis", 3))
ZERO_ROWS = list(range(0, 64, 4))   # 16 output weights exactly 0
TINY_ROWS = list(range(1, 64, 8))   # 8 output weights +-1e-30
GEO_NAMES = ["space_cache", "sdf.w1", "sdf.w2", "sdf.w3"]
P, R, HH, WW, S, SEED = 2, 16, 7, 5, 13, 10
RCK = dict(inv_std=100.0, rgb_grad_shrink=0.7, cos_anneal_ratio=1.0)


def scene(scaled=False, far=3.2):
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


def oracle(scaled=False):
    """fp32 and fp64 oracle gradients (planes + sdf net), evaluated once per scene and process."""
    if scaled not in _ORACLE:
        cache, sw, fw, ro, rd, ts, te, bg, cd, c2w, proj = scene(scaled)

        def run(d):
            c = cache.to(d).requires_grad_(True)
            sws = [w.to(d).requires_grad_(True) for w in sw]
            out = O.render(c, sws, [w.to(d) for w in fw], ro.to(d), rd.to(d), ts.to(d), te.to(d), bg.to(d), cd.to(d),
                           c2w.to(d), **RCK)
            return list(torch.autograd.grad(O.synthetic_loss(out, {k: v.to(d) for k, v in proj.items()}), [c] + sws))
        _ORACLE[scaled] = (run(torch.float32), run(torch.float64))
    return _ORACLE[scaled]


_H1_REF = {}


def h1_reference(far, dtype=torch.float64):
    """z = W1 f per sample (n, 64) with f from the oracle's plane sampling in `dtype`, the per-entry exclusion threshold
    1e-5 ||W1_i||_1 max |f| (float64 only means anything), and the samples that lie clearly outside every plane's bilinear
    support."""
    if (far, dtype) not in _H1_REF:
        cache, sw, fw, ro, rd, ts, te = [t.to(dtype) if torch.is_tensor(t) else [w.to(dtype) for w in t]
                                         for t in scene(far=far)[:7]]
        n_rays = P * HH * WW
        tm = ((ts + te) / 2.0).reshape(n_rays, S, 1)
        pos = ro.reshape(n_rays, 1, 3) + rd.reshape(n_rays, 1, 3) * tm
        geo = O.geometry_forward(pos.reshape(P, HH * WW * S, 3), cache, sw, fw, output_normal=False)
        f = geo["enc_geo"]  # (n, 32)
        z = f @ sw[0].T
        thr = 1e-5 * sw[0].abs().sum(dim=1)[None, :] * f.abs().max(dim=1, keepdim=True).values
        # a plane has no in-bounds texel once one of its two coordinates is beyond the bilinear support; every plane is out
        # when two of the three coordinates are (radius 1: plane coordinates = positions)
        outside = pos.reshape(-1, 3).abs().sort(dim=1).values[:, 1] > 1.0 + 2.0 / R
        assert (f[outside] == 0).all()
        _H1_REF[(far, dtype)] = (z, thr, outside)
    return _H1_REF[(far, dtype)]
