"""Test-only torch restatement of one training forward of `generative-space-mesh-rasterize-renderer`, written from the
reference's own step (custom/triplaneturbo/models/renderers/generative_space_mesh_rasterize_renderer.py:110-514 and the
marching-cubes helper, triplaneturbo_executable/utils/mesh_exporter.py:29-75) on the test side's existing pieces:

    field          oracle.cpu_ref.geometry_forward + vanilla_mlp (the deformation head) on the helper's grid in [-1, 1]
    shrink         s * x + (1 - s) * x.detach(), the deformation with sdf_grad_shrink too (reference :455-465)
    marching cubes topology from mc_reference.marching_cubes on GIVEN float32 fields (the discrete inside / outside
                   decisions are frozen by the caller: the HIP fields on the GPU, the float32 oracle's on the CPU);
                   vertex positions from mc_reference.vertex_positions_torch on the oracle's own fields.  The helper
                   passes the deformation to the kernel as it is (grid-cell units, mesh_exporter.py:69-73) and maps the
                   [0, 1] vertices through its points_range; isosurface() maps them on to [-1, 1].
    normals        mesh_reference.vertex_normals_torch
    raster         [v, 1] @ mvp^T, raster_reference.rasterize / interpolate / antialias (antialias on the detached rast)
    shading        everything between the G-buffer and the output dictionary, restated below

It runs on the CPU in float32 and in float64 (raster_reference computes in float64 whatever it is given; its inputs
and outputs are rounded to the working dtype here).  One deliberate difference from the reference: the hashgrid
background gets the prompt's own row of text_embed (the reference hands it every prompt's rows, :386-390, which its
per-view repeat only accepts for one prompt); triplaneturbo_amd.mesh_renderer documents the same choice.

The scene (scene()) is the one tests/test_mesh_renderer_oracle.py and tests/test_gpu_mesh_renderer_oracle.py share."""
import json
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

import mc_reference as M
import mesh_reference as MR
import raster_reference as R
from oracle import cpu_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, N_VIEW, H, W, RES, PLANE = 2, 2, 40, 48, 24, 32
B = P * N_VIEW
FOVY = 60.0
SDF_GRAD_SHRINK, DEF_GRAD_SHRINK = 0.3, 0.7  # different, and neither 0 nor 1: the blend factors can be told apart
SEED = 3
IMAGE_KEYS = ("opacity", "depth", "disparity", "comp_normal", "comp_normal_cam_vis", "comp_normal_cam_vis_white",
              "comp_rgb", "comp_rgb_bg")
CHANNELS = {"opacity": 1, "depth": 1, "disparity": 1, "comp_normal": 3, "comp_normal_cam_vis": 3,
            "comp_normal_cam_vis_white": 3, "comp_rgb": 3, "comp_rgb_bg": 3}
GEO_NAMES = ["space_cache", "sdf.w1", "sdf.w2", "sdf.w3", "feat.v1", "feat.v2", "feat.v3", "def.d1", "def.d2", "def.d3"]
BG_NAMES = ["bg.table", "bg.W0", "bg.ln_w", "bg.ln_b", "bg.W1", "bg.b1"]
# state-dict keys of the background module, in the order of BG_NAMES
BG_KEYS = ["encoding.encoding.encoding.params", "hypernet.layers.0.weight", "hypernet.layers.1.weight",
           "hypernet.layers.1.bias", "hypernet.layers.3.weight", "hypernet.layers.3.bias"]


def configs():
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    return s, t


def perspective(fovy_deg, aspect, near=0.1, far=1000.0):
    """threestudio get_projection_matrix (utils/ops.py): [1,1] negated"""
    t = math.tan(math.radians(fovy_deg) / 2)
    m = torch.zeros(4, 4)
    m[0, 0], m[1, 1] = 1 / (t * aspect), -1 / t
    m[2, 2], m[2, 3], m[3, 2] = -(far + near) / (far - near), -2 * far * near / (far - near), -1
    return m


_SCENE = None


def scene():
    """2 prompts x 2 views at 40 x 48 (not square), 32 x 32 planes, a 24^3 deformable grid.  Seeded random planes
    (std 0.3) and nn.Linear-initialised MLPs: the sphere bias keeps each prompt's surface closed and near radius 0.5;
    the deformation head's last layer is scaled so that the deformation is a visible fraction of a cell (measured in
    tests/test_mesh_renderer_oracle.py).  The four cameras stand 90 degrees apart from azimuth 20, so no view is a
    mirror image of another and a shifted view slice shows.  All float32 on the CPU; never modified."""
    global _SCENE
    if _SCENE is not None:
        return _SCENE
    g = torch.Generator().manual_seed(SEED)
    sc = SimpleNamespace()
    sc.cache = torch.randn(P, 6, 32, PLANE, PLANE, generator=g) * 0.3
    sc.sdf_w = O.init_mlp_weights([32, 64, 64, 1], g)
    sc.feat_w = O.init_mlp_weights([96, 64, 64, 3], g)
    sc.def_w = O.init_mlp_weights([32, 64, 64, 3], g)
    sc.def_w[2] = sc.def_w[2] * 4.0
    sc.text = torch.randn(P, 1024, generator=g)
    _, total = O.hashgrid_levels()
    sc.bg = [torch.randn(total * 2, generator=g) * 0.5,                       # table
             torch.randn(64, 1024, generator=g) * math.sqrt(2.0 / (64 + 1024)),  # hypernet.layers.0.weight
             1.0 + 0.1 * torch.randn(64, generator=g), 0.1 * torch.randn(64, generator=g),  # LayerNorm
             torch.randn(16 * 64 + 64 * 3, 64, generator=g) * 0.2, 0.05 * torch.randn(16 * 64 + 64 * 3, generator=g)]
    _, rays_d, c2w, dist = O.make_cameras(B, H, W, fovy_deg=FOVY, azimuth_start_deg=20.0)
    sc.c2w, sc.camera_distances, sc.rays_d = c2w, dist, rays_d
    sc.mvp = perspective(FOVY, W / H)[None] @ torch.inverse(c2w)
    sc.camera_positions = c2w[:, :3, 3].contiguous()
    sc.proj = {k: torch.randn(B, H, W, c, generator=g) for k, c in CHANNELS.items()}
    sc.w_lin = torch.randn(B, H, W, generator=g)
    sc.w_eik = torch.rand(B, H, W, generator=g)
    _SCENE = sc
    return sc


def grid_points(dtype):
    """DiffMarchingCubeHelper.grid_vertices (points_range (0, 1)) mapped to the [-1, 1] box (reference :443-447)"""
    x = torch.linspace(0, 1, RES, dtype=dtype)
    verts = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), dim=-1).reshape(-1, 3)
    return O.scale_tensor(verts, (0, 1), (-1, 1))


def leaves(sc, dtype, background):
    """name -> leaf tensor (requires grad) of everything a training step differentiates"""
    vals = [sc.cache] + sc.sdf_w + sc.feat_w + sc.def_w
    names = list(GEO_NAMES)
    if background == "hashgrid":
        vals, names = vals + sc.bg, names + BG_NAMES
    return {n: v.detach().to(dtype).clone().requires_grad_(True) for n, v in zip(names, vals)}


def field(lv, dtype):
    """sdf (P, R^3) and deformation (P, R^3, 3) of the grid query, autograd-connected to the leaves"""
    pts = grid_points(dtype)[None].expand(P, -1, -1)
    go = O.geometry_forward(pts, lv["space_cache"], [lv[f"sdf.w{i}"] for i in (1, 2, 3)],
                            [lv[f"feat.v{i}"] for i in (1, 2, 3)], output_normal=False)
    deform = O.vanilla_mlp(go["enc_geo"], [lv[f"def.d{i}"] for i in (1, 2, 3)])
    return go["sdf"].reshape(P, -1), deform.reshape(P, -1, 3)


def topology_fields(sdf, deform):
    """the float32 numpy fields mc_reference.marching_cubes takes its discrete decisions from, one pair per prompt"""
    sdf, deform = sdf.detach().float().cpu().numpy(), deform.detach().float().cpu().numpy()
    return [(sdf[p].reshape(RES, RES, RES), deform[p].reshape(RES, RES, RES, 3)) for p in range(P)]


def _lerp(a, b, w):
    return a + w * (b - a)


def background_hidden(dirs, text_embed, table, hyper):
    """(n_view, H, W, 64): the pre-activations of the background MLP's one ReLU layer, from the pieces
    oracle.cpu_ref.hypernet_background is made of (the hyper-network's first matrix applied to the hash encoding)"""
    W0, ln_w, ln_b, W1, b1 = hyper
    h = F.silu(F.layer_norm(F.linear(text_embed, W0), (W0.shape[0],), ln_w, ln_b))
    m1 = F.linear(h, W1, b1)[:, :16 * 64].reshape(16, 64)
    enc = O.hashgrid_encode(((dirs + 1.0) / 2.0).reshape(-1, 3), table)
    return (enc @ m1).reshape(*dirs.shape[:-1], 64)


def geometry_hidden(geo, sdf_w, feat_w):
    """(N, 256): the pre-activations h of the two ReLU layers of the sdf net and of the feature net at the decoded
    points, each as a fraction of its scale sum_k |w_k x_k| (the measure parity.kink_free_rays uses)"""
    pre = []
    for x, ws in ((geo["enc_geo"], sdf_w), (geo["enc_tex"], feat_w)):
        for w in ws[:-1]:
            h = x @ w.T
            pre.append(h / (x.abs() @ w.abs().T).clamp_min(1e-300))
            x = torch.relu(h)
    return torch.cat(pre, dim=-1)


def restate(sc, dtype, topo, normal_direction="camera", enable_bg_rays=True, background="hashgrid",
            sdf_grad_shrink=SDF_GRAD_SHRINK, def_grad_shrink=DEF_GRAD_SHRINK):
    """One training forward.  Returns a namespace: out (the renderer's output dictionary: images (B,H,W,C), "sdf" and
    "sdf_grad" per prompt), leaves, ids (B,H,W) int64 triangle ids + 1, ambiguous (B,H,W) bool, covered (B,H,W) bool
    (the mask the per-point decode selects with), meshes [(v_pos, t_pos_idx)] and bg_hidden (B,H,W,64), the
    pre-activations of the hashgrid background's ReLU layer (None for the solid background), and geo_hidden
    (B,H,W,256), those of the sdf and feature nets at the decoded pixels as fractions of their scale (inf elsewhere)."""
    lv = leaves(sc, dtype, background)
    sdf_w = [lv[f"sdf.w{i}"] for i in (1, 2, 3)]
    feat_w = [lv[f"feat.v{i}"] for i in (1, 2, 3)]
    cast = lambda t: t.to(dtype)  # noqa: E731
    mvp, c2w, cam_pos, cam_dist, rays_d = (cast(t) for t in (sc.mvp, sc.c2w, sc.camera_positions, sc.camera_distances,
                                                              sc.rays_d))
    sdf, deform = field(lv, dtype)
    # reference :455-465 (the deformation is blended with sdf_grad_shrink; def_grad_shrink only switches it off)
    sdf = sdf_grad_shrink * sdf + (1 - sdf_grad_shrink) * sdf.detach() if sdf_grad_shrink != 0 else sdf.detach()
    deform = sdf_grad_shrink * deform + (1 - sdf_grad_shrink) * deform.detach() if def_grad_shrink != 0 \
        else deform.detach()

    outs, ids_all, amb_all, cov_all, meshes, bg_pre, geo_pre = [], [], [], [], [], [], []
    for p in range(P):
        sl = slice(p * N_VIEW, (p + 1) * N_VIEW)
        mc = M.marching_cubes(topo[p][0], topo[p][1], 0.0)
        v01 = M.vertex_positions_torch(mc, sdf[p].reshape(RES, RES, RES), deform[p].reshape(RES, RES, RES, 3), 0.0)
        v_pos = O.scale_tensor(v01 * (1 - 0) + 0, (0, 1), (-1, 1))  # helper :73, then isosurface() to [-1, 1]
        tri = torch.from_numpy(mc.t_pos_idx.astype(np.int64))
        v_nrm = MR.vertex_normals_torch(v_pos, tri)
        meshes.append((v_pos, tri))

        pos_clip = torch.cat([v_pos, torch.ones_like(v_pos[:, :1])], -1) @ mvp[sl].transpose(1, 2)  # (n_view,V,4)
        rast, amb = R.rasterize(pos_clip, tri, H, W)
        rast = cast(rast)
        rast_vis = rast.detach()
        depth = cast(R.interpolate(pos_clip, rast, tri))[..., -2:-1]  # clip z (reference :153-154)
        mask = rast_vis[..., 3:] > 0
        if mask.sum() == 0:  # reference :170-172
            mask[:1] = True
        maskf = cast(mask)
        ids_all.append(rast_vis[..., 3].round().long())
        amb_all.append(amb)
        cov_all.append(mask[..., 0])

        pre_aa = {"opacity": maskf}  # what the reference sends through antialias, by output key
        out = {"depth": depth}
        sqrt3 = math.sqrt(3.0)
        far = (cam_dist + sqrt3)[sl, None, None, None]
        near = (cam_dist - sqrt3)[sl, None, None, None]
        disparity = ((far - torch.minimum(depth, far)) / (far - near)).clamp(0, 1)
        pre_aa["disparity"] = _lerp(torch.zeros_like(depth), disparity, maskf)

        gb_normal = F.normalize(cast(R.interpolate(v_nrm[None], rast, tri)), dim=-1)
        pre_aa["comp_normal"] = _lerp(torch.zeros_like(gb_normal), (gb_normal + 1.0) / 2.0, maskf)
        if normal_direction == "camera":
            rotate = torch.inverse(c2w[sl])[:, :3, :3]
            n_cam = torch.einsum("bhwj,bij->bhwi", gb_normal, rotate)  # row vector times rotate^T
            n_cam = n_cam * torch.tensor([-1.0, 1.0, 1.0], dtype=dtype)  # flip_x
            n_cam = (F.normalize(n_cam, dim=-1) + 1.0) / 2.0
            bg_normal = torch.tensor([0.5, 0.5, 1.0], dtype=dtype).expand_as(gb_normal)
            pre_aa["comp_normal_cam_vis"] = _lerp(bg_normal, n_cam, maskf)
            pre_aa["comp_normal_cam_vis_white"] = _lerp(torch.ones_like(gb_normal), n_cam, maskf)
        elif normal_direction == "front":
            rotate = torch.inverse(c2w[p * N_VIEW])[:3, :3]  # the prompt's first view, for all of its views
            n_cam = torch.einsum("bhwj,ij->bhwi", gb_normal, rotate)
            n_cam = (F.normalize(n_cam, dim=-1) + 1.0) / 2.0
            pre_aa["comp_normal_cam_vis_white"] = _lerp(torch.ones_like(gb_normal), n_cam, maskf)
        else:
            assert normal_direction == "world"

        selector = mask[..., 0]
        gb_pos = cast(R.interpolate(v_pos[None], rast, tri))
        gb_viewdirs = F.normalize(gb_pos - cam_pos[sl, None, None, :], dim=-1)
        positions = gb_pos[selector]  # stays in the graph: d / d points and the second order through sdf_grad
        geo = O.geometry_forward(positions[None], lv["space_cache"][p:p + 1], sdf_w, feat_w, output_normal=True,
                                 create_graph=True)
        out["sdf"], out["sdf_grad"] = geo["sdf"], geo["sdf_grad"]
        with torch.no_grad():  # uncovered pixels decode nothing: infinitely far from every kink
            geo_pre.append(torch.full((N_VIEW, H, W, 256), float("inf"), dtype=dtype).index_put(
                (selector,), geometry_hidden(geo, sdf_w, feat_w)))
        rgb_fg = O.sigmoid_mipnerf(geo["features"])  # no-material (the interpolated shading normal is not used by it)
        gb_rgb_fg = torch.zeros(N_VIEW, H, W, 3, dtype=dtype).index_put((selector,), rgb_fg)
        dirs = rays_d[sl] if enable_bg_rays else gb_viewdirs
        if background == "hashgrid":
            gb_rgb_bg = O.hypernet_background(dirs, cast(sc.text)[p:p + 1], lv["bg.table"],
                                              [lv[n] for n in BG_NAMES[1:]], color_activation="sigmoid-mipnerf")
            with torch.no_grad():
                bg_pre.append(background_hidden(dirs, cast(sc.text)[p:p + 1], lv["bg.table"],
                                                [lv[n] for n in BG_NAMES[1:]]))
        else:
            gb_rgb_bg = torch.ones(3, dtype=dtype).expand(N_VIEW, H, W, 3)  # solid-color-background, white
        pre_aa["comp_rgb"] = _lerp(gb_rgb_bg, gb_rgb_fg, maskf)
        out["comp_rgb_bg"] = gb_rgb_bg

        # antialias acts on every channel alike: one call on the channels of all keys is the reference's call per key
        keys = list(pre_aa)
        aa = cast(R.antialias(torch.cat([pre_aa[k] for k in keys], -1), rast_vis, pos_clip, tri))
        for k, img in zip(keys, torch.split(aa, [pre_aa[k].shape[-1] for k in keys], dim=-1)):
            out[k] = img
        outs.append(out)

    merged = {}
    for k in outs[0]:
        vals = [o[k] for o in outs]
        merged[k] = vals if k in ("sdf", "sdf_grad") else torch.cat(vals, 0)
    return SimpleNamespace(out=merged, leaves=lv, ids=torch.cat(ids_all), ambiguous=torch.cat(amb_all),
                           covered=torch.cat(cov_all), meshes=meshes, bg_hidden=torch.cat(bg_pre) if bg_pre else None,
                           geo_hidden=torch.cat(geo_pre))


def dilate(amb):
    """ambiguous pixels and their 4-neighbours (antialias pairs reach one pixel across)"""
    a = amb.clone()
    a[:, 1:] |= amb[:, :-1]
    a[:, :-1] |= amb[:, 1:]
    a[:, :, 1:] |= amb[:, :, :-1]
    a[:, :, :-1] |= amb[:, :, 1:]
    return a


KINK_SLACK = 4.0  # parity.check_outputs' factor on the float32 restatement's own error


def keep_mask(r64, r32):
    """(B,H,W) bool, the pixels that carry loss weight, and the measured kink margins {"background", "geometry"}.
    Two kinds of discrete decision are frozen by leaving pixels out instead of widening a tolerance:
      * visibility: the pixels raster_reference.rasterize reports as ambiguous, dilated twice (an antialias pair
        reaches one pixel across, and the pair's partner must be certain too);
      * ReLU kinks of the per-pixel networks: the sdf and feature nets at the decoded pixels and the hashgrid
        background's MLP at every pixel.  A gradient jumps where a hidden pre-activation crosses zero, and one sample on
        the other side moves a whole gradient by 1e-3 of its norm (parity.kink_free_rays has the volume renderer's
        case; the float32 restatement itself lands on the other side of such a kink on some CPUs).  The background
        is the worst: its input is a hash encoding whose finest level multiplies the float32 rounding of a direction
        by 256 cells.  A pixel is kept when every unit's float64 pre-activation is farther from zero than KINK_SLACK
        times the largest distance of the float32 restatement's pre-activations (which are continuous across a kink)
        from the float64 ones on this scene, dilated once: antialias blends a pixel's colour into its neighbour."""
    keep = ~dilate(dilate(r64.ambiguous))
    margins = {}
    for name, h64, h32 in (("background", r64.bg_hidden, r32.bg_hidden), ("geometry", r64.geo_hidden, r32.geo_hidden)):
        if h64 is None:
            continue
        both = torch.isfinite(h64) & torch.isfinite(h32)
        margins[name] = KINK_SLACK * float((h32.double() - h64)[both].abs().max())
        keep &= ~dilate((h64.abs() <= margins[name]).any(-1))
    return keep, margins


def loss(out, sc, keep, covered, keys=IMAGE_KEYS, point_terms=True):
    """A fixed random projection of every image output in `keys` that the run has, plus per-point terms on out["sdf"]
    (linear) and out["sdf_grad"] (eikonal).  The per-point weights are (B,H,W) images gathered at the run's own covered
    pixels, so two runs whose masks differ on excluded pixels still weigh the same points; every weight is zero
    outside `keep`."""
    total = 0.0
    for k in keys:
        if k in out:
            total = total + (out[k] * (sc.proj[k] * keep[..., None]).to(out[k])).sum()
    if point_terms:
        for p in range(P):
            sl = slice(p * N_VIEW, (p + 1) * N_VIEW)
            sel = covered[sl].cpu()
            sdf, sdf_grad = out["sdf"][p], out["sdf_grad"][p]
            w_lin = (sc.w_lin * keep)[sl][sel].to(sdf)
            w_eik = (sc.w_eik * keep)[sl][sel].to(sdf)
            total = total + (w_lin * sdf[:, 0]).sum() + (w_eik * (sdf_grad.norm(dim=-1) - 1.0) ** 2).sum()
    return total


def gradients(run, sc, keep, keys=IMAGE_KEYS, point_terms=True, retain_graph=False):
    """(loss value, name -> d loss / d leaf) of a restate() run; leaves the loss does not reach are left out"""
    names = list(run.leaves)
    val = loss(run.out, sc, keep, run.covered, keys, point_terms)
    grads = torch.autograd.grad(val, [run.leaves[n] for n in names], allow_unused=True, retain_graph=retain_graph)
    return float(val.detach()), {n: g.detach() for n, g in zip(names, grads) if g is not None}
