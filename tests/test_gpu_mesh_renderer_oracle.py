"""One training step of `generative-space-mesh-rasterize-renderer` (mesh_renderer.forward / shade / _raster_prompt /
_raster_batched / isosurface, DiffMarchingCubeHelper, Mesh.v_nrm) against the float64 restatement of the reference's
step (tests/mesh_renderer_reference.py): every image output and the gradients of the space cache, the nine MLP
matrices and the background's parameters, on one small scene, for the looped and the batched raster path, the three
normal directions, background rays on and off, and the solid background.

Bars (tests/parity.py, nothing new): outputs within 4x the float32 restatement's own distance from float64 (floor
2e-5); every gradient within 1e-4 of the float32 restatement in relative norm, and as close to float64 as
max(1e-4, 3x the float32 restatement's distance).  Discrete decisions are frozen, not tolerated: the topology comes
from mc_reference on the HIP float32 fields, and pixels of uncertain visibility or on a ReLU kink of a per-pixel
network (sdf, feature, background) carry no loss weight (mesh_renderer_reference.keep_mask); outside the ambiguous
pixels the HIP triangle ids must be the oracle's exactly."""
import time

import pytest
import torch

import mesh_renderer_reference as X
import triplaneturbo_amd as tt
from parity import check_grads, check_outputs, report

pytestmark = pytest.mark.gpu
_ORACLE_CACHE = {}
_TOPOLOGY = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _modules(dev, normal_direction, enable_bg_rays, background):
    sc = X.scene()
    s, t = X.configs()
    g = tt.find(t["geometry_type"])(t["geometry"]).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    if background == "hashgrid":
        b = tt.find(t["background_type"])(t["background"]).to(dev)
        b.load_state_dict(dict(zip(X.BG_KEYS, sc.bg)))
    else:
        b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    with torch.no_grad():
        for net, ws in ((g.sdf_network, sc.sdf_w), (g.feature_network, sc.feat_w), (g.deformation_network, sc.def_w)):
            for dst, src in zip(net.weights(), ws):
                dst.copy_(src)
    cfg = dict(s["renderer"], enable_bg_rays=enable_bg_rays, normal_direction=normal_direction,
               isosurface_resolution=X.RES, sdf_grad_shrink=X.SDF_GRAD_SHRINK, def_grad_shrink=X.DEF_GRAD_SHRINK)
    r = tt.find(s["renderer_type"])(cfg, geometry=g, material=m, background=b).to(dev)
    r.train()
    r.update_step(0, 0)
    params = [g.sdf_network.weights(), g.feature_network.weights(), g.deformation_network.weights()]
    params = [w for ws in params for w in ws]
    if background == "hashgrid":
        named = dict(b.named_parameters())
        params += [named[k] for k in X.BG_KEYS]
    return r, g, params


def _topology(dev):
    """the HIP float32 sdf and deformation on the helper's grid: what the oracle's marching cubes decides from"""
    if "topo" not in _TOPOLOGY:
        sc = X.scene()
        _, g, _ = _modules(dev, "camera", True, "solid")
        with torch.no_grad():
            pts = X.grid_points(torch.float32).to(dev)[None].expand(X.P, -1, -1)
            sdf, deform = g.forward_field(pts, sc.cache.to(dev))
        _TOPOLOGY["topo"] = X.topology_fields(sdf.reshape(X.P, -1), deform.reshape(X.P, -1, 3))
    return _TOPOLOGY["topo"]


def _oracle(dev, normal_direction, enable_bg_rays, background, keys=X.IMAGE_KEYS, point_terms=True):
    """the float32 and float64 restatements of one configuration, computed once"""
    key = (normal_direction, enable_bg_rays, background, keys, point_terms)
    if key not in _ORACLE_CACHE:
        sc = X.scene()
        topo = _topology(dev)
        r64 = X.restate(sc, torch.float64, topo, normal_direction, enable_bg_rays, background)
        r32 = X.restate(sc, torch.float32, topo, normal_direction, enable_bg_rays, background)
        keep, margin = X.keep_mask(r64, r32)
        l64, g64 = X.gradients(r64, sc, keep, keys, point_terms)
        l32, g32 = X.gradients(r32, sc, keep, keys, point_terms)
        _ORACLE_CACHE[key] = (r32, r64, keep, margin, g32, g64)
    return _ORACLE_CACHE[key]


def _hip(dev, normal_direction, enable_bg_rays, background, batch_prompts, keep, keys=X.IMAGE_KEYS, point_terms=True):
    sc = X.scene()
    r, g, params = _modules(dev, normal_direction, enable_bg_rays, background)
    r.batch_prompts = batch_prompts
    cache = sc.cache.to(dev).requires_grad_(True)
    mvp = sc.mvp.to(dev)
    out = r(mvp, sc.camera_positions.to(dev), sc.camera_positions.to(dev), X.H, X.W, space_cache=cache,
            text_embed=sc.text.to(dev), rays_d_rasterize=sc.rays_d.to(dev),
            camera_distances=sc.camera_distances.to(dev), c2w=sc.c2w.to(dev))
    ids = []
    with torch.no_grad():  # the renderer's own rasterize call (bit-repeatable) on its own meshes
        for p, mesh in enumerate(out["mesh"]):
            clip = r.ctx.vertex_transform(mesh.v_pos.detach(), mvp[p * X.N_VIEW:(p + 1) * X.N_VIEW])
            rast, _ = r.ctx.rasterize(clip, mesh.t_pos_idx, (X.H, X.W))
            ids.append(rast[..., 3].round().long().cpu())
    ids = torch.cat(ids)
    val = X.loss(out, sc, keep, ids > 0, keys, point_terms)
    grads = torch.autograd.grad(val, [cache] + params, allow_unused=True)
    return out, ids, [None if x is None else x.detach().cpu() for x in grads]


def _kept_outputs(out, covered, keep):
    """the images on the kept pixels and the per-point outputs of the kept covered pixels, flat"""
    res = {k: out[k].detach().cpu()[keep] for k in X.IMAGE_KEYS if k in out}
    for k in ("sdf", "sdf_grad"):
        rows = []
        for p in range(X.P):
            sl = slice(p * X.N_VIEW, (p + 1) * X.N_VIEW)
            rows.append(out[k][p].detach().cpu()[keep[sl][covered[sl]]])
        res[k] = torch.cat(rows)
    return res


def _check(dev, case, normal_direction, enable_bg_rays, background, batch_prompts):
    t0 = time.time()
    r32, r64, keep, margin, g32, g64 = _oracle(dev, normal_direction, enable_bg_rays, background)
    t1 = time.time()
    out, ids, g_hip = _hip(dev, normal_direction, enable_bg_rays, background, batch_prompts, keep)
    amb = r64.ambiguous
    report(case + " scene", {"ambiguous_fraction": amb.float().mean().item(), "kept_fraction": keep.float().mean().item(),
                             "kink_margins": margin, "oracle_seconds": t1 - t0, "hip_seconds": time.time() - t1})
    assert amb.float().mean() < 1e-3, amb.float().mean()
    for p, mesh in enumerate(out["mesh"]):
        assert torch.equal(mesh.t_pos_idx.cpu().long(), r64.meshes[p][1])
    assert torch.equal(ids[~amb], r64.ids[~amb]), (ids != r64.ids)[~amb].sum()

    want_keys = {"camera": X.IMAGE_KEYS, "front": tuple(k for k in X.IMAGE_KEYS if k != "comp_normal_cam_vis"),
                 "world": tuple(k for k in X.IMAGE_KEYS if "cam_vis" not in k)}[normal_direction]
    assert set(out) == set(want_keys) | {"mesh", "sdf", "sdf_grad"} == set(r64.out) | {"mesh"}
    for k in want_keys:
        assert out[k].shape == (X.B, X.H, X.W, X.CHANNELS[k]), (k, out[k].shape)
    flat = [_kept_outputs(o, c, keep) for o, c in ((out, ids > 0), (r32.out, r32.covered), (r64.out, r64.covered))]
    flat[0]["v_pos"] = torch.cat([m.v_pos.detach().cpu() for m in out["mesh"]])
    flat[1]["v_pos"] = torch.cat([v.detach() for v, _ in r32.meshes])
    flat[2]["v_pos"] = torch.cat([v.detach() for v, _ in r64.meshes])
    check_outputs(case + " outputs", *flat, list(want_keys) + ["sdf", "sdf_grad", "v_pos"])

    names = list(g64)
    assert names == X.GEO_NAMES + (X.BG_NAMES if background == "hashgrid" else [])
    assert all(g is not None for g in g_hip), [n for n, g in zip(names, g_hip) if g is None]
    assert g_hip[0][:, 3:].abs().sum() > 0  # the texture planes, through comp_rgb
    check_grads(case + " gradients", g_hip, [g32[n] for n in names], [g64[n] for n in names], names=names, elem=False)


@pytest.mark.parametrize("enable_bg_rays", [False, True])
@pytest.mark.parametrize("normal_direction", ["camera", "front", "world"])
@pytest.mark.parametrize("batch_prompts", [False, True])
def test_training_step_matches_the_float64_restatement(dev, batch_prompts, normal_direction, enable_bg_rays):
    _check(dev, f"mesh renderer oracle: normal={normal_direction} bg_rays={enable_bg_rays} batched={batch_prompts}",
           normal_direction, enable_bg_rays, "hashgrid", batch_prompts)


@pytest.mark.parametrize("batch_prompts", [False, True])
def test_solid_background_separates_foreground_from_background(dev, batch_prompts):
    _check(dev, f"mesh renderer oracle: solid background batched={batch_prompts}", "camera", False, "solid",
           batch_prompts)


@pytest.mark.parametrize("batch_prompts", [False, True])
def test_opacity_alone_reaches_the_geometry_planes(dev, batch_prompts):
    """A loss on the antialiased opacity only: the silhouette gradient reaches the cache through antialias -> clip
    positions -> marching cubes -> field, and through nothing else."""
    cfg = ("camera", True, "solid")
    r32, r64, keep, _, g32, g64 = _oracle(dev, *cfg, keys=("opacity",), point_terms=False)
    _, _, g_hip = _hip(dev, *cfg, batch_prompts, keep, keys=("opacity",), point_terms=False)
    names = [n for n in X.GEO_NAMES if not n.startswith("feat")]
    # the oracle's opacity does not reach the feature net either: its one antialias call on the channels of all keys
    # hands autograd exact zeros for the other keys' channels, where a call per key would hand it nothing
    assert set(names) <= set(g64) <= set(X.GEO_NAMES)
    for g in (g32, g64):
        assert all(g[n].abs().max() == 0 for n in g if n.startswith("feat"))
        assert g["space_cache"][:, :3].abs().sum() > 0 and g["space_cache"][:, 3:].abs().max() == 0
    got = dict(zip(X.GEO_NAMES, g_hip))
    assert all(got[n] is None or got[n].abs().max() == 0 for n in X.GEO_NAMES if n.startswith("feat"))
    assert got["space_cache"][:, :3].abs().sum() > 0 and got["space_cache"][:, 3:].abs().max() == 0
    check_grads(f"mesh renderer oracle: opacity only batched={batch_prompts}", [got[n] for n in names],
                [g32[n] for n in names], [g64[n] for n in names], names=names, elem=False)
