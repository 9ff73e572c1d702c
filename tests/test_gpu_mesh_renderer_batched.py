"""`generative-space-mesh-rasterize-renderer` with `batch_prompts = True`: all prompts of a training step through one
set of range-mode raster launches.  Against the default per-prompt loop on identical inputs the images are the same
bits, the gradients agree within the loop's own run-to-run spread, and the launch counts are 1 against one per prompt.

Shape: 2 prompts x 2 views, 32x32 images, seeded random planes (std 0.3) on the training config's geometry, and
isosurface_resolution = 16: the sphere bias of the field gives both prompts a surface at that resolution (asserted
below)."""
import json
import math
import os

import pytest
import torch

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOVY = 60.0
P, N_VIEW, H, W, RES = 2, 2, 32, 32, 16
IMAGE_KEYS = ("opacity", "depth", "disparity", "comp_normal", "comp_normal_cam_vis", "comp_normal_cam_vis_white",
              "comp_rgb", "comp_rgb_bg")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def perspective(fovy_deg, aspect, near=0.1, far=1000.0):
    t = math.tan(math.radians(fovy_deg) / 2)
    M = torch.zeros(4, 4)
    M[0, 0], M[1, 1] = 1 / (t * aspect), -1 / t
    M[2, 2], M[2, 3], M[3, 2] = -(far + near) / (far - near), -2 * far * near / (far - near), -1
    return M


def _cameras(n_view, dev):
    rays_o, rays_d, c2w, dist = synthetic.make_cameras(n_view, H, W, fovy_deg=FOVY)
    mvp = perspective(FOVY, W / H)[None] @ torch.inverse(c2w)
    pos = c2w[:, :3, 3]
    return {k: v.to(dev) for k, v in dict(mvp_mtx=mvp, camera_positions=pos, light_positions=pos, c2w=c2w,
                                           camera_distances=dist).items()}


def _modules(dev, **rend_over):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(t["geometry"]).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    cfg = dict(s["renderer"], enable_bg_rays=False, isosurface_resolution=RES, **rend_over)
    r = tt.find(s["renderer_type"])(cfg, geometry=g, material=m, background=b).to(dev)
    r.train()
    r.update_step(0, 100)
    return r, g


def _inputs(dev):
    cam = _cameras(P * N_VIEW, dev)
    cache = (torch.randn(P, 6, 32, 32, 32, device=dev, generator=torch.Generator(dev).manual_seed(1)) * 0.3)
    return cam, cache, torch.zeros(P, 1024, device=dev)


def _render(r, cam, cache, text, batch_prompts):
    r.batch_prompts = batch_prompts
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        out = r(cam["mvp_mtx"], cam["camera_positions"], cam["light_positions"], H, W, space_cache=cache,
                text_embed=text, camera_distances=cam["camera_distances"], c2w=cam["c2w"])
    finally:
        ops.set_kernel_timer(None)
        r.batch_prompts = False
    labels = [e[0] for e in timer.events]
    return out, labels.count("tt_rast_fwd"), labels.count("tt_rast_range_fwd")


def _assert_same_outputs(a, b):
    assert list(a.keys()) == list(b.keys())
    for k in a:
        if k == "mesh":
            for x, y in zip(a[k], b[k]):
                assert torch.equal(x.v_pos, y.v_pos) and torch.equal(x.t_pos_idx, y.t_pos_idx)
        elif k in ("sdf", "sdf_grad"):
            assert len(a[k]) == len(b[k]) == P
            for x, y in zip(a[k], b[k]):
                assert torch.equal(x, y), k
        else:
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
            assert a[k].requires_grad == b[k].requires_grad, k
            assert torch.equal(a[k], b[k]), (k, (a[k].float() - b[k].float()).abs().max())
    for k in IMAGE_KEYS:
        assert k in a and a[k].shape[:3] == (P * N_VIEW, H, W), k


def test_forward_is_bitwise_the_loop_and_launches_once(dev):
    r, _ = _modules(dev)
    cam, cache, text = _inputs(dev)
    with torch.no_grad():
        loop, n_inst, n_range = _render(r, cam, cache, text, False)
        assert (n_inst, n_range) == (P, 0)  # the default: one instance-mode rasterize per prompt
        both, n_inst, n_range = _render(r, cam, cache, text, True)
        assert (n_inst, n_range) == (0, 1)  # one range-mode rasterize for the step
    assert all(m.t_pos_idx.shape[0] > 0 for m in loop["mesh"])
    assert (loop["opacity"].flatten(1).sum(1) > 0).all()  # every view shows its mesh
    _assert_same_outputs(loop, both)
    r.eval()  # eval keeps the loop
    with torch.no_grad():
        _, n_inst, n_range = _render(r, cam, cache, text, True)
    assert (n_inst, n_range) == (P, 0)


def test_an_empty_prompt_inside_the_batch(dev):
    """prompt 1's field is all positive: the InstantMesh fix-up and the empty_flag detaches run inside the batch"""
    r, g = _modules(dev, allow_empty_flag=True)
    cam, cache, text = _inputs(dev)
    field = g.forward_field

    def one_empty(points, space_cache):
        sdf, deformation = field(points, space_cache)
        lift = torch.zeros(sdf.shape[0], *([1] * (sdf.dim() - 1)), device=sdf.device)
        lift[1] = 10.0
        return sdf + lift, deformation

    g.forward_field = one_empty
    cache.requires_grad_(True)
    loop, _, _ = _render(r, cam, cache, text, False)
    assert not r.empty_flag
    both, n_inst, n_range = _render(r, cam, cache, text, True)
    assert not r.empty_flag and (n_inst, n_range) == (0, 1)
    assert all(m.t_pos_idx.shape[0] > 0 for m in both["mesh"])
    assert not both["comp_rgb"].requires_grad and both["opacity"].dtype == torch.bool
    _assert_same_outputs(loop, both)


def _gradients(r, g, cam, cache, text, batch_prompts):
    params = {"space_cache": cache}
    for net in ("sdf_network", "feature_network", "deformation_network"):
        for i, w in enumerate(getattr(g, net).parameters()):
            params[f"{net}.{i}"] = w
    for p in params.values():
        p.grad = None
    out, _, _ = _render(r, cam, cache, text, batch_prompts)
    gen = torch.Generator().manual_seed(3)
    loss = sum((out[k] * torch.randn(out[k].shape, generator=gen).to(out[k].device)).sum()
               for k in ("comp_rgb", "opacity", "comp_normal_cam_vis", "disparity"))
    loss.backward()
    return {k: p.grad.detach().double().clone() for k, p in params.items() if p.grad is not None}


def test_backward_is_within_the_loops_own_spread(dev):
    """Both paths sum their vertex gradients with fp32 atomics.  d0 = relative L2 difference of two runs of the loop
    (its run-to-run spread), per gradient tensor; the batched path must be within 10 max(d0, 1e-7) of the loop (1e-7:
    one fp32 ulp; 10: another summation order over at most 4 views)."""
    r, g = _modules(dev)
    cam, cache, text = _inputs(dev)
    cache.requires_grad_(True)
    loop_a = _gradients(r, g, cam, cache, text, False)
    loop_b = _gradients(r, g, cam, cache, text, False)
    both = _gradients(r, g, cam, cache, text, True)
    assert set(both) == set(loop_a) and "space_cache" in loop_a and len(loop_a) >= 4
    failed = []
    for k, ref in loop_a.items():
        assert ref.norm() > 0, k
        d0 = float((loop_b[k] - ref).norm() / ref.norm())
        d = float((both[k] - ref).norm() / ref.norm())
        print(f"grad {k}: loop-vs-loop d0 = {d0:.3e}, batched-vs-loop = {d:.3e}, bar = {10 * max(d0, 1e-7):.3e}")
        if not d <= 10 * max(d0, 1e-7):
            failed.append((k, d0, d))
    assert not failed, failed
