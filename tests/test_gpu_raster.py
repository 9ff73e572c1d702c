"""HIP rasterize / interpolate / antialias (tt_raster.hip, triplaneturbo_amd.raster) against the float64 oracle of the
contract (tests/raster_reference.py): visibility and (u, v, z/w) on random soups, an MC sphere, clipped, off-screen,
degenerate and empty scenes; bit-repeatable launches; a crack-free MC silhouette; gradients of every op and of an
end-to-end antialias(interpolate(...)) loss against oracle autograd."""
import math
import os
import sys

import pytest
import torch

from triplaneturbo_amd import ops, raster, synthetic

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raster_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu
F64 = torch.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def perspective(fovy_deg, aspect, near=0.1, far=1000.0):
    """threestudio get_projection_matrix (utils/ops.py): [1,1] negated"""
    t = math.tan(math.radians(fovy_deg) / 2)
    P = torch.zeros(4, 4)
    P[0, 0] = 1 / (t * aspect)
    P[1, 1] = -1 / t
    P[2, 2] = -(far + near) / (far - near)
    P[2, 3] = -2 * far * near / (far - near)
    P[3, 2] = -1
    return P


def mvp_for(n_view, H, W, fovy=60.0, **kw):
    _, _, c2w, dist = synthetic.make_cameras(n_view, H, W, fovy_deg=fovy, **kw)
    return perspective(fovy, W / H)[None] @ torch.inverse(c2w), c2w, dist


def clip(v, mvp):
    return torch.cat([v, torch.ones(v.shape[0], 1, dtype=v.dtype)], -1) @ mvp.transpose(1, 2).to(v.dtype)


def mc_sphere(dev, R=64, radius=0.5):
    x = torch.linspace(-1, 1, R, device=dev)
    g = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), -1)
    v, t = ops.marching_cubes(g.norm(dim=-1) - radius)
    return (v * 2 - 1).cpu(), t.cpu()


def soup(seed, B=3, T=60, V=90):
    g = torch.Generator().manual_seed(seed)
    pos = torch.rand(B, V, 4, generator=g) * 2.4 - 1.2
    pos[..., 3] = 0.6 + torch.rand(B, V, generator=g)
    pos[..., :3] *= pos[..., 3:4]
    tri = torch.randint(0, V, (T, 3), generator=g, dtype=torch.int32)
    return pos, tri


def scenes():
    out = {}
    out["soup"] = soup(0) + (48, 40)
    out["soup_big"] = soup(1, B=2, T=400, V=300) + (64, 64)
    v, t = mc_sphere("cuda")
    mvp, _, _ = mvp_for(3, 64, 64)
    out["mc_sphere"] = (clip(v, mvp).float(), t, 64, 64)
    # crossing w = 0 and the far plane, off-screen, degenerate (repeated index, collinear, zero w area), T = 0
    pos = torch.tensor([[[-0.5, -0.5, 0.0, 1.0], [0.5, -0.4, 0.2, -0.6], [0.0, 0.7, 0.1, 0.8],  # straddles w = 0
                         [-0.9, 0.2, 0.5, 1.0], [0.9, 0.3, 2.5, 1.0], [0.1, 0.9, 0.4, 1.0],  # crosses z/w = 1
                         [3.0, 3.0, 0.0, 1.0], [4.0, 3.0, 0.0, 1.0], [3.5, 4.0, 0.0, 1.0],  # off-screen
                         [-0.3, -0.3, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0], [0.3, 0.3, 0.0, 1.0],  # collinear
                         [0.2, -0.8, -0.3, 1.0], [0.8, -0.2, -1.6, 1.0], [0.6, -0.9, 0.3, 1.0]]])  # near plane
    pos = torch.cat([pos, pos * torch.tensor([1.3, 1.1, 1.0, 1.2])])
    # off the pixel lattice: round NDC values put vertices exactly on scanlines and pair midpoints, where float32 and
    # float64 legitimately disagree about a crossing
    pos[..., :2] += 1e-3 * torch.sin(torch.arange(pos[..., :2].numel(), dtype=torch.float32) * 1.7).reshape(2, -1, 2)
    tri = torch.tensor([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11], [0, 0, 2], [12, 13, 14]], dtype=torch.int32)
    out["clipped"] = (pos, tri, 40, 56)
    out["empty"] = (pos, torch.zeros(0, 3, dtype=torch.int32), 16, 24)
    return out


def _dilate(amb):
    """ambiguous pixels and their 4-neighbours (antialias pairs reach one pixel across)"""
    a = amb.clone()
    a[:, 1:] |= amb[:, :-1]
    a[:, :-1] |= amb[:, 1:]
    a[:, :, 1:] |= amb[:, :, :-1]
    a[:, :, :-1] |= amb[:, :, 1:]
    return a


def _check_rast(rast, ref, amb):
    rast = rast.cpu().double()
    ok = ~amb
    assert amb.float().mean() < 1e-3, amb.float().mean()
    assert torch.equal(rast[..., 3][ok], ref[..., 3][ok].detach()), (rast[..., 3][ok] != ref[..., 3][ok]).sum()
    assert (rast[..., :3][ok] - ref[..., :3][ok].detach()).abs().max() <= 1e-5


@pytest.mark.parametrize("name", ["soup", "soup_big", "mc_sphere", "clipped", "empty"])
def test_rasterize_matches_oracle_and_repeats_bitwise(dev, name):
    pos, tri, H, W = scenes()[name]
    rast = raster.rasterize(pos.to(dev), tri.to(dev), (H, W))
    ref, amb = R.rasterize(pos.double(), tri, H, W)
    _check_rast(rast, ref, amb)
    if name in ("soup", "soup_big", "mc_sphere"):
        assert (rast[..., 3] > 0).float().mean() > 0.05
    if name == "empty":
        assert rast.abs().max() == 0
    again = raster.rasterize(pos.to(dev), tri.to(dev), (H, W))
    assert torch.equal(rast, again)  # bit-identical
    c = torch.rand(pos.shape[0], H, W, 3, device=dev)
    a1 = raster.antialias(c, rast, pos.to(dev), tri.to(dev))
    a2 = raster.antialias(c, rast, pos.to(dev), tri.to(dev))
    assert torch.equal(a1, a2)


def test_mc_sphere_silhouette_has_no_cracks(dev):
    H = W = 128
    v, t = mc_sphere(dev)
    mvp, c2w, dist = mvp_for(4, H, W)
    pos = clip(v, mvp).float().to(dev)
    rast = raster.rasterize(pos, t.to(dev), (H, W)).cpu()
    fov = math.radians(60.0)
    for b in range(4):
        # the sphere's projected disc: angular radius asin(r / d) around the image centre
        rad = math.tan(math.asin(0.5 / float(dist[b]))) / math.tan(fov / 2) * H / 2
        yy, xx = torch.meshgrid(torch.arange(H) + 0.5 - H / 2, torch.arange(W) + 0.5 - W / 2, indexing="ij")
        inner = (yy ** 2 + xx ** 2).sqrt() < rad - 1.0
        ids = rast[b, ..., 3]
        assert (ids[inner] > 0).all(), (~(ids[inner] > 0)).sum()
        # and what shows there is the front surface: one orientation sign (a crack would show a back face)
        o = R.orientation(pos[b:b + 1].cpu(), t)[0]
        signs = o[(ids[inner].long() - 1)]
        assert (signs == signs[0]).all() and signs[0] != 0


def test_interpolate_backward_matches_oracle(dev):
    pos, tri, H, W = scenes()["soup_big"]
    rast = raster.rasterize(pos.to(dev), tri.to(dev), (H, W))
    g = torch.Generator().manual_seed(7)
    for A in (pos.shape[0], 1):
        attr = torch.randn(A, pos.shape[1], 5, generator=g)
        wts = torch.randn(pos.shape[0], H, W, 5, generator=g)
        a = attr.to(dev).requires_grad_(True)
        r = rast.detach().clone().requires_grad_(True)
        out = raster.interpolate(a, r, tri.to(dev))
        (out * wts.to(dev)).sum().backward()
        a64 = attr.double().requires_grad_(True)
        r64 = rast.detach().cpu().double().requires_grad_(True)
        ref = R.interpolate(a64, r64, tri)
        (ref * wts.double()).sum().backward()
        assert (out.detach().cpu().double() - ref.detach()).abs().max() < 1e-5
        assert (a.grad.cpu().double() - a64.grad).norm() <= 1e-4 * a64.grad.norm()
        assert (r.grad.cpu().double()[..., :2] - r64.grad[..., :2]).norm() <= 1e-4 * r64.grad[..., :2].norm()
        assert r.grad[..., 2:].abs().max() == 0


@pytest.mark.parametrize("name", ["soup_big", "mc_sphere"])
def test_rasterize_backward_matches_oracle(dev, name):
    pos, tri, H, W = scenes()[name]
    ref, amb = R.rasterize(pos.double(), tri, H, W)
    wts = torch.randn(pos.shape[0], H, W, 2, generator=torch.Generator().manual_seed(3)) * (~_dilate(amb))[..., None]
    p = pos.to(dev).requires_grad_(True)
    rast = raster.rasterize(p, tri.to(dev), (H, W))
    (rast[..., :2] * wts.to(dev)).sum().backward()
    p64 = pos.double().requires_grad_(True)
    (R.rasterize(p64, tri, H, W)[0][..., :2] * wts.double()).sum().backward()
    assert (p.grad.cpu().double() - p64.grad).norm() <= 1e-4 * p64.grad.norm()
    assert p.grad[..., 2].abs().max() == 0


@pytest.mark.parametrize("name", ["soup_big", "mc_sphere", "clipped"])
def test_antialias_backward_matches_oracle(dev, name):
    pos, tri, H, W = scenes()[name]
    rast = raster.rasterize(pos.to(dev), tri.to(dev), (H, W)).detach()
    g = torch.Generator().manual_seed(11)
    color = torch.rand(pos.shape[0], H, W, 3, generator=g)
    wts = torch.randn(pos.shape[0], H, W, 3, generator=g)
    c = color.to(dev).requires_grad_(True)
    p = pos.to(dev).requires_grad_(True)
    out = raster.antialias(c, rast, p, tri.to(dev))
    (out * wts.to(dev)).sum().backward()
    c64 = color.double().requires_grad_(True)
    p64 = pos.double().requires_grad_(True)
    ref = R.antialias(c64, rast.cpu().double(), p64, tri)
    (ref * wts.double()).sum().backward()
    assert (out.detach().cpu().double() - ref.detach()).abs().max() < 1e-4
    assert (out.detach().cpu() != color).any()
    assert (c.grad.cpu().double() - c64.grad).norm() <= 1e-4 * c64.grad.norm()
    assert (p.grad.cpu().double() - p64.grad).norm() <= 1e-4 * max(p64.grad.norm(), 1e-12)
    if name != "clipped":
        assert p64.grad.norm() > 0


def test_end_to_end_loss_backward_to_v_pos(dev):
    H = W = 64
    v, t = mc_sphere(dev, R=32)
    mvp, _, _ = mvp_for(2, H, W)
    g = torch.Generator().manual_seed(5)
    col = torch.rand(v.shape[0], 3, generator=g)
    _, amb = R.rasterize(clip(v.double(), mvp.double()), t, H, W)
    keep = ~_dilate(_dilate(amb))  # pixels whose own and neighbours' visibility is certain
    wts = torch.randn(2, H, W, 3, generator=g) * keep[..., None]
    ctx = raster.RasterizerContext("cuda", dev)

    vd = v.to(dev).requires_grad_(True)
    pos = ctx.vertex_transform(vd, mvp.to(dev))
    rast, _ = ctx.rasterize(pos, t.to(dev), (H, W))
    img, _ = ctx.interpolate_one(col.to(dev), rast, t.to(dev))
    out = ctx.antialias(img, rast, pos, t.to(dev))
    (out * wts.to(dev)).sum().backward()

    v64 = v.double().requires_grad_(True)
    pos64 = clip(v64, mvp.double())
    r64, amb = R.rasterize(pos64, t, H, W)
    assert amb.float().mean() < 1e-3
    img64 = R.interpolate(col.double()[None], r64, t)
    out64 = R.antialias(img64, r64.detach(), pos64, t)
    (out64 * wts.double()).sum().backward()
    assert (out.detach().cpu().double() - out64.detach())[keep].abs().max() < 1e-4
    assert (vd.grad.cpu().double() - v64.grad).norm() <= 1e-4 * v64.grad.norm()
