"""HIP UV atlas, texture bake and fill (tt_uv_*, tt_tex_fill; ops.uv_atlas / texture_fill) and the
`multiprompt-mesh-exporter` end to end: against the numpy restatement (tests/uv_reference.py) on small marching-cubes
meshes, the atlas invariants on every mesh (the bench scene at 1024^2), determinism, the bake against a torch
recomputation, the fill against brute-force nearest distances, and the written OBJ / PNG against colorize_mesh."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops
from triplaneturbo_amd.export import read_png, save_obj
from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, Mesh, colorize_mesh, isosurface

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uv_reference as U  # noqa: E402
from test_isosurface_oracle import sphere, torus, two_spheres  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 0.3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mc_mesh(level, dev):
    v, t = ops.marching_cubes(torch.from_numpy(level).to(dev))
    return Mesh(v * 2 - 1, t)


@pytest.fixture(scope="module")
def small_meshes(dev):
    return {"sphere": _mc_mesh(sphere(48), dev), "torus": _mc_mesh(torus(40), dev),
            "two_spheres": _mc_mesh(two_spheres(40), dev)}


@pytest.fixture(scope="module")
def bench_mesh(dev):
    torch.manual_seed(0)
    g = tt.find("few-step-triplane-dual-stable-diffusion")({"isosurface_deformable_grid": True}).to(dev)
    cache = (torch.randn(1, 6, 32, 256, 256, generator=torch.Generator().manual_seed(8)) * 0.5).to(dev)
    with torch.no_grad():
        (mesh,) = isosurface(cache, g.forward_field, DiffMarchingCubeHelper(128).to(dev))
    return mesh


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres"])
def test_atlas_matches_the_restatement(small_meshes, name):
    mesh = small_meshes[name]
    N, pad = 256, 2
    v_tex, t_tex, info = ops.uv_atlas(mesh.v_pos, mesh.t_pos_idx, mesh.topology, N, pad)
    v = mesh.v_pos.cpu().numpy()
    tri = mesh.t_pos_idx.cpu().numpy().astype(np.int64)
    pairs = U.face_pairs(tri)
    assert np.array_equal(pairs, mesh.topology.face_pairs.cpu().numpy())
    lab = U.labels(v, tri, pairs, 8, TAU)
    assert np.array_equal(info["labels"].cpu().numpy(), lab)
    chart = U.charts(tri, pairs, lab, info["singleton"].cpu().numpy())
    assert np.array_equal(info["chart"].cpu().numpy(), chart)
    box = U.chart_boxes(v, tri, lab, chart)
    assert np.array_equal(info["chart_box"].numpy(), box)
    off, s = U.pack(box, N, pad)
    assert np.array_equal(info["offsets"].numpy(), off) and info["scale"] == s
    want_tex, want_idx = U.emit(v, tri, lab, chart, box, off, s, N, pad)
    assert np.array_equal(t_tex.cpu().numpy(), want_idx)
    assert np.abs(v_tex.cpu().numpy() - want_tex).max() <= 1e-6
    # texel coverage: the overlap kernel's view is the rasterizer's, which the float64 count must equal away from
    # centres within rounding of an edge line
    cnt, amb = U.coverage(v_tex.cpu().numpy(), t_tex.cpu().numpy(), N)
    assert cnt.max() <= 1
    uv4 = torch.cat((v_tex * 2 - 1, torch.zeros_like(v_tex[:, :1]), torch.ones_like(v_tex[:, :1])), -1)
    rast = tt.raster.rasterize(uv4[None], t_tex, N)[0]
    covered = (rast[..., 3] > 0).cpu().numpy()
    assert np.array_equal(covered[~amb], cnt[~amb] > 0)
    assert abs(info["fill_ratio"] - covered.mean()) <= amb.mean() + 1e-9


def _invariants(mesh, v_tex, t_tex, info, N, pad):
    vt = v_tex.double().cpu()
    assert vt.min() >= 0 and vt.max() <= 1
    tri = mesh.t_pos_idx.long().cpu()
    tt_ = t_tex.long().cpu()
    v = mesh.v_pos.double().cpu()
    lab = info["labels"].long().cpu()
    chart = info["chart"].long().cpu()
    box = info["chart_box"].double()
    off = info["offsets"].double()
    s = info["scale"]
    # every UV vertex comes from one mesh vertex of one chart
    pair = torch.stack([tt_.reshape(-1), tri.reshape(-1)], 1).unique(dim=0)
    assert len(pair) == len(vt) and torch.equal(pair[:, 0], torch.arange(len(vt)))
    # UV = s * projection + chart offset, to float rounding
    ax = torch.tensor(U.AXES)
    cu, cv = ax[lab][:, 0], ax[lab][:, 1]
    P = v[tri]  # (T,3,3)
    pu = P.gather(2, cu[:, None, None].expand(-1, 3, 1))[..., 0]
    pv = P.gather(2, cv[:, None, None].expand(-1, 3, 1))[..., 0]
    Uw = off[chart, 0][:, None] + pad + 0.5 + (pu - box[chart, 0][:, None]) * s
    Vw = off[chart, 1][:, None] + pad + 0.5 + (pv - box[chart, 1][:, None]) * s
    got = vt[tt_] * N
    assert (got[..., 0] - Uw).abs().max() <= 2e-3 and (got[..., 1] - Vw).abs().max() <= 2e-3
    # signed UV area >= tau s^2 (3-D area) > 0 on faces whose area is far above float rounding
    e1, e2 = got[:, 1] - got[:, 0], got[:, 2] - got[:, 0]
    area_uv = 0.5 * (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    area_3d = 0.5 * torch.linalg.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]).norm(dim=-1) * s * s
    big = area_3d > 1e-3
    assert big.float().mean() > 0.5
    assert (area_uv[big] > 0).all()
    assert (area_uv[big] >= TAU * area_3d[big] * (1 - 1e-3) - 1e-4).all()
    # chart texel boxes (content + pad + 1/2 texel on every side) inside the texture and disjoint, so the contents of
    # two charts are more than 2 pad texels apart
    occ = torch.zeros(N, N, dtype=torch.int32)
    w = box[:, 2:] - box[:, :2]
    for c in range(info["charts"]):
        x0, y0 = int(off[c, 0]), int(off[c, 1])
        bw = int(np.ceil(float(w[c, 0]) * s)) + 2 * pad + 1
        bh = int(np.ceil(float(w[c, 1]) * s)) + 2 * pad + 1
        assert x0 >= 0 and y0 >= 0 and x0 + bw <= N and y0 + bh <= N
        occ[y0:y0 + bh, x0:x0 + bw] += 1
    assert occ.max() == 1
    lo, hi = got.amin(1), got.amax(1)  # every UV triangle inside its chart's box, pad + 1/2 texel from its border
    assert (lo[:, 0] >= off[chart, 0] + pad + 0.5 - 2e-3).all() and (lo[:, 1] >= off[chart, 1] + pad + 0.5 - 2e-3).all()
    # zero texel centres are covered twice (a fresh count by the overlap kernel)
    lib_flags = torch.empty(len(tri), device=v_tex.device, dtype=torch.uint8)
    tot = torch.empty(4, device=v_tex.device, dtype=torch.int32)
    lib = tt._lib.load()
    ws = torch.empty(int(lib.tt_uv_workspace_bytes(mesh.v_pos.shape[0], len(tri), N)), device=v_tex.device,
                     dtype=torch.uint8)
    tt._lib.check(lib.tt_uv_overlap(ops._ptr(v_tex), ops._ptr(t_tex), len(vt), mesh.v_pos.shape[0], len(tri), N,
                                    ops._ptr(ws), ops._ptr(lib_flags), ops._ptr(tot), ops._stream()), "overlap")
    assert int(tot[0]) == 0


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "bench"])
def test_atlas_invariants(small_meshes, bench_mesh, name):
    mesh = bench_mesh if name == "bench" else small_meshes[name]
    # the random-plane bench scene is a noise surface: ~55k charts at 128^3, whose (2p+1)^2-texel minimum boxes alone
    # exceed 1024^2 (uv_atlas raises for it); 2048^2 holds them
    N = 2048 if name == "bench" else 256
    v_tex, t_tex, info = ops.uv_atlas(mesh.v_pos, mesh.t_pos_idx, mesh.topology, N, 2)
    _invariants(mesh, v_tex, t_tex, info, N, 2)
    if name == "sphere":  # six axis caps, plus at most a few islands where the caps meet
        counts = torch.bincount(info["chart"].long().cpu())
        assert 6 <= info["charts"] <= 12
        assert counts.sort(descending=True)[0][:6].sum() >= 0.98 * counts.sum()


def test_bench_scene_does_not_fit_1024_and_says_so(bench_mesh):
    with pytest.raises(RuntimeError, match="do not fit a 1024"):
        ops.uv_atlas(bench_mesh.v_pos, bench_mesh.t_pos_idx, bench_mesh.topology, 1024, 2)


def test_atlas_and_texture_are_bit_identical_across_runs(bench_mesh):
    m = bench_mesh
    a = ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 2048, 2)
    b = ops.uv_atlas(m.v_pos, m.t_pos_idx, m.topology, 2048, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g = torch.Generator(device=m.v_pos.device).manual_seed(0)
    img = torch.rand(512, 512, 3, device=m.v_pos.device, generator=g)
    mask = torch.rand(512, 512, device=m.v_pos.device, generator=g) < 0.2
    assert torch.equal(ops.texture_fill(img, mask), ops.texture_fill(img, mask))


@pytest.mark.parametrize("H,W,frac", [(300, 200, 0.05), (256, 256, 0.3), (97, 301, 0.002)])
def test_fill_is_nearest(dev, H, W, frac):
    g = torch.Generator(device=dev).manual_seed(H)
    mask = torch.rand(H, W, device=dev, generator=g) < frac
    img = torch.rand(H, W, 4, device=dev, generator=g)
    out = ops.texture_fill(img, mask)
    assert torch.equal(out[mask], img[mask])
    # the source texel of every empty texel: fill an image of texel coordinates
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    src = ops.texture_fill(torch.stack([yy, xx], -1).float(), mask)
    d_src = ((src[..., 0].double() - yy) ** 2 + (src[..., 1].double() - xx) ** 2).sqrt().cpu().numpy()
    d_bf = np.sqrt(U.nearest_sq_dist(mask.cpu().numpy()))
    assert (d_src <= d_bf + 1.0 + 1e-9).all()
    assert (np.abs(d_src - d_bf) < 1e-9).mean() >= 0.999
    # ... and the value there
    s = src.long()
    assert torch.equal(out, img[s[..., 0], s[..., 1]])


def _exporter_modules(dev, resolution=64):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    r = tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=resolution), geometry=g, material=m,
                                    background=b).to(dev)
    # a smooth scene: planes drawn at 8^2 and upsampled
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    return r, g, m, b, cache


def test_exporter_bake_and_files(dev, tmp_path):
    r, g, m, b, cache = _exporter_modules(dev)
    N = 512
    exp = tt.find("multiprompt-mesh-exporter")({"save_uv": True, "texture_size": N, "texture_format": "png"},
                                               geometry=g, material=m, background=b)
    (out,) = exp(cache)
    assert out.save_name == "model.obj" and out.save_type == "obj"
    assert set(out.params) == {"mesh", "save_mat", "save_normal", "save_uv", "save_vertex_color", "map_Kd", "map_Ks",
                               "map_Bump", "map_Pm", "map_Pr", "map_format"}
    mesh, kd = out.params["mesh"], out.params["map_Kd"]
    assert kd.shape == (N, N, 3) and kd.min() >= 0 and kd.max() <= 1
    with torch.no_grad():
        want_mesh = r.isosurface(cache)[0]
    assert torch.equal(mesh.t_pos_idx, want_mesh.t_pos_idx)
    # bake: every covered texel = material.export(geometry.export(p)), p recomputed in torch from the UV triangle
    uv4 = torch.cat((mesh.v_tex * 2 - 1, torch.zeros_like(mesh.v_tex[:, :1]), torch.ones_like(mesh.v_tex[:, :1])), -1)
    rast = tt.raster.rasterize(uv4[None], mesh.t_tex_idx, N)[0]
    cov = rast[..., 3] > 0
    tid = rast[..., 3][cov].long() - 1
    py, px = torch.nonzero(cov, as_tuple=True)
    c = torch.stack([(px.double() + 0.5) / N, (py.double() + 0.5) / N], -1)
    T3 = mesh.v_tex.double()[mesh.t_tex_idx.long()[tid]]
    d = (T3[:, 1, 0] - T3[:, 0, 0]) * (T3[:, 2, 1] - T3[:, 0, 1]) - (T3[:, 1, 1] - T3[:, 0, 1]) * (T3[:, 2, 0] - T3[:, 0, 0])
    b1 = ((c[:, 0] - T3[:, 0, 0]) * (T3[:, 2, 1] - T3[:, 0, 1]) - (c[:, 1] - T3[:, 0, 1]) * (T3[:, 2, 0] - T3[:, 0, 0])) / d
    b2 = ((T3[:, 1, 0] - T3[:, 0, 0]) * (c[:, 1] - T3[:, 0, 1]) - (T3[:, 1, 1] - T3[:, 0, 1]) * (c[:, 0] - T3[:, 0, 0])) / d
    P3 = mesh.v_pos.double()[mesh.t_pos_idx.long()[tid]]
    p = (1 - b1 - b2)[:, None] * P3[:, 0] + b1[:, None] * P3[:, 1] + b2[:, None] * P3[:, 2]
    with torch.no_grad():
        want = m.export(**g.export(points=p.float(), space_cache=cache[:1]))["albedo"]
    assert (kd[cov] - want).abs().max().item() <= 1e-5
    # files: OBJ + MTL + PNG round trip; sampling the texture at each vertex's OBJ uv matches colorize_mesh's colour
    paths = save_obj(str(tmp_path / out.save_name), **out.params)
    assert sorted(os.path.basename(x) for x in paths) == ["model.mtl", "model.obj", "texture_kd.png"]
    lines = open(tmp_path / "model.obj").read().splitlines()
    vts = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("vt ")])
    faces = [ln.split()[1:] for ln in lines if ln.startswith("f ")]
    assert len(vts) == mesh.v_tex.shape[0] and len(faces) == mesh.t_pos_idx.shape[0]
    img = read_png(str(tmp_path / "texture_kd.png"))
    assert np.array_equal(img, (kd.cpu().numpy() * 255.0).astype(np.uint8))
    vpair = np.array([[int(x.split("/")[0]) - 1, int(x.split("/")[1]) - 1] for f in faces for x in f])
    col = colorize_mesh(cache[:1], g.export, [Mesh(mesh.v_pos, mesh.t_pos_idx)],
                        lambda f: m(f).clamp(0, 1))[0].v_rgb.cpu().numpy()
    tx = np.clip(np.floor(vts[vpair[:, 1], 0] * N), 0, N - 1).astype(int)
    ty = np.clip(np.floor((1.0 - vts[vpair[:, 1], 1]) * N), 0, N - 1).astype(int)  # undo the OBJ's v flip
    err = np.abs(img[ty, tx].astype(np.float64) / 255.0 - col[vpair[:, 0]])
    print(f"texture vs vertex colour: mean {err.mean():.4f} max {err.max():.4f}")
    assert err.mean() <= 0.02 and err.max() <= 0.15


def test_exporter_obj_format_sets_vertex_colours(dev):
    r, g, m, b, cache = _exporter_modules(dev)
    exp = tt.find("multiprompt-mesh-exporter")({"fmt": "obj"}, geometry=g, material=m, background=b)
    (out,) = exp(cache)
    assert out.params["save_vertex_color"] is True and out.params["save_mat"] is False
    mesh = out.params["mesh"]
    assert mesh.v_rgb.shape == mesh.v_pos.shape and mesh.v_rgb.min() >= 0 and mesh.v_rgb.max() <= 1
