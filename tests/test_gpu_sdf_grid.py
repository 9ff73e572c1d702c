"""HIP mesh to SDF grid (tt_sdfgrid_*; ops.mesh_sdf_grid, Mesh.sdf_grid, Mesh.solidify, the exporter's
solidify_resolution) against the composition of the existing queries, bit for bit: level ==
mesh.signed_distance(corners).clamp(-tau, tau) for closed inputs, d2 / face of mesh.closest_point on the band corners
for every input, and the far-sign rule evaluated in torch for open ones.  Mesh.solidify is held to conditions that
follow from the field being 1-Lipschitz (tests/sdf_grid_reference.py holds its numpy restatement to the same ones).
Grids of at most 40^3, meshes from marching cubes of analytic fields at no more than 32^3."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import triplaneturbo_amd as tt
from triplaneturbo_amd import ops, viewer
from triplaneturbo_amd.export import save_obj
from triplaneturbo_amd.isosurface import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mc_reference as M  # noqa: E402
import sdf_grid_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF_GRID = ((-0.0371, 0.0193, -0.0517), 1.09)  # explicit bounds that line up with nothing


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


_MESHES = {}


def gpu_mesh(name, dev, res=32):
    if (name, res) not in _MESHES:
        v, t = S.mesh(name, res)
        _MESHES[name, res] = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(t).to(dev))
    return _MESHES[name, res]


def to_mesh(v, t, dev):
    return Mesh(torch.as_tensor(np.asarray(v, np.float32)).to(dev), torch.as_tensor(np.asarray(t, np.int32)).to(dev))


def corners(info, R):
    idx = torch.stack(torch.meshgrid(*[torch.arange(R, device=info["lo"].device)] * 3, indexing="ij"), -1)
    return (info["lo"] + idx.float() * info["h"]).view(-1, 3)


def far_rule(sign_mask, inside):
    """+-1 per corner: a sign corner's own sign, else that of the nearest sign corner below it along the last axis,
    + when there is none."""
    R = sign_mask.shape[0]
    k = torch.arange(R, device=sign_mask.device).expand(R, R, R)
    last = torch.cummax(torch.where(sign_mask, k, torch.full_like(k, -1)), dim=2)[0]
    own = torch.where(inside, -1.0, 1.0)
    return torch.where(last >= 0, torch.gather(own, 2, last.clamp(min=0)), torch.ones_like(own))


def check_grid(mesh, R, band, bounds=None, closed=False):
    """Every statement of the contract that holds for any input; with closed=True the oracle at every corner too."""
    level, info = mesh.sdf_grid(R, band, bounds)
    tau, h = info["tau"], info["h"]
    assert tau == float(np.float32(band) * np.float32(h))
    if bounds is not None:
        assert h == float(np.float32(bounds[1]) / np.float32(R - 1))
        assert info["lo"].tolist() == [float(np.float32(x)) for x in bounds[0]]
    P = corners(info, R)
    d2, face, _ = mesh.closest_point(P)
    d = d2.sqrt()
    band_mask = d < tau
    n_band = int(band_mask.sum())
    print(f"R {R} band {band}: {n_band} band corners of {R ** 3}, {info['sign_corners']} sign corners")
    assert info["band_corners"] == n_band
    got_face = info["face"].view(-1)
    assert torch.equal(got_face >= 0, band_mask)
    assert torch.equal(got_face[band_mask], face[band_mask])
    assert (got_face[~band_mask] == -1).all()
    oracle = mesh.signed_distance(P).clamp(-tau, tau)
    assert torch.equal(level.view(-1)[band_mask], oracle[band_mask])  # bit for bit: d2, the root, the sign
    # the other corners: +-tau, by the far-sign rule from the sign corners
    sign_tau = float(np.float32(max(band, S.SIGN_BAND)) * np.float32(h))
    sign_mask = d < sign_tau
    assert info["sign_corners"] == int(sign_mask.sum())
    if band >= S.SIGN_BAND:
        assert torch.equal(sign_mask, band_mask)
    inside = torch.zeros_like(sign_mask)
    inside[sign_mask] = mesh.winding_number(P[sign_mask]) > 0.5
    sgn = far_rule(sign_mask.view(R, R, R), inside.view(R, R, R))
    want = sgn * torch.where(band_mask, d, torch.full_like(d, tau)).view(R, R, R)
    assert torch.equal(level, want)
    if closed:
        assert torch.equal(level, oracle.view(R, R, R))
    return level, info


# ---- 1. equals the oracle, bit for bit ----
@pytest.mark.parametrize("band", [0.5, 2.0, 3.5])
@pytest.mark.parametrize("grid", ["default33", "explicit24"])
@pytest.mark.parametrize("name", list(S.FIELDS))
def test_equals_the_composition_of_the_queries(dev, name, grid, band):
    mesh = gpu_mesh(name, dev)
    R, bounds = (33, None) if grid == "default33" else (24, OFF_GRID)
    _, info = check_grid(mesh, R, band, bounds, closed=True)
    assert 0 < info["band_corners"] < R ** 3


# ---- 2. where the scatter can go wrong ----
def test_one_triangle_larger_than_the_grid(dev):
    mesh = to_mesh([[-5.0, -4.0, 0.31], [6.0, -3.0, 0.4], [0.2, 7.0, 0.55]], [[0, 1, 2]], dev)
    _, info = check_grid(mesh, 16, 2.0, ((0.0, 0.0, 0.0), 1.0))
    assert info["band_corners"] >= 16 * 16 * 3  # the slab of the plane, through the whole grid


def test_mesh_partly_outside_the_bounds(dev):
    mesh = gpu_mesh("sphere", dev)
    _, info = check_grid(mesh, 20, 2.0, ((0.4, 0.3, 0.2), 0.5))
    assert info["band_corners"] > 0
    _, info = check_grid(mesh, 12, 3.0, ((2.0, 2.0, 2.0), 0.5))  # nowhere near: no band corner, all +tau
    assert info["band_corners"] == 0


def test_zero_area_triangles_among_good_ones(dev):
    v, t = S.mesh("sphere", 16)
    extra = np.array([[0, 0, 5], [7, 7, 7], [3, 9, 3]], np.int32)
    v2 = np.concatenate([v, [[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.3, 0.3, 0.3]]]).astype(np.float32)  # a collinear one
    n = len(v)
    t2 = np.concatenate([extra, t, [[n, n + 1, n + 2]]]).astype(np.int32)
    check_grid(to_mesh(v2, t2, dev), 24, 2.0, OFF_GRID)


def test_triangles_lying_exactly_in_grid_planes(dev):
    # h = 1/16 exactly: the triangles lie in the planes k = 8 and i = 4, with vertices on corners and between them
    v = [[0.25, 0.25, 0.5], [0.75, 0.3125, 0.5], [0.40625, 0.8125, 0.5],
         [0.25, 0.125, 0.125], [0.25, 0.875, 0.25], [0.25, 0.5, 0.9375]]
    mesh = to_mesh(v, [[0, 1, 2], [3, 4, 5]], dev)
    level, info = check_grid(mesh, 17, 2.0, ((0.0, 0.0, 0.0), 1.0))
    assert info["h"] == 0.0625
    assert (level[:, :, 8] == 0).any() and (level[4] == 0).any()  # corners ON a triangle: distance exactly 0


def test_coincident_triangles_tie_to_the_smaller_face(dev):
    v, t = S.mesh("sphere", 12)
    t2 = np.concatenate([t[40:60], t, t[:30]]).astype(np.int32)  # faces 0..19 again at 60.., faces 20..49 again at the end
    mesh = to_mesh(v, t2, dev)
    _, info = check_grid(mesh, 24, 2.0, OFF_GRID)
    face = info["face"][info["face"] >= 0]
    assert not ((face >= 20 + 40) & (face < 20 + 60)).any() and not (face >= 20 + len(t)).any()  # never the later copy
    assert (face < 20).any()


@pytest.mark.parametrize("band,R", [(0.5, 6), (3.0, 10), (16.0, 36)])
def test_resolution_at_its_minimum_for_the_band(dev, band, R):
    mesh = gpu_mesh("sphere", dev, 16)
    check_grid(mesh, R, band, closed=band <= 3.0)
    with pytest.raises(ValueError, match="leaves no room"):
        mesh.sdf_grid(R - 1, band)


# ---- 3. open input ----
@pytest.mark.parametrize("band", [2.0, 3.5])
def test_open_inputs_follow_the_far_sign_rule(dev, band):
    v, t = S.mesh("sphere", 24)
    upper = t[(v[t.astype(np.int64)][:, :, 2] > 0.5).all(1)]  # a hemisphere, open along its rim
    _, info = check_grid(to_mesh(v, upper, dev), 33, band)
    assert 0 < info["band_corners"] < 33 ** 3
    tri = to_mesh([[0.2, 0.3, 0.4], [0.9, 0.35, 0.5], [0.45, 0.8, 0.65]], [[0, 1, 2]], dev)
    check_grid(tri, 24, band)
    check_grid(tri, 24, band, OFF_GRID)


# ---- 4. determinism ----
def test_two_calls_and_permuted_triangles_are_bit_identical(dev):
    v, t = S.mesh("torus", 16)
    mesh = to_mesh(v, t, dev)
    R, band = 24, 2.0
    level, info = mesh.sdf_grid(R, band, OFF_GRID)
    level2, info2 = mesh.sdf_grid(R, band, OFF_GRID)
    assert torch.equal(level, level2) and torch.equal(info["face"], info2["face"])
    perm = np.random.default_rng(5).permutation(len(t))
    shuffled = to_mesh(v, t[perm], dev)
    level3, info3 = shuffled.sdf_grid(R, band, OFF_GRID)
    assert torch.equal(level, level3) and info3["band_corners"] == info["band_corners"]
    # face maps through the permutation wherever the minimum is unique (float64: the runner-up is clearly farther)
    band_mask = (info["face"] >= 0).view(-1).cpu().numpy()
    P = corners(info, R).cpu().numpy()[band_mask]
    two = np.sort(S.D.pair_matrix(P, v, t).numpy(), 1)[:, :2]
    unique = two[:, 1] - two[:, 0] > 1e-6 * info["tau"] ** 2
    old = info["face"].view(-1).cpu().numpy()[band_mask]
    new = info3["face"].view(-1).cpu().numpy()[band_mask]
    assert unique.sum() > 100
    assert np.array_equal(perm[new[unique]], old[unique])


# ---- 5. solidify: derivable conditions only ----
def arrays(mesh):
    return mesh.v_pos.cpu().numpy(), mesh.t_pos_idx.cpu().numpy()


def within(mesh, points):
    return mesh.closest_point(points)[0].sqrt().max().item()


@pytest.mark.parametrize("name", list(S.FIELDS))
def test_solidify_of_a_closed_input(dev, name):
    src = gpu_mesh(name, dev, 24)
    out = src.solidify(32, band=2.0)
    ex = out.extras["solidify"]
    v, t = arrays(out)
    comps, chi = S.GENUS_SUM[name]
    assert S.is_closed(t, len(v)) and S.n_components(v, t) == comps and M.euler_characteristic(v, t) == chi
    assert M.signed_volume(v, t) > 0
    far = within(src, out.v_pos)
    print(f"{name}: {ex}, farthest vertex {far / ex['h']:.4f} h")
    assert far <= ex["h"] * (1 + 1e-4)
    assert ex["resolution"] == 32 and ex["faces"] == len(t) and ex["components_dropped"] == 0 and ex["band_corners"] > 0
    assert not out.v_pos.requires_grad


def test_solidify_merges_overlapping_spheres(dev):
    parts = [S.analytic_sphere(c, r, 24) for c, r in S.OVERLAP]
    out = to_mesh(*S.concat(*parts), dev).solidify(32, band=2.0)
    sd = torch.stack([to_mesh(*p, dev).signed_distance(out.v_pos) for p in parts], -1).cpu().numpy()
    S.check_overlap(*arrays(out), sd, out.extras["solidify"]["h"])


def test_solidify_drops_a_cavity_wall_unless_asked_to_keep_it(dev):
    c, r_out, r_in = S.NESTED
    src = to_mesh(*S.sphere_with_cavity(24), dev)
    out = src.solidify(32, band=2.0)
    v, t = arrays(out)
    assert out.extras["solidify"]["components_dropped"] == 1
    assert S.is_closed(t, len(v)) and S.n_components(v, t) == 1
    outer = to_mesh(*S.analytic_sphere(c, r_out, 24), dev)
    assert within(outer, out.v_pos) <= out.extras["solidify"]["h"] * (1 + 1e-4)
    kept = src.solidify(32, band=2.0, keep_cavities=True)
    v2, t2 = arrays(kept)
    assert kept.extras["solidify"]["components_dropped"] == 0
    assert S.is_closed(t2, len(v2)) and S.n_components(v2, t2) == 2


def test_solidify_closes_a_simplified_mesh(dev):
    out = gpu_mesh("sphere", dev).simplify(grid=10).solidify(32)
    v, t = arrays(out)
    assert S.is_closed(t, len(v))


def test_solidify_offset_and_its_limit(dev):
    r = 0.33
    src = to_mesh(*S.analytic_sphere((0.5, 0.5, 0.5), r, 32), dev)
    h = src.sdf_grid(32, 3.0)[1]["h"]
    out = src.solidify(32, band=3.0, offset=2 * h)
    v, t = arrays(out)
    assert S.is_closed(t, len(v))
    radius = np.linalg.norm(v.astype(np.float64) - 0.5, axis=-1)
    print(f"offset 2h: radius - (r + 2h) in [{(radius - r - 2 * h).min() / h:.4f}, {(radius - r - 2 * h).max() / h:.4f}] h")
    assert np.abs(radius - (r + 2 * h)).max() <= h
    eroded = src.solidify(32, band=3.0, offset=-2 * h)
    assert S.is_closed(eroded.t_pos_idx.cpu().numpy(), eroded.v_pos.shape[0])
    with pytest.raises(ValueError, match="beyond tau - h"):
        src.solidify(32, band=3.0, offset=2.01 * h)
    with pytest.raises(ValueError, match="beyond tau - h"):
        src.solidify(32, band=1.5, offset=-0.6 * h)


def test_solidify_project_and_vertex_colours(dev):
    src = gpu_mesh("torus", dev, 24)
    col = Mesh(src.v_pos, src.t_pos_idx)
    col.set_vertex_color(src.v_pos.clone())  # colour = position: the interpolated colour is the closest point
    out = col.solidify(32, project=True)
    side = 31 * out.extras["solidify"]["h"]
    d2 = src.closest_point(out.v_pos)[0]
    print(f"project: max d / side {d2.sqrt().max().item() / side:.2e}")
    assert d2.max().item() <= (1e-5 * side) ** 2
    assert out.v_rgb.shape == out.v_pos.shape and torch.equal(out.v_rgb, out.v_pos)
    v, t = arrays(out)
    assert S.is_closed(t, len(v))
    plain = col.solidify(32)
    assert (plain.v_rgb - plain.v_pos).norm(dim=-1).max().item() <= out.extras["solidify"]["h"] * (1 + 1e-4)


# ---- 6. the exporter (the set-up of tests/test_gpu_export.py::_exporter_modules) ----
@pytest.fixture(scope="module")
def modules(dev):
    s = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_mesh_renderer_config.json")))
    t = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_training_config.json")))
    torch.manual_seed(0)
    g = tt.find(t["geometry_type"])(dict(t["geometry"], isosurface_deformable_grid=False)).to(dev)
    m = tt.find(t["material_type"])(t["material"]).to(dev)
    b = tt.find("solid-color-background")({"color": (1.0, 1.0, 1.0)}).to(dev)
    r = tt.find(s["renderer_type"])(dict(s["renderer"], isosurface_resolution=32), geometry=g, material=m,
                                    background=b).to(dev)
    low = torch.randn(2, 6 * 32, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.5
    cache = F.interpolate(low, size=(64, 64), mode="bilinear", align_corners=True).reshape(2, 6, 32, 64, 64).to(dev)
    return r, g, m, b, cache


def test_exporter_solidifies_on_request_and_is_untouched_otherwise(modules, tmp_path):
    r, g, m, b, cache = modules
    cfg = {"save_uv": True, "texture_size": 256, "texture_format": "png"}
    make = lambda: tt.find("multiprompt-mesh-exporter")(cfg, geometry=g, material=m, background=b)  # noqa: E731
    exp = make()
    assert exp.solidify_resolution is None and exp.solidify_offset == 0.0
    exp.solidify_resolution = 40
    (out,) = exp(cache)
    mesh = out.params["mesh"]
    with torch.no_grad():
        full = r.isosurface(cache)[0]
    want = full.solidify(40)
    assert torch.equal(mesh.v_pos, want.v_pos) and torch.equal(mesh.t_pos_idx, want.t_pos_idx)
    v, t = arrays(mesh)
    assert S.is_closed(t, len(v))
    assert mesh.extras["solidify"]["resolution"] == 40
    paths = save_obj(str(tmp_path / out.save_name), **out.params)
    assert "model.obj" in [os.path.basename(x) for x in paths]
    loaded, tex = viewer.load_obj(str(tmp_path / "model.obj"), device=mesh.v_pos.device)
    assert loaded.t_pos_idx.shape[0] == len(t) and tex is not None
    lv, lt = arrays(loaded)
    assert S.is_closed(lt, len(lv))
    # solidify feeds the other steps
    exp.decimate_target_faces = max(len(t) // 2, 8)
    (dec,) = exp(cache)
    assert 0 < dec.params["mesh"].t_pos_idx.shape[0] < len(t)
    exp.decimate_target_faces = None
    # unset: bit for bit the output of an exporter whose attributes were never touched
    exp.solidify_resolution = None
    (plain,) = exp(cache)
    (fresh,) = make()(cache)
    for key in ("v_pos", "t_pos_idx", "v_tex", "t_tex_idx"):
        assert torch.equal(getattr(plain.params["mesh"], key), getattr(fresh.params["mesh"], key))
    assert torch.equal(plain.params["mesh"].t_pos_idx, full.t_pos_idx)
    assert torch.equal(plain.params["map_Kd"], fresh.params["map_Kd"])
    assert "solidify" not in plain.params["mesh"].extras
    exp.solidify_offset = 0.01
    with pytest.raises(ValueError, match="solidify_offset needs solidify_resolution"):
        exp(cache)
