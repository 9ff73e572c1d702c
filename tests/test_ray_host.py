"""Ray casting without a GPU: the header and the binding, the fp32 restatement of the slice walk against its own brute
force (tests/ray_reference.py), the committed ray sets' share of unclean rays, the direction table of the ambient-occlusion
rays, and the MTL writer's map_Ka."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ray_reference as R  # noqa: E402

from triplaneturbo_amd import _lib, export, ops  # noqa: E402

GRIDS = (1, 2, 3, 6, 7, 33)


def test_header_declares_and_lib_binds():
    for name in ("tt_ray_cast", "tt_ray_any", "tt_ray_ao"):
        assert name in _lib.SYMBOLS and name in _lib._PROTOS
    assert _lib.TT_RAY_MAX_DIRS == 1024
    assert _lib._expected_abi() == 17
    restype, argtypes = _lib._PROTOS["tt_ray_cast"]
    assert restype is _lib._I32 and len(argtypes) == 21 and argtypes[4] is _lib._F and argtypes[3] is _lib._I32
    assert len(_lib._PROTOS["tt_ray_any"][1]) == 19 and len(_lib._PROTOS["tt_ray_ao"][1]) == 21
    assert "tt_ray.hip" in _lib.SOURCES
    header = open(os.path.join(_lib.INCLUDE, "tt_abi.h")).read()
    assert "ray casting (tt_ray.hip)" in header
    for line in header.splitlines():  # the two older sections no longer list the query as missing
        if "Out of scope" in line:
            assert "ray casting" not in line


@pytest.mark.parametrize("name", ["lattice", "sphere24"])
def test_walk_equals_brute_force(name):
    """The restated slice walk gives the restated brute force's (t, face) bit for bit, and the any-hit walk its
    face >= 0, at every grid: seeded random rays, rays aimed in fp32 at vertices and edge midpoints from origins on
    the 1/6 lattice, axis-parallel rays lying in face planes."""
    v, tri = R.mesh(name)
    o1, d1 = R.random_rays(300, 7)
    o2, d2 = R.special_rays(name)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    hit, t, _ = R.pair_f32(o, d, v, tri)
    bt, bf = R.brute_f32(hit, t)
    assert (bf >= 0).sum() > len(o) // 2 and (bf < 0).sum() > 50
    for G in GRIDS:
        grid = R.Grid(v, tri, G)
        cells = []
        wt, wf = R.walk_f32(o, d, grid, hit, t, count=cells)
        assert np.array_equal(wf, bf), (name, G, np.nonzero(wf != bf)[0][:8])
        assert np.array_equal(wt.view(np.uint32), bt.view(np.uint32)), (name, G)
        assert np.array_equal(R.walk_f32(o, d, grid, hit, t, any_hit=True), bf >= 0), (name, G)
        assert max(cells) <= 3 * G + 2 * G  # a ray visits a few cells per slice, never the grid
    # with a t_max in the middle of the hits
    tm = float(np.median(bt[bf >= 0]))
    hit2, t2, _ = R.pair_f32(o, d, v, tri, t_max=tm)
    b2t, b2f = R.brute_f32(hit2, t2)
    assert (b2f < 0).sum() > (bf < 0).sum()
    for G in (1, 3, 7):
        wt, wf = R.walk_f32(o, d, R.Grid(v, tri, G), hit2, t2, t_max=tm)
        assert np.array_equal(wf, b2f) and np.array_equal(wt.view(np.uint32), b2t.view(np.uint32))


@pytest.mark.parametrize("name", ["tetra", "cube", "lattice", "sphere24"])
def test_committed_rays_are_clean_and_restatement_is_within_the_bar(name):
    """At most 1 % of a committed random set is unclean (checked with the float64 reference alone), and on the clean rays
    the fp32 restatement of the pair reports the reference's face with t within the bar."""
    v, tri = R.mesh(name)
    o, d, c = R.case(name)
    assert c["unclean"].mean() <= 0.01
    t, face, bary = R.restated(name)
    clean = ~c["unclean"]
    assert np.array_equal(face[clean], c["face"][clean])
    m = clean & (face >= 0)
    assert m.sum() > 300
    assert (np.abs(t[m].astype(np.float64) - c["t"][m]) <= R.T_BAR * c["s"][m]).all()
    assert (bary[m] >= 0).all() and (np.abs(bary[m].astype(np.float64).sum(1) - 1) <= 1e-6).all()


def test_faces_without_area_never_hit_in_the_restatement():
    for name in ("degenerate", "point"):
        v, tri = R.mesh(name)
        o1, d1 = R.random_rays(300, 5)
        o2, d2 = R.aimed_rays(v, tri, R.SIXTH_ORIGINS)
        o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
        hit, t, _ = R.pair_f32(o, d, v, tri)
        assert not hit.any() and not np.isnan(t).any()


def test_ao_directions():
    for K in (1, 2, 63, 64, 1024):
        d = ops.ao_directions(K)
        assert tuple(d.shape) == (K, 3) and d.dtype.is_floating_point and d.element_size() == 4
        x = d.numpy().astype(np.float64)
        assert np.abs(np.linalg.norm(x, axis=1) - 1).max() <= 1e-7
        assert (x[:, 2] > 0).all()
        assert np.array_equal(d.numpy(), ops.ao_directions(K).numpy())
        assert np.array_equal(d.numpy(), R.ao_directions(K))
    x = ops.ao_directions(1024).numpy().astype(np.float64)
    assert abs(x[:, 2].mean() - 2.0 / 3.0) < 2e-3  # cosine weighted: E[z] = 2/3
    assert np.abs(x[:, :2].mean(0)).max() < 2e-3
    for bad in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            ops.ao_directions(bad)


def _toy_mesh():
    return types.SimpleNamespace(v_pos=np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32),
                                 t_pos_idx=np.array([[0, 1, 2]], np.int32),
                                 v_tex=np.array([[0, 0], [1, 0], [0, 1]], np.float32),
                                 t_tex_idx=np.array([[0, 1, 2]], np.int32))


def test_save_mtl_map_ka(tmp_path):
    ao = np.linspace(0, 1, 64, dtype=np.float32).reshape(8, 8, 1)
    paths = export._save_mtl(str(tmp_path / "m.mtl"), "default", map_Ka=ao, map_format="png")
    assert str(tmp_path / "texture_ao.png") in paths
    text = open(tmp_path / "m.mtl").read()
    assert "map_Ka texture_ao.png\n" in text
    img = export.read_png(str(tmp_path / "texture_ao.png"))
    assert img.shape[:2] == (8, 8)
    assert np.array_equal(img[..., 0], (np.clip(ao[..., 0], 0, 1) * 255.0).astype(np.uint8))
    kd = np.full((8, 8, 3), 0.5, np.float32)
    os.makedirs(tmp_path / "a")
    files = export.save_obj(str(tmp_path / "a" / "model.obj"), _toy_mesh(), save_mat=True, save_uv=True, map_Kd=kd,
                            map_Ka=ao, map_format="png")
    assert any(f.endswith("texture_ao.png") for f in files)
    assert "map_Ka texture_ao.png\n" in open(tmp_path / "a" / "model.mtl").read()


def test_save_obj_without_map_ka_writes_what_it_wrote(tmp_path):
    kd = np.full((8, 8, 3), 0.5, np.float32)
    os.makedirs(tmp_path / "a")
    os.makedirs(tmp_path / "b")
    fa = export.save_obj(str(tmp_path / "a" / "model.obj"), _toy_mesh(), save_mat=True, save_uv=True, map_Kd=kd,
                         map_format="png")
    fb = export.save_obj(str(tmp_path / "b" / "model.obj"), _toy_mesh(), save_mat=True, save_uv=True, map_Kd=kd,
                         map_format="png", map_Ka=None)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) == ["model.mtl", "model.obj",
                                                                                        "texture_kd.png"]
    assert [os.path.basename(f) for f in fa] == [os.path.basename(f) for f in fb]
    for name in os.listdir(tmp_path / "a"):
        assert open(tmp_path / "a" / name, "rb").read() == open(tmp_path / "b" / name, "rb").read()
    # the text of the MTL as the writer has always written it
    assert open(tmp_path / "a" / "model.mtl").read() == ("newmtl default\nKa 0.0 0.0 0.0\nmap_Kd texture_kd.png\n"
                                                          "Ks 0.0 0.0 0.0\n")
