"""The numpy restatement of isotropic remeshing (tests/remesh_reference.py) on itself, without a GPU: on the three inputs
of the GPU test it must keep the topology, leave no edge with len2 > hi2, and strictly improve the share of short
edges, the mean minimum angle and (on the marching-cubes mesh) the mean |valence - 6|; its own trace must pass its
checker and replay to its output."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_reference as D  # noqa: E402
import mc_reference as MC  # noqa: E402
import remesh_reference as R  # noqa: E402


@pytest.fixture(scope="module")
def sphere():
    mc = MC.marching_cubes(R.bumpy_sphere_level(20))
    assert len(mc.t_pos_idx) == 1312 and D.manifold_stats(mc.t_pos_idx) == (True, 2, 1)
    return mc.v_pos, mc.t_pos_idx


def run(v, t, factor, is_mc):
    L = factor * R.mean_edge(v, t)
    v2, t2, info = R.remesh(v, t, L)
    before, after = R.quality(v, t, L), R.quality(v2, t2, L)
    print(f"L = {factor} x mean edge: {before} -> {after}; rounds {info['rounds']}, split {info['n_split']}, "
          f"collapsed {info['n_collapsed']}, flipped {info['n_flipped']}, reverted {info['n_reverted']}")
    assert D.manifold_stats(t2) == D.manifold_stats(t)
    assert not info["split_capped"] and not info["rounds_capped"] and after["n_long"] == 0
    assert after["short_share"] < before["short_share"]
    assert after["min_angle_mean"] > before["min_angle_mean"]
    if is_mc:
        assert after["valence_dev"] < before["valence_dev"]
    R.check_trace(v, t, L, info["trace"], final=(v2, t2))
    return info


def test_mc_sphere_coarser(sphere):
    info = run(*sphere, 1.5, True)
    assert sum(info["n_collapsed"]) > 0 and sum(info["n_flipped"]) > 0


def test_mc_sphere_finer(sphere):
    info = run(*sphere, 0.6, True)
    assert info["n_split"][0] > 0


def test_torus():
    v, t = D.torus(32, 16)
    assert D.manifold_stats(t) == (True, 0, 1)
    run(v, t, 1.0, False)


def test_split_templates_conform_and_keep_the_surface(sphere):
    """One pass on a mesh where faces have 0, 1, 2 and 3 marked edges: the area is kept, the topology is kept, every
    new vertex is the fp32 midpoint of its edge."""
    v, t = sphere
    L = 0.75 * R.mean_edge(v, t)
    hi2 = R.thresholds(L)[0]
    v2, t2, edges = R.split_pass(v, t, hi2)
    assert len(v2) == len(v) + len(edges) and 0 < len(edges)
    area = lambda p, f: np.linalg.norm(np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]), axis=1).sum() / 2
    assert abs(area(v2.astype(np.float64), t2) - area(v.astype(np.float64), t)) < 1e-6
    assert D.manifold_stats(t2) == D.manifold_stats(t)
    assert np.array_equal(v2[len(v):], R.midpoint(v[edges[:, 0]], v[edges[:, 1]]))
    all_edges, _, fe2e, _, _ = R.edge_table(t, len(v))
    marked = R.len2(v[all_edges[:, 0]], v[all_edges[:, 1]]) > hi2
    per_face = marked[fe2e].reshape(-1, 3).sum(1)
    assert set(per_face.tolist()) == {0, 1, 2, 3}  # every template is exercised
    assert len(t2) == len(t) + per_face.sum()
