"""Mesh decimation without a GPU: the numpy restatement of the contract (tests/decimate_reference.py) and its trace
checker run on themselves, the header's constants and symbols, and the argument errors of ops.mesh_decimate that are
raised before any GPU work."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimate_reference as R  # noqa: E402

from triplaneturbo_amd import _lib, ops  # noqa: E402


def test_header_declares_the_decimation_entry_points_and_constants():
    names = ["workspace_bytes", "quadrics", "lock", "edges", "mark", "select", "apply", "emit_count", "emit"]
    assert all(f"tt_decimate_{n}" in _lib.SYMBOLS for n in names)
    assert 0.0 < _lib.TT_DECIMATE_QUANTILE < 1.0 and _lib.TT_DECIMATE_SELECT_PASSES >= 1
    assert _lib.TT_DECIMATE_MIN_FACES == 4
    assert "tt_decimate.hip" in _lib.SOURCES
    text = open(os.path.join(_lib.INCLUDE, "tt_abi.h")).read()
    for const in ("0x9E3779B1", "0x7F4A7C15", "0x85EBCA77", "0xC2B2AE3D", "0x7FEB352D", "0x846CA68B"):
        assert const in text  # the hash the restatement copies is written out in the contract


def test_hash_is_a_32_bit_mix_of_all_three_arguments():
    h = R.hash32(3, 7, 0)
    assert 0 <= h < 2 ** 32
    assert len({h, R.hash32(7, 3, 0), R.hash32(3, 7, 1), R.hash32(3, 8, 0), R.hash32(4, 7, 0)}) == 5


def test_icosphere_keeps_its_euler_characteristic_and_its_trace_checks():
    v, t = R.icosphere(2)
    assert t.shape == (320, 3) and R.manifold_stats(t) == (True, 2, 1)
    v2, t2, info = R.decimate(v, t, 80)
    assert R.manifold_stats(t2) == (True, 2, 1)
    assert 79 <= len(t2) <= 80 and not info["stalled"] and info["n_locked"] == 0
    assert info["n_rounds"] == len(info["trace"]) >= 2
    R.check_trace(v, t, info["trace"], 80, final=(v2, t2, info["vertex_map"]))
    # every input vertex ends in an output vertex, every output vertex is someone's image
    assert info["vertex_map"].min() >= 0 and set(info["vertex_map"].tolist()) == set(range(len(v2)))


def test_tetrahedron_stalls_at_four_faces():
    v, t = R.tetrahedron()
    v2, t2, info = R.decimate(v, t, 2)
    assert info["stalled"] and info["n_rounds"] == 0 and np.array_equal(t2, t) and np.array_equal(v2, v)
    R.check_trace(v, t, info["trace"], 2, final=(v2, t2, info["vertex_map"]), stalled=True)


def test_octahedron_stays_manifold():
    v, t = R.octahedron()
    v2, t2, info = R.decimate(v, t, 4)
    closed, chi, comps = R.manifold_stats(t2)
    assert closed and chi == 2 and comps == 1 and 4 <= len(t2) <= 8
    R.check_trace(v, t, info["trace"], 4, final=(v2, t2, info["vertex_map"]), stalled=info["stalled"])


def test_locked_vertices_of_an_open_and_of_a_non_manifold_mesh():
    v, t = R.height_field(5)
    topo = R.Topology(t, len(v))
    assert int(topo.locked.sum()) == 16
    v2, t2, info = R.decimate(v, t, 4)
    vm = info["vertex_map"]
    assert all(vm[i] >= 0 and np.array_equal(v2[vm[i]], v[i]) for i in np.flatnonzero(topo.locked))
    v, t = R.two_tetrahedra_sharing_an_edge()
    assert np.flatnonzero(R.Topology(t, len(v)).locked).tolist() == [0, 1]
    assert R.decimate(v, t, 4)[2]["stalled"]


def test_checker_rejects_two_kept_edges_that_share_a_neighbour():
    v, t = R.icosphere(2)
    topo, cost_bits, xopt, _ = R.round_edges(v, t, R.vertex_quadrics(v, t))
    valid = np.flatnonzero(cost_bits != R.INVALID)
    e0 = int(valid[0])
    e1 = next(int(e) for e in valid[1:] if topo.closed(*topo.edges[e]) & topo.closed(*topo.edges[e0])
              and not set(topo.edges[e].tolist()) & set(topo.edges[e0].tolist()))
    good = [(topo.edges[[e0]], xopt[[e0]], cost_bits[[e0]])]
    R.check_trace(v, t, good, 80)
    bad = [(topo.edges[[e0, e1]], xopt[[e0, e1]], cost_bits[[e0, e1]])]
    with pytest.raises(AssertionError, match="neighbourhood"):
        R.check_trace(v, t, bad, 80)


def test_checker_rejects_a_kept_edge_that_violates_the_link_condition():
    v, t = R.torus(3, 8)  # a ring of three: the endpoints of a ring edge share the third ring vertex as well
    topo = R.Topology(t, len(v))
    a, b = 0, 8
    assert (a, b) in topo.edge_index and len(np.intersect1d(topo.N(a), topo.N(b))) == 3
    Q = R.vertex_quadrics(v, t)
    x, cost, _ = R.solve_edge(Q[a] + Q[b], v[a], v[b])
    bad = [(np.array([[a, b]]), x.astype(np.float32)[None], np.array([R.cost_bits_of(cost)]))]
    with pytest.raises(AssertionError, match="link rule"):
        R.check_trace(v, t, bad, 8)
    assert R.round_edges(v, t, Q)[1][topo.edge_index[(a, b)]] == R.INVALID


def test_flip_test_rejects_collapses_on_a_noisy_sphere():
    v, t = R.icosphere(2, noise=0.03, seed=0)
    would_flip = R.round_edges(v, t, R.vertex_quadrics(v, t))[3]
    assert would_flip.any()


@pytest.mark.parametrize("target", [3, 0, -1, 2.5, "8", True, None])
def test_bad_target_faces_raises_before_any_gpu_work(target):
    v, t = (torch.from_numpy(x) for x in R.octahedron())  # CPU tensors: the argument check comes first
    with pytest.raises((TypeError, ValueError), match="target_faces"):
        ops.mesh_decimate(v, t, target)


def test_cpu_tensors_and_bad_max_rounds_raise():
    v, t = (torch.from_numpy(x) for x in R.octahedron())
    with pytest.raises(ValueError, match="max_rounds"):
        ops.mesh_decimate(v, t, 4, max_rounds=-1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mesh_decimate(v, t, 4)
