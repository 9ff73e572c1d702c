"""The one cell rule of the triangle grid (csrc/tt_trigrid.h: cell(x) = clamp(floor((x - lo) * inv_h), 0, G - 1) in fp32)
across its consumers -- the distance grid's build, the point keys, the winding tree's leaves -- against the numpy
restatements the other tests already use (distance_reference.cell, winding_reference.face_keys).  Integers throughout,
so every comparison is exact.  The lattice mesh has its vertices on multiples of 1/6: many coordinates fall exactly on
cell planes for G in {2, 3, 6}, where a rule that rounded differently in one consumer would bin them differently."""
import os
import sys

import numpy as np
import pytest
import torch

from triplaneturbo_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_reference as D  # noqa: E402
import ray_reference as R  # noqa: E402
import winding_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu
GRIDS = (1, 2, 3, 6, 7, 33)
LEVELS = (0, 1, 3)
MESHES = {"lattice": lambda: R.mesh("lattice"), "spanning": D.spanning}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mesh(name):
    v, tri = MESHES[name]()
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(tri, np.int32)


def _key(c, G):
    return (c[:, 0] * G + c[:, 1]) * G + c[:, 2]


def _restated_csr(v, tri, G):
    """(cell_ptr (G^3 + 1), the faces of every row in ascending order): every face into the cells between the cells of
    its box's two corners."""
    lo, _, _, inv_h = D.box(v, G)
    p3 = v[tri]
    c0 = D.cell(p3.min(1), lo, inv_h, G)
    c1 = np.maximum(c0, D.cell(p3.max(1), lo, inv_h, G))
    rows, faces = [], []
    for f in range(len(tri)):
        z, y, x = np.meshgrid(*(np.arange(c0[f, a], c1[f, a] + 1) for a in range(3)), indexing="ij")
        rows.append(((z * G + y) * G + x).reshape(-1))
        faces.append(np.full(rows[-1].size, f, np.int64))
    rows, faces = np.concatenate(rows), np.concatenate(faces)
    ptr = np.zeros(G ** 3 + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=G ** 3))
    return ptr, faces[np.lexsort((faces, rows))]


@pytest.mark.parametrize("name", sorted(MESHES))
def test_grid_rows_are_the_restated_binning(dev, name):
    v, tri = _mesh(name)
    T = len(tri)
    for G in GRIDS:
        tg = ops.TriangleGrid(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev), grid=G)
        ptr, faces = _restated_csr(v, tri, G)
        got_ptr = tg.cell_ptr.cpu().numpy().astype(np.int64)
        assert np.array_equal(got_ptr, ptr), G
        assert tg.M == ptr[-1] == len(faces), G
        row = np.repeat(np.arange(G ** 3), np.diff(got_ptr))
        got = np.sort(row * T + tg.cell_tri.cpu().numpy().astype(np.int64)) % T  # arrival order inside a row means nothing
        assert np.array_equal(got, faces), G


@pytest.mark.parametrize("name", sorted(MESHES))
def test_point_keys_are_the_restated_keys(dev, name):
    v, tri = _mesh(name)
    ext = D.box(v, 1)[1]
    shifts = [np.zeros(3, np.float32)] + [s * np.float32(2) * ext * np.eye(3, dtype=np.float32)[a]
                                          for a in range(3) for s in (np.float32(-1), np.float32(1))]
    pts = np.concatenate([v + s for s in shifts] + [np.array([[0, np.nan, 0]], np.float32)]).astype(np.float32)
    p = torch.from_numpy(pts).to(dev)
    for G in GRIDS:
        tg = ops.TriangleGrid(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev), grid=G)
        keys = torch.empty(len(pts), device=dev, dtype=torch.int64)
        ops._launch("tt_dist_keys", p, len(pts), tg.G, *tg.lo, tg.ext, tg.inv_h, keys)
        lo, e, _, inv_h = D.box(v, G)
        q = np.minimum(np.maximum(pts[:-1], lo), lo + e)
        want = np.append(_key(D.cell(q, lo, inv_h, G), G), -1)
        assert np.array_equal(keys.cpu().numpy(), want), G


@pytest.mark.parametrize("name", sorted(MESHES))
def test_tree_leaves_are_the_restated_face_keys(dev, name):
    v, tri = _mesh(name)
    for L in LEVELS:
        tree = ops.WindingTree(torch.from_numpy(v).to(dev), torch.from_numpy(tri).to(dev), levels=L)
        ptr = np.zeros(8 ** L + 1, np.int64)
        ptr[1:] = np.cumsum(np.bincount(W.face_keys(v, tri, L), minlength=8 ** L))
        assert np.array_equal(tree.leaf_ptr.cpu().numpy().astype(np.int64), ptr), L
