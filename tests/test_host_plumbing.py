"""The host plumbing the mesh-stage wrappers share, without a GPU: every constant of include/tt_abi.h through _lib, the
one CSR builder (ops._csr) against a plain loop and against the three formulations it replaced, and the shared
validators (ops._chk's wildcard shapes, ops._chk_index, ops._minmax / _chk_range, ops._chk_size)."""
import os
import re

import pytest
import torch

from triplaneturbo_amd import _lib, ops, raster

HEADER = open(os.path.join(_lib.INCLUDE, "tt_abi.h")).read()


def test_every_constant_of_the_header_is_bound():
    loose = set(re.findall(r"#\s*define\s+(TT_\w+)[ \t]+[^\s/]", HEADER))  # a name, then anything but a comment
    assert len(loose) > 40 and loose - set(_lib._DEFINES) == set()
    for name, value in _lib._DEFINES.items():
        assert getattr(_lib, name) is value
    assert _lib.TT_MESH_MAX_ITEMS == 1 << 28 and _lib.TT_RAST_MAX_TRIS == 1 << 24
    assert _lib.TT_UV_MAX_FACES == (1 << 24) - 1
    assert (_lib.TT_UV_DEFAULT_TAU, _lib.TT_UV_MAX_TAU, _lib.TT_MESH_COS_EPS, _lib.TT_UV_PACK_REL_PREC) == \
        (0.3, 0.577, 1e-8, 1e-4)
    assert (_lib.TT_OK, _lib.TT_ERR_BAD_ARG, _lib.TT_ERR_UNSUPPORTED, _lib.TT_ERR_LAUNCH, _lib.TT_ERR_DEVICE) == \
        (0, -1, -2, -3, -4)
    assert (_lib.TT_PLACE_TT, _lib.TT_PLACE_CENTER) == (0, 1) and _lib.PLACEMENTS == {"tt": 0, "center": 1}
    assert ops.UV_DEFAULT_TAU is _lib.TT_UV_DEFAULT_TAU and ops.UV_DEFAULT_ROUNDS == 8
    assert ops.UV_MAX_OVERLAP_ROUNDS == 4 and raster.MAX_TRIS == 1 << 24


def test_constant_expressions_are_parsed_not_guessed():
    _, d = _lib._parse_abi("#define TT_A ((1 << 24) - 1)\n#define TT_B -(2) + 0x10\n#define TT_C 1e-4\n"
                           "#define TT_D .5F /* half */\n#define TT_GUARD\nenum e { TT_E = -2, TT_F = 1 << 3 };\n")
    assert d == {"TT_A": 16777215, "TT_B": 14, "TT_C": 1e-4, "TT_D": 0.5, "TT_E": -2, "TT_F": 8}
    assert type(d["TT_A"]) is int and type(d["TT_C"]) is float
    for bad in ("#define TT_X (1 << )\n", "#define TT_X 2 * 3\n", "#define TT_X 1u\n", "#define TT_X TT_Y\n",
                "#define TT_X __import__('os')\n", "#define TT_X 1.5.2\n", "enum e { TT_X, TT_Y };\n"):
        with pytest.raises(ValueError, match="TT_X"):
            _lib._parse_abi(bad)


# ---------------------------------------------------------------------------------------------------------------
def _csr_loop(row, col, n_rows):
    rows = [sorted(c for r, c in zip(row.tolist(), col.tolist()) if r == k) for k in range(n_rows)]
    ptr = [0]
    for r in rows:
        ptr.append(ptr[-1] + len(r))
    return ptr, [c for r in rows for c in r]


def _old_ptr(src, n):
    ptr = torch.zeros(n + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.bincount(src, minlength=n), 0)
    return ptr.int()


def _old_tet_grid(edges, Nv):  # TetGrid.vert_ptr / vert_col as it was
    Ne = edges.shape[0]
    src = edges.long().t().reshape(-1)
    eid = torch.arange(Ne).repeat(2)
    order = torch.sort(torch.add(eid, src, alpha=Ne), stable=True)[1]
    return _old_ptr(src, Nv), eid[order].int()


def _old_nbr(edges, V):  # MeshTopology._nbr as it was
    e0, e1 = edges.long().unbind(1)
    src, dst = torch.cat([e0, e1]), torch.cat([e1, e0])
    order = torch.sort(torch.add(dst, src, alpha=max(V, 1)), stable=True)[1]
    return _old_ptr(src, V), dst[order].int()


def _old_corners(idx, G):  # mesh_tangents' group -> corner table as it was
    key = idx.reshape(-1).long()
    return _old_ptr(key, G), torch.sort(key, stable=True)[1].int()


CSR_EDGES = {  # (pairs, n_rows): pairs double as edge lists (a, b) for the old formulations
    "rows_1_and_3_empty": ([[0, 2], [2, 2], [0, 0]], 4),  # two self pairs: (2, 2) and (0, 0) appear twice as neighbours
    "descending": ([[4, 5], [3, 4], [2, 4], [1, 3], [0, 1]], 6),
    "one_row": ([[0, 0], [0, 0]], 1),
    "empty": ([], 3),
}


@pytest.mark.parametrize("case", sorted(CSR_EDGES))
def test_csr_builder_matches_a_loop_and_the_three_old_tables(case):
    pairs, n = CSR_EDGES[case]
    edges = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    E = edges.shape[0]

    def check(row, col, n_rows, n_cols, old):
        ptr, out = ops._csr(row, col, n_rows, n_cols)
        want_ptr, want_col = _csr_loop(row, col, n_rows)
        assert ptr.dtype == out.dtype == torch.int32 and ptr.is_contiguous() and out.is_contiguous()
        assert ptr.tolist() == want_ptr and out.tolist() == want_col
        assert torch.equal(ptr, old[0]) and torch.equal(out, old[1])

    e0, e1 = edges.unbind(1)
    check(torch.cat([e0, e1]), torch.cat([e1, e0]), n, n, _old_nbr(edges, n))
    check(edges.t().reshape(-1), torch.arange(E).repeat(2), n, E, _old_tet_grid(edges, n))
    tri = torch.cat([edges, edges[:, :1]], 1)  # faces (a, b, a): every group's corners in ascending corner id
    check(tri.reshape(-1), torch.arange(3 * E), n, 3 * E, _old_corners(tri, n))
    for got, want in zip(ops._csr(tri.reshape(-1), None, n, 3 * E), _old_corners(tri, n)):  # col = None: col[i] = i
        assert torch.equal(got, want) and got.dtype == torch.int32


def test_csr_builder_on_random_tables():
    g = torch.Generator().manual_seed(5)
    for n_rows, n_cols, m in ((1, 1, 7), (5, 3, 40), (17, 64, 300)):
        row = torch.randint(0, n_rows, (m,), generator=g)
        col = torch.randint(0, n_cols, (m,), generator=g)
        ptr, out = ops._csr(row, col, n_rows, n_cols)
        want = _csr_loop(row, col, n_rows)
        assert ptr.tolist() == want[0] and out.tolist() == want[1]


# ---------------------------------------------------------------------------------------------------------------
def test_validators_refuse_what_is_not_a_gpu_tensor():
    for fn in (lambda t: ops._chk(t, "x", (None, 3)), lambda t: ops._chk_index(t, "x", 3)):
        with pytest.raises(TypeError, match="x must be a tensor"):
            fn([[0, 1, 2]])
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.TetGrid(torch.zeros(4, 3), torch.zeros(1, 4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.MeshTopology(torch.zeros(1, 3, dtype=torch.int32), 3)


def test_wildcard_shapes_and_index_tables(monkeypatch):
    monkeypatch.setattr(ops, "_chk_gpu", lambda t, name: None)  # the shape / dtype rules, on CPU tensors
    x = torch.zeros(5, 3)
    assert ops._chk(x, "x", (None, 3)) is x and ops._chk(x, "x", (5, None)) is x and ops._chk(x, "x") is x
    assert ops._chk(x.t(), "x", (3, None)).is_contiguous()
    for shape in ((None, 2), (4, None), (None,), (None, 3, None)):
        with pytest.raises(ValueError, match=r"x has shape \(5, 3\), expected \(.*\*.*\)"):
            ops._chk(x, "x", shape)
    with pytest.raises(ValueError, match=r"expected \(4, 3\)"):
        ops._chk(x, "x", (4, 3))
    with pytest.raises(TypeError):
        ops._chk(x.double(), "x", (None, 3))
    for dtype in (torch.int32, torch.int64):
        t = torch.zeros(5, 3, dtype=dtype)
        assert ops._chk_index(t, "t", 3) is t and ops._chk_index(t, "t", 3, 5) is t
        assert ops._chk_index(t[:0], "t", 3, 0).shape == (0, 3)
        with pytest.raises(ValueError, match="t has 5 rows, expected 4"):
            ops._chk_index(t, "t", 3, 4)
        with pytest.raises(TypeError, match="t must be"):
            ops._chk_index(t, "t", 4)
        with pytest.raises(TypeError):
            ops._chk_index(t.reshape(-1), "t", 3)
    for dtype in (torch.float32, torch.int16, torch.uint8):
        with pytest.raises(TypeError, match="int32 / int64"):
            ops._chk_index(torch.zeros(5, 3, dtype=dtype), "t", 3)


def test_range_and_size_checks():
    for lo, hi in ((-1, 3), (0, 4)):
        with pytest.raises(ValueError, match=r"t holds an index outside \[0, 4\)"):
            ops._chk_range("t", lo, hi, 4)
    ops._chk_range("t", 0, 3, 4)
    ops._chk_range("t", 0, -1, 4)  # an empty table
    ops._chk_range("t", 0, -1, 0)
    a = torch.tensor([[3, 0, 2], [1, 1, 0]], dtype=torch.int32)
    b = torch.tensor([[7, 5, 6]], dtype=torch.int32)
    assert ops._minmax(a).tolist() == [0, 3]
    assert ops._minmax(a, b, a[:0]).tolist() == [0, 3, 5, 7, 0, -1]
    ops._chk_size("mesh", V=_lib.TT_MESH_MAX_ITEMS, T=0)
    with pytest.raises(ValueError, match=r"mesh: V=3, T=268435457 \(limit TT_MESH_MAX_ITEMS = 268435456\)"):
        ops._chk_size("mesh", V=3, T=_lib.TT_MESH_MAX_ITEMS + 1)
