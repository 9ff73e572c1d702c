"""Range mode of the rasterizer, the parts that need no GPU: raster.pack_ranges (vertex offsets, ranges, the edge
topology assembled by offsetting the pieces' tables) and the C ABI's additive range-mode entries."""
import os
import re

import torch

from triplaneturbo_amd import _lib, raster

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANGE_ENTRIES = ["tt_rast_range_workspace_bytes", "tt_rast_range_fwd", "tt_rast_range_bwd", "tt_aa_range_fwd",
                 "tt_aa_range_bwd"]

TETRA = torch.tensor([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], dtype=torch.int32)
OCTA = torch.tensor([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]],
                    dtype=torch.int32)


def test_pack_ranges_offsets_ranges_and_topology():
    tris = [TETRA, OCTA, TETRA]  # the tetrahedron twice (the same tensor object), the octahedron once
    n_vert = [4, 6, 4]
    pos = [torch.full((n, 4), float(i)) for i, n in enumerate(n_vert)]
    topo = [raster.edge_topology(t, n) for t, n in zip(tris, n_vert)]
    pk = raster.pack_ranges(pos, tris, topo)
    assert pk.vertex_offsets == [0, 4, 10] and pk.tri_offsets == [0, 4, 12]
    assert pk.ranges.dtype == torch.int32 and not pk.ranges.is_cuda
    assert pk.ranges.tolist() == [[0, 4], [4, 8], [12, 4]]
    assert pk.pos.shape == (14, 4) and pk.tri.shape == (16, 3) and pk.tri.dtype == torch.int32
    for i, (first, count) in enumerate(pk.ranges.tolist()):
        assert torch.equal(pk.tri[first:first + count] - pk.vertex_offsets[i], tris[i])
        assert (pk.pos[pk.vertex_offsets[i]:pk.vertex_offsets[i] + n_vert[i]] == float(i)).all()
    ref_ofs, ref_tri = raster.edge_topology(pk.tri, 14)
    assert torch.equal(pk.topology[0], ref_ofs) and pk.topology[0].dtype == torch.int32
    assert torch.equal(pk.topology[1], ref_tri) and pk.topology[1].dtype == torch.int32
    assert raster.pack_ranges(pos, tris).topology is None


def test_pack_ranges_keeps_autograd_to_every_piece():
    pos = [torch.randn(4, 4, requires_grad=True), torch.randn(6, 4, requires_grad=True)]
    pk = raster.pack_ranges(pos, [TETRA, OCTA])
    (pk.pos * torch.arange(10.0)[:, None]).sum().backward()
    assert torch.equal(pos[0].grad, torch.arange(4.0)[:, None].expand(4, 4))
    assert torch.equal(pos[1].grad, torch.arange(4.0, 10.0)[:, None].expand(6, 4))


def test_header_declares_the_range_entries_and_keeps_its_version():
    text = open(os.path.join(ROOT, "include", "tt_abi.h")).read()
    for name in RANGE_ENTRIES:
        assert re.search(r"^(int|int64_t) %s\(" % name, text, re.M), name
        assert name in _lib.SYMBOLS
    assert int(re.search(r"^#define TT_ABI_VERSION (\d+)", text, re.M).group(1)) == 17
    protos, _ = _lib._parse_abi()
    # the forward takes the ranges twice (device, host) behind pos and tri
    assert len(protos["tt_rast_range_fwd"][1]) == len(protos["tt_rast_fwd"][1]) + 2
    for a, b in (("tt_rast_range_bwd", "tt_rast_bwd"), ("tt_aa_range_fwd", "tt_aa_fwd"), ("tt_aa_range_bwd", "tt_aa_bwd")):
        assert protos[a] == protos[b]  # same argument list; pos / grad_pos are (V,4)
