"""Differentiable rasterization on the HIP kernels of tt_raster.hip and tt_texture.hip (include/tt_abi.h, "rasterize /
interpolate / antialias" and "texture sampling"): the drop-in for nvdiffrast's `rasterize`, `interpolate`, `texture`
and `antialias` in instance and range mode, and `RasterizerContext`, a drop-in for threestudio's
`NVDiffRasterizerContext` (threestudio/utils/rasterize.py).

    from triplaneturbo_amd.raster import RasterizerContext
    ctx = RasterizerContext("cuda", device)
    pos = ctx.vertex_transform(v_pos, mvp)                 # (B,V,4) clip space
    rast, _ = ctx.rasterize(pos, tri, (H, W))              # (B,H,W,4) = (u, v, z/w, tri + 1)
    feat, _ = ctx.interpolate(pos, rast, tri)              # (B,H,W,4)
    uv, _ = ctx.interpolate(v_tex, rast, t_tex_idx)        # (B,H,W,2)
    color = ctx.texture(map_Kd[None], uv, boundary_mode="clamp")   # (B,H,W,3); tex (B or 1,TH,TW,C)
    img = ctx.antialias(color, rast, pos, tri)             # (B,H,W,C)

Range mode renders different meshes in one call: one vertex buffer (V,4), per image a (first, count) range of tri.

    pk = pack_ranges([pos_a, pos_b], [tri_a, tri_b])       # pos (Va+Vb,4), tri (Ta+Tb,3), ranges (2,2) on the CPU
    rast, _ = ctx.rasterize(pk.pos, pk.tri, (H, W), ranges=pk.ranges)   # (2,H,W,4), ids index pk.tri
    feat, _ = ctx.interpolate(pk.pos, rast, pk.tri)        # a 2-D attr (V,C) is shared by the images
    img = ctx.antialias(color, rast, pk.pos, pk.tri)       # gradients come back (V,4)

texture() filters "nearest" and "linear" with boundary "wrap", "clamp" and "zero" and is differentiable w.r.t. the
texture and the UVs.  No mipmaps: no rast_db / diff_attrs, no uv_da / mip_level_bias / mip / max_mip_level, no
"linear-mipmap-*" filters and no cube maps (each raises NotImplementedError); minification is the caller's
(triplaneturbo_amd.viewer supersamples).  There is no CPU path."""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .ops import _chk, _launch, _workspace, sort_face_edges

Tensor = torch.Tensor
MAX_TRIS = _lib.TT_RAST_MAX_TRIS  # tri + 1 is stored as a float


def _check_tri(tri: Tensor) -> Tensor:
    tri = _chk(tri, "tri", (None, 3), torch.int32)
    if tri.shape[0] >= MAX_TRIS:
        raise ValueError(f"{tri.shape[0]} triangles: at most {MAX_TRIS - 1} (the id channel is a float)")
    return tri


def edge_topology(tri: Tensor, n_vertices: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The edge -> triangles table antialias() needs (tt_abi.h "topology"): edge_ofs (3T,2) int32 = (first, count)
    of the group of triangle edge 3t + k (vertices k, (k+1) % 3) in the sorted edge list, edge_tri (3T) int32 = the
    triangle of each sorted entry.  Depends on tri only (torch sort as plumbing): build it once per mesh."""
    n = int(n_vertices) if n_vertices is not None else int(tri.max().item()) + 1 if tri.shape[0] else 0
    return sort_face_edges(tri, n).antialias_tables()


class _RasterizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, H, W):
        B, V, _ = pos.shape
        T = tri.shape[0]
        ws = _workspace("tt_rast_workspace_bytes", B, T, H, W, device=pos.device)
        rast = torch.empty((B, H, W, 4), device=pos.device, dtype=torch.float32)
        _launch("tt_rast_fwd", pos, tri, B, V, T, H, W, ws, rast, label="tt_rast_fwd")
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rast):
        pos, tri, rast = ctx.saved_tensors
        if g_rast is None or not ctx.needs_input_grad[0]:
            return None, None, None, None
        B, V, _ = pos.shape
        H, W = rast.shape[1], rast.shape[2]
        g_pos = torch.empty_like(pos)
        _launch("tt_rast_bwd", pos, tri, rast, g_rast.contiguous(), B, V, tri.shape[0], H, W, g_pos)
        return g_pos, None, None, None


class _RasterizeRangeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, tri, ranges, H, W):
        V, T, B = pos.shape[0], tri.shape[0], ranges.shape[0]
        ranges_dev = ranges.to(pos.device)
        ws = _workspace("tt_rast_range_workspace_bytes", B, int(ranges[:, 1].sum()), H, W, device=pos.device)
        rast = torch.empty((B, H, W, 4), device=pos.device, dtype=torch.float32)
        # `ranges` (host memory) is read during the call only
        _launch("tt_rast_range_fwd", pos, tri, ranges_dev, ranges, B, V, T, H, W, ws, rast, label="tt_rast_range_fwd")
        ctx.save_for_backward(pos, tri, rast)
        return rast

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rast):
        pos, tri, rast = ctx.saved_tensors
        if g_rast is None or not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        B, H, W, _ = rast.shape
        g_pos = torch.empty_like(pos)
        _launch("tt_rast_range_bwd", pos, tri, rast, g_rast.contiguous(), B, pos.shape[0], tri.shape[0], H, W, g_pos)
        return g_pos, None, None, None, None


def _check_ranges(ranges, n_tri: int) -> Tensor:
    if not isinstance(ranges, torch.Tensor) or ranges.is_cuda or ranges.dtype != torch.int32:
        raise ValueError("ranges must be an int32 CPU tensor (B,2) of (first triangle, triangle count) rows")
    if ranges.dim() != 2 or ranges.shape[1] != 2 or ranges.shape[0] < 1:
        raise ValueError(f"ranges must be (B,2) with B >= 1, got {tuple(ranges.shape)}")
    ranges = ranges.contiguous()
    for b, (first, count) in enumerate(ranges.tolist()):
        if first < 0 or count < 0 or first + count > n_tri:
            raise ValueError(f"ranges[{b}] = (first {first}, count {count}) leaves the {n_tri} triangles of tri")
    return ranges


def rasterize(pos: Tensor, tri: Tensor, resolution: Union[int, Tuple[int, int]],
              ranges: Optional[Tensor] = None) -> Tensor:
    """rast (B,H,W,4) = (u, v, z/w, tri + 1), 0 where empty.  pos (B,V,4) clip space, tri (T,3) int32.
    Differentiable w.r.t. pos through u, v (dr.rasterize without rast_db).
    Range mode: pos (V,4) and `ranges`, an int32 CPU tensor (B,2) of (first triangle, triangle count) per image;
    the id channel indexes the whole tri."""
    H, W = (resolution, resolution) if isinstance(resolution, int) else (int(resolution[0]), int(resolution[1]))
    if H < 1 or W < 1:
        raise ValueError(f"resolution must be positive, got {(H, W)}")
    pos = _chk(pos, "pos")
    if pos.dim() == 2 or ranges is not None:
        if pos.dim() != 2 or pos.shape[-1] != 4:
            raise ValueError(f"ranges go with a 2-D pos (V,4) (range mode), got pos {tuple(pos.shape)}")
        if ranges is None:
            raise ValueError("a 2-D pos (V,4) selects range mode and needs ranges (B,2)")
        tri = _check_tri(tri)
        return _RasterizeRangeFn.apply(pos, tri, _check_ranges(ranges, tri.shape[0]), H, W)
    if pos.dim() != 3 or pos.shape[-1] != 4 or pos.shape[0] < 1:
        raise ValueError(f"pos must be (B,V,4) with B >= 1, got {tuple(pos.shape)}")
    return _RasterizeFn.apply(pos, _check_tri(tri), H, W)


class _InterpolateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, tri):
        A, V, C = attr.shape
        B, H, W, _ = rast.shape
        out = torch.empty((B, H, W, C), device=attr.device, dtype=torch.float32)
        _launch("tt_interp_fwd", attr, A, rast, tri, B, V, tri.shape[0], H, W, C, out)
        ctx.save_for_backward(attr, rast, tri)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        attr, rast, tri = ctx.saved_tensors
        A, V, C = attr.shape
        B, H, W, _ = rast.shape
        g_attr = torch.empty_like(attr) if ctx.needs_input_grad[0] else None
        g_rast = torch.empty_like(rast) if ctx.needs_input_grad[1] else None
        if g_attr is None and g_rast is None:
            return None, None, None
        _launch("tt_interp_bwd", attr, A, rast, tri, g_out.contiguous(), B, V, tri.shape[0], H, W, C, g_attr, g_rast)
        return g_attr, g_rast, None


def interpolate(attr: Tensor, rast: Tensor, tri: Tensor, rast_db=None, diff_attrs=None) -> Tensor:
    """out (B,H,W,C) = u a0 + v a1 + (1-u-v) a2 (0 where empty); attr (B,V,C) or (1,V,C) (broadcast over views).
    Differentiable w.r.t. attr and rast (its u, v channels).  rast_db / diff_attrs are not supported.
    A 2-D attr (V,C) means (1,V,C): with a range-mode rast (global ids) that is range-mode interpolation."""
    if rast_db is not None or diff_attrs is not None:
        raise NotImplementedError("rast_db / diff_attrs (attribute derivatives for mip texturing) are not supported")
    attr = _chk(attr, "attr")
    rast = _chk(rast, "rast", (None, None, None, 4))
    if attr.dim() == 2:
        attr = attr[None]
    if attr.dim() != 3 or attr.shape[0] not in (1, rast.shape[0]) or attr.shape[2] < 1:
        raise ValueError(f"attr must be (B,V,C) or (1,V,C) with C >= 1, got {tuple(attr.shape)} for B={rast.shape[0]}")
    return _InterpolateFn.apply(attr, rast, _check_tri(tri))


_TEX_FILTERS = {"nearest": _lib.TT_TEX_FILTER_NEAREST, "linear": _lib.TT_TEX_FILTER_LINEAR}
_TEX_BOUNDARIES = {"wrap": _lib.TT_TEX_BOUNDARY_WRAP, "clamp": _lib.TT_TEX_BOUNDARY_CLAMP,
                   "zero": _lib.TT_TEX_BOUNDARY_ZERO}
_TEX_MIP_OPTIONS = ("uv_da", "mip_level_bias", "mip", "max_mip_level")


class _TextureFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, filt, boundary):
        N, TH, TW, C = tex.shape
        B, H, W, _ = uv.shape
        out = torch.empty((B, H, W, C), device=tex.device, dtype=torch.float32)
        _launch("tt_tex_fwd", tex, N, uv, B, H, W, TH, TW, C, filt, boundary, out)
        ctx.save_for_backward(tex, uv)
        ctx.modes = (filt, boundary)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        tex, uv = ctx.saved_tensors
        N, TH, TW, C = tex.shape
        B, H, W, _ = uv.shape
        g_tex = torch.empty_like(tex) if ctx.needs_input_grad[0] else None
        g_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        if g_tex is None and g_uv is None:
            return None, None, None, None
        _launch("tt_tex_bwd", tex, N, uv, g_out.contiguous(), B, H, W, TH, TW, C, *ctx.modes, g_tex, g_uv)
        return g_tex, g_uv, None, None


def texture(tex: Tensor, uv: Tensor, filter_mode: str = "linear", boundary_mode: str = "wrap", **kw) -> Tensor:
    """out (B,H,W,C) = tex (B,TH,TW,C) or (1,TH,TW,C) (shared by the images) sampled at uv (B,H,W,2) (dr.texture
    without mipmaps; tt_abi.h "texture sampling"): u along the width, v along the height, texel (i, j) centred at
    ((i + 0.5) / TW, (j + 0.5) / TH).  filter_mode "nearest" | "linear", boundary_mode "wrap" | "clamp" | "zero".
    Differentiable w.r.t. tex and uv (grad_uv is 0 under "nearest"); a non-finite uv gives 0 and no gradient.
    The mipmap filters, "cube" and uv_da / mip_level_bias / mip / max_mip_level raise NotImplementedError."""
    for k, v in kw.items():
        if k not in _TEX_MIP_OPTIONS:
            raise TypeError(f"texture() got an unexpected keyword argument {k!r}")
        if v is not None:
            raise NotImplementedError(f"{k}: mipmapped texture sampling is not supported (supersample instead)")
    if filter_mode in ("linear-mipmap-nearest", "linear-mipmap-linear"):
        raise NotImplementedError(f"filter_mode {filter_mode!r}: mipmapped texture sampling is not supported "
                                  f"(supersample instead)")
    if boundary_mode == "cube":
        raise NotImplementedError("boundary_mode 'cube': cube maps are not supported")
    if filter_mode not in _TEX_FILTERS:
        raise ValueError(f"filter_mode must be one of {sorted(_TEX_FILTERS)}, got {filter_mode!r}")
    if boundary_mode not in _TEX_BOUNDARIES:
        raise ValueError(f"boundary_mode must be one of {sorted(_TEX_BOUNDARIES)}, got {boundary_mode!r}")
    tex = _chk(tex, "tex")
    uv = _chk(uv, "uv", (None, None, None, 2))
    if tex.dim() != 4 or tex.shape[0] not in (1, uv.shape[0]) or min(tex.shape[1:]) < 1:
        raise ValueError(f"tex must be (B,TH,TW,C) or (1,TH,TW,C) with TH, TW, C >= 1, got {tuple(tex.shape)} for "
                         f"B={uv.shape[0]}")
    return _TextureFn.apply(tex, uv, _TEX_FILTERS[filter_mode], _TEX_BOUNDARIES[boundary_mode])


class _AntialiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, rast, pos, tri, edge_ofs, edge_tri):
        B, H, W, C = color.shape
        V = pos.shape[-2]
        out = torch.empty_like(color)
        _launch("tt_aa_fwd" if pos.dim() == 3 else "tt_aa_range_fwd", color, rast, pos, tri, edge_ofs, edge_tri, B, V,
                tri.shape[0], H, W, C, out)
        ctx.save_for_backward(color, rast, pos, tri, edge_ofs, edge_tri)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        color, rast, pos, tri, edge_ofs, edge_tri = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
            return (None,) * 6
        B, H, W, C = color.shape
        V = pos.shape[-2]
        g_color = torch.empty_like(color)
        g_pos = torch.empty_like(pos) if ctx.needs_input_grad[2] else None
        _launch("tt_aa_bwd" if pos.dim() == 3 else "tt_aa_range_bwd", color, rast, pos, tri, edge_ofs, edge_tri,
                g_out.contiguous(), B, V, tri.shape[0], H, W, C, g_color, g_pos)
        return (g_color if ctx.needs_input_grad[0] else None), None, g_pos, None, None, None


def antialias(color: Tensor, rast: Tensor, pos: Tensor, tri: Tensor,
              topology: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
    """Analytic silhouette antialiasing (Laine et al. 2020, section 4.3; tt_abi.h "antialias"): color (B,H,W,C),
    rast from rasterize(pos, tri), pos (B,V,4).  Differentiable w.r.t. color and pos (none to rast).  `topology`
    = edge_topology(tri), computed here when not given.  Range mode: pos (V,4), rast from rasterize(pos, tri, ranges=..);
    the topology is that of the whole tri, so only meshes that share vertices see each other's edges."""
    color = _chk(color, "color")
    rast = _chk(rast, "rast", (None, None, None, 4))
    pos = _chk(pos, "pos")
    tri = _check_tri(tri)
    if color.dim() != 4 or tuple(color.shape[:3]) != tuple(rast.shape[:3]):
        raise ValueError(f"color must be (B,H,W,C) matching rast {tuple(rast.shape)}, got {tuple(color.shape)}")
    if pos.dim() == 2 and pos.shape[1] != 4 or pos.dim() != 2 and (
            pos.dim() != 3 or pos.shape[0] != rast.shape[0] or pos.shape[2] != 4):
        raise ValueError(f"pos must be (B,V,4) with B={rast.shape[0]}, or (V,4) in range mode, got {tuple(pos.shape)}")
    if topology is None:
        topology = edge_topology(tri, pos.shape[-2])
    edge_ofs = _chk(topology[0], "edge_ofs", (tri.shape[0] * 3, 2), dtype=torch.int32)
    edge_tri = _chk(topology[1], "edge_tri", (tri.shape[0] * 3,), dtype=torch.int32)
    return _AntialiasFn.apply(color, rast, pos, tri, edge_ofs, edge_tri)


class PackedRanges(NamedTuple):
    """pack_ranges' result: the arguments of a range-mode rasterize / interpolate / antialias."""
    pos: Tensor                  # (sum V_i, 4): torch.cat of the pieces, so autograd reaches every one
    tri: Tensor                  # (sum T_i, 3) int32, piece i's indices shifted by vertex_offsets[i]
    ranges: Tensor               # (B,2) int32 on the CPU: (tri_offsets[i], T_i)
    vertex_offsets: List[int]    # first row of piece i in pos
    tri_offsets: List[int]       # first row of piece i in tri
    topology: Optional[Tuple[Tensor, Tensor]]  # edge_topology(tri, sum V_i), when the pieces' tables were given


def pack_ranges(pos_list: Sequence[Tensor], tri_list: Sequence[Tensor],
                topologies: Optional[Sequence[Tuple[Tensor, Tensor]]] = None) -> PackedRanges:
    """One image per piece: B clip-space buffers (V_i,4) and B triangle lists (T_i,3) (the same tensor may appear
    several times) as one range-mode batch.  With the pieces' edge_topology tables, the table of the concatenation is
    assembled by offsetting them (no sort): the pieces share no vertices and the sorted edge list is ordered by
    (lower, higher) vertex index and stable, so it is the pieces' lists one after the other."""
    n = len(pos_list)
    if n < 1 or n != len(tri_list) or (topologies is not None and len(topologies) != n):
        raise ValueError("pack_ranges needs B >= 1 positions, B triangle lists (and B topologies, when given)")
    v_ofs, t_ofs, tris, rows = [], [], [], []
    nv = nt = 0
    for pos, tri in zip(pos_list, tri_list):
        if pos.dim() != 2 or pos.shape[1] != 4 or tri.dim() != 2 or tri.shape[1] != 3:
            raise ValueError(f"pack_ranges takes pieces pos (V,4), tri (T,3), got {tuple(pos.shape)}, {tuple(tri.shape)}")
        v_ofs.append(nv)
        t_ofs.append(nt)
        tris.append(tri.int() + nv)
        rows.append((nt, tri.shape[0]))
        nv += pos.shape[0]
        nt += tri.shape[0]
    if nt >= MAX_TRIS:
        raise ValueError(f"{nt} triangles: at most {MAX_TRIS - 1} (the id channel is a float)")
    topology = None
    if topologies is not None:
        edge_ofs = torch.cat([torch.stack([ofs[:, 0] + 3 * t0, ofs[:, 1]], 1) for (ofs, _), t0 in zip(topologies, t_ofs)])
        edge_tri = torch.cat([et + t0 for (_, et), t0 in zip(topologies, t_ofs)])
        topology = (edge_ofs, edge_tri)
    return PackedRanges(torch.cat(list(pos_list)), torch.cat(tris), torch.tensor(rows, dtype=torch.int32).reshape(-1, 2),
                        v_ofs, t_ofs, topology)


class RasterizerContext:
    """threestudio's NVDiffRasterizerContext (threestudio/utils/rasterize.py) on the HIP kernels: same methods,
    signatures and tuple returns.  `context_type` ("gl" / "cuda") is accepted and ignored."""

    def __init__(self, context_type: str = "cuda", device: Optional[torch.device] = None) -> None:
        self.device = device
        self.context_type = context_type
        self._topo_tri = None  # the tri tensor the cached table was built from (held, so it cannot be recycled)
        self._topo_key = None
        self._topo = None

    def vertex_transform(self, verts: Tensor, mvp_mtx: Tensor) -> Tensor:
        verts_homo = torch.cat([verts, torch.ones([verts.shape[0], 1]).to(verts)], dim=-1)
        return torch.matmul(verts_homo, mvp_mtx.permute(0, 2, 1))

    def rasterize(self, pos: Tensor, tri: Tensor, resolution: Union[int, Tuple[int, int]],
                  ranges: Optional[Tensor] = None):
        """(rast, None): there is no rast_db.  A 2-D pos with `ranges` is range mode."""
        return rasterize(pos.float(), tri.int(), resolution, ranges=ranges), None

    def rasterize_one(self, pos: Tensor, tri: Tensor, resolution: Union[int, Tuple[int, int]]):
        rast, _ = self.rasterize(pos[None, ...], tri, resolution)
        return rast[0], None

    def antialias(self, color: Tensor, rast: Tensor, pos: Tensor, tri: Tensor,
                  topology: Optional[Tuple[Tensor, Tensor]] = None) -> Tensor:
        tri = tri.int()
        if topology is None:  # one cached table: consecutive calls on the same mesh reuse it
            key = (tri._version, pos.shape[-2])
            if tri is not self._topo_tri or key != self._topo_key:
                self._topo_tri, self._topo_key, self._topo = tri, key, edge_topology(tri, pos.shape[-2])
            topology = self._topo
        return antialias(color.float(), rast, pos.float(), tri, topology)

    def interpolate(self, attr: Tensor, rast: Tensor, tri: Tensor, rast_db=None, diff_attrs=None):
        """(out, empty tensor): there are no attribute derivatives."""
        out = interpolate(attr.float(), rast, tri.int(), rast_db=rast_db, diff_attrs=diff_attrs)
        return out, torch.empty(0, device=out.device)

    def interpolate_one(self, attr: Tensor, rast: Tensor, tri: Tensor, rast_db=None, diff_attrs=None):
        return self.interpolate(attr[None, ...], rast, tri, rast_db, diff_attrs)

    def texture(self, tex: Tensor, uv: Tensor, filter_mode: str = "linear", boundary_mode: str = "wrap", **kw) -> Tensor:
        return texture(tex.float(), uv.float(), filter_mode=filter_mode, boundary_mode=boundary_mode, **kw)
