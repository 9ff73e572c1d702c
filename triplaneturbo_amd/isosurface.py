"""Mesh extraction: the reference's DiffMarchingCubeHelper / isosurface / colorize_mesh
(triplaneturbo_executable/utils/mesh_exporter.py:22-183) on the HIP marching cubes (ops.marching_cubes, tt_mc_* in
include/tt_abi.h) instead of the CUDA-only `diso.DiffMC`.

    from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface, colorize_mesh
    helper = DiffMarchingCubeHelper(160).to("cuda")
    meshes = isosurface(space_cache, geometry.forward_field, helper)
    meshes = colorize_mesh(space_cache, geometry.export, meshes, torch.sigmoid)

MarchingTetrahedraHelper (threestudio/models/isosurface.py:126-327, isosurface_method "mt") runs on the HIP marching
tetrahedra (ops.marching_tets, tt_mt_*); kuhn_tet_grid / write_tet_grid make the tet grid the reference loads from a file.

Same signatures and behaviour as the reference; Mesh keeps what these functions and their users touch plus the
training system's regularisers and outlier removal, and threestudio's UV unwrap (`unwrap_uv`, lazy `v_tex` /
`t_tex_idx`) on the HIP axis-projection atlas (ops.uv_atlas) instead of xatlas, and its tangents (`v_tng`, and `v_tng_tex`
per UV vertex; ops.mesh_tangents).  File output (OBJ + MTL +
texture) is triplaneturbo_amd.export: `multiprompt-mesh-exporter` and `save_obj`."""
from __future__ import annotations

from functools import cached_property
from typing import Any, Callable, Dict, List, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

Tensor = torch.Tensor


def scale_tensor(dat: Tensor, inp_scale, tgt_scale) -> Tensor:
    """triplaneturbo_executable/utils/general_utils.py:12-25"""
    if inp_scale is None:
        inp_scale = (0, 1)
    if tgt_scale is None:
        tgt_scale = (0, 1)
    if isinstance(tgt_scale, Tensor):
        assert dat.shape[-1] == tgt_scale.shape[-1]
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    dat = dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]
    return dat


def cache_batch_device(space_cache: Any) -> Tuple[int, torch.device]:
    """Prompts and device of a space cache: a (P,6,32,R,R) tensor, or the hyper net's Dict[str, List[Tensor]]."""
    first = space_cache if torch.is_tensor(space_cache) else next(iter(space_cache.values()))[0]
    return first.shape[0], first.device


def prompt_slice(space_cache: Any, i: int) -> Any:
    """Prompt i's slice of a space cache, batch dimension kept: a view of a tensor, lists of views of a dict."""
    if torch.is_tensor(space_cache):
        return space_cache[i:i + 1]
    return {k: [w[i:i + 1] for w in v] for k, v in space_cache.items()}


def obj_uv(v_tex: Tensor) -> Tensor:
    """The UVs an OBJ file carries for v_tex (N,2) fp32, back in the internal orientation: (u, 1 - (1 - v)) with both
    subtractions rounded to fp32.  save_obj writes `vt u (1 - v)` with 1 - v in fp32, which costs a v below 0.5 up to
    2^-25; viewer.load_obj undoes the flip, so its v_tex is exactly obj_uv(the exporter's v_tex), and obj_uv is
    idempotent (one of the two subtractions is always exact).  Mesh.v_tng_tex is built on these."""
    v = v_tex.detach()
    return torch.stack([v[:, 0], 1.0 - (1.0 - v[:, 1])], dim=1)


class Mesh:
    """The part of threestudio's Mesh (threestudio/models/mesh.py; triplaneturbo_executable/utils/mesh.py is its
    subset) that mesh extraction, colouring, the mesh renderer and the training system use: positions, int32
    triangles, vertex colours, area-weighted vertex normals (mesh.py:114-140), edges, the normal-consistency and
    Laplacian regularisers and remove_outlier, the last three on the tt_mesh_* kernels (include/tt_abi.h)."""

    def __init__(self, v_pos: Tensor, t_pos_idx: Tensor, **kwargs) -> None:
        self.v_pos = v_pos
        self.t_pos_idx = t_pos_idx
        self._v_nrm: Optional[Tensor] = None
        self._v_rgb: Optional[Tensor] = None
        self._v_tex: Optional[Tensor] = None
        self._t_tex_idx: Optional[Tensor] = None
        self._v_tng: Optional[Tensor] = None
        self._v_tng_tex: Optional[Tensor] = None
        self.uv_info: Optional[Dict[str, Any]] = None  # ops.uv_atlas's info of the last unwrap
        self.extras: Dict[str, Any] = {}
        for k, v in kwargs.items():
            self.add_extra(k, v)

    def add_extra(self, k, v) -> None:
        self.extras[k] = v

    @property
    def v_nrm(self) -> Tensor:
        if self._v_nrm is None:
            self._v_nrm = self._compute_vertex_normal()
        return self._v_nrm

    @property
    def v_rgb(self) -> Optional[Tensor]:
        return self._v_rgb

    @property
    def v_tex(self) -> Tensor:
        """(Vt,2) fp32 UVs in [0,1], unwrapped on first use with the defaults (mesh.py:112-116)."""
        if self._v_tex is None:
            self._v_tex, self._t_tex_idx = self._unwrap_uv()
        return self._v_tex

    @property
    def t_tex_idx(self) -> Tensor:
        """(T,3) int32 UV-vertex ids, face f = face f of t_pos_idx (mesh.py:118-122; the reference's are int64)."""
        if self._t_tex_idx is None:
            self._v_tex, self._t_tex_idx = self._unwrap_uv()
        return self._t_tex_idx

    @property
    def v_tng(self) -> Tensor:
        """(V,3) unit tangents per position vertex, perpendicular to v_nrm (mesh.py:162-205; ops.mesh_tangents,
        group "pos"); unwraps the UVs on first use, as v_tex does.  Computed from detached positions, UVs and normals:
        it never requires grad.  Where the reference yields NaN (an unreferenced vertex, a tangent parallel to the
        normal) it holds a fixed unit vector perpendicular to the normal."""
        if self._v_tng is None:
            self._v_tng = ops.mesh_tangents(self.v_pos, self.t_pos_idx, self.v_tex, self.t_tex_idx, self.v_nrm, "pos")
        return self._v_tng

    @property
    def v_tng_tex(self) -> Tensor:
        """(Vt,3) unit tangents per UV vertex (ops.mesh_tangents, group "tex"): the corners of one UV vertex only, so
        tangents split at chart seams, perpendicular to v_nrm of the UV vertex's position vertex.  What the normal-map
        bake and the viewer interpolate through t_tex_idx.  Detached like v_tng: it never requires grad.

        Built on obj_uv(v_tex), the UVs as an OBJ file carries them, not on v_tex itself: the frame a normal map is
        encoded in has to be the one a reader of the files rebuilds.  A simplified mesh has UV triangles well under a
        texel wide, whose tangents amplify the 2^-25 that the file's `1 - v` costs by 1 / (UV edge length), to 2e-5 of
        tangent at a 256^2 atlas; with obj_uv the exported mesh and the loaded one feed the kernel the same numbers
        (up to v_nrm, whose scatter_add may differ by an ulp from run to run)."""
        if self._v_tng_tex is None:
            self._v_tng_tex = ops.mesh_tangents(self.v_pos, self.t_pos_idx, obj_uv(self.v_tex), self.t_tex_idx,
                                                self.v_nrm, "tex")
        return self._v_tng_tex

    def _unwrap_uv(self, xatlas_chart_options: Optional[dict] = None, xatlas_pack_options: Optional[dict] = None,
                   texture_size: Optional[int] = None, method: Optional[str] = "axis") -> Tuple[Tensor, Tensor]:
        """mesh.py:207-242 on the HIP axis-projection atlas (ops.uv_atlas, include/tt_abi.h "UV atlas and texture
        fill").  Of xatlas's options only PackOptions.padding (texels around every chart, default 2 as the exporter's
        inpaint radius) and PackOptions.resolution (the atlas size; else texture_size, else 1024) mean something here;
        any other option raises NotImplementedError naming it.  `method`: "axis" (None means the same), or "lscm" for
        conformal maps of the same charts (include/tt_abi.h, "conformal UV charts")."""
        method = ops.uv_method(method)
        chart_opts, pack_opts = dict(xatlas_chart_options or {}), dict(xatlas_pack_options or {})
        for k in chart_opts:
            raise NotImplementedError(f"xatlas chart option {k!r}: the atlas is axis-projection charts, not xatlas")
        for k in pack_opts:
            if k not in ("padding", "resolution"):
                raise NotImplementedError(f"xatlas pack option {k!r}: only 'padding' and 'resolution' are supported")
        N = int(pack_opts.get("resolution") or texture_size or 1024)
        v_tex, t_tex_idx, info = ops.uv_atlas(self.v_pos.detach(), self.t_pos_idx, self.topology, texture_size=N,
                                              padding=int(pack_opts.get("padding", 2)), method=method)
        self.uv_info = info
        return v_tex, t_tex_idx

    def unwrap_uv(self, xatlas_chart_options: Optional[dict] = None, xatlas_pack_options: Optional[dict] = None,
                  texture_size: Optional[int] = None, method: Optional[str] = "axis") -> None:
        """mesh.py:244-249; `texture_size` (the exporter's) sizes the atlas unless the pack options name a resolution;
        `method` as in _unwrap_uv."""
        self._v_tex, self._t_tex_idx = self._unwrap_uv(xatlas_chart_options, xatlas_pack_options, texture_size, method)
        self._v_tng = self._v_tng_tex = None  # tangents belong to the UVs they were built from

    @property
    def requires_grad(self) -> bool:
        return self.v_pos.requires_grad

    @cached_property
    def topology(self) -> ops.MeshTopology:
        """The mesh's one connectivity object; depends on t_pos_idx and V only, so it is built once."""
        return ops.mesh_topology(self.t_pos_idx, self.v_pos.shape[0])

    @property
    def edges(self) -> Tensor:
        """(E,2) unique sorted vertex pairs of the face edges in lexicographic order, self pairs of degenerate faces
        included, dtype of t_pos_idx: the values and order of the reference's _compute_edges (mesh.py:255-267)."""
        return self.topology.edges

    def set_vertex_color(self, v_rgb: Tensor) -> None:
        assert v_rgb.shape[0] == self.v_pos.shape[0]
        self._v_rgb = v_rgb

    def normal_consistency(self) -> Tensor:
        """mean over the edges of 1 - cos(n_a, n_b) of the vertex normals (mesh.py:269-274); differentiable to v_pos
        through v_nrm."""
        return ops.mesh_normal_consistency_loss(self.v_nrm, self.topology)

    def laplacian(self) -> Tensor:
        """mean row norm of the uniform Laplacian applied to v_pos (mesh.py:276-308), without the sparse matrix."""
        return ops.mesh_laplacian_loss(self.v_pos, self.topology)

    def remove_outlier(self, outlier_n_faces_threshold: Union[int, float]) -> Mesh:
        """mesh.py:31-95: drop the connected components with fewer faces than the threshold (a float t: int(faces of
        the largest component * t); an int: as given) and the vertices they leave unreferenced; a differentiable
        mesh comes back as it is (self).  A new Mesh that inherits extras.  Two deliberate differences from the
        reference's trimesh path: vertices are identified by index (trimesh's process=True would also merge
        bitwise-equal positions), and the output keeps the original relative order of vertices and faces (trimesh
        concatenates component by component).  A mesh without faces comes back as it is (the reference raises)."""
        if self.requires_grad:
            return self
        if self.t_pos_idx.shape[0] == 0:
            return self
        v_pos, t_pos_idx = ops.mesh_remove_small_components(self.v_pos, self.t_pos_idx, outlier_n_faces_threshold,
                                                            self.topology)
        clean_mesh = Mesh(v_pos, t_pos_idx)
        if len(self.extras) > 0:
            clean_mesh.extras = self.extras
        return clean_mesh

    @cached_property
    def triangle_grid(self) -> ops.TriangleGrid:
        """The mesh's uniform grid for closest-point queries, built on first use from the detached positions (a Mesh
        whose v_pos is replaced afterwards needs a new Mesh, as for `topology`)."""
        return ops.TriangleGrid(self.v_pos, self.t_pos_idx)

    def closest_point(self, points: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """(d2, face, bary) of the closest point of this mesh to every row of points (N,3): ops.mesh_closest_point on
        `triangle_grid` (include/tt_abi.h "point-to-mesh distance").  Not differentiable; ops.point_mesh_distance2 is."""
        return ops.mesh_closest_point(points, self.triangle_grid)

    @cached_property
    def winding_tree(self) -> ops.WindingTree:
        """The mesh's dipole octree for winding-number queries, built on first use from the detached positions (as
        `triangle_grid`: a Mesh whose v_pos is replaced afterwards needs a new Mesh)."""
        return ops.WindingTree(self.v_pos, self.t_pos_idx)

    def winding_number(self, points: Tensor, beta: float = 2.0, exact: bool = False, cell_order: bool = False) -> Tensor:
        """w (N,) fp32 of this mesh about every row of points (N,3): ops.mesh_winding_number on `winding_tree`
        (include/tt_abi.h "winding number"); 1 inside, 0 outside for the outward orientation the extractors give."""
        return ops.mesh_winding_number(points, self.winding_tree, beta=beta, exact=exact, cell_order=cell_order)

    def contains(self, points: Tensor) -> Tensor:
        """(N,) bool: which rows of points (N,3) lie inside this mesh (winding number above 0.5)."""
        return ops.mesh_contains(points, self.winding_tree)

    def signed_distance(self, points: Tensor) -> Tensor:
        """Signed distance (N,) of every row of points (N,3) to this mesh, negative inside (ops.mesh_signed_distance on
        `triangle_grid` and `winding_tree`); differentiable w.r.t. points and v_pos."""
        return ops.mesh_signed_distance(points, self.v_pos, self.t_pos_idx, tg=self.triangle_grid,
                                        tree=self.winding_tree)

    def sdf_grid(self, resolution: int = 128, band: float = 3.0, bounds=None) -> Tuple[Tensor, Dict[str, Any]]:
        """(level (R,R,R), info) of ops.mesh_sdf_grid on `triangle_grid` and `winding_tree`: this mesh's signed
        distance on a regular grid, clamped to +-band cells (include/tt_abi.h "mesh to SDF grid").  Not
        differentiable."""
        ops._chk_sdf_grid_args(resolution, band, bounds is None)  # before the grid and the tree are built
        return ops.mesh_sdf_grid(self.v_pos, self.t_pos_idx, resolution, band=band, bounds=bounds,
                                 tg=self.triangle_grid, tree=self.winding_tree)

    def solidify(self, resolution: int = 256, band: float = 3.0, offset: float = 0.0, keep_cavities: bool = False,
                 project: bool = False) -> Mesh:
        """A watertight copy through the field: `sdf_grid`, ops.marching_cubes at isovalue `offset`, the vertices
        mapped back through the grid's lo and h, then the connected components (tt_mesh_components); unless
        `keep_cavities`, every component whose signed volume (summed in fp64 in face order) is negative -- the wall of
        a closed cavity -- is dropped, and nothing else is.  `offset` (same units as v_pos; positive thickens,
        negative erodes) needs |offset| <= tau - h = (band - 1) h so that the surface stays inside the band, else
        ValueError.  project=True, for offset == 0 only, moves every vertex to its closest point on this mesh.

        For a closed input the result is a closed manifold (every directed edge once, its reverse once), outward
        oriented, with every vertex within h of this surface: the signed distance is 1-Lipschitz, so a grid edge with a
        sign change has |d0| + |d1| <= h and its interpolated point lies within (|d0| + |d1| + h) / 2 <= h.  Interior
        surfaces and overlaps of closed components disappear (the winding number is above 1/2 there).  An open input is
        closed along winding number 1/2, which is behaviour, not a guarantee.  Features thinner than h vanish.  Vertex
        colours, when this mesh carries them, are interpolated at the closest point of this mesh.  A new Mesh that
        inherits extras, with extras["solidify"] = {resolution, h, band_corners, components_dropped, faces}; it never
        requires grad."""
        ops._chk_sdf_grid_args(resolution, band, True)
        if isinstance(offset, bool) or not isinstance(offset, (int, float)) or not np.isfinite(offset):
            raise ValueError(f"offset must be a finite number, got {offset!r}")
        if band < 1.0:
            raise ValueError(f"solidify needs band >= 1 (|offset| <= tau - h = (band - 1) h), got band {band}")
        if project and offset != 0:
            raise ValueError("project=True moves vertices onto this mesh: it goes with offset == 0 only")
        level, info = self.sdf_grid(resolution, band)
        h, tau = info["h"], info["tau"]
        if abs(offset) > tau - h:
            raise ValueError(f"|offset| = {abs(offset)} is beyond tau - h = {tau - h} (band {band}, h {h}): "
                             f"use a wider band or a coarser grid")
        v_pos, tri = ops.marching_cubes(level, isovalue=float(offset))
        v_pos = v_pos * ((resolution - 1) * h) + info["lo"]
        dropped = 0
        if tri.shape[0] > 0:
            labels = ops.mesh_face_components(ops.mesh_topology(tri, v_pos.shape[0]))
            if not keep_cavities:
                p = v_pos[tri.long()].double()
                vol = ((p[:, 0] * torch.cross(p[:, 1], p[:, 2], dim=-1)).sum(-1) / 6.0).cpu().numpy()
                _, comp = np.unique(labels.cpu().numpy(), return_inverse=True)
                cavity = np.bincount(comp, weights=vol) < 0.0  # one pass in face order: a fixed summation order
                dropped = int(cavity.sum())
                if dropped:
                    keep = torch.from_numpy(~cavity[comp]).to(tri.device)
                    tri = tri[keep]
                    used = torch.zeros(v_pos.shape[0], dtype=torch.bool, device=tri.device)
                    used[tri.long().reshape(-1)] = True
                    new_id = torch.cumsum(used, 0, dtype=torch.int32) - 1
                    v_pos, tri = v_pos[used], new_id[tri.long()].contiguous()
        mesh = Mesh(v_pos.contiguous(), tri)
        mesh.extras = dict(self.extras)
        mesh.extras["solidify"] = {"resolution": resolution, "h": h, "band_corners": info["band_corners"],
                                   "components_dropped": dropped, "faces": int(tri.shape[0])}
        if v_pos.shape[0] > 0 and (project or self._v_rgb is not None):
            _, face, bary = self.closest_point(mesh.v_pos)
            corner_ids = self.t_pos_idx.long()[face.long()]
            if project:
                mesh.v_pos = (bary[:, :, None] * self.v_pos.detach()[corner_ids]).sum(1)
            if self._v_rgb is not None:
                corners = self._v_rgb.detach()[corner_ids]
                mesh._v_rgb = (bary.to(corners.dtype)[:, :, None] * corners).sum(1)
        return mesh

    def ray_cast(self, origins: Tensor, dirs: Tensor, t_max: float = float("inf"),
                 cell_order: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
        """(t, face, bary) of the closest hit of every ray origins[i] + t dirs[i] with this mesh, 0 <= t <= t_max:
        ops.mesh_ray_cast on `triangle_grid` (include/tt_abi.h "ray casting").  A miss is (inf, -1, 0).  Not
        differentiable; ops.ray_mesh_depth is."""
        return ops.mesh_ray_cast(origins, dirs, self.triangle_grid, t_max=t_max, cell_order=cell_order)

    def occluded(self, origins: Tensor, dirs: Tensor, t_max: float = float("inf")) -> Tensor:
        """(N,) bool: whether ray i meets this mesh at 0 <= t <= t_max (ops.mesh_ray_occluded on `triangle_grid`)."""
        return ops.mesh_ray_occluded(origins, dirs, self.triangle_grid, t_max=t_max)

    def ambient_occlusion(self, points: Optional[Tensor] = None, normals: Optional[Tensor] = None, n_rays: int = 64,
                          max_distance: Optional[float] = None, bias: Optional[float] = None) -> Tensor:
        """Ambient occlusion (N,) fp32 in [0,1], 1 = open, of `points` with `normals` against this mesh
        (ops.mesh_ambient_occlusion on `triangle_grid`); with no points given, per vertex with v_nrm."""
        if points is None:
            if normals is not None:
                raise ValueError("normals without points: give both or neither")
            points, normals = self.v_pos.detach(), self.v_nrm.detach()
        elif normals is None:
            raise ValueError("points without normals: give both or neither")
        return ops.mesh_ambient_occlusion(points, normals, self.triangle_grid, n_rays=n_rays,
                                          max_distance=max_distance, bias=bias)

    def _bbox_diagonal(self) -> Tensor:
        v = self.v_pos.detach()
        return (v.amax(0) - v.amin(0)).norm()

    def distance_to(self, other: Mesh, spacing: Optional[float] = None, _cache: Optional[dict] = None) -> Dict[str, Any]:
        """How far this mesh (a) and `other` (b) lie apart, measured on surface samples: both surfaces are sampled so
        that every surface point is within `spacing` of a sample (ops.mesh_surface_samples; default: the larger
        bounding-box diagonal / 200) and every sample is sent to the other mesh (ops.mesh_closest_point).  Returns
        {a_to_b, b_to_a: {max, mean, rms, argmax_point} over the samples -- NOT area-weighted: a face contributes by
        its lattice, shared edges more than once --, hausdorff: the larger of the two maxima, spacing, n_samples:
        (S_a, S_b)}.  Distance to a surface is 1-Lipschitz, so the true symmetric Hausdorff distance of the two
        surfaces is at most hausdorff + spacing (and at least hausdorff)."""
        if not isinstance(other, Mesh):
            raise TypeError(f"other must be a Mesh, got {type(other).__name__}")
        if spacing is None:
            spacing = float(torch.maximum(self._bbox_diagonal(), other._bbox_diagonal())) / 200.0
        spacing = ops._chk_spacing(spacing)
        cache = {} if _cache is None else _cache  # simplify(max_error=): one side's samples and grid serve every probe
        sides = []
        for key, m in (("a", self), ("b", other)):
            if key not in cache:
                cache[key] = (ops.mesh_surface_samples(m.v_pos, m.t_pos_idx, spacing)[0], m.triangle_grid)
            sides.append(cache[key])
        (sa, ga), (sb, gb) = sides
        a_to_b, b_to_a = ops.one_sided_distance(sa, gb), ops.one_sided_distance(sb, ga)
        return {"a_to_b": a_to_b, "b_to_a": b_to_a, "hausdorff": max(a_to_b["max"], b_to_a["max"]),
                "spacing": spacing, "n_samples": (sa.shape[0], sb.shape[0])}

    def _simplify_max_error(self, max_error: float) -> Mesh:
        """The bisection of simplify(max_error=): the smallest grid in 2..256 the bisection finds whose result passes
        hausdorff + spacing <= max_error, spacing = max_error / 4, both directions measured per probe."""
        spacing = max_error / 4.0
        cache: dict = {}
        lo, hi, best = 2, 257, None  # every grid below lo failed; hi passed (257: none has yet)
        while lo < hi:
            mid = (lo + hi) // 2
            probe = ops.mesh_simplify(self.v_pos, self.t_pos_idx, mid)
            if probe[2]["unchanged"]:
                return self
            err = None
            if probe[1].shape[0] > 0:
                cache.pop("a", None)
                err = Mesh(probe[0], probe[1]).distance_to(self, spacing, _cache=cache)
            if err is not None and err["hausdorff"] + spacing <= max_error:
                hi, best = mid, (probe, err)
            else:
                lo = mid + 1
        if best is None:
            return self
        (v_pos, t_pos_idx, info), err = best
        mesh = Mesh(v_pos, t_pos_idx)
        mesh.extras = dict(self.extras)
        mesh.extras["simplify"] = {k: info[k] for k in ("grid", "cell", "n_clusters", "vertex_map")}
        mesh.extras["simplify"]["error"] = dict(err, max_error=max_error)
        return mesh

    def simplify(self, grid: Optional[int] = None, target_faces: Optional[int] = None,
                 max_error: Optional[float] = None) -> Mesh:
        """A low-poly copy for export: vertex clustering on a grid^3 lattice with quadric-error placement
        (ops.mesh_simplify; include/tt_abi.h "mesh simplification").  Exactly one of `grid` (2..1024), `target_faces`
        and `max_error` must be given; target_faces bisects over grids 2..256 for the largest one whose result has at
        most that many faces (at most 8 runs; the grid-2 result when even that has more).  A new Mesh that inherits
        extras, with extras["simplify"] = {grid, cell, n_clusters, vertex_map}; the mesh itself comes back when it has
        no vertices, faces or extent.  The result never requires grad.  Not guaranteed manifold.

        max_error (a finite positive length) bounds the deviation instead: with spacing = max_error / 4 the full mesh
        is sampled and gridded once, and grids 2..256 are bisected (8 runs) for the coarsest whose result r has
        r.distance_to(self)["hausdorff"] + spacing <= max_error, both directions measured per probe -- so the symmetric
        Hausdorff distance between the two surfaces is at most max_error.  The returned mesh is always one whose check
        passed (the mesh itself if none did) and carries the measurement as a fifth key, extras["simplify"]["error"] =
        that distance_to dict (a = the result, b = this mesh) plus max_error.  The bisection assumes that the deviation
        falls as the grid grows, as target_faces assumes for the face count: the result meets the budget but need not
        be the coarsest possible.  A max_error so small that its sampling exceeds TT_DIST_MAX_SAMPLES is a ValueError."""
        if sum(x is not None for x in (grid, target_faces, max_error)) != 1:
            raise ValueError("simplify: give exactly one of grid, target_faces and max_error")
        if max_error is not None:
            try:
                ok = not isinstance(max_error, bool) and 0.0 < float(max_error) < float("inf")
            except (TypeError, ValueError):
                ok = False
            if not ok:
                raise ValueError(f"max_error must be a finite positive number, got {max_error!r}")
            if 0 in (self.v_pos.shape[0], self.t_pos_idx.shape[0]):
                return self
            return self._simplify_max_error(float(max_error))
        if grid is not None:
            result = ops.mesh_simplify(self.v_pos, self.t_pos_idx, grid)
        else:
            if isinstance(target_faces, bool) or not isinstance(target_faces, int) or target_faces < 1:
                raise ValueError(f"target_faces must be a positive int, got {target_faces!r}")
            lo, hi = 1, 256  # lo = 1: no grid fits; every grid above hi has been seen to give too many faces
            result = None
            while lo < hi:
                mid = (lo + hi + 1) // 2
                probe = ops.mesh_simplify(self.v_pos, self.t_pos_idx, mid)
                if probe[2]["unchanged"]:
                    return self
                if probe[1].shape[0] <= target_faces:
                    lo, result = mid, probe
                else:
                    hi = mid - 1
                    if hi == 1:
                        result = probe  # grid 2 still has more: its result is returned
        v_pos, t_pos_idx, info = result
        if info["unchanged"]:
            return self
        mesh = Mesh(v_pos, t_pos_idx)
        mesh.extras = dict(self.extras)
        mesh.extras["simplify"] = {k: info[k] for k in ("grid", "cell", "n_clusters", "vertex_map")}
        return mesh

    def decimate(self, target_faces: int) -> Mesh:
        """A low-poly copy with this mesh's topology: rounds of parallel quadric edge collapses down to at most
        target_faces (>= 4) faces (ops.mesh_decimate; include/tt_abi.h "mesh decimation").  A closed 2-manifold stays
        one, with the same genus and number of components, and no face flips; vertices on a boundary or a non-manifold
        edge stay where they are.  A new Mesh that inherits extras, with extras["decimate"] = ops.mesh_decimate's info
        ({target_faces, n_rounds, stalled, n_locked, vertex_map, unchanged}); a mesh that is empty, small enough or
        admits no collapse comes back with its own tensors.  The result never requires grad."""
        v_pos, t_pos_idx, info = ops.mesh_decimate(self.v_pos, self.t_pos_idx, target_faces)
        mesh = Mesh(v_pos, t_pos_idx)
        mesh.extras = dict(self.extras)
        mesh.extras["decimate"] = info
        return mesh

    def remesh(self, edge_length: Optional[float] = None, target_faces: Optional[int] = None,
               iterations: Optional[int] = None) -> Mesh:
        """A copy with near-equilateral triangles of one size on this mesh's surface: isotropic remeshing (split the
        long edges, collapse the short ones, flip towards valence 6, relax tangentially and pull back onto this
        surface; ops.mesh_remesh; include/tt_abi.h "isotropic remeshing").  Exactly one of `edge_length` (the target
        edge length L) and `target_faces` must be given; target_faces sets L = sqrt(4 A / (sqrt(3) target_faces)) with
        A this mesh's area, the edge at which equilateral triangles cover A with that many faces -- the face count of
        the result FOLLOWS this estimate, it is not exact.  `iterations` defaults to TT_REMESH_DEFAULT_ITERATIONS.  A
        closed 2-manifold stays one, with the same genus and number of components, no face flips, vertices on a
        boundary or a non-manifold edge stay where they are, and no edge of the result is longer than 4/3 L (unless
        extras["remesh"]["split_capped"]).  Short edges whose collapse is blocked remain, sharp features are not
        preserved, nothing is differentiable.  A new Mesh that inherits extras, with extras["remesh"] =
        ops.mesh_remesh's info; vertex colours, when this mesh carries them, are interpolated at the closest point of
        this mesh to every new vertex (source_face / source_bary).  A mesh that is empty or that nothing changes comes
        back with its own tensors.  The result never requires grad."""
        if (edge_length is None) == (target_faces is None):
            raise ValueError("remesh: give exactly one of edge_length and target_faces")
        if target_faces is not None:
            if isinstance(target_faces, bool) or not isinstance(target_faces, int) or target_faces < 1:
                raise ValueError(f"target_faces must be a positive int, got {target_faces!r}")
            p = self.v_pos.detach()[self.t_pos_idx.long()]
            area = 0.5 * float(torch.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0], dim=-1).norm(dim=-1).double().sum())
            if not area > 0.0:
                raise ValueError("remesh(target_faces=): the mesh has no area; give edge_length")
            edge_length = ops.remesh_edge_length(area, target_faces)
        v_pos, t_pos_idx, info = ops.mesh_remesh(self.v_pos, self.t_pos_idx, edge_length, iterations)
        mesh = Mesh(v_pos, t_pos_idx)
        mesh.extras = dict(self.extras)
        mesh.extras["remesh"] = info
        if self._v_rgb is not None:
            if info["unchanged"]:
                mesh._v_rgb = self._v_rgb
            else:
                corners = self._v_rgb.detach()[self.t_pos_idx.long()[info["source_face"].long()]]  # (V',3,C)
                mesh._v_rgb = (info["source_bary"].to(corners.dtype)[:, :, None] * corners).sum(1)
        return mesh

    def _compute_vertex_normal(self) -> Tensor:
        i0, i1, i2 = (self.t_pos_idx[:, c].long() for c in range(3))
        v0, v1, v2 = self.v_pos[i0, :], self.v_pos[i1, :], self.v_pos[i2, :]
        face_normals = torch.cross(v1 - v0, v2 - v0, dim=-1)
        v_nrm = torch.zeros_like(self.v_pos)
        v_nrm.scatter_add_(0, i0[:, None].repeat(1, 3), face_normals)
        v_nrm.scatter_add_(0, i1[:, None].repeat(1, 3), face_normals)
        v_nrm.scatter_add_(0, i2[:, None].repeat(1, 3), face_normals)
        v_nrm = torch.where((v_nrm * v_nrm).sum(-1, keepdim=True) > 1e-20, v_nrm,
                            torch.as_tensor([0.0, 0.0, 1.0]).to(v_nrm))
        return F.normalize(v_nrm, dim=1)


class IsosurfaceHelper(nn.Module):
    points_range: Tuple[float, float] = (0, 1)

    @property
    def grid_vertices(self) -> Tensor:
        raise NotImplementedError


class DiffMarchingCubeHelper(IsosurfaceHelper):
    """mesh_exporter.py:29-75 with the HIP marching cubes in place of diso.DiffMC."""

    def __init__(self, resolution: int, point_range: Tuple[float, float] = (0, 1)) -> None:
        super().__init__()
        self.resolution = resolution
        self.points_range = point_range
        self.mc_func: Callable = ops.marching_cubes
        self._grid_vertices: Optional[Tensor] = None
        self.register_buffer("_dummy", torch.zeros(0, dtype=torch.float32), persistent=False)

    @property
    def grid_vertices(self) -> Tensor:
        if self._grid_vertices is None:
            # on the CPU, like the reference (very large resolutions); callers move them
            x, y, z = (torch.linspace(*self.points_range, self.resolution) for _ in range(3))
            x, y, z = torch.meshgrid(x, y, z, indexing="ij")
            verts = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
            verts = verts * (self.points_range[1] - self.points_range[0]) + self.points_range[0]
            self._grid_vertices = verts
        return self._grid_vertices

    def forward(self, level: Tensor, deformation: Optional[Tensor] = None, isovalue=0.0) -> Mesh:
        R = self.resolution
        level = level.view(R, R, R)
        if deformation is not None:
            deformation = deformation.view(R, R, R, 3)
        v_pos, t_pos_idx = self.mc_func(level, deformation, isovalue=isovalue)
        v_pos = v_pos * (self.points_range[1] - self.points_range[0]) + self.points_range[0]
        return Mesh(v_pos=v_pos, t_pos_idx=t_pos_idx)


_KUHN_PATHS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2))  # three even, three odd permutations


def kuhn_tet_grid(resolution: int) -> Tuple[Tensor, Tensor]:
    """A tetrahedral grid on the unit cube for MarchingTetrahedraHelper: `vertices` (R^3,3) fp32, the R points per axis
    of DiffMarchingCubeHelper(R).grid_vertices in its order (index i R^2 + j R + k = (x_i, y_j, z_k)), and `indices`
    (6 (R-1)^3, 4) int64, six Kuhn tetrahedra per cell: one per order in which a path from the cell's corner (i,j,k) to
    (i+1,j+1,k+1) takes its x, y and z step.  All cells are cut alike, so neighbouring cells agree on the diagonal of
    the face they share and the grid is conforming.  Every tet is positively oriented, det[v1-v0, v2-v0, v3-v0] > 0
    (the odd step orders list their two middle corners the other way round): with that the reference's triangle table
    (threestudio/models/isosurface.py:141-169) yields closed surfaces whose normals point toward level > 0.  CPU
    tensors.  The reference loads such grids from load/tets/{R}_tets.npz, files it does not ship."""
    R = int(resolution)
    if R < 2:
        raise ValueError(f"kuhn_tet_grid needs at least 2 points per axis, got {R}")
    x = torch.linspace(0, 1, R)
    vertices = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), dim=-1).reshape(-1, 3)
    c = torch.arange(R - 1)
    origin = (c[:, None, None] * R * R + c[None, :, None] * R + c[None, None, :]).reshape(-1, 1)
    stride = (R * R, R, 1)
    corners = []
    for n, (a, b, d) in enumerate(_KUHN_PATHS):
        v1, v2 = stride[a], stride[a] + stride[b]
        if n >= 3:  # an odd permutation: swap the middle corners for a positive volume
            v1, v2 = v2, v1
        corners.append([0, v1, v2, stride[0] + stride[1] + stride[2]])
    indices = (origin[:, None, :] + torch.tensor(corners)[None, :, :]).reshape(-1, 4)
    return vertices, indices


def write_tet_grid(path: str, resolution: int) -> None:
    """kuhn_tet_grid(resolution) as an npz file in the reference's format (arrays `vertices`, `indices`,
    isosurface.py:179-189), e.g. load/tets/{R}_tets.npz."""
    import numpy as np
    vertices, indices = kuhn_tet_grid(resolution)
    np.savez_compressed(path, vertices=vertices.numpy(), indices=indices.numpy())


class MarchingTetrahedraHelper(IsosurfaceHelper):
    """threestudio/models/isosurface.py:126-327 on the HIP marching tetrahedra (ops.marching_tets, tt_mt_* in
    include/tt_abi.h): same attributes, same meshes (vertices, faces and their order), same extras.  The grid comes from
    `tets_path` (the reference's npz: `vertices`, `indices`), from a ready ops.TetGrid, or, with neither, from
    kuhn_tet_grid(resolution).  The static tables (ops.TetGrid) are built on the first use on the GPU.

    center_indices / border_indices, (n,1) int64: the vertex sets of the mesh renderer's empty-field fix-up, chosen by
    position so that any grid works (the reference indexes an R^3 lattice whatever the file holds).  With the bounding
    box of the vertices and h = its extent / (R - 1) per axis: the border is every vertex with a coordinate closer than
    1.5 h to a face of the box; the centre is the one vertex nearest to box_min + (R // 2) h (lowest index on a tie).
    On an R^3 lattice these are the two outer layers and the vertex (R//2, R//2, R//2), the reference's sets."""

    def __init__(self, resolution: int, tets_path: Optional[str] = None, point_range: Tuple[float, float] = (0, 1),
                 tet_grid: Optional[ops.TetGrid] = None) -> None:
        super().__init__()
        self.resolution = resolution
        self.tets_path = tets_path
        self.points_range = point_range
        self._tet_grid = tet_grid
        if tet_grid is not None:
            if tets_path is not None:
                raise ValueError("give tets_path or tet_grid, not both")
            vertices, indices = tet_grid.vertices, tet_grid.tets.long()
        elif tets_path is not None:
            import numpy as np
            tets = np.load(tets_path)
            vertices, indices = torch.from_numpy(tets["vertices"]).float(), torch.from_numpy(tets["indices"]).long()
        else:
            vertices, indices = kuhn_tet_grid(resolution)
        self.register_buffer("_grid_vertices", vertices, persistent=False)
        self.register_buffer("indices", indices, persistent=False)
        lo, hi = vertices.amin(0), vertices.amax(0)
        h = (hi - lo) / max(resolution - 1, 1)
        border = ((vertices - lo < 1.5 * h) | (hi - vertices < 1.5 * h)).any(dim=1)
        centre = (vertices - (lo + (resolution // 2) * h)).square().sum(dim=1).argmin()
        self.register_buffer("border_indices", torch.nonzero(border), persistent=False)
        self.register_buffer("center_indices", centre.reshape(1, 1), persistent=False)
        self._all_edges: Optional[Tensor] = None

    def normalize_grid_deformation(self, grid_vertex_offsets: Tensor) -> Tensor:
        # half a tet is about 1 / resolution (isosurface.py:193-200)
        return (self.points_range[1] - self.points_range[0]) / self.resolution * torch.tanh(grid_vertex_offsets)

    @property
    def grid_vertices(self) -> Tensor:
        return self._grid_vertices

    @property
    def tet_grid(self) -> ops.TetGrid:
        if self._tet_grid is None or self._tet_grid.tets.device != self.indices.device:
            self._tet_grid = ops.TetGrid(self._grid_vertices, self.indices)
            self._all_edges = None
        return self._tet_grid

    @property
    def all_edges(self) -> Tensor:
        if self._all_edges is None:
            self._all_edges = self.tet_grid.edges.long()
        return self._all_edges

    def forward(self, level: Tensor, deformation: Optional[Tensor] = None) -> Mesh:
        if deformation is not None:
            grid_vertices = self.grid_vertices + self.normalize_grid_deformation(deformation)
        else:
            grid_vertices = self.grid_vertices
        v_pos, t_pos_idx = ops.marching_tets(grid_vertices, level, self.tet_grid)
        return Mesh(v_pos=v_pos, t_pos_idx=t_pos_idx, grid_vertices=grid_vertices, tet_edges=self.all_edges,
                    grid_level=level, grid_deformation=deformation)


def isosurface(space_cache: Any, forward_field: Callable, isosurface_helper: Callable) -> List[Mesh]:
    """mesh_exporter.py:78-141: query the field on the helper's grid (mapped to the hard-coded [-1, 1] bbox), one
    mesh per prompt, |p| - 1 in place of a field without a level set, vertices mapped back to [-1, 1]."""
    batch_size, device = cache_batch_device(space_cache)
    points = scale_tensor(isosurface_helper.grid_vertices.to(device), isosurface_helper.points_range, [-1, 1])
    sdf_batch, deformation_batch = forward_field(points[None, ...].expand(batch_size, -1, -1), space_cache)
    mesh_list = []
    for index in range(sdf_batch.shape[0]):
        sdf = sdf_batch[index]
        deformation = None if deformation_batch is None else deformation_batch[index]
        if torch.all(sdf > 0) or torch.all(sdf < 0):
            print("All sdf values are positive or negative, no isosurface")
            sdf = torch.norm(points, dim=-1) - 1
        mesh = isosurface_helper(sdf, deformation)
        mesh.v_pos = scale_tensor(mesh.v_pos, isosurface_helper.points_range, [-1, 1])
        mesh_list.append(mesh)
    return mesh_list


def colorize_mesh(space_cache: Any, export_fn: Callable, mesh_list: List[Mesh], activation: Callable) -> List[Mesh]:
    """mesh_exporter.py:143-183: per mesh, the prompt's slice of the space cache, export_fn on the vertices, and
    activation(features) as the vertex colours."""
    for i, mesh in enumerate(mesh_list):
        points = mesh.v_pos[None, ...]
        out = export_fn(points, prompt_slice(space_cache, i))
        if "features" in out:
            mesh._v_rgb = activation(out["features"].squeeze(0))
    return mesh_list
