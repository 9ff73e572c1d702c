"""`generative-space-mesh-rasterize-renderer`: the reference's first training renderer
(custom/triplaneturbo/models/renderers/generative_space_mesh_rasterize_renderer.py) on this package's pieces: the
grid query `geometry.forward_field`, the HIP marching cubes (isosurface.DiffMarchingCubeHelper, "diffmc") or marching
tetrahedra (isosurface.MarchingTetrahedraHelper, "mt"), the HIP rasterizer
(raster.RasterizerContext in place of nvdiffrast) and the per-pixel `geometry(points, output_normal=True)` decode.
Same registry name, Config fields, forward signature, per-prompt loop and output keys as the reference; the image
plumbing between the kernels (normal rotation, lerps, disparity) stays torch, as in the reference."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Union

import torch
import torch.nn.functional as F

from . import ops, raster
from .isosurface import (DiffMarchingCubeHelper, MarchingTetrahedraHelper, Mesh, cache_batch_device, prompt_slice,
                         scale_tensor)
from .registry import BaseModule, C, register

Tensor = torch.Tensor


class _GBuffer(NamedTuple):
    """What the raster stage hands one prompt's shading: (n_view,H,W,.) images of its views."""
    rast: Tensor              # (u, v, z/w, id); only `id > 0` is used behind the raster stage
    depth: Tensor             # clip w
    normal: Tensor            # interpolated v_nrm, not normalized
    pos: Optional[Tensor]     # interpolated v_pos (render_rgb)


class _PreAA(NamedTuple):
    """An output image that still has to go through antialias (per prompt, or all prompts' at once)."""
    img: Tensor
    detach: bool  # rendered from a fixed-up empty field

    def resolve(self, aa: Callable[[Tensor], Tensor]) -> Tensor:
        out = aa(self.img)
        return out.detach() if self.detach else out


@register("generative-space-mesh-rasterize-renderer")
class GenerativeSpaceMeshRasterizeRenderer(BaseModule):
    @dataclass
    class Config(BaseModule.Config):
        radius: float = 1.0  # Renderer.Config
        context_type: str = "cuda"
        isosurface_resolution: int = 128
        isosurface_remove_outliers: bool = False
        isosurface_outlier_n_faces_threshold: Union[int, float] = 0.01
        isosurface_method: str = "mt"  # "mt" or "mc-cpu" or "diffmc" ("diffmc" and "mt" are built here)
        enable_bg_rays: bool = False
        normal_direction: str = "camera"  # "camera" or "world" or "front"
        sdf_grad_shrink: Any = 1.0
        def_grad_shrink: Any = 1.0
        allow_empty_flag: bool = True

    cfg: Config

    def configure(self, geometry, material, background, tet_grid=None) -> None:
        """`tet_grid` (isosurface_method="mt" only): the tetrahedral grid, an ops.TetGrid (e.g. of
        isosurface.kuhn_tet_grid(R)) or the path of an npz file in the reference's format; without it the reference's
        load/tets/{R}_tets.npz is used when that file exists."""
        c = self.cfg
        R = c.isosurface_resolution
        if c.isosurface_method == "diffmc":
            helper = DiffMarchingCubeHelper(R)
        elif c.isosurface_method == "mt":
            default_path = f"load/tets/{R}_tets.npz"  # reference :72-77
            if isinstance(tet_grid, ops.TetGrid):
                helper = MarchingTetrahedraHelper(R, tet_grid=tet_grid)
            elif tet_grid is not None:
                helper = MarchingTetrahedraHelper(R, os.fspath(tet_grid))
            elif os.path.exists(default_path):
                helper = MarchingTetrahedraHelper(R, default_path)
            else:
                raise NotImplementedError(
                    f"isosurface_method='mt' needs a tetrahedral grid and {default_path} does not exist: pass "
                    f"tet_grid=ops.TetGrid(*isosurface.kuhn_tet_grid({R})) (tensors on the GPU) or the path of an npz "
                    f"file with `vertices` and `indices` (isosurface.write_tet_grid writes one) to the renderer")
        else:
            raise NotImplementedError(f"isosurface_method={c.isosurface_method!r}: 'diffmc' (the reference training "
                                      f"config) and 'mt' are built; 'mc-cpu' needs a CPU helper")
        if c.isosurface_remove_outliers:
            raise NotImplementedError("isosurface_remove_outliers=True (Mesh.remove_outlier) is not built")
        if getattr(material, "requires_tangent", False):
            raise NotImplementedError("materials that need tangents (Mesh.v_tng) are not supported")
        self.geometry, self.material, self.background = geometry, material, background
        self.ctx = raster.RasterizerContext(c.context_type, None)
        self.geometry.isosurface = self.isosurface  # overwrite the geometry's (reference :74)
        self.isosurface_helper = helper
        self.sdf_grad_shrink = C(c.sdf_grad_shrink, 0, 0)
        self.def_grad_shrink = C(c.def_grad_shrink, 0, 0)
        self.empty_flag = False
        # an extra the reference does not have (so not a Config field): in training, rasterize, interpolate and
        # antialias every prompt's views in one range-mode call each instead of once per prompt
        self.batch_prompts = False
        # follow InstantMesh (reference :97-107): a positive shell and a negative centre for an empty field
        if c.isosurface_method == "mt":  # by position, for any tet grid (MarchingTetrahedraHelper's docstring)
            self.center_indices, self.border_indices = helper.center_indices, helper.border_indices
            return
        v = torch.zeros([R] * 3, dtype=torch.bool)
        v[R // 2:R // 2 + 1, R // 2:R // 2 + 1, R // 2:R // 2 + 1] = True
        self.center_indices = torch.nonzero(v.reshape(-1))
        v = torch.zeros([R] * 3, dtype=torch.bool)
        v[:2, :, :] = True
        v[-2:, :, :] = True
        v[:, :2, :] = True
        v[:, -2:, :] = True
        v[:, :, :2] = True
        v[:, :, -2:] = True
        self.border_indices = torch.nonzero(v.reshape(-1))

    # ------------------------------------------------------------------------------------------
    def forward(self, mvp_mtx: Tensor, camera_positions: Tensor, light_positions: Tensor, height: int, width: int,
                noise: Optional[Tensor] = None, space_cache: Optional[Tensor] = None,
                text_embed: Optional[Tensor] = None, render_rgb: bool = True,
                rays_d_rasterize: Optional[Tensor] = None, camera_distances: Optional[Tensor] = None,
                c2w: Optional[Tensor] = None, **kwargs) -> Dict[str, Any]:
        """reference :110-404.  mvp_mtx (B,4,4) with B = P * views; space_cache (P,6,32,R,R)."""
        batch_size = mvp_mtx.shape[0]
        batch_size_space_cache = text_embed.shape[0] if text_embed is not None else batch_size
        num_views_per_batch = batch_size // batch_size_space_cache

        if space_cache is None:
            space_cache = self.geometry.generate_space_cache(styles=noise, text_embed=text_embed)

        mesh_list = self.isosurface(space_cache)

        if self.empty_flag:  # detach everything rendered from a fixed-up empty field
            is_empty = True
            self.empty_flag = False
        else:
            is_empty = False

        def keep(t: Tensor) -> Tensor:
            return t.detach() if is_empty else t

        batched = self.batch_prompts and self.training
        if batched:
            gbuffers, aa_all = self._raster_batched(mesh_list, mvp_mtx, num_views_per_batch, height, width, render_rgb)

        def shade(batch_idx: int, mesh: Mesh, g: _GBuffer) -> Dict[str, Any]:
            """One prompt's images from its G-buffer; a _PreAA entry still wants its antialias."""
            sl = slice(batch_idx * num_views_per_batch, (batch_idx + 1) * num_views_per_batch)
            depth = g.depth
            mask = g.rast[..., 3:] > 0
            if mask.sum() == 0:  # no visible points: the first view's pixels stand in (reference :160-163)
                mask[:1] = True

            # disparity, as required by RichDreamer
            sqrt3 = torch.sqrt(3 * torch.ones(1, device=camera_distances.device))
            far = (camera_distances + sqrt3)[sl, None, None, None]
            near = (camera_distances - sqrt3)[sl, None, None, None]
            disparity_tmp = depth.clamp_max(far)
            disparity_norm = ((far - disparity_tmp) / (far - near)).clamp(0, 1)
            disparity_norm = torch.lerp(torch.zeros_like(depth), disparity_norm, mask.float())

            out = {"opacity": _PreAA(mask.float(), False) if not is_empty else mask.detach(), "mesh": mesh,
                   "depth": keep(depth), "disparity": _PreAA(disparity_norm, is_empty)}

            gb_normal = F.normalize(g.normal, dim=-1)
            gb_normal_aa = torch.lerp(torch.zeros_like(gb_normal), (gb_normal + 1.0) / 2.0, mask.float())
            out["comp_normal"] = _PreAA(gb_normal_aa, False)  # in [0, 1]

            if self.cfg.normal_direction == "camera":
                bg_normal = 0.5 * torch.ones_like(gb_normal)
                bg_normal[..., 2] = 1.0
                bg_normal_white = torch.ones_like(gb_normal)
                w2c = torch.inverse(c2w[sl])
                rotate = w2c[:, :3, :3]
                gb_normal_cam = gb_normal[..., None, :] @ rotate.permute(0, 2, 1)[..., None, None, :, :]
                flip_x = torch.eye(3).to(w2c)  # pixel space flip axis
                flip_x[0, 0] = -1
                gb_normal_cam = (gb_normal_cam @ flip_x[None, None, None, ...]).squeeze(-2)
                gb_normal_cam = (F.normalize(gb_normal_cam, dim=-1) + 1.0) / 2.0
                out["comp_normal_cam_vis"] = _PreAA(torch.lerp(bg_normal, gb_normal_cam, mask.float()), is_empty)
                out["comp_normal_cam_vis_white"] = _PreAA(torch.lerp(bg_normal_white, gb_normal_cam, mask.float()),
                                                          is_empty)
            elif self.cfg.normal_direction == "front":
                bg_normal_white = torch.ones_like(gb_normal)
                c2w_front = c2w[batch_idx * num_views_per_batch][None, ...].repeat(num_views_per_batch, 1, 1)
                rotate_front = torch.inverse(c2w_front)[:, :3, :3]
                gb_normal_cam = (gb_normal[..., None, :] @ rotate_front.permute(0, 2, 1)[..., None, None, :, :])
                gb_normal_cam = (F.normalize(gb_normal_cam.squeeze(-2), dim=-1) + 1.0) / 2.0
                out["comp_normal_cam_vis_white"] = _PreAA(torch.lerp(bg_normal_white, gb_normal_cam, mask.float()),
                                                          is_empty)

            if render_rgb:
                space_cache_slice = prompt_slice(space_cache, batch_idx)
                selector = mask[..., 0]
                gb_pos = g.pos
                gb_viewdirs = F.normalize(gb_pos - camera_positions[sl, None, None, :], dim=-1)
                gb_light_positions = light_positions[sl, None, None, :].expand(-1, height, width, -1)
                positions = gb_pos[selector]
                geo_out = self.geometry(positions[None, ...], space_cache_slice, output_normal=self.training)

                extra_geo_info = {}
                if getattr(self.material, "requires_normal", False):
                    extra_geo_info["shading_normal"] = keep(gb_normal[selector])
                geo_out.pop("shading_normal", None)
                if "sdf_grad" in geo_out:
                    out["sdf_grad"] = geo_out["sdf_grad"]
                if "sdf" in geo_out:
                    out["sdf"] = geo_out["sdf"]

                rgb_fg = self.material(viewdirs=gb_viewdirs[selector], positions=positions,
                                       light_positions=gb_light_positions[selector], **extra_geo_info, **geo_out)
                gb_rgb_fg = torch.zeros(num_views_per_batch, height, width, 3).to(rgb_fg)
                gb_rgb_fg[selector] = rgb_fg

                if self.cfg.enable_bg_rays:
                    assert rays_d_rasterize is not None
                    view_dirs = rays_d_rasterize[sl]
                else:
                    view_dirs = gb_viewdirs
                if getattr(self.background, "enabling_hypernet", False):
                    emb = kwargs["text_embed_bg"] if "text_embed_bg" in kwargs else text_embed
                    if emb is not None and emb.shape[0] == len(mesh_list):
                        # the prompt's own row (the reference passes every prompt's, which its background's
                        # per-view repeat only accepts for one prompt)
                        emb = emb[batch_idx:batch_idx + 1]
                    gb_rgb_bg = self.background(dirs=view_dirs, text_embed=emb)
                else:
                    gb_rgb_bg = self.background(dirs=view_dirs)

                out["comp_rgb"] = _PreAA(torch.lerp(gb_rgb_bg, gb_rgb_fg, mask.float()), is_empty)
                out["comp_rgb_bg"] = keep(gb_rgb_bg)
            return out

        out_list = []
        for batch_idx, mesh in enumerate(mesh_list):
            if batched:
                out_list.append(shade(batch_idx, mesh, gbuffers[batch_idx]))
                continue
            sl = slice(batch_idx * num_views_per_batch, (batch_idx + 1) * num_views_per_batch)
            g, aa = self._raster_prompt(mesh, mvp_mtx[sl], height, width, render_rgb)
            out = shade(batch_idx, mesh, g)
            out_list.append({k: v.resolve(aa) if isinstance(v, _PreAA) else v for k, v in out.items()})

        out = {}
        for key in out_list[0].keys():
            vals = [o[key] for o in out_list]
            if key in ["mesh", "sdf_grad", "sdf"]:
                out[key] = vals
            elif isinstance(vals[0], _PreAA):  # batched: every prompt's image through one antialias
                out[key] = _PreAA(torch.concat([v.img for v in vals], dim=0), vals[0].detach).resolve(aa_all)
            else:
                out[key] = torch.concat(vals, dim=0)
        return out

    def _raster_prompt(self, mesh: Mesh, mvp_mtx: Tensor, height: int, width: int, render_rgb: bool):
        """The raster stage of one prompt in instance mode: its G-buffer and its antialias."""
        v_pos_clip = self.ctx.vertex_transform(mesh.v_pos, mvp_mtx)
        tri = mesh.t_pos_idx
        topo = mesh.topology.antialias_tables
        if self.training:
            rast, _ = self.ctx.rasterize(v_pos_clip, tri, (height, width))
            gb_feat, _ = self.ctx.interpolate(v_pos_clip, rast, tri)
            depth = gb_feat[..., -2:-1]
        else:  # about 40 views: rasterize 4 at a time (reference :145-156)
            rast_list, depth_list = [], []
            n_views_per_rasterize = 4
            for i in range(0, v_pos_clip.shape[0], n_views_per_rasterize):
                r, _ = self.ctx.rasterize(v_pos_clip[i:i + n_views_per_rasterize], tri, (height, width))
                rast_list.append(r)
                gb_feat, _ = self.ctx.interpolate(v_pos_clip[i:i + n_views_per_rasterize], r, tri)
                depth_list.append(gb_feat[..., -2:-1])
            rast = torch.cat(rast_list, dim=0)
            depth = torch.cat(depth_list, dim=0)
        gb_normal, _ = self.ctx.interpolate_one(mesh.v_nrm, rast, tri)
        gb_pos = self.ctx.interpolate_one(mesh.v_pos, rast, tri)[0] if render_rgb else None

        def aa(img: Tensor) -> Tensor:
            return self.ctx.antialias(img, rast, v_pos_clip, tri, topology=topo)

        return _GBuffer(rast, depth, gb_normal, gb_pos), aa

    def _raster_batched(self, mesh_list: List[Mesh], mvp_mtx: Tensor, n_view: int, height: int, width: int,
                        render_rgb: bool):
        """The raster stage of all prompts in range mode (batch_prompts): every (prompt, view) image is one range of
        one packed vertex buffer, so one rasterize, one interpolate per attribute and, later, one antialias per
        output serve the whole step.  Returns the per-prompt G-buffers and the antialias of the (P n_view) images."""
        pos, tri, topo, nrm, v_pos = [], [], [], [], []
        for batch_idx, mesh in enumerate(mesh_list):
            # the looped path's call, so the clip positions have its bits
            clip = self.ctx.vertex_transform(mesh.v_pos, mvp_mtx[batch_idx * n_view:(batch_idx + 1) * n_view])
            pos += [clip[v] for v in range(n_view)]
            tri += [mesh.t_pos_idx] * n_view
            topo += [mesh.topology.antialias_tables] * n_view
            nrm += [mesh.v_nrm] * n_view
            v_pos += [mesh.v_pos] * n_view
        pk = raster.pack_ranges(pos, tri, topo)
        rast, _ = self.ctx.rasterize(pk.pos, pk.tri, (height, width), ranges=pk.ranges)
        depth = self.ctx.interpolate(pk.pos, rast, pk.tri)[0][..., -2:-1]
        gb_normal, _ = self.ctx.interpolate(torch.cat(nrm), rast, pk.tri)
        gb_pos = self.ctx.interpolate(torch.cat(v_pos), rast, pk.tri)[0] if render_rgb else None

        def aa(img: Tensor) -> Tensor:
            return self.ctx.antialias(img, rast, pk.pos, pk.tri, topology=pk.topology)

        gbuffers = []
        for batch_idx in range(len(mesh_list)):
            sl = slice(batch_idx * n_view, (batch_idx + 1) * n_view)
            gbuffers.append(_GBuffer(rast[sl], depth[sl], gb_normal[sl], gb_pos[sl] if render_rgb else None))
        return gbuffers, aa

    def update_step(self, epoch: int, global_step: int, on_load_weights: bool = False) -> None:
        self.sdf_grad_shrink = C(self.cfg.sdf_grad_shrink, epoch, global_step)
        self.def_grad_shrink = C(self.cfg.def_grad_shrink, epoch, global_step)

    def isosurface(self, space_cache: Any) -> List[Mesh]:
        """reference :416-514: grid query on the [-1, 1] box, gradient shrink, the InstantMesh fix-up of an empty
        field, one marching-cubes helper per prompt ("mt": one helper for all), vertices mapped back to [-1, 1]."""
        batch_size, device = cache_batch_device(space_cache)
        helper = self.isosurface_helper
        points = scale_tensor(helper.grid_vertices.to(device), helper.points_range, [-1, 1])
        sdf_batch, deformation_batch = self.geometry.forward_field(points[None, ...].expand(batch_size, -1, -1),
                                                                   space_cache)
        if self.sdf_grad_shrink != 0:
            sdf_batch = self.sdf_grad_shrink * sdf_batch + (1 - self.sdf_grad_shrink) * sdf_batch.detach()
        else:
            sdf_batch = sdf_batch.detach()
        if deformation_batch is not None:
            if self.def_grad_shrink != 0:
                # (the reference scales the deformation by sdf_grad_shrink here, :446-448)
                deformation_batch = self.sdf_grad_shrink * deformation_batch + \
                    (1 - self.sdf_grad_shrink) * deformation_batch.detach()
            else:
                deformation_batch = deformation_batch.detach()

        mesh_list = []
        for index in range(sdf_batch.shape[0]):
            sdf = sdf_batch[index]
            deformation = None if deformation_batch is None else deformation_batch[index]
            if torch.all(sdf > 0) or torch.all(sdf < 0):
                print("All sdf values are positive or negative, no isosurface")
                self.empty_flag = self.cfg.allow_empty_flag
                # follow InstantMesh (src/models/lrm_mesh.py)
                update_sdf = torch.zeros_like(sdf)
                max_sdf, min_sdf = sdf.max(), sdf.min()
                update_sdf[self.center_indices.to(sdf.device)] += (-1 - max_sdf)  # smaller than zero
                update_sdf[self.border_indices.to(sdf.device)] += (1 - min_sdf)  # larger than zero
                new_sdf = sdf + update_sdf
                update_mask = (new_sdf == 0).float()
                sdf = new_sdf * (1 - update_mask) + sdf * update_mask
            if index > 0 and self.cfg.isosurface_method == "diffmc":  # one helper per prompt (reference :514-524)
                name = f"isosurface_helper_{index}"
                if not hasattr(self, name):
                    setattr(self, name, DiffMarchingCubeHelper(self.cfg.isosurface_resolution))
                mesh = getattr(self, name)(sdf, deformation)
            else:
                mesh = helper(sdf, deformation)
            mesh.v_pos = scale_tensor(mesh.v_pos, helper.points_range, [-1, 1])
            mesh_list.append(mesh)
        return mesh_list

    def train(self, mode=True):
        if hasattr(self.geometry, "train"):
            self.geometry.train(mode)
        return super().train(mode=mode)

    def eval(self):
        if hasattr(self.geometry, "eval"):
            self.geometry.eval()
        return super().eval()
