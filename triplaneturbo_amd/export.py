"""Textured mesh export: the reference's `multiprompt-mesh-exporter`
(custom/triplaneturbo/models/exporters/multiprompt_mesh_exporter.py) and the OBJ / MTL / texture writer it hands its
params to (threestudio/utils/saving.py:491-691, `save_obj`), on this package's pieces: the mesh renderer's isosurface,
the HIP UV atlas (Mesh.unwrap_uv -> ops.uv_atlas) in place of xatlas, the HIP rasterizer in place of nvdiffrast, the
per-texel `geometry.export` / `material.export` decode and the HIP nearest-texel fill (ops.texture_fill) in place of
cv2.inpaint.  Same registry name, Config fields and defaults, call signature and `params` keys as the reference.

    exporter = tt.find("multiprompt-mesh-exporter")({"save_uv": True}, geometry=g, material=m, background=b)
    (out,) = exporter(space_cache)                     # g.isosurface: installed by the mesh renderer's configure
    save_obj(os.path.join(d, out.save_name), **out.params)   # model.obj, model.mtl, texture_kd.jpg

PNG is written with the standard library (zlib + struct); JPEG needs PIL."""
from __future__ import annotations

import os
import struct
import zlib
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import ops, raster
from .isosurface import prompt_slice
from .registry import Updateable, parse_structured, register

Tensor = torch.Tensor


@dataclass
class ExporterOutput:
    """threestudio/models/exporters/base.py:11-15"""
    save_name: str
    save_type: str
    params: Dict[str, Any]


class Exporter(Updateable):
    """threestudio/models/exporters/base.py:18-52 (a BaseObject: Config parsed like the modules', no weights)."""

    @dataclass
    class Config:
        save_video: bool = False

    cfg: Config

    def __init__(self, cfg: Optional[Any] = None, *args, **kwargs) -> None:
        self.cfg = parse_structured(self.Config, cfg)
        self.configure(*args, **kwargs)

    def configure(self, geometry, material, background) -> None:
        @dataclass
        class SubModules:
            geometry: Any
            material: Any
            background: Any

        self.sub_modules = SubModules(geometry, material, background)

    @property
    def geometry(self):
        return self.sub_modules.geometry

    @property
    def material(self):
        return self.sub_modules.material

    @property
    def background(self):
        return self.sub_modules.background

    @property
    def device(self) -> torch.device:
        return torch.device("cuda", torch.cuda.current_device())

    def __call__(self, *args, **kwargs) -> List[ExporterOutput]:
        raise NotImplementedError


@register("multiprompt-mesh-exporter")
class MultipromptMeshExporter(Exporter):
    @dataclass
    class Config(Exporter.Config):
        fmt: str = "obj-mtl"  # in ['obj-mtl', 'obj']
        save_name: str = "model"
        save_normal: bool = False
        save_uv: bool = False
        save_texture: bool = True
        texture_size: int = 1024
        texture_format: str = "jpg"
        xatlas_chart_options: dict = field(default_factory=dict)
        xatlas_pack_options: dict = field(default_factory=dict)
        context_type: str = "cuda"

    cfg: Config

    def configure(self, geometry, material, background) -> None:
        super().configure(geometry, material, background)
        self.ctx = raster.RasterizerContext(self.cfg.context_type, None)
        # Mesh.simplify's arguments; attributes, not Config fields (the Config mirrors the reference's).  With one of
        # them set the exported mesh is the simplified mesh[0] (more than one is a ValueError at call time); with all
        # None it is the isosurface mesh untouched.
        self.simplify_grid: Optional[int] = None
        self.simplify_target_faces: Optional[int] = None
        self.simplify_max_error: Optional[float] = None
        # Mesh.decimate's argument, an attribute for the same reason: with it set the exported mesh is mesh[0] decimated
        # to at most that many faces (manifold-preserving edge collapse); together with a simplify attribute it is a
        # ValueError at call time.
        self.decimate_target_faces: Optional[int] = None
        # Mesh.remesh's arguments, attributes for the same reason: with one of them set the exported mesh is mesh[0]
        # remeshed isotropically (at that edge length, or towards that many faces); both, or one together with a
        # simplify attribute or decimate_target_faces, is a ValueError at call time.
        self.remesh_edge_length: Optional[float] = None
        self.remesh_target_faces: Optional[int] = None
        # Mesh.solidify's arguments, attributes for the same reason: with solidify_resolution set mesh[0] goes through
        # the field first (a watertight surface without interior walls, thickened or eroded by solidify_offset) and
        # simplify / decimate / remesh, when set, work on that.  Unset, the export is what it is without the attribute;
        # solidify_offset alone is a ValueError at call time.
        self.solidify_resolution: Optional[int] = None
        self.solidify_offset: float = 0.0
        # the tangent-space normal map of the exported mesh (map_Bump, ops.bake_normal_map) on the obj-mtl path with
        # save_texture, and the number of projection steps it takes towards the iso-surface; attributes for the same
        # reason.  Unset, params are exactly what they are without the bake.
        # the flattening of the atlas' charts (Mesh.unwrap_uv's `method`: "axis", or "lscm" for conformal charts); an
        # attribute for the same reason.  None means "axis": unset, the export is what it is without the attribute.
        self.uv_method: Optional[str] = None
        self.bake_normal_map: bool = False
        self.bake_project_steps: int = 2
        self.bake_info: Optional[Dict[str, Any]] = None  # ops.bake_normal_map's info of the last bake
        # the ambient-occlusion map of the exported mesh (map_Ka, ops.bake_ambient_occlusion: the simplified mesh when
        # a simplify attribute is set) on the same path: its rays per texel and their length (None: a quarter of the
        # bounding-box diagonal).  Unset, params carry no "map_Ka" key and every other map is what it is without it.
        self.bake_ambient_occlusion: bool = False
        self.ao_rays: int = 64
        self.ao_distance: Optional[float] = None
        self.ao_info: Optional[Dict[str, Any]] = None  # ops.bake_ambient_occlusion's info of the last bake

    @torch.no_grad()
    def __call__(self, space_cache) -> List[ExporterOutput]:
        simplify = {"grid": self.simplify_grid, "target_faces": self.simplify_target_faces,
                    "max_error": self.simplify_max_error}
        if sum(v is not None for v in simplify.values()) > 1:
            raise ValueError("multiprompt-mesh-exporter: set at most one of simplify_grid, simplify_target_faces and "
                             "simplify_max_error")
        if self.decimate_target_faces is not None and any(v is not None for v in simplify.values()):
            raise ValueError("multiprompt-mesh-exporter: decimate_target_faces cannot be combined with a simplify_* "
                             "attribute")
        remesh = {"edge_length": self.remesh_edge_length, "target_faces": self.remesh_target_faces}
        if all(v is not None for v in remesh.values()):
            raise ValueError("multiprompt-mesh-exporter: set at most one of remesh_edge_length and remesh_target_faces")
        if any(v is not None for v in remesh.values()) and (
                self.decimate_target_faces is not None or any(v is not None for v in simplify.values())):
            raise ValueError("multiprompt-mesh-exporter: remesh_edge_length / remesh_target_faces cannot be combined "
                             "with a simplify_* attribute or decimate_target_faces")
        if self.solidify_resolution is None and self.solidify_offset != 0:
            raise ValueError("multiprompt-mesh-exporter: solidify_offset needs solidify_resolution")
        isosurface = getattr(self.geometry, "isosurface", None)
        if isosurface is None:
            raise RuntimeError("geometry.isosurface is not set: configure a generative-space-mesh-rasterize-renderer "
                               "with this geometry first (its configure installs it, as the reference's does)")
        mesh = isosurface(space_cache)
        if type(mesh) == list:
            mesh = mesh[0]
        if self.solidify_resolution is not None:
            mesh = mesh.solidify(self.solidify_resolution, offset=self.solidify_offset)
        if any(v is not None for v in simplify.values()):
            mesh = mesh.simplify(**simplify)
        if self.decimate_target_faces is not None:
            mesh = mesh.decimate(self.decimate_target_faces)
        if any(v is not None for v in remesh.values()):
            mesh = mesh.remesh(**remesh)
        # the texture belongs to mesh[0]: decode it from the first prompt's slice of the space cache
        space_cache = prompt_slice(space_cache, 0)
        if self.cfg.fmt == "obj-mtl":
            return self.export_obj_with_mtl(mesh, space_cache)
        elif self.cfg.fmt == "obj":
            return self.export_obj(mesh, space_cache)
        else:
            raise ValueError(f"Unsupported mesh export format: {self.cfg.fmt}")

    def _params(self, mesh, save_mat: bool) -> Dict[str, Any]:
        return {"mesh": mesh, "save_mat": save_mat, "save_normal": self.cfg.save_normal, "save_uv": self.cfg.save_uv,
                "save_vertex_color": False, "map_Kd": None, "map_Ks": None, "map_Bump": None, "map_Pm": None,
                "map_Pr": None, "map_format": self.cfg.texture_format}

    def _unwrap(self, mesh) -> None:
        mesh.unwrap_uv(self.cfg.xatlas_chart_options, self.cfg.xatlas_pack_options, texture_size=self.cfg.texture_size,
                       method=self.uv_method)

    def _bake_max_step(self, mesh) -> float:
        """The longest projection step: the cell of a simplified mesh, else one cell of the isosurface grid."""
        simp = mesh.extras.get("simplify")
        if simp is not None:
            return float(simp["cell"])
        renderer = getattr(getattr(self.geometry, "isosurface", None), "__self__", None)
        res = getattr(getattr(renderer, "cfg", None), "isosurface_resolution", None)
        if res is None:
            raise RuntimeError("bake_normal_map: the isosurface resolution is unknown (geometry.isosurface is not a "
                               "mesh renderer's); simplify the mesh or call ops.bake_normal_map with max_step")
        return 2.0 * float(self.geometry.cfg.radius) / float(res)

    def export_obj_with_mtl(self, mesh, space_cache) -> List[ExporterOutput]:
        params = self._params(mesh, True)
        if self.cfg.save_uv:
            self._unwrap(mesh)
        if self.cfg.save_texture:
            assert self.cfg.save_uv, "save_uv must be True when save_texture is True"
            N = self.cfg.texture_size
            uv_clip = mesh.v_tex * 2.0 - 1.0  # clip space
            uv_clip4 = torch.cat((uv_clip, torch.zeros_like(uv_clip[..., 0:1]), torch.ones_like(uv_clip[..., 0:1])),
                                 dim=-1)
            rast, _ = self.ctx.rasterize_one(uv_clip4, mesh.t_tex_idx, (N, N))
            hole_mask = ~(rast[:, :, 3] > 0)

            def uv_padding(image: Tensor) -> Tensor:  # nearest covered texel, not cv2's Telea inpainting
                return ops.texture_fill(image.float(), ~hole_mask).to(image)

            gb_pos, _ = self.ctx.interpolate_one(mesh.v_pos, rast[None, ...], mesh.t_pos_idx)  # world positions
            gb_pos = gb_pos[0]
            geo_out = self.geometry.export(points=gb_pos, space_cache=space_cache)
            mat_out = self.material.export(points=gb_pos, **geo_out)
            if "albedo" in mat_out:
                params["map_Kd"] = uv_padding(mat_out["albedo"])
            else:
                print("save_texture is True but no albedo texture found, using default white texture")
            if "metallic" in mat_out:
                params["map_Pm"] = uv_padding(mat_out["metallic"])
            if "roughness" in mat_out:
                params["map_Pr"] = uv_padding(mat_out["roughness"])
            if "bump" in mat_out:
                params["map_Bump"] = uv_padding(mat_out["bump"])
            if self.bake_normal_map:
                def field(p: Tensor):
                    out = self.geometry.forward(p[None], space_cache, output_normal=True)
                    return out["sdf"], out["sdf_grad"]

                bump, self.bake_info = ops.bake_normal_map(mesh, field, N, project_steps=self.bake_project_steps,
                                                           max_step=self._bake_max_step(mesh), rast=rast)
                params["map_Bump"] = uv_padding(bump)
            if self.bake_ambient_occlusion:
                ao, self.ao_info = ops.bake_ambient_occlusion(mesh, N, n_rays=self.ao_rays,
                                                              max_distance=self.ao_distance, rast=rast)
                params["map_Ka"] = uv_padding(ao)
        return [ExporterOutput(save_name=f"{self.cfg.save_name}.obj", save_type="obj", params=params)]

    def export_obj(self, mesh, space_cache) -> List[ExporterOutput]:
        params = self._params(mesh, False)
        if self.cfg.save_uv:
            self._unwrap(mesh)
        if self.cfg.save_texture:
            geo_out = self.geometry.export(points=mesh.v_pos, space_cache=space_cache)
            mat_out = self.material.export(points=mesh.v_pos, **geo_out)
            if "albedo" in mat_out:
                mesh.set_vertex_color(mat_out["albedo"])
                params["save_vertex_color"] = True
            else:
                print("save_texture is True but no albedo texture found, not saving vertex color")
        return [ExporterOutput(save_name=f"{self.cfg.save_name}.obj", save_type="obj", params=params)]


# ---------------------------------------------------------------------------------------------------------------
# files: saving.py:491-691
def _np(x: Any) -> Optional[np.ndarray]:
    if x is None:
        return None
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _rgb_u8(img: np.ndarray) -> np.ndarray:
    """saving.py:78-110 (HWC, data_range (0, 1)): clip, * 255, truncate to uint8, 3 channels (padded with zeros)."""
    if img.dtype != np.uint8:
        img = (np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8)
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[-1] < 3:
        img = np.concatenate([img, np.zeros(img.shape[:2] + (3 - img.shape[-1],), np.uint8)], axis=-1)
    return np.ascontiguousarray(img[..., :3])


def _gray_u8(img: np.ndarray) -> np.ndarray:
    """saving.py:180-191 (data_range (0, 1), no colour map): nan -> 0, clip, * 255, uint8, repeated to 3 channels."""
    img = np.nan_to_num(img.astype(np.float64))
    if img.ndim == 3:
        img = img[..., 0]
    img = (np.clip(img, 0.0, 1.0) * 255.0).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(img[..., None], 3, axis=2))


def png_bytes(img: np.ndarray) -> bytes:
    """uint8 (H,W), (H,W,1), (H,W,3) or (H,W,4) -> an 8-bit PNG (filter 0 rows, zlib), standard library only."""
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError(f"png_bytes needs uint8, got {img.dtype}")
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    ctype = {1: 0, 3: 2, 4: 6}.get(C)
    if ctype is None:
        raise ValueError(f"png_bytes: 1, 3 or 4 channels, got {C}")
    raw = np.concatenate([np.zeros((H, 1), np.uint8), img.reshape(H, W * C)], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, ctype, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """The inverse of png_bytes for what it writes (8-bit grey / RGB / RGBA, any of the five row filters)."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path} is not a PNG")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            break
    W, H, depth, ctype, _, _, interlace = hdr
    C = {0: 1, 2: 3, 6: 4}.get(ctype)
    if depth != 8 or C is None or interlace:
        raise ValueError(f"{path}: only 8-bit non-interlaced grey / RGB / RGBA PNGs are read")
    raw = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(H, W * C + 1)
    out = np.zeros((H, W * C), np.int32)
    prev = np.zeros(W * C, np.int32)
    for y in range(H):
        f, row = raw[y, 0], raw[y, 1:].astype(np.int32)
        if f == 0:
            cur = row
        elif f == 2:
            cur = (row + prev) & 255
        else:  # 1 (sub), 3 (average), 4 (Paeth): left-dependent, byte by byte
            cur = np.zeros_like(row)
            for i in range(W * C):
                a = cur[i - C] if i >= C else 0
                b, c = prev[i], (prev[i - C] if i >= C else 0)
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) // 2
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (row[i] + p) & 255
        out[y], prev = cur, cur
    return out.astype(np.uint8).reshape(H, W, C)


def save_image(path: str, img: np.ndarray) -> str:
    """uint8 image -> path by extension: .png with the standard library, .jpg / .jpeg / anything else through PIL."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        with open(path, "wb") as f:
            f.write(png_bytes(img))
        return path
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"writing {path!r} needs PIL (Pillow), which is not installed; use map_format='png' "
                           f"(written with the standard library)") from None
    Image.fromarray(img).save(path)
    return path


def _save_obj_text(path: str, v_pos, t_pos_idx, v_nrm=None, v_tex=None, t_tex_idx=None, v_rgb=None, matname=None,
                   mtllib=None) -> str:
    """saving.py:551-594, line for line."""
    lines = []
    if matname is not None:
        lines += [f"mtllib {mtllib}\n", "g object\n", f"usemtl {matname}\n"]
    for i in range(len(v_pos)):
        s = f"v {v_pos[i][0]} {v_pos[i][1]} {v_pos[i][2]}"
        if v_rgb is not None:
            s += f" {v_rgb[i][0]} {v_rgb[i][1]} {v_rgb[i][2]}"
        lines.append(s + "\n")
    if v_nrm is not None:
        lines += [f"vn {v[0]} {v[1]} {v[2]}\n" for v in v_nrm]
    if v_tex is not None:
        lines += [f"vt {v[0]} {1.0 - v[1]}\n" for v in v_tex]
    for i in range(len(t_pos_idx)):
        s = "f"
        for j in range(3):
            s += f" {t_pos_idx[i][j] + 1}/"
            if v_tex is not None:
                s += f"{t_tex_idx[i][j] + 1}"
            s += "/"
            if v_nrm is not None:
                s += f"{t_pos_idx[i][j] + 1}"
        lines.append(s + "\n")
    with open(path, "w") as f:
        f.write("".join(lines))
    return path


def _save_mtl(path: str, matname: str, Ka=(0.0, 0.0, 0.0), Kd=(1.0, 1.0, 1.0), Ks=(0.0, 0.0, 0.0), map_Kd=None,
              map_Ks=None, map_Bump=None, map_Pm=None, map_Pr=None, map_format: str = "jpg", map_Ka=None) -> List[str]:
    """saving.py:596-691: the MTL text and the texture images next to it.  map_Ka (not in the reference): the
    ambient-occlusion map, written as gray texture_ao.<fmt>."""
    d = os.path.dirname(path)
    paths = [path]
    mtl = f"newmtl {matname}\n"
    mtl += f"Ka {Ka[0]} {Ka[1]} {Ka[2]}\n"
    if map_Kd is not None:
        mtl += f"map_Kd texture_kd.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_kd.{map_format}"), _rgb_u8(map_Kd)))
    else:
        mtl += f"Kd {Kd[0]} {Kd[1]} {Kd[2]}\n"
    if map_Ks is not None:
        mtl += f"map_Ks texture_ks.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_ks.{map_format}"), _rgb_u8(map_Ks)))
    else:
        mtl += f"Ks {Ks[0]} {Ks[1]} {Ks[2]}\n"
    if map_Bump is not None:
        mtl += f"map_Bump texture_nrm.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_nrm.{map_format}"), _rgb_u8(map_Bump)))
    if map_Pm is not None:
        mtl += f"map_Pm texture_metallic.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_metallic.{map_format}"), _gray_u8(map_Pm)))
    if map_Pr is not None:
        mtl += f"map_Pr texture_roughness.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_roughness.{map_format}"), _gray_u8(map_Pr)))
    if map_Ka is not None:
        mtl += f"map_Ka texture_ao.{map_format}\n"
        paths.append(save_image(os.path.join(d, f"texture_ao.{map_format}"), _gray_u8(map_Ka)))
    with open(path, "w") as f:
        f.write(mtl)
    return paths


def save_obj(path: str, mesh, save_mat: bool = False, save_normal: bool = False, save_uv: bool = False,
             save_vertex_color: bool = False, map_Kd: Optional[Tensor] = None, map_Ks: Optional[Tensor] = None,
             map_Bump: Optional[Tensor] = None, map_Pm: Optional[Tensor] = None, map_Pr: Optional[Tensor] = None,
             map_format: str = "jpg", map_Ka: Optional[Tensor] = None) -> List[str]:
    """saving.py:491-549 as a standalone writer: `path` (".obj" appended if missing), with save_mat the MTL file
    (same name, ".mtl") and its texture images in the same directory.  Takes the exporter's params as keywords.
    Returns the written paths."""
    if not path.endswith(".obj"):
        path += ".obj"
    v_pos, t_pos_idx = _np(mesh.v_pos), _np(mesh.t_pos_idx)
    v_nrm = _np(mesh.v_nrm) if save_normal else None
    v_tex, t_tex_idx = (_np(mesh.v_tex), _np(mesh.t_tex_idx)) if save_uv else (None, None)
    v_rgb = _np(mesh.v_rgb) if save_vertex_color else None
    paths: List[str] = []
    matname, mtllib = None, None
    if save_mat:
        matname = "default"
        mtl_path = path.replace(".obj", ".mtl")
        mtllib = os.path.basename(mtl_path)
        paths += _save_mtl(mtl_path, matname, map_Kd=_np(map_Kd), map_Ks=_np(map_Ks), map_Bump=_np(map_Bump),
                           map_Pm=_np(map_Pm), map_Pr=_np(map_Pr), map_format=map_format, map_Ka=_np(map_Ka))
    paths.append(_save_obj_text(path, v_pos, t_pos_idx, v_nrm=v_nrm, v_tex=v_tex, t_tex_idx=t_tex_idx, v_rgb=v_rgb,
                                matname=matname, mtllib=mtllib))
    return paths
