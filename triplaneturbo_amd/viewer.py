"""Render what the exporter wrote: read an OBJ + MTL + map_Kd back (`load_obj`, the inverse of export.save_obj) and
put the texture on the mesh with the HIP rasterizer and texture sampler (`render_textured`, `turntable`) -- the last
step of the reference's text -> mesh -> images pipeline (evaluation/mesh_visualize.py renders the exported OBJs from a
few azimuths for CLIPScore, with CUDA-only tools).

    mesh, map_Kd = load_obj("model.obj", device="cuda")
    imgs = turntable(mesh, map_Kd, n_views=4, height=512, width=512, ssaa=2)      # (4,512,512,3) in [0,1]

    map_Bump = load_normal_map("model.obj", device="cuda")                        # the MTL's map_Bump, or None
    imgs = turntable(mesh, map_Kd, mode="normal_map", map_Bump=map_Bump)          # the detail normals, (n + 1) / 2

    map_Ka = load_ao_map("model.obj", device="cuda")                              # the MTL's map_Ka, or None
    imgs = turntable(mesh, map_Kd, map_Ka=map_Ka)                                 # map_Kd times the ambient occlusion
    imgs = turntable(mesh, map_Kd, mode="ao", map_Ka=map_Ka)                      # the occlusion alone, gray

    python -m triplaneturbo_amd.viewer model.obj --out views [--num_views 4] [--normal] [--bump] [--ao] [--size 512] [--ssaa 2]
    # views/rgb_0.png ... (normal_0.png ... with --normal, bump_0.png ... with --bump when the MTL names a normal map,
    # ao_0.png ... and occlusion-shaded rgb_0.png ... with --ao when it names an ambient-occlusion map)

Torch plumbing between kernels, like mesh_renderer.py: rasterize, interpolate, texture and antialias are
triplaneturbo_amd.raster.  The sampler has no mipmaps (tt_abi.h "texture sampling"): a texture that is minified on
screen is antialiased by supersampling (`ssaa`: render at ssaa x the size, average down), which is this module's only
answer to minification.  Differentiable w.r.t. map_Kd and mesh.v_pos, so a baked map can be refined against renders."""
from __future__ import annotations

import argparse
import math
import os
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import export, synthetic
from .isosurface import Mesh
from .raster import RasterizerContext

Tensor = torch.Tensor


def _read_image(path: str) -> np.ndarray:
    if os.path.splitext(path)[1].lower() == ".png":
        return export.read_png(path)
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError(f"reading {path!r} needs PIL (Pillow), which is not installed; use map_format='png' "
                           f"(read with the standard library)") from None
    return np.asarray(Image.open(path).convert("RGB"))


def _map_path(mtl_path: str, key: str = "map_Kd") -> Optional[str]:
    if not os.path.exists(mtl_path):
        return None
    for line in open(mtl_path):
        tok = line.split(None, 1)
        if len(tok) == 2 and tok[0] == key:
            return os.path.join(os.path.dirname(mtl_path), tok[1].strip())
    return None


def _image_tensor(path: str, device) -> Tensor:
    img = _read_image(path)
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[-1] < 3:
        img = np.repeat(img[..., :1], 3, axis=-1)
    return (torch.from_numpy(np.ascontiguousarray(img[..., :3])).to(torch.float32) / 255.0).to(device=device)


def _mtl_map(obj_path: str, key: str) -> Optional[str]:
    mtllib = None
    with open(obj_path) as fh:
        for line in fh:
            if line.startswith("mtllib"):
                mtllib = line.split(None, 1)[1].strip()
                break
    return _map_path(os.path.join(os.path.dirname(obj_path), mtllib), key) if mtllib else None


def load_ao_map(obj_path: str, device=None) -> Optional[Tensor]:
    """The ambient-occlusion map an exported OBJ's MTL names (`map_Ka`, export.save_obj's texture_ao.<fmt>) as float
    (N,N,1) in [0,1] (uint8 / 255), None when the OBJ has no MTL or the MTL no map_Ka.  Row 0 is v = 0, like map_Kd."""
    path = _mtl_map(obj_path, "map_Ka")
    return _image_tensor(path, device)[..., :1].contiguous() if path is not None else None


def load_normal_map(obj_path: str, device=None) -> Optional[Tensor]:
    """The tangent-space normal map an exported OBJ's MTL names (`map_Bump`, export.save_obj's texture_nrm.<fmt>) as
    float (N,N,3) in [0,1] (uint8 / 255), None when the OBJ has no MTL or the MTL no map_Bump.  Row 0 is v = 0 of
    load_obj's v_tex, like map_Kd."""
    path = _mtl_map(obj_path, "map_Bump")
    return _image_tensor(path, device) if path is not None else None


def read_obj_geometry(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(v (V,3) float64, f (T,3) int64) of any OBJ file: `v x y z ...` and `f` corners in the forms i, i/j, i/j/k and
    i//k (only the position index is read; negative indices count back from the last vertex read so far); a polygon
    becomes the fan (0, k, k+1) about its first corner.  Everything else (vt, vn, groups, materials) is skipped."""
    v, f = [], []
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                v.append([float(x) for x in tok[1:4]])
            elif tok[0] == "f":
                idx = [int(c.split("/")[0]) for c in tok[1:]]
                if len(idx) < 3:
                    raise ValueError(f"{path}: a face needs three corners, got {line.strip()!r}")
                idx = [i - 1 if i > 0 else len(v) + i for i in idx]
                if min(idx) < 0 or "0" in (c.split("/")[0] for c in tok[1:]):
                    raise ValueError(f"{path}: index out of range in {line.strip()!r}")
                f += [[idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1)]
    v_arr, f_arr = np.asarray(v, np.float64).reshape(-1, 3), np.asarray(f, np.int64).reshape(-1, 3)
    if f_arr.size and f_arr.max() >= len(v_arr):
        raise ValueError(f"{path}: a face names vertex {int(f_arr.max()) + 1} of {len(v_arr)}")
    return v_arr, f_arr


def load_obj(path: str, device=None) -> Tuple[Mesh, Optional[Tensor]]:
    """(mesh, map_Kd) from what export.save_obj writes: `v x y z [r g b]` -> v_pos (and v_rgb), `vt u v` -> v_tex with
    the writer's 1 - v flip undone, `f a/b/c` triangles -> t_pos_idx, t_tex_idx (int32), `mtllib` -> the MTL's map_Kd
    image as float (N,N,3) in [0,1] (uint8 / 255), None without one.  `vn` lines are read and ignored (Mesh.v_nrm
    recomputes the normals).  Quads, negative indices and several materials are not read (save_obj never writes them)."""
    v, rgb, vt, f_pos, f_tex, mtllib = [], [], [], [], [], None
    with open(path) as fh:
        for line in fh:
            tok = line.split()
            if not tok:
                continue
            if tok[0] == "v":
                v.append([float(x) for x in tok[1:4]])
                if len(tok) >= 7:
                    rgb.append([float(x) for x in tok[4:7]])
            elif tok[0] == "vt":
                vt.append([float(tok[1]), 1.0 - float(tok[2])])
            elif tok[0] == "f":
                if len(tok) != 4:
                    raise ValueError(f"{path}: only triangles are read, got {line.strip()!r}")
                corners = [c.split("/") for c in tok[1:]]
                f_pos.append([int(c[0]) - 1 for c in corners])
                if all(len(c) > 1 and c[1] for c in corners):
                    f_tex.append([int(c[1]) - 1 for c in corners])
            elif tok[0] == "mtllib":
                mtllib = line.split(None, 1)[1].strip()
    if rgb and len(rgb) != len(v):
        raise ValueError(f"{path}: {len(rgb)} of {len(v)} vertices carry a colour")
    if f_tex and (len(f_tex) != len(f_pos) or not vt):
        raise ValueError(f"{path}: {len(f_tex)} of {len(f_pos)} faces carry texture indices")
    if min((i for f in f_pos + f_tex for i in f), default=0) < 0:
        raise ValueError(f"{path}: negative (relative) indices are not read")

    def tensor(rows, dtype, width):
        return torch.tensor(rows, dtype=torch.float64 if dtype.is_floating_point else dtype).reshape(-1, width).to(
            device=device, dtype=dtype)

    mesh = Mesh(tensor(v, torch.float32, 3), tensor(f_pos, torch.int32, 3))
    if rgb:
        mesh.set_vertex_color(tensor(rgb, torch.float32, 3))
    if f_tex:
        mesh._v_tex, mesh._t_tex_idx = tensor(vt, torch.float32, 2), tensor(f_tex, torch.int32, 3)
    map_kd = None
    kd_path = _map_path(os.path.join(os.path.dirname(path), mtllib), "map_Kd") if mtllib else None
    if kd_path is not None:
        map_kd = _image_tensor(kd_path, device)
    return mesh, map_kd


def get_projection_matrix(fovy_deg: float, aspect_wh: float, near: float = 0.1, far: float = 1000.0) -> Tensor:
    """threestudio's get_projection_matrix (threestudio/utils/ops.py): OpenGL perspective with [1,1] negated, so image
    row 0 is the top."""
    t = math.tan(math.radians(fovy_deg) / 2)
    proj = torch.zeros(4, 4)
    proj[0, 0] = 1 / (t * aspect_wh)
    proj[1, 1] = -1 / t
    proj[2, 2] = -(far + near) / (far - near)
    proj[2, 3] = -2 * far * near / (far - near)
    proj[3, 2] = -1
    return proj


def world_normal_from_map(mesh: Mesh, rast: Tensor, map_Bump: Tensor, filter_mode: str = "linear",
                          ctx: Optional[RasterizerContext] = None) -> Tensor:
    """(B,H,W,3) unit world normals at the pixels of rast (B,H,W,4) (any rasterisation of the mesh's faces: a camera
    view, or the UV-space one the map was baked on), rebuilt from the tangent-space normal map map_Bump (TH,TW,3):
    x = 2 map - 1 sampled at the interpolated v_tex (boundary "clamp"), n = normalize(x_0 t^ + x_1 b^ + x_2 n^) in the
    frame n^ = normalize(interpolated v_nrm), t^ = normalize(t - (t . n^) n^) with t the interpolated v_tng_tex,
    b^ = t^ x n^ -- the frame tt_bake_encode writes the map in (include/tt_abi.h, "tangents and normal-map baking").
    Empty pixels hold zeros.  Composed from the differentiable interpolate / texture ops and torch arithmetic."""
    ctx = ctx or RasterizerContext("cuda", mesh.v_pos.device)
    uv, _ = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)
    n_hat = F.normalize(ctx.interpolate(mesh.v_nrm[None], rast, mesh.t_pos_idx.int())[0], dim=-1)
    tng, _ = ctx.interpolate(mesh.v_tng_tex[None], rast, mesh.t_tex_idx)
    t_hat = F.normalize(tng - (tng * n_hat).sum(-1, keepdim=True) * n_hat, dim=-1)
    b_hat = torch.cross(t_hat, n_hat, dim=-1)
    x = ctx.texture(map_Bump[None], uv, filter_mode=filter_mode, boundary_mode="clamp") * 2.0 - 1.0
    return F.normalize(x[..., 0:1] * t_hat + x[..., 1:2] * b_hat + x[..., 2:3] * n_hat, dim=-1)


def render_textured(mesh: Mesh, map_Kd: Optional[Tensor], mvp_mtx: Tensor, height: int, width: int, mode: str = "rgb",
                    ssaa: int = 1, background: float = 1.0, filter_mode: str = "linear", antialias: bool = True,
                    ctx: Optional[RasterizerContext] = None, map_Bump: Optional[Tensor] = None,
                    light_dir: Optional[Tensor] = None, map_Ka: Optional[Tensor] = None) -> Tensor:
    """(B,height,width,3) views of `mesh` under mvp_mtx (B,4,4).  mode "rgb": map_Kd (TH,TW,3) sampled at the
    interpolated v_tex (boundary "clamp"), or the interpolated v_rgb when the mesh has no UVs; with both map_Bump and
    light_dir (3,) (towards the light, world space) that colour times max(0, n . l), n the world normal of mode
    "normal_map".  mode "normal": (normalize(interpolated v_nrm) + 1) / 2.  mode "normal_map": (n + 1) / 2 with n the
    world normal rebuilt per pixel from map_Bump (TH,TW,3), a tangent-space normal map as the exporter bakes it:
    x = 2 map - 1 sampled at the interpolated v_tex, n = normalize(x_0 t^ + x_1 b^ + x_2 n^) in the frame n^ =
    normalize(interpolated v_nrm), t^ = normalize(t - (t . n^) n^) with t the interpolated v_tng_tex, b^ = t^ x n^
    (include/tt_abi.h, "tangents and normal-map baking").  map_Ka (TH,TW,1), an ambient-occlusion map as the exporter
    bakes it, sampled at the interpolated v_tex: it multiplies the colour of mode "rgb" (the one shading cue an unlit
    map_Kd render can have), and mode "ao" shows it alone, as gray.  Then a lerp to `background` by the coverage mask, silhouette
    antialiasing and, for ssaa > 1, the average of ssaa x ssaa samples per pixel (rendered at ssaa x the size).
    Differentiable w.r.t. map_Kd, map_Bump and mesh.v_pos (v_tng_tex is a constant)."""
    if mode not in ("rgb", "normal", "normal_map", "ao"):
        raise ValueError(f"mode must be 'rgb', 'normal', 'normal_map' or 'ao', got {mode!r}")
    if ssaa < 1:
        raise ValueError(f"ssaa must be >= 1, got {ssaa}")
    ctx = ctx or RasterizerContext("cuda", mesh.v_pos.device)
    tri = mesh.t_pos_idx.int()
    pos = ctx.vertex_transform(mesh.v_pos, mvp_mtx)
    rast, _ = ctx.rasterize(pos, tri, (ssaa * height, ssaa * width))
    mask = (rast[..., 3:] > 0).float()
    if mode == "normal_map" and (map_Bump is None or mesh._v_tex is None):
        raise ValueError("mode 'normal_map' needs a mesh with v_tex and a map_Bump")
    if mode == "ao" and (map_Ka is None or mesh._v_tex is None):
        raise ValueError("mode 'ao' needs a mesh with v_tex and a map_Ka")
    occlusion = None
    if map_Ka is not None and mesh._v_tex is not None and mode in ("rgb", "ao"):
        uv_ka, _ = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)
        occlusion = ctx.texture(map_Ka[..., :1].contiguous()[None], uv_ka, filter_mode=filter_mode, boundary_mode="clamp")
    shaded = mode == "rgb" and map_Bump is not None and light_dir is not None and mesh._v_tex is not None
    world_nrm = None
    if mode == "normal_map" or shaded:
        world_nrm = world_normal_from_map(mesh, rast, map_Bump, filter_mode=filter_mode, ctx=ctx)
    if mode == "normal_map":
        color = (world_nrm + 1.0) / 2.0
    elif mode == "ao":
        color = occlusion.expand(-1, -1, -1, 3)
    elif mode == "normal":
        nrm, _ = ctx.interpolate(mesh.v_nrm[None], rast, tri)
        color = (F.normalize(nrm, dim=-1) + 1.0) / 2.0
    elif mesh._v_tex is not None and map_Kd is not None:
        uv, _ = ctx.interpolate(mesh.v_tex[None], rast, mesh.t_tex_idx)
        color = ctx.texture(map_Kd[None], uv, filter_mode=filter_mode, boundary_mode="clamp")
        if shaded:
            l = F.normalize(torch.as_tensor(light_dir, dtype=torch.float32, device=color.device).reshape(3), dim=0)
            color = color * (world_nrm * l).sum(-1, keepdim=True).clamp_min(0.0)
    elif mesh.v_rgb is not None:
        color, _ = ctx.interpolate(mesh.v_rgb[None], rast, tri)
    else:
        raise ValueError("mode 'rgb' needs a mesh with v_tex and a map_Kd, or with vertex colours")
    if mode == "rgb" and occlusion is not None:
        color = color * occlusion
    img = torch.lerp(torch.full_like(color, float(background)), color, mask)
    if antialias:
        img = ctx.antialias(img, rast, pos, tri)
    if ssaa > 1:
        img = F.avg_pool2d(img.permute(0, 3, 1, 2), ssaa).permute(0, 2, 3, 1)
    return img


def turntable(mesh: Mesh, map_Kd: Optional[Tensor], n_views: int = 4, elevation_deg: float = 15.0,
              fovy_deg: float = 40.0, height: int = 512, width: int = 512, **render_kw) -> Tensor:
    """(n_views,height,width,3): render_textured from n_views equally spaced azimuths at one elevation, cameras from
    synthetic.make_cameras (z up, looking at the origin)."""
    _, _, c2w, _ = synthetic.make_cameras(n_views, height, width, fovy_deg=fovy_deg, elevation_deg=elevation_deg)
    mvp = get_projection_matrix(fovy_deg, width / height)[None] @ torch.inverse(c2w)
    return render_textured(mesh, map_Kd, mvp.to(mesh.v_pos.device), height, width, **render_kw)


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m triplaneturbo_amd.viewer", description=__doc__.split("\n\n")[0])
    ap.add_argument("obj", metavar="MODEL.obj")
    ap.add_argument("--out", required=True, help="directory for rgb_{i}.png (and normal_{i}.png, bump_{i}.png, ao_{i}.png)")
    ap.add_argument("--num_views", type=int, default=4)
    ap.add_argument("--normal", action="store_true", help="also write normal_{i}.png")
    ap.add_argument("--bump", action="store_true",
                    help="also write bump_{i}.png (mode normal_map) when the MTL names a map_Bump")
    ap.add_argument("--ao", action="store_true",
                    help="also write ao_{i}.png (mode ao) when the MTL names a map_Ka, and shade rgb_{i}.png with it")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ssaa", type=int, default=2)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    mesh, map_kd = load_obj(a.obj, device=dev)
    map_bump = load_normal_map(a.obj, device=dev) if a.bump else None
    map_ka = load_ao_map(a.obj, device=dev) if a.ao else None
    os.makedirs(a.out, exist_ok=True)
    modes = [("rgb", "rgb")] + ([("normal", "normal")] if a.normal else [])
    if map_bump is not None:
        modes.append(("bump", "normal_map"))
    if map_ka is not None:
        modes.append(("ao", "ao"))
    with torch.no_grad():
        for name, mode in modes:
            kw = {"map_Bump": map_bump} if mode == "normal_map" else {}
            if map_ka is not None and mode in ("rgb", "ao"):
                kw["map_Ka"] = map_ka
            imgs = turntable(mesh, map_kd, n_views=a.num_views, height=a.size, width=a.size, mode=mode, ssaa=a.ssaa,
                             **kw)
            for i, img in enumerate(imgs.cpu().numpy()):
                print(export.save_image(os.path.join(a.out, f"{name}_{i}.png"), export._rgb_u8(img)))


if __name__ == "__main__":
    main()
