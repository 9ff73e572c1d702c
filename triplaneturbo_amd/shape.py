"""Guide-shape occupancy loss on the GPU: MeshOBJ, ce_pq_loss and ShapeLoss with the names, signatures, shapes and
devices of threestudio/utils/ops.py:482-584 (the Latent-NeRF shape loss), on the HIP winding number and point-to-mesh
distance (include/tt_abi.h, "winding number" and "point-to-mesh distance") in place of libigl.  The query never leaves
the GPU.

    before:  from threestudio.utils.ops import MeshOBJ, ShapeLoss, ce_pq_loss
    after:   from triplaneturbo_amd.shape import MeshOBJ, ShapeLoss, ce_pq_loss

Two deliberate differences: the winding number is this project's dipole tree at beta = 2 (libigl's fast winding number is
an expansion of another order; both approximate the same exact sum), and the squared distance is exact in fp32."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch import Tensor

from . import ops
from .viewer import read_obj_geometry

_AXES = torch.eye(3, dtype=torch.float32)


class MeshOBJ:
    """A guide mesh held as numpy arrays: v (V,3) float, f (T,3) int.  Keeps the reference's attributes (v_tensor,
    f_center, face_normals and their tensors, the unit axes dx, dy, dz as (1,3) tensors).  The GPU structures of a
    query (ops.WindingTree, ops.TriangleGrid) are built on the query's device at its first use and kept."""

    dx, dy, dz = _AXES[0:1], _AXES[1:2], _AXES[2:3]

    def __init__(self, v: np.ndarray, f: np.ndarray):
        self.v = v
        self.f = f
        self.dx, self.dy, self.dz = MeshOBJ.dx, MeshOBJ.dy, MeshOBJ.dz
        self.v_tensor = torch.from_numpy(self.v)
        corners = self.v[self.f, :]
        self.f_center = corners.mean(axis=1)
        self.f_center_tensor = torch.from_numpy(self.f_center).float()
        n = np.cross(corners[:, 1, :] - corners[:, 0, :], corners[:, 2, :] - corners[:, 0, :])
        with np.errstate(invalid="ignore", divide="ignore"):  # a face without area has no normal (NaN), as in the reference
            self.face_normals = n / np.linalg.norm(n, axis=-1)[:, None]
        self.face_normals_tensor = torch.from_numpy(self.face_normals)
        self._gpu: Dict[torch.device, Tuple[Tensor, Tensor, ops.WindingTree, ops.TriangleGrid]] = {}

    def normalize_mesh(self, target_scale=0.5):
        """A new MeshOBJ about the mean of the vertices, the farthest vertex at distance target_scale."""
        centred = self.v - self.v.mean(axis=0)
        return MeshOBJ(centred / np.max(np.linalg.norm(centred, axis=1)) * target_scale, self.f)

    def _on(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError("MeshOBJ queries run on the GPU (triplaneturbo_amd has no CPU path): move the query there")
        device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
        if device not in self._gpu:
            v = torch.from_numpy(np.ascontiguousarray(self.v, dtype=np.float32)).to(device)
            f = torch.from_numpy(np.ascontiguousarray(self.f).astype(np.int32)).to(device)
            self._gpu[device] = (v, f, ops.WindingTree(v, f), ops.TriangleGrid(v, f))
        return self._gpu[device]

    @torch.no_grad()
    def winding_number(self, query: Tensor) -> Tensor:
        """w of every point of query (..., 3): shape query.shape[:-1], fp32, on query's device."""
        _, _, tree, _ = self._on(query.device)
        flat = query.detach().reshape(-1, 3).float()
        return ops.mesh_winding_number(flat, tree).reshape(query.shape[:-1])

    @torch.no_grad()
    def gaussian_weighted_distance(self, query: Tensor, sigma) -> Tensor:
        """exp(-d2 / (2 sigma^2)) with d2 the squared distance of every point of query (..., 3) to the mesh."""
        _, _, _, tg = self._on(query.device)
        d2 = ops.mesh_closest_point(query.detach().reshape(-1, 3).float(), tg)[0].reshape(query.shape[:-1])
        return torch.exp(-(d2 / (2 * sigma ** 2)))


def ce_pq_loss(p, q, weight=None):
    """Summed cross entropy -(p log q + (1 - p) log(1 - q)), q and 1 - q clamped to [1e-4, 1 - 1e-4], p viewed in q's
    shape, times `weight` when given."""
    floor = 1e-4
    log_q = q.clamp(floor, 1 - floor).log()
    log_not_q = (1 - q).clamp(floor, 1 - floor).log()
    occupancy = p.reshape(q.shape)
    terms = occupancy * log_q + (1 - occupancy) * log_not_q
    return -(terms if weight is None else terms * weight).sum()


class ShapeLoss(nn.Module):
    """Occupancy loss towards a guide shape: the density's occupancy 1 - exp(-delta sigma) (clamped to [0, 1.1])
    against the indicator w > 0.5 of the guide mesh, weighted by 1 - exp(-d2 / (2 proximal_surface^2)).  The mesh is the
    OBJ at `guide_shape`, centred on its vertex mean, scaled so that its farthest vertex is at mesh_scale, and rotated
    by R_x(90 deg) R_y(90 deg).  The gradient reaches `sigmas` only."""

    def __init__(self, guide_shape):
        super().__init__()
        self.mesh_scale = 0.7
        self.proximal_surface = 0.3
        self.delta = 0.2
        self.shape_path = guide_shape
        v, f = read_obj_geometry(self.shape_path)
        rot_x = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]])
        rot_y = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]])
        scaled = MeshOBJ(v, f).normalize_mesh(self.mesh_scale)
        self.sketchshape = MeshOBJ(np.ascontiguousarray(scaled.v @ (rot_x @ rot_y).T), f)

    def forward(self, xyzs, sigmas):
        guide = self.sketchshape
        inside = (guide.winding_number(xyzs) > 0.5).to(sigmas.dtype)  # a constant: no gradient reaches xyzs
        density_occupancy = torch.clamp(1 - torch.exp(-self.delta * sigmas), 0, 1.1)
        away_from_surface: Optional[Tensor] = None
        if self.proximal_surface > 0:  # the loss fades towards the guide's surface
            away_from_surface = 1 - guide.gaussian_weighted_distance(xyzs, self.proximal_surface)
        return ce_pq_loss(density_occupancy, inside, weight=away_from_surface)
