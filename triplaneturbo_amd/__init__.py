"""triplaneturbo_amd -- MI355X-native (gfx950) triplane volume-render hot path of TriplaneTurbo.

Host side: Python on PyTorch-ROCm (memory, streams, torch.distributed).  Compute: hand-written HIP
kernels in libtt_hip.so behind the C ABI of include/tt_abi.h.  No CPU fallback.

    from triplaneturbo_amd import find, register      # threestudio-style plugin registry
    Renderer = find("generative-space-sdf-volume-renderer")
    from triplaneturbo_amd.isosurface import DiffMarchingCubeHelper, isosurface, colorize_mesh  # mesh extraction
    from triplaneturbo_amd.export import save_obj      # `multiprompt-mesh-exporter` + OBJ / MTL / texture files
    from triplaneturbo_amd.viewer import load_obj, turntable   # read the export back, textured turntable renders
"""
from . import _lib  # noqa: F401
from . import isosurface  # noqa: F401
from .registry import C, find, register  # noqa: F401


def _register_plugins():
    from . import background, export, geometry, mesh_renderer, renderer  # noqa: F401  (import = registration)


_register_plugins()
__all__ = ["find", "register", "C"]
