"""The h2 sign-mask entries are ADDITIVE: include/tt_abi.h declares tt_render_fwd_h2mask / tt_render_bwd_geo_h2mask next to
the entries they extend, the binding reads them from the header, the built library exports them, and the ABI version stays
17 (tt_render_cfg and every existing signature are unchanged)."""
import ctypes

from triplaneturbo_amd import _lib


def _argtypes(name):
    return _lib._PROTOS[name][1]


def test_header_declares_the_mask_entries_as_extensions():
    for base, ext in (("tt_render_fwd", "tt_render_fwd_h2mask"), ("tt_render_bwd_geo", "tt_render_bwd_geo_h2mask")):
        assert ext in _lib.SYMBOLS
        a, b = _argtypes(base), _argtypes(ext)
        # = the base entry's arguments + the mask pointer in front of the stream
        assert len(b) == len(a) + 1
        assert b[:len(a) - 1] == a[:-1] and b[-2] is ctypes.c_void_p and b[-1] == a[-1]
        assert _lib._PROTOS[ext][0] is ctypes.c_int32
    assert _lib._DEFINES["TT_ABI_VERSION"] == 17


def test_library_exports_and_binds_the_mask_entries():
    path = _lib.build()  # hipcc cross-compiles for gfx950 without a GPU; no-op when up to date
    lib = ctypes.CDLL(path)
    lib.tt_abi_version.restype = ctypes.c_int
    assert lib.tt_abi_version() == 17
    for name in ("tt_render_fwd_h2mask", "tt_render_bwd_geo_h2mask"):
        assert hasattr(lib, name), name


def test_render_config_defaults_to_the_mask_path():
    from triplaneturbo_amd import ops
    assert ops.RenderConfig().fwd_mask is True
    assert ops.RenderConfig(precision="split2", tile_sb=2, tile_chunk=0, grad_copies=1).fwd_mask is True
    assert ops.RenderConfig(fwd_mask=False).fwd_mask is False
