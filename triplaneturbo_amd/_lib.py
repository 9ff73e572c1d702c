"""Build + load libtt_hip.so (the C-ABI HIP library, include/tt_abi.h) with ctypes.

There is NO fallback: if the shared library is missing or a symbol is absent the import of
any op fails loudly.  ``build()`` cross-compiles for gfx950 with hipcc (works without a GPU).
"""
from __future__ import annotations

import ast
import ctypes
import hashlib
import operator
import os
import re
import subprocess
import tempfile
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(_ROOT, "include")
LIB_PATH = os.path.join(_HERE, "libtt_hip.so")
# dev-only variant built with -DTT_TUNING: honours the TT_DEBUG_FLAGS / TT_SB / TT_CHUNK / TT_UNIT / TT_ORDER
# environment variables (profiling ablations and tuning sweeps, tools/).  The product library above never calls getenv.
_DEFAULT_LIB_PATH = LIB_PATH
TUNING_LIB_PATH = os.path.join(_HERE, "libtt_hip_tuning.so")
SOURCES = ["tt_forward.hip", "tt_march.hip", "tt_backward.hip", "tt_backward_tex.hip", "tt_points.hip", "tt_composite.hip", "tt_grad2.hip", "tt_sampler.hip", "tt_hashgrid.hip", "tt_isosurface.hip", "tt_tets.hip", "tt_raster.hip", "tt_texture.hip", "tt_mesh.hip", "tt_uv.hip", "tt_uv_lscm.hip", "tt_simplify.hip", "tt_decimate.hip", "tt_remesh.hip", "tt_bake.hip", "tt_dist.hip", "tt_wind.hip", "tt_ray.hip", "tt_host.cpp"]
# per-translation-unit flags: the texture backward is faster under hipcc's max-ILP scheduling strategy (3.11 -> 3.02 ms;
# the other kernels are not); the geometry backward is faster with its transient MFMA results in VGPRs rather than AGPRs
# (-amdgpu-mfma-vgpr-form: 471 -> 248 v_accvgpr_read, 3.045 -> 2.995 ms; texture backward slower, forward neutral) and
# without the scheduler's register-pressure rescheduling stage, which has nothing to win at one wave per SIMD
# (-amdgpu-disable-unclustered-high-rp-reschedule: 2.945 -> 2.865 ms; forward slower, texture neutral):
# profiles/experiments/README.md
# Round 6 (dense-rank scatter): the texture unit is now faster WITHOUT max-ILP and, like the geometry unit, without the
# register-pressure rescheduling stage (same-box A/B, texture backward 3.36 max-ilp / 3.32 no flags / 3.30 this).
# Register-form scatter operand: the texture unit now takes -amdgpu-mfma-vgpr-form as well -- with ebar^T
# held in registers across the three planes it spills 28-30 registers without the flag and none with it, and it is the
# faster setting on the parent's code too (same-box A/B 3.274 / 3.243 ms without / with: profiles/scatter_regs_ab.txt).
SOURCE_FLAGS = {"tt_backward_tex.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form",
                                        "-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"],
                "tt_backward.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form",
                                    "-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]}
# the -DTT_TUNING build only: with -amdgpu-mfma-vgpr-form hipcc (ROCm 7.2) crashes in its AGPR-copy rewrite pass on the
# texture unit's phase-timer + STATS instantiation (the pass that removes spills of reassigned registers: the product
# build's split-mode instantiations have none), so the tuning build keeps that unit's earlier flags
TUNING_SOURCE_FLAGS = {"tt_backward_tex.hip": ["-mllvm", "-amdgpu-disable-unclustered-high-rp-reschedule"]}
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fPIC", "-shared", "-fno-gpu-rdc"]

def _unit_flags(tuning: bool, source_flags: Optional[dict]) -> dict:
    """Per-translation-unit flags of a build: `source_flags` if given (dev A/B), else SOURCE_FLAGS (+ the tuning build's)."""
    if source_flags is not None:
        return dict(source_flags)
    return dict(SOURCE_FLAGS, **TUNING_SOURCE_FLAGS) if tuning else dict(SOURCE_FLAGS)


def _sources() -> List[str]:
    return [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]


def _expected_abi() -> int:
    if "TT_ABI_VERSION" not in _DEFINES:
        raise RuntimeError("include/tt_abi.h has no TT_ABI_VERSION")
    return _DEFINES["TT_ABI_VERSION"]


def _deps() -> List[str]:
    deps = _sources() + [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".h")]
    deps.append(os.path.join(INCLUDE, "tt_abi.h"))
    return deps


def source_hash(tuning: bool = False, defines: Optional[List[str]] = None, source_flags: Optional[dict] = None) -> str:
    """sha256 over every source / header of the library AND the flags it is built with.  build() embeds it in the
    binary (`tt_source_hash()`, marker string TT_SOURCE_HASH=...); needs_build() compares the embedded value with the
    tree, so a .so that travelled with equal or newer mtimes than its sources (a pushed tree, a checkout) is never
    silently reused for different sources."""
    h = hashlib.sha256()
    for d in _deps():
        h.update(os.path.basename(d).encode() + b"\0")
        h.update(open(d, "rb").read())
        h.update(b"\0")
    flags = _unit_flags(tuning, source_flags)
    h.update(repr((HIPCC_FLAGS, sorted(flags.items()), bool(tuning), list(defines or []))).encode())
    return h.hexdigest()


_HASH_RE = re.compile(rb"TT_SOURCE_HASH=([0-9a-f]{64})")


def embedded_hash(path: str) -> Optional[str]:
    """The source hash a built library carries (read from the file, no dlopen), or None."""
    try:
        m = _HASH_RE.search(open(path, "rb").read())
    except OSError:
        return None
    return m.group(1).decode() if m else None


def needs_build(path: str = LIB_PATH, tuning: bool = False, defines: Optional[List[str]] = None,
                source_flags: Optional[dict] = None) -> bool:
    if not os.path.exists(path):
        return True
    return embedded_hash(path) != source_hash(tuning, defines, source_flags)


_FLAG_OK: dict = {}


def _flag_supported(hipcc: str, pair: List[str]) -> bool:
    """Performance-only `-mllvm` options are hidden LLVM flags: probe each once on an empty translation unit, so that a
    hipcc without one of them builds the library without it (with a warning) instead of failing the whole build."""
    key = " ".join(pair)
    if key not in _FLAG_OK:
        with tempfile.TemporaryDirectory(prefix="tt_flag_") as d:
            src = os.path.join(d, "e.hip")
            open(src, "w").write("#include <hip/hip_runtime.h>\n__global__ void k() {}\n")
            base = [hipcc, "--offload-arch=gfx950", "-c", src, "-o", os.path.join(d, "e.o")]
            if subprocess.run(base, capture_output=True, text=True).returncode != 0:
                return True  # the probe itself does not compile here: keep the flag and let the real build speak
            r = subprocess.run(base + pair, capture_output=True, text=True)
        _FLAG_OK[key] = r.returncode == 0
        if r.returncode != 0:
            print(f"triplaneturbo_amd: hipcc rejects '{key}' (performance-only flag): building without it")
    return _FLAG_OK[key]


def _usable_flags(hipcc: str, flags: List[str]) -> List[str]:
    out, i = [], 0
    while i < len(flags):
        pair = flags[i:i + 2] if flags[i] == "-mllvm" else flags[i:i + 1]
        if flags[i] != "-mllvm" or _flag_supported(hipcc, pair):
            out += pair
        i += len(pair)
    return out


def build(force: bool = False, verbose: bool = False, tuning: bool = False, variant: Optional[str] = None,
          defines: Optional[List[str]] = None, source_flags: Optional[dict] = None) -> str:
    """hipcc --offload-arch=gfx950 ... -shared -> triplaneturbo_amd/libtt_hip.so (in-tree).  One hipcc process per
    translation unit, in parallel, then a link.  tuning=True builds the dev variant libtt_hip_tuning.so instead;
    variant="x" + defines=["-DFOO"] builds an experiment library libtt_hip_x.so (dev A/B runs, tools/ab.sh).
    Up to date = the source hash embedded in the library equals the hash of the tree (source_hash), not mtimes."""
    out = TUNING_LIB_PATH if tuning else LIB_PATH
    if variant:
        out = os.path.join(_HERE, f"libtt_hip_{variant}.so")
    if not force and not needs_build(out, tuning, defines, source_flags):
        return out
    # One builder at a time per output file: a multi-rank launch on a stale checkout (every rank's load() lands here) must not
    # compile and link concurrently into the same paths.  The ranks serialise on an fcntl lock next to the library; whoever
    # gets it SECOND finds the library up to date and returns.  Objects go to a per-process directory, the link to a
    # per-process temporary that os.replace() moves into place atomically.
    import fcntl
    import shutil
    os.makedirs(os.path.join(_HERE, "build"), exist_ok=True)
    with open(os.path.join(_HERE, "build", os.path.basename(out) + ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not needs_build(out, tuning, defines, source_flags):
                return out
            objdir = os.path.join(_HERE, "build", (variant or ("tuning" if tuning else "release")) + f".{os.getpid()}")
            try:
                return _build_locked(out, objdir, verbose, tuning, defines, source_flags)
            finally:
                shutil.rmtree(objdir, ignore_errors=True)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(out: str, objdir: str, verbose: bool, tuning: bool, defines: Optional[List[str]],
                  source_flags: Optional[dict]) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(objdir, exist_ok=True)
    digest = source_hash(tuning, defines, source_flags)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + (["-DTT_TUNING"] if tuning else []) + list(defines or [])
    flags.append(f'-DTT_SOURCE_HASH_STR="{digest}"')
    procs = []
    for s in _sources():
        obj = os.path.join(objdir, os.path.basename(s) + ".o")
        per_unit = _usable_flags(hipcc, _unit_flags(tuning, source_flags).get(os.path.basename(s), []))
        cmd = [hipcc] + flags + per_unit + ["-I", INCLUDE, "-I", CSRC, "-x", "hip", "-c", s, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((obj, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    objs = []
    for obj, pr in procs:
        so, se = pr.communicate()
        if pr.returncode != 0:
            raise RuntimeError(f"hipcc failed ({pr.returncode}):\n{so}\n{se}")
        objs.append(obj)
    tmp = f"{out}.{os.getpid()}.tmp"
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-fno-gpu-rdc"] + objs + ["-o", tmp]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc link failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    if embedded_hash(tmp) != digest:
        os.unlink(tmp)
        raise RuntimeError(f"{out} does not carry the source hash it was built with")
    os.replace(tmp, out)
    return out


def use_tuning_build() -> None:
    """Dev tools only: build and bind the -DTT_TUNING variant for the rest of this process (before the first op)."""
    global _lib, LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_tuning_build() must be called before the library is first loaded")
    LIB_PATH = build(tuning=True)


def use_variant(name: str) -> None:
    """Dev tools only: bind an experiment library built by build(variant=name, defines=[...]) (must exist already)."""
    global _lib, LIB_PATH
    if _lib is not None:
        raise RuntimeError("use_variant() must be called before the library is first loaded")
    path = os.path.join(_HERE, f"libtt_hip_{name}.so")
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is not built")
    LIB_PATH = path


_lib: Optional[ctypes.CDLL] = None

_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_F = ctypes.c_float


class MlpWeights(ctypes.Structure):
    _fields_ = [(n, _P) for n in ("w1", "w2", "w3", "v1", "v2", "v3")]


class RenderCfg(ctypes.Structure):
    _fields_ = [
        ("n_prompts", _I32), ("views_per_prompt", _I32), ("plane_h", _I32), ("plane_w", _I32),
        ("rays_per_view", _I32), ("n_samples", _I32), ("n_rays", _I64), ("radius", _F),
        ("sdf_bias_radius", _F), ("inv_std", _F), ("cos_anneal_ratio", _F), ("rgb_grad_shrink", _F),
        ("flags", _I32), ("image_w", _I32), ("tile_sb", _I32), ("grad_copies", _I32), ("tile_chunk", _I32),
        ("skip_eps_tex", _F), ("skip_eps_geo", _F), ("inv_std_dev", _P), ("stats", _P),
    ]


class HashGridCfg(ctypes.Structure):  # tt_hashgrid_cfg
    _fields_ = [("n_levels", _I32), ("n_features_per_level", _I32), ("log2_hashmap_size", _I32),
                ("base_resolution", _I32), ("per_level_scale", _F)]


_SCALARS = {"int": _I32, "int32_t": _I32, "int64_t": _I64, "float": _F, "double": ctypes.c_double}
_STRUCT_POINTERS = {"tt_mlp_weights": MlpWeights, "tt_mlp_grads": MlpWeights,  # same layout: six pointers
                    "tt_render_cfg": RenderCfg, "tt_hashgrid_cfg": HashGridCfg}
_PROTO_RE = re.compile(r"^[ \t]*((?:const\s+)?\w+\s*\*?)\s*(tt_\w+)\s*\(([^()]*)\)\s*;", re.M)
_PARAM_RE = re.compile(r"(?:const\s+)?(\w+)\s*(\*?)\s*\w*")
_DEFINE_RE = re.compile(r"^#define[ \t]+(TT_\w+)[ \t]+(\S.*?)[ \t]*$", re.M)
_ENUM_RE = re.compile(r"\benum\b[^{};]*\{([^{}]*)\}")
_FLOAT_RE = re.compile(r"(?=.*[.eE])(\d*\.?\d*(?:[eE][+-]?\d+)?)[fF]?")
_INT_OPS = {ast.LShift: operator.lshift, ast.Add: operator.add, ast.Sub: operator.sub}


def _ctype(decl: str, proto: str):
    """The ctypes type of one C return / parameter declaration (`proto` only names the prototype in the error)."""
    m = _PARAM_RE.fullmatch(decl.strip())
    base, star = m.groups() if m else (None, None)
    if star:
        if base == "char":
            return ctypes.c_char_p
        return ctypes.POINTER(_STRUCT_POINTERS[base]) if base in _STRUCT_POINTERS else _P
    if base not in _SCALARS:  # never guess: a wrong width shifts every argument behind it
        raise ValueError(f"include/tt_abi.h: {proto}: no ctypes type for {decl.strip()!r}")
    return _SCALARS[base]


def _int_expr(node: ast.AST) -> int:
    """An integer constant expression as a tree: integer literals, parentheses, <<, +, - and unary minus, nothing else."""
    if isinstance(node, ast.Constant) and type(node.value) is int:
        return node.value
    if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
        return -_int_expr(node.operand)
    if isinstance(node, ast.BinOp) and type(node.op) in _INT_OPS:
        return _INT_OPS[type(node.op)](_int_expr(node.left), _int_expr(node.right))
    raise ValueError(ast.dump(node))


def _constant(name: str, expr: str):
    """The value of one `#define TT_*` / enumerator: a float literal (its f suffix dropped) or an integer constant
    expression.  Parsed, never evaluated as code; anything else raises (never skip: a constant that silently went
    missing would come back as a hand-written copy)."""
    m = _FLOAT_RE.fullmatch(expr)
    try:
        return float(m.group(1)) if m else _int_expr(ast.parse(expr, mode="eval").body)
    except (SyntaxError, ValueError):
        raise ValueError(f"include/tt_abi.h: {name}: no constant for {expr!r}") from None


def _parse_abi(text: Optional[str] = None):
    """include/tt_abi.h (or `text`) as ({name: (restype, argtypes)} of every tt_* prototype, {name: value} of every
    value-carrying #define TT_* and every enumerator).  The header is the one description of the C ABI: load() binds
    from this, SYMBOLS and the TT_* constants below are read from it."""
    if text is None:
        text = open(os.path.join(INCLUDE, "tt_abi.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = {}
    for ret, name, params in _PROTO_RE.findall(text):
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (_ctype(ret, name), [_ctype(p, name) for p in params])
    consts = _DEFINE_RE.findall(text)
    for body in _ENUM_RE.findall(text):  # enumerators carry explicit values here: `NAME = value`, nothing to count
        consts += [tuple(x.strip() for x in item.partition("=")[::2]) for item in body.split(",") if item.strip()]
    return protos, {name: _constant(name, expr) for name, expr in consts}


_PROTOS, _DEFINES = _parse_abi()
SYMBOLS = list(_PROTOS)  # every symbol include/tt_abi.h declares
globals().update(_DEFINES)  # TT_R_*, TT_Q_*, TT_ERR_*, TT_MESH_MAX_ITEMS, TT_UV_DEFAULT_TAU, ... as module attributes

# Precision of the per-point MLP products (include/tt_abi.h, "precision of the matrix products"):
#   "split3" (default)  fp32-grade: three fp16 pieces per operand, six product terms on the fp16 matrix pipe
#   "f32"               every product on the fp32-input MFMA (the A/B reference)
#   "split2"            the FAST mode: two pieces, three terms, ~2^-21.5 per product (tolerance-bounded)
DEFAULT_PRECISION = "split3"
_PRECISION_FLAGS = {"split3": (_DEFINES["TT_R_SPLIT3"], _DEFINES["TT_Q_SPLIT3"]),
                    "split2": (_DEFINES["TT_R_SPLIT2"], _DEFINES["TT_Q_SPLIT2"]),
                    "f32": (_DEFINES["TT_R_EXACT_F32"], _DEFINES["TT_Q_EXACT_F32"])}
_PRECISION_ALIASES = {"fast": "split2", "exact_f32": "f32", "fp32_mfma": "f32"}


def resolve_precision(precision: Optional[str] = None, exact_f32: bool = False) -> str:
    """Canonical precision name.  `exact_f32=True` (the switch of rounds 2-4) means "f32"; naming both is an error
    unless they agree."""
    if precision is None:
        return "f32" if exact_f32 else DEFAULT_PRECISION
    name = _PRECISION_ALIASES.get(precision, precision)
    if name not in _PRECISION_FLAGS:
        raise ValueError(f"unknown precision {precision!r}: one of {sorted(_PRECISION_FLAGS)} / {sorted(_PRECISION_ALIASES)}")
    if exact_f32 and name != "f32":
        raise ValueError(f"exact_f32=True contradicts precision={precision!r}")
    return name


def r_flag(name: str) -> int:
    return _PRECISION_FLAGS[name][0]


def q_flag(name: str) -> int:
    return _PRECISION_FLAGS[name][1]


PLACEMENTS = {"tt": _DEFINES["TT_PLACE_TT"], "center": _DEFINES["TT_PLACE_CENTER"]}  # enum tt_sample_placement


def load() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (hipcc --offload-arch=gfx950). triplaneturbo_amd has no CPU/PyTorch fallback.")
    if LIB_PATH == _DEFAULT_LIB_PATH and embedded_hash(LIB_PATH) != source_hash():
        # a library built from OTHER sources (an edited checkout, a stale copy): never bind it silently -- rebuild in-tree,
        # or say so when there is no compiler (dev variants bound by use_variant / use_tuning_build carry their own hash)
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        if not os.path.exists(hipcc):
            raise RuntimeError(f"{LIB_PATH} was built from different sources than this checkout (embedded hash "
                               f"{embedded_hash(LIB_PATH)}, tree {source_hash()}) and {hipcc} is not there to rebuild it")
        build()
    lib = ctypes.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise RuntimeError(f"{LIB_PATH} lacks symbols {missing}; rebuild it")
    if lib.tt_abi_version() != _expected_abi():  # (int (void): callable before it is bound)
        # argument lists moved between ABI versions: calling a stale library would shift pointer arguments
        raise RuntimeError(f"{LIB_PATH} has ABI version {lib.tt_abi_version()}, include/tt_abi.h declares "
                           f"{_expected_abi()}: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    for name, (restype, argtypes) in _PROTOS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != 0:
        raise RuntimeError(f"{what} failed: {load().tt_strerror(status).decode()} ({status})")
