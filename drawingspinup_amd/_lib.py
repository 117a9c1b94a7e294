"""ctypes binding of libdsu_hip.so, derived from include/dsu_hip.h.

The header is the single statement of the C ABI: _header.py reads its integer #defines, struct
definitions and prototypes at import, and everything here (the Structure classes, DEFINES, the
argument and return types lib() sets) comes from that reading.  A new entry point is declared in the
header and defined in its .hip file; nothing is restated in Python.

There is no CPU fallback: if the shared library is missing, or a kernel is asked to run
on a non-GPU tensor, the call raises.  `python -m drawingspinup_amd.build` (or
`__graft_entry__.build()`) produces the library in-tree.
"""
import ctypes as C
import os

import torch

from ._header import DsuError, read as _read_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSU_HIP_LIB=<path>: load a variant built by `python -m drawingspinup_amd.build --variant ...`
# (A/B measurements); unset = the in-tree library.
LIB_PATH = os.environ.get("DSU_HIP_LIB") or os.path.join(_HERE, "libdsu_hip.so")

_HEADER = _read_header()
DEFINES = _HEADER.defines                              # DSU_* integer constants of the header
MAX_LEVELS = DEFINES["DSU_MAX_LEVELS"]
ADAMW_MAX_TENSORS = DEFINES["DSU_ADAMW_MAX_TENSORS"]
ABI_VERSION = DEFINES["DSU_ABI_VERSION"]              # lib() refuses a library built from another one

_STRUCT_NAMES = {
    "dsu_hashgrid_cfg": "HashGridCfg", "dsu_hashgrid_levels": "HashGridLevels", "dsu_sdf_mlp": "SdfMlp",
    "dsu_tex_mlp": "TexMlp", "dsu_partial_reduce": "PartialReduce",
    "dsu_occgrid_refresh_args": "OccRefreshArgs", "dsu_render_texture": "RenderTexture",
    "dsu_norm_cfg": "NormCfg", "dsu_ray_loss_cfg": "RayLossCfg", "dsu_adamw_tensor": "AdamwTensor",
    "dsu_nsr_driver_cfg": "NsrDriverCfg", "dsu_nsr_step_args": "NsrStepArgs"}
for _c, _py in _STRUCT_NAMES.items():
    _HEADER.structs[_c].__name__ = _HEADER.structs[_c].__qualname__ = _py
    globals()[_py] = _HEADER.structs[_c]

_PROTOS = {name: args for name, (_, args) in _HEADER.protos.items()}      # name -> argtypes

_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DsuError(
                f"{LIB_PATH} is missing: the HIP extension is not built "
                "(run `python -m drawingspinup_amd.build`). There is no CPU fallback.")
        h = C.CDLL(LIB_PATH)
        if h.dsu_abi_version() != ABI_VERSION:         # before the table: a stale library may lack its names
            raise DsuError(f"{LIB_PATH} has ABI version {h.dsu_abi_version()}, this package binds version "
                           f"{ABI_VERSION}: rebuild it (`python -m drawingspinup_amd.build`).")
        for name, (restype, args) in _HEADER.protos.items():
            fn = getattr(h, name)  # AttributeError here = header/library mismatch
            fn.restype, fn.argtypes = restype, args
        _lib = h
    return _lib


def check(rc, what):
    if rc != 0:
        raise DsuError(f"{what} failed: {lib().dsu_strerror(rc).decode()} ({rc})")


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor; None -> NULL."""
    if t is None:
        return None
    if not t.is_cuda:
        raise DsuError("libdsu_hip kernels need device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise DsuError("libdsu_hip kernels need contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise DsuError(f"expected dtype {dtype}, got {t.dtype}")
    return C.c_void_p(t.data_ptr())


def publish_sync(device=None):
    """Before a lazily built device tensor goes into a process-wide cache: wait for the stream that
    produced it.  Several drawings may be in flight on one GPU (one Python thread + one stream each,
    bench.py --inflight): another thread's stream must not read a cached table ahead of the copies /
    kernels that fill it."""
    if torch.cuda.is_available() and torch.cuda.is_initialized() and (device is None or torch.device(device).type == "cuda"):
        torch.cuda.current_stream(device).synchronize()


def stream():
    """Raw handle of torch's current stream on the current device.  (The public
    torch.cuda.current_stream() wrapper costs ~9 us per call: 0.17 ms of a 2 ms optimisation
    step that launches ~100 kernels.)"""
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


def hashgrid_levels(cfg: HashGridCfg):
    """Host-only level table (works without a GPU)."""
    lv = HashGridLevels()
    check(lib().dsu_hashgrid_make_levels(C.byref(cfg), C.byref(lv)), "dsu_hashgrid_make_levels")
    n = cfg.n_levels
    return {
        "offsets": [lv.offsets[i] for i in range(n + 1)],
        "resolution": [lv.resolution[i] for i in range(n)],
        "scale": [lv.scale[i] for i in range(n)],
        "hashed": [lv.hashed[i] for i in range(n)],
    }
