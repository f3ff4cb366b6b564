"""ctypes binding of libgraphode.so, derived at import from include/graphode.h (the one statement of the C ABI).

The library is the product: if it is missing, every op raises.  There is no
eager/PyTorch fallback behind these calls.
"""
import ctypes
import os

import torch  # noqa: F401  (imported first so that libamdhip64 is torch's copy)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgraphode.so")

HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "graphode.h"))


class GraphodeLibraryError(RuntimeError):
    pass


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise GraphodeLibraryError("graphode.h not found at %s - the binding is derived from it. "
                                   "There is no fallback table." % HEADER_PATH)
    with open(HEADER_PATH) as f:
        return _abi.parse(f.read())


# CONSTANTS: the header's `#define GODE_NAME <integer>`; STRUCTS: typedef name -> ctypes.Structure;
# SIGNATURES: name -> (restype, argtypes), also the list the symbol-export test walks.
CONSTANTS, STRUCTS, SIGNATURES = _read_header()
GODE_MAX_TERMS = CONSTANTS["GODE_MAX_TERMS"]
GODE_ADAM_MAX_TENSORS = CONSTANTS["GODE_ADAM_MAX_TENSORS"]

LinComb = STRUCTS["gode_lincomb_t"]
SpmmEpilogue = STRUCTS["gode_spmm_epilogue_t"]
Graph = STRUCTS["gode_graph_t"]
GcnOdeFunc = STRUCTS["gode_gcn_odefunc_t"]
GatProj = STRUCTS["gode_gat_proj_t"]                 # member `as` is `as_` here (Python keyword)
GatAct = STRUCTS["gode_gat_act_t"]
Rk4Workspace = STRUCTS["gode_rk4_workspace_t"]
ReduceSeg = STRUCTS["gode_reduce_seg_t"]
GatOdeFunc = STRUCTS["gode_gat_odefunc_t"]
GatWorkspace = STRUCTS["gode_gat_workspace_t"]
AdamArgs = STRUCTS["gode_adam_args_t"]

_lib = None


def load():
    """Load libgraphode.so or raise; never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GraphodeLibraryError(
            "libgraphode.so not found at %s - build it with `python __graft_entry__.py` "
            "(or `make -C graph_odenet_amd/csrc`). There is no fallback path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: loud by design
        fn.restype = res
        fn.argtypes = args
    if lib.gode_abi_version() != 1:
        raise GraphodeLibraryError("libgraphode.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gode_error_string(rc)
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg.decode() if msg else "?", rc))


def lincomb(terms):
    """terms: list of (coef, tensor) -> LinComb struct (keeps no references; caller keeps tensors alive)."""
    lc = LinComb()
    terms = [(c, t) for (c, t) in terms if t is not None]
    if len(terms) > GODE_MAX_TERMS:
        raise ValueError("too many lincomb terms")
    lc.n = len(terms)
    for j, (c, t) in enumerate(terms):
        lc.coef[j] = float(c)
        lc.ptr[j] = t.data_ptr()
    return lc


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def current_stream_handle(device_index=None):
    """hipStream_t of torch's current stream on the (current) device as an int.  torch.cuda.current_stream() builds a
    Stream object (~10 us); this is the raw query underneath it (~0.3 us) - every launch through the ABI asks once, and an
    eager QC step or an adaptive solve makes hundreds of them."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device() if device_index is None else device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


def stream_ptr():
    return ctypes.c_void_p(current_stream_handle())


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None
