"""ctypes binding of ``csrc/libnarfs2.so``, derived from its C-ABI header ``include/nar_fs2.h``.

The header is read when this module is imported (``_abi.py`` states the subset of C and the type rule): every prototype becomes
an entry of ``SIGNATURES``, every struct with a body a ``ctypes.Structure`` with the header's field names, order and nesting, and
every integer ``#define`` an entry of ``NS``.  Nothing here restates a signature, a layout or a value.

There is no CPU fallback: if the header or the library is missing or a symbol is absent the import fails loudly.  ``torch`` is
imported first on purpose — it brings its own ``libamdhip64.so.7`` and the library must bind to that same HIP runtime so that
torch's device pointers and streams are valid in our launches.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede the CDLL: one HIP runtime per process)

from ._abi import Abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libnarfs2.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "nar_fs2.h")
if not os.path.exists(HEADER_PATH):
    raise ImportError(f"{HEADER_PATH} is missing: the binding is read from the C-ABI header, which stays next to the package")
with open(HEADER_PATH, encoding="utf-8") as _f:
    ABI = Abi(_f.read(), HEADER_PATH)

NS = ABI.constants           # every `#define NS_X <integer>`: NS["NS_KM_GRID_CAP"]
SIGNATURES = ABI.signatures  # name -> (restype, argtypes), one entry per prototype
STRUCTS = ABI.structs        # C name -> Structure

NsConfig = STRUCTS["ns_config"]
NsLossArgs = STRUCTS["ns_loss_args"]
NsLossgGrads = STRUCTS["ns_lossg_grads"]
NsVtState = STRUCTS["ns_vt_state"]
NsVtArgs = STRUCTS["ns_vt_args"]
NsOptTensor = STRUCTS["ns_opt_tensor"]
NsOptPlan = STRUCTS["ns_opt_plan"]
NsOptRecord = STRUCTS["ns_opt_record"]
NsOptHyper = STRUCTS["ns_opt_hyper"]
NsPgShape = STRUCTS["ns_pg_shape"]
NsPgWeights = STRUCTS["ns_pg_weights"]
NsPgGrads = STRUCTS["ns_pg_grads"]
NsAgShape = STRUCTS["ns_ag_shape"]
NsAgWeights = STRUCTS["ns_ag_weights"]
NsAgGrads = STRUCTS["ns_ag_grads"]
NsXgShape = STRUCTS["ns_xg_shape"]
NsXgWeights = STRUCTS["ns_xg_weights"]
NsXgGrads = STRUCTS["ns_xg_grads"]
NsPnShape = STRUCTS["ns_pn_shape"]
NsPnWeights = STRUCTS["ns_pn_weights"]
NsPnGrads = STRUCTS["ns_pn_grads"]
NsFgShape = STRUCTS["ns_fg_shape"]
NsFgWeights = STRUCTS["ns_fg_weights"]
NsFgGrads = STRUCTS["ns_fg_grads"]
NsMeShape = STRUCTS["ns_me_shape"]
NsMeWeights = STRUCTS["ns_me_weights"]
NsMeGrads = STRUCTS["ns_me_grads"]
NsMhShape = STRUCTS["ns_mh_shape"]
NsMhWeights = STRUCTS["ns_mh_weights"]
NsMhGrads = STRUCTS["ns_mh_grads"]
NsKmMask = STRUCTS["ns_km_mask"]
NsMelConfig = STRUCTS["ns_mel_config"]
NsGlConfig = STRUCTS["ns_gl_config"]


def fields(c_name: str) -> tuple:
    """Field names of a struct, in the header's order."""
    return tuple(n for n, _ in STRUCTS[c_name]._fields_)


# the parameters of each trainable layer in checkpoint order = the fields of its weights struct
PG_NAMES, AG_NAMES, FG_NAMES, ME_NAMES, MH_NAMES = (fields(f"ns_{p}_weights") for p in ("pg", "ag", "fg", "me", "mh"))
PN_MAX_LAYERS = NS["NS_PN_MAX_LAYERS"]
PN_PARAMS = fields("ns_pn_layer_grads")                      # per PostNet layer
PN_BUFFERS = fields("ns_pn_layer")[len(PN_PARAMS):]          # what follows them in ns_pn_layer

KM_MAX_MASKS, KM_GRID_CAP, KM_TABLE_ROW_BYTES = NS["NS_KM_MAX_MASKS"], NS["NS_KM_GRID_CAP"], NS["NS_KM_TABLE_ROW_BYTES"]
STATUS_TRUNCATED, STATUS_BAD_TOKEN = NS["NS_STATUS_TRUNCATED"], NS["NS_STATUS_BAD_TOKEN"]

_lib = None


def load():
    """Load the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for this path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = load().ns_last_error()
        raise RuntimeError(f"{what}: {msg.decode() if msg else 'error'} (rc={rc})")


def ptr(t, struct=None):
    """Device (or host) pointer of a contiguous tensor; None -> NULL.  ``struct``: the Structure the memory holds, for the
    parameters the header types as a pointer to it (``ns_vt_state*``, ``ns_opt_record*``: device memory)."""
    assert t is None or t.is_contiguous(), "tensor must be contiguous"
    p = C.c_void_p(0 if t is None else t.data_ptr())
    return p if struct is None else C.cast(p, C.POINTER(struct))


def stream_ptr(device=None) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
