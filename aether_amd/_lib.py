"""ctypes binding of libaether_hip.so, derived at import from include/aether_hip.h (_header.py): the header's structs,
integer #defines and prototypes are the only statement of the ABI, and a new entry point needs no edit here.

The product path has no CPU fallback: if the library is missing or a call fails,
the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os

from ._header import AetherHipError, parse

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libaether_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "aether_hip.h")      # where build.py finds it too

# Order and names follow struct AetherParams in include/aether_hip.h; the second
# element is the reference state_dict key.
PARAM_FIELDS = [
    ("field_w0", "field_net.net.0.weight"), ("field_b0", "field_net.net.0.bias"),
    ("field_w2", "field_net.net.2.weight"), ("field_b2", "field_net.net.2.bias"),
    ("field_w4", "field_net.net.4.weight"), ("field_b4", "field_net.net.4.bias"),
    ("field_emb", "field_net.class_embedding.weight"),
    ("l1_msg_w0", "gnn.layer_1.message_fn.0.weight"), ("l1_msg_b0", "gnn.layer_1.message_fn.0.bias"),
    ("l1_msg_w2", "gnn.layer_1.message_fn.2.weight"), ("l1_msg_b2", "gnn.layer_1.message_fn.2.bias"),
    ("l1_res_w", "gnn.layer_1.res.weight"), ("l1_res_b", "gnn.layer_1.res.bias"),
    ("l1_upd_w0", "gnn.layer_1.update_fn.0.weight"), ("l1_upd_b0", "gnn.layer_1.update_fn.0.bias"),
    ("l1_upd_w2", "gnn.layer_1.update_fn.2.weight"), ("l1_upd_b2", "gnn.layer_1.update_fn.2.bias"),
    ("ln_msg_w0", "gnn.layer_{}.message_fn.0.weight"), ("ln_msg_b0", "gnn.layer_{}.message_fn.0.bias"),
    ("ln_msg_w2", "gnn.layer_{}.message_fn.2.weight"), ("ln_msg_b2", "gnn.layer_{}.message_fn.2.bias"),
    ("ln_upd_w0", "gnn.layer_{}.update_fn.0.weight"), ("ln_upd_b0", "gnn.layer_{}.update_fn.0.bias"),
    ("ln_upd_w2", "gnn.layer_{}.update_fn.2.weight"), ("ln_upd_b2", "gnn.layer_{}.update_fn.2.bias"),
    ("out_w0", "gnn.out_mlp.0.weight"), ("out_b0", "gnn.out_mlp.0.bias"),
    ("out_w3", "gnn.out_mlp.3.weight"), ("out_b3", "gnn.out_mlp.3.bias"),
    ("out_w6", "gnn.out_mlp.6.weight"), ("out_b6", "gnn.out_mlp.6.bias"),
]

S2S_LAUNCH_KINDS = ("k_s2s_linear_jobs", "k_s2s_gemm_split<1>", "k_s2s_gemm_split<2>", "k_s2s_gemm_split_r1<1>",
                    "k_s2s_gemm_split_r1<2>")

# The structs this module has always exported as binding types: a pointer to one of them is POINTER(struct) in SIGNATURES.
# Every other pointer is c_void_p, so a data_ptr(), a byref() or (host-only tests) any non-null integer passes.
TYPED_POINTERS = ("AetherParams", "AetherGraphInfo", "AetherS2SLaunchStats", "AetherDynScenePack")


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse(f.read(), TYPED_POINTERS)
    except OSError as e:
        raise AetherHipError(f"{HEADER_PATH} cannot be read ({e}): the binding is derived from it") from e


# {AETHER_NAME: int}, {struct name: ctypes.Structure}, {function: (restype, argtypes)}: everything the header declares
CONSTANTS, STRUCTS, SIGNATURES = _read_header()
globals().update(STRUCTS)                                # every struct under its header name: _lib.AetherS2SPriorParams, ...
AetherParams, AetherGraphInfo, AetherS2SLaunchStats, AetherDynScenePack = (STRUCTS[n] for n in TYPED_POINTERS)
globals().update({k[len("AETHER_"):]: v for k, v in CONSTANTS.items()      # FLAG_*, EGNN_*, CLOF_*: the calls' flag bits
                  if k.startswith(("AETHER_FLAG_", "AETHER_EGNN_", "AETHER_CLOF_"))})
S2S_LAUNCH_LOG = CONSTANTS["AETHER_S2S_LAUNCH_LOG"]
assert len(S2S_LAUNCH_KINDS) == CONSTANTS["AETHER_S2S_LAUNCH_KINDS"], "S2S_LAUNCH_KINDS: the header counts other kinds"
assert [n for n, _ in AetherParams._fields_] == [n for n, _ in PARAM_FIELDS], "PARAM_FIELDS: not the header's AetherParams"


def params_struct(tensors: dict) -> AetherParams:
    """Fill an AetherParams from {state_dict key: tensor-like with .data_ptr()}."""
    p = AetherParams()
    for name, key in PARAM_FIELDS:
        if "{}" in key:
            arr = (C.c_void_p * 3)(*[tensors[key.format(l)].data_ptr() for l in (2, 3, 4)])
            setattr(p, name, arr)
        else:
            setattr(p, name, tensors[key].data_ptr())
    return p


_lib = None


def load(path=None):
    """Load the library (once).  Raises if it has not been built.  ``path``: load that build instead (an older one as a
    timing yardstick, tools/s2s_charges_time.py --lib); entries it does not have yet stay unbound."""
    global _lib
    if _lib is not None:
        return _lib
    lib_path = LIB_PATH if path is None else os.path.abspath(path)
    if not os.path.exists(lib_path):
        raise AetherHipError(
            f"{lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `python aether_amd/build.py`).  There is no CPU fallback.")
    lib = C.CDLL(lib_path)
    for name, (res, args) in SIGNATURES.items():
        if path is not None and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what):
    if status < 0:
        msg = load().aether_last_error().decode()
        raise AetherHipError(f"{what} failed ({status}): {msg}")
    return status
