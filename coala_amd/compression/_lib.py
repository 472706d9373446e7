"""ctypes binding of the codec's C ABI (include/coalac.h) — the only way the host side reaches the GPU.

There is deliberately no CPU fallback: if the HIP library is missing or cannot be loaded, every codec
call raises. (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes
import os
import threading

from .. import _build

COALAC_FLAG_FORCE_EXACT = 1
COALAC_FLAG_GENERIC_SELECT = 2
COALAC_FLAG_STAMPS = 4
COALAC_FLAG_NO_FORK = 8
COALAC_AGG_DIV = 0     # acc / total            (torch CPU division by a scalar)
COALAC_AGG_RECIP = 1   # acc * (1.0f / total)   (torch GPU division by a host scalar)
COALAC_AGG_SUM = 2     # acc                    (weighted_sum: the multi-GPU per-rank sum)
COALAC_AGGD_CODES = 0   # coalac_aggregate_dense reads uint8 codes, one range per segment (wire v2 dense)
COALAC_AGGD_PACKED = 1  # ... the wire v4 stream, one range per segment
COALAC_AGGD_BLOCK = 2   # ... the wire v4 stream, one range per 4096-element block (wire v5)
COALAC_AGGS_ENTRIES = 0  # coalac_aggregate_uploads reads each upload's idx / vals arrays (wire v2)
COALAC_AGGS_COMPACT = 1  # ... each upload's wire v3 stream
AGGD_DEPTH = 4          # clients whose code words k_aggregate_dense loads together (AGD_DEPTH in coalac.hip)

ERRORS = {
    -1: "COALAC_EINVAL",
    -2: "COALAC_EBITS",
    -3: "COALAC_EWORKSPACE",
    -4: "COALAC_EHIP",
    -5: "COALAC_EDEVICE",
    -6: "COALAC_ENOMEM",
}

# every symbol include/coalac.h declares: (name, restype, argtypes)
_P = ctypes.c_void_p
_U64 = ctypes.c_uint64
_I = ctypes.c_int
SIGNATURES = [
    ("coalac_version", _I, []),
    ("coalac_last_error", ctypes.c_char_p, []),
    ("coalac_plan_create", _I, [_P, _I, _I, ctypes.POINTER(_P)]),
    ("coalac_plan_destroy", _I, [_P]),
    ("coalac_plan_query", _I, [_P, ctypes.POINTER(_U64), ctypes.POINTER(_U64), ctypes.POINTER(_U64),
                               ctypes.POINTER(_U64)]),
    # encode: plan, in / seg pointers, base, idx, vals, mn, scale, ustart, ws, ws_bytes, flags, stream (+ events)
    ("coalac_encode", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _U64, ctypes.c_uint, _P]),
    ("coalac_encode_segptr", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _U64, ctypes.c_uint, _P]),
    # decode: plan, idx, vals, mn, scale, ustart, base, out, stream (+ events)
    ("coalac_decode", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # error feedback: plan, in, seg pointers, base, resid, stream / plan, idx, vals, mn, scale, ustart, resid, stream
    ("coalac_ef_accumulate", _I, [_P, _P, _P, _P, _P, _P]),
    ("coalac_ef_commit", _I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    # compact payload: plan, bytes / plan, idx, vals, packed, packed_bytes, stream / plan, packed, packed_bytes, ustart,
    # idx, vals, stream
    ("coalac_plan_packed_bytes", _I, [_P, ctypes.POINTER(_U64)]),
    ("coalac_pack", _I, [_P, _P, _P, _P, _U64, _P]),
    ("coalac_unpack", _I, [_P, _P, _U64, _P, _P, _P, _P]),
    # bit-packed dense codes: plan, bytes / plan, vals, packed, packed_bytes, stream / plan, packed, packed_bytes, vals,
    # stream / plan, packed, packed_bytes, mn, scale, base, out, stream
    ("coalac_plan_dense_packed_bytes", _I, [_P, ctypes.POINTER(_U64)]),
    ("coalac_pack_dense", _I, [_P, _P, _P, _U64, _P]),
    ("coalac_unpack_dense", _I, [_P, _P, _U64, _P, _P]),
    ("coalac_decode_packed", _I, [_P, _P, _U64, _P, _P, _P, _P, _P]),
    # block-wise dense: plan, in, seg pointers, base, bmn, bscale, packed, packed_bytes, stream / plan, packed,
    # packed_bytes, bmn, bscale, base, out, stream
    ("coalac_encode_block", _I, [_P, _P, _P, _P, _P, _P, _P, _U64, _P]),
    ("coalac_decode_block", _I, [_P, _P, _U64, _P, _P, _P, _P, _P]),
    # stochastic rounding: plan, in, seg pointers, base, vals, mn, scale, ws, ws_bytes, seed, flags, stream / plan, in,
    # seg pointers, base, bmn, bscale, packed, packed_bytes, seed, stream
    ("coalac_encode_sr", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _U64, _U64, ctypes.c_uint, _P]),
    ("coalac_encode_block_sr", _I, [_P, _P, _P, _P, _P, _P, _P, _U64, _U64, _P]),
    # block-wise with error feedback in one pass: plan, in, seg pointers, base, resid, bmn, bscale, packed, packed_bytes,
    # stream
    ("coalac_encode_block_ef", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _U64, _P]),
    # block sizes 256 / 1024 / 4096: plan, block, count / the block-wise twins' arguments with `block` behind the plan
    # (the aggregate: behind clients, in the place of kind)
    ("coalac_plan_block_count", _I, [_P, ctypes.c_uint32, ctypes.POINTER(_U64)]),
    ("coalac_encode_block_g", _I, [_P, ctypes.c_uint32, _P, _P, _P, _P, _P, _P, _U64, _P]),
    ("coalac_decode_block_g", _I, [_P, ctypes.c_uint32, _P, _U64, _P, _P, _P, _P, _P]),
    ("coalac_aggregate_dense_g", _I, [_P, _I, ctypes.c_uint32, _P, _U64, _P, _P, _P, ctypes.c_float, _I, _P, _P, _P, _P]),
    # rotated block-wise: coalac_encode_block's arguments with rot_seed (and the SR seed) ahead of the
    # stream / coalac_decode_block's with rot_seed behind bscale
    ("coalac_encode_block_rot", _I, [_P, _P, _P, _P, _P, _P, _P, _U64, _U64, _P]),
    ("coalac_encode_block_rot_sr", _I, [_P, _P, _P, _P, _P, _P, _P, _U64, _U64, _U64, _P]),
    ("coalac_decode_block_rot", _I, [_P, _P, _U64, _P, _P, _U64, _P, _P, _P]),
    ("coalac_encode_ev", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _U64, ctypes.c_uint, _P, _P]),
    ("coalac_decode_ev", _I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    # aggregate: plan, clients, idx, vals, mn, scale, ustart, weights, total, mode, mask, base, out, stream (+ events)
    ("coalac_aggregate", _I, [_P, _I, _P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P, _P, _P, _P]),
    ("coalac_aggregate_ev", _I, [_P, _I, _P, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P, _P, _P, _P, _P]),
    # dense aggregate: plan, clients, kind, codes[], code_bytes, mn[], scale[], weights, total, mode, mask, base, out, stream
    ("coalac_aggregate_dense", _I, [_P, _I, _I, _P, _U64, _P, _P, _P, ctypes.c_float, _I, _P, _P, _P, _P]),
    # sparse aggregate from the uploads: plan, clients, kind, idx[], packed[], packed_bytes, vals[], mn[], scale[], ustart[],
    # weights, total, mode, mask, base, out, stream
    ("coalac_aggregate_uploads", _I, [_P, _I, _I, _P, _P, _U64, _P, _P, _P, _P, _P, ctypes.c_float, _I, _P, _P, _P, _P]),
    ("coalac_gather", _I, [_P, _I, _I, _P, _P]),
    ("coalac_workspace_fallbacks", _I, [_P, _P, _P, ctypes.POINTER(_I)]),
    ("coalac_debug_stamps", _I, [_P, _P, _P, ctypes.POINTER(ctypes.c_uint64), _I]),
    ("coalac_debug_brackets", _I, [_P, _P, _P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), _I]),
]

ABI_VERSION = 11
# added without a version step (purely additive): a library of the same ABI version built before them (a COALAC_LIB
# variant of an earlier commit) loads without them, and only a call that needs one fails
ADDED_FOR_BLOCK_SIZES = ("coalac_plan_block_count", "coalac_encode_block_g", "coalac_decode_block_g",
                         "coalac_aggregate_dense_g")
ADDED_FOR_ROTATION = ("coalac_encode_block_rot", "coalac_encode_block_rot_sr", "coalac_decode_block_rot")
ADDED_IN_ABI_11 = (("coalac_encode_sr", "coalac_encode_block_sr", "coalac_encode_block_ef") + ADDED_FOR_BLOCK_SIZES
                   + ADDED_FOR_ROTATION)


class CodecError(RuntimeError):
    pass


class SegDesc(ctypes.Structure):
    _fields_ = [("in_off", _U64), ("n", _U64), ("k", _U64), ("out_off", _U64)]


_lock = threading.Lock()
_lib = None


def lib_path():
    """The in-tree library; COALAC_LIB names another build of the same source (A/B variants under tools/)."""
    return os.environ.get("COALAC_LIB") or _build.LIB


def load(build_if_missing=True):
    """Load libcoalac.so (building it first if it is missing and hipcc is available)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = lib_path()
        if not os.environ.get("COALAC_LIB") and (
                not os.path.exists(path) or (build_if_missing and _build.stale() and _can_build())):
            if not build_if_missing:
                raise CodecError(f"HIP codec library not found at {path}; run __graft_entry__.build()")
            _build.build()
        lib = ctypes.CDLL(path)
        # the version first: a library of another ABI (a COALAC_LIB variant, a stale .so where hipcc is absent) may
        # lack symbols this binding names, and must fail with the version message, not an AttributeError
        lib.coalac_version.restype, lib.coalac_version.argtypes = _I, []
        v = lib.coalac_version()
        if v != ABI_VERSION:
            raise CodecError(f"libcoalac ABI version {v} != expected {ABI_VERSION} ({path}: rebuild it from this tree)")
        for name, res, args in SIGNATURES:
            if name in ADDED_IN_ABI_11 and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def _can_build():
    try:
        _build.hipcc()
        return True
    except RuntimeError:
        return False


def check(rc, what):
    if rc != 0:
        msg = _lib.coalac_last_error().decode(errors="replace") if _lib is not None else ""
        raise CodecError(f"{what} failed: {ERRORS.get(rc, rc)}: {msg}")
