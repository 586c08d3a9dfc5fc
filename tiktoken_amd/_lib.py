"""ctypes binding of csrc/libtiktoken_amd.so (the C ABI declared in include/tiktoken_amd.h).

This is the only door from Python into the HIP encode path.  There is deliberately no
fallback: if the shared library is missing or no MI355X is visible, construction of a CoreBPE
fails loudly (RuntimeError) instead of silently encoding on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# ($TIKTOKEN_AMD_LIB: another build of the same library -- kernel experiments with other compile-time parameters, tools/build_variant.sh)
_SO = os.environ.get("TIKTOKEN_AMD_LIB") or os.path.join(_HERE, "csrc", "libtiktoken_amd.so")
_lock = threading.Lock()
_lib = None

TK_OK, TK_VALUE_ERROR, TK_KEY_ERROR, TK_RUNTIME_ERROR, TK_UNSUPPORTED, TK_DISALLOWED_SPECIAL = range(6)
TK_JSONL_ERROR = 6  # (the JSON Lines calls raise JsonlError themselves: _tiktoken.py)


class JsonlBad(ctypes.Structure):
    """tk_jsonl_bad: the line a JSON Lines call under TK_JSONL_RAISE refuses (include/tiktoken_amd.h)."""
    _fields_ = [("line", ctypes.c_uint64), ("pos", ctypes.c_uint64), ("status", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


JSONL_OK, JSONL_BLANK, JSONL_MISSING, JSONL_NOT_STRING, JSONL_BAD = range(5)  # TK_JSONL_OK ..: the status of a line
JSONL_MODES = {"raise": 0, "skip": 1, "empty": 2}                             # on_error -> TK_JSONL_RAISE, TK_JSONL_SKIP, TK_JSONL_EMPTY


class SpecialHit(ctypes.Structure):
    """tk_special_hit: the first disallowed special token a checked call met (include/tiktoken_amd.h)."""
    _fields_ = [("doc", ctypes.c_uint64), ("pos", ctypes.c_uint64), ("id", ctypes.c_uint32), ("len", ctypes.c_uint32)]


class FingerprintSpec(ctypes.Structure):
    """tk_fingerprint_spec: shingle length, permutations, bands and seed of a fingerprint call (include/tiktoken_amd.h)."""
    _fields_ = [("ngram", ctypes.c_uint32), ("n_perm", ctypes.c_uint32), ("bands", ctypes.c_uint32), ("seed", ctypes.c_uint64)]


class RowsSpec(ctypes.Structure):
    """tk_rows_spec: how a packed batch is cut into training rows (include/tiktoken_amd.h)."""
    _fields_ = [("seq_len", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32), ("pad_id", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


ROWS_NO_TOKEN, ROWS_DROP_LAST, ROWS_IDS16 = 0xFFFFFFFF, 1, 2


class PadSpec(ctypes.Structure):
    """tk_pad_spec: how a packed batch becomes padded rows (include/tiktoken_amd.h)."""
    _fields_ = [("max_len", ctypes.c_uint32), ("stride", ctypes.c_uint32), ("width_multiple", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32),
                ("pad_id", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


PAD_WINDOWS, PAD_KEEP_TAIL, PAD_LEFT, PAD_IDS16 = 1, 2, 4, 8


class SplitSep(ctypes.Structure):
    """tk_split_sep: a separator, the bytes before a token boundary and the bytes from it on (include/tiktoken_amd.h)."""
    _fields_ = [("tail_len", ctypes.c_uint8), ("head_len", ctypes.c_uint8), ("tail", ctypes.c_uint8 * 16), ("head", ctypes.c_uint8 * 16)]


class SplitSpec(ctypes.Structure):
    """tk_split_spec: how the documents of a batch are cut into chunks (include/tiktoken_amd.h)."""
    _fields_ = [("max_tokens", ctypes.c_uint32), ("min_tokens", ctypes.c_uint32), ("overlap", ctypes.c_uint32), ("n_levels", ctypes.c_uint32),
                ("seg_tokens", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_seps", ctypes.c_uint32 * 4), ("sep", SplitSep * 4 * 4)]


SPLIT_HARD, SPLIT_FORCED, SPLIT_END = 0xFD, 0xFE, 0xFF


class SmpSpec(ctypes.Structure):
    """tk_smp_spec: how the parts of a packed batch become supervised samples (include/tiktoken_amd.h)."""
    _fields_ = [("max_len", ctypes.c_uint32), ("width_multiple", ctypes.c_uint32), ("bos_id", ctypes.c_uint32), ("eos_id", ctypes.c_uint32), ("pad_id", ctypes.c_uint32),
                ("ignore_index", ctypes.c_int32), ("flags", ctypes.c_uint32)]


SMP_KEEP_TAIL, SMP_LEFT, SMP_SKIP_LONG, SMP_IGNORE_FIRST = 1, 2, 4, 8


class DrowsSpec(ctypes.Structure):
    """tk_drows_spec: how the rows of an id matrix are trimmed before they are decoded (include/tiktoken_amd.h)."""
    _fields_ = [("flags", ctypes.c_uint32), ("n_stop", ctypes.c_uint32), ("n_skip", ctypes.c_uint32), ("stop_ids", ctypes.c_uint32 * 16), ("skip_ids", ctypes.c_uint32 * 16)]


DROWS_KEEP_STOP, DROWS_SKIP_SPECIAL, DROWS_I32, DROWS_I64 = 1, 2, 4, 8
U8_REPLACE, U8_IGNORE = 0, 1  # TK_U8_REPLACE, TK_U8_IGNORE
U8_BYTES = 2  # TK_U8_BYTES (the stop-string entries over id matrices: no repair)
STOPS_KEEP = 1  # TK_STOPS_KEEP


class Stops(ctypes.Structure):  # tk_stops
    _fields_ = [("n", ctypes.c_uint32), ("blob", ctypes.c_void_p), ("off", ctypes.c_void_p)]


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(_SO):
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "libtiktoken_amd.so"])
    return _SO


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_SO):
            raise ImportError(
                f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  tiktoken_amd has no CPU implementation to fall back to."
            )
        L = ctypes.CDLL(_SO)
        vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
        P = ctypes.POINTER
        L.tk_last_error.restype = ctypes.c_char_p
        L.tk_device_count.restype = i32
        L.tk_pattern_id.restype = i32
        L.tk_pattern_id.argtypes = [ctypes.c_char_p]
        L.tk_create.restype = i32
        L.tk_create.argtypes = [vp, vp, vp, u64, vp, vp, vp, u64, ctypes.c_char_p, i32, P(vp)]
        L.tk_destroy.argtypes = [vp]
        L.tk_encode_batch.restype = i32
        L.tk_encode_batch.argtypes = [vp, vp, vp, u64, i32, vp, u64, P(vp), P(u64), vp]
        L.tk_encode_batch_device.restype = i32
        L.tk_encode_batch_device.argtypes = [vp, vp, u64, vp, vp, u64, i32, vp, u64, vp, P(vp), P(u64), P(vp)]
        L.tk_pretokenize_batch.restype = i32
        L.tk_pretokenize_batch.argtypes = [vp, vp, vp, u64, i32, vp, u64, P(vp), P(u64)]
        L.tk_encode_ordinary.restype = i32
        L.tk_encode_ordinary.argtypes = [vp, vp, u64, P(vp), P(u64)]
        L.tk_encode.restype = i32
        L.tk_encode.argtypes = [vp, vp, u64, vp, u64, P(vp), P(u64)]
        L.tk_encode_single_piece.restype = i32
        L.tk_encode_single_piece.argtypes = [vp, vp, u64, P(vp), P(u64)]
        L.tk_byte_pair_encode.restype = i32
        L.tk_byte_pair_encode.argtypes = [vp, vp, u64, P(vp), P(u64)]
        L.tk_encode_single_token.restype = i32
        L.tk_encode_single_token.argtypes = [vp, vp, u64, P(u32)]
        L.tk_decode_bytes.restype = i32
        L.tk_decode_bytes.argtypes = [vp, vp, u64, P(vp), P(u64)]
        L.tk_decode_batch.restype = i32
        L.tk_decode_batch.argtypes = [vp, vp, vp, u64, P(vp), P(u64), vp]
        L.tk_decode_batch_device.restype = i32
        L.tk_decode_batch_device.argtypes = [vp, vp, u64, vp, u64, vp, P(vp), P(u64), P(vp)]
        L.tk_token_spans_device.restype = i32
        L.tk_token_spans_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, P(vp), P(vp), P(vp), P(vp)]
        L.tk_decode_batch_spans.restype = i32
        L.tk_decode_batch_spans.argtypes = [vp, vp, vp, u64, i32, P(vp), P(u64), P(vp), P(vp), vp, vp, P(u64)]
        L.tk_encode_batch_spans.restype = i32
        L.tk_encode_batch_spans.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(vp), P(u64), vp, P(vp), P(vp), P(SpecialHit)]
        L.tk_pack_rows_device.restype = i32
        L.tk_pack_rows_device.argtypes = [vp, vp, u64, vp, u64, P(RowsSpec), vp, P(vp), P(vp), P(vp), P(vp), P(vp), P(u64), P(u64), P(u64), P(u64)]
        L.tk_encode_batch_rows.restype = i32
        L.tk_encode_batch_rows.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(RowsSpec), P(vp), P(vp), P(vp), P(vp), P(vp), P(u64), P(u64), P(u64), P(u64),
                                           P(SpecialHit)]
        L.tk_pad_batch_device.restype = i32
        L.tk_pad_batch_device.argtypes = [vp, vp, u64, vp, u64, P(PadSpec), vp, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(u64), P(u64)]
        L.tk_encode_batch_padded.restype = i32
        L.tk_encode_batch_padded.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(PadSpec), P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(u64), P(u64), P(SpecialHit)]
        if hasattr(L, "tk_split_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_split_device.restype = i32
            L.tk_split_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, P(SplitSpec), vp, *[P(vp)] * 9, P(u64)]
            L.tk_encode_batch_split.restype = i32
            L.tk_encode_batch_split.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(SplitSpec), *[P(vp)] * 9, P(u64), P(vp), P(u64), vp, P(SpecialHit)]
        if hasattr(L, "tk_fingerprint_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_fingerprint_device.restype = i32
            L.tk_fingerprint_device.argtypes = [vp, vp, u64, vp, u64, P(FingerprintSpec), vp, vp, vp, vp, vp]
            L.tk_fingerprint.restype = i32
            L.tk_fingerprint.argtypes = [vp, vp, vp, u64, P(FingerprintSpec), vp, vp, vp, vp]
            L.tk_encode_batch_fingerprint.restype = i32
            L.tk_encode_batch_fingerprint.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(FingerprintSpec), vp, vp, vp, vp, vp, P(vp), P(u64), P(SpecialHit)]
        if hasattr(L, "tk_jsonl_extract_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_jsonl_extract_device.restype = i32
            L.tk_jsonl_extract_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, *[P(vp)] * 5, *[P(u64)] * 3, P(JsonlBad)]
            L.tk_jsonl_extract.restype = i32
            L.tk_jsonl_extract.argtypes = [vp, vp, u64, vp, u64, u32, *[P(vp)] * 5, *[P(u64)] * 3, P(JsonlBad)]
            L.tk_encode_jsonl.restype = i32
            L.tk_encode_jsonl.argtypes = [vp, vp, u64, vp, u64, u32, i32, vp, u64, vp, u64, P(vp), P(u64), P(vp), P(vp), P(vp), P(u64), P(u64), P(SpecialHit), P(JsonlBad)]
        L.tk_assemble_samples_device.restype = i32
        L.tk_assemble_samples_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, P(SmpSpec), vp, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(u64), P(u64)]
        L.tk_encode_batch_samples.restype = i32
        L.tk_encode_batch_samples.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, P(SmpSpec), P(vp), P(vp), P(vp), P(vp), P(vp), P(vp),
                                              P(u64), P(u64), P(SpecialHit)]
        if hasattr(L, "tk_pack_samples_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_pack_samples_device.restype = i32
            L.tk_pack_samples_device.argtypes = [vp, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, P(SmpSpec), vp, *[P(vp)] * 12, P(u64), P(u64)]
            L.tk_encode_batch_sample_rows.restype = i32
            L.tk_encode_batch_sample_rows.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, vp, vp, u64, u32, vp, vp, vp, P(SmpSpec), *[P(vp)] * 12, P(u64), P(u64),
                                                      P(SpecialHit)]
        if hasattr(L, "tk_decode_rows_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_decode_rows_device.restype = i32
            L.tk_decode_rows_device.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), vp, *[P(vp)] * 6, P(u64), P(u64)]
            L.tk_decode_rows.restype = i32
            L.tk_decode_rows.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), *[P(vp)] * 6, P(u64), P(u64)]
        if hasattr(L, "tk_utf8_repair_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_utf8_repair_device.restype = i32
            L.tk_utf8_repair_device.argtypes = [vp, vp, u64, vp, u64, u32, vp, P(vp), P(u64), P(vp), P(vp), P(vp), P(u64)]
            L.tk_decode_batch_text.restype = i32
            L.tk_decode_batch_text.argtypes = [vp, vp, vp, u64, u32, P(vp), P(u64), P(vp), P(vp), P(vp), P(u64)]
            L.tk_decode_rows_text_device.restype = i32
            L.tk_decode_rows_text_device.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), u32, vp, *[P(vp)] * 8, P(u64), P(u64), P(u64)]
            L.tk_decode_rows_text.restype = i32
            L.tk_decode_rows_text.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), u32, *[P(vp)] * 8, P(u64), P(u64), P(u64)]
        if hasattr(L, "tk_stop_text_device"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_stop_text_device.restype = i32
            L.tk_stop_text_device.argtypes = [vp, vp, u64, vp, u64, P(Stops), u32, vp, P(vp), P(u64), P(vp), P(vp), P(u64)]
            L.tk_decode_rows_until_device.restype = i32
            L.tk_decode_rows_until_device.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), P(Stops), u32, u32, vp, *[P(vp)] * 10, *[P(u64)] * 4]
            L.tk_decode_rows_until.restype = i32
            L.tk_decode_rows_until.argtypes = [vp, vp, u64, u64, u64, vp, vp, P(DrowsSpec), P(Stops), u32, u32, *[P(vp)] * 10, *[P(u64)] * 4]
        if hasattr(L, "tk_stream_create"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            outs = [P(vp), P(u64), P(vp), P(vp), P(vp), P(vp)]  # text, n_text, text_off, char_off, state, hit
            L.tk_stream_create.restype = i32
            L.tk_stream_create.argtypes = [vp, u64, u32, P(DrowsSpec), P(Stops), u32, u32, P(vp)]
            L.tk_stream_destroy.argtypes = [vp]
            L.tk_stream_dtype.restype = i32
            L.tk_stream_dtype.argtypes = [vp, u32]
            L.tk_stream_step_device.restype = i32
            L.tk_stream_step_device.argtypes = [vp, vp, u64, u64, vp, vp, vp, *outs]
            L.tk_stream_step.restype = i32
            L.tk_stream_step.argtypes = [vp, vp, u64, u64, vp, vp, *outs]
            L.tk_stream_fetch.restype = i32
            L.tk_stream_fetch.argtypes = [vp, *outs]
            L.tk_stream_flush.restype = i32
            L.tk_stream_flush.argtypes = [vp, vp, u64, *outs]
            L.tk_stream_reset.restype = i32
            L.tk_stream_reset.argtypes = [vp, vp, u64]
            L.tk_stream_rows.restype = i32
            L.tk_stream_rows.argtypes = [vp, vp, vp, vp, vp, vp]
        L.tk_decode_single_token_bytes.restype = i32
        L.tk_decode_single_token_bytes.argtypes = [vp, u32, P(vp), P(u64)]
        L.tk_n_tokens.restype = u64
        L.tk_n_tokens.argtypes = [vp]
        L.tk_sorted_token.restype = i32
        L.tk_sorted_token.argtypes = [vp, u64, P(vp), P(u64), P(u32)]
        L.tk_sorted_tokens_packed.restype = i32
        L.tk_sorted_tokens_packed.argtypes = [vp, P(vp), P(vp), P(u64)]
        L.tk_group_create.restype = i32
        L.tk_group_create.argtypes = [vp, u32, P(vp)]
        L.tk_group_destroy.argtypes = [vp]
        L.tk_group_size.restype = u32
        L.tk_group_size.argtypes = [vp]
        L.tk_group_encode_batch.restype = i32
        L.tk_group_encode_batch.argtypes = [vp, vp, vp, u64, i32, vp, u64, P(vp), P(u64), vp]
        L.tk_group_encode_batch_device.restype = i32
        L.tk_group_encode_batch_device.argtypes = [vp, vp, vp, u64, i32, vp, u64, P(vp), P(u64), P(vp)]
        L.tk_group_stat.restype = u64
        L.tk_group_stat.argtypes = [vp, ctypes.c_char_p]
        L.tk_parse_tiktoken_bpe.restype = i32
        L.tk_parse_tiktoken_bpe.argtypes = [vp, u64, P(vp), P(vp), P(vp), P(u64)]
        L.tk_validate_utf8.restype = i32
        L.tk_validate_utf8.argtypes = [vp, u64, P(u64)]
        L.tk_free.argtypes = [vp]
        L.tk_set_output_buffers.restype = i32
        L.tk_set_output_buffers.argtypes = [vp, ctypes.c_uint32]
        L.tk_set_profiling.argtypes = [vp, i32]
        L.tk_reset_kernel_ms.argtypes = [vp]
        L.tk_get_kernel_ms.restype = i32
        L.tk_get_kernel_ms.argtypes = [vp, ctypes.c_char_p, P(ctypes.c_double), P(u64)]
        L.tk_last_stats.argtypes = [vp, P(u64), P(u64), P(u64), P(u64), P(u64), P(u64)]
        if hasattr(L, "tk_encode_batch_checked"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB: a checked call then fails with AttributeError)
            L.tk_encode_batch_checked.restype = i32
            L.tk_encode_batch_checked.argtypes = [vp, vp, vp, u64, i32, vp, u64, vp, u64, P(vp), P(u64), vp, P(SpecialHit)]
            L.tk_encode_batch_device_checked.restype = i32
            L.tk_encode_batch_device_checked.argtypes = [vp, vp, u64, vp, vp, u64, i32, vp, u64, vp, P(vp), P(u64), P(vp), vp, u64, P(SpecialHit)]
            L.tk_group_encode_batch_checked.restype = i32
            L.tk_group_encode_batch_checked.argtypes = [vp, vp, vp, u64, i32, vp, u64, P(vp), P(u64), vp, vp, u64, P(SpecialHit)]
        if hasattr(L, "tk_train_bpe"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_train_bpe.restype = i32
            L.tk_train_bpe.argtypes = [vp, vp, vp, u64, u32, P(vp), P(vp), P(u64)]
        if hasattr(L, "tk_stat"):  # (absent from older builds selected through $TIKTOKEN_AMD_LIB)
            L.tk_stat.restype = u64
            L.tk_stat.argtypes = [vp, ctypes.c_char_p]
        _lib = L
    return _lib


def last_error() -> str:
    return lib().tk_last_error().decode("utf-8", "replace")


def device_count() -> int:
    try:
        return int(lib().tk_device_count())
    except ImportError:
        return 0


def raise_for(rc: int, key=None):
    """Map a C-ABI status to the exception type the reference raises (src/py.rs:21-22,46,142,160,171)."""
    if rc == TK_OK:
        return
    msg = last_error()
    if rc in (TK_VALUE_ERROR, TK_UNSUPPORTED, TK_DISALLOWED_SPECIAL, TK_JSONL_ERROR):  # (the checked calls raise DisallowedSpecialError themselves: _tiktoken.py)
        raise ValueError(msg)
    if rc == TK_KEY_ERROR:
        raise KeyError(key if key is not None else msg)
    raise RuntimeError(msg)
