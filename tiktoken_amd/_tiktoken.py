"""`CoreBPE` -- the drop-in for the reference's Rust extension class `tiktoken._tiktoken.CoreBPE`
(reference src/py.rs:13-184), implemented as a thin ctypes shim over the HIP library.

Same constructor and the same eleven methods, same exception types.  Two additive entry points,
`encode_batch_packed` and `pretokenize_packed`, expose the batch shape the GPU actually runs
(one launch sequence per batch instead of one FFI call per document); `decode_batch_spans_packed`, `token_spans_device` and
`encode_batch_spans_packed` give, for whole batches, where every token starts in its document (bytes and chars); `pack_rows_device` and
`encode_batch_rows_packed` cut a batch into fixed-length training rows with document ids, positions and cu_seqlens; `pad_batch_device` and
`encode_batch_padded_packed` give one padded row per document (or overlapping windows) with an attention mask; `split_device` and
`encode_batch_split_packed` cut every document into chunks of at most so many tokens, at separators and never inside a char; `assemble_samples_device` and
`encode_batch_samples_packed` join the parts of supervised samples with their roles' ids into rows with labels; `decode_rows_device` and
`decode_rows_packed` decode the rows of an id matrix, each cut at its first stop id and stripped of skipped and special ids; `train_bpe_packed`
trains a vocabulary: the merges of the reference's educational `bpe_train`, made on the device.  With `disallowed_special` the batch
calls also search the text for those special tokens, on the device, and raise `DisallowedSpecialError`.
"""
from __future__ import annotations

import atexit
import ctypes
import dataclasses
import weakref
from typing import AbstractSet, NamedTuple, Sequence

import numpy as np

from . import _lib

# Cores that are still alive when the interpreter shuts down are destroyed by an atexit handler -- i.e. BEFORE the HIP runtime's own static
# destructors run at process exit.  A tk_destroy from a late __del__ (module teardown, or later still) would free streams and page-locked
# buffers of a runtime that is already gone.
_live_cores: "weakref.WeakSet[CoreBPE]" = weakref.WeakSet()


@atexit.register
def _destroy_live_cores():
    for core in sorted(_live_cores, key=lambda c: getattr(c, "_group", None) is None):  # (a group before the replicas it refers to)
        try:
            core.close()
        except Exception:
            pass

# char::is_whitespace (Rust, lib.rs:583) = the Unicode White_Space property
_WHITE_SPACE = frozenset(map(chr, [9, 10, 11, 12, 13, 32, 0x85, 0xA0, 0x1680, *range(0x2000, 0x200B), 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))


def _pack_pairs(items: Sequence[tuple[bytes, int]]):
    blob = b"".join(k for k, _ in items)
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    if items:
        np.cumsum(np.fromiter((len(k) for k, _ in items), dtype=np.uint64, count=len(items)), out=off[1:])
    ids = np.fromiter((v for _, v in items), dtype=np.uint32, count=len(items))
    data = np.frombuffer(blob, dtype=np.uint8) if blob else np.zeros(1, dtype=np.uint8)
    return data, off, ids if len(items) else np.zeros(1, dtype=np.uint32)


class _OwnedBuffer:
    """A library-owned result buffer (page-locked host memory for large results) seen through the array interface: numpy views it in
    place, and it goes back to the library (tk_free) when the last view is gone.  The counterpart of the reference's TiktokenBuffer
    (src/py.rs:186-249)."""

    def __init__(self, ptr: int, n: int, typestr: str = "<u4"):
        self._ptr = ptr
        self.__array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, True), "version": 3}

    def __del__(self):
        ptr, self._ptr = getattr(self, "_ptr", None), None
        if ptr:
            try:
                _lib.lib().tk_free(ptr)
            except Exception:
                pass


def _take_u32(ptr: ctypes.c_void_p, n: int) -> np.ndarray:
    """numpy array of a library-owned uint32 result: large ones in place (no second copy), small ones copied and released."""
    if not n:
        _lib.lib().tk_free(ptr)
        return np.zeros(0, dtype=np.uint32)
    if n >= (1 << 16):
        return np.asarray(_OwnedBuffer(ptr.value, n))
    out = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctypes.c_uint32)), shape=(n,)).copy()
    _lib.lib().tk_free(ptr)
    return out


def _take(ptr: ctypes.c_void_p, n: int, dtype) -> np.ndarray:
    """... of a uint32 or uint16 result"""
    dtype = np.dtype(dtype)
    if dtype == np.uint32:
        return _take_u32(ptr, n)
    if n >= (1 << 16):
        return np.asarray(_OwnedBuffer(ptr.value, n, "<u2"))
    out = np.frombuffer(ctypes.string_at(ptr, n * 2), dtype=np.uint16).copy() if n else np.zeros(0, dtype=np.uint16)
    _lib.lib().tk_free(ptr)
    return out


def _take_u8(ptr: ctypes.c_void_p, n: int) -> np.ndarray:
    """... of a uint8 result (read-only use: decoded bytes)."""
    if n >= (1 << 16):
        return np.asarray(_OwnedBuffer(ptr.value, n, "|u1"))
    out = np.frombuffer(ctypes.string_at(ptr, n), dtype=np.uint8)
    _lib.lib().tk_free(ptr)
    return out


def _take_u64(ptr: ctypes.c_void_p, n: int) -> np.ndarray:
    """... of a uint64 result"""
    if n >= (1 << 16):
        return np.asarray(_OwnedBuffer(ptr.value, n, "<u8"))
    out = np.frombuffer(ctypes.string_at(ptr, n * 8), dtype=np.uint64).copy() if n else np.zeros(0, dtype=np.uint64)
    _lib.lib().tk_free(ptr)
    return out


def _check_packed(blob: np.ndarray, doc_off: np.ndarray) -> None:
    """The C ABI reads doc_off[n_docs] bytes of the blob: refuse offsets that do not describe it."""
    if doc_off.ndim != 1 or len(doc_off) < 1:
        raise ValueError("doc_off must hold n_docs + 1 offsets (at least one)")
    if int(doc_off[0]) != 0 or int(doc_off[-1]) != len(blob):
        raise ValueError("doc_off[0] must be 0 and doc_off[-1] must equal len(blob)")
    if len(doc_off) > 1 and bool(np.any(doc_off[1:] < doc_off[:-1])):
        raise ValueError("doc_off must be non-decreasing")


def invalid_utf8_at(data: bytes) -> int | None:
    """Offset of the first byte of `data` that is not part of a well-formed UTF-8 char, or None (tk_validate_utf8: for callers that hand the
    C ABI bytes they cannot vouch for -- a Python str is valid by construction, as the reference's &str is)."""
    buf = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(1, dtype=np.uint8)
    pos = ctypes.c_uint64()
    return None if _lib.lib().tk_validate_utf8(buf.ctypes.data, len(data), ctypes.byref(pos)) == 0 else int(pos.value)


def disallowed_special_message(token: str) -> str:
    """The reference's text for a disallowed special token (raise_disallowed_special_token, tiktoken/core.py:441-449)."""
    return (
        f"Encountered text corresponding to disallowed special token {token!r}.\n"
        "If you want this text to be encoded as a special token, "
        f"pass it to `allowed_special`, e.g. `allowed_special={{{token!r}, ...}}`.\n"
        f"If you want this text to be encoded as normal text, disable the check for this token "
        f"by passing `disallowed_special=(enc.special_tokens_set - {{{token!r}}})`.\n"
        "To disable this check for all special tokens, pass `disallowed_special=()`.\n"
    )


class PackedRows(NamedTuple):
    """A batch as training rows (tk_encode_batch_rows; the rule: include/tiktoken_amd.h).  The stream is [bos] document [eos] for every
    document in order, cut into rows of seq_len; `doc` is the document of a position (0xFFFFFFFF on padding), `pos` its position in its
    segment -- positions restart at every document and at every row --, `cu_seqlens` the positions where a segment starts plus the end,
    `row_seg[r]` the number of segments that start before row r: cu_seqlens[row_seg[a] : row_seg[b] + 1] - a * seq_len are the
    cu_seqlens of the rows a .. b alone.  With drop_last the positions that do not fill a row come as the tail_ arrays (to be carried
    into the caller's next batch) and cu_seqlens / row_seg cover them too; without it the last row is padded and the tails are empty."""
    ids: np.ndarray  # [R, seq_len], uint32 or uint16
    doc: np.ndarray  # [R, seq_len] uint32
    pos: np.ndarray  # [R, seq_len] uint32
    cu_seqlens: np.ndarray  # uint32[n_segs + 1]
    row_seg: np.ndarray  # uint32[R + 1]
    n_stream: int
    tail_ids: np.ndarray
    tail_doc: np.ndarray
    tail_pos: np.ndarray


class RowsDevice(NamedTuple):
    """`pack_rows_device`: device pointers (the core's buffers, valid until its next rows call) and the figures that size them:
    ids / doc / pos hold n_rows * seq_len + n_tail elements, cu_seqlens n_segs + 1, row_seg n_rows + 1."""
    ids: int
    doc: int
    pos: int
    cu_seqlens: int
    row_seg: int
    n_rows: int
    n_segs: int
    n_stream: int
    n_tail: int


class PaddedBatch(NamedTuple):
    """A batch as padded model inputs (tk_encode_batch_padded; the rule: include/tiktoken_amd.h): one row per document, truncated to
    max_length -- or, with windows, as many rows as a long document needs, consecutive ones sharing `stride` tokens.  Row r belongs to
    document row_doc[r], starts at its body token row_tok[r] and holds lengths[r] elements ([bos] body [eos]) where attention_mask is 1;
    everywhere else input_ids is the pad id.  The rows of document d are doc_row[d] .. doc_row[d + 1]."""
    input_ids: np.ndarray  # [R, W], uint32 or uint16
    attention_mask: np.ndarray  # [R, W] uint8
    lengths: np.ndarray  # uint32[R]
    row_doc: np.ndarray  # uint32[R]
    row_tok: np.ndarray  # uint32[R]
    doc_row: np.ndarray  # uint32[n_docs + 1]


class PaddedDevice(NamedTuple):
    """`pad_batch_device`: device pointers (the core's buffers, valid until its next padded call) and the figures that size them:
    input_ids / attention_mask hold n_rows * width elements, lengths / row_doc / row_tok n_rows, doc_row n_docs + 1."""
    input_ids: int
    attention_mask: int
    lengths: int
    row_doc: int
    row_tok: int
    doc_row: int
    n_rows: int
    width: int


class TextChunks:
    """A batch cut into chunks (tk_encode_batch_split; the rule: include/tiktoken_amd.h): per chunk, in document order, `doc`, `tok_begin` /
    `tok_end` (token indices inside the document), `byte_begin` / `byte_end` and `char_begin` / `char_end` (the same places in the
    document's text) and `cut` (the separator level the chunk ends at, or SPLIT_HARD, SPLIT_FORCED, SPLIT_END); `doc_chunk[d]` is the
    first chunk of document d, `doc_chunk[-1]` the number of chunks; `tokens` and `tok_off` are the batch's ids.  `text(i)` and `ids(i)`
    give chunk i's text and ids."""
    SPLIT_HARD, SPLIT_FORCED, SPLIT_END = _lib.SPLIT_HARD, _lib.SPLIT_FORCED, _lib.SPLIT_END
    FIELDS = ("doc", "tok_begin", "tok_end", "byte_begin", "byte_end", "char_begin", "char_end", "cut", "doc_chunk")

    def __init__(self, arrays, tokens: np.ndarray, tok_off: np.ndarray, blob: np.ndarray, doc_off: np.ndarray):
        for name, a in zip(self.FIELDS, arrays):
            setattr(self, name, a)
        self.tokens, self.tok_off = tokens, tok_off
        self._blob, self._doc_off = blob, doc_off

    def __len__(self) -> int:
        return len(self.doc)

    def text_bytes(self, i: int) -> bytes:
        a = int(self._doc_off[int(self.doc[i])])
        return self._blob[a + int(self.byte_begin[i]):a + int(self.byte_end[i])].tobytes()

    def text(self, i: int, errors: str = "replace") -> str:
        return self.text_bytes(i).decode("utf-8", errors)

    def ids(self, i: int) -> np.ndarray:
        a = int(self.tok_off[int(self.doc[i])])
        return self.tokens[a + int(self.tok_begin[i]):a + int(self.tok_end[i])]


class SplitDevice(NamedTuple):
    """`split_device`: device pointers (the core's buffers, valid until its next split call that succeeds) to the arrays of `TextChunks`
    -- uint32[n_chunks] each, `cut` uint8[n_chunks], `doc_chunk` uint32[n_docs + 1] -- and the number of chunks."""
    doc: int
    tok_begin: int
    tok_end: int
    byte_begin: int
    byte_end: int
    char_begin: int
    char_end: int
    cut: int
    doc_chunk: int
    n_chunks: int


DEFAULT_SEPARATORS = ((("\n\n", ""),), (("\n", ""),), ((".", " "), ("?", " "), ("!", " ")), (("", " "),))


class Role(NamedTuple):
    """A role of a sample's parts (tk_assemble_samples_device): the token ids put before and after the body of every part of that role -- a
    chat template's header and footer, given as ids, never as text --, and whether the part is trained: its body and its `after` ids get
    labels, its `before` ids never do."""
    before: Sequence[int] = ()
    after: Sequence[int] = ()
    train: bool = False


class SampleBatch(NamedTuple):
    """A batch as supervised samples (tk_encode_batch_samples; the rule: include/tiktoken_amd.h): one row per sample -- [bos], for every
    part the before ids of its role, its tokens, the after ids, [eos] -- cut to max_length at the head or the tail.  attention_mask is 1
    on the row's elements, input_ids the pad id elsewhere; labels holds the id where the element is trained and ignore_index everywhere
    else (not shifted: the model shifts).  length[s] elements are in the row, full_length[s] the sample had before the cut, n_trained[s]
    of the trained ones survived it."""
    input_ids: np.ndarray  # [R, W] uint32
    attention_mask: np.ndarray  # [R, W] uint8
    labels: np.ndarray  # [R, W] int32
    length: np.ndarray  # uint32[R]
    full_length: np.ndarray  # uint64[R]
    n_trained: np.ndarray  # uint32[R]


class SamplesDevice(NamedTuple):
    """`assemble_samples_device`: device pointers (the core's buffers, valid until its next samples call that succeeds) and the figures that
    size them: input_ids / attention_mask / labels hold n_rows * width elements, length / full_length / n_trained n_rows."""
    input_ids: int
    attention_mask: int
    labels: int
    length: int
    full_length: int
    n_trained: int
    n_rows: int
    width: int


class SampleRows(NamedTuple):
    """A batch as packed sample rows (tk_encode_batch_sample_rows; the rule: include/tiktoken_amd.h): the samples of `SampleBatch`, several
    whole ones to a row of max_length, placed next-fit in input order.  Per position: input_ids (the pad id on a row's tail), labels (not
    shifted; ignore_index where nothing is trained), segment_ids (the sample; 2^32 - 1 on padding) and position_ids (restarting at every
    sample, and at a row's padding tail).  cu_seqlens holds the flat positions where a segment starts and, last, R * max_length --
    cu_seqlens[row_seg[a] : row_seg[b] + 1] - a * max_length are the boundaries of the rows a .. b alone.  Per sample: length, full_length,
    n_trained (0 for a sample that is not placed), sample_row (2^32 - 1: not placed) and sample_col; row_sample[r] is row r's first sample."""
    input_ids: np.ndarray  # [R, L] uint32
    labels: np.ndarray  # [R, L] int32
    segment_ids: np.ndarray  # [R, L] uint32
    position_ids: np.ndarray  # [R, L] uint32
    cu_seqlens: np.ndarray  # uint32[n_segs + 1]
    row_seg: np.ndarray  # uint32[R + 1]
    row_sample: np.ndarray  # uint32[R + 1]
    length: np.ndarray  # uint32[n_samples]
    full_length: np.ndarray  # uint64[n_samples]
    n_trained: np.ndarray  # uint32[n_samples]
    sample_row: np.ndarray  # uint32[n_samples]
    sample_col: np.ndarray  # uint32[n_samples]


class SampleRowsDevice(NamedTuple):
    """`pack_samples_device`: device pointers (the core's buffers, valid until its next packed-samples call that succeeds) and the figures
    that size them: input_ids / labels / segment_ids / position_ids hold n_rows * max_length elements, cu_seqlens n_segs + 1, row_seg and
    row_sample n_rows + 1, the others n_samples."""
    input_ids: int
    labels: int
    segment_ids: int
    position_ids: int
    cu_seqlens: int
    row_seg: int
    row_sample: int
    length: int
    full_length: int
    n_trained: int
    sample_row: int
    sample_col: int
    n_rows: int
    n_segs: int


class DecodedRows(NamedTuple):
    """The rows of an id matrix, trimmed and decoded (tk_decode_rows; the rule: include/tiktoken_amd.h).  Row r is live from begin[r] to its
    first stop id, stop_col[r] (end[r] when it has none, so stop_col[r] < end[r] says that the row finished); of the live ids those in
    `skip` (and, with skip_special, the special tokens) are dropped, the n_kept[r] others are tokens[tok_off[r] : tok_off[r + 1]] and decode
    to data[byte_off[r] : byte_off[r + 1]]."""
    data: np.ndarray  # uint8: the rows' bytes back to back
    byte_off: np.ndarray  # uint64[R + 1]
    tokens: np.ndarray  # uint32[K]
    tok_off: np.ndarray  # uint64[R + 1]
    n_kept: np.ndarray  # uint32[R]
    stop_col: np.ndarray  # uint32[R]


class DecodedRowsDevice(NamedTuple):
    """`decode_rows_device`: device pointers and the figures that size them: tokens holds n_tokens ids, data n_bytes bytes, tok_off and
    byte_off n_rows + 1 entries, n_kept and stop_col n_rows.  tokens .. stop_col are the core's buffers, valid until its next decode-rows
    call that succeeds; data and byte_off are its decode buffers, valid until its next decode call."""
    tokens: int
    tok_off: int
    n_kept: int
    stop_col: int
    data: int
    byte_off: int
    n_tokens: int
    n_bytes: int


class RepairedText(NamedTuple):
    """Packed, well-formed UTF-8 (tk_decode_batch_text; the rule: include/tiktoken_amd.h, tk_utf8_repair_device): document d is
    data[text_off[d] : text_off[d + 1]], has char_off[d + 1] - char_off[d] chars, and repl_off[d + 1] - repl_off[d] of its units were
    ill-formed (replaced by U+FFFD, or dropped with errors="ignore")."""
    data: np.ndarray  # uint8
    text_off: np.ndarray  # uint64[n + 1]
    char_off: np.ndarray  # uint64[n + 1]
    repl_off: np.ndarray  # uint64[n + 1]


class RepairedDevice(NamedTuple):
    """`utf8_repair_device`: device pointers and the figures that size them: data holds n_bytes bytes, the three offset arrays n_docs + 1
    entries.  The core's buffers, valid until its next repair call -- but with n_replaced == 0 data and text_off are the caller's own input
    pointers: nothing was written."""
    data: int
    text_off: int
    char_off: int
    repl_off: int
    n_bytes: int
    n_replaced: int


@dataclasses.dataclass(frozen=True)
class DecodedRowsText:
    """`DecodedRows` with text for bytes (tk_decode_rows_text): data is well-formed UTF-8, row r is data[byte_off[r] : byte_off[r + 1]];
    char_off and repl_off as in `RepairedText`.  tokens, tok_off, n_kept and stop_col are those of `decode_rows_packed`."""
    data: np.ndarray  # uint8: the rows' text back to back
    byte_off: np.ndarray  # uint64[R + 1]
    tokens: np.ndarray  # uint32[K]
    tok_off: np.ndarray  # uint64[R + 1]
    n_kept: np.ndarray  # uint32[R]
    stop_col: np.ndarray  # uint32[R]
    char_off: np.ndarray  # uint64[R + 1]
    repl_off: np.ndarray  # uint64[R + 1]

    @property
    def text_off(self) -> np.ndarray:
        return self.byte_off


class DecodedRowsTextDevice(NamedTuple):
    """`decode_rows_text_device`: `DecodedRowsDevice` with the repaired text in data / byte_off (n_bytes bytes), char_off, repl_off and
    n_replaced.  tokens .. stop_col are valid until the core's next decode-rows call that succeeds, the others until its next repair call
    (with n_replaced == 0 data and byte_off are the decode buffers: until its next decode call)."""
    tokens: int
    tok_off: int
    n_kept: int
    stop_col: int
    data: int
    byte_off: int
    char_off: int
    repl_off: int
    n_tokens: int
    n_bytes: int
    n_replaced: int


class StoppedTextDevice(NamedTuple):
    """`stop_text_device`: device pointers and the figures that size them: data holds n_bytes bytes, text_off n_docs + 1 entries, hit
    n_docs.  The core's buffers, valid until its next stop-string call -- but with n_hit == 0 data and text_off are the caller's own input
    pointers: nothing was written."""
    data: int
    text_off: int
    hit: int
    n_bytes: int
    n_hit: int


@dataclasses.dataclass(frozen=True)
class StoppedRows:
    """`DecodedRowsText` of rows that were cut at their first stop string as well (tk_decode_rows_until; the rule:
    include/tiktoken_amd.h, tk_stop_text_device): row r is data[byte_off[r] : byte_off[r + 1]]; hit[r] is the index of the stop string
    that ended it (NO_HIT: none did); n_tok[r] counts the row's kept tokens whose first byte lies before the end of the kept text.
    char_off and repl_off are None in the bytes mode, which repairs nothing."""
    data: np.ndarray  # uint8
    byte_off: np.ndarray  # uint64[R + 1]
    char_off: "np.ndarray | None"  # uint64[R + 1]
    repl_off: "np.ndarray | None"  # uint64[R + 1]
    tokens: np.ndarray  # uint32[K]
    tok_off: np.ndarray  # uint64[R + 1]
    n_kept: np.ndarray  # uint32[R]
    stop_col: np.ndarray  # uint32[R]
    hit: np.ndarray  # uint32[R]
    n_tok: np.ndarray  # uint32[R]

    NO_HIT = 0xFFFFFFFF


class StoppedRowsDevice(NamedTuple):
    """`decode_rows_until_device`: `DecodedRowsTextDevice` with hit and n_tok (valid until the core's next stop-string call) and n_hit;
    char_off and repl_off are 0 in the bytes mode."""
    tokens: int
    tok_off: int
    n_kept: int
    stop_col: int
    data: int
    byte_off: int
    char_off: int
    repl_off: int
    hit: int
    n_tok: int
    n_tokens: int
    n_bytes: int
    n_replaced: int
    n_hit: int


class StreamPacked(NamedTuple):
    """What a call of a decode stream emitted, as arrays (copies: the stream's own buffers last until its next call): row r emitted
    text[text_off[r] : text_off[r + 1]], char_off counts its chars (None in the bytes mode); state and hit: the rows' state (0 live, 1 ended
    by a stop id, 2 by a stop string, 3 flushed) and the stop string that ended them (NO_HIT: none) after the call."""
    text: np.ndarray  # uint8
    text_off: np.ndarray  # uint64[R + 1]
    char_off: "np.ndarray | None"  # uint64[R + 1]
    state: np.ndarray  # uint32[R]
    hit: np.ndarray  # uint32[R]

    NO_HIT = 0xFFFFFFFF


class StreamStep(NamedTuple):
    """`DecodeStream.step` / `flush`: text[r] is what row r emitted (str; bytes under errors=None), finished[r] says that the row has ended."""
    text: list
    finished: np.ndarray  # bool[R]
    state: np.ndarray  # uint32[R]
    hit: np.ndarray  # uint32[R]


class NativeStream:
    """A tk_stream and the calls on it; made by `CoreBPE.stream_create`.  Keeps its core alive: the stream must go first."""

    def __init__(self, core: "CoreBPE", handle, n_rows: int, w_max: int, mode: int):
        self._core, self._h, self.n_rows, self.w_max, self.mode = core, handle, n_rows, w_max, mode
        self._dtype = _lib.DROWS_I64

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self._core, "_h", None):  # (a core that is closed has taken its device's buffers along)
            try:
                self._core._L.tk_stream_destroy(h)
            except Exception:
                pass

    __del__ = close

    def _handle(self):
        if not self._h:
            raise ValueError("the decode stream is closed")
        return self._h

    def _set_dtype(self, dtype) -> None:
        try:
            flag = CoreBPE._ROW_DTYPES[np.dtype(dtype)]
        except (KeyError, TypeError):
            raise ValueError("an id matrix holds uint32, int32 or int64") from None
        if flag != self._dtype:
            _lib.raise_for(self._core._L.tk_stream_dtype(self._handle(), flag))
            self._dtype = flag

    @staticmethod
    def _outs():
        out = [ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()]
        return out, [ctypes.byref(x) for x in out]

    def _packed(self, out) -> StreamPacked:
        def arr(ptr, n, dtype):
            if not n or not ptr.value:
                return np.zeros(0 if not n else n, dtype)
            return np.frombuffer(ctypes.string_at(ptr.value, n * np.dtype(dtype).itemsize), dtype)

        R = self.n_rows
        return StreamPacked(arr(out[0], int(out[1].value), np.uint8), arr(out[2], R + 1, np.uint64), arr(out[3], R + 1, np.uint64) if self.mode != _lib.U8_BYTES else None,
                            arr(out[4], R, np.uint32), arr(out[5], R, np.uint32))

    def step_host(self, ids: np.ndarray, width: int, ld: int, begin, end) -> StreamPacked:
        self._set_dtype(ids.dtype)
        out, refs = self._outs()
        rc = self._core._L.tk_stream_step(self._handle(), ids.ctypes.data if self.n_rows and width else None, width, ld, None if begin is None else begin.ctypes.data,
                                          None if end is None else end.ctypes.data, *refs)
        _lib.raise_for(rc)
        return self._packed(out)

    def step_device(self, d_ids: int, width: int, ld: int, dtype, d_begin: int = 0, d_end: int = 0, stream: int = 0) -> StreamPacked:
        self._set_dtype(dtype)
        out, refs = self._outs()
        _lib.raise_for(self._core._L.tk_stream_step_device(self._handle(), d_ids or None, width, ld, d_begin or None, d_end or None, stream or None, *refs))
        out, refs = self._outs()
        _lib.raise_for(self._core._L.tk_stream_fetch(self._handle(), *refs))
        return self._packed(out)

    def _rows_arg(self, rows):
        if rows is None:
            return None, 0
        a = np.ascontiguousarray([int(r) for r in rows], dtype=np.int64)
        if len(a) and (int(a.min()) < 0 or int(a.max()) >= self.n_rows):
            raise ValueError(f"rows must name slots 0 .. {self.n_rows - 1} of the stream")
        a = np.concatenate([a, [0]]).astype(np.uint32)  # (never an empty buffer)
        return a, len(a) - 1

    def flush(self, rows=None) -> StreamPacked:
        a, n = self._rows_arg(rows)
        out, refs = self._outs()
        _lib.raise_for(self._core._L.tk_stream_flush(self._handle(), None if a is None else a.ctypes.data, n, *refs))
        return self._packed(out)

    def reset(self, rows=None) -> None:
        a, n = self._rows_arg(rows)
        _lib.raise_for(self._core._L.tk_stream_reset(self._handle(), None if a is None else a.ctypes.data, n))

    def rows(self) -> "dict[str, np.ndarray]":
        """state, hit (uint32[R]) and the totals n_kept, n_text, n_chars (uint64[R]) of the slots"""
        R = self.n_rows
        a = dict(state=np.zeros(R + 1, np.uint32), hit=np.zeros(R + 1, np.uint32), n_kept=np.zeros(R + 1, np.uint64), n_text=np.zeros(R + 1, np.uint64),
                 n_chars=np.zeros(R + 1, np.uint64))
        _lib.raise_for(self._core._L.tk_stream_rows(self._handle(), *[v.ctypes.data for v in a.values()]))
        return {k: v[:R] for k, v in a.items()}


def until_mode(errors: "str | None") -> int:
    """errors= of the stop-string entries -> TK_U8_REPLACE / TK_U8_IGNORE, None -> TK_U8_BYTES"""
    return _lib.U8_BYTES if errors is None else repair_mode(errors)


class _StopSet:
    """stop strings (str: its UTF-8; bytes) as a tk_stops, with the arrays it points into"""

    def __init__(self, stop_text):
        if isinstance(stop_text, (str, bytes, bytearray)):
            stop_text = (stop_text,)
        strings = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in stop_text]
        self.strings = strings
        self.blob = np.frombuffer(b"".join(strings) + b"\0", dtype=np.uint8)
        self.off = np.zeros(len(strings) + 1, dtype=np.uint32)
        total = sum(map(len, strings))
        if total >= 1 << 32:
            raise ValueError("stop strings of 4 GiB or more")
        if strings:
            self.off[1:] = np.cumsum([len(s) for s in strings])
        self.c = _lib.Stops(len(strings), self.blob.ctypes.data, self.off.ctypes.data)


def repair_mode(errors: str) -> int:
    """errors= of the text entries -> TK_U8_REPLACE / TK_U8_IGNORE"""
    if errors == "replace":
        return _lib.U8_REPLACE
    if errors == "ignore":
        return _lib.U8_IGNORE
    raise ValueError(f"errors={errors!r}: the packed text entries repair on the device with errors='replace' or 'ignore'; for 'strict' and other "
                     "handlers use decode, decode_batch or decode_rows (or decode_with_offsets_packed, which validates)")


class JsonlError(ValueError):
    """A JSON Lines call with on_error="raise" met a line that is neither a record nor blank: its index `line`, the byte offset `pos` it
    starts at in the buffer and its `status` (JSONL_MISSING, JSONL_NOT_STRING or JSONL_BAD)."""

    def __init__(self, line: int, pos: int, status: int, message: str):
        super().__init__(message)
        self.line, self.pos, self.status = line, pos, status


class JsonlText(NamedTuple):
    """One field of every line of a JSON Lines buffer (tk_jsonl_extract; the rule: include/tiktoken_amd.h): `text` uint8, the unescaped
    values back to back, `doc_off` uint64[n_docs + 1] their boundaries -- what the packed encode entries take --, `line` uint64[n_docs]
    the line every document came from, `status` uint8[n_lines] the status of every line, `line_off` uint64[n_lines + 1] where it starts."""
    text: np.ndarray
    doc_off: np.ndarray
    line: np.ndarray
    status: np.ndarray
    n_lines: int
    line_off: np.ndarray

    def text_bytes(self, i: int) -> bytes:
        return self.text[int(self.doc_off[i]):int(self.doc_off[i + 1])].tobytes()

    def texts(self) -> "list[str]":
        off, blob = self.doc_off.tolist(), self.text.tobytes()
        return [blob[a:b].decode("utf-8") for a, b in zip(off[:-1], off[1:])]


class JsonlTokens(NamedTuple):
    """A JSON Lines buffer encoded (tk_encode_jsonl): `tokens` and `tok_off` as `encode_batch_packed` gives them, `line` and `status` as in
    `JsonlText`."""
    tokens: np.ndarray
    tok_off: np.ndarray
    line: np.ndarray
    status: np.ndarray
    n_lines: int


class JsonlDevice(NamedTuple):
    """`jsonl_extract_device`: device pointers (the core's buffers, valid until its next JSON Lines call that succeeds) to the arrays of
    `JsonlText`, and the counts."""
    text: int
    doc_off: int
    line: int
    line_off: int
    status: int
    n_docs: int
    n_lines: int
    n_text: int


class Fingerprints(NamedTuple):
    """Near-duplicate fingerprints of a batch (tk_fingerprint; the rule: include/tiktoken_amd.h): `sig` uint32[n, P] the MinHash signatures
    over token shingles, `band` uint64[n, B] the LSH keys of their bands, `exact` uint64[n] a hash of the whole document, `n_shingles`
    uint64[n], `length` uint64[n] the documents' token counts.  The helpers run on the host, in numpy, and are deterministic."""
    sig: np.ndarray
    band: np.ndarray
    exact: np.ndarray
    n_shingles: np.ndarray
    length: np.ndarray

    def jaccard(self, i: int, j: int) -> float:
        """The share of signature positions documents i and j agree in: an estimate of their shingle sets' Jaccard index."""
        return float(np.count_nonzero(self.sig[i] == self.sig[j])) / self.sig.shape[1]

    def exact_groups(self) -> np.ndarray:
        """int64[n]: for every document the lowest index of a document with the same (exact, length)."""
        if not len(self.exact):
            return np.zeros(0, dtype=np.int64)
        _, first, inv = np.unique(np.stack([self.exact, self.length], axis=1), axis=0, return_index=True, return_inverse=True)
        return first[inv.reshape(-1)].astype(np.int64)

    def duplicate_groups(self, threshold: float = 0.8) -> np.ndarray:
        """int64[n]: the lowest index of every document's group.  Per band, the documents with shingles that share a key are each compared
        with the lowest of them and joined to it (union-find) when `jaccard` >= threshold: n * B comparisons at the most."""
        n, P = self.sig.shape
        parent = list(range(n))

        def find(x: int) -> int:
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        live = np.flatnonzero(self.n_shingles > 0)
        for j in range(self.band.shape[1] if len(live) else 0):
            _, first, inv = np.unique(self.band[live, j], return_index=True, return_inverse=True)
            rep = live[first[inv.reshape(-1)]]  # (live ascends: the first occurrence of a key is its lowest index)
            other = rep != live
            a, b = live[other], rep[other]
            close = np.count_nonzero(self.sig[a] == self.sig[b], axis=1) / P >= threshold
            for x, y in zip(a[close].tolist(), b[close].tolist()):
                rx, ry = find(x), find(y)
                if rx != ry:
                    parent[max(rx, ry)] = min(rx, ry)  # (the root of a group is its lowest index)
        return np.fromiter((find(x) for x in range(n)), dtype=np.int64, count=n)

    def keep_mask(self, threshold: float = 0.8) -> np.ndarray:
        """bool[n]: true for the representative (the lowest index) of every group of `duplicate_groups`."""
        return self.duplicate_groups(threshold) == np.arange(len(self.exact))


class DisallowedSpecialError(ValueError):
    """A batch holds a disallowed special token: the first occurrence -- document `doc`, byte offset `pos` inside it, the `token` (the
    longest disallowed one that matches there).  What the reference raises as a plain ValueError, with its message."""

    def __init__(self, doc: int, pos: int, token: str):
        super().__init__(disallowed_special_message(token))
        self.doc, self.pos, self.token = doc, pos, token


def default_devices() -> list[int]:
    """Devices a CoreBPE uses when none are named: $TIKTOKEN_AMD_DEVICES (comma-separated ordinals, or "all"), else device 0."""
    import os

    v = os.environ.get("TIKTOKEN_AMD_DEVICES", "").strip()
    if not v:
        return [0]
    if v == "all":
        return list(range(max(_lib.device_count(), 1)))
    return [int(x) for x in v.split(",") if x.strip()]


class CoreBPE:
    def __init__(self, encoder: dict[bytes, int], special_tokens_encoder: dict[str, int], pattern: str, *,
                 device: int | None = None, devices: Sequence[int] | None = None):
        """`devices`: several GPUs of this node (one replica of the tables per device; batches are split by documents into
        contiguous ranges of about equal byte counts -- tk_group_encode_batch).  A device may be named twice (virtual ranks)."""
        L = _lib.lib()
        if devices is None:
            devices = [device] if device is not None else default_devices()
        devices = list(devices)
        if not devices:
            raise ValueError("devices must name at least one GPU")
        device = devices[0]
        self._replicas: list[CoreBPE] = []
        self._group = None
        self._specials = dict(special_tokens_encoder)
        sb, so, si = _pack_pairs([(k.encode("utf-8"), v) for k, v in self._specials.items()])
        # vocab_io.RankTable: the arrays straight from the native parser (its dict may not even be filled yet: nothing here walks it)
        packed = getattr(encoder, "packed", None)
        fresh = packed is not None and getattr(encoder, "_pending", None) is not None
        h = ctypes.c_void_p()
        for attempt in (0, 1):
            if packed is not None and (fresh or len(packed[2]) == len(encoder)):
                rb, ro, ri = packed
            else:
                for v in encoder.values():
                    if not 0 <= v <= 0xFFFFFFFF:
                        raise OverflowError("rank does not fit in u32")  # PyO3 would refuse the conversion too
                rb, ro, ri = _pack_pairs(list(encoder.items()))
            rc = L.tk_create(rb.ctypes.data, ro.ctypes.data, ri.ctypes.data, len(ro) - 1, sb.ctypes.data, so.ctypes.data,
                             si.ctypes.data, len(self._specials), pattern.encode("utf-8"), device, ctypes.byref(h))
            if rc != _lib.TK_OK and fresh and attempt == 0 and "duplicate key" in _lib.last_error():
                # a file that lists a token twice: the dict keeps the later rank (as the reference's does) -- build from the dict
                encoder.materialize()
                packed, fresh = encoder.packed, False
                continue
            break
        _lib.raise_for(rc)
        if fresh:
            encoder._distinct = True  # (tk_create refuses a token listed twice)
        self._h = h
        self._L = L
        _live_cores.add(self)
        self.device = device
        self.devices = devices
        if len(devices) > 1:
            self._replicas = [CoreBPE(encoder, special_tokens_encoder, pattern, devices=[d]) for d in devices[1:]]
            handles = (ctypes.c_void_p * len(devices))(h, *[r._h for r in self._replicas])
            grp = ctypes.c_void_p()
            _lib.raise_for(L.tk_group_create(handles, len(devices), ctypes.byref(grp)))
            self._group = grp

    def __del__(self):
        self.close()

    def close(self):
        """Releases the native core (tables, workspace, streams).  Idempotent; the object is unusable afterwards."""
        g, self._group = getattr(self, "_group", None), None
        if g:
            try:
                self._L.tk_group_destroy(g)
            except Exception:
                pass
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._L.tk_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ helpers
    def _allowed_ids(self, allowed_special: AbstractSet[str]) -> tuple[np.ndarray, int]:
        if isinstance(allowed_special, str):
            if allowed_special != "all":
                raise ValueError("allowed_special must be a set of special-token strings or 'all'")
            allowed_special = self._specials.keys()
        ids = [self._specials[s] for s in allowed_special if s in self._specials]
        return np.asarray(ids if ids else [0], dtype=np.uint32), len(ids)

    def _disallowed_ids(self, disallowed_special) -> tuple[np.ndarray, int]:
        """ids of the special tokens a checked call searches for (None or empty: none, the unchecked call)"""
        if disallowed_special is None:
            return np.zeros(1, dtype=np.uint32), 0
        if isinstance(disallowed_special, str):
            if disallowed_special != "all":
                raise ValueError("disallowed_special must be a collection of special-token strings or 'all'")
            disallowed_special = self._specials.keys()
        unknown = [s for s in disallowed_special if s not in self._specials]
        if unknown:  # (the device searches for registered special tokens only; Encoding keeps its host search for any other string)
            raise ValueError(f"not a special token of this encoding: {unknown[0]!r}")
        ids = sorted({self._specials[s] for s in disallowed_special})
        return np.asarray(ids if ids else [0], dtype=np.uint32), len(ids)

    def _raise_hit(self, hit: "_lib.SpecialHit"):
        # (two special strings may share an id: the length tells them apart)
        token = next((s for s, i in self._specials.items() if i == hit.id and len(s.encode("utf-8")) == hit.len), None)
        if token is None:
            raise RuntimeError(f"internal error: the library reported special token id {hit.id} of {hit.len} bytes, which is not registered")
        raise DisallowedSpecialError(int(hit.doc), int(hit.pos), token)

    def _batch_args(self, blob, doc_off, allowed_special, disallowed_special):
        """A packed batch and its special-token arguments as the tk_encode_batch* entries take them: (the arguments from utf8 to n_allowed,
        disallowed_ids and n_disallowed, n_docs, the arrays behind the pointers -- to be kept until the call is over)."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        _check_packed(blob, doc_off)
        n_docs = len(doc_off) - 1
        src = blob if len(blob) else np.zeros(1, dtype=np.uint8)
        ids, k = (np.zeros(1, dtype=np.uint32), 0) if allowed_special is None else self._allowed_ids(allowed_special)
        dis, n_dis = self._disallowed_ids(disallowed_special)
        return ((src.ctypes.data, doc_off.ctypes.data, n_docs, 0 if allowed_special is None else 1, ids.ctypes.data, k), (dis.ctypes.data, n_dis), n_docs,
                (src, doc_off, ids, dis))

    def _raise_for(self, rc: int, hit: "_lib.SpecialHit") -> None:
        if rc == _lib.TK_DISALLOWED_SPECIAL:
            self._raise_hit(hit)
        _lib.raise_for(rc)

    @staticmethod
    def _as_u8(data: bytes) -> np.ndarray:
        return np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)

    def _encode_np(self, data: bytes, allowed_special: AbstractSet[str] | None) -> np.ndarray:
        buf = self._as_u8(data)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        if allowed_special is None:
            rc = self._L.tk_encode_ordinary(self._h, buf.ctypes.data, len(data), ctypes.byref(out), ctypes.byref(n))
        else:
            ids, k = self._allowed_ids(allowed_special)
            rc = self._L.tk_encode(self._h, buf.ctypes.data, len(data), ids.ctypes.data, k, ctypes.byref(out), ctypes.byref(n))
        _lib.raise_for(rc)
        return _take_u32(out, n.value)

    # ------------------------------------------------------------------ encoding (src/py.rs:29-131)
    def encode_ordinary(self, text: str) -> list[int]:
        # str.encode raises UnicodeEncodeError on lone surrogates, as PyO3's &str extraction does;
        # Encoding.encode_ordinary relies on that to trigger its repair path (core.py:77-80)
        return self._encode_np(text.encode("utf-8"), None).tolist()

    def encode(self, text: str, allowed_special: AbstractSet[str]) -> list[int]:
        return self._encode_np(text.encode("utf-8"), allowed_special).tolist()

    def encode_to_tiktoken_buffer(self, text: str, allowed_special: AbstractSet[str]):
        """Object with the buffer protocol: read-only, 1-D, itemsize 4, format 'I' (src/py.rs:186-249)."""
        arr = self._encode_np(text.encode("utf-8"), allowed_special)
        arr.setflags(write=False)
        return arr

    def encode_batch_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *,
                            disallowed_special=None):
        """One GPU batch: `blob` = documents packed back to back (uint8), `doc_off` = uint64[n+1].
        Returns (tokens uint32[T], tok_off uint64[n+1]).
        `disallowed_special`: special-token strings (or "all") the text must not spell -- searched for on the device in the same call
        (tk_encode_batch_checked); DisallowedSpecialError names the first occurrence.  None or empty: no search."""
        text, dis, n_docs, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        tok_off = np.empty(n_docs + 1, dtype=np.uint64)
        out, n, hit = ctypes.c_void_p(), ctypes.c_uint64(), _lib.SpecialHit()
        res = (ctypes.byref(out), ctypes.byref(n), tok_off.ctypes.data)
        grouped = self._group is not None and n_docs > 1
        if dis[1] and grouped:
            rc = self._L.tk_group_encode_batch_checked(self._group, *text, *res, *dis, ctypes.byref(hit))
        elif dis[1]:
            rc = self._L.tk_encode_batch_checked(self._h, *text, *dis, *res, ctypes.byref(hit))
        elif grouped:
            rc = self._L.tk_group_encode_batch(self._group, *text, *res)
        else:
            rc = self._L.tk_encode_batch(self._h, *text, *res)
        self._raise_for(rc, hit)
        return _take_u32(out, n.value), tok_off

    def encode_batch_gathered(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None):
        """Multi-GPU batch with the token ids gathered on the FIRST device (peer copies over xGMI): returns
        (d_tokens_ptr, n_tokens, d_tok_off_ptr), device pointers owned by this CoreBPE and valid until its next call."""
        if self._group is None:
            raise ValueError("encode_batch_gathered needs a CoreBPE built with several devices")
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        _check_packed(blob, doc_off)
        if allowed_special is None:
            ids, k, mode = np.zeros(1, dtype=np.uint32), 0, 0
        else:
            ids, k = self._allowed_ids(allowed_special)
            mode = 1
        src = blob if len(blob) else np.zeros(1, dtype=np.uint8)
        dt, dn, do = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
        rc = self._L.tk_group_encode_batch_device(self._group, src.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, mode, ids.ctypes.data, k,
                                                  ctypes.byref(dt), ctypes.byref(dn), ctypes.byref(do))
        _lib.raise_for(rc)
        return dt.value, dn.value, do.value

    def group_stat(self, name: str) -> int:
        return int(self._L.tk_group_stat(self._group, name.encode())) if self._group is not None else 0

    def encode_batch_device(self, d_text_ptr: int, n_bytes: int, d_doc_off_ptr: int, h_doc_off: np.ndarray | None,
                            n_docs: int, allowed_special: AbstractSet[str] | None = None, stream: int = 0, *, disallowed_special=None):
        """Device-resident batch (tk_encode_batch_device): inputs already in HBM, results stay in HBM.
        Returns (d_tokens_ptr, n_tokens, d_tok_off_ptr); the pointers are owned by this CoreBPE and valid
        until its next encode call.  d_text must be readable 64 bytes past n_bytes.
        `disallowed_special`: as in encode_batch_packed (tk_encode_batch_device_checked)."""
        dt, dn, do = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
        if allowed_special is None:
            ids, k, mode = np.zeros(1, dtype=np.uint32), 0, 0
        else:
            ids, k = self._allowed_ids(allowed_special)
            mode = 1
        h_ptr = None
        if h_doc_off is not None:
            h_doc_off = np.ascontiguousarray(h_doc_off, dtype=np.uint64)
            h_ptr = h_doc_off.ctypes.data
        dis, n_dis = self._disallowed_ids(disallowed_special)
        if n_dis:
            hit = _lib.SpecialHit()
            rc = self._L.tk_encode_batch_device_checked(self._h, d_text_ptr, n_bytes, d_doc_off_ptr, h_ptr, n_docs, mode, ids.ctypes.data, k, stream or None,
                                                        ctypes.byref(dt), ctypes.byref(dn), ctypes.byref(do), dis.ctypes.data, n_dis, ctypes.byref(hit))
            if rc == _lib.TK_DISALLOWED_SPECIAL:
                self._raise_hit(hit)
        else:
            rc = self._L.tk_encode_batch_device(self._h, d_text_ptr, n_bytes, d_doc_off_ptr, h_ptr, n_docs, mode, ids.ctypes.data, k,
                                                stream or None, ctypes.byref(dt), ctypes.byref(dn), ctypes.byref(do))
        _lib.raise_for(rc)
        return dt.value, dn.value, do.value

    def pretokenize_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None) -> np.ndarray:
        """Piece start offsets (uint32, ascending, plus a final sentinel = total bytes) of a packed batch --
        what `regex.find_iter` yields at src/lib.rs:365/405, computed by the GPU pre-tokeniser.  Chars the pattern does not match
        (generic engine only) are steps of their own; their offsets are also left in `self.last_gaps`."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        _check_packed(blob, doc_off)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        src = blob if len(blob) else np.zeros(1, dtype=np.uint8)
        if allowed_special is None:
            ids, k, mode = np.zeros(1, dtype=np.uint32), 0, 0
        else:
            ids, k = self._allowed_ids(allowed_special)
            mode = 1
        rc = self._L.tk_pretokenize_batch(self._h, src.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, mode,
                                          ids.ctypes.data, k, ctypes.byref(out), ctypes.byref(n))
        _lib.raise_for(rc)
        starts = _take_u32(out, n.value)
        # bit 31: a char at which a pat_str of the generic engine matches nothing (find_iter skips it: no token) -- kept in self.last_gaps
        self.last_gaps = (starts[starts >= 0x80000000] & 0x7FFFFFFF).astype(np.uint32)
        return starts & np.uint32(0x7FFFFFFF) if len(self.last_gaps) else starts

    def encode_single_token(self, piece: bytes) -> int:
        tok = ctypes.c_uint32()
        rc = self._L.tk_encode_single_token(self._h, self._as_u8(piece).ctypes.data, len(piece), ctypes.byref(tok))
        _lib.raise_for(rc, key=piece)
        return tok.value

    def encode_single_piece(self, piece: bytes) -> list[int]:
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._L.tk_encode_single_piece(self._h, self._as_u8(piece).ctypes.data, len(piece), ctypes.byref(out), ctypes.byref(n))
        _lib.raise_for(rc)
        return _take_u32(out, n.value).tolist()

    def _byte_pair_encode(self, piece: bytes) -> list[int]:
        """byte_pair_encode (src/lib.rs:198-211): the merge loop without the whole-piece shortcut."""
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._L.tk_byte_pair_encode(self._h, self._as_u8(piece).ctypes.data, len(piece), ctypes.byref(out), ctypes.byref(n))
        _lib.raise_for(rc)
        return _take_u32(out, n.value).tolist()

    # -- byte-level / unstable entry points: host logic over the primitives above
    def _last_piece_token_len(self, data: bytes, allowed_special: AbstractSet[str] | None = None) -> int:
        """Tokens contributed by the last regex piece (second value of CoreBPE::encode, src/lib.rs:439-441);
        0 when the text ends with an allowed special token (lib.rs:433)."""
        if not data:
            return 0
        starts = self.pretokenize_packed(np.frombuffer(data, dtype=np.uint8), np.array([0, len(data)], dtype=np.uint64),
                                         allowed_special)
        tail = data[int(starts[-2]):]
        if allowed_special and any(tail == s.encode("utf-8") for s in allowed_special if s in self._specials):
            return 0
        return len(self.encode_single_piece(tail))

    def _token_is_all_space(self, token: int) -> bool:
        try:
            b = self.decode_single_token_bytes(token)
        except KeyError:
            return False
        return all(c in b" \n\t" for c in b)

    def _increase_last_piece_token_len(self, tokens: list[int], last: int) -> int:
        # src/lib.rs:444-481
        if last > 0 and self._token_is_all_space(tokens[len(tokens) - last]):
            while last < len(tokens) and self._token_is_all_space(tokens[len(tokens) - last - 1]):
                last += 1
        return last

    def _encode_bytes(self, data: bytes) -> list[int]:
        """src/py.rs:72-115: bytes that may end in (or contain) invalid UTF-8."""
        try:
            data.decode("utf-8")
            return self._encode_np(data, None).tolist()
        except UnicodeDecodeError as e:
            valid = e.start
        head = data[:valid]
        tokens = self._encode_np(head, None).tolist()
        last = self._increase_last_piece_token_len(tokens, self._last_piece_token_len(head)) if tokens else 0
        if tokens and last > 0:
            unstable = self.decode_bytes(tokens[len(tokens) - last:]) + data[valid:]
            del tokens[len(tokens) - last:]
        else:
            unstable = data[valid:]
        if unstable:
            tokens.extend(self.encode_single_piece(unstable))
        return tokens

    def encode_with_unstable(self, text: str, allowed_special: AbstractSet[str]):
        """src/lib.rs:483-599 (`_encode_unstable_native`), restated on the host over the GPU primitives."""
        data = text.encode("utf-8")
        tokens = self._encode_np(data, allowed_special).tolist()
        last = self._last_piece_token_len(data, allowed_special)
        if last == 0:
            return tokens, []
        last = self._increase_last_piece_token_len(tokens, last)
        unstable = self.decode_bytes(tokens[len(tokens) - last:])
        del tokens[len(tokens) - last:]
        completions: set[tuple[int, ...]] = set()
        if not unstable:
            return tokens, []
        import bisect

        sorted_tokens = self._sorted_tokens()
        point = bisect.bisect_left(sorted_tokens, unstable)
        while point < len(sorted_tokens) and sorted_tokens[point].startswith(unstable):
            completions.add((self.encode_single_token(sorted_tokens[point]),))
            point += 1
        for i in range(1, len(unstable)):
            prefix, suffix = unstable[:i], unstable[i:]
            point = bisect.bisect_left(sorted_tokens, suffix)
            while point < len(sorted_tokens) and sorted_tokens[point].startswith(suffix):
                possibility = prefix + sorted_tokens[point]
                try:
                    possibility.decode("utf-8")
                    encoded = self._encode_np(possibility, None).tolist()
                except UnicodeDecodeError:
                    encoded = self._byte_pair_encode(possibility)  # lib.rs:555
                seq, seq_len = [], 0
                for t in encoded:
                    seq.append(t)
                    seq_len += len(self.decode_single_token_bytes(t))
                    if seq_len >= len(unstable):
                        break
                completions.add(tuple(seq))
                point += 1
        if len(unstable) > 1:
            # last code point of the unstable bytes: bstr::decode_last_utf8 (lib.rs:581-596); char::is_whitespace is the
            # Unicode White_Space property (not str.isspace(), which also accepts U+001C..U+001F)
            ch, k = None, 1
            for start in range(max(0, len(unstable) - 4), len(unstable)):
                try:
                    cand = unstable[start:].decode("utf-8")
                except UnicodeDecodeError:
                    continue
                if len(cand) == 1:
                    ch, k = cand, len(unstable) - start
                    break
            if ch is not None and len(unstable) - k > 0 and ch in _WHITE_SPACE:
                re = self._byte_pair_encode(unstable[:len(unstable) - k]) + self._byte_pair_encode(unstable[len(unstable) - k:])
                completions.add(tuple(re))
        return tokens, [list(c) for c in completions]

    # ------------------------------------------------------------------ decoding (src/py.rs:156-183)
    def decode_bytes(self, tokens: Sequence[int]) -> bytes:
        arr = np.asarray(tokens, dtype=np.uint32) if len(tokens) else np.zeros(1, dtype=np.uint32)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._L.tk_decode_bytes(self._h, arr.ctypes.data, len(tokens), ctypes.byref(out), ctypes.byref(n))
        _lib.raise_for(rc)
        data = ctypes.string_at(out, n.value)
        self._L.tk_free(out)
        return data

    def decode_batch_packed(self, tokens: np.ndarray, tok_off: np.ndarray, as_array: bool = False):
        """One GPU call for a packed batch: (all bytes back to back, byte_off uint64[n_docs + 1])  -- tk_decode_batch.
        as_array: the bytes as a read-only uint8 array over the library's (page-locked) result buffer instead of a `bytes` copy."""
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
        if tok_off.ndim != 1 or len(tok_off) < 1 or int(tok_off[-1]) != len(tokens):
            raise ValueError("tok_off must hold n_docs + 1 offsets ending at len(tokens)")
        byte_off = np.empty(len(tok_off), dtype=np.uint64)
        out, n = ctypes.c_void_p(), ctypes.c_uint64()
        src = tokens if len(tokens) else np.zeros(1, dtype=np.uint32)
        rc = self._L.tk_decode_batch(self._h, src.ctypes.data, tok_off.ctypes.data, len(tok_off) - 1, ctypes.byref(out), ctypes.byref(n),
                                     byte_off.ctypes.data)
        _lib.raise_for(rc)
        if as_array and n.value >= (1 << 16):
            return np.asarray(_OwnedBuffer(out.value, n.value, "|u1")), byte_off
        data = ctypes.string_at(out, n.value)
        self._L.tk_free(out)
        return (np.frombuffer(data, dtype=np.uint8) if as_array else data), byte_off

    def decode_batch_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_docs: int, stream: int = 0):
        """Device-resident decode (tk_decode_batch_device): pointers to uint32 ids and uint64 token offsets (0: none) on this core's device ->
        (device pointer to the bytes, number of bytes, device pointer to the n_docs + 1 byte offsets or 0).  The buffers are the library's and
        stay valid until the next decode call."""
        db, nb, do = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p()
        rc = self._L.tk_decode_batch_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_docs, stream or None, ctypes.byref(db),
                                            ctypes.byref(nb), ctypes.byref(do))
        _lib.raise_for(rc)
        return db.value or 0, nb.value, do.value or 0

    # ------------------------------------------------------------------ id matrices (no reference counterpart: the host loop of its users)
    _ROW_DTYPES = {np.dtype(np.uint32): 0, np.dtype(np.int32): _lib.DROWS_I32, np.dtype(np.int64): _lib.DROWS_I64}

    @classmethod
    def _drows_spec(cls, dtype, stop, skip, skip_special: bool, keep_stop: bool) -> "_lib.DrowsSpec":
        try:
            flags = cls._ROW_DTYPES[np.dtype(dtype)]
        except (KeyError, TypeError):
            raise ValueError("an id matrix holds uint32, int32 or int64") from None
        stop, skip = [int(t) for t in stop], [int(t) for t in skip]
        for name, ids in (("stop", stop), ("skip", skip)):
            if len(ids) > 16:
                raise ValueError(f"more than 16 {name} ids")
            if any(not 0 <= t <= 0xFFFFFFFF for t in ids):
                raise ValueError(f"{name} ids must be token ids below 2^32")
        flags |= (_lib.DROWS_SKIP_SPECIAL if skip_special else 0) | (_lib.DROWS_KEEP_STOP if keep_stop else 0)
        U16 = ctypes.c_uint32 * 16
        return _lib.DrowsSpec(flags, len(stop), len(skip), U16(*stop), U16(*skip))

    def decode_rows_device(self, d_ids: int, n_rows: int, width: int, ld: int | None = None, *, dtype=np.int64, d_begin: int = 0, d_end: int = 0, stop: Sequence[int] = (),
                           skip: Sequence[int] = (), skip_special: bool = False, keep_stop: bool = False, stream: int = 0) -> DecodedRowsDevice:
        """Device-resident decode of an id matrix (tk_decode_rows_device): a pointer to element (0, 0) of n_rows x width ids of `dtype`
        (uint32, int32, int64) on this core's device, rows `ld` elements apart (None: width) -- a column slice of a wider matrix goes in as
        it lies --, d_begin / d_end: pointers to uint32[n_rows] (0: every row is live from column 0 / to column width); see `DecodedRows`
        for the rule and the arrays."""
        self._one_device("decode_rows_device")
        spec = self._drows_spec(dtype, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(6, 2)
        rc = self._L.tk_decode_rows_device(self._h, d_ids or None, n_rows, width, width if ld is None else ld, d_begin or None, d_end or None, ctypes.byref(spec),
                                           stream or None, *refs)
        _lib.raise_for(rc)
        return DecodedRowsDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    @staticmethod
    def _row_bounds(x, n_rows: int, name: str):
        if x is None:
            return None
        a = np.asarray(x)
        if a.shape != (n_rows,) or (len(a) and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF)):
            raise ValueError(f"{name} must hold one column index below 2^32 per row")
        return np.ascontiguousarray(a, dtype=np.uint32)

    def _host_matrix(self, ids, begin, end, stop, skip, skip_special: bool, keep_stop: bool):
        """(ids, n_rows, width, ld, begin, end, spec) of an id matrix in host memory, checked"""
        ids = np.asarray(ids)
        if ids.ndim != 2:
            raise ValueError("an id matrix has two dimensions")
        spec = self._drows_spec(ids.dtype, stop, skip, skip_special, keep_stop)
        n_rows, width = ids.shape
        item = ids.itemsize
        if n_rows and width > 1 and ids.strides[1] != item:  # (the strides of an array without elements say nothing)
            raise ValueError("the column stride of an id matrix must be one element")
        ld = width
        if n_rows > 1 and width:
            if ids.strides[0] % item or ids.strides[0] < width * item:
                raise ValueError("the row stride of an id matrix must be a whole number of elements, at least a row")
            ld = ids.strides[0] // item
        return ids, n_rows, width, ld, self._row_bounds(begin, n_rows, "begin"), self._row_bounds(end, n_rows, "end"), spec

    def decode_rows_packed(self, ids: np.ndarray, *, begin=None, end=None, stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False,
                           keep_stop: bool = False) -> DecodedRows:
        """One GPU call for an id matrix in host memory (tk_decode_rows): a 2-D array of uint32, int32 or int64 whose column stride is one
        element -- any row stride of at least a row: a column slice of a wider matrix is not copied first."""
        self._one_device("decode_rows_packed")
        ids, n_rows, width, ld, begin, end, spec = self._host_matrix(ids, begin, end, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(6, 2)
        rc = self._L.tk_decode_rows(self._h, ids.ctypes.data if n_rows and width else None, n_rows, width, ld, None if begin is None else begin.ctypes.data,
                                    None if end is None else end.ctypes.data, ctypes.byref(spec), *refs)
        _lib.raise_for(rc)
        n_tokens, n_bytes = (int(x.value) for x in cnt)
        return DecodedRows(_take_u8(out[4], n_bytes), _take_u64(out[5], n_rows + 1), _take_u32(out[0], n_tokens), _take_u64(out[1], n_rows + 1),
                           _take_u32(out[2], n_rows), _take_u32(out[3], n_rows))

    # ------------------------------------------------------------------ text instead of bytes: errors="replace" / "ignore" on the device
    def utf8_repair_device(self, d_bytes: int, n_bytes: int, d_byte_off: int, n_docs: int, errors: str = "replace", stream: int = 0) -> RepairedDevice:
        """UTF-8 repair of packed text that is on this core's device (tk_utf8_repair_device): d_bytes 16-byte aligned and readable for 16
        bytes past n_bytes (the decode buffers are), d_byte_off uint64[n_docs + 1] ascending from 0 to n_bytes."""
        self._one_device("utf8_repair_device")
        out, cnt = [ctypes.c_void_p() for _ in range(4)], [ctypes.c_uint64(), ctypes.c_uint64()]
        rc = self._L.tk_utf8_repair_device(self._h, d_bytes or None, n_bytes, d_byte_off or None, n_docs, repair_mode(errors), stream or None, ctypes.byref(out[0]),
                                           ctypes.byref(cnt[0]), ctypes.byref(out[1]), ctypes.byref(out[2]), ctypes.byref(out[3]), ctypes.byref(cnt[1]))
        _lib.raise_for(rc)
        return RepairedDevice(*[x.value or 0 for x in out], int(cnt[0].value), int(cnt[1].value))

    def decode_batch_text_packed(self, tokens: np.ndarray, tok_off: np.ndarray, errors: str = "replace") -> "tuple[RepairedText, int]":
        """One GPU call for a packed batch (tk_decode_batch_text): (`RepairedText`, units replaced)."""
        self._one_device("decode_batch_text_packed")
        mode = repair_mode(errors)
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
        if tok_off.ndim != 1 or len(tok_off) < 1 or int(tok_off[-1]) != len(tokens):
            raise ValueError("tok_off must hold n_docs + 1 offsets ending at len(tokens)")
        n_docs = len(tok_off) - 1
        out, cnt = [ctypes.c_void_p() for _ in range(4)], [ctypes.c_uint64(), ctypes.c_uint64()]
        src = tokens if len(tokens) else np.zeros(1, dtype=np.uint32)
        rc = self._L.tk_decode_batch_text(self._h, src.ctypes.data, tok_off.ctypes.data, n_docs, mode, ctypes.byref(out[0]), ctypes.byref(cnt[0]), ctypes.byref(out[1]),
                                          ctypes.byref(out[2]), ctypes.byref(out[3]), ctypes.byref(cnt[1]))
        _lib.raise_for(rc)
        return RepairedText(_take_u8(out[0], int(cnt[0].value)), *[_take_u64(p, n_docs + 1) for p in out[1:]]), int(cnt[1].value)

    def decode_rows_text_device(self, d_ids: int, n_rows: int, width: int, ld: int | None = None, *, dtype=np.int64, d_begin: int = 0, d_end: int = 0,
                                stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False, keep_stop: bool = False, errors: str = "replace",
                                stream: int = 0) -> DecodedRowsTextDevice:
        """`decode_rows_device` with text for bytes (tk_decode_rows_text_device)."""
        self._one_device("decode_rows_text_device")
        mode = repair_mode(errors)
        spec = self._drows_spec(dtype, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(8, 3)
        rc = self._L.tk_decode_rows_text_device(self._h, d_ids or None, n_rows, width, width if ld is None else ld, d_begin or None, d_end or None, ctypes.byref(spec), mode,
                                                stream or None, *refs)
        _lib.raise_for(rc)
        return DecodedRowsTextDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def decode_rows_text_packed(self, ids: np.ndarray, *, begin=None, end=None, stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False,
                                keep_stop: bool = False, errors: str = "replace") -> DecodedRowsText:
        """`decode_rows_packed` with text for bytes (tk_decode_rows_text); the matrix as there."""
        self._one_device("decode_rows_text_packed")
        mode = repair_mode(errors)
        ids, n_rows, width, ld, begin, end, spec = self._host_matrix(ids, begin, end, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(8, 3)
        rc = self._L.tk_decode_rows_text(self._h, ids.ctypes.data if n_rows and width else None, n_rows, width, ld, None if begin is None else begin.ctypes.data,
                                         None if end is None else end.ctypes.data, ctypes.byref(spec), mode, *refs)
        _lib.raise_for(rc)
        n_tokens, n_bytes, _ = (int(x.value) for x in cnt)
        return DecodedRowsText(_take_u8(out[4], n_bytes), _take_u64(out[5], n_rows + 1), _take_u32(out[0], n_tokens), _take_u64(out[1], n_rows + 1),
                               _take_u32(out[2], n_rows), _take_u32(out[3], n_rows), _take_u64(out[6], n_rows + 1), _take_u64(out[7], n_rows + 1))

    # ------------------------------------------------------------------ stop strings: rows and documents cut at the first stop text
    def stop_text_device(self, d_bytes: int, n_bytes: int, d_byte_off: int, n_docs: int, stop_text, keep_stop_text: bool = False, stream: int = 0) -> StoppedTextDevice:
        """Packed text on this core's device cut at every document's first stop string (tk_stop_text_device): the buffers as
        `utf8_repair_device` takes them; stop_text: up to 16 str (their UTF-8) or bytes of 1 .. 64 bytes each."""
        self._one_device("stop_text_device")
        stops = _StopSet(stop_text)
        out, cnt = [ctypes.c_void_p() for _ in range(3)], [ctypes.c_uint64(), ctypes.c_uint64()]
        rc = self._L.tk_stop_text_device(self._h, d_bytes or None, n_bytes, d_byte_off or None, n_docs, ctypes.byref(stops.c), _lib.STOPS_KEEP if keep_stop_text else 0,
                                         stream or None, ctypes.byref(out[0]), ctypes.byref(cnt[0]), ctypes.byref(out[1]), ctypes.byref(out[2]), ctypes.byref(cnt[1]))
        _lib.raise_for(rc)
        return StoppedTextDevice(*[x.value or 0 for x in out], int(cnt[0].value), int(cnt[1].value))

    def decode_rows_until_device(self, d_ids: int, n_rows: int, width: int, ld: int | None = None, *, stop_text, dtype=np.int64, d_begin: int = 0, d_end: int = 0,
                                 stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False, keep_stop: bool = False, keep_stop_text: bool = False,
                                 errors: "str | None" = "replace", stream: int = 0) -> StoppedRowsDevice:
        """`decode_rows_text_device` with stop strings (tk_decode_rows_until_device); errors=None: the cut bytes, not repaired."""
        self._one_device("decode_rows_until_device")
        mode = until_mode(errors)
        stops = _StopSet(stop_text)
        spec = self._drows_spec(dtype, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(10, 4)
        rc = self._L.tk_decode_rows_until_device(self._h, d_ids or None, n_rows, width, width if ld is None else ld, d_begin or None, d_end or None, ctypes.byref(spec),
                                                 ctypes.byref(stops.c), _lib.STOPS_KEEP if keep_stop_text else 0, mode, stream or None, *refs)
        _lib.raise_for(rc)
        return StoppedRowsDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def decode_rows_until_packed(self, ids: np.ndarray, stop_text, *, begin=None, end=None, stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False,
                                 keep_stop: bool = False, keep_stop_text: bool = False, errors: "str | None" = "replace") -> StoppedRows:
        """`decode_rows_text_packed` with stop strings (tk_decode_rows_until); the matrix as there; errors=None: the cut bytes."""
        self._one_device("decode_rows_until_packed")
        mode = until_mode(errors)
        stops = _StopSet(stop_text)
        ids, n_rows, width, ld, begin, end, spec = self._host_matrix(ids, begin, end, stop, skip, skip_special, keep_stop)
        out, cnt, refs = self._outs(10, 4)
        rc = self._L.tk_decode_rows_until(self._h, ids.ctypes.data if n_rows and width else None, n_rows, width, ld, None if begin is None else begin.ctypes.data,
                                          None if end is None else end.ctypes.data, ctypes.byref(spec), ctypes.byref(stops.c), _lib.STOPS_KEEP if keep_stop_text else 0, mode,
                                          *refs)
        _lib.raise_for(rc)
        n_tokens, n_bytes = int(cnt[0].value), int(cnt[1].value)
        text = mode != _lib.U8_BYTES
        return StoppedRows(_take_u8(out[4], n_bytes), _take_u64(out[5], n_rows + 1), _take_u64(out[6], n_rows + 1) if text else None,
                           _take_u64(out[7], n_rows + 1) if text else None, _take_u32(out[0], n_tokens), _take_u64(out[1], n_rows + 1), _take_u32(out[2], n_rows),
                           _take_u32(out[3], n_rows), _take_u32(out[8], n_rows), _take_u32(out[9], n_rows))

    # ------------------------------------------------------------------ streaming decode: row slots on the device, fed a few ids per step
    def stream_create(self, n_rows: int, stop_text=(), *, w_max: int = 1, stop: Sequence[int] = (), skip: Sequence[int] = (), skip_special: bool = False,
                      keep_stop: bool = False, keep_stop_text: bool = False, errors: "str | None" = "replace") -> "NativeStream":
        """A decode stream of n_rows slots on this core's device (tk_stream_create); the arguments as in `decode_rows_until_packed`."""
        self._one_device("decode_stream")
        mode = until_mode(errors)
        stops = _StopSet(stop_text)
        spec = self._drows_spec(np.int64, stop, skip, skip_special, keep_stop)
        h = ctypes.c_void_p()
        _lib.raise_for(self._L.tk_stream_create(self._h, n_rows, w_max, ctypes.byref(spec), ctypes.byref(stops.c), _lib.STOPS_KEEP if keep_stop_text else 0, mode, ctypes.byref(h)))
        return NativeStream(self, h, n_rows, w_max, mode)

    # ------------------------------------------------------------------ token spans (tiktoken/core.py:303-335 over batches)
    def _one_device(self, what: str) -> None:
        if self._group is not None:
            raise ValueError(f"{what} runs on one device: this CoreBPE was built with {len(self.devices)}")

    def decode_batch_spans_packed(self, tokens: np.ndarray, tok_off: np.ndarray, *, want_bytes: bool = True, validate: bool = True):
        """One GPU call for a packed batch (tk_decode_batch_spans): where every token starts in its own document.
        Returns (data, byte_off, char_off, byte_start, char_start, invalid_doc):
          data         uint8 array of all decoded bytes back to back (None without want_bytes)
          byte_off     uint64[n_docs + 1], the bytes of the documents before each document; char_off likewise in chars
          byte_start   uint32[T], the byte of its document at which token i starts: its bytes are data[byte_off[d] + byte_start[i] : ...]
          char_start   uint32[T], the reference's offset (Encoding.decode_with_offsets, core.py:327-331)
          invalid_doc  with validate: the first document whose bytes are not well-formed UTF-8, or None -- the reference raises for it
                       (core.py:334); decode that document's bytes to get Python's own UnicodeDecodeError."""
        self._one_device("decode_batch_spans_packed")
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
        if tok_off.ndim != 1 or len(tok_off) < 1 or int(tok_off[-1]) != len(tokens):
            raise ValueError("tok_off must hold n_docs + 1 offsets ending at len(tokens)")
        n_docs = len(tok_off) - 1
        byte_off, char_off = np.empty(n_docs + 1, dtype=np.uint64), np.empty(n_docs + 1, dtype=np.uint64)
        data, nb, bs, cs, bad = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        src = tokens if len(tokens) else np.zeros(1, dtype=np.uint32)
        rc = self._L.tk_decode_batch_spans(self._h, src.ctypes.data, tok_off.ctypes.data, n_docs, 1 if validate else 0, ctypes.byref(data) if want_bytes else None,
                                           ctypes.byref(nb), ctypes.byref(bs), ctypes.byref(cs), byte_off.ctypes.data, char_off.ctypes.data, ctypes.byref(bad))
        _lib.raise_for(rc)
        n = len(tokens)
        return (_take_u8(data, nb.value) if want_bytes else None, byte_off, char_off, _take_u32(bs, n), _take_u32(cs, n),
                int(bad.value) if validate and bad.value != 0xFFFFFFFFFFFFFFFF else None)

    def token_spans_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_docs: int, d_doc_off: int = 0, stream: int = 0):
        """Device-resident spans (tk_token_spans_device): pointers to uint32 ids and uint64[n_docs + 1] token offsets on this core's device ->
        device pointers (byte_start uint32[n_tokens], char_start uint32[n_tokens], byte_off uint64[n_docs + 1], char_off uint64[n_docs + 1]),
        the library's buffers, valid until the next decode or spans call.  d_doc_off: the offsets of the documents' text when the ids are
        the result of `encode_batch_device` -- ValueError if a document's tokens do not add up to its text."""
        self._one_device("token_spans_device")
        out = [ctypes.c_void_p() for _ in range(4)]
        rc = self._L.tk_token_spans_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_docs, d_doc_off or None, stream or None,
                                           *[ctypes.byref(x) for x in out])
        _lib.raise_for(rc)
        return tuple(x.value or 0 for x in out)

    def encode_batch_spans_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *,
                                  disallowed_special=None):
        """`encode_batch_packed` plus the spans of the tokens it returns (tk_encode_batch_spans), computed while the ids are on the device:
        (tokens uint32[T], tok_off uint64[n+1], byte_start uint32[T], char_start uint32[T]); token i of document d is
        blob[doc_off[d] + byte_start[i] : ...].  ValueError naming the document where a pat_str leaves characters of the text unmatched."""
        self._one_device("encode_batch_spans_packed")
        text, dis, n_docs, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        tok_off = np.empty(n_docs + 1, dtype=np.uint64)
        out, n, bs, cs, hit = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_void_p(), _lib.SpecialHit()
        rc = self._L.tk_encode_batch_spans(self._h, *text, *dis, ctypes.byref(out), ctypes.byref(n), tok_off.ctypes.data, ctypes.byref(bs), ctypes.byref(cs),
                                           ctypes.byref(hit))
        self._raise_for(rc, hit)
        return _take_u32(out, n.value), tok_off, _take_u32(bs, n.value), _take_u32(cs, n.value)

    # ------------------------------------------------------------------ training rows (no reference counterpart: the host loop of its users)
    @staticmethod
    def _ids_spec(bos, eos, pad, dtype) -> "tuple[int, int, int, bool, bool]":
        """What tk_rows_spec and tk_pad_spec share: (bos_id, eos_id, pad_id, whether the caller has named a pad id -- eos stands in for it,
        whether the ids are 16-bit)"""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint32), np.dtype(np.uint16)):
            raise ValueError("dtype must be uint32 or uint16")
        for name, v in (("bos", bos), ("eos", eos), ("pad", pad)):
            if v is not None and not 0 <= int(v) < 0xFFFFFFFF:
                raise ValueError(f"{name} must be a token id below 2^32 - 1")
        if pad is None:
            pad = eos
        none = _lib.ROWS_NO_TOKEN
        return none if bos is None else int(bos), none if eos is None else int(eos), 0 if pad is None else int(pad), pad is not None, dtype == np.uint16

    @staticmethod
    def _width_spec(keep: str, padding_side: str, pad_to_multiple_of, **fit32) -> "tuple[bool, bool, int]":
        """What tk_pad_spec and tk_smp_spec share: (keep the tail, pad on the left, width_multiple); `fit32`: what else must fit 32 bits"""
        if keep not in ("head", "tail"):
            raise ValueError("keep must be 'head' or 'tail'")
        if padding_side not in ("right", "left"):
            raise ValueError("padding_side must be 'right' or 'left'")
        if pad_to_multiple_of is not None and int(pad_to_multiple_of) < 1:
            raise ValueError("pad_to_multiple_of must be at least 1 (None: the fixed width max_length)")
        for name, v in (*fit32.items(), ("pad_to_multiple_of", pad_to_multiple_of or 0)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit 32 bits")
        return keep == "tail", padding_side == "left", int(pad_to_multiple_of or 0)

    @staticmethod
    def _outs(n_ptr: int, n_cnt: int):
        """(pointers, counts, all of them by reference) for the result arrays and the figures a C entry hands back"""
        out, cnt = [ctypes.c_void_p() for _ in range(n_ptr)], [ctypes.c_uint64() for _ in range(n_cnt)]
        return out, cnt, [ctypes.byref(x) for x in out + cnt]

    @staticmethod
    def _own_mask(ptr: ctypes.c_void_p, n: int) -> np.ndarray:
        """A result's mask bytes.  A small result comes as a view of a bytes object: the caller gets an array of its own, as for the ids"""
        mask = _take_u8(ptr, n)
        return mask if mask.flags.writeable else mask.copy()

    @classmethod
    def _rows_spec(cls, seq_len: int, bos, eos, pad, drop_last: bool, dtype) -> "tuple[_lib.RowsSpec, bool]":
        """(the tk_rows_spec, whether the caller has named a pad id)"""
        bos_id, eos_id, pad_id, has_pad, ids16 = cls._ids_spec(bos, eos, pad, dtype)
        if not 0 <= int(seq_len) <= 0xFFFFFFFF:
            raise ValueError("seq_len must fit 32 bits")
        flags = (_lib.ROWS_DROP_LAST if drop_last else 0) | (_lib.ROWS_IDS16 if ids16 else 0)
        return _lib.RowsSpec(int(seq_len), bos_id, eos_id, pad_id, flags), has_pad

    @staticmethod
    def _pad_needed(has_pad: bool, drop_last: bool, n_stream: int, seq_len: int) -> None:
        if not has_pad and not drop_last and seq_len and n_stream % seq_len:
            raise ValueError(f"the stream of {n_stream} ids does not fill rows of {seq_len}: name a pad or eos id, or pass drop_last=True")

    def pack_rows_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_docs: int, *, seq_len: int, bos: int | None = None, eos: int | None = None,
                         pad: int | None = None, drop_last: bool = False, dtype=np.uint32, stream: int = 0) -> RowsDevice:
        """Device-resident rows (tk_pack_rows_device): pointers to uint32 ids and uint64[n_docs + 1] token offsets on this core's device -- e.g.
        what `encode_batch_device` returns, which stays intact -- cut into rows of `seq_len`; see `PackedRows` for the arrays.  `bos` / `eos`:
        ids put before / after every document; `pad` (default: eos) fills the last row unless `drop_last`; dtype uint16: 16-bit ids."""
        self._one_device("pack_rows_device")
        spec, has_pad = self._rows_spec(seq_len, bos, eos, pad, drop_last, dtype)
        k = (bos is not None) + (eos is not None)
        self._pad_needed(has_pad, drop_last, n_tokens + n_docs * k, spec.seq_len)
        out, cnt, refs = self._outs(5, 4)
        rc = self._L.tk_pack_rows_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_docs, ctypes.byref(spec), stream or None, *refs)
        _lib.raise_for(rc)
        return RowsDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def encode_batch_rows_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                 seq_len: int, bos: int | None = None, eos: int | None = None, pad: int | None = None, drop_last: bool = False,
                                 dtype=np.uint32) -> PackedRows:
        """`encode_batch_packed` with its result cut into training rows while the ids are on the device (tk_encode_batch_rows): only the row
        arrays come back.  The special-token arguments as in `encode_batch_packed`, the others as in `pack_rows_device`."""
        self._one_device("encode_batch_rows_packed")
        text, dis, n_docs, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        spec, has_pad = self._rows_spec(seq_len, bos, eos, pad, drop_last, dtype)
        hit = _lib.SpecialHit()
        out, cnt, refs = self._outs(5, 4)
        rc = self._L.tk_encode_batch_rows(self._h, *text, *dis, ctypes.byref(spec), *refs, ctypes.byref(hit))
        self._raise_for(rc, hit)
        n_rows, n_segs, n_stream, n_tail = (int(x.value) for x in cnt)
        L = spec.seq_len
        m = n_rows * L + n_tail
        arrays = [_take(out[0], m, dtype), _take_u32(out[1], m), _take_u32(out[2], m)]
        cu, row_seg = _take_u32(out[3], n_segs + 1), _take_u32(out[4], n_rows + 1)
        self._pad_needed(has_pad, drop_last, n_stream, L)
        return PackedRows(*[a[: n_rows * L].reshape(n_rows, L) for a in arrays], cu, row_seg, n_stream, *[a[n_rows * L:] for a in arrays])

    # ------------------------------------------------------------------ padded model inputs (no reference counterpart: the host loop of its users)
    @classmethod
    def _pad_spec(cls, max_length: int, stride: int, windows: bool, keep: str, padding_side: str, pad_to_multiple_of, bos, eos, pad, dtype) -> "tuple[_lib.PadSpec, bool]":
        """(the tk_pad_spec, whether the caller has named a pad id)"""
        bos_id, eos_id, pad_id, has_pad, ids16 = cls._ids_spec(bos, eos, pad, dtype)
        tail, left, width_multiple = cls._width_spec(keep, padding_side, pad_to_multiple_of, max_length=max_length, stride=stride)
        flags = (_lib.PAD_WINDOWS if windows else 0) | (_lib.PAD_KEEP_TAIL if tail else 0) | (_lib.PAD_LEFT if left else 0) | (_lib.PAD_IDS16 if ids16 else 0)
        return _lib.PadSpec(int(max_length), int(stride), width_multiple, bos_id, eos_id, pad_id, flags), has_pad

    @staticmethod
    def _pad_id_needed(has_pad: bool, n_rows: int, width: int, lengths) -> None:
        if not has_pad and n_rows and int(lengths.min()) < width:
            raise ValueError(f"a row of {int(lengths.min())} ids does not fill the width of {width}: name a pad or eos id")

    def pad_batch_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_docs: int, *, max_length: int, stride: int = 0, windows: bool = False,
                         keep: str = "head", padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None,
                         pad: int | None = None, dtype=np.uint32, stream: int = 0) -> PaddedDevice:
        """Device-resident padded rows (tk_pad_batch_device): pointers to uint32 ids and uint64[n_docs + 1] token offsets on this core's
        device -- e.g. what `encode_batch_device` returns, which stays intact --, one row per document cut to `max_length` (`keep`: its
        head or its tail) or, with `windows`, further rows that overlap by `stride`; see `PaddedBatch` for the arrays.  `bos` / `eos`: ids
        put before / after every row's body; `pad` (default: eos; one of the two must be named); `pad_to_multiple_of`: the width is the longest row rounded up to a
        multiple of it, at most `max_length` (None: `max_length`); dtype uint16: 16-bit ids."""
        self._one_device("pad_batch_device")
        spec, has_pad = self._pad_spec(max_length, stride, windows, keep, padding_side, pad_to_multiple_of, bos, eos, pad, dtype)
        if not has_pad:  # (the lengths stay on the device: whether a row needs padding cannot be seen from here)
            raise ValueError("pad_batch_device: name a pad or eos id")
        out, cnt, refs = self._outs(6, 2)
        rc = self._L.tk_pad_batch_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_docs, ctypes.byref(spec), stream or None, *refs)
        _lib.raise_for(rc)
        return PaddedDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def encode_batch_padded_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                   max_length: int, stride: int = 0, windows: bool = False, keep: str = "head", padding_side: str = "right",
                                   pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None, pad: int | None = None,
                                   dtype=np.uint32) -> PaddedBatch:
        """`encode_batch_packed` with its result padded while the ids are on the device (tk_encode_batch_padded): only the padded arrays
        come back.  The special-token arguments as in `encode_batch_packed`, the others as in `pad_batch_device`."""
        self._one_device("encode_batch_padded_packed")
        text, dis, n_docs, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        spec, has_pad = self._pad_spec(max_length, stride, windows, keep, padding_side, pad_to_multiple_of, bos, eos, pad, dtype)
        hit = _lib.SpecialHit()
        out, cnt, refs = self._outs(6, 2)
        rc = self._L.tk_encode_batch_padded(self._h, *text, *dis, ctypes.byref(spec), *refs, ctypes.byref(hit))
        self._raise_for(rc, hit)
        n_rows, width = (int(x.value) for x in cnt)
        input_ids = _take(out[0], n_rows * width, dtype).reshape(n_rows, width)
        mask = self._own_mask(out[1], n_rows * width).reshape(n_rows, width)
        lengths, row_doc, row_tok, doc_row = _take_u32(out[2], n_rows), _take_u32(out[3], n_rows), _take_u32(out[4], n_rows), _take_u32(out[5], n_docs + 1)
        self._pad_id_needed(has_pad, n_rows, width, lengths)
        return PaddedBatch(input_ids, mask, lengths, row_doc, row_tok, doc_row)

    # ------------------------------------------------------------------ text chunks (no reference counterpart: the host loop of its users)
    @staticmethod
    def _split_spec(max_tokens: int, min_tokens, overlap: int, separators, seg_tokens: int) -> "_lib.SplitSpec":
        """The tk_split_spec.  min_tokens None: max(overlap + 1, max_tokens // 2).  separators: levels, best first, of (tail, head) pairs
        of str or bytes; a bare str / bytes x means (x, "").  What does not fit the structure is refused here, in the library's words;
        the library refuses the rest."""
        if min_tokens is None:
            min_tokens = max(int(overlap) + 1, int(max_tokens) // 2)
        for name, v in (("max_tokens", max_tokens), ("min_tokens", min_tokens), ("overlap", overlap), ("seg_tokens", seg_tokens)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit 32 bits")
        levels = [list(lv) for lv in separators]
        if len(levels) > 4:
            raise ValueError("n_levels: at most 4 levels of separators")
        spec = _lib.SplitSpec(int(max_tokens), int(min_tokens), int(overlap), len(levels), int(seg_tokens), 0)
        for l, seps in enumerate(levels):
            if len(seps) > 4:
                raise ValueError("n_seps: at most 4 separators in a level")
            spec.n_seps[l] = len(seps)
            for k, sp in enumerate(seps):
                tail, head = (sp, b"") if isinstance(sp, (str, bytes)) else sp
                tail, head = (x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in (tail, head))
                if len(tail) > 16 or len(head) > 16:
                    raise ValueError("separators: a part (tail, head) is at most 16 bytes")
                o = spec.sep[l][k]
                o.tail_len, o.head_len = len(tail), len(head)
                o.tail[:len(tail)] = tail
                o.head[:len(head)] = head
        return spec

    def split_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_docs: int, d_utf8: int, d_doc_off: int, *, max_tokens: int, min_tokens: int | None = None,
                     overlap: int = 0, separators=DEFAULT_SEPARATORS, seg_tokens: int = 0, stream: int = 0) -> SplitDevice:
        """Device-resident text chunks (tk_split_device): pointers to uint32 ids, uint64[n_docs + 1] token offsets, the text they were encoded
        from and its uint64[n_docs + 1] byte offsets on this core's device -- e.g. the arguments and results of `encode_batch_device`, which
        stay intact; every document is cut into chunks of at most `max_tokens` tokens at the best separator in the window
        [`min_tokens`, `max_tokens`], consecutive chunks sharing up to `overlap` tokens; see `TextChunks` for the arrays."""
        self._one_device("split_device")
        spec = self._split_spec(max_tokens, min_tokens, overlap, separators, seg_tokens)
        out, cnt, refs = self._outs(9, 1)
        rc = self._L.tk_split_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_docs, d_utf8 or None, d_doc_off or None, ctypes.byref(spec), stream or None, *refs)
        _lib.raise_for(rc)
        return SplitDevice(*[x.value or 0 for x in out], int(cnt[0].value))

    def encode_batch_split_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                  max_tokens: int, min_tokens: int | None = None, overlap: int = 0, separators=DEFAULT_SEPARATORS, seg_tokens: int = 0) -> TextChunks:
        """`encode_batch_packed` with the text cut into chunks while ids and text are on the device (tk_encode_batch_split).  The
        special-token arguments as in `encode_batch_packed`, the others as in `split_device`."""
        self._one_device("encode_batch_split_packed")
        text, dis, n_docs, keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        spec = self._split_spec(max_tokens, min_tokens, overlap, separators, seg_tokens)
        hit = _lib.SpecialHit()
        out, cnt, _ = self._outs(10, 2)
        tok_off = np.empty(n_docs + 1, dtype=np.uint64)
        refs = [ctypes.byref(x) for x in (*out[:9], cnt[0], out[9], cnt[1])]
        rc = self._L.tk_encode_batch_split(self._h, *text, *dis, ctypes.byref(spec), *refs, tok_off.ctypes.data, ctypes.byref(hit))
        self._raise_for(rc, hit)
        C, n = int(cnt[0].value), int(cnt[1].value)
        arrays = [_take_u32(x, C) for x in out[:7]] + [self._own_mask(out[7], C), _take_u32(out[8], n_docs + 1)]
        return TextChunks(arrays, _take_u32(out[9], n), tok_off, keep[0], keep[1])

    # ------------------------------------------------------------------ JSON Lines (no reference counterpart: the host loop of its users)
    @staticmethod
    def _jsonl_args(field, on_error: str):
        f = field.encode("utf-8") if isinstance(field, str) else bytes(field)
        if on_error not in _lib.JSONL_MODES:
            raise ValueError(f"on_error={on_error!r}: 'raise', 'skip' or 'empty'")
        return np.frombuffer(f + b"\0", dtype=np.uint8), len(f), _lib.JSONL_MODES[on_error]

    @staticmethod
    def _jsonl_bytes(data) -> np.ndarray:
        """bytes, bytearray, memoryview, mmap or a uint8 array as a uint8 view: no copy"""
        a = data if isinstance(data, np.ndarray) else np.frombuffer(data, dtype=np.uint8)
        if a.dtype != np.uint8 or a.ndim != 1 or not a.flags.c_contiguous:
            raise ValueError("data must be contiguous bytes (bytes, bytearray, memoryview, mmap or a one-dimensional uint8 array)")
        return a

    def _jsonl_raise(self, rc: int, bad: "_lib.JsonlBad", hit=None) -> None:
        if rc == _lib.TK_JSONL_ERROR:
            raise JsonlError(int(bad.line), int(bad.pos), int(bad.status), _lib.last_error())
        if hit is not None:
            self._raise_for(rc, hit)
        _lib.raise_for(rc)

    def jsonl_extract_device(self, d_bytes: int, n_bytes: int, field="text", on_error: str = "raise", stream: int = 0) -> JsonlDevice:
        """Device-resident JSON Lines (tk_jsonl_extract_device): a pointer to n_bytes bytes on this core's device; the unescaped text of
        `field` of every line stays there, packed as `encode_batch_device` takes it.  See `JsonlText` for the arrays."""
        self._one_device("jsonl_extract_device")
        f, flen, mode = self._jsonl_args(field, on_error)
        out, cnt, refs = self._outs(5, 3)
        bad = _lib.JsonlBad()
        rc = self._L.tk_jsonl_extract_device(self._h, d_bytes or None, n_bytes, f.ctypes.data, flen, mode, stream or None, *refs, ctypes.byref(bad))
        self._jsonl_raise(rc, bad)
        return JsonlDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def jsonl_extract_packed(self, data, field="text", on_error: str = "raise") -> JsonlText:
        """One field of every line of a JSON Lines buffer (tk_jsonl_extract): host bytes in, a `JsonlText` out."""
        self._one_device("jsonl_extract_packed")
        src = self._jsonl_bytes(data)
        f, flen, mode = self._jsonl_args(field, on_error)
        out, cnt, refs = self._outs(5, 3)
        bad = _lib.JsonlBad()
        rc = self._L.tk_jsonl_extract(self._h, src.ctypes.data if len(src) else None, len(src), f.ctypes.data, flen, mode, *refs, ctypes.byref(bad))
        self._jsonl_raise(rc, bad)
        n_docs, n_lines, n_text = (int(x.value) for x in cnt)
        return JsonlText(self._own_mask(out[0], n_text), _take_u64(out[1], n_docs + 1), _take_u64(out[2], n_docs), self._own_mask(out[4], n_lines), n_lines,
                         _take_u64(out[3], n_lines + 1))

    def encode_jsonl_packed(self, data, field="text", on_error: str = "raise", allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None) -> JsonlTokens:
        """A JSON Lines buffer encoded (tk_encode_jsonl): the field is extracted and encoded while it is on the device.  The special-token
        arguments as in `encode_batch_packed`; a `DisallowedSpecialError` names the document (`doc`), not the line."""
        self._one_device("encode_jsonl_packed")
        src = self._jsonl_bytes(data)
        f, flen, mode = self._jsonl_args(field, on_error)
        ids, k = (np.zeros(1, dtype=np.uint32), 0) if allowed_special is None else self._allowed_ids(allowed_special)
        dis, n_dis = self._disallowed_ids(disallowed_special)
        out, cnt = [ctypes.c_void_p() for _ in range(4)], [ctypes.c_uint64() for _ in range(3)]
        hit, bad = _lib.SpecialHit(), _lib.JsonlBad()
        rc = self._L.tk_encode_jsonl(self._h, src.ctypes.data if len(src) else None, len(src), f.ctypes.data, flen, mode, 0 if allowed_special is None else 1, ids.ctypes.data, k,
                                     dis.ctypes.data, n_dis, ctypes.byref(out[0]), ctypes.byref(cnt[0]), ctypes.byref(out[1]), ctypes.byref(out[2]), ctypes.byref(out[3]),
                                     ctypes.byref(cnt[1]), ctypes.byref(cnt[2]), ctypes.byref(hit), ctypes.byref(bad))
        self._jsonl_raise(rc, bad, hit)
        n_tok, n_docs, n_lines = (int(x.value) for x in cnt)
        return JsonlTokens(_take_u32(out[0], n_tok), _take_u64(out[1], n_docs + 1), _take_u64(out[2], n_docs), self._own_mask(out[3], n_lines), n_lines)

    # ------------------------------------------------------------------ near-duplicate fingerprints (no reference counterpart: the host step of its users)
    @staticmethod
    def _fp_spec(ngram: int, n_perm: int, bands: int, seed: int) -> "_lib.FingerprintSpec":
        """The tk_fingerprint_spec; what does not fit the structure is refused here, the library refuses the rest."""
        for name, v in (("ngram", ngram), ("n_perm", n_perm), ("bands", bands)):
            if not 0 <= int(v) <= 0xFFFFFFFF:
                raise ValueError(f"{name} must fit 32 bits")
        if not 0 <= int(seed) <= 0xFFFFFFFFFFFFFFFF:
            raise ValueError("seed must fit 64 bits")
        return _lib.FingerprintSpec(int(ngram), int(n_perm), int(bands), int(seed))

    def fingerprint_device(self, tokens, tok_off, *, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0, sig=None, band=None, exact=None, n_shingles=None,
                           stream: int | None = None) -> None:
        """Device-resident fingerprints (tk_fingerprint_device): torch tensors on this core's device, taken by pointer -- `tokens` (a
        32-bit dtype) and `tok_off` (a 64-bit dtype, n_docs + 1 entries ascending from 0 to len(tokens)) in; the caller's tensors out, any
        of which may be None: `sig` (32-bit, n_docs * n_perm), `band` (64-bit, n_docs * bands), `exact` and `n_shingles` (64-bit, n_docs).
        The work is queued on `stream` -- a HIP stream handle; default: torch's current stream of the device; 0 is the null stream, which is
        torch's default stream -- and the call does not wait for it: it is ordered on that stream like a kernel torch itself had launched."""
        import torch

        self._one_device("fingerprint_device")
        spec = self._fp_spec(ngram, n_perm, bands, seed)
        n_docs = tok_off.numel() - 1
        if n_docs < 0:
            raise ValueError("tok_off must hold n_docs + 1 entries")
        for name, t, size, count in (("tokens", tokens, 4, tokens.numel()), ("tok_off", tok_off, 8, n_docs + 1), ("sig", sig, 4, n_docs * spec.n_perm),
                                     ("band", band, 8, n_docs * spec.bands), ("exact", exact, 8, n_docs), ("n_shingles", n_shingles, 8, n_docs)):
            if t is None:
                continue
            if not t.is_cuda or t.device.index != self.device or not t.is_contiguous() or t.element_size() != size or t.numel() != count:
                raise ValueError(f"{name} must be a contiguous tensor of {count} elements of {size} bytes on this core's GPU")
        if stream is None:
            stream = torch.cuda.current_stream(tokens.device).cuda_stream
        ptr = [t.data_ptr() if t is not None and t.numel() else None for t in (sig, band, exact, n_shingles)]
        rc = self._L.tk_fingerprint_device(self._h, tokens.data_ptr() if tokens.numel() else None, tokens.numel(), tok_off.data_ptr(), n_docs, ctypes.byref(spec),
                                           stream or None, *ptr)  # (a null handle is the null stream here, not the core's stream)
        _lib.raise_for(rc)

    def fingerprint_packed(self, tokens: np.ndarray, tok_off: np.ndarray, *, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> Fingerprints:
        """The fingerprints of packed tokens (tk_fingerprint): host arrays in -- `tokens` uint32[T], `tok_off` uint64[n + 1] --, a
        `Fingerprints` out."""
        self._one_device("fingerprint_packed")
        tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        tok_off = np.ascontiguousarray(tok_off, dtype=np.uint64)
        if tok_off.ndim != 1 or tokens.ndim != 1 or len(tok_off) < 1 or int(tok_off[-1]) != len(tokens):
            raise ValueError("tok_off must hold n + 1 offsets that end at len(tokens)")
        spec = self._fp_spec(ngram, n_perm, bands, seed)
        n = len(tok_off) - 1
        out = self._fp_outs(n, spec)
        rc = self._L.tk_fingerprint(self._h, tokens.ctypes.data if len(tokens) else None, tok_off.ctypes.data, n, ctypes.byref(spec), *[a.ctypes.data for a in out])
        _lib.raise_for(rc)
        return Fingerprints(*out, np.diff(tok_off))

    @staticmethod
    def _fp_outs(n: int, spec: "_lib.FingerprintSpec"):
        """(sig, band, exact, n_shingles) for n documents, to be filled by the library (one spare element each: no empty array's pointer)"""
        P, B = max(int(spec.n_perm), 1), max(int(spec.bands), 1)
        return (np.zeros(n * P + 1, dtype=np.uint32)[:n * P].reshape(n, P), np.zeros(n * B + 1, dtype=np.uint64)[:n * B].reshape(n, B),
                np.zeros(n + 1, dtype=np.uint64)[:n], np.zeros(n + 1, dtype=np.uint64)[:n])

    def encode_batch_fingerprint_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                        ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> Fingerprints:
        """`encode_batch_packed` with its result fingerprinted while the ids are on the device (tk_encode_batch_fingerprint): the ids stay
        there, only the `Fingerprints` come back.  The special-token arguments as in `encode_batch_packed`."""
        self._one_device("encode_batch_fingerprint_packed")
        text, dis, n_docs, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        spec = self._fp_spec(ngram, n_perm, bands, seed)
        hit = _lib.SpecialHit()
        out = self._fp_outs(n_docs, spec)
        tok_off = np.zeros(n_docs + 1, dtype=np.uint64)
        rc = self._L.tk_encode_batch_fingerprint(self._h, *text, *dis, ctypes.byref(spec), *[a.ctypes.data for a in out], tok_off.ctypes.data, None, None, ctypes.byref(hit))
        self._raise_for(rc, hit)
        return Fingerprints(*out, np.diff(tok_off))

    # ------------------------------------------------------------------ supervised samples (no reference counterpart: the host loop of its users)
    @staticmethod
    def _role_table(roles: "Sequence[Role]"):
        """(n_roles, role_ids uint32[], role_off uint32[2 n + 1], role_train uint8[n]) of a sequence of Role; the limits are the library's to refuse"""
        ids, off, train = [], [0], []
        for r in roles:
            before, after, t = r
            for run in (before, after):
                for v in run:
                    if not 0 <= int(v) <= 0xFFFFFFFF:
                        raise ValueError("a role's ids must be token ids below 2^32")
                    ids.append(int(v))
                off.append(len(ids))
            train.append(1 if t else 0)
        return (len(train), np.array(ids if ids else [0], dtype=np.uint32), np.array(off, dtype=np.uint32), np.array(train if train else [0], dtype=np.uint8))

    @classmethod
    def _smp_spec(cls, max_length: int, keep: str, padding_side: str, pad_to_multiple_of, bos, eos, pad: int, ignore_index: int) -> "_lib.SmpSpec":
        tail, left, width_multiple = cls._width_spec(keep, padding_side, pad_to_multiple_of, max_length=max_length, pad=pad)
        for name, v in (("bos", bos), ("eos", eos)):
            if v is not None and not 0 <= int(v) < 0xFFFFFFFF:
                raise ValueError(f"{name} must be a token id below 2^32 - 1")
        if not -(1 << 31) <= int(ignore_index) < (1 << 31):
            raise ValueError("ignore_index must fit a signed 32-bit integer")
        none = _lib.ROWS_NO_TOKEN
        flags = (_lib.SMP_KEEP_TAIL if tail else 0) | (_lib.SMP_LEFT if left else 0)
        return _lib.SmpSpec(int(max_length), width_multiple, none if bos is None else int(bos), none if eos is None else int(eos), int(pad), int(ignore_index), flags)

    def assemble_samples_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_parts: int, d_part_role: int, d_sample_off: int, n_samples: int,
                                roles: "Sequence[Role]", *, max_length: int, keep: str = "head", padding_side: str = "right", pad_to_multiple_of: int | None = None,
                                bos: int | None = None, eos: int | None = None, pad: int = 0, ignore_index: int = -100, stream: int = 0) -> SamplesDevice:
        """Device-resident supervised samples (tk_assemble_samples_device): pointers to uint32 ids and uint64[n_parts + 1] token offsets on
        this core's device -- e.g. what `encode_batch_device` returns, which stays intact --, to uint8[n_parts] roles of the parts and to
        uint64[n_samples + 1] offsets that group the parts into samples; `roles`: a sequence of `Role` (host side).  One row per sample, cut
        to `max_length` (`keep`: its head or its tail); see `SampleBatch` for the arrays."""
        self._one_device("assemble_samples_device")
        spec = self._smp_spec(max_length, keep, padding_side, pad_to_multiple_of, bos, eos, pad, ignore_index)
        n_roles, ids, off, train = self._role_table(roles)
        out, cnt, refs = self._outs(6, 2)
        rc = self._L.tk_assemble_samples_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_parts, d_part_role or None, d_sample_off or None, n_samples,
                                                n_roles, ids.ctypes.data, off.ctypes.data, train.ctypes.data, ctypes.byref(spec), stream or None, *refs)
        _lib.raise_for(rc)
        return SamplesDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def encode_batch_samples_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                    part_role, sample_off, roles: "Sequence[Role]", max_length: int, keep: str = "head", padding_side: str = "right",
                                    pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None, pad: int = 0,
                                    ignore_index: int = -100) -> SampleBatch:
        """`encode_batch_packed` over the parts' text with the samples assembled while the ids are on the device (tk_encode_batch_samples):
        only the sample arrays come back.  doc_off holds the parts' byte offsets; `part_role` (one index into `roles` per part) and
        `sample_off` (n_samples + 1 part offsets) group them.  The special-token arguments as in `encode_batch_packed` -- a disallowed
        special token raises DisallowedSpecialError whose `doc` is the part --, the others as in `assemble_samples_device`."""
        self._one_device("encode_batch_samples_packed")
        text, dis, n_parts, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        roles_in = np.asarray(part_role)
        if roles_in.size and (roles_in.min() < 0 or roles_in.max() > 255):
            raise ValueError("part_role must hold role indices below 256")
        part_role = np.ascontiguousarray(roles_in, dtype=np.uint8)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        if part_role.ndim != 1 or len(part_role) != n_parts:
            raise ValueError("part_role must hold one role per part")
        if sample_off.ndim != 1 or len(sample_off) < 1:
            raise ValueError("sample_off must hold n_samples + 1 offsets (at least one)")
        n_samples = len(sample_off) - 1
        spec = self._smp_spec(max_length, keep, padding_side, pad_to_multiple_of, bos, eos, pad, ignore_index)
        n_roles, ids, off, train = self._role_table(roles)
        hit = _lib.SpecialHit()
        out, cnt, refs = self._outs(6, 2)
        held = part_role if n_parts else np.zeros(1, dtype=np.uint8)
        rc = self._L.tk_encode_batch_samples(self._h, *text, *dis, held.ctypes.data, sample_off.ctypes.data, n_samples, n_roles, ids.ctypes.data, off.ctypes.data,
                                             train.ctypes.data, ctypes.byref(spec), *refs, ctypes.byref(hit))
        self._raise_for(rc, hit)
        n_rows, width = (int(x.value) for x in cnt)
        n = n_rows * width
        input_ids = _take_u32(out[0], n).reshape(n_rows, width)
        mask = self._own_mask(out[1], n)
        labels = _take_u32(out[2], n).view(np.int32).reshape(n_rows, width)
        return SampleBatch(input_ids, mask.reshape(n_rows, width), labels, _take_u32(out[3], n_rows), _take_u64(out[4], n_rows), _take_u32(out[5], n_rows))

    # ------------------------------------------------------------------ packed sample rows (no reference counterpart: the collator of its users)
    @classmethod
    def _srow_spec(cls, max_length: int, keep: str, skip_long: bool, ignore_first: bool, padding_side: str, pad_to_multiple_of, bos, eos, pad: int,
                   ignore_index: int) -> "_lib.SmpSpec":
        """The tk_smp_spec of a packed-samples call; `padding_side` and `pad_to_multiple_of` are passed on for the library to refuse"""
        spec = cls._smp_spec(max_length, keep, padding_side, pad_to_multiple_of, bos, eos, pad, ignore_index)
        spec.flags |= (_lib.SMP_SKIP_LONG if skip_long else 0) | (_lib.SMP_IGNORE_FIRST if ignore_first else 0)
        return spec

    def pack_samples_device(self, d_tokens: int, n_tokens: int, d_tok_off: int, n_parts: int, d_part_role: int, d_sample_off: int, n_samples: int,
                            roles: "Sequence[Role]", *, max_length: int, keep: str = "head", skip_long: bool = False, ignore_first: bool = False,
                            padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None, pad: int = 0,
                            ignore_index: int = -100, stream: int = 0) -> SampleRowsDevice:
        """Device-resident packed sample rows (tk_pack_samples_device): the arguments of `assemble_samples_device`; the samples go several
        to a row of `max_length`, next-fit in input order; see `SampleRows` for the arrays.  `skip_long`: an over-long sample is left out
        instead of cut; `ignore_first`: the label of every sample's first element is `ignore_index`.  The rows are `max_length` wide and
        padded on the right: `padding_side="left"` and `pad_to_multiple_of` are refused."""
        self._one_device("pack_samples_device")
        spec = self._srow_spec(max_length, keep, skip_long, ignore_first, padding_side, pad_to_multiple_of, bos, eos, pad, ignore_index)
        n_roles, ids, off, train = self._role_table(roles)
        out, cnt, refs = self._outs(12, 2)
        rc = self._L.tk_pack_samples_device(self._h, d_tokens or None, n_tokens, d_tok_off or None, n_parts, d_part_role or None, d_sample_off or None, n_samples,
                                            n_roles, ids.ctypes.data, off.ctypes.data, train.ctypes.data, ctypes.byref(spec), stream or None, *refs)
        _lib.raise_for(rc)
        return SampleRowsDevice(*[x.value or 0 for x in out], *[int(x.value) for x in cnt])

    def encode_batch_sample_rows_packed(self, blob: np.ndarray, doc_off: np.ndarray, allowed_special: AbstractSet[str] | None = None, *, disallowed_special=None,
                                        part_role, sample_off, roles: "Sequence[Role]", max_length: int, keep: str = "head", skip_long: bool = False,
                                        ignore_first: bool = False, padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None,
                                        eos: int | None = None, pad: int = 0, ignore_index: int = -100) -> SampleRows:
        """`encode_batch_packed` over the parts' text with the samples packed into rows while the ids are on the device
        (tk_encode_batch_sample_rows): only the row arrays come back.  The text and special-token arguments as in
        `encode_batch_samples_packed`, the others as in `pack_samples_device`."""
        self._one_device("encode_batch_sample_rows_packed")
        text, dis, n_parts, _keep = self._batch_args(blob, doc_off, allowed_special, disallowed_special)
        roles_in = np.asarray(part_role)
        if roles_in.size and (roles_in.min() < 0 or roles_in.max() > 255):
            raise ValueError("part_role must hold role indices below 256")
        part_role = np.ascontiguousarray(roles_in, dtype=np.uint8)
        sample_off = np.ascontiguousarray(sample_off, dtype=np.uint64)
        if part_role.ndim != 1 or len(part_role) != n_parts:
            raise ValueError("part_role must hold one role per part")
        if sample_off.ndim != 1 or len(sample_off) < 1:
            raise ValueError("sample_off must hold n_samples + 1 offsets (at least one)")
        n_samples = len(sample_off) - 1
        spec = self._srow_spec(max_length, keep, skip_long, ignore_first, padding_side, pad_to_multiple_of, bos, eos, pad, ignore_index)
        n_roles, ids, off, train = self._role_table(roles)
        hit = _lib.SpecialHit()
        out, cnt, refs = self._outs(12, 2)
        held = part_role if n_parts else np.zeros(1, dtype=np.uint8)
        rc = self._L.tk_encode_batch_sample_rows(self._h, *text, *dis, held.ctypes.data, sample_off.ctypes.data, n_samples, n_roles, ids.ctypes.data, off.ctypes.data,
                                                 train.ctypes.data, ctypes.byref(spec), *refs, ctypes.byref(hit))
        self._raise_for(rc, hit)
        n_rows, n_segs = (int(x.value) for x in cnt)
        L = int(spec.max_len)
        n = n_rows * L
        grid = [_take_u32(out[i], n).reshape(n_rows, L) for i in range(4)]
        grid[1] = grid[1].view(np.int32)
        return SampleRows(*grid, _take_u32(out[4], n_segs + 1), _take_u32(out[5], n_rows + 1), _take_u32(out[6], n_rows + 1), _take_u32(out[7], n_samples),
                          _take_u64(out[8], n_samples), _take_u32(out[9], n_samples), _take_u32(out[10], n_samples), _take_u32(out[11], n_samples))

    # ------------------------------------------------------------------ training (tiktoken/_educational.py: bpe_train)
    def train_bpe_packed(self, blob: np.ndarray, doc_off: np.ndarray, vocab_size: int) -> tuple[np.ndarray, np.ndarray]:
        """The merges the reference's `bpe_train` makes on a packed batch under this core's pat_str (tk_train_bpe; the rule:
        include/tiktoken_amd.h): (pairs uint32[n, 2], counts uint64[n]) with n = vocab_size - 256 -- merge k joins the symbols pairs[k]
        (0..255: the bytes, 256 + j: merge j) into symbol 256 + k, and counts[k] is that pair's weighted count when it won.  The core's
        ranks play no part.  ValueError for vocab_size < 256, for a text that runs out of pairs, for a document longer than a chunk."""
        self._one_device("train_bpe_packed")
        if not 0 <= int(vocab_size) <= 0xFFFFFFFF:
            raise ValueError("vocab_size must fit 32 bits")
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        doc_off = np.ascontiguousarray(doc_off, dtype=np.uint64)
        _check_packed(blob, doc_off)
        src = blob if len(blob) else np.zeros(1, dtype=np.uint8)
        pairs, counts, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._L.tk_train_bpe(self._h, src.ctypes.data, doc_off.ctypes.data, len(doc_off) - 1, int(vocab_size), ctypes.byref(pairs), ctypes.byref(counts),
                                  ctypes.byref(n))
        _lib.raise_for(rc)
        k = int(n.value)
        p = np.frombuffer(ctypes.string_at(pairs, k * 8), dtype=np.uint32).reshape(k, 2).copy()
        cn = np.frombuffer(ctypes.string_at(counts, k * 8), dtype=np.uint64).copy()
        self._L.tk_free(pairs)
        self._L.tk_free(counts)
        return p, cn

    def decode_single_token_bytes(self, token: int) -> bytes:
        if not 0 <= token <= 0xFFFFFFFF:
            raise KeyError(str(token))
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        rc = self._L.tk_decode_single_token_bytes(self._h, token, ctypes.byref(p), ctypes.byref(n))
        _lib.raise_for(rc, key=str(token))
        return ctypes.string_at(p, n.value)

    def token_byte_values(self) -> list[bytes]:
        return list(self._sorted_tokens())

    def _sorted_tokens(self) -> list[bytes]:
        """All token byte strings in lexicographic order (lib.rs:648-650), fetched once per CoreBPE in one call."""
        cached = getattr(self, "_sorted_cache", None)
        if cached is None:
            pb, po, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
            _lib.raise_for(self._L.tk_sorted_tokens_packed(self._h, ctypes.byref(pb), ctypes.byref(po), ctypes.byref(n)))
            off = np.ctypeslib.as_array(ctypes.cast(po, ctypes.POINTER(ctypes.c_uint64)), shape=(n.value + 1,))
            blob = ctypes.string_at(pb, int(off[-1]))
            bounds = off.tolist()
            cached = self._sorted_cache = [blob[a:b] for a, b in zip(bounds[:-1], bounds[1:])]
        return cached

    def set_output_buffers(self, n: int):
        """`encode_batch_device` alternates between n (1 or 2) pairs of result buffers: with 2 the result of a call stays valid while the
        next call runs (tk_set_output_buffers; the several-process gather of tiktoken_amd.distributed sends from it without a copy)."""
        _lib.raise_for(self._L.tk_set_output_buffers(self._h, int(n)))

    # ------------------------------------------------------------------ instrumentation
    def set_profiling(self, on: bool):
        self._L.tk_set_profiling(self._h, 1 if on else 0)

    def reset_kernel_ms(self):
        self._L.tk_reset_kernel_ms(self._h)

    def kernel_ms(self, name: str) -> tuple[float, int]:
        ms, n = ctypes.c_double(), ctypes.c_uint64()
        self._L.tk_get_kernel_ms(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value

    def last_stats(self) -> dict:
        v = [ctypes.c_uint64() for _ in range(6)]
        self._L.tk_last_stats(self._h, *[ctypes.byref(x) for x in v])
        return dict(zip(("bytes", "pieces", "tokens", "docs", "medium_pieces", "long_pieces"), (x.value for x in v)))

    def stat(self, name: str) -> int:
        """One named figure of the last encode call (tk_stat): "chunks", "small_calls", "mid_calls", "workspace_bytes", ..."""
        return int(self._L.tk_stat(self._h, name.encode())) if hasattr(self._L, "tk_stat") else 0
