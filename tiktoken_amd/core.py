"""`Encoding` -- the user-facing tokenizer object, call-for-call compatible with the reference's
`tiktoken.core.Encoding` (reference tiktoken/core.py:16-428), on top of the HIP `CoreBPE`.

Differences that matter for speed, none for results:
  * `encode_ordinary_batch` / `encode_batch` hand the WHOLE batch to the GPU in one call
    (`CoreBPE.encode_batch_packed`) instead of mapping documents over a thread pool
    (core.py:174-176, 202-206); `num_threads` is accepted for compatibility.
  * `encode_*_batch_packed` / `encode_to_numpy` return numpy arrays and skip the
    `list[list[int]]` materialisation, which costs more than the encode itself.
"""
from __future__ import annotations

import functools
from typing import TYPE_CHECKING, AbstractSet, Collection, Literal, NoReturn, Sequence

import numpy as np

from . import _tiktoken

if TYPE_CHECKING:
    import re

    import numpy.typing as npt

_SURROGATE_FIX = ("utf-16", "surrogatepass", "utf-16", "replace")


def _repair_surrogates(text: str) -> str:
    # same repair as core.py:79,135: join surrogate pairs, replace lone ones with U+FFFD
    return text.encode(_SURROGATE_FIX[0], _SURROGATE_FIX[1]).decode(_SURROGATE_FIX[2], _SURROGATE_FIX[3])


class Encoding:
    def __init__(self, name: str, *, pat_str: str, mergeable_ranks: dict[bytes, int], special_tokens: dict[str, int],
                 explicit_n_vocab: int | None = None):
        """See tiktoken_ext/openai_public.py for how the stock encodings call this.

        name: identifies the behaviour (encodings with different special tokens need different names).
        pat_str: the regex that splits text into pieces before BPE, compiled once (reference: src/lib.rs:623).  The r50k/gpt2, cl100k and
            o200k patterns -- in any of their spellings, with variations of the contraction list, the digit group length, the suffix set
            after punctuation and the white-space rules, e.g. Qwen2's or Llama-3's -- run on hand-written GPU scanners; any other
            pattern runs on the generic GPU regex engine (classes, \\p{..} General_Category values and scripts, groups, (?i: ), greedy / lazy /
            possessive quantifiers, atomic groups, look-ahead, \\b, look-behind of fixed length).  ValueError with the reason for what neither takes:
            look-behind of variable length, back-references, binary properties, patterns that can match the empty string.  There is no CPU regex fallback.
        mergeable_ranks: token bytes -> rank; ranks are merge priorities.
        special_tokens: special token string -> id.
        explicit_n_vocab: if given, checked against the number of tokens and the largest id.
        """
        self.name = name
        self._pat_str = pat_str
        self._ranks = mergeable_ranks
        self._special_tokens = special_tokens
        self._special_token_values = set(special_tokens.values())
        # The reference checks explicit_n_vocab BEFORE it builds the core (core.py:96-101): an inconsistent explicit_n_vocab is an AssertionError
        # whatever else is wrong with the vocabulary, and nothing has touched the GPU by then.  A lazily parsed file (vocab_io.RankTable) gives
        # count and largest rank from its packed arrays without a dict walk; they are the dict's unless the file lists a token twice (the
        # dict keeps the later rank, as the reference's load.py:159-171 does).  So: with explicit_n_vocab and arrays not yet known to be
        # distinct, the DICT decides, before the core is built (the stock encodings that pass explicit_n_vocab have 50 k tokens: 40 ms);
        # without explicit_n_vocab nothing is asserted and the arrays' figures are corrected after tk_create if it met such a token.
        def check(n_tokens: int, top: int) -> None:
            self.max_token_value = max(top, max(special_tokens.values(), default=0))
            if explicit_n_vocab:
                assert n_tokens + len(special_tokens) == explicit_n_vocab
                assert self.max_token_value == explicit_n_vocab - 1

        pending = getattr(mergeable_ranks, "_pending", None)
        n_seen = None
        if pending is not None and not explicit_n_vocab and not getattr(mergeable_ranks, "_distinct", False):
            ids = pending[2]
            n_seen = len(ids)
            check(n_seen, int(ids.max()) if len(ids) else 0)
        else:
            check(len(mergeable_ranks), mergeable_ranks.max_rank() if hasattr(mergeable_ranks, "max_rank") else max(mergeable_ranks.values()))
        self._core_bpe = _tiktoken.CoreBPE(mergeable_ranks, special_tokens, pat_str)
        if n_seen is not None and len(mergeable_ranks) != n_seen:  # (a token listed twice: collapsed by now; nothing to assert, the figure follows the dict)
            check(len(mergeable_ranks), mergeable_ranks.max_rank())

    @property
    def _mergeable_ranks(self) -> dict[bytes, int]:
        """(a RankTable is filled before it leaves: C code that reads a dict's storage directly would see it empty otherwise)"""
        r = self._ranks
        return r.materialize() if hasattr(r, "materialize") else r

    @_mergeable_ranks.setter
    def _mergeable_ranks(self, ranks: dict[bytes, int]) -> None:
        # (the reference's attribute is a plain one: subclasses and patches assign it.  As there, the core that was built is not rebuilt.)
        self._ranks = ranks

    def __repr__(self) -> str:
        return f"<Encoding {self.name!r}>"

    # ------------------------------------------------------------------ special-token policy
    def _special_policy(self, allowed_special, disallowed_special):
        """Resolve the "all" shorthands (core.py:116-119)."""
        if allowed_special == "all":
            allowed_special = self.special_tokens_set
        if disallowed_special == "all":
            disallowed_special = self.special_tokens_set - allowed_special
        return allowed_special, disallowed_special

    @staticmethod
    def _reject_disallowed(text: str, disallowed_special) -> None:
        if not disallowed_special:
            return
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        hit = _special_token_regex(disallowed_special).search(text)
        if hit:
            raise_disallowed_special_token(hit.group())

    # ------------------------------------------------------------------ encoding
    def encode_ordinary(self, text: str) -> list[int]:
        """Encode ignoring special tokens; same result as `encode(text, disallowed_special=())`."""
        try:
            return self._core_bpe.encode_ordinary(text)
        except UnicodeEncodeError:
            return self._core_bpe.encode_ordinary(_repair_surrogates(text))

    def encode(self, text: str, *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
               disallowed_special: Literal["all"] | Collection[str] = "all") -> list[int]:
        """Encode a string.  Text that spells a special token raises ValueError unless the token is in
        `allowed_special` (then it is emitted as the special id) or removed from `disallowed_special`
        (then it is encoded as ordinary text).  Both arguments accept "all"."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        self._reject_disallowed(text, disallowed_special)
        try:
            return self._core_bpe.encode(text, allowed_special)
        except UnicodeEncodeError:
            return self._core_bpe.encode(_repair_surrogates(text), allowed_special)

    def encode_to_numpy(self, text: str, *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                        disallowed_special: Literal["all"] | Collection[str] = "all") -> "npt.NDArray[np.uint32]":
        """Like `encode`, returning a uint32 array without building a Python list."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        self._reject_disallowed(text, disallowed_special)
        buffer = self._core_bpe.encode_to_tiktoken_buffer(text, allowed_special)
        return np.frombuffer(buffer, dtype=np.uint32)

    @staticmethod
    def _pack_repaired(texts: Sequence[str]):
        """(blob uint8, doc_off uint64[n+1], repaired): the texts as UTF-8, back to back, encoded text by text without a Python-level call
        per text.  (One encode of the joined string was measured and is no faster even for ASCII batches, and 2.4 times slower where the
        joined str has wide chars: profiles/r08_default_args.txt.)  Texts with surrogate code units, which the encode refuses, get the
        reference's repair (core.py:79,135); `repaired` says whether any text needed it."""
        if not isinstance(texts, (list, tuple)):
            texts = list(texts)
        repaired = False
        try:
            chunks = list(map(str.encode, texts))
        except UnicodeEncodeError:
            chunks = []
            for t in texts:
                try:
                    chunks.append(t.encode("utf-8"))
                except UnicodeEncodeError:
                    chunks.append(_repair_surrogates(t).encode("utf-8"))
                    repaired = True
        off = np.zeros(len(chunks) + 1, dtype=np.uint64)
        if chunks:
            np.cumsum(np.fromiter(map(len, chunks), dtype=np.uint64, count=len(chunks)), out=off[1:])
        return np.frombuffer(b"".join(chunks), dtype=np.uint8), off, repaired

    @staticmethod
    def _pack(texts: Sequence[str]):
        return Encoding._pack_repaired(texts)[:2]

    @staticmethod
    def _unpack(tokens: np.ndarray, tok_off: np.ndarray) -> list[list[int]]:
        # one tolist per document: the ints are created once, straight into their list (a flat list sliced afterwards costs twice)
        bounds = tok_off.tolist()
        return [tokens[a:b].tolist() for a, b in zip(bounds[:-1], bounds[1:])]

    def encode_ordinary_batch_packed(self, text: Sequence[str]):
        """(tokens uint32[T], tok_off uint64[n+1]) for a batch, ignoring special tokens."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_packed(blob, off, None)

    def encode_batch_packed(self, text: Sequence[str], *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                            disallowed_special: Literal["all"] | Collection[str] = "all"):
        """(tokens uint32[T], tok_off uint64[n+1]) for a batch; see `encode` for the special-token arguments.  The search for disallowed
        special tokens runs on the device, in the same call and on the text the encode has moved there anyway, when every member of
        `disallowed_special` is a special token of this encoding and no text needed surrogate repair; otherwise on the host, text by
        text, as the reference does it (any string may be disallowed there, and a surrogate pair spelled as two code units matches a
        str differently from its repaired bytes).  The ValueError is the host search's either way."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(text)
            return self._core_bpe.encode_batch_packed(blob, off, allowed_special)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_packed(blob, off, allowed_special)
        try:
            return self._core_bpe.encode_batch_packed(blob, off, allowed_special, disallowed_special=disallowed_special)
        except _tiktoken.DisallowedSpecialError as e:
            # today's search on that one document: the message -- which token is named where one is a prefix of another -- is the host's
            self._reject_disallowed(text[e.doc], disallowed_special)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    def encode_ordinary_batch_offsets_packed(self, text: Sequence[str]):
        """`encode_ordinary_batch_packed` plus where every token starts in its text: (tokens uint32[T], tok_off uint64[n+1],
        byte_start uint32[T], char_start uint32[T]) -- offsets into the text's UTF-8 and into the text (what `decode_with_offsets` of the
        same tokens gives), computed in the same GPU call."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_spans_packed(blob, off, None)

    def encode_batch_offsets_packed(self, text: Sequence[str], *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                                    disallowed_special: Literal["all"] | Collection[str] = "all"):
        """`encode_batch_packed` plus where every token starts in its text (see `encode_ordinary_batch_offsets_packed`); the special-token
        arguments as in `encode`.  A text that needed surrogate repair is measured in its repaired form."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(text)
            return self._core_bpe.encode_batch_spans_packed(blob, off, allowed_special)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_spans_packed(blob, off, allowed_special)
        try:
            return self._core_bpe.encode_batch_spans_packed(blob, off, allowed_special, disallowed_special=disallowed_special)
        except _tiktoken.DisallowedSpecialError as e:
            self._reject_disallowed(text[e.doc], disallowed_special)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    def encode_ordinary_batch_rows(self, text: Sequence[str], seq_len: int, *, bos: int | None = None, eos: int | None = None, pad: int | None = None,
                                   drop_last: bool = False, dtype=np.uint32) -> "_tiktoken.PackedRows":
        """A batch as fixed-length training rows, ignoring special tokens: every text is encoded, `bos` / `eos` (token ids) go before / after
        it, the results are concatenated and cut into rows of `seq_len` -- in one GPU call, only the rows come back.  Returns a
        `PackedRows`: `ids`, `doc` (the text a position belongs to) and `pos` (its position in its segment: they restart at every text and
        at every row) as [R, seq_len] arrays, `cu_seqlens` and `row_seg` for variable-length attention, `n_stream`, and -- with `drop_last`,
        which keeps whole rows only -- what is left over as `tail_ids`, `tail_doc`, `tail_pos`.  Without `drop_last` the last row is filled
        with `pad` (default: `eos`); ValueError if that is needed and neither is given.  dtype uint16: 16-bit ids, for vocabularies that fit."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_rows_packed(blob, off, None, seq_len=seq_len, bos=bos, eos=eos, pad=pad, drop_last=drop_last, dtype=dtype)

    def encode_batch_rows(self, text: Sequence[str], seq_len: int, *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                          disallowed_special: Literal["all"] | Collection[str] = "all", bos: int | None = None, eos: int | None = None,
                          pad: int | None = None, drop_last: bool = False, dtype=np.uint32) -> "_tiktoken.PackedRows":
        """`encode_ordinary_batch_rows` with the special-token arguments of `encode` -- the policy, and the error, of `encode_batch_packed`."""
        rows = dict(seq_len=seq_len, bos=bos, eos=eos, pad=pad, drop_last=drop_last, dtype=dtype)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(text)
            return self._core_bpe.encode_batch_rows_packed(blob, off, allowed_special, **rows)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_rows_packed(blob, off, allowed_special, **rows)
        try:
            return self._core_bpe.encode_batch_rows_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **rows)
        except _tiktoken.DisallowedSpecialError as e:
            self._reject_disallowed(text[e.doc], disallowed_special)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    # ------------------------------------------------------------------ JSON Lines
    @staticmethod
    def _from_device(tensor, ptr: int, n: int, typestr: str) -> np.ndarray:
        """n elements at a device pointer of `tensor`'s device, on the host (through torch, which the caller has: the tensor is its)"""
        import torch

        if not n:
            return np.zeros(0, dtype=np.dtype(typestr))

        class View:
            __cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}  # (torch takes no read-only view; the copy below is all that touches it)

        return torch.as_tensor(View(), device=tensor.device).cpu().numpy()

    def _jsonl_device(self, data, field, on_error):
        """(the JsonlDevice of a uint8 tensor on the encoding's GPU, taken by pointer)"""
        import torch

        if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous() or not data.is_cuda or data.device.index != self._core_bpe.device:
            raise ValueError("a tensor as data must be a contiguous one-dimensional uint8 tensor on the encoding's GPU")
        torch.cuda.current_stream(data.device).synchronize()  # (the library runs on a stream of its own)
        return self._core_bpe.jsonl_extract_device(data.data_ptr() if data.numel() else 0, data.numel(), field, on_error)

    def extract_jsonl(self, data, field: str = "text", on_error: str = "raise") -> "_tiktoken.JsonlText":
        """One field of every line of a JSON Lines buffer, unescaped on the GPU: what `[json.loads(l)[field] for l in f]` gives, packed as
        the batch entries take it.  `data`: bytes, bytearray, memoryview, an mmap or a uint8 numpy array (no copy before staging), or a uint8
        torch tensor on the encoding's GPU (by pointer).  `on_error`: "raise" (`JsonlError` with the first line that is neither a record nor
        blank), "skip" (such lines are left out; `line` says which line a document came from) or "empty" (an empty document for every
        non-blank line, so documents align with records).  The rule -- one field at depth 1, keys compared as raw bytes, the last duplicate
        wins, lone surrogate escapes become U+FFFD, no full JSON validation -- is stated in include/tiktoken_amd.h."""
        if hasattr(data, "data_ptr"):
            v = self._jsonl_device(data, field, on_error)
            return _tiktoken.JsonlText(self._from_device(data, v.text, v.n_text, "|u1"), self._from_device(data, v.doc_off, v.n_docs + 1, "<u8"),
                                       self._from_device(data, v.line, v.n_docs, "<u8"), self._from_device(data, v.status, v.n_lines, "|u1"), v.n_lines,
                                       self._from_device(data, v.line_off, v.n_lines + 1, "<u8"))
        return self._core_bpe.jsonl_extract_packed(data, field, on_error)

    def _encode_jsonl(self, data, field, on_error, allowed_special, disallowed_special) -> "_tiktoken.JsonlTokens":
        if not hasattr(data, "data_ptr"):
            return self._core_bpe.encode_jsonl_packed(data, field, on_error, allowed_special, disallowed_special=disallowed_special)
        v = self._jsonl_device(data, field, on_error)
        line, status = self._from_device(data, v.line, v.n_docs, "<u8"), self._from_device(data, v.status, v.n_lines, "|u1")
        doc_off = self._from_device(data, v.doc_off, v.n_docs + 1, "<u8")
        d_tok, n_tok, d_off = self._core_bpe.encode_batch_device(v.text, v.n_text, v.doc_off, doc_off, v.n_docs, allowed_special, disallowed_special=disallowed_special)
        return _tiktoken.JsonlTokens(self._from_device(data, d_tok, n_tok, "<u4"), self._from_device(data, d_off, v.n_docs + 1, "<u8"), line, status, v.n_lines)

    def encode_ordinary_jsonl_packed(self, data, field: str = "text", on_error: str = "raise") -> "_tiktoken.JsonlTokens":
        """A JSON Lines buffer encoded, ignoring special tokens: `extract_jsonl` and `encode_ordinary_batch_packed` in one GPU call -- the
        text never visits the host.  Returns a `JsonlTokens` (tokens, tok_off, line, status)."""
        return self._encode_jsonl(data, field, on_error, None, None)

    def encode_jsonl_packed(self, data, field: str = "text", on_error: str = "raise", *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                            disallowed_special: Literal["all"] | Collection[str] = "all") -> "_tiktoken.JsonlTokens":
        """`encode_ordinary_jsonl_packed` with the special-token arguments of `encode` -- the policy of `encode_batch_packed`.  A disallowed
        special token raises `DisallowedSpecialError` with the reference's message and, besides `doc`, the `line` it stands in."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            return self._encode_jsonl(data, field, on_error, allowed_special, None)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        if not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search, on the extracted text)
            ex = self.extract_jsonl(data, field, on_error)
            for d, t in enumerate(ex.texts()):
                self._reject_jsonl(t, disallowed_special, d, int(ex.line[d]))
            return self._encode_jsonl(data, field, on_error, allowed_special, None)
        try:
            return self._encode_jsonl(data, field, on_error, allowed_special, disallowed_special)
        except _tiktoken.DisallowedSpecialError as e:
            ex = self.extract_jsonl(data, field, on_error)  # (the message is the host search's, run on that one document's text)
            self._reject_jsonl(ex.text_bytes(e.doc).decode("utf-8"), disallowed_special, e.doc, int(ex.line[e.doc]), e)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    @staticmethod
    def _reject_jsonl(text: str, disallowed_special, doc: int, line: int, found=None) -> None:
        hit = _special_token_regex(disallowed_special).search(text)
        if hit:
            err = _tiktoken.DisallowedSpecialError(doc, found.pos if found is not None else len(text[:hit.start()].encode("utf-8")), hit.group())
            err.line = line
            raise err

    # ------------------------------------------------------------------ near-duplicate fingerprints
    def fingerprint_ordinary_batch(self, text: Sequence[str], *, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> "_tiktoken.Fingerprints":
        """Near-duplicate fingerprints of a batch, ignoring special tokens: every text is encoded and, while its ids are on the GPU,
        fingerprinted -- a MinHash signature of `n_perm` values over its shingles of `ngram` tokens, the LSH keys of the signature's `bands`,
        an exact hash and the shingle count; the ids never come back.  Returns a `Fingerprints`, whose `exact_groups`, `duplicate_groups`
        and `keep_mask` find the duplicates on the host.  The rule is stated in include/tiktoken_amd.h."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_fingerprint_packed(blob, off, None, ngram=ngram, n_perm=n_perm, bands=bands, seed=seed)

    def fingerprint_batch(self, text: Sequence[str], *, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0,
                          allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                          disallowed_special: Literal["all"] | Collection[str] = "all") -> "_tiktoken.Fingerprints":
        """`fingerprint_ordinary_batch` with the special-token arguments of `encode` -- the policy, and the error, of `encode_batch_packed`."""
        fp = dict(ngram=ngram, n_perm=n_perm, bands=bands, seed=seed)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if not disallowed_special:
            return self._core_bpe.encode_batch_fingerprint_packed(blob, off, allowed_special, **fp)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_fingerprint_packed(blob, off, allowed_special, **fp)
        return self._core_bpe.encode_batch_fingerprint_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **fp)

    def fingerprint_tokens_packed(self, tokens, tok_off, *, ngram: int = 5, n_perm: int = 128, bands: int = 16, seed: int = 0) -> "_tiktoken.Fingerprints":
        """The fingerprints of tokens that are packed already (`tokens` uint32[T], `tok_off` uint64[n + 1], e.g. `encode_batch_packed`'s)."""
        return self._core_bpe.fingerprint_packed(tokens, tok_off, ngram=ngram, n_perm=n_perm, bands=bands, seed=seed)

    def split_ordinary_batch_packed(self, text: Sequence[str], max_tokens: int, *, min_tokens: int | None = None, overlap: int = 0,
                                    separators=_tiktoken.DEFAULT_SEPARATORS, seg_tokens: int = 0) -> "_tiktoken.TextChunks":
        """A batch cut into chunks of at most `max_tokens` tokens, ignoring special tokens: every text is encoded and cut, each cut at the
        best separator among the token boundaries in [`min_tokens`, `max_tokens`] from the chunk's start -- `separators` lists levels,
        best first, of (tail, head) pairs: the text before the cut ends with tail, the text behind it starts with head (a bare str x means
        (x, "")) --, never inside a char; consecutive chunks share up to `overlap` tokens.  In one GPU call.  Returns a `TextChunks`.  The
        budget counts the text's own tokens: a chunk encoded on its own may differ by a few at its edges.  `min_tokens` defaults to
        max(overlap + 1, max_tokens // 2)."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_split_packed(blob, off, None, max_tokens=max_tokens, min_tokens=min_tokens, overlap=overlap, separators=separators,
                                                        seg_tokens=seg_tokens)

    def _split_packed(self, text: Sequence[str], max_tokens: int, *, min_tokens: int | None = None, overlap: int = 0, separators=_tiktoken.DEFAULT_SEPARATORS,
                      allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                      disallowed_special: Literal["all"] | Collection[str] = "all", seg_tokens: int = 0):
        """(the TextChunks of `split_batch_packed`, whether a text with surrogates was repaired before it was encoded)"""
        rows = dict(max_tokens=max_tokens, min_tokens=min_tokens, overlap=overlap, separators=separators, seg_tokens=seg_tokens)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if not disallowed_special:
            return self._core_bpe.encode_batch_split_packed(blob, off, allowed_special, **rows), repaired
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_split_packed(blob, off, allowed_special, **rows), repaired
        try:
            return self._core_bpe.encode_batch_split_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **rows), repaired
        except _tiktoken.DisallowedSpecialError as e:
            self._reject_disallowed(text[e.doc], disallowed_special)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    def split_batch_packed(self, text: Sequence[str], max_tokens: int, *, min_tokens: int | None = None, overlap: int = 0, separators=_tiktoken.DEFAULT_SEPARATORS,
                           allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                           disallowed_special: Literal["all"] | Collection[str] = "all", seg_tokens: int = 0) -> "_tiktoken.TextChunks":
        """`split_ordinary_batch_packed` with the special-token arguments of `encode` -- the policy, and the error, of `encode_batch_packed`."""
        return self._split_packed(text, max_tokens, min_tokens=min_tokens, overlap=overlap, separators=separators, allowed_special=allowed_special,
                                  disallowed_special=disallowed_special, seg_tokens=seg_tokens)[0]

    def split_batch(self, text: Sequence[str], max_tokens: int, **kwargs) -> "list[list[str]]":
        """The chunks of every text as strings (`split_batch_packed`, each str sliced by the chunks' char offsets)."""
        if not isinstance(text, (list, tuple)):
            text = list(text)
        ch, repaired = self._split_packed(text, max_tokens, **kwargs)
        first, a, b = ch.doc_chunk.tolist(), ch.char_begin.tolist(), ch.char_end.tolist()
        if not repaired:
            return [[t[a[i]:b[i]] for i in range(first[d], first[d + 1])] for d, t in enumerate(text)]
        # (a text with surrogates was repaired before it was encoded: the offsets speak of the repaired text, which the chunks hold)
        return [[ch.text(i) for i in range(first[d], first[d + 1])] for d in range(len(text))]

    def encode_ordinary_batch_padded(self, text: Sequence[str], max_length: int, *, stride: int = 0, windows: bool = False, keep: str = "head",
                                     padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None,
                                     pad: int | None = None, dtype=np.uint32) -> "_tiktoken.PaddedBatch":
        """A batch as padded model inputs, ignoring special tokens: every text is encoded and becomes one row `[bos] tokens [eos]` of at most
        `max_length` elements -- its head, or with keep="tail" its tail --, or with `windows` as many rows as it needs, consecutive ones
        sharing `stride` tokens; in one GPU call, only the padded arrays come back.  Returns a `PaddedBatch`: `input_ids` and
        `attention_mask` as [R, W] arrays, `lengths`, `row_doc` (the text of a row), `row_tok` (the row's first token inside its text) and
        `doc_row` (the first row of every text).  W is `max_length`, or with `pad_to_multiple_of` the longest row rounded up to a multiple of
        it.  Rows are filled with `pad` (default: `eos`) on the right or, padding_side="left", on the left; ValueError if that is needed
        and neither is given.  dtype uint16: 16-bit ids, for vocabularies that fit."""
        blob, off = self._pack(text)
        return self._core_bpe.encode_batch_padded_packed(blob, off, None, max_length=max_length, stride=stride, windows=windows, keep=keep, padding_side=padding_side,
                                                         pad_to_multiple_of=pad_to_multiple_of, bos=bos, eos=eos, pad=pad, dtype=dtype)

    def encode_batch_padded(self, text: Sequence[str], max_length: int, *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                            disallowed_special: Literal["all"] | Collection[str] = "all", stride: int = 0, windows: bool = False, keep: str = "head",
                            padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None,
                            pad: int | None = None, dtype=np.uint32) -> "_tiktoken.PaddedBatch":
        """`encode_ordinary_batch_padded` with the special-token arguments of `encode` -- the policy, and the error, of `encode_batch_packed`."""
        rows = dict(max_length=max_length, stride=stride, windows=windows, keep=keep, padding_side=padding_side, pad_to_multiple_of=pad_to_multiple_of, bos=bos, eos=eos,
                    pad=pad, dtype=dtype)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(text)
            return self._core_bpe.encode_batch_padded_packed(blob, off, allowed_special, **rows)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(text)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for t in text:
                self._reject_disallowed(t, disallowed_special)
            return self._core_bpe.encode_batch_padded_packed(blob, off, allowed_special, **rows)
        try:
            return self._core_bpe.encode_batch_padded_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **rows)
        except _tiktoken.DisallowedSpecialError as e:
            self._reject_disallowed(text[e.doc], disallowed_special)
            raise RuntimeError(f"internal error: the device reported the disallowed special token {e.token!r} in document {e.doc} at byte "
                               f"{e.pos}, the host search finds none there") from e

    def encode_ordinary_batch_samples(self, parts: Sequence[str], sample_off, part_role, roles: "Sequence[_tiktoken.Role]", max_length: int, *, keep: str = "head",
                                      padding_side: str = "right", pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None,
                                      pad: int = 0, ignore_index: int = -100) -> "_tiktoken.SampleBatch":
        """A batch as supervised fine-tuning samples, ignoring special tokens in the text: every part is encoded as ordinary text, sample s
        is the parts `sample_off[s] .. sample_off[s + 1]`, and its row is `[bos]`, then for each part `roles[part_role[p]].before`, the
        part's tokens, `.after`, then `[eos]` -- cut to `max_length` at its head or, keep="tail", its tail, padded with `pad` on the right
        or the left; in one GPU call, only the sample arrays come back.  Returns a `SampleBatch`: `input_ids`, `attention_mask` and `labels`
        as [R, W] arrays -- labels hold the id where the element is trained (the tokens and the `after` ids of a part whose role trains, the
        eos behind such a part) and `ignore_index` elsewhere, not shifted --, `length`, `full_length` (before the cut) and `n_trained` (what
        of the trained elements survived it).  W is `max_length`, or with `pad_to_multiple_of` the longest row rounded up to a multiple of
        it.  A role's ids are token ids, never text: encode a template's few header and footer strings once."""
        blob, off = self._pack(parts)
        return self._core_bpe.encode_batch_samples_packed(blob, off, None, part_role=part_role, sample_off=sample_off, roles=roles, max_length=max_length, keep=keep,
                                                          padding_side=padding_side, pad_to_multiple_of=pad_to_multiple_of, bos=bos, eos=eos, pad=pad,
                                                          ignore_index=ignore_index)

    def encode_batch_samples(self, parts: Sequence[str], sample_off, part_role, roles: "Sequence[_tiktoken.Role]", max_length: int, *,
                             allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                             disallowed_special: Literal["all"] | Collection[str] = "all", keep: str = "head", padding_side: str = "right",
                             pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None, pad: int = 0,
                             ignore_index: int = -100) -> "_tiktoken.SampleBatch":
        """`encode_ordinary_batch_samples` with the special-token arguments of `encode`; the policy holds for all parts.  A part that holds a
        disallowed special token raises `DisallowedSpecialError` -- a ValueError with the reference's message -- whose `doc` is the part's
        index, `pos` the byte offset inside it."""
        rows = dict(part_role=part_role, sample_off=sample_off, roles=roles, max_length=max_length, keep=keep, padding_side=padding_side,
                    pad_to_multiple_of=pad_to_multiple_of, bos=bos, eos=eos, pad=pad, ignore_index=ignore_index)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(parts)
            return self._core_bpe.encode_batch_samples_packed(blob, off, allowed_special, **rows)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(parts)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for i, t in enumerate(parts):
                if match := _special_token_regex(disallowed_special).search(t):
                    raise _tiktoken.DisallowedSpecialError(i, len(t[: match.start()].encode("utf-8", "surrogatepass")), match.group())
            return self._core_bpe.encode_batch_samples_packed(blob, off, allowed_special, **rows)
        return self._core_bpe.encode_batch_samples_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **rows)

    def encode_chat_batch(self, conversations: "Sequence[Sequence[tuple[str, str]]]", template: "dict[str, _tiktoken.Role]", max_length: int, *,
                          allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                          disallowed_special: Literal["all"] | Collection[str] = "all", keep: str = "head", padding_side: str = "right",
                          pad_to_multiple_of: int | None = None, bos: int | None = None, eos: int | None = None, pad: int = 0,
                          ignore_index: int = -100) -> "_tiktoken.SampleBatch":
        """Conversations as supervised samples: `conversations` is a sequence of sequences of `(role_name, text)`, `template` maps a role
        name to its `Role` (header ids, footer ids, whether the turn is trained).  Flattens to the arrays of `encode_batch_samples` and
        calls it: message text is encoded as text, so with the default `disallowed_special="all"` content that spells a special token
        raises `DisallowedSpecialError` with `doc` = the index of the message among all messages; the template's special tokens go in as
        ids.  An unknown role name is a ValueError."""
        names = list(template)
        index = {name: i for i, name in enumerate(names)}
        parts, part_role, sample_off = [], [], [0]
        for conv in conversations:
            for role, text in conv:
                if role not in index:
                    raise ValueError(f"unknown role {role!r}: the template has {names}")
                parts.append(text)
                part_role.append(index[role])
            sample_off.append(len(parts))
        return self.encode_batch_samples(parts, sample_off, part_role, [template[n] for n in names], max_length, allowed_special=allowed_special,
                                         disallowed_special=disallowed_special, keep=keep, padding_side=padding_side, pad_to_multiple_of=pad_to_multiple_of, bos=bos,
                                         eos=eos, pad=pad, ignore_index=ignore_index)

    def encode_ordinary_batch_sample_rows(self, parts: Sequence[str], sample_off, part_role, roles: "Sequence[_tiktoken.Role]", max_length: int, *, keep: str = "head",
                                          skip_long: bool = False, ignore_first: bool = False, bos: int | None = None, eos: int | None = None, pad: int = 0,
                                          ignore_index: int = -100) -> "_tiktoken.SampleRows":
        """The samples of `encode_ordinary_batch_samples`, several whole ones packed into every row of `max_length`: next-fit in the order
        given (shuffle or sort the samples first: that order is the packing policy), an over-long sample cut at its head or tail -- or,
        `skip_long`, left out --, in one GPU call.  Returns a `SampleRows`: `input_ids`, `labels` (not shifted), `segment_ids` and
        `position_ids` (restarting at every sample) as [R, max_length] arrays, `cu_seqlens` / `row_seg` for variable-length attention, and
        per sample `length`, `full_length`, `n_trained`, `sample_row`, `sample_col`.  `ignore_first`: the label of every sample's first
        element is `ignore_index`, so that after the model's shift no sample is predicted from the one before it."""
        blob, off = self._pack(parts)
        return self._core_bpe.encode_batch_sample_rows_packed(blob, off, None, part_role=part_role, sample_off=sample_off, roles=roles, max_length=max_length, keep=keep,
                                                              skip_long=skip_long, ignore_first=ignore_first, bos=bos, eos=eos, pad=pad, ignore_index=ignore_index)

    def encode_batch_sample_rows(self, parts: Sequence[str], sample_off, part_role, roles: "Sequence[_tiktoken.Role]", max_length: int, *,
                                 allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                                 disallowed_special: Literal["all"] | Collection[str] = "all", keep: str = "head", skip_long: bool = False,
                                 ignore_first: bool = False, bos: int | None = None, eos: int | None = None, pad: int = 0,
                                 ignore_index: int = -100) -> "_tiktoken.SampleRows":
        """`encode_ordinary_batch_sample_rows` with the special-token arguments of `encode`; the policy holds for all parts.  A part that
        holds a disallowed special token raises `DisallowedSpecialError` whose `doc` is the part's index, `pos` the byte offset inside it."""
        rows = dict(part_role=part_role, sample_off=sample_off, roles=roles, max_length=max_length, keep=keep, skip_long=skip_long, ignore_first=ignore_first, bos=bos,
                    eos=eos, pad=pad, ignore_index=ignore_index)
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        if not disallowed_special:
            blob, off = self._pack(parts)
            return self._core_bpe.encode_batch_sample_rows_packed(blob, off, allowed_special, **rows)
        if not isinstance(disallowed_special, frozenset):
            disallowed_special = frozenset(disallowed_special)
        blob, off, repaired = self._pack_repaired(parts)
        if repaired or not all(t in self._special_tokens for t in disallowed_special):  # (as encode_batch_packed: the host's search)
            for i, t in enumerate(parts):
                if match := _special_token_regex(disallowed_special).search(t):
                    raise _tiktoken.DisallowedSpecialError(i, len(t[: match.start()].encode("utf-8", "surrogatepass")), match.group())
            return self._core_bpe.encode_batch_sample_rows_packed(blob, off, allowed_special, **rows)
        return self._core_bpe.encode_batch_sample_rows_packed(blob, off, allowed_special, disallowed_special=disallowed_special, **rows)

    def encode_chat_batch_rows(self, conversations: "Sequence[Sequence[tuple[str, str]]]", template: "dict[str, _tiktoken.Role]", max_length: int, *,
                               allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                               disallowed_special: Literal["all"] | Collection[str] = "all", keep: str = "head", skip_long: bool = False,
                               ignore_first: bool = False, bos: int | None = None, eos: int | None = None, pad: int = 0,
                               ignore_index: int = -100) -> "_tiktoken.SampleRows":
        """`encode_chat_batch` with the conversations packed several to a row (`encode_batch_sample_rows`): the same flattening, the same
        `DisallowedSpecialError` with `doc` = the index of the message among all messages, the same ValueError for an unknown role name."""
        names = list(template)
        index = {name: i for i, name in enumerate(names)}
        parts, part_role, sample_off = [], [], [0]
        for conv in conversations:
            for role, text in conv:
                if role not in index:
                    raise ValueError(f"unknown role {role!r}: the template has {names}")
                parts.append(text)
                part_role.append(index[role])
            sample_off.append(len(parts))
        return self.encode_batch_sample_rows(parts, sample_off, part_role, [template[n] for n in names], max_length, allowed_special=allowed_special,
                                             disallowed_special=disallowed_special, keep=keep, skip_long=skip_long, ignore_first=ignore_first, bos=bos, eos=eos, pad=pad,
                                             ignore_index=ignore_index)

    def encode_ordinary_batch(self, text: list[str], *, num_threads: int = 8) -> list[list[int]]:
        """Encode a list of strings, ignoring special tokens (one GPU batch; `num_threads` is kept for
        signature compatibility)."""
        return self._unpack(*self.encode_ordinary_batch_packed(text))

    def encode_batch(self, text: list[str], *, num_threads: int = 8,
                     allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                     disallowed_special: Literal["all"] | Collection[str] = "all") -> list[list[int]]:
        """Encode a list of strings; see `encode` for the special-token arguments."""
        return self._unpack(*self.encode_batch_packed(text, allowed_special=allowed_special,
                                                      disallowed_special=disallowed_special))

    def encode_with_unstable(self, text: str, *, allowed_special: Literal["all"] | AbstractSet[str] = set(),  # noqa: B006
                             disallowed_special: Literal["all"] | Collection[str] = "all") -> tuple[list[int], list[list[int]]]:
        """Stable prefix tokens plus the possible token sequences that could complete the unstable tail."""
        allowed_special, disallowed_special = self._special_policy(allowed_special, disallowed_special)
        self._reject_disallowed(text, disallowed_special)
        return self._core_bpe.encode_with_unstable(text, allowed_special)

    def encode_single_token(self, text_or_bytes: str | bytes) -> int:
        """Id of the token whose bytes are exactly the argument (special tokens included); KeyError otherwise."""
        if isinstance(text_or_bytes, str):
            text_or_bytes = text_or_bytes.encode("utf-8")
        return self._core_bpe.encode_single_token(text_or_bytes)

    # ------------------------------------------------------------------ decoding
    def decode_bytes(self, tokens: Sequence[int]) -> bytes:
        return self._core_bpe.decode_bytes(tokens)

    def decode(self, tokens: Sequence[int], errors: str = "replace") -> str:
        """Decode to str.  Lossy by default: token boundaries need not be UTF-8 boundaries, so invalid
        sequences are replaced unless `errors="strict"`."""
        return self._core_bpe.decode_bytes(tokens).decode("utf-8", errors=errors)

    def decode_single_token_bytes(self, token: int) -> bytes:
        return self._core_bpe.decode_single_token_bytes(token)

    def _decode_tokens_bytes_host(self, tokens: Sequence[int]) -> list[bytes]:
        return [self.decode_single_token_bytes(t) for t in tokens]

    def _spans_on_device(self, tokens: Sequence[int]) -> bool:
        """Whether the single forms below go through the batch call.  Not when the ids are too sparse for the device table or the core has
        several devices (the batch call refuses both), and not when an id has no token or does not fit uint32: the per-token path then
        raises what it always raised (KeyError with the id).  Any other error of the batch call is the caller's to see."""
        core = self._core_bpe
        if getattr(core, "_group", None) is not None or self.max_token_value >= 1 << 26:
            return False
        try:
            arr = np.asarray(tokens, dtype=np.int64)
        except (OverflowError, TypeError, ValueError):
            return False
        return arr.ndim == 1 and (not len(arr) or (0 <= int(arr.min()) and int(arr.max()) <= 0xFFFFFFFF))

    def decode_tokens_bytes(self, tokens: Sequence[int]) -> list[bytes]:
        if self._spans_on_device(tokens):
            try:
                return self.decode_tokens_bytes_batch([tokens])[0]
            except KeyError:  # (an id without a token)
                pass
        return self._decode_tokens_bytes_host(tokens)

    def decode_with_offsets(self, tokens: Sequence[int]) -> tuple[str, list[int]]:
        """Text plus, per token, the index of the character in which the token starts (a token that begins
        with a continuation byte is attributed to the character it continues).  Strict UTF-8."""
        if self._spans_on_device(tokens):
            try:
                return self.decode_with_offsets_batch([tokens])[0]
            except KeyError:  # (an id without a token)
                pass
        pieces = self._decode_tokens_bytes_host(tokens)
        offsets: list[int] = []
        n_chars = 0
        for piece in pieces:
            starts_mid_char = 0x80 <= piece[0] < 0xC0
            offsets.append(max(0, n_chars - (1 if starts_mid_char else 0)))
            n_chars += sum(1 for b in piece if not 0x80 <= b < 0xC0)
        return b"".join(pieces).decode("utf-8", errors="strict"), offsets

    # ---- the same for whole batches: one GPU call (tk_decode_batch_spans), no per-token work on the host
    @staticmethod
    def _flatten(batch: Sequence[Sequence[int]]):
        """(ids uint32[T], tok_off uint64[n + 1]) of a batch of token lists"""
        lens = np.fromiter((len(t) for t in batch), dtype=np.uint64, count=len(batch))
        tok_off = np.zeros(len(batch) + 1, dtype=np.uint64)
        np.cumsum(lens, out=tok_off[1:])
        return np.fromiter((t for doc in batch for t in doc), dtype=np.uint32, count=int(tok_off[-1])), tok_off

    def decode_with_offsets_packed(self, tokens: "npt.NDArray[np.uint32]", tok_off: "npt.NDArray[np.uint64]"):
        """`decode_with_offsets` for a packed batch (ids of all documents back to back, tok_off uint64[n + 1]), as arrays:
        (data uint8 -- the documents' UTF-8 back to back --, byte_off uint64[n + 1], char_off uint64[n + 1], byte_start uint32[T],
        char_start uint32[T]).  char_start[i] is the reference's offset of token i in its own document's text, byte_start[i] the same
        in bytes: the token's bytes are data[byte_off[d] + byte_start[i] : ...].  Like the reference, raises UnicodeDecodeError (Python's
        own, for the first such document) when a document is not valid UTF-8, and KeyError for an id without a token."""
        data, byte_off, char_off, byte_start, char_start, bad = self._core_bpe.decode_batch_spans_packed(tokens, tok_off)
        if bad is not None:
            bytes(data[int(byte_off[bad]):int(byte_off[bad + 1])]).decode("utf-8", "strict")
            raise RuntimeError(f"internal error: the device reported document {bad} as invalid UTF-8, Python decodes it")
        return data, byte_off, char_off, byte_start, char_start

    def decode_with_offsets_batch(self, batch: Sequence[Sequence[int]]) -> list[tuple[str, list[int]]]:
        """`decode_with_offsets` of every document of a batch, in one GPU call."""
        flat, tok_off = self._flatten(batch)
        data, byte_off, _, _, char_start = self.decode_with_offsets_packed(flat, tok_off)
        view = memoryview(data)
        bb, tb = byte_off.tolist(), tok_off.tolist()
        return [(str(view[bb[d]:bb[d + 1]], "utf-8", "strict") if bb[d + 1] > bb[d] else "", char_start[tb[d]:tb[d + 1]].tolist()) for d in range(len(batch))]

    def decode_tokens_bytes_batch(self, batch: Sequence[Sequence[int]]) -> list[list[bytes]]:
        """`decode_tokens_bytes` of every document of a batch: the packed bytes of one GPU call, cut at the tokens' byte offsets."""
        flat, tok_off = self._flatten(batch)
        data, byte_off, _, byte_start, _, _ = self._core_bpe.decode_batch_spans_packed(flat, tok_off, validate=False)
        starts = byte_start.astype(np.uint64) + np.repeat(byte_off[:-1], np.diff(tok_off).astype(np.int64))  # in the batch: ascending, so a token ends where the next starts
        cuts = starts.tolist() + [int(byte_off[-1])]
        raw = data.tobytes()
        pieces = [raw[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        tb = tok_off.tolist()
        return [pieces[tb[d]:tb[d + 1]] for d in range(len(batch))]

    def decode_batch(self, batch: Sequence[Sequence[int]], *, errors: str = "replace", num_threads: int = 8) -> list[str]:
        """Decode a batch; the whole batch goes to the GPU in one call (`num_threads` is accepted for compatibility)."""
        data, bounds = self._decode_packed(batch)
        if data is None:
            return [self.decode_bytes(t).decode("utf-8", errors=errors) for t in batch]
        view = memoryview(data)  # (str() decodes a slice of the result buffer in place: no bytes object per document in between)
        return [str(view[a:b], "utf-8", errors) if b > a else "" for a, b in zip(bounds[:-1], bounds[1:])]

    def _decode_packed(self, batch: Sequence[Sequence[int]]):
        """(uint8 array of all bytes back to back -- a view of the library's result buffer --, list of n + 1 byte offsets), or (None, None)
        when the ids are too sparse for the device table."""
        flat, tok_off = self._flatten(batch)
        try:
            data, byte_off = self._core_bpe.decode_batch_packed(flat, tok_off, as_array=True)
        except ValueError:  # (ids too sparse for the device table)
            return None, None
        return data, byte_off.tolist()

    def decode_bytes_batch(self, batch: Sequence[Sequence[int]], *, num_threads: int = 8) -> list[bytes]:
        """One GPU call for the whole batch (tk_decode_batch) instead of one pool task per document."""
        data, bounds = self._decode_packed(batch)
        if data is None:
            return [self.decode_bytes(t) for t in batch]
        view = memoryview(data)
        return [bytes(view[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]

    # ---- id matrices, as a generation loop hands them back: rows cut at their first stop id, pad and special ids dropped, on the device
    def _row_ids(self, ids, what: str) -> list[int]:
        """stop / skip as ids: a special token may be named by its string"""
        if isinstance(ids, (str, int)):
            ids = (ids,)
        out = []
        for t in ids:
            if isinstance(t, str):
                if t not in self._special_tokens:
                    raise ValueError(f"{what}: {t!r} is no special token of this encoding")
                t = self._special_tokens[t]
            out.append(int(t))
        return out

    def decode_rows_packed(self, ids, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False,
                           keep_stop: bool = False) -> "_tiktoken.DecodedRows":
        """Decode the rows of an id matrix [R, W] in one GPU call (tk_decode_rows / tk_decode_rows_device), as arrays -- see
        `_tiktoken.DecodedRows`.  Row r is read from column begin[r] (default 0) up to its first id in `stop`, or to end[r] (default W)
        when it has none; ids in `skip`, and with `skip_special` every special token, are dropped.  `stop` and `skip` take up to 16 ids or
        special-token strings each; with `keep_stop` the stop id belongs to its row.  An id outside the live range or in `skip` may be
        anything (a pad id outside the vocabulary); a kept id without a token raises KeyError with its row and column.
        `ids`: a 2-D numpy array of uint32, int32 or int64 whose column stride is one element (any row stride: `out[:, prompt_len:]` is not
        copied), or a torch tensor of int32 / int64 on this encoding's GPU, which goes in by pointer."""
        kw = dict(stop=self._row_ids(stop, "stop"), skip=self._row_ids(skip, "skip"), skip_special=skip_special, keep_stop=keep_stop)
        if hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda"):
            return self._decode_rows_tensor(ids, begin, end, kw)
        return self._core_bpe.decode_rows_packed(ids, begin=begin, end=end, **kw)

    def _decode_rows_tensor(self, ids, begin, end, kw) -> "_tiktoken.DecodedRows":
        r, host = self._rows_tensor_call(ids, begin, end, lambda **a: self._core_bpe.decode_rows_device(**a, **kw))
        n_rows = ids.shape[0]
        return _tiktoken.DecodedRows(host(r.data, r.n_bytes, "|u1", np.uint8), host(r.byte_off, n_rows + 1, "<i8", np.uint64), host(r.tokens, r.n_tokens, "<i4", np.uint32),
                                     host(r.tok_off, n_rows + 1, "<i8", np.uint64), host(r.n_kept, n_rows, "<i4", np.uint32), host(r.stop_col, n_rows, "<i4", np.uint32))

    def decode_rows_bytes(self, ids, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False) -> list[bytes]:
        """The bytes of every row of an id matrix; the arguments as in `decode_rows_packed`."""
        rows = self.decode_rows_packed(ids, begin=begin, end=end, stop=stop, skip=skip, skip_special=skip_special, keep_stop=keep_stop)
        view, bounds = memoryview(rows.data), rows.byte_off.tolist()
        return [bytes(view[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]

    def decode_rows(self, ids, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                    errors: str = "replace") -> list[str]:
        """The text of every row of an id matrix: `[enc.decode(trimmed_row) for row in ids]` without the host loop that trims.  The
        arguments as in `decode_rows_packed`; `errors` as in `decode`, applied per row on the host.  The defaults skip nothing and stop
        nowhere."""
        rows = self.decode_rows_packed(ids, begin=begin, end=end, stop=stop, skip=skip, skip_special=skip_special, keep_stop=keep_stop)
        view, bounds = memoryview(rows.data), rows.byte_off.tolist()
        return [str(view[a:b], "utf-8", errors) if b > a else "" for a, b in zip(bounds[:-1], bounds[1:])]

    # ---- packed text: errors="replace" / "ignore" applied on the device, the result well-formed UTF-8 in one array
    def decode_batch_text_packed(self, tokens: "npt.NDArray[np.uint32]", tok_off: "npt.NDArray[np.uint64]", errors: str = "replace") -> "_tiktoken.RepairedText":
        """`decode_batch(..., errors=errors)` for a packed batch (ids of all documents back to back, tok_off uint64[n + 1]) as ONE array of
        well-formed UTF-8: (data, text_off, char_off, repl_off) -- document d is data[text_off[d] : text_off[d + 1]], the bytes of
        `decode(doc, errors=errors).encode()`; char_off counts its chars and repl_off the ill-formed units that were replaced by U+FFFD
        (errors="replace") or dropped ("ignore"), both as running totals of n + 1 entries.  One GPU call (tk_decode_batch_text), no host
        loop over the documents: the array goes into an Arrow string column or a JSONL writer as it is.  KeyError for an id without a
        token, as `decode_batch`.  errors="strict" and other handlers are not run on the device: ValueError naming the entries that take them."""
        return self._core_bpe.decode_batch_text_packed(tokens, tok_off, errors)[0]

    def decode_rows_text_packed(self, ids, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                                errors: str = "replace") -> "_tiktoken.DecodedRowsText":
        """`decode_rows_packed` with text for bytes (tk_decode_rows_text / tk_decode_rows_text_device): the rows are trimmed and decoded as
        there, then repaired on the device -- a char that the stop id, begin, end or a skipped id cuts becomes U+FFFD (errors="replace")
        or nothing ("ignore"), as in `decode_rows(..., errors=errors)`, and data is well-formed UTF-8.  See `_tiktoken.DecodedRowsText`;
        `ids` and the other arguments as in `decode_rows_packed`."""
        _tiktoken.repair_mode(errors)  # (refused before anything runs)
        kw = dict(stop=self._row_ids(stop, "stop"), skip=self._row_ids(skip, "skip"), skip_special=skip_special, keep_stop=keep_stop)
        if not (hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda")):
            return self._core_bpe.decode_rows_text_packed(ids, begin=begin, end=end, errors=errors, **kw)
        r, host = self._rows_tensor_call(ids, begin, end, lambda **a: self._core_bpe.decode_rows_text_device(errors=errors, **a, **kw))
        n_rows = ids.shape[0]
        return _tiktoken.DecodedRowsText(host(r.data, r.n_bytes, "|u1", np.uint8), host(r.byte_off, n_rows + 1, "<i8", np.uint64), host(r.tokens, r.n_tokens, "<i4", np.uint32),
                                         host(r.tok_off, n_rows + 1, "<i8", np.uint64), host(r.n_kept, n_rows, "<i4", np.uint32), host(r.stop_col, n_rows, "<i4", np.uint32),
                                         host(r.char_off, n_rows + 1, "<i8", np.uint64), host(r.repl_off, n_rows + 1, "<i8", np.uint64))

    # ---- rows cut at a stop STRING as well (until=, stop=, stop_strings=): searched in the decoded bytes, on the device
    def decode_rows_until_packed(self, ids, stop_text, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                                 keep_stop_text: bool = False, errors: "str | None" = "replace") -> "_tiktoken.StoppedRows":
        """`decode_rows_text_packed` whose rows also end at the first place where one of `stop_text` lies (tk_decode_rows_until /
        tk_decode_rows_until_device): up to 16 stop strings, each a str (its UTF-8 is searched) or bytes, of 1 .. 64 bytes.  A stop
        string is text, not a token -- it may be one id, several, or the tail of one -- so it is searched in the row's decoded bytes: the
        earliest match wins, and at one place the string listed first.  The row rule of `decode_rows_packed` runs first (begin, end,
        stop ids, skipped ids: what lies behind a stop id is never searched), then the search, the cut, and the repair of the cut text
        (errors="replace" / "ignore"; None: the cut bytes as they are).  keep_stop_text: the stop string stays at the row's end.
        See `_tiktoken.StoppedRows`: hit[r] names the string that ended row r, n_tok[r] the tokens the kept text covers."""
        _tiktoken.until_mode(errors)  # (refused before anything runs)
        kw = dict(stop=self._row_ids(stop, "stop"), skip=self._row_ids(skip, "skip"), skip_special=skip_special, keep_stop=keep_stop, keep_stop_text=keep_stop_text,
                  errors=errors)
        if not (hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda")):
            return self._core_bpe.decode_rows_until_packed(ids, stop_text, begin=begin, end=end, **kw)
        r, host = self._rows_tensor_call(ids, begin, end, lambda **a: self._core_bpe.decode_rows_until_device(stop_text=stop_text, **a, **kw))
        n_rows = ids.shape[0]
        text = errors is not None
        return _tiktoken.StoppedRows(host(r.data, r.n_bytes, "|u1", np.uint8), host(r.byte_off, n_rows + 1, "<i8", np.uint64),
                                     host(r.char_off, n_rows + 1, "<i8", np.uint64) if text else None, host(r.repl_off, n_rows + 1, "<i8", np.uint64) if text else None,
                                     host(r.tokens, r.n_tokens, "<i4", np.uint32), host(r.tok_off, n_rows + 1, "<i8", np.uint64), host(r.n_kept, n_rows, "<i4", np.uint32),
                                     host(r.stop_col, n_rows, "<i4", np.uint32), host(r.hit, n_rows, "<i4", np.uint32), host(r.n_tok, n_rows, "<i4", np.uint32))

    def decode_rows_until(self, ids, stop_text, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                          keep_stop_text: bool = False, errors: str = "replace") -> list[str]:
        """The text of every row of an id matrix up to its first stop string; the arguments as in `decode_rows_until_packed`
        (errors: "replace" or "ignore")."""
        _tiktoken.repair_mode(errors)  # (text: no bytes mode here)
        rows = self.decode_rows_until_packed(ids, stop_text, begin=begin, end=end, stop=stop, skip=skip, skip_special=skip_special, keep_stop=keep_stop,
                                             keep_stop_text=keep_stop_text, errors=errors)
        view, bounds = memoryview(rows.data), rows.byte_off.tolist()
        return [str(view[a:b], "utf-8") if b > a else "" for a, b in zip(bounds[:-1], bounds[1:])]

    def decode_rows_until_bytes(self, ids, stop_text, *, begin=None, end=None, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                                keep_stop_text: bool = False) -> list[bytes]:
        """The bytes of every row of an id matrix up to its first stop string, not repaired; the arguments as in `decode_rows_until_packed`."""
        rows = self.decode_rows_until_packed(ids, stop_text, begin=begin, end=end, stop=stop, skip=skip, skip_special=skip_special, keep_stop=keep_stop,
                                             keep_stop_text=keep_stop_text, errors=None)
        view, bounds = memoryview(rows.data), rows.byte_off.tolist()
        return [bytes(view[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]

    # ---- the same for rows that arrive a few ids per step: a generation loop's incremental detokenizer, its state on the device
    def decode_stream(self, n_rows: int, stop_text=(), *, w_max: int = 1, stop=(), skip=(), skip_special: bool = False, keep_stop: bool = False,
                      keep_stop_text: bool = False, errors: "str | None" = "replace") -> "DecodeStream":
        """A decode stream of `n_rows` row slots whose state lives on the GPU (tk_stream_create): `step(ids)` takes the [n_rows, W] ids a
        generation step made, W <= w_max <= 64, and returns per row the text that became final -- never half a UTF-8 char, never the
        first half of a stop string that may still complete --; a row ends at a stop id or the moment a stop string completes.  Everything
        a row emits, concatenated, is what `decode_rows_until` returns for all the live columns it was fed.  The arguments as in
        `decode_rows_until_packed`; errors=None: bytes, not repaired.  See `DecodeStream`."""
        _tiktoken.until_mode(errors)  # (refused before anything runs)
        native = self._core_bpe.stream_create(n_rows, stop_text, w_max=w_max, stop=self._row_ids(stop, "stop"), skip=self._row_ids(skip, "skip"), skip_special=skip_special,
                                              keep_stop=keep_stop, keep_stop_text=keep_stop_text, errors=errors)
        return DecodeStream(self, native, errors)

    def _rows_tensor_call(self, ids, begin, end, call):
        """An id tensor on this encoding's GPU through a device entry: (the entry's result, host(ptr, n, typestr, dtype): one of its buffers
        copied to the host)."""
        import torch

        core = self._core_bpe
        if not ids.is_cuda or ids.device.index != core.device:
            raise ValueError(f"the id tensor lives on {ids.device}: this encoding runs on GPU {core.device} (numpy arrays go through the host entry)")
        dtype = {torch.int32: np.int32, torch.int64: np.int64}.get(ids.dtype)
        if ids.dim() != 2 or dtype is None:
            raise ValueError("an id tensor has two dimensions and holds int32 or int64")
        n_rows, width = ids.shape
        if n_rows and width > 1 and ids.stride(1) != 1:
            raise ValueError("the column stride of an id matrix must be one element")
        ld = ids.stride(0) if n_rows > 1 and width else width

        def bounds(x, name):
            if x is None:
                return None
            if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.int32 and x.is_contiguous() and x.shape == (n_rows,)):
                x = torch.from_numpy(core._row_bounds(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, n_rows, name).view(np.int32)).to(ids.device)
            return x

        d_begin, d_end = bounds(begin, "begin"), bounds(end, "end")
        torch.cuda.current_stream(ids.device).synchronize()  # (the library runs on a stream of its own: the ids must be there)
        r = call(d_ids=ids.data_ptr() if n_rows and width else 0, n_rows=n_rows, width=width, ld=ld, dtype=dtype, d_begin=d_begin.data_ptr() if d_begin is not None else 0,
                 d_end=d_end.data_ptr() if d_end is not None else 0)

        def host(ptr, n, typestr, np_dtype):  # a buffer of the library, copied to the host
            if not n:
                return np.zeros(0, np_dtype)
            return torch.as_tensor(_DeviceArray(ptr, n, typestr), device=ids.device).cpu().numpy().view(np_dtype)

        return r, host

    def token_byte_values(self) -> list[bytes]:
        return self._core_bpe.token_byte_values()

    @property
    def eot_token(self) -> int:
        return self._special_tokens["<|endoftext|>"]

    @functools.cached_property
    def special_tokens_set(self) -> set[str]:
        return set(self._special_tokens.keys())

    def is_special_token(self, token: int) -> bool:
        assert isinstance(token, int)
        return token in self._special_token_values

    @property
    def n_vocab(self) -> int:
        """Kept for backwards compatibility; `max_token_value + 1`."""
        return self.max_token_value + 1

    # ------------------------------------------------------------------ private
    def _encode_single_piece(self, text_or_bytes: str | bytes) -> list[int]:
        """BPE of the argument's bytes with no regex split and no special tokens."""
        if isinstance(text_or_bytes, str):
            text_or_bytes = text_or_bytes.encode("utf-8")
        return self._core_bpe.encode_single_piece(text_or_bytes)

    def _encode_only_native_bpe(self, text: str) -> list[int]:
        """Regex split in Python (`regex` module), BPE per piece on the device."""
        import regex

        out: list[int] = []
        for piece in regex.findall(regex.compile(self._pat_str), text):
            out.extend(self._core_bpe.encode_single_piece(piece.encode("utf-8")))
        return out

    def _encode_bytes(self, text: bytes) -> list[int]:
        return self._core_bpe._encode_bytes(text)

    def __getstate__(self) -> object:
        from . import plugins

        if plugins._CATALOGUE.registered(self):
            return self.name  # registered encodings pickle by name
        return {"name": self.name, "pat_str": self._pat_str, "mergeable_ranks": self._mergeable_ranks,
                "special_tokens": self._special_tokens}

    def __setstate__(self, value: object) -> None:
        from . import plugins

        if isinstance(value, str):
            self.__dict__ = plugins.get_encoding(value).__dict__
            return
        self.__init__(**value)


class DecodeStream:
    """`Encoding.decode_stream`: row slots on the GPU, fed a few ids per step.  A context manager; `close()` releases the device buffers.
    A call that is refused (KeyError for a kept id without a token, ValueError for W > w_max, begin > end, end > W) changes nothing."""

    def __init__(self, enc: Encoding, native: "_tiktoken.NativeStream", errors: "str | None"):
        self._enc, self._native, self._errors = enc, native, errors
        self.n_rows, self.w_max = native.n_rows, native.w_max

    def close(self) -> None:
        self._native.close()

    def __enter__(self) -> "DecodeStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def step_packed(self, ids, begin=None, end=None) -> "_tiktoken.StreamPacked":
        """One step, as arrays (see `_tiktoken.StreamPacked`).  `ids`: what `decode_rows` takes -- a numpy array of uint32, int32 or
        int64 of any row stride, or a torch tensor of int32 / int64 on this encoding's GPU, which goes in by pointer (`out[:, t:t + W]`
        is not copied) --, [n_rows, W] or 1-D as [n_rows, 1]; begin / end: per row, as there."""
        core, native = self._enc._core_bpe, self._native
        if hasattr(ids, "data_ptr") and hasattr(ids, "is_cuda"):
            if ids.dim() == 1:
                ids = ids.unsqueeze(1)
            if ids.dim() == 2 and ids.shape[0] != self.n_rows:
                raise ValueError(f"the stream has {self.n_rows} rows: the ids have {ids.shape[0]}")
            r, _ = self._enc._rows_tensor_call(ids, begin, end, lambda d_ids, n_rows, width, ld, dtype, d_begin, d_end: native.step_device(d_ids, width, ld, dtype, d_begin, d_end))
            return r
        ids = np.asarray(ids)
        if ids.ndim == 1:
            ids = ids.reshape(len(ids), 1)
        if ids.ndim == 2 and ids.shape[0] != self.n_rows:
            raise ValueError(f"the stream has {self.n_rows} rows: the ids have {ids.shape[0]}")
        ids, _, width, ld, begin, end, _ = core._host_matrix(ids, begin, end, (), (), False, False)
        return native.step_host(ids, width, ld, begin, end)

    def _texts(self, p: "_tiktoken.StreamPacked") -> "_tiktoken.StreamStep":
        view, bounds = memoryview(p.text), p.text_off.tolist()
        if self._errors is None:
            text = [bytes(view[a:b]) for a, b in zip(bounds[:-1], bounds[1:])]
        else:
            text = [str(view[a:b], "utf-8") if b > a else "" for a, b in zip(bounds[:-1], bounds[1:])]
        return _tiktoken.StreamStep(text, p.state != 0, p.state, p.hit)

    def step(self, ids, begin=None, end=None) -> "_tiktoken.StreamStep":
        """One step: `StreamStep(text, finished, state, hit)`, text[r] what row r emitted (str; bytes under errors=None)."""
        return self._texts(self.step_packed(ids, begin, end))

    def flush_packed(self, rows=None) -> "_tiktoken.StreamPacked":
        return self._native.flush(rows)

    def flush(self, rows=None) -> "_tiktoken.StreamStep":
        """The live rows among `rows` (None: all) emit what they held back -- an unfinished char becomes U+FFFD under errors="replace"
        -- and are flushed (state 3)."""
        return self._texts(self._native.flush(rows))

    def reset(self, rows=None) -> None:
        """`rows` (None: all) are live again, with nothing held back and zero totals: a slot taken by the next request."""
        self._native.reset(rows)

    @property
    def state(self) -> np.ndarray:
        return self._native.rows()["state"]

    @property
    def hit(self) -> np.ndarray:
        return self._native.rows()["hit"]

    @property
    def n_kept(self) -> np.ndarray:
        return self._native.rows()["n_kept"]

    @property
    def n_text(self) -> np.ndarray:
        return self._native.rows()["n_text"]

    @property
    def n_chars(self) -> np.ndarray:
        return self._native.rows()["n_chars"]


class _DeviceArray:
    """A device buffer of the library seen through __cuda_array_interface__ (torch.as_tensor reads it in place)."""

    def __init__(self, ptr: int, n: int, typestr: str):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


@functools.lru_cache(maxsize=128)
def _special_token_regex(tokens: frozenset[str]) -> "re.Pattern[str]":
    try:
        import regex as re
    except ImportError:
        import re
    return re.compile("(" + "|".join(re.escape(t) for t in tokens) + ")")


def raise_disallowed_special_token(token: str) -> NoReturn:
    raise ValueError(_tiktoken.disallowed_special_message(token))
