/* C ABI of libtiktoken_amd.so -- the MI355X-native replacement for the reference's Rust
 * `_tiktoken` extension on the BPE encode path.
 *
 * Each entry point names the reference interface it replaces (paths into openai/tiktoken v0.14.0).
 * The reference-side binding a maintainer would add is shown in INTEGRATION.md; the Python shim
 * that ships here is tiktoken_amd/_tiktoken.py (ctypes).  All pointers are plain host pointers
 * unless the name says `_device`; no torch/HIP types appear in any signature.
 *
 * Status codes: every function returning int returns one of TK_OK ... TK_DISALLOWED_SPECIAL; on failure
 * tk_last_error() holds a message (thread-local).  The Python shim maps them to the reference's
 * exception types: TK_VALUE_ERROR -> ValueError (src/py.rs:21-22,46), TK_KEY_ERROR -> KeyError
 * (src/py.rs:142,160,171), TK_RUNTIME_ERROR -> RuntimeError (HIP failures; no reference analogue),
 * TK_DISALLOWED_SPECIAL -> DisallowedSpecialError, a ValueError (tiktoken/core.py:441-449; the _checked calls only).
 *
 * There is no CPU implementation behind these calls: without a usable HIP device tk_create fails
 * with TK_RUNTIME_ERROR.
 */
#ifndef TIKTOKEN_AMD_H
#define TIKTOKEN_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { TK_OK = 0, TK_VALUE_ERROR = 1, TK_KEY_ERROR = 2, TK_RUNTIME_ERROR = 3, TK_UNSUPPORTED = 4, TK_DISALLOWED_SPECIAL = 5,
       TK_JSONL_ERROR = 6 /* the JSON Lines entries under TK_JSONL_RAISE: a line that is neither a record nor blank (JsonlError, a ValueError) */ };

typedef struct tk_core tk_core;

const char* tk_last_error(void);
int tk_device_count(void);

/* CoreBPE.__new__(encoder, special_tokens_encoder, pattern)            src/py.rs:15-23, src/lib.rs:618-663
 * ranks: n_ranks byte strings ranks_blob[ranks_off[i]..ranks_off[i+1]) with ids ranks_ids[i];
 * specials likewise (UTF-8).  pat_str: the split regex, compiled once here (Regex::new, src/lib.rs:623).  The three families of
 * tiktoken_ext/openai_public.py:12-14,89,104-114 (stock strings, their other spellings, variations of the contraction list, digit
 * group, suffix set and white-space rules) run on hand-written scanners; any other pattern in the syntax fancy-regex shares with
 * Python `regex` -- classes (with && and --, POSIX classes), \p{General_Category}, \p{Script}, the binary properties of the UCD, alternation,
 * groups, (?i: ), greedy / lazy / possessive quantifiers, atomic groups, look-ahead, look-behind of fixed length, \b, ^ $ -- is compiled
 * for the generic GPU engine (tk_regex.cpp): into a DFA (leftmost-first; tk_regex_dfa.inc) that every lane walks out of LDS, and -- for
 * what a table cannot express: look-around of several chars, atomic groups and possessive repeats around groups -- into a backtracking
 * program that the GPU interprets ($TIKTOKEN_AMD_RX_MATCHER=program forces the program for every pattern).  Refused with TK_UNSUPPORTED and the reason: look-behind of variable length,
 * back-references (fancy-regex has them; they stay refused here), a pattern that can match the empty string.  Text a pattern does not
 * match yields no tokens, as the reference's find_iter skips it (src/lib.rs:365,405).
 * Text must be valid UTF-8 (the reference's boundary is &str); other bytes never crash but their split is unspecified: a caller that
 * cannot vouch for its bytes checks them with tk_validate_utf8 first.
 * Duplicate ranks -> TK_VALUE_ERROR (the reference panics, src/lib.rs:636-641).  device = HIP device ordinal.
 * Threads: a core may be used from several threads (src/lib.rs:232-238).  Calls on one document of at most 128 KiB without special tokens take
 * no lock (seventy-two slots per core; callers that arrive together share one launch); every other call on a core is serialised by the core's mutex.
 * What a call costs: one kernel launch for a document of up to 128 KiB without special tokens (~22 us for 11 bytes, ~70 us for 4 KiB, ~110 us
 * for 64 KiB: cut at certain piece starts into segments, a workgroup each), the general pipeline's dozen launches otherwise (~0.15 ms and up):
 * the path is for batches. */
int tk_create(const uint8_t* ranks_blob, const uint64_t* ranks_off, const uint32_t* ranks_ids, uint64_t n_ranks,
              const uint8_t* spec_blob, const uint64_t* spec_off, const uint32_t* spec_ids, uint64_t n_spec,
              const char* pat_str, int device, tk_core** out);
void tk_destroy(tk_core* core);

/* How a pat_str would run: 0 r50k/gpt2, 1 cl100k, 2 o200k -- a family the library has hand-written scanners for (the stock patterns,
 * their other spellings, and variations of the contraction list, digit group, suffix set and white-space rules: tk_pattern.cpp);
 * 3 -- the generic engine (tk_regex.cpp); -1 -- not supported (tk_create would say why).  Reference: the regex compiled once per
 * Encoding, src/lib.rs:623. */
int tk_pattern_id(const char* pat_str);

/* Encoding.encode_ordinary_batch / encode_batch                        tiktoken/core.py:164-206
 * == ThreadPool map of CoreBPE.encode_ordinary / encode                src/py.rs:29-49, src/lib.rs:360-442
 * Documents are packed back to back in `utf8`; doc_off has n_docs+1 entries (doc_off[0] == 0).
 * use_special = 0: encode_ordinary semantics.  use_special = 1: special tokens whose id is in
 * allowed_ids[0..n_allowed) are emitted as their id, all other text is ordinary text.
 * On success *tokens_out (library-owned, release with tk_free) holds the token ids of all
 * documents back to back and tok_off_out[0..n_docs] (caller-owned array) their boundaries. */
int tk_encode_batch(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                    const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                    uint64_t* tok_off_out);

/* Encoding.encode / encode_batch with disallowed_special                 tiktoken/core.py:116-124, raise_disallowed_special_token :441-449
 * The reference searches every text for the disallowed special tokens, on the host, before it encodes anything.  The _checked calls do
 * that search in the same call, on the text they have moved to the device anyway (one more read of it per chunk: tk_k_spec_find).
 * disallowed_ids[0..n_disallowed): ids of registered special tokens (any other id: TK_VALUE_ERROR).  The search looks at the raw text,
 * whatever allowed_ids makes of it, and an id in both lists is disallowed (the reference searches first; for "all" its Python layer
 * has subtracted the allowed set already, core.py:100-106).
 * No occurrence: exactly what the unchecked call does and returns.  n_disallowed == 0 IS the unchecked call (no extra launch).
 * Otherwise TK_DISALLOWED_SPECIAL: *hit describes the first occurrence -- the lowest document, in it the lowest byte offset, there the
 * longest disallowed token that fits its document (a token that would run across a document boundary is no occurrence) --, no
 * tokens are handed out (*tokens_out is not written), and tk_last_error() names document, offset and id.  The core stays usable. */
typedef struct {
    uint64_t doc, pos; /* pos: byte offset inside document `doc` */
    uint32_t id, len;  /* the token's id and its length in bytes */
} tk_special_hit;
int tk_encode_batch_checked(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                            const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                            uint32_t** tokens_out, uint64_t* n_tokens_out, uint64_t* tok_off_out, tk_special_hit* hit);

/* Same, with inputs already resident in HBM and results left in HBM (bench / torch interop).
 * d_utf8 must be readable for 64 bytes past n_bytes.  d_doc_off: uint64[n_docs+1] on the device,
 * h_doc_off: the same offsets on the host (needed only when n_bytes exceeds the per-launch chunk,
 * may be NULL otherwise).  stream: a hipStream_t (NULL = the library's own stream).  The returned
 * device pointers are owned by the core and stay valid until its next encode call. */
int tk_encode_batch_device(tk_core* core, const void* d_utf8, uint64_t n_bytes, const void* d_doc_off,
                           const uint64_t* h_doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                           uint64_t n_allowed, void* stream, const uint32_t** d_tokens_out, uint64_t* n_tokens_out,
                           const uint64_t** d_tok_off_out);
/* ... checked (see tk_encode_batch_checked); on a hit the few bytes at it, and d_doc_off where h_doc_off is NULL, are copied to the host */
int tk_encode_batch_device_checked(tk_core* core, const void* d_utf8, uint64_t n_bytes, const void* d_doc_off,
                                   const uint64_t* h_doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                   uint64_t n_allowed, void* stream, const uint32_t** d_tokens_out, uint64_t* n_tokens_out,
                                   const uint64_t** d_tok_off_out, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                                   tk_special_hit* hit);

/* Test / debug entry with no reference counterpart: the piece boundaries the GPU pre-tokeniser
 * finds, i.e. what `regex.find_iter` yields at src/lib.rs:365 and :405.  *starts_out receives
 * n_pieces+1 ascending uint32 offsets (last = total bytes); release with tk_free.  Single chunk, less
 * than 2 GiB (bit 31 of an offset marks a char a generic pat_str does not match). */
int tk_pretokenize_batch(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                         const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** starts_out, uint64_t* n_out);

/* CoreBPE.encode_ordinary(text) / CoreBPE.encode(text, allowed_special)  src/py.rs:29-49
 * (also backs encode_to_tiktoken_buffer, src/py.rs:51-70: the result is a plain uint32 buffer). */
int tk_encode_ordinary(tk_core* core, const uint8_t* utf8, uint64_t len, uint32_t** tokens_out, uint64_t* n_tokens_out);
int tk_encode(tk_core* core, const uint8_t* utf8, uint64_t len, const uint32_t* allowed_ids, uint64_t n_allowed,
              uint32_t** tokens_out, uint64_t* n_tokens_out);

/* CoreBPE.encode_single_piece(piece): BPE of raw bytes without regex splitting   src/py.rs:145-150 */
int tk_encode_single_piece(tk_core* core, const uint8_t* piece, uint64_t len, uint32_t** tokens_out,
                           uint64_t* n_tokens_out);
/* byte_pair_encode(piece, &self.encoder) proper: the merge WITHOUT the whole-piece shortcut (single bytes map to their
 * rank).  What `_encode_unstable_native` calls on re-split candidates      src/lib.rs:198-211, call sites :555,:585-590 */
int tk_byte_pair_encode(tk_core* core, const uint8_t* piece, uint64_t len, uint32_t** tokens_out, uint64_t* n_tokens_out);
/* CoreBPE.encode_single_token(piece)   TK_KEY_ERROR if absent                     src/py.rs:133-143 */
int tk_encode_single_token(tk_core* core, const uint8_t* piece, uint64_t len, uint32_t* token_out);
/* CoreBPE.decode_bytes(tokens)         TK_KEY_ERROR "Invalid token for decoding: N"  src/py.rs:156-162, lib.rs:345-358 */
int tk_decode_bytes(tk_core* core, const uint32_t* tokens, uint64_t n, uint8_t** bytes_out, uint64_t* len_out);
/* The same for a packed batch, on the device: tokens of all documents back to back, tok_off[n_docs + 1] token offsets.  One call
 * replaces the per-document thread pool of Encoding.decode_bytes_batch / decode_batch (tiktoken/core.py:331-350).  *bytes_out:
 * library-owned (tk_free), byte_off_out (may be null): n_docs + 1 byte offsets.  TK_KEY_ERROR as tk_decode_bytes; TK_UNSUPPORTED
 * when the ids are too sparse for a direct table (>= 2^26). */
int tk_decode_batch(tk_core* core, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, uint8_t** bytes_out,
                    uint64_t* n_bytes_out, uint64_t* byte_off_out);
/* The same with everything resident in HBM: ids (uint32) and token offsets (uint64[n_docs + 1], may be null) on the core's device in,
 * *d_bytes_out / *d_byte_off_out (library-owned device buffers, valid until the core's next decode call; *d_byte_off_out null without
 * d_tok_off) and *n_bytes_out out.  `stream`: a hipStream_t or null (the core's).  The counterpart of tk_encode_batch_device for a
 * consumer that keeps text on the device; no reference counterpart (the reference returns owned Vec<u8>s, src/lib.rs:345-358). */
int tk_decode_batch_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, void* stream,
                           const uint8_t** d_bytes_out, uint64_t* n_bytes_out, const uint64_t** d_byte_off_out);
/* Encoding.decode_with_offsets / decode_tokens_bytes for whole batches     tiktoken/core.py:312-335, :303-310
 * Token spans: for every token of a packed batch where it starts in ITS document -- byte_start (the sum of the lengths of the document's
 * tokens before it) and char_start (core.py:327-331: the chars, i.e. bytes outside 0x80..0xBF, before it, less one when the token's first
 * byte is a continuation byte, never below 0) --, both uint32; and per document byte_off / char_off (uint64[n_docs + 1]): the bytes / chars
 * of the documents before it.  A token's bytes are bytes[byte_off[d] + byte_start[i] ..), the next token's start or byte_off[d + 1] their end.
 * TK_KEY_ERROR as tk_decode_bytes; TK_UNSUPPORTED when the ids are too sparse for a direct table (as tk_decode_batch); TK_VALUE_ERROR for a
 * document that decodes to 4 GiB or more.  One device per call: a group has no spans entry.
 *
 * Device pointers in (ids uint32, d_tok_off uint64[n_docs + 1], required), device pointers out: buffers of the core, valid until its next
 * decode or spans call.  d_doc_off (may be null): the byte offsets of the documents' TEXT when the ids come from an encode call
 * (tk_encode_batch_device's d_doc_off) -- then every document's tokens must add up to its length; they do not only where a pat_str of the
 * generic engine leaves chars unmatched (find_iter skips them, src/lib.rs:365,405): TK_UNSUPPORTED naming the first such document. */
int tk_token_spans_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const void* d_doc_off,
                          void* stream, const uint32_t** d_byte_start_out, const uint32_t** d_char_start_out, const uint64_t** d_byte_off_out,
                          const uint64_t** d_char_off_out);
/* Host buffers in and out (core.py:312-335 over a batch).  bytes_out null: spans only.  *bytes_out, *byte_start_out, *char_start_out:
 * library-owned (tk_free); byte_off_out / char_off_out (may be null): caller's arrays of n_docs + 1.  validate != 0: the decoded documents are
 * checked on the device as bytes.decode("utf-8", "strict") checks them (core.py:334) and *invalid_doc_out is the first document, in order,
 * that is not well-formed (all ones: none; a sequence cut by a document boundary is ill-formed in both documents).  The call still returns
 * TK_OK and every output: the caller decodes that one document to raise the reference's UnicodeDecodeError.  Batches of 32 Mi ids and more run
 * in overlapped ranges of 16 Mi ids, as tk_decode_batch's do. */
int tk_decode_batch_spans(tk_core* core, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, int validate, uint8_t** bytes_out,
                          uint64_t* n_bytes_out, uint32_t** byte_start_out, uint32_t** char_start_out, uint64_t* byte_off_out,
                          uint64_t* char_off_out, uint64_t* invalid_doc_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked -- plus the spans of the tokens it returns (core.py:312-335 applied to
 * core.py:164-206's result without a decode call in between): the span pass runs over the ids while they are on the device, against
 * doc_off.  *byte_start_out / *char_start_out: library-owned (tk_free).  TK_UNSUPPORTED for text a generic pat_str leaves unmatched (above). */
int tk_encode_batch_spans(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                          const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                          uint32_t** tokens_out, uint64_t* n_tokens_out, uint64_t* tok_off_out, uint32_t** byte_start_out,
                          uint32_t** char_start_out, tk_special_hit* hit);
/* Training rows: a packed batch -> fixed-length rows with document ids, positions and segment boundaries.  Replaces nothing in the
 * reference: it is the host loop of the reference's users, the data-preparation script that appends a separator to every encoded document,
 * concatenates the lists and reshapes -- here one call on ids that are on the device anyway.
 * The stream holds, for every document d in order, [bos_id] tokens[tok_off[d] .. tok_off[d + 1]) [eos_id] (TK_ROWS_NO_TOKEN: none; k = how
 * many of the two there are, so document d starts at tok_off[d] + d * k and the stream has S = n_tokens + n_docs * k elements; with k == 0
 * an empty document owns no position).  It is cut into rows of seq_len (L): R = ceil(S / L) rows, the last one filled with pad_id, M = R * L
 * positions -- or, with TK_ROWS_DROP_LAST, R = floor(S / L) whole rows followed by the n_tail = S - R * L positions left over (M = S), so that
 * a caller can carry them into its next batch.  Per position j < M:
 *   ids[j]   the stream element (pad_id from S on); uint16 with TK_ROWS_IDS16, else uint32
 *   doc[j]   the document whose stream range holds j (TK_ROWS_NO_TOKEN on padding)
 *   pos[j]   j - max(start of that document (S on padding), start of the row): positions restart at every document and at every row
 * cu_seqlens[0 .. n_segs]: the positions with pos == 0, ascending, then M (the boundaries variable-length attention takes); row_seg[0 .. R]:
 * the number of segment starts below r * L, so cu_seqlens[row_seg[a] .. row_seg[b]] - a * L are the boundaries of the rows a .. b alone.
 * TK_VALUE_ERROR: seq_len == 0; max(S, R * L) >= 2^32 or n_docs >= 2^32 - 1 (the outputs are 32-bit); tok_off that does not ascend from 0
 * to n_tokens (checked on the device before anything is indexed with it; the message names the first offending document); TK_ROWS_IDS16
 * unless every id of the vocabulary, the special tokens, bos_id, eos_id and pad_id fit 16 bits.  One device per call: a group has no rows entry. */
#define TK_ROWS_NO_TOKEN 0xFFFFFFFFu
#define TK_ROWS_DROP_LAST 1u
#define TK_ROWS_IDS16 2u
typedef struct {
    uint32_t seq_len, bos_id, eos_id, pad_id, flags;
} tk_rows_spec;
/* Device pointers in (ids uint32, d_tok_off uint64[n_docs + 1]: e.g. the results of tk_encode_batch_device), device pointers out: buffers
 * of the core, valid until its next rows call and apart from the encode, decode and span buffers (packing an encode call's result leaves it
 * intact).  *d_ids_out .. *d_pos_out: M elements each (*n_rows_out rows of seq_len, then *n_tail_out more); *d_cu_seqlens_out: *n_segs_out + 1;
 * *d_row_seg_out: *n_rows_out + 1; *n_stream_out: S.  `stream`: a hipStream_t or null (the core's); the call returns when the rows are there. */
int tk_pack_rows_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_rows_spec* spec,
                        void* stream, const void** d_ids_out, const uint32_t** d_doc_out, const uint32_t** d_pos_out,
                        const uint32_t** d_cu_seqlens_out, const uint32_t** d_row_seg_out, uint64_t* n_rows_out, uint64_t* n_segs_out,
                        uint64_t* n_stream_out, uint64_t* n_tail_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked -- with its result packed into rows while the ids are on the device:
 * host text in, host rows out, and only the row arrays cross the link (the ids themselves are not handed out).  *ids_out .. *row_seg_out:
 * library-owned (tk_free), sized as above.  On TK_DISALLOWED_SPECIAL nothing is handed out. */
int tk_encode_batch_rows(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                         const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                         const tk_rows_spec* spec, void** ids_out, uint32_t** doc_out, uint32_t** pos_out, uint32_t** cu_seqlens_out,
                         uint32_t** row_seg_out, uint64_t* n_rows_out, uint64_t* n_segs_out, uint64_t* n_stream_out, uint64_t* n_tail_out,
                         tk_special_hit* hit);
/* Padded model inputs: a packed batch -> one row per document, truncated to a maximum length and padded, with an attention mask -- or a
 * long document continued in further rows that overlap by `stride` tokens.  Replaces nothing in the reference: it is the host loop of the
 * reference's users (`enc.encode(t)[:n]` plus list padding, a token-window text splitter; elsewhere `tokenizer(batch, padding=...,
 * truncation=..., max_length=..., stride=..., return_overflowing_tokens=True)`) -- here one call on ids that are on the device anyway.
 * The rule.  Input: tokens uint32[T], tok_off uint64[n_docs + 1].  bos_id / eos_id: TK_ROWS_NO_TOKEN for none; k = how many of the two
 * exist, has_bos = 0 or 1, c = max_len - k the body capacity of a row.  Document d has n_d = tok_off[d + 1] - tok_off[d] body tokens.
 *  Rows of a document.  Every document owns at least one row, an empty one too ([bos][eos], or nothing but padding).  Without
 *   TK_PAD_WINDOWS there is one row: its body is tokens [0, min(n_d, c)) of the document, with TK_PAD_KEEP_TAIL [max(n_d - c, 0), n_d).
 *   With TK_PAD_WINDOWS let step = c - stride: n_d <= c gives one row, otherwise w_d = 1 + ceil((n_d - c) / step) rows, row j holding body
 *   tokens [j * step, min(j * step + c, n_d)) -- the last row may be short, consecutive rows share `stride` tokens, every row gets its
 *   own bos / eos.
 *  Row contents.  Row r belongs to document row_doc[r] and starts at body token row_tok[r], an index inside the document;
 *   len[r] = k + (body tokens it holds).  Its elements are [bos] body [eos]: with TK_PAD_LEFT in columns [W - len, W), otherwise in
 *   [0, len); everywhere else ids = pad_id.  mask (uint8) is 1 on elements and 0 on padding.
 *  Row order.  Rows are in document order; doc_row[d] (uint32[n_docs + 1]) is the first row of document d, doc_row[n_docs] = R.
 *  Width.  width_multiple == 0: W = max_len.  Otherwise W = min(max_len, ceil(longest / width_multiple) * width_multiple) with
 *   longest = max len[r], 0 when there is no row.  W = 0 is a legal result (only empty documents, no bos / eos, width_multiple = 1):
 *   ids and mask are [R, 0] then, and len, row_doc, row_tok, doc_row are still filled.
 *  TK_VALUE_ERROR: max_len == 0 or c == 0; stride >= c; stride != 0 without TK_PAD_WINDOWS; TK_PAD_KEEP_TAIL together with
 *   TK_PAD_WINDOWS; n_docs >= 2^32 - 1, T >= 2^32, R >= 2^32 or R * W >= 2^32 (found after the count, before any output is written);
 *   TK_PAD_IDS16 unless every id of the vocabulary, the special tokens, bos_id, eos_id and pad_id fit 16 bits (as TK_ROWS_IDS16); a tok_off
 *   that does not ascend from 0 to n_tokens (checked on the device before anything is indexed with it; the message names the first
 *   offending document).  No kernel reads or writes out of bounds, whatever tok_off holds.  One device per call: a group has no padded entry. */
#define TK_PAD_WINDOWS 1u   /* a document that does not fit goes on in further rows */
#define TK_PAD_KEEP_TAIL 2u /* without WINDOWS: keep a long document's last tokens, not its first */
#define TK_PAD_LEFT 4u      /* padding in front of the row's elements, not behind */
#define TK_PAD_IDS16 8u     /* ids as uint16 (same condition as TK_ROWS_IDS16) */
typedef struct {
    uint32_t max_len, stride, width_multiple, bos_id, eos_id, pad_id, flags;
} tk_pad_spec;
/* Device pointers in (ids uint32, d_tok_off uint64[n_docs + 1]: e.g. the results of tk_encode_batch_device), device pointers out: buffers
 * of the core, valid until its next padded call that succeeds (a refused call writes into none of them) and apart from the encode, decode,
 * span and rows buffers (padding an encode call's result leaves it intact).  *d_ids_out (uint32 or uint16) and *d_mask_out: *n_rows_out x *width_out; *d_len_out, *d_row_doc_out, *d_row_tok_out:
 * *n_rows_out; *d_doc_row_out: n_docs + 1.  `stream`: a hipStream_t or null (the core's); the call returns when the rows are there. */
int tk_pad_batch_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_pad_spec* spec,
                        void* stream, const void** d_ids_out, const uint8_t** d_mask_out, const uint32_t** d_len_out, const uint32_t** d_row_doc_out,
                        const uint32_t** d_row_tok_out, const uint32_t** d_doc_row_out, uint64_t* n_rows_out, uint64_t* width_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked -- with its result padded while the ids are on the device: host text
 * in, and only the padded arrays cross the link (the ids themselves are not handed out).  *ids_out .. *doc_row_out: library-owned
 * (tk_free), sized as above.  On TK_DISALLOWED_SPECIAL nothing is handed out. */
int tk_encode_batch_padded(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                           const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                           const tk_pad_spec* spec, void** ids_out, uint8_t** mask_out, uint32_t** len_out, uint32_t** row_doc_out,
                           uint32_t** row_tok_out, uint32_t** doc_row_out, uint64_t* n_rows_out, uint64_t* width_out, tk_special_hit* hit);
/* Text chunks: every document of a batch cut into pieces of at most max_tokens tokens, each cut placed at the best separator that fits
 * (a blank line before a line break before a sentence end before a space) and never inside a char.  Replaces nothing in the reference: it
 * is the host loop of the reference's users, the text splitter of a retrieval or embedding ingest that counts tokens with the encoder
 * (elsewhere `RecursiveCharacterTextSplitter.from_tiktoken_encoder`) -- here one call on ids and text that are on the device anyway.
 * The rule.  Input: tokens uint32[T], tok_off uint64[n_docs + 1]; the text they were encoded from, utf8 and doc_off uint64[n_docs + 1]; a
 * tk_split_spec: max_tokens N, min_tokens M, overlap O, n_levels L <= 4 levels of up to 4 separators each (level 0 is the best place to
 * cut), seg_tokens K.  A separator is a pair (tail, head) of byte strings of 0 .. 16 bytes, not both empty.  Document d has
 * n_d = tok_off[d + 1] - tok_off[d] tokens.
 *  Token boundaries.  Boundary i of a document (0 < i < n_d) lies before its token i, at byte p = byte_start[i] of the document (the
 *   span rule of tk_token_spans_device).  It MATCHES a separator when the document's bytes before p end with tail and its bytes from p on
 *   start with head -- both inside the document: ("\n\n", "") cuts behind a blank line, ("", " ") before a space, (".", " ") behind a
 *   sentence's full stop but not inside 3.14.  It is LEGAL when the byte at p is not a continuation byte 0x80 .. 0xBF.  Its LEVEL is the
 *   lowest level with a separator it matches, if it is legal and there is one.  Only legal boundaries are chosen, so no chunk starts or
 *   ends inside a char.
 *  The chain of a document.  The first chunk starts at s = 0; an empty document owns no chunk.  If n_d - s <= N the chunk is [s, n_d), its
 *   cut is TK_SPLIT_END and the chain ends.  Otherwise look at the legal boundaries e in [s + M, s + N] (all interior): take the lowest
 *   level that occurs among them and of that level the largest e, cut = that level; if none of them has a level the largest legal e,
 *   cut = TK_SPLIT_HARD; if none is legal e = s + N, cut = TK_SPLIT_FORCED (with N - M >= 3 only on ill-formed text: a char is at most
 *   four tokens).  The chunk is [s, e).  The next chunk starts at the smallest legal boundary in [e - O, e], at e if there is none;
 *   O < M makes every start larger than the one before.
 *  Output.  Per chunk, in document order (C of them): doc; tok_begin, tok_end: token indices inside the document; byte_begin, byte_end and
 *   char_begin, char_end: the same places in the document's text, bytes and chars (byte_start / char_start of the span rule, the
 *   document's length at its end; chars are exact at legal boundaries); cut (uint8).  doc_chunk uint32[n_docs + 1]: the first chunk of
 *   every document, C at the end.
 *  What the chunks promise.  tok_end - tok_begin <= N counts the document's OWN tokenisation: a chunk's text encoded on its own may
 *   tokenise differently at its two edges, so its count may differ by a few.  With O == 0 the byte ranges of a document's chunks tile it
 *   exactly.  The result depends on nothing but the rule: not on K, which only sets how the work is spread (0: the library's choice).
 *  TK_VALUE_ERROR: M == 0, M + 3 > N, O >= M; a separator part longer than 16 bytes or a separator with both parts empty; more than 4
 *   levels or more than 4 separators in a level; K neither 0 nor a multiple of 64; an unknown flag; T >= 2^32 or n_docs >= 2^32 - 1; a
 *   tok_off that does not ascend from 0 to n_tokens (checked on the device before anything is indexed with it; the message names the first
 *   offending document).  What tk_token_spans_device refuses is refused in its words: TK_UNSUPPORTED for ids too sparse for a direct table
 *   and for text a generic pat_str leaves unmatched, TK_VALUE_ERROR for a document of 4 GiB, TK_KEY_ERROR for an id without an entry.
 *   A refused call leaves the previous result whole.  One device per call: a group has no split entry.
 *  NOT built: a bound on the count of a chunk encoded on its own; separators longer than 16 bytes; regex separators; an overlap that
 *   snaps to separators (it snaps to chars only); several GPUs. */
#define TK_SPLIT_HARD 0xFDu   /* cut: no separator in the window, the last legal boundary */
#define TK_SPLIT_FORCED 0xFEu /* cut: no legal boundary in the window either (ill-formed text) */
#define TK_SPLIT_END 0xFFu    /* cut: the document's end */
typedef struct {
    uint8_t tail_len, head_len;
    uint8_t tail[16], head[16];
} tk_split_sep;
typedef struct {
    uint32_t max_tokens, min_tokens, overlap, n_levels, seg_tokens, flags; /* flags: none defined, must be 0 */
    uint32_t n_seps[4];                                                   /* separators of every level */
    tk_split_sep sep[4][4];
} tk_split_spec;
/* Device pointers in (ids uint32, d_tok_off and d_doc_off uint64[n_docs + 1], d_utf8 the text: e.g. the arguments and results of
 * tk_encode_batch_device), device pointers out: buffers of the core, valid until its next split call that succeeds (a refused call writes
 * into none of them) and apart from all others, except that the span buffers are used on the way (a split call ends the validity of
 * tk_token_spans_device's results).  *d_doc_out .. *d_char_end_out (uint32) and *d_cut_out (uint8): *n_chunks_out each; *d_doc_chunk_out:
 * n_docs + 1.  `stream`: a hipStream_t or null (the core's); the call returns when the chunks are there. */
int tk_split_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const void* d_utf8,
                    const void* d_doc_off, const tk_split_spec* spec, void* stream, const uint32_t** d_doc_out, const uint32_t** d_tok_begin_out,
                    const uint32_t** d_tok_end_out, const uint32_t** d_byte_begin_out, const uint32_t** d_byte_end_out,
                    const uint32_t** d_char_begin_out, const uint32_t** d_char_end_out, const uint8_t** d_cut_out,
                    const uint32_t** d_doc_chunk_out, uint64_t* n_chunks_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked -- with the text cut into chunks while ids and text are on the
 * device: host text in; the chunk arrays and the ids come out.  *doc_out .. *doc_chunk_out and *tokens_out: library-owned (tk_free), sized
 * as above; tok_off_out (may be null): the caller's array of n_docs + 1.  On TK_DISALLOWED_SPECIAL nothing is handed out. */
int tk_encode_batch_split(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                          const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed,
                          const tk_split_spec* spec, uint32_t** doc_out, uint32_t** tok_begin_out, uint32_t** tok_end_out,
                          uint32_t** byte_begin_out, uint32_t** byte_end_out, uint32_t** char_begin_out, uint32_t** char_end_out,
                          uint8_t** cut_out, uint32_t** doc_chunk_out, uint64_t* n_chunks_out, uint32_t** tokens_out, uint64_t* n_tokens_out,
                          uint64_t* tok_off_out, tk_special_hit* hit);
/* JSON Lines: a buffer of lines {"text": "...", "meta": ...}\n -> the unescaped text of ONE field per line, packed as the encode entries
 * take it (text, doc_off), with the status of every line.  Replaces nothing in the reference: it is the host loop of the reference's
 * users, `for line in f: json.loads(line)["text"]`, in front of every batch encode -- here a pass over bytes that go to the device anyway.
 * The rule (its plain C++: tiktoken_amd/csrc/tk_jsonl_rule.h; restated in tests/jsonl_ref.py).  The buffer is cut into lines at every raw
 * 0x0A; a last line without a newline counts; a \r before the newline is trailing whitespace; a UTF-8 BOM at byte 0 is skipped.  JSON
 * forbids a raw newline inside a string, so string state never crosses a line: lines are independent, which makes the pass parallel.
 * Within a line: a byte is ESCAPED if an odd run of backslashes ends right before it; an unescaped " toggles the IN-STRING state; outside
 * strings { [ raise the DEPTH and } ] lower it.  A KEY is a string that opens at depth 1 and whose closing quote is followed, after any of
 * space \t \r, by ':'.  The FIELD (1 .. 64 bytes, no ", \ or byte < 0x20) matches a key whose raw bytes between the quotes equal it -- a
 * key spelled with escapes does not match.  Of several matching keys the last wins, as with json.loads.  After the colon and whitespace,
 * if the next byte is " the VALUE is the string that opens there; anything else gives TK_JSONL_NOT_STRING.  UNESCAPE: \" \\ \/ \b \f \n
 * \r \t become one byte each; \uXXXX (hex in either case) the UTF-8 of the code point; a high surrogate escape directly followed by a low
 * one becomes one 4-byte char; a surrogate escape without its partner becomes U+FFFD (what Encoding.encode makes of the str json.loads
 * returns for it); other bytes are copied.  Every escape shrinks: the text never exceeds n_bytes.
 * STATUS per line (uint8): TK_JSONL_OK; TK_JSONL_BLANK: only whitespace, never a record; TK_JSONL_MISSING: no matching key at depth 1;
 * TK_JSONL_NOT_STRING; TK_JSONL_BAD: the first non-whitespace byte is not '{'; a string is open at the line's end; the depth is not 0 at
 * the line's end or drops below 1 before the last structural byte; a raw byte < 0x20 inside any string; inside the SELECTED VALUE a
 * backslash followed by anything outside the list above or \u without four hex digits; inside the selected value ill-formed UTF-8, by
 * the strictness of tk_validate_utf8.  BAD takes precedence over the others.  THE PASS IS NOT A JSON VALIDATOR: numbers, literals, commas
 * and escapes in strings other than the selected value are not checked.  For every line json.loads accepts as an object, status and text
 * equal what json.loads(line).get(field) gives, with the surrogate repair above.
 * flags: TK_JSONL_RAISE refuses the call (TK_JSONL_ERROR) with the first line that is neither OK nor BLANK: *bad and tk_last_error() name
 * its index, its byte offset and its status; a refused call leaves the previous result whole.  TK_JSONL_SKIP leaves such lines out.
 * TK_JSONL_EMPTY keeps an empty document for every non-blank line, so documents align with records.
 * Results: text uint8[n_text] and doc_off uint64[n_docs + 1] (what tk_encode_batch_device takes; 64 readable bytes follow the text);
 * line uint64[n_docs]: the line every document came from; line_off uint64[n_lines + 1]: where every line starts, n_bytes at the end;
 * status uint8[n_lines].  TK_VALUE_ERROR: a field that is not 1 .. 64 bytes or holds ", \ or a byte < 0x20; an unknown flag; more than
 * 0xFFFF0000 bytes.  NOT built: several fields or a nested path; keys spelled with escapes; full JSON validation; gzip / zstd input;
 * several GPUs; the row, padded, chunk and sample entries fed straight from JSON Lines (they chain through the device entries). */
#define TK_JSONL_OK 0u
#define TK_JSONL_BLANK 1u
#define TK_JSONL_MISSING 2u
#define TK_JSONL_NOT_STRING 3u
#define TK_JSONL_BAD 4u
#define TK_JSONL_RAISE 0u
#define TK_JSONL_SKIP 1u
#define TK_JSONL_EMPTY 2u
typedef struct {
    uint64_t line, pos; /* the refused line's index and where it starts in the buffer */
    uint32_t status, reserved;
} tk_jsonl_bad;
/* Device pointer in, device pointers out: buffers of the core, valid until its next JSON Lines call that succeeds and apart from all
 * others.  `stream`: a hipStream_t or null (the core's); the call returns when the results are there.  bad may be null. */
int tk_jsonl_extract_device(tk_core* core, const void* d_bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, void* stream,
                            const uint8_t** d_text_out, const uint64_t** d_doc_off_out, const uint64_t** d_line_out, const uint64_t** d_line_off_out,
                            const uint8_t** d_status_out, uint64_t* n_docs_out, uint64_t* n_lines_out, uint64_t* n_text_out, tk_jsonl_bad* bad);
/* Host in, host out: the arrays are library-owned (tk_free). */
int tk_jsonl_extract(tk_core* core, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, uint8_t** text_out,
                     uint64_t** doc_off_out, uint64_t** line_out, uint64_t** line_off_out, uint8_t** status_out, uint64_t* n_docs_out, uint64_t* n_lines_out,
                     uint64_t* n_text_out, tk_jsonl_bad* bad);
/* Extracts, then encodes the text while it is in HBM (tk_encode_batch_device, with n_disallowed != 0 tk_encode_batch_device_checked): the
 * text never visits the host.  tokens, tok_off uint64[n_docs + 1], line and status are library-owned (tk_free).  On
 * TK_DISALLOWED_SPECIAL hit->doc is the document; its line is line[doc] of an extract call with the same arguments. */
int tk_encode_jsonl(tk_core* core, const uint8_t* bytes, uint64_t n_bytes, const uint8_t* field, uint64_t field_len, uint32_t flags, int use_special,
                    const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, uint32_t** tokens_out,
                    uint64_t* n_tokens_out, uint64_t** tok_off_out, uint64_t** line_out, uint8_t** status_out, uint64_t* n_docs_out, uint64_t* n_lines_out,
                    tk_special_hit* hit, tk_jsonl_bad* bad);
/* Near-duplicate fingerprints: a packed batch -> per document a MinHash signature over its token shingles, the LSH band keys of that
 * signature, an exact hash and the shingle count.  Replaces nothing in the reference: it is the host step of the reference's users
 * between "tokenise" and "pack rows", duplicate and near-duplicate removal -- here one call on ids that are on the device anyway.
 * The rule.  All arithmetic is unsigned, modulo 2^64 unless a narrower width is said.
 *  mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; the result is
 *   z ^ (z >> 31).
 *  Parameters (tk_fingerprint_spec): ngram k in 1 .. 32; n_perm P in 1 .. 256; bands B in 1 .. P with P % B == 0, r = P / B; seed, a
 *   uint64.  Anything else is TK_VALUE_ERROR, and nothing is written.
 *  Shingles.  Document d holds the tokens t[s .. e), s = tok_off[d], e = tok_off[d + 1], L = e - s.  L == 0: it has no shingle.
 *   1 <= L < k: it has one shingle, over all its L ids (m = L).  L >= k: it has L - k + 1 shingles, one per start position, of m = k ids.
 *   A shingle never crosses a document boundary.
 *  A shingle's hash over the ids u[0 .. m): x = mix(seed ^ m), then for j = 0 .. m - 1: x = mix(x ^ u[j]); the hash h is the last x.
 *   Ids are taken as uint32 values, whatever they are: an id need not be a token of the vocabulary.
 *  Permutation p (0 <= p < P): a_p = mix(seed + 2p + 1) | 1, b_p = mix(seed + 2p + 2); its value at h is (uint32)((a_p * h + b_p) >> 32).
 *  sig[d][p]: the minimum of permutation p's values over the hashes of d's shingles; 0xFFFFFFFF if d has none.
 *  n_shingles[d] (uint64): how many shingles d has.
 *  band[d][j] (0 <= j < B): x = mix(seed ^ 0x42414E4400000000 ^ j), then for i = 0 .. r - 1: x = mix(x ^ sig[d][j * r + i]); the key is
 *   the last x.  It is defined for empty documents too; consumers skip documents with n_shingles == 0.
 *  exact[d] = mix(L ^ sum over i < L of mix(seed ^ ((i + 1) << 32) ^ t[s + i])): the position makes it depend on the order.
 *  Minimum and sum are commutative: the result is a function of (tokens, tok_off, spec) alone.
 * NOT built: shingles of the text's words or chars; grouping on the device; an index across batches; several GPUs; b-bit signatures;
 *  entries fed from JSON Lines or from chunks. */
typedef struct {
    uint32_t ngram, n_perm, bands;
    uint64_t seed;
} tk_fingerprint_spec;
/* Device pointers in (ids uint32, d_tok_off uint64[n_docs + 1]: e.g. the results of tk_encode_batch_device), the caller's device arrays
 * out, any of which may be null: d_sig uint32[n_docs * P], d_band uint64[n_docs * B], d_exact and d_n_shingles uint64[n_docs].  Everything
 * is queued on `stream` and the call returns without waiting: the arrays are ready when the stream has got there, and whoever reads them
 * orders the read behind this call on that stream, as the call orders itself behind whatever made d_tokens and d_tok_off there.  `stream`
 * is a hipStream_t exactly as a kernel launch takes one; null is HIP's null stream -- not the core's own stream, as in the entries
 * that wait before they return: the caller could not wait on that.  With d_band but without d_sig the signatures pass through a buffer
 * of the core; the library orders the calls that use that buffer among themselves on the device (an event, no host wait), whatever
 * their streams and entries, so nothing is asked of the caller.  d_tok_off is not checked: it must ascend from 0 to n_tokens; one that does not gives values nobody has defined, never
 * an access outside the arrays.  d_exact holds the sum until the last pass closes it.  n_docs == 0 and n_tokens == 0 are valid. */
int tk_fingerprint_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec,
                          void* stream, uint32_t* d_sig, uint64_t* d_band, uint64_t* d_exact, uint64_t* d_n_shingles);
/* The same from host arrays to the caller's host arrays (sized as above, any may be null); tok_off[n_docs] is the number of tokens, and
 * a tok_off that does not ascend from 0 is TK_VALUE_ERROR. */
int tk_fingerprint(tk_core* core, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, const tk_fingerprint_spec* spec, uint32_t* sig_out,
                   uint64_t* band_out, uint64_t* exact_out, uint64_t* n_shingles_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked -- with the fingerprints of the ids while they are on the device:
 * host text in, the caller's host arrays out (sized as above, any may be null; tok_off_out: n_docs + 1).  The ids stay on the device
 * unless tokens_out is there (library-owned, tk_free; *n_tokens_out ids).  On TK_DISALLOWED_SPECIAL nothing is handed out. */
int tk_encode_batch_fingerprint(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special, const uint32_t* allowed_ids,
                                uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const tk_fingerprint_spec* spec, uint32_t* sig_out,
                                uint64_t* band_out, uint64_t* exact_out, uint64_t* n_shingles_out, uint64_t* tok_off_out, uint32_t** tokens_out,
                                uint64_t* n_tokens_out, tk_special_hit* hit);
/* Supervised samples: a packed batch whose documents are the PARTS of samples -- the messages of a conversation, a prompt and its answer --
 * -> one row per sample with the template's ids around every part, an attention mask and labels.  Replaces nothing in the reference: it is
 * the host loop of the reference's users, the fine-tuning script that calls encode_ordinary once per message, adds header and footer ids and
 * builds ids and labels as Python lists -- here one call on ids that are on the device anyway.
 * The rule.  Input: tokens uint32[T]; tok_off uint64[n_parts + 1]: part p (what the encode call knows as a document) has
 * n_p = tok_off[p + 1] - tok_off[p] body tokens; part_role uint8[n_parts]; sample_off uint64[n_samples + 1], ascending from 0 to n_parts:
 * sample s is the parts [sample_off[s], sample_off[s + 1]), and a sample with no parts is legal.  The role table (host memory in every
 * entry): n_roles <= 256; role_ids uint32[], at most 4096 in all; role_off uint32[2 * n_roles + 1] ascending from 0: the BEFORE ids of role r
 * are role_ids[role_off[2r] .. role_off[2r + 1]), its AFTER ids role_ids[role_off[2r + 1] .. role_off[2r + 2]), either may be empty;
 * role_train uint8[n_roles].
 *  Stream of a sample.  [bos_id], then for each of its parts in order before(role) body after(role), then [eos_id] (TK_ROWS_NO_TOKEN: no
 *   bos / no eos).  Its length is full_len[s].  A part that contributes no element owns no position.
 *  Trained elements.  The body and the after ids of a part whose role has role_train != 0.  Before ids and bos never; eos iff the sample
 *   has a part and its last part's role trains.
 *  Truncation.  len[s] = min(full_len[s], max_len); the row holds the stream elements [0, len), with TK_SMP_KEEP_TAIL
 *   [full_len - len, full_len).  The stream is cut as it is: nothing is re-inserted, and a cut may fall inside a before run, a body or an
 *   after run.
 *  Row s of [R = n_samples, W].  Its elements are in columns [0, len), with TK_SMP_LEFT in [W - len, W).  ids (uint32): the element, pad_id
 *   elsewhere.  mask (uint8): 1 on elements, 0 elsewhere.  labels (int32): the id where the element is trained, ignore_index everywhere
 *   else, padding included.  Labels are NOT shifted: the model shifts them.
 *  Per sample.  len uint32[R]; full_len uint64[R] (a caller drops over-long samples by it); n_trained uint32[R]: the trained elements that
 *   survived the cut (a caller drops samples with nothing to learn by it, and normalises the loss).
 *  Width.  As tk_pad_batch_device: width_multiple == 0: W = max_len, otherwise W = min(max_len, ceil(longest / width_multiple) *
 *   width_multiple) with longest = max len[s], 0 when there is no sample.  W = 0 is a legal result.
 *  TK_VALUE_ERROR, every one found before any output is written (a refused call leaves the previous result whole): max_len == 0;
 *   n_roles == 0 while there are parts; n_roles > 256, more than 4096 role ids or a role_off that does not ascend from 0;
 *   part_role[p] >= n_roles (the message names the first such part); a tok_off that does not ascend from 0 to n_tokens (the first offending
 *   part, called a document as in the other passes); a sample_off that does not ascend from 0 to n_parts (the first offending sample);
 *   T >= 2^32; n_parts or n_samples >= 2^32 - 1; 2^32 elements or more over all parts; R * W >= 2^32.  The three device arrays are checked
 *   on the device before anything is indexed with them: no kernel reads or writes out of bounds, whatever they hold.
 *  One device per call: a group has no samples entry.  NOT built: 16-bit ids; windows for over-long samples; a special-token policy per
 *   part (the call's policy holds for all parts); a template language (callers encode their few header and footer strings once and pass
 *   the ids).  Several samples in one row: tk_pack_samples_device below.  TK_SMP_SKIP_LONG and TK_SMP_IGNORE_FIRST mean something there
 *   only: this entry refuses them with TK_VALUE_ERROR, as it refuses every flag bit it does not know. */
#define TK_SMP_KEEP_TAIL 1u    /* keep an over-long sample's last elements, not its first */
#define TK_SMP_LEFT 2u         /* padding in front of the row's elements, not behind (tk_assemble_samples_device only) */
#define TK_SMP_SKIP_LONG 4u    /* tk_pack_samples_device only: leave an over-long sample out instead of cutting it */
#define TK_SMP_IGNORE_FIRST 8u /* tk_pack_samples_device only: the label of every sample's first element is ignore_index */
typedef struct {
    uint32_t max_len, width_multiple, bos_id, eos_id, pad_id;
    int32_t ignore_index;
    uint32_t flags;
} tk_smp_spec;
/* Device pointers in (ids uint32, d_tok_off uint64[n_parts + 1]: e.g. the results of tk_encode_batch_device; d_part_role uint8[n_parts],
 * d_sample_off uint64[n_samples + 1]), the role table in host memory (role_ids / role_off / role_train may be null where they would be
 * empty), device pointers out: buffers of the core, valid until its next samples call that succeeds (a refused call writes into none of
 * them) and apart from the encode, decode, span, rows and padded buffers (assembling an encode call's result leaves it intact).  *d_ids_out,
 * *d_mask_out, *d_labels_out: *n_rows_out x *width_out; *d_len_out, *d_full_len_out, *d_n_trained_out: *n_rows_out.  `stream`: a hipStream_t
 * or null (the core's); the call returns when the rows are there. */
int tk_assemble_samples_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_parts, const void* d_part_role,
                               const void* d_sample_off, uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off,
                               const uint8_t* role_train, const tk_smp_spec* spec, void* stream, const uint32_t** d_ids_out, const uint8_t** d_mask_out,
                               const int32_t** d_labels_out, const uint32_t** d_len_out, const uint64_t** d_full_len_out, const uint32_t** d_n_trained_out,
                               uint64_t* n_rows_out, uint64_t* width_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked, whose *hit names the PART -- over the parts' text (doc_off: n_parts + 1
 * byte offsets), with the samples assembled while the ids are on the device: host text, part_role and sample_off in, and only the sample
 * arrays cross the link back (the ids themselves are not handed out).  *ids_out .. *n_trained_out: library-owned (tk_free), sized as above.
 * On TK_DISALLOWED_SPECIAL nothing is handed out. */
int tk_encode_batch_samples(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_parts, int use_special, const uint32_t* allowed_ids,
                            uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const uint8_t* part_role, const uint64_t* sample_off,
                            uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train,
                            const tk_smp_spec* spec, uint32_t** ids_out, uint8_t** mask_out, int32_t** labels_out, uint32_t** len_out, uint64_t** full_len_out,
                            uint32_t** n_trained_out, uint64_t* n_rows_out, uint64_t* width_out, tk_special_hit* hit);
/* Packed sample rows: the samples of tk_assemble_samples_device, several whole ones to a row of max_len, with what block-diagonal /
 * variable-length attention needs to keep them apart.  Replaces nothing in the reference: it is the packing loop of its users' SFT data
 * collators -- here one call on ids that are on the device anyway, and a third less padding through the model than one row per sample.
 * The rule.  Inputs, role table, stream of a sample, trained elements, truncation (len[s] = min(full_len[s], max_len), TK_SMP_KEEP_TAIL) and
 * full_len are exactly those of tk_assemble_samples_device, and so is the tk_smp_spec.  L = max_len.
 *  Placed length.  plen[s] = len[s]; with TK_SMP_SKIP_LONG plen[s] = 0 where full_len[s] > L: the sample is left out instead of cut.  A
 *   sample with plen == 0 owns no position.
 *  Placement is next-fit in input order -- it keeps the caller's order, so the caller's shuffle or sort is the policy:
 *     row = 0; fill = 0; any = false
 *     for s in 0 .. n_samples - 1:
 *         p = plen[s]
 *         if p == 0: sample_row[s] = TK_ROWS_NO_TOKEN; sample_col[s] = 0; continue
 *         if fill + p > L: row += 1; fill = 0
 *         sample_row[s] = row; sample_col[s] = fill; fill += p; any = true
 *     R = any ? row + 1 : 0
 *   row_sample uint32[R + 1]: the first sample with sample_row == r, and row_sample[R] = n_samples.  Every row holds at least one element.
 *   The width is L always.
 *  Per position (r, c) of [R, L], fill_r being the placed lengths of row r's samples together:
 *   ids (uint32)    the element, or pad_id on the row's tail (c >= fill_r)
 *   labels (int32)  as in tk_assemble_samples_device, unshifted: the id where the element is trained, ignore_index everywhere else; with
 *                   TK_SMP_IGNORE_FIRST also ignore_index at pos == 0 of every sample (after the model's shift that element would be
 *                   predicted from the previous sample's last token)
 *   seg (uint32)    the sample, or TK_ROWS_NO_TOKEN on padding
 *   pos (uint32)    c - sample_col[seg] on elements, c - fill_r on the tail: a row's padding tail is a segment of its own, as padding is in
 *                   tk_pack_rows_device
 *  Segments.  cu_seqlens uint32[n_segs + 1]: the flat positions r * L + c with pos == 0, ascending, then R * L; row_seg uint32[R + 1]: the
 *   segment starts below r * L, so cu_seqlens[row_seg[a] .. row_seg[b]] - a * L are the boundaries of the rows a .. b alone.
 *   n_segs = placed samples + rows with fill_r < L.
 *  Per sample.  len uint32[n_samples] and full_len uint64[n_samples] as in tk_assemble_samples_device (of an unplaced sample too);
 *   n_trained uint32[n_samples]: the labels of the sample that are not ignore_index by the rule -- tk_assemble_samples_device's figure, one
 *   less where TK_SMP_IGNORE_FIRST masks a trained first element, and 0 for a sample that is not placed; sample_row, sample_col uint32[n_samples].
 *  TK_VALUE_ERROR, every one found before any output is written (a refused call leaves the previous result of this entry, and the encode
 *   result, whole): everything tk_assemble_samples_device refuses; width_multiple != 0; TK_SMP_LEFT; R * L >= 2^32.  The three device
 *   arrays are checked on the device before anything is indexed with them: no kernel reads or writes out of bounds, whatever they hold.
 *  One device per call: a group has no packed-samples entry.  NOT built: best-fit or sorted packing (sort the samples before the call);
 *   16-bit ids; windows for over-long samples; a special-token policy per part. */
/* Device pointers in and the role table in host memory as in tk_assemble_samples_device, device pointers out: buffers of the core, valid
 * until its next packed-samples call that succeeds (a refused call writes into none of them) and apart from every other entry's buffers
 * (packing an encode call's result leaves it intact, and so does it a tk_assemble_samples_device result).  *d_ids_out, *d_labels_out,
 * *d_seg_out, *d_pos_out: *n_rows_out x max_len; *d_cu_seqlens_out: *n_segs_out + 1; *d_row_seg_out, *d_row_sample_out: *n_rows_out + 1;
 * *d_len_out .. *d_sample_col_out: n_samples.  `stream`: a hipStream_t or null (the core's); the call returns when the rows are there. */
int tk_pack_samples_device(tk_core* core, const void* d_tokens, uint64_t n_tokens, const void* d_tok_off, uint64_t n_parts, const void* d_part_role,
                           const void* d_sample_off, uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off,
                           const uint8_t* role_train, const tk_smp_spec* spec, void* stream, const uint32_t** d_ids_out, const int32_t** d_labels_out,
                           const uint32_t** d_seg_out, const uint32_t** d_pos_out, const uint32_t** d_cu_seqlens_out, const uint32_t** d_row_seg_out,
                           const uint32_t** d_row_sample_out, const uint32_t** d_len_out, const uint64_t** d_full_len_out, const uint32_t** d_n_trained_out,
                           const uint32_t** d_sample_row_out, const uint32_t** d_sample_col_out, uint64_t* n_rows_out, uint64_t* n_segs_out);
/* tk_encode_batch -- with n_disallowed != 0: tk_encode_batch_checked, whose *hit names the PART -- over the parts' text (doc_off: n_parts + 1
 * byte offsets), with the samples packed into rows while the ids are on the device: host text, part_role and sample_off in, and only the
 * row arrays cross the link back.  *ids_out .. *sample_col_out: library-owned (tk_free), sized as above.  On TK_DISALLOWED_SPECIAL nothing
 * is handed out. */
int tk_encode_batch_sample_rows(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_parts, int use_special, const uint32_t* allowed_ids,
                                uint64_t n_allowed, const uint32_t* disallowed_ids, uint64_t n_disallowed, const uint8_t* part_role, const uint64_t* sample_off,
                                uint64_t n_samples, uint32_t n_roles, const uint32_t* role_ids, const uint32_t* role_off, const uint8_t* role_train,
                                const tk_smp_spec* spec, uint32_t** ids_out, int32_t** labels_out, uint32_t** seg_out, uint32_t** pos_out, uint32_t** cu_seqlens_out,
                                uint32_t** row_seg_out, uint32_t** row_sample_out, uint32_t** len_out, uint64_t** full_len_out, uint32_t** n_trained_out,
                                uint32_t** sample_row_out, uint32_t** sample_col_out, uint64_t* n_rows_out, uint64_t* n_segs_out, tk_special_hit* hit);
/* Decoding id matrices: what a generation, evaluation or reranking loop hands back -- an id matrix [R, W] in HBM -- -> the text of every
 * row.  Replaces nothing in the reference: it is the host loop of the reference's users (the matrix copied to the host, every row cut at its
 * first eos and stripped of pad and special ids in Python, the lists handed to decode_batch; elsewhere `batch_decode(ids,
 * skip_special_tokens=True)`) -- here one call on ids that are on the device anyway.  The decode-side counterpart of tk_pad_batch_device.
 * The rule.  Input: ids holds R rows of W columns, element (r, c) at ids[r * ld + c] with ld >= W, so a column slice of a wider matrix
 *  needs no copy; its elements are uint32, with TK_DROWS_I32 int32, with TK_DROWS_I64 int64.  begin / end (uint32[R] each, may be null: 0
 *  and W).  Up to 16 stop_ids and up to 16 skip_ids (uint32) in the spec.
 *  Live range of row r.  stop_col[r] = the least c in [begin[r], end[r]) whose id is in stop_ids, or end[r] when there is none; columns
 *   before begin[r] are never looked at.  The live range is [begin[r], stop_col[r]), with TK_DROWS_KEEP_STOP also stop_col[r] itself when a
 *   stop was found.  stop_col[r] < end[r] says that the row finished.
 *  Kept tokens.  A live column is kept unless its id is in skip_ids or -- TK_DROWS_SKIP_SPECIAL -- is a special token of the vocabulary.
 *   The stop test comes first: a kept stop id then passes the skip test like any other id.
 *  Output.  tokens uint32[K]: the kept ids of all rows back to back, in row and column order; tok_off uint64[R + 1]: each row's place in
 *   tokens; n_kept uint32[R] and stop_col uint32[R]; bytes and byte_off uint64[R + 1]: what tk_decode_batch_device makes of (tokens,
 *   tok_off), by the same kernels.  R == 0, W == 0 and K == 0 are legal.
 *  TK_VALUE_ERROR: more than 16 stop or skip ids; both dtype flags; an unknown flag; ld < W; R >= 2^32 - 1, W >= 2^32 or K >= 2^32; a
 *   matrix of 2^60 elements or more; a row with begin > end or end > W (checked on the device before anything is indexed with either;
 *   the message names the first such row).  TK_KEY_ERROR: a kept column whose id has no decode entry -- a negative element, or one at
 *   or above 2^32 in a 64-bit matrix, is such an id; in no list either --: the reference's "Invalid token for decoding: N", then the row and
 *   column of the first such element in row-major order.  Ids outside the live range are never judged, and skipped ids are not either: a
 *   pad id outside the vocabulary is legal in skip_ids.  TK_UNSUPPORTED where tk_decode_batch returns it: ids at or above 2^26.
 *   Every refusal is found before any output is written: a refused call leaves the previous result whole.  No kernel reads outside the
 *   (R - 1) * ld + W elements of the matrix, whatever begin and end hold.  One device per call: a group has no such entry.
 *  Text instead of bytes (errors="replace" / "ignore" applied on the device): tk_decode_rows_text_device / tk_decode_rows_text below.
 *  Rows cut at a stop STRING as well (until=, stop=, stop_strings=): tk_decode_rows_until_device / tk_decode_rows_until below.
 *  Rows that arrive a few columns per step (a generation loop): tk_stream_create below.
 *  NOT built: uint16 matrices; token spans of a matrix (feed tokens and tok_off to tk_token_spans_device). */
#define TK_DROWS_KEEP_STOP 1u    /* the stop id that ends a row belongs to it */
#define TK_DROWS_SKIP_SPECIAL 2u /* special tokens are dropped as if they were in skip_ids */
#define TK_DROWS_I32 4u          /* the matrix holds int32 */
#define TK_DROWS_I64 8u          /* the matrix holds int64 */
typedef struct {
    uint32_t flags, n_stop, n_skip;
    uint32_t stop_ids[16], skip_ids[16];
} tk_drows_spec;
/* Device pointers in (d_ids; d_begin / d_end uint32[n_rows] or null), device pointers out: *d_tokens_out .. *d_stop_col_out are buffers
 * of the core, valid until its next decode-rows call that succeeds (a refused call writes into none of them) and apart from every other
 * entry's buffers; *d_bytes_out and *d_byte_off_out are the decode buffers of tk_decode_batch_device, valid until the core's next decode
 * call.  *n_tokens_out: K.  `stream`: a hipStream_t or null (the core's); the call returns when the bytes are there. */
int tk_decode_rows_device(tk_core* core, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                          const tk_drows_spec* spec, void* stream, const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out,
                          const uint32_t** d_n_kept_out, const uint32_t** d_stop_col_out, const uint8_t** d_bytes_out,
                          const uint64_t** d_byte_off_out, uint64_t* n_tokens_out, uint64_t* n_bytes_out);
/* The same for a matrix in host memory ((n_rows - 1) * ld + width elements travel to the device as they lie): host arrays out,
 * library-owned (tk_free), sized as above. */
int tk_decode_rows(tk_core* core, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                   const tk_drows_spec* spec, uint32_t** tokens_out, uint64_t** tok_off_out, uint32_t** n_kept_out, uint32_t** stop_col_out,
                   uint8_t** bytes_out, uint64_t** byte_off_out, uint64_t* n_tokens_out, uint64_t* n_bytes_out);
/* Encoding.decode(tokens, errors="replace")                                  tiktoken/core.py:275-287
 * UTF-8 repair on the device: packed bytes in HBM -> packed, well-formed UTF-8 in HBM.  The reference's decode is
 * bytes.decode("utf-8", errors) on one document; this is that call on every document of a packed batch (bytes uint8[n_bytes], byte_off
 * uint64[n_docs + 1]), each on its own, without the text leaving the device and without a host loop over the documents.
 * The rule.  A document's bytes fall into consecutive units:
 *  ASCII byte (00..7F): a unit of its own, copied.
 *  Lead byte with a declared length: C2..DF declares L = 2, E0..EF L = 3, F0..F4 L = 4.  It accepts the bytes that follow it while they
 *   are fewer than L - 1, lie inside the document, and each is a continuation byte 80..BF; the FIRST accepted byte has a narrower range
 *   after four leads: E0: A0..BF, ED: 80..9F, F0: 90..BF, F4: 80..8F.  With all L - 1 bytes accepted the unit is well-formed and its L
 *   bytes are copied.  Otherwise the lead and what it accepted are one ill-formed unit (the "maximal subpart").
 *  Any other byte -- C0, C1, F5..FF, a continuation byte that no lead accepted -- is an ill-formed unit of one byte.
 *  TK_U8_REPLACE writes EF BF BD (U+FFFD) for every ill-formed unit, TK_U8_IGNORE writes nothing for it.
 *  Nothing crosses a document boundary: a sequence cut by one is ill-formed on both sides.
 *  Under TK_U8_REPLACE the output is at most three times the input (a run of stray continuation bytes).
 *  The same length does not mean clean: F0 9F 98 at a document's end becomes EF BF BD.  "Nothing replaced" is a count of its own,
 *   *n_replaced_out == 0, never *n_text_out == n_bytes.
 * Whether a byte starts a unit, is swallowed by one or is replaced depends on the three bytes before it and the three behind it, inside
 * its document: the pass is local (tk_utf8_repair.h).
 * Output.  text uint8[n_text]; text_off, char_off, repl_off uint64[n_docs + 1]: the bytes of the output, its chars (code points, U+FFFD
 *  included) and the ill-formed units (replaced or dropped) of the documents before each document; entry n_docs is the total.
 * In: d_bytes on the core's device, 16-byte aligned and readable for 16 bytes past n_bytes (the core's decode buffers are); d_byte_off
 *  uint64[n_docs + 1] there, ascending from 0 to n_bytes.  mode: TK_U8_REPLACE or TK_U8_IGNORE.  n_bytes == 0 and n_docs == 0 are legal.
 * Out: buffers of the core that belong to this entry alone, valid until the core's next repair call (this entry, tk_decode_batch_text,
 *  tk_decode_rows_text_device, tk_decode_rows_text) -- except that with *n_replaced_out == 0 nothing is written: *d_text_out == d_bytes
 *  and *d_text_off_out == d_byte_off, the caller's own (char_off and repl_off are made all the same).  The input must not be this entry's
 *  own previous output buffer.
 * TK_VALUE_ERROR: a misaligned pointer, an unknown mode, n_bytes of 2^43 or more, offsets that do not ascend from 0 to n_bytes (checked on the device before
 *  anything is indexed with them; the message names the first offending document).  A refused call leaves the previous result whole.
 *  No kernel reads outside [d_bytes, d_bytes + n_bytes + 16), whatever the offsets hold.  Holds the core's mutex; `stream`: a
 *  hipStream_t or null (the core's); the call returns when the text is there.  One device per call: a group has no such entry.
 * NOT built: token spans inside repaired text (tk_token_spans_device speaks of the bytes before repair).  Stop strings are searched in
 *  the bytes BEFORE the repair (tk_stop_text_device below, which says why that is the same cut for well-formed stop strings). */
#define TK_U8_REPLACE 0u /* errors="replace" */
#define TK_U8_IGNORE 1u  /* errors="ignore" */
int tk_utf8_repair_device(tk_core* core, const void* d_bytes, uint64_t n_bytes, const void* d_byte_off, uint64_t n_docs, uint32_t mode, void* stream,
                          const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out,
                          const uint64_t** d_repl_off_out, uint64_t* n_replaced_out);
/* Encoding.decode_batch(batch, errors=...) as packed text              tiktoken/core.py:337-343
 * tk_decode_batch's input, host to host: the ids decoded on the device, the repair over their bytes, one copy out.  *text_out ..
 * *repl_off_out: library-owned (tk_free), text_off / char_off / repl_off of n_docs + 1 entries as above.  Errors: those of
 * tk_decode_batch (TK_KEY_ERROR "Invalid token for decoding: N", TK_UNSUPPORTED for ids at or above 2^26), and an unknown mode.
 * One pass over the whole batch: the overlapped ranges of 16 Mi ids that tk_decode_batch runs large batches in are NOT built here. */
int tk_decode_batch_text(tk_core* core, const uint32_t* tokens, const uint64_t* tok_off, uint64_t n_docs, uint32_t mode, uint8_t** text_out,
                         uint64_t* n_text_out, uint64_t** text_off_out, uint64_t** char_off_out, uint64_t** repl_off_out, uint64_t* n_replaced_out);
/* tk_decode_rows_device / tk_decode_rows with text for bytes: the rows passes run unchanged (the rule, the tk_drows_spec and every refusal
 * are theirs), then the repair runs over the rows' bytes, every row a document.  A multi-byte char spelled by byte-level tokens is
 * routinely split by the stop id, by begin, by end and by skipped ids: here the packed result is well-formed UTF-8 all the same.
 * *d_tokens_out .. *d_stop_col_out as tk_decode_rows_device; *d_text_out .. *d_repl_off_out as tk_utf8_repair_device (with
 * *n_replaced_out == 0 text and text_off ARE the decode buffers, valid until the core's next decode call). */
int tk_decode_rows_text_device(tk_core* core, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                               const tk_drows_spec* spec, uint32_t mode, void* stream, const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out,
                               const uint32_t** d_n_kept_out, const uint32_t** d_stop_col_out, const uint8_t** d_text_out, const uint64_t** d_text_off_out,
                               const uint64_t** d_char_off_out, const uint64_t** d_repl_off_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                               uint64_t* n_replaced_out);
int tk_decode_rows_text(tk_core* core, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                        const tk_drows_spec* spec, uint32_t mode, uint32_t** tokens_out, uint64_t** tok_off_out, uint32_t** n_kept_out, uint32_t** stop_col_out,
                        uint8_t** text_out, uint64_t** text_off_out, uint64_t** char_off_out, uint64_t** repl_off_out, uint64_t* n_tokens_out,
                        uint64_t* n_text_out, uint64_t* n_replaced_out);
/* Stop strings: packed text in HBM -> every document cut at the first place where one of a few stop strings lies.  What evaluation
 * harnesses call until=["\n\n", "Question:"], servers stop=[...] and generate stop_strings: the end of a generated row that is a piece of
 * TEXT, not a token -- "\n\n" may be one id, two ids or the tail of ".\n\n" -- and can therefore only be found in the decoded bytes.
 * Replaces nothing in the reference: it is the host loop of its users (the text copied to the host, find per row and per string).
 * The rule.  Input: packed text (bytes uint8[n_bytes], byte_off uint64[n_docs + 1]) under the contract of tk_utf8_repair_device, and a
 *  stop set: n strings, 0 <= n <= 16, of 1 .. 64 bytes each, given as a host blob and off uint32[n + 1] ascending from 0.  Any bytes are
 *  legal: the search is a byte search.
 *  Hit.  Document d has the bytes B.  A hit is a pair (p, k) with B[p : p + len(s_k)] == s_k that lies entirely inside the document: a
 *   match that needs a byte of the next document is none, and neither is one that needs a byte behind n_bytes.
 *  Per document.  cut[d] = the least p over all hits, or len(B) without one.  hit[d] = the least k among the hits at p == cut[d], or
 *   0xFFFFFFFF without one: position decides before list order, and list order between "ab" and "abc" at one place.  The kept length
 *   is cut[d]; with TK_STOPS_KEEP and a hit, cut[d] + len(s_hit): the stop string that ends a document then belongs to it.
 *  Output.  text: the kept prefixes back to back; text_off uint64[n_docs + 1]; hit uint32[n_docs]; *n_hit_out: the documents with a hit.
 *   With *n_hit_out == 0 nothing is written: *d_text_out == d_bytes and *d_text_off_out == d_byte_off, the caller's own, as the repair
 *   hands them back with *n_replaced_out == 0; hit is made all the same.  n == 0, n_docs == 0 and n_bytes == 0 are legal.
 *  TK_VALUE_ERROR, before any output is written (a refused call leaves the previous result whole): more than 16 strings, an empty
 *   string, a string over 64 bytes, stop offsets that do not ascend from 0, an unknown flag, a misaligned pointer, and the repair's limits
 *   on n_bytes and byte_off (checked on the device before anything is indexed with them; the message names the first offending
 *   document).  No kernel reads outside [d_bytes, d_bytes + n_bytes + 16), whatever the offsets hold.
 * Order with the repair: search, cut, then repair.  For well-formed stop strings the order does not matter: a stop string starts with an
 *  ASCII byte or a lead byte, and no ill-formed unit before it can swallow that byte (a unit only ever accepts continuation bytes); its
 *  last char is complete, so the unit that ends it ends with it.  The repair of the bytes before a hit is therefore the same whether or
 *  not the hit and what follows is still there: repair(cut(B)) is the matching prefix of repair(B).  Under TK_U8_REPLACE, for stop strings
 *  that do not contain U+FFFD themselves, the cut is where str.find on the replaced text puts it.  The search IS on the bytes before the
 *  repair: under TK_U8_IGNORE, dropping a unit can join "ab" and "cd" around it into a "bc" that the text shows and the search never
 *  saw; and a stop string that contains U+FFFD matches the bytes EF BF BD of the input only, never a replaced unit.
 * In / out: d_bytes and d_byte_off as tk_utf8_repair_device takes them.  *d_text_out, *d_text_off_out, *d_hit_out: buffers of the core
 *  that belong to this entry alone, valid until the core's next stop-string call (this entry, tk_decode_rows_until_device,
 *  tk_decode_rows_until).  The input must not be this entry's own previous output.  Holds the core's mutex; `stream`: a hipStream_t or
 *  null (the core's); the call returns when the text is there.  One device per call: a group has no such entry.
 * Text that arrives piece by piece, the state carried between the calls: tk_stream_create below. */
#define TK_STOPS_KEEP 1u /* the stop string that ends a document belongs to it */
typedef struct {
    uint32_t n;           /* strings: 0 .. 16 */
    const uint8_t* blob;  /* the strings back to back (host memory) */
    const uint32_t* off;  /* uint32[n + 1], ascending from 0: string k is blob[off[k] : off[k + 1]]; may be null with n == 0 */
} tk_stops;
int tk_stop_text_device(tk_core* core, const void* d_bytes, uint64_t n_bytes, const void* d_byte_off, uint64_t n_docs, const tk_stops* stops, uint32_t flags,
                        void* stream, const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint32_t** d_hit_out,
                        uint64_t* n_hit_out);
/* tk_decode_rows_text_device / tk_decode_rows_text with stop strings.  The tk_decode_rows_device rule runs unchanged first -- begin, end,
 * stop ids, skip ids; its refusals and errors, TK_KEY_ERROR included, come first and unchanged --, each row's kept bytes are then a
 * document of the search above, and the cut text is repaired: mode TK_U8_REPLACE, TK_U8_IGNORE, or TK_U8_BYTES -- no repair, the cut bytes
 * as they are, *d_char_off_out and *d_repl_off_out null.  What lies behind a stop id is never searched; a stop string may be spelled
 * across a skipped id.  One more output, n_tok uint32[R]: the number of the row's kept tokens whose first byte lies before the end of
 * the kept text (before the repair) -- 0 for empty kept text; a token that the cut splits counts.  With empty skip lists begin[r] +
 * n_tok[r] is the column behind the last token used.  *d_hit_out and *d_n_tok_out are valid until the core's next stop-string call.
 * NOT built: that column under skip lists. */
#define TK_U8_BYTES 2u /* tk_decode_rows_until*: no repair */
int tk_decode_rows_until_device(tk_core* core, const void* d_ids, uint64_t n_rows, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end,
                                const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode, void* stream,
                                const uint32_t** d_tokens_out, const uint64_t** d_tok_off_out, const uint32_t** d_n_kept_out, const uint32_t** d_stop_col_out,
                                const uint8_t** d_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out, const uint64_t** d_repl_off_out,
                                const uint32_t** d_hit_out, const uint32_t** d_n_tok_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                                uint64_t* n_replaced_out, uint64_t* n_hit_out);
/* ... for a matrix in host memory: host arrays out, library-owned (tk_free); *char_off_out and *repl_off_out null under TK_U8_BYTES. */
int tk_decode_rows_until(tk_core* core, const void* ids, uint64_t n_rows, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end,
                         const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode, uint32_t** tokens_out, uint64_t** tok_off_out,
                         uint32_t** n_kept_out, uint32_t** stop_col_out, uint8_t** text_out, uint64_t** text_off_out, uint64_t** char_off_out,
                         uint64_t** repl_off_out, uint32_t** hit_out, uint32_t** n_tok_out, uint64_t* n_tokens_out, uint64_t* n_text_out,
                         uint64_t* n_replaced_out, uint64_t* n_hit_out);
/* Streaming decode: tk_decode_rows_until for rows that arrive a few ids per step.  A generation loop has one column per step, or a few
 * under speculative decoding; it must show text as it arrives, notice a stop string the moment it completes, and print neither half a
 * UTF-8 char nor the first half of "\n\nQuestion:".  A stream is n_rows row slots whose state lives in HBM; a step takes ids [n_rows, W]
 * and returns, per row, the text that became final.  Replaces nothing in the reference: it is the per-row incremental detokenizer of its
 * users' serving loops.
 * The rule.  A stream is created with a tk_drows_spec, a tk_stops set with its flag and a mode -- the arguments and limits of
 *  tk_decode_rows_until_device, refused the same way -- and w_max, 1 .. 64, the widest step.  Per row r: state[r] (0 live, 1 ended by a
 *  stop id, 2 ended by a stop string, 3 flushed), hit[r] as in tk_stop_text_device, tail[r]: at most 66 kept, decoded bytes that are not
 *  emitted yet and begin on a unit boundary of the row's text, and the running totals n_kept, n_text, n_chars.
 *  Step on ids [n_rows, W], element (r, c) at ids[r * ld + c], begin / end uint32[n_rows] or null.  A row whose state is not 0 emits
 *   nothing; none of its columns is read or judged, its begin and end neither.  For a live row:
 *   1. the tk_decode_rows_device row rule runs on its columns [begin, end): stop_col and the kept ids; a kept id without a decode entry is
 *      TK_KEY_ERROR with the reference's message, the row and the column; begin > end or end > W is TK_VALUE_ERROR;
 *   2. N = the bytes of the kept ids, B = tail ++ N;
 *   3. full hits are searched in B by the tk_stop_text_device rule, B the document: the least p wins, then the least k.  On a hit (p, k)
 *      the row emits B[:p] -- B[:p + len(s_k)] with TK_STOPS_KEEP -- repaired as the end of a document, takes state 2 and hit k; otherwise,
 *      if a stop id was found, it emits all of B, repaired as the end of a document, and takes state 1;
 *   4. otherwise it stays live.  e0 = the least p such that B[p:] is a non-empty proper prefix of a stop string, or len(B).  B is parsed
 *      into the units of tk_utf8_repair_device from offset 0, with one difference: a lead byte that has accepted every byte up to the end
 *      of B, fewer than L - 1 of them, is unfinished, not ill-formed; e1 = its offset, or len(B).  e = the greatest unit start <= min(e0,
 *      e1); under TK_U8_BYTES e = e0.  The row emits B[:e], repaired, and its new tail is B[e:]: at most 63 + 3 bytes.
 *  Flush (some rows, or all): a live row emits its tail repaired as the end of a document -- an unfinished char becomes U+FFFD under
 *   TK_U8_REPLACE -- and takes state 3.  Reset (some rows, or all): the slot is live again, its tail empty, its totals zero, its hit
 *   0xFFFFFFFF; continuous batching reuses slots this way.
 *  For every row, everything emitted, concatenated, equals what tk_decode_rows_until returns for the row made of all the live columns
 *   fed to it, up to and including the step that ended it (or the flush): bytes, hit and mode alike.  Columns fed afterwards do not exist
 *   for that row.  Why: (a) B[:e] ends on a unit boundary and no unit reaches back over one, so the repair of the pieces is the pieces of
 *   the repair.  (b) A hit cannot start in bytes already emitted: when those were emitted the hit was not complete, so B[p:] was a proper
 *   prefix of the string, e0 <= p held it back, and e <= e0.  (c) A hit that is found is final: another one at a lower position that
 *   would complete later needs columns of a later step, which the row, ended by this one, never consumes -- and every hit that lies inside
 *   this step's B takes part in this step's minimum.  (d) Without a hit nothing behind e0 is emitted, so a string that completes later is
 *   still whole in the tail.
 * Output of a step (and of a flush): text uint8[*n_text_out], the emitted pieces back to back; text_off and char_off uint64[n_rows + 1]
 *  (char_off null under TK_U8_BYTES); state and hit uint32[n_rows]: the rows' state and hit after the call.
 * tk_stream_create.  TK_VALUE_ERROR for what tk_decode_rows_until_device refuses in spec, stops, flags and mode; w_max outside 1 .. 64;
 *  more than 65536 rows; a vocabulary and w_max whose row buffer 66 + w_max * (the longest token's bytes) exceeds the 16000 bytes of LDS
 *  a row takes (the message says to use tk_decode_rows_until for such input).  TK_UNSUPPORTED where tk_decode_batch returns it.  The stream belongs to the core and must be destroyed before it; several
 *  streams per core are legal; every call of a stream holds the core's mutex.  The element type of the matrices is the spec's dtype flag
 *  until tk_stream_dtype names another.
 * tk_stream_step_device: d_ids, d_begin, d_end on the core's device.  *d_text_out .. *d_hit_out are buffers of the stream, valid until
 *  its next call.  W > w_max, ld < W, begin > end, end > W and TK_KEY_ERROR refuse the step: state, totals and the previous outputs stay
 *  whole (the row kernel writes into a second copy of the slots that the host swaps in on success).  No kernel reads outside the
 *  (n_rows - 1) * ld + W elements of the matrix, whatever begin and end hold.  Two launches per call, whatever n_rows, W and the data
 *  are (tk_k_stream_row, tk_k_stream_pack under tk_get_kernel_ms), and one wait.  W == 0 and n_rows == 0 are legal.
 * tk_stream_step: the matrix in host memory; tk_stream_fetch: the last accepted call's outputs as host arrays of the stream, valid until
 *  its next call; tk_stream_flush / tk_stream_reset: rows uint32[n_listed] in host memory, or null for all; a row at or beyond n_rows is
 *  TK_VALUE_ERROR.  tk_stream_rows: the slots' state, hit and totals into the caller's arrays of n_rows entries (each may be null).
 * NOT built: n_tok per step; token spans in streamed text; W > 64; a stream across several GPUs. */
typedef struct tk_stream tk_stream;
int tk_stream_create(tk_core* core, uint64_t n_rows, uint32_t w_max, const tk_drows_spec* spec, const tk_stops* stops, uint32_t stop_flags, uint32_t mode,
                     tk_stream** stream_out);
void tk_stream_destroy(tk_stream* stream);
int tk_stream_dtype(tk_stream* stream, uint32_t dtype_flags); /* 0 (uint32), TK_DROWS_I32 or TK_DROWS_I64: of the matrices from here on */
int tk_stream_step_device(tk_stream* stream, const void* d_ids, uint64_t width, uint64_t ld, const void* d_begin, const void* d_end, void* hip_stream,
                          const uint8_t** d_text_out, uint64_t* n_text_out, const uint64_t** d_text_off_out, const uint64_t** d_char_off_out,
                          const uint32_t** d_state_out, const uint32_t** d_hit_out);
int tk_stream_step(tk_stream* stream, const void* ids, uint64_t width, uint64_t ld, const uint32_t* begin, const uint32_t* end, const uint8_t** text_out,
                   uint64_t* n_text_out, const uint64_t** text_off_out, const uint64_t** char_off_out, const uint32_t** state_out, const uint32_t** hit_out);
int tk_stream_fetch(tk_stream* stream, const uint8_t** text_out, uint64_t* n_text_out, const uint64_t** text_off_out, const uint64_t** char_off_out,
                    const uint32_t** state_out, const uint32_t** hit_out);
int tk_stream_flush(tk_stream* stream, const uint32_t* rows, uint64_t n_listed, const uint8_t** text_out, uint64_t* n_text_out, const uint64_t** text_off_out,
                    const uint64_t** char_off_out, const uint32_t** state_out, const uint32_t** hit_out);
int tk_stream_reset(tk_stream* stream, const uint32_t* rows, uint64_t n_listed);
int tk_stream_rows(tk_stream* stream, uint32_t* state, uint32_t* hit, uint64_t* n_kept, uint64_t* n_text, uint64_t* n_chars);
/* bpe_train(data, vocab_size, pat_str, visualise=None)                    tiktoken/_educational.py:119-185
 * Training a vocabulary: the merges the reference's educational trainer makes on the same text -- the same pairs in the same order -- for a
 * packed batch of documents, under the core's pat_str (stock scanners or the generic engine).  The core's ranks and special tokens play
 * no part.  On success *pairs_out holds *n_out = vocab_size - 256 pairs {left, right} and *counts_out the count of each pair when it won
 * (both library-owned: tk_free); token 256 + k is the bytes of left followed by the bytes of right.  The rule:
 *  1. Words: the pieces the pre-tokeniser yields for every document, in document order, each as its UTF-8 bytes; a piece never crosses a
 *     document boundary, chars a generic pat_str leaves unmatched are no words.  Symbols 0..255 are the bytes, symbol 256 + k is merge k.
 *  2. Equal pieces are ONE word with a weight, the number of its occurrences (64-bit), and the byte offset of its first occurrence in the
 *     whole corpus (64-bit, across documents and chunks).  A symbol keeps, for its whole life, the offset of its first byte inside its
 *     word; a merged symbol keeps that of its left part.  A symbol's position is word offset + symbol offset: ascending positions are the
 *     order in which the reference's loop over its word list meets symbols first.
 *  3. A step counts every adjacent pair (a, b) inside words, each occurrence with its word's weight.  cmax = the largest count; the
 *     winner is the pair found at the smallest position among all positions whose pair has count cmax (= the reference's max() over a
 *     Counter: the first maximal key in insertion order, which is the order of first occurrence).  counts_out[k] = cmax of step k.
 *  4. In every word, from left to right, non-overlapping occurrences of the winner are replaced by the new symbol: for a == b a run of k
 *     equal symbols gives floor(k / 2) merges from the run's first symbol on and leaves a lone one at its end if k is odd.
 *  5. After vocab_size - 256 steps the call returns.  A step that finds no pair at all: TK_VALUE_ERROR (the reference raises ValueError
 *     from max() there).  vocab_size < 256: TK_VALUE_ERROR before anything runs; vocab_size == 256: no merges, *n_out = 0.
 *  6. NOT built: a merge that spells an existing token (two different pairs with the same concatenated bytes).  The reference overwrites
 *     the dict entry and runs one step more, which leaves ids with holes.  This call returns pairs, not byte strings, and knows nothing of
 *     spellings; whoever assembles the byte strings (tiktoken_amd.train.merges_to_ranks) refuses such a list with an error that names
 *     the two pairs instead of building the hole-ridden ids.
 * A corpus longer than the core's chunk size goes chunk by chunk, cut at document boundaries, into one word table, offsets kept global; a
 * single document longer than a chunk (at most 2 GiB): TK_VALUE_ERROR -- split it into documents.  More than 4 GiB of DISTINCT words:
 * TK_VALUE_ERROR.  The merge loop runs without a host wait; every step counts from scratch (tk_train.h).  Holds the core's mutex.  One
 * device per call, host text in: a device-resident entry and several devices are not built. */
int tk_train_bpe(tk_core* core, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, uint32_t vocab_size,
                 uint32_t** pairs_out /* n x {left, right} */, uint64_t** counts_out /* cmax of each step */, uint64_t* n_out);
/* CoreBPE.decode_single_token_bytes(token)  (pointer into the core; do not free)  src/py.rs:164-172 */
int tk_decode_single_token_bytes(tk_core* core, uint32_t token, const uint8_t** bytes_out, uint64_t* len_out);
/* CoreBPE.token_byte_values(): tokens in lexicographic byte order                  src/py.rs:178-183, lib.rs:648-650 */
uint64_t tk_n_tokens(tk_core* core);
int tk_sorted_token(tk_core* core, uint64_t i, const uint8_t** bytes_out, uint64_t* len_out, uint32_t* rank_out);
/* The same list in one call: packed bytes + n+1 offsets, owned by the core (valid until tk_destroy). */
int tk_sorted_tokens_packed(tk_core* core, const uint8_t** blob_out, const uint64_t** off_out, uint64_t* n_out);

/* Several GPUs of one node in one process: the batch is split by documents into contiguous ranges of about equal byte counts, every
 * core (one per device; created with tk_create) encodes its range from its own host thread, the token ids come back in document
 * order.  Replaces nothing in the reference (its scaling knob is the thread pool of tiktoken/core.py:175); BASELINE north_star:
 * "inputs shard by document across the GPUs of one node".  The group does not own the cores. */
typedef struct tk_group tk_group;
int tk_group_create(tk_core** cores, uint32_t n, tk_group** out);
void tk_group_destroy(tk_group* group);
uint32_t tk_group_size(tk_group* group);
/* same contract as tk_encode_batch */
int tk_group_encode_batch(tk_group* group, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                          const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                          uint64_t* tok_off_out);
/* ... checked (see tk_encode_batch_checked): every shard searches its own text; *hit is the hit with the lowest document index, in the
 * batch's document numbers */
int tk_group_encode_batch_checked(tk_group* group, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                  const uint32_t* allowed_ids, uint64_t n_allowed, uint32_t** tokens_out, uint64_t* n_tokens_out,
                                  uint64_t* tok_off_out, const uint32_t* disallowed_ids, uint64_t n_disallowed, tk_special_hit* hit);
/* Results gathered on the first core's device; only the text crosses PCIe (every shard's ids stay on its device until the gather).
 * The gather is ONE exchange over xGMI: grouped ncclSend / ncclRecv through RCCL (rccl.h:700-722, loaded on first use) when the
 * group's devices are pairwise distinct, concurrent peer copies (one stream per source device) when a device is named twice or
 * RCCL cannot be loaded ($TIKTOKEN_AMD_NO_RCCL forces the latter).  The pointers are owned by the group (valid until its next call). */
int tk_group_encode_batch_device(tk_group* group, const uint8_t* utf8, const uint64_t* doc_off, uint64_t n_docs, int use_special,
                                 const uint32_t* allowed_ids, uint64_t n_allowed, const uint32_t** d_tokens_out, uint64_t* n_tokens_out,
                                 const uint64_t** d_tok_off_out);
/* "gathers_rccl" / "gathers_peer": how many device gathers of this group ran on RCCL / on peer copies */
uint64_t tk_group_stat(tk_group* group, const char* name);

/* Vocabulary wire format: the text of a `.tiktoken` file (`base64(token) SP rank` per line) -> the packed arrays tk_create takes.
 * Replaces the per-line Python loop of tiktoken/load.py:159-171, and reads what that loop reads: lines ending in \n, \r or \r\n, two fields
 * between runs of ASCII white space, base64 as b64decode() takes it without validation (bytes outside the alphabet skipped, anything behind
 * the padding ignored), the rank as int() takes it (sign, underscores between digits).  Release the three arrays with tk_free.
 * TK_VALUE_ERROR with "Error parsing line N ..." on malformed input, and on a rank that is negative or does not fit 32 bits (where the
 * reference fails one step later, in CoreBPE's constructor). */
int tk_parse_tiktoken_bpe(const uint8_t* text, uint64_t len, uint8_t** blob_out, uint64_t** off_out, uint32_t** ids_out, uint64_t* n_out);

/* The reference's text boundary is &str -- valid UTF-8 by construction (PyO3 extracts it, src/py.rs:29).  A C caller has bytes: 0 if
 * utf8[0..len) is well-formed UTF-8 (no overlong forms, no surrogates, nothing above U+10FFFF, no truncated char), else TK_VALUE_ERROR
 * with *bad_pos (may be null) = offset of the first byte that is not part of a well-formed char.  Host code; a few GB/s. */
int tk_validate_utf8(const uint8_t* utf8, uint64_t len, uint64_t* bad_pos);

void tk_free(void* p);

/* tk_encode_batch_device alternates between n (1 or 2; default 1) pairs of result buffers: with 2 the ids and offsets of call k stay valid
 * while call k + 1 runs, so a consumer on another stream -- the RCCL send of a shard's ids to the root rank (tiktoken_amd/distributed.py) --
 * overlaps the next encode without a copy of its own.  No reference counterpart (the reference returns owned Vec<u32>s, src/lib.rs:360). */
int tk_set_output_buffers(tk_core* core, uint32_t n);

/* Instrumentation for bench.py: when enabled, every kernel launch of the next encode call is
 * bracketed by HIP events on the stream it runs on; tk_get_kernel_ms returns the summed
 * duration and launch count per kernel name since the last tk_reset_kernel_ms. */
void tk_set_profiling(tk_core* core, int enabled);
void tk_reset_kernel_ms(tk_core* core);
int tk_get_kernel_ms(tk_core* core, const char* kernel_name, double* ms_out, uint64_t* launches_out);
/* Pieces / tokens / bytes handled by the last encode call (for roofline accounting). */
void tk_last_stats(tk_core* core, uint64_t* n_bytes, uint64_t* n_pieces, uint64_t* n_tokens, uint64_t* n_docs,
                   uint64_t* n_medium, uint64_t* n_long);
/* One named figure of the last encode call; 0 for a name it does not know: "chunks", "small_launches", "small_calls", "mid_calls",
 * "back_streams", "regrown", "workspace_bytes", "front_wgs_per_cu", "compute_units", "spec_find_launches" (launches of the disallowed scan since
 * the core was made: one per chunk of a _checked call), "spec_mark_launches" (launches of the pair of kernels that marks allowed special tokens
 * since the core was made: one per chunk encoded with an allowed set), "stage_bytes" (host-buffer batches of twice that many bytes and more are pipelined),
 * "train_table_moves" / "train_blob_moves" (of the last tk_train_bpe: how often the word table was rehashed into a larger one, and how often
 * the distinct words' bytes were copied into a larger blob; both 0 for a corpus of one chunk); and of the core itself, by its vocabulary's ids:
 * "pair_table_packed" (1: every rank fits the packed pair table; 0: 16-byte slots and a merge kernel per length bin), "short_table" (0: an id
 * above 0x3FFFFFFE, tokens of 1 .. 4 bytes live in the mid table), "decode_table_ids" (entries of the device decode table; 0: an id of 2^26
 * or above, the decode entries answer TK_UNSUPPORTED); and of the last split call (tk_split_device, tk_encode_batch_split): "split_segments"
 * (document parts per block of K positions), "split_joined" (blocks in which the true chain met the speculative walk), "split_stitch_steps"
 * (steps of the stitch pass) and "split_spec_steps" (steps of the speculative walks); "jsonl_tile": the bytes of a tile of the JSON Lines
 * passes (a constant of the build); "fingerprint_tile": the token positions of a tile of the fingerprint pass (likewise). */
uint64_t tk_stat(tk_core* core, const char* name);

#ifdef __cplusplus
}
#endif
#endif
