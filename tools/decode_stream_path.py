"""Time per step of a decode stream (Encoding.decode_stream) on the GPU, beside the two routes a generation loop has without it:
(a) tk_decode_rows_until_device on the step's [R, W] slice alone -- cheaper to call than it is correct (a char or a stop string that
    straddles a step is lost), so it is the cost to beat, not an answer to match;
(b) the host route: the slice copied out, then a per-row incremental detokenizer in Python (decode_single_token_bytes, find, an
    incomplete-char check).
Shaped o200k vocabulary, four stop strings, ids on the device, R in (256, 4096), W in (1, 4).  Every call ends in a wait of the host, so a
host clock around a run of steps measures them; each route is warmed up on the shapes it is timed on, the routes take turns, and the
median over the turns is reported with the spread.  Kernel times come from a profiled run of their own (tk_get_kernel_ms).
Usage: python tools/decode_stream_path.py [out.txt]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tiktoken_amd  # noqa: E402

STOPS = ["\n\nQuestion:", "</answer>", "###", "<|user|>"]
STEPS, TURNS = 64, 5


def incomplete(buf: bytes) -> int:
    """bytes at the end of buf that are the start of an unfinished char"""
    for back in (1, 2, 3):
        if back > len(buf):
            break
        b = buf[-back]
        if b >= 0xC0:
            need = 2 if b < 0xE0 else 3 if b < 0xF0 else 4
            return back if need > back else 0
        if b < 0x80:
            break
    return 0


def host_route(enc, ids_host, tails, done, stops_b, longest):
    out = []
    for r, row in enumerate(ids_host):
        if done[r]:
            out.append("")
            continue
        buf = tails[r] + b"".join(enc.decode_single_token_bytes(int(t)) for t in row)
        at = min((p for p in (buf.find(s) for s in stops_b) if p >= 0), default=-1)
        if at >= 0:
            done[r], tails[r] = True, b""
            out.append(buf[:at].decode("utf-8", "replace"))
            continue
        hold = 0
        for n in range(min(longest - 1, len(buf)), 0, -1):
            if any(s.startswith(buf[-n:]) for s in stops_b):
                hold = n
                break
        cut = len(buf) - hold
        cut -= incomplete(buf[:cut])
        tails[r] = buf[cut:]
        out.append(buf[:cut].decode("utf-8", "replace"))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    enc = tiktoken_amd.get_encoding("o200k_shaped")
    core = enc._core_bpe
    rng = np.random.default_rng(0x57)
    text = "The quick brown fox jumps over the lazy dog. naïve café 中文 😀 x = y + z; 1234\n"
    base = np.array(enc.encode_ordinary(text * 8), np.int64)
    stops_b = [s.encode() for s in STOPS]
    lines = [f"decode_stream: time per step, {STEPS} steps per run, median of {TURNS} turns (min .. max), o200k_shaped, {len(STOPS)} stop strings, ids on the device"]
    for R in (256, 4096):
        for W in (1, 4):
            T = STEPS * W
            m = base[(rng.integers(0, len(base) - T, size=R)[:, None] + np.arange(T)[None, :])]
            dev = torch.from_numpy(m).cuda()
            torch.cuda.synchronize()
            times = {"stream": [], "(a) one-shot on the slice": [], "(b) host route": []}

            def run_stream():
                with enc.decode_stream(R, STOPS, w_max=W) as s:
                    n = s._native
                    t0 = time.perf_counter()
                    for k in range(STEPS):
                        n._set_dtype(np.int64)
                        out, refs = n._outs()
                        core._L.tk_stream_step_device(n._h, dev.data_ptr() + 8 * k * W, W, T, None, None, None, *refs)
                    return (time.perf_counter() - t0) / STEPS

            def run_one_shot():
                t0 = time.perf_counter()
                for k in range(STEPS):
                    core.decode_rows_until_device(dev.data_ptr() + 8 * k * W, R, W, T, stop_text=STOPS, dtype=np.int64)
                return (time.perf_counter() - t0) / STEPS

            def run_host():
                tails, done = [b""] * R, [False] * R
                steps = 8  # (a Python loop over the rows: fewer steps tell as much)
                t0 = time.perf_counter()
                for k in range(steps):
                    host_route(enc, dev[:, k * W:(k + 1) * W].cpu().numpy(), tails, done, stops_b, max(map(len, stops_b)))
                return (time.perf_counter() - t0) / steps

            routes = {"stream": run_stream, "(a) one-shot on the slice": run_one_shot, "(b) host route": run_host}
            for f in routes.values():
                f()  # warm-up on this shape
            for _ in range(TURNS):
                for name, f in routes.items():
                    times[name].append(f() * 1e3)
            core.set_profiling(True)
            core.reset_kernel_ms()
            run_stream()
            k_row, k_pack = core.kernel_ms("tk_k_stream_row"), core.kernel_ms("tk_k_stream_pack")
            core.reset_kernel_ms()
            run_one_shot()
            one_shot_launches = sum(core.kernel_ms(k)[1] for k in ("tk_k_drows_stop", "tk_k_drows_count", "tk_k_drows_scan", "tk_k_drows_rows", "tk_k_drows_write", "tk_k_dec_len",
                                                                   "tk_k_dec_copy", "tk_k_u8r_check", "tk_k_stops_find", "tk_k_stops_rows", "tk_k_stops_scan", "tk_k_stops_docs",
                                                                   "tk_k_stops_cut", "tk_k_stops_ntok", "tk_k_span_mark", "tk_k_u8r_count", "tk_k_u8r_scan", "tk_k_u8r_docs",
                                                                   "tk_k_u8r_write"))
            core.set_profiling(False)
            lines.append(f"R = {R}, W = {W}:")
            for name, v in times.items():
                lines.append(f"  {name:28s} {statistics.median(v):9.4f} ms/step  ({min(v):.4f} .. {max(v):.4f})")
            lines.append(f"  kernels per step (profiled run): tk_k_stream_row {k_row[0] / STEPS:.4f} ms, tk_k_stream_pack {k_pack[0] / STEPS:.4f} ms, "
                         f"{(k_row[1] + k_pack[1]) // STEPS} timed launches; the one-shot route: {one_shot_launches // STEPS} timed launches")
    report = "\n".join(lines)
    print(report)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
