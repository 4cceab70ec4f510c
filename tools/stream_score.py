"""Scoring 300-frame clips in chunks (xcp.score_in_chunks): frames/s and peak memory per chunk size (MI355X).

XceptionLSTMV(128), eval, bf16 compute, B clips of 300 frames of 299^2.  For chunk sizes 8 / 16 / 32 the whole
clip is scored with the LSTM state carried from chunk to chunk; for comparison the unchunked call
(extract_features over all B*T frames, then the model) at the largest T that fits: in memory, and in the 256
frames per backbone pass that the benchmark and the suite exercise the kernels' index arithmetic at (B*T <= 256;
halved while the call runs out of memory).  Each line: frames/s (one timed call after one warm-up, HIP events)
and torch.cuda.max_memory_allocated of the timed call (the clips themselves included: fp32, 643 MB at 2 x 300).
Records, not thresholds.

Every measurement runs in a child process of its own under its own time limit; after a child that was killed
by a signal or its time limit nothing more is started.

usage: python tools/stream_score.py [--clips B] [--out profiles/lstm_state_stream.txt]
"""
import argparse
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]

FRAMES, SIZE = 300, 299
MAX_FRAMES = 256                         # frames per backbone pass of the unchunked call (bench.py's 16 x 16)
LIMIT = 240                              # seconds per child
OOM = 3                                  # a child's exit status for "does not fit"


def child(mode, n, clips_n):
    import torch

    import xcp
    from Models.XceptionLSTMV import XceptionLSTMV
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = XceptionLSTMV(128, pretrained=False).to(dev).eval()
    T = FRAMES if mode == "chunk" else n
    clips = torch.rand((clips_n, T, 3, SIZE, SIZE), device=dev)
    lens = torch.full((clips_n,), T, device=dev)

    def run():
        with torch.no_grad(), xcp.precision("bf16"):
            if mode == "chunk":
                return xcp.score_in_chunks(m, clips, lens, chunk=n)
            return m(m.extract_features(clips), lens)

    try:
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        prob = run()
        e.record()
        torch.cuda.synchronize()
    except torch.OutOfMemoryError:
        print(f"{mode} {n}: out of memory", flush=True)
        return OOM
    ms = s.elapsed_time(e)
    what = f"chunk {n:3d}, T {T}" if mode == "chunk" else f"unchunked, T {T}"
    print(f"{what:22s} {clips_n} clips: {clips_n * T / ms * 1e3:8.1f} frames/s, {ms:8.1f} ms, "
          f"peak {torch.cuda.max_memory_allocated() / 2 ** 20:9.1f} MiB, mean prob {float(prob.mean()):.4f}", flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lstm_state_stream.txt"))
    ap.add_argument("--child", nargs=2, metavar=("MODE", "N"))
    a = ap.parse_args()
    if a.child:
        sys.exit(child(a.child[0], int(a.child[1]), a.clips))
    lines = [f"tools/stream_score.py: XceptionLSTMV(128), eval, bf16, {a.clips} clips x {FRAMES} frames x {SIZE}^2"]

    def one(mode, n):
        """0 done, OOM does not fit, None: stop (killed, timed out or failed)"""
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--clips", str(a.clips), "--child", mode,
                                str(n)], capture_output=True, text=True, timeout=LIMIT)
        except subprocess.TimeoutExpired:
            lines.append(f"{mode} {n}: no result within {LIMIT} s; stopping")
            return None
        lines.extend(r.stdout.strip().splitlines())
        if r.returncode not in (0, OOM):
            lines.append(f"{mode} {n}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}")
            return None
        return r.returncode

    ok = True
    for n in (8, 16, 32):
        if one("chunk", n) is None:
            ok = False
            break
    if ok:
        t = min(FRAMES, MAX_FRAMES // a.clips)
        while t >= 1:
            rc = one("whole", t)
            if rc is None:
                ok = False
            if rc != OOM:
                break
            t //= 2
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
