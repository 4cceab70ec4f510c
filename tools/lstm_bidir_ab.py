"""Both directions of the LSTM recurrence in shared launches (dirs = 3) against two back-to-back one-direction
calls of the same kernel family (the length-aware entries at full lengths, so H = 512 is per-step on both
sides), forward + backward, timed with HIP events at XceptionLSTMV's shape (B 16, T 16, H 128) and
XceptionLSTMA's (B 16, T 120, H 512).  The two forms alternate inside every round; the figure is the median
over the rounds of a window of `iters` calls after a warm-up.  The x-projection and weight-gradient GEMMs are
the same work either way and are not in the window.

usage: python tools/lstm_bidir_ab.py [rounds]
"""
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]
from xcp import ops  # noqa: E402


def timeit(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    dev = torch.device("cuda:0")
    ops._lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    for (B, T, H, iters) in ((16, 16, 128, 200), (16, 120, 512, 20)):
        G4 = 4 * H
        f = dict(device=dev)
        xp = torch.randn(2, B * T, G4, generator=g, **f)
        whh = torch.randn(2, G4, H, generator=g, **f) / H ** 0.5
        bih, bhh = torch.zeros(2, G4, **f), torch.zeros(2, G4, **f)
        full = torch.full((B,), T, dtype=torch.int32, device=dev)
        # dirs = 3: stacked state, interleaved out
        out2, dout2 = torch.empty(B, T, 2 * H, **f), torch.randn(B, T, 2 * H, generator=g, **f)
        hp2, cs2 = torch.empty(2, B, T, H, **f), torch.empty(2, B, T, H, **f)
        gt2, dg2 = torch.empty(2, B * T, G4, **f), torch.empty(2, B * T, G4, **f)
        hn2, cn2 = torch.empty(2, B, H, **f), torch.empty(2, B, H, **f)
        # two one-direction calls: per-direction tensors
        out1 = [torch.empty(B, T, H, **f) for _ in range(2)]
        dout1 = [dout2[..., d * H:(d + 1) * H].contiguous() for d in range(2)]
        hn1, cn1 = torch.empty(2, B, H, **f), torch.empty(2, B, H, **f)

        def both():
            ops.lstm_fwd_dir(xp, whh, None, bih, bhh, out2, hp2, cs2, gt2, hn2, cn2, B, T, H, 3, 0, full)
            ops.lstm_bwd_dir(dout2, None, None, whh, cs2, gt2, dg2, B, T, H, 3, 0, full)

        def twice():
            for d in range(2):
                ops.lstm_fwd(xp[d], whh[d], None, bih[d], bhh[d], out1[d], hp2[d], cs2[d], gt2[d], hn1[d], cn1[d], B, T,
                             H, 0, full)
            for d in range(2):
                ops.lstm_bwd(dout1[d], None, None, whh[d], cs2[d], gt2[d], dg2[d], B, T, H, 0, full)

        t = {"both": [], "twice": []}
        for _ in range(rounds):
            t["twice"].append(timeit(twice, iters))
            t["both"].append(timeit(both, iters))
        a, b = statistics.median(t["twice"]), statistics.median(t["both"])
        sp = lambda v: f"[{min(v):.1f} .. {max(v):.1f}]"   # noqa: E731
        print(f"B={B} T={T} H={H} fwd+bwd, {rounds} rounds x {iters} calls: two one-direction calls {a:9.1f} us "
              f"{sp(t['twice'])}   dirs=3 {b:9.1f} us {sp(t['both'])}   ratio {b / a:.3f}", flush=True)


if __name__ == "__main__":
    main()
