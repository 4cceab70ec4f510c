"""Measurements for the class-activation maps (HIP events, MI355X); writes profiles/gradcam.txt's timing section.

1. The clip model at the bench shape (XceptionLSTMV, 16 clips x 16 frames x 299^2, bf16): xcp.grad_cam at "exit"
   (no backbone backward) and at "block11" (the 19^2 maps; the backward stops after the exit flow and block12),
   beside the eval-mode scoring forward and xcp.input_gradient (a whole backbone backward) in the same process.
2. The two kernels alone at those shapes: us per launch and achieved bytes/s for their algorithmic bytes (A and G
   read once, the raw map written; the raw map read, the heat map written), beside xcp_stream_copy moving the
   same number of bytes (half read, half written).

usage: python tools/cam_bench.py [out-file]   (default: standard output only)
"""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]

import xcp  # noqa: E402
from xcp import _lib, ops  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timeit(fn, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]   # ms: median, min, max


def clip_model(dev):
    from Models.XceptionLSTMV import XceptionLSTMV
    B, T, S = 16, 16, 299
    torch.manual_seed(0)
    m = XceptionLSTMV(128, pretrained=False).to(dev).eval()
    x = torch.rand(B, T, 3, S, S, device=dev)
    say(f"XceptionLSTMV(128), {B} clips x {T} frames x {S}^2, bf16 backbone, eval mode; ms per call, median of 10 "
        "(min, max), device events, 3 warm-ups")

    def score():
        with torch.no_grad():
            return m(m.extract_features(x))

    with xcp.precision("bf16"):
        for name, fn in (("eval scoring forward (extract_features + head)", score),
                         ('xcp.grad_cam, layer "exit" (10^2 maps, no backbone backward)', lambda: xcp.grad_cam(m, x)),
                         ('xcp.grad_cam, layer "block11" (19^2 maps, 2 of 14 backward stages)',
                          lambda: xcp.grad_cam(m, x, layer="block11")),
                         ('xcp.grad_cam, layer "block11", hirescam', lambda: xcp.grad_cam(m, x, layer="block11", method="hirescam")),
                         ("xcp.frame_relevance", lambda: xcp.frame_relevance(m, x)),
                         ("xcp.input_gradient (whole backbone backward)", lambda: xcp.input_gradient(m, x))):
            med, lo, hi = timeit(fn)
            say(f"  {name:72s} {med:8.2f}  ({lo:.2f}, {hi:.2f})")


def copy_rate(dev, nbytes):
    """xcp_stream_copy moving nbytes in all (half in, half out), rounded up to its 16 KiB granule"""
    n16 = max(1024, (nbytes // 2 // 16 + 1023) // 1024 * 1024)
    a = torch.empty(n16 * 16, device=dev, dtype=torch.uint8)
    b = torch.empty_like(a)
    med, _, _ = timeit(lambda: _lib.call("xcp_stream_copy", a.data_ptr(), b.data_ptr(), n16, ops.stream()), iters=20)
    return med, 2 * n16 * 16


def kernels(dev):
    say()
    say("the kernels alone, 256 frames, bf16; us per launch (median of 20) and achieved bytes/s on the algorithmic "
        "bytes; xcp_stream_copy on the same number of bytes beside it")
    g = torch.Generator(device=dev).manual_seed(0)

    def line(name, ms, byts):
        cms, cb = copy_rate(dev, byts)
        say(f"  {name:64s} {ms * 1e3:8.1f} us  {byts / 1e6:8.1f} MB  {byts / ms / 1e9:6.2f} TB/s   "
            f"(copy: {cms * 1e3:7.1f} us, {cb / cms / 1e9:5.2f} TB/s)")

    N = 256
    for tag, HW, C, CP in (("exit 10^2 x 2048", 100, 2048, 2048), ("block11 19^2 x 728 (pitch 736)", 361, 728, 736)):
        A = torch.randn(N, HW, CP, device=dev, generator=g).bfloat16()
        G = torch.randn(N, HW, CP, device=dev, generator=g).bfloat16()
        al = torch.randn(N, C, device=dev, generator=g)
        sc, sh = torch.randn(C, device=dev, generator=g), torch.randn(C, device=dev, generator=g)
        one = N * HW * CP * 2
        t, _, _ = timeit(lambda: ops.cam(A, N, HW, C, CP, alpha=al, a_scale=sc, a_shift=sh), iters=20)
        line(f"xcp_cam {tag}, alpha given, BN + ReLU on load", t, one + N * HW * 4)
        t, _, _ = timeit(lambda: ops.cam(A, N, HW, C, CP, G=G), iters=20)
        line(f"xcp_cam {tag}, gradcam, alpha from G", t, 2 * one + N * HW * 4)
        t, _, _ = timeit(lambda: ops.cam(A, N, HW, C, CP, G=G, mode=1), iters=20)
        line(f"xcp_cam {tag}, hirescam", t, 2 * one + N * HW * 4)
    for h in (10, 19):
        raw = torch.randn(16, 16, h, h, device=dev, generator=g)
        t, _, _ = timeit(lambda: ops.cam_render(raw, (299, 299)), iters=20)
        line(f"xcp_cam_render {h}^2 -> 299^2, normalize", t, N * (h * h + 299 * 299) * 4)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("cam_bench needs the GPU (there is no CPU timing)")
    dev = torch.device("cuda:0")
    _lib.load()
    with torch.cuda.device(dev):
        clip_model(dev)
        kernels(dev)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
