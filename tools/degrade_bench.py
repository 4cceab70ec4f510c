"""Measurements for the clip degradation (HIP events, MI355X); writes profiles/degrade.txt's timing section.

xcp_clip_degrade at the bench batch (16 clips x 16 frames x 256^2 uint8) with JPEG alone, blur (R = 4) alone,
noise alone and all three, beside
  (a) a device copy of the same bytes in and out,
  (b) the same stages composed from stock torch ops on the same device tensors (fp32: depthwise conv2d on a
      reflect-padded clip, randn noise, a matrix DCT as two matmuls per direction on 8 x 8 blocks, avg_pool2d
      and bilinear interpolate for the chroma), which computes a float approximation of the same pictures,
  (c) the 36 ms headline training step (README).
The kernel's output at this frame size is first compared byte for byte with degrade_reference on one clip.

usage: python tools/degrade_bench.py [out-file]   (default: standard output only)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]

from xcp import _lib, ops  # noqa: E402
from xcp.degrade import CHROMA_Q, DCT_C, LUMA_Q, DegradeParams, degrade_reference, gaussian_taps, quant_table  # noqa: E402

LINES = []
B, T, S = 16, 16, 256
HEADLINE_MS = 36.0
CONFIGS = (("identity (copy through the kernel)", dict()),
           ("JPEG q = 75", dict(quality=75)),
           ("blur sigma 1.3 (R = 4)", dict(sigma=1.3)),
           ("noise sigma 8", dict(noise=8.0)),
           ("blur + noise + JPEG", dict(quality=75, sigma=1.3, noise=8.0)))


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timeit(fn, iters=20, warm=5):
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


def frames(dev):
    """Smooth structure plus noise, as the tests' frames (a flat or a purely random clip quantises untypically)."""
    g = torch.Generator(device=dev).manual_seed(0)
    y = torch.arange(S, device=dev, dtype=torch.float32).view(1, 1, S, 1, 1)
    x = torch.arange(S, device=dev, dtype=torch.float32).view(1, 1, 1, S, 1)
    ph = 6.28 * torch.rand((B, T, 1, 1, 3), device=dev, generator=g)
    v = 128 + 0.3 * (y - S / 2) - 0.2 * (x - S / 2) + 60 * torch.sin(0.11 * y + 0.07 * x + ph)
    v = v + 12 * torch.randn((B, T, S, S, 3), device=dev, generator=g)
    return v.round().clamp(0, 255).to(torch.uint8)


class Stock:
    """The three stages in stock torch ops, fp32, on [N, 3, H, W] planes."""

    def __init__(self, dev, quality, sigma, noise):
        self.q, self.noise = quality, noise
        R, w = gaussian_taps(sigma)
        self.R = R
        if R:
            k = torch.tensor([w[abs(i)] for i in range(-R, R + 1)], dtype=torch.float32, device=dev) / 2048
            self.kx, self.ky = k.view(1, 1, 1, -1).repeat(3, 1, 1, 1), k.view(1, 1, -1, 1).repeat(3, 1, 1, 1)
        self.C = torch.tensor(DCT_C / 4096.0, dtype=torch.float32, device=dev)
        if quality:
            self.QL = torch.tensor(quant_table(LUMA_Q, quality), dtype=torch.float32, device=dev)
            self.QC = torch.tensor(quant_table(CHROMA_Q, quality), dtype=torch.float32, device=dev)
        self.rgb2ycc = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]],
                                    device=dev)

    def codec(self, p, Q):
        n, h, w = p.shape
        b = (p - 128).view(n, h // 8, 8, w // 8, 8).permute(0, 1, 3, 2, 4)
        f = self.C @ b @ self.C.t()
        f = torch.round(f / Q) * Q
        r = self.C.t() @ f @ self.C
        return (r + 128).round().clamp(0, 255).permute(0, 1, 3, 2, 4).reshape(n, h, w)

    def __call__(self, u8):
        x = u8.view(-1, S, S, 3).permute(0, 3, 1, 2).float()
        if self.R:
            x = F.conv2d(F.pad(x, (self.R, self.R, 0, 0), mode="reflect"), self.kx, groups=3)
            x = F.conv2d(F.pad(x, (0, 0, self.R, self.R), mode="reflect"), self.ky, groups=3).round()
        if self.noise:
            x = (x + self.noise * torch.randn_like(x)).round().clamp(0, 255)
        if self.q:
            ycc = torch.einsum("kc,nchw->nkhw", self.rgb2ycc, x)
            Y = self.codec(ycc[:, 0].round(), self.QL)
            c = F.avg_pool2d(ycc[:, 1:] + 128, 2).round()
            c = torch.stack([self.codec(c[:, 0], self.QC), self.codec(c[:, 1], self.QC)], 1)
            c = F.interpolate(c, scale_factor=2, mode="bilinear", align_corners=False) - 128
            x = torch.stack([Y + 1.402 * c[:, 1], Y - 0.344136 * c[:, 0] - 0.714136 * c[:, 1], Y + 1.772 * c[:, 0]], 1)
            x = x.round().clamp(0, 255)
        return x.to(torch.uint8).permute(0, 2, 3, 1).reshape(u8.shape)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("degrade_bench needs the GPU (there is no CPU timing)")
    dev = torch.device("cuda:0")
    _lib.load()
    with torch.cuda.device(dev):
        u8 = frames(dev)
        lengths = torch.full((B,), T, dtype=torch.int32, device=dev)
        out = torch.empty_like(u8)
        nbytes = u8.numel()
        # the kernel's result at this frame size, on one clip of two frames
        one = DegradeParams.fixed(1, quality=75, sigma=1.3, noise=8.0, seed=3)
        got = ops.clip_degrade(u8[:1, :2].contiguous(), lengths[:1].clamp(max=2), one).cpu()
        same = torch.equal(got, degrade_reference(u8[:1, :2].cpu(), [2], one))
        say(f"xcp_clip_degrade, {B} clips x {T} frames x {S}^2 x 3 uint8 = {nbytes / 1e6:.1f} MB in, as much out; ms per "
            "call, median of 20 (min, max), device events, 5 warm-ups, three rounds")
        say(f"byte for byte degrade_reference on one clip of two {S}^2 frames, all three stages: {same}")
        if not same:
            raise SystemExit("the kernel disagrees with degrade_reference")
        copy = []
        for _ in range(3):
            copy.append(timeit(lambda: out.copy_(u8)))
        cm = float(np.median([c[0] for c in copy]))
        say(f"  (a) device copy of the same bytes (Tensor.copy_): {', '.join(f'{c[0]:.3f}' for c in copy)} ms "
            f"= {2 * nbytes / cm / 1e9:.2f} TB/s read + written")
        say()
        say(f"  {'stages':36s} {'xcp ms (three rounds)':>30s} {'min':>7s} {'x copy':>7s} {'stock ms':>9s} {'xcp/stock':>9s} "
            f"{'% of the ' + format(HEADLINE_MS, 'g') + ' ms step':>20s}")
        for name, kw in CONFIGS:
            tab = DegradeParams.fixed(B, seed=1, **kw).to(dev)
            stock = Stock(dev, kw.get("quality", 0), kw.get("sigma", 0.0), kw.get("noise", 0.0))
            xs, ss = [], []
            for _ in range(3):   # the two paths alternating
                xs.append(timeit(lambda: ops.clip_degrade(u8, lengths, tab, out=out)))
                ss.append(timeit(lambda: stock(u8), iters=5, warm=2))
            xm, sm = float(np.median([v[0] for v in xs])), float(np.median([v[0] for v in ss]))
            say(f"  {name:36s} {', '.join(f'{v[0]:.3f}' for v in xs):>30s} {min(v[1] for v in xs):7.3f} {xm / cm:7.1f} "
                f"{sm:9.2f} {xm / sm:9.3f} {100 * xm / HEADLINE_MS:19.1f}%")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
