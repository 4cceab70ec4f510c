"""Measurements for the conv1 data gradient and the frozen-statistics backward (HIP events, MI355X).

1. xcp_conv1_dgrad_bn alone at the bench's stem shape (256 x 299^2, bf16): us per launch and the fraction of
   8 TB/s for its algorithmic bytes (dZ and Y read once, dX written once), beside the plain kernel on a stored
   dC1 and the yardstick: xcp_bn_bwd_apply followed by ATen's torch.nn.grad.conv2d_input on the same shape.
2. The backbone step (forward + backward of XceptionLSTMV, 16 clips x 16 frames x 299^2, bf16, parameters
   unfrozen, no optimiser) in train mode, on frozen statistics, and on frozen statistics with the frames'
   gradient -- for information: the frozen-statistics step did not run before this kernel existed.

usage: python tools/input_grad_bench.py [kernel] [step]   (default: both)
"""
import os
import sys

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]

import xcp  # noqa: E402
from xcp import ops  # noqa: E402
from xcp.engine import Stats  # noqa: E402

HBM = 8e12   # B/s (MI355X_MICROARCH.md)


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters   # ms


def kernel(dev):
    N, IH, IW = 256, 299, 299
    OH, OW = (IH - 3) // 2 + 1, (IW - 3) // 2 + 1
    rows = N * OH * OW
    g = torch.Generator(device=dev).manual_seed(0)
    dz = torch.randn(rows, 32, device=dev, generator=g).bfloat16()
    y = torch.randn(rows, 32, device=dev, generator=g).bfloat16()
    w = torch.randn(32, 3, 3, 3, device=dev, generator=g) * 0.2
    coef = torch.randn(96, device=dev, generator=g)
    st = Stats(32, dev)
    st.scale.copy_(torch.randn(32, device=dev, generator=g))
    st.shift.copy_(torch.randn(32, device=dev, generator=g))
    dc1 = torch.empty_like(dz)
    dx = torch.empty(N, 3, IH, IW, device=dev)
    in_b, out_b = rows * 32 * 2, N * 3 * IH * IW * 4
    print(f"conv1 data gradient, {N} x {IH} x {IW}, bf16; algorithmic bytes: fused {(2 * in_b + out_b) / 1e9:.3f} GB, "
          f"plain {(in_b + out_b) / 1e9:.3f} GB")

    def line(name, ms, byts=None):
        s = f"  {name:58s} {ms * 1e3:9.1f} us"
        if byts:
            s += f"  {byts / ms / 1e9:7.2f} TB/s = {100 * byts / (ms * 1e-3) / HBM:5.1f} % of 8 TB/s"
        print(s, flush=True)

    t_f = timeit(lambda: ops.conv1_dgrad_bn(dz, y, w, coef, st, dx, N, IH, IW, 32, relu=True))
    line("xcp_conv1_dgrad_bn (BN apply + ReLU mask on load)", t_f, 2 * in_b + out_b)
    t_a = timeit(lambda: ops.bn_apply_coef(dz, y, dc1, coef, st, rows, 32, True))
    line("xcp_bn_bwd_apply (stores dC1)", t_a, 3 * in_b)
    t_p = timeit(lambda: ops.conv1_dgrad(dc1, w, dx, N, IH, IW))
    line("xcp_conv1_dgrad (plain, stored dC1)", t_p, in_b + out_b)
    line("  apply + plain", t_a + t_p)
    # the yardstick: ATen's own data gradient (MIOpen) of the stored dC1, channels_last bf16 and fp32
    g_cl = dc1.view(N, OH, OW, 32).permute(0, 3, 1, 2)
    for name, gg, ww in (("bf16", g_cl, w.bfloat16()), ("fp32", g_cl.float(), w)):
        t = timeit(lambda: torch.nn.grad.conv2d_input((N, 3, IH, IW), ww, gg, stride=2, padding=0), iters=10)
        line(f"ATen conv2d_input, {name} channels_last gradient", t)
        line(f"  xcp_bn_bwd_apply + ATen conv2d_input ({name}): the yardstick", t_a + t)


def step(dev):
    from Models.XceptionLSTMV import XceptionLSTMV
    B, T, S = 16, 16, 299
    torch.manual_seed(0)
    m = XceptionLSTMV(128, pretrained=False)
    for p in m.feature_extractor.parameters():
        p.requires_grad = True
    m = m.to(dev)
    x = torch.rand(B, T, 3, S, S, device=dev)
    yb = (torch.arange(B, device=dev) % 2).float().view(B, 1)
    print(f"backbone step, forward + backward, {B} x {T} x {S}^2 bf16, parameters unfrozen, no optimiser "
          "(the parent commit cannot run the frozen-statistics rows: nothing to compare them with)")

    def one(x_grad):
        for p in m.parameters():
            p.grad = None
        xx = x.detach().requires_grad_(x_grad)
        with xcp.precision("bf16"):
            nn.BCELoss()(m(m.extract_features(xx)), yb).backward()

    for name, bn_train, x_grad in (("train mode (batch statistics)", True, False),
                                   ("frozen statistics (BatchNorms in eval mode)", False, False),
                                   ("frozen statistics + gradient w.r.t. the frames", False, True),
                                   ("train mode + gradient w.r.t. the frames", True, True)):
        m.train()
        m.fc_layers.eval()
        for b in m.feature_extractor.modules():
            if isinstance(b, nn.BatchNorm2d):
                b.train(bn_train)
        ms = timeit(lambda: one(x_grad), iters=10, warm=3)
        print(f"  {name:58s} {ms:9.2f} ms  {B / ms * 1e3:8.1f} clips/s", flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_bench needs the GPU (there is no CPU timing)")
    dev = torch.device("cuda:0")
    ops._lib.load()
    sel = set(sys.argv[1:]) or {"kernel", "step"}
    with torch.cuda.device(dev):
        if "kernel" in sel:
            kernel(dev)
        if "step" in sel:
            step(dev)


if __name__ == "__main__":
    main()
