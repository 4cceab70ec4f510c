"""The stem conv1 data gradient (xcp_conv1_dgrad, xcp_conv1_dgrad_bn; csrc/stem.hip) on the MI355X.

Reference: torch.nn.grad.conv2d_input in fp64 on the CPU, from the very values the kernel reads (for a
bf16 gradient: the already-rounded ones).  Per-element bound

    |dx - ref| <= 2e-5 * conv2d_input(|g|, |W|)

-- at most 128 products per input pixel accumulated in fp32 (128 * 2^-24 = 7.6e-6 of the sum of their
magnitudes) plus an allowance of 2^-17 = 7.6e-6 for a split-bf16 MFMA product, the stem forward's.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, IH, IW): odd sizes; uncovered last row; uncovered last column; both (the audio family); the bench's
# row width over more than one chunk of row pairs; the wide fallback (frames too wide for the staged rows)
SHAPES = [(3, 11, 11), (2, 12, 13), (2, 13, 12), (2, 64, 64), (2, 35, 299), (1, 5, 700)]
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops(gpu):
    from xcp import ops as o
    o._lib.load()
    return o


def _operands(N, IH, IW, dt, gpu):
    OH, OW = (IH - 3) // 2 + 1, (IW - 3) // 2 + 1
    g = torch.Generator().manual_seed(1000 * IH + IW)
    dc1 = torch.randn(N, OH, OW, 32, generator=g).to(dt)   # NHWC, the engine's layout
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.2
    return dc1, w, OH, OW


def _reference(dc1, w, N, IH, IW):
    """(fp64 conv2d_input, the same over magnitudes) from the stored values"""
    g64 = dc1.double().permute(0, 3, 1, 2).contiguous()
    ref = torch.nn.grad.conv2d_input((N, 3, IH, IW), w.double(), g64, stride=2, padding=0)
    mag = torch.nn.grad.conv2d_input((N, 3, IH, IW), w.double().abs(), g64.abs(), stride=2, padding=0)
    return ref, mag


def _check(dx, ref, mag, IH, IW):
    err = (dx.double().cpu() - ref).abs()
    worst = (err / mag.clamp_min(1e-30)).max().item()
    print(f"conv1_dgrad {tuple(dx.shape)}: worst |dx - ref| / conv2d_input(|g|, |W|) = {worst:.3e}")
    assert torch.all(err <= 2e-5 * mag), worst
    # rows / columns no 3x3 stride-2 window covers: written by the kernel, exactly zero
    if IH % 2 == 0:
        assert torch.all(dx[:, :, IH - 1, :] == 0)
    if IW % 2 == 0:
        assert torch.all(dx[:, :, :, IW - 1] == 0)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,IH,IW", SHAPES)
def test_conv1_dgrad_vs_fp64(ops, gpu, N, IH, IW, dt):
    dc1, w, OH, OW = _operands(N, IH, IW, dt, gpu)
    ref, mag = _reference(dc1, w, N, IH, IW)
    # (NaN-filled: every element must be written by the kernel, the uncovered edges included)
    dx = torch.full((N, 3, IH, IW), float("nan"), device=gpu)
    ops.conv1_dgrad(dc1.to(gpu), w.to(gpu), dx, N, IH, IW)
    torch.cuda.synchronize()
    _check(dx, ref, mag, IH, IW)
    dx2 = torch.full((N, 3, IH, IW), float("nan"), device=gpu)
    ops.conv1_dgrad(dc1.to(gpu), w.to(gpu), dx2, N, IH, IW)
    assert torch.equal(dx, dx2)   # no atomics: two runs give the same bits


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,IH,IW", SHAPES)
def test_conv1_dgrad_bn_equals_apply_then_dgrad(ops, gpu, N, IH, IW, dt, relu):
    """the fused form (BN1's backward apply, and the ReLU mask, formed on load) against xcp_bn_bwd_apply
    followed by the plain kernel on the stored tensor: bit for bit, and within the fp64 bound"""
    from xcp.engine import Stats
    dz, w, OH, OW = _operands(N, IH, IW, dt, gpu)
    g = torch.Generator().manual_seed(7)
    y = torch.randn(N, OH, OW, 32, generator=g).to(dt).to(gpu)
    dz, w = dz.to(gpu), w.to(gpu)
    coef = (torch.randn(3 * 32, generator=g) * 0.5).to(gpu)   # alpha, bcoef, delta
    st = Stats(32, gpu)
    st.scale.copy_(torch.randn(32, generator=g))
    st.shift.copy_(torch.randn(32, generator=g) * 0.3)
    rows = N * OH * OW
    dc1 = torch.empty_like(dz)
    ops.bn_apply_coef(dz, y, dc1, coef, st, rows, 32, relu)
    a = torch.full((N, 3, IH, IW), float("nan"), device=gpu)
    ops.conv1_dgrad(dc1, w, a, N, IH, IW)
    b = torch.full((N, 3, IH, IW), float("nan"), device=gpu)
    ops.conv1_dgrad_bn(dz, y, w, coef, st, b, N, IH, IW, 32, relu=relu)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    ref, mag = _reference(dc1.cpu(), w.cpu(), N, IH, IW)
    _check(b, ref, mag, IH, IW)
