"""Depthwise forward: the workgroup -> work-item map for frame counts that are a multiple of 8 (frames dealt
round-robin to the XCDs, csrc/dwconv.hip fwd_item_id) against the XCD-contiguous map every other frame count
takes.  One call over N frames must equal, bit for bit, the same op over slices of the batch whose frame
counts are no multiple of 8 (the map the parity tests of test_gpu_kernels.py pin): every item is computed
once, by the same arithmetic, whichever workgroup runs it.  The output is pre-filled with NaN, so an item
no workgroup takes shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu):
    from xcp import ops as o
    o._lib.load()
    return o


# (N, chunk, H, W, C, dtype, act): chunk = frames per reference call (no chunk's frame count is a multiple of 8)
CASES = [
    (8, 3, 19, 19, 736, torch.bfloat16, 2),    # the middle flow's shape: one tile per frame, 23 channel slices
    (24, 7, 19, 19, 736, torch.bfloat16, 1),   # three rounds of 8 frames
    (16, 5, 37, 37, 256, torch.bfloat16, 2),   # four tiles per frame
    (8, 3, 10, 10, 1536, torch.bfloat16, 2),   # 128-B channel slices (dw_fwd_kernel)
    (8, 3, 19, 19, 64, torch.float32, 0),      # fp32 form
]


@pytest.mark.parametrize("N,chunk,H,W,C,dt,act", CASES)
def test_dw_fwd_frame_round_robin_is_bitwise(ops, gpu, N, chunk, H, W, C, dt, act):
    g = torch.Generator(device=gpu).manual_seed(N * 100 + H + C + act)
    X = torch.randn(N * H * W, C, device=gpu, generator=g).to(dt)
    Wt = torch.randn(9, C, device=gpu, generator=g) * 0.3
    sc = torch.rand(C, device=gpu, generator=g) + 0.5
    sh = torch.randn(C, device=gpu, generator=g) * 0.5
    Y = torch.full((N * H * W, C), float("nan"), device=gpu, dtype=dt)
    ops.dw_fwd(act, X, Y, Wt, sc, sh, N, H, W, C)
    ref = torch.full_like(Y, float("nan"))
    px = H * W
    for n0 in range(0, N, chunk):
        n = min(chunk, N - n0)
        assert n % 8 != 0
        ops.dw_fwd(act, X[n0 * px:(n0 + n) * px], ref[n0 * px:(n0 + n) * px], Wt, sc, sh, n, H, W, C)
    torch.cuda.synchronize()
    assert not torch.isnan(Y.float()).any()
    assert torch.equal(Y, ref)
