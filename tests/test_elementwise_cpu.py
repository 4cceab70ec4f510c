"""The element-wise measure of tests/elementwise.py, proven on the CPU before it judges a kernel.

Sound: CPU emulations of the depthwise forward, the depthwise backward and an NT GEMM -- torch fp32
with bf16 roundings at the kernels' rounding points, summed in two different orders -- pass it at
every depthwise and NT GEMM shape of test_gpu_elementwise.py, on the very data that file feeds the
kernels (the inputs are generated on the CPU), with the excluded share <= 1e-4 and the nearest
share >= 0.99.  The nine-slice pool references are checked against torch's own pooling.

Sharp: planted defects that the norm measure of test_gpu_kernels.py lets through make it raise.
"""
import pytest
import torch
import torch.nn.functional as F

import elementwise as E


def rel_err(a, b):   # the measure of test_gpu_kernels.py
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ emulations (fp32 arithmetic)
def emu_taps(a32, w32, transposed, order):
    """3x3 taps in fp32, products rounded (no fma), tap order forward (0) or reversed (1)"""
    N, H, W, C = a32.shape
    p = F.pad(a32, (0, 0, 1, 1, 1, 1))
    acc = torch.zeros_like(a32)
    taps = range(9) if order == 0 else range(8, -1, -1)
    for t in taps:
        ky, kx = divmod(t, 3)
        oy, ox = (2 - ky, 2 - kx) if transposed else (ky, kx)
        acc = acc + p[:, oy:oy + H, ox:ox + W] * w32[t]
    return acc


def emu_act(x, act, sc, sh, round_bf16):
    """(activated fp32 value as the taps see it, ReLU mask); the fma is one rounding, as on the GPU"""
    if act == 2:
        z = (x.double() * sc.double() + sh.double()).float()
    else:
        z = x.float()
    a = z.clamp_min(0) if act else z
    if round_bf16:
        a = a.bfloat16().float()
    return a, ((z > 0) if act else torch.ones_like(z, dtype=torch.bool))


def emu_dw_fwd(d, act, round_bf16, order):
    a, _ = emu_act(d["x"], act, d["scale"], d["shift"], round_bf16)
    return emu_taps(a, d["wt"], False, order).bfloat16()


def psum(t, order):
    """fp32 sum over the pixels in two orders"""
    if order == 0:
        return t.sum((0, 1, 2))
    return t.permute(2, 1, 0, 3).contiguous().sum(0).sum(0).sum(0)


def emu_dw_bwd(d, act, form, order):
    x, dy = d["x"], d["dy"]
    N, H, W, C = x.shape
    a, mask = emu_act(x, act, d["scale"], d["shift"], False)
    s = emu_taps(dy.float(), d["wt"], True, order)
    up = None
    if "skip" in form:
        up = torch.zeros(N, H, W, C)
        up[:, ::2, ::2] = d["dskip"].float()
    if form == "skip_pre":
        s = s + up
    s = s * mask
    dz = s.bfloat16()   # the masked gradient as stored when nothing is added after the mask
    if form in ("res", "res+skip", "resbn"):
        s = s + d["dres"].float()
    if form in ("skip", "res+skip"):
        s = s + up
    dx = s.bfloat16()
    p = F.pad(a, (0, 0, 1, 1, 1, 1))
    dw = torch.stack([psum(dy.float() * p[:, ky:ky + H, kx:kx + W], order) for ky in range(3) for kx in range(3)])
    sums = None
    if form in ("plain", "skip_pre", "resbn") and act == 2:
        src, dzz = (d["yb"], dx) if form == "resbn" else (x, dz)
        zhat = (src.float() - d["mean"]) * d["invstd"]
        sums = torch.stack([psum(dzz.float(), order), psum(dzz.float() * zhat, order)])
    return dx, dw, sums


def emu_gemm_nt(A, B, order):
    A, B = A.float(), B.float()
    if order == 0:
        return (A @ B.t()).bfloat16()
    h = A.shape[1] // 2   # the upper half of K first, then the lower
    return ((A[:, h:] @ B[:, h:].t()) + (A[:, :h] @ B[:, :h].t())).bfloat16()


def bwd_kwargs(d, form):
    return dict(dres=d["dres"] if form in ("res", "res+skip", "resbn") else None,
                dskip=d["dskip"] if "skip" in form else None, skip_pre=form == "skip_pre")


# ------------------------------------------------------------------ sound
@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("shape", E.DW_FWD_SHAPES, ids=str)
def test_sound_dw_fwd(shape, act, order):
    N, C, H, W = shape
    d = E.dw_inputs(N, C, H, W)
    rb = E.dw_staged_bf16(W)
    ref, ab, extra = E.dw_fwd_ref(d["x"], d["wt"], act, d["scale"], d["shift"], rb)
    st = E.assert_bf16_stored(emu_dw_fwd(d, act, rb, order), ref, ab, 9, extra=extra)
    assert st["nearest"] >= 0.99 and st["excluded"] == 0


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("form,act", E.DW_BWD_FORMS)
@pytest.mark.parametrize("shape", E.DW_BWD_SHAPES, ids=str)
def test_sound_dw_bwd(shape, form, act, order):
    N, C, H, W = shape
    d = E.dw_inputs(N, C, H, W)
    r = E.dw_bwd_ref(d["dy"], d["x"], d["wt"], act, d["scale"], d["shift"], **bwd_kwargs(d, form))
    dx, dw, sums = emu_dw_bwd(d, act, form, order)
    st = E.assert_bf16_stored(dx, r["dx"], r["dx_abs"], 11, exclude=r["dx_excl"])
    assert st["excluded"] <= 1e-4 and st["nearest"] >= 0.99
    E.assert_f32_sum(dw, r["dw"], r["dw_abs"], N * H * W)
    if sums is not None:
        # over the stored dX (resbn: against yb; else against x -- the stored dX is the masked dz)
        ref, ab = E.bn_sums_ref(dx, d["yb"] if form == "resbn" else d["x"], d["mean"], d["invstd"])
        E.assert_f32_sum(sums, ref, ab, N * H * W)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", E.GEMM_NT_SHAPES, ids=str)
def test_sound_gemm_nt(shape, order):
    M, N, K, lda = shape
    Abuf, B = E.gemm_nt_inputs(M, N, K, lda)
    ref, ab = E.gemm_nt_ref(Abuf[:, :K], B)
    st = E.assert_bf16_stored(emu_gemm_nt(Abuf[:, :K], B, order), ref, ab, K)
    assert st["nearest"] >= 0.99


def test_sound_tie_allowance():
    """An intermediate exactly on a bf16 tie, rounded the other way, stays inside the bound only
    through `extra`."""
    d = E.dw_inputs(1, 8, 3, 9)
    x = torch.ones(1, 3, 9, 8).bfloat16()
    sc, sh = torch.full((8,), 1.0), torch.full((8,), 2.0 ** -8)   # z = 1 + 2^-8: the tie between 1 and 1 + 2^-7
    ref, ab, extra = E.dw_fwd_ref(x, d["wt"], 2, sc, sh, True)
    assert (extra > 0).all()
    a_other = torch.full((1, 3, 9, 8), 1.0 + 2.0 ** -7)           # RNE gives 1.0; the neighbour
    out = emu_taps(a_other, d["wt"], False, 0).bfloat16()
    E.assert_bf16_stored(out, ref, ab, 9, extra=extra, nearest_floor=0.0)
    with pytest.raises(AssertionError):
        E.assert_bf16_stored(emu_taps(a_other * 1.02, d["wt"], False, 0).bfloat16(), ref, ab, 9, extra=extra,
                             nearest_floor=0.0)


def test_excluded_share_is_a_condition():
    ref = torch.ones(100, 100, dtype=torch.float64)
    ex = torch.zeros(100, 100, dtype=torch.bool)
    ex[0, :2] = True
    with pytest.raises(AssertionError, match="excluded"):
        E.assert_bf16_stored(ref.bfloat16(), ref, ref, 1, exclude=ex)


# ------------------------------------------------------------------ sharp
@pytest.fixture(scope="module")
def fwd_case():
    N, C, H, W = 8, 728, 19, 19
    d = E.dw_inputs(N, C, H, W)
    ref, ab, extra = E.dw_fwd_ref(d["x"], d["wt"], 2, d["scale"], d["shift"], True)
    out = emu_dw_fwd(d, 2, True, 0)
    E.assert_bf16_stored(out, ref, ab, 9, extra=extra)
    return d, ref, ab, extra, out


def caught(out, ref, ab, n, extra=None):
    assert rel_err(out.float(), ref) < 1e-2          # the old measure lets it through
    with pytest.raises(AssertionError, match="outside the bf16-neighbour bound"):
        E.assert_bf16_stored(out, ref, ab, n, extra=extra)


def test_sharp_two_ulps(fwd_case):
    d, ref, ab, extra, out = fwd_case
    bad = out.clone()
    v = bad[3, 7, 11, 100].double()
    bad[3, 7, 11, 100] = (v + 2 * E.ulp_bf16(v)).bfloat16()
    caught(bad, ref, ab, 9, extra)


def test_sharp_tap_dropped_at_a_corner(fwd_case):
    d, ref, ab, extra, out = fwd_case
    a, _ = emu_act(d["x"], 2, d["scale"], d["shift"], True)
    bad = out.clone()
    # output (0, 0) of frame 5 without its (ky, kx) = (2, 2) tap, every channel
    bad[5, 0, 0] = (out[5, 0, 0].float() - a[5, 1, 1] * d["wt"][8]).bfloat16()
    caught(bad, ref, ab, 9, extra)


def test_sharp_channel_pair_swapped(fwd_case):
    d, ref, ab, extra, out = fwd_case
    bad = out.clone()
    bad[2, 18, 18, 726], bad[2, 18, 18, 727] = out[2, 18, 18, 727], out[2, 18, 18, 726]
    caught(bad, ref, ab, 9, extra)


def test_sharp_gemm_last_row_from_the_row_above():
    M, N, K = 77073, 264, 40    # the last 256-row tile holds 17 rows
    Abuf, B = E.gemm_nt_inputs(M, N, K, K)
    ref, ab = E.gemm_nt_ref(Abuf, B)
    out = emu_gemm_nt(Abuf, B, 0)
    E.assert_bf16_stored(out, ref, ab, K)
    bad = out.clone()
    bad[M - 1] = out[M - 2]
    caught(bad, ref, ab, K)


def test_sharp_wgrad_pixel_dropped():
    """One pixel's contribution missing from one lane's (a channel pair's) weight gradient: the old
    tolerance (rel_err < 1e-2 over the whole dW) passes, the fp32-sum bound does not."""
    N, C, H, W = 3, 728, 19, 19
    d = E.dw_inputs(N, C, H, W)
    r = E.dw_bwd_ref(d["dy"], d["x"], d["wt"], 2, d["scale"], d["shift"])
    _, dw, _ = emu_dw_bwd(d, 2, "plain", 0)
    E.assert_f32_sum(dw, r["dw"], r["dw_abs"], N * H * W)
    a, _ = emu_act(d["x"], 2, d["scale"], d["shift"], False)
    bad = dw.clone()
    p = (1, 9, 9)
    for c in (40, 41):
        for t in range(9):
            ky, kx = divmod(t, 3)
            bad[t, c] -= d["dy"][p][c].float() * a[p[0], p[1] + ky - 1, p[2] + kx - 1, c]
    assert rel_err(bad, r["dw"]) < 1e-2
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, r["dw"], r["dw_abs"], N * H * W)


# ------------------------------------------------------------------ pools
@pytest.mark.parametrize("H,W", [(19, 20), (20, 19), (1, 2)])
def test_maxpool_refs_against_torch(H, W):
    """the nine-slice max pool and its scatter backward equal torch's (fp64, no ties in random data)"""
    g = torch.Generator().manual_seed(H * W)
    z = torch.randn(2, H, W, 8, generator=g, dtype=torch.float64).requires_grad_(True)
    ref = F.max_pool2d(z.permute(0, 3, 1, 2), 3, 2, 1)
    m, am = E.maxpool3s2_ref(z.detach())
    assert torch.equal(m.permute(0, 3, 1, 2), ref)
    d = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ref.backward(d)
    dz, ab = E.maxpool3s2_bwd_ref(d.permute(0, 2, 3, 1), am, H, W)
    torch.testing.assert_close(dz, z.grad, rtol=0, atol=1e-15)
    assert (ab >= dz.abs() - 1e-15).all()


def test_maxpool_first_max_rule():
    z = torch.zeros(1, 3, 3, 1)
    z[0, 1, 1, 0] = z[0, 2, 2, 0] = 5.0      # window (1, 1) holds both: taps 0 and 4, the first wins
    m, am = E.maxpool3s2_ref(z)
    assert am[0, :, :, 0].tolist() == [[8, 6], [2, 0]] and (m == 5).all()
