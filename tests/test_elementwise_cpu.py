"""The element-wise measure of tests/elementwise.py, proven on the CPU before it judges a kernel.

Sound: CPU emulations of the depthwise forward, the depthwise backward and an NT GEMM -- torch fp32
with bf16 roundings at the kernels' rounding points, summed in two different orders -- pass it at
every depthwise and NT GEMM shape of test_gpu_elementwise.py, on the very data that file feeds the
kernels (the inputs are generated on the CPU), with the excluded share <= 1e-4 and the nearest
share >= 0.99.  The nine-slice pool references are checked against torch's own pooling.

Sharp: planted defects that the norm measure of test_gpu_kernels.py lets through make it raise.

The block tails and pools (E.POOL_SHAPES, E.TAIL_PLAIN_SHAPES: the small and odd frames of the 64^2, 75^2, 224^2
and 256^2 families) get the same two halves after the pool references: fp32 emulations of the pooled and the
un-pooled tail, the max-pool backward and the fused BN sums, and four defects of those edges, one thread's share each.

The second half does the same for the stem convolutions and the BatchNorm statistics chain
(test_gpu_elementwise_stem_bn.py): the split-bf16 allowance of the conv1 row kernels is shown to be enough by
an emulation that forms hi / lo with .bfloat16() and adds the product groups in fp32; the finalize bounds by
the kernels' fp64 expression with the partial rows summed in another order and the outputs cast to fp32.

The third part serves test_gpu_elementwise_gather.py: gather_rows against torch's own convolutions, fp32
emulations of the gathered NT products, their stats rows, the split-K slabs and the slab reduction in two
orders, and chunk-sized planted defects (a chunk from the neighbouring pixel, a wrapped tap, a border tap that
is not zero, a row counted in two slabs or in none, a stats row counting a stored row twice).
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
@pytest.mark.parametrize("H,W", sorted({(1, 2)} | {s[2:] for s in E.POOL_SHAPES}))
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


# ------------------------------------------------------------------ block tails and pools at small and odd frames
def emu_tail(d, pool, bn_skip):
    """the block tail in fp32: fmaf as fma32, the first-max pool of the exact fp32 values, one fp32 add, a bf16
    store -> (out bf16, argmax taps or None)"""
    z = E.fma32(d["y"], d["s1"], d["t1"])
    am = None
    if pool:
        z, am = E.maxpool3s2_ref(z)
    sk = E.fma32(d["ys"], d["s2"], d["t2"]) if bn_skip else d["ys"].float()
    return (z + sk).bfloat16(), am


def emu_maxpool_bwd(dout, amax, H, W):
    """maxpool3s2_bwd_ref's scatter with fp32 additions (window order), stored bf16"""
    N, OH, OW, C = dout.shape
    g = torch.zeros(N, H + 2, W + 2, C)
    d = dout.float()
    for t in range(9):
        ky, kx = divmod(t, 3)
        g[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += d * (amax == t)
    return g[:, 1:H + 1, 1:W + 1].bfloat16()


def emu_bn_sums(dz, y, st, order=0):
    """(sum dz, sum dz zhat) over the stored dz in fp32, zhat by the kernel's two fp32 operations"""
    dzf = dz.float()
    return torch.stack([psum(dzf, order), psum(dzf * ((y.float() - st["mean"]) * st["invstd"]), order)])


def pool_refs(d, bn_skip=True):
    """(ref64, abs_terms, argmax) of the pooled tail's out"""
    H, W = d["y"].shape[1:3]
    m, am = E.maxpool3s2_ref(E.fma32(d["y"], d["s1"], d["t1"]))
    sk = (E.fma32(d["ys"], d["s2"], d["t2"]) if bn_skip else d["ys"]).double()
    return m.double() + sk, m.double().abs() + sk.abs(), am


def test_pool_shapes_reach_what_their_comments_say():
    """the launch geometry restated from make_chanred (the GPU file asserts the library's P equals it)"""
    geo = {s: E.chanred_geo(s[0] * ((s[2] - 1) // 2 + 1) * ((s[3] - 1) // 2 + 1), s[1]) for s in E.POOL_SHAPES}
    g = geo[(16, 736, 8, 8)]
    assert (g["nch"], g["CVB"], g["SPB"]) == (2, 46, 5) and 256 - g["CVB"] * g["SPB"] == 26
    assert geo[(60, 1024, 4, 4)]["SPB"] == 4 and geo[(200, 1024, 2, 2)]["SPB"] == 4
    assert geo[(2, 8, 7, 9)]["SPB"] == 256 and geo[(300, 64, 1, 1)]["SPB"] == 32
    assert (geo[(200, 1024, 2, 2)]["rpc"], geo[(200, 1024, 2, 2)]["P"]) == (16, 13)     # 12 full chunks and one of 8
    odd = [s for s in E.POOL_SHAPES if ((s[2] - 1) // 2 + 1) % 2 or ((s[3] - 1) // 2 + 1) % 2]
    assert len(odd) >= 7 and (2, 256, 14, 14) in odd and all(s[0] * s[2] * s[3] <= 1100 for s in E.POOL_SHAPES)


@pytest.mark.parametrize("bn_skip", [True, False], ids=["bn_skip", "identity_skip"])
@pytest.mark.parametrize("shape", E.POOL_SHAPES, ids=str)
def test_sound_tail_pool(shape, bn_skip):
    """the fp32 emulation of the pooled tail, the max-pool backward and the fused BN sums sits inside the bounds
    the GPU files hold the kernels to, on their data"""
    N, C, H, W = shape
    d = E.pool_inputs(N, C, H, W)
    ref, ab, am = pool_refs(d, bn_skip)
    out, am_e = emu_tail(d, True, bn_skip)
    st = E.assert_bf16_stored(out, ref, ab, 2)
    assert st["nearest"] >= 0.99 and torch.equal(am_e, am)
    zref, zab = E.maxpool3s2_bwd_ref(d["d"], am, H, W)
    dz = emu_maxpool_bwd(d["d"], am, H, W)
    assert E.assert_bf16_stored(dz, zref, zab, 4)["nearest"] >= 0.99
    stats = E.batch_stats(d["y"])
    sref, sab = E.bn_sums_ref(dz, d["y"], stats["mean"], stats["invstd"])
    for order in (0, 1):
        E.assert_f32_sum(emu_bn_sums(dz, d["y"], stats, order), sref, sab, N * H * W)


@pytest.mark.parametrize("bn_skip", [True, False], ids=["bn_skip", "identity_skip"])
@pytest.mark.parametrize("shape", E.TAIL_PLAIN_SHAPES, ids=str)
def test_sound_tail_plain(shape, bn_skip):
    N, C, H, W = shape
    d = E.pool_inputs(N, C, H, W, pool=False)
    ref, ab = E.tail_plain_ref(d["y"], d["s1"], d["t1"], d["ys"], *((d["s2"], d["t2"]) if bn_skip else ()))
    st = E.assert_bf16_stored(emu_tail(d, False, bn_skip)[0], ref, ab, 2)
    assert st["nearest"] >= 0.99 and st["excluded"] == 0


# Sharp at these edges.  Each defect is planted at the grain of ONE THREAD of the kernel it models (a quad of pixels
# and 8 channels; a lane's channel pair in the depthwise backward): the tensors here are small (16 000 to 750 000
# elements), and a defect across all channels of a column or a frame is norm-wise visible in them -- the last
# output column of (1, 128, 37, 21) shifted in every row and channel is rel_err 0.060, one frame's lost window row
# at (60, 1024, 4, 4) 0.049, one frame left out of every channel's sums at (200, 1024, 2, 2) 0.063.  One thread's
# share passes rel_err < 1e-2 and is the harder catch for the element-wise measure.
def test_sharp_tail_pool_last_column_from_the_clamped_window():
    """(1, 128, 37, 21) -> 19 x 11: the ragged quad column.  The last output column of the last quad row takes its
    window one pixel to the left (columns 18 .. 20 instead of 19 .. 21, the clamped start), 8 channels."""
    N, C, H, W = 1, 128, 37, 21
    d = E.pool_inputs(N, C, H, W)
    ref, ab, _ = pool_refs(d)
    out, _ = emu_tail(d, True, True)
    E.assert_bf16_stored(out, ref, ab, 2)
    OH, OW = d["OH"], d["OW"]
    assert OH % 2 == 1 and OW % 2 == 1
    z = E.fma32(d["y"], d["s1"], d["t1"])
    p = F.pad(z, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    ow, c = OW - 1, slice(40, 48)
    left = torch.stack([p[:, ky:ky + 2 * OH:2, 2 * ow + kx - 1] for ky in range(3) for kx in range(3)]).max(0)[0]
    sk = E.fma32(d["ys"], d["s2"], d["t2"])
    oh = OH - 1                                   # the corner quad holds this one valid output
    bad = out.clone()
    bad[:, oh, ow, c] = (left[:, oh, c] + sk[:, oh, ow, c]).bfloat16()
    assert 1 <= (bad != out).sum() <= 8
    caught(bad, ref, ab, 2)


def test_sharp_maxpool_bwd_window_below_taken_as_absent():
    """(60, 1024, 4, 4) -> 2 x 2: in one frame, quad (0, 0) treats window (a + 1, b) as absent, as the last quad
    row rightly does: pixels (1, 0) and (1, 1) lose what that window sends them (taps 1 and 2), 8 channels."""
    N, C, H, W = 60, 1024, 4, 4
    d = E.pool_inputs(N, C, H, W)
    _, _, am = pool_refs(d)
    ref, ab = E.maxpool3s2_bwd_ref(d["d"], am, H, W)
    E.assert_bf16_stored(emu_maxpool_bwd(d["d"], am, H, W), ref, ab, 4)
    n, c = 17, slice(40, 48)
    absent = am.clone()
    w = absent[n, 1, 0, c]                         # window (a + 1, b) = (1, 0) of quad (0, 0)
    w[(w == 1) | (w == 2)] = 0xFF                   # never matches a tap
    bad = emu_maxpool_bwd(d["d"], absent, H, W)
    lost = (bad != emu_maxpool_bwd(d["d"], am, H, W))
    assert 1 <= lost.sum() <= 8 and lost[n, 1, :2, c].sum() == lost.sum()
    caught(bad, ref, ab, 4)


def test_sharp_dw_bwd_corner_tap_at_two_by_two():
    """(16, 1536, 2, 2), plain, act 2: the bottom-right pixel's dX of one frame without the tap from its upper-left
    neighbour (dY[0, 0] w[8]: one of its four live taps), one lane's channel pair"""
    N, C, H, W = 16, 1536, 2, 2
    d = E.dw_inputs(N, C, H, W)
    r = E.dw_bwd_ref(d["dy"], d["x"], d["wt"], 2, d["scale"], d["shift"])
    dx, _, _ = emu_dw_bwd(d, 2, "plain", 0)
    E.assert_bf16_stored(dx, r["dx"], r["dx_abs"], 11, exclude=r["dx_excl"])
    n = 9
    _, mask = emu_act(d["x"], 2, d["scale"], d["shift"], False)
    live = [c for c in range(0, C, 2) if mask[n, 1, 1, c] and mask[n, 1, 1, c + 1]][3]      # both channels pass the ReLU
    c = slice(live, live + 2)
    s = emu_taps(d["dy"].float(), d["wt"], True, 0)[n, 1, 1, c]
    bad = dx.clone()
    bad[n, 1, 1, c] = (s - d["dy"][n, 0, 0, c].float() * d["wt"][8, c]).bfloat16()
    assert (bad != dx).sum() == 2
    assert rel_err(bad.float(), r["dx"]) < 1e-2
    with pytest.raises(AssertionError, match="outside the bf16-neighbour bound"):
        E.assert_bf16_stored(bad, r["dx"], r["dx_abs"], 11, exclude=r["dx_excl"])


def test_sharp_pool_bn_sums_skip_a_frame_after_a_chunk_boundary():
    """(200, 1024, 2, 2) -> 1 x 1: a quad is a frame, SPB = 4, 13 chunks of 16.  One thread's 8 channels leave out the
    first frame of chunk 1 (an advance() that overshoots by one frame): the sums stay within rel_err < 1e-2 and
    leave the fp32 bound of their 800 terms."""
    N, C, H, W = 200, 1024, 2, 2
    d = E.pool_inputs(N, C, H, W, salt=1)
    _, _, am = pool_refs(d)
    dz = emu_maxpool_bwd(d["d"], am, H, W)
    st = E.batch_stats(d["y"])
    ref, ab = E.bn_sums_ref(dz, d["y"], st["mean"], st["invstd"])
    good = emu_bn_sums(dz, d["y"], st)
    E.assert_f32_sum(good, ref, ab, N * H * W)
    f = E.chanred_geo(N, C)["rpc"]
    assert f == 16
    keep = torch.arange(N) != f
    bad = good.clone()
    bad[:, 40:48] = emu_bn_sums(dz[keep], d["y"][keep], st)[:, 40:48]
    assert (bad != good).any(0).sum() == 8
    assert rel_err(bad, ref) < 1e-2
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, ref, ab, N * H * W)


# ================================================================== stem convs and BN statistics
BF, FP = torch.bfloat16, torch.float32


def split(v):
    """bf16 head and tail of an fp32 tensor, as fp32 (v - hi is exact in fp32)"""
    hi = v.bfloat16().float()
    return hi, (v - hi).bfloat16().float()


def patches(x):
    """[N, 27, OH OW] fp32 im2col of the 3x3 stride-2 valid conv, k = ci 9 + ky 3 + kx"""
    return F.unfold(x, 3, stride=2)


def emu_conv1_fwd(x, w, path, order, dtype):
    """27 fp32 products per output added one by one (k ascending or descending); path "row": the products are
    the three groups lo.hi, hi.lo, hi.hi of the split operands (bf16 x bf16 is exact in fp32)"""
    P, w2 = patches(x), w.reshape(32, 27)
    N, _, L = P.shape
    ks = list(range(27)) if order == 0 else list(range(26, -1, -1))
    groups = [(P, w2)]
    if path == "row":
        (ph, pl), (wh, wl) = split(P), split(w2)
        groups = [(pl, wh), (ph, wl), (ph, wh)]
        if order:
            groups.reverse()
    acc = torch.zeros(N, L, 32)
    for a, b in groups:
        for k in ks:
            acc = acc + a[:, k, :, None] * b[:, k]
    OH, OW = E.conv1_out(x.shape[2], x.shape[3])
    return acc.view(N, OH, OW, 32).to(dtype)


def emu_conv1_wgrad(x, dy, path, order):
    """dW[co][k] = sum_p dy[p][co] patch[p][k] in fp32, the pixels in two orders (forward in one product;
    reversed and in two halves); path "row": X split into head and tail, two product groups"""
    P = patches(x).permute(0, 2, 1).reshape(-1, 27)
    g = dy.float().reshape(-1, 32)
    if order:
        P, g = P.flip(0), g.flip(0)
    parts = split(P)[::-1] if path == "row" else (P,)
    h = P.shape[0] // 2
    acc = torch.zeros(32, 27)
    for a in parts:
        acc = acc + (g.t() @ a if order == 0 else (g[h:].t() @ a[h:] + g[:h].t() @ a[:h]))
    return acc.view(32, 3, 3, 3)


def conv1_fwd_cases():
    return [("bf16", s) for s in E.CONV1_ROW_SHAPES] + E.CONV1_FWD_OTHER


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt,shape", conv1_fwd_cases(), ids=str)
def test_sound_conv1_fwd(dt, shape, order):
    d = E.conv1_inputs(*shape)
    path = E.conv1_path(dt == "bf16", shape[2])
    ref, ab, extra = E.conv1_ref(d["x"], d["w"], split=path == "row")
    out = emu_conv1_fwd(d["x"], d["w"], path, order, BF if dt == "bf16" else FP)
    if dt == "bf16":
        assert E.assert_bf16_stored(out, ref, ab, 27, extra=extra)["nearest"] >= 0.99
    else:
        E.assert_f32_sum(out, ref, ab, 27)


def test_conv1_paths():
    """the kernel each shape list is meant for, restated from the launchers"""
    assert all(E.conv1_path(True, s[2]) == "row" for s in E.CONV1_ROW_SHAPES)
    assert [E.conv1_path(dt == "bf16", s[2]) for dt, s in E.CONV1_FWD_OTHER] == ["tile"] * 5 + ["pixel"] * 2
    assert E.conv1_path(True, 3) == "tile" and E.conv1_path(True, E.CONV1_TILE_WIDEST + 1) == "pixel"
    assert [E.conv1_path(True, s[2], True) for s in E.CONV1_WGRAD_SHAPES] == \
        ["row", "row", "row", "tile", "pixel", "tile", "row"]
    assert [E.conv1_path(False, s[2], True) for s in E.CONV1_WGRAD_SHAPES] == \
        ["tile", "tile", "tile", "tile", "pixel", "tile", "tile"]


def test_conv1_wgrad_ref_is_the_sum_over_pixels():
    """conv2d_weight with stride 2 on an even-sized frame (uncovered last row / column) against the im2col sum"""
    d = E.conv1_inputs(2, 12, 13)
    ref, ab, _, n = E.conv1_wgrad_ref(d["x"], d["dy"])
    P = patches(d["x"].double()).permute(0, 2, 1).reshape(-1, 27)
    torch.testing.assert_close(ref.reshape(32, 27), d["dy"].double().reshape(-1, 32).t() @ P, rtol=0, atol=1e-12)
    assert n == 2 * 5 * 6 and (ab >= ref.abs() - 1e-12).all()


def wgrad_case(shape, dt, sparse=False):
    d = E.conv1_inputs(*shape)
    dy = d["dy"].to(BF if dt == "bf16" else FP)
    if sparse:
        dy = E.sparse_rows_gradient(dy, *E.conv1_wgrad_groups(*shape, dt == "bf16"))
    return d, dy, E.conv1_path(dt == "bf16", shape[2], True)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.CONV1_WGRAD_SHAPES + [E.CONV1_WGRAD_SPARSE], ids=str)
def test_sound_conv1_wgrad(shape, dt, order):
    d, dy, path = wgrad_case(shape, dt, shape == E.CONV1_WGRAD_SPARSE)
    ref, ab, extra, n = E.conv1_wgrad_ref(d["x"], dy, split=path == "row")
    assert n <= 1100
    E.assert_f32_sum(emu_conv1_wgrad(d["x"], dy, path, order), ref, ab, n, extra=extra)


def test_sparse_gradient_covers_the_tile_edges():
    shape = E.CONV1_WGRAD_SPARSE
    tiles, G = E.conv1_wgrad_groups(*shape, True)
    assert (tiles, G) == (1120, 560)
    dy = E.sparse_rows_gradient(E.conv1_inputs(*shape)["dy"], tiles, G)
    nz = (dy != 0).any(-1).view(tiles, -1)               # [tile][ow]
    assert nz.sum() <= 1000
    for b in (0, G - 1):                                  # first and last workgroup: tiles b and b + G
        assert nz[b, 0] and nz[b, -1] and nz[b + G, 0] and nz[b + G, -1]


def emu_conv3_dgrad(dy, w, order):
    p = F.pad(dy.float(), (0, 0, 2, 2, 2, 2))
    wf = w.float().permute(1, 0, 2, 3).flip(2, 3)
    N, H, W, _ = p.shape
    acc = torch.zeros(N, H - 2, W - 2, 32)
    for t in (range(9) if order == 0 else range(8, -1, -1)):
        ky, kx = divmod(t, 3)
        acc = acc + p[:, ky:ky + H - 2, kx:kx + W - 2] @ wf[:, :, ky, kx].t()
    return acc.bfloat16()


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("shape", E.CONV3_DGRAD_SHAPES, ids=str)
def test_sound_conv3x3_dgrad(shape, order):
    d = E.conv3_inputs(*shape, 64)
    ref, ab = E.conv3x3_dgrad_ref(d["x"], d["w"])
    assert ref.shape[1:3] == (shape[1] + 2, shape[2] + 2)
    assert E.assert_bf16_stored(emu_conv3_dgrad(d["x"], d["w"], order), ref, ab, 576)["nearest"] >= 0.99
    # against autograd's input gradient
    want = torch.nn.grad.conv2d_input((shape[0], 32, shape[1] + 2, shape[2] + 2), d["w"].double(),
                                      d["x"].double().permute(0, 3, 1, 2))
    torch.testing.assert_close(ref.permute(0, 3, 1, 2), want, rtol=0, atol=1e-12)


def conv3_wgrad_case(shape, bn):
    d = E.conv3_wgrad_inputs(*shape)
    dy = d["dy"]
    a, flip = E.bn_relu_on_load(d["x"], d["s"], d["t"]) if bn else (d["x"].double(), None)
    return d, dy, a, flip


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("shape", E.CONV3_WGRAD_SHAPES, ids=str)
def test_sound_conv3x3_wgrad(shape, bn, order):
    d, dy, a, flip = conv3_wgrad_case(shape, bn)
    ref, ab, extra = E.conv3x3_wgrad_ref(dy, a, flip)
    N, OH, OW, _ = dy.shape
    g, a32 = dy.float().reshape(-1, 64), a.float()
    if order:
        g = g.flip(0)
    out = torch.stack([g.t() @ (s.flip(0) if order else s) for s in
                       (a32[:, ky:ky + OH, kx:kx + OW].reshape(-1, 32) for ky in range(3) for kx in range(3))], 1)
    E.assert_f32_sum(out, ref, ab, N * OH * OW, extra=extra)
    want = torch.nn.grad.conv2d_weight(a.permute(0, 3, 1, 2), (64, 32, 3, 3), dy.double().permute(0, 3, 1, 2))
    torch.testing.assert_close(ref.view(64, 3, 3, 32).permute(0, 3, 1, 2), want, rtol=0, atol=1e-10)


def emu_chan_sums(mode, d, order):
    y, dz = d["y"].float(), d["dz"].float()
    if mode == 0:
        t = (y, y * y)
    else:
        if mode == 2:
            dz = dz * (E.fma32(d["y"], d["ms"], d["mt"]) > 0)
        t = (dz, dz * ((y - d["mean"]) * d["invstd"]))
    if order == 0:
        return torch.stack([v.sum(0) for v in t])
    return torch.stack([sum(v.flip(0)[i::5].sum(0) for i in range(5)) for v in t])


def chan_ref(mode, d):
    if mode == 0:
        return E.chan_sums_ref(0, d["y"])
    return E.chan_sums_ref(mode, d["dz"], d["y"], d["mean"], d["invstd"], d["ms"], d["mt"])


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.CHAN_SHAPES, ids=str)
def test_sound_chan_sums(shape, dt, mode, order):
    d = E.chan_inputs(*shape, dt)
    ref, ab, extra = chan_ref(mode, d)
    E.assert_f32_sum(emu_chan_sums(mode, d, order), ref, ab, shape[0], extra=extra)


def wave_sums(part, C, nw=16):
    """column sums in the order of fin_reduce: rows w, w + nw, ... per wave, then the waves; more than
    FIN_MAX_ROWS rows are first folded to 256 fp32 group sums (ops._fold)"""
    p = part[:, :, :C]
    if p.shape[0] > E.FIN_MAX_ROWS:
        R = p.shape[0]
        grp = torch.arange(R) * 256 // R
        p = torch.stack([p[grp == i].double().sum(0).float() for i in range(256)])
    p = p.double()
    s = sum(p[w::nw].flip(0).sum(0) for w in range(min(nw, p.shape[0])))
    return s[0], s[1]


def emu_bn_finalize(d, swap_mean=None):
    C = d["gamma"].shape[0]
    s, q = wave_sums(d["part"], C)
    mom, eps = float(torch.tensor(d["momentum"], dtype=FP)), float(torch.tensor(d["eps"], dtype=FP))
    mean = s / d["count"]
    var = (q / d["count"] - mean * mean).clamp_min(0)
    unb = var * d["count"] / (d["count"] - 1) if d["count"] > 1 else var
    inv = (1 / (var + eps).sqrt()).float()
    sc = d["gamma"] * inv
    m32 = mean.float()
    if swap_mean is not None:      # the planted defect: channel c's shift from channel c + 1's mean
        m32 = m32.clone()
        m32[swap_mean] = mean.float()[swap_mean + 1]
    return {"mean": mean.float(), "invstd": inv, "scale": sc, "shift": d["beta"] - m32 * sc,
            "running_mean": ((1 - mom) * d["rmean"].double() + mom * mean).float(),
            "running_var": ((1 - mom) * d["rvar"].double() + mom * unb).float()}


def emu_bn_bwd_finalize(d, form, nw=16):
    C = d["gamma"].shape[0]
    sdz, sdzy = wave_sums(d["part"], C, nw)
    inv, gm, mu = d["invstd"].double()[:C], d["gamma"].double(), d["mean"].double()[:C]
    a = gm * inv
    mdz, mdzy = sdz / d["count"], sdzy / d["count"]
    z = torch.zeros(C)
    fro, acc = "frozen" in form, "accumulate" in form
    return {"alpha": a.float(), "bcoef": z if fro else (-a * inv * mdzy).float(),
            "delta": z if fro else (-a * mdz + a * inv * mu * mdzy).float(),
            "dgamma": d["dgamma0"] + sdzy.float() if acc else sdzy.float(),
            "dbeta": d["dbeta0"] + sdz.float() if acc else sdz.float()}


def fin_ref(d):
    return E.bn_finalize_ref(d["part"], d["count"], d["gamma"], d["beta"], d["rmean"], d["rvar"], d["momentum"],
                             d["eps"])


def fin_bwd_ref(d, form):
    base = (d["dgamma0"], d["dbeta0"]) if "accumulate" in form else None
    return E.bn_bwd_finalize_ref(d["part"], d["count"], d["gamma"], d["mean"], d["invstd"], "frozen" in form, base)


@pytest.mark.parametrize("C,CP", E.FIN_CHANNELS)
@pytest.mark.parametrize("R", E.FIN_ROWS)
def test_sound_bn_finalize(R, C, CP):
    d = E.fin_fwd_inputs(R, C, CP)
    ref, out = fin_ref(d), emu_bn_finalize(d)
    for k, (r, b) in ref.items():
        E.assert_within(out[k], r, b, tag=k)
    # the constant channel: var is exactly zero, whatever the order of the sums
    assert ref["invstd"][0][1].float() == (1 / torch.tensor(1e-5, dtype=FP).double().sqrt()).float()
    assert out["mean"][1] == 3.0 and out["invstd"][1] == out["invstd"][0]


@pytest.mark.parametrize("form", E.FIN_BWD_FORMS)
@pytest.mark.parametrize("C,CP", E.FIN_CHANNELS)
@pytest.mark.parametrize("R", E.FIN_ROWS)
def test_sound_bn_bwd_finalize(R, C, CP, form):
    d = E.fin_bwd_inputs(R, C, CP)
    out = emu_bn_bwd_finalize(d, form, 4 if "narrow" in form else 16)
    for k, (r, b) in fin_bwd_ref(d, form).items():
        E.assert_within(out[k], r, b, tag=k)


# ------------------------------------------------------------------ sharp: stem and statistics
@pytest.fixture(scope="module")
def conv1_case():
    """the bench frame of test_conv1_fwd_wgrad (2 x 299 x 299, bf16: the row kernel)"""
    d = E.conv1_inputs(2, 299, 299)
    ref, ab, extra = E.conv1_ref(d["x"], d["w"], split=True)
    out = emu_conv1_fwd(d["x"], d["w"], "row", 0, BF)
    E.assert_bf16_stored(out, ref, ab, 27, extra=extra)
    return d, ref, ab, extra, out


def test_sharp_conv1_tap_dropped_at_one_pixel(conv1_case):
    d, ref, ab, extra, out = conv1_case
    bad = out.clone()
    n, oh, ow, k = 1, 148, 0, 26                    # tap (ci, ky, kx) = (2, 2, 2) of the first pixel of the last row
    xv = d["x"][n, 2, 2 * oh + 2, 2 * ow + 2]
    bad[n, oh, ow] = (out[n, oh, ow].float() - xv * d["w"].reshape(32, 27)[:, k]).bfloat16()
    caught(bad, ref, ab, 27, extra)


def test_sharp_conv1_last_column_from_the_clamped_row(conv1_case):
    """pixel OW - 1 of one row stored from A row OW - 2"""
    d, ref, ab, extra, out = conv1_case
    bad = out.clone()
    bad[0, 77, 148] = out[0, 77, 147]
    caught(bad, ref, ab, 27, extra)


def test_sharp_conv1_wgrad_pixel_dropped():
    """One pixel (the last of a workgroup's last tile) missing from one output channel's sum, at the sparse
    gradient's 752 nonzero pixels: rel_err < 1e-2 over dW passes, the fp32-sum bound does not."""
    d, dy, path = wgrad_case(E.CONV1_WGRAD_SPARSE, "bf16", True)
    ref, ab, extra, n = E.conv1_wgrad_ref(d["x"], dy, split=True)
    out = emu_conv1_wgrad(d["x"], dy, path, 0)
    E.assert_f32_sum(out, ref, ab, n, extra=extra)
    N, OH, OW, _ = dy.shape
    P = patches(d["x"]).permute(0, 2, 1).reshape(-1, 27)
    p = N * OH * OW - 1
    co = int((dy.reshape(-1, 32)[p].float().abs() - 0.5).abs().argmin())      # a gradient of middling size
    assert 0.25 < dy.reshape(-1, 32)[p, co].abs() < 1
    bad = out.clone()
    bad[co] -= (dy.reshape(-1, 32)[p, co].float() * P[p]).view(3, 3, 3)
    assert rel_err(bad, ref) < 1e-2
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, ref, ab, n, extra=extra)


def test_sharp_row_dropped_from_the_gradient_sums():
    """chanred (bn_bwd_reduce) without the last row of a ragged chunk, at a gradient of realistic size: dbeta /
    dgamma move by less than test_bn_forward_backward's atol 1e-3, and leave the fp32-sum bound."""
    rows, C = 1083, 728
    d = E.chan_inputs(rows, C, BF)
    d["dz"] = (d["dz"].float() * 1e-4).bfloat16()
    ref, ab, extra = chan_ref(1, d)
    out = emu_chan_sums(1, d, 0)
    E.assert_f32_sum(out, ref, ab, rows, extra=extra)
    short = dict(d, y=d["y"][:-1], dz=d["dz"][:-1])
    bad = emu_chan_sums(1, short, 0)
    torch.testing.assert_close(bad.double(), ref, rtol=1e-4, atol=1e-3)
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, ref, ab, rows, extra=extra)


def test_sharp_row_dropped_from_row_stats():
    """row_stats without its last row: the normalised bf16 output it leads to passes rel_err < 1e-2 (the bf16
    measure of test_bn_forward_backward), the sums leave the bound."""
    rows, C = 1083, 728
    d = E.chan_inputs(rows, C, BF)
    ref, ab, extra = chan_ref(0, d)
    bad = emu_chan_sums(0, dict(d, y=d["y"][:-1]), 0)

    def normalised(s):
        mean = s[0] / rows
        inv = 1 / (s[1] / rows - mean * mean + 1e-5).sqrt()
        return ((d["y"].double() - mean) * inv).bfloat16()

    assert rel_err(normalised(bad.double()).float(), normalised(ref)) < 1e-2
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, ref, ab, rows, extra=extra)


def test_sharp_last_partial_row_left_out_of_a_finalize():
    """R = 769: one row past the 16 x 48 rows of fin_reduce's first pass.  Without it dgamma / dbeta and the
    coefficients stay within rtol 1e-4 / atol 1e-3 and leave their bounds."""
    d = E.fin_bwd_inputs(769, 728, 736)
    d["part"] = d["part"] * 0.1                      # partial sums of 1e-4: one row moves a sum by << 1e-3
    ref = fin_bwd_ref(d, "plain")
    bad = emu_bn_bwd_finalize(dict(d, part=d["part"][:-1]), "plain")
    for k in ("dgamma", "dbeta", "bcoef", "delta"):          # (channels 3 ..: invstd of ordinary size)
        r, b = ref[k]
        torch.testing.assert_close(bad[k][3:].double(), r[3:], rtol=1e-4, atol=1e-3)
        with pytest.raises(AssertionError, match="outside the fp32 bound"):
            E.assert_within(bad[k][3:], r[3:], b[3:], tag=k)
    # the forward finalize, the last two data rows small (0.01) in the ordinary channels 3 ..
    f = E.fin_fwd_inputs(769, 40, 40)
    f["part"][-1, 0, 3:], f["part"][-1, 1, 3:] = 2 * 0.01, 2 * 0.01 ** 2
    rf = fin_ref(f)
    badf = emu_bn_finalize(dict(f, part=f["part"][:-1]))
    for k in ("mean", "shift"):
        r, b = rf[k]
        torch.testing.assert_close(badf[k][3:].double(), r[3:], rtol=1e-4, atol=1e-3)
        with pytest.raises(AssertionError, match="outside the fp32 bound"):
            E.assert_within(badf[k][3:], r[3:], b[3:], tag=k)


def test_sharp_shift_from_the_neighbouring_channels_mean():
    """shift[c] formed with channel c + 1's mean, the two means 5e-4 apart: inside atol 1e-3, outside the bound"""
    d = E.fin_fwd_inputs(17, 40, 40)
    c = 7
    d["part"][:, 0, c + 1] = d["part"][:, 0, c] + 1e-3          # two data rows per partial row
    ref = fin_ref(d)
    bad = emu_bn_finalize(d, swap_mean=c)
    torch.testing.assert_close(bad["shift"].double(), ref["shift"][0], rtol=1e-4, atol=1e-3)
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_within(bad["shift"], *ref["shift"], tag="shift")


# ================================================================== gathered GEMMs and split-K slabs
GATHER_CASES = [(1, s) for s in E.GATHER1_SHAPES] + [(m, s) for m in (2, 3) for s in E.IM2COL_SHAPES]
TN_GATHER_CASES = [c for c in GATHER_CASES if c[0] != 3]      # xcp_gemm_tn gathers in modes 0 to 2


def gather_case(mode, shape, dt):
    return E.gather1_inputs(shape, dt) if mode == 1 else E.im2col_inputs(shape, mode, dt)


@pytest.mark.parametrize("mode,shape", GATHER_CASES, ids=str)
def test_gather_rows_against_torch_convs(mode, shape):
    """gather_rows (slices) times the weights equals fp64 F.conv2d(stride=S) / F.conv2d / F.conv_transpose2d:
    two independent statements of the operand, to fp64 rounding.  (The NaNs of the mode-1 frame become 1e3 for
    torch's conv: `gathered` has shown that the slices hold none of them.)"""
    d = gather_case(mode, shape, FP)
    H, W, OH, OW, S, gC = d["geom"]
    N, K, Co = shape[0], d["K"], d["N"]
    Bd = d["B"].double()
    got = E.gathered(d).double() @ Bd.t()
    x = d["A"].double().permute(0, 3, 1, 2)
    if mode == 1:
        want = F.conv2d(torch.nan_to_num(x[:, :K], nan=1e3), Bd.view(Co, K, 1, 1), stride=S)
    elif mode == 2:
        want = F.conv2d(x, Bd.view(Co, 3, 3, gC).permute(0, 3, 1, 2))
    else:
        want = F.conv_transpose2d(x, Bd.view(Co, 3, 3, gC).permute(3, 0, 1, 2))
    assert want.shape[0] * want.shape[2] * want.shape[3] == d["M"]
    torch.testing.assert_close(got.view(N, *want.shape[2:], Co).permute(0, 3, 1, 2), want, rtol=0, atol=1e-12)


def test_mode3_zero_taps():
    """at (1, 3, 3) every pixel of the 3 x 3 frame sees the single gradient pixel through exactly one tap"""
    d = E.im2col_inputs((1, 3, 3, 32), 3, FP)
    X = E.gathered(d).view(9, 9, 32)
    for p in range(9):
        assert [t for t in range(9) if X[p, t].abs().sum() > 0] == [p] and torch.equal(X[p, p], d["A"][0, 0, 0])


def emu_nt(A, B, order, dt):
    """fp32 products and sums in two orders, stored in dt"""
    A, B = A.float(), B.float()
    if order == 0:
        return (A @ B.t()).to(dt)
    h = A.shape[1] // 2
    return ((A[:, h:] @ B[:, h:].t()) + (A[:, :h] @ B[:, :h].t())).to(dt)


def emu_nt_stats(C, order, twice=None):
    """fp32 (sum, sum of squares) of the stored rows of each 128-row tile, the rows forward or reversed;
    twice: the planted defect, that row of the last tile added once more"""
    out = []
    for r in range(0, C.shape[0], 128):
        t = C[r:r + 128].float()
        if twice is not None and r + 128 >= C.shape[0]:
            t = torch.cat([t, C[twice:twice + 1].float()])
        if order:
            t = t.flip(0)
        acc = torch.zeros(2, C.shape[1])
        for row in t:                      # one fp32 addition per row, the square rounded to fp32 first
            acc[0] = acc[0] + row
            acc[1] = acc[1] + row * row
        out.append(acc)
    return torch.stack(out)


def emu_tn_slabs(G, X, rps, order):
    out = []
    for b, e in E.tn_splits(G.shape[0], rps):
        g, x = G[b:e].float(), X[b:e].float()
        if order:
            h = (e - b) // 2
            out.append(g[h:].flip(0).t() @ x[h:].flip(0) + g[:h].t() @ x[:h])
        else:
            out.append(g.t() @ x)
    return torch.stack(out)


def emu_reduce(P, base=None):
    """ops.reduce_slabs: the slabs summed in fp64 and rounded once; accumulate: one fp32 addition"""
    s = P.double().sum(0).float()
    return s if base is None else base + s


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode,shape", GATHER_CASES, ids=str)
def test_sound_gathered_nt(mode, shape, dt, order):
    d = gather_case(mode, shape, dt)
    X = E.gathered(d)
    ref, ab = E.gemm_nt_ref(X, d["B"])
    out = emu_nt(X, d["B"], order, dt)
    E.judge_gathered_nt(out, emu_nt_stats(out, order), ref, ab, d["K"])


def test_rows_per_split_restated():
    """the 128x128 kernel's own split: ceil(M / 256) splits at most (five of the 1083 rows, one of the 200)"""
    assert E.tn_rows_per_split_128(1083, 728, 256) == 224 and E.tn_rows_per_split_128(200, 1024, 728) == 224
    assert E.tn_rows_per_split_128(5000, 128, 64) == 256 and E.tn_rows_per_split_128(1, 8, 8) == 32
    assert E.tn_rows_per_split_128(92416, 728, 728) == 3328          # 28 splits of 36 tiles: 1008 workgroups


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("M,N,K", E.TN_SLAB_SHAPES)
def test_sound_dense_slabs(M, N, K, dt, order):
    G, X = E.gemm_tn_inputs(M, N, K, dt)
    for rps in sorted({r for _, r in E.TN_SLAB_FORMS}):
        ref, ab, n = E.gemm_tn_slabs_ref(G, X, rps)
        assert 4 <= len(n) <= 10 and n[-1] < rps           # several splits, the last one ragged
        E.assert_f32_sum(emu_tn_slabs(G, X, rps, order), ref, ab, n)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dt", [BF, FP], ids=["bf16", "fp32"])
@pytest.mark.parametrize("mode,shape", TN_GATHER_CASES, ids=str)
def test_sound_gathered_slabs_and_weight_grad(mode, shape, dt, order):
    d = gather_case(mode, shape, dt)
    X, G, M = E.gathered(d), d["G"], d["M"]
    assert M <= 1083
    wref, wab = E.gemm_tn_ref(G, X)
    base = torch.randn(d["N"], d["K"], generator=torch.Generator().manual_seed(M))
    for rps in (E.tn_rows_per_split_128(M, d["N"], d["K"]), 32):
        ref, ab, n = E.gemm_tn_slabs_ref(G, X, rps)
        P = emu_tn_slabs(G, X, rps, order)
        E.assert_f32_sum(P, ref, ab, n)
        E.assert_f32_sum(emu_reduce(P), wref, wab, M, extra=E.weight_grad_extra(wab))
        E.assert_f32_sum(emu_reduce(P, base), wref + base.double(), wab, M, extra=E.weight_grad_extra(wab, base))


# ------------------------------------------------------------------ sharp: gathered operands, slabs, stats rows
def nt_defect(mode, shape, plant):
    """(bad, ref, ab, K): the bf16 emulation of a gathered NT case with `plant(X, d)` applied to the dense
    operand; the clean emulation passes the element-wise measure"""
    d = gather_case(mode, shape, BF)
    X = E.gathered(d)
    ref, ab = E.gemm_nt_ref(X, d["B"])
    E.judge_gathered_nt(emu_nt(X, d["B"], 0, BF), None, ref, ab, d["K"])
    Xb = X.clone()
    plant(Xb, d)
    assert (Xb != X).any(1).sum() == 1 and (Xb != X).sum() <= 8          # one chunk of one row
    return emu_nt(Xb, d["B"], 0, BF), ref, ab, d["K"]


def test_sharp_mode1_chunk_from_the_pixel_to_the_right():
    """one 16-byte chunk (8 channels) of one output row read one pixel to the right of the sampled one -- an
    unsampled pixel, so the data is given there first.  1 row of 1083, 8 of 256 channels: 0.008 norm-wise."""
    n, oh, ow, c0 = 1, 7, 11, 104

    def plant(X, d):
        H, W, OH, OW, S, _ = d["geom"]
        right = torch.randn(8, generator=torch.Generator().manual_seed(5)).bfloat16()
        assert torch.isnan(d["A"][n, oh * S, ow * S + 1, c0:c0 + 8]).all()        # the neighbour is not sampled
        X[(n * OH + oh) * OW + ow, c0:c0 + 8] = right
    caught(*nt_defect(1, E.GATHER1_SHAPES[0], plant))


def test_sharp_mode2_last_tap_wraps_into_the_next_row():
    """the last pixel of a frame's row: one chunk of its tap (ky, kx) = (2, 2), column W - 1, taken from column 0
    of the row below, where W would be.  gC = 64: 8 of 576 columns of 1 row of 646."""
    n, oh, c0 = 1, 3, 40

    def plant(X, d):
        H, W, OH, OW, S, gC = d["geom"]
        X[(n * OH + oh) * OW + OW - 1, 8 * gC + c0:8 * gC + c0 + 8] = d["A"][n, oh + 3, 0, c0:c0 + 8]
    caught(*nt_defect(2, (2, 21, 19, 64), plant))


def test_sharp_mode3_corner_tap_from_the_neighbouring_frame():
    """pixel (0, 0) of frame 1 sees the gradient through tap (0, 0) alone; one chunk of its tap (1, 0) -- gradient
    row -1 -- taken from where that index lands, the last row of frame 0, instead of zero"""
    c0 = 16

    def plant(X, d):
        H, W, OH, OW, S, gC = d["geom"]
        assert (X[H * W, gC:] == 0).all()
        X[H * W, 3 * gC + c0:3 * gC + c0 + 8] = d["A"][0, OH - 1, 0, c0:c0 + 8]
    caught(*nt_defect(3, (2, 21, 19, 32), plant))


@pytest.mark.parametrize("dt,thr,scale", [(BF, 1e-3, 2.0 ** -6), (FP, 1e-5, 2.0 ** -13)], ids=["bf16", "fp32"])
@pytest.mark.parametrize("defect", ["twice", "dropped"])
def test_sharp_split_boundary_row(defect, dt, thr, scale):
    """The last row of a split counted in the next slab as well, or in neither, on the stride-2 skip conv's
    weight gradient (1083 rows, 34 splits of 32).  A whole row of ordinary size is 0.03 of dW's norm and the old
    measure (rel_err < 1e-3 bf16, 1e-5 fp32 on ops.weight_grad's output) sees it; gradients of a training step
    span orders of magnitude over the pixels, so the row is given a gradient of 2^-6 (2^-13) of the others'.
    The old measure passes; the slab it lands in (or is missing from) leaves the bound of its 32 rows' sum.  The
    bound of the whole sum (n = 1083) still holds the fp32 defect: the slabs are what sees it."""
    d = gather_case(1, E.GATHER1_SHAPES[0], dt)
    X, M, rps, s = E.gathered(d), d["M"], 32, 20
    m = (s + 1) * rps - 1                                   # the last row of split s
    G = d["G"].clone()
    G[m] = (G[m].float() * scale).to(dt)
    ref, ab, n = E.gemm_tn_slabs_ref(G, X, rps)
    P = emu_tn_slabs(G, X, rps, 0)
    E.assert_f32_sum(P, ref, ab, n)
    term = G[m].float()[:, None] * X[m].float()[None, :]
    bad = P.clone()
    if defect == "twice":
        bad[s + 1] += term
    else:
        bad[s] -= term
    wref, wab = E.gemm_tn_ref(G, X)
    assert rel_err(emu_reduce(bad), wref) < thr
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, ref, ab, n)
    if dt == FP:
        E.assert_f32_sum(emu_reduce(bad), wref, wab, M, extra=E.weight_grad_extra(wab))


def test_sharp_stats_row_counts_a_stored_row_twice():
    """the ragged last tile (59 rows of 1083) adds its last stored row twice: C itself is untouched, the
    normalised output the sums lead to passes rel_err < 1e-2, the stats row leaves its fp32 bound"""
    d = gather_case(1, E.GATHER1_SHAPES[0], BF)
    X, M = E.gathered(d), d["M"]
    C = emu_nt(X, d["B"], 0, BF)
    sref, sabs = E.nt_stats_ref(C)
    good, bad = emu_nt_stats(C, 0), emu_nt_stats(C, 0, twice=M - 1)
    E.assert_f32_sum(good, sref, sabs, 128)
    assert torch.equal(bad[:-1], good[:-1])

    def normalised(part):
        s = part.double().sum(0)
        mean = s[0] / M
        return ((C.double() - mean) / (s[1] / M - mean * mean + 1e-5).sqrt()).bfloat16()

    assert rel_err(normalised(bad).float(), normalised(sref)) < 1e-2
    with pytest.raises(AssertionError, match="outside the fp32 bound"):
        E.assert_f32_sum(bad, sref, sabs, 128)
