"""The bf16 kernels the bitwise chains of test_gpu_kernels.py rest on, element by element against
an fp64 restatement (tests/elementwise.py: every bound is derived there, none is fitted):
dw_fwd (tile, w2, 128-B-slice and tiny-frame kernels), dw_bwd (every launch form), the NT GEMMs
(128x128, 256x256, persistent) with their BN partial sums, the TN GEMMs and the fused unit backward;
then, with the same helper, the pooled block tail (BN'd and identity skip) and max-pool backward on non-square,
odd and tiny frames (E.POOL_SHAPES: down to 1 x 1, 8 to 1024 channels), the un-pooled block tail, the average
pool (HW from 100 down to 1), bn_act / bn_apply_coef and the stem conv3x3 forward.  The depthwise lists hold the
frames of the 299^2 family and the small and odd ones of the 64^2, 75^2, 224^2 and 256^2 families.
The shapes are the smallest ragged ones that reach each path; the inputs are generated on the CPU,
so test_elementwise_cpu.py has judged the measure on the same data.  Outputs start as NaN.

Every case prints one "ELEMENTWISE" line per output: the worst d/lim, and for bf16 outputs the
share rounded to nearest and the share excluded (profiles/elementwise_fp64_bounds.txt,
profiles/elementwise_small_frames.txt)."""
import pytest
import torch

import elementwise as E

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops(gpu):
    from xcp import ops as o
    o._lib.load()
    return o


def record(case, what, st):
    print(f"ELEMENTWISE {case} {what}: " + " ".join(f"{k}={v:.6g}" for k, v in st.items()), flush=True)


def to(d, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("shape", E.DW_FWD_SHAPES, ids=str)
def test_dw_fwd(ops, gpu, shape, act):
    N, C, H, W = shape
    d = to(E.dw_inputs(N, C, H, W), gpu)
    Y = torch.full((N, H, W, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.dw_fwd(act, d["x"], Y, d["wt"], d["scale"], d["shift"], N, H, W, C)
    torch.cuda.synchronize()
    ref, ab, extra = E.dw_fwd_ref(d["x"], d["wt"], act, d["scale"], d["shift"], E.dw_staged_bf16(W))
    case = f"dw_fwd {shape} act{act}"
    record(case, "Y", E.assert_bf16_stored(Y, ref, ab, 9, extra=extra, tag=case))


@pytest.mark.parametrize("form,act", E.DW_BWD_FORMS)
@pytest.mark.parametrize("shape", E.DW_BWD_SHAPES, ids=str)
def test_dw_bwd(ops, gpu, shape, form, act):
    """dX (<= 11 terms: nine taps, residual, skip), dW (N H W terms per tap) and, where the stored dX is what
    the sums are taken over (plain / skip_pre: the masked dz; res_bn_input: the final dX against Yb), the BN
    partial sums against the stored dX, as the kernel's comment says."""
    N, C, H, W = shape
    d = to(E.dw_inputs(N, C, H, W), gpu)
    res = d["dres"] if form in ("res", "res+skip", "resbn") else None
    skip = d["dskip"] if "skip" in form else None
    sums_of = {"plain": "x", "skip_pre": "x", "resbn": "yb"}.get(form) if act == 2 else None
    st = {"mean": d["mean"], "invstd": d["invstd"]} if sums_of else None
    dX = torch.full((N, H, W, C), NAN, device=gpu, dtype=torch.bfloat16)
    dW = torch.full((C * 9,), NAN, device=gpu)
    bnpart, P = ops.dw_bwd(act, d["dy"], d["x"], d["wt"], d["scale"], d["shift"], dX, dW, N, H, W, C, dRes=res,
                           dSkip=skip, skip_geom=(d["OH"], d["OW"], 2) if skip is not None else (0, 0, 1), bn_stats=st,
                           skip_pre=form == "skip_pre", res_bn_input=d["yb"] if form == "resbn" else None)
    torch.cuda.synchronize()
    r = E.dw_bwd_ref(d["dy"], d["x"], d["wt"], act, d["scale"], d["shift"], dres=res, dskip=skip,
                     skip_pre=form == "skip_pre")
    case = f"dw_bwd {shape} {form} act{act}"
    record(case, "dX", E.assert_bf16_stored(dX, r["dx"], r["dx_abs"], 11, exclude=r["dx_excl"], tag=case + " dX"))
    record(case, "dW", E.assert_f32_sum(dW.view(C, 9).t(), r["dw"], r["dw_abs"], N * H * W, tag=case + " dW"))
    if sums_of:
        ref, ab = E.bn_sums_ref(dX, d[sums_of], d["mean"], d["invstd"])
        sums = bnpart.view(P, 2, C).double().sum(0)
        record(case, "bnsums", E.assert_f32_sum(sums, ref, ab, N * H * W, tag=case + " BN sums"))


@pytest.mark.parametrize("tile", [1, 2, 3])
@pytest.mark.parametrize("shape", E.GEMM_NT_SHAPES, ids=str)
def test_gemm_nt(ops, gpu, shape, tile):
    """C within a bf16 neighbour of the fp64 product; stats row r = the fp32 sum / sum of squares of the
    stored rows [128 r, 128 r + 128) (a bf16 square is exact in fp32: 128 terms each)."""
    M, N, K, lda = shape
    Abuf, B = (t.to(gpu) for t in E.gemm_nt_inputs(M, N, K, lda))
    C = torch.full((M, N), NAN, device=gpu, dtype=torch.bfloat16)
    R = ops.nt_stat_rows(M)
    part = torch.full((R, 2, N), NAN, device=gpu)
    ops.gemm_nt(Abuf, B, C, M, N, K, lda=lda, stats=part, tile=tile)
    torch.cuda.synchronize()
    ref, ab = E.gemm_nt_ref(Abuf[:, :K], B)
    case = f"gemm_nt {shape} tile{tile}"
    record(case, "C", E.assert_bf16_stored(C, ref, ab, K, tag=case))
    Cd = torch.zeros(R * 128, N, device=gpu, dtype=torch.float64)
    Cd[:M] = C.double()
    Cd = Cd.view(R, 128, N)
    sref = torch.stack([Cd.sum(1), (Cd * Cd).sum(1)], 1)
    sabs = torch.stack([Cd.abs().sum(1), (Cd * Cd).sum(1)], 1)
    record(case, "stats", E.assert_f32_sum(part, sref, sabs, 128, tag=case + " stats"))


@pytest.mark.parametrize("tile", [2, 1, 0], ids=["tn256", "tn128", "auto"])
@pytest.mark.parametrize("shape", E.GEMM_TN_SHAPES, ids=str)
def test_gemm_tn(ops, gpu, shape, tile):
    M, N, K = shape
    g = torch.Generator().manual_seed(M + N)
    G = torch.randn(M, N, generator=g).bfloat16().to(gpu)
    X = torch.randn(M, K, generator=g).bfloat16().to(gpu)
    out = torch.full((N * K,), NAN, device=gpu)
    ops.weight_grad(G, X, M, N, K, out, tile=tile)
    torch.cuda.synchronize()
    ref, ab = E.gemm_tn_ref(G, X)
    case = f"gemm_tn {shape} tile{tile}"
    record(case, "dW", E.assert_f32_sum(out.view(N, K), ref, ab, M, tag=case))


@pytest.mark.parametrize("shape", E.UNIT_BWD_SHAPES, ids=str)
def test_unit_bwd(ops, gpu, shape):
    """dD = dY Wt^T over the restated dY = bf16(fmaf(alpha, G, fmaf(bcoef, Y, delta))) (CO terms, with the tie
    allowance through |Wt|), dW = dY^T X (M terms, the allowance through |X|), and the accumulate form."""
    M, CO, CI = shape
    g = torch.Generator().manual_seed(M + CO + CI)
    G = torch.randn(M, CO, generator=g).bfloat16().to(gpu)
    Y = torch.randn(M, CO, generator=g).bfloat16().to(gpu)
    coef = (torch.randn(3 * CO, generator=g) * 0.5).to(gpu)
    Wt = (torch.randn(CI, CO, generator=g) / CO ** 0.5).bfloat16().to(gpu)
    X = torch.randn(M, CI, generator=g).bfloat16().to(gpu)
    base = torch.randn(CO * CI, generator=g).to(gpu)
    dD = torch.full((M, CI), NAN, device=gpu, dtype=torch.bfloat16)
    dW = torch.full((CO * CI,), NAN, device=gpu)
    ops.unit_bwd(G, Y, coef, Wt, X, dD, M, CO, CI, dW)
    acc = base.clone()
    dD2 = torch.full_like(dD, NAN)
    ops.unit_bwd(G, Y, coef, Wt, X, dD2, M, CO, CI, acc, accumulate=True)
    torch.cuda.synchronize()
    dY, flip = E.unit_dy(G, Y, coef)
    case = f"unit_bwd {shape}"
    ref, ab = E.gemm_nt_ref(dY, Wt)
    record(case, "dD", E.assert_bf16_stored(dD, ref, ab, CO, extra=flip @ Wt.double().abs().t(), tag=case + " dD"))
    assert torch.equal(dD2, dD)
    wref, wab = E.gemm_tn_ref(dY, X)
    wextra = flip.t() @ X.double().abs()
    record(case, "dW", E.assert_f32_sum(dW.view(CO, CI), wref, wab, M, extra=wextra, tag=case + " dW"))
    b = base.view(CO, CI).double()
    record(case, "dW+=", E.assert_f32_sum(acc.view(CO, CI), wref + b, wab + b.abs(), M + 1, extra=wextra,
                                          tag=case + " dW accumulate"))


@pytest.mark.parametrize("bn_skip", [True, False], ids=["bn_skip", "identity_skip"])
@pytest.mark.parametrize("shape", E.POOL_SHAPES, ids=str)
def test_tail_maxpool(ops, gpu, shape, bn_skip):
    """Block tail out = maxpool3x3s2(fmaf(y, s1, t1)) + fmaf(skip, s2, t2) (two fp32 values, one fp32 add: n = 2;
    identity_skip: s2 = t2 = None, the skip added as it is) on frames whose windows hang over both edges, down to
    1 x 1, with odd OH / OW (the ragged output quad) and 8 to 1024 channels; the argmax bytes against the
    first-max rule, and maxpool_bwd (<= 4 windows per pixel) from those bytes."""
    N, C, H, W = shape
    d = to(E.pool_inputs(N, C, H, W), gpu)
    OH, OW = d["OH"], d["OW"]
    s2, t2 = (d["s2"], d["t2"]) if bn_skip else (None, None)
    out = torch.full((N, OH, OW, C), NAN, device=gpu, dtype=torch.bfloat16)
    amax = torch.full((N, OH, OW, C), 0xEE, device=gpu, dtype=torch.uint8)
    ops.tail_fwd(d["y"], d["s1"], d["t1"], True, d["ys"], s2, t2, out, amax, N, H, W, C)
    dz = torch.full((N, H, W, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.maxpool_bwd(d["d"], amax, dz, N, H, W, C)
    torch.cuda.synchronize()
    m, am = E.maxpool3s2_ref(E.fma32(d["y"], d["s1"], d["t1"]))
    sk = (E.fma32(d["ys"], s2, t2) if bn_skip else d["ys"]).double()
    case = f"tail_fwd {shape}{'' if bn_skip else ' identity_skip'}"
    record(case, "out", E.assert_bf16_stored(out, m.double() + sk, m.double().abs() + sk.abs(), 2, tag=case))
    assert torch.equal(amax, am), f"{case}: {(amax != am).sum().item()} argmax bytes differ from the first-max rule"
    ref, ab = E.maxpool3s2_bwd_ref(d["d"], am, H, W)
    case = f"maxpool_bwd {shape}{'' if bn_skip else ' identity_skip'}"
    record(case, "dz", E.assert_bf16_stored(dz, ref, ab, 4, tag=case))


@pytest.mark.parametrize("bn_skip", [False, True], ids=["identity_skip", "bn_skip"])
@pytest.mark.parametrize("shape", E.TAIL_PLAIN_SHAPES, ids=str)
def test_tail_plain(ops, gpu, shape, bn_skip):
    """The un-pooled block tail (tail_fwd_kernel, pool = 0): out = fmaf(y, s1, t1) + skip -- the residual add of the
    middle-flow blocks -- or + fmaf(skip, s2, t2); n = 2.  No argmax buffer is passed."""
    N, C, H, W = shape
    d = to(E.pool_inputs(N, C, H, W, pool=False), gpu)
    s2, t2 = (d["s2"], d["t2"]) if bn_skip else (None, None)
    out = torch.full((N, H, W, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.tail_fwd(d["y"], d["s1"], d["t1"], False, d["ys"], s2, t2, out, None, N, H, W, C)
    torch.cuda.synchronize()
    ref, ab = E.tail_plain_ref(d["y"], d["s1"], d["t1"], d["ys"], s2, t2)
    case = f"tail_plain {shape} {'bn_skip' if bn_skip else 'identity_skip'}"
    record(case, "out", E.assert_bf16_stored(out, ref, ab, 2, tag=case))


@pytest.mark.parametrize("N,C,HW", E.AVGPOOL_SHAPES)
def test_avgpool(ops, gpu, N, C, HW):
    """F = (sum_p max(fmaf(y, s, t), 0)) / HW in fp32 (HW terms, down to HW = 1); dz = bf16(mask * (dF * fp32(1 / HW)))
    (one exact-in-fp64 product), the mask excluded where fmaf's sign is within rounding of undecided."""
    g = torch.Generator().manual_seed(N + C + HW)
    y = torch.randn(N, HW, C, generator=g).bfloat16().to(gpu)
    s = (torch.rand(C, generator=g) + 0.5).to(gpu)
    t = torch.randn(C, generator=g).to(gpu)
    dF = torch.randn(N, C, generator=g).to(gpu)
    Fo = torch.full((N, C), NAN, device=gpu)
    ops.avgpool_fwd(y, s, t, Fo, N, HW, C)
    dz = torch.full((N, HW, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.avgpool_bwd(dF, y, s, t, dz, N, HW, C)
    torch.cuda.synchronize()
    z = E.fma32(y, s, t)
    a = z.clamp_min(0).double()
    case = f"avgpool ({N}, {C}, {HW})"
    record(case, "F", E.assert_f32_sum(Fo, a.sum(1) / HW, a.sum(1) / HW, HW, tag=case + " fwd"))
    inv = (torch.ones((), device=gpu) / HW).double()          # 1.f / (float)HW
    ref = (dF.double() * inv)[:, None, :] * (z > 0)
    record(case, "dz", E.assert_bf16_stored(dz, ref, ref.abs(), 1, exclude=E.fma_unsure(y, s, t), tag=case + " bwd"))


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,C", [(3 * 361, 728), (50, 2048), (5, 64)])
def test_bn_act_and_apply(ops, gpu, rows, C, relu):
    """bn_act: Y = bf16([relu] fmaf(x, s, t)) (2 terms); bn_apply_coef: dY = bf16(fmaf(alpha, dz', fmaf(bcoef, y,
    delta))) (3 terms), dz' masked by fmaf(y, scale, shift) > 0 when relu (excluded where undecided).  Row
    counts that are no multiple of the apply kernel's 2 / 4 rows per thread."""
    g = torch.Generator().manual_seed(rows + C)
    x = (torch.randn(rows, C, generator=g) * 2 + 0.7).bfloat16().to(gpu)
    dz = torch.randn(rows, C, generator=g).bfloat16().to(gpu)
    s = (torch.rand(C, generator=g) + 0.5).to(gpu)
    t = (torch.randn(C, generator=g) * 0.3).to(gpu)
    coef = (torch.randn(3 * C, generator=g) * 0.5).to(gpu)
    Y = torch.full((rows, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.bn_act(x, Y, s, t, relu, rows, C)
    dY = torch.full((rows, C), NAN, device=gpu, dtype=torch.bfloat16)
    ops.bn_apply_coef(dz, x, dY, coef, {"scale": s, "shift": t}, rows, C, relu=relu)
    torch.cuda.synchronize()
    xs, td = x.double() * s.double(), t.double()
    ref = xs + td
    case = f"bn ({rows}, {C}) relu{int(relu)}"
    record(case, "act", E.assert_bf16_stored(Y, ref.clamp_min(0) if relu else ref, xs.abs() + td.abs(), 2,
                                             tag=case + " bn_act"))
    al, bc, de = (coef[i * C:(i + 1) * C].double() for i in range(3))
    dzd = dz.double() * (E.fma32(x, s, t) > 0) if relu else dz.double()
    terms = (al * dzd, bc * x.double(), de.expand(rows, C))
    record(case, "apply", E.assert_bf16_stored(dY, sum(terms), sum(v.abs() for v in terms), 3,
                                               exclude=E.fma_unsure(x, s, t) if relu else None, tag=case + " bn_apply"))


@pytest.mark.parametrize("bn_on_load", [False, True])
@pytest.mark.parametrize("N,IH,IW", [(3, 21, 38), (1, 6, 147), (3, 3, 3)])
def test_conv3x3_fwd(ops, gpu, N, IH, IW, bn_on_load):
    """Stem conv2 forward (csrc/conv3.hip, 32 -> 64, 288 terms), plain and with BN1 + ReLU applied on load:
    a = bf16(max(fmaf(x, s, t), 0)) (c3_act), its tie allowance carried through |w|; the BN partial sums are
    the fp32 sums of the stored output (at most N OH OW terms per row)."""
    g = torch.Generator().manual_seed(IH * IW + N)
    x = torch.randn(N, IH, IW, 32, generator=g).bfloat16().to(gpu)
    w = (torch.randn(64, 32, 3, 3, generator=g) / 288 ** 0.5).bfloat16().to(gpu)
    s = (torch.rand(32, generator=g) + 0.5).to(gpu)
    t = (torch.randn(32, generator=g) * 0.3).to(gpu)
    OH, OW = IH - 2, IW - 2
    R = ops.conv3x3_parts(0, N, IH, IW)
    stats = torch.full((R, 2, 64), NAN, device=gpu)
    Y = torch.full((N, OH, OW, 64), NAN, device=gpu, dtype=torch.bfloat16)
    Wp = w.permute(0, 2, 3, 1).reshape(64, 9 * 32).contiguous()          # [co][tap][ci]
    kw = {"in_scale": s, "in_shift": t} if bn_on_load else {}
    ops.conv3x3(0, x, Wp, Y, stats, N, IH, IW, **kw)
    torch.cuda.synchronize()
    if bn_on_load:
        a32 = E.fma32(x, s, t).clamp_min(0)
        a, flip = a32.bfloat16().double(), E.tie_flip(a32)
    else:
        a, flip = x.double(), None
    ref, ab, extra = E.conv3x3_valid_ref(a, w, flip)
    case = f"conv3x3 ({N}, {IH}, {IW}) bn{int(bn_on_load)}"
    record(case, "Y", E.assert_bf16_stored(Y, ref, ab, 288, extra=extra, tag=case))
    Yd = Y.double().view(-1, 64)
    sref = torch.stack([Yd.sum(0), (Yd * Yd).sum(0)])
    sabs = torch.stack([Yd.abs().sum(0), (Yd * Yd).sum(0)])
    record(case, "stats", E.assert_f32_sum(stats.double().sum(0), sref, sabs, N * OH * OW, tag=case + " stats"))
