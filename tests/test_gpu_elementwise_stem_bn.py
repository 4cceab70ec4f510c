"""The stem convolutions (csrc/stem.hip, csrc/conv3.hip) and the BatchNorm statistics chain (csrc/bn.hip),
element by element against the fp64 restatements of tests/elementwise.py: conv1 forward (row, tile and
per-pixel kernels), conv1_fwd_stats, the conv1 weight gradient in its three forms (plain, accumulate, BN1's
backward apply fused), the conv2 input gradient and its weight gradient in the three XCP_CONV3_WGRAD forms,
the channel reductions (row_stats, bn_bwd_reduce without and with the ReLU mask, maxpool_bwd_bnred at every
E.POOL_SHAPES frame, its dz judged here too), the
finalize kernels on partial rows the test writes (every R edge, padded pitch, a dead, a constant and a
far-from-zero channel), bn_act_strided and relu_bwd.

The inputs are generated on the CPU (test_elementwise_cpu.py has judged every bound on the same data), the
outputs start as NaN and are judged on the CPU by the same reference code.  Shapes are the smallest that
reach each path; where a launcher's arithmetic decides the path, elementwise.conv1_path restates it.

Every case prints one "ELEMENTWISE" line per output (profiles/elementwise_stem_bn.txt,
profiles/elementwise_small_frames.txt)."""
import pytest
import torch

import elementwise as E

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF, FP = torch.bfloat16, torch.float32
DTS = {"bf16": BF, "fp32": FP}


@pytest.fixture(scope="module")
def ops(gpu):
    from xcp import ops as o
    o._lib.load()
    return o


def record(case, what, st):
    print(f"ELEMENTWISE {case} {what}: " + " ".join(f"{k}={v:.6g}" for k, v in st.items()), flush=True)


def nan(shape, dev, dt=FP):
    return torch.full(shape, NAN, device=dev, dtype=dt)


# ------------------------------------------------------------------ conv1
def test_conv1_row_kernels_take_four_columns_or_more(ops):
    """xrow_chunks ends a row's last 16-B chunk at column IW - 1; a 3-wide frame has no room for one and goes
    through the tile kernels (a host call: nothing is launched)"""
    assert not ops.conv1_wgrad_fused(BF, 5, 3)
    assert ops.conv1_wgrad_fused(BF, 5, 4)
    assert not ops.conv1_wgrad_fused(FP, 5, 4) and not ops.conv1_wgrad_fused(BF, 5, 321)


def conv1_fwd_case(ops, gpu, dt, shape):
    N, IH, IW = shape
    d = E.conv1_inputs(*shape)
    x, w = d["x"].to(gpu), d["w"].to(gpu)
    Y = nan((N, d["OH"], d["OW"], 32), gpu, DTS[dt])
    ops.conv1_fwd(x, w, Y, N, IH, IW)
    torch.cuda.synchronize()
    path = E.conv1_path(dt == "bf16", IW)
    ref, ab, extra = E.conv1_ref(d["x"], d["w"], split=path == "row")
    case = f"conv1_fwd {shape} {dt} {path}"
    if dt == "bf16":
        record(case, "Y", E.assert_bf16_stored(Y.cpu(), ref, ab, 27, extra=extra, tag=case))
    else:
        record(case, "Y", E.assert_f32_sum(Y.cpu(), ref, ab, 27, tag=case))
    return d, x, w, Y


@pytest.mark.parametrize("shape", E.CONV1_ROW_SHAPES, ids=str)
def test_conv1_fwd_row(ops, gpu, shape):
    """The row kernel (split-bf16 MFMA products: conv1_ref's allowance) and, on the same shapes, conv1_fwd_stats:
    Y bitwise the plain forward's, partial row r the fp32 sums of the stored outputs of tiles r, r + R, ...
    (n = OW x the tiles of that workgroup)."""
    N, IH, IW = shape
    assert ops.conv1_wgrad_fused(BF, IH, IW)
    d, x, w, Y = conv1_fwd_case(ops, gpu, "bf16", shape)
    Y1 = nan(Y.shape, gpu, BF)
    part, R = ops.conv1_fwd_stats(x, w, Y1, N, IH, IW)
    torch.cuda.synchronize()
    assert torch.equal(Y1, Y)
    assert R == min(N * d["OH"], 1024)
    ref, ab, n = E.conv1_stats_ref(Y.cpu(), N, d["OH"], d["OW"], R)
    case = f"conv1_fwd_stats {shape}"
    record(case, "part", E.assert_f32_sum(part.view(R, 2, 32).cpu(), ref, ab, n, tag=case))


@pytest.mark.parametrize("dt,shape", E.CONV1_FWD_OTHER, ids=str)
def test_conv1_fwd_tile_and_pixel(ops, gpu, dt, shape):
    """The tile kernel (fp32 output; bf16 frames of 3 columns or more than 320, up to the 512 its LDS formula
    admits: (27 * 512 + 864) * 4 B <= 64 KB, the next pitch is not) and the per-pixel kernel: plain fp32 FMAs"""
    conv1_fwd_case(ops, gpu, dt, shape)


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.CONV1_WGRAD_SHAPES + [E.CONV1_WGRAD_SPARSE], ids=str)
def test_conv1_wgrad(ops, gpu, shape, dt, accumulate):
    """Row (bf16, X split: 2^-18 abs_terms), tile and per-pixel forms at <= 1100 output pixels; (70, 33, 9), 4480
    pixels on 560 workgroups of two tiles each, with the sparse gradient (elementwise.sparse_rows_gradient);
    accumulate: one more fp32 addition (n + 1)."""
    N, IH, IW = shape
    d = E.conv1_inputs(*shape)
    dy = d["dy"].to(DTS[dt])
    if shape == E.CONV1_WGRAD_SPARSE:
        dy = E.sparse_rows_gradient(dy, *E.conv1_wgrad_groups(*shape, dt == "bf16"))
    path = E.conv1_path(dt == "bf16", IW, True)
    base = torch.randn(32, 3, 3, 3, generator=torch.Generator().manual_seed(IW))
    out = base.to(gpu).flatten().clone() if accumulate else nan((32 * 27,), gpu)
    ops.conv1_wgrad(d["x"].to(gpu), dy.to(gpu), out, N, IH, IW, accumulate=accumulate)
    torch.cuda.synchronize()
    ref, ab, extra, n = E.conv1_wgrad_ref(d["x"], dy, split=path == "row")
    assert n <= 1100
    if accumulate:
        ref, ab, n = ref + base.double(), ab + base.double().abs(), n + 1
    case = f"conv1_wgrad {shape} {dt} {path}{' +=' if accumulate else ''}"
    record(case, "dW", E.assert_f32_sum(out.view(32, 3, 3, 3).cpu(), ref, ab, n, extra=extra, tag=case))


def test_conv1_wgrad_bn(ops, gpu):
    """conv1_wgrad_bn against the fp64 sum over the restated dC1 = bf16(fmaf(alpha, g, fmaf(bcoef, y, delta))), g =
    dZ masked by fmaf(y, ms, mt) > 0 (as E.unit_dy restates the unit backward's): its tie allowance, and |alpha dZ|
    where the mask's sign is within rounding of undecided, go through |x|."""
    N, IH, IW = shape = (5, 17, 23)
    d = E.conv1_inputs(*shape)
    OH, OW = d["OH"], d["OW"]
    rows = N * OH * OW
    g = torch.Generator().manual_seed(rows)
    dZ, Yv = (torch.randn(rows, 32, generator=g).bfloat16() for _ in range(2))
    coef = torch.randn(96, generator=g) * 0.5
    st = {"scale": torch.rand(32, generator=g) + 0.5, "shift": torch.randn(32, generator=g) * 0.3}
    out = nan((32 * 27,), gpu)
    ops.conv1_wgrad_bn(d["x"].to(gpu), dZ.to(gpu), Yv.to(gpu), coef.to(gpu), {k: v.to(gpu) for k, v in st.items()}, out,
                       N, IH, IW, 32, relu=True)
    torch.cuda.synchronize()
    mask = E.fma32(Yv, st["scale"], st["shift"]) > 0
    dC1, flip = E.unit_dy(dZ * mask, Yv, coef)
    unsure = E.fma_unsure(Yv, st["scale"], st["shift"])
    flip = flip + unsure * ((coef[:32].double() * dZ.double()).abs() + E.ulp_bf16(dC1.double()))
    ref, ab, extra, n = E.conv1_wgrad_ref(d["x"], dC1.view(N, OH, OW, 32), split=True, flip=flip.view(N, OH, OW, 32))
    case = f"conv1_wgrad_bn {shape}"
    record(case, "dW", E.assert_f32_sum(out.view(32, 3, 3, 3).cpu(), ref, ab, n, extra=extra, tag=case))


# ------------------------------------------------------------------ conv2 gradients
@pytest.mark.parametrize("shape", E.CONV3_DGRAD_SHAPES, ids=str)
def test_conv3x3_dgrad(ops, gpu, shape):
    """Every output row and column, the two-pixel border (1 to 6 taps) included; (1, 3, 147) is MAXIW_DGRAD"""
    N, OH, OW = shape
    d = E.conv3_inputs(N, OH, OW, 64)
    WT = d["w"].permute(1, 2, 3, 0).reshape(32, 9 * 64).contiguous()          # [ci][tap][co]
    DX = nan((N, OH + 2, OW + 2, 32), gpu, BF)
    ops.conv3x3(1, d["x"].to(gpu), WT.to(gpu), DX, None, N, OH, OW)
    torch.cuda.synchronize()
    ref, ab = E.conv3x3_dgrad_ref(d["x"], d["w"])
    case = f"conv3x3_dgrad {shape}"
    record(case, "dX", E.assert_bf16_stored(DX.cpu(), ref, ab, 576, tag=case))


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bn_on_load"])
@pytest.mark.parametrize("form", ["0", "1", "2"])
@pytest.mark.parametrize("shape", E.CONV3_WGRAD_SHAPES, ids=str)
def test_conv3x3_wgrad(ops, gpu, monkeypatch, shape, form, bn):
    """The three forms, plain and with BN1 + ReLU on load (a = bf16(relu(fma32(x, s, t))), its tie allowance
    carried through |dy|); 160 is the shifted forms' ring width, (1, 40, 34) has four bands of output rows"""
    monkeypatch.setenv("XCP_CONV3_WGRAD", form)
    N, IH, IW = shape
    d = E.conv3_wgrad_inputs(*shape)
    assert ops.conv3x3_wgrad_parts(N, IH, IW) > 0
    out = nan((64 * 288,), gpu)
    kw = {"in_scale": d["s"].to(gpu), "in_shift": d["t"].to(gpu)} if bn else {}
    ops.conv3x3_wgrad(d["dy"].to(gpu), d["x"].to(gpu), out, N, IH, IW, **kw)
    torch.cuda.synchronize()
    a, flip = E.bn_relu_on_load(d["x"], d["s"], d["t"]) if bn else (d["x"].double(), None)
    ref, ab, extra = E.conv3x3_wgrad_ref(d["dy"], a, flip)
    case = f"conv3x3_wgrad {shape} form{form} bn{int(bn)}"
    record(case, "dW", E.assert_f32_sum(out.view(64, 9, 32).cpu(), ref, ab, N * (IH - 2) * (IW - 2), extra=extra,
                                        tag=case))


# ------------------------------------------------------------------ channel reductions
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["row_stats", "bwd_reduce", "bwd_reduce_relu"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.CHAN_SHAPES, ids=str)
def test_chan_sums(ops, gpu, shape, dt, mode):
    """chanred_kernel: the fp64 sum of its partial rows against the fp64 sum of the terms (n = rows); rows below,
    at and off multiples of 8 SPB, CV below and above 64"""
    rows, C = shape
    d = E.chan_inputs(rows, C, DTS[dt])
    dev = {k: v.to(gpu) for k, v in d.items()}
    if mode == 0:
        part, R = ops.row_stats(dev["y"], rows, C)
        ref, ab, extra = E.chan_sums_ref(0, d["y"])
    else:
        R = ops._lib.call("xcp_chanred_parts", rows, C)
        part = nan((R * 2 * C,), gpu)
        ms, mt = (ops._p(dev["ms"]), ops._p(dev["mt"])) if mode == 2 else (0, 0)
        ops._lib.call("xcp_bn_bwd_reduce", ops.DT[DTS[dt]], ops._p(dev["dz"]), ops._p(dev["y"]), ops._p(dev["mean"]),
                      ops._p(dev["invstd"]), ms, mt, rows, C, ops._p(part), ops.stream())
        ref, ab, extra = E.chan_sums_ref(mode, d["dz"], d["y"], d["mean"], d["invstd"], d["ms"], d["mt"])
    torch.cuda.synchronize()
    case = f"chanred{mode} {shape} {dt} R{R}"
    record(case, "sums", E.assert_f32_sum(part.view(R, 2, C).double().sum(0).cpu(), ref, ab, rows, extra=extra, tag=case))


@pytest.mark.parametrize("shape", E.POOL_SHAPES, ids=str)
def test_maxpool_bwd_bnred(ops, gpu, shape):
    """dz bitwise maxpool_bwd's, and that dz against the fp64 scatter of the pooled gradient (<= 4 windows per pixel);
    the partial sums against the stored dz and y (n = N H W <= 1083).  maxpool_bwd_red_kernel walks SPB quads at a
    time, several whole frames at the 4 x 4, 2 x 2 and 1 x 1 cases; R is make_chanred's P as E.chanred_geo restates
    it."""
    N, C, H, W = shape
    d = E.pool_inputs(N, C, H, W, salt=1)
    OH, OW = d["OH"], d["OW"]
    y = d["y"]
    st = E.batch_stats(y)
    yg, ys, dOut = y.to(gpu), d["ys"].to(gpu), d["d"].to(gpu)
    s1, s2, t1, t2 = (d[k].to(gpu) for k in ("s1", "s2", "t1", "t2"))
    out = nan((N, OH, OW, C), gpu, BF)
    amax = torch.full((N, OH, OW, C), 0xEE, device=gpu, dtype=torch.uint8)
    ops.tail_fwd(yg, s1, t1, True, ys, s2, t2, out, amax, N, H, W, C)
    dz0, dz = nan((N, H, W, C), gpu, BF), nan((N, H, W, C), gpu, BF)
    ops.maxpool_bwd(dOut, amax, dz0, N, H, W, C)
    part, R = ops.maxpool_bwd_bnred(dOut, amax, dz, yg, {k: v.to(gpu) for k, v in st.items()}, N, H, W, C)
    torch.cuda.synchronize()
    assert R == E.chanred_geo(N * OH * OW, C)["P"]
    assert torch.equal(dz, dz0)
    _, am = E.maxpool3s2_ref(E.fma32(y, d["s1"], d["t1"]))
    assert torch.equal(amax.cpu(), am)
    zref, zab = E.maxpool3s2_bwd_ref(d["d"], am, H, W)
    case = f"maxpool_bwd_bnred {shape} R{R}"
    record(case, "dz", E.assert_bf16_stored(dz0.cpu(), zref, zab, 4, tag=case + " dz"))
    ref, ab = E.bn_sums_ref(dz.cpu(), y, st["mean"], st["invstd"])
    record(case, "sums", E.assert_f32_sum(part.view(R, 2, C).double().sum(0).cpu(), ref, ab, N * H * W, tag=case))


# ------------------------------------------------------------------ element-wise
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", E.BN_STRIDED_SHAPES, ids=str)
def test_bn_act_strided(ops, gpu, shape, relu):
    """Y[n, oh, ow] = bf16([relu] fmaf(X[n, 2 oh, 2 ow], s, t)): the bn_act bound (2 terms) on the strided pixels"""
    N, H, W, C = shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(H * W + C)
    x = (torch.randn(N, H, W, C, generator=g) * 2 + 0.7).bfloat16()
    s, t = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    Y = nan((N, OH, OW, C), gpu, BF)
    ops.bn_act_strided(x.to(gpu), Y, s.to(gpu), t.to(gpu), relu, N, H, W, OH, OW, 2, C)
    torch.cuda.synchronize()
    xs, td = x[:, ::2, ::2].double() * s.double(), t.double()
    ref = xs + td
    case = f"bn_act_strided {shape} relu{int(relu)}"
    record(case, "Y", E.assert_bf16_stored(Y.cpu(), ref.clamp_min(0) if relu else ref, xs.abs() + td.abs(), 2, tag=case))


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("rows,C", [(5, 64), (1083, 728)])
def test_relu_bwd(ops, gpu, rows, C, dt):
    """in place, bitwise torch.where(x > 0, dx, 0); x holds exact zeros and -0.0"""
    g = torch.Generator().manual_seed(rows + C)
    x = torch.randn(rows, C, generator=g)
    x[torch.rand(rows, C, generator=g) < 0.1] = 0.0
    x[torch.rand(rows, C, generator=g) < 0.1] = -0.0
    x, dx = x.to(DTS[dt]), torch.randn(rows, C, generator=g).to(DTS[dt])
    assert (x == 0).sum() > 0 and torch.signbit(x[x == 0]).any()
    got = dx.to(gpu).clone()
    ops.relu_bwd(got, x.to(gpu), rows, C)
    torch.cuda.synchronize()
    want = torch.where(x > 0, dx, torch.zeros_like(dx))
    bits = torch.int16 if dt == "bf16" else torch.int32
    assert torch.equal(got.cpu().view(bits), want.view(bits))


# ------------------------------------------------------------------ finalize kernels
def check(case, got, ref):
    for k, (r, b) in ref.items():
        record(case, k, E.assert_within(got[k].cpu(), r, b, tag=f"{case} {k}"))


@pytest.mark.parametrize("C,CP", E.FIN_CHANNELS)
@pytest.mark.parametrize("R", E.FIN_ROWS)
def test_finalize_stats(ops, gpu, R, C, CP):
    """bn_finalize_part_kernel on partial rows the test writes (fin_fwd_inputs), R at 1, around fin_reduce's 16
    waves and its 16 x 48-row pass, at FIN_MAX_ROWS and above it (ops._fold).  All six outputs against
    bn_finalize_ref; padding channels exactly zero; track=False leaves the buffers alone."""
    d = E.fin_fwd_inputs(R, C, CP)
    bn = {"weight": d["gamma"].to(gpu), "bias": d["beta"].to(gpu), "running_mean": d["rmean"].to(gpu),
          "running_var": d["rvar"].to(gpu), "eps": d["eps"], "momentum": d["momentum"], "track": True}
    out = {k: nan((CP,), gpu) for k in ("mean", "invstd", "scale", "shift")}
    ops.finalize_stats(d["part"].to(gpu), R, C, d["count"], bn, True, out, CP)
    torch.cuda.synchronize()
    got = {k: v[:C] for k, v in out.items()}
    got.update(running_mean=bn["running_mean"], running_var=bn["running_var"])
    ref = E.bn_finalize_ref(d["part"], d["count"], d["gamma"], d["beta"], d["rmean"], d["rvar"], d["momentum"], d["eps"])
    check(f"finalize_stats R{R} C{C}/{CP}", got, ref)
    for v in out.values():
        assert (v[C:] == 0).all()
    # the dead and the constant channel: var is exactly zero (their sums are small integers)
    is0 = (1 / torch.tensor(d["eps"], dtype=FP).double().sqrt()).float()
    assert out["invstd"][0].item() == is0.item() == out["invstd"][1].item()
    assert out["mean"][0].item() == 0.0 and out["mean"][1].item() == 3.0 and out["shift"][0].item() == d["beta"][0].item()
    bn2 = dict(bn, running_mean=d["rmean"].to(gpu), running_var=d["rvar"].to(gpu), track=False)
    out2 = {k: nan((CP,), gpu) for k in out}
    ops.finalize_stats(d["part"].to(gpu), R, C, d["count"], bn2, True, out2, CP)
    torch.cuda.synchronize()
    assert torch.equal(bn2["running_mean"].cpu(), d["rmean"]) and torch.equal(bn2["running_var"].cpu(), d["rvar"])
    for k in out:
        assert torch.equal(out2[k], out[k])


@pytest.mark.parametrize("C,CP", E.FIN_CHANNELS)
def test_eval_stats(ops, gpu, C, CP):
    """xcp_bn_finalize with train = 0: the running statistics as mean / var"""
    d = E.fin_fwd_inputs(1, C, CP)
    d["rvar"][0], d["rmean"][0] = 0.0, 0.0                     # a dead channel: invstd = fl32(1 / sqrt(eps))
    bn = {"weight": d["gamma"].to(gpu), "bias": d["beta"].to(gpu), "running_mean": d["rmean"].to(gpu),
          "running_var": d["rvar"].to(gpu), "eps": d["eps"], "momentum": d["momentum"], "track": True}
    out = {k: nan((CP,), gpu) for k in ("mean", "invstd", "scale", "shift")}
    ops.eval_stats(C, bn, out, gpu, CP)
    torch.cuda.synchronize()
    check(f"eval_stats C{C}/{CP}", {k: v[:C] for k, v in out.items()},
          E.bn_eval_ref(d["gamma"], d["beta"], d["rmean"], d["rvar"], d["eps"]))
    for v in out.values():
        assert (v[C:] == 0).all()
    assert torch.equal(bn["running_mean"].cpu(), d["rmean"]) and torch.equal(bn["running_var"].cpu(), d["rvar"])


@pytest.mark.parametrize("form", E.FIN_BWD_FORMS)
@pytest.mark.parametrize("C,CP", E.FIN_CHANNELS)
@pytest.mark.parametrize("R", E.FIN_ROWS)
def test_bn_backward_coef_from_partial_rows(ops, gpu, R, C, CP, form):
    """bn_bwd_finalize_part_kernel (16 waves; narrow: 4) on partial rows the test writes: alpha, bcoef, delta,
    dgamma, dbeta against bn_bwd_finalize_ref; frozen: bcoef = delta = 0 exactly; the coefficients of the padding
    channels are zero and dgamma / dbeta past C stay NaN."""
    d = E.fin_bwd_inputs(R, C, CP)
    acc, frozen = "accumulate" in form, "frozen" in form
    dg, db = nan((CP,), gpu), nan((CP,), gpu)
    if acc:
        dg[:C], db[:C] = d["dgamma0"].to(gpu), d["dbeta0"].to(gpu)
    st = {"mean": d["mean"].to(gpu), "invstd": d["invstd"].to(gpu)}
    dummy = torch.zeros(8, device=gpu, dtype=BF)
    coef = ops.bn_backward_coef(dummy, dummy, d["count"], C, {"weight": d["gamma"].to(gpu)}, st, dg, db,
                                part=d["part"].to(gpu), R=R, accumulate=acc, CP=CP, narrow="narrow" in form,
                                frozen=frozen)
    torch.cuda.synchronize()
    co = coef.view(3, CP)
    got = {"alpha": co[0, :C], "bcoef": co[1, :C], "delta": co[2, :C], "dgamma": dg[:C], "dbeta": db[:C]}
    ref = E.bn_bwd_finalize_ref(d["part"], d["count"], d["gamma"], d["mean"], d["invstd"], frozen,
                                (d["dgamma0"], d["dbeta0"]) if acc else None)
    check(f"bn_backward_coef R{R} C{C}/{CP} {form}", got, ref)
    assert (co[:, C:] == 0).all()
    assert torch.isnan(dg[C:]).all() and torch.isnan(db[C:]).all()
    if frozen:
        assert (co[1:] == 0).all()
