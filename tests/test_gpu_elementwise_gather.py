"""The gathered GEMMs (csrc/gemm.hip gather modes 1 to 3, NT and TN) and the split-K weight-gradient slabs,
element by element against the fp64 restatements of tests/elementwise.py: the gathered operand is
materialised by plain slicing (gather_rows, proven against torch's convolutions on the CPU), the product
and its `abs_terms` come from gemm_nt_ref / gemm_tn_ref, every bound is derived from the number of terms.

gemm_nt, mode 1 (the stride-2 skip conv): bf16 and fp32, with and without the BN partial sums, a K tail, a
pitch wider than K, M = 1, strides 1 to 3, and the skip convs of the small frames (29 -> 15 down to 2 -> 1, 450 to 3
rows) at the workload's channel counts.  Every element of A the gather must not read is NaN; A, like
every gathered operand here, sits between NaN margins; C and the partial sums start as NaN.
gemm_nt, modes 2 / 3 (conv2 forward and input gradient): one output pixel, one visible tap per pixel, M-tiles
that span frames, five frames in one tile, gC 8 / 32 / 64.
gemm_tn: every slab P[s] of the dense kernels (128x128; 256x256) at splits of 32 and
64 rows with a ragged last one, of the gathered kernel in modes 1 and 2 at the library's own split and at 32
rows; ops.weight_grad end to end, plain and accumulating.
The gather geometry guard of xcp_gemm_nt / xcp_gemm_tn: inconsistent calls are rejected before any launch.

The inputs are generated on the CPU (test_elementwise_cpu.py has judged the measure on the same data).
Every case prints one "ELEMENTWISE" line per output (profiles/elementwise_gather_gemm.txt,
profiles/elementwise_small_frames.txt)."""
import pytest
import torch

import elementwise as E

pytestmark = pytest.mark.gpu
NAN = float("nan")
BF, FP = torch.bfloat16, torch.float32
DTS = {"bf16": BF, "fp32": FP}
MARGIN = 4096      # elements of NaN before and after a gathered operand (keeps its 16-byte alignment)


@pytest.fixture(scope="module")
def ops(gpu):
    from xcp import ops as o
    o._lib.load()
    return o


def record(case, what, st):
    print(f"ELEMENTWISE {case} {what}: " + " ".join(f"{k}={v:.6g}" for k, v in st.items()), flush=True)


def nan(shape, dev, dt=FP):
    return torch.full(shape, NAN, device=dev, dtype=dt)


def between_nans(t, dev):
    """t on the device, as a view into a buffer that is NaN before and after it"""
    buf = nan((t.numel() + 2 * MARGIN,), dev, t.dtype)
    v = buf[MARGIN:MARGIN + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def on_gpu(d, dev):
    g = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    g["A"] = between_nans(d["A"], dev)
    return g


def run_nt(ops, d, stats, case):
    """C = gathered(A) B^T by the kernel, judged; -> (C, part)"""
    M, N, K = d["M"], d["N"], d["K"]
    dev = d["B"].device
    C = nan((M, N), dev, d["B"].dtype)
    part = nan((ops.nt_stat_rows(M), 2, N), dev) if stats else None
    ops.gemm_nt(d["A"], d["B"], C, M, N, K, lda=d["ld"], stats=part, gather=d["gather"])
    torch.cuda.synchronize()
    ref, ab = E.gemm_nt_ref(E.gathered(d), d["B"])
    st = E.judge_gathered_nt(C, part, ref, ab, K, tag=case)
    record(case, "C", st)
    return C, part


# ------------------------------------------------------------------ gemm_nt
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.GATHER1_SHAPES, ids=str)
def test_gemm_nt_mode1(ops, gpu, shape, dt, stats):
    """The strided 1x1 conv.  Nothing outside the sampled pixels' K channels is read (it is all NaN); the
    stride-1 form is bitwise the dense call."""
    d = on_gpu(E.gather1_inputs(shape, DTS[dt]), gpu)
    N, H, W, K, Cout, lda, S = shape
    assert (d["unread"] > 0) == (lda > K or (S > 1 and H * W > 1))
    assert int(torch.isnan(d["A"]).sum()) == d["unread"]          # the NaNs arrived on the device
    case = f"nt mode1 {shape} {dt} {'stats' if stats else 'plain'}"
    C, part = run_nt(ops, d, stats, case)
    if S == 1:
        C0 = nan(C.shape, gpu, C.dtype)
        part0 = nan(part.shape, gpu) if stats else None
        ops.gemm_nt(d["A"], d["B"], C0, d["M"], Cout, K, lda=lda, stats=part0)
        torch.cuda.synchronize()
        assert torch.equal(C0, C) and (not stats or torch.equal(part0, part))


@pytest.mark.parametrize("mode,stats", [(2, False), (2, True), (3, False)], ids=["mode2", "mode2-stats", "mode3"])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("shape", E.IM2COL_SHAPES, ids=str)
def test_gemm_nt_im2col(ops, gpu, shape, dt, mode, stats):
    """conv2 as an im2col GEMM (mode 2, 64 outputs, with the BN partial sums as the engine asks for them) and its
    input gradient (mode 3, 32 outputs: the taps that look outside the OH x OW frame are zero chunks); K terms
    at most"""
    d = on_gpu(E.im2col_inputs(shape, mode, DTS[dt]), gpu)
    run_nt(ops, d, stats, f"nt mode{mode} {shape} {dt} {'stats' if stats else 'plain'}")


# ------------------------------------------------------------------ gemm_tn
def run_slabs(ops, G, X, M, N, K, rps, case, Xg=None, **kw):
    """every P[s] of one xcp_gemm_tn call against G[mbeg:mend]^T X[mbeg:mend], n = the split's rows"""
    S = (M + rps - 1) // rps
    P = nan((S * N * K,), G.device)
    ops.gemm_tn(G, X, P, M, N, K, S, rps, **kw)
    torch.cuda.synchronize()
    ref, ab, n = E.gemm_tn_slabs_ref(G, X if Xg is None else Xg, rps)
    assert ref.shape[0] == S
    record(case, f"P[{S}]", E.assert_f32_sum(P.view(S, N, K), ref, ab, n, tag=case))


@pytest.mark.parametrize("form", [("bf16", 1, 32), ("bf16", 1, 64), ("fp32", 1, 32), ("fp32", 1, 64),
                                  ("bf16", 2, 64)], ids=str)
@pytest.mark.parametrize("shape", E.TN_SLAB_SHAPES, ids=str)
def test_gemm_tn_dense_slabs(ops, gpu, shape, form):
    """gemm_tn_kernel (tile 1) and the 256x256 kernel (tile 2: gemm_tn256q_kernel) at 4 to 10 splits with a
    ragged last one: mbeg / mend of every split"""
    M, N, K = shape
    dt, tile, rps = form
    assert (tile, rps) in E.TN_SLAB_FORMS
    G, X = (t.to(gpu) for t in E.gemm_tn_inputs(M, N, K, DTS[dt]))
    run_slabs(ops, G, X, M, N, K, rps, f"tn dense {shape} {dt} tile{tile} rps{rps}", tile=tile)


TN_GATHER_CASES = [(1, s) for s in E.GATHER1_SHAPES] + [(2, s) for s in E.IM2COL_SHAPES]


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("mode,shape", TN_GATHER_CASES, ids=str)
def test_gemm_tn_gathered(ops, gpu, mode, shape, dt):
    """The skip conv's and conv2's weight gradients: the slabs at the library's own split and at 32 rows, then
    ops.weight_grad against the fp64 sum over all M <= 1083 rows (n = M; the slab reduction's one fp32
    rounding per level and the accumulate form's addition go in as `extra`)."""
    d = E.gather1_inputs(shape, DTS[dt]) if mode == 1 else E.im2col_inputs(shape, mode, DTS[dt])
    d = on_gpu(d, gpu)
    M, N, K, G = d["M"], d["N"], d["K"], d["G"]
    Xg = E.gathered(d)
    kw = {"ldx": d["ld"], "gather": d["gather"]}
    own = ops._lib.call("xcp_gemm_tn_rows_per_split", ops.DT[DTS[dt]], mode, M, N, K, 0)
    assert own == E.tn_rows_per_split_128(M, N, K)
    case = f"tn mode{mode} {shape} {dt}"
    for rps in (own, 32):
        run_slabs(ops, G, d["A"], M, N, K, rps, f"{case} rps{rps}", Xg=Xg, **kw)
    assert M <= 1083
    ref, ab = E.gemm_tn_ref(G, Xg)
    out = nan((N * K,), gpu)
    ops.weight_grad(G, d["A"], M, N, K, out, **kw)
    base = torch.randn(N, K, generator=torch.Generator().manual_seed(M)).to(gpu)
    acc = base.clone()
    ops.weight_grad(G, d["A"], M, N, K, acc.view(-1), accumulate=True, **kw)
    torch.cuda.synchronize()
    record(case, "dW", E.assert_f32_sum(out.view(N, K), ref, ab, M, extra=E.weight_grad_extra(ab), tag=case))
    record(case, "dW+=", E.assert_f32_sum(acc, ref + base.double(), ab, M, extra=E.weight_grad_extra(ab, base),
                                          tag=case + " accumulate"))


# ------------------------------------------------------------------ the geometry guard
#           gather (mode, H, W, OH, OW, S, gC), M, K, ld
BAD_GEOMETRY = [((1, 9, 9, 5, 5, 2, 0), 49, 8, 8),        # M is no multiple of OH OW
                ((1, 9, 9, 6, 5, 2, 0), 60, 8, 8),        # (OH - 1) S > H - 1
                ((1, 9, 9, 5, 6, 2, 0), 60, 8, 8),        # (OW - 1) S > W - 1
                ((1, 9, 9, 5, 5, 2, 0), 50, 16, 8),       # K > ld
                ((1, 0, 9, 1, 5, 2, 0), 10, 8, 8),        # an extent of zero
                ((1, 9, 9, 5, -5, 2, 0), 50, 8, 8),       # a negative one
                ((2, 7, 7, 5, 5, 1, 8), 49, 72, 8),       # M is no multiple of OH OW
                ((2, 7, 7, 6, 5, 1, 8), 60, 72, 8),       # OH + 2 > H
                ((2, 7, 7, 5, 6, 1, 8), 60, 72, 8),       # OW + 2 > W
                ((2, 7, 7, 5, 0, 1, 8), 50, 72, 8),
                ((3, 7, 7, 5, 5, 1, 8), 97, 72, 8),       # mode 3: M is no multiple of H W
                ((3, 7, 7, 0, 5, 1, 8), 98, 72, 8)]


@pytest.mark.parametrize("gather,M,K,ld", BAD_GEOMETRY, ids=str)
def test_gather_geometry_guard(ops, gpu, gather, M, K, ld):
    """A gather that cannot be addressed inside the frames it describes is XCP_EINVAL (1001) from both entry
    points, before any launch: the outputs stay NaN.  (The operands are far larger than any of these geometries
    reaches; the calls every other test of this file makes are the accepted ones.)"""
    N = 16
    A, B, G = (torch.zeros(1 << 16, device=gpu, dtype=BF) for _ in range(3))
    C = nan((M * N,), gpu, BF)
    with pytest.raises(ops._lib.XcpError, match="xcp_gemm_nt failed with status 1001"):
        ops.gemm_nt(A, B, C, M, N, K, lda=ld, gather=gather)
    P = nan((2 * N * K,), gpu)
    if gather[0] != 3:
        with pytest.raises(ops._lib.XcpError, match="xcp_gemm_tn failed with status 1001"):
            ops.gemm_tn(G, A, P, M, N, K, 2, 32, ldx=ld, gather=gather)
    torch.cuda.synchronize()
    assert torch.isnan(C).all() and torch.isnan(P).all()
