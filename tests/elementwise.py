"""Element-wise fp64 bounds for kernels that accumulate in fp32 and store bf16 or fp32.

The norm measure of test_gpu_kernels.py (rel_err < 1e-2 over the whole tensor) cannot see a
defect that holds less than 1e-4 of the output's energy: a tap dropped at one pixel, one wrong row
of a ragged tile.  The measure here is per element and has no fitted constant.

ref64      the kernel's expression evaluated in fp64 on the kernel's actual (already rounded) inputs
abs_terms  sum of |terms| of that expression, in fp64
n          number of terms

fp32 accumulation of n terms in ANY order (products by fma or rounded, n <= 2^20) gives a value v
with |v - ref64| <= e,

    e = (n + 2) * 2^-24 * abs_terms + extra

((n - 1) additions and up to one product rounding per term are n * 2^-24 to first order; the + 2
covers the second order for n <= 2^20 and one more rounding, e.g. of an fp32 store).  `extra` is what
a kernel-internal bf16 rounding that lies on a tie may move the expression by (see near_tie).

* stored in bf16 (assert_bf16_stored): the kernel stores one of the two bf16 neighbours of v, so
      |got - ref64| <= ulp_bf16(|ref64| + e) + e,        ulp_bf16(x) = 2^(floor(log2 x) - 7)
  (|got - v| < ulp_bf16(v) <= ulp_bf16(|ref64| + e)), and since e is far below an ulp, at least
  `nearest_floor` of the elements are ref64 rounded to nearest (0.99: the figure of
  test_gemm_nt_entry_flow_shapes_vs_fp64, whose `lim` this generalises).
* stored in fp32 (assert_f32_sum): |got - ref64| <= e.  This is only sharper than a dropped term
  (about abs_terms / n) while n^2 * 2^-24 << 1, so it is used for sums of n <~ 1100 terms.

Intermediates the kernels round to bf16 are restated with the kernel's own operations: a
bf16 x fp32 product is exact in fp64, so (x.double() * s.double() + t.double()).float() is the
kernel's fmaf(x, s, t) (up to fp64's own rounding of the sum, which can matter only within 2^-29 of
an fp32 tie).  An intermediate within 16 fp32 ulps (>= 2^-20 relative) of a bf16 rounding tie might
round the other way; its one-ulp flip goes into the bound through `extra`, carried through the
linear map that follows (3x3 taps, GEMM weights) -- no output is excluded for it.

`exclude` is for true discontinuities only (a ReLU mask whose argument is within rounding of zero,
max-pool ties); the share of excluded elements must be <= max_excluded: a condition on the test's
data (pick another seed), not a tolerance.

The references are plain tensor ops in fp64 (the depthwise one nine shifted slices of a zero-padded
tensor); they run on whatever device their inputs are on, so the CPU emulations of
test_elementwise_cpu.py and the kernels of test_gpu_elementwise.py are judged by the same code.
All image tensors are NHWC.

The second half (stem conv1 / conv2 gradients, channel reductions, BN finalize kernels) serves
test_gpu_elementwise_stem_bn.py, which judges the kernels' outputs on the CPU: the conv references are fp64
F.conv2d / conv2d_weight there.  Two more allowances are derived next to their references: the split-bf16
products of the conv1 row kernels (conv1_ref) and the per-output rounding counts of the finalize kernels
(bn_finalize_ref, bn_bwd_finalize_ref; judged by assert_within, since their bounds are not sums of n terms).

The gathered GEMMs and the split-K slabs (test_gpu_elementwise_gather.py) need no new bound: gather_rows
materialises the gathered operand by slicing, gemm_nt_ref / gemm_tn_ref give (ref64, abs_terms) with n = K
(n = the split's rows for a slab, n <= 128 for a stats row), and weight_grad_extra counts the roundings of
the slab reduction.
"""
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32
TIE_ULPS32 = 16           # |fp32 value - bf16 tie| in fp32 ulps that counts as "near a tie" (2^-20 relative or more)


def ulp_bf16(v):
    """spacing of bf16 at |v| (fp64 tensor): 2^(floor(log2 |v|) - 7); zero -> the smallest normal's"""
    _, e = torch.frexp(v.double().abs().clamp_min(2.0 ** -126))   # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - 8)


def near_tie(v32):
    """fp32 tensor -> bool: within TIE_ULPS32 fp32 ulps of a midpoint between two bf16 values"""
    assert v32.dtype == torch.float32
    low = v32.contiguous().view(torch.int32) & 0xFFFF
    return (low - 0x8000).abs() <= TIE_ULPS32


def tie_flip(v32):
    """what rounding v32 to bf16 the other way would move it by: ulp_bf16 where near a tie, else 0 (fp64)"""
    return near_tie(v32).double() * ulp_bf16(v32.double())


def _where(t, flat):
    return tuple(int(i) for i in torch.unravel_index(torch.as_tensor(flat), t.shape))


def assert_bf16_stored(got, ref64, abs_terms, n, extra=None, nearest_floor=0.99, exclude=None, max_excluded=1e-4,
                       tag=""):
    """See the module docstring.  Returns {"worst": max d/lim, "nearest": share, "excluded": share}."""
    assert ref64.dtype == torch.float64 and abs_terms.dtype == torch.float64
    assert got.shape == ref64.shape == abs_terms.shape, (got.shape, ref64.shape, abs_terms.shape)
    g = got.double()
    assert not torch.isnan(g).any(), f"{tag}: NaN at {_where(g, torch.isnan(g).flatten().nonzero()[0, 0])}"
    e = abs_terms * ((n + 2) * U32)
    if extra is not None:
        e = e + extra
    lim = ulp_bf16(ref64.abs() + e) + e
    d = (g - ref64).abs()
    keep = torch.ones_like(d, dtype=torch.bool) if exclude is None else ~exclude
    excluded = 0.0 if exclude is None else exclude.double().mean().item()
    assert excluded <= max_excluded, f"{tag}: {excluded:.3g} of the elements excluded (max {max_excluded})"
    ratio = torch.where(keep, d / lim, torch.zeros_like(d))
    worst, at = ratio.flatten().max(0)
    worst = worst.item()
    nearest = ((g == ref64.to(torch.bfloat16).double()) | ~keep).double().mean().item()
    stats = {"worst": worst, "nearest": nearest, "excluded": excluded}
    if worst > 1.0:
        idx = _where(d, at)
        bad = int((ratio > 1.0).sum())
        raise AssertionError(f"{tag}: {bad} element(s) outside the bf16-neighbour bound; worst d/lim = {worst:.3f} "
                             f"at {idx}: got {g[idx].item()!r}, fp64 {ref64[idx].item()!r}, lim {lim[idx].item():.3g}")
    assert nearest >= nearest_floor, f"{tag}: only {nearest:.4f} of the elements rounded to nearest (min {nearest_floor})"
    return stats


def assert_f32_sum(got, ref64, abs_terms, n, extra=None, tag=""):
    """fp32-stored sum of n terms: |got - ref64| <= (n + 2) 2^-24 abs_terms (+ extra).  Returns {"worst": ...}."""
    assert ref64.dtype == torch.float64 and abs_terms.dtype == torch.float64
    assert got.shape == ref64.shape == abs_terms.shape, (got.shape, ref64.shape, abs_terms.shape)
    g = got.double()
    assert not torch.isnan(g).any(), f"{tag}: NaN at {_where(g, torch.isnan(g).flatten().nonzero()[0, 0])}"
    lim = abs_terms * ((n + 2) * U32)
    if extra is not None:
        lim = lim + extra
    d = (g - ref64).abs()
    ratio = torch.where(d == 0, torch.zeros_like(d), d / lim.clamp_min(1e-300))
    worst, at = ratio.flatten().max(0)
    worst = worst.item()
    if worst > 1.0:
        idx = _where(d, at)
        raise AssertionError(f"{tag}: {int((ratio > 1.0).sum())} sum(s) outside the fp32 bound; worst d/lim = "
                             f"{worst:.3f} at {idx}: got {g[idx].item()!r}, fp64 {ref64[idx].item()!r}, "
                             f"lim {lim[idx].item():.3g}")
    return {"worst": worst}


# ------------------------------------------------------------------ depthwise 3x3 (stride 1, pad 1), NHWC
def dw3x3(a, w, transposed=False):
    """a [N,H,W,C] fp64, w [9,C] fp64 (tap = ky*3 + kx): out[h,w] = sum_tap a[h+ky-1, w+kx-1] w[tap];
    transposed: out[h,w] = sum_tap a[h-ky+1, w-kx+1] w[tap].  Nine shifted slices of the zero-padded tensor."""
    N, H, W, C = a.shape
    p = F.pad(a, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(a)
    for ky in range(3):
        for kx in range(3):
            oy, ox = (2 - ky, 2 - kx) if transposed else (ky, kx)
            out += p[:, oy:oy + H, ox:ox + W] * w[ky * 3 + kx]
    return out


def dw3x3_wgrad(dy, a):
    """(dW [9,C], sum of |terms| [9,C]): dW[tap] = sum_p dy[p] a[p + off(tap)]"""
    N, H, W, C = a.shape
    p = F.pad(a, (0, 0, 1, 1, 1, 1))
    dw, ab = [], []
    for ky in range(3):
        for kx in range(3):
            t = dy * p[:, ky:ky + H, kx:kx + W]
            dw.append(t.sum((0, 1, 2)))
            ab.append(t.abs().sum((0, 1, 2)))
    return torch.stack(dw), torch.stack(ab)


class Act:
    """The depthwise kernels' input transform (csrc/dwconv.hip act1 / stage), restated exactly.
    z   fp32: fmaf(x, scale, shift) (act 2), else x
    a32 fp32: the activated value before any storage rounding
    a   fp64: the value the taps multiply: bf16(a32) when the kernel stages it in bf16 (round_bf16), else a32
    flip fp64: the possible one-ulp flip of that bf16 rounding (zero elsewhere)
    unsure bool: the ReLU argument is within rounding of zero (|z| <= 2^-22 (|x s| + |t|))"""

    def __init__(self, x, act, scale, shift, round_bf16):
        xd = x.double()
        if act == 2:
            self.z = (xd * scale.double() + shift.double()).float()
            self.unsure = self.z.double().abs() <= 2.0 ** -22 * ((xd * scale.double()).abs() + shift.double().abs())
        else:
            self.z = x.float()
            self.unsure = torch.zeros_like(self.z, dtype=torch.bool)
        self.a32 = self.z.clamp_min(0) if act else self.z
        self.flip = torch.zeros_like(xd)
        self.a = self.a32.double()
        if round_bf16 and act == 2:   # (act 0 / 1: a bf16 input is its own rounding)
            self.a = self.a32.bfloat16().double()
            self.flip = tie_flip(self.a32)
        self.mask = (self.z > 0) if act else torch.ones_like(self.z, dtype=torch.bool)


def dw_fwd_ref(x, wt, act, scale, shift, round_bf16):
    """-> (ref64, abs_terms, extra) of Y = dw3x3(act(x)), 9 terms.  (max(z, 0) is continuous: nothing to exclude.)"""
    A = Act(x, act, scale, shift, round_bf16)
    w = wt.double()
    return dw3x3(A.a, w), dw3x3(A.a.abs(), w.abs()), dw3x3(A.flip, w.abs())


def upsample_skip(dskip, H, W, stride):
    N, OH, OW, C = dskip.shape
    up = torch.zeros(N, H, W, C, dtype=torch.float64, device=dskip.device)
    up[:, ::stride, ::stride] = dskip.double()
    return up


def dw_bwd_ref(dy, x, wt, act, scale, shift, dres=None, dskip=None, stride=2, skip_pre=False):
    """The fused backward of csrc/dwconv.hip (header of the "Fused backward" section), fp64:
      dX = mask * (dw3x3^T(dY) [+ skip if skip_pre]) + dRes [+ skip if not skip_pre]      (<= 11 terms)
      dW[tap] = sum_p dY[p] a32[p + off(tap)]   (the backward multiplies the UNROUNDED fp32 activation)
    -> dict(dx, dx_abs, dx_excl, dw [9,C], dw_abs, act)"""
    N, H, W, C = x.shape
    A = Act(x, act, scale, shift, False)
    w = wt.double()
    g = dy.double()
    s = dw3x3(g, w, transposed=True)
    ab = dw3x3(g.abs(), w.abs(), transposed=True)
    up = upsample_skip(dskip, H, W, stride) if dskip is not None else None
    if up is not None and skip_pre:
        s, ab = s + up, ab + up.abs()
    m = A.mask.double()
    s, ab = s * m, ab * m
    if dres is not None:
        s, ab = s + dres.double(), ab + dres.double().abs()
    if up is not None and not skip_pre:
        s, ab = s + up, ab + up.abs()
    dw, dw_abs = dw3x3_wgrad(g, A.a32.double())
    return {"dx": s, "dx_abs": ab, "dx_excl": A.unsure, "dw": dw, "dw_abs": dw_abs, "act": A}


def bn_sums_ref(dz, src, mean, invstd):
    """The BN-backward partial sums as the kernel takes them: over the STORED dz, against
    zhat = (src - mean) * invstd computed in fp32 (two roundings, the same two operations here).
    -> (sums [2,C] fp64, abs [2,C])"""
    zhat = ((src.float() - mean) * invstd).double()
    d = dz.double()
    t = d * zhat
    return torch.stack([d.sum((0, 1, 2)), t.sum((0, 1, 2))]), torch.stack([d.abs().sum((0, 1, 2)), t.abs().sum((0, 1, 2))])


# ------------------------------------------------------------------ GEMMs
def gemm_nt_ref(A, B):
    """C = A B^T, K terms -> (ref64, abs_terms)"""
    return A.double() @ B.double().t(), A.double().abs() @ B.double().abs().t()


def gemm_tn_ref(G, X):
    """out[N][K] = G^T X, M terms -> (ref64, abs_terms)"""
    return G.double().t() @ X.double(), G.double().abs().t() @ X.double().abs()


def gather_rows(x, mode, geom):
    """The gathered GEMM operand as a dense [M, K] tensor (x's dtype), by slicing the NHWC tensor: the header of
    `Gather` in csrc/gemm.hip restated without its index arithmetic.  geom = (H, W, OH, OW, S, Cg), the gather
    tuple the ops take after the mode; x holds the K = C channels that are read (a wider pitch is sliced off by
    the caller).
      mode 1  x [N,H,W,C]:   row (n, oh, ow) = pixel (n, oh S, ow S); K = C
      mode 2  x [N,H,W,C]:   row (n, oh, ow), column tap C + c = pixel (n, oh + ky, ow + kx), tap = 3 ky + kx; K = 9 C
      mode 3  x [N,OH,OW,C]: row (n, h, w) over H x W, column tap C + c = pixel (n, h - ky, w - kx) of the OH x OW
              frame, zero outside it; K = 9 C"""
    H, W, OH, OW, S, Cg = geom
    N, C = x.shape[0], x.shape[3]
    if mode == 1:
        assert x.shape[1:3] == (H, W)
        rows = x[:, ::S, ::S]
        assert rows.shape[1:3] == (OH, OW), (rows.shape, geom)
        return rows.reshape(N * OH * OW, C)
    assert Cg == C and (OH, OW) == (H - 2, W - 2), geom
    if mode == 2:
        assert x.shape[1:3] == (H, W)
        return torch.cat([x[:, ky:ky + OH, kx:kx + OW] for ky in range(3) for kx in range(3)], 3).reshape(-1, 9 * C)
    assert mode == 3 and x.shape[1:3] == (OH, OW)
    p = F.pad(x, (0, 0, 2, 2, 2, 2))                      # p[h + 2, w + 2] = x[h, w], zero outside
    return torch.cat([p[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W] for ky in range(3) for kx in range(3)],
                     3).reshape(-1, 9 * C)


def nt_stats_ref(C, rows=128):
    """gemm_nt's BN partial sums: row r = (sum, sum of squares) over the STORED C rows [128 r, 128 r + 128) below M
    -> (ref64 [R,2,N], abs_terms), n <= 128 (a bf16 square is exact in fp32; an fp32 one is the term's one
    product rounding)"""
    M, N = C.shape
    R = (M + rows - 1) // rows
    Cd = torch.zeros(R * rows, N, dtype=torch.float64, device=C.device)
    Cd[:M] = C.double()
    Cd = Cd.view(R, rows, N)
    q = (Cd * Cd).sum(1)
    return torch.stack([Cd.sum(1), q], 1), torch.stack([Cd.abs().sum(1), q], 1)


def judge_gathered_nt(C, part, ref, ab, K, tag=""):
    """What both files assert of a gathered NT product (bf16 C: a bf16 neighbour, >= 99 % nearest, nothing excluded
    -- these kernels have no ReLU mask; fp32 C: the fp32-sum bound) and of its partial sums (part, or None)
    -> {"worst", ["nearest", "excluded",] ["stats"]}"""
    if C.dtype == torch.bfloat16:
        st = assert_bf16_stored(C, ref, ab, K, nearest_floor=0.99, exclude=None, tag=tag)
        assert st["excluded"] == 0 and st["nearest"] >= 0.99
    else:
        st = assert_f32_sum(C, ref, ab, K, tag=tag)
    if part is not None:
        sref, sabs = nt_stats_ref(C)
        st["stats"] = assert_f32_sum(part, sref, sabs, 128, tag=tag + " stats")["worst"]
    return st


def tn_splits(M, rps):
    """[(mbeg, mend)] of xcp_gemm_tn's S = ceil(M / rps) row splits"""
    return [(b, min(M, b + rps)) for b in range(0, M, rps)]


def tn_rows_per_split_128(M, N, K):
    """xcp_gemm_tn_rows_per_split for the 128x128 kernel (every fp32 or gathered call), restated: about 1024
    workgroups, splits of 256 rows or more, rounded up to 32 (the GPU file asserts it equals the library's)"""
    cdiv = lambda a, b: -(-a // b)
    S = max(1, min(1024 // (cdiv(N, 128) * cdiv(K, 128)), cdiv(M, 256)))
    return cdiv(cdiv(M, S), 32) * 32


def gemm_tn_slabs_ref(G, X, rps):
    """P[s] = G[mbeg:mend]^T X[mbeg:mend] -> (ref64 [S,N,K], abs_terms, n [S,1,1] = the rows of split s)"""
    Gd, Xd = G.double(), X.double()
    sp = tn_splits(G.shape[0], rps)
    ref = torch.stack([Gd[b:e].t() @ Xd[b:e] for b, e in sp])
    ab = torch.stack([Gd[b:e].abs().t() @ Xd[b:e].abs() for b, e in sp])
    n = torch.tensor([e - b for b, e in sp], dtype=torch.float64, device=G.device).view(-1, 1, 1)
    return ref, ab, n


REDUCE_LEVELS = 2         # ops.reduce_slabs: fp64 sums of the slabs rounded to fp32 once per level, two levels at most


def weight_grad_extra(ab, base=None):
    """What ops.weight_grad's slab reduction adds to the (M + 2) 2^-24 abs_terms of the slabs' own sums: one fp32
    rounding per reduction level, and for the accumulate form (base) one fp32 addition.  |value| <= abs_terms."""
    if base is None:
        return ab * (REDUCE_LEVELS * U32)
    return (ab + base.double().abs()) * ((REDUCE_LEVELS + 1) * U32)


def unit_dy(G, Y, coef):
    """csrc/unitbwd.hip stage_tile: dY = bf16(fmaf(alpha, G, fmaf(bcoef, Y, delta))) -> (dY bf16, flip fp64)"""
    CO = G.shape[1]
    al, bc, de = (coef[i * CO:(i + 1) * CO].double() for i in range(3))
    inner = (bc * Y.double() + de).float()
    outer = (al * G.double() + inner.double()).float()
    return outer.bfloat16(), tie_flip(outer)


# ------------------------------------------------------------------ the cases (shared by the CPU and the GPU file)
# N, C, H, W
DW_FWD_SHAPES = [(2, 64, 17, 41),      # tile_geo: ntw 2, TW 21, WP 27, nth 2: 2 x 2 ragged tiles, ragged last segment
                 (8, 728, 19, 19),     # N % 8 == 0: frames dealt to the XCDs (fwd_item_id); last group 24 of 32 channels
                 (3, 728, 19, 19),     # the xcd_remap order
                 (2, 72, 5, 9),        # W = 9: the narrowest frame past dwframe.hip's W <= 8 gate (W = 3, 5, 6, 7 are
                                       # not among its widths and reach the tile kernels too: below); last group 8 channels
                 (3, 1536, 10, 10),    # 128-B slices
                 (3, 200, 7, 8), (5, 728, 3, 4), (2, 64, 1, 2),   # dwframe.hip (fp32 windows: no bf16 staging)
                 # the small and odd frames of the 64^2, 75^2, 224^2 and 256^2 families
                 (40, 728, 1, 1),      # dwframe W = 1 (a 1 x 1 exit): only the centre tap sees the frame
                 (16, 1536, 2, 2),     # dwframe W = 2: the 64^2 exit flow, every pixel a corner
                 (6, 728, 4, 4),       # dwframe W = 4: the 64^2 middle flow
                 (3, 728, 5, 3),       # 75^2 exit: W = 3 is not a dwframe width -> tile kernel, one 5-pixel segment of 3
                 (4, 1024, 3, 3),      # 75^2 exit, 128-B slices (2 C % 128 == 0): dw_fwd_kernel, 3 x 3
                 (2, 64, 6, 7),        # W = 7, H = 6, 128-B slices with a single group of 64 channels
                 (2, 72, 1, 9),        # H = 1 in the tile kernel: both halo rows are padding
                 (3, 728, 7, 7),       # 224^2 exit flow: tile kernel, two segments 5 + 2
                 (3, 256, 15, 15),     # 64^2 entry flow (256 channels: 17 x 17 > 256 halo pixels, so 64-B slices)
                 (2, 128, 29, 29)]     # 64^2 entry flow: WP 32, three row tiles 10 + 10 + 9
DW_BWD_SHAPES = [(2, 72, 9, 21),       # two column groups, 20 + 1
                 (2, 64, 64, 5),       # three row bands
                 (3, 728, 19, 19),
                 (2, 128, 15, 15),
                 # the frames below 9 x 21: one row band and (up to 15 x 8) one 20-column group, most or all pixels
                 # edge pixels; the skip forms see a 1 x 1, 2 x 2, 3 x 2, ... dskip
                 (40, 728, 1, 1),      # H = 1: dY rows -1 and 1 are both padding, one live column of the 22 staged
                 (16, 1536, 2, 2),     # 64^2 exit flow (1536 channels)
                 (8, 1024, 2, 2),      # 64^2 exit flow (1024 channels)
                 (6, 728, 4, 4),       # 64^2 middle flow
                 (3, 728, 5, 3),       # 75^2 exit, non-square
                 (4, 1024, 3, 3),      # 75^2 exit
                 (3, 728, 7, 7),       # 224^2 exit flow
                 (2, 128, 8, 8),       # 256^2 / 64^2: 8 x 8
                 (2, 256, 15, 8),      # non-square, odd x even: dskip 8 x 4
                 (1, 128, 29, 29)]     # 64^2 entry flow: two column groups 20 + 9, dskip 15 x 15
# form, act
DW_BWD_FORMS = [("plain", 0), ("plain", 1), ("plain", 2), ("res", 1), ("skip", 2), ("res+skip", 1), ("resbn", 2),
                ("skip_pre", 2)]
# M, N, K, lda
GEMM_NT_SHAPES = [(256, 256, 32, 32), (1000, 728, 728, 728), (300, 2048, 1536, 1536), (77, 64, 288, 288),
                  (513, 264, 40, 40), (4100, 1024, 728, 1456)]
GEMM_TN_SHAPES = [(229, 256, 264), (33, 512, 2048), (300, 2048, 1536)]
UNIT_BWD_SHAPES = [(M, CO, CI) for M in (453, 1000) for CO, CI in ((128, 128), (128, 64), (256, 128), (256, 256))]
# gather mode 1 (strided 1x1 conv): N, H, W, Cin, Cout, lda, S
GATHER1_SHAPES = [(3, 37, 37, 256, 728, 256, 2),     # 1083 rows: 9 M-tiles, the last of 59 rows; 6 N-tiles, the last ragged
                  (2, 19, 20, 728, 1024, 736, 2),    # K = 11 * 64 + 24, pitch wider than K, even W: the last column never sampled
                  (2, 10, 7, 8, 8, 8, 2),            # one 16-byte bf16 chunk per row
                  (1, 1, 1, 64, 64, 64, 2),          # M = 1
                  (2, 11, 8, 40, 24, 48, 3),         # stride 3: 4 x 3 of 11 x 8, pitch 48
                  (2, 5, 9, 72, 136, 72, 1),         # stride 1: bitwise the dense call
                  # the skip convs of the 64^2 family (and 256^2's 8 -> 4) at the workload's channel counts
                  (2, 29, 29, 64, 128, 64, 2),       # 29 -> 15: 450 rows, K = one 64-column stage
                  (3, 15, 15, 128, 256, 128, 2),     # 15 -> 8: 192 rows, odd W: the last column is sampled
                  (4, 8, 8, 256, 728, 256, 2),       # 8 -> 4: 64 rows (half an M-tile), even W
                  (5, 4, 4, 728, 1024, 736, 2),      # 4 -> 2: 20 rows, K tail of 24, pitch 736
                  (3, 2, 2, 728, 1024, 736, 2)]      # 2 -> 1: 3 rows, one sampled pixel of four per frame
# gather modes 2 / 3 (im2col of the 3x3 valid conv and its transpose): N, H, W, gC (K = 9 gC)
IM2COL_SHAPES = [(2, 21, 19, 32),     # K = 288 = 4 * 64 + 32: a half-filled last K-stage (bf16)
                 (1, 3, 3, 32),       # one output pixel (mode 2); every pixel sees exactly one tap (mode 3)
                 (3, 5, 40, 32),      # 114-pixel frames: the M-tiles span frames
                 (5, 6, 7, 32),       # mode 2: five 20-pixel frames inside one 128-row tile
                 (2, 21, 19, 8),      # K = 72: each 16-byte bf16 chunk is another tap's whole channel set
                 (2, 21, 19, 64)]     # K = 576
IM2COL_COUT = {2: 64, 3: 32}          # the engine's output widths: conv2 forward, its input gradient
# dense split-K slabs: (M, N, K) x (tile, rows_per_split): 4 to 10 splits, the last one ragged
TN_SLAB_SHAPES = [(229, 256, 264), (300, 512, 256)]
TN_SLAB_FORMS = [(1, 32), (1, 64), (2, 64)]


def dw_staged_bf16(W):
    """the tile kernels stage the activation in bf16; dwframe.hip (W in 1, 2, 4, 8) keeps fp32 windows"""
    return W not in (1, 2, 4, 8)


def dw_inputs(N, C, H, W, seed=0):
    """Everything a depthwise case reads, generated on the CPU (so both files judge the same data)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + C + 31 * H + W)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(N, H, W, C).bfloat16(), "wt": r(9, C) / 3, "scale": torch.rand(C, generator=g) + 0.5,
            "shift": r(C) * 0.2, "dy": r(N, H, W, C).bfloat16(), "dres": r(N, H, W, C).bfloat16(),
            "dskip": r(N, OH, OW, C).bfloat16(), "yb": r(N, H, W, C).bfloat16(), "mean": r(C) * 0.1,
            "invstd": torch.rand(C, generator=g) + 0.5, "OH": OH, "OW": OW}


def gemm_nt_inputs(M, N, K, lda):
    g = torch.Generator().manual_seed(M + N + K)
    Abuf = torch.randn(M, lda, generator=g).bfloat16()
    B = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    return Abuf, B


def gemm_tn_inputs(M, N, K, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(M + N)
    return torch.randn(M, N, generator=g).to(dtype), torch.randn(M, K, generator=g).to(dtype)


def gather1_inputs(shape, dtype):
    """A strided 1x1 conv as the gathered GEMMs take it.  A [N,H,W,lda] is NaN wherever the gather must not
    read: the unsampled pixels and the pitch columns [K, lda).  B [Cout,K] the forward's weights (K^-1/2), G
    [M,Cout] the weight gradient's output gradient; signed data."""
    N, H, W, K, Cout, lda, S = shape
    g = torch.Generator().manual_seed(7 * N + 31 * H + W + K + Cout + 1000 * S)
    OH, OW = (H - 1) // S + 1, (W - 1) // S + 1
    A = torch.randn(N, H, W, lda, generator=g)
    unread = torch.ones(N, H, W, lda, dtype=torch.bool)
    unread[:, ::S, ::S, :K] = False
    A[unread] = float("nan")
    M = N * OH * OW
    return {"A": A.to(dtype), "B": (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dtype),
            "G": torch.randn(M, Cout, generator=g).to(dtype), "M": M, "N": Cout, "K": K, "ld": lda,
            "geom": (H, W, OH, OW, S, 0), "gather": (1, H, W, OH, OW, S, 0), "unread": int(unread.sum())}


def im2col_inputs(shape, mode, dtype):
    """The 3x3 valid conv gC -> 64 as an im2col GEMM (mode 2: A the input [N,H,W,gC], M = N OH OW rows, G the
    weight gradient's output gradient) or its input gradient (mode 3: A the output gradient [N,OH,OW,gC] -> 32
    channels, M = N H W rows); B [Cout, 9 gC], k = tap gC + c."""
    N, H, W, gC = shape
    g = torch.Generator().manual_seed(7 * N + 31 * H + W + gC + 1000 * mode)
    OH, OW = H - 2, W - 2
    K, Cout = 9 * gC, IM2COL_COUT[mode]
    M = N * OH * OW if mode == 2 else N * H * W
    A = torch.randn((N, H, W, gC) if mode == 2 else (N, OH, OW, gC), generator=g)
    return {"A": A.to(dtype), "B": (torch.randn(Cout, K, generator=g) / K ** 0.5).to(dtype),
            "G": torch.randn(M, Cout, generator=g).to(dtype), "M": M, "N": Cout, "K": K, "ld": gC,
            "geom": (H, W, OH, OW, 1, gC), "gather": (mode, H, W, OH, OW, 1, gC)}


def gathered(d):
    """the dense [M, K] operand of a gather1_inputs / im2col_inputs case; it holds none of A's NaNs"""
    X = gather_rows(d["A"][..., :d["K"]] if d["gather"][0] == 1 else d["A"], d["gather"][0], d["geom"])
    assert X.shape == (d["M"], d["K"]) and not torch.isnan(X).any()
    return X


# ------------------------------------------------------------------ element-wise BN kernels, pools (csrc/bn.hip)
def fma32(x, s, t):
    """fmaf(x, s, t) for a bf16 x (the product is exact in fp64), as an fp32 tensor"""
    return (x.double() * s.double() + t.double()).float()


def fma_unsure(x, s, t):
    """the sign of fmaf(x, s, t) is within rounding of undecided: |z| <= 2^-22 (|x s| + |t|)"""
    xs = x.double() * s.double()
    return (xs + t.double()).abs() <= 2.0 ** -22 * (xs.abs() + t.double().abs())


def maxpool3s2_ref(z):
    """3x3 stride-2 pad-1 max pool of z [N,H,W,C] with the kernels' first-max rule in (ky, kx) order
    (tail_fwd_kernel / tail_pool_quad_kernel; torch.max returns the first maximal index).  z is an exactly
    restated fp32 value, so a tie is an exact tie and the rule decides it: nothing to exclude.
    -> (max [N,OH,OW,C] in z's dtype, tap index uint8)"""
    N, H, W, C = z.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = F.pad(z, (0, 0, 1, 1, 1, 1), value=float("-inf"))
    win = torch.stack([p[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] for ky in range(3) for kx in range(3)])
    m, am = win.max(0)
    return m, am.to(torch.uint8)


def maxpool3s2_bwd_ref(dout, amax, H, W):
    """dz[pixel] = sum of dOut over the (<= 4) windows whose argmax tap is this pixel -> (ref64, abs_terms)"""
    N, OH, OW, C = dout.shape
    g = torch.zeros(N, H + 2, W + 2, C, dtype=torch.float64, device=dout.device)
    ab = torch.zeros_like(g)
    d = dout.double()
    for t in range(9):
        ky, kx = divmod(t, 3)
        sel = d * (amax == t)
        g[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += sel
        ab[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2] += sel.abs()
    return g[:, 1:H + 1, 1:W + 1].contiguous(), ab[:, 1:H + 1, 1:W + 1].contiguous()


def tail_plain_ref(y, s1, t1, skip, s2=None, t2=None):
    """The un-pooled block tail (tail_fwd_kernel, pool = 0): out = fmaf(y, s1, t1) + (skip, or fmaf(skip, s2, t2)):
    two exactly restated fp32 values and one fp32 add, n = 2 -> (ref64, abs_terms)"""
    z = fma32(y, s1, t1).double()
    sk = skip.double() if s2 is None else fma32(skip, s2, t2).double()
    return z + sk, z.abs() + sk.abs()


# N, C, H, W of the pooled tail, max-pool backward and its fused BN reduce.  N H W <= ~1100: the fp32-sum bound of
# the reduce is sharp only there (assert_f32_sum).  tail_pool_quad_kernel works per 2 x 2 quad of outputs, so an odd
# OH or OW is its ragged quad (clamped skip loads, skipped stores); maxpool_bwd_red_kernel's advance() steps
# SPB = 256 / CVB quads (chanred_geo) at a time, which is several whole frames where OH OW < SPB.
POOL_SHAPES = [(2, 128, 19, 20), (2, 128, 20, 19),    # -> 10 x 10 from an odd and an even extent: windows over both edges
               (1, 128, 37, 21),      # 299^2's 37 -> 19, by 11: odd x odd outputs, both quad edges ragged
               (1, 128, 29, 29),      # 64^2: 29 -> 15
               (4, 256, 15, 15),      # 64^2: 15 -> 8, 256 channels (SPB 8)
               (16, 736, 8, 8),       # 8 -> 4 at the pitch of 728: nch 2, CVB 46, SPB 5, 26 idle threads per workgroup
               (60, 1024, 4, 4),      # 4 -> 2: SPB 4 = one frame of quads per step
               (200, 1024, 2, 2),     # 2 -> 1: a step of advance() is four frames
               (300, 64, 1, 1),       # 1 -> 1: one pixel, tap 4 only; SPB 32
               (3, 728, 5, 3),        # 75^2 exit: -> 3 x 2, non-square
               (2, 8, 7, 9),          # C = 8: one channel vector, SPB 256 > the 40 quads
               (2, 256, 14, 14)]      # 224^2: 14 -> 7, an even input with an odd output
TAIL_PLAIN_SHAPES = [(3, 736, 19, 19),   # the middle flow's residual add at the pitch of 728
                     (2, 1024, 2, 3),    # 12 pixels, non-square (an exit-flow frame)
                     (5, 64, 1, 1)]      # 40 threads
AVGPOOL_SHAPES = [(3, 264, 100), (2, 2048, 49),       # N, C, HW
                  (3, 2048, 4), (2, 2048, 1), (5, 2048, 9), (2, 8, 6)]   # 64^2, a 1 x 1 exit, 75^2; one channel vector


def pool_inputs(N, C, H, W, pool=True, salt=0):
    """What a block-tail / max-pool case reads, generated on the CPU: y [N,H,W,C], the skip ys and the pooled
    gradient d at the output size, the two BN affines"""
    OH, OW = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (H, W)
    g = torch.Generator().manual_seed(H * 100 + W + salt)
    d = {"y": torch.randn(N, H, W, C, generator=g).bfloat16(), "ys": torch.randn(N, OH, OW, C, generator=g).bfloat16()}
    d["s1"], d["s2"] = (torch.rand(C, generator=g) + 0.5 for _ in range(2))
    d["t1"], d["t2"] = (torch.randn(C, generator=g) for _ in range(2))
    d["d"] = torch.randn(N, OH, OW, C, generator=g).bfloat16()
    d["OH"], d["OW"] = OH, OW
    return d


def batch_stats(y):
    """the batch's own mean / invstd of y [N,H,W,C] (so the dz zhat sums cancel) as fp32"""
    yd = y.double()
    return {"mean": yd.mean((0, 1, 2)).float(), "invstd": (1 / (yd.var((0, 1, 2), unbiased=False) + 1e-5).sqrt()).float()}


def chanred_geo(rows, C, cpt=8, target=1024):
    """make_chanred (csrc/bn.hip) restated: nch channel chunks of CVB vectors, SPB row slots per workgroup, P row
    chunks of rpc rows (the partial rows the reduce writes)"""
    cdiv = lambda a, b: -(-a // b)
    CV = C // cpt
    nch = cdiv(CV, 64)
    CVB = cdiv(CV, nch)
    SPB = 256 // CVB
    P = max(1, min(max(1, target // nch), cdiv(rows, 4 * SPB)))
    rpc = cdiv(rows, P)
    return {"nch": nch, "CVB": CVB, "SPB": SPB, "rpc": rpc, "P": cdiv(rows, rpc)}


def conv3x3_valid_ref(a, w, flip=None):
    """3x3, stride 1, no padding: a [N,IH,IW,CI] fp64, w [CO,CI,3,3] -> (ref64, abs_terms, extra) [N,OH,OW,CO],
    9 CI terms, as nine shifted slices times the tap's [CI][CO] matrix; flip: the one-ulp allowance of a
    (see tie_flip), carried through |w|."""
    N, IH, IW, CI = a.shape
    OH, OW = IH - 2, IW - 2
    wd = w.double()
    ref = torch.zeros(N, OH, OW, w.shape[0], dtype=torch.float64, device=a.device)
    ab, extra = torch.zeros_like(ref), torch.zeros_like(ref)
    for ky in range(3):
        for kx in range(3):
            wt = wd[:, :, ky, kx].t()
            ref += a[:, ky:ky + OH, kx:kx + OW] @ wt
            ab += a[:, ky:ky + OH, kx:kx + OW].abs() @ wt.abs()
            if flip is not None:
                extra += flip[:, ky:ky + OH, kx:kx + OW] @ wt.abs()
    return ref, ab, extra


# ------------------------------------------------------------------ stem conv1 (csrc/stem.hip): 3 -> 32, 3x3, stride 2, valid
U_SPLIT = 2.0 ** -18      # what x - hi - lo leaves of x after the bf16 head / tail split (see conv1_ref)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def conv1_out(IH, IW):
    return (IH - 3) // 2 + 1, (IW - 3) // 2 + 1


def conv1_path(bf16_out, IW, wgrad=False):
    """Which kernel xcp_conv1_fwd / xcp_conv1_wgrad launches, restated from the launchers:
    "row"   bf16 and 4 <= IW <= 320 (xcp_conv1_wgrad_fused): split-bf16 MFMA products
    "tile"  the LDS budget holds: forward (27 pitch + 864) floats, weight gradient 15 pitch floats + two rows of fp32 dY
    "pixel" wider frames.   pitch = IW rounded up to 64."""
    if bf16_out and 4 <= IW <= 320:
        return "row"
    pitch = (IW + 63) // 64 * 64
    if wgrad:
        return "tile" if 15 * pitch * 4 + 2 * conv1_out(3, IW)[1] * 32 * 4 <= 65536 else "pixel"
    return "tile" if (27 * pitch + 864) * 4 <= 65536 else "pixel"


CONV1_TILE_WIDEST = 512   # (27 * 512 + 864) * 4 = 58752 <= 65536; pitch 576 gives 65664


def conv1_ref(x, w, split=False):
    """x fp32 [N,3,IH,IW], w fp32 [32,3,3,3] -> (ref64, abs_terms, extra) [N,OH,OW,32], n = 27: fp64 F.conv2d of
    the values and of their magnitudes (an fp32 x fp32 product is exact in fp64).

    split: the forward row kernel's allowance.  It multiplies on the matrix cores with both operands split into
    a bf16 head and tail, hi = bf16(x), lo = bf16(x - hi).  Counting bf16's 8 significant bits as
    |x - hi| <= 2^-9 |x| and |x - hi - lo| <= 2^-18 |x| = r_x, the three products hi.hi + lo.hi + hi.lo miss
    r_x w + x r_w + lo_x lo_w, so extra = 3 * 2^-18 (1 + 2^-8) abs_terms (test_gpu_conv1_dgrad.py quotes 2^-17
    for the same products).  Round-to-nearest's strict worst case is half an ulp of 2^-7, i.e. 2^-8 and 2^-16:
    the allowance is a quarter of the worst case of one term, and it is what 27 terms of either sign are held
    to.  The weight-gradient row kernel splits X only (dC1 is bf16 already): 2^-18 abs_terms
    (conv1_wgrad_ref).  The tile and per-pixel kernels are plain fp32 FMAs: no extra."""
    xd, wd = x.double(), w.double()
    ref = _nhwc(F.conv2d(xd, wd, None, 2))
    ab = _nhwc(F.conv2d(xd.abs(), wd.abs(), None, 2))
    extra = ab * (3 * U_SPLIT * (1 + 2.0 ** -8)) if split else torch.zeros_like(ab)
    return ref, ab, extra


def conv1_wgrad_ref(x, dy, split=False, flip=None):
    """x fp32 [N,3,IH,IW], dy [N,OH,OW,32] (NHWC, any dtype) -> (ref64 [32,3,3,3], abs_terms, extra, n): fp64
    conv2d_weight of the values and of the magnitudes; n = the number of output pixels at which dy is nonzero
    (an exactly-zero term adds no rounding, wherever it falls in the summation tree).  split: the row kernel's
    2^-18 abs_terms (conv1_ref); flip: a per-element allowance of dy (tie_flip of a restated dC1), carried
    through |x|."""
    xd, g = x.double(), _nchw(dy.double())
    wg = lambda a, b: torch.nn.grad.conv2d_weight(a, (32, 3, 3, 3), b, stride=2)
    ref, ab = wg(xd, g), wg(xd.abs(), g.abs())
    extra = ab * U_SPLIT if split else torch.zeros_like(ab)
    if flip is not None:
        extra = extra + wg(xd.abs(), _nchw(flip.double()))
    n = int((dy != 0).any(-1).sum())
    return ref, ab, extra, n


def conv1_stats_ref(Y, N, OH, OW, R):
    """conv1_fwd_stats: partial row r = (sum y, sum y^2) over the STORED bf16 outputs of the output rows (tiles)
    r, r + R, ... (a bf16 square is exact in fp32) -> (ref64 [R,2,32], abs_terms, n [R,1,1] = OW * tiles of r)"""
    T = N * OH
    y = Y.double().view(T, OW, 32)
    ref = torch.zeros(R, 2, 32, dtype=torch.float64, device=Y.device)
    ab = torch.zeros_like(ref)
    for r in range(R):
        t = y[r::R]
        ref[r, 0], ref[r, 1] = t.sum((0, 1)), (t * t).sum((0, 1))
        ab[r, 0], ab[r, 1] = t.abs().sum((0, 1)), ref[r, 1]
    tiles = torch.tensor([len(range(r, T, R)) for r in range(R)], dtype=torch.float64, device=Y.device)
    return ref, ab, (tiles * OW).view(R, 1, 1)


def conv1_inputs(N, IH, IW, seed=1):
    """signed frames (rand - 0.3: the sums cancel, abs_terms is not the result itself), kernel, dense gradient.
    (The split products leave about 0.5 % of the row kernel's outputs not rounded to nearest; of the 256 outputs
    of (2, 9, 4) that is one or two, and under seeds 0 and 2 three; and the weight gradient of that shape sums
    8 pixels only, so its split residuals hardly average: seeds 3 and 4 reach 1.09 and 1.03 of the 2^-18 allowance
    (see conv1_ref on its worst case).  Both are conditions on the data, as for `exclude`: seed 1.)"""
    g = torch.Generator().manual_seed(100003 * seed + 977 * N + 31 * IH + IW)
    OH, OW = conv1_out(IH, IW)
    return {"x": torch.rand(N, 3, IH, IW, generator=g) - 0.3, "w": torch.randn(32, 3, 3, 3, generator=g) / 5,
            "dy": torch.randn(N, OH, OW, 32, generator=g), "OH": OH, "OW": OW}


def conv1_wgrad_groups(N, IH, IW, bf16_dy):
    """(tiles, workgroups) of the weight-gradient kernel: the row kernel walks N OH one-row tiles, the tile kernel
    N ceil(OH / 2) two-row tiles, with min(N ceil(OH / 2), 1024) workgroups either way (xcp_conv1_wgrad_parts)"""
    OH, _ = conv1_out(IH, IW)
    G = min(N * ((OH + 1) // 2), 1024)
    return (N * OH if conv1_path(bf16_dy, IW, True) == "row" else N * ((OH + 1) // 2)), G


def sparse_rows_gradient(dy, tiles, G, max_pixels=1000):
    """The fp32-sum bound is sharp only while n^2 2^-24 << 1, so a frame batch of more than ~1100 output pixels
    gets a gradient that is zero except at the first and last pixel of the first and last tile a workgroup
    walks (tiles b and b + k G), for every step-th workgroup and the last one: <= max_pixels pixels.
    dy [N,OH,OW,32]; a tile is tiles-th of the N OH OW pixels in order."""
    N, OH, OW, C = dy.shape
    per = N * OH * OW // tiles                       # pixels per tile (the sparse shapes have even OH)
    step = max(1, -(-4 * G // max_pixels))
    keep = torch.zeros(N * OH * OW, dtype=torch.bool)
    for b in sorted(set(range(0, G, step)) | {G - 1}):
        for t in (b, b + (tiles - 1 - b) // G * G):
            keep[t * per] = keep[t * per + per - 1] = True
    return dy * keep.view(N, OH, OW, 1)


# the cases: (N, IH, IW)
CONV1_ROW_SHAPES = [(2, 9, 4),       # OW = 1
                    (3, 11, 35),     # OW = 17: one 16-pixel group + 1
                    (2, 12, 13),     # even sizes: the last row and column are covered by no window
                    (1, 5, 299),     # bench width
                    (1, 7, 320),     # widest: three chunks per thread
                    (70, 33, 9)]     # N OH = 1120 > 1024 workgroups: 96 walk two tiles, the prefetch clamped at T - 1
CONV1_FWD_OTHER = [("bf16", (1, 9, 331)), ("bf16", (2, 5, 3)), ("bf16", (1, 5, CONV1_TILE_WIDEST)),   # tile kernel
                   ("fp32", (2, 12, 13)), ("fp32", (1, 19, 75)),       # OH = 9: the last 4-row tile holds one row
                   ("bf16", (1, 5, 700)), ("fp32", (1, 5, 700))]       # per-pixel kernel
CONV1_WGRAD_SHAPES = [(5, 17, 23), (2, 12, 13), (1, 7, 320), (1, 9, 331), (1, 5, 700), (2, 5, 3), (2, 9, 4)]
CONV1_WGRAD_SPARSE = (70, 33, 9)


# ------------------------------------------------------------------ stem conv2 (csrc/conv3.hip) gradients
def conv3x3_dgrad_ref(dy, w):
    """dy [N,OH,OW,64], w [64,32,3,3] -> (ref64, abs_terms) [N,OH+2,OW+2,32]: the valid 3x3 conv of the pad-2
    gradient with the flipped, transposed kernel, 9 * 64 = 576 terms (border pixels see 1 to 6 taps, the rest
    of their terms are exact zeros)"""
    p = F.pad(dy.double(), (0, 0, 2, 2, 2, 2))
    ref, ab, _ = conv3x3_valid_ref(p, w.double().permute(1, 0, 2, 3).flip(2, 3))
    return ref, ab


def conv3x3_wgrad_ref(dy, a, flip=None):
    """dy [N,OH,OW,64], a fp64 [N,IH,IW,32] -> (dW [64][9][32], abs_terms, extra), n = N OH OW:
    dW[co][tap][ci] = sum_p dy[p][co] a[p + off(tap)][ci]; flip: the one-ulp allowance of a, carried through |dy|"""
    N, OH, OW, CO = dy.shape
    g = dy.double().reshape(-1, CO).t()
    ref, ab, ex = [], [], []
    for ky in range(3):
        for kx in range(3):
            s = a[:, ky:ky + OH, kx:kx + OW].reshape(-1, a.shape[3])
            ref.append(g @ s)
            ab.append(g.abs() @ s.abs())
            ex.append(g.abs() @ flip[:, ky:ky + OH, kx:kx + OW].reshape(-1, a.shape[3]) if flip is not None
                      else torch.zeros_like(ref[-1]))
    return torch.stack(ref, 1), torch.stack(ab, 1), torch.stack(ex, 1)


def bn_relu_on_load(x, s, t):
    """c3_act: a = bf16(max(fmaf(x, s, t), 0)) -> (a fp64, its tie allowance)"""
    a32 = fma32(x, s, t).clamp_min(0)
    return a32.bfloat16().double(), tie_flip(a32)


def conv3_inputs(N, IH, IW, cin, seed=0):
    g = torch.Generator().manual_seed(7919 * seed + 1009 * N + 37 * IH + IW + cin)
    return {"x": (torch.randn(N, IH, IW, cin, generator=g) * 1.5 + 0.3).bfloat16(),
            "w": (torch.randn(64, 32, 3, 3, generator=g) / 288 ** 0.5).bfloat16(),
            "s": torch.rand(32, generator=g) + 0.5, "t": torch.randn(32, generator=g) * 0.3, "g": g}


def conv3_wgrad_inputs(N, IH, IW):
    d = conv3_inputs(N, IH, IW, 32)
    d["dy"] = torch.randn(N, IH - 2, IW - 2, 64, generator=d["g"]).bfloat16()
    return d


CONV3_DGRAD_SHAPES = [(3, 3, 3), (2, 7, 17), (3, 19, 36), (1, 4, 145), (1, 3, 147)]    # the gradient's (N, OH, OW)
CONV3_WGRAD_SHAPES = [(3, 3, 3), (1, 6, 147), (2, 12, 34), (1, 5, 160), (1, 40, 34)]   # the input's (N, IH, IW)


# ------------------------------------------------------------------ BN statistics (csrc/bn.hip)
def chan_sums_ref(mode, a, b=None, mean=None, invstd=None, ms=None, mt=None):
    """chanred_kernel's sums over the rows of a [rows, C] -> (ref64 [2,C], abs_terms, extra), n = rows (valid for
    any partition into partial rows: the test sums the partial rows in fp64).
    mode 0: (sum x, sum x^2) -- fmaf(x, x, acc): the square is exact.
    mode 1: (sum dz, sum dz zhat), zhat = fl32(fl32(y - mu) is) restated with the same two fp32 operations, so
            the term dz zhat is exact in fp64.
    mode 2: dz masked by fmaf(y, ms, mt) > 0; where that sign is within rounding of undecided (fma_unsure) the
            element's |term| goes into extra (a sum cannot exclude an element)."""
    ad = a.double()
    if mode == 0:
        t = full = (ad, ad * ad)
    else:
        zhat = ((b.float() - mean) * invstd).double()
        full = (ad, ad * zhat)                                   # the unmasked terms
        keep = (fma32(b, ms, mt) > 0) if mode == 2 else torch.ones_like(ad, dtype=torch.bool)
        t = tuple(v * keep for v in full)
    ref = torch.stack([v.sum(0) for v in t])
    ab = torch.stack([v.abs().sum(0) for v in t])
    extra = torch.zeros_like(ab)
    if mode == 2:
        unsure = fma_unsure(b, ms, mt)
        extra = torch.stack([(v.abs() * unsure).sum(0) for v in full])
    return ref, ab, extra


def chan_inputs(rows, C, dtype, seed=0):
    """y, dz and the batch's own mean / invstd (so the dz zhat sums cancel), a ReLU affine"""
    g = torch.Generator().manual_seed(104729 * seed + 13 * rows + C)
    y = (torch.randn(rows, C, generator=g) * 1.3 + 0.4).to(dtype)
    dz = torch.randn(rows, C, generator=g).to(dtype)
    yd = y.double()
    mean = yd.mean(0)
    var = (yd * yd).mean(0) - mean * mean
    return {"y": y, "dz": dz, "mean": mean.float(), "invstd": (1 / (var + 1e-5).sqrt()).float(),
            "ms": torch.rand(C, generator=g) + 0.5, "mt": torch.randn(C, generator=g) * 0.3}


CHAN_SHAPES = [(1083, 728), (1083, 736), (50, 2048), (5, 64), (147, 32), (1, 8), (1001, 8)]   # rows, C
BN_STRIDED_SHAPES = [(2, 19, 20, 128), (1, 7, 5, 728), (3, 4, 4, 64)]                         # N, H, W, C

FIN_ROWS = [1, 15, 16, 17, 767, 768, 769, 2048, 2049]     # 2049 > FIN_MAX_ROWS: pre-reduced by ops._fold
FIN_CHANNELS = [(32, 32), (40, 40), (728, 736)]           # C, CP
FIN_MAX_ROWS = 2048
FIN_BWD_FORMS = ["plain", "accumulate", "narrow", "frozen", "narrow+accumulate"]
U64 = 2.0 ** -53


def _fin_sums(part, C):
    """fp64 column sums of the fp32 partial rows part [R,2,CP] and what they may be off by: the fp64 summation
    order, R 2^-53 sum |part|; above FIN_MAX_ROWS rows ops._fold pre-reduces them to fp32 group sums, each
    rounded once: 2^-24 sum |part|."""
    R = part.shape[0]
    p = part.double()[:, :, :C]
    s, a = p.sum(0), p.abs().sum(0)
    noise = a * (R * U64 + (U32 if R > FIN_MAX_ROWS else 0.0))
    return s[0], s[1], noise[0], noise[1]


def bn_finalize_ref(part, count, gamma, beta, rmean, rvar, momentum, eps):
    """bn_finalize_part_kernel's fp64 expression on the fp32 partial rows part [R,2,CP] (C = len(gamma)):
        mean = s / count, var = max(q / count - mean^2, 0), is = 1 / sqrt(var + eps),
        scale = gamma fl32(is), shift = beta - fl32(mean) scale (fp32, fma or not),
        running = (1 - momentum) running + momentum (mean | var count / (count - 1))
    -> {name: (ref64 [C], bound [C])}.  Each bound counts the code's own roundings: one fp32 rounding (2^-24
    relative) for mean, invstd and the running statistics, one more for scale, 2^-24 (|beta| + 2 |mean scale|) for
    shift plus what the errors of fl32(mean) and scale carry into it; the noise of the sums (_fin_sums) is
    carried through var's cancellation and through 1 / sqrt by evaluating is at var -+ dvar (negligible except
    for a constant channel)."""
    C = gamma.shape[0]
    s, q, ds, dq = _fin_sums(part, C)
    gm, be = gamma.double(), beta.double()
    mom, ep = float(torch.tensor(momentum, dtype=torch.float32)), float(torch.tensor(eps, dtype=torch.float32))
    mean = s / count
    dmean = ds / count + 2 * U64 * mean.abs()
    q1 = q / count
    var = (q1 - mean * mean).clamp_min(0)
    dvar = dq / count + 2 * mean.abs() * dmean + 4 * U64 * (q1.abs() + mean * mean)
    inv = 1 / (var + ep).sqrt()
    dis = torch.maximum(1 / ((var - dvar).clamp_min(0) + ep).sqrt() - inv, inv - 1 / (var + dvar + ep).sqrt())
    dis = dis + 4 * U64 * inv
    e_mean = dmean + U32 * mean.abs()                       # of fl32(mean)
    e_is = dis + U32 * inv                                  # of fl32(is)
    scale = gm * inv
    e_scale = gm.abs() * e_is + U32 * scale.abs()
    shift = be - mean * scale
    e_shift = U32 * (be.abs() + 2 * (mean * scale).abs()) + mean.abs() * e_scale + scale.abs() * e_mean
    unb = var * count / (count - 1) if count > 1 else var
    dunb = dvar * (count / (count - 1) if count > 1 else 1.0)
    rm = (1 - mom) * rmean.double() + mom * mean
    rv = (1 - mom) * rvar.double() + mom * unb
    return {"mean": (mean, e_mean), "invstd": (inv, e_is), "scale": (scale, e_scale), "shift": (shift, e_shift),
            "running_mean": (rm, U32 * rm.abs() + mom * dmean + 4 * U64 * (rmean.double().abs() + mean.abs())),
            "running_var": (rv, U32 * rv.abs() + mom * dunb + 4 * U64 * (rvar.double().abs() + unb.abs()))}


def bn_eval_ref(gamma, beta, rmean, rvar, eps):
    """xcp_bn_finalize with train = 0: mean = running_mean, var = running_var (both fp32 already)"""
    gm, be, mean = gamma.double(), beta.double(), rmean.double()
    ep = float(torch.tensor(eps, dtype=torch.float32))
    inv = 1 / (rvar.double() + ep).sqrt()
    e_is = (U32 + 4 * U64) * inv
    scale = gm * inv
    e_scale = gm.abs() * e_is + U32 * scale.abs()
    shift = be - mean * scale
    return {"mean": (mean, torch.zeros_like(mean)), "invstd": (inv, e_is), "scale": (scale, e_scale),
            "shift": (shift, U32 * (be.abs() + 2 * (mean * scale).abs()) + mean.abs() * e_scale)}


def bn_bwd_finalize_ref(part, count, gamma, mean, invstd, frozen=False, base=None):
    """bn_bwd_finalize_part_kernel's fp64 expression on the fp32 partial rows (sum dz, sum dz zhat):
        a = gamma is, alpha = fl32(a), bcoef = fl32(-a is mdzy), delta = fl32(-a mdz + a is mu mdzy)
        (mdz = sdz / count, ...; frozen: bcoef = delta = 0 exactly), dgamma = fl32(sdzy), dbeta = fl32(sdz);
        base = (dgamma0, dbeta0): the accumulate form adds them in fp32 (one more rounding).
    -> {name: (ref64 [C], bound [C])}: one fp32 rounding each, plus the sums' noise (_fin_sums) through the
    expression, plus fp64's own rounding of delta's cancellation."""
    C = gamma.shape[0]
    sdz, sdzy, ds, dq = _fin_sums(part, C)
    inv, gm, mu = invstd.double()[:C], gamma.double(), mean.double()[:C]
    a = gm * inv
    mdz, mdzy = sdz / count, sdzy / count
    z = torch.zeros_like(a)
    bc = -a * inv * mdzy
    t1, t2 = -a * mdz, a * inv * mu * mdzy
    e_bc = U32 * bc.abs() + (a * inv).abs() * dq / count + 4 * U64 * bc.abs()
    e_de = U32 * (t1 + t2).abs() + a.abs() * ds / count + (a * inv * mu).abs() * dq / count \
        + 6 * U64 * (t1.abs() + t2.abs())
    out = {"alpha": (a, U32 * a.abs()), "bcoef": (z, z) if frozen else (bc, e_bc),
           "delta": (z, z) if frozen else (t1 + t2, e_de)}
    for name, sm, dn, b0 in (("dgamma", sdzy, dq, None if base is None else base[0]),
                             ("dbeta", sdz, ds, None if base is None else base[1])):
        ref, e = sm, U32 * sm.abs() + dn
        if b0 is not None:
            ref, e = sm + b0.double()[:C], e + U32 * (sm.abs() + b0.double()[:C].abs())
        out[name] = (ref, e)
    return out


def assert_within(got, ref64, bound, tag=""):
    """|got - ref64| <= bound per element, through assert_f32_sum (no terms, the bound as `extra`)"""
    return assert_f32_sum(got, ref64, torch.zeros_like(ref64), 0, extra=bound, tag=tag)


def fin_fwd_inputs(R, C, CP, seed=0):
    """Partial rows written as fp32 sums of two data rows each (count = 2 R, q consistent with s), with, among the
    channels: 0 all zero, 1 constant 3.0 (var exactly 0: the sums are small integers), 2 with |mean| = 50 std;
    gamma, beta and non-trivial running statistics.  The padding channels of part hold junk the kernel must not
    use."""
    g = torch.Generator().manual_seed(15485863 * seed + 31 * R + C)
    x = torch.randn(R, 2, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)
    x[:, :, 0] = 0.0
    x[:, :, 1] = 3.0
    x[:, :, 2] = 50.0 + torch.randn(R, 2, generator=g)
    part = torch.randn(R, 2, CP, generator=g)
    part[:, 0, :C] = x[:, 0] + x[:, 1]
    part[:, 1, :C] = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]
    return {"part": part, "count": 2 * R, "gamma": torch.rand(C, generator=g) + 0.5, "beta": torch.randn(C, generator=g),
            "rmean": torch.randn(C, generator=g) * 0.3, "rvar": torch.rand(C, generator=g) + 0.5, "momentum": 0.1,
            "eps": 1e-5}


def fin_bwd_inputs(R, C, CP, seed=0):
    """gradient partial rows of realistic size (1e-3), statistics with the three special channels of
    fin_fwd_inputs (zero: invstd = 1 / sqrt(eps); constant; |mean| = 50 std), earlier dgamma / dbeta"""
    g = torch.Generator().manual_seed(32452843 * seed + 17 * R + C)
    part = torch.randn(R, 2, CP, generator=g) * 1e-3
    mean, invstd = torch.randn(CP, generator=g), 1 / (torch.rand(CP, generator=g) + 0.3)
    mean[0], invstd[0] = 0.0, float(1 / torch.tensor(1e-5, dtype=torch.float64).sqrt())
    mean[1], invstd[1] = 3.0, invstd[0]
    mean[2], invstd[2] = 50.0, 1.0
    return {"part": part, "count": 2 * R, "gamma": torch.rand(C, generator=g) + 0.5, "mean": mean, "invstd": invstd,
            "dgamma0": torch.randn(C, generator=g), "dbeta0": torch.randn(C, generator=g)}
