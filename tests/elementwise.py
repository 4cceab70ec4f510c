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
                 (2, 72, 5, 9),        # narrowest frame of the tile kernel; last group 8 channels
                 (3, 1536, 10, 10),    # 128-B slices
                 (3, 200, 7, 8), (5, 728, 3, 4), (2, 64, 1, 2)]   # dwframe.hip (fp32 windows: no bf16 staging)
DW_BWD_SHAPES = [(2, 72, 9, 21),       # two column groups, 20 + 1
                 (2, 64, 64, 5),       # three row bands
                 (3, 728, 19, 19),
                 (2, 128, 15, 15)]
# form, act
DW_BWD_FORMS = [("plain", 0), ("plain", 1), ("plain", 2), ("res", 1), ("skip", 2), ("res+skip", 1), ("resbn", 2),
                ("skip_pre", 2)]
# M, N, K, lda
GEMM_NT_SHAPES = [(256, 256, 32, 32), (1000, 728, 728, 728), (300, 2048, 1536, 1536), (77, 64, 288, 288),
                  (513, 264, 40, 40), (4100, 1024, 728, 1456)]
GEMM_TN_SHAPES = [(229, 256, 264), (33, 512, 2048), (300, 2048, 1536)]
UNIT_BWD_SHAPES = [(M, CO, CI) for M in (453, 1000) for CO, CI in ((128, 128), (128, 64), (256, 128), (256, 256))]


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
