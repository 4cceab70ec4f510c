"""Clip degradation on the GPU: Gaussian blur, sensor noise and JPEG compression of the uint8 clip.

Detectors are judged on recompressed, blurred and noisy video (FaceForensics++ c23 / c40, every
re-encode of a social network), and the reference's trainers augment for it (train_au_patch.py:193
``augment_train=True``).  ``xcp_clip_degrade`` (csrc/degrade.hip) acts where a camera and a codec
act, on the uint8 clip, and hands a uint8 clip of the same shape to the unchanged
``xcp_clip_augment`` / ``xcp_frames_prep``.  The data-dependent part is a table of 16 ints per clip,
shared by the clip's frames.

The arithmetic -- the contract between the kernel and ``degrade_reference`` -- is integer and fits
int32 at every step, so the two agree byte for byte.  ``>>`` is an arithmetic shift,
``rs(a, n) = (a + (1 << (n - 1))) >> n``.  Per clip, in this order, each stage skipped when its
parameter is 0; frames t >= clamp(len, 0, Tmax) are zero:

  blur   separable, radius R <= 7, taps w[0..7] summing to 2048 per pass:
         h[y][x] = sum_k w[|k|] p[y][refl(x + k, W)], v[y][x] = sum_k w[|k|] h[refl(y + k, H)][x],
         out = rs(v, 22).  refl(i, n) = -i for i < 0, 2n - 2 - i for i >= n, else i (reflect-101),
         then clamped to [0, n - 1] (frames smaller than R).
  noise  Philox4x32-10, key (seed_lo, seed_hi), counter (y W + x, t, c, 0); S = the sum of the eight
         16-bit halves of the four output words, z2 = 2 S - 524280, n = rs(namp z2, 20),
         out = clamp(p + n, 0, 255).  namp = round(sigma_n 2^20 / 107019.7), the divisor being the
         standard deviation of z2.  The amplitude law is an 8-fold Irwin-Hall sum (a piecewise
         polynomial bell with support +-4.9 sigma), not an exact Gaussian.
  JPEG   baseline, 4:2:0, IJG quality q: libjpeg's integer colour conversion, edge-replicated
         padding to multiples of 16, 2 x 2 chroma averaging, an integer matrix DCT (``DCT_C``,
         12-bit cosines) with rounding shifts 9 and 15 per pass, the Annex K tables scaled by q,
         quantise / dequantise, the inverse DCT, libjpeg's triangle chroma up-sampling and the
         integer conversion back to RGB.  ``_jpeg_frame`` spells each step out.
"""
import math

import numpy as np
import torch

DEG_COLS = 16            # XCP_DEG_COLS of include/xcp.h
NOISE_Z2_STD = 107019.7  # 2 sqrt(8 (65536^2 - 1) / 12): the standard deviation of z2
MAX_NOISE = 64.0
MAX_RADIUS = 7
_INT_FIELDS = (("quality", 0), ("radius", 1), ("namp", 10), ("seed_lo", 11), ("seed_hi", 12))

LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)
DCT_C = np.array([[1448] * 8,
                  [2009, 1703, 1138, 400, -400, -1138, -1703, -2009],
                  [1892, 784, -784, -1892, -1892, -784, 784, 1892],
                  [1703, -400, -2009, -1138, 1138, 2009, 400, -1703],
                  [1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448],
                  [1138, -2009, 400, 1703, -1703, -400, 2009, -1138],
                  [784, -1892, 1892, -784, -784, 1892, -1892, 784],
                  [400, -1138, 1703, -2009, 2009, -1703, 1138, -400]], np.int64)   # C[u][x]


def _clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _rs(a, n):
    return (a + (1 << (n - 1))) >> n


def gaussian_taps(sigma):
    """(R, w[0..7]) of a Gaussian of standard deviation ``sigma`` pixels: R = min(7, ceil(3 sigma)),
    g_k = exp(-k^2 / 2 sigma^2) normalised over -R..R, w_k = round(2048 g_k) for k >= 1 and
    w_0 = 2048 - 2 sum_{k >= 1} w_k.  sigma 0: R = 0 (no blur)."""
    sigma = float(sigma)
    if not 0.0 <= sigma < math.inf:
        raise ValueError("blur sigma must be finite and >= 0")
    w = [0] * 8
    if sigma == 0.0:
        return 0, w
    R = min(MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    g = [math.exp(-k * k / (2.0 * sigma * sigma)) for k in range(R + 1)]
    total = g[0] + 2.0 * sum(g[1:])
    for k in range(1, R + 1):
        w[k] = int(np.rint(2048.0 * g[k] / total))
    w[0] = 2048 - 2 * sum(w[1:])
    return R, w


def noise_amplitude(sigma_n):
    """namp of a noise of standard deviation ``sigma_n`` grey levels (refused above 64)."""
    sigma_n = float(sigma_n)
    if not 0.0 <= sigma_n <= MAX_NOISE:
        raise ValueError(f"noise sigma must be in [0, {MAX_NOISE:g}] grey levels")
    return int(np.rint(sigma_n * (1 << 20) / NOISE_Z2_STD))


MAX_NAMP = int(np.rint(MAX_NOISE * (1 << 20) / NOISE_Z2_STD))


def _as_i32(v):
    """Python ints / uint32 bit patterns -> int32 tensor of the same bits."""
    a = np.asarray(v, dtype=np.int64).reshape(-1) & 0xffffffff
    return torch.from_numpy(a.astype(np.uint32).view(np.int32).copy())


class DegradeParams:
    """The per-clip table as named host tensors: int32 [B] ``quality`` (0: no JPEG), ``radius``
    (0: no blur), ``namp`` (0: no noise), ``seed_lo``, ``seed_hi`` (the Philox key's bit patterns)
    and int32 [B, 8] ``taps``.  ``pack()`` / ``to(device)`` give the int32 [B, 16] form the kernel
    reads (include/xcp.h lists the columns)."""

    def __init__(self, quality, radius, taps, namp, seed_lo, seed_hi):
        B = len(quality)
        self.quality = torch.as_tensor(quality, dtype=torch.int32).reshape(B).clone()
        self.radius = torch.as_tensor(radius, dtype=torch.int32).reshape(B).clone()
        self.taps = torch.as_tensor(taps, dtype=torch.int32).reshape(B, 8).clone()
        self.namp = torch.as_tensor(namp, dtype=torch.int32).reshape(B).clone()
        self.seed_lo = torch.as_tensor(seed_lo, dtype=torch.int32).reshape(B).clone()
        self.seed_hi = torch.as_tensor(seed_hi, dtype=torch.int32).reshape(B).clone()

    def __len__(self):
        return self.quality.numel()

    @classmethod
    def fixed(cls, B, quality=0, sigma=0.0, noise=0.0, seed=0):
        """Every clip the same JPEG quality (0: none), blur sigma in pixels and noise sigma in grey
        levels.  ``seed``: an int, clip b then draws its noise with the 64-bit key seed + b, or a
        sequence of B ints."""
        quality = int(quality)
        if not 0 <= quality <= 100:
            raise ValueError("JPEG quality must be in 1..100, or 0 for no JPEG")
        R, w = gaussian_taps(sigma)
        namp = noise_amplitude(noise)
        seeds = [int(seed) + b for b in range(B)] if np.ndim(seed) == 0 else [int(s) for s in seed]
        if len(seeds) != B:
            raise ValueError(f"{len(seeds)} seeds for {B} clips")
        return cls([quality] * B, [R] * B, [w] * B, [namp] * B, _as_i32([s & 0xffffffff for s in seeds]),
                   _as_i32([(s >> 32) & 0xffffffff for s in seeds]))

    @classmethod
    def identity(cls, B):
        """No stage: real frames are copied, padding frames zeroed."""
        return cls.fixed(B)

    def pack(self, out=None):
        """int32 [B, 16] host tensor (``out``: a preallocated, e.g. pinned, one to fill)."""
        B = len(self)
        t = torch.zeros((B, DEG_COLS), dtype=torch.int32) if out is None else out
        if t.dtype != torch.int32 or tuple(t.shape) != (B, DEG_COLS):
            raise ValueError(f"pack: out must be int32 [{B}, {DEG_COLS}]")
        t.zero_()
        for k, c in _INT_FIELDS:
            t[:, c] = getattr(self, k)
        t[:, 2:10] = self.taps
        return t

    @classmethod
    def unpack(cls, packed):
        t = packed.detach().cpu().contiguous()
        return cls(taps=t[:, 2:10], **{k: t[:, c] for k, c in _INT_FIELDS})

    def to(self, device, non_blocking=False):
        """The packed table on ``device``: what ``ops.clip_degrade`` takes and a captured graph
        re-reads (overwrite it in place with ``copy_`` of another table's ``pack()``)."""
        return self.pack().to(device, non_blocking=non_blocking)

    def equal(self, other):
        return all(torch.equal(getattr(self, k), getattr(other, k)) for k, _ in _INT_FIELDS) \
            and torch.equal(self.taps, other.taps)

    def validate(self, B=None):
        """Raise ValueError unless this is a table (for B clips) that needs no clamping: quality in
        [0, 100], radius in [0, 7], non-negative taps that sum to 2048 per pass over -R..R, namp
        no larger than a 64-grey-level noise gives."""
        if B is not None and len(self) != B:
            raise ValueError(f"degrade table has {len(self)} rows for {B} clips")
        k = torch.arange(8).view(1, 8)
        live = (k <= self.radius.view(-1, 1)).to(torch.int64)
        total = (self.taps.long() * live * torch.where(k == 0, 1, 2)).sum(1)
        bad = ((self.quality < 0) | (self.quality > 100) | (self.radius < 0) | (self.radius > MAX_RADIUS)
               | (self.namp < 0) | (self.namp > MAX_NAMP) | (self.taps < 0).any(1)
               | ((self.radius > 0) & (total != 2048)))
        if bool(bad.any()):
            raise ValueError(f"degrade table rows {bad.nonzero().flatten().tolist()} are out of range: need quality in "
                             f"[0, 100], radius in [0, {MAX_RADIUS}], taps >= 0 summing to 2048, namp in [0, {MAX_NAMP}] "
                             f"(noise sigma <= {MAX_NOISE:g})")

    def row(self, i):
        """Row i as Python ints, clamped exactly as the kernel clamps what it reads."""
        return dict(quality=_clampi(int(self.quality[i]), 0, 100), radius=_clampi(int(self.radius[i]), 0, MAX_RADIUS),
                    taps=[int(v) for v in self.taps[i]], namp=_clampi(int(self.namp[i]), 0, 1023),
                    seed_lo=int(self.seed_lo[i]) & 0xffffffff, seed_hi=int(self.seed_hi[i]) & 0xffffffff)


# ---- the restatement -----------------------------------------------------------------------------

def _refl(i, n):
    i = np.asarray(i, np.int64)
    r = np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))
    return np.clip(r, 0, n - 1)


def _blur(p, R, w):
    """p int64 [T, H, W, 3] -> blurred int64, same shape."""
    _, H, W, _ = p.shape
    ks = range(-R, R + 1)
    xs, ys = np.arange(W), np.arange(H)
    h = sum(w[abs(k)] * p[:, :, _refl(xs + k, W)] for k in ks)
    v = sum(w[abs(k)] * h[:, _refl(ys + k, H)] for k in ks)
    return _rs(v, 22)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11).  counter: four uint32 arrays of one shape; key: two
    ints.  -> four uint64 arrays holding the 32-bit output words."""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff
    c = [np.asarray(x, np.uint64) & np.uint64(mask) for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & mask, int(key[1]) & mask
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(mask)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(mask)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c


def _noise(p, namp, key):
    """p int64 [T, H, W, 3] (frame t is source frame t) -> noisy int64 in [0, 255]."""
    T, H, W, _ = p.shape
    pix = (np.arange(H, dtype=np.int64).reshape(1, H, 1, 1) * W + np.arange(W, dtype=np.int64).reshape(1, 1, W, 1))
    words = philox4x32_10((pix, np.arange(T).reshape(T, 1, 1, 1), np.arange(3).reshape(1, 1, 1, 3),
                           np.zeros((1, 1, 1, 1), np.int64)), key)
    S = sum((x & np.uint64(0xffff)) + (x >> np.uint64(16)) for x in words).astype(np.int64)
    z2 = 2 * S - 524280
    return np.clip(p + _rs(namp * z2, 20), 0, 255)


def quant_table(base, q):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((base * s + 50) // 100, 1, 255)


def _blocks(plane):
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    nh, nw = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(nh * 8, nw * 8)


def _codec(plane, Q):
    """One padded plane through the forward DCT, quantiser and inverse DCT."""
    C = DCT_C
    p = _blocks(plane) - 128                         # [.., y, x]
    t = _rs(p @ C.T, 9)                              # t[y][u] = sum_x C[u][x] p[y][x]
    F = _rs(C @ t, 15)                               # F[v][u] = sum_y C[v][y] t[y][u]
    k = np.sign(F) * ((np.abs(F) + (Q >> 1)) // Q)
    F = k * Q
    t = _rs(C.T @ F, 9)                              # t'[y][u] = sum_v C[v][y] F'[v][u]
    r = _rs(t @ C, 15) + 128                         # r[y][x] = sum_u C[u][x] t'[y][u]
    return _unblocks(np.clip(r, 0, 255))


def _upsample(c):
    """libjpeg's triangle ("fancy") 2 x 2 up-sampling with edge replication."""
    up, dn = np.concatenate([c[:1], c[:-1]], 0), np.concatenate([c[1:], c[-1:]], 0)
    v = np.empty((2 * c.shape[0], c.shape[1]), np.int64)
    v[0::2], v[1::2] = 3 * c + up, 3 * c + dn
    lf, rt = np.concatenate([v[:, :1], v[:, :-1]], 1), np.concatenate([v[:, 1:], v[:, -1:]], 1)
    o = np.empty((v.shape[0], 2 * v.shape[1]), np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * v + lf + 8) >> 4, (3 * v + rt + 7) >> 4
    return o


def _jpeg_frame(p, q):
    """p int64 [H, W, 3] -> what a baseline 4:2:0 JPEG of quality q decodes to, int64 [H, W, 3]."""
    H, W, _ = p.shape
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    pad = ((0, -H % 16), (0, -W % 16))
    Y, Cb, Cr = (np.pad(x, pad, mode="edge") for x in (Y, Cb, Cr))
    Cb, Cr = ((x[0::2, 0::2] + x[0::2, 1::2] + x[1::2, 0::2] + x[1::2, 1::2] + 2) >> 2 for x in (Cb, Cr))
    QL, QC = quant_table(LUMA_Q, q), quant_table(CHROMA_Q, q)
    Y = _codec(Y, QL)[:H, :W]
    cb = _upsample(_codec(Cb, QC))[:H, :W] - 128
    cr = _upsample(_codec(Cr, QC))[:H, :W] - 128
    out = np.stack([Y + ((91881 * cr + 32768) >> 16),
                    Y + ((-22554 * cb - 46802 * cr + 32768) >> 16),
                    Y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255)


def degrade_reference(frames_u8, lengths, params):
    """``ops.clip_degrade`` restated with numpy integers on the CPU (module docstring), byte for
    byte.  frames_u8 uint8 [B, Tmax, H, W, 3], lengths [B], params a ``DegradeParams`` (clamped
    here as the kernel clamps it).  -> uint8 tensor [B, Tmax, H, W, 3]."""
    f = torch.as_tensor(frames_u8).cpu().numpy()
    B, Tmax = f.shape[:2]
    out = np.zeros_like(f)
    for b in range(B):
        g = params.row(b)
        L = _clampi(int(lengths[b]), 0, Tmax)
        if L == 0:
            continue
        p = f[b, :L].astype(np.int64)
        if g["radius"]:
            p = _blur(p, g["radius"], g["taps"])
        if g["namp"]:
            p = _noise(p, g["namp"], (g["seed_lo"], g["seed_hi"]))
        if g["quality"]:
            p = np.stack([_jpeg_frame(x, g["quality"]) for x in p])
        out[b, :L] = p.astype(np.uint8)
    return torch.from_numpy(out)


# ---- the sampler ---------------------------------------------------------------------------------

class ClipDegrade:
    """Sampler of ``DegradeParams``.  Per clip, independently: with probability ``jpeg_p`` a JPEG of
    integer quality uniform in ``jpeg``; with ``blur_p`` a Gaussian blur of sigma uniform in ``blur``
    pixels; with ``noise_p`` a noise of standard deviation uniform in ``noise`` grey levels (at
    most 64), with its own 64-bit seed."""

    def __init__(self, jpeg=(30, 95), jpeg_p=0.5, blur=(0.3, 2.0), blur_p=0.3, noise=(1.0, 8.0), noise_p=0.3):
        self.jpeg = (int(jpeg[0]), int(jpeg[1]))
        self.blur, self.noise = tuple(map(float, blur)), tuple(map(float, noise))
        self.jpeg_p, self.blur_p, self.noise_p = float(jpeg_p), float(blur_p), float(noise_p)
        if not 1 <= self.jpeg[0] <= self.jpeg[1] <= 100 or not 0 < self.blur[0] <= self.blur[1] < math.inf \
                or not 0 < self.noise[0] <= self.noise[1] <= MAX_NOISE \
                or not all(0 <= p <= 1 for p in (self.jpeg_p, self.blur_p, self.noise_p)):
            raise ValueError("ClipDegrade: bad argument (1 <= jpeg lo <= hi <= 100, 0 < blur lo <= hi, "
                             f"0 < noise lo <= hi <= {MAX_NOISE:g}, probabilities in [0, 1])")

    def sample(self, B, generator):
        """One independent draw per clip and stage from ``generator`` (a numpy.random.Generator), in
        clip order: jpeg, blur, noise, seed.  -> DegradeParams."""
        if generator is None:
            raise ValueError("ClipDegrade.sample: pass a numpy.random.Generator")
        q, R, taps, namp, lo, hi = [], [], [], [], [], []
        for _ in range(int(B)):
            use, quality = generator.random() < self.jpeg_p, int(generator.integers(self.jpeg[0], self.jpeg[1] + 1))
            q.append(quality if use else 0)
            use, sigma = generator.random() < self.blur_p, generator.uniform(*self.blur)
            r, w = gaussian_taps(sigma if use else 0.0)
            R.append(r)
            taps.append(w)
            use, sn = generator.random() < self.noise_p, generator.uniform(*self.noise)
            namp.append(noise_amplitude(sn if use else 0.0))
            s = generator.integers(0, 1 << 32, size=2, dtype=np.uint64)
            lo.append(int(s[0]))
            hi.append(int(s[1]))
        return DegradeParams(q, R, taps, namp, _as_i32(lo), _as_i32(hi))


def robustness_sweep(model, frames_u8, lengths, levels, size, chunk=None):
    """Clip probabilities of a clip model under a list of degradations, without leaving the GPU.

    frames_u8: uint8 [B, T, H, W, 3] on the model's device; lengths: int32 [B] there; levels: a list
    of ``dict(quality=, sigma=, noise=)`` (``DegradeParams.fixed``'s arguments; a missing one is 0),
    each applied to the whole batch; size: the model's input (OH, OW).  Each degraded clip is prepared
    with ``ClipAugment.eval(size)`` and scored by ``model(model.extract_features(clips), lengths)``, or
    by ``score_in_chunks(model, clips, lengths, chunk)`` when ``chunk`` is given, in eval mode under
    ``no_grad`` (the model's modes are restored).  -> probabilities [len(levels), B] on the device;
    with ``xcp.metrics`` that is AUC against quality."""
    from . import ops
    from .augment import ClipAugment
    from .streaming import score_in_chunks
    B, _, H, W, _ = frames_u8.shape
    prep = ClipAugment.eval(size)
    table = prep.sample([0] * B, H, W).to(frames_u8.device)   # the eval preset ignores the lengths: no host read
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    rows = []
    try:
        with torch.no_grad():
            for level in levels:
                d = ops.clip_degrade(frames_u8, lengths, DegradeParams.fixed(B, **level))
                clips, ln = ops.clip_augment(d, lengths, table, prep.size)
                if chunk is None:
                    p = model(model.extract_features(clips), ln)
                else:
                    p = score_in_chunks(model, clips, ln, chunk)
                rows.append(p.reshape(B))
    finally:
        for m, t in modes:
            m.training = t
    return torch.stack(rows)
