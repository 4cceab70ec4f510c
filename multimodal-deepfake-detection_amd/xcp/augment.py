"""Clip augmentation on the GPU: the per-clip parameter table, its host-side sampler and the
pure-torch restatement of ``xcp_clip_augment`` (frames.hip) that the tests use as their oracle.

The reference's training scripts augment (train_au_patch.py:193 ``augment_train=True``,
``augment_minority`` in train_visual.py) and Xception.py:12-17 asks for mean 0.5 / std 0.5 and a
resize + centre crop at evaluation.  Here the data-dependent part is a table of a few dozen
bytes per clip, drawn on the host; one kernel reads the uint8 clip once and writes the model's
input once.  Every frame of a clip shares the clip's parameters (a face must not jump between
frames).

Order of operations -- the contract between the kernel and ``augment_reference``:
  1. out_len = min(Tout, max(0, ceil((clamp(len, 0, Tmax) - t0) / tstride))); output frame t is
     source frame t0 + t * tstride; frames t >= out_len are zero (no affine, no fill);
  2. sub-pixel = (float)byte / 255.f;
  3. the crop box (y0, x0, bh, bw) is resampled bilinearly to (OH, OW), align_corners=False,
     with ATen's fp32 index / weight formulas on box-relative indices, products then sums;
  4. flip: output column ow takes resampled column OW - 1 - ow;
  5. v = v * a[c], rounded, then v = v + b[c], rounded (no FMA);
  6. v = fill[c] inside the erase rectangle (post-flip output coordinates, clipped to the output);
  7. cast to the output dtype (bf16: round to nearest even).
"""
import math

import numpy as np
import torch

AUG_COLS = 24   # XCP_AUG_COLS of include/xcp.h
_INT_FIELDS = ("t0", "tstride", "y0", "x0", "bh", "bw", "flip", "ey0", "ex0", "eh", "ew")   # columns 0..10
_F32_FIELDS = (("a", 12), ("b", 15), ("fill", 18))                                           # 3 columns each


def _clampi(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class AugmentParams:
    """The per-clip table as named host tensors: int32 [B] ``t0, tstride, y0, x0, bh, bw, flip,
    ey0, ex0, eh, ew`` and fp32 [B, 3] ``a, b, fill``.  ``pack()`` / ``to(device)`` give the
    int32 [B, 24] form the kernel reads (include/xcp.h lists the columns)."""

    def __init__(self, **fields):
        B = len(fields["t0"])
        for k in _INT_FIELDS:
            setattr(self, k, torch.as_tensor(fields[k], dtype=torch.int32).reshape(B).clone())
        for k, _ in _F32_FIELDS:
            setattr(self, k, torch.as_tensor(fields[k], dtype=torch.float32).reshape(B, 3).clone())

    def __len__(self):
        return self.t0.numel()

    @classmethod
    def identity(cls, B, H, W):
        """Whole frame, no flip, a = 1, b = 0, no erase, t0 = 0, stride 1: ``frames_prep``."""
        z = torch.zeros(B, dtype=torch.int32)
        return cls(t0=z, tstride=z + 1, y0=z, x0=z, bh=z + H, bw=z + W, flip=z, ey0=z, ex0=z, eh=z, ew=z,
                   a=torch.ones(B, 3), b=torch.zeros(B, 3), fill=torch.zeros(B, 3))

    def pack(self, out=None):
        """int32 [B, 24] host tensor (``out``: a preallocated, e.g. pinned, one to fill)."""
        B = len(self)
        t = torch.zeros((B, AUG_COLS), dtype=torch.int32) if out is None else out
        if t.dtype != torch.int32 or tuple(t.shape) != (B, AUG_COLS):
            raise ValueError(f"pack: out must be int32 [{B}, {AUG_COLS}]")
        t.zero_()
        for i, k in enumerate(_INT_FIELDS):
            t[:, i] = getattr(self, k)
        for k, c in _F32_FIELDS:
            t[:, c:c + 3] = getattr(self, k).contiguous().view(torch.int32)
        return t

    @classmethod
    def unpack(cls, packed):
        t = packed.detach().cpu().contiguous()
        f = {k: t[:, i] for i, k in enumerate(_INT_FIELDS)}
        f.update({k: t[:, c:c + 3].contiguous().view(torch.float32) for k, c in _F32_FIELDS})
        return cls(**f)

    def to(self, device, non_blocking=False):
        """The packed table on ``device``: what ``ops.clip_augment`` takes and a captured graph
        re-reads (overwrite it in place with ``copy_`` of another table's ``pack()``)."""
        return self.pack().to(device, non_blocking=non_blocking)

    def equal(self, other):
        return all(torch.equal(getattr(self, k), getattr(other, k))
                   for k in _INT_FIELDS + tuple(k for k, _ in _F32_FIELDS))

    def validate(self, B, H, W):
        """Raise ValueError unless this is a table for B clips of H x W frames that needs no clamping."""
        if len(self) != B:
            raise ValueError(f"augment table has {len(self)} rows for {B} clips")
        bad = ((self.t0 < 0) | (self.tstride < 1) | (self.bh < 1) | (self.bw < 1) | (self.y0 < 0) | (self.x0 < 0)
               | (self.y0.long() + self.bh > H) | (self.x0.long() + self.bw > W) | (self.flip < 0) | (self.flip > 1)
               | (self.eh < 0) | (self.ew < 0))
        if bool(bad.any()):
            raise ValueError(f"augment table rows {bad.nonzero().flatten().tolist()} are out of range: need t0 >= 0, "
                             f"tstride >= 1, a crop box inside the {H} x {W} frame, flip in (0, 1), eh, ew >= 0")
        for k, _ in _F32_FIELDS:
            if not bool(torch.isfinite(getattr(self, k)).all()):
                raise ValueError(f"augment table: {k} is not finite")

    def row(self, i, Tmax, H, W):
        """Row i as Python ints, clamped exactly as the kernel clamps what it reads."""
        g = {k: int(getattr(self, k)[i]) for k in _INT_FIELDS}
        bh, bw = _clampi(g["bh"], 1, H), _clampi(g["bw"], 1, W)
        g.update(t0=_clampi(g["t0"], 0, Tmax), tstride=_clampi(g["tstride"], 1, Tmax), bh=bh, bw=bw,
                 y0=_clampi(g["y0"], 0, H - bh), x0=_clampi(g["x0"], 0, W - bw), flip=int(g["flip"] != 0))
        return g


def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _lin_idx(n_out, n_in, scale):
    """lin_idx of frames.hip for every destination index, in fp32 tensor ops (one rounding each)."""
    dst = torch.arange(n_out, dtype=torch.float32)
    src = scale * (dst + 0.5) - 0.5
    src = torch.where(src < 0, torch.zeros_like(src), src)
    i0 = src.floor().to(torch.int64).clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l1 = (src - i0.to(torch.float32)).clamp(0.0, 1.0)
    return i0, i1, 1.0 - l1, l1


def augment_reference(frames_u8, lengths, params, size, out_frames=None, dtype=torch.float32, channels_last=False):
    """``ops.clip_augment`` restated in torch on the CPU: explicit gathers and one fp32 operation
    per step, in the kernel's order (module docstring), so the two agree bit for bit.
    frames_u8 uint8 [B, Tmax, H, W, 3], lengths [B], params an ``AugmentParams`` (clamped here
    as the kernel clamps it).  Returns (clips [B, Tout, 3, OH, OW], out_lengths int32 [B])."""
    frames_u8 = torch.as_tensor(frames_u8).cpu()
    B, Tmax, H, W, _ = frames_u8.shape
    OH, OW = size
    Tout = Tmax if out_frames is None else int(out_frames)
    out = torch.zeros((B, Tout, OH, OW, 3), dtype=torch.float32)
    out_len = torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        g = params.row(b, Tmax, H, W)
        L = _clampi(int(lengths[b]), 0, Tmax)
        n = min(Tout, max(0, -(-(L - g["t0"]) // g["tstride"])))
        out_len[b] = n
        if n == 0:
            continue
        src = g["t0"] + g["tstride"] * torch.arange(n)
        box = frames_u8[b, src, g["y0"]:g["y0"] + g["bh"], g["x0"]:g["x0"] + g["bw"]].to(torch.float32) / 255.0
        h0, h1, lh0, lh1 = _lin_idx(OH, g["bh"], _f32(g["bh"]) / _f32(OH))
        w0, w1, lw0, lw1 = _lin_idx(OW, g["bw"], _f32(g["bw"]) / _f32(OW))
        lw0, lw1 = lw0.view(1, 1, OW, 1), lw1.view(1, 1, OW, 1)
        lh0, lh1 = lh0.view(1, OH, 1, 1), lh1.view(1, OH, 1, 1)
        r0, r1 = box[:, h0], box[:, h1]                             # [n, OH, bw, 3]
        t0 = r0[:, :, w0] * lw0 + r0[:, :, w1] * lw1                # products, then the sum
        t1 = r1[:, :, w0] * lw0 + r1[:, :, w1] * lw1
        v = t0 * lh0 + t1 * lh1                                     # [n, OH, OW, 3]
        if g["flip"]:
            v = v.flip(2)
        v = v * params.a[b].view(1, 1, 1, 3)
        v = v + params.b[b].view(1, 1, 1, 3)
        ylo, yhi = max(g["ey0"], 0), min(g["ey0"] + g["eh"], OH)
        xlo, xhi = max(g["ex0"], 0), min(g["ex0"] + g["ew"], OW)
        if yhi > ylo and xhi > xlo:
            v[:, ylo:yhi, xlo:xhi] = params.fill[b].view(1, 1, 1, 3)
        out[b, :n] = v
    out = out.to(dtype)
    if channels_last:
        return out.permute(0, 1, 4, 2, 3), out_len
    return out.permute(0, 1, 4, 2, 3).contiguous(), out_len


class ClipAugment:
    """Sampler of ``AugmentParams``: random-resized crop, horizontal flip, contrast / brightness
    folded with mean / std into one per-channel affine, random erase, frame sub-sampling.

    size: (OH, OW) of the model input.  scale: range of the crop's share of the frame area;
    ratio: range of its width / height, log-uniform (absolute, as torchvision's
    RandomResizedCrop: ratio (1, 1) on a non-square frame is a square box).  flip: probability.
    contrast c: kappa ~ U(1 - c, 1 + c) about 0.5; brightness beta: delta ~ U(-beta, beta);
    x -> ((x - 0.5) kappa + 0.5 + delta - mean) / std = a x + b.  erase: probability of one
    zero-filled rectangle of erase_scale of the output area, erase_ratio width / height.
    frames: output frames per clip (None: as many as the batch has); strides: the temporal
    strides to draw from; t0 is uniform over the starts that keep ``frames`` real frames when the
    clip is long enough for that, else 0."""

    def __init__(self, size, scale=(0.6, 1.0), ratio=(3 / 4, 4 / 3), flip=0.5, brightness=0.0, contrast=0.0,
                 mean=(0.5,) * 3, std=(0.5,) * 3, erase=0.0, erase_scale=(0.02, 0.2), erase_ratio=(0.3, 3.3),
                 frames=None, strides=(1,)):
        self.size = (int(size[0]), int(size[1]))
        self.scale, self.ratio = tuple(map(float, scale)), tuple(map(float, ratio))
        self.flip, self.brightness, self.contrast, self.erase = float(flip), float(brightness), float(contrast), float(erase)
        self.mean, self.std = np.asarray(mean, np.float64).reshape(3), np.asarray(std, np.float64).reshape(3)
        self.erase_scale, self.erase_ratio = tuple(map(float, erase_scale)), tuple(map(float, erase_ratio))
        self.frames = None if frames is None else int(frames)
        self.strides = tuple(int(s) for s in strides)
        self.crop_fraction = None   # set by eval(): the deterministic centred box
        if min(self.size) < 1 or not 0 < self.scale[0] <= self.scale[1] or not 0 < self.ratio[0] <= self.ratio[1] \
                or not 0 <= self.flip <= 1 or not 0 <= self.erase <= 1 or self.brightness < 0 or self.contrast < 0 \
                or (self.std <= 0).any() or not 0 < self.erase_scale[0] <= self.erase_scale[1] \
                or not 0 < self.erase_ratio[0] <= self.erase_ratio[1] or not self.strides or min(self.strides) < 1 \
                or (self.frames is not None and self.frames < 1):
            raise ValueError("ClipAugment: bad argument (ranges are 0 < lo <= hi, probabilities in [0, 1], "
                             "std > 0, strides >= 1, frames >= 1)")

    @classmethod
    def eval(cls, size, crop_fraction=299 / 333, mean=(0.5,) * 3, std=(0.5,) * 3):
        """The deterministic evaluation preset: a centred box of round(H f) x round(W f) resized
        to ``size``, normalised, nothing random.  This is crop-then-resize; torchvision's
        Resize + CenterCrop is resize-then-crop, which samples the same region of the frame
        through a different (two-step) filter."""
        if not 0 < crop_fraction <= 1:
            raise ValueError("ClipAugment.eval: crop_fraction must be in (0, 1]")
        self = cls(size, scale=(1.0, 1.0), ratio=(1.0, 1.0), flip=0.0, mean=mean, std=std)
        self.crop_fraction = float(crop_fraction)
        return self

    def fold(self, kappa, delta):
        """Contrast kappa about 0.5, then brightness delta, then (x - mean) / std, as one
        per-channel a x + b: (a, b), fp64 [3] each."""
        return kappa / self.std, (0.5 - 0.5 * kappa + delta - self.mean) / self.std

    def _box(self, rng, H, W):
        if self.crop_fraction is not None:
            bh = _clampi(int(round(H * self.crop_fraction)), 1, H)
            bw = _clampi(int(round(W * self.crop_fraction)), 1, W)
            return (H - bh) // 2, (W - bw) // 2, bh, bw
        s = rng.uniform(*self.scale)
        r = math.exp(rng.uniform(math.log(self.ratio[0]), math.log(self.ratio[1])))
        bh = _clampi(int(round(math.sqrt(s * H * W / r))), 1, H)
        bw = _clampi(int(round(math.sqrt(s * H * W * r))), 1, W)
        return int(rng.integers(0, H - bh + 1)), int(rng.integers(0, W - bw + 1)), bh, bw

    def sample(self, lengths, H, W, generator=None):
        """One independent draw per clip from ``generator`` (a numpy.random.Generator; only the
        ``eval`` preset, which ignores its draws, may omit it), in clip order: box, flip,
        contrast, brightness, erase, stride, start.  -> AugmentParams."""
        if generator is None:
            if self.crop_fraction is None:
                raise ValueError("ClipAugment.sample: pass a numpy.random.Generator")
            generator = np.random.default_rng(0)
        OH, OW = self.size
        rows = {k: [] for k in _INT_FIELDS}
        a, b = [], []
        for ln in [int(x) for x in lengths]:
            y0, x0, bh, bw = self._box(generator, H, W)
            flip = int(generator.random() < self.flip)
            kappa = generator.uniform(1 - self.contrast, 1 + self.contrast)
            delta = generator.uniform(-self.brightness, self.brightness)
            ey0 = ex0 = eh = ew = 0
            if generator.random() < self.erase:
                es = generator.uniform(*self.erase_scale)
                er = math.exp(generator.uniform(math.log(self.erase_ratio[0]), math.log(self.erase_ratio[1])))
                eh = _clampi(int(round(math.sqrt(es * OH * OW / er))), 1, OH)
                ew = _clampi(int(round(math.sqrt(es * OH * OW * er))), 1, OW)
                ey0, ex0 = int(generator.integers(0, OH - eh + 1)), int(generator.integers(0, OW - ew + 1))
            ts = self.strides[int(generator.integers(0, len(self.strides)))]
            t0 = 0
            if self.frames is not None:
                spare = ln - ((self.frames - 1) * ts + 1)
                t0 = int(generator.integers(0, spare + 1)) if spare >= 0 else 0
            for k, v in zip(_INT_FIELDS, (t0, ts, y0, x0, bh, bw, flip, ey0, ex0, eh, ew)):
                rows[k].append(v)
            ab = self.fold(kappa, delta)
            a.append(ab[0])
            b.append(ab[1])
        n = len(a)
        return AugmentParams(a=np.asarray(a, np.float64).reshape(n, 3), b=np.asarray(b, np.float64).reshape(n, 3),
                             fill=torch.zeros(n, 3), **rows)
