"""MFCC front end of the audio model: the arithmetic contract of ``xcp_mfcc_logmel`` /
``xcp_mfcc_dct`` (csrc/mfcc.hip), its tables, its fp64 restatement with an element-wise error
bound, the per-clip waveform-augmentation table with its host-side sampler, and the module that
turns padded PCM waveforms into XceptionLSTMA's input.

The reference prepares its audio off line (wavfake_audio_dataset.py:43):
``librosa.feature.mfcc(y, sr=16000, n_mfcc=13, n_fft=400, hop_length=160)``, then frames [0:120] /
[120:144] / [144:168] for train / eval / test, saved as ``.npy``.  librosa is not a dependency here
and is not installed where this is tested: fidelity to it rests on the formulas below (librosa's
own definitions of the Slaney mel scale, ``power_to_db`` and the orthonormal DCT-II) and on the
table anchors of tests/test_mfcc_cpu.py; it is not claimed as measured.

Tables (``MfccPlan``): built in fp64, each rounded once to fp32; the kernels take them as inputs and
never evaluate a sine or a cosine:
  window   periodic Hann w[n] = 0.5 - 0.5 cos(2 pi n / n_fft);
  twiddle  (cos, sin)(2 pi j / n_fft), j < n_fft; bin k, sample n uses entry (k n) mod n_fft;
  mel      the Slaney filterbank: mel = hz / (200 / 3) below 1 kHz, 15 + ln(hz / 1000) / (ln(6.4) / 27)
           above; n_mels + 2 points equally spaced in mel from fmin to fmax; triangles over the
           n_fft / 2 + 1 bin centres k sr / n_fft, each scaled by 2 / (f[i + 2] - f[i]); packed per
           filter as (first bin, count, weights);
  dct      orthonormal DCT-II rows D[0, j] = sqrt(1 / n_mels), D[i, j] = sqrt(2 / n_mels)
           cos(pi i (2 j + 1) / (2 n_mels)), i < n_mfcc.

Per clip b, in this order -- the contract between the kernels and ``mfcc_reference``:
  1. usable samples: n = clamp(len[b], 0, Nmax) - shift[b], y[i] = wav[b, shift[b] + i]; int16 is
     converted as (float) v / 32768.f; then times gain[b] in fp32 (one rounding); n <= 0: no frames;
  2. framing: Fall = 1 + n // hop; frame f covers y[f hop - n_fft / 2 ... + n_fft), zeros outside
     [0, n) (librosa's center=True, pad_mode="constant");
  3. spectrum: xw = y w (fp32); X_k = sum_n xw[n] (cos - i sin), k <= n_fft / 2, fp32 accumulation in any
     order; P_k = re^2 + im^2;
  4. mel: m_j = sum_k M[j, k] P_k; L_j = 10 log10f(max(m_j, amin)) (the accurate log10f);
  5. floor, if top_db is not None: L = max(L, Lmax - top_db), Lmax over ALL Fall frames and all bands
     of the clip, not only the emitted ones (the reference slices after power_to_db);
  6. output: c_i = sum_j D[i, j] L_j (fp32); emitted frame t is frame f0[b] + t;
     out_len[b] = min(Tout, max(0, Fall - f0[b])); rows t >= out_len[b] are zero; [B, Tout, n_mfcc], or
     [B, Tout, C, n_mfcc] with the row written C times (AudioDataset's unsqueeze(1).repeat(1, 3, 1)).

The kernels clamp shift to [0, Nmax] and f0 to >= 0 (``WaveParams.row``), so no table reads out of bounds.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24        # unit roundoff of fp32
LOG10F_ULPS = 4         # allowance for log10f and the multiplication by 10 (see mfcc_reference)
WAVE_COLS = 4           # XCP_MFCC_COLS of include/xcp.h: shift, f0, gain (fp32 bits), unused


class MfccConfig:
    """sr, n_fft, hop, n_mels, n_mfcc, fmin, fmax (None: sr / 2), top_db (None: no floor), amin.
    Supported: n_fft even in [16, 1024], hop >= 1, n_mfcc <= n_mels <= 128."""

    def __init__(self, sr=16000, n_fft=400, hop=160, n_mels=128, n_mfcc=13, fmin=0.0, fmax=None, top_db=80.0,
                 amin=1e-10):
        self.sr, self.n_fft, self.hop, self.n_mels, self.n_mfcc = int(sr), int(n_fft), int(hop), int(n_mels), int(n_mfcc)
        self.fmin = float(fmin)
        self.fmax = self.sr / 2 if fmax is None else float(fmax)
        self.top_db = None if top_db is None else float(top_db)
        self.amin = float(amin)
        if self.sr < 1 or self.n_fft % 2 or not 16 <= self.n_fft <= 1024 or self.hop < 1 \
                or not 1 <= self.n_mfcc <= self.n_mels <= 128 or not 0 <= self.fmin < self.fmax <= self.sr / 2 \
                or not (self.amin > 0 and math.isfinite(self.amin)) \
                or (self.top_db is not None and not (self.top_db >= 0 and math.isfinite(self.top_db))):
            raise ValueError("MfccConfig: need n_fft even in [16, 1024], hop >= 1, 1 <= n_mfcc <= n_mels <= 128, "
                             "0 <= fmin < fmax <= sr / 2, amin > 0, top_db >= 0 or None")

    @property
    def n_bins(self):
        return self.n_fft // 2 + 1

    def frames(self, n):
        """Fall of step 2 for n usable samples."""
        return 1 + n // self.hop if n > 0 else 0


# ---------------------------------------------------------------- tables (fp64)
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = 15.0                         # 1000 Hz at 200 / 3 Hz per mel
_LOGSTEP = math.log(6.4) / 27.0


def hz_to_mel(hz):
    hz = np.asarray(hz, np.float64)
    log_part = _MIN_LOG_MEL + np.log(np.maximum(hz, 1e-300) / _MIN_LOG_HZ) / _LOGSTEP
    return np.where(hz >= _MIN_LOG_HZ, log_part, hz * 3.0 / 200.0)


def mel_to_hz(mel):
    mel = np.asarray(mel, np.float64)
    return np.where(mel >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (mel - _MIN_LOG_MEL)), mel * 200.0 / 3.0)


def hann_window(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)


def mel_points(cfg):
    """The n_mels + 2 corner frequencies in Hz."""
    return mel_to_hz(np.linspace(hz_to_mel(cfg.fmin), hz_to_mel(cfg.fmax), cfg.n_mels + 2))


def mel_filterbank(cfg, normalised=True):
    """fp64 [n_mels, n_bins]; ``normalised=False``: the plain triangles (peak 1)."""
    f = mel_points(cfg)
    freqs = np.arange(cfg.n_bins, dtype=np.float64) * cfg.sr / cfg.n_fft
    fdiff = np.diff(f)
    ramps = f[:, None] - freqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    M = np.maximum(0.0, np.minimum(lower, upper))
    if normalised:
        M = M * (2.0 / (f[2:] - f[:-2]))[:, None]
    return M


def dct_rows(n_mfcc, n_mels):
    j = np.arange(n_mels, dtype=np.float64)
    D = math.sqrt(2.0 / n_mels) * np.cos(np.pi * np.arange(n_mfcc, dtype=np.float64)[:, None] * (2 * j + 1) / (2 * n_mels))
    D[0] = math.sqrt(1.0 / n_mels)
    return D


class DevicePlan:
    """The tables of an ``MfccPlan`` on a device, in the form the kernels read."""

    def __init__(self, plan, device):
        self.cfg = plan.cfg
        self.win = torch.from_numpy(plan.win).to(device)
        self.tw = torch.from_numpy(plan.tw).to(device)
        self.mel_fc = torch.from_numpy(plan.mel_fc).to(device)
        self.mel_w = torch.from_numpy(plan.mel_w).to(device)
        self.dct = torch.from_numpy(plan.dct).to(device)
        self.device = self.win.device


class MfccPlan:
    """The fp32 tables of a config (module docstring): ``win`` [n_fft], ``tw`` [n_fft, 2] (cos, sin),
    ``mel`` [n_mels, n_bins] dense and its packed form ``mel_fc`` int32 [n_mels, 2] (first bin, count) +
    ``mel_w`` [n_mels, max count], ``dct`` [n_mfcc, n_mels].  ``to(device)`` gives (and caches) the
    device form."""

    def __init__(self, cfg=None):
        self.cfg = cfg = MfccConfig() if cfg is None else cfg
        self.win = hann_window(cfg.n_fft).astype(np.float32)
        ang = 2.0 * np.pi * np.arange(cfg.n_fft, dtype=np.float64) / cfg.n_fft
        self.tw = np.stack([np.cos(ang), np.sin(ang)], 1).astype(np.float32)
        self.mel = mel_filterbank(cfg).astype(np.float32)
        self.dct = dct_rows(cfg.n_mfcc, cfg.n_mels).astype(np.float32)
        fc = np.zeros((cfg.n_mels, 2), np.int32)
        for j in range(cfg.n_mels):
            nz = np.nonzero(self.mel[j])[0]
            if nz.size:
                fc[j] = (nz[0], nz[-1] - nz[0] + 1)
        self.mel_fc = fc
        self.mel_w = np.zeros((cfg.n_mels, max(1, int(fc[:, 1].max()))), np.float32)
        for j in range(cfg.n_mels):
            self.mel_w[j, :fc[j, 1]] = self.mel[j, fc[j, 0]:fc[j, 0] + fc[j, 1]]
        self._dev = {}

    def empty_filters(self):
        return [j for j in range(self.cfg.n_mels) if self.mel_fc[j, 1] == 0]

    def to(self, device):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = DevicePlan(self, device)
        return self._dev[device]


# ---------------------------------------------------------------- the per-clip table
class WaveParams:
    """Per-clip table as host tensors: int32 [B] ``shift`` (first usable sample) and ``f0`` (first emitted
    frame), fp32 [B] ``gain``.  ``pack()`` / ``to(device)`` give the int32 [B, 4] form the kernels read
    (columns: shift, f0, gain's bit pattern, unused)."""

    def __init__(self, shift, f0, gain):
        B = len(shift)
        self.shift = torch.as_tensor(shift, dtype=torch.int32).reshape(B).clone()
        self.f0 = torch.as_tensor(f0, dtype=torch.int32).reshape(B).clone()
        self.gain = torch.as_tensor(gain, dtype=torch.float32).reshape(B).clone()

    def __len__(self):
        return self.shift.numel()

    @classmethod
    def identity(cls, B, f0=0):
        z = torch.zeros(B, dtype=torch.int32)
        return cls(z, z + int(f0), torch.ones(B))

    def pack(self, out=None):
        B = len(self)
        t = torch.zeros((B, WAVE_COLS), dtype=torch.int32) if out is None else out
        if t.dtype != torch.int32 or tuple(t.shape) != (B, WAVE_COLS):
            raise ValueError(f"pack: out must be int32 [{B}, {WAVE_COLS}]")
        t.zero_()
        t[:, 0] = self.shift
        t[:, 1] = self.f0
        t[:, 2] = self.gain.contiguous().view(torch.int32)
        return t

    @classmethod
    def unpack(cls, packed):
        t = packed.detach().cpu().contiguous()
        return cls(t[:, 0], t[:, 1], t[:, 2].contiguous().view(torch.float32))

    def to(self, device, non_blocking=False):
        """The packed table on ``device``: what ``ops.mfcc`` takes and a captured graph re-reads
        (overwrite it in place with ``copy_`` of another table's ``pack()``)."""
        return self.pack().to(device, non_blocking=non_blocking)

    def equal(self, other):
        return all(torch.equal(getattr(self, k), getattr(other, k)) for k in ("shift", "f0", "gain"))

    def validate(self, B, Nmax):
        """Raise ValueError unless this is a table for B clips of Nmax samples that needs no clamping."""
        if len(self) != B:
            raise ValueError(f"wave table has {len(self)} rows for {B} clips")
        bad = (self.shift < 0) | (self.shift > Nmax) | (self.f0 < 0)
        if bool(bad.any()):
            raise ValueError(f"wave table rows {bad.nonzero().flatten().tolist()} are out of range: need "
                             f"0 <= shift <= {Nmax}, f0 >= 0")
        if not bool(torch.isfinite(self.gain).all()):
            raise ValueError("wave table: gain is not finite")

    def row(self, i, Nmax):
        """(shift, f0, gain) of row i, clamped exactly as the kernels clamp what they read."""
        s, f = int(self.shift[i]), int(self.f0[i])
        return min(max(s, 0), Nmax), max(f, 0), self.gain[i].item()


class WaveAugment:
    """Sampler of ``WaveParams`` (``ClipAugment``'s style): a sub-hop re-framing offset
    shift ~ U{0..max_shift}, a gain of U(lo, hi) dB, and the start frame of a window of ``frames`` frames,
    uniform over the starts that keep the window inside the clip (``split_offset`` when the clip is
    too short, and added to every start).  Draws come from a numpy.random.Generator in clip order:
    shift, gain, start."""

    def __init__(self, cfg, frames, max_shift=0, gain_db=(0.0, 0.0), split_offset=0):
        self.cfg = cfg
        self.frames = int(frames)
        self.max_shift = int(max_shift)
        self.gain_db = (float(gain_db[0]), float(gain_db[1]))
        self.split_offset = int(split_offset)
        self.fixed_f0 = None   # set by eval()
        if self.frames < 1 or self.max_shift < 0 or not self.gain_db[0] <= self.gain_db[1] or self.split_offset < 0 \
                or not all(math.isfinite(g) for g in self.gain_db):
            raise ValueError("WaveAugment: need frames >= 1, max_shift >= 0, gain_db = (lo, hi) with lo <= hi, "
                             "split_offset >= 0")

    @classmethod
    def eval(cls, cfg, frames, f0=0):
        """The deterministic preset: no shift, gain 1, frames [f0, f0 + frames).  (frames, f0) = (120, 0) /
        (24, 120) / (24, 144) are the reference's train / eval / test splits."""
        if f0 < 0:
            raise ValueError("WaveAugment.eval: f0 >= 0")
        self = cls(cfg, frames)
        self.fixed_f0 = int(f0)
        return self

    def sample(self, lengths, generator=None):
        lengths = [int(x) for x in lengths]
        if self.fixed_f0 is not None:
            return WaveParams.identity(len(lengths), self.fixed_f0)
        if generator is None:
            raise ValueError("WaveAugment.sample: pass a numpy.random.Generator")
        shift, f0, gain = [], [], []
        for ln in lengths:
            s = int(generator.integers(0, self.max_shift + 1))
            s = min(s, max(ln, 0))
            db = generator.uniform(*self.gain_db)
            spare = self.cfg.frames(ln - s) - self.split_offset - self.frames
            start = int(generator.integers(0, spare + 1)) if spare >= 0 else 0
            shift.append(s)
            f0.append(self.split_offset + start)
            gain.append(10.0 ** (db / 20.0))
        return WaveParams(shift, f0, np.asarray(gain, np.float64))


# ---------------------------------------------------------------- fp64 restatement + bound
def _ulp32(v):
    """spacing of fp32 at |v| (fp64 array); zero -> the smallest normal's"""
    _, e = np.frexp(np.maximum(np.abs(v), 2.0 ** -126))
    return np.ldexp(1.0, e - 24)


def frame_matrix(y32, n_frames, cfg):
    """fp32 [n_frames, n_fft]: frame f = y[f hop - n_fft / 2 ... + n_fft), zeros outside y (step 2)."""
    pad = cfg.n_fft // 2
    need = (n_frames - 1) * cfg.hop + cfg.n_fft
    buf = np.zeros(max(need, pad + y32.size), np.float32)
    buf[pad:pad + y32.size] = y32
    idx = np.arange(n_frames)[:, None] * cfg.hop + np.arange(cfg.n_fft)[None, :]
    return buf[idx]


def clip_samples(wav_row, length, shift, gain):
    """Step 1 on one clip: fp32 y [n] (n may be 0)."""
    Nmax = wav_row.shape[0]
    L = min(max(int(length), 0), Nmax)
    seg = wav_row[shift:L] if L > shift else wav_row[:0]
    if seg.dtype == np.int16:
        seg = seg.astype(np.float32) / np.float32(32768.0)
    return seg.astype(np.float32) * np.float32(gain)


def mfcc_reference(wav, lengths, plan, table=None, out_frames=None, channels=3):
    """Steps 1-6 of the module docstring in fp64 on the fp32-rounded inputs (waveform, gain, tables).
    wav: fp32 or int16 [B, Nmax]; lengths [B]; table: a ``WaveParams`` or None (identity).
    Returns (ref64, lim, out_len): fp64 tensors [B, Tout, channels, n_mfcc] ([B, Tout, n_mfcc] for
    channels = 1, as ``ops.mfcc``) and int32 [B].

    ``lim`` bounds |kernel - ref64| element by element with no fitted constant, propagated as an
    interval.  e(n, A) = (n + 2) 2^-24 A is tests/elementwise.py's bound for an fp32 sum of n terms whose
    absolute values sum to A, accumulated in any order, products fused or not.
      re, im   n = n_fft + 1 (one to spare; xw itself is restated bit for bit):
               d_re = e(n_fft + 1, sum |xw| |cos|), d_im likewise;
      P        |P' - P| <= 2 |re| d_re + d_re^2 + 2 |im| d_im + d_im^2 + 3 * 2^-24 * ((|re| + d_re)^2 + (|im| + d_im)^2)
               (the squares and their sum: three roundings, fewer when fused);
      m        d_m = sum M d_P + e(count_j, sum M (P + d_P));
      L        10 log10 of [max(m - d_m, amin), max(m + d_m, amin)], each end moved outward by 4 ulp of
               its fp32 value: the ROCm device library documents log10f at 2 ulp, which is at most 2.5 ulp
               of ten times it, and the multiplication by 10 adds half an ulp; 4 is that documentation
               with a margin, not a measurement;
      floor    [max Llo, max Lhi] is the interval of Lmax; minus top_db, moved outward by one fp32
               rounding of the difference; max(L, .) end by end (the map is 1-Lipschitz and monotone);
      c        the half-widths h through |D|: lim = sum |D| h + e(n_mels, sum |D| (|L| + h)).
    """
    cfg = plan.cfg
    wav = np.ascontiguousarray(wav.detach().cpu().numpy() if torch.is_tensor(wav) else wav)
    if wav.dtype not in (np.float32, np.int16) or wav.ndim != 2:
        raise ValueError("mfcc_reference: wav is fp32 or int16 [B, Nmax]")
    B, Nmax = wav.shape
    table = WaveParams.identity(B) if table is None else table
    Tout = 1 + Nmax // cfg.hop if out_frames is None else int(out_frames)
    nb, n_fft = cfg.n_bins, cfg.n_fft
    kn = (np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    Cm, Sm = plan.tw[kn, 0].astype(np.float64), plan.tw[kn, 1].astype(np.float64)     # [nb, n_fft]
    M, D = plan.mel.astype(np.float64), plan.dct.astype(np.float64)
    cnt = plan.mel_fc[:, 1].astype(np.float64)
    amin = float(np.float32(cfg.amin))
    ref = np.zeros((B, Tout, cfg.n_mfcc))
    lim = np.zeros((B, Tout, cfg.n_mfcc))
    out_len = np.zeros(B, np.int32)
    for b in range(B):
        shift, f0, gain = table.row(b, Nmax)
        y = clip_samples(wav[b], lengths[b], shift, gain)
        Fall = cfg.frames(y.size)
        n_out = min(Tout, max(0, Fall - f0))
        out_len[b] = n_out
        if n_out == 0:
            continue
        xw = (frame_matrix(y, Fall, cfg) * plan.win[None, :]).astype(np.float64)      # fp32 product, then widened
        axw = np.abs(xw)
        re, im = xw @ Cm.T, xw @ Sm.T
        d_re = (n_fft + 3) * U32 * (axw @ np.abs(Cm).T)
        d_im = (n_fft + 3) * U32 * (axw @ np.abs(Sm).T)
        P = re * re + im * im
        are, aim = np.abs(re), np.abs(im)
        d_P = 2 * are * d_re + d_re ** 2 + 2 * aim * d_im + d_im ** 2 + 3 * U32 * ((are + d_re) ** 2 + (aim + d_im) ** 2)
        m = P @ M.T
        d_m = d_P @ M.T + (cnt[None, :] + 2) * U32 * ((P + d_P) @ M.T)
        L = 10.0 * np.log10(np.maximum(m, amin))
        Llo = 10.0 * np.log10(np.maximum(m - d_m, amin))
        Lhi = 10.0 * np.log10(np.maximum(m + d_m, amin))
        Llo, Lhi = Llo - LOG10F_ULPS * _ulp32(Llo), Lhi + LOG10F_ULPS * _ulp32(Lhi)
        if cfg.top_db is not None:
            td = float(np.float32(cfg.top_db))
            fl, flo, fhi = L.max() - td, Llo.max() - td, Lhi.max() - td
            flo, fhi = flo - U32 * abs(flo), fhi + U32 * abs(fhi)
            L, Llo, Lhi = np.maximum(L, fl), np.maximum(Llo, flo), np.maximum(Lhi, fhi)
        sel = slice(f0, f0 + n_out)
        L, h = L[sel], np.maximum(Lhi[sel] - L[sel], L[sel] - Llo[sel])
        ref[b, :n_out] = L @ D.T
        lim[b, :n_out] = h @ np.abs(D).T + (cfg.n_mels + 2) * U32 * ((np.abs(L) + h) @ np.abs(D).T)
    ref, lim = torch.from_numpy(ref), torch.from_numpy(lim)
    if channels and channels > 1:
        ref = ref.unsqueeze(2).repeat(1, 1, channels, 1)
        lim = lim.unsqueeze(2).repeat(1, 1, channels, 1)
    return ref, lim, torch.from_numpy(out_len)


# ---------------------------------------------------------------- the module
class WaveFrontEnd:
    """Padded PCM waveforms -> XceptionLSTMA's input, on the GPU: ``(wav [B, Nmax] fp32 or int16, lengths
    int32 [B], generator=None) -> (x [B, T, 3, n_mfcc], seq_lengths int32 [B])``, both on wav's device,
    for ``model.extract_features(x)`` and ``model(features, seq_lengths)``.  augment: a ``WaveAugment``
    (T = its ``frames``; lengths are then read on the host to draw the table, so pass host lengths or
    accept the synchronisation) or None (every frame of the batch, no table, nothing read back)."""

    def __init__(self, cfg=None, augment=None, dtype=torch.float32):
        self.plan = MfccPlan(cfg)
        self.cfg = self.plan.cfg
        self.augment = augment
        self.dtype = dtype

    def __call__(self, wav, lengths, generator=None):
        from . import ops
        table, T = None, None
        if self.augment is not None:
            table = self.augment.sample(lengths.tolist() if torch.is_tensor(lengths) else lengths, generator)
            T = self.augment.frames
        if not torch.is_tensor(lengths):
            lengths = torch.as_tensor(lengths, dtype=torch.int32)
        lengths = lengths.to(device=wav.device, dtype=torch.int32)
        return ops.mfcc(wav, lengths, self.plan, table, T, 3, self.dtype)
