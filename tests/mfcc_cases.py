"""Shared by test_mfcc_cpu.py and test_gpu_mfcc.py: the test signals, an fp32 torch emulation of steps 1-6
of xcp/audio.py's contract (with the mutations the sensitivity tests apply), and the judgement
|got - ref64| <= lim, element by element, nothing excluded."""
import numpy as np
import torch

from elementwise import ulp_bf16
from xcp.audio import MfccConfig, MfccPlan, WaveParams, clip_samples, frame_matrix, mfcc_reference  # noqa: F401

SR = 16000


def noise(seed, n, amp=0.3):
    return (amp * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def stepped_noise(seed=3, n=16000):
    """"The noise case": one second of Gaussian noise in three levels -- loud (0.2 s), 40 dB down (0.4 s),
    90 dB down (0.4 s).  With f0 = 30, Tout = 60 the emitted frames 30..89 lie in the two quiet parts: the
    clip-wide maximum (the loud part, not emitted) puts the quietest frames on the floor, the maximum
    of the emitted frames alone would not."""
    env = np.concatenate([np.full(3200, 0.3), np.full(6400, 3e-3), np.full(n - 9600, 1e-5)])
    return (env * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


STEPPED = dict(f0=30, frames=60)


def tone_plus_weak_noise(seed=4, n=8000):
    t = np.arange(n) / SR
    return (0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.5e-4 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def chirp(n=8000):
    t = np.arange(n) / SR
    return (0.4 * np.sin(2 * np.pi * (100.0 * t + 0.5 * 14000.0 * t * t))).astype(np.float32)


def to_i16(x):
    return np.clip(np.round(x * 32767.0), -32768, 32767).astype(np.int16)


def batch(rows, dtype=np.float32):
    """Zero-padded [B, Nmax] tensor + int32 lengths from a list of 1-D arrays."""
    Nmax = max(1, max(len(r) for r in rows))
    w = np.zeros((len(rows), Nmax), dtype)
    for i, r in enumerate(rows):
        w[i, :len(r)] = r
    return torch.from_numpy(w), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def emulate_f32(wav, lengths, plan, table=None, out_frames=None, channels=3, drop_bin=None, drop_weight=None, hop=None,
                lmax_emitted_only=False):
    """Steps 1-6 in fp32 torch ops on the CPU (matmuls for the three sums: some fp32 order).  The keyword
    arguments are the mutations of the sensitivity test: a spectrum bin left out, one mel weight (j, k)
    left out, a different hop, Lmax over the emitted frames only."""
    cfg = plan.cfg
    wav = wav.numpy() if torch.is_tensor(wav) else wav
    B, Nmax = wav.shape
    table = WaveParams.identity(B) if table is None else table
    hop = cfg.hop if hop is None else hop
    fcfg = MfccConfig(cfg.sr, cfg.n_fft, hop, cfg.n_mels, cfg.n_mfcc, cfg.fmin, cfg.fmax, cfg.top_db, cfg.amin)
    Tout = 1 + Nmax // cfg.hop if out_frames is None else out_frames
    kn = (np.arange(cfg.n_bins)[:, None] * np.arange(cfg.n_fft)[None, :]) % cfg.n_fft
    Cm, Sm = torch.from_numpy(plan.tw[kn, 0]), torch.from_numpy(plan.tw[kn, 1])
    M, D = torch.from_numpy(plan.mel.copy()), torch.from_numpy(plan.dct)
    if drop_weight is not None:
        assert M[drop_weight] != 0
        M[drop_weight] = 0
    out = torch.zeros((B, Tout, cfg.n_mfcc), dtype=torch.float32)
    for b in range(B):
        shift, f0, gain = table.row(b, Nmax)
        y = clip_samples(wav[b], lengths[b], shift, gain)
        Fall = fcfg.frames(y.size)
        n_out = min(Tout, max(0, Fall - f0))
        if n_out == 0:
            continue
        xw = torch.from_numpy(frame_matrix(y, Fall, fcfg) * plan.win[None, :])
        re, im = xw @ Cm.T, xw @ Sm.T
        P = re * re + im * im
        if drop_bin is not None:
            P[:, drop_bin] = 0
        L = 10.0 * torch.log10(torch.clamp_min(P @ M.T, float(np.float32(cfg.amin))))
        if cfg.top_db is not None:
            lmax = L[f0:f0 + n_out].max() if lmax_emitted_only else L.max()
            L = torch.maximum(L, lmax - np.float32(cfg.top_db))
        out[b, :n_out] = L[f0:f0 + n_out] @ D.T
    assert out.dtype == torch.float32
    return out if channels == 1 else out.unsqueeze(2).repeat(1, 1, channels, 1)


def ratio(got, ref64, lim):
    """max over the elements of |got - ref64| / lim (0 / 0 = 0, x / 0 = inf)."""
    d = (got.double() - ref64).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / lim.clamp_min(1e-300))
    return r.max().item() if r.numel() else 0.0


def assert_within_lim(got, ref64, lim, tag=""):
    assert got.shape == ref64.shape == lim.shape, (got.shape, ref64.shape, lim.shape)
    assert not torch.isnan(got.double()).any(), f"{tag}: NaN"
    worst = ratio(got, ref64, lim)
    print(f"{tag}: worst d/lim = {worst:.4f}")
    assert worst <= 1.0, f"{tag}: worst d/lim = {worst:.3f}"
    return worst


def assert_bf16_within_lim(got, ref64, lim, tag=""):
    """elementwise.assert_bf16_stored's neighbour rule with e = lim: the kernel stores a bf16 neighbour of an
    fp32 value within lim of ref64, so |got - ref64| <= ulp_bf16(|ref64| + lim) + lim."""
    assert got.dtype == torch.bfloat16
    return assert_within_lim(got, ref64, ulp_bf16(ref64.abs() + lim) + lim, tag)


def assert_zero_rows(got, out_len):
    """rows t >= out_len[b] are zero, bit for bit (+0)."""
    bits = got.contiguous().view(torch.int32 if got.dtype == torch.float32 else torch.int16)
    for b, n in enumerate(out_len.tolist()):
        assert not bits[b, n:].any(), f"clip {b}: a padded row is not +0"
