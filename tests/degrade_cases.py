"""Shared inputs of the clip-degradation tests (test_degrade_cpu.py, test_gpu_degrade.py).

Frames are seeded uint8 with smooth structure (two gradients and a sinusoid per channel) plus
noise: a purely random frame and a flat frame exercise too few quantisation outcomes.
"""
import functools

import numpy as np
import torch

SIZES = [(1, 1), (5, 6), (8, 8), (16, 16), (17, 19), (24, 40), (37, 53)]
SEAM = (45, 83)          # larger than the kernel's 32 x 32 workgroup tile both ways, no multiple of it or of 16
LENGTHS = (3, 1, 0)
QUALITIES = (1, 20, 50, 75, 100)
RADII = {1: 0.3, 3: 1.0, 7: 2.3}    # R -> a sigma whose ceil(3 sigma) is R
NOISES = (1.0, 8.0, 64.0)


def frames_u8(seed, shape):
    """Seeded uint8 [..., H, W, 3] frames: smooth structure plus noise, clipped to [0, 255]."""
    rng = np.random.default_rng(seed)
    *lead, H, W, C = shape
    y = np.arange(H, dtype=np.float64).reshape(H, 1, 1)
    x = np.arange(W, dtype=np.float64).reshape(1, W, 1)
    n = int(np.prod(lead)) if lead else 1
    out = np.empty((n, H, W, C), np.uint8)
    for i in range(n):
        a, b = rng.uniform(-3.0, 3.0, (2, 1, 1, C))
        ph, fy, fx = rng.uniform(0, 6.28, (1, 1, C)), rng.uniform(0.05, 0.6, (1, 1, C)), rng.uniform(0.05, 0.6, (1, 1, C))
        smooth = 128.0 + a * (y - H / 2) + b * (x - W / 2) + 60.0 * np.sin(fy * y + fx * x + ph)
        out[i] = np.clip(np.rint(smooth + rng.normal(0.0, 12.0, (H, W, C))), 0, 255).astype(np.uint8)
    return torch.from_numpy(out.reshape(shape))


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float((d * d).mean()), 1e-12))


def table(stage, i):
    """Three clips' ``DegradeParams``, each clip its own parameters: ``stage`` in ("jpeg", "blur",
    "noise", "all"), ``i`` rotates through the parameter lists."""
    from xcp.degrade import DegradeParams
    rows = []
    for b in range(3):
        q = QUALITIES[(i + b) % 5] if stage in ("jpeg", "all") else 0
        s = list(RADII.values())[(i + b) % 3] if stage in ("blur", "all") else 0.0
        n = NOISES[(i + b) % 3] if stage in ("noise", "all") else 0.0
        rows.append(DegradeParams.fixed(1, q, s, n, seed=(0x1234567 << 32) + 77 * i + b))
    return concat(rows)


def concat(rows):
    from xcp.degrade import DegradeParams
    return DegradeParams(*(torch.cat([getattr(r, k) for r in rows])
                           for k in ("quality", "radius", "taps", "namp", "seed_lo", "seed_hi")))


STAGES = ("jpeg", "blur", "noise", "all")


@functools.lru_cache(maxsize=None)
def batch_case(size, stage, i=0):
    """(frames uint8 [3, 3, H, W, 3], lengths, table, reference): computed once, shared, never modified."""
    from xcp.degrade import degrade_reference
    H, W = size
    u8 = frames_u8(1000 + 37 * H + W, (3, 3, H, W, 3))
    lengths = torch.tensor(LENGTHS, dtype=torch.int32)
    tab = table(stage, i)
    return u8, lengths, tab, degrade_reference(u8, lengths, tab)
