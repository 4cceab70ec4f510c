"""Shared cases of the clip-augmentation tests (test_augment_cpu.py, test_gpu_augment.py).

CASES: (crop box (y0, x0, bh, bw) on a 24 x 20 frame, output size, interpolated?).  The boxes
whose resampling touches no second source pixel with a non-zero weight (a box of the output's
size; the exact 2:1 x 3:1 reduction 16 x 15 -> 8 x 5) compare with ``torch.equal``; every other
one within atol = 2e-6 * max|a|, rtol = 1e-6 (ATen's other summation order, as
test_frames_prep_vs_torch grants it, scaled by the affine).
"""
import functools

import torch

H, W = 24, 20
A = (2.4, -1.7, 0.31)
B_ = (-1.0, 0.25, 0.5)
CASES = [
    ((0, 0, 24, 20), (24, 20), False),
    ((0, 0, 24, 20), (17, 13), True),
    ((0, 0, 24, 20), (29, 31), True),
    ((0, 0, 24, 20), (299, 299), True),
    ((3, 2, 17, 13), (17, 13), False),
    ((5, 7, 7, 5), (17, 13), True),
    ((23, 19, 1, 1), (4, 6), True),     # the 1 x 1 box at the last pixel
    ((10, 4, 1, 9), (8, 8), True),      # one source row
    ((2, 11, 20, 1), (7, 5), True),     # one source column
    ((4, 3, 16, 15), (8, 5), False),    # weights 0.5 / 0.5 down, 1 / 0 across
]
IDS = ["{}x{}at{},{}-to-{}x{}".format(b[2], b[3], b[0], b[1], s[0], s[1]) for b, s, _ in CASES]

LENGTHS = (5, 1, 3, 0)
T0_STRIDE = ((0, 1), (1, 2), (4, 1), (0, 3))


def clip_u8(seed, shape=(1, 5, H, W, 3)):
    """Seeded uint8 frames that hold every byte value (so x / 255 is exercised on all 256)."""
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
    u8.view(-1)[:256] = torch.arange(256, dtype=torch.uint8)[torch.randperm(256, generator=g)]
    return u8


def batch_table(box, size, flip, h=H, w=W, rot=0):
    """A 4-clip table around one case: clip 0 gets the case's box and flip and the affine of
    test 1; the others a shifted / shrunk box, the opposite or same flip, their own affine,
    erase rectangle (none, hanging over the right and bottom edges, interior, full frame)
    and t0 / stride pair (the pairs of the frame-sampling test, rotated by ``rot``)."""
    from xcp.augment import AugmentParams
    y0, x0, bh, bw = box
    OH, OW = size
    boxes = [box,
             (max(y0 - 1, 0), min(x0 + 1, w - bw), bh, bw) if (y0 > 0 or x0 + bw < w) else (1, 0, h - 1, w),
             (0, 0, h, w) if box != (0, 0, h, w) else (2, 3, h - 5, w - 4),
             (h - max(bh // 2, 1), w - max(bw // 2, 1), max(bh // 2, 1), max(bw // 2, 1))]
    ys, xs, bhs, bws = zip(*boxes)
    er = [(0, 0, 0, 0), (OH - 2, OW - 3, 5, 7), (OH // 3, OW // 4, max(OH // 3, 1), max(OW // 2, 1)), (0, 0, OH, OW)]
    ey0, ex0, eh, ew = zip(*er)
    ts = [T0_STRIDE[(i + rot) % 4] for i in range(4)]
    return AugmentParams(t0=[p[0] for p in ts], tstride=[p[1] for p in ts], y0=ys, x0=xs, bh=bhs, bw=bws,
                         flip=[flip, 1 - flip, flip, 1 - flip], ey0=ey0, ex0=ex0, eh=eh, ew=ew,
                         a=[A, (1.0, 1.0, 1.0), (-0.75, 3.0, 1.5), (2.0, 2.0, 2.0)],
                         b=[B_, (0.0, 0.0, 0.0), (0.1, -0.2, 0.3), (-1.0, -1.0, -1.0)],
                         fill=[(0.0, 0.0, 0.0), (0.5, -0.5, 0.25), (1.0, 2.0, 3.0), (-0.125, 0.0, 7.0)])


@functools.lru_cache(maxsize=None)
def batch_case(i, flip):
    """(frames uint8 [4, 5, H, W, 3], lengths, table, size, out_frames, reference clips fp32
    planar, reference lengths) of case i: computed once, shared, never modified."""
    from xcp.augment import augment_reference
    box, size, _ = CASES[i]
    u8 = clip_u8(100 + i, (4, 5, H, W, 3))
    lengths = torch.tensor(LENGTHS, dtype=torch.int32)
    table = batch_table(box, size, flip, rot=i)
    out_frames = 4 if flip else None
    ref, ref_len = augment_reference(u8, lengths, table, size, out_frames)
    return u8, lengths, table, size, out_frames, ref, ref_len
