"""CPU tests of the clip augmentation's host side (xcp/augment.py): ``augment_reference`` (the
GPU tests' oracle) against an independent torch composition, frame sampling, erase, clamping,
the ``ClipAugment`` sampler and the PinnedClipReader's per-batch tables."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import augment_cases as AC
from xcp.augment import AugmentParams, ClipAugment, augment_reference


def compose(u8, box, size, flip, a, b, erase=None, fill=(0.0, 0.0, 0.0)):
    """One clip [T, H, W, 3] uint8 -> [T, 3, OH, OW]: slice, / 255, F.interpolate, flip, affine, erase."""
    y0, x0, bh, bw = box
    x = u8[:, y0:y0 + bh, x0:x0 + bw].to(torch.float32).permute(0, 3, 1, 2) / 255.0
    if (bh, bw) != tuple(size):
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    if flip:
        x = x.flip(-1)
    x = x * torch.tensor(a).view(1, 3, 1, 1) + torch.tensor(b).view(1, 3, 1, 1)
    if erase is not None:
        ylo, yhi, xlo, xhi = erase
        x[:, :, ylo:yhi, xlo:xhi] = torch.tensor(fill).view(1, 3, 1, 1)
    return x


def one_clip(box, flip=0, a=AC.A, b=AC.B_, erase=(0, 0, 0, 0), fill=(0.0, 0.0, 0.0), t0=0, tstride=1):
    return AugmentParams(t0=[t0], tstride=[tstride], y0=[box[0]], x0=[box[1]], bh=[box[2]], bw=[box[3]], flip=[flip],
                         ey0=[erase[0]], ex0=[erase[1]], eh=[erase[2]], ew=[erase[3]], a=[a], b=[b], fill=[fill])


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("case", range(len(AC.CASES)), ids=AC.IDS)
def test_reference_vs_composition(case, flip):
    box, size, interpolated = AC.CASES[case]
    u8 = AC.clip_u8(case)
    got, n = augment_reference(u8, torch.tensor([5]), one_clip(box, flip), size)
    want = compose(u8[0], box, size, flip, AC.A, AC.B_)
    assert n.tolist() == [5] and got.shape == (1, 5, 3) + size and got.is_contiguous()
    if interpolated:
        err = (got[0] - want).abs().max().item()
        print(f"max |reference - composition| = {err:.3g}")
        torch.testing.assert_close(got[0], want, rtol=1e-6, atol=2e-6 * max(abs(v) for v in AC.A))
    else:
        assert torch.equal(got[0], want)
    # dtype and layout: the same values cast / permuted
    cl, _ = augment_reference(u8, torch.tensor([5]), one_clip(box, flip), size, None, torch.bfloat16, True)
    assert cl.dtype == torch.bfloat16 and cl.permute(0, 1, 3, 4, 2).is_contiguous()
    assert torch.equal(cl, got.to(torch.bfloat16))


def test_frame_sampling():
    """out_len = min(Tout, max(0, ceil((len - t0) / stride))); output frame t is source frame
    t0 + t * stride; padding frames are exactly zero although b != 0 and the erase rectangle
    (fill != 0) covers the frame."""
    u8 = AC.clip_u8(50, (4, 5, AC.H, AC.W, 3))
    lengths = torch.tensor(AC.LENGTHS, dtype=torch.int32)
    box, size = (0, 0, AC.H, AC.W), (AC.H, AC.W)
    for rot in range(4):
        pairs = [AC.T0_STRIDE[(i + rot) % 4] for i in range(4)]
        for tout in (None, 2):
            p = AugmentParams.identity(4, AC.H, AC.W)
            p.t0[:] = torch.tensor([q[0] for q in pairs])
            p.tstride[:] = torch.tensor([q[1] for q in pairs])
            p.b[:] = 0.5
            got, n = augment_reference(u8, lengths, p, size, tout)
            T = 5 if tout is None else tout
            want = [min(T, max(0, math.ceil((ln - t0) / ts))) for ln, (t0, ts) in zip(AC.LENGTHS, pairs)]
            assert n.tolist() == want and got.shape[1] == T
            for b, (t0, ts) in enumerate(pairs):
                for t in range(want[b]):
                    src = u8[b, t0 + t * ts].to(torch.float32).permute(2, 0, 1) / 255.0 + 0.5
                    assert torch.equal(got[b, t], src)
                assert float(got[b, want[b]:].abs().sum()) == 0.0
            p.eh[:], p.ew[:], p.fill[:] = AC.H, AC.W, 3.0
            got, n = augment_reference(u8, lengths, p, size, tout)
            for b in range(4):
                assert bool((got[b, :want[b]] == 3.0).all()) and float(got[b, want[b]:].abs().sum()) == 0.0


@pytest.mark.parametrize("flip", [0, 1])
def test_erase(flip):
    """Empty rectangle, one hanging over the right and bottom edges, one over the top-left
    corner, the full frame; in post-flip output coordinates."""
    u8 = AC.clip_u8(51)
    box, size, fill = (3, 2, 17, 13), (11, 9), (0.5, -2.0, 7.0)
    plain = augment_reference(u8, torch.tensor([5]), one_clip(box, flip), size)[0][0]
    for rect, span in [((4, 2, 0, 3), None), ((4, 2, 3, 0), None), ((8, 5, 6, 9), (8, 11, 5, 9)),
                       ((-2, -3, 4, 5), (0, 2, 0, 2)), ((0, 0, 11, 9), (0, 11, 0, 9)), ((2, 1, 3, 4), (2, 5, 1, 5))]:
        got, _ = augment_reference(u8, torch.tensor([5]), one_clip(box, flip, erase=rect, fill=fill), size)
        want = compose(u8[0], box, size, flip, AC.A, AC.B_, span, fill)
        torch.testing.assert_close(got[0], want, rtol=1e-6, atol=2e-6 * max(abs(v) for v in AC.A))
        inside = torch.zeros(size, dtype=torch.bool)
        if span is not None:
            inside[span[0]:span[1], span[2]:span[3]] = True
        for c in range(3):   # the fill inside, the un-erased value outside, exactly
            assert bool((got[0][:, c][:, inside] == fill[c]).all())
            assert torch.equal(got[0][:, c][:, ~inside], plain[:, c][:, ~inside])


def test_clamping():
    """An out-of-range table gives what its clamped form gives (the kernel clamps the same way)."""
    u8 = AC.clip_u8(52, (6, 5, AC.H, AC.W, 3))
    lengths = torch.tensor([5, 5, 3, 9, -2, 5], dtype=torch.int32)   # 9 -> Tmax, -2 -> 0
    z = [0] * 6
    bad = AugmentParams(t0=[-3, 7, 1, 0, 0, 0], tstride=[0, 1, 100, -5, 1, 2], y0=[-4, 20, 3, 0, 0, 30],
                        x0=[5, -1, 18, 0, 0, 30], bh=[30, 10, 0, 24, 24, -7], bw=[10, 25, 5, 20, 20, 9],
                        flip=[2, -1, 0, 1, 0, 0], ey0=z, ex0=z, eh=[-1, 0, 3, 0, 0, 0], ew=[4, 0, 3, 0, 0, 0],
                        a=torch.ones(6, 3), b=torch.zeros(6, 3), fill=torch.ones(6, 3))
    good = AugmentParams(t0=[0, 5, 1, 0, 0, 0], tstride=[1, 1, 5, 1, 1, 2], y0=[0, 14, 3, 0, 0, 23],
                         x0=[5, 0, 15, 0, 0, 11], bh=[24, 10, 1, 24, 24, 1], bw=[10, 20, 5, 20, 20, 9],
                         flip=[1, 1, 0, 1, 0, 0], ey0=z, ex0=z, eh=[0, 0, 3, 0, 0, 0], ew=[4, 0, 3, 0, 0, 0],
                         a=torch.ones(6, 3), b=torch.zeros(6, 3), fill=torch.ones(6, 3))
    with pytest.raises(ValueError):
        bad.validate(6, AC.H, AC.W)
    good.validate(6, AC.H, AC.W)
    got, n = augment_reference(u8, lengths, bad, (9, 7))
    want, m = augment_reference(u8, torch.tensor([5, 5, 3, 5, 0, 5]), good, (9, 7))
    assert n.tolist() == m.tolist() == [5, 0, 1, 5, 0, 3]
    assert torch.equal(got, want)


def test_params_pack_roundtrip():
    p = AC.batch_table((5, 7, 7, 5), (17, 13), 1)
    t = p.pack()
    assert t.dtype == torch.int32 and t.shape == (4, 24) and t.is_contiguous()
    assert AugmentParams.unpack(t).equal(p)
    assert t[:, 11].abs().sum() == 0 and t[:, 21:].abs().sum() == 0
    i = AugmentParams.identity(3, 24, 20)
    assert i.bh.tolist() == [24] * 3 and i.bw.tolist() == [20] * 3 and i.tstride.tolist() == [1] * 3
    assert float(i.a.sum()) == 9.0 and float(i.b.abs().sum() + i.fill.abs().sum()) == 0.0
    for k in ("t0", "y0", "x0", "flip", "ey0", "ex0", "eh", "ew"):
        assert getattr(i, k).tolist() == [0] * 3


def test_sampler():
    H, W = 40, 56
    aug = ClipAugment((32, 32), scale=(0.3, 0.9), ratio=(0.5, 2.0), flip=0.5, brightness=0.2, contrast=0.3,
                      mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.3), erase=0.5, frames=4, strides=(1, 2, 3))
    lengths = [3, 4, 7, 10, 12, 30] * 40
    p = aug.sample(lengths, H, W, np.random.default_rng(7))
    assert len(p) == len(lengths)
    assert p.equal(aug.sample(lengths, H, W, np.random.default_rng(7)))          # same seed, same table
    assert not p.equal(aug.sample(lengths, H, W, np.random.default_rng(8)))
    p.validate(len(lengths), H, W)                                                # boxes inside the frame
    # one draw per clip: no two clips share a row, and a prefix of the batch draws the same prefix
    rows = {tuple(r) for r in p.pack().tolist()}
    assert len(rows) == len(lengths)
    q = aug.sample(lengths[:5], H, W, np.random.default_rng(7))
    assert torch.equal(q.pack(), p.pack()[:5])
    bh, bw = p.bh.double(), p.bw.double()
    area, ratio = bh * bw / (H * W), bw / bh
    # rounding bh, bw to integers moves each by at most 0.5
    assert float(((bh + 0.5) * (bw + 0.5) / (H * W)).min()) >= 0.3, area
    assert float(((bh - 0.5) * (bw - 0.5) / (H * W)).max()) <= 0.9, area
    assert float(((bw + 0.5) / (bh - 0.5)).min()) >= 0.5 and float(((bw - 0.5) / (bh + 0.5)).max()) <= 2.0, ratio
    assert float(area.max() - area.min()) > 0.3 and float(ratio.max() / ratio.min()) > 2.0   # the ranges are used
    assert 0.3 < float(p.flip.float().mean()) < 0.7
    er = (p.eh > 0) & (p.ew > 0)
    assert 0.3 < float(er.float().mean()) < 0.7 and bool(((p.eh > 0) == (p.ew > 0)).all())
    assert bool((p.ey0 >= 0).all() and (p.ey0 + p.eh <= 32).all() and (p.ex0 >= 0).all() and (p.ex0 + p.ew <= 32).all())
    assert float(p.fill.abs().sum()) == 0.0
    # frames: stride from the list; the start keeps 4 real frames where the clip has them, else 0
    assert set(p.tstride.tolist()) == {1, 2, 3}
    for ln, t0, ts in zip(lengths, p.t0.tolist(), p.tstride.tolist()):
        need = 3 * ts + 1
        assert (0 <= t0 <= ln - need) if ln >= need else t0 == 0
    assert len(set(p.t0[5::6].tolist())) > 5   # length-30 clips start at many places
    # a, b: one kappa and one delta per clip, inside their ranges, shared by the three channels
    mean, std = np.array([0.4, 0.5, 0.6]), np.array([0.2, 0.25, 0.3])
    kappa = p.a.double().numpy() * std
    delta = p.b.double().numpy() * std + mean - (0.5 - 0.5 * kappa)
    assert kappa.min() >= 0.7 - 1e-6 and kappa.max() <= 1.3 + 1e-6 and np.abs(delta).max() <= 0.2 + 1e-6
    assert np.abs(kappa - kappa[:, :1]).max() <= 1e-6 and np.abs(delta - delta[:, :1]).max() <= 1e-6
    assert kappa.max() - kappa.min() > 0.4 and delta.max() - delta.min() > 0.25
    # the folding: contrast about 0.5, then brightness, then normalise, step by step in fp64
    for k, d in [(1.0, 0.0), (0.7, 0.2), (1.3, -0.2), (0.9, 0.05)]:
        a, b = aug.fold(k, d)
        assert a.dtype == np.float64 and a.shape == b.shape == (3,)
        for x in (0.0, 0.3, 1.0):
            step = (x - 0.5) * k + 0.5
            step = step + d
            step = (step - mean) / std
            np.testing.assert_allclose(a * x + b, step, rtol=0, atol=1e-6)
    # ... and the table holds fold()'s values, rounded to fp32
    one = ClipAugment((8, 8), brightness=0.0, contrast=0.0, mean=(0.4, 0.5, 0.6), std=(0.2, 0.25, 0.3))
    a, b = one.fold(1.0, 0.0)
    t = one.sample([3], H, W, np.random.default_rng(0))
    assert torch.equal(t.a[0], torch.tensor(a).float()) and torch.equal(t.b[0], torch.tensor(b).float())


def test_sampler_identity_and_eval():
    ident = ClipAugment((32, 32), scale=(1, 1), ratio=(1, 1), flip=0.0, mean=(0.0,) * 3, std=(1.0,) * 3)
    p = ident.sample([5, 1, 3], 48, 48, np.random.default_rng(0))   # ratio is absolute: a square frame
    assert p.equal(AugmentParams.identity(3, 48, 48))
    ev = ClipAugment.eval((299, 299))
    a, b = ev.sample([4, 9], 333, 301), ev.sample([4, 9], 333, 301, np.random.default_rng(5))
    assert a.equal(b)                                               # nothing random
    assert a.bh.tolist() == [299, 299] and a.bw.tolist() == [round(301 * 299 / 333)] * 2
    assert a.y0.tolist() == [17, 17] and a.x0.tolist() == [(301 - 270) // 2] * 2   # centred
    assert a.flip.tolist() == [0, 0] and a.eh.tolist() == [0, 0] and a.t0.tolist() == [0, 0]
    assert a.tstride.tolist() == [1, 1]
    assert torch.equal(a.a, torch.full((2, 3), 2.0)) and torch.equal(a.b, torch.full((2, 3), -1.0))
    with pytest.raises(ValueError):
        ClipAugment((32, 32)).sample([3], 48, 48)
    with pytest.raises(ValueError):
        ClipAugment((32, 32), scale=(0.0, 1.0))


def test_pinned_reader_tables(tmp_path):
    """PinnedClipReader(augment=...): the table of batch i in epoch e is a function of (seed, e,
    i) and the batch alone -- two readers visiting the batches in different orders agree; other
    seeds, epochs and batches draw other tables."""
    from Dataset.video_dataloader import PinnedClipReader
    rs = np.random.RandomState(4)
    for i, t in enumerate((4, 7, 2, 5, 3)):
        np.save(tmp_path / f"{'real' if i % 2 else 'fake'}_{i}.npy", rs.randint(0, 256, (t, 12, 16, 3), dtype=np.uint8))
    aug = ClipAugment((8, 8), flip=0.5, contrast=0.2, erase=0.5, frames=2, strides=(1, 2))

    def tables(reader, epoch, order):
        out = {}
        for i in order:
            _, frames, _, ln = PinnedClipReader.read_batch(reader.batches()[i])
            out[i] = reader.augment_table(epoch, i, ln, frames.shape[2], frames.shape[3])
        return out

    r1 = PinnedClipReader(str(tmp_path), 2, "cpu", augment=aug, seed=3)
    r2 = PinnedClipReader(str(tmp_path), 2, "cpu", augment=aug, seed=3)
    a, b = tables(r1, 1, [0, 1, 2]), tables(r2, 1, [2, 0, 1])
    for i in range(3):
        assert a[i].equal(b[i]) and len(a[i]) == len(r1.batches()[i])
        a[i].validate(len(a[i]), 12, 16)
    assert not a[0].equal(a[1])
    assert not a[0].equal(tables(r1, 2, [0])[0])
    assert not a[0].equal(tables(PinnedClipReader(str(tmp_path), 2, "cpu", augment=aug, seed=4), 1, [0])[0])
    with pytest.raises(ValueError):
        PinnedClipReader(str(tmp_path), 2, "cpu", size=(9, 9), augment=aug)
