"""``xcp.degrade`` on the CPU: the integer restatement ``degrade_reference`` against what its
arithmetic implies (flat frames, padding frames, the identity table), against libjpeg through PIL,
the noise law's moments, and the sampler."""
import io

import numpy as np
import pytest
import torch

import degrade_cases as DC
from xcp.degrade import (DCT_C, ClipDegrade, DegradeParams, degrade_reference, gaussian_taps, noise_amplitude,
                         philox4x32_10)


def test_dct_matrix_is_the_rounded_cosine_table():
    u, x = np.arange(8).reshape(8, 1), np.arange(8).reshape(1, 8)
    s = np.where(u == 0, 1 / (2 * np.sqrt(2)), 0.5)
    assert np.array_equal(DCT_C, np.rint(4096 * s * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64))


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    z, f = np.zeros(1, np.uint32), np.full(1, 0xffffffff, np.uint32)
    assert [int(w[0]) for w in philox4x32_10((z, z, z, z), (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert [int(w[0]) for w in philox4x32_10((f, f, f, f), (0xffffffff, 0xffffffff))] == \
        [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    pi = [np.full(1, v, np.uint32) for v in (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344)]
    assert [int(w[0]) for w in philox4x32_10(pi, (0xa4093822, 0x299f31d0))] == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


@pytest.mark.parametrize("q", [1, 50, 100])
def test_flat_grey_survives_jpeg(q):
    u8 = torch.full((1, 2, 19, 21, 3), 128, dtype=torch.uint8)
    out = degrade_reference(u8, [2], DegradeParams.fixed(1, quality=q))
    assert torch.equal(out, u8)


def test_lengths_identity_and_padding():
    u8 = DC.frames_u8(1, (3, 3, 17, 19, 3))
    out = degrade_reference(u8, DC.LENGTHS, DegradeParams.identity(3))
    assert torch.equal(out[0], u8[0]) and torch.equal(out[1, :1], u8[1, :1])
    assert not out[1, 1:].any() and not out[2].any()
    for stage in DC.STAGES:
        out = degrade_reference(u8, DC.LENGTHS, DC.table(stage, 0))
        assert out.dtype == torch.uint8 and out.shape == u8.shape
        assert not out[1, 1:].any() and not out[2].any()
        assert not torch.equal(out[0], u8[0])
    # lengths outside [0, Tmax] are clamped
    assert torch.equal(degrade_reference(u8, (9, -2, 3), DegradeParams.identity(3))[1], torch.zeros_like(u8[1]))


@pytest.mark.parametrize("sigma", [0.3, 1.0, 2.3])
def test_taps_and_flat_blur(sigma):
    R, w = gaussian_taps(sigma)
    assert R == min(7, int(np.ceil(3 * sigma))) and len(w) == 8
    assert all(v >= 0 for v in w) and all(v == 0 for v in w[R + 1:])
    assert w[0] + 2 * sum(w[1:]) == 2048 and all(w[k] >= w[k + 1] for k in range(7))
    for value in (0, 77, 255):
        u8 = torch.full((1, 1, 5, 9, 3), value, dtype=torch.uint8)
        assert torch.equal(degrade_reference(u8, [1], DegradeParams.fixed(1, sigma=sigma)), u8)


def test_psnr_rises_with_quality():
    u8 = DC.frames_u8(7, (1, 1, 64, 80, 3))
    got = [DC.psnr(degrade_reference(u8, [1], DegradeParams.fixed(1, quality=q)), u8) for q in (10, 30, 50, 75, 90, 100)]
    print("PSNR over q:", [round(v, 2) for v in got])
    assert all(b >= a for a, b in zip(got, got[1:]))


@pytest.mark.parametrize("size", [(16, 33), (24, 40), (37, 53), (64, 80)])
@pytest.mark.parametrize("q", [20, 75, 95])
def test_against_libjpeg(size, q):
    Image = pytest.importorskip("PIL.Image")
    u8 = DC.frames_u8(11 + size[0], (1, 1, *size, 3))
    src = u8[0, 0].numpy()
    buf = io.BytesIO()
    Image.fromarray(src).save(buf, format="JPEG", quality=q, subsampling=2)
    pil = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))
    ours = degrade_reference(u8, [1], DegradeParams.fixed(1, quality=q))[0, 0].numpy()
    gap = abs(DC.psnr(ours, src) - DC.psnr(pil, src))
    mad = float(np.abs(ours.astype(np.int64) - pil.astype(np.int64)).mean())
    print(f"{size[0]}x{size[1]} q={q}: PSNR ours {DC.psnr(ours, src):.2f} PIL {DC.psnr(pil, src):.2f} gap {gap:.3f} dB, "
          f"mean |byte diff| {mad:.2f}")
    assert gap <= 0.75


def test_noise_law():
    assert noise_amplitude(8.0) == 78
    grey = torch.full((1, 4, 64, 64, 3), 128, dtype=torch.uint8)
    a = degrade_reference(grey, [4], DegradeParams.fixed(1, noise=8.0, seed=5))
    n = a.numpy().astype(np.float64) - 128.0
    assert (78 * 524280 + (1 << 19)) >> 20 == 39 and 20 <= np.abs(n).max() <= 39   # the largest |n|: nothing clamps
    N = n.size
    sd = np.sqrt((78 * 107019.7 / 2 ** 20) ** 2 + 1 / 12)
    assert abs(n.mean()) <= 4 * sd / np.sqrt(N)
    # standard error of a sample standard deviation: sd sqrt((kurtosis - 1) / 4N); a sum of 8 uniforms has 3 - 1.2 / 8
    print(f"noise: mean {n.mean():+.4f} (se {sd / np.sqrt(N):.4f}), sd {n.std():.4f} against {sd:.4f} "
          f"(se {sd * np.sqrt(1.85 / (4 * N)):.4f})")
    assert abs(n.std() - sd) <= 4 * sd * np.sqrt(1.85 / (4 * N))
    b = degrade_reference(grey, [4], DegradeParams.fixed(1, noise=8.0, seed=6))
    assert not torch.equal(a, b)
    assert not torch.equal(a[0, 0], a[0, 1])
    assert not torch.equal(a[0, 0, :, :, 0], a[0, 0, :, :, 1])
    assert torch.equal(a, degrade_reference(grey, [4], DegradeParams.fixed(1, noise=8.0, seed=5)))
    # a 64-bit seed reaches both key words; clip b of fixed() draws with seed + b
    two = DegradeParams.fixed(2, noise=8.0, seed=(3 << 32) + 5)
    assert two.seed_lo.tolist() == [5, 6] and two.seed_hi.tolist() == [3, 3]


def test_sampler_and_pack():
    deg = ClipDegrade()
    a, b = deg.sample(64, np.random.default_rng(3)), deg.sample(64, np.random.default_rng(3))
    c = deg.sample(64, np.random.default_rng(4))
    assert a.equal(b) and not a.equal(c)
    a.validate(64)
    on = (a.quality > 0)
    assert 10 < int(on.sum()) < 54 and int(a.quality[on].min()) >= 30 and int(a.quality.max()) <= 95
    assert 4 < int((a.radius > 0).sum()) < 40 and 4 < int((a.namp > 0).sum()) < 40
    assert len(set(zip(a.seed_lo.tolist(), a.seed_hi.tolist()))) == 64
    packed = a.pack()
    assert packed.dtype == torch.int32 and tuple(packed.shape) == (64, 16) and not packed[:, 13:].any()
    assert DegradeParams.unpack(packed).equal(a)
    assert torch.equal(a.pack(torch.empty((64, 16), dtype=torch.int32)), packed)
    with pytest.raises(ValueError):
        a.pack(torch.empty((64, 24), dtype=torch.int32))
    always = ClipDegrade(jpeg=(40, 40), jpeg_p=1.0, blur=(1.0, 1.0), blur_p=1.0, noise=(8.0, 8.0), noise_p=1.0)
    s = always.sample(2, np.random.default_rng(0))
    assert s.quality.tolist() == [40, 40] and s.radius.tolist() == [3, 3] and s.namp.tolist() == [78, 78]
    assert s.taps[0].tolist() == gaussian_taps(1.0)[1]


def test_validation():
    with pytest.raises(ValueError):
        DegradeParams.fixed(1, noise=64.5)
    with pytest.raises(ValueError):
        DegradeParams.fixed(1, quality=101)
    with pytest.raises(ValueError):
        ClipDegrade(noise=(1.0, 65.0))
    p = DegradeParams.fixed(2, quality=50, sigma=1.0, noise=4.0)
    p.validate(2)
    with pytest.raises(ValueError):
        p.validate(3)
    for field, value in (("quality", 250), ("radius", 99), ("namp", 10 ** 6)):
        bad = DegradeParams.fixed(2, quality=50, sigma=1.0, noise=4.0)
        getattr(bad, field)[1] = value
        with pytest.raises(ValueError):
            bad.validate(2)
    bad = DegradeParams.fixed(2, sigma=1.0)
    bad.taps[0, 0] += 1
    with pytest.raises(ValueError):
        bad.validate(2)
