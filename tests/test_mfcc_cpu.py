"""CPU tests of the MFCC front end's arithmetic contract (xcp/audio.py): the tables against their
definitions, the fp64 restatement and its element-wise bound against an fp32 emulation and against
mutants that the bound must catch, the sampler, the waveform loader and the wrapper's validation.

librosa is not installed here, so nothing below compares with it: the anchors are scipy's Hann
window and DCT and the closed-form properties of the Slaney mel scale."""
import math

import numpy as np
import pytest
import torch

import mfcc_cases as MC
from xcp import audio as A


@pytest.fixture(scope="module")
def plan():
    return A.MfccPlan()


@pytest.fixture(scope="module")
def stepped(plan):
    """The noise case, its table, and the reference (computed once)."""
    wav, lengths = MC.batch([MC.stepped_noise()])
    table = A.WaveParams.identity(1, MC.STEPPED["f0"])
    ref, lim, out_len = A.mfcc_reference(wav, lengths, plan, table, MC.STEPPED["frames"], 1)
    assert out_len.tolist() == [60]
    return wav, lengths, table, ref, lim


# ------------------------------------------------------------------ tables
def test_hann_and_dct_equal_scipy():
    sig = pytest.importorskip("scipy.signal")
    fft = pytest.importorskip("scipy.fft")
    # two fp64 evaluations of the same formula: the arguments (up to 2 pi, and up to 12 pi for the DCT's rows
    # of amplitude 1 / 8) carry roundings of up to ulp(2 pi) = 2^-50 and ulp(12 pi) / 8 = 2^-50; allow 2^-49
    assert np.abs(A.hann_window(400) - sig.get_window("hann", 400, fftbins=True)).max() <= 2.0 ** -49
    assert np.abs(A.dct_rows(13, 128) - fft.dct(np.eye(128), type=2, norm="ortho", axis=0)[:13]).max() <= 2.0 ** -49


def test_mel_scale_anchors():
    assert A.hz_to_mel(1000.0) == 15
    for hz in (0.0, 500.0, 1000.0, 4000.0, 8000.0):
        assert abs(A.mel_to_hz(A.hz_to_mel(hz)) - hz) <= 1e-12 * max(hz, 1.0)
    assert abs(A.hz_to_mel(6400.0) - 42.0) <= 1e-12      # 27 log steps take 1 kHz to 6.4 kHz


def test_triangles_partition_unity_and_none_is_empty(plan):
    cfg = plan.cfg
    tri = A.mel_filterbank(cfg, normalised=False)
    f = A.mel_points(cfg)
    freqs = np.arange(cfg.n_bins) * cfg.sr / cfg.n_fft
    inside = (freqs >= f[1]) & (freqs <= f[-2])
    assert inside.sum() > 150
    assert np.abs(tri[:, inside].sum(0) - 1.0).max() <= 1e-12
    assert plan.empty_filters() == []
    assert plan.mel_fc[:, 1].max() <= 9                               # what the packed device form relies on
    assert (plan.mel[:, -1] == 0).all()                               # the Nyquist bin is the last corner: weight 0
    dense = np.zeros_like(plan.mel)
    for j, (first, count) in enumerate(plan.mel_fc):
        dense[j, first:first + count] = plan.mel_w[j, :count]
    assert np.array_equal(dense, plan.mel)
    assert np.array_equal(plan.tw[:, 0], np.cos(2 * np.pi * np.arange(400) / 400).astype(np.float32))


def test_config_range():
    for bad in (dict(n_fft=401), dict(n_fft=14), dict(n_fft=1026), dict(hop=0), dict(n_mels=129), dict(n_mfcc=14, n_mels=13),
                dict(fmax=9000.0), dict(amin=0.0), dict(top_db=-1.0)):
        with pytest.raises(ValueError):
            A.MfccConfig(**bad)
    A.MfccConfig(n_fft=16, hop=1)
    A.MfccConfig(n_fft=1024, top_db=None)


# ------------------------------------------------------------------ the restatement
def test_zero_clip(plan):
    wav, lengths = MC.batch([np.zeros(800, np.float32)])
    ref, lim, out_len = A.mfcc_reference(wav, lengths, plan, None, None, 1)
    assert out_len.tolist() == [6] and ref.shape == (1, 6, 13)
    # -100 sqrt(128), with amin and the DCT's first row as fp32 holds them
    c0 = 10.0 * math.log10(float(np.float32(1e-10))) * float(np.float32(math.sqrt(1 / 128))) * 128
    assert abs(c0 + 100 * math.sqrt(128)) < 1e-4
    assert torch.allclose(ref[0, :, 0], torch.full((6,), c0, dtype=torch.float64), rtol=1e-14, atol=0)
    # rows 1.. of the DCT sum to zero before they are rounded to fp32: |100 sum_j D32[i, j]| <= 100 * 128 * 2^-25 / 8
    assert ref[0, :, 1:].abs().max() <= 100 * 128 * 2.0 ** -25 / 8
    assert (lim > 0).all()


@pytest.mark.parametrize("n, frames", [(0, 0), (1, 1), (159, 1), (160, 2), (161, 2)])
def test_frame_counts(plan, n, frames):
    wav, _ = MC.batch([MC.noise(1, 400)])
    lengths = torch.tensor([n], dtype=torch.int32)
    ref, lim, out_len = A.mfcc_reference(wav, lengths, plan, None, 4, 3)
    assert ref.shape == (1, 4, 3, 13) and out_len.tolist() == [frames]
    assert not ref[0, frames:].any() and not lim[0, frames:].any()
    if frames:
        assert ref[0, :frames].abs().sum() > 0


def test_shift_and_f0_past_the_end(plan):
    wav, lengths = MC.batch([MC.noise(2, 400)] * 5)
    # 400 samples: 3 frames; shift 81 leaves 319: 2 frames; shift 400 leaves none; f0 2 leaves one; f0 3 none
    table = A.WaveParams([0, 81, 400, 0, 0], [0, 0, 0, 2, 3], [1, 1, 1, 1, 1])
    ref, _, out_len = A.mfcc_reference(wav, lengths, plan, table, 2, 1)
    assert out_len.tolist() == [2, 2, 0, 1, 0]
    lengths[0] = 1000            # a length beyond the buffer is clamped to Nmax
    assert A.mfcc_reference(wav, lengths, plan, table, 5, 1)[2].tolist() == [3, 2, 0, 1, 0]
    assert not ref[2].any() and not ref[4].any() and not ref[3, 1].any() and ref[3, 0].any()


def test_floor_uses_the_clip_wide_maximum(plan):
    """A loud frame outside the emitted window changes the emitted rows."""
    quiet = MC.noise(5, 1600, 1e-5)
    loud = quiet.copy()
    loud[:160] = MC.noise(6, 160, 0.5)
    (wav, lengths), table = MC.batch([quiet, loud]), A.WaveParams.identity(2, 5)
    ref, lim, out_len = A.mfcc_reference(wav, lengths, plan, table, 4, 1)     # frames 5..8: samples 600 and later only
    assert out_len.tolist() == [4, 4]
    assert (ref[0] - ref[1]).abs().max() > 100 * lim.max()
    nofloor = A.MfccPlan(A.MfccConfig(top_db=None))
    ref, lim, _ = A.mfcc_reference(wav, lengths, nofloor, table, 4, 1)
    assert torch.equal(ref[0], ref[1])


CASES = {
    "noise": lambda: MC.batch([MC.noise(7, 4000)]),
    "tone+weak noise": lambda: MC.batch([MC.tone_plus_weak_noise()]),
    "chirp": lambda: MC.batch([MC.chirp()]),
    "zeros": lambda: MC.batch([np.zeros(1000, np.float32)]),
    "int16": lambda: MC.batch([MC.to_i16(MC.noise(8, 3000)), MC.to_i16(MC.chirp(1500))], np.int16),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_emulation_within_lim(plan, case):
    wav, lengths = CASES[case]()
    table = A.WaveParams([0, 37][:len(lengths)], [0, 1][:len(lengths)], [1.0, 0.7][:len(lengths)])
    ref, lim, out_len = A.mfcc_reference(wav, lengths, plan, table, None, 3)
    got = MC.emulate_f32(wav, lengths, plan, table, None, 3)
    MC.assert_within_lim(got, ref, lim, case)
    MC.assert_zero_rows(got, out_len)


def test_fp32_emulation_within_lim_stepped(plan, stepped):
    wav, lengths, table, ref, lim = stepped
    MC.assert_within_lim(MC.emulate_f32(wav, lengths, plan, table, 60, 1), ref, lim, "stepped noise")


# ------------------------------------------------------------------ sensitivity (a condition on the test data)
def test_mutants_land_outside_lim(plan, stepped):
    """Each defect moves the result of the noise case (mfcc_cases.stepped_noise) outside lim.  The issue's
    "Nyquist bin dropped" cannot be seen in any MFCC at fmax = sr / 2: the Nyquist bin is the filterbank's
    last corner and carries weight 0 in every filter (asserted above), so a kernel that leaves it out
    computes the same numbers; the mutant here leaves out the highest bin that does carry weight."""
    wav, lengths, table, ref, lim = stepped
    top = plan.cfg.n_bins - 2
    assert plan.mel[:, top].max() > 0

    def outside(got):
        return MC.ratio(got, ref, lim)

    args = (lengths, plan, table, 60, 1)
    zeroed = wav.clone()
    zeroed[0, 8000] = 0                                # (in the emitted, unfloored part)
    assert wav[0, 8000] != 0
    mutants = {
        "one sample zeroed": MC.emulate_f32(zeroed, *args),
        "top weighted bin dropped": MC.emulate_f32(wav, *args, drop_bin=top),
        "one mel weight dropped": MC.emulate_f32(wav, *args, drop_weight=(100, int(plan.mel_fc[100, 0]) + 2)),
        "hop off by one": MC.emulate_f32(wav, *args, hop=161),
        "Lmax over the emitted frames": MC.emulate_f32(wav, *args, lmax_emitted_only=True),
    }
    for name, got in mutants.items():
        r = outside(got)
        print(f"{name}: {r:.1f} x lim")
        assert r > 1.0, name


# ------------------------------------------------------------------ sampler, loader, validation
def test_wave_augment_draws():
    cfg = A.MfccConfig()
    aug = A.WaveAugment(cfg, 20, max_shift=159, gain_db=(-6.0, 6.0), split_offset=2)
    lengths = [16000, 3000, 100, 0]
    a = aug.sample(lengths, np.random.default_rng(1))
    b = aug.sample(lengths, np.random.default_rng(1))
    c = aug.sample(lengths, np.random.default_rng(2))
    assert a.equal(b) and not a.equal(c)
    a.validate(4, 16000)
    assert ((a.shift >= 0) & (a.shift <= 159)).all() and a.shift[3] == 0
    assert ((a.gain >= 10 ** -0.3 - 1e-6) & (a.gain <= 10 ** 0.3 + 1e-6)).all()
    for ln, s, f0 in zip(lengths, a.shift.tolist(), a.f0.tolist()):
        fall = cfg.frames(ln - s)
        assert f0 >= 2 and (f0 + 20 <= fall or f0 == 2)
    with pytest.raises(ValueError):
        aug.sample(lengths)
    ev = A.WaveAugment.eval(cfg, 24, 120)
    e = ev.sample(lengths, np.random.default_rng(5))
    assert e.equal(ev.sample(lengths)) and e.f0.tolist() == [120] * 4 and not e.shift.any() and (e.gain == 1).all()
    with pytest.raises(ValueError):
        A.WaveAugment(cfg, 0)


def test_pack_round_trip():
    t = A.WaveParams([0, 5, 159], [0, 120, 144], [1.0, 0.5, 1.9952623])
    p = t.pack()
    assert p.dtype == torch.int32 and p.shape == (3, A.WAVE_COLS) and p[1].tolist()[:2] == [5, 120]
    assert p[0, 2].item() == 0x3F800000 and not p[:, 3].any()
    assert A.WaveParams.unpack(p).equal(t)
    buf = torch.full((3, A.WAVE_COLS), -1, dtype=torch.int32)
    assert t.pack(buf) is buf and torch.equal(buf, p)
    for bad in (A.WaveParams([-1], [0], [1.0]), A.WaveParams([11], [0], [1.0]), A.WaveParams([0], [-1], [1.0]),
                A.WaveParams([0], [0], [float("inf")])):
        with pytest.raises(ValueError):
            bad.validate(1, 10)
    with pytest.raises(ValueError):
        t.validate(2, 1000)


def test_wave_dataset_and_collate(tmp_path):
    from Dataset.audio_dataloader import WaveDataset, collate_wave, get_wave_dataloader
    rs = np.random.RandomState(0)
    clips = {"fake_b.npy": rs.randint(-3000, 3000, 7).astype(np.int16), "real_a.npy": rs.randint(-3000, 3000, 4).astype(np.int16),
             "Real_c.npy": rs.randint(-3000, 3000, 9).astype(np.int16)}
    for k, v in clips.items():
        np.save(tmp_path / k, v)
    ds = WaveDataset(str(tmp_path))
    assert [p.split("/")[-1] for p in ds.npy_files] == sorted(clips)
    wav, lengths, labels = collate_wave([ds[i] for i in range(3)])
    assert wav.dtype == torch.int16 and wav.shape == (3, 9) and lengths.tolist() == [9, 7, 4] and lengths.dtype == torch.int32
    assert labels.tolist() == [[0.0], [1.0], [0.0]]
    assert np.array_equal(wav[1, :7].numpy(), clips["fake_b.npy"]) and not wav[1, 7:].any() and not wav[2, 4:].any()
    batches = list(get_wave_dataloader(str(tmp_path), batch_size=2))
    assert [b[0].shape for b in batches] == [(2, 9), (1, 4)]
    np.save(tmp_path / "real_d.npy", (clips["real_a.npy"] / 32768.0).astype(np.float32))     # a mixed batch becomes fp32
    ds = WaveDataset(str(tmp_path))
    wav, lengths, _ = collate_wave([ds[2], ds[3]])
    assert wav.dtype == torch.float32 and torch.equal(wav[0, :4], wav[1, :4]) and lengths.tolist() == [4, 4]


def test_ops_mfcc_meta_and_validation(plan):
    from xcp import ops, torch_ops
    assert "mfcc" in torch_ops.OPS and hasattr(torch.ops.xcp, "mfcc")

    def meta(*shape, dt=torch.float32):
        return torch.empty(shape, device="meta", dtype=dt)

    wav, lengths = meta(4, 1000), meta(4, dt=torch.int32)
    out, n = ops.mfcc(wav, lengths, plan)
    assert out.shape == (4, 7, 3, 13) and out.dtype == torch.float32 and n.shape == (4,) and n.dtype == torch.int32
    out, _ = ops.mfcc(meta(4, 1000, dt=torch.int16), lengths, plan, A.WaveParams.identity(4, 2), 5, 1, torch.bfloat16)
    assert out.shape == (4, 5, 13) and out.dtype == torch.bfloat16
    out, _ = ops.mfcc(wav, lengths, plan, meta(4, A.WAVE_COLS, dt=torch.int32), 120)
    assert out.shape == (4, 120, 3, 13)
    bad_calls = [
        lambda: ops.mfcc(meta(4, 1000, dt=torch.float64), lengths, plan),
        lambda: ops.mfcc(meta(4, 1000, 1), lengths, plan),
        lambda: ops.mfcc(meta(1000, 4).t(), lengths, plan),                                  # not contiguous
        lambda: ops.mfcc(wav, meta(4, dt=torch.int64), plan),
        lambda: ops.mfcc(wav, meta(3, dt=torch.int32), plan),
        lambda: ops.mfcc(wav, lengths, plan.cfg),
        lambda: ops.mfcc(wav, lengths, plan, A.WaveParams.identity(3)),                      # table rows
        lambda: ops.mfcc(wav, lengths, plan, A.WaveParams([0, 0, 0, 1001], [0] * 4, [1.0] * 4)),
        lambda: ops.mfcc(wav, lengths, plan, A.WaveParams([0, 0, 0, -1], [0] * 4, [1.0] * 4)),
        lambda: ops.mfcc(wav, lengths, plan, A.WaveParams([0] * 4, [0, -1, 0, 0], [1.0] * 4)),
        lambda: ops.mfcc(wav, lengths, plan, A.WaveParams([0] * 4, [0] * 4, [1.0, float("nan"), 1.0, 1.0])),
        lambda: ops.mfcc(wav, lengths, plan, meta(4, 3, dt=torch.int32)),
        lambda: ops.mfcc(wav, lengths, plan, None, 0),
        lambda: ops.mfcc(wav, lengths, plan, None, None, 0),
        lambda: ops.mfcc(wav, lengths, plan, None, None, 3, torch.float16),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} did not raise")
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.mfcc(torch.zeros(1, 100), torch.tensor([100], dtype=torch.int32), plan)
