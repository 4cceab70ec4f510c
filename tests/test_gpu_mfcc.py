"""GPU tests of the MFCC front end (csrc/mfcc.hip through ``ops.mfcc``): every comparison is
|got - ref64| <= lim element by element (xcp.audio.mfcc_reference: fp64 on the kernel's fp32 inputs, an
interval bound with no fitted constant, nothing excluded), bf16 outputs by elementwise.py's neighbour rule
with e = lim, plus bit-exact out_len, bit-exact zero rows and bit-identical channel copies."""
import numpy as np
import pytest
import torch

import mfcc_cases as MC
from xcp import audio as A

pytestmark = pytest.mark.gpu

RUN = 8   # frames one workgroup of xcp_mfcc_logmel walks at the configs below (asserted in the tests that rely on it)


def check(gpu, wav, lengths, plan, table, out_frames, tag, channels=(1, 3), dtypes=(torch.float32, torch.bfloat16)):
    """ops.mfcc on (wav, lengths, table) against the reference, over output dtypes and channel counts.
    Returns the worst d / lim of the fp32 outputs."""
    from xcp import ops
    ref, lim, ref_len = A.mfcc_reference(wav, lengths, plan, table, out_frames, 1)
    w, ln = wav.to(gpu), lengths.to(gpu)
    tab = None if table is None else table.to(gpu)
    worst = 0.0
    for dtype in dtypes:
        one = None
        for ch in channels:
            out, n = ops.mfcc(w, ln, plan, tab, out_frames, ch, dtype)
            torch.cuda.synchronize()
            out, n = out.cpu(), n.cpu()
            assert out.dtype == dtype and n.dtype == torch.int32 and torch.equal(n, ref_len), (n, ref_len)
            assert out.shape == (ref.shape if ch == 1 else (ref.shape[0], ref.shape[1], ch, ref.shape[2]))
            MC.assert_zero_rows(out, ref_len)
            first = out if ch == 1 else out[:, :, 0]
            for c in range(1, ch):
                assert torch.equal(out[:, :, c].view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                                   first.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)), "channel copies differ"
            if dtype == torch.float32:
                worst = max(worst, MC.assert_within_lim(first, ref, lim, f"{tag} fp32 C{ch}"))
            else:
                MC.assert_bf16_within_lim(first.contiguous(), ref, lim, f"{tag} bf16 C{ch}")
            if one is None:
                one = first.clone()
            else:
                assert torch.equal(one, first), "channels = 1 and channels = 3 differ"
    return worst


EDGE_LENGTHS = (1, 159, 160, 1000, 0)   # 1, 1, 2, 7 and 0 frames: centre padding, frame counts, the right edge


def edge_batch(in_dtype):
    x = MC.noise(11, 5 * 1000).reshape(5, 1000)
    wav = torch.from_numpy(MC.to_i16(x) if in_dtype == torch.int16 else x)
    return wav, torch.tensor(EDGE_LENGTHS, dtype=torch.int32)


@pytest.mark.parametrize("top_db", [80.0, None])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_default_config_edges(gpu, in_dtype, top_db):
    plan = A.MfccPlan(A.MfccConfig(top_db=top_db))
    wav, lengths = edge_batch(in_dtype)
    ref_len = A.mfcc_reference(wav, lengths, plan, None, None, 1)[2]
    assert ref_len.tolist() == [1, 1, 2, 7, 0]
    check(gpu, wav, lengths, plan, None, None, f"edges {in_dtype} top_db {top_db}")


@pytest.mark.parametrize("out_frames", [3, 9])
@pytest.mark.parametrize("in_dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
def test_default_config_per_clip_table(gpu, in_dtype, out_frames):
    """Every clip its own shift, f0 and gain; clip 0 has f0 >= Fall; clip 3 has Fall - f0 = 5 frames, more than
    Tout = 3 and fewer than Tout = 9."""
    plan = A.MfccPlan()
    wav, lengths = edge_batch(in_dtype)
    table = A.WaveParams([0, 10, 0, 37, 5], [1, 0, 1, 2, 0], [1.0, 0.5, 2.0, 0.7, 1.3])
    ref_len = A.mfcc_reference(wav, lengths, plan, table, out_frames, 1)[2]
    assert ref_len.tolist() == [0, 1, 1, min(out_frames, 5), 0]
    check(gpu, wav, lengths, plan, table, out_frames, f"table {in_dtype} Tout {out_frames}")


def test_more_frames_than_one_workgroup_walks(gpu):
    """17 = 2 * RUN + 1 frames: the third workgroup of clip 0 holds a single frame.  Clip 1 (13 frames) is clip 0
    with everything after its first hop 80 dB quieter, so most of its bands sit on a floor: Lmax - 80 from
    the loud start, and amin."""
    from xcp import _lib
    plan = A.MfccPlan()
    assert _lib.call("xcp_mfcc_run_frames", 400, 160) == RUN
    a = MC.noise(12, 2560, 0.03)
    b = a[:2000].copy()
    b[160:] *= 1e-4
    wav, lengths = MC.batch([a, b])
    ref_len = A.mfcc_reference(wav, lengths, plan, None, None, 1)[2]
    assert ref_len.tolist() == [2 * RUN + 1, 13]
    check(gpu, wav, lengths, plan, None, None, "17 frames")
    check(gpu, wav, lengths, plan, A.WaveParams([3, 0], [7, 9], [1.0, 1.0]), 12, "17 frames, f0 across workgroups",
          channels=(3,), dtypes=(torch.float32,))


def test_second_config(gpu):
    from xcp import _lib
    plan = A.MfccPlan(A.MfccConfig(n_fft=512, hop=128, n_mels=40, n_mfcc=20, fmin=20.0, fmax=7600.0))
    assert _lib.call("xcp_mfcc_run_frames", 512, 128) == RUN
    wav, lengths = MC.batch([MC.noise(13, 700), MC.chirp(1200)])
    assert A.mfcc_reference(wav, lengths, plan, None, None, 1)[2].tolist() == [6, 10]
    check(gpu, wav, lengths, plan, None, None, "512/128/40/20")
    check(gpu, torch.from_numpy(MC.to_i16(wav.numpy())), lengths, plan, A.WaveParams([5, 100], [1, 0], [0.9, 1.1]), 4,
          "512/128/40/20 i16", channels=(3,))


def test_smallest_config(gpu):
    plan = A.MfccPlan(A.MfccConfig(n_fft=16, hop=1))
    wav, lengths = MC.batch([MC.noise(14, 40)])
    assert A.mfcc_reference(wav, lengths, plan, None, None, 1)[2].tolist() == [41]
    check(gpu, wav, lengths, plan, None, None, "16/1")


@pytest.mark.parametrize("in_dtype", [torch.float32, torch.int16], ids=["f32", "i16"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 2), (2, 1), (3, 1), (1, 3), (1, 401), (13, 43)], ids=str)
def test_buffer_end(gpu, shape, in_dtype):
    """The waveform tensor is the whole allocation (B Nmax = 1, 2, 3, 401, 559 samples): the staged span of the
    last frames of the last clip ends where the buffer ends."""
    B, Nmax = shape
    x = MC.noise(15, B * Nmax).reshape(B, Nmax)
    wav = torch.from_numpy(MC.to_i16(x) if in_dtype == torch.int16 else x)
    lengths = torch.full((B,), Nmax, dtype=torch.int32)
    check(gpu, wav, lengths, A.MfccPlan(), None, None, f"buffer end {shape}", channels=(3,), dtypes=(torch.float32,))


def test_graph_replay_with_rewritten_inputs(gpu):
    """One captured call (a linear chain of two kernels), replayed after the waveform, the lengths and the packed
    table were overwritten in place, equals a fresh eager call bit for bit."""
    from xcp import ops
    plan = A.MfccPlan()
    first = (torch.from_numpy(MC.noise(16, 3 * 1500).reshape(3, 1500)), torch.tensor([1500, 700, 0], dtype=torch.int32),
             A.WaveParams([0, 3, 0], [0, 1, 0], [1.0, 0.8, 1.0]))
    second = (torch.from_numpy(MC.noise(17, 3 * 1500).reshape(3, 1500)), torch.tensor([900, 1500, 320], dtype=torch.int32),
              A.WaveParams([100, 0, 159], [2, 4, 0], [1.2, 1.0, 0.5]))
    w, ln, tab = first[0].to(gpu), first[1].to(gpu), first[2].to(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.mfcc(w, ln, plan, tab, 6, 3, torch.float32)   # warm-up (loads the library, uploads the plan)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, n = ops.mfcc(w, ln, plan, tab, 6, 3, torch.float32)
    seen = []
    for wav, lengths, table in (first, second):
        w.copy_(wav)
        ln.copy_(lengths)
        tab.copy_(table.pack())
        graph.replay()
        torch.cuda.synchronize()
        got, got_n = out.cpu().clone(), n.cpu().clone()
        eager, eager_n = ops.mfcc(wav.to(gpu), lengths.to(gpu), plan, table, 6, 3, torch.float32)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), eager.cpu().view(torch.int32)) and torch.equal(got_n, eager_n.cpu())
        ref, lim, ref_len = A.mfcc_reference(wav, lengths, plan, table, 6, 3)
        assert torch.equal(got_n, ref_len)
        MC.assert_within_lim(got, ref, lim, "graph replay")
        seen.append(got)
    assert not torch.equal(seen[0], seen[1])


def test_front_end_feeds_the_audio_model(gpu):
    from Models.XceptionLSTMA import XceptionLSTMA
    import xcp
    torch.manual_seed(0)
    model = XceptionLSTMA(32, pretrained=False).to(gpu).eval()
    front = xcp.WaveFrontEnd(xcp.MfccConfig())
    wav, lengths = MC.batch([MC.noise(18, 400), MC.noise(19, 200)])      # 3 and 2 frames
    with torch.no_grad():
        x, seq = front(wav.to(gpu), lengths.to(gpu))
        assert x.shape == (2, 3, 3, 13) and x.dtype == torch.float32 and seq.dtype == torch.int32
        ref, lim, ref_len = A.mfcc_reference(wav, lengths, front.plan, None, None, 3)
        assert torch.equal(seq.cpu(), ref_len) and ref_len.tolist() == [3, 2]
        MC.assert_within_lim(x.cpu(), ref, lim, "front end")
        assert not x[1, 2].any()                                            # the padded frame's input rows
        prob = model(model.extract_features(x), seq)
    torch.cuda.synchronize()
    assert prob.shape == (2, 1) and torch.isfinite(prob).all() and ((prob > 0) & (prob < 1)).all()
    aug = xcp.WaveFrontEnd(xcp.MfccConfig(), xcp.WaveAugment(front.cfg, 2, max_shift=30, gain_db=(-3.0, 3.0)))
    x, seq = aug(wav.to(gpu), lengths, np.random.default_rng(0))
    assert x.shape == (2, 2, 3, 13) and seq.tolist() == [2, 2] and torch.isfinite(x).all()
