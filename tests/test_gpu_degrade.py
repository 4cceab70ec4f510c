"""GPU tests of ``xcp_clip_degrade`` (degrade.hip): byte for byte against ``degrade_reference`` (the
kernel and the restatement perform the same integer arithmetic), each stage alone and all three, across
the workgroup tile's seams, at the ends of the buffers, with an out-of-range table, replayed from a HIP
graph, through the PinnedClipReader, and ``robustness_sweep``."""
import numpy as np
import pytest
import torch

import degrade_cases as DC

pytestmark = pytest.mark.gpu


def run(gpu, u8, lengths, tab):
    from xcp import ops
    out = ops.clip_degrade(u8.to(gpu), torch.as_tensor(lengths, dtype=torch.int32).to(gpu), tab)
    torch.cuda.synchronize()
    return out.cpu()


def mismatch(got, ref):
    bad = (got != ref).nonzero()
    return f"{len(bad)} bytes differ, first at {bad[0].tolist() if len(bad) else None}"


@pytest.mark.parametrize("stage", DC.STAGES)
@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stages_bytewise(gpu, size, stage):
    """B = 3, T = 3, lengths (3, 1, 0), each clip its own parameters; i = 0, 2, 4 walk the clips that have
    frames through every q in {1, 20, 50, 75, 100}, R in {1, 3, 7} and noise sigma in {1, 8, 64}."""
    for i in (0, 2, 4):
        u8, lengths, tab, ref = DC.batch_case(size, stage, i)
        got = run(gpu, u8, lengths, tab)
        assert torch.equal(got, ref), (i, mismatch(got, ref))


def test_tile_seams(gpu):
    """45 x 83: two by three 32 x 32 workgroup tiles, the last of each direction partial, all three stages
    on.  A wrong blur or chroma halo shows along the seams."""
    u8, lengths, tab, ref = DC.batch_case(DC.SEAM, "all", 1)
    got = run(gpu, u8, lengths, tab)
    assert torch.equal(got, ref), mismatch(got, ref)
    u8, lengths, tab, ref = DC.batch_case(DC.SEAM, "jpeg", 3)
    got = run(gpu, u8, lengths, tab)
    assert torch.equal(got, ref), mismatch(got, ref)


@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_buffer_ends(gpu, size):
    """in and out carved out of larger allocations at odd offsets, sentinel bytes before and after: the
    sentinels stay, the last frame of the last clip is right."""
    from xcp import ops
    from xcp.degrade import degrade_reference
    u8, _, tab, _ = DC.batch_case(size, "all", 0)
    lengths = torch.tensor((1, 2, 3), dtype=torch.int32)
    ref = degrade_reference(u8, lengths, tab)
    n, pre = u8.numel(), 13
    src = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    dst = torch.full((n + 64,), 0x5A, dtype=torch.uint8, device=gpu)
    src[pre:pre + n] = u8.to(gpu).view(-1)
    got = ops.clip_degrade(src[pre:pre + n].view(u8.shape), lengths.to(gpu), tab, out=dst[pre + 2:pre + 2 + n].view(u8.shape))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ref), mismatch(got.cpu(), ref)
    assert torch.equal(got.cpu()[2, 2], ref[2, 2])
    d = dst.cpu()
    assert bool((d[:pre + 2] == 0x5A).all()) and bool((d[pre + 2 + n:] == 0x5A).all())
    s = src.cpu()
    assert bool((s[:pre] == 0xA5).all()) and bool((s[pre + n:] == 0xA5).all()) and torch.equal(s[pre:pre + n], u8.view(-1))


def test_offsets_past_2_31(gpu):
    """10,924 one-frame clips of 256^2: the last clip starts past byte 2^31 of in and out.  Every other clip has
    length 0 (zeros written, nothing to restate); the last is compared with the restatement of that clip alone
    (clip b of ``fixed`` draws its noise with seed + b)."""
    from xcp import ops
    from xcp.degrade import DegradeParams, degrade_reference
    B, S = 10924, 256
    assert (B - 1) * S * S * 3 > 2 ** 31
    last = DC.frames_u8(61, (1, 1, S, S, 3))
    u8 = torch.zeros((B, 1, S, S, 3), dtype=torch.uint8, device=gpu)
    u8[-1] = last[0].to(gpu)
    lengths = torch.zeros(B, dtype=torch.int32, device=gpu)
    lengths[-1] = 1
    out = torch.full_like(u8, 0x5A)
    ops.clip_degrade(u8, lengths, DegradeParams.fixed(B, quality=50, sigma=1.0, noise=8.0, seed=3), out=out)
    torch.cuda.synchronize()
    ref = degrade_reference(last, [1], DegradeParams.fixed(1, quality=50, sigma=1.0, noise=8.0, seed=3 + B - 1))
    assert torch.equal(out[-1].cpu(), ref[0]), mismatch(out[-1].cpu(), ref[0])
    assert not bool(out[:-1].any())


def test_out_of_range_table(gpu):
    """quality 250, R 99, namp 10^6 in a packed device table: the kernel's clamps (100, 7, 1023), which
    ``DegradeParams.row`` restates; nothing outside out changes."""
    from xcp import ops
    from xcp.degrade import DegradeParams, degrade_reference, gaussian_taps
    H, W = 17, 19
    u8 = DC.frames_u8(31, (3, 2, H, W, 3))
    lengths = torch.tensor((2, 2, 1), dtype=torch.int32)
    wild = DegradeParams.fixed(3, seed=9)
    wild.taps[:] = torch.tensor(gaussian_taps(2.5)[1])
    wild.quality[:] = torch.tensor([250, -7, 250])
    wild.radius[:] = torch.tensor([99, 99, -3])
    wild.namp[:] = torch.tensor([10 ** 6, -5, 10 ** 6])
    with pytest.raises(ValueError):
        ops.clip_degrade(u8.to(gpu), lengths.to(gpu), wild)
    clamped = DegradeParams.unpack(wild.pack())
    clamped.quality[:] = torch.tensor([100, 0, 100])
    clamped.radius[:] = torch.tensor([7, 7, 0])
    clamped.namp[:] = torch.tensor([1023, 0, 1023])
    ref = degrade_reference(u8, lengths, clamped)
    assert torch.equal(ref, degrade_reference(u8, lengths, wild))
    n = u8.numel()
    dst = torch.full((n + 128,), 0x5A, dtype=torch.uint8, device=gpu)
    got = ops.clip_degrade(u8.to(gpu), lengths.to(gpu), wild.to(gpu), out=dst[64:64 + n].view(u8.shape))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), ref), mismatch(got.cpu(), ref)
    d = dst.cpu()
    assert bool((d[:64] == 0x5A).all()) and bool((d[64 + n:] == 0x5A).all())


def test_graph_replay_with_rewritten_table(gpu):
    """One captured call, replayed after the device table was overwritten in place, computes the second
    table's result."""
    from xcp import ops
    from xcp.degrade import degrade_reference
    u8 = DC.frames_u8(41, (3, 3, 24, 40, 3))
    lengths = torch.tensor(DC.LENGTHS, dtype=torch.int32)
    first, second = DC.table("all", 0), DC.table("all", 1)
    assert not first.equal(second)
    f, ln, tab = u8.to(gpu), lengths.to(gpu), first.to(gpu)
    out = torch.empty_like(f)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.clip_degrade(f, ln, tab, out=out)   # warm-up
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.clip_degrade(f, ln, tab, out=out)
    for table in (first, second):
        tab.copy_(table.pack())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), degrade_reference(u8, lengths, table))


def test_pinned_reader_degrade(gpu, tmp_path):
    """PinnedClipReader(degrade=..., augment=...) yields ops.clip_degrade then ops.clip_augment of
    read_batch's host frames with the same seeded tables; degrade=None is today's output."""
    from Dataset.video_dataloader import PinnedClipReader, get_face_dataloader
    from xcp import ops
    from xcp.augment import ClipAugment
    from xcp.degrade import ClipDegrade, degrade_reference
    rs = np.random.RandomState(6)
    for i, t in enumerate((4, 7, 2, 5, 3)):
        np.save(tmp_path / f"{'real' if i % 2 else 'fake'}_{i}.npy", rs.randint(0, 256, (t, 16, 12, 3), dtype=np.uint8))
    aug = ClipAugment((11, 9), scale=(0.4, 1.0), flip=0.5, brightness=0.1, contrast=0.2, erase=0.5, frames=3,
                      strides=(1, 2))
    deg = ClipDegrade(jpeg_p=0.7, blur_p=0.6, noise_p=0.6)
    reader = PinnedClipReader(str(tmp_path), 2, "cuda:0", augment=aug, degrade=deg, seed=11, dtype=torch.bfloat16)
    seen = 0
    for epoch in range(2):
        got = [(c.cpu(), lab.cpu(), ln.cpu()) for c, lab, ln in reader]
        assert len(got) == 3
        for i, (paths, (c, lab, ln)) in enumerate(zip(reader.batches(), got)):
            _, frames, labels, lengths = PinnedClipReader.read_batch(paths)
            for b, n in enumerate(lengths.tolist()):
                frames[b, n:] = 0   # read_batch leaves them as they are; both kernels ignore them
            dtab = reader.degrade_table(epoch, i, len(paths))
            seen += int((dtab.quality > 0).sum() + (dtab.radius > 0).sum() + (dtab.namp > 0).sum())
            table = reader.augment_table(epoch, i, lengths, 16, 12)
            d = ops.clip_degrade(frames.to(gpu), lengths.to(gpu), dtab)
            assert torch.equal(d.cpu(), degrade_reference(frames, lengths, dtab))
            ref, ref_len = ops.clip_augment(d, lengths.to(gpu), table, aug.size, aug.frames, torch.bfloat16)
            assert torch.equal(c, ref.cpu()) and torch.equal(ln, ref_len.cpu()) and torch.equal(lab, labels)
    assert seen > 6   # the tables did degrade
    # without augment: degrade then frames_prep
    only = PinnedClipReader(str(tmp_path), 2, "cuda:0", degrade=deg, seed=11)
    for i, (paths, (c, _, ln)) in enumerate(zip(only.batches(), only)):
        _, frames, _, lengths = PinnedClipReader.read_batch(paths)
        d = ops.clip_degrade(frames.to(gpu), lengths.to(gpu), only.degrade_table(0, i, len(paths)))
        assert torch.equal(c, ops.frames_prep(d, lengths.to(gpu))) and torch.equal(ln.cpu(), lengths)
    ref = list(get_face_dataloader(str(tmp_path), batch_size=2))
    plain = [(c.cpu(), lab.cpu()) for c, lab, _ in PinnedClipReader(str(tmp_path), 2, "cuda:0", degrade=None)]
    assert len(plain) == len(ref)
    for (c, lab), (rc, rl) in zip(plain, ref):
        assert torch.equal(c, rc) and torch.equal(lab, rl)


def test_wrapper_validates(gpu):
    from xcp import ops
    from xcp.degrade import DegradeParams
    u8 = torch.zeros((2, 3, 8, 8, 3), dtype=torch.uint8, device=gpu)
    lengths = torch.tensor([3, 2], dtype=torch.int32, device=gpu)
    ok = DegradeParams.fixed(2, quality=50)
    with pytest.raises(ValueError):
        ops.clip_degrade(u8.float(), lengths, ok)
    with pytest.raises(ValueError):
        ops.clip_degrade(u8[..., :2], lengths, ok)
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths.long(), ok)
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths, DegradeParams.fixed(3, quality=50))
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths, torch.zeros((2, 24), dtype=torch.int32, device=gpu))
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths, ok, out=u8)
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths, ok, out=torch.empty((2, 3, 8, 8, 3), dtype=torch.int32, device=gpu))
    over = DegradeParams.fixed(2, noise=64.0)
    over.namp[:] = int(round(65.0 * 2 ** 20 / 107019.7))
    with pytest.raises(ValueError):
        ops.clip_degrade(u8, lengths, over)
    with pytest.raises(ValueError):
        DegradeParams.fixed(2, noise=64.5)
    assert ops.clip_degrade(u8, lengths, ok).shape == u8.shape


def test_robustness_sweep(gpu):
    """A level with everything 0 is the plain scoring path bit for bit; the shape is [L, B]; chunked and whole
    scoring agree in the logit to test_gpu_stream_score.py's 1e-4."""
    import xcp
    from Models.XceptionLSTMV import XceptionLSTMV
    from xcp import ops
    from xcp.augment import ClipAugment
    torch.manual_seed(0)
    m = XceptionLSTMV(8, pretrained=False).to(gpu).eval()
    u8 = DC.frames_u8(51, (2, 2, 64, 64, 3)).to(gpu)
    lengths = torch.tensor([2, 1], dtype=torch.int32, device=gpu)
    levels = [dict(quality=0, sigma=0.0, noise=0.0), dict(quality=30), dict(quality=75, sigma=1.0, noise=4.0)]
    with xcp.precision("fp32"):
        got = xcp.robustness_sweep(m, u8, lengths, levels, (64, 64))
        chunked = xcp.robustness_sweep(m, u8, lengths, levels, (64, 64), chunk=1)
        with torch.no_grad():
            clips, ln = ops.clip_augment(u8, lengths, ClipAugment.eval((64, 64)).sample([2, 1], 64, 64), (64, 64))
            plain = m(m.extract_features(clips), ln)
    torch.cuda.synchronize()
    assert got.shape == (3, 2) and chunked.shape == (3, 2) and got.device == u8.device and not got.requires_grad
    assert torch.equal(got[0], plain.reshape(2))
    print("sweep probabilities:", got.tolist())
    # every level is that level's degraded clip through the same path (the untrained head is too flat for the
    # probabilities themselves to tell the levels apart)
    from xcp.degrade import DegradeParams
    with xcp.precision("fp32"), torch.no_grad():
        for i, level in enumerate(levels[1:], 1):
            d = ops.clip_degrade(u8, lengths, DegradeParams.fixed(2, **level))
            assert not torch.equal(d[0], u8[0])
            clips, ln = ops.clip_augment(d, lengths, ClipAugment.eval((64, 64)).sample([2, 1], 64, 64), (64, 64))
            assert torch.equal(got[i], m(m.extract_features(clips), ln).reshape(2))
    assert float(got.min()) > 0.0 and float(got.max()) < 1.0

    def logit(p):
        p = p.double().cpu()
        return (p / (1 - p)).log()
    d = float((logit(got) - logit(chunked)).abs().max())
    print(f"whole vs chunked logit: max abs diff {d:.2e}")
    assert d <= 1e-4
