"""GPU tests of ``xcp_clip_augment`` (frames.hip): bit for bit against ``augment_reference``
(the kernel and the restatement perform the same IEEE operations in the same order), the
identity table against ``xcp_frames_prep``, replay from a HIP graph after the device table was
rewritten in place, and the PinnedClipReader's augmenting path."""
import numpy as np
import pytest
import torch

import augment_cases as AC

pytestmark = pytest.mark.gpu

VARIANTS = [(torch.float32, False), (torch.float32, True), (torch.bfloat16, False), (torch.bfloat16, True)]


def check_all_variants(gpu, u8, lengths, table, size, out_frames, ref, ref_len):
    from xcp import ops
    f, ln, tab = u8.to(gpu), lengths.to(gpu), table.to(gpu)
    for dtype, cl in VARIANTS:
        out, n = ops.clip_augment(f, ln, tab, size, out_frames, dtype, cl)
        torch.cuda.synchronize()
        assert out.shape == ref.shape and out.dtype == dtype
        assert out.permute(0, 1, 3, 4, 2).is_contiguous() if cl else out.is_contiguous()
        assert torch.equal(n.cpu(), ref_len)
        assert torch.equal(out.cpu(), ref.to(dtype)), (dtype, cl)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("case", range(len(AC.CASES)), ids=AC.IDS)
def test_clip_augment_bitwise(gpu, case, flip):
    """B = 4 clips of up to 5 frames, lengths (5, 1, 3, 0); every clip its own box, flip, affine,
    erase rectangle and t0 / stride; fp32 and bf16, planar and channels_last."""
    check_all_variants(gpu, *AC.batch_case(case, flip))


@pytest.mark.parametrize("flip", [0, 1])
def test_clip_augment_bitwise_odd_sizes(gpu, flip):
    """Odd W, OW and OH; a second column tile (OW > 128) whose last wave is partly empty."""
    from xcp.augment import augment_reference
    h, w = 22, 19
    u8 = AC.clip_u8(200 + flip, (4, 5, h, w, 3))
    lengths = torch.tensor(AC.LENGTHS, dtype=torch.int32)
    for box, size in [((3, 2, 15, 11), (15, 21)), ((0, 0, h, w), (33, 139))]:
        table = AC.batch_table(box, size, flip, h, w, rot=1 + flip)
        ref, ref_len = augment_reference(u8, lengths, table, size, 3)
        check_all_variants(gpu, u8, lengths, table, size, 3, ref, ref_len)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 1, 1, 2), (1, 1, 1, 3), (1, 1, 2, 2), (2, 1, 1, 2), (1, 2, 3, 5)])
def test_clip_augment_buffer_end(gpu, shape):
    """The kernel fetches a source pixel pair with one 8-byte load that it keeps inside the
    buffer: the last pixels of the last frame of the last clip (here the whole, tiny, buffer:
    3 and 6 bytes are read bytewise, 9 and more through loads moved back from the end)."""
    from xcp.augment import AugmentParams, augment_reference
    B, T, h, w = shape
    u8 = AC.clip_u8(500, (64, 1, 2, 2, 3)).reshape(-1)[:B * T * h * w * 3].reshape(B, T, h, w, 3).contiguous()
    lengths = torch.full((B,), T, dtype=torch.int32)
    table = AugmentParams.identity(B, h, w)
    table.flip[:] = 1
    table.a[:] = torch.tensor(AC.A)
    for size in [(h, w), (3, 4)]:
        ref, ref_len = augment_reference(u8, lengths, table, size)
        check_all_variants(gpu, u8, lengths, table, size, None, ref, ref_len)


@pytest.mark.parametrize("size", [None, (17, 40)])
def test_identity_table_equals_frames_prep(gpu, size):
    from xcp import ops
    from xcp.augment import AugmentParams
    u8 = AC.clip_u8(300, (3, 4, AC.H, AC.W, 3)).to(gpu)
    lengths = torch.tensor([4, 1, 3], dtype=torch.int32, device=gpu)
    ident = AugmentParams.identity(3, AC.H, AC.W)
    for dtype, cl in VARIANTS:
        want = ops.frames_prep(u8, lengths, size, dtype, cl)
        got, n = ops.clip_augment(u8, lengths, ident, size or (AC.H, AC.W), None, dtype, cl)
        torch.cuda.synchronize()
        assert got.stride() == want.stride() and torch.equal(got, want), (dtype, cl)
        assert torch.equal(n, lengths)


def test_wrapper_validates(gpu):
    from xcp import ops
    from xcp.augment import AugmentParams
    u8 = torch.zeros((2, 3, 8, 8, 3), dtype=torch.uint8, device=gpu)
    lengths = torch.tensor([3, 2], dtype=torch.int32, device=gpu)
    bad = AugmentParams.identity(2, 8, 8)
    bad.bw[1] = 9
    with pytest.raises(ValueError):
        ops.clip_augment(u8, lengths, bad, (8, 8))
    with pytest.raises(ValueError):
        ops.clip_augment(u8, lengths, AugmentParams.identity(3, 8, 8), (8, 8))
    with pytest.raises(ValueError):
        ops.clip_augment(u8, lengths, torch.zeros((2, 12), dtype=torch.int32, device=gpu), (8, 8))
    with pytest.raises(RuntimeError):
        ops.clip_augment(u8.cpu(), lengths, AugmentParams.identity(2, 8, 8), (8, 8))


def test_graph_replay_with_rewritten_table(gpu):
    """One captured call, replayed after the device table was overwritten in place, computes
    the second table's result: the kernel reads everything data-dependent from device memory."""
    from xcp import ops
    from xcp.augment import ClipAugment, augment_reference
    u8 = AC.clip_u8(400, (4, 5, AC.H, AC.W, 3))
    lengths = torch.tensor(AC.LENGTHS, dtype=torch.int32)
    aug = ClipAugment((17, 13), scale=(0.3, 1.0), flip=0.5, brightness=0.2, contrast=0.3, erase=0.7, frames=3,
                      strides=(1, 2))
    first = aug.sample(lengths.tolist(), AC.H, AC.W, np.random.default_rng(1))
    second = aug.sample(lengths.tolist(), AC.H, AC.W, np.random.default_rng(2))
    assert not first.equal(second)
    f, ln, tab = u8.to(gpu), lengths.to(gpu), first.to(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ops.clip_augment(f, ln, tab, aug.size, aug.frames, torch.bfloat16)   # warm-up
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, n = ops.clip_augment(f, ln, tab, aug.size, aug.frames, torch.bfloat16)
    for table in (first, second):
        tab.copy_(table.pack())
        graph.replay()
        torch.cuda.synchronize()
        ref, ref_len = augment_reference(u8, lengths, table, aug.size, aug.frames, torch.bfloat16)
        assert torch.equal(out.cpu(), ref) and torch.equal(n.cpu(), ref_len)


def test_pinned_reader_augment(gpu, tmp_path):
    """PinnedClipReader(augment=...) equals augment_reference on read_batch's host frames with
    the same per-batch tables, over two epochs; augment=None is today's output."""
    from Dataset.video_dataloader import PinnedClipReader, get_face_dataloader
    from xcp.augment import ClipAugment, augment_reference
    rs = np.random.RandomState(6)
    for i, t in enumerate((4, 7, 2, 5, 3)):
        np.save(tmp_path / f"{'real' if i % 2 else 'fake'}_{i}.npy", rs.randint(0, 256, (t, 16, 12, 3), dtype=np.uint8))
    aug = ClipAugment((11, 9), scale=(0.4, 1.0), flip=0.5, brightness=0.1, contrast=0.2, erase=0.5, frames=3,
                      strides=(1, 2))
    reader = PinnedClipReader(str(tmp_path), 2, "cuda:0", augment=aug, seed=11, dtype=torch.bfloat16)
    for epoch in range(2):
        got = [(c.cpu(), lab.cpu(), ln.cpu()) for c, lab, ln in reader]
        assert len(got) == 3
        for i, (paths, (c, lab, ln)) in enumerate(zip(reader.batches(), got)):
            _, frames, labels, lengths = PinnedClipReader.read_batch(paths)
            table = reader.augment_table(epoch, i, lengths, 16, 12)
            ref, ref_len = augment_reference(frames, lengths, table, aug.size, aug.frames, torch.bfloat16)
            assert torch.equal(c, ref) and torch.equal(ln, ref_len) and torch.equal(lab, labels)
    ref = list(get_face_dataloader(str(tmp_path), batch_size=2))
    plain = [(c.cpu(), lab.cpu()) for c, lab, _ in PinnedClipReader(str(tmp_path), 2, "cuda:0", augment=None)]
    assert len(plain) == len(ref)
    for (c, lab), (rc, rl) in zip(plain, ref):
        assert torch.equal(c, rc) and torch.equal(lab, rl)
