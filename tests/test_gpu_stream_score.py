"""``xcp.score_in_chunks`` and the clip models' ``forward_state`` on the GPU: XceptionLSTMV(128), fp32, seeded,
three clips x 5 frames x 3 x 64^2 with lengths [5, 1, 3], scored in chunks of 2, 2 and 1 frames with the LSTM
state carried, against the unchunked ``extract_features`` -> ``lstm(lengths=)`` -> head path.  The backbone sees
another batch size per chunk than in the whole run (other GEMM tilings), so the pre-sigmoid logits are compared
within 1e-4 absolute -- the fp32 logit bound of SURVEY section 8c -- not bit for bit."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence

pytestmark = pytest.mark.gpu

B, T, S, CHUNK = 3, 5, 64, 2
LENS = [5, 1, 3]


@pytest.fixture(scope="module")
def setup(gpu):
    import xcp
    from Models.XceptionLSTMV import XceptionLSTMV
    torch.manual_seed(0)
    m = XceptionLSTMV(128, pretrained=False).to(gpu).eval()
    clips = torch.rand((B, T, 3, S, S), generator=torch.Generator().manual_seed(5))
    for b, L in enumerate(LENS):
        clips[b, L:] = 0.0
    clips = clips.to(gpu)
    with torch.no_grad(), xcp.precision("fp32"):   # the unchunked reference, computed once
        _, (h, _) = m.lstm(m.extract_features(clips), lengths=torch.tensor(LENS))
        logit = m.fc_out(m.fc_layers(h[0]))
        prob = m(m.extract_features(clips), torch.tensor(LENS))
    torch.cuda.synchronize()
    return m, clips, logit.cpu(), prob.cpu()


def logit_of(prob):
    p = prob.double()
    return (p / (1 - p)).log().float()


def test_chunked_logit_equals_unchunked(setup, gpu):
    import xcp
    m, clips, want, want_prob = setup
    lens = torch.tensor(LENS, device=gpu)
    sizes, state, first = [], None, None
    with torch.no_grad(), xcp.precision("fp32"):
        for off in range(0, T, CHUNK):
            feats = m.extract_features(clips[:, off:off + CHUNK])
            sizes.append(feats.shape[1])
            prob, state = m.forward_state(feats, (lens - off).clamp(0, CHUNK), state)
            first = state if first is None else first
        early = m.fc_out(m.fc_layers(first[0][0])).cpu()   # the logits after the first chunk alone
        logit = m.fc_out(m.fc_layers(state[0][0]))
        scored = xcp.score_in_chunks(m, clips, torch.tensor(LENS), chunk=CHUNK)
    torch.cuda.synchronize()
    assert sizes == [2, 2, 1]
    d = float((logit.cpu() - want).abs().max())
    print(f"chunked vs unchunked logit: max abs diff {d:.2e}, |logit| {float(want.abs().max()):.3e}")
    assert d <= 1e-4
    # the comparison can see a state that is dropped: the 5-frame clip's logit still moves after chunk 1 by more
    # than the bound (1.6e-4 measured: the untrained head is flat), while the 1-frame clip, which has length 0 in
    # the later chunks, keeps its state bit for bit
    moved = (early - want).abs()
    print(f"logit after chunk 1 vs final: {moved.flatten().tolist()}, "
          f"|h| moved {float((first[0][0, 0] - state[0][0, 0]).abs().max()):.2e}")
    assert float(moved[0]) > 1e-4
    assert torch.equal(first[0][0, 1], state[0][0, 1]) and torch.equal(first[1][0, 1], state[1][0, 1])
    assert float(want_prob.min()) > 0.0 and float(want_prob.max()) < 1.0
    np.testing.assert_allclose(prob.cpu().numpy(), torch.sigmoid(logit).cpu().numpy(), rtol=0, atol=1e-6)
    np.testing.assert_allclose(scored.cpu().numpy(), torch.sigmoid(logit).cpu().numpy(), rtol=0, atol=1e-6)
    assert scored.shape == (B, 1) and not scored.requires_grad


def test_one_chunk_reproduces_the_unchunked_call(setup, gpu):
    import xcp
    m, clips, want, want_prob = setup
    with xcp.precision("fp32"):
        for chunk in (T, 16):
            got = xcp.score_in_chunks(m, clips, torch.tensor(LENS), chunk=chunk).cpu()
            assert float((logit_of(got) - want).abs().max()) <= 1e-4
            assert float((got - want_prob).abs().max()) <= 1e-4
        # without lengths every clip has T frames
        got = xcp.score_in_chunks(m, clips, chunk=CHUNK).cpu()
        with torch.no_grad():
            whole = m(m.extract_features(clips)).cpu()
    assert float((logit_of(got) - logit_of(whole)).abs().max()) <= 1e-4


def test_modes_grads_and_buffers_untouched(setup, gpu):
    import xcp
    m, clips, _, _ = setup
    m.train()
    m.fc_layers.eval()
    modes = {n: s.training for n, s in m.named_modules()}
    bufs = {n: b.clone() for n, b in m.named_buffers()}
    try:
        with xcp.precision("fp32"):
            xcp.score_in_chunks(m, clips, torch.tensor(LENS), chunk=CHUNK)
        torch.cuda.synchronize()
        assert {n: s.training for n, s in m.named_modules()} == modes
        assert all(p.grad is None for p in m.parameters())
        assert bufs and all(torch.equal(b, bufs[n]) for n, b in m.named_buffers())
    finally:
        m.eval()


def test_lstma_forward_state(gpu):
    """XceptionLSTMA(64): one forward_state(features, seq_lengths, state) on random [2, 4, 2048] features -- the
    H = 64 kernels -- against nn.LSTM + the head on the CPU."""
    from Models.XceptionLSTMA import XceptionLSTMA
    torch.manual_seed(0)
    m = XceptionLSTMA(64, pretrained=False).eval()
    ref_lstm = nn.LSTM(2048, 64, 1, batch_first=True)
    ref_lstm.load_state_dict(m.lstm.state_dict())
    fc_layers, fc_out = copy.deepcopy(m.fc_layers).eval(), copy.deepcopy(m.fc_out)
    m = m.to(gpu)
    g = torch.Generator().manual_seed(9)
    feats = torch.randn((2, 4, 2048), generator=g)
    feats[1, 2:] = 0.0
    lens = [4, 2]
    h0, c0 = torch.randn((1, 2, 64), generator=g), torch.randn((1, 2, 64), generator=g)
    with torch.no_grad():
        _, (h, c) = ref_lstm(pack_padded_sequence(feats, torch.tensor(lens), batch_first=True, enforce_sorted=False),
                             (h0, c0))
        want = torch.sigmoid(fc_out(fc_layers(h[0])))
        prob, (hn, cn) = m.forward_state(feats.to(gpu), torch.tensor(lens), (h0.to(gpu), c0.to(gpu)))
    np.testing.assert_allclose(hn.cpu().numpy(), h.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(cn.cpu().numpy(), c.numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(prob.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
