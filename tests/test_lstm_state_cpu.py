"""CPU tests of the LSTM initial-state surface: ``hx`` is validated before the device check, the two state ops
are registered with fake kernels, the C ABI's three new entries are declared and bound alike, the clip models
keep ``forward`` and gain ``forward_state``, and ``xcp.score_in_chunks`` walks a clip with the right offsets,
per-chunk lengths and carried state (backbone and LSTM monkeypatched, as tests/test_input_grad_cpu.py does)."""
import inspect
import os
import re

import pytest
import torch


def meta(*shape, dt=torch.float32):
    return torch.empty(shape, device="meta", dtype=dt)


def _lstm(H=64):
    from xcp.lstm import LSTM
    return LSTM(8, H, 1, batch_first=True)


@pytest.mark.parametrize("hx,exc,match", [
    ((torch.zeros(1, 3, 64),), ValueError, "tuple of two"),                                    # one tensor
    (torch.zeros(1, 3, 64), ValueError, "tuple of two"),                                       # not a tuple
    ((torch.zeros(1, 3, 64), torch.zeros(1, 3, 64), torch.zeros(1, 3, 64)), ValueError, "tuple of two"),
    ((torch.zeros(3, 64), torch.zeros(3, 64)), RuntimeError, "should also be 3-D"),            # nn.LSTM's words
    ((torch.zeros(1, 2, 64), torch.zeros(1, 2, 64)), RuntimeError, r"Expected hidden\[0\] size \(1, 3, 64\)"),
    ((torch.zeros(1, 3, 64), torch.zeros(1, 3, 32)), RuntimeError, r"Expected hidden\[1\] size \(1, 3, 64\)"),
    ((torch.zeros(2, 3, 64), torch.zeros(2, 3, 64)), RuntimeError, r"Expected hidden\[0\] size"),
    ((torch.zeros(1, 3, 64, dtype=torch.int64), torch.zeros(1, 3, 64)), ValueError, "floating"),
    ((meta(1, 3, 64), meta(1, 3, 64)), RuntimeError, "not at the same device"),
])
def test_hx_is_validated_before_the_device_check(hx, exc, match):
    with pytest.raises(exc, match=match):
        _lstm()(torch.zeros(3, 5, 8), hx)


def test_wrong_batch_message_is_nn_lstm_s():
    """the wrong-B refusal reads as torch.nn.LSTM's own"""
    import torch.nn as nn
    bad = (torch.zeros(1, 2, 64), torch.zeros(1, 2, 64))
    with pytest.raises(RuntimeError) as theirs:
        nn.LSTM(8, 64, 1, batch_first=True)(torch.zeros(3, 5, 8), bad)
    with pytest.raises(RuntimeError) as ours:
        _lstm()(torch.zeros(3, 5, 8), bad)
    assert str(ours.value) == str(theirs.value)


def test_well_formed_cpu_call_reaches_the_device_check():
    from torch.nn.utils.rnn import pack_padded_sequence
    lstm, x = _lstm(), torch.zeros(3, 5, 8)
    hx = (torch.zeros(1, 3, 64), torch.zeros(1, 3, 64))
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x, hx)
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x, hx, lengths=torch.tensor([5, 1, 3]))
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(pack_padded_sequence(x, torch.tensor([5, 1, 3]), batch_first=True, enforce_sorted=False), hx)
    with pytest.raises(ValueError, match="lengths"):   # the lengths rule still comes first
        lstm(x, hx, lengths=torch.tensor([5, 0, 3]))
    from xcp.lstm import LSTM
    with pytest.raises(NotImplementedError):           # the other refusals stay
        LSTM(8, 64, 2, batch_first=True)(x, hx)
    with pytest.raises(NotImplementedError):
        lstm(torch.zeros(5, 8), (torch.zeros(1, 64), torch.zeros(1, 64)))


def test_state_ops_registered_with_fake_kernels():
    from xcp import torch_ops
    for name in ("lstm_state", "lstm_state_backward"):
        assert name in torch_ops.OPS and hasattr(torch.ops.xcp, name), name
    B, T, I, H = 4, 16, 2048, 128
    x, w_ih, w_hh = meta(B, T, I), meta(4 * H, I), meta(4 * H, H)
    for lens in (None, meta(B, dt=torch.int32)):
        out = torch.ops.xcp.lstm_state(x, w_ih, w_hh, meta(4 * H), meta(4 * H), meta(1, B, H), meta(1, B, H), lens, 0)
        assert [tuple(t.shape) for t in out] == [(B, T, H), (1, B, H), (1, B, H), (B, T, H), (B, T, H), (B, T, 4 * H)]
        assert all(t.dtype == torch.float32 for t in out)
        for need_dx, need_h, need_c in ((True, True, True), (False, True, False), (True, False, False)):
            g = torch.ops.xcp.lstm_state_backward(meta(B, T, H), meta(1, B, H), None, x, w_ih, w_hh, meta(1, B, H),
                                                  meta(B, T, H), meta(B, T, H), meta(B, T, 4 * H), lens, 0, need_dx,
                                                  need_h, need_c)
            assert [tuple(t.shape) for t in g] == [(B, T, I) if need_dx else (0,), (4 * H, I), (4 * H, H), (4 * H,),
                                                   (1, B, H) if need_h else (0,), (1, B, H) if need_c else (0,)]
            assert all(t.dtype == torch.float32 for t in g)


def test_state_entry_points_declared_and_bound():
    from xcp import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xcp.h")).read()
    decls = dict(re.findall(r"int\s+(xcp_\w+)\(([^;]*)\);", hdr, re.S))
    want = {"xcp_lstm_state_needs_whhT": 3, "xcp_lstm_fwd_state": 19, "xcp_lstm_bwd_state": 17}
    for name, n in want.items():
        assert name in decls and name in _lib.SIGNATURES, name
        args = [a.strip() for a in decls[name].split(",") if a.strip()]
        assert len(args) == len(_lib.SIGNATURES[name]) == n, name
        for a, ct in zip(args, _lib.SIGNATURES[name]):   # pointers bound as pointers, ints as ints
            assert (("*" in a) or a.startswith("xcp_stream_t")) == (ct is _lib.P), (name, a)
    assert "xcp_lstm_state_needs_whhT" in _lib.SIZE_QUERIES
    assert hdr.count("nn.LSTM(...)(x, (h0, c0))") >= 3          # each entry cites the reference op
    for name, nargs in (("xcp_lstm_fwd", 16), ("xcp_lstm_bwd", 13), ("xcp_lstm_fwd_varlen", 17),
                        ("xcp_lstm_bwd_varlen", 14)):           # the four existing entries keep their signatures
        assert len(_lib.SIGNATURES[name]) == nargs == len([a for a in decls[name].split(",") if a.strip()])


def test_ops_refuse_half_a_state():
    from xcp import ops
    t = torch.zeros(1, 2, 64)
    with pytest.raises(ValueError, match="together"):
        ops.lstm_fwd(*([None] * 11), 2, 3, 64, 0, None, t, None)


def test_model_forward_unchanged_and_forward_state_shape(monkeypatch):
    from Models.XceptionLSTMA import XceptionLSTMA
    from Models.XceptionLSTMV import XceptionLSTMV
    from xcp import lstm as xl
    seen = []

    def fake(self, input, hx=None, lengths=None):  # noqa: A002
        seen.append((hx, lengths))
        B, T, H = input.shape[0], input.shape[1], self.hidden_size
        return torch.zeros(B, T, H), (torch.ones(1, B, H), torch.ones(1, B, H))

    monkeypatch.setattr(xl.LSTM, "forward", fake)
    for cls in (XceptionLSTMV, XceptionLSTMA):
        p = inspect.signature(cls.forward).parameters
        assert list(p) == ["self", "features", "seq_lengths"], cls
        p = inspect.signature(cls.forward_state).parameters
        assert list(p) == ["self", "features", "seq_lengths", "state"] and p["state"].default is None
        torch.manual_seed(0)
        m = cls(64, pretrained=False).eval()
        feats = torch.zeros(2, 4, 2048)
        seen.clear()
        assert m(feats).shape == (2, 1) and seen == [(None, None)]          # today's call, no state passed
        state = (torch.zeros(1, 2, 64), torch.zeros(1, 2, 64))
        lens = torch.tensor([4, 2])
        seen.clear()
        prob, (h, c) = m.forward_state(feats, lens, state)
        assert prob.shape == (2, 1) and h.shape == (1, 2, 64) and c.shape == (1, 2, 64)
        assert seen[0][0] is state and seen[0][1] is lens
        with torch.no_grad():
            assert torch.equal(prob, m.sigmoid(m.fc_out(m.fc_layers(h[0]))))


def test_score_in_chunks_arithmetic(monkeypatch):
    """T = 7, chunk = 3, lengths [7, 1, 4, 3]: offsets 0 / 3 / 6, a short last chunk, per-chunk lengths
    clamp(L - off, 0, chunk), the state handed from chunk to chunk, modes restored, eval + no_grad inside."""
    import xcp
    from Models.XceptionLSTMV import XceptionLSTMV
    from xcp import lstm as xl
    B, T, H = 4, 7, 64
    frames, calls = [], []

    def fake_features(self, video_batch, device=None):
        assert not self.training and not self.feature_extractor.training and not torch.is_grad_enabled()
        frames.append(video_batch[0, :, 0, 0, 0].tolist())
        return video_batch[:, :, 0, 0, :1].expand(-1, -1, 2048).contiguous()

    def fake_lstm(self, input, hx=None, lengths=None):  # noqa: A002
        calls.append((input.shape[1], None if lengths is None else lengths.tolist(), hx))
        n = len(calls)
        return input[..., :H], (torch.full((1, B, H), float(n)), torch.full((1, B, H), -float(n)))

    monkeypatch.setattr(XceptionLSTMV, "extract_features", fake_features)
    monkeypatch.setattr(xl.LSTM, "forward", fake_lstm)
    torch.manual_seed(0)
    m = XceptionLSTMV(H, pretrained=False).train()
    m.fc_layers.eval()
    modes = {n: s.training for n, s in m.named_modules()}
    clips = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1, 1).expand(B, T, 3, 4, 4).contiguous()
    prob = xcp.score_in_chunks(m, clips, torch.tensor([7, 1, 4, 0 + 3]), chunk=3)
    assert frames == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0]]
    assert [c[0] for c in calls] == [3, 3, 1]
    assert [c[1] for c in calls] == [[3, 1, 3, 3], [3, 0, 1, 0], [1, 0, 0, 0]]
    assert calls[0][2] is None
    for n in (1, 2):   # chunk n + 1 starts from what chunk n returned
        h, c = calls[n][2]
        assert torch.equal(h, torch.full((1, B, H), float(n))) and torch.equal(c, torch.full((1, B, H), -float(n)))
    assert prob.shape == (B, 1) and not prob.requires_grad
    assert {n: s.training for n, s in m.named_modules()} == modes
    m.eval()
    with torch.no_grad():   # the head reads the last chunk's h_n
        assert torch.equal(prob, m.sigmoid(m.fc_out(m.fc_layers(torch.full((B, H), 3.0)))))

    # no lengths: none are made up; chunk >= T is one call
    calls.clear()
    xcp.score_in_chunks(m, clips, chunk=16)
    assert [(c[0], c[1]) for c in calls] == [(7, None)] and calls[0][2] is None
    # the refusals of input_gradient: 5-D clips only
    with pytest.raises(ValueError, match=r"\[B, T, 3, H, W\]"):
        xcp.score_in_chunks(m, torch.zeros(2, 3, 3, 13))
    with pytest.raises(ValueError, match="chunk"):
        xcp.score_in_chunks(m, clips, chunk=0)
    with pytest.raises(ValueError, match="seq_lengths"):
        xcp.score_in_chunks(m, clips, torch.tensor([7, 1, 4]))
