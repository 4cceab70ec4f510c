"""CPU tests of the bidirectional LSTM surface: ``LSTM(..., bidirectional=True)`` validates its arguments and then
reaches the device check instead of refusing the configuration, the two ops are registered with fake kernels, the
C ABI's three direction-aware entries are declared and bound alike, and the clip models take ``bidirectional=``
without changing their default form (LSTM monkeypatched, as tests/test_lstm_state_cpu.py does)."""
import os
import re

import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence


def meta(*shape, dt=torch.float32):
    return torch.empty(shape, device="meta", dtype=dt)


def _lstm(H=64):
    from xcp.lstm import LSTM
    return LSTM(8, H, 1, batch_first=True, bidirectional=True)


def test_well_formed_cpu_calls_reach_the_device_check():
    lstm, x = _lstm(), torch.zeros(3, 5, 8)
    hx = (torch.zeros(2, 3, 64), torch.zeros(2, 3, 64))
    lens = torch.tensor([5, 1, 3])
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x)
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x, lengths=lens)
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x, hx)
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(x, hx, lengths=lens)
    for h in (None, hx):
        with pytest.raises(RuntimeError, match="MI355X"):
            lstm(pack_padded_sequence(x, lens, batch_first=True, enforce_sorted=False), h)


def test_validation_comes_before_the_device_check():
    lstm, x = _lstm(), torch.zeros(3, 5, 8)
    hx = (torch.zeros(2, 3, 64), torch.zeros(2, 3, 64))
    with pytest.raises(ValueError, match="lengths"):
        lstm(x, hx, lengths=torch.tensor([5, 0, 3]))
    with pytest.raises(ValueError, match="lengths"):
        lstm(x, lengths=torch.tensor([5, 1]))
    with pytest.raises(RuntimeError, match=r"Expected hidden\[0\] size \(2, 3, 64\)"):
        lstm(x, (torch.zeros(1, 3, 64), torch.zeros(1, 3, 64)))
    with pytest.raises(RuntimeError, match=r"Expected hidden\[1\] size \(2, 3, 64\)"):
        lstm(x, (torch.zeros(2, 3, 64), torch.zeros(1, 3, 64)))
    with pytest.raises(ValueError, match="tuple of two"):
        lstm(x, torch.zeros(2, 3, 64))


def test_one_direction_state_message_is_nn_lstm_s():
    """a [1, B, H] state for a bidirectional module is refused in torch.nn.LSTM's own words"""
    bad = (torch.zeros(1, 3, 64), torch.zeros(1, 3, 64))
    with pytest.raises(RuntimeError) as theirs:
        nn.LSTM(8, 64, 1, batch_first=True, bidirectional=True)(torch.zeros(3, 5, 8), bad)
    with pytest.raises(RuntimeError) as ours:
        _lstm()(torch.zeros(3, 5, 8), bad)
    assert str(ours.value) == str(theirs.value)


def test_the_other_refusals_stay():
    from xcp.lstm import LSTM
    x = torch.zeros(3, 5, 8)
    with pytest.raises(NotImplementedError):
        LSTM(8, 64, 2, batch_first=True, bidirectional=True)(x)
    with pytest.raises(NotImplementedError):
        LSTM(8, 64, 2, batch_first=True)(x)
    with pytest.raises(NotImplementedError):
        LSTM(8, 64, 1, batch_first=True, bidirectional=True, bias=False)(x)
    with pytest.raises(NotImplementedError):
        LSTM(8, 64, 1, bidirectional=True)(x)                      # not batch_first
    with pytest.raises(NotImplementedError):
        _lstm()(torch.zeros(5, 8))                                 # unbatched


def test_parameters_are_nn_lstm_s():
    """names, shapes and init (same RNG consumption) as nn.LSTM, so its checkpoints load"""
    torch.manual_seed(3)
    ours = _lstm()
    torch.manual_seed(3)
    theirs = nn.LSTM(8, 64, 1, batch_first=True, bidirectional=True)
    assert list(ours.state_dict()) == list(theirs.state_dict())
    assert "weight_hh_l0_reverse" in ours.state_dict()
    for k, v in theirs.state_dict().items():
        assert torch.equal(ours.state_dict()[k], v), k
    ours.load_state_dict(theirs.state_dict())


def test_bidir_ops_registered_with_fake_kernels():
    from xcp import torch_ops
    for name in ("lstm_bidir", "lstm_bidir_backward"):
        assert name in torch_ops.OPS and hasattr(torch.ops.xcp, name), name
    B, T, I, H = 4, 16, 2048, 128
    x = meta(B, T, I)
    w = lambda: (meta(4 * H, I), meta(4 * H, H), meta(4 * H), meta(4 * H))   # noqa: E731
    (w_ih, w_hh, b_ih, b_hh), (w_ih_r, w_hh_r, b_ih_r, b_hh_r) = w(), w()
    for state in (False, True):
        h0, c0 = (meta(2, B, H), meta(2, B, H)) if state else (None, None)
        for lens in (None, meta(B, dt=torch.int32)):
            out = torch.ops.xcp.lstm_bidir(x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r, h0, c0, lens, 0)
            assert [tuple(t.shape) for t in out] == [(B, T, 2 * H), (2, B, H), (2, B, H), (2, B, T, H), (2, B, T, H),
                                                     (2, B * T, 4 * H)]
            assert all(t.dtype == torch.float32 for t in out)
            for need_dx, need_h, need_c in ((True, True, True), (False, True, False), (True, False, False),
                                            (False, False, False)):
                g = torch.ops.xcp.lstm_bidir_backward(meta(B, T, 2 * H), meta(2, B, H), None, x, w_ih, w_hh, w_ih_r,
                                                      w_hh_r, c0, out[3], out[4], out[5], lens, 0, need_dx, need_h,
                                                      need_c)
                per = [(4 * H, I), (4 * H, H), (4 * H,)]
                assert [tuple(t.shape) for t in g] == [(B, T, I) if need_dx else (0,), *per, *per,
                                                       (2, B, H) if need_h else (0,), (2, B, H) if need_c else (0,)]
                assert all(t.dtype == torch.float32 for t in g)


def test_dir_entry_points_declared_and_bound():
    from xcp import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xcp.h")).read()
    decls = dict(re.findall(r"int\s+(xcp_\w+)\(([^;]*)\);", hdr, re.S))
    want = {"xcp_lstm_dir_needs_whhT": 3, "xcp_lstm_fwd_dir": 20, "xcp_lstm_bwd_dir": 18}
    for name, n in want.items():
        assert name in decls and name in _lib.SIGNATURES, name
        args = [a.strip() for a in decls[name].split(",") if a.strip()]
        assert len(args) == len(_lib.SIGNATURES[name]) == n, name
        for a, ct in zip(args, _lib.SIGNATURES[name]):   # pointers bound as pointers, ints as ints
            assert (("*" in a) or a.startswith("xcp_stream_t")) == (ct is _lib.P), (name, a)
        assert n == 3 or args[-2] == "int dirs", name
    assert "xcp_lstm_dir_needs_whhT" in _lib.SIZE_QUERIES
    assert hdr.count("nn.LSTM(I, H, 1, batch_first=True, bidirectional=True)") >= 3   # each cites the reference op
    for name, nargs in (("xcp_lstm_needs_whhT", 3), ("xcp_lstm_fwd", 16), ("xcp_lstm_bwd", 13),
                        ("xcp_lstm_fwd_varlen", 17), ("xcp_lstm_bwd_varlen", 14), ("xcp_lstm_fwd_state", 19),
                        ("xcp_lstm_bwd_state", 17)):            # the existing entries keep their signatures
        assert len(_lib.SIGNATURES[name]) == nargs == len([a for a in decls[name].split(",") if a.strip()])


def test_ops_refuse_a_bad_mask_and_half_a_state():
    from xcp import ops
    t = torch.zeros(2, 2, 64)
    for dirs in (0, 4, -1):
        with pytest.raises(ValueError, match="dirs"):
            ops.lstm_fwd_dir(*([None] * 11), 2, 3, 64, dirs)
        with pytest.raises(ValueError, match="dirs"):
            ops.lstm_bwd_dir(*([None] * 7), 2, 3, 64, dirs)
    with pytest.raises(ValueError, match="together"):
        ops.lstm_fwd_dir(*([None] * 11), 2, 3, 64, 3, 0, None, t, None)


# state_dict keys of the default clip models, as the parent commit has them
DEFAULT_KEYS_TAIL = ["lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"] + \
    [f"fc_layers.{i}.{p}" for i in (0, 3, 6, 9) for p in ("weight", "bias")] + ["fc_out.weight", "fc_out.bias"]


@pytest.fixture(scope="module")
def models():
    from Models.XceptionLSTMA import XceptionLSTMA
    from Models.XceptionLSTMV import XceptionLSTMV
    made = {}
    for cls in (XceptionLSTMV, XceptionLSTMA):
        torch.manual_seed(0)
        plain = cls(64, pretrained=False)
        torch.manual_seed(0)
        same = cls(64, pretrained=False, bidirectional=False)
        torch.manual_seed(0)
        both = cls(64, pretrained=False, bidirectional=True)
        made[cls.__name__] = (plain, same, both)
    return made


@pytest.mark.parametrize("name", ["XceptionLSTMV", "XceptionLSTMA"])
def test_model_default_is_unchanged_and_bidirectional_adds_the_reverse_keys(models, name):
    plain, same, both = models[name]
    keys = list(plain.state_dict())
    head = [k for k in keys if not k.startswith("feature_extractor.")]
    assert head == DEFAULT_KEYS_TAIL
    assert keys[:len(keys) - len(head)] == [k for k in keys if k.startswith("feature_extractor.")]   # module order
    assert not plain.lstm.bidirectional and plain.fc_layers[0].weight.shape == (1024, 64)
    assert list(same.state_dict()) == keys
    for k, v in plain.state_dict().items():          # the keyword's default consumes the RNG as before
        assert torch.equal(v, same.state_dict()[k]), k
    bkeys = list(both.state_dict())
    rev = [f"lstm.{p}_l0_reverse" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    assert [k for k in bkeys if k not in keys] == rev and [k for k in keys if k not in bkeys] == []
    assert both.lstm.bidirectional and both.fc_layers[0].weight.shape == (1024, 128)
    assert both.state_dict()["lstm.weight_ih_l0_reverse"].shape == (256, 2048)


@pytest.mark.parametrize("name", ["XceptionLSTMV", "XceptionLSTMA"])
def test_bidirectional_model_feeds_the_head_both_final_states(models, name, monkeypatch):
    import xcp
    from xcp import lstm as xl
    seen = []
    g = torch.Generator().manual_seed(5)
    hn = torch.randn((2, 2, 64), generator=g)

    def fake(self, input, hx=None, lengths=None):  # noqa: A002
        seen.append((hx, lengths))
        B, T, H = input.shape[0], input.shape[1], self.hidden_size
        return torch.zeros(B, T, 2 * H), (hn, torch.ones(2, B, H))

    monkeypatch.setattr(xl.LSTM, "forward", fake)
    m = models[name][2].eval()
    feats, lens = torch.zeros(2, 4, 2048), torch.tensor([4, 2])
    with torch.no_grad():
        want = m.sigmoid(m.fc_out(m.fc_layers(torch.cat((hn[0], hn[1]), dim=1))))
        assert torch.equal(m(feats), want) and seen == [(None, None)]
        seen.clear()
        assert torch.equal(m(feats, lens), want) and seen[0][0] is None and seen[0][1] is lens
    with pytest.raises(ValueError, match="bidirectional"):
        m.forward_state(feats, lens, None)
    with pytest.raises(ValueError, match="bidirectional"):
        xcp.score_in_chunks(m, torch.zeros(2, 4, 3, 8, 8), lens, chunk=2)
