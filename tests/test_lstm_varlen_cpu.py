"""CPU tests of the variable-length LSTM surface: the two length-aware ops are registered with fake
kernels (meta device), ``xcp.lstm.LSTM`` validates host lengths by ``pack_padded_sequence``'s rule
before it looks at the device, and the clip models accept ``seq_lengths``."""
import inspect

import pytest
import torch


def meta(*shape, dt=torch.float32):
    return torch.empty(shape, device="meta", dtype=dt)


def test_varlen_ops_registered_with_fake_kernels():
    from xcp import torch_ops
    for name in ("lstm_varlen", "lstm_varlen_backward"):
        assert name in torch_ops.OPS and hasattr(torch.ops.xcp, name), name
    B, T, I, H = 4, 16, 2048, 128
    x, w_ih, w_hh, lens = meta(B, T, I), meta(4 * H, I), meta(4 * H, H), meta(B, dt=torch.int32)
    out = torch.ops.xcp.lstm_varlen(x, w_ih, w_hh, meta(4 * H), meta(4 * H), lens, 0)
    assert [tuple(t.shape) for t in out] == [(B, T, H), (1, B, H), (1, B, H), (B, T, H), (B, T, H), (B, T, 4 * H)]
    assert all(t.dtype == torch.float32 for t in out)
    for need_dx, dx_shape in ((True, (B, T, I)), (False, (0,))):
        g = torch.ops.xcp.lstm_varlen_backward(meta(B, T, H), meta(1, B, H), None, x, w_ih, w_hh, meta(B, T, H),
                                               meta(B, T, H), meta(B, T, 4 * H), lens, 0, need_dx)
        assert [tuple(t.shape) for t in g] == [dx_shape, (4 * H, I), (4 * H, H), (4 * H,)]


@pytest.mark.parametrize("lengths", [torch.tensor([3, 2]), torch.tensor([[3, 2, 1]]), torch.tensor([3, 0, 2]),
                                     torch.tensor([3, 6, 2]), torch.tensor([3, -1, 2], dtype=torch.int32)])
def test_host_lengths_are_validated(lengths):
    """Shape [B] and 1 <= L <= T, else ValueError -- before the device check, so a CPU input shows it."""
    from xcp.lstm import LSTM
    lstm = LSTM(8, 64, 1, batch_first=True)
    with pytest.raises(ValueError, match="lengths"):
        lstm(torch.zeros(3, 5, 8), lengths=lengths)


def test_valid_host_lengths_reach_the_device_check():
    from torch.nn.utils.rnn import pack_padded_sequence
    from xcp.lstm import LSTM
    lstm = LSTM(8, 64, 1, batch_first=True)
    x = torch.zeros(3, 5, 8)
    for lens in (torch.tensor([5, 1, 3]), torch.tensor([5, 1, 3], dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="MI355X"):
            lstm(x, lengths=lens)
    with pytest.raises(RuntimeError, match="MI355X"):
        lstm(pack_padded_sequence(x, torch.tensor([5, 1, 3]), batch_first=True, enforce_sorted=False))
    with pytest.raises(ValueError, match="lengths"):
        lstm(x, lengths=torch.tensor([5.0, 1.0, 3.0]))


def test_model_forwards_accept_seq_lengths():
    from Models.XceptionLSTMA import XceptionLSTMA
    from Models.XceptionLSTMV import XceptionLSTMV
    for cls in (XceptionLSTMV, XceptionLSTMA):
        p = inspect.signature(cls.forward).parameters
        assert list(p) == ["self", "features", "seq_lengths"] and p["seq_lengths"].default is None, cls
    from xcp.lstm import LSTM
    p = inspect.signature(LSTM.forward).parameters
    assert list(p) == ["self", "input", "hx", "lengths"] and p["lengths"].default is None
