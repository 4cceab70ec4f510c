"""Variable-length clips through ``xcp.lstm.LSTM`` (lstm.hip with lengths) against ``torch.nn.LSTM`` on the CPU in
fp32 fed ``pack_padded_sequence(..., enforce_sorted=False)``, weights copied from the module under test.
Tolerances are those of test_gpu_kernels.py::test_lstm_module_vs_oracle: out / h_n / c_n rtol 1e-4,
atol 1e-5; dx and the parameter gradients rtol 1e-3, atol 1e-5.  The backward is driven by one seeded
random cotangent on out, h_n and c_n at once, with large garbage on the padded rows of out's cotangent,
so a kernel that reads dout past a clip's end fails."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

pytestmark = pytest.mark.gpu

I = 64   # input size (as test_opcheck_xcp_ops)
PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def make_lstm(H, dev, kernel=0, seed=0):
    from xcp.lstm import LSTM
    torch.manual_seed(seed)
    lstm = LSTM(I, H, 1, batch_first=True).to(dev)
    lstm.xcp_kernel = kernel
    return lstm


def make_inputs(B, T, H, lens, seed=0, pad_scale=0.0):
    """x [B,T,I] with the padded rows zero (or seeded values of magnitude pad_scale), and the cotangents
    of out / h_n / c_n, the padded rows of out's carrying garbage of magnitude 1e6."""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randn((B, T, I), generator=g)
    pad = torch.randn((B, T, I), generator=g) * pad_scale
    r = torch.randn((B, T, H), generator=g)
    junk = torch.randn((B, T, H), generator=g) * 1e6
    rh, rc = torch.randn((1, B, H), generator=g), torch.randn((1, B, H), generator=g)
    for b, L in enumerate(lens):
        L = min(max(int(L), 0), T)
        x[b, L:] = pad[b, L:]
        r[b, L:] = junk[b, L:]
    return x, r, rh, rc


def run_xcp(lstm, x, cot, dev, lengths=None, packed=False):
    """out, h_n, c_n, dx and the parameter gradients of one forward + backward on the GPU."""
    r, rh, rc = (t.to(dev) for t in cot)
    xg = x.to(dev).requires_grad_(True)
    for p in lstm.parameters():
        p.grad = None
    if packed:
        o, (h, c) = lstm(pack_padded_sequence(xg, lengths, batch_first=True, enforce_sorted=False))
        res_packed = o
        o, _ = pad_packed_sequence(o, batch_first=True, total_length=x.shape[1])
    else:
        o, (h, c) = lstm(xg) if lengths is None else lstm(xg, lengths=lengths)
        res_packed = None
    torch.autograd.backward([o, h, c], [r, rh, rc])
    torch.cuda.synchronize()
    res = {"out": o.detach().cpu(), "h_n": h.detach().cpu(), "c_n": c.detach().cpu(), "dx": xg.grad.cpu()}
    for n in PARAMS:
        res[n] = getattr(lstm, n).grad.cpu()
    if packed:
        res["packed"] = res_packed
    return res


def run_ref(lstm, x, cot, lens):
    """The same through nn.LSTM on the CPU with packed input (total_length = T)."""
    H, T = lstm.hidden_size, x.shape[1]
    ref = nn.LSTM(I, H, 1, batch_first=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
    xc = x.clone().requires_grad_(True)
    pk = pack_padded_sequence(xc, torch.as_tensor(lens, dtype=torch.int64), batch_first=True, enforce_sorted=False)
    po, (h, c) = ref(pk)
    o, _ = pad_packed_sequence(po, batch_first=True, total_length=T)
    torch.autograd.backward([o, h, c], list(cot))
    res = {"out": o.detach(), "h_n": h.detach(), "c_n": c.detach(), "dx": xc.grad, "packed": po}
    for n in PARAMS:
        res[n] = getattr(ref, n).grad
    return res


def assert_close(got, ref, keys=("out", "h_n", "c_n", "dx") + PARAMS):
    for k in keys:
        tol = dict(rtol=1e-4, atol=1e-5) if k in ("out", "h_n", "c_n") else dict(rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), err_msg=k, **tol)


def assert_identical(a, b, keys=("out", "h_n", "c_n", "dx") + PARAMS):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


def cyc(B, T):
    return [1 + b % T for b in range(B)]


CASES = {
    "H64": (64, 5, 7, [7, 1, 4, 7, 2], 0),
    "H128": (128, 5, 7, [7, 1, 4, 7, 2], 0),
    "H128-B33": (128, 33, 4, [4, 1, 3] * 11, 0),            # more clips than the per-step limit: per-clip kernel
    "H256-B17": (256, 17, 5, [5, 1, 3, 5, 2, 4] * 2 + [5, 1, 3, 2, 5], 0),   # crosses the backward's 16-clip pass
    # B = LS_MAXB.  At H 512 the per-step forward's LDS budget ends at 25 clips, so this shape takes the
    # generic pair (as it does without lengths); H512-B25 and H256-B32 are the per-step kernels' own edges
    "H512-B32": (512, 32, 5, cyc(32, 5), 0),
    "H512-B25": (512, 25, 5, cyc(25, 5), 0),
    "H256-B32": (256, 32, 5, cyc(32, 5), 0),
    "H1024": (1024, 3, 4, [2, 4, 1], 0),
    "H128-generic": (128, 5, 7, [7, 1, 4, 7, 2], 1),
}


@pytest.mark.parametrize("case", list(CASES))
def test_parity_by_kernel_family(gpu, case):
    """Each length-aware kernel family against the packed CPU nn.LSTM; host lengths, unsorted, with 1, T
    and repeats.  out and dx are exactly zero past each clip's length."""
    H, B, T, lens, kernel = CASES[case]
    assert len(lens) == B and 1 in lens and T in lens
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, T, H, lens)
    got = run_xcp(lstm, x, cot, gpu, lengths=torch.tensor(lens))
    ref = run_ref(lstm, x, cot, lens)
    for b, L in enumerate(lens):
        assert not got["out"][b, L:].any() and not got["dx"][b, L:].any(), b
    assert_close(got, ref)


BITWISE = {   # H, B, T, kernel: every kernel family that exists with and without lengths
    "64": (64, 3, 5, 0),                # register-resident
    "128": (128, 3, 5, 0),
    "256": (256, 3, 5, 0),              # per-step, KS = 8
    "512": (512, 3, 5, 0),              # per-step, KS = 16
    "1024": (1024, 3, 4, 0),            # per-step, KS = 32
    "128-generic": (128, 3, 5, 1),      # the generic pair, pinned
    "96": (96, 3, 5, 0),                # generic by shape: an H no special kernel takes
    "256-B17": (256, 17, 5, 0),         # crosses the per-step backward's 16-clip pass
}


@pytest.mark.parametrize("case", list(BITWISE))
def test_full_lengths_equal_fixed_path_bitwise(gpu, monkeypatch, case):
    """lengths = [T] * B is bit-identical to the call without lengths in every output and gradient: the
    two are instantiations of one kernel body.  (H 256 / 512: XCP_LSTM_PERSIST=0, so the call without
    lengths runs the per-step kernels too.)"""
    monkeypatch.setenv("XCP_LSTM_PERSIST", "0")
    H, B, T, kernel = BITWISE[case]
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, T, H, [T] * B)
    fixed = run_xcp(lstm, x, cot, gpu)
    full = run_xcp(lstm, x, cot, gpu, lengths=torch.tensor([T] * B))
    assert_identical(full, fixed)


@pytest.mark.parametrize("H", [128, 512])
def test_padding_content_does_not_matter(gpu, H):
    """Same lengths, padded input rows once zero and once seeded finite values of magnitude 1e3: every
    output and gradient is bit-identical, since the padding only ever meets exact zeros.  (NaN or Inf in
    the padding is out of contract: 0 x NaN is NaN in the weight-gradient GEMMs.)"""
    B, T, lens = 4, 6, [3, 6, 1, 4]
    lstm = make_lstm(H, gpu)
    x0, *cot = make_inputs(B, T, H, lens)
    x1, *_ = make_inputs(B, T, H, lens, pad_scale=1e3)
    assert float(x1[0, 3:].abs().max()) > 1e3 and torch.equal(x0[0, :3], x1[0, :3])
    a = run_xcp(lstm, x0, cot, gpu, lengths=torch.tensor(lens))
    b = run_xcp(lstm, x1, cot, gpu, lengths=torch.tensor(lens))
    assert_identical(a, b)


@pytest.mark.parametrize("H", [128, 256])
def test_device_lengths_are_clamped(gpu, H):
    """An int32 device tensor is passed through unread and clamped by the kernels: the 0 clip gives zero
    out / h_n / c_n / dx and adds nothing to the parameter gradients (the CPU reference runs without it),
    the over-long clip equals L = T, nothing is NaN."""
    B, T, lens = 4, 5, [0, 9, 2, 5]
    lstm = make_lstm(H, gpu)
    x, r, rh, rc = make_inputs(B, T, H, lens)
    got = run_xcp(lstm, x, (r, rh, rc), gpu, lengths=torch.tensor(lens, dtype=torch.int32, device=gpu))
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    for k in ("out", "dx"):
        assert not got[k][0].any(), k
    assert not got["h_n"][0, 0].any() and not got["c_n"][0, 0].any()
    same = run_xcp(lstm, x, (r, rh, rc), gpu, lengths=torch.tensor([0, T, 2, 5], dtype=torch.int32, device=gpu))
    assert_identical(got, same)
    ref = run_ref(lstm, x[1:], (r[1:], rh[:, 1:], rc[:, 1:]), [T, 2, 5])
    sub = {k: (v[1:] if k in ("out", "dx") else v[:, 1:] if k in ("h_n", "c_n") else v) for k, v in got.items()}
    assert_close(sub, ref)


def test_graph_replay_follows_the_lengths_tensor(gpu):
    """Forward and backward with a device lengths tensor captured in one graph; the lengths are overwritten
    in place and the replay is bit-identical to an eager call with the new lengths (no host read of them)."""
    H, B, T = 128, 4, 6
    lstm = make_lstm(H, gpu)
    params = [getattr(lstm, n) for n in PARAMS]
    x, *cot = make_inputs(B, T, H, [T] * B)
    xg = x.to(gpu).requires_grad_(True)
    r, rh, rc = (t.to(gpu) for t in cot)
    lens = torch.tensor([6, 2, 5, 1], dtype=torch.int32, device=gpu)

    def step():
        o, (h, c) = lstm(xg, lengths=lens)
        return [o, h, c] + list(torch.autograd.grad([o, h, c], [xg] + params, [r, rh, rc]))

    step()   # eager warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    lens.copy_(torch.tensor([3, 6, 1, 4], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in static]
    eager = step()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(replayed, eager)):
        assert torch.equal(a, b), i
    assert not replayed[0][0, 3:].any() and replayed[0][0, :3].any()


def test_packed_sequence_input(gpu):
    """lstm(PackedSequence) returns a PackedSequence with the input's batch_sizes / sorted_indices /
    unsorted_indices (those of the CPU module), data and states within tolerance, gradients flow to x."""
    H, B, T, lens = 128, 4, 6, [2, 6, 1, 4]
    lstm = make_lstm(H, gpu)
    x, *cot = make_inputs(B, T, H, lens)
    got = run_xcp(lstm, x, cot, gpu, lengths=torch.tensor(lens), packed=True)
    ref = run_ref(lstm, x, cot, lens)
    pg, pr = got["packed"], ref["packed"]
    assert isinstance(pg, PackedSequence)
    assert torch.equal(pg.batch_sizes, pr.batch_sizes)
    assert torch.equal(pg.sorted_indices.cpu(), pr.sorted_indices)
    assert torch.equal(pg.unsorted_indices.cpu(), pr.unsorted_indices)
    assert pg.data.is_cuda and pg.data.requires_grad
    np.testing.assert_allclose(pg.data.detach().cpu().numpy(), pr.data.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert got["dx"].any()
    assert_close(got, ref)


@pytest.mark.parametrize("name,H", [("XceptionLSTMV", 128), ("XceptionLSTMA", 512)])
def test_models_feed_the_head_the_last_real_state(gpu, monkeypatch, name, H):
    """forward(features, seq_lengths) against a plain-torch restatement (CPU packed nn.LSTM -> h_n[0] ->
    fc_layers -> fc_out -> sigmoid); forward(features) equals full lengths bit for bit and differs from
    the call with a short clip's length (a length that is accepted and dropped would not).
    XCP_LSTM_PERSIST=0 as in the bitwise test above: at H 512 the call without lengths would otherwise
    take the persistent forward, which sums the W_hh dot products in another order than the per-step
    kernels a call with lengths always takes."""
    import importlib
    monkeypatch.setenv("XCP_LSTM_PERSIST", "0")
    B, T, lens = 3, 6, [6, 2, 4]
    torch.manual_seed(0)
    m = getattr(importlib.import_module(f"Models.{name}"), name)(H, pretrained=False).eval()
    ref_lstm = nn.LSTM(2048, H, 1, batch_first=True)
    ref_lstm.load_state_dict(m.lstm.state_dict())
    fc_layers, fc_out = copy.deepcopy(m.fc_layers).eval(), copy.deepcopy(m.fc_out)
    m = m.to(gpu)
    feats = torch.randn((B, T, 2048), generator=torch.Generator().manual_seed(77))
    for b, L in enumerate(lens):
        feats[b, L:] = 0.0
    with torch.no_grad():
        _, (h_n, _) = ref_lstm(pack_padded_sequence(feats, torch.tensor(lens), batch_first=True, enforce_sorted=False))
        want = torch.sigmoid(fc_out(fc_layers(h_n[0])))
        fg = feats.to(gpu)
        got = m(fg, torch.tensor(lens))
        plain = m(fg)
        full = m(fg, torch.full((B,), T))
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
    assert torch.equal(plain, full)
    assert torch.equal(plain[0], got[0])   # the full-length clip
    assert not torch.equal(plain[1], got[1]) and not torch.equal(plain[2], got[2])


def test_opcheck_lstm_varlen(gpu):
    from xcp import torch_ops  # noqa: F401
    g = torch.Generator(device=gpu).manual_seed(0)

    def r(*shape):
        return torch.randn(shape, device=gpu, generator=g).requires_grad_(True)

    args = (r(2, 5, 64), r(512, 64), r(512, 128), r(512), r(512), torch.tensor([5, 3], dtype=torch.int32, device=gpu), 0)
    torch.library.opcheck(torch.ops.xcp.lstm_varlen, args,
                          test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
