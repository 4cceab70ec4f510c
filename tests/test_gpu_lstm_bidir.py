"""``xcp.lstm.LSTM(..., bidirectional=True)`` (lstm.hip's direction-aware instantiations) against
``torch.nn.LSTM(64, H, 1, batch_first=True, bidirectional=True)`` on the CPU in fp32 with weights copied, fed
packed input with ``enforce_sorted=False``.  Input size 64; inputs, states and one cotangent on out, h_n and c_n at
once are seeded, with 1e6 garbage on the padded rows of out's cotangent.  Tolerances are the project's LSTM ones
(test_gpu_lstm_state.py): out / h_n / c_n rtol 1e-4, atol 1e-5; dx, dh0, dc0 and the eight parameter gradients
rtol 1e-3, atol 1e-5.

What a tolerance cannot see is pinned exactly: direction 0 is the old kernel bit for bit, the reverse direction is
the forward kernel on mirrored time bit for bit, a zero state equals no state, full lengths equal no lengths, and a
clip of length 0 hands its state and its state's gradient on unchanged in both directions."""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from test_gpu_lstm_state import FAMILIES, cyc
from test_gpu_lstm_varlen import I, PARAMS, make_inputs

pytestmark = pytest.mark.gpu

BPARAMS = PARAMS + tuple(p + "_reverse" for p in PARAMS)
KEYS = ("out", "h_n", "c_n", "dx", "dh0", "dc0") + BPARAMS
MODES = {"fixed": (False, False), "lengths": (False, True), "state": (True, False), "state-lengths": (True, True)}


def make_bilstm(H, dev, kernel=0, seed=0):
    from xcp.lstm import LSTM
    torch.manual_seed(seed)
    lstm = LSTM(I, H, 1, batch_first=True, bidirectional=True).to(dev)
    lstm.xcp_kernel = kernel
    return lstm


def make_bi_inputs(B, T, H, lens, seed=0):
    """x [B,T,I] (padded rows zero) and the cotangents of out [B,T,2H] (1e6 garbage on its padded rows), h_n and
    c_n [2,B,H]: the one-direction generator of test_gpu_lstm_varlen.py, drawn once per direction"""
    x, r0, rh0, rc0 = make_inputs(B, T, H, lens, seed=seed)
    _, r1, rh1, rc1 = make_inputs(B, T, H, lens, seed=seed + 50)
    return x, torch.cat((r0, r1), 2), torch.cat((rh0, rh1), 0), torch.cat((rc0, rc1), 0)


def make_bi_state(B, H, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randn((2, B, H), generator=g), torch.randn((2, B, H), generator=g)


def run_xcp(lstm, x, cot, dev, hx=None, lengths=None, packed=False):
    """out, h_n, c_n, dx, dh0, dc0 and the eight parameter gradients of one forward + backward on the GPU"""
    r, rh, rc = (None if t is None else t.to(dev) for t in cot)
    xg = x.to(dev).requires_grad_(True)
    hxg = None if hx is None else tuple(t.to(dev).requires_grad_(True) for t in hx)
    for p in lstm.parameters():
        p.grad = None
    res = {}
    if packed:
        o, (h, c) = lstm(pack_padded_sequence(xg, lengths, batch_first=True, enforce_sorted=False), hxg)
        res["packed"] = o
        o, _ = pad_packed_sequence(o, batch_first=True, total_length=x.shape[1])
    else:
        o, (h, c) = lstm(xg, hxg, lengths=lengths)
    outs = [(t, g) for t, g in ((o, r), (h, rh), (c, rc)) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    torch.cuda.synchronize()
    res.update(out=o.detach().cpu(), h_n=h.detach().cpu(), c_n=c.detach().cpu(), dx=xg.grad.cpu())
    if hx is not None:
        res["dh0"], res["dc0"] = hxg[0].grad.cpu(), hxg[1].grad.cpu()
    for n in BPARAMS:
        res[n] = getattr(lstm, n).grad.cpu()
    return res


def run_ref(state_dict, H, x, cot, lens, hx):
    """The same through nn.LSTM(bidirectional=True) on the CPU, packed input (lens None: every clip has T frames)"""
    B, T = x.shape[:2]
    ref = nn.LSTM(I, H, 1, batch_first=True, bidirectional=True)
    ref.load_state_dict(state_dict)
    xc = x.clone().requires_grad_(True)
    hxc = None if hx is None else tuple(t.clone().requires_grad_(True) for t in hx)
    lens = [T] * B if lens is None else lens
    pk = pack_padded_sequence(xc, torch.as_tensor(lens, dtype=torch.int64), batch_first=True, enforce_sorted=False)
    po, (h, c) = ref(pk, hxc)
    o, _ = pad_packed_sequence(po, batch_first=True, total_length=T)
    outs = [(t, g) for t, g in zip((o, h, c), cot) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    res = {"out": o.detach(), "h_n": h.detach(), "c_n": c.detach(), "dx": xc.grad, "packed": po}
    if hx is not None:
        res["dh0"], res["dc0"] = hxc[0].grad, hxc[1].grad
    for n in BPARAMS:
        res[n] = getattr(ref, n).grad
    return res


def cpu_state_dict(lstm):
    return {k: v.detach().cpu() for k, v in lstm.state_dict().items()}


@functools.lru_cache(maxsize=None)
def family_reference(case, mode):
    """inputs and the CPU reference of one (family, mode), computed once and never modified (the module's
    weights are a function of the seed, so they are made here on the CPU)"""
    H, B, T, _ = FAMILIES[case]
    state, varlen = MODES[mode]
    lens = cyc(B, T) if varlen else None
    x, *cot = make_bi_inputs(B, T, H, lens or [T] * B)
    hx = make_bi_state(B, H) if state else None
    sd = cpu_state_dict(make_bilstm(H, "cpu"))
    return x, cot, lens, hx, run_ref(sd, H, x, cot, lens, hx)


def assert_close(got, ref, keys=KEYS):
    for k in keys:
        if k not in ref:
            continue
        tol = dict(rtol=1e-4, atol=1e-5) if k in ("out", "h_n", "c_n") else dict(rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), err_msg=k, **tol)


def assert_identical(a, b, keys):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(FAMILIES))
def test_parity_by_kernel_family(gpu, case, mode):
    """Every direction-aware kernel family, fixed / lengths / state / state + lengths (1 and T both occur among
    the lengths); out (both halves) and dx are exactly zero past each clip's length."""
    H, B, T, kernel = FAMILIES[case]
    x, cot, lens, hx, ref = family_reference(case, mode)
    lstm = make_bilstm(H, gpu, kernel)
    got = run_xcp(lstm, x, cot, gpu, hx, lengths=None if lens is None else torch.tensor(lens))
    assert got["out"].shape == (B, T, 2 * H) and got["h_n"].shape == (2, B, H) and got["c_n"].shape == (2, B, H)
    for b, L in enumerate(lens or []):
        assert not got["out"][b, L:].any() and not got["dx"][b, L:].any(), b
    assert_close(got, ref)


@pytest.mark.parametrize("state", [False, True], ids=["nostate", "state"])
def test_packed_sequence(gpu, state):
    """lstm(PackedSequence[, hx]), unsorted lengths: the data is packed like the CPU module's, hx and h_n / c_n
    are in the caller's batch order."""
    H, B, T, lens = 128, 4, 6, [2, 6, 1, 4]
    lstm = make_bilstm(H, gpu)
    x, *cot = make_bi_inputs(B, T, H, lens)
    hx = make_bi_state(B, H, seed=5) if state else None
    got = run_xcp(lstm, x, cot, gpu, hx, lengths=torch.tensor(lens), packed=True)
    ref = run_ref(cpu_state_dict(lstm), H, x, cot, lens, hx)
    pg, pr = got["packed"], ref["packed"]
    assert isinstance(pg, PackedSequence)
    assert torch.equal(pg.batch_sizes, pr.batch_sizes)
    assert torch.equal(pg.sorted_indices.cpu(), pr.sorted_indices)
    assert torch.equal(pg.unsorted_indices.cpu(), pr.unsorted_indices)
    np.testing.assert_allclose(pg.data.detach().cpu().numpy(), pr.data.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert_close(got, ref)


# ------------------------------------------------------------------ exact pins at the kernel (ops) level
def _weights(H, D, gpu, seed=7):
    g = torch.Generator().manual_seed(seed)
    k = H ** -0.5
    whh = ((torch.rand((D, 4 * H, H), generator=g) * 2 - 1) * k).to(gpu)
    bih, bhh = (((torch.rand((D, 4 * H), generator=g) * 2 - 1) * k).to(gpu) for _ in range(2))
    return whh, bih, bhh


def _dir_fwd(xproj, whh, bih, bhh, lens, kernel, dirs, h0=None, c0=None):
    """xproj [D, B, T, 4H]; every saved tensor starts as zeros, so rows no kernel writes compare equal"""
    from xcp import ops
    D, B, T, G4 = xproj.shape
    H = G4 // 4
    dev = xproj.device
    whhT = whh.transpose(1, 2).contiguous() if ops.lstm_dir_needs_whhT(B, H, kernel) else None
    out = torch.zeros(B, T, D * H, device=dev)
    hprev, cst = torch.zeros(D, B, T, H, device=dev), torch.zeros(D, B, T, H, device=dev)
    gates = torch.zeros(D, B * T, G4, device=dev)
    hn, cn = torch.empty(D, B, H, device=dev), torch.empty(D, B, H, device=dev)
    ops.lstm_fwd_dir(xproj.view(D, B * T, G4), whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, B, T, H, dirs, kernel,
                     lens, h0, c0)
    return dict(out=out, hprev=hprev, cst=cst, gates=gates, hn=hn, cn=cn)


def _dir_bwd(dout, dhn, dcn, whh, saved, lens, kernel, dirs, c0=None, state=False):
    from xcp import ops
    D, B, T, H = saved["cst"].shape
    dev = dout.device
    dgates = torch.empty(D, B * T, 4 * H, device=dev)
    dh0 = torch.empty(D, B, H, device=dev) if state else None
    dc0 = torch.empty(D, B, H, device=dev) if state else None
    ops.lstm_bwd_dir(dout, dhn, dcn, whh, saved["cst"], saved["gates"], dgates, B, T, H, dirs, kernel, lens, c0=c0,
                     dh0=dh0, dc0=dc0)
    return dgates.view(D, B, T, 4 * H), dh0, dc0


@pytest.mark.parametrize("case", list(FAMILIES))
def test_direction_0_is_the_old_kernel_bitwise(gpu, case):
    """out[..., :H], h_n[0], c_n[0] and the forward direction's parameter gradients of xcp::lstm_bidir equal
    xcp::lstm_varlen's at full lengths bit for bit, the cotangent confined to direction 0's outputs
    (lstm_varlen never takes the persistent kernels, so H 256 / 512 compare like with like).  Then the same with
    dirs = 1 through ops: out, h_n, c_n, the saved state and dgates."""
    H, B, T, kernel = FAMILIES[case]
    lstm = make_bilstm(H, gpu, kernel)
    x, r, rh, rc = make_bi_inputs(B, T, H, [T] * B)
    r[..., H:], rh[1], rc[1] = 0, 0, 0
    full = torch.full((B,), T, dtype=torch.int32, device=gpu)
    fw = [getattr(lstm, n) for n in PARAMS]

    xg = x.to(gpu).requires_grad_(True)
    o, h, c, *_ = torch.ops.xcp.lstm_bidir(xg, *fw, *(getattr(lstm, n) for n in BPARAMS[4:]), None, None, full, kernel)
    g2 = torch.autograd.grad([o, h, c], [xg] + fw, [r.to(gpu), rh.to(gpu), rc.to(gpu)])
    xo = x.to(gpu).requires_grad_(True)
    o1, h1, c1, *_ = torch.ops.xcp.lstm_varlen(xo, *fw, full, kernel)
    g1 = torch.autograd.grad([o1, h1, c1], [xo] + fw, [r[..., :H].contiguous().to(gpu), rh[:1].to(gpu), rc[:1].to(gpu)])
    torch.cuda.synchronize()
    assert torch.equal(o[..., :H], o1) and torch.equal(h[0], h1[0]) and torch.equal(c[0], c1[0])
    for n, a, b in zip(PARAMS, g2[1:], g1[1:]):
        assert torch.equal(a, b), n

    from xcp import ops
    g = torch.Generator().manual_seed(11)
    xproj = torch.randn((1, B, T, 4 * H), generator=g).to(gpu)
    whh, bih, bhh = _weights(H, 1, gpu)
    dout = torch.randn((B, T, H), generator=g).to(gpu)
    dhn, dcn = (torch.randn((1, B, H), generator=g).to(gpu) for _ in range(2))
    new = _dir_fwd(xproj, whh, bih, bhh, full, kernel, 1)
    ndg, _, _ = _dir_bwd(dout, dhn, dcn, whh, new, full, kernel, 1)
    whhT = whh[0].t().contiguous() if ops.lstm_needs_whhT(B, H, kernel, full) else None
    old = {k: torch.zeros_like(v[0] if k in ("hprev", "cst", "gates") else v) for k, v in new.items()}
    ops.lstm_fwd(xproj[0], whh[0], whhT, bih[0], bhh[0], old["out"], old["hprev"], old["cst"], old["gates"], old["hn"],
                 old["cn"], B, T, H, kernel, full)
    odg = torch.empty(B, T, 4 * H, device=gpu)
    ops.lstm_bwd(dout, dhn, dcn, whh[0], old["cst"], old["gates"], odg, B, T, H, kernel, full)
    torch.cuda.synchronize()
    for k in ("out", "hn", "cn"):
        assert torch.equal(new[k], old[k]), k
    for k in ("hprev", "cst", "gates"):
        assert torch.equal(new[k][0], old[k]), k
    assert torch.equal(ndg[0], odg)


def _mirror(t, lens_l):
    """t [B, T, ...] with each clip's first L rows reversed in time (rows past L stay)"""
    B, T = t.shape[:2]
    idx = torch.arange(T).repeat(B, 1)
    for b, L in enumerate(lens_l):
        idx[b, :L] = torch.arange(L - 1, -1, -1)
    return t[torch.arange(B)[:, None], idx.to(t.device)].contiguous()


@pytest.mark.parametrize("varlen", [False, True], ids=["fixed", "varlen"])
@pytest.mark.parametrize("case", list(FAMILIES))
def test_reverse_is_the_forward_kernel_on_mirrored_time_bitwise(gpu, case, varlen):
    """dirs = 2 on a seeded xproj, state and lengths against dirs = 1 on xproj mirrored inside each clip's length,
    same weights: out, cst and gates are identical after mirroring back, hn / cn identical; the two backward
    calls' dgates (mirrored back), dh0 and dc0 identical.  The device lengths include 1, T and 0."""
    H, B, T, kernel = FAMILIES[case]
    g = torch.Generator().manual_seed(13)
    xproj = torch.randn((1, B, T, 4 * H), generator=g).to(gpu)
    whh, bih, bhh = _weights(H, 1, gpu)
    h0, c0 = (torch.randn((1, B, H), generator=g).to(gpu) for _ in range(2))
    dout = torch.randn((B, T, H), generator=g).to(gpu)
    dhn, dcn = (torch.randn((1, B, H), generator=g).to(gpu) for _ in range(2))
    lens_l = [T] * B
    if varlen:
        lens_l = cyc(B, T)
        lens_l[1] = 0
        assert 0 in lens_l and 1 in lens_l and T in lens_l
    lens = torch.tensor(lens_l, dtype=torch.int32, device=gpu) if varlen else None

    rev = _dir_fwd(xproj, whh, bih, bhh, lens, kernel, 2, h0, c0)
    rdg, rdh0, rdc0 = _dir_bwd(dout, dhn, dcn, whh, rev, lens, kernel, 2, c0=c0, state=True)
    fwd = _dir_fwd(_mirror(xproj[0], lens_l)[None], whh, bih, bhh, lens, kernel, 1, h0, c0)
    fdg, fdh0, fdc0 = _dir_bwd(_mirror(dout, lens_l), dhn, dcn, whh, fwd, lens, kernel, 1, c0=c0, state=True)
    torch.cuda.synchronize()
    assert torch.equal(rev["out"], _mirror(fwd["out"], lens_l))
    for k in ("cst", "hprev"):
        assert torch.equal(rev[k][0], _mirror(fwd[k][0], lens_l)), k
    assert torch.equal(rev["gates"].view(B, T, -1), _mirror(fwd["gates"].view(B, T, -1), lens_l))
    assert torch.equal(rev["hn"], fwd["hn"]) and torch.equal(rev["cn"], fwd["cn"])
    assert torch.equal(rdg[0], _mirror(fdg[0], lens_l))
    assert torch.equal(rdh0, fdh0) and torch.equal(rdc0, fdc0)
    assert rev["out"].any() and rdg.any() and rdh0.any()


# ------------------------------------------------------------------ edges
@functools.lru_cache(maxsize=None)
def single_step_reference(case, zero_x):
    H, B, _, _ = FAMILIES[case]
    x, *cot = make_bi_inputs(B, 1, H, [1] * B)
    if zero_x:
        x = torch.zeros_like(x)
    hx = make_bi_state(B, H, seed=1 + zero_x)
    return x, cot, hx, run_ref(cpu_state_dict(make_bilstm(H, "cpu")), H, x, cot, None, hx)


@pytest.mark.parametrize("case", list(FAMILIES))
def test_single_step(gpu, case):
    """T = 1: both directions meet the state, dh_n / dc_n and dh0 / dc0 in one step."""
    H, B, _, kernel = FAMILIES[case]
    x, cot, hx, ref = single_step_reference(case, False)
    assert_close(run_xcp(make_bilstm(H, gpu, kernel), x, cot, gpu, hx), ref)


@pytest.mark.parametrize("case", list(FAMILIES))
def test_reverse_recurrent_weight_gradient_sees_the_state(gpu, case):
    """x = 0, T = 1, state given: dW_hh_reverse = dgates_r^T h0[1] and nothing else -- a kernel that leaves the
    saved hprev row at L - 1 zero passes every forward check and fails here."""
    H, B, _, kernel = FAMILIES[case]
    x, cot, hx, ref = single_step_reference(case, True)
    got = run_xcp(make_bilstm(H, gpu, kernel), x, cot, gpu, hx)
    assert float(ref["weight_hh_l0_reverse"].abs().max()) > 1e-3
    assert_close(got, ref, keys=("weight_hh_l0_reverse", "weight_hh_l0", "h_n", "c_n", "dh0", "dc0"))


@pytest.mark.parametrize("H", [64, 128, 256, 96])
def test_empty_clip_hands_the_state_on_in_both_directions(gpu, H):
    """Device lengths containing 0: that clip's h_n == h0, c_n == c0, dh0 == dh_n, dc0 == dc_n exactly, in both
    directions; its rows of out and dx are zero and nothing of it reaches the parameter gradients (the CPU
    reference runs without that clip)."""
    B, T, lens = 4, 5, [3, 0, 5, 1]
    lstm = make_bilstm(H, gpu)
    x, r, rh, rc = make_bi_inputs(B, T, H, lens)
    h0, c0 = make_bi_state(B, H, seed=3)
    got = run_xcp(lstm, x, (r, rh, rc), gpu, (h0, c0), lengths=torch.tensor(lens, dtype=torch.int32, device=gpu))
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    assert torch.equal(got["h_n"][:, 1], h0[:, 1]) and torch.equal(got["c_n"][:, 1], c0[:, 1])
    assert torch.equal(got["dh0"][:, 1], rh[:, 1]) and torch.equal(got["dc0"][:, 1], rc[:, 1])
    assert not got["out"][1].any() and not got["dx"][1].any()
    keep = [0, 2, 3]
    ref = run_ref(cpu_state_dict(lstm), H, x[keep], (r[keep], rh[:, keep], rc[:, keep]), [lens[b] for b in keep],
                  (h0[:, keep], c0[:, keep]))
    sub = {k: (v[keep] if k in ("out", "dx") else v[:, keep] if k in ("h_n", "c_n", "dh0", "dc0") else v)
           for k, v in got.items()}
    assert_close(sub, ref)


@pytest.mark.parametrize("case", list(FAMILIES))
def test_zero_state_is_no_state_and_full_lengths_are_no_lengths_bitwise(gpu, case):
    """hx = zeros is bit-identical to hx = None, and lengths = [T] * B to no lengths, in out, h_n, c_n, dx and the
    eight parameter gradients: the four instantiations of a family's direction-aware kernel are one body."""
    H, B, T, kernel = FAMILIES[case]
    lstm = make_bilstm(H, gpu, kernel)
    x, *cot = make_bi_inputs(B, T, H, [T] * B)
    keys = ("out", "h_n", "c_n", "dx") + BPARAMS
    none = run_xcp(lstm, x, cot, gpu)
    zero = run_xcp(lstm, x, cot, gpu, (torch.zeros(2, B, H), torch.zeros(2, B, H)))
    assert_identical(zero, none, keys)
    full = run_xcp(lstm, x, cot, gpu, lengths=torch.full((B,), T, dtype=torch.int32, device=gpu))
    assert_identical(full, none, keys)


def test_entries_refuse_a_bad_mask_and_half_a_state(gpu):
    """XCP_EINVAL (1001) from the C entries themselves, before any launch: a mask outside 1..3, and h0 without c0."""
    from xcp import ops
    t = torch.zeros(2, 2, 64, device=gpu)
    for dirs in (0, 4):
        with pytest.raises(ops._lib.XcpError, match="xcp_lstm_fwd_dir failed with status 1001"):
            ops._lib.call("xcp_lstm_fwd_dir", *([0] * 14), 2, 3, 64, 0, dirs, 0)
        with pytest.raises(ops._lib.XcpError, match="xcp_lstm_bwd_dir failed with status 1001"):
            ops._lib.call("xcp_lstm_bwd_dir", *([0] * 12), 2, 3, 64, 0, dirs, 0)
    half = [0] * 14
    half[5] = t.data_ptr()   # h0 without c0
    with pytest.raises(ops._lib.XcpError, match="xcp_lstm_fwd_dir failed with status 1001"):
        ops._lib.call("xcp_lstm_fwd_dir", *half, 2, 3, 64, 0, 3, 0)


def test_captured_replay_equals_eager_bitwise(gpu):
    """forward + backward with device lengths captured in a graph: the replay (after the lengths changed in
    place) equals the eager run bit for bit -- nothing in the call reads the lengths on the host."""
    H, B, T = 128, 4, 6
    lstm = make_bilstm(H, gpu)
    params = [getattr(lstm, n) for n in BPARAMS]
    x, *cot = make_bi_inputs(B, T, H, [T] * B)
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
    assert not replayed[0][0, 3:].any() and replayed[0][0, :3, :H].any() and replayed[0][0, :3, H:].any()


def test_model_forward_and_gradients(gpu):
    """XceptionLSTMV(64, bidirectional=True).forward(features, seq_lengths) on seeded [3,5,2048] features against
    the same head on the CPU reference LSTM; gradients reach all eight LSTM parameters."""
    from Models.XceptionLSTMV import XceptionLSTMV
    torch.manual_seed(0)
    m = XceptionLSTMV(64, pretrained=False, bidirectional=True).eval()
    ref_lstm = nn.LSTM(2048, 64, 1, batch_first=True, bidirectional=True)
    ref_lstm.load_state_dict(m.lstm.state_dict())
    g = torch.Generator().manual_seed(21)
    feats = torch.randn((3, 5, 2048), generator=g)
    lens = torch.tensor([5, 2, 1])
    feats[1, 2:], feats[2, 1:] = 0, 0
    with torch.no_grad():
        pk = pack_padded_sequence(feats, lens, batch_first=True, enforce_sorted=False)
        _, (h, _) = ref_lstm(pk)
        want = m.sigmoid(m.fc_out(m.fc_layers(torch.cat((h[0], h[1]), 1))))
    m = m.to(gpu)
    prob = m(feats.to(gpu), lens)
    prob.sum().backward()
    torch.cuda.synchronize()
    assert prob.shape == (3, 1)
    np.testing.assert_allclose(prob.detach().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
    for n in BPARAMS:
        gr = getattr(m.lstm, n).grad
        assert gr is not None and torch.isfinite(gr).all() and gr.any(), n
