"""``xcp.lstm.LSTM`` started from an initial state (lstm.hip's state-aware instantiations) against
``torch.nn.LSTM`` on the CPU in fp32 with weights copied, ``hx`` given and the input packed with
``enforce_sorted=False``.  Input size 64; h0, c0 ~ N(0, 1), seeded.  Tolerances are the project's own
(test_gpu_lstm_varlen.py): out / h_n / c_n rtol 1e-4, atol 1e-5; dx, dh0, dc0 and the parameter gradients
rtol 1e-3, atol 1e-5.  The backward is driven by one seeded cotangent on out, h_n and c_n at once, with 1e6
garbage on the padded rows of out's cotangent.

What a tolerance cannot see is pinned exactly: a zero state equals no state bit for bit, a sequence run in
chunks with the state carried equals the whole run bit for bit at the kernel level (the state crosses the
chunk boundary in fp32 memory either way), and a clip of length 0 hands its state and its state's gradient on
unchanged."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence

from test_gpu_lstm_varlen import I, PARAMS, assert_identical, make_inputs, make_lstm

pytestmark = pytest.mark.gpu

STATE_KEYS = ("out", "h_n", "c_n", "dx", "dh0", "dc0") + PARAMS

FAMILIES = {   # H, B, T, kernel
    "H64": (64, 5, 7, 0),                # register-resident
    "H128": (128, 5, 7, 0),
    "H128-B33": (128, 33, 4, 0),
    "H256-B17": (256, 17, 5, 0),         # per-step, crosses the backward's 16-clip pass
    "H512-B25": (512, 25, 5, 0),         # per-step, the forward's LDS budget edge
    "H256-B32": (256, 32, 5, 0),         # per-step, B = LS_MAXB
    "H1024": (1024, 3, 4, 0),            # per-step, KS = 32
    "H96": (96, 3, 5, 0),                # generic by shape
    "H128-generic": (128, 5, 7, 1),      # the generic pair, pinned
}


def cyc(B, T):
    """lengths cycling 1 + b % T; where B < T the cycle stops short of T, so the last clip is full: 1 and T
    both occur at every shape used here"""
    lens = [1 + b % T for b in range(B)]
    lens[-1] = T
    assert 1 in lens and T in lens
    return lens


def make_state(B, H, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn((1, B, H), generator=g), torch.randn((1, B, H), generator=g)


def run_xcp(lstm, x, cot, dev, hx, lengths=None, packed=False, state_grad=True):
    """out, h_n, c_n, dx, dh0, dc0 and the parameter gradients of one forward + backward on the GPU; cot's out
    entry may be None (only h_n / c_n are used then)."""
    r, rh, rc = (None if t is None else t.to(dev) for t in cot)
    xg = x.to(dev).requires_grad_(True)
    h0, c0 = (None, None) if hx is None else (t.to(dev).requires_grad_(state_grad) for t in hx)
    for p in lstm.parameters():
        p.grad = None
    hxg = None if hx is None else (h0, c0)
    res_packed = None
    if packed:
        o, (h, c) = lstm(pack_padded_sequence(xg, lengths, batch_first=True, enforce_sorted=False), hxg)
        res_packed = o
        o, _ = pad_packed_sequence(o, batch_first=True, total_length=x.shape[1])
    else:
        o, (h, c) = lstm(xg, hxg, lengths=lengths)
    outs = [(t, g) for t, g in ((o, r), (h, rh), (c, rc)) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    torch.cuda.synchronize()
    res = {"out": o.detach().cpu(), "h_n": h.detach().cpu(), "c_n": c.detach().cpu(), "dx": xg.grad.cpu()}
    if hx is not None:
        res["dh0"] = None if h0.grad is None else h0.grad.cpu()
        res["dc0"] = None if c0.grad is None else c0.grad.cpu()
    for n in PARAMS:
        res[n] = getattr(lstm, n).grad.cpu()
    if packed:
        res["packed"] = res_packed
    return res


def run_ref(lstm, x, cot, lens, hx):
    """The same through nn.LSTM on the CPU, hx given, packed input (lens None: every clip has T frames)."""
    H, (B, T) = lstm.hidden_size, x.shape[:2]
    ref = nn.LSTM(I, H, 1, batch_first=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in lstm.state_dict().items()})
    xc = x.clone().requires_grad_(True)
    h0, c0 = (t.clone().requires_grad_(True) for t in hx)
    lens = [T] * B if lens is None else lens
    pk = pack_padded_sequence(xc, torch.as_tensor(lens, dtype=torch.int64), batch_first=True, enforce_sorted=False)
    po, (h, c) = ref(pk, (h0, c0))
    o, _ = pad_packed_sequence(po, batch_first=True, total_length=T)
    outs = [(t, g) for t, g in zip((o, h, c), cot) if g is not None]
    torch.autograd.backward([t for t, _ in outs], [g for _, g in outs])
    res = {"out": o.detach(), "h_n": h.detach(), "c_n": c.detach(), "dx": xc.grad, "dh0": h0.grad, "dc0": c0.grad,
           "packed": po}
    for n in PARAMS:
        res[n] = getattr(ref, n).grad
    return res


def assert_close(got, ref, keys=STATE_KEYS):
    for k in keys:
        tol = dict(rtol=1e-4, atol=1e-5) if k in ("out", "h_n", "c_n") else dict(rtol=1e-3, atol=1e-5)
        np.testing.assert_allclose(got[k].numpy(), ref[k].numpy(), err_msg=k, **tol)


@pytest.mark.parametrize("varlen", [False, True], ids=["fixed", "varlen"])
@pytest.mark.parametrize("case", list(FAMILIES))
def test_parity_by_kernel_family(gpu, case, varlen):
    """Every state-aware kernel family against the CPU nn.LSTM fed hx, with and without lengths (1 and T
    both occur); out and dx are exactly zero past each clip's length."""
    H, B, T, kernel = FAMILIES[case]
    lens = cyc(B, T) if varlen else None
    assert lens is None or (1 in lens and T in lens)
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, T, H, lens or [T] * B)
    hx = make_state(B, H)
    got = run_xcp(lstm, x, cot, gpu, hx, lengths=None if lens is None else torch.tensor(lens))
    ref = run_ref(lstm, x, cot, lens, hx)
    for b, L in enumerate(lens or []):
        assert not got["out"][b, L:].any() and not got["dx"][b, L:].any(), b
    assert_close(got, ref)


@pytest.mark.parametrize("case", list(FAMILIES))
def test_single_step(gpu, case):
    """T = 1: step 0 is also the last step, so c0, dh_n, dc_n and dh0 meet in one step."""
    H, B, _, kernel = FAMILIES[case]
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, 1, H, [1] * B)
    hx = make_state(B, H, seed=1)
    assert_close(run_xcp(lstm, x, cot, gpu, hx), run_ref(lstm, x, cot, None, hx))


@pytest.mark.parametrize("case", list(FAMILIES))
def test_recurrent_weight_gradient_sees_the_state(gpu, case):
    """x = 0, T = 1: dW_hh = dgates^T h0 and nothing else.  A kernel that leaves the saved hprev[:, 0] zero
    passes every forward check and fails here."""
    H, B, _, kernel = FAMILIES[case]
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, 1, H, [1] * B)
    x.zero_()
    hx = make_state(B, H, seed=2)
    got, ref = run_xcp(lstm, x, cot, gpu, hx), run_ref(lstm, x, cot, None, hx)
    assert float(ref["weight_hh_l0"].abs().max()) > 1e-3
    assert_close(got, ref, keys=("weight_hh_l0", "h_n", "c_n", "dh0", "dc0"))


@pytest.mark.parametrize("varlen", [False, True], ids=["fixed", "varlen"])
@pytest.mark.parametrize("case", list(FAMILIES))
def test_zero_state_is_no_state_bitwise(gpu, monkeypatch, case, varlen):
    """hx = zeros is bit-identical to hx=None in out, h_n, c_n, dx and the parameter gradients: the state-aware
    kernels are instantiations of the body the others are.  (XCP_LSTM_PERSIST=0, so that at H 256 / 512 the call
    without a state and without lengths runs the per-step kernels too.)"""
    monkeypatch.setenv("XCP_LSTM_PERSIST", "0")
    H, B, T, kernel = FAMILIES[case]
    lens = torch.tensor(cyc(B, T)) if varlen else None
    lstm = make_lstm(H, gpu, kernel)
    x, *cot = make_inputs(B, T, H, cyc(B, T) if varlen else [T] * B)
    none = run_xcp(lstm, x, cot, gpu, None, lengths=lens)
    zero = run_xcp(lstm, x, cot, gpu, (torch.zeros(1, B, H), torch.zeros(1, B, H)), lengths=lens)
    assert_identical(zero, none)


def _kernel_fwd(xproj, whh, bih, bhh, lens, kernel, h0=None, c0=None):
    from xcp import ops
    B, T, G4 = xproj.shape
    H = G4 // 4
    dev = xproj.device
    whhT = whh.t().contiguous() if ops.lstm_needs_whhT(B, H, kernel, lens, state=h0 is not None) else None
    out, hprev, cst = (torch.zeros(B, T, H, device=dev) for _ in range(3))
    gates = torch.zeros(B, T, G4, device=dev)
    hn, cn = torch.empty(1, B, H, device=dev), torch.empty(1, B, H, device=dev)
    ops.lstm_fwd(xproj, whh, whhT, bih, bhh, out, hprev, cst, gates, hn, cn, B, T, H, kernel, lens, h0, c0)
    return dict(out=out, hprev=hprev, cst=cst, gates=gates, hn=hn, cn=cn)


def _kernel_bwd(dout, dhn, dcn, whh, saved, lens, kernel, c0=None, state=False):
    from xcp import ops
    B, T, H = saved["out"].shape
    dev = dout.device
    dgates = torch.empty(B, T, 4 * H, device=dev)
    dh0 = torch.empty(1, B, H, device=dev) if state else None
    dc0 = torch.empty(1, B, H, device=dev) if state else None
    ops.lstm_bwd(dout, dhn, dcn, whh, saved["cst"], saved["gates"], dgates, B, T, H, kernel, lens, c0=c0, dh0=dh0,
                 dc0=dc0)
    return dgates, dh0, dc0


@pytest.mark.parametrize("case", list(FAMILIES))
def test_chunked_equals_whole_bitwise_at_the_kernel_level(gpu, case):
    """One x-projection; the recurrence once whole with lengths and once in chunks of 3, 3 and 1 steps over
    contiguous copies of its slices, h_n / c_n carried into h0 / c0 and the chunk lengths clamp(L - off, 0, C):
    out, the final h_n / c_n and the saved cst on live rows are equal bit for bit.  Then the backward the same
    way, last chunk first, dh0 / dc0 fed back as dhn / dcn: dgates is equal bit for bit."""
    H, B, _, kernel = FAMILIES[case]
    T, chunks = 7, (3, 3, 1)
    g = torch.Generator().manual_seed(7)
    xproj = torch.randn((B, T, 4 * H), generator=g).to(gpu)
    k = H ** -0.5
    whh = ((torch.rand((4 * H, H), generator=g) * 2 - 1) * k).to(gpu)
    bih, bhh = (((torch.rand((4 * H,), generator=g) * 2 - 1) * k).to(gpu) for _ in range(2))
    dout = torch.randn((B, T, H), generator=g).to(gpu)
    dhn, dcn = (torch.randn((1, B, H), generator=g).to(gpu) for _ in range(2))
    lens_l = cyc(B, T)
    lens = torch.tensor(lens_l, dtype=torch.int32, device=gpu)
    whole = _kernel_fwd(xproj, whh, bih, bhh, lens, kernel)
    wdg, _, _ = _kernel_bwd(dout, dhn, dcn, whh, whole, lens, kernel)

    h, c = torch.zeros(1, B, H, device=gpu), torch.zeros(1, B, H, device=gpu)
    parts, off = [], 0
    for C in chunks:
        cl = (lens - off).clamp(0, C)
        saved = _kernel_fwd(xproj[:, off:off + C].contiguous(), whh, bih, bhh, cl, kernel, h, c)
        parts.append((off, C, cl, c, saved))
        h, c = saved["hn"], saved["cn"]
        off += C
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p[4]["out"] for p in parts], 1), whole["out"])
    assert torch.equal(h, whole["hn"]) and torch.equal(c, whole["cn"])
    live = (torch.arange(T, device=gpu)[None, :] < lens[:, None])[..., None]
    ccst = torch.cat([p[4]["cst"] for p in parts], 1)
    assert torch.equal(torch.where(live, ccst, 0.0), torch.where(live, whole["cst"], 0.0))

    gh, gc, cdg = dhn, dcn, []
    for off, C, cl, c0, saved in reversed(parts):
        dg, gh, gc = _kernel_bwd(dout[:, off:off + C].contiguous(), gh, gc, whh, saved, cl, kernel, c0=c0, state=True)
        cdg.insert(0, dg)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(cdg, 1), wdg)


@pytest.mark.parametrize("H", [64, 128, 256, 96])
def test_empty_chunk_hands_the_state_on(gpu, H):
    """A clip of length 0 (device int32 lengths): h_n == h0, c_n == c0, dh0 == dh_n, dc0 == dc_n exactly, zero
    out / dx, and nothing of it in the parameter gradients (the CPU reference runs without that clip)."""
    B, T, lens = 4, 5, [3, 0, 5, 1]
    lstm = make_lstm(H, gpu)
    x, r, rh, rc = make_inputs(B, T, H, lens)
    h0, c0 = make_state(B, H, seed=3)
    got = run_xcp(lstm, x, (r, rh, rc), gpu, (h0, c0), lengths=torch.tensor(lens, dtype=torch.int32, device=gpu))
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    assert torch.equal(got["h_n"][0, 1], h0[0, 1]) and torch.equal(got["c_n"][0, 1], c0[0, 1])
    assert torch.equal(got["dh0"][0, 1], rh[0, 1]) and torch.equal(got["dc0"][0, 1], rc[0, 1])
    assert not got["out"][1].any() and not got["dx"][1].any()
    keep = [0, 2, 3]
    ref = run_ref(lstm, x[keep], (r[keep], rh[:, keep], rc[:, keep]), [lens[b] for b in keep],
                  (h0[:, keep], c0[:, keep]))
    sub = {k: (v[keep] if k in ("out", "dx") else v[:, keep] if k in ("h_n", "c_n", "dh0", "dc0") else v)
           for k, v in got.items()}
    assert_close(sub, ref)
    # only h_n wanted: the absent cotangents pass through as zero
    only = run_xcp(lstm, x, (None, rh, None), gpu, (h0, c0), lengths=torch.tensor(lens, dtype=torch.int32, device=gpu))
    assert torch.equal(only["dh0"][0, 1], rh[0, 1]) and not only["dc0"][0, 1].any()


@pytest.mark.parametrize("H", [128, 256])
def test_autograd_through_the_carried_state(gpu, H):
    """Two module calls, the second's hx being the first's (h_n, c_n) undetached, loss on the second's h_n:
    parameter gradients and dx equal the whole-sequence reference.  With the state detached nothing reaches
    the first chunk."""
    B, T, C = 3, 6, 3
    lstm = make_lstm(H, gpu)
    x, _, rh, _ = make_inputs(B, T, H, [T] * B)
    zero = (torch.zeros(1, B, H), torch.zeros(1, B, H))
    ref = run_ref(lstm, x, (None, rh, None), None, zero)

    def two_calls(detach):
        for p in lstm.parameters():
            p.grad = None
        x1, x2 = (t.contiguous().to(gpu).requires_grad_(True) for t in (x[:, :C], x[:, C:]))
        _, state = lstm(x1)
        if detach:
            state = tuple(s.detach() for s in state)
        _, (h, _) = lstm(x2, state)
        torch.autograd.backward([h], [rh.to(gpu)])
        torch.cuda.synchronize()
        return h.detach().cpu(), x1.grad, x2.grad

    h, g1, g2 = two_calls(False)
    got = {"h_n": h, "dx": torch.cat([g1, g2], 1).cpu(), **{n: getattr(lstm, n).grad.cpu() for n in PARAMS}}
    assert_close(got, ref, keys=("h_n", "dx") + PARAMS)
    _, g1, g2 = two_calls(True)
    assert g1 is None or not g1.any()
    assert g2.any()


def test_no_state_gradient_wanted_and_no_dout(gpu):
    """h0 / c0 that do not require grad get None and change no other gradient (bit for bit); with only h_n
    used the backward gets no dout and still matches the reference."""
    H, B, T = 128, 3, 5
    lstm = make_lstm(H, gpu)
    x, *cot = make_inputs(B, T, H, [T] * B)
    hx = make_state(B, H, seed=4)
    want = run_xcp(lstm, x, cot, gpu, hx)
    none = run_xcp(lstm, x, cot, gpu, hx, state_grad=False)
    assert none["dh0"] is None and none["dc0"] is None
    assert_identical(none, want)
    cot = (None, cot[1], None)
    assert_close(run_xcp(lstm, x, cot, gpu, hx), run_ref(lstm, x, cot, None, hx),
                 keys=("h_n", "dx", "dh0", "dc0") + PARAMS)


def test_packed_sequence_with_state(gpu):
    """lstm(PackedSequence, hx), unsorted lengths: hx and h_n / c_n are in the caller's batch order, the result
    is packed like the CPU module's."""
    H, B, T, lens = 128, 4, 6, [2, 6, 1, 4]
    lstm = make_lstm(H, gpu)
    x, *cot = make_inputs(B, T, H, lens)
    hx = make_state(B, H, seed=5)
    got = run_xcp(lstm, x, cot, gpu, hx, lengths=torch.tensor(lens), packed=True)
    ref = run_ref(lstm, x, cot, lens, hx)
    pg, pr = got["packed"], ref["packed"]
    assert isinstance(pg, PackedSequence)
    assert torch.equal(pg.batch_sizes, pr.batch_sizes)
    assert torch.equal(pg.sorted_indices.cpu(), pr.sorted_indices)
    assert torch.equal(pg.unsorted_indices.cpu(), pr.unsorted_indices)
    np.testing.assert_allclose(pg.data.detach().cpu().numpy(), pr.data.detach().numpy(), rtol=1e-4, atol=1e-5)
    assert_close(got, ref)


def test_opcheck_lstm_state_ops(gpu):
    from xcp import torch_ops  # noqa: F401
    g = torch.Generator(device=gpu).manual_seed(0)
    H, B, T = 64, 2, 3

    def r(*shape):
        return torch.randn(shape, device=gpu, generator=g).requires_grad_(True)

    for lens in (None, torch.tensor([3, 2], dtype=torch.int32, device=gpu)):
        args = (r(B, T, I), r(4 * H, I), r(4 * H, H), r(4 * H), r(4 * H), r(1, B, H), r(1, B, H), lens, 0)
        torch.library.opcheck(torch.ops.xcp.lstm_state, args,
                              test_utils=("test_schema", "test_faketensor", "test_autograd_registration"))
        x, w_ih, w_hh, _, _, _, c0 = (t.detach() for t in args[:7])
        out, hn, cn, hprev, cst, gates = torch.ops.xcp.lstm_state(*(t.detach() if torch.is_tensor(t) else t
                                                                    for t in args))
        for need in ((True, True, True), (False, True, False), (True, False, False)):
            bargs = (torch.randn_like(out), torch.randn_like(hn), None, x, w_ih, w_hh, c0, hprev, cst, gates, lens, 0,
                     *need)
            torch.library.opcheck(torch.ops.xcp.lstm_state_backward, bargs, test_utils=("test_schema", "test_faketensor"))
