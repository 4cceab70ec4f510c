"""FusedAdamClip's AdamW / GradScaler bookkeeping and FusedAveragedModel's errors (CPU, no kernel runs).

As tests/test_optim_counters.py: ``_lib.call`` is replaced by a numpy restatement of csrc/optim.hip's
entry points (the chunk table rows are host addresses on the CPU), the AMP ones included -- decoupled
decay, the gradient scale and the found_inf flag -- so what is tested is the host side: which entry
point a configuration calls and with what, and that a step GradScaler's ``found_inf`` skips leaves every
parameter's step count where it was.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

AMP_ENTRY_POINTS = {"xcp_opt_sumsq_amp", "xcp_opt_adam_amp", "xcp_opt_adam_amp_dev", "xcp_opt_average"}


def _arr(ptr, n, ct=ctypes.c_float):
    return np.ctypeslib.as_array((ct * n).from_address(ptr))


def _rows(tab, n, w=6):
    return np.ctypeslib.as_array((ctypes.c_longlong * (w * n)).from_address(tab)).reshape(n, w)


def _adam(rows, c, lr, b1, b2, eps, wd, pmul, bc1, bc2):
    f = np.float32
    for p, g, m, v, o, L in rows:
        P, G, M, V = (_arr(int(a) + 4 * int(o), int(L)) for a in (p, g, m, v))
        pv = P * f(pmul)
        gi = G * f(c) + f(wd) * pv
        M[:] = f(b1) * M + f(1 - b1) * gi
        V[:] = f(b2) * V + f(1 - b2) * gi * gi
        P[:] = pv - f(lr) / f(bc1) * M / (np.sqrt(V) / f(bc2) + f(eps))


@pytest.fixture
def fake_opt(monkeypatch):
    from xcp import _lib, ops
    calls = []

    def sumsq(tab, n, max_norm, scale, out):
        t = 0.0
        for p, g, m, v, o, L in _rows(tab, n):
            t += float((_arr(int(g) + 4 * int(o), int(L)).astype(np.float64) ** 2).sum())
        inv = np.float32(1.0) / _arr(scale, 1)[0] if scale else np.float32(1.0)
        norm = np.float32(np.sqrt(t)) * inv
        coef = min(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6))) if max_norm > 0 else np.float32(1)
        o = _arr(out, 2)
        o[0], o[1] = coef * inv, norm

    def fake_call(name, *args):
        calls.append((name, args))
        if name == "xcp_opt_sumsq":
            tab, n, part, max_norm, out, _ = args
            sumsq(tab, n, max_norm, 0, out)
        elif name == "xcp_opt_sumsq_amp":
            tab, n, part, max_norm, scale, out, _ = args
            sumsq(tab, n, max_norm, scale, out)
        elif name == "xcp_opt_adam_dev":
            tab, n, coef, lr, b1, b2, eps, wd, tdev, _ = args
            t = float(_arr(tdev, 1)[0])
            _adam(_rows(tab, n), _arr(coef, 1)[0] if coef else 1.0, lr, b1, b2, eps, wd, 1.0, 1.0 - b1 ** t,
                  np.sqrt(1.0 - b2 ** t))
        elif name in ("xcp_opt_adam_amp_dev", "xcp_opt_adam_amp"):
            if name == "xcp_opt_adam_amp_dev":
                tab, n, coef, lr, b1, b2, eps, wd, pmul, tdev, gscale, found_inf, _ = args
                t = float(_arr(tdev, 1)[0])
                bc1, bc2 = 1.0 - b1 ** t, np.sqrt(1.0 - b2 ** t)
            else:
                tab, n, coef, lr, b1, b2, eps, wd, pmul, bc1, bc2, gscale, found_inf, _ = args
            if found_inf and _arr(found_inf, 1)[0] != 0:
                return 0
            c = _arr(coef, 1)[0] if coef else (np.float32(1.0) / _arr(gscale, 1)[0] if gscale else 1.0)
            _adam(_rows(tab, n), c, lr, b1, b2, eps, wd, pmul, bc1, bc2)
        else:
            raise AssertionError(name)
        return 0

    class _S:
        cuda_stream = 0

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(ops, "check_gpu", lambda *a: None)
    monkeypatch.setattr(ops, "device_guard", lambda t: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _S())
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    return calls


def _make(shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    init = [torch.randn(s, generator=gen) for s in shapes]
    return [t.clone().requires_grad_(True) for t in init], [t.clone().requires_grad_(True) for t in init], gen


def test_attribute_contract():
    """GradScaler hands grad_scale / found_inf over exactly when the step counts live on the device"""
    from xcp import ops
    from xcp.optim import FusedAdamClip
    mp = pytest.MonkeyPatch()
    mp.setattr(ops, "check_gpu", lambda *a: None)
    try:
        p = [torch.zeros(3, requires_grad=True)]
        assert FusedAdamClip(p, capturable=True)._step_supports_amp_scaling is True
        assert not getattr(FusedAdamClip(p), "_step_supports_amp_scaling", False)
        assert not getattr(FusedAdamClip(p, decoupled_weight_decay=True), "_step_supports_amp_scaling", False)
        assert FusedAdamClip(p, decoupled_weight_decay=True).param_groups[0]["decoupled_weight_decay"] is True
        assert FusedAdamClip(p).param_groups[0]["decoupled_weight_decay"] is False
    finally:
        mp.undo()


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_unchanged_calls_without_amp(fake_opt, max_norm):
    """L2 decay with nothing attached: the entry points and argument lists of before, none of the new ones"""
    from xcp.optim import FusedAdamClip
    shapes = [(10,), (4, 4)]
    pa, pb, gen = _make(shapes, 1)
    opt = FusedAdamClip(pb, lr=1e-3, weight_decay=1e-4, max_norm=max_norm, capturable=True)
    for _ in range(2):
        for q in pb:
            q.grad = torch.randn(q.shape, generator=gen)
        opt.step()
    names = [n for n, _ in fake_opt]
    assert not AMP_ENTRY_POINTS & set(names)
    assert names == (["xcp_opt_sumsq", "xcp_opt_adam_dev"] if max_norm else ["xcp_opt_adam_dev"]) * 2
    for n, a in fake_opt:
        assert len(a) == (10 if n == "xcp_opt_adam_dev" else 6)
    assert float(opt.last_step_skipped) == 0.0


@pytest.mark.parametrize("capturable", [False, True])
def test_decoupled_matches_adamw(fake_opt, capturable):
    from xcp.optim import FusedAdamClip
    shapes = [(37, 5), (64,)]
    pa, pb, gen = _make(shapes, 2)
    ref = torch.optim.AdamW(pa, lr=1e-2, weight_decay=1e-2)
    opt = FusedAdamClip(pb, lr=1e-2, weight_decay=1e-2, decoupled_weight_decay=True, capturable=capturable)
    for _ in range(3):
        for p, q in zip(pa, pb):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        ref.step()
        opt.step()
    assert {n for n, _ in fake_opt} == {"xcp_opt_adam_amp_dev" if capturable else "xcp_opt_adam_amp"}
    for p, q in zip(pa, pb):
        torch.testing.assert_close(q, p, rtol=2e-6, atol=2e-7)


def test_skipped_step_keeps_every_count(fake_opt):
    """found_inf set by hand, as GradScaler.step sets it: the skipped steps (one of them the step on
    which parameter 1 gets its first gradient, one a step parameter 2 sits out, so its counter is split)
    write nothing and advance no count; the steps after match torch.optim.AdamW fed the same gradients
    on the steps that were not skipped"""
    from xcp.optim import FusedAdamClip
    shapes = [(37, 5), (64,), (3, 3, 3)]
    pa, pb, gen = _make(shapes, 3)
    S = 1024.0
    ref = torch.optim.AdamW(pa, lr=1e-2, weight_decay=1e-2)
    opt = FusedAdamClip(pb, lr=1e-2, weight_decay=1e-2, decoupled_weight_decay=True, capturable=True)
    # (skipped, which parameters have a gradient)
    sched = [(False, (0, 2)), (True, (0, 1, 2)), (False, (0, 1, 2)), (True, (0, 1)), (False, (0, 1)), (False, (0, 1, 2))]
    for skipped, have in sched:
        grads = [torch.randn(s, generator=gen) * 1e-2 if i in have else None for i, s in enumerate(shapes)]
        before = [q.detach().clone() for q in pb]
        moments = {i: (opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone())
                   for i, q in enumerate(pb) if opt.state[q]}
        counts = [float(opt.state[q]["step"]) if opt.state[q] else 0.0 for q in pb]
        for q, g in zip(pb, grads):
            q.grad = None if g is None else g * S
        opt.grad_scale, opt.found_inf = torch.tensor(S), torch.tensor(1.0 if skipped else 0.0)
        opt.step()
        del opt.grad_scale, opt.found_inf
        assert float(opt.last_step_skipped) == float(skipped)
        if skipped:
            assert all(torch.equal(q, b) for q, b in zip(pb, before))
            for i, (m, v) in moments.items():
                assert torch.equal(opt.state[pb[i]]["exp_avg"], m) and torch.equal(opt.state[pb[i]]["exp_avg_sq"], v)
            assert [float(opt.state[q]["step"]) if opt.state[q] else 0.0 for q in pb] == counts
            continue
        for p, g in zip(pa, grads):
            p.grad = g
        ref.step()
        for p, q in zip(pa, pb):
            torch.testing.assert_close(q, p, rtol=1e-6, atol=1e-7)
            if p in ref.state and ref.state[p]:
                assert float(opt.state[q]["step"]) == float(ref.state[p]["step"])
    assert [float(opt.state[q]["step"]) for q in pb] == [4.0, 3.0, 3.0]
    assert {n for n, _ in fake_opt} == {"xcp_opt_adam_amp_dev"}


def test_scaled_clip_returns_unscaled_norm(fake_opt):
    """max_norm under a grad_scale: xcp_opt_sumsq_amp gets the scale's pointer, step() returns
    ||g|| / S, and the update equals clip_grad_norm_ + AdamW on the unscaled gradients"""
    from xcp.optim import FusedAdamClip
    shapes = [(50,), (8, 9)]
    pa, pb, gen = _make(shapes, 4)
    S = 2.0 ** 12
    ref = torch.optim.AdamW(pa, lr=1e-2, weight_decay=1e-2)
    opt = FusedAdamClip(pb, lr=1e-2, weight_decay=1e-2, max_norm=0.05, decoupled_weight_decay=True, capturable=True)
    for _ in range(2):
        for p, q in zip(pa, pb):
            p.grad = torch.randn(p.shape, generator=gen) * 1e-2
            q.grad = p.grad * S
        opt.grad_scale, opt.found_inf = torch.tensor(S), torch.tensor(0.0)
        got = opt.step()
        del opt.grad_scale, opt.found_inf
        want = torch.nn.utils.clip_grad_norm_(pa, 0.05)
        ref.step()
        torch.testing.assert_close(got, want, rtol=1e-6, atol=0)
        for p, q in zip(pa, pb):
            torch.testing.assert_close(q, p, rtol=1e-6, atol=1e-7)
    assert [n for n, _ in fake_opt] == ["xcp_opt_sumsq_amp", "xcp_opt_adam_amp_dev"] * 2


def test_unscaled_first_order_passes_no_scale(fake_opt):
    """after scaler.unscale_ GradScaler attaches grad_scale None: the plain sum of squares, found_inf alone"""
    from xcp.optim import FusedAdamClip
    pa, pb, gen = _make([(20,)], 5)
    opt = FusedAdamClip(pb, lr=1e-2, max_norm=1.0, capturable=True)
    pb[0].grad = torch.randn(20, generator=gen)
    opt.grad_scale, opt.found_inf = None, torch.tensor(0.0)
    opt.step()
    assert [n for n, _ in fake_opt] == ["xcp_opt_sumsq", "xcp_opt_adam_amp_dev"]
    args = fake_opt[1][1]
    assert args[10] == 0 and args[11] != 0 and args[8] == 1.0   # no scale, the flag, pmul 1 (L2 decay)


def test_averaged_model_errors():
    from torch.optim.swa_utils import get_ema_multi_avg_fn
    from xcp.optim import FusedAveragedModel
    m = torch.nn.Linear(3, 2)
    with pytest.raises(ValueError, match="avg_fn"):
        FusedAveragedModel(m, avg_fn=lambda a, b, n: a)
    with pytest.raises(ValueError, match="avg_fn"):
        FusedAveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAveragedModel(m)
    with pytest.raises(ValueError, match="decay"):
        FusedAveragedModel(m, decay=1.5)
