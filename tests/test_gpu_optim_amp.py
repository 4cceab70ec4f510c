"""The AMP optimiser tail on the GPU (csrc/optim.hip's xcp_opt_sumsq_amp / xcp_opt_adam_amp /
xcp_opt_adam_amp_dev / xcp_opt_average through xcp.optim and xcp.auface):

* FusedAdamClip(decoupled_weight_decay=True) against clip_grad_norm_ + torch.optim.AdamW;
* under torch.amp.GradScaler a capturable instance unscales inside the kernels -- bit for bit what the
  non-capturable instance computes from gradients GradScaler unscaled -- skips an overflow step on
  the device, and replays the whole AMP step from a HIP graph;
* FusedAveragedModel against torch.optim.swa_utils.AveragedModel;
* AUFaceTrainer(fused_optimizer=True) against the torch tail.

Synthetic tensors of test_fused_adam_clip_vs_torch's shapes (below, at and above one 16384-element chunk,
a tail that is no multiple of 4), gradients of about 1e-2 * randn (nothing subnormal after scaling
or unscaling), and a variant whose ``p.grad`` are views of one flat buffer at odd element offsets (the
GradBuckets pattern: 4-byte alignment only).
"""
import contextlib
import copy

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

SHAPES = [(3,), (128, 129), (16384,), (40000,), (7, 5, 3, 3)]


def _params(gpu, seed, copies=2):
    g = torch.Generator(device=gpu).manual_seed(seed)
    init = [torch.randn(s, device=gpu, generator=g) for s in SHAPES]
    return [[t.clone().requires_grad_(True) for t in init] for _ in range(copies)] + [g]


def _attach_grads(params, flat):
    """zeroed ``p.grad`` for every parameter: separate tensors, or views flat[o:o+n] of one flat fp32
    buffer with every offset o odd"""
    if not flat:
        for p in params:
            p.grad = torch.zeros_like(p)
        return
    offs, o = [], 1
    for p in params:
        offs.append(o)
        o += p.numel()
        o += 1 - (o & 1)
    buf = torch.zeros(o, device=params[0].device)
    for p, o in zip(params, offs):
        assert o % 2 == 1
        p.grad = buf[o:o + p.numel()].view(p.shape)


@contextlib.contextmanager
def _no_host_sync():
    """a host read of device memory (.item(), a blocking copy) inside raises"""
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(prev)


# ---------------------------------------------------------------- 1. AdamW against torch
@pytest.mark.parametrize("flat", [False, True], ids=["own_grads", "flat_odd_offsets"])
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("max_norm", [None, 1.0, 1e-3])
def test_fused_adamw_vs_torch(gpu, max_norm, capturable, flat):
    """three steps of FusedAdamClip(decoupled_weight_decay=True) against clip_grad_norm_ +
    torch.optim.AdamW, at the project's optimiser tolerance (test_fused_adam_clip_vs_torch)"""
    from xcp.optim import FusedAdamClip
    a, b, g = _params(gpu, 11)
    opt_a = FusedAdamClip(a, lr=1e-2, weight_decay=1e-2, max_norm=max_norm, capturable=capturable,
                          decoupled_weight_decay=True)
    opt_b = torch.optim.AdamW(b, lr=1e-2, weight_decay=1e-2)
    _attach_grads(a, flat)
    _attach_grads(b, False)
    for step in range(3):
        for p, q in zip(a, b):
            gr = 1e-2 * torch.randn(p.shape, device=gpu, generator=g)
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        na = opt_a.step()
        if max_norm is not None:
            nb = torch.nn.utils.clip_grad_norm_(b, max_norm)
            torch.testing.assert_close(na, nb, rtol=1e-5, atol=0)
        else:
            assert na is None
        opt_b.step()
        for p, q in zip(a, b):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)
    for p in a:
        assert float(opt_a.state[p]["step"]) == 3.0


@pytest.mark.parametrize("capturable", [False, True])
def test_coupled_decay_still_torch_adam(gpu, capturable):
    """decoupled_weight_decay=False spelled out is the L2 update of before (torch.optim.Adam)"""
    from xcp.optim import FusedAdamClip
    a, b, g = _params(gpu, 12)
    opt_a = FusedAdamClip(a, lr=1e-2, weight_decay=1e-2, max_norm=1.0, capturable=capturable,
                          decoupled_weight_decay=False)
    opt_b = torch.optim.Adam(b, lr=1e-2, weight_decay=1e-2)
    _attach_grads(a, True)
    _attach_grads(b, False)
    for step in range(3):
        for p, q in zip(a, b):
            gr = 1e-2 * torch.randn(p.shape, device=gpu, generator=g)
            p.grad.copy_(gr)
            q.grad.copy_(gr)
        na = opt_a.step()
        torch.testing.assert_close(na, torch.nn.utils.clip_grad_norm_(b, 1.0), rtol=1e-5, atol=0)
        opt_b.step()
        for p, q in zip(a, b):
            torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- the synthetic AMP step
class _AmpRun:
    """loss = sum((p * c).sum()) under a GradScaler; ``order``: "step" (scaler.step alone), "visual"
    (torch clip_grad_norm_ of the SCALED gradients, then scaler.step: train_visual.py's order) or
    "unscale" (scaler.unscale_, [torch clip,] scaler.step: train_au_face.py's order)"""

    def __init__(self, gpu, params, make_opt, order="step", flat=False, torch_clip=None, init_scale=2.0 ** 16):
        self.params, self.order, self.torch_clip = params, order, torch_clip
        self.opt = make_opt(params)
        self.scaler = torch.amp.GradScaler(init_scale=init_scale)
        self.c = [torch.zeros_like(p) for p in params]
        _attach_grads(params, flat)
        self.ret = None

    def set_c(self, cs):
        for c, new in zip(self.c, cs):
            c.copy_(new)

    def step(self):
        self.opt.zero_grad(set_to_none=False)
        loss = sum((p * c).sum() for p, c in zip(self.params, self.c))
        self.scaler.scale(loss).backward()
        if self.order == "unscale":
            self.scaler.unscale_(self.opt)
        if self.torch_clip is not None:
            self.ret = torch.nn.utils.clip_grad_norm_(self.params, self.torch_clip)
        r = self.scaler.step(self.opt)
        if self.torch_clip is None:
            self.ret = r
        self.scaler.update()

    def state(self):
        out = []
        for p in self.params:
            st = self.opt.state[p]
            out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])))
        return out


def _cs(gpu, g, poison=None):
    cs = [1e-2 * torch.randn(s, device=gpu, generator=g) for s in SHAPES]
    if poison is not None:
        cs[3].view(-1)[20001] = poison
    return cs


def _assert_state_equal(a, b):
    for (pa, ma, va, ta), (pb, mb, vb, tb) in zip(a, b):
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and ta == tb


# ---------------------------------------------------------------- 2. in-kernel unscale is exact
@pytest.mark.parametrize("flat", [False, True], ids=["own_grads", "flat_odd_offsets"])
@pytest.mark.parametrize("order,max_norm,torch_clip", [("step", 1.0, None), ("visual", None, 1.0), ("unscale", 1.0, None),
                                                       ("unscale", None, 1.0)],
                         ids=["step_clip_inside", "visual_order", "unscale_first_our_clip", "unscale_first_torch_clip"])
def test_in_kernel_unscale_bitwise(gpu, order, max_norm, torch_clip, flat):
    """the capturable instance (GradScaler hands it grad_scale / found_inf; the kernels unscale) against
    the non-capturable one (GradScaler unscales the gradients in place first): the scale 2^16 is a
    power of two, so multiplying by it and by its reciprocal commutes with every fp32 rounding, and
    parameters, moments and returned norms are bit for bit equal"""
    from xcp.optim import FusedAdamClip
    a, b, g = _params(gpu, 21)
    runs = [_AmpRun(gpu, ps, lambda ps, capt=capt: FusedAdamClip(ps, lr=1e-2, weight_decay=1e-4, max_norm=max_norm,
                                                                capturable=capt), order, flat, torch_clip)
            for ps, capt in ((a, True), (b, False))]
    for step in range(3):
        cs = _cs(gpu, g)
        for r in runs:
            r.set_c(cs)
            r.step()
        assert runs[0].ret is not None and torch.equal(runs[0].ret, runs[1].ret)
        _assert_state_equal(runs[0].state(), runs[1].state())
        assert runs[0].scaler.get_scale() == 2.0 ** 16
    assert all(s[3] == 3.0 for s in runs[0].state())


# ---------------------------------------------------------------- 3. overflow is skipped on the device
def _torch_amp_reference(gpu, params, seq, clip, init_scale=2.0 ** 16):
    """torch.optim.AdamW + GradScaler (unscale_, clip_grad_norm_, step, update) over the same steps"""
    ref = _AmpRun(gpu, params, lambda ps: torch.optim.AdamW(ps, lr=1e-2, weight_decay=1e-2), "unscale", False, clip,
                  init_scale)
    for cs in seq:
        ref.set_c(cs)
        ref.step()
    return ref


@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_overflow_step_skipped_on_device(gpu, monkeypatch, poison):
    """finite, overflowing, finite: the middle step writes nothing (parameters and moments bit for bit,
    step counts still 1, the exposed flag 1, the scale halved) and GradScaler never takes its host
    path.  Step one builds the chunk tables (a host-to-device copy); steps two and three run with
    host synchronisation forbidden."""
    from xcp.optim import FusedAdamClip

    def host_path(*a, **k):
        raise AssertionError("GradScaler._maybe_opt_step (found_inf read on the host) was entered")

    a, b, g = _params(gpu, 31)
    seq = [_cs(gpu, g), _cs(gpu, g, poison), _cs(gpu, g)]
    ref = _torch_amp_reference(gpu, b, seq, 1.0)
    monkeypatch.setattr(torch.amp.GradScaler, "_maybe_opt_step", host_path)
    run = _AmpRun(gpu, a, lambda ps: FusedAdamClip(ps, lr=1e-2, weight_decay=1e-2, max_norm=1.0, capturable=True,
                                                   decoupled_weight_decay=True), "step", True)
    run.set_c(seq[0])
    run.step()
    one = run.state()
    assert float(run.opt.last_step_skipped) == 0.0
    run.set_c(seq[1])
    with _no_host_sync():
        run.step()
    _assert_state_equal(run.state(), one)
    assert all(s[3] == 1.0 for s in run.state())
    assert run.scaler.get_scale() == 2.0 ** 15
    assert float(run.opt.last_step_skipped) == 1.0
    run.set_c(seq[2])
    with _no_host_sync():
        run.step()
    assert float(run.opt.last_step_skipped) == 0.0
    assert all(s[3] == 2.0 for s in run.state()) and ref.scaler.get_scale() == run.scaler.get_scale() == 2.0 ** 15
    for p, q in zip(a, b):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(run.ret, ref.ret, rtol=1e-5, atol=0)


# ---------------------------------------------------------------- 4. the AMP step replays as a graph
def test_amp_step_replays_as_graph(gpu):
    """scaler.scale(loss).backward(); scaler.step(opt); scaler.update() captured after one eager step and
    replayed three times, an inf copied into the static input before the middle replay: bit for bit the
    same optimiser class run eagerly, torch.optim.AdamW + GradScaler at 1e-5 / 1e-6, the skipped replay
    a no-op, step counts 3 (warm-up plus two)"""
    from xcp.optim import FusedAdamClip
    a, b, c, g = _params(gpu, 41, copies=3)
    seq = [_cs(gpu, g), _cs(gpu, g), _cs(gpu, g, float("inf")), _cs(gpu, g)]

    def make(ps):
        return FusedAdamClip(ps, lr=1e-2, weight_decay=1e-2, max_norm=1.0, capturable=True, decoupled_weight_decay=True)

    eager = _AmpRun(gpu, b, make, "step", True)
    for cs in seq:
        eager.set_c(cs)
        eager.step()
    ref = _torch_amp_reference(gpu, c, seq, 1.0)

    run = _AmpRun(gpu, a, make, "step", True)
    run.set_c(seq[0])
    run.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    run.set_c(seq[1])
    with torch.cuda.graph(graph):
        run.step()
    # (capture runs nothing: the state is still the warm-up's)
    assert all(s[3] == 1.0 for s in run.state())
    graph.replay()
    torch.cuda.synchronize()
    after_first = run.state()
    run.set_c(seq[2])
    graph.replay()
    torch.cuda.synchronize()
    _assert_state_equal(run.state(), after_first)
    assert float(run.opt.last_step_skipped) == 1.0
    run.set_c(seq[3])
    graph.replay()
    torch.cuda.synchronize()
    _assert_state_equal(run.state(), eager.state())
    assert all(s[3] == 3.0 for s in run.state())
    assert run.scaler.get_scale() == eager.scaler.get_scale() == ref.scaler.get_scale() == 2.0 ** 15
    for p, q in zip(a, c):
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-6)


# ---------------------------------------------------------------- 5. averaged model against torch
def _perturb(model, g):
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.1 * torch.randn(p.shape, device=p.device, generator=g))
        for n, b in model.named_buffers():
            if b.dtype == torch.float32:
                b.add_(0.1 * torch.rand(b.shape, device=b.device, generator=g))
            else:
                b.add_(3)


@pytest.mark.parametrize("decay,use_buffers", [(None, False), (None, True), (0.999, False)],
                         ids=["equal", "equal_use_buffers", "ema"])
def test_fused_averaged_model_vs_torch(gpu, decay, use_buffers):
    """five updates, the source perturbed in between: the first is a copy (bitwise), the later ones
    agree to rtol 1e-5 / atol 1e-5 (<= 4 fp32 roundings at magnitude <= 8 per update).  With
    use_buffers=True torch's own GPU path cannot average BatchNorm's int64 num_batches_tracked (its
    foreach update raises on integer tensors), so that case's reference is AveragedModel(use_buffers=True)
    on CPU copies of the same source, torch's per-tensor formula."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from xcp.optim import FusedAveragedModel
    torch.manual_seed(5)
    model = nn.Sequential(nn.Conv2d(3, 8, 3), nn.BatchNorm2d(8), nn.Linear(300, 70)).to(gpu)   # 21000 > one chunk
    g = torch.Generator(device=gpu).manual_seed(51)
    _perturb(model, g)
    ref_dev = torch.device("cpu") if use_buffers else gpu
    src = copy.deepcopy(model).to(ref_dev)
    ref = AveragedModel(src, use_buffers=use_buffers,
                        multi_avg_fn=None if decay is None else get_ema_multi_avg_fn(decay)).to(ref_dev)
    avg = FusedAveragedModel(model, use_buffers=use_buffers, decay=decay)
    assert avg.n_averaged.is_cuda and list(avg.state_dict()) == list(ref.state_dict())
    one = torch.ones((), device=gpu)
    for k in range(5):
        _perturb(model, g)
        src.load_state_dict({n: t.to(ref_dev) for n, t in model.state_dict().items()})
        before = {n: t.clone() for n, t in avg.state_dict().items()}
        avg.update_parameters(model, skip=one)
        for n, t in avg.state_dict().items():
            assert torch.equal(t, before[n]), n
        versions = [t._version for t in avg.module.parameters()]
        avg.update_parameters(model)
        ref.update_parameters(src)
        assert all(t._version > v for t, v in zip(avg.module.parameters(), versions))
        assert int(avg.n_averaged) == int(ref.n_averaged) == k + 1
        got, want = avg.state_dict(), ref.state_dict()
        for n in want:
            if k == 0 and n != "n_averaged":   # the first update is a copy
                assert torch.equal(got[n], model.state_dict()[n[len("module."):]]), n
            if want[n].dtype == torch.float32:
                torch.testing.assert_close(got[n].cpu(), want[n].cpu(), rtol=1e-5, atol=1e-5)
            else:
                assert torch.equal(got[n].cpu(), want[n].cpu()), n
    if not use_buffers:   # the buffers follow the model
        for n, t in model.named_buffers():
            assert torch.equal(avg.state_dict()["module." + n], t)


# ---------------------------------------------------------------- 6. trainer switch
def _small_model(seed=0):
    from Models.AUFaceModel import AUFaceCrossDetector
    torch.manual_seed(seed)
    return AUFaceCrossDetector(num_aus=17, face_dim=512, au_dim=512, lstm_hidden=256)


def _seeded(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _train_four(gpu, fused, **kw):
    from xcp.auface import AUFaceTrainer
    m = _small_model().to(gpu)
    torch.manual_seed(7)
    tr = AUFaceTrainer(m, samples_per_cls=(300, 1700), steps_per_epoch=8, fused_optimizer=fused, **kw)
    tr.train()
    lr0 = tr.optimizer.param_groups[0]["lr"]
    torch.manual_seed(8)   # (the embed head's dropout)
    for i in range(4):
        batch = (_seeded((2, 3, 3, 64, 64), 20 + i), _seeded((2, 4, 3, 64, 64), 30 + i), torch.tensor([i % 2, 1]),
                 torch.ones(2, 4), torch.ones(2, 4))
        loss, logits, probs = tr.micro_step(i, 8, batch)
        assert torch.isfinite(loss) and logits.shape == (2, 2) and probs.shape == (2,)
    torch.cuda.synchronize()
    return tr, lr0


def test_auface_trainer_fused_optimizer(gpu):
    """AUFaceTrainer(fused_optimizer=True): FusedAdamClip(AdamW, clip inside, capturable) and
    FusedAveragedModel in place of the torch tail -- one optimiser step after four micro-batches, the
    averaged model a bitwise copy, the scheduler advanced, and (fp32) every parameter's after-step sum
    within the suite's fp32 after-step contract of the torch tail's; then the same under autocast +
    GradScaler(2^8)."""
    from xcp.optim import FusedAdamClip, FusedAveragedModel
    ta, lr0 = _train_four(gpu, False, use_amp=False)
    tb, lr0b = _train_four(gpu, True, use_amp=False)
    assert isinstance(tb.optimizer, FusedAdamClip) and isinstance(tb.ema_model, FusedAveragedModel)
    assert isinstance(tb.ema_embed, FusedAveragedModel) and lr0b == lr0
    assert tb.optimizer_steps == 1 and int(tb.ema_model.n_averaged) == 1 and int(tb.ema_embed.n_averaged) == 1
    assert tb.optimizer.param_groups[0]["lr"] != lr0
    assert tb.optimizer.param_groups[0]["lr"] == ta.optimizer.param_groups[0]["lr"]
    for pa, pm in zip(tb.ema_model.module.parameters(), tb.model.parameters()):
        assert torch.equal(pa, pm)
    for pa, pm in zip(tb.ema_embed.module.parameters(), tb.embed_head.parameters()):
        assert torch.equal(pa, pm)
    bad = []
    for (n, p), q in zip([("model." + n, p) for n, p in tb.model.named_parameters()]
                         + [("embed." + n, p) for n, p in tb.embed_head.named_parameters()]
                         + [("arcface." + n, p) for n, p in tb.arcface.named_parameters()], ta.params):
        got, want = p.detach().double().sum().item(), q.detach().double().sum().item()
        tol = 2 * lr0 * max(5e-3 * p.numel(), 2) + 1e-6 * abs(want) + 1e-7
        if abs(got - want) > tol:
            bad.append((n, got, want, tol))
    assert not bad, bad[:5]
    # autocast + GradScaler: the scale and found_inf stay on the device inside scaler.step
    tc, lr0c = _train_four(gpu, True, use_amp=True, init_scale=2.0 ** 8)
    assert tc.scaler.get_scale() == 2.0 ** 8, f"the scaler skipped the step (scale now {tc.scaler.get_scale()})"
    assert tc.optimizer_steps == 1 and int(tc.ema_model.n_averaged) == 1
    assert all(float(tc.optimizer.state[p]["step"]) == 1.0 for p in tc.params if tc.optimizer.state[p])
    s = tc.eval_scores((_seeded((2, 3, 3, 64, 64), 40), _seeded((2, 4, 3, 64, 64), 41), torch.tensor([0, 1])))
    assert s.shape == (2,) and bool(((s >= 0) & (s <= 1)).all())
