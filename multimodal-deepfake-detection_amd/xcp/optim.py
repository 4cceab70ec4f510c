"""Fused gradient clipping + Adam for the training step (train_visual.py:533, :575-577;
train_audio.py:21, :40-44): ``clip_grad_norm_(params, max_norm)`` followed by
``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` in two HIP launches over a chunk
table of every parameter (csrc/optim.hip), with the clip coefficient kept on the device.

A ``torch.optim.Optimizer``: ``param_groups`` (so ReduceLROnPlateau / OneCycleLR adjust
``lr``), per-parameter ``state`` with torch Adam's keys (``step``, ``exp_avg``,
``exp_avg_sq``; checkpoints interchange with torch.optim.Adam), ``zero_grad``,
``state_dict`` / ``load_state_dict``, and ``GradScaler.step`` (which unscales the grads
of ``param_groups`` before calling ``step``).  As torch Adam, parameters whose ``grad`` is
None are skipped, so a backbone that is frozen when the optimiser is built (the
reference's first three epochs, train_visual.py:547-553) starts training when it is
unfrozen.

Same update as torch's Adam (L2 weight decay, bias correction from each parameter's own
step count, no amsgrad / maximize).  With ``max_norm`` the gradients are clipped to that
total norm inside the update; ``param.grad`` keeps the unclipped gradient and ``step()``
returns the pre-clip total norm as a fresh 0-d device tensor (clip_grad_norm_'s return).
Without ``max_norm`` the script's own clip_grad_norm_ call does the clipping (as the
reference scripts do) and ``step()`` returns None.

``capturable=True`` (torch Adam's flag of that name): the step counts live on the device,
incremented and turned into the bias corrections there (xcp_opt_adam_dev), so the step can be
captured in a HIP graph and replayed -- no host arithmetic, no host sync.  Parameters whose counts
are equal share one 0-d device counter (``state["step"]`` is that tensor), so a group normally costs
one Adam launch.  Which parameters share a counter is decided on the host, without a device read,
so that torch Adam's per-parameter semantics hold: a parameter whose state is created after its group has stepped (a backbone
unfrozen after epoch 3, train_visual.py:547-556), a parameter whose grad is None on a step while its
counter-mates step, and a loaded state whose count differs from the others each get a counter of
their own (one more launch), never the group's count.

``decoupled_weight_decay=True`` (torch.optim.Adam's argument of that name) gives torch.optim.AdamW's
update: ``p *= 1 - lr * weight_decay`` and no ``weight_decay * p`` term in the gradient
(xcp_opt_adam_amp / xcp_opt_adam_amp_dev), with or without ``capturable`` and ``max_norm``.

GradScaler on the device: an instance built with ``capturable=True`` sets
``_step_supports_amp_scaling``, so ``GradScaler.step`` hands it ``grad_scale`` and ``found_inf`` as
device tensors instead of reading ``found_inf`` back on the host (torch/amp/grad_scaler.py,
``_maybe_opt_step``).  The kernels multiply each gradient by ``1 / grad_scale`` on load (or by the
clip coefficient over the unscaled norm, xcp_opt_sumsq_amp; ``param.grad`` keeps the scaled
gradient) and write nothing when ``found_inf`` is set; no step count advances on such a step, and
``last_step_skipped`` (a 0-d device tensor, 1.0 after a skipped step) says so without a host read --
pass it as ``FusedAveragedModel.update_parameters(model, skip=...)``.  So a whole AMP step
(``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()``) can be captured in a HIP
graph, overflow steps included.  With ``max_norm``, ``step()`` returns the unscaled pre-clip norm.
Supported orders: ``scaler.step(opt)`` alone; torch ``clip_grad_norm_`` on the scaled gradients and
then ``scaler.step(opt)`` (train_visual.py); ``scaler.unscale_(opt)``, a clip, ``scaler.step(opt)``
(train_au_face.py).  A non-capturable instance keeps its step counts on the host, where a skipped
step could not be taken back, so it leaves the attribute unset and GradScaler treats it as before.
Not supported: ``lr`` as a device tensor (a captured step keeps the ``lr`` it was captured with, so
OneCycleLR inside a graph is not), replacing GradScaler's own non-finite check pass, amsgrad and
maximize.

``FusedAveragedModel`` is ``torch.optim.swa_utils.AveragedModel`` with ``update_parameters`` as one
launch (xcp_opt_average) that reads ``n_averaged`` on the device.
"""
import itertools
import math

import torch
from torch.autograd.graph import increment_version

from . import _lib, ops

CHUNK = 16384


class FusedAdamClip(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None,
                 capturable=False, decoupled_weight_decay=False):
        if lr < 0.0 or eps < 0.0 or weight_decay < 0.0 or not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("FusedAdamClip: invalid hyper-parameter")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      decoupled_weight_decay=bool(decoupled_weight_decay)))
        for grp in self.param_groups:
            for p in grp["params"]:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise ValueError("FusedAdamClip: fp32 contiguous parameters only")
                ops.check_gpu(p)
        self.max_norm = max_norm
        self.capturable = capturable
        # GradScaler.step attaches grad_scale / found_inf and calls step() with no host read
        self._step_supports_amp_scaling = bool(capturable)
        self._skipped = None   # 0-d device flag of the last step, once a found_inf has been seen
        self._counters = {}   # capturable: id(device step counter) -> the counter
        self._tables = {}
        self._out = None

    def _state(self, p, counter=None):
        st = self.state[p]
        if not st:
            st["step"] = counter if self.capturable else torch.tensor(0.0)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @staticmethod
    def _key(kind, rows):
        """cache key of a chunk table: every pointer a row of it holds (param, grad and both
        moment buffers), so a replaced state tensor (load_state_dict, a re-zeroed moment) or a
        re-attached gradient can never reuse a table that points at the old storage"""
        return (kind,) + tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
                               for p, g, m, v in rows)

    @staticmethod
    def _decay(grp):
        """(wd, pmul) of the update: the L2 coefficient and the factor on p before it.  AdamW's
        1 - lr * weight_decay is formed in double here, as torch forms it, and passed as a float"""
        if grp.get("decoupled_weight_decay", False):
            return 0.0, float(1.0 - grp["lr"] * grp["weight_decay"])
        return float(grp["weight_decay"]), 1.0

    @property
    def last_step_skipped(self):
        """0-d fp32 device tensor: 1.0 if GradScaler's found_inf made the last step() write nothing"""
        if self._skipped is None:
            p = self.param_groups[0]["params"][0]
            self._skipped = torch.zeros((), device=p.device, dtype=torch.float32)
        return self._skipped

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables.clear()   # the moment buffers were replaced

    def _table(self, key, rows, dev):
        """device chunk table for a list of (param, grad, exp_avg, exp_avg_sq), cached by pointers"""
        tab = self._tables.get(key)
        if tab is None:
            r = []
            for p, g, m, v in rows:
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise ValueError("FusedAdamClip: fp32 contiguous gradients only")
                n = p.numel()
                for s in range(0, n, CHUNK):
                    r.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s, min(CHUNK, n - s)])
            tab = torch.tensor(r, dtype=torch.int64).to(dev)
            if len(self._tables) > 64:
                self._tables.clear()
            self._tables[key] = tab
        return tab

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.capturable:
            return self._step_capturable(loss)
        # parameters with a gradient, grouped by (param group, step count) for the bias corrections
        launches, every = [], []
        for gi, grp in enumerate(self.param_groups):
            by_step = {}
            for p in grp["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdamClip does not support sparse gradients")
                st = self._state(p)
                st["step"] += 1
                row = (p, p.grad, st["exp_avg"], st["exp_avg_sq"])
                by_step.setdefault(int(st["step"].item()), []).append(row)
                every.append(row)
            for t, rows in by_step.items():
                launches.append((grp, t, rows))
        if not every:
            return loss
        dev = every[0][0].device
        with ops.device_guard(every[0][0]):
            s = ops.stream()
            coef = 0
            if self.max_norm is not None:
                tab = self._table(self._key("all", every), every, dev)
                part = torch.empty(tab.shape[0], device=dev, dtype=torch.float32)
                self._out = torch.empty(2, device=dev, dtype=torch.float32)
                _lib.call("xcp_opt_sumsq", tab.data_ptr(), tab.shape[0], part.data_ptr(), float(self.max_norm),
                          self._out.data_ptr(), s)
                coef = self._out.data_ptr()
            for grp, t, rows in launches:
                tab = self._table(self._key("grp", rows), rows, dev)
                b1, b2 = grp["betas"]
                if grp.get("decoupled_weight_decay", False):
                    wd, pmul = self._decay(grp)
                    _lib.call("xcp_opt_adam_amp", tab.data_ptr(), tab.shape[0], coef, float(grp["lr"]), float(b1),
                              float(b2), float(grp["eps"]), wd, pmul, float(1.0 - b1 ** t),
                              float(math.sqrt(1.0 - b2 ** t)), 0, 0, s)
                    continue
                _lib.call("xcp_opt_adam", tab.data_ptr(), tab.shape[0], coef, float(grp["lr"]), float(b1), float(b2),
                          float(grp["eps"]), float(grp["weight_decay"]), float(1.0 - b1 ** t),
                          float(math.sqrt(1.0 - b2 ** t)), s)
        # the kernels wrote the parameters through raw pointers: bump their autograd version
        # counters as an in-place torch op would, so that consumers keyed on them (the xcp
        # engine's packed-weight cache, engine.pack) see the update
        increment_version([row[0] for row in every])
        if loss is not None:
            return loss
        return self._out[1].clone() if self.max_norm is not None else None

    def _counter(self, value, device=None):
        """a new device step counter: a fresh one holding the host number `value`, or a copy of the
        device counter `value`.  Never inside a graph capture: the replay would re-run the fill /
        copy, so the count would restart on every replay"""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamClip(capturable=True): the set of parameters with gradients changed "
                               "inside a graph capture; run one eager step with the captured structure first")
        if torch.is_tensor(value):
            t = value.clone()
        else:
            t = torch.full((), float(value), device=device, dtype=torch.float32)
        self._counters[id(t)] = t
        return t

    @staticmethod
    def _amp_flag(t, dev):
        """GradScaler's scale as one fp32 on the parameters' device (it already is one there)"""
        if t is None:
            return None
        if t.dtype != torch.float32 or t.device != dev:
            t = t.to(device=dev, dtype=torch.float32)
        return t

    def _step_capturable(self, loss):
        """step() with the step counts on the device: per distinct counter, t += 1 on the device,
        then one Adam launch reading t (no .item(), no host-side bias corrections).  Counters are
        regrouped on the host by which parameters hold them (never by reading a count), so that every
        parameter's count is its own number of steps, as in torch Adam: a fresh state starts a fresh
        counter at 0, a loaded state joins a counter of its own count, and a counter whose parameters
        do not all step this time is split (a device copy) before the stepping ones advance it."""
        launches, every = [], []
        for gi, grp in enumerate(self.param_groups):
            stepping = []
            fresh = None
            for p in grp["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("FusedAdamClip does not support sparse gradients")
                if not self.state[p]:
                    if fresh is None:
                        fresh = self._counter(0, p.device)
                    self._state(p, fresh)
                stepping.append(p)
            # adopt loaded (host / foreign) step tensors: one shared counter per distinct count
            adopted = {}
            for p in grp["params"]:
                st = self.state.get(p)
                if not st or id(st["step"]) in self._counters:
                    continue
                v = int(float(st["step"]))
                if v not in adopted:
                    adopted[v] = self._counter(v, p.device)
                st["step"] = adopted[v]
            # group the stepping parameters by counter; split counters whose other members skip
            members = {}
            for p in grp["params"]:
                if p in self.state and self.state[p]:
                    members.setdefault(id(self.state[p]["step"]), set()).add(p)
            by_counter = {}
            for p in stepping:
                by_counter.setdefault(id(self.state[p]["step"]), []).append(p)
            for cid, ps in by_counter.items():
                t = self._counters[cid]
                if len(ps) != len(members[cid]):
                    t = self._counter(t)
                    for p in ps:
                        self.state[p]["step"] = t
                rows = [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for p in ps]
                launches.append((grp, t, rows))
                every.extend(rows)
        # forget counters no parameter holds any more
        live = {id(st["step"]) for st in self.state.values() if st and "step" in st}
        for cid in [c for c in self._counters if c not in live]:
            del self._counters[cid]
        if not every:
            return loss
        dev = every[0][0].device
        # what GradScaler.step attached (grad_scale is None after an explicit scaler.unscale_)
        gscale, found_inf = self._amp_flag(getattr(self, "grad_scale", None), dev), getattr(self, "found_inf", None)
        if found_inf is not None:
            self.last_step_skipped.copy_(found_inf.reshape(()) != 0)
        elif self._skipped is not None:
            self._skipped.zero_()
        skipped = self._skipped if found_inf is not None else None
        with ops.device_guard(every[0][0]):
            s = ops.stream()
            coef = 0
            if self.max_norm is not None:
                tab = self._table(self._key("all", every), every, dev)
                part = torch.empty(tab.shape[0], device=dev, dtype=torch.float32)
                self._out = torch.empty(2, device=dev, dtype=torch.float32)
                if gscale is None:
                    _lib.call("xcp_opt_sumsq", tab.data_ptr(), tab.shape[0], part.data_ptr(), float(self.max_norm),
                              self._out.data_ptr(), s)
                else:
                    _lib.call("xcp_opt_sumsq_amp", tab.data_ptr(), tab.shape[0], part.data_ptr(),
                              float(self.max_norm), gscale.data_ptr(), self._out.data_ptr(), s)
                coef = self._out.data_ptr()
            for grp, t, rows in launches:
                t.add_(1.0)
                if skipped is not None:
                    t.sub_(skipped)   # a skipped step is no step: the count advances by 1 - found_inf
                tab = self._table(self._key("grp", rows), rows, dev)
                b1, b2 = grp["betas"]
                if gscale is None and skipped is None and not grp.get("decoupled_weight_decay", False):
                    _lib.call("xcp_opt_adam_dev", tab.data_ptr(), tab.shape[0], coef, float(grp["lr"]), float(b1),
                              float(b2), float(grp["eps"]), float(grp["weight_decay"]), t.data_ptr(), s)
                    continue
                wd, pmul = self._decay(grp)
                _lib.call("xcp_opt_adam_amp_dev", tab.data_ptr(), tab.shape[0], coef, float(grp["lr"]), float(b1),
                          float(b2), float(grp["eps"]), wd, pmul, t.data_ptr(),
                          0 if gscale is None else gscale.data_ptr(), 0 if skipped is None else skipped.data_ptr(), s)
        increment_version([row[0] for row in every])
        if loss is not None:
            return loss
        return self._out[1].clone() if self.max_norm is not None else None


class FusedAveragedModel(torch.optim.swa_utils.AveragedModel):
    """``torch.optim.swa_utils.AveragedModel`` (train_au_face.py:604-605, :690-693) with
    ``update_parameters`` as one launch over every fp32 parameter (xcp_opt_average): the equal
    running average (``decay=None``, torch's default) or the exponential one (``decay=d``, what
    ``multi_avg_fn=get_ema_multi_avg_fn(d)`` computes).  ``n_averaged`` is read by the kernel and
    advanced on the device, so an update makes no host read.  Same ``state_dict`` as torch's
    (``n_averaged`` and ``module.``-prefixed keys).  ``avg_fn`` / ``multi_avg_fn`` are not
    supported, and neither are modules off the GPU: there is no CPU fallback.

    As torch's, with ``use_buffers=False`` the buffers are copied from the model on every update (the
    fp32 ones as plain-copy rows of the same launch, the others -- BatchNorm's int64
    ``num_batches_tracked`` -- by torch), and with ``use_buffers=True`` they are averaged with the
    parameters (the non-fp32 ones by torch ops on the device, in torch's own formula).

    ``update_parameters(model, skip=flag)``: a 0-d device tensor (``FusedAdamClip.last_step_skipped``);
    non-zero, the call changes nothing, ``n_averaged`` and the buffers included."""

    def __init__(self, model, device=None, avg_fn=None, multi_avg_fn=None, use_buffers=False, decay=None):
        if avg_fn is not None or multi_avg_fn is not None:
            raise ValueError("FusedAveragedModel: avg_fn / multi_avg_fn are not supported; decay=None is the equal "
                             "average and decay=d the exponential one")
        if decay is not None and not 0.0 <= decay <= 1.0:
            raise ValueError(f"FusedAveragedModel: invalid decay {decay}")
        super().__init__(model, device=device, use_buffers=use_buffers)
        self.decay = decay
        for t in itertools.chain(self.module.parameters(), self.module.buffers(), model.parameters(), model.buffers()):
            ops.check_gpu(t)
        if not self.n_averaged.is_cuda:   # torch leaves it on the CPU unless `device` is given; the kernel reads it
            self.n_averaged = self.n_averaged.to(next(self.module.parameters()).device)
        self._tab_key, self._tab, self._own_modules = None, None, None

    @staticmethod
    def _members(modules):
        """the parameters and the buffers of a list of modules, in Module.parameters() / .buffers() order
        (each tensor once), read from the modules' own dicts"""
        ps, bs, seen = [], [], set()
        for m in modules:
            for t in m._parameters.values():
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    ps.append(t)
            for t in m._buffers.values():
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    bs.append(t)
        return ps, bs

    def _pairs(self, model):
        """(fused rows (avg, src, plain copy), other (avg, src, plain copy)) in torch's pairing"""
        if self._own_modules is None:   # the averaged copy's module tree never changes; the model's is walked
            self._own_modules = list(self.module.modules())
        own_p, own_b = self._members(self._own_modules)
        src_p, src_b = self._members(model.modules())
        if len(own_p) != len(src_p) or len(own_b) != len(src_b):
            raise ValueError("FusedAveragedModel: the model does not match the averaged module")
        pairs = [(a, b, False) for a, b in zip(own_p, src_p)]
        pairs += [(a, b, not self.use_buffers) for a, b in zip(own_b, src_b)]
        fused, other = [], []
        for a, b, plain in pairs:
            if a.shape != b.shape:
                raise ValueError("FusedAveragedModel: the model does not match the averaged module")
            if a.numel() == 0:
                continue
            if a.dtype == torch.float32 and b.dtype == torch.float32:
                ops.check_gpu(a, b)
                if not (a.is_contiguous() and b.is_contiguous() and a.device == b.device):
                    raise ValueError("FusedAveragedModel: fp32 tensors must be contiguous and on one device")
                fused.append((a, b, plain))
            else:
                other.append((a, b, plain))
        return fused, other

    def _table(self, fused, dev):
        key = tuple((a.data_ptr(), b.data_ptr(), a.numel(), plain) for a, b, plain in fused)
        if key != self._tab_key:
            r = []
            for a, b, plain in fused:
                n = a.numel()
                for s in range(0, n, CHUNK):
                    r.append([a.data_ptr(), b.data_ptr(), s, min(CHUNK, n - s), int(plain)])
            self._tab = torch.tensor(r, dtype=torch.int64).to(dev)
            self._tab_key = key
        return self._tab

    @torch.no_grad()
    def update_parameters(self, model, skip=None):
        fused, other = self._pairs(model)
        n = self.n_averaged
        ops.check_gpu(n)
        if skip is not None:
            ops.check_gpu(skip)
            skip = skip.reshape(())
            if skip.dtype != torch.float32 or skip.device != n.device:
                skip = skip.to(device=n.device, dtype=torch.float32)
        if fused:
            with ops.device_guard(n):
                tab = self._table(fused, n.device)
                _lib.call("xcp_opt_average", tab.data_ptr(), tab.shape[0], n.data_ptr(),
                          -1.0 if self.decay is None else float(self.decay), 0 if skip is None else skip.data_ptr(),
                          ops.stream())
        for a, b, plain in other:   # the few non-fp32 tensors (num_batches_tracked): torch ops, no host read
            b = b.to(a.device)
            if plain:
                new = b
            elif self.decay is None:
                new = torch.where(n == 0, b, a + (b - a) / (n + 1))
            else:
                new = torch.where(n == 0, b, a * self.decay + b * (1 - self.decay))
            if skip is not None:
                new = torch.where(skip != 0, a, new.to(a.dtype))
            a.copy_(new)
        if skip is None:
            n.add_(1)
        else:
            n.add_((skip == 0).to(n.dtype))
        # the kernel wrote through raw pointers: bump the version counters as an in-place op would
        # (the engine repacks its kernel-layout weights by them before the averaged model is evaluated)
        increment_version([a for a, _, _ in fused])
