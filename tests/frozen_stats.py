"""Shared set-up of the frozen-statistics / input-gradient GPU tests (test_gpu_frozen_bn.py,
test_gpu_input_grad.py): a backbone with non-trivial running statistics, the CPU oracle's answers
(computed once per shape and mode, never modified) and one engine run.

Running statistics: a seeded ``xception(num_classes=1)`` put through 20 train-mode oracle forwards on
seeded U[0,1) batches of 4 x 64^2, the updated buffers chained back in.  (With the initial buffers --
mean 0, variance 1 -- the eval-mode features collapse to ~3e-3 after one pass; after 20 they are ~0.08
and |dx| ~0.03: gradients large enough for a relative bound to mean something.)
"""
import functools

import torch
import torch.nn as nn


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def prepared_state():
    """state_dict (CPU, fp32) of the seeded backbone after the 20 statistics passes"""
    from Models.Xception import xception
    from oracle import xception_oracle as O
    torch.manual_seed(0)
    sd = {k: v.clone() for k, v in xception(num_classes=1).state_dict().items()}
    g = torch.Generator().manual_seed(2024)
    with torch.no_grad():
        for _ in range(20):
            out = {}
            O.backbone_forward(torch.rand((4, 3, 64, 64), generator=g), sd, train=True, stats_out=out)
            sd.update(out)
    return sd


def param_names():
    return [k for k, v in prepared_state().items()
            if not k.startswith("fc.") and "running_" not in k and "num_batches" not in k]


# Seeds of the frames.  The graph is only piecewise smooth (max-pool argmax, ReLU): on a draw with a near-tie,
# rounding alone routes a gradient elsewhere and the CPU oracle in fp32 lands 1e-3 .. 1e-2 from itself in fp64,
# in train mode, where batch statistics couple the frames -- above the bounds it is to referee.  Of the draws
# tried at 3 x 75^2 (seeds 375, 0 .. 5) the oracle's own fp32-to-fp64 distance in dx was 5.6e-3, 6.9e-6, 6.4e-3,
# 1.1e-2, 6.7e-4, 7.6e-6, 1.4e-4: bimodal.  The seed is the first with a well-posed reference (a property of
# the oracle alone, asserted by the train-mode test); the other shapes' first draw is well-posed already.
SEEDS = {(3, 75): 0}


@functools.lru_cache(maxsize=None)
def frames(N, S):
    return torch.rand((N, 3, S, S), generator=torch.Generator().manual_seed(SEEDS.get((N, S), 100 * N + S)))


def loss_of(feats):
    return (feats * torch.linspace(-1, 1, 2048, device=feats.device, dtype=feats.dtype)).sum()


@functools.lru_cache(maxsize=None)
def oracle(N, S, train, dtype=torch.float32):
    """the CPU oracle under autograd: features, dx and every parameter gradient, computed in ``dtype`` from
    the fp32 state and frames"""
    from oracle import xception_oracle as O
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in prepared_state().items()}
    params = {k: sd[k].clone().requires_grad_(True) for k in param_names()}
    sd.update(params)
    x = frames(N, S).to(dtype, copy=True).requires_grad_(True)
    f = O.backbone_forward(x, sd, train=train)
    gr = torch.autograd.grad(loss_of(f), [x] + list(params.values()))
    return {"features": f.detach(), "dx": gr[0], "grads": dict(zip(params, gr[1:]))}


def backbone(gpu, frozen=False):
    from Models.Xception import xception
    m = xception(num_classes=1)
    m.load_state_dict(prepared_state())
    m.fc = nn.Identity()
    for p in m.parameters():
        p.requires_grad = not frozen
    return m.to(gpu)


def set_mode(m, mode):
    """'eval'; 'train': batch statistics; 'train_bn_eval': model.train() with every BatchNorm in eval mode"""
    if mode == "eval":
        m.eval()
    else:
        m.train()
        if mode == "train_bn_eval":
            for b in m.modules():
                if isinstance(b, nn.BatchNorm2d):
                    b.eval()
    return m


def run(m, x, x_grad, prec="fp32"):
    """one forward + backward of the loss through the backbone: features, dx, parameter gradients"""
    import xcp
    for p in m.parameters():
        p.grad = None
    x = x.clone().requires_grad_(x_grad)
    with xcp.precision(prec):
        f = m(x)
        loss_of(f).backward()
    torch.cuda.synchronize()
    return {"features": f.detach(), "dx": x.grad,
            "grads": {n: p.grad for n, p in m.named_parameters() if p.grad is not None}}


def check_param_grads(got, ref, tag=""):
    """DESIGN section 2's fp32 bounds: rel-L2 of every whole gradient tensor <= 1e-3, BN affine <= 5e-3"""
    assert set(got) == set(ref), set(ref) ^ set(got)
    worst = {}
    for n, r in ref.items():
        affine = r.dim() == 1
        e = rel(got[n], r)
        k = "bn" if affine else "w"
        if e > worst.get(k, ("", -1.0))[1]:
            worst[k] = (n, e)
    print(f"{tag} worst parameter-gradient rel-L2: {worst}")
    for n, r in ref.items():
        assert rel(got[n], r) <= (5e-3 if r.dim() == 1 else 1e-3), (n, rel(got[n], r))
