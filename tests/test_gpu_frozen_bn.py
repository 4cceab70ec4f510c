"""Backward through the fused engine on frozen BatchNorm statistics (eval-mode BatchNorms, XCP_FIN_FROZEN)
against the CPU oracle under autograd, fp32.  Bounds: features 1e-4, every parameter
gradient 1e-3 rel-L2 of the whole tensor, BN affine gradients 5e-3.  The fp32 CPU oracle itself is ~1e-6
from fp64 on this set-up, so the bounds leave three orders of magnitude for summation order, while a missing
or wrong coefficient is O(1)."""
import pytest
import torch
import torch.nn as nn

import frozen_stats as FS

pytestmark = pytest.mark.gpu

SHAPES = [(4, 64), (3, 75)]


@pytest.fixture(scope="module")
def model(gpu):
    return FS.backbone(gpu)


def _buffers(m):
    return {n: b.clone() for n, b in m.named_buffers()}


@pytest.mark.parametrize("mode", ["eval", "train_bn_eval"])
@pytest.mark.parametrize("N,S", SHAPES)
def test_parameter_gradients_on_running_statistics(model, gpu, N, S, mode):
    """(a) eval mode, (b) model.train() with every BatchNorm in eval mode: the oracle's eval-mode parameter
    gradients; running buffers and num_batches_tracked bit-identical before and after"""
    ref = FS.oracle(N, S, False)
    FS.set_mode(model, mode)
    assert model.training == (mode != "eval")
    before = _buffers(model)
    got = FS.run(model, FS.frames(N, S).to(gpu), x_grad=False)
    after = _buffers(model)
    e = FS.rel(got["features"], ref["features"])
    print(f"{mode} {N}x{S}^2 features rel {e:.2e}")
    assert e <= 1e-4
    FS.check_param_grads(got["grads"], ref["grads"], f"{mode} {N}x{S}^2")
    assert before.keys() == after.keys() and len(before) > 100
    for n in before:
        assert torch.equal(before[n], after[n]), n


def test_both_recipes_give_the_same_bits(model, gpu):
    """(b) is the same computation as (a)"""
    x = FS.frames(3, 75).to(gpu)
    a = FS.run(FS.set_mode(model, "eval"), x, x_grad=False)
    b = FS.run(FS.set_mode(model, "train_bn_eval"), x, x_grad=False)
    assert torch.equal(a["features"], b["features"])
    for n in a["grads"]:
        assert torch.equal(a["grads"][n], b["grads"][n]), n


def test_train_mode_still_updates_the_buffers(model, gpu):
    """the other side of the flag: BatchNorms in train mode use batch statistics and update their buffers"""
    FS.set_mode(model, "train")
    before = _buffers(model)
    try:
        FS.run(model, FS.frames(3, 75).to(gpu), x_grad=False)
        assert not torch.equal(before["bn1.running_mean"], model.bn1.running_mean)
        assert int(model.bn1.num_batches_tracked) == int(before["bn1.num_batches_tracked"]) + 1
    finally:
        model.load_state_dict(before, strict=False)   # (module-scoped model: the prepared statistics back)
    assert isinstance(model.fc, nn.Identity)
