"""Input-frame gradients and frozen-statistics BatchNorm backward, without a GPU: the new op's registration
and fake kernel, the C ABI's binding, and a dry run of the engine's host orchestration through the
recording fake library of tests/test_engine_dryrun.py."""
import os
import re

import pytest
import torch
import torch.nn as nn

from test_engine_dryrun import install_fake_lib


@pytest.fixture
def fake_lib(monkeypatch):
    return install_fake_lib(monkeypatch)


def test_stem_conv1_dgrad_registered_with_fake_kernel():
    from xcp import torch_ops
    assert "stem_conv1_dgrad" in torch_ops.OPS and hasattr(torch.ops.xcp, "stem_conv1_dgrad")
    for dt in (torch.float32, torch.bfloat16):
        g = torch.empty((5, 32, 31, 149), device="meta", dtype=dt)
        w = torch.empty((32, 3, 3, 3), device="meta")
        for IH, IW in ((63, 299), (64, 300)):   # both frame sizes give a 31 x 149 output
            dx = torch.ops.xcp.stem_conv1_dgrad(g, w, IH, IW)
            assert dx.shape == (5, 3, IH, IW) and dx.dtype == torch.float32 and dx.is_contiguous()


def test_new_entry_points_declared_and_bound():
    from xcp import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xcp.h")).read()
    decls = dict(re.findall(r"int\s+(xcp_\w+)\(([^;]*)\);", hdr, re.S))
    for name in ("xcp_conv1_dgrad", "xcp_conv1_dgrad_bn"):
        assert name in decls and name in _lib.SIGNATURES
        assert len([a for a in decls[name].split(",") if a.strip()]) == len(_lib.SIGNATURES[name])
    assert re.search(r"#define\s+XCP_FIN_FROZEN\s+4\b", hdr)
    common = open(os.path.join(os.path.dirname(__file__), "..", "multimodal-deepfake-detection_amd", "xcp", "csrc",
                               "common.h")).read()
    assert re.search(r"\bXCP_FIN_FROZEN\s*=\s*4\b", common)


def _backbone():
    from Models.Xception import xception
    torch.manual_seed(0)
    m = xception(num_classes=1)
    m.fc = nn.Identity()
    return m


def _record_args(monkeypatch, name):
    """the argument tuples of every call of one entry point (the recorder keeps names only)"""
    from xcp import _lib
    seen, inner = [], _lib.call

    def call(n, *args):
        if n == name:
            seen.append(args)
        return inner(n, *args)

    monkeypatch.setattr(_lib, "call", call)
    return seen


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_eval_frozen_parameters_input_gradient(fake_lib, prec):
    """eval mode, every parameter frozen, frames requiring grad: the backward runs (it raised before), launches
    no weight-gradient GEMM and exactly one conv1 data gradient -- the fused form where the fused weight
    gradient is used (bf16, frames <= 320 wide)"""
    import xcp
    m = _backbone().eval()
    for p in m.parameters():
        p.requires_grad = False
    x = torch.rand(2, 3, 71, 71, requires_grad=True)
    with xcp.precision(prec):
        f = m(x)
        assert f.requires_grad
        torch.nan_to_num(f).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype
    assert "xcp_gemm_tn" not in fake_lib
    assert "xcp_conv1_wgrad" not in fake_lib and "xcp_conv1_wgrad_bn" not in fake_lib
    assert "xcp_conv3x3_wgrad" not in fake_lib and "xcp_colreduce_f32" not in fake_lib
    assert fake_lib.count("xcp_conv1_dgrad") + fake_lib.count("xcp_conv1_dgrad_bn") == 1
    assert ("xcp_conv1_dgrad_bn" in fake_lib) == (prec == "bf16")
    assert "xcp_bn_finalize_part" not in fake_lib            # no batch statistics, no buffer update
    assert all(p.grad is None for p in m.parameters())


def test_eval_unfrozen_parameters_pass_the_frozen_flag(fake_lib, monkeypatch):
    m = _backbone().eval()
    seen = _record_args(monkeypatch, "xcp_bn_bwd_finalize_part")
    nbt = [b.num_batches_tracked.clone() for b in m.modules() if isinstance(b, nn.BatchNorm2d)]
    x = torch.rand(2, 3, 71, 71, requires_grad=True)
    torch.nan_to_num(m(x)).sum().backward()
    assert len(seen) == len(nbt) and all(a[13] & 4 for a in seen)
    assert "xcp_bn_finalize_part" not in fake_lib
    assert all(torch.equal(a, b.num_batches_tracked)
               for a, b in zip(nbt, (b for b in m.modules() if isinstance(b, nn.BatchNorm2d))))
    assert x.grad is not None and all(p.grad is not None for p in m.parameters())
    # train mode: the flag is absent
    seen.clear()
    m.train()
    torch.nan_to_num(m(torch.rand(2, 3, 71, 71))).sum().backward()
    assert seen and not any(a[13] & 4 for a in seen)


def test_train_module_with_eval_batchnorms_runs_on_running_statistics(fake_lib):
    """model.train() followed by .eval() on every BatchNorm (fine-tuning on frozen statistics): the engine's
    train flag is the BatchNorms' mode, not Xception.training"""
    m = _backbone().train()
    for b in m.modules():
        if isinstance(b, nn.BatchNorm2d):
            b.eval()
    assert m.training and m._engine().bn_training() is False
    torch.nan_to_num(m(torch.rand(2, 3, 71, 71))).sum().backward()
    assert "xcp_bn_finalize_part" not in fake_lib and "xcp_bn_bwd_finalize_part" in fake_lib


def test_mixed_batchnorm_modes_raise(fake_lib):
    m = _backbone().train()
    m.bn1.eval()
    m.block4.rep[2].eval()
    with pytest.raises(NotImplementedError, match=r"bn1.*block4\.rep\.2"):
        m(torch.rand(2, 3, 71, 71))


def test_train_mode_launch_sequence_unchanged_without_input_gradient(fake_lib):
    """frames that need no gradient: no data-gradient launch, in either mode"""
    m = _backbone().train()
    torch.nan_to_num(m(torch.rand(2, 3, 71, 71))).sum().backward()
    assert "xcp_conv1_dgrad" not in fake_lib and "xcp_conv1_dgrad_bn" not in fake_lib
    assert "xcp_gemm_tn" in fake_lib


def test_lstma_refuses_an_input_that_requires_grad(fake_lib):
    from Models.XceptionLSTMA import XceptionLSTMA
    torch.manual_seed(0)
    m = XceptionLSTMA(64, pretrained=False)
    a = torch.rand(2, 3, 3, 13, requires_grad=True)
    with pytest.raises(NotImplementedError, match="MFCC"):
        m.extract_features(a)
    with torch.no_grad():
        assert m.extract_features(a).shape == (2, 3, 2048)


def test_input_gradient_helper_restores_modes_and_leaves_param_grads(fake_lib, monkeypatch):
    import xcp
    from xcp import lstm as xl
    from Models.XceptionLSTMV import XceptionLSTMV
    # (the recorder's LSTM stand-in returns no input gradient: a differentiable one for this test)
    monkeypatch.setattr(xl.LSTM, "forward", lambda self, input, hx=None, lengths=None: (
        torch.nan_to_num(input[..., :self.hidden_size]) * 1.0, None))
    torch.manual_seed(0)
    m = XceptionLSTMV(64, pretrained=False).train()
    m.fc_layers.eval()
    modes = {n: s.training for n, s in m.named_modules()}
    clips = torch.rand(2, 3, 3, 71, 71)
    dx = xcp.input_gradient(m, clips)
    assert dx.shape == clips.shape and not clips.requires_grad
    assert {n: s.training for n, s in m.named_modules()} == modes
    assert all(p.grad is None for p in m.parameters())
    assert "xcp_bn_finalize_part" not in fake_lib and "xcp_gemm_tn" not in fake_lib
