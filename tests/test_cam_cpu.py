"""CPU side of the class-activation maps (xcp/attribution.py, csrc/cam.hip): the tapped restatement of the
oracle, the closed form of the exit map's gradient, the render reference against F.interpolate, argument
validation, the ops' meta kernels, and the well-posedness of the references the GPU tests compare against."""
import pytest
import torch
import torch.nn.functional as F

import cam_cases as CC
import frozen_stats as FS


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_tapped_restatement_is_the_oracle(N, S):
    from oracle import xception_oracle as O
    sd = FS.prepared_state()
    with torch.no_grad():
        f, acts = CC.tapped_forward(FS.frames(N, S), sd)
        assert torch.equal(f, O.backbone_forward(FS.frames(N, S), sd, train=False))
    assert set(acts) == {"exit"} | {f"block{k}" for k in range(1, 13)}
    assert acts["exit"].shape[:2] == (N, 2048) and acts["block12"].shape[:2] == (N, 1024)
    assert acts["block11"].shape[1] == 728 and acts["block1"].shape[1] == 128
    assert torch.equal(f, CC.oracle(N, S, -1)["features"])


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_exit_gradient_closed_form(N, S):
    """G_exit[n, c, p] == dF[n, c] / (h w) at every pixel, exactly, in fp64: the "exit" layer needs no backbone
    backward.  Hence gradcam and hirescam coincide there."""
    o = CC.oracle(N, S, -1, torch.float64)
    G = o["G"]["exit"]
    hw = G.shape[2] * G.shape[3]
    assert torch.equal(G, (o["dF"] / hw)[:, :, None, None].expand_as(G))
    a, _ = CC.raw_maps(o["A"]["exit"], G, "gradcam")
    b, _ = CC.raw_maps(o["A"]["exit"], G, "hirescam")
    assert torch.allclose(a, b, rtol=0, atol=1e-12 * a.abs().max().item())


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_sign_coverage_on_the_oracle(N, S):
    """a condition on the data: +FS.loss_of leaves no positive evidence anywhere (the all-zero map), -FS.loss_of
    gives every frame some"""
    for dtype in (torch.float32, torch.float64):
        o = CC.oracle(N, S, +1, dtype)
        raw, _ = CC.raw_maps(o["A"]["exit"], o["G"]["exit"], "gradcam")
        assert (raw < 0).all()
        o = CC.oracle(N, S, -1, dtype)
        raw, _ = CC.raw_maps(o["A"]["exit"], o["G"]["exit"], "gradcam")
        assert (raw.amax((1, 2)) > 0).all()


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_references_are_well_posed(N, S):
    """A condition, not a tolerance: for every (shape, layer, method) the GPU tests use, the oracle's fp32 raw
    map lies within 1e-5 ||abs-sum map|| of its fp64 one, so no ReLU / max-pool near-tie decides the answer."""
    o32, o64 = CC.oracle(N, S, -1), CC.oracle(N, S, -1, torch.float64)
    for layer in CC.LAYERS:
        for method in CC.METHODS:
            r32, _ = CC.raw_maps(o32["A"][layer], o32["G"][layer], method)
            r64, abs64 = CC.raw_maps(o64["A"][layer], o64["G"][layer], method)
            e = CC.abs_rel(r32, r64, abs64)
            print(f"{N}x{S}^2 {layer} {method}: fp32-to-fp64 {e:.2e}, ||raw|| / ||abs|| {(r64.norm() / abs64.norm()).item():.3f}")
            assert e <= 1e-5, (layer, method, e)


@pytest.mark.parametrize("h,w,OH,OW", [(1, 1, 7, 5), (2, 2, 64, 64), (10, 10, 299, 299), (19, 19, 37, 53), (10, 10, 10, 10)])
def test_render_reference_against_interpolate(h, w, OH, OW):
    g = torch.Generator().manual_seed(h * 100 + OH)
    raw = torch.randn((2, 3, h, w), generator=g, dtype=torch.float64)
    raw[0, 1] = -raw[0, 1].abs()   # a frame without positive evidence
    raw[:, :, 0, 0] = raw[:, :, 0, 0].abs() + 0.1
    raw[0, 1, 0, 0] = 0.0
    r = torch.relu(raw)
    up = F.interpolate(r.view(6, 1, h, w), (OH, OW), mode="bilinear", align_corners=False).view(2, 3, OH, OW)
    m = r.amax((2, 3), keepdim=True)
    want = torch.where(m > 0, up / m.clamp_min(1e-300), torch.zeros_like(up))
    got = CC.render_reference(raw, (OH, OW), dtype=torch.float64)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-14)
    assert torch.all(got[0, 1] == 0) and not torch.isnan(got).any()
    assert torch.allclose(CC.render_reference(raw, (OH, OW), normalize=False, dtype=torch.float64), up, rtol=1e-12, atol=1e-14)
    lens = torch.tensor([3, 2])
    masked = CC.render_reference(raw, (OH, OW), lens, dtype=torch.float64)
    assert torch.all(masked[1, 2] == 0) and torch.equal(masked[0], got[0]) and torch.equal(masked[1, :2], got[1, :2])
    # fp32, the kernel's arithmetic: in [0, 1], and exactly 1 where the map's maximum is a sampled pixel
    g32 = CC.render_reference(raw.float(), (OH, OW))
    assert g32.min() >= 0 and g32.max() <= 1
    top = torch.zeros(1, 1, h, w)
    top[0, 0, 0, 0] = 3.7
    assert CC.render_reference(top, (OH, OW)).max() == 1


def test_argument_validation():
    """argument errors are ValueErrors raised before anything touches the GPU (none is needed here)"""
    import xcp
    clips = torch.zeros(2, 3, 3, 8, 8)
    for kw in ({"layer": "block13"}, {"layer": "conv4"}, {"method": "gradcam++"}, {"normalize": "clip"},
               {"target": torch.zeros(3)}, {"target": torch.zeros(2, 2)}, {"target": [0, 1]}, {"size": (0, 4)}):
        with pytest.raises(ValueError):
            xcp.grad_cam(object(), clips, **kw)
    with pytest.raises(ValueError):
        xcp.grad_cam(object(), clips[0])
    with pytest.raises(ValueError):
        xcp.frame_relevance(object(), clips[0])
    with pytest.raises(ValueError):
        xcp.frame_relevance(object(), clips, target=torch.zeros(5))
    frames = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError):
        xcp.backbone_cam(object(), frames, lambda f: f.sum(), layer="block0")
    with pytest.raises(ValueError):
        xcp.backbone_cam(object(), frames, lambda f: f.sum(), method="scorecam")
    with pytest.raises(ValueError):
        xcp.backbone_cam(object(), clips, lambda f: f.sum())
    from xcp.engine import XceptionEngine
    assert XceptionEngine.LAYERS == xcp.attribution.LAYERS and XceptionEngine.TAP != XceptionEngine.INPUT


def test_meta_kernels():
    from xcp import torch_ops
    assert {"cam", "cam_render"} <= set(torch_ops.OPS)
    for dt in (torch.float32, torch.bfloat16):
        A = torch.empty((3, 25, 736), device="meta", dtype=dt)
        raw = torch.ops.xcp.cam(A, A, None, None, None, 728, 1)
        assert raw.shape == (3, 25) and raw.dtype == torch.float32
        s = torch.empty(728, device="meta")
        raw = torch.ops.xcp.cam(A, None, torch.empty((3, 728), device="meta"), s, s, 728, 0)
        assert raw.shape == (3, 25) and raw.dtype == torch.float32
    out = torch.ops.xcp.cam_render(torch.empty((2, 3, 10, 10), device="meta"),
                                   torch.empty(2, device="meta", dtype=torch.int32), 299, 299, True)
    assert out.shape == (2, 3, 299, 299) and out.dtype == torch.float32
    assert torch.ops.xcp.cam_render(torch.empty((2, 3, 1, 1), device="meta"), None, 7, 5, False).shape == (2, 3, 7, 5)


# ------------------------------------------------------------------ dry runs on the recording fake library
@pytest.fixture
def fake_lib(monkeypatch):
    from test_engine_dryrun import install_fake_lib
    return install_fake_lib(monkeypatch)


def test_entry_points_declared_and_bound():
    import os
    import re
    from xcp import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "xcp.h")).read()
    decls = dict(re.findall(r"int\s+(xcp_\w+)\(([^;]*)\);", hdr, re.S))
    for name in ("xcp_cam", "xcp_cam_render"):
        assert name in decls and name in _lib.SIGNATURES
        assert len([a for a in decls[name].split(",") if a.strip()]) == len(_lib.SIGNATURES[name])
    assert hdr.count("no reference op: build-defined") >= 2


def _frozen_backbone():
    import torch.nn as nn
    from Models.Xception import xception
    torch.manual_seed(0)
    m = xception(num_classes=1)
    m.fc = nn.Identity()
    for p in m.parameters():
        p.requires_grad = False
    return m


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_launches_of_backbone_cam(fake_lib, prec):
    """"exit" runs no engine backward at all; a block layer's backward stops after the blocks above the tap (two
    depthwise backward launches for the exit flow, one per unit of each block above) and launches no weight
    gradient; a registered forward hook is not called and does not send the call down the module path"""
    import xcp
    from oracle import xception_oracle as O
    m = _frozen_backbone().train()
    m.block4.eval()
    modes = {n: s.training for n, s in m.named_modules()}
    seen = []
    hook = m.block4.register_forward_hook(lambda mod, inp, out: seen.append(1))
    x = torch.rand(2, 3, 71, 71)
    score = lambda f: torch.nan_to_num(f).sum()   # noqa: E731  (the fake library computes nothing)
    units = [len([e for e in O.block_layout(*cfg) if e[0] == "sep"]) for cfg in O.BLOCKS]
    try:
        with xcp.precision(prec):
            raw = xcp.backbone_cam(m, x, score)
            assert raw.shape == (2, 3, 3) and raw.dtype == torch.float32
            assert fake_lib.count("xcp_cam") == 1 and "xcp_avgpool_bwd" not in fake_lib and "xcp_dw_bwd" not in fake_lib
            for layer, k, hw in (("block12", 12, 3), ("block11", 11, 5), ("block3", 3, 5), ("block1", 1, 17)):
                del fake_lib[:]
                raw = xcp.backbone_cam(m, x, score, layer=layer, method="hirescam")
                assert raw.shape == (2, hw, hw)
                assert fake_lib.count("xcp_cam") == 1 and fake_lib.count("xcp_avgpool_bwd") == 1
                assert fake_lib.count("xcp_dw_bwd") == 2 + sum(units[k:]), layer
                assert "xcp_gemm_tn" not in fake_lib and "xcp_conv1_dgrad" not in fake_lib
                assert "xcp_conv1_dgrad_bn" not in fake_lib and "xcp_bn_finalize_part" not in fake_lib
    finally:
        hook.remove()
    assert not seen
    assert {n: s.training for n, s in m.named_modules()} == modes
    assert all(p.grad is None and not p.requires_grad for p in m.parameters())


def test_backward_without_a_tap_launches_what_it_launched(fake_lib):
    """tap=None: the same launches in the same order as a backward with a tap and input_grad (which runs to
    the end), and no TAP key"""
    from xcp.engine import XceptionEngine
    m = _frozen_backbone().eval()
    eng = m._engine()
    x = torch.rand(2, 3, 71, 71)
    dF = torch.ones(2, 2048)
    eng.backward(eng.forward(x, False, for_backward=True)[1], dF, need=set())   # (packs the backward's weights once)
    runs = []
    for tap in (None, "block6"):
        _, S = eng.forward(x, False, for_backward=True)
        del fake_lib[:]
        grads = eng.backward(S, dF, need=set(), input_grad=True, tap=tap)
        runs.append(list(fake_lib))
        assert (XceptionEngine.TAP in grads) == (tap is not None) and XceptionEngine.INPUT in grads
    assert runs[0] == runs[1]
    with pytest.raises(ValueError):
        eng.backward(S, dF, tap="exit")
    with pytest.raises(ValueError):
        eng.tap_activation(S, "block13")
