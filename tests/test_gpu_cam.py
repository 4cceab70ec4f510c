"""Class-activation maps on the GPU: the two kernels of csrc/cam.hip element-wise against fp64 / bit for bit,
the engine's taps and the public functions of xcp/attribution.py against the tapped CPU oracle (cam_cases.py).

Bounds.  xcp_cam: tests/elementwise.py's fp32-sum rule, |got - ref64| <= (n + 2) 2^-24 abs_terms, n derived in
cam_cases.cam_reference.  xcp_cam_render: bit for bit against the fp32 restatement in the kernel's own order.
fp32 engine: A and G rel-L2 <= 1e-3, features <= 1e-4 (DESIGN section 2's fp32 bounds for dx and features; G is the
same kind of quantity one step upstream); raw maps ||got - ref|| <= 2e-3 ||abs-sum map|| (1e-3 per factor; the
maps cancel to 0.01 - 0.25 of the abs-sum map, and a wrong tap, sign or pitch is O(1) in this measure).  bf16
engine: test_gpu_input_grad's rule -- at most 1.5 x the error of the oracle graph under torch.autocast(bfloat16)
with the same taps, + 0.01, both in the abs-sum measure."""
import pytest
import torch

import cam_cases as CC
import elementwise as EW
import frozen_stats as FS

pytestmark = pytest.mark.gpu

KERNEL_SHAPES = [(3, 1, 2048, 2048), (3, 4, 2048, 2048), (1, 9, 1024, 1024), (3, 25, 728, 736), (2, 100, 2048, 2048),
                 (2, 361, 728, 736), (2, 225, 128, 128)]
RENDER_SIZES = [(1, 1, 7, 5), (2, 2, 64, 64), (10, 10, 299, 299), (19, 19, 37, 53), (10, 10, 10, 10)]


# ------------------------------------------------------------------ xcp_cam
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,HW,C,CP", KERNEL_SHAPES)
def test_cam_kernel_elementwise(gpu, N, HW, C, CP, dtype):
    from xcp import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.xcp.*)
    g = torch.Generator().manual_seed(N * 1000 + HW)
    A = torch.randn((N, HW, CP), generator=g)
    G = torch.randn((N, HW, CP), generator=g) * 0.1
    if CP > C:   # the pad channels hold large finite garbage: they must be ignored, not relied on to be zero
        A[..., C:] = 1e30
        G[..., C:] = -1e30
    A, G = A.to(gpu, dtype), G.to(gpu, dtype)
    alpha = (torch.randn((N, C), generator=g) * 0.1).to(gpu)
    scale = (torch.rand(C, generator=g) + 0.5) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    scale, shift = scale.to(gpu), (torch.randn(C, generator=g) * 0.5).to(gpu)
    for bn in (False, True):
        sc, sh = (scale, shift) if bn else (None, None)
        for mode, al, gr in ((0, alpha, None), (0, None, G), (1, None, G)):
            tag = f"{N}x{HW}x{C}/{CP} {dtype} mode {mode} alpha {'given' if al is not None else 'computed'} bn {bn}"
            got = ops.cam(A, N, HW, C, CP, G=gr, alpha=al, a_scale=sc, a_shift=sh, mode=mode)
            again = ops.cam(A, N, HW, C, CP, G=gr, alpha=al, a_scale=sc, a_shift=sh, mode=mode)
            assert got.shape == (N, HW) and got.dtype == torch.float32
            assert torch.equal(got, again), tag   # no atomics: reproducible bit for bit
            ref64, abs_terms, n = CC.cam_reference(A, sc, sh, gr, al, mode, C)
            r = EW.assert_f32_sum(got.cpu(), ref64, abs_terms, n, tag=tag)
            print(f"{tag}: worst d / lim {r['worst']:.4f} (n = {n})")
    # through the registered op
    raw = torch.ops.xcp.cam(A, G, None, None, None, C, 1)
    assert torch.equal(raw, ops.cam(A, N, HW, C, CP, G=G, mode=1))


def test_cam_kernel_bad_arguments(gpu):
    from xcp import _lib, ops
    lib = _lib.load()
    A = torch.zeros((2, 4, 16), device=gpu)
    raw = torch.zeros((2, 4), device=gpu)
    v = torch.zeros(4096, device=gpu)
    a, r, p, st = A.data_ptr(), raw.data_ptr(), v.data_ptr(), ops.stream()
    EINVAL, EUNSUPPORTED = 1001, 1002
    assert lib.xcp_cam(0, 1, a, None, None, a, None, r, 2, 4, 16, 16, st) == 0
    assert lib.xcp_cam(0, 1, a, None, None, a, None, r, 2, 4, 17, 16, st) == EINVAL       # C > CP
    assert lib.xcp_cam(0, 1, a, None, None, a, None, r, 2, 4, 12, 12, st) == EINVAL       # CP % 8
    assert lib.xcp_cam(0, 1, a, None, None, None, None, r, 2, 4, 16, 16, st) == EINVAL    # hirescam without G
    assert lib.xcp_cam(0, 1, a, None, None, a, p, r, 2, 4, 16, 16, st) == EINVAL          # hirescam with alpha
    assert lib.xcp_cam(0, 0, a, None, None, None, None, r, 2, 4, 16, 16, st) == EINVAL    # gradcam without weights
    assert lib.xcp_cam(0, 2, a, None, None, a, None, r, 2, 4, 16, 16, st) == EINVAL       # unknown mode
    assert lib.xcp_cam(0, 0, a, p, None, a, None, r, 2, 4, 16, 16, st) == EINVAL          # half a BN
    assert lib.xcp_cam(0, 0, a, None, None, a, None, r, 0, 4, 16, 16, st) == EINVAL
    assert lib.xcp_cam(0, 0, a, None, None, a, None, r, 2, 0, 16, 16, st) == EINVAL
    assert lib.xcp_cam(0, 0, None, None, None, a, None, r, 2, 4, 16, 16, st) == EINVAL
    assert lib.xcp_cam(2, 0, a, None, None, a, None, r, 2, 4, 16, 16, st) == EUNSUPPORTED  # dtype
    assert lib.xcp_cam(0, 0, a, None, None, a, None, r, 2, 4, 2056, 2056, st) == EUNSUPPORTED   # C beyond the LDS
    assert lib.xcp_cam_render(r, None, p, 1, 2, 2, 2, 4, 4, 1, st) == 0
    assert lib.xcp_cam_render(r, None, p, 1, 2, 2, 2, 4, 4, 2, st) == EINVAL
    assert lib.xcp_cam_render(r, None, p, 1, 2, 0, 2, 4, 4, 1, st) == EINVAL
    assert lib.xcp_cam_render(r, None, p, 1, 2, 2, 2, 0, 4, 1, st) == EINVAL
    assert lib.xcp_cam_render(None, None, p, 1, 2, 2, 2, 4, 4, 1, st) == EINVAL
    assert lib.xcp_cam_render(r, None, p, 1, 2, 91, 91, 4, 4, 1, st) == EUNSUPPORTED     # h w beyond the LDS
    assert lib.xcp_cam_render(r, None, p, 1, 2, 2, 2, 1, 2049, 1, st) == EUNSUPPORTED    # OW beyond the LDS
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.cam(A, 2, 4, 16, 16, G=A.bfloat16(), mode=1)
    with pytest.raises(ValueError):
        ops.cam_render(raw, (4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.cam_render(torch.zeros(1, 1, 2, 2), (4, 4))


# ------------------------------------------------------------------ xcp_cam_render
@pytest.mark.parametrize("h,w,OH,OW", RENDER_SIZES)
def test_cam_render_bitwise(gpu, h, w, OH, OW):
    from xcp import ops, torch_ops  # noqa: F401  (torch_ops registers torch.ops.xcp.*)
    g = torch.Generator().manual_seed(h * 100 + OH)
    raw = torch.randn((2, 3, h, w), generator=g)
    raw[0, 1] = -raw[0, 1].abs()           # no positive evidence (and a zero in it)
    raw[0, 1, 0, 0] = 0.0
    raw[1, 0] = raw[1, 0].clamp_max(1.0)   # this frame's maximum is its first pixel, which every size here samples
    raw[1, 0, 0, 0] = 2.5
    lens = torch.tensor([3, 2], dtype=torch.int32)
    x = raw.to(gpu)
    for normalize in (True, False):
        got = ops.cam_render(x, (OH, OW), None, normalize)
        want = CC.render_reference(raw, (OH, OW), None, normalize)
        assert got.shape == (2, 3, OH, OW) and got.dtype == torch.float32
        assert torch.equal(got.cpu(), want), (normalize, (got.cpu() - want).abs().max())
        assert torch.all(got[0, 1] == 0) and not torch.isnan(got).any()
        masked = ops.cam_render(x, (OH, OW), lens.to(gpu), normalize)
        assert torch.equal(masked.cpu(), CC.render_reference(raw, (OH, OW), lens, normalize))
        assert torch.all(masked[1, 2] == 0) and torch.equal(masked[0], got[0]) and torch.equal(masked[1, :2], got[1, :2])
        if normalize:
            assert got.min() >= 0 and got.max() <= 1
            assert got[1, 0].max() == 1   # exactly
            if (h, w) in ((1, 1), (OH, OW)):   # a constant plane / the identity: every frame with evidence reaches 1
                pos = (raw.amax((2, 3)) > 0).to(gpu)
                assert torch.all(got.amax((2, 3))[pos] == 1)
        else:
            assert torch.equal(got[1, 0].max().cpu(), torch.tensor(2.5))
    assert torch.equal(torch.ops.xcp.cam_render(x, lens.to(gpu), OH, OW, True), ops.cam_render(x, (OH, OW), lens.to(gpu)))


# ------------------------------------------------------------------ engine taps
@pytest.fixture(scope="module")
def frozen_model(gpu):
    return FS.backbone(gpu, frozen=True).eval()


def engine_taps(model, x, layer, sign, prec="fp32", **kw):
    """one engine forward, the features' gradient by autograd, the tapped activation and (a block layer) the
    tapped gradient of a backward: NCHW fp32 (A, G), the features, the backward's result"""
    import xcp
    from xcp.engine import XceptionEngine
    with xcp.precision(prec), torch.no_grad():
        eng = model._engine()
        feats, S = eng.forward(x, False, for_backward=True)
        with torch.enable_grad():
            f = feats.clone().requires_grad_(True)
            (dF,) = torch.autograd.grad(sign * FS.loss_of(f), f)
        A, sc, sh, N, h, w, C, CP = eng.tap_activation(S, layer)
        A = CC.to_nchw(A, N, h, w, C, CP)
        if layer == "exit":
            A = torch.relu(A * sc[None, :, None, None] + sh[None, :, None, None])
            return A, (dF / (h * w))[:, :, None, None].expand_as(A), feats, {}
        kw.setdefault("need", set())
        grads = eng.backward(S, dF, tap=layer, **kw)
        tap = grads[XceptionEngine.TAP]
        assert tap.dtype == eng.dtype and tap.numel() == N * h * w * CP
        return A, CC.to_nchw(tap, N, h, w, C, CP), feats, grads


@pytest.mark.parametrize("layer", CC.LAYERS)
@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_engine_taps_fp32(frozen_model, gpu, N, S, layer):
    import xcp
    ref = CC.oracle(N, S, -1)
    x = FS.frames(N, S).to(gpu)
    A, G, feats, _ = engine_taps(frozen_model, x, layer, -1)
    eA, eG, eF = FS.rel(A, ref["A"][layer]), FS.rel(G, ref["G"][layer]), FS.rel(feats, ref["features"])
    print(f"{N}x{S}^2 {layer}: A rel-L2 {eA:.2e}, G rel-L2 {eG:.2e}, features {eF:.2e}")
    assert A.shape == ref["A"][layer].shape and G.shape == ref["G"][layer].shape
    assert eF <= 1e-4 and eA <= 1e-3 and eG <= 1e-3
    for method in CC.METHODS:
        want, abs_map = CC.raw_maps(ref["A"][layer], ref["G"][layer], method)
        with xcp.precision("fp32"):
            raw = xcp.backbone_cam(frozen_model, x, lambda f: -FS.loss_of(f), layer=layer, method=method)
        e = CC.abs_rel(raw, want, abs_map)
        print(f"{N}x{S}^2 {layer} {method}: raw ||d|| / ||abs|| {e:.2e}, ||raw|| / ||abs|| "
              f"{(want.norm() / abs_map.norm()).item():.3f}")
        assert raw.shape == want.shape and raw.dtype == torch.float32
        assert e <= 2e-3
    assert all(p.grad is None for p in frozen_model.parameters()) and not frozen_model.training


@pytest.mark.parametrize("layer", ["block12", "block6", "block1"])
def test_tap_early_stop_equals_full_backward(frozen_model, gpu, layer):
    """the tap of a backward that stops after producing it is the tap of a full one (need=set(), input_grad=True),
    whose dx is the dx of the run without a tap"""
    from xcp.engine import XceptionEngine
    N, S = 3, 75
    x = FS.frames(N, S).to(gpu)
    _, G, _, early = engine_taps(frozen_model, x, layer, +1)
    _, Gf, _, full = engine_taps(frozen_model, x, layer, +1, input_grad=True)
    assert set(early) == {XceptionEngine.TAP} and set(full) == {XceptionEngine.TAP, XceptionEngine.INPUT}
    assert torch.equal(G, Gf) and torch.equal(early[XceptionEngine.TAP], full[XceptionEngine.TAP])
    plain = FS.run(frozen_model, x, x_grad=True)
    assert torch.equal(full[XceptionEngine.INPUT], plain["dx"])


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_sign_coverage_and_rendered_maps(frozen_model, gpu, N, S):
    """+FS.loss_of: no positive evidence anywhere, the all-zero map; -FS.loss_of: every frame has some"""
    import xcp
    from xcp import ops
    x = FS.frames(N, S).to(gpu)
    for sign in (+1, -1):
        o = CC.oracle(N, S, sign)
        want, _ = CC.raw_maps(o["A"]["exit"], o["G"]["exit"], "gradcam")
        assert (want < 0).all() if sign > 0 else (want.amax((1, 2)) > 0).all()   # a condition on the data
        with xcp.precision("fp32"):
            raw = xcp.backbone_cam(frozen_model, x, lambda f: sign * FS.loss_of(f))
        maps = ops.cam_render(raw[None], (S, S))[0]
        assert maps.shape == (N, S, S)
        if sign > 0:
            assert (raw < 0).all() and torch.all(maps == 0)
        else:
            assert (raw.amax((1, 2)) > 0).all()
            ref = CC.render_reference(want[None], (S, S), dtype=torch.float64)[0]
            d = (maps.double().cpu() - ref).abs().max().item()
            print(f"{N}x{S}^2 rendered exit maps: max |d| to the fp64 oracle's {d:.2e}")
            assert maps.min() >= 0 and maps.max() <= 1 and not torch.isnan(maps).any()
            assert torch.equal(maps.cpu(), CC.render_reference(raw[None], (S, S))[0])


@pytest.mark.parametrize("N,S", CC.SHAPES)
def test_bf16_raw_maps_vs_torch_autocast(frozen_model, gpu, N, S):
    import xcp
    ref = CC.oracle(N, S, -1)
    x = FS.frames(N, S).to(gpu)
    sd = {k: v.to(gpu) for k, v in FS.prepared_state().items()}
    with torch.autocast("cuda", dtype=torch.bfloat16):
        auto = CC.taps_of(lambda f: -FS.loss_of(f.float()), x, sd)
    for layer in CC.LAYERS:
        for method in CC.METHODS:
            want, abs_map = CC.raw_maps(ref["A"][layer], ref["G"][layer], method)
            ra, _ = CC.raw_maps(auto["A"][layer].float(), auto["G"][layer].float(), method)
            with xcp.precision("bf16"):
                raw = xcp.backbone_cam(frozen_model, x, lambda f: -FS.loss_of(f), layer=layer, method=method)
            e16, ea = CC.abs_rel(raw, want, abs_map), CC.abs_rel(ra, want, abs_map)
            print(f"bf16 {N}x{S}^2 {layer} {method}: engine {e16:.3e}, torch autocast {ea:.3e}")
            assert e16 <= 1.5 * ea + 0.01, (layer, method)


# ------------------------------------------------------------------ clip models
@pytest.fixture(scope="module")
def clip_model(gpu):
    from Models.XceptionLSTMV import XceptionLSTMV
    torch.manual_seed(3)
    m = XceptionLSTMV(16, pretrained=False)
    m.feature_extractor.load_state_dict({k: v for k, v in FS.prepared_state().items() if not k.startswith("fc.")})
    return m.to(gpu)


def test_clip_grad_cam(clip_model, gpu):
    import xcp
    from oracle import xception_oracle as O
    m = clip_model.train()
    m.fc_layers.eval()
    B, T, S = 2, 3, 64
    clips = torch.rand((B, T, 3, S, S), generator=torch.Generator().manual_seed(11))
    x = clips.to(gpu)
    lens = torch.tensor([3, 2], device=gpu)
    modes = {n: s.training for n, s in m.named_modules()}
    flags = {n: p.requires_grad for n, p in m.named_parameters()}
    bufs = {n: b.clone() for n, b in m.named_buffers()}
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    o = CC.taps_of(lambda f: O.head_forward(f.view(B, T, -1), sd)[0].sum(), clips.reshape(B * T, 3, S, S), sd,
                   prefix="feature_extractor.", layers=["exit", "block11"])
    with xcp.precision("fp32"):
        for layer in ("exit", "block11"):
            maps, raw = xcp.grad_cam(m, x, layer=layer, return_raw=True)
            want, abs_map = CC.raw_maps(o["A"][layer], o["G"][layer], "gradcam")
            assert maps.shape == (B, T, S, S) and maps.dtype == torch.float32
            assert raw.shape == (B, T) + want.shape[1:] and raw.dtype == torch.float32
            e = CC.abs_rel(raw.reshape(want.shape), want, abs_map)
            print(f"clip {layer}: raw ||d|| / ||abs|| {e:.2e}")
            assert e <= 2e-3
            assert maps.min() >= 0 and maps.max() <= 1 and not torch.isnan(maps).any()
        # lengths: the padded frame is exactly zero; a clip equals itself run alone at its own length
        maps, raw = xcp.grad_cam(m, x, seq_lengths=lens, return_raw=True)
        again, raw2 = xcp.grad_cam(m, x, seq_lengths=lens, return_raw=True)
        assert torch.equal(maps, again) and torch.equal(raw, raw2)
        assert torch.all(maps[1, 2] == 0) and torch.all(raw[1, 2] == 0)
        _, alone = xcp.grad_cam(m, x[1:2, :2], return_raw=True)
        e = FS.rel(raw[1, :2], alone[0])
        print(f"clip 1 with lengths against itself alone at T = 2: rel-L2 {e:.2e}")
        assert e <= 1e-5
        # a target: the evidence for the stated class; for class 0 the map of 1 - prob
        t = torch.tensor([1.0, 0.0], device=gpu)
        _, rt = xcp.grad_cam(m, x, target=t, return_raw=True)
        _, r0 = xcp.grad_cam(m, x, return_raw=True)
        assert FS.rel(rt[0], r0[0]) <= 1e-5 and FS.rel(rt[1], -r0[1]) <= 1e-5
        sized = xcp.grad_cam(m, x, size=(37, 53), normalize="none", method="hirescam", layer="block3")
        assert sized.shape == (B, T, 37, 53) and sized.min() >= 0
        # frame relevance: gradient x input on the clip features
        rel = xcp.frame_relevance(m, x)
        prod = o["dF"] * o["features"]
        d = (rel.double().cpu().reshape(-1) - prod.double().sum(1)).norm() / prod.double().abs().sum(1).norm()
        print(f"frame relevance: ||d|| / ||abs|| {d.item():.2e}")
        assert rel.shape == (B, T) and rel.dtype == torch.float32 and d.item() <= 2e-3
        rl = xcp.frame_relevance(m, x, seq_lengths=lens)
        assert rl[1, 2] == 0 and torch.isfinite(rl).all()
    with xcp.precision("bf16"):
        maps16 = xcp.grad_cam(m, x, seq_lengths=lens)
        assert maps16.shape == (B, T, S, S) and torch.all(maps16[1, 2] == 0) and not torch.isnan(maps16).any()
    assert {n: s.training for n, s in m.named_modules()} == modes
    assert {n: p.requires_grad for n, p in m.named_parameters()} == flags
    assert all(p.grad is None for p in m.parameters())
    assert all(torch.equal(b, bufs[n]) for n, b in m.named_buffers())


def test_audio_and_bidirectional_models(gpu):
    import xcp
    from Models.XceptionLSTMA import XceptionLSTMA
    from Models.XceptionLSTMV import XceptionLSTMV
    torch.manual_seed(5)
    a = XceptionLSTMA(16, pretrained=False).to(gpu)
    mf = torch.rand(2, 3, 3, 13, device=gpu)
    lens = torch.tensor([2, 3], device=gpu)
    maps, raw = xcp.grad_cam(a, mf, seq_lengths=lens, layer="block12", return_raw=True)
    assert maps.shape == (2, 3, 64, 64) and raw.shape == (2, 3, 2, 2)
    assert torch.isfinite(maps).all() and torch.isfinite(raw).all() and torch.all(maps[0, 2] == 0)
    assert xcp.frame_relevance(a, mf, seq_lengths=lens).shape == (2, 3)
    with pytest.raises(ValueError):
        xcp.grad_cam(a, torch.rand(2, 3, 3, 64, 64, device=gpu))
    v = XceptionLSTMV(16, pretrained=False, bidirectional=True).to(gpu)
    clips = torch.rand(2, 3, 3, 64, 64, device=gpu)
    maps = xcp.grad_cam(v, clips, seq_lengths=lens, target=torch.tensor([[1.0], [0.0]], device=gpu))
    assert maps.shape == (2, 3, 64, 64) and torch.isfinite(maps).all() and torch.all(maps[0, 2] == 0)
    rel = xcp.frame_relevance(v, clips, seq_lengths=lens)
    assert rel.shape == (2, 3) and torch.isfinite(rel).all() and rel[0, 2] == 0
    assert all(p.grad is None for p in list(a.parameters()) + list(v.parameters()))
