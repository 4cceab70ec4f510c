"""Gradients w.r.t. the input frames through the fused engine, the module path and the clip model, against
the CPU oracle under autograd.  fp32 bounds: dx 1e-3 rel-L2, parameter gradients 1e-3
(BN affine 5e-3), features 1e-4; the fp32 CPU oracle is ~1e-6 from fp64 on this set-up, and a wrong tap, a
wrong parity or a missing coefficient is O(1).  bf16: the rule of test_bf16_gradient_noise_vs_torch_autocast
-- the engine's dx error against the fp32 oracle at most 1.5 x that of the oracle graph run on the GPU under
torch.autocast(bfloat16) on the same inputs, + 0.01."""
import pytest
import torch
import torch.nn as nn

import frozen_stats as FS

pytestmark = pytest.mark.gpu

SHAPES = [(4, 64), (3, 75)]


@pytest.fixture(scope="module")
def frozen_model(gpu):
    return FS.backbone(gpu, frozen=True).eval()


@pytest.fixture(scope="module")
def model(gpu):
    return FS.backbone(gpu)


@pytest.fixture(scope="module")
def eval_dx(frozen_model, gpu):
    """(c) eval mode, frozen parameters, frames requiring grad: one engine run per shape, shared"""
    cache = {}

    def get(N, S):
        if (N, S) not in cache:
            cache[N, S] = FS.run(frozen_model, FS.frames(N, S).to(gpu), x_grad=True)
        return cache[N, S]
    return get


@pytest.mark.parametrize("N,S", SHAPES)
def test_eval_frozen_parameters_dx(eval_dx, frozen_model, N, S):
    ref = FS.oracle(N, S, False)
    got = eval_dx(N, S)
    assert got["dx"] is not None and got["dx"].shape == (N, 3, S, S) and got["dx"].dtype == torch.float32
    e = FS.rel(got["dx"], ref["dx"])
    print(f"eval frozen {N}x{S}^2: dx rel-L2 {e:.2e}, |dx| {ref['dx'].norm():.3e}, "
          f"features rel {FS.rel(got['features'], ref['features']):.2e}")
    assert FS.rel(got["features"], ref["features"]) <= 1e-4
    assert e <= 1e-3
    if S % 2 == 0:   # the last row / column of an even-sized frame is covered by no window
        assert torch.all(got["dx"][:, :, -1, :] == 0) and torch.all(got["dx"][:, :, :, -1] == 0)
    assert not got["grads"]   # frozen parameters get no gradient


@pytest.mark.parametrize("N,S", SHAPES)
def test_train_mode_dx_and_unchanged_parameter_gradients(model, gpu, N, S):
    """(d) train mode with frames requiring grad: dx against the train-mode oracle; the parameter gradients
    are bit-identical to the same call without x.requires_grad.

    The reference must be well-posed on the draw (frozen_stats.SEEDS): the oracle in fp32 and in fp64 agree
    to a tenth of the bound, so no max-pool / ReLU near-tie decides the answer."""
    ref = FS.oracle(N, S, True)
    ref64 = FS.oracle(N, S, True, torch.float64)
    own = FS.rel(ref["dx"], ref64["dx"])
    print(f"train {N}x{S}^2: the oracle's own fp32-to-fp64 distance in dx {own:.2e}")
    assert own <= 1e-4
    FS.set_mode(model, "train")
    keep = {n: b.clone() for n, b in model.named_buffers()}
    try:
        x = FS.frames(N, S).to(gpu)
        plain = FS.run(model, x, x_grad=False)
        got = FS.run(model, x, x_grad=True)
    finally:
        model.load_state_dict(keep, strict=False)
    assert plain["dx"] is None
    e = FS.rel(got["dx"], ref["dx"])
    print(f"train {N}x{S}^2: dx rel-L2 {e:.2e} (to the fp64 oracle {FS.rel(got['dx'], ref64['dx']):.2e})")
    assert e <= 1e-3
    assert torch.equal(plain["features"], got["features"])
    assert set(plain["grads"]) == set(got["grads"]) == set(FS.param_names())
    for n in plain["grads"]:
        assert torch.equal(plain["grads"][n], got["grads"][n]), n
    FS.check_param_grads(got["grads"], ref["grads"], f"train {N}x{S}^2")


@pytest.mark.parametrize("N,S", SHAPES)
def test_module_path_dx_agrees(eval_dx, frozen_model, gpu, N, S):
    """(e) a forward hook sends the call through forward_modules (xcp::stem_conv1_dgrad): the same dx"""
    seen = []
    h = frozen_model.block4.register_forward_hook(lambda mod, inp, out: seen.append(out.shape))
    try:
        got = FS.run(frozen_model, FS.frames(N, S).to(gpu), x_grad=True)
    finally:
        h.remove()
    assert seen
    e = FS.rel(got["dx"], eval_dx(N, S)["dx"])
    print(f"module path {N}x{S}^2: dx rel-L2 to the engine's {e:.2e}")
    assert e <= 1e-4
    assert FS.rel(got["dx"], FS.oracle(N, S, False)["dx"]) <= 1e-3


def test_bench_frame_size_fp32_and_bf16(model, gpu):
    """2 x 299^2 (the row kernels, the fused BN-apply data gradient, block1's shapes), eval mode, parameters
    unfrozen, frames requiring grad"""
    from oracle import xception_oracle as O
    N, S = 2, 299
    ref = FS.oracle(N, S, False)
    FS.set_mode(model, "eval")
    x = FS.frames(N, S).to(gpu)
    got = FS.run(model, x, x_grad=True, prec="fp32")
    e32 = FS.rel(got["dx"], ref["dx"])
    print(f"299^2 fp32: dx rel-L2 {e32:.2e}, features {FS.rel(got['features'], ref['features']):.2e}")
    assert FS.rel(got["features"], ref["features"]) <= 1e-4
    assert e32 <= 1e-3
    FS.check_param_grads(got["grads"], ref["grads"], "299^2 fp32")
    # bf16 against PyTorch's own bf16 autocast of the oracle graph, same inputs, same process
    sd = {k: v.to(gpu) for k, v in FS.prepared_state().items()}
    xa = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        fa = O.backbone_forward(xa, sd, train=False)
    (dxa,) = torch.autograd.grad(FS.loss_of(fa.float()), xa)
    ea = FS.rel(dxa, ref["dx"])
    got16 = FS.run(model, x, x_grad=True, prec="bf16")
    e16 = FS.rel(got16["dx"], ref["dx"])
    print(f"299^2 bf16: dx rel-L2 engine {e16:.3e}, torch autocast {ea:.3e}")
    assert e16 <= 1.5 * ea + 0.01
    assert set(got16["grads"]) == set(FS.param_names())


@pytest.fixture(scope="module")
def clip_model(gpu):
    from Models.XceptionLSTMV import XceptionLSTMV
    torch.manual_seed(3)
    m = XceptionLSTMV(128, pretrained=False)
    m.feature_extractor.load_state_dict({k: v for k, v in FS.prepared_state().items() if not k.startswith("fc.")})
    return m.to(gpu)


def test_clip_input_gradient(clip_model, gpu):
    """xcp.input_gradient on XceptionLSTMV, B = 2, T = 3, 75^2, seq_lengths [3, 1], against oracle autograd
    through backbone_forward -> lstm_forward -> head_forward (each clip cut at its own length)"""
    import xcp
    from oracle import xception_oracle as O
    m = clip_model.train()
    m.fc_layers.eval()
    m.lstm.eval()
    modes = {n: s.training for n, s in m.named_modules()}
    B, T, S = 2, 3, 75
    clips = torch.rand((B, T, 3, S, S), generator=torch.Generator().manual_seed(11))
    lens = [3, 1]
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    xr = clips.clone().requires_grad_(True)
    feats = O.backbone_forward(xr.reshape(B * T, 3, S, S), sd, train=False, prefix="feature_extractor.").view(B, T, -1)
    score = sum(O.head_forward(feats[b:b + 1, :lens[b]], sd)[0].sum() for b in range(B))
    (ref,) = torch.autograd.grad(score, xr)
    with xcp.precision("fp32"):
        dx = xcp.input_gradient(m, clips.to(gpu), seq_lengths=torch.tensor(lens))
    torch.cuda.synchronize()
    assert dx.shape == clips.shape
    e = FS.rel(dx, ref)
    print(f"clip input gradient: rel-L2 {e:.2e}, |ref| {ref.norm():.3e}")
    assert ref.norm() > 0 and e <= 1e-3
    assert torch.all(dx[1, 1:] == 0)            # the padded frames
    assert torch.all(ref[1, 1:] == 0)
    assert all(p.grad is None for p in m.parameters())
    assert {n: s.training for n, s in m.named_modules()} == modes
    # BCE against a target: the FGSM direction
    y = torch.tensor([[1.0], [0.0]])
    xr2 = clips.clone().requires_grad_(True)
    f2 = O.backbone_forward(xr2.reshape(B * T, 3, S, S), sd, train=False, prefix="feature_extractor.").view(B, T, -1)
    prob = torch.cat([O.head_forward(f2[b:b + 1, :lens[b]], sd)[0] for b in range(B)])
    (ref2,) = torch.autograd.grad(nn.functional.binary_cross_entropy(prob, y, reduction="sum"), xr2)
    with xcp.precision("fp32"):
        dx2 = xcp.input_gradient(m, clips.to(gpu), seq_lengths=torch.tensor(lens), target=y.to(gpu))
    assert FS.rel(dx2, ref2) <= 1e-3


def test_lstma_input_requiring_grad_raises(gpu):
    from Models.XceptionLSTMA import XceptionLSTMA
    torch.manual_seed(0)
    m = XceptionLSTMA(64, pretrained=False).to(gpu).eval()
    a = torch.rand(2, 3, 3, 13, device=gpu, requires_grad=True)
    with pytest.raises(NotImplementedError, match="MFCC"):
        m.extract_features(a)
    assert m.extract_features(a.detach()).shape == (2, 3, 2048)
