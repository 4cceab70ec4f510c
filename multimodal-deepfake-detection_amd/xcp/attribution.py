"""Attribution for the clip models: input gradients, class-activation maps, per-frame relevance.

Saliency maps ("which pixels made this clip fake"), FGSM / PGD robustness checks and adversarial
training all start from d(score)/d(frames).  The backbone's autograd node produces it with the
hand-written conv1 data-gradient kernel (csrc/stem.hip) after a backward through the backbone on its
running BatchNorm statistics (eval mode); the LSTM (``need_dx``) and the torch head complete the chain.

As a picture a pixel gradient is noise at the scale of single pixels, and it costs a whole backbone backward.
``grad_cam`` draws the class-activation map of a backbone layer instead (Grad-CAM / HiResCAM over the face:
which region made a frame look fake): the engine's saved forward state holds every block output, its backward
hands out the gradient w.r.t. a block output (``XceptionEngine.backward(..., tap=)``) and stops there, and
for the last feature map the gradient is known in closed form, so the default layer runs no backbone backward
at all.  Two HIP kernels (csrc/cam.hip) reduce activation x gradient to the raw maps and render them.
``frame_relevance`` is the per-frame companion: gradient x input on the clip features.  DESIGN.md section 4.5
has the definitions.
"""
import torch
import torch.nn.functional as F


def input_gradient(model, clips, seq_lengths=None, target=None):
    """d(score)/d(clips) for a clip model with ``extract_features`` / ``forward`` (XceptionLSTMV).

    clips: [B, T, 3, H, W] on the model's device; seq_lengths: the per-clip frame counts of a
    zero-padded batch (the padded frames' gradient is then zero); target ([B] or [B, 1], 0 / 1): the
    score is the binary cross-entropy against it (the direction FGSM / PGD ascend), otherwise the summed
    clip probability.  The model runs in eval mode (running BatchNorm statistics, no dropout) and gets
    its previous mode back, module by module; ``torch.autograd.grad`` is used, so no ``param.grad`` is
    touched.  Returns a tensor of clips' shape and dtype."""
    if clips.dim() != 5:
        raise ValueError("input_gradient: clips must be [B, T, 3, H, W]")
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        with torch.enable_grad():
            x = clips.detach().requires_grad_(True)
            feats = model.extract_features(x)
            prob = model(feats, seq_lengths) if seq_lengths is not None else model(feats)
            if target is None:
                score = prob.sum()
            else:
                score = F.binary_cross_entropy(prob, target.to(prob).reshape(prob.shape), reduction="sum")
            (dx,) = torch.autograd.grad(score, x)
    finally:
        for m, t in modes:
            m.training = t
    return dx


METHODS = ("gradcam", "hirescam")
NORMALIZE = ("frame", "none")
LAYERS = ("exit",) + tuple(f"block{k}" for k in range(1, 13))


def _check_names(fn, layer, method, normalize="frame"):
    if layer not in LAYERS:
        raise ValueError(f"{fn}: unknown layer {layer!r}; one of {', '.join(LAYERS)}")
    if method not in METHODS:
        raise ValueError(f"{fn}: unknown method {method!r}; one of {', '.join(METHODS)}")
    if normalize not in NORMALIZE:
        raise ValueError(f"{fn}: unknown normalize {normalize!r}; one of {', '.join(NORMALIZE)}")


def _check_target(fn, target, B):
    if target is not None and (not torch.is_tensor(target) or tuple(target.shape) not in ((B,), (B, 1))):
        raise ValueError(f"{fn}: target must be a tensor of shape [{B}] or [{B}, 1] (0 / 1 per clip)")


def _evidence(prob, target):
    """the summed evidence for "fake" (no target) or for each clip's stated class: not input_gradient's
    cross-entropy, which is a direction of ascent -- a map shows what supports a class"""
    if target is None:
        return prob.sum()
    t = target.to(prob).reshape(prob.shape)
    return (t * prob + (1 - t) * (1 - prob)).sum()


class _eval_mode:
    """eval mode for the call (running BatchNorm statistics, no dropout); every module gets its own previous
    mode back"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()

    def __exit__(self, *exc):
        for m, t in self.modes:
            m.training = t


def backbone_cam(backbone, frames, score_fn, layer="exit", method="gradcam"):
    """Raw class-activation maps [N, h, w] fp32 (before any ReLU) of ``layer`` of an ``Xception`` backbone for
    ``frames`` [N, 3, IH, IW].

    ``score_fn(features [N, 2048]) -> scalar`` runs under torch autograd (``torch.autograd.grad``: no
    ``param.grad`` is touched); the features are the backbone's output before ``fc``, so a plain classifier
    passes ``lambda f: backbone.fc(f)[:, k].sum()``.  layer: "exit", the map relu(bn4(conv4)) the global average
    pool reads -- its gradient is dF / (h w) at every pixel, so no backbone backward runs -- or "block1" ..
    "block12", that Block's output, whose gradient the engine's backward hands out before it stops.  method:
    "gradcam" (channel weights = the spatial mean of the gradient) or "hirescam" (gradient x activation per
    pixel); they coincide at "exit".  The backbone runs in eval mode through its fused engine directly, in the
    active ``xcp.precision``: forward hooks registered on its sub-modules are NOT called (stock CAM tools hook
    modules, which sends ``Xception.forward`` down the module path; this function needs no hook).  One training
    forward's activation memory is held for the call."""
    _check_names("backbone_cam", layer, method)
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError("backbone_cam: frames must be [N, 3, H, W]")
    from . import ops
    from .engine import XceptionEngine
    ops.check_gpu(frames)
    with _eval_mode(backbone), ops.device_guard(frames):
        eng = backbone._engine()
        backbone._xcp_wait_buffers()
        with torch.no_grad():
            feats, S = eng.forward(frames.detach(), False, for_backward=True)
        with torch.enable_grad():
            f = feats.detach().requires_grad_(True)
            score = score_fn(f)
            if not torch.is_tensor(score) or score.numel() != 1:
                raise ValueError("backbone_cam: score_fn must return a scalar tensor")
            (dF,) = torch.autograd.grad(score.reshape(()), f)
        with torch.no_grad():
            A, scale, shift, N, h, w, C, CP = eng.tap_activation(S, layer)
            if layer == "exit":
                raw = ops.cam(A, N, h * w, C, CP, alpha=(dF / (h * w)).contiguous(), a_scale=scale, a_shift=shift)
            else:
                G = eng.backward(S, dF, need=set(), tap=layer)[XceptionEngine.TAP]
                raw = ops.cam(A, N, h * w, C, CP, G=G, mode=ops.CAM_MODES[method])
    return raw.view(N, h, w)


def _check_clips(fn, model, clips):
    """(B, T, the model's own frame preparation or None) of a clip batch; XceptionLSTMA takes MFCC input
    [B, T, 3, n_mfcc] and draws its 64^2 images from it (``input_frames``)"""
    prep = getattr(model, "input_frames", None)
    if not torch.is_tensor(clips) or clips.dim() != (5 if prep is None else 4):
        raise ValueError(f"{fn}: clips must be " + ("[B, T, 3, H, W]" if prep is None else "[B, T, 3, n_mfcc]"))
    return clips.shape[0], clips.shape[1], prep


def _lengths(seq_lengths, dev):
    return None if seq_lengths is None else torch.as_tensor(seq_lengths).to(device=dev, dtype=torch.int32).contiguous()


def grad_cam(model, clips, seq_lengths=None, target=None, layer="exit", method="gradcam", size=None,
             normalize="frame", return_raw=False):
    """Heat maps [B, T, OH, OW] fp32 in [0, 1] over the frames of a clip model (XceptionLSTMV: clips
    [B, T, 3, H, W]; XceptionLSTMA: [B, T, 3, n_mfcc], drawn over its 64^2 input images; one or both LSTM
    directions): which region supports the score.

    Score: the summed clip probability (the evidence for "fake"), or with ``target`` ([B] or [B, 1], 0 / 1) the
    probability of each clip's stated class.  layer / method: ``backbone_cam``.  The raw map's ReLU is
    up-sampled bilinearly (align_corners=False) to ``size`` (default: the backbone's input frame size);
    normalize "frame": divided by the low-resolution map's maximum (a frame without positive evidence is all
    zero, never NaN), "none": the ReLU'd map's own scale (a per-clip scale is one ``amax`` away).  Frames at
    t >= seq_lengths[b] are zero; the lengths stay on the device.  ``return_raw``: also the raw maps
    [B, T, h, w].  Eval mode for the call (every module's mode restored), ``torch.autograd.grad`` only, no
    buffer, ``param.grad`` or ``requires_grad`` flag touched."""
    _check_names("grad_cam", layer, method, normalize)
    B, T, prep = _check_clips("grad_cam", model, clips)
    _check_target("grad_cam", target, B)
    if size is not None and (len(size) != 2 or min(size) < 1):
        raise ValueError("grad_cam: size must be (OH, OW)")
    from . import ops
    ops.check_gpu(clips)
    with _eval_mode(model):
        frames = clips.reshape(B * T, *clips.shape[2:]) if prep is None else prep(clips)

        def score_fn(f):
            feats = f.view(B, T, -1)
            prob = model(feats, seq_lengths) if seq_lengths is not None else model(feats)
            return _evidence(prob, target)

        raw = backbone_cam(model.feature_extractor, frames, score_fn, layer, method)
        raw = raw.view(B, T, *raw.shape[1:])
        with ops.device_guard(raw):
            maps = ops.cam_render(raw, tuple(size) if size is not None else tuple(frames.shape[2:]),
                                  _lengths(seq_lengths, raw.device), normalize == "frame")
    return (maps, raw) if return_raw else maps


def frame_relevance(model, clips, seq_lengths=None, target=None):
    """Per-frame relevance [B, T] fp32 of a clip: sum_c dF * F over the frame's 2048 features (gradient x
    input on the clip features; the score is ``grad_cam``'s).  Plain torch on ``extract_features``: one scoring
    forward and the LSTM / head backward, no backbone backward.  Frames at t >= seq_lengths[b] are zero."""
    B, T, _ = _check_clips("frame_relevance", model, clips)
    _check_target("frame_relevance", target, B)
    with _eval_mode(model):
        with torch.no_grad():
            feats = model.extract_features(clips)
        with torch.enable_grad():
            f = feats.detach().float().requires_grad_(True)
            prob = model(f, seq_lengths) if seq_lengths is not None else model(f)
            (dF,) = torch.autograd.grad(_evidence(prob, target), f)
        rel = (dF * f.detach()).sum(-1)
        if seq_lengths is not None:
            t = torch.arange(T, device=rel.device)
            rel = torch.where(t[None, :] < _lengths(seq_lengths, rel.device)[:, None], rel, torch.zeros_like(rel))
    return rel
