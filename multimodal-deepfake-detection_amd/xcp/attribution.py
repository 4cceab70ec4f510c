"""Input attribution for the clip models: the gradient of a clip's score w.r.t. its frames.

Saliency maps ("which pixels made this clip fake"), FGSM / PGD robustness checks and adversarial
training all start from d(score)/d(frames).  The backbone's autograd node produces it with the
hand-written conv1 data-gradient kernel (csrc/stem.hip) after a backward through the backbone on its
running BatchNorm statistics (eval mode); the LSTM (``need_dx``) and the torch head complete the chain.
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
