"""Shared set-up of the class-activation-map tests (test_cam_cpu.py, test_gpu_cam.py): a tapped restatement of
the oracle's backbone, the fp64 references of the two kernels (csrc/cam.hip) and the oracle's maps, computed
once per (shape, sign, dtype) and never modified.

The set-up is tests/frozen_stats.py's: ``FS.prepared_state()``, ``FS.frames(N, S)``, eval mode, and
``+-FS.loss_of`` as the score (``sign`` below).  With ``+FS.loss_of`` every exit-layer raw value is negative on
both shapes (the all-zero-map case); with ``-FS.loss_of`` every frame has positive evidence.
"""
import functools

import torch
import torch.nn.functional as F

import frozen_stats as FS

SHAPES = [(4, 64), (3, 75)]
LAYERS = ["exit", "block12", "block11", "block6", "block3", "block1"]
METHODS = ["gradcam", "hirescam"]
U32 = 2.0 ** -24


def tapped_forward(x, sd, prefix=""):
    """``oracle.xception_oracle.backbone_forward`` in eval mode, composed from the oracle's own pieces, recording
    every Block output ("block1" .. "block12") and the map the global average pool reads ("exit").
    Returns (features [N, 2048], {layer: tensor NCHW})."""
    from oracle import xception_oracle as O
    p, acts = prefix, {}
    x = F.conv2d(x, sd[p + "conv1.weight"], None, 2, 0)
    x = F.relu(O._bn(x, sd, p + "bn1", False, None))
    x = F.conv2d(x, sd[p + "conv2.weight"], None, 1, 0)
    x = F.relu(O._bn(x, sd, p + "bn2", False, None))
    for i, cfg in enumerate(O.BLOCKS):
        x = O.block_forward(x, sd, f"{p}block{i + 1}", cfg, False, None)
        acts[f"block{i + 1}"] = x
    x = O.sepconv(x, sd, p + "conv3")
    x = F.relu(O._bn(x, sd, p + "bn3", False, None))
    x = O.sepconv(x, sd, p + "conv4")
    x = F.relu(O._bn(x, sd, p + "bn4", False, None))
    acts["exit"] = x
    x = F.adaptive_avg_pool2d(x, (1, 1))
    return x.view(x.size(0), -1), acts


def raw_maps(A, G, method):
    """(raw [N, h, w], abs-sum map [N, h, w]) of NCHW A and G in their dtype: the issue's definitions"""
    if method == "gradcam":
        alpha = G.mean((2, 3), keepdim=True)
        return (alpha * A).sum(1), (alpha.abs() * A.abs()).sum(1)
    return (G * A).sum(1), (G.abs() * A.abs()).sum(1)


def taps_of(score_of, x, sd, prefix="", layers=LAYERS):
    """{"features", "dF", "A": {layer}, "G": {layer}} by autograd through the tapped restatement"""
    x = x.clone().requires_grad_(True)   # (a graph even where every parameter is a constant)
    f, acts = tapped_forward(x, sd, prefix)
    taps = [acts[l] for l in layers]
    gr = torch.autograd.grad(score_of(f), [f] + taps)
    return {"features": f.detach(), "dF": gr[0], "A": {l: a.detach() for l, a in zip(layers, taps)},
            "G": dict(zip(layers, gr[1:]))}


@functools.lru_cache(maxsize=None)
def oracle(N, S, sign, dtype=torch.float32):
    """the CPU oracle's taps for FS.frames(N, S) under score = sign * FS.loss_of, computed in ``dtype``"""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in FS.prepared_state().items()}
    return taps_of(lambda f: sign * FS.loss_of(f), FS.frames(N, S).to(dtype), sd)


def abs_rel(got, ref, abs_map):
    """the measure of the raw maps, which cancel heavily (||raw|| is 0.01 - 0.25 of ||sum_c |alpha A| ||):
    ||got - ref|| / ||abs-sum map||"""
    got, ref, abs_map = (t.detach().double().cpu() for t in (got, ref, abs_map))
    return ((got - ref).norm() / abs_map.norm().clamp_min(1e-300)).item()


# ------------------------------------------------------------------ xcp_cam, fp64 on the kernel's actual inputs
def cam_reference(A, scale, shift, G, alpha, mode, C):
    """A, G [N, HW, CP] (any float dtype, as the kernel reads them), scale / shift [C] or None, alpha [N, C] or
    None -> (ref64 [N, HW], abs_terms [N, HW], n) in tests/elementwise.py's sense (assert_f32_sum).

    The kernel's sum per pixel: C products accumulated by fmaf (one rounding each) and the shuffle tree -- any
    order of C terms is within (C - 1) u of sum |terms| -- plus, with scale / shift, the one rounding of each
    activation fmaf(a, s, t): n = C.  Where the kernel forms the weights itself, w_c = (sum_p G) / HW costs HW - 1
    additions and one division, each within u of mean_p |G|: HW + 1 more, against abs_terms built from
    mean_p |G| (>= |w_c|)."""
    a = A[..., :C].double().cpu()
    if scale is not None:
        a = torch.relu(a * scale[:C].double().cpu() + shift[:C].double().cpu())
    HW = A.shape[1]
    if mode == 1:
        g = G[..., :C].double().cpu()
        return (g * a).sum(-1), (g.abs() * a.abs()).sum(-1), C
    if alpha is not None:
        w = alpha.double().cpu()[:, None, :]
        return (w * a).sum(-1), (w.abs() * a.abs()).sum(-1), C
    g = G[..., :C].double().cpu()
    w, wabs = g.sum(1, keepdim=True) / HW, g.abs().sum(1, keepdim=True) / HW
    return (w * a).sum(-1), (wabs * a.abs()).sum(-1), C + HW + 1


# ------------------------------------------------------------------ xcp_cam_render
def _lin_idx(out, inn, dtype):
    """ATen's upsample_bilinear2d (align_corners=False) source index and weights, computed in ``dtype`` in the
    kernel's order of operations"""
    scale = torch.tensor(float(inn), dtype=dtype) / torch.tensor(float(out), dtype=dtype)
    src = (scale * (torch.arange(out, dtype=dtype) + 0.5) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(inn - 1)
    i1 = i0 + (i0 < inn - 1).long()
    l1 = (src - i0.to(dtype)).clamp(0, 1)
    return i0, i1, 1 - l1, l1


def render_reference(raw, size, lengths=None, normalize=True, dtype=torch.float32):
    """raw [B, T, h, w] -> [B, T, OH, OW] in ``dtype`` (CPU), the kernel's operations in its order: relu, the
    division by the low-resolution maximum, then (a w0 + b w1) h0 + (c w0 + d w1) h1, products before sums,
    each operation rounded once (torch's element-wise CPU kernels fuse nothing).  In fp32 it is the kernel bit
    for bit; in fp64 it is F.interpolate(relu(raw)) / max up to fp64 rounding."""
    r = torch.relu(raw.detach().cpu().to(dtype))
    B, T, h, w = r.shape
    OH, OW = size
    if normalize:
        m = r.amax((2, 3), keepdim=True)
        r = torch.where(m > 0, r / torch.where(m > 0, m, torch.ones_like(m)), r)
    h0, h1, lh0, lh1 = _lin_idx(OH, h, dtype)
    w0, w1, lw0, lw1 = _lin_idx(OW, w, dtype)
    top, bot = r[:, :, h0, :], r[:, :, h1, :]
    t0 = top[..., w0] * lw0 + top[..., w1] * lw1
    t1 = bot[..., w0] * lw0 + bot[..., w1] * lw1
    out = t0 * lh0[:, None] + t1 * lh1[:, None]
    if lengths is not None:
        keep = torch.arange(T)[None, :] < torch.as_tensor(lengths).cpu()[:, None]
        out = out * keep[:, :, None, None].to(dtype)
    return out


# ------------------------------------------------------------------ layouts
def to_nchw(t, N, h, w, C, CP):
    """engine NHWC at pitch CP (flat or shaped) -> [N, C, h, w] fp32"""
    return t.reshape(N, h, w, CP)[..., :C].permute(0, 3, 1, 2).float()
