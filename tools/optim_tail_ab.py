"""A/B of the optimiser tail of the train_au_face.py step (BASELINE config C5) on the C5 model's real
parameter set -- AUFaceCrossDetector(num_aus=17) + embed head + ArcFace head, gradients filled with
seeded noise, no forward or backward:

  (a) torch:  scaler.unscale_, clip_grad_norm_(1.0), scaler.step(torch.optim.AdamW), scaler.update,
              two AveragedModel.update_parameters               (AUFaceTrainer's default tail)
  (b) fused:  scaler.step(FusedAdamClip(AdamW, clip inside, capturable)), scaler.update,
              two FusedAveragedModel.update_parameters           (AUFaceTrainer(fused_optimizer=True))

Each repetition is bracketed by HIP events on one stream; the two paths alternate in one process (5
warm-ups, 20 timed repetitions each by default).  The gradients are rewritten (scaled noise) before
every repetition, outside the timed window.  The host time spent issuing each tail is recorded beside
the event time (a tail whose two numbers agree is bound by the host, not by HBM).  Prints one JSON
line; --out writes it to a file too.

usage: python tools/optim_tail_ab.py [--reps 20] [--warmup 5] [--out FILE]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "multimodal-deepfake-detection_amd"), REPO]


class Tail:
    def __init__(self, modules, fused, noise, scale):
        from torch.optim.swa_utils import AveragedModel
        from xcp.optim import FusedAdamClip, FusedAveragedModel
        self.model, self.embed, self.arc = modules
        self.params = [p for m in modules for p in m.parameters()]
        dev = self.params[0].device
        n = sum(p.numel() for p in self.params)
        self.flat = torch.zeros(n, device=dev)   # one flat gradient buffer, as xcp.ddp.GradBuckets keeps
        o = 0
        for p in self.params:
            p.grad = self.flat[o:o + p.numel()].view(p.shape)
            o += p.numel()
        self.noise, self.fused = noise, fused
        averaged = FusedAveragedModel if fused else AveragedModel
        self.avg_model, self.avg_embed = averaged(self.model).to(dev), averaged(self.embed).to(dev)
        if fused:
            self.opt = FusedAdamClip(self.params, lr=1e-4, weight_decay=0.01, max_norm=1.0, decoupled_weight_decay=True,
                                     capturable=True)
        else:
            self.opt = torch.optim.AdamW(self.params, lr=1e-4, weight_decay=0.01)
        self.scaler = torch.amp.GradScaler(init_scale=scale)
        self.scaler.scale(torch.zeros((), device=dev))   # creates the scale tensor
        self.scale = scale
        self.enqueue_ms = []

    def fill(self):
        torch.mul(self.noise, self.scale, out=self.flat)

    def run(self):
        if not self.fused:
            self.scaler.unscale_(self.opt)
            torch.nn.utils.clip_grad_norm_(self.params, 1.0)
        self.scaler.step(self.opt)
        self.scaler.update()
        self.avg_model.update_parameters(self.model)
        self.avg_embed.update_parameters(self.embed)

    def timed(self):
        self.fill()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        t0 = time.perf_counter()
        self.run()
        self.enqueue_ms.append((time.perf_counter() - t0) * 1e3)   # host time to issue the tail
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)


def stats(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4), "all_ms": [round(t, 4) for t in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_tail_ab: needs the GPU (HIP events); there is nothing to time on the CPU")
    from Models.AUFaceModel import AUFaceCrossDetector
    from xcp.heads import ArcFaceHead
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = AUFaceCrossDetector(num_aus=17)
    embed = nn.Sequential(nn.Linear(1024, 256), nn.ReLU(inplace=True), nn.Dropout(0.2), nn.Linear(256, 128))
    arc = ArcFaceHead(feat_dim=128, num_classes=2, s=30.0, m=0.30)
    mods_a = [m.to(dev) for m in (model, embed, arc)]
    mods_b = [copy.deepcopy(m) for m in mods_a]
    n = sum(p.numel() for m in mods_a for p in m.parameters())
    noise = 1e-3 * torch.randn(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    a, b = Tail(mods_a, False, noise, 2.0 ** 8), Tail(mods_b, True, noise, 2.0 ** 8)
    for _ in range(args.warmup):
        a.timed()
        b.timed()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(a.timed())
        tb.append(b.timed())
    # the two tails computed the same thing (clip + AdamW + equal average, every repetition a real step)
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(a.params, b.params))
    steps = {float(b.opt.state[p]["step"]) for p in b.params}
    res = {"what": "optimiser tail of the C5 step: unscale, clip 1.0, AdamW, scaler.update, two averaged-model updates",
           "device": torch.cuda.get_device_name(0), "parameters": n, "tensors": len(a.params),
           "reps": args.reps, "warmup": args.warmup, "scale": 2.0 ** 8,
           "torch_tail": stats(ta), "fused_tail": stats(tb),
           "torch_tail_host_enqueue_median_ms": round(statistics.median(a.enqueue_ms[-args.reps:]), 4),
           "fused_tail_host_enqueue_median_ms": round(statistics.median(b.enqueue_ms[-args.reps:]), 4),
           "fused_over_torch_median": round(statistics.median(tb) / statistics.median(ta), 4),
           "max_abs_param_difference_after": worst, "fused_step_counts": sorted(steps),
           "scales_after": [a.scaler.get_scale(), b.scaler.get_scale()]}
    c5 = os.path.join(REPO, "profiles", "r06_v6_auface.json")
    if os.path.exists(c5):
        mb = json.load(open(c5))["ms_per_step"]
        res["c5_micro_batch_ms"] = mb
        res["torch_tail_share_of_micro_batch"] = round(statistics.median(ta) / mb, 4)
        res["fused_tail_share_of_micro_batch"] = round(statistics.median(tb) / mb, 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
