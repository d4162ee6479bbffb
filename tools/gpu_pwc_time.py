"""Cost of the late-training PWC-Net mask (eavsr_amd/pwc.py) at configs[3] (2 clips x 7 frames, LR 96 x 96, x4):

  1. get_backwarp for the 14 frame pairs, device events around 20 calls after warm-up, and the per-launch ops.profile() table
     (each eavsr_pwc_conv3x3_f32 launch shape with its achieved TF/s against the 157 TF/s fp32 matrix peak);
  2. the graphed training step (graph.GraphedTrainStep) at epoch < npost and at epoch >= npost.

    python tools/gpu_pwc_time.py [--out pwc_time.json] [--steps 10] [--only-backwarp]

`rocprofv3 --kernel-trace --stats -- python tools/gpu_pwc_time.py --only-backwarp` names the kernels.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFS = 157.0


def weights():
    from eavsr_amd.pwc import PWCNET
    from eavsr_amd.utils.synthetic import fill_state_dict
    shapes = {k: tuple(v.shape) for k, v in PWCNET().state_dict().items()}
    return fill_state_dict(shapes, "default", seed=7)


def time_backwarp(dev, iters=20):
    from eavsr_amd import ops, pwc
    from eavsr_amd.utils.synthetic import synthetic_clip
    net = pwc.PWCNET()
    net.load_state_dict(weights())
    net = net.to(dev).eval()
    lr = synthetic_clip(2, 7, 96, 96, seed=1).reshape(14, 3, 96, 96).to(dev)
    hr = synthetic_clip(2, 7, 384, 384, seed=2).reshape(14, 3, 384, 384).to(dev)
    for _ in range(3):
        pwc.get_backwarp(lr, hr, net, 4)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        pwc.get_backwarp(lr, hr, net, 4)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    with ops.profile() as prof:
        pwc.get_backwarp(lr, hr, net, 4)
    summ = prof.summary()
    kernels = {k: {"calls": v["calls"], "ms": round(v["ms"], 4), "gflop": round(v["flops"] / 1e9, 3)} for k, v in summ.items()}
    # per conv launch: group by (algorithmic flops) = by launch shape
    convs = []
    for flops, (calls, cms) in sorted(prof.by_flops("pwc_conv3x3").items(), key=lambda kv: -kv[0]):
        us = cms / calls * 1e3
        tfs = flops / (us * 1e-6) / 1e12
        convs.append({"gflop": round(flops / 1e9, 4), "calls": calls, "us_per_call": round(us, 1), "tf_s": round(tfs, 2),
                      "frac_of_peak": round(tfs / PEAK_TFS, 4)})
    total_flop = sum(v["flops"] for v in summ.values())
    return {"get_backwarp_ms": round(ms, 3), "launches": sum(v["calls"] for v in summ.values()),
            "gflop": round(total_flop / 1e9, 2), "kernels": kernels, "conv_launches": convs}


def time_train(dev, steps=10):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:      # the weights are read at the first masked forward (the recapture)
        path = os.path.join(tmp, "pwc-default")
        torch.save({k.replace("net", "module"): v for k, v in weights().items()}, path)
        opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9,
                        beta2=0.999, weight_decay=0.0, npost=350, load_path="", pwc_path=path)
        return _time_train(EAVSRPModel(opt), steps)


def _time_train(model, steps):
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import synthetic_clip
    data = {"lr_seq": synthetic_clip(2, 7, 96, 96, seed=1), "hr_seq": synthetic_clip(2, 7, 384, 384, seed=2), "fname": "x"}
    model.set_input(data, epoch=349)
    step = GraphedTrainStep(model, warmup=2)
    out = {}
    try:
        for epoch, key in ((349, "train_step_ms_unmasked"), (350, "train_step_ms_masked")):
            step.step(epoch=epoch)          # the first call at 350 recaptures
            step.step(epoch=epoch)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                step.step(epoch=epoch)
            e1.record()
            torch.cuda.synchronize()
            out[key] = round(e0.elapsed_time(e1) / steps, 2)
        out["mask_fraction"] = round(float(model.mask.float().mean()), 4)
    finally:
        step.close()
    out["masked_over_unmasked"] = round(out["train_step_ms_masked"] / out["train_step_ms_unmasked"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only-backwarp", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "config": "configs[3]: 2 clips x 7 frames, LR 96x96 -> HR 384x384",
           "backwarp": time_backwarp(dev)}
    if not a.only_backwarp:
        res["train"] = time_train(dev, a.steps)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
