"""The opt-in bf16 training mode (networks.set_train_precision) against the default fp32 mode at configs[3]: the graphed training
step (graph.GraphedTrainStep: 2 clips x 7 frames, LR 96 x 96 -> HR 384 x 384, L1, Adam), the two modes in alternating order
(A/B, B/A, ..) over --rounds rounds of --steps timed replays each (every switch recaptures the graph, then two untimed replays);
medians and ranges per mode.  --kernels adds device-event times of the two kernel families the mode changes, per launch at the
crop: the 2 x 64 x 96 x 96 forward convolution (exact eavsr_conv3x3_f32x6s against eavsr_conv3x3_bf16x1s) and the 7-segment
3x3 weight gradient with its reduction (eavsr_conv_wgrad_bias_multi_f32 against _bf16).

    python tools/gpu_train_precision_time.py [--rounds 5] [--steps 10] [--kernels] [--modes fp32,bf16] [--out FILE]

`rocprofv3 --kernel-trace --stats -- python tools/gpu_train_precision_time.py --modes bf16 --rounds 1` names the kernels of
the bf16 step (no --pmc in the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us per call


def time_kernels(dev, iters=200, rounds=5):
    from eavsr_amd import ops
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 64, 96, 96, generator=g).to(dev)
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(dev)
    b = torch.randn(64, generator=g).to(dev)
    dys = [torch.randn(2, 64, 96, 96, generator=g).to(dev) for _ in range(7)]
    xs = [[torch.randn(2, 64, 96, 96, generator=g).to(dev)] for _ in range(7)]
    dw, db = torch.empty(64, 64, 3, 3, device=dev), torch.empty(64, device=dev)
    res = {k: [] for k in ("conv_fp32_us", "conv_bf16_us", "wgrad7_fp32_us", "wgrad7_bf16_us")}
    for _ in range(rounds):
        res["conv_fp32_us"].append(_events(lambda: ops.conv2d(x, w, b, act="relu"), iters))
        res["conv_bf16_us"].append(_events(lambda: ops.conv2d(x, w, b, act="relu", precision="bf16"), iters))
        res["wgrad7_fp32_us"].append(_events(lambda: ops.conv_wgrad_multi(dys, xs, 3, out=dw, bias_out=db), iters // 4))
        res["wgrad7_bf16_us"].append(_events(lambda: ops.conv_wgrad_multi(dys, xs, 3, out=dw, bias_out=db, precision="bf16"), iters // 4))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in res.items()}


def time_train(dev, modes, rounds, steps):
    from eavsr_amd import networks as Nw
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import synthetic_clip
    opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350)
    model = EAVSRPModel(opt)
    data = {"lr_seq": synthetic_clip(2, 7, 96, 96, seed=1), "hr_seq": synthetic_clip(2, 7, 384, 384, seed=2), "fname": "x"}
    model.set_input(data, epoch=0)
    times = {m: [] for m in modes}
    losses = {m: [] for m in modes}
    with Nw.train_precision(modes[0]):
        step = GraphedTrainStep(model, warmup=2)
    try:
        for r in range(rounds):
            for mode in (modes if r % 2 == 0 else modes[::-1]):
                with Nw.train_precision(mode):
                    step.step()                  # recaptures when the mode changed
                    step.step()
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(steps):
                        step.step()
                    e1.record()
                    torch.cuda.synchronize()
                    times[mode].append(e0.elapsed_time(e1) / steps)
                    losses[mode].append(model.get_current_losses()["EAVSRP_L1"])
    finally:
        step.close()
    out = {}
    for m in modes:
        v = times[m]
        out[m] = {"step_ms_median": round(statistics.median(v), 2), "step_ms_min": round(min(v), 2), "step_ms_max": round(max(v), 2),
                  "lr_frames_per_s": round(2 * 7 / (statistics.median(v) * 1e-3), 1), "rounds_ms": [round(t, 2) for t in v],
                  "last_l1": [round(x, 6) for x in losses[m]]}
    if len(modes) == 2:
        out["bf16_over_fp32"] = round(out["bf16"]["step_ms_median"] / out["fp32"]["step_ms_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    modes = a.modes.split(",")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "config": "configs[3]: graphed training step, 2 clips x 7 frames, LR 96x96 -> HR 384x384, L1, Adam",
           "rounds": a.rounds, "steps_per_round": a.steps, "order": "alternating (A/B, B/A, ..); each switch recaptures"}
    if a.kernels:
        res["kernels_per_launch"] = time_kernels(dev)
        print(json.dumps(res["kernels_per_launch"]), flush=True)
    res["train"] = time_train(dev, modes, a.rounds, a.steps)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
