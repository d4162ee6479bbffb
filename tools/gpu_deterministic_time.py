"""The opt-in deterministic training mode (networks.set_deterministic) against the default mode at configs[3], in fp32 and in
bf16 training precision: the graphed training step (graph.GraphedTrainStep: 2 clips x 7 frames, LR 96 x 96 -> HR 384 x 384, L1,
Adam), default and deterministic in alternating order (A/B, B/A, ..) over --rounds rounds of --steps timed replays each (every
switch recaptures the graph, then two untimed replays); medians and ranges per (precision, mode).  --kernels adds device-event
times per launch of the three backward ops the mode changes, at their configs[3] shapes, atomic against deterministic.

    python tools/gpu_deterministic_time.py [--rounds 5] [--steps 10] [--precisions fp32,bf16] [--only det] [--kernels] [--out FILE]

`rocprofv3 --kernel-trace --stats -- python tools/gpu_deterministic_time.py --precisions fp32 --only det --rounds 1` names the
kernels of the deterministic step (no --pmc in the same run).
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


def time_kernels(dev, iters=100, rounds=5):
    from eavsr_amd import autograd as AG, ops
    g = torch.Generator().manual_seed(0)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
    # flow_warp: 2 x 64 x 96 x 96 features, flows of a few pixels; resize: x0.25 of a 2 x 144 x 96 x 96 offset field; DCNv2: 2 x 64 x 96 x 96
    x, flow, dout = r(2, 64, 96, 96), r(2, 2, 96, 96, k=2.0), r(2, 64, 96, 96)
    rs_out = r(2, 144, 24, 24)
    off, mask, wt = r(2, 144, 96, 96, k=2.0), torch.rand(2, 72, 96, 96, generator=g).to(dev), r(64, 64, 3, 3, k=1 / 24)
    res = {k: [] for k in ("flow_warp_dx_atomic_us", "flow_warp_dx_det_us", "resize_bwd_atomic_us", "resize_bwd_det_us",
                           "dcn_bwd_atomic_us", "dcn_bwd_det_us")}
    for _ in range(rounds):
        res["flow_warp_dx_atomic_us"].append(_events(lambda: ops.flow_warp_bwd(x, flow, None, dout, True, False), iters))
        res["flow_warp_dx_det_us"].append(_events(lambda: ops.flow_warp_bwd_dx_det(flow, None, dout), iters))
        res["resize_bwd_atomic_us"].append(_events(lambda: ops.resize_bilinear_ac_bwd(rs_out, (2, 144, 96, 96), 0.25), iters))
        res["resize_bwd_det_us"].append(_events(lambda: ops.resize_bilinear_ac_bwd_det(rs_out, (2, 144, 96, 96), 0.25), iters))
        res["dcn_bwd_atomic_us"].append(_events(lambda: ops.dcnv2_bwd(x, off, mask, wt, dout, 8, need_dx=True), iters // 4))
        res["dcn_bwd_det_us"].append(_events(lambda: (ops.dcnv2_bwd(x, off, mask, wt, dout, 8, need_dx=False),
                                                      ops.dcnv2_col2im_dx_det(off, mask, ops.conv2d(dout, AG._dcn_wt(wt), None), 8)),
                                             iters // 4))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in res.items()}


def time_train(dev, precision, modes, rounds, steps):
    from eavsr_amd import networks as Nw
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import synthetic_clip
    opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350)
    times = {m: [] for m in modes}
    losses = {m: [] for m in modes}
    with Nw.train_precision(precision):
        model = EAVSRPModel(opt)
        data = {"lr_seq": synthetic_clip(2, 7, 96, 96, seed=1), "hr_seq": synthetic_clip(2, 7, 384, 384, seed=2), "fname": "x"}
        model.set_input(data, epoch=0)
        with Nw.deterministic(modes[0] == "det"):
            step = GraphedTrainStep(model, warmup=2)
        try:
            for r in range(rounds):
                for mode in (modes if r % 2 == 0 else modes[::-1]):
                    with Nw.deterministic(mode == "det"):
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
                  "rounds_ms": [round(t, 2) for t in v], "last_l1": [round(x, 6) for x in losses[m]]}
    if len(modes) == 2:
        out["det_over_default"] = round(out["det"]["step_ms_median"] / out["default"]["step_ms_median"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--only", default="", help="det or default: time one mode only")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    modes = [a.only] if a.only else ["default", "det"]
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "config": "configs[3]: graphed training step, 2 clips x 7 frames, LR 96x96 -> HR 384x384, L1, Adam",
           "rounds": a.rounds, "steps_per_round": a.steps, "order": "alternating (A/B, B/A, ..); each switch recaptures"}
    if a.kernels:
        res["kernels_per_launch"] = time_kernels(dev)
        print(json.dumps(res["kernels_per_launch"]), flush=True)
    res["train"] = {}
    for p in a.precisions.split(","):
        res["train"][p] = time_train(dev, p, modes, a.rounds, a.steps)
        print(json.dumps({p: res["train"][p]}), flush=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
