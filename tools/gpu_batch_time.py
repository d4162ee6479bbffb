"""What building a training batch costs: the gather kernel (`ops.gather_pairs`, csrc/batch.hip) against a torch restatement on the
device and against the host path the reference takes, and the graphed training step fed by `dataset.TrainBatches`.

  --part gather   for two batches -- 2 x 7, patch 96, x4 (BASELINE configs[3]'s) and 8 x 7, patch 64, x2 -- and each of the 8 flag
                  combinations (every sample of the batch carries the same flags; origins and windows are drawn as `epoch_plan`
                  draws them):
                    kernel   one `ops.gather_pairs` into preallocated outputs
                    torch    the same batch by torch on the device, built here: per sample and resolution `index_select` of the
                             window, slice, `flip`, `transpose`, a converting `copy_` into the output (which makes it contiguous),
                             then one in-place division by a 0-dim device tensor 255 per resolution (a true division; a Python
                             scalar divisor is multiplied by its reciprocal); `torch.equal` to the kernel's output is recorded
                  Device events around --launches back-to-back calls, microseconds per call; --rounds rounds, the variants
                  alternated inside a round; the median over the rounds.  Fraction of --peak-tbs on 5 bytes per produced sample.
                    host     the reference's path, restated here in numpy on uint8 frames in host memory (one process, no DataLoader
                             workers): per item `np.float32(frame) / 255` on the window's FULL frames, crop, flips +
                             `np.ascontiguousarray`, `np.stack`; collate (`np.stack` over the items), pin, H2D, synchronise.
                             Wall clock, median of --rounds; flags 0 and 7 only (the host's cost does not depend on the kernel).
  --part step     BASELINE configs[3]'s graphed training step (`graph.GraphedTrainStep`, 2 x 7 x 3 x 96 x 96 -> 384 x 384):
                    fixed    replaying the batch that is in the static buffers
                    fed      every step preceded by one gather straight into the static buffers (`TrainBatches(out=...)`)
                    copied   `step(batch)` with batches `TrainBatches` allocates (gather + the step's two copies)
                  Wall clock over --steps steps with a device synchronise on both sides, ms per step; --rounds rounds, the
                  variants alternated inside a round; medians.

Results are merged into --out (JSON), so the two parts can run as two processes, each under its own time limit:

    timeout -k 10 300 python tools/gpu_batch_time.py --part gather --out profiles/r13_batch_time.json && \
    timeout -k 10 420 python tools/gpu_batch_time.py --part step --out profiles/r13_batch_time.json

`rocprofv3 --kernel-trace --stats -- python tools/gpu_batch_time.py --part gather --rounds 1` names the kernels (no --pmc in the
same run).
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SEQ, T = 50, 7
SHAPES = [dict(tag="2x7_p96_x4", n=2, patch=96, scale=4, h=180, w=320), dict(tag="8x7_p64_x2", n=8, patch=64, scale=2, h=360, w=640)]


def byte_frames(f, h, w, seed):
    """(F, 3, h, w) uint8: the synthetic clip of the benchmarks, quantised"""
    from eavsr_amd.utils.synthetic import synthetic_clip
    clips = [(synthetic_clip(1, T, h, w, seed=100 * seed + i)[0] * 255.0).round().clamp(0, 255).to(torch.uint8) for i in range((f + T - 1) // T)]
    return torch.cat(clips)[:f].contiguous()


def plan(n, patch, h, w, flags, seed):
    from eavsr_amd import dataset, harness
    rng = random.Random(seed)
    keys = [rng.randrange(N_SEQ) for _ in range(n)]
    frames = np.asarray([harness.train_window(k, k % N_SEQ, T, N_SEQ) for k in keys], np.int32)
    desc = np.zeros((n, 4), np.int32)
    for i in range(n):
        desc[i, :2] = dataset.draw_item(rng, h, w, patch)[:2]
    desc[:, 2] = flags
    dataset.check_plan(frames, desc, N_SEQ, h, w, patch)
    return frames, desc


def torch_batch(store, frames_dev, desc, patch, s, out, divisor):
    for i, (top, left, flags, _) in enumerate(desc.tolist()):
        v = store.index_select(0, frames_dev[i])[:, :, s * top:s * (top + patch), s * left:s * (left + patch)]
        if flags & 1:
            v = v.flip(3)
        if flags & 2:
            v = v.flip(2)
        if flags & 4:
            v = v.transpose(2, 3)
        out[i].copy_(v)
    out.div_(divisor)      # a 0-dim device tensor: a true division (a Python scalar becomes a multiply by 1 / 255)


def host_batch(lr, hr, frames, desc, patch, s, dev):
    """the reference's item (realvsr_dataset.py:62-94, util.py:223-248) and collate on host arrays, then pinned H2D"""
    def aug(img, flags):
        if flags & 1:
            img = img[:, :, ::-1]
        if flags & 2:
            img = img[:, ::-1, :]
        if flags & 4:
            img = img.transpose(0, 2, 1)
        return np.ascontiguousarray(img)
    items_lr, items_hr = [], []
    for win, (top, left, flags, _) in zip(frames.tolist(), desc.tolist()):
        lr_seq = [np.float32(lr[k]) / 255 for k in win]
        hr_seq = [np.float32(hr[k]) / 255 for k in win]
        lr_seq = [v[..., top:top + patch, left:left + patch] for v in lr_seq]
        hr_seq = [v[..., s * top:s * (top + patch), s * left:s * (left + patch)] for v in hr_seq]
        items_lr.append(np.stack([aug(v, flags) for v in lr_seq], 0))
        items_hr.append(np.stack([aug(v, flags) for v in hr_seq], 0))
    a = torch.from_numpy(np.stack(items_lr, 0)).pin_memory().to(dev, non_blocking=True)
    b = torch.from_numpy(np.stack(items_hr, 0)).pin_memory().to(dev, non_blocking=True)
    torch.cuda.synchronize()
    return a, b


def event_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def med(v):
    return round(statistics.median(v), 3)


def part_gather(a, res):
    from eavsr_amd import ops
    dev = torch.device("cuda:0")
    divisor = torch.full((), 255.0, device=dev)
    res["gather"] = {"timing": f"device events around {a.launches} back-to-back calls, us per call; median of {a.rounds} rounds, variants "
                               "alternated inside a round", "peak_tbs": a.peak_tbs, "bytes_per_sample": 5, "shapes": {}}
    for sh in SHAPES:
        n, patch, s, h, w = sh["n"], sh["patch"], sh["scale"], sh["h"], sh["w"]
        lr_host, hr_host = byte_frames(N_SEQ, h, w, seed=1), byte_frames(N_SEQ, s * h, s * w, seed=2)
        lr, hr = lr_host.to(dev), hr_host.to(dev)
        out_k = (torch.empty((n, T, 3, patch, patch), device=dev), torch.empty((n, T, 3, s * patch, s * patch), device=dev))
        out_t = (torch.empty_like(out_k[0]), torch.empty_like(out_k[1]))
        samples = out_k[0].numel() + out_k[1].numel()
        row = {"n": n, "t": T, "patch": patch, "scale": s, "lr_frame": [h, w], "store_frames": N_SEQ, "samples": samples, "flags": {}}
        for flags in range(8):
            frames, desc = plan(n, patch, h, w, flags, seed=100 + flags)
            frames_dev, desc_dev = torch.from_numpy(frames).to(dev), torch.from_numpy(desc).to(dev)
            kernel = lambda: ops.gather_pairs(lr, hr, frames_dev, desc_dev, patch, s, out=out_k)

            def restated():
                torch_batch(lr, frames_dev, desc, patch, 1, out_t[0], divisor)
                torch_batch(hr, frames_dev, desc, patch, s, out_t[1], divisor)
            for _ in range(3):
                kernel()
                restated()
            equal = bool(torch.equal(out_k[0], out_t[0]) and torch.equal(out_k[1], out_t[1]))
            us = {"kernel": [], "torch": []}
            for _ in range(a.rounds):
                us["kernel"].append(event_us(kernel, a.launches))
                us["torch"].append(event_us(restated, a.launches))
            k, t_ = med(us["kernel"]), med(us["torch"])
            entry = {"kernel_us": k, "kernel_us_rounds": [round(v, 3) for v in us["kernel"]], "torch_us": t_,
                     "torch_us_rounds": [round(v, 3) for v in us["torch"]], "torch_over_kernel": round(t_ / k, 2),
                     "kernel_GBs": round(5 * samples / k / 1e3, 1), "kernel_fraction_of_peak": round(5 * samples / (k * 1e-6) / (a.peak_tbs * 1e12), 4),
                     "kernel_equals_torch": equal}
            if flags in (0, 7):
                ms = []
                host_batch(lr_host.numpy(), hr_host.numpy(), frames, desc, patch, s, dev)
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    got = host_batch(lr_host.numpy(), hr_host.numpy(), frames, desc, patch, s, dev)
                    ms.append((time.perf_counter() - t0) * 1e3)
                entry["host_ms"] = med(ms)
                entry["host_ms_rounds"] = [round(v, 3) for v in ms]
                entry["host_equals_kernel"] = bool(torch.equal(got[0], out_k[0]) and torch.equal(got[1], out_k[1]))
                entry["host_over_kernel"] = round(entry["host_ms"] * 1e3 / k, 1)
            row["flags"][str(flags)] = entry
            print(json.dumps({sh["tag"]: {str(flags): entry}}), flush=True)
        plain = statistics.median([row["flags"][str(f)]["kernel_us"] for f in range(4)])
        transposed = statistics.median([row["flags"][str(f)]["kernel_us"] for f in range(4, 8)])
        row["transposed_over_plain"] = round(transposed / plain, 3)
        row["transposed_over_plain_by_flips"] = {str(f): round(row["flags"][str(f + 4)]["kernel_us"] / row["flags"][str(f)]["kernel_us"], 3)
                                                 for f in range(4)}
        row["kernel_not_above_torch_everywhere"] = all(e["kernel_us"] <= e["torch_us"] for e in row["flags"].values())
        res["gather"]["shapes"][sh["tag"]] = row
        del lr, hr


def part_step(a, res):
    from eavsr_amd import dataset
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of
    dev = torch.device("cuda:0")
    sh = SHAPES[0]
    n, patch, s, h, w = sh["n"], sh["patch"], sh["scale"], sh["h"], sh["w"]
    store = dataset.FramePairs(byte_frames(N_SEQ, h, w, seed=1), byte_frames(N_SEQ, s * h, s * w, seed=2), s, N_SEQ, device=dev)
    opt = Namespace(predict=False, n_frame=T, n_flow=5, scale=s, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350)
    model = EAVSRPModel(opt)
    sd0 = model.netEAVSRP.state_dict()
    model.netEAVSRP.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
    allocating = dataset.TrainBatches(store, n, patch, T, seed=0)
    model.set_input(next(iter(allocating)), epoch=0)
    step = GraphedTrainStep(model, warmup=2)
    into = dataset.TrainBatches(store, n, patch, T, seed=0, out=(step.static_lr, step.static_hr))
    assert len(into) >= a.steps, (len(into), a.steps)

    def fixed():
        for _ in range(a.steps):
            step.step()

    def fed():
        for i, _ in enumerate(into):
            if i == a.steps:
                break
            step.step()

    def copied():
        for i, batch in enumerate(allocating):
            if i == a.steps:
                break
            step.step(batch)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    variants = {"fixed": fixed, "fed": fed, "copied": copied}
    for fn in variants.values():
        fn()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            ms[k].append(wall_ms(fn))
    out = {"timing": f"wall clock over {a.steps} steps, device synchronise on both sides, ms per step; median of {a.rounds} rounds, "
                     "variants alternated inside a round", "batch": [n, T, 3, patch, patch], "scale": s,
           "loss_after": float(model.loss_EAVSRP_L1.item())}
    for k in variants:
        out[k + "_ms"] = med(ms[k])
        out[k + "_ms_rounds"] = [round(v, 3) for v in ms[k]]
    out["fed_minus_fixed_ms"] = round(out["fed_ms"] - out["fixed_ms"], 3)
    out["fed_minus_fixed_percent"] = round(100.0 * (out["fed_ms"] - out["fixed_ms"]) / out["fixed_ms"], 3)
    out["copied_minus_fixed_ms"] = round(out["copied_ms"] - out["fixed_ms"], 3)
    out["fixed_spread_percent"] = round(100.0 * (max(ms["fixed"]) - min(ms["fixed"])) / out["fixed_ms"], 3)
    res["step"] = out
    step.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gather", "step"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fraction is quoted against, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_batch_time: needs a GPU (a measurement does not fall back)")
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    (part_gather if a.part == "gather" else part_step)(a, res)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
