"""NIQE against producing the frames it scores, on one GPU: 7 x 3 x 720 x 1280 (BASELINE configs[1]'s item) and
1 x 3 x 2160 x 3840.

  (a) forward   the x4 model on the 1 x 7 x 3 x 180 x 320 clip (the 720p item only)
  (b) kernels   `ops.niqe_moments` at scale 1 (fp32 frames, block 96), `ops.niqe_half`, `ops.niqe_moments` at scale 2 (fp64 plane,
                block 48): wall clock and device events, as a share of HBM peak on their algorithmic bytes (every input sample
                read once, every output written once)
  (c) torch     the same maps restated with torch on the device: fp64 `conv2d` for mu and sigma, `unfold` into blocks, `roll`,
                masked sums (the resize is not restated); close to (b), not equal
  (d) host      `NIQE.scores` on the moments read back: features and the distance, numpy
  (e) whole     `NIQE(...)(frames)`: launches, one read-back, host part

Wall times: after --warmup calls, the median of --reps calls, each with a device synchronise on both sides.  No figure is set in
advance: the file records what was measured.  The pristine model is synthetic (none ships); the score's value means nothing here.

    python tools/gpu_niqe_time.py [--reps 20] [--warmup 3] [--out FILE]
    python tools/gpu_niqe_time.py --parity [--out FILE]

--parity instead writes profiles/r23_niqe_parity.json: the largest relative difference between `NIQE(...)` and the float64
restatement (tests/niqe_ref.py) over the images of tests/test_hip_niqe.py, which sets that test's bound (ten times the figure).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"720p_item": (7, 3, 720, 1280), "2160p_frame": (1, 3, 2160, 3840)}


def wall(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": reps}


def model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (36, 36))
    return rng.normal(0, 1, 36), a @ a.T + np.eye(36)


def torch_moments(plane, block):
    """plane (N, 1, h, w) fp64 -> (N, blocks, 25) by torch ops: conv2d with the 7 x 7 window on a replicate-padded plane, unfold"""
    from eavsr_amd.niqe import gaussian_window
    g = torch.from_numpy(gaussian_window()[1].copy()).to(plane.device)[None, None]
    pad = F.pad(plane, (3, 3, 3, 3), mode="replicate")
    mu = F.conv2d(pad, g)
    sigma = (F.conv2d(pad * pad, g) - mu * mu).abs().sqrt()
    m = (plane - mu) / (sigma + 1)
    n = plane.shape[0]
    blocks = F.unfold(m, block, stride=block).view(n, block, block, -1).permute(0, 3, 1, 2)      # (N, blocks, p, p)
    out = []
    for v in [blocks] + [blocks * torch.roll(blocks, s, dims=(2, 3)) for s in ((0, 1), (1, 0), (1, 1), (1, -1))]:
        neg, pos, sq = v < 0, v > 0, v * v
        out += [neg.sum((2, 3)).double(), pos.sum((2, 3)).double(), (sq * neg).sum((2, 3)), (sq * pos).sum((2, 3)), v.abs().sum((2, 3))]
    return torch.stack(out, -1)


def device_us(ops, name, fn, reps):
    us = []
    for _ in range(reps):
        with ops.profile() as prof:
            fn()
            us.append(prof.summary()[name]["ms"] * 1e3)
    return {"device_median_us": round(statistics.median(us), 2), "device_min_us": round(min(us), 2), "device_max_us": round(max(us), 2)}


def parity(out_path):
    from eavsr_amd.niqe import NIQE
    from tests import niqe_ref as R
    from tests.test_hip_niqe import SCORE_CASES
    mu_p, cov_p = model()
    scorer = NIQE((mu_p, cov_p))
    rows = []
    for c, h, w, seed, border in SCORE_CASES:
        img = R.test_image(c, h, w, seed)
        want, margin, bad = R.niqe(img, mu_p, cov_p, 255.0, border)
        got = scorer(torch.from_numpy(img[None]).cuda(), 255.0, border)[0]
        rows.append({"case": [c, h, w, seed, border], "device": got, "reference": want, "rel_diff": abs(got - want) / want,
                     "smallest_fit_margin": float(margin), "nan_rows": bad})
    res = {"device": torch.cuda.get_device_name(0), "cases": rows, "max_rel_diff": max(r["rel_diff"] for r in rows),
           "note": "NIQE(...) on the device against tests/niqe_ref.py (float64, block arrays); synthetic pristine model"}
    txt = json.dumps(res, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernels' fractions are quoted against, TB/s")
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parity:
        return parity(a.out or os.path.join(ROOT, "profiles", "r23_niqe_parity.json"))
    from eavsr_amd import ops
    from eavsr_amd.niqe import NIQE, resize_tables
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    dev = torch.device("cuda:0")
    scorer = NIQE(model())
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup, "peak_tbs": a.peak_tbs,
           "timing": "wall clock, device synchronise on both sides, median of reps; device events around each C-ABI call",
           "weights": "synthetic (EAVSRP trained_like); synthetic pristine model"}
    for tag, (n, c, h, w) in SHAPES.items():
        out = {"frames": [n, c, h, w]}
        if tag == "720p_item":
            from eavsr_amd.eavsrp_model import EAVSRP
            net = EAVSRP(Namespace(predict=False, n_frame=n, n_flow=5, scale=4), None)
            sd0 = net.state_dict()
            net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
            net = net.to(dev).eval()
            lr = synthetic_clip(1, n, h // 4, w // 4, seed=1).to(dev)
            with torch.no_grad():
                out["a_forward"] = wall(lambda: net(lr), a.reps, a.warmup)
                frames = net(lr).detach().clamp(0, 1).reshape(n, c, h, w).contiguous()
            del net
        else:
            frames = synthetic_clip(1, n, h, w, seed=3).to(dev).reshape(n, c, h, w).contiguous()
        bh, bw = h // 96, w // 96
        ch, cw = bh * 96, bw * 96
        px = n * ch * cw
        _, luma = ops.niqe_moments(frames)
        tables = ops.niqe_half_tables(resize_tables(ch), resize_tables(cw), dev)
        half = ops.niqe_half(luma, tables)
        steps = {"moments_scale1": ("niqe_moments", lambda: ops.niqe_moments(frames), px * (4 * c + 8) + n * bh * bw * 200),
                 "half": ("niqe_half", lambda: ops.niqe_half(luma, tables), px * 8 + px * 2),
                 "moments_scale2": ("niqe_moments", lambda: ops.niqe_moments(half, 1.0, 48), px * 2 + n * bh * bw * 200)}
        for name, (op, fn, algo) in steps.items():
            row = dict(wall(fn, a.reps, a.warmup))
            row.update(device_us(ops, op, fn, a.reps))
            row.update(algorithmic_bytes=algo, algorithmic_GBs=round(algo / row["device_median_us"] / 1e3, 1),
                       fraction_of_peak=round(algo / (row["device_median_us"] * 1e-6) / (a.peak_tbs * 1e12), 4))
            out["b_" + name] = row
            print(json.dumps({tag + " " + name: row["device_median_us"]}), flush=True)
        out["c_torch_scale1"] = wall(lambda: torch_moments(luma, 96), max(3, a.reps // 4), 1)
        out["c_torch_scale2"] = wall(lambda: torch_moments(half, 48), max(3, a.reps // 4), 1)
        t1, k1 = torch_moments(luma, 96), ops.niqe_moments(frames)[0].view(n, -1, 25)
        out["c_torch_scale1"].update(count_differs_by=float((t1[..., 0] - k1[..., 0]).abs().max()),
                                     sums_rel_diff=float(((t1 - k1).abs() / k1.abs().clamp_min(1e-300)).max()),
                                     note="fp64 torch ops, a 49-tap window and another summation order: near the kernel, not equal")
        del t1
        moments = scorer.moments(frames).cpu().numpy()
        ts = []
        for _ in range(max(3, a.reps // 4)):
            t0 = time.perf_counter()
            scorer.scores(moments)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["d_host_scores"] = {"median_ms": round(statistics.median(ts), 3), "blocks_per_frame": bh * bw}
        out["e_niqe_whole"] = wall(lambda: scorer(frames), a.reps, a.warmup)
        if "a_forward" in out:
            out["e_over_a"] = round(out["e_niqe_whole"]["median_ms"] / out["a_forward"]["median_ms"], 4)
        res[tag] = out
        del frames, luma, half
        torch.cuda.empty_cache()
    txt = json.dumps(res, indent=1)
    print(txt)
    path = a.out or os.path.join(ROOT, "profiles", "r23_niqe_time.json")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
