"""What making the LR frames costs: `ops.resize_cubic_u8` (csrc/resize_cubic.hip) at a scene of 50 x 3 x 720 x 1280 bytes -> 180 x 320
(x4) and -> 360 x 640 (x2), against two restatements at the same shape, and `FramePairs.from_wide` end to end.

  kernel     one `ops.resize_cubic_u8` into a preallocated output.  Bytes = F C (H W + h w); fraction of --peak-tbs on those bytes.
  torch      the same filter by torch on the same device, for TIME only (float arithmetic, not bit-exact; the share of samples that
             differ from the kernel's is recorded): bytes -> float, one strided `conv2d` with the 4 x 4 kernel of the half-sample
             case ((-192, 1216, 1216, -192) / 2048 per axis; x2: replicate padding 1, stride 2; x4: stride 4), round, clamp, -> bytes.
  host       the numpy oracle (tests/resample_ref.py) on ONE frame, wall clock.  It is a reference for values, not a fast host
             implementation; OpenCV is not available to this project, so cv2's host time is NOT measured and none is quoted.
  from_wide  a 50-frame scene from PINNED host memory: `upload` = the chunked H2D copies alone, `resize` = the kernel launches alone
             on frames already on the device, `from_wide` = `FramePairs.from_wide(.., hr=None, chunk=16)`, wall clock with a device
             synchronise on both sides.

Device events around --launches back-to-back calls, microseconds per call; --rounds rounds with kernel and torch alternated inside a
round; medians.

    timeout -k 10 400 python tools/gpu_resample_time.py --out profiles/r14_resample_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_SEQ, C, H, W = 50, 3, 720, 1280


def byte_frames(f, h, w, seed):
    """(f, 3, h, w) uint8: the synthetic clip of the benchmarks, quantised"""
    from eavsr_amd.utils.synthetic import synthetic_clip
    t = 5
    clips = [(synthetic_clip(1, t, h, w, seed=100 * seed + i)[0] * 255.0).round().clamp(0, 255).to(torch.uint8) for i in range((f + t - 1) // t)]
    return torch.cat(clips)[:f].contiguous()


def torch_resize(x, scale, weight):
    v = x.reshape(-1, 1, x.shape[2], x.shape[3]).float()
    if scale == 2:
        v = F.pad(v, (1, 1, 1, 1), mode="replicate")
    v = F.conv2d(v, weight, stride=scale)
    return v.round_().clamp_(0, 255).to(torch.uint8).reshape(x.shape[0], x.shape[1], x.shape[2] // scale, x.shape[3] // scale)


def event_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fraction is quoted against, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_resample_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import ops
    from eavsr_amd.dataset import FramePairs
    from tests import resample_ref as R
    dev = torch.device("cuda:0")
    host = byte_frames(N_SEQ, H, W, seed=3)
    x = host.to(dev)
    w1 = torch.tensor([-192.0, 1216.0, 1216.0, -192.0]) / 2048.0
    weight = (w1[:, None] * w1[None, :]).reshape(1, 1, 4, 4).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "frames": [N_SEQ, C, H, W], "peak_tbs": a.peak_tbs,
           "timing": f"device events around {a.launches} back-to-back calls, us per call; median of {a.rounds} rounds, kernel and torch "
                     "alternated inside a round", "cv2_host_time": "not measured: OpenCV is not available to this project", "scales": {}}
    for scale in (4, 2):
        h, w = H // scale, W // scale
        out = torch.empty((N_SEQ, C, h, w), device=dev, dtype=torch.uint8)
        kernel = lambda: ops.resize_cubic_u8(x, (h, w), out=out)
        restated = lambda: torch_resize(x, scale, weight)
        for _ in range(3):
            kernel()
            got_t = restated()
        differ = float((got_t != out).float().mean().item())
        us = {"kernel": [], "torch": []}
        for _ in range(a.rounds):
            us["kernel"].append(event_us(kernel, a.launches))
            us["torch"].append(event_us(restated, a.launches))
        nbytes = N_SEQ * C * (H * W + h * w)
        k, t_ = med(us["kernel"]), med(us["torch"])
        one = host[0].numpy()
        want = R.resize_cubic_u8(one, (h, w))[0]
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            R.resize_cubic_u8(one, (h, w))
            ms.append((time.perf_counter() - t0) * 1e3)
        entry = {"out": [h, w], "bytes": nbytes, "kernel_us": k, "kernel_us_rounds": [round(v, 3) for v in us["kernel"]],
                 "kernel_GBs": round(nbytes / k / 1e3, 1), "kernel_fraction_of_peak": round(nbytes / (k * 1e-6) / (a.peak_tbs * 1e12), 4),
                 "kernel_us_per_frame": round(k / N_SEQ, 3), "torch_us": t_, "torch_us_rounds": [round(v, 3) for v in us["torch"]],
                 "torch_over_kernel": round(t_ / k, 2), "torch_share_of_samples_differing": round(differ, 6),
                 "oracle_host_ms_one_frame": med(ms), "kernel_frame0_equals_oracle": bool(np.array_equal(out[0].cpu().numpy(), want))}
        res["scales"]["x%d" % scale] = entry
        print(json.dumps({"x%d" % scale: entry}), flush=True)
        del out, got_t

    # FramePairs.from_wide from pinned host memory, x4, split into its two parts
    chunk, scale = 16, 4
    h, w = H // scale, W // scale
    pinned = host.pin_memory()
    lr = torch.empty((N_SEQ, C, h, w), device=dev, dtype=torch.uint8)

    def upload():
        for lo in range(0, N_SEQ, chunk):
            pinned[lo:lo + chunk].to(dev, non_blocking=True)

    def resize():
        for lo in range(0, N_SEQ, chunk):
            ops.resize_cubic_u8(x[lo:lo + chunk], (h, w), out=lr[lo:lo + chunk])

    def from_wide():
        return FramePairs.from_wide(pinned, None, scale, N_SEQ, device=dev, chunk=chunk)
    store = from_wide()
    equal = bool(torch.equal(store.lr, ops.resize_cubic_u8(x, (h, w))))
    parts = {"upload": upload, "resize": resize, "from_wide": from_wide}
    ms = {k_: [] for k_ in parts}
    for fn in parts.values():
        fn()
    for _ in range(a.rounds):
        for k_, fn in parts.items():
            ms[k_].append(wall_ms(fn))
    res["from_wide"] = {"timing": f"wall clock, device synchronise on both sides, ms per 50-frame scene; median of {a.rounds} rounds, the parts "
                                  "alternated inside a round", "scale": scale, "chunk": chunk, "source": "pinned host memory",
                        "wide_bytes": int(host.numel()), "equals_one_launch_over_the_scene": equal,
                        **{k_ + "_ms": med(v) for k_, v in ms.items()}, **{k_ + "_ms_rounds": [round(t, 3) for t in v] for k_, v in ms.items()}}
    res["from_wide"]["upload_GBs"] = round(host.numel() / res["from_wide"]["upload_ms"] / 1e6, 1)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
