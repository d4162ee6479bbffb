"""Measurements of the 16-bit feature cache: the two kernels against torch's `.to()`, `forward_long` of the 50-frame scene
of r12_longclip_time.json with cache_dtype in (None, fp16, bf16), the host cache at 15 frames each way, and the PSNR of each 16-bit
run against the fp32 cache's output (synthetic weights: it says nothing about a trained model).  Device events, median of --reps,
the variants of one case alternated round by round.

    python tools/gpu_cache16_time.py --case kernels | scene50 | host15 | parity  [--out FILE] [--reps 5]

Every case prints one JSON object and, with --out, merges it into that JSON file under the case's name.
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_longclip_time import DEV, drop, net_x4, rotate      # noqa: E402
from eavsr_amd import framestore as FS, networks as Nw, ops  # noqa: E402
from eavsr_amd.utils.synthetic import synthetic_clip         # noqa: E402

HBM_PEAK = 8.0e12
DTYPES = (None, "fp16", "bf16")


def timed(fn, reps, warmup=3):
    out = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out), min(out)


def case_kernels(reps):
    """one 64 x 540 x 960 frame, and a 15-item step (the window's bound with no earlier branch: 12 pyramid tensors of the three sizes
    plus three more full-size frames), hipcc's kernels in one launch against torch's `.to()` per tensor.  6 bytes move per element."""
    full, d2, d4 = (64, 540, 960), (64, 270, 480), (64, 135, 240)
    out = {"hbm_peak_TBps": HBM_PEAK / 1e12, "bytes_per_element": 6, "timing": "device events around one call, median / min, us"}
    for label, shapes in (("frame_64x540x960", [full]), ("step_15_items", [full, d2, d4] * 4 + [full] * 3)):
        x32 = [torch.randn(s, device=DEV) for s in shapes]
        nbytes = 6.0 * sum(t.numel() for t in x32)
        row = {"items": len(shapes), "bytes": nbytes}
        for name, dt in FS.CACHE_DTYPES.items():
            x16 = [torch.empty(s, dtype=dt, device=DEV) for s in shapes]
            back = [torch.empty(s, device=DEV) for s in shapes]
            variants = {"pack16": lambda: ops.pack16(x32, x16, dt), "torch_to_16": lambda: [a.copy_(b) for a, b in zip(x16, x32)],
                        "unpack16": lambda: ops.unpack16(x16, back), "torch_to_32": lambda: [a.copy_(b) for a, b in zip(back, x16)]}
            for key, fn in variants.items():
                med, lo = timed(fn, reps)
                row[f"{name}_{key}"] = {"us": round(med, 2), "min_us": round(lo, 2), "TBps": round(nbytes / med / 1e6, 3),
                                        "frac_of_8TBps": round(nbytes / med / 1e6 / 8.0, 4)}
            for ours, theirs in (("pack16", "torch_to_16"), ("unpack16", "torch_to_32")):
                row[f"{name}_{ours}_vs_torch"] = round(row[f"{name}_{ours}"]["us"] / row[f"{name}_{theirs}"]["us"], 3)
        out[label] = row
    return out


def _capture_stores():
    """`framestore.make_store` wrapped so that every store reports its `nbytes()["total"]` when the run finishes with it (the store
    itself is not kept: it would stay resident into the next variant's peak)"""
    totals, real = {}, FS.make_store

    def make(*a, **k):
        store = real(*a, **k)
        finish = store.finish

        def finish_and_report():
            totals[str(getattr(store, "cache_dtype", None))] = store.nbytes()["total"]
            del store.finish      # (store -> this closure -> store: without this the store outlives the call until a collection)
            finish()
        store.finish = finish_and_report
        return store
    FS.make_store = make
    return totals, real


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * math.log10(1.0 / mse) if mse > 0 else float("inf")


def case_long(net, t, cache, reps, backbone="fp16"):
    n, h, w = 1, 540, 960
    clip = torch.cat([synthetic_clip(n, min(10, t - a), h, w, seed=40 + a // 10) for a in range(0, t, 10)], 1)
    u8 = (clip * 255).round().to(torch.uint8).pin_memory()
    del clip
    seen, real = _capture_stores()
    out = {"shape": [n, t, 3, h, w], "backbone": backbone, "frame_chunk": 3, "cache": cache, "input": "uint8, pinned host memory",
           "reps": reps, "timing": "device events, median, variants alternated per round", "variants": {}}
    try:
        with torch.no_grad(), Nw.backbone_dtype(backbone):
            res = rotate({str(d): lambda d=d: net.forward_long(u8, frame_chunk=3, cache=cache, sink=drop, cache_dtype=d) for d in DTYPES}, reps)
            totals = dict(seen)
            # PSNR of frames 0 .. 5 of a 6-frame run (the SR clip of the whole scene is never held): synthetic weights
            part = u8[:, :6]
            outs = {str(d): net.forward_long(part, frame_chunk=3, cache=cache, cache_dtype=d) for d in DTYPES}
    finally:
        FS.make_store = real
    for d in DTYPES:
        row = res[str(d)]
        row["store_nbytes_total"] = totals[str(d)]
        row["vs_fp32_cache_time"] = round(row["ms"] / res["None"]["ms"], 4)
        row["vs_fp32_cache_peak"] = round(row["peak_bytes"] / res["None"]["peak_bytes"], 4)
        if d is not None:
            row["psnr_db_vs_fp32_cache_first_6_frames"] = round(_psnr(outs[str(d)], outs["None"]), 2)
        out["variants"][str(d)] = row
    out["note"] = "synthetic weights: the PSNR says nothing about a trained model"
    return out


def case_parity(net):
    """the figures tests/test_hip_cache16.py::test_the_16_bit_cache_stays_close_to_the_fp32_cache asserts against: 1 x 5 x 64 x 64,
    seed 41, frame_chunk=2, fp32 backbone, PSNR with peak 1 against the cache_dtype=None output"""
    big = synthetic_clip(1, 5, 68, 68, seed=41)
    x = (big[..., :64, :64] * 255).round().to(torch.uint8).contiguous().to(DEV)
    with torch.no_grad():
        plain = net.forward_long(x, frame_chunk=2)
        got = {d: _psnr(net.forward_long(x, frame_chunk=2, cache_dtype=d), plain) for d in ("fp16", "bf16")}
        host = {d: bool(torch.equal(net.forward_long(x, frame_chunk=2, cache_dtype=d, cache="host"),
                                    net.forward_long(x, frame_chunk=2, cache_dtype=d))) for d in ("fp16", "bf16")}
    return {"shape": [1, 5, 3, 64, 64], "seed": 41, "frame_chunk": 2, "backbone": "fp32", "weights": "synthetic (trained_like, seed 0)",
            "psnr_db_vs_fp32_cache": {k: round(v, 2) for k, v in got.items()}, "host_cache_bit_identical_to_device_cache": host,
            "note": "synthetic weights: this says nothing about a trained model"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["kernels", "scene50", "host15", "parity"])
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.case == "kernels":
        res = case_kernels(max(a.reps, 20))
    elif a.case == "scene50":
        res = case_long(net_x4(), 50, "device", a.reps)
    elif a.case == "host15":
        res = case_long(net_x4(), 15, "host", a.reps)
    else:
        res = case_parity(net_x4())
    print(json.dumps(res))
    if a.out:
        merged = {}
        if a.case != "parity" and os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged = res if a.case == "parity" else dict(merged, **{a.case: res})
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
