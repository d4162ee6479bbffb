"""What the census of the 16-bit feature cache costs (addendum): `ops.pack16_census` against the unchanged `ops.pack16` at
the two sizes of r24_cache16_time.json's kernel case, and `forward_long` of its 50-frame scene with cache_check in (None, "report",
"bf16") on an fp16 cache (no overflow occurs with the synthetic weights, so "bf16" never falls back: what is measured is the census
and the one read-back before stage 3).  Device events, the variants of one case alternated round by round.

    python tools/gpu_census_time.py --case kernels | scene50  [--out FILE] [--reps 5]

Every case prints one JSON object and, with --out, merges it into that JSON file under the case's name.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_longclip_time import DEV, drop, net_x4, rotate      # noqa: E402
from eavsr_amd import framestore as FS, networks as Nw, ops  # noqa: E402
from eavsr_amd.utils.synthetic import synthetic_clip         # noqa: E402

CHECKS = (None, "report", "bf16")


def rotate_us(variants, reps, warmup=3):
    """every round runs each variant once, in turn -> {name: sorted list of us}"""
    times = {k: [] for k in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1) * 1e3)
    return {k: sorted(v) for k, v in times.items()}


def case_kernels(reps):
    """one 64 x 540 x 960 frame, and the 15-item step of r24_cache16_time.json: `pack16_census` into one zeroed record against
    `pack16`, alternated.  'spread_us' is pack16's own run-to-run spread (its 90th minus its 10th percentile): the yardstick for
    whether the census costs anything that can be told from noise."""
    full, d2, d4 = (64, 540, 960), (64, 270, 480), (64, 135, 240)
    out = {"bytes_per_element": 6, "reps": reps, "timing": "device events around one call, us, variants alternated per round"}
    for label, shapes in (("frame_64x540x960", [full]), ("step_15_items", [full, d2, d4] * 4 + [full] * 3)):
        x32 = [torch.randn(s, device=DEV) for s in shapes]
        nbytes = 6.0 * sum(t.numel() for t in x32)
        row = {"items": len(shapes), "bytes": nbytes}
        for name, dt in FS.CACHE_DTYPES.items():
            x16 = [torch.empty(s, dtype=dt, device=DEV) for s in shapes]
            record = torch.zeros(5, dtype=torch.int64, device=DEV)
            got = rotate_us({"pack16": lambda: ops.pack16(x32, x16, dt), "pack16_census": lambda: ops.pack16_census(x32, x16, dt, record)}, reps)
            for key, v in got.items():
                row[f"{name}_{key}"] = {"us": round(statistics.median(v), 2), "min_us": round(v[0], 2),
                                        "p10_us": round(v[len(v) // 10], 2), "p90_us": round(v[(9 * len(v)) // 10], 2),
                                        "TBps": round(nbytes / statistics.median(v) / 1e6, 3)}
            base = row[f"{name}_pack16"]
            row[f"{name}_census_vs_pack16"] = round(row[f"{name}_pack16_census"]["us"] / base["us"], 4)
            row[f"{name}_census_minus_pack16_us"] = round(row[f"{name}_pack16_census"]["us"] - base["us"], 2)
            row[f"{name}_pack16_spread_us"] = round(base["p90_us"] - base["p10_us"], 2)
        out[label] = row
    return out


def case_scene50(net, reps, backbone="fp16"):
    n, t, h, w = 1, 50, 540, 960
    clip = torch.cat([synthetic_clip(n, min(10, t - a), h, w, seed=40 + a // 10) for a in range(0, t, 10)], 1)
    u8 = (clip * 255).round().to(torch.uint8).pin_memory()
    del clip
    out = {"shape": [n, t, 3, h, w], "backbone": backbone, "frame_chunk": 3, "cache": "device", "cache_dtype": "fp16",
           "input": "uint8, pinned host memory", "reps": reps, "timing": "device events, median, variants alternated per round", "variants": {}}

    def run(check):
        net.cache_census.clear()
        if check is None:
            return net.forward_long(u8, frame_chunk=3, sink=drop, cache_dtype="fp16")
        return net.forward_long(u8, frame_chunk=3, sink=drop, cache_dtype="fp16", cache_check=check)
    with torch.no_grad(), Nw.backbone_dtype(backbone):
        res = rotate({str(c): lambda c=c: run(c) for c in CHECKS}, reps)
        run("report")
        entry = net.cache_census[0]
    for c in CHECKS:
        row = res[str(c)]
        row["vs_no_check_time"] = round(row["ms"] / res["None"]["ms"], 4)
        row["vs_no_check_peak"] = round(row["peak_bytes"] / res["None"]["peak_bytes"], 4)
        out["variants"][str(c)] = row
    base = sorted(res["None"]["all_ms"])
    out["no_check_spread_ms"] = round(base[-1] - base[0], 3)
    out["census"] = {"fallback": entry["fallback"], "summary": FS.census_summary([entry]),
                     "max_abs_per_key": {k: r["max_abs"] for k, r in entry["keys"].items()}}
    out["note"] = "synthetic weights: the feature range says nothing about a trained model"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["kernels", "scene50"])
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = case_kernels(max(a.reps, 40)) if a.case == "kernels" else case_scene50(net_x4(), a.reps)
    print(json.dumps(res))
    if a.out:
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged[a.case] = res
        with open(a.out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
