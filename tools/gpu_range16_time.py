"""What the range census of the 16-bit backbone costs (addendum): `ops.range16_words` / `ops.range16_as_rounded` alone at
one 64 x 540 x 960 tensor against the bytes they read, the one-lane stamp launch, and the configs[4]-shaped forward (1 x 15 x 540 x
960, fp16 backbone) with `networks.backbone_check` unset, "report" and "bf16" (no overflow occurs with the synthetic weights, so
"bf16" never falls back: what is measured is the census and its read-backs).  Device events, the variants of one case alternated
round by round.

    python tools/gpu_range16_time.py --case kernels | forward15  [--out FILE] [--reps 5]

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

from gpu_census_time import rotate_us                         # noqa: E402
from gpu_longclip_time import DEV, net_x4, rotate             # noqa: E402
from eavsr_amd import networks as Nw, ops                     # noqa: E402
from eavsr_amd.utils.synthetic import synthetic_clip          # noqa: E402

CHECKS = (None, "report", "bf16")


def _stats(v, nbytes):
    med = statistics.median(v)
    return {"us": round(med, 2), "min_us": round(v[0], 2), "p10_us": round(v[len(v) // 10], 2), "p90_us": round(v[(9 * len(v)) // 10], 2),
            "spread_us": round(v[(9 * len(v)) // 10] - v[len(v) // 10], 2), "TBps": round(nbytes / med / 1e6, 3)}


def case_kernels(reps):
    """one 64 x 540 x 960 tensor: the words flavour reads 2 bytes per element, the as-rounded flavour 4; `pack16_census` (reads 4,
    writes 2) beside them as the yardstick; the stamp launch alone"""
    shape = (64, 540, 960)
    x32 = torch.randn(shape, device=DEV)
    n = x32.numel()
    out = {"shape": list(shape), "elements": n, "reps": reps, "timing": "device events around one call, us, variants alternated per round"}
    for name, dt in ops.CACHE16_DTYPES.items():
        x16, dst = x32.to(dt), torch.empty(shape, dtype=dt, device=DEV)
        record = torch.zeros(6, dtype=torch.int64, device=DEV)
        census = ops.RangeCensus(name, DEV)
        row = census._row("timing", "words", 0)
        got = rotate_us({"range16_words": lambda: ops.range16_words([x16], record[:5]),
                         "range16_as_rounded": lambda: ops.range16_as_rounded([x32], name, record[:5]),
                         "pack16_census": lambda: ops.pack16_census([x32], [dst], name, record[:5]),
                         "range16_stamp": lambda: census._count(lambda r: None, row)}, reps)
        nbytes = {"range16_words": 2.0 * n, "range16_as_rounded": 4.0 * n, "pack16_census": 6.0 * n, "range16_stamp": 48.0}
        out[name] = {k: dict(_stats(v, nbytes[k]), bytes=nbytes[k]) for k, v in got.items()}
    return out


def case_forward15(net, reps):
    n, t, h, w = 1, 15, 540, 960
    x = synthetic_clip(n, t, h, w, seed=4).to(DEV)
    out = {"shape": [n, t, 3, h, w], "backbone": "fp16", "reps": reps, "timing": "device events, median, variants alternated per round",
           "variants": {}}

    def run(check):
        net.backbone_census.clear()
        with Nw.backbone_check(check):
            return net(x)
    with torch.no_grad(), Nw.backbone_dtype("fp16"):
        res = rotate({str(c): lambda c=c: run(c) for c in CHECKS}, reps)
        with ops.profile() as prof:
            run(None)
        plain = prof.summary()
        with ops.profile() as prof:
            run("report")
        checked = prof.summary()
        entry = net.backbone_census[0]
    for c in CHECKS:
        row = res[str(c)]
        v = sorted(row["all_ms"])
        row["spread_ms"] = round(v[-1] - v[0], 3)
        row["vs_unset_time"] = round(row["ms"] / res["None"]["ms"], 4)
        row["vs_unset_peak"] = round(row["peak_bytes"] / res["None"]["peak_bytes"], 4)
        out["variants"][str(c)] = row
    census_names = ("range16_words", "range16_as_rounded", "range16_stamp")
    out["launches"] = {"unset": sum(v["calls"] for v in plain.values()), "report": sum(v["calls"] for v in checked.values()),
                       "census": {k: checked[k]["calls"] for k in census_names if k in checked},
                       "census_ms": {k: round(checked[k]["ms"], 3) for k in census_names if k in checked},
                       "others_equal_unset": {k: v["calls"] for k, v in checked.items() if k not in census_names} ==
                                             {k: v["calls"] for k, v in plain.items()}}
    sites = entry["sites"]
    worst = sorted(sites, key=lambda s: s["headroom"])[:8]
    out["census"] = {"summary": Nw.range_summary([entry]), "sites": len(sites), "elements": sum(s["elements"] for s in sites),
                     "least_headroom": [{k: s[k] for k in ("site", "max_abs", "headroom", "subnormal", "elements")} for s in worst]}
    out["note"] = "synthetic weights: the range says nothing about a trained model"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["kernels", "forward15"])
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    res = case_kernels(max(a.reps, 40)) if a.case == "kernels" else case_forward15(net_x4(), a.reps)
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
