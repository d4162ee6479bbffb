"""What the padded ingest costs: `ops.ingest_pad` beside `ops.u8_to_f32` (unchanged by the padding work: the same
kernel as before it) and a torch restatement on the device.  No number here is a pass/fail bound; nothing is retried.

  padded      15 x 3 x 270 x 480 -> 272 x 480 (1080p / 4), uint8 planes, interleaved, fp32 planes: `ingest_pad` (reflect) against
              `u8_to_f32` on the same unpadded frames followed by `F.pad(mode="reflect")` -- what a user without the kernel
              would write on the device -- and, for scale, `u8_to_f32` alone (which does not pad).
  unpadded    15 x 3 x 540 x 960 with H = h, W = w in the three layouts: `ingest_pad` against `u8_to_f32` (bytes) or a `clone`
              (fp32) on the same frames.  The reference point is `u8_to_f32` at this shape: profiles/r12_longclip_time.json
              has it at 0.50 of the HBM peak.

Timing as tools/gpu_longclip_time.py times the ingest (so that the figures compare): device events around ONE call (the output's
allocation from torch's caching allocator included), --reps calls per variant and round, the variants alternated inside a round,
--rounds rounds; per variant the median over all calls and the spread of the rounds' medians (the run-to-run spread inside this
process).  Bytes: every source byte read once and every fp32 output sample written once; fraction of --peak-tbs.  Every result is
compared with the restatement bit for bit before anything is timed.

    timeout -k 10 300 python tools/gpu_pad_time.py --out profiles/r19_pad_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def one_call_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def measure(variants, reps, rounds):
    """{name: {'us': median of all calls, 'round_medians': {median, min, max}}}"""
    for fn in variants.values():
        for _ in range(3):
            fn()      # warm-up: code objects, the allocator's blocks
    torch.cuda.synchronize()
    per_round = {k: [] for k in variants}
    every = {k: [] for k in variants}
    for rnd in range(rounds):
        order = list(variants) if rnd % 2 == 0 else list(variants)[::-1]
        ts = {k: [] for k in variants}
        for _ in range(reps):
            for k in order:
                ts[k].append(one_call_us(variants[k]))
        for k in variants:
            per_round[k].append(statistics.median(ts[k]))
            every[k] += ts[k]
    return {k: {"us": round(statistics.median(every[k]), 2), "min_us": round(min(every[k]), 2),
                "round_medians": {"median": round(statistics.median(per_round[k]), 2), "min": round(min(per_round[k]), 2),
                                  "max": round(max(per_round[k]), 2)}} for k in variants}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the fractions are quoted against, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_pad_time: needs a GPU (a measurement does not fall back)")
    import torch.nn.functional as F
    from eavsr_amd import ops
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs,
           "timing": f"device events around one call, us; {a.reps} calls per variant and round, variants alternated, {a.rounds} rounds; 'us' is "
                     "the median of all calls, 'round_medians' the spread of the rounds' medians",
           "bytes": "source bytes read once + 4 bytes per output sample written once", "cases": {}}
    g = torch.Generator(device=dev).manual_seed(1)

    def sources(f, h, w):
        planes = torch.randint(0, 256, (f, 3, h, w), dtype=torch.uint8, device=dev, generator=g)
        return {"u8_planes": planes, "u8_interleaved": planes.permute(0, 2, 3, 1).contiguous(), "f32_planes": ops.u8_to_f32(planes)}

    def record(case, layout, src, H, W, variants):
        f, c = int(src.shape[0]), 3
        nbytes = src.numel() * src.element_size() + 4 * f * c * H * W
        m = measure(variants, a.reps, a.rounds)
        for k, v in m.items():
            counted = src.numel() * 5 if k == "u8_to_f32" else nbytes      # u8_to_f32 alone writes the unpadded frames
            v["bytes"] = counted
            v["tbs"] = round(counted / v["us"] / 1e6, 3)
            v["fraction_of_peak"] = round(counted / v["us"] / 1e6 / a.peak_tbs, 3)
        entry = {"source": list(src.shape), "dtype": str(src.dtype).replace("torch.", ""), "out": [f, c, H, W], **m}
        base = "u8_to_f32" if "u8_to_f32" in m else "torch"
        entry["ingest_pad_over_" + base] = round(m["ingest_pad"]["us"] / m[base]["us"], 3)
        res["cases"].setdefault(case, {})[layout] = entry
        print(case, layout, json.dumps(entry), flush=True)

    # padded: 270 x 480 -> 272 x 480
    f, h, w, H, W = 15, 270, 480, 272, 480
    for layout, src in sources(f, h, w).items():
        hwc = layout == "u8_interleaved"
        if src.dtype == torch.uint8:
            restated = lambda src=src, hwc=hwc: F.pad(ops.u8_to_f32(src, hwc=hwc), (0, W - w, 0, H - h), mode="reflect")
            variants = {"ingest_pad": lambda src=src, hwc=hwc: ops.ingest_pad(src, H, W, hwc=hwc), "torch": restated,
                        "u8_to_f32": lambda src=src, hwc=hwc: ops.u8_to_f32(src, hwc=hwc)}
        else:
            restated = lambda src=src: F.pad(src, (0, W - w, 0, H - h), mode="reflect")
            variants = {"ingest_pad": lambda src=src: ops.ingest_pad(src, H, W), "torch": restated}
        assert torch.equal(variants["ingest_pad"]().view(torch.int32), restated().view(torch.int32)), layout
        record("padded_270x480_to_272x480", layout, src, H, W, variants)
    # unpadded: 540 x 960
    f, h, w = 15, 540, 960
    for layout, src in sources(f, h, w).items():
        hwc = layout == "u8_interleaved"
        if src.dtype == torch.uint8:
            variants = {"ingest_pad": lambda src=src, hwc=hwc: ops.ingest_pad(src, h, w, hwc=hwc),
                        "u8_to_f32": lambda src=src, hwc=hwc: ops.u8_to_f32(src, hwc=hwc)}
            restated = variants["u8_to_f32"]
        else:
            variants = {"ingest_pad": lambda src=src: ops.ingest_pad(src, h, w), "torch": lambda src=src: src.clone()}
            restated = variants["torch"]
        assert torch.equal(variants["ingest_pad"]().view(torch.int32), restated().view(torch.int32)), layout
        record("unpadded_540x960", layout, src, h, w, variants)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
