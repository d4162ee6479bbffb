"""Time the antialiased bicubic resize of SR frames on the GPU -> profiles/r28_resize_time.json.

  kernels   `resize.resize_frames` at 7 x 3 x 720 x 1280 -> 1080 x 1920 (up, 4 taps) and 7 x 3 x 2160 x 3840 -> 1080 x 1920 (down, 10
            taps), beside torch's `F.interpolate(mode="bicubic", antialias=True)` at the same shapes.  torch's kernel constant is
            a = -0.75: a TIME to stand beside, never values to compare with.  Device events around one call after warm-up, the
            variants alternated, `--reps` calls per round, `--rounds` rounds; the fraction of the HBM peak is quoted on the
            algorithmic bytes of this op -- the source read once, the intermediate (N C, oh, W) written and read, the result written.
  scene     `harness.super_resolve` of the 15 x 540 x 960 scene of profiles/r20_tile_time.json (synthetic weights, uint8 frames on the
            device, no files, no HR frames) with and without out_size=(1620, 2880), alternated in the same run; the overhead in per
            cent beside the spread of the plain runs.  --no-scene: the kernels only.

    python tools/gpu_resize_time.py --out profiles/r28_resize_time.json
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


def one_call_us(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def measure(variants, reps, rounds):
    """{name: {'us': median of all calls, 'min_us', 'round_medians': {median, min, max}}}"""
    for fn in variants.values():
        for _ in range(3):
            fn()      # warm-up: code objects, the tables, the allocator's blocks
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the fractions are quoted against, TB/s")
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--scene-runs", type=int, default=3)
    ap.add_argument("--no-scene", action="store_true", help="the kernels only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_resize_time: needs a GPU (a measurement does not fall back)")
    import torch.nn.functional as F
    from eavsr_amd import harness, resize
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs,
           "timing": f"kernels: device events around one call, us; {a.reps} calls per variant and round, variants alternated, {a.rounds} "
                     "rounds; 'us' is the median of all calls, 'round_medians' the spread of the rounds' medians.  scene: "
                     f"{a.scene_runs} runs per variant after one warm-up run each, alternated, host clock between device synchronisations",
           "caveats": "values not compared with MATLAB or any package; the fp32 path on [0, 1] is not MATLAB's uint8 path; torch's "
                      "antialiased bicubic uses a = -0.75: a time only; the scene runs on synthetic weights",
           "cases": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")

    g = torch.Generator(device=dev).manual_seed(1)
    for name, (n, c, H, W), (oh, ow) in (("up_7x3x720x1280_to_1080x1920", (7, 3, 720, 1280), (1080, 1920)),
                                         ("down_7x3x2160x3840_to_1080x1920", (7, 3, 2160, 3840), (1080, 1920))):
        x = torch.rand((n, c, H, W), device=dev, generator=g)
        out = torch.empty((n, c, oh, ow), device=dev)
        got = measure({"resize_frames": lambda: resize.resize_frames(x, (oh, ow), out=out),
                       "torch_interpolate_bicubic_antialias": lambda: F.interpolate(x, size=(oh, ow), mode="bicubic", antialias=True)},
                      a.reps, a.rounds)
        nbytes = 4 * n * c * (H * W + 2 * oh * W + oh * ow)
        taps = (int(resize.axis_tables(H, oh)[0].shape[1]), int(resize.axis_tables(W, ow)[0].shape[1]))
        for k, v in got.items():
            v["algorithmic_bytes"] = nbytes
            v["fraction_of_peak"] = round(nbytes / (v["us"] * 1e-6) / (a.peak_tbs * 1e12), 3)
        got["taps_rows_columns"] = taps
        got["resize_frames_over_torch"] = round(got["resize_frames"]["us"] / got["torch_interpolate_bicubic_antialias"]["us"], 3)
        res["cases"][name] = got
        print(name, json.dumps(got), flush=True)
        del x, out
        torch.cuda.empty_cache()
        dump()

    if not a.no_scene:
        from eavsr_amd.eavsrp_model import EAVSRP
        from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        sd0 = net.state_dict()
        net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
        net = net.to(dev).eval()
        clip = (synthetic_clip(1, a.frames, 540, 960, seed=3)[0] * 255).round().to(torch.uint8).to(dev)      # (f, 3, h, w)
        variants = {"plain": {}, "out_size_1620x2880": {"out_size": (1620, 2880)}}
        for kw in variants.values():
            harness.super_resolve(net, clip, frame_chunk=3, **kw)      # warm-up
        secs = {k: [] for k in variants}
        for i in range(a.scene_runs):
            for k in (list(variants) if i % 2 == 0 else list(variants)[::-1]):
                torch.cuda.empty_cache()
                secs[k].append(harness.super_resolve(net, clip, frame_chunk=3, **variants[k])["seconds"])
        kept = {k: {"seconds": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in secs.items()}
        plain = kept["plain"]
        kept["overhead_percent"] = round(100.0 * (kept["out_size_1620x2880"]["seconds"] / plain["seconds"] - 1.0), 2)
        kept["plain_spread_percent"] = round(100.0 * (plain["max"] - plain["min"]) / plain["seconds"], 2)
        res["cases"][f"scene_{a.frames}x540x960"] = kept
        print("scene", json.dumps(kept), flush=True)
    dump()


if __name__ == "__main__":
    main()
