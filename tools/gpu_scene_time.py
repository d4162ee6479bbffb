"""What videos of any length cost: the scene-cut statistics kernel, the segmented `super_resolve` against the whole
scene, and the seam between two windows.  One part per process (--part), nothing is retried; no number here is a pass/fail bound.

  kernel    `ops.frame_change` at --frames x 3 x 540 x 960, planar and interleaved: device events around --launches back-to-back
            calls (the wrapper's two zero-fills included), median of --rounds rounds, the layouts and a torch restatement on the
            device alternated inside a round.  Algorithmic bytes: every byte of the clip ONCE (a run of frames re-reads the frame
            before it: the kernel's own traffic is (1 + (runs - 1) / F) times that, recorded beside it); fraction of --peak-tbs.
  scene     `harness.super_resolve` of a 60-frame 180 x 320 scene, whole against max_frames=20, overlap=4: seconds, peak_bytes, the
            measured time ratio beside 20 / 16, the plan.  Runs alternated, median of --scene-rounds.
  seam      a 40-frame 64 x 96 clip, max_frames=16, overlap in {0, 2, 4, 8}: per emitted frame the max-abs and the 8-bit PSNR of the
            segmented output against the whole-clip output, grouped by the frame's distance from the nearest artificial window
            end.  SYNTHETIC weights: the size of the seam says nothing about a trained model.

Every part is a GPU step of its own under its own time limit; a part merges its section into the file the parts before it wrote:

    timeout -k 10 120 python tools/gpu_scene_time.py --part kernel --out profiles/r18_scene_time.json &&
    timeout -k 10 300 python tools/gpu_scene_time.py --part scene --out profiles/r18_scene_time.json &&
    timeout -k 10 300 python tools/gpu_scene_time.py --part seam --out profiles/r18_scene_time.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def torch_frame_change(x):
    """the definition restated with torch on the device (planar (F, 3, h, w)): what a user without the kernel would write"""
    r, g, b = (x[:, c].to(torch.int32) for c in range(3))
    y = (77 * r + 150 * g + 29 * b + 128) >> 8
    f = y.shape[0]
    idx = (y >> 2).reshape(f, -1).to(torch.int64) + 64 * torch.arange(f, device=x.device).view(f, 1)
    hist = torch.bincount(idx.reshape(-1), minlength=64 * f).view(f, 64).to(torch.int32)
    sad = (y[1:] - y[:-1]).abs().reshape(f - 1, -1).sum(1, dtype=torch.int64)
    return hist, sad


def drifting_clip(t, h, w, seed):
    """(1, t, 3, h, w) fp32 in [0, 1): `synthetic_clip`'s recipe (a low-pass random texture under a sub-pixel-free drift plus a little
    noise) with a drift that turns round every 20 frames, so that a clip may have any length"""
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    base = torch.rand(1, 3, h // 4 + 8, w // 4 + 8, generator=g)
    base = torch.nn.functional.interpolate(base, scale_factor=4, mode="bicubic", align_corners=False)
    frames = []
    for i in range(t):
        k = i % 40
        dy, dx = 6 + int(round(2.0 * math.sin(0.9 * i))), 6 + (k if k <= 20 else 40 - k)
        frames.append(base[:, :, dy:dy + h, dx:dx + w] + 0.03 * torch.rand(1, 3, h, w, generator=g))
    return torch.stack(frames, 1).clamp(0.0, 0.999).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--scene-rounds", type=int, default=3)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fraction is quoted against, TB/s")
    ap.add_argument("--part", choices=("kernel", "scene", "seam"), required=True, help="the one measurement this process makes")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_scene_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.segments import plan_segments
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of
    dev = torch.device("cuda:0")
    res = {}
    if a.out and os.path.exists(a.out):      # the sections the earlier parts wrote
        with open(a.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs})

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    # kernel
    if a.part == "kernel":
        F, h, w = a.frames, 540, 960
        g = torch.Generator(device=dev).manual_seed(1)
        planar = torch.randint(0, 256, (F, 3, h, w), dtype=torch.uint8, device=dev, generator=g)
        inter = planar.permute(0, 2, 3, 1).contiguous()
        want = torch_frame_change(planar)
        for name, src in (("planar", planar), ("interleaved", inter)):
            got = ops.frame_change(src)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
        variants = {"planar": lambda: ops.frame_change(planar), "interleaved": lambda: ops.frame_change(inter),
                    "torch": lambda: torch_frame_change(planar)}
        us = {k: [] for k in variants}
        for fn in variants.values():
            fn()      # warm-up
        for rnd in range(a.rounds):
            order = list(variants) if rnd % 2 == 0 else list(variants)[::-1]
            for k in order:
                us[k].append(event_us(variants[k], a.launches))
        nbytes = planar.numel()
        blocks = (h * w + 4095) // 4096
        runs = max(1, min((2048 + blocks - 1) // blocks, (F + 7) // 8))
        run = (F + runs - 1) // runs
        runs = (F + run - 1) // run
        res["kernel"] = {
            "shape": [F, 3, h, w], "algorithmic_bytes": nbytes,
            "bytes_note": "every byte of the clip counted once; the kernel cuts the frames into runs and a run re-reads the frame before it",
            "runs": runs, "bytes_read_by_the_kernel": int(nbytes * (1 + (runs - 1) / F)),
            "timing": f"device events around {a.launches} back-to-back calls (zero-fills of hist / sad included), us per call; median / min / "
                      f"max of {a.rounds} rounds, variants alternated",
            "us": {k: spread(v) for k, v in us.items()},
            "tbs": {k: round(nbytes / statistics.median(us[k]) / 1e6, 3) for k in ("planar", "interleaved")},
            "fraction_of_peak": {k: round(nbytes / statistics.median(us[k]) / 1e6 / a.peak_tbs, 3) for k in ("planar", "interleaved")},
            "torch_over_kernel": round(statistics.median(us["torch"]) / statistics.median(us["planar"]), 2),
        }
        print(json.dumps(res["kernel"]), flush=True)
        dump()
        return

    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
    fixed = {k: v for k, v in net.state_dict().items() if k.endswith(("regular_matrix", "mean", "std"))}
    net.load_state_dict(fill_state_dict(shapes_of(net.state_dict()), "trained_like", 0, fixed=fixed), strict=True)
    net = net.to(dev).eval()
    res["weights"] = "synthetic (fill_state_dict 'trained_like'): timings and memory are representative, image quality is not"

    # scene
    if a.part == "scene":
        lr = (drifting_clip(60, 180, 320, seed=2) * 255).round().to(torch.uint8).to(dev)
        kinds = {"whole": {}, "segmented": {"max_frames": 20, "overlap": 4}}
        harness.super_resolve(net, lr[:, :20])      # warm-up
        runs_ = {k: [] for k in kinds}
        for rnd in range(a.scene_rounds):
            for k in (list(kinds) if rnd % 2 == 0 else list(kinds)[::-1]):
                runs_[k].append(harness.super_resolve(net, lr, **kinds[k]))
        sec = {k: statistics.median(r["seconds"] for r in v) for k, v in runs_.items()}
        res["scene"] = {
            "shape": [1, 60, 3, 180, 320], "plan": runs_["segmented"][0]["segments"],
            "seconds": {k: spread([r["seconds"] for r in v]) for k, v in runs_.items()},
            "peak_bytes": {k: max(r["peak_bytes"] for r in v) for k, v in runs_.items()},
            "time_ratio": round(sec["segmented"] / sec["whole"], 4), "ratio_of_the_strides": 20 / 16,
            "frames_through_stages_1_2": sum(b - s for s, b, _, _ in runs_["segmented"][0]["segments"]),
            "timing": f"wall clock of super_resolve (device-synchronised on both sides), median / min / max of {a.scene_rounds}, alternated",
        }
        print(json.dumps(res["scene"]), flush=True)
        dump()
        del lr

    # seam
    if a.part == "seam":
        t, mf = 40, 16
        clip = drifting_clip(t, 64, 96, seed=3).to(dev)
        with torch.no_grad():
            whole = net.forward_long(clip)
            q_whole = ops.rgb8(whole[0], 255.0).to(torch.float64)
            seam = {}
            for ov in (0, 2, 4, 8):
                plan = plan_segments(t, [], mf, ov)
                seg = net.forward_segments(clip, plan)
                q = ops.rgb8(seg[0], 255.0).to(torch.float64)
                by_dist = {}
                for s, e, ea, eb in plan:
                    for f in range(ea, eb):
                        ends = ([f - s] if s != 0 else []) + ([e - 1 - f] if e != t else [])      # frames between f and an artificial end
                        d = min(ends)
                        mse = float(((q[f] - q_whole[f]) ** 2).mean())
                        by_dist.setdefault(d, []).append((float((seg[0, f] - whole[0, f]).abs().max()),
                                                          99.0 if mse == 0 else 10 * math.log10(255.0 ** 2 / mse)))
                seam[str(ov)] = {"plan": plan, "by_distance_from_an_artificial_window_end": {
                    str(d): {"frames": len(v), "max_abs": max(x for x, _ in v), "psnr8_min_db": round(min(p for _, p in v), 2)}
                    for d, v in sorted(by_dist.items())}}
        res["seam"] = {"shape": [1, t, 3, 64, 96], "max_frames": mf, "overlap": seam,
                       "note": "synthetic weights: NOT representative of a trained model; psnr 99 = identical 8-bit frames"}
        print(json.dumps(res["seam"]), flush=True)
        dump()


if __name__ == "__main__":
    main()
