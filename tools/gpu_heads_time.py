"""The predictor's 5x5 heads (eavsr_conv_f32x6, 64 -> 120, mask sigmoid in the epilogue) alone at 180 x 320, by images per launch:
per-image time at 2, 10, 12 and 22 images.  HIP events around each launch, enqueued behind a device-side delay so that the launches run
back to back (as bench.py's profile pass); the image counts are visited in rotation, `--rounds` times, `--reps` launches each.
    python tools/gpu_heads_time.py [--out profiles/rNN_heads_time.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eavsr_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, D, h, w = torch.device("cuda:0"), 8, 180, 320
    g = torch.Generator().manual_seed(0)
    ws = [torch.randn(c, 64, 5, 5, generator=g).mul_(0.02).to(dev) for c in (4 * D, 2 * D, 9 * D)]
    bs = [torch.randn(c, generator=g).mul_(0.1).to(dev) for c in (4 * D, 2 * D, 9 * D)]
    counts = (2, 10, 12, 22)
    xs = {n: torch.randn(n, 64, h, w, generator=g).to(dev) for n in counts}
    res = {str(n): {"images": n, "tiles_per_workgroup": int(ops.lib().eavsr_conv_f32x6_tiles_per_workgroup(n, 64, 15 * D, h, w, 5)),
                    "launch_ms": []} for n in counts}
    with torch.no_grad():
        for n in counts:
            for _ in range(3):
                ops.conv2d(xs[n], ws, bs, sigmoid_from=6 * D)
        for _ in range(args.rounds):
            for n in counts:
                torch.cuda.synchronize()
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
                torch.cuda._sleep(int(0.05 * 2.0e9))
                keep = []
                for e0, e1 in evs:
                    e0.record()
                    keep.append(ops.conv2d(xs[n], ws, bs, sigmoid_from=6 * D))
                    e1.record()
                torch.cuda.synchronize()
                res[str(n)]["launch_ms"] += [e0.elapsed_time(e1) for e0, e1 in evs]
                del keep
    for r in res.values():
        ms = sorted(r.pop("launch_ms"))
        q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
        r.update(launches=len(ms), launch_ms_median=q(0.5), launch_ms_p10=q(0.1), launch_ms_p90=q(0.9), launch_ms_min=ms[0],
                 per_image_us_median=1e3 * q(0.5) / r["images"], per_image_us_p10=1e3 * q(0.1) / r["images"],
                 per_image_us_p90=1e3 * q(0.9) / r["images"])
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"what": __doc__.split("\n    python")[0], "shape": "n x 64 x 180 x 320 -> n x 120 x 180 x 320", "by_images": res},
                  open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
