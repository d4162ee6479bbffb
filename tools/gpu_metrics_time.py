"""Scoring one test item against producing it: 1 x 7 x 3 x 720 x 1280 (BASELINE configs[1]'s frame size) on one GPU.

  (a) forward        the x4 model on the item's 1 x 7 x 3 x 180 x 320 clip
  (b) parent         what `harness.evaluate(..., calc_ssim_flag=True)` runs per item without `per_frame`: get_current_visuals'
                     clamp * 255 round of both sequences + calc_psnr + calc_ssim (float64 conv2d), on the same device tensors; if the
                     device refuses float64 conv2d the exception text is recorded and the same calls are timed on CPU tensors
  (c) frame_metrics  `harness.frame_metrics` (the fused kernel + the per-frame host arithmetic)
  (d) (c) with the 8-bit frames (`ops.frame_metrics(..., rgb8=True)` + the same host arithmetic)
  kernel             device-event time of the `eavsr_frame_metrics_f32` call alone (both launches), algorithmic bytes, bytes with the
                     tiles' apron re-reads, fraction of --peak-tbs

Wall times: after --warmup calls, the median of --reps calls, each with a device synchronise on both sides.

    python tools/gpu_metrics_time.py [--reps 20] [--warmup 3] [--parts forward,parent,metrics,kernel] [--out FILE]

`rocprofv3 --kernel-trace --stats -- python tools/gpu_metrics_time.py --parts metrics --reps 5` names the kernels (no --pmc in
the same run).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, C, H, W, SCALE = 7, 3, 720, 1280, 4


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


def staged_samples(h, w):
    """samples one plane's tiles stage: 64 x 32 valid outputs + the 10-sample apron per tile, clipped to the plane"""
    total = 0
    for y0 in range(0, h - 10, 32):
        for x0 in range(0, w - 10, 64):
            total += min(74, w - x0) * min(42, h - y0)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="forward,parent,metrics,kernel")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fraction is quoted against, TB/s")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    parts = a.parts.split(",")
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "item": [1, T, C, H, W], "reps": a.reps, "warmup": a.warmup,
           "timing": "wall clock, device synchronise on both sides, median of reps"}

    hr = synthetic_clip(1, T, H, W, seed=2).to(dev)
    if "forward" in parts:
        net = EAVSRP(Namespace(predict=False, n_frame=T, n_flow=5, scale=SCALE), None)
        sd0 = net.state_dict()
        net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
        net = net.to(dev).eval()
        lr = synthetic_clip(1, T, H // SCALE, W // SCALE, seed=1).to(dev)
        with torch.no_grad():
            res["a_forward"] = wall(lambda: net(lr), a.reps, a.warmup)
            sr = net(lr).detach()
        del net
    else:
        sr = (hr + torch.randn_like(hr) * (4.0 / 255.0)).contiguous()
    print(json.dumps({k: v for k, v in res.items() if k.startswith("a_")}), flush=True)

    visuals = lambda v: torch.clamp(v.detach() * 255.0, 0, 255).round()      # EAVSRPModel.get_current_visuals

    def parent(s, h):
        qs, qh = visuals(s), visuals(h)
        return harness.calc_psnr(qs, qh), harness.calc_ssim(qs, qh)

    if "parent" in parts:
        try:
            ref = parent(sr, hr)
            res["b_parent"] = dict(wall(lambda: parent(sr, hr), a.reps, a.warmup), path="device tensors")
        except Exception as e:      # float64 conv2d refused on the device
            res["b_parent_device_error"] = f"{type(e).__name__}: {e}"[:600]
            torch.set_num_threads(int(os.environ.get("OMP_NUM_THREADS", "16")))
            c_sr, c_hr = sr.cpu(), hr.cpu()
            ref = parent(c_sr, c_hr)
            res["b_parent"] = dict(wall(lambda: parent(c_sr, c_hr), a.reps, 1),
                                   path=f"CPU tensors, {torch.get_num_threads()} threads (device refused float64 conv2d)")
        res["b_parent"]["psnr"], res["b_parent"]["ssim"] = ref
        print(json.dumps({"b_parent": res["b_parent"]}), flush=True)

    if "metrics" in parts:
        res["c_frame_metrics"] = wall(lambda: harness.frame_metrics(sr, hr), a.reps, a.warmup)

        def with_rgb8():
            sse, ssim, img = ops.frame_metrics(sr.reshape(T, C, H, W), hr.reshape(T, C, H, W), 255.0, rgb8=True)
            return [harness.psnr_from_sse(v, C * H * W) for v in sse.tolist()], ssim.tolist(), img

        res["d_frame_metrics_rgb8"] = wall(with_rgb8, a.reps, a.warmup)
        got = harness.frame_metrics(sr, hr)
        res["c_frame_metrics"]["psnr"], res["c_frame_metrics"]["ssim"] = got["psnr"], got["ssim"]
        if "b_parent" in res:      # the item's values the two paths report (mean SSIM of the frames; PSNR of the summed error)
            res["ssim_item_diff"] = abs(sum(got["ssim"]) / T - res["b_parent"]["ssim"])
        print(json.dumps({"c": res["c_frame_metrics"]["median_ms"], "d": res["d_frame_metrics_rgb8"]["median_ms"]}), flush=True)

    if "kernel" in parts:
        s4, h4 = sr.reshape(T, C, H, W), hr.reshape(T, C, H, W)
        out = {}
        for tag, flag in (("kernel", False), ("kernel_rgb8", True)):
            for _ in range(a.warmup):
                ops.frame_metrics(s4, h4, 255.0, rgb8=flag)
            us = []
            for _ in range(a.reps):
                with ops.profile() as prof:
                    ops.frame_metrics(s4, h4, 255.0, rgb8=flag)
                    us.append(prof.summary()["frame_metrics"]["ms"] * 1e3)
            n = T * C * H * W
            algo = 8 * n + (n if flag else 0)
            halo = 8 * T * C * staged_samples(H, W) + (n if flag else 0)
            med = statistics.median(us)
            out[tag] = {"median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                        "algorithmic_bytes": algo, "bytes_with_halo": halo, "halo_overfetch": round(staged_samples(H, W) / (H * W), 4),
                        "algorithmic_GBs": round(algo / med / 1e3, 1), "fraction_of_peak": round(algo / (med * 1e-6) / (a.peak_tbs * 1e12), 4),
                        "timing": "device events around the eavsr_frame_metrics_f32 call (tile kernel + per-frame sum kernel)"}
        res.update(out)
        res["peak_tbs"] = a.peak_tbs
        res["partials_per_frame"] = ops.lib().eavsr_frame_metrics_partials(T, C, H, W)

    if "a_forward" in res and "c_frame_metrics" in res:
        res["c_over_a"] = round(res["c_frame_metrics"]["median_ms"] / res["a_forward"]["median_ms"], 5)
    if "b_parent" in res and "c_frame_metrics" in res:
        res["b_over_c"] = round(res["b_parent"]["median_ms"] / res["c_frame_metrics"]["median_ms"], 2)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
