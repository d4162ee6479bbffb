"""The temporal metrics of one test item against producing it: 7 x 3 x 720 x 1280 (BASELINE configs[1]'s frame size) on one GPU.

  (a) forward   the x4 model on the item's 1 x 7 x 3 x 180 x 320 clip
  (b) flows     `harness.pair_flows` on the 7 HR frames (PWC-Net, both directions of the 6 pairs) and the forward flow of the SR
                frames -- what flow_from="hr" estimates per item; synthetic PWC-Net weights (none ship)
  (c) kernel    `ops.temporal_metrics` on those flows (both launches), wall clock and device events, algorithmic bytes
  (d) torch     the same definition restated with torch on the device (`grid_sample` for the bilinear reads, masks, float64 sums):
                fused multiply-adds and another summation order, so close to (c), not equal; the differences are recorded
  (e) harness   `harness.temporal_metrics`, flows included: what `evaluate(per_frame=True, temporal=...)` adds per item

Wall times: after --warmup calls, the median of --reps calls, each with a device synchronise on both sides.  No ratio is set in
advance: the file records what was measured.

    python tools/gpu_temporal_time.py [--reps 20] [--warmup 3] [--parts forward,flows,kernel,torch,harness] [--out FILE]

`rocprofv3 --kernel-trace --stats -- python tools/gpu_temporal_time.py --parts kernel --reps 5` names the kernels (no --pmc in the
same run).
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
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, C, H, W, SCALE = 7, 3, 720, 1280, 4
DEFAULT_OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22_temporal_time.json")


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


def torch_restatement(seq, fw, bw, flow_b, scale=255.0, shares=False):
    """(err, count, epe) per pair by torch ops on the device: the definition of csrc/temporal.hip without its rounding contract.
    shares=True: instead the share of all pixels that pass each of the three tests on its own, and all three, over all pairs"""
    f, c, h, w = seq.shape
    q = torch.clamp(seq * scale, 0, 255).round()
    ys, xs = torch.meshgrid(torch.arange(h, device=seq.device, dtype=torch.float32),
                            torch.arange(w, device=seq.device, dtype=torch.float32), indexing="ij")
    u, v = fw[:, 0], fw[:, 1]
    sx, sy = xs + u, ys + v
    inside = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
    grid = torch.stack([sx * (2.0 / max(w - 1, 1)) - 1.0, sy * (2.0 / max(h - 1, 1)) - 1.0], -1)
    sample = lambda x: F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=True)
    b = sample(bw)
    bu, bv = b[:, 0], b[:, 1]
    m_f, m_b, m_fb = u * u + v * v, bu * bu + bv * bv, (u + bu) ** 2 + (v + bv) ** 2
    right = torch.cat([fw[..., 1:], fw[..., -1:]], 3) - fw
    below = torch.cat([fw[:, :, 1:], fw[:, :, -1:]], 2) - fw
    g = (right * right).sum(1) + (below * below).sum(1)
    consistent, smooth = m_fb <= 0.01 * (m_f + m_b) + 0.5, g <= 0.01 * m_f + 0.002
    valid = inside & consistent & smooth
    if shares:
        share = lambda m: round(float(m.double().mean()), 4)
        return {"inside_frame": share(inside), "forward_backward_consistent": share(consistent), "no_motion_boundary": share(smooth),
                "valid": share(valid), "max_abs_fw_px": round(float(fw.abs().max()), 3)}
    d =(q[:-1] - sample(q[1:])).double()
    err = (d * d * valid[:, None]).sum((1, 2, 3))
    e = (flow_b - fw).double()
    epe = (e * e).sum(1).sqrt().sum((1, 2))
    return err, valid.sum((1, 2)), epe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="forward,flows,kernel,torch,harness")
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fraction is quoted against, TB/s")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    parts = a.parts.split(",")
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.pwc import PWCNET
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "item": [1, T, C, H, W], "reps": a.reps, "warmup": a.warmup,
           "timing": "wall clock, device synchronise on both sides, median of reps",
           "weights": "synthetic (EAVSRP trained_like, PWC-Net default fill seed 7): the flows are not those of a trained estimator"}

    hr = synthetic_clip(1, T, H, W, seed=2).to(dev)
    if "forward" in parts:
        net = EAVSRP(Namespace(predict=False, n_frame=T, n_flow=5, scale=SCALE), None)
        sd0 = net.state_dict()
        net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
        net = net.to(dev).eval()
        lr = synthetic_clip(1, T, H // SCALE, W // SCALE, seed=1).to(dev)
        with torch.no_grad():
            res["a_forward"] = wall(lambda: net(lr), a.reps, a.warmup)
            sr = net(lr).detach().clamp(0, 1)
        del net
    else:
        sr = (hr + torch.randn_like(hr) * (4.0 / 255.0)).clamp(0, 1).contiguous()
    print(json.dumps({k: v for k, v in res.items() if k.startswith("a_")}), flush=True)

    pwc = PWCNET()
    pwc.load_state_dict(fill_state_dict({k: tuple(v.shape) for k, v in pwc.state_dict().items()}, "default", seed=7), strict=True)
    pwc = pwc.to(dev).eval()
    sr4, hr4 = sr.reshape(T, C, H, W), hr.reshape(T, C, H, W)
    if "flows" in parts:
        res["b_flows_hr_both_directions"] = wall(lambda: harness.pair_flows(hr4, pwc), a.reps, a.warmup)
        res["b_flow_sr_forward"] = wall(lambda: harness._flows(sr4, pwc, 255.0, False), a.reps, a.warmup)
        print(json.dumps({"b": res["b_flows_hr_both_directions"]["median_ms"], "b_sr": res["b_flow_sr_forward"]["median_ms"]}), flush=True)
    fw, bw = harness.pair_flows(hr4, pwc)
    flow_b = harness._flows(sr4, pwc, 255.0, False)[0]
    # the synthetic PWC-Net gives nearly the same small, almost constant flow in both directions: the pixels are inside the frame,
    # but fw + bw(s) is nowhere near zero, the consistency test rejects every pixel and no frame sample is read.  The kernel's cost
    # depends on how many pixels are valid, so a second field -- smooth, about 2 pixels, bw = -fw: most pixels valid, every tap
    # read -- is timed as well; `pixel_shares` records what passes each test for both
    small =F.interpolate(torch.randn(T - 1, 2, H // 40, W // 40, device=dev), size=(H, W), mode="bilinear", align_corners=False) * 2.0
    fields = {"pwc_synthetic": (fw, bw, flow_b), "smooth_2px": (small, -small, small + 0.25)}
    res["pixel_shares"] = {tag: torch_restatement(sr4, f_w, b_w, f_b, shares=True) for tag, (f_w, b_w, f_b) in fields.items()}
    print(json.dumps(res["pixel_shares"]), flush=True)

    if "kernel" in parts:
        for tag, (f_w, b_w, f_b) in fields.items():
            out = dict(wall(lambda: ops.temporal_metrics(sr4, f_w, b_w, 255.0, f_b), a.reps, a.warmup))
            us = []
            for _ in range(a.reps):
                with ops.profile() as prof:
                    ops.temporal_metrics(sr4, f_w, b_w, 255.0, f_b)
                    us.append(prof.summary()["temporal_metrics"]["ms"] * 1e3)
            px = (T - 1) * H * W
            algo = 4 * px * (2 + 2 + 2 + 2 * C)      # fw, bw, flow_b, two frames of C planes per pair: each sample once
            med = statistics.median(us)
            err, count, epe = ops.temporal_metrics(sr4, f_w, b_w, 255.0, f_b)
            out.update(device_median_us=round(med, 2), device_min_us=round(min(us), 2), device_max_us=round(max(us), 2),
                       algorithmic_bytes=algo, algorithmic_GBs=round(algo / med / 1e3, 1),
                       fraction_of_peak=round(algo / (med * 1e-6) / (a.peak_tbs * 1e12), 4),
                       valid_share=[round(v / (H * W), 4) for v in count.tolist()],
                       timing_device="device events around the eavsr_temporal_metrics_f32 call (tile kernel + per-pair sum kernel)")
            if not any(count.tolist()):
                out["note"] = ("no pixel is valid, so no frame sample is read: algorithmic_GBs / fraction_of_peak count bytes that were "
                               "not moved and are not a bandwidth")
            res["c_kernel_" + tag] = out
            print(json.dumps({"c_" + tag: out["median_ms"], "us": out["device_median_us"]}), flush=True)
        res["peak_tbs"] = a.peak_tbs
        res["partials_per_pair"] = ops.lib().eavsr_temporal_metrics_partials(T, C, H, W)

    if "torch" in parts:
        for tag, (f_w, b_w, f_b) in fields.items():
            out = dict(wall(lambda: torch_restatement(sr4, f_w, b_w, f_b), a.reps, a.warmup))
            e_t, n_t, p_t = torch_restatement(sr4, f_w, b_w, f_b)
            e_k, n_k, p_k = ops.temporal_metrics(sr4, f_w, b_w, 255.0, f_b)
            rel = lambda x, y: float(((x - y).abs() / y.abs().clamp_min(1e-300)).max())
            out.update(count_differs_by=int((n_t - n_k).abs().max()), err_rel_diff=rel(e_t, e_k), epe_rel_diff=rel(p_t, p_k),
                       note="fp32 torch ops (fused multiply-adds, normalised grid): near the kernel's values, not equal to them")
            res["d_torch_" + tag] = out
            print(json.dumps({"d_" + tag: out["median_ms"]}), flush=True)

    if "harness" in parts:
        res["e_harness_temporal_metrics_hr"] = wall(lambda: harness.temporal_metrics(sr, hr, pwc), a.reps, a.warmup)
        res["e_harness_temporal_metrics_sr"] = wall(lambda: harness.temporal_metrics(sr, None, pwc), a.reps, a.warmup)

    for tag in fields:
        if "c_kernel_" + tag in res and "d_torch_" + tag in res:
            res[f"d_over_c_{tag}"] = round(res["d_torch_" + tag]["median_ms"] / res["c_kernel_" + tag]["median_ms"], 3)
            res["d_over_c_basis"] = "wall clock of the torch restatement over wall clock of ops.temporal_metrics (not its device-event time)"
    if "a_forward" in res and "c_kernel_smooth_2px" in res:
        res["c_over_a"] = round(res["c_kernel_smooth_2px"]["median_ms"] / res["a_forward"]["median_ms"], 5)
    if "a_forward" in res and "e_harness_temporal_metrics_hr" in res:
        res["e_over_a"] = round(res["e_harness_temporal_metrics_hr"]["median_ms"] / res["a_forward"]["median_ms"], 4)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
