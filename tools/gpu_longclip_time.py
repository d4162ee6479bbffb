"""Measurements of the long-clip path: cost of chunking against `forward`, the host cache, a scene that did not fit,
the 8-bit ingest kernel.  Device events, median of --reps (>= 5), the variants of one case alternated round by round.

    python tools/gpu_longclip_time.py --case chunk15 | chunk_sub | host15 | scene50 | ingest | parity  [--out FILE] [--reps 5]

Every case prints one JSON object and, with --out, merges it into that JSON file under the case's name.
"""
import argparse
import json
import os
import statistics
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eavsr_amd import networks as Nw, ops                      # noqa: E402
from eavsr_amd.eavsrp_model import EAVSRP                      # noqa: E402
from eavsr_amd.utils.synthetic import fill_state_dict, synthetic_clip      # noqa: E402
from eavsr_amd.utils.synthetic import shapes_of                # noqa: E402

DEV = torch.device("cuda:0")


def net_x4():
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
    fixed = {k: v for k, v in net.state_dict().items() if k.endswith(("regular_matrix", "mean", "std"))}
    net.load_state_dict(fill_state_dict(shapes_of(net.state_dict()), "trained_like", 0, fixed=fixed), strict=True)
    return net.to(DEV).eval()


def rotate(variants, reps, warmup=1):
    """variants: {name: fn}; every round runs each variant once, in turn.  -> {name: {'ms': median, 'all_ms', 'peak_bytes'}}"""
    times = {k: [] for k in variants}
    peaks = {k: 0 for k in variants}
    for r in range(warmup + reps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            del out
            if r >= warmup:
                times[name].append(e0.elapsed_time(e1))
                peaks[name] = max(peaks[name], torch.cuda.max_memory_allocated())
    return {k: {"ms": statistics.median(v), "all_ms": [round(x, 3) for x in v], "peak_bytes": peaks[k]} for k, v in times.items()}


def drop(first, sr):
    pass


def case_chunk(net, n, t, h, w, dtype, chunks, reps):
    x = synthetic_clip(n, t, h, w, seed=4).to(DEV)
    variants = {"forward": lambda: net(x)}
    for fc in chunks:
        variants[f"forward_long_chunk{fc}"] = lambda fc=fc: net.forward_long(x, frame_chunk=fc)
        variants[f"forward_long_chunk{fc}_sink"] = lambda fc=fc: net.forward_long(x, frame_chunk=fc, sink=drop)
    with torch.no_grad(), Nw.backbone_dtype(dtype):
        res = rotate(variants, reps)
    base = res["forward"]["ms"]
    for v in res.values():
        v["vs_forward"] = round(v["ms"] / base, 4)
    return {"shape": [n, t, 3, h, w], "backbone": dtype or "fp32", "reps": reps, "timing": "device events, median, variants alternated per round",
            "variants": res}


def case_host(net, reps):
    n, t, h, w = 1, 15, 540, 960
    x = synthetic_clip(n, t, h, w, seed=4).to(DEV)
    with torch.no_grad(), Nw.backbone_dtype("fp16"):
        res = rotate({"device_chunk3_sink": lambda: net.forward_long(x, frame_chunk=3, cache="device", sink=drop),
                      "host_chunk3_sink": lambda: net.forward_long(x, frame_chunk=3, cache="host", sink=drop)}, reps)
    # the copy stream's busy share from the bytes it moves: every per-frame tensor goes to the host once and comes back once per
    # reader (pyramid: 4 branches + `spatial` once more for the tail; a branch: its later branches + the tail; a flow: 2 branches)
    px = n * h * w * 4
    pyr = 64 * (1 + 1 / 4 + 1 / 16)
    down = t * px * (pyr + 4 * 64 + 3) + (t - 1) * px * 4
    up = t * px * (4 * pyr + 64 + (3 + 2 + 1 + 0 + 4) * 64 + 3) + (t - 1) * px * 4 * 2
    res["copy_bytes"] = {"device_to_host": down, "host_to_device": up}
    res["host_vs_device"] = round(res["host_chunk3_sink"]["ms"] / res["device_chunk3_sink"]["ms"], 4)
    return {"shape": [n, t, 3, h, w], "backbone": "fp16", "reps": reps, "variants": res}


def case_scene50(net):
    import time
    n, t, h, w = 1, 50, 540, 960
    # (synthetic_clip pans its base image one pixel per frame and has room for 15 frames: a scene of 50 is five such pans)
    clip = torch.cat([synthetic_clip(n, 10, h, w, seed=40 + k) for k in range(t // 10)], 1)
    u8 = (clip * 255).round().to(torch.uint8).pin_memory()
    del clip
    R = n * h * w * 4 * (64 * (1 + 1 / 4 + 1 / 16) + 4 * 64 + 2 * 2 + 3)
    out = {"shape": [n, t, 3, h, w], "backbone": "fp16", "frame_chunk": 3, "cache": "device", "input": "uint8, pinned host memory",
           "R_bytes_per_frame": R, "resident_predicted_bytes": t * R}
    with torch.no_grad(), Nw.backbone_dtype("fp16"):
        net.forward_long(u8[:, :4], frame_chunk=3, sink=drop)      # packed weights
        runs = []
        for _ in range(2):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.time()
            net.forward_long(u8, frame_chunk=3, sink=drop)
            torch.cuda.synchronize()
            runs.append(time.time() - t0)
        out.update(seconds=min(runs), all_seconds=[round(v, 3) for v in runs], frames_per_s=t / min(runs),
                   peak_bytes=torch.cuda.max_memory_allocated())
    return out


def case_ingest(reps):
    f, h, w = 15, 540, 960
    g = torch.Generator().manual_seed(0)
    chw = torch.randint(0, 256, (f, 3, h, w), generator=g, dtype=torch.uint8).to(DEV)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    out = {"shape": [f, 3, h, w], "bytes_per_sample": 5, "hbm_peak_TBps": 8.0}
    for name, src in (("chw", chw), ("hwc", hwc)):
        for _ in range(3):
            ops.u8_to_f32(src)
        ts = []
        for _ in range(max(reps, 20)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.u8_to_f32(src)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        us = statistics.median(ts)
        out[name] = {"us": round(us, 2), "min_us": round(min(ts), 2), "TBps": round(5.0 * src.numel() / (us * 1e-6) / 1e12, 3),
                     "frac_of_8TBps": round(5.0 * src.numel() / (us * 1e-6) / 8e12, 4)}
    return out


def case_parity(net):
    """what tests/test_hip_longclip.py asserts, as figures"""
    out = {}
    x = synthetic_clip(2, 9, 64, 96, seed=5).to(DEV)
    with torch.no_grad():
        want = net(x)
        out["fp32_2x9x3x64x96_max_abs_vs_forward"] = {f"frame_chunk_{fc}": float((net.forward_long(x, frame_chunk=fc) - want).abs().max())
                                                      for fc in (1, 2, 4)}
        out["excepted_layers"] = []
        q = lambda v: torch.clamp(v * 255.0, 0, 255).round()
        psnr = lambda a, b: float("inf") if torch.equal(q(a), q(b)) else float(-10.0 * torch.log10((q(a) - q(b)).div(255.0).pow(2).mean()))
        x6 = synthetic_clip(2, 9, 64, 96, seed=6).to(DEV)
        y32 = net(x6)
        with Nw.backbone_dtype("bf16"):
            whole, chunked = net(x6), net.forward_long(x6, frame_chunk=2)
        out["bf16_2x9x3x64x96"] = {"psnr_whole_batch_vs_fp32_db": psnr(whole, y32), "psnr_frame_chunk_2_vs_fp32_db": psnr(chunked, y32),
                                   "bit_identical": bool(torch.equal(whole, chunked))}
        big = synthetic_clip(1, 6, 540, 960, seed=4).to(DEV)
        with Nw.backbone_dtype("fp16"):
            whole, chunked = net(big), net.forward_long(big, frame_chunk=2)
        out["fp16_1x6x3x540x960"] = {"max_abs_frame_chunk_2_vs_forward": float((whole - chunked).abs().max()),
                                     "psnr_frame_chunk_2_vs_forward_db": psnr(chunked, whole), "bit_identical": bool(torch.equal(whole, chunked))}
        del whole, chunked
        w32, c32 = net(big), net.forward_long(big, frame_chunk=2)
        out["fp32_1x6x3x540x960"] = {"max_abs_frame_chunk_2_vs_forward": float((w32 - c32).abs().max()), "bit_identical": bool(torch.equal(w32, c32))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--out")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    net = net_x4() if a.case != "ingest" else None
    if a.case == "chunk15":
        res = case_chunk(net, 1, 15, 540, 960, "fp16", (1, 3, 15), a.reps)
    elif a.case == "chunk_sub":
        res = case_chunk(net, 2, 7, 180, 320, None, (1, 3, 7), a.reps)
    elif a.case == "host15":
        res = case_host(net, a.reps)
    elif a.case == "scene50":
        res = case_scene50(net)
    elif a.case == "ingest":
        res = case_ingest(a.reps)
    elif a.case == "parity":
        res = case_parity(net)
    else:
        raise SystemExit(f"unknown case {a.case}")
    print(json.dumps({a.case: res}), flush=True)
    if a.out:
        doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
        doc[a.case] = res
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
