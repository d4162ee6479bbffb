"""What writing the SR frames costs: the device PNG encoder (csrc/png.hip) at F x 2160 x 3840 x 3 bytes, and
`harness.super_resolve` with `out_dir` set, `png_encoder="host"` against `"device"`.  One process, nothing is retried.

  kernels   `ops.png_filter` and `ops.deflate_huffman` (32-row stripes) on frames already on the device, into preallocated outputs
            where the op takes one.  Device events around --launches back-to-back calls, microseconds per call, median of --rounds
            rounds with the two alternated inside a round.  Bytes = read + written; fraction of --peak-tbs on those bytes.
  size      the device streams against the raw scanlines and against `write_png`'s file for the same frames (zlib level 6 on
            filter-0 scanlines), and `write_png`'s host time per frame on this machine's host, wall clock.
  small     the 256 x 256 image of tests/test_hip_png.py: the device stream against zlib's own Huffman-only coder framed the same way.
  scene     `super_resolve` of a --scene-frames x 540 x 960 scene (x4: 2160 x 3840 frames), fp16 backbone, frame_chunk 5, files
            written to --tmp: frames/s with the host encoder and with the device encoder, alternated, --scene-rounds rounds each.

Run it from a checkout: the test image of `small` and zlib's Huffman-only framing come from tests/png_images.py and tests/png_ref.py.

    timeout -k 10 900 python tools/gpu_png_time.py --out profiles/r16_png_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, C = 2160, 3840, 3


def event_us(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / launches


def camera_like(h, w, c, seed):
    """smooth gradients spanning the frame (whatever its size, so nothing saturates) plus sigma 3 noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 80 * np.sin(6.0 * x / w + k) * np.cos(4.0 * y / h) + 30.0 * x / w for k in range(c)], 2)
    return np.clip(base + rng.normal(0, 3, (h, w, c)), 0, 255).round().astype(np.uint8)


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--scene-frames", type=int, default=10)
    ap.add_argument("--scene-rounds", type=int, default=2)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernels' fractions are quoted against, TB/s")
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_png_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import harness, networks as Nw, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    from tests import png_images as I
    from tests import png_ref as P
    dev = torch.device("cuda:0")
    F = a.frames
    frames = np.stack([camera_like(H, W, C, seed=k) for k in range(F)])
    x = torch.from_numpy(frames).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "frames": [F, H, W, C], "peak_tbs": a.peak_tbs, "stripe_rows": 32,
           "image": "smooth gradients spanning the frame plus sigma 3 noise (camera_like)",
           "timing": f"device events around {a.launches} back-to-back calls, us per call; median of {a.rounds} rounds, the two passes "
                     "alternated inside a round"}

    # kernels
    rows = ops.png_filter(x)
    flat = rows.view(F, -1)
    stripe = 32 * rows.shape[2]
    ws = torch.empty(ops.deflate_workspace_bytes(F, flat.shape[1], stripe), device=dev, dtype=torch.uint8)
    enc = ops.deflate_huffman(flat, stripe, workspace=ws)
    sizes = enc.sizes.tolist()
    us = {"filter": [], "deflate": []}
    for _ in range(a.rounds):
        us["filter"].append(event_us(lambda: ops.png_filter(x, out=rows), a.launches))
        us["deflate"].append(event_us(lambda: ops.deflate_huffman(flat, stripe, workspace=ws), a.launches))
    fb = x.numel() + rows.numel()
    db = 2 * rows.numel() + 3 * sum(sizes)      # two reads of the scanlines; the stripes written, then read and written again by the gather
    kf, kd = med(us["filter"]), med(us["deflate"])
    res["kernels"] = {
        "filter_us": kf, "filter_us_rounds": [round(v, 3) for v in us["filter"]], "filter_bytes": fb,
        "filter_fraction_of_peak": round(fb / (kf * 1e-6) / (a.peak_tbs * 1e12), 4), "filter_ms_per_frame": round(kf / F / 1e3, 4),
        "deflate_us": kd, "deflate_us_rounds": [round(v, 3) for v in us["deflate"]], "deflate_bytes": db,
        "deflate_fraction_of_peak": round(db / (kd * 1e-6) / (a.peak_tbs * 1e12), 4), "deflate_ms_per_frame": round(kd / F / 1e3, 4)}
    print(json.dumps({"kernels": res["kernels"]}), flush=True)

    # size
    tmp = a.tmp or tempfile.mkdtemp(prefix="png_time_")
    host_ms, host_bytes = [], []
    for k in range(min(F, 2)):
        t0 = time.perf_counter()
        path = harness.write_png(torch.from_numpy(frames[k]), os.path.join(tmp, "host_%d.png" % k), hwc=True)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        host_bytes.append(os.path.getsize(path))
    files = harness.encode_png_frames(x[:2])
    ok = True
    for k, data in enumerate(files):      # read_png's Python unfilter loops take a while at this size: two frames
        path = os.path.join(tmp, "dev_%d.png" % k)
        with open(path, "wb") as f:
            f.write(data)
        ok = ok and torch.equal(harness.read_png(path), torch.from_numpy(frames[k]).permute(2, 0, 1))
    raw = int(rows[0].numel())
    res["size"] = {"raw_scanline_bytes": raw, "device_stream_bytes": sizes, "device_over_raw": [round(s / raw, 4) for s in sizes],
                   "write_png_file_bytes": host_bytes, "device_file_bytes": [len(f) for f in files],
                   "device_over_write_png": [round(len(f) / b, 4) for f, b in zip(files, host_bytes)],
                   "write_png_host_ms_per_frame": [round(v, 1) for v in host_ms], "device_files_decode_to_the_frames": bool(ok)}
    print(json.dumps({"size": res["size"]}), flush=True)

    # the 256 x 256 image of the test
    small = I.gradient_noise(256, 256, 3, seed=6)
    s_enc = ops.png_encode(torch.from_numpy(small[None]).to(dev))
    s_dev = int(s_enc.sizes[0].item())
    s_ref = len(P.huffman_only_stripes(P.filter_rows(small).tobytes(), 32 * (1 + 256 * 3)))
    res["small"] = {"image": [256, 256, 3], "device_stream_bytes": s_dev, "zlib_huffman_only_bytes": s_ref, "ratio": round(s_dev / s_ref, 4)}
    print(json.dumps({"small": res["small"]}), flush=True)

    # super_resolve, files written, host encoder against device encoder
    t = a.scene_frames
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
    fixed = {k: v for k, v in net.state_dict().items() if k.endswith(("regular_matrix", "mean", "std"))}
    net.load_state_dict(fill_state_dict(shapes_of(net.state_dict()), "trained_like", 0, fixed=fixed), strict=True)
    net = net.to(dev).eval()
    lr = (synthetic_clip(1, t, 540, 960, seed=4)[0] * 255).round().to(torch.uint8).to(dev)
    fps = {"host": [], "device": []}
    with Nw.backbone_dtype("fp16"):
        harness.super_resolve(net, lr[:5], frame_chunk=5)      # warm-up, nothing written
        for _ in range(a.scene_rounds):
            for encoder in ("host", "device"):
                out = harness.super_resolve(net, lr, out_dir=os.path.join(tmp, "scene_" + encoder), frame_chunk=5, png_encoder=encoder)
                fps[encoder].append(out["frames_per_s"])
        nofile = harness.super_resolve(net, lr, frame_chunk=5)["frames_per_s"]
    res["scene"] = {"frames": [t, 3, 540, 960], "scale": 4, "backbone": "fp16", "frame_chunk": 5,
                    "timing": "super_resolve's own wall clock (device-synchronised on both sides), files written to a local directory; "
                              "encoders alternated",
                    "frames_per_s_host": [round(v, 3) for v in fps["host"]], "frames_per_s_device": [round(v, 3) for v in fps["device"]],
                    "frames_per_s_without_files": round(nofile, 3),
                    "device_over_host": round(statistics.median(fps["device"]) / statistics.median(fps["host"]), 2)}
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
