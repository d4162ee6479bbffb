"""What reading PNG frames costs: the device scanline unfilter (csrc/png_decode.hip), the host inflate beside it, and
`harness.decode_png_frames` / `harness.super_resolve` from paths with the host decoder (`read_png`) against the device decoder.
One process, nothing is retried.

  kernels   `ops.png_unfilter` at F x 2160 x 3840 x 3 and F x 720 x 1280 x 3 on scanlines already on the device, into a preallocated
            output: five inputs of one pure filter type each and the adaptive choice of tests/png_ref.py, all of the same camera-like
            image.  Device events around --launches back-to-back calls, median of --rounds rounds, the six inputs alternated inside a
            round.  One wave per frame: a launch's time is a frame's latency, so it is quoted per launch and per frame at F = --frames
            and at F = 256 (a wave on every CU).  Bytes = scanlines read + planes written; fraction of --peak-tbs.
  chunk     16 files of 720 x 1280 x 3 (adaptive filters, zlib level 6): the pool's inflate alone (`inflate_png_frames`, wall clock),
            the copy and the kernel alone (device events), `decode_png_frames` over 8 chunks in a loop, end to end in frames/s; and
            `read_png` of two of the files.
  scene     `super_resolve` of a --scene-frames x 540 x 960 scene (the one of profiles/r16_png_time.json) from PNG paths with both
            decoders: wall clock around the whole call, decode included.

Run it from a checkout (the filters come from tests/png_ref.py):

    timeout -k 10 900 python tools/gpu_png_decode_time.py --out profiles/r17_png_decode_time.json
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
import zlib
from argparse import Namespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C = 3
KINDS = ("none", "sub", "up", "average", "paeth", "adaptive")


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


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def scanlines(P, img):
    """the six inputs of one image: (6, H, 1 + W C)"""
    cand = P.filter_candidates(img)
    h = cand.shape[1]
    best = P.choose_filters(P.row_costs(cand))
    out = []
    for k in range(6):
        ft = np.full(h, k) if k < 5 else best
        out.append(np.concatenate([ft.astype(np.uint8)[:, None], cand[ft, np.arange(h)]], 1))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--scene-frames", type=int, default=10)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the kernel's fractions are quoted against, TB/s")
    ap.add_argument("--skip-scene", action="store_true")
    ap.add_argument("--tmp", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_png_decode_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import harness, networks as Nw, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
    from tests import png_ref as P
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs,
           "image": "smooth gradients spanning the frame plus sigma 3 noise (camera_like)",
           "timing": f"device events around {a.launches} back-to-back calls, us per call; median / min / max of {a.rounds} rounds, the "
                     "inputs alternated inside a round"}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    # kernels
    res["kernels"] = {}
    for (h, w) in ((720, 1280), (2160, 3840)):
        six = scanlines(P, camera_like(h, w, C, seed=1))
        entry = {}
        for F in (a.frames, 256) if h == 720 else (a.frames,):
            rows = [torch.from_numpy(six[k]).to(dev).unsqueeze(0).repeat(F, 1, 1).contiguous() for k in range(6)]
            out = torch.empty((F, C, h, w), device=dev, dtype=torch.uint8)
            for k in range(6):
                ops.png_unfilter(rows[k], C, out=out)      # warm-up
            us = {k: [] for k in KINDS}
            for _ in range(a.rounds):
                for k, kind in enumerate(KINDS):
                    us[kind].append(event_us(lambda: ops.png_unfilter(rows[k], C, out=out), a.launches))
            nbytes = rows[0].numel() + out.numel()
            entry[f"F{F}"] = {kind: {"us_per_launch": spread(us[kind]), "ms_per_frame": round(statistics.median(us[kind]) / F / 1e3, 4),
                                    "bytes": nbytes,
                                    "fraction_of_peak": round(nbytes / (statistics.median(us[kind]) * 1e-6) / (a.peak_tbs * 1e12), 5)}
                              for kind in KINDS}
            del rows, out
        res["kernels"][f"{h}x{w}x{C}"] = entry
        print(json.dumps({f"{h}x{w}": entry}), flush=True)
        dump()

    # a chunk of 16 files of 720 x 1280 x 3
    tmp = a.tmp or tempfile.mkdtemp(prefix="png_decode_time_")
    h, w = 720, 1280
    imgs = [camera_like(h, w, C, seed=10 + k) for k in range(16)]
    files = [P.png_file(zlib.compress(P.filter_rows(im).tobytes(), 6), h, w, C) for im in imgs]
    paths = []
    for k, data in enumerate(files):
        paths.append(os.path.join(tmp, "%05d.png" % k))
        with open(paths[-1], "wb") as f:
            f.write(data)
    threads = min(16, len(os.sched_getaffinity(0)))
    got = harness.decode_png_frames(paths, dev)
    ok = all(torch.equal(got[k].cpu(), torch.from_numpy(imgs[k]).permute(2, 0, 1)) for k in range(16))
    inflate_ms = []
    for _ in range(a.rounds + 1):
        t0 = time.perf_counter()
        rows_host = harness.inflate_png_frames(paths)[0]
        inflate_ms.append((time.perf_counter() - t0) * 1e3)
    inflate_ms = inflate_ms[1:]
    dev_rows = torch.empty(tuple(rows_host.shape), device=dev, dtype=torch.uint8)
    out = torch.empty((16, C, h, w), device=dev, dtype=torch.uint8)
    copy_us, kern_us = [], []
    for _ in range(a.rounds):
        copy_us.append(event_us(lambda: dev_rows.copy_(rows_host, non_blocking=True), a.launches))
        kern_us.append(event_us(lambda: ops.png_unfilter(dev_rows, C, out=out), a.launches))
    fps = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _k in range(8):
            harness.decode_png_frames(paths, dev, out=out)
        torch.cuda.synchronize()
        fps.append(8 * 16 / (time.perf_counter() - t0))
    read_ms = []
    for k in range(2):
        t0 = time.perf_counter()
        ref = harness.read_png(paths[k])
        read_ms.append((time.perf_counter() - t0) * 1e3)
        ok = ok and torch.equal(ref, got[k].cpu())
    copy_kernel_ms = (statistics.median(copy_us) + statistics.median(kern_us)) / 1e3
    res["chunk"] = {"files": [16, h, w, C], "file_bytes": [len(f) for f in files], "threads": threads, "decodes_to_the_images": bool(ok),
                    "inflate_ms_per_chunk": spread(inflate_ms), "copy_us_per_chunk": spread(copy_us), "kernel_us_per_chunk": spread(kern_us),
                    "copy_plus_kernel_ms": round(copy_kernel_ms, 3),
                    "copy_plus_kernel_is_shorter_than_the_inflate": bool(copy_kernel_ms < statistics.median(inflate_ms)),
                    "decode_png_frames_frames_per_s": spread(fps),
                    "inflate_alone_frames_per_s": round(16 / (statistics.median(inflate_ms) * 1e-3), 1),
                    "read_png_ms_per_frame": [round(v, 1) for v in read_ms],
                    "read_png_frames_per_s": round(1e3 / statistics.median(read_ms), 3)}
    print(json.dumps({"chunk": res["chunk"]}), flush=True)
    dump()

    # super_resolve from paths, host decoder against device decoder
    if not a.skip_scene:
        t = a.scene_frames
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        fixed = {k: v for k, v in net.state_dict().items() if k.endswith(("regular_matrix", "mean", "std"))}
        net.load_state_dict(fill_state_dict(shapes_of(net.state_dict()), "trained_like", 0, fixed=fixed), strict=True)
        net = net.to(dev).eval()
        lr = (synthetic_clip(1, t, 540, 960, seed=4)[0] * 255).round().to(torch.uint8)
        scene = [os.path.join(tmp, "scene", "000_%05d.png" % i) for i in range(t)]
        os.makedirs(os.path.dirname(scene[0]), exist_ok=True)
        for i in range(t):      # adaptive filters, as a real encoder writes them
            with open(scene[i], "wb") as f:
                f.write(P.png_file(zlib.compress(P.filter_rows(lr[i].permute(1, 2, 0).numpy()).tobytes(), 6), 540, 960, C))
        wall = {}
        with Nw.backbone_dtype("fp16"):
            harness.super_resolve(net, lr[:5].to(dev), frame_chunk=5)      # warm-up
            for decoder in ("device", "host"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = harness.super_resolve(net, scene, frame_chunk=5, png_decoder=decoder)
                torch.cuda.synchronize()
                wall[decoder] = {"wall_s": round(time.perf_counter() - t0, 3), "forward_s": round(r["seconds"], 3)}
                wall[decoder]["frames_per_s_wall"] = round(t / wall[decoder]["wall_s"], 3)
        res["scene"] = {"frames": [t, 3, 540, 960], "scale": 4, "backbone": "fp16", "frame_chunk": 5, "rounds": 1,
                        "timing": "wall clock around the whole super_resolve call (device-synchronised), decode included; no files written",
                        **wall, "device_over_host": round(wall["host"]["wall_s"] / wall["device"]["wall_s"], 2)}
        print(json.dumps({"scene": res["scene"]}), flush=True)
    if not a.tmp:
        shutil.rmtree(tmp, ignore_errors=True)
    dump()
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
