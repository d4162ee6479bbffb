"""What spatial tiling costs.  No number here is a pass/fail bound; nothing is retried.

  ingest_window   15 x 3 x 540 x 960 uint8 frames, the window 288 x 512 at (252, 448) (the last tile of the 288 x 512 plan) in the
                  three layouts: `ops.ingest_window` against the torch restatement `u8_to_f32(x[..., window].contiguous())` (fp32:
                  the `.contiguous()` alone), and against `u8_to_f32` of an equal-sized contiguous tensor (fp32: a `clone`).
  tile_blend      one 15 x 3 x 1152 x 2048 SR tile (288 x 512 at x4) into the 15 x 3 x 2160 x 3840 accumulator, from the strided view
                  `forward_long` holds: `ops.tile_blend` against the torch restatement `acc[window] += w * v` with w = wy[:, None] *
                  wx[None, :] prepared outside the timed call.  Bytes: 12 per sample (the accumulator read and written, the tile
                  read); fraction of --peak-tbs.
  scene           `harness.super_resolve` of a 15 x 540 x 960 scene (synthetic weights, uint8 frames on the device, no files, no
                  metrics), whole and with tile 288 x 512 at overlap 32: seconds and `peak_bytes` of one run each after one warm-up
                  run each, the recompute factor (seconds tiled / seconds whole) beside (tiled area / frame area).  --no-scene
                  leaves it out.
  seam            with the same synthetic weights, the PSNR (peak 1) of the tiled output against the whole-frame output in a band of
                  16 SR columns on either side of the vertical seam's centre line and in a 64 x 64 SR patch at a tile's centre.  It
                  says how far the per-tile networks disagree with the whole-frame one for THESE weights; nothing about a trained model.

Timing of the two kernels as tools/gpu_pad_time.py times the ingest: device events around ONE call, --reps calls per variant and
round, the variants alternated inside a round, --rounds rounds; the median over all calls and the spread of the rounds' medians.
Every kernel result is compared with its restatement before anything is timed (the ingest bit for bit; the blend bit for bit as
well -- torch's `w * v` then `+=` rounds the same three operations).

    timeout -k 10 900 python tools/gpu_tile_time.py --out profiles/r20_tile_time.json
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


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return math.inf if mse == 0 else 10.0 * math.log10(1.0 / mse)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the fractions are quoted against, TB/s")
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--no-scene", action="store_true", help="the two kernels only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_tile_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import harness, ops
    from eavsr_amd.segments import plan_tiles, tile_axis, tile_weights
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "peak_tbs": a.peak_tbs,
           "timing": f"kernels: device events around one call, us; {a.reps} calls per variant and round, variants alternated, {a.rounds} "
                     "rounds; 'us' is the median of all calls, 'round_medians' the spread of the rounds' medians.  scene: one "
                     "run after one warm-up run, host clock between device synchronisations", "cases": {}}

    def dump():
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")

    g = torch.Generator(device=dev).manual_seed(1)
    f, h, w, s = a.frames, 540, 960, 4
    tile, overlap = (288, 512), 32
    tiles = plan_tiles(h, w, tile, overlap)
    y0, y1, x0, x1 = tiles[-1]
    wh, ww = y1 - y0, x1 - x0

    # -- ingest_window
    planes = torch.randint(0, 256, (f, 3, h, w), dtype=torch.uint8, device=dev, generator=g)
    layouts = {"u8_planes": planes, "u8_interleaved": planes.permute(0, 2, 3, 1).contiguous(), "f32_planes": ops.u8_to_f32(planes)}
    for layout, src in layouts.items():
        hwc = layout == "u8_interleaved"
        part = (lambda src=src: src[:, y0:y1, x0:x1]) if hwc else (lambda src=src: src[..., y0:y1, x0:x1])
        equal = part().contiguous()
        if src.dtype == torch.uint8:
            variants = {"ingest_window": lambda src=src, hwc=hwc: ops.ingest_window(src, y0, x0, wh, ww, hwc=hwc),
                        "torch_slice": lambda part=part, hwc=hwc: ops.u8_to_f32(part().contiguous(), hwc=hwc),
                        "contiguous_equal_size": lambda equal=equal, hwc=hwc: ops.u8_to_f32(equal, hwc=hwc)}
        else:
            variants = {"ingest_window": lambda src=src: ops.ingest_window(src, y0, x0, wh, ww),
                        "torch_slice": lambda part=part: part().contiguous(),
                        "contiguous_equal_size": lambda equal=equal: equal.clone()}
        assert torch.equal(variants["ingest_window"]().view(torch.int32), variants["torch_slice"]().view(torch.int32)), layout
        m = measure(variants, a.reps, a.rounds)
        nbytes = f * 3 * wh * ww * (src.element_size() + 4)
        for v in m.values():
            v["bytes"] = nbytes
            v["fraction_of_peak"] = round(nbytes / v["us"] / 1e6 / a.peak_tbs, 3)
        entry = {"source": list(src.shape), "window": [y0, y1, x0, x1], **m,
                 "ingest_window_over_torch_slice": round(m["ingest_window"]["us"] / m["torch_slice"]["us"], 3),
                 "ingest_window_over_contiguous_equal_size": round(m["ingest_window"]["us"] / m["contiguous_equal_size"]["us"], 3)}
        res["cases"].setdefault("ingest_window_288x512_of_540x960", {})[layout] = entry
        print("ingest_window", layout, json.dumps(entry), flush=True)
    del planes, layouts, src, equal, variants
    dump()

    # -- tile_blend
    wy = torch.from_numpy(tile_weights(h, tile_axis(h, tile[0], overlap), s)).to(dev)[-1]
    wx = torch.from_numpy(tile_weights(w, tile_axis(w, tile[1], overlap), s)).to(dev)[-1]
    acc = torch.randn((1, f, 3, s * h, s * w), device=dev, generator=g)
    frame_major = torch.randn((f, 1, 3, s * wh, s * ww), device=dev, generator=g)
    sr = frame_major.transpose(0, 1)      # the view `forward_long` holds
    w2 = (wy[:, None] * wx[None, :]).contiguous()
    Y0, X0 = s * y0, s * x0

    def restated(target):
        target[..., Y0:Y0 + s * wh, X0:X0 + s * ww] += w2 * sr
        return target
    a1, a2 = acc.clone(), acc.clone()
    ops.tile_blend(a1, sr, Y0, X0, wy, wx)
    restated(a2)
    res["cases"]["tile_blend_equals_torch_bit_for_bit"] = bool(torch.equal(a1.view(torch.int32), a2.view(torch.int32)))
    res["cases"]["tile_blend_max_abs_diff_to_torch"] = float((a1 - a2).abs().max())
    del a1, a2
    m = measure({"tile_blend": lambda: ops.tile_blend(acc, sr, Y0, X0, wy, wx), "torch": lambda: restated(acc)}, a.reps, a.rounds)
    nbytes = 12 * sr.numel()
    for v in m.values():
        v["bytes"] = nbytes
        v["tbs"] = round(nbytes / v["us"] / 1e6, 3)
        v["fraction_of_peak"] = round(nbytes / v["us"] / 1e6 / a.peak_tbs, 3)
    entry = {"acc": list(acc.shape), "tile": list(sr.shape), "at": [Y0, X0], **m,
             "tile_blend_over_torch": round(m["tile_blend"]["us"] / m["torch"]["us"], 3)}
    res["cases"]["tile_blend_1152x2048_into_2160x3840"] = entry
    print("tile_blend", json.dumps(entry), flush=True)
    del acc, frame_major, sr, w2
    torch.cuda.empty_cache()
    dump()

    # -- scene: whole against tiled, and the seam
    if not a.no_scene:
        from eavsr_amd.eavsrp_model import EAVSRP
        from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        sd0 = net.state_dict()
        net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
        net = net.to(dev).eval()
        clip = (synthetic_clip(1, f, h, w, seed=3)[0] * 255).round().to(torch.uint8).to(dev)      # (f, 3, h, w)
        kept = {}

        def run(name, **kw):
            harness.super_resolve(net, clip, frame_chunk=3, **kw)      # warm-up
            torch.cuda.empty_cache()
            r = harness.super_resolve(net, clip, frame_chunk=3, **kw)
            kept[name] = {"seconds": round(r["seconds"], 3), "peak_bytes": r["peak_bytes"], "peak_gib": round(r["peak_bytes"] / 2 ** 30, 2),
                          "tiles": [list(v) for v in r["tiles"]]}
            print("scene", name, json.dumps(kept[name]), flush=True)
        run("tiled_288x512_overlap_32", tile=tile, tile_overlap=overlap)
        res["cases"]["scene_15x540x960"] = kept
        dump()
        run("whole")
        area = sum((b - t) * (r - l) for t, b, l, r in tiles) / float(h * w)
        kept["tiled_area_over_frame_area"] = round(area, 3)
        kept["seconds_tiled_over_whole"] = round(kept["tiled_288x512_overlap_32"]["seconds"] / kept["whole"]["seconds"], 3)
        kept["peak_tiled_over_whole"] = round(kept["tiled_288x512_overlap_32"]["peak_bytes"] / kept["whole"]["peak_bytes"], 3)
        dump()
        # the seam, on 3 frames (the outputs are held whole here)
        with torch.no_grad():
            few = clip[:3].unsqueeze(0)
            whole = net.forward_long(few, frame_chunk=3)
            tiled = net.forward_tiled(few, tile, overlap=overlap, frame_chunk=3)
        cols = tile_axis(w, tile[1], overlap)
        seam_x = s * (cols[1][0] + cols[0][1]) // 2      # the centre line of the two column windows' overlap
        cy, cx = s * tile[0] // 2, s * tile[1] // 2       # the first tile's centre
        res["cases"]["seam_psnr_synthetic_weights"] = {
            "frames": 3, "peak": 1.0, "note": "synthetic weights: says nothing about a trained model",
            "seam_band_32_columns": round(psnr(tiled[..., seam_x - 16:seam_x + 16], whole[..., seam_x - 16:seam_x + 16]), 2),
            "tile_centre_64x64": round(psnr(tiled[..., cy - 32:cy + 32, cx - 32:cx + 32], whole[..., cy - 32:cy + 32, cx - 32:cx + 32]), 2),
            "whole_frame": round(psnr(tiled, whole), 2)}
        print("seam", json.dumps(res["cases"]["seam_psnr_synthetic_weights"]), flush=True)
    dump()


if __name__ == "__main__":
    main()
