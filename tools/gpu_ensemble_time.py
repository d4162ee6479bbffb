"""What the self-ensemble costs.  No number here is a pass/fail bound; nothing is retried.

  dihedral        per mode k: `ops.dihedral` of 15 x 3 x 540 x 960 fp32 frames against the torch restatement (`flip` / `transpose` and
                  `.contiguous()`; mode 0: `clone`).  Bytes: 8 per sample (read once, written once); fraction of --peak-tbs.
  blend_dihedral  per mode k: one 15 x 3 x 1152 x 2048 SR tile (for a transposed mode stored as 2048 x 1152), the strided view
                  `forward_long` holds, into the 15 x 3 x 2160 x 3840 accumulator at (1008, 1792): `ops.blend_dihedral` against
                  `ops.tile_blend` at that shape IN THE SAME RUN (untouched code: the yardstick) and against the torch restatement on
                  the device, `acc[win] += w * inv_k(sr)` with w = wy[:, None] * wx[None, :] prepared outside the timed call.  12
                  bytes per sample.
  scene           `harness.super_resolve` of the 15 x 540 x 960 scene of tools/gpu_tile_time.py (synthetic weights, uint8 frames on
                  the device, `frame_chunk=3`, no files, no metrics) with ensemble None and 8, untiled and with tile 288 x 512: seconds
                  and `peak_bytes` of one run each after one warm-up run each.  --no-scene leaves it out.
  distance        with the same synthetic weights, on 3 frames of 288 x 512: the PSNR (peak 1) of the ensemble-of-8 output against the
                  plain output.  It says how far the modes disagree for THESE weights; nothing about a trained model, and nothing
                  about quality.

Timing as tools/gpu_tile_time.py: device events around ONE call, --reps calls per variant and round, the variants alternated inside a
round, --rounds rounds; the median over all calls and the spread of the rounds' medians.  Every kernel result is compared with its
restatement, bit for bit, before anything is timed.

    timeout -k 10 1100 python tools/gpu_ensemble_time.py --out profiles/r21_ensemble_time.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from argparse import Namespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_tile_time import measure, psnr      # noqa: E402 -- one timing rule for both tools


def g(x, k):
    a = x.flip(-1) if k & 1 else x
    b = a.flip(-2) if k & 2 else a
    return b.transpose(-1, -2) if k & 4 else b


def inv(z, k):
    u = z.transpose(-1, -2) if k & 4 else z
    a = u.flip(-1) if k & 1 else u
    return a.flip(-2) if k & 2 else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--peak-tbs", type=float, default=8.0, help="HBM peak the fractions are quoted against, TB/s")
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--no-scene", action="store_true", help="the two kernels only")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_ensemble_time: needs a GPU (a measurement does not fall back)")
    from eavsr_amd import harness, ops
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

    gen = torch.Generator(device=dev).manual_seed(1)
    f, h, w, s = a.frames, 540, 960, 4

    # -- dihedral
    x = torch.randn((f, 3, h, w), device=dev, generator=gen)
    nbytes = 8 * x.numel()
    for k in range(8):
        restated = (lambda: x.clone()) if k == 0 else (lambda k=k: g(x, k).contiguous())
        assert torch.equal(ops.dihedral(x, k).view(torch.int32), restated().view(torch.int32)), k
        m = measure({"dihedral": lambda k=k: ops.dihedral(x, k), "torch": restated}, a.reps, a.rounds)
        for v in m.values():
            v["tbs"] = round(nbytes / v["us"] / 1e6, 3)
            v["fraction_of_peak"] = round(nbytes / v["us"] / 1e6 / a.peak_tbs, 3)
        entry = {"frames": list(x.shape), "bytes": nbytes, **m, "dihedral_over_torch": round(m["dihedral"]["us"] / m["torch"]["us"], 3)}
        res["cases"].setdefault("dihedral_15x3x540x960", {})[f"mode_{k}"] = entry
        print("dihedral", k, json.dumps(entry), flush=True)
    del x
    torch.cuda.empty_cache()
    dump()

    # -- blend_dihedral
    th, tw, Y0, X0 = 1152, 2048, 1008, 1792
    wy, wx = torch.rand(th, device=dev, generator=gen), torch.rand(tw, device=dev, generator=gen)
    w2 = (wy[:, None] * wx[None, :]).contiguous()
    acc = torch.randn((1, f, 3, s * h, s * w), device=dev, generator=gen)
    straight = torch.randn((f, 1, 3, th, tw), device=dev, generator=gen)
    nbytes = 12 * straight.numel()
    for k in range(8):
        sr = (straight.view(f, 1, 3, tw, th) if k & 4 else straight).transpose(0, 1)      # the view `forward_long` holds
        plain = straight.transpose(0, 1)

        def restated(target, sr=sr, k=k):
            target[..., Y0:Y0 + th, X0:X0 + tw] += w2 * inv(sr, k)
            return target
        a1, a2 = acc.clone(), acc.clone()
        ops.blend_dihedral(a1, sr, k, Y0, X0, wy, wx)
        restated(a2)
        equal = bool(torch.equal(a1.view(torch.int32), a2.view(torch.int32)))
        del a1, a2
        m = measure({"blend_dihedral": lambda sr=sr, k=k: ops.blend_dihedral(acc, sr, k, Y0, X0, wy, wx),
                     "tile_blend": lambda: ops.tile_blend(acc, plain, Y0, X0, wy, wx), "torch": lambda: restated(acc)}, a.reps, a.rounds)
        for v in m.values():
            v["tbs"] = round(nbytes / v["us"] / 1e6, 3)
            v["fraction_of_peak"] = round(nbytes / v["us"] / 1e6 / a.peak_tbs, 3)
        entry = {"acc": list(acc.shape), "source": list(sr.shape), "at": [Y0, X0], "bytes": nbytes, "equals_torch_bit_for_bit": equal, **m,
                 "blend_dihedral_over_tile_blend": round(m["blend_dihedral"]["us"] / m["tile_blend"]["us"], 3),
                 "blend_dihedral_over_torch": round(m["blend_dihedral"]["us"] / m["torch"]["us"], 3)}
        res["cases"].setdefault("blend_dihedral_1152x2048_into_2160x3840", {})[f"mode_{k}"] = entry
        print("blend_dihedral", k, json.dumps(entry), flush=True)
        acc.normal_(generator=gen)      # 160 blends of random values later the accumulator would hold infinities
    del acc, straight, sr, plain, w2
    torch.cuda.empty_cache()
    dump()

    # -- scene: plain against the ensemble of 8, untiled and tiled; the distance between the two outputs
    if not a.no_scene:
        from eavsr_amd.eavsrp_model import EAVSRP
        from eavsr_amd.utils.synthetic import fill_state_dict, shapes_of, synthetic_clip
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        sd0 = net.state_dict()
        net.load_state_dict(fill_state_dict(shapes_of(sd0), "trained_like", fixed=sd0), strict=True)
        net = net.to(dev).eval()
        clip = (synthetic_clip(1, f, h, w, seed=3)[0] * 255).round().to(torch.uint8).to(dev)      # (f, 3, h, w)
        kept = {}
        res["cases"]["scene_15x540x960"] = kept

        def run(name, **kw):
            harness.super_resolve(net, clip, frame_chunk=3, **kw)      # warm-up
            torch.cuda.empty_cache()
            r = harness.super_resolve(net, clip, frame_chunk=3, **kw)
            kept[name] = {"seconds": round(r["seconds"], 3), "peak_bytes": r["peak_bytes"], "peak_gib": round(r["peak_bytes"] / 2 ** 30, 2),
                          "tiles": len(r["tiles"]), "ensemble": list(r["ensemble"])}
            print("scene", name, json.dumps(kept[name]), flush=True)
            dump()
        run("tiled_288x512_plain", tile=(288, 512))
        run("tiled_288x512_ensemble_8", tile=(288, 512), ensemble=8)
        run("whole_plain")
        run("whole_ensemble_8", ensemble=8)
        kept["seconds_ensemble_over_plain_whole"] = round(kept["whole_ensemble_8"]["seconds"] / kept["whole_plain"]["seconds"], 3)
        kept["seconds_ensemble_over_plain_tiled"] = round(kept["tiled_288x512_ensemble_8"]["seconds"] / kept["tiled_288x512_plain"]["seconds"], 3)
        dump()
        with torch.no_grad():
            few = clip[:3, :, :288, :512].contiguous().unsqueeze(0)
            plain = net.forward_long(few)
            mean = net.forward_ensemble(few, 8)
            one = inv(net.forward_long(few, transform=5), 5)
        res["cases"]["ensemble_against_plain_synthetic_weights"] = {
            "frames": 3, "size": [288, 512], "peak": 1.0,
            "note": "synthetic weights: how far the modes disagree for THESE weights; says nothing about a trained model or about quality",
            "ensemble_8_vs_plain_db": round(psnr(mean, plain), 2), "mode_5_turned_back_vs_plain_db": round(psnr(one, plain), 2)}
        print("distance", json.dumps(res["cases"]["ensemble_against_plain_synthetic_weights"]), flush=True)
    dump()


if __name__ == "__main__":
    main()
