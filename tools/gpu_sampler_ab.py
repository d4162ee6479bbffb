"""ONE library (EAVSR_LIB_PATH) on every kernel that holds a bilinear sampler: per kernel the median and the range of
SAMPLES device-event samples (each `reps` back-to-back launches after a warm-up) and a hash of the output bits on ordinary inputs
(sigma = 2 offsets / flows; -0 hashed as +0).  A visit runs the libraries to compare in rotation, one process each, and merges the lines:

    for r in 1 2 3; do for lib in new parent; do EAVSR_LIB_PATH=... python tools/gpu_sampler_ab.py $lib >> out.jsonl; done; done
    python tools/gpu_sampler_ab.py --merge out.jsonl > profiles/r29_sampler_domain_time.json

The lab-only kernels (dcnv2_ws, dcnv2_x9) are timed when the library is a lab build."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SAMPLES = 7


def merge(path):
    runs = [json.loads(l) for l in open(path) if l.startswith("{")]
    out = {"method": f"device events, {SAMPLES} samples of `reps` launches per process after 20 warm-up launches; processes in rotation; "
                     "us per launch: median of all samples of a library, [min, max]; ratio = new / parent of the medians",
           "kernels": {}, "output_bits": {}}
    libs = sorted({r["lib"] for r in runs})
    for k in sorted({k for r in runs for k in r["us"]}):
        row = {}
        for lib in libs:
            s = sorted(v for r in runs if r["lib"] == lib for v in r["us"].get(k, []))
            if s:
                row[lib] = {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "samples": len(s)}
        base = "parent_lab" if k in ("dcnv2_ws", "dcnv2_x9") else "parent"
        new = "new_lab" if k in ("dcnv2_ws", "dcnv2_x9") else "new"
        if base in row and new in row:
            row["ratio"] = round(row[new]["median"] / row[base]["median"], 4)
        out["kernels"][k] = row
        hs = {lib: sorted({r["hash"][k] for r in runs if r["lib"] == lib and k in r["hash"]}) for lib in libs}
        out["output_bits"][k] = "same" if len({h for v in hs.values() for h in v}) == 1 else hs
    print(json.dumps(out, indent=1))


def _canon(o):
    """the output with -0 written as +0 (DESIGN 7p makes flow_warp's empty pixels +0.0; every other bit counts)"""
    if o.is_floating_point():
        return o + 0
    return o.masked_fill((o & 0x7fff) == 0, 0)      # 16-bit IL8 forms travel as integers


def main(tag):
    import torch
    from eavsr_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    R = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev)
    n, c, h, w, dg = 2, 64, 180, 320, 8
    x, off, mask = R(n, c, h, w), R(n, dg * 18, h, w, scale=2.0), torch.rand(n, dg * 9, h, w, generator=gen).to(dev)
    wt, b, flow, flow2 = R(64, c, 3, 3, scale=1 / 24), R(64, scale=0.1), R(n, 2, h, w, scale=2.0), R(n, 2, h, w, scale=0.5)
    heads = torch.cat([R(n, 4 * dg, h, w, scale=0.2) + torch.tensor([1.0, 0, 0, 1.0]).repeat(dg).view(1, 4 * dg, 1, 1).to(dev),
                       R(n, 2 * dg, h, w, scale=1.5), R(n, 9 * dg, h, w, scale=2.0)], 1).contiguous()
    xil, x16 = ops.to_il8(x), ops.to_il8_h16(x, "bf16")
    xg, offg, maskg, wtg = R(n, 48, h, w), off, mask, R(64, 48, 3, 3, scale=1 / 20)      # 6 channels per group: the generic kernel
    hb, wb = 96, 96                                                                        # the training crop: backward kernels
    xb, offb, maskb = R(n, c, hb, wb), R(n, dg * 18, hb, wb, scale=2.0), torch.rand(n, dg * 9, hb, wb, generator=gen).to(dev)
    dyb, dcol, flowb = R(n, 64, hb, wb), R(n, 576, hb, wb), R(n, 2, hb, wb, scale=2.0)

    def il(impl, **kw):
        def f():
            ops.set_dcn_il_impl(impl)
            return ops.dcnv2_il(xil, kw.get("o", off), kw.get("m", mask), wt, b, dg, nprod=6, heads=kw.get("heads", False))
        return f

    def mdc(mode, xx=x, ww=wt):
        def f():
            ops.set_dcn_mode(mode)
            return ops.modulated_deform_conv2d(xx, off, mask, ww, b, 1, 1, 1, 1, dg)
        return f

    todo = [
        ("dcnv2_il2", il("il2"), 200, 0), ("dcnv2_il2_heads", il("il2", o=heads, m=None, heads=True), 200, 0), ("dcnv2_il", il("il"), 200, 0),
        ("dcnv2_il16", lambda: ops.dcnv2_il16(x16, off, mask, wt, b, dg), 200, 0),
        ("dcnv2_il16_heads", lambda: ops.dcnv2_il16(x16, heads, None, wt, b, dg, heads=True), 200, 0),
        ("dcnv2_nchw", mdc("native"), 50, 0), ("dcnv2_generic", mdc("il6", xg, wtg), 10, 0),
        ("dcnv2_bwd", lambda: ops.dcnv2_bwd(xb, offb, maskb, wt, dyb, dg), 50, (1, 2)),
        ("dcnv2_im2col", lambda: ops.dcnv2_im2col(xb, offb, maskb, dg), 100, 0),
        ("dcnv2_col2im", lambda: ops.dcnv2_col2im(xb, offb, maskb, dcol, dg), 50, (1, 2)),
        ("dcnv2_col2im_dx_det", lambda: ops.dcnv2_col2im_dx_det(offb, maskb, dcol, dg), 20, 0),
        ("flow_warp", lambda: ops.flow_warp(x, flow), 200, 0),
        ("flow_warp_border_flow2", lambda: ops.flow_warp(x, flow, padding_mode="border", flow2=flow2), 200, 0),
        ("flow_warp_reflection", lambda: ops.flow_warp(x, flow, padding_mode="reflection"), 200, 0),
        ("flow_warp_single_il8", lambda: ops.flow_warp_single(x, flow, il8=True), 200, 0),
        ("flow_warp_pair_il8_bf16", lambda: ops.flow_warp_pair(x, x, flow, b_il8="bf16"), 200, 1),
        ("flow_warp_bwd", lambda: ops.flow_warp_bwd(xb, flowb, None, dyb, True, True), 100, (1,)),
        ("flow_warp_bwd_dx_det", lambda: ops.flow_warp_bwd_dx_det(flowb, None, dyb), 20, 0),
        ("pwc_backwarp", lambda: ops.pwc_backwarp(x, flow), 200, 0),
    ]
    if ops.lab_available():
        todo = [("dcnv2_ws", il("ws"), 200, 0), ("dcnv2_x9", mdc("bf16x9"), 200, 0)]
    us, hashes = {}, {}
    for name, f, reps, pick in todo:
        for _ in range(20):
            out = f()
        torch.cuda.synchronize()
        outs = out if isinstance(out, (tuple, list)) else (out,)
        sel = [outs[i] for i in (pick if isinstance(pick, tuple) else (pick,))]      # (atomic dx: order-dependent bits, not hashed)
        hashes[name] = hashlib.sha1(b"".join(_canon(o).contiguous().view(torch.uint8).cpu().numpy().tobytes() for o in sel)).hexdigest()[:12]
        ts = []
        for _ in range(SAMPLES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
        us[name] = ts
    print(json.dumps({"lib": tag, "us": us, "hash": hashes}), flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "--merge":
        merge(sys.argv[2])
    else:
        main(sys.argv[1])
