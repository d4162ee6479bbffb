"""The Winograd convolution kernel (csrc/conv_wino6.hip, routes wino4 / wino5) held to its contract (tests/wino4_contract.py,
DESIGN.md 4b), pixel by pixel and slot by slot:

  a. |out - fp64| <= K u E + epilogue terms at EVERY pixel, on frames of mixed dynamic range, a large mean and white noise
  b. one-hot inputs: exact zero outside the Winograd tiles whose patch holds an impulse, also on a workgroup's second tile
  c. one inf / NaN: non-finite outputs cover the receptive field and stay inside the tiles whose patch holds the pixel
  d. per-tile channel sums and border pieces against fp64, slot by slot, no absolute constant
  e. the packed weights against exact integer arithmetic, bit for bit

Every launch is asserted (ops.profile) to be the Winograd kernel.  EAVSR_W4_CONTRACT_REPORT=<file> appends the measured figures
as JSON lines (profiles/r32_wino4_contract.json was collected that way)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import conv_routes
from tests import wino4_contract as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACT_CODE = {None: 0, "relu": 1, "lrelu": 2}


def _report(**row):
    path = os.environ.get("EAVSR_W4_CONTRACT_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _ops():
    from eavsr_amd import ops as _o
    _o.lib()      # fails loudly if the HIP extension is missing
    return _o


@pytest.fixture(scope="module")
def ops(cuda):
    return _ops()


class _Forced:
    """every launch, however small, goes to the Winograd kernels: mode winograd4, F(2x2,5x5) for the 5x5 heads, gates at zero"""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        o = self.ops
        self.was = (o.CONV_MODE, o.CONV5_MODE)
        o.set_conv_mode("winograd4")
        o.CONV5_MODE = "wino"
        self.thr = conv_routes.thresholds(o, wino_min=0, x6s_max=0)
        self.thr.__enter__()
        return o

    def __exit__(self, *exc):
        self.thr.__exit__(*exc)
        self.ops.CONV5_MODE = self.was[1]
        self.ops.set_conv_mode(self.was[0])


@pytest.fixture()
def forced(ops):
    with _Forced(ops) as o:
        yield o


def _g(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _split(a, sizes, axis):
    return np.split(a, np.cumsum(sizes)[:-1], axis=axis)


def launch(ops, dev, k, chans, couts, x, w, bias=None, act=None, residual=None, res_scale=None, shuffle=False, part=False, border=False,
           via="ops", ca=None):
    """one launch of the Winograd kernel -> dict(out, part, pieces) as numpy; asserts the kernel's name in the profile"""
    cin, cout = sum(chans), sum(couts)
    srcs = [_g(s, dev) for s in _split(x, chans, 1)]
    if ca is not None:      # the fused prologue is a lab instantiation: LabBuildRequired (a skip, tests/conftest.py) on the product library
        ops.require_lab("the channel-attention prologue inside the F(4x4,3x3) kernel")
        assert via == "ops" and len(chans) == 1
        ca = (_g(ca[0], dev), _g(ca[1], dev))
    if via == "cabi":
        assert k == 3 and not (res_scale is not None or shuffle or part or border)
        from eavsr_amd import _native as Nn
        wu = ops._packed_wino([_g(w, dev)], four=True)
        bg, rg = _g(bias, dev), _g(residual, dev)
        out = torch.empty(x.shape[0], cout, x.shape[2], x.shape[3], device=dev)
        d = Nn.ConvDesc()
        for i, s_ in enumerate(srcs):
            d.src[i] = s_.data_ptr(); d.src_c[i] = chans[i]
        d.n_src = len(chans); d.ksize = 3
        d.bias = 0 if bg is None else bg.data_ptr()
        d.residual = 0 if rg is None else rg.data_ptr()
        d.out = out.data_ptr()
        d.n, d.h, d.w, d.cin, d.cout = x.shape[0], x.shape[2], x.shape[3], cin, cout
        d.act, d.slope = ACT_CODE[act], float(W.SLOPE)
        with torch.cuda.device(dev):
            code = ops.lib().eavsr_conv3x3_wino4_f32(C.byref(d), C.c_void_p(wu.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0, ops.lib().eavsr_last_error()
        torch.cuda.synchronize(dev)
        return dict(out=out.cpu().numpy(), part=None, pieces=None)
    ws = [_g(a, dev) for a in _split(w, couts, 0)]
    bs = None if bias is None else [_g(a, dev) for a in _split(bias, couts, 0)]
    if len(couts) == 1:
        ws, bs = ws[0], None if bs is None else bs[0]
    with ops.profile() as prof:
        res = ops.conv2d(srcs, ws, bs, act=act, slope=float(W.SLOPE), residual=_g(residual, dev), res_scale=_g(res_scale, dev),
                         pixel_shuffle2=shuffle, chan_partial=part, border=border, ca=ca)
    assert list(prof.summary()) == [f"conv{k}x{k}_{cin}to{cout}_{'wino4' if k == 3 else 'wino'}{'' if ca is None else '_ca'}"], list(prof.summary())
    res = list(res) if isinstance(res, tuple) else [res]
    out = dict(out=res[0].cpu().numpy(), part=res[1].cpu().numpy() if part else None, pieces=None)
    if border:
        pc = res[-1]
        assert pc is not None, "border=True returned no pieces: the grouped kernel did not run"
        out["pieces"] = (pc.data.cpu().numpy(), pc.p_rows, pc.p_cols)
    return out


def launch_case(ops, dev, c, x, p, plain=False, ca_x=None):
    ca = (p["ca_scale"], ca_x) if c.ca else None
    if plain:
        return launch(ops, dev, c.k, c.chans, c.couts, x, p["w"], via=c.via, ca=ca)
    return launch(ops, dev, c.k, c.chans, c.couts, x, p["w"], p["bias"], c.act, p["residual"], p["res_scale"], c.shuffle, c.part, c.border, c.via, ca)


def local_bound_of_case(ops, dev, c, kinds=W.INPUT_KINDS, schedule=""):
    """test a for one case: the plain convolution (its err / (u E) is the figure K is about) and the case's own epilogue"""
    p = c.params()
    for kind in kinds:
        x, xx, cv, x32 = c.operands(kind, p)
        plain = launch_case(ops, dev, c, x, p, plain=True, ca_x=xx)["out"]
        ratio = W.ratio_uE(plain, cv.conv, cv.E)
        old = W.old_global(plain, cv.conv)
        emu = W.ratio_uE(W.emulate32(x32, p["w"]), cv.conv, cv.E)
        print(f"{c.id}/{kind}{schedule}: kernel err/(u E) {ratio:.4f} (emulation {emu:.4f}, K {W.K:.3f})  old metric {old:.2e}")
        _report(test="a", case=c.id, input=kind, schedule=schedule, kernel_ratio=ratio, emulation_ratio=emu, K=W.K, old_metric=old)
        W.check_local(plain, cv.epilogue(), what=f"{c.id}/{kind}/plain")
        r = cv.epilogue(**c.epilogue_args(p))
        got = launch_case(ops, dev, c, x, p, ca_x=xx)
        rel = W.check_local(got["out"], r, what=f"{c.id}/{kind}")
        print(f"{c.id}/{kind}{schedule}: with its epilogue err/bound {rel:.3f}")


def impulse_of_case(ops, dev, ic, schedule=""):
    x, w = ic.x(), ic.weight()
    if ic.ca:      # r one-hot, ca_x zero: the kernel's input is r * scale, zero wherever r is
        eff, err = W.fused_input(x, ic.ca_scale(), np.zeros_like(x))
        r = W.Conv(eff, w, err).epilogue()
        out = launch(ops, dev, ic.k, (ic.cin,), (ic.cout,), x, w, ca=(ic.ca_scale(), np.zeros_like(x)))["out"]
    else:
        r = W.Conv(x, w).epilogue()
        out = launch(ops, dev, ic.k, (ic.cin,), (ic.cout,), x, w, via=ic.via)["out"]
    zeros = W.check_impulse(out, x, r, ic.k, ic.id)
    print(f"{ic.id}{schedule}: {zeros} pixels exactly zero, {out.size - zeros} inside the tiles that saw an impulse")
    _report(test="b", case=ic.id, schedule=schedule, exact_zero_pixels=zeros, pixels=int(out.size))
    assert zeros > 0
    return zeros


# ------------------------------------------------------------------------------------------ a. the local bound
@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_every_pixel_within_its_own_bound(forced, cuda, c):
    local_bound_of_case(forced, cuda, c)


@pytest.mark.parametrize("act", [None, "relu", "lrelu"])
@pytest.mark.parametrize("residual", [False, True])
def test_local_bound_with_each_activation_and_residual(forced, cuda, act, residual):
    import dataclasses
    c = dataclasses.replace(W.case("h9_w68"), id=f"h9_w68_{act}_{int(residual)}", act=act, residual=residual, part=False, couts=(40,))
    local_bound_of_case(forced, cuda, c, kinds=("noise", "blocks_off"))


def test_duty_pair_schedule_with_even_chunks_in_a_child_process(ops, cuda):
    """EAVSR_W4_GRP is read once per process: ONE fresh child with EAVSR_W4_GRP=0 runs the cases marked `child` (even chunk counts,
    which the grouped kernel takes in this process) on the duty-pair kernel: local bound and impulse locality"""
    assert ops.lib().eavsr_wino4_schedule() == 1 or os.environ.get("EAVSR_W4_GRP") == "0"
    env = dict(os.environ, EAVSR_W4_GRP="0")
    code = "from tests import test_hip_wino4_contract as T; T.child_main()"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(res.stdout[-4000:])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "child: duty-pair schedule, all checks passed" in res.stdout


def child_main():
    ops = _ops()
    assert ops.lib().eavsr_wino4_schedule() == 0, "EAVSR_W4_GRP=0 did not select the duty-pair schedule"
    dev = torch.device("cuda:0")
    with _Forced(ops) as o:
        for c in W.CASES:
            if c.child:
                local_bound_of_case(o, dev, c, kinds=("noise", "blocks_off"), schedule="/duty")
        for ic in W.IMPULSES:
            if ic.child:
                impulse_of_case(o, dev, ic, schedule="/duty")
    print("child: duty-pair schedule, all checks passed")


# ------------------------------------------------------------------------------------------ b. impulse locality
@pytest.mark.parametrize("ic", W.IMPULSES, ids=lambda i: i.id)
def test_impulse_touches_only_the_tiles_whose_patch_holds_it(forced, cuda, ic):
    impulse_of_case(forced, cuda, ic)


# ------------------------------------------------------------------------------------------ c. non-finite containment
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "lab_ca"])
@pytest.mark.parametrize("val", [np.inf, np.nan], ids=["inf", "nan"])
def test_one_non_finite_pixel_costs_its_tiles_and_nothing_else(forced, cuda, val, fused):
    n, cin, h, wd = W.NONFINITE_SHAPE
    c = W._c("nf", n, h, wd, [cin], 8, ca=fused)
    p = c.params()
    if fused:
        forced.require_lab("the channel-attention prologue inside the F(4x4,3x3) kernel")
        p["ca_scale"] = (0.5 + 0.5 * p["ca_scale"]).astype(np.float32)      # (no zero scale: inf * 0 is a NaN all the same, but keep it plain)
    for act in (None, "lrelu"):
        for (y, x_) in W.NONFINITE_PIXELS:
            x = c.x("noise")
            x0 = x.copy()
            x0[1, 3, y, x_] = 0
            x[1, 3, y, x_] = val
            if fused:
                xx = c.x("noise", "_x")
                eff0, err0 = W.fused_input(x0, p["ca_scale"], xx)
                r0 = W.Conv(eff0, p["w"], err0).epilogue(bias=p["bias"], act=act)
                out = launch(forced, cuda, 3, c.chans, c.couts, x, p["w"], p["bias"], act, ca=(p["ca_scale"], xx))["out"]
            else:
                r0 = W.Conv(x0, p["w"]).epilogue(bias=p["bias"], act=act)
                out = launch(forced, cuda, 3, c.chans, c.couts, x, p["w"], p["bias"], act)["out"]
            cnt = W.check_nonfinite(out, (1, 3, y, x_), p["w"], r0, 3, f"{val} at ({y}, {x_}), act {act}")
            print(f"{val} at ({y}, {x_}) act {act}: {cnt} non-finite outputs")
            _report(test="c", value=str(val), fused=fused, pixel=[y, x_], act=act, non_finite_outputs=cnt)


# ------------------------------------------------------------------------------------------ d. channel sums and border pieces
@pytest.mark.parametrize("c", [c for c in W.CASES if c.part], ids=lambda c: c.id)
def test_channel_sums_and_border_pieces_slot_by_slot(forced, cuda, c):
    p = c.params()
    for kind in ("noise", "blocks_off"):
        x = c.x(kind)
        r = W.Conv(x, p["w"]).epilogue(**c.epilogue_args(p))
        got = launch_case(forced, cuda, c, x, p)
        rel = W.check_part(got["part"], r, c.k, f"{c.id}/{kind}")
        old = W.old_part_ok(got["part"], r.pre)
        rel_p = None
        if c.border:
            data, pr, pc = got["pieces"]
            rel_p = W.check_pieces(data, pr, pc, r, f"{c.id}/{kind}")
        print(f"{c.id}/{kind}: channel sums err/tol {rel:.3f}, pieces err/tol {rel_p}, old check ok {old}")
        _report(test="d", case=c.id, input=kind, part_ratio=rel, pieces_ratio=rel_p)


# ------------------------------------------------------------------------------------------ e. the packed weights
def _one_hot_weight(cout, cin, k):
    """every (co, ci) holds ONE tap, (co cin + ci) mod k^2, of value 1 + (co + 3 ci) mod 7: no position of U has two terms"""
    m = np.zeros((cout, cin, k, k), np.int64)
    co, ci = np.meshgrid(np.arange(cout), np.arange(cin), indexing="ij")
    tap = (co * cin + ci) % (k * k)
    m[co, ci, tap // k, tap % k] = 1 + (co + 3 * ci) % 7
    return m


@pytest.mark.parametrize("kind,k,couts,cin", [("f4", 3, (70,), 8), ("f4", 3, (64,), 12), ("f5", 5, (7, 40, 24), 8)],
                         ids=["f4_70x8", "f4_64x12", "f5_stacked_71x8"])
def test_packed_weights_equal_G_g_Gt_bit_for_bit(ops, cuda, kind, k, couts, cin):
    cout = sum(couts)
    rng = np.random.default_rng(k * 1000 + cout)
    for name, m in (("one-hot", _one_hot_weight(cout, cin, k)), ("dense", rng.integers(-8, 9, (cout, cin, k, k)))):
        w = (576 * m).astype(np.float32)
        ws = [_g(a, cuda) for a in _split(w, couts, 0)]
        packed = ops._packed_wino(ws, four=True) if kind == "f4" else ops._packed_wino(ws, kind="f5")
        flat = packed.cpu().numpy().ravel()
        assert flat.size == -(-cout // 64) * (cin // 4) * 36 * 4 * 64
        u = W.unpack_u(flat, cout, cin)
        W.check_pack(u[:cout], m, f"{kind} {name}")
        if name == "one-hot":
            assert np.array_equal(u[:cout], W.pack_exact(m).astype(np.float32))
        pad = u[cout:]
        assert not pad.any() and not np.signbit(pad).any(), "the padding for co >= cout is not exactly +0"
