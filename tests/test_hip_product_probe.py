"""The fp32-in, fp32-out kernels that contract on the bf16 matrix pipe keep every partial product they claim: probes in which
every output element is ONE product x * w plus exact zeros (tests/product_probe.py; the bounds and their derivation are there and in
DESIGN.md, "Product contract"), over a schedule of one-hot weights that visits every (tap, input channel) pair of the layer once,
and one dense check per route scaled by the element's own sum |x||w|.  The fp32-MFMA routes take the same probes at 2 u.

Every case prints its largest measured error relative to its bound before it asserts; EAVSR_PROBE_JSON=<file> collects them."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_routes as R
from tests import product_probe as P

pytestmark = pytest.mark.gpu

IMG, IMG16, IMG4 = (2, 9, 33), (2, 17, 40), (2, 9, 36)      # one 8 x 32 tile + a ragged row and column; 16-row tiles; the same with w % 4 == 0
IMG9 = (2, 33, 36)                                          # the nine-product 3x3 kernel: one 32-row tile + a ragged row and column, w % 4 == 0
THR = dict(wino_min=192, x6s_max=256)                       # as shipped: these launches are far below the Winograd gate
D = 8
RATIOS = {}


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    state = lambda: (_ops.WINO_MIN_TILES, _ops.X6S_MAX_TILES, _ops.CONV3_SMALL, _ops.CONV_MODE, _ops.CONV5_MODE, _ops.CONV7_MODE,
                     _ops.CONV3_H16, _ops._ROUTE_BATCH, _ops.DCN_MODE, _ops.DCN_IL_IMPL)
    before = state()
    yield _ops
    assert state() == before, "a test of this file left a threshold, a mode or a pinned route batch behind"
    if os.environ.get("EAVSR_PROBE_JSON"):
        with open(os.environ["EAVSR_PROBE_JSON"], "w") as f:
            json.dump({"unit": "largest measured error / its bound", "lab": _ops.lab_available(), "ratios": RATIOS}, f, indent=1, sort_keys=True)


def _note(key, err, bound):
    RATIOS[key] = max(RATIOS.get(key, 0.0), err / bound)
    print(f"{key}: largest error {err / P.U:.3f} u, bound {bound / P.U:.3f} u, ratio {err / bound:.3f}")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------ convolutions
# name -> (k, cin, cout, images, conv2d options, modes, family, nprod, native)
CONV_ROUTES = {
    "x6-7x7-8to32": (7, 8, 32, (IMG, IMG16), {}, {}, "x6", 6, False),
    "x6-7x7-32to64": (7, 32, 64, (IMG, IMG16), {}, {}, "x6", 6, False),
    "x6-7x7-16to2": (7, 16, 2, (IMG, IMG16), {}, {}, "x6", 6, False),
    "x6-5x5-64to120": (5, 64, 120, (IMG, IMG16), {}, {}, "x6", 6, False),
    "x6s-64to64": (3, 64, 64, (IMG,), {}, {}, "x6s", 6, False),
    "x6s-dgrad-64to64": (3, 64, 64, (IMG,), dict(dgrad=True), {}, "x6s", 6, False),
    "x9-64to64": (3, 64, 64, (IMG9,), {}, dict(conv="bf16x9"), "x9", 9, False),                       # lab build only
    "direct-3x3-64to64": (3, 64, 64, (IMG,), {}, dict(conv="direct"), "direct", 0, True),
    "direct-7x7-8to32": (7, 8, 32, (IMG,), {}, dict(conv="direct", conv7="direct"), "direct", 0, True),
    "direct-5x5-64to120": (5, 64, 120, (IMG,), {}, dict(conv="direct", conv5="direct"), "direct", 0, True),
}


def _conv_case(name, img):
    k, cin, cout, _, opts, modes, fam, nprod, native = CONV_ROUTES[name]
    rb = R.rows32_batches(img[1], img[2])[1] if fam == "x9" else None      # the nine-product kernel runs where the tiles have 32 rows
    return R._case(f"probe-{name}", "P", img, k, (cin,), cout, opts, modes, THR, route_batch=rb), fam, nprod, native


def _run_conv(ops, case, fam, x, wt, dev):
    """one ops.conv2d call of a probe weight under the case's modes; the kernel that ran is the family's"""
    route = case.route(lab=ops.lab_available())
    assert route.families == (fam,), (case.id, route.families)
    if case.o["dgrad"]:      # `weight` is the FORWARD weight: the call convolves with its transposed, flipped form
        wt = wt.flip(2, 3).transpose(0, 1).contiguous()
    with ops.profile() as prof:
        out = ops.conv2d(x, wt, None, dgrad=case.o["dgrad"])
    names = [rec[0] for rec in prof.records]
    assert names == list(route.kernels), f"{case.id}: launched {names}, predicted {list(route.kernels)}"
    return out


@pytest.mark.parametrize("cls", list(P.CLASSES))
@pytest.mark.parametrize("name", list(CONV_ROUTES))
def test_conv_single_products(ops, cuda, name, cls):
    k, cin, cout, images = CONV_ROUTES[name][:4]
    for img in images:
        case, fam, nprod, native = _conv_case(name, img)
        bound = P.one_product_bound(cls, nprod, native)
        n, h, w = img
        x, _ = P.probe_pair(cls, (n, cin, h, w), 1, seed=h)
        worst = 0.0
        with R.case_setup(ops, case), torch.no_grad():
            xd = _t(x, cuda)
            for j, (ci, tap) in enumerate(P.conv_schedule(k, cin, cout)):
                _, vals = P.probe_pair(cls, 1, cout, seed=1000 * h + j)
                out = _run_conv(ops, case, fam, xd, _t(P.onehot_weight(k, cin, ci, tap, vals), cuda), cuda).cpu().numpy()
                xs, ws, inside = P.onehot_expected(x, k, ci, tap, vals)
                assert P.zeros_ok(out, xs, ws, inside), f"{name} {cls} {img} tensor {j}: an output without a product is not zero"
                e = P.rel_error(out, xs, ws, inside)
                assert e <= bound, (f"{name} class {cls} image {img} weight tensor {j} (channels {ci.min()}..{ci.max()}, taps "
                                    f"{sorted(set(tap[tap >= 0]))}): {e / P.U:.2f} u > {bound / P.U:.2f} u")
                worst = max(worst, e)
        _note(f"{name}/{cls}", worst, bound)


def _dense_check(key, out, x, wt, k, nprod, native, dgrad=False):
    xd, wd = torch.from_numpy(x).double(), torch.from_numpy(wt).double()
    ref = F.conv2d(xd, wd, padding=k // 2).numpy()
    S = F.conv2d(xd.abs(), wd.abs(), padding=k // 2).numpy()
    bound = P.dense_bound(wt.shape[1] * k * k, nprod, native)
    ratio = float((np.abs(out.astype(np.float64) - ref) / S).max())
    _note(f"{key}/dense", ratio, bound)
    assert np.isfinite(out).all() and ratio <= bound, f"{key}: dense {ratio / P.U:.2f} u sum|x||w| > {bound / P.U:.2f} u"


@pytest.mark.parametrize("name", list(CONV_ROUTES))
def test_conv_dense(ops, cuda, name):
    k, cin, cout, images = CONV_ROUTES[name][:4]
    case, fam, nprod, native = _conv_case(name, images[-1])
    n, h, w = images[-1]
    x, wt = P.dense_inputs(n, cin, cout, h, w, k)
    with R.case_setup(ops, case), torch.no_grad():
        out = _run_conv(ops, case, fam, _t(x, cuda), _t(wt, cuda), cuda).cpu().numpy()
    _dense_check(name, out, x, wt, k, nprod, native)


def test_nine_products_hold_the_three_that_six_drop_conv(ops, cuda):
    """lab build: the nine-product 3x3 kernel against the six-product one on the same class-D probes (product_probe.nine_minus_six)"""
    n, h, w = IMG9
    x, _ = P.probe_pair("D", (n, 64, h, w), 1, seed=h)
    outs = {}
    for name in ("x9-64to64", "x6s-64to64"):
        case, fam, _, _ = _conv_case(name, IMG9)
        got, X, W = [], [], []
        with R.case_setup(ops, case), torch.no_grad():
            for j, (ci, tap) in enumerate(P.conv_schedule(3, 64, 64)):
                _, vals = P.probe_pair("D", 1, 64, seed=77 + j)
                out = _run_conv(ops, case, fam, _t(x, cuda), _t(P.onehot_weight(3, 64, ci, tap, vals), cuda), cuda).cpu().numpy()
                xs, ws, inside = P.onehot_expected(x, 3, ci, tap, vals)
                got.append(out[inside]), X.append(xs[inside]), W.append(ws[inside])
        outs[name] = np.concatenate(got)
    g, want = P.nine_minus_six(outs["x9-64to64"], outs["x6s-64to64"], np.concatenate(X), np.concatenate(W))
    _note("x9-64to64/nine-minus-six (fraction of the dropped products still missing)", max(want - g, 0.0), want)
    assert g >= 0.75 * want, (g, want)


# ------------------------------------------------------------------------------------------ DCNv2
def _heads_tensor(n, h, w, masks, logits):
    """(n, 15 D, h, w): identity transforms, zero translations (offsets exactly zero), the masks as they are or as logits of 1"""
    hd = np.zeros((n, 15 * D, h, w), np.float32)
    for d in range(D):
        hd[:, 4 * d] = hd[:, 4 * d + 3] = 1.0
    hd[:, 6 * D:] = 40.0 if logits else masks.reshape(n, 9 * D, h, w)      # sigmoid(40) = 1 / (1 + 2^-57.7) = 1.0 in fp32
    return hd


DCN_VARIANTS = ("zero", "shift", "mask", "heads", "heads2", "heads2-mask")
# name -> (mode switches, nprod, native, variants)
DCN_ROUTES = {
    **{f"{impl}-{np_}": (dict(dcn_il_impl=impl), np_, False, ("zero", "shift", "mask", "heads") + (("heads2", "heads2-mask") if impl == "il2" else ()))
       for impl in ("il", "il2") for np_ in (6, 9)},
    "native": (dict(dcn="native"), 0, True, ("zero", "shift", "mask")),
    "ws-6": (dict(dcn_il_impl="ws"), 6, False, ("zero", "shift", "mask", "heads")),                 # lab build only
    "ws-9": (dict(dcn_il_impl="ws"), 9, False, ("zero", "shift", "mask", "heads")),                 # lab build only
    "bf16x9": (dict(dcn="bf16x9"), 9, False, ("zero", "shift", "mask")),                             # lab build only
}


def _dcn_operands(variant, cls, img, seed):
    """x, integer offsets (n, D, 9, 2, h, w) or None, masks (n, D, 9, h, w) or None"""
    n, h, w = img
    x, _ = P.probe_pair(cls, (n, 64, h, w), 1, seed=seed)
    rng = np.random.default_rng(seed)
    offs = rng.integers(-2, 3, (n, D, 9, 2, h, w)) if variant == "shift" else None      # inside the LDS window (6 up, 8 left)
    masks = P.probe(24, (n, D, 9, h, w), rng) if variant.endswith("mask") else None
    return x, offs, masks


def _run_dcn(ops, route, variant, x, offs, masks, wt, dev):
    modes, nprod, native, _ = DCN_ROUTES[route]
    n, _, h, w = x.shape
    off = np.zeros((n, 18 * D, h, w), np.float32) if offs is None else offs.reshape(n, 18 * D, h, w).astype(np.float32)
    msk = np.ones((n, 9 * D, h, w), np.float32) if masks is None else masks.reshape(n, 9 * D, h, w)
    with ops.modes(**modes), ops.profile() as prof, torch.no_grad():
        if "dcn" in modes:
            out = ops.modulated_deform_conv2d(_t(x, dev), _t(off, dev), _t(msk, dev), wt, None, 1, 1, 1, 1, D)
            want = ["dcnv2" if native else "dcnv2_x9"]
        elif variant.startswith("heads"):
            two = variant.startswith("heads2")
            hd = _heads_tensor(n, h, w, msk, logits=not two)
            out = ops.dcnv2_il(ops.to_il8(_t(x, dev)), _t(hd, dev), None, wt, None, D, nprod=nprod, heads=True, mask_activated=two)
            want = ["nchw_to_il8", "dcnv2_il_heads"]
        else:
            out = ops.dcnv2_il(ops.to_il8(_t(x, dev)), _t(off, dev), _t(msk, dev), wt, None, D, nprod=nprod)
            want = ["nchw_to_il8", "dcnv2_il"]
        assert ops.DCN_IL_IMPL == modes.get("dcn_il_impl", ops.DCN_IL_IMPL) and ops.DCN_MODE == modes.get("dcn", ops.DCN_MODE)
    assert [rec[0] for rec in prof.records] == want, (route, variant, [rec[0] for rec in prof.records])
    return out.cpu().numpy()


def _dcn_expected(x, offs, masks, ci, tap, vals):
    g = ci // (64 // D)
    co = np.arange(len(ci))
    dy = None if offs is None else offs[:, g, tap, 0]
    dx = None if offs is None else offs[:, g, tap, 1]
    xs, ws, inside = P.onehot_expected(x, 3, ci, tap, vals, dy, dx)
    if masks is not None:
        xs = xs.astype(np.float64) * masks[:, g, tap]
    return xs, ws, inside


@pytest.mark.parametrize("route", list(DCN_ROUTES))
def test_dcn_single_products(ops, cuda, route):
    modes, nprod, native, variants = DCN_ROUTES[route]
    img = IMG4 if route == "bf16x9" else IMG
    with ops.modes(**modes):      # a lab schedule on the product library: LabBuildRequired = a skip, before anything runs
        pass
    sched = P.conv_schedule(3, 64, 64)
    for variant in variants:
        masked = variant.endswith("mask")
        for cls in ("D",) if masked else tuple(P.CLASSES):      # a probe mask makes every sample a 24-bit number
            bound = P.one_product_bound(cls, nprod, native, mask=masked)
            x, offs, masks = _dcn_operands(variant, cls, img, seed=5)
            worst = 0.0
            for j, (ci, tap) in enumerate(sched):
                _, vals = P.probe_pair(cls, 1, 64, seed=300 + j)
                out = _run_dcn(ops, route, variant, x, offs, masks, _t(P.onehot_weight(3, 64, ci, tap, vals), cuda), cuda)
                xs, ws, inside = _dcn_expected(x, offs, masks, ci, tap, vals)
                assert P.zeros_ok(out, xs, ws, inside), f"dcn {route} {variant} {cls} tensor {j}: an output without a product is not zero"
                e = P.rel_error(out, xs, ws, inside)
                assert e <= bound, f"dcn {route} {variant} class {cls} weight tensor {j}: {e / P.U:.2f} u > {bound / P.U:.2f} u"
                worst = max(worst, e)
            _note(f"dcn-{route}/{variant}/{cls}", worst, bound)


@pytest.mark.parametrize("route", list(DCN_ROUTES))
def test_dcn_dense(ops, cuda, route):
    modes, nprod, native, _ = DCN_ROUTES[route]
    n, h, w = img = IMG4 if route == "bf16x9" else IMG
    with ops.modes(**modes):
        pass
    x, wt = P.dense_inputs(n, 64, 64, h, w, 3)
    out = _run_dcn(ops, route, "zero", x, None, None, _t(wt, cuda), cuda)
    _dense_check(f"dcn-{route}", out, x, wt, 3, nprod, native)


@pytest.mark.parametrize("impl", ["il", "il2", "ws"])
def test_nine_products_hold_the_three_that_six_drop_dcn(ops, cuda, impl):
    """nprod = 9 against nprod = 6 of the same schedule on the same class-D probes: the difference is the three dropped products
    (product_probe.nine_minus_six; a nine that ran six, or lost mid*lo or lo*mid, gives at most half of them)"""
    with ops.modes(dcn_il_impl=impl):
        pass
    x, _, _ = _dcn_operands("zero", "D", IMG, seed=9)
    outs, X, W = {6: [], 9: []}, [], []
    for j, (ci, tap) in enumerate(P.conv_schedule(3, 64, 64)):
        _, vals = P.probe_pair("D", 1, 64, seed=500 + j)
        xs, ws, inside = _dcn_expected(x, None, None, ci, tap, vals)
        wd = _t(P.onehot_weight(3, 64, ci, tap, vals), cuda)
        for np_ in (6, 9):
            outs[np_].append(_run_dcn(ops, f"{impl}-{np_}", "zero", x, None, None, wd, cuda)[inside])
        X.append(xs[inside]), W.append(ws[inside])
    g, want = P.nine_minus_six(np.concatenate(outs[9]), np.concatenate(outs[6]), np.concatenate(X), np.concatenate(W))
    _note(f"dcn-{impl}/nine-minus-six (fraction of the dropped products still missing)", max(want - g, 0.0), want)
    assert g >= 0.75 * want, (impl, g, want)


# ------------------------------------------------------------------------------------------ weight gradient, split path
def _wgrad(ops, multi, dy, x, dev):
    cout, cin = dy.shape[1], x.shape[1]
    with ops.profile() as prof, torch.no_grad():
        if multi:      # two uses of the weight: the second use's dY is zero, its sources are the same
            out = torch.empty(cout, cin, 3, 3, device=dev)
            ops.conv_wgrad_multi([_t(dy, dev), torch.zeros_like(_t(dy, dev))], [[_t(x, dev)], [_t(x, dev)]], 3, out=out)
        else:
            out = ops.conv_wgrad(_t(dy, dev), [_t(x, dev)], 3)
    assert [rec[0] for rec in prof.records] == ["conv_wgrad3x3"], [rec[0] for rec in prof.records]
    return out.cpu().numpy()


@pytest.mark.parametrize("multi", [False, True], ids=["conv_wgrad", "conv_wgrad_multi"])
@pytest.mark.parametrize("cls", list(P.CLASSES))
def test_wgrad_single_products(ops, cuda, cls, multi):
    """dY[co] is non-zero at one pixel p(co): dW[co, ci, t] = dY[co, p] x[ci, p + t]; p(co) visits every position of an 8 x 32 tile
    (two of the kernel's 4 x 32 tiles) and the first row and column of the ragged tiles behind it.  w % 4 == 0 and aligned tensors:
    the bf16-split kernel (any other launch runs the fp32 kernel)."""
    if ops.lib().eavsr_wgrad3_mode() != 1:
        pytest.skip("EAVSR_WGRAD3=fp32: the bf16x6 3x3 weight-gradient kernel is switched off in this process")
    n, h, w = IMG4
    x, _ = P.probe_pair(cls, (n, 64, h, w), 1, seed=21)
    bound, worst = P.one_product_bound(cls, 6), 0.0
    for j, where in enumerate(P.wgrad_schedule(h, w, 64)):
        _, vals = P.probe_pair(cls, 1, 64, seed=600 + j)
        out = _wgrad(ops, multi, P.wgrad_onehot(n, h, w, where, vals), x, cuda)
        xs, ws, inside = P.wgrad_expected(x, where, vals)
        assert P.zeros_ok(out, xs, ws, inside), f"wgrad {cls} tensor {j}: a gradient without a product is not zero"
        e = P.rel_error(out, xs, ws, inside)
        assert e <= bound, f"wgrad class {cls} dY tensor {j} (positions {where[0, 1:]}..): {e / P.U:.2f} u > {bound / P.U:.2f} u"
        worst = max(worst, e)
    _note(f"wgrad{'-multi' if multi else ''}/{cls}", worst, bound)


def test_wgrad_dense(ops, cuda):
    if ops.lib().eavsr_wgrad3_mode() != 1:
        pytest.skip("EAVSR_WGRAD3=fp32: the bf16x6 3x3 weight-gradient kernel is switched off in this process")
    n, h, w = IMG4
    rng = np.random.default_rng(31)
    sx, sy = np.linspace(-20, 20, 64).round(), np.linspace(-12, 12, 64).round()
    rng.shuffle(sx), rng.shuffle(sy)
    x = (rng.standard_normal((n, 64, h, w)) * 2.0 ** sx[None, :, None, None]).astype(np.float32)
    dy = (rng.standard_normal((n, 64, h, w)) * 2.0 ** sy[None, :, None, None]).astype(np.float32)
    out = _wgrad(ops, False, dy, x, cuda)
    cols = F.unfold(torch.from_numpy(x).double(), 3, padding=1).view(n, 64, 9, h * w)
    dyd = torch.from_numpy(dy).double().view(n, 64, -1)
    ref = torch.einsum("nop,nctp->oct", dyd, cols).view(64, 64, 3, 3).numpy()
    S = torch.einsum("nop,nctp->oct", dyd.abs(), cols.abs()).view(64, 64, 3, 3).numpy()
    bound = P.dense_bound(n * h * w, 6)      # the reduction runs over the pixels of every image
    ratio = float((np.abs(out.astype(np.float64) - ref) / S).max())
    _note("wgrad/dense", ratio, bound)
    assert np.isfinite(out).all() and ratio <= bound
