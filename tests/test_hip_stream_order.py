"""The stream-order contract of eavsr_amd.ops (graph.py: every kernel is launched on torch.cuda.current_stream()), op by op, over
the table of tests/stream_cases.py, and of the derived-weight caches (eavsr_amd/weight_cache.py).

(a) An op stays behind its stream.  The buffers hold the decoy values B; a fresh side stream sleeps, copies A into the buffers and
    makes the call.  A launch that left the stream (stream 0, a forgotten second kernel, a table uploaded elsewhere) runs while
    the side stream still sleeps and computes on B: the result then differs from want_A, which was computed eagerly on the default
    stream -- and checked against the op's host restatement where tests/*_ref.py has one.  The side stream must still be busy when
    the call returns: the call did not wait for the device, and the comparison is conclusive.
(b) An op replays: one call captured in a torch.cuda.graph (a single linear branch), replayed on A and then on B.
(c) A derived weight is ordered after its derivation on any stream: stream A packs behind a sleep, stream B hits the cache at once.

The stall of (a) is 20 x the host time of the row's warmed-up eager call (the margin is over host jitter on a shared machine),
at least 20 ms, in ticks of torch's spin kernel calibrated once per module as StreamedForward.__init__ calibrates them; a row
that would need more than 500 ms has a shape that is too large.  Outputs are compared bit for bit: every op of the table is
documented as fixed-order.  Both value sets are valid inputs: no kernel ever runs on anything else."""
import math
import time

import pytest
import torch

from tests import conv_routes as R
from tests import stream_cases as S

pytestmark = pytest.mark.gpu

SEED = 20
MIN_STALL_MS, MAX_STALL_MS, MARGIN = 20.0, 500.0, 20.0
_READY = {}
# Part (c): the caches each parameter must fill (it may fill more: a transposed weight is packed as well).  Every test asserts its
# own line, and test_the_parameters_of_part_c_name_every_weight_cache asserts that the lines together name every cache.
FILLS = {
    "stream_smallco": ["ops._smallco_pack_cache"], "stream_x6s": ["ops._conv7_pack_cache"],
    "stream_wino4": ["ops.pack_cache", "ops._wino_pack_cache"], "stream_wino4_2src": ["ops._wino_pack_cache"],
    "stream_wino5": ["ops._wino_pack_cache"], "stream_x6_5x5": ["ops._conv7_pack_cache"], "stream_x6_7x7": ["ops._conv7_pack_cache"],
    "stream_direct_2src": ["ops.pack_cache"], "stream_direct_1x1": ["ops.pack_cache"], "stream_direct_ragged": ["ops.pack_cache"],
    "stream_heads": ["ops._bias_cache", "ops._wcat_cache", "ops._smallco_pack_cache"], "stream_x6s_dgrad": ["ops._conv7_pack_cache"],
    "stream_direct_dgrad": ["ops._dgrad_w_cache"], "stream_x6s_bf16": ["ops._bf16_pack_cache"], "stream_h16g": ["ops._h16g_pack_cache"],
    "stream_h16x1": ["ops._h16x1_pack_cache"], "lpips_conv": ["ops._lpips_pack_cache"], "pwc_conv3x3": ["ops._pwc_pack_cache"],
    "dcnv2_il-il": ["ops._x9_pack_cache"], "dcnv2_il-il2": ["ops._il2_pack_cache"], "dcnv2_il16": ["ops._il16_pack_cache"],
    "conv3x3_c64_h16": ["ops._h16_pack_cache"], "conv3x3_c64_h16_act-shuffle": ["ops._h16_ps_cache"],
    "conv3x3_c64to3_h16": ["ops._h16_last_cache"], "conv5x5_c64_h16": ["ops._wcat_cache", "ops._h16_pack5_cache"],
    "autograd-conv-dgrad": ["autograd._dgrad_cache"], "autograd-dcn-columns": ["autograd._dcn_wt_cache"],
}


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def tick(cuda):
    """ticks of torch's spin kernel per millisecond on this device"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(1_000_000)
    torch.cuda.synchronize(cuda)
    e0.record()
    torch.cuda._sleep(20_000_000)
    e1.record()
    torch.cuda.synchronize(cuda)
    return 20_000_000 / max(1e-3, e0.elapsed_time(e1))


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    yield
    _READY.clear()
    torch.cuda.empty_cache()


def _bits(t):
    t = t.detach().contiguous()
    if t.is_floating_point():
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def _same_bits(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _host(row, outs):
    """the outputs on the host (None results dropped), cut to what the op defines"""
    got = [o.detach().cpu().clone() for o in outs if o is not None]
    return row.trim(got) if row.trim is not None else got


def _load(case, values):
    for buf, v in zip(case.bufs, values):      # (constants ride behind the buffers and have no values)
        buf.copy_(v)


def _filler(out, wants):
    """a value no result holds, for an `out=` buffer: NaN for floats (the inputs are finite), for integers the first value that
    occurs in none of the results of that dtype.  A uint8 image of more than a few thousand random bytes (rgb8, png_filter,
    resize_cubic_u8, png_unfilter) holds every value: there the rarest one is taken, which differs from what belongs there in
    all but about 1 / 256 of the positions -- an output left unwritten still differs from both results."""
    if out.is_floating_point():
        return math.nan
    held = torch.cat([w.flatten() for ws in wants for w in ws if w.dtype == out.dtype] or [torch.zeros(0, dtype=out.dtype)])
    counts = torch.bincount(held.long().clamp(0, 255), minlength=256)
    return int(counts.argmin())


def _prefill(p):
    for out, v in zip(p["case"].outs, p["fill"]):
        out.fill_(v)


def _prepared(ops, row, cuda):
    """the row's case, its value sets on the device and the eager results want_A / want_B on the default stream: computed once"""
    if row.name in _READY:
        return _READY[row.name]
    case = row.make(SEED, cuda)
    p = {"case": case, "A": [a.to(cuda) for a in case.A], "B": [b.to(cuda) for b in case.B], "fill": [math.nan if o.is_floating_point() else 0xA5 for o in case.outs]}
    for key in ("A", "B"):
        _load(case, p[key])
        _prefill(p)
        outs = row.call(ops, case.bufs, case.outs)
        torch.cuda.synchronize(cuda)
        p["want_" + key] = _host(row, outs)
    p["fill"] = [_filler(o, (p["want_A"], p["want_B"])) for o in case.outs]
    if case.A:
        assert not _same_bits(p["want_A"], p["want_B"]), f"{row.name}: the decoy B gives the result of A: the row shows nothing"
    if row.ref is not None:      # the thing compared with is known good
        want = [w if isinstance(w, tuple) else S._t(w) for w in row.ref(*case.A)]
        want = row.trim(want) if row.trim is not None else want
        assert len(want) == len(p["want_A"]), (row.name, len(want), len(p["want_A"]))
        for g, w in zip(p["want_A"], want):
            if row.same is not None:
                row.same(g, w)
            else:
                assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), f"{row.name}: differs from its host restatement"
    if case.expect is not None:
        assert _same_bits(p["want_A"], case.expect), f"{row.name}: differs from what its builder started from"
    if row.verify is not None:
        row.verify(p["want_A"], case.A)
    _READY[row.name] = p
    return p


def _verdict(row, got, p, what):
    if _same_bits(got, p["want_A"]):
        return
    if p["case"].A and _same_bits(got, p["want_B"]):
        raise AssertionError(f"{row.name}: {what}: the result is that of the decoy values B: ran ahead of its stream")
    bad = [i for i, (g, w) in enumerate(zip(got, p["want_A"])) if not _same_bits([g], [w])]
    raise AssertionError(f"{row.name}: {what}: outputs {bad} equal neither want_A nor want_B")


@pytest.mark.parametrize("row", S.ROWS, ids=lambda r: r.name)
def test_an_op_stays_behind_its_stream(ops, cuda, tick, row):
    p = _prepared(ops, row, cuda)
    case = p["case"]
    # the host time of the warmed-up eager call, taken without synchronising
    _load(case, p["B"])
    torch.cuda.synchronize(cuda)
    t0 = time.perf_counter()
    row.call(ops, case.bufs, case.outs)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize(cuda)
    stall_ms = max(MIN_STALL_MS, MARGIN * host_ms)
    print(f"{row.name}: eager call {host_ms:.3f} ms of host time, stall {stall_ms:.1f} ms")
    assert stall_ms <= MAX_STALL_MS, f"{row.name}: a stall of {stall_ms:.0f} ms: the row's shape is too large"
    _load(case, p["B"])
    _prefill(p)
    torch.cuda.synchronize(cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(stall_ms * tick))
        _load(case, p["A"])
        outs = row.call(ops, case.bufs, case.outs)
        still_stalled = not side.query()
    side.synchronize()
    _verdict(row, _host(row, outs), p, "behind a sleeping side stream")
    if row.name not in S.HOST_SYNC:
        assert still_stalled, (f"{row.name}: the side stream had drained when the call returned: the call waited for the device "
                               f"(or took longer than the {stall_ms:.0f} ms stall) and the comparison shows nothing")


@pytest.mark.parametrize("row", [r for r in S.ROWS if r.name not in S.HOST_SYNC and r.name not in S.NOT_CAPTURED], ids=lambda r: r.name)
def test_an_op_replays(ops, cuda, row):
    p = _prepared(ops, row, cuda)
    case = p["case"]
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        _load(case, p["A"])
        row.call(ops, case.bufs, case.outs)
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = row.call(ops, case.bufs, case.outs)
    for key in ("A", "B"):
        _load(case, p[key])
        _prefill(p)
        graph.replay()
        torch.cuda.synchronize(cuda)
        got = _host(row, outs)
        assert _same_bits(got, p["want_" + key]), f"{row.name}: the replay on {key} does not give the eager result on {key}"
    del graph


# --------------------------------------------------------------------------------------------------------- (c) the weight caches
def _cache_names():
    from eavsr_amd import autograd, ops as _ops, weight_cache
    names = {}
    for mod in (_ops, autograd):
        for k, v in vars(mod).items():
            if isinstance(v, weight_cache.WeightCache):
                names[id(v)] = f"{mod.__name__.rsplit('.', 1)[-1]}.{k}"
    return names


def _device_bytes(value):
    vs = value if isinstance(value, (tuple, list)) else (value,)
    return [v.numel() * v.element_size() for v in vs if isinstance(v, torch.Tensor) and v.is_cuda]


def _conv_case(name, shape, k, chans, couts, opts=None, modes=None):
    return R._case("stream_" + name, "stream", shape, k, chans, couts, opts, modes)


def _conv_cases():
    """a conv2d per route, one launch each (conv_routes.ROUTE_SHAPES, thresholds LOWERED), then the forms only an option or a mode
    reaches: several weights in one launch (bias and weight concatenation), the input-gradient forms, bf16 training, 16-bit modes"""
    # (smallco_w18, the classic small-cout kernel, reads one weight as it is: it derives nothing and fills no cache)
    out = [_conv_case(n, *v[:4], None, v[4]) for n, v in R.ROUTE_SHAPES.items() if n != "smallco_w18"]
    out += [_conv_case("heads", (2, 12, 16), 3, (64,), (4, 2), None, None),
            _conv_case("x6s_dgrad", (1, 20, 28), 3, (64,), 64, dict(dgrad=True), None),
            _conv_case("direct_dgrad", (1, 13, 37), 3, (64, 64), 64, dict(dgrad=True), None),
            _conv_case("x6s_bf16", (1, 20, 28), 3, (64,), 64, R.OPTION_SETS["bf16"], None),
            _conv_case("h16g", (2, 13, 68), 3, (64,), 64, None, dict(h16="bf16", grad=False)),
            _conv_case("h16x1", (1, 10, 19), 7, (8,), 32, None, dict(h16="fp16", grad=False))]
    return out


def _weights_of(t, dev):
    return [w.to(dev) for w in t["weights"]], None if t["biases"] is None else [b.to(dev) for b in t["biases"]]


def _two_streams(cuda, tick, caches, run, fresh):
    """`run(weights)` with one fresh set of weights on stream A behind a sleep and at once on stream B, which has not waited
    for A -> (out_a, out_b, names of the caches that grew, whether A was still asleep when B's call returned).  A pilot call
    with weights of its own tells which caches the call fills and how large the derived forms are: blocks of those sizes, full
    of NaN, are allocated and freed on stream A first, so that the allocator is likely to hand them to the packer."""
    names = _cache_names()
    before = {id(c): set(c.snapshot()) for c in caches}
    pilot = fresh()      # (held: an entry goes when its weight dies)
    run(pilot)
    torch.cuda.synchronize(cuda)
    sizes = [b for c in caches for k, e in c.snapshot().items() if k not in before[id(c)] for b in _device_bytes(e[1])]
    assert sizes, "the pilot call derived nothing: no cache is exercised"
    weights = fresh()
    torch.cuda.synchronize(cuda)
    lens = {id(c): len(c) for c in caches}
    a, b = torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)
    cur = torch.cuda.current_stream(cuda)
    a.wait_stream(cur)
    b.wait_stream(cur)
    with torch.cuda.stream(a):
        junk = [torch.full((max(n // 4, 1),), math.nan, device=cuda) for n in sizes]
        del junk
        # 60 ms: three times part (a)'s floor, for the two calls made meanwhile (0.1 ms of host time each on this library);
        # not derived per call as in (a), because `asleep` below is asserted: a sleep that was too short fails, it cannot pass
        torch.cuda._sleep(int(60.0 * tick))
        out_a = run(weights)
    grew = [names.get(id(c), "?") for c in caches if len(c) > lens[id(c)]]
    with torch.cuda.stream(b):
        out_b = run(weights)
        asleep = not a.query()
    a.synchronize()
    b.synchronize()
    return out_a, out_b, grew, asleep


@pytest.mark.parametrize("case", _conv_cases(), ids=lambda c: c.id)
def test_a_conv_weight_form_is_ordered_after_its_derivation(ops, cuda, tick, case):
    from tests.test_hip_conv_routes import BF16_BOUND, CONV_TOL
    from eavsr_amd.weight_cache import WEIGHT_CACHES
    route = case.route(lab=ops.lab_available())
    assert not route.raises, (case.id, route.why)
    fam, o, t = route.families[0], case.o, R.inputs_of(case)
    ref = R.reference_of(case, "bf16" if fam == "bf16s" else case.m["h16"] if fam in ("h16g", "h16x1") else None)
    srcs = [s.to(cuda) for s in t["srcs"]]
    residual = None if t["residual"] is None else t["residual"].to(cuda)
    torch.cuda.synchronize(cuda)

    def run(wb):
        ws, bs = wb
        one = len(ws) == 1
        r = ops.conv2d(srcs if len(srcs) > 1 else srcs[0], ws[0] if one else ws, None if bs is None else bs[0] if one else bs, act=o["act"],
                       slope=R.SLOPE, residual=residual, dgrad=o["dgrad"], precision=o["precision"])
        return r[0] if isinstance(r, tuple) else r

    with R.case_setup(ops, case):
        out_a, out_b, grew, asleep = _two_streams(cuda, tick, list(WEIGHT_CACHES), run, lambda: _weights_of(t, cuda))
    print(f"{case.id}: {fam}: filled {grew}")
    assert set(FILLS[case.id]) <= set(grew), f"{case.id}: the call with fresh weights filled {grew}, not {FILLS[case.id]}"
    assert asleep, f"{case.id}: stream A had drained when stream B's call returned: nothing was shown"
    bound = BF16_BOUND * ref["S"].max().item() if fam == "bf16s" else CONV_TOL[fam] * max(1.0, ref["out"].abs().max().item())
    for which, out in (("the deriving stream", out_a), ("the stream that hit the cache", out_b)):
        e = (out.detach().cpu().double() - ref["out"]).abs().max().item()
        print(f"{case.id}: {which}: max|out - ref64| {e:.3e} bound {bound:.3e}")
        assert e <= bound, f"{case.id}: on {which}: {e:.3e} > {bound:.3e} (nan: the cached form was read before it was derived)"


def test_the_lpips_weight_form_is_ordered_after_its_derivation(ops, cuda, tick):
    """lpips_conv on AlexNet's features.3 weight against F.conv2d in float64, with test_hip_lpips.py's bound for a layer's
    features: max|gpu - ref64| <= max(8 max|ref32 - ref64|, 2^-20 max|ref64|)"""
    from tests import lpips_ref
    from tests.golden import cases as G
    import torch.nn.functional as F
    sd = lpips_ref.synthetic_weights(0)
    w, bias = sd["net.slice2.3.weight"], sd["net.slice2.3.bias"]
    x = G.rand(5, 2, 64, 5, 7)
    ref = F.relu(F.conv2d(x.double(), w.double(), bias.double(), padding=2))
    bound = max(8 * (F.relu(F.conv2d(x, w, bias, padding=2)).double() - ref).abs().max().item(), 2.0 ** -20 * ref.abs().max().item())
    xd = x.to(cuda)
    torch.cuda.synchronize(cuda)
    out_a, out_b, grew, asleep = _two_streams(cuda, tick, [ops._lpips_pack_cache], lambda wb: ops.lpips_conv(xd, *wb),
                                              lambda: (w.to(cuda), bias.to(cuda)))
    assert grew == FILLS["lpips_conv"] and asleep
    for out in (out_a, out_b):
        e = (out.cpu().double() - ref).abs().max().item()
        print(f"lpips_conv: max|out - ref64| {e:.3e} bound {bound:.3e}")
        assert e <= bound


def test_the_pwc_weight_form_is_ordered_after_its_derivation(ops, cuda, tick):
    """pwc_conv3x3 against F.conv2d in float64, with test_hip_pwc.py's bound for that op (2e-5 of the output scale)"""
    from tests.golden import cases as G
    import torch.nn.functional as F
    x, w, bias = G.randn(6, 2, 6, 19, 37), G.randn(71, 8, 6, 3, 3, scale=0.1), G.randn(72, 8, scale=0.1)
    ref = F.leaky_relu(F.conv2d(x.double(), w.double(), bias.double(), padding=1), 0.1)
    xd = x.to(cuda)
    torch.cuda.synchronize(cuda)
    out_a, out_b, grew, asleep = _two_streams(cuda, tick, [ops._pwc_pack_cache], lambda wb: ops.pwc_conv3x3(xd, *wb),
                                              lambda: (w.to(cuda), bias.to(cuda)))
    assert grew == FILLS["pwc_conv3x3"] and asleep
    for out in (out_a, out_b):
        e = (out.cpu().double() - ref).abs().max().item()
        print(f"pwc_conv3x3: max|out - ref64| {e:.3e}")
        assert e <= 2e-5 * max(1.0, ref.abs().max().item())


# the rest of the caches: each call against the SAME call made eagerly on the default stream with weights of its own (the pilot
# of _two_streams does exactly that), within the bound the op's own test puts on it against its reference
def _il8_inputs(ops, cuda, c=64, cout=64, dg=8, n=2, h=13, w=37):
    from tests.test_hip_h16 import _dcn_inputs16
    x, off, mask, wt, b = _dcn_inputs16(n, c, h, w, cout, dg, 2.0)
    return x.to(cuda), off.to(cuda), mask.to(cuda), wt, b, dg


def _dcn_il(impl):
    def build(ops, cuda):
        x, off, mask, wt, b, dg = _il8_inputs(ops, cuda)
        xi = ops.to_il8(x)

        def run(wb):
            with ops.modes(dcn_il_impl=impl):
                return ops.dcnv2_il(xi, off, mask, wb[0], wb[1], dg)
        return run, lambda: (wt.to(cuda), b.to(cuda)), 2e-5, 0.0      # fp32 accumulation of exact products, as the fp32 convolutions
    return build


def _dcn_il16(ops, cuda):
    x, off, mask, wt, b, dg = _il8_inputs(ops, cuda)
    xi = ops.to_il8_h16(x, "bf16")
    return (lambda wb: ops.dcnv2_il16(xi, off, mask, wb[0], wb[1], dg)), (lambda: (wt.to(cuda), b.to(cuda))), 8e-3, 0.0


def _nhwc16(cuda, seed, n=2, h=19, w=37):
    from tests.golden import cases as G
    return G.randn(seed, n, 64, h, w).to(torch.bfloat16).permute(0, 2, 3, 1).contiguous().to(cuda)


EPS_BF16 = 2.0 ** -8      # tests/test_hip_h16.py EPS: one rounding of the fp32 result to bf16


def _h16_conv(cout, scale_seed, **kw):
    def build(ops, cuda):
        from tests.golden import cases as G
        xh, wt, b = _nhwc16(cuda, 1), G.randn(scale_seed, cout, 64, 3, 3, scale=1.0 / 24.0), G.randn(scale_seed + 1, cout, scale=0.1)
        if cout == 3:
            run = lambda wb: ops.conv3x3_c64to3_h16(xh, wb[0], wb[1])
            return run, lambda: (wt.to(cuda), b.to(cuda)), 2e-5, 0.0
        fn = ops.conv3x3_c64_h16_act if "act" in kw else ops.conv3x3_c64_h16
        return (lambda wb: fn(xh, wb[0], wb[1], **kw).float()), (lambda: (wt.to(cuda), b.to(cuda))), EPS_BF16 * 1.01, 1e-5
    return build


def _h16_conv5(ops, cuda):
    from tests.golden import cases as G
    couts = (32, 16, 72)
    xh = _nhwc16(cuda, 1)
    ws = [G.randn(2 + i, c, 64, 5, 5, scale=1.0 / 40.0) for i, c in enumerate(couts)]
    bs = [G.randn(9 + i, c, scale=0.1) for i, c in enumerate(couts)]
    return (lambda wb: ops.conv5x5_c64_h16(xh, wb[0], wb[1])), (lambda: ([w.to(cuda) for w in ws], [b.to(cuda) for b in bs])), 2e-5, 0.0


def _grad_of_input(fn, x, g):
    x = x.detach().clone().requires_grad_(True)
    fn(x).backward(g)
    return x.grad


def _ag_conv(ops, cuda):
    """the input gradient of a recorded 3x3 convolution: autograd's transposed, flipped weight (the crop-sized kernel's bound)"""
    from eavsr_amd import autograd as AG
    from tests.golden import cases as G
    x, g = G.randn(31, 1, 64, 20, 28).to(cuda), G.randn(32, 1, 64, 20, 28).to(cuda)
    wt, b = G.randn(33, 64, 64, 3, 3, scale=1.0 / 24.0), G.randn(34, 64, scale=0.1)
    return (lambda wb: _grad_of_input(lambda v: AG.conv2d([v, v], wb[0], wb[1]), x, g)), \
        (lambda: (torch.cat([wt, wt], 1).to(cuda), b.to(cuda))), 2e-5, 0.0


def _ag_dcn(ops, cuda):
    """the input gradient of a DCNv2 that the column backward takes (16 -> 32 channels, two groups): W^T . dOut through
    autograd's (cin 9, cout, 1, 1) weight; col2im adds with float atomics, whose order moves a sum of <= 9 x 32 fp32 terms by a
    few ulps of its largest partial sum: 1e-5 of the gradient's scale"""
    from eavsr_amd import autograd as AG
    from tests.golden import cases as G
    x, off, mask, wt, b, dg = _il8_inputs(ops, cuda, c=16, cout=32, dg=2, n=1, h=9, w=33)
    g = G.randn(41, 1, 32, 9, 33).to(cuda)
    return (lambda wb: _grad_of_input(lambda v: AG.modulated_deform_conv2d(v, off, mask, wb[0], wb[1], 1, 1, 1, 1, dg), x, g)), \
        (lambda: (wt.to(cuda), b.to(cuda))), 1e-5, 0.0


OTHER_CACHES = [("dcnv2_il-il", _dcn_il("il")), ("dcnv2_il-il2", _dcn_il("il2")), ("dcnv2_il16", _dcn_il16),
                ("conv3x3_c64_h16", _h16_conv(64, 2, relu=True)), ("conv3x3_c64_h16_act-shuffle", _h16_conv(256, 14, act="lrelu", slope=0.1, pixel_shuffle2=True)),
                ("conv3x3_c64to3_h16", _h16_conv(3, 22)), ("conv5x5_c64_h16", _h16_conv5), ("autograd-conv-dgrad", _ag_conv),
                ("autograd-dcn-columns", _ag_dcn)]


@pytest.mark.parametrize("name,build", OTHER_CACHES, ids=[n for n, _ in OTHER_CACHES])
def test_a_derived_weight_is_ordered_after_its_derivation(ops, cuda, tick, name, build):
    from eavsr_amd.weight_cache import WEIGHT_CACHES
    run, fresh, rel, floor = build(ops, cuda)
    with torch.no_grad() if not name.startswith("autograd") else torch.enable_grad():
        eager = run(fresh()).float().cpu()
        torch.cuda.synchronize(cuda)
        out_a, out_b, grew, asleep = _two_streams(cuda, tick, list(WEIGHT_CACHES), run, fresh)
    print(f"{name}: filled {grew}")
    assert set(FILLS[name]) <= set(grew), f"{name}: the call with fresh weights filled {grew}, not {FILLS[name]}"
    assert asleep, f"{name}: stream A had drained when stream B's call returned: nothing was shown"
    bound = rel * max(1.0, eager.abs().max().item()) + floor
    for which, out in (("the deriving stream", out_a), ("the stream that hit the cache", out_b)):
        e = (out.float().cpu() - eager).abs().max().item()
        print(f"{name}: {which}: max|out - eager| {e:.3e} bound {bound:.3e}")
        assert e <= bound, f"{name}: on {which}: {e:.3e} > {bound:.3e} (nan: the cached form was read before it was derived)"


def test_the_parameters_of_part_c_name_every_weight_cache(ops):
    """FILLS has a line per parameter of part (c), each asserted by its own test; together they name every cache of ops and
    autograd (none is lab-only: a cache that only a lab mode fills would turn its parameter into a skip on the default library)"""
    names = _cache_names()
    assert len(names) >= 21
    ids = [c.id for c in _conv_cases()] + [n for n, _ in OTHER_CACHES] + ["lpips_conv", "pwc_conv3x3"]
    assert sorted(ids) == sorted(FILLS), sorted(set(ids) ^ set(FILLS))
    missing = sorted(set(names.values()) - {c for line in FILLS.values() for c in line})
    assert not missing, f"no parameter of part (c) fills {missing}"


H16_OPS = sorted(k for k, v in S.MODEL_OPS.items() if v == "test_graphed_forward_in_the_16bit_mode_reproduces_the_eager_forward")


def test_graphed_forward_in_the_16bit_mode_reproduces_the_eager_forward(ops, cuda, monkeypatch):
    """the x2 model in the bf16 backbone mode, captured whole (graph.GraphedForward) and replayed on two clips, bit for bit the
    eager forward -- once as shipped and once with the RCAB attention after the second convolution (scale_residual_h16) -- and
    every 16-bit op that stream_cases.MODEL_OPS sends here was called while capturing"""
    from argparse import Namespace
    from eavsr_amd import networks as Nw
    from eavsr_amd.eavsrp_model import EAVSRP
    from eavsr_amd.graph import GraphedForward
    from eavsr_amd.utils.synthetic import synthetic_clip
    from tests import helpers as H
    called, capturing = set(), [False]

    def counted(name, fn):
        def wrapper(*a, **k):
            if capturing[0]:
                called.add(name)
            return fn(*a, **k)
        return wrapper
    for name in H16_OPS:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))
    net = EAVSRP(Namespace(predict=False, n_frame=3, n_flow=5, scale=2), None)
    net.load_state_dict(H.filled(H.model_shapes("x2"), "trained_like"), strict=True)
    net = net.to(cuda).eval()
    a, b = synthetic_clip(1, 3, 64, 64, seed=31).to(cuda), synthetic_clip(1, 3, 64, 64, seed=32).to(cuda)
    try:
        Nw.set_backbone_dtype("bf16")
        for pre in (True, False):
            Nw.set_rcab_h16_pre(pre)
            with torch.no_grad():
                ya, yb = net(a).clone(), net(b).clone()
            capturing[0] = True
            g = GraphedForward(net, a, warmup=1)      # (its warm-up and its capture)
            capturing[0] = False
            assert torch.equal(g(a), ya) and torch.equal(g(b), yb) and torch.equal(g(a), ya)
            del g
    finally:
        Nw.set_rcab_h16_pre(True)
        Nw.set_backbone_dtype(None)
    assert sorted(called) == H16_OPS, f"never called under capture: {sorted(set(H16_OPS) - called)}"
