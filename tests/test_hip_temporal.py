"""The temporal metrics on the GPU: `ops.temporal_metrics` against the float32 numpy restatement (tests/temporal_ref.py),
and its plumbing -- `harness.pair_flows`, `harness.temporal_metrics`, `evaluate`, `super_resolve` -- against values computed by hand
from `pwc.estimate` and the op.

Bounds.  `count` is compared for equality.  err and epe are sums of non-negative float64 terms, each term the same bits on both
sides (every float32 operation of the definition is rounded on its own on both sides; the float64 products are exact), added in a
different order: the relative error of such a sum is at most n 2^-53, and the largest case has n = 3 * 64 * 130 terms -> 3e-12.
The tests ask for 1e-10.  All weights are synthetic."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import temporal_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SHAPES = [(2, 1, 1, 1), (2, 3, 2, 3), (3, 3, 11, 13), (9, 3, 17, 63), (2, 3, 16, 64), (2, 1, 16, 65), (3, 3, 64, 130)]

_NETS = {}


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """the networks this module caches are dropped when it ends, and the allocator's blocks with them"""
    yield
    _NETS.clear()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ the kernel
def _flow(rng, F, H, W, sigma):
    """constant over 8 x 8 blocks plus a little per-pixel noise: some pixels pass the motion-boundary test, some do not"""
    if sigma == 0:
        return np.zeros((F - 1, 2, H, W), np.float32)
    coarse = rng.normal(0, sigma, (F - 1, 2, -(-H // 8), -(-W // 8)))
    fine = np.repeat(np.repeat(coarse, 8, axis=2), 8, axis=3)[:, :, :H, :W]
    return (fine + rng.normal(0, 0.01, fine.shape)).astype(np.float32)


def _same_sums(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), what
    assert (np.abs(got[fin] - want[fin]) <= RTOL * np.abs(want[fin])).all(), (what, got, want)


def _check(ops, cuda, seq, fw, bw, scale, flow_b, what):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    err, count, epe = ops.temporal_metrics(dev(seq), dev(fw), dev(bw), scale, dev(flow_b))
    F = seq.shape[0]
    assert err.is_cuda and err.dtype == torch.float64 and count.dtype == torch.int64 and tuple(err.shape) == tuple(count.shape) == (F - 1,)
    want_err, want_count, want_epe = R.temporal_ref32(seq, fw, bw, scale, flow_b)
    assert count.cpu().numpy().tolist() == want_count.tolist(), (what, count.tolist(), want_count.tolist())
    _same_sums(err.cpu().numpy(), want_err, what + " err")
    if flow_b is None:
        assert epe is None
    else:
        assert epe.dtype == torch.float64 and tuple(epe.shape) == (F - 1,)
        _same_sums(epe.cpu().numpy(), want_epe, what + " epe")
    return want_count


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_float32_restatement(ops, cuda, shape):
    F, C, H, W = shape
    rng = np.random.default_rng(100 + SHAPES.index(shape))
    valid = 0
    case = 0
    for sigma in (0.0, 0.7, 6.0):
        for consistent in (True, False):
            seq = rng.random((F, C, H, W)).astype(np.float32)
            fw = _flow(rng, F, H, W, sigma)
            bw = (-fw + rng.normal(0, 0.05, fw.shape)).astype(np.float32) if consistent else _flow(rng, F, H, W, max(sigma, 0.7))
            scale = 255.0 if case % 2 == 0 else 1.0
            if scale == 1.0:
                seq = (seq * 300 - 20).astype(np.float32)      # samples below 0 and above 255 as well
            flow_b = _flow(rng, F, H, W, 1.5) if case % 3 != 2 else None
            valid += int(_check(ops, cuda, seq, fw, bw, scale, flow_b, f"{shape} sigma {sigma} consistent {consistent}").sum())
            case += 1
    assert valid > 0


@pytest.mark.parametrize("shape", [(3, 3, 11, 13), (2, 3, 16, 64), (2, 1, 16, 65)])
def test_kernel_on_flows_that_leave_the_frame_and_on_nan_and_inf(ops, cuda, shape):
    F, C, H, W = shape
    rng = np.random.default_rng(7)
    seq = rng.random((F, C, H, W)).astype(np.float32)
    flow_b = _flow(rng, F, H, W, 1.0)
    # out of every side: the whole field points left / right / up / down by more than the frame in one quarter each
    fw = _flow(rng, F, H, W, 0.3)
    fw[:, 0, :H // 2, :W // 2] -= W
    fw[:, 0, :H // 2, W // 2:] += W
    fw[:, 1, H // 2:, :W // 2] -= H
    fw[:, 1, H // 2:, W // 2:] += H
    _check(ops, cuda, seq, fw, -fw, 255.0, flow_b, f"{shape} out of frame")
    # flows of +-1e4
    fw = _flow(rng, F, H, W, 0.3)
    fw[:, :, ::3, ::4] = 1e4
    fw[:, :, 1::3, 1::4] = -1e4
    _check(ops, cuda, seq, fw, -fw, 255.0, flow_b, f"{shape} 1e4")
    # NaN and inf at scattered pixels of fw, of bw and of flow_b
    fw, bw, fb = _flow(rng, F, H, W, 0.3), _flow(rng, F, H, W, 0.3), flow_b.copy()
    for k, (field, value) in enumerate(((fw, np.nan), (fw, np.inf), (fw, -np.inf), (bw, np.nan), (bw, np.inf), (fb, np.nan), (fb, -np.inf))):
        ys, xs = rng.integers(0, H, 3), rng.integers(0, W, 3)
        field[(k // 2) % (F - 1), k % 2, ys, xs] = value
    count = _check(ops, cuda, seq, fw, bw, 255.0, fb, f"{shape} nan / inf")
    assert 0 < count.sum() < (F - 1) * H * W
    # zero flow on every pixel: s lies on the last row / column for the pixels there, and everything is valid
    z = np.zeros_like(fw)
    assert _check(ops, cuda, seq, z, z, 255.0, None, f"{shape} zero").tolist() == [H * W] * (F - 1)
    # a whole pixel to the right and down: exactly on the last column / row from the one before it
    one = np.ones_like(fw)
    assert _check(ops, cuda, seq, one, -one, 255.0, None, f"{shape} one").tolist() == [(H - 1) * (W - 1)] * (F - 1)


def test_kernel_inputs_may_be_views_and_two_calls_agree_bit_for_bit(ops, cuda):
    F, C, H, W = 3, 3, 17, 63
    rng = np.random.default_rng(11)
    seq, fw, bw, fb = rng.random((F, C, H, W)).astype(np.float32), _flow(rng, F, H, W, 0.7), _flow(rng, F, H, W, 0.7), _flow(rng, F, H, W, 1.0)
    d = lambda a: torch.from_numpy(a).to(cuda)
    first = ops.temporal_metrics(d(seq), d(fw), d(bw), 255.0, d(fb))
    again = ops.temporal_metrics(d(seq), d(fw), d(bw), 255.0, d(fb))
    # the same values behind strides: a channels-last sequence, a flow cut out of a wider one, a flow stored column by column
    seq_v = d(seq).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    fw_v = torch.cat([d(fw), d(fw)], 3)[..., :W]
    bw_v = d(bw).transpose(2, 3).contiguous().transpose(2, 3)
    assert not seq_v.is_contiguous() and not fw_v.is_contiguous() and not bw_v.is_contiguous()
    views = ops.temporal_metrics(seq_v, fw_v, bw_v, 255.0, d(fb))
    for other in (again, views):
        for a, b in zip(first, other):
            assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    # what the op does not take is refused on the host
    with pytest.raises(ValueError):
        ops.temporal_metrics(d(seq), d(fw)[:1], d(bw), 255.0)
    with pytest.raises(ValueError):
        ops.temporal_metrics(d(seq), d(fw), d(bw), 255.0, d(fb)[:, :1])
    with pytest.raises(RuntimeError):
        ops.temporal_metrics(d(seq).double(), d(fw), d(bw))
    with pytest.raises(RuntimeError):
        ops.temporal_metrics(torch.from_numpy(seq), d(fw), d(bw))
    with pytest.raises(RuntimeError, match="C=2"):
        ops.temporal_metrics(d(seq)[:, :2], d(fw), d(bw))


# ------------------------------------------------------------------------------------------------------------ the harness
# Two estimators, because one cannot show everything.  "random": the synthetic PWC-Net weights of tests/test_hip_pwc.py -- flows of
# a pixel or two that differ between SR and HR frames, so tOF is a positive number that depends on the frames; but its forward and
# backward flows are nearly the same constant, the consistency test rejects every pixel, count is 0 and E_warp is `nan`.  "zero":
# PWC-Net with every weight and bias zero -- the flow is exactly 0 both ways, every pixel is valid, and E_warp is the mean squared
# difference of the two 8-bit SR frames, a finite positive number that depends on exactly which frames reached `seq` (the wrong
# sequence, a stale held frame or an uncropped frame would change it); tOF is 0.  Every harness test runs under both, and asserts
# that the numbers it compares exist: a positive valid share and a finite E_warp under "zero", a finite positive tOF under "random".
ESTIMATORS = ["zero", "random"]


def _pwc(cuda, kind="random"):
    if kind not in _NETS:
        from eavsr_amd.pwc import PWCNET
        from tests.test_pwc_host import pwc_weights
        net = PWCNET()
        sd = pwc_weights() if kind == "random" else {k: torch.zeros_like(v) for k, v in net.state_dict().items()}
        net.load_state_dict(sd, strict=True)
        _NETS[kind] = net.to(cuda).eval()
    return _NETS[kind]


def _frame_difference(sr):
    """E_warp under zero flow, from its meaning: the mean squared difference of consecutive 8-bit frames over 255^2 (exact integers)"""
    q = torch.clamp(sr * 255.0, 0, 255).round().double()
    sse = ((q[:-1] - q[1:]) ** 2).sum((1, 2, 3)).tolist()
    return [v / (int(sr.shape[1]) * int(sr.shape[2]) * int(sr.shape[3])) / (255.0 * 255.0) for v in sse]


def _scored(cols, kind, pairs):
    """the columns hold `pairs` entries, and the numbers the estimator can give are there"""
    for k in ("ewarp", "valid"):
        assert sum(v is not None for v in cols[k]) == pairs, (k, cols[k])
    if kind == "zero":
        assert all(v == 1.0 for v in cols["valid"] if v is not None)
        assert all(math.isfinite(v) and v > 0 for v in cols["ewarp"] if v is not None), cols["ewarp"]
    if cols["tof"] is not None and any(v is not None for v in cols["tof"]):
        assert sum(v is not None for v in cols["tof"]) == pairs
        assert all((v == 0.0) if kind == "zero" else (math.isfinite(v) and v > 0) for v in cols["tof"] if v is not None), cols["tof"]


def _sr_net(cuda):
    if "x4" not in _NETS:
        from eavsr_amd.eavsrp_model import EAVSRP
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        net.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
        _NETS["x4"] = net.to(cuda).eval()
    return _NETS["x4"]


def _clip(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return big[..., :h, :w].contiguous()


def _u8(n, t, h, w, seed):
    return (_clip(n, t, h, w, seed) * 255).round().to(torch.uint8)


def _by_hand(ops, sr, hr, net, flow_from="hr"):
    """one clip sr / hr (t, 3, H, W) in [0, 1]: `pwc.estimate` per direction, the op, the host's float64 formulas"""
    from eavsr_amd import pwc
    t, c, h, w = (int(v) for v in sr.shape)
    src = hr if flow_from == "hr" else sr
    with torch.no_grad():
        fw = pwc.estimate(src[:-1].contiguous(), src[1:].contiguous(), net)
        bw = pwc.estimate(src[1:].contiguous(), src[:-1].contiguous(), net)
        fb = pwc.estimate(sr[:-1].contiguous(), sr[1:].contiguous(), net) if flow_from == "hr" else None
    err, count, epe = ops.temporal_metrics(sr, fw, bw, 255.0, fb)
    err, count = err.tolist(), count.tolist()
    return {"ewarp": [e / (c * k) / (255.0 * 255.0) if k else math.nan for e, k in zip(err, count)],
            "valid": [k / (h * w) for k in count], "tof": None if epe is None else [v / (h * w) for v in epe.tolist()]}


def _same(a, b, nan_ok=False):
    """two lists of numbers / None, equal entry by entry; a `nan` equals nothing unless `nan_ok` (the "random" estimator's E_warp,
    which is `nan` by construction and is not what that estimator is there to check)"""
    if a is None or b is None:
        return a is None and b is None
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and
                                                                  (x == y or (nan_ok and x != x and y != y))) for x, y in zip(a, b))


def _same_cols(got, want, kind):
    return _same(got["ewarp"], want["ewarp"], nan_ok=kind == "random") and _same(got["valid"], want["valid"]) and _same(got["tof"], want["tof"])


def test_pair_flows_do_not_depend_on_the_pairs_that_share_the_call(cuda, monkeypatch):
    from eavsr_amd import harness, pwc
    net = _pwc(cuda)
    frames = _clip(1, 5, 70, 66, 3)[0].to(cuda)
    fw, bw = harness.pair_flows(frames, net)
    assert tuple(fw.shape) == tuple(bw.shape) == (4, 2, 70, 66)
    for t in range(4):
        fw1, bw1 = harness.pair_flows(frames[t:t + 2], net)
        assert torch.equal(fw1[0].view(torch.int32), fw[t].view(torch.int32)) and torch.equal(bw1[0].view(torch.int32), bw[t].view(torch.int32))
    with torch.no_grad():
        assert torch.equal(pwc.estimate(frames[:-1].contiguous(), frames[1:].contiguous(), net), fw)
        assert torch.equal(pwc.estimate(frames[1:].contiguous(), frames[:-1].contiguous(), net), bw)
    monkeypatch.setattr(harness, "_FLOW_PIXELS", 1)      # one pair per call
    fw2, bw2 = harness.pair_flows(frames, net)
    assert torch.equal(fw2, fw) and torch.equal(bw2, bw)
    # samples 0 .. 255 with scale 1 are brought to [0, 1] by one fp32 product
    levels = (frames[:2] * 255.0).round()
    fw3, bw3 = harness.pair_flows(levels, net, scale=1.0)
    fw4, bw4 = harness.pair_flows(levels * torch.tensor(1.0 / 255.0, dtype=torch.float32, device=cuda), net)
    assert torch.equal(fw3, fw4) and torch.equal(bw3, bw4)


@pytest.mark.parametrize("kind", ESTIMATORS)
@pytest.mark.parametrize("size", [(64, 64), (70, 66)])
def test_harness_temporal_metrics_equals_the_op_on_flows_estimated_by_hand(ops, cuda, size, kind):
    from eavsr_amd import harness
    net = _pwc(cuda, kind)
    h, w = size
    hr = _clip(2, 4, h, w, 5).to(cuda)
    sr = (hr + 0.03 * torch.randn(hr.shape, generator=torch.Generator().manual_seed(1)).to(cuda)).clamp(0, 1)
    for flow_from in ("hr", "sr"):
        got = harness.temporal_metrics(sr, hr if flow_from == "hr" else None, net, flow_from=flow_from if flow_from == "sr" else None)
        hand = [_by_hand(ops, sr[b], hr[b], net, flow_from) for b in range(2)]
        want = {k: None if hand[0][k] is None else hand[0][k] + hand[1][k] for k in ("ewarp", "valid", "tof")}
        assert (got["tof"] is None) == (flow_from == "sr") and _same_cols(got, want, kind), (flow_from, got, want)
        _scored(got, kind, 6)
        if kind == "zero":      # the SR frames are what is scored, not the HR frames, and every clip with its own
            assert got["ewarp"] == _frame_difference(sr[0]) + _frame_difference(sr[1])
            assert got["ewarp"] != _frame_difference(hr[0]) + _frame_difference(hr[1])
    assert _same_cols(harness.temporal_metrics(sr, hr, net, flow_from="sr"), harness.temporal_metrics(sr, None, net), kind)


@pytest.mark.parametrize("kind", ESTIMATORS)
def test_evaluate_reports_the_pairs_inside_every_item(ops, cuda, kind):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRPModel
    net = _pwc(cuda, kind)
    model = EAVSRPModel(Namespace(predict=False, n_frame=5, n_flow=5, scale=4, isTrain=False, gpu_ids=[0]))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    items = [{"lr_seq": _clip(1, 5, 64, 64, 10 + k), "hr_seq": _clip(1, 5, 256, 256, 20 + k),
              "fname": [["%03d_%05d.png" % (k, 5 * k + i)] for i in range(5)]} for k in range(2)]
    plain = harness.evaluate(model, items, per_frame=True)
    rep = harness.evaluate(model, items, per_frame=True, temporal=net)
    assert "frame_ewarp" not in plain and "ewarp" not in plain["report"]["final"]
    assert rep["frame_psnr"] == plain["frame_psnr"] and rep["frame_ssim"] == plain["frame_ssim"]
    want = {"ewarp": [], "valid": [], "tof": []}
    difference = []
    for data in items:
        model.set_input(data, 0)
        model.test()
        hand = _by_hand(ops, model.data_sr_seq[0], model.data_hr_seq[0], net)
        difference += [None] + _frame_difference(model.data_sr_seq[0])
        for k in want:
            assert len(hand[k]) == 4
            want[k] += [None] + hand[k]
    got = _got_frames(rep)
    assert len(rep["frame_ewarp"]) == 10 and rep["frame_ewarp"][0] is None and rep["frame_ewarp"][5] is None
    assert _same_cols(got, want, kind), (got, want)
    _scored(got, kind, 8)
    assert _same([fr["ewarp"] for fr in rep["report"]["frames"]], want["ewarp"], nan_ok=kind == "random")
    assert rep["report"]["scenes"]["000"]["tof"] == sum(want["tof"][1:5]) / 4
    if kind == "zero":
        assert rep["frame_ewarp"] == difference and rep["report"]["scenes"]["001"]["ewarp"] == sum(difference[6:]) / 4
    # the flows of the output itself: no tOF
    rep_sr = harness.evaluate(model, items[:1], per_frame=True, temporal=net, temporal_flow="sr")
    assert rep_sr["frame_tof"] == [None] * 5 and rep_sr["report"]["final"]["tof"] is None
    _scored(_got_frames(rep_sr), kind, 4)
    if kind == "zero":
        assert rep_sr["frame_ewarp"] == difference[:5]


def _hr_u8(t, h, w, seed):
    return (_clip(1, t, h, w, seed)[0] * 255).round().to(torch.uint8)


def _want_frames(ops, cuda, sr, hr_u8, runs, kind, flow_from="hr"):
    """per-frame columns of one clip: sr (t, 3, H, W) on the device, scored by hand inside each run [a, b) of frames; the numbers
    the estimator can give exist, and under zero flow E_warp is the difference of the frames of `sr`"""
    hr = ops.u8_to_f32(hr_u8.to(cuda))
    cols = {k: [None] * int(sr.shape[0]) for k in ("ewarp", "valid", "tof")}
    for a, b in runs:
        hand = _by_hand(ops, sr[a:b].contiguous(), hr[a:b].contiguous(), _pwc(cuda, kind), flow_from)
        if kind == "zero":
            assert hand["ewarp"] == _frame_difference(sr[a:b])
        for k in cols:
            if hand[k] is not None:
                cols[k][a + 1:b] = hand[k]
    _scored(cols, kind, sum(b - a - 1 for a, b in runs))
    return cols


def _got_frames(res):
    return {"ewarp": res["frame_ewarp"], "valid": res["frame_valid"], "tof": res["frame_tof"]}


@pytest.mark.parametrize("kind", ESTIMATORS)
def test_super_resolve_scores_every_pair_once_whatever_the_chunks(ops, cuda, monkeypatch, kind):
    from eavsr_amd import harness
    from eavsr_amd.segments import plan_segments
    for name in ("EAVSR_TEMPORAL", "EAVSR_MAX_FRAMES", "EAVSR_SCENE_CUTS", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_ENSEMBLE"):
        monkeypatch.delenv(name, raising=False)
    net, flow = _sr_net(cuda), _pwc(cuda, kind)
    u8, hr = _u8(1, 9, 64, 64, 41), _hr_u8(9, 256, 256, 42)
    with torch.no_grad():
        sr = net.forward_video(u8.to(cuda))[0].clone()
    want = _want_frames(ops, cuda, sr, hr, [(0, 9)], kind)
    assert want["ewarp"][0] is None and all(v is not None for v in want["ewarp"][1:])
    assert len(set(want["tof" if kind == "random" else "ewarp"][1:])) == 8      # eight different pairs: a mix-up would show
    plain = harness.super_resolve(net, u8[0], hr=hr)
    assert "frame_ewarp" not in plain and "ewarp" not in plain["report"]["final"]
    for chunk in (9, 4, 1):
        res = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=chunk, temporal=flow)
        assert _same_cols(_got_frames(res), want, kind), (chunk, _got_frames(res), want)
        assert res["frame_psnr"] == plain["frame_psnr"] and res["frame_ssim"] == plain["frame_ssim"]
        assert _same([fr["ewarp"] for fr in res["report"]["frames"]], want["ewarp"], nan_ok=kind == "random")
        assert res["report"]["final"]["tof"] == sum(want["tof"][1:]) / 8
        if kind == "zero":
            assert res["report"]["final"]["ewarp"] == sum(want["ewarp"][1:]) / 8
    # windows of six frames that share two: the pair across two emit ranges is scored once, on the frames that were emitted
    plan = plan_segments(9, [], 6, 2)
    assert len(plan) > 1
    with torch.no_grad():
        sr_seg = net.forward_video(u8.to(cuda), segments=plan)[0].clone()
    assert not torch.equal(sr_seg, sr)      # other frames than the one window's: the numbers below are these frames'
    want_seg = _want_frames(ops, cuda, sr_seg, hr, [(0, 9)], kind)
    for chunk in (None, 1):
        res = harness.super_resolve(net, u8[0], hr=hr, max_frames=6, overlap=2, frame_chunk=chunk, temporal=flow)
        assert [tuple(s) for s in res["segments"]] == plan and _same_cols(_got_frames(res), want_seg, kind), chunk
    # a scene cut: the pair (4, 5) is absent, every other pair is what it is by hand on the same frames
    plan = plan_segments(9, [5])
    with torch.no_grad():
        sr_cut = net.forward_video(u8.to(cuda), segments=plan)[0].clone()
    want_cut = _want_frames(ops, cuda, sr_cut, hr, [(0, 5), (5, 9)], kind)
    for chunk in (None, 2):
        res = harness.super_resolve(net, u8[0], hr=hr, cuts=[0, 5], frame_chunk=chunk, temporal=flow)
        assert res["scene_starts"] == [5] and res["frame_ewarp"][5] is None and res["frame_tof"][5] is None
        assert _same_cols(_got_frames(res), want_cut, kind), chunk
    # a 0 alone in the list is the clip's own start: one window, every pair scored, as without cuts
    res = harness.super_resolve(net, u8[0], hr=hr, cuts=[0], temporal=flow)
    assert res["scene_starts"] == [] and [tuple(s) for s in res["segments"]] == [(0, 9, 0, 9)] and _same_cols(_got_frames(res), want, kind)
    # the output's own flows, without ground truth: no tOF and no report
    want_sr = _want_frames(ops, cuda, sr, hr, [(0, 9)], kind, "sr")
    res = harness.super_resolve(net, u8[0], frame_chunk=4, temporal=flow)
    assert "report" not in res and res["frame_tof"] == [None] * 9 and _same_cols(_got_frames(res), want_sr, kind)
    res = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=4, temporal=flow, temporal_flow="sr")
    assert _same_cols(_got_frames(res), want_sr, kind) and res["report"]["final"]["tof"] is None
    if kind == "random":
        return
    # the refusals, before a frame is read
    with pytest.raises(ValueError, match="needs the HR frames"):
        harness.super_resolve(net, u8[0], temporal=flow, temporal_flow="hr")
    with pytest.raises(ValueError, match="no-such-file"):
        harness.super_resolve(net, u8[0], hr=hr, temporal="no-such-file")
    with pytest.raises(ValueError, match="temporal_flow"):
        harness.super_resolve(net, u8[0], hr=hr, temporal=flow, temporal_flow="lr")
    with pytest.raises(ValueError, match="only C = 3"):
        harness.super_resolve(net, torch.zeros(9, 1, 64, 64), temporal=flow)


@pytest.mark.parametrize("kind", ESTIMATORS)
def test_super_resolve_scores_the_cropped_frames_of_a_padded_clip(ops, cuda, monkeypatch, kind):
    from eavsr_amd import harness
    for name in ("EAVSR_TEMPORAL", "EAVSR_PAD_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    net, flow = _sr_net(cuda), _pwc(cuda, kind)
    u8, hr = _u8(1, 9, 66, 70, 43), _hr_u8(9, 264, 280, 44)
    with torch.no_grad():
        sr = net.forward_video(u8.to(cuda), pad="reflect")[0].clone()
    assert tuple(sr.shape) == (9, 3, 264, 280)
    want = _want_frames(ops, cuda, sr, hr, [(0, 9)], kind)
    for chunk in (None, 4):
        res = harness.super_resolve(net, u8[0], hr=hr, pad="reflect", frame_chunk=chunk, temporal=flow)
        assert _same_cols(_got_frames(res), want, kind), (chunk, _got_frames(res), want)


@pytest.mark.parametrize("kind", ESTIMATORS)
@pytest.mark.parametrize("extra", [dict(tile=64), dict(ensemble=2)], ids=["tile", "ensemble"])
def test_super_resolve_composes_with_tiles_and_the_ensemble(ops, cuda, monkeypatch, tmp_path, extra, kind):
    from eavsr_amd import harness
    for name in ("EAVSR_TEMPORAL", "EAVSR_TILE", "EAVSR_ENSEMBLE"):
        monkeypatch.delenv(name, raising=False)
    net, flow = _sr_net(cuda), _pwc(cuda, kind)
    u8, hr = _u8(1, 3, 96, 112, 45), _hr_u8(3, 384, 448, 46)
    with torch.no_grad():      # the frames the sink sees: the blend of the tiles, the mean of the modes
        if "tile" in extra:
            sr = net.forward_tiled(u8.to(cuda), 64, overlap=32)[0].clone()
        else:
            sr = net.forward_ensemble(u8.to(cuda), 2)[0].clone()
    want = _want_frames(ops, cuda, sr, hr, [(0, 3)], kind)
    res = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=2, temporal=flow, **extra)
    got = _got_frames(res)
    assert _same_cols(got, want, kind), (got, want)
    rep = res["report"]
    assert _same([fr["ewarp"] for fr in rep["frames"]], res["frame_ewarp"], nan_ok=kind == "random")
    assert rep["final"]["tof"] == sum(want["tof"][1:]) / 2 and "tof" in rep["scenes"]["000"]
    assert rep["final"]["ewarp"] == (sum(want["ewarp"][1:]) / 2 if kind == "zero" else None)
    text = open(harness.write_metrics_log(rep, str(tmp_path / "log.txt"))).read().splitlines()
    assert text[1].endswith("  ewarp -  tof -") and "  ewarp " in text[2] and "  tof " in text[-1]
