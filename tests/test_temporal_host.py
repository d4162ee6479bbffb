"""The temporal metrics without a device: the two numpy restatements against each other and against hand-built cases
with known answers, the report's new columns, the refusals, the C ABI."""
import math
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(rng, F, C, H, W):
    """8-bit frames as the samples 0 .. 255 (scale 1)"""
    return rng.integers(0, 256, (F, C, H, W)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the two restatements agree
@pytest.mark.parametrize("seed,shape", [(1, (3, 3, 11, 13)), (2, (2, 1, 16, 65)), (3, (4, 3, 9, 31))])
def test_ref32_equals_ref64_where_every_fp32_operation_is_exact(seed, shape):
    """fw in multiples of 1/8 pixel, bw in multiples of 1/2, 8-bit frames: every float32 sum and product of the warp and of the
    flow magnitudes is exact (at most 20 significant bits), so float32 and float64 compute the same numbers"""
    rng = np.random.default_rng(seed)
    F, C, H, W = shape
    seq = _frames(rng, F, C, H, W)
    # constant over 4 x 4 blocks: pixels inside a block pass the motion-boundary test, so the count is not trivially zero
    coarse = rng.integers(-12, 13, (F - 1, 2, -(-H // 4), -(-W // 4))) / 8.0
    fw = np.repeat(np.repeat(coarse, 4, axis=2), 4, axis=3)[:, :, :H, :W].astype(np.float32)
    bw = (np.round(-fw * 2) / 2).astype(np.float32)
    flow_b = (rng.integers(-24, 25, (F - 1, 2, H, W)) / 8.0).astype(np.float32)
    e32, n32, p32 = R.temporal_ref32(seq, fw, bw, 1.0, flow_b)
    e64, n64, p64 = R.temporal_ref64(seq, fw, bw, 1.0, flow_b)
    assert np.array_equal(n32, n64) and n32.sum() > 0
    assert np.allclose(e32, e64, rtol=1e-12, atol=0) and np.allclose(p32, p64, rtol=1e-12, atol=0)
    assert (e32 > 0).any() and (p32 > 0).all()


# ---------------------------------------------------------------------------------------------- hand-built cases
@pytest.mark.parametrize("ref", [R.temporal_ref32, R.temporal_ref64])
def test_zero_flow_is_the_frame_difference_with_every_pixel_valid(ref):
    rng = np.random.default_rng(5)
    seq = _frames(rng, 3, 3, 7, 9)
    z = np.zeros((2, 2, 7, 9), np.float32)
    err, count, epe = ref(seq, z, z, 1.0, z)
    assert count.tolist() == [63, 63] and epe.tolist() == [0.0, 0.0]
    want = [float(((seq[t].astype(np.float64) - seq[t + 1]) ** 2).sum()) for t in range(2)]
    assert err.tolist() == want
    # the same frames in [0, 1] with scale 255
    err255, count255, _ = ref(seq / np.float32(255), z, z, 255.0)
    assert err255.tolist() == want and count255.tolist() == [63, 63]


@pytest.mark.parametrize("dx,dy", [(2, 0), (-3, 1), (0, -2), (1, 3)])
def test_integer_shift_has_no_error_inside_the_frame(dx, dy):
    rng = np.random.default_rng(6)
    H, W = 10, 12
    big = _frames(rng, 1, 3, H + 8, W + 8)[0]
    cur = big[:, 4:4 + H, 4:4 + W]
    nxt = big[:, 4 - dy:4 - dy + H, 4 - dx:4 - dx + W]      # content moves by (dx, dy): nxt[y + dy, x + dx] = cur[y, x]
    fw = np.zeros((1, 2, H, W), np.float32)
    fw[0, 0], fw[0, 1] = dx, dy
    for ref in (R.temporal_ref32, R.temporal_ref64):
        err, count, _, mask = ref(np.stack([cur, nxt]), fw, -fw, 1.0, masks=True)
        assert err.tolist() == [0.0] and count.tolist() == [(W - abs(dx)) * (H - abs(dy))]
        ys, xs = np.nonzero(mask[0])
        assert ((xs + dx >= 0) & (xs + dx <= W - 1) & (ys + dy >= 0) & (ys + dy <= H - 1)).all()


def test_inconsistent_backward_flow_masks_exactly_its_region():
    rng = np.random.default_rng(7)
    H, W = 12, 14
    seq = _frames(rng, 2, 3, H, W)
    fw = np.zeros((1, 2, H, W), np.float32)
    bw = np.zeros_like(fw)
    bw[0, 0, 3:6, 4:9] = 2.0      # |fw + bw|^2 = 4 > 0.01 * 4 + 0.5 there, 0 elsewhere
    for ref in (R.temporal_ref32, R.temporal_ref64):
        _, count, _, mask = ref(seq, fw, bw, 1.0, masks=True)
        want = np.ones((H, W), bool)
        want[3:6, 4:9] = False
        assert np.array_equal(mask[0], want) and count.tolist() == [H * W - 15]


def test_flow_step_edge_masks_the_motion_boundary():
    rng = np.random.default_rng(8)
    H, W = 8, 16
    seq = _frames(rng, 2, 1, H, W)
    fw = np.zeros((1, 2, H, W), np.float32)
    fw[0, 0, :, 8:] = 1.0         # the right half moves one pixel to the right; bw agrees with it everywhere it is read
    bw = -fw
    for ref in (R.temporal_ref32, R.temporal_ref64):
        _, _, _, mask = ref(seq, fw, bw, 1.0, masks=True)
        want = np.ones((H, W), bool)
        want[:, 7] = False        # the forward difference to the right is 1 there: 1 > 0.01 * 0 + 0.002
        want[:, W - 1] = False    # x + 1 leaves the frame
        assert np.array_equal(mask[0], want)


def test_nan_and_inf_flow_remove_exactly_the_pixels_that_read_them():
    rng = np.random.default_rng(9)
    H, W = 9, 11
    seq = _frames(rng, 2, 3, H, W)
    fw = np.zeros((1, 2, H, W), np.float32)
    bw = np.zeros_like(fw)
    fw[0, 0, 4, 5] = np.nan
    fw[0, 1, 2, 8] = np.inf
    fw[0, 0, 7, 1] = -np.inf
    for ref in (R.temporal_ref32, R.temporal_ref64):
        err, count, _, mask = ref(seq, fw, bw, 1.0, masks=True)
        want = np.ones((H, W), bool)
        for y, x in ((4, 5), (2, 8), (7, 1)):      # the pixel itself, and the neighbours whose forward differences read it
            want[y, x] = want[y, x - 1] = want[y - 1, x] = False
        assert np.array_equal(mask[0], want) and count.tolist() == [H * W - 9] and np.isfinite(err).all()


def test_a_sample_on_the_last_row_or_column_is_valid_and_reads_nothing_outside():
    rng = np.random.default_rng(10)
    H, W = 6, 7
    seq = _frames(rng, 2, 3, H, W)
    fw = np.zeros((1, 2, H, W), np.float32)
    fw[0, 0, :, W - 3:] = 1.0         # column W - 2 lands exactly on column W - 1; its neighbours move with it (no motion boundary)
    fw[0, 1, H - 2:, :3] = 1.0        # pixels (H - 2, 0) and (H - 2, 1) land exactly on the last row
    bw = np.zeros_like(fw)
    bw[0, 0, :, W - 2:] = -1.0
    bw[0, 1, H - 1, :3] = -1.0
    for ref in (R.temporal_ref32, R.temporal_ref64):
        err, count, _, mask = ref(seq, fw, bw, 1.0, masks=True)      # an index past the frame would raise in numpy
        assert mask[0, :H - 2, W - 2].all() and mask[0, H - 2, 0] and mask[0, H - 2, 1]
        assert not mask[0, :, W - 1].any() and not mask[0, H - 1, :3].any()      # one step further is out of frame
        # every flow is a whole number of pixels: the warped sample is the sample itself, with weight 1
        ys, xs = np.nonzero(mask[0])
        ty, tx = ys + fw[0, 1, ys, xs].astype(int), xs + fw[0, 0, ys, xs].astype(int)
        want = ((seq[0][:, ys, xs].astype(np.float64) - seq[1][:, ty, tx]) ** 2).sum()
        assert err.tolist() == [float(want)] and count.tolist() == [len(ys)]


# ---------------------------------------------------------------------------------------------- the report
def _report_inputs():
    names = ["000_00000.png", "000_00001.png", "000_00002.png", "001_00003.png", "001_00004.png"]
    return names, [30.0, 31.0, 32.0, 20.0, 22.0], [0.9, 0.91, 0.92, 0.8, 0.82]


def test_scene_report_and_log_carry_the_temporal_columns(tmp_path):
    from eavsr_amd import harness
    names, psnr, ssim = _report_inputs()
    temporal = {"ewarp": [None, 0.001, 0.003, None, 0.01], "tof": [None, 0.5, 0.7, None, 0.2]}
    rep = harness.scene_report(names, psnr, ssim, temporal=temporal)
    assert [fr["ewarp"] for fr in rep["frames"]] == temporal["ewarp"] and [fr["tof"] for fr in rep["frames"]] == temporal["tof"]
    assert rep["scenes"]["000"]["ewarp"] == (0.001 + 0.003) / 2 and rep["scenes"]["001"]["ewarp"] == 0.01
    assert rep["scenes"]["000"]["tof"] == (0.5 + 0.7) / 2 and rep["scenes"]["001"]["tof"] == 0.2
    assert rep["final"]["ewarp"] == ((0.001 + 0.003) / 2 + 0.01) / 2 and rep["final"]["tof"] == ((0.5 + 0.7) / 2 + 0.2) / 2
    assert rep["final"]["psnr"] == (31.0 + 21.0) / 2      # the other columns are untouched
    text = open(harness.write_metrics_log(rep, str(tmp_path / "a.txt"))).read().splitlines()
    assert text[1] == "  000_00000.png  psnr 30.00  ssim 0.9000  ewarp -  tof -"
    assert text[2] == "  000_00001.png  psnr 31.00  ssim 0.9100  ewarp 0.001000  tof 0.5000"
    assert text[4] == "  mean of 3 frames  psnr 31.00  ssim 0.9100  ewarp 0.002000  tof 0.6000"
    assert text[-1] == "final, mean of 2 scenes  psnr 26.00  ssim 0.8600  ewarp 0.006000  tof 0.4000"
    # no HR flows: no tOF anywhere; a scene of one frame has no pair at all
    rep = harness.scene_report(names[:4], psnr[:4], ssim[:4], lpips=[0.1] * 4, temporal={"ewarp": [None, 0.5, 0.25, None], "tof": None})
    assert rep["scenes"]["001"]["ewarp"] is None and rep["final"]["ewarp"] == 0.375 and rep["final"]["tof"] is None
    text = open(harness.write_metrics_log(rep, str(tmp_path / "b.txt"))).read().splitlines()
    assert text[2] == "  000_00001.png  psnr 31.00  ssim 0.9100  lpips 0.100  ewarp 0.500000  tof -"
    assert text[-2] == "  mean of 1 frames  psnr 20.00  ssim 0.8000  lpips 0.100  ewarp -  tof -"
    with pytest.raises(ValueError, match="ewarp"):
        harness.scene_report(names, psnr, ssim, temporal={"ewarp": [None], "tof": None})
    # a pair without a valid pixel is `nan`: the frame keeps it, the means leave it out; a scene of nothing else has no mean
    rep = harness.scene_report(names, psnr, ssim, temporal={"ewarp": [None, math.nan, 0.003, None, math.nan], "tof": [None, 0.5, 0.7, None, 0.2]})
    assert math.isnan(rep["frames"][1]["ewarp"]) and rep["scenes"]["000"]["ewarp"] == 0.003 and rep["scenes"]["001"]["ewarp"] is None
    assert rep["final"]["ewarp"] == 0.003 and rep["final"]["tof"] == ((0.5 + 0.7) / 2 + 0.2) / 2
    text = open(harness.write_metrics_log(rep, str(tmp_path / "c.txt"))).read().splitlines()
    assert text[2] == "  000_00001.png  psnr 31.00  ssim 0.9100  ewarp nan  tof 0.5000"
    assert text[-2] == "  mean of 2 frames  psnr 21.00  ssim 0.8100  ewarp -  tof 0.2000"


def test_a_zero_in_an_explicit_cut_list_is_the_clips_own_start():
    """`super_resolve(cuts=[0, 5])` is `cuts=[5]` and `cuts=[0]` is `cuts=[]`; `plan_segments` itself goes on refusing a 0"""
    from eavsr_amd import harness
    from eavsr_amd.segments import plan_segments
    assert harness.explicit_cuts([0]) == [] and harness.explicit_cuts([]) == [] and harness.explicit_cuts([5, 0]) == [5]
    assert harness.explicit_cuts((7, 3)) == [3, 7]
    assert plan_segments(9, harness.explicit_cuts([0])) == plan_segments(9, []) == [(0, 9, 0, 9)]
    assert plan_segments(9, harness.explicit_cuts([0, 5])) == plan_segments(9, [5]) == [(0, 5, 0, 5), (5, 9, 5, 9)]
    with pytest.raises(ValueError):
        plan_segments(9, [0])
    with pytest.raises(ValueError):
        plan_segments(9, harness.explicit_cuts([0, 9]))      # every other start outside (0, t) is still refused


def test_report_and_log_without_temporal_are_what_they_were(tmp_path):
    from eavsr_amd import harness
    names, psnr, ssim = _report_inputs()
    for lp in (None, [0.1, 0.2, 0.3, 0.4, 0.5]):
        rep = harness.scene_report(names, psnr, ssim, lp)
        cols = {"name", "scene", "psnr", "ssim"} | ({"lpips"} if lp else set())
        assert all(set(fr) == cols for fr in rep["frames"]) and "ewarp" not in rep["final"] and "tof" not in rep["scenes"]["000"]
        got = open(harness.write_metrics_log(rep, str(tmp_path / "log.txt")), "rb").read()
        third = (lambda v: "  lpips %.3f" % v) if lp else (lambda v: "")
        want = ["scene 000"] + ["  %s  psnr %.2f  ssim %.4f" % (names[i], psnr[i], ssim[i]) + third(lp[i] if lp else 0) for i in range(3)]
        want.append("  mean of 3 frames  psnr 31.00  ssim 0.9100" + third(0.2))
        want += ["scene 001"] + ["  %s  psnr %.2f  ssim %.4f" % (names[i], psnr[i], ssim[i]) + third(lp[i] if lp else 0) for i in (3, 4)]
        want.append("  mean of 2 frames  psnr 21.00  ssim 0.8100" + third(0.45))
        want.append("final, mean of 2 scenes  psnr 26.00  ssim 0.8600" + third((0.2 + 0.45) / 2))
        assert got == ("\n".join(want) + "\n").encode()


def test_temporal_values_on_the_host():
    from eavsr_amd import harness
    vals = harness.temporal_values([650.25 * 6, 0.0], [2, 0], [12.0, 3.0], 3, 2, 3)
    assert vals["ewarp"][0] == 650.25 * 6 / 6 / 65025.0 and math.isnan(vals["ewarp"][1])
    assert vals["valid"] == [2 / 6, 0.0] and vals["tof"] == [2.0, 0.5]
    assert harness.temporal_values([1.0], [1], None, 1, 1, 1)["tof"] is None


# ---------------------------------------------------------------------------------------------- the refusals: before any launch
class _Wrapper:
    """as much of a model wrapper as `evaluate` / `super_resolve` look at before they refuse"""
    device = torch.device("cpu")

    def __init__(self, **opt):
        self.opt = Namespace(**opt)

    def eval(self):
        raise AssertionError("refused too late: the model was touched")

    def parameters(self):
        raise AssertionError("refused too late: the model was touched")


def test_refusals(tmp_path, monkeypatch):
    from eavsr_amd import harness, pwc
    monkeypatch.delenv("EAVSR_TEMPORAL", raising=False)
    missing = str(tmp_path / "no-such-pwc-file")
    with pytest.raises(ValueError, match="per_frame"):
        harness.evaluate(_Wrapper(), [], temporal=missing)
    with pytest.raises(ValueError, match="no-such-pwc-file"):
        harness.evaluate(_Wrapper(), [], per_frame=True, temporal=missing)
    with pytest.raises(ValueError, match="no-such-pwc-file"):
        harness.evaluate(_Wrapper(pwc_path=missing), [], per_frame=True, temporal=True)
    with pytest.raises(ValueError, match="no-such-pwc-file"):
        harness.evaluate(_Wrapper(pwc_path=missing, temporal="sr"), [], per_frame=True)
    with pytest.raises(ValueError, match="opt.pwc_path"):
        harness.evaluate(_Wrapper(), [], per_frame=True, temporal=True)
    monkeypatch.setenv("EAVSR_TEMPORAL", "hr")
    with pytest.raises(ValueError, match="no-such-pwc-file"):
        harness.evaluate(_Wrapper(pwc_path=missing), [], per_frame=True)
    monkeypatch.setenv("EAVSR_TEMPORAL", "yes")
    with pytest.raises(ValueError, match="EAVSR_TEMPORAL='yes'"):
        harness.temporal_option(None)
    monkeypatch.delenv("EAVSR_TEMPORAL")
    assert harness.temporal_option(None) is None and harness.temporal_option(Namespace(temporal=False)) is None
    assert harness.temporal_option(Namespace(temporal="sr")) == "sr" and harness.temporal_option(Namespace(temporal=True)) is True
    with pytest.raises(ValueError, match="opt.temporal"):
        harness.temporal_option(Namespace(temporal="both"))
    with pytest.raises(ValueError, match="temporal=3"):
        harness.temporal_net(3)
    net = pwc.PWCNET()      # host memory; never run
    assert harness.temporal_net(net) is net
    sr = torch.zeros(1, 3, 3, 8, 8)
    with pytest.raises(ValueError, match="flow_from='hr' needs the HR frames"):
        harness.temporal_metrics(sr, None, net, flow_from="hr")
    with pytest.raises(ValueError, match="flow_from='both'"):
        harness.temporal_metrics(sr, sr, net, flow_from="both")
    with pytest.raises(ValueError, match="only C = 3"):
        harness.temporal_metrics(torch.zeros(1, 3, 1, 8, 8), None, net)
    with pytest.raises(ValueError, match="only C = 3"):
        harness.pair_flows(torch.zeros(3, 1, 8, 8), net)
    with pytest.raises(ValueError, match="a pair needs two"):
        harness.temporal_metrics(torch.zeros(1, 1, 3, 8, 8), None, net)
    with pytest.raises(ValueError, match="F >= 2"):
        harness.pair_flows(torch.zeros(1, 3, 8, 8), net)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_in_the_stable_header_bound_and_check_their_arguments_on_the_host():
    from eavsr_amd import _native, build
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header.split("EXPERIMENTAL -- exported by the LAB build only")[0]
    for name, res in (("eavsr_temporal_metrics_partials", "int32_t"), ("eavsr_temporal_metrics_f32", "int")):
        assert name in _native.SIGNATURES and re.search(r"^%s %s\(" % (res, name), stable, flags=re.M), name
    m = re.search(r"int eavsr_temporal_metrics_f32\(([^;]*)\);", stable)
    assert len(m.group(1).split(",")) == len(_native.SIGNATURES["eavsr_temporal_metrics_f32"][1]) == 14
    src = os.path.join(ROOT, "eavsr_amd", "csrc", "temporal.hip")
    assert src in build.sources() and src in build.sources(lab=True)
    assert "-ffp-contract=off" in build.PER_FILE_FLAGS["temporal.hip"]      # the definition rounds every operation on its own
    lib = _native.load()
    parts = lib.eavsr_temporal_metrics_partials
    assert parts(2, 1, 1, 1) == 1 and parts(3, 3, 64, 130) == 4 * 3 and parts(2, 3, 17, 63) == 2 and parts(2, 3, 720, 1280) == 45 * 20
    for bad in ((1, 3, 8, 8), (65537, 3, 8, 8), (2, 2, 8, 8), (2, 3, 0, 8), (2, 3, 8, 0), (2, 3, (1 << 24) + 1, 8)):
        assert parts(*bad) == -2, bad
    assert b"F=1" in (parts(1, 3, 8, 8), lib.eavsr_last_error())[1]
    g = lib.eavsr_temporal_metrics_f32
    p = 64      # an aligned, never dereferenced address: every call below returns before a launch
    assert g(None, p, p, None, 255.0, 2, 3, 8, 8, p, p, p, None, None) == -1 and b"NULL" in lib.eavsr_last_error()
    assert g(p, p, p, None, 255.0, 2, 3, 8, 8, None, p, p, None, None) == -1
    assert g(p, p, p, p, 255.0, 2, 3, 8, 8, p, p, p, None, None) == -1 and b"go together" in lib.eavsr_last_error()
    assert g(p, p, p, None, 255.0, 2, 3, 8, 8, p, p, p, p, None) == -1
    assert g(p, p, p, None, 255.0, 1, 3, 8, 8, p, p, p, None, None) == -2
    assert g(p, p, p, None, 255.0, 2, 4, 8, 8, p, p, p, None, None) == -2
    assert g(p, p, p, None, 255.0, 2, 3, 8, 8, p + 4, p, p, None, None) == -2 and b"aligned" in lib.eavsr_last_error()
