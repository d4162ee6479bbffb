"""NIQE on the GPU: `ops.niqe_moments` and `ops.niqe_half` against the float64 restatement (tests/niqe_ref.py),
`niqe.NIQE` end to end, and the plumbing through `harness.frame_metrics`, `evaluate` and `super_resolve`.  The pristine model is
synthetic (mu random, cov = A A^T + I): no pristine model ships, and the values depend on it.

Bounds.  The counts are compared for equality: the kernel and the restatement compute M by the same float64 operations in the same
order (no fused multiply-add on either side), so M's signs are the same.  The sums are sums of at most 96 * 96 non-negative float64
terms, the same terms on both sides in another order: relative error <= 9216 * 2^-53 = 1e-12; the tests ask for 1e-10, the bound of
the project's other fixed-order float64 sums.  `niqe_half`: 16 products of weights with |sum| <= 1.5 and values <= 255, each
rounded to 2^-53 relative, against a matrix product in another order: below 1e-12 absolute.
The score: measured on one MI355X, the largest relative difference between `NIQE(...)` and the restatement over SCORE_CASES is
1.5e-15 (profiles/r23_niqe_parity.json, written by tools/gpu_niqe_time.py --parity); SCORE_RTOL is ten times that."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import niqe_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-10
SCORE_RTOL = 1.5e-14
# (C, H, W, seed, crop_border): two blocks and more, extra rows / columns that are cropped away, with and without a border
SCORE_CASES = [(3, 96, 192, 11, 0), (1, 200, 130, 12, 0), (3, 202, 298, 13, 5), (3, 192, 192, 14, 0)]

_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """the networks and the resize tables this module caches are dropped when it ends, and the allocator's blocks with them"""
    yield
    from eavsr_amd import niqe
    _CACHE.clear()
    niqe.clear_device_tables()
    torch.cuda.empty_cache()


def _model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (36, 36))
    return rng.normal(0, 1, 36), a @ a.T + np.eye(36)


def _scorer():
    if "scorer" not in _CACHE:
        from eavsr_amd.niqe import NIQE
        _CACHE["scorer"] = NIQE(_model())
    return _CACHE["scorer"]


def _ref_plane(img, scale, y0, x0, h, w):
    """the reference's cropped luma plane of one frame (C, H, W): float64 integers"""
    return R.luma(R.quantise(img[:, y0:y0 + h, x0:x0 + w], scale)).astype(np.float64)


def _same_moments(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(-1, 5, 5), want.reshape(-1, 5, 5)
    assert np.array_equal(g[..., :2], w[..., :2]), (what, "counts")
    assert (np.abs(g[..., 2:] - w[..., 2:]) <= RTOL * np.abs(w[..., 2:])).all(), (what, np.abs(g[..., 2:] / np.maximum(w[..., 2:], 1e-300) - 1).max())


# ------------------------------------------------------------------------------------------------------------ niqe_moments
@pytest.mark.parametrize("blocks", [(1, 1), (1, 2), (2, 1), (3, 2)])
def test_moments_equal_the_restatement(ops, cuda, blocks):
    bh, bw = blocks
    k = [(1, 1), (1, 2), (2, 1), (3, 2)].index(blocks)
    # the frame that holds exactly the blocks, and frames with 1 .. 95 extra rows and columns (and an origin off the corner)
    for case, (eh, ew, y0, x0, c, scale) in enumerate([(0, 0, 0, 0, 3, 255.0), (1 + 31 * k, 95 - 31 * k, 0, 0, 1, 255.0), (37, 10, 5, 5, 3, 1.0)]):
        h, w = bh * 96, bw * 96
        img = R.test_image(c, h + eh + y0, w + ew + x0, 100 + 10 * k + case, constant_block=(bh - 1, bw - 1) if case == 0 else None)
        if scale == 1.0:
            img = (img * 300 - 20).astype(np.float32)      # samples below 0 and above 255 as well
        crop = (y0, x0, h, w)
        got, luma = ops.niqe_moments(torch.from_numpy(img[None]).to(cuda), scale, 96, crop=None if case < 2 else crop)
        assert got.dtype == torch.float64 and tuple(got.shape) == (1, bh, bw, 25) and tuple(luma.shape) == (1, 1, h, w)
        plane = _ref_plane(img, scale, *crop)
        assert np.array_equal(luma[0, 0].cpu().numpy(), plane), (blocks, case)
        want = R.plane_moments(plane, 96)
        _same_moments(got[0].cpu().numpy(), want, (blocks, case))
        if case == 0:      # the constant block: no value on either side of 0 in any map
            assert (want[bh - 1, bw - 1].reshape(5, 5)[:, :2] == 0).all() and (got[0, bh - 1, bw - 1].cpu().numpy() == 0).all()


def test_moments_of_constant_frames(ops, cuda):
    for value, c in ((0.0, 3), (1.0, 3), (0.0, 1), (1.0, 1)):
        img = np.full((1, c, 96, 192), value, np.float32)
        got, luma = ops.niqe_moments(torch.from_numpy(img).to(cuda))
        plane = _ref_plane(img[0], 255.0, 0, 0, 96, 192)
        assert plane.min() == plane.max() == {(0.0, 3): 16, (1.0, 3): 235, (0.0, 1): 0, (1.0, 1): 255}[(value, c)]
        _same_moments(got[0].cpu().numpy(), R.plane_moments(plane, 96), (value, c))
        assert np.array_equal(luma[0, 0].cpu().numpy(), plane)
    assert (got[0].cpu().numpy().reshape(-1, 5, 5)[..., 0] + got[0].cpu().numpy().reshape(-1, 5, 5)[..., 1] <= 96 * 96).all()


def test_moments_of_an_fp64_plane_in_blocks_of_48(ops, cuda):
    rng = np.random.default_rng(3)
    plane = np.stack([R.imresize(_ref_plane(R.test_image(3, 192, 288, 30 + i), 255.0, 0, 0, 192, 288), 0.5) for i in range(2)])
    plane[1] += rng.normal(0, 1e-3, plane[1].shape)
    got, luma = ops.niqe_moments(torch.from_numpy(plane[:, None]).to(cuda), 255.0, 48)
    assert luma is None and tuple(got.shape) == (2, 2, 3, 25)
    for i in range(2):
        _same_moments(got[i].cpu().numpy(), R.plane_moments(plane[i], 48), i)
    # a block that is no multiple of the strip, off the corner
    got, _ = ops.niqe_moments(torch.from_numpy(plane[:1, None]).to(cuda), 1.0, 40, crop=(7, 9, 80, 120))
    _same_moments(got[0].cpu().numpy(), R.plane_moments(plane[0, 7:87, 9:129], 40), "block 40")


def test_moments_alone_and_in_company_twice_and_from_a_view(ops, cuda):
    imgs = np.stack([R.test_image(3, 130, 200, 40 + i) for i in range(3)])
    dev = torch.from_numpy(imgs).to(cuda)
    got, luma = ops.niqe_moments(dev)
    again, luma2 = ops.niqe_moments(dev)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64)) and torch.equal(luma, luma2)      # bit for bit
    for i in range(3):
        alone, plane = ops.niqe_moments(dev[i:i + 1])
        assert torch.equal(alone[0].view(torch.int64), got[i].view(torch.int64)) and torch.equal(plane[0], luma[i])
    _same_moments(got[1].cpu().numpy(), R.plane_moments(_ref_plane(imgs[1], 255.0, 0, 0, 96, 192), 96), "company")
    # a non-contiguous source: every second column of a wider tensor, and a channels-last tensor
    wide = torch.zeros((3, 3, 130, 400), device=cuda)
    wide[..., ::2] = dev
    view = wide[..., ::2]
    assert not view.is_contiguous()
    assert torch.equal(ops.niqe_moments(view)[0].view(torch.int64), got.view(torch.int64))
    assert torch.equal(ops.niqe_moments(dev.contiguous(memory_format=torch.channels_last))[0].view(torch.int64), got.view(torch.int64))


def test_moments_refusals(ops, cuda):
    x = torch.zeros((1, 3, 100, 200), device=cuda)
    for bad in ((0, 0, 96, 100), (0, 0, 192, 96), (10, 0, 96, 96), (-1, 0, 96, 96), (0, 0, 0, 96)):
        with pytest.raises(ValueError, match="crop"):
            ops.niqe_moments(x, crop=bad)
    with pytest.raises(ValueError, match="block"):
        ops.niqe_moments(x, block=97)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        ops.niqe_moments(x[:, :2])
    with pytest.raises(ValueError):
        ops.niqe_moments(x.half())
    with pytest.raises(RuntimeError):
        ops.niqe_moments(x.cpu())
    with pytest.raises(RuntimeError, match="block <= 80"):      # the C ABI's own refusal: an fp64 block of 96 does not fit the LDS
        ops.niqe_moments(x[:, :1].double(), block=96)


# ------------------------------------------------------------------------------------------------------------ niqe_half
@pytest.mark.parametrize("shape", [(96, 96), (96, 192), (288, 192)])
def test_half_equals_the_general_imresize(ops, cuda, shape):
    from eavsr_amd.niqe import resize_tables
    rng = np.random.default_rng(shape[1])
    planes = np.stack([_ref_plane(R.test_image(3, *shape, 50), 255.0, 0, 0, *shape), rng.random(shape) * 255])
    got = ops.niqe_half(torch.from_numpy(planes[:, None]).to(cuda), (resize_tables(shape[0]), resize_tables(shape[1])))
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 1, shape[0] // 2, shape[1] // 2)
    for i in range(2):
        assert np.abs(got[i, 0].cpu().numpy() - R.imresize(planes[i], 0.5)).max() <= 1e-12
    tables = ops.niqe_half_tables(resize_tables(shape[0]), resize_tables(shape[1]), cuda)
    assert torch.equal(ops.niqe_half(torch.from_numpy(planes[:, None]).to(cuda), tables), got)
    # another scale through the same kernel: the tables are general
    third = ops.niqe_half(torch.from_numpy(planes[:1, None]).to(cuda), (resize_tables(shape[0], 0.3), resize_tables(shape[1], 0.3)))
    assert np.abs(third[0, 0].cpu().numpy() - R.imresize(planes[0], 0.3)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------ NIQE(...)
def score_case(case):
    """(frame (C, H, W) float32, crop_border, the restatement's score): no fit near a tie, no nan row -- asserted"""
    if ("case", case) not in _CACHE:
        c, h, w, seed, border = case
        img = R.test_image(c, h, w, seed)
        mu_p, cov_p = _model()
        want, margin, bad = R.niqe(img, mu_p, cov_p, 255.0, border)
        assert margin > 1e-9 and bad == 0 and math.isfinite(want), (case, margin, bad, want)
        _CACHE[("case", case)] = (img, border, want)
    return _CACHE[("case", case)]


@pytest.mark.parametrize("case", SCORE_CASES)
def test_niqe_equals_the_restatement(cuda, case):
    img, border, want = score_case(case)
    got = _scorer()(torch.from_numpy(img[None]).to(cuda), 255.0, border)
    print("niqe", case, got[0], want, abs(got[0] - want) / want)
    assert len(got) == 1 and abs(got[0] - want) <= SCORE_RTOL * want, (got, want)


def test_niqe_of_several_frames_drops_a_constant_block_and_refuses_one_block(cuda):
    scorer = _scorer()
    imgs = np.stack([R.test_image(3, 192, 288, 60), R.test_image(3, 192, 288, 61, constant_block=(1, 1)), R.test_image(3, 192, 288, 62)])
    got = scorer(torch.from_numpy(imgs).to(cuda))
    mu_p, cov_p = _model()
    for i in range(3):
        want, margin, bad = R.niqe(imgs[i], mu_p, cov_p)
        assert margin > 1e-9 and bad == (1 if i == 1 else 0)
        assert abs(got[i] - want) <= SCORE_RTOL * want, (i, got[i], want)
        assert scorer(torch.from_numpy(imgs[i:i + 1]).to(cuda)) == [got[i]]      # the same alone as in company
    # fewer than two blocks: nan, with and without a border that removes a block
    assert all(math.isnan(v) for v in scorer(torch.from_numpy(imgs[:2, :, :96, :96]).to(cuda)))
    assert all(math.isnan(v) for v in scorer(torch.from_numpy(imgs[:1, :, :100, :192]).to(cuda), 255.0, 3))
    assert math.isfinite(scorer(torch.from_numpy(imgs[:1, :, :102, :198]).to(cuda), 255.0, 3)[0])
    with pytest.raises(ValueError, match="crop_border"):
        scorer(torch.from_numpy(imgs[:1]).to(cuda), 255.0, -1)


# ------------------------------------------------------------------------------------------------------------ the harness
def _sr_net(cuda):
    if "x4" not in _CACHE:
        from eavsr_amd.eavsrp_model import EAVSRP
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        net.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
        _CACHE["x4"] = net.to(cuda).eval()
    return _CACHE["x4"]


def _pwc(cuda):
    if "pwc" not in _CACHE:
        from eavsr_amd.pwc import PWCNET
        net = PWCNET()
        net.load_state_dict({k: torch.zeros_like(v) for k, v in net.state_dict().items()}, strict=True)
        _CACHE["pwc"] = net.to(cuda).eval()
    return _CACHE["pwc"]


def _clip(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return big[..., :h, :w].contiguous()


def _u8(t, h, w, seed):
    return (_clip(1, t, h, w, seed)[0] * 255).round().to(torch.uint8)


def _scored(values, count):
    assert len(values) == count and all(math.isfinite(v) and v > 0 for v in values) and len(set(values)) == count, values


def test_frame_metrics_and_evaluate_report_the_column(cuda, tmp_path):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRPModel
    scorer = _scorer()
    model = EAVSRPModel(Namespace(predict=False, n_frame=5, n_flow=5, scale=4, isTrain=False, gpu_ids=[0]))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    items = [{"lr_seq": _clip(1, 5, 64, 64, 10 + k), "hr_seq": _clip(1, 5, 256, 256, 20 + k),
              "fname": [["%03d_%05d.png" % (k, 5 * k + i)] for i in range(5)]} for k in range(2)]
    plain = harness.evaluate(model, items, per_frame=True)
    rep = harness.evaluate(model, items, per_frame=True, niqe=scorer, niqe_crop=2)
    assert "frame_niqe" not in plain and "niqe" not in plain["report"]["final"]
    assert rep["frame_psnr"] == plain["frame_psnr"] and rep["frame_ssim"] == plain["frame_ssim"]
    want, want_fm = [], []
    for data in items:
        model.set_input(data, 0)
        model.test()
        vis = model.get_current_visuals()["data_sr_seq"]      # 0 .. 255: scale 1
        frames = vis.reshape((-1,) + tuple(vis.shape[-3:])).to(cuda).float()
        want += scorer(frames, 1.0, 2)
        want_fm += scorer(frames, 1.0, 0)
        fm = harness.frame_metrics(model.data_sr_seq, model.data_hr_seq, niqe=scorer)
        assert fm["niqe"] == want_fm[-5:] and fm["psnr"] == harness.frame_metrics(model.data_sr_seq, model.data_hr_seq)["psnr"]
        assert "niqe" not in harness.frame_metrics(model.data_sr_seq, model.data_hr_seq)
    _scored(want, 10)
    assert want != want_fm
    assert rep["frame_niqe"] == want and [fr["niqe"] for fr in rep["report"]["frames"]] == want
    assert rep["report"]["scenes"]["001"]["niqe"] == sum(want[5:]) / 5
    assert rep["report"]["final"]["niqe"] == (sum(want[:5]) / 5 + sum(want[5:]) / 5) / 2
    # the option forms: opt.niqe_path / opt.niqe_crop, and True
    path = str(tmp_path / "model.npz")
    np.savez(path, mu_pris_param=scorer.params[0], cov_pris_param=scorer.params[1])
    model.opt.niqe_path, model.opt.niqe_crop = path, 2
    assert harness.evaluate(model, items[:1], per_frame=True)["frame_niqe"] == want[:5]
    assert harness.evaluate(model, items[:1], per_frame=True, niqe=True, niqe_crop=0)["frame_niqe"] == want_fm[:5]
    assert "frame_niqe" not in harness.evaluate(model, items[:1], per_frame=True, niqe=False)


def test_super_resolve_scores_footage_without_ground_truth_whatever_the_chunks(cuda, monkeypatch, tmp_path):
    from eavsr_amd import harness
    for name in ("EAVSR_NIQE", "EAVSR_TEMPORAL", "EAVSR_MAX_FRAMES", "EAVSR_SCENE_CUTS", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_ENSEMBLE"):
        monkeypatch.delenv(name, raising=False)
    net, scorer = _sr_net(cuda), _scorer()
    u8 = _u8(9, 96, 192, 41)
    with torch.no_grad():
        sr = net.forward_video(u8[None].to(cuda))[0].clone()
    assert tuple(sr.shape) == (9, 3, 384, 768)
    want = scorer(sr)
    _scored(want, 9)
    plain = harness.super_resolve(net, u8)
    assert "frame_niqe" not in plain and "report" not in plain
    for chunk in (9, 4, 1):
        res = harness.super_resolve(net, u8, frame_chunk=chunk, niqe=scorer)
        assert res["frame_niqe"] == want, (chunk, res["frame_niqe"], want)      # identical, not close
        rows = res["report"]["frames"]
        assert [set(fr) for fr in rows] == [{"name", "scene", "niqe"}] * 9 and [fr["niqe"] for fr in rows] == want
        assert res["report"]["final"] == {"scenes": 1, "niqe": sum(want) / 9} and "frame_psnr" not in res
    text = open(harness.write_metrics_log(res["report"], str(tmp_path / "log.txt"))).read().splitlines()
    assert text[1] == "  000_00000.png  niqe %.4f" % want[0] and text[-1] == "final, mean of 1 scenes  niqe %.4f" % (sum(want) / 9)
    # a border, from the argument and from the environment's path
    want5 = scorer(sr, 255.0, 5)
    assert want5 != want and harness.super_resolve(net, u8, niqe=scorer, niqe_crop=5)["frame_niqe"] == want5
    path = str(tmp_path / "model.npz")
    np.savez(path, mu_pris_param=scorer.params[0], cov_pris_param=scorer.params[1])
    monkeypatch.setenv("EAVSR_NIQE", path)
    assert harness.super_resolve(net, u8, frame_chunk=4)["frame_niqe"] == want
    assert "frame_niqe" not in harness.super_resolve(net, u8, niqe=False)
    monkeypatch.delenv("EAVSR_NIQE")
    # with ground truth: the old columns are what they were, the new one is beside them
    hr = (_clip(1, 9, 384, 768, 42)[0] * 255).round().to(torch.uint8)
    old = harness.super_resolve(net, u8, hr=hr, frame_chunk=4)
    res = harness.super_resolve(net, u8, hr=hr, frame_chunk=4, niqe=scorer, max_frames=6, overlap=2)
    seg = harness.super_resolve(net, u8, hr=hr, frame_chunk=4, max_frames=6, overlap=2)
    assert res["frame_psnr"] == seg["frame_psnr"] and res["frame_ssim"] == seg["frame_ssim"] and "niqe" not in old["report"]["final"]
    with torch.no_grad():
        sr_seg = net.forward_video(u8[None].to(cuda), segments=res["segments"])[0].clone()
    assert res["frame_niqe"] == scorer(sr_seg) and res["report"]["frames"][3]["niqe"] == res["frame_niqe"][3]
    assert res["report"]["final"]["psnr"] == seg["report"]["final"]["psnr"]
    # the refusals, before a frame is read
    with pytest.raises(ValueError, match="no-such-file"):
        harness.super_resolve(net, u8, niqe="no-such-file.npz")
    with pytest.raises(ValueError, match="niqe_crop"):
        harness.super_resolve(net, u8, niqe=scorer, niqe_crop=-1)
    with pytest.raises(ValueError, match="opt.niqe_path"):
        harness.super_resolve(net, u8, niqe=True)


@pytest.mark.parametrize("extra", ["pad", "tile", "ensemble", "temporal", "png"])
def test_super_resolve_scores_the_frames_the_sink_sees(cuda, monkeypatch, tmp_path, extra):
    from eavsr_amd import harness
    for name in ("EAVSR_NIQE", "EAVSR_TEMPORAL", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_ENSEMBLE", "EAVSR_PNG_ENCODER"):
        monkeypatch.delenv(name, raising=False)
    net, scorer = _sr_net(cuda), _scorer()
    t = 3
    u8 = _u8(t, 66, 70, 43) if extra == "pad" else _u8(t, 96, 192, 44)
    args = {"pad": dict(pad="reflect"), "tile": dict(tile=64), "ensemble": dict(ensemble=2), "temporal": dict(temporal=_pwc(cuda)),
            "png": dict(out_dir=str(tmp_path / "out"), png_encoder="device")}[extra]
    with torch.no_grad():
        x = u8[None].to(cuda)
        if extra == "pad":
            sr = net.forward_video(x, pad="reflect")[0].clone()
            assert tuple(sr.shape) == (t, 3, 264, 280)
        elif extra == "tile":
            sr = net.forward_tiled(x, 64, overlap=32)[0].clone()
        elif extra == "ensemble":
            sr = net.forward_ensemble(x, 2)[0].clone()
        else:
            sr = net.forward_video(x)[0].clone()
    want = scorer(sr)
    _scored(want, t)
    res = harness.super_resolve(net, u8, frame_chunk=2, niqe=scorer, **args)
    assert res["frame_niqe"] == want, (extra, res["frame_niqe"], want)
    assert [fr["niqe"] for fr in res["report"]["frames"]] == want
    if extra == "temporal":
        assert res["frame_ewarp"] == harness.super_resolve(net, u8, frame_chunk=2, **args)["frame_ewarp"] and res["frame_ewarp"][1] is not None
    if extra == "png":
        host = harness.super_resolve(net, u8, frame_chunk=2, niqe=scorer, out_dir=str(tmp_path / "host"), png_encoder="host")
        assert host["frame_niqe"] == want and len(res["written"]) == len(host["written"]) == t
        assert torch.equal(harness.read_png(res["written"][1]), harness.read_png(host["written"][1]))
