"""Videos of any length on the GPU (`pytest -m gpu`): the scene-cut statistics kernel (`ops.frame_change`, csrc/scene.hip)
against the numpy oracle of tests/scene_ref.py, `harness.scene_changes`, detection end to end, and the segmented forward --
`EAVSRP.forward_long(emit=)`, `EAVSRP.forward_segments`, `harness.super_resolve(max_frames=, cuts=)` -- against `forward_long`
on each frame's window, bit for bit."""
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import scene_ref as R

pytestmark = pytest.mark.gpu


def _frames(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8))


def _check(dev_frames, host_frames, hwc):
    from eavsr_amd import ops
    hist, sad = ops.frame_change(dev_frames, hwc=hwc)
    want_hist, want_sad = R.frame_change(host_frames.numpy(), hwc=hwc)
    assert hist.dtype == torch.int32 and sad.dtype == torch.int64
    assert tuple(hist.shape) == (host_frames.shape[0], 64) and tuple(sad.shape) == (host_frames.shape[0] - 1,)
    assert torch.equal(hist.cpu(), torch.from_numpy(want_hist)) and torch.equal(sad.cpu(), torch.from_numpy(want_sad))
    return hist, sad


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("f", [1, 2, 5])
@pytest.mark.parametrize("c,h,w", [(3, 64, 96), (3, 67, 131), (1, 33, 17)])
def test_frame_change_equals_the_oracle(cuda, f, c, h, w):
    """planar and (C = 3) interleaved; 64 x 96 is two workgroups' worth of 16-pixel lanes on the aligned path, 67 x 131 = 8777 pixels
    (three workgroups, a 9-pixel tail, every plane at another alignment), 33 x 17 less than one workgroup"""
    from eavsr_amd import ops
    x = _frames((f, c, h, w), seed=f * 1000 + h)
    _check(x.to(cuda), x, False)
    if c == 3:
        y = x.permute(0, 2, 3, 1).contiguous()
        hist, sad = _check(y.to(cuda), y, True)
        again = ops.frame_change(x.to(cuda))      # the layouts agree, and `hwc` is inferred
        assert torch.equal(again[0], hist) and torch.equal(again[1], sad)


@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_frame_change_takes_a_source_at_any_alignment(cuda, shift, hwc):
    shape = (3, 64, 96, 3) if hwc else (3, 3, 64, 96)
    x = _frames(shape, seed=40 + shift)
    raw = torch.empty(x.numel() + 64, dtype=torch.uint8, device=cuda)
    base = (-raw.data_ptr()) % 16 + shift
    view = raw[base:base + x.numel()].view(shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == shift
    _check(view, x, hwc)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("f,h,w", [(9, 67, 131), (20, 67, 131), (17, 64, 96)])
def test_frame_change_across_runs_of_frames(cuda, f, h, w, hwc, shift):
    """More than 8 frames are cut into several runs (gridDim.y), and a run that does not start at frame 0 reloads the frame before it
    for the pair that straddles the two runs: F = 9 is runs of 5 + 4, F = 20 of 7 + 7 + 6, F = 17 of 6 + 6 + 5 -- ragged last runs,
    three pixel blocks with a 9-pixel tail (67 x 131) or two full ones (64 x 96), both layouts, the base on and 3 bytes past a
    16-byte boundary.  Every `sad`, the straddling pairs included, and every histogram against the oracle."""
    shape = (f, h, w, 3) if hwc else (f, 3, h, w)
    x = _frames(shape, seed=100 * f + shift)
    raw = torch.empty(x.numel() + 64, dtype=torch.uint8, device=cuda)
    base = (-raw.data_ptr()) % 16 + shift
    view = raw[base:base + x.numel()].view(shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == shift
    _, sad = _check(view, x, hwc)
    assert int(sad.min()) > 0      # random frames: a pair the kernel skipped would read 0


def test_scene_changes_with_the_default_chunk(cuda):
    """the default chunk of 64 frames: every call inside is cut into runs; 70 frames from the host are two uploads (64 + 6 behind the
    carried frame), 13 frames on the device one call -- against the oracle on the whole clip"""
    from eavsr_amd import harness
    x = _frames((70, 3, 33, 50), seed=13)
    want_hist, want_sad = (torch.from_numpy(v) for v in R.frame_change(x.numpy()))
    for src, k in ((x, 70), (x.to(cuda), 70), (x[:13].to(cuda), 13), (x[:13].permute(0, 2, 3, 1).contiguous(), 13)):
        hist, sad = harness.scene_changes(src, device=cuda)
        assert torch.equal(hist.cpu(), want_hist[:k]) and torch.equal(sad.cpu(), want_sad[:k - 1]), (src.device, tuple(src.shape))


def test_frame_change_on_constant_frames_and_single_bins(cuda):
    zeros = torch.zeros((2, 3, 67, 131), dtype=torch.uint8)
    hist, sad = _check(zeros.to(cuda), zeros, False)
    assert hist[:, 0].tolist() == [67 * 131] * 2 and sad.tolist() == [0]
    full = torch.full((2, 67, 131, 3), 255, dtype=torch.uint8)
    hist, sad = _check(full.to(cuda), full, True)
    assert hist[:, 63].tolist() == [67 * 131] * 2 and sad.tolist() == [0]
    # every pixel of a frame in ONE bin (the lumas 100 .. 103 are bin 25), from samples that differ: the worst case for the LDS atomics
    one_bin = _frames((3, 1, 64, 96), seed=7) % 4 + 100
    hist, _ = _check(one_bin.to(cuda), one_bin, False)
    assert hist[:, 25].tolist() == [64 * 96] * 3
    both = torch.cat([zeros[:1], torch.full((1, 3, 67, 131), 255, dtype=torch.uint8), zeros[:1]], 0)
    _, sad = _check(both.to(cuda), both, False)
    assert sad.tolist() == [255 * 67 * 131] * 2


def test_frame_change_twice_is_bit_identical_and_refuses_bad_input(cuda):
    from eavsr_amd import ops
    x = _frames((5, 3, 67, 131), seed=9).to(cuda)
    a, b = ops.frame_change(x), ops.frame_change(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for bad in (x.float(), x[0], x[:, :2], x[:0]):
        with pytest.raises(ValueError):
            ops.frame_change(bad)
    with pytest.raises(ValueError):
        ops.frame_change(x, hwc=True)      # (5, 3, 67, 131) is not interleaved
    with pytest.raises(RuntimeError):
        ops.frame_change(x.cpu())


def test_sad_is_64_bits_wide_end_to_end(cuda):
    """2 x 1 x 4112 x 4112: frame 0 all zeros, frame 1 all 255.  255 x 4112^2 = 4,311,638,720 > 2^32: a signed or an unsigned 32-bit
    accumulator anywhere on the way shows"""
    from eavsr_amd import ops
    x = torch.zeros((2, 1, 4112, 4112), dtype=torch.uint8, device=cuda)
    x[1].fill_(255)
    hist, sad = ops.frame_change(x)
    assert 255 * 4112 * 4112 > 2 ** 32
    assert sad.tolist() == [255 * 4112 * 4112]
    assert int(hist[1, 63]) == 4112 * 4112 and int(hist[0, 0]) == 4112 * 4112 and int(hist.sum()) == 2 * 4112 * 4112


@pytest.mark.parametrize("chunk", [1, 2, 3])
def test_scene_changes_in_chunks_equals_one_call(cuda, chunk):
    from eavsr_amd import harness, ops
    x = _frames((7, 3, 67, 131), seed=11)
    want = ops.frame_change(x.to(cuda))
    for src in (x, x.pin_memory(), x.to(cuda), x.permute(0, 2, 3, 1).contiguous()):
        hist, sad = harness.scene_changes(src, chunk=chunk, device=cuda)
        assert hist.is_cuda and torch.equal(hist, want[0]) and torch.equal(sad, want[1]), (src.device, tuple(src.shape))
    clips = torch.stack([x, x.flip(0)], 0)      # (n, t, ...): per clip
    hist, sad = harness.scene_changes(clips, chunk=chunk, device=cuda)
    assert tuple(hist.shape) == (2, 7, 64) and tuple(sad.shape) == (2, 6)
    assert torch.equal(hist[0], want[0]) and torch.equal(hist[1], want[0].flip(0)) and torch.equal(sad[1], want[1].flip(0))


def _two_scene_clip():
    """1 x 12 x 3 x 64 x 96 uint8: frames 0-6 hold bytes in 0 .. 127, frames 7-11 bytes in 128 .. 255; each frame is its predecessor
    rolled by one pixel with wrap-around.  The lumas of a scene are then a permutation of its first frame's: histogram distance
    exactly 0 inside a scene; across the cut the lumas move from bins 0 .. 31 to bins 32 .. 63: distance exactly 1, and every
    pixel changes by at least 1 (a luma below 128 against one of at least 128)"""
    g = np.random.default_rng(21)
    a = g.integers(0, 128, size=(3, 64, 96), dtype=np.uint8)
    b = g.integers(128, 256, size=(3, 64, 96), dtype=np.uint8)
    frames = [np.roll(a, k, axis=2) for k in range(7)] + [np.roll(b, k, axis=2) for k in range(5)]
    return torch.from_numpy(np.stack(frames)).unsqueeze(0)


def test_detection_end_to_end(cuda):
    from eavsr_amd import harness
    from eavsr_amd.segments import find_cuts, plan_segments
    clip = _two_scene_clip()
    hist, sad = harness.scene_changes(clip[0], device=cuda)
    pixels = 64 * 96
    d = (hist[1:] - hist[:-1]).abs().sum(1).tolist()
    assert d == [0] * 6 + [2 * pixels] + [0] * 4
    assert int(sad[6]) >= pixels
    assert find_cuts(hist, sad, pixels, 0.5, 1.0) == [7]
    assert plan_segments(12, find_cuts(hist, sad, pixels, 0.5, 1.0)) == [(0, 7, 0, 7), (7, 12, 7, 12)]


# ------------------------------------------------------------------------------------------------------------- the segmented forward
@functools.lru_cache(maxsize=None)
def _net():
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)      # the model tests/test_hip_longclip.py builds
    net.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    return net.to("cuda:0").eval()


@functools.lru_cache(maxsize=None)
def _clip(t, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    return synthetic_clip(1, t, 64, 96, seed=seed).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _whole(t, seed, frame_chunk):
    """forward_long on the whole clip: computed once, shared, never written to"""
    with torch.no_grad():
        return _net().forward_long(_clip(t, seed), frame_chunk=frame_chunk)


@pytest.mark.parametrize("frame_chunk", [None, 2])
@pytest.mark.parametrize("emit", [(0, 9), (2, 7), (8, 9)])
def test_forward_long_emit_is_a_slice_of_the_whole_run(cuda, frame_chunk, emit):
    net, clip, want = _net(), _clip(9, 31), _whole(9, 31, frame_chunk)
    a, b = emit
    with torch.no_grad():
        got = net.forward_long(clip, frame_chunk=frame_chunk, emit=emit)
        seen = []
        assert net.forward_long(clip, frame_chunk=frame_chunk, emit=emit, sink=lambda first, sr: seen.append((first, sr))) is None
    assert tuple(got.shape) == (1, b - a, 3, 256, 384) and torch.equal(got, want[:, a:b])
    # the sink: `first` counted from the start of the clip passed in, the chunks' parts inside [a, b) in order
    step = 9 if frame_chunk is None else frame_chunk
    parts = [(max(lo, a), min(lo + step, 9, b)) for lo in range(0, 9, step) if max(lo, a) < min(lo + step, 9, b)]
    assert [(first, first + int(sr.shape[1])) for first, sr in seen] == parts
    assert torch.equal(torch.cat([sr for _, sr in seen], 1), want[:, a:b])
    for bad in ((3, 3), (-1, 2), (0, 10), (5, 4)):
        with pytest.raises(ValueError), torch.no_grad():
            net.forward_long(clip, emit=bad)


def test_forward_long_takes_a_single_frame(cuda):
    """segments.MIN_SCENE_FLOOR: the shortest clip `forward_long` takes is one frame"""
    from eavsr_amd.segments import MIN_SCENE_FLOOR
    assert MIN_SCENE_FLOOR == 1
    with torch.no_grad():
        one = _net().forward_long(_clip(9, 31)[:, :1])
    assert tuple(one.shape) == (1, 1, 3, 256, 384) and bool(torch.isfinite(one).all())


def test_forward_segments_gives_each_frame_of_its_window(cuda):
    from eavsr_amd.segments import plan_segments
    net, clip = _net(), _clip(11, 33)
    plan = plan_segments(11, [], 5, 2)
    assert plan == [(0, 5, 0, 4), (3, 8, 4, 7), (6, 11, 7, 11)]
    seen = []
    with torch.no_grad():
        got = net.forward_segments(clip, plan)
        assert net.forward_segments(clip, plan, frame_chunk=2, sink=lambda first, sr: seen.append((first, sr))) is None
        for a, b, ea, eb in plan:
            window = net.forward_long(clip[:, a:b])
            assert torch.equal(got[:, ea:eb], window[:, ea - a:eb - a]), (a, b, ea, eb)
    assert tuple(got.shape) == (1, 11, 3, 256, 384)
    # the sink: global frame numbers, increasing, every frame once; chunked stages change no bit
    at = 0
    for first, sr in seen:
        assert first == at
        at += int(sr.shape[1])
    assert at == 11 and torch.equal(torch.cat([sr for _, sr in seen], 1), got)
    # the windows matter: a frame next to a window end differs from the whole clip's
    assert not torch.equal(got, _whole(11, 33, None))
    with torch.no_grad():
        assert torch.equal(net.forward_segments(clip, plan_segments(11, [])), _whole(11, 33, None))      # one window = forward_long
    with pytest.raises(ValueError), torch.no_grad():
        net.forward_segments(clip, [(0, 5, 0, 4), (3, 11, 5, 11)])


def test_a_cut_isolates_the_scenes(cuda):
    from eavsr_amd import harness
    net = _net()
    clip = _two_scene_clip()
    with torch.no_grad():
        first_scene = net.forward_long(clip[:, :7].to(cuda))
        whole = net.forward_long(clip.to(cuda))
    # super_resolve with an explicit cut plans two windows; the fp32 frames of that plan through forward_segments
    res = harness.super_resolve(net, clip, cuts=[7])
    assert res["segments"] == [(0, 7, 0, 7), (7, 12, 7, 12)] and res["scene_starts"] == [7]
    with torch.no_grad():
        got = net.forward_segments(clip.to(cuda), res["segments"])
    assert torch.equal(got[:, :7], first_scene)
    assert not torch.equal(got[:, :7], whole[:, :7])
    # and detection on the device finds that plan
    res = harness.super_resolve(net, clip, cuts="device", cut_thresholds=(0.5, 1.0))
    assert res["segments"] == [(0, 7, 0, 7), (7, 12, 7, 12)] and res["scene_starts"] == [7]


def test_super_resolve_segmented_writes_reports_and_defaults_to_todays_path(cuda, tmp_path):
    from eavsr_amd import harness, ops
    from eavsr_amd.segments import plan_segments
    net = _net()
    lr = _clip(11, 33)
    hr = torch.nn.functional.interpolate(lr[0], scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    names = ["%03d_%05d.png" % (i // 6, i) for i in range(11)]
    plan = plan_segments(11, [], 5, 2)
    with torch.no_grad():
        want = ops.rgb8(net.forward_segments(lr, plan)[0], 255.0).cpu()
    res = harness.super_resolve(net, lr[0], out_dir=str(tmp_path / "seg"), hr=hr, names=names, max_frames=5, overlap=2)
    assert res["segments"] == plan and res["scene_starts"] == [] and res["frames"] == 11
    assert res["written"] == [str(tmp_path / "seg" / name) for name in names]
    for i, path in enumerate(res["written"]):
        assert torch.equal(harness.read_png(path), want[i].permute(2, 0, 1)), i
    assert res["frame_names"] == names and len(res["frame_psnr"]) == len(res["frame_ssim"]) == 11
    with torch.no_grad():
        sse, _, _ = ops.frame_metrics(net.forward_segments(lr, plan)[0], hr, 255.0)
    assert res["frame_psnr"] == [harness.psnr_from_sse(v, 3 * 256 * 384) for v in sse.tolist()]      # one entry per frame, in order
    # max_frames=None, cuts=None: the call without the new arguments, byte for byte
    plain = harness.super_resolve(net, lr[0], out_dir=str(tmp_path / "plain"), names=names, frame_chunk=4)
    same = harness.super_resolve(net, lr[0], out_dir=str(tmp_path / "same"), names=names, frame_chunk=4, max_frames=None, cuts=None)
    assert same["segments"] == plain["segments"] == [(0, 11, 0, 11)] and same["scene_starts"] == []
    for p, q in zip(plain["written"], same["written"]):
        assert open(p, "rb").read() == open(q, "rb").read()
    # cuts="device" reads one clip of 8-bit frames
    u8 = (lr * 255).round().to(torch.uint8)
    with pytest.raises(ValueError):
        harness.super_resolve(net, torch.cat([u8, u8], 0), cuts="device")
    with pytest.raises(ValueError):
        harness.super_resolve(net, lr, cuts="device")      # fp32 frames
    with pytest.raises(ValueError):
        harness.super_resolve(net, u8, cuts="host")
    with pytest.raises(ValueError):
        harness.super_resolve(net, u8, max_frames=4, overlap=4)
    with pytest.raises(ValueError):
        harness.super_resolve(net, u8, cuts="device", max_frames=4, overlap=4)      # refused before detection runs
    with pytest.raises(ValueError):
        harness.super_resolve(net, u8, cuts="device", min_scene=0)


def test_a_window_bound_from_the_environment_alone_is_taken(cuda, monkeypatch):
    """EAVSR_MAX_FRAMES=8 without an overlap beside it: the default overlap of 8 would be refused (overlap < max_frames), so the
    option path takes min(8, max_frames // 2); explicit arguments still hold as given"""
    from eavsr_amd import harness
    from eavsr_amd.segments import plan_segments
    net, lr = _net(), _clip(11, 33)
    monkeypatch.setenv("EAVSR_MAX_FRAMES", "8")
    assert harness.super_resolve(net, lr)["segments"] == plan_segments(11, [], 8, 4)
    monkeypatch.setenv("EAVSR_SEGMENT_OVERLAP", "2")
    assert harness.super_resolve(net, lr)["segments"] == plan_segments(11, [], 8, 2)
    assert harness.super_resolve(net, lr, max_frames=5, overlap=1)["segments"] == plan_segments(11, [], 5, 1)


def test_segments_bound_the_peak_memory(cuda):
    """1 x 24 x 3 x 64 x 96, whole against max_frames=6, overlap=2, in one test: the frame store grows with t, so the segmented run's
    peak is strictly below the whole run's -- no margin"""
    from eavsr_amd import harness
    net = _net()
    lr = _clip(24, 35)
    harness.super_resolve(net, lr[:, :6])      # warm-up: packed weights and workspaces exist before either run is measured
    whole = harness.super_resolve(net, lr)
    seg = harness.super_resolve(net, lr, max_frames=6, overlap=2)
    print(f"peak_bytes: whole {whole['peak_bytes']}, max_frames=6 {seg['peak_bytes']}")
    assert len(seg["segments"]) == 6 and max(b - a for a, b, _, _ in seg["segments"]) == 6
    assert seg["peak_bytes"] < whole["peak_bytes"]
