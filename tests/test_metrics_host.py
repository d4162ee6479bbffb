"""Host side of the per-frame PSNR / SSIM report (no GPU): argument errors of the new entry points, the workspace helper, the
scene averaging of psnr_total.py:89-133, the log's rounding and the interleaved-uint8 path of the PNG writer."""
import math
import os

import pytest
import torch

from eavsr_amd import _native, harness


def test_argument_errors_and_their_messages():
    lib = _native.load()
    # NULL pointers: -1 (the integers stand for device pointers; nothing is launched on an argument error)
    assert lib.eavsr_frame_metrics_f32(None, 16, 255.0, 1, 3, 16, 16, 16, 16, 16, None, None) == -1
    assert b"NULL" in lib.eavsr_last_error()
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 3, 16, 16, None, 16, 16, None, None) == -1
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 3, 16, 16, 16, None, 16, None, None) == -1
    assert lib.eavsr_rgb8_f32(None, 255.0, 1, 3, 16, 16, 16, None) == -1
    assert b"NULL" in lib.eavsr_last_error()
    assert lib.eavsr_rgb8_f32(16, 255.0, 1, 3, 16, 16, None, None) == -1
    # a frame smaller than the window, a plane count that is neither grey nor RGB: -2
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 3, 10, 64, 16, 16, 16, None, None) == -2
    assert b"11-tap window" in lib.eavsr_last_error()
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 3, 64, 10, 16, 16, 16, None, None) == -2
    assert b"11-tap window" in lib.eavsr_last_error()
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 2, 64, 64, 16, 16, 16, None, None) == -2
    assert b"C=2" in lib.eavsr_last_error()
    assert lib.eavsr_frame_metrics_f32(16, 16, 255.0, 1, 4, 64, 64, 16, 16, 16, None, None) == -2
    assert lib.eavsr_rgb8_f32(16, 255.0, 1, 2, 16, 16, 16, None) == -2
    assert b"C=2" in lib.eavsr_last_error()
    assert lib.eavsr_frame_metrics_partials(1, 3, 10, 64) == -2
    assert lib.eavsr_frame_metrics_partials(1, 5, 64, 64) == -2


def test_partials_are_positive_and_grow_with_the_frame():
    lib = _native.load()
    sizes = [(11, 11), (37, 53), (64, 96), (180, 320), (720, 1280), (2160, 3840)]
    counts = [lib.eavsr_frame_metrics_partials(7, 3, h, w) for h, w in sizes]
    assert counts[0] == 1 and all(c > 0 for c in counts)
    assert counts == sorted(counts) and counts[-1] > counts[-2] > counts[-3] > counts[0]
    # per frame: neither the frame count nor the plane count changes it
    assert lib.eavsr_frame_metrics_partials(1, 1, 720, 1280) == counts[4]
    # every valid output belongs to one workgroup's tile
    for (h, w), c in zip(sizes, counts):
        assert c * 64 * 32 >= (h - 10) * (w - 10)


def test_ops_wrappers_refuse_cpu_tensors():
    from eavsr_amd import ops
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.frame_metrics(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rgb8(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        harness.frame_metrics(x[None], x[None])


def test_psnr_from_sse():
    assert harness.psnr_from_sse(0, 3 * 16 * 16) == math.inf
    # every sample off by one: mse = 1 / 255^2
    assert harness.psnr_from_sse(768, 768) == pytest.approx(20 * math.log10(255.0), abs=1e-12)


def test_scene_report_is_the_mean_of_scene_means():
    names = ["000_00000.png", "000_00001.png", "000_00002.png", "001_00000.png"]
    psnr = [30.0, 32.0, 34.0, 20.0]
    ssim = [0.9, 0.8, 0.7, 0.5]
    rep = harness.scene_report(names, psnr, ssim)
    assert [f["name"] for f in rep["frames"]] == names and [f["scene"] for f in rep["frames"]] == ["000", "000", "000", "001"]
    assert list(rep["scenes"]) == ["000", "001"]
    assert rep["scenes"]["000"]["frames"] == 3 and rep["scenes"]["001"]["frames"] == 1
    assert rep["scenes"]["000"]["psnr"] == pytest.approx(32.0) and rep["scenes"]["000"]["ssim"] == pytest.approx(0.8)
    assert rep["scenes"]["001"]["psnr"] == 20.0 and rep["scenes"]["001"]["ssim"] == 0.5
    # two scenes of unequal length: (32 + 20) / 2, not (30 + 32 + 34 + 20) / 4 = 29
    assert rep["final"]["psnr"] == pytest.approx(26.0) and rep["final"]["ssim"] == pytest.approx(0.65)
    assert rep["final"]["scenes"] == 2
    # the order the frames arrive in does not matter, scenes come out sorted
    order = [3, 1, 0, 2]
    rep2 = harness.scene_report([names[i] for i in order], [psnr[i] for i in order], [ssim[i] for i in order])
    assert list(rep2["scenes"]) == ["000", "001"] and rep2["final"]["psnr"] == pytest.approx(26.0)
    # identical frames score inf, and a mean over them stays inf
    assert harness.scene_report(["000_a", "000_b"], [math.inf, 30.0], [1.0, 0.9])["final"]["psnr"] == math.inf
    with pytest.raises(ValueError):
        harness.scene_report(names, psnr[:3], ssim)


def test_write_metrics_log_rounds_psnr_to_2_and_ssim_to_4_decimals(tmp_path):
    rep = harness.scene_report(["000_00000.png", "000_00001.png", "001_00000.png"], [31.23456, 33.33333, 28.005001],
                               [0.912345, 0.87656, 0.99996])
    path = harness.write_metrics_log(rep, str(tmp_path / "logs" / "log_patch_0.txt"))
    text = open(path).read()
    lines = text.splitlines()
    assert lines == [
        "scene 000",
        "  000_00000.png  psnr 31.23  ssim 0.9123",
        "  000_00001.png  psnr 33.33  ssim 0.8766",
        "  mean of 2 frames  psnr 32.28  ssim 0.8945",
        "scene 001",
        "  001_00000.png  psnr 28.01  ssim 1.0000",
        "  mean of 1 frames  psnr 28.01  ssim 1.0000",
        "final, mean of 2 scenes  psnr 30.14  ssim 0.9472",
    ]
    assert text.endswith("\n") and "lpips" not in text.lower()


@pytest.mark.parametrize("c", [3, 1])
def test_write_png_interleaved_uint8_path_writes_the_float_paths_file(tmp_path, c):
    g = torch.Generator().manual_seed(11)
    img = torch.randint(0, 256, (c, 37, 53), generator=g).float()      # a get_current_visuals() frame
    a = harness.write_png(img, str(tmp_path / "float.png"))
    hwc = img.to(torch.uint8).permute(1, 2, 0).contiguous()
    assert hwc.shape == (37, 53, c)
    b = harness.write_png(hwc, str(tmp_path / "u8.png"))
    assert open(a, "rb").read() == open(b, "rb").read()
    assert torch.equal(harness.read_png(b), img.to(torch.uint8))
    # the explicit form, and what it refuses
    b2 = harness.write_png(hwc, str(tmp_path / "u8b.png"), hwc=True)
    assert open(b2, "rb").read() == open(a, "rb").read()
    with pytest.raises(ValueError):
        harness.write_png(hwc.float(), str(tmp_path / "bad.png"), hwc=True)
    # a uint8 planar image is still read as planes
    p = harness.write_png(img.to(torch.uint8), str(tmp_path / "planes.png"))
    assert open(p, "rb").read() == open(a, "rb").read()


def test_save_frames_rgb8_paths(tmp_path):
    frames = torch.randint(0, 256, (2, 12, 14, 3), generator=torch.Generator().manual_seed(3)).to(torch.uint8)
    paths = harness.save_frames_rgb8(frames, [["000_00000.png"], "001_00007.png"], str(tmp_path), load_iter="5")
    assert paths == [os.path.join(str(tmp_path), "sr_patch_5", "000", "00000.png"),
                     os.path.join(str(tmp_path), "sr_patch_5", "001", "00007.png")]
    for i, p in enumerate(paths):
        assert torch.equal(harness.read_png(p), frames[i].permute(2, 0, 1))
    with pytest.raises(ValueError):
        harness.save_frames_rgb8(frames, "x", str(tmp_path))
