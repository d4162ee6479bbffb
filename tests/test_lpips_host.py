"""LPIPS (AlexNet) without a GPU: properties of the float64 restatement the GPU tests compare with (tests/lpips_ref.py), the two
weight-file layouts of `eavsr_amd.lpips.load_lpips_weights` and their strictness, and the report's third column."""
import math

import pytest
import torch

from tests import lpips_ref as R


def test_restatement_is_zero_on_identical_images_symmetric_and_non_negative():
    sd = R.synthetic_weights(0)
    sr, hr = R.image_pair(2, 48, 61, seed=1)
    assert torch.equal(R.lpips(hr, hr.clone(), sd), torch.zeros(2, dtype=torch.float64))
    a, b = R.lpips(sr, hr, sd), R.lpips(hr, sr, sd)
    assert a.dtype == torch.float64 and tuple(a.shape) == (2,)
    assert torch.equal(a, b)
    assert (a > 0).all() and (a < 2.0).all()
    # ReLU kills a real share of the activations and the lin weights have exact zeros, as the maker promises
    feats = R.features(hr, sd)
    for f in feats:
        dead = (f == 0).double().mean().item()
        assert 0.05 < dead < 0.95, dead
    for i in range(5):
        w = sd[f"lin{i}.model.1.weight"]
        assert (w >= 0).all() and (w == 0).any() and (w > 0).any()
    # tap sizes of the issue's table
    sizes = [tuple(t.shape[1:]) for t in R.features(torch.zeros(1, 3, 720, 1280), sd, dtype=torch.float32)]
    assert sizes == [(64, 179, 319), (192, 89, 159), (384, 44, 79), (256, 44, 79), (256, 44, 79)]


def test_restatement_sees_the_quantised_images_only():
    sd = R.synthetic_weights(0)
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 256, (1, 3, 40, 40), generator=g).float()
    a = (q + 0.3) / 255.0
    b = (q - 0.3) / 255.0
    assert not torch.equal(a, b) and torch.equal(R.quantise(a, 255.0), R.quantise(b, 255.0))
    assert torch.equal(R.lpips(a, b, sd), torch.zeros(1, dtype=torch.float64))
    # scale 1 on the visuals is the same number as scale 255 on the [0, 1] tensors
    sr, hr = R.image_pair(1, 40, 40, seed=2)
    assert torch.equal(R.lpips(sr, hr, sd), R.lpips(R.quantise(sr, 255.0), R.quantise(hr, 255.0), sd, scale=1.0))
    # half to even: 0.5 -> 0, 1.5 -> 2
    assert R.quantise(torch.tensor([0.5, 1.5, 2.5, -3.0, 300.0]), 1.0).tolist() == [0.0, 2.0, 2.0, 0.0, 255.0]


def test_frames_smaller_than_31_pixels_raise():
    sd = R.synthetic_weights(0)
    with pytest.raises(ValueError, match="31"):
        R.lpips(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64), sd)
    assert R.lpips(torch.zeros(1, 3, 31, 31), torch.zeros(1, 3, 31, 31), sd).item() == 0.0
    from eavsr_amd.lpips import LPIPSAlex
    net = LPIPSAlex()
    with pytest.raises(RuntimeError, match="GPU only"):
        net(torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 64, 64))


def _pair_files(sd, tmp_path):
    """the pair the packages distribute: torchvision's AlexNet state dict and the lpips lin file"""
    alex = {}
    for key, *_ in R.LAYERS:
        idx = key.rsplit(".", 1)[1]
        alex[f"features.{idx}.weight"] = sd[key + ".weight"]
        alex[f"features.{idx}.bias"] = sd[key + ".bias"]
    alex["classifier.1.weight"] = torch.zeros(8, 8)
    alex["classifier.1.bias"] = torch.zeros(8)
    lins = {f"lin{i}.model.1.weight": sd[f"lin{i}.model.1.weight"] for i in range(5)}
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")
    torch.save(alex, pa)
    torch.save(lins, pl)
    return pl, pa, lins, alex


def test_both_weight_layouts_load_into_identical_parameters(tmp_path):
    from eavsr_amd.lpips import LPIPSAlex, load_lpips_weights
    sd = R.synthetic_weights(5)
    net = LPIPSAlex()
    assert set(net.state_dict()) == set(sd)
    assert all(tuple(v.shape) == tuple(sd[k].shape) for k, v in net.state_dict().items())
    assert not any(p.requires_grad for p in net.parameters()) and not net.training
    # the single file, with the package's `lins` aliases in it
    single = dict(sd)
    for i in range(5):
        single[f"lins.{i}.model.1.weight"] = sd[f"lin{i}.model.1.weight"]
    p1 = str(tmp_path / "lpips_alex_full.pth")
    torch.save(single, p1)
    one = load_lpips_weights(LPIPSAlex(), p1)
    pl, pa, _, _ = _pair_files(sd, tmp_path)
    two = load_lpips_weights(LPIPSAlex(), pl, alexnet_path=pa)
    a, b = one.state_dict(), two.state_dict()
    assert set(a) == set(b) == set(sd)
    for k in sd:
        assert torch.equal(a[k], sd[k]), k
        assert torch.equal(b[k], sd[k]), k


def test_weight_files_are_checked_as_strictly_as_checkpoints(tmp_path):
    from eavsr_amd.lpips import LPIPSAlex, load_lpips_weights
    sd = R.synthetic_weights(5)
    save = lambda d, name: (torch.save(d, str(tmp_path / name)), str(tmp_path / name))[1]
    # single file: unknown key, missing key, wrong shape
    with pytest.raises(RuntimeError, match=r"net\.slice9\.0\.weight"):
        load_lpips_weights(LPIPSAlex(), save({**sd, "net.slice9.0.weight": torch.zeros(1)}, "a.pth"))
    with pytest.raises(RuntimeError, match=r"net\.slice3\.6\.bias"):
        load_lpips_weights(LPIPSAlex(), save({k: v for k, v in sd.items() if k != "net.slice3.6.bias"}, "b.pth"))
    with pytest.raises(RuntimeError, match=r"lin2\.model\.1\.weight"):
        load_lpips_weights(LPIPSAlex(), save({**sd, "lin2.model.1.weight": torch.zeros(1, 383, 1, 1)}, "c.pth"))
    # the pair
    pl, pa, lins, alex = _pair_files(sd, tmp_path)
    with pytest.raises(RuntimeError, match=r"features\.12\.weight"):
        load_lpips_weights(LPIPSAlex(), pl, save({**alex, "features.12.weight": torch.zeros(1)}, "d.pth"))
    with pytest.raises(RuntimeError, match=r"net\.slice2\.3\.weight"):
        load_lpips_weights(LPIPSAlex(), pl, save({k: v for k, v in alex.items() if k != "features.3.weight"}, "e.pth"))
    with pytest.raises(RuntimeError, match=r"net\.slice1\.0\.weight"):
        load_lpips_weights(LPIPSAlex(), pl, save({**alex, "features.0.weight": torch.zeros(64, 3, 7, 7)}, "f.pth"))
    with pytest.raises(RuntimeError, match=r"net\.slice1\.0\.weight"):      # a full state dict is not the lin file
        load_lpips_weights(LPIPSAlex(), save(sd, "g.pth"), pa)
    with pytest.raises(RuntimeError, match=r"lin4\.model\.1\.weight"):
        load_lpips_weights(LPIPSAlex(), save({k: v for k, v in lins.items() if k != "lin4.model.1.weight"}, "h.pth"), pa)
    with pytest.raises(FileNotFoundError):
        load_lpips_weights(LPIPSAlex(), str(tmp_path / "nothing.pth"))


def test_report_and_log_carry_the_third_column(tmp_path):
    from eavsr_amd import harness
    names = ["000_00000.png", "000_00001.png", "000_00002.png", "001_00000.png"]
    psnr, ssim, lp = [30.0, 31.0, 32.0, 20.0], [0.9, 0.8, 0.7, 0.5], [0.1, 0.2, 0.3, 0.5004]
    rep = harness.scene_report(names, psnr, ssim, lp)
    assert [fr["lpips"] for fr in rep["frames"]] == lp
    assert rep["scenes"]["000"]["lpips"] == pytest.approx(0.2, abs=1e-15) and rep["scenes"]["001"]["lpips"] == 0.5004
    # the mean of the scene means, not of the frames
    assert rep["final"]["lpips"] == pytest.approx((0.2 + 0.5004) / 2, abs=1e-15)
    assert rep["final"]["lpips"] != pytest.approx(sum(lp) / 4, abs=1e-6)
    assert rep["final"]["psnr"] == pytest.approx((31.0 + 20.0) / 2)
    text = open(harness.write_metrics_log(rep, str(tmp_path / "with.txt"))).read().splitlines()
    assert text[1] == "  000_00000.png  psnr 30.00  ssim 0.9000  lpips 0.100"
    assert text[4] == "  mean of 3 frames  psnr 31.00  ssim 0.8000  lpips 0.200"
    assert text[-1] == "final, mean of 2 scenes  psnr 25.50  ssim 0.6500  lpips 0.350"
    assert all("lpips" in ln for ln in text if not ln.startswith("scene "))
    # without LPIPS: no field anywhere, and the file of old, byte for byte
    plain = harness.scene_report(names, psnr, ssim)
    assert "lpips" not in plain["final"] and all("lpips" not in fr for fr in plain["frames"])
    assert all("lpips" not in v for v in plain["scenes"].values())
    old = open(harness.write_metrics_log(plain, str(tmp_path / "without.txt"))).read()
    assert "lpips" not in old
    assert old.splitlines() == [ln.split("  lpips ")[0] for ln in text]
    with pytest.raises(ValueError):
        harness.scene_report(names, psnr, ssim, lp[:3])
    assert math.isnan(harness.scene_report([], [], [], [])["final"]["lpips"])


def test_evaluate_refuses_lpips_without_the_per_frame_report():
    from eavsr_amd import harness
    with pytest.raises(ValueError, match="per_frame"):
        harness.evaluate(object(), [], lpips="weights.pth")
