"""PWC-Net of the late-training mask, host side (no GPU): the CPU restatement against the reference's fixtures, the cost volume
by known answers, the module tree's keys and the weight-file reader."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import pwc_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["x2_64", "x4_72x88"]
REFINER_PUSH = (0.12, -0.08)      # tests/golden/gen_golden_pwc.py


def pwc_weights():
    """the synthetic weights the fixtures were made with (tests/golden/gen_golden_pwc.py)"""
    from eavsr_amd.pwc import PWCNET
    from eavsr_amd.utils.synthetic import fill_state_dict
    shapes = {k: tuple(v.shape) for k, v in PWCNET().state_dict().items()}
    sd = fill_state_dict(shapes, "default", seed=7)
    sd["netRefiner.netMain.12.bias"] = sd["netRefiner.netMain.12.bias"] + torch.tensor(REFINER_PUSH)
    return sd


def load_case(name):
    z = dict(np.load(os.path.join(GOLDEN, f"pwc_{name}.npz")))
    z.update(np.load(os.path.join(GOLDEN, f"pwc_{name}.part1.npz")))
    lr = torch.from_numpy(z["lr"]).float() / 255.0
    hr = torch.from_numpy(z["hr"]).float() / 255.0
    return lr, hr, int(z["scale"]), z


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference_fixtures(name):
    lr, hr, scale, z = load_case(name)
    hr_align, mask, ones, flow = pwc_ref.get_backwarp(pwc_weights(), lr, hr, scale)
    assert float((flow - torch.from_numpy(z["flow"])).abs().max()) <= 1e-5
    assert torch.equal(mask, torch.from_numpy(z["mask"]).float())
    assert 0 < float(mask.mean()) < 1
    assert float((ones - torch.from_numpy(z["ones"])).abs().max()) <= 1e-5
    assert float((hr_align - torch.from_numpy(z["hr_align"]).float()).abs().max()) <= 1e-3


@pytest.mark.parametrize("c", [1, 32, 196])
def test_correlation_known_answers(c):
    h, w = 11, 13
    for (y, x, dy, dx) in [(5, 6, 0, 0), (5, 6, -4, 3), (0, 0, 4, 4), (10, 12, -4, -4), (3, 2, 2, -1)]:
        a = torch.zeros(1, c, h, w)
        b = torch.zeros(1, c, h, w)
        ch = c // 2
        a[0, ch, y, x] = 1.0
        b[0, ch, y + dy, x + dx] = 3.0
        out = pwc_ref.correlation(a, b)
        expect = torch.zeros(1, 81, h, w)
        expect[0, (dy + 4) * 9 + (dx + 4), y, x] = 3.0 / c
        assert torch.allclose(out, expect, rtol=0, atol=1e-7), (y, x, dy, dx)
    # beyond +-4 and outside the image: nothing
    a = torch.zeros(1, c, h, w)
    b = torch.zeros(1, c, h, w)
    a[0, 0, 5, 5] = 1.0
    b[0, 0, 5, 10] = 2.0        # dx = 5
    b[0, 0, 0, 0] = 2.0         # dy = dx = -5
    assert float(pwc_ref.correlation(a, b).abs().max()) == 0.0
    a = torch.zeros(1, c, h, w)
    a[0, 0, 0, 0] = 1.0
    b = torch.ones(1, c, h, w)
    out = pwc_ref.correlation(a, b)[0, :, 0, 0].view(9, 9)
    assert float(out[:4].abs().max()) == 0.0 and float(out[:, :4].abs().max()) == 0.0     # dy < 0 or dx < 0: off the image
    assert torch.allclose(out[4:, 4:], torch.full((5, 5), 1.0 / c))


def test_module_tree_keys_equal_the_reference():
    from eavsr_amd.pwc import PWCNET
    with open(os.path.join(GOLDEN, "pwc_keys.json")) as f:
        keys = json.load(f)
    assert list(PWCNET().state_dict().keys()) == keys
    assert "netRefiner.netMain.12.bias" in keys and "netExtractor.netOne.0.weight" in keys


def test_load_pwc_weights_renames_module_to_net(tmp_path):
    from eavsr_amd.pwc import load_pwc_weights

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.netMain = nn.Sequential(nn.Conv2d(2, 3, 3))
            self.netOther = nn.Linear(4, 2)

    src = Tiny()
    for p in src.parameters():
        nn.init.uniform_(p)
    sniklaus = {k.replace("net", "module"): v for k, v in src.state_dict().items()}
    assert "moduleMain.0.weight" in sniklaus
    path = str(tmp_path / "pwc-tiny")
    torch.save(sniklaus, path)
    got = load_pwc_weights(Tiny(), path)
    for k, v in src.state_dict().items():
        assert torch.equal(got.state_dict()[k], v), k
    # keys already renamed load as they are
    torch.save(src.state_dict(), path)
    got = load_pwc_weights(Tiny(), path)
    assert all(torch.equal(got.state_dict()[k], v) for k, v in src.state_dict().items())
    torch.save({"moduleMain.0.weight": src.netMain[0].weight.detach()}, path)
    with pytest.raises(RuntimeError):
        load_pwc_weights(Tiny(), path)          # strict: a missing key is an error


def test_pwcnet_forward_refuses_cpu_tensors():
    from eavsr_amd.pwc import PWCNET
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(RuntimeError):
        PWCNET().forward_stacked(x)
