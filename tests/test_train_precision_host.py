"""The bf16 training mode's switch, its ABI and the float64 reference helpers, without a GPU."""
import os
import re
import subprocess
import sys

import pytest
import torch

from eavsr_amd import _native
from tests import train_bf16_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["eavsr_conv_weight_bf16x1_bytes", "eavsr_pack_conv_weight_bf16x1", "eavsr_pack_conv_weight_bf16x1_dgrad",
               "eavsr_pack_conv_weight_bf16x1_multi", "eavsr_conv3x3_bf16x1s", "eavsr_conv_wgrad_bias_multi_bf16"]


def test_set_train_precision_accepts_the_two_modes_and_rejects_others():
    from eavsr_amd import networks as Nw
    prev = Nw.get_train_precision()
    try:
        for m in ("bf16", "fp32", "bf16"):
            Nw.set_train_precision(m)
            assert Nw.get_train_precision() == m
        for bad in ("fp16", "BF16", "", None, "tf32"):
            with pytest.raises(ValueError):
                Nw.set_train_precision(bad)
        assert Nw.get_train_precision() == "bf16"      # a rejected value changes nothing
    finally:
        Nw.set_train_precision(prev)


def test_context_manager_restores_the_previous_mode():
    from eavsr_amd import networks as Nw
    prev = Nw.get_train_precision()
    try:
        Nw.set_train_precision("fp32")
        with Nw.train_precision("bf16"):
            assert Nw.get_train_precision() == "bf16"
            with Nw.train_precision("fp32"):
                assert Nw.get_train_precision() == "fp32"
            assert Nw.get_train_precision() == "bf16"
        assert Nw.get_train_precision() == "fp32"
        with pytest.raises(RuntimeError):
            with Nw.train_precision("bf16"):
                raise RuntimeError("inside")
        assert Nw.get_train_precision() == "fp32"
        with pytest.raises(ValueError):
            with Nw.train_precision("fp8"):
                pass
        assert Nw.get_train_precision() == "fp32"
    finally:
        Nw.set_train_precision(prev)


def test_environment_sets_the_default_and_rejects_bad_values():
    code = "from eavsr_amd import networks as N; print(N.get_train_precision())"
    env = dict(os.environ, EAVSR_TRAIN_PRECISION="bf16")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bf16", r.stderr
    env.pop("EAVSR_TRAIN_PRECISION")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "fp32", r.stderr
    env["EAVSR_TRAIN_PRECISION"] = "half"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode != 0 and "ValueError" in r.stderr


def test_ops_precision_arguments_are_checked():
    from eavsr_amd import ops
    with pytest.raises(ValueError):
        ops.check_precision("fp16")
    with pytest.raises(ValueError):      # before any tensor is looked at
        ops.conv2d(torch.zeros(1, 64, 8, 8), torch.zeros(64, 64, 3, 3), precision="fp16")


def test_header_stable_section_and_abi_32():
    src = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    assert re.search(r"#define EAVSR_ABI_VERSION 32\b", src)
    assert _native.ABI_VERSION == 32
    stable = src.split("EXPERIMENTAL -- exported by the LAB build only")[0]
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", stable), name
        assert name in _native.SIGNATURES, name


def test_rne_reference_rounds_ties_to_even_and_negatives():
    # 1 + 2^-8 is halfway between the bf16 neighbours 1 and 1 + 2^-7: the tie goes to the even one (1)
    # 1 + 3 * 2^-8 is halfway between 1 + 2^-7 and 1 + 2^-6: to even (1 + 2^-6); truncation gives the lower one both times
    x = torch.tensor([1 + 2 ** -8, 1 + 3 * 2 ** -8, -(1 + 3 * 2 ** -8), -1.00390625 - 2 ** -20, 3.0], dtype=torch.float32)
    assert R.bf16_rne(x).tolist() == [1.0, 1 + 2 ** -6, -(1 + 2 ** -6), -(1 + 2 ** -7), 3.0]
    assert R.bf16_trunc(x).tolist() == [1.0, 1 + 2 ** -7, -(1 + 2 ** -7), -1.0, 3.0]


def test_conv_and_wgrad_references_on_hand_made_cases():
    x = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    x[0, 0, 1, 1] = -2.0
    x[0, 0, 0, 0] = 1.0
    w = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    w[0, 0, 1, 1] = 3.0                 # centre tap
    w[0, 0, 0, 0] = -0.5                # top-left tap: y[i, j] += -0.5 x[i - 1, j - 1]
    y, s = R.conv3x3_ref(x, w, torch.tensor([0.25]))
    assert y[0, 0, 1, 1].item() == 3.0 * -2.0 - 0.5 * 1.0 + 0.25
    assert s[0, 0, 1, 1].item() == 6.0 + 0.5
    assert y[0, 0, 0, 0].item() == 3.0 + 0.25 and s[0, 0, 0, 0].item() == 3.0
    dy = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
    dy[0, 0, 1, 1] = -1.0
    g, gs = R.wgrad3x3_ref([dy, dy], [x, -x])       # two segments cancel in g, add in S
    assert torch.equal(g, torch.zeros(1, 1, 3, 3, dtype=torch.float64))
    assert gs[0, 0, 1, 1].item() == 4.0 and gs[0, 0, 0, 0].item() == 2.0
    g1, _ = R.wgrad3x3_ref([dy], [x])
    assert g1[0, 0, 1, 1].item() == 2.0 and g1[0, 0, 0, 0].item() == -1.0
