"""The deterministic training mode's switch, its plumbing and its entry points in the header, without a GPU."""
import os
import re
import subprocess
import sys
from argparse import Namespace

import pytest
import torch

from eavsr_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["eavsr_resize_bilinear_ac_bwd_det_f32", "eavsr_flow_warp_bwd_dx_det_workspace_floats", "eavsr_flow_warp_bwd_dx_det_f32",
               "eavsr_dcnv2_col2im_dx_det_workspace_floats", "eavsr_dcnv2_col2im_dx_det_f32"]


def test_set_deterministic_accepts_bools_only():
    from eavsr_amd import networks as Nw, ops
    prev = ops.DETERMINISTIC
    try:
        for f in (True, False, True):
            Nw.set_deterministic(f)
            assert Nw.get_deterministic() is f and ops.DETERMINISTIC is f
        for bad in (1, 0, "1", "true", None, 1.0):
            with pytest.raises(ValueError):
                Nw.set_deterministic(bad)
        assert Nw.get_deterministic() is True      # a rejected value changes nothing
    finally:
        ops.DETERMINISTIC = prev


def test_context_manager_restores_the_previous_setting():
    from eavsr_amd import networks as Nw, ops
    prev = ops.DETERMINISTIC
    try:
        Nw.set_deterministic(False)
        with Nw.deterministic():
            assert Nw.get_deterministic()
            with Nw.deterministic(False):
                assert not Nw.get_deterministic()
            assert Nw.get_deterministic()
        assert not Nw.get_deterministic()
        with pytest.raises(RuntimeError):
            with Nw.deterministic(True):
                raise RuntimeError("inside")
        assert not Nw.get_deterministic()
        with pytest.raises(ValueError):
            with Nw.deterministic("yes"):
                pass
        assert not Nw.get_deterministic()
    finally:
        ops.DETERMINISTIC = prev


def test_torch_deterministic_algorithms_engage_the_mode():
    from eavsr_amd import networks as Nw, ops
    prev_t, prev = torch.are_deterministic_algorithms_enabled(), ops.DETERMINISTIC
    try:
        ops.DETERMINISTIC = False
        torch.use_deterministic_algorithms(False)
        assert not Nw.get_deterministic() and not ops.deterministic_active()
        torch.use_deterministic_algorithms(True)
        assert Nw.get_deterministic() and ops.deterministic_active()
        with Nw.deterministic(False):      # the switch cannot turn torch's own request off
            assert Nw.get_deterministic()
    finally:
        torch.use_deterministic_algorithms(prev_t)
        ops.DETERMINISTIC = prev


def test_environment_sets_the_default_and_rejects_bad_values():
    code = "from eavsr_amd import networks as N; print(N.get_deterministic())"
    env = dict(os.environ, EAVSR_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "True", r.stderr
    for v in ("0", None):
        if v is None:
            env.pop("EAVSR_DETERMINISTIC")
        else:
            env["EAVSR_DETERMINISTIC"] = v
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip() == "False", r.stderr
    for bad in ("yes", "2", "true", ""):
        env["EAVSR_DETERMINISTIC"] = bad
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode != 0 and "ValueError" in r.stderr and "EAVSR_DETERMINISTIC" in r.stderr, (bad, r.stderr)


def test_opt_deterministic_reaches_the_switch(monkeypatch):
    """EAVSRPModel.__init__ hands opt.deterministic to networks.set_deterministic before it needs a GPU (the constructor then
    stops at its device check here)"""
    from eavsr_amd import eavsrp_model, networks as Nw, ops
    seen = []
    monkeypatch.setattr(Nw, "set_deterministic", lambda f: seen.append(f))
    for value, want in ((True, [True]), (False, [False]), (None, [])):
        seen.clear()
        opt = Namespace(predict=False, n_frame=3, n_flow=5, scale=4, isTrain=True, gpu_ids=[], lr=1e-4, beta1=0.9, beta2=0.999,
                        weight_decay=0.0, npost=350, deterministic=value)
        with pytest.raises(RuntimeError):      # gpu_ids == []: no CPU path
            eavsrp_model.EAVSRPModel(opt)
        assert seen == want
    assert isinstance(ops.DETERMINISTIC, bool)


def test_header_stable_section_holds_the_new_entry_points():
    src = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = src.split("EXPERIMENTAL -- exported by the LAB build only")[0]
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", stable), name
        assert name in _native.SIGNATURES, name


def _groups(monkeypatch, det, last_uses, uses=11):
    """how grad_sink groups `uses` uses of one weight into weight-gradient launches, with `last_uses` recorded for that weight
    by an earlier backward (the launch itself is replaced by a recorder: no GPU)"""
    from eavsr_amd import autograd as AG, ops
    seen = []
    monkeypatch.setattr(ops, "conv_wgrad_multi", lambda dys, srcs, k, out, accumulate, bias_out, precision: seen.append(
        ([int(g[0, 0, 0, 0]) for g in dys], accumulate)))
    monkeypatch.setattr(ops, "DETERMINISTIC", det)
    w = torch.zeros(4, 4, 3, 3)
    monkeypatch.setattr(AG.grad_sink, "_last_uses", {(id(w),): last_uses})
    with AG.grad_sink() as sink:
        for i in range(uses):
            sink.add_use([w], None, 3, torch.full((1, 4, 2, 2), float(i)), [torch.zeros(1, 4, 2, 2)])
        sink.flush = lambda: [AG.grad_sink._launch(e) for e in sink.entries.values()]      # (no .grad hand-over of CPU stand-ins)
    return seen


def test_deterministic_weight_gradient_grouping_ignores_earlier_backwards(monkeypatch):
    """The default mode launches a weight's gradient as soon as it has seen as many uses as in the PREVIOUS backward; a stale
    count (another shape, another phase, or a freed model whose weights had the same id()) then splits the uses differently --
    another rounding of the same sum.  In the deterministic mode the groups are BATCH uses in backward order, whatever came before."""
    from eavsr_amd import autograd as AG
    B = AG.grad_sink.BATCH
    fresh = _groups(monkeypatch, True, -1)
    assert fresh == [(list(range(B)), False), (list(range(B, 11)), True)]
    for stale in (3, 5, B, 11):
        assert _groups(monkeypatch, True, stale) == fresh, stale
    assert _groups(monkeypatch, False, 3)[0] == ([0, 1, 2], False)      # (the default mode's early launch, unchanged)
