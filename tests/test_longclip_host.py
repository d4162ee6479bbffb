"""The long-clip path (EAVSRP.forward_long, eavsr_amd/framestore.py, ops.u8_to_f32, harness.super_resolve), what needs no GPU: the
prefetch schedule of the host cache as a pure function, the switches, the argument checks and the C ABI's new entry points."""
import os
import re
import subprocess
import sys
from argparse import Namespace

import pytest
import torch

from eavsr_amd import framestore as FS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRANCHES = ["backward_1", "forward_1", "backward_2", "forward_2"]


def _reference_reads(t, backward, others):
    """What `EAVSRP.propagate` (eavsrp_model.py:242-329) indexes at every step, restated from its own index lists (frame_idx,
    flow_idx, mapping_idx) rather than from framestore's arithmetic: flows has t - 1 entries, flow j joins frames j and j + 1."""
    tf = t - 1
    frame_idx = list(range(0, tf + 1))
    flow_idx = list(range(-1, tf))
    mapping_idx = list(range(0, t))
    mapping_idx += mapping_idx[::-1]
    if backward:
        frame_idx = frame_idx[::-1]
        flow_idx = frame_idx
    step = 1 if backward else -1
    fkey = "flow_backward" if backward else "flow_forward"
    reads = []
    for i, idx in enumerate(frame_idx):
        r = {(k, mapping_idx[idx]) for k in FS.PYR}
        if i > 0:
            r |= {(k, mapping_idx[idx + step]) for k in FS.PYR}
            r.add((fkey, flow_idx[i]))
            if i > 1:
                r |= {(k, mapping_idx[idx + 2 * step]) for k in FS.PYR}
                r.add((fkey, flow_idx[i - 1]))
        r |= {(k, idx) for k in others}
        reads.append(r)
    return reads


@pytest.mark.parametrize("t", [1, 2, 3, 7, 12])
@pytest.mark.parametrize("backward", [True, False])
@pytest.mark.parametrize("n_others", [0, 3])
def test_prefetch_schedule_has_every_read_resident_in_time_and_stays_within_its_window(t, backward, n_others):
    others = BRANCHES[:n_others]
    reads = FS.propagate_reads(t, backward, others)
    want = _reference_reads(t, backward, others)
    assert len(reads) == t and [set(r) for r in reads] == want
    for r in reads:      # every index exists: frames 0 .. t - 1, flows 0 .. t - 2
        for key, idx in r:
            assert 0 <= idx < (t - 1 if key in FS.FLOW_KEYS else t), (key, idx)
    sched = FS.prefetch_schedule(reads)
    assert len(sched.fetch) == len(sched.evict) == t
    last_use = {}
    for i, r in enumerate(reads):
        for it in r:
            last_use[it] = i
    bound = FS.window_bound(n_others)
    resident = set(sched.prologue)
    fetched = list(sched.prologue)
    for i in range(t):
        # step i's copies are issued when step i is enqueued: what step i reads was issued BEFORE that (prologue / step i - 1)
        assert set(reads[i]) <= resident, (i, set(reads[i]) - resident)
        resident |= set(sched.fetch[i])
        fetched += sched.fetch[i]
        # the window while step i computes
        assert len(resident) <= bound["items"], (i, len(resident))
        for level in FS.PYR:
            assert sum(1 for k, _ in resident if k == level) <= bound["pyramid_frames"]
        assert sum(1 for k, _ in resident if k in FS.FLOW_KEYS) <= bound["flows"]
        for o in others:
            assert sum(1 for k, _ in resident if k == o) <= bound["frames_per_other_branch"]
        for it in sched.evict[i]:
            assert it in resident and last_use[it] <= i, (i, it)      # nothing leaves before its last use
        resident -= set(sched.evict[i])
    assert not resident                                            # the window is empty when the branch is done
    assert len(fetched) == len(set(fetched)) == len(last_use)      # every tensor crosses the link once per branch
    # the schedule looks one step ahead, no further: step i's copies are exactly what step i + 1 newly needs
    for i in range(t - 1):
        assert set(sched.fetch[i]) == set(reads[i + 1]) - set().union(*[set(r) for r in reads[:i + 1]])


def test_schedule_is_a_pure_function():
    a = FS.prefetch_schedule(FS.propagate_reads(7, True, BRANCHES[:2]))
    b = FS.prefetch_schedule(FS.propagate_reads(7, True, BRANCHES[:2]))
    assert a == b
    with pytest.raises(ValueError):
        FS.propagate_reads(0, True)
    with pytest.raises(ValueError):
        FS.check_cache("disk")


def test_long_clip_switches_from_options_and_environment(monkeypatch):
    from eavsr_amd.eavsrp_model import long_clip_options
    monkeypatch.delenv("EAVSR_FRAME_CHUNK", raising=False)
    monkeypatch.delenv("EAVSR_CPU_CACHE", raising=False)
    assert long_clip_options(Namespace()) == (None, False)
    assert long_clip_options(None) == (None, False)
    assert long_clip_options(Namespace(frame_chunk=3, cpu_cache=True)) == (3, True)
    assert long_clip_options(Namespace(frame_chunk=0)) == (None, False)
    monkeypatch.setenv("EAVSR_FRAME_CHUNK", "4")
    monkeypatch.setenv("EAVSR_CPU_CACHE", "1")
    assert long_clip_options(Namespace()) == (4, True)
    assert long_clip_options(Namespace(frame_chunk=2, cpu_cache=False)) == (2, False)      # the options win
    for bad in ("0", "-1", "three", "2.5"):
        monkeypatch.setenv("EAVSR_FRAME_CHUNK", bad)
        with pytest.raises(ValueError):
            long_clip_options(Namespace())
    monkeypatch.delenv("EAVSR_FRAME_CHUNK")
    monkeypatch.setenv("EAVSR_CPU_CACHE", "yes")
    with pytest.raises(ValueError):
        long_clip_options(Namespace())
    monkeypatch.delenv("EAVSR_CPU_CACHE")
    for bad in (Namespace(frame_chunk=-2), Namespace(frame_chunk=1.5), Namespace(frame_chunk=True), Namespace(cpu_cache=1)):
        with pytest.raises(ValueError):
            long_clip_options(bad)


def test_forward_long_raises_under_grad_on_cpu_tensors_and_on_bad_arguments():
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None).eval()
    x = torch.zeros(1, 3, 3, 64, 64)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="no_grad"):
            net.forward_long(x)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="GPU only"):
            net.forward_long(x)
        with pytest.raises(RuntimeError, match="GPU only"):      # 8-bit frames may live on the host, the network may not
            net.forward_long(torch.zeros(1, 3, 3, 64, 64, dtype=torch.uint8))
        with pytest.raises(ValueError):
            net.forward_long(x, cache="disk")
        with pytest.raises(ValueError):
            net.forward_long(x[0])


def test_route_batch_pins_the_routing_predicates_and_restores_them():
    from eavsr_amd import ops
    lib = ops.lib()
    assert ops._ROUTE_BATCH is None and ops._rn(3) == 3
    # the direct kernel's tile height is chosen from the batch size: 8-row tiles for 2 x 96 x 96, taller ones for 64 x 96 x 96
    big = lib.eavsr_conv2d_tile_rows(64, 96, 96, 3)
    assert lib.eavsr_conv2d_tile_rows(2, 96, 96, 3) == 8 and big > 8
    small = ops.x6s_takes(1, 64, 96)
    with ops.route_batch(64):
        assert ops._rn(3) == 64
        assert lib.eavsr_conv2d_tile_rows(2, 96, 96, 3) == big and lib.eavsr_conv2d_tiles(2, 96, 96, 3) == lib.eavsr_conv2d_tiles(64, 96, 96, 3)
        assert not ops.x6s_takes(1, 64, 96)          # 64 images of 64 x 96 are no crop-sized launch
        with ops.route_batch(None):
            assert ops._rn(3) == 3 and lib.eavsr_conv2d_tile_rows(2, 96, 96, 3) == 8
        assert ops._rn(3) == 64 and lib.eavsr_conv2d_tile_rows(2, 96, 96, 3) == big
    assert ops._ROUTE_BATCH is None and lib.eavsr_conv2d_tile_rows(2, 96, 96, 3) == 8 and ops.x6s_takes(1, 64, 96) == small
    with pytest.raises(RuntimeError):
        with ops.route_batch(8):
            raise RuntimeError("boom")
    assert ops._ROUTE_BATCH is None and lib.eavsr_route_batch(0) == 0
    with pytest.raises(ValueError):
        with ops.route_batch(0):
            pass


def test_u8_to_f32_is_in_the_stable_header_and_checks_its_arguments_on_the_host():
    from eavsr_amd import _native, ops
    src = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = src.split("EXPERIMENTAL -- exported by the LAB build only")[0]
    for name in ("eavsr_u8_to_f32", "eavsr_route_batch"):
        assert re.search(r"\b" + name + r"\(", stable), name
        assert name in _native.SIGNATURES, name
    lib = _native.load()
    assert lib.eavsr_u8_to_f32(None, 16, 1, 3, 8, 8, 0, None) == -1 and b"NULL" in lib.eavsr_last_error()
    assert lib.eavsr_u8_to_f32(16, 16, 1, 2, 8, 8, 1, None) == -2       # interleaved frames have 3 channels
    assert lib.eavsr_u8_to_f32(16, 16, 1, 3, 8, 8, 2, None) == -2       # layout 0 or 1
    assert lib.eavsr_u8_to_f32(16, 20, 1, 3, 8, 8, 0, None) == -2 and b"aligned" in lib.eavsr_last_error()
    assert lib.eavsr_u8_to_f32(16, 16, 70000, 3, 8, 8, 0, None) == -2
    assert lib.eavsr_u8_to_f32(16, 16, 0, 3, 8, 8, 0, None) == 0        # no frames: nothing is launched
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.u8_to_f32(torch.zeros(1, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(TypeError):
        ops.u8_to_f32([1, 2])
    # the reference's division is not a multiplication by the rounded reciprocal: the two differ for some byte values, which is
    # why the kernel divides (and why the GPU test compares with the host's division, not with torch's device `x / 255`)
    v = torch.arange(256, dtype=torch.float32)
    assert not torch.equal(v / 255.0, v * torch.tensor(1.0 / 255.0, dtype=torch.float32))


def test_super_resolve_checks_its_arguments_without_a_gpu():
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None).eval()
    with pytest.raises(RuntimeError, match="GPU"):
        harness.super_resolve(net, torch.zeros(2, 3, 64, 64, dtype=torch.uint8))


def test_model_wrappers_take_the_long_path_only_for_inference_with_a_switch():
    """EAVSRPModel.forward(): forward_long when not isTrain and a switch is set, the plain forward otherwise (checked on the source:
    constructing the wrapper needs a GPU)"""
    code = ("import inspect; from eavsr_amd.eavsrp_model import EAVSRPModel; from eavsr_amd.eavsrpx2_model import EAVSRPx2Model; "
            "s = inspect.getsource(EAVSRPModel.forward); "
            "assert 'not self.isTrain and (self.frame_chunk is not None or self.cpu_cache)' in s and 'forward_long' in s; "
            "assert EAVSRPx2Model.forward is EAVSRPModel.forward; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
