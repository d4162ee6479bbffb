"""The range census of the 16-bit backbone without a GPU (addendum): the numpy reference at the edges of both formats,
`headroom`, every spelling of the option and its refusals, the error's message, the order of reads and re-runs of a checked window on
spies, the ABI, and the kernel's head / vectors / tail arithmetic against numpy slicing."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import census_ref as C
from tests import range16_cases as K
from tests import range16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _w(*bits):
    return np.array(bits, np.uint16)


def _f(*bits):
    return np.array(bits, np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------------------ the reference
def test_words_at_the_edges_of_fp16():
    # 65504, the smallest normal, the largest and the smallest subnormal, +-0, +-inf, two NaN payloads
    rec = R.words(_w(0x7BFF, 0x0400, 0x03FF, 0x0001, 0x8001, 0x0000, 0x8000, 0x7C00, 0xFC00, 0x7C01, 0xFE00), "fp16")
    assert rec == {"elements": 11, "max_abs": 65504.0, "nonfinite": 4, "overflow": 0, "flushed": 0, "subnormal": 3}
    assert R.words(_w(0x0000, 0x8000), "fp16")["max_abs"] == 0.0 and R.words(_w(0x7E00), "fp16") == {
        "elements": 1, "max_abs": 0.0, "nonfinite": 1, "overflow": 0, "flushed": 0, "subnormal": 0}
    assert R.words(_w(0xFBFF), "fp16")["max_abs"] == 65504.0 and R.words(_w(0x0400), "fp16")["max_abs"] == 2.0 ** -14


def test_words_at_the_edges_of_bf16():
    rec = R.words(_w(0x7F7F, 0x0080, 0x007F, 0x0001, 0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0xFF81), "bf16")
    assert rec == {"elements": 10, "max_abs": R.FORMAT_MAX["bf16"], "nonfinite": 4, "overflow": 0, "flushed": 0, "subnormal": 2}
    assert R.FORMAT_MAX["bf16"] == float(_f(0x7F7F0000)[0]) and R.FORMAT_MAX["fp16"] == 65504.0
    # the same bits mean other things in the other format: 0x7C00 is a finite bf16
    assert R.words(_w(0x7C00), "bf16")["nonfinite"] == 0 and R.words(_w(0x7F80), "fp16")["nonfinite"] == 1


def test_as_rounded_is_the_cache_census_at_the_overflow_boundaries():
    # 65504 stays, the float below 65520 rounds to 65504, 65520 overflows; bf16: the largest float that stays finite, the tie to inf
    x = _f(0x477FE000, C.F16_MAX_IN, C.F16_INF_IN, C.F16_NORMAL_IN, C.F16_BELOW_NORMAL_IN, C.F16_TINY_IN, C.F16_ZERO_IN, 0, 0x80000000,
           0x7F800000, 0xFF800000, 0x7FC00001, C.BF16_MAX_IN, C.BF16_INF_IN)
    got = R.as_rounded(x, "fp16")
    assert got == C.census(x, "fp16") and got["overflow"] == 3 and got["nonfinite"] == 3 and got["flushed"] == 1
    assert got["subnormal"] == 1      # the float below 2^-14 rounds UP to the smallest normal; the float above 2^-25 is the one subnormal
    got = R.as_rounded(x, "bf16")
    assert got["overflow"] == 1 and got["nonfinite"] == 3 and got["max_abs"] == float(_f(C.BF16_INF_IN)[0])
    # a stored tensor counted as words and the same values counted as rounded agree wherever both are defined
    o = np.arange(65536, dtype=np.uint16)
    for name in ("fp16", "bf16"):
        a, b = R.words(o, name), R.as_rounded(R.widen(o, name), name)
        assert a == b and a["nonfinite"] > 0 and a["subnormal"] > 0, name


def test_headroom():
    from eavsr_amd import ops
    assert ops.headroom(65504.0, "fp16") == 1.0 and ops.headroom(1.0, torch.float16) == 65504.0 and ops.headroom(0.0, "bf16") == float("inf")
    assert ops.headroom(2.0, "bf16") == R.FORMAT_MAX["bf16"] / 2 and ops.headroom(131008.0, "fp16") == 0.5
    assert ops.FORMAT_MAX == R.FORMAT_MAX and R.headroom(4.0, "fp16") == ops.headroom(4.0, "fp16")
    with pytest.raises(ValueError):
        ops.headroom(float("nan"), "fp16")
    with pytest.raises(ValueError):
        ops.headroom(1.0, "fp32")


# ------------------------------------------------------------------------------------------------------------ the option
@pytest.fixture
def N(monkeypatch):
    from eavsr_amd import networks
    monkeypatch.setattr(networks, "BACKBONE_CHECK", None)
    monkeypatch.setattr(networks, "_BACKBONE_CHECK_FROM", "env")
    monkeypatch.setattr(networks, "BACKBONE_DTYPE", None)
    monkeypatch.setattr(networks, "RCAB_H16_FUSED", False)
    monkeypatch.setattr(networks.ops, "CONV3_H16", None)
    return networks


def test_every_spelling_and_refusal_of_the_mode(N, monkeypatch):
    for bad in ("warn", "Report", True, 1, ""):
        with pytest.raises(ValueError, match="None, 'report', 'raise' or 'bf16'"):
            N.check_backbone_check(bad)
    assert [N.check_backbone_check(m) for m in (None, "report", "raise", "bf16")] == [None, "report", "raise", "bf16"]
    with pytest.raises(ValueError, match="without a 16-bit backbone"):
        N.set_backbone_check("report")
    assert N.BACKBONE_CHECK is None
    N.set_backbone_dtype("bf16")
    with pytest.raises(ValueError, match="fallback is from an fp16 backbone"):
        N.set_backbone_check("bf16")
    N.set_backbone_check("raise")
    assert N.BACKBONE_CHECK == "raise"
    with N.backbone_check("report"):
        assert N.BACKBONE_CHECK == "report"
        with pytest.raises(ValueError):
            with N.backbone_check("bf16"):
                pass
        assert N.BACKBONE_CHECK == "report"
    assert N.BACKBONE_CHECK == "raise"
    N.set_backbone_check(None)
    N.set_backbone_dtype("fp16")
    with N.backbone_check("bf16"):
        with torch.no_grad():
            assert N.active_backbone_check() == ("bf16", "fp16")
        with pytest.raises(ValueError, match="under autograd"):
            N.active_backbone_check()
        # the lab's one-launch RCAB, and a backbone that was turned off behind the check: refused at the call
        monkeypatch.setattr(N, "RCAB_H16_FUSED", True)
        with torch.no_grad(), pytest.raises(ValueError, match="RCAB_H16_FUSED"):
            N.active_backbone_check()
        monkeypatch.setattr(N, "RCAB_H16_FUSED", False)
        N.set_backbone_dtype(None)
        with torch.no_grad(), pytest.raises(ValueError, match="without a 16-bit backbone"):
            N.active_backbone_check()
    assert N.BACKBONE_CHECK is None and N.active_backbone_check() is None
    monkeypatch.setattr(N, "RCAB_H16_FUSED", True)
    N.set_backbone_dtype("fp16")
    with pytest.raises(ValueError, match="RCAB_H16_FUSED"):
        N.set_backbone_check("report")
    N.set_backbone_dtype(None)


def test_the_option_and_the_environment(N, monkeypatch):
    from eavsr_amd import eavsrp_model as M
    monkeypatch.delenv("EAVSR_BACKBONE_CHECK", raising=False)
    assert M.backbone_check_option(None) is None and M.backbone_check_option(Namespace()) is None
    for mode in ("report", "raise", "bf16"):
        assert M.backbone_check_option(Namespace(backbone_check=mode)) == mode
        monkeypatch.setenv("EAVSR_BACKBONE_CHECK", mode)
        assert M.backbone_check_option(Namespace()) == mode and M.backbone_check_option(Namespace(backbone_check=None)) == mode
    assert M.backbone_check_option(Namespace(backbone_check="report")) == "report"      # the option wins over the environment
    for bad in ("Raise", "fp16", True, 3):
        with pytest.raises(ValueError):
            M.backbone_check_option(Namespace(backbone_check=bad))
    monkeypatch.setenv("EAVSR_BACKBONE_CHECK", "loud")
    with pytest.raises(ValueError):
        M.backbone_check_option(Namespace())
    with pytest.raises(ValueError):
        M.long_clip_options(Namespace())      # validated with the other inference options
    # isTrain: an option is refused, the environment is not read
    monkeypatch.setenv("EAVSR_BACKBONE_CHECK", "raise")
    assert M.wrapper_backbone_check(Namespace(), True) is None and M.wrapper_backbone_check(Namespace(backbone_check=None), True) is None
    assert M.wrapper_backbone_check(Namespace(), False) == "raise" and M.wrapper_backbone_check(Namespace(backbone_check="bf16"), False) == "bf16"
    with pytest.raises(ValueError, match="opt.backbone_check: the census belongs to the 16-bit backbone"):
        M.wrapper_backbone_check(Namespace(backbone_check="report"), True)
    # ... and a mode that only the environment set is ignored under autograd, where one that was asked for is refused
    monkeypatch.setattr(N, "BACKBONE_CHECK", "report")
    monkeypatch.setattr(N, "_BACKBONE_CHECK_FROM", "env")
    N.set_backbone_dtype("fp16")
    assert N.active_backbone_check() is None
    with torch.no_grad():
        assert N.active_backbone_check() == ("report", "fp16")
    monkeypatch.setattr(N, "_BACKBONE_CHECK_FROM", "call")
    with pytest.raises(ValueError, match="under autograd"):
        N.active_backbone_check()
    N.set_backbone_dtype(None)


# ------------------------------------------------------------------------------------------------------------ the error and the order
def _site(name, max_abs=1.0, nonfinite=0, overflow=0, elements=100):
    return {"site": name, "scope": name.split("/")[0], "op": name.split("/")[1], "index": 0, "flavour": "words", "elements": elements,
            "dtype": "fp16", "max_abs": max_abs, "nonfinite": nonfinite, "overflow": overflow, "flushed": 0, "subnormal": 0,
            "headroom": 65504.0 / max_abs, "tripped_at": 0}


def test_the_error_names_the_first_site_in_call_order(N):
    sites = [_site("encoder/conv3x3_h16g", 3.0), _site("backward_1/conv3x3_c64_h16_res", 65504.0, nonfinite=7),
             _site("backward_1/conv3x3_c64_h16", 9.0, overflow=2)]
    sites[1]["tripped_at"], sites[2]["tripped_at"] = 40, 90      # (shared rows: the order in time is the stamps')
    entry = dict(asked="fp16", used="fp16", fallback=False, tail_fallback=[], frames=5, size=(64, 96), sites=sites)
    assert [s["site"] for s in N.tripped(sites)] == ["backward_1/conv3x3_c64_h16_res", "backward_1/conv3x3_c64_h16"]
    err = N.BackboneRangeError(entry, "stages 1-2")
    assert isinstance(err, ValueError) and err.entry is entry and err.site is sites[1]
    msg = str(err)
    assert "fp16 backbone out of range in stages 1-2 of a window of 5 frames of 64 x 96" in msg
    assert "first at backward_1/conv3x3_c64_h16_res: max |x| 65504, 7 non-finite, 0 overflowed of 100" in msg
    assert "2 sites in all" in msg and "nothing of it has reached the sink" in msg
    assert N.range_summary([entry]) == {"windows": 1, "worst_site": "backward_1/conv3x3_c64_h16_res", "max_abs": 65504.0, "headroom": 1.0,
                                        "fallbacks": [], "tail_fallbacks": [], "nonfinite": 7, "overflow": 2, "subnormal": 0}
    calm = dict(entry, sites=sites[:1], fallback=True, tail_fallback=[2])
    assert N.range_summary([entry, calm])["fallbacks"] == [1] and N.range_summary([calm])["worst_site"] == "encoder/conv3x3_h16g"
    assert N.range_summary([calm])["tail_fallbacks"] == [(0, 2)] and N.range_summary([])["worst_site"] is None


class _Spy:
    """a fake model: `run(tag)` is a stage; its launches trip where `bad` says so for the dtype it runs under"""

    def __init__(self, bad):
        import contextlib
        self.bad, self.events, self.dtype, self.active = bad, [], "fp16", None
        outer = self

        class Census:
            def __init__(self, dtype):
                self.dtype, self.count = dtype, 0
                outer.events.append(("open", dtype))

            def read(self):
                outer.events.append(("read", self.dtype))
                return [_site("s/op", nonfinite=self.count)]
        self.open_census = Census

        @contextlib.contextmanager
        def counting(census):
            prev, self.active = self.active, census
            try:
                yield
            finally:
                self.active = prev
        self.counting = counting

        @contextlib.contextmanager
        def as_dtype(dtype):
            prev, self.dtype = self.dtype, dtype
            self.events.append(("dtype", dtype))
            try:
                yield
            finally:
                self.dtype = prev
        self.as_dtype = as_dtype

    def run(self, tag):
        def go():
            assert self.active is not None and self.active.dtype == self.dtype
            self.events.append(("run", tag, self.dtype))
            if (tag, self.dtype) in self.bad:
                self.active.count += 1
            return (tag, self.dtype)
        return go

    def window(self, N, mode, log):
        return N.BackboneWindow(mode, "fp16", dict(frames=5, size=(64, 64), device="nowhere"), log, self.open_census, self.counting, self.as_dtype)


def test_report_reads_once_when_the_call_ends(N):
    spy, log = _Spy({("fill", "fp16"), ("tail2", "fp16")}), []
    win = spy.window(N, "report", log)
    assert win.stages(spy.run("fill")) == ("fill", "fp16") and win.tail(0, spy.run("tail0")) == ("tail0", "fp16")
    assert win.tail(2, spy.run("tail2")) == ("tail2", "fp16") and log == []
    entry = win.close()
    assert spy.events == [("open", "fp16"), ("run", "fill", "fp16"), ("run", "tail0", "fp16"), ("run", "tail2", "fp16"), ("read", "fp16")]
    assert log == [entry] and entry["sites"][0]["nonfinite"] == 2 and entry["fallback"] is False and entry["tail_fallback"] == []
    assert set(entry) == {"asked", "used", "fallback", "tail_fallback", "frames", "size", "sites"} and "device" not in entry


def test_raise_reads_behind_every_stage_and_stops_before_the_next(N):
    spy, log = _Spy({("tail2", "fp16")}), []
    win = spy.window(N, "raise", log)
    win.stages(spy.run("fill"))
    win.tail(0, spy.run("tail0"))
    with pytest.raises(N.BackboneRangeError, match="the tail of the chunk at frame 2"):
        win.tail(2, spy.run("tail2"))
    assert spy.events == [("open", "fp16"), ("run", "fill", "fp16"), ("read", "fp16"), ("run", "tail0", "fp16"), ("read", "fp16"),
                          ("run", "tail2", "fp16"), ("read", "fp16")]
    assert len(log) == 1 and log[0]["fallback"] is False
    spy, log = _Spy({("fill", "fp16")}), []
    with pytest.raises(N.BackboneRangeError, match="stages 1-2"):
        spy.window(N, "raise", log).stages(spy.run("fill"))
    assert [e[0] for e in spy.events] == ["open", "run", "read"] and len(log) == 1


def test_bf16_runs_the_window_again_and_stays_there(N):
    spy, log = _Spy({("fill", "fp16")}), []
    win = spy.window(N, "bf16", log)
    assert win.stages(spy.run("fill")) == ("fill", "bf16")
    assert win.tail(0, spy.run("tail0")) == ("tail0", "bf16") and win.tail(2, spy.run("tail2")) == ("tail2", "bf16")
    entry = win.close()
    assert spy.events == [("open", "fp16"), ("run", "fill", "fp16"), ("read", "fp16"), ("open", "bf16"), ("dtype", "bf16"),
                          ("run", "fill", "bf16"), ("dtype", "bf16"), ("run", "tail0", "bf16"), ("dtype", "bf16"), ("run", "tail2", "bf16"),
                          ("read", "bf16")]
    assert (entry["asked"], entry["used"], entry["fallback"], entry["tail_fallback"]) == ("fp16", "bf16", True, [])
    assert entry["sites"][0]["nonfinite"] == 1 and entry["sites_used"][0]["nonfinite"] == 0 and spy.dtype == "fp16"


def test_bf16_runs_one_chunks_tail_again_and_the_next_chunk_in_fp16(N):
    spy, log = _Spy({("tail2", "fp16")}), []
    win = spy.window(N, "bf16", log)
    assert win.stages(spy.run("fill")) == ("fill", "fp16") and win.tail(0, spy.run("tail0")) == ("tail0", "fp16")
    assert win.tail(2, spy.run("tail2")) == ("tail2", "bf16") and win.tail(4, spy.run("tail4")) == ("tail4", "fp16")
    entry = win.close()
    assert (entry["used"], entry["fallback"], entry["tail_fallback"]) == ("fp16", False, [2])
    assert [e for e in spy.events if e[0] == "run"] == [("run", "fill", "fp16"), ("run", "tail0", "fp16"), ("run", "tail2", "fp16"),
                                                         ("run", "tail2", "bf16"), ("run", "tail4", "fp16")]
    assert spy.events.count(("read", "fp16")) == 4 and spy.events[-1] == ("read", "bf16") and log == [entry]


# ------------------------------------------------------------------------------------------------------------ the injection, on the CPU
def test_the_scaled_block_leaves_fp16s_range_in_fp32_and_not_bf16s():
    last = K.clip_u8(1, 5, 64, 64, 41)[0, 4:5].float() / 255
    calm = K.hot_block_fp32(K.state_dict("x4"), last)
    hot = K.hot_block_fp32(K.state_dict("x4", "block"), last)
    assert torch.isfinite(hot).all() and 65520.0 < float(hot.abs().max()) < 1e30 and float(calm.abs().max()) < 6e4
    assert torch.isinf(hot.to(torch.float16)).any() and torch.isfinite(hot.to(torch.bfloat16)).all()


# ------------------------------------------------------------------------------------------------------------ the ABI and the cut
def test_the_entry_points_are_in_the_header_and_the_binding():
    from eavsr_amd import _native
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header[:header.index(" * EXPERIMENTAL -- exported by the LAB build only")]
    for name in ("eavsr_range16_words", "eavsr_range16_as_rounded"):
        assert re.search(rf"\bint {name}\(const void\* const\* src_list, const int64_t\* n_list, int32_t nseg, int32_t dtype,\s*uint64_t\* census,"
                         r"\s*void\* stream\);", stable), name
        assert len(_native.SIGNATURES[name][1]) == 6
    src = open(os.path.join(ROOT, "eavsr_amd", "csrc", "range16.hip")).read()
    assert '#include "cache16_census.h"' in src and '#include "round16.h"' in src and "tally.commit(record)" in src
    assert "printf" not in src and not re.search(r"(?<!static_)assert\(", src) and "atomicAdd(" not in src     # (the record's updates are cache16_census.h's)
    assert '#include "round16.h"' in open(os.path.join(ROOT, "eavsr_amd", "csrc", "cache16.hip")).read()


@pytest.mark.parametrize("per_vector", [8, 4])
def test_head_vectors_and_tail_cover_every_element_once(per_vector):
    """the kernel's address arithmetic, transcribed (tests/range16_ref.py: range16_cut / range16_item), against numpy slicing: lengths 1 .. 1100 at
    every misalignment; every vector starts on a 16-byte boundary and lies inside the segment"""
    from eavsr_amd import ops
    for mis in range(per_vector):
        for n in range(1, 1101):
            head, nvec, tail = R.range16_cut(mis, n, per_vector)
            assert head + per_vector * nvec + tail == n and 0 <= head < per_vector and 0 <= tail < per_vector
            assert nvec == 0 or (mis + head) % per_vector == 0
            items = nvec + head + tail
            seen = np.zeros(n, np.int32)
            for i in range(items):
                a, b = R.range16_item(i, head, nvec, tail, per_vector)
                assert 0 <= a < b <= n and (b - a == 1 or (b - a == per_vector and (mis + a) % per_vector == 0))
                seen[a:b] += 1
            assert (seen == 1).all(), (mis, n)
            assert R.range16_item(items, head, nvec, tail, per_vector) == (0, 0)
    with pytest.raises(ValueError):
        R.range16_cut(per_vector, 5, per_vector)


def test_contiguous_rows_of_a_strided_tensor():
    from eavsr_amd import ops
    x = torch.arange(2 * 6 * 8 * 4).view(2, 6, 8, 4)
    for view in (x, x[:, 1:5], x[:, :, 2:7], x[..., 1:3], x[1:], x[:, ::2], x.permute(0, 2, 1, 3), x[:, :, :0]):
        run, offsets = ops.contiguous_runs(view.shape, view.stride())
        flat = x.reshape(-1)[view.storage_offset():]
        got = torch.cat([flat[o:o + run] for o in offsets]) if offsets else flat[:0]
        assert run * len(offsets) == view.numel() and sorted(got.tolist()) == sorted(view.reshape(-1).tolist())
    assert ops.contiguous_runs((2, 6, 8, 4), x.stride()) == (384, [0]) and ops.contiguous_runs((2, 4, 8, 4), x[:, 1:5].stride()) == (128, [0, 192])


def test_a_census_names_its_sites_by_scope_and_position_and_refuses_an_undeclared_16_bit_launch(monkeypatch):
    from eavsr_amd import ops
    counted = []
    monkeypatch.setattr(ops, "range16_words", lambda ts, row: counted.append(("words", len(ts))))
    monkeypatch.setattr(ops, "range16_as_rounded", lambda ts, dt, row: counted.append(("as_rounded", dt)))
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: stamps.append(name))
    monkeypatch.setattr(ops, "_stream", lambda t: None)
    stamps = []
    c = ops.RangeCensus("fp16", "cpu")
    out16, in32 = torch.zeros(6, dtype=torch.float16), torch.zeros(4)
    for step in range(3):      # three time steps of one branch: the same two positions, the same rows
        c.mark("backward_1")
        for _ in range(2):
            assert c.around("conv3x3_c64_h16", (out16,), None, lambda: "ran") == "ran"
    c.mark("encoder")
    c.around("conv3x3_h16g", None, ([in32], "fp16"), lambda: None)
    c.around("conv2d", None, None, lambda: None)                 # an fp32 launch: nothing to say
    c.around("conv5x5_c64_h16", (), None, lambda: None)          # a 16-bit launch that rounds nothing
    assert [(s["site"], s["elements"]) for s in c.sites] == [("backward_1/conv3x3_c64_h16#0", 18), ("backward_1/conv3x3_c64_h16#1", 18),
                                                               ("encoder/conv3x3_h16g#0:in", 4)]
    assert counted == [("words", 1)] * 6 + [("as_rounded", "fp16")] and stamps == ["range16_stamp"] * 7 and c._tick == 7
    with pytest.raises(RuntimeError, match="does not say what it rounds"):
        c.around("rcab_convs_h16", None, None, lambda: None)
    with pytest.raises(RuntimeError, match="rounds to 'bf16'"):
        c.around("conv3x3_h16g", None, ([in32], "bf16"), lambda: None)
    assert ops.RangeCensus.is_16bit("dcnv2_il16") and not ops.RangeCensus.is_16bit("flow_warp_pair") and ops.RANGE16 is None
