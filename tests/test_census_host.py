"""The census of the 16-bit feature cache (addendum), everything that needs no GPU: the numpy reference on hand-built
values at the edges of both formats, `ops.census_record`, every spelling and refusal of `cache_check` as an argument and as an option,
`CacheRangeError`'s message, the order of a checked `forward_long` call on a fake store (`framestore.checked_window`), the stores'
bookkeeping with the kernel replaced by the reference, and the C-ABI declaration."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import census_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)


def _one(bits, dtype):
    """(the 16-bit result, the census without 'elements' and 'max_abs') of one element"""
    c = R.census(_f32(bits), dtype)
    return int(R.round16(_f32(bits), dtype)[0]), (c["nonfinite"], c["overflow"], c["flushed"], c["subnormal"])


# --------------------------------------------------------------------------------------------------------------- the reference
def test_the_reference_at_the_edges_of_fp16():
    assert _f32(R.F16_MAX_IN)[0] < 65520.0 == _f32(R.F16_INF_IN)[0] and _f32(R.F16_ZERO_IN)[0] == 2.0 ** -25
    assert _f32(R.F16_NORMAL_IN)[0] == 2.0 ** -14 and _f32(R.F16_TINY_IN)[0] == np.nextafter(np.float32(2.0 ** -25), np.float32(1))
    assert _f32(R.F16_BELOW_NORMAL_IN)[0] == np.nextafter(np.float32(2.0 ** -14), np.float32(0))
    #                                      o       nonfinite overflow flushed subnormal
    assert _one(R.F16_MAX_IN, "fp16") == (0x7BFF, (0, 0, 0, 0))                  # 65504, the largest fp16
    assert _one(R.F16_INF_IN, "fp16") == (0x7C00, (0, 1, 0, 0))                  # 65520: the overflow threshold
    assert _one(R.F16_INF_IN | 0x80000000, "fp16") == (0xFC00, (0, 1, 0, 0))
    assert _one(R.F16_ZERO_IN, "fp16") == (0x0000, (0, 0, 1, 0))                 # 2^-25: the tie goes to even, 0
    assert _one(R.F16_ZERO_IN | 0x80000000, "fp16") == (0x8000, (0, 0, 1, 0))    # -0 is a flush as well
    assert _one(R.F16_TINY_IN, "fp16") == (0x0001, (0, 0, 0, 1))                 # the next float up: 2^-24, the smallest subnormal
    assert _one(R.F16_NORMAL_IN, "fp16") == (0x0400, (0, 0, 0, 0))               # 2^-14: normal
    # the float below 2^-14 lies 2^-38 under it, far closer than half a subnormal step (2^-25): numpy rounds it UP to the normal
    assert _one(R.F16_BELOW_NORMAL_IN, "fp16") == (0x0400, (0, 0, 0, 0))
    assert _one(0x387FE000, "fp16") == (0x0400, (0, 0, 0, 0)) and _one(0x387FDFFF, "fp16") == (0x03FF, (0, 0, 0, 1))      # the tie and below it
    c = R.census(_f32(R.F16_INF_IN), "fp16")
    assert c["max_abs"] == 65520.0 and c["elements"] == 1       # what overflowed is finite going in: it counts for max_abs


def test_the_reference_at_the_edges_of_bf16():
    assert _one(R.BF16_MAX_IN, "bf16") == (0x7F7F, (0, 0, 0, 0))                 # finite
    assert _one(R.BF16_INF_IN, "bf16") == (0x7F80, (0, 1, 0, 0))                 # the tie rounds to even: inf
    assert _one(R.BF16_INF_IN | 0x80000000, "bf16") == (0xFF80, (0, 1, 0, 0))
    assert _one(R.F16_INF_IN, "bf16") == (0x4780, (0, 0, 0, 0))                  # fp16's overflow is nothing here
    assert _one(0x00000001, "bf16") == (0x0000, (0, 0, 1, 0))                    # the smallest fp32 subnormal is flushed
    assert _one(0x00008000, "bf16") == (0x0000, (0, 0, 1, 0)) and _one(0x00008001, "bf16") == (0x0001, (0, 0, 0, 1))
    assert _one(0x007F8000, "bf16") == (0x0080, (0, 0, 0, 0)) and _one(0x007F7FFF, "bf16") == (0x007F, (0, 0, 0, 1))
    # against torch's own conversion over a spread of exponents (NaN aside, where only the payload differs)
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(4096) * np.exp2(rng.integers(-140, 128, 4096))).astype(np.float32)
    assert np.array_equal(R.round16(x, "bf16"), torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(R.round16(x, "fp16"), torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy().view(np.uint16))


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_the_reference_on_zeros_infinities_and_nan(dtype):
    inf16 = 0x7C00 if dtype == "fp16" else 0x7F80
    assert _one(0x00000000, dtype) == (0x0000, (0, 0, 0, 0)) and _one(0x80000000, dtype) == (0x8000, (0, 0, 0, 0))      # +-0: nothing
    assert _one(0x7F800000, dtype) == (inf16, (1, 0, 0, 0))                      # +-inf: non-finite, NOT an overflow
    assert _one(0xFF800000, dtype) == (inf16 | 0x8000, (1, 0, 0, 0))
    o, counts = _one(0x7FC00000, dtype)
    assert (o & 0x7FFF) > inf16 and counts == (1, 0, 0, 0)                       # a NaN stays a NaN: non-finite
    for bits in (0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001):
        assert R.census(_f32(bits), dtype)["max_abs"] == 0.0                     # none of them is a finite magnitude
    both = R.census(np.concatenate([_f32(b) for b in R.BOUNDARY_BITS]), dtype)
    assert both["elements"] == len(R.BOUNDARY_BITS) == 21 and both["nonfinite"] == 3
    assert both["max_abs"] == float(_f32(R.BF16_INF_IN)[0])
    assert both["overflow"] == (2 * 3 if dtype == "fp16" else 2)                 # fp16: 65520 and the two bf16 edges, of each sign
    assert R.add(R.census(_f32(R.F16_INF_IN), dtype), R.census(_f32(0x7FC00000), dtype)) == \
        R.census(np.concatenate([_f32(R.F16_INF_IN), _f32(0x7FC00000)]), dtype)


# ------------------------------------------------------------------------------------------------------------- census_record
def test_census_record_turns_a_row_into_numbers():
    from eavsr_amd import ops
    assert ops.CENSUS_SLOTS == R.SLOTS
    rec = ops.census_record(torch.tensor([R.F16_INF_IN, 1, 2, 3, 4]), 10, "fp16")
    assert rec == {"elements": 10, "dtype": "fp16", "max_abs": 65520.0, "nonfinite": 1, "overflow": 2, "flushed": 3, "subnormal": 4}
    assert isinstance(rec["max_abs"], float) and all(isinstance(rec[k], int) for k in R.SLOTS[1:])
    assert ops.census_record([0, 0, 0, 0, 0], 0, torch.bfloat16) == {"elements": 0, "dtype": "bf16", "max_abs": 0.0, "nonfinite": 0,
                                                                     "overflow": 0, "flushed": 0, "subnormal": 0}
    x = (np.random.default_rng(0).standard_normal(1000) * 1e5).astype(np.float32)
    want = R.census(x, "fp16")
    assert ops.census_record(np.array(R.row(want), np.int64), 1000, torch.float16) == dict(want, dtype="fp16")
    for row, elements, dtype in (([0] * 4, 1, "fp16"), ([0] * 5, -1, "fp16"), ([0] * 5, True, "fp16"), ([0] * 5, 1, "fp32"),
                                 ([0x7F800000, 0, 0, 0, 0], 1, "fp16"), ([0, 2, 0, 0, 0], 1, "bf16"), ([-1, 0, 0, 0, 0], 1, "bf16")):
        with pytest.raises(ValueError):
            ops.census_record(row, elements, dtype)


def test_the_op_refuses_before_anything_is_launched():
    from eavsr_amd import ops
    src, dst, ok = [torch.zeros(8)], [torch.zeros(8, dtype=torch.float16)], torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pack16_census(src, dst, "fp16", ok)
    for bad in (torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int64), torch.zeros(1, 5, dtype=torch.int64),
                torch.zeros(5, 2, dtype=torch.int64)[:, 0], torch.zeros(5)):
        with pytest.raises(ValueError, match="census"):
            ops.pack16_census(src, dst, "fp16", bad)
    with pytest.raises(TypeError, match="census"):
        ops.pack16_census(src, dst, "fp16", np.zeros(5, np.int64))
    with pytest.raises(ValueError):
        ops.pack16_census(src, dst, "fp32", ok)
    with pytest.raises(ValueError):
        ops.pack16_census(src, [], "fp16", ok)


# ------------------------------------------------------------------------------------------------- the argument and the option
def test_cache_check_in_all_its_spellings_and_its_refusals():
    from eavsr_amd import framestore as FS
    assert FS.CACHE_CHECKS == ("report", "raise", "bf16")
    assert FS.check_cache_check(None, None) is None and FS.check_cache_check(None, "fp16") is None
    for dtype in ("fp16", "bf16"):
        assert FS.check_cache_check("report", dtype) == "report" and FS.check_cache_check("raise", dtype) == "raise"
    assert FS.check_cache_check("bf16", "fp16") == "bf16"
    for bad in ("warn", "Report", "", "fp16", True, False, 1, torch.bfloat16, ("report",)):
        with pytest.raises(ValueError, match="cache_check"):
            FS.check_cache_check(bad, "fp16")
    for check in FS.CACHE_CHECKS:
        with pytest.raises(ValueError, match="without cache_dtype"):
            FS.check_cache_check(check, None)
    with pytest.raises(ValueError, match="fp16 cache"):
        FS.check_cache_check("bf16", "bf16")
    assert issubclass(FS.CacheRangeError, ValueError)


def test_the_option_function_reads_opt_then_env_then_default(monkeypatch):
    from eavsr_amd.eavsrp_model import cache_check_option, long_clip_options
    monkeypatch.delenv("EAVSR_CACHE_CHECK", raising=False)
    assert cache_check_option() is None and cache_check_option(Namespace()) is None and cache_check_option(Namespace(cache_check=None)) is None
    for value in ("report", "raise", "bf16"):
        assert cache_check_option(Namespace(cache_check=value)) == value
    monkeypatch.setenv("EAVSR_CACHE_CHECK", "raise")
    assert cache_check_option() == "raise" and cache_check_option(Namespace()) == "raise"
    assert cache_check_option(Namespace(cache_check="report")) == "report"      # the options win
    assert long_clip_options(Namespace()) == (None, False)
    monkeypatch.setenv("EAVSR_CACHE_CHECK", "")
    assert cache_check_option() is None
    monkeypatch.setenv("EAVSR_CACHE_CHECK", "warn")
    with pytest.raises(ValueError, match="EAVSR_CACHE_CHECK"):
        cache_check_option()
    with pytest.raises(ValueError, match="EAVSR_CACHE_CHECK"):
        long_clip_options(Namespace())      # validated with the others
    assert cache_check_option(Namespace(cache_check="bf16")) == "bf16"      # a bad environment is not read where the options decide
    for bad in ("warn", True, 1, torch.bfloat16, ("raise",)):
        with pytest.raises(ValueError, match="opt.cache_check"):
            cache_check_option(Namespace(cache_check=bad))


def test_arguments_are_refused_before_anything_runs(monkeypatch):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRP, EAVSRPModel
    for name in ("EAVSR_CACHE_DTYPE", "EAVSR_CACHE_CHECK"):
        monkeypatch.delenv(name, raising=False)
    net = EAVSRP.__new__(EAVSRP)
    x = torch.zeros(1, 2, 3, 96, 112)
    plan = [(0, 2, 0, 2)]
    with torch.no_grad():
        for dtype, check, match in (("fp16", "warn", "cache_check"), ("fp16", True, "cache_check"), (None, "report", "without cache_dtype"),
                                    (None, "bf16", "without cache_dtype"), ("bf16", "bf16", "fp16 cache"), (torch.bfloat16, "bf16", "fp16 cache")):
            for call in (lambda: EAVSRP.forward_long(net, x, cache_dtype=dtype, cache_check=check),
                         lambda: EAVSRP.forward_tiled(net, x, 64, cache_dtype=dtype, cache_check=check),
                         lambda: EAVSRP.forward_segments_padded(net, x, plan, None, cache_dtype=dtype, cache_check=check),
                         lambda: EAVSRP.forward_cached(net, x, dtype, cache_check=check),
                         lambda: EAVSRP.forward_cached(net, x, dtype, ensemble=2, cache_check=check),
                         lambda: harness.super_resolve(None, ["/nonexistent/frame.png"], cache_dtype=dtype, cache_check=check)):
                with pytest.raises(ValueError, match=match):
                    call()
    with pytest.raises(ValueError, match="opt.cache_check"):
        harness.super_resolve(Namespace(opt=Namespace(cache_dtype="fp16", cache_check="warn")), x[0])
    with pytest.raises(ValueError, match="without cache_dtype"):
        harness.super_resolve(Namespace(opt=Namespace(cache_check="raise")), x[0])
    monkeypatch.setenv("EAVSR_CACHE_CHECK", "bf16")
    with pytest.raises(ValueError, match="fp16 cache"):
        harness.super_resolve(None, ["/nonexistent/frame.png"], cache_dtype="bf16")
    monkeypatch.delenv("EAVSR_CACHE_CHECK")
    with pytest.raises(ValueError, match="opt.cache_check"):      # a training wrapper refuses the option before it builds anything
        EAVSRPModel(Namespace(scale=4, isTrain=True, cache_check="report", gpu_ids=[0]))
    with pytest.raises(ValueError, match="without cache_dtype"):      # and an inference wrapper a check with nothing to check
        EAVSRPModel(Namespace(scale=4, isTrain=False, cache_check="report", gpu_ids=[0]))
    with pytest.raises(ValueError, match="fp16 cache"):
        EAVSRPModel(Namespace(scale=4, isTrain=False, cache_dtype="bf16", cache_check="bf16", gpu_ids=[0]))


def test_a_call_without_a_check_hands_no_new_keyword_on():
    """the methods `forward_cached` leads to, replaced by recorders: without a check each is called exactly as before; with one, the
    keyword travels to whichever path is taken"""
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP.__new__(EAVSRP)
    calls = []
    for name in ("forward_long", "forward_segments_padded", "forward_tiled"):
        net.__dict__[name] = lambda *a, _n=name, **k: calls.append((_n, k)) or _n
    x = torch.zeros(1, 4, 3, 96, 112)
    plan = [(0, 3, 0, 2), (1, 4, 2, 4)]
    with torch.no_grad():
        for tile, segments, path in ((64, plan, "forward_tiled"), (None, plan, "forward_segments_padded"), (None, None, "forward_long")):
            for ensemble in (None, 1):
                calls.clear()
                assert net.forward_cached(x, "fp16", ensemble=ensemble, tile=tile, overlap=16, segments=segments) == path
                assert len(calls) == 1 and "cache_check" not in calls[0][1] and calls[0][1]["cache_dtype"] == "fp16"
                calls.clear()
                assert net.forward_cached(x, "fp16", ensemble=ensemble, tile=tile, overlap=16, segments=segments, cache_check="bf16") == path
                assert len(calls) == 1 and calls[0][1]["cache_check"] == "bf16" and calls[0][1]["cache_dtype"] == "fp16"


# ------------------------------------------------------------------------------------------------------------------ the policy
def _record(**kw):
    return dict({"elements": 100, "dtype": "fp16", "max_abs": 1.5, "nonfinite": 0, "overflow": 0, "flushed": 0, "subnormal": 0}, **kw)


class _FakeStore:
    def __init__(self, events, dtype, census, keys):
        self.events, self.dtype, self.takes_census, self.keys = events, dtype, census, keys
        events.append(("make", dtype, census))

    def finish(self):
        self.events.append(("finish", self.dtype))

    def census(self):
        assert self.takes_census
        self.events.append(("census", self.dtype))
        return self.keys[self.dtype]


def _run(check, keys, dtype="fp16"):
    from eavsr_amd import framestore as FS
    events, log = [], []
    make = lambda dt, census: _FakeStore(events, dt, census, keys)
    fill = lambda store: events.append(("fill", store.dtype)) or ["backward_1"]
    drain = lambda store, state: events.append(("drain", store.dtype, tuple(state))) or "frames"
    try:
        out = FS.checked_window(make, fill, drain, dtype, check, None if check is None else dict(frames=5, size=(64, 80)), log)
    except FS.CacheRangeError as e:
        out = e
    return out, events, log


def test_the_order_of_a_checked_window_on_a_fake_store():
    from eavsr_amd import framestore as FS
    fine = {"fp16": {"spatial": _record(), "backward_1": _record(flushed=3, subnormal=9)}, "bf16": {"spatial": _record(dtype="bf16")}}
    over = {"fp16": {"spatial": _record(max_abs=7e4, overflow=12), "backward_1": _record()}, "bf16": {"spatial": _record(dtype="bf16", max_abs=7e4)}}
    nan = {"fp16": {"spatial": _record(nonfinite=2)}, "bf16": {}}
    drain16, drainbf = ("drain", "fp16", ("backward_1",)), ("drain", "bf16", ("backward_1",))

    # no check: a store without a census, and nothing is logged
    out, events, log = _run(None, fine)
    assert out == "frames" and events == [("make", "fp16", False), ("fill", "fp16"), drain16, ("finish", "fp16")] and log == []

    # "report": the read-back comes after stage 3 and after finish(), whatever the census holds
    for keys in (fine, over, nan):
        out, events, log = _run("report", keys)
        assert out == "frames"
        assert events == [("make", "fp16", True), ("fill", "fp16"), drain16, ("finish", "fp16"), ("census", "fp16")]
        assert log == [dict(asked="fp16", used="fp16", fallback=False, frames=5, size=(64, 80), keys=keys["fp16"])]

    # "raise": the read-back comes before stage 3; a window in range goes on, one that is not never reaches drain
    out, events, log = _run("raise", fine)
    assert out == "frames" and events == [("make", "fp16", True), ("fill", "fp16"), ("census", "fp16"), drain16, ("finish", "fp16")]
    assert log == [dict(asked="fp16", used="fp16", fallback=False, frames=5, size=(64, 80), keys=fine["fp16"])]
    for keys in (over, nan):
        out, events, log = _run("raise", keys)
        assert isinstance(out, FS.CacheRangeError) and out.entry is log[0] and len(log) == 1 and log[0]["keys"] == keys["fp16"]
        assert events == [("make", "fp16", True), ("fill", "fp16"), ("census", "fp16"), ("finish", "fp16")]
    out, events, log = _run("raise", {"bf16": {"spatial": _record(dtype="bf16", nonfinite=1)}}, dtype="bf16")
    assert isinstance(out, FS.CacheRangeError) and log[0]["asked"] == "bf16"

    # "bf16": the same point; an overflow rebuilds the store ONCE, as bf16, and stages 1-2 run again before stage 3 runs once
    out, events, log = _run("bf16", fine)
    assert out == "frames" and events == [("make", "fp16", True), ("fill", "fp16"), ("census", "fp16"), drain16, ("finish", "fp16")]
    assert log[0]["fallback"] is False and log[0]["used"] == "fp16" and "keys_used" not in log[0]
    out, events, log = _run("bf16", over)
    assert out == "frames"
    assert events == [("make", "fp16", True), ("fill", "fp16"), ("census", "fp16"), ("finish", "fp16"),
                      ("make", "bf16", True), ("fill", "bf16"), drainbf, ("finish", "bf16"), ("census", "bf16")]
    assert log == [dict(asked="fp16", used="bf16", fallback=True, frames=5, size=(64, 80), keys=over["fp16"], keys_used=over["bf16"])]
    # inf / NaN going in is reported and triggers nothing: bf16 cannot cure it
    out, events, log = _run("bf16", nan)
    assert out == "frames" and [e[0] for e in events] == ["make", "fill", "census", "drain", "finish"]
    assert log[0]["fallback"] is False and log[0]["keys"]["spatial"]["nonfinite"] == 2


def test_the_error_names_the_keys_their_range_and_the_counts():
    from eavsr_amd import framestore as FS
    keys = {"spatial": _record(max_abs=70123.5, overflow=12, elements=4096), "spatial_d2": _record(),
            "forward_2": _record(max_abs=3.25, nonfinite=7, elements=512)}
    assert FS.out_of_range(keys) == ["spatial", "forward_2"]
    text = str(FS.CacheRangeError(dict(asked="fp16", used="fp16", fallback=False, frames=5, size=(64, 80), keys=keys)))
    assert "'fp16'" in text and "5 frames of 64 x 80" in text
    assert "spatial: max |x| 70123.5, 12 overflowed, 0 non-finite of 4096" in text
    assert "forward_2: max |x| 3.25, 0 overflowed, 7 non-finite of 512" in text
    assert "spatial_d2" not in text and "cache_check='bf16'" in text


def test_the_summary_of_a_run():
    from eavsr_amd import framestore as FS
    log = [dict(asked="fp16", used="bf16", fallback=True, frames=5, size=(64, 64), keys={"spatial": _record(max_abs=7e4, overflow=12, flushed=1)},
                keys_used={"spatial": _record(dtype="bf16", max_abs=7e4)}),
           dict(asked="fp16", used="fp16", fallback=False, frames=5, size=(64, 64),
                keys={"spatial": _record(max_abs=2.0, subnormal=5), "backward_1": _record(max_abs=9.0, flushed=2, nonfinite=1)})]
    assert FS.census_summary(log) == {"windows": 2, "fallbacks": 1, "max_abs": 7e4, "nonfinite": 1, "overflow": 12, "flushed": 3, "subnormal": 5}
    assert FS.census_summary([]) == {"windows": 0, "fallbacks": 0, "max_abs": 0.0, "nonfinite": 0, "overflow": 0, "flushed": 0, "subnormal": 0}


# ------------------------------------------------------------------------------------------------------------------ the stores
def test_a_store_with_a_census_counts_per_key(monkeypatch):
    """`DeviceStore16(census=True)` on CPU tensors with the kernel replaced by the numpy reference: every pack of a key adds into the
    key's row of ONE (7, 5) tensor, the elements are counted on the host, `census()` returns the keys that were put"""
    from eavsr_amd import framestore as FS, ops
    launches = []

    def fake(srcs, dsts, dtype, census):
        launches.append(census.data_ptr())
        for s, d in zip(srcs, dsts):
            d.copy_(s)
            got = R.census(s.numpy(), dtype)
            census[0] = max(int(census[0]), R.row(got)[0])
            census[1:] += torch.tensor(R.row(got)[1:])
        return dsts
    monkeypatch.setattr(ops, "pack16_census", fake)
    monkeypatch.setattr(ops, "pack16", lambda *a: pytest.fail("a store with a census packs with the census"))
    n, t = 1, 4
    store = FS.make_store("device", n, t, "cpu", dtype="fp16", census=True)
    assert type(store) is FS.DeviceStore16 and tuple(store._counts.shape) == (7, 5) and store._counts.dtype == torch.int64
    assert FS.CENSUS_KEYS == FS.PYR + ("backward_1", "forward_1", "backward_2", "forward_2") and all(map(FS.is_feature_key, FS.CENSUS_KEYS))
    assert store.census() == {}
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(2, 4, 8, 8, generator=g) * 3e4, torch.randn(2, 4, 8, 8, generator=g) * 1e-6
    store.put_range("spatial", 0, a)
    store.put_range("spatial", 2, b)
    store.put_range("lr", 0, torch.zeros(4, 3, 8, 8))                 # fp32 keys: no pack, no census
    store.put_range("flow_forward", 0, torch.full((3, 2, 8, 8), 1e9))
    store.new_branch("backward_1", torch.zeros(n, 4, 8, 8))
    outs = [torch.randn(1, 4, 8, 8, generator=g) * 1e5 for _ in range(t)]
    for i, o in enumerate(outs):
        store.put("backward_1", t - 1 - i, o)
    got = store.census()
    assert list(got) == ["spatial", "backward_1"]
    assert got["spatial"] == dict(R.add(R.census(a.numpy(), "fp16"), R.census(b.numpy(), "fp16")), dtype="fp16")
    assert got["backward_1"] == dict(R.add(*[R.census(o.numpy(), "fp16") for o in outs]), dtype="fp16")
    assert got["spatial"]["overflow"] > 0 and got["spatial"]["flushed"] > 0 and got["backward_1"]["elements"] == t * 256
    assert len(launches) == 2 + t and len(set(launches)) == 2       # two rows of the one tensor
    with pytest.raises(ValueError, match="census"):
        store.put_range("branch_0", 0, a)                            # a feature key without a row
    # the other ways of making a store
    plain = FS.make_store("device", n, t, "cpu", dtype="fp16")
    assert plain._counts is None
    with pytest.raises(RuntimeError, match="census=True"):
        plain.census()
    with pytest.raises(ValueError, match="census"):
        FS.make_store("device", n, t, "cpu", census=True)           # the fp32 stores round nothing
    assert FS.make_store.__kwdefaults__ == {"census": False}
    assert issubclass(FS.HostStore16, FS._Census) and not hasattr(FS.DeviceStore, "census") and not hasattr(FS.HostStore, "census")


# --------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_entry_point_is_declared_without_an_abi_bump_and_bound():
    from eavsr_amd import _native as N
    with open(os.path.join(ROOT, "include", "eavsr_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+EAVSR_ABI_VERSION\s+32\b", header) and N.ABI_VERSION == 32
    stable = header[:header.index("EXPERIMENTAL -- exported by the LAB build only")]
    m = re.search(r"^int eavsr_pack16_census\(([^;]*)\);", stable, flags=re.M)
    assert m, "eavsr_pack16_census is not declared in the stable section"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    res, argtypes = N.SIGNATURES["eavsr_pack16_census"]
    assert len(args) == len(argtypes) == 7 and args[5].startswith("uint64_t*")
    for a, t in zip(args, argtypes):
        assert (t is N.vp) == ("*" in a), (a, t)
        assert (t is N.i32) == a.startswith("int32_t"), (a, t)
    # pack16's arguments with the record put in before the stream
    assert argtypes[:5] + argtypes[6:] == N.SIGNATURES["eavsr_pack16"][1]
    lib = N.load()
    assert hasattr(lib, "eavsr_pack16_census") and lib.eavsr_abi_version() == 32
    with open(os.path.join(ROOT, "eavsr_amd", "csrc", "cache16.hip")) as f:
        source = f.read()
    assert "pack16_census_kernel" in source and '#include "cache16_census.h"' in source
    assert len(re.findall(r"void pack_passes\(", source)) == 1      # one body for both pack kernels
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        assert "eavsr_pack16_census" in f.read()
