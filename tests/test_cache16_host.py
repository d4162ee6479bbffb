"""The 16-bit feature cache of the long-clip path, everything that needs no GPU: `framestore.check_cache_dtype`, the option
function, the C-ABI declarations, how a segment list is split into launches, `nbytes()` against the 1360 h w formula, and a Python
transcription of the kernels' head / vector / tail cut (`ops.cache16_cut` / `cache16_item`) against numpy slicing."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_check_cache_dtype_in_all_its_spellings_and_its_refusals():
    from eavsr_amd import framestore as FS
    assert FS.check_cache_dtype(None) is None
    assert FS.check_cache_dtype("fp16") == FS.check_cache_dtype(torch.float16) == FS.check_cache_dtype(torch.half) == "fp16"
    assert FS.check_cache_dtype("bf16") == FS.check_cache_dtype(torch.bfloat16) == "bf16"
    for bad in ("fp32", "half", "FP16", "", 16, True, False, torch.float32, torch.float64, torch.int16, np.float16, ("fp16",)):
        with pytest.raises(ValueError, match="cache_dtype"):
            FS.check_cache_dtype(bad)
    assert FS.check_cache("device") == "device" and FS.check_cache("host") == "host"      # unchanged
    with pytest.raises(ValueError):
        FS.check_cache("fp16")
    assert FS.is_feature_key("spatial") and FS.is_feature_key("spatial_d4") and FS.is_feature_key("backward_1")
    assert not any(FS.is_feature_key(k) for k in FS.FLOW_KEYS + ("lr",))


def test_the_option_function_reads_opt_then_env_then_default(monkeypatch):
    from eavsr_amd.eavsrp_model import cache_dtype_option, long_clip_options
    monkeypatch.delenv("EAVSR_CACHE_DTYPE", raising=False)
    assert cache_dtype_option() is None and cache_dtype_option(Namespace()) is None and cache_dtype_option(Namespace(cache_dtype=None)) is None
    assert cache_dtype_option(Namespace(cache_dtype="fp16")) == "fp16" and cache_dtype_option(Namespace(cache_dtype=torch.bfloat16)) == "bf16"
    monkeypatch.setenv("EAVSR_CACHE_DTYPE", "bf16")
    assert cache_dtype_option() == "bf16" and cache_dtype_option(Namespace()) == "bf16"
    assert cache_dtype_option(Namespace(cache_dtype="fp16")) == "fp16"      # the options win
    assert long_clip_options(Namespace()) == (None, False)                  # its two values, as before
    monkeypatch.setenv("EAVSR_CACHE_DTYPE", "")
    assert cache_dtype_option() is None
    monkeypatch.setenv("EAVSR_CACHE_DTYPE", "fp32")
    with pytest.raises(ValueError, match="EAVSR_CACHE_DTYPE"):
        cache_dtype_option()
    with pytest.raises(ValueError, match="EAVSR_CACHE_DTYPE"):
        long_clip_options(Namespace())      # validated with the others
    assert cache_dtype_option(Namespace(cache_dtype="bf16")) == "bf16"      # a bad environment is not read where the options decide
    for bad in ("fp32", 16, True, torch.float32):
        with pytest.raises(ValueError, match="opt.cache_dtype"):
            cache_dtype_option(Namespace(cache_dtype=bad))


def test_arguments_are_refused_before_anything_runs(monkeypatch):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRP, EAVSRPModel
    monkeypatch.delenv("EAVSR_CACHE_DTYPE", raising=False)
    net = EAVSRP.__new__(EAVSRP)
    x = torch.zeros(1, 2, 3, 96, 112)
    with torch.no_grad():
        for bad in ("fp32", torch.float32, 16, True):
            for call in (lambda: EAVSRP.forward_long(net, x, cache_dtype=bad), lambda: EAVSRP.forward_tiled(net, x, 64, cache_dtype=bad),
                         lambda: EAVSRP.forward_segments_padded(net, x, [(0, 2, 0, 2)], None, cache_dtype=bad),
                         lambda: EAVSRP.forward_cached(net, x, bad), lambda: EAVSRP.forward_cached(net, x, bad, ensemble=2)):
                with pytest.raises(ValueError, match="cache_dtype"):
                    call()
    for bad in ("fp32", torch.float64, 8):
        with pytest.raises(ValueError, match="cache_dtype"):
            harness.super_resolve(None, ["/nonexistent/frame.png"], cache_dtype=bad)      # ... before a file is read
    with pytest.raises(ValueError, match="opt.cache_dtype"):
        harness.super_resolve(Namespace(opt=Namespace(cache_dtype="fp8")), x[0])
    with pytest.raises(ValueError, match="opt.cache_dtype"):      # a training wrapper refuses the option before it builds anything
        EAVSRPModel(Namespace(scale=4, isTrain=True, cache_dtype="fp16", gpu_ids=[0]))


def test_entry_points_are_declared_without_an_abi_bump_and_bound():
    from eavsr_amd import _native as N, build, ops
    with open(os.path.join(ROOT, "include", "eavsr_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+EAVSR_ABI_VERSION\s+32\b", header) and N.ABI_VERSION == 32
    stable = header[:header.index("EXPERIMENTAL -- exported by the LAB build only")]
    for name in ("eavsr_pack16", "eavsr_unpack16"):
        m = re.search(r"^int %s\(([^;]*)\);" % name, stable, flags=re.M)
        assert m, f"{name} is not declared in the stable section"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = N.SIGNATURES[name]
        assert len(args) == len(argtypes) == 6
        for a, t in zip(args, argtypes):
            assert (t is N.vp) == ("*" in a), (a, t)
            assert (t is N.i32) == a.startswith("int32_t"), (a, t)
    assert "eavsr_cache16_max_segments" in N.SIGNATURES and re.search(r"^int eavsr_cache16_max_segments\(void\);", stable, flags=re.M)
    m = re.search(r"#define\s+EAVSR_CACHE16_MAX_SEGMENTS\s+(\d+)", stable)
    assert m and int(m.group(1)) == ops.CACHE16_MAX_SEGMENTS
    lib = N.load()      # the library is built on import of the package's build step; the constant is the one the kernels were built with
    assert lib.eavsr_cache16_max_segments() == ops.CACHE16_MAX_SEGMENTS and lib.eavsr_abi_version() == 32
    assert any(p.endswith(os.sep + "cache16.hip") for p in build.sources()) and any(p.endswith("cache16.hip") for p in build.sources(lab=True))
    with open(os.path.join(ROOT, "eavsr_amd", "csrc", "cache16.hip")) as f:
        source = f.read()
    assert "__shared__" not in source and "atomic" not in source.lower().replace("no atomics", "")
    m = re.search(r"kThreads = (\d+);", source), re.search(r"kUnroll = (\d+);", source)
    assert int(m[0].group(1)) * int(m[1].group(1)) == ops.CACHE16_BLOCK_ITEMS
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert "eavsr_pack16" in text and "eavsr_unpack16" in text


def test_a_segment_list_is_split_into_launches_of_at_most_the_maximum():
    from eavsr_amd import ops
    M = ops.CACHE16_MAX_SEGMENTS
    assert ops.cache16_batches(0) == []
    assert ops.cache16_batches(1) == [(0, 1)]
    assert ops.cache16_batches(M) == [(0, M)]
    assert ops.cache16_batches(M + 1) == [(0, M), (M, M + 1)]
    assert ops.cache16_batches(2 * M + 3) == [(0, M), (M, 2 * M), (2 * M, 2 * M + 3)]
    for nseg in (0, 1, M, M + 1, 2 * M + 3):
        parts = ops.cache16_batches(nseg)
        assert [i for a, b in parts for i in range(a, b)] == list(range(nseg)) and all(0 < b - a <= M for a, b in parts)
    with pytest.raises(ValueError):
        ops.cache16_batches(-1)
    # no GPU: the wrappers refuse host tensors, wrong dtypes and views before anything is launched
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.pack16([torch.zeros(8)], [torch.zeros(8, dtype=torch.float16)], "fp16")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.unpack16([torch.zeros(8, dtype=torch.bfloat16)], [torch.zeros(8)])
    with pytest.raises(ValueError):
        ops.pack16([torch.zeros(8)], [torch.zeros(8, dtype=torch.float16)], "fp32")
    with pytest.raises(ValueError):
        ops.pack16([torch.zeros(8)], [], "fp16")
    with pytest.raises(ValueError):
        ops.unpack16([torch.zeros(8)], [torch.zeros(8)])
    with pytest.raises(TypeError):
        ops.pack16([np.zeros(8, np.float32)], [torch.zeros(8, dtype=torch.float16)], "fp16")
    assert ops.pack16([], [], "bf16") == [] and ops.unpack16([], []) == []


def test_the_cut_of_a_segment_against_numpy_slicing():
    """lengths 0 .. 40 at every misalignment 0 .. 7 of the 16-bit side: the items of `cache16_cut` / `cache16_item` -- vectors of 8 that
    start on a 16-byte boundary of the 16-bit side, single elements before and behind them -- cover the segment exactly once, in the
    kernels' item order, and converting item by item is converting the slice"""
    from eavsr_amd import ops
    rng = np.random.default_rng(0)
    for mis in range(8):
        for n in range(41):
            head, nvec, tail = ops.cache16_cut(mis, n)
            assert head + 8 * nvec + tail == n and 0 <= head <= 7 and 0 <= tail <= 7
            assert head == min((8 - mis) % 8, n) and (nvec == 0 or (mis + head) % 8 == 0)
            assert nvec == (n - head) // 8
            base = rng.standard_normal(mis + n + 8).astype(np.float32)
            src = base[mis:mis + n]                                # the slice a test reaches the misalignment through
            out = np.full(mis + n + 8, np.float16(-7), np.float16)
            seen = np.zeros(n, np.int32)
            items = nvec + head + tail
            for i in range(items + 3):                              # (the lanes past the last item do nothing)
                a, b = ops.cache16_item(i, head, nvec, tail)
                if i < nvec:
                    assert b - a == 8 and (mis + a) % 8 == 0        # one 16-byte access on the 16-bit side
                elif i < items:
                    assert b - a == 1 and (a < head or a >= head + 8 * nvec)
                else:
                    assert a == b
                out[mis + a:mis + b] = src[a:b].astype(np.float16)
                seen[a:b] += 1
            assert np.all(seen == 1)
            assert np.array_equal(out[mis:mis + n].view(np.uint16), src.astype(np.float16).view(np.uint16))
            assert np.all(out[:mis] == np.float16(-7)) and np.all(out[mis + n:] == np.float16(-7))      # nothing outside the segment
            assert ops.cache16_passes(mis, n) == -(-items // ops.CACHE16_BLOCK_ITEMS)
    assert ops.cache16_cut(0, 2 ** 33 + 5) == (0, 2 ** 30, 5) and ops.cache16_passes(3, 2 ** 33) == -(-(2 ** 30 - 1 + 5 + 3) // 1024)
    for bad in ((-1, 4), (8, 4), (0, -1)):
        with pytest.raises(ValueError):
            ops.cache16_cut(*bad)


def _fill(store, n, t, h, w, put):
    """what `forward_long` puts, by shape: the pyramid and LR frames in two chunks, the flows, four branch buffers"""
    from eavsr_amd import framestore as FS
    z = lambda *s: torch.zeros(*s)
    for a, b in ((0, 2), (2, t)):
        put(store, "lr", a, z((b - a) * n, 3, h, w))
        for key, d in zip(FS.PYR, (1, 2, 4)):
            put(store, key, a, z((b - a) * n, 64, h // d, w // d))
    for key in FS.FLOW_KEYS:
        put(store, key, 0, z((t - 1) * n, 2, h, w))
    for i in (1, 2):
        for d in ("backward", "forward"):
            store.new_branch(f"{d}_{i}", z(n, 64, h, w))


def test_nbytes_against_the_1360_h_w_formula(monkeypatch):
    from eavsr_amd import framestore as FS
    n, t, h, w = 2, 5, 16, 24
    want32, want16 = FS.expected_nbytes(n, t, h, w), FS.expected_nbytes(n, t, h, w, dtype="bf16")
    feature = [k for k in want32 if k != "total" and FS.is_feature_key(k)]
    assert sum(want32[k] for k in feature) == 1360 * h * w * n * t and len(feature) == 7
    assert sum(want16[k] for k in feature) == 680 * h * w * n * t
    for k in FS.FLOW_KEYS:
        assert want32[k] == want16[k] == 2 * h * w * 4 * n * (t - 1)      # the flows at full size
    assert want32["lr"] == want16["lr"] == 12 * h * w * n * t
    assert want32["total"] - want16["total"] == 680 * h * w * n * t
    assert FS.expected_nbytes(1, 50, 540, 960)["total"] - FS.expected_nbytes(1, 50, 540, 960, dtype="fp16")["total"] == 680 * 540 * 960 * 50

    # the fp32 device store takes CPU tensors as they are
    store = FS.make_store("device", n, t, "cpu")
    assert type(store) is FS.DeviceStore
    _fill(store, n, t, h, w, lambda s, key, first, x: s.put_range(key, first, x))
    assert store.nbytes() == want32
    # the 16-bit device store rounds with a kernel: here the rounding is torch's, the bookkeeping is the class's own
    for name, dt in FS.CACHE_DTYPES.items():
        store = FS.make_store("device", n, t, "cpu", dtype=dt)
        assert type(store) is FS.DeviceStore16 and store.cache == "device" and store.cache_dtype == name and store.out_slot("backward_1", 0) is None
        monkeypatch.setattr(store, "_pack", lambda src, dst: dst.copy_(src))
        _fill(store, n, t, h, w, lambda s, key, first, x: s.put_range(key, first, x))
        assert store.nbytes() == FS.expected_nbytes(n, t, h, w, dtype=name)
        for k in feature:
            assert store.nbytes()[k] * 2 == want32[k]
        assert store.get("flow_forward", 1).dtype == torch.float32 and store.get_range("lr", 1, 4).shape[0] == 3 * n
    # dtype=None is today's object for both caches (the host store opens a stream: its class is all that is checked here)
    assert FS.make_store.__defaults__ == (None,) and issubclass(FS.HostStore16, FS.HostStore) and FS.HostStore16.cache == "host"
    with pytest.raises(ValueError):
        FS.make_store("device", 1, 1, "cpu", dtype="fp32")
    with pytest.raises(ValueError):
        FS.make_store("disk", 1, 1, "cpu", dtype="fp16")


def test_the_16_bit_device_store_follows_the_schedule_with_one_widening_per_step(monkeypatch):
    """`DeviceStore16` on CPU tensors with torch's conversions in place of the two kernels: what a step reads is in the window when
    the step runs, everything a step fetches is ONE unpack call, `done` evicts, and a tensor comes back as x.to(dtype).float()"""
    from eavsr_amd import framestore as FS, ops
    n, t, h, w = 1, 4, 8, 8
    calls = []

    def unpack(srcs, dsts):
        calls.append(len(srcs))
        for s, d in zip(srcs, dsts):
            d.copy_(s)
        return dsts
    monkeypatch.setattr(ops, "unpack16", unpack)
    monkeypatch.setattr(ops, "pack16", lambda srcs, dsts, dtype: [d.copy_(s) for s, d in zip(srcs, dsts)])
    g = torch.Generator().manual_seed(0)
    store = FS.make_store("device", n, t, "cpu", dtype="bf16")
    held = {}
    for key, d in zip(FS.PYR, (1, 2, 4)):
        held[key] = torch.randn(t * n, 4, h // d, w // d, generator=g)
        store.put_range(key, 0, held[key])
    flows = torch.randn((t - 1) * n, 2, h, w, generator=g)
    store.put_range("flow_backward", 0, flows)
    reads = FS.propagate_reads(t, True, ())
    schedule = FS.prefetch_schedule(reads)
    store.begin(schedule)
    assert calls == [3]      # the prologue: three pyramid levels, one launch
    store.new_branch("backward_1", torch.zeros(n, 4, h, w))
    for i, items in enumerate(reads):
        before = len(calls)
        store.step(i)
        assert len(calls) - before == (1 if any(FS.is_feature_key(k) for k, _ in schedule.fetch[i]) else 0)
        for key, idx in items:
            got = store.get(key, idx)
            want = flows[idx:idx + 1] if key == "flow_backward" else held[key][idx:idx + 1].to(torch.bfloat16).float()
            assert got.dtype == torch.float32 and torch.equal(got, want), (i, key, idx)
        out = torch.randn(n, 4, h, w, generator=g)
        store.put("backward_1", t - 1 - i, out)
        held.setdefault("backward_1", torch.zeros(t * n, 4, h, w))[t - 1 - i] = out[0]
        store.done(i)
    assert store._window == {} and store.peak_window_items <= FS.window_bound(0)["items"]
    assert torch.equal(store.get_range("backward_1", 1, 3), held["backward_1"][1:3].to(torch.bfloat16).float())
    assert torch.equal(store.get_range("spatial", 0, t), held["spatial"].to(torch.bfloat16).float())
