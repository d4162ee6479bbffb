"""The census of the 16-bit feature cache on the GPU (`pytest -m gpu`, DESIGN 7n addendum): `ops.pack16_census` against the numpy
reference (tests/census_ref.py) -- the five numbers equal, the 16-bit output `ops.pack16`'s bit for bit --, the two stores with
census=True against the reference applied to what was put, and `cache_check` through `forward_long` and the paths built on it, on
the synthetic weights and on a copy of them whose encoder overflows fp16 in one channel."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import census_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
HOT_CHANNEL, HOT_BIAS = 3, 7e4      # one output channel of the encoder's last convolution, pushed past fp16's 65520


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    yield
    _NETS.clear()
    _SHARED.clear()
    torch.cuda.empty_cache()


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _launches(ops, fn):
    with ops.profile() as prof:
        try:
            out = fn()
        except Exception as e:      # noqa: BLE001 -- handed back to the caller, with what was launched on the way
            out = e
    return out, {k: v["calls"] for k, v in prof.summary().items()}


def _spread(count, seed, lo=-150, hi=120):
    """finite fp32 values over nearly all binades: in both formats some are flushed and some land among the subnormals, many
    overflow fp16, and the fp32 subnormals are there too"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(count) * np.exp2(rng.integers(lo, hi, count))).astype(np.float32)


def _census_of(ops, cuda, x, name, census=None):
    """(16-bit output, the record as read back) of one call on a host array"""
    src = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    dst = torch.empty(src.shape, dtype=DTYPES[name], device=cuda)
    census = torch.zeros(5, dtype=torch.int64, device=cuda) if census is None else census
    assert ops.pack16_census([src], [dst], name, census)[0] is dst
    return dst, census


def _plain(ops, cuda, x, name):
    src = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    dst = torch.empty(src.shape, dtype=DTYPES[name], device=cuda)
    ops.pack16([src], [dst], name)
    return dst


def _same_numbers(census, elements, name, want, ops):
    got = ops.census_record(census.cpu(), elements, name)
    assert got == dict(want, dtype=name), (got, want)


# ------------------------------------------------------------------------------------------------------------------ the op
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_every_16_bit_pattern_and_the_hand_built_edges(ops, cuda, name):
    """all 65 536 fp16 and all 65 536 bf16 patterns widened to fp32, with the hand-built boundary values of both formats scattered at
    random positions among them: the five numbers, and the output against `ops.pack16` and (NaN aside) against numpy"""
    pat = torch.arange(65536, dtype=torch.int32)
    f16 = pat.to(torch.int16).view(torch.float16).float().numpy()
    bf16 = (pat << 16).view(torch.float32).numpy()
    x = np.concatenate([f16, bf16]).astype(np.float32)
    rng = np.random.default_rng(5)
    edges = R.BOUNDARY_BITS + R.BF16_TINY_BITS
    where = rng.choice(x.size, 4 * len(edges), replace=False)
    x.view(np.uint32)[where] = np.tile(np.array(edges, np.uint32), 4)
    want = R.census(x, name)
    assert want["overflow"] > 0 and want["flushed"] > 0 and want["subnormal"] > 0 and want["nonfinite"] > 2000
    dst, census = _census_of(ops, cuda, x, name)
    _same_numbers(census, x.size, name, want, ops)
    assert torch.equal(_bits16(dst), _bits16(_plain(ops, cuda, x, name)))
    ok = ~np.isnan(x)
    assert np.array_equal(_bits16(dst).numpy().view(np.uint16)[ok], R.round16(x, name)[ok])
    # the edges alone, one element per launch into one record each: nothing depends on the neighbours
    for bits in edges:
        one = np.array([bits], np.uint32).view(np.float32)
        _, c = _census_of(ops, cuda, one, name)
        _same_numbers(c, 1, name, R.census(one, name), ops)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_lengths_1_to_1100_at_every_misalignment(ops, cuda, name):
    """head, vectors, tail and the end of a workgroup pass at 1024 items; the fp32 side's alignment moves with the 16-bit side's, so
    its 16-, 8- and 4-byte reads all run.  One record per length; the outputs against ONE `ops.pack16` call over the same layout"""
    slot, lengths = 1120, list(range(1, 1101))
    x = _spread(len(lengths) * slot + 8, 11)
    src = torch.from_numpy(x).to(cuda)
    for mis in range(8):
        out = torch.full((len(lengths) * slot + 8,), -7.0, dtype=DTYPES[name], device=cuda)
        ref = out.clone()
        census = torch.zeros((len(lengths), 5), dtype=torch.int64, device=cuda)
        assert (out.data_ptr() // 2) % 8 == 0
        srcs = [src[i * slot + mis:i * slot + mis + n] for i, n in enumerate(lengths)]
        for i, n in enumerate(lengths):
            ops.pack16_census([srcs[i]], [out[i * slot + mis:i * slot + mis + n]], name, census[i])
        ops.pack16(srcs, [ref[i * slot + mis:i * slot + mis + n] for i, n in enumerate(lengths)], name)
        assert torch.equal(_bits16(out), _bits16(ref)), mis      # also: nothing outside a segment was written
        rows = census.cpu().tolist()
        for i, n in enumerate(lengths):
            want = R.census(x[i * slot + mis:i * slot + mis + n], name)
            assert rows[i] == R.row(want), (mis, n, rows[i], want)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_past_the_grid_cap_the_registers_carry_across_passes(ops, cuda, name):
    """2^24 + 13 elements: 2 097 153 vectors + 5 scalars are 2049 passes of 1024 items on 2048 workgroups -- the grid stride runs,
    and workgroup 0 carries its tally from its first pass into its second"""
    n = 2 ** 24 + 13
    assert ops.cache16_passes(0, n) == 2049
    g = torch.Generator(device=cuda).manual_seed(7)
    src = torch.randn(n, generator=g, device=cuda) * torch.exp2(torch.randint(-140, 120, (n,), generator=g, device=cuda).float())
    src[-3] = float("inf")
    src[1024 * 8 * 2048 + 5] = 3e38      # in the pass past the cap
    dst = torch.empty(n, dtype=DTYPES[name], device=cuda)
    census = torch.zeros(5, dtype=torch.int64, device=cuda)
    _, launched = _launches(ops, lambda: ops.pack16_census([src], [dst], name, census))
    assert launched == {"pack16_census": 1}
    ref = torch.empty_like(dst)
    ops.pack16([src], [ref], name)
    assert torch.equal(dst.view(torch.int16), ref.view(torch.int16))
    want = R.census(src.cpu().numpy(), name)
    assert want["max_abs"] == float(np.float32(3e38)) and want["nonfinite"] == 1 and want["flushed"] > 0 and want["subnormal"] > 0
    _same_numbers(census, n, name, want, ops)
    again = torch.zeros(5, dtype=torch.int64, device=cuda)
    ops.pack16_census([src], [dst], name, again)
    assert torch.equal(again, census)      # integer max and add: two calls agree


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_lists_accumulation_and_the_degenerate_sources(ops, cuda, name):
    dt = DTYPES[name]
    # a list with an empty segment, and 19 segments: two launches into one record
    sizes = [5, 0, 1031, 8, 64, 1, 9000, 17, 0, 3, 2048, 777, 12, 1025, 33, 2, 40000, 7, 129]
    assert len(sizes) == 19 > ops.CACHE16_MAX_SEGMENTS
    xs = [_spread(n, 20 + i) for i, n in enumerate(sizes)]
    srcs = [torch.from_numpy(x).to(cuda) for x in xs]
    dsts = [torch.empty(n, dtype=dt, device=cuda) for n in sizes]
    census = torch.zeros((3, 5), dtype=torch.int64, device=cuda)      # a row of a larger tensor
    _, launched = _launches(ops, lambda: ops.pack16_census(srcs, dsts, name, census[1]))
    assert launched == {"pack16_census": 2}
    want = R.add(*[R.census(x, name) for x in xs])
    _same_numbers(census[1], sum(sizes), name, want, ops)
    assert int(census[0].abs().sum()) == 0 and int(census[2].abs().sum()) == 0      # the neighbouring rows are untouched
    refs = [torch.empty(n, dtype=dt, device=cuda) for n in sizes]
    ops.pack16(srcs, refs, name)
    assert all(torch.equal(_bits16(d), _bits16(r)) for d, r in zip(dsts, refs))
    _, launched = _launches(ops, lambda: ops.pack16_census(srcs[:3], dsts[:3], name, census[2]))
    assert launched == {"pack16_census": 1}
    _same_numbers(census[2], sum(sizes[:3]), name, R.add(*[R.census(x, name) for x in xs[:3]]), ops)
    # a record that already holds counts: the launch adds, and keeps a larger maximum
    held = torch.tensor([0x7F000000, 5, 6, 7, 8], dtype=torch.int64, device=cuda)
    ops.pack16_census(srcs[2:3], dsts[2:3], name, held)
    one = R.row(R.census(xs[2], name))
    assert held.tolist() == [0x7F000000] + [a + b for a, b in zip((5, 6, 7, 8), one[1:])]
    held = torch.tensor([1, 0, 0, 0, 0], dtype=torch.int64, device=cuda)
    ops.pack16_census(srcs[2:3], dsts[2:3], name, held)
    assert held.tolist() == one
    # nothing to convert: nothing is launched, the record stays
    _, launched = _launches(ops, lambda: ops.pack16_census([srcs[1]], [dsts[1]], name, held))
    assert launched == {} and held.tolist() == one
    assert ops.pack16_census([], [], name, held) == []
    # only zeros: max_abs 0 and nothing else; only NaN: max_abs 0, all non-finite
    zeros = np.zeros(3000, np.float32)
    zeros[::2] = -0.0
    _, c = _census_of(ops, cuda, zeros, name)
    assert c.tolist() == [0, 0, 0, 0, 0]
    _, c = _census_of(ops, cuda, np.full(3000, np.nan, np.float32), name)
    assert c.tolist() == [0, 3000, 0, 0, 0]


def test_the_op_refuses_before_anything_is_launched(ops, cuda):
    x = torch.zeros(64, device=cuda)
    d = torch.zeros(64, dtype=torch.float16, device=cuda)
    ok = torch.zeros(5, dtype=torch.int64, device=cuda)
    for fn in (lambda: ops.pack16_census([x], [d], "fp16", torch.zeros(5, dtype=torch.int32, device=cuda)),
               lambda: ops.pack16_census([x], [d], "fp16", torch.zeros(6, dtype=torch.int64, device=cuda)),
               lambda: ops.pack16_census([x], [d], "fp16", torch.zeros((5, 2), dtype=torch.int64, device=cuda)[:, 0]),
               lambda: ops.pack16_census([x], [d], "fp16", torch.zeros(5, dtype=torch.int64)),
               lambda: ops.pack16_census([x], [d], "fp32", ok),
               lambda: ops.pack16_census([x], [d], "bf16", ok),
               lambda: ops.pack16_census([x[::2]], [d[:32]], "fp16", ok),
               lambda: ops.pack16_census([x], [d[:63]], "fp16", ok),
               lambda: ops.pack16_census([x], [d], "fp16", None)):
        out, launched = _launches(ops, fn)
        assert isinstance(out, (ValueError, RuntimeError, TypeError)) and launched == {}, out
    assert ok.tolist() == [0] * 5


# --------------------------------------------------------------------------------------------------------------- the stores
@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("cache", ["device", "host"])
def test_a_store_with_a_census_counts_what_was_put_per_key(ops, cuda, cache, name):
    from eavsr_amd import framestore as FS
    n, t, c, h, w = 2, 4, 5, 12, 20
    store = FS.make_store(cache, n, t, cuda, dtype=name, census=True)
    assert type(store) is (FS.HostStore16 if cache == "host" else FS.DeviceStore16) and store.census() == {}
    put = {}
    for i, (key, d) in enumerate(zip(FS.PYR, (1, 2, 4))):
        x = torch.from_numpy(_spread(t * n * c * (h // d) * (w // d), 30 + i).reshape(t * n, c, h // d, w // d))
        for a, b in ((0, 3), (3, t)):      # two chunks: two launches into the key's row
            _, launched = _launches(ops, lambda: store.put_range(key, a, x[a * n:b * n].to(cuda)))
            assert launched == {"pack16_census": 1}
        put[key] = x
    _, launched = _launches(ops, lambda: store.put_range("flow_backward", 0, torch.full(((t - 1) * n, 2, h, w), 1e9, device=cuda)))
    assert "pack16_census" not in launched and "pack16" not in launched      # fp32 keys: no rounding, no census
    store.new_branch("forward_2", torch.zeros(n, c, h, w, device=cuda))
    outs = torch.from_numpy(_spread(t * n * c * h * w, 40).reshape(t, n, c, h, w))
    for idx in range(t):
        store.put("forward_2", idx, outs[idx].to(cuda))
    put["forward_2"] = outs
    got = store.census()
    assert list(got) == list(FS.PYR) + ["forward_2"]
    for key, x in put.items():
        assert got[key] == dict(R.census(x.numpy(), name), dtype=name), key
    assert got["spatial"]["flushed"] > 0 and (name == "bf16" or got["spatial"]["overflow"] > 0)
    # what the store returns is what a store without a census returns
    assert torch.equal(_bits32(store.get_range("spatial", 1, 3)), _bits32(put["spatial"][n:3 * n].to(DTYPES[name]).float()))
    store.finish()
    plain = FS.make_store(cache, n, t, cuda, dtype=name)
    _, launched = _launches(ops, lambda: plain.put_range("spatial", 0, put["spatial"].to(cuda)))
    assert launched == {"pack16": 1}      # census=False: today's launch
    plain.finish()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the model
_NETS = {}
_SHARED = {}


def _net(cuda, tag="x4"):
    """"x4": the synthetic weights; "hot": a network of its own with the same weights and HOT_BIAS added to one bias of the encoder's tail"""
    if tag not in _NETS:
        from eavsr_amd.eavsrp_model import EAVSRP
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4), None)
        net.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
        net = net.to(cuda).eval()
        if tag == "hot":
            with torch.no_grad():
                net.encoder.tail.bias[HOT_CHANNEL] += HOT_BIAS
        _NETS[tag] = net
    return _NETS[tag]


def _clip_u8(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return (big[..., :h, :w] * 255).round().to(torch.uint8).contiguous()


def _shared(cuda, tag, name, cache="device"):
    """`forward_long(cache_dtype=name)` of the 1 x 5 x 64 x 64 clip without a check, computed once and never written to"""
    key = (tag, name, cache)
    if key not in _SHARED:
        with torch.no_grad():
            _SHARED[key] = _net(cuda, tag).forward_long(_clip_u8(1, 5, 64, 64, 41).to(cuda), frame_chunk=2, cache=cache, cache_dtype=name)
    return _SHARED[key]


def _put_per_key(monkeypatch, fn):
    """run fn with every tensor a store's census takes recorded on the host, per key, in the order it was put"""
    from eavsr_amd import framestore as FS
    seen = {}
    row = FS._Census._census_row

    def recording(self, key, src):
        seen.setdefault(key, []).append(src.detach().cpu().numpy().copy())
        return row(self, key, src)
    with monkeypatch.context() as m:
        m.setattr(FS._Census, "_census_row", recording)
        out = fn()
    return out, seen


def _pyramid_of_an_fp32_run(monkeypatch, net, x):
    """the pyramid levels an fp32 `forward_long` puts into its store (the encoder does not read the store: they are the 16-bit run's)"""
    from eavsr_amd import framestore as FS
    seen = {}

    class Recording(FS.DeviceStore):
        def put_range(self, key, first, frames):
            if key in FS.PYR:
                seen.setdefault(key, []).append(frames.detach().cpu().numpy().copy())
            super().put_range(key, first, frames)
    with monkeypatch.context() as m:
        m.setattr(FS, "make_store", lambda cache, n, t, device, dtype=None: Recording(n, t, device))
        net.forward_long(x, frame_chunk=2)
    return seen


@pytest.mark.parametrize("cache", ["device", "host"])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_report_changes_no_frame_and_counts_what_went_into_the_store(ops, cuda, monkeypatch, name, cache):
    """1 x 5 x 64 x 64, frame_chunk=2, the synthetic weights: "report" is cache_check=None bit for bit with `pack16_census` in
    `pack16`'s place and no other launch changed; its census is the reference applied to every tensor the store took, per key, and
    for the pyramid -- which does not depend on the store -- to the features of an fp32 run"""
    from eavsr_amd import framestore as FS
    net = _net(cuda)
    x = _clip_u8(1, 5, 64, 64, 41).to(cuda)
    want = _shared(cuda, "x4", name, cache)
    with torch.no_grad():
        net.cache_census.clear()
        (got, launched), put = _put_per_key(monkeypatch, lambda: _launches(
            ops, lambda: net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype=name, cache_check="report")))
        assert torch.equal(_bits32(got), _bits32(want))
        _, plain = _launches(ops, lambda: net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype=name))
        assert "pack16" not in launched and launched["pack16_census"] == plain["pack16"]
        assert {k: v for k, v in launched.items() if k != "pack16_census"} == {k: v for k, v in plain.items() if k != "pack16"}
        assert len(net.cache_census) == 1
        entry = net.cache_census[0]
        assert {k: entry[k] for k in ("asked", "used", "fallback", "frames", "size")} == dict(asked=name, used=name, fallback=False,
                                                                                              frames=5, size=(64, 64))
        assert list(entry["keys"]) == list(FS.CENSUS_KEYS)
        for key in FS.CENSUS_KEYS:
            assert entry["keys"][key] == dict(R.add(*[R.census(p, name) for p in put[key]]), dtype=name), key
            assert entry["keys"][key]["overflow"] == 0 and entry["keys"][key]["nonfinite"] == 0 and entry["keys"][key]["max_abs"] > 0
        assert entry["keys"]["spatial"]["elements"] == 5 * 64 * 64 * 64 and entry["keys"]["spatial_d4"]["elements"] == 5 * 64 * 16 * 16
        if cache == "device":
            fp32 = _pyramid_of_an_fp32_run(monkeypatch, net, x)
            for key in FS.PYR:
                assert entry["keys"][key] == dict(R.add(*[R.census(p, name) for p in fp32[key]]), dtype=name), key
        # "raise" and (fp16) "bf16" on a window that is in range: the same frames again, one more entry each
        checks = ("raise", "bf16") if name == "fp16" else ("raise",)
        for check in checks:
            assert torch.equal(net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype=name, cache_check=check), want)
        assert len(net.cache_census) == 1 + len(checks)
        assert all(e["keys"] == entry["keys"] and e["fallback"] is False and "keys_used" not in e for e in net.cache_census)
        net.cache_census.clear()


@pytest.mark.parametrize("cache", ["device", "host"])
def test_an_encoder_that_overflows_fp16_is_reported_refused_or_run_in_bf16(ops, cuda, cache):
    """the same clip on the network whose encoder adds 7e4 to one output channel: every element of that channel of `spatial` rounds
    to inf in fp16"""
    from eavsr_amd import framestore as FS
    net = _net(cuda, "hot")
    x = _clip_u8(1, 5, 64, 64, 41).to(cuda)
    want_bf16 = _shared(cuda, "hot", "bf16", cache)
    assert torch.isfinite(want_bf16).all()
    sunk = []
    with torch.no_grad():
        net.cache_census.clear()
        # "raise": a CacheRangeError, a ValueError, and the sink has seen nothing
        with pytest.raises(FS.CacheRangeError, match="spatial: max") as info:
            net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype="fp16", cache_check="raise", sink=lambda a, sr: sunk.append(a))
        assert sunk == [] and isinstance(info.value, ValueError) and info.value.entry is net.cache_census[0]
        spatial = net.cache_census[0]["keys"]["spatial"]
        assert spatial["overflow"] >= 5 * 64 * 64 and spatial["max_abs"] > 65520.0 and spatial["nonfinite"] == 0
        assert "spatial" in FS.out_of_range(net.cache_census[0]["keys"])
        # "bf16": forward_long(cache_dtype="bf16"), bit for bit; the entry keeps the fp16 attempt's census
        got = net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype="fp16", cache_check="bf16")
        assert torch.equal(_bits32(got), _bits32(want_bf16))
        entry = net.cache_census[1]
        assert entry["asked"] == "fp16" and entry["used"] == "bf16" and entry["fallback"] is True
        assert entry["keys"]["spatial"] == spatial and entry["keys"]["spatial"]["overflow"] > 0
        assert entry["keys_used"]["spatial"]["overflow"] == 0 and entry["keys_used"]["spatial"]["dtype"] == "bf16"
        assert entry["keys_used"]["spatial"]["max_abs"] == spatial["max_abs"] and list(entry["keys_used"]) == list(FS.CENSUS_KEYS)
        # with a sink: every frame arrives once, from the bf16 run
        net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype="fp16", cache_check="bf16", sink=lambda a, sr: sunk.append((a, sr)))
        assert [a for a, _ in sunk] == [0, 2, 4] and torch.equal(torch.cat([sr for _, sr in sunk], 1), want_bf16)
        # "report": the frames of cache_check=None, non-finite as they are, and the census says why
        got = net.forward_long(x, frame_chunk=2, cache=cache, cache_dtype="fp16", cache_check="report")
        assert torch.equal(_bits32(got), _bits32(_shared(cuda, "hot", "fp16", cache))) and not torch.isfinite(got).all()
        entry = net.cache_census[3]
        assert entry["fallback"] is False and entry["used"] == "fp16" and entry["keys"]["spatial"] == spatial
        assert len(net.cache_census) == 4
        net.cache_census.clear()


def test_tiles_and_the_ensemble_make_one_entry_per_forward_long_call(cuda):
    from eavsr_amd import framestore as FS
    net, hot = _net(cuda), _net(cuda, "hot")
    with torch.no_grad():
        u8 = _clip_u8(1, 3, 64, 112, 31).to(cuda)
        for model in (net, hot):
            model.cache_census.clear()
        want = net.forward_tiled(u8, 64, overlap=16, cache_dtype="fp16")
        assert torch.equal(net.forward_tiled(u8, 64, overlap=16, cache_dtype="fp16", cache_check="bf16"), want)      # nothing overflowed
        assert [(e["fallback"], e["size"], e["frames"]) for e in net.cache_census] == [(False, (64, 64), 3)] * 2      # two tiles
        # the hot network: both tiles fall back, and the blend is the bf16 run's
        assert torch.equal(hot.forward_tiled(u8, 64, overlap=16, cache_dtype="fp16", cache_check="bf16"),
                           hot.forward_tiled(u8, 64, overlap=16, cache_dtype="bf16"))
        assert [(e["fallback"], e["used"]) for e in hot.cache_census] == [(True, "bf16")] * 2
        with pytest.raises(FS.CacheRangeError):
            hot.forward_tiled(u8, 64, overlap=16, cache_dtype="fp16", cache_check="raise")
        assert len(hot.cache_census) == 3      # the first tile was refused; the second never ran
        x = _clip_u8(1, 5, 64, 64, 41).to(cuda)
        net.cache_census.clear()
        want = net.forward_cached(x, "fp16", ensemble=2)
        assert torch.equal(net.forward_cached(x, "fp16", ensemble=2, cache_check="report"), want)
        assert len(net.cache_census) == 2 and all(e["used"] == "fp16" and e["keys"]["forward_2"]["elements"] == 5 * 64 * 64 * 64
                                                  for e in net.cache_census)
        assert net.cache_census[0]["keys"] != net.cache_census[1]["keys"]      # the network is not equivariant: the modes differ
        hot.cache_census.clear()
        assert torch.equal(hot.forward_cached(x, "fp16", ensemble=2, cache_check="bf16"), hot.forward_cached(x, "bf16", ensemble=2))
        assert [e["fallback"] for e in hot.cache_census] == [True, True]
        for model in (net, hot):
            model.cache_census.clear()


def _wrapper(**extra):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    model = EAVSRPModel(Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0], **extra))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    return model


def test_super_resolve_and_evaluate_with_the_option(cuda, monkeypatch):
    from eavsr_amd import framestore as FS, harness
    for var in ("EAVSR_CACHE_DTYPE", "EAVSR_CACHE_CHECK", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_ENSEMBLE", "EAVSR_MAX_FRAMES",
                "EAVSR_FRAME_CHUNK", "EAVSR_CPU_CACHE"):
        monkeypatch.delenv(var, raising=False)
    net, hot = _net(cuda), _net(cuda, "hot")
    u8 = _clip_u8(1, 5, 64, 64, 41)
    hr = torch.zeros(5, 3, 256, 256, dtype=torch.uint8)
    plain = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=2, cache_dtype="fp16")
    assert "cache_census" not in plain and "cache_range" not in plain
    net.cache_census.append("stale")
    res = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=2, cache_dtype="fp16", cache_check="report")
    assert res["frame_psnr"] == plain["frame_psnr"] and res["cache_census"] is net.cache_census and len(res["cache_census"]) == 1
    keys = res["cache_census"][0]["keys"]
    assert res["cache_range"] == {"windows": 1, "fallbacks": 0, "max_abs": max(r["max_abs"] for r in keys.values()), "nonfinite": 0,
                                  "overflow": 0, "flushed": sum(r["flushed"] for r in keys.values()),
                                  "subnormal": sum(r["subnormal"] for r in keys.values())}
    assert 0 < res["cache_range"]["max_abs"] < 65504
    # two windows of frames on the hot network, the environment setting the check: both fall back, the frames are the bf16 cache's
    monkeypatch.setenv("EAVSR_CACHE_CHECK", "bf16")
    want = harness.super_resolve(hot, u8[0], hr=hr, max_frames=3, overlap=1, cache_dtype="bf16", cache_check="report")
    res = harness.super_resolve(hot, u8[0], hr=hr, max_frames=3, overlap=1, cache_dtype="fp16")
    assert len(res["segments"]) == 2 and res["frame_psnr"] == want["frame_psnr"]
    assert res["cache_range"]["windows"] == 2 and res["cache_range"]["fallbacks"] == 2 and res["cache_range"]["overflow"] >= 2 * 3 * 64 * 64
    assert res["cache_range"]["max_abs"] > 65520 and want["cache_range"]["fallbacks"] == 0 and want["cache_range"]["overflow"] == 0
    monkeypatch.delenv("EAVSR_CACHE_CHECK")
    with pytest.raises(FS.CacheRangeError):
        harness.super_resolve(hot, u8[0], frame_chunk=2, cache_dtype="fp16", cache_check="raise")
    # evaluate: the wrapper hands its option to the long path
    lr = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
    hr5 = torch.zeros(1, 5, 3, 256, 256)
    wrapper = _wrapper(cache_dtype="fp16", cache_check="bf16", frame_chunk=2)
    assert wrapper.cache_check == "bf16" and wrapper.netEAVSRP.cache_census == []
    harness.evaluate(wrapper, [{"lr_seq": lr, "hr_seq": hr5, "fname": ["000_%05d.png" % i for i in range(5)]}], per_frame=True)
    assert torch.equal(wrapper.data_sr_seq, _shared(cuda, "x4", "fp16"))
    assert [(e["asked"], e["used"], e["fallback"]) for e in wrapper.netEAVSRP.cache_census] == [("fp16", "fp16", False)]
    for model in (net, hot):
        model.cache_census.clear()


def test_refusals_come_before_any_launch(ops, cuda, monkeypatch):
    from eavsr_amd import harness
    for var in ("EAVSR_CACHE_DTYPE", "EAVSR_CACHE_CHECK"):
        monkeypatch.delenv(var, raising=False)
    net = _net(cuda)
    x = _clip_u8(1, 2, 96, 112, 31).to(cuda)
    with torch.no_grad():
        refused = [lambda: net.forward_long(x, cache_dtype="fp16", cache_check="warn"), lambda: net.forward_long(x, cache_check="report"),
                   lambda: net.forward_long(x, cache_dtype="bf16", cache_check="bf16"),
                   lambda: net.forward_tiled(x, 64, cache_dtype="fp16", cache_check=True), lambda: net.forward_tiled(x, 64, cache_check="raise"),
                   lambda: net.forward_segments_padded(x, [(0, 2, 0, 2)], None, cache_dtype=torch.bfloat16, cache_check="bf16"),
                   lambda: net.forward_cached(x, None, cache_check="report"), lambda: net.forward_cached(x, "fp16", ensemble=2, cache_check="fp16"),
                   lambda: harness.super_resolve(net, x[0], cache_check="bf16"),
                   lambda: harness.super_resolve(net, x[0], cache_dtype="fp16", cache_check="Raise")]
        for i, fn in enumerate(refused):
            out, launched = _launches(ops, fn)
            assert isinstance(out, ValueError) and launched == {}, (i, out, launched)
    assert net.cache_census == []
