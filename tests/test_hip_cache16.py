"""The 16-bit feature cache of the long-clip path on the GPU (`pytest -m gpu`): `ops.pack16` / `ops.unpack16` against the
CPU's `torch.Tensor.to` bit for bit, the two 16-bit stores against `x.to(dtype).float()`, `EAVSRP.forward_long(cache_dtype=...)` against
the same call on a reference store that rounds with torch, bit for bit, and the paths built on it against their hand-assembled
statements.  All weights are synthetic."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_on_the_device():
    """the networks and outputs this module caches are dropped when it ends, and the allocator's blocks with them"""
    yield
    _NETS.clear()
    _OUT.clear()
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


def _pack(ops, x, dt):
    out = torch.empty(x.shape, dtype=dt, device=x.device)
    ops.pack16([x], [out], dt)
    return out


def _unpack(ops, x):
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ops.unpack16([x], [out])
    return out


def _same_but_nan(got, want):
    """equal bits wherever `want` is not a NaN; a NaN wherever it is"""
    nan = torch.isnan(want.float())
    view = _bits16 if want.dtype != torch.float32 else _bits32
    return bool(torch.equal(view(got)[~nan], view(want)[~nan]) and torch.isnan(got.float().cpu()[nan]).all())


# ------------------------------------------------------------------------------------------------------------- the kernels: values
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_all_65536_patterns_widen_exactly_and_round_back_to_themselves(ops, cuda, name):
    dt = DTYPES[name]
    every = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dt)
    wide = _unpack(ops, every.to(cuda))
    assert wide.dtype == torch.float32 and _same_but_nan(wide.cpu(), every.to(torch.float32))
    back = _pack(ops, wide, dt)
    assert _same_but_nan(back.cpu(), every)
    assert int(torch.isnan(every.float()).sum()) == (2046 if name == "fp16" else 254)


def _f32(*values):
    return torch.tensor(values, dtype=torch.float64).to(torch.float32)


def _from_bits(*bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


SPECIAL = {
    # the last finite value, the largest value that still rounds to it, the tie that goes to inf, and past it; the smallest
    # subnormal, half of it (a tie: to even, 0), the next float above that (rounds up); ties on both sides of even at 11 bits
    "fp16": torch.cat([_f32(65504.0, 65519.996, 65520.0, 65536.0, 2.0 ** -24, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
                            2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 6.0e-8, 1.0e-8),
                       _from_bits(0x33000001, 0x32FFFFFF, 0x3F801000, 0x3F801001, 0x3F800FFF, 0x3F803000, 0x3F803001, 0x3F802FFF)]),
    # ties at 1 + 2^-8 (to even: down) and 1 + 3 2^-8 (to even: up), one ulp of fp32 to either side of each; the carry into inf
    "bf16": torch.cat([_f32(1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0e-40, 3.0e38),
                       _from_bits(0x3F808000, 0x3F808001, 0x3F807FFF, 0x3F818000, 0x3F818001, 0x3F817FFF, 0x7F7F8000, 0x7F7F7FFF,
                                  0x00008000, 0x00008001, 0x00018000)]),
}
COMMON = torch.cat([_f32(0.0, -0.0, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38, 1.0, -1.0),
                    _from_bits(0x7FC01234, 0xFFC00001, 0x7F800001, 0x00000001, 0x80000001, 0x007FFFFF)])


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_rounding_is_the_cpu_conversion_bit_for_bit(ops, cuda, name):
    dt = DTYPES[name]
    g = torch.Generator().manual_seed(16)
    anything = torch.randint(-2 ** 31, 2 ** 31, (1 << 18,), dtype=torch.int64, generator=g).to(torch.int32).view(torch.float32)
    near = torch.randn(1 << 16, generator=g) * 4.0
    x = torch.cat([SPECIAL[name], -SPECIAL[name], COMMON, anything, near, near * 3.0e4, near * 1.0e-6])
    want = x.to(dt)      # the CPU's conversion
    got = _pack(ops, x.to(cuda), dt)
    assert _same_but_nan(got.cpu(), want)
    k = len(SPECIAL[name])
    assert torch.equal(_bits16(got[:2 * k + 4]), _bits16(want[:2 * k + 4])), name      # the hand-built cases and +-0, +-inf, one by one
    if name == "fp16":
        assert got[:4].float().cpu().tolist() == [65504.0, 65504.0, float("inf"), float("inf")]
        assert got[4:8].float().cpu().tolist() == [2.0 ** -24, 0.0, 1.0, 1.0 + 2.0 ** -9] and float(got[12].float()) == 2.0 ** -24
    else:
        assert got[:2].float().cpu().tolist() == [1.0, 1.0 + 2.0 ** -6]
        assert float(got[4 + 6].float()) == float("inf") and float(got[4 + 7].float()) == 3.3895313892515355e38
    assert torch.isnan(got[2 * k + 4].float()) and torch.signbit(got[2 * k + 1].float()) and not torch.signbit(got[2 * k].float())
    again = _pack(ops, x.to(cuda), dt)
    assert torch.equal(_bits16(again), _bits16(got))      # two calls agree bit for bit


# ------------------------------------------------------------------------------------------------------------- the kernels: shapes
LENGTHS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4099]


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_every_length_at_every_misalignment_of_either_side(ops, cuda, name):
    """sources and destinations sliced 0 .. 7 elements off a 16-byte boundary, independently: 64 pairs per length, sixteen segments per
    launch; the elements on either side of every destination keep their bits"""
    dt = DTYPES[name]
    g = torch.Generator().manual_seed(1)
    M = ops.CACHE16_MAX_SEGMENTS
    for n in LENGTHS:
        x = torch.randn(n, generator=g) * 100.0
        want16, x_dev = x.to(dt), x.to(cuda)
        want32 = want16.to(torch.float32)
        pairs = [(a, b) for a in range(8) for b in range(8)]
        for at in range(0, 64, M):
            part = pairs[at:at + M]
            src32 = [torch.zeros(n + 16, device=cuda) for _ in part]
            dst16 = [torch.full((n + 16,), 7.0, dtype=dt, device=cuda) for _ in part]
            dst32 = [torch.full((n + 16,), 7.0, device=cuda) for _ in part]
            assert all(t.data_ptr() % 16 == 0 for t in src32 + dst16 + dst32)
            for (a, b), s in zip(part, src32):
                s[a:a + n] = x_dev
            _, launched = _launches(ops, lambda: ops.pack16([s[a:a + n] for (a, b), s in zip(part, src32)],
                                                            [d[b:b + n] for (a, b), d in zip(part, dst16)], name))
            assert launched == {"pack16": 1}
            # ... and back: the 16-bit side at offset b, the fp32 side at offset a
            _, launched = _launches(ops, lambda: ops.unpack16([d[b:b + n] for (a, b), d in zip(part, dst16)],
                                                              [d[a:a + n] for (a, b), d in zip(part, dst32)]))
            assert launched == {"unpack16": 1}
            for (a, b), d16, d32 in zip(part, dst16, dst32):
                assert torch.equal(_bits16(d16[b:b + n]), _bits16(want16)), (name, n, a, b)
                assert torch.equal(_bits32(d32[a:a + n]), _bits32(want32)), (name, n, a, b)
                assert bool((d16[:b] == 7).all() and (d16[b + n:] == 7).all() and (d32[:a] == 7).all() and (d32[a + n:] == 7).all()), (name, n, a, b)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_lists_of_unequal_segments_with_an_empty_one_among_them(ops, cuda, name):
    dt = DTYPES[name]
    M = ops.CACHE16_MAX_SEGMENTS
    g = torch.Generator().manual_seed(2)
    for nseg, launches in ((1, 1), (2, 1), (M, 1), (M + 1, 2)):
        lengths = [(0 if i == 1 else 1 + 37 * i + (3000 if i % 5 == 0 else 0)) for i in range(nseg)]
        if nseg == 1:
            lengths = [2500]      # more than two passes of 1024 items would need 16 K elements: three passes of a 2500-element tail mix
        xs = [torch.randn(n, generator=g) for n in lengths]
        srcs = [x.to(cuda) for x in xs]
        dsts = [torch.empty(n, dtype=dt, device=cuda) for n in lengths]
        _, launched = _launches(ops, lambda: ops.pack16(srcs, dsts, dt))
        assert launched == {"pack16": launches}, (nseg, launched)
        back = [torch.empty(n, device=cuda) for n in lengths]
        _, launched = _launches(ops, lambda: ops.unpack16(dsts, back))
        assert launched == {"unpack16": launches}
        for x, d, b in zip(xs, dsts, back):
            assert torch.equal(_bits16(d), _bits16(x.to(dt))) and torch.equal(_bits32(b), _bits32(x.to(dt).float()))
    # nothing but empty segments, and no segments: nothing is launched
    e32, e16 = torch.empty(0, device=cuda), torch.empty(0, dtype=dt, device=cuda)
    assert _launches(ops, lambda: ops.pack16([e32, e32], [e16, e16], dt))[1] == {}
    assert _launches(ops, lambda: ops.unpack16([], []))[1] == {}
    # a segment of several workgroup passes with a grid-stride (more passes than the grid's cap is a matter of the extent tests)
    big = torch.randn(3 * 1024 * 8 + 5, generator=g)
    assert torch.equal(_bits16(_pack(ops, big.to(cuda), dt)), _bits16(big.to(dt)))
    # refusals launch nothing
    x = torch.zeros(64, device=cuda)
    for fn in (lambda: ops.pack16([x], [torch.zeros(64, dtype=torch.float16, device=cuda)], "bf16"),
               lambda: ops.pack16([x[::2]], [torch.zeros(32, dtype=dt, device=cuda)], dt),
               lambda: ops.pack16([x], [torch.zeros(63, dtype=dt, device=cuda)], dt),
               lambda: ops.unpack16([torch.zeros(64, dtype=dt, device=cuda)], [torch.zeros(64, dtype=torch.float64, device=cuda)]),
               lambda: ops.pack16([x], [torch.zeros(64, dtype=dt)], dt)):
        out, launched = _launches(ops, fn)
        assert isinstance(out, (ValueError, RuntimeError)) and launched == {}, out


# ------------------------------------------------------------------------------------------------------------- the stores
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
@pytest.mark.parametrize("cache", ["device", "host"])
def test_a_tensor_that_went_through_a_store_is_x_to_dtype_float(ops, cuda, cache, name, n):
    from eavsr_amd import framestore as FS
    dt = DTYPES[name]
    t, c, h, w = 4, 5, 12, 20
    g = torch.Generator().manual_seed(n)
    store, plain = FS.make_store(cache, n, t, cuda, dtype=name), FS.make_store(cache, n, t, cuda)
    assert type(plain) in (FS.DeviceStore, FS.HostStore) and store.cache == cache and store.cache_dtype == name
    held = {}
    for key, d in zip(FS.PYR, (1, 2, 4)):
        held[key] = torch.randn(t * n, c, h // d, w // d, generator=g) * 50.0
        for a, b in ((0, 3), (3, t)):      # two chunks
            for s in (store, plain):
                s.put_range(key, a, held[key][a * n:b * n].to(cuda))
    held["flow_backward"] = torch.randn((t - 1) * n, 2, h, w, generator=g)
    held["lr"] = torch.rand(t * n, 3, h, w, generator=g)
    for s in (store, plain):
        s.put_range("flow_backward", 0, held["flow_backward"].to(cuda))
        s.put_range("lr", 0, held["lr"].to(cuda))
    reads = FS.propagate_reads(t, True, ())
    schedule = FS.prefetch_schedule(reads)
    _, launched = _launches(ops, lambda: store.begin(schedule))
    assert launched == {"unpack16": 1}      # the three levels of the prologue: one launch
    held["backward_1"] = torch.randn(t * n, c, h, w, generator=g)
    for s in (store, plain):
        s.new_branch("backward_1", torch.zeros(n, c, h, w, device=cuda))
    assert store.out_slot("backward_1", 0) is None
    for i, items in enumerate(reads):
        _, launched = _launches(ops, lambda: store.step(i))
        assert launched == ({"unpack16": 1} if any(FS.is_feature_key(k) for k, _ in schedule.fetch[i]) else {})
        for key, idx in items:
            got = store.get(key, idx)
            x = held[key][idx * n:(idx + 1) * n]
            want = x if key == "flow_backward" else x.to(dt).float()
            assert got.dtype == torch.float32 and torch.equal(_bits32(got), _bits32(want)), (i, key, idx)
        idx = t - 1 - i
        store.put("backward_1", idx, held["backward_1"][idx * n:(idx + 1) * n].to(cuda))
        store.done(i)
    for key in ("spatial", "backward_1"):
        for a, b in ((0, t), (1, 3), (2, 4)):
            got, launched = _launches(ops, lambda: store.get_range(key, a, b))
            assert launched == {"unpack16": 1}
            assert torch.equal(_bits32(got), _bits32(held[key][a * n:b * n].to(dt).float())), (key, a, b)
    assert torch.equal(store.get_range("lr", 1, 3).cpu(), held["lr"][n:3 * n])
    assert torch.equal(store.get_range("flow_backward", 0, t - 1).cpu(), held["flow_backward"])
    store.finish()
    torch.cuda.synchronize()
    nb, nb32 = store.nbytes(), plain.nbytes()
    for key in nb32:
        if key != "total":
            assert nb[key] * (2 if FS.is_feature_key(key) else 1) == nb32[key], key
    assert nb["total"] == sum(v for k, v in nb.items() if k != "total") < nb32["total"]
    plain.finish()


# ------------------------------------------------------------------------------------------------------------- the model
_NETS = {}
_OUT = {}


def _net(cuda, tag="x4"):
    if tag not in _NETS:
        from eavsr_amd.eavsrp_model import EAVSRP, EAVSRPx2
        opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4 if tag == "x4" else 2)
        net = EAVSRP(opt, None) if tag == "x4" else EAVSRPx2(opt, None)
        net.load_state_dict(H.filled(H.model_shapes(tag), "trained_like"), strict=True)
        _NETS[tag] = net.to(cuda).eval()
    return _NETS[tag]


def _clip_u8(n, t, h, w, seed):
    from eavsr_amd.utils.synthetic import synthetic_clip
    big = synthetic_clip(n, t, h + (-h) % 4 + 4, w + (-w) % 4 + 4, seed=seed)
    return (big[..., :h, :w] * 255).round().to(torch.uint8).contiguous()


def _reference_store(dtype):
    """a `DeviceStore` that returns x.to(dtype).float() for the feature keys, rounded by torch when a tensor is put; no slot to write
    into, so a step keeps its own unrounded output as the 16-bit stores' steps do"""
    from eavsr_amd import framestore as FS

    class Rounding(FS.DeviceStore):
        def _round(self, key, x):
            return x.to(dtype).to(torch.float32) if FS.is_feature_key(key) else x

        def put_range(self, key, first, frames):
            super().put_range(key, first, self._round(key, frames))

        def out_slot(self, key, idx):
            return None

        def put(self, key, idx, frame):
            FS.DeviceStore.get(self, key, idx).copy_(self._round(key, frame))
    return lambda cache, n, t, device, dtype=None: Rounding(n, t, device)


def _reference(monkeypatch, net, x, name, **kw):
    from eavsr_amd import framestore as FS
    with monkeypatch.context() as m:
        m.setattr(FS, "make_store", _reference_store(DTYPES[name]))
        return net.forward_long(x, **kw)


def _long(cuda, tag, n, t, h, w, seed, name, cache="device", **kw):
    """`forward_long(cache_dtype=name)` of the synthetic clip, computed once per setting and never written to"""
    key = (tag, n, t, h, w, seed, name, cache, tuple(sorted(kw.items())))
    if key not in _OUT:
        with torch.no_grad():
            _OUT[key] = _net(cuda, tag).forward_long(_clip_u8(n, t, h, w, seed).to(cuda), cache=cache, cache_dtype=name, **kw)
    return _OUT[key]


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_forward_long_is_forward_long_on_a_store_that_rounds_with_torch(cuda, monkeypatch, name):
    """1 x 5 x 64 x 64, frame_chunk=2: both caches, bit for bit; n = 2; and the launches of a call without `cache_dtype` are unchanged"""
    from eavsr_amd import ops
    net = _net(cuda)
    x = _clip_u8(1, 5, 64, 64, 41).to(cuda)
    with torch.no_grad():
        want = _reference(monkeypatch, net, x, name, frame_chunk=2)
        dev, host = _long(cuda, "x4", 1, 5, 64, 64, 41, name, frame_chunk=2), _long(cuda, "x4", 1, 5, 64, 64, 41, name, "host", frame_chunk=2)
        assert tuple(dev.shape) == (1, 5, 3, 256, 256) and torch.isfinite(dev).all()
        assert torch.equal(_bits32(dev), _bits32(want)) and torch.equal(_bits32(host), _bits32(dev))
        assert torch.equal(net.forward_long(x, frame_chunk=2, cache_dtype=DTYPES[name]), dev)      # the torch dtype is the same setting
        plain, launches = _launches(ops, lambda: net.forward_long(x, frame_chunk=2))
        assert not torch.equal(plain, dev) and "pack16" not in launches and "unpack16" not in launches
        _, with16 = _launches(ops, lambda: net.forward_long(x, frame_chunk=2, cache_dtype=name))
        extra = {k: v for k, v in with16.items() if launches.get(k) != v}
        assert set(extra) == {"pack16", "unpack16"}, extra      # no compute kernel more or less
        x2 = _clip_u8(2, 5, 64, 64, 42).to(cuda)
        want2 = _reference(monkeypatch, net, x2, name, frame_chunk=2)
        assert torch.equal(net.forward_long(x2, frame_chunk=2, cache_dtype=name), want2)
        assert torch.equal(net.forward_long(x2, frame_chunk=2, cache="host", cache_dtype=name), want2)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_with_emit_pad_window_transform_and_the_x2_network(cuda, monkeypatch, name):
    net = _net(cuda)
    x = _clip_u8(1, 5, 64, 64, 41).to(cuda)
    odd = _clip_u8(1, 5, 66, 70, 43).to(cuda)
    wide = _clip_u8(1, 5, 72, 96, 44).to(cuda)
    cases = [(net, x, dict(emit=(1, 4))), (net, odd, dict(pad="reflect")), (net, wide, dict(window=(4, 68, 17, 81))),
             (net, x, dict(transform=5)), (_net(cuda, "x2"), x, dict())]
    with torch.no_grad():
        for model, clip, kw in cases:
            want = _reference(monkeypatch, model, clip, name, frame_chunk=2, **kw)
            for cache in ("device", "host"):
                got = model.forward_long(clip, frame_chunk=2, cache=cache, cache_dtype=name, **kw)
                assert torch.equal(_bits32(got), _bits32(want)), (name, cache, kw)


def test_tiles_ensemble_and_segments_are_their_blends_of_forward_long_with_the_cache(cuda):
    from eavsr_amd.segments import plan_segments
    from tests import ensemble_ref as E
    from tests import tile_ref as R
    net = _net(cuda)
    name = "fp16"
    u8 = _clip_u8(1, 3, 96, 112, 31)
    with torch.no_grad():
        tiles = R.plan_tiles(96, 112, 64, 16)
        per_tile = [net.forward_long(u8[..., y0:y1, x0:x1].contiguous().to(cuda), cache_dtype=name).cpu().numpy() for y0, y1, x0, x1 in tiles]
        want = torch.from_numpy(R.blend_tiles(per_tile, tiles, 96, 112, 4, 64, 16))
        got = net.forward_tiled(u8.to(cuda), 64, overlap=16, cache_dtype=name)
        assert torch.equal(_bits32(got), _bits32(want))
        assert not torch.equal(got, net.forward_tiled(u8.to(cuda), 64, overlap=16))
        assert torch.equal(net.forward_cached(u8.to(cuda), name, tile=64, overlap=16), got)

        x = _clip_u8(1, 4, 64, 64, 45).to(cuda)
        plan = plan_segments(4, [], 3, 2)
        assert len(plan) == 2
        parts = [net.forward_long(x[:, a:b], emit=(ea - a, eb - a), cache_dtype=name, cache="host") for a, b, ea, eb in plan]
        seg = net.forward_segments_padded(x, plan, None, cache="host", cache_dtype=name)
        assert torch.equal(seg, torch.cat(parts, 1)) and torch.equal(net.forward_cached(x, name, segments=plan), seg)
        assert torch.equal(net.forward_cached(x, None, segments=plan), net.forward_segments(x, plan))      # None: today's call

        modes = (0, 1)
        per_mode = [[net.forward_long(x, transform=k, cache_dtype=name).cpu().numpy() for k in modes]]
        ones = lambda m: np.ones((1, m), np.float32)
        want = torch.from_numpy(E.ensemble_blend(per_mode, [(0, 64, 0, 64)], modes, 64, 64, 4, ones(256), ones(256), 1))
        ens = net.forward_cached(x, name, ensemble=2)
        assert torch.equal(_bits32(ens), _bits32(want))
        assert not torch.equal(ens, net.forward_ensemble(x, ensemble=2))


def _wrapper(**extra):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    model = EAVSRPModel(Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0], **extra))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    return model


def _hr_for(u8):
    t = u8.shape[0]
    hr = torch.nn.functional.interpolate(u8.float(), scale_factor=4, mode="bicubic", align_corners=False)
    hr = hr + 4.0 * torch.randn(hr.shape, generator=torch.Generator().manual_seed(3))
    return hr.clamp(0, 255).round().to(torch.uint8).view(t, 3, 4 * u8.shape[2], 4 * u8.shape[3])


def test_super_resolve_of_66x70_png_files_and_evaluate_with_the_option(cuda, tmp_path, monkeypatch):
    from eavsr_amd import harness, ops
    for var in ("EAVSR_CACHE_DTYPE", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_ENSEMBLE", "EAVSR_MAX_FRAMES", "EAVSR_FRAME_CHUNK", "EAVSR_CPU_CACHE"):
        monkeypatch.delenv(var, raising=False)
    model = _wrapper()
    u8 = _clip_u8(1, 3, 66, 70, 46)
    hr = _hr_for(u8[0])
    names = ["000_%05d.png" % i for i in range(3)]
    paths = [harness.write_png(u8[0, i], str(tmp_path / "lr" / names[i])) for i in range(3)]
    hr_paths = [harness.write_png(hr[i], str(tmp_path / "hr" / names[i])) for i in range(3)]
    with torch.no_grad():
        want = model.netEAVSRP.forward_long(u8.to(cuda), pad="reflect", frame_chunk=2, cache_dtype="fp16")
    assert tuple(want.shape) == (1, 3, 3, 264, 280)
    want_metrics = harness.frame_metrics(want, ops.u8_to_f32(hr.to(cuda)).unsqueeze(0), 255.0)
    want_rgb8 = ops.rgb8(want[0], 255.0)
    for encoder in ("host", "device"):
        res = harness.super_resolve(model, paths, out_dir=str(tmp_path / encoder), hr=hr_paths, pad="reflect", frame_chunk=2,
                                    cache_dtype="fp16", png_encoder=encoder)
        assert res["cache_dtype"] == "fp16" and res["frames"] == 3 and res["frame_names"] == names
        assert res["frame_psnr"] == want_metrics["psnr"] and res["frame_ssim"] == want_metrics["ssim"]
        decoded = harness.decode_png_frames(res["written"], cuda, channels=3)
        assert torch.equal(decoded.permute(0, 2, 3, 1), want_rgb8)
    plain = harness.super_resolve(model, paths, hr=hr_paths, pad="reflect", frame_chunk=2)
    assert plain["cache_dtype"] is None and plain["frame_psnr"] != res["frame_psnr"]
    # the environment alone, then the options over the environment; the host cache gives the same frames
    monkeypatch.setenv("EAVSR_CACHE_DTYPE", "fp16")
    res = harness.super_resolve(model.netEAVSRP, u8[0], hr=hr, names=names, pad="reflect", frame_chunk=2, cache="host")
    assert res["cache_dtype"] == "fp16" and res["frame_psnr"] == want_metrics["psnr"]
    monkeypatch.setenv("EAVSR_CACHE_DTYPE", "bf16")
    model.opt.cache_dtype = torch.float16
    res = harness.super_resolve(model, paths, hr=hr_paths, pad="reflect", frame_chunk=2)
    assert res["cache_dtype"] == "fp16" and res["frame_psnr"] == want_metrics["psnr"]
    monkeypatch.delenv("EAVSR_CACHE_DTYPE")

    # evaluate: the wrapper takes the long path where the option is set
    x = _clip_u8(1, 5, 64, 64, 41)
    lr = torch.from_numpy(np.float32(x.numpy()) / np.float32(255))
    hr5 = (_hr_for(x[0]).float() / 255).unsqueeze(0)
    names5 = ["000_%05d.png" % i for i in range(5)]
    wrapper = _wrapper(cache_dtype="bf16", frame_chunk=2)
    rep = harness.evaluate(wrapper, [{"lr_seq": lr, "hr_seq": hr5, "fname": names5}], per_frame=True, calc_ssim_flag=True)
    with torch.no_grad():
        want5 = wrapper.netEAVSRP.forward_long(lr.to(cuda), frame_chunk=2, cache_dtype="bf16")
    assert torch.equal(wrapper.data_sr_seq, want5)
    fm = harness.frame_metrics(want5, hr5.to(cuda), 255.0)
    assert rep["frame_psnr"] == fm["psnr"] and rep["frame_ssim"] == fm["ssim"] and rep["frame_names"] == names5


def test_refusals_come_before_any_launch(cuda, monkeypatch):
    from eavsr_amd import harness, ops
    monkeypatch.delenv("EAVSR_CACHE_DTYPE", raising=False)
    net = _net(cuda)
    x = _clip_u8(1, 2, 96, 112, 31).to(cuda)
    with torch.no_grad():
        refused = [lambda: net.forward_long(x, cache_dtype="fp32"), lambda: net.forward_long(x, cache_dtype=torch.float32),
                   lambda: net.forward_long(x, cache_dtype=16), lambda: net.forward_tiled(x, 64, cache_dtype="half"),
                   lambda: net.forward_segments_padded(x, [(0, 2, 0, 2)], None, cache_dtype="fp8"),
                   lambda: net.forward_cached(x, "float16"), lambda: net.forward_cached(x, "f16", ensemble=2),
                   lambda: harness.super_resolve(net, x[0], cache_dtype="fp32")]
        for i, fn in enumerate(refused):
            out, launched = _launches(ops, fn)
            assert isinstance(out, ValueError) and launched == {}, (i, out, launched)


# ------------------------------------------------------------------------------------------------------------- closeness
def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * np.log10(1.0 / mse) if mse > 0 else float("inf")


def test_the_16_bit_cache_stays_close_to_the_fp32_cache(cuda):
    """1 x 5 x 64 x 64, synthetic weights, seed 41, frame_chunk=2: PSNR (peak 1) of each 16-bit run against the cache_dtype=None output
    of the same call.  The bound is the figure measured once on the MI355X (profiles/r24_cache16_parity.json) minus 6 dB -- one bit
    of headroom for another kernel route on another build.  And bf16 (8 significant bits) must not beat fp16 (11) by more than 1 dB:
    if it does, the two dtypes are wired the wrong way round.  Says nothing about a trained model."""
    with open(os.path.join(ROOT, "profiles", "r24_cache16_parity.json")) as f:
        measured = json.load(f)["psnr_db_vs_fp32_cache"]
    with torch.no_grad():
        plain = _net(cuda).forward_long(_clip_u8(1, 5, 64, 64, 41).to(cuda), frame_chunk=2)
    got = {name: _psnr(_long(cuda, "x4", 1, 5, 64, 64, 41, name, frame_chunk=2), plain) for name in ("fp16", "bf16")}
    print("PSNR against the fp32 cache (dB):", got, "measured:", measured)
    for name in ("fp16", "bf16"):
        assert got[name] >= measured[name] - 6.0, (name, got[name], measured[name])
    assert got["bf16"] <= got["fp16"] + 1.0, got
