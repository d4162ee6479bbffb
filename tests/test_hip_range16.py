"""The range census of the 16-bit backbone on the GPU (`pytest -m gpu`, DESIGN 3.6 addendum): `ops.range16_words` /
`ops.range16_as_rounded` against the numpy reference (tests/range16_ref.py) and against `ops.pack16_census`, and
`networks.backbone_check` through `EAVSRP.forward`, `forward_long` and the paths built on it -- on the synthetic weights and on two
copies of them that leave fp16's range at one known place (tests/range16_cases.py)."""
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import range16_cases as K
from tests import range16_ref as R

pytestmark = pytest.mark.gpu

DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    from eavsr_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def N():
    from eavsr_amd import networks
    return networks


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    from eavsr_amd import networks
    yield
    networks.set_backbone_check(None)
    networks.set_backbone_dtype(None)
    _NETS.clear()
    _SHARED.clear()
    torch.cuda.empty_cache()


def _bits32(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _words_t(o16: np.ndarray, name, cuda):
    return torch.from_numpy(np.ascontiguousarray(o16).view(np.int16)).to(cuda).view(DTYPES[name])


def _record(ops, census, elements, name):
    return ops.census_record(census.cpu(), elements, name)


def _spread(count, seed, lo=-150, hi=120):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(count) * np.exp2(rng.integers(lo, hi, count))).astype(np.float32)


def _zeros5(cuda):
    return torch.zeros(5, dtype=torch.int64, device=cuda)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_all_65536_words_and_the_widened_table(ops, cuda, name):
    """every 16-bit pattern, twice over in a random order so that the edges lie scattered among the others: the five integers of
    `range16_words` equal the reference's; the same values widened, with the hand-built fp32 edges of both formats among them,
    through `range16_as_rounded` equal the reference AND `pack16_census`'s record"""
    from tests import census_ref as C
    rng = np.random.default_rng(3)
    o = rng.permutation(np.tile(np.arange(65536, dtype=np.uint16), 2))
    want = R.words(o, name)
    assert want["nonfinite"] > 200 and want["subnormal"] > 200 and want["overflow"] == 0 and want["flushed"] == 0
    assert want["max_abs"] == R.FORMAT_MAX[name]
    census = _zeros5(cuda)
    assert ops.range16_words([_words_t(o, name, cuda)], census) == o.size
    assert _record(ops, census, o.size, name) == dict(want, dtype=name)
    x = R.widen(o, name).copy()
    edges = C.BOUNDARY_BITS + C.BF16_TINY_BITS
    x.view(np.uint32)[rng.choice(x.size, len(edges), replace=False)] = np.array(edges, np.uint32)
    want = R.as_rounded(x, name)
    assert want["overflow"] > 0 and want["flushed"] > 0
    src = torch.from_numpy(x).to(cuda)
    census, packed = _zeros5(cuda), _zeros5(cuda)
    assert ops.range16_as_rounded([src], name, census) == x.size
    ops.pack16_census([src], [torch.empty(x.size, dtype=DTYPES[name], device=cuda)], name, packed)
    assert census.tolist() == packed.tolist() == R.row(want)
    # the edges alone, one element per launch
    for bits in edges:
        one = np.array([bits], np.uint32).view(np.float32)
        c = _zeros5(cuda)
        ops.range16_as_rounded([torch.from_numpy(one).to(cuda)], name, c)
        assert c.tolist() == R.row(R.as_rounded(one, name)), hex(bits)


@pytest.mark.parametrize("flavour", ["words", "as_rounded"])
@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_lengths_1_to_1100_at_every_misalignment(ops, cuda, name, flavour):
    """head, vectors, tail and the end of a workgroup pass at 1024 items, one record per length"""
    per_vec = 8 if flavour == "words" else 4
    slot, lengths = 1120, list(range(1, 1101))
    x = _spread(len(lengths) * slot + 8, 11)
    if flavour == "words":
        o = np.random.default_rng(12).integers(0, 65536, x.size).astype(np.uint16)
        dev = _words_t(o, name, cuda)
    else:
        dev = torch.from_numpy(x).to(cuda)
    assert dev.data_ptr() % 16 == 0
    for mis in range(per_vec):
        census = torch.zeros((len(lengths), 5), dtype=torch.int64, device=cuda)
        for i, n in enumerate(lengths):
            seg = dev[i * slot + mis:i * slot + mis + n]
            if flavour == "words":
                ops.range16_words([seg], census[i])
            else:
                ops.range16_as_rounded([seg], name, census[i])
        got = census.cpu().tolist()
        for i, n in enumerate(lengths):
            a = i * slot + mis
            want = R.words(o[a:a + n], name) if flavour == "words" else R.as_rounded(x[a:a + n], name)
            assert got[i] == R.row(want), (mis, n)


@pytest.mark.parametrize("name", ["fp16", "bf16"])
def test_lists_slices_accumulation_and_repeatability(ops, cuda, name):
    rng = np.random.default_rng(21)
    # 19 segments (two launches), one of them empty, at mixed alignments
    parts = [rng.integers(0, 65536, n).astype(np.uint16) for n in [5, 0, 17, 1, 2049, 8, 7, 9, 300, 64, 3, 1025, 16, 15, 33, 2, 1, 4096, 11]]
    buf = np.concatenate(parts)
    dev = _words_t(buf, name, cuda)
    at, tensors = 0, []
    for p in parts:
        tensors.append(dev[at:at + p.size])
        at += p.size
    assert len(tensors) == 19
    census = _zeros5(cuda)
    assert ops.range16_words(tensors, census) == buf.size
    want = R.words(buf, name)
    assert census.tolist() == R.row(want)
    again = _zeros5(cuda)
    ops.range16_words(tensors, again)
    assert again.tolist() == census.tolist()                    # two calls identical
    ops.range16_words(tensors, census)                          # accumulation into a non-zero record
    assert census.tolist() == R.row(R.add(want, want))
    assert ops.range16_words([], census) == 0 and ops.range16_words([dev[:0]], census) == 0
    # a non-contiguous NHWC slice: counted through its contiguous rows
    x = _spread(2 * 6 * 10 * 64, 22, -20, 10).reshape(2, 6, 10, 64)      # (|x| < 2^13: nothing but the 7e4 below leaves fp16's range)
    x[1, 2, 4, 7], x[0, 0, 0, 0] = np.float32(7e4), np.float32("nan")      # inside / outside the slice below
    t16 = torch.from_numpy(x).to(cuda).to(DTYPES[name])
    view = t16[:, 1:5, 2:9]
    assert not view.is_contiguous()
    c = _zeros5(cuda)
    assert ops.range16_words([view], c) == view.numel()
    o16 = view.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)
    assert c.tolist() == R.row(R.words(o16, name)) and c[1].item() == (1 if name == "fp16" else 0)
    x32 = torch.from_numpy(x).to(cuda)
    c = _zeros5(cuda)
    ops.range16_as_rounded([x32[:, 1:5, 2:9]], name, c)
    assert c.tolist() == R.row(R.as_rounded(x[:, 1:5, 2:9], name))
    with pytest.raises(ValueError, match="contiguous rows"):
        ops.range16_words([t16.permute(3, 0, 1, 2)], c)
    with pytest.raises(ValueError):
        ops.range16_words([x32], c)                               # fp32 words
    with pytest.raises(ValueError):
        ops.range16_as_rounded([t16], name, c)
    with pytest.raises(ValueError):
        ops.range16_words([t16], torch.zeros(5, dtype=torch.int32, device=cuda))
    # all zeros, all NaN
    for fill, rec in ((0.0, [0, 0, 0, 0, 0]), (float("nan"), [0, 3001, 0, 0, 0])):
        c = _zeros5(cuda)
        ops.range16_words([torch.full((3001,), fill, dtype=DTYPES[name], device=cuda)], c)
        assert c.tolist() == rec
        c = _zeros5(cuda)
        ops.range16_as_rounded([torch.full((3001,), fill, device=cuda)], name, c)
        assert c.tolist() == rec


def test_past_the_grid_cap(ops, cuda):
    """2^24 + 13 elements: 2049 workgroup passes of words on a grid of 2048"""
    n = (1 << 24) + 13
    g = torch.Generator(device="cpu").manual_seed(5)
    o = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int16)
    c = _zeros5(cuda)
    assert ops.range16_words([o.to(cuda).view(torch.float16)], c) == n
    assert c.tolist() == R.row(R.words(o.numpy().view(np.uint16), "fp16"))
    x = o.view(torch.float16).float()
    x[-5] = 65520.0
    c = _zeros5(cuda)
    ops.range16_as_rounded([x.to(cuda)], "fp16", c)
    assert c.tolist() == R.row(R.as_rounded(x.numpy(), "fp16")) and c[2].item() == 1


# ---------------------------------------------------------------------------------------------------------------- the model
_NETS = {}
_SHARED = {}


def _net(cuda, hot=None, tag="x4"):
    if (hot, tag) not in _NETS:
        from eavsr_amd.eavsrp_model import EAVSRP
        net = EAVSRP(Namespace(predict=False, n_frame=7, n_flow=5, scale=4 if tag == "x4" else 2), None)
        net.load_state_dict(K.state_dict(tag, hot), strict=True)
        _NETS[(hot, tag)] = net.to(cuda).eval()
    return _NETS[(hot, tag)]


def _clip(cuda, seed=41, t=5):
    return K.clip_u8(1, t, 64, 64, seed).to(cuda).float() / 255


def _unchecked(cuda, N, hot, name, how="forward", tag="x4"):
    """the unchecked run under backbone dtype `name`, computed once and never written to"""
    key = (hot, name, how, tag)
    if key not in _SHARED:
        net = _net(cuda, hot, tag)
        with torch.no_grad(), N.backbone_dtype(name):
            _SHARED[key] = net(_clip(cuda)) if how == "forward" else net.forward_long(_clip(cuda), frame_chunk=2)
    return _SHARED[key]


def _spied(ops, monkeypatch, fn):
    """run fn, unchecked, with a spy on the launch wrapper and on `ops.range_mark`: every tensor a census WOULD count, copied to the
    host, under the key the census would give it -- (scope, entry point, flavour, position since the scope's last mark) -- in launch
    order; and every launch's name"""
    seen, names, state = [], [], {"scope": "", "pos": {}}
    plain = ops._launch_plain

    def mark(scope):
        state["scope"], state["pos"] = str(scope), {}

    def key(what, flavour):
        k = state["pos"].get((what, flavour), 0)
        state["pos"][(what, flavour)] = k + 1
        return (state["scope"], what, flavour, k)

    def spy(name, flops, nbytes, t, launch, what, stored=None, rounded=None):
        names.append(what)
        if rounded is not None:
            seen.append((key(what, "as_rounded"), [s.detach().cpu().numpy().copy() for s in rounded[0]]))
        plain(name, flops, nbytes, t, launch, what)
        if stored:
            seen.append((key(what, "words"), [s.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy() for s in stored]))
    with monkeypatch.context() as m:
        m.setattr(ops, "_launch", spy)
        m.setattr(ops, "range_mark", mark)
        out = fn()
    return out, seen, names


def _reference_sites(seen, name):
    """{key: (the reference's record summed over the key's launches, the 1-based count of counting launches at which the key first
    held a non-finite or overflowed element, 0: never)}, the keys in the order of their first launch"""
    ref = {}
    for tick, (key, arrs) in enumerate(seen, 1):
        flat = np.concatenate([a.reshape(-1) for a in arrs])
        rec = R.words(flat, name) if key[2] == "words" else R.as_rounded(flat, name)
        old, at = ref.get(key, (None, 0))
        rec = rec if old is None else R.add(old, rec)
        ref[key] = (rec, at or (tick if rec["nonfinite"] + rec["overflow"] > 0 else 0))
    return ref


def _same_sites(sites, ref, name):
    """every site's record, name, headroom and stamp equal the reference's, site by site, in call order"""
    assert [(s["scope"], s["op"], s["flavour"], s["index"]) for s in sites] == list(ref)
    for s, (key, (rec, at)) in zip(sites, ref.items()):
        assert {k: s[k] for k in rec} == rec, (key, s, rec)
        assert s["tripped_at"] == at and s["dtype"] == name and s["headroom"] == R.headroom(rec["max_abs"], name), (key, s, at)
        assert s["site"] == f"{key[0] or '-'}/{key[1]}#{key[3]}" + (":in" if key[2] == "as_rounded" else "")


def _launch_names(ops, monkeypatch, fn):
    names = []
    real = ops._launch

    def spy(name, flops, nbytes, t, launch, what, **kw):
        names.append(what)
        return real(name, flops, nbytes, t, launch, what, **kw)
    with monkeypatch.context() as m:
        m.setattr(ops, "_launch", spy)
        out = fn()
    return out, names


@pytest.mark.parametrize("tag, name", [("x4", "fp16"), ("x4", "bf16"), ("x2", "fp16")])
def test_report_changes_no_frame_and_counts_every_site(ops, N, cuda, monkeypatch, name, tag):
    net, x = _net(cuda, None, tag), _clip(cuda)
    want = _unchecked(cuda, N, None, name, "forward", tag)
    with torch.no_grad(), N.backbone_dtype(name):
        net.backbone_census.clear()
        with N.backbone_check("report"):
            got = net(x)
        assert torch.equal(_bits32(got), _bits32(want)) and len(net.backbone_census) == 1
        entry = net.backbone_census.pop()
        assert {k: entry[k] for k in ("asked", "used", "fallback", "tail_fallback", "frames", "size")} == dict(
            asked=name, used=name, fallback=False, tail_fallback=[], frames=5, size=(64, 64))
        # the reference, applied to what a spy on the launch wrapper of a second, unchecked run saw
        _, seen, names = _spied(ops, monkeypatch, lambda: net(x))
    assert not any(nm.startswith("range16") for nm in names) and len(seen) > 300
    sites, ref = entry["sites"], _reference_sites(seen, name)
    # site by site: the record of every (scope, entry point, flavour, position) is the reference summed over that key's launches --
    # the five time steps of a branch share the rows of the first -- and no site is uncounted or unfed
    assert 100 < len(ref) < len(seen) and sum(s["elements"] for s in sites) == sum(a.size for _, arrs in seen for a in arrs)
    _same_sites(sites, ref, name)
    ops16 = {s["op"] for s in sites}
    assert {"nchw_f32_to_nhwc_h16", "conv3x3_c64_h16_b", "conv3x3_c64_h16_res", "conv3x3_c64_h16", "conv3x3_c64_h16_act", "conv3x3_h16g",
            "conv_h16x1", "flow_warp_pair"} <= ops16, ops16
    assert {s["scope"] for s in sites} == {"spynet", "encoder", "backward_1", "forward_1", "backward_2", "forward_2", "tail"}
    assert len([s for s in sites if s["op"] == "conv3x3_c64_h16_act" and s["scope"] == "tail"]) == (3 if tag == "x4" else 2)
    assert all(s["nonfinite"] == 0 and s["overflow"] == 0 and s["headroom"] > 1 and s["tripped_at"] == 0 for s in sites)
    assert all(s["flushed"] == 0 for s in sites if s["flavour"] == "words")


def test_unset_launches_what_the_hook_free_wrapper_launches(ops, N, cuda, monkeypatch):
    net, x = _net(cuda), _clip(cuda)
    with torch.no_grad(), N.backbone_dtype("fp16"):
        assert N.BACKBONE_CHECK is None and ops.RANGE16 is None
        got, names = _launch_names(ops, monkeypatch, lambda: net(x))
        with monkeypatch.context() as m:      # the hook removed: the wrapper as it was before the census
            m.setattr(ops, "_launch", lambda name, flops, nbytes, t, fn, what, stored=None, rounded=None:
                      (names_plain.append(what), ops._launch_plain(name, flops, nbytes, t, fn, what))[1])
            names_plain = []
            want = net(x)
        assert names == names_plain and torch.equal(got, want) and not any(n.startswith("range16") for n in names)
        assert net.backbone_census == []
        with N.backbone_check("report"):
            _, checked = _launch_names(ops, monkeypatch, lambda: net(x))
        assert [n for n in checked if not n.startswith("range16")] == names and len(checked) > len(names)
        net.backbone_census.clear()


def test_an_overflowing_block_is_reported_refused_or_run_in_bf16(ops, N, cuda, monkeypatch):
    net, x = _net(cuda, "block"), _clip(cuda)
    want16, want_bf = _unchecked(cuda, N, "block", "fp16", "long"), _unchecked(cuda, N, "block", "bf16", "long")
    assert torch.isfinite(want_bf).all() and not torch.isfinite(want16).all()
    want_bf_forward = _unchecked(cuda, N, "block", "bf16")
    sunk = []
    with torch.no_grad(), N.backbone_dtype("fp16"):
        net.backbone_census.clear()
        with N.backbone_check("report"):
            got = net.forward_long(x, frame_chunk=2)
        assert torch.equal(_bits32(got), _bits32(want16))
        first = N.tripped(net.backbone_census[0]["sites"])[0]
        assert first["scope"] == "backward_1" and first["index"] == 0 and first["op"] in ("conv3x3_c64_h16_res", "conv3x3_c64_h16")
        assert first["nonfinite"] > 0 and first["max_abs"] <= 65504.0
        with N.backbone_check("raise"), pytest.raises(N.BackboneRangeError, match="first at " + re.escape(first["site"])) as info:
            net.forward_long(x, frame_chunk=2, sink=lambda a, sr: sunk.append(a))
        assert sunk == [] and info.value.site["site"] == first["site"] and info.value.entry is net.backbone_census[1]
        with N.backbone_check("raise"), pytest.raises(N.BackboneRangeError):
            net(x)
        with N.backbone_check("bf16"):
            got = net.forward_long(x, frame_chunk=2)
            assert N.BACKBONE_DTYPE == "fp16"
        entry = net.backbone_census[3]
        assert torch.equal(_bits32(got), _bits32(want_bf))
        assert (entry["asked"], entry["used"], entry["fallback"], entry["tail_fallback"]) == ("fp16", "bf16", True, [])
        assert N.tripped(entry["sites"])[0]["site"] == first["site"] and not N.tripped(entry["sites_used"])
        with N.backbone_check("bf16"):
            assert torch.equal(_bits32(net(x)), _bits32(want_bf_forward))
        # every site's record and WHEN it first left the range, against the reference over a spied, unchecked run of `forward`
        net.backbone_census.clear()
        with N.backbone_check("report"):
            net(x)
        sites = net.backbone_census.pop()["sites"]
        _, seen, _ = _spied(ops, monkeypatch, lambda: net(x))
        ref = _reference_sites(seen, "fp16")
        _same_sites(sites, ref, "fp16")
        order = [s["site"] for s in N.tripped(sites)]
        assert order[0] == first["site"] and len(order) > 50 and len({s["tripped_at"] for s in N.tripped(sites)}) == len(order)
        assert [s["site"] for s in sites if s["tripped_at"]] != order      # call order is NOT the order in time: rows are shared
        net.backbone_census.clear()


def test_one_window_of_two_falls_back(N, cuda):
    """the synthetic weights; the input frames of the second window scaled: that window alone leaves fp16's range"""
    net = _net(cuda)
    x = _clip(cuda, t=6).clone()
    x[:, 3:] *= 3.0e4
    plan = [(0, 3, 0, 3), (3, 6, 3, 6)]
    with torch.no_grad():
        with N.backbone_dtype("fp16"):
            w16 = net.forward_segments(x, plan)
        with N.backbone_dtype("bf16"):
            wbf = net.forward_segments(x, plan)
        assert torch.isfinite(w16[:, :3]).all() and not torch.isfinite(w16[:, 3:]).all() and torch.isfinite(wbf).all()
        net.backbone_census.clear()
        with N.backbone_dtype("fp16"), N.backbone_check("bf16"):
            got = net.forward_segments(x, plan)
        assert [e["fallback"] for e in net.backbone_census] == [False, True]      # per window, not sticky
        assert torch.equal(_bits32(got[:, :3]), _bits32(w16[:, :3])) and torch.equal(_bits32(got[:, 3:]), _bits32(wbf[:, 3:]))
        net.backbone_census.clear()


def test_a_tail_that_overflows_falls_back_chunk_by_chunk(ops, N, cuda, monkeypatch):
    net, x = _net(cuda, "tail"), _clip(cuda)
    want16 = _unchecked(cuda, N, "tail", "fp16", "long")
    chunks = [a for a in (0, 2, 4) if not torch.isfinite(want16[:, a:a + 2]).all()]
    assert chunks, "conv_hr's scale must leave fp16's range in some chunk"
    calls = []      # (the backbone dtype of the call, clones of its inputs), in order
    tail = net._upsample_tm

    def recording(srcs, lq):
        calls.append((N.BACKBONE_DTYPE, [s.clone() for s in srcs], lq.clone()))
        return tail(srcs, lq)
    sunk = []
    with torch.no_grad(), N.backbone_dtype("fp16"):
        net.backbone_census.clear()
        with N.backbone_check("bf16"), monkeypatch.context() as m:
            m.setattr(net, "_upsample_tm", recording)
            got = net.forward_long(x, frame_chunk=2, sink=lambda a, sr: sunk.append((a, sr.clone())))
        entry = net.backbone_census.pop()
        assert got is None and [a for a, _ in sunk] == [0, 2, 4]
        assert entry["fallback"] is False and entry["used"] == "fp16" and entry["tail_fallback"] == chunks
        first = N.tripped(entry["sites"])[0]
        assert first["scope"] == "tail" and first["op"] == "conv3x3_c64_h16_act"
        # a chunk that fell back: the bf16 tail on the features the fp16 stages made; the others: the fp16 run's frames
        assert [c[0] for c in calls] == [d for a in (0, 2, 4) for d in (("fp16", "bf16") if a in chunks else ("fp16",))]
        at = 0
        for a, sr in sunk:
            if a in chunks:      # the second call ran on the tensors of the first ...
                (_, srcs, lq), (_, srcs2, lq2) = calls[at], calls[at + 1]
                assert all(torch.equal(p, q) for p, q in zip(srcs + [lq], srcs2 + [lq2]))
                with N.backbone_dtype("bf16"), ops.route_batch(5):
                    ref = tail(srcs, lq)      # ... and is the bf16 tail on them
                assert torch.equal(_bits32(sr.transpose(0, 1).reshape(ref.shape)), _bits32(ref)) and torch.isfinite(sr).all(), a
                at += 2
            else:
                assert torch.equal(_bits32(sr), _bits32(want16[:, a:a + 2])), a
                at += 1
        seen = []
        with N.backbone_check("raise"), pytest.raises(N.BackboneRangeError, match="the tail of the chunk at frame %d" % chunks[0]):
            net.forward_long(x, frame_chunk=2, sink=lambda a, sr: seen.append(a))
        assert seen == [a for a in (0, 2, 4) if a < chunks[0]]
        net.backbone_census.clear()


def test_tiles_ensemble_and_the_16_bit_cache_with_report(N, cuda):
    net = _net(cuda)
    with torch.no_grad(), N.backbone_dtype("fp16"):
        u8 = K.clip_u8(1, 3, 64, 112, 31).to(cuda)
        x = K.clip_u8(1, 5, 64, 64, 41).to(cuda)
        want = (net.forward_tiled(u8, 64, overlap=16), net.forward_ensemble(x, ensemble=2),
                net.forward_long(x, frame_chunk=2, cache_dtype="fp16", cache_check="report"))
        net.backbone_census.clear()
        net.cache_census.clear()
        with N.backbone_check("report"):
            assert torch.equal(net.forward_tiled(u8, 64, overlap=16), want[0]) and len(net.backbone_census) == 2      # two tiles
            assert torch.equal(net.forward_ensemble(x, ensemble=2), want[1]) and len(net.backbone_census) == 4      # two modes
            assert torch.equal(net.forward_long(x, frame_chunk=2, cache_dtype="fp16", cache_check="report"), want[2])
        assert len(net.backbone_census) == 5 and len(net.cache_census) == 1
        assert all(e["sites"] and not N.tripped(e["sites"]) and e["frames"] in (3, 5) for e in net.backbone_census)
        net.backbone_census.clear()
        net.cache_census.clear()


def test_the_cache_census_describes_the_store_that_a_fallen_back_window_used(N, cuda):
    """the block network, fp16 backbone, a bf16 cache (the block's 1e6 fits it) with a cache_check: the backbone's fallback refills the
    store `checked_window` owns, so the cache census is the bf16 re-run's -- finite -- and "raise" on the cache has nothing to refuse"""
    from eavsr_amd import framestore as FS
    net, x = _net(cuda, "block"), _clip(cuda)
    with torch.no_grad():
        net.cache_census.clear()
        with N.backbone_dtype("bf16"):
            want = net.forward_long(x, frame_chunk=2, cache_dtype="bf16", cache_check="report")
            want_keys = net.cache_census.pop()["keys"]
        assert torch.isfinite(want).all() and not FS.out_of_range(want_keys) and max(r["max_abs"] for r in want_keys.values()) > 65520
        with N.backbone_dtype("fp16"):
            net.backbone_census.clear()
            for check in ("report", "raise"):
                with N.backbone_check("bf16"):
                    got = net.forward_long(x, frame_chunk=2, cache_dtype="bf16", cache_check=check)
                assert torch.equal(_bits32(got), _bits32(want)), check
                entry = net.cache_census.pop()
                assert entry["keys"] == want_keys and entry["fallback"] is False and entry["used"] == "bf16", check
                assert net.backbone_census.pop()["fallback"] is True and net.cache_census == []
            # the fp16 attempt's poisoned store is what a cache census says where the backbone does not fall back: refused
            with N.backbone_check("report"), pytest.raises(FS.CacheRangeError):
                net.forward_long(x, frame_chunk=2, cache_dtype="bf16", cache_check="raise")
            assert FS.out_of_range(net.cache_census.pop()["keys"])
        net.cache_census.clear()
        net.backbone_census.clear()


def _wrapper(**extra):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    model = EAVSRPModel(Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0], **extra))
    model.netEAVSRP.load_state_dict(K.state_dict("x4"), strict=True)
    model.eval()
    return model


def test_super_resolve_evaluate_and_the_refusals(ops, N, cuda, monkeypatch):
    from eavsr_amd import harness
    for var in ("EAVSR_BACKBONE_CHECK", "EAVSR_CACHE_DTYPE", "EAVSR_CACHE_CHECK", "EAVSR_FRAME_CHUNK", "EAVSR_CPU_CACHE", "EAVSR_MAX_FRAMES"):
        monkeypatch.delenv(var, raising=False)
    net = _net(cuda)
    u8 = K.clip_u8(1, 5, 64, 64, 41)
    hr = torch.zeros(5, 3, 256, 256, dtype=torch.uint8)
    with N.backbone_dtype("fp16"):
        plain = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=2)
        assert "backbone_census" not in plain and "backbone_range" not in plain and net.backbone_census == []
        with N.backbone_check("report"):
            res = harness.super_resolve(net, u8[0], hr=hr, frame_chunk=2)
        assert res["frame_psnr"] == plain["frame_psnr"] and res["backbone_census"] is net.backbone_census and len(net.backbone_census) == 1
        line = res["backbone_range"]
        assert line == N.range_summary(net.backbone_census) and line["windows"] == 1 and line["fallbacks"] == [] and line["nonfinite"] == 0
        assert 0 < line["max_abs"] < 65504 and line["headroom"] == 65504.0 / line["max_abs"] and line["worst_site"]
        # evaluate: the wrapper reads opt.backbone_check
        lr = torch.from_numpy(np.float32(u8.numpy()) / np.float32(255))
        item = {"lr_seq": lr, "hr_seq": torch.zeros(1, 5, 3, 256, 256), "fname": ["000_%05d.png" % i for i in range(5)]}
        wrapper = _wrapper(backbone_check="raise")
        assert wrapper.backbone_check == "raise"
        out = harness.evaluate(wrapper, [item], per_frame=True)
        with torch.no_grad():
            want = net(lr.to(cuda))      # (the unchecked forward of the item's own frames, divided on the host as the loader does)
        assert torch.equal(_bits32(wrapper.data_sr_seq), _bits32(want))
        assert len(out["backbone_census"]) == 1 and out["backbone_range"]["overflow"] == 0 and out["backbone_census"][0]["asked"] == "fp16"
        assert "backbone_census" not in harness.evaluate(_wrapper(), [item], per_frame=True)
    net.backbone_census.clear()
    # refusals, before any launch
    x = _clip(cuda)
    names = []
    with monkeypatch.context() as m:
        real = ops._launch
        m.setattr(ops, "_launch", lambda *a, **k: (names.append(a[5]), real(*a, **k))[1])
        with torch.no_grad():
            monkeypatch.setattr(N, "BACKBONE_CHECK", "report")      # a check that outlived its backbone
            for fn in (lambda: net(x), lambda: net.forward_long(x, frame_chunk=2), lambda: harness.super_resolve(net, u8[0])):
                with pytest.raises(ValueError, match="without a 16-bit backbone"):
                    fn()
            monkeypatch.setattr(N, "BACKBONE_CHECK", None)
            with N.backbone_dtype("bf16"):
                with pytest.raises(ValueError, match="fp16 backbone"):
                    N.set_backbone_check("bf16")
        with N.backbone_dtype("fp16"), N.backbone_check("report"), pytest.raises(ValueError, match="under autograd"):
            net(x)
    assert names == [] and net.backbone_census == []


def test_report_is_capturable_and_raise_under_capture_is_refused(N, cuda, monkeypatch):
    net, x = _net(cuda), _clip(cuda)
    with torch.no_grad(), N.backbone_dtype("fp16"):
        net.backbone_census.clear()
        with N.backbone_check("report"):
            eager = net(x)
            want = net.backbone_census.pop()["sites"]
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                net(x)      # (warm-up on the side stream: every packed weight is in its cache)
                net.backbone_census.clear()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = net(x)
            entry = net.backbone_census.pop()
            assert entry["sites"] is None
            for _ in range(2):
                graph.replay()
                torch.cuda.synchronize()
                assert entry["pending"].read() == want and torch.equal(out, eager)
            # "raise" reads the census back: refused where the stream is capturing (asked of torch, answered here by a stand-in: a
            # capture that ends in an exception is not something to stage on a shared device)
            with N.backbone_check("raise"), monkeypatch.context() as m:
                m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
                with pytest.raises(ValueError, match="under stream capture"):
                    net(x)
        net.backbone_census.clear()
