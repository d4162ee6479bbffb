"""Self-ensemble inference, what needs no GPU: the eight modes and their inverses, the ensemble spec in every spelling, the
valid region by brute force, transcriptions of the four kernels' address arithmetic against numpy slicing, the C ABI's entry points,
and the argument checks that come before any device work."""
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from eavsr_amd import segments as S
from tests import ensemble_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = range(8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the modes
def test_inv_after_g_is_the_identity_on_non_square_arrays():
    x = np.arange(2 * 3 * 5 * 7, dtype=np.float32).reshape(2, 3, 5, 7)
    seen = set()
    for k in MODES:
        z = E.g(x, k)
        assert z.shape == ((2, 3, 7, 5) if k & 4 else (2, 3, 5, 7))
        assert np.array_equal(E.inv(z, k), x)
        seen.add(np.ascontiguousarray(z).tobytes())
    assert len(seen) == 8                                             # eight different arrangements
    assert np.array_equal(E.g(x, 1), x[..., ::-1]) and np.array_equal(E.g(x, 2), x[..., ::-1, :])
    assert np.array_equal(E.g(x, 4), x.swapaxes(-1, -2)) and np.array_equal(E.g(x, 7), x[..., ::-1, ::-1].swapaxes(-1, -2))


# ------------------------------------------------------------------------------------------------------------- the spec
def test_check_ensemble_takes_every_spelling():
    assert S.check_ensemble(None) is None and S.check_ensemble(1) is None
    assert S.check_ensemble(2) == (0, 1)
    assert S.check_ensemble(4) == S.check_ensemble("flips") == (0, 1, 2, 3)
    assert S.check_ensemble(8) == tuple(range(8))
    assert S.check_ensemble((0,)) == (0,) and S.check_ensemble([5, 0]) == (0, 5) and S.check_ensemble((7, 3, 1)) == (1, 3, 7)
    assert S.check_ensemble(list(range(8))) == tuple(range(8))


@pytest.mark.parametrize("bad", [0, 3, 5, 16, -1, True, False, 8.0, "8", "all", "", (), [], (0, 0), (0, 8), (-1,), (0, 1.0), (True,), {0, 1},
                                 ("flips",), ((0, 1),), b"8"])
def test_check_ensemble_refuses(bad):
    with pytest.raises(ValueError, match="ensemble"):
        S.check_ensemble(bad, "ensemble")


def test_ensemble_options(monkeypatch):
    from eavsr_amd.eavsrp_model import long_clip_options
    monkeypatch.delenv("EAVSR_ENSEMBLE", raising=False)
    assert S.ensemble_options(None) is None and S.ensemble_options(Namespace(ensemble=None)) is None
    assert S.ensemble_options(Namespace(ensemble=8)) == tuple(range(8))
    assert S.ensemble_options(Namespace(ensemble="flips")) == (0, 1, 2, 3) and S.ensemble_options(Namespace(ensemble="0,1,4")) == (0, 1, 4)
    assert S.ensemble_options(Namespace(ensemble=(4, 0))) == (0, 4) and S.ensemble_options(Namespace(ensemble=1)) is None
    for text, want in (("8", tuple(range(8))), ("4", (0, 1, 2, 3)), ("flips", (0, 1, 2, 3)), ("2", (0, 1)), ("1", None), ("0,1,4", (0, 1, 4)),
                       ("4,0", (0, 4)), ("0", (0,)), ("5", (5,)), ("", None)):
        monkeypatch.setenv("EAVSR_ENSEMBLE", text)
        assert S.ensemble_options(None) == want, text
        assert S.ensemble_options(Namespace(ensemble=2)) == (0, 1)      # the options beat the environment
    for bad in ("9", "0,0", "0,8", "a", "0,", ",", "-1", "8.0", "flip", "0 1"):
        monkeypatch.setenv("EAVSR_ENSEMBLE", bad)
        with pytest.raises(ValueError, match="EAVSR_ENSEMBLE"):
            S.ensemble_options(None)
        with pytest.raises(ValueError, match="EAVSR_ENSEMBLE"):
            long_clip_options(Namespace())      # validated with the others
        assert S.ensemble_options(Namespace(ensemble=8)) == tuple(range(8))      # a bad environment is not read where opt decides
    monkeypatch.delenv("EAVSR_ENSEMBLE")
    for bad in (3, "3,3", True, 8.0, (), (0, 9)):
        with pytest.raises(ValueError, match="opt.ensemble"):
            S.ensemble_options(Namespace(ensemble=bad))
        with pytest.raises(ValueError, match="opt.ensemble"):
            long_clip_options(Namespace(ensemble=bad))
    assert long_clip_options(Namespace(ensemble="flips")) == (None, False)


def test_the_weights_are_exact_for_2_4_and_8():
    for spec in (2, 4, 8):
        modes = S.check_ensemble(spec)
        wgt = S.ensemble_weight(modes)
        assert wgt.dtype == np.float32 and wgt == E.weight(modes) and float(wgt) * len(modes) == 1.0
        assert np.frexp(wgt)[0] == 0.5                                # a power of two: wy * weight rounds nothing away
        wy = np.random.default_rng(spec).random(64, dtype=np.float32)
        assert np.array_equal((wy * wgt).astype(np.float64) * len(modes), wy.astype(np.float64))
    assert S.ensemble_weight((0, 1, 4)) == np.float32(1) / np.float32(3)


# ------------------------------------------------------------------------------------------------------------- the valid region
def test_valid_region_by_brute_force():
    """h, w in 1 .. 80: g_k of the padded index image, cut to the region and inverted, is the unpadded image (scale 1; at scale s every
    bound is s times that)"""
    for h in range(1, 81):
        for w in range(1, 81):
            H, W = S.padded_size(h, w)
            img = np.full((H, W), -1, np.int64)
            img[:h, :w] = np.arange(h * w).reshape(h, w)
            for k in MODES:
                r0, r1, c0, c1 = S.valid_region(k, h, w, H, W, 1)
                assert (r0, r1, c0, c1) == E.valid_region(k, h, w, H, W, 1)
                back = E.inv(E.g(img, k)[r0:r1, c0:c1], k)
                assert back.shape == (h, w) and np.array_equal(back, img[:h, :w]), (k, h, w)
    assert S.valid_region(0, 66, 70, 68, 72, 4) == (0, 264, 0, 280) and S.valid_region(3, 66, 70, 68, 72, 4) == (8, 272, 8, 288)
    assert S.valid_region(5, 66, 70, 68, 72, 4) == (8, 288, 0, 264) and S.valid_region(6, 66, 70, 68, 72, 2) == (0, 140, 4, 136)
    for s in (2, 4):
        for k in MODES:
            assert S.valid_region(k, 50, 70, 64, 72, s) == tuple(s * v for v in S.valid_region(k, 50, 70, 64, 72, 1)) == E.valid_region(k, 50, 70, 64, 72, s)
    for bad in ((8, 4, 4, 4, 4, 1), (-1, 4, 4, 4, 4, 1), (0, 5, 4, 4, 4, 1), (0, 4, 0, 4, 4, 1), (0, 4, 4, 4, 4, 0)):
        with pytest.raises(ValueError):
            S.valid_region(*bad)


# ------------------------------------------------------------------------------------------------------------- the kernels, restated
def _frames(F, C, H, W, seed):
    x = np.random.default_rng(seed).standard_normal((F, C, H, W)).astype(np.float32)
    special = np.array([0x7FC01234, 0xFF800000, 0x80000000], np.uint32)[:x.size]      # a NaN with a payload, -inf, -0: bits are kept
    x.reshape(-1)[:special.size].view(np.uint32)[:] = special
    return x


@pytest.mark.parametrize("k", MODES)
def test_dihedral_address_arithmetic_is_numpy_slicing(k):
    """1 x 1, 3 x 5, 7 x 18 (mirrored quads and a tail of 2), 66 x 70 (four LDS tiles, tails on both axes), 4 x 260 (a second pass along
    the row), planes F x C = 2 x 2 and 1 x 1, sources and destinations at every alignment class"""
    seen = {16: 0, 8: 0, 4: 0}
    for (F, C, H, W), bases in (((1, 1, 1, 1), (0, 0)), ((2, 2, 3, 5), (16, 4)), ((1, 2, 7, 18), (8, 16)), ((1, 1, 66, 70), (4, 8)),
                                ((1, 1, 4, 260), (32, 48)), ((1, 1, 6, 16), (0, 0))):
        x = _frames(F, C, H, W, seed=H * W + k)
        got, widths = E.dihedral_transcription(x, k, bases=bases)
        assert got.shape == E.g(x, k).shape and np.array_equal(_bits(got), _bits(E.g(x, k))), (k, F, C, H, W)
        for a in seen:
            seen[a] += widths[a]
    assert seen[4] > 0 and (k & 4 or (seen[16] > 0 and seen[8] > 0)), seen
    x = _frames(1, 1, 11, 9, seed=k)
    assert np.array_equal(_bits(E.dihedral_transcription(x, k, grid_x=1)[0]), _bits(E.g(x, k)))      # one workgroup strides over all rows


@pytest.mark.parametrize("X0", [0, 1, 2, 3])
@pytest.mark.parametrize("k", MODES)
def test_blend_dihedral_address_arithmetic_is_numpy(k, X0):
    """a strided (frame-major, cropped) source into 2 x 2 x 2 x 30 x 84; tiles of 10 x 16, 10 x 18 (a quad tail of 2) and 9 x 70 (two LDS
    tiles along one axis, a tail on both); acc, source and weights at every alignment class; everything outside the tile untouched"""
    rng = np.random.default_rng(8 * k + X0)
    n, F, C, SH, SW = 2, 2, 2, 30, 84
    for (th, tw), bases in (((10, 16), (0, 0, 0, 0)), ((10, 18), (16, 8, 4, 8)), ((9, 70), (32, 4, 0, 12))):
        rows_s, row_s = (tw, th) if k & 4 else (th, tw)
        Hp, Wp = rows_s + 3, row_s + 5                               # the source is a window of padded frames of Hp x Wp, frame-major
        off = 5 + 2 * Wp + 3                                          # ... that starts 2 rows and 3 columns in
        store = rng.standard_normal(F * n * C * Hp * Wp + 8).astype(np.float32)
        strides = (C * Hp * Wp, n * C * Hp * Wp, Hp * Wp, Wp)         # (F, n, C, Hp, Wp) transposed to (n, F, ...)
        view = np.lib.stride_tricks.as_strided(store[off:], (n, F, C, rows_s, row_s), tuple(4 * v for v in strides + (1,)))
        acc = rng.standard_normal((n, F, C, SH, SW)).astype(np.float32)
        wy, wx = rng.random(th, dtype=np.float32), rng.random(tw, dtype=np.float32)
        want = E.blend_oracle(acc.copy(), view, k, 7, X0, wy, wx)
        got, widths = E.blend_dihedral_transcription(acc, store, off, (n, F, C, rows_s, row_s), strides, k, 7, X0, wy, wx, bases=bases)
        assert np.array_equal(_bits(got), _bits(want)), (k, X0, th, tw, bases)
        untouched = np.ones_like(acc, bool)
        untouched[..., 7:7 + th, X0:X0 + tw] = False
        assert np.array_equal(_bits(got[untouched]), _bits(acc[untouched]))
    got, _ = E.blend_dihedral_transcription(acc, store, off, (n, F, C, rows_s, row_s), strides, k, 7, X0, wy, wx, grid_x=1)
    assert np.array_equal(_bits(got), _bits(want))


def test_blend_of_a_transformed_frame_with_unit_weights_restores_it():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 2, 3, 9, 13)).astype(np.float32)
    ones = lambda m: np.ones(m, np.float32)
    for k in MODES:
        z = np.ascontiguousarray(E.g(x, k))
        got = E.blend_oracle(np.zeros_like(x), z, k, 0, 0, ones(9), ones(13))
        assert np.array_equal(got, x)
    mean = E.ensemble_blend([[np.ascontiguousarray(E.g(x, k)) for k in MODES]], [(0, 9, 0, 13)], tuple(MODES), 9, 13, 1,
                            np.ones((1, 9), np.float32), np.ones((1, 13), np.float32), 1)
    assert np.abs(mean - x).max() <= 8 * 2.0 ** -24 * np.abs(x).max()      # eight equal terms of x / 8, summed in fp32


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_in_the_stable_section_and_bound():
    from eavsr_amd import _native as N, build, ops
    with open(os.path.join(ROOT, "include", "eavsr_hip.h")) as f:
        header = f.read()
    stable = header[:header.index("EXPERIMENTAL -- exported by the LAB build only")]
    for name, count in (("eavsr_dihedral_f32", 8), ("eavsr_blend_dihedral_f32", 19)):
        m = re.search(r"^int %s\(([^;]*)\);" % name, stable, flags=re.M)
        assert m, f"{name} is not declared in the stable section"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, argtypes = N.SIGNATURES[name]
        assert len(args) == len(argtypes) == count
        for a, t in zip(args, argtypes):
            assert (t is N.vp) == ("*" in a), (a, t)
            assert (t is N.i32) == a.startswith("int32_t"), (a, t)
            assert (t is N.i64) == a.startswith("int64_t"), (a, t)
    assert any(p.endswith(os.sep + "blend.hip") for p in build.sources()) and any(p.endswith("blend.hip") for p in build.sources(lab=True))
    assert callable(ops.dihedral) and callable(ops.blend_dihedral)
    with open(os.path.join(ROOT, "eavsr_amd", "csrc", "blend.hip")) as f:
        source = f.read()
    assert "fp contract(off)" in source and "atomic" not in source.lower()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    assert "eavsr_dihedral_f32" in text and "eavsr_blend_dihedral_f32" in text


# ------------------------------------------------------------------------------------------------------------- before any device work
def test_arguments_are_refused_before_anything_runs(monkeypatch):
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    for name in ("EAVSR_ENSEMBLE", "EAVSR_TILE", "EAVSR_TILE_OVERLAP", "EAVSR_PAD_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    net = EAVSRP.__new__(EAVSRP)
    x = torch.zeros(1, 2, 3, 96, 112)
    with torch.no_grad():
        for bad in (3, 0, "8", (0, 0), (8,), True, ()):
            with pytest.raises(ValueError, match="ensemble"):
                EAVSRP.forward_ensemble(net, x, bad)
        with pytest.raises(ValueError, match="tile|overlap"):
            EAVSRP.forward_ensemble(net, x, 8, tile=66)
        with pytest.raises(ValueError, match="tile|overlap"):
            EAVSRP.forward_ensemble(net, x, 8, tile=64, overlap=40)
        with pytest.raises(ValueError, match="pad"):
            EAVSRP.forward_ensemble(net, x, 8, pad="symmetric")
        with pytest.raises(ValueError, match="segments"):
            EAVSRP.forward_ensemble(net, x, 8, segments=[(0, 1, 0, 1)])
        with pytest.raises(ValueError, match="frame_chunk"):
            EAVSRP.forward_ensemble(net, x, 8, frame_chunk=0)
        for bad in (8, -1, 1.0, True, "1"):
            with pytest.raises(ValueError, match="transform"):
                EAVSRP.forward_long(net, x.to(torch.uint8), transform=bad)
    with pytest.raises(RuntimeError, match="no_grad"):
        EAVSRP.forward_ensemble(net, x, 8)
    with pytest.raises(RuntimeError, match="no_grad"):
        EAVSRP.forward_long(net, x, transform=1)
    for bad in (3, "3,3", "9", (0, 0), True, 8.0):
        with pytest.raises(ValueError, match="ensemble"):
            harness.super_resolve(None, ["/nonexistent/frame.png"], ensemble=bad)      # ... before a file is read
    with pytest.raises(ValueError, match="opt.ensemble"):
        harness.super_resolve(Namespace(opt=Namespace(ensemble=3)), x[0])
    monkeypatch.setenv("EAVSR_ENSEMBLE", "7,7")
    with pytest.raises(ValueError, match="EAVSR_ENSEMBLE"):
        harness.super_resolve(None, ["/nonexistent/frame.png"])
    cpu = torch.zeros(1, 1, 1, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.dihedral(torch.zeros(1, 3, 8, 8), 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.blend_dihedral(cpu, torch.zeros(1, 1, 1, 4, 4), 5, 0, 0, torch.ones(4), torch.ones(4))
    with pytest.raises(TypeError):
        ops.dihedral(np.zeros((1, 3, 8, 8), np.float32), 1)
    with pytest.raises(TypeError):
        ops.blend_dihedral(np.zeros((1, 1, 1, 8, 8), np.float32), torch.zeros(1, 1, 1, 4, 4), 5, 0, 0, torch.ones(4), torch.ones(4))
    for bad in (8, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="mode"):
            ops.blend_dihedral(cpu, torch.zeros(1, 1, 1, 4, 4), bad, 0, 0, torch.ones(4), torch.ones(4))


def test_the_published_parameter_lists():
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRP
    assert inspect.signature(EAVSRP.forward_long).parameters["transform"].default is None
    assert inspect.signature(harness.super_resolve).parameters["ensemble"].default is None
    sig = inspect.signature(EAVSRP.forward_ensemble)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [
        ("ensemble", 8), ("tile", None), ("overlap", 32), ("segments", None), ("pad", None), ("frame_chunk", None), ("cache", "device"),
        ("sink", None)]


def test_an_ensemble_that_is_off_is_forward_video():
    """the three methods `forward_video` chooses between replaced by recorders: `forward_ensemble` with 1, None and (0,) makes the call
    `forward_video` makes with the same arguments -- the same method, the same arguments -- and touches nothing else"""
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP.__new__(EAVSRP)
    calls = []
    for name in ("forward_long", "forward_segments_padded", "forward_tiled"):
        net.__dict__[name] = lambda *a, _n=name, **k: calls.append((_n, a, k)) or _n
    x = torch.zeros(1, 4, 3, 96, 112)
    plan = [(0, 3, 0, 2), (1, 4, 2, 4)]
    with torch.no_grad():
        for tile, segments, path in ((64, plan, "forward_tiled"), (64, None, "forward_tiled"), (128, plan, "forward_segments_padded"),
                                     (None, plan, "forward_segments_padded"), (128, None, "forward_long"), (None, None, "forward_long")):
            calls.clear()
            assert net.forward_video(x, segments=segments, tile=tile, tile_overlap=16, pad="edge", frame_chunk=2, cache="host") == path
            want = list(calls)
            assert len(want) == 1 and want[0][0] == path and want[0][1][0] is x
            for spec in (1, None, (0,), [0]):
                calls.clear()
                assert net.forward_ensemble(x, spec, tile=tile, overlap=16, segments=segments, pad="edge", frame_chunk=2, cache="host") == path
                assert calls == want
        calls.clear()
        assert net.forward_ensemble(x, 1, tile=64, overlap=16, segments=plan, pad="edge", frame_chunk=2, cache="host") == "forward_tiled"
    assert calls ==[("forward_tiled", (x, 64), dict(overlap=16, segments=plan, pad="edge", frame_chunk=2, cache="host", sink=None,
                                                     cache_dtype=None))]


# ------------------------------------------------------------------------------------------------------------- the shared loop
def _fake_clip_run(net, calls, blends):
    """`forward_long` and `ops.blend_dihedral` as recorders on a bare network whose clips "run" on the CPU: the first records the
    arguments that decide what it computes and feeds its sink one zero chunk of the shape the real call emits; the second records
    where, under which mode and with which weights that chunk is blended"""
    def forward_long(lrs, frame_chunk=None, cache="device", sink=None, emit=None, pad=None, window=None, transform=None, cache_dtype=None):
        calls.append(dict(frames=int(lrs.shape[1]), window=window, emit=emit, pad=pad, transform=transform or None,      # 0 is None
                          cache_dtype=cache_dtype, frame_chunk=frame_chunk, cache=cache))
        y0, y1, x0, x1 = window or (0, int(lrs.shape[2]), 0, int(lrs.shape[3]))
        th, tw = net.scale * (y1 - y0), net.scale * (x1 - x0)
        sink(emit[0], torch.zeros((int(lrs.shape[0]), emit[1] - emit[0], 3) + ((tw, th) if (transform or 0) & 4 else (th, tw))))

    def blend(acc, sr, k, Y0, X0, wy, wx):
        blends.append((tuple(acc.shape), tuple(sr.shape), k, Y0, X0, wy.numpy().tobytes(), wx.numpy().tobytes()))
    net.__dict__["forward_long"] = forward_long
    net.__dict__["_clip_device"] = lambda lrs: torch.device("cpu")
    return blend


@pytest.mark.parametrize("plan", [None, [(0, 2, 0, 1), (0, 2, 1, 2)]])
def test_the_tiled_and_the_ensemble_path_run_one_accumulator_loop(plan, monkeypatch):
    """1 x 2 x 96 x 112 x 3 bytes, tile 64 at overlap 16 (2 x 2 tiles), one segment and a plan of two: `forward_tiled`,
    `forward_ensemble((0, 5))` on the same tiles and the untiled `forward_ensemble((0, 5))` call `forward_long` tile-major, modes in
    increasing order inside a tile, with exactly the window, emit, pad, transform, cache_dtype, frame_chunk and cache that the plan
    gives; each SR chunk is blended at the tile's place with the tile's rows of `tile_weights`, wy scaled by fp32(1 / modes) on the
    host; the sink gets the accumulator in `frame_chunk` pieces -- copies while a segment is still to come, views after the last"""
    from eavsr_amd import ops
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP.__new__(EAVSRP)
    net.__dict__["scale"] = s = 4
    calls, blends, sunk = [], [], []
    monkeypatch.setattr(ops, "blend_dihedral", _fake_clip_run(net, calls, blends))
    clip = torch.zeros(1, 2, 96, 112, 3, dtype=torch.uint8)
    h, w, t = 96, 112, 2
    tiles = S.plan_tiles(h, w, 64, 16)
    rows, cols = S.tile_axis(h, 64, 16), S.tile_axis(w, 64, 16)
    assert len(tiles) == 4 and len(cols) == 2
    segs = plan or [(0, t, 0, t)]
    sink = lambda first, chunk: sunk.append((first, tuple(chunk.shape), chunk.untyped_storage().data_ptr()))
    common = dict(segments=plan, pad="reflect", frame_chunk=1, cache="host", sink=sink)
    runs = (("tiled", (0,), tiles, rows, cols, "bf16", lambda: net.forward_tiled(clip, 64, overlap=16, cache_dtype="bf16", **common)),
            ("ensemble, tiled", (0, 5), tiles, rows, cols, None, lambda: net.forward_ensemble(clip, (5, 0), tile=64, overlap=16, **common)),
            ("ensemble, tiled, 16-bit cache", (0, 5), tiles, rows, cols, "fp16",
             lambda: net.forward_cached(clip, torch.float16, ensemble=(0, 5), tile=64, overlap=16, **common)),
            ("ensemble", (0, 5), [None], [(0, h)], [(0, w)], None, lambda: net.forward_ensemble(clip, (0, 5), **common)))
    for name, modes, windows, rows_, cols_, cache_dtype, run in runs:
        calls.clear(), blends.clear(), sunk.clear()
        with torch.no_grad():
            assert run() is None, name
        wy = (S.tile_weights(h, rows_, s) * S.ensemble_weight(modes)).astype(np.float32)
        wx = S.tile_weights(w, cols_, s)
        want_calls, want_blends = [], []
        for a, b, ea, eb in segs:
            for ti, window in enumerate(windows):
                y0, y1, x0, x1 = window or (0, h, 0, w)
                for k in modes:
                    want_calls.append(dict(frames=b - a, window=window, emit=(ea - a, eb - a), pad="reflect", transform=k or None,
                                           cache_dtype=cache_dtype, frame_chunk=1, cache="host"))
                    th, tw = s * (y1 - y0), s * (x1 - x0)
                    want_blends.append(((1, eb - ea, 3, s * h, s * w), (1, eb - ea, 3) + ((tw, th) if k & 4 else (th, tw)), k, s * y0, s * x0,
                                        wy[ti // len(cols_)].tobytes(), wx[ti % len(cols_)].tobytes()))
        assert calls == want_calls, name
        assert blends == want_blends, name
        assert [(first, shape) for first, shape, _ in sunk] == [(f, (1, 1, 3, s * h, s * w)) for f in range(t)], name
        # two segments: frame 0 leaves as a copy, segment 1 zeroes and refills the accumulator; one: both chunks are views of it
        assert (sunk[0][2] == sunk[1][2]) == (plan is None), name
    assert S.ensemble_weight((0,)) == np.float32(1) and S.ensemble_weight((0, 5)) == np.float32(0.5)
