"""Spatial tiling, what needs no GPU: the plan by brute force, the blending weights against their scalar restatement
(tests/tile_ref.py) and as a partition of unity, transcriptions of both kernels' address arithmetic against numpy slicing, the C
ABI's entry points, the options, and the argument checks that come before any device work."""
import inspect
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from eavsr_amd import segments as S
from tests import tile_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = (64, 68, 96)


# ------------------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("tile", TILES)
def test_plan_by_brute_force(tile):
    """sizes 1 .. 300, every overlap multiple of 4 up to tile / 2: windows inside the axis, all of side min(tile, size), every sample
    covered, starts strictly increasing, neighbours share at least `overlap` samples, at most 3 windows over a sample"""
    for overlap in range(0, tile // 2 + 1, 4):
        for size in range(1, 301):
            wins = S.tile_axis(size, tile, overlap)
            assert wins == R.plan_axis(size, tile, overlap)
            side = min(tile, size)
            assert all(0 <= a < b <= size and b - a == side for a, b in wins), (size, tile, overlap)
            cover = R.coverage(size, wins, 1)
            assert cover.min() >= 1 and cover.max() <= 3, (size, tile, overlap)
            starts = [a for a, _ in wins]
            assert all(p < q for p, q in zip(starts, starts[1:]))
            assert all(a1 - b0 >= overlap for (_, a1), (b0, _) in zip(wins, wins[1:])), (size, tile, overlap)
            assert wins[0][0] == 0 and wins[-1][1] == size


def test_plan_is_the_row_major_product_of_its_axes():
    plan = S.plan_tiles(96, 112, 64, 16)
    assert plan == [(0, 64, 0, 64), (0, 64, 48, 112), (32, 96, 0, 64), (32, 96, 48, 112)] == R.plan_tiles(96, 112, 64, 16)
    assert S.plan_tiles(70, 300, (64, 96), 32) == R.plan_tiles(70, 300, (64, 96), 32)
    assert S.plan_tiles(50, 60, 64, 32) == [(0, 50, 0, 60)]               # one window, the frame
    assert S.plan_tiles(540, 960, (288, 512), 32) == [(0, 288, 0, 512), (0, 288, 448, 960), (252, 540, 0, 512), (252, 540, 448, 960)]
    assert len({(y1 - y0, x1 - x0) for y0, y1, x0, x1 in S.plan_tiles(299, 301, (68, 96), 20)}) == 1


@pytest.mark.parametrize("tile, overlap", [(60, 0), (66, 0), (63, 0), ((64, 62), 0), ((32, 64), 0), (64, -1), (64, 33), ((64, 128), 40),
                                           ((128, 64), 33), (64.0, 0), (True, 0), ((64, 64, 64), 0), (None, 0), ("64", 0), (64, 1.5)])
def test_plan_refusals(tile, overlap):
    with pytest.raises(ValueError):
        S.plan_tiles(200, 200, tile, overlap)
    with pytest.raises(ValueError):      # ... also where the frame is smaller than the tile: the arguments are wrong, not the frame
        S.plan_tiles(10, 10, tile, overlap)


def test_plan_takes_the_limits():
    assert S.plan_tiles(200, 200, 64, 32)[1] == (0, 64, 32, 96)
    assert S.plan_tiles(200, 200, (64, 128), 32)
    with pytest.raises(ValueError):
        S.plan_tiles(0, 200, 64, 0)


# ------------------------------------------------------------------------------------------------------------- the weights
@pytest.mark.parametrize("scale", [2, 4])
def test_weights_are_the_scalar_restatement_and_a_partition_of_unity(scale):
    for tile, overlap, sizes in ((64, 0, (64, 65, 130)), (64, 32, (1, 63, 96, 97, 129, 130, 200)), (68, 20, (69, 150, 299)),
                                 (96, 48, (100, 193, 300)), (64, 16, (96, 112, 70))):
        for size in sizes:
            wins = S.tile_axis(size, tile, overlap)
            got = S.tile_weights(size, wins, scale)
            assert got.dtype == np.float32 and got.shape == (len(wins), scale * min(tile, size))
            assert np.array_equal(got.view(np.uint32), R.weights(size, wins, scale).view(np.uint32)), (tile, overlap, size)
            cover = R.coverage(size, wins, scale)
            total = np.zeros(scale * size, np.float64)
            for k, (a, b) in enumerate(wins):
                total[scale * a:scale * b] += got[k].astype(np.float64)
                once = cover[scale * a:scale * b] == 1
                assert (got[k][once] == np.float32(1.0)).all()
                assert (got[k] > 0).all()
            assert (np.abs(total - 1.0) <= cover * 2.0 ** -25).all(), (tile, overlap, size, np.abs(total - 1.0).max())


def test_two_neighbours_get_a_linear_ramp():
    wins = S.tile_axis(112, 64, 16)                                   # [0, 64), [48, 112): SR samples 192 .. 255 are shared at x4
    w = S.tile_weights(112, wins, 4)
    right = (np.arange(64) + 0.5) / 64                                # the right window's raw weight is X - 192 + 0.5, the sum 64
    assert np.array_equal(w[1][:64], right.astype(np.float32)) and np.array_equal(w[0][192:], right[::-1].astype(np.float32))
    assert (w[0][:192] == 1).all() and (w[1][64:] == 1).all()
    with pytest.raises(ValueError):
        S.tile_weights(112, [(0, 64), (70, 112)], 4)                  # windows of two lengths
    with pytest.raises(ValueError):
        S.tile_weights(200, [(0, 64), (100, 164)], 4)                 # a gap


# ------------------------------------------------------------------------------------------------------------- the kernels, restated
def _source(kind, F, C, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == R.U8_INTERLEAVED:
        return rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if kind == R.U8_PLANES:
        return rng.integers(0, 256, (F, C, h, w), dtype=np.uint8)
    x = rng.standard_normal((F, C, h, w)).astype(np.float32)
    x.reshape(-1)[:3].view(np.uint32)[:] = (0x7FC01234, 0xFF800000, 0x80000000)      # a NaN with a payload, -inf, -0: bits are kept
    return x


@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("kind", [R.U8_PLANES, R.U8_INTERLEAVED, R.F32_PLANES])
def test_ingest_window_address_arithmetic_is_slicing_then_np_pad(kind, mode):
    """frames of 22 x 27 (a pitch that is no multiple of 4), windows at x0 0 .. 3 and 7, y0 0 and 5, outputs of the window's size, wider
    (W % 4 == 0: reflected quads) and of a width that is no multiple of 4, sources 0 .. 3 bytes (fp32: words) past an aligned address"""
    hwc = kind == R.U8_INTERLEAVED
    x = _source(kind, 2, 3 if hwc else 2, 22, 27, seed=kind)
    for (y0, x0, wh, ww, H, W) in ((0, 0, 16, 16, 16, 16), (5, 1, 16, 16, 16, 16), (5, 2, 12, 20, 16, 24), (0, 3, 22, 8, 24, 8),
                                   (5, 7, 9, 20, 9, 23), (0, 0, 22, 27, 24, 28), (5, 7, 17, 20, 17, 20)):
        want = R.window_oracle(x, y0, x0, wh, ww, H, W, mode, hwc=hwc)
        for off in range(4):
            base = 64 + (4 * off if kind == R.F32_PLANES else off)
            got, wide, narrow = R.ingest_window_transcription(x, y0, x0, wh, ww, H, W, mode, kind, base=base)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, mode, (y0, x0, wh, ww, H, W), off)
    got, _, _ = R.ingest_window_transcription(x, 5, 2, 12, 20, 40, 24, mode, kind, base=3 if kind != R.F32_PLANES else 4, grid_x=2)
    assert np.array_equal(got.view(np.uint32), R.window_oracle(x, 5, 2, 12, 20, 40, 24, mode, hwc=hwc).view(np.uint32))


def test_ingest_window_takes_the_wide_loads_where_the_address_allows():
    x = _source(R.U8_PLANES, 1, 1, 8, 32, seed=1)
    got, wide, narrow = R.ingest_window_transcription(x, 0, 4, 8, 16, 8, 16, "reflect", R.U8_PLANES, base=64)      # pitch 32, x0 = 4
    assert (wide, narrow) == (8 * 4, 0)
    got, wide, narrow = R.ingest_window_transcription(x, 0, 5, 8, 16, 8, 16, "reflect", R.U8_PLANES, base=64)      # x0 = 5: no row is aligned
    assert (wide, narrow) == (0, 8 * 16)
    y = _source(R.U8_PLANES, 1, 1, 8, 30, seed=2)      # pitch 30, x0 = 0: every other row starts on a 4-byte boundary
    got, wide, narrow = R.ingest_window_transcription(y, 0, 0, 8, 16, 8, 16, "reflect", R.U8_PLANES, base=64)
    assert (wide, narrow) == (4 * 4, 4 * 16) and np.array_equal(got, R.window_oracle(y, 0, 0, 8, 16, 8, 16, "reflect"))


@pytest.mark.parametrize("X0", [0, 2, 4, 5, 50])
def test_tile_blend_address_arithmetic_is_numpy(X0):
    """a strided (transposed, cropped) tile into 2 x 3 x 3 x 24 x 72; widths 16, 20 and 18 (a tail of 2); acc, tile and wx at every
    alignment class: 16-, 8- and 4-byte accesses all occur, and the result is the numpy statement's, bit for bit"""
    rng = np.random.default_rng(X0)
    n, F, C, SH, SW = 2, 3, 3, 24, 72
    seen = {16: 0, 8: 0, 4: 0}
    for tw, bases in ((16, (0, 0, 0, 0)), (20, (16, 8, 4, 8)), (18, (32, 4, 0, 12)), (16, (8, 16, 8, 0))):
        th, Hp, Wp = 10, 12, tw + 4                                   # the tile is the top left of padded frames of Hp x Wp, frame-major
        store = rng.standard_normal(F * n * C * Hp * Wp + 5).astype(np.float32)
        off = 5
        strides = (C * Hp * Wp, n * C * Hp * Wp, Hp * Wp, Wp)          # (F, n, C, Hp, Wp) transposed to (n, F, ...)
        view = np.lib.stride_tricks.as_strided(store[off:], (n, F, C, th, tw), tuple(4 * v for v in strides + (1,)))
        acc = rng.standard_normal((n, F, C, SH, SW)).astype(np.float32)
        wy, wx = rng.random(th, dtype=np.float32), rng.random(tw, dtype=np.float32)
        want = R.blend_oracle(acc.copy(), view, 7, X0, wy, wx)
        got, widths = R.tile_blend_transcription(acc, store, off, (n, F, C, th, tw), strides, 7, X0, wy, wx, bases=bases)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (X0, tw, bases)
        untouched = np.ones_like(acc, bool)
        untouched[..., 7:7 + th, X0:X0 + tw] = False
        assert np.array_equal(got[untouched].view(np.uint32), acc[untouched].view(np.uint32))
        for k in seen:
            seen[k] += widths[k]
    assert all(v > 0 for v in seen.values()), seen
    got, _ = R.tile_blend_transcription(acc, store, off, (n, F, C, th, tw), strides, 7, X0, wy, wx, grid_x=1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_blend_of_weighted_tiles_restores_a_frame():
    """the weights are a partition of unity: tiles cut from ONE frame blend back to it within m 2^-24 relative per axis pair"""
    rng = np.random.default_rng(3)
    h, w, s = 96, 112, 2
    frame = rng.random((1, 1, 3, s * h, s * w), dtype=np.float32)
    tiles = R.plan_tiles(h, w, 64, 16)
    cut = [frame[..., s * y0:s * y1, s * x0:s * x1] for y0, y1, x0, x1 in tiles]
    got = R.blend_tiles(cut, tiles, h, w, s, 64, 16)
    assert np.abs(got.astype(np.float64) - frame).max() <= 16 * 2.0 ** -24
    assert np.array_equal(got[..., :s * 32, :s * 48], frame[..., :s * 32, :s * 48])      # covered once: weight 1.0, acc 0 + v


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_in_the_stable_section_and_bound():
    from eavsr_amd import _native as N, build, ops
    with open(os.path.join(ROOT, "include", "eavsr_hip.h")) as f:
        header = f.read()
    stable = header[:header.index("EXPERIMENTAL -- exported by the LAB build only")]
    for name, count in (("eavsr_ingest_window", 15), ("eavsr_tile_blend_f32", 18)):
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
    assert callable(ops.ingest_window) and callable(ops.tile_blend)
    with open(os.path.join(ROOT, "eavsr_amd", "csrc", "blend.hip")) as f:
        source = f.read()
    assert "fp contract(off)" in source and "atomic" not in source.lower()


# ------------------------------------------------------------------------------------------------------------- the options
def test_tile_options(monkeypatch):
    from eavsr_amd.eavsrp_model import long_clip_options
    monkeypatch.delenv("EAVSR_TILE", raising=False)
    monkeypatch.delenv("EAVSR_TILE_OVERLAP", raising=False)
    assert S.tile_options(None) == (None, None) and S.tile_options(Namespace(tile=None, tile_overlap=None)) == (None, None)
    assert S.tile_options(Namespace(tile=512)) == ((512, 512), None)
    assert S.tile_options(Namespace(tile=(288, 512), tile_overlap=16)) == ((288, 512), 16)
    assert S.tile_options(Namespace(tile="288x512")) == ((288, 512), None) and S.tile_options(Namespace(tile="64")) == ((64, 64), None)
    assert S.DEFAULT_TILE_OVERLAP == 32
    monkeypatch.setenv("EAVSR_TILE", "288x512")
    monkeypatch.setenv("EAVSR_TILE_OVERLAP", "8")
    assert S.tile_options(None) == ((288, 512), 8) and S.tile_options(Namespace(tile=None)) == ((288, 512), 8)
    assert S.tile_options(Namespace(tile=128, tile_overlap=0)) == ((128, 128), 0)      # the options beat the environment
    monkeypatch.setenv("EAVSR_TILE", "512")
    assert S.tile_options(None)[0] == (512, 512)
    monkeypatch.setenv("EAVSR_TILE", "")
    assert S.tile_options(None)[0] is None
    for bad in ("66", "32x512", "512x", "x", "a", "512x512x512", "-64", "64.0"):
        monkeypatch.setenv("EAVSR_TILE", bad)
        with pytest.raises(ValueError, match="EAVSR_TILE"):
            S.tile_options(None)
        with pytest.raises(ValueError, match="EAVSR_TILE"):
            long_clip_options(Namespace())      # validated with the others
        assert S.tile_options(Namespace(tile=64))[0] == (64, 64)      # a bad environment is not read where opt decides
    monkeypatch.delenv("EAVSR_TILE")
    monkeypatch.setenv("EAVSR_TILE_OVERLAP", "-1")
    with pytest.raises(ValueError, match="EAVSR_TILE_OVERLAP"):
        S.tile_options(None)
    monkeypatch.delenv("EAVSR_TILE_OVERLAP")
    for bad in (66, "66", (64,), True, 64.0, (64, 32)):
        with pytest.raises(ValueError, match="opt.tile"):
            S.tile_options(Namespace(tile=bad))
        with pytest.raises(ValueError, match="opt.tile"):
            long_clip_options(Namespace(tile=bad))
    for bad in (-1, True, "8", 1.5):
        with pytest.raises(ValueError, match="opt.tile_overlap"):
            S.tile_options(Namespace(tile_overlap=bad))
    assert long_clip_options(Namespace(tile="288x512", tile_overlap=16)) == (None, False)


def test_arguments_are_refused_before_anything_runs(monkeypatch):
    """tile and overlap are checked before the device is looked at: a CPU tensor and a network without parameters reach the check"""
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    for name in ("EAVSR_TILE", "EAVSR_TILE_OVERLAP", "EAVSR_PAD_FRAMES"):
        monkeypatch.delenv(name, raising=False)
    net = EAVSRP.__new__(EAVSRP)
    x = torch.zeros(1, 2, 3, 96, 112)
    with torch.no_grad():
        for tile, overlap in ((60, 0), (66, 0), (64, 33), (64, -1), (None, 0), ((64, 32), 0)):
            with pytest.raises(ValueError, match="tile|overlap"):
                EAVSRP.forward_tiled(net, x, tile, overlap=overlap)
        with pytest.raises(ValueError, match="pad"):
            EAVSRP.forward_tiled(net, x, 64, pad="symmetric")
        with pytest.raises(ValueError, match="segments"):
            EAVSRP.forward_tiled(net, x, 64, segments=[(0, 1, 0, 1)])
        with pytest.raises(ValueError, match="window"):
            EAVSRP.forward_long(net, x.cuda() if False else x.to(torch.uint8), window=(0, 64, 60, 124))
        with pytest.raises(ValueError, match="window"):
            EAVSRP.forward_long(net, x.to(torch.uint8), window=(0, 64, 0))
    with pytest.raises(RuntimeError, match="no_grad"):
        EAVSRP.forward_tiled(net, x, 64)
    for kwargs in (dict(tile=66), dict(tile=64, tile_overlap=40), dict(tile="64x", tile_overlap=0), dict(tile=(64, 60))):
        with pytest.raises(ValueError, match="tile|overlap"):
            harness.super_resolve(None, x[0], **kwargs)
    with pytest.raises(ValueError, match="opt.tile"):
        harness.super_resolve(Namespace(opt=Namespace(tile=66)), x[0])
    u8 = torch.zeros(1, 3, 20, 20, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ingest_window(u8, 0, 0, 8, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.tile_blend(torch.zeros(1, 1, 1, 8, 8), torch.zeros(1, 1, 1, 4, 4), 0, 0, torch.ones(4), torch.ones(4))
    with pytest.raises(TypeError):
        ops.ingest_window(np.zeros((1, 3, 20, 20), np.uint8), 0, 0, 8, 8)
    with pytest.raises(TypeError):
        ops.tile_blend(np.zeros((1, 1, 1, 8, 8), np.float32), torch.zeros(1, 1, 1, 4, 4), 0, 0, torch.ones(4), torch.ones(4))


# ------------------------------------------------------------------------------------------------------------- the dispatch
def test_forward_video_chooses_one_of_the_four_paths():
    """`EAVSRP.forward_video` with the four methods replaced by recorders: no tile and no plan -> forward_long; a plan -> the segment
    path; more than one tile -> the tiled path (the plan handed on); a tile that covers the frame -> as if no tile were given"""
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP.__new__(EAVSRP)
    calls = []
    for name in ("forward_long", "forward_segments", "forward_segments_padded", "forward_tiled"):
        net.__dict__[name] = lambda *a, _n=name, **k: calls.append((_n, a, k)) or _n
    x = torch.zeros(1, 4, 3, 96, 112)
    u8_hwc = torch.zeros(1, 4, 96, 112, 3, dtype=torch.uint8)
    plan = [(0, 3, 0, 2), (1, 4, 2, 4)]
    common = dict(frame_chunk=2, cache="host", sink=None)
    handed = dict(common, cache_dtype=None)      # what each of the four is called with: `forward_video` has no 16-bit cache
    with torch.no_grad():
        for lrs in (x, u8_hwc):
            calls.clear()
            assert net.forward_video(lrs, pad="edge", **common) == "forward_long"
            assert calls == [("forward_long", (lrs,), dict(handed, pad="edge"))]
            calls.clear()
            assert net.forward_video(lrs, segments=plan, pad="edge", **common) == "forward_segments_padded"
            assert calls == [("forward_segments_padded", (lrs, plan, "edge"), handed)]
            calls.clear()      # one segment is still a plan: its frames go through the segment path
            assert net.forward_video(lrs, segments=[(0, 4, 0, 4)], **common) == "forward_segments_padded"
            assert calls == [("forward_segments_padded", (lrs, [(0, 4, 0, 4)], None), handed)]
            for tile, segments in ((64, None), ((64, 112), plan), ((96, 64), None)):      # 2 x 2, 2 x 1 and 1 x 2 tiles
                calls.clear()
                assert net.forward_video(lrs, segments=segments, tile=tile, tile_overlap=16, pad="reflect", **common) == "forward_tiled"
                assert calls == [("forward_tiled", (lrs, tile), dict(handed, overlap=16, segments=segments, pad="reflect"))]
            for tile in (128, (96, 112)):      # one tile
                calls.clear()
                assert net.forward_video(lrs, segments=plan, tile=tile, **common) == "forward_segments_padded"
                assert calls == [("forward_segments_padded", (lrs, plan, None), handed)]
                calls.clear()
                assert net.forward_video(lrs, tile=tile, **common) == "forward_long"
                assert calls == [("forward_long", (lrs,), dict(handed, pad=None))]
        calls.clear()
        for tile, overlap in ((66, 0), (64, 33), ((64, 32), 0)):      # refused here, before any of the four is called
            with pytest.raises(ValueError, match="tile|overlap"):
                net.forward_video(x, tile=tile, tile_overlap=overlap)
        assert calls == []
    sig = inspect.signature(EAVSRP.forward_video)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[2:]] == [
        ("segments", None), ("tile", None), ("tile_overlap", 32), ("pad", None), ("frame_chunk", None), ("cache", "device"), ("sink", None)]
