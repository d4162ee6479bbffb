"""Output at any target size, on the host: the tables of `eavsr_amd.resize`, the numpy restatement the GPU tests compare
with (tests/resize_ref.py), the option's spellings and the kernels' address arithmetic transcribed to Python."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest

from eavsr_amd import niqe, resize
from tests import resize_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("length", [1, 2, 7, 64])
def test_the_same_length_is_one_tap_of_weight_one(length):
    idx, w = resize.axis_tables(length, length)
    assert idx.dtype == np.int32 and w.dtype == np.float32 and idx.shape == w.shape == (length, 1)
    assert (idx[:, 0] == np.arange(length)).all() and (w == 1.0).all()


@pytest.mark.parametrize("length", [10, 48, 96])
def test_half_the_length_is_niqe_resize_tables(length):
    idx, w = resize.axis_tables64(length, length // 2)
    ridx, rw = niqe.resize_tables(length, 0.5)
    assert idx.shape == ridx.shape and (idx == ridx).all()
    assert w.dtype == np.float64 and (w == rw).all()
    i32, w32 = resize.axis_tables(length, length // 2)
    assert (i32 == idx).all() and w32.dtype == np.float32 and (w32 == w.astype(np.float32)).all()


SIZES = [(16, 40), (264, 200), (97, 40), (2051, 700), (1000, 63), (64, 96), (131, 53), (33, 264), (65, 17), (1, 5), (2, 7), (5, 3)]


def test_tap_counts():
    taps = lambda a, b: resize.axis_tables(a, b)[0].shape[1]
    assert taps(16, 40) == 4 and taps(64, 96) == 4 and taps(33, 264) == 4
    assert taps(264, 200) == 6 and taps(97, 40) == 10 and taps(2051, 700) == 12 and taps(1000, 63) == 64
    idx, w = resize.axis_tables(264, 200)
    assert int((w == 0).sum()) == 147      # single zeros inside kept columns: the op skips them


@pytest.mark.parametrize("length,out", SIZES)
def test_rows_of_float32_weights_sum_to_one(length, out):
    _, w = resize.axis_tables(length, out)
    err = np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f"{length} -> {out}: max |row sum - 1| {err:.3e}")
    assert err <= 1e-7


def _dense(length, out):
    idx, w = resize.axis_tables(length, out)
    a = np.zeros((out, length), np.float64)
    for k in range(idx.shape[1]):
        np.add.at(a, (np.arange(out), idx[:, k]), w[:, k].astype(np.float64))
    return a


@pytest.mark.parametrize("length,out", SIZES)
def test_the_tables_of_a_flipped_axis_are_the_flipped_tables(length, out):
    """as operators: columns that are dropped may differ between the two ends, and a weight and its mirror image are computed
    from arguments that differ in the last bit, so the dense (out, length) matrices are compared, within one float32 rounding"""
    a = _dense(length, out)
    assert np.abs(a - a[::-1, ::-1]).max() <= 1e-7


@pytest.mark.parametrize("length,out", [(1, 5), (2, 7), (5, 3), (3, 200), (1000, 63)])
def test_indices_stay_in_range_where_reflection_wraps(length, out):
    idx, w = resize.axis_tables(length, out)
    assert idx.min() >= 0 and idx.max() <= length - 1 and np.isfinite(w).all()


def test_sixty_four_taps_are_accepted_and_sixty_five_refused():
    assert resize.axis_tables(1000, 63)[0].shape == (63, 64)
    with pytest.raises(ValueError, match="65 taps"):
        resize.axis_tables(1000, 62)
    for bad in ((0, 4), (4, 0), (4.0, 2), (True, 2)):
        with pytest.raises(ValueError):
            resize.axis_tables(*bad)


# ---------------------------------------------------------------------------------------------------------------------- reference
def test_float32_reference_against_float64():
    rng = np.random.default_rng(3)
    for shape, size in (((64, 64), (96, 160)), ((97, 131), (40, 53)), ((33, 65), (264, 17)), ((5, 7), (3, 2))):
        x = rng.random(shape, dtype=np.float32)
        e = np.abs(RR.resize(x, size).astype(np.float64) - RR.resize(x, size, np.float64)).max()
        print(f"{shape} -> {size}: max |f32 - f64| {e:.3e}")
        assert e <= 1e-5


def test_a_ramp_is_reproduced_at_the_mapped_coordinates():
    """cubic convolution reproduces degree 1: ramp[j] = j / 16 (exact in fp32), upscaled 16 -> 40; output x = 1 .. 40 sits at the
    1-based coordinate u = x / s + (1 - 1 / s) / 2, so its value is (u - 1) / 16 wherever no tap is reflected"""
    ramp = np.tile(np.arange(16, dtype=np.float32) / 16.0, (6, 1))
    got = RR.resize(ramp, (6, 40))
    s = 40.0 / 16.0
    u = np.arange(1, 41) / s + 0.5 * (1.0 - 1.0 / s)
    inside = (np.floor(u - 2.0) + 1 >= 1) & (np.floor(u - 2.0) + 4 <= 16)      # the four taps with a weight: all inside 1 .. 16
    assert inside.sum() >= 30
    e = np.abs(got[:, inside].astype(np.float64) - ((u - 1.0) / 16.0)[inside][None, :]).max()
    print(f"ramp 16 -> 40: max error in the interior {e:.3e}")
    assert e <= 1e-6


def test_one_inf_reaches_exactly_the_outputs_whose_taps_read_it():
    x = np.random.default_rng(5).random((8, 9), dtype=np.float32)
    x[3, 4] = np.inf
    got = RR.resize(x, (5, 13))
    want = RR.touched((8, 9), (5, 13), 3, 4)
    assert 0 < want.sum() < want.size
    assert (~np.isfinite(got) == want).all()


# ------------------------------------------------------------------------------------------------------------ options and symbols
def test_every_spelling_of_the_option(monkeypatch):
    monkeypatch.delenv("EAVSR_OUT_SIZE", raising=False)
    assert resize.out_size_option(None) is None and resize.out_size_option(Namespace()) is None
    assert resize.out_size_option(Namespace(out_size=(1080, 1920))) == (1080, 1920)
    assert resize.out_size_option(Namespace(out_size=[200, 300])) == (200, 300)
    assert resize.out_size_option(Namespace(out_size="1080x1920")) == (1080, 1920)
    monkeypatch.setenv("EAVSR_OUT_SIZE", "720x1280")
    assert resize.out_size_option(None) == (720, 1280)
    assert resize.out_size_option(Namespace(out_size=(5, 7))) == (5, 7)      # the options decide
    monkeypatch.setenv("EAVSR_OUT_SIZE", "")
    assert resize.out_size_option(None) is None
    for bad in ("1080", "axb", "10x", "10x20x30", "-4x8", "0x8", (0, 5), (5,), (1, 2, 3), (1.5, 2), (True, 2), 7, ((1 << 24) + 1, 4)):
        with pytest.raises(ValueError, match=r"^opt\.out_size="):
            resize.out_size_option(Namespace(out_size=bad))
    monkeypatch.setenv("EAVSR_OUT_SIZE", "1080*1920")
    with pytest.raises(ValueError, match=r"^EAVSR_OUT_SIZE="):
        resize.out_size_option(None)
    # the options decide: a bad environment is not read beside them
    assert resize.out_size_option(Namespace(out_size="8x9")) == (8, 9)


def test_out_size_is_refused_in_training_and_bad_values_before_anything_runs(monkeypatch):
    from eavsr_amd.eavsrp_model import EAVSRPModel, long_clip_options
    monkeypatch.delenv("EAVSR_OUT_SIZE", raising=False)
    with pytest.raises(ValueError, match=r"opt\.out_size"):
        EAVSRPModel(Namespace(scale=4, isTrain=True, out_size=(200, 300), gpu_ids=[0]))
    with pytest.raises(ValueError, match=r"^opt\.out_size="):
        long_clip_options(Namespace(out_size="200"))
    from eavsr_amd import harness
    with pytest.raises(ValueError, match=r"super_resolve: out_size="):      # before the network is looked at, or a file read
        harness.super_resolve(object(), ["no_such_file.png"], out_size="200")


def test_the_library_exports_the_entry_point():
    from eavsr_amd import _native, build
    build.build_native()
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "eavsr_resize_aa_f32" in set(re.findall(r" T (eavsr_[a-z0-9_]+)$", nm, flags=re.M))
    assert "eavsr_resize_aa_f32" in _native.SIGNATURES and len(_native.SIGNATURES["eavsr_resize_aa_f32"][1]) == 19
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header.split(" * EXPERIMENTAL -- exported by the LAB build only")[0]
    assert re.search(r"^int\s+eavsr_resize_aa_f32\s*\(", stable, flags=re.M)
    assert build.PER_FILE_FLAGS["resize_aa.hip"] == ["-ffp-contract=off"]


# -------------------------------------------------------------------------------------------------------------- address arithmetic
def _case(shape, size, base, crop=(0, 0, 0, 0), seed=0):
    """a source of `shape` (N, C, H, W) that is the crop [top:H0 - bottom, left:W0 - right] of contiguous planes starting at
    element `base` of a flat array -> (mem, first element, strides, the source as numpy sees it)"""
    n, c, h, w = shape
    top, bottom, left, right = crop
    H0, W0 = h + top + bottom, w + left + right
    mem = np.full(base + n * c * H0 * W0 + 8, np.nan, np.float32)
    full = np.random.default_rng(seed).random((n, c, H0, W0), dtype=np.float32)
    mem[base:base + full.size] = full.reshape(-1)
    view = full[:, :, top:top + h, left:left + w]
    return mem, base + top * W0 + left, (c * H0 * W0, H0 * W0, W0), view


ADDRESS_CASES = [((1, 1, 1, 1), (5, 7), 0, (0, 0, 0, 0)), ((1, 3, 2, 3), (7, 5), 0, (0, 0, 0, 0)), ((2, 3, 5, 7), (3, 2), 0, (0, 0, 0, 0)),
                 ((1, 2, 12, 16), (9, 21), 0, (0, 0, 0, 0)), ((1, 2, 12, 16), (9, 21), 1, (0, 0, 0, 0)), ((1, 1, 9, 13), (6, 20), 2, (0, 0, 0, 0)),
                 ((1, 1, 9, 13), (6, 20), 3, (0, 0, 0, 0)), ((1, 2, 11, 14), (7, 30), 0, (1, 2, 3, 1)), ((1, 1, 6, 37), (4, 11), 0, (1, 2, 3, 1))]


@pytest.mark.parametrize("shape,size,base,crop", ADDRESS_CASES)
def test_both_passes_address_arithmetic_is_numpy_slicing(shape, size, base, crop):
    mem, first, strides, view = _case(shape, size, base, crop)
    got, stats = RR.transcription(mem, first, strides, shape, size)
    want = RR.resize(view, size)
    assert got.shape == want.shape and (got.view(np.int32) == want.view(np.int32)).all()
    print(shape, size, base, crop, stats)


def test_the_vertical_pass_takes_the_wide_loads_where_the_address_allows():
    # contiguous planes of 16 columns on a boundary: every quad of every row is one float4 load
    mem, first, strides, _ = _case((1, 2, 12, 16), (9, 21), 0)
    assert RR.transcription(mem, first, strides, (1, 2, 12, 16), (9, 21))[1]["scalar"] == 0
    # one element past the boundary, row stride still a multiple of 4: a head of 3, a tail of 1, float4 between them
    mem, first, strides, _ = _case((1, 2, 12, 16), (9, 21), 1)
    stats = RR.transcription(mem, first, strides, (1, 2, 12, 16), (9, 21))[1]
    assert stats["vec"] > 0 and stats["scalar"] > 0 and stats["vec"] * 4 == 3 * stats["scalar"]
    # an odd row stride: only the rows whose offset keeps the plane's phase are read wide
    mem, first, strides, _ = _case((1, 1, 9, 13), (6, 20), 0)
    stats = RR.transcription(mem, first, strides, (1, 1, 9, 13), (6, 20))[1]
    assert stats["vec"] > 0 and stats["scalar"] > 3 * stats["vec"]


def test_a_long_row_goes_through_the_horizontal_pass_in_pieces():
    c = RR.kernel_constants()
    W = c["kLdsRow"] + 3
    shape, size = (1, 1, 2, W), (2, 700)
    mem, first, strides, view = _case(shape, size, 0)
    got, stats = RR.transcription(mem, first, strides, shape, size)
    assert stats["pieces"] == -(-700 // RR.piece_columns(W, 700, 12)) >= 3 and stats["span"] <= c["kLdsRow"]
    assert (got.view(np.int32) == RR.resize(view, size).view(np.int32)).all()


def test_the_span_of_a_piece_fits_the_staged_row_at_every_ratio():
    """the entry point sizes a piece from W / ow alone; the span its columns really read (from the tables) must fit kLdsRow"""
    c = RR.kernel_constants()
    for W, ow in [(1000, 63), (1000, 64), (4096, 265), (3840, 1920), (2051, 700), (8192, 529), (720, 1920), (97, 40), (5000, 4999), (3, 200)]:
        idx, _ = resize.axis_tables(W, ow)
        cols = RR.piece_columns(W, ow, idx.shape[1], c)
        assert 1 <= cols and cols * idx.shape[1] <= c["kLdsTable"]
        spans = [int(idx[a:a + cols].max() - idx[a:a + cols].min() + 1) for a in range(0, ow, cols)]
        print(f"{W} -> {ow}: {idx.shape[1]} taps, pieces of {cols} columns, widest span {max(spans)}")
        assert max(spans) <= c["kLdsRow"]
    lds = (2 * c["kLdsTable"] + c["kThreads"] // 64 * c["kLdsRow"] + 8) * 4
    assert lds <= 64 * 1024 and 2 * lds <= 160 * 1024      # beside a second workgroup on a CU, without raising the dynamic limit
