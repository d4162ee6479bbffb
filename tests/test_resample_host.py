"""The LR synthesis (dataset.cubic_tables, FramePairs.from_wide, ops.resize_cubic_u8, csrc/resize_cubic.hip), what needs no GPU: known
answers of the oracle (tests/resample_ref.py, OpenCV's CV_8U INTER_CUBIC restated), the product's tables against the oracle's, and the
argument checks, which run before anything is moved to a device."""
import re

import numpy as np
import pytest
import torch

from tests import resample_ref as R

HALF = (-192, 1216, 1216, -192)


def _bytes(shape, seed=0):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the oracle's known answers
def test_oracle_same_size_is_the_identity():
    x = _bytes((2, 13, 22))
    out, _ = R.resize_cubic_u8(x, (13, 22))
    assert np.array_equal(out, x)
    assert all(c == (0, 2048, 0, 0) for c in R.axis_tables(22, 22)[1])


def test_oracle_a_third_is_plain_decimation():
    x = _bytes((3, 21, 33), 1)
    out, _ = R.resize_cubic_u8(x, (7, 11))
    assert np.array_equal(out, x[:, 1::3, 1::3])


@pytest.mark.parametrize("name, block, want", [
    # sum w_i w_j p with w = (-3, 19, 19, -3): the 4 centre samples weigh 361, the 8 edge ones -57, the 4 corners 9
    ("undershoots to 0", [[255, 255, 255, 255], [255, 0, 0, 255], [255, 0, 0, 255], [255, 255, 255, 255]], 0),     # -107100
    ("overshoots to 255", [[0, 0, 0, 0], [0, 255, 255, 0], [0, 255, 255, 0], [0, 0, 0, 0]], 255),                    # 368220
    ("an exact tie rounds up", [[6, 12, 0, 0], [0, 6, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]], 2),                      # 1536 = 1.5 * 1024
])
def test_oracle_one_4x4_block(name, block, want):
    p = np.asarray(block, np.uint8)
    w = np.asarray([-3, 19, 19, -3], np.int64)
    acc = int((w[:, None] * w[None, :] * p.astype(np.int64)).sum())
    by_hand = min(max((acc + 512) >> 10, 0), 255)
    assert by_hand == want, (name, acc)
    out, v = R.resize_cubic_u8(p, (1, 1))
    assert int(out[0, 0]) == want and int(v[0, 0]) == acc * 4096      # (64 w_i)(64 w_j) = 4096 w_i w_j
    if "tie" in name:
        assert (acc + 512) % 1024 == 0 and R.counts(v)[0] == 1


@pytest.mark.parametrize("src, dst, first", [(64, 16, 1), (64, 32, 0)])
def test_oracle_half_sample_coefficients(src, dst, first):
    ofs, coef = R.axis_tables(src, dst)
    step = src // dst
    assert ofs == [first + step * d for d in range(dst)] and all(c == HALF for c in coef)


def test_oracle_coefficient_sums_are_not_corrected():
    sums = lambda s, d: {sum(c) for c in R.axis_tables(s, d)[1]}
    assert 2047 in sums(70, 17)
    assert sums(37, 9) - {2048} and sums(100, 33) - {2048}


def test_oracle_border_clamp_of_a_2x2_input():
    """2 -> 1: s = 0, x = 0.5, taps -1, 0, 1, 2 clamp to 0, 0, 1, 1: weights (1024, 1024) per axis, the mean rounded half up"""
    assert R.axis_tables(2, 1) == ([0], [HALF])
    for p in ([[10, 20], [30, 41]], [[0, 0], [0, 255]], [[255, 254], [255, 255]], [[1, 0], [0, 1]]):
        p = np.asarray(p, np.uint8)
        out, v = R.resize_cubic_u8(p, (1, 1))
        assert int(v[0, 0]) == 1024 * 1024 * int(p.sum()) and int(out[0, 0]) == (int(p.sum()) + 2) >> 2


# ------------------------------------------------------------------------------------------------ the product's tables
def test_cubic_tables_equal_the_oracles():
    from eavsr_amd.dataset import cubic_tables
    for src in range(8, 97):
        for dst in range(-(-src // 8), src + 1):
            ofs, coef = cubic_tables(src, dst)
            want_ofs, want_coef = R.axis_tables(src, dst)
            assert ofs.dtype == np.int32 and coef.dtype == np.int16 and ofs.shape == (dst,) and coef.shape == (dst, 4)
            assert ofs.tolist() == want_ofs and [tuple(c) for c in coef.tolist()] == want_coef, (src, dst)


def test_cubic_tables_fit_the_rectangle_the_kernel_stages():
    """csrc/resize_cubic.hip bounds the source samples of a tile of T outputs by min(src, floor(src (T - 1) / dst) + 7) from the sizes
    alone (the tables are device memory there); with these tables the bound must never bind.  T = 64 columns, 16 rows."""
    from eavsr_amd.dataset import cubic_tables
    pairs = [(s, d) for s in range(8, 97) for d in range(-(-s // 8), s + 1)] + [(1280, 320), (720, 180), (517, 129), (1000, 125), (4099, 513),
                                                                              (2047, 1023), (1999, 250)]
    for src, dst in pairs:
        ofs = cubic_tables(src, dst)[0].astype(np.int64)
        for T in (16, 64):
            d0 = np.arange(0, dst, T)
            d1 = np.minimum(d0 + T, dst) - 1
            span = np.minimum(ofs[d1] + 2, src - 1) - np.maximum(ofs[d0] - 1, 0) + 1
            assert span.max() <= min(src, (src * (T - 1)) // dst + 7), (src, dst, T)


def test_cubic_tables_are_cached_read_only_and_refuse_other_ratios():
    from eavsr_amd.dataset import cubic_tables
    a, b = cubic_tables(70, 17), cubic_tables(70, 17)
    assert a[0] is b[0] and a[1] is b[1] and not a[0].flags.writeable and not a[1].flags.writeable
    for src, dst in ((16, 0), (16, -1), (16, 17), (17, 2), (9, 1), (0, 1)):
        with pytest.raises(ValueError, match="at least one output|ratio"):
            cubic_tables(src, dst)
    assert cubic_tables(8, 1)[0].tolist() == [3] and cubic_tables(16, 16)[0].shape == (16,)


# ------------------------------------------------------------------------------------------------ argument checks, no device
def test_from_wide_checks_its_arguments_before_anything_is_moved():
    from eavsr_amd.dataset import FramePairs
    wide, hr = _bytes((8, 3, 16, 24)), _bytes((8, 3, 16, 24), 1)
    dev = "cuda:0"      # never reached: every call below fails in the shape checks
    with pytest.raises(ValueError, match="same size"):
        FramePairs.from_wide(wide, hr[:, :, :12], 4, 4, device=dev)
    with pytest.raises(ValueError, match="same size"):
        FramePairs.from_wide(wide, hr[:4], 4, 4, device=dev)
    with pytest.raises(ValueError, match="same size"):
        FramePairs.from_wide(np.ascontiguousarray(wide.transpose(0, 2, 3, 1)), hr[:, :1], 4, 4, device=dev)
    with pytest.raises(ValueError, match=r"H % scale == 0 and W % scale == 0"):
        FramePairs.from_wide(_bytes((8, 3, 18, 24)), None, 4, 4, device=dev)
    with pytest.raises(ValueError, match=r"H % scale == 0 and W % scale == 0"):
        FramePairs.from_wide(wide, hr, 5, 4, device=dev)
    with pytest.raises(ValueError, match="whole scenes"):
        FramePairs.from_wide(wide, hr, 4, 3, device=dev)
    with pytest.raises(ValueError, match="names"):
        FramePairs.from_wide(wide, hr, 4, 4, names=["a"], device=dev)
    with pytest.raises(ValueError, match="scale"):
        FramePairs.from_wide(wide, hr, 16, 4, device=dev)
    with pytest.raises(ValueError, match="chunk"):
        FramePairs.from_wide(wide, hr, 4, 4, device=dev, chunk=0)
    with pytest.raises(ValueError, match="uint8"):
        FramePairs.from_wide(wide.astype(np.float32), hr, 4, 4, device=dev)
    with pytest.raises(ValueError, match="2 wide and 1 HR"):
        FramePairs.from_wide_files(["a", "b"], ["c"], 4, 2, device=dev)


def test_resize_cubic_u8_refuses_cpu_tensors_without_touching_a_device():
    from eavsr_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_cubic_u8(torch.zeros(1, 3, 16, 16, dtype=torch.uint8), (4, 4))
    with pytest.raises(TypeError):
        ops.resize_cubic_u8([1, 2], (4, 4))


def test_resize_cubic_u8_is_in_the_stable_header_and_checks_its_arguments_on_the_host():
    import os
    from eavsr_amd import _native
    lib = _native.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eavsr_hip.h")).read()
    stable = header.split(" * EXPERIMENTAL -- exported by the LAB build only")[0]
    assert "eavsr_resize_cubic_u8" in _native.SIGNATURES and re.search(r"^int eavsr_resize_cubic_u8\(", stable, flags=re.M)
    g = lib.eavsr_resize_cubic_u8
    p = 64      # an aligned, never dereferenced address: every call below fails (or returns) before a launch
    assert g(None, p, p, p, p, p, 1, 3, 16, 16, 4, 4, None) == -1 and b"NULL" in lib.eavsr_last_error()
    assert g(p, p, p, p, p, None, 1, 3, 16, 16, 4, 4, None) == -1
    assert g(p, p, p, p, p, p, 1, 0, 16, 16, 4, 4, None) == -2
    assert g(p, p, p, p, p, p, 1, 3, 16, 36, 4, 4, None) == -2 and b"ratio" in lib.eavsr_last_error()      # 36 / 4 = 9
    assert g(p, p, p, p, p, p, 1, 3, 16, 16, 17, 4, None) == -2 and b"ratio" in lib.eavsr_last_error()     # upscaling
    assert g(p, p, p, p, p, p, 1, 1, 65536, 32768, 8192, 4096, None) == -2 and b"2^31 - 1" in lib.eavsr_last_error()
    assert g(p, p, p + 2, p, p, p, 1, 3, 16, 16, 4, 4, None) == -2 and b"aligned" in lib.eavsr_last_error()
    assert g(p, p, p, p + 4, p, p, 1, 3, 16, 16, 4, 4, None) == -2 and b"aligned" in lib.eavsr_last_error()
    # planes and tiles share grid x: 2^24 - 1 workgroups per launch.  64 x 64 outputs are 4 tiles: 4194303 planes pass the check
    # (F = 0 stops before the launch, so the passing side is shown by the count alone), 4194304 do not
    assert g(p, p, p, p, p, p, 1398102, 3, 256, 256, 64, 64, None) == -2
    msg = lib.eavsr_last_error()
    assert b"4194306 planes" in msg and b"16777215" in msg and b"grid x" in msg
    assert g(p, p, p, p, p, p, 0, 3, 256, 256, 64, 64, None) == 0
