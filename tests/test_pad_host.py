"""Frames of any size, what needs no GPU: the padded size, the index functions of `ops.ingest_pad` against np.pad, the
option, the argument checks that come before any device work, the C ABI's entry point, and a transcription of the kernels'
address arithmetic (tests/pad_ref.py) against np.pad."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest
import torch

from eavsr_amd import segments as S
from tests import pad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------- padded size
@pytest.mark.parametrize("size, want", [((270, 480), (272, 480)), ((66, 70), (68, 72)), ((40, 50), (64, 64)), ((64, 64), (64, 64)),
                                        ((1, 1), (64, 64)), ((480, 854), (480, 856)), ((486, 720), (488, 720)), ((63, 65), (64, 68))])
def test_padded_size(size, want):
    assert S.padded_size(*size) == want
    H, W = S.padded_size(*size)
    assert H >= max(size[0], 64) and W >= max(size[1], 64) and H % 4 == 0 and W % 4 == 0
    assert S.padded_size(H, W) == (H, W)
    with pytest.raises(ValueError):
        S.padded_size(0, 64)


# ------------------------------------------------------------------------------------------------------------- index functions
@pytest.mark.parametrize("mode", ["reflect", "edge"])
def test_index_functions_are_np_pad_for_every_pad_width(mode):
    """s = 1 .. 40, pads 0 .. 70 (up to 70 times the axis): `segments.pad_index`, and the transcription of the kernel's `src_index`"""
    for s in range(1, 41):
        axis = np.arange(s)
        want = np.pad(axis, (0, 70), mode=mode)
        got = [S.pad_index(i, s, mode) for i in range(s + 70)]
        assert got == want.tolist(), (s, mode)
        assert [R.src_index(i, s, mode == "edge") for i in range(s + 70)] == want.tolist(), (s, mode)
        for pad in range(0, 71):      # every shorter pad is a prefix
            assert np.array_equal(np.pad(axis, (0, pad), mode=mode), want[:s + pad])


def test_index_function_refuses_what_it_cannot_index():
    for bad in ((-1, 4, "reflect"), (0, 0, "reflect"), (3, 4, "symmetric")):
        with pytest.raises(ValueError):
            S.pad_index(*bad)
    assert S.pad_index(2 ** 31 - 2, 2 ** 31 - 1, "reflect") == 2 ** 31 - 2
    assert R.src_index(2 ** 32 - 1, 2 ** 31 - 1, False) == S.pad_index(2 ** 32 - 1, 2 ** 31 - 1, "reflect")      # 2 (s - 1) < 2^32


# ------------------------------------------------------------------------------------------------------------- the option
def test_pad_option(monkeypatch):
    from eavsr_amd.eavsrp_model import long_clip_options
    monkeypatch.delenv("EAVSR_PAD_FRAMES", raising=False)
    assert S.pad_option(None) is None and S.pad_option(Namespace()) is None and S.pad_option(Namespace(pad_frames=None)) is None
    assert S.pad_option(Namespace(pad_frames="edge")) == "edge"
    monkeypatch.setenv("EAVSR_PAD_FRAMES", "reflect")
    assert S.pad_option(None) == "reflect" and S.pad_option(Namespace(pad_frames=None)) == "reflect"
    assert S.pad_option(Namespace(pad_frames="edge")) == "edge"      # the options beat the environment
    monkeypatch.setenv("EAVSR_PAD_FRAMES", "")
    assert S.pad_option(None) is None
    monkeypatch.setenv("EAVSR_PAD_FRAMES", "symmetric")
    with pytest.raises(ValueError, match="EAVSR_PAD_FRAMES"):
        S.pad_option(None)
    with pytest.raises(ValueError, match="EAVSR_PAD_FRAMES"):
        long_clip_options(Namespace())      # validated with the others
    assert S.pad_option(Namespace(pad_frames="reflect")) == "reflect"      # ... and a bad environment is not read where opt decides
    monkeypatch.delenv("EAVSR_PAD_FRAMES")
    for bad in ("symmetric", True, 1, ""):
        with pytest.raises(ValueError, match="opt.pad_frames"):
            S.pad_option(Namespace(pad_frames=bad))
        with pytest.raises(ValueError, match="opt.pad_frames"):
            long_clip_options(Namespace(pad_frames=bad))
    assert long_clip_options(Namespace(pad_frames="reflect")) == (None, False)


def test_arguments_are_refused_before_anything_runs(monkeypatch):
    """`pad` is checked before the device is looked at: a CPU tensor reaches the check"""
    from eavsr_amd import harness, ops
    from eavsr_amd.eavsrp_model import EAVSRP
    monkeypatch.delenv("EAVSR_PAD_FRAMES", raising=False)
    net = EAVSRP.__new__(EAVSRP)      # no parameters are needed to reach the check
    x = torch.zeros(1, 2, 3, 66, 70)
    with torch.no_grad():
        with pytest.raises(ValueError, match="pad"):
            EAVSRP.forward_long(net, x, pad="symmetric")
        with pytest.raises(ValueError, match="pad"):
            EAVSRP.forward_segments_padded(net, x, [(0, 2, 0, 2)], "zeros")
    with pytest.raises(ValueError, match="pad"):
        harness.super_resolve(None, x[0], pad="symmetric")
    with pytest.raises(ValueError, match="opt.pad_frames"):
        harness.super_resolve(Namespace(opt=Namespace(pad_frames="wrap")), x[0])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ingest_pad(torch.zeros(1, 3, 5, 7, dtype=torch.uint8), 8, 8)
    with pytest.raises(TypeError):
        ops.ingest_pad(np.zeros((1, 3, 5, 7), np.uint8), 8, 8)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_point_is_declared_in_the_stable_section_and_bound():
    from eavsr_amd import _native as N
    with open(os.path.join(ROOT, "include", "eavsr_hip.h")) as f:
        header = f.read()
    stable = header[:header.index("EXPERIMENTAL -- exported by the LAB build only")]
    m = re.search(r"int eavsr_ingest_pad\(([^;]*)\);", stable)
    assert m, "eavsr_ingest_pad is not declared in the stable section"
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    res, argtypes = N.SIGNATURES["eavsr_ingest_pad"]
    assert len(args) == len(argtypes) == 11
    for a, t in zip(args, argtypes):
        assert (t is N.vp) == ("*" in a), (a, t)
        assert (t is N.i32) == a.startswith("int32_t"), (a, t)
    assert os.path.exists(os.path.join(ROOT, "eavsr_amd", "csrc", "ingest_pad.hip"))
    from eavsr_amd import build
    assert any(p.endswith("ingest_pad.hip") for p in build.sources())


# ------------------------------------------------------------------------------------------------------------- the kernel, restated
def _source(kind, F, C, h, w, seed):
    rng = np.random.default_rng(seed)
    if kind == R.U8_INTERLEAVED:
        return rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if kind == R.U8_PLANES:
        return rng.integers(0, 256, (F, C, h, w), dtype=np.uint8)
    x = rng.standard_normal((F, C, h, w)).astype(np.float32)
    x.reshape(-1)[:3].view(np.uint32)[:] = (0x7FC01234, 0xFF800000, 0x80000000)      # a NaN with a payload, -inf, -0: bits are kept
    return x


SHAPES = [(5, 7, 8, 8), (2, 2, 64, 64), (1, 3, 4, 4), (33, 35, 64, 64), (66, 70, 68, 72), (16, 16, 16, 16), (7, 9, 7, 10), (3, 5, 9, 270)]


@pytest.mark.parametrize("mode", ["reflect", "edge"])
@pytest.mark.parametrize("kind", [R.U8_PLANES, R.U8_INTERLEAVED, R.F32_PLANES])
def test_kernel_address_arithmetic_is_np_pad(kind, mode):
    """every shape of the GPU test (64 x 64 stands at 16 x 16: same paths) and one whose rows are longer than a wave's 256 samples,
    F = 2, at the byte offsets 0 .. 3 of a byte source (fp32: 0, 4, 8, 12, the offsets inside a 16-byte line)"""
    for si, (h, w, H, W) in enumerate(SHAPES):
        C = 3 if kind == R.U8_INTERLEAVED or si % 2 else 1
        x = _source(kind, 2, C, h, w, seed=si)
        want = R.pad_oracle(x, H, W, mode, hwc=kind == R.U8_INTERLEAVED)
        for off in range(4):
            base = 64 + (4 * off if kind == R.F32_PLANES else off)
            got, wide, narrow = R.kernel_transcription(x, H, W, mode, kind, base=base)
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (kind, mode, (h, w, H, W), off)


def test_transcription_takes_the_wide_loads_where_the_kernel_is_meant_to():
    """an aligned planar byte source without padding: wide loads only; 1 .. 3 bytes past a 4-byte boundary with w % 4 == 0: none; a
    capped grid (more rows than the grid covers at once) changes nothing"""
    x = _source(R.U8_PLANES, 1, 1, 8, 16, seed=1)
    want = R.pad_oracle(x, 8, 16, "reflect")
    got, wide, narrow = R.kernel_transcription(x, 8, 16, "reflect", R.U8_PLANES, base=64)
    assert (wide, narrow) == (8 * 4, 0) and np.array_equal(got, want)
    for off in (1, 2, 3):
        got, wide, narrow = R.kernel_transcription(x, 8, 16, "reflect", R.U8_PLANES, base=64 + off)
        assert (wide, narrow) == (0, 8 * 16) and np.array_equal(got, want)
    got, wide, narrow = R.kernel_transcription(x, 12, 20, "reflect", R.U8_PLANES, base=64)      # 4 straight quads + 1 reflected per row
    assert (wide, narrow) == (12 * 4, 12 * 4) and np.array_equal(got, R.pad_oracle(x, 12, 20, "reflect"))
    y = _source(R.U8_INTERLEAVED, 2, 3, 9, 6, seed=2)
    for gx in (1, 2):
        got, _, _ = R.kernel_transcription(y, 21, 8, "edge", R.U8_INTERLEAVED, base=3, grid_x=gx)
        assert np.array_equal(got, R.pad_oracle(y, 21, 8, "edge", hwc=True))
    assert R.row_blocks(540, 45) == 45 and R.row_blocks(64, 3) == 16 and R.row_blocks(7, 4096) == 1
