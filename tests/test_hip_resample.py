"""The LR synthesis on the GPU (`pytest -m gpu`): ops.resize_cubic_u8 (csrc/resize_cubic.hip) and FramePairs.from_wide / from_wide_files.

The expected value everywhere is tests/resample_ref.py, OpenCV's CV_8U INTER_CUBIC resize restated in integers with its own tables.
Every comparison is torch.equal: bytes in, integer arithmetic, bytes out -- there is no tolerance to choose.  The kernel's tile is
16 output rows x 64 output columns; it stores 4 bytes at once when the output width is a multiple of 4 and bytes otherwise."""
import os

import numpy as np
import pytest
import torch

from tests import large_extents as L
from tests import resample_ref as R

pytestmark = pytest.mark.gpu


def _bytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(got, want, what=""):
    assert tuple(got.shape) == want.shape and got.dtype == torch.uint8, (tuple(got.shape), want.shape, got.dtype)
    got, want = got.cpu(), torch.from_numpy(want)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{what}: {bad.shape[0]} of {want.numel()} samples differ, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].item()} vs {want[tuple(bad[0])].item()}")


def _check(cuda, x, size, what=""):
    from eavsr_amd import ops
    want, v = R.resize_cubic_u8(x, size)
    _same(ops.resize_cubic_u8(_dev(x, cuda), size), want, what)
    return want, v


@pytest.fixture(scope="module")
def x4_case():
    """2 x 3 x 256 x 320 random bytes whose x4 result holds ties and both saturations (the oracle says so), and that result"""
    for seed in range(64):
        x = _bytes((2, 3, 256, 320), seed)
        want, v = R.resize_cubic_u8(x, (64, 80))
        ties, low, high = R.counts(v)
        if ties >= 8 and low >= 100 and high >= 100:
            print(f"x4 case: seed {seed}: {ties} ties, {low} samples clamped to 0, {high} to 255 of {want.size}")
            return x, want
    raise AssertionError("no seed below 64 gives 8 ties and 100 saturated samples on each side")


@pytest.fixture(scope="module")
def x2_case():
    x = _bytes((2, 1, 38, 70), 2)
    return x, R.resize_cubic_u8(x, (19, 35))[0]


# ------------------------------------------------------------------------------------------------------------- the kernel
def test_exact_x4_with_ties_and_both_saturations(cuda, x4_case):
    from eavsr_amd import ops
    x, want = x4_case
    _same(ops.resize_cubic_u8(_dev(x, cuda), (64, 80)), want, "x4")


def test_exact_x2_odd_output_sizes_one_channel(cuda, x2_case):
    """w = 35: the byte-store tail; W = 70: rows start at phases 0 and 2"""
    from eavsr_amd import ops
    x, want = x2_case
    _same(ops.resize_cubic_u8(_dev(x, cuda), (19, 35)), want, "x2")


@pytest.mark.parametrize("shape, size", [((1, 1, 37, 53), (9, 13)), ((1, 1, 100, 70), (33, 17)), ((1, 3, 203, 517), (50, 129)),
                                         ((2, 2, 131, 473), (41, 150))],
                         ids=["37x53", "100x70", "203x517", "131x473-3x3-tiles"])
def test_non_integer_ratios(cuda, shape, size):
    """coefficient rows that sum to 2047 / 2049 on both axes (37 -> 9, 100 -> 33, 70 -> 17); the last shape is 2 full tiles and a
    ragged one on both axes (41 = 2 x 16 + 9 rows, 150 = 2 x 64 + 22 columns), W % 4 = 1, w % 4 = 2"""
    H, W = shape[2:]
    sums = lambda s, d: {sum(c) for c in R.axis_tables(s, d)[1]}
    assert sums(H, size[0]) - {2048} and sums(W, size[1]) - {2048}
    assert W % 4 != 0
    _check(cuda, _bytes(shape, sum(shape)), size)


@pytest.mark.parametrize("shape, size", [((2, 3, 16, 24), (16, 24)), ((1, 3, 64, 128), (8, 16)), ((3, 1, 4, 4), (1, 1)), ((2, 3, 5, 9), (2, 3))],
                         ids=["ratio1", "ratio8", "4x4-to-1", "5x9-to-2x3"])
def test_limits(cuda, shape, size):
    """ratio 1 is the identity; ratio 8 is the largest; 5 x 9 -> 2 x 3: both output rows read a clamped source row, and the first and
    last output columns begin / end at the plane's edge (9 -> 3 is plain decimation: taps 3 d .. 3 d + 3)"""
    x = _bytes(shape, 7)
    want, _ = _check(cuda, x, size)
    if shape[2:] == size:
        assert np.array_equal(want, x)
    if shape[2:] == (5, 9):
        assert all(s - 1 < 0 or s + 2 > 4 for s in R.axis_tables(5, 2)[0])
        assert R.axis_tables(9, 3)[0] == [1, 4, 7]


@pytest.mark.parametrize("shape, size", [((1, 3, 96, 128), (24, 32)), ((1, 1, 203, 203), (50, 50))], ids=["x4", "203-to-50"])
def test_checkerboard_saturates_on_both_sides(cuda, shape, size):
    yy, xx = np.indices(shape[2:])
    board = np.where(((yy // 3) + (xx // 3)) % 2 == 0, 0, 255).astype(np.uint8)
    x = np.ascontiguousarray(np.broadcast_to(board, shape))
    _, v = _check(cuda, x, size)
    _, low, high = R.counts(v)
    assert low > 0 and high > 0, (low, high)


def test_unaligned_input_and_output(cuda, x4_case, x2_case):
    """a contiguous view 1, 2 and 3 bytes into a buffer: the aligned dwords that cover a row begin before the view (and, for the
    view that ends the buffer, end after it); an unaligned `out` with w % 4 == 0 takes the byte stores"""
    from eavsr_amd import ops
    for (x, want), size in ((x4_case, (64, 80)), (x2_case, (19, 35))):
        n = x.size
        for off in (1, 2, 3):
            buf = torch.zeros(off + n, dtype=torch.uint8, device=cuda)
            view = buf[off:].view(x.shape)
            view.copy_(_dev(x, cuda))
            assert view.data_ptr() % 4 == off and view.is_contiguous()
            _same(ops.resize_cubic_u8(view, size), want, f"input at +{off}")
            obuf = torch.zeros(off + want.size, dtype=torch.uint8, device=cuda)
            out = obuf[off:].view(want.shape)
            assert ops.resize_cubic_u8(_dev(x, cuda), size, out=out) is out
            _same(out, want, f"out at +{off}")
            assert int(obuf[:off].sum()) == 0


def test_out_and_argument_errors(cuda):
    from eavsr_amd import ops
    x = _dev(_bytes((2, 3, 32, 48), 3), cuda)
    want, _ = R.resize_cubic_u8(x.cpu().numpy(), (8, 12))
    store = torch.zeros(5, 3, 8, 12, dtype=torch.uint8, device=cuda)
    r = ops.resize_cubic_u8(x, (8, 12), out=store[2:4])
    assert r.data_ptr() == store[2:4].data_ptr()
    _same(store[2:4], want)
    assert int(store[:2].sum()) == 0 and int(store[4:].sum()) == 0
    with pytest.raises(ValueError, match="out"):
        ops.resize_cubic_u8(x, (8, 12), out=store[:2, :, :, :8])
    with pytest.raises(ValueError, match="out"):
        ops.resize_cubic_u8(x, (8, 12), out=store[:3])
    with pytest.raises(ValueError, match="out"):
        ops.resize_cubic_u8(x, (8, 12), out=store[:2].float())
    with pytest.raises(ValueError, match="out"):
        ops.resize_cubic_u8(x, (8, 12), out=store[:2].cpu())
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.resize_cubic_u8(x.cpu(), (8, 12))
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_cubic_u8(x.float(), (8, 12))
    with pytest.raises(ValueError, match="uint8"):
        ops.resize_cubic_u8(x[0], (8, 12))
    with pytest.raises(ValueError, match="contiguous"):
        ops.resize_cubic_u8(x[:, :, :, ::2], (8, 12))
    with ops.profile() as prof:
        with pytest.raises(ValueError, match="ratio"):
            ops.resize_cubic_u8(_dev(_bytes((1, 1, 36, 36), 4), cuda), (4, 4))      # ratio 9
        with pytest.raises(ValueError, match="ratio"):
            ops.resize_cubic_u8(x, (33, 12))                                          # upscaling
    assert prof.summary() == {}                                                       # refused on the host: nothing was launched


def test_profile_sees_one_launch_per_call(cuda):
    from eavsr_amd import ops
    x = _dev(_bytes((2, 3, 64, 96), 5), cuda)
    with ops.profile() as prof:
        ops.resize_cubic_u8(x, (16, 24))
    s = prof.summary()
    assert list(s) == ["resize_cubic_u8"] and s["resize_cubic_u8"]["calls"] == 1
    assert s["resize_cubic_u8"]["bytes"] == 2 * 3 * (64 * 96 + 16 * 24)
    with ops.profile() as prof:
        ops.resize_cubic_u8(x, (16, 24))
        ops.resize_cubic_u8(x, (32, 48))
    assert prof.summary()["resize_cubic_u8"]["calls"] == 2


# ------------------------------------------------------------------------------------------------------------- the store
def _wide_hr(F, C, H, W, seed):
    return _bytes((F, C, H, W), seed), _bytes((F, C, H, W), seed + 1)


def test_from_wide_equals_the_oracle_planar_and_interleaved_and_does_not_depend_on_chunk(cuda):
    from eavsr_amd.dataset import FramePairs
    wide, hr = _wide_hr(8, 3, 40, 56, 11)
    want = R.resize_cubic_u8(wide, (10, 14))[0]
    stores = {"planar": FramePairs.from_wide(wide, hr, 4, 4, device=cuda),
              "interleaved": FramePairs.from_wide(wide.transpose(0, 2, 3, 1), torch.from_numpy(hr).permute(0, 2, 3, 1), 4, 4, device=cuda),
              "chunk1": FramePairs.from_wide(torch.from_numpy(wide), hr, 4, 4, device=cuda, chunk=1),
              "chunk3": FramePairs.from_wide(wide, hr, 4, 4, device=cuda, chunk=3),
              "chunk8": FramePairs.from_wide(_dev(wide, cuda), _dev(hr, cuda), 4, 4, chunk=8),
              "chunk100": FramePairs.from_wide(wide, hr, 4, 4, device=cuda, chunk=100)}
    for name, s in stores.items():
        assert s.lr.device == cuda and s.scale == 4 and s.n_seq == 4 and len(s) == 8 and s.frame_size == (10, 14), name
        _same(s.lr, want, name)
        _same(s.hr, hr, name)
        assert s.names[5] == "001_00001.png"
    x2 = FramePairs.from_wide(wide, None, 2, 8, names=[f"f{i}" for i in range(8)], device=cuda)
    assert x2.hr is None and x2.names[3] == "f3"
    _same(x2.lr, R.resize_cubic_u8(wide, (20, 28))[0], "x2, no hr")


def _mirrored_window(key, n_frame, n_seq):
    """the reference's window around key frame `key`: a neighbour that would leave the scene is mirrored about the key frame"""
    frame, half = key % n_seq, n_frame // 2
    return [key + o if 0 <= frame + o < n_seq else key - o for o in range(-half, n_frame - half)]


def _item(frames_u8, top, left, patch, flags):
    """the reference's item from (t, C, H, W) bytes: crop, then [:, :, ::-1] (hflip), [:, ::-1, :] (vflip), transpose(0, 2, 1), then
    np.float32(.) / 255"""
    out = []
    for img in frames_u8:
        img = img[:, top:top + patch, left:left + patch]
        if flags & 1:
            img = img[:, :, ::-1]
        if flags & 2:
            img = img[:, ::-1, :]
        if flags & 4:
            img = img.transpose(0, 2, 1)
        out.append(np.float32(img) / np.float32(255))
    return np.stack(out)


def test_an_epoch_of_train_batches_from_a_wide_store(cuda):
    """F = 8, n_seq = 4, 96 x 128 frames, scale 4: every batch of one epoch is, bit for bit, the reference's item built from the
    ORACLE's LR frames and the HR bytes (window, crop and flips restated above; the crop origin and the flips are the plan's)"""
    from eavsr_amd.dataset import FramePairs, TrainBatches
    wide, hr = _wide_hr(8, 3, 96, 128, 21)
    lr = R.resize_cubic_u8(wide, (24, 32))[0]
    store = FramePairs.from_wide(wide, hr, 4, 4, device=cuda, chunk=3)
    batches = TrainBatches(store, batch_size=2, patch_size=16, n_frame=3, seed=5, rank=0, world=1)
    assert len(batches) == 4
    frames, desc = batches.frames.cpu().numpy(), batches.desc.cpu().numpy()
    seen, flag_sets = [], set()
    for b, batch in enumerate(batches):
        for j in range(2):
            key = int(frames[b, j, 1])
            window = _mirrored_window(key, 3, 4)
            assert frames[b, j].tolist() == window and batch["fname"][j] == store.names[key]
            top, left, flags = (int(v) for v in desc[b, j, :3])
            want_lr = _item(lr[window], top, left, 16, flags)
            want_hr = _item(hr[window], 4 * top, 4 * left, 64, flags)
            assert torch.equal(batch["lr_seq"][j].cpu(), torch.from_numpy(want_lr)), (b, j)
            assert torch.equal(batch["hr_seq"][j].cpu(), torch.from_numpy(want_hr)), (b, j)
            seen.append(key)
            flag_sets.add(flags)
    assert sorted(seen) == list(range(8)) and len(flag_sets) > 1
    assert any(len(set(_mirrored_window(k, 3, 4))) == 2 for k in seen)      # a mirrored window was among them


def test_from_wide_files_equals_from_wide(cuda, tmp_path):
    from eavsr_amd import harness
    from eavsr_amd.dataset import FramePairs
    wide, hr = _wide_hr(4, 3, 8, 12, 31)
    paths = {"wide": [], "tele": []}
    for kind, frames in (("wide", wide), ("tele", hr)):
        for i, img in enumerate(frames):
            paths[kind].append(harness.write_png(torch.from_numpy(img), os.path.join(tmp_path, f"{kind}_{i}.png")))
    a = FramePairs.from_wide_files(paths["wide"], paths["tele"], 2, 2, device=cuda, chunk=3)
    b = FramePairs.from_wide(wide, hr, 2, 2, device=cuda)
    assert torch.equal(a.lr, b.lr) and torch.equal(a.hr, b.hr) and a.names == b.names
    _same(a.lr, R.resize_cubic_u8(wide, (4, 6))[0])
    c = FramePairs.from_wide_files(paths["wide"], None, 2, 4, device=cuda)
    assert c.hr is None and torch.equal(c.lr, b.lr)


# ------------------------------------------------------------------------------------------------------------- large extents
def test_a_wide_input_above_4_gib(cuda):
    """21900 x 3 x 256 x 256 = 4.306e9 bytes in (past 2^31 and 2^32 samples and 2^32 bytes), x4.  A: the first and last frames and
    the frames that hold samples 2^31 and 2^32, against the oracle; B: the whole result, bit for bit, against the op run over 4096
    frames at a time.  65700 planes: more than a grid's y or z extent takes, so this also shows that planes are folded into grid x
    (the limit of THAT, 2^24 - 1 workgroups, is refused by name: tests/test_resample_host.py)."""
    from eavsr_amd import ops
    n, c, H, W = 21900, 3, 256, 256
    need = n * c * (H * W + 2 * (H // 4) * (W // 4)) + 2 ** 30
    free = torch.cuda.mem_get_info(cuda)[0]
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory, {free / 2 ** 30:.1f} GiB are free")
    x = L.fill_chunks(torch.empty((n, c, H, W), device=cuda, dtype=torch.uint8), lambda t, g: t.random_(0, 256, generator=g), 41, 1024)
    assert n * c > 65535 and x.numel() > 2 ** 32
    rep = L.check_extents("resize_cubic_u8", lambda lo, hi: ops.resize_cubic_u8(x[lo:hi], (H // 4, W // 4)),
                          lambda i: torch.from_numpy(R.resize_cubic_u8(x[i].cpu().numpy(), (H // 4, W // 4))[0]), n, 4096,
                          extent_of=x, must_cross=("elem31", "byte32", "elem32"), profile=ops.profile, route=ops.route_batch)
    assert rep["kernels"] == ["resize_cubic_u8"]
    assert {"first", "last", "in:elem31", "in:byte32"} <= set(rep["images"]) and len(set(rep["images"].values())) >= 4
    del x
    torch.cuda.empty_cache()
