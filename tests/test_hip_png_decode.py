"""The device PNG decoder (csrc/png_decode.hip) on the GPU.  The expected pixels are always the image a test started from
(tests/png_ref.py filters it, the kernel must undo that bit for bit); where a file exists, `harness.read_png` of it is a second,
independent witness."""
import struct
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import png_images, png_ref

pytestmark = pytest.mark.gpu

SIG = b"\x89PNG\r\n\x1a\n"
CTYPE = {1: 0, 3: 2, 4: 6}
SIZES = [(1, 1), (2, 2), (3, 5), (63, 21), (64, 22), (65, 64), (129, 65), (200, 130)]


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    return _ops


def _random(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def _planes(img, channels=4):
    return torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)[:channels]))


def _unfilter(ops, cuda, rows, c, **kw):
    return ops.png_unfilter(torch.from_numpy(np.ascontiguousarray(rows)).to(cuda), c, **kw).cpu()


def _file(img, types=None, cuts=None, level=6):
    h, w, c = img.shape
    stream = zlib.compress(png_ref.filter_rows(img, types).tobytes(), level)
    cuts = [0] + list(cuts or []) + [len(stream)]
    idats = b"".join(png_ref.chunk(b"IDAT", stream[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
    return (SIG + png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, CTYPE[c], 0, 0, 0)) + idats + png_ref.chunk(b"IEND", b""))


# ------------------------------------------------------------------------------------------------------------- ops.png_unfilter
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("h,w", SIZES)
def test_every_pure_filter_type_gives_back_the_image(ops, cuda, h, w, c):
    """first row, first pixel, both sides of a 64-row band, three bands; (1 + w c) % 4 takes all four values over the sizes"""
    img = _random(h, w, c, seed=h * 1000 + w * 10 + c)
    rows = np.stack([png_ref.filter_rows(img, t) for t in range(5)])
    got = _unfilter(ops, cuda, rows, c, channels=c)
    for t in range(5):
        assert torch.equal(got[t], _planes(img)), f"filter type {t}"


def test_the_sizes_start_rows_at_every_byte_alignment():
    assert {(1 + w * c) % 4 for _, w in SIZES for c in (1, 3, 4)} == {0, 1, 2, 3}


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_a_random_filter_type_per_row(ops, cuda, seed):
    img = png_images.gradient_noise(130, 67, 3, seed=seed)
    types = np.random.default_rng(100 + seed).integers(0, 5, 130)
    assert torch.equal(_unfilter(ops, cuda, png_ref.filter_rows(img, types)[None], 3)[0], _planes(img))


def test_the_adaptive_choice_and_five_winners(ops, cuda):
    img = png_images.gradient_noise(150, 96, 3, seed=4)
    rows = png_ref.filter_rows(img)
    assert len(set(rows[:, 0].tolist())) > 1
    assert torch.equal(_unfilter(ops, cuda, rows[None], 3)[0], _planes(img))
    five = png_images.five_winners()
    rows = png_ref.filter_rows(five)
    assert set(rows[:, 0].tolist()) == {0, 1, 2, 3, 4}
    assert torch.equal(_unfilter(ops, cuda, rows[None], 3)[0], _planes(five))


@pytest.mark.parametrize("c", [1, 3, 4])
def test_paeth_ties_and_the_average_carry(ops, cuda, c):
    """uniform bytes, and bytes from {0, 1, 127, 128, 254, 255} only: equal predictor distances and 9-bit sums"""
    rng = np.random.default_rng(7 + c)
    for img in (_random(70, 33, c, seed=c), rng.choice(np.array([0, 1, 127, 128, 254, 255], np.uint8), (70, 33, c))):
        rows = np.stack([png_ref.filter_rows(img, 3), png_ref.filter_rows(img, 4), png_ref.filter_rows(img, rng.integers(3, 5, 70))])
        got = _unfilter(ops, cuda, rows, c, channels=c)
        for k in range(3):
            assert torch.equal(got[k], _planes(img)), k


def test_a_frame_wider_than_the_hand_over_row_kept_in_lds(ops, cuda):
    img = png_images.gradient_noise(66, 5000, 4, seed=9)
    assert torch.equal(_unfilter(ops, cuda, png_ref.filter_rows(img, 4)[None], 4, channels=4)[0], _planes(img))


def test_channels(ops, cuda):
    img = _random(70, 19, 4, seed=11)
    rows = png_ref.filter_rows(img, np.arange(70) % 5)[None]
    four = _unfilter(ops, cuda, rows, 4, channels=4)
    three = _unfilter(ops, cuda, rows, 4, channels=3)
    assert tuple(four.shape) == (1, 4, 70, 19) and torch.equal(four[0], _planes(img))
    assert tuple(three.shape) == (1, 3, 70, 19) and torch.equal(three, four[:, :3])
    assert torch.equal(_unfilter(ops, cuda, rows, 4)[0], four[0, :3])      # the default drops alpha
    rgb = torch.from_numpy(png_ref.filter_rows(img[:, :, :3])[None]).to(cuda)
    for bad in (0, 5, -1, 3.0, True):
        with pytest.raises(ValueError, match="channels"):
            ops.png_unfilter(rgb, 3, channels=bad)
    with pytest.raises(ValueError, match="channels=4"):
        ops.png_unfilter(rgb, 3, channels=4)
    with pytest.raises(ValueError, match="c=2"):
        ops.png_unfilter(rgb, 2)
    with pytest.raises(ValueError, match="rows"):
        ops.png_unfilter(rgb, 4, channels=4)      # 1 + 19 x 3 bytes are not 1 + W x 4


def test_three_frames_with_different_type_patterns_in_one_launch(ops, cuda):
    imgs = [png_images.gradient_noise(77, 41, 3, seed=20 + i) for i in range(3)]
    rng = np.random.default_rng(21)
    rows = np.stack([png_ref.filter_rows(imgs[0], 4), png_ref.filter_rows(imgs[1], rng.integers(0, 5, 77)), png_ref.filter_rows(imgs[2])])
    got = _unfilter(ops, cuda, rows, 3)
    for i in range(3):
        assert torch.equal(got[i], _planes(imgs[i], 3)), i


def test_out_is_a_slice_of_a_store_with_odd_frames(ops, cuda):
    imgs = [_random(67, 23, 3, seed=30 + i) for i in range(3)]      # 3 x 67 x 23 = 4623 bytes per frame: odd
    rows = torch.from_numpy(np.stack([png_ref.filter_rows(im, np.arange(67) % 5) for im in imgs])).to(cuda)
    store = torch.full((5, 3, 67, 23), 0xAB, device=cuda, dtype=torch.uint8)
    ret = ops.png_unfilter(rows, 3, out=store[1:4])
    assert ret.data_ptr() == store[1:4].data_ptr()
    host = store.cpu()
    for i in range(3):
        assert torch.equal(host[1 + i], _planes(imgs[i], 3)), i
    assert bool((host[0] == 0xAB).all()) and bool((host[4] == 0xAB).all())      # nothing outside the slice


def test_a_wrong_out_is_refused(ops, cuda):
    rows = torch.from_numpy(png_ref.filter_rows(_random(5, 6, 3, seed=1))[None]).to(cuda)
    for bad in (torch.empty((1, 3, 5, 7), device=cuda, dtype=torch.uint8), torch.empty((1, 3, 5, 6), device=cuda, dtype=torch.int8),
                torch.empty((1, 3, 5, 6), dtype=torch.uint8), torch.empty((1, 3, 6, 5), device=cuda, dtype=torch.uint8).transpose(2, 3)):
        with pytest.raises(ValueError, match="png_unfilter: out"):
            ops.png_unfilter(rows, 3, out=bad)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_unfilter(rows.cpu(), 3)


def test_two_calls_are_bit_equal(ops, cuda):
    img = png_images.gradient_noise(140, 90, 3, seed=40)
    rows = torch.from_numpy(png_ref.filter_rows(img)[None]).to(cuda)
    assert torch.equal(ops.png_unfilter(rows, 3), ops.png_unfilter(rows, 3))


def test_a_type_byte_above_four_returns(ops, cuda):
    """the robustness contract of the public entry: the kernel reads its type byte as 0 and stays inside its buffers"""
    rows = png_ref.filter_rows(_random(70, 9, 3, seed=41), 2)
    rows[3, 0], rows[66, 0] = 5, 255
    out = _unfilter(ops, cuda, rows[None], 3)
    assert tuple(out.shape) == (1, 3, 70, 9)


# ------------------------------------------------------------------------------------------------------------ decode_png_frames
def test_decode_files_from_write_png(cuda, tmp_path):
    from eavsr_amd import harness
    imgs = [png_images.gradient_noise(37, 29, 3, seed=50 + i) for i in range(4)]
    paths = [harness.write_png(torch.from_numpy(im), str(tmp_path / f"{i}.png"), hwc=True) for i, im in enumerate(imgs)]
    got = harness.decode_png_frames(paths, cuda)
    assert got.device == cuda and got.dtype == torch.uint8 and tuple(got.shape) == (4, 3, 37, 29)
    for i in range(4):
        assert torch.equal(got[i].cpu(), _planes(imgs[i], 3)) and torch.equal(got[i].cpu(), harness.read_png(paths[i]))
    grey = png_images.gradient_noise(20, 31, 1, seed=55)
    gp = harness.write_png(torch.from_numpy(grey[:, :, 0]), str(tmp_path / "grey.png"))
    assert torch.equal(harness.decode_png_frames([gp], cuda).cpu()[0], harness.read_png(gp))


def test_decode_files_of_the_device_encoder(cuda, tmp_path):
    from eavsr_amd import harness
    frames = np.stack([png_images.gradient_noise(100, 64, 3, seed=60 + i) for i in range(3)])      # four 32-row stripes each
    files = harness.encode_png_frames(torch.from_numpy(frames).to(cuda))
    got = harness.decode_png_frames(files, cuda).cpu()
    for i in range(3):
        path = tmp_path / f"{i}.png"
        path.write_bytes(files[i])
        assert torch.equal(got[i], _planes(frames[i], 3)) and torch.equal(got[i], harness.read_png(str(path)))


def test_decode_multi_idat_bytes_and_paths_mixed(cuda, tmp_path):
    from eavsr_amd import harness
    imgs = [_random(66, 17, 4, seed=70 + i) for i in range(3)]
    files = [_file(imgs[0], np.arange(66) % 5, cuts=[7, 7, 300]), _file(imgs[1], 4), _file(imgs[2])]
    path = tmp_path / "one.png"
    path.write_bytes(files[1])
    got4 = harness.decode_png_frames([files[0], str(path), bytearray(files[2])], cuda, channels=4).cpu()
    got3 = harness.decode_png_frames([files[0], path, files[2]], cuda).cpu()
    for i in range(3):
        assert torch.equal(got4[i], _planes(imgs[i])) and torch.equal(got3[i], _planes(imgs[i], 3))
    assert torch.equal(got3[1], harness.read_png(str(path))[:3])


def test_decode_rejects_before_anything_is_launched(cuda, tmp_path, ops):
    from eavsr_amd import harness
    img = png_images.gradient_noise(12, 10, 3, seed=80)
    good = tmp_path / "good.png"
    good.write_bytes(_file(img))

    def refused(name, data, match):
        bad = tmp_path / name
        bad.write_bytes(data)
        with ops.profile() as prof:
            with pytest.raises(ValueError, match=match):
                harness.decode_png_frames([str(good), str(bad)], cuda)
        assert prof.summary() == {}

    refused("other_size.png", _file(png_images.gradient_noise(12, 11, 3, seed=80)), "other_size.png")
    refused("grey.png", _file(img[:, :, :1]), "grey.png")
    short = zlib.compress(png_ref.filter_rows(img).tobytes()[:-1])
    refused("short.png", png_ref.png_file(short, 12, 10, 3), "short.png")
    stream = bytearray(zlib.compress(png_ref.filter_rows(img).tobytes()))
    stream[len(stream) // 2] ^= 0xFF
    stream[-1] ^= 0xFF      # the Adler-32 as well: whatever the flipped byte decodes to
    refused("corrupt.png", png_ref.png_file(bytes(stream), 12, 10, 3), "corrupt.png")
    rows = png_ref.filter_rows(img)
    rows[7, 0] = 5
    refused("type5.png", png_ref.png_file(zlib.compress(rows.tobytes()), 12, 10, 3), "type5.png: scanline filter 5")
    with pytest.raises(ValueError, match="channels=4"):
        harness.decode_png_frames([str(good)], cuda, channels=4)
    with pytest.raises(ValueError, match="decode_png_frames: out"):
        harness.decode_png_frames([str(good)], cuda, out=torch.empty((1, 3, 12, 11), device=cuda, dtype=torch.uint8))
    with pytest.raises(ValueError, match="no files"):
        harness.decode_png_frames([], cuda)


def test_decode_does_not_depend_on_the_number_of_threads(cuda):
    from eavsr_amd import harness
    files = [_file(png_images.gradient_noise(40, 50, 3, seed=90 + i)) for i in range(9)]
    one = harness.decode_png_frames(files, cuda, threads=1)
    four = harness.decode_png_frames(files, cuda, threads=4)
    again = harness.decode_png_frames(files, cuda)      # the third call reuses the first call's pinned buffer
    assert torch.equal(one, four) and torch.equal(one, again)


# ----------------------------------------------------------------------------------------------------------------------- stores
@pytest.fixture(scope="module")
def pair_files(tmp_path_factory):
    from eavsr_amd import harness
    root = tmp_path_factory.mktemp("pairs")
    lr = [png_images.gradient_noise(16, 24, 3, seed=200 + i) for i in range(8)]
    hr = [png_images.gradient_noise(64, 96, 3, seed=300 + i) for i in range(8)]
    wide = [png_images.gradient_noise(32, 48, 3, seed=400 + i) for i in range(8)]
    tele = [png_images.gradient_noise(32, 48, 3, seed=500 + i) for i in range(8)]
    put = lambda tag, imgs: [harness.write_png(torch.from_numpy(im), str(root / tag / f"{i:05d}.png"), hwc=True) for i, im in enumerate(imgs)]
    return {"lr": put("lr", lr), "hr": put("hr", hr), "wide": put("wide", wide), "tele": put("tele", tele)}


def test_from_files_on_the_device_equals_the_default_reader(cuda, pair_files):
    from eavsr_amd.dataset import FramePairs
    want = FramePairs.from_files(pair_files["lr"], pair_files["hr"], 4, 4, device=cuda)
    for chunk in (3, 1, 8):
        got = FramePairs.from_files(pair_files["lr"], pair_files["hr"], 4, 4, device=cuda, reader="device", chunk=chunk)
        assert got.lr.device == cuda and torch.equal(got.lr, want.lr) and torch.equal(got.hr, want.hr), chunk
        assert got.names == want.names and got.scale == 4 and got.n_seq == 4
    lr_only = FramePairs.from_files(pair_files["lr"], None, 4, 8, device=cuda, reader="device")
    assert lr_only.hr is None and torch.equal(lr_only.lr, want.lr)


def test_from_wide_files_on_the_device_equals_the_default_reader(cuda, pair_files):
    from eavsr_amd.dataset import FramePairs
    want = FramePairs.from_wide_files(pair_files["wide"], pair_files["tele"], 4, 4, device=cuda)
    for chunk in (3, 1, 8):
        got = FramePairs.from_wide_files(pair_files["wide"], pair_files["tele"], 4, 4, device=cuda, reader="device", chunk=chunk)
        assert tuple(got.lr.shape) == (8, 3, 8, 12) and torch.equal(got.lr, want.lr) and torch.equal(got.hr, want.hr), chunk


# ---------------------------------------------------------------------------------------------------------------- super_resolve
def test_super_resolve_from_paths_with_the_device_decoder(cuda, tmp_path, monkeypatch):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.utils.synthetic import synthetic_clip
    monkeypatch.delenv("EAVSR_PNG_DECODER", raising=False)
    opt = Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0])
    model = EAVSRPModel(opt)
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    lr = (synthetic_clip(1, 5, 64, 96, seed=13)[0] * 255).round().to(torch.uint8)
    hr = torch.nn.functional.interpolate(lr.float(), scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 255).round().to(torch.uint8)
    names = ["000_%05d.png" % i for i in range(5)]
    paths = [harness.write_png(lr[i], str(tmp_path / "lr" / names[i])) for i in range(5)]
    hr_paths = [harness.write_png(hr[i], str(tmp_path / "hr" / names[i])) for i in range(5)]
    read = lambda res: [open(p, "rb").read() for p in res["written"]]
    keys = ("frames", "frame_names", "frame_psnr", "frame_ssim", "report")

    host = harness.super_resolve(model, paths, out_dir=str(tmp_path / "host"), hr=hr_paths, png_decoder="host")
    tensors = harness.super_resolve(model, lr, out_dir=str(tmp_path / "tensors"), hr=hr, names=names)
    assert read(host) == read(tensors) and all(host[k] == tensors[k] for k in keys)      # hr as paths: the frames `hr` as a tensor holds
    with _profile() as prof:
        dev = harness.super_resolve(model, paths, out_dir=str(tmp_path / "dev"), hr=hr_paths, png_decoder="device")
    assert prof.summary()["png_unfilter_u8"]["calls"] == 2
    assert [p.rsplit("/", 1)[1] for p in dev["written"]] == names and read(dev) == read(host)
    assert all(dev[k] == host[k] for k in keys)

    def unfilter_calls(m, **kw):
        with _profile() as prof:
            res = harness.super_resolve(m, paths, out_dir=str(tmp_path / "opt"), **kw)
        assert read(res) == read(host)
        return prof.summary().get("png_unfilter_u8", {"calls": 0})["calls"]
    assert unfilter_calls(model) == 0                                            # the default is the host decoder
    model.opt.png_decoder = "device"
    assert unfilter_calls(model) == 1 and unfilter_calls(model, png_decoder="host") == 0
    del model.opt.png_decoder
    monkeypatch.setenv("EAVSR_PNG_DECODER", "device")
    assert unfilter_calls(model) == 1 and unfilter_calls(model.netEAVSRP) == 1
    model.opt.png_decoder = "host"
    assert unfilter_calls(model) == 0                                            # the options win over the environment
    with pytest.raises(ValueError, match="png_decoder"):
        harness.super_resolve(model, paths, png_decoder="gpu")


def _profile():
    from eavsr_amd import ops
    return ops.profile()


# ---------------------------------------------------------------------------------------------------------------------- extents
def test_unfilter_past_2_31_bytes(ops, cuda):
    """F H (1 + W C) = 2.16e9 > 2^31 (and F Cout H W = 2.16e9 as well): the first and the last frame of the big call equal the same
    frames decoded in calls of their own"""
    f, h, w, c = 910, 720, 1100, 3
    r = 1 + w * c
    assert f * h * r > 2 ** 31 and f * c * h * w > 2 ** 31
    need = f * h * r + f * c * h * w + 2 ** 30
    if torch.cuda.mem_get_info(cuda)[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory")
    g = torch.Generator(device=cuda).manual_seed(5)
    rows = torch.empty((f, h, r), device=cuda, dtype=torch.uint8)
    for lo in range(0, f, 128):
        part = rows[lo:lo + 128]
        part.copy_(torch.randint(0, 256, tuple(part.shape), device=cuda, dtype=torch.uint8, generator=g))
        part[:, :, 0] %= 5
    big = ops.png_unfilter(rows, c)
    for i in (0, f - 1):
        assert torch.equal(big[i:i + 1], ops.png_unfilter(rows[i:i + 1], c)), i
    del rows, big
    torch.cuda.empty_cache()
