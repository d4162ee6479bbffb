"""The host half of the device PNG decoder, no GPU: the chunk walk `harness.parse_png` that `read_png` and
`decode_png_frames` share, its rejections, the decoder option, the header's declaration, and the argument checks of the store's
reader="device" that run before the device is touched."""
import os
import struct
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from eavsr_amd import harness
from tests import png_images, png_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = b"\x89PNG\r\n\x1a\n"
CTYPE = {1: 0, 3: 2, 4: 6}


def _ihdr(h, w, c, depth=8, ctype=None, interlace=0):
    return png_ref.chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, CTYPE[c] if ctype is None else ctype, 0, 0, interlace))


def _file(img, types=None, cuts=None, extra=b"", **hdr):
    """a PNG file of img (H, W, C); `cuts`: split the zlib stream over IDAT chunks at these offsets"""
    h, w, c = img.shape
    stream = zlib.compress(png_ref.filter_rows(img, types).tobytes(), 6)
    cuts = [0] + list(cuts or []) + [len(stream)]
    idats = b"".join(png_ref.chunk(b"IDAT", stream[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
    return SIG + _ihdr(h, w, c, **hdr) + extra + idats + png_ref.chunk(b"IEND", b"")


@pytest.mark.parametrize("c", [1, 3, 4])
def test_parse_png_returns_the_size_and_the_whole_stream(c):
    img = png_images.gradient_noise(9, 7, c, seed=c)
    rows = png_ref.filter_rows(img)
    # one stream over three IDAT chunks, one of them empty, behind an ancillary chunk
    data = _file(img, cuts=[5, 5], extra=png_ref.chunk(b"tEXt", b"Comment\0three IDATs"))
    h, w, cc, idat = harness.parse_png(data, "split.png")
    assert (h, w, cc) == (9, 7, c)
    assert zlib.decompress(idat) == rows.tobytes()
    bodies = png_ref.split_png(data)[1]
    assert len(bodies) == 3 and bodies[1] == b"" and b"".join(bodies) == idat


def test_parse_png_on_write_png_and_png_ref_files(tmp_path):
    img = png_images.gradient_noise(6, 5, 3, seed=1)
    path = harness.write_png(torch.from_numpy(img), str(tmp_path / "a.png"), hwc=True)
    h, w, c, idat = harness.parse_png(open(path, "rb").read(), path)
    assert (h, w, c) == (6, 5, 3) and zlib.decompress(idat) == png_ref.filter_rows(img, 0).tobytes()
    stream = zlib.compress(png_ref.filter_rows(img).tobytes())
    assert harness.parse_png(png_ref.png_file(stream, 6, 5, 3), "b") == (6, 5, 3, stream)
    grey = img[:, :, :1]
    gs = zlib.compress(png_ref.filter_rows(grey).tobytes())
    assert harness.parse_png(png_ref.png_file(gs, 6, 5, 1), "g") == (6, 5, 1, gs)


def _rejections():
    img = png_images.gradient_noise(4, 3, 3, seed=2)
    good = _file(img)
    flipped = bytearray(good)
    flipped[good.index(b"IDAT") + 6] ^= 0x40      # a byte of the IDAT body: its CRC no longer matches
    yield "signature", b"\x89PNX" + good[4:]
    yield "crc", bytes(flipped)
    yield "depth16", _file(img, depth=16)
    yield "palette", _file(img, ctype=3)
    yield "interlace", _file(img, interlace=1)
    yield "no_idat", SIG + _ihdr(4, 3, 3) + png_ref.chunk(b"IEND", b"")
    yield "no_ihdr", SIG + png_ref.chunk(b"IDAT", zlib.compress(b"\0" * 40)) + png_ref.chunk(b"IEND", b"")
    yield "cut_mid_chunk", good[:good.index(b"IDAT") + 9]
    yield "cut_mid_header", good[:8 + 25 + 5]


@pytest.mark.parametrize("name,data", list(_rejections()), ids=[n for n, _ in _rejections()])
def test_parse_png_rejects_with_the_files_name(name, data, tmp_path):
    with pytest.raises(ValueError, match="some/file.png"):
        harness.parse_png(data, "some/file.png")
    path = tmp_path / (name + ".png")
    path.write_bytes(data)
    with pytest.raises(ValueError, match=name + ".png"):      # read_png goes through the same walk
        harness.read_png(str(path))


def test_read_png_keeps_its_messages(tmp_path):
    img = png_images.gradient_noise(4, 3, 3, seed=2)
    p = tmp_path / "x.png"
    p.write_bytes(b"not a png at all")
    with pytest.raises(ValueError, match="x.png: not a PNG file"):
        harness.read_png(str(p))
    p.write_bytes(_file(img, depth=16))
    with pytest.raises(ValueError, match="x.png: only non-interlaced 8-bit grey / RGB / RGBA"):
        harness.read_png(str(p))
    bad = bytearray(_file(img))
    bad[-1] ^= 1      # the IEND chunk's CRC
    p.write_bytes(bytes(bad))
    with pytest.raises(ValueError, match=r"x.png: CRC mismatch in chunk b'IEND'"):
        harness.read_png(str(p))
    rows = png_ref.filter_rows(img, 0)
    rows[2, 0] = 7
    p.write_bytes(png_ref.png_file(zlib.compress(rows.tobytes()), 4, 3, 3))
    with pytest.raises(ValueError, match="x.png: scanline filter 7"):
        harness.read_png(str(p))


def test_read_png_still_round_trips_write_png(tmp_path):
    rgb = png_images.gradient_noise(11, 13, 3, seed=3)
    got = harness.read_png(harness.write_png(torch.from_numpy(rgb).permute(2, 0, 1), str(tmp_path / "rgb.png")))
    assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(rgb).permute(2, 0, 1))
    grey = png_images.gradient_noise(5, 4, 1, seed=4)[:, :, 0]
    got = harness.read_png(harness.write_png(torch.from_numpy(grey), str(tmp_path / "grey.png")))
    assert tuple(got.shape) == (1, 5, 4) and torch.equal(got[0], torch.from_numpy(grey))
    # every filter type and RGBA through the shared walk
    rgba = np.random.default_rng(5).integers(0, 256, (10, 6, 4), dtype=np.uint8)
    p = tmp_path / "rgba.png"
    p.write_bytes(_file(rgba, types=np.arange(10) % 5))
    assert torch.equal(harness.read_png(str(p)), torch.from_numpy(rgba).permute(2, 0, 1))


def test_check_png_decoder():
    assert harness.check_png_decoder("host") == "host" and harness.check_png_decoder("device") == "device"
    assert harness.PNG_DECODERS == ("host", "device")
    for bad in ("gpu", None, 1, ""):
        with pytest.raises(ValueError, match="png_decoder"):
            harness.check_png_decoder(bad)


def test_png_decoder_option_precedence(monkeypatch):
    from eavsr_amd.eavsrp_model import png_decoder_option
    monkeypatch.delenv("EAVSR_PNG_DECODER", raising=False)
    assert png_decoder_option() == "host" and png_decoder_option(Namespace()) == "host"
    assert png_decoder_option(Namespace(png_decoder="device")) == "device"
    monkeypatch.setenv("EAVSR_PNG_DECODER", "device")
    assert png_decoder_option() == "device" and png_decoder_option(Namespace()) == "device"
    assert png_decoder_option(Namespace(png_decoder="host")) == "host"      # the options win over the environment
    monkeypatch.setenv("EAVSR_PNG_DECODER", "fast")
    with pytest.raises(ValueError, match="EAVSR_PNG_DECODER"):
        png_decoder_option()
    assert png_decoder_option(Namespace(png_decoder="device")) == "device"
    with pytest.raises(ValueError, match="opt.png_decoder"):
        png_decoder_option(Namespace(png_decoder="gpu"))


def test_header_declares_the_unfilter():
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header.split(" * EXPERIMENTAL -- exported by the LAB build only")[0]
    want = ("int eavsr_png_unfilter_u8(const uint8_t* rows, uint8_t* out, int32_t F, int32_t H, int32_t W, int32_t C, int32_t Cout, "
            "void* stream);")
    assert want in " ".join(stable.split())
    from eavsr_amd import _native
    assert "eavsr_png_unfilter_u8" in _native.SIGNATURES


def test_from_files_device_reader_checks_its_lists_before_the_device(tmp_path):
    from eavsr_amd.dataset import FramePairs
    with pytest.raises(ValueError, match="2 LR and 1 HR files"):
        FramePairs.from_files(["a.png", "b.png"], ["c.png"], 4, 1, reader="device")
    with pytest.raises(ValueError, match="2 wide and 3 HR files"):
        FramePairs.from_wide_files(["a.png", "b.png"], ["c.png"] * 3, 4, 1, reader="device")
    with pytest.raises(ValueError, match="reader='gpu'"):
        FramePairs.from_files(["a.png"], None, 4, 1, reader="gpu")
    img = png_images.gradient_noise(4, 6, 3, seed=7)
    lr = tmp_path / "lr.png"
    lr.write_bytes(_file(img))
    hr = tmp_path / "hr.png"
    hr.write_bytes(_file(png_images.gradient_noise(16, 20, 3, seed=8)))
    with pytest.raises(ValueError, match="hr must be scale 4 x lr"):      # from the two headers, before anything is decoded
        FramePairs.from_files([str(lr)], [str(hr)], 4, 1, reader="device")
    with pytest.raises(ValueError, match="not whole scenes"):
        FramePairs.from_files([str(lr)] * 3, None, 4, 2, reader="device")
