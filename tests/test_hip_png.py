"""The device PNG encoder on the GPU (`pytest -m gpu`): csrc/png.hip through ops.png_filter / deflate_huffman / png_encode,
harness.encode_png_frames, save_frames_rgb8(encoder="device") and super_resolve(png_encoder="device").

The filter pass is compared with the numpy oracle (tests/png_ref.py) bit for bit.  The entropy pass has no bit-exact reference -- any
valid Huffman code will do -- so zlib is the judge: `zlib.decompress` must consume the whole stream (it then has verified the
Adler-32) and return the input, and the oracle's parser describes what the stream is made of.  Shapes are the smallest at which the
named part can fail."""
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import png_images as I
from tests import png_ref as P

pytestmark = pytest.mark.gpu


def _frames(f, h, w, c, seed=0):
    return np.stack([I.gradient_noise(h, w, c, seed=seed + 31 * k) for k in range(f)])


def _streams(enc):
    data, offsets, sizes = enc.data.cpu().numpy(), enc.offsets.tolist(), enc.sizes.tolist()
    return [data[o:o + n].tobytes() for o, n in zip(offsets, sizes)]


# --------------------------------------------------------------------------------------------------------------- filter pass
FILTER_CASES = [
    ("rgb 1x1", _frames(1, 1, 1, 3)),
    ("rgb 3x5", _frames(1, 3, 5, 3, 1)),
    ("rgb 7x13", _frames(1, 7, 13, 3, 2)),
    ("grey 5x9", _frames(1, 5, 9, 1, 3)),
    ("rgb 33x64, three frames", _frames(3, 33, 64, 3, 4)),
    ("noise 33x64, three frames", np.random.default_rng(9).integers(0, 256, (3, 33, 64, 3), dtype=np.uint8)),
    ("every filter wins a row", I.five_winners()[None]),
    ("a row longer than the workgroup", _frames(2, 4, 301, 3, 5)),
]


@pytest.mark.parametrize("name, frames", FILTER_CASES, ids=[c[0] for c in FILTER_CASES])
def test_filter_pass_equals_the_oracle(cuda, name, frames):
    from eavsr_amd import ops
    want = P.filter_frames(frames)
    got = ops.png_filter(torch.from_numpy(frames).to(cuda))
    assert got.shape == want.shape and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    if "every filter" in name:
        assert set(want[0, :, 0].tolist()) == {0, 1, 2, 3, 4}
    out = torch.empty_like(got)
    assert ops.png_filter(torch.from_numpy(frames).to(cuda), out=out) is out and torch.equal(out, got)


# ---------------------------------------------------------------------------------------------------------------- round trip
def _check_idat(stream, frame):
    raw = P.inflate_all(stream)      # consumed to the last byte: zlib has verified the Adler-32
    assert raw == P.filter_rows(frame).tobytes()


def _check_file(data, frame, tmp_path, tag):
    from eavsr_amd import harness
    h, w, c = frame.shape
    hdr, idat = P.split_png(data)
    assert hdr == (w, h, 8, 2 if c == 3 else 0, 0, 0, 0) and len(idat) == 1
    _check_idat(idat[0], frame)
    path = tmp_path / f"{tag}.png"
    path.write_bytes(data)
    assert torch.equal(harness.read_png(str(path)), torch.from_numpy(frame).permute(2, 0, 1))


ROUND_TRIP = [("h1", 1, 1), ("h31", 1, 31), ("h32", 1, 32), ("h33", 1, 33), ("h65", 1, 65), ("constant", 1, 40), ("three frames", 3, 33)]


@pytest.mark.parametrize("name, f, h", ROUND_TRIP, ids=[r[0] for r in ROUND_TRIP])
def test_png_encode_round_trip(cuda, tmp_path, name, f, h):
    """stripe_rows = 32: a short stripe, an exact one, one row more, a ragged last stripe; a constant image (every residual 0: a
    two-symbol code); three frames"""
    from eavsr_amd import harness, ops
    frames = np.full((f, h, 21, 3), 77, np.uint8) if name == "constant" else _frames(f, h, 21, 3, seed=h)
    x = torch.from_numpy(frames).to(cuda)
    enc = ops.png_encode(x, stripe_rows=32)
    again = ops.png_encode(x, stripe_rows=32)
    assert torch.equal(enc.sizes, again.sizes) and torch.equal(enc.offsets, again.offsets)
    streams, streams_again = _streams(enc), _streams(again)
    assert streams == streams_again      # two calls, equal bytes (the slots' unused tails are not part of the streams)
    cap = enc.data.numel() // f
    for k in range(f):
        _check_idat(streams[k], frames[k])
        assert enc.offsets[k].item() == k * cap and len(streams[k]) <= cap
        _check_file(P.png_file(streams[k], h, 21, 3), frames[k], tmp_path, f"enc{k}")
    files = harness.encode_png_frames(x)
    assert len(files) == f
    for k in range(f):
        _check_file(files[k], frames[k], tmp_path, f"file{k}")
        assert P.split_png(files[k])[1][0] == streams[k]
    names = ["%03d_%05d.png" % (0, k) for k in range(f)]
    written = harness.save_frames_rgb8(x, names, str(tmp_path / "root"), encoder="device")
    host = harness.save_frames_rgb8(x, names, str(tmp_path / "root_host"))
    assert [p.split("root/")[1] for p in written] == [p.split("root_host/")[1] for p in host]
    for k, path in enumerate(written):
        assert open(path, "rb").read() == files[k]
        assert torch.equal(harness.read_png(path), harness.read_png(host[k]))


def test_no_frames_is_no_launch(cuda):
    from eavsr_amd import harness, ops
    x = torch.empty((0, 4, 5, 3), dtype=torch.uint8, device=cuda)
    enc = ops.png_encode(x)
    assert tuple(ops.png_filter(x).shape) == (0, 4, 16) and enc.data.numel() == 0 and enc.sizes.numel() == 0 and enc.offsets.numel() == 0
    assert harness.encode_png_frames(x) == []


def test_grey_frames_round_trip(cuda, tmp_path):
    from eavsr_amd import harness
    frames = _frames(2, 35, 19, 1, seed=8)
    for k, data in enumerate(harness.encode_png_frames(torch.from_numpy(frames).to(cuda), stripe_rows=16)):
        _check_file(data, frames[k], tmp_path, f"grey{k}")


# -------------------------------------------------------------------------------------------------------------- entropy pass
def _fibonacci_bytes(first, n, seed):
    """n symbols whose counts are consecutive Fibonacci numbers from the `first`-th on, shuffled"""
    fib = [1, 1]
    while len(fib) < first + n:
        fib.append(fib[-1] + fib[-2])
    counts = fib[first:first + n]
    data = np.repeat(np.arange(n, dtype=np.uint8) * 11 + 3, counts)
    np.random.default_rng(seed).shuffle(data)
    return data


def _deflate(cuda, raw, stripe_bytes):
    from eavsr_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(raw)).to(cuda)
    x = x.view(1, -1) if x.dim() == 1 else x
    enc = ops.deflate_huffman(x, stripe_bytes)
    again = ops.deflate_huffman(x, stripe_bytes)
    streams = _streams(enc)
    assert streams == _streams(again) and torch.equal(enc.sizes, again.sizes)
    rows = x.cpu().numpy()
    parsed = []
    for k, s in enumerate(streams):
        assert P.inflate_all(s) == rows[k].tobytes()
        got = P.parse_zlib(s)
        assert got["data"] == rows[k].tobytes() and got["adler_ok"] and got["consumed"] == len(s)
        for b in got["blocks"]:
            assert not b["has_match"]
            if b["type"] == "dynamic":      # literals and end-of-block only: 257 lengths, one distance code of zero bits
                assert len(b["lit_lengths"]) == 257 and b["dist_lengths"] == [0] and not b["final"]
                assert max(b["lit_lengths"]) <= 15 and P.kraft(b["lit_lengths"]) <= 1.0 and max(b["cl_lengths"]) <= 7
        assert got["blocks"][-1] == {"final": True, "has_match": False, "type": "fixed", "bytes": 0}
        assert all(not b["final"] for b in got["blocks"][:-1])
        parsed.append(got["blocks"][:-1])
    return streams, parsed


def test_fibonacci_counts_meet_the_15_bit_limit(cuda):
    raw = _fibonacci_bytes(0, 22, seed=1)      # 1, 1, 2, 3, ... 17711: 46367 bytes
    assert raw.size == 46367
    _, parsed = _deflate(cuda, raw, raw.size)
    assert [b["type"] for b in parsed[0]] == ["dynamic", "stored"] and parsed[0][1]["bytes"] == 0
    # from the second Fibonacci number on the counts 1 (end-of-block), 1, 2, 3, 5, ... form one chain whatever the tie rule: the
    # unlimited tree is 22 deep, so the limiter must act -- and a limited code of 23 symbols that uses 15 bits is still complete
    chain = _fibonacci_bytes(1, 22, seed=2)
    assert chain.size == 75023
    _, parsed = _deflate(cuda, chain, chain.size)
    lens = parsed[0][0]["lit_lengths"]
    assert max(lens) == 15 and P.kraft(lens) == 1.0


def test_adler_of_70000_times_ff(cuda):
    """b passes 2^32 without the periodic modulo: sum of 255 i for i <= 70000 is 6.2e11"""
    raw = np.full(70000, 0xFF, np.uint8)
    streams, parsed = _deflate(cuda, raw, 70000)
    assert [b["type"] for b in parsed[0]] == ["dynamic", "stored"]
    assert sorted(n for n in parsed[0][0]["lit_lengths"] if n) == [1, 1] and len(streams[0]) < 70000 // 8 + 64


def test_random_bytes_are_stored(cuda):
    from eavsr_amd import _native
    stripe = 67232      # 32 rows of a 700-pixel RGB image
    raw = np.random.default_rng(3).integers(0, 256, stripe, dtype=np.uint8)
    streams, parsed = _deflate(cuda, raw, stripe)
    assert [b["type"] for b in parsed[0]] == ["stored", "stored"] and [b["bytes"] for b in parsed[0]] == [65535, stripe - 65535]
    assert len(streams[0]) - 8 == stripe + 10 <= stripe + 5 * -(-stripe // 65535) + 9
    assert len(streams[0]) <= _native.load().eavsr_png_capacity(stripe, stripe)


def test_one_byte(cuda):
    streams, parsed = _deflate(cuda, np.array([200], np.uint8), 32)
    assert [b["type"] for b in parsed[0]] == ["stored"] and len(streams[0]) == 2 + 6 + 6      # 5 + 1 stored beats any dynamic header


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_ragged_stripes_frames_and_alignment(cuda, offset):
    """nbytes is no multiple of stripe_bytes, two frames, stripes that begin at every phase of a dword (2501 and 1001 are odd, and the
    tensor itself starts `offset` bytes into its allocation)"""
    from eavsr_amd import ops
    base = torch.from_numpy(np.concatenate([np.zeros(offset, np.uint8), I.gradient_noise(2, 2501, 1, seed=4).reshape(-1)])).to(cuda)
    x = base[offset:].view(2, 2501)
    enc = ops.deflate_huffman(x, 1001)
    rows = x.cpu().numpy()
    for k, s in enumerate(_streams(enc)):
        assert P.inflate_all(s) == rows[k].tobytes()
        blocks = P.parse_zlib(s)["blocks"]
        assert [b["bytes"] for b in blocks if b["bytes"]] == [1001, 1001, 499] and not any(b["has_match"] for b in blocks)


# ---------------------------------------------------------------------------------------------------------------------- size
def test_size_against_zlibs_huffman_only_coder_and_against_write_png(cuda, tmp_path):
    """256 x 256 RGB, smooth gradients plus sigma 3 noise.  The device stream against zlib's own Huffman-only coder on the same
    filtered bytes, framed the same way: 2 % allowance (a dynamic header is about 100 bytes against about 12 KB per stripe, and the
    length limiter is idle on such residuals).  And the file must be smaller than write_png's."""
    from eavsr_amd import harness, ops
    frame = I.gradient_noise(256, 256, 3, seed=6)
    x = torch.from_numpy(frame[None]).to(cuda)
    stream = _streams(ops.png_encode(x, stripe_rows=32))[0]
    rows = P.filter_rows(frame).tobytes()
    assert P.inflate_all(stream) == rows
    ref = P.huffman_only_stripes(rows, 32 * (1 + 256 * 3))
    assert P.inflate_all(ref) == rows
    print(f"device {len(stream)} bytes, zlib Huffman-only {len(ref)} bytes, ratio {len(stream) / len(ref):.4f}; raw {len(rows)}")
    assert len(stream) <= 1.02 * len(ref)
    host = open(harness.write_png(torch.from_numpy(frame), str(tmp_path / "host.png"), hwc=True), "rb").read()
    dev = harness.encode_png_frames(x)[0]
    print(f"device file {len(dev)} bytes, write_png {len(host)} bytes, ratio {len(dev) / len(host):.4f}")
    assert len(dev) < len(host)


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_super_resolve_with_the_device_encoder_writes_the_same_pictures(cuda, tmp_path):
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.utils.synthetic import synthetic_clip
    model = EAVSRPModel(Namespace(predict=False, n_frame=7, n_flow=5, scale=4, isTrain=False, gpu_ids=[0]))
    model.netEAVSRP.load_state_dict(H.filled(H.model_shapes("x4"), "trained_like"), strict=True)
    model.eval()
    assert model.png_encoder == "host"
    lr = synthetic_clip(1, 5, 64, 96, seed=13)
    hr = torch.nn.functional.interpolate(lr.view(5, 3, 64, 96), scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    names = ["%03d_%05d.png" % (i // 3, i) for i in range(5)]
    res = {}
    for enc in ("host", "device"):      # frame_chunk = 2: chunks of 2, 2 and 1 frames -- two deferred writes and the one after the forward
        res[enc] = harness.super_resolve(model, lr[0], out_dir=str(tmp_path / enc), hr=hr, names=names, frame_chunk=2, png_encoder=enc)
    assert [p.split("/host/")[1] for p in res["host"]["written"]] == [p.split("/device/")[1] for p in res["device"]["written"]] == names
    for a, b in zip(res["host"]["written"], res["device"]["written"]):
        assert torch.equal(harness.read_png(a), harness.read_png(b))
        assert len(P.split_png(open(b, "rb").read())[1]) == 1
    assert res["host"]["report"] == res["device"]["report"]
    assert res["host"]["frame_psnr"] == res["device"]["frame_psnr"] and res["host"]["frame_names"] == res["device"]["frame_names"] == names
    # the option a model wrapper read at construction selects the encoder too
    model.png_encoder = "device"
    via_opt = harness.super_resolve(model, lr[0], out_dir=str(tmp_path / "opt"), names=names, frame_chunk=3)
    for a, b in zip(res["device"]["written"], via_opt["written"]):
        assert open(a, "rb").read() == open(b, "rb").read()
