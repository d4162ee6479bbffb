"""The device PNG encoder (csrc/png.hip, ops.png_filter / deflate_huffman / png_encode, harness.encode_png_frames), what needs no GPU:
the oracle (tests/png_ref.py) against zlib and `harness.read_png`, the heuristic's tie rule on hand-made rows, the C ABI's host-side
argument checks, and the option that selects the encoder."""
import os
import re
import zlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import png_ref as P


def _image(h, w, c, seed=0):
    """smooth gradients plus sigma 3 noise: camera-like, every filter has something to do"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(2.0 * x + 1.0 * y + 40 * k) % 256 for k in range(c)], 2)
    return np.clip(base * 0.8 + 20 + rng.normal(0, 3, (h, w, c)), 0, 255).round().astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("types", [0, 1, 2, 3, 4, None, "cycle"])
@pytest.mark.parametrize("c", [1, 3])
def test_oracle_rows_decode_to_the_pixels_under_every_filter_type(tmp_path, types, c):
    from eavsr_amd import harness
    img = _image(11, 13, c, seed=c)
    forced = np.arange(11) % 5 if types == "cycle" else types
    rows = P.filter_rows(img, forced)
    assert rows.shape == (11, 1 + 13 * c)
    if types in (0, 1, 2, 3, 4):
        assert (rows[:, 0] == types).all()
    path = tmp_path / "a.png"
    path.write_bytes(P.png_file(zlib.compress(rows.tobytes(), 6), 11, 13, c))
    assert torch.equal(harness.read_png(str(path)), torch.from_numpy(img).permute(2, 0, 1))


def test_oracle_filter_0_is_what_write_png_writes(tmp_path):
    from eavsr_amd import harness
    img = _image(9, 7, 3)
    path = harness.write_png(torch.from_numpy(img), str(tmp_path / "w.png"), hwc=True)
    hdr, idat = P.split_png(open(path, "rb").read())
    assert hdr == (7, 9, 8, 2, 0, 0, 0) and len(idat) == 1
    assert P.inflate_all(idat[0]) == P.filter_rows(img, 0).tobytes()


def test_heuristic_ties_go_to_the_lowest_filter_number():
    # nothing to predict: all five filters cost 0 -> filter 0
    assert (P.filter_rows(np.zeros((3, 4, 3), np.uint8))[:, 0] == 0).all()
    # row 0 has no previous row: up == none and Paeth == sub byte for byte, so 2 and 4 never win there; a ramp makes sub cheaper
    ramp = np.tile((np.arange(16, dtype=np.uint8) * 3 + 100)[None, :, None], (1, 1, 3))
    cand = P.filter_candidates(ramp)
    costs = P.row_costs(cand)
    assert np.array_equal(cand[0], cand[2]) and np.array_equal(cand[1], cand[4])
    assert costs[1, 0] == costs[4, 0] < costs[3, 0] < costs[0, 0] and P.filter_rows(ramp)[0, 0] == 1
    # hand-made costs: the first minimum wins
    assert P.choose_filters(np.array([[5], [3], [3], [4], [3]])).tolist() == [1]
    assert P.choose_filters(np.array([[7], [9], [7], [7], [8]])).tolist() == [0]
    assert P.choose_filters(np.array([[9], [9], [9], [2], [2]])).tolist() == [3]
    # signed reading: 255 is -1 and costs 1, 128 is -128 and costs 128
    assert P.row_costs(np.array([[[255, 1, 128, 0]]], np.uint8)).tolist() == [[130]]
    # identical rows: row 1 is predicted exactly by up (2), and so by Paeth and nothing cheaper -- 2 wins over 4
    two = np.concatenate([ramp, ramp], 0) + np.random.default_rng(0).integers(0, 40, (1, 16, 3), dtype=np.uint8)
    assert P.filter_rows(two)[1, 0] == 2 and P.row_costs(P.filter_candidates(two))[2, 1] == P.row_costs(P.filter_candidates(two))[4, 1] == 0


def test_each_filter_wins_somewhere_in_the_mixed_image():
    from tests.png_images import five_winners
    assert set(P.filter_rows(five_winners())[:, 0].tolist()) == {0, 1, 2, 3, 4}


@pytest.mark.parametrize("how", ["stored", "fixed", "level1", "level6", "huffman"])
def test_parser_describes_zlibs_own_streams(how):
    raw = _image(24, 40, 3, seed=7).tobytes() + bytes(300)
    if how == "stored":
        stream = zlib.compress(raw, 0)
    elif how == "fixed":
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_FIXED)
        stream = c.compress(raw) + c.flush()
    elif how == "huffman":
        stream = P.huffman_only_stripes(raw, 1000)
    else:
        stream = zlib.compress(raw, 1 if how == "level1" else 6)
    got = P.parse_zlib(stream)
    assert got["data"] == raw and got["adler_ok"] and got["consumed"] == len(stream) and got["blocks"][-1]["final"]
    kinds = {b["type"] for b in got["blocks"]}
    if how == "stored":
        assert kinds == {"stored"} and not any(b["has_match"] for b in got["blocks"])
    if how == "fixed":
        assert kinds == {"fixed"} and any(b["has_match"] for b in got["blocks"])      # the run of zeros
    if how == "huffman":
        assert not any(b["has_match"] for b in got["blocks"]) and sum(b["bytes"] for b in got["blocks"]) == len(raw)
        assert P.inflate_all(stream) == raw
    for b in got["blocks"]:
        if b["type"] == "dynamic":
            assert max(b["lit_lengths"]) <= 15 and max(b["cl_lengths"]) <= 7 and P.kraft(b["lit_lengths"]) <= 1.0


# ------------------------------------------------------------------------------------------------ the C ABI, without a device
def test_png_entry_points_are_in_the_stable_header_and_check_their_arguments_on_the_host():
    from eavsr_amd import _native
    lib = _native.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eavsr_hip.h")).read()
    stable = header.split(" * EXPERIMENTAL -- exported by the LAB build only")[0]
    for name in ("eavsr_png_filter_u8", "eavsr_deflate_huffman_u8", "eavsr_png_capacity", "eavsr_deflate_workspace_bytes"):
        assert name in _native.SIGNATURES and re.search(r"^int(64_t)? %s\(" % name, stable, flags=re.M), name
    assert lib.eavsr_abi_version() == 32
    p = 64      # an aligned, never dereferenced address: every call below fails (or returns) before a launch
    g = lib.eavsr_png_filter_u8
    assert g(None, p, 1, 4, 4, 3, None) == -1 and b"NULL" in lib.eavsr_last_error()
    assert g(p, None, 1, 4, 4, 3, None) == -1
    for c in (0, 2, 4):
        assert g(p, p, 1, 4, 4, c, None) == -2 and b"grey (1) or RGB (3)" in lib.eavsr_last_error()
    assert g(p, p, 1, 0, 4, 3, None) == -2 and g(p, p, 1, 4, -1, 3, None) == -2 and g(p, p, -1, 4, 4, 3, None) == -2
    assert g(p, p, 65536, 4, 4, 3, None) == -2 and b"grid y" in lib.eavsr_last_error()
    assert g(p, p, 1, 1, (1 << 24) + 1, 1, None) == -2 and b"2^24" in lib.eavsr_last_error()
    assert g(p, p, 1, 46341, 46341, 1, None) == -2 and b"2^31 - 1" in lib.eavsr_last_error()      # 46341 x 46342 > 2^31 - 1
    assert g(p, p, 0, 4, 4, 3, None) == 0                                                          # F = 0: nothing is launched
    d = lib.eavsr_deflate_huffman_u8
    assert d(None, p, p, p, p, 1, 100, 10, None) == -1 and b"NULL" in lib.eavsr_last_error()
    for k in range(1, 5):
        args = [p] * 5
        args[k] = None
        assert d(*args, 1, 100, 10, None) == -1
    assert d(p, p, p, p, p, 1, 0, 10, None) == -2 and d(p, p, p, p, p, 1, 100, 0, None) == -2 and d(p, p, p, p, p, -1, 100, 10, None) == -2
    assert d(p, p, p, p, p, 1, 1 << 31, 1 << 20, None) == -2 and b"2^31 - 1" in lib.eavsr_last_error()
    assert d(p, p, p, p, p, 1, 65536, 1, None) == -2 and b"65535 stripes" in lib.eavsr_last_error()
    assert d(p, p, p, p, p, 65536, 100, 10, None) == -2 and b"grid y" in lib.eavsr_last_error()
    assert d(p, p, p, p, p + 4, 1, 100, 10, None) == -2 and b"aligned" in lib.eavsr_last_error()
    assert d(p, p, p + 4, p, p, 1, 100, 10, None) == -2 and b"aligned" in lib.eavsr_last_error()
    assert d(p, p, p, p, p, 0, 100, 10, None) == 0


def test_capacity_is_the_documented_formula():
    from eavsr_amd import _native
    lib = _native.load()
    per_stripe = lambda s: s + 5 * -(-s // 65535) + 9
    assert lib.eavsr_png_capacity(67232 * 3 + 5, 67232) == 4 * per_stripe(67232) + 8
    assert lib.eavsr_png_capacity(65535, 65535) == 65535 + 5 + 9 + 8 and lib.eavsr_png_capacity(65536, 65536) == 65536 + 10 + 9 + 8
    assert lib.eavsr_png_capacity(10, 1000) == per_stripe(10) + 8      # a stripe longer than the frame is the frame
    assert lib.eavsr_png_capacity(1, 1) == 1 + 5 + 9 + 8
    assert lib.eavsr_png_capacity(0, 1) == -2 and lib.eavsr_png_capacity(1, 0) == -2 and lib.eavsr_png_capacity(1 << 31, 1 << 20) == -2
    assert lib.eavsr_deflate_workspace_bytes(2, 100, 10) >= 2 * 10 * (10 + 5 + 9) and lib.eavsr_deflate_workspace_bytes(2, 100, 10) % 8 == 0
    assert lib.eavsr_deflate_workspace_bytes(65536, 100, 10) == -2


def test_ops_refuse_cpu_tensors_without_touching_a_device():
    from eavsr_amd import harness, ops
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8)
    for call in (lambda: ops.png_filter(img), lambda: ops.png_encode(img), lambda: ops.deflate_huffman(img.view(1, -1), 16),
                 lambda: harness.encode_png_frames(img), lambda: harness.save_frames_rgb8(img, ["000_00000.png"], "unused", encoder="device")):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    with pytest.raises(TypeError):
        ops.png_filter([1, 2])
    with pytest.raises(ValueError, match="encoder"):
        harness.save_frames_rgb8(img, ["000_00000.png"], "unused", encoder="gpu")


# ----------------------------------------------------------------------------------------------------------------- the option
def test_png_encoder_option_defaults_to_host_and_rejects_unknown_values(monkeypatch):
    import inspect
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import long_clip_options, png_encoder_option
    monkeypatch.delenv("EAVSR_PNG_ENCODER", raising=False)
    assert png_encoder_option(None) == "host" and png_encoder_option(Namespace()) == "host"
    assert png_encoder_option(Namespace(png_encoder="device")) == "device"
    assert inspect.signature(harness.super_resolve).parameters["png_encoder"].default is None      # None: the option, else "host"
    assert inspect.signature(harness.save_frames_rgb8).parameters["encoder"].default == "host"
    monkeypatch.setenv("EAVSR_PNG_ENCODER", "device")
    assert png_encoder_option(Namespace()) == "device" and png_encoder_option(Namespace(png_encoder="host")) == "host"      # the options win
    assert long_clip_options(Namespace()) == (None, False)
    monkeypatch.setenv("EAVSR_PNG_ENCODER", "gpu")
    with pytest.raises(ValueError, match="EAVSR_PNG_ENCODER"):
        png_encoder_option(Namespace())
    with pytest.raises(ValueError, match="EAVSR_PNG_ENCODER"):
        long_clip_options(Namespace())
    monkeypatch.delenv("EAVSR_PNG_ENCODER")
    for bad in ("gpu", "", True, 1):
        with pytest.raises(ValueError, match="png_encoder"):
            png_encoder_option(Namespace(png_encoder=bad))
        with pytest.raises(ValueError, match="png_encoder"):
            long_clip_options(Namespace(png_encoder=bad))


def test_super_resolve_rejects_an_unknown_png_encoder_before_any_work(monkeypatch):
    from eavsr_amd import harness
    net = torch.nn.Linear(1, 1)      # never used: the encoder's name is checked first
    with pytest.raises(ValueError, match="png_encoder"):
        harness.super_resolve(net, torch.zeros(2, 3, 64, 64), png_encoder="gpu")
    monkeypatch.setenv("EAVSR_PNG_ENCODER", "fast")
    with pytest.raises(ValueError, match="EAVSR_PNG_ENCODER"):
        harness.super_resolve(net, torch.zeros(2, 3, 64, 64))
    with pytest.raises(ValueError, match="png_encoder"):
        harness.super_resolve(Namespace(opt=Namespace(png_encoder="fast")), torch.zeros(2, 3, 64, 64))
    assert harness.check_png_encoder("host") == "host" and harness.check_png_encoder("device") == "device"
