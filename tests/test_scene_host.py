"""Host side of the segmented path, no GPU: `segments.plan_segments` by brute force, `segments.find_cuts` on hand-made
statistics, the option parsing, the C entry's declaration, and the numpy oracle of tests/scene_ref.py on a hand-computed case."""
import os
import re
from argparse import Namespace

import numpy as np
import pytest

from eavsr_amd import segments as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START_LISTS = ([], [1], [3], [5, 6], [7, 20], [2, 4, 6, 8], [10, 11, 12, 30], [39])


def _scenes(t, starts, min_scene):
    """the merge rule restated: scene bounds after dropping starts that would leave a scene shorter than min_scene"""
    kept, last = [], 0
    for s in sorted(starts):
        if s - last >= min_scene and t - s >= min_scene:
            kept.append(s)
            last = s
    return [0] + kept + [t]


@pytest.mark.parametrize("min_scene", [1, 2, 5])
def test_plan_segments_brute_force(min_scene):
    checked = 0
    for t in range(1, 41):
        for starts in START_LISTS:
            starts = [s for s in starts if 0 < s < t]
            bounds = _scenes(t, starts, min_scene)
            for max_frames in [None] + list(range(1, 13)):
                for overlap in ([0, 3] if max_frames is None else range(max_frames)):
                    plan = S.plan_segments(t, starts, max_frames, overlap, min_scene)
                    checked += 1
                    at = 0
                    for a, b, ea, eb in plan:
                        assert a <= ea < eb <= b, (t, starts, max_frames, overlap, plan)
                        assert ea == at, (t, starts, max_frames, overlap, plan)      # emit ranges partition [0, t) in order
                        at = eb
                        scene = [k for k in range(len(bounds) - 1) if bounds[k] <= a < bounds[k + 1]][0]
                        s, e = bounds[scene], bounds[scene + 1]
                        assert s <= a and b <= e, (t, starts, max_frames, overlap, plan)      # no window crosses a kept start
                        want = e - s if max_frames is None else min(e - s, max_frames)
                        assert b - a == want, (t, starts, max_frames, overlap, plan)
                        if max_frames is not None:      # an emitted frame is overlap // 2 inside any artificial window end
                            if a != s:
                                assert ea - a >= overlap // 2, (t, starts, max_frames, overlap, plan)
                            if b != e:
                                assert b - eb >= overlap // 2, (t, starts, max_frames, overlap, plan)
                    assert at == t
                    for k in range(len(bounds) - 1):      # every scene starts and ends a window: nothing propagates across a kept start
                        assert any(a == bounds[k] for a, _, _, _ in plan) and any(b == bounds[k + 1] for _, b, _, _ in plan)
    assert checked > 10000


def test_plan_segments_examples():
    assert S.plan_segments(11, [], 5, 2) == [(0, 5, 0, 4), (3, 8, 4, 7), (6, 11, 7, 11)]
    # stride 16; the last window is shifted back to full length and overlaps its predecessor by more than `overlap`
    assert S.plan_segments(60, [], 20, 4) == [(0, 20, 0, 18), (16, 36, 18, 34), (32, 52, 34, 46), (40, 60, 46, 60)]
    assert S.plan_segments(12, [7]) == [(0, 7, 0, 7), (7, 12, 7, 12)]
    assert S.plan_segments(12, [7], 5, 0) == [(0, 5, 0, 3), (2, 7, 3, 7), (7, 12, 7, 12)]      # m = (2 + 5) // 2
    assert S.plan_segments(1, []) == [(0, 1, 0, 1)]


def test_short_scenes_join_their_predecessor():
    assert S.keep_starts(12, [1, 7, 11], 2) == [7]           # 1: a one-frame first scene; 11: a one-frame last scene
    assert S.keep_starts(12, [5, 6, 8], 2) == [5, 8]         # 6 lies one frame after the kept 5
    assert S.keep_starts(12, [5, 6, 8], 3) == [5, 8]
    assert S.keep_starts(12, [5, 6, 8], 4) == [5]            # 8 - 5 = 3 < 4
    assert S.keep_starts(12, [8, 5, 6], 1) == [5, 6, 8]      # sorted; min_scene 1 keeps every start
    assert S.plan_segments(12, [1, 7, 11]) == [(0, 7, 0, 7), (7, 12, 7, 12)]
    assert S.MIN_SCENE_FLOOR == 1
    with pytest.raises(ValueError):
        S.plan_segments(12, [7], min_scene=0)


@pytest.mark.parametrize("kwargs", [dict(t=10, starts=[], max_frames=0), dict(t=10, starts=[], max_frames=4, overlap=-1),
                                    dict(t=10, starts=[], max_frames=4, overlap=4), dict(t=10, starts=[], max_frames=4, overlap=5),
                                    dict(t=0, starts=[]), dict(t=10, starts=[0]), dict(t=10, starts=[10]), dict(t=10, starts=[-1]),
                                    dict(t=10, starts=[3, 12]), dict(t=10, starts=[], overlap=-1)])
def test_plan_segments_refuses(kwargs):
    with pytest.raises(ValueError):
        S.plan_segments(**kwargs)


def test_check_plan():
    plan = S.plan_segments(11, [], 5, 2)
    assert S.check_plan(11, plan) == plan
    for bad in ([(0, 5, 0, 4), (3, 8, 5, 7), (6, 11, 7, 11)],      # frame 4 never emitted
                [(0, 5, 0, 4), (3, 8, 4, 7)],                      # stops early
                [(0, 5, 0, 6), (5, 11, 6, 11)],                    # emits outside its window
                [(0, 12, 0, 12)], [(0, 11, 0)]):
        with pytest.raises(ValueError):
            S.check_plan(11, bad)


def _stats(pairs, pixels=1000):
    """hist / sad of frames whose consecutive histogram distances and mean SADs are `pairs` = [(moved pixels, sad)]"""
    hist = [[pixels] + [0] * 63]
    for moved, _ in pairs:
        row = [0] * 64
        # alternate which pair of bins holds the pixels, so that `moved` pixels change bin against the previous frame
        prev = hist[-1]
        home = prev.index(max(prev))
        row[home] = pixels - moved
        row[(home + 7) % 64] = moved
        hist.append(row)
    return hist, [s for _, s in pairs]


def test_find_cuts_needs_both_criteria_and_is_inclusive():
    pixels = 1000
    # pair 0: histogram only (a brightness change); pair 1: SAD only (translation); pair 2: both; pair 3: neither
    hist, sad = _stats([(600, 100), (0, 50000), (600, 50000), (10, 10)], pixels)
    assert S.find_cuts(hist, sad, pixels, 0.5, 10.0) == [3]
    assert S.find_cuts(hist, sad, pixels, 0.0, 0.0) == [1, 2, 3, 4]
    # exactly at the thresholds: 500 moved pixels = distance 0.5, SAD 10000 = mean 10.0
    hist, sad = _stats([(500, 10000), (499, 10000), (500, 9999)], pixels)
    assert S.find_cuts(hist, sad, pixels, 0.5, 10.0) == [1]
    # numpy arrays and empty sad
    assert S.find_cuts(np.array(hist, dtype=np.int32), np.array(sad, dtype=np.int64), pixels, 0.5, 10.0) == [1]
    assert S.find_cuts([[pixels] + [0] * 63], [], pixels, 0.0, 0.0) == []
    assert S.find_cuts(np.zeros((1, 64), np.int32), np.zeros((0,), np.int64), pixels) == []
    with pytest.raises(ValueError):
        S.find_cuts(hist, sad[:-1], pixels, 0.5, 10.0)
    assert isinstance(S.DEFAULT_HIST_THRESHOLD, float) and isinstance(S.DEFAULT_SAD_THRESHOLD, float) and S.DEFAULT_OVERLAP == 8


def test_segment_options(monkeypatch):
    for name in ("EAVSR_MAX_FRAMES", "EAVSR_SEGMENT_OVERLAP", "EAVSR_SCENE_CUTS"):
        monkeypatch.delenv(name, raising=False)
    # nothing set: every argument of super_resolve stays at today's value
    assert S.segment_options(None) == (None, None, None) and S.segment_options(Namespace()) == (None, None, None)
    assert S.segment_options(Namespace(max_frames=None, segment_overlap=None, scene_cuts=None)) == (None, None, None)
    assert S.segment_options(Namespace(max_frames=20, segment_overlap=4, scene_cuts="device")) == (20, 4, "device")
    assert S.segment_options(Namespace(max_frames=20, segment_overlap=0)) == (20, 0, None)
    monkeypatch.setenv("EAVSR_MAX_FRAMES", "30")
    monkeypatch.setenv("EAVSR_SEGMENT_OVERLAP", "6")
    monkeypatch.setenv("EAVSR_SCENE_CUTS", "device")
    assert S.segment_options(None) == (30, 6, "device")
    assert S.segment_options(Namespace(max_frames=12, segment_overlap=2)) == (12, 2, "device")      # the options win
    for name, bad in (("EAVSR_MAX_FRAMES", "0"), ("EAVSR_MAX_FRAMES", "x"), ("EAVSR_SEGMENT_OVERLAP", "-1"), ("EAVSR_SCENE_CUTS", "host")):
        with monkeypatch.context() as m:
            m.setenv(name, bad)
            with pytest.raises(ValueError):
                S.segment_options(None)
    for bad in (Namespace(max_frames=0), Namespace(max_frames=True), Namespace(max_frames=2.5), Namespace(segment_overlap=-1),
                Namespace(scene_cuts="host"), Namespace(scene_cuts=True)):
        with pytest.raises(ValueError):
            S.segment_options(bad)
    # validated with the other long-clip options when a model wrapper reads them
    from eavsr_amd.eavsrp_model import long_clip_options
    with pytest.raises(ValueError):
        long_clip_options(Namespace(max_frames=0))


def test_super_resolve_signature_defaults_are_todays_path():
    import inspect
    from eavsr_amd import harness
    from eavsr_amd.eavsrp_model import EAVSRP
    p = inspect.signature(harness.super_resolve).parameters
    assert p["max_frames"].default is None and p["cuts"].default is None and p["cut_thresholds"].default is None
    assert p["overlap"].default == 8 and p["min_scene"].default == 2
    assert inspect.signature(EAVSRP.forward_long).parameters["emit"].default is None
    assert list(inspect.signature(EAVSRP.forward_segments).parameters)[1:] == ["lrs", "segments", "frame_chunk", "cache", "sink"]


def test_entry_point_is_declared_without_an_abi_bump():
    from eavsr_amd import _native
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    assert re.search(r"^int eavsr_frame_change_u8\(const uint8_t\* in, int32_t\* hist, int64_t\* sad,", header, flags=re.M)
    assert "eavsr_frame_change_u8" in _native.SIGNATURES
    assert re.search(r"#define\s+EAVSR_ABI_VERSION\s+32\b", header)


def test_frame_change_refuses_what_u8_to_f32_refuses():
    import torch
    from eavsr_amd import ops
    with pytest.raises(TypeError):
        ops.frame_change(np.zeros((2, 3, 8, 8), np.uint8))
    with pytest.raises(RuntimeError):
        ops.frame_change(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))      # a host tensor


def test_oracle_on_a_hand_computed_case():
    from tests import scene_ref as R
    planar = np.zeros((2, 3, 1, 2), np.uint8)
    planar[0, :, 0, 0] = (255, 255, 255)      # (77 + 150 + 29) 255 + 128 >> 8 = 255
    planar[0, :, 0, 1] = (10, 20, 30)         # 770 + 3000 + 870 + 128 = 4768 >> 8 = 18
    planar[1, :, 0, 0] = (0, 0, 1)            # 29 + 128 >> 8 = 0
    planar[1, :, 0, 1] = (255, 0, 0)          # 19635 + 128 >> 8 = 77
    hist, sad = R.frame_change(planar)
    assert hist.dtype == np.int32 and sad.dtype == np.int64 and hist.shape == (2, 64) and sad.shape == (1,)
    assert hist[0, 63] == 1 and hist[0, 4] == 1 and hist[1, 0] == 1 and hist[1, 19] == 1 and hist.sum() == 4
    assert sad[0] == 255 + (77 - 18)
    hist2, sad2 = R.frame_change(np.ascontiguousarray(np.moveaxis(planar, 1, 3)), hwc=True)
    assert np.array_equal(hist, hist2) and np.array_equal(sad, sad2)
    grey = np.array([[[[0, 3, 4, 255]]], [[[255, 3, 0, 255]]]], np.uint8)
    hist, sad = R.frame_change(grey)
    assert hist[0].tolist()[:2] == [2, 1] and hist[0, 63] == 1 and sad.tolist() == [259]


# ------------------------------------------------------------------------------------------------------------- every option reader
_ENV_NAMES = ("EAVSR_FRAME_CHUNK", "EAVSR_CPU_CACHE", "EAVSR_PNG_ENCODER", "EAVSR_PNG_DECODER", "EAVSR_MAX_FRAMES",
              "EAVSR_SEGMENT_OVERLAP", "EAVSR_SCENE_CUTS", "EAVSR_PAD_FRAMES", "EAVSR_TILE", "EAVSR_TILE_OVERLAP")


def _readers():
    from eavsr_amd import eavsrp_model as M
    return {"long": M.long_clip_options, "enc": M.png_encoder_option, "dec": M.png_decoder_option, "seg": S.segment_options,
            "pad": S.pad_option, "tile": S.tile_options}


# (reader, opt fields, environment, what it returns -- or the ValueError's text): written down from the readers as they stood before
# they shared `segments.read_option`; opt.<name> where it is not None, else the variable where it is set and not empty, else the default
_OPTION_TABLE = [
    ("long", {}, {}, (None, False)),
    ("long", {"frame_chunk": 3, "cpu_cache": True}, {"EAVSR_FRAME_CHUNK": "x", "EAVSR_CPU_CACHE": "x"}, (3, True)),
    ("long", {"frame_chunk": 0, "cpu_cache": False}, {"EAVSR_FRAME_CHUNK": "5", "EAVSR_CPU_CACHE": "1"}, (None, False)),
    ("long", {"frame_chunk": None, "cpu_cache": None}, {"EAVSR_FRAME_CHUNK": "5", "EAVSR_CPU_CACHE": "1"}, (5, True)),
    ("long", {}, {"EAVSR_FRAME_CHUNK": "", "EAVSR_CPU_CACHE": "0"}, (None, False)),
    ("long", {}, {"EAVSR_FRAME_CHUNK": "0"}, "EAVSR_FRAME_CHUNK='0': a positive number of frames"),
    ("long", {}, {"EAVSR_FRAME_CHUNK": "-2"}, "EAVSR_FRAME_CHUNK='-2': a positive number of frames"),
    ("long", {}, {"EAVSR_FRAME_CHUNK": "2.0"}, "EAVSR_FRAME_CHUNK='2.0': a positive number of frames"),
    ("long", {"frame_chunk": -1}, {}, "opt.frame_chunk=-1: a positive number of frames, or None"),
    ("long", {"frame_chunk": True}, {}, "opt.frame_chunk=True: a positive number of frames, or None"),
    ("long", {"frame_chunk": "4"}, {}, "opt.frame_chunk='4': a positive number of frames, or None"),
    ("long", {}, {"EAVSR_CPU_CACHE": "yes"}, "EAVSR_CPU_CACHE='yes': 0 or 1"),
    ("long", {}, {"EAVSR_CPU_CACHE": ""}, "EAVSR_CPU_CACHE='': 0 or 1"),      # the one variable that may not be empty
    ("long", {"cpu_cache": 1}, {}, "opt.cpu_cache=1: True or False"),
    ("long", {"cpu_cache": "1"}, {}, "opt.cpu_cache='1': True or False"),
    ("long", {}, {"EAVSR_PNG_ENCODER": "gpu"}, "EAVSR_PNG_ENCODER='gpu': host or device"),      # validated with the others
    ("long", {"png_decoder": "gpu"}, {}, "opt.png_decoder='gpu': 'host' or 'device'"),
    ("long", {}, {"EAVSR_MAX_FRAMES": "0"}, "EAVSR_MAX_FRAMES='0': a positive number of frames"),
    ("enc", {}, {}, "host"),
    ("enc", {}, {"EAVSR_PNG_ENCODER": ""}, "host"),
    ("enc", {}, {"EAVSR_PNG_ENCODER": "device"}, "device"),
    ("enc", {"png_encoder": "host"}, {"EAVSR_PNG_ENCODER": "device"}, "host"),
    ("enc", {"png_encoder": "device"}, {"EAVSR_PNG_ENCODER": "gpu"}, "device"),
    ("enc", {"png_encoder": None}, {"EAVSR_PNG_ENCODER": "gpu"}, "EAVSR_PNG_ENCODER='gpu': host or device"),
    ("enc", {"png_encoder": "Device"}, {}, "opt.png_encoder='Device': 'host' or 'device'"),
    ("enc", {"png_encoder": True}, {}, "opt.png_encoder=True: 'host' or 'device'"),
    ("dec", {}, {}, "host"),
    ("dec", {}, {"EAVSR_PNG_DECODER": "device", "EAVSR_PNG_ENCODER": "gpu"}, "device"),
    ("dec", {"png_decoder": "host"}, {"EAVSR_PNG_DECODER": "device"}, "host"),
    ("dec", {}, {"EAVSR_PNG_DECODER": "0"}, "EAVSR_PNG_DECODER='0': host or device"),
    ("dec", {"png_decoder": ""}, {}, "opt.png_decoder='': 'host' or 'device'"),
    ("seg", {}, {}, (None, None, None)),
    ("seg", {"max_frames": 40, "segment_overlap": 0, "scene_cuts": "device"}, {}, (40, 0, "device")),
    ("seg", {}, {"EAVSR_MAX_FRAMES": "30", "EAVSR_SEGMENT_OVERLAP": "4", "EAVSR_SCENE_CUTS": "device"}, (30, 4, "device")),
    ("seg", {"max_frames": 12}, {"EAVSR_MAX_FRAMES": "x", "EAVSR_SEGMENT_OVERLAP": "", "EAVSR_SCENE_CUTS": ""}, (12, None, None)),
    ("seg", {"max_frames": 0}, {}, "opt.max_frames=0: a positive number of frames, or None"),
    ("seg", {"max_frames": 2.0}, {}, "opt.max_frames=2.0: a positive number of frames, or None"),
    ("seg", {"segment_overlap": -1}, {}, "opt.segment_overlap=-1: a number of frames, 0 or more, or None"),
    ("seg", {"segment_overlap": False}, {}, "opt.segment_overlap=False: a number of frames, 0 or more, or None"),
    ("seg", {}, {"EAVSR_SEGMENT_OVERLAP": "-1"}, "EAVSR_SEGMENT_OVERLAP='-1': a number of frames, 0 or more"),
    ("seg", {}, {"EAVSR_SCENE_CUTS": "host"}, "EAVSR_SCENE_CUTS='host': device (or unset)"),
    ("seg", {"scene_cuts": "host"}, {}, "opt.scene_cuts='host': 'device' or None"),
    ("seg", {"scene_cuts": [3]}, {}, "opt.scene_cuts=[3]: 'device' or None"),
    ("pad", {}, {}, None),
    ("pad", {}, {"EAVSR_PAD_FRAMES": "edge"}, "edge"),
    ("pad", {"pad_frames": "reflect"}, {"EAVSR_PAD_FRAMES": "wrap"}, "reflect"),
    ("pad", {}, {"EAVSR_PAD_FRAMES": "wrap"}, "EAVSR_PAD_FRAMES='wrap': 'reflect', 'edge' or None"),
    ("pad", {"pad_frames": ""}, {}, "opt.pad_frames='': 'reflect', 'edge' or None"),
    ("pad", {"pad_frames": 1}, {}, "opt.pad_frames=1: 'reflect', 'edge' or None"),
    ("tile", {}, {}, (None, None)),
    ("tile", {"tile": 128, "tile_overlap": 0}, {"EAVSR_TILE": "x", "EAVSR_TILE_OVERLAP": "x"}, ((128, 128), 0)),
    ("tile", {"tile": "288x512"}, {"EAVSR_TILE_OVERLAP": "8"}, ((288, 512), 8)),
    ("tile", {"tile": [64, 128]}, {}, ((64, 128), None)),
    ("tile", {}, {"EAVSR_TILE": "512", "EAVSR_TILE_OVERLAP": ""}, ((512, 512), None)),
    ("tile", {}, {"EAVSR_TILE": "64x"}, "EAVSR_TILE='64x': LR pixels as '512' or '288x512' (rows x columns)"),
    ("tile", {}, {"EAVSR_TILE": "66"}, "EAVSR_TILE=66: a tile side is a multiple of 4 and at least 64 (what the network takes)"),
    ("tile", {"tile": "a"}, {}, "opt.tile='a': LR pixels as '512' or '288x512' (rows x columns)"),
    ("tile", {"tile": 64.0}, {}, "opt.tile=64.0: a number of LR pixels or (rows, columns), or None"),
    ("tile", {"tile": (64, 32)}, {}, "opt.tile=(64, 32): a tile side is a multiple of 4 and at least 64 (what the network takes)"),
    ("tile", {"tile_overlap": "8"}, {}, "opt.tile_overlap='8': a number of LR pixels, 0 or more, or None"),
    ("tile", {}, {"EAVSR_TILE_OVERLAP": "1.5"}, "EAVSR_TILE_OVERLAP='1.5': a number of LR pixels, 0 or more"),
]


def test_every_option_reader_returns_what_it_returned_before_they_shared_one_helper(monkeypatch):
    readers = _readers()
    for reader, fields, env, want in _OPTION_TABLE:
        for name in _ENV_NAMES:
            monkeypatch.delenv(name, raising=False)
        for name, value in env.items():
            monkeypatch.setenv(name, value)
        for opt in ([Namespace(**fields)] if fields else [None, Namespace()]):
            if isinstance(want, str) and ("=" in want):
                with pytest.raises(ValueError) as e:
                    readers[reader](opt)
                assert str(e.value) == want, (reader, fields, env)
            else:
                assert readers[reader](opt) == want, (reader, fields, env)
