"""Videos of any length: where a scene is cut, and which windows of it `EAVSRP.forward_segments` runs.

Pure host logic, no device: `find_cuts` turns the statistics of `ops.frame_change` into scene starts, `plan_segments` turns scene
starts and a bound on a window's length into (start, stop, emit_start, emit_stop) windows, `segment_options` reads the opt-in
settings the way `eavsrp_model.long_clip_options` reads its own.  And frames of any size: `padded_size`, `pad_index` and
`pad_option` at the end of the file.

The thresholds below are SETTINGS, not measurements: nobody has validated them on real footage (no real clips and no trained
weights exist in this project).  A cut is a hard cut between two consecutive frames; fades and dissolves change neither
statistic enough between any two frames and are not detected.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

# a new scene starts where BOTH hold between two consecutive frames: half the L1 distance of the 64-bin luma histograms, as a
# fraction of the pixels (0 = the same distribution, 1 = disjoint), and the mean absolute luma difference in 8-bit levels
DEFAULT_HIST_THRESHOLD = 0.35
DEFAULT_SAD_THRESHOLD = 12.0
# frames two neighbouring windows share (harness.super_resolve's default): a setting, not a measured optimum
DEFAULT_OVERLAP = 8
# the shortest clip `EAVSRP.forward_long` / `_propagate_long` take is ONE frame (no frame pair: SPyNet is skipped, every branch runs
# its first step only), so that is min_scene's lower bound; the default of 2 keeps a frame from being restored without a neighbour
MIN_SCENE_FLOOR = 1

Segment = Tuple[int, int, int, int]


def find_cuts(hist, sad, pixels: int, hist_threshold: float = DEFAULT_HIST_THRESHOLD,
              sad_threshold: float = DEFAULT_SAD_THRESHOLD) -> List[int]:
    """Scene starts (sorted frame indices > 0) from `ops.frame_change`'s statistics of one clip: hist (F, 64) and sad (F - 1,) --
    tensors, arrays or nested lists of integers -- and the pixels per frame.  A scene starts at f + 1 iff both
        sum_b |hist[f][b] - hist[f + 1][b]| / (2 pixels) >= hist_threshold    and    sad[f] / pixels >= sad_threshold.
    Two criteria because translating content has a large SAD under an unchanged histogram, a brightness change the opposite.
    Evaluated in Python integers / float64 on the host: F - 1 comparisons."""
    hist = hist.tolist() if hasattr(hist, "tolist") else [list(r) for r in hist]
    sad = sad.tolist() if hasattr(sad, "tolist") else list(sad)
    pixels = int(pixels)
    if pixels < 1:
        raise ValueError(f"find_cuts: pixels {pixels!r}: at least 1")
    if len(hist) != len(sad) + 1:
        raise ValueError(f"find_cuts: {len(hist)} histograms and {len(sad)} differences: F and F - 1")
    cuts = []
    for f in range(len(sad)):
        d = sum(abs(int(a) - int(b)) for a, b in zip(hist[f], hist[f + 1]))
        if d / (2.0 * pixels) >= hist_threshold and int(sad[f]) / float(pixels) >= sad_threshold:
            cuts.append(f + 1)
    return cuts


def keep_starts(t: int, starts: Sequence[int], min_scene: int = 2) -> List[int]:
    """The scene starts that survive the merge of short scenes: walking `starts` in increasing order, a start is kept only if it lies
    at least `min_scene` after the last kept one (0 is implicit) and at most at t - min_scene; a scene that would be shorter joins
    its predecessor."""
    t, min_scene = int(t), int(min_scene)
    if t < 1:
        raise ValueError(f"plan_segments: t {t!r}: at least one frame")
    if min_scene < MIN_SCENE_FLOOR:
        raise ValueError(f"plan_segments: min_scene {min_scene!r}: at least {MIN_SCENE_FLOOR} (the shortest clip forward_long takes)")
    starts = sorted(int(s) for s in starts)
    for s in starts:
        if not 0 < s < t:
            raise ValueError(f"plan_segments: scene start {s} outside (0, {t})")
    kept, last = [], 0
    for s in starts:
        if s - last >= min_scene and s <= t - min_scene:
            kept.append(s)
            last = s
    return kept


def plan_segments(t: int, starts: Sequence[int], max_frames: Optional[int] = None, overlap: int = 0,
                  min_scene: int = 2) -> List[Segment]:
    """(start, stop, emit_start, emit_stop) windows of a clip of t frames with scenes starting at `starts`: `forward_long` runs on
    frames [start, stop) and frames [emit_start, emit_stop) of its result are kept.  The emit ranges partition [0, t) in order.

    Scenes shorter than `min_scene` are merged first (`keep_starts`).  A scene [s, e) no longer than `max_frames` (or any scene when
    max_frames is None) is one window that emits itself.  A longer one is cut into windows of exactly max_frames frames that start
    at s + k (max_frames - overlap) while s + k (max_frames - overlap) + max_frames < e, and a last window [e - max_frames, e) --
    shifted back to full length, not left short.  Two consecutive windows [a0, a1), [b0, b1) share [b0, a1): the first emits up to
    m = (b0 + a1) // 2, the second from m, so every emitted frame lies at least overlap // 2 frames inside any window end that
    is not a scene end."""
    kept = keep_starts(t, starts, min_scene)
    t = int(t)
    if max_frames is not None:
        max_frames = int(max_frames)
        if max_frames < 1:
            raise ValueError(f"plan_segments: max_frames {max_frames!r}: at least 1, or None")
    overlap = int(overlap)
    if overlap < 0:
        raise ValueError(f"plan_segments: overlap {overlap!r}: not negative")
    if max_frames is not None and overlap >= max_frames:
        raise ValueError(f"plan_segments: overlap {overlap} must be smaller than max_frames {max_frames}")
    plan: List[Segment] = []
    bounds = [0] + kept + [t]
    for s, e in zip(bounds[:-1], bounds[1:]):
        if max_frames is None or e - s <= max_frames:
            plan.append((s, e, s, e))
            continue
        stride = max_frames - overlap
        windows = []
        a = s
        while a + max_frames < e:
            windows.append((a, a + max_frames))
            a += stride
        windows.append((e - max_frames, e))
        emit_from = s
        for k, (a0, a1) in enumerate(windows):
            emit_to = e if k + 1 == len(windows) else (windows[k + 1][0] + a1) // 2
            plan.append((a0, a1, emit_from, emit_to))
            emit_from = emit_to
    return plan


def check_plan(t: int, segments: Sequence[Segment]) -> List[Segment]:
    """a plan as `forward_segments` takes it: windows inside [0, t) whose emit ranges lie inside them and partition [0, t) in order"""
    plan = [tuple(int(v) for v in seg) for seg in segments]
    at = 0
    for seg in plan:
        if len(seg) != 4:
            raise ValueError(f"segments: (start, stop, emit_start, emit_stop) tuples, got {seg!r}")
        a, b, ea, eb = seg
        if not (0 <= a <= ea < eb <= b <= t) or ea != at:
            raise ValueError(f"segments: {seg!r} after frame {at} of {t}: emit ranges partition [0, t) in order, inside their windows")
        at = eb
    if at != t:
        raise ValueError(f"segments: the plan emits {at} of {t} frames")
    return plan


def read_option(opt, name: str, env_name: str, from_opt, from_env, default=None, empty_is_unset: bool = True):
    """One opt-in setting, as every reader of this package finds it: `opt.<name>` where the options carry it (anything but None),
    else the environment variable `env_name` where it is set (and not empty, unless `empty_is_unset` is False), else `default`.
    `from_opt(value, "opt.<name>")` / `from_env(text, env_name)` return the setting or raise the ValueError that refuses it, which
    opens with `<who>=<value>: `; a bad environment is therefore not read where the options decide."""
    value = getattr(opt, name, None)
    if value is not None:
        return from_opt(value, f"opt.{name}")
    env = os.environ.get(env_name)
    if env is None or (env == "" and empty_is_unset):
        return default
    return from_env(env, env_name)


def one_of(choices, what: str):
    """a `read_option` check: the value itself where it is among `choices`, else `<who>=<value>: <what>`"""
    def check(value, who):
        if value not in choices:
            raise ValueError(f"{who}={value!r}: {what}")
        return value
    return check


def whole_number(least: int, what: str):
    """a `read_option` check for `opt.<name>`: an int (no bool) >= least"""
    def check(value, who):
        if isinstance(value, bool) or not isinstance(value, int) or value < least:
            raise ValueError(f"{who}={value!r}: {what}")
        return value
    return check


def digits(least: int, what: str):
    """a `read_option` check for an environment variable: decimal digits, as an int >= least"""
    def check(text, who):
        if not text.isdigit() or int(text) < least:
            raise ValueError(f"{who}={text!r}: {what}")
        return int(text)
    return check


def _count(opt, name: str, env_name: str, least: int, what: str) -> Optional[int]:
    return read_option(opt, name, env_name, whole_number(least, what + ", or None"), digits(least, what))


def segment_options(opt=None):
    """(max_frames, overlap, cuts) of the opt-in segmented path, each None where nothing sets it (`harness.super_resolve` then keeps
    its own default -- with all three None today's one `forward_long` call): `opt.max_frames` (frames per window), `opt.segment_overlap`
    (frames two windows share), `opt.scene_cuts` ("device": detect cuts on the 8-bit frames), each falling back to the environment
    where the options do not carry it -- EAVSR_MAX_FRAMES=<positive integer>, EAVSR_SEGMENT_OVERLAP=<integer >= 0>,
    EAVSR_SCENE_CUTS=device.  None is among the reference's options."""
    mf = _count(opt, "max_frames", "EAVSR_MAX_FRAMES", 1, "a positive number of frames")
    ov = _count(opt, "segment_overlap", "EAVSR_SEGMENT_OVERLAP", 0, "a number of frames, 0 or more")
    sc = read_option(opt, "scene_cuts", "EAVSR_SCENE_CUTS", one_of(("device",), "'device' or None"), one_of(("device",), "device (or unset)"))
    return mf, ov, sc


# -- frames of any size: what `ops.ingest_pad` pads to, and which source sample a padded sample repeats ------------------
PAD_MODES = ("reflect", "edge")      # the order is the C entry point's `mode` argument
MIN_SIDE = 64                        # `EAVSRP.forward` asserts h, w >= 64 (SPyNet's six-level pyramid)
SIDE_MULTIPLE = 4                    # `ops.pyramid` halves the features twice


def padded_size(h: int, w: int) -> Tuple[int, int]:
    """(H, W) the network takes for frames of h x w: each side rounded up to a multiple of 4, and to 64 where it is smaller"""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"padded_size: frames of {h} x {w}")
    up = lambda v: max(MIN_SIDE, SIDE_MULTIPLE * ((v + SIDE_MULTIPLE - 1) // SIDE_MULTIPLE))
    return up(h), up(w)


def pad_index(i: int, s: int, mode: str = "reflect") -> int:
    """The source index, in [0, s), that index i >= 0 of a padded axis repeats (`ops.ingest_pad`, csrc/ingest_pad.hip `src_index`).
    "reflect": the triangle wave m = i mod 2 (s - 1), r = m if m < s else 2 (s - 1) - m, and 0 for s = 1 -- np.pad(mode="reflect")
    for every pad width, pads several times the axis included.  "edge": min(i, s - 1)."""
    i, s = int(i), int(s)
    if i < 0 or s < 1:
        raise ValueError(f"pad_index: index {i} of an axis of {s}")
    if mode not in PAD_MODES:
        raise ValueError(f"pad_index: mode {mode!r}: one of {PAD_MODES}")
    if i < s:
        return i
    if mode == "edge" or s == 1:
        return s - 1
    period = 2 * (s - 1)
    m = i % period
    return m if m < s else period - m


def check_pad(pad, what: str = "pad") -> Optional[str]:
    """None, "reflect" or "edge"; anything else is a ValueError that names `what`"""
    if pad is not None and pad not in PAD_MODES:
        raise ValueError(f"{what}={pad!r}: 'reflect', 'edge' or None")
    return pad


def pad_option(opt=None) -> Optional[str]:
    """`opt.pad_frames` ("reflect" / "edge": frames of any size are padded on the device and the output is cropped), falling back to
    the environment where the options do not carry it (EAVSR_PAD_FRAMES=reflect|edge), None -- off -- where neither does.  Not
    among the reference's options."""
    return read_option(opt, "pad_frames", "EAVSR_PAD_FRAMES", check_pad, check_pad)


# -- frames of any resolution: which spatial windows `EAVSRP.forward_tiled` runs, and how their SR tiles are blended -----
DEFAULT_TILE_OVERLAP = 32            # LR pixels two neighbouring tiles share: a setting, not a measured optimum

Tile = Tuple[int, int, int, int]


def check_tile(tile, what: str = "tile") -> Optional[Tuple[int, int]]:
    """None, or (th, tw) from an int (a square tile) or a pair: every side a multiple of 4 and at least 64 -- the model's own limit
    for the frames it takes (`padded_size`); anything else is a ValueError that names `what`"""
    if tile is None:
        return None
    sides = (tile, tile) if isinstance(tile, int) else tuple(tile) if isinstance(tile, (tuple, list)) else None
    if sides is None or len(sides) != 2 or any(isinstance(v, bool) or not isinstance(v, int) for v in sides):
        raise ValueError(f"{what}={tile!r}: a number of LR pixels or (rows, columns), or None")
    for v in sides:
        if v < MIN_SIDE or v % SIDE_MULTIPLE:
            raise ValueError(f"{what}={tile!r}: a tile side is a multiple of {SIDE_MULTIPLE} and at least {MIN_SIDE} (what the network takes)")
    return sides


def tile_axis(size: int, tile: int, overlap: int) -> List[Tuple[int, int]]:
    """[a, b) windows of one axis of `size` samples, `plan_segments`' rule in space: an axis no longer than `tile` is one window, the
    whole axis; a longer one gets windows of exactly `tile` samples that start at k (tile - overlap) while start + tile < size, and a
    last window [size - tile, size) -- shifted back to full length, not left short"""
    size, tile, overlap = int(size), int(tile), int(overlap)
    if size < 1:
        raise ValueError(f"plan_tiles: an axis of {size} samples")
    if overlap < 0:
        raise ValueError(f"plan_tiles: overlap {overlap!r}: not negative")
    if overlap > tile // 2:
        raise ValueError(f"plan_tiles: overlap {overlap} must be at most half the tile side {tile}")
    if size <= tile:
        return [(0, size)]
    windows, a = [], 0
    while a + tile < size:
        windows.append((a, a + tile))
        a += tile - overlap
    windows.append((size - tile, size))
    return windows


def plan_tiles(h: int, w: int, tile, overlap: int = DEFAULT_TILE_OVERLAP) -> List[Tile]:
    """(y0, y1, x0, x1) LR windows of frames of h x w in row-major order, `tile_axis` on either axis: all windows of a plan have the
    same size -- min(tile, size) per axis -- so every tile takes the same kernel routes.  Refused with a ValueError before anything
    runs: a tile side that is no multiple of 4 or below 64, overlap < 0, overlap > tile // 2 on either axis."""
    sides = check_tile(tile, "plan_tiles: tile")
    if sides is None:
        raise ValueError("plan_tiles: tile=None")
    if isinstance(overlap, bool) or not isinstance(overlap, int):
        raise ValueError(f"plan_tiles: overlap {overlap!r}: a number of LR pixels")
    for side in sides:      # both axes are checked, also where the frame is smaller than the tile
        tile_axis(1, side, overlap)
    rows, cols = tile_axis(h, sides[0], overlap), tile_axis(w, sides[1], overlap)
    return [(y0, y1, x0, x1) for y0, y1 in rows for x0, x1 in cols]


def tile_weights(size: int, windows_1d: Sequence[Tuple[int, int]], scale: int):
    """float32 numpy (k, scale * tile_len): one row of SR-resolution blending weights per window [a, b) of one axis of `size` LR
    samples (`tile_axis`; all of one length).  For SR sample X in [s a, s b) the raw weight is min(dl, dr) with
    dl = X - s a + 0.5 if a > 0 else inf, dr = s b - X - 0.5 if b < size else inf -- the distance to the nearest window edge that is
    not a frame edge -- and 1 where both are inf; the weight is the raw weight over the sum of the raw weights of all windows that
    cover X: a partition of unity, a linear ramp across the overlap of two neighbours, exactly 1.0 where one window covers X.
    Computed in float64 and rounded once."""
    import numpy as np
    size, s = int(size), int(scale)
    windows = [(int(a), int(b)) for a, b in windows_1d]
    if s < 1 or not windows or any(not 0 <= a < b <= size for a, b in windows) or len({b - a for a, b in windows}) != 1:
        raise ValueError(f"tile_weights: windows {windows!r} of one length inside [0, {size}), scale {scale!r}")
    total = np.zeros(s * size, np.float64)
    raws = []
    for a, b in windows:
        X = np.arange(s * a, s * b, dtype=np.float64)
        dl = X - s * a + 0.5 if a > 0 else np.full(X.shape, np.inf)
        dr = s * b - X - 0.5 if b < size else np.full(X.shape, np.inf)
        raw = np.minimum(dl, dr)
        raw[np.isinf(raw)] = 1.0
        total[s * a:s * b] += raw
        raws.append(raw)
    if not (total > 0).all():
        raise ValueError(f"tile_weights: windows {windows!r} do not cover [0, {size})")
    return np.stack([raw / total[s * a:s * b] for raw, (a, b) in zip(raws, windows)], 0).astype(np.float32)


def parse_tile(text: str, what: str) -> Tuple[int, int]:
    """"512" or "288x512" (rows x columns) -> (th, tw), checked as `check_tile`"""
    parts = text.split("x")
    if len(parts) not in (1, 2) or not all(p.isdigit() for p in parts):
        raise ValueError(f"{what}={text!r}: LR pixels as '512' or '288x512' (rows x columns)")
    sides = [int(p) for p in parts]
    return check_tile(sides[0] if len(sides) == 1 else tuple(sides), what)


def tile_options(opt=None):
    """(tile, overlap) of the opt-in tiled path, each None where nothing sets it: `opt.tile` -- an int, (rows, columns) or
    the text form "512" / "288x512" -- and `opt.tile_overlap` (LR pixels two tiles share; `harness.super_resolve` and the model
    wrapper take DEFAULT_TILE_OVERLAP = 32 where it is None: a setting, not a measured optimum), each falling back to the environment
    where the options do not carry it: EAVSR_TILE=512|288x512, EAVSR_TILE_OVERLAP=<integer >= 0>.  tile is returned as (th, tw).
    Neither is among the reference's options."""
    tile = read_option(opt, "tile", "EAVSR_TILE", lambda v, who: parse_tile(v, who) if isinstance(v, str) else check_tile(v, who), parse_tile)
    ov = _count(opt, "tile_overlap", "EAVSR_TILE_OVERLAP", 0, "a number of LR pixels, 0 or more")
    return tile, ov


# -- self-ensemble inference: which of the eight flips / transposes `EAVSRP.forward_ensemble` averages ----------------------
ENSEMBLE_MODES = 8                   # mode k: bit 0 hflip, bit 1 vflip, bit 2 transpose, in that order (the flags of `dataset.py`)
ENSEMBLE_NAMED = {1: (0,), 2: (0, 1), 4: (0, 1, 2, 3), "flips": (0, 1, 2, 3), 8: tuple(range(8))}


def check_ensemble(spec, what: str = "ensemble") -> Optional[Tuple[int, ...]]:
    """The ensemble spec as a tuple of distinct modes in increasing order, or None (off): None and 1 are off; 2 is modes (0, 1); 4
    and "flips" are (0, 1, 2, 3); 8 is all eight; a non-empty sequence of distinct modes 0 .. 7 is itself, sorted.  Anything else
    is a ValueError that names `what`."""
    if spec is None:
        return None
    if isinstance(spec, (int, str)) and not isinstance(spec, bool):
        if spec in ENSEMBLE_NAMED:
            return None if spec == 1 else ENSEMBLE_NAMED[spec]
    elif isinstance(spec, (tuple, list)) and spec:
        modes = tuple(spec)
        if (all(isinstance(k, int) and not isinstance(k, bool) and 0 <= k < ENSEMBLE_MODES for k in modes)
                and len(set(modes)) == len(modes)):
            return tuple(sorted(modes))
    raise ValueError(f"{what}={spec!r}: None, 1 (off), 2, 4, 'flips', 8, or distinct modes 0 .. 7 (bit 0 hflip, bit 1 vflip, "
                     f"bit 2 transpose)")


def parse_ensemble(text: str, what: str) -> Optional[Tuple[int, ...]]:
    """"8", "4", "2", "1", "flips", or a list of modes as "0,1,4" -> `check_ensemble`'s tuple"""
    if text == "flips":
        return check_ensemble(text, what)
    parts = text.split(",")
    if not all(p.isdigit() for p in parts):
        raise ValueError(f"{what}={text!r}: 1, 2, 4, 8, flips, or modes as '0,1,4'")
    if len(parts) == 1:
        value = int(parts[0])
        return check_ensemble(value if value in ENSEMBLE_NAMED else (value,), what)
    return check_ensemble(tuple(int(p) for p in parts), what)


def ensemble_options(opt=None) -> Optional[Tuple[int, ...]]:
    """The modes of the opt-in self-ensemble, None where nothing sets it or it is off: `opt.ensemble` -- anything
    `check_ensemble` takes, or the text form -- falling back to the environment where the options do not carry it:
    EAVSR_ENSEMBLE=8|4|2|1|flips|0,1,4.  Not among the reference's options."""
    return read_option(opt, "ensemble", "EAVSR_ENSEMBLE",
                       lambda v, who: parse_ensemble(v, who) if isinstance(v, str) else check_ensemble(v, who), parse_ensemble)


def ensemble_weight(modes) -> "np.float32":
    """np.float32(1) / np.float32(len(modes)): exact for 2, 4 and 8 modes"""
    import numpy as np
    return np.float32(1) / np.float32(len(modes))


def valid_region(k: int, h: int, w: int, H: int, W: int, scale: int) -> Tuple[int, int, int, int]:
    """(r0, r1, c0, c1): where the SR samples of the h x w frame lie inside the SR frame of mode k, when the frame was padded at the
    bottom and right to H x W and THEN transformed -- g_k's image of [0, s h) x [0, s w).  A flip moves the padding to the top /
    left; a transposed mode swaps the axes (its SR frame is s W x s H)."""
    k, s = int(k), int(scale)
    if not 0 <= k < ENSEMBLE_MODES or not (1 <= h <= H and 1 <= w <= W and s >= 1):
        raise ValueError(f"valid_region: mode {k}, a {h} x {w} frame inside {H} x {W}, scale {s}")
    ys = (s * (H - h), s * H) if k & 2 else (0, s * h)
    xs = (s * (W - w), s * W) if k & 1 else (0, s * w)
    return (*xs, *ys) if k & 4 else (*ys, *xs)
