"""Device-resident training data: the reference's dataset (data/realvsr_dataset.py, data/mvsr4x_dataset.py) with the frames held on
the GPU as bytes and a step's batch built by one gather launch (`ops.gather_pairs`, csrc/batch.hip).

What stays on the host is what decides WHAT to gather -- the permutation of key frames, the mirrored windows (`harness.train_window`),
the crop origin and the three flips of every item -- as pure functions (`draw_item`, `epoch_plan`, `check_plan`), so it is tested
without a GPU.  An epoch's plan is two small int32 arrays, uploaded once.

    store = FramePairs(lr_u8, hr_u8, scale=4, n_seq=50)                 # or FramePairs.from_files(lr_paths, hr_paths, ...)
    batches = TrainBatches(store, batch_size=2, patch_size=96, n_frame=7, seed=0)
    for epoch in range(epochs):
        batches.set_epoch(epoch)
        for batch in batches:                                           # {'lr_seq', 'hr_seq', 'fname'}: fp32, on the device
            step.step(batch)                                            # graph.GraphedTrainStep, or model.set_input(batch) + optimize_parameters()

Zero-copy variant: `TrainBatches(..., out=(step.static_lr, step.static_hr))` gathers straight into the captured graph's input
buffers; iterate and call `step.step()` with no batch.

LR frames are either supplied, or made on the device from the full-size "wide" frames as the reference's loaders make them
(`cv2.resize(img, (w // scale, h // scale), interpolation=cv2.INTER_CUBIC)`, data/mvsr4x_dataset.py:192-201,
data/realvsr_dataset.py:200): `FramePairs.from_wide` / `from_wide_files`, `ops.resize_cubic_u8` (csrc/resize_cubic.hip) with the
tables of `cubic_tables`, which restates OpenCV's 8-bit fixed-point path; OpenCV itself is not needed.

Out of scope here: file lists and option parsing, a host-memory store, random numbers on the device.
"""
from __future__ import annotations

import functools
import os
import random
from typing import Callable, Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import harness

HFLIP, VFLIP, TRANSPOSE = 1, 2, 4


def draw_item(rng: random.Random, ih: int, iw: int, patch: int) -> Tuple[int, int, int]:
    """(top, left, flags) of one training item, consuming `rng` exactly as the reference consumes the `random` module for it:
    `_crop_patch` (realvsr_dataset.py:166-169) draws the COLUMN first, `randrange(0, iw - patch + 1)`, then the row,
    `randrange(0, ih - patch + 1)`; `augment_basic` (util.py:242-245) then draws hflip, vflip and the transpose, each
    `random() < 0.5`.  The same seed gives the reference's crop and flips."""
    if patch < 1 or patch > ih or patch > iw:
        raise ValueError(f"draw_item: patch {patch} does not fit a {ih} x {iw} frame")
    left = rng.randrange(0, iw - patch + 1)
    top = rng.randrange(0, ih - patch + 1)
    hflip = rng.random() < 0.5
    vflip = rng.random() < 0.5
    rot90 = rng.random() < 0.5
    return top, left, (HFLIP if hflip else 0) | (VFLIP if vflip else 0) | (TRANSPOSE if rot90 else 0)


def default_name(idx: int, n_seq: int) -> str:
    """'SSS_FFFFF.png': scene and frame within the scene, the datasets' naming (the scene is what `harness.scene_report` groups by)"""
    return "%03d_%05d.png" % (idx // n_seq, idx % n_seq)


def epoch_plan(n_items: int, n_frame: int, n_seq: int, batch_size: int, ih: int, iw: int, patch: int, seed: int, epoch: int,
               rank: int = 0, world: int = 1, names: Optional[Sequence[str]] = None):
    """What one rank gathers in one epoch: (frames (B, n, t) int32, desc (B, n, 4) int32 = top, left, flags, 0, names: B lists of
    the n key frames' names).

    Key frames are one permutation of range(n_items) per (seed, epoch), the same on every rank; rank r takes entries r, r + world,
    ... of it, and every rank the same number: n_items // world, cut down to whole batches (the graphed step needs fixed
    shapes, so the incomplete tail is dropped).  An item's window is `harness.train_window` (mirrored at the ends of its scene of
    n_seq frames); its crop and flips are one `draw_item` from a generator seeded by (seed, epoch, key frame) -- so they depend
    neither on `world` nor on `batch_size`, only on which frame it is."""
    if n_items < 1 or n_seq < 1 or n_items % n_seq != 0:
        raise ValueError(f"epoch_plan: {n_items} frames are not whole scenes of n_seq {n_seq}")
    if n_frame < 1 or n_frame > n_seq:      # train_window's mirroring assumes this (NOTE: the reference does not check it)
        raise ValueError(f"epoch_plan: n_frame {n_frame} must be in [1, n_seq {n_seq}]")
    if batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"epoch_plan: batch_size {batch_size}, rank {rank} of {world}")
    if patch < 1 or patch > ih or patch > iw:
        raise ValueError(f"epoch_plan: patch {patch} does not fit a {ih} x {iw} frame")
    perm = list(range(n_items))
    random.Random(f"eavsr-epoch:{int(seed)}:{int(epoch)}").shuffle(perm)
    n_batches = (n_items // world) // batch_size
    keys = perm[rank::world][:n_batches * batch_size]
    frames = np.zeros((n_batches, batch_size, n_frame), np.int32)
    desc = np.zeros((n_batches, batch_size, 4), np.int32)
    out_names: List[List[str]] = []
    for i, key in enumerate(keys):
        b, j = divmod(i, batch_size)
        frames[b, j] = harness.train_window(key, key % n_seq, n_frame, n_seq)
        desc[b, j, :3] = draw_item(random.Random(f"eavsr-item:{int(seed)}:{int(epoch)}:{key}"), ih, iw, patch)
        if j == 0:
            out_names.append([])
        out_names[-1].append(names[key] if names is not None else default_name(key, n_seq))
    return frames, desc, out_names


def check_plan(frames, desc, n_items: int, ih: int, iw: int, patch) -> None:
    """Host validation of a plan before it is uploaded (the kernel clamps instead of trusting it; a plan that needed the clamp is a
    bug): every frame index in [0, n_items), every origin inside the frame, no flag above bit 2, and no transpose unless the patch
    is square.  ValueError otherwise."""
    ph, pw = (int(patch), int(patch)) if isinstance(patch, int) else (int(patch[0]), int(patch[1]))
    frames, desc = np.asarray(frames), np.asarray(desc)
    if frames.dtype != np.int32 or desc.dtype != np.int32 or desc.shape[-1] != 4 or frames.shape[:-1] != desc.shape[:-1]:
        raise ValueError(f"check_plan: frames int32 (..., t) and desc int32 (..., 4), got {frames.dtype} {frames.shape} / {desc.dtype} {desc.shape}")
    if ph < 1 or pw < 1 or ph > ih or pw > iw:
        raise ValueError(f"check_plan: patch {ph} x {pw} does not fit a {ih} x {iw} frame")
    if frames.size == 0:
        return
    if frames.min() < 0 or frames.max() >= n_items:
        raise ValueError(f"check_plan: frame indices {int(frames.min())}..{int(frames.max())} outside the store's [0, {n_items})")
    top, left, flags = desc[..., 0], desc[..., 1], desc[..., 2]
    if top.min() < 0 or top.max() > ih - ph or left.min() < 0 or left.max() > iw - pw:
        raise ValueError(f"check_plan: a {ph} x {pw} crop at rows {int(top.min())}..{int(top.max())}, columns {int(left.min())}.."
                         f"{int(left.max())} leaves the {ih} x {iw} frame")
    if (flags & ~7).any():
        raise ValueError("check_plan: flags are bit 0 hflip, bit 1 vflip, bit 2 transpose; a higher bit is set")
    if ph != pw and (flags & TRANSPOSE).any():
        raise ValueError(f"check_plan: the transpose flag needs a square patch, got {ph} x {pw}")


CUBIC_MAX_RATIO = 8


@functools.lru_cache(maxsize=64)
def _cubic_tables(src: int, dst: int):
    scale = 1.0 / (dst / src)                                   # float64; OpenCV inverts the inverse scale
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    x = (f - s).astype(np.float32)                              # float32 - float32 (s is integral and exact)
    one, A = np.float32(1), np.float32(-0.75)
    A2, A3, A4, A5, A8 = A + np.float32(2), A + np.float32(3), np.float32(4) * A, np.float32(5) * A, np.float32(8) * A
    x1, xm = x + one, one - x
    c = np.empty((dst, 4), np.float32)
    c[:, 0] = ((A * x1 - A5) * x1 + A8) * x1 - A4
    c[:, 1] = (A2 * x - A3) * x * x + one
    c[:, 2] = (A2 * xm - A3) * xm * xm + one
    c[:, 3] = one - c[:, 0] - c[:, 1] - c[:, 2]
    coef = np.clip(np.rint(c * np.float32(2048)), -32768, 32767).astype(np.int16)
    ofs = s.astype(np.int32)
    ofs.setflags(write=False)
    coef.setflags(write=False)
    return ofs, coef


def cubic_tables(src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """One axis of OpenCV's `resize` for CV_8U, INTER_CUBIC, from `src` samples to `dst`: (ofs int32[dst], coef int16[dst, 4]), both
    read-only (cached per (src, dst)).  Output d reads the source samples ofs[d] - 1 .. ofs[d] + 2, each index clamped into
    [0, src - 1] (replicate border), with the weights coef[d] / 2048:

        scale = 1.0 / (dst / src) in float64;  f = float32((d + 0.5) * scale - 0.5);  ofs = floor(f);  x = float32(f - ofs)
        with A = -0.75f, in float32, left to right, every operation rounded (no FMA):
          c0 = ((A*(x+1) - 5*A)*(x+1) + 8*A)*(x+1) - 4*A;   c1 = ((A+2)*x - (A+3))*x*x + 1
          c2 = ((A+2)*(1-x) - (A+3))*(1-x)*(1-x) + 1;       c3 = 1 - c0 - c1 - c2
        coef[d][j] = saturate_int16(round_half_even(c_j * 2048))

    The four weights are NOT corrected to sum to 2048 (2047 or 2049 at some positions, e.g. 70 -> 17); OpenCV does not either.  The
    image: hor = sum_j coefx * src (int32, exact), v = sum_j coefy * hor (int32), out = clamp((v + 2^21) >> 22, 0, 255): the
    scalar C++ path of OpenCV, which rounds exact ties up; a SIMD build's vertical pass rounds them to even instead.
    Built on the host: inside a kernel the compiler would contract a*b+c into an FMA and could move a weight by one.

    ValueError for dst < 1 and for a ratio src / dst outside [1, 8] (no upscaling; the bound limits the kernel's footprint)."""
    src, dst = int(src), int(dst)
    if dst < 1:
        raise ValueError(f"cubic_tables: {src} -> {dst}: at least one output sample")
    if src < dst or src > CUBIC_MAX_RATIO * dst:
        raise ValueError(f"cubic_tables: {src} -> {dst}: the ratio src / dst must be in [1, {CUBIC_MAX_RATIO}] (no upscaling)")
    return _cubic_tables(src, dst)


def _as_u8_frames(x, what: str) -> torch.Tensor:
    if isinstance(x, np.ndarray):
        if x.dtype != np.uint8:
            raise ValueError(f"FramePairs: {what}: uint8 frames, got {x.dtype}")
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"FramePairs: {what}: a tensor or an ndarray, got {type(x)}")
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError(f"FramePairs: {what}: uint8 (F, C, h, w) or (F, h, w, C), got {x.dtype} {tuple(x.shape)}")
    return x


def _interleaved(x: torch.Tensor) -> bool:
    return x.shape[3] in (1, 3) and x.shape[1] not in (1, 3)


def _check_device_reader(reader: str, what: str) -> None:
    if reader != "device":
        raise ValueError(f"{what}: reader={reader!r}: a callable, or 'device' for harness.decode_png_frames")


def _png_shape(path) -> Tuple[int, int, int]:
    """(C, H, W) of the planes `harness.decode_png_frames(.., channels=3)` makes of a PNG file, from its chunks alone"""
    with open(os.fspath(path), "rb") as f:
        h, w, c, _ = harness.parse_png(f.read(), os.fspath(path))
    return min(c, 3), h, w


def _decode_files(paths, shape, dev, chunk: int) -> torch.Tensor:
    """one PNG file per frame -> a preallocated uint8 (F, C, H, W) device tensor, `chunk` files per `decode_png_frames` call"""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError(f"FramePairs: chunk {chunk}")
    store = torch.empty((len(paths),) + tuple(shape), device=dev, dtype=torch.uint8)
    for lo in range(0, len(paths), chunk):
        harness.decode_png_frames(paths[lo:lo + chunk], dev, channels=3, out=store[lo:lo + chunk])
    return store


class FramePairs:
    """The store: every LR frame and its HR frame as bytes on the device, CHW.

    lr (F, C, h, w) / hr (F, C, scale h, scale w): uint8 tensors or ndarrays, planes or interleaved (F, h, w, C) (a last dimension
    of 1 or 3 where the second is not; permuted ONCE here, as bytes, never in the gather kernel).  hr may be None (inference-only
    stores).  The F frames are whole scenes of n_seq consecutive frames.  `names`: one per frame (default 'SSS_FFFFF.png').
    `device`: where the store lives (default cuda:<current>); the shape checks run before anything is moved there."""

    def __init__(self, lr, hr, scale: int, n_seq: int, names: Optional[Sequence[str]] = None, device=None):
        lr = _as_u8_frames(lr, "lr")
        hr = _as_u8_frames(hr, "hr") if hr is not None else None
        lr_hwc, hr_hwc = _interleaved(lr), hr is not None and _interleaved(hr)
        chw = lambda x, il: tuple(int(x.shape[i]) for i in ((0, 3, 1, 2) if il else (0, 1, 2, 3)))
        f, c, h, w = chw(lr, lr_hwc)
        scale, n_seq = int(scale), int(n_seq)
        if scale < 1:
            raise ValueError(f"FramePairs: scale {scale}")
        if hr is not None and chw(hr, hr_hwc) != (f, c, scale * h, scale * w):
            raise ValueError(f"FramePairs: hr must be scale {scale} x lr {(f, c, h, w)} = {(f, c, scale * h, scale * w)}, got {chw(hr, hr_hwc)}")
        if n_seq < 1 or f == 0 or f % n_seq != 0:
            raise ValueError(f"FramePairs: {f} frames are not whole scenes of n_seq {n_seq}")
        if names is not None and len(names) != f:
            raise ValueError(f"FramePairs: {len(names)} names for {f} frames")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        put = lambda x, il: (x.to(dev).permute(0, 3, 1, 2) if il else x.to(dev)).contiguous()
        self.lr = put(lr, lr_hwc)
        self.hr = put(hr, hr_hwc) if hr is not None else None
        self.scale, self.n_seq = scale, n_seq
        self.names = list(names) if names is not None else [default_name(i, n_seq) for i in range(f)]

    @classmethod
    def from_files(cls, lr_paths: Sequence[str], hr_paths: Optional[Sequence[str]], scale: int, n_seq: int,
                   names: Optional[Sequence[str]] = None, device=None, reader=harness.read_png, chunk: int = 16) -> "FramePairs":
        """Read one file per frame.  `reader(path)` returns a uint8 (C, H, W) tensor or array; the default, `harness.read_png`, undoes
        the PNG scanline filters in a Python loop (seconds per full-size frame).  reader="device" decodes non-interlaced 8-bit grey /
        RGB / RGBA PNG files with `harness.decode_png_frames` instead: zlib in a thread pool, the scanline unfilter on the
        device, `chunk` files at a time straight into the preallocated stores -- decoded frames never exist on the host.  The sizes
        are checked on the first LR and HR file, before the bulk of the work.  Other formats: pass your own reader."""
        if hr_paths is not None and len(hr_paths) != len(lr_paths):
            raise ValueError(f"FramePairs.from_files: {len(lr_paths)} LR and {len(hr_paths)} HR files")
        if isinstance(reader, str):
            _check_device_reader(reader, "FramePairs.from_files")
            scale, n_seq = int(scale), int(n_seq)
            n = len(lr_paths)
            if n_seq < 1 or n == 0 or n % n_seq != 0:
                raise ValueError(f"FramePairs.from_files: {n} frames are not whole scenes of n_seq {n_seq}")
            if names is not None and len(names) != n:
                raise ValueError(f"FramePairs.from_files: {len(names)} names for {n} frames")
            lr_shape = _png_shape(lr_paths[0])
            if hr_paths is not None:
                c, h, w = lr_shape
                if scale < 1 or _png_shape(hr_paths[0]) != (c, scale * h, scale * w):
                    raise ValueError(f"FramePairs.from_files: hr must be scale {scale} x lr {lr_shape} = {(c, scale * h, scale * w)}, "
                                     f"got {_png_shape(hr_paths[0])} ({hr_paths[0]})")
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            lr = _decode_files(lr_paths, lr_shape, dev, chunk)
            hr = _decode_files(hr_paths, _png_shape(hr_paths[0]), dev, chunk) if hr_paths is not None else None
            return cls(lr, hr, scale, n_seq, names=names, device=dev)
        read = lambda paths: torch.stack([torch.as_tensor(np.asarray(reader(p))) for p in paths])
        return cls(read(lr_paths), read(hr_paths) if hr_paths is not None else None, scale, n_seq, names=names, device=device)

    @classmethod
    def _from_wide_chunks(cls, what: str, n: int, get: Callable[[int, int], torch.Tensor], hr, scale: int, n_seq: int, names,
                          device, chunk: int) -> "FramePairs":
        """`get(lo, hi)`: wide frames [lo, hi) as uint8 (hi - lo, C, H, W) or (hi - lo, H, W, C), anywhere.  Every check runs on
        the first chunk's shape, before anything is moved to the device."""
        scale, n_seq, chunk = int(scale), int(n_seq), int(chunk)
        if scale < 1 or scale > CUBIC_MAX_RATIO:
            raise ValueError(f"{what}: scale {scale} must be in [1, {CUBIC_MAX_RATIO}]")
        if chunk < 1:
            raise ValueError(f"{what}: chunk {chunk}")
        if n_seq < 1 or n == 0 or n % n_seq != 0:
            raise ValueError(f"{what}: {n} frames are not whole scenes of n_seq {n_seq}")
        if names is not None and len(names) != n:
            raise ValueError(f"{what}: {len(names)} names for {n} frames")
        chw = lambda x: tuple(int(x.shape[i]) for i in ((0, 3, 1, 2) if _interleaved(x) else (0, 1, 2, 3)))
        first = _as_u8_frames(get(0, min(chunk, n)), "wide")
        _, c, H, W = chw(first)
        if hr is not None and chw(hr) != (n, c, H, W):
            raise ValueError(f"{what}: wide and hr frames must have the same size: wide {(n, c, H, W)}, hr {chw(hr)}")
        if H % scale or W % scale:
            raise ValueError(f"{what}: H % scale == 0 and W % scale == 0 is required (the store holds hr = scale x lr exactly; nothing "
                             f"is cropped here): {H} x {W} frames, scale {scale}")
        from . import ops
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        lr = torch.empty((n, c, H // scale, W // scale), device=dev, dtype=torch.uint8)
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            part = first if lo == 0 else _as_u8_frames(get(lo, hi), "wide")
            if chw(part) != (hi - lo, c, H, W):
                raise ValueError(f"{what}: wide frames {lo}..{hi - 1} are {chw(part)[1:]}, the first ones {(c, H, W)}")
            part = part.to(dev, non_blocking=True)
            part = (part.permute(0, 3, 1, 2) if _interleaved(part) else part).contiguous()
            ops.resize_cubic_u8(part, (H // scale, W // scale), out=lr[lo:hi])
        return cls(lr, hr, scale, n_seq, names=names, device=dev)

    @classmethod
    def from_wide(cls, wide, hr, scale: int, n_seq: int, names: Optional[Sequence[str]] = None, device=None,
                  chunk: int = 16) -> "FramePairs":
        """The store of a data set kept as the reference keeps it: `wide` frames of the SAME size as the `hr` ("tele") frames, the LR
        frame being `cv2.resize(wide, (W // scale, H // scale), interpolation=cv2.INTER_CUBIC)` (data/mvsr4x_dataset.py:192-201,
        data/realvsr_dataset.py:200) -- computed here on the device by `ops.resize_cubic_u8`, bit for bit as `cubic_tables` defines it.

        wide, hr: uint8 (F, C, H, W) or (F, H, W, C), ndarrays or tensors, on the host or the device; hr None: an inference-only
        store.  H % scale == 0 and W % scale == 0 (ValueError otherwise: nothing is cropped silently).  `wide` is uploaded and
        resized `chunk` frames at a time into the preallocated LR store, so the full-size wide frames are never all on the device;
        the result does not depend on `chunk`."""
        wide = _as_u8_frames(wide, "wide")
        hr = _as_u8_frames(hr, "hr") if hr is not None else None
        return cls._from_wide_chunks("FramePairs.from_wide", int(wide.shape[0]), lambda lo, hi: wide[lo:hi], hr, scale, n_seq, names,
                                     device, chunk)

    @classmethod
    def from_wide_files(cls, wide_paths: Sequence[str], hr_paths: Optional[Sequence[str]], scale: int, n_seq: int,
                        names: Optional[Sequence[str]] = None, device=None, reader=harness.read_png, chunk: int = 16) -> "FramePairs":
        """`from_wide` from one file per frame, read `chunk` wide files at a time (`reader`: see `from_files`).  reader="device": a
        chunk of wide frames is decoded on the device (`harness.decode_png_frames`) and resized there; the HR files are decoded in
        chunks into a preallocated device tensor."""
        if hr_paths is not None and len(hr_paths) != len(wide_paths):
            raise ValueError(f"FramePairs.from_wide_files: {len(wide_paths)} wide and {len(hr_paths)} HR files")
        if isinstance(reader, str):
            _check_device_reader(reader, "FramePairs.from_wide_files")
            if len(wide_paths) == 0:
                raise ValueError("FramePairs.from_wide_files: 0 frames")
            if hr_paths is not None and _png_shape(hr_paths[0]) != _png_shape(wide_paths[0]):
                raise ValueError(f"FramePairs.from_wide_files: wide and hr frames must have the same size: wide "
                                 f"{_png_shape(wide_paths[0])}, hr {_png_shape(hr_paths[0])}")
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
            hr = _decode_files(hr_paths, _png_shape(hr_paths[0]), dev, chunk) if hr_paths is not None else None
            get = lambda lo, hi: harness.decode_png_frames(wide_paths[lo:hi], dev, channels=3)
            return cls._from_wide_chunks("FramePairs.from_wide_files", len(wide_paths), get, hr, scale, n_seq, names, dev, chunk)
        read = lambda paths: torch.stack([torch.as_tensor(np.asarray(reader(p))) for p in paths])
        hr = _as_u8_frames(read(hr_paths), "hr") if hr_paths is not None else None
        return cls._from_wide_chunks("FramePairs.from_wide_files", len(wide_paths), lambda lo, hi: read(wide_paths[lo:hi]), hr, scale,
                                     n_seq, names, device, chunk)

    def __len__(self) -> int:
        return int(self.lr.shape[0])

    @property
    def frame_size(self) -> Tuple[int, int]:
        return int(self.lr.shape[2]), int(self.lr.shape[3])

    @property
    def device(self) -> torch.device:
        return self.lr.device


class TrainBatches:
    """The training loader: iterating yields one epoch's `{'lr_seq': (n, t, C, p, p), 'hr_seq': (n, t, C, s p, s p), 'fname': [n
    names]}`, fp32 on the store's device, each from one `ops.gather_pairs` launch.  `set_epoch(e)` draws epoch e's plan
    (`epoch_plan`), checks it (`check_plan`) and uploads it once; the same (seed, epoch) gives the same batches on every run.

    rank / world default to torch.distributed's when it is initialised (else 0 / 1).  `out=(lr, hr)`: gather every batch into
    these buffers (`GraphedTrainStep.static_lr` / `static_hr`: the batch then needs no copy and `step()` is called without one);
    the yielded tensors are those buffers, overwritten by the next batch.  Without it every batch is newly allocated."""

    def __init__(self, store: FramePairs, batch_size: int, patch_size: int, n_frame: int, seed: int = 0, rank: Optional[int] = None,
                 world: Optional[int] = None, out=None):
        if store.hr is None:
            raise ValueError("TrainBatches: the store has no HR frames")
        import torch.distributed as dist
        if rank is None or world is None:
            live = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if live else 0) if rank is None else rank
            world = (dist.get_world_size() if live else 1) if world is None else world
        self.store, self.batch_size, self.patch_size, self.n_frame = store, int(batch_size), int(patch_size), int(n_frame)
        self.seed, self.rank, self.world, self.out = int(seed), int(rank), int(world), out
        self.epoch = None
        self.set_epoch(0)

    def set_epoch(self, epoch: int) -> None:
        s = self.store
        ih, iw = s.frame_size
        frames, desc, names = epoch_plan(len(s), self.n_frame, s.n_seq, self.batch_size, ih, iw, self.patch_size, self.seed, epoch,
                                         self.rank, self.world, s.names)
        check_plan(frames, desc, len(s), ih, iw, self.patch_size)
        self.epoch, self.names = int(epoch), names
        self.frames = torch.from_numpy(frames).to(s.device)
        self.desc = torch.from_numpy(desc).to(s.device)

    def __len__(self) -> int:
        return int(self.frames.shape[0])

    def __iter__(self) -> Iterator[Dict]:
        from . import ops
        s = self.store
        for b in range(len(self)):
            lr, hr = ops.gather_pairs(s.lr, s.hr, self.frames[b], self.desc[b], self.patch_size, s.scale, out=self.out)
            yield {"lr_seq": lr, "hr_seq": hr, "fname": self.names[b]}


def _items(store: FramePairs, windows: List[List[int]], top: int, left: int, patch) -> Iterator[Dict]:
    from . import ops
    ih, iw = store.frame_size
    frames = np.asarray(windows, np.int32).reshape(len(windows), 1, -1)
    desc = np.zeros((len(windows), 1, 4), np.int32)
    desc[..., 0], desc[..., 1] = top, left
    check_plan(frames, desc, len(store), ih, iw, patch)
    frames_dev, desc_dev = torch.from_numpy(frames).to(store.device), torch.from_numpy(desc).to(store.device)
    for i, win in enumerate(windows):
        lr, hr = ops.gather_pairs(store.lr, store.hr, frames_dev[i], desc_dev[i], patch, store.scale, may_transpose=False)
        item = {"lr_seq": lr, "fname": [store.names[k] for k in win]}
        if hr is not None:
            item["hr_seq"] = hr
        yield item


def val_items(store: FramePairs, n_frame: int, p: int = 256) -> Iterator[Dict]:
    """The validation items (`_getitem_val`, realvsr_dataset.py:96-128): for every frame the mirrored window around it
    (`harness.train_window`), centre-cropped to p x p LR / scale p x scale p HR as `harness.crop_center` does, no flips, batch 1 --
    what `harness.evaluate` consumes.  'fname' names every frame of the window (the per-frame report needs one each; the reference
    carries a single name).  The HR crop's origin is scale x the LR crop's, which is the centre crop of the HR frame only when
    h - p and w - p are even: ValueError otherwise."""
    ih, iw = store.frame_size
    if p > ih or p > iw:
        raise ValueError(f"val_items: a {p} x {p} crop does not fit the {ih} x {iw} frames")
    if (ih - p) % 2 or (iw - p) % 2:
        raise ValueError(f"val_items: {ih} x {iw} frames minus a crop of {p} leave an odd margin: the HR centre crop is not scale x the LR one")
    windows = [harness.train_window(i, i % store.n_seq, n_frame, store.n_seq) for i in range(len(store))]
    return _items(store, windows, (ih - p) // 2, (iw - p) // 2, p)


def test_items(store: FramePairs, n_frame: int) -> Iterator[Dict]:
    """The test items (`_getitem_test`, realvsr_dataset.py:130-147): every scene cut into n_seq / n_frame non-overlapping windows
    (`harness.test_window_starts`), full frames, no flips, batch 1, 'fname' the window's frame names."""
    starts = harness.test_window_starts(len(store), store.n_seq, n_frame)
    return _items(store, [list(range(s0, s0 + n_frame)) for s0 in starts], 0, 0, store.frame_size)


test_items.__test__ = False      # a name pytest would otherwise collect when a test module imports it
