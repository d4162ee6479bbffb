"""Evaluation harness either side of the hot path (f4).

Counterparts of the reference's test loop (test_basic.py:56-83: set_input -> synchronize -> model.test() ->
synchronize, PSNR on the clamp*255*round visuals), of `calc_psnr` (util/util.py:302-320) and of the frame-window
index maps of the datasets (data/mvsr4x_dataset.py:105-147), of the frame writing of test_basic.py:85-92 (8-bit RGB PNG
files under `<root>/sr_{full,patch}_<iter>/<scene>/<frame>`; a dependency-free encoder: zlib + struct) and of the SSIM of
psnr_total.py:39-44 (skimage's `structural_similarity(win_size=11, data_range=255, multichannel=True,
gaussian_weights=True)`, restated in torch).  `evaluate(..., per_frame=True)` gives psnr_total.py's report -- every frame on its
own, the mean per scene, the mean of the scenes (psnr_total.py:88-143) -- from one fused HIP pass (`ops.frame_metrics`,
csrc/metrics.hip), and with an LPIPS network (`eavsr_amd.lpips.LPIPSAlex`, csrc/lpips.hip; its pretrained weights come from a path
the user names, `opt.lpips_path`: none ship here) the report's third column, LPIPS (psnr_total.py:27-35), as well; `calc_psnr` / `calc_ssim` stay as the host restatements its tests compare with.  No dataset files: the benchmarks feed synthetic clips, a user's loader
feeds `{'lr_seq', 'hr_seq', 'fname'}` dicts exactly as the reference's does.
"""
from __future__ import annotations

import contextlib
import math
import os
import struct
import time
import zlib
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .segments import DEFAULT_OVERLAP

Tensor = torch.Tensor


def calc_psnr(sr: Tensor, hr: Tensor, range: float = 255.0) -> float:
    """-10 log10(mean(((sr - hr) / range)^2)) over the whole tensor (util/util.py:302-320); inputs are the
    `get_current_visuals()` tensors (already x255, clamped and rounded)."""
    with torch.no_grad():
        diff = (sr.float() - hr.float()) / range
        mse = torch.pow(diff, 2).mean()
        return (-10 * torch.log10(mse)).item()


def calc_ssim(sr: Tensor, hr: Tensor, data_range: float = 255.0, win_size: int = 11, sigma: float = 1.5) -> float:
    """Mean SSIM of two images as psnr_total.py:39-44 computes it: skimage.metrics.structural_similarity(out, ref,
    win_size=11, data_range=255, multichannel=True, gaussian_weights=True) -- per channel, an 11-tap gaussian window of
    sigma 1.5 (truncate 3.5), sample covariances (x NP / (NP - 1), NP = 11^2), K1 = 0.01, K2 = 0.03, the SSIM map cropped by
    (win_size - 1) / 2 on every side, mean over pixels and channels; float64 arithmetic as skimage's for 8-bit inputs.
    sr / hr: (..., C, H, W) tensors in [0, data_range] (the `get_current_visuals()` frames); leading dimensions are averaged."""
    if sr.shape != hr.shape or sr.dim() < 3:
        raise ValueError(f"calc_ssim: shapes {tuple(sr.shape)} / {tuple(hr.shape)}")
    h, w = sr.shape[-2:]
    if min(h, w) < win_size:
        raise ValueError(f"calc_ssim: image {h} x {w} smaller than the {win_size}-tap window")
    with torch.no_grad():
        x = sr.reshape(-1, 1, h, w).to(torch.float64)
        y = hr.reshape(-1, 1, h, w).to(torch.float64)
        r = win_size // 2
        k = torch.exp(-0.5 * (torch.arange(-r, r + 1, dtype=torch.float64, device=x.device) / sigma) ** 2)
        k = k / k.sum()
        kh, kw = k.view(1, 1, -1, 1), k.view(1, 1, 1, -1)
        filt = lambda t: torch.nn.functional.conv2d(torch.nn.functional.conv2d(t, kh), kw)      # "valid": exactly the cropped region
        ux, uy = filt(x), filt(y)
        cov_norm = (win_size * win_size) / (win_size * win_size - 1.0)
        vx = cov_norm * (filt(x * x) - ux * ux)
        vy = cov_norm * (filt(y * y) - uy * uy)
        vxy = cov_norm * (filt(x * y) - ux * uy)
        c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
        s_map = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
        return s_map.mean().item()


def _png_chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png(image: Tensor, path: str, level: int = 6, hwc: Optional[bool] = None) -> str:
    """One 8-bit image, (3, H, W) RGB or (1, H, W) / (H, W) grey, values 0..255 (a `get_current_visuals()` frame: already
    clamped and rounded), as a PNG file -- what `dataset_test.imio.write(np.array(frame).astype(np.uint8), path)` leaves
    (test_basic.py:85-92; data/imlib.py:164-166 creates the directory).  Colour type 2 / 0, bit depth 8, filter 0, one IDAT.
    A uint8 (H, W, 3) / (H, W, 1) tensor -- one frame of `ops.frame_metrics(..., rgb8=True)` / `ops.rgb8` -- is taken as the
    scanlines themselves: no float pass and no permute.  `hwc` says which layout a uint8 tensor has; by default a uint8 tensor
    whose last dimension is 1 or 3 and whose first is not is interleaved (an H of 1 or 3 reads as planes, as it always did)."""
    t = image.detach()
    if hwc is None:
        hwc = t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] in (1, 3) and t.shape[0] not in (1, 3)
    if hwc:
        if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] not in (1, 3):
            raise ValueError(f"write_png: an interleaved image is uint8 (H, W, 3) or (H, W, 1), got {t.dtype} {tuple(image.shape)}")
        h, w, c = (int(v) for v in t.shape)
        u8 = t.contiguous().cpu()
    else:
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[0] not in (1, 3):
            raise ValueError(f"write_png: (3, H, W), (1, H, W) or (H, W), got {tuple(image.shape)}")
        c, h, w = (int(v) for v in t.shape)
        u8 = t.to(torch.float32).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu()      # astype(np.uint8): truncation
    rows = torch.cat([torch.zeros(h, 1, dtype=torch.uint8), u8.view(h, w * c)], 1)                  # filter byte 0 per scanline
    raw = rows.numpy().tobytes()
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n")
        f.write(_png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0)))
        f.write(_png_chunk(b"IDAT", zlib.compress(raw, level)))
        f.write(_png_chunk(b"IEND", b""))
    return path


def parse_png(data: bytes, what: str = ""):
    """The chunk walk of a PNG file held in memory -> (h, w, c, idat): the size, the bytes per pixel (1 grey, 3 RGB, 4 RGBA) and the
    concatenated IDAT bodies (one zlib stream).  Checks the signature, every chunk's CRC-32 and the IHDR (8 bits per sample, colour
    type 0 / 2 / 6, no interlace); ancillary chunks are ignored.  ValueError, prefixed with `what` (the file's name), for anything
    else, a missing IHDR or IDAT and a file that ends inside a chunk.  Shared by `read_png` and `decode_png_frames`."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{what}: not a PNG file")
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        if pos + 8 > len(data):
            raise ValueError(f"{what}: truncated: the file ends inside a chunk header")
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + n > len(data):
            raise ValueError(f"{what}: truncated: the file ends inside chunk {tag!r}")
        body = data[pos + 8:pos + 8 + n]
        if zlib.crc32(tag + body) & 0xFFFFFFFF != struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0]:
            raise ValueError(f"{what}: CRC mismatch in chunk {tag!r}")
        if tag == b"IHDR":
            if n != 13:
                raise ValueError(f"{what}: IHDR of {n} bytes")
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        pos += 12 + n
    if hdr is None:
        raise ValueError(f"{what}: no IHDR chunk")
    w, h, depth, ctype, _, _, interlace = hdr
    if depth != 8 or ctype not in (0, 2, 6) or interlace:
        raise ValueError(f"{what}: only non-interlaced 8-bit grey / RGB / RGBA")
    if not idat:
        raise ValueError(f"{what}: no IDAT chunk")
    if w < 1 or h < 1:
        raise ValueError(f"{what}: an image of {w} x {h}")
    return h, w, {0: 1, 2: 3, 6: 4}[ctype], b"".join(idat)


def read_png(path: str) -> Tensor:
    """Decoder for the files `write_png` writes and for any non-interlaced 8-bit grey / RGB / RGBA PNG (all five scanline
    filters): (C, H, W) uint8.  For round trips and for feeding stored frames back; not a general PNG reader.  The scanline filters
    are undone in a Python loop (seconds per full-size frame): `decode_png_frames` does that half on the device."""
    data = open(path, "rb").read()
    h, w, c, idat = parse_png(data, path)
    raw = bytearray(zlib.decompress(idat))
    stride = w * c
    out = bytearray(h * stride)
    prev = bytearray(stride)
    for y in range(h):
        ft = raw[y * (stride + 1)]
        line = raw[y * (stride + 1) + 1:(y + 1) * (stride + 1)]
        if ft == 1:
            for i in range(c, stride):
                line[i] = (line[i] + line[i - c]) & 255
        elif ft == 2:
            for i in range(stride):
                line[i] = (line[i] + prev[i]) & 255
        elif ft == 3:
            for i in range(stride):
                line[i] = (line[i] + (((line[i - c] if i >= c else 0) + prev[i]) >> 1)) & 255
        elif ft == 4:
            for i in range(stride):
                a = line[i - c] if i >= c else 0
                b = prev[i]
                cc = prev[i - c] if i >= c else 0
                pa, pb, pc = abs(b - cc), abs(a - cc), abs(a + b - 2 * cc)
                line[i] = (line[i] + (a if (pa <= pb and pa <= pc) else b if pb <= pc else cc)) & 255
        elif ft != 0:
            raise ValueError(f"{path}: scanline filter {ft}")
        out[y * stride:(y + 1) * stride] = line
        prev = line
    return torch.frombuffer(out, dtype=torch.uint8).view(h, w, c).permute(2, 0, 1).contiguous()


def _png_file(idat: bytes, h: int, w: int, c: int) -> bytes:
    """signature, IHDR (8-bit grey or RGB, no interlace), one IDAT holding `idat` (a complete zlib stream), IEND"""
    return (b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 0, 0, 0, 0))
            + _png_chunk(b"IDAT", idat) + _png_chunk(b"IEND", b""))


PNG_ENCODERS = ("host", "device")


def check_png_encoder(encoder) -> str:
    if encoder not in PNG_ENCODERS:
        raise ValueError(f"png_encoder={encoder!r}: one of {PNG_ENCODERS}")
    return encoder


PNG_DECODERS = ("host", "device")


def check_png_decoder(decoder) -> str:
    if decoder not in PNG_DECODERS:
        raise ValueError(f"png_decoder={decoder!r}: one of {PNG_DECODERS}")
    return decoder


class _PngStaging:
    """The host side of the device PNG encoder: two pinned staging buffers used in turn.  `enqueue(rgb8)` launches the
    filter and entropy passes (`ops.png_encode`) on the current stream and, on a side stream behind them, the copy of the streams and
    their sizes into one of the buffers, followed by an event; it returns a job without waiting for anything.  `files(job)` waits for
    that job's event alone and wraps every stream into a file (the chunk CRC-32 is `zlib.crc32` over the compressed bytes, which are
    on the host by then).  The compressed sizes are not known to the host when the copy is enqueued, so the copy covers every frame's
    whole slot (`eavsr_png_capacity`); a copy sized to the data would need a wait in between.  A buffer is reused by the job after
    the next one: take a job's files before enqueueing the second job after it."""

    def __init__(self, stripe_rows: int = 32):
        self.stripe_rows = stripe_rows
        self.slots = [None, None]      # (pinned bytes, pinned sizes)
        self.turn = 0
        self.side = None

    def _slot(self, nbytes: int, frames: int):
        cur = self.slots[self.turn]
        if cur is None or cur[0].numel() < nbytes or cur[1].numel() < frames:
            cur = self.slots[self.turn] = (torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.empty(frames, dtype=torch.int64, pin_memory=True))
        self.turn ^= 1
        return cur

    def enqueue(self, rgb8: Tensor):
        from . import ops
        enc = ops.png_encode(rgb8, self.stripe_rows)      # refuses a CPU tensor before anything else happens
        f, h, w, c = (int(v) for v in rgb8.shape)
        host_bytes, host_sizes = self._slot(enc.data.numel(), f)
        device = rgb8.device
        if self.side is None or self.side.device != device:
            self.side = torch.cuda.Stream(device)
        self.side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(self.side):
            host_bytes[:enc.data.numel()].copy_(enc.data, non_blocking=True)
            host_sizes[:f].copy_(enc.sizes, non_blocking=True)
            done = torch.cuda.Event()
            done.record(self.side)
        enc.data.record_stream(self.side)
        enc.sizes.record_stream(self.side)
        return {"done": done, "bytes": host_bytes, "sizes": host_sizes, "frames": f, "cap": enc.data.numel() // max(f, 1), "hwc": (h, w, c)}

    @staticmethod
    def files(job) -> List[bytes]:
        job["done"].synchronize()
        h, w, c = job["hwc"]
        raw = job["bytes"].numpy()
        sizes = job["sizes"][:job["frames"]].tolist()
        return [_png_file(raw[i * job["cap"]:i * job["cap"] + n].tobytes(), h, w, c) for i, n in enumerate(sizes)]


_STAGING: Dict[int, "_PngStaging"] = {}


def _shared_staging(stripe_rows: int) -> "_PngStaging":
    """the staging object `encode_png_frames` reuses between calls (its pinned buffers grow to the largest item and stay); each
    call takes its files before it returns, so the two buffers are free again.  Not for concurrent use from several threads."""
    if stripe_rows not in _STAGING:
        _STAGING[stripe_rows] = _PngStaging(stripe_rows)
    return _STAGING[stripe_rows]


def encode_png_frames(rgb8: Tensor, stripe_rows: int = 32) -> List[bytes]:
    """uint8 device frames (F, H, W, C), C 1 or 3 (`ops.rgb8` / `ops.frame_metrics(.., rgb8=True)`) -> F complete PNG files as bytes:
    signature, IHDR, one IDAT, IEND.  Scanline filters and the entropy coder run on the device (`ops.png_encode`: per-row filter
    choice, Huffman coding without LZ77 matching); the host adds the chunk framing and CRC-32.  `read_png` and any PNG reader decode
    them; the pixels are the input's."""
    if not isinstance(rgb8, torch.Tensor) or rgb8.dim() != 4 or rgb8.dtype != torch.uint8:
        raise ValueError(f"encode_png_frames: uint8 (F, H, W, C), got {getattr(rgb8, 'dtype', type(rgb8))} {tuple(getattr(rgb8, 'shape', ()))}")
    staging = _shared_staging(stripe_rows)
    return staging.files(staging.enqueue(rgb8.contiguous()))


class _PngDecodeStaging:
    """The host side of the device PNG decoder: two pinned buffers used in turn, each with the event of the copy that last
    read it.  `slot(nbytes)` hands out the next buffer once that copy has ended, so a caller looping over chunks inflates chunk k + 1
    into one buffer while chunk k's copy and kernel still run from the other.  Not for concurrent use from several threads."""

    def __init__(self):
        self.slots = [None, None]      # [pinned bytes, event or None]
        self.turn = 0

    def slot(self, nbytes: int):
        cur = self.slots[self.turn]
        if cur is not None and cur[1] is not None:
            cur[1].synchronize()
            cur[1] = None
        if cur is None or cur[0].numel() < nbytes:
            cur = self.slots[self.turn] = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), None]
        self.turn ^= 1
        return cur


_DECODE_STAGING = _PngDecodeStaging()
_DECODE_POOLS: Dict[int, "object"] = {}


def _decode_pool(threads: Optional[int]):
    """the thread pool of `decode_png_frames`, kept between calls; sized by the CPUs this process may run on, never by the machine's"""
    if threads is None:
        threads = min(16, len(os.sched_getaffinity(0)))
    if isinstance(threads, bool) or not isinstance(threads, int) or threads < 1:
        raise ValueError(f"decode_png_frames: threads={threads!r}: a positive number of workers")
    if threads not in _DECODE_POOLS:
        from concurrent.futures import ThreadPoolExecutor
        _DECODE_POOLS[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="eavsr-png")
    return _DECODE_POOLS[threads]


def _png_item_name(item, i: int) -> str:
    return f"<bytes #{i}>" if isinstance(item, (bytes, bytearray, memoryview)) else os.fspath(item)


def inflate_png_frames(files, threads: Optional[int] = None):
    """The host half of `decode_png_frames`: read and `parse_png` every file, inflate every IDAT stream into one row of a pinned
    staging buffer (`zlib.decompress` releases the GIL: a thread pool), validate.  Returns (rows, h, w, c, slot): rows a pinned uint8
    (F, h, 1 + w c) view of the slot's buffer; set slot[1] to the event of the copy that reads it."""
    import numpy as np
    files = list(files)
    if not files:
        raise ValueError("decode_png_frames: no files")
    pool = _decode_pool(threads)
    names = [_png_item_name(f, i) for i, f in enumerate(files)]

    def parse(i):
        f = files[i]
        data = bytes(f) if isinstance(f, (bytes, bytearray, memoryview)) else open(os.fspath(f), "rb").read()
        return parse_png(data, names[i])
    parsed = list(pool.map(parse, range(len(files))))
    h, w, c, _ = parsed[0]
    for i, (hi, wi, ci, _) in enumerate(parsed):
        if (hi, wi, ci) != (h, w, c):
            raise ValueError(f"{names[i]}: {hi} x {wi} x {ci}, but {names[0]} is {h} x {w} x {c}: one call decodes frames of one size")
    r = 1 + w * c
    slot = _DECODE_STAGING.slot(len(files) * h * r)
    rows = slot[0][:len(files) * h * r].view(len(files), h, r)
    host = rows.numpy()

    def inflate(i):
        try:
            raw = zlib.decompress(parsed[i][3])
        except zlib.error as e:
            raise ValueError(f"{names[i]}: zlib: {e}") from None
        if len(raw) != h * r:
            raise ValueError(f"{names[i]}: the IDAT stream inflates to {len(raw)} bytes, {h} scanlines of 1 + {w} x {c} bytes are {h * r}")
        host[i] = np.frombuffer(raw, np.uint8).reshape(h, r)
    list(pool.map(inflate, range(len(files))))
    types = host[:, :, 0]
    if int(types.max()) > 4:
        i = int(np.argmax(types.max(1) > 4))
        raise ValueError(f"{names[i]}: scanline filter {int(types[i].max())}")
    return rows, h, w, c, slot


def decode_png_frames(files, device=None, channels: int = 3, out: Optional[Tensor] = None, threads: Optional[int] = None) -> Tensor:
    """PNG files -> uint8 (F, min(c, channels), H, W) planes ON THE DEVICE.  `files`: paths and / or `bytes` holding whole files, all
    non-interlaced 8-bit grey / RGB / RGBA of ONE size.  The host reads, walks the chunks (`parse_png`) and inflates (zlib in a pool of
    `threads` workers, default min(16, the CPUs this process may use)) into one of two pinned buffers; then ONE asynchronous copy and
    ONE launch (`ops.png_unfilter`) undo the scanline filters and leave the planes -- in `out` (for example store[lo:hi])
    when given.  Nothing waits for the device, so a loop over chunks inflates chunk k + 1 while chunk k is copied and unfiltered.
    channels=3 drops alpha as `read_png(p)[:3]` does.  ValueError naming the file, before anything is launched: a broken file
    (`parse_png`), frames of differing size, a zlib error, an inflated length other than h (1 + w c), a filter type above 4."""
    from . import ops
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 4:
        raise ValueError(f"decode_png_frames: channels={channels!r}: 1 .. 4")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError(f"decode_png_frames: device {dev}: the unfilter runs on the GPU only (`read_png` is the host decoder)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    rows, h, w, c, slot = inflate_png_frames(files, threads)
    f = int(rows.shape[0])
    if channels == 4 and c != 4:
        raise ValueError(f"decode_png_frames: channels=4 needs RGBA files, these have {c} bytes per pixel")
    shape = (f, min(c, channels), h, w)
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape
                            or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"decode_png_frames: out: a contiguous uint8 {shape} tensor on {dev}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    with torch.cuda.device(dev):
        dev_rows = torch.empty(tuple(rows.shape), device=dev, dtype=torch.uint8)
        dev_rows.copy_(rows, non_blocking=True)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(dev))
        slot[1] = done
        return ops.png_unfilter(dev_rows, c, channels, out=out)


def _write_file(path: str, data: bytes) -> str:
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    return path


def save_visuals(res: Dict[str, Tensor], fnames: Sequence, root: str, load_iter="0", full_res: bool = False) -> List[str]:
    """The frame writing of test_basic.py:85-92 for one test item: frame i of `res['data_sr_seq'][0]` goes to
    `<root>/sr_{full|patch}_<load_iter>/<fname[i][0][:3]>/<fname[i][0][-9:]>` (the scene is the first three characters of the
    frame's file name, the file its last nine: `000/00000.png`-style names of the datasets).  `root` is the reference's
    `./ckpt/<opt.name>`; `fnames` the item's `data['fname']` (a list of one-element lists / tuples, as the DataLoader collates
    them, or plain strings).  Returns the written paths."""
    seq = res["data_sr_seq"]
    if seq.dim() != 5:
        raise ValueError(f"save_visuals: data_sr_seq must be (n, t, c, h, w), got {tuple(seq.shape)}")
    paths = []
    for i in range(seq.shape[1]):
        name = fnames[i]
        name = name[0] if isinstance(name, (list, tuple)) else name
        folder = os.path.join(root, "sr_%s_%s" % ("full" if full_res else "patch", load_iter), name[:3])
        paths.append(write_png(seq[0, i], os.path.join(folder, name[-9:])))
    return paths


def _frame_name(fnames, i: int, b: int = 0) -> str:
    """name of frame i of batch entry b in an item's `fname` (a list of per-frame names, each a string or the one-element list /
    tuple the DataLoader collates it into)"""
    if isinstance(fnames, str) or fnames is None or len(fnames) <= i:
        raise ValueError(f"fname: one name per frame is needed, got {fnames!r} for frame {i}")
    name = fnames[i]
    return name[b] if isinstance(name, (list, tuple)) else name


def save_frames_rgb8(rgb8: Tensor, fnames: Sequence, root: str, load_iter="0", full_res: bool = False, encoder: str = "host") -> List[str]:
    """`save_visuals` for frames that already are 8-bit interleaved: rgb8 (t, H, W, C) uint8, the quantised frames of one item as
    `ops.frame_metrics(..., rgb8=True)` / `ops.rgb8` leave them; the same paths (test_basic.py:85-92).  encoder="device": the files
    come from `encode_png_frames` (the frames must be on the device) -- other bytes, the same pixels."""
    check_png_encoder(encoder)
    if rgb8.dim() != 4 or rgb8.dtype != torch.uint8:
        raise ValueError(f"save_frames_rgb8: uint8 (t, H, W, C), got {rgb8.dtype} {tuple(rgb8.shape)}")
    files = encode_png_frames(rgb8) if encoder == "device" else None
    frames = rgb8.cpu() if files is None else rgb8      # one copy for the item
    paths = []
    for i in range(frames.shape[0]):
        name = _frame_name(fnames, i)
        folder = os.path.join(root, "sr_%s_%s" % ("full" if full_res else "patch", load_iter), name[:3])
        if files is None:
            paths.append(write_png(frames[i], os.path.join(folder, name[-9:]), hwc=True))
        else:
            paths.append(_write_file(os.path.join(folder, name[-9:]), files[i]))
    return paths


def frame_metrics(sr_seq: Tensor, hr_seq: Tensor, scale: float = 255.0, lpips=None, niqe=None, niqe_crop: int = 0) -> Dict[str, List[float]]:
    """PSNR and SSIM of every frame on its own, as psnr_total.py:39-44 scores the stored PNG files: sr_seq / hr_seq (n, t, C, H, W)
    device tensors (scale 255: the model's [0, 1] output and target; scale 1: `get_current_visuals()` tensors), quantised to the
    8-bit image inside the kernel (`ops.frame_metrics`).  PSNR = -10 log10(sse / (C H W) / 255^2) in float64 on the host from the
    kernel's exact integer sse (`inf` for identical frames); SSIM is skimage's gaussian-window definition in fp64 (`calc_ssim`).
    Returns {'psnr': [...], 'ssim': [...]} in (n, t) order; with `lpips` (an `eavsr_amd.lpips.LPIPSAlex` on the tensors' device)
    also 'lpips': the AlexNet LPIPS of every frame pair on the same 8-bit images (psnr_total.py:27-35); with `niqe` (an
    `eavsr_amd.niqe.NIQE`, or what `niqe_scorer` makes one from) also 'niqe': the no-reference score of every SR frame on the same
    8-bit image, `niqe_crop` pixels removed on every side."""
    from . import ops
    if niqe is not None:
        niqe = niqe_scorer(niqe, None, "frame_metrics")
    if sr_seq.dim() != 5 or sr_seq.shape != hr_seq.shape:
        raise ValueError(f"frame_metrics: (n, t, C, H, W) tensors of one shape, got {tuple(sr_seq.shape)} / {tuple(hr_seq.shape)}")
    c, h, w = (int(v) for v in sr_seq.shape[2:])
    sse, ssim, _ = ops.frame_metrics(sr_seq.detach().reshape(-1, c, h, w), hr_seq.detach().reshape(-1, c, h, w), scale)
    out = {"psnr": [psnr_from_sse(v, c * h * w) for v in sse.tolist()], "ssim": ssim.tolist()}
    if lpips is not None:
        out["lpips"] = lpips(sr_seq.detach().reshape(-1, c, h, w), hr_seq.detach().reshape(-1, c, h, w), scale).tolist()
    if niqe is not None:
        out["niqe"] = niqe(sr_seq.detach().reshape(-1, c, h, w), scale, niqe_crop)
    return out


# -- NIQE, the no-reference column ---------------------------------------------------------------------------------------------
def niqe_option(opt=None):
    """(`opt.niqe_path`, else EAVSR_NIQE=<path>, else None: NIQE is off and nothing is launched for it;  `opt.niqe_crop`, else 0)"""
    from .segments import read_option, whole_number

    def a_path(value, who):
        if not isinstance(value, (str, os.PathLike)) or not os.fspath(value):
            raise ValueError(f"{who}={value!r}: the file name of a pristine model (see niqe.load_niqe_params)")
        return os.fspath(value)
    path = read_option(opt, "niqe_path", "EAVSR_NIQE", a_path, a_path)
    crop = getattr(opt, "niqe_crop", None)
    return path, (0 if crop is None else whole_number(0, "a number of pixels >= 0")(crop, "opt.niqe_crop"))


def niqe_scorer(niqe, opt=None, who: str = "niqe"):
    """The scorer behind `niqe=`: an `eavsr_amd.niqe.NIQE` as it is; a file name or a mapping, read with `niqe.load_niqe_params`;
    True: `opt.niqe_path`.  A missing or malformed file is a ValueError that names it -- raised before anything is launched."""
    from .niqe import NIQE
    if isinstance(niqe, NIQE):
        return niqe
    if niqe is True:
        niqe = getattr(opt, "niqe_path", None)
        if niqe is None:
            raise ValueError(f"{who}: niqe=True reads the pristine model from opt.niqe_path, and the options carry none "
                             "(no pristine model ships with this project)")
    if isinstance(niqe, (str, os.PathLike)) or hasattr(niqe, "keys"):
        return NIQE(niqe)
    raise ValueError(f"{who}: niqe={niqe!r}: a niqe.NIQE, the file name of a pristine model, a mapping, or True (opt.niqe_path)")


def _resolve_niqe(niqe, niqe_crop, opt, who: str):
    """(scorer or None, crop) for the `niqe=` / `niqe_crop=` arguments of `evaluate` and `super_resolve`: an argument left None is
    `niqe_option`'s; niqe=False is off whatever the options say."""
    opt_path, opt_crop = niqe_option(opt)
    if niqe is None:
        niqe = opt_path
    if niqe_crop is None:
        niqe_crop = opt_crop
    if isinstance(niqe_crop, bool) or not isinstance(niqe_crop, int) or niqe_crop < 0:
        raise ValueError(f"{who}: niqe_crop={niqe_crop!r}: a number of pixels >= 0")
    if niqe is None or niqe is False:
        return None, niqe_crop
    return niqe_scorer(niqe, opt, who), niqe_crop


def _niqe_values(niqe, parts) -> List[float]:
    """The scores of the frames behind `parts` = [(frames, `NIQE.moments` of them on the device, or None), ...], in order: the
    moments are read back once (per frame size), at the end, so nothing waits for the device while the frames are produced."""
    held = [m for _, m in parts if m is not None]
    if held and all(m.shape[1:] == held[0].shape[1:] for m in held):
        host = torch.cat(held, 0).cpu().numpy()
        host = iter(np.split(host, np.cumsum([int(m.shape[0]) for m in held])[:-1]))
    else:
        host = iter([m.cpu().numpy() for m in held])
    out: List[float] = []
    for count, m in parts:
        out += [math.nan] * count if m is None else niqe.scores(next(host))
    return out


# -- temporal consistency: warping error and tOF of consecutive frames -----------------------------------------------------
TEMPORAL_FLOWS = ("hr", "sr")
# padded image pixels one PWC-Net call may hold (its level buffers take about 200 bytes per image pixel): the pairs of a clip are
# estimated this many at a time.  A pair's flow does not depend on the split (every pwc.hip kernel computes an output sample from
# its own pair alone, in an order that does not look at the batch), so this bounds memory and nothing else.
_FLOW_PIXELS = 1 << 22


def check_temporal_flow(flow_from, what: str = "flow_from") -> Optional[str]:
    if flow_from is not None and flow_from not in TEMPORAL_FLOWS:
        raise ValueError(f"{what}={flow_from!r}: 'hr' (flows of the ground truth), 'sr' (flows of the output itself) or None")
    return flow_from


def temporal_option(opt=None):
    """`opt.temporal` -- True, "hr" or "sr" (a flow source also switches the metric on); False is off -- else EAVSR_TEMPORAL=hr|sr,
    else None: the temporal metrics are off and nothing is launched for them."""
    from .segments import read_option, one_of
    value = read_option(opt, "temporal", "EAVSR_TEMPORAL", one_of((True, False) + TEMPORAL_FLOWS, "True, 'hr', 'sr' or None"),
                        one_of(TEMPORAL_FLOWS, "hr or sr (or unset)"))
    return None if value is False else value


def temporal_net(temporal, opt=None, device=None, who: str = "temporal"):
    """The PWC-Net behind `temporal=`: a `pwc.PWCNET` as it is, a path read with `pwc.load_pwc_weights`, True: `opt.pwc_path`.
    A missing file is a ValueError that names it -- raised before anything is launched."""
    from . import pwc
    if isinstance(temporal, pwc.PWCNET):
        return temporal
    if temporal is True:
        path = getattr(opt, "pwc_path", None)
        if path is None:
            raise ValueError(f"{who}: temporal=True reads the PWC-Net weights from opt.pwc_path, and the options carry none "
                             "(no PWC-Net weights ship with this project)")
    elif isinstance(temporal, (str, os.PathLike)):
        path = temporal
    else:
        raise ValueError(f"{who}: temporal={temporal!r}: a pwc.PWCNET, the path of its weights, or True (opt.pwc_path)")
    path = os.fspath(path)
    if not os.path.isfile(path):
        raise ValueError(f"{who}: PWC-Net weights {path!r} not found (no PWC-Net weights ship with this project: name the file)")
    net = pwc.load_pwc_weights(pwc.PWCNET(), path).to(device).eval()
    for p in net.parameters():
        p.requires_grad_(False)
    return net


def _check_flow_frames(frames, who: str):
    if not isinstance(frames, torch.Tensor) or frames.dim() != 4 or int(frames.shape[0]) < 2:
        raise ValueError(f"{who}: frames are an (F, 3, H, W) tensor with F >= 2, got "
                         f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames)}")
    if int(frames.shape[1]) != 3:
        raise ValueError(f"{who}: PWC-Net reads RGB frames: C = {int(frames.shape[1])}, only C = 3 is accepted")


def _flows(frames: Tensor, net, scale: float, backward: bool):
    """(fw, bw or None) of the F - 1 consecutive pairs of frames (F, 3, H, W): both directions of as many pairs as _FLOW_PIXELS
    allows share one `pwc.estimate` call (rows [0, p): t -> t + 1, rows [p, 2p): t + 1 -> t)."""
    from . import pwc
    f, _, h, w = (int(v) for v in frames.shape)
    x = frames.detach().to(torch.float32)
    if float(scale) != 255.0:      # scale takes a sample to 0 .. 255 (ops.frame_metrics); PWC-Net reads [0, 1]
        x = x * (float(scale) / 255.0)
    hp, wp = -(-h // 64) * 64, -(-w // 64) * 64
    per_call = max(1, _FLOW_PIXELS // ((4 if backward else 2) * hp * wp))
    fw = torch.empty((f - 1, 2, h, w), device=x.device, dtype=torch.float32)
    bw = torch.empty_like(fw) if backward else None
    with torch.no_grad():
        for a in range(0, f - 1, per_call):
            p = min(per_call, f - 1 - a)
            first, second = x[a:a + p], x[a + 1:a + 1 + p]
            if backward:
                flow = pwc.estimate(torch.cat([first, second], 0), torch.cat([second, first], 0), net)
                fw[a:a + p].copy_(flow[:p])
                bw[a:a + p].copy_(flow[p:])
            else:
                fw[a:a + p].copy_(pwc.estimate(first, second, net))
    return fw, bw


def pair_flows(frames: Tensor, net, scale: float = 255.0):
    """The optical flow between consecutive frames, both ways, by the project's PWC-Net (`pwc.estimate`): frames (F, 3, H, W) on the
    device (scale 255: samples in [0, 1]; scale 1: 0 .. 255) -> (fw, bw), each (F - 1, 2, H, W) in pixels, channel 0 = x; fw[t] is
    the flow t -> t + 1, bw[t] the flow t + 1 -> t.  A pair's flow is the same bits whether it is estimated alone or with others."""
    _check_flow_frames(frames, "pair_flows")
    return _flows(frames, net, scale, True)


def _temporal_device(sr: Tensor, hr: Optional[Tensor], net, scale: float, flow_from: str):
    """(err, count, epe or None) of `ops.temporal_metrics` for one clip sr (F, C, H, W) [/ hr of the same shape], on the device"""
    from . import ops
    if flow_from == "hr":
        fw, bw = _flows(hr, net, scale, True)
        flow_b = _flows(sr, net, scale, False)[0]
    else:
        (fw, bw), flow_b = _flows(sr, net, scale, True), None
    return ops.temporal_metrics(sr.detach(), fw, bw, scale, flow_b)


def temporal_values(err, count, epe, c: int, h: int, w: int) -> Dict[str, List]:
    """The sums of `ops.temporal_metrics` as the report's numbers, in float64 on the host: 'ewarp' = err / (C count) / 255^2 (`nan`
    where no pixel is valid), 'valid' = count / (H W), 'tof' = epe / (H W) (None without epe)."""
    err, count = [float(v) for v in err], [int(v) for v in count]
    out = {"ewarp": [e / (c * n) / (255.0 * 255.0) if n else math.nan for e, n in zip(err, count)],
           "valid": [n / (h * w) for n in count], "tof": None}
    if epe is not None:
        out["tof"] = [float(v) / (h * w) for v in epe]
    return out


def _resolve_flow_from(flow_from, has_hr: bool, who: str) -> str:
    check_temporal_flow(flow_from, f"{who}: flow_from")
    if flow_from is None:
        return "hr" if has_hr else "sr"
    if flow_from == "hr" and not has_hr:
        raise ValueError(f"{who}: flow_from='hr' needs the HR frames (flow_from='sr' scores footage without ground truth)")
    return flow_from


def temporal_metrics(sr_seq: Tensor, hr_seq: Optional[Tensor], net, scale: float = 255.0, flow_from: Optional[str] = None) -> Dict:
    """Temporal consistency of every pair of consecutive frames: sr_seq (n, t, 3, H, W) [hr_seq of the same shape, or
    None] on the device, `net` a `pwc.PWCNET` -> {'ewarp', 'valid', 'tof'}, lists in (n, t - 1) order.
    'ewarp': the warping error -- frame t + 1 warped back to frame t along the flow, mean squared difference of the 8-bit images over
    the pixels that are neither occluded, nor on a motion boundary, nor out of frame, over 255^2 (`nan` where none is left);
    'valid': the share of such pixels; 'tof': the mean endpoint distance between the SR pair's flow and the HR pair's.
    flow_from="hr" (the default where hr_seq is given): the warp and its mask use the HR frames' flows, and tOF is reported;
    "sr" (footage without ground truth): the SR frames' own flows, 'tof' is None.  The flows are PWC-Net's (`pair_flows`): the
    values are this project's own and compare with nothing computed with another estimator."""
    if not isinstance(sr_seq, torch.Tensor) or sr_seq.dim() != 5 or (hr_seq is not None and hr_seq.shape != sr_seq.shape):
        raise ValueError("temporal_metrics: (n, t, 3, H, W) tensors of one shape, got "
                         f"{tuple(sr_seq.shape)} / {None if hr_seq is None else tuple(hr_seq.shape)}")
    flow_from = _resolve_flow_from(flow_from, hr_seq is not None, "temporal_metrics")
    n, t, c, h, w = (int(v) for v in sr_seq.shape)
    if t < 2:
        raise ValueError(f"temporal_metrics: {t} frame(s): a pair needs two")
    _check_flow_frames(sr_seq[0], "temporal_metrics")
    out = {"ewarp": [], "valid": [], "tof": [] if flow_from == "hr" else None}
    parts = [_temporal_device(sr_seq[b], hr_seq[b] if flow_from == "hr" else None, net, scale, flow_from) for b in range(n)]
    for err, count, epe in parts:
        vals = temporal_values(err.tolist(), count.tolist(), None if epe is None else epe.tolist(), c, h, w)
        out["ewarp"] += vals["ewarp"]
        out["valid"] += vals["valid"]
        if epe is not None:
            out["tof"] += vals["tof"]
    return out


def psnr_from_sse(sse: int, count: int, range: float = 255.0) -> float:
    """-10 log10(sse / count / range^2) in float64 (psnr_total.py:13-20 on the 8-bit image); `inf` when sse == 0"""
    return math.inf if sse == 0 else -10.0 * math.log10(sse / count / (range * range))


TEMPORAL_COLUMNS = ("ewarp", "tof")


def scene_report(names: Sequence[str], psnr: Optional[Sequence[float]], ssim: Optional[Sequence[float]],
                 lpips: Optional[Sequence[float]] = None, temporal: Optional[Dict] = None, niqe: Optional[Sequence[float]] = None) -> Dict:
    """The averaging of psnr_total.py:89-133 (host only): frames are grouped by the scene in the first three characters of their
    name, every scene's frames are averaged, then the scene means are averaged -- NOT the frames, so a short scene weighs as much
    as a long one.  Returns {'frames': [{'name', 'scene', 'psnr', 'ssim'}, ...] in the given order, 'scenes': {scene: {'psnr',
    'ssim', 'frames': count}} sorted by scene, 'final': {'psnr', 'ssim', 'scenes': count}}.
    With `lpips` (one value per frame: the third column of the reference's log, psnr_total.py:116-138) every frame, every scene and
    'final' carry an 'lpips' field as well, averaged exactly as the other two; without it the report has no such field.
    With `temporal` = {'ewarp': [...], 'tof': [...] or None} (one entry per frame: the pair (previous frame, this
    frame), None for a frame that has no predecessor in its clip) every frame, scene and 'final' carry 'ewarp' and 'tof': a scene's
    mean runs over its entries that are not None, the final mean over the scene means that are not None; None where there is none.
    A pair without a valid pixel has the warping error `nan`: the frame keeps it, the means leave it out as they leave out None (one
    fully masked pair does not turn a column into `nan`).  Without it the report has no such fields.
    With `niqe` (one score per frame, `nan` for a frame too small to score) every frame, scene and 'final' carry 'niqe':
    the frame keeps a `nan`, the means leave it out as the temporal columns do; None where nothing is left.  Footage without
    ground truth: psnr = ssim = None (both; `niqe` is then required) -- no row, scene or 'final' has a 'psnr' / 'ssim' field at
    all, they carry the names, the counts and 'niqe'; `lpips` and `temporal` keep their meaning."""
    if (psnr is None) != (ssim is None):
        raise ValueError("scene_report: psnr and ssim are given together or both None")
    scored = psnr is not None
    if not scored:
        if niqe is None:
            raise ValueError("scene_report: without psnr / ssim the report needs niqe")
        psnr = ssim = [math.nan] * len(names)
    if niqe is not None and len(niqe) != len(names):
        raise ValueError(f"scene_report: {len(names)} names and {len(niqe)} NIQE values")
    if not (len(names) == len(psnr) == len(ssim)):
        raise ValueError(f"scene_report: {len(names)} names, {len(psnr)} PSNR and {len(ssim)} SSIM values")
    if lpips is not None and len(lpips) != len(names):
        raise ValueError(f"scene_report: {len(names)} names and {len(lpips)} LPIPS values")
    if temporal is not None:
        temporal = {k: ([None] * len(names) if temporal.get(k) is None else list(temporal[k])) for k in TEMPORAL_COLUMNS}
        for k, v in temporal.items():
            if len(v) != len(names):
                raise ValueError(f"scene_report: {len(names)} names and {len(v)} {k} entries")
    frames = [{"name": str(nm), "scene": str(nm)[:3], "psnr": float(p), "ssim": float(s)} for nm, p, s in zip(names, psnr, ssim)]
    cols = ["psnr", "ssim"]
    if not scored:
        cols = []
        for fr in frames:
            del fr["psnr"], fr["ssim"]
    if lpips is not None:
        cols.append("lpips")
        for fr, v in zip(frames, lpips):
            fr["lpips"] = float(v)
    mean = lambda v: sum(v) / len(v) if v else math.nan
    scenes = {}
    for scene in sorted({fr["scene"] for fr in frames}):
        rows = [fr for fr in frames if fr["scene"] == scene]
        scenes[scene] = {**{k: mean([r[k] for r in rows]) for k in cols}, "frames": len(rows)}
    final = {**{k: mean([v[k] for v in scenes.values()]) for k in cols}, "scenes": len(scenes)}
    if temporal is not None:
        some = lambda v: sum(v) / len(v) if v else None
        has = lambda v: v is not None and math.isfinite(v)
        for k in TEMPORAL_COLUMNS:
            for fr, v in zip(frames, temporal[k]):
                fr[k] = None if v is None else float(v)
            for scene, row in scenes.items():
                row[k] = some([fr[k] for fr in frames if fr["scene"] == scene and has(fr[k])])
            final[k] = some([row[k] for row in scenes.values() if row[k] is not None])
    if niqe is not None:
        some = lambda v: sum(v) / len(v) if v else None
        for fr, v in zip(frames, niqe):
            fr["niqe"] = float(v)
        for scene, row in scenes.items():
            row["niqe"] = some([fr["niqe"] for fr in frames if fr["scene"] == scene and math.isfinite(fr["niqe"])])
        final["niqe"] = some([row["niqe"] for row in scenes.values() if row["niqe"] is not None])
    return {"frames": frames, "scenes": scenes, "final": final}


def write_metrics_log(report: Dict, path: str) -> str:
    """A `scene_report` as a text file: per scene its frames and its mean, then the final line; PSNR to 2 decimals and SSIM to 4,
    the precision of the reference's log (psnr_total.py:116-138), in this project's own layout.  A report with LPIPS (see
    `scene_report`) gets `  lpips %.3f` at the end of every line, the reference's three decimals; one without it produces the
    file it always produced.  A report with the temporal columns gets `  ewarp %.6f  tof %.4f` after that, `-` where a row has no
    value (a frame without a predecessor; tOF without HR flows).  A report with NIQE gets `  niqe %.4f` after that, `-` where the
    value is `nan` or absent; a report without PSNR / SSIM (footage without ground truth) has no `psnr` / `ssim` cells."""
    lines = []
    cell = lambda fmt, v: "-" if v is None else fmt % v
    scored = "psnr" in report["final"]
    first = lambda row: "  psnr %.2f  ssim %.4f" % (row["psnr"], row["ssim"]) if scored else ""

    def third(row):
        text = "  lpips %.3f" % row["lpips"] if "lpips" in report["final"] else ""
        if "ewarp" in report["final"]:
            text += "  ewarp %s  tof %s" % (cell("%.6f", row["ewarp"]), cell("%.4f", row["tof"]))
        if "niqe" in report["final"]:
            text += "  niqe %s" % cell("%.4f", None if row["niqe"] is None or row["niqe"] != row["niqe"] else row["niqe"])
        return text
    for scene, mean in report["scenes"].items():
        lines.append(f"scene {scene}")
        for fr in report["frames"]:
            if fr["scene"] == scene:
                lines.append("  %s" % fr["name"] + first(fr) + third(fr))
        lines.append("  mean of %d frames" % mean["frames"] + first(mean) + third(mean))
    final = report["final"]
    lines.append("final, mean of %d scenes" % final["scenes"] + first(final) + third(final))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def test_window_starts(n_images: int, n_seq: int, n_frame: int) -> List[int]:
    """First frame of every test item (mvsr4x_dataset.py:130-136): each scene of `n_seq` consecutive frames is cut
    into n_seq / n_frame non-overlapping windows of n_frame frames.  Raises as the reference does when n_seq is not
    a multiple of n_frame."""
    if n_seq % n_frame != 0:
        raise ValueError(f"n_seq {n_seq} is not a multiple of n_frame {n_frame}")
    per_scene = n_seq // n_frame
    index = [i * n_frame for i in range(per_scene)]
    n_items = (n_images // n_seq) * per_scene
    return [(i // per_scene) * n_seq + index[i % per_scene] for i in range(n_items)]


def train_window(idx: int, frame: int, n_frame: int, n_seq: int) -> List[int]:
    """Image indices of the training / validation item whose key frame is image `idx`, the `frame`-th frame of its
    scene of `n_seq` frames (mvsr4x_dataset.py:62-90, :97-125): a window of n_frame frames centred on the key frame;
    at the first / last frames of a scene the missing neighbours are mirrored about the key frame, so the window
    never crosses into another scene."""
    half = n_frame // 2
    out = [0] * n_frame
    if frame - half < 0:                      # front of the scene
        for i in range(half - frame):
            out[i] = idx + half - i
        for i in range(half - frame, n_frame):
            out[i] = idx + i - half
    elif frame + half >= n_seq:               # back of the scene
        for i in range(half, (n_seq - 1) - frame, -1):
            out[i + half] = idx - i
        for i in range(half + n_seq - frame):
            out[i] = idx + i - half
    else:
        for i in range(n_frame):
            out[i] = idx + i - half
    return out


def crop_center(img: Tensor, p: int) -> Tensor:
    """Centre p x p crop of an (..., H, W) tensor (the `_crop_center` of the training items, mvsr4x_dataset.py:123-124)."""
    h, w = img.shape[-2:]
    top, left = (h - p) // 2, (w - p) // 2
    return img[..., top:top + p, left:left + p]


def evaluate(model, items: Iterable[Dict], calc_psnr_flag: bool = True, calc_ssim_flag: bool = False,
             save_root: Optional[str] = None, load_iter="0", full_res: bool = False, per_frame: bool = False, lpips=None,
             temporal=None, temporal_flow: Optional[str] = None, niqe=None, niqe_crop: Optional[int] = None) -> Dict:
    """The timed loop of test_basic.py:56-83 for a model wrapper (EAVSRPModel / EAVSRPx2Model); with `save_root` the frames are
    written as the reference's `--save_imgs` does (test_basic.py:85-92, `save_visuals`); `calc_ssim_flag` adds psnr_total.py's SSIM
    per item (mean over the item's frames).

    Every item is a `{'lr_seq': (n,t,3,h,w), 'hr_seq': (n,t,3,sh,sw), 'fname': ...}` dict in [0,1].  Returns the
    per-item PSNR list, their mean, the wall time of the `model.test()` calls (device-synchronised on both sides,
    as the reference's) and frames/s over all items (the reference discards its first iteration inside
    `EAVSRPModel.forward`, eavsrp_model.py:104-107; `model.time` / `model.num` keep that convention).

    `per_frame=True` scores with the fused kernel instead (`ops.frame_metrics` on `model.data_sr_seq` / `data_hr_seq`, no
    `get_current_visuals` pass): the per-item 'psnr' / 'ssim' keep their meaning (the item's PSNR from the summed squared error, the
    mean of its frames' SSIM), and the result gains 'frame_psnr' / 'frame_ssim' (every frame on its own, in item, n, t order),
    'frame_names' and 'report' -- psnr_total.py's per-scene and final means (`scene_report`) over the items' `fname`s, which must
    then name every frame.  With `save_root` the PNG files are written from the kernel's 8-bit frames.

    `lpips` (with `per_frame=True` only; it raises otherwise): an `eavsr_amd.lpips.LPIPSAlex`, or the path of its weights (one file
    in the lpips package's state-dict layout, see `lpips.load_lpips_weights`), read once; the default is `model.opt.lpips_path`
    where the options have one.  The result then gains 'frame_lpips' and the report its 'lpips' column (psnr_total.py:27-35, every
    frame pair on the same 8-bit images).  Items without HR frames are skipped, as they are for PSNR and SSIM.

    `temporal` (with `per_frame=True` only; it raises otherwise): a `pwc.PWCNET`, the path of its weights, or True
    (`opt.pwc_path`); the default is `opt.temporal` / EAVSR_TEMPORAL (`temporal_option`).  Every pair of consecutive frames inside
    an item, separately for each batch entry, is scored with `temporal_metrics` (`temporal_flow`: its `flow_from`): the result gains
    'frame_ewarp' / 'frame_tof' / 'frame_valid' -- one entry per frame, None for an item's first frame -- and the report its
    'ewarp' / 'tof' columns.  Unset, nothing is launched for it and the result is what it was.

    `niqe` (with `per_frame=True` only; it raises otherwise): an `eavsr_amd.niqe.NIQE`, the file name of a pristine model, or
    True (`opt.niqe_path`); the default is `opt.niqe_path` / EAVSR_NIQE (`niqe_option`); `niqe_crop` (default `opt.niqe_crop`, else
    0) pixels are removed on every side.  Every SR frame of an item with HR frames is scored: the result gains 'frame_niqe' and the
    report its 'niqe' column.  Unset, nothing is launched for it and the result is what it was."""
    if niqe is not None and niqe is not False and not per_frame:
        raise ValueError("evaluate: niqe needs per_frame=True (NIQE is part of the per-frame report)")
    niqe, niqe_crop = _resolve_niqe(niqe, niqe_crop, getattr(model, "opt", None), "evaluate") if per_frame else (None, 0)
    niqe_parts = []
    if lpips is not None and not per_frame:
        raise ValueError("evaluate: lpips needs per_frame=True (LPIPS is part of the per-frame report)")
    if temporal is False:
        temporal = None
    if temporal is not None and not per_frame:
        raise ValueError("evaluate: temporal needs per_frame=True (the temporal metrics are part of the per-frame report)")
    check_temporal_flow(temporal_flow, "evaluate: temporal_flow")
    if temporal is None and per_frame:
        temporal = temporal_option(getattr(model, "opt", None))
        if temporal in TEMPORAL_FLOWS:
            temporal, temporal_flow = True, (temporal if temporal_flow is None else temporal_flow)
    if temporal is not None:
        temporal = temporal_net(temporal, getattr(model, "opt", None), model.device, "evaluate")
    frame_temporal = {"ewarp": [], "tof": [], "valid": []}
    if lpips is None and per_frame:
        lpips = getattr(getattr(model, "opt", None), "lpips_path", None)
    if isinstance(lpips, (str, os.PathLike)):
        from .lpips import build_lpips
        lpips = build_lpips(os.fspath(lpips), device=model.device)
    frame_lpips: List[float] = []
    model.eval()
    checked_net = getattr(model, "netEAVSRP", None) if getattr(model, "backbone_check", None) is not None else None
    if checked_net is not None:
        checked_net.backbone_census = []
    psnr: List[float] = []
    ssim: List[float] = []
    written: List[str] = []
    frame_psnr: List[float] = []
    frame_ssim: List[float] = []
    frame_names: List[str] = []
    seconds = 0.0
    frames = 0
    for data in items:
        model.set_input(data, 0)
        torch.cuda.synchronize()
        t0 = time.time()
        model.test()
        torch.cuda.synchronize()
        seconds += time.time() - t0
        frames += int(model.data_sr_seq.shape[0] * model.data_sr_seq.shape[1])
        if per_frame:
            from . import ops
            sr = model.data_sr_seq.detach()
            n, t, c, h, w = (int(v) for v in sr.shape)
            rgb8 = None
            if model.data_hr_seq is not None:
                hr = model.data_hr_seq.detach()
                sse, fs, rgb8 = ops.frame_metrics(sr.reshape(n * t, c, h, w), hr.reshape(n * t, c, h, w), 255.0,
                                                  rgb8=save_root is not None)
                sse, fs = sse.tolist(), fs.tolist()
                frame_psnr += [psnr_from_sse(v, c * h * w) for v in sse]
                frame_ssim += fs
                if lpips is not None:
                    frame_lpips += lpips(sr.reshape(n * t, c, h, w), hr.reshape(n * t, c, h, w), 255.0).tolist()
                if niqe is not None:
                    niqe_parts.append((n * t, niqe.moments(sr.reshape(n * t, c, h, w), 255.0, niqe_crop)))
                if temporal is not None:
                    vals = ({"ewarp": [], "valid": [], "tof": None} if t < 2 else
                            temporal_metrics(model.data_sr_seq.detach(), hr, temporal, 255.0, temporal_flow))
                    for k in frame_temporal:
                        for b in range(n):
                            frame_temporal[k] += [None] + ([None] * (t - 1) if vals[k] is None else vals[k][b * (t - 1):(b + 1) * (t - 1)])
                frame_names += [_frame_name(data.get("fname"), i, b) for b in range(n) for i in range(t)]
                if calc_psnr_flag:
                    psnr.append(psnr_from_sse(sum(sse), n * t * c * h * w))
                if calc_ssim_flag:
                    ssim.append(sum(fs) / len(fs))
            elif save_root is not None:
                rgb8 = ops.rgb8(sr.reshape(n * t, c, h, w), 255.0)
            if save_root is not None:
                written += save_frames_rgb8(rgb8[:t], data["fname"], save_root, load_iter, full_res)      # batch entry 0, as save_visuals
            continue
        res = None
        if (calc_psnr_flag or calc_ssim_flag) and model.data_hr_seq is not None:
            res = model.get_current_visuals()
            if calc_psnr_flag:
                psnr.append(calc_psnr(res["data_sr_seq"], res["data_hr_seq"]))
            if calc_ssim_flag:
                ssim.append(calc_ssim(res["data_sr_seq"], res["data_hr_seq"]))
        if save_root is not None:
            res = res if res is not None else model.get_current_visuals()
            written += save_visuals(res, data["fname"], save_root, load_iter, full_res)
    out = {
        "psnr": psnr,
        "psnr_mean": (sum(psnr) / len(psnr)) if psnr else math.nan,
        "ssim": ssim,
        "ssim_mean": (sum(ssim) / len(ssim)) if ssim else math.nan,
        "written": written,
        "seconds": seconds,
        "frames": frames,
        "frames_per_s": frames / seconds if seconds > 0 else math.nan,
    }
    if per_frame:
        frame_niqe = None if niqe is None else _niqe_values(niqe, niqe_parts)
        out.update(frame_psnr=frame_psnr, frame_ssim=frame_ssim, frame_names=frame_names,
                   report=scene_report(frame_names, frame_psnr, frame_ssim, frame_lpips if lpips is not None else None,
                                       **({} if temporal is None else {"temporal": frame_temporal}),
                                       **({} if niqe is None else {"niqe": frame_niqe})))
        if lpips is not None:
            out["frame_lpips"] = frame_lpips
        if niqe is not None:
            out["frame_niqe"] = frame_niqe
        if temporal is not None:
            out.update(frame_ewarp=frame_temporal["ewarp"], frame_tof=frame_temporal["tof"], frame_valid=frame_temporal["valid"])
    if checked_net is not None:      # opt.backbone_check (addendum): one entry per window of every item, and the one line
        from .networks import range_summary
        out.update(backbone_census=checked_net.backbone_census, backbone_range=range_summary(checked_net.backbone_census))
    return out


def explicit_cuts(cuts) -> List[int]:
    """The scene starts of `super_resolve(cuts=[...])` as `segments.plan_segments` takes them: sorted integers without a 0 -- frame 0
    starts a scene whether it is listed or not, so `cuts=[0]` is `cuts=[]` and `cuts=[0, 5]` is `cuts=[5]` (`plan_segments` itself
    refuses a 0, and goes on refusing every other start outside (0, t))."""
    return sorted(int(c) for c in cuts if int(c) != 0)


def scene_changes(frames, chunk: int = 64, device=None):
    """`ops.frame_change` of a clip that need not be on the device: uint8 frames (t, C, h, w), C 1 or 3, or (t, h, w, 3), in host or
    device memory -> (hist int32 (t, 64), sad int64 (t - 1,)) on the device, the same numbers as one call on the whole clip.  A
    host-resident clip is uploaded `chunk` frames at a time into one buffer of chunk + 1 frames, each chunk behind the previous
    chunk's last frame (the pair that straddles two chunks); a device-resident clip is read in place, chunk + 1 frames per call.
    With a leading clip dimension, (n, t, ...), the statistics are per clip: (n, t, 64) and (n, t - 1).  `device`: where a host clip
    goes (default: the current device)."""
    from . import ops
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() not in (4, 5):
        raise ValueError("scene_changes: a uint8 (t, C, h, w) or (t, h, w, 3) tensor, optionally with a leading n")
    if isinstance(chunk, bool) or not isinstance(chunk, int) or chunk < 1:
        raise ValueError(f"scene_changes: chunk {chunk!r}: a positive number of frames")
    if frames.dim() == 5:
        per_clip = [scene_changes(clip, chunk, device) for clip in frames]
        return torch.stack([h for h, _ in per_clip], 0), torch.stack([s for _, s in per_clip], 0)
    t = int(frames.shape[0])
    if t < 1:
        raise ValueError("scene_changes: at least one frame")
    hwc = frames.shape[3] == 3 and frames.shape[1] != 3
    if frames.is_cuda:
        device = frames.device
    else:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    buf = None if frames.is_cuda else torch.empty((min(chunk, t) + 1,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=device)
    hists, sads, held = [], [], 0      # held: frames of the previous chunk in buf[1:]
    for a in range(0, t, chunk):
        k = min(chunk, t - a)
        if frames.is_cuda:
            seq = frames[max(a - 1, 0):a + k]
        else:
            if a > 0:
                buf[0].copy_(buf[held])      # the previous chunk's last frame, ahead of the upload that overwrites it
            buf[1:1 + k].copy_(frames[a:a + k], non_blocking=True)
            seq, held = (buf[0:1 + k] if a > 0 else buf[1:1 + k]), k
        h, s = ops.frame_change(seq, hwc=hwc)
        hists.append(h if a == 0 else h[1:])
        sads.append(s)
    return torch.cat(hists, 0), torch.cat(sads, 0)


def resize_frames(frames, size):
    """The "Bicubic" row of an SR table: frames in the layouts `super_resolve` takes -- uint8 (t, 3, h, w) / (t, h, w, 3) or fp32 in
    [0, 1] (t, C, h, w), with or without a leading n, on the device -- resized to size = (H, W) or "HxW" by `resize.resize_frames`
    (MATLAB's antialiased bicubic `imresize`) -> fp32 in the same arrangement of planes, (.., C, H, W).  uint8 frames go
    through `ops.u8_to_f32` first, so the result is the fp32 path on v / 255 -- NOT MATLAB's uint8 path, which computes in double on
    0 .. 255 and rounds to a byte; nothing is clamped here."""
    from . import ops
    from .resize import check_out_size, resize_frames as _resize_frames
    size = check_out_size(tuple(size) if isinstance(size, list) else size, "resize_frames: size")
    if size is None:
        raise ValueError("resize_frames: size=None: (rows, columns) or 'HxW'")
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
        raise ValueError("resize_frames: frames is a (t, 3, h, w) tensor (uint8: also (t, h, w, 3)), optionally with a leading n")
    if not frames.is_cuda:
        raise RuntimeError(f"resize_frames: tensor is on {frames.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if frames.dtype == torch.uint8:
        lead = tuple(frames.shape[:-3])
        x = ops.u8_to_f32(frames.reshape((-1,) + tuple(frames.shape[-3:])))
        return _resize_frames(x.view(lead + tuple(x.shape[1:])), size)
    if not frames.is_floating_point():
        raise ValueError(f"resize_frames: frames is uint8 or floating point, got {frames.dtype}")
    return _resize_frames(frames.to(torch.float32), size)


@contextlib.contextmanager
def _backbone_checked(mode, net):
    """the body's forwards under `networks.backbone_check(mode)`, the network's `backbone_census` cleared first; None: nothing"""
    if mode is None:
        yield
        return
    from . import networks
    net.backbone_census = []
    with networks.backbone_check(mode):
        yield


def super_resolve(model, frames, out_dir: Optional[str] = None, hr=None, names: Optional[Sequence] = None,
                  frame_chunk: Optional[int] = None, cache: str = "device", lpips=None, png_encoder: Optional[str] = None,
                  png_decoder: Optional[str] = None, max_frames: Optional[int] = None, overlap: int = DEFAULT_OVERLAP, cuts=None,
                  cut_thresholds=None, min_scene: int = 2, pad: Optional[str] = None, tile=None,
                  tile_overlap: Optional[int] = None, ensemble=None, temporal=None, temporal_flow: Optional[str] = None, niqe=None,
                  niqe_crop: Optional[int] = None, cache_dtype=None, cache_check: Optional[str] = None, out_size=None) -> Dict:
    """Frames in, frames out: a whole scene through `EAVSRP.forward_long`, one chunk of frames at a time.

    `model` is a model wrapper (EAVSRPModel / EAVSRPx2Model) or the network itself.  `frames` is the scene: a list of PNG paths
    (`read_png`), or a tensor -- uint8 (t, 3, h, w) / (t, h, w, 3) or fp32 in [0, 1] (t, 3, h, w), with or without a leading clip
    dimension n, in host or device memory; 8-bit frames stay bytes until the device converts them (`ops.u8_to_f32`).
    `frame_chunk` / `cache` are `forward_long`'s.  The SR clip is never held as a whole: per finished chunk a sink
      * writes `<out_dir>/<name>` for every frame (of clip 0) from the kernel's 8-bit frames (`ops.rgb8`) when `out_dir` is given,
      * scores the chunk against `hr` (same layouts as `frames`, at the output size) with `ops.frame_metrics` -- and `lpips`, an
        `eavsr_amd.lpips.LPIPSAlex` or the path of its weights -- when `hr` is given.
    `png_encoder`: "host" (the default: `write_png`, zlib on one host thread, after a blocking copy of the frames) or "device"
    (filters and entropy coding on the device, `ops.png_encode`; the sink then enqueues the encoder and an asynchronous copy
    of the compressed bytes into one of two pinned buffers and waits for nothing; the files of a chunk are written when the next
    chunk has been enqueued, the last chunk's when the forward has ended).  None: `opt.png_encoder` of a model wrapper, else
    EAVSR_PNG_ENCODER, else "host".  The files differ in bytes, not in pixels; 'written' and the report are the same.
    `png_decoder`: who decodes `frames` / `hr` given as lists of paths -- "host" (the default: `read_png`, a Python loop per byte) or
    "device" (`decode_png_frames`, zlib in a thread pool and the scanline unfilter on the device; the 8-bit clip is then on
    the device already).  None: `opt.png_decoder` of a model wrapper, else EAVSR_PNG_DECODER, else "host".  The same pixels.
    `names`: one name per frame (default: the paths' base names, else `000_00000.png`, ...); a name's first three characters are its
    scene in the report.  Returns 'frames', 'seconds' (device-synchronised on both sides), 'frames_per_s', 'peak_bytes'
    (`torch.cuda.max_memory_allocated` over the run), 'written', and with `hr` the 'frame_psnr' / 'frame_ssim' / 'frame_names' /
    'report' (/ 'frame_lpips') of `evaluate(per_frame=True)`, in (n, t) order.

    Videos of any length, opt-in: `max_frames` bounds the frames one `forward_long` call sees -- a longer scene runs as
    windows of max_frames frames that share `overlap` frames (`segments.plan_segments`), so what is resident no longer grows with
    t; `cuts` keeps the recurrence from running across a scene change: "device" finds the cuts on the 8-bit frames (`scene_changes`
    + `segments.find_cuts` with `cut_thresholds` = (hist_threshold, sad_threshold), default the untuned constants of `segments`;
    one clip of uint8 frames only), a list names the scene starts.  Scenes shorter than `min_scene` join their predecessor.  Then
    `EAVSRP.forward_segments` feeds the same sink: files, metrics and LPIPS are unchanged, every frame is what `forward_long` gives
    for it on its window.  With max_frames and cuts both None -- and `opt.max_frames` / EAVSR_MAX_FRAMES, `opt.scene_cuts` /
    EAVSR_SCENE_CUTS unset (`segments.segment_options`; they stand in for arguments left None, and then `opt.segment_overlap` /
    EAVSR_SEGMENT_OVERLAP for `overlap`; a max_frames from the options without an overlap beside it takes
    min(overlap, max_frames // 2), so that EAVSR_MAX_FRAMES=8 alone is not refused for the default overlap of 8) -- the one
    `forward_long` call as before.  The result also carries 'segments' (the plan:
    (start, stop, emit_start, emit_stop) per window) and 'scene_starts'.

    Frames of any size, opt-in: `pad` = "reflect" / "edge" is `forward_long`'s -- frames whose sides are below 64 or no
    multiple of 4 are padded at the bottom and right while the device converts them and every SR chunk is cropped before the sink
    sees it, so `hr` is expected, and the files are written, at (s h, s w); the scene-cut statistics read the unpadded bytes.
    None: `opt.pad_frames` of a model wrapper, else EAVSR_PAD_FRAMES=reflect|edge, else off -- such sizes are refused as before.

    Frames of any resolution, opt-in: `tile` (LR pixels: an int, (rows, columns) or "288x512") runs the network on
    overlapped spatial tiles that share `tile_overlap` LR pixels and blends their SR frames (`EAVSRP.forward_tiled`), so memory
    follows the tile's area instead of the frame's; the same sink is fed, and it composes with `max_frames` / `cuts` / `pad`.  The
    output is the blend of per-tile results, not the whole-frame result.  An argument left None: `opt.tile` / `opt.tile_overlap`
    of a model wrapper, else EAVSR_TILE / EAVSR_TILE_OVERLAP (`segments.tile_options`), else no tiling / 32 pixels (a setting, not
    a measured optimum).  The result carries 'tiles': the plan's (y0, y1, x0, x1) windows (one window, the frame: not tiled).

    Self-ensemble, opt-in: `ensemble` -- 2, 4 / "flips", 8, or a sequence of modes 0 .. 7 (bit 0 hflip, bit 1 vflip, bit 2
    transpose; `segments.check_ensemble`) -- runs every window under each mode and feeds the sink their mean, turned back on the
    device (`EAVSRP.forward_ensemble`); it composes with everything above, and the scene cuts read the untransformed bytes.  About
    len(modes) times the work.  The network is not equivariant, so the modes differ; whether their mean is BETTER is not known
    here (no trained weights exist in this project).  None: `opt.ensemble` of a model wrapper, else EAVSR_ENSEMBLE=8|4|2|flips|0,1,4
    (`segments.ensemble_options`), else off.  The result carries 'ensemble': the tuple of modes that ran ((0,): off).

    Temporal consistency, opt-in: `temporal` -- a `pwc.PWCNET`, the path of its weights, or True (`opt.pwc_path`) -- scores
    every pair of consecutive frames of every clip with `ops.temporal_metrics` on PWC-Net flows (`pair_flows`); `temporal_flow` is
    `temporal_metrics`' `flow_from`: "hr" (the default with `hr`; tOF is reported) or "sr" (no ground truth needed).  The sink keeps
    the last SR / HR frame of the previous chunk, so a pair that straddles two chunks, two windows or two emit ranges is scored once
    and the numbers do not depend on `frame_chunk`; a pair across a scene start the forward honoured (`cuts`, after the merge of
    short scenes; a 0 in an explicit list is the clip's own start and is dropped) is not scored.  The frames scored are the ones the
    sink sees: cropped (`pad`), blended (`tile`), averaged (`ensemble`).  The result gains 'frame_ewarp' / 'frame_tof' /
    'frame_valid', one entry per frame in (n, t) order and None for a frame without a scored predecessor, and the report (with `hr`)
    its 'ewarp' / 'tof' columns.  None: `opt.temporal` of a model wrapper, else EAVSR_TEMPORAL=hr|sr (`temporal_option`; the weights
    then come from `opt.pwc_path`), else off: no launch and no byte differs from a run without it.

    NIQE, opt-in: `niqe` -- an `eavsr_amd.niqe.NIQE`, the file name of a pristine model, or True (`opt.niqe_path`) -- scores
    every frame the sink sees (cropped, blended, averaged, as above) without ground truth, `niqe_crop` pixels removed on every side:
    two moment launches and one resize per chunk, the moments read back once when the forward has ended.  The result gains
    'frame_niqe' ((n, t) order; `nan` for frames below two 96 x 96 blocks) and the report its 'niqe' column; with hr=None there is
    a 'report' all the same, whose rows carry the names and 'niqe' only (`scene_report`).  A frame's score does not depend on
    `frame_chunk`.  None: `opt.niqe_path` of a model wrapper, else EAVSR_NIQE=<path>, else off (`niqe_option`; `niqe_crop`:
    `opt.niqe_crop`, else 0): no launch and no byte differs from a run without it.

    16-bit feature cache, opt-in: `cache_dtype` = "fp16" / "bf16" (or the torch dtypes) is `forward_long`'s -- the frame
    store holds the pyramid and the branches' outputs in 16 bits, about half the resident bytes of a window (twice the `max_frames` on
    the same card) and half the bytes over the link with cache="host"; it composes with everything above.  The frames are NOT the
    fp32 cache's bit for bit; which dtype is better for quality is not known here (no trained weights exist in this project).  None:
    `opt.cache_dtype` of a model wrapper, else EAVSR_CACHE_DTYPE=fp16|bf16 (`eavsrp_model.cache_dtype_option`), else off: no launch
    and no byte differs from a run without it.  The result carries 'cache_dtype': None, "fp16" or "bf16".

    The census of that cache (addendum), opt-in beside `cache_dtype`: `cache_check` = "report" / "raise" / "bf16" is
    `forward_long`'s -- the packs count what the rounding did per feature key; "report" reads the counts when a window has ended,
    "raise" refuses a window that overflowed or held inf / NaN before any of its frames is written (`framestore.CacheRangeError`),
    "bf16" runs an fp16 window that overflowed again on a bf16 cache, window by window.  None: `opt.cache_check` of a model wrapper,
    else EAVSR_CACHE_CHECK=report|raise|bf16 (`eavsrp_model.cache_check_option`), else off: no launch and no byte differs, and the
    result has neither field.  With a check the network's `cache_census` is cleared at entry and returned as 'cache_census' (one
    entry per `forward_long` call: window, tile, mode), with 'cache_range' = `framestore.census_summary` of it: the largest |x| any
    key of any window held, the totals of 'overflow', 'nonfinite', 'flushed' and 'subnormal', and how many windows fell back.

    Output at any target size, opt-in: `out_size` = (H, W) or "1080x1920" resizes every SR chunk to that size as the sink's
    first statement (`resize.resize_frames`: MATLAB's antialiased bicubic `imresize`, one HIP op) -- after the `pad` crop, the tile
    blend and the ensemble mean, because it acts on what the sink is handed.  Every consumer sees the resized frames: the files of both
    PNG encoders, PSNR / SSIM / LPIPS against `hr` -- which is now expected at `out_size` --, NIQE, and the temporal columns, whose
    flows are computed at that size.  None: `opt.out_size` of a model wrapper, else EAVSR_OUT_SIZE=HxW (`resize.out_size_option`),
    else off: no launch and no byte differs, and the result has no such field.  Set, the result carries 'out_size': (H, W).  The
    values have not been compared with MATLAB or any package, and the fp32 path is not MATLAB's uint8 path (eavsr_amd/resize.py)."""
    from . import ops
    from .resize import check_out_size, out_size_option, resize_frames as _resize_frames
    if out_size is None:      # a bad value is refused here, before a file is read
        out_size = out_size_option(getattr(model, "opt", None))
    out_size = check_out_size(out_size, "super_resolve: out_size")
    from .segments import (check_pad, check_tile, find_cuts, keep_starts, pad_option, parse_tile, plan_segments, plan_tiles, segment_options,
                           tile_options, DEFAULT_HIST_THRESHOLD, DEFAULT_SAD_THRESHOLD, DEFAULT_TILE_OVERLAP,
                           check_ensemble, ensemble_options, parse_ensemble)
    from .framestore import check_cache_dtype
    if cache_dtype is None:      # a bad value is refused here, before a file is read
        from .eavsrp_model import cache_dtype_option
        cache_dtype = cache_dtype_option(getattr(model, "opt", None))
    cache_dtype = check_cache_dtype(cache_dtype)
    from .framestore import check_cache_check
    if cache_check is None:
        from .eavsrp_model import cache_check_option
        cache_check = cache_check_option(getattr(model, "opt", None))
    cache_check = check_cache_check(cache_check, cache_dtype)
    # the range census of the 16-bit backbone (addendum): `networks.set_backbone_check`'s mode, else `opt.backbone_check` of
    # a model wrapper, else EAVSR_BACKBONE_CHECK; refused here, before a file is read, as every call below would refuse it
    from . import networks as _networks
    backbone_check = _networks.BACKBONE_CHECK
    if backbone_check is None:
        from .eavsrp_model import backbone_check_option
        backbone_check = backbone_check_option(getattr(model, "opt", None))
    backbone_check = _networks.check_backbone_check(backbone_check, _networks.BACKBONE_DTYPE)
    if ensemble is None:      # a bad spec is refused here, before a file is read
        modes = ensemble_options(getattr(model, "opt", None))
    elif isinstance(ensemble, str):
        modes = parse_ensemble(ensemble, "super_resolve: ensemble")
    else:
        modes = check_ensemble(ensemble, "super_resolve: ensemble")
    modes = modes or (0,)
    if pad is None:
        pad = pad_option(getattr(model, "opt", None))
    check_pad(pad, "super_resolve: pad")
    opt_tile, opt_tile_overlap = tile_options(getattr(model, "opt", None))
    tile = parse_tile(tile, "super_resolve: tile") if isinstance(tile, str) else check_tile(tile, "super_resolve: tile")
    if tile is None:
        tile = opt_tile
    if tile_overlap is None:
        tile_overlap = DEFAULT_TILE_OVERLAP if opt_tile_overlap is None else opt_tile_overlap
    if tile is not None:      # a bad tile / overlap is refused here, before a file is read or anything is allocated
        plan_tiles(tile[0], tile[1], tile, tile_overlap)
    if png_encoder is None:      # a model wrapper has read its options already; the bare network has none
        png_encoder = getattr(model, "png_encoder", None)
    if png_encoder is None:
        from .eavsrp_model import png_encoder_option
        png_encoder = png_encoder_option(getattr(model, "opt", None))
    check_png_encoder(png_encoder)
    if png_decoder is None:
        from .eavsrp_model import png_decoder_option
        png_decoder = png_decoder_option(getattr(model, "opt", None))
    check_png_decoder(png_decoder)
    net = getattr(model, "netEAVSRP", model)
    device = next(net.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("super_resolve: the network must be on the GPU (eavsr_amd has no CPU path)")
    niqe, niqe_crop = _resolve_niqe(niqe, niqe_crop, getattr(model, "opt", None), "super_resolve")      # refused before a file is read
    niqe_parts = []
    if temporal is False:
        temporal = None
    check_temporal_flow(temporal_flow, "super_resolve: temporal_flow")
    if temporal is None:
        temporal = temporal_option(getattr(model, "opt", None))
        if temporal in TEMPORAL_FLOWS:
            temporal, temporal_flow = True, (temporal if temporal_flow is None else temporal_flow)
    if temporal is not None:      # refused here, before a file is read: a missing weights file, "hr" without HR frames
        temporal_flow = _resolve_flow_from(temporal_flow, hr is not None, "super_resolve")
        temporal = temporal_net(temporal, getattr(model, "opt", None), device, "super_resolve")
    paths = None
    if isinstance(frames, (list, tuple)):
        paths = [os.fspath(p) for p in frames]
        if png_decoder == "device":
            frames = decode_png_frames(paths, device, channels=3)
        else:
            frames = torch.stack([read_png(p)[:3] for p in paths], 0)
            frames = frames.pin_memory()
    if isinstance(hr, (list, tuple)):
        hr_paths = [os.fspath(p) for p in hr]
        if png_decoder == "device":
            hr = decode_png_frames(hr_paths, device, channels=3)
        else:
            hr = torch.stack([read_png(p)[:3] for p in hr_paths], 0)

    def as_clip(x, what):
        if not isinstance(x, torch.Tensor) or x.dim() not in (4, 5):
            raise ValueError(f"super_resolve: {what} is a (t, 3, h, w) tensor (uint8: also (t, h, w, 3)), optionally with a leading n")
        if x.dtype != torch.uint8 and not x.is_floating_point():
            raise ValueError(f"super_resolve: {what} is uint8 or floating point, got {x.dtype}")
        return x.unsqueeze(0) if x.dim() == 4 else x
    lrs = as_clip(frames, "frames")
    if lrs.dtype != torch.uint8:
        lrs = lrs.to(device=device, dtype=torch.float32)
    n, t = int(lrs.shape[0]), int(lrs.shape[1])
    if temporal is not None:      # refused before anything runs: the SR frames have the input's channels, and PWC-Net reads RGB
        channels = int(lrs.shape[4] if (lrs.dtype == torch.uint8 and lrs.shape[4] == 3 and lrs.shape[2] != 3) else lrs.shape[2])
        if channels != 3:
            raise ValueError(f"super_resolve: temporal: PWC-Net reads RGB frames: C = {channels}, only C = 3 is accepted")
    if hr is not None:
        hr = as_clip(hr, "hr")
        if tuple(hr.shape[:2]) != (n, t):
            raise ValueError(f"super_resolve: hr holds {tuple(hr.shape[:2])} (n, t) frames, the scene {(n, t)}")
    if names is None:
        names = [os.path.basename(p) for p in paths] if paths is not None else ["000_%05d.png" % i for i in range(t)]
    if len(names) != t:
        raise ValueError(f"super_resolve: {len(names)} names for {t} frames")
    if isinstance(lpips, (str, os.PathLike)):
        from .lpips import build_lpips
        lpips = build_lpips(os.fspath(lpips), device=device)
    if lpips is not None and hr is None:
        raise ValueError("super_resolve: lpips needs hr")
    opt_frames, opt_overlap, opt_cuts = segment_options(getattr(model, "opt", None))
    if max_frames is None and opt_frames is not None:
        # (a window bound that comes from the options alone must not be refused for the default overlap of 8)
        max_frames, overlap = opt_frames, (min(overlap, opt_frames // 2) if opt_overlap is None else opt_overlap)
    if cuts is None:
        cuts = opt_cuts
    if isinstance(cuts, str):
        if cuts != "device":
            raise ValueError(f"super_resolve: cuts={cuts!r}: None, 'device' or a list of scene starts")
        if n != 1 or lrs.dtype != torch.uint8:
            raise ValueError(f"super_resolve: cuts='device' reads one clip of 8-bit frames, got n={n}, {lrs.dtype}")
    elif cuts is not None:
        cuts = explicit_cuts(cuts)
    hist_thr, sad_thr = (DEFAULT_HIST_THRESHOLD, DEFAULT_SAD_THRESHOLD) if cut_thresholds is None else cut_thresholds
    segmented = max_frames is not None or cuts is not None
    if segmented:      # max_frames / overlap / min_scene / explicit starts are refused here, before anything is allocated or run
        plan_segments(t, [] if cuts == "device" else (cuts or []), max_frames, overlap, min_scene)
    frame_h, frame_w = (int(v) for v in (lrs.shape[2:4] if (lrs.dtype == torch.uint8 and lrs.shape[4] == 3 and lrs.shape[2] != 3)
                                         else lrs.shape[3:5]))
    tiles = [(0, frame_h, 0, frame_w)] if tile is None else plan_tiles(frame_h, frame_w, tile, tile_overlap)
    written: List[str] = []
    sse_parts, ssim_parts, lpips_parts, counts = [], [], [], []
    staging = _PngStaging() if (out_dir is not None and png_encoder == "device") else None
    pending = []      # at most one (job, paths): the chunk whose files are still on their way

    def write_pending():
        while pending:
            job, targets = pending.pop(0)
            for path, data in zip(targets, _PngStaging.files(job)):
                written.append(_write_file(path, data))

    def hr_chunk(a, b):
        part = hr[:, a:b]
        if not part.is_cuda:
            part = part.to(device, non_blocking=True)
        part = part.reshape((n * (b - a),) + tuple(part.shape[2:]))
        return ops.u8_to_f32(part) if part.dtype == torch.uint8 else part.to(torch.float32)

    # temporal consistency: the last frame of the previous chunk is kept (a copy: a chunk may be a view of storage the forward
    # reuses), so the pair that straddles two sink calls is scored with the later one
    held = {"next": None, "sr": None, "hr": None}
    scene_bounds: List[int] = []      # the scene starts the forward honours: no pair is scored across one
    temporal_parts = []               # (clip frame of the first pair's second frame, [(err, count, epe) per clip]), on the device
    temporal_shape = []

    def score_pairs(first, sr, ref):
        k = int(sr.shape[1])
        temporal_shape[:] = [int(v) for v in sr.shape[2:]]

        def score(at, seq_sr, seq_hr):      # frames [at - 1, at - 1 + len) of the clip: one run inside a scene
            temporal_parts.append((at, [_temporal_device(seq_sr[b], None if seq_hr is None else seq_hr[b], temporal, 255.0,
                                                         temporal_flow) for b in range(n)]))

        if held["next"] == first and first not in scene_bounds:      # the pair that straddles two sink calls, on its own
            score(first, torch.cat([held["sr"], sr[:, :1]], 1), None if ref is None else torch.cat([held["hr"], ref[:, :1]], 1))
        bounds = [first] + [s for s in scene_bounds if first < s < first + k] + [first + k]
        for lo, hi in zip(bounds[:-1], bounds[1:]):      # the chunk's own pairs, in place
            if hi - lo >= 2:
                score(lo + 1, sr[:, lo - first:hi - first], None if ref is None else ref[:, lo - first:hi - first])
        held.update(next=first + k, sr=sr[:, -1:].clone(), hr=None if ref is None else ref[:, -1:].clone())

    def sink(first, sr):
        if out_size is not None:      # every consumer below sees the resized frames
            sr = _resize_frames(sr, out_size)
        k = int(sr.shape[1])
        c, hh, ww = (int(v) for v in sr.shape[2:])
        flat = sr.reshape(n * k, c, hh, ww)
        rgb8 = None
        if hr is not None:
            ref = hr_chunk(first, first + k)
            if ref.shape != flat.shape:
                raise ValueError(f"super_resolve: hr frames are {tuple(ref.shape[1:])}, the output {tuple(flat.shape[1:])}")
            sse, fs, rgb8 = ops.frame_metrics(flat, ref, 255.0, rgb8=out_dir is not None)
            sse_parts.append(sse.view(n, k))
            ssim_parts.append(fs.view(n, k))
            counts.append(c * hh * ww)
            if lpips is not None:
                lpips_parts.append(lpips(flat, ref, 255.0).view(n, k))
        elif out_dir is not None:
            rgb8 = ops.rgb8(flat, 255.0)
        if niqe is not None:
            niqe_parts.append((first, k, niqe.moments(flat, 255.0, niqe_crop)))
        if temporal is not None:
            score_pairs(first, sr, ref.view(n, k, c, hh, ww) if temporal_flow == "hr" else None)
        if staging is not None:
            job = staging.enqueue(rgb8[:k])      # clip 0, as save_visuals; nothing here waits for the device
            write_pending()                      # the previous chunk's files, while this chunk's encoder runs
            pending.append((job, [os.path.join(out_dir, _frame_name(names, first + j)) for j in range(k)]))
        elif out_dir is not None:
            host = rgb8[:k].cpu()      # clip 0, as save_visuals
            for j in range(k):
                written.append(write_png(host[j], os.path.join(out_dir, _frame_name(names, first + j)), hwc=True))

    # the resize reads strides: a cropped chunk (`pad`) is handed over as the view it is, not copied first
    sink.takes_views = out_size is not None

    torch.cuda.synchronize(device)
    torch.cuda.reset_peak_memory_stats(device)
    t0 = time.time()
    with torch.no_grad():
        if not segmented:
            starts, plan = [], [(0, t, 0, t)]
        else:
            if cuts == "device":
                hwc = lrs.shape[4] == 3 and lrs.shape[2] != 3
                stat_hist, stat_sad = scene_changes(lrs[0], device=device)
                pixels = int(lrs.shape[2] * lrs.shape[3]) if hwc else int(lrs.shape[3] * lrs.shape[4])
                starts = find_cuts(stat_hist, stat_sad, pixels, hist_thr, sad_thr)
            else:
                starts = list(cuts or [])
            plan = plan_segments(t, starts, max_frames, overlap, min_scene)
            scene_bounds[:] = keep_starts(t, starts, min_scene)
        with _backbone_checked(backbone_check, net):
            if cache_check is not None:
                net.cache_census = []
                net.forward_cached(lrs, cache_dtype, ensemble=None if modes == (0,) else modes, tile=tile, overlap=tile_overlap,
                                   segments=plan if segmented else None, pad=pad, frame_chunk=frame_chunk, cache=cache, sink=sink,
                                   cache_check=cache_check)
            elif cache_dtype is not None:
                net.forward_cached(lrs, cache_dtype, ensemble=None if modes == (0,) else modes, tile=tile, overlap=tile_overlap,
                                   segments=plan if segmented else None, pad=pad, frame_chunk=frame_chunk, cache=cache, sink=sink)
            elif modes == (0,):
                net.forward_video(lrs, segments=plan if segmented else None, tile=tile, tile_overlap=tile_overlap, pad=pad,
                                  frame_chunk=frame_chunk, cache=cache, sink=sink)
            else:
                net.forward_ensemble(lrs, ensemble=modes, tile=tile, overlap=tile_overlap, segments=plan if segmented else None, pad=pad,
                                     frame_chunk=frame_chunk, cache=cache, sink=sink)
    write_pending()
    torch.cuda.synchronize(device)
    seconds = time.time() - t0
    out = {"frames": n * t, "seconds": seconds, "frames_per_s": n * t / seconds if seconds > 0 else math.nan,
           "peak_bytes": int(torch.cuda.max_memory_allocated(device)), "written": written,
           "segments": plan, "scene_starts": starts, "tiles": tiles, "ensemble": modes, "cache_dtype": cache_dtype}
    if out_size is not None:
        out["out_size"] = out_size
    if cache_check is not None:
        from .framestore import census_summary
        out.update(cache_census=net.cache_census, cache_range=census_summary(net.cache_census))
    if backbone_check is not None:      # one entry per window / tile / mode, and the one line over them
        out.update(backbone_census=net.backbone_census, backbone_range=_networks.range_summary(net.backbone_census))
    frame_temporal = None
    if temporal is not None:
        rows = {key: [[None] * t for _ in range(n)] for key in ("ewarp", "tof", "valid")}
        for at, per_clip in temporal_parts:
            for b, (err, count, epe) in enumerate(per_clip):
                vals = temporal_values(err.tolist(), count.tolist(), None if epe is None else epe.tolist(), *temporal_shape)
                for key, row in rows.items():
                    if vals[key] is not None:
                        row[b][at:at + len(vals[key])] = vals[key]
        frame_temporal = {key: [v for row in rows[key] for v in row] for key in rows}      # (n, t) order
        out.update(frame_ewarp=frame_temporal["ewarp"], frame_tof=frame_temporal["tof"], frame_valid=frame_temporal["valid"])
    frame_niqe = None
    if niqe is not None:
        values = _niqe_values(niqe, [(n * k, m) for _, k, m in niqe_parts])      # per chunk in (n, k) order
        rows, at = [[math.nan] * t for _ in range(n)], 0
        for first, k, _ in niqe_parts:
            for b in range(n):
                rows[b][first:first + k] = values[at + b * k:at + (b + 1) * k]
            at += n * k
        frame_niqe = out["frame_niqe"] = [v for row in rows for v in row]      # (n, t) order
    if hr is not None:
        sse = torch.cat(sse_parts, 1).reshape(-1).tolist()      # (n, t) order, as evaluate
        frame_ssim = torch.cat(ssim_parts, 1).reshape(-1).tolist()
        frame_psnr = [psnr_from_sse(v, counts[0]) for v in sse]
        frame_names = [_frame_name(names, i, b) for b in range(n) for i in range(t)]
        frame_lpips = torch.cat(lpips_parts, 1).reshape(-1).tolist() if lpips is not None else None
        out.update(frame_psnr=frame_psnr, frame_ssim=frame_ssim, frame_names=frame_names,
                   report=scene_report(frame_names, frame_psnr, frame_ssim, frame_lpips,
                                       **({} if frame_temporal is None else {"temporal": frame_temporal}),
                                       **({} if frame_niqe is None else {"niqe": frame_niqe})))
        if lpips is not None:
            out["frame_lpips"] = frame_lpips
    elif frame_niqe is not None:      # footage without ground truth: the names and the no-reference column
        frame_names = [_frame_name(names, i, b) for b in range(n) for i in range(t)]
        out.update(frame_names=frame_names, report=scene_report(frame_names, None, None, niqe=frame_niqe))
    return out
