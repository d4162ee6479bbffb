"""Functional host-side wrappers over the C ABI (include/eavsr_hip.h).

PyTorch is plumbing here: it owns device memory (outputs come from torch.empty on the caching
allocator) and the stream (torch.cuda.current_stream()).  Every function launches HIP kernels
from libeavsr_hip.so asynchronously on that stream and raises on any error.  Inputs must be
fp32 CUDA(HIP) tensors; there is no CPU path.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import re as _re
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _native as N
from .weight_cache import WEIGHT_CACHES, WeightCache      # (WEIGHT_CACHES: the registry, also read as ops.WEIGHT_CACHES)

Tensor = torch.Tensor

ACT = {"none": 0, None: 0, "relu": 1, "lrelu": 2, "relu_mask": 3}      # relu_mask: conv2d(residual = the ReLU's forward output), direct kernels only


def _chk(t: Tensor, name: str) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: dtype {t.dtype} unsupported (fp32 only in this round)")
    return t if t.is_contiguous() else t.contiguous()


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _stream(t: Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


class _DeviceOf:
    """Make sure launches go to the device that owns the tensors."""

    def __init__(self, t: Tensor):
        self.idx = t.device.index
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


def lib():
    return N.load()


class LabBuildRequired(RuntimeError):
    """A mode / op that exists only in the lab build of the library (`python -m eavsr_amd.build --lab`): the retired schedules
    kept for A/B measurements (eavsr_amd/build.py LAB_SOURCES; the EXPERIMENTAL section of include/eavsr_hip.h)."""


def lab_available() -> bool:
    return N.lab_build()


def require_lab(what: str) -> None:
    if not lab_available():
        raise LabBuildRequired(f"{what} is part of the lab build only: rebuild with `python -m eavsr_amd.build --lab` "
                               "(the default library holds the product path and its documented modes)")


def _wino_tiles(h: int, w: int) -> int:
    """8 x 32-pixel tiles of an image (the granularity the Winograd gates count in; eavsr_conv3x3_wino_tiles of the lab build)"""
    return ((h + 7) // 8) * ((w + 31) // 32)


# Route pinning.  Which kernel a convolution runs on depends on its launch size (n x tiles against WINO_MIN_TILES, X6S_MAX_TILES, the
# direct kernel's tile height), and different kernels round differently.  A caller that cuts ONE batch into several launches
# (EAVSRP.forward_long's frame chunks) wraps them in `with route_batch(n_whole):` -- every routing predicate below then sees the
# batch size of the whole batch (`_rn`), and the library's own tile-height choice follows (eavsr_route_batch), so each chunk runs the
# kernels the whole batch would and is bit-identical to its rows of the whole-batch result.  None = off: the launch's own n.
_ROUTE_BATCH: Optional[int] = None


def _rn(n: int) -> int:
    """the batch size the routing predicates count with"""
    return int(n) if _ROUTE_BATCH is None else _ROUTE_BATCH


@contextlib.contextmanager
def route_batch(n: Optional[int]):
    """`with ops.route_batch(t * n):` -- convolutions launched inside choose their kernels as a batch of `n` images would, whatever
    their own batch size (None: no pinning).  Restores the previous setting on exit, also when the body raises.  Not re-entrant
    across threads: the pin is process-wide, like the kernel modes."""
    global _ROUTE_BATCH
    if n is not None and int(n) < 1:
        raise ValueError(f"route_batch: a batch size >= 1 or None, got {n!r}")
    prev = _ROUTE_BATCH
    _ROUTE_BATCH = None if n is None else int(n)
    lib().eavsr_route_batch(0 if n is None else int(n))
    try:
        yield
    finally:
        _ROUTE_BATCH = prev
        lib().eavsr_route_batch(0 if prev is None else prev)


# ------------------------------------------------------------------------------------------
# optional per-launch timing (HIP events on the launch stream); off unless `with profile():`
# ------------------------------------------------------------------------------------------
class Profile:
    """Collects (kernel name, algorithmic flops, algorithmic bytes, start/end event) per launch.
    Events are recorded on the stream the kernel is launched on, so the elapsed time is the
    device-side duration of that launch (plus ~1 us of event overhead)."""

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, nbytes, e0, e1 in self.records:
            d = out.setdefault(name, {"calls": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            d["calls"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += flops
            d["bytes"] += nbytes
        return out

    def by_flops(self, name: str):
        """the launches of one kernel name grouped by their algorithmic FLOP count (= by launch shape): {flops: (calls, ms)}"""
        torch.cuda.synchronize()
        out = {}
        for nm, flops, _nbytes, e0, e1 in self.records:
            if nm == name:
                c, ms = out.get(flops, (0, 0.0))
                out[flops] = (c + 1, ms + e0.elapsed_time(e1))
        return out


_prof: Optional[Profile] = None


class profile:
    def __enter__(self):
        global _prof
        _prof = Profile()
        return _prof

    def __exit__(self, *a):
        global _prof
        _prof = None


# The range census of the 16-bit backbone modes (addendum): None, or the `RangeCensus` that every launch of a 16-bit op
# counts into while a `networks.backbone_check` is on.  `_launch` is the one place that reads it.
RANGE16: Optional["RangeCensus"] = None


def _launch(name: str, flops: float, nbytes: float, t: Tensor, fn, what: str, stored=None, rounded=None):
    """Run `fn()` (a C-ABI call returning an int status) on t's device and check it.
    What an op of the 16-bit modes rounds, declared where it launches: `stored` -- the 16-bit tensors the launch writes, counted behind
    it (`range16_words`); `rounded` -- (fp32 tensors, dtype) that its kernel rounds on the way in, counted in front of it
    (`range16_as_rounded`); `stored=()` says that a 16-bit op rounds nothing the census could see.  Read only while RANGE16 is set,
    which then refuses a 16-bit launch (`RangeCensus.is_16bit`) that declares neither."""
    if RANGE16 is not None and not name.startswith("range16"):
        # (a site is named after `what`, the entry point: several of them share one profile name)
        return RANGE16.around(what, stored, rounded, lambda: _launch_plain(name, flops, nbytes, t, fn, what))
    return _launch_plain(name, flops, nbytes, t, fn, what)


def _launch_plain(name: str, flops: float, nbytes: float, t: Tensor, fn, what: str):
    with _DeviceOf(t):
        if _prof is None:
            code = fn()
        else:
            st = torch.cuda.current_stream(t.device)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record(st)
            code = fn()
            e1.record(st)
            _prof.records.append((name, flops, nbytes, e0, e1))
    N.check(code, what)


def selftest_mfma(device="cuda:0") -> int:
    """Number of accumulator elements that disagree with the assumed MFMA lane layout (0 = OK)."""
    s = torch.zeros(8192, device=device, dtype=torch.float32)
    with _DeviceOf(s):
        N.check(lib().eavsr_selftest_mfma_f32(s.data_ptr(), _stream(s)), "selftest_mfma")
    return int(s[0].item())


# ------------------------------------------------------------------------------------------
# flow_warp  (networks.py:699-739, eavsrp_model.py:587-626)
# ------------------------------------------------------------------------------------------
def flow_warp(x: Tensor, flow: Tensor, padding_mode: str = "zeros", flow2: Optional[Tensor] = None,
              flow_layout: str = "nchw", interpolation: str = "bilinear", align_corners: bool = True) -> Tensor:
    x = _chk(x, "x")
    n, c, h, w = x.shape
    if flow_layout == "nchw":
        if tuple(flow.shape) != (n, 2, h, w):
            raise ValueError(f"The spatial sizes of input ({(h, w)}) and flow ({tuple(flow.shape)}) are not the same.")
        layout = 0
    elif flow_layout == "nhwc":
        if tuple(flow.shape) != (n, h, w, 2):
            raise ValueError(f"The spatial sizes of input ({(h, w)}) and flow ({tuple(flow.shape)}) are not the same.")
        # a permuted view of an NCHW tensor (the reference passes flow.permute(0,2,3,1)) is used in place
        if not flow.is_contiguous() and flow.permute(0, 3, 1, 2).is_contiguous():
            flow = flow.permute(0, 3, 1, 2)
            layout = 0
        else:
            layout = 1
    else:
        raise ValueError(flow_layout)
    pm = {"zeros": 0, "border": 1, "reflection": 2}.get(padding_mode)
    if pm is None:
        raise ValueError(f"padding_mode={padding_mode!r}: 'zeros', 'border' or 'reflection'")
    if interpolation not in ("bilinear", "nearest"):
        raise ValueError(f"interpolation={interpolation!r}: 'bilinear' or 'nearest'")
    pm |= (0x10 if interpolation == "nearest" else 0) | (0 if align_corners else 0x20)
    flow = _chk(flow, "flow")
    if flow2 is not None:
        flow2 = _chk(flow2, "flow2")
        if flow2.shape != flow.shape:
            raise ValueError("flow2 must have the shape/layout of flow")
    out = torch.empty_like(x)
    st = _stream(x)
    _launch("flow_warp", 8.0 * n * c * h * w, 4.0 * n * h * w * (2 * c + 2 + (2 if flow2 is not None else 0)), x,
            lambda: lib().eavsr_flow_warp_f32(_p(x), _p(flow), _p(flow2), _p(out), n, c, h, w, layout, pm, st),
            "flow_warp")
    return out


def _warp_pad_code(padding_mode: str, who: str) -> int:
    pm = {"zeros": 0, "border": 1}.get(padding_mode)
    if pm is None:
        raise ValueError(f"{who}: padding_mode={padding_mode!r}: 'zeros' or 'border'")
    return pm


def flow_warp_pair(xa: Tensor, xb: Tensor, flow: Tensor, flow2: Optional[Tensor] = None, b_il8=False, padding_mode: str = "zeros"):
    """(flow_warp(xa, flow [+ flow2]), flow_warp(xb, flow [+ flow2])) in one launch (networks.py:621,623); with b_il8 the
    second result comes in the IL8 layout (n, c/8, h, w, 8) of `dcnv2_il` -- fp32 (True) or rounded to 'fp16' / 'bf16' for
    `dcnv2_il16`."""
    pad = _warp_pad_code(padding_mode, "flow_warp_pair")
    xa, xb, flow = _chk(xa, "xa"), _chk(xb, "xb"), _chk(flow, "flow")
    n, c, h, w = xa.shape
    if xb.shape != xa.shape or tuple(flow.shape) != (n, 2, h, w):
        raise ValueError("flow_warp_pair: xa, xb (n,c,h,w) and flow (n,2,h,w)")
    if flow2 is not None:
        flow2 = _chk(flow2, "flow2")
        if flow2.shape != flow.shape:
            raise ValueError("flow2 must have the shape of flow")
    if b_il8 and c % 8:
        raise ValueError("flow_warp_pair: IL8 output needs c % 8 == 0")
    outa = torch.empty_like(xa)
    if isinstance(b_il8, str):
        code = h16_code(b_il8)                      # 1 fp16, 2 bf16
        outb = torch.empty((n, c // 8, h, w, 8), device=xa.device, dtype=_H16_TORCH[code])
        mode = 1 + code
    else:
        outb = torch.empty((n, c // 8, h, w, 8) if b_il8 else tuple(xb.shape), device=xa.device, dtype=torch.float32)
        mode = 1 if b_il8 else 0
    st = _stream(xa)
    _launch("flow_warp_pair", 16.0 * n * c * h * w, 4.0 * n * h * w * (4 * c + 2 + (2 if flow2 is not None else 0)), xa,
            lambda: lib().eavsr_flow_warp_pair_f32(_p(xa), _p(xb), _p(flow), _p(flow2), _p(outa), _p(outb), n, c, h, w,
                                                   mode | (N.WARP_PAIR_BORDER if pad else 0), st), "flow_warp_pair",
            stored=(outb,) if isinstance(b_il8, str) else None)
    return outa, outb


def flow_warp_single(x: Tensor, flow: Tensor, flow2: Optional[Tensor] = None, il8=False, padding_mode: str = "zeros") -> Tensor:
    """flow_warp(x, flow [+ flow2]) by ONE half of `flow_warp_pair`'s kernel as a launch of its own (the same kernel code, the same
    bits as that launch's result for the same tensor): il8=False -- (n, c, h, w), the pair's first result; il8=True / 'fp16' /
    'bf16' -- the IL8 layout (n, c/8, h, w, 8) of `dcnv2_il` / `dcnv2_il16`, the pair's second result.  The alignment module's two
    warps once its predictors run ahead of the recurrence (networks.MultiAdSTN.predict / .sample)."""
    x, flow = _chk(x, "x"), _chk(flow, "flow")
    n, c, h, w = x.shape
    if tuple(flow.shape) != (n, 2, h, w):
        raise ValueError("flow_warp_single: x (n,c,h,w) and flow (n,2,h,w)")
    if flow2 is not None:
        flow2 = _chk(flow2, "flow2")
        if flow2.shape != flow.shape:
            raise ValueError("flow2 must have the shape of flow")
    if il8 and c % 8:
        raise ValueError("flow_warp_single: IL8 output needs c % 8 == 0")
    pad = _warp_pad_code(padding_mode, "flow_warp_single")
    if isinstance(il8, str):
        code = h16_code(il8)                      # 1 fp16, 2 bf16
        out, mode = torch.empty((n, c // 8, h, w, 8), device=x.device, dtype=_H16_TORCH[code]), 1 + code
    elif il8:
        out, mode = torch.empty((n, c // 8, h, w, 8), device=x.device, dtype=torch.float32), 1
    else:
        out, mode = torch.empty_like(x), 0
    st = _stream(x)
    # (recorded under the kernel's name: both forms launch flow_warp_pair_kernel)
    _launch("flow_warp_pair", 8.0 * n * c * h * w,
            4.0 * n * h * w * (2 * c + 2 + (2 if flow2 is not None else 0)), x,
            lambda: lib().eavsr_flow_warp_single_f32(_p(x), _p(flow), _p(flow2), _p(out), n, c, h, w, mode, pad, st), "flow_warp_single",
            stored=(out,) if isinstance(il8, str) else None)
    return out


# ------------------------------------------------------------------------------------------
# packed conv weights (cached per parameter version)
# ------------------------------------------------------------------------------------------
# One cache per form, under the name tests and tools know it by.  The exact bf16-split forms (_conv7_pack_cache) and the one-plane
# forms of the bf16 training mode (_bf16_pack_cache) never share one, whatever the mode was when either was packed.
pack_cache, _smallco_pack_cache, _conv7_pack_cache, _bf16_pack_cache = WeightCache(), WeightCache(), WeightCache(), WeightCache()
_h16g_pack_cache, _h16x1_pack_cache, _il2_pack_cache, _il16_pack_cache = WeightCache(), WeightCache(), WeightCache(), WeightCache()
_x9_pack_cache, _wino_pack_cache, _lpips_pack_cache, _h16_pack_cache = WeightCache(), WeightCache(), WeightCache(), WeightCache()
_h16_pack5_cache, _pwc_pack_cache = WeightCache(), WeightCache()


class _Form(NamedTuple):
    """One packed form of a conv weight.  The entry points are written with their scalar arguments, "name cout cin k code" (`k` the
    kernel size, `code` the h16_code of a 16-bit form); a pack entry point takes them between (weight, packed) and the stream."""
    cache: WeightCache
    tag: Optional[str]          # what the caller's variant is, and the cache tag: None, "code", "kind", or "dgrad" (True -> the "_dgrad" pack entry point, tag "dgrad")
    many: Optional[str]         # None: one weight.  A list stacked along cout: "cat" = concatenated for the pack alone, "wcat" = through _cat_weights (cached)
    shape: Optional[tuple]      # accepted (cout, cin, k) of a square kernel, each None (any), a number or a container of numbers; None: not checked here
    size: Union[str, int]       # the entry point that sizes the buffer, or the element count itself
    in_bytes: bool              # `size` counts bytes (else elements of `dtype`)
    dtype: Optional[torch.dtype]      # of the buffer; None: the 16-bit type of `code`
    pack: str
    error: Optional[str]        # the NotImplementedError of a weight outside `shape` or of a size <= 0 ({s}: its shape); None: nothing is checked
    chk: Optional[Callable] = _chk    # the weight's own check: _chk, _lp (no copy), None (checked by the caller)


_S3 = (None, None, 3)
_FORMS = {
    "f32": _Form(pack_cache, None, "cat", (None, None, None), "eavsr_packed_weight_elems cout cin k", False, torch.float32,
                 "eavsr_pack_conv_weight_f32 cout cin k", "conv weight shape {s} unsupported (square kernels only)"),
    "smallco": _Form(_smallco_pack_cache, None, "wcat", None, "eavsr_smallco_packed_elems cout cin", False, torch.float32,
                     "eavsr_pack_smallco_weight cout cin", None),
    "x6": _Form(_conv7_pack_cache, "dgrad", "wcat", None, "eavsr_conv_weight_x6_bytes k cout cin", True, torch.uint8,
                "eavsr_pack_conv_weight_x6 k cout cin", None),
    "bf16x1": _Form(_bf16_pack_cache, "dgrad", "wcat", None, "eavsr_conv_weight_bf16x1_bytes k cout cin", True, torch.uint8,
                    "eavsr_pack_conv_weight_bf16x1 k cout cin", None),
    "h16g": _Form(_h16g_pack_cache, "code", "wcat", None, "eavsr_conv3x3_h16g_weight_bytes cout cin", True, torch.uint8,
                  "eavsr_pack_conv3x3_h16g cout cin code", None),
    "h16x1": _Form(_h16x1_pack_cache, "code", "wcat", None, "eavsr_conv_weight_h16x1_bytes k cout cin", True, torch.uint8,
                   "eavsr_pack_conv_weight_h16x1 k cout cin code", None),
    "il2": _Form(_il2_pack_cache, None, None, _S3, "eavsr_dcn_weight_il2_bytes cout cin", True, torch.int32,
                 "eavsr_pack_dcn_weight_il2 cout cin", "il2 weight shape {s} unsupported"),
    "il16": _Form(_il16_pack_cache, "code", None, _S3, "eavsr_dcn_il16_weight_bytes cout cin", True, torch.int32,
                  "eavsr_pack_dcn_il16_weight cout cin code", "dcnv2_il16 weight shape {s} unsupported (3x3 only)"),
    "x9": _Form(_x9_pack_cache, None, "cat", _S3, "eavsr_dcn_weight_x9_bytes cout cin", True, torch.int32,
                "eavsr_pack_dcn_weight_x9 cout cin", "bf16x9 weight shape {s} unsupported (the bf16x9 kernels are 3x3)"),
    "wino_f2": _Form(_wino_pack_cache, "kind", "cat", _S3, "eavsr_wino_weight_elems cout cin", False, torch.float32,
                     "eavsr_pack_conv_weight_wino cout cin", "winograd weight shape {s} unsupported"),
    "wino_f4": _Form(_wino_pack_cache, "kind", "cat", _S3, "eavsr_wino4_weight_elems cout cin", False, torch.float32,
                     "eavsr_pack_conv_weight_wino4 cout cin", "winograd weight shape {s} unsupported"),
    "wino_f5": _Form(_wino_pack_cache, "kind", "cat", (None, None, 5), "eavsr_wino4_weight_elems cout cin", False, torch.float32,
                     "eavsr_pack_conv_weight_wino5x5 cout cin", "winograd weight shape {s} unsupported"),
    "lpips": _Form(_lpips_pack_cache, None, None, (None, None, None), "eavsr_lpips_conv_weight_elems cout cin k", False, torch.float32,
                   "eavsr_lpips_pack_conv_f32 cout cin k", "lpips_conv: weight shape {s} unsupported", lambda t, name: _lp(t, name)),
    "h16": _Form(_h16_pack_cache, "code", None, (64, 64, 3), 64 * 576, False, None,
                 "eavsr_pack_conv3x3_c64_h16 code", "the 16-bit backbone kernel is the 3x3 64->64 convolution"),
    "h16_5x5": _Form(_h16_pack5_cache, "code", None, (range(129), 64, 5), "eavsr_conv5x5_c64_h16_weight_bytes", True, None,
                     "eavsr_pack_conv5x5_c64_h16 cout code", "the 16-bit heads kernel is the 5x5 convolution 64 -> (<= 128) channels", None),
    "pwc": _Form(_pwc_pack_cache, None, None, _S3, "eavsr_pwc_conv3x3_weight_elems cout cin", False, torch.float32,
                 "eavsr_pwc_pack_conv3x3_f32 cout cin", "pwc_conv3x3: weight shape {s} unsupported (3x3 only)"),
}


def _packed(form: str, weights, variant=None):
    """The packed form `form` of a weight (of a list of them where the form takes one), cached per weight objects and versions and
    verified by identity: on a miss the weight is checked, the library sizes the buffer and its pack kernel fills it on the
    weight's device and current stream, right in front of the store."""
    f = _FORMS[form]
    sources = weights if f.many else (weights,)
    tag = ("dgrad" if variant else None) if f.tag == "dgrad" else variant

    def make():
        w = sources[0] if len(sources) == 1 else _cat_weights(sources) if f.many == "wcat" else torch.cat([x.detach() for x in sources], 0)
        w = w if f.chk is None else f.chk(w.detach(), "weight")
        s = tuple(int(x) for x in w.shape)
        if f.error is not None and not (len(s) == 4 and s[2] == s[3] and all(
                p is None or (x == p if isinstance(p, int) else x in p) for p, x in zip(f.shape, s))):
            raise NotImplementedError(f.error.format(s=s))
        v = {"cout": s[0], "cin": s[1], "k": s[-1], "code": variant}
        size, (pack, *pack_args) = f.size, f.pack.split()
        if isinstance(size, str):
            name, *args = size.split()
            sized = dict(v, cout=s[1], cin=s[0]) if tag == "dgrad" else v      # as the input-gradient convolution's (cin, cout, k, k) weight
            size = int(getattr(lib(), name)(*[sized[a] for a in args]))
            if f.error is not None and size <= 0:
                raise NotImplementedError(f.error.format(s=s))
        if tag == "dgrad":
            pack += "_dgrad"      # transposed and flipped by the pack kernel itself: no materialised copy
        dtype = _H16_TORCH[variant] if f.dtype is None else f.dtype
        packed = torch.empty(size // dtype.itemsize if f.in_bytes else size, device=w.device, dtype=dtype)
        with _DeviceOf(w):
            N.check(getattr(lib(), pack)(_p(w), _p(packed), *[v[a] for a in pack_args], _stream(w)), pack[len("eavsr_"):])
        return packed
    return f.cache.derive(sources, tag, make)


def _packed_f32(weights: Sequence[Tensor]) -> Tensor:
    """the packed form of a conv weight (or of several stacked along cout) for eavsr_conv2d_f32"""
    return _packed("f32", weights)


def _cat_bias(biases: Sequence[Optional[Tensor]]) -> Optional[Tensor]:
    if biases[0] is None:
        return None
    return biases[0] if len(biases) == 1 else torch.cat([b.detach() for b in biases], 0)


_bias_cache = WeightCache()


def _bias_of(biases: Sequence[Optional[Tensor]]) -> Optional[Tensor]:
    if len(biases) == 1:
        return None if biases[0] is None else _chk(biases[0].detach(), "bias")
    return _bias_cache.derive(biases, None, lambda: _chk(_cat_bias(biases), "bias"))


_wcat_cache = WeightCache()


def _cat_weights(weights: Sequence[Tensor]) -> Tensor:
    """cat(weights, 0) in the original layout, cached per (object, version) like the packed weights"""
    if len(weights) == 1:
        return _chk(weights[0].detach(), "weight")
    return _wcat_cache.derive(weights, None, lambda: _chk(torch.cat([w.detach() for w in weights], 0), "weight"))


# Small-cout 3x3 convolutions (64 -> 6 / 18 -> 2 heads of the pyramid levels, conv_last): eavsr_conv3x3_smallco_lite_f32 wherever the
# shape allows -- 30-39 registers, weights as scalar operands, so that its waves fit beside a resident Winograd workgroup of the other
# stream (48 registers / 28 KB are left on such a CU): conv_last 1,723 -> 850 us, and with 4 x 32-pixel tiles on the small launches
# the step 240.0 -> 236.8 ms.  EAVSR_SMALLCO=classic: round 2's 112-184-register kernels (the A/B reference).
SMALLCO_LITE = os.environ.get("EAVSR_SMALLCO", "lite") != "classic"
SMALLCO_LITE_MIN_TILES = 0


def _packed_smallco(weights: Sequence[Tensor]) -> Tensor:
    """[ci][kx][block] form of a small-cout 3x3 weight (eavsr_pack_smallco_weight)"""
    return _packed("smallco", weights)


# 7x7 convolutions (SPyNet's basic module) and the 5x5 heads of the predictor: "bf16x6" = eavsr_conv_f32x6 (fp32 operands split
# exactly into bf16 terms, the contraction on the bf16 matrix pipe); otherwise the fp32-MFMA kernels (7x7: the implicit GEMM of
# eavsr_conv2d_f32; 5x5: F(2x2,5x5)).  A/B switches.
CONV7_MODE = os.environ.get("EAVSR_CONV7", "bf16x6")
CONV5_MODE = os.environ.get("EAVSR_CONV5", "bf16x6")


def _packed_conv_x6(weights: Sequence[Tensor], dgrad: bool = False) -> Tensor:
    """A-operand form of a 7x7 / 5x5 / 3x3 weight (eavsr_pack_conv_weight_x6); cached per weight objects and versions.
    dgrad=True: the form of the INPUT-GRADIENT convolution of the (single) forward weight -- transposed and flipped by the pack
    kernel itself (eavsr_pack_conv_weight_x6_dgrad), no materialised copy."""
    return _packed("x6", weights, dgrad)


# The opt-in bf16 training mode (networks.set_train_precision / EAVSR_TRAIN_PRECISION): "fp32" (the default: every convolution
# exact) or "bf16" -- the 3x3 64 -> 64 convolutions that autograd records, their input-gradient convolutions and their weight
# gradients, where the crop-sized kernel runs (x6s_takes), take their operands rounded once to bf16 (csrc/conv3_x6s.hip NP = 1,
# csrc/conv_wgrad.hip NP = 1).  autograd reads this at each recorded forward; ops itself only follows its `precision` arguments.
TRAIN_PRECISIONS = ("fp32", "bf16")
TRAIN_PRECISION = os.environ.get("EAVSR_TRAIN_PRECISION", "fp32")
if TRAIN_PRECISION not in TRAIN_PRECISIONS:
    raise ValueError(f"EAVSR_TRAIN_PRECISION={TRAIN_PRECISION!r}: one of {TRAIN_PRECISIONS}")


def check_precision(precision: str) -> str:
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"precision {precision!r}: one of {TRAIN_PRECISIONS}")
    return precision


# The opt-in deterministic training mode (networks.set_deterministic / EAVSR_DETERMINISTIC=0|1): the backward of flow_warp, of
# resize_bilinear_ac and of DCNv2 compute their input gradients without float atomics (csrc/det_scatter.hip), so that a training step
# is bitwise reproducible.  Also on whenever torch.are_deterministic_algorithms_enabled().  autograd reads deterministic_active() at
# each recorded forward; ops itself only follows what it is asked to launch.
_det_env = os.environ.get("EAVSR_DETERMINISTIC", "0")
if _det_env not in ("0", "1"):
    raise ValueError(f"EAVSR_DETERMINISTIC={_det_env!r}: 0 or 1")
DETERMINISTIC = _det_env == "1"


def deterministic_active() -> bool:
    return DETERMINISTIC or torch.are_deterministic_algorithms_enabled()


def _packed_conv3_bf16(weights: Sequence[Tensor], dgrad: bool = False) -> Tensor:
    """_packed_conv_x6 for eavsr_conv3x3_bf16x1s (the bf16 training mode): every value rounded once to bf16 (nearest even), one
    plane (eavsr_pack_conv_weight_bf16x1*); in _bf16_pack_cache, never among the exact forms"""
    return _packed("bf16x1", weights, dgrad)


def prepack_conv3_x6(weights: Sequence[Tensor], precision: Optional[str] = None) -> int:
    """Both packed forms (forward and input-gradient) of every (64, 64, 3, 3) weight in `weights` that the cache does not hold at
    the weight's current version, in ceil(count / 48) launches (eavsr_pack_conv_weight_x6_multi) instead of one launch per weight and
    form at its first use: what the training step calls once, in front of its forward (540 launches of 4.7 us on its one dependent
    chain otherwise).  precision (default: TRAIN_PRECISION, the mode the training convolutions run in): "bf16" packs the one-plane
    forms of the bf16 training mode instead (eavsr_pack_conv_weight_bf16x1_multi).  Returns the number of forms packed."""
    f = _FORMS["bf16x1" if check_precision(TRAIN_PRECISION if precision is None else precision) == "bf16" else "x6"]
    cache, nbytes_fn, multi = f.cache, f.size.split()[0], f.pack.split()[0] + "_multi"
    todo = []
    for w in weights:
        if tuple(w.shape) != (64, 64, 3, 3) or not w.is_cuda or not w.is_contiguous() or w.dtype != torch.float32:
            continue
        for dg in (False, True):
            if cache.lookup((w,), "dgrad" if dg else None) is None:
                todo.append((w, dg))
    if not todo:
        return 0
    dev = todo[0][0].device
    nbytes = int(getattr(lib(), nbytes_fn)(3, 64, 64))
    store = torch.empty((len(todo), nbytes), device=dev, dtype=torch.uint8)
    cnt = len(todo)
    srcs = (C.c_void_p * cnt)(*[w.detach().data_ptr() for w, _ in todo])
    dsts = (C.c_void_p * cnt)(*[store[i].data_ptr() for i in range(cnt)])
    trs = (C.c_int32 * cnt)(*[int(dg) for _, dg in todo])
    with _DeviceOf(todo[0][0]):
        N.check(getattr(lib(), multi)(srcs, dsts, trs, cnt, 3, 64, _stream(todo[0][0])), multi[len("eavsr_"):])
    for i, (w, dg) in enumerate(todo):
        cache.store((w,), "dgrad" if dg else None, store[i])
    return cnt


# The 16-bit modes' generic 3x3 convolution (csrc/conv3_h16.hip): None = off (fp32 everywhere, the default), "bf16" / "fp16" =
# every plain 3x3 convolution with >= 32 output channels whose sources have channel counts % 16 == 0 rounds its operands to that
# type (fp32 NCHW in and out).  Set by networks.set_backbone_dtype (EAVSR_CONV3_16BIT=0 keeps these convolutions fp32: A/B switch).
CONV3_H16 = None
CONV3_H16_ENABLED = os.environ.get("EAVSR_CONV3_16BIT", "1") == "1"


def set_conv3_h16(dtype) -> None:
    global CONV3_H16
    if dtype is not None:
        h16_code(dtype)
    CONV3_H16 = dtype if CONV3_H16_ENABLED else None


def _packed_h16g(weights: Sequence[Tensor], code: int) -> Tensor:
    return _packed("h16g", weights, code)


# SPyNet's 7x7 layers with >= 16 output channels in the 16-bit modes (one operand plane of csrc/conv_x6.hip); EAVSR_CONV7_16BIT=0
# keeps them on the exact bf16x6 form (A/B switch)
CONV7_H16_ENABLED = os.environ.get("EAVSR_CONV7_16BIT", "1") == "1"


def _packed_h16x1(weights: Sequence[Tensor], code: int) -> Tensor:
    return _packed("h16x1", weights, code)


# ------------------------------------------------------------------------------------------
# dense conv  (nn.Conv2d, stride 1, "same" padding)
# ------------------------------------------------------------------------------------------
# The launch-size gates, each written once, over plain numbers: conv_route and the public predicates below all ask these.
def _x6s_gate(n: int, h: int, w: int) -> bool:
    """mode and size of the crop-sized bf16x6 kernel (eavsr_conv3x3_f32x6s): at most X6S_MAX_TILES of its 8 x 32-pixel tiles"""
    return (CONV3_SMALL == "x6s" and CONV_MODE in ("winograd", "winograd4")
            and _rn(n) * lib().eavsr_conv3x3_x6s_tiles(h, w) <= X6S_MAX_TILES)


def _wino_gate(n: int, h: int, w: int) -> bool:
    """mode and size of the Winograd 3x3 kernels: at least WINO_MIN_TILES 8 x 32-pixel tiles"""
    return CONV_MODE in ("winograd", "winograd4") and _rn(n) * _wino_tiles(h, w) >= WINO_MIN_TILES


def _wino4_gate(n: int, h: int, w: int) -> bool:
    """F(4x4, 3x3) behind _wino_gate: same 512-pixel-per-workgroup granularity (8 x 64)"""
    return CONV_MODE == "winograd4" and 2 * _rn(n) * lib().eavsr_conv3x3_wino4_tiles(h, w) >= WINO_MIN_TILES


def _wino5_gate(n: int, h: int, w: int, cout: int) -> bool:
    """5x5 (the predictor's offset / mask heads) by F(2x2, 5x5): the same 6 x 6 tile pipeline, 4 x 32-pixel tiles"""
    return CONV_MODE == "winograd4" and _rn(n) * lib().eavsr_conv5x5_wino_tiles(h, w) * ((cout + 63) // 64) >= 2 * WINO_MIN_TILES


def _wino_ca_gate(n: int, h: int, w: int, c: int, mod16: int) -> bool:
    """the channel-attention prologue inside the Winograd kernel's input transform (lab build)"""
    return lab_available() and w % 4 == 0 and c % 8 == 0 and c <= 256 and mod16 == 0 and _wino_gate(n, h, w)


def _direct_ca_gate(n: int, h: int, w: int, c: int, cout: int, mod16: int) -> bool:
    """the channel-attention prologue of the direct kernel: its 32-row, 16-byte-DMA path"""
    return (w % 4 == 0 and c % 4 == 0 and c <= 256 and 32 < cout <= 64 and mod16 == 0
            and lib().eavsr_conv2d_tile_rows(n, h, w, 3) == 32)


def x6s_takes(n: int, h: int, w: int) -> bool:
    """a single-source 3x3 64 -> 64 launch of this size runs on eavsr_conv3x3_f32x6s (the crop-sized bf16x6 kernel) in the current mode"""
    return CONV3_H16 is None and _x6s_gate(n, h, w)


def _wino_fusable(x: Tensor) -> bool:
    return x.dim() == 4 and x.is_contiguous() and _wino_ca_gate(*(int(v) for v in (x.shape[0], x.shape[2], x.shape[3], x.shape[1])), x.data_ptr() % 16)


def ca_fusable(x: Tensor, cout: int = 64) -> bool:
    """Can the channel-attention tail `r * scale + x` be folded into the next 3x3 conv?  Yes where the Winograd kernel
    runs (its input transform applies it), or on the direct kernel's 32-row, 16-byte-DMA path."""
    if _wino_fusable(x):
        return True
    return (x.dim() == 4 and x.is_contiguous()
            and _direct_ca_gate(int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), int(x.shape[1]), cout, x.data_ptr() % 16))


# EAVSR_FUSE_SHUFFLE=0: the upsampling tail's PixelShuffle(2) as a torch copy instead of the conv kernel's store pattern (A/B switch)
FUSE_PIXEL_SHUFFLE = os.environ.get("EAVSR_FUSE_SHUFFLE", "1") == "1"


_dgrad_w_cache = WeightCache()


def dgrad_weight(w: Tensor) -> Tensor:
    """(cin, cout, k, k) transposed and flipped copy of a forward weight: the weight of its input-gradient convolution; cached
    per weight object and version"""
    return _dgrad_w_cache.derive((w,), None, lambda: w.detach().flip(2, 3).transpose(0, 1).contiguous())


class BorderPieces:
    """what conv2d(.., border=True) leaves beside the per-tile channel sums: `data` (n, 4, stride, 64) -- border 0 / 1 = image row 0 /
    h - 1 (`p_rows` pieces of 64 columns), 2 / 3 = image column 0 / w - 1 (`p_cols` pieces of 4 rows) of act(conv + bias), i.e. of what the
    channel sums add up: the convolution's output BEFORE the residual (desc.border_pieces; DESIGN.md 4b has the layout)"""
    __slots__ = ("data", "p_rows", "p_cols")

    def __init__(self, data: Tensor, p_rows: int, p_cols: int):
        self.data, self.p_rows, self.p_cols = data, int(p_rows), int(p_cols)


class ConvRoute(NamedTuple):
    """what conv_route decides for one conv2d call: ONE convolution launch and the steps behind it"""
    family: str                         # the kernel family (a key of _CONV_KERNELS, "_ca" appended with the fused prologue)
    name: str                           # the name ops.profile records for the launch
    post: Tuple[str, ...] = ()          # then, in order: "plane_sum" / "scale_residual" (launches), "pixel_shuffle" / "sigmoid" (torch)
    cat: bool = False                   # the ragged sources are concatenated first
    materialise: bool = False           # dgrad: the launch takes dgrad_weight(weight) as a forward weight (else: packed in place)
    part_tiles: Optional[int] = None    # the tile axis of the chan_partial / sum_mul result
    pieces: bool = False                # border=True returns BorderPieces (else None)

    @property
    def kernels(self) -> Tuple[str, ...]:
        """the names ops.profile records, in launch order"""
        return (self.name,) + tuple(p for p in self.post if p in ("plane_sum", "scale_residual"))

    @property
    def families(self) -> Tuple[str, ...]:
        return (self.family,) + self.kernels[1:]


def conv_route(n: int, h: int, w: int, k: int, chans: Sequence[int], cout: int, n_weights: int = 1, bias: bool = True, *,
               act: Optional[str] = None, residual: bool = False, chan_partial: bool = False, ca: bool = False, ca_out: bool = False,
               pixel_shuffle2: bool = False, res_scale: bool = False, sum_mul: bool = False, dgrad: bool = False,
               sigmoid_from: Optional[int] = None, border: bool = False, precision: str = "fp32", src_mod: Optional[Sequence[int]] = None,
               residual_mod: int = 0, ca_mod: int = 0, sum_mul_mod: int = 0, sum_mul_shaped: bool = True, grad: bool = True) -> ConvRoute:
    """Which kernel one conv2d call runs on and what follows it, from plain values alone: no tensor, no allocation, no launch, no
    device.  chans: the sources' channel counts; cout: the call's OUTPUT channels (dgrad: the forward weight's input channels); the
    option flags say whether conv2d's argument of that name is given; *_mod: the operand's address modulo 16 (src_mod: one per
    source); sum_mul_shaped: sum_mul has the output's shape; grad: autograd is enabled.  Reads the kernel modes and thresholds of
    this module, the pinned route batch and the library's host-side tile counters.  Raises what conv2d raises for a combination its
    docstring rules out (ValueError) and for a prologue no kernel can fuse (NotImplementedError)."""
    chans = tuple(int(c) for c in chans)
    cin, single = sum(chans), len(chans) == 1
    src_mod = tuple(src_mod) if src_mod is not None else (0,) * len(chans)
    masked = act == "relu_mask"    # out = residual > 0 ? conv : 0 (a ReLU's backward inside the input-gradient convolution): direct kernels only
    cat = False

    def route(fam, **kw):
        ca_ = "_ca" if ca else ""
        return ConvRoute(fam + ca_, f"conv{k}x{k}_{cin}to{cout}{_CONV_KERNELS[fam][0]}{ca_}", cat=cat, **kw)

    def two_step(step, **opts):
        """a fallback form: the route of the simpler call (on the sources as they are by now) and one more step behind it"""
        r = conv_route(n, h, w, k, chans, cout, **{**dict(n_weights=n_weights, bias=bias, act=act, src_mod=src_mod, grad=grad), **opts})
        return r._replace(post=r.post + step, cat=cat or r.cat, part_tiles=1 if step == ("plane_sum",) else r.part_tiles)

    check_precision(precision)
    if sum_mul and (not dgrad or chan_partial or ca or pixel_shuffle2 or sigmoid_from is not None or res_scale or masked):
        raise ValueError("sum_mul: input-gradient convolutions only (dgrad=True; no channel sums / prologue / shuffle / sigmoid / mask)")
    if dgrad:
        if n_weights != 1 or bias or chan_partial or ca or pixel_shuffle2 or sigmoid_from is not None or res_scale:
            # (res_scale: on every route -- the materialised-weight routes below would drop it)
            raise ValueError("dgrad: one forward weight, no bias / channel sums / prologue / shuffle / sigmoid / scaled residual")
        # only the small-launch bf16x6 kernel reads the forward weight in place (necessary conditions; the decision is below)
        if not (k == 3 and single and cin == 64 and cout not in (2, 3, 4, 6) and x6s_takes(n, h, w)):
            r = two_step(("plane_sum",) if sum_mul else (), bias=False, residual=residual, residual_mod=residual_mod)
            return r._replace(materialise=True)
    if pixel_shuffle2 and (cout % 4 or residual or chan_partial or ca):
        raise ValueError("pixel_shuffle2: cout % 4 == 0, no residual / channel sums / channel-attention prologue")
    if res_scale and (not residual or chan_partial or ca or pixel_shuffle2 or sigmoid_from is not None or dgrad or masked):
        raise ValueError("res_scale: with `residual`; no channel sums / prologue / shuffle / sigmoid / dgrad / mask")
    if masked and (not residual or chan_partial or ca or pixel_shuffle2 or sigmoid_from is not None):
        raise ValueError("act='relu_mask': residual = the ReLU's forward output; no channel sums / prologue / shuffle / sigmoid")
    if ca_out and not ca:          # before any early return (the bf16x6 route used to skip this check)
        raise ValueError("ca_out needs ca")
    x6_mode = ((k == 7 and CONV7_MODE == "bf16x6") or (k == 5 and CONV5_MODE == "bf16x6")) and single and cin % 8 == 0
    if sigmoid_from is not None:   # validated once, for every route (routes used to differ)
        if not 0 <= int(sigmoid_from) < cout:
            raise ValueError(f"sigmoid_from {int(sigmoid_from)}: 0 <= value < cout = {cout}")
        if residual or chan_partial or ca or pixel_shuffle2:
            raise ValueError("sigmoid_from: plain convolutions only")
        if not (x6_mode and int(sigmoid_from) % 8 == 0):      # every other kernel: the activations are one more pass over the output
            return two_step(("sigmoid",), act=None)           # (without `act`: the tail channels take the sigmoid INSTEAD of it)
    # ---- the kernels with a shape of their own
    if k == 3 and single and cout in (2, 3, 4, 6) and not chan_partial and not ca and not masked and not res_scale:
        lite = (SMALLCO_LITE and w % 4 == 0 and src_mod[0] == 0 and h * w * cin * 4 < 2 ** 32
                and _rn(n) * ((h + 7) // 8) * ((w + 63) // 64) >= SMALLCO_LITE_MIN_TILES)
        return route("smallco_lite" if lite else "smallco_classic", post=("pixel_shuffle",) if pixel_shuffle2 else ())
    bare = not (residual or chan_partial or ca or pixel_shuffle2)
    h16 = CONV3_H16 is not None and sigmoid_from is None and bare and not grad
    if h16 and k == 7 and CONV7_H16_ENABLED and single and cin % 8 == 0 and cout >= 16:
        return route("h16x1")      # SPyNet's feature layers (its 16 -> 2 flow head stays exact)
    if x6_mode and bare:
        return route("x6")
    if h16 and k == 3 and w % 4 == 0 and cout >= 32 and all(c % 16 == 0 for c in chans) and not any(src_mod):
        return route("h16g")
    # ---- the descriptor kernels
    if any(c % lib().eavsr_conv2d_ck(k) for c in chans[:-1]):
        chans, src_mod, single, cat = (cin,), (0,), True, True      # ragged middle source: materialise (tiny SPyNet inputs only)
    if CONV_MODE in ("winograd", "bf16x9"):      # (set through the environment: set_conv_mode() checks at the call)
        require_lab(f"conv mode {CONV_MODE!r}")
    lab = lab_available()
    base_ok = k == 3 and w % 4 == 0 and all(c % 8 == 0 for c in chans) and not any(src_mod)
    wino = _wino_gate(n, h, w) and base_ok and not masked and (not ca or (lab and single and cin <= 256 and ca_mod == 0))
    # F(4x4, 3x3): no fused channel-attention prologue
    wino4 = wino and (not residual or residual_mod == 0) and _wino4_gate(n, h, w)
    if wino and not wino4 and not lab:
        wino = False      # default build: F(2x2,3x3) is a lab kernel -- what F(4x4,3x3) does not take runs the direct kernel
    if res_scale and not (wino4 and cin % 8 == 0 and lib().eavsr_wino4_schedule() >= 1):
        return two_step(("scale_residual",))      # every other kernel: the convolution, then the tail as its own launch
    if pixel_shuffle2 and not (wino4 and FUSE_PIXEL_SHUFFLE):
        return two_step(("pixel_shuffle",))       # every other kernel: plain output, shuffled by torch
    wino5 = (k == 5 and not ca and not masked and w % 4 == 0 and all(c % 4 == 0 for c in chans) and not any(src_mod)
             and (not residual or residual_mod % 8 == 0) and _wino5_gate(n, h, w, cout))
    # small launches of the 64-channel 3x3 convolution (a training crop, a pyramid level): exact bf16x6 instead of the fp32 MFMA
    # (the explicit modes "direct" / "bf16x9" keep their own kernels: they are the A/B references)
    x6s = k == 3 and single and cin == 64 and not ca and not pixel_shuffle2 and not wino and _x6s_gate(n, h, w)
    if sum_mul and not (x6s and w % 4 == 0 and sum_mul_shaped and src_mod[0] == 0 and sum_mul_mod == 0
                        and (not residual or residual_mod == 0)):
        # the kernel's epilogue form does not apply: a plane-sum launch behind the input-gradient convolution
        return two_step(("plane_sum",), bias=False, dgrad=True, residual=residual, residual_mod=residual_mod, precision=precision)
    if ca:
        if not single:
            raise ValueError("ca=(scale, x): one source, x of the same shape, scale (n, cin)")
        if not wino and (k != 3 or ca_mod or not (_wino_ca_gate(n, h, w, cin, src_mod[0]) or _direct_ca_gate(n, h, w, cin, cout, src_mod[0]))):
            raise NotImplementedError("fused channel-attention prologue unavailable for this shape; use "
                                      "scale_residual + conv2d (see ops.ca_fusable)")
    if x6s:      # precision="bf16" (the bf16 training mode): the same launch with its operands rounded once to bf16
        fam, tiles = "bf16s" if precision == "bf16" else "x6s", lib().eavsr_conv3x3_x6s_tiles
    elif wino5:
        fam, tiles = "wino5", lib().eavsr_conv5x5_wino_tiles
    elif wino4:
        fam, tiles = "wino4", lib().eavsr_conv3x3_wino4_tiles
    elif wino:
        fam, tiles = "wino", _wino_tiles
    else:
        x9 = CONV_MODE == "bf16x9" and base_ok and not ca and not masked and lib().eavsr_conv2d_tile_rows(n, h, w, 3) == 32
        fam, tiles = "x9" if x9 else "direct", lambda h_, w_: lib().eavsr_conv2d_tiles(n, h_, w_, k)
    pieces = bool(border and chan_partial and wino4 and cout == 64 and cin % 8 == 0 and not ca and not pixel_shuffle2 and not res_scale
                  and lib().eavsr_wino4_schedule() == 1)
    return route(fam, materialise=dgrad and not x6s,      # (e.g. a large input-gradient launch that the Winograd kernel takes)
                 part_tiles=int(tiles(h, w)) if chan_partial or sum_mul else None, pieces=pieces)


def _flat(entry: str, *fields: str, aux: bool = False):
    """the launch of a kernel with a flat argument list: x, weight, then the named descriptor fields [, aux], stream"""
    return lambda L, d, wq, a, st: getattr(L, entry)(d.src[0], wq, *(getattr(d, f) for f in fields), *((a,) if aux else ()), st)


# family -> (suffix of the profile name, the descriptor's weight(weights, aux), the kernel's own weight(weights, dgrad, aux),
#            launch(library, descriptor, own weight's address, aux, stream), the `what` of N.check)
# aux: the 16-bit type code (h16x1, h16g); the first channel of the fused sigmoid or -1 (x6)
_SMALLCO_ARGS = ("bias", "residual", "out", "n", "cin", "h", "w", "cout", "act", "slope")
_X6_ARGS = ("bias", "out", "n", "cin", "cout", "h", "w", "ksize", "act", "slope")
_CONV_KERNELS = {
    "smallco_lite": ("", None, lambda ws, dg, a: _packed_smallco(list(ws)), _flat("eavsr_conv3x3_smallco_lite_f32", *_SMALLCO_ARGS), "conv3x3_smallco_lite"),
    "smallco_classic": ("", None, lambda ws, dg, a: _cat_weights(ws), _flat("eavsr_conv3x3_smallco_f32", *_SMALLCO_ARGS), "conv3x3_smallco"),
    "x6": ("_x6", None, lambda ws, dg, a: _packed_conv_x6(ws), _flat("eavsr_conv_f32x6", *_X6_ARGS, aux=True), "conv_f32x6"),
    "h16x1": ("_h16x1", None, lambda ws, dg, a: _packed_h16x1(ws, a), _flat("eavsr_conv_h16x1", *_X6_ARGS, aux=True), "conv_h16x1"),
    "h16g": ("_h16g", lambda ws, a: _packed_h16g(ws, a), None, lambda L, d, wq, a, st: L.eavsr_conv3x3_h16g_f32(C.byref(d), a, st), "conv3x3_h16g"),
    # (the x6s kernel has its own packed form, also of the input-gradient convolution's weight, straight from the forward weight)
    "bf16s": ("_bf16s", None, lambda ws, dg, a: _packed_conv3_bf16(ws, dgrad=dg), lambda L, d, wq, a, st: L.eavsr_conv3x3_bf16x1s(C.byref(d), wq, st), "conv3x3_bf16x1s"),
    "x6s": ("_x6s", None, lambda ws, dg, a: _packed_conv_x6(ws, dgrad=dg), lambda L, d, wq, a, st: L.eavsr_conv3x3_f32x6s(C.byref(d), wq, st), "conv3x3_f32x6s"),
    "wino5": ("_wino", lambda ws, a: _packed_f32(ws), lambda ws, dg, a: _packed_wino(ws, kind="f5"), lambda L, d, wq, a, st: L.eavsr_conv5x5_wino_f32(C.byref(d), wq, st), "conv5x5_wino"),
    "wino4": ("_wino4", lambda ws, a: _packed_f32(ws), lambda ws, dg, a: _packed_wino(ws, four=True), lambda L, d, wq, a, st: L.eavsr_conv3x3_wino4_f32(C.byref(d), wq, st), "conv3x3_wino4"),
    "wino": ("_wino", lambda ws, a: _packed_f32(ws), lambda ws, dg, a: _packed_wino(ws), lambda L, d, wq, a, st: L.eavsr_conv3x3_wino_f32(C.byref(d), wq, st), "conv3x3_wino"),
    "x9": ("_x9", lambda ws, a: _packed_f32(ws), lambda ws, dg, a: _packed_x9(ws), lambda L, d, wq, a, st: L.eavsr_conv3x3_f32x9(C.byref(d), wq, st), "conv3x3_f32x9"),
    "direct": ("", lambda ws, a: _packed_f32(ws), None, lambda L, d, wq, a, st: L.eavsr_conv2d_f32(C.byref(d), st), "conv2d"),
}


def _conv_desc(srcs: Sequence[Tensor], k: int, cout: int, weight_packed, bias, out, act, slope: float) -> "N.ConvDesc":
    """struct eavsr_conv2d_desc of a plain convolution; the caller adds the optional operands"""
    d = N.ConvDesc()      # (zero-filled: unused sources, every optional operand)
    for i, s in enumerate(srcs):
        d.src[i], d.src_c[i] = _p(s), int(s.shape[1])
    d.n_src, d.ksize = len(srcs), k
    d.weight_packed, d.bias, d.out = _p(weight_packed), _p(bias), _p(out)
    d.n, d.h, d.w = int(srcs[0].shape[0]), int(srcs[0].shape[2]), int(srcs[0].shape[3])
    d.cin, d.cout = sum(int(s.shape[1]) for s in srcs), cout
    d.act, d.slope = ACT[act], float(slope)
    return d


def _conv_cost(n: int, h: int, w: int, k: int, cin: int, cout: int, residual: bool, reads_per_input: int = 1) -> Tuple[float, float]:
    """algorithmic (FLOPs, bytes) of one convolution launch as `_launch` records them.  reads_per_input: 2 with the channel-attention
    prologue (the input and `x`), 3 when the effective input is written back as well (ca_out)"""
    px = float(n) * h * w
    return 2.0 * cin * cout * k * k * px, 4.0 * px * (cin * reads_per_input + cout + (cout if residual else 0))


def conv2d(srcs: Union[Tensor, Sequence[Tensor]], weight: Union[Tensor, Sequence[Tensor]],
           bias: Union[None, Tensor, Sequence[Optional[Tensor]]] = None, act: Optional[str] = None,
           slope: float = 0.0, residual: Optional[Tensor] = None, chan_partial: bool = False,
           ca: Optional[Tuple[Tensor, Tensor]] = None, ca_out: bool = False, pixel_shuffle2: bool = False,
           sigmoid_from: Optional[int] = None, dgrad: bool = False, res_scale: Optional[Tensor] = None, border: bool = False,
           sum_mul: Optional[Tensor] = None, precision: str = "fp32"):
    """conv over the virtual channel-concatenation of `srcs`; `weight` may be a list of weights
    that are concatenated along cout (several heads in one launch).
    border=True (with chan_partial=True): a last result, the sums of act(conv + bias) (before the residual) over the four border lines per border tile
    (`BorderPieces`, for ca_scale_pre(.., border=)) where the grouped F(4x4,3x3) kernel runs, None on every other route.
    res_scale (n, cout) with `residual`: out = residual + res_scale[n, co] * act(conv + bias) -- RCABlock's tail as the epilogue of
    the F(4x4,3x3) kernel (the attention from ca_scale_pre BEFORE the launch); other routes: the convolution, then scale_residual.
    dgrad=True: `weight` is ONE forward weight (cout_w, cin_w, k, k) and the call computes the input gradient of its stride-1
    "same" convolution from srcs = dY (cout_w channels): the convolution with the transposed, flipped weight.  The small-launch
    bf16x6 kernel packs that form straight from `weight`; every other route materialises it once per weight version.
    sigmoid_from=c: output channels >= c (a multiple of 8) leave through the sigmoid instead of `act` (the mask head of the
    predictor, networks.py:313-314) -- in the epilogue of the bf16x6 5x5 / 7x7 kernel, by torch on every other route.
    pixel_shuffle2=True returns F.pixel_shuffle(out, 2) -- written by the F(4x4,3x3) kernel's epilogue itself where that kernel
    runs (the upsampling tail, eavsrp_model.py:343-347), by torch otherwise.
    ca=(scale (n,c), x (n,c,h,w)): the conv input is srcs * scale[n,c] + x (RCABlock tail fused into this
    conv); with ca_out=True that effective input is also returned.
    sum_mul=m (n, cout, h, w), with dgrad: also returns (n, rows, cout) partial sums over the plane of out * m -- `sum_hw d r`, what the
    backward of the PREVIOUS RCAB's tail starts with -- from the epilogue of the small-launch bf16x6 kernel (desc.sum_mul), by a
    plane-sum launch behind every other kernel (rows = 1).
    precision="bf16" (the bf16 training mode; autograd passes it): where the crop-sized kernel takes the launch (x6s_takes), it runs
    with its operands rounded once to bf16 (eavsr_conv3x3_bf16x1s); every other route ignores it and stays as it is.
    Returns out, then the per-tile channel sums when chan_partial=True, then the effective input when
    ca_out=True.  Which kernel runs, and every combination that is refused: conv_route."""
    # ---- the arguments, normalised
    check_precision(precision)      # (before any tensor is looked at)
    srcs = [_chk(s, f"src{i}") for i, s in enumerate([srcs] if isinstance(srcs, torch.Tensor) else srcs)]
    weights = [weight] if isinstance(weight, torch.Tensor) else list(weight)
    biases = [bias] if (bias is None or isinstance(bias, torch.Tensor)) else list(bias)
    residual, res_scale, sum_mul = (None if t is None else _chk(t, nm) for t, nm in
                                    ((residual, "residual"), (res_scale, "res_scale"), (sum_mul, "sum_mul")))
    if ca is not None:
        ca = (_chk(ca[0], "ca scale"), _chk(ca[1], "ca x"))
    sigmoid_from = None if sigmoid_from is None else int(sigmoid_from)
    # ---- the facts of the call
    if not 1 <= len(srcs) <= 5:
        raise ValueError("1..5 sources")
    n, _, h, w = (int(v) for v in srcs[0].shape)
    if any(s.shape[0] != n or tuple(s.shape[2:]) != (h, w) for s in srcs):
        raise ValueError("all sources must share n,h,w")
    chans = [int(s.shape[1]) for s in srcs]
    cin, k = sum(chans), int(weights[0].shape[-1])
    cout = int(weights[0].shape[1]) if dgrad else sum(int(x.shape[0]) for x in weights)
    if dgrad and len(weights) == 1 and int(weights[0].shape[0]) != cin:
        raise ValueError(f"dgrad: the forward weight has {int(weights[0].shape[0])} output channels, dY gives {cin}")
    if not dgrad and any(int(x.shape[1]) != cin for x in weights):
        raise ValueError(f"weight expects {[int(x.shape[1]) for x in weights]} input channels, sources give {cin}")
    if residual is not None and tuple(residual.shape) != (n, cout, h, w):
        raise ValueError("residual shape mismatch")
    if res_scale is not None and tuple(res_scale.shape) != (n, cout):
        raise ValueError(f"res_scale must be (n, cout) = ({n}, {cout})")
    if ca is not None and (tuple(ca[1].shape) != (n, cin, h, w) or tuple(ca[0].shape) != (n, cin)):
        raise ValueError("ca=(scale, x): one source, x of the same shape, scale (n, cin)")
    mod16 = lambda t: 0 if t is None else t.data_ptr() % 16
    r = conv_route(n, h, w, k, chans, cout, len(weights), any(b is not None for b in biases), act=act, residual=residual is not None,
                   chan_partial=chan_partial, ca=ca is not None, ca_out=ca_out, pixel_shuffle2=pixel_shuffle2,
                   res_scale=res_scale is not None, sum_mul=sum_mul is not None, dgrad=dgrad, sigmoid_from=sigmoid_from, border=border,
                   precision=precision, src_mod=[mod16(s) for s in srcs], residual_mod=mod16(residual),
                   ca_mod=0 if ca is None else mod16(ca[1]), sum_mul_mod=mod16(sum_mul),
                   sum_mul_shaped=sum_mul is None or tuple(sum_mul.shape) == (n, cout, h, w), grad=torch.is_grad_enabled())
    # ---- what the route asks for in front of the launch, and what the launch itself applies (the rest: r.post)
    if r.cat:
        srcs = [torch.cat(srcs, 1)]
    if r.materialise:
        weights, dgrad = [dgrad_weight(weights[0])], False
    fam = r.family[:-3] if ca is not None else r.family
    l_act = None if "sigmoid" in r.post else act
    l_res, l_scale = (None, None) if "scale_residual" in r.post else (residual, res_scale)
    l_mul = None if "plane_sum" in r.post else sum_mul
    aux = h16_code(CONV3_H16) if fam in ("h16x1", "h16g") else -1 if sigmoid_from is None or "sigmoid" in r.post else int(sigmoid_from)
    # ---- allocate, describe, launch
    dev = srcs[0].device
    out = torch.empty((n, cout, h, w), device=dev, dtype=torch.float32)
    # The kernels with 16-byte stores want an aligned output.  Not a routing input: the caching allocator aligns a fresh tensor
    # far beyond 16 bytes, so this never chose a route -- an allocator that stops doing so must not pass silently.
    if out.data_ptr() % 16:
        raise RuntimeError(f"conv2d: the output was allocated at {out.data_ptr():#x}, not on a 16-byte boundary")
    part = torch.empty((n, r.part_tiles, cout), device=dev, dtype=torch.float32) if chan_partial or l_mul is not None else None
    xs = torch.empty_like(ca[1]) if ca is not None and ca_out else None
    _, desc_weight, own_weight, call, what = _CONV_KERNELS[fam]
    wd = None if desc_weight is None else desc_weight(weights, aux)
    wq = None if own_weight is None else own_weight(weights, dgrad, aux)
    b = _bias_of(biases)
    d = _conv_desc(srcs, k, cout, wd, b, out, l_act, slope)
    d.residual, d.chan_partial, d.res_scale, d.sum_mul = _p(l_res), _p(part), _p(l_scale), _p(l_mul)
    pieces = None
    if r.pieces:
        pr, pc = C.c_int32(0), C.c_int32(0)
        N.check(lib().eavsr_conv3x3_wino4_border_pieces(h, w, C.byref(pr), C.byref(pc)), "conv3x3_wino4_border_pieces")
        stride = max(pr.value, pc.value)
        pieces = BorderPieces(torch.empty((n, 4, stride, 64), device=dev, dtype=torch.float32), pr.value, pc.value)
        d.border_pieces, d.border_stride = _p(pieces.data), stride
    if pixel_shuffle2 and "pixel_shuffle" not in r.post:
        d.out_shuffle = 2
        out = out.view(n, cout // 4, 2 * h, 2 * w)      # the same buffer, written in the shuffled layout
    if ca is not None:
        d.ca_scale, d.ca_x, d.ca_out = _p(ca[0]), _p(ca[1]), _p(xs)
    st = _stream(out)
    flops, nbytes = _conv_cost(n, h, w, k, cin, cout, l_res is not None, 1 if ca is None else 3 if ca_out else 2)
    # (the 16-bit routes round their fp32 sources inside the kernel: counted as rounded, in front of the launch, under a census)
    _launch(r.name, flops, nbytes, out, lambda: call(lib(), d, _p(wq), aux, st), what,
            rounded=(srcs, CONV3_H16) if fam in ("h16x1", "h16g") else None)
    # ---- the second step of a fallback form
    for step in r.post:
        if step == "plane_sum":
            part = plane_sum(out, sum_mul).view(n, 1, -1)
        elif step == "scale_residual":
            out = scale_residual(out, res_scale, residual)
        elif step == "pixel_shuffle":
            out = torch.nn.functional.pixel_shuffle(out, 2)
        else:      # "sigmoid": the tail channels, and `act` on the others
            out[:, sigmoid_from:] = torch.sigmoid(out[:, sigmoid_from:])
            if ACT[act] == 1:
                out[:, :sigmoid_from].clamp_(min=0.0)
            elif ACT[act] == 2:
                torch.nn.functional.leaky_relu(out[:, :sigmoid_from], float(slope), inplace=True)
    res = [out] + ([part] if part is not None else []) + ([xs] if xs is not None else []) + ([pieces] if border else [])
    return res[0] if len(res) == 1 else tuple(res)


# ------------------------------------------------------------------------------------------
# DCNv2  (mmcv.ops.modulated_deform_conv2d as called at networks.py:627-630)
# ------------------------------------------------------------------------------------------
def _one(v):
    return int(v[0]) if isinstance(v, (tuple, list)) else int(v)


def modulated_deform_conv2d(input: Tensor, offset: Tensor, mask: Tensor, weight: Tensor,
                            bias: Optional[Tensor] = None, stride=1, padding=0, dilation=1, groups=1,
                            deform_groups=1) -> Tensor:
    """Same signature as mmcv.ops.modulated_deform_conv2d.  The reference's configuration (3x3, stride 1, padding 1,
    dilation 1, groups 1, channels per deformable group a multiple of 8: networks.py:577-583 + eavsrp_model.py:143) runs
    the fused LDS-window MFMA kernel; every other configuration of the signature runs eavsr_dcnv2_generic_f32 (a plain
    kernel, forward only).  There is no CPU path."""
    x = _chk(input, "input")
    cout, cin_g, kh, kw = (int(v) for v in weight.shape)
    n, cin, h, w = x.shape
    two = lambda v: (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))
    (sh, sw), (ph, pw), (dh, dw) = two(stride), two(padding), two(dilation)
    if cin_g * groups != cin:
        raise ValueError("weight / input channel mismatch")
    if cin % deform_groups or cout % groups:
        raise ValueError("channels not divisible by groups / deform_groups")
    ho = (h + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1
    wo = (w + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1
    offset = _chk(offset, "offset")
    mask = _chk(mask, "mask")
    if tuple(offset.shape) != (n, deform_groups * 2 * kh * kw, ho, wo):
        raise ValueError(f"offset shape {tuple(offset.shape)} != {(n, deform_groups * 2 * kh * kw, ho, wo)}")
    if tuple(mask.shape) != (n, deform_groups * kh * kw, ho, wo):
        raise ValueError(f"mask shape {tuple(mask.shape)} != {(n, deform_groups * kh * kw, ho, wo)}")
    b = None if bias is None else _chk(bias.detach(), "bias")
    out = torch.empty((n, cout, ho, wo), device=x.device, dtype=torch.float32)
    on_path = ((kh, kw) == (3, 3) and (sh, sw, ph, pw, dh, dw) == (1, 1, 1, 1, 1, 1) and groups == 1
               and (cin // deform_groups) % 8 == 0)
    if not on_path:
        if groups > 1 and (cout // groups) % 8:
            raise NotImplementedError("modulated_deform_conv2d: with conv groups > 1 the output channels per group must be "
                                      "a multiple of 8")
        wt = _chk(weight.detach(), "weight")
        st = _stream(x)
        _launch("dcnv2_generic", 2.0 * cin_g * kh * kw * cout * n * ho * wo,
                4.0 * n * (cin * h * w + (3 * deform_groups * kh * kw + cout) * ho * wo), x,
                lambda: lib().eavsr_dcnv2_generic_f32(_p(x), _p(offset), _p(mask), _p(wt), _p(b), _p(out), n, cin, h, w, cout,
                                                      kh, kw, sh, sw, ph, pw, dh, dw, groups, deform_groups, st),
                "dcnv2_generic")
        return out
    st = _stream(x)
    px = float(n) * h * w
    flops, nbytes = 2.0 * cin * 9 * cout * px, 4.0 * px * (cin + 27 * deform_groups + cout)
    octets = (cin // deform_groups) // 8
    if DCN_MODE in ("il6", "il9") and octets & (octets - 1) == 0:     # the IL8 kernel wants a power-of-two number of octets per group
        # generic callers hold an NCHW tensor: one conversion pass to the IL8 layout, then the hot-path kernel (inside
        # MultiAdSTN the warp before the call writes IL8 itself and the predictor heads are passed instead of offset / mask)
        return dcnv2_il(to_il8(x), offset, mask, weight, b, deform_groups, nprod=int(DCN_MODE[2]), heads=False)
    if DCN_MODE == "bf16x9":
        require_lab("dcn mode 'bf16x9'")
    if DCN_MODE == "bf16x9" and w % 4 == 0 and x.data_ptr() % 16 == 0:
        wx = _packed_dcn_x9(weight)
        _launch("dcnv2_x9", flops, nbytes, x,
                lambda: lib().eavsr_dcnv2_f32x9(_p(x), _p(offset), _p(mask), _p(wx), _p(b), _p(out), n, cin, h, w, cout,
                                                deform_groups, st), "dcnv2_f32x9")
        return out
    wp = _packed_f32([weight])
    _launch("dcnv2", flops, nbytes, x,
            lambda: lib().eavsr_dcnv2_f32(_p(x), _p(offset), _p(mask), _p(wp), _p(b), _p(out), n, cin, h, w, cout,
                                          deform_groups, st), "dcnv2")
    return out


def to_il8(x: Tensor) -> Tensor:
    """(n, c, h, w) fp32 -> "IL8" (n, c/8, h, w, 8): the 8 channels of a deformable group interleaved per pixel, the input
    layout of eavsr_dcnv2_il_f32"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    if c % 8:
        raise ValueError("to_il8: channels must be a multiple of 8")
    out = torch.empty((n, c // 8, h, w, 8), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("nchw_to_il8", 0.0, 8.0 * x.numel(), x,
            lambda: lib().eavsr_nchw_to_il8_f32(_p(x), _p(out), n, c, h, w, st), "nchw_to_il8")
    return out


def _dcn_il_args(op: str, x_il8: Tensor, offset_or_heads: Tensor, mask: Optional[Tensor], weight: Tensor, bias: Optional[Tensor],
                 deform_groups: int, heads: bool):
    """what `dcnv2_il` and `dcnv2_il16` ask of their arguments beyond the input's dtype (checked by the caller): the IL8 shape, the
    weight's channels, offset / mask or heads against it; (n, cin, h, w, cout, D, offset_or_heads, mask, bias) as the launch takes them"""
    n, oct_, h, w, e = x_il8.shape
    if e != 8:
        raise ValueError(f"{op}: input must be IL8 (n, c/8, h, w, 8)")
    cin, cout, D = oct_ * 8, int(weight.shape[0]), int(deform_groups)
    if tuple(weight.shape[1:]) != (cin, 3, 3):
        raise ValueError(f"{op}: weight / input channel mismatch")
    oh = _chk(offset_or_heads, "offset_or_heads")
    if heads:
        if tuple(oh.shape) != (n, 15 * D, h, w):
            raise ValueError(f"{op}: heads shape {tuple(oh.shape)} != {(n, 15 * D, h, w)}")
        mask = None
    else:
        mask = _chk(mask, "mask")
        if tuple(oh.shape) != (n, 18 * D, h, w) or tuple(mask.shape) != (n, 9 * D, h, w):
            raise ValueError(f"{op}: offset / mask shape")
    return n, cin, h, w, cout, D, oh, mask, None if bias is None else _chk(bias.detach(), "bias")


def dcnv2_il(x_il8: Tensor, offset_or_heads: Tensor, mask: Optional[Tensor], weight: Tensor, bias: Optional[Tensor],
             deform_groups: int, nprod: int = 6, heads: bool = False, mask_activated: bool = False) -> Tensor:
    """DCNv2 (3x3, stride 1, pad 1) on an IL8 input.  heads=False: `offset_or_heads` / `mask` as mmcv's offset (n,18D,h,w)
    and mask (n,9D,h,w).  heads=True: `offset_or_heads` is the (n,15D,h,w) output of AdaptBlockOffset's three 5x5 heads and
    the kernel applies networks.py:302-315 (affine -> offsets, sigmoid) itself.  nprod: 9 = exact bf16x9, 6 = the three
    smallest products dropped (together below 2^-21 of each product x * w: DESIGN.md 4a)."""
    x_il8 = _chk(x_il8, "x_il8")
    n, cin, h, w, cout, D, oh, mask, b = _dcn_il_args("dcnv2_il", x_il8, offset_or_heads, mask, weight, bias, deform_groups, heads)
    if heads and _dcn_probe is not None:
        _dcn_probe.append(dcn_offset_stats(oh, D))
    impl = DCN_IL_IMPL
    if impl == "il2" and cin % 16:
        impl = "il"           # the round-4 schedule contracts groups in pairs
    if mask_activated and not (heads and impl == "il2"):
        raise ValueError("mask_activated: heads mode of the 'il2' schedule only (see heads_mask_activated())")
    wx = _packed_dcn_il2(weight) if impl == "il2" else _packed_dcn_x9(weight)
    out = torch.empty((n, cout, h, w), device=x_il8.device, dtype=torch.float32)
    st = _stream(out)
    px = float(n) * h * w
    # algorithmic bytes of the DCNv2 op as SURVEY 8d defines them (input + 27 D offset/mask + output); in heads mode the
    # kernel itself moves (cin + 15 D + cout) floats per pixel
    if impl == "ws":
        require_lab("the wave-specialised DCNv2 schedule 'ws'")
    fn = getattr(lib(), {"ws": "eavsr_dcnv2_ws_f32", "il": "eavsr_dcnv2_il_f32", "il2": "eavsr_dcnv2_il2_f32"}[impl])
    _launch("dcnv2_il" + ("_heads" if heads else ""), 2.0 * cin * 9 * cout * px, 4.0 * px * (cin + 27 * D + cout), out,
            lambda: fn(_p(x_il8), _p(oh), _p(mask), _p(wx), _p(b), _p(out), n, cin, h, w, cout, D,
                       int(nprod), (2 if mask_activated else 1) if heads else 0, st), "dcnv2_il")
    return out


def heads_mask_activated(cin: int, deform_groups: int = 8) -> bool:
    """True when the fused alignment should ask the predictor's heads convolution for MASKS (sigmoid in its epilogue,
    networks.py:313-314) rather than mask logits: the round-4 DCNv2 schedule takes them as they are (heads = 2), which moves four
    vector instructions per sample out of the kernel whose bound is vector issue.  The epilogue activates whole octets of output
    channels, so the first mask channel 6 D must be a multiple of 8 (D = 4, 8, ..; ADVICE r4: D = 1 / 2 used to raise)."""
    return (DCN_IL_IMPL == "il2" and cin % 16 == 0 and CONV5_MODE == "bf16x6" and HEADS_MASK_ACTIVATED
            and (6 * int(deform_groups)) % 8 == 0)


_dcn_probe = None      # bench.py: a list that collects offset statistics of every heads-mode DCNv2 call inside `dcn_probe()`


class dcn_probe:
    """Collect, per heads-mode DCNv2 call inside the scope, what the sampler saw: the offsets implied by the predictor heads
    (networks.py:302-315) and how many samples left the kernel's LDS window (served from global memory)."""

    def __enter__(self):
        global _dcn_probe
        _dcn_probe = []
        return _dcn_probe

    def __exit__(self, *exc):
        global _dcn_probe
        _dcn_probe = None
        return False


def dcn_offset_stats(heads: Tensor, D: int, tile_h: int = 8, tile_w: int = 32, margin_up: int = 6, margin_left: int = 8,
                     win_h: int = 20, win_w: int = 48) -> dict:
    """Statistics of the 18 D offsets that AdaptBlockOffset's heads imply (offset = T.R - R + t per deformable group) and the
    fraction of (pixel, tap) samples whose bilinear corners leave the DCNv2 kernel's LDS window (tile 8 x 32, window rows
    y0-6 .. y0+13, columns x0-8 .. x0+39: csrc/dcnv2_il2.hip).  Plain torch on the tensor's device; measurement only."""
    n, _, h, w = heads.shape
    T = heads[:, :4 * D].view(n, D, 2, 2, h, w)
    t = heads[:, 4 * D:6 * D].view(n, D, 2, 1, h, w)
    ky = torch.tensor([-1., -1., -1., 0., 0., 0., 1., 1., 1.], device=heads.device)
    kx = torch.tensor([-1., 0., 1., -1., 0., 1., -1., 0., 1.], device=heads.device)
    R = torch.stack([ky, kx], 0).view(1, 1, 2, 9, 1, 1)
    off = (T[:, :, :, 0:1] * R[:, :, 0:1] + T[:, :, :, 1:2] * R[:, :, 1:2]) - R + t      # (n, D, 2, 9, h, w): dy, dx per tap
    dy, dx = off[:, :, 0], off[:, :, 1]
    ys = torch.arange(h, device=heads.device).view(1, 1, 1, h, 1) % tile_h
    xs = torch.arange(w, device=heads.device).view(1, 1, 1, 1, w) % tile_w
    ry = margin_up + ys + ky.view(1, 1, 9, 1, 1) + torch.floor(dy)
    rx = margin_left + xs + kx.view(1, 1, 9, 1, 1) + torch.floor(dx)
    outside = (ry < 0) | (ry > win_h - 2) | (rx < 0) | (rx > win_w - 2)
    mag = torch.sqrt(dy * dy + dx * dx)
    return {"mean_abs_dy": float(dy.abs().mean()), "mean_abs_dx": float(dx.abs().mean()), "mean_norm": float(mag.mean()),
            "sigma_dy": float(dy.std()), "sigma_dx": float(dx.std()), "max_abs": float(torch.maximum(dy.abs().max(), dx.abs().max())),
            "frac_outside_lds_window": float(outside.float().mean())}


# Schedule of the IL8 DCNv2 kernel (same arithmetic, same arguments): "il" = eavsr_dcnv2_il_f32, every wave samples and
# contracts (default: faster at the alignment's offsets, |offset| of a few pixels); "ws" = eavsr_dcnv2_ws_f32, wave-specialised
# samplers / contractors (csrc/dcnv2_ws.hip): ~18 % slower there, 8-15 % faster when many samples leave the LDS window
# (sigma = 4 px), because its out-of-window samples are blended in line instead of in a second MFMA pass.  DESIGN.md 4b.
# "il2" = eavsr_dcnv2_il2_f32 (csrc/dcnv2_il2.hip, round 4): the two groups of a pair as nine full k-steps in one software
# pipeline across group / pair / tile boundaries (same operands and products; falls back to "il" when cin % 16 != 0).
DCN_IL_IMPL = os.environ.get("EAVSR_DCN_IL_IMPL", "il2")
HEADS_MASK_ACTIVATED = os.environ.get("EAVSR_HEADS_SIGMOID", "1") != "0"      # A/B switch of heads_mask_activated()


def set_dcn_il_impl(impl: str) -> None:
    global DCN_IL_IMPL
    if impl not in ("il", "ws", "il2"):
        raise ValueError(f"dcn il impl {impl!r}: 'il', 'il2' or 'ws'")
    if impl == "ws":
        require_lab("the wave-specialised DCNv2 schedule 'ws'")
    DCN_IL_IMPL = impl


def _packed_dcn_il2(weight: Tensor) -> Tensor:
    """Pre-split (3 x bf16) weight slab of a 3x3 DCNv2 weight in the pair-step order of eavsr_dcnv2_il2_f32"""
    return _packed("il2", weight)


def _packed_il16(weight: Tensor, code: int) -> Tensor:
    return _packed("il16", weight, code)


def to_il8_h16(x: Tensor, dtype) -> Tensor:
    """(n, c, h, w) fp32 -> IL8 (n, c/8, h, w, 8) rounded to 'fp16' / 'bf16'"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    if c % 8:
        raise ValueError("to_il8_h16: channels must be a multiple of 8")
    code = h16_code(dtype)
    out = torch.empty((n, c // 8, h, w, 8), device=x.device, dtype=_H16_TORCH[code])
    st = _stream(x)
    _launch("nchw_to_il8_h16", 0.0, 6.0 * x.numel(), x,
            lambda: lib().eavsr_nchw_to_il8_h16(_p(x), _p(out), n, c, h, w, code, st), "nchw_to_il8_h16", stored=(out,))
    return out


def dcnv2_il16(x_il8: Tensor, offset_or_heads: Tensor, mask: Optional[Tensor], weight: Tensor, bias: Optional[Tensor],
               deform_groups: int, heads: bool = False) -> Tensor:
    """DCNv2 (3x3, stride 1, pad 1) on a 16-bit IL8 input (bf16 / fp16 samples and weights, fp32 blend and accumulation,
    fp32 output); arguments as `dcnv2_il`."""
    x_il8 = _chk_h16(x_il8, "x_il8")
    n, cin, h, w, cout, D, oh, mask, b = _dcn_il_args("dcnv2_il16", x_il8, offset_or_heads, mask, weight, bias, deform_groups, heads)
    code = h16_code(x_il8.dtype)
    wp = _packed_il16(weight, code)
    out = torch.empty((n, cout, h, w), device=x_il8.device, dtype=torch.float32)
    st = _stream(out)
    px = float(n) * h * w
    # algorithmic bytes of the 16-bit DCNv2 as SURVEY 8a counts them: 344 elements x 2 bytes per pixel
    _launch("dcnv2_il16" + ("_heads" if heads else ""), 2.0 * cin * 9 * cout * px, 2.0 * px * (cin + 27 * D + cout), out,
            lambda: lib().eavsr_dcnv2_il16(_p(x_il8), _p(oh), _p(mask), _p(wp), _p(b), _p(out), n, cin, h, w, cout, D, code,
                                           1 if heads else 0, st), "dcnv2_il16", stored=())
    return out


# How DCNv2 runs (fp32 tensors in and out in every mode):
#   "il6" (default) = the round-2 hot-path kernel eavsr_dcnv2_il_f32: IL8 input layout, both fp32 operands split exactly into
#              three bf16 terms, the six partial products that matter on the bf16 MFMA, fp32 accumulation (the three dropped
#              products are < 2^-21 of their product x * w together, mid*lo and lo*mid < 2^-22 each: eight units of 2^-24, not
#              "one fp32 rounding" -- DESIGN.md 4a, tests/product_probe.py).  Inside MultiAdSTN (inference) it is fed by the
#              paired warp (IL8 output) and by the predictor's head channels directly (affine -> offsets and the mask sigmoid
#              happen in the kernel); a plain modulated_deform_conv2d call converts its NCHW input first.
#   "il9"    = the same kernel with all nine partial products (exact operands, only the fp32 accumulation rounds)
#   "native" = round 1's LDS-window kernel on v_mfma_f32_32x32x2_f32 (an fp32 fma chain)
#   "bf16x9" = round 1's bf16x9 kernel (NCHW input, LDS window per channel plane)
DCN_MODE = os.environ.get("EAVSR_DCN_MODE", "il6")


def set_dcn_mode(mode: str) -> None:
    global DCN_MODE
    if mode not in ("native", "bf16x9", "il6", "il9"):
        raise ValueError(f"dcn mode {mode!r}: 'native', 'bf16x9', 'il6' or 'il9'")
    if mode == "bf16x9":
        require_lab("dcn mode 'bf16x9' (the round-1 NCHW kernel with nine partial products)")
    DCN_MODE = mode


def _packed_x9(weights: Sequence[Tensor]) -> Tensor:
    """Pre-split (3 x bf16) weight slab of a 3x3 weight -- or of several stacked along cout -- for the bf16x9 kernels"""
    return _packed("x9", weights)


def _packed_dcn_x9(weight: Tensor) -> Tensor:
    return _packed_x9([weight])


# How the large 3x3 convolutions are computed (all fp32 in, fp32 out, fp32 accumulation):
#   "winograd" = Winograd F(2x2, 3x3) on v_mfma_f32_16x16x4_f32 (eavsr_conv3x3_wino_f32): 2.25x fewer
#                multiplications, what cuDNN / MIOpen run for fp32 3x3 convolutions; measured closer to fp64 than the
#                direct sum (tests/test_hip_ops.py)
#   "winograd4" (default) = Winograd F(4x4, 3x3) (eavsr_conv3x3_wino4_f32): 4x fewer multiplications, ~1e-5 relative
#                error per convolution instead of 4e-7 (end to end on the bench clip: 2.4e-7 against 1.8e-7, the path's
#                bound is 1e-3); falls back to F(2x2, 3x3) for the fused channel-attention prologue
#   "direct"   = direct sum on v_mfma_f32_32x32x2_f32 (eavsr_conv2d_f32) -- also what every shape the Winograd kernel
#                does not cover runs (small images, widths not a multiple of 4, channels not a multiple of 8, 1x1/5x5/7x7)
#   "bf16x9"   = direct sum with an exact three-way bf16 split of both operands, nine partial products in fp32
#                (eavsr_conv3x3_f32x9), opt-in
def _norm_conv_mode(mode: str) -> str:
    mode = {"native": "direct"}.get(mode, mode)
    if mode not in ("direct", "winograd", "winograd4", "bf16x9"):
        raise ValueError(f"conv mode {mode!r}: 'winograd', 'winograd4', 'direct' or 'bf16x9'")
    return mode


CONV_MODE = _norm_conv_mode(os.environ.get("EAVSR_CONV_MODE", "winograd4"))
# 3x3 64 -> cout launches of at most X6S_MAX_TILES 8 x 32-pixel tiles (where the fp32-MFMA small kernel's time is one workgroup's
# chain of matrix instructions): "x6s" = csrc/conv3_x6s.hip (exact bf16x6), "direct" = the fp32 MFMA kernels (A/B switch)
CONV3_SMALL = os.environ.get("EAVSR_CONV3_SMALL", "x6s")
X6S_MAX_TILES = int(os.environ.get("EAVSR_X6S_MAX_TILES", "256"))
WINO_MIN_TILES = int(os.environ.get("EAVSR_WINO_MIN_TILES", "192"))   # 8 x 32-px tiles per launch below which the direct kernel runs


def set_conv_mode(mode: str) -> None:
    global CONV_MODE
    mode = _norm_conv_mode(mode)
    if mode in ("winograd", "bf16x9"):      # F(2x2,3x3) and the nine-product direct kernel: retired schedules
        require_lab(f"conv mode {mode!r}")
    CONV_MODE = mode


@contextlib.contextmanager
def modes(conv: Optional[str] = None, dcn: Optional[str] = None, dcn_il_impl: Optional[str] = None):
    """Scoped kernel selection: `with ops.modes(conv="direct", dcn="native"): ...` switches the process-wide defaults for the
    body and restores them on exit (also on an exception), so that a caller -- a test, an A/B measurement -- never leaves another
    mode behind.  The switches select between implementations of the same arithmetic; they are process-wide (one forward runs one
    kernel set), not per call."""
    prev = (CONV_MODE, DCN_MODE, DCN_IL_IMPL)
    try:
        if conv is not None:
            set_conv_mode(conv)
        if dcn is not None:
            set_dcn_mode(dcn)
        if dcn_il_impl is not None:
            set_dcn_il_impl(dcn_il_impl)
        yield
    finally:
        set_conv_mode(prev[0])
        set_dcn_mode(prev[1])
        set_dcn_il_impl(prev[2])


def _packed_wino(weights: Sequence[Tensor], four: bool = False, kind: Optional[str] = None) -> Tensor:
    """G g G^T of a conv weight (or of several stacked along cout); kind "f2" = F(2x2, 3x3), "f4" = F(4x4, 3x3),
    "f5" = F(2x2, 5x5)"""
    kind = kind or ("f4" if four else "f2")
    if kind == "f2":
        require_lab("Winograd F(2x2,3x3)")
    return _packed("wino_" + kind, weights, kind)


# ------------------------------------------------------------------------------------------
# predictor pieces
# ------------------------------------------------------------------------------------------
def adapt_frontend(x: Tensor, h_hr: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """`out`: an existing contiguous fp32 tensor of x's shape to write into (rows of a frame-major stack) instead of a new one"""
    x, h_hr = _chk(x, "x"), _chk(h_hr, "h_hr")
    if x.shape != h_hr.shape:
        raise ValueError("x and h_hr must have the same shape")
    n, c, h, w = x.shape
    if tuple(w1.shape) != (2 * c, 1, 3, 3) or tuple(w2.shape) != (c, 2, 3, 3):
        raise ValueError("adapt_frontend weight shapes")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("adapt_frontend: `out` must be a contiguous fp32 GPU tensor of x's shape")
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    st = _stream(x)
    _launch("adapt_frontend", 2.0 * 27 * c * n * h * w, 4.0 * 3 * c * n * h * w, x,
            lambda: lib().eavsr_adapt_frontend_f32(_p(x), _p(h_hr), _p(w1), _p(b1), _p(w2), _p(b2), _p(out),
                                                   n, c, h, w, st), "adapt_frontend")
    return out


def flow_level(x: Tensor, h_hr: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, head_ws: Sequence[Tensor],
               head_bs: Sequence[Tensor], wt: Tensor, bt: Tensor) -> Tensor:
    """TransOffsetworelu(AdaptBlock2_3x3(x, h_hr)) as one kernel (networks.py:334-348 + 566-571): (n,c,h,w) x 2 -> (n,2,h,w).
    head_ws / head_bs: [transform_matrix_conv, translation_conv] parameters (4 + 2 output channels)."""
    require_lab("ops.flow_level (one kernel per pyramid level)")
    x, h_hr = _chk(x, "x"), _chk(h_hr, "h_hr")
    if x.shape != h_hr.shape:
        raise ValueError("x and h_hr must have the same shape")
    n, c, h, w = x.shape
    wh, bh = _cat_weights(list(head_ws)), _bias_of(list(head_bs))
    if tuple(w1.shape) != (2 * c, 1, 3, 3) or tuple(w2.shape) != (c, 2, 3, 3) or tuple(wh.shape) != (6, c, 3, 3) or \
            tuple(wt.shape) != (2, 18, 3, 3) or bh is None:
        raise ValueError("flow_level: parameter shapes")
    w1, b1, w2, b2, wt, bt = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2, wt, bt))
    out = torch.empty((n, 2, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch("flow_level", 2.0 * px * (27 * c + 54 * c + 324), 4.0 * px * (2 * c + 2), x,
            lambda: lib().eavsr_flow_level_f32(_p(x), _p(h_hr), _p(w1), _p(b1), _p(w2), _p(b2), _p(wh), _p(bh), _p(wt), _p(bt),
                                               _p(out), n, c, h, w, st), "flow_level")
    return out


def affine_offsets(heads: Tensor, D: int, with_mask: bool) -> Tuple[Tensor, Optional[Tensor]]:
    heads = _chk(heads, "heads")
    n, hc, h, w = heads.shape
    if hc != (15 * D if with_mask else 6 * D):
        raise ValueError(f"heads has {hc} channels, expected {15 * D if with_mask else 6 * D}")
    off = torch.empty((n, 18 * D, h, w), device=heads.device, dtype=torch.float32)
    mask = torch.empty((n, 9 * D, h, w), device=heads.device, dtype=torch.float32) if with_mask else None
    st = _stream(heads)
    _launch("affine_offsets", 60.0 * D * n * h * w, 4.0 * n * h * w * (hc + 18 * D + (9 * D if with_mask else 0)), heads,
            lambda: lib().eavsr_affine_offsets_f32(_p(heads), _p(off), _p(mask), n, D, h, w, st), "affine_offsets")
    return off, mask


# ------------------------------------------------------------------------------------------
# resampling glue
# ------------------------------------------------------------------------------------------
def resize_bilinear_ac(x: Tensor, size: Tuple[int, int], scale: float = 1.0, pre_add: Optional[Tensor] = None,
                       post_add: Optional[Tensor] = None) -> Tensor:
    """scale * F.interpolate(x [+ pre_add], size, bilinear, align_corners=True) [+ post_add]"""
    x = _chk(x, "x")
    n, c, hin, win = x.shape
    hout, wout = int(size[0]), int(size[1])
    if pre_add is not None:
        pre_add = _chk(pre_add, "pre_add")
        if pre_add.shape != x.shape:
            raise ValueError("pre_add shape")
    out = torch.empty((n, c, hout, wout), device=x.device, dtype=torch.float32)
    if post_add is not None:
        post_add = _chk(post_add, "post_add")
        if post_add.shape != out.shape:
            raise ValueError("post_add shape")
    st = _stream(x)
    _launch("resize_bilinear_ac", 0.0, 4.0 * n * c * (hin * win + hout * wout), x,
            lambda: lib().eavsr_resize_bilinear_ac_f32(_p(x), _p(pre_add), _p(post_add), _p(out), n, c, hin, win, hout,
                                                       wout, float(scale), st), "resize_bilinear_ac")
    return out


def pyramid(x: Tensor) -> Tuple[Tensor, Tensor]:
    """(down2, down4) of eavsrp_model.py:218-220"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    if h % 4 or w % 4:
        raise ValueError(f"h={h}, w={w} must be divisible by 4 (eavsrp_model.py:223-224)")
    d2 = torch.empty((n, c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    d4 = torch.empty((n, c, h // 4, w // 4), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("pyramid", 0.0, 4.0 * n * c * h * w * (1 + 0.25 + 0.0625), x,
            lambda: lib().eavsr_pyramid_f32(_p(x), _p(d2), _p(d4), n * c, h, w, st), "pyramid")
    return d2, d4


def add(a: Tensor, b: Tensor, c: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """a + b (+ c); `out`: an existing contiguous fp32 tensor of the same shape to write into (e.g. one frame's slice of a
    frame-major buffer) instead of a new one"""
    a, b = _chk(a, "a"), _chk(b, "b")
    if a.shape != b.shape or (c is not None and c.shape != a.shape):
        raise ValueError("add: shape mismatch")
    if c is not None:
        c = _chk(c, "c")
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("add: `out` must be a contiguous fp32 GPU tensor of the operands' shape")
    st = _stream(a)
    _launch("add", float(a.numel()), 4.0 * a.numel() * (3 if c is None else 4), a,
            lambda: lib().eavsr_add_f32(_p(a), _p(b), _p(c), _p(out), a.numel(), st), "add")
    return out


def normalize(x: Tensor, mean: Tensor, std: Tensor) -> Tensor:
    """(x - mean) / std per channel (models/eavsrp_model.py:436-437, networks.py:550); mean / std: c floats on the device"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    mean, std = _chk(mean.reshape(-1), "mean"), _chk(std.reshape(-1), "std")
    if mean.numel() != c or std.numel() != c:
        raise ValueError("normalize: one mean / std per channel")
    out = torch.empty_like(x)
    st = _stream(x)
    _launch("normalize", 2.0 * x.numel(), 8.0 * x.numel(), x,
            lambda: lib().eavsr_normalize_f32(_p(x), _p(mean), _p(std), _p(out), n, c, h * w, st), "normalize")
    return out


def avg_pool2(x: Tensor) -> Tensor:
    """F.avg_pool2d(x, 2, 2, count_include_pad=False) for even h, w (models/eavsrp_model.py:450-462)"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    if h % 2 or w % 2:
        raise ValueError(f"avg_pool2: h={h}, w={w} must be even")
    out = torch.empty((n, c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("avg_pool2", 4.0 * out.numel(), 4.0 * (x.numel() + out.numel()), x,
            lambda: lib().eavsr_avg_pool2_f32(_p(x), _p(out), n * c, h, w, st), "avg_pool2")
    return out


def resize_bilinear(x: Tensor, size: Tuple[int, int], channel_mul: Optional[Tuple[float, float]] = None,
                    out: Optional[Tensor] = None) -> Tensor:
    """F.interpolate(x, size, mode='bilinear', align_corners=False); `channel_mul` = (m0, m1) multiplies channels 0 / 1 of the
    result (the flow rescaling of models/eavsrp_model.py:519-521); `out`: an existing contiguous fp32 tensor of the result's
    shape to write into (e.g. one half of a stacked batch) instead of a new one"""
    x = _chk(x, "x")
    n, c, hin, win = x.shape
    hout, wout = int(size[0]), int(size[1])
    if out is None:
        out = torch.empty((n, c, hout, wout), device=x.device, dtype=torch.float32)
    elif tuple(out.shape) != (n, c, hout, wout) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("resize_bilinear: `out` must be a contiguous fp32 GPU tensor of the result's shape")
    m0, m1 = (1.0, 1.0) if channel_mul is None else (float(channel_mul[0]), float(channel_mul[1]))
    st = _stream(x)
    _launch("resize_bilinear", 8.0 * out.numel(), 4.0 * (x.numel() + out.numel()), x,
            lambda: lib().eavsr_resize_bilinear_f32(_p(x), _p(out), n, c, hin, win, hout, wout, 0 if channel_mul is None else c,
                                                    m0, m1, st), "resize_bilinear")
    return out


def concat3(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    """torch.cat([a, b, c], 1) (models/eavsrp_model.py:486)"""
    a, b, c = _chk(a, "a"), _chk(b, "b"), _chk(c, "c")
    n, ca, h, w = a.shape
    if b.shape[0] != n or c.shape[0] != n or b.shape[2:] != a.shape[2:] or c.shape[2:] != a.shape[2:]:
        raise ValueError("concat3: shape mismatch")
    cb, cc = b.shape[1], c.shape[1]
    out = torch.empty((n, ca + cb + cc, h, w), device=a.device, dtype=torch.float32)
    st = _stream(a)
    _launch("concat3", 0.0, 8.0 * out.numel(), a,
            lambda: lib().eavsr_concat3_f32(_p(a), ca, _p(b), cb, _p(c), cc, _p(out), n, h * w, st), "concat3")
    return out


# ------------------------------------------------------------------------------------------
# per-frame PSNR / SSIM and the 8-bit frame  (psnr_total.py:39-44, test_basic.py:85-92)
# ------------------------------------------------------------------------------------------
def frame_metrics(sr: Tensor, hr: Tensor, scale: float = 255.0, rgb8: bool = False):
    """sr, hr (F, C, H, W), C 1 or 3, H, W >= 11 -> (sse int64 (F,), ssim float64 (F,), rgb8 uint8 (F, H, W, C) or None), all on
    the device, of the frames quantised as `get_current_visuals` quantises them (rint(clamp(v * scale, 0, 255)); scale = 1 for
    tensors that already are visuals): sse the exact sum of squared differences per frame, ssim the mean SSIM of psnr_total.py:41
    (11-tap gaussian window, fp64), rgb8 the quantised `sr` as interleaved bytes.  One fused launch and a fixed-order sum: two
    calls on the same input agree bit for bit."""
    sr, hr = _chk(sr, "sr"), _chk(hr, "hr")
    if sr.dim() != 4 or sr.shape != hr.shape:
        raise ValueError(f"frame_metrics: (F, C, H, W) tensors of one shape, got {tuple(sr.shape)} / {tuple(hr.shape)}")
    f, c, h, w = (int(v) for v in sr.shape)
    parts = lib().eavsr_frame_metrics_partials(f, c, h, w)
    if parts < 0:
        N.check(parts, "frame_metrics")
    ws = torch.empty((max(f * parts, 1), 2), device=sr.device, dtype=torch.int64)      # 16 bytes per workgroup partial
    sse = torch.empty(f, device=sr.device, dtype=torch.int64)
    ssim_sum = torch.empty(f, device=sr.device, dtype=torch.float64)
    img = torch.empty((f, h, w, c), device=sr.device, dtype=torch.uint8) if rgb8 else None
    st = _stream(sr)
    _launch("frame_metrics", 2.0 * 110.0 * sr.numel(), 8.0 * sr.numel() + (sr.numel() if rgb8 else 0), sr,
            lambda: lib().eavsr_frame_metrics_f32(_p(sr), _p(hr), float(scale), f, c, h, w, _p(ws), _p(sse), _p(ssim_sum), _p(img),
                                                  st), "frame_metrics")
    return sse, ssim_sum / float(c * (h - 10) * (w - 10)), img


def temporal_metrics(seq: Tensor, fw: Tensor, bw: Tensor, scale: float = 255.0, flow_b: Optional[Tensor] = None):
    """Warping error and tOF of every pair of consecutive frames (csrc/temporal.hip): seq (F, C, H, W), C 1 or 3, F >= 2;
    fw, bw (F - 1, 2, H, W) the flows t -> t + 1 and t + 1 -> t in pixels (channel 0 = x); flow_b (optional, fw's shape) the flow
    `fw` is compared with -> (err float64 (F - 1,), count int64 (F - 1,), epe float64 (F - 1,) or None), all on the device: per
    pair the squared difference, summed over the `count` pixels that pass the occlusion / motion-boundary / in-frame test and the C
    planes, between frame t and frame t + 1 warped back along fw, both quantised as `frame_metrics` quantises; and the endpoint
    distance |flow_b - fw| summed over every pixel.  E_warp = err / (C count) / 255^2, tOF = epe / (H W) (`harness.temporal_metrics`).
    Non-contiguous inputs are copied.  One fused launch and a fixed-order sum: two calls on the same input agree bit for bit."""
    seq, fw, bw = _chk(seq, "seq"), _chk(fw, "fw"), _chk(bw, "bw")
    if flow_b is not None:
        flow_b = _chk(flow_b, "flow_b")
    if seq.dim() != 4:
        raise ValueError(f"temporal_metrics: seq is an (F, C, H, W) tensor, got {tuple(seq.shape)}")
    f, c, h, w = (int(v) for v in seq.shape)
    for name, flow in (("fw", fw), ("bw", bw), ("flow_b", flow_b)):
        if flow is not None and tuple(flow.shape) != (f - 1, 2, h, w):
            raise ValueError(f"temporal_metrics: {name} is {tuple(flow.shape)}, the {f} frames of {h} x {w} need {(f - 1, 2, h, w)}")
        if flow is not None and flow.device != seq.device:
            raise ValueError(f"temporal_metrics: {name} is on {flow.device}, seq on {seq.device}")
    parts = lib().eavsr_temporal_metrics_partials(f, c, h, w)
    if parts < 0:
        N.check(parts, "temporal_metrics")
    ws = torch.empty(((f - 1) * parts, 3), device=seq.device, dtype=torch.int64)      # 24 bytes per workgroup record
    err = torch.empty(f - 1, device=seq.device, dtype=torch.float64)
    count = torch.empty(f - 1, device=seq.device, dtype=torch.int64)
    epe = torch.empty(f - 1, device=seq.device, dtype=torch.float64) if flow_b is not None else None
    st = _stream(seq)
    px = float(f - 1) * h * w
    _launch("temporal_metrics", px * (60.0 + 30.0 * c), 4.0 * px * (4 + 2 * c + (2 if flow_b is not None else 0)), seq,
            lambda: lib().eavsr_temporal_metrics_f32(_p(seq), _p(fw), _p(bw), _p(flow_b), float(scale), f, c, h, w, _p(ws), _p(err),
                                                     _p(count), _p(epe), st), "temporal_metrics")
    return err, count, epe


# ------------------------------------------------------------------------------------------
# NIQE, the report's no-reference column: block moments and the antialiased half-size resize  (csrc/niqe.hip)
# ------------------------------------------------------------------------------------------
NIQE_HALF_TILE = 32      # output columns per workgroup of eavsr_niqe_half_f64: one col_lo entry each


def niqe_moments(src: Tensor, scale: float = 255.0, block: int = 96, crop: Optional[Tuple[int, int, int, int]] = None):
    """The 25 moments of every `block` x `block` block of a luma plane, one launch over all frames of the call.
    src: the (N, C, H, W) fp32 frames, C 1 or 3 -- quantised as `frame_metrics` quantises (rint(clamp(v * scale, 0, 255))) and, for
    C = 3, turned into the integer BT.601 studio-range luma inside the kernel -- or an (N, 1, h, w) fp64 plane, read as it is (`scale`
    is not used).  crop = (y0, x0, h, w): the plane is src[:, :, y0:y0 + h, x0:x0 + w], h and w multiples of `block` (default: the
    largest such window from the top left).  Per block the map M = (I - mu) / (sigma + 1) of the 7-tap gaussian window
    (`niqe.gaussian_window`; the edge of the CROPPED plane replicated) and, for M and its products with `np.roll(M, s)`, s = (0, 1),
    (1, 0), (1, 1), (1, -1), the five numbers (n_neg, n_pos, sum v^2 over v < 0, sum v^2 over v > 0, sum |v|).
    -> (moments fp64 (N, h / block, w / block, 25), luma fp64 (N, 1, h, w) for fp32 frames -- the cropped plane `niqe_half` reads --
    or None for an fp64 plane), on the device.  A non-contiguous source is copied.  Fixed-order sums, no atomics: two calls on the
    same input agree bit for bit, and a frame's numbers do not depend on the frames that share the call."""
    from .niqe import gaussian_window
    if not isinstance(src, torch.Tensor):
        raise TypeError(f"niqe_moments: expected a tensor, got {type(src)}")
    if not src.is_cuda:
        raise RuntimeError(f"niqe_moments: tensor is on {src.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if src.dtype not in (torch.float32, torch.float64) or src.dim() != 4:
        raise ValueError(f"niqe_moments: (N, C, H, W) fp32 frames or an (N, 1, h, w) fp64 plane, got {src.dtype} {tuple(src.shape)}")
    f64 = src.dtype == torch.float64
    n, c, H, W = (int(v) for v in src.shape)
    if n < 1 or (c != 1 if f64 else c not in (1, 3)):
        raise ValueError(f"niqe_moments: {tuple(src.shape)} {src.dtype}: N >= 1 and C = 1 or 3 (an fp64 plane: C = 1)")
    if isinstance(block, bool) or not isinstance(block, int) or not 8 <= block <= 96:
        raise ValueError(f"niqe_moments: block {block!r}: an int in 8..96")
    if crop is None:
        crop = (0, 0, H // block * block, W // block * block)
    y0, x0, h, w = (int(v) for v in crop)
    if min(y0, x0) < 0 or h < block or w < block or h % block or w % block or y0 + h > H or x0 + w > W:
        raise ValueError(f"niqe_moments: crop {crop}: whole blocks of {block} (at least one) inside the {H} x {W} frame")
    src = src if src.is_contiguous() else src.contiguous()
    bh, bw = h // block, w // block
    out = torch.empty((n, bh, bw, 25), device=src.device, dtype=torch.float64)
    luma = None if f64 else torch.empty((n, 1, h, w), device=src.device, dtype=torch.float64)
    window = (C.c_double * 7)(*gaussian_window()[0].tolist())
    st = _stream(src)
    px = float(n) * h * w
    _launch("niqe_moments", px * 90.0, px * ((8.0 if f64 else 4.0 * c + 8.0)) + 200.0 * n * bh * bw, src,
            lambda: lib().eavsr_niqe_moments(_p(src), int(f64), float(scale), n, c, H, W, y0, x0, block, bh, bw, window, _p(luma), _p(out),
                                             st), "niqe_moments")
    return out, luma


class NiqeHalfTables(NamedTuple):
    """The tables of `niqe_half` on the device (`niqe_half_tables`)"""
    row_idx: Tensor
    row_w: Tensor
    col_idx: Tensor
    col_w: Tensor
    col_lo: Tensor
    span: int


def niqe_half_tables(rows, cols, device) -> NiqeHalfTables:
    """Host tables (`niqe.resize_tables`: (idx int32 (out, taps), weight fp64 (out, taps)) per axis) -> their device copies, with
    the first input column and the widest span of every run of NIQE_HALF_TILE output columns (what a workgroup stages)."""
    import numpy as np
    bundle = []
    for name, (idx, wgt) in (("rows", rows), ("cols", cols)):
        idx, wgt = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(wgt, np.float64)
        if idx.ndim != 2 or idx.shape != wgt.shape or idx.shape[0] < 1 or not 1 <= idx.shape[1] <= 64:
            raise ValueError(f"niqe_half: {name}: (idx, weight) of one (out, taps) shape with 1..64 taps, got {idx.shape} / {wgt.shape}")
        bundle.append((idx, wgt))
    cidx = bundle[1][0]
    runs = [cidx[a:a + NIQE_HALF_TILE] for a in range(0, cidx.shape[0], NIQE_HALF_TILE)]
    lo = np.array([int(r.min()) for r in runs], np.int32)
    span = max(int(r.max()) - int(r.min()) + 1 for r in runs)
    dev = lambda a: torch.from_numpy(a).to(device)
    return NiqeHalfTables(dev(bundle[0][0]), dev(bundle[0][1]), dev(bundle[1][0]), dev(bundle[1][1]), dev(lo), span)


def niqe_half(y: Tensor, tables) -> Tensor:
    """The antialiased resize between the two scales of NIQE: y (N, 1, H, W) fp64 on the device, `tables` =
    (rows, cols) from `niqe.resize_tables(H)` / `(W)` (or their device copies, `niqe_half_tables`) -> (N, 1, h, w) fp64.  Rows
    (along H) first, then columns, each an fp64 accumulation in tap order; nothing is rounded or clamped between the two."""
    if not isinstance(y, torch.Tensor) or not y.is_cuda:
        raise RuntimeError("niqe_half: an fp64 tensor on the GPU (eavsr_amd has no CPU path)")
    if y.dtype != torch.float64 or y.dim() != 4 or int(y.shape[1]) != 1 or int(y.shape[0]) < 1:
        raise ValueError(f"niqe_half: an (N, 1, H, W) fp64 plane, got {y.dtype} {tuple(y.shape)}")
    if not isinstance(tables, NiqeHalfTables):
        tables = niqe_half_tables(tables[0], tables[1], y.device)
    y = y if y.is_contiguous() else y.contiguous()
    n, _, H, W = (int(v) for v in y.shape)
    h, kr = (int(v) for v in tables.row_idx.shape)
    w, kc = (int(v) for v in tables.col_idx.shape)
    if tables.row_idx.device != y.device:
        raise ValueError(f"niqe_half: tables on {tables.row_idx.device}, the plane on {y.device}")
    if int(tables.col_lo.numel()) != -(-w // NIQE_HALF_TILE):
        raise ValueError(f"niqe_half: {int(tables.col_lo.numel())} col_lo entries for {w} output columns")
    out = torch.empty((n, 1, h, w), device=y.device, dtype=torch.float64)
    st = _stream(y)
    _launch("niqe_half", 2.0 * n * (h * W * kr + h * w * kc), 8.0 * n * (H * W + h * w), y,
            lambda: lib().eavsr_niqe_half_f64(_p(y), _p(out), _p(tables.row_idx), _p(tables.row_w), kr, _p(tables.col_idx), _p(tables.col_w),
                                              kc, _p(tables.col_lo), int(tables.span), n, H, W, h, w, st), "niqe_half")
    return out


def rgb8(sr: Tensor, scale: float = 255.0) -> Tensor:
    """sr (F, C, H, W), C 1 or 3 -> uint8 (F, H, W, C): rint(clamp(v * scale, 0, 255)) interleaved, the bytes of the frame's PNG
    scanlines (test_basic.py:85-92), without the metrics"""
    sr = _chk(sr, "sr")
    if sr.dim() != 4:
        raise ValueError(f"rgb8: an (F, C, H, W) tensor, got {tuple(sr.shape)}")
    f, c, h, w = (int(v) for v in sr.shape)
    img = torch.empty((f, h, w, c), device=sr.device, dtype=torch.uint8)
    st = _stream(sr)
    _launch("rgb8", 0.0, 5.0 * sr.numel(), sr, lambda: lib().eavsr_rgb8_f32(_p(sr), float(scale), f, c, h, w, _p(img), st), "rgb8")
    return img


def u8_to_f32(frames: Tensor, hwc: Optional[bool] = None) -> Tensor:
    """uint8 frames (F, C, h, w) planes or (F, h, w, 3) interleaved -> fp32 (F, C, h, w), every sample float(v) / 255.0f as an IEEE
    division: the reference's `np.float32(img) / 255` on the device (csrc/ingest.hip).  `hwc` names the layout; by default a tensor
    whose last dimension is 3 and whose second is not is interleaved.  Any base alignment (a slice of a byte tensor) is taken."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"u8_to_f32: expected a tensor, got {type(frames)}")
    if not frames.is_cuda:
        raise RuntimeError(f"u8_to_f32: tensor is on {frames.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"u8_to_f32: a uint8 (F, C, h, w) or (F, h, w, 3) tensor, got {frames.dtype} {tuple(frames.shape)}")
    if hwc is None:
        hwc = frames.shape[3] == 3 and frames.shape[1] != 3
    if hwc and frames.shape[3] != 3:
        raise ValueError(f"u8_to_f32: an interleaved source is (F, h, w, 3), got {tuple(frames.shape)}")
    x = frames if frames.is_contiguous() else frames.contiguous()
    if hwc:
        f, h, w, c = (int(v) for v in x.shape)
    else:
        f, c, h, w = (int(v) for v in x.shape)
    out = torch.empty((f, c, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("u8_to_f32", 0.0, 5.0 * x.numel(), x, lambda: lib().eavsr_u8_to_f32(_p(x), _p(out), f, c, h, w, 1 if hwc else 0, st), "u8_to_f32")
    return out


def _ingest_frames(who: str, frames: Tensor, window, H, W, mode: str, hwc: Optional[bool]) -> Tensor:
    """The body of `ingest_pad` (window None: the whole frame) and `ingest_window` (window = (y0, x0, wh, ww)): the checks under the
    caller's name, the allocation and the one launch of csrc/ingest_pad.hip's kernels."""
    from .segments import PAD_MODES
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"{who}: expected a tensor, got {type(frames)}")
    if not frames.is_cuda:
        raise RuntimeError(f"{who}: tensor is on {frames.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if frames.dtype not in (torch.uint8, torch.float32) or frames.dim() != 4:
        raise ValueError(f"{who}: a uint8 (F, C, h, w) / (F, h, w, 3) or fp32 (F, C, h, w) tensor, got {frames.dtype} {tuple(frames.shape)}")
    if mode not in PAD_MODES:
        raise ValueError(f"{who}: mode {mode!r}: one of {PAD_MODES}")
    u8 = frames.dtype == torch.uint8
    if hwc is None:
        hwc = u8 and frames.shape[3] == 3 and frames.shape[1] != 3
    if hwc and (not u8 or frames.shape[3] != 3):
        raise ValueError(f"{who}: an interleaved source is uint8 (F, h, w, 3), got {frames.dtype} {tuple(frames.shape)}")
    x = frames if frames.is_contiguous() else frames.contiguous()
    if hwc:
        f, h, w, c = (int(v) for v in x.shape)
    else:
        f, c, h, w = (int(v) for v in x.shape)
    if window is None:
        given, named = (H, W), f"H, W {H!r}, {W!r}"
    else:
        H, W = (window[2] if H is None else H), (window[3] if W is None else W)
        given = (*window, H, W)
        named = f"y0, x0, wh, ww, H, W {given!r}"
    if any(isinstance(v, bool) or not isinstance(v, int) for v in given):
        raise ValueError(f"{who}: {named}: integers")
    if f > 0 and (c < 1 or h < 1 or w < 1):
        raise ValueError(f"{who}: empty frames {tuple(x.shape)}")
    if window is None:
        y0, x0, wh, ww = 0, 0, h, w
        if H < h or W < w:
            raise ValueError(f"{who}: the output {H} x {W} is smaller than the frames {h} x {w} (padding only)")
    else:
        y0, x0, wh, ww = window
        if y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > max(h, 1) or x0 + ww > max(w, 1):
            raise ValueError(f"{who}: the window [{y0}, {y0 + wh}) x [{x0}, {x0 + ww}) does not lie inside frames of {h} x {w}")
        if H < wh or W < ww:
            raise ValueError(f"{who}: the output {H} x {W} is smaller than the window {wh} x {ww} (padding only)")
    if f > 65535 or c > 65535:
        raise ValueError(f"{who}: F={f}, C={c}: at most 65535 each (grid dimensions)")
    out = torch.empty((f, c, H, W), device=x.device, dtype=torch.float32)
    if f == 0:
        return out
    if out.data_ptr() % 16:
        raise ValueError(f"{who}: the output is not 16-byte aligned")
    st = _stream(x)
    kind, m = 1 if hwc else (0 if u8 else 2), PAD_MODES.index(mode)
    if window is None:
        fn = lambda: lib().eavsr_ingest_pad(_p(x), _p(out), f, c, h, w, H, W, kind, m, st)
    else:
        fn = lambda: lib().eavsr_ingest_window(_p(x), _p(out), f, c, h, w, y0, x0, wh, ww, H, W, kind, m, st)
    _launch(who, 0.0, float(f * c * wh * ww * x.element_size() + 4 * out.numel()), x, fn, who)
    return out


def ingest_pad(frames: Tensor, H: int, W: int, mode: str = "reflect", hwc: Optional[bool] = None) -> Tensor:
    """Frames of any size -> fp32 (F, C, H, W), H >= h and W >= w, padded at the bottom and right in one launch (csrc/ingest_pad.hip,
    DESIGN 7i): out[f, c, y, x] = src[f, c, ry(y), rx(x)] with `segments.pad_index` -- mode "reflect" is np.pad(mode="reflect") for
    every pad width, "edge" repeats the last row / column.  `frames`: uint8 (F, C, h, w) planes or (F, h, w, 3) interleaved (`hwc` as
    `u8_to_f32`), every sample float(v) / 255.0f as `u8_to_f32` gives it, at any base alignment; or fp32 (F, C, h, w), copied bit
    for bit.  F == 0: an empty tensor, nothing is launched.  H == h and W == w: `u8_to_f32`'s result (a copy for fp32)."""
    return _ingest_frames("ingest_pad", frames, None, H, W, mode, hwc)


def ingest_window(frames: Tensor, y0: int, x0: int, wh: int, ww: int, H: Optional[int] = None, W: Optional[int] = None,
                  mode: str = "reflect", hwc: Optional[bool] = None) -> Tensor:
    """`ingest_pad` reading the window [y0, y0 + wh) x [x0, x0 + ww) of the frames (the same kernels, csrc/ingest_pad.hip)
    -> fp32 (F, C, H, W), H >= wh and W >= ww (default: the window's size): out[f, c, y, x] = conv(src[f, c, y0 + ry(y), x0 + rx(x)])
    with `segments.pad_index` taken relative to the window (r(i) = pad_index(i, wh or ww, mode)).  `frames`, `mode`, `hwc` and conv are
    `ingest_pad`'s: uint8 planes or interleaved at any base alignment, or fp32 planes copied bit for bit.  The window is read in
    place, with the frames' own pitch: no copy of the slice is made.  F == 0: an empty tensor, nothing is launched.  The whole
    frame as the window: `ingest_pad`'s result."""
    return _ingest_frames("ingest_window", frames, (y0, x0, wh, ww), H, W, mode, hwc)


def _blend(who: str, acc: Tensor, sr: Tensor, k: int, Y0: int, X0: int, wy: Tensor, wx: Tensor) -> Tensor:
    """The body of `tile_blend` (k = 0) and `blend_dihedral` (k = 1 .. 7): the checks under the caller's name and the one launch of
    csrc/blend.hip's kernels."""
    for name, t in (("acc", acc), ("sr", sr), ("wy", wy), ("wx", wx)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name}: expected a tensor, got {type(t)}")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: {name} is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
        if t.dtype != torch.float32 or t.device != acc.device:
            raise ValueError(f"{who}: {name}: fp32 on {acc.device}, got {t.dtype} on {t.device}")
    if acc.dim() != 5 or sr.dim() != 5 or not acc.is_contiguous():
        either = "," if k == 0 else " -- (n, F, C, tw, th) for a transposed mode --"
        raise ValueError(f"{who}: acc is a contiguous (n, F, C, SH, SW) tensor and sr (n, F, C, th, tw){either} got {tuple(acc.shape)} "
                         f"(contiguous: {acc.is_contiguous()}) and {tuple(sr.shape)}")
    n, f, c, SH, SW = (int(v) for v in acc.shape)
    rows, row = int(sr.shape[3]), int(sr.shape[4])      # of the source; the tile as acc sees it is th x tw
    th, tw = (row, rows) if k & 4 else (rows, row)
    if tuple(sr.shape[:3]) != (n, f, c):
        raise ValueError(f"{who}: sr holds {tuple(sr.shape[:3])} (n, F, C) planes, acc {(n, f, c)}")
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (Y0, X0)):
        raise ValueError(f"{who}: Y0, X0 {Y0!r}, {X0!r}: integers")
    if n * f > 0 and (c < 1 or th < 1 or tw < 1):
        raise ValueError(f"{who}: an empty tile {tuple(sr.shape)}")
    if Y0 < 0 or X0 < 0 or Y0 + th > SH or X0 + tw > SW:
        raise ValueError(f"{who}: the tile [{Y0}, {Y0 + th}) x [{X0}, {X0 + tw}) does not lie inside frames of {SH} x {SW}")
    if tuple(wy.shape) != (th,) or tuple(wx.shape) != (tw,) or not wy.is_contiguous() or not wx.is_contiguous():
        raise ValueError(f"{who}: wy, wx are contiguous ({th},) and ({tw},) tensors, got {tuple(wy.shape)} and {tuple(wx.shape)}")
    sn, sf, sc, sy, sx = (int(v) for v in sr.stride())
    sn, sf, sc = (0 if d == 1 else v for d, v in zip((n, f, c), (sn, sf, sc)))      # the stride of a dimension of 1 is never used
    if (row > 1 and sx != 1) or min(sn, sf, sc, sy) < 0 or (rows > 1 and sy < row):
        raise ValueError(f"{who}: sr has unit stride along {'x' if k == 0 else 'its rows'} and non-negative strides elsewhere, "
                         f"got {tuple(sr.stride())}")
    if n * f > 65535 or c > 65535:
        raise ValueError(f"{who}: n F={n * f}, C={c}: at most 65535 each (grid dimensions)")
    if n * f == 0:
        return acc
    st = _stream(acc)
    if k == 0:
        fn = lambda: lib().eavsr_tile_blend_f32(_p(acc), _p(sr), _p(wy), _p(wx), n, f, c, SH, SW, th, tw, Y0, X0, sn, sf, sc, max(sy, row), st)
    else:
        fn = lambda: lib().eavsr_blend_dihedral_f32(_p(acc), _p(sr), _p(wy), _p(wx), n, f, c, SH, SW, th, tw, Y0, X0, k, sn, sf, sc,
                                                    max(sy, row), st)
    _launch(who, 3.0 * sr.numel(), 12.0 * sr.numel(), acc, fn, who)
    return acc


def tile_blend(acc: Tensor, sr: Tensor, Y0: int, X0: int, wy: Tensor, wx: Tensor) -> Tensor:
    """acc[n, f, c, Y0 + y, X0 + x] += (wy[y] * wx[x]) * sr[n, f, c, y, x], in place, one launch (csrc/blend.hip): three
    separately rounded fp32 operations in that order, never a fused multiply-add -- bit for bit what numpy computes.  `acc`: a
    contiguous fp32 (n, F, C, SH, SW); `sr`: fp32 (n, F, C, th, tw) with any non-negative strides on n, f, c and rows and unit stride
    along x (the transposed, cropped view `forward_long` holds is taken as it is, not copied); `wy` (th,), `wx` (tw,): contiguous fp32
    rows of `segments.tile_weights` on the device.  Plain stores: tiles that overlap are blended one after another on one stream.
    Returns `acc`."""
    return _blend("tile_blend", acc, sr, 0, Y0, X0, wy, wx)


def _dihedral_mode(who: str, k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 0 <= k <= 7:
        raise ValueError(f"{who}: mode {k!r}: an integer 0 .. 7 (bit 0 hflip, bit 1 vflip, bit 2 transpose)")
    return k


def dihedral(x: Tensor, k: int) -> Tensor:
    """g_k(x): fp32 (F, C, H, W) frames under one of the eight flips / transposes of the plane, a new contiguous tensor, one launch
    (csrc/blend.hip).  Mode k: bit 0 hflip, bit 1 vflip, bit 2 transpose, applied in that order on the last two axes
    (`dataset.py`'s augmentation flags); a transposed mode returns (F, C, W, H).  The 32 bits of every sample are copied.  F == 0:
    an empty tensor, nothing is launched."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"dihedral: expected a tensor, got {type(x)}")
    if not x.is_cuda:
        raise RuntimeError(f"dihedral: tensor is on {x.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError(f"dihedral: an fp32 (F, C, H, W) tensor, got {x.dtype} {tuple(x.shape)}")
    k = _dihedral_mode("dihedral", k)
    x = x if x.is_contiguous() else x.contiguous()
    f, c, h, w = (int(v) for v in x.shape)
    if f > 0 and (c < 1 or h < 1 or w < 1):
        raise ValueError(f"dihedral: empty frames {tuple(x.shape)}")
    if f > 65535 or c > 65535:
        raise ValueError(f"dihedral: F={f}, C={c}: at most 65535 each (grid dimensions)")
    out = torch.empty((f, c, w, h) if k & 4 else (f, c, h, w), device=x.device, dtype=torch.float32)
    if f == 0:
        return out
    st = _stream(x)
    _launch("dihedral", 0.0, 8.0 * x.numel(), x, lambda: lib().eavsr_dihedral_f32(_p(x), _p(out), f, c, h, w, k, st), "dihedral")
    return out


def blend_dihedral(acc: Tensor, sr: Tensor, k: int, Y0: int, X0: int, wy: Tensor, wx: Tensor) -> Tensor:
    """acc[n, f, c, Y0 + y, X0 + x] += (wy[y] * wx[x]) * inv_k(sr)[n, f, c, y, x], in place, one launch (csrc/blend.hip, DESIGN
    7k): `tile_blend` with the inverse of `dihedral`'s mode k on the load -- the same three separately rounded fp32 operations,
    bit for bit what numpy computes.  `acc`: a contiguous fp32 (n, F, C, SH, SW); `sr`: fp32 (n, F, C, th, tw) or, for a transposed
    mode, (n, F, C, tw, th), with any non-negative strides on n, f, c and rows and unit stride along its rows (the cropped,
    transposed view `forward_long` holds is taken as it is); `wy` (th,), `wx` (tw,): contiguous fp32 on the device.  Plain stores:
    calls that overlap are ordered on one stream.  k == 0 is `tile_blend`, the existing launch.  Returns `acc`."""
    k = _dihedral_mode("blend_dihedral", k)
    return _blend("blend_dihedral" if k else "tile_blend", acc, sr, k, Y0, X0, wy, wx)


# ------------------------------------------------------------------------------------------
# the 16-bit feature cache of the long-clip path (csrc/cache16.hip)
# ------------------------------------------------------------------------------------------
CACHE16_MAX_SEGMENTS = 16      # include/eavsr_hip.h: EAVSR_CACHE16_MAX_SEGMENTS (pointers and extents by value in the kernel arguments)
CACHE16_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
_CACHE16_CODE = {torch.float16: 0, torch.bfloat16: 1}
CACHE16_BLOCK_ITEMS = 1024     # csrc/cache16.hip: kThreads x kUnroll items (a vector of 8 elements, or one scalar element) per workgroup pass


def cache16_dtype(dtype) -> torch.dtype:
    """"fp16" | "bf16" | torch.float16 | torch.bfloat16 -> the torch dtype; anything else is refused"""
    if isinstance(dtype, str) and dtype in CACHE16_DTYPES:
        return CACHE16_DTYPES[dtype]
    if isinstance(dtype, torch.dtype) and dtype in _CACHE16_CODE:
        return dtype
    raise ValueError(f"cache16: dtype {dtype!r}: 'fp16' or 'bf16' (torch.float16 / torch.bfloat16)")


def cache16_batches(nseg: int, limit: int = CACHE16_MAX_SEGMENTS) -> List[Tuple[int, int]]:
    """the launches of a list of `nseg` segments: [(a, b)] slices of at most `limit` segments, in order; an empty list: none"""
    if nseg < 0 or limit < 1:
        raise ValueError(f"cache16_batches: {nseg} segments in launches of {limit}")
    return [(a, min(a + limit, nseg)) for a in range(0, nseg, limit)]


def cache16_cut(misalign16: int, n: int) -> Tuple[int, int, int]:
    """(head, vectors, tail) of a segment of n elements whose 16-bit side starts `misalign16` elements (0 .. 7) past a 16-byte
    boundary -- csrc/cache16.hip's cut_of: `head` scalar elements up to the next boundary (all n where the segment ends before it),
    vectors of 8 elements from there, the remaining 0 .. 7 elements scalar again"""
    if not 0 <= misalign16 <= 7 or n < 0:
        raise ValueError(f"cache16_cut: misalignment {misalign16} (0 .. 7 elements), {n} elements")
    head = min((8 - misalign16) & 7, n)
    nvec = (n - head) >> 3
    return head, nvec, n - head - 8 * nvec


def cache16_item(i: int, head: int, nvec: int, tail: int) -> Tuple[int, int]:
    """the elements [a, b) of its segment that item i of the kernels serves: the vectors first, then the head's and the tail's elements"""
    if i < nvec:
        return head + 8 * i, head + 8 * i + 8
    j = i - nvec
    if j >= head + tail:
        return 0, 0
    e = j if j < head else j + 8 * nvec
    return e, e + 1


def cache16_passes(misalign16: int, n: int) -> int:
    """workgroup passes the kernels spend on such a segment"""
    head, nvec, tail = cache16_cut(misalign16, n)
    return -(-(nvec + head + tail) // CACHE16_BLOCK_ITEMS)


def _cache16_lists(who: str, srcs, dsts, src_dtype, dst_dtype):
    srcs, dsts = list(srcs), list(dsts)
    if len(srcs) != len(dsts):
        raise ValueError(f"{who}: {len(srcs)} sources and {len(dsts)} destinations")
    device = None
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        for name, t, dt in (("source", s, src_dtype), ("destination", d, dst_dtype)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{who}: {name} {i}: expected a tensor, got {type(t)}")
            if not t.is_cuda:
                raise RuntimeError(f"{who}: {name} {i} is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
            device = t.device if device is None else device
            if t.dtype != dt or t.device != device:
                raise ValueError(f"{who}: {name} {i}: {dt} on {device}, got {t.dtype} on {t.device}")
            if not t.is_contiguous():
                raise ValueError(f"{who}: {name} {i} is not contiguous (a segment is one run of memory; it is converted in place)")
        if s.numel() != d.numel():
            raise ValueError(f"{who}: segment {i}: {s.numel()} source and {d.numel()} destination elements")
    return srcs, dsts


def _cache16_run(who: str, entry: str, srcs, dsts, code: int, extra=()):
    """`extra`: the entry point's arguments between the dtype code and the stream (the census record)"""
    st = None
    for a, b in cache16_batches(len(srcs)):
        part = [(s, d) for s, d in zip(srcs[a:b], dsts[a:b])]
        total = sum(s.numel() for s, _ in part)
        if total == 0:
            continue      # nothing but empty segments: nothing is launched
        st = _stream(part[0][0]) if st is None else st
        sl, dl = _ptr_array([s for s, _ in part]), _ptr_array([d for _, d in part])
        nl = (C.c_int64 * len(part))(*[s.numel() for s, _ in part])
        _launch(who, 0.0, 6.0 * total, part[0][0], lambda: getattr(lib(), entry)(sl, dl, nl, len(part), code, *extra, st), who)
    return dsts


def pack16(srcs: Sequence[Tensor], dsts: Sequence[Tensor], dtype) -> List[Tensor]:
    """dsts[s] = srcs[s] rounded from fp32 to `dtype` ("fp16" / "bf16" or the torch dtype), for a list of contiguous segments in one
    launch per CACHE16_MAX_SEGMENTS segments (csrc/cache16.hip).  Round to nearest even; fp16 overflows to +-inf and
    produces subnormals; NaN stays NaN, +-0 keep their sign: bit for bit `x.to(dtype)` of the CPU for every input that is not a NaN.
    srcs: fp32 tensors; dsts: tensors of `dtype` with the same numbers of elements, written in place; both contiguous, on one device,
    at any element alignment (slices are taken as they are).  A segment may be empty.  Returns `dsts`."""
    dt = cache16_dtype(dtype)
    srcs, dsts = _cache16_lists("pack16", srcs, dsts, torch.float32, dt)
    return _cache16_run("pack16", "eavsr_pack16", srcs, dsts, _CACHE16_CODE[dt])


CENSUS_SLOTS = ("max_abs", "nonfinite", "overflow", "flushed", "subnormal")      # csrc/cache16_census.h: the record's five words


def pack16_census(srcs: Sequence[Tensor], dsts: Sequence[Tensor], dtype, census: Tensor) -> List[Tensor]:
    """`pack16` -- the same lists, checks, launches and 16-bit result, bit for bit -- that also counts what the rounding did (DESIGN 7n,
    addendum).  `census`: an int64 device tensor of five elements, contiguous, on the sources' device (typically a row of a larger
    tensor), that every launch ADDS into -- the caller zeroes it -- in the order of CENSUS_SLOTS: the largest finite |x| as its fp32
    bits, the non-finite inputs, the finite inputs rounded to +-inf, the finite non-zero inputs rounded to +-0, the subnormal
    results.  `census_record` turns a row read back into numbers.  Integer max and add: two calls give identical records.  A wrong
    dtype, shape or device is refused before anything is launched.  Returns `dsts`."""
    dt = cache16_dtype(dtype)
    if not isinstance(census, torch.Tensor):
        raise TypeError(f"pack16_census: census: expected a tensor, got {type(census)}")
    if census.dtype != torch.int64 or tuple(census.shape) != (len(CENSUS_SLOTS),) or not census.is_contiguous():
        raise ValueError(f"pack16_census: census: a contiguous int64 tensor of {len(CENSUS_SLOTS)} elements, got {census.dtype} "
                         f"{tuple(census.shape)}{'' if census.is_contiguous() else ', not contiguous'}")
    srcs, dsts = _cache16_lists("pack16_census", srcs, dsts, torch.float32, dt)
    if not census.is_cuda:
        raise RuntimeError(f"pack16_census: census is on {census.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if srcs and census.device != srcs[0].device:
        raise ValueError(f"pack16_census: census on {census.device}, the segments on {srcs[0].device}")
    cp = C.c_void_p(census.data_ptr())
    return _cache16_run("pack16_census", "eavsr_pack16_census", srcs, dsts, _CACHE16_CODE[dt], (cp,))


def census_record(row, elements: int, dtype) -> Dict:
    """A census row read back from the device (five integers, `pack16_census`) as numbers -- pure host code: 'elements' (the
    caller's count of what was packed), 'dtype' ("fp16" / "bf16"), 'max_abs' as a Python float (the largest finite |x| that went in;
    0.0 where none did) and the four counts 'nonfinite', 'overflow', 'flushed', 'subnormal'"""
    import struct
    dt = cache16_dtype(dtype)
    vals = [int(v) for v in (row.tolist() if hasattr(row, "tolist") else row)]
    if len(vals) != len(CENSUS_SLOTS):
        raise ValueError(f"census_record: a row of {len(CENSUS_SLOTS)} integers, got {len(vals)}")
    if isinstance(elements, bool) or not isinstance(elements, int) or elements < 0:
        raise ValueError(f"census_record: elements {elements!r}: a non-negative integer")
    if not 0 <= vals[0] < 0x7F800000 or any(not 0 <= v <= elements for v in vals[1:]):
        raise ValueError(f"census_record: {vals} is no census of {elements} elements")
    out = {"elements": elements, "dtype": next(k for k, v in CACHE16_DTYPES.items() if v == dt),
           "max_abs": struct.unpack("<f", struct.pack("<I", vals[0]))[0]}
    out.update(zip(CENSUS_SLOTS[1:], vals[1:]))
    return out


def unpack16(srcs: Sequence[Tensor], dsts: Sequence[Tensor]) -> List[Tensor]:
    """dsts[s] = srcs[s] widened to fp32, exactly: `pack16`'s list the other way round, one launch per CACHE16_MAX_SEGMENTS segments.
    srcs: fp16 or bf16 tensors, all of one dtype; dsts: fp32, written in place.  Returns `dsts`."""
    srcs, dsts = list(srcs), list(dsts)
    if not srcs:
        if dsts:
            raise ValueError(f"unpack16: 0 sources and {len(dsts)} destinations")
        return dsts
    if not isinstance(srcs[0], torch.Tensor):
        raise TypeError(f"unpack16: source 0: expected a tensor, got {type(srcs[0])}")
    dt = cache16_dtype(srcs[0].dtype)
    srcs, dsts = _cache16_lists("unpack16", srcs, dsts, dt, torch.float32)
    return _cache16_run("unpack16", "eavsr_unpack16", srcs, dsts, _CACHE16_CODE[dt])


# ------------------------------------------------------------------------------------------
# the range census of the 16-bit backbone modes (csrc/range16.hip, DESIGN 3.6 addendum)
# ------------------------------------------------------------------------------------------
RANGE16_MAX_ROWS = 4096        # contiguous rows a non-contiguous tensor may be counted through; beyond it the call is refused
RANGE16_FLAVOURS = ("words", "as_rounded")
FORMAT_MAX = {"fp16": 65504.0, "bf16": float.fromhex("0x1.fep127")}      # the largest finite value of each format


def contiguous_runs(shape: Sequence[int], strides: Sequence[int]) -> Tuple[int, List[int]]:
    """(run, offsets): a strided tensor as rows of `run` contiguous elements that start `offsets` elements past its first -- pure
    host code.  The trailing dimensions that lie densely in memory make a row; the leading ones are walked in index order.  Sizes of
    1 are ignored; an empty tensor has no rows.  Overlapping or negative strides are the caller's to refuse."""
    dims = [(int(n), int(s)) for n, s in zip(shape, strides) if n != 1]
    if any(n == 0 for n, _ in dims):
        return 0, []
    run = 1
    while dims and dims[-1][1] == run:
        run *= dims.pop()[0]
    offsets = [0]
    for n, s in dims:
        offsets = [o + i * s for o in offsets for i in range(n)]
    return run, offsets


def _range16_segments(who: str, tensors, dtype_ok) -> Tuple[List[Tuple[int, int]], int, Optional[Tensor]]:
    """[(address, elements)] of every contiguous run of the tensors, the elements in all, and the first tensor"""
    segs, first = [], None
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: tensor {i}: expected a tensor, got {type(t)}")
        if not t.is_cuda:
            raise RuntimeError(f"{who}: tensor {i} is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
        if not dtype_ok(t.dtype):
            raise ValueError(f"{who}: tensor {i}: dtype {t.dtype}")
        first = t if first is None else first
        if t.device != first.device:
            raise ValueError(f"{who}: tensor {i} on {t.device}, tensor 0 on {first.device}")
        if any(s < 0 for s in t.stride()):
            raise ValueError(f"{who}: tensor {i} has a negative stride")
        run, offsets = contiguous_runs(t.shape, t.stride())
        if len(offsets) > RANGE16_MAX_ROWS:
            raise ValueError(f"{who}: tensor {i} ({tuple(t.shape)}, strides {tuple(t.stride())}) is {len(offsets)} contiguous rows of "
                             f"{run} elements; at most {RANGE16_MAX_ROWS} are counted row by row -- pass a contiguous tensor")
        if len(offsets) > 1 and len(set(offsets)) * run != t.numel():
            raise ValueError(f"{who}: tensor {i} overlaps itself (strides {tuple(t.stride())}): an element would be counted twice")
        es = t.element_size()
        segs += [(t.data_ptr() + o * es, run) for o in offsets]
    return segs, sum(n for _, n in segs), first


def _range16(who: str, tensors, dtype, census: Tensor, rounded: bool) -> int:
    dt = cache16_dtype(dtype)
    if not isinstance(census, torch.Tensor):
        raise TypeError(f"{who}: census: expected a tensor, got {type(census)}")
    if census.dtype != torch.int64 or tuple(census.shape) != (len(CENSUS_SLOTS),) or not census.is_contiguous():
        raise ValueError(f"{who}: census: a contiguous int64 tensor of {len(CENSUS_SLOTS)} elements, got {census.dtype} "
                         f"{tuple(census.shape)}{'' if census.is_contiguous() else ', not contiguous'}")
    if not census.is_cuda:
        raise RuntimeError(f"{who}: census is on {census.device}; eavsr_amd runs on the GPU only (no CPU path)")
    want = (lambda d: d == torch.float32) if rounded else (lambda d: d == dt)
    segs, total, first = _range16_segments(who, list(tensors), want)
    if first is not None and census.device != first.device:
        raise ValueError(f"{who}: census on {census.device}, the tensors on {first.device}")
    if total == 0:
        return 0
    cp, st, entry = C.c_void_p(census.data_ptr()), _stream(first), "eavsr_" + who
    for a, b in cache16_batches(len(segs)):
        part = [s for s in segs[a:b] if s[1]]
        if not part:
            continue
        sl = (C.c_void_p * len(part))(*[p for p, _ in part])
        nl = (C.c_int64 * len(part))(*[n for _, n in part])
        _launch(who, 0.0, (4.0 if rounded else 2.0) * sum(n for _, n in part), first,
                lambda: getattr(lib(), entry)(sl, nl, len(part), _CACHE16_CODE[dt], cp, st), who)
    return total


def range16_words(tensors: Sequence[Tensor], census: Tensor) -> int:
    """Count the 16-bit words of `tensors` -- fp16 or bf16, all of one dtype, what some kernel has stored -- into `census`
    (`pack16_census`'s record: five int64 on the tensors' device, ADDED into, slots CENSUS_SLOTS) in one launch per
    CACHE16_MAX_SEGMENTS contiguous runs (csrc/range16.hip).  An element's fp32 bits are the exact widening of its word: 'max_abs' is
    the largest finite stored value, 'nonfinite' counts inf / NaN words, 'subnormal' subnormal words; 'overflow' and 'flushed' stay 0.
    A non-contiguous tensor is counted through its contiguous rows (at most RANGE16_MAX_ROWS; more, or a tensor that overlaps
    itself, is refused).  Writes nothing but the record.  Returns the number of elements counted: the caller's to keep."""
    tensors = list(tensors)
    if not tensors:
        return 0
    if not isinstance(tensors[0], torch.Tensor):
        raise TypeError(f"range16_words: tensor 0: expected a tensor, got {type(tensors[0])}")
    return _range16("range16_words", tensors, tensors[0].dtype, census, False)


def range16_as_rounded(tensors: Sequence[Tensor], dtype, census: Tensor) -> int:
    """Count the fp32 `tensors` as a kernel that rounds them to `dtype` ("fp16" / "bf16") would leave them: `pack16_census`'s record
    of the same values -- the same rounding function -- without the store.  Lists, rows, record and return value as `range16_words`."""
    return _range16("range16_as_rounded", list(tensors), dtype, census, True)


def headroom(max_abs: float, dtype) -> float:
    """the largest finite value of the format over the largest |x| seen: 65504 / max_abs (fp16); inf where nothing but zeros was seen"""
    name = next(k for k, v in CACHE16_DTYPES.items() if v == cache16_dtype(dtype))
    if not max_abs >= 0.0:
        raise ValueError(f"headroom: max_abs {max_abs!r}")
    return float("inf") if max_abs == 0.0 else FORMAT_MAX[name] / float(max_abs)


class RangeCensus:
    """One census of a checked call: a device tensor of (CAPACITY, 5) int64 rows, zeroed once, and the host's table of sites.  A SITE is
    (scope, op, flavour, k): the k-th launch of `op` since the scope was last marked (`mark`) -- the model marks a scope at every
    time step of a branch and at every chunk of a batched stage, so the same position of every time step shares one row; the
    elements counted per row accumulate here, on the host.  `around` is `_launch`'s hook.  No synchronisation before `read`."""
    CAPACITY = 1024
    _16BIT = _re.compile(r"h16|il16")

    def __init__(self, dtype, device):
        self.dtype = next(k for k, v in CACHE16_DTYPES.items() if v == cache16_dtype(dtype))
        # (a row: the record's five words, then the tick at which it first held a non-finite or an overflowed element, 0: never)
        self.rows = torch.zeros((self.CAPACITY, len(CENSUS_SLOTS) + 1), dtype=torch.int64, device=device)
        self._tick = 0
        self.sites: List[Dict] = []
        self._index: Dict[Tuple, int] = {}
        self._scope, self._seen = "", {}

    @classmethod
    def is_16bit(cls, name: str) -> bool:
        """a launch that must say what it rounds: the kernels named after the 16-bit types"""
        return cls._16BIT.search(name) is not None

    def mark(self, scope: str) -> None:
        """the launches that follow belong to `scope`, counted from its first position again"""
        self._scope, self._seen = str(scope), {}

    def _row(self, op: str, flavour: str, elements: int) -> Tensor:
        k = self._seen.get((op, flavour), 0)
        self._seen[(op, flavour)] = k + 1
        key = (self._scope, op, flavour, k)
        i = self._index.get(key)
        if i is None:
            if len(self.sites) >= self.CAPACITY:
                raise RuntimeError(f"range census: more than {self.CAPACITY} sites in one call")
            i = self._index[key] = len(self.sites)
            self.sites.append({"site": f"{self._scope or '-'}/{op}#{k}" + (":in" if flavour == "as_rounded" else ""), "scope": self._scope,
                               "op": op, "index": k, "flavour": flavour, "elements": 0})
        self.sites[i]["elements"] += int(elements)
        return self.rows[i]

    def _count(self, count, row: Tensor) -> None:
        """one counting call into a site's row, and the stamp behind it (csrc/range16.hip: when the row first left the range)"""
        count(row[:len(CENSUS_SLOTS)])
        self._tick += 1
        rp, sp, tick, st = C.c_void_p(row.data_ptr()), C.c_void_p(row[len(CENSUS_SLOTS):].data_ptr()), self._tick, _stream(row)
        _launch("range16_stamp", 0.0, 48.0, row, lambda: lib().eavsr_range16_stamp(rp, sp, tick, st), "range16_stamp")

    def around(self, name: str, stored, rounded, launch):
        if stored is None and rounded is None:
            if self.is_16bit(name):
                raise RuntimeError(f"range census: the 16-bit launch {name!r} does not say what it rounds (ops._launch(stored=, rounded=))")
            return launch()
        if rounded is not None and len(rounded[0]):
            tensors, dtype = rounded
            if cache16_dtype(dtype) != CACHE16_DTYPES[self.dtype]:
                raise RuntimeError(f"range census of {self.dtype}: {name!r} rounds to {dtype!r}")
            self._count(lambda r: range16_as_rounded(tensors, dtype, r), self._row(name, "as_rounded", sum(int(t.numel()) for t in tensors)))
        out = launch()
        if stored:
            if any(t.dtype != CACHE16_DTYPES[self.dtype] for t in stored):
                raise RuntimeError(f"range census of {self.dtype}: {name!r} stored {[t.dtype for t in stored]}")
            self._count(lambda r: range16_words(stored, r), self._row(name, "words", sum(int(t.numel()) for t in stored)))
        return out

    def read(self) -> List[Dict]:
        """the sites in call order (of their first launch), each `census_record`'s fields beside its name and a 'headroom' -- ONE read-back (the host waits)"""
        rows = self.rows[:len(self.sites)].cpu().tolist() if self.sites else []
        out = []
        for site, row in zip(self.sites, rows):
            rec = census_record(row[:len(CENSUS_SLOTS)], site["elements"], self.dtype)
            # 'tripped_at': the count of counting launches at which the row first held inf / NaN or an overflow (0: never) -- rows are
            # shared by time steps, so call order alone does not say which site left the range first
            out.append({**site, **rec, "headroom": headroom(rec["max_abs"], self.dtype), "tripped_at": int(row[len(CENSUS_SLOTS)])})
        return out


@contextlib.contextmanager
def range_census(census: Optional[RangeCensus]):
    """`with ops.range_census(c):` -- the 16-bit launches of the body count into `c` (None: no census); the previous one is restored"""
    global RANGE16
    prev, RANGE16 = RANGE16, census
    try:
        yield census
    finally:
        RANGE16 = prev


def range_mark(scope: str) -> None:
    """name the part of the model whose launches follow (a branch's time step, a chunk of a batched stage): nothing without a census"""
    if RANGE16 is not None:
        RANGE16.mark(scope)


def frame_change(frames: Tensor, hwc: Optional[bool] = None):
    """Scene-cut statistics of uint8 frames (F, C, h, w) planes, C 1 or 3, or (F, h, w, 3) interleaved (`hwc` as `u8_to_f32`), F >= 1,
    in one launch (csrc/scene.hip) -> (hist int32 (F, 64), sad int64 (F - 1,)) on the device.  With the luma
    Y = (77 R + 150 G + 29 B + 128) >> 8 (the sample itself for C = 1): hist[f][Y >> 2] counts frame f's pixels, sad[f] is the sum
    of |Y_f - Y_{f+1}|.  Integers throughout: exact, and two calls agree bit for bit.  Any base alignment is taken."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"frame_change: expected a tensor, got {type(frames)}")
    if not frames.is_cuda:
        raise RuntimeError(f"frame_change: tensor is on {frames.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"frame_change: a uint8 (F, C, h, w) or (F, h, w, 3) tensor, got {frames.dtype} {tuple(frames.shape)}")
    if hwc is None:
        hwc = frames.shape[3] == 3 and frames.shape[1] != 3
    if hwc and frames.shape[3] != 3:
        raise ValueError(f"frame_change: an interleaved source is (F, h, w, 3), got {tuple(frames.shape)}")
    x = frames if frames.is_contiguous() else frames.contiguous()
    if hwc:
        f, h, w, c = (int(v) for v in x.shape)
    else:
        f, c, h, w = (int(v) for v in x.shape)
    if f < 1 or c not in (1, 3) or min(h, w) < 1:
        raise ValueError(f"frame_change: F >= 1 frames of 1 or 3 channels and h, w >= 1, got {tuple(frames.shape)}")
    if h * w >= 2 ** 31:
        raise ValueError(f"frame_change: frames of {h * w} pixels, fewer than 2^31 (a histogram bin is 32 bits)")
    hist = torch.zeros((f, 64), device=x.device, dtype=torch.int32)      # the kernel adds: zeroed on the launch's stream
    sad = torch.zeros((f - 1,), device=x.device, dtype=torch.int64)
    st = _stream(x)
    _launch("frame_change", 0.0, float(x.numel()), x,
            lambda: lib().eavsr_frame_change_u8(_p(x), _p(hist), _p(sad) if f > 1 else None, f, c, h, w, 1 if hwc else 0, st),
            "frame_change")
    return hist, sad


def gather_pairs(lr_store: Tensor, hr_store: Optional[Tensor], frames: Tensor, desc: Tensor, patch, scale: int, out=None,
                 may_transpose: bool = True):
    """One launch builds a batch from device-resident 8-bit frames (csrc/batch.hip): the reference's training item -- window, crop,
    hflip / vflip / transpose, `np.float32(img) / 255` (data/realvsr_dataset.py:62-94, util/util.py:223-248) -- for LR and HR together.

    lr_store (F, C, h, w) and hr_store (F, C, scale h, scale w) uint8 (hr_store None: LR only); frames (n, t) int32 indices into F;
    desc (n, 4) int32 = top, left, flags, 0 in LR pixels, flags bit 0 hflip, bit 1 vflip, bit 2 transpose; `patch` the LR patch size,
    an int or (ph, pw).  frames / desc are read on the device (the launch is graph-capturable; overwrite them in place between
    replays), so their CONTENTS are not checked here: the kernel clamps what is out of range, `dataset.check_plan` validates a plan
    on the host.  `may_transpose=False` promises that no sample carries the transpose flag and lifts the square-patch requirement
    (the kernel ignores the flag when ph != pw).  `out=(lr_out, hr_out)`: fp32 contiguous buffers of the result's shapes to write
    into (GraphedTrainStep.static_lr / static_hr); nothing is allocated then.  Returns (lr (n, t, C, ph, pw), hr (n, t, C, s ph,
    s pw) or None), every sample float(v) / 255.0f as an IEEE division."""
    for nm, v in (("lr_store", lr_store), ("frames", frames), ("desc", desc)) + ((("hr_store", hr_store),) if hr_store is not None else ()):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"gather_pairs: {nm}: expected a tensor, got {type(v)}")
        if not v.is_cuda:
            raise RuntimeError(f"gather_pairs: {nm} is on {v.device}; eavsr_amd runs on the GPU only (no CPU path)")
        if v.device != lr_store.device:
            raise ValueError(f"gather_pairs: {nm} is on {v.device}, lr_store on {lr_store.device}")
    ph, pw = (int(patch), int(patch)) if isinstance(patch, int) else (int(patch[0]), int(patch[1]))
    s = int(scale)
    if lr_store.dtype != torch.uint8 or lr_store.dim() != 4:
        raise ValueError(f"gather_pairs: lr_store: a uint8 (F, C, h, w) tensor, got {lr_store.dtype} {tuple(lr_store.shape)}")
    F_, c, h, w = (int(v) for v in lr_store.shape)
    if hr_store is not None and (hr_store.dtype != torch.uint8 or tuple(hr_store.shape) != (F_, c, s * h, s * w)):
        raise ValueError(f"gather_pairs: hr_store: uint8 {(F_, c, s * h, s * w)} (scale {s} x the LR store {tuple(lr_store.shape)}), got "
                         f"{hr_store.dtype} {tuple(hr_store.shape)}")
    if s < 1 or ph < 1 or pw < 1 or ph > h or pw > w:
        raise ValueError(f"gather_pairs: patch {ph} x {pw} (scale {s}) does not fit the {h} x {w} frames")
    if may_transpose and ph != pw:
        raise ValueError(f"gather_pairs: the transpose flag needs a square patch, got {ph} x {pw} (may_transpose=False: no sample carries it)")
    if frames.dtype != torch.int32 or frames.dim() != 2 or desc.dtype != torch.int32 or tuple(desc.shape) != (frames.shape[0], 4):
        raise ValueError(f"gather_pairs: frames int32 (n, t) and desc int32 (n, 4), got {frames.dtype} {tuple(frames.shape)} / "
                         f"{desc.dtype} {tuple(desc.shape)}")
    n, t = (int(v) for v in frames.shape)
    if t < 1 or F_ < 1:
        raise ValueError(f"gather_pairs: no frames (store of {F_}, windows of {t})")
    if not (lr_store.is_contiguous() and frames.is_contiguous() and desc.is_contiguous() and (hr_store is None or hr_store.is_contiguous())):
        raise ValueError("gather_pairs: stores and index tensors must be contiguous (nothing is copied here)")
    shapes = [(n, t, c, ph, pw), (n, t, c, s * ph, s * pw)]
    if out is not None:
        lr_out, hr_out = out
        for nm, o, shp in (("lr", lr_out, shapes[0]), ("hr", hr_out, shapes[1])):
            if o is None and nm == "hr" and hr_store is None:
                continue
            if (not isinstance(o, torch.Tensor) or o.dtype != torch.float32 or tuple(o.shape) != shp or not o.is_contiguous()
                    or o.device != lr_store.device):
                raise ValueError(f"gather_pairs: out[{nm}]: a contiguous fp32 {shp} tensor on {lr_store.device}, got "
                                 f"{getattr(o, 'dtype', type(o))} {tuple(getattr(o, 'shape', ()))}")
        if hr_store is None:
            hr_out = None
    else:
        lr_out = torch.empty(shapes[0], device=lr_store.device, dtype=torch.float32)
        hr_out = torch.empty(shapes[1], device=lr_store.device, dtype=torch.float32) if hr_store is not None else None
    st = _stream(lr_store)
    samples = lr_out.numel() + (hr_out.numel() if hr_out is not None else 0)
    _launch("gather_pairs_u8", 0.0, 5.0 * samples, lr_store,
            lambda: lib().eavsr_gather_pairs_u8(_p(lr_store), _p(hr_store) if hr_store is not None else None, _p(frames), _p(desc), _p(lr_out),
                                                _p(hr_out) if hr_out is not None else None, F_, n, t, c, h, w, s, ph, pw, st), "gather_pairs")
    return lr_out, hr_out


# the device copies of `dataset.cubic_tables(src, dst)`: {(src, dst, device): (ofs int32[dst], coef int16[dst, 4])}.  Two small
# arrays per axis length pair, a function of the sizes alone (no parameter behind them: not a WeightCache); a data set has one or
# two pairs, so the table is simply bounded.
_cubic_tables_dev: dict = {}
_CUBIC_TABLES_MAX = 64


def _cubic_tables_on(src: int, dst: int, device) -> Tuple[Tensor, Tensor]:
    key = (src, dst, str(device))
    hit = _cubic_tables_dev.get(key)
    if hit is None:
        from .dataset import cubic_tables
        ofs, coef = cubic_tables(src, dst)                  # ValueError for a ratio outside [1, 8], before anything is launched
        if len(_cubic_tables_dev) >= _CUBIC_TABLES_MAX:
            _cubic_tables_dev.clear()
        hit = _cubic_tables_dev[key] = (torch.from_numpy(ofs).to(device), torch.from_numpy(coef).to(device))
    return hit


def resize_cubic_u8(frames: Tensor, size: Tuple[int, int], out: Optional[Tensor] = None) -> Tensor:
    """uint8 planes (F, C, H, W) -> uint8 (F, C, h, w), size = (h, w): `cv2.resize(img, (w, h), interpolation=cv2.INTER_CUBIC)` of
    every plane, bit for bit as OpenCV's fixed-point path defines it (`dataset.cubic_tables`, csrc/resize_cubic.hip; DESIGN 7e also
    says where a SIMD build of OpenCV may differ by 1 on exact ties) -- how the reference's loaders make an LR frame from the
    full-size one.  Each axis shrinks by a ratio in [1, 8] (ValueError otherwise: no upscaling).  The tensor is taken as it is,
    contiguous and on the device; `out`: a contiguous uint8 (F, C, h, w) tensor on the same device to write into (returned)."""
    if not isinstance(frames, torch.Tensor):
        raise TypeError(f"resize_cubic_u8: expected a tensor, got {type(frames)}")
    if not frames.is_cuda:
        raise RuntimeError(f"resize_cubic_u8: tensor is on {frames.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if frames.dtype != torch.uint8 or frames.dim() != 4:
        raise ValueError(f"resize_cubic_u8: a uint8 (F, C, H, W) tensor, got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_contiguous():
        raise ValueError("resize_cubic_u8: frames must be contiguous (nothing is copied here)")
    f, c, H, W = (int(v) for v in frames.shape)
    h, w = (int(v) for v in size)
    if min(c, H, W) < 1:
        raise ValueError(f"resize_cubic_u8: empty planes {tuple(frames.shape)}")
    yofs, ycoef = _cubic_tables_on(H, h, frames.device)
    xofs, xcoef = _cubic_tables_on(W, w, frames.device)
    if out is None:
        out = torch.empty((f, c, h, w), device=frames.device, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (f, c, h, w) or not out.is_contiguous()
          or out.device != frames.device):
        raise ValueError(f"resize_cubic_u8: out: a contiguous uint8 {(f, c, h, w)} tensor on {frames.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    st = _stream(frames)
    _launch("resize_cubic_u8", 0.0, float(f * c) * (H * W + h * w), frames,
            lambda: lib().eavsr_resize_cubic_u8(_p(frames), _p(out), _p(xofs), _p(xcoef), _p(yofs), _p(ycoef), f, c, H, W, h, w, st),
            "resize_cubic_u8")
    return out


# ------------------------------------------------------------------------------------------
# the outgoing PNG file: scanline filters and a Huffman-only deflate coder  (csrc/png.hip)
# ------------------------------------------------------------------------------------------
class Deflated(NamedTuple):
    """F zlib streams in one buffer: frame f is data[offsets[f] : offsets[f] + sizes[f]]; offsets / sizes are int64 on the device"""
    data: Tensor
    offsets: Tensor
    sizes: Tensor


def _bytes_on_device(t, what: str, dim: int) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if t.dtype != torch.uint8 or t.dim() != dim:
        raise ValueError(f"{what}: a uint8 tensor of {dim} dimensions, got {t.dtype} {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: must be contiguous (nothing is copied here)")
    return t


def png_filter(rgb8: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """uint8 frames (F, H, W, C), C 1 or 3 -- what `rgb8` / `frame_metrics(.., rgb8=True)` leave -> the PNG scanlines (F, H, 1 + W C):
    byte 0 of a row is its filter type (0 - 4), chosen per row by the smallest sum of absolute signed filtered bytes, ties to the
    lowest number (libpng's default heuristic); neighbours outside the image are 0.  `out`: a contiguous uint8 tensor of that shape
    on the same device to write into (returned)."""
    x = _bytes_on_device(rgb8, "png_filter", 4)
    f, h, w, c = (int(v) for v in x.shape)
    if c not in (1, 3) or min(h, w) < 1:
        raise ValueError(f"png_filter: (F, H, W, C) with C 1 or 3 and H, W >= 1, got {tuple(x.shape)}")
    shape = (f, h, 1 + w * c)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError(f"png_filter: out: a contiguous uint8 {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    if f == 0:
        return out
    st = _stream(x)
    _launch("png_filter_u8", 0.0, float(x.numel() + out.numel()), x,
            lambda: lib().eavsr_png_filter_u8(_p(x), _p(out), f, h, w, c, st), "png_filter")
    return out


def deflate_huffman(data: Tensor, stripe_bytes: int, workspace: Optional[Tensor] = None) -> Deflated:
    """uint8 (F, nbytes), any bytes -> F zlib streams that inflate to them, coded on the device (csrc/png.hip): every stripe of
    `stripe_bytes` is one dynamic-Huffman block of literals only (no LZ77 matching), or stored blocks where that is not smaller.
    Returns `Deflated(data, offsets, sizes)`: the streams lie at offsets[f] = f x capacity in a buffer allocated from the shape
    alone (`eavsr_png_capacity`), sizes[f] bytes each; nothing is read back, so the call does not wait for the device.
    `workspace`: a uint8 tensor of at least `deflate_workspace_bytes(F, nbytes, stripe_bytes)` bytes to reuse between calls."""
    x = _bytes_on_device(data, "deflate_huffman", 2)
    f, nbytes = (int(v) for v in x.shape)
    stripe = int(stripe_bytes)
    cap = lib().eavsr_png_capacity(nbytes, stripe)
    need = lib().eavsr_deflate_workspace_bytes(f, nbytes, stripe)
    if cap < 0 or need < 0:
        raise ValueError(f"deflate_huffman: {lib().eavsr_last_error().decode(errors='replace')}")
    if workspace is None:
        workspace = torch.empty(need, device=x.device, dtype=torch.uint8)
    elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.numel() < need
          or not workspace.is_contiguous() or workspace.device != x.device):
        raise ValueError(f"deflate_huffman: workspace: a contiguous uint8 tensor of at least {need} bytes on {x.device}")
    out = torch.empty(f * cap, device=x.device, dtype=torch.uint8)
    offsets = torch.empty(f, device=x.device, dtype=torch.int64)
    sizes = torch.empty(f, device=x.device, dtype=torch.int64)
    if f == 0:      # nothing to launch (and an empty tensor has no address to pass)
        return Deflated(out, offsets, sizes)
    st = _stream(x)
    # bytes: the input is read twice (histogram, packing); the streams are written, then read and written again by the gather --
    # their size is data, so the profile counts the two reads alone, a lower bound
    _launch("deflate_huffman_u8", 0.0, 2.0 * x.numel(), x,
            lambda: lib().eavsr_deflate_huffman_u8(_p(x), _p(out), _p(offsets), _p(sizes), _p(workspace), f, nbytes, stripe, st),
            "deflate_huffman")
    return Deflated(out, offsets, sizes)


def deflate_workspace_bytes(frames: int, nbytes: int, stripe_bytes: int) -> int:
    need = lib().eavsr_deflate_workspace_bytes(int(frames), int(nbytes), int(stripe_bytes))
    if need < 0:
        raise ValueError(f"deflate_workspace_bytes: {lib().eavsr_last_error().decode(errors='replace')}")
    return int(need)


def png_encode(rgb8: Tensor, stripe_rows: int = 32) -> Deflated:
    """uint8 frames (F, H, W, C), C 1 or 3 -> the IDAT payload of every frame's PNG file: `png_filter`, then `deflate_huffman` with
    stripes of `stripe_rows` whole scanlines.  (`harness.encode_png_frames` wraps the payloads into files.)"""
    x = _bytes_on_device(rgb8, "png_encode", 4)
    if isinstance(stripe_rows, bool) or not isinstance(stripe_rows, int) or stripe_rows < 1:
        raise ValueError(f"png_encode: stripe_rows={stripe_rows!r}: a positive number of scanlines")
    rows = png_filter(x)
    f, h, r = (int(v) for v in rows.shape)
    return deflate_huffman(rows.view(f, h * r), min(stripe_rows, h) * r)


def png_unfilter(rows: Tensor, c: int, channels: int = 3, out: Optional[Tensor] = None) -> Tensor:
    """The scanline half of a PNG decode (csrc/png_decode.hip).  rows: uint8 (F, H, 1 + W c) on the device, the inflated
    IDAT payloads of F frames of one size (per scanline its filter-type byte 0 - 4, then W c filtered bytes); c: bytes per pixel, 1
    (grey), 3 (RGB) or 4 (RGBA).  Returns planar uint8 (F, min(c, channels), H, W): channels=3 drops the alpha of an RGBA file as
    `read_png(p)[:3]` does, channels=4 keeps it (and needs c = 4).  `out`: a contiguous uint8 tensor of that shape on the same device
    to write into (returned) -- a slice store[lo:hi] of a preallocated store, at any byte alignment.  A type byte above 4 is
    reconstructed as type 0: `harness.decode_png_frames` rejects such files before anything is launched."""
    x = _bytes_on_device(rows, "png_unfilter", 3)
    f, h, r = (int(v) for v in x.shape)
    if isinstance(c, bool) or not isinstance(c, int) or c not in (1, 3, 4):
        raise ValueError(f"png_unfilter: c={c!r}: 1 (grey), 3 (RGB) or 4 (RGBA) bytes per pixel")
    if isinstance(channels, bool) or not isinstance(channels, int) or not 1 <= channels <= 4:
        raise ValueError(f"png_unfilter: channels={channels!r}: 1 .. 4")
    if channels == 4 and c != 4:
        raise ValueError(f"png_unfilter: channels=4 needs RGBA rows (c=4), got c={c}")
    if h < 1 or r < 1 + c or (r - 1) % c:
        raise ValueError(f"png_unfilter: rows (F, H, 1 + W c) with H, W >= 1 and c={c}, got {tuple(x.shape)}")
    w, cout = (r - 1) // c, min(c, channels)
    shape = (f, cout, h, w)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.uint8)
    elif (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous()
          or out.device != x.device):
        raise ValueError(f"png_unfilter: out: a contiguous uint8 {shape} tensor on {x.device}, got "
                         f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    if f == 0:
        return out
    st = _stream(x)
    _launch("png_unfilter_u8", 0.0, float(x.numel() + out.numel()), x,
            lambda: lib().eavsr_png_unfilter_u8(_p(x), _p(out), f, h, w, c, cout, st), "png_unfilter")
    return out


# ------------------------------------------------------------------------------------------
# LPIPS (AlexNet), the report's third column  (psnr_total.py:27-35; csrc/lpips.hip)
# ------------------------------------------------------------------------------------------
def _lp(t: Tensor, name: str, dim: Optional[int] = 4) -> Tensor:
    """an fp32 contiguous GPU tensor, taken as it is: the LPIPS entry points copy nothing"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: dtype {t.dtype} unsupported (fp32 only)")
    if dim is not None and t.dim() != dim:
        raise ValueError(f"{name}: expected {dim} dimensions, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous, strides {t.stride()} for shape {tuple(t.shape)}")
    return t


def _packed_lpips_conv(weight: Tensor) -> Tensor:
    """[k^2][cin padded to 4][cout] form of a (cout, cin, k, k) weight for eavsr_lpips_conv1_f32 / eavsr_lpips_conv_f32"""
    return _packed("lpips", weight)


def lpips_conv1(sr: Tensor, hr: Tensor, weight: Tensor, bias: Tensor, shift: Tensor, scl: Tensor, scale: float = 255.0) -> Tensor:
    """sr, hr (F, 3, H, W) -> (2F, cout, (H - 7) // 4 + 1, (W - 7) // 4 + 1): relu(conv2d(front(cat(sr, hr)), weight (cout, 3, 11,
    11), bias, stride 4, padding 2)) with front(v) = ((rint(clamp(v * scale, 0, 255)) / 127.5 - 1) - shift[c]) / scl[c] applied in
    registers (the 8-bit image of `frame_metrics`, lpips' im2tensor and ScalingLayer)."""
    sr, hr = _lp(sr, "sr"), _lp(hr, "hr")
    if sr.shape != hr.shape or sr.shape[1] != 3:
        raise ValueError(f"lpips_conv1: (F, 3, H, W) tensors of one shape, got {tuple(sr.shape)} / {tuple(hr.shape)}")
    if tuple(weight.shape[1:]) != (3, 11, 11):
        raise ValueError(f"lpips_conv1: weight {tuple(weight.shape)}, expected (cout, 3, 11, 11)")
    f, _, h, w = (int(v) for v in sr.shape)
    cout = int(weight.shape[0])
    wp = _packed_lpips_conv(weight)
    b, shift, scl = _lp(bias.detach(), "bias", 1), _lp(shift.detach(), "shift", None), _lp(scl.detach(), "scale", None)
    if b.numel() != cout or shift.numel() != 3 or scl.numel() != 3:
        raise ValueError("lpips_conv1: bias (cout), shift and scale of three values each")
    ho, wo = (h - 7) // 4 + 1, (w - 7) // 4 + 1
    out = torch.empty((2 * f, cout, max(ho, 0), max(wo, 0)), device=sr.device, dtype=torch.float32)
    st = _stream(sr)
    px = 2.0 * f * max(ho, 0) * max(wo, 0)
    _launch("lpips_conv1", 2.0 * 363 * cout * px, 4.0 * (2 * sr.numel() + out.numel()), sr,
            lambda: lib().eavsr_lpips_conv1_f32(_p(sr), _p(hr), float(scale), _p(shift), _p(scl), _p(wp), _p(b), _p(out), f, h, w, cout,
                                                 st), "lpips_conv1")
    return out


def lpips_conv(x: Tensor, weight: Tensor, bias: Tensor) -> Tensor:
    """relu(F.conv2d(x, weight (cout, cin, k, k), bias, padding=k // 2)) in fp32 on the matrix pipe: AlexNet features.3 / 6 / 8 / 10"""
    x = _lp(x, "x")
    n, cin, h, w = (int(v) for v in x.shape)
    cout, k = int(weight.shape[0]), int(weight.shape[2])
    if int(weight.shape[1]) != cin:
        raise ValueError(f"lpips_conv: weight takes {int(weight.shape[1])} channels, input has {cin}")
    wp = _packed_lpips_conv(weight)
    b = _lp(bias.detach(), "bias", 1)
    if b.numel() != cout:
        raise ValueError(f"lpips_conv: bias of {b.numel()} values for {cout} channels")
    out = torch.empty((n, cout, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch("lpips_conv", 2.0 * k * k * cin * cout * px, 4.0 * px * (cin + cout), x,
            lambda: lib().eavsr_lpips_conv_f32(_p(x), _p(wp), _p(b), _p(out), n, cin, h, w, cout, k, st), "lpips_conv")
    return out


def lpips_maxpool(x: Tensor) -> Tensor:
    """F.max_pool2d(x, 3, 2) of an (n, c, h, w) tensor, h, w >= 3"""
    x = _lp(x, "x")
    n, c, h, w = (int(v) for v in x.shape)
    out = torch.empty((n, c, max((h - 3) // 2 + 1, 0), max((w - 3) // 2 + 1, 0)), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("lpips_maxpool", 0.0, 4.0 * (x.numel() + out.numel()), x,
            lambda: lib().eavsr_lpips_maxpool3s2_f32(_p(x), _p(out), n * c, h, w, st), "lpips_maxpool")
    return out


def lpips_tap(feat: Tensor, lin_weight: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """feat (2F, C, h, w): images [0:F] and [F:2F] are the two sides; lin_weight the tap's (1, C, 1, 1) weight.  Returns the float64
    (F,) means over the pixels of sum_c lin_c (f^_a - f^_b)^2, f^ = f / (sqrt(sum_c f^2) + 1e-10); with `out` (float64 (F,)) the
    means are ADDED to it.  Fixed-order sums: two calls agree bit for bit."""
    feat = _lp(feat, "feat")
    n2, c, h, w = (int(v) for v in feat.shape)
    if n2 % 2:
        raise ValueError(f"lpips_tap: an even number of images (SR then HR), got {n2}")
    f = n2 // 2
    lin = _lp(lin_weight.detach(), "lin_weight", None)
    if lin.numel() != c:
        raise ValueError(f"lpips_tap: lin weight of {lin.numel()} values for {c} channels")
    parts = lib().eavsr_lpips_tap_partials(h, w)
    if parts < 0:
        N.check(parts, "lpips_tap")
    ws = torch.empty(max(f * parts, 1), device=feat.device, dtype=torch.float64)
    accumulate = out is not None
    if out is None:
        out = torch.empty(f, device=feat.device, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (f,) or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"lpips_tap: `out` must be a contiguous float64 ({f},) device tensor")
    st = _stream(feat)
    _launch("lpips_tap", 8.0 * feat.numel(), 4.0 * feat.numel(), feat,
            lambda: lib().eavsr_lpips_tap_f32(_p(feat), _p(lin), _p(ws), _p(out), f, c, h, w, int(accumulate), st), "lpips_tap")
    return out


# ------------------------------------------------------------------------------------------
# channel attention
# ------------------------------------------------------------------------------------------
def ca_scale(partial: Tensor, hw: int, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, with_mean: bool = False):
    """partial (n, tiles, c) channel sums -> sigmoid(W2 relu(W1 mean + b1) + b2), shape (n, c); with_mean: also the means (n, c)"""
    partial = _chk(partial, "partial")
    n, tiles, c = partial.shape
    cr = int(w1.shape[0])
    scale = torch.empty((n, c), device=partial.device, dtype=torch.float32)
    mean = torch.empty((n, c), device=partial.device, dtype=torch.float32) if with_mean else None
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    st = _stream(partial)
    _launch("ca_scale", 0.0, 4.0 * partial.numel(), partial,
            lambda: lib().eavsr_ca_scale_mean_f32(_p(partial), tiles, hw, _p(w1), _p(b1), _p(w2), _p(b2), _p(scale), _p(mean), n, c,
                                                  cr, st), "ca_scale")
    return (scale, mean) if with_mean else scale


def ca_tail(r: Tensor, partial: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, x: Tensor, with_stats: bool = False):
    """the RCAB tail in one launch: r * sigmoid(W2 relu(W1 mean_hw(r) + b1) + b2) + x with mean_hw(r) from the conv's per-tile
    channel sums `partial` (n, tiles, c); falls back to ca_scale + scale_residual where the fused kernel's alignment rules fail.
    with_stats=True also returns the attention (n, c) and the channel means (n, c) (the backward of CALayer needs them):
    (out, scale, mean)."""
    r, x, partial = _chk(r, "r"), _chk(x, "x"), _chk(partial, "partial")
    n, c, h, w = r.shape
    if x.shape != r.shape or partial.shape[0] != n or partial.shape[2] != c:
        raise ValueError("ca_tail: shape mismatch")
    hw = h * w
    if hw % 4 or (r.data_ptr() | x.data_ptr()) % 16 or c > 256:
        if with_stats:
            scale, mean = ca_scale(partial, hw, w1, b1, w2, b2, with_mean=True)
            return scale_residual(r, scale, x), scale, mean
        return scale_residual(r, ca_scale(partial, hw, w1, b1, w2, b2), x)
    tiles = int(partial.shape[1])
    cr = int(w1.shape[0])
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    out = torch.empty_like(r)
    scale = torch.empty((n, c), device=r.device, dtype=torch.float32) if with_stats else None
    mean = torch.empty((n, c), device=r.device, dtype=torch.float32) if with_stats else None
    st = _stream(r)
    _launch("ca_tail", 2.0 * r.numel(), 12.0 * r.numel(), r,
            lambda: lib().eavsr_ca_tail_stats_f32(_p(r), _p(partial), tiles, _p(w1), _p(b1), _p(w2), _p(b2), _p(x), _p(out),
                                                  _p(scale), _p(mean), n, c, cr, hw, st), "ca_tail")
    return (out, scale, mean) if with_stats else out


def scale_residual(r: Tensor, scale: Tensor, x: Tensor) -> Tensor:
    """r * scale[n,c] + x"""
    r, x, scale = _chk(r, "r"), _chk(x, "x"), _chk(scale, "scale")
    n, c, h, w = r.shape
    if x.shape != r.shape or tuple(scale.shape) != (n, c):
        raise ValueError("scale_residual: shape mismatch")
    out = torch.empty_like(r)
    st = _stream(r)
    _launch("scale_residual", 2.0 * r.numel(), 12.0 * r.numel(), r,
            lambda: lib().eavsr_scale_residual_f32(_p(r), _p(scale), _p(x), _p(out), n, c, h * w, st), "scale_residual")
    return out


# ==========================================================================================
# backward kernels (training step; used by eavsr_amd/autograd.py)
# ==========================================================================================
def act_bwd(dy: Tensor, y: Tensor, act: str, slope: float = 0.0) -> Tensor:
    dy, y = _chk(dy, "dy"), _chk(y, "y")
    g = torch.empty_like(dy)
    st = _stream(dy)
    _launch("act_bwd", float(dy.numel()), 12.0 * dy.numel(), dy,
            lambda: lib().eavsr_act_bwd_f32(_p(dy), _p(y), _p(g), dy.numel(), ACT[act], float(slope), st), "act_bwd")
    return g


def plane_sum(a: Tensor, b: Optional[Tensor] = None, scale: float = 1.0) -> Tensor:
    """(n,c,h,w) -> (n,c): scale * sum_hw a (* b)"""
    a = _chk(a, "a")
    n, c, h, w = a.shape
    if b is not None:
        b = _chk(b, "b")
    out = torch.empty((n, c), device=a.device, dtype=torch.float32)
    st = _stream(a)
    _launch("plane_sum", float(a.numel()), 4.0 * a.numel() * (2 if b is not None else 1), a,
            lambda: lib().eavsr_plane_sum_f32(_p(a), _p(b), _p(out), n * c, h * w, float(scale), st), "plane_sum")
    return out


def channel_sum(a: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """(n,c,h,w) -> (c,): sum over batch and plane (bias gradient); `out` (+)= when given"""
    a = _chk(a, "a")
    n, c, h, w = a.shape
    if out is None:
        out = torch.empty((c,), device=a.device, dtype=torch.float32)
        accumulate = False
    elif tuple(out.shape) != (c,) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != a.device:
        raise ValueError("channel_sum: out must be a contiguous fp32 (c,) tensor on the input's device")
    if n == 0 or c == 0:
        return out if accumulate else out.zero_()
    st = _stream(a)
    _launch("channel_sum", float(a.numel()), 4.0 * a.numel(), a,
            lambda: lib().eavsr_channel_sum_f32(_p(a), _p(out), n, c, h * w, int(accumulate), st), "channel_sum")
    return out


def scale_residual_bwd(d: Tensor, scale: Tensor, dmean: Optional[Tensor]) -> Tensor:
    d, scale = _chk(d, "d"), _chk(scale, "scale")
    n, c, h, w = d.shape
    if dmean is not None:
        dmean = _chk(dmean, "dmean")
    dr = torch.empty_like(d)
    st = _stream(d)
    _launch("scale_residual_bwd", float(d.numel()), 8.0 * d.numel(), d,
            lambda: lib().eavsr_scale_residual_bwd_f32(_p(d), _p(scale), _p(dmean), _p(dr), n, c, h * w, st),
            "scale_residual_bwd")
    return dr


def ca_mlp_bwd(mean: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, dscale: Tensor):
    mean, dscale = _chk(mean, "mean"), _chk(dscale, "dscale")
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    n, c = mean.shape
    cr = int(w1.shape[0])
    dmean = torch.empty_like(mean)
    dw1, db1, dw2, db2 = torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)
    st = _stream(mean)
    _launch("ca_mlp_bwd", 0.0, 0.0, mean,
            lambda: lib().eavsr_ca_mlp_bwd_f32(_p(mean), _p(w1), _p(b1), _p(w2), _p(b2), _p(dscale), _p(dmean), _p(dw1),
                                               _p(db1), _p(dw2), _p(db2), n, c, cr, st), "ca_mlp_bwd")
    return dmean, dw1, db1, dw2, db2


def rcab_tail_bwd_supported(c: int, cr: int) -> bool:
    return c == 64 and cr in (1, 2, 4, 8)


def rcab_tail_bwd(d: Tensor, r: Tensor, mean: Tensor, scale: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor,
                  grads=None, accumulate: bool = False, dsum: Optional[Tensor] = None):
    """Backward of out = r * sigmoid(W2 relu(W1 mean_hw(r) + b1) + b2) + x w.r.t. r and the four MLP parameters: the plane
    sums sum_hw d r, then ONE launch (eavsr_rcab_tail_bwd_f32) for the MLP's backward, the broadcast of the mean's gradient and
    dr = d * scale + dmean / hw.  `grads` = (dw1, db1, dw2, db2) buffers to write or, with `accumulate`, to add to; fresh ones
    when None.  dsum: (n, rows, c) partial sums of d * r that the launch adds up itself (conv2d(.., dgrad=True, sum_mul=r) where d was
    produced) -- then there is no plane-sum launch.  Returns (dr, dw1, db1, dw2, db2)."""
    d, r, mean, scale = _chk(d, "d"), _chk(r, "r"), _chk(mean, "mean"), _chk(scale, "scale")
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    n, c, h, w = d.shape
    cr = int(w1.shape[0])
    if not rcab_tail_bwd_supported(c, cr):
        raise NotImplementedError(f"rcab_tail_bwd: {c} channels / {cr} hidden units")
    # `mean` (n, c), or the conv epilogue's partial channel sums (n, rows, c) that the kernel adds up itself
    if mean.dim() == 3:
        if tuple(mean.shape[::2]) != (n, c):
            raise ValueError("rcab_tail_bwd: partial sums must be (n, rows, c)")
        mean_rows = int(mean.shape[1])
    elif tuple(mean.shape) == (n, c):
        mean_rows = 0
    else:
        raise ValueError("rcab_tail_bwd: mean must be (n, c) or (n, rows, c)")
    if dsum is not None:
        dsum = _chk(dsum, "dsum")
        if dsum.dim() != 3 or tuple(dsum.shape[::2]) != (n, c):
            raise ValueError("rcab_tail_bwd: dsum must be (n, rows, c)")
        dscale, ds_rows = dsum, int(dsum.shape[1])
    else:
        dscale, ds_rows = plane_sum(d, r), 0
    if grads is None:
        grads = (torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2))
        accumulate = False
    dw1, db1, dw2, db2 = grads
    dr = torch.empty_like(d)
    st = _stream(d)
    _launch("rcab_tail_bwd", 2.0 * d.numel(), 8.0 * d.numel(), d,
            lambda: lib().eavsr_rcab_tail_bwd_f32(_p(d), _p(scale), _p(mean), _p(w1), _p(b1), _p(w2), _p(b2), _p(dscale), _p(dr),
                                                  _p(dw1), _p(db1), _p(dw2), _p(db2), n, c, cr, h * w, mean_rows, ds_rows,
                                                  int(accumulate), st),
            "rcab_tail_bwd")
    return dr, dw1, db1, dw2, db2


def flow_warp_bwd(x: Tensor, flow: Tensor, flow2: Optional[Tensor], dout: Tensor, need_dx: bool, need_dflow: bool):
    x, flow, dout = _chk(x, "x"), _chk(flow, "flow"), _chk(dout, "dout")
    n, c, h, w = x.shape
    if flow2 is not None:
        flow2 = _chk(flow2, "flow2")
    dx = torch.zeros_like(x) if need_dx else None
    dflow = torch.empty_like(flow) if need_dflow else None
    st = _stream(x)
    _launch("flow_warp_bwd", 16.0 * x.numel(), 4.0 * x.numel() * 3, x,
            lambda: lib().eavsr_flow_warp_bwd_f32(_p(x), _p(flow), _p(flow2), _p(dout), _p(dx), _p(dflow), n, c, h, w, st),
            "flow_warp_bwd")
    return dx, dflow


def resize_bilinear_ac_bwd(dout: Tensor, in_shape, scale: float) -> Tensor:
    dout = _chk(dout, "dout")
    n, c, hin, win = in_shape
    hout, wout = dout.shape[2:]
    din = torch.zeros((n, c, hin, win), device=dout.device, dtype=torch.float32)
    st = _stream(dout)
    _launch("resize_bilinear_ac_bwd", 0.0, 4.0 * (dout.numel() + din.numel()), dout,
            lambda: lib().eavsr_resize_bilinear_ac_bwd_f32(_p(dout), _p(din), n, c, hin, win, hout, wout, float(scale), st),
            "resize_bilinear_ac_bwd")
    return din


def resize_bilinear_ac_bwd_det(dout: Tensor, in_shape, scale: float) -> Tensor:
    """resize_bilinear_ac_bwd without atomics (deterministic mode): every input pixel gathers its output pixels in a fixed order"""
    dout = _chk(dout, "dout")
    n, c, hin, win = in_shape
    hout, wout = dout.shape[2:]
    din = torch.empty((n, c, hin, win), device=dout.device, dtype=torch.float32)
    st = _stream(dout)
    _launch("resize_bilinear_ac_bwd_det", 0.0, 4.0 * (dout.numel() + din.numel()), dout,
            lambda: lib().eavsr_resize_bilinear_ac_bwd_det_f32(_p(dout), _p(din), n, c, hin, win, hout, wout, float(scale), st),
            "resize_bilinear_ac_bwd_det")
    return din


def flow_warp_bwd_dx_det(flow: Tensor, flow2: Optional[Tensor], dout: Tensor) -> Tensor:
    """dx of flow_warp_bwd without atomics (deterministic mode): an inverted index per sample, one fixed-order sum per cell and channel"""
    flow, dout = _chk(flow, "flow"), _chk(dout, "dout")
    if flow2 is not None:
        flow2 = _chk(flow2, "flow2")
    n, c, h, w = dout.shape
    dx = torch.empty_like(dout)
    ws = torch.empty(int(lib().eavsr_flow_warp_bwd_dx_det_workspace_floats(n, h, w)), device=dout.device, dtype=torch.int32)
    st = _stream(dout)
    _launch("flow_warp_bwd_dx_det", 8.0 * dout.numel(), 4.0 * dout.numel() * 3, dout,
            lambda: lib().eavsr_flow_warp_bwd_dx_det_f32(_p(flow), _p(flow2), _p(dout), _p(dx), _p(ws), n, c, h, w, st),
            "flow_warp_bwd_dx_det")
    return dx


def dcnv2_col2im_dx_det(offset: Tensor, mask: Tensor, dcol: Tensor, dg: int) -> Tensor:
    """DCNv2's dx from the column gradient dcol = W^T . dY (n, 576, h, w) without atomics (deterministic mode): a gather-form col2im
    through an inverted index per (sample, deformable group); 64 channels, 8 groups"""
    offset, mask, dcol = _chk(offset, "offset"), _chk(mask, "mask"), _chk(dcol, "dcol")
    n, c9, h, w = dcol.shape
    if c9 != 576 or dg != 8 or tuple(offset.shape) != (n, 144, h, w) or tuple(mask.shape) != (n, 72, h, w):
        raise NotImplementedError("dcnv2_col2im_dx_det: 64 channels, 8 deformable groups, 3x3")
    dx = torch.empty((n, 64, h, w), device=dcol.device, dtype=torch.float32)
    ws = torch.empty(int(lib().eavsr_dcnv2_col2im_dx_det_workspace_floats(n, h, w)), device=dcol.device, dtype=torch.int32)
    st = _stream(dcol)
    _launch("dcnv2_col2im_dx_det", 2.0 * dcol.numel() * 4, 4.0 * (dcol.numel() + dx.numel()), dcol,
            lambda: lib().eavsr_dcnv2_col2im_dx_det_f32(_p(offset), _p(mask), _p(dcol), _p(dx), _p(ws), n, 64, h, w, dg, st),
            "dcnv2_col2im_dx_det")
    return dx


def pyramid_bwd(dd2: Tensor, dd4: Tensor) -> Tensor:
    dd2, dd4 = _chk(dd2, "dd2"), _chk(dd4, "dd4")
    n, c, h2, w2 = dd2.shape
    din = torch.empty((n, c, 2 * h2, 2 * w2), device=dd2.device, dtype=torch.float32)
    st = _stream(dd2)
    _launch("pyramid_bwd", 0.0, 4.0 * din.numel() * 1.3125, dd2,
            lambda: lib().eavsr_pyramid_bwd_f32(_p(dd2), _p(dd4), _p(din), n * c, 2 * h2, 2 * w2, st), "pyramid_bwd")
    return din


def affine_offsets_bwd(doff: Tensor, dmask: Optional[Tensor], mask: Optional[Tensor], D: int) -> Tensor:
    doff = _chk(doff, "doff")
    n, _, h, w = doff.shape
    with_mask = mask is not None
    if with_mask:
        mask = _chk(mask, "mask")
        dmask = _chk(dmask, "dmask") if dmask is not None else torch.zeros_like(mask)
    dheads = torch.empty((n, (15 if with_mask else 6) * D, h, w), device=doff.device, dtype=torch.float32)
    st = _stream(doff)
    _launch("affine_offsets_bwd", 0.0, 4.0 * (doff.numel() + dheads.numel()), doff,
            lambda: lib().eavsr_affine_offsets_bwd_f32(_p(doff), _p(dmask) if with_mask else None,
                                                       _p(mask) if with_mask else None, _p(dheads), n, D, h, w, st),
            "affine_offsets_bwd")
    return dheads


def conv_wgrad(dy: Tensor, srcs: Sequence[Tensor], ksize: int, out: Optional[Tensor] = None,
               accumulate: bool = False, precision: str = "fp32") -> Tensor:
    """Weight gradient (cout, cin_total, k, k) of a conv over the virtual concatenation of `srcs`; written to (or, with
    `accumulate`, added to) `out` when given.  precision="bf16": see conv_wgrad_multi."""
    if check_precision(precision) == "bf16" and wgrad_bf16_takes([dy], [srcs], ksize):
        dy_ = _chk(dy, "dy")
        cin_ = sum(int(s.shape[1]) for s in srcs)
        if out is None:
            out, accumulate = torch.empty((int(dy_.shape[1]), cin_, ksize, ksize), device=dy_.device, dtype=torch.float32), False
        return conv_wgrad_multi([dy_], [srcs], ksize, out=out, accumulate=accumulate, precision="bf16")
    dy = _chk(dy, "dy")
    srcs = [_chk(s, f"src{i}") for i, s in enumerate(srcs)]
    n, cout, h, w = dy.shape
    cin = sum(int(s.shape[1]) for s in srcs)
    if out is None:
        dw = torch.empty((cout, cin, ksize, ksize), device=dy.device, dtype=torch.float32)
        accumulate = False
    else:
        dw = out
        if (tuple(dw.shape) != (cout, cin, ksize, ksize) or not dw.is_contiguous() or dw.dtype != torch.float32
                or dw.device != dy.device):
            raise ValueError("conv_wgrad: out must be a contiguous fp32 (cout, cin, k, k) tensor on dy's device")
    acc = int(accumulate)
    blocks = lib().eavsr_conv_wgrad_blocks(n, h, w, ksize)
    if blocks <= 0:
        raise NotImplementedError(f"conv_wgrad: kernel size {ksize}")
    if n == 0:      # an empty batch has no device pointer to pass (the entry points refuse NULL): zeros, or what was there
        return dw if accumulate else dw.zero_()
    st = _stream(dy)
    if ksize == 1 and max(int(s.shape[1]) for s in srcs) > 64:
        # every 64-channel block of a source in ONE launch + one reduction (DCNv2's 576-channel column tensor: nine of each before)
        ws = torch.empty(blocks * 64 * 64 * max((int(s.shape[1]) + 63) // 64 for s in srcs), device=dy.device, dtype=torch.float32)
        base = 0
        for s in srcs:
            cs = int(s.shape[1])
            for co0 in range(0, cout, 64):
                _launch("conv_wgrad1x1", 2.0 * min(64, cout - co0) * cs * n * h * w, 4.0 * n * h * w * (64 + cs), dy,
                        lambda s=s, cs=cs, co0=co0, base=base: lib().eavsr_conv_wgrad_span_f32(
                            _p(dy), _p(s), _p(dw), _p(ws), n, h, w, cout, co0, cs, cin, base, acc, st), "conv_wgrad_span")
            base += cs
        return dw
    ws = torch.empty(blocks * 64 * 64 * ksize * ksize, device=dy.device, dtype=torch.float32)
    base = 0
    for s in srcs:
        cs = int(s.shape[1])
        for ci0 in range(0, cs, 64):
            for co0 in range(0, cout, 64):
                _launch(f"conv_wgrad{ksize}x{ksize}", 2.0 * min(64, cout - co0) * min(64, cs - ci0) * ksize * ksize * n * h * w,
                        4.0 * n * h * w * 128, dy,
                        lambda s=s, cs=cs, ci0=ci0, co0=co0, base=base: lib().eavsr_conv_wgrad_f32(
                            _p(dy), _p(s), _p(dw), _p(ws), n, h, w, cout, co0, cs, ci0, cin, base + ci0, ksize, acc, st),
                        "conv_wgrad")
        base += cs
    return dw


WGRAD_MAX_SEGMENTS = 8      # csrc/conv_wgrad.hip: WG_MAX_SEG (pointers by value in the kernel arguments)


def _ptr_array(tensors):
    import ctypes as _C
    return (_C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def wgrad_bf16_takes(dys: Sequence[Tensor], srcs_list: Sequence[Sequence[Tensor]], ksize: int) -> bool:
    """the bf16 training mode's weight gradient (eavsr_conv_wgrad_bias_multi_bf16) takes these uses: 3x3 at a size where the
    crop-sized convolution kernel runs (x6s_takes), w % 4 == 0 and 16-byte aligned tensors; anything else stays on the exact kernels"""
    n, _, h, w = dys[0].shape
    return (ksize == 3 and w % 4 == 0 and x6s_takes(int(n), int(h), int(w))
            and all(t.data_ptr() % 16 == 0 and t.is_contiguous() for t in list(dys) + [s_ for ss in srcs_list for s_ in ss]))


def conv_wgrad_multi(dys: Sequence[Tensor], srcs_list: Sequence[Sequence[Tensor]], ksize: int, out: Tensor,
                     accumulate: bool = False, bias_out: Optional[Tensor] = None, precision: str = "fp32") -> Tensor:
    """`conv_wgrad` over several USES of one weight in one launch per (source, 64-channel block): dys[s] / srcs_list[s] are
    the (dY, sources) pairs of use s, all of the same shapes (the frames of the recurrence: eavsrp_model.py:271-324).  The K
    dimension of the weight-gradient GEMM becomes pixels x uses -- a 2 x 96 x 96 training crop has 72 tiles per use for 256
    CUs -- and the per-use accumulation into `out` becomes one slab reduction.  At most WGRAD_MAX_SEGMENTS uses per call.
    bias_out (cout,): the bias gradient sum(dY) is written (or, accumulate=True, added) there as well -- by the bf16x6 3x3 kernel
    itself, which stages dY anyway, by a channel-sum launch otherwise (eavsr_conv_wgrad_bias_multi_f32).
    precision="bf16" (the bf16 training mode): where wgrad_bf16_takes holds, dY and X are rounded once to bf16
    (eavsr_conv_wgrad_bias_multi_bf16: the same slabs and fixed-order reduction); elsewhere the exact kernels as before."""
    bf16 = check_precision(precision) == "bf16" and wgrad_bf16_takes(dys, srcs_list, ksize)
    nseg = len(dys)
    if not 1 <= nseg <= WGRAD_MAX_SEGMENTS or len(srcs_list) != nseg:
        raise ValueError(f"conv_wgrad_multi: 1..{WGRAD_MAX_SEGMENTS} segments")
    dys = [_chk(d, "dy") for d in dys]
    srcs_list = [[_chk(s_, "src") for s_ in ss] for ss in srcs_list]
    n, cout, h, w = dys[0].shape
    shapes = [tuple(s_.shape) for s_ in srcs_list[0]]
    for d, ss in zip(dys, srcs_list):
        if tuple(d.shape) != (n, cout, h, w) or [tuple(s_.shape) for s_ in ss] != shapes:
            raise ValueError("conv_wgrad_multi: every segment must have the shapes of the first")
    cin = sum(sh[1] for sh in shapes)
    dw = out
    if (tuple(dw.shape) != (cout, cin, ksize, ksize) or not dw.is_contiguous() or dw.dtype != torch.float32
            or dw.device != dys[0].device):
        raise ValueError("conv_wgrad_multi: out must be a contiguous fp32 (cout, cin, k, k) tensor on dy's device")
    acc = int(accumulate)
    blocks = lib().eavsr_conv_wgrad_blocks(n * nseg, h, w, ksize)
    if blocks <= 0:
        raise NotImplementedError(f"conv_wgrad: kernel size {ksize}")
    if bias_out is not None and (tuple(bias_out.shape) != (cout,) or not bias_out.is_contiguous() or bias_out.dtype != torch.float32
                                 or bias_out.device != dw.device):
        raise ValueError("conv_wgrad_multi: bias_out must be a contiguous fp32 (cout,) tensor on dy's device")
    if n == 0:      # as conv_wgrad: no pointers to pass
        if not accumulate:
            dw.zero_()
            if bias_out is not None:
                bias_out.zero_()
        return dw
    ws = torch.empty(blocks * (64 * 64 * ksize * ksize + 64), device=dw.device, dtype=torch.float32)
    st = _stream(dw)
    dyl = _ptr_array(dys)
    base = 0
    for si, sh in enumerate(shapes):
        cs = int(sh[1])
        xl = _ptr_array([ss[si] for ss in srcs_list])
        for ci0 in range(0, cs, 64):
            for co0 in range(0, cout, 64):
                db = bias_out if (si == 0 and ci0 == 0) else None      # once per 64-channel block of outputs
                _launch(f"conv_wgrad{ksize}x{ksize}", 2.0 * min(64, cout - co0) * min(64, cs - ci0) * ksize * ksize * n * nseg * h * w,
                        4.0 * n * nseg * h * w * 128, dw,
                        lambda xl=xl, cs=cs, ci0=ci0, co0=co0, base=base, db=db: (
                            lib().eavsr_conv_wgrad_bias_multi_bf16 if bf16 else lib().eavsr_conv_wgrad_bias_multi_f32)(
                            dyl, xl, nseg, _p(dw), _p(db), _p(ws), n, h, w, cout, co0, cs, ci0, cin, base + ci0, ksize, acc, st),
                        "conv_wgrad_bf16" if bf16 else "conv_wgrad")
        base += cs
    return dw


def channel_sum_multi(tensors: Sequence[Tensor], out: Tensor, accumulate: bool = False) -> Tensor:
    """`channel_sum` over several tensors of one shape in one launch (the bias gradient of conv_wgrad_multi's segments)"""
    nseg = len(tensors)
    if not 1 <= nseg <= WGRAD_MAX_SEGMENTS:
        raise ValueError(f"channel_sum_multi: 1..{WGRAD_MAX_SEGMENTS} segments")
    tensors = [_chk(t, "a") for t in tensors]
    n, c, h, w = tensors[0].shape
    if any(tuple(t.shape) != (n, c, h, w) for t in tensors):
        raise ValueError("channel_sum_multi: every segment must have the shape of the first")
    if tuple(out.shape) != (c,) or not out.is_contiguous() or out.dtype != torch.float32 or out.device != tensors[0].device:
        raise ValueError("channel_sum: out must be a contiguous fp32 (c,) tensor on the input's device")
    if n == 0 or c == 0:
        return out if accumulate else out.zero_()
    st = _stream(out)
    al = _ptr_array(tensors)
    _launch("channel_sum", float(tensors[0].numel() * nseg), 4.0 * tensors[0].numel() * nseg, out,
            lambda: lib().eavsr_channel_sum_multi_f32(al, nseg, _p(out), n, c, h * w, int(accumulate), st), "channel_sum")
    return out


# DCNv2's backward: "sampler" = csrc/dcn_bwd.hip (one kernel, no column tensor; 64 -> 64 channels, 8 groups), "columns" = rounds 1-5
# (im2col -> column tensor -> two GEMM launches -> col2im; any configuration).  EAVSR_DCN_BWD=columns: A/B switch.
DCN_BWD = os.environ.get("EAVSR_DCN_BWD", "sampler")


def dcnv2_bwd_supported(x: Tensor, weight: Tensor, dg: int) -> bool:
    return (DCN_BWD == "sampler" and x.dim() == 4 and int(x.shape[1]) == 64 and tuple(weight.shape) == (64, 64, 3, 3) and dg == 8
            and x.numel() < 2 ** 31)


def dcnv2_bwd(x: Tensor, offset: Tensor, mask: Tensor, weight: Tensor, dy: Tensor, dg: int, need_dx: bool = True,
              dweight: Optional[Tensor] = None, accumulate: bool = False):
    """dx (NCHW or None), doffset, dmask, dweight of modulated_deform_conv2d(x, offset, mask, weight) for the upstream gradient dy, by
    eavsr_dcnv2_bwd_f32 (csrc/dcn_bwd.hip): x goes to the IL8 layout, dx comes back from it.  `dweight` (64, 64, 3, 3): written or,
    accumulate=True, added to (autograd.grad_sink); a new tensor when None."""
    x, offset, mask, dy = _chk(x, "x"), _chk(offset, "offset"), _chk(mask, "mask"), _chk(dy, "dy")
    w_ = _chk(weight.detach(), "weight")
    n, c, h, w = x.shape
    if not dcnv2_bwd_supported(x, weight, dg) or tuple(dy.shape) != (n, 64, h, w):
        raise NotImplementedError("dcnv2_bwd: 64 -> 64 channels, 8 deformable groups, 3x3 (use dcnv2_im2col / dcnv2_col2im)")
    xil = to_il8(x)
    dxil = torch.zeros_like(xil) if need_dx else None
    doff, dmask = torch.empty_like(offset), torch.empty_like(mask)
    if dweight is None:
        dweight, accumulate = torch.empty_like(w_), False
    elif tuple(dweight.shape) != (64, 64, 3, 3) or not dweight.is_contiguous() or dweight.dtype != torch.float32:
        raise ValueError("dcnv2_bwd: dweight must be a contiguous fp32 (64, 64, 3, 3) tensor")
    ws = torch.empty(int(lib().eavsr_dcnv2_bwd_workspace_floats(n, h, w)), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch("dcnv2_bwd", 2.0 * 2.0 * 64 * 576 * px, 4.0 * px * (64 * 3 + 27 * dg * 2), x,
            lambda: lib().eavsr_dcnv2_bwd_f32(_p(xil), _p(offset), _p(mask), _p(w_), _p(dy), _p(dxil), _p(doff), _p(dmask), _p(dweight),
                                              _p(ws), n, c, h, w, 64, dg, int(accumulate), st), "dcnv2_bwd")
    dx = None
    if need_dx:
        dx = torch.empty_like(x)
        _launch("il8_to_nchw", 0.0, 8.0 * x.numel(), x,
                lambda: lib().eavsr_il8_to_nchw_f32(_p(dxil), _p(dx), n, c, h, w, st), "il8_to_nchw")
    return dx, doff, dmask, dweight


def dcnv2_im2col(x: Tensor, offset: Tensor, mask: Tensor, dg: int) -> Tensor:
    x, offset, mask = _chk(x, "x"), _chk(offset, "offset"), _chk(mask, "mask")
    n, c, h, w = x.shape
    col = torch.empty((n, c * 9, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("dcnv2_im2col", 0.0, 4.0 * col.numel(), x,
            lambda: lib().eavsr_dcnv2_im2col_f32(_p(x), _p(offset), _p(mask), _p(col), n, c, h, w, dg, st), "dcnv2_im2col")
    return col


def dcnv2_col2im(x: Tensor, offset: Tensor, mask: Tensor, dcol: Tensor, dg: int, need_dx: bool = True):
    x, offset, mask, dcol = _chk(x, "x"), _chk(offset, "offset"), _chk(mask, "mask"), _chk(dcol, "dcol")
    n, c, h, w = x.shape
    dx = torch.zeros_like(x) if need_dx else None
    doff, dmask = torch.empty_like(offset), torch.empty_like(mask)
    st = _stream(x)
    _launch("dcnv2_col2im", 0.0, 4.0 * dcol.numel(), x,
            lambda: lib().eavsr_dcnv2_col2im_f32(_p(x), _p(offset), _p(mask), _p(dcol), _p(dx), _p(doff), _p(dmask), n, c,
                                                 h, w, dg, st), "dcnv2_col2im")
    return dx, doff, dmask


def gconv3x3(x: Tensor, weight: Tensor, bias: Optional[Tensor], cpg: int, act: Optional[str] = None,
             slope: float = 0.0) -> Tensor:
    x, weight = _chk(x, "x"), _chk(weight.detach(), "weight")
    n, cin, h, w = x.shape
    cout = int(weight.shape[0])
    if cin != cout * cpg or tuple(weight.shape) != (cout, cpg, 3, 3):
        raise ValueError("gconv3x3: one output channel per group, cpg input channels per group")
    b = None if bias is None else _chk(bias.detach(), "bias")
    out = torch.empty((n, cout, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    _launch("gconv3x3", 18.0 * cpg * out.numel(), 4.0 * (x.numel() + out.numel()), x,
            lambda: lib().eavsr_gconv3x3_fwd_f32(_p(x), _p(weight), _p(b), _p(out), n, cout, cpg, h, w, ACT[act],
                                                 float(slope), st), "gconv3x3_fwd")
    return out


def gconv3x3_bwd(g: Tensor, x: Tensor, weight: Tensor, cpg: int, grads=None, accumulate: bool = False):
    """grads=(dweight, dbias) buffers: written -- or, accumulate=True, added to -- in place (autograd.grad_sink)"""
    g, x, weight = _chk(g, "g"), _chk(x, "x"), _chk(weight.detach(), "weight")
    n, cout, h, w = g.shape
    dx = torch.empty_like(x)
    if grads is None:
        dw, db = torch.empty_like(weight), torch.empty(cout, device=g.device, dtype=torch.float32)
        accumulate = False
    else:
        dw, db = grads
        if (tuple(dw.shape) != tuple(weight.shape) or tuple(db.shape) != (cout,) or not dw.is_contiguous() or dw.dtype != torch.float32
                or db.dtype != torch.float32 or dw.device != g.device or db.device != g.device):
            raise ValueError("gconv3x3_bwd: grads = contiguous fp32 (dweight, dbias) of the parameters' shapes on g's device")
    st = _stream(g)
    _launch("gconv3x3_bwd", 36.0 * cpg * g.numel(), 4.0 * (2 * x.numel() + g.numel()), g,
            lambda: lib().eavsr_gconv3x3_bwd_acc_f32(_p(g), _p(x), _p(weight), _p(dx), _p(dw), _p(db), n, cout, cpg, h, w,
                                                     int(bool(accumulate)), st),
            "gconv3x3_bwd")
    return dx, dw, db


# ==========================================================================================
# 16-bit residual backbone (NHWC bf16 / fp16 activations, fp32 accumulate)
# ==========================================================================================
_H16 = {torch.float16: 1, torch.bfloat16: 2, "fp16": 1, "f16": 1, "bf16": 2}
_H16_TORCH = {1: torch.float16, 2: torch.bfloat16}


def h16_code(dtype) -> int:
    try:
        return _H16[dtype]
    except KeyError:
        raise ValueError(f"16-bit dtype expected (torch.float16 / torch.bfloat16 / 'fp16' / 'bf16'), got {dtype!r}")


def _chk_h16(t: Tensor, name: str) -> Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if t.dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError(f"{name}: dtype {t.dtype}, expected a 16-bit float")
    return t if t.is_contiguous() else t.contiguous()


def to_nhwc_h16(x: Tensor, dtype) -> Tensor:
    """fp32 NCHW (n,c,h,w) -> 16-bit NHWC (n,h,w,c)"""
    x = _chk(x, "x")
    n, c, h, w = x.shape
    code = h16_code(dtype)
    out = torch.empty((n, h, w, c), device=x.device, dtype=_H16_TORCH[code])
    st = _stream(x)
    _launch("nchw_f32_to_nhwc_h16", 0.0, 6.0 * x.numel(), x,
            lambda: lib().eavsr_nchw_f32_to_nhwc_h16(_p(x), _p(out), n, c, h * w, code, st), "nchw_f32_to_nhwc_h16", stored=(out,))
    return out


def from_nhwc_h16(x: Tensor, residual: Optional[Tensor] = None) -> Tensor:
    """16-bit NHWC (n,h,w,c) -> fp32 NCHW (n,c,h,w) (+ residual)"""
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    code = h16_code(x.dtype)
    out = torch.empty((n, c, h, w), device=x.device, dtype=torch.float32)
    if residual is not None:
        residual = _chk(residual, "residual")
        if residual.shape != out.shape:
            raise ValueError("residual shape mismatch")
    st = _stream(x)
    _launch("nhwc_h16_to_nchw_f32", 0.0, 6.0 * x.numel(), x,
            lambda: lib().eavsr_nhwc_h16_to_nchw_f32(_p(x), _p(residual), _p(out), n, c, h * w, code, st),
            "nhwc_h16_to_nchw_f32", stored=())
    return out


def _packed_h16(weight: Tensor, code: int) -> Tensor:
    return _packed("h16", weight, code)


def conv3x3_c64_h16(x: Tensor, weight: Tensor, bias: Optional[Tensor], relu: bool = False, chan_partial: bool = False,
                    border: bool = False):
    """x: 16-bit NHWC (n,h,w,64); weight: the fp32 (64,64,3,3) parameter (packed + rounded once per version).
    border=True (with chan_partial): a third result, the `BorderPieces` of the output (for ca_scale_pre_h16(.., border=))."""
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    if c != 64:
        raise NotImplementedError("the 16-bit backbone kernel needs 64 channels")
    code = h16_code(x.dtype)
    wp = _packed_h16(weight, code)
    b = None if bias is None else _chk(bias.detach(), "bias")
    out = torch.empty_like(x)
    part = None
    if chan_partial:
        part = torch.empty((n, lib().eavsr_conv_h16_partial_rows(n, h, w), 64), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    if border and chan_partial:
        pr, pc = C.c_int32(0), C.c_int32(0)
        N.check(lib().eavsr_conv_h16_border_pieces(h, w, C.byref(pr), C.byref(pc)), "conv_h16_border_pieces")
        stride = max(pr.value, pc.value)
        pieces = BorderPieces(torch.empty((n, 4, stride, 64), device=x.device, dtype=torch.float32), pr.value, pc.value)
        _launch("conv3x3_64to64_h16", 2.0 * 64 * 64 * 9 * px, 2.0 * px * 128, x,
                lambda: lib().eavsr_conv3x3_c64_h16_b(_p(x), _p(wp), _p(b), _p(out), _p(part), _p(pieces.data), stride, n, h, w,
                                                      1 if relu else 0, code, st), "conv3x3_c64_h16_b", stored=(out,))
        return out, part, pieces
    _launch("conv3x3_64to64_h16", 2.0 * 64 * 64 * 9 * px, 2.0 * px * 128, x,
            lambda: lib().eavsr_conv3x3_c64_h16(_p(x), _p(wp), _p(b), _p(out), _p(part), n, h, w, 1 if relu else 0, code, st),
            "conv3x3_c64_h16", stored=(out,))
    return (out, part) if chan_partial else out




def ca_scale_pre_h16(t: Tensor, partial: Tensor, conv_weight: Tensor, conv_bias: Optional[Tensor], w1: Tensor, b1: Tensor,
                     w2: Tensor, b2: Tensor, border: Optional["BorderPieces"] = None) -> Tensor:
    """The attention of an RCAB (CALayer, networks.py:444-447) BEFORE its second convolution runs: t = the 16-bit NHWC input of
    that convolution, partial = the per-tile channel sums of t from conv3x3_c64_h16(.., relu=True, chan_partial=True),
    conv_weight / conv_bias = the second convolution's parameters.  (n, 64) fp32 for conv3x3_c64_h16(.., skip=, scale=)."""
    t, partial = _chk_h16(t, "t"), _chk(partial, "partial")
    n, h, w, c = t.shape
    if c != 64 or tuple(conv_weight.shape) != (64, 64, 3, 3) or partial.shape[0] != n or partial.shape[2] != 64:
        raise ValueError("ca_scale_pre_h16: 64 channels, a (64, 64, 3, 3) convolution, partial (n, rows, 64)")
    code = h16_code(t.dtype)
    cw = _chk(conv_weight.detach(), "conv_weight")
    cb = None if conv_bias is None else _chk(conv_bias.detach(), "conv_bias")
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    cr = int(w1.shape[0])
    scale = torch.empty((n, 64), device=t.device, dtype=torch.float32)
    st = _stream(t)
    if border is not None:      # the border lines as pieces from the first convolution's epilogue: ONE launch
        bd = _chk(border.data, "border pieces")
        if tuple(bd.shape[:2]) != (n, 4) or bd.shape[3] != 64 or bd.shape[2] < max(border.p_rows, border.p_cols):
            raise ValueError("ca_scale_pre_h16: border pieces must be (n, 4, stride >= max(p_rows, p_cols), 64)")
        _launch("ca_scale_pre_h16", 0.0, 4.0 * (partial.numel() + bd.numel()), t,
                lambda: lib().eavsr_ca_scale_pre_pieces(_p(t), _p(partial), int(partial.shape[1]), _p(bd), border.p_rows, border.p_cols,
                                                        int(bd.shape[2]), _p(cw), _p(cb), _p(w1), _p(b1), _p(w2), _p(b2), _p(scale),
                                                        n, h, w, cr, code, st), "ca_scale_pre_pieces", stored=())
        return scale
    ws = torch.empty(int(lib().eavsr_ca_scale_pre_ws_floats(n)), device=t.device, dtype=torch.float32)
    _launch("ca_scale_pre_h16", 0.0, 4.0 * partial.numel(), t,
            lambda: lib().eavsr_ca_scale_pre_h16(_p(t), _p(partial), int(partial.shape[1]), _p(cw), _p(cb), _p(w1), _p(b1), _p(w2), _p(b2),
                                                 _p(scale), _p(ws), n, h, w, cr, code, st), "ca_scale_pre_h16", stored=())
    return scale


def ca_scale_pre(t: Tensor, partial: Tensor, conv_weight: Tensor, conv_bias: Optional[Tensor], w1: Tensor, b1: Tensor,
                 w2: Tensor, b2: Tensor, border: Optional["BorderPieces"] = None) -> Tensor:
    """ca_scale_pre_h16 for the fp32 NCHW path: t (n, 64, h, w) = ReLU(conv1(x)), partial = its per-tile channel sums (the first
    convolution's chan_partial), conv_weight / conv_bias = the SECOND convolution's.  (n, 64) for conv2d(.., residual=, res_scale=)."""
    t, partial = _chk(t, "t"), _chk(partial, "partial")
    n, c, h, w = t.shape
    if c != 64 or tuple(conv_weight.shape) != (64, 64, 3, 3) or partial.shape[0] != n or partial.shape[2] != 64:
        raise ValueError("ca_scale_pre: 64 channels, a (64, 64, 3, 3) convolution, partial (n, tiles, 64)")
    cw = _chk(conv_weight.detach(), "conv_weight")
    cb = None if conv_bias is None else _chk(conv_bias.detach(), "conv_bias")
    w1, b1, w2, b2 = (_chk(v.detach(), "param") for v in (w1, b1, w2, b2))
    cr = int(w1.shape[0])
    scale = torch.empty((n, 64), device=t.device, dtype=torch.float32)
    st = _stream(t)
    if border is not None:      # the border lines as pieces from the first convolution's epilogue: ONE launch
        bd = _chk(border.data, "border pieces")
        if tuple(bd.shape[:2]) != (n, 4) or bd.shape[3] != 64 or bd.shape[2] < max(border.p_rows, border.p_cols):
            raise ValueError("ca_scale_pre: border pieces must be (n, 4, stride >= max(p_rows, p_cols), 64)")
        _launch("ca_scale_pre", 0.0, 4.0 * (partial.numel() + bd.numel()), t,
                lambda: lib().eavsr_ca_scale_pre_pieces(_p(t), _p(partial), int(partial.shape[1]), _p(bd), border.p_rows, border.p_cols,
                                                        int(bd.shape[2]), _p(cw), _p(cb), _p(w1), _p(b1), _p(w2), _p(b2), _p(scale),
                                                        n, h, w, cr, 0, st), "ca_scale_pre_pieces")
        return scale
    ws = torch.empty(int(lib().eavsr_ca_scale_pre_ws_floats(n)), device=t.device, dtype=torch.float32)
    _launch("ca_scale_pre", 0.0, 4.0 * partial.numel(), t,
            lambda: lib().eavsr_ca_scale_pre_f32(_p(t), _p(partial), int(partial.shape[1]), _p(cw), _p(cb), _p(w1), _p(b1), _p(w2), _p(b2),
                                                 _p(scale), _p(ws), n, h, w, cr, st), "ca_scale_pre")
    return scale


def conv3x3_c64_h16_res(x: Tensor, weight: Tensor, bias: Optional[Tensor], skip: Tensor, scale: Tensor) -> Tensor:
    """skip + scale[n, co] * (conv3x3(x) + bias), rounded once: the RCAB's second convolution with its tail as the epilogue
    (networks.py:461-464); x, skip 16-bit NHWC (n,h,w,64), scale (n, 64) fp32 from ca_scale_pre_h16"""
    x, skip, scale = _chk_h16(x, "x"), _chk_h16(skip, "skip"), _chk(scale, "scale")
    n, h, w, c = x.shape
    if c != 64 or skip.shape != x.shape or skip.dtype != x.dtype or tuple(scale.shape) != (n, 64):
        raise ValueError("conv3x3_c64_h16_res: x / skip (n,h,w,64) of one 16-bit type, scale (n, 64)")
    code = h16_code(x.dtype)
    wp = _packed_h16(weight, code)
    b = None if bias is None else _chk(bias.detach(), "bias")
    out = torch.empty_like(x)
    st = _stream(x)
    px = float(n) * h * w
    _launch("conv3x3_64to64_h16", 2.0 * 64 * 64 * 9 * px, 3.0 * px * 128, x,
            lambda: lib().eavsr_conv3x3_c64_h16_res(_p(x), _p(wp), _p(b), _p(out), _p(skip), _p(scale), n, h, w, code, st),
            "conv3x3_c64_h16_res", stored=(out,))
    return out


# The one-launch RCAB convolutions stream their weights per tile (11.5 us per tile whatever the launch); the resident-weights
# kernel amortises its weight load and prologue over a workgroup's tiles (7.1 us per tile and convolution at 4 tiles per
# workgroup, 5 us at 8).  Measured (tools/gpu_rcab_h16_time.py): 4 x 256 x 256 (4 tiles per workgroup) 49.7 us against 52.3 for the two
# launches, 2 x 180 x 320 (1.8) 25.3 against 31.0, 1 x 540 x 960 (8) 94.1 against 81.7 -- so the fused form is the default up to
# RCAB_FUSED_MAX_TILES tiles per launch (EAVSR_RCAB_FUSED_MAX_TILES overrides).
RCAB_FUSED_MAX_TILES = int(os.environ.get("EAVSR_RCAB_FUSED_MAX_TILES", "1536"))


def rcab_convs_h16_preferred(x: Tensor) -> bool:
    n, h, w, _ = x.shape
    return _rn(n) * ((h + 7) // 8) * ((w + 31) // 32) <= RCAB_FUSED_MAX_TILES


def rcab_convs_h16(x: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor], chan_partial: bool = True):
    """r = conv3x3(ReLU(conv3x3(x))) of one RCAB (networks.py:461-462) as ONE launch on 16-bit NHWC tensors
    (csrc/rcab_h16.hip: streamed weights, the intermediate lives in LDS); with `chan_partial` also the channel sums of r for the
    channel attention, in the row layout of conv3x3_c64_h16."""
    require_lab("ops.rcab_convs_h16 (conv -> ReLU -> conv of a 16-bit RCAB as one launch)")
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    if c != 64:
        raise NotImplementedError("the 16-bit backbone kernel needs 64 channels")
    code = h16_code(x.dtype)
    wp1, wp2 = _packed_h16(w1, code), _packed_h16(w2, code)
    bb1 = None if b1 is None else _chk(b1.detach(), "bias")
    bb2 = None if b2 is None else _chk(b2.detach(), "bias")
    out = torch.empty_like(x)
    part = None
    if chan_partial:
        part = torch.empty((n, lib().eavsr_rcab_h16_partial_rows(n, h, w), 64), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch("rcab_convs_h16", 2.0 * 2.0 * 64 * 64 * 9 * px, 2.0 * px * 128, x,
            lambda: lib().eavsr_rcab_convs_h16(_p(x), _p(wp1), _p(bb1), _p(wp2), _p(bb2), _p(out), _p(part), n, h, w, code, st),
            "rcab_convs_h16")      # (no declaration: its intermediate never leaves LDS, a census refuses the launch)
    return (out, part) if chan_partial else out


_h16_ps_cache = WeightCache()
_h16_last_cache = WeightCache()


def _packed_h16_ps2(weight: Tensor, bias: Optional[Tensor], code: int):
    """(256, 64, 3, 3) weight of a conv + PixelShuffle(2) stage -> four packed 64 -> 64 matrices (slice k = 2 dy + dx: the output
    channels 4 c + k as channel c) and the bias in the same order (4 x 64)"""
    sources = (weight,) if bias is None else (weight, bias)

    def make():
        w = _chk(weight.detach(), "weight")
        if tuple(w.shape) != (256, 64, 3, 3):
            raise NotImplementedError("the 16-bit pixel-shuffle stage is the 3x3 64 -> 256 convolution")
        sl = w.view(64, 4, 64, 3, 3).permute(1, 0, 2, 3, 4).contiguous()      # [k][c][ci][3][3]
        packed = torch.empty(4, 64 * 576, device=w.device, dtype=_H16_TORCH[code])
        st = _stream(w)
        with _DeviceOf(w):
            for k in range(4):
                N.check(lib().eavsr_pack_conv3x3_c64_h16(_p(sl[k]), _p(packed[k]), code, st), "pack_conv3x3_c64_h16")
        return packed, None if bias is None else _chk(bias.detach(), "bias").view(64, 4).t().contiguous()
    return _h16_ps_cache.derive(sources, code, make)


def conv3x3_c64_h16_act(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: Optional[str] = None, slope: float = 0.0,
                        pixel_shuffle2: bool = False) -> Tensor:
    """The upsampling tail in the 16-bit modes: x 16-bit NHWC (n,h,w,64); weight (64,64,3,3) -> act(conv + bias), or, with
    pixel_shuffle2, weight (256,64,3,3) -> act(PixelShuffle(2)(conv + bias)) as (n,2h,2w,64) (eavsrp_model.py:343-357)"""
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    if c != 64:
        raise NotImplementedError("the 16-bit backbone kernel needs 64 channels")
    code = h16_code(x.dtype)
    if pixel_shuffle2:
        wp, b = _packed_h16_ps2(weight, bias, code)
        out = torch.empty((n, 2 * h, 2 * w, 64), device=x.device, dtype=x.dtype)
    else:
        wp = _packed_h16(weight, code)
        b = None if bias is None else _chk(bias.detach(), "bias")
        out = torch.empty_like(x)
    a = ACT[act]
    st = _stream(x)
    px = float(n) * h * w
    co = 256 if pixel_shuffle2 else 64
    _launch("conv3x3_64to256_h16_ps2" if pixel_shuffle2 else "conv3x3_64to64_h16", 2.0 * 64 * co * 9 * px, px * (128 + 2 * co), x,
            lambda: lib().eavsr_conv3x3_c64_h16_act(_p(x), _p(wp), _p(b), _p(out), n, h, w, a, float(slope), 1 if pixel_shuffle2 else 0, code, st),
            "conv3x3_c64_h16_act", stored=(out,))
    return out


def conv3x3_c64to3_h16(x: Tensor, weight: Tensor, bias: Optional[Tensor], residual: Optional[Tensor] = None) -> Tensor:
    """conv_last of the tail in the 16-bit modes: x 16-bit NHWC (n,h,w,64), weight (3,64,3,3) fp32 -> fp32 NCHW (n,3,h,w) (+ residual)"""
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    if c != 64 or tuple(weight.shape) != (3, 64, 3, 3):
        raise NotImplementedError("the 16-bit conv_last kernel is the 3x3 64 -> 3 convolution")
    # [ky][kx][8-channel block][co][8 channels], rounded to the activation type (scalar loads in the kernel)
    wt = _h16_last_cache.derive((weight,), x.dtype,
                                lambda: _chk(weight.detach(), "weight").view(3, 8, 8, 3, 3).permute(3, 4, 1, 0, 2).contiguous().to(x.dtype))
    b = None if bias is None else _chk(bias.detach(), "bias")
    r = None if residual is None else _chk(residual, "residual")
    if r is not None and tuple(r.shape) != (n, 3, h, w):
        raise ValueError("residual must be (n, 3, h, w)")
    out = torch.empty((n, 3, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch("conv3x3_64to3_h16", 2.0 * 64 * 3 * 9 * px, px * (128 + 12 + (12 if r is not None else 0)), x,
            lambda: lib().eavsr_conv3x3_c64to3_h16(_p(x), _p(wt), _p(b), _p(r), _p(out), n, h, w, h16_code(x.dtype), st),
            "conv3x3_c64to3_h16", stored=())
    return out


def _packed5_h16(wcat: Tensor, code: int) -> Tensor:
    """(cout, 64, 5, 5) fp32 (a parameter or the cached concatenation of several) -> the 16-bit MFMA-fragment order"""
    return _packed("h16_5x5", wcat, code)


def conv5x5_c64_h16(x: Tensor, weights, biases) -> Tensor:
    """the predictor's 5x5 heads in the 16-bit modes: x 16-bit NHWC (n,h,w,64); weights / biases: one fp32 (cout,64,5,5) /
    (cout,) parameter or a list of them (concatenated along the output channels); returns fp32 NCHW (n, cout, h, w)"""
    x = _chk_h16(x, "x")
    n, h, w, c = x.shape
    if c != 64:
        raise NotImplementedError("the 16-bit heads kernel needs 64 input channels")
    code = h16_code(x.dtype)
    weights = list(weights) if isinstance(weights, (list, tuple)) else [weights]
    biases = list(biases) if isinstance(biases, (list, tuple)) else [biases]
    wcat = _cat_weights(weights)
    wp = _packed5_h16(wcat, code)
    cout = int(wcat.shape[0])
    b = None
    if any(bb is not None for bb in biases):
        if not all(bb is not None for bb in biases):
            raise ValueError("conv5x5_c64_h16: all heads need a bias or none")
        b = _cat_weights(biases)
    out = torch.empty((n, cout, h, w), device=x.device, dtype=torch.float32)
    st = _stream(x)
    px = float(n) * h * w
    _launch(f"conv5x5_64to{cout}_h16", 2.0 * 64 * cout * 25 * px, px * (128 + 4.0 * cout), x,
            lambda: lib().eavsr_conv5x5_c64_h16(_p(x), _p(wp), _p(b), _p(out), n, h, w, cout, code, st), "conv5x5_c64_h16", stored=())
    return out


def scale_residual_h16(r: Tensor, scale: Tensor, x: Tensor) -> Tensor:
    r, x, scale = _chk_h16(r, "r"), _chk_h16(x, "x"), _chk(scale, "scale")
    n, h, w, c = r.shape
    if x.shape != r.shape or x.dtype != r.dtype or tuple(scale.shape) != (n, c):
        raise ValueError("scale_residual_h16: shape / dtype mismatch")
    out = torch.empty_like(r)
    code = h16_code(r.dtype)
    st = _stream(r)
    _launch("scale_residual_h16", 2.0 * r.numel(), 6.0 * r.numel(), r,
            lambda: lib().eavsr_scale_residual_h16(_p(r), _p(scale), _p(x), _p(out), n, c, h * w, code, st),
            "scale_residual_h16", stored=(out,))
    return out


# ------------------------------------------------------------------------------------------
# PWC-Net of the late-training validity mask (models/pwc_net.py, models/base_model.py:294-354; csrc/pwc.hip).  Operands may be
# channel slices of a larger buffer: (c, h, w) contiguous, any batch stride.
# ------------------------------------------------------------------------------------------
def _batch_stride(t: Tensor, name: str) -> int:
    """batch stride (elements) of a 4-D fp32 GPU tensor whose (c, h, w) part is contiguous -- a channel slice of an NCHW buffer"""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; eavsr_amd runs on the GPU only (no CPU path)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name}: dtype {t.dtype} unsupported (fp32 only)")
    if t.dim() != 4:
        raise ValueError(f"{name}: expected (n, c, h, w), got {tuple(t.shape)}")
    n, c, h, w = t.shape
    s = t.stride()
    if (c > 1 and s[1] != h * w) or (h > 1 and s[2] != w) or (w > 1 and s[3] != 1):
        raise ValueError(f"{name}: (c, h, w) must be contiguous (a channel slice of an NCHW buffer), strides {s}")
    chw = c * h * w
    if n == 1:
        return max(int(s[0]), chw)
    if s[0] < chw:
        raise ValueError(f"{name}: batch stride {s[0]} < c*h*w = {chw}")
    return int(s[0])


def _out_or_new(out: Optional[Tensor], shape, like: Tensor, name: str) -> Tuple[Tensor, int]:
    if out is None:
        out = torch.empty(shape, device=like.device, dtype=torch.float32)
    elif tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name}: `out` has shape {tuple(out.shape)}, expected {tuple(shape)}")
    return out, _batch_stride(out, name)


def _packed_pwc_conv3x3(weight: Tensor) -> Tensor:
    """[9][cin even][cout padded] form of a (cout, cin, 3, 3) weight for eavsr_pwc_conv3x3_f32"""
    return _packed("pwc", weight)


def pwc_conv3x3(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, stride: int = 1, dilation: int = 1,
                act: Optional[str] = "lrelu", slope: float = 0.1, out: Optional[Tensor] = None) -> Tensor:
    """act(F.conv2d(x, weight, bias, stride, padding=dilation, dilation)) for act None | 'lrelu'; `x` and `out` may be channel
    slices of larger buffers (models/pwc_net.py Extractor / Decoder / Refiner)"""
    xs = _batch_stride(x, "x")
    n, cin, h, w = x.shape
    cout = int(weight.shape[0])
    if int(weight.shape[1]) != cin:
        raise ValueError(f"pwc_conv3x3: weight takes {int(weight.shape[1])} channels, input has {cin}")
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    wp = _packed_pwc_conv3x3(weight)
    b = None if bias is None else _chk(bias.detach(), "bias")
    out, os_ = _out_or_new(out, (n, cout, ho, wo), x, "out")
    st = _stream(x)
    px = float(n) * ho * wo
    _launch("pwc_conv3x3", 2.0 * 9 * cin * cout * px, 4.0 * px * (cin + cout), x,
            lambda: lib().eavsr_pwc_conv3x3_f32(_p(x), xs, _p(wp), _p(b), _p(out), os_, n, cin, h, w, cout, int(stride),
                                                 int(dilation), ACT[act], float(slope), st), "pwc_conv3x3")
    return out


def pwc_deconv4x4s2(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """F.conv_transpose2d(x, weight (cin, 2, 4, 4), bias, stride=2, padding=1): netUpflow / netUpfeat (pwc_net.py:113-116)"""
    xs = _batch_stride(x, "x")
    n, cin, h, w = x.shape
    if tuple(weight.shape) != (cin, 2, 4, 4):
        raise ValueError(f"pwc_deconv4x4s2: weight {tuple(weight.shape)}, expected ({cin}, 2, 4, 4)")
    wt = _chk(weight.detach(), "weight")
    b = None if bias is None else _chk(bias.detach(), "bias")
    out, os_ = _out_or_new(out, (n, 2, 2 * h, 2 * w), x, "out")
    st = _stream(x)
    _launch("pwc_deconv4x4s2", 2.0 * 4 * 4 * cin * 2 * n * h * w, 4.0 * n * h * w * (cin + 8), x,
            lambda: lib().eavsr_pwc_deconv4x4s2_f32(_p(x), xs, _p(wt), _p(b), _p(out), os_, n, cin, h, w, st), "pwc_deconv4x4s2")
    return out


def pwc_correlation(a: Tensor, b: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """leaky_relu(FunctionCorrelation(a, b), 0.1) (pwc/correlation/correlation.py:35-103, pwc_net.py:157-167): (n, 81, h, w)"""
    as_, bs_ = _batch_stride(a, "a"), _batch_stride(b, "b")
    if a.shape != b.shape:
        raise ValueError(f"pwc_correlation: shapes {tuple(a.shape)} / {tuple(b.shape)} differ")
    n, c, h, w = a.shape
    out, os_ = _out_or_new(out, (n, 81, h, w), a, "out")
    st = _stream(a)
    _launch("pwc_correlation", 2.0 * 81 * c * n * h * w, 4.0 * n * h * w * (2 * c + 81), a,
            lambda: lib().eavsr_pwc_correlation_f32(_p(a), as_, _p(b), bs_, _p(out), os_, n, c, h, w, st), "pwc_correlation")
    return out


def pwc_backwarp(x: Tensor, flow: Tensor, flow_mul: float = 1.0, out: Optional[Tensor] = None, with_mask: bool = False):
    """Decoder.backwarp (pwc_net.py:184-207) / BaseModel.backwarp + get_backwarp's threshold (base_model.py:321-354): x warped by
    flow_mul x flow (read nearest-upsampled by h / flow_h) on the align_corners=False grid, times the validity mask.  Returns
    `out`, or (out, mask (n, 1, h, w)) with `with_mask`."""
    xs, fs = _batch_stride(x, "x"), _batch_stride(flow, "flow")
    n, c, h, w = x.shape
    if flow.shape[0] != n or flow.shape[1] != 2:
        raise ValueError(f"pwc_backwarp: flow {tuple(flow.shape)} for x {tuple(x.shape)}")
    fh, fw = int(flow.shape[2]), int(flow.shape[3])
    out, os_ = _out_or_new(out, (n, c, h, w), x, "out")
    mask = torch.empty((n, 1, h, w), device=x.device, dtype=torch.float32) if with_mask else None
    st = _stream(x)
    _launch("pwc_backwarp", 8.0 * (c + 1) * n * h * w, 4.0 * n * h * w * (2 * c + 2 + (1 if with_mask else 0)), x,
            lambda: lib().eavsr_pwc_backwarp_f32(_p(x), xs, _p(flow), fs, _p(out), os_, _p(mask), n, c, h, w, fh, fw,
                                                  float(flow_mul), st), "pwc_backwarp")
    return (out, mask) if with_mask else out
