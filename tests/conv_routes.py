"""Helper of tests/test_hip_conv_routes.py (checked on the CPU by tests/test_conv_routes_host.py): which kernels one `ops.conv2d`
call is expected to launch, what it is expected to return, and the case matrix both test files walk.

`predict_route` is a restatement of the router as a decision procedure over plain numbers -- shape, channel lists, options,
pointer offsets, modes, thresholds, the pinned route batch -- that never looks at `ops.py`.  Tile counts come from the library's
own host-side counters (they need no device).  `reference` is the float64 result of one call for any accepted option set.
`boundary_shapes` finds, from a counter, the smallest launches on either side of a threshold.

Names.  A route's `kernels` are the names `ops.profile` records, in launch order; `families` says which kernel family each is
(the small-cout kernels and the direct kernel share the name form `conv3x3_<cin>to<cout>`, their families differ)."""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

OPT_DEFAULTS = dict(act=None, residual=False, chan_partial=False, ca=False, ca_out=False, pixel_shuffle2=False, res_scale=False,
                    sum_mul=False, dgrad=False, sigmoid_from=None, border=False, precision="fp32")
MODE_DEFAULTS = dict(conv="winograd4", conv5="bf16x6", conv7="bf16x6", small="x6s", h16=None, grad=True)
SHIPPED = dict(wino_min=192, x6s_max=256)       # ops.WINO_MIN_TILES / ops.X6S_MAX_TILES as shipped
LOWERED = dict(wino_min=4, x6s_max=6)           # the same gates at h, w <= 96
LAB_MODES = ("winograd", "bf16x9")
PRODUCT_FAMILIES = ("smallco_lite", "smallco_classic", "x6", "h16x1", "h16g", "x6s", "bf16s", "wino5", "wino4", "direct", "direct_ca",
                    "scale_residual", "plane_sum")
LAB_FAMILIES = ("wino4_ca", "wino", "wino_ca", "x9")
SLOPE = 0.1


# ------------------------------------------------------------------------------------------ the library's counters
class Counters:
    """the host-side tile counters of the library (no device needed)"""

    def __init__(self):
        from eavsr_amd import _native
        self.lib = _native.load()

    def x6s(self, h, w):
        return int(self.lib.eavsr_conv3x3_x6s_tiles(h, w))

    def wino4(self, h, w):
        return int(self.lib.eavsr_conv3x3_wino4_tiles(h, w))

    def wino5(self, h, w):
        return int(self.lib.eavsr_conv5x5_wino_tiles(h, w))

    def wino(self, h, w):
        """8 x 32-pixel tiles: the unit WINO_MIN_TILES counts in (the x6s kernel's tile; eavsr_conv3x3_wino_tiles is lab only)"""
        return -(-h // 8) * -(-w // 32)

    def direct(self, n, h, w, k, route_batch=None):
        with self.pinned(route_batch):
            return int(self.lib.eavsr_conv2d_tiles(n, h, w, k))

    def tile_rows(self, n, h, w, k, route_batch=None):
        with self.pinned(route_batch):
            return int(self.lib.eavsr_conv2d_tile_rows(n, h, w, k))

    def ck(self, k):
        return int(self.lib.eavsr_conv2d_ck(k))

    def schedule(self):
        return int(self.lib.eavsr_wino4_schedule())

    @contextlib.contextmanager
    def pinned(self, route_batch):
        prev = self.lib.eavsr_route_batch(int(route_batch or 0))
        try:
            yield
        finally:
            self.lib.eavsr_route_batch(prev)


@functools.lru_cache(None)
def counters() -> Counters:
    return Counters()


@contextlib.contextmanager
def thresholds(ops, wino_min=None, x6s_max=None, conv3_small=None):
    """set ops.WINO_MIN_TILES / X6S_MAX_TILES / CONV3_SMALL for the body (None: leave), restore all three on exit, also on an exception"""
    saved = (ops.WINO_MIN_TILES, ops.X6S_MAX_TILES, ops.CONV3_SMALL)
    try:
        if wino_min is not None:
            ops.WINO_MIN_TILES = int(wino_min)
        if x6s_max is not None:
            ops.X6S_MAX_TILES = int(x6s_max)
        if conv3_small is not None:
            ops.CONV3_SMALL = conv3_small
        yield
    finally:
        ops.WINO_MIN_TILES, ops.X6S_MAX_TILES, ops.CONV3_SMALL = saved


# ------------------------------------------------------------------------------------------ predict_route
@dataclass
class Route:
    raises: Optional[str] = None          # "ValueError" / "NotImplementedError": before any launch
    kernels: Tuple[str, ...] = ()
    families: Tuple[str, ...] = ()
    part_tiles: Optional[int] = None      # the tile axis of the chan_partial / sum_mul result
    pieces: bool = False                  # border=True returns BorderPieces (else None)
    why: str = ""

    @property
    def lab_only(self):
        return any(f in LAB_FAMILIES for f in self.families)


def _rejected(k, chans, cout, o, n_weights, bias) -> Optional[str]:
    """the option combinations conv2d's docstring rules out, whatever the route"""
    masked = o["act"] == "relu_mask"
    if o["precision"] not in ("fp32", "bf16"):
        return "precision"
    if o["sum_mul"] and (not o["dgrad"] or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"] or o["sigmoid_from"] is not None
                         or o["res_scale"] or masked):
        return "sum_mul: input-gradient convolutions only"
    if o["dgrad"] and (n_weights != 1 or bias or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"] or o["sigmoid_from"] is not None
                       or o["res_scale"]):
        return "dgrad: one weight, no bias / sums / prologue / shuffle / sigmoid / scaled residual"
    if o["pixel_shuffle2"] and (cout % 4 or o["residual"] or o["chan_partial"] or o["ca"]):
        return "pixel_shuffle2: cout % 4, no residual / sums / prologue"
    if o["res_scale"] and (not o["residual"] or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"] or o["sigmoid_from"] is not None or masked):
        return "res_scale: with residual only"
    if masked and (not o["residual"] or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"] or o["sigmoid_from"] is not None):
        return "relu_mask: residual = the ReLU's output"
    if o["ca_out"] and not o["ca"]:
        return "ca_out needs ca"
    if o["sigmoid_from"] is not None:
        if not 0 <= o["sigmoid_from"] < cout:
            return "sigmoid_from out of range"
        if o["residual"] or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"]:
            return "sigmoid_from: plain convolutions only"
    return None


def predict_route(n: int, h: int, w: int, k: int, chans: Sequence[int], cout: int, opts: Optional[dict] = None,
                  offsets: Optional[Dict[str, int]] = None, modes: Optional[dict] = None, thr: Optional[dict] = None,
                  route_batch: Optional[int] = None, lab: bool = False, n_weights: int = 1, bias: bool = True,
                  cnt: Optional[Counters] = None) -> Route:
    """chans: the sources' channel counts; cout: the OUTPUT channels of the call (dgrad: the forward weight's input channels).
    offsets: {"src" | "residual" | "ca_x" | "sum_mul": floats past a 16-byte boundary} (the source offset applies to every source).
    thr: {"wino_min", "x6s_max"}; modes: MODE_DEFAULTS keys; lab: the lab library is loaded."""
    o = {**OPT_DEFAULTS, **(opts or {})}
    m = {**MODE_DEFAULTS, **(modes or {})}
    t = {**SHIPPED, **(thr or {})}
    off = {"src": 0, "residual": 0, "ca_x": 0, "sum_mul": 0, **(offsets or {})}
    cnt = cnt or counters()
    chans = tuple(chans)
    cin = sum(chans)
    nr = route_batch or n                       # the batch size every gate counts with
    al16 = lambda name: off[name] % 4 == 0
    al8 = lambda name: off[name] % 2 == 0
    masked = o["act"] == "relu_mask"
    single = len(chans) == 1
    wino_mode = m["conv"] in ("winograd", "winograd4")
    again = lambda **kw: predict_route(n, h, w, k, **{**dict(chans=chans, cout=cout, opts=o, offsets=off, modes=m, thr=t, route_batch=route_batch,
                                                                lab=lab, n_weights=n_weights, bias=bias, cnt=cnt), **kw})
    plain = lambda **keep: {**OPT_DEFAULTS, "act": o["act"], **keep}

    why = _rejected(k, chans, cout, o, n_weights, bias)
    if why:
        return Route(raises="ValueError", why=why)
    x6s_size = nr * cnt.x6s(h, w) <= t["x6s_max"]
    x6s_mode = m["small"] == "x6s" and wino_mode and m["h16"] is None
    # ---- forms that are another call plus a second step
    if o["dgrad"] and not (x6s_mode and k == 3 and single and cin == 64 and cout not in (2, 3, 4, 6) and x6s_size):
        inner = again(opts=plain(residual=o["residual"]), bias=False)       # the materialised transposed weight, a forward call
        if inner.raises or not o["sum_mul"]:
            return inner
        return Route(kernels=inner.kernels + ("plane_sum",), families=inner.families + ("plane_sum",), part_tiles=1, why="dgrad fallback")
    if o["sigmoid_from"] is not None:
        fused = (((k == 7 and m["conv7"] == "bf16x6") or (k == 5 and m["conv5"] == "bf16x6")) and single and cin % 8 == 0
                 and o["sigmoid_from"] % 8 == 0)
        if not fused:
            return again(opts=OPT_DEFAULTS)      # the bare convolution; the two activations by torch: no launch of ours
    # ---- kernels chosen by shape alone
    if k == 3 and single and cout in (2, 3, 4, 6) and not o["chan_partial"] and not o["ca"] and not masked and not o["res_scale"]:
        lite = w % 4 == 0 and al16("src") and h * w * cin * 4 < 2 ** 32
        return Route(kernels=(f"conv3x3_{cin}to{cout}",), families=("smallco_lite" if lite else "smallco_classic",))
    bare = not (o["residual"] or o["chan_partial"] or o["ca"] or o["pixel_shuffle2"])
    if m["h16"] is not None and k == 7 and o["sigmoid_from"] is None and single and cin % 8 == 0 and cout >= 16 and bare and not m["grad"]:
        return Route(kernels=(f"conv7x7_{cin}to{cout}_h16x1",), families=("h16x1",))
    if ((k == 7 and m["conv7"] == "bf16x6") or (k == 5 and m["conv5"] == "bf16x6")) and single and cin % 8 == 0 and bare:
        return Route(kernels=(f"conv{k}x{k}_{cin}to{cout}_x6",), families=("x6",))
    if (m["h16"] is not None and k == 3 and o["sigmoid_from"] is None and bare and w % 4 == 0 and cout >= 32 and not m["grad"]
            and all(c % 16 == 0 for c in chans) and al16("src")):
        return Route(kernels=(f"conv3x3_{cin}to{cout}_h16g",), families=("h16g",))
    # ---- the descriptor kernels
    if any(c % cnt.ck(k) for c in chans[:-1]):          # a ragged source in front: one fresh (aligned) concatenation
        chans, off, single = (cin,), {**off, "src": 0}, True
    if o["ca"] and not single:
        return Route(raises="ValueError", why="ca: one source")
    base = k == 3 and w % 4 == 0 and all(c % 8 == 0 for c in chans) and al16("src")
    wino = (wino_mode and base and not masked and nr * cnt.wino(h, w) >= t["wino_min"]
            and (not o["ca"] or (lab and single and cin <= 256 and al16("ca_x"))))
    wino4 = (wino and m["conv"] == "winograd4" and (not o["residual"] or al16("residual"))
             and 2 * nr * cnt.wino4(h, w) >= t["wino_min"])
    if wino and not wino4 and not lab:
        wino = False
    if o["res_scale"] and not (wino4 and cnt.schedule() >= 1):
        inner = again(chans=chans, offsets=off, opts=plain())
        return Route(kernels=inner.kernels + ("scale_residual",), families=inner.families + ("scale_residual",), why="res_scale fallback")
    if o["pixel_shuffle2"] and not wino4:
        return again(chans=chans, offsets=off, opts=plain())
    wino5 = (m["conv"] == "winograd4" and k == 5 and not o["ca"] and not masked and w % 4 == 0
             and all(c % 4 == 0 for c in chans) and al16("src") and (not o["residual"] or al8("residual"))
             and nr * cnt.wino5(h, w) * -(-cout // 64) >= 2 * t["wino_min"])
    x6s = (m["small"] == "x6s" and wino_mode and k == 3 and single and cin == 64 and not o["ca"] and not o["pixel_shuffle2"] and not wino
           and x6s_size)
    if o["sum_mul"] and not (x6s and w % 4 == 0 and al16("src") and al16("sum_mul") and (not o["residual"] or al16("residual"))):
        inner = again(chans=chans, offsets=off, opts={**o, "sum_mul": False}, bias=False)
        return Route(kernels=inner.kernels + ("plane_sum",), families=inner.families + ("plane_sum",), part_tiles=1, why="sum_mul fallback")
    if o["ca"] and not wino:
        rows32 = cnt.tile_rows(n, h, w, 3, route_batch) == 32
        direct_ok = w % 4 == 0 and cin % 4 == 0 and cin <= 256 and 32 < cout <= 64 and al16("src") and rows32
        lab_ok = lab and wino_mode and w % 4 == 0 and cin % 8 == 0 and cin <= 256 and al16("src") and nr * cnt.wino(h, w) >= t["wino_min"]
        if k != 3 or not (lab_ok or direct_ok) or not al16("ca_x"):
            return Route(raises="NotImplementedError", why="no fused channel-attention prologue for this launch")
    ca = "_ca" if o["ca"] else ""
    sums = o["chan_partial"] or o["sum_mul"]
    if x6s:
        fam = "bf16s" if o["precision"] == "bf16" else "x6s"
        return Route(kernels=(f"conv3x3_{cin}to{cout}_{fam}",), families=(fam,), part_tiles=cnt.x6s(h, w) if sums else None)
    if wino5:
        return Route(kernels=(f"conv5x5_{cin}to{cout}_wino",), families=("wino5",), part_tiles=cnt.wino5(h, w) if sums else None)
    if wino4:
        pieces = (o["border"] and o["chan_partial"] and cout == 64 and cin % 8 == 0 and not o["ca"] and not o["pixel_shuffle2"]
                  and not o["res_scale"] and cnt.schedule() == 1)
        return Route(kernels=(f"conv3x3_{cin}to{cout}_wino4{ca}",), families=("wino4" + ca,), part_tiles=cnt.wino4(h, w) if sums else None,
                     pieces=bool(pieces))
    if wino:
        return Route(kernels=(f"conv3x3_{cin}to{cout}_wino{ca}",), families=("wino" + ca,), part_tiles=cnt.wino(h, w) if sums else None)
    tiles = cnt.direct(n, h, w, k, route_batch) if sums else None
    if m["conv"] == "bf16x9" and base and not o["ca"] and not masked and cnt.tile_rows(n, h, w, 3, route_batch) == 32:
        return Route(kernels=(f"conv3x3_{cin}to{cout}_x9",), families=("x9",), part_tiles=tiles)
    return Route(kernels=(f"conv{k}x{k}_{cin}to{cout}{ca}",), families=("direct" + ca,), part_tiles=tiles)


# ------------------------------------------------------------------------------------------ reference
def reference(srcs, weights, biases, opts: Optional[dict] = None, residual=None, ca=None, res_scale=None, sum_mul=None,
              slope: float = SLOPE, round_to=None) -> dict:
    """float64 result of ops.conv2d(srcs, weights, biases, **opts) on CPU tensors: {"out", "sums" (chan_partial: the plane sums of
    the activated convolution, before the residual; "abs_sums": of its magnitude), "xs" (ca_out), "rows" (sum_mul: plane sums of out * sum_mul), "S" (the same
    convolution of |x| and |w|: the scale of an accumulation-error bound)}.  round_to: a 16-bit dtype the operands are rounded to
    once (the bf16 training mode, the 16-bit modes)."""
    o = {**OPT_DEFAULTS, **(opts or {})}
    rnd = (lambda v: v.to(round_to).double()) if round_to is not None else (lambda v: v.double())
    x = torch.cat([s.double() for s in srcs], 1)
    xs = None
    if o["ca"]:
        scale, cx = ca
        x = x * scale.double()[:, :, None, None] + cx.double()
        xs = x
    ws = [weights] if isinstance(weights, torch.Tensor) else list(weights)
    if o["dgrad"]:
        wt, b = ws[0].flip(2, 3).transpose(0, 1), None
    else:
        wt = torch.cat(ws, 0)
        bs = [biases] if (biases is None or isinstance(biases, torch.Tensor)) else list(biases)
        b = None if all(v is None for v in bs) else torch.cat([torch.zeros(w_.shape[0]) if v is None else v for v, w_ in zip(bs, ws)]).double()
    k = wt.shape[-1]
    raw = F.conv2d(rnd(x), rnd(wt), b, padding=k // 2)
    S = F.conv2d(rnd(x).abs(), rnd(wt).abs(), None, padding=k // 2)
    y = {"relu": F.relu, "lrelu": lambda v: F.leaky_relu(v, slope)}.get(o["act"], lambda v: v)(raw)
    if o["sigmoid_from"] is not None:
        y = torch.cat([y[:, :o["sigmoid_from"]], torch.sigmoid(raw[:, o["sigmoid_from"]:])], 1)
    out = {"sums": y.sum((2, 3)), "abs_sums": y.abs().sum((2, 3)), "xs": xs, "S": S, "rows": None}
    if o["act"] == "relu_mask":
        y = torch.where(residual > 0, y, torch.zeros_like(y))
    elif o["res_scale"]:
        y = residual.double() + res_scale.double()[:, :, None, None] * y
    elif o["residual"]:
        y = y + residual.double()
    if o["sum_mul"]:
        out["rows"] = (y * sum_mul.double()).sum((2, 3))
    out["out"] = F.pixel_shuffle(y, 2) if o["pixel_shuffle2"] else y
    return out


# ------------------------------------------------------------------------------------------ boundary_shapes
def boundary_shapes(threshold: int, count: Callable[[int, int], int], accept: Callable[[int, int, int], bool] = lambda n, h, w: True,
                    max_n: int = 4, max_h: int = 96, max_w: int = 96) -> Dict[str, Tuple[int, int, int]]:
    """{"below": (n, h, w), "at": ..., "above": ...}: the smallest launches (fewest pixels) with n * count(h, w) equal to threshold - 1,
    threshold and threshold + 1 -- or, where no accepted shape has that count, the nearest reachable count on that side ("at" is
    left out when the threshold itself cannot be reached)"""
    best: Dict[int, Tuple[int, Tuple[int, int, int]]] = {}
    for h in range(1, max_h + 1):
        for w in range(1, max_w + 1):
            c1 = None
            for n in range(1, max_n + 1):
                if not accept(n, h, w):
                    continue
                c1 = count(h, w) if c1 is None else c1
                c, px = n * c1, n * h * w
                if c not in best or px < best[c][0]:
                    best[c] = (px, (n, h, w))
    lower = [c for c in best if c < threshold]
    upper = [c for c in best if c > threshold]
    out = {}
    if lower:
        out["below"] = best[max(lower)][1]
    if threshold in best:
        out["at"] = best[threshold][1]
    if upper:
        out["above"] = best[min(upper)][1]
    return out


# ------------------------------------------------------------------------------------------ the case matrix
@dataclass(frozen=True)
class Case:
    id: str
    group: str
    n: int
    h: int
    w: int
    k: int
    chans: Tuple[int, ...]
    couts: Tuple[int, ...]                       # one weight per entry (several heads in one launch)
    opts: Tuple[Tuple[str, object], ...] = ()
    modes: Tuple[Tuple[str, object], ...] = ()
    thr: Tuple[Tuple[str, int], ...] = tuple(LOWERED.items())
    route_batch: Optional[int] = None
    offsets: Tuple[Tuple[str, int], ...] = ()
    side: Optional[str] = None                   # group A: which side of its threshold ("below" / "at" / "above")
    gate: Optional[str] = None                   # group A: the threshold's name

    @property
    def cout(self):
        return sum(self.couts)

    @property
    def o(self):
        return {**OPT_DEFAULTS, **dict(self.opts)}

    @property
    def m(self):
        return {**MODE_DEFAULTS, **dict(self.modes)}

    @property
    def bias(self):
        return not self.o["dgrad"]

    def route(self, lab: bool = False, **kw) -> Route:
        args = dict(opts=self.o, offsets=dict(self.offsets), modes=self.m, thr=dict(self.thr), route_batch=self.route_batch, lab=lab,
                    n_weights=len(self.couts), bias=self.bias)
        args.update(kw)
        return predict_route(self.n, self.h, self.w, self.k, self.chans, self.cout, **args)


def _case(id, group, shape, k, chans, couts, opts=None, modes=None, thr=LOWERED, **kw):
    n, h, w = shape
    return Case(id, group, n, h, w, k, tuple(chans), tuple(couts) if isinstance(couts, (tuple, list)) else (couts,),
                tuple(sorted((opts or {}).items())), tuple(sorted((modes or {}).items(), key=lambda kv: kv[0])), tuple(sorted(thr.items())), **kw)


ALL3 = dict(act="relu", residual=True, chan_partial=True)

# every option, alone or in the smallest accepted company, and the combinations the docstring rules out
OPTION_SETS = {
    "plain": {}, "relu": dict(act="relu"), "lrelu": dict(act="lrelu"), "residual": dict(residual=True), "sums": dict(chan_partial=True),
    "all3": ALL3, "ca": dict(ca=True), "ca_out": dict(ca=True, ca_out=True, act="relu", chan_partial=True),
    "shuffle": dict(pixel_shuffle2=True, act="lrelu"), "res_scale": dict(res_scale=True, residual=True),
    "dgrad": dict(dgrad=True), "dgrad_res": dict(dgrad=True, residual=True), "dgrad_mask": dict(dgrad=True, residual=True, act="relu_mask"),
    "sum_mul": dict(dgrad=True, residual=True, sum_mul=True), "mask": dict(residual=True, act="relu_mask"),
    "sigmoid": dict(sigmoid_from=8, act="relu"), "border": dict(border=True, chan_partial=True, act="relu"), "border_alone": dict(border=True),
    "bf16": dict(precision="bf16", act="relu", residual=True), "bf16_sum_mul": dict(precision="bf16", dgrad=True, residual=True, sum_mul=True),
    # rejected on every route
    "x_ca_out": dict(ca_out=True), "x_shuffle_res": dict(pixel_shuffle2=True, residual=True), "x_res_scale": dict(res_scale=True),
    "x_sum_mul": dict(sum_mul=True, residual=True), "x_mask": dict(act="relu_mask"), "x_sigmoid_res": dict(sigmoid_from=8, residual=True),
    "x_dgrad_sums": dict(dgrad=True, chan_partial=True), "x_dgrad_res_scale": dict(dgrad=True, residual=True, res_scale=True),
    "x_mask_sums": dict(act="relu_mask", residual=True, chan_partial=True),
}
REJECTED = tuple(k for k in OPTION_SETS if k.startswith("x_"))

# one launch per route (thresholds LOWERED): name -> (shape, k, chans, couts, modes)
ROUTE_SHAPES = {
    "smallco": ((2, 12, 16), 3, (64,), 3, {}),
    "smallco_w18": ((1, 9, 18), 3, (20,), 6, {}),
    "x6s": ((1, 20, 28), 3, (64,), 64, {}),
    "wino4": ((2, 13, 68), 3, (64,), 64, {}),
    "wino4_2src": ((1, 24, 64), 3, (8, 16), 40, {}),
    "wino5": ((2, 12, 36), 5, (16,), 40, dict(conv5="wino")),
    "x6_5x5": ((2, 12, 36), 5, (16,), 40, {}),
    "x6_7x7": ((1, 10, 19), 7, (8,), 32, {}),
    "direct_2src": ((1, 13, 37), 3, (64, 64), 64, {}),
    "direct_1x1": ((2, 9, 35), 1, (64, 64, 64), 64, {}),
    "direct_ragged": ((1, 11, 20), 3, (3, 5, 8), 24, {}),
}
# the family each of them runs on with no option set, in the default mode
ROUTE_FAMILY = {"smallco": "smallco_lite", "smallco_w18": "smallco_classic", "x6s": "x6s", "wino4": "wino4", "wino4_2src": "wino4",
                "wino5": "wino5", "x6_5x5": "x6", "x6_7x7": "x6", "direct_2src": "direct", "direct_1x1": "direct", "direct_ragged": "direct"}
CONV_MODES = ("winograd4", "direct")


def _count_of(name):
    return getattr(counters(), name)


def _group_a():
    cnt = counters()
    out = []
    for mode in CONV_MODES + LAB_MODES:
        md = dict(conv=mode)
        # WINO_MIN_TILES (the 8 x 32-pixel count); the second gate (2 n wino4_tiles) must hold on the upper side
        for label, thr, lim in (("lowered", LOWERED, dict()), ("shipped", SHIPPED, dict(max_w=256))):
            if label == "shipped" and mode != "winograd4":
                continue
            tri = boundary_shapes(thr["wino_min"], cnt.wino, lambda n, h, w: w % 4 == 0 and h % 8 == 0 and n * cnt.x6s(h, w) <= thr["x6s_max"], **lim)
            for side, shape in tri.items():
                out.append(_case(f"A-wino_min-{label}-{mode}-{side}", "A", shape, 3, (64,), 64, ALL3, md, thr, side=side, gate=f"wino_min-{label}"))
            tri = boundary_shapes(thr["x6s_max"], cnt.x6s, lambda n, h, w: w % 4 == 1 and w > 32 and h % 8 == 1, **lim)
            for side, shape in tri.items():
                out.append(_case(f"A-x6s_max-{label}-{mode}-{side}", "A", shape, 3, (64,), 64, ALL3, md, thr, side=side, gate=f"x6s_max-{label}"))
        # the 5x5 gate n * tiles * ceil(cout / 64) >= 2 * WINO_MIN_TILES = 8: 2, 4 and 8 tiles of 4 x 32 pixels
        for cout in (40, 64, 72, 128):
            for shape in ((1, 8, 32), (1, 16, 32), (1, 32, 32)):
                c = cnt.wino5(*shape[1:]) * -(-cout // 64)
                side = "below" if c < 2 * LOWERED["wino_min"] else "at" if c == 2 * LOWERED["wino_min"] else "above"
                out.append(_case(f"A-wino5-o{cout}-{mode}-{shape[1]}x{shape[2]}", "A", shape, 5, (64,), cout, ALL3, dict(md, conv5="wino"),
                                 side=side, gate=f"wino5-o{cout}"))
        # tile_rows == 32: the fused channel-attention prologue of the direct kernel, the nine-product kernel.  No launch of n <= 4,
        # h, w <= 96 has 32-row tiles of its own; a pinned route batch (forward_long's chunks) gives them to a one-image launch
        lo, hi = rows32_batches(32, 32)
        for side, rb in (("below", lo), ("at", hi)):
            out.append(_case(f"A-rows32-ca-{mode}-{side}", "A", (1, 32, 32), 3, (64,), 64, dict(ca=True, ca_out=True, act="relu", chan_partial=True),
                             md, route_batch=rb, side=side, gate="rows32-ca"))
            if mode == "bf16x9":
                out.append(_case(f"A-rows32-x9-{side}", "A", (1, 32, 32), 3, (64,), 64, ALL3, md, route_batch=rb, side=side, gate="rows32-x9"))
    return out


def rows32_batches(h, w):
    """(the largest pinned batch below which an (h, w) launch has no 32-row tiles, the smallest at which it has)"""
    cnt = counters()
    rb = next(r for r in range(1, 4096) if cnt.tile_rows(1, h, w, 3, r) == 32)
    assert cnt.tile_rows(1, h, w, 3, rb - 1) != 32
    return rb - 1, rb


def _group_b():
    out = []
    for rname, (shape, k, chans, couts, md) in ROUTE_SHAPES.items():
        for oname, opts in OPTION_SETS.items():
            for mode in CONV_MODES:      # (innermost: the two modes share the cached operands and reference)
                # dgrad: `couts` is the forward weight's input-channel count, its output channels are the sources' (one weight)
                out.append(_case(f"B-{rname}-{oname}-{mode}", "B", shape, k, chans, couts, opts, dict(md, conv=mode)))
    for mode in LAB_MODES:      # the retired schedules: the plain forms and the prologue
        for rname in ("x6s", "wino4", "direct_2src"):
            shape, k, chans, couts, md = ROUTE_SHAPES[rname]
            for oname in ("all3", "ca_out", "mask", "shuffle"):
                out.append(_case(f"B-{rname}-{oname}-{mode}", "B", shape, k, chans, couts, OPTION_SETS[oname], dict(md, conv=mode)))
    # the predictor's three heads in one launch, the sigmoid on the last
    for mode in CONV_MODES:
        for conv5 in ("bf16x6", "wino"):
            out.append(_case(f"B-heads5x5-{conv5}-{mode}", "B", (2, 12, 36), 5, (64,), (8, 8, 16), dict(sigmoid_from=16), dict(conv=mode, conv5=conv5)))
        out.append(_case(f"B-heads5x5-2src-{mode}", "B", (2, 12, 36), 5, (32, 32), (8, 8, 16), dict(sigmoid_from=16), dict(conv=mode)))
        out.append(_case(f"B-heads5x5-odd-{mode}", "B", (2, 12, 36), 5, (64,), (8, 8, 16), dict(sigmoid_from=12), dict(conv=mode)))
    return out


def _group_c():
    out = []
    rb = rows32_batches(32, 32)[1]
    for o in (1, 2, 3):
        for rname in ("smallco", "x6s", "wino4", "wino5", "x6_5x5", "direct_2src", "direct_1x1"):
            shape, k, chans, couts, md = ROUTE_SHAPES[rname]
            for which in ("src", "residual"):
                opts = dict(act="relu") if (which, rname[:3]) == ("src", "x6_") else dict(act="relu", residual=True)
                if rname in ("x6s", "wino4", "direct_2src") and which == "src":
                    opts = ALL3
                out.append(_case(f"C-{rname}-{which}+{o}", "C", shape, k, chans, couts, opts, md, offsets=((which, o),)))
        for which in ("src", "ca_x"):
            out.append(_case(f"C-ca-{which}+{o}", "C", (1, 32, 32), 3, (64,), 64, dict(ca=True, ca_out=True), {}, route_batch=rb, offsets=((which, o),)))
        for which in ("src", "residual", "sum_mul"):
            for mode, shape in (("winograd4", (1, 16, 32)), ("direct", (1, 16, 32)), ("winograd4", (2, 13, 68))):
                out.append(_case(f"C-sum_mul-{which}+{o}-{mode}-{shape[2]}", "C", shape, 3, (64,), 64, OPTION_SETS["sum_mul"], dict(conv=mode),
                                 offsets=((which, o),)))
    return out


# D: one batch whose whole and whose single rows fall on different sides of a gate
ROUTE_BATCH_CASES = (
    _case("D-wino_min", "D", (2, 8, 64), 3, (64,), 64, ALL3),
    _case("D-x6s_max", "D", (2, 17, 33), 3, (64,), 64, ALL3),
    _case("D-wino5", "D", (2, 8, 32), 5, (64,), 128, ALL3, dict(conv5="wino")),
)


def _group_e():
    out = []
    tiny = ((1, 1, 5), (2, 2, 3), (1, 3, 1), (1, 5, 2), (1, 1, 4))
    thr = dict(wino_min=0, x6s_max=6)      # every launch the Winograd kernels accept reaches them
    for rname in ("smallco", "x6s", "wino5", "x6_5x5", "x6_7x7", "direct_2src", "direct_1x1"):
        _, k, chans, couts, md = ROUTE_SHAPES[rname]
        for shape in tiny:
            for mode in CONV_MODES:
                out.append(_case(f"E-{rname}-{mode}-{shape[0]}x{shape[1]}x{shape[2]}", "E", shape, k, chans, couts,
                                 dict(act="relu") if rname.startswith("x6_") else dict(act="relu", residual=True), dict(md, conv=mode), thr))
    for mode in CONV_MODES:
        # an empty batch, where the library is known to accept one (the bf16x6 kernels; the direct kernel's entry wants buffers)
        for rname in ("x6s", "x6_5x5", "x6_7x7") if mode == "winograd4" else ("x6_5x5", "x6_7x7"):
            _, k, chans, couts, md = ROUTE_SHAPES[rname]
            out.append(_case(f"E-{rname}-{mode}-empty", "E", (0, 9, 9), k, chans, couts, {}, dict(md, conv=mode), thr))
    return out


def _group_f():
    out = []
    for dt in ("bf16", "fp16"):
        for tag, shape, k, chans, cout, grad in (("h16g", (1, 9, 16), 3, (64,), 64, False), ("h16g-2src", (2, 7, 8), 3, (64, 16), 96, False),
                                                 ("grad", (1, 9, 16), 3, (64,), 64, True), ("w18", (1, 9, 18), 3, (64,), 64, False),
                                                 ("o16", (1, 9, 16), 3, (64,), 16, False), ("c24", (1, 9, 16), 3, (24,), 64, False),
                                                 ("h16x1", (1, 9, 12), 7, (8,), 32, False), ("k7-grad", (1, 9, 12), 7, (8,), 32, True),
                                                 ("k7-o2", (1, 9, 12), 7, (16,), 2, False)):
            out.append(_case(f"F-{dt}-{tag}", "F", shape, k, chans, cout, dict(act="relu"), dict(h16=dt, grad=grad)))
    return out


@functools.lru_cache(None)
def cases() -> Tuple[Case, ...]:
    out = _group_a() + _group_b() + _group_c() + list(ROUTE_BATCH_CASES) + _group_e() + _group_f()
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    return tuple(out)


@contextlib.contextmanager
def case_setup(ops, case):
    """the case's modes, thresholds, route batch and grad mode for the body; everything is put back on exit"""
    m, thr = case.m, dict(case.thr)
    was = ops.CONV5_MODE, ops.CONV7_MODE, ops.CONV3_H16
    with contextlib.ExitStack() as st:
        st.enter_context(ops.modes(conv=m["conv"]))      # a lab mode on the product library: LabBuildRequired = a skip (conftest.py)
        st.enter_context(thresholds(ops, thr["wino_min"], thr["x6s_max"], m["small"]))

        def back():
            ops.CONV5_MODE, ops.CONV7_MODE, ops.CONV3_H16 = was
        st.callback(back)
        ops.CONV5_MODE, ops.CONV7_MODE = m["conv5"], m["conv7"]
        ops.set_conv3_h16(m["h16"])
        st.enter_context(ops.route_batch(case.route_batch))
        st.enter_context(torch.enable_grad() if m["grad"] else torch.no_grad())
        yield


# ------------------------------------------------------------------------------------------ a case's tensors and its reference
@functools.lru_cache(maxsize=128)
def inputs(n, h, w, k, chans, couts, opts) -> dict:
    """seeded CPU operands of a case (shared by the cases that differ in mode, thresholds or pointer offsets only): inputs randn,
    weights randn / sqrt(cin k^2), biases 0.1 randn"""
    o = {**OPT_DEFAULTS, **dict(opts)}
    g = torch.Generator().manual_seed(1000 + 17 * h + w + k)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    cin, cout = sum(chans), sum(couts)
    t = {"srcs": [rn(n, c, h, w) for c in chans]}
    if o["dgrad"]:      # ONE forward weight (dY channels, output channels, k, k), no bias
        t["weights"], t["biases"] = [rn(cin, cout, k, k, scale=(cout * k * k) ** -0.5)], None
    else:
        t["weights"] = [rn(co, cin, k, k, scale=(cin * k * k) ** -0.5) for co in couts]
        t["biases"] = [rn(co, scale=0.1) for co in couts]
    r = rn(n, cout, h, w)
    t["residual"] = (torch.relu(r) if o["act"] == "relu_mask" else r) if o["residual"] else None
    t["ca"] = (torch.rand(n, cin, generator=g), rn(n, cin, h, w)) if o["ca"] else None
    t["res_scale"] = torch.rand(n, cout, generator=g) if o["res_scale"] else None
    t["sum_mul"] = rn(n, cout, h, w) if o["sum_mul"] else None
    return t


def inputs_of(case: Case) -> dict:
    return inputs(case.n, case.h, case.w, case.k, case.chans, case.couts, case.opts)


_ROUND = {"bf16": torch.bfloat16, "fp16": torch.float16}


@functools.lru_cache(maxsize=128)
def _reference(n, h, w, k, chans, couts, opts, round_to):
    t = inputs(n, h, w, k, chans, couts, opts)
    return reference(t["srcs"], t["weights"], t["biases"], dict(opts), t["residual"], t["ca"], t["res_scale"], t["sum_mul"],
                     round_to=_ROUND.get(round_to))


def reference_of(case: Case, round_to: Optional[str] = None) -> dict:
    """the (cached, never modified) float64 reference of a case; round_to: "bf16" / "fp16" for the routes that round their operands"""
    return _reference(case.n, case.h, case.w, case.k, case.chans, case.couts, case.opts, round_to)
