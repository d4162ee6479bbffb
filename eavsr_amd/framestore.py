"""Per-frame tensors of a long clip (EAVSRP.forward_long): where they live and when they move.

A clip of t frames keeps, per frame, the encoder's pyramid (`spatial`, `spatial_d2`, `spatial_d4`), the four propagation
branches, the two flows and the fp32 LR frame.  `DeviceStore` keeps them in device memory as `EAVSRP.forward` does (frame-major
buffers, a frame is a contiguous slice).  `HostStore` is the `cpu_cache` of the BasicVSR family: every frame lives in pinned host
memory and the device holds a WINDOW -- what the current and the next time step of `propagate` read -- filled by copies on one
side stream that run ahead of the compute stream, ordered by events only.

The order in which `propagate` reads its inputs is known before it starts (`propagate_reads`), so the copies follow a schedule
computed on the host (`prefetch_schedule`): both are pure functions of (t, direction, earlier branches) and are tested without a
GPU.
"""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor
Item = Tuple[str, int]

PYR = ("spatial", "spatial_d2", "spatial_d4")
FLOW_KEYS = ("flow_backward", "flow_forward")


def propagate_reads(t: int, backward: bool, others: Sequence[str] = ()) -> List[List[Item]]:
    """What time step i of one propagation branch over t frames reads from the store, as (key, frame) pairs in the order the step
    uses them (eavsrp_model.py:242-329): the current frame's pyramid; from the second step on the neighbour's pyramid and the flow
    between the two; from the third step on the second neighbour's pyramid and the flow one step further; the frame's features of
    every earlier branch (`others`).  A backward branch walks frames t-1 .. 0 and reads `flow_backward`, a forward branch walks
    0 .. t-1 and reads `flow_forward`; flow j joins frames j and j + 1.  (The branch's own last two outputs are the recurrence's
    state: they never leave the device and are not listed.)"""
    if t < 1:
        raise ValueError(f"propagate_reads: t >= 1, got {t}")
    order = list(range(t))[::-1] if backward else list(range(t))
    step = 1 if backward else -1
    fkey = FLOW_KEYS[0] if backward else FLOW_KEYS[1]
    reads: List[List[Item]] = []
    for i, idx in enumerate(order):
        r: List[Item] = [(k, idx) for k in PYR]
        if i > 0:
            r += [(k, idx + step) for k in PYR]
            r.append((fkey, idx if backward else idx - 1))
            if i > 1:
                r += [(k, idx + 2 * step) for k in PYR]
                r.append((fkey, idx + 1 if backward else idx - 2))
        r += [(k, idx) for k in others]
        reads.append(r)
    return reads


class Schedule(NamedTuple):
    """prologue: copied in before step 0 is enqueued (what step 0 reads).  fetch[i]: copies started when step i is enqueued -- what
    step i + 1 reads and the window does not hold yet; they overlap step i's kernels.  evict[i]: dropped from the window once step
    i is enqueued (nothing step i + 1 reads)."""
    prologue: List[Item]
    fetch: List[List[Item]]
    evict: List[List[Item]]


def prefetch_schedule(reads: Sequence[Sequence[Item]]) -> Schedule:
    """One step of lookahead: while step i computes, the window holds reads[i] and reads[i + 1].  Every tensor is read in
    consecutive steps only (a pyramid frame as current, neighbour, second neighbour; a flow twice; an earlier branch's frame once),
    so nothing is ever fetched twice and nothing is dropped before its last use."""
    def unique(items):
        return list(dict.fromkeys(items))
    prologue = unique(reads[0]) if reads else []
    resident = set(prologue)
    fetch, evict = [], []
    for i in range(len(reads)):
        nxt = unique(reads[i + 1]) if i + 1 < len(reads) else []
        f = [it for it in nxt if it not in resident]
        resident.update(f)
        keep = set(nxt)
        e = sorted(it for it in resident if it not in keep)
        resident.difference_update(e)
        fetch.append(f)
        evict.append(e)
    return Schedule(prologue, fetch, evict)


def window_bound(n_others: int) -> Dict[str, int]:
    """The most frames of each kind the window of `prefetch_schedule(propagate_reads(..))` ever holds: four pyramid frames (current,
    two neighbours, the next step's new frame) at each of the three levels, three flows, two frames of every earlier branch."""
    return {"pyramid_frames": 4, "flows": 3, "frames_per_other_branch": 2, "items": 3 * 4 + 3 + 2 * int(n_others)}


def check_cache(cache: str) -> str:
    if cache not in ("device", "host"):
        raise ValueError(f"cache {cache!r}: 'device' or 'host'")
    return cache


CACHE_DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def check_cache_dtype(x) -> Optional[str]:
    """None (fp32 features, today's stores) | "fp16" | "bf16", also given as torch.float16 / torch.bfloat16 -> None, "fp16" or "bf16";
    anything else is refused"""
    if x is None:
        return None
    if isinstance(x, str) and x in CACHE_DTYPES:
        return x
    if isinstance(x, torch.dtype):
        for name, dt in CACHE_DTYPES.items():
            if x == dt:
                return name
    raise ValueError(f"cache_dtype {x!r}: None, 'fp16' or 'bf16' (torch.float16 / torch.bfloat16)")


CACHE_CHECKS = ("report", "raise", "bf16")
# the rows of a store's census tensor, one per key a 16-bit store rounds (`is_feature_key`): the pyramid and the four branches
CENSUS_KEYS = PYR + ("backward_1", "forward_1", "backward_2", "forward_2")


def check_cache_check(x, cache_dtype) -> Optional[str]:
    """`cache_check` beside a `cache_dtype` that `check_cache_dtype` has passed (addendum): None (no census: today's
    launches) | "report" (count what the rounding did, read it when the window has ended) | "raise" (read it before the first frame
    leaves, refuse a window that overflowed or held inf / NaN) | "bf16" (likewise, and run an fp16 window that overflowed again on a
    bf16 store).  Refused: anything else, a check without a 16-bit cache to check, "bf16" where the cache is not fp16."""
    if x is None:
        return None
    if not isinstance(x, str) or x not in CACHE_CHECKS:
        raise ValueError(f"cache_check {x!r}: None, 'report', 'raise' or 'bf16'")
    if cache_dtype is None:
        raise ValueError(f"cache_check {x!r} without cache_dtype: the census is taken where features are rounded to 16 bits")
    if x == "bf16" and cache_dtype != "fp16":
        raise ValueError(f"cache_check 'bf16' with cache_dtype {cache_dtype!r}: the fallback is from an fp16 cache")
    return x


def out_of_range(keys: Dict[str, Dict]) -> List[str]:
    """the keys of a census whose features did not fit: a finite value rounded to inf, or inf / NaN going in"""
    return [k for k, r in keys.items() if r["overflow"] > 0 or r["nonfinite"] > 0]


class CacheRangeError(ValueError):
    """a window whose features do not fit the 16-bit cache (`cache_check="raise"`); `entry` is the window's census entry"""

    def __init__(self, entry: Dict):
        self.entry = entry
        keys = entry["keys"]
        parts = [f"{k}: max |x| {keys[k]['max_abs']:.6g}, {keys[k]['overflow']} overflowed, {keys[k]['nonfinite']} non-finite "
                 f"of {keys[k]['elements']}" for k in out_of_range(keys)]
        super().__init__(f"cache_dtype {entry['asked']!r}: features out of range in a window of {entry['frames']} frames of "
                         f"{entry['size'][0]} x {entry['size'][1]} -- " + "; ".join(parts) +
                         " (nothing of this window has reached the sink; cache_check='bf16' runs such a window on a bf16 cache)")


def checked_window(make, fill, drain, cache_dtype, cache_check, about: Dict, log: List):
    """The order of one `forward_long` call under a `cache_check` -- pure host code over three callables: `make(dtype, census)` builds
    a store, `fill(store)` runs stages 1 and 2 (every pack of the window) and returns what `drain(store, state)`, stage 3 -- the only
    stage that feeds the sink -- needs.  None: make, fill, drain, finish, as ever.  "report": the same with a census, read back once
    after `finish`.  "raise" / "bf16": the census is read between fill and drain (the one synchronisation the check adds); "raise"
    refuses a window that is `out_of_range`; "bf16" drops the store of a window that overflowed, makes a bf16 one and fills it again
    -- once -- and reads that store's census after `finish` ('keys_used').  Every checked call appends its entry to `log`, a refused
    one before it raises.  Returns what `drain` returned."""
    store = make(cache_dtype, cache_check is not None)
    state = fill(store)
    if cache_check is None:
        out = drain(store, state)
        store.finish()
        return out
    entry = dict(asked=cache_dtype, used=cache_dtype, fallback=False, **about, keys=None)
    if cache_check != "report":
        entry["keys"] = store.census()
        if cache_check == "raise" and out_of_range(entry["keys"]):
            store.finish()
            log.append(entry)
            raise CacheRangeError(entry)
        if cache_check == "bf16" and any(r["overflow"] > 0 for r in entry["keys"].values()):
            store.finish()
            store = state = None      # the fp16 store's memory goes before the bf16 store's is taken
            store = make("bf16", True)
            state = fill(store)
            entry.update(used="bf16", fallback=True)
    out = drain(store, state)
    store.finish()
    if cache_check == "report":
        entry["keys"] = store.census()
    elif entry["fallback"]:
        entry["keys_used"] = store.census()
    log.append(entry)
    return out


class StoreBox:
    """What `checked_window` owns where a caller may have to fill a window twice (`EAVSRP.forward_long` under a
    `networks.backbone_check` that falls back): `store` is the store in use, `renew()` finishes and drops it and makes a fresh one
    with the same arguments -- the old store's memory goes before the new one's is taken.  `census` and `finish` are the store's in
    use, so the cache census describes the features that stage 3 read."""

    def __init__(self, make):
        self._make, self.store = make, make()

    def renew(self) -> None:
        self.store.finish()
        self.store = None
        self.store = self._make()

    def census(self):
        return self.store.census()

    def finish(self) -> None:
        self.store.finish()


def census_summary(log: Sequence[Dict]) -> Dict:
    """one line over the entries of `EAVSRP.cache_census`: the largest |x| any key of any window held, the totals of its counts, and
    how many windows fell back to bf16 (the counts of a window that fell back are its fp16 attempt's, 'keys')"""
    rows = [r for e in log for r in (e["keys"] or {}).values()]
    out = {"windows": len(log), "fallbacks": sum(1 for e in log if e["fallback"]), "max_abs": max([r["max_abs"] for r in rows], default=0.0)}
    out.update({k: sum(r[k] for r in rows) for k in ("nonfinite", "overflow", "flushed", "subnormal")})
    return out


class _Census:
    """What a 16-bit store adds with census=True: one int64 (len(CENSUS_KEYS), 5) tensor on the device, zeroed once; a key's packs add
    into the key's row (`ops.pack16_census`); the elements put per key are counted on the host."""

    def _census_init(self, census: bool, device) -> None:
        self._counts: Optional[Tensor] = torch.zeros((len(CENSUS_KEYS), 5), dtype=torch.int64, device=device) if census else None
        self._elements: Dict[str, int] = {}

    def _census_row(self, key: str, src: Tensor) -> Tensor:
        if key not in CENSUS_KEYS:
            raise ValueError(f"census: no row for feature key {key!r} ({', '.join(CENSUS_KEYS)})")
        self._elements[key] = self._elements.get(key, 0) + int(src.numel())
        return self._counts[CENSUS_KEYS.index(key)]

    def census(self) -> Dict[str, Dict]:
        """{key: `ops.census_record`} for the keys that were put, from ONE read-back of the tensor (the host waits for the packs)"""
        if self._counts is None:
            raise RuntimeError("census(): the store was made without census=True")
        from . import ops
        rows = self._counts.cpu().tolist()
        return {key: ops.census_record(rows[i], self._elements[key], self.dtype) for i, key in enumerate(CENSUS_KEYS) if key in self._elements}


def is_feature_key(key: str) -> bool:
    """what a 16-bit store rounds: the pyramid levels and every branch's outputs -- 64 channels each.  The flows (2 channels of pixel
    offsets) and the LR frames stay fp32."""
    return key not in FLOW_KEYS and key != "lr"


def expected_nbytes(n: int, t: int, h: int, w: int, branches: int = 4, dtype=None, channels: int = 64) -> Dict[str, int]:
    """`nbytes()` of a store that holds a whole clip of n x t frames of h x w, from shapes alone: per frame and clip
    channels h w (1 + 1/4 + 1/16 + branches) feature elements of 4 bytes (2 with a 16-bit `dtype`) -- 1360 h w bytes in fp32 with four
    branches -- plus the t - 1 flows of each direction and the LR frames at full size"""
    size = 4 if check_cache_dtype(dtype) is None else 2
    out = {"spatial": channels * h * w, "spatial_d2": channels * (h // 2) * (w // 2), "spatial_d4": channels * (h // 4) * (w // 4)}
    out.update({f"{d}_{i}": channels * h * w for i in (1, 2) for d in ("backward", "forward")} if branches == 4 else
               {f"branch_{i}": channels * h * w for i in range(branches)})
    out = {k: v * size * n * t for k, v in out.items()}
    out.update({k: 2 * h * w * 4 * n * (t - 1) for k in FLOW_KEYS})
    out["lr"] = 3 * h * w * 4 * n * t
    out["total"] = sum(out.values())
    return out


class DeviceStore:
    """Today's residency: every frame stays in device memory.  A range of frames put as one frame-major tensor ((k n, c, h, w),
    frame-major rows) is kept as that tensor; a frame, or an aligned range, is a contiguous slice of it."""
    cache = "device"

    def __init__(self, n: int, t: int, device):
        self.n, self.t, self.device = int(n), int(t), device
        self._blocks: Dict[str, List[Tuple[int, int, Tensor]]] = {}      # key -> [(first frame, frames, tensor)]
        self._where: Dict[Item, Tuple[Tensor, int]] = {}                 # (key, frame) -> (tensor, frame offset in it)

    def put_range(self, key: str, first: int, frames: Tensor) -> None:
        k = int(frames.shape[0]) // self.n
        self._blocks.setdefault(key, []).append((first, k, frames))
        for j in range(k):
            self._where[(key, first + j)] = (frames, j)

    def new_branch(self, key: str, like: Tensor) -> None:
        """one frame-major buffer for a branch's t outputs: `out_slot` hands out its rows, `upsample` reads it without a torch.cat"""
        self.put_range(key, 0, like.new_empty((self.t * self.n,) + tuple(like.shape[1:])))

    def out_slot(self, key: str, idx: int) -> Optional[Tensor]:
        return self.get(key, idx)

    def put(self, key: str, idx: int, frame: Tensor) -> None:
        if (key, idx) not in self._where:      # (a branch writes into its out_slot: nothing to do then)
            self.put_range(key, idx, frame)

    def get(self, key: str, idx: int) -> Tensor:
        block, j = self._where[(key, idx)]
        return block[j * self.n:(j + 1) * self.n]

    def get_range(self, key: str, a: int, b: int) -> Tensor:
        for first, k, block in self._blocks[key]:
            if first <= a and b <= first + k:
                return block[(a - first) * self.n:(b - first) * self.n]
        return torch.cat([self.get(key, i) for i in range(a, b)], 0)

    # the schedule is the host store's business
    def begin(self, schedule: Schedule) -> None:
        pass

    def step(self, i: int) -> None:
        pass

    def done(self, i: int) -> None:
        pass

    def prefetch_range(self, key: str, a: int, b: int) -> None:
        pass

    def finish(self) -> None:
        pass

    def nbytes(self) -> Dict[str, int]:
        """bytes resident per key, and their "total": what the store's own blocks hold"""
        out = {key: sum(int(b.numel()) * b.element_size() for _, _, b in blocks) for key, blocks in self._blocks.items()}
        out["total"] = sum(out.values())
        return out


class HostStore:
    """`cpu_cache`: frames in pinned host memory, a device window filled ahead of use.

    Every copy, in either direction, runs on ONE side stream.  Device -> host: the side stream waits for an event recorded on the
    compute stream behind the producer; the source is kept from reuse until the copy has run (`record_stream`).  Host -> device:
    the target is allocated on the compute stream, the side stream waits for an event recorded there at that moment (whatever
    used that memory before has finished), copies, and records the event the compute stream waits for at the tensor's first use.
    The host never synchronises: it enqueues step i + 1's copies when it enqueues step i's kernels.  Host memory is written and
    read back by the same stream, in order."""
    cache = "host"

    def __init__(self, n: int, t: int, device):
        self.n, self.t, self.device = int(n), int(t), device
        self.side = torch.cuda.Stream(device=device)
        self._host: Dict[str, Tensor] = {}                                # key -> pinned (frames, n, c, h, w)
        self._window: Dict[Tuple, List] = {}                              # (key, frame) or (key, (a, b)) -> [device tensor, event or None]
        self._schedule: Optional[Schedule] = None
        self.peak_window_items = 0

    def _main(self):
        return torch.cuda.current_stream(self.device)

    def _held_as(self, key: str, like: Tensor) -> torch.dtype:
        return like.dtype

    def _host_buffer(self, key: str, like: Tensor) -> Tensor:
        buf = self._host.get(key)
        if buf is None:
            frames = self.t - 1 if key in FLOW_KEYS else self.t
            buf = torch.empty((max(frames, 1), self.n) + tuple(like.shape[1:]), dtype=self._held_as(key, like), pin_memory=True)
            self._host[key] = buf
        return buf

    def put_range(self, key: str, first: int, frames: Tensor) -> None:
        k = int(frames.shape[0]) // self.n
        dst = self._host_buffer(key, frames)[first:first + k]
        ready = torch.cuda.Event()
        ready.record(self._main())
        self.side.wait_event(ready)
        with torch.cuda.stream(self.side):
            dst.view((k * self.n,) + tuple(frames.shape[1:])).copy_(frames, non_blocking=True)
        frames.record_stream(self.side)

    def new_branch(self, key: str, like: Tensor) -> None:
        self._host_buffer(key, like)

    def out_slot(self, key: str, idx: int) -> Optional[Tensor]:
        return None      # a fresh tensor per step; it leaves for the host once written

    def put(self, key: str, idx: int, frame: Tensor) -> None:
        self.put_range(key, idx, frame)

    def _fetch(self, entries) -> None:
        """entries: [(window key, host view)] -> device tensors, copied on the side stream"""
        entries = [(wk, src) for wk, src in entries if wk not in self._window]
        if not entries:
            return
        targets = [torch.empty(src.shape, dtype=src.dtype, device=self.device) for _, src in entries]
        free = torch.cuda.Event()
        free.record(self._main())
        self.side.wait_event(free)
        with torch.cuda.stream(self.side):
            for (wk, src), dev in zip(entries, targets):
                dev.copy_(src, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self.side)
                self._window[wk] = [dev, ev]
        self.peak_window_items = max(self.peak_window_items, len(self._window))

    def _take(self, wk) -> Tensor:
        entry = self._window[wk]
        if entry[1] is not None:
            self._main().wait_event(entry[1])
            entry[1] = None
        return entry[0]

    def _frame(self, item: Item):
        return item, self._host[item[0]][item[1]]

    def begin(self, schedule: Schedule) -> None:
        self._schedule = schedule
        self._fetch([self._frame(it) for it in schedule.prologue])

    def step(self, i: int) -> None:
        self._fetch([self._frame(it) for it in self._schedule.fetch[i]])

    def done(self, i: int) -> None:
        for it in self._schedule.evict[i]:
            self._window.pop(it, None)

    def get(self, key: str, idx: int) -> Tensor:
        return self._take((key, idx))

    def prefetch_range(self, key: str, a: int, b: int) -> None:
        src = self._host[key][a:b]
        self._fetch([((key, (a, b)), src.view(((b - a) * self.n,) + tuple(src.shape[2:])))])

    def get_range(self, key: str, a: int, b: int) -> Tensor:
        self.prefetch_range(key, a, b)
        out = self._take((key, (a, b)))
        del self._window[(key, (a, b))]
        return out

    def finish(self) -> None:
        """the compute stream waits for the side stream's last copy (the pinned buffers are about to be released)"""
        self._window.clear()
        last = torch.cuda.Event()
        last.record(self.side)
        self._main().wait_event(last)

    def nbytes(self) -> Dict[str, int]:
        """bytes resident per key, and their "total": the pinned buffers (the device window is not counted)"""
        out = {key: int(buf.numel()) * buf.element_size() for key, buf in self._host.items()}
        out["total"] = sum(out.values())
        return out


def _contiguous(x: Tensor) -> Tensor:
    return x if x.is_contiguous() else x.contiguous()


class DeviceStore16(_Census, DeviceStore):
    """The device cache with its features held in 16 bits: `HostStore` with "host" meaning 16-bit device memory and
    "copy" meaning a kernel.  A feature tensor (`is_feature_key`) is rounded to `dtype` when it is put (`ops.pack16`) and the step that
    produced it keeps its fp32 tensor in hand; reads follow the schedule as the host cache's do -- everything a time step fetches is
    widened into fp32 tensors by ONE `ops.unpack16` launch on the compute stream and dropped by `done`; `get_range` widens a range in
    one launch.  What comes back is `x.to(dtype).to(torch.float32)`, bit for bit.  Flows and LR frames stay fp32 and are served as
    `DeviceStore` serves them.  The hoisted predictors of a one-chunk run read every frame at once: this store keeps the per-step
    form (`hoists`).  census=True: every pack also counts what the rounding did, per key (`_Census`)."""
    hoists = False

    def __init__(self, n: int, t: int, device, dtype, census: bool = False):
        super().__init__(n, t, device)
        self.cache_dtype = check_cache_dtype(dtype)
        self.dtype = CACHE_DTYPES[self.cache_dtype]
        self._census_init(census, device)
        self._window: Dict[Tuple, Tensor] = {}      # (key, frame) -> fp32 tensor
        self._schedule: Optional[Schedule] = None
        self.peak_window_items = 0

    def _pack(self, src: Tensor, dst: Tensor) -> None:
        from . import ops
        ops.pack16([_contiguous(src)], [dst], self.dtype)

    def _pack_census(self, key: str, src: Tensor, dst: Tensor) -> None:
        from . import ops
        ops.pack16_census([_contiguous(src)], [dst], self.dtype, self._census_row(key, src))

    def put_range(self, key: str, first: int, frames: Tensor) -> None:
        if not is_feature_key(key):
            return super().put_range(key, first, frames)
        if (key, first) in self._where:      # rows of a branch's buffer
            block, j = self._where[(key, first)]
            dst = block[j * self.n:j * self.n + int(frames.shape[0])]
        else:
            dst = torch.empty(frames.shape, dtype=self.dtype, device=frames.device)
            super().put_range(key, first, dst)
        if self._counts is None:
            self._pack(frames, dst)
        else:
            self._pack_census(key, frames, dst)

    def new_branch(self, key: str, like: Tensor) -> None:
        super().put_range(key, 0, torch.empty((self.t * self.n,) + tuple(like.shape[1:]), dtype=self.dtype, device=like.device))

    def out_slot(self, key: str, idx: int) -> Optional[Tensor]:
        return None      # a fresh fp32 tensor per step: the step keeps it, `put` rounds it into the buffer

    def put(self, key: str, idx: int, frame: Tensor) -> None:
        self.put_range(key, idx, frame)

    def _held(self, item: Item) -> Tensor:
        return super().get(*item)

    def _fetch(self, items: Sequence[Item]) -> None:
        from . import ops
        items = [it for it in items if is_feature_key(it[0]) and it not in self._window]
        if not items:
            return
        srcs = [self._held(it) for it in items]
        dsts = [torch.empty(s.shape, dtype=torch.float32, device=s.device) for s in srcs]
        ops.unpack16(srcs, dsts)
        self._window.update(zip(items, dsts))
        self.peak_window_items = max(self.peak_window_items, len(self._window))

    def begin(self, schedule: Schedule) -> None:
        self._schedule = schedule
        self._fetch(schedule.prologue)

    def step(self, i: int) -> None:
        self._fetch(self._schedule.fetch[i])

    def done(self, i: int) -> None:
        for it in self._schedule.evict[i]:
            self._window.pop(it, None)

    def get(self, key: str, idx: int) -> Tensor:
        if not is_feature_key(key):
            return super().get(key, idx)
        return self._window[(key, idx)]

    def get_range(self, key: str, a: int, b: int) -> Tensor:
        if not is_feature_key(key):
            return super().get_range(key, a, b)
        from . import ops
        for first, k, block in self._blocks[key]:
            if first <= a and b <= first + k:
                srcs = [block[(a - first) * self.n:(b - first) * self.n]]
                break
        else:
            srcs = [self._held((key, i)) for i in range(a, b)]
        out = torch.empty((sum(int(s.shape[0]) for s in srcs),) + tuple(srcs[0].shape[1:]), dtype=torch.float32, device=srcs[0].device)
        rows, dsts = 0, []
        for s in srcs:
            dsts.append(out[rows:rows + int(s.shape[0])])
            rows += int(s.shape[0])
        ops.unpack16(srcs, dsts)
        return out

    def finish(self) -> None:
        self._window.clear()


class HostStore16(_Census, HostStore):
    """The host cache with its features held in 16 bits: the pinned buffers of the feature keys are 16-bit, half the bytes
    cross the link each way.  `put_range` rounds on the compute stream into a temporary 16-bit device tensor (`ops.pack16`) and copies
    that on the side stream; `_fetch` copies 16-bit frames into staging tensors and widens all of them with ONE `ops.unpack16` launch
    ON THE SIDE STREAM, and the event the compute stream waits on is recorded behind that launch.  Streams, events and
    `record_stream` as `HostStore`; the host never synchronises.  The same bits as `DeviceStore16`.  census=True: the device-side
    pack also counts what the rounding did, per key (`_Census`); the counts stay on the device until `census()` is called."""

    def __init__(self, n: int, t: int, device, dtype, census: bool = False):
        super().__init__(n, t, device)
        self.cache_dtype = check_cache_dtype(dtype)
        self.dtype = CACHE_DTYPES[self.cache_dtype]
        self._census_init(census, device)

    def _held_as(self, key: str, like: Tensor) -> torch.dtype:
        return self.dtype if is_feature_key(key) else like.dtype

    def put_range(self, key: str, first: int, frames: Tensor) -> None:
        if not is_feature_key(key):
            return super().put_range(key, first, frames)
        from . import ops
        k = int(frames.shape[0]) // self.n
        dst = self._host_buffer(key, frames)[first:first + k]
        packed = torch.empty(frames.shape, dtype=self.dtype, device=frames.device)
        if self._counts is None:
            ops.pack16([_contiguous(frames)], [packed], self.dtype)      # on the compute stream, behind the producer
        else:
            ops.pack16_census([_contiguous(frames)], [packed], self.dtype, self._census_row(key, frames))
        ready = torch.cuda.Event()
        ready.record(self._main())
        self.side.wait_event(ready)
        with torch.cuda.stream(self.side):
            dst.view((k * self.n,) + tuple(frames.shape[1:])).copy_(packed, non_blocking=True)
        packed.record_stream(self.side)

    def _fetch(self, entries) -> None:
        from . import ops
        entries = [(wk, src) for wk, src in entries if wk not in self._window]
        if not entries:
            return
        targets = [torch.empty(src.shape, dtype=torch.float32, device=self.device) for _, src in entries]
        free = torch.cuda.Event()
        free.record(self._main())
        self.side.wait_event(free)
        with torch.cuda.stream(self.side):
            staged, widened = [], []
            for (wk, src), dev in zip(entries, targets):
                if src.dtype == torch.float32:      # a flow, LR frames: today's copy and its own event
                    dev.copy_(src, non_blocking=True)
                    ev = torch.cuda.Event()
                    ev.record(self.side)
                    self._window[wk] = [dev, ev]
                else:      # (the staging tensor is allocated, written, read and released on the side stream alone)
                    stage = torch.empty(src.shape, dtype=src.dtype, device=self.device)
                    stage.copy_(src, non_blocking=True)
                    staged.append(stage)
                    widened.append((wk, dev))
            if staged:
                ops.unpack16(staged, [dev for _, dev in widened])
                ev = torch.cuda.Event()
                ev.record(self.side)
                for wk, dev in widened:
                    self._window[wk] = [dev, ev]
        self.peak_window_items = max(self.peak_window_items, len(self._window))


def make_store(cache: str, n: int, t: int, device, dtype=None, *, census=False):
    """dtype=None: the fp32 stores.  "fp16" / "bf16" (`check_cache_dtype`): the stores that hold the feature keys in 16 bits.
    census=True (a 16-bit store only: the fp32 stores round nothing and take no census): the store counts what its packs did,
    `store.census()`.  census=False: every launch is the one it was."""
    host = check_cache(cache) == "host"
    if check_cache_dtype(dtype) is None:
        if census:
            raise ValueError("make_store: census=True without a 16-bit dtype: the fp32 stores round nothing")
        return (HostStore if host else DeviceStore)(n, t, device)
    if not census:
        return (HostStore16 if host else DeviceStore16)(n, t, device, dtype)
    return (HostStore16 if host else DeviceStore16)(n, t, device, dtype, census=True)
