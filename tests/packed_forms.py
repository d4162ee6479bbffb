"""Helper of tests/test_hip_packed_forms.py: every packed weight form of eavsr_amd.ops, reached through its `_packed_*` name only,
with what a first call does pinned in tests/golden/packed_forms.json.  Not a test file.

A case is a `_packed_*` function, seeded fp32 weights at the shapes part (c) of tests/test_hip_stream_order.py uses for the same
cache, and keyword arguments: for the list-taking forms one two-weight list, for the bf16-split conv forms `dgrad=True`, for the
coded forms both codes (1 fp16, 2 bf16).  `observe` wraps a recording proxy around the real library for one first call and returns
  * log:    the library entry points in call order with their scalar arguments (the device pointers and the stream left out),
  * packed: dtype and element count of each tensor of the value,
  * grew:   the caches that gained an entry and the tag it went under,
  * bytes:  the sha256 of the packed bytes,
and then asserts nothing itself: the test compares them with the recording.

`python -m tests.packed_forms --record` writes the recording (run on the tree whose behaviour is to be kept).  A pack kernel may
leave padding unwritten and torch.empty does not clear it, so the recorder packs every case twice, each time right after a buffer
of the value's dtype and size was filled with 0x00 / 0xFF bytes and freed: a case whose two digests differ is stored with
"bytes": null and a note, and is compared by its log only.  `--lab` records the lab-only cases (Winograd F(2x2,3x3)) into the same
file, with the lab library loaded."""
from __future__ import annotations

import hashlib
import json
import os
import sys
from typing import Dict, List, NamedTuple, Tuple

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_forms.json")
MAX_NULL_FRACTION = 0.25      # at most a quarter of the cases may go without a digest


class Case(NamedTuple):
    id: str
    fn: str                     # the name in eavsr_amd.ops
    shapes: Tuple[tuple, ...]   # one fp32 tensor each, seeded by the case's position
    listed: bool                # the tensors go in as ONE list argument (else one positional argument each)
    kw: Tuple[tuple, ...]
    lab: bool = False


def _c(id, fn, *shapes, listed=False, lab=False, **kw):
    return Case(id, fn, tuple(shapes), listed, tuple(sorted(kw.items())), lab)


C64, HEADS = (64, 64, 3, 3), ((4, 64, 3, 3), (2, 64, 3, 3))
CASES: List[Case] = [
    _c("f32_direct_2src", "_packed_f32", (64, 128, 3, 3), listed=True), _c("f32_1x1", "_packed_f32", (64, 192, 1, 1), listed=True),
    _c("f32_ragged", "_packed_f32", (24, 16, 3, 3), listed=True), _c("f32_7x7", "_packed_f32", (32, 8, 7, 7), listed=True),
    _c("f32_list", "_packed_f32", *HEADS, listed=True),
    _c("smallco", "_packed_smallco", (3, 64, 3, 3), listed=True), _c("smallco_list", "_packed_smallco", *HEADS, listed=True),
    _c("x6_3x3", "_packed_conv_x6", C64, listed=True), _c("x6_3x3_dgrad", "_packed_conv_x6", C64, listed=True, dgrad=True),
    _c("x6_5x5", "_packed_conv_x6", (40, 16, 5, 5), listed=True), _c("x6_7x7", "_packed_conv_x6", (32, 8, 7, 7), listed=True),
    _c("x6_list", "_packed_conv_x6", (24, 16, 5, 5), (16, 16, 5, 5), listed=True),
    _c("bf16", "_packed_conv3_bf16", C64, listed=True), _c("bf16_dgrad", "_packed_conv3_bf16", C64, listed=True, dgrad=True),
    _c("bf16_list", "_packed_conv3_bf16", (32, 64, 3, 3), (32, 64, 3, 3), listed=True),
    _c("h16g_fp16", "_packed_h16g", C64, listed=True, code=1), _c("h16g_bf16", "_packed_h16g", C64, listed=True, code=2),
    _c("h16g_list", "_packed_h16g", (32, 64, 3, 3), (32, 64, 3, 3), listed=True, code=2),
    _c("h16x1_fp16", "_packed_h16x1", (32, 8, 7, 7), listed=True, code=1), _c("h16x1_bf16", "_packed_h16x1", (32, 8, 7, 7), listed=True, code=2),
    _c("h16x1_list", "_packed_h16x1", (16, 8, 7, 7), (16, 8, 7, 7), listed=True, code=1),
    _c("dcn_il2", "_packed_dcn_il2", C64), _c("dcn_il2_16to32", "_packed_dcn_il2", (32, 16, 3, 3)),
    _c("il16_fp16", "_packed_il16", C64, code=1), _c("il16_bf16", "_packed_il16", C64, code=2),
    _c("x9", "_packed_x9", C64, listed=True), _c("x9_list", "_packed_x9", (32, 64, 3, 3), (32, 64, 3, 3), listed=True),
    _c("dcn_x9", "_packed_dcn_x9", C64),
    _c("wino_f4", "_packed_wino", C64, listed=True, four=True), _c("wino_f4_2src", "_packed_wino", (40, 24, 3, 3), listed=True, four=True),
    _c("wino_f4_kind", "_packed_wino", C64, listed=True, kind="f4"), _c("wino_f5", "_packed_wino", (40, 16, 5, 5), listed=True, kind="f5"),
    _c("wino_f4_list", "_packed_wino", (16, 24, 3, 3), (24, 24, 3, 3), listed=True, four=True),
    _c("wino_f2", "_packed_wino", C64, listed=True, lab=True), _c("wino_f2_list", "_packed_wino", (16, 24, 3, 3), (24, 24, 3, 3), listed=True, lab=True),
    _c("lpips_5x5", "_packed_lpips_conv", (192, 64, 5, 5)), _c("lpips_11x11", "_packed_lpips_conv", (64, 3, 11, 11)),
    _c("h16_fp16", "_packed_h16", C64, code=1), _c("h16_bf16", "_packed_h16", C64, code=2),
    _c("h16_ps2_fp16", "_packed_h16_ps2", (256, 64, 3, 3), (256,), code=1), _c("h16_ps2_bf16", "_packed_h16_ps2", (256, 64, 3, 3), (256,), code=2),
    _c("h16_5x5_fp16", "_packed5_h16", (120, 64, 5, 5), code=1), _c("h16_5x5_bf16", "_packed5_h16", (120, 64, 5, 5), code=2),
    _c("pwc", "_packed_pwc_conv3x3", (8, 6, 3, 3)), _c("pwc_first", "_packed_pwc_conv3x3", (16, 3, 3, 3)),
]
BY_ID: Dict[str, Case] = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def weights_of(case: Case, device) -> List[torch.Tensor]:
    """fresh tensor objects (a miss in every cache), the same values at every call"""
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    return [(torch.randn(*s, generator=g) * 0.05).to(device) for s in case.shapes]


def call(ops, case: Case, ws):
    fn = getattr(ops, case.fn)
    return fn(list(ws), **dict(case.kw)) if case.listed else fn(*ws, **dict(case.kw))


class _Recorder:
    """stands in for ops.lib(): every entry point asked for is the real one, its call logged"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def logged(*args):
            pack = "pack_" in name      # (pointer, pointer, scalars.., stream); the size functions take scalars only
            self._log.append([name, [int(a) for a in (args[2:-1] if pack else args)]])
            return fn(*args)
        return logged


def _tensors(value):
    return [v for v in (value if isinstance(value, (tuple, list)) else (value,)) if v is not None]


def _cache_names(ops):
    from eavsr_amd import weight_cache
    return {id(v): k for k, v in vars(ops).items() if isinstance(v, weight_cache.WeightCache)}


def observe(ops, case: Case, ws, before=None):
    """One call of the case with the library recorded -> (what it did, the value).  `before()` runs after the weights exist and
    before the call (the recorder poisons the allocator's free memory there)."""
    names = _cache_names(ops)
    caches = [c for c in ops.WEIGHT_CACHES if id(c) in names]
    had = {id(c): set(c.snapshot()) for c in caches}
    if before is not None:
        before()
    log, real = [], ops.lib
    ops.lib = lambda: _Recorder(real(), log)
    try:
        value = call(ops, case, ws)
    finally:
        ops.lib = real
    grew = sorted([names[id(c)], key[0]] for c in caches for key in set(c.snapshot()) - had[id(c)])
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in _tensors(value):
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    seen = {"log": log, "packed": [[str(t.dtype), t.numel()] for t in _tensors(value)], "grew": json.loads(json.dumps(grew)),
            "bytes": h.hexdigest()}
    return seen, value


def golden() -> dict:
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def _poison(like, byte):
    def fill():
        for t in like:
            torch.empty(t.numel() * t.element_size(), device=t.device, dtype=torch.uint8).fill_(byte)
        torch.cuda.synchronize()      # (the buffers are free again here: the next torch.empty of that size gets their memory)
    return fill


def record(lab: bool) -> None:
    from eavsr_amd import ops
    assert ops.lab_available() == lab, "--lab goes with the lab library (EAVSR_BUILD_LAB=1), and only with it"
    dev = torch.device("cuda:0")
    out = {}
    if lab:
        with open(GOLDEN) as f:
            out = json.load(f)["cases"]
    for case in [c for c in CASES if c.lab == lab]:
        _, first = observe(ops, case, weights_of(case, dev))
        like = [torch.empty_like(t) for t in _tensors(first)]
        del first
        seen = []
        for byte in (0x00, 0xFF):
            for c in ops.WEIGHT_CACHES:
                c.clear()
            seen.append(observe(ops, case, weights_of(case, dev), _poison(like, byte))[0])
        entry = seen[0]
        assert seen[1]["log"] == entry["log"] and seen[1]["packed"] == entry["packed"] and seen[1]["grew"] == entry["grew"], case.id
        if seen[1]["bytes"] != entry["bytes"]:
            entry["bytes"] = None
            entry["note"] = "the digest follows what the buffer held before: the pack kernel leaves part of it unwritten"
        out[case.id] = entry
        print(f"{case.id}: {entry['log']} {entry['packed']} {entry['grew']} {entry['bytes']}")
    nulls = sorted(k for k, v in out.items() if v["bytes"] is None)
    print(f"{len(out)} cases, {len(nulls)} without a digest: {nulls}")
    with open(GOLDEN, "w") as f:
        json.dump({"what": "tests/packed_forms.py --record", "cases": out}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if "--record" not in sys.argv[1:]:
        sys.exit("usage: python -m tests.packed_forms --record [--lab]")
    record("--lab" in sys.argv[1:])
