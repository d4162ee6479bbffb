"""Helper of tests/test_hip_large_extents.py: run one batched op on a tensor whose flat extent passes the 32-bit boundaries and
check it twice -- (A) the images at the boundaries against an independent high-precision reference of those images alone,
(B) every image, bit for bit, against the same op run chunk by chunk.  Device-agnostic (tests/test_large_extents_host.py drives
it with torch CPU ops and shrunken boundaries, and shows that it catches a wrapped flat index).

Boundaries, as (name, unit, value): the flat ELEMENT index 2^31 (a signed 32-bit index), the flat BYTE offset 2^32 (an unsigned
32-bit byte offset) and the flat element index 2^32 (an unsigned 32-bit index)."""
from __future__ import annotations

import contextlib
from typing import Callable, Dict, Optional, Sequence

import torch

LIMITS = {"elem31": ("elements", 2 ** 31), "byte32": ("bytes", 2 ** 32), "elem32": ("elements", 2 ** 32)}


def crossed(n: int, per_image: int, itemsize: int, limits=LIMITS) -> Dict[str, bool]:
    """which boundaries lie strictly inside a contiguous (n, per_image) tensor of `itemsize`-byte elements"""
    total = n * per_image
    return {k: (total > v if unit == "elements" else total * itemsize > v) for k, (unit, v) in limits.items()}


def boundary_images(n: int, per_image: int, itemsize: int, limits=LIMITS) -> Dict[str, int]:
    """{"first": 0, "<boundary>": the image that holds the first element at or past that boundary and -- when the boundary falls
    between two images -- "<boundary>-": the image that ends there, "last": n - 1}; boundaries outside the tensor are left out"""
    out = {"first": 0}
    for k, (unit, v) in limits.items():
        elem = v if unit == "elements" else -(-v // itemsize)      # the first element at or past the boundary
        if elem >= n * per_image:
            continue
        out[k] = elem // per_image
        if elem % per_image == 0 and elem > 0:
            out[k + "-"] = elem // per_image - 1
    out["last"] = n - 1
    return out


def fill_chunks(t: torch.Tensor, fill: Callable[[torch.Tensor, torch.Generator], None], seed: int, chunk: int) -> torch.Tensor:
    """fill t[i:i + chunk] in place, chunk after chunk, from one seeded generator on t's device (no host copy of the whole)"""
    g = torch.Generator(device=t.device).manual_seed(seed)
    for lo in range(0, t.shape[0], chunk):
        fill(t[lo:lo + chunk], g)
    return t


# the comparison rules of check A: compare(got, want, what) asserts and returns the error it measured
def equal(got: torch.Tensor, want: torch.Tensor, what: str) -> float:
    """torch.equal after the cast of the reference to the result's dtype"""
    assert torch.equal(got, want.to(got.dtype)), f"{what} differs from its reference"
    return 0.0


def within(tol: float, absolute: bool = False, extra: float = 0.0):
    """max|got - ref| <= tol * max(1, max|ref|) + extra (absolute=True: <= tol)"""
    def compare(got, want, what):
        err = (got.double() - want.double()).abs().max().item()
        bound = tol if absolute else tol * max(1.0, want.abs().max().item()) + extra
        print(f"{what}: max|got - ref| {err:.3e} bound {bound:.3e}")
        assert err <= bound, f"{what}: {err:.3e} > {bound:.3e}"
        return err
    compare.rule = f"{tol:g}" + ("" if absolute else " max(1, |ref|max)") + (f" + {extra:g}" if extra else "")
    return compare


def _tuple(v):
    return v if isinstance(v, tuple) else (v,)


def check_extents(label: str, run: Callable, ref: Callable, n: int, chunk: int, compare=equal,
                  must_cross: Sequence[str] = ("elem31", "byte32"), extent_of=None, images: Optional[Dict[str, int]] = None,
                  whole_vs_chunk: bool = True, profile=None, route=None, limits=LIMITS) -> dict:
    """run(lo, hi): the op on images [lo, hi) -> a tensor (or a tuple of tensors) with hi - lo leading entries (0, n: the whole
    tensor, one call).  ref(i): the reference of image i alone, CPU tensor(s) (float64 for inexact ops).  compare: one rule
    (`equal`, `within(..)`, or any callable of that form), or one per output.  extent_of: the operand whose extent must pass
    `must_cross` -- a tensor, or a callable evaluated after the whole run (default: the first result).  images: the images check
    A looks at (default: the boundary images of the first result and of `extent_of`).  profile / route: ops.profile and
    ops.route_batch on the GPU, None on the host; every run is made under route(n), and the chunks must launch the kernel names
    the whole run launched.  Returns the figures a report needs."""
    route = route or (lambda _n: contextlib.nullcontext())
    profile = profile or (lambda: contextlib.nullcontext())
    names_of = lambda prof: None if prof is None else sorted(prof.summary())
    with route(n), profile() as prof:
        whole = _tuple(run(0, n))
    names = names_of(prof)
    assert all(w.shape[0] == n for w in whole), ([w.shape for w in whole], n)
    rules = list(compare) if isinstance(compare, (tuple, list)) else [compare] * len(whole)
    big = whole[0] if extent_of is None else extent_of() if callable(extent_of) else extent_of
    per, item = big[0].numel(), big.element_size()
    cross = crossed(big.shape[0], per, item, limits)
    assert big.is_contiguous() and all(cross[k] for k in must_cross), (label, tuple(big.shape), cross)
    if images is None:
        images = boundary_images(n, whole[0][0].numel(), whole[0].element_size(), limits)
        if big is not whole[0] and big.shape[0] == n:
            for k, v in boundary_images(n, per, item, limits).items():
                images.setdefault("in:" + k, v)
    report = {"op": label, "shape": list(big.shape), "elements": big.numel(), "bytes": big.numel() * item, "crossed": cross,
              "kernels": names, "rule": [getattr(r, "rule", r.__name__) for r in rules], "images": images, "err": {}}
    for name, i in images.items():
        wants = _tuple(ref(i))
        report["err"][name] = max(rule(w[i].cpu(), want, f"{label}: image {i} ({name})") for rule, w, want in zip(rules, whole, wants))
    if whole_vs_chunk:
        chunk_names = set()
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            with route(n), profile() as prof:
                parts = _tuple(run(lo, hi))
            chunk_names.update(names_of(prof) or [])
            for part, w in zip(parts, whole):
                if not torch.equal(part, w[lo:hi]):
                    bad = (part != w[lo:hi]).reshape(hi - lo, -1).any(1).nonzero().flatten()
                    raise AssertionError(f"{label}: images {[lo + int(b) for b in bad[:8]]} of the whole-tensor run differ from the "
                                         f"run over [{lo}, {hi})")
            del parts
        if names is not None:
            assert sorted(chunk_names) == names, (label, names, sorted(chunk_names))
    print("large-extent report:", report)
    return report
