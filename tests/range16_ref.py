"""The range census of the 16-bit backbone (addendum) in numpy, one line per slot and flavour.  `words`: a stored 16-bit
word o, whose fp32 bits u are its exact widening.  `as_rounded`: an fp32 value about to be rounded -- tests/census_ref.py's census,
imported as it is."""
import numpy as np

from tests import census_ref

SLOTS = census_ref.SLOTS
FORMAT_MAX = {"fp16": 65504.0, "bf16": float.fromhex("0x1.fep127")}


def widen(o16: np.ndarray, dtype) -> np.ndarray:
    """the exact fp32 value of every 16-bit word"""
    o16 = np.ascontiguousarray(o16, dtype=np.uint16).reshape(-1)
    if census_ref.is_bf16(dtype):
        return (o16.astype(np.uint32) << 16).view(np.float32)
    return o16.view(np.float16).astype(np.float32)


def words(o16: np.ndarray, dtype) -> dict:
    """the record of `ops.range16_words` over the words o16 (uint16)"""
    o = np.ascontiguousarray(o16, dtype=np.uint16).reshape(-1).astype(np.uint32)
    bf = census_ref.is_bf16(dtype)
    r = o & 0x7FFF
    finite = r < (0x7F80 if bf else 0x7C00)
    x = np.abs(widen(o16, dtype))
    return {"elements": int(o.size),
            "max_abs": float(x[finite].max()) if finite.any() else 0.0,          # the largest finite stored value
            "nonfinite": int(np.count_nonzero(~finite)),                          # inf / NaN words
            "overflow": 0,                                                        # by construction: a finite u widens from a finite o
            "flushed": 0,                                                         # by construction: u != 0 exactly where r != 0
            "subnormal": int(np.count_nonzero((r > 0) & (r < (0x0080 if bf else 0x0400))))}


def as_rounded(x32: np.ndarray, dtype) -> dict:
    """the record of `ops.range16_as_rounded`: `pack16_census`'s"""
    return census_ref.census(x32, dtype)


def headroom(max_abs: float, dtype) -> float:
    return float("inf") if max_abs == 0.0 else FORMAT_MAX["bf16" if census_ref.is_bf16(dtype) else "fp16"] / max_abs


add, row = census_ref.add, census_ref.row


# ---- the kernel's address arithmetic (csrc/range16.hip: cut_of, scalar_index), transcribed: tests/test_range16_host.py holds it to
# numpy slicing
def range16_cut(misalign: int, n: int, per_vector: int):
    """(head, vectors, tail) of a segment of n elements that starts `misalign` elements (0 .. per_vector - 1) past a 16-byte boundary
    -- csrc/range16.hip's cut_of; per_vector: 8 (16-bit words) or 4 (fp32 values)"""
    if per_vector not in (4, 8) or not 0 <= misalign < per_vector or n < 0:
        raise ValueError(f"range16_cut: misalignment {misalign} of {per_vector} elements per vector, {n} elements")
    head = min((per_vector - misalign) & (per_vector - 1), n)
    nvec = (n - head) // per_vector
    return head, nvec, n - head - per_vector * nvec


def range16_item(i: int, head: int, nvec: int, tail: int, per_vector: int):
    """the elements [a, b) of its segment that item i of the kernel reads: the vectors first, then the head's and the tail's elements"""
    if i < nvec:
        return head + per_vector * i, head + per_vector * (i + 1)
    j = i - nvec
    if j >= head + tail:
        return 0, 0
    e = j if j < head else j + per_vector * nvec
    return e, e + 1
