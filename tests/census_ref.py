"""The census of the 16-bit feature cache (addendum) in numpy: the 16-bit result of every element -- fp16 from
`x.astype(np.float16)`, bf16 from the integer formula in csrc/cache16.hip's header comment -- and the five counts, each a function
of an element's fp32 bits u and its 16-bit result o alone."""
import numpy as np

SLOTS = ("max_abs", "nonfinite", "overflow", "flushed", "subnormal")

# hand-built fp32 bit patterns at the edges of both formats (tests/test_census_host.py pins what each becomes)
F16_MAX_IN = 0x477FEFFF          # the largest float that rounds to 65504
F16_INF_IN = 0x477FF000          # 65520: the smallest that rounds to inf
F16_ZERO_IN = 0x33000000         # 2^-25: the tie between 0 and the smallest subnormal, to even: 0
F16_TINY_IN = 0x33000001         # the next float up: 2^-24, the smallest subnormal
F16_NORMAL_IN = 0x38800000       # 2^-14: the smallest normal
F16_BELOW_NORMAL_IN = 0x387FFFFF  # the float below it
BF16_MAX_IN = 0x7F7F7FFF         # the largest float that stays finite in bf16
BF16_INF_IN = 0x7F7F8000         # the tie that rounds to even: inf
SPECIALS = (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000)      # +-0, +-inf, a NaN
BOUNDARY_BITS = (F16_MAX_IN, F16_INF_IN, F16_ZERO_IN, F16_TINY_IN, F16_NORMAL_IN, F16_BELOW_NORMAL_IN, BF16_MAX_IN, BF16_INF_IN) + SPECIALS
BOUNDARY_BITS = BOUNDARY_BITS + tuple(b | 0x80000000 for b in BOUNDARY_BITS[:8])      # and their negatives
# bf16's small end: fp32 subnormals that are flushed (the second one a tie, to even), the smallest that is not, the largest bf16
# subnormal's upper neighbour (rounds down to it) and the tie that rounds up to the smallest normal
BF16_TINY_BITS = (0x00000001, 0x00008000, 0x00008001, 0x007F7FFF, 0x007F8000)


def is_bf16(dtype) -> bool:
    name = str(dtype)
    if name in ("bf16", "torch.bfloat16"):
        return True
    if name in ("fp16", "torch.float16"):
        return False
    raise ValueError(f"census_ref: dtype {dtype!r}")


def round16(x32: np.ndarray, dtype) -> np.ndarray:
    """the 16-bit result of every element, as uint16"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).reshape(-1)
    u = x32.view(np.uint32)
    if not is_bf16(dtype):
        with np.errstate(over="ignore"):
            return x32.astype(np.float16).view(np.uint16)
    o = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)      # nearest even; the carry is the overflow to inf
    o[(u & 0x7FFFFFFF) > 0x7F800000] = 0x7FC0                                          # NaN: torch's
    return o


def census(x32: np.ndarray, dtype) -> dict:
    """{'elements', 'max_abs' (a Python float), 'nonfinite', 'overflow', 'flushed', 'subnormal'} of rounding x32 to `dtype`"""
    x32 = np.ascontiguousarray(x32, dtype=np.float32).reshape(-1)
    u = x32.view(np.uint32)
    o = round16(x32, dtype).astype(np.uint32)
    bf = is_bf16(dtype)
    a, r = u & 0x7FFFFFFF, o & 0x7FFF
    finite = a < 0x7F800000
    top = np.uint32(a[finite].max() if finite.any() else 0)
    return {"elements": int(x32.size),
            "max_abs": float(np.array([top], np.uint32).view(np.float32)[0]),
            "nonfinite": int(np.count_nonzero(~finite)),
            "overflow": int(np.count_nonzero(finite & (r == (0x7F80 if bf else 0x7C00)))),
            "flushed": int(np.count_nonzero(finite & (a != 0) & (r == 0))),
            "subnormal": int(np.count_nonzero((r > 0) & (r < (0x0080 if bf else 0x0400))))}


def add(*records) -> dict:
    """the census of several tensors put under one key: what launches that share a record accumulate"""
    out = {"elements": 0, "max_abs": 0.0, "nonfinite": 0, "overflow": 0, "flushed": 0, "subnormal": 0}
    for r in records:
        out["max_abs"] = max(out["max_abs"], r["max_abs"])
        for k in ("elements", "nonfinite", "overflow", "flushed", "subnormal"):
            out[k] += r[k]
    return out


def row(record: dict) -> list:
    """the five integers of the device's record"""
    return [int(np.array([record["max_abs"]], np.float32).view(np.uint32)[0])] + [record[k] for k in SLOTS[1:]]
