"""The helper behind tests/test_hip_large_extents.py, on the CPU with the boundaries shrunk by 2^16 (2^15 elements, 2^16 bytes,
2^16 elements): it passes a correct op, it fails on stand-ins whose flat index wraps, and it picks the straddling images.
This is what shows that the GPU file would notice a 32-bit wrap."""
import pytest
import torch

from tests import large_extents as L

SMALL = {"elem31": ("elements", 2 ** 15), "byte32": ("bytes", 2 ** 16), "elem32": ("elements", 2 ** 16)}
ALL3 = ("elem31", "byte32", "elem32")


def _input(n, per):
    return L.fill_chunks(torch.empty(n, per), lambda t, g: t.normal_(generator=g), seed=7, chunk=5)


def _correct(x):
    return x * 2.0 + 1.0


def _wrapped(bits, frm, what="both"):
    """a "kernel" whose flat element index is computed in `bits` bits once it reaches `frm`: the read index, the write index or
    both land at i mod 2^bits"""
    def op(x):
        flat = x.reshape(-1)
        out = torch.full_like(flat, -77.0)             # what no thread wrote
        i = torch.arange(flat.numel())
        j = torch.where(i >= frm, i & ((1 << bits) - 1), i)
        rd, wr = (j if what in ("both", "read") else i), (j if what in ("both", "write") else i)
        for lo in range(0, flat.numel(), 1 << bits):      # in index order, so a wrapped write lands AFTER the right one
            k = slice(lo, lo + (1 << bits))
            out[wr[k]] = flat[rd[k]] * 2.0 + 1.0
        return out.view_as(x)
    return op


def _check(op, n=90, per=1000, must=ALL3, **kw):
    x = _input(n, per)
    return L.check_extents("standin", lambda lo, hi: op(x[lo:hi]), lambda i: x[i].double() * 2.0 + 1.0, n, chunk=7,
                           must_cross=must, limits=SMALL, **kw)


def test_a_correct_op_passes_and_the_report_names_the_extent():
    rep = _check(_correct)
    assert rep["elements"] == 90000 and rep["bytes"] == 360000 and all(rep["crossed"].values())
    assert rep["images"] == {"first": 0, "elem31": 32, "byte32": 16, "elem32": 65, "last": 89}


@pytest.mark.parametrize("what", ["both", "read", "write"])
@pytest.mark.parametrize("bits,frm", [(16, 2 ** 16), (15, 2 ** 15), (14, 2 ** 14)], ids=["u32-index", "s32-index", "u32-byte-offset"])
def test_a_wrapped_flat_index_is_caught_by_both_checks(bits, frm, what):
    """a wrapped read leaves every element written, with another element's value; a wrapped write leaves the elements past the
    boundary unwritten and overwrites low ones"""
    with pytest.raises(AssertionError, match="differs from its reference"):       # check A, at a boundary image
        _check(_wrapped(bits, frm, what), whole_vs_chunk=False)
    x = _input(90, 1000)
    with pytest.raises(AssertionError, match="differ from the run over"):          # check B alone (a reference that agrees with the op)
        whole = _wrapped(bits, frm, what)(x)
        L.check_extents("standin", lambda lo, hi: _wrapped(bits, frm, what)(x[lo:hi]), lambda i: whole[i], 90, chunk=7, limits=SMALL,
                        must_cross=ALL3)


def test_check_b_sees_an_image_that_is_at_no_boundary():
    def op(x):
        y = _correct(x)
        if x.shape[0] == 90:
            y[50, 123] += 1e-3      # only the whole-tensor run, only image 50
        return y
    with pytest.raises(AssertionError, match=r"images \[50\]"):
        _check(op)
    _check(op, whole_vs_chunk=False)      # ... which check A alone does not look at


def test_an_extent_that_does_not_cross_is_an_error_not_a_pass():
    with pytest.raises(AssertionError):
        _check(_correct, n=60)            # 60 000 elements < 2^16
    _check(_correct, n=60, must=("elem31", "byte32"))


def test_tolerance_rule_and_kernel_name_comparison():
    x = _input(40, 1000)
    ref = lambda i: x[i].double() * 2.0 + 1.0
    L.check_extents("tol", lambda lo, hi: _correct(x[lo:hi]) + 1e-6, ref, 40, chunk=8, compare=L.within(2e-5), limits=SMALL)
    with pytest.raises(AssertionError, match="image 0"):
        L.check_extents("tol", lambda lo, hi: _correct(x[lo:hi]) + 1e-3, ref, 40, chunk=8, compare=L.within(2e-5), limits=SMALL)
    with pytest.raises(AssertionError, match="image 0"):      # |ref| reaches ~9: 2e-5 absolute is the tighter rule
        L.check_extents("tol", lambda lo, hi: _correct(x[lo:hi]) + 5e-5, ref, 40, chunk=8, compare=L.within(2e-5, absolute=True), limits=SMALL)
    L.check_extents("tol", lambda lo, hi: _correct(x[lo:hi]) + 5e-5, ref, 40, chunk=8, compare=L.within(2e-5), limits=SMALL)
    # an op with two results, one rule each
    two = lambda lo, hi: (_correct(x[lo:hi]), x[lo:hi].sum(1))
    ref2 = lambda i: (ref(i), x[i].double().sum())
    L.check_extents("two", two, ref2, 40, chunk=8, compare=(L.equal, L.within(1e-5)), limits=SMALL)
    with pytest.raises(AssertionError, match="image 0"):
        L.check_extents("two", two, lambda i: (ref(i), x[i].double().sum() + 1.0), 40, chunk=8, compare=(L.equal, L.within(1e-5)), limits=SMALL)

    class Prof:          # stands for ops.profile(): the whole run "launches" another kernel than the chunks
        def __init__(self):
            self.names = []

        def __enter__(self):
            return self

        def __exit__(self, *a):
            pass

        def summary(self):
            return {n: {} for n in self.names}
    made = []

    def profile():
        made.append(Prof())
        return made[-1]

    def run(lo, hi):
        made[-1].names.append("big" if hi - lo == 40 else "small")
        return _correct(x[lo:hi])
    with pytest.raises(AssertionError, match="big"):
        L.check_extents("names", run, ref, 40, chunk=8, limits=SMALL, profile=profile)


def test_boundary_chooser_returns_the_straddling_images():
    # fp32 images of 1000 elements: byte 2^16 = element 16384 is in image 16, element 2^15 in image 32, element 2^16 in image 65
    assert L.boundary_images(90, 1000, 4, SMALL) == {"first": 0, "elem31": 32, "byte32": 16, "elem32": 65, "last": 89}
    # 1-byte elements: byte 2^16 is element 2^16
    assert L.boundary_images(90, 1000, 1, SMALL) == {"first": 0, "elem31": 32, "byte32": 65, "elem32": 65, "last": 89}
    # a boundary between two images names both; one outside the tensor is left out
    assert L.boundary_images(40, 1024, 4, SMALL) == {"first": 0, "elem31": 32, "elem31-": 31, "byte32": 16, "byte32-": 15, "last": 39}
    assert L.crossed(40, 1024, 4, SMALL) == {"elem31": True, "byte32": True, "elem32": False}
    # the real boundaries: 2740 images of 64 x 96 x 128 fp32
    per = 64 * 96 * 128
    idx = L.boundary_images(2740, per, 4)
    assert idx["elem31"] == 2 ** 31 // per and idx["byte32"] == 2 ** 30 // per and "elem32" not in idx
    lo = idx["elem31"] * per
    assert lo <= 2 ** 31 < lo + per
