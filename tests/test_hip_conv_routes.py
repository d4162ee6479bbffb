"""ops.conv2d's router: every case of tests/conv_routes.py's matrix launches the kernels `predict_route` names (the list
`ops.profile` records, in order) and returns what the float64 `reference` gives, within the bound the project's per-kernel tests
assert for the kernel family that ran.  Groups: A the launch-size gates from both sides, B every option on every route and its
fallback form on the others (the combinations the docstring rules out raise before any launch), C pointers 4 / 8 / 12 bytes past a
16-byte boundary, D one batch run whole and row by row under ops.route_batch, E degenerate sizes, F the 16-bit modes' routing."""
import pytest
import torch

from tests import conv_routes as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    _ops.lib()
    state = lambda: (_ops.WINO_MIN_TILES, _ops.X6S_MAX_TILES, _ops.CONV3_SMALL, _ops.CONV_MODE, _ops.CONV5_MODE, _ops.CONV7_MODE,
                     _ops.CONV3_H16, _ops._ROUTE_BATCH)
    before = state()
    yield _ops
    assert state() == before, "a test of this file left a threshold, a mode or a pinned route batch behind"


# max|got - ref64| <= tol * max(1, |ref64|max), per kernel family, from the per-kernel tests of tests/test_hip_ops.py (test_hip_h16.py):
CONV_TOL = {
    "direct": 2e-5, "direct_ca": 2e-5,          # test_conv2d_vs_torch_cpu (the fused prologue: test_conv3x3_fused_channel_attention_prologue)
    "smallco_lite": 2e-5, "smallco_classic": 2e-5,      # test_conv3x3_small_cout_co_resident_variant
    "x6s": 3e-6,                                # test_conv3x3_small_launches_bf16x6_matches_fp64_and_the_fp32_kernel (e6)
    "x6": 3e-6,                                 # test_conv5x5_bf16x6_matches_fp64_and_winograd / test_conv7x7_bf16x6_... (e6)
    "wino4": 3e-5, "wino4_ca": 3e-5,            # test_conv3x3_winograd4_error_against_fp64_and_fallbacks (e4)
    "wino5": 3e-5,                              # test_conv5x5_winograd_vs_torch_cpu
    "h16g": 3e-5, "h16x1": 3e-5,                # test_conv3x3_h16g_vs_fp64_on_rounded_inputs / test_conv7x7_h16x1_... (rounded operands)
    "wino": 2e-5, "wino_ca": 2e-5, "x9": 2e-5,  # test_conv3x3_winograd_vs_torch_cpu / test_conv3x3_bf16x9_vs_torch_cpu (lab)
}
BF16_BOUND = 2e-6       # test_hip_train_bf16.py CONV_BOUND: max|got - ref of the bf16-rounded operands| / max S (tests/train_bf16_refs.py)


def _sums_bound(fam, ref, case):
    """the bound the same tests put on the per-tile channel sums, added up over the tile axis"""
    s = ref["sums"].abs().max().item()
    if fam == "x6s":
        return 2e-5 * max(1.0, s)
    if fam == "bf16s":      # test_conv_training_epilogues_and_dgrad_form
        return BF16_BOUND * ref["S"].sum((2, 3)).max().item() + 1e-6 * ref["abs_sums"].max().item()
    if fam in ("wino4", "wino4_ca", "wino5"):
        return 1e-5 * s + 5e-3
    if fam in ("wino", "wino_ca", "x9"):
        return 2e-6 * s + 2e-3
    return 2e-3             # test_conv2d_vs_torch_cpu


def _place(t, dev, off=0):
    """t on the device; off > 0: a contiguous view `off` floats past a 16-byte boundary of a larger allocation"""
    if t is None:
        return None
    if not off:
        return t.to(dev).contiguous()
    buf = torch.empty(t.numel() + 4, device=dev, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (t.numel() == 0 or v.data_ptr() % 16 == 4 * off)
    return v


_setup = R.case_setup      # the case's modes, thresholds, route batch and grad mode (shared with tests/test_conv_routes_host.py)


def _call(ops, case, dev, rows=slice(None)):
    """one ops.conv2d call of the case (on its batch rows `rows`) under ops.profile -> (results by name, launched kernel names)"""
    t, o, off = R.inputs_of(case), case.o, dict(case.offsets)
    put = lambda v, name=None: None if v is None else _place(v[rows], dev, off.get(name, 0))
    srcs = [put(s, "src") for s in t["srcs"]]
    ws = [w_.to(dev) for w_ in t["weights"]]
    bs = None if t["biases"] is None else [b.to(dev) for b in t["biases"]]
    one = len(ws) == 1
    kw = dict(act=o["act"], slope=R.SLOPE, residual=put(t["residual"], "residual"), chan_partial=o["chan_partial"],
              ca=None if t["ca"] is None else (put(t["ca"][0]), put(t["ca"][1], "ca_x")), ca_out=o["ca_out"],
              pixel_shuffle2=o["pixel_shuffle2"], sigmoid_from=o["sigmoid_from"], dgrad=o["dgrad"], res_scale=put(t["res_scale"]),
              border=o["border"], sum_mul=put(t["sum_mul"], "sum_mul"), precision=o["precision"])
    with ops.profile() as prof:
        try:
            r = ops.conv2d(srcs if len(srcs) > 1 else srcs[0], ws[0] if one else ws, None if bs is None else bs[0] if one else bs, **kw)
        except (ValueError, NotImplementedError) as e:
            return e, [rec[0] for rec in prof.records]
    names = [rec[0] for rec in prof.records]
    r = list(r) if isinstance(r, tuple) else [r]
    res = {}
    if o["border"]:
        res["pieces"] = r.pop()
    res["out"] = r.pop(0)
    if o["chan_partial"] or o["sum_mul"]:
        res["part"] = r.pop(0)
    if o["ca_out"]:
        res["xs"] = r.pop(0)
    assert not r, f"{case.id}: {len(r)} results more than the options ask for"
    return res, names


def _err(got, want):
    return (got.detach().cpu().double() - want).abs().max().item() if want.numel() else 0.0


def _check(ops, case, dev):
    """route and values of one case; returns (results, route, reference) for the tests that compare further"""
    route = case.route(lab=ops.lab_available())
    with _setup(ops, case):
        res, names = _call(ops, case, dev)
    if route.raises:
        assert isinstance(res, Exception) and type(res).__name__ == route.raises and names == [], \
            f"{case.id}: expected {route.raises} ({route.why}) before any launch, got {res!r} after launching {names}"
        return None, route, None
    assert not isinstance(res, Exception), f"{case.id}: predicted {list(route.kernels)}, raised {res!r}"
    assert names == list(route.kernels), f"{case.id}: launched {names}, predicted {list(route.kernels)} ({route.families})"
    fam, o = route.families[0], case.o
    rounded = "bf16" if fam == "bf16s" else case.m["h16"] if fam in ("h16g", "h16x1") else None
    ref = R.reference_of(case, rounded)
    out = res["out"]
    assert tuple(out.shape) == tuple(ref["out"].shape), (case.id, tuple(out.shape), tuple(ref["out"].shape))
    if case.n == 0:
        return res, route, ref
    scale = max(1.0, ref["out"].abs().max().item())
    # an option a family has no bound of its own for adds one fp32 operation to the plain convolution: the family's bound, on
    # the scale of what is returned
    bound = BF16_BOUND * ref["S"].max().item() if fam == "bf16s" else CONV_TOL[fam] * scale
    e = _err(out, ref["out"])
    print(f"{case.id}: {fam} max|out - ref64| {e:.3e} bound {bound:.3e}")
    assert e <= bound, f"{case.id}: {fam} output {e:.3e} > {bound:.3e}"
    if o["act"] == "relu_mask":
        assert (out.cpu()[R.inputs_of(case)["residual"] == 0] == 0).all()
    if o["chan_partial"]:
        part = res["part"]
        assert tuple(part.shape) == (case.n, route.part_tiles, case.cout), (case.id, tuple(part.shape), route.part_tiles)
        sb = _sums_bound(fam, ref, case)
        es = _err(part.sum(1), ref["sums"])
        print(f"{case.id}: channel sums {es:.3e} bound {sb:.3e}")
        assert es <= sb, f"{case.id}: {fam} channel sums {es:.3e} > {sb:.3e}"
    if o["sum_mul"]:
        rows = res["part"]
        assert tuple(rows.shape) == (case.n, route.part_tiles, case.cout), (case.id, tuple(rows.shape), route.part_tiles)
        # test_conv2d_dgrad_sum_mul_* (tests/test_hip_backward.py): 2e-6 max(1, sum |out| |m|) against the kernel's own output; the
        # output's error e <= bound moves a plane sum by at most bound * sum |m|
        m = R.inputs_of(case)["sum_mul"].double()
        rb = 2e-6 * max(1.0, (ref["out"].abs() * m.abs()).sum((2, 3)).max().item()) + bound * m.abs().sum((2, 3)).max().item()
        er = _err(rows.sum(1), ref["rows"])
        print(f"{case.id}: sum_mul rows {er:.3e} bound {rb:.3e}")
        assert er <= rb, f"{case.id}: sum_mul rows {er:.3e} > {rb:.3e}"
    if o["ca_out"]:
        assert _err(res["xs"], ref["xs"]) <= 1e-6 * max(1.0, ref["xs"].abs().max().item())      # (the prologue tests: 1e-6)
    if o["border"]:
        assert (res["pieces"] is not None) == route.pieces, (case.id, route.pieces)
        if route.pieces:        # test_rcab_attention_before_the_second_convolution_fp32: the pieces are the output's border lines
            p, y = res["pieces"], out.cpu().double()
            lines = [y[:, :, 0, :].sum(-1), y[:, :, -1, :].sum(-1), y[:, :, :, 0].sum(-1), y[:, :, :, -1].sum(-1)]
            for bi, (want, cnt) in enumerate(zip(lines, (p.p_rows, p.p_rows, p.p_cols, p.p_cols))):
                assert _err(p.data[:, bi, :cnt].sum(1), want) <= 1e-5 * max(1.0, want.abs().max().item()), (case.id, bi)
    return res, route, ref


def _by_group(*groups):
    return [c for c in R.cases() if c.group in groups]


@pytest.mark.parametrize("case", _by_group("A"), ids=lambda c: c.id)
def test_each_gate_from_both_sides(ops, cuda, case):
    _check(ops, case, cuda)


@pytest.mark.parametrize("case", _by_group("B"), ids=lambda c: c.id)
def test_every_option_on_every_route(ops, cuda, case):
    _check(ops, case, cuda)


@pytest.mark.parametrize("case", _by_group("C"), ids=lambda c: c.id)
def test_pointers_past_a_16_byte_boundary(ops, cuda, case):
    """the same data 4, 8 and 12 bytes past a 16-byte boundary: the reference result on the predicted (dword) route, or the
    documented NotImplementedError of the fused prologue -- and the aligned call of the same case gives the same values"""
    res, route, ref = _check(ops, case, cuda)
    if res is not None:
        import dataclasses
        aligned, route_a, _ = _check(ops, dataclasses.replace(case, id=case.id + "-aligned", offsets=()), cuda)
        scale = max(1.0, ref["out"].abs().max().item())      # each is within its family's bound of the reference
        assert _err(res["out"], aligned["out"].cpu().double()) <= (CONV_TOL[route.families[0]] + CONV_TOL[route_a.families[0]]) * scale


@pytest.mark.parametrize("case", _by_group("E"), ids=lambda c: c.id)
def test_degenerate_sizes(ops, cuda, case):
    _check(ops, case, cuda)


@pytest.mark.parametrize("case", _by_group("F"), ids=lambda c: c.id)
def test_16_bit_mode_routing(ops, cuda, case):
    _check(ops, case, cuda)


@pytest.mark.parametrize("case", R.ROUTE_BATCH_CASES, ids=lambda c: c.id)
def test_route_batch_pins_the_rows_to_the_whole_batch(ops, cuda, case):
    """forward_long's contract: under ops.route_batch(n) the rows [i:i+1] launch the kernels the whole batch launches and are
    bit-identical to its rows; without the pin a row is predicted onto the other route, and takes it"""
    import dataclasses
    whole, route, _ = _check(ops, case, cuda)
    row = dataclasses.replace(case, n=1)
    unpinned = row.route(lab=ops.lab_available())
    assert unpinned.kernels != route.kernels, (case.id, unpinned.kernels)
    for i in range(case.n):
        with _setup(ops, dataclasses.replace(case, route_batch=case.n)):
            part, names = _call(ops, case, cuda, rows=slice(i, i + 1))
        assert names == list(route.kernels), (case.id, i, names)
        for key in ("out", "part"):
            assert torch.equal(part[key], whole[key][i:i + 1]), f"{case.id}: row {i} of {key} differs from the whole-batch run"
        with _setup(ops, case):
            _, names = _call(ops, case, cuda, rows=slice(i, i + 1))
        assert names == list(unpinned.kernels), (case.id, i, names, unpinned.kernels)


FUSED_AND_FALLBACK = {      # option -> (the shape its fused form runs at, LOWERED thresholds; the fallback: the same call in mode "direct")
    "res_scale": "wino4", "shuffle": "wino4", "sum_mul": "x6s", "dgrad": "x6s",
}


@pytest.mark.parametrize("oname", sorted(FUSED_AND_FALLBACK))
def test_fused_and_fallback_forms_agree(ops, cuda, oname):
    """the epilogue form of an option and its two-step form, same shape and data: each within its bound of the float64 reference
    (the real check, in _check), and so within the sum of the two bounds of each other"""
    by_id = {c.id: c for c in R.cases()}
    rname = FUSED_AND_FALLBACK[oname]
    fused, route_f, ref = _check(ops, by_id[f"B-{rname}-{oname}-winograd4"], cuda)
    plain, route_p, _ = _check(ops, by_id[f"B-{rname}-{oname}-direct"], cuda)
    assert route_f.kernels != route_p.kernels and len(route_f.kernels) == 1, (route_f.kernels, route_p.kernels)
    scale = max(1.0, ref["out"].abs().max().item())
    both = (CONV_TOL[route_f.families[0]] + CONV_TOL[route_p.families[0]]) * scale
    assert _err(fused["out"], plain["out"].cpu().double()) <= both
    if oname == "sum_mul":
        m = R.inputs_of(by_id[f"B-{rname}-{oname}-direct"])["sum_mul"].double()
        rows_bound = 2 * 2e-6 * max(1.0, (ref["out"].abs() * m.abs()).sum((2, 3)).max().item()) + both * m.abs().sum((2, 3)).max().item()
        assert _err(fused["part"].sum(1), plain["part"].sum(1).cpu().double()) <= rows_bound
