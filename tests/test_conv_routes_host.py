"""The router of ops.conv2d on the CPU.  `ops.conv_route` -- the route decision over plain numbers -- gives, for every case of the
matrix, the kernels, families, tile count and border pieces that tests/conv_routes.py's independent `predict_route` names (what
tests/test_hip_conv_routes.py then checks against the launches themselves), and the public gates `x6s_takes`, `wgrad_bf16_takes` and
`ca_fusable` agree with it at the boundary shapes.  The helper itself: `predict_route` names every product route somewhere in the
case matrix and changes sides exactly at each gate, `reference` agrees with a plain torch restatement of every option, the
threshold context manager restores what it found, and `boundary_shapes` returns the launches next to a threshold.  The tile counts
come from the library's host-side counters (no device)."""
import contextlib
import types

import pytest
import torch
import torch.nn.functional as F

from tests import conv_routes as R


def test_every_product_route_is_asserted_by_some_case():
    """each kernel family of ops._CONV_KERNELS that conv2d can launch on the product library (and the two second steps of the
    fallback forms) is in the predicted kernel list of at least one case; with the lab library loaded the retired schedules are too"""
    seen, seen_lab = set(), set()
    for c in R.cases():
        seen.update(c.route(lab=False).families)
        seen_lab.update(c.route(lab=True).families)
    assert not set(R.PRODUCT_FAMILIES) - seen, sorted(set(R.PRODUCT_FAMILIES) - seen)
    assert not seen & set(R.LAB_FAMILIES) - {"x9"} and not {"wino", "wino4_ca", "x9"} - seen_lab, (seen, seen_lab)
    for name, (shape, k, chans, couts, md) in R.ROUTE_SHAPES.items():
        assert R.predict_route(*shape, k, chans, couts, modes=md, thr=R.LOWERED).families == (R.ROUTE_FAMILY[name],), name
    from eavsr_amd import ops
    assert {f[:-3] if f.endswith("_ca") else f for f in R.PRODUCT_FAMILIES + R.LAB_FAMILIES} - {"scale_residual", "plane_sum"} == set(ops._CONV_KERNELS)


@pytest.fixture
def ops():
    from eavsr_amd import ops as _ops
    state = lambda: (_ops.WINO_MIN_TILES, _ops.X6S_MAX_TILES, _ops.CONV3_SMALL, _ops.CONV_MODE, _ops.CONV5_MODE, _ops.CONV7_MODE,
                     _ops.CONV3_H16, _ops._ROUTE_BATCH, torch.is_grad_enabled())
    before = state()
    yield _ops
    assert state() == before, "a test of this file left a threshold, a mode, a pinned route batch or a grad mode behind"


@contextlib.contextmanager
def _under(ops, case):
    """the body under the case's setup; yields False instead, where that is a lab-only conv mode on the product library (what the
    GPU test skips: LabBuildRequired)"""
    with contextlib.ExitStack() as st:
        try:
            st.enter_context(R.case_setup(ops, case))
        except ops.LabBuildRequired:
            assert case.m["conv"] in R.LAB_MODES and not ops.lab_available(), case.id
            yield False
            return
        yield True


def _route_of(ops, case, **kw):
    """ops.conv_route on the plain facts of a case (under its setup): a pointer `o` floats past a 16-byte boundary has the address
    residue 4 o"""
    o, off = case.o, dict(case.offsets)
    mod = lambda name: 4 * off.get(name, 0) % 16
    facts = dict(act=o["act"], residual=o["residual"], chan_partial=o["chan_partial"], ca=o["ca"], ca_out=o["ca_out"],
                 pixel_shuffle2=o["pixel_shuffle2"], res_scale=o["res_scale"], sum_mul=o["sum_mul"], dgrad=o["dgrad"],
                 sigmoid_from=o["sigmoid_from"], border=o["border"], precision=o["precision"], src_mod=[mod("src")] * len(case.chans),
                 residual_mod=mod("residual"), ca_mod=mod("ca_x"), sum_mul_mod=mod("sum_mul"), sum_mul_shaped=True,
                 grad=torch.is_grad_enabled())
    return ops.conv_route(case.n, case.h, case.w, case.k, case.chans, case.cout, len(case.couts), case.bias, **{**facts, **kw})


def test_conv_route_names_what_predict_route_names_for_every_case(ops):
    """the route decision of ops.py against the restatement that never looked at it, on the whole matrix: the same exception type
    where one is predicted; otherwise the same kernel names in launch order (the second step of a fallback form included), the
    same families, tile count of the sums and border pieces"""
    lab = ops.lab_available()
    differ, left_out = [], 0
    for c in R.cases():
        want = c.route(lab=lab)
        with _under(ops, c) as ok:
            if not ok:
                left_out += 1
                continue
            try:
                got = _route_of(ops, c)
                got = (None, got.kernels, got.families, got.part_tiles, got.pieces)
            except (ValueError, NotImplementedError) as e:
                got = (type(e).__name__, (), (), None, False)
        if got != (want.raises, want.kernels, want.families, want.part_tiles, want.pieces):
            differ.append((c.id, got, want))
    assert not differ, (len(differ), differ[:5])
    assert left_out == (0 if lab else sum(c.m["conv"] in R.LAB_MODES for c in R.cases()))


def test_public_gates_agree_with_conv_route_at_the_boundary_shapes(ops):
    """x6s_takes / wgrad_bf16_takes (what autograd and the model ask before a launch) and ca_fusable share their predicates with
    the router: on each side of every group-A gate, the crop-sized kernel runs exactly where x6s_takes says and the Winograd kernel
    does not take the launch first; the bf16 forms and the in-place input-gradient weight follow it; the bf16 weight gradient asks
    w % 4 == 0 on top; the prologue is accepted exactly where ca_fusable says"""
    seen = set()
    for c in R.cases():
        if c.group != "A" or c.k != 3:
            continue
        with _under(ops, c) as ok:
            if not ok:
                continue
            takes = ops.x6s_takes(c.n, c.h, c.w)
            plain = ops.conv_route(c.n, c.h, c.w, 3, (64,), 64)
            x6s = takes and not plain.family.startswith("wino")
            seen.add((c.gate.split("-")[0], takes, plain.family))
            assert (plain.family == "x6s") == x6s, (c.id, takes, plain)
            assert (ops.conv_route(c.n, c.h, c.w, 3, (64,), 64, precision="bf16").family == "bf16s") == x6s, c.id
            dg = ops.conv_route(c.n, c.h, c.w, 3, (64,), 64, bias=False, dgrad=True)
            assert dg.materialise == (not x6s) and dg.family == plain.family, (c.id, dg)
            t = torch.empty(c.n, 1, c.h, c.w)
            assert ops.wgrad_bf16_takes([t], [[t]], 3) == (takes and c.w % 4 == 0), c.id
            assert not ops.wgrad_bf16_takes([t], [[t]], 5) and not ops.wgrad_bf16_takes([t], [[t[:, :, :, 1:]]], 3)
            if c.o["ca"]:
                try:
                    fused = _route_of(ops, c).family.endswith("_ca")
                except NotImplementedError:
                    fused = False
                assert ops.ca_fusable(torch.empty(c.n, 64, c.h, c.w), c.cout) == fused, c.id
                seen.add(("ca", fused))
    # both answers of each gate were seen
    assert {("x6s_max", True, "x6s"), ("x6s_max", False, "direct"), ("wino_min", True, "x6s"), ("wino_min", True, "wino4"),
            ("ca", True), ("ca", False)} <= seen, seen


def test_every_gate_has_a_case_on_each_side_and_the_kernel_changes_exactly_there():
    gates = {}
    for c in R.cases():
        if c.group == "A" and c.m["conv"] == "winograd4":
            r = c.route()
            gates.setdefault(c.gate, {}).setdefault(c.side, set()).add(r.raises or r.kernels)
    assert {"wino_min-lowered", "wino_min-shipped", "x6s_max-lowered", "x6s_max-shipped", "rows32-ca"} <= set(gates)
    assert {f"wino5-o{co}" for co in (40, 64, 72, 128)} <= set(gates)
    for gate, sides in gates.items():
        low = sides["below"]
        # x6s_max is an upper limit (<=): `at` is on the lower side; every other gate is a lower limit (>=)
        high = sides["above"] if gate.startswith("x6s_max") else sides.get("above", set()) | sides["at"]
        low = low | sides["at"] if gate.startswith("x6s_max") else low
        assert len(low) == 1 and len(high) == 1 and low != high, (gate, sides)
    # the ceil(cout / 64) factor moves the 16 x 32 launch across the 5x5 gate
    assert gates["wino5-o64"]["below"] == {("conv5x5_64to64",)} and gates["wino5-o72"]["at"] == {("conv5x5_64to72_wino",)}
    by_id = {c.id: c for c in R.cases()}
    assert by_id["A-wino5-o64-winograd4-16x32"].side == "below" and by_id["A-wino5-o72-winograd4-16x32"].side == "at"
    # the boundary triples are next to their thresholds
    cnt = R.counters()
    for label, thr in (("lowered", R.LOWERED), ("shipped", R.SHIPPED)):
        tri = {s: by_id[f"A-wino_min-{label}-winograd4-{s}"] for s in ("below", "at", "above")}
        counts = {s: c.n * cnt.wino(c.h, c.w) for s, c in tri.items()}
        assert counts["below"] < thr["wino_min"] == counts["at"] < counts["above"], counts
        tri = {s: by_id[f"A-x6s_max-{label}-winograd4-{s}"] for s in ("below", "at", "above")}
        counts = {s: c.n * cnt.x6s(c.h, c.w) for s, c in tri.items()}
        assert counts["below"] < thr["x6s_max"] == counts["at"] < counts["above"] and all(c.w % 4 for c in tri.values()), counts


def test_the_second_winograd_gate_never_disagrees_with_the_first():
    """2 n wino4_tiles >= WINO_MIN_TILES whenever n tiles(8 x 32) >= WINO_MIN_TILES: the F(4x4,3x3) tile is 8 x 64 pixels, and
    2 ceil(w / 64) >= ceil(w / 32).  There is no launch on which the first gate passes and the second fails -- the matrix has no such
    case because none exists; this is what says so."""
    cnt = R.counters()
    for h in (1, 7, 8, 9, 64, 96, 180):
        for w in range(4, 644, 4):
            assert 2 * cnt.wino4(h, w) >= cnt.wino(h, w), (h, w)


def test_route_batch_cases_change_sides_without_the_pin():
    import dataclasses
    for c in R.ROUTE_BATCH_CASES:
        whole, row = c.route(), dataclasses.replace(c, n=1).route()
        pinned = dataclasses.replace(c, n=1, route_batch=c.n).route()
        assert whole.kernels == pinned.kernels != row.kernels, (c.id, whole.kernels, row.kernels)


def test_rejected_combinations_are_rejected_on_every_route_and_misaligned_cases_never_take_a_16_byte_route():
    for c in R.cases():
        r = c.route()
        if c.group == "B" and c.id.split("-")[-2] in R.REJECTED:
            assert r.raises == "ValueError", c.id
        if c.group == "C":
            which, off = c.offsets[0]
            vec = {"src": {"wino4", "wino5", "smallco_lite", "h16g"}, "residual": {"wino4"}}.get(which, set())
            assert r.raises == "NotImplementedError" or not vec & set(r.families) or (which, off, r.families[0]) == ("residual", 2, "wino5"), c.id
            if c.o["ca"]:
                assert r.raises == "NotImplementedError"
            if c.o["sum_mul"]:
                assert r.families[-1] == "plane_sum", c.id


def test_thresholds_context_manager_restores_also_on_an_exception():
    ops = types.SimpleNamespace(WINO_MIN_TILES=192, X6S_MAX_TILES=256, CONV3_SMALL="x6s")
    with R.thresholds(ops, 4, 6, "direct"):
        assert (ops.WINO_MIN_TILES, ops.X6S_MAX_TILES, ops.CONV3_SMALL) == (4, 6, "direct")
        with R.thresholds(ops, x6s_max=9):
            assert (ops.WINO_MIN_TILES, ops.X6S_MAX_TILES, ops.CONV3_SMALL) == (4, 9, "direct")
        assert ops.X6S_MAX_TILES == 6
    with pytest.raises(KeyError):
        with R.thresholds(ops, 1, 2):
            raise KeyError("x")
    assert (ops.WINO_MIN_TILES, ops.X6S_MAX_TILES, ops.CONV3_SMALL) == (192, 256, "x6s")


def test_boundary_shapes_returns_the_smallest_launches_next_to_a_threshold():
    tiles = lambda h, w: -(-h // 8) * -(-w // 32)
    got = R.boundary_shapes(6, tiles)
    assert {k: v[0] * tiles(*v[1:]) for k, v in got.items()} == {"below": 5, "at": 6, "above": 7}
    assert got["at"] in ((1, 41, 1), (2, 17, 1), (3, 9, 1), (1, 17, 33), (1, 9, 65))      # 6 tiles on the fewest pixels
    assert got["at"] == (3, 9, 1)
    # counts that cannot be reached: the nearest on each side, and no "at"
    got = R.boundary_shapes(7, tiles, accept=lambda n, h, w: n == 2)
    assert {k: v[0] * tiles(*v[1:]) for k, v in got.items()} == {"below": 6, "above": 8}


def _t(seed, *shape, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def test_reference_agrees_with_a_plain_torch_restatement_of_each_option():
    n, h, w = 2, 5, 6
    x, x2 = _t(1, n, 8, h, w), _t(2, n, 4, h, w)
    wt, b = _t(3, 8, 12, 3, 3, scale=0.1), _t(4, 8, scale=0.1)
    res, m = _t(5, n, 8, h, w), _t(6, n, 8, h, w)
    conv = F.conv2d(torch.cat([x, x2], 1), wt, b, padding=1)
    close = lambda got, want: torch.allclose(got.float(), want, rtol=1e-5, atol=1e-5)
    ref = lambda opts, **kw: R.reference([x, x2], wt, b, opts, **kw)
    assert close(ref({})["out"], conv)
    assert close(ref(dict(act="relu"))["out"], conv.clamp_min(0))
    assert close(ref(dict(act="lrelu"))["out"], torch.where(conv > 0, conv, 0.1 * conv))
    r = ref(dict(act="relu", residual=True, chan_partial=True), residual=res)
    assert close(r["out"], conv.clamp_min(0) + res) and close(r["sums"], conv.clamp_min(0).flatten(2).sum(2))
    s = torch.rand(n, 8, generator=torch.Generator().manual_seed(7))
    assert close(ref(dict(residual=True, res_scale=True, act="relu"), residual=res, res_scale=s)["out"], res + s[:, :, None, None] * conv.clamp_min(0))
    mask = res.clamp_min(0)
    assert close(ref(dict(residual=True, act="relu_mask"), residual=mask)["out"], conv * (mask > 0))
    sig = ref(dict(sigmoid_from=4, act="relu"))["out"]
    assert close(sig[:, :4], conv[:, :4].clamp_min(0)) and close(sig[:, 4:], 1 / (1 + torch.exp(-conv[:, 4:])))
    ps = ref(dict(pixel_shuffle2=True))["out"]
    assert ps.shape == (n, 2, 2 * h, 2 * w)
    for c in range(2):
        for i in range(2):
            for j in range(2):
                assert close(ps[:, c, i::2, j::2], conv[:, 4 * c + 2 * i + j])
    # the channel-attention prologue, its side output; several weights
    sc, cx = torch.rand(n, 8, generator=torch.Generator().manual_seed(8)), _t(9, n, 8, h, w)
    w8 = _t(10, 6, 8, 3, 3, scale=0.1)
    r = R.reference([x], [w8[:2], w8[2:]], [None, b[:4]], dict(ca=True, ca_out=True), ca=(sc, cx))
    eff = x * sc[:, :, None, None] + cx
    assert close(r["xs"], eff) and close(r["out"], F.conv2d(eff, w8, torch.cat([torch.zeros(2), b[:4]]), padding=1))
    # dgrad: the input gradient of the forward convolution, by autograd; sum_mul: plane sums of the stored value times m
    wf = _t(11, 12, 8, 3, 3, scale=0.1)       # forward weight: 8 -> 12 channels; dY has 12 channels
    dy = torch.cat([x, x2], 1)
    xin = torch.zeros(n, 8, h, w, requires_grad=True)
    F.conv2d(xin, wf, None, padding=1).backward(dy)
    r = R.reference([x, x2], wf, None, dict(dgrad=True, residual=True, sum_mul=True), residual=res, sum_mul=m)
    assert close(r["out"], xin.grad + res) and close(r["rows"], ((xin.grad + res) * m).flatten(2).sum(2))
    # operands rounded once to a 16-bit type; S bounds the accumulation
    r = R.reference([x], w8, None, {}, round_to=torch.bfloat16)
    assert close(r["out"], F.conv2d(x.bfloat16().float(), w8.bfloat16().float(), None, padding=1))
    assert (r["S"] >= r["out"].abs() - 1e-12).all()
