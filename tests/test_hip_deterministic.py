"""The opt-in deterministic training mode (networks.set_deterministic, csrc/det_scatter.hip): the atomic-free backward kernels
against float64 references and against themselves (bitwise, launch after launch), whole training steps that repeat bit for
bit -- eager, graphed, bf16, past npost, the x2 model, after a checkpoint resume, under torch.use_deterministic_algorithms --
plus the switch's reach (recapture, kernel names).  Every test switches the mode through networks.deterministic (or restores
torch's flag itself)."""
from argparse import Namespace

import pytest
import torch

from tests import backward_refs as R
from tests import helpers as H
from tests.test_hip_backward_kernels import PIX, RED, RESIZE, WARP_SHAPES, close, leaf, vjp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def AG(cuda):
    from eavsr_amd import autograd as _ag, ops
    ops.lib()
    return _ag


def _Nw():
    from eavsr_amd import networks
    return networks


def _ops():
    from eavsr_amd import ops
    return ops


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _repeat3(fn):
    """fn() three times: the results must be torch.equal (the first one is returned)"""
    outs = [fn() for _ in range(3)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0]


# ------------------------------------------------------------------------------------------ 1. resize_bilinear_ac, gather form
@pytest.mark.parametrize("pre,post", [("none", "none"), ("grad", "grad"), ("grad", "const"), ("const", "grad")],
                         ids=["plain", "pre_post_grad", "pre_grad", "post_grad"])
@pytest.mark.parametrize("case", list(RESIZE))
def test_resize_backward_gather_against_float64(AG, cuda, case, pre, post):
    ops = _ops()
    hw_in, hw_out, scale = RESIZE[case]
    n, c = 2, 12
    x = R.randn64(700, n, c, *hw_in)
    p_ = None if pre == "none" else R.randn64(701, n, c, *hw_in)
    q_ = None if post == "none" else R.randn64(702, n, c, *hw_out)
    G = R.randn64(703, n, c, *hw_out)
    grads = {"x": True, "pre": pre == "grad", "post": post == "grad"}
    cl = [None if t is None else leaf(t, grad=grads[k]) for k, t in (("x", x), ("pre", p_), ("post", q_))]
    gl = [None if t is None else leaf(t, cuda, grad=grads[k]) for k, t in (("x", x), ("pre", p_), ("post", q_))]
    ref_out = R.resize_ac(cl[0], hw_out, scale, cl[1], cl[2])
    with _Nw().deterministic(True), ops.profile() as prof:
        got_out = AG.resize_bilinear_ac(gl[0], hw_out, scale, pre_add=gl[1], post_add=gl[2])
        got = vjp(got_out, G, [t for t in gl if t is not None])
    names = set(prof.summary())
    assert "resize_bilinear_ac_bwd_det" in names and "resize_bilinear_ac_bwd" not in names, names
    ref = vjp(ref_out, G, [t for t in cl if t is not None])
    keys = [k for k, t in zip(("x", "pre", "post"), cl) if t is not None]
    close(f"resize det {case} pre {pre} post {post}", {f"d{k}": (g, r) for k, g, r in zip(keys, got, ref)}, PIX)


@pytest.mark.parametrize("case", list(RESIZE))
def test_resize_backward_gather_repeats_and_matches_the_atomic_kernel(cuda, case):
    ops = _ops()
    hw_in, hw_out, scale = RESIZE[case]
    shape = (2, 144, *hw_in)
    dout = R.randn64(710, 2, 144, *hw_out).float().to(cuda)
    det = _repeat3(lambda: ops.resize_bilinear_ac_bwd_det(dout, shape, scale))
    atom = ops.resize_bilinear_ac_bwd(dout, shape, scale)
    assert _rel(det, atom) <= PIX, _rel(det, atom)      # (the compiler may contract rh * oy - y0 differently in the two kernels)
    assert torch.equal(det == 0, atom == 0)      # the same cells are reached


# ------------------------------------------------------------------------------------------ 2. flow_warp dx, inverted index
def _collision_flow(kind, n, h, w):
    """zoom: every sample moves 80 % of the way to the centre (four to five sources per reached cell); collapse: every pixel
    samples one position, (10.37, 7.61) -- four cells receive every source"""
    gy, gx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    if kind == "zoom":
        tx, ty = (w - 1) / 2 + 0.2 * (gx - (w - 1) / 2) + 0.013, (h - 1) / 2 + 0.2 * (gy - (h - 1) / 2) + 0.017
    else:
        tx, ty = torch.full_like(gx, 10.37), torch.full_like(gy, 7.61)
    return torch.stack((tx - gx, ty - gy), 0).expand(n, 2, h, w).float().double()


def _warp_det(AG, cuda, x, flow, G, need_flow):
    ops = _ops()
    gl = [leaf(x, cuda), leaf(flow, cuda, grad=need_flow)]
    with _Nw().deterministic(True), ops.profile() as prof:
        got = vjp(AG.flow_warp(*gl), G, gl)
    names = set(prof.summary())
    assert "flow_warp_bwd_dx_det" in names, names
    assert ("flow_warp_bwd" in names) == need_flow, names      # the fixed-order dflow half, only when asked for
    return got


@pytest.mark.parametrize("c", [64, 2], ids=lambda c: f"c{c}")
@pytest.mark.parametrize("shape", list(WARP_SHAPES))
@pytest.mark.parametrize("region", ["mixed", "edge", "far"])
def test_flow_warp_dx_det_against_float64(AG, cuda, region, shape, c):
    n, h, w = WARP_SHAPES[shape]
    x = R.randn64(720, n, c, h, w)
    flow = R.warp_flow(721, n, h, w, region)
    G = R.randn64(722, n, c, h, w)
    cl = [leaf(x), leaf(flow)]
    ref = vjp(R.flow_warp(*cl), G, cl)
    got = _warp_det(AG, cuda, x, flow, G, True)
    close(f"flow_warp det {region} {shape} c{c}", {"dx": (got[0], ref[0]), "dflow": (got[1], ref[1])}, PIX)
    unreached = ~R.reached(flow)
    assert (got[0].cpu().permute(1, 0, 2, 3)[:, unreached] == 0).all()


@pytest.mark.parametrize("kind,shape", [("zoom", (2, 96, 96)), ("collapse", (1, 33, 130)), ("collapse", (2, 48, 64))],
                         ids=["zoom_2x96x96", "collapse_1x33x130", "collapse_2x48x64"])
def test_flow_warp_dx_det_with_colliding_samples(AG, cuda, kind, shape):
    n, h, w = shape
    c = 12
    x = R.randn64(730, n, c, h, w)
    flow = _collision_flow(kind, n, h, w)
    G = R.randn64(731, n, c, h, w)
    cl = [leaf(x), leaf(flow, grad=False)]
    ref = vjp(R.flow_warp(*cl), G, cl)
    got = _warp_det(AG, cuda, x, flow, G, False)
    close(f"flow_warp det {kind} {n}x{h}x{w}", {"dx": (got[0], ref[0])}, RED)      # lists of up to h * w entries: a reduction
    if kind == "collapse":
        nz = (got[0].cpu() != 0).sum(dim=(0, 1))
        assert int((nz > 0).sum()) == 4      # exactly the four corners of (10.37, 7.61)


@pytest.mark.parametrize("kind", ["mixed", "zoom", "collapse"])
def test_flow_warp_dx_det_repeats_and_matches_the_atomic_kernel(cuda, kind):
    ops = _ops()
    n, c, h, w = 2, 64, 45, 77
    flow = (R.warp_flow(740, n, h, w, "mixed") if kind == "mixed" else _collision_flow(kind, n, h, w)).float().to(cuda)
    flow2 = R.randn64(741, n, 2, h, w, scale=0.5).float().to(cuda)
    f1 = (flow - flow2).contiguous()
    x = R.randn64(742, n, c, h, w).float().to(cuda)
    dout = R.randn64(743, n, c, h, w).float().to(cuda)
    for fa, fb in ((flow, None), (f1, flow2)):
        det = _repeat3(lambda: ops.flow_warp_bwd_dx_det(fa, fb, dout))
        atom = ops.flow_warp_bwd(x, fa, fb, dout, True, False)[0]
        assert _rel(det, atom) <= (PIX if kind != "collapse" else RED), _rel(det, atom)


# ------------------------------------------------------------------------------------------ 3. DCNv2 dx, gather-form col2im
def _dcn_case(AG, cuda, sigma, n, h, w, seed):
    dg = 8
    x = R.randn64(seed, n, 64, h, w)
    off = R.dcn_offsets(seed + 1, n, dg, h, w, sigma)
    mask = R.uniform64(seed + 2, 0.0, 1.0, n, dg * 9, h, w)
    wt = R.randn64(seed + 3, 64, 64, 3, 3, scale=1.0 / 24)
    b = R.randn64(seed + 4, 64, scale=0.1)
    G = R.randn64(seed + 5, n, 64, h, w)
    return dg, (x, off, mask, wt, b), G


@pytest.mark.parametrize("sigma", [1.0, 6.0, 20.0], ids=["sigma1", "sigma6", "sigma20"])
def test_dcnv2_dx_det_against_float64(AG, cuda, sigma):
    """sigma = 20: most corners leave the sampler backward's LDS window (and many the image)"""
    ops = _ops()
    n, h, w = 2, 48, 64
    dg, ts, G = _dcn_case(AG, cuda, sigma, n, h, w, 750)
    cl = [leaf(t) for t in ts]
    ref_out = R.dcnv2(*cl, dg)
    ref = vjp(ref_out, G, cl)
    gl = [leaf(t, cuda) for t in ts]
    with _Nw().deterministic(True), ops.profile() as prof:
        got_out = AG.modulated_deform_conv2d(gl[0], gl[1], gl[2], gl[3], gl[4], 1, 1, 1, 1, dg)
        got = vjp(got_out, G, gl)
    names = set(prof.summary())
    assert {"dcnv2_bwd", "dcnv2_col2im_dx_det"} <= names and "dcnv2_col2im" not in names and "il8_to_nchw" not in names, names
    keys = ["dx", "doffset", "dmask", "dweight", "dbias"]
    close(f"dcnv2 det bwd {n}x64x{h}x{w} sigma{sigma:g}", dict(zip(keys, zip(got, ref))), RED)


@pytest.mark.parametrize("sigma", [1.0, 6.0, 20.0], ids=["sigma1", "sigma6", "sigma20"])
def test_dcnv2_dx_det_repeats_and_matches_the_sampler_backward(AG, cuda, sigma):
    ops = _ops()
    n, h, w = 2, 48, 64
    dg, ts, G = _dcn_case(AG, cuda, sigma, n, h, w, 760)
    x, off, mask, wt, _ = [t.float().to(cuda) for t in ts]
    dy = G.float().to(cuda)
    dcol = ops.conv2d(dy, AG._dcn_wt(wt), None)
    det = _repeat3(lambda: ops.dcnv2_col2im_dx_det(off, mask, dcol, dg))
    atom = ops.dcnv2_bwd(x, off, mask, wt, dy, dg, need_dx=True)[0]
    assert _rel(det, atom) <= RED, _rel(det, atom)


def test_dcnv2_columns_backward_is_refused_in_deterministic_mode(AG, cuda, monkeypatch):
    ops = _ops()
    dg, ts, _ = _dcn_case(AG, cuda, 1.0, 1, 8, 16, 770)
    gl = [leaf(t, cuda) for t in ts]
    monkeypatch.setattr(ops, "DCN_BWD", "columns")
    with _Nw().deterministic(True):
        with torch.no_grad():      # no backward, nothing to refuse
            ops.modulated_deform_conv2d(*[t.detach() for t in gl[:4]], gl[4].detach(), 1, 1, 1, 1, dg)
        y = AG.modulated_deform_conv2d(gl[0], gl[1], gl[2], gl[3], gl[4], 1, 1, 1, 1, dg)
        with pytest.raises(RuntimeError, match="deterministic training mode.*EAVSR_DCN_BWD=columns"):
            y.sum().backward()
    AG.modulated_deform_conv2d(gl[0], gl[1], gl[2], gl[3], gl[4], 1, 1, 1, 1, dg).sum().backward()      # the default mode takes it


# ------------------------------------------------------------------------------------------ 4. whole training steps
def _opt(scale=4, **kw):
    o = Namespace(predict=False, n_frame=3, n_flow=5, scale=scale, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                  weight_decay=0.0, npost=350, load_path="")
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _model(sd, scale=4, **kw):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    from eavsr_amd.eavsrpx2_model import EAVSRPx2Model
    m = (EAVSRPModel if scale == 4 else EAVSRPx2Model)(_opt(scale, **kw))
    m.netEAVSRP.load_state_dict(sd, strict=True)
    return m


def _data(scale, seeds, lr_hw=64):
    from eavsr_amd.utils.synthetic import synthetic_clip
    return [{"lr_seq": synthetic_clip(1, 3, lr_hw, lr_hw, seed=s), "hr_seq": synthetic_clip(1, 3, lr_hw * scale, lr_hw * scale, seed=s + 100),
             "fname": "x"} for s in seeds]


def _snapshot(m):
    named = dict(m.netEAVSRP.named_parameters())
    return ({k: p.detach().clone() for k, p in named.items()},
            {k: p.grad.detach().clone() for k, p in named.items() if p.grad is not None})


def _run(sd, steps=3, graphed=False, scale=4, epoch=0, **kw):
    """`steps` training steps of a fresh model from sd: (losses, per step (params, grads))"""
    from eavsr_amd.graph import GraphedTrainStep
    m = _model(sd, scale, **kw)
    data = _data(scale, [21, 22, 23, 24][:steps])
    losses, snaps = [], []
    if graphed:
        m.set_input(data[0], epoch=epoch)
        g = GraphedTrainStep(m, warmup=1)
        assert g.deterministic is True
        for d in data:
            g.step({k: v.to(m.device) for k, v in d.items() if k != "fname"}, epoch=epoch)
            losses.append(m.loss_EAVSRP_L1.detach().clone())
            snaps.append(_snapshot(m))
        g.close()
    else:
        for d in data:
            m.set_input(d, epoch=epoch)
            m.optimize_parameters()
            losses.append(m.loss_EAVSRP_L1.detach().clone())
            snaps.append(_snapshot(m))
    return losses, snaps


def _assert_bitwise(a, b):
    """loss, every p.grad and every parameter after every step: torch.equal"""
    la, sa = a
    lb, sb = b
    assert len(la) == len(lb) >= 3
    for i, (x, y) in enumerate(zip(la, lb)):
        assert torch.equal(x, y), (i, x.item(), y.item())
    for i, ((pa, ga), (pb, gb)) in enumerate(zip(sa, sb)):
        assert set(ga) == set(gb) and len(ga) > 0
        for k in pa:
            assert torch.equal(pa[k], pb[k]), (i, "param", k, (pa[k] - pb[k]).abs().max().item())
        for k in ga:
            assert torch.equal(ga[k], gb[k]), (i, "grad", k, (ga[k] - gb[k]).abs().max().item())


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_training_steps_repeat_bit_for_bit(cuda, graphed):
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    with _Nw().deterministic(True):
        a = _run(sd, graphed=graphed)
        b = _run(sd, graphed=graphed)
    _assert_bitwise(a, b)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_bf16_training_steps_repeat_bit_for_bit(cuda, graphed):
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    Nw = _Nw()
    with Nw.deterministic(True), Nw.train_precision("bf16"):
        a = _run(sd, graphed=graphed)
        b = _run(sd, graphed=graphed)
    _assert_bitwise(a, b)


def test_x2_training_steps_repeat_bit_for_bit_after_an_x4_run(cuda):
    """an x4 run first: its freed weights' id()s are reused by the x2 model (history that must not reach the x2 steps)"""
    with _Nw().deterministic(True):
        _run(H.filled(H.model_shapes("x4"), "trained_like"), steps=1)
        sd = H.filled(H.model_shapes("x2"), "trained_like")
        a = _run(sd, scale=2)
        b = _run(sd, scale=2)
    _assert_bitwise(a, b)


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_masked_training_steps_past_npost_repeat_bit_for_bit(cuda, tmp_path, graphed):
    from tests.test_hip_pwc import _write_pwc_file
    _write_pwc_file(tmp_path)
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    kw = dict(pwc_path=str(tmp_path / "pwc-default"))
    with _Nw().deterministic(True):
        a = _run(sd, graphed=graphed, epoch=350, **kw)
        b = _run(sd, graphed=graphed, epoch=350, **kw)
    _assert_bitwise(a, b)


def test_checkpoint_resume_is_bitwise_in_deterministic_mode(cuda, tmp_path):
    """the deterministic twin of test_hip_backward.py's resume check (there: equal to 1e-6)"""
    from eavsr_amd.eavsrp_model import EAVSRPModel
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    data = _data(4, [31, 32, 33])
    kw = dict(checkpoints_dir=str(tmp_path), name="run", optimizer="Adam")
    with _Nw().deterministic(True):
        model = _model(sd, **kw)
        for d in data[:2]:
            model.set_input(d, epoch=0)
            model.optimize_parameters()
        model.save_networks(7)
        model.set_input(data[2], epoch=0)
        model.optimize_parameters()
        want = {k: v.detach().clone() for k, v in model.netEAVSRP.state_dict().items()}
        want_loss = model.loss_EAVSRP_L1.detach().clone()
        resumed = EAVSRPModel(_opt(4, **kw))
        resumed.load_networks(7)
        resumed.load_optimizers(7)
        resumed.set_input(data[2], epoch=0)
        resumed.optimize_parameters()
        got = resumed.netEAVSRP.state_dict()
    assert torch.equal(resumed.loss_EAVSRP_L1, want_loss)
    for k in want:
        assert torch.equal(got[k], want[k]), (k, (got[k].float() - want[k].float()).abs().max().item())


# ------------------------------------------------------------------------------------------ 5. the switch's reach
def _bwd_kernels(m, d):
    ops = _ops()
    with ops.profile() as prof:
        m.set_input(d, epoch=0)
        m.optimize_parameters()
    return set(prof.summary())


DET_KERNELS = {"flow_warp_bwd_dx_det", "resize_bilinear_ac_bwd_det", "dcnv2_col2im_dx_det"}


def test_mode_switch_recaptures_and_the_context_restores_the_default_kernels(cuda):
    from eavsr_amd.graph import GraphedTrainStep
    Nw = _Nw()
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    data = _data(4, [41, 42])
    on_dev = lambda d: {k: v.to(cuda) for k, v in d.items() if k != "fname"}
    assert not Nw.get_deterministic()
    e = _model(sd)      # eager, for the kernel names
    default = _bwd_kernels(e, data[0])
    assert not (DET_KERNELS & default) and {"resize_bilinear_ac_bwd", "flow_warp_bwd"} <= default, default
    m = _model(sd)
    m.set_input(data[0], epoch=0)
    g = GraphedTrainStep(m, warmup=1)
    assert g.deterministic is False
    old = g.graph
    with Nw.deterministic():
        assert Nw.get_deterministic()
        g.step(on_dev(data[1]))
        assert g.graph is not old and g.deterministic is True
        det = _bwd_kernels(e, data[1])
        assert DET_KERNELS <= det and "resize_bilinear_ac_bwd" not in det, det
        old = g.graph
        g.step(on_dev(data[0]))
        assert g.graph is old                    # no change, no recapture
    assert not Nw.get_deterministic()
    g.step(on_dev(data[1]))
    assert g.graph is not old and g.deterministic is False
    g.close()
    assert _bwd_kernels(e, data[0]) == default


def test_torch_use_deterministic_algorithms_engages_the_mode(cuda):
    Nw = _Nw()
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    prev = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)      # (fills torch.empty with NaN: every kernel must write what it is read for)
        assert Nw.get_deterministic() and not _ops().DETERMINISTIC
        data = _data(4, [51])
        m = _model(sd)
        names = _bwd_kernels(m, data[0])
        assert DET_KERNELS <= names, names
        a, b = _run(sd), _run(sd)
        c, d = _run(sd, graphed=True), _run(sd, graphed=True)
    finally:
        torch.use_deterministic_algorithms(prev)
    _assert_bitwise(a, b)
    _assert_bitwise(c, d)
    for k, p in a[1][-1][0].items():      # (torch.empty is NaN-filled under the flag: nothing read what nobody wrote)
        assert torch.isfinite(p).all(), k
    assert not Nw.get_deterministic()
