"""The opt-in bf16 training mode (networks.set_train_precision("bf16")): its kernels against float64 references of the
bf16-rounded operands, the mode's reach (it engages in recorded training convolutions and nowhere else), training with it, and
GraphedTrainStep's recapture when the mode changes.  Every test switches modes through networks.train_precision (the autouse
fixture of tests/conftest.py does not know this global)."""
from argparse import Namespace

import pytest
import torch

from tests import helpers as H
from tests import train_bf16_refs as R

pytestmark = pytest.mark.gpu

CONV_BOUND = 2e-6       # max |kernel - ref| / max S for the convolutions (fp32 accumulation over K = 576)
WGRAD_BOUND = 1e-5      # ... for the weight gradient (K up to 7 x 2 x 96 x 96 = 129 K pixels)


@pytest.fixture(scope="module")
def ops(cuda):
    from eavsr_amd import ops as _ops
    return _ops


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(torch.float32)


def _err(got, ref):
    return (got.detach().cpu().to(torch.float64) - ref).abs().max().item()


SHAPES = [(2, 96, 96), (1, 19, 37), (3, 40, 64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_rounds_once_to_nearest_even_with_one_product(ops, cuda, shape):
    """bias + ReLU, residual and plain forms; cout 64 (two 32-channel tiles per packed `cot`) and 32 (one)"""
    n, h, w = shape
    assert ops.x6s_takes(n, h, w)
    g = torch.Generator().manual_seed(100 + h)
    x = _rand(g, n, 64, h, w)
    for cout in (64, 32):
        wt = _rand(g, cout, 64, 3, 3, scale=0.05)
        b = _rand(g, cout, scale=0.1)
        res = _rand(g, n, cout, h, w)
        xd, wd, bd = x.to(cuda), wt.to(cuda), b.to(cuda)
        ref, S = R.conv3x3_ref(R.bf16_rne(x), R.bf16_rne(wt), b)
        smax = S.max().item()
        y = ops.conv2d(xd, wd, bd, act="relu", precision="bf16")
        assert _err(y, ref.clamp_min(0)) <= CONV_BOUND * smax
        y = ops.conv2d(xd, wd, bd, residual=res.to(cuda), precision="bf16")
        assert _err(y, ref + res.to(torch.float64)) <= CONV_BOUND * smax
        y = ops.conv2d(xd, wd, bd, precision="bf16")
        e_rne = _err(y, ref)
        assert e_rne <= CONV_BOUND * smax, (e_rne, smax)
        # pins round-to-nearest-even: a truncating kernel is as close to the truncated reference as this one is to its own
        ref_tr, _ = R.conv3x3_ref(R.bf16_trunc(x), R.bf16_trunc(wt), b)
        e_tr = _err(y, ref_tr)
        assert e_rne * 20 <= e_tr, (e_rne, e_tr)
        # ... and shows the mode is really bf16: the exact kernel on the same data is far closer to the unrounded convolution
        ref_ex, _ = R.conv3x3_ref(x, wt, b)
        y_ex = ops.conv2d(xd, wd, bd)
        assert _err(y, ref_ex) >= 10 * _err(y_ex, ref_ex), (_err(y, ref_ex), _err(y_ex, ref_ex))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv_training_epilogues_and_dgrad_form(ops, cuda, shape):
    """the forms the training path uses: RELU_MASK, per-tile channel sums, the input-gradient (dgrad) weight form, sum_mul"""
    n, h, w = shape
    g = torch.Generator().manual_seed(200 + h)
    x = _rand(g, n, 64, h, w)
    wt = _rand(g, 64, 64, 3, 3, scale=0.05)
    b = _rand(g, 64, scale=0.1)
    t = _rand(g, n, 64, h, w)
    d = _rand(g, n, 64, h, w)
    m = _rand(g, n, 64, h, w)
    xd, wd, bd = x.to(cuda), wt.to(cuda), b.to(cuda)
    xr, wr = R.bf16_rne(x), R.bf16_rne(wt)
    ref, S = R.conv3x3_ref(xr, wr, b)
    smax = S.max().item()
    # channel sums of the RCAB's second convolution: sum over the tiles = the plane sum of the output
    y, part = ops.conv2d(xd, wd, bd, chan_partial=True, precision="bf16")
    assert part.shape == (n, ops.lib().eavsr_conv3x3_x6s_tiles(h, w), 64)
    assert _err(y, ref) <= CONV_BOUND * smax
    assert _err(part.sum(1), ref.sum((2, 3))) <= CONV_BOUND * S.sum((2, 3)).max().item() + 1e-6 * ref.abs().sum((2, 3)).max().item()
    # the ReLU's backward mask inside the input-gradient convolution (dgrad form: W transposed and flipped, packed in place)
    wdg = wr.flip(2, 3).transpose(0, 1)
    refd, Sd = R.conv3x3_ref(xr, wdg)
    sdmax = Sd.max().item()
    y = ops.conv2d(xd, wd, None, act="relu_mask", residual=t.to(cuda), dgrad=True, precision="bf16")
    assert _err(y, torch.where(t.to(torch.float64) > 0, refd, torch.zeros_like(refd))) <= CONV_BOUND * sdmax
    y = ops.conv2d(xd, wd, None, dgrad=True, precision="bf16")
    assert _err(y, refd) <= CONV_BOUND * sdmax
    # the RCAB backward's last convolution: + d, and the per-row sums of (stored value) x r_prev
    y, rows = ops.conv2d(xd, wd, None, residual=d.to(cuda), dgrad=True, sum_mul=m.to(cuda), precision="bf16")
    want = refd + d.to(torch.float64)
    assert _err(y, want) <= CONV_BOUND * sdmax
    prod = want * m.to(torch.float64)
    bound = CONV_BOUND * (Sd * m.abs().to(torch.float64)).sum((2, 3)).max().item() + 1e-6 * prod.abs().sum((2, 3)).max().item()
    assert _err(rows.sum(1), prod.sum((2, 3))) <= bound


@pytest.mark.parametrize("nseg,shape", [(7, (2, 96, 96)), (3, (3, 40, 64))], ids=["7seg-2x96x96", "3seg-3x40x64"])
def test_wgrad_multi_segment_rne_and_deterministic(ops, cuda, nseg, shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(300 + nseg)
    dys = [_rand(g, n, 64, h, w) for _ in range(nseg)]
    xs = [_rand(g, n, 64, h, w) for _ in range(nseg)]
    dyd, xsd = [t.to(cuda) for t in dys], [[t.to(cuda)] for t in xs]
    assert ops.wgrad_bf16_takes(dyd, xsd, 3)

    def run():
        dw = torch.empty(64, 64, 3, 3, device=cuda)
        db = torch.empty(64, device=cuda)
        ops.conv_wgrad_multi(dyd, xsd, 3, out=dw, bias_out=db, precision="bf16")
        return dw, db

    dw, db = run()
    dw2, db2 = run()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)      # fixed-order reduction, no atomics
    ref, S = R.wgrad3x3_ref([R.bf16_rne(t) for t in dys], [R.bf16_rne(t) for t in xs])
    e = _err(dw, ref)
    assert e <= WGRAD_BOUND * S.max().item(), (e, S.max().item())
    dsum = sum(t.to(torch.float64).sum((0, 2, 3)) for t in dys)
    assert _err(db, dsum) <= 1e-5 * sum(t.abs().to(torch.float64).sum((0, 2, 3)) for t in dys).max().item()   # fp32 bias, not rounded
    if nseg == 3:
        ref_tr, _ = R.wgrad3x3_ref([R.bf16_trunc(t) for t in dys], [R.bf16_trunc(t) for t in xs])
        assert e * 20 <= _err(dw, ref_tr)
        # accumulate=True adds onto what is there
        dw3, db3 = dw.clone(), db.clone()
        ops.conv_wgrad_multi(dyd, xsd, 3, out=dw3, bias_out=db3, accumulate=True, precision="bf16")
        assert torch.allclose(dw3, 2 * dw, rtol=1e-6, atol=1e-6 * dw.abs().max().item())


# ---------------------------------------------------------------------------------------------------------- the mode's reach
def _net(cuda, sd):
    from eavsr_amd.eavsrp_model import EAVSRP
    net = EAVSRP(Namespace(predict=False, n_frame=3, n_flow=5, scale=4), None)
    net.load_state_dict(sd, strict=True)
    return net.to(cuda).train()


def _grads(net, clip, hr, mode):
    from eavsr_amd import autograd as AG
    from eavsr_amd import networks as Nw
    net.zero_grad(set_to_none=True)
    with Nw.train_precision(mode):
        out = net(clip)
        loss = (out - hr).abs().mean()
        with AG.grad_sink():
            loss.backward()
    return out.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def test_mode_engages_in_training_and_stays_contained(ops, cuda):
    from eavsr_amd import networks as Nw
    from eavsr_amd.utils.synthetic import synthetic_clip
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    net = _net(cuda, sd)
    clip, hr = synthetic_clip(1, 3, 64, 64, seed=21).to(cuda), synthetic_clip(1, 3, 256, 256, seed=22).to(cuda)
    out_a, ga = _grads(net, clip, hr, "fp32")
    out_b, gb = _grads(net, clip, hr, "bf16")
    out_c, gc = _grads(net, clip, hr, "fp32")
    assert ga.keys() == gb.keys() == gc.keys() and len(ga) > 0
    # fp32 -> bf16 -> fp32: the fp32 forward is bit-identical (no bf16 packed form served to fp32); its gradients equal up to the
    # float atomics of two scatter kernels of the backward (test_graphed_training_step_matches_eager)
    assert torch.equal(out_a, out_c)
    for k in ga:
        assert (ga[k] - gc[k]).norm().item() <= 1e-5 * max(ga[k].norm().item(), 1e-30), k
    num = sum(((gb[k] - ga[k]).double().norm() ** 2).item() for k in ga) ** 0.5
    den = sum((ga[k].double().norm() ** 2).item() for k in ga) ** 0.5
    assert num / den > 1e-5, num / den       # the mode ran
    rel = {k: ((gb[k] - ga[k]).norm() / ga[k].norm().clamp_min(1e-30)).item() for k in ga}
    gmax = max(ga[k].norm().item() for k in ga)
    big = [k for k in ga if ga[k].norm().item() >= 1e-4 * gmax]
    worst_big = max(rel[k] for k in big)
    worst = max(rel.values())
    print(f"bf16 vs fp32 first-step gradients: total relative {num / den:.3e}; worst of the {len(big)} / {len(ga)} tensors with "
          f"|g| >= 1e-4 max|g| {worst_big:.3e}; worst overall {worst:.3e} ({max(rel, key=rel.get)})")
    # Measured on MI355X: total 3.2e-3; worst of the tensors with |g| >= 1e-4 max|g| 0.35, worst overall 0.58 -- both in the
    # deformable alignment's offset / transform heads, whose gradients are sums with heavy cancellation (1e-8 .. 1e-6 here), where
    # rounding the activations once moves the small remainder.  The 30-step test below shows training is unaffected.
    assert num / den <= 1e-2, num / den
    assert worst_big <= 0.6, (worst_big, sorted(((rel[k], k) for k in big), reverse=True)[:5])
    assert worst <= 1.0, worst
    assert not torch.equal(out_a, out_b)
    # no-grad forwards are not in the mode's scope: bit-identical
    with torch.no_grad():
        with Nw.train_precision("fp32"):
            y32 = net(clip)
        with Nw.train_precision("bf16"):
            y16 = net(clip)
    assert torch.equal(y32, y16)


def _model(sd, lr=1e-4):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    m = EAVSRPModel(Namespace(predict=False, n_frame=3, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=lr, beta1=0.9,
                              beta2=0.999, weight_decay=0.0, npost=350))
    m.netEAVSRP.load_state_dict(sd, strict=True)
    return m


def test_bf16_training_still_trains(ops, cuda):
    from eavsr_amd import networks as Nw
    from eavsr_amd.utils.synthetic import synthetic_clip
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    data = {"lr_seq": synthetic_clip(1, 3, 64, 64, seed=31), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=32), "fname": "x"}
    final = {}
    for mode in ("fp32", "bf16"):
        m = _model(sd)
        losses = []
        with Nw.train_precision(mode):
            for _ in range(30):
                m.set_input(data, epoch=0)
                m.optimize_parameters()
                losses.append(m.get_current_losses()["EAVSRP_L1"])
        assert losses[-1] < losses[0], (mode, losses)
        final[mode] = losses[-1]
    print(f"final L1 after 30 steps: fp32 {final['fp32']:.6f}, bf16 {final['bf16']:.6f}")
    assert abs(final["bf16"] - final["fp32"]) <= 0.02 * final["fp32"], final


def test_graphed_bf16_step_matches_eager_and_recaptures_on_mode_change(ops, cuda):
    from eavsr_amd import networks as Nw
    from eavsr_amd.graph import GraphedTrainStep
    from eavsr_amd.utils.synthetic import synthetic_clip
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    data = {"lr_seq": synthetic_clip(1, 3, 64, 64, seed=1), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=2), "fname": "x"}
    data2 = {"lr_seq": synthetic_clip(1, 3, 64, 64, seed=3), "hr_seq": synthetic_clip(1, 3, 256, 256, seed=4), "fname": "y"}
    on_dev = lambda d: {k: v.to(cuda) for k, v in d.items() if k != "fname"}
    with Nw.train_precision("bf16"):
        eager = _model(sd)
        want = []
        for d in (data, data, data2, data):
            eager.set_input(d, epoch=0)
            eager.optimize_parameters()
            want.append(eager.get_current_losses()["EAVSRP_L1"])
        graphed = _model(sd)
        graphed.set_input(data, epoch=0)
        g = GraphedTrainStep(graphed, warmup=1)
        assert g.precision == "bf16"
        got = []
        for d in (data, data2, data):
            g.step(on_dev(d))
            got.append(graphed.get_current_losses()["EAVSRP_L1"])
        assert all(abs(a - b) <= 2e-5 * max(1.0, abs(b)) for a, b in zip(got, want[1:])), (got, want)
        pe, pg = dict(eager.netEAVSRP.named_parameters()), dict(graphed.netEAVSRP.named_parameters())
        worst = max((pe[k].detach() - pg[k].detach()).abs().max().item() for k in pe)
        assert worst <= 2.5e-4, worst
    # another mode between two replays: the next step recaptures, and its loss is that of an eager fp32 training forward
    snap = {k: v.detach().clone() for k, v in graphed.netEAVSRP.state_dict().items()}
    old = g.graph
    with Nw.train_precision("fp32"):
        ref = _model(snap)
        ref.set_input(data2, epoch=0)
        ref.forward()
        want32 = (ref.data_hr_seq - ref.data_sr_seq).abs().mean().item()
        g.step(on_dev(data2))
        assert g.graph is not old and g.precision == "fp32"
        got32 = graphed.get_current_losses()["EAVSRP_L1"]
    assert abs(got32 - want32) <= 2e-5 * max(1.0, abs(want32)), (got32, want32)
