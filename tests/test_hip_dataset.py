"""The device-resident training data on the GPU (`pytest -m gpu`): ops.gather_pairs (csrc/batch.hip) and eavsr_amd/dataset.py.

The expected value everywhere is `_restate` (tests/helpers.py restate_pairs), a numpy restatement of the reference's item, in the reference's
order: crop -> [:, :, ::-1] -> [:, ::-1, :] -> transpose(0, 2, 1) -> np.float32(.) / 255 (data/realvsr_dataset.py:166-175,
util/util.py:223-227).  The comparison is torch.equal, bit for bit: bytes in, one correctly rounded division out -- there is no
tolerance to choose."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.helpers import restate_pairs as _restate

pytestmark = pytest.mark.gpu


def _stores(F, C, h, w, s, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (F, C, h, w), dtype=np.uint8), rng.integers(0, 256, (F, C, s * h, s * w), dtype=np.uint8)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(got, want):
    assert tuple(got.shape) == want.shape and got.dtype == torch.float32
    got = got.cpu()
    want = torch.from_numpy(want)
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        raise AssertionError(f"{bad.shape[0]} of {want.numel()} samples differ, first at {bad[0].tolist()}: "
                             f"{got[tuple(bad[0])].item()!r} vs {want[tuple(bad[0])].item()!r}")


# ------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("C,h,w,patch,s", [(3, 110, 133, 96, 4), (3, 70, 101, 64, 2), (3, 70, 101, 50, 2), (3, 70, 101, 50, 4),
                                           (1, 70, 101, 64, 4), (1, 59, 67, 50, 2)],
                         ids=["p96x4", "p64x2", "p50x2-tail", "p50x4-tail", "gray-p64x4", "gray-p50x2-tail"])
def test_every_flag_combination_at_every_alignment(cuda, C, h, w, patch, s):
    """all 8 flag combinations x left = 0, 1, 2, 3 (mod 4) and the last valid column x top = 0 and the last valid row, one sample
    each, in one launch; the frame widths are not multiples of 4, so the row starts are unaligned as well"""
    from eavsr_amd import ops
    assert w % 4 != 0
    lr, hr = _stores(3, C, h, w, s, seed=patch + s)
    rows = [(top, left, flags) for flags in range(8) for left in (0, 1, 2, 3, w - patch) for top in (0, h - patch)]
    assert {l % 4 for _, l, _ in rows} == {0, 1, 2, 3}
    desc = np.zeros((len(rows), 4), np.int32)
    desc[:, :3] = rows
    frames = (np.arange(len(rows), dtype=np.int32) % 3).reshape(-1, 1)
    got_lr, got_hr = ops.gather_pairs(_dev(lr, cuda), _dev(hr, cuda), _dev(frames, cuda), _dev(desc, cuda), patch, s)
    _same(got_lr, _restate(lr, frames, desc, patch, patch))
    _same(got_hr, _restate(hr, frames, desc, patch, patch, s))


def test_a_non_square_patch_without_the_transpose(cuda):
    from eavsr_amd import ops
    lr, hr = _stores(2, 3, 70, 101, 2, seed=1)
    ph, pw = 40, 52
    rows = [(top, left, flags) for flags in range(4) for left in (0, 3, 101 - pw) for top in (0, 70 - ph)]
    desc = np.zeros((len(rows), 4), np.int32)
    desc[:, :3] = rows
    frames = np.ones((len(rows), 2), np.int32) * np.array([[1, 0]], np.int32)
    args = (_dev(lr, cuda), _dev(hr, cuda), _dev(frames, cuda), _dev(desc, cuda), (ph, pw), 2)
    with pytest.raises(ValueError, match="square patch"):
        ops.gather_pairs(*args)
    got_lr, got_hr = ops.gather_pairs(*args, may_transpose=False)
    _same(got_lr, _restate(lr, frames, desc, ph, pw))
    _same(got_hr, _restate(hr, frames, desc, ph, pw, 2))


def test_mixed_flags_in_one_batch_with_mirrored_windows_and_without_hr(cuda):
    from eavsr_amd import harness, ops
    n_seq, t = 10, 7
    lr, hr = _stores(2 * n_seq, 3, 70, 101, 4, seed=2)
    keys = [0, 9, 12, 18]      # front of scene 0, back of scene 0, front and back of scene 1: every window is mirrored
    frames = np.asarray([harness.train_window(k, k % n_seq, t, n_seq) for k in keys], np.int32)
    assert all(len(set(win)) < t for win in frames.tolist())
    desc = np.asarray([[3, 5, 5, 0], [0, 37, 2, 0], [6, 1, 7, 0], [2, 18, 0, 0]], np.int32)
    with ops.profile() as prof:
        got_lr, got_hr = ops.gather_pairs(_dev(lr, cuda), _dev(hr, cuda), _dev(frames, cuda), _dev(desc, cuda), 64, 4)
    summary = prof.summary()
    assert list(summary) == ["gather_pairs_u8"] and summary["gather_pairs_u8"]["calls"] == 1      # LR and HR: one launch
    assert summary["gather_pairs_u8"]["bytes"] == 5.0 * (got_lr.numel() + got_hr.numel())
    _same(got_lr, _restate(lr, frames, desc, 64, 64))
    _same(got_hr, _restate(hr, frames, desc, 64, 64, 4))
    only_lr, none = ops.gather_pairs(_dev(lr, cuda), None, _dev(frames, cuda), _dev(desc, cuda), 64, 4)
    assert none is None
    _same(only_lr, _restate(lr, frames, desc, 64, 64))


def test_an_interleaved_store_equals_the_same_store_in_planes(cuda):
    from eavsr_amd import dataset as D
    lr, hr = _stores(4, 3, 70, 101, 2, seed=3)
    a = D.FramePairs(lr, hr, 2, 4, device=cuda)
    b = D.FramePairs(lr.transpose(0, 2, 3, 1), hr.transpose(0, 2, 3, 1), 2, 4, device=cuda)
    c = D.FramePairs(torch.from_numpy(np.ascontiguousarray(lr.transpose(0, 2, 3, 1))), torch.from_numpy(hr), 2, 4, device=cuda)
    for other in (b, c):
        assert torch.equal(a.lr, other.lr) and torch.equal(a.hr, other.hr) and other.lr.is_contiguous() and other.hr.is_contiguous()
    ba, bb = next(iter(D.TrainBatches(a, 2, 64, 3, seed=4))), next(iter(D.TrainBatches(b, 2, 64, 3, seed=4)))
    assert torch.equal(ba["lr_seq"], bb["lr_seq"]) and torch.equal(ba["hr_seq"], bb["hr_seq"]) and ba["fname"] == bb["fname"]


def test_out_writes_into_the_callers_buffers_and_allocates_nothing(cuda):
    from eavsr_amd import ops
    lr, hr = _stores(3, 3, 70, 101, 2, seed=5)
    frames = np.asarray([[0, 1, 2], [2, 1, 0]], np.int32)
    desc = np.asarray([[1, 2, 4, 0], [5, 30, 3, 0]], np.int32)
    args = (_dev(lr, cuda), _dev(hr, cuda), _dev(frames, cuda), _dev(desc, cuda), 64, 2)
    lr_out = torch.full((2, 3, 3, 64, 64), -1.0, device=cuda)
    hr_out = torch.full((2, 3, 3, 128, 128), -1.0, device=cuda)
    r = ops.gather_pairs(*args, out=(lr_out, hr_out))
    assert r[0] is lr_out and r[1] is hr_out
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(cuda)
    r = ops.gather_pairs(*args, out=(lr_out, hr_out))
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(cuda) == before
    _same(lr_out, _restate(lr, frames, desc, 64, 64))
    _same(hr_out, _restate(hr, frames, desc, 64, 64, 2))
    with pytest.raises(ValueError, match=r"out\[hr\]"):
        ops.gather_pairs(*args, out=(lr_out, hr_out[:, :, :, :64]))
    with pytest.raises(ValueError, match=r"out\[lr\]"):
        ops.gather_pairs(*args, out=(lr_out.double(), hr_out))


def test_a_captured_gather_replays_with_new_descriptors(cuda):
    """one gather_pairs in a torch.cuda.graph (a single linear branch); frames / desc are overwritten in place, then a replay"""
    from eavsr_amd import ops
    lr, hr = _stores(6, 3, 70, 101, 4, seed=6)
    frames0 = np.asarray([[0, 1, 2], [3, 4, 5]], np.int32)
    desc0 = np.asarray([[0, 0, 0, 0], [6, 37, 6, 0]], np.int32)
    frames1 = np.asarray([[5, 4, 3], [1, 0, 1]], np.int32)
    desc1 = np.asarray([[4, 19, 7, 0], [1, 2, 1, 0]], np.int32)
    lr_d, hr_d, fr_d, de_d = _dev(lr, cuda), _dev(hr, cuda), _dev(frames0, cuda), _dev(desc0, cuda)
    lr_out = torch.zeros((2, 3, 3, 64, 64), device=cuda)
    hr_out = torch.zeros((2, 3, 3, 256, 256), device=cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        ops.gather_pairs(lr_d, hr_d, fr_d, de_d, 64, 4, out=(lr_out, hr_out))
    torch.cuda.current_stream(cuda).wait_stream(side)
    torch.cuda.synchronize(cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gather_pairs(lr_d, hr_d, fr_d, de_d, 64, 4, out=(lr_out, hr_out))
    lr_out.zero_()
    hr_out.zero_()
    graph.replay()
    _same(lr_out, _restate(lr, frames0, desc0, 64, 64))
    _same(hr_out, _restate(hr, frames0, desc0, 64, 64, 4))
    fr_d.copy_(_dev(frames1, cuda))
    de_d.copy_(_dev(desc1, cuda))
    graph.replay()
    _same(lr_out, _restate(lr, frames1, desc1, 64, 64))
    _same(hr_out, _restate(hr, frames1, desc1, 64, 64, 4))


# ------------------------------------------------------------------------------------------------------------- the loader
def test_train_batches_equal_the_plan_and_the_restatement_over_two_epochs(cuda):
    from eavsr_amd import dataset as D
    n_seq, t, bs, patch = 6, 5, 3, 48
    lr, hr = _stores(2 * n_seq, 3, 59, 67, 2, seed=7)
    store = D.FramePairs(lr, hr, 2, n_seq, device=cuda)
    batches = D.TrainBatches(store, bs, patch, t, seed=9)
    assert (batches.rank, batches.world) == (0, 1)
    seen = []
    for epoch in (0, 1):
        batches.set_epoch(epoch)
        frames, desc, names = D.epoch_plan(2 * n_seq, t, n_seq, bs, 59, 67, patch, 9, epoch)
        assert len(batches) == frames.shape[0] == 4
        got = list(batches)
        assert len(got) == 4
        for b, batch in enumerate(got):
            assert batch["fname"] == names[b] and batch["lr_seq"].device == store.device
            _same(batch["lr_seq"], _restate(lr, frames[b], desc[b], patch, patch))
            _same(batch["hr_seq"], _restate(hr, frames[b], desc[b], patch, patch, 2))
        seen.append(desc)
    assert not np.array_equal(seen[0], seen[1])
    # a rank of two sees its half of the same epoch
    half = D.TrainBatches(store, bs, patch, t, seed=9, rank=1, world=2)
    frames, desc, _ = D.epoch_plan(2 * n_seq, t, n_seq, bs, 59, 67, patch, 9, 0, rank=1, world=2)
    got = list(half)
    assert len(got) == 2
    _same(got[1]["hr_seq"], _restate(hr, frames[1], desc[1], patch, patch, 2))
    # out=: every batch lands in the caller's buffers
    out = (torch.empty((bs, t, 3, patch, patch), device=cuda), torch.empty((bs, t, 3, 2 * patch, 2 * patch), device=cuda))
    into = D.TrainBatches(store, bs, patch, t, seed=9, out=out)
    frames, desc, _ = D.epoch_plan(2 * n_seq, t, n_seq, bs, 59, 67, patch, 9, 0)
    for b, batch in enumerate(into):
        assert batch["lr_seq"] is out[0] and batch["hr_seq"] is out[1]
        _same(out[0], _restate(lr, frames[b], desc[b], patch, patch))


def test_val_and_test_items_equal_crop_center_and_test_window_starts(cuda):
    from eavsr_amd import dataset as D
    from eavsr_amd import harness
    n_seq, t = 6, 3
    lr, hr = _stores(2 * n_seq, 3, 58, 66, 2, seed=8)
    store = D.FramePairs(lr, hr, 2, n_seq, device=cuda)
    lr_f, hr_f = torch.from_numpy(np.float32(lr) / 255), torch.from_numpy(np.float32(hr) / 255)
    vals = list(D.val_items(store, t, p=40))
    assert len(vals) == 2 * n_seq
    for i, item in enumerate(vals):
        win = harness.train_window(i, i % n_seq, t, n_seq)
        assert item["fname"] == [store.names[k] for k in win]
        assert torch.equal(item["lr_seq"].cpu(), harness.crop_center(lr_f[win], 40)[None])
        assert torch.equal(item["hr_seq"].cpu(), harness.crop_center(hr_f[win], 80)[None])
    tests = list(D.test_items(store, t))
    starts = harness.test_window_starts(2 * n_seq, n_seq, t)
    assert len(tests) == len(starts) == 4
    for item, s0 in zip(tests, starts):
        assert item["fname"] == store.names[s0:s0 + t]
        assert torch.equal(item["lr_seq"].cpu(), lr_f[s0:s0 + t][None]) and torch.equal(item["hr_seq"].cpu(), hr_f[s0:s0 + t][None])
    lr_only = D.FramePairs(lr, None, 2, n_seq, device=cuda)
    first = next(iter(D.test_items(lr_only, t)))
    assert "hr_seq" not in first and torch.equal(first["lr_seq"].cpu(), lr_f[:t][None])


# ------------------------------------------------------------------------------------------------------------- into the model
def _model(sd):
    from eavsr_amd.eavsrp_model import EAVSRPModel
    opt = Namespace(predict=False, n_frame=3, n_flow=5, scale=4, isTrain=True, gpu_ids=[0], lr=1e-4, beta1=0.9, beta2=0.999,
                    weight_decay=0.0, npost=350, load_path="")
    m = EAVSRPModel(opt)
    m.netEAVSRP.load_state_dict(sd, strict=True)
    return m


def test_a_training_step_takes_the_batches_and_is_bitwise_the_step_on_the_restatement(cuda):
    """x4, patch 64, n = 1, t = 3: the loss of a step fed by TrainBatches is finite and, in the deterministic mode, bit-identical to
    the loss of the same step fed by the numpy restatement uploaded as fp32"""
    from eavsr_amd import dataset as D
    from eavsr_amd import networks as Nw
    n_seq, t, patch = 6, 3, 64
    rng = np.random.default_rng(10)
    # smooth frames (a random field would do for the equality, but a loss on noise says little): a few low frequencies, quantised
    yy, xx = np.mgrid[0:4 * 70, 0:4 * 101].astype(np.float32)
    hr = np.stack([np.stack([127.5 + 100 * np.sin(yy / (9 + f + c) + rng.uniform(0, 6)) * np.cos(xx / (13 + 2 * c) + f) for c in range(3)])
                   for f in range(n_seq)]).clip(0, 255).astype(np.uint8)
    lr = hr[:, :, 1::4, 2::4].copy()
    store = D.FramePairs(lr, hr, 4, n_seq, device=cuda)
    batch = next(iter(D.TrainBatches(store, 1, patch, t, seed=12)))
    frames, desc, names = D.epoch_plan(n_seq, t, n_seq, 1, 70, 101, patch, 12, 0)
    assert batch["fname"] == names[0] and tuple(batch["lr_seq"].shape) == (1, 3, 3, 64, 64) and tuple(batch["hr_seq"].shape) == (1, 3, 3, 256, 256)
    restated = {"lr_seq": torch.from_numpy(_restate(lr, frames[0], desc[0], patch, patch)).to(cuda),
                "hr_seq": torch.from_numpy(_restate(hr, frames[0], desc[0], patch, patch, 4)).to(cuda), "fname": names[0]}
    sd = H.filled(H.model_shapes("x4"), "trained_like")
    losses = []
    with Nw.deterministic(True):
        for data in (batch, restated):
            m = _model(sd)
            m.set_input(data)
            m.optimize_parameters()
            losses.append(m.loss_EAVSRP_L1.detach().clone())
    assert torch.isfinite(losses[0]).item() and losses[0].item() > 0
    assert torch.equal(losses[0], losses[1]), (losses[0].item(), losses[1].item())
