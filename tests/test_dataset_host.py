"""The device-resident training data (eavsr_amd/dataset.py, ops.gather_pairs, csrc/batch.hip), what needs no GPU: the host logic that
decides what the gather kernel gathers -- `draw_item` against a literal replay of the reference's calls on `random`, `epoch_plan`'s
permutation / sharding / windows / crops -- and every validation error, raised before a device is touched."""
import os
import random
import re

import numpy as np
import pytest
import torch

from eavsr_amd import dataset as D
from eavsr_amd import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_draws(rng, ih, iw, patch):
    """data/realvsr_dataset.py:166-169 `_crop_patch`, then util/util.py:242-245 `augment_basic`, call for call"""
    pw = rng.randrange(0, iw - patch + 1)
    ph = rng.randrange(0, ih - patch + 1)
    hflip = rng.random() < 0.5
    vflip = rng.random() < 0.5
    rot90 = rng.random() < 0.5
    return ph, pw, hflip, vflip, rot90


@pytest.mark.parametrize("ih,iw,patch", [(70, 101, 50), (128, 256, 96), (64, 64, 64), (64, 200, 64), (300, 96, 96), (5, 7, 1)])
def test_draw_item_replays_the_reference_call_order(ih, iw, patch):
    for seed in range(40):
        top, left, flags = D.draw_item(random.Random(seed), ih, iw, patch)
        ph, pw, hflip, vflip, rot90 = _reference_draws(random.Random(seed), ih, iw, patch)
        assert (top, left) == (ph, pw), seed
        assert flags == (1 if hflip else 0) | (2 if vflip else 0) | (4 if rot90 else 0), seed
        assert 0 <= top <= ih - patch and 0 <= left <= iw - patch
    # the generator is left where the reference leaves it: the next item continues the same stream
    a, b = random.Random(7), random.Random(7)
    D.draw_item(a, ih, iw, patch)
    _reference_draws(b, ih, iw, patch)
    assert a.random() == b.random()


def test_draw_item_with_a_single_valid_origin():
    seen = set()
    for seed in range(64):
        top, left, flags = D.draw_item(random.Random(seed), 48, 48, 48)
        assert (top, left) == (0, 0)
        seen.add(flags)
    assert seen == set(range(8))      # all eight flip combinations occur
    with pytest.raises(ValueError, match="does not fit"):
        D.draw_item(random.Random(0), 48, 48, 49)


PLAN = dict(n_items=60, n_frame=7, n_seq=20, batch_size=4, ih=70, iw=101, patch=50, seed=11, epoch=3)


def _keys(frames, n_frame):
    return frames[..., n_frame // 2].reshape(-1).tolist()      # the centre of a window is its key frame, mirrored or not


def test_epoch_plan_is_a_function_of_its_arguments():
    f1, d1, n1 = D.epoch_plan(**PLAN)
    f2, d2, n2 = D.epoch_plan(**PLAN)
    assert f1.dtype == np.int32 and d1.dtype == np.int32
    assert f1.shape == (15, 4, 7) and d1.shape == (15, 4, 4) and len(n1) == 15 and all(len(b) == 4 for b in n1)
    assert np.array_equal(f1, f2) and np.array_equal(d1, d2) and n1 == n2
    f3, d3, _ = D.epoch_plan(**{**PLAN, "epoch": 4})
    assert not np.array_equal(f1, f3) and not np.array_equal(d1, d3)
    f4, _, _ = D.epoch_plan(**{**PLAN, "seed": 12})
    assert not np.array_equal(f1, f4)
    assert sorted(_keys(f1, 7)) == list(range(60))      # 60 = 15 x 4: nothing dropped, every frame is a key frame once
    assert n1[0][0] == D.default_name(_keys(f1, 7)[0], 20) and re.fullmatch(r"\d{3}_\d{5}\.png", n1[0][0])
    names = [f"n{i}" for i in range(60)]
    assert D.epoch_plan(**PLAN, names=names)[2][2][1] == f"n{_keys(f1, 7)[2 * 4 + 1]}"
    assert (d1[..., 3] == 0).all()


@pytest.mark.parametrize("world,batch_size", [(1, 4), (2, 4), (3, 7), (4, 8), (7, 2)])
def test_epoch_plan_ranks_are_disjoint_and_cover_all_but_the_dropped_tail(world, batch_size):
    kw = {**PLAN, "batch_size": batch_size}
    per_rank = (60 // world) // batch_size * batch_size
    seen = []
    for rank in range(world):
        frames, desc, names = D.epoch_plan(**kw, rank=rank, world=world)
        assert frames.shape == (per_rank // batch_size, batch_size, 7)      # every rank the same number of whole batches
        seen += _keys(frames, 7)
    assert len(seen) == len(set(seen)) == per_rank * world
    assert set(seen) <= set(range(60)) and 60 - len(seen) < world * batch_size + world      # only a tail is dropped


@pytest.mark.parametrize("n_frame,n_seq", [(7, 20), (5, 5), (3, 10), (1, 4)])
def test_epoch_plan_windows_are_train_window_and_stay_in_their_scene(n_frame, n_seq):
    n_items = 3 * n_seq
    frames, desc, _ = D.epoch_plan(n_items, n_frame, n_seq, 1, 70, 101, 50, seed=5, epoch=0)
    assert frames.shape[0] == n_items
    for win in frames.reshape(-1, n_frame).tolist():
        key = win[n_frame // 2]
        assert win == harness.train_window(key, key % n_seq, n_frame, n_seq)
        assert {k // n_seq for k in win} == {key // n_seq}
    assert (desc[..., 0] >= 0).all() and (desc[..., 0] <= 70 - 50).all()
    assert (desc[..., 1] >= 0).all() and (desc[..., 1] <= 101 - 50).all()
    assert ((desc[..., 2] >= 0) & (desc[..., 2] < 8)).all()
    assert len({tuple(r) for r in desc.reshape(-1, 4).tolist()}) > n_items // 2      # items do not share one draw
    D.check_plan(frames, desc, n_items, 70, 101, 50)


def test_an_items_crop_does_not_depend_on_world_or_batch_size():
    def by_key(**kw):
        out = {}
        for rank in range(kw.get("world", 1)):
            frames, desc, _ = D.epoch_plan(**{**PLAN, **kw}, rank=rank)
            for k, d in zip(_keys(frames, 7), desc.reshape(-1, 4).tolist()):
                out[k] = tuple(d)
        return out
    base = by_key()
    assert len(base) == 60
    for kw in (dict(world=2), dict(world=3, batch_size=5), dict(batch_size=1), dict(batch_size=6, world=5)):
        other = by_key(**kw)
        assert len(other) >= 50 and all(base[k] == v for k, v in other.items()), kw


def test_epoch_plan_and_check_plan_refuse_what_the_kernel_would_have_to_clamp():
    with pytest.raises(ValueError, match="does not fit"):
        D.epoch_plan(**{**PLAN, "patch": 71})
    with pytest.raises(ValueError, match="whole scenes"):
        D.epoch_plan(**{**PLAN, "n_items": 61})
    with pytest.raises(ValueError, match="rank"):
        D.epoch_plan(**PLAN, rank=2, world=2)
    frames, desc, _ = D.epoch_plan(**PLAN)
    D.check_plan(frames, desc, 60, 70, 101, 50)
    bad = frames.copy()
    bad[0, 0, 0] = 60
    with pytest.raises(ValueError, match="frame indices"):
        D.check_plan(bad, desc, 60, 70, 101, 50)
    bad = desc.copy()
    bad[1, 2, 0] = 21
    with pytest.raises(ValueError, match="leaves the"):
        D.check_plan(frames, bad, 60, 70, 101, 50)
    bad = desc.copy()
    bad[1, 2, 1] = -1
    with pytest.raises(ValueError, match="leaves the"):
        D.check_plan(frames, bad, 60, 70, 101, 50)
    bad = desc.copy()
    bad[0, 0, 2] = 8
    with pytest.raises(ValueError, match="flags"):
        D.check_plan(frames, bad, 60, 70, 101, 50)
    with pytest.raises(ValueError, match="does not fit"):
        D.check_plan(frames, desc, 60, 70, 101, (71, 50))
    # transpose with a non-square patch: refused with the flag, taken without it
    flat = np.zeros_like(desc)
    D.check_plan(frames, flat, 60, 70, 101, (40, 50))
    flat[3, 1, 2] = 4
    with pytest.raises(ValueError, match="square patch"):
        D.check_plan(frames, flat, 60, 70, 101, (40, 50))
    with pytest.raises(ValueError, match="int32"):
        D.check_plan(frames.astype(np.int64), desc, 60, 70, 101, 50)


def test_frame_pairs_validation_happens_before_anything_moves_to_a_device():
    lr = np.zeros((8, 3, 10, 12), np.uint8)
    hr = np.zeros((8, 3, 20, 24), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        D.FramePairs(lr.astype(np.float32), hr, 2, 4)
    with pytest.raises(ValueError, match="uint8"):
        D.FramePairs(torch.zeros(8, 3, 10, 12), torch.from_numpy(hr), 2, 4)
    with pytest.raises(ValueError, match="scale 2 x lr"):
        D.FramePairs(lr, np.zeros((8, 3, 20, 25), np.uint8), 2, 4)
    with pytest.raises(ValueError, match="scale 4 x lr"):
        D.FramePairs(lr, hr, 4, 4)
    with pytest.raises(ValueError, match="scale 2 x lr"):
        D.FramePairs(lr, hr[:4], 2, 4)
    with pytest.raises(ValueError, match="whole scenes"):
        D.FramePairs(lr, hr, 2, 3)
    with pytest.raises(ValueError, match="names"):
        D.FramePairs(lr, hr, 2, 4, names=["a"])
    with pytest.raises(ValueError, match="scale 2 x lr"):      # interleaved LR against planes HR of another size
        D.FramePairs(np.zeros((8, 10, 12, 3), np.uint8), np.zeros((8, 3, 20, 26), np.uint8), 2, 4)
    with pytest.raises(TypeError):
        D.FramePairs([1, 2], hr, 2, 4)
    # a host store can be built (device='cpu') but not gathered from: there is no CPU path
    store = D.FramePairs(np.zeros((8, 10, 12, 3), np.uint8), hr, 2, 4, device="cpu")
    assert tuple(store.lr.shape) == (8, 3, 10, 12) and store.frame_size == (10, 12) and len(store) == 8
    assert store.names[5] == "001_00001.png"
    with pytest.raises(RuntimeError, match="GPU only"):
        next(iter(D.TrainBatches(store, 2, 8, 3)))
    with pytest.raises(ValueError, match="does not fit"):
        D.TrainBatches(store, 2, 11, 3)
    with pytest.raises(ValueError, match="does not fit"):
        D.val_items(store, 3, p=12)
    with pytest.raises(ValueError, match="odd margin"):
        D.val_items(store, 3, p=7)
    with pytest.raises(ValueError, match="not a multiple"):
        D.test_items(store, 3)


def test_gather_pairs_refuses_cpu_tensors_and_bad_shapes_without_touching_a_device():
    from eavsr_amd import ops
    lr = torch.zeros(4, 3, 10, 12, dtype=torch.uint8)
    hr = torch.zeros(4, 3, 20, 24, dtype=torch.uint8)
    frames = torch.zeros(2, 3, dtype=torch.int32)
    desc = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gather_pairs(lr, hr, frames, desc, 8, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.gather_pairs(lr, None, frames, desc, 8, 2)
    with pytest.raises(TypeError):
        ops.gather_pairs([1], hr, frames, desc, 8, 2)
    # the shape checks, on 'meta' tensors made to look like device tensors: no device exists here, and none is needed
    class OnDevice(torch.Tensor):
        is_cuda = True
    dev = lambda t: t.to("meta").as_subclass(OnDevice)
    with pytest.raises(ValueError, match="square patch"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames), dev(desc), (8, 6), 2)
    with pytest.raises(ValueError, match="does not fit"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames), dev(desc), 11, 2)
    with pytest.raises(ValueError, match="does not fit"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames), dev(desc), (8, 13), 2, may_transpose=False)
    with pytest.raises(ValueError, match="hr_store"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames), dev(desc), 8, 4)
    with pytest.raises(ValueError, match="lr_store"):
        ops.gather_pairs(dev(lr.float()), dev(hr), dev(frames), dev(desc), 8, 2)
    with pytest.raises(ValueError, match="int32"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames.long()), dev(desc), 8, 2)
    with pytest.raises(ValueError, match="int32"):
        ops.gather_pairs(dev(lr), dev(hr), dev(frames), dev(torch.zeros(3, 4, dtype=torch.int32)), 8, 2)


def test_the_entry_point_is_in_the_stable_header_and_checks_its_arguments_on_the_host():
    from eavsr_amd import _native
    header = open(os.path.join(ROOT, "include", "eavsr_hip.h")).read()
    stable = header.split(" * EXPERIMENTAL -- exported by the LAB build only")[0]
    assert "eavsr_gather_pairs_u8" in _native.SIGNATURES and re.search(r"^int eavsr_gather_pairs_u8\(", stable, flags=re.M)
    lib = _native.load()
    g = lib.eavsr_gather_pairs_u8
    # (lr_store, hr_store, frames, desc, lr_out, hr_out, F, n, t, C, h, w, s, ph, pw, stream); every call returns before a launch
    assert g(None, None, 16, 16, 16, None, 4, 1, 3, 3, 10, 12, 2, 8, 8, None) == -1 and b"NULL" in lib.eavsr_last_error()
    assert g(16, 16, 16, 16, 16, None, 4, 1, 3, 3, 10, 12, 2, 8, 8, None) == -1      # an HR store without an HR output
    assert g(16, None, 16, 16, 16, None, 4, 1, 3, 3, 10, 12, 2, 11, 8, None) == -2 and b"does not fit" in lib.eavsr_last_error()
    assert g(16, None, 16, 16, 16, None, 4, 1, 3, 3, 10, 12, 2, 8, 13, None) == -2
    assert g(16, None, 16, 16, 16, None, 0, 1, 3, 3, 10, 12, 2, 8, 8, None) == -2       # an empty store
    assert g(18, None, 16, 16, 16, None, 4, 1, 3, 3, 10, 12, 2, 8, 8, None) == -2 and b"4-byte" in lib.eavsr_last_error()
    assert g(16, None, 16, 16, 20, None, 4, 1, 3, 3, 10, 12, 2, 8, 8, None) == -2 and b"16-byte" in lib.eavsr_last_error()
    assert g(16, None, 16, 16, 16, None, 4, 30000, 3, 3, 10, 12, 2, 8, 8, None) == -2 and b"planes" in lib.eavsr_last_error()
    assert g(16, None, 16, 16, 16, None, 4, 0, 3, 3, 10, 12, 2, 8, 8, None) == 0        # an empty batch: nothing is launched


def test_the_kernel_source_is_plain_hip():
    """no inline assembly in csrc/batch.hip (the issue's source-hygiene condition; the build scans for the rest)"""
    src = open(os.path.join(ROOT, "eavsr_amd", "csrc", "batch.hip")).read()
    assert "asm" not in src.replace("assembly", "")
    assert "/ 255.0f" in src and "1.0f / 255" not in src      # a division, not a reciprocal
