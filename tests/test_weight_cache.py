"""eavsr_amd.weight_cache.WeightCache on its own: host only, CPU parameters, no library."""
import gc

import torch

from eavsr_amd.weight_cache import WEIGHT_CACHES, WeightCache


def _param(*shape):
    return torch.nn.Parameter(torch.zeros(*shape))


def _bump(p):
    with torch.no_grad():
        p.add_(1.0)


def test_a_new_cache_is_registered_by_its_constructor():
    c = WeightCache()
    assert any(r is c for r in WEIGHT_CACHES)
    assert len(c) == 0


def test_miss_then_hit_returns_the_identical_object():
    c, a, b = WeightCache(), _param(3), _param(3)
    assert c.lookup([a, b]) is None
    value = object()
    assert c.store([a, b], None, value) is value
    assert c.lookup([a, b]) is value and c.lookup((a, b)) is value
    assert c.lookup([b, a]) is None and c.lookup([a]) is None           # the sources in their order, all of them
    assert c.lookup([a, b], "tag") is None


def test_an_inplace_update_misses_and_the_next_store_leaves_one_entry():
    c, a = WeightCache(), _param(3)
    c.store((a,), None, "v0")
    c.store((a,), "f4", "v0 f4")
    assert len(c) == 2
    _bump(a)
    assert c.lookup((a,)) is None and c.lookup((a,), "f4") is None
    c.store((a,), None, "v1")
    assert len(c) == 1 and c.lookup((a,)) == "v1"                        # the stale version went under every tag


def test_stale_entries_go_whatever_their_grouping_and_other_sources_stay():
    c, a, b, other = WeightCache(), _param(3), _param(3), _param(3)
    c.store((a, b), None, "ab v0")
    c.store((b,), "dgrad", "b v0")
    c.store((other,), None, "other")
    _bump(b)
    c.store((b,), None, "b v1")
    assert c.lookup((a, b)) is None and len(c) == 2
    assert c.lookup((other,)) == "other" and c.lookup((b,)) == "b v1"


def test_tags_and_groupings_of_one_source_at_one_version_coexist():
    c, a, b = WeightCache(), _param(3), _param(3)
    c.store((a,), 1, "fp16")
    c.store((a,), 2, "bf16")
    c.store((a,), (0, 64), "slice")
    c.store((a, b), 1, "pair")
    assert len(c) == 4
    assert c.lookup((a,), 1) == "fp16" and c.lookup((a,), 2) == "bf16" and c.lookup((a,), (0, 64)) == "slice"
    assert c.lookup((a, b), 1) == "pair"


def test_a_multi_source_entry_misses_when_one_source_is_another_tensor():
    c, a, b, b2 = WeightCache(), _param(3), _param(3), _param(3)
    c.store((a, b), None, "ab")
    assert c.lookup((a, b2)) is None and c.lookup((b2, b)) is None
    assert c.lookup((a, b)) == "ab"


def test_a_dead_source_takes_its_entries_with_it():
    c, a, b = WeightCache(), _param(3), _param(3)
    c.store((a, b), None, "ab")
    c.store((b,), "t", "b")
    c.store((a,), None, "a")
    del b
    gc.collect()
    assert len(c) == 1 and c.lookup((a,)) == "a"


class _StandIn:
    """a different object whose key collides with a tensor's: what a freed tensor's reused id looks like to the dict"""

    def __init__(self, t):
        self._id, self._version = id(t), t._version


def test_a_key_collision_with_another_object_is_a_miss(monkeypatch):
    import builtins
    import eavsr_amd.weight_cache as wc
    c, a = WeightCache(), _param(3)
    c.store((a,), None, "a")
    stand_in = _StandIn(a)
    real_id = builtins.id
    monkeypatch.setattr(wc, "id", lambda o: o._id if isinstance(o, _StandIn) else real_id(o), raising=False)
    key = (None, (wc.id(stand_in), stand_in._version))
    assert key in c._d                                                   # the dict alone would call this a hit
    assert c.lookup((stand_in,)) is None
    assert c.lookup((a,)) == "a"


def test_clear_and_snapshot():
    c, a = WeightCache(), _param(3)
    value = object()
    c.store((a,), None, value)
    snap = c.snapshot()
    c.clear()
    assert len(c) == 0 and c.lookup((a,)) is None
    assert len(snap) == 1 and next(iter(snap.values()))[1] is value      # a snapshot keeps what it saw


def _counting(values):
    """make() for derive: hands out `values` in turn and counts its calls"""
    calls = []

    def make():
        calls.append(len(calls))
        return values[len(calls) - 1]
    return make, calls


def test_derive_makes_once_on_a_miss_and_never_on_a_hit():
    c, a, b = WeightCache(), _param(3), _param(3)
    first = object()
    make, calls = _counting([first, object()])
    assert c.derive([a, b], None, make) is first and calls == [0]
    assert c.lookup([a, b]) is first                                     # the returned object is the stored one
    assert c.derive([a, b], None, make) is first and c.derive((a, b), None, make) is first
    assert calls == [0] and len(c) == 1


def test_derive_makes_again_after_a_version_bump_and_under_another_tag():
    c, a = WeightCache(), _param(3)
    values = [object(), object(), object()]
    make, calls = _counting(values)
    assert c.derive((a,), None, make) is values[0]
    assert c.derive((a,), "f4", make) is values[1] and len(calls) == 2   # another tag: a form of its own
    assert c.derive((a,), None, make) is values[0] and c.derive((a,), "f4", make) is values[1] and len(calls) == 2
    _bump(a)
    assert c.derive((a,), None, make) is values[2] and len(calls) == 3
    assert len(c) == 1 and c.lookup((a,)) is values[2]                   # the stale version went under every tag


def test_derive_looks_up_first_and_stores_right_behind_make(monkeypatch):
    c, a = WeightCache(), _param(3)
    order = []
    lookup, store = c.lookup, c.store
    monkeypatch.setattr(c, "lookup", lambda *k: (order.append("lookup"), lookup(*k))[1])
    monkeypatch.setattr(c, "store", lambda *k: (order.append("store"), store(*k))[1])
    value = c.derive((a,), 1, lambda: order.append("make") or "v")
    assert value == "v" and order == ["lookup", "make", "store"]
    assert c.derive((a,), 1, lambda: order.append("make") or "w") == "v" and order == ["lookup", "make", "store", "lookup"]


def test_a_raising_make_stores_nothing_and_propagates():
    c, a, b = WeightCache(), _param(3), _param(3)
    c.store((b,), None, "b")

    def make():
        raise NotImplementedError("unsupported shape")
    try:
        c.derive((a,), None, make)
    except NotImplementedError as e:
        assert "unsupported shape" in str(e)
    else:
        raise AssertionError("derive swallowed the exception of make()")
    assert len(c) == 1 and c.lookup((a,)) is None and c.lookup((b,)) == "b"
    assert c.derive((a,), None, lambda: "a") == "a" and len(c) == 2       # nothing poisoned: the next derivation goes through
