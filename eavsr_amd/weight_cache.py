"""The one cache of forms DERIVED from parameters (packed / transformed / split / transposed weights, concatenated biases).

An entry is keyed by the (id, _version) of every tensor it was derived from plus a variant tag, holds weak references to
those tensors and counts as a hit only if each reference still points at the very tensor asked for: a freed tensor whose
id is reused can never produce a stale hit.  nn.Parameters live as long as their module, so the hot path always hits.
Every instance is in WEIGHT_CACHES from its construction on: graph.clear_weight_caches() empties them all around a capture
(a replayed graph updates the parameters without bumping `_version`).

Stream order.  A value is derived by kernels queued on the stream that was current at its `store`; until they have run, the
buffer holds whatever the allocator left in it.  `store` therefore remembers that stream and an event recorded on it.  A hit on
the deriving stream costs one comparison.  A `lookup` from ANOTHER stream makes that stream wait for the event -- until one
lookup finds it complete, after which nobody waits again -- and, the first time each such stream asks, tells the allocator that
the value is in use there (`record_stream`), so that an evicted value is not handed out again under a reader's feet.  That is
why an entry keeps its stream order after the event has completed: a lookup from another stream goes on paying for the current
stream's handle and a set lookup (no driver call), which is the price of protecting a stream that asks for the first time later;
dropping the order then would make such hits free and leave that stream unprotected.  Host values
and CPU tensors take none of this path.  While the current stream is capturing, `store` records nothing and `lookup` waits for
nothing: a dependency may not cross a capture boundary, and whoever captures synchronises the device between warm-up and
capture (graph.py)."""
import weakref

import torch

WEIGHT_CACHES = []


def _device_tensors(value):
    """the CUDA tensors of a cached value: the value itself, or the members of a tuple / list of them"""
    vs = value if isinstance(value, (tuple, list)) else (value,)
    return [v for v in vs if isinstance(v, torch.Tensor) and v.is_cuda]


class WeightCache:
    def __init__(self):
        self._d = {}        # (tag, (id, version) per source) -> (weakref per source, value, None or the stream order of its derivation)
        WEIGHT_CACHES.append(self)

    def __len__(self):
        return len(self._d)

    def clear(self):
        self._d.clear()

    def snapshot(self):
        """the entries as a dict of its own: whoever holds it keeps their values alive (a captured graph reads them)"""
        return dict(self._d)

    def lookup(self, sources, tag=None):
        """the value stored for these tensors (a sequence, in order) at their current versions under `tag`, or None; the
        current stream is ordered after the value's derivation"""
        key = (tag, *[(id(t), t._version) for t in sources])
        hit = self._d.get(key)
        if hit is None:
            return None
        for r, t in zip(hit[0], sources):
            if r() is not t:
                return None
        if hit[2] is not None:
            self._order_after_derivation(hit)
        return hit[1]

    @staticmethod
    def _order_after_derivation(hit):
        order = hit[2]      # [the deriving stream's handle, its device, the event or None once seen complete, handles of the streams recorded]
        cur = torch.cuda.current_stream(order[1])
        if cur.cuda_stream == order[0]:
            return
        if torch.cuda.is_current_stream_capturing():      # (before the event is touched: it may not be queried under a global capture)
            return
        if order[2] is not None:
            if order[2].query():
                order[2] = None
            else:
                cur.wait_event(order[2])
        if cur.cuda_stream not in order[3]:
            order[3].add(cur.cuda_stream)
            for v in _device_tensors(hit[1]):
                v.record_stream(cur)

    def store(self, sources, tag, value):
        """Insert `value` and return it.  Drops every entry, whatever its tag, that holds one of `sources` at another version;
        the new entry goes when any of its sources dies."""
        d = self._d
        key = (tag, *[(id(t), t._version) for t in sources])
        cur = dict(key[1:])
        # (over a copy of the keys: the weak-reference callbacks below pop entries whenever the collector frees a source, also
        #  in the middle of this loop -- "dictionary changed size during iteration")
        for k in [k for k in tuple(d) if any(cur.get(i, v) != v for i, v in k[1:])]:
            d.pop(k, None)
        order = None
        on_device = _device_tensors(value)
        if on_device and not torch.cuda.is_current_stream_capturing():
            stream = torch.cuda.current_stream(on_device[0].device)
            event = torch.cuda.Event()
            event.record(stream)
            order = [stream.cuda_stream, on_device[0].device, event, set()]
        d[key] = (tuple(weakref.ref(t, lambda _r: d.pop(key, None)) for t in sources), value, order)
        return value

    def derive(self, sources, tag, make):
        """`lookup(sources, tag)`, or on a miss `store(sources, tag, make())`: `make` derives the value on the current stream and
        the store's event is recorded right behind it, with nothing in between.  If `make` raises, nothing is stored."""
        hit = self.lookup(sources, tag)
        if hit is not None:
            return hit
        return self.store(sources, tag, make())
