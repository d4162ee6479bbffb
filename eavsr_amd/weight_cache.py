"""The one cache of forms DERIVED from parameters (packed / transformed / split / transposed weights, concatenated biases).

An entry is keyed by the (id, _version) of every tensor it was derived from plus a variant tag, holds weak references to
those tensors and counts as a hit only if each reference still points at the very tensor asked for: a freed tensor whose
id is reused can never produce a stale hit.  nn.Parameters live as long as their module, so the hot path always hits.
Every instance is in WEIGHT_CACHES from its construction on: graph.clear_weight_caches() empties them all around a capture
(a replayed graph updates the parameters without bumping `_version`)."""
import weakref

WEIGHT_CACHES = []


class WeightCache:
    def __init__(self):
        self._d = {}        # (tag, (id, version) per source) -> (weakref per source, value)
        WEIGHT_CACHES.append(self)

    def __len__(self):
        return len(self._d)

    def clear(self):
        self._d.clear()

    def snapshot(self):
        """the entries as a dict of its own: whoever holds it keeps their values alive (a captured graph reads them)"""
        return dict(self._d)

    def lookup(self, sources, tag=None):
        """the value stored for these tensors (a sequence, in order) at their current versions under `tag`, or None"""
        hit = self._d.get((tag, *[(id(t), t._version) for t in sources]))
        if hit is None:
            return None
        for r, t in zip(hit[0], sources):
            if r() is not t:
                return None
        return hit[1]

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
        d[key] = (tuple(weakref.ref(t, lambda _r: d.pop(key, None)) for t in sources), value)
        return value
