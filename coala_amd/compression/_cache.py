"""The two caches of the codec's host path. Both key by id(), which Python reuses once an object is freed: a
hit is served only after an identity check against the very object(s) the entry was made for."""
import threading
import weakref
from collections import OrderedDict
from operator import is_


class IdentityCache:
    """At most `limit` values, make(*args), keyed by the identity of one object, or of each object of a tuple (the
    empty tuple: by `extra` alone), plus hashable extras. ANY tuple means "these objects": a key object that is itself
    a tuple goes in as (obj,). An entry holds its key objects strongly, so a live entry's id cannot be reused. Reads
    take no lock; inserts take the cache's own and evict the oldest."""

    def __init__(self, limit):
        self.limit, self._d, self._lock = limit, OrderedDict(), threading.Lock()

    def __len__(self):
        return len(self._d)

    def get(self, objs, extra=(), make=None, *args):
        many = type(objs) is tuple
        key = (extra, *map(id, objs)) if many else (extra, id(objs))
        hit = self._d.get(key)
        if hit is not None and (all(map(is_, hit[0], objs)) if many else hit[0] is objs):
            return hit[1]
        value = make(*args)  # (arguments, not a closure: a hit then builds no function object)
        with self._lock:
            self._d[key] = (objs, value)
            while len(self._d) > self.limit:
                self._d.popitem(last=False)
        return value


class WeakIdCache:
    """id(obj) -> (weakref to obj, value): one value, make(obj) (never None), per live object, built under the cache's
    own lock; entries of dead objects are swept once there are more than `sweep_at`. still_valid(value) false builds
    the value again. Reads, still_valid included, take no lock: it must be safe to run from several threads."""

    def __init__(self, sweep_at, still_valid=None):
        self.sweep_at, self._valid, self._d, self._lock = sweep_at, still_valid, {}, threading.RLock()

    def __len__(self):
        return len(self._d)

    def values(self):
        return [v for _, v in list(self._d.values())]

    def _live(self, obj):
        hit = self._d.get(id(obj))
        if hit is not None and hit[0]() is obj and (self._valid is None or self._valid(hit[1])):
            return hit[1]

    def get(self, obj, make):
        hit = self._d.get(id(obj))  # (_live, in line: this is on every encode's and decode's path)
        if hit is not None and hit[0]() is obj and (self._valid is None or self._valid(hit[1])):
            return hit[1]
        with self._lock:
            value = self._live(obj)  # (another thread built it meanwhile: one value per object)
            if value is None:
                value = self.set(obj, make(obj))
        return value

    def set(self, obj, value):
        """Replace obj's value (one its user found stale)."""
        with self._lock:  # (re-entrant: get holds it already)
            self._d[id(obj)] = (weakref.ref(obj), value)
            if len(self._d) > self.sweep_at:
                for k in [k for k, (r, _) in self._d.items() if r() is None]:
                    del self._d[k]
        return value
