"""The two id()-keyed caches of the codec's host path (coala_amd/compression/_cache.py): an id() reused after
garbage collection must never serve another object's value; and the seams of the codec.py split — the carrier's
pickle name, validate.py without torch, the re-exported names."""
import gc
import os
import pickle
import subprocess
import sys
import threading
import weakref

import pytest
import torch

from coala_amd.compression._cache import IdentityCache, WeakIdCache


class Key(list):
    """A list that can be weakly referenced (two equal Keys are distinct key objects)."""


class Obj:
    pass


def _entries():
    return Key([{"name": "w", "kind": "seg", "n": 4}, {"name": "c", "kind": "raw"}])


def test_identity_cache_hit_miss_and_extras():
    cache, calls = IdentityCache(8), []

    def make(tag):
        def f():
            calls.append(tag)
            return [tag]
        return f
    a, b = _entries(), _entries()
    assert a == b and a is not b
    va = cache.get(a, make=make("a"))
    assert cache.get(a, make=make("a again")) is va and calls == ["a"]  # the same object: a hit, make not called
    vb = cache.get(b, make=make("b"))
    assert vb == ["b"] and vb is not va and calls == ["a", "b"]  # equal but distinct: a miss
    v1 = cache.get(a, (0.01, 8), make("a/0.01"))
    v2 = cache.get(a, (0.05, 8), make("a/0.05"))
    assert v1 == ["a/0.01"] and v2 == ["a/0.05"] and cache.get(a, (0.01, 8), make("x")) is v1
    assert cache.get(a, make=make("y")) is va and len(cache) == 4
    # a tuple of objects: every one of them must be the very object
    vab = cache.get((a, b), (), make("ab"))
    assert cache.get((a, b), (), make("z")) is vab
    assert cache.get((a, _entries()), (), make("ab2")) == ["ab2"]
    assert cache.get((b, a), (), make("ba")) == ["ba"]
    # no object at all: keyed by the extras' value
    assert cache.get((), ("sig", 1), make("v")) is cache.get((), ("sig", 1), make("w"))
    assert calls == ["a", "b", "a/0.01", "a/0.05", "ab", "ab2", "ba", "v"]


def test_identity_cache_keeps_its_key_alive_until_eviction():
    cache = IdentityCache(2)
    k = _entries()
    ref = weakref.ref(k)
    cache.get(k, make=lambda: "k")
    del k
    gc.collect()
    assert ref() is not None  # held by the entry: its id cannot be reused while the entry lives
    assert cache.get(ref(), make=lambda: "rebuilt") == "k"
    others = [_entries(), _entries()]
    for o in others:
        cache.get(o, make=lambda: "o")
    gc.collect()
    assert ref() is None and len(cache) == 2  # evicted: freed


def test_identity_cache_bound_evicts_the_oldest_first():
    limit = 5
    cache = IdentityCache(limit)
    keys = [_entries() for _ in range(limit + 3)]
    for i, k in enumerate(keys):
        assert cache.get(k, make=lambda i=i: i) == i
    assert len(cache) == limit
    for i, k in enumerate(keys[3:], 3):  # the newest `limit` are still there ...
        assert cache.get(k, make=lambda: "rebuilt") == i
    assert len(cache) == limit
    for k in keys[:3]:  # ... the three oldest are gone
        assert cache.get(k, make=lambda: "rebuilt") == "rebuilt"
    assert len(cache) == limit


def test_identity_cache_under_threads():
    limit = 8
    cache = IdentityCache(limit)
    keys = [_entries() for _ in range(3 * limit)]
    errs = []

    def run(t):
        try:
            for i in range(2000):
                k = keys[(i * (2 * t + 1) + t) % len(keys)]
                extra = (i % 2,)
                v = cache.get(k, extra, lambda k=k, extra=extra: (k, extra))
                assert v[0] is k and v[1] == extra  # the value make built for that very object and extras
        except BaseException as e:  # reported below
            errs.append(e)
    ts = [threading.Thread(target=run, args=(t,)) for t in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    assert len(cache) == limit


def test_weak_id_cache():
    cache = WeakIdCache(4)
    extra = Obj()  # (alive from the start: it cannot take a dead object's id)
    objs = [Obj() for _ in range(4)]
    vals = [cache.get(o, lambda o, i=i: ("v", i)) for i, o in enumerate(objs)]
    assert all(cache.get(o, lambda o: "rebuilt") is v for o, v in zip(objs, vals)) and len(cache) == 4
    assert cache.values() == vals
    del objs[:3]
    gc.collect()
    assert len(cache) == 4  # dead entries stay until the sweep threshold passes ...
    cache.get(extra, lambda o: "e")
    assert len(cache) == 2 and sorted(map(str, cache.values())) == sorted(map(str, [vals[3], "e"]))  # ... then they go
    # set() replaces a value its user found stale
    assert cache.set(extra, "e2") == "e2" and cache.get(extra, lambda o: "rebuilt") == "e2"
    # still_valid false: the value is built again
    ok = [True]
    checked = WeakIdCache(4, still_valid=lambda v: ok[0])
    o = Obj()
    assert checked.get(o, lambda o: "first") == "first" and checked.get(o, lambda o: "second") == "first"
    ok[0] = False
    assert checked.get(o, lambda o: "second") == "second"
    ok[0] = True
    assert checked.get(o, lambda o: "third") == "second"


def test_weak_id_cache_never_serves_a_reused_id():
    cache = WeakIdCache(1 << 20)  # (never swept here: the dead entries stay in the way)
    seen = {}
    reused = None
    for i in range(10000):
        o = Obj()
        if id(o) in seen:
            reused = (o, seen[id(o)])
            break
        seen[id(o)] = i
        assert cache.get(o, lambda o, i=i: ("obj", i)) == ("obj", i)  # (the value must not hold o: o has to die)
        del o
    if reused is not None:  # (an allocator that never hands an address out twice: nothing to force)
        o, old = reused
        assert id(o) in cache._d and cache._d[id(o)][1] == ("obj", old)  # the dead object's entry is in the way
        assert cache.get(o, lambda o: "new") == "new"  # ... and is not served: make ran for this very object
        assert cache.get(o, lambda o: "rebuilt") == "new"


def _small_update():
    from coala_amd.compression import UpdateCodec
    from tests.oracle_backend import OracleBackend
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.BatchNorm1d(5))
    return UpdateCodec(0.3, 8, "weights", OracleBackend()).encode(model.state_dict())


def test_carrier_pickles_under_its_codec_name():
    from coala_amd.compression.codec import CompressedUpdate
    assert CompressedUpdate.__module__ == "coala_amd.compression.codec"
    up = _small_update()
    blob = pickle.dumps(up)
    assert b"coala_amd.compression.codec" in blob and b"CompressedUpdate" in blob
    back = pickle.loads(blob)
    assert type(back) is CompressedUpdate and back.header["total_k"] == up.header["total_k"] > 0
    for f in ("idx", "vals", "mn", "scale"):
        assert torch.equal(getattr(back.encoded, f), getattr(up.encoded, f).cpu())
    assert list(back.raw) == list(up.raw) and all(torch.equal(back.raw[n], up.raw[n]) for n in up.raw)


def test_validate_module_does_not_load_torch():
    out = subprocess.run([sys.executable, "-c", "import sys; import coala_amd.compression.validate as v; "
                          "assert callable(v.validate) and v.MODES; print('torch' in sys.modules)"],
                         capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip() == "False"


@pytest.mark.parametrize("name,home", [
    ("FlatState", "state"), ("RawState", "state"), ("flatten_state", "state"), ("module_tensors", "state"),
    ("describe_tensors", "state"), ("describe_state", "state"), ("layout_of", "state"), ("as_numpy", "state"),
    ("module_with_state", "clone"), ("release_decode_pool", "clone"), ("validate", "validate"), ("MODES", "validate")])
def test_codec_reexports_the_moved_names(name, home):
    from importlib import import_module
    codec = import_module("coala_amd.compression.codec")
    assert getattr(codec, name) is getattr(import_module("coala_amd.compression." + home), name)
