"""Decoded state -> nn.Module: a template's module tree rebuilt around new tensors from a per-template recipe,
and the pool that recycles decoded modules once nothing outside the codec references them."""
import copy
import sys
import threading
from collections import OrderedDict
from itertools import chain, repeat
from operator import is_, itemgetter

import torch
from torch import nn

from ._cache import WeakIdCache
from .state import RawState


def _segment_views(flat, table, entries):
    """Views of the decoded flat buffer, one per fp32 segment (in segment order), shaped like the header's
    entries, at the decoder's own offsets (never the untrusted header's): ONE split of the buffer into
    segments and alignment pads, and a view only where a shape is not already the 1-D piece (a slice +
    view per entry cost ~3 us each, ~1 ms per ResNet-50 decode)."""
    split = table.__dict__.get("_split")
    if split is None:
        sizes, keep, prev = [], [], 0
        for off, n in zip(table.offsets, table.sizes):
            if off > prev:
                sizes.append(off - prev)
            keep.append(len(sizes))
            sizes.append(n)
            prev = off + n
        split = table.__dict__["_split"] = (sizes, keep, prev)
    sizes, keep, end = split
    pieces = flat[:end].split_with_sizes(sizes)
    seg_entries = [e for e in entries if e["kind"] == "seg"]
    out = []
    for j, e in zip(keep, seg_entries):
        t, shape = pieces[j], e["shape"]
        out.append(t if len(shape) == 1 else t.view(shape))
    return out


_PLAIN_TYPES = frozenset((bool, int, float, complex, str, bytes, type(None), torch.dtype, torch.device))
_CONTAINER_TYPES = frozenset((dict, OrderedDict, list, set))
_MODULE_TABLES = frozenset(("_parameters", "_buffers", "_modules"))
_TABLES3 = itemgetter("_parameters", "_buffers", "_modules")
_make_param = torch.Tensor._make_subclass


def _plain(v):
    """An attribute value a clone may share with the template: immutable and holding no tensor / module."""
    tv = type(v)
    if tv in _PLAIN_TYPES:
        return True
    if tv is tuple or tv is frozenset:
        return all(_plain(x) for x in v)
    return False


class _TreeRecipe:
    """How to rebuild a template's module tree around new tensors, classified once per template (the
    server's global model is one object for the whole task): the modules in pre-order (a submodule shared
    by several parents is cloned once, as copy.deepcopy would), and per module the attributes a clone
    shares (immutable plain values), gets as fresh empty containers (hook dicts, ...), deep-copies (any
    other object: non-empty containers, hook objects, unregistered modules — with a memo that maps the
    template's modules / parameters / buffers to the clone's, so bound hooks are rebound as deepcopy would)
    or clones (unregistered tensors), plus its parameter / buffer / child slots. A module whose attribute
    set, table sizes or special attribute types changed since is re-classified."""

    def __init__(self, template):
        self.pool, self.pool_lock = [], threading.Lock()
        self.tick = 0  # idle_skeleton calls so far (a pooled tree's last use is one of these)
        self.mods, self.prefixes, self.index = [], [], {}
        stack = [(template, "")]
        while stack:
            m, prefix = stack.pop()
            if id(m) in self.index:
                continue
            self.index[id(m)] = len(self.mods)
            self.mods.append(m)
            self.prefixes.append(prefix)
            stack.extend((c, prefix + n + ".") for n, c in reversed(list(m._modules.items())) if c is not None)
        self.info = [self.classify(m, p) for m, p in zip(self.mods, self.prefixes)]

    def classify(self, m, prefix):
        d = m.__dict__
        fresh, deep, tens = [], [], []
        for k, v in d.items():
            if k in _MODULE_TABLES or _plain(v):
                continue
            tv = type(v)
            if tv in _CONTAINER_TYPES and not v:
                fresh.append((k, tv))
            elif isinstance(v, torch.Tensor):
                tens.append((k, tv))
            else:
                deep.append((k, tv))
        params = tuple((n, prefix + n, p is None or p.requires_grad) for n, p in m._parameters.items())
        buffers = tuple((n, prefix + n) for n in m._buffers)
        children = tuple((n, None if c is None else self.index[id(c)]) for n, c in m._modules.items())
        sizes = (len(d), len(m._parameters), len(m._buffers), len(m._modules))
        return sizes, tuple(fresh), tuple(deep), tuple(tens), params, buffers, children

    def valid(self, i):
        """Check that module i still matches its classification: attribute / table sizes, its
        fresh containers still empty (a hook registered later must be deep-copied, not dropped) and the
        types of its deep-copied / cloned attributes."""
        m = self.mods[i]
        sizes, fresh, deep, tens = self.info[i][:4]
        d = m.__dict__
        if sizes != (len(d), len(m._parameters), len(m._buffers), len(m._modules)):
            return False
        if any(d.get(k) for k, _ in fresh):
            return False
        return all(type(d.get(k)) is tv for k, tv in tens + deep)

    def _current(self):
        """Re-classify the template modules that changed since (attribute / table sizes, hooks registered, the
        types of special attributes); returns the per-module fast tables. A change also retires every pooled
        skeleton (they were built from the old classification)."""
        mods, info = self.mods, self.info
        if self.__dict__.get("fast") is not None and self._unchanged():
            return self.fast
        stale = [i for i in range(len(mods)) if not self.valid(i)]  # (only once the whole-tree check has failed)
        if stale:
            for i in stale:
                info[i] = self.classify(mods[i], self.prefixes[i])
            with self.pool_lock:
                self.pool.clear()
        fast = self.__dict__.get("fast")
        if fast is None or stale:
            fast = self.fast = [self._fast(x) for x in info]
            self.plain = [tuple(k for k in m.__dict__ if k not in _MODULE_TABLES and k not in set(f[5] + f[9] + f[10]))
                          for m, f in zip(mods, fast)]
            self._flat_tables()
        return fast

    def _flat_tables(self):
        """The per-call checks and the refresh as C-level maps over the whole tree (a Python loop over a
        ResNet-50's 132 modules and their ~1,600 hook containers cost more than the decode itself)."""
        dicts = self.t_dicts = [m.__dict__ for m in self.mods]
        self.t_dlens = list(map(len, dicts))
        self.t_tables = list(chain.from_iterable(map(_TABLES3, dicts)))
        self.t_sizes = list(map(len, self.t_tables))
        self.t_fresh = [d[k] for d, x in zip(dicts, self.info) for k, _ in x[1]]  # the template's empty containers
        self.t_typed = [(d, k, tv) for d, x in zip(dicts, self.info) for k, tv in x[3] + x[2]]
        self.p_src = [d for d, keys in zip(dicts, self.plain) for _ in keys]
        self.p_keys = [k for keys in self.plain for k in keys]
        self.p_mod = [i for i, keys in enumerate(self.plain) for _ in keys]
        self.special = [i for i, f in enumerate(self.fast) if f[9] or f[10]]

    def _unchanged(self):
        """Every template module as classified: __dict__ and table sizes, the same table objects, its fresh
        containers still empty (a hook registered later must be deep-copied), its special attributes' types."""
        dicts = self.t_dicts
        if list(map(len, dicts)) != self.t_dlens or any(self.t_fresh):
            return False
        tabs = list(chain.from_iterable(map(_TABLES3, dicts)))
        if not all(map(is_, tabs, self.t_tables)) or list(map(len, tabs)) != self.t_sizes:
            return False
        return all(type(d.get(k)) is tv for d, k, tv in self.t_typed)

    def tree_unchanged(self):
        """The template's module tree is still the one this recipe walked: every child slot holds the same
        module object (a replaced submodule — model.head = nn.Linear(...) — needs a new recipe)."""
        kids = self.__dict__.get("t_kids")
        if kids is None:  # (read without a lock, _RECIPES' still_valid: two threads here fill in the same tables)
            self.t_kid_dicts = [m._modules for m in self.mods if m._modules]
            kids = self.t_kids = [tuple(d.values()) for d in self.t_kid_dicts]
        return list(map(tuple, map(dict.values, self.t_kid_dicts))) == kids

    def build(self, state):
        return self._build(state)[0]

    def _build(self, state):
        """The new module tree: the list of new module objects in recipe order (root first)."""
        mods = self.mods
        fast = self._current()
        new = [m.__class__.__new__(m.__class__) for m in mods]
        get = state.get
        deep_todo = []
        for i, m in enumerate(mods):
            pnames, pkeys, prgs, bnames, bkeys, fkeys, ftypes, cnames, cidx, tens, deep = fast[i]
            ts = list(map(get, pkeys))
            if any(map(is_, ts, repeat(None))):  # a parameter the state lacks (or a None slot): the template's, cloned
                src = m._parameters
                ts = [t if t is not None else (None if src[n] is None else src[n].detach().clone())
                      for n, t in zip(pnames, ts)]
                P = {n: None if t is None else _make_param(nn.Parameter, t, rg) for n, t, rg in zip(pnames, ts, prgs)}
            else:
                P = dict(zip(pnames, map(_make_param, repeat(nn.Parameter), ts, prgs)))
            B = dict(zip(bnames, map(get, bkeys)))
            if any(map(is_, B.values(), repeat(None))):
                srcb = m._buffers
                B = {n: (t if t is not None else (None if srcb[n] is None else srcb[n].clone())) for n, t in B.items()}
            d = m.__dict__.copy()  # plain attributes shared (read now: e.g. `training` follows the template)
            if fkeys:
                d.update(zip(fkeys, [tv() for tv in ftypes]))
            for k in tens:
                d[k] = d[k].clone()
            d["_parameters"] = P
            d["_buffers"] = B
            d["_modules"] = dict(zip(cnames, [None if j is None else new[j] for j in cidx]))
            new[i].__dict__.update(d)  # (a fresh object's dict: no Module.__setattr__ on the way)
            if deep:
                deep_todo.append((i, deep))
        if deep_todo:  # after every clone is filled in, so the memo maps every module / tensor
            memo = self._memo(new, state)
            for i, deep in deep_todo:
                nd = new[i].__dict__
                for k in deep:
                    nd[k] = copy.deepcopy(nd[k], memo)
        return new

    # -- recycling of decoded modules (UpdateCodec.decode_module) ------------------------------------------
    POOL_MAX = 64            # skeletons kept per template (a server needs two rounds' uploads: 2 x clients)
    POOL_BYTES = 16 << 30    # ... and at most this many bytes of decoded storage
    POOL_FRACTION = 8        # ... nor more than 1/8 of the device's memory
    EVICT_SLACK = 16         # a tree not handed out for 2 x pool size + this many calls is dropped from the pool

    def pool_limit(self, device):
        lim = self.__dict__.get("_pool_limit")
        if lim is None or lim[0] != device:
            total = None
            if device is not None and device.type == "cuda":
                total = torch.cuda.get_device_properties(device).total_memory
            lim = self._pool_limit = (device, self.POOL_BYTES if total is None else
                                      min(self.POOL_BYTES, total // self.POOL_FRACTION))
        return lim[1]

    def build_and_adopt(self, box, D, flat, raws, raw, device, adopt=True):
        """Build the module tree for the decoded state in box (a one-element list, emptied here: the caller
        keeps no reference to the state) and keep it in the pool as a skeleton for later decodes of the same
        layout (unless adopt is False). Returns the root module."""
        state = box.pop()
        new = self._build(state)
        del state
        root = new[0]
        if (not adopt or (flat is None and not raws) or not isinstance(raw, RawState)
                or len(self.pool) >= self.POOL_MAX):
            return root
        nbytes = (flat.numel() * 4 if flat is not None else 0) + sum(r.numel() * r.element_size() for r in raws or ())
        limit = self.pool_limit(device)
        stream = torch.cuda.current_stream(device) if device is not None and device.type == "cuda" else None
        with self.pool_lock:
            if sum(sk.nbytes for sk in self.pool) + nbytes > limit or len(self.pool) >= self.POOL_MAX:
                return root
            sk = _Skeleton(root, new, flat, list(raws or ()), D, raw.signature(), device, nbytes)
            sk.adopt(self)
            sk.stream, sk.last = stream, self.tick
            del new
            sk.base = sk.counts()
            sk.base[0][0] -= 1  # the root: this frame's `root` is the only transient reference
            self.pool.append(sk)
        return root

    def idle_skeleton(self, D, raw, device):
        """A pooled skeleton of this layout that nothing outside the pool references any more (every module,
        parameter and buffer object at its idle reference count, the decoded storage at its idle use count,
        every module's tables unchanged) and its root — (None, None) if there is none. The root is taken
        while the pool lock is held, so the moment a tree is chosen it is no longer idle for any other
        thread (the remote server decodes from one thread per upload, coala/server/service.py:74).
        Idle trees not handed out for a while (2 x the pool size + EVICT_SLACK calls: more than a round needs)
        are dropped from the pool; held ones stay."""
        if not self.pool or not isinstance(raw, RawState):
            return None, None
        self._current()
        sig = raw.signature()
        with self.pool_lock:
            self.tick += 1
            found = root = None
            for sk in self.pool:
                if sk.D is D and sk.device == device and sk.raw_sig == sig and sk.counts() == sk.base:
                    found, root = sk, sk.root
                    sk.generation += 1
                    sk.last = self.tick
                    break
            # only IDLE trees go: a tree still held (a server keeps round r's uploads until round r + 1 replaces them,
            # coala/server/base.py:377-381) becomes reusable when its holder lets go, however long that takes
            horizon = 2 * len(self.pool) + self.EVICT_SLACK
            if any(self.tick - sk.last > horizon for sk in self.pool):
                self.pool[:] = [sk for sk in self.pool
                                if self.tick - sk.last <= horizon or sk is found or sk.counts() != sk.base]
            return found, root

    def refresh(self, sk):
        """Bring a recycled tree's attributes in line with the template's CURRENT ones, as a fresh build would:
        plain attributes copied, hook containers emptied if a previous holder registered hooks, special
        attributes re-copied unless still equal."""
        memo = None
        list(map(dict.__setitem__, sk.p_dst, self.p_keys, map(dict.__getitem__, self.p_src, self.p_keys)))
        if any(sk.fresh):  # a previous holder registered hooks on the recycled tree: empty containers again
            for i, c in enumerate(sk.mods):
                nd, f = c.__dict__, self.fast[i]
                for k, tv in zip(f[5], f[6]):
                    if nd.get(k):
                        nd[k] = tv()
            sk.adopt(self)
        for i in self.special:
            m, c = self.mods[i], sk.mods[i]
            d, nd = m.__dict__, c.__dict__
            f = self.fast[i]
            for k in f[9]:
                nd[k] = d[k].clone()
            for k in f[10]:
                try:
                    same = bool(nd.get(k) == d[k])
                except Exception:
                    same = False
                if not same:
                    if memo is None:
                        memo = self._memo(sk.mods, {})
                    nd[k] = copy.deepcopy(d[k], memo)

    @staticmethod
    def _fast(x):
        _, fresh, deep, tens, params, buffers, children = x
        return (tuple(n for n, _, _ in params), tuple(k for _, k, _ in params), tuple(rg for _, _, rg in params),
                tuple(n for n, _ in buffers), tuple(k for _, k in buffers),
                tuple(k for k, _ in fresh), tuple(tv for _, tv in fresh),
                tuple(n for n, _ in children), tuple(j for _, j in children),
                tuple(k for k, _ in tens), tuple(k for k, _ in deep))

    def _memo(self, new, state=None):
        """deepcopy memo: template module / parameter / buffer -> its counterpart in the clone."""
        memo = {id(m): c for m, c in zip(self.mods, new)}
        for m, c in zip(self.mods, new):
            for name, t in m._parameters.items():
                if t is not None and name in c.__dict__.get("_parameters", {}):
                    memo[id(t)] = c._parameters[name]
            for name, t in m._buffers.items():
                if t is not None and name in c.__dict__.get("_buffers", {}):
                    memo[id(t)] = c._buffers[name]
        return memo


class _Skeleton:
    """A decoded module tree kept for reuse: its objects (modules, then their parameter / buffer tensors), the
    decoded storage they view (the flat fp32 decode output and the passthrough groups) and their idle
    reference counts."""

    __slots__ = ("root", "mods", "objs", "dicts", "dlens", "tables", "tsizes", "flat", "raws", "D", "raw_sig",
                 "device", "nbytes", "base", "generation", "p_dst", "fresh", "stream", "last")

    def __init__(self, root, mods, flat, raws, D, raw_sig, device, nbytes):
        self.root, self.mods = root, mods
        self.objs = list(mods)
        for c in mods:
            self.objs.extend(t for t in c._parameters.values() if t is not None)
            self.objs.extend(t for t in c._buffers.values() if t is not None)
        self.dicts = [c.__dict__ for c in mods]
        self.dlens = list(map(len, self.dicts))
        self.tables = list(chain.from_iterable(map(_TABLES3, self.dicts)))
        self.tsizes = list(map(len, self.tables))
        self.flat, self.raws, self.D, self.raw_sig, self.device, self.nbytes = flat, raws, D, raw_sig, device, nbytes
        self.generation = 0
        self.stream, self.last = None, 0

    def adopt(self, recipe):
        """The recipe's flat refresh tables for this tree: where each plain attribute goes, and the tree's own
        (empty) hook containers, checked in one pass per recycle."""
        self.p_dst = [self.dicts[i] for i in recipe.p_mod]
        self.fresh = [c.__dict__[k] for c, f in zip(self.mods, recipe.fast) for k in f[5]]

    def counts(self):
        """Idle fingerprint: every object's reference count, the decoded storage's use counts, and whether every
        module still has its attribute count and its very table objects at their sizes (an attribute added or a
        table replaced by a previous holder keeps the tree from being recycled)."""
        refs = list(map(sys.getrefcount, self.objs))
        store = [torch._C._storage_Use_Count(t.untyped_storage()._cdata) for t in [self.flat] + self.raws
                 if t is not None]
        tabs = list(chain.from_iterable(map(_TABLES3, self.dicts)))
        same = (list(map(len, self.dicts)) == self.dlens and all(map(is_, tabs, self.tables))
                and list(map(len, tabs)) == self.tsizes)
        return [refs, store, same]


_RECIPES = WeakIdCache(32, still_valid=_TreeRecipe.tree_unchanged)  # template -> its _TreeRecipe, while its tree stands


def _recipe(template):
    """The template's _TreeRecipe (one per template object: the server's global model, for a whole task)."""
    return _RECIPES.get(template, _TreeRecipe)


def release_decode_pool():
    """Drop every template's pooled decoded modules (UpdateCodec.release_pool)."""
    for r in _RECIPES.values():
        with r.pool_lock:
            r.pool.clear()


def _reuse_after(sk, stream, caller):
    """Order a recycled tree's rewrite after its previous holder's work and retire stale autograd state.
    `stream` (None on the CPU) is where the rewrite runs, `caller` the caller's current stream (the stream
    the module is handed out on). The host reference counts that made the tree idle do not see GPU work:
    the rewrite waits for everything enqueued so far on the stream the tree was last handed out on (where
    its holder's work ran, unless the holder moved it to another stream itself — torch's own contract for
    that is Tensor.record_stream, which a recycled tree cannot honour: pass recycle=False then). The decode
    kernel writes through raw pointers, so the storage's version counter is bumped here: an autograd graph
    that saved the previous values raises in backward instead of using the new ones."""
    if stream is not None and sk.stream is not None and sk.stream != stream and sk.stream != caller:
        stream.wait_stream(sk.stream)  # (the rewrite's stream already waits for the caller's)
    sk.stream = caller
    torch._C._increment_version([t for t in [sk.flat] + sk.raws if t is not None])


def module_with_state(template, state):
    """A new nn.Module shaped like `template` whose parameters / buffers ARE the tensors of `state`
    (views into the decode output: no parameter data is copied; `template` is never aliased).

    The module tree is rebuilt from a per-template recipe (_TreeRecipe) — new objects of the same classes,
    their __dict__ copied one level deep with fresh tables and hook dicts, other attributes deep-copied —
    instead of copy.deepcopy, whose generic recursion cost ~8 ms per ResNet-50 on the server's per-upload
    path. Tensors outside the state (non-persistent buffers, unregistered tensors) are cloned."""
    return _recipe(template).build(state)
