"""State and layout description: a state_dict (or a module's tensors, read in place) as aligned fp32 segments
plus raw passthrough entries, and the per-layout tables the encode and the decode derive from it."""
from collections import OrderedDict
from collections.abc import Mapping
from functools import lru_cache
from itertools import chain
from operator import attrgetter, is_, itemgetter

import numpy as np
import torch

from ._cache import IdentityCache, WeakIdCache
from .spec import ALIGN, align_up


class FlatState:
    """A state_dict split into one aligned flat fp32 buffer (segments) plus raw passthrough entries."""

    def __init__(self, entries, flat, raw):
        self.entries = entries  # list of dicts: name, dtype, shape, kind, (seg, off, n) | ()
        self.flat = flat        # fp32 [span] on device (None if no fp32 entry)
        self.raw = raw          # OrderedDict name -> tensor
        self._on = {}           # device -> flat copy (a snapshot taken on one device, used on another)

    def flat_on(self, device):
        """The flat buffer on `device` (copied once per device and cached: the w_global snapshot of a
        round is immutable)."""
        if self.flat is None or self.flat.device == torch.device(device):
            return self.flat
        key = str(device)
        t = self._on.get(key)
        if t is None:
            t = self._on[key] = self.flat.to(device)
        return t


def layout_of(state):
    """[(name, dtype str, shape)] of a state_dict — what must match between encoder and decoder."""
    return [(k, _dtype_name(v.dtype), tuple(v.shape)) for k, v in state.items()]


@lru_cache(maxsize=None)
def _dtype_name(dt):
    return str(dt).replace("torch.", "")


class _Layout:
    """The header entries of one state_dict layout (the (name, dtype, shape) sequence) and the names of its
    fp32 segments / raw passthrough entries. Built once per layout: a model's layout is fixed for a whole FL
    task, and the per-entry Python of building them was most of a ResNet-50 encode call's host time. The
    entries are shared by every header of that layout and never mutated."""

    def __init__(self, items):
        self.entries, self.seg_names, self.raw_names = [], [], []
        self.seg_idx, self.raw_idx = [], []
        off = seg = 0
        for i, (name, dt, shape) in enumerate(items):
            n = 1
            for d in shape:
                n *= d
            e = {"name": name, "dtype": _dtype_name(dt), "shape": list(shape)}
            if dt == torch.float32 and n > 0:
                e.update(kind="seg", seg=seg, off=off, n=n)
                self.seg_names.append(name)
                self.seg_idx.append(i)
                off = align_up(off + n)
                seg += 1
            else:
                e["kind"] = "raw"
                self.raw_names.append(name)
                self.raw_idx.append(i)
            self.entries.append(e)
        self.sizes = [e["n"] for e in self.entries if e["kind"] == "seg"]
        self.sizes_key = tuple(self.sizes)
        # the passthrough entries as one group when they are all scalars of one dtype (BatchNorm counters)
        raw_items = [items[i] for i in self.raw_idx]
        self.raw_scalars = (None if not raw_items or any(len(sh) for _, _, sh in raw_items)
                            or len({dt for _, dt, _ in raw_items}) != 1
                            else [(n, (), 1) for n, _, _ in raw_items])


_LAYOUTS = IdentityCache(16)  # keyed by value: the (name, dtype, shape) signature -> _Layout


def _layout(state):
    return _layout_sig(tuple((k, v.dtype, v.shape) for k, v in state.items()))


def _layout_sig(sig):
    return _LAYOUTS.get((), sig, _Layout, sig)


_MOD_TABLES = itemgetter("_parameters", "_buffers", "_modules", "_non_persistent_buffers_set")


class _StateWalk:
    """The tensors of a module's state_dict, in state_dict order, without building the state_dict: the
    module tree walked once (pre-order, as Module.state_dict recurses), then per call each module's
    parameter and persistent-buffer tables read in place (no per-entry detach, no prefix strings, no
    state-dict hooks: the reference's models register none). Re-walked when a table's size changes, when a
    table object or a submodule is replaced (each module's children are compared by identity: a client that
    keeps one root module across rounds may swap `model.head`), or when the non-persistent buffer set changes.
    The per-call checks and the gather run as C-level maps over the modules' __dict__ tables (a Python loop
    over ResNet-50's 161 modules cost more than the encode's own launches)."""

    def __init__(self, module):
        self.mods, names = [], []
        srcs, keys = [], []  # per state entry: the table it lives in, its key
        self.npbs = []  # (module, non-persistent buffer names) of the modules that have some
        self.hooked = False
        for prefix, m in module.named_modules(remove_duplicate=False):
            self.hooked = self.hooked or bool(m._state_dict_hooks or m._state_dict_pre_hooks)
            pn = tuple(k for k, v in m._parameters.items() if v is not None)
            bn = tuple(k for k, v in m._buffers.items() if v is not None and k not in m._non_persistent_buffers_set)
            self.mods.append(m)
            srcs.extend([m._parameters] * len(pn) + [m._buffers] * len(bn))
            keys.extend(pn + bn)
            if m._non_persistent_buffers_set:
                self.npbs.append((m, frozenset(m._non_persistent_buffers_set)))
            p = prefix + "." if prefix else ""
            names.extend(p + k for k in pn + bn)
        self.dicts = [m.__dict__ for m in self.mods]
        self.tables = self._tables()           # every module's 4 table objects, flattened
        self.sizes = list(map(len, self.tables))
        self.kid_dicts = [m._modules for m in self.mods if m._modules]  # the child tables, and their children now
        self.kids = [tuple(d.values()) for d in self.kid_dicts]
        self.srcs, self.keys = srcs, keys
        self.names = tuple(names)
        self.last = None  # _Described: the last describe_tensors of these tensors

    def _tables(self):
        return list(chain.from_iterable(map(_MOD_TABLES, self.dicts)))

    def tensors(self):
        """The tensors, or None when the tree changed since the walk (a table's size or object, a replaced or
        added submodule, the non-persistent buffer set): the caller walks again."""
        tables = self._tables()
        if list(map(len, tables)) != self.sizes or not all(map(is_, tables, self.tables)):
            return None
        if list(map(tuple, map(dict.values, self.kid_dicts))) != self.kids:  # (identity first: a swap is unequal)
            return None
        for m, npb in self.npbs:
            if m._non_persistent_buffers_set != npb:
                return None
        return list(map(dict.__getitem__, self.srcs, self.keys))


class _Described:
    """describe_tensors' result for one list of tensors: reused while the same tensor objects sit at the same
    storage (a dtype or shape change of a tensor in place moves its storage; a reshape of a parameter's .data
    that keeps its storage start is not looked for)."""

    __slots__ = ("tensors", "ptrs", "L", "seg_ptrs", "raw_ptrs", "raw_ok")

    def __init__(self, tensors, ptrs, L):
        self.tensors, self.ptrs, self.L = tensors, ptrs, L
        self.seg_ptrs = tuple(ptrs[i] for i in L.seg_idx)
        self.raw_ptrs = tuple(ptrs[i] for i in L.raw_idx)
        self.raw_ok = None  # the gather's own checks of the raw scalars, once


_WALKS = WeakIdCache(64)  # module -> its _StateWalk


def module_tensors(module):
    """(names, tensors) of module.state_dict() — the same names and tensor storage, in the same order — via a
    cached _StateWalk. A module tree with state-dict hooks takes state_dict() itself."""
    return _module_walk(module)[:2]


def _module_walk(module):
    """module_tensors' (names, tensors) and the walk (None when state_dict() was taken)."""
    if module._state_dict_hooks or module._state_dict_pre_hooks:
        st = module.state_dict()
        return tuple(st), list(st.values()), None
    w = _WALKS.get(module, _StateWalk)
    ts = w.tensors()
    if ts is None:  # a table changed size, or a table or submodule was replaced: walk again
        w = _WALKS.set(module, _StateWalk(module))
        ts = w.tensors()
    if w.hooked:
        st = module.state_dict()
        return tuple(st), list(st.values()), None
    return w.names, ts, w


_get_dtype, _get_shape = attrgetter("dtype"), attrgetter("shape")
_data_ptr, _is_contig, _get_device = torch.Tensor.data_ptr, torch.Tensor.is_contiguous, torch.Tensor.get_device


def describe_tensors(names, tensors, walk=None, gather=None):
    """describe_state() over (names, tensors) in state_dict order (module_tensors). walk: the _StateWalk the
    tensors came from — the layout is then reused while the same tensor objects sit at the same storage (see
    _Described), instead of reading every tensor's dtype and shape. gather: a backend's one-launch copy of
    one-element tensors (HipBackend.gather_scalars) for the passthrough scalars."""
    d, segs = _layout_walk(names, tensors, walk)
    return d.L, segs, _raw_snapshot(d, tensors, gather)


def _layout_walk(names, tensors, walk):
    """(_Described, fp32 segment tensors) of the tensors: the layout part of describe_tensors."""
    ptrs = tuple(map(_data_ptr, tensors))
    d = walk.last if walk is not None else None
    if d is None or d.ptrs != ptrs or not all(map(is_, tensors, d.tensors)):
        dts, shs = list(map(_get_dtype, tensors)), list(map(_get_shape, tensors))
        d = _Described(tensors, ptrs, _layout_sig(tuple(zip(names, dts, shs))))
        if walk is not None:
            walk.last = d
    return d, list(map(tensors.__getitem__, d.L.seg_idx))


def _raw_snapshot(d, tensors, gather):
    """The passthrough entries' RawState: one gather launch for a group of scalars of one dtype."""
    L = d.L
    raw_ts = list(map(tensors.__getitem__, L.raw_idx))
    raw = None
    if L.raw_scalars is not None:
        flat = gather(raw_ts, d) if gather is not None else None
        if flat is not None:
            raw = RawState([(flat, L.raw_scalars)], L.raw_names)
        else:
            try:
                with torch.no_grad():  # one stack of the scalar counters: no per-entry checks
                    raw = RawState([(torch.stack(raw_ts), L.raw_scalars)], L.raw_names)
            except RuntimeError:  # (counters on several devices)
                raw = None
    if raw is None:
        raw = RawState.snapshot(list(zip(L.raw_names, raw_ts)))
    return raw


def describe_state(state):
    """state_dict -> (entries as flatten_state would write them, fp32 segment tensors in order, raw
    passthrough entries), WITHOUT copying the fp32 data: the zero-copy encode reads the tensors in place."""
    L, segs, raw = _describe(state)
    return L.entries, segs, raw


def _describe(state):
    L = _layout(state)
    segs = [state[n] for n in L.seg_names]  # read in place by the kernels (pointer, numel, dtype, contiguity)
    return L, segs, RawState.snapshot([(n, state[n]) for n in L.raw_names])


def _to_host(*ts):
    """numpy copies of tensors, with ONE device-to-host transfer when they live on a GPU."""
    if not ts or ts[0].device.type == "cpu":
        return [t.numpy() for t in ts]
    parts = [t.contiguous().view(torch.uint8).reshape(-1) for t in ts]
    host = torch.cat(parts).cpu().numpy()
    out, o = [], 0
    for t, p in zip(ts, parts):
        n = p.numel()
        out.append(host[o:o + n].view(_NP_DTYPES[t.dtype]))
        o += n
    return out


_NP_DTYPES = {torch.float32: np.float32, torch.int32: np.int32, torch.uint8: np.uint8, torch.int64: np.int64,
              torch.uint32: np.uint32}
# the dtypes a passthrough entry of a blob may name (a state_dict's non-fp32 or empty entries); a blob naming
# anything else is rejected rather than handed to getattr(torch, ...)
_RAW_DTYPES = {_dtype_name(d): d for d in (torch.float32, torch.float64, torch.float16, torch.bfloat16, torch.int64,
                                          torch.int32, torch.int16, torch.int8, torch.uint8, torch.bool,
                                          torch.complex64, torch.complex128)}


class RawState(Mapping):
    """The passthrough (non-fp32) entries of an update — BatchNorm's int64 num_batches_tracked and the like —
    held as ONE flat tensor per (dtype, device) with the entries' names and shapes, in state order. Taking
    the snapshot is one copy kernel per group (not one per entry); the per-entry tensors are views made on
    first access (one unbind / split call per group). A read-only mapping name -> tensor."""

    def __init__(self, groups, order):
        self._groups = groups    # [(flat, [(name, shape, numel)])]
        self._order = order      # names in state order
        self._views = None

    @classmethod
    def snapshot(cls, items):
        """Copies of (name, tensor) items taken now, grouped per (dtype, device)."""
        groups, index = [], {}
        for name, t in items:
            key = (t.dtype, t.device)
            g = index.get(key)
            if g is None:
                g = index[key] = []
                groups.append((key, g))
            g.append((name, t))
        out = []
        with torch.no_grad():
            for _, members in groups:
                ts = [t for _, t in members]
                if all(t.dim() == 0 for t in ts):
                    flat = torch.stack(ts)  # (one kernel: the usual case, scalar counters)
                else:
                    flat = torch.cat([t.reshape(-1) for t in ts])
                out.append((flat, [(n, tuple(t.shape), t.numel()) for n, t in members]))
        return cls(out, [n for n, _ in items])

    def _make_views(self, groups):
        views = {}
        for flat, members in groups:
            if all(len(shape) == 0 for _, shape, _ in members):
                views.update(zip((n for n, _, _ in members), flat.unbind()))
            else:
                for (n, shape, _), piece in zip(members, flat.split_with_sizes([m for _, _, m in members])):
                    views[n] = piece.view(shape)
        return views

    def __getitem__(self, name):
        if self._views is None:
            self._views = self._make_views(self._groups)
        return self._views[name]

    def __iter__(self):
        return iter(self._order)

    def __len__(self):
        return len(self._order)

    @property
    def nbytes(self):
        return sum(f.numel() * f.element_size() for f, _ in self._groups)

    @classmethod
    def from_entries(cls, entries, rawb):
        """From a blob's raw section: entries with "dtype", "shape", "off", "nbytes" (in state order). Runs of
        same-dtype entries stored back to back become one tensor (one copy of the bytes)."""
        groups, order, run = [], [], []

        def flush():
            if run:
                dt = _RAW_DTYPES.get(run[0]["dtype"])
                if dt is None:
                    raise ValueError(f"COALAQ1: unsupported raw entry dtype {run[0]['dtype']!r}")
                size = torch.empty(0, dtype=dt).element_size()
                members = []
                for e in run:  # every entry's byte count must match its own shape (not only the run's total)
                    m = int(np.prod(e["shape"], dtype=np.int64))
                    if m < 0 or int(e["nbytes"]) != m * size:
                        raise ValueError(f"COALAQ1: raw entry {e['name']!r}: {e['nbytes']} bytes for shape "
                                         f"{e['shape']} of {e['dtype']}")
                    members.append((e["name"], tuple(e["shape"]), m))
                lo, hi = run[0]["off"], run[-1]["off"] + run[-1]["nbytes"]
                if lo < 0 or hi > len(rawb):
                    raise ValueError("COALAQ1: raw entries past the end of the blob")
                buf = bytearray(rawb[lo:hi])
                flat = torch.frombuffer(buf, dtype=dt) if buf else torch.empty(0, dtype=dt)
                groups.append((flat, members))
                run.clear()
        for e in entries:
            if run and (e["dtype"] != run[-1]["dtype"] or e["off"] != run[-1]["off"] + run[-1]["nbytes"]):
                flush()
            run.append(e)
            order.append(e["name"])
        flush()
        return cls(groups, order)

    def entry_bytes(self):
        """{name: little-endian bytes} with one device-to-host copy per group."""
        out = {}
        for flat, members in self._groups:
            b = flat.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()
            per = flat.element_size()
            o = 0
            for n, _, m in members:
                out[n] = b[o:o + m * per]
                o += m * per
        return {n: out[n] for n in self._order}

    def fresh_groups(self, device=None):
        """(the per-group flat copies, {name: view of them}): storage of its own (one copy per group, onto `device`
        if given) — what a decode hands out, so decoded modules never alias the update or each other."""
        groups = [(f.to(device, copy=True) if device is not None else f.clone(), m) for f, m in self._groups]
        views = self._make_views(groups)
        return [f for f, _ in groups], {n: views[n] for n in self._order}

    def signature(self):
        """What a copy into another RawState's group buffers needs to match: dtype, size and members per group."""
        return tuple((f.dtype, f.numel(), tuple(m)) for f, m in self._groups)


def _snapshot_raw(raw):
    """Copies of the passthrough entries taken now (RawState: one copy kernel per dtype / device)."""
    return RawState.snapshot(list(raw.items()))


def flatten_state(state, device=None):
    """state_dict -> FlatState with every fp32 entry at an ALIGN-aligned offset of one flat buffer.

    One torch.cat over the tensors and zero pads (a single device copy kernel), not one copy per entry.
    """
    L = _layout(state)
    parts, pad_src = [], None
    for e in L.entries:
        if e["kind"] != "seg":
            continue
        t, end = state[e["name"]], e["off"] + e["n"]
        if device is None:
            device = t.device
        parts.append(t.detach().reshape(-1).to(device))
        if align_up(end) > end:
            if pad_src is None:
                pad_src = torch.zeros(ALIGN, dtype=torch.float32, device=device)
            parts.append(pad_src[:align_up(end) - end])
    raw = OrderedDict((n, state[n].detach().clone()) for n in L.raw_names)
    return FlatState(L.entries, torch.cat(parts) if parts else None, raw)


_SAME_LAYOUT = IdentityCache(64)  # (entries, base entries): pairs of entry lists already found equal
_DECODE_LAYOUTS = IdentityCache(64)  # entries -> _DecodeLayout
_DENSE = IdentityCache(32)  # entries -> fp32 elements


def _check_same_layout(entries, base_entries):
    def compare():  # (header entries are never mutated: an equal pair stays equal; an unequal one is not cached)
        a = [(e["name"], e["dtype"], tuple(e["shape"])) for e in entries]
        b = [(e["name"], e["dtype"], tuple(e["shape"])) for e in base_entries]
        if a != b:
            raise ValueError("update and base model have different state_dict layouts")
        return True
    if entries is not base_entries:  # (states of one layout share their entries list: _Layout)
        _SAME_LAYOUT.get((entries, base_entries), (), compare)


class _DecodeLayout:
    """Per header-entries list: the state names, the fp32 segment sizes and where segments / raw entries sit."""

    def __init__(self, entries):
        self.names = tuple(e["name"] for e in entries)
        self.sizes = tuple(e["n"] for e in entries if e["kind"] == "seg")
        self.seg_pos = [i for i, e in enumerate(entries) if e["kind"] == "seg"]
        self.raw = [(i, e["name"]) for i, e in enumerate(entries) if e["kind"] != "seg"]


def _decode_layout(entries):
    return _DECODE_LAYOUTS.get(entries, (), _DecodeLayout, entries)


def _dense_elements(entries):
    return _DENSE.get(entries, (), lambda: sum(e["n"] for e in entries if e["kind"] == "seg"))


def as_numpy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
