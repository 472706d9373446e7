"""Device-side codec plan: one segment table (a model layout × clients) bound to one GPU.

Thin typed wrapper over coalac_plan_create / coalac_encode / coalac_decode. Tensors are torch tensors
used purely as device memory; streams are torch's current HIP stream unless one is passed. Every
argument is checked against what the kernels assume (dtype, device, contiguity, length, 16-B
alignment) BEFORE a launch.
"""
import contextlib
import ctypes
from dataclasses import dataclass

import torch

from . import _lib
from .spec import RAW_BITS, UNIT, VALID_BITS, SegmentTable, SubTable


@dataclass
class Encoded:
    """Device buffers of one encode: idx int32[K], vals uint8[K] (fp32[K] when bits == 32),
    mn fp32[T], scale fp32[T], and (wire v2) ustart int32[U]: per 4096-element unit, the segment-relative
    index of its first kept entry — a decoder then needs no search of the idx lists (None: not available).
    packed: a dense-packed update's bit-packed code stream (wire v4, uint32[P]) where its holder has it on the
    buffers' device — CodecPlan.decode_packed reads it instead of vals, which may then be None until
    CodecPlan.unpack_dense makes the codes (None: the update is not dense-packed, or only its codes are here). A
    block-wise update (wire v5): mn / scale hold one entry per 4096-element block, packed is the stream
    CodecPlan.decode_block reads, vals is None unless a blob was unpacked on the host."""
    idx: torch.Tensor
    vals: torch.Tensor
    mn: torch.Tensor
    scale: torch.Tensor
    ustart: torch.Tensor = None
    packed: torch.Tensor = None

    FIELDS = ("idx", "vals", "mn", "scale", "ustart")

    def to(self, device, non_blocking=False):
        return Encoded(*(None if t is None else t.to(device, non_blocking=non_blocking)
                         for t in (self.idx, self.vals, self.mn, self.scale, self.ustart, self.packed)))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _idx_ptr(t):
    """idx of an Encoded: NULL when it holds nothing (a dense plan's implied indices)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)


def _on(stream):
    """Allocation context for buffers a call creates itself: on the stream the kernels run on, so the
    caching allocator never hands their memory to other work before those kernels are done."""
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


_NULL_CTX = contextlib.nullcontext()


def _device_ctx(device):
    """torch.cuda.device(device), or nothing when it is already the current device (the common case: the
    context manager's exchange costs a few us per call on the hooks' path)."""
    return _NULL_CTX if torch.cuda.current_device() == device.index else torch.cuda.device(device)


def _stream_handle(stream):
    s = torch.cuda.current_stream() if stream is None else stream
    return ctypes.c_void_p(s.cuda_stream)


class CodecPlan:
    """Plan for `clients` copies of a layout given by fp32 segment sizes.

    Args:
        sizes: element count of every fp32 segment of ONE client, in state_dict order.
        ratio: top-k ratio in (0, 1].
        bits:  1..8 (uint8 codes) or 32 (raw fp32 values).
        clients: number of client updates batched into one launch sequence.
        device: CUDA/HIP device (default: current).
    """

    def __init__(self, sizes, ratio, bits=8, clients=1, device=None, table=None):
        if bits not in VALID_BITS:
            raise ValueError(f"bits must be one of {VALID_BITS}, got {bits}")
        self.table = SegmentTable(sizes, ratio, clients) if table is None else table
        self.bits = int(bits)
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None
                                   else torch.device(device).index or 0)
        self._lib = _lib.load()
        segs = self.table.segs
        arr = (_lib.SegDesc * len(segs))()
        for i, (a, b, c, d) in enumerate(segs.tolist()):
            arr[i] = _lib.SegDesc(a, b, c, d)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.coalac_plan_create(arr, len(segs), self.bits, ctypes.byref(h)),
                       "coalac_plan_create")
        self._h = h
        ws, tk, span, nu = (ctypes.c_uint64() for _ in range(4))
        _lib.check(self._lib.coalac_plan_query(h, ctypes.byref(ws), ctypes.byref(tk), ctypes.byref(span),
                                               ctypes.byref(nu)), "coalac_plan_query")
        self.ws_bytes = ws.value
        self.total_k, self.span, self.n_units = tk.value, span.value, nu.value
        if self.total_k != self.table.total_k:
            raise _lib.CodecError(f"plan total_k {self.total_k} != table {self.table.total_k}")
        if self.n_units != self.table.n_units:
            raise _lib.CodecError(f"plan n_units {self.n_units} != table {self.table.n_units}")
        # every segment keeps all its elements: the library's dense codec (indices implied, never materialised
        # unless a caller passes a buffer for them); at ratio 1 (the wire's "dense" updates) the encoded buffers
        # carry no idx / starts by default
        segs = self.table.segs
        self.dense = bool(len(segs)) and bool((segs[:, 1] == segs[:, 2]).all())
        self.implied_idx = self.dense and getattr(self.table, "ratio", None) is not None and self.table.ratio >= 1.0

    @classmethod
    def from_segments(cls, segs, bits=8, device=None):
        """Plan over explicit coalac_seg_t rows (in_off, n, k, out_off), offsets absolute: e.g. a
        contiguous slice of a SegmentTable, whose results land in the buffers of the whole table
        (SplitPipeline's segment ranges of one update). mn / scale of such a plan are indexed by row of
        `segs`."""
        return cls(None, None, bits, device=device, table=SubTable(segs))

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            with torch.cuda.device(self.device):
                self._lib.coalac_plan_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- buffers ----------------------------------------------------------------------------------
    @property
    def n_segments(self):
        return self.table.n_segments

    @property
    def vals_dtype(self):
        return torch.float32 if self.bits == RAW_BITS else torch.uint8

    def empty_flat(self):
        return torch.empty(self.span, dtype=torch.float32, device=self.device)

    def empty_encoded(self, with_idx=None):
        """The five output buffers of an encode as views of ONE allocation (16-byte aligned each). with_idx
        (default: not implied_idx): False leaves idx empty and ustart None (ratio 1: the indices are implied)."""
        if with_idx is None:
            with_idx = not self.implied_idx
        if not with_idx:
            vb = 4 if self.bits == RAW_BITS else 1
            T = self.n_segments
            buf = torch.empty((vb * self.total_k + 15) // 16 * 16 + 8 * T, dtype=torch.uint8, device=self.device)
            o = (vb * self.total_k + 15) // 16 * 16
            return Encoded(torch.empty(0, dtype=torch.int32, device=self.device), buf[:vb * self.total_k].view(self.vals_dtype),
                           buf[o:o + 4 * T].view(torch.float32), buf[o + 4 * T:o + 8 * T].view(torch.float32), None)
        geo = self.__dict__.get("_enc_geometry")
        if geo is None:
            K, T, U = self.total_k, self.n_segments, self.n_units
            vb = 4 if self.bits == RAW_BITS else 1
            views, o = [], 0
            dts = (torch.int32, self.vals_dtype, torch.float32, torch.float32, torch.int32)
            for nbytes, dt in zip((4 * K, vb * K, 4 * T, 4 * T, 4 * U), dts):
                views.append((o, nbytes, dt))
                o = (o + nbytes + 15) // 16 * 16
            geo = self._enc_geometry = (max(o, 16), tuple(views))
        buf = torch.empty(geo[0], dtype=torch.uint8, device=self.device)
        return Encoded(*[buf[a:a + n].view(dt) for a, n, dt in geo[1]])

    def empty_workspace(self):
        return torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.device)

    # -- checks -----------------------------------------------------------------------------------
    def _check_flat(self, t, name, need=None):
        if t is None:
            return
        need = self.span if need is None else need
        if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError(f"{name}: need a contiguous float32 tensor on {self.device}, got "
                             f"{t.dtype} on {t.device} (contiguous={t.is_contiguous()})")
        if t.numel() < need:
            raise ValueError(f"{name}: {t.numel()} elements < required {need}")
        if t.data_ptr() % 16:
            raise ValueError(f"{name}: storage must be 16-byte aligned")

    def _check_encoded(self, e):
        """Dtype, device, contiguity and length of every encoded buffer; returns the ustart pointer to pass (its
        length must be exactly the plan's unit count: a buffer of another layout is an error, not a hint)."""
        want = ((e.idx, torch.int32, 0 if self.dense and e.idx.numel() == 0 else self.total_k),
                (e.vals, self.vals_dtype, self.total_k),
                (e.mn, torch.float32, self.n_segments), (e.scale, torch.float32, self.n_segments))
        if e.ustart is not None:
            want += ((e.ustart, torch.int32, self.n_units),)
            if e.ustart.numel() != self.n_units:
                raise ValueError(f"encoded ustart: {e.ustart.numel()} entries, the plan has {self.n_units} units")
        for t, dt, n in want:
            if t.device != self.device or t.dtype != dt or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"encoded buffer mismatch: need {dt}[{n}] on {self.device}, got "
                                 f"{t.dtype}[{t.numel()}] on {t.device}")
        return _ptr(e.ustart)

    # -- codec ------------------------------------------------------------------------------------
    def encode(self, flat, base=None, out=None, workspace=None, flags=0, stream=None, events=None):
        """Encode flat (fp32[span]) [- base] -> Encoded. Asynchronous on `stream`.

        events: 5 timing events recorded at the kernel boundaries (coalac_encode_ev)."""
        self._check_flat(flat, "input")
        self._check_flat(base, "base")
        with _on(stream):
            out = self.empty_encoded() if out is None else out
            ws = self.empty_workspace() if workspace is None else workspace
        ust = self._check_encoded(out)
        if ws.device != self.device or ws.numel() * ws.element_size() < self.ws_bytes:
            raise ValueError(f"workspace: need {self.ws_bytes} bytes on {self.device}")
        args = (self._h, _ptr(flat), _ptr(base), _idx_ptr(out.idx), _ptr(out.vals), _ptr(out.mn),
                _ptr(out.scale), ust, _ptr(ws), ctypes.c_uint64(self.ws_bytes), ctypes.c_uint(flags),
                _stream_handle(stream))
        with torch.cuda.device(self.device):
            if events is None:
                rc = self._lib.coalac_encode(*args)
            else:
                rc = self._lib.coalac_encode_ev(*args, _event_array(events, 5))
        _lib.check(rc, "coalac_encode")
        return out

    def segment_pointers(self, tensors, checked=False, ptrs=None, stream=None):
        """Device array of the tensors' data pointers (one per segment), for encode_segments; cached per
        pointer tuple (a model's parameter storage does not move between rounds). checked: the caller has
        verified device, dtype, contiguity, alignment and sizes (UpdateCodec.encode); ptrs: their data
        pointers, if the caller has them. The array is marked as in use by `stream` (the launch stream), so
        an eviction from the cache never hands its memory to other work while a kernel still reads it."""
        segs = self.table.segs
        if len(tensors) != len(segs):
            raise ValueError(f"need {len(segs)} segment tensors, got {len(tensors)}")
        for i, t in enumerate(() if checked else tensors):
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"segment {i}: need a contiguous float32 tensor on {self.device}")
            if t.numel() != int(segs[i, 1]):
                raise ValueError(f"segment {i}: {t.numel()} elements, the plan says {int(segs[i, 1])}")
            if t.data_ptr() % 16:
                raise ValueError(f"segment {i}: storage must be 16-byte aligned")
        key = ptrs if ptrs is not None else tuple(t.data_ptr() for t in tensors)
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        last = self.__dict__.get("_segptr_last")  # the same pointer tuple object on the same stream: no hashing
        if last is not None and last[0] is key and last[2] == st:
            return last[1]
        cache = self.__dict__.setdefault("_segptr_cache", {})
        d = cache.get(key)
        if d is None:
            if len(cache) >= 8:  # LRU-ish: drop the oldest entry (dicts keep insertion order)
                cache.pop(next(iter(cache)))
            with torch.cuda.stream(st):
                d = torch.tensor(key, dtype=torch.int64).to(self.device, non_blocking=False)
            cache[key] = (d, st)
        else:
            d, home = d
            if home != st:
                d.record_stream(st)
        self._segptr_last = (key, d, st)
        return d

    def encode_segments(self, tensors, base=None, out=None, workspace=None, flags=0, stream=None, checked=False,
                        ptrs=None, launch=None):
        """Encode with segment i read from tensors[i] itself (coalac_encode_segptr): e.g. a model's
        parameters, no flattening copy. base: flat fp32[span] (delta mode), as encode(). launch: the current
        stream when stream is None, if the caller already has it."""
        if launch is None:
            launch = torch.cuda.current_stream(self.device) if stream is None else stream
        ptrs = self.segment_pointers(tensors, checked=checked, ptrs=ptrs, stream=launch)
        self._check_flat(base, "base")
        mine = out is None  # (buffers this call allocates need no checking)
        with _on(stream):
            out = self.empty_encoded() if out is None else out
            ws = self.empty_workspace() if workspace is None else workspace
        ust = _ptr(out.ustart) if mine else self._check_encoded(out)
        if ws.device != self.device or ws.numel() * ws.element_size() < self.ws_bytes:
            raise ValueError(f"workspace: need {self.ws_bytes} bytes on {self.device}")
        with _device_ctx(self.device):
            rc = self._lib.coalac_encode_segptr(self._h, _ptr(ptrs), _ptr(base), _idx_ptr(out.idx), _ptr(out.vals),
                                                _ptr(out.mn), _ptr(out.scale), ust, _ptr(ws),
                                                ctypes.c_uint64(self.ws_bytes), ctypes.c_uint(flags),
                                                ctypes.c_void_p(launch.cuda_stream))
        _lib.check(rc, "coalac_encode_segptr")
        return out

    def encode_sr(self, flat=None, tensors=None, base=None, seed=0, out=None, workspace=None, flags=0, stream=None,
                  checked=False, ptrs=None):
        """The dense (every k == n, bits 1..8) encode with stochastic (unbiased) rounding (coalac_encode_sr, DESIGN.md
        §18): mn / scale as encode() computes them, every code floor(t) or floor(t) + 1 by a hash of `seed` (64 bits)
        and the element's position — the same seed gives the same codes, from `flat` (fp32[span]) as from `tensors`
        (one per segment, as encode_segments reads them); exactly one of the two. base, out, workspace as encode();
        idx and the per-unit starts are implied and not written. Asynchronous on `stream`."""
        self._need_dense("encode_sr")
        if (flat is None) == (tensors is None):
            raise ValueError("encode_sr: give exactly one of flat and tensors")
        self._check_flat(base, "base")
        launch = torch.cuda.current_stream(self.device) if stream is None else stream
        if tensors is not None:
            seg, x = _ptr(self.segment_pointers(tensors, checked=checked, ptrs=ptrs, stream=launch)), _ptr(None)
        else:
            self._check_flat(flat, "input")
            seg, x = _ptr(None), _ptr(flat)
        with _on(stream):
            out = self.empty_encoded(with_idx=False) if out is None else out
            ws = self.empty_workspace() if workspace is None else workspace
        self._check_encoded(out)
        if ws.device != self.device or ws.numel() * ws.element_size() < self.ws_bytes:
            raise ValueError(f"workspace: need {self.ws_bytes} bytes on {self.device}")
        fn = self._sr_entry("coalac_encode_sr")
        with _device_ctx(self.device):
            rc = fn(self._h, x, seg, _ptr(base), _ptr(out.vals), _ptr(out.mn), _ptr(out.scale), _ptr(ws),
                    ctypes.c_uint64(self.ws_bytes), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                    ctypes.c_uint(flags), ctypes.c_void_p(launch.cuda_stream))
        _lib.check(rc, "coalac_encode_sr")
        return out

    # -- error feedback ---------------------------------------------------------------------------
    def ef_accumulate(self, resid, flat=None, tensors=None, base=None, stream=None, checked=False, ptrs=None):
        """resid = (x - base) + resid over every segment (coalac_ef_accumulate; fp32 subtract then add, base None:
        x + resid), x read from `flat` (fp32[span]) or from `tensors` (one per segment, as encode_segments reads
        them) — exactly one of the two. The padding between segments is not written. Asynchronous on `stream`.
        An error-feedback round is ef_accumulate, encode(resid), ef_commit, all on one stream."""
        if (flat is None) == (tensors is None):
            raise ValueError("ef_accumulate: give exactly one of flat and tensors")
        self._check_flat(resid, "residual")
        self._check_flat(base, "base")
        launch = torch.cuda.current_stream(self.device) if stream is None else stream
        if tensors is not None:
            seg, x = _ptr(self.segment_pointers(tensors, checked=checked, ptrs=ptrs, stream=launch)), _ptr(None)
        else:
            self._check_flat(flat, "input")
            seg, x = _ptr(None), _ptr(flat)
        with _device_ctx(self.device):
            rc = self._lib.coalac_ef_accumulate(self._h, x, seg, _ptr(base), _ptr(resid),
                                                ctypes.c_void_p(launch.cuda_stream))
        _lib.check(rc, "coalac_ef_accumulate")
        return resid

    def ef_commit(self, enc, resid, stream=None):
        """resid[pos] -= what decode(enc) reconstructs there, at every kept entry of enc (coalac_ef_commit; +0.0
        where the difference is not finite); the other positions are left as they are. enc: the Encoded of
        encode(resid) on the same stream. A sparse plan needs enc.ustart (the encode writes it)."""
        ust = self._check_encoded(enc)
        if not self.dense and (enc.ustart is None or enc.idx.numel() < self.total_k):
            raise ValueError("ef_commit: a sparse plan needs the encode's idx and per-unit starts (ustart)")
        self._check_flat(resid, "residual")
        with _device_ctx(self.device):
            rc = self._lib.coalac_ef_commit(self._h, _idx_ptr(enc.idx), _ptr(enc.vals), _ptr(enc.mn), _ptr(enc.scale),
                                            ust, _ptr(resid), _stream_handle(stream))
        _lib.check(rc, "coalac_ef_commit")
        return resid

    # -- compact payload (wire v3) ----------------------------------------------------------------
    @property
    def packed_words(self):
        """uint32 words of the plan's packed entry stream: ceil(total_k * (12 + code bits) / 32) (wire.py)."""
        n = self.__dict__.get("_packed_words")
        if n is None:
            b = ctypes.c_uint64()
            _lib.check(self._lib.coalac_plan_packed_bytes(self._h, ctypes.byref(b)), "coalac_plan_packed_bytes")
            n = self._packed_words = b.value // 4
        return n

    def _check_packed(self, t, name):
        if t.device != self.device or t.dtype != torch.uint32 or not t.is_contiguous() or t.numel() < self.packed_words:
            raise ValueError(f"{name}: need a contiguous uint32[{self.packed_words}] tensor on {self.device}, got "
                             f"{t.dtype}[{t.numel()}] on {t.device}")

    def pack(self, enc, out=None, stream=None):
        """enc.idx / enc.vals -> the packed entry stream, uint32[packed_words] (coalac_pack: one (12 + code bits)-bit
        field per entry position; at bits 32 the values are not read). Asynchronous on `stream`; a dense plan has
        nothing to pack (ValueError)."""
        if self.dense:
            raise ValueError("pack: a dense plan's indices are implied, there is nothing to pack")
        self._check_encoded(enc)
        if enc.idx.numel() < self.total_k:
            raise ValueError(f"pack: idx holds {enc.idx.numel()} entries, the plan has {self.total_k}")
        if enc.idx.data_ptr() % 16 or enc.vals.data_ptr() % 16:
            raise ValueError("pack: idx / vals storage must be 16-byte aligned")
        with _on(stream):
            if out is None:
                out = torch.empty(self.packed_words, dtype=torch.uint32, device=self.device)
        self._check_packed(out, "packed output")
        with _device_ctx(self.device):
            rc = self._lib.coalac_pack(self._h, _ptr(enc.idx), _ptr(enc.vals), _ptr(out),
                                       ctypes.c_uint64(4 * out.numel()), _stream_handle(stream))
        _lib.check(rc, "coalac_pack")
        return out

    def unpack(self, packed, ustart, out=None, stream=None):
        """The packed entry stream + the per-unit starts -> (idx int32[total_k], vals) (coalac_unpack). out: an
        (idx, vals) pair to write into — only the positions of the plan's own segments are written; at bits 32 vals
        is not written (the fp32 values travel in their own section). Asynchronous on `stream`."""
        if self.dense:
            raise ValueError("unpack: a dense plan's indices are implied, there is nothing to unpack")
        self._check_packed(packed, "packed stream")
        if ustart.device != self.device or ustart.dtype != torch.int32 or not ustart.is_contiguous() or \
                ustart.numel() != self.n_units:
            raise ValueError(f"unpack: need the plan's {self.n_units} per-unit starts as a contiguous int32 tensor on "
                             f"{self.device}, got {ustart.dtype}[{ustart.numel()}] on {ustart.device}")
        with _on(stream):
            if out is None:
                out = (torch.empty(self.total_k, dtype=torch.int32, device=self.device),
                       torch.empty(self.total_k, dtype=self.vals_dtype, device=self.device))
        idx, vals = out
        for t, dt in ((idx, torch.int32), (vals, self.vals_dtype)):
            if t.device != self.device or t.dtype != dt or not t.is_contiguous() or t.numel() < self.total_k:
                raise ValueError(f"unpack output: need {dt}[{self.total_k}] on {self.device}, got "
                                 f"{t.dtype}[{t.numel()}] on {t.device}")
        with _device_ctx(self.device):
            rc = self._lib.coalac_unpack(self._h, _ptr(packed), ctypes.c_uint64(4 * packed.numel()), _ptr(ustart),
                                         _ptr(idx), _ptr(vals), _stream_handle(stream))
        _lib.check(rc, "coalac_unpack")
        return idx, vals

    # -- bit-packed dense codes (wire v4) ---------------------------------------------------------
    @property
    def dense_packed_words(self):
        """uint32 words of a dense plan's bit-packed code stream: the sum over its segment rows of
        ceil(n * bits / 32) (wire.dense_packed_words). A sparse plan, or bits 32, has none (ValueError)."""
        n = self.__dict__.get("_dense_packed_words")
        if n is None:
            self._need_dense("dense_packed_words")
            b = ctypes.c_uint64()
            _lib.check(self._lib.coalac_plan_dense_packed_bytes(self._h, ctypes.byref(b)),
                       "coalac_plan_dense_packed_bytes")
            n = self._dense_packed_words = b.value // 4
        return n

    def _need_dense(self, who):
        if not self.dense:
            raise ValueError(f"{who}: needs a dense plan (every segment keeps all its elements); a sparse plan's "
                             "payload is packed by pack / unpack")
        if self.bits == RAW_BITS:
            raise ValueError(f"{who}: bits 32 has no codes to pack")

    def _check_dense_packed(self, t, name):
        n = self.dense_packed_words
        if t.device != self.device or t.dtype != torch.uint32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError(f"{name}: need a contiguous uint32[{n}] tensor on {self.device}, got "
                             f"{t.dtype}[{t.numel()}] on {t.device}")

    def _check_codes(self, t, name):
        if t.device != self.device or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() < self.total_k:
            raise ValueError(f"{name}: need a contiguous uint8[{self.total_k}] tensor on {self.device}, got "
                             f"{t.dtype}[{t.numel()}] on {t.device}")
        if t.data_ptr() % 4:  # (the kernels take whole dwords where a unit's codes start on one)
            raise ValueError(f"{name}: storage must be 4-byte aligned")

    def pack_dense(self, enc, out=None, stream=None):
        """A dense plan's uint8 codes (enc: an Encoded, or the codes tensor itself) -> the bit-packed stream,
        uint32[dense_packed_words] (coalac_pack_dense: every code as a `bits`-bit field, each segment's fields from a
        word boundary on). Asynchronous on `stream`."""
        self._need_dense("pack_dense")
        vals = enc.vals if isinstance(enc, Encoded) else enc
        self._check_codes(vals, "pack_dense codes")
        with _on(stream):
            if out is None:
                out = torch.empty(self.dense_packed_words, dtype=torch.uint32, device=self.device)
        self._check_dense_packed(out, "packed output")
        with _device_ctx(self.device):
            rc = self._lib.coalac_pack_dense(self._h, _ptr(vals), _ptr(out), ctypes.c_uint64(4 * out.numel()),
                                             _stream_handle(stream))
        _lib.check(rc, "coalac_pack_dense")
        return out

    def unpack_dense(self, packed, out=None, stream=None):
        """The bit-packed stream -> the uint8 codes, uint8[total_k] (coalac_unpack_dense); `out`: a buffer to write
        into — only the positions of the plan's own segments are written. Asynchronous on `stream`."""
        self._need_dense("unpack_dense")
        self._check_dense_packed(packed, "packed stream")
        with _on(stream):
            if out is None:
                out = torch.empty(self.total_k, dtype=torch.uint8, device=self.device)
        self._check_codes(out, "unpack_dense output")
        with _device_ctx(self.device):
            rc = self._lib.coalac_unpack_dense(self._h, _ptr(packed), ctypes.c_uint64(4 * packed.numel()), _ptr(out),
                                               _stream_handle(stream))
        _lib.check(rc, "coalac_unpack_dense")
        return out

    def _check_ranges(self, who, n, names, *ts):
        for t in ts:
            if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
                raise ValueError(f"{who}: need {names} as float32[{n}] on {self.device}, got "
                                 f"{t.dtype}[{t.numel()}] on {t.device}")

    def _decode_stream(self, fn, who, n, names, packed, r0, r1, base, out, stream):
        # decode_packed / decode_block: one call of fn, the ranges (r0, r1: `names`, n of each) one per segment or unit
        self._need_dense(who)
        self._check_dense_packed(packed, "packed stream")
        self._check_ranges(who, n, names, r0, r1)
        self._check_flat(base, "base")
        with _on(stream):
            if out is None:
                out = self.empty_flat() if base is None else torch.empty_like(base)
        self._check_flat(out, "output")
        with _device_ctx(self.device):
            rc = fn(self._h, _ptr(packed), ctypes.c_uint64(4 * packed.numel()), _ptr(r0), _ptr(r1), _ptr(base),
                    _ptr(out), _stream_handle(stream))
        _lib.check(rc, fn.__name__)
        return out

    def decode_packed(self, packed, mn, scale, base=None, out=None, stream=None):
        """decode() of a dense plan straight from the bit-packed stream (coalac_decode_packed: no byte-per-element
        intermediate) -> dense flat fp32[span] (+ base, fused); bit-identical to unpack_dense followed by decode.
        Asynchronous on `stream`."""
        return self._decode_stream(self._lib.coalac_decode_packed, "decode_packed", self.n_segments, "mn / scale",
                                   packed, mn, scale, base, out, stream)

    # -- block-wise dense quantisation (wire v5) --------------------------------------------------
    def empty_block_encoded(self, block=UNIT):
        """(bmn fp32[n_units], bscale fp32[n_units], packed uint32[dense_packed_words]) as views of ONE allocation
        (16-byte aligned each): the outputs of encode_block; with another block size (encode_block_g) the ranges hold
        block_count(block) entries."""
        U, P = self.block_count(block), self.dense_packed_words
        a = (4 * U + 15) // 16 * 16
        buf = torch.empty(2 * a + 4 * P, dtype=torch.uint8, device=self.device)
        return (buf[:4 * U].view(torch.float32), buf[a:a + 4 * U].view(torch.float32),
                buf[2 * a:2 * a + 4 * P].view(torch.uint32))

    def encode_block(self, flat=None, tensors=None, base=None, out=None, stream=None, checked=False, ptrs=None):
        """Block-wise encode of a dense plan (coalac_encode_block): every 4096-element unit quantised over its own
        range, in one pass -> (bmn fp32[n_units], bscale fp32[n_units], packed uint32[dense_packed_words]), the code
        stream in wire v4's layout. The update is read from `flat` (fp32[span]) or from `tensors` (one per segment, as
        encode_segments reads them) — exactly one of the two; base: flat fp32[span] (delta mode). out: such a triple
        to write into. Asynchronous on `stream`."""
        return self._encode_block("encode_block", None, flat, tensors, base, out, stream, checked, ptrs)

    def encode_block_sr(self, flat=None, tensors=None, base=None, seed=0, out=None, stream=None, checked=False,
                        ptrs=None):
        """encode_block with stochastic (unbiased) rounding (coalac_encode_block_sr): the same ranges,
        every code floor(t) or floor(t) + 1 by a hash of `seed` (64 bits) and the element's position — the same seed
        gives the same stream, and decode_block / aggregate_dense read it as any other."""
        return self._encode_block("encode_block_sr", seed, flat, tensors, base, out, stream, checked, ptrs)

    @property
    def has_block_ef(self):
        """Whether the loaded library exports coalac_encode_block_ef (an ABI-11 build from before it does not)."""
        return hasattr(self._lib, "coalac_encode_block_ef")

    def encode_block_ef(self, residual, flat=None, tensors=None, base=None, out=None, stream=None, checked=False,
                        ptrs=None):
        """encode_block with error feedback in the same pass (coalac_encode_block_ef): the unit
        quantised is a = (x - base) + residual, and residual (fp32[span], this plan's flat layout, as ef_accumulate
        takes it) leaves as a - decoded (+0.0 where that is not finite), rewritten in place; the padding between
        segments is not written. Bit for bit ef_accumulate, encode_block(flat=residual) and the subtraction of
        decode_block's output, in one launch. Returns encode_block's triple, an ordinary delta-mode wire v5 payload.
        Asynchronous on `stream`."""
        return self._encode_block("encode_block_ef", None, flat, tensors, base, out, stream, checked, ptrs,
                                  resid=residual)

    def _sr_entry(self, name, since="stochastic rounding"):
        fn = getattr(self._lib, name, None)
        if fn is None:
            raise _lib.CodecError(f"the loaded codec library has no {name} (built before {since})")
        return fn

    def _encode_block(self, who, seed, flat, tensors, base, out, stream, checked, ptrs, resid=None, block=UNIT,
                      rot_seed=None):
        # encode_block / encode_block_sr (seed None: the deterministic entry point) / encode_block_ef (resid given) /
        # encode_block_g (block below 4096) / encode_block_rot (rot_seed given; seed None: round to nearest)
        self._need_dense(who)
        if (flat is None) == (tensors is None):
            raise ValueError(f"{who}: give exactly one of flat and tensors")
        ef = who == "encode_block_ef"
        if ef:
            if resid is None:
                raise ValueError("encode_block_ef: residual is None")
            self._check_flat(resid, "residual")
        self._check_flat(base, "base")
        launch = torch.cuda.current_stream(self.device) if stream is None else stream
        if tensors is not None:
            seg, x = _ptr(self.segment_pointers(tensors, checked=checked, ptrs=ptrs, stream=launch)), _ptr(None)
        else:
            self._check_flat(flat, "input")
            seg, x = _ptr(None), _ptr(flat)
        if out is None:
            with _on(stream):
                out = self.empty_block_encoded(block)
        bmn, bscale, packed = out
        self._check_ranges(who, self.block_count(block), "bmn / bscale", bmn, bscale)
        self._check_dense_packed(packed, "packed output")
        args = (self._h, x, seg, _ptr(base), _ptr(bmn), _ptr(bscale), _ptr(packed), ctypes.c_uint64(4 * packed.numel()))
        st = ctypes.c_void_p(launch.cuda_stream)
        if rot_seed is not None:
            who = "encode_block_rot" if seed is None else "encode_block_rot_sr"
            fn = self._sr_entry("coalac_" + who, since="the rotated block-wise quantisation")
            seeds = [ctypes.c_uint64(int(s) & 0xFFFFFFFFFFFFFFFF) for s in ((rot_seed,) if seed is None else (rot_seed, seed))]
            with _device_ctx(self.device):
                rc = fn(*args, *seeds, st)
        elif block != UNIT:
            with _device_ctx(self.device):
                rc = self._lib.coalac_encode_block_g(self._h, ctypes.c_uint32(block), *args[1:], st)
        elif ef:
            fn = self._sr_entry("coalac_encode_block_ef", since="the fused block-wise error feedback")
            with _device_ctx(self.device):
                rc = fn(*args[:4], _ptr(resid), *args[4:], st)
        elif seed is None:
            with _device_ctx(self.device):
                rc = self._lib.coalac_encode_block(*args, st)
        else:
            fn = self._sr_entry("coalac_encode_block_sr")
            with _device_ctx(self.device):
                rc = fn(*args, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), st)
        _lib.check(rc, "coalac_" + who)
        return bmn, bscale, packed

    # -- rotated block-wise quantisation -------------------------------------------
    @property
    def has_block_rot(self):
        """Whether the loaded library exports the rotated entry points (an ABI-11 build from before them does not)."""
        return all(hasattr(self._lib, n) for n in _lib.ADDED_FOR_ROTATION)

    def encode_block_rot(self, flat=None, tensors=None, base=None, rot_seed=0, seed=None, out=None, stream=None,
                         checked=False, ptrs=None):
        """encode_block with every full 4096-element unit rotated first (coalac_encode_block_rot): a sign
        diagonal drawn from `rot_seed` (64 bits) and the orthonormal Walsh-Hadamard transform, the coefficients quantised
        as encode_block quantises the values; a unit shorter than 4096 is encode_block's. seed: None rounds to nearest,
        a 64-bit seed rounds stochastically as encode_block_sr does (coalac_encode_block_rot_sr). The triple has
        encode_block's shapes; only decode_block_rot with the same rot_seed reads it. Asynchronous on `stream`."""
        return self._encode_block("encode_block_rot", seed, flat, tensors, base, out, stream, checked, ptrs,
                                  rot_seed=rot_seed)

    def decode_block_rot(self, packed, bmn, bscale, rot_seed, base=None, out=None, stream=None):
        """Decode of a rotated block-wise stream (coalac_decode_block_rot): decode_block, then the inverse rotation of
        every full unit under `rot_seed` -> dense flat fp32[span] (+ base, fused). Asynchronous on `stream`."""
        raw = self._sr_entry("coalac_decode_block_rot", since="the rotated block-wise quantisation")
        rs = ctypes.c_uint64(int(rot_seed) & 0xFFFFFFFFFFFFFFFF)

        def fn(h, packed_p, nbytes, r0, r1, *rest):
            return raw(h, packed_p, nbytes, r0, r1, rs, *rest)
        fn.__name__ = "coalac_decode_block_rot"
        return self._decode_stream(fn, "decode_block_rot", self.n_units, "bmn / bscale", packed, bmn, bscale, base, out,
                                   stream)

    # -- block-wise with 256- and 1024-element blocks ------------------------------
    BLOCK_SIZES = (256, 1024, UNIT)

    @property
    def has_block_g(self):
        """Whether the loaded library exports the block-size entry points (an ABI-11 build from before them does not:
        only block size 4096 works on it, through the entry points it has)."""
        return all(hasattr(self._lib, n) for n in _lib.ADDED_FOR_BLOCK_SIZES)

    def _block_size(self, who, block):
        if isinstance(block, bool) or not isinstance(block, int) or block not in self.BLOCK_SIZES:
            raise ValueError(f"{who}: block size {block!r}, need one of {self.BLOCK_SIZES}")
        if block != UNIT and not self.has_block_g:
            raise _lib.CodecError(f"{who}: the loaded codec library has no {_lib.ADDED_FOR_BLOCK_SIZES[1]} (built before "
                                  f"block sizes other than {UNIT})")
        return block

    def block_count(self, block=UNIT):
        """NB, the plan's number of `block`-element blocks: the sum over its segment rows of ceil(n / block)
        (coalac_plan_block_count; wire.block_count of the rows' sizes). At 4096 it is n_units."""
        self._need_dense("block_count")
        if self._block_size("block_count", block) == UNIT:
            return self.n_units
        cache = self.__dict__.setdefault("_block_counts", {})
        n = cache.get(block)
        if n is None:
            b = ctypes.c_uint64()
            _lib.check(self._lib.coalac_plan_block_count(self._h, ctypes.c_uint32(block), ctypes.byref(b)),
                       "coalac_plan_block_count")
            n = cache[block] = b.value
        return n

    def encode_block_g(self, block, flat=None, tensors=None, base=None, out=None, stream=None, checked=False, ptrs=None):
        """encode_block with `block`-element blocks (256, 1024 or 4096; coalac_encode_block_g): every block quantised over
        its own range -> (bmn fp32[NB], bscale fp32[NB], packed uint32[dense_packed_words]), NB = block_count(block);
        the stream's layout does not depend on the block size. Deterministic rounding only. At 4096 it is encode_block,
        bit for bit. Asynchronous on `stream`."""
        if self._block_size("encode_block_g", block) == UNIT:
            return self.encode_block(flat, tensors, base, out, stream, checked, ptrs)
        return self._encode_block("encode_block_g", None, flat, tensors, base, out, stream, checked, ptrs, block=block)

    def decode_block_g(self, block, packed, bmn, bscale, base=None, out=None, stream=None):
        """decode_block of a stream with `block`-element blocks (coalac_decode_block_g): bmn / bscale hold
        block_count(block) entries. At 4096 it is decode_block, bit for bit. Asynchronous on `stream`."""
        if self._block_size("decode_block_g", block) == UNIT:
            return self.decode_block(packed, bmn, bscale, base, out, stream)
        raw = self._lib.coalac_decode_block_g

        def fn(h, *args):
            return raw(h, ctypes.c_uint32(block), *args)
        fn.__name__ = "coalac_decode_block_g"
        return self._decode_stream(fn, "decode_block_g", self.block_count(block), "bmn / bscale", packed, bmn, bscale,
                                   base, out, stream)

    def aggregate_dense_g(self, block, codes, mns, scales, weights, total=None, base=None, out=None, mode="recip",
                          avg_mask=None, stream=None):
        """aggregate_dense, kind "block", of uploads with `block`-element blocks (coalac_aggregate_dense_g): every mn /
        scale holds block_count(block) entries. At 4096 it is aggregate_dense(kind="block"), bit for bit."""
        self._need_dense("aggregate_dense_g")
        self._block_size("aggregate_dense_g", block)
        return self.aggregate_dense(codes, mns, scales, weights, total, base, out, mode, avg_mask, "block", stream,
                                    _block=block)

    def decode_block(self, packed, bmn, bscale, base=None, out=None, stream=None):
        """Decode of a block-wise stream (coalac_decode_block: decode_packed with each unit's own range) -> dense flat
        fp32[span] (+ base, fused). Asynchronous on `stream`."""
        return self._decode_stream(self._lib.coalac_decode_block, "decode_block", self.n_units, "bmn / bscale",
                                   packed, bmn, bscale, base, out, stream)

    def unit_starts(self, idx, stream=None):
        """The per-unit starts (wire v2) of this plan's idx list, computed on the device for a payload that carries
        none (a version-1 blob, or an Encoded built without them): for unit j of segment s, the number of the
        segment's kept indices below j * 4096 — one searchsorted over the entries' global unit numbers, which are
        non-decreasing across the plan (segments in order, indices ascending). An unsorted (untrusted) list gives
        wrong but in-range starts; the decode kernels clamp them to their unit."""
        aux = self.__dict__.get("_starts_aux")
        if aux is None:
            segs = self.table.segs.astype("int64")
            n, k, oo = segs[:, 1], segs[:, 2], segs[:, 3]
            nu = (n + UNIT - 1) // UNIT
            ubase = torch.from_numpy((nu.cumsum() - nu).astype("int32"))
            kk, nnu = torch.from_numpy(k), torch.from_numpy(nu)
            first = torch.from_numpy((k.cumsum() - k).astype("int32"))  # each segment's first entry in the plan's list
            ents = None
            if not (oo == (k.cumsum() - k)).all():  # (a SubTable: the segments' entries sit at absolute offsets)
                ents = torch.cat([torch.arange(int(o), int(o) + int(c), dtype=torch.int64) for o, c in zip(oo, k)])
            aux = self._starts_aux = (torch.repeat_interleave(ubase, kk).to(self.device),
                                      torch.repeat_interleave(first, nnu).to(self.device),
                                      torch.arange(int(nu.sum()), dtype=torch.int32).to(self.device),
                                      None if ents is None else ents.to(self.device))
        ubase_rep, first_rep, units, ents = aux
        with _on(stream):
            own = idx[:self.total_k] if ents is None else idx[ents]
            gu = ubase_rep + torch.bitwise_right_shift(own, 12)
            return (torch.searchsorted(gu, units, out_int32=True) - first_rep).to(torch.int32)

    def _starts_for(self, enc, stream):
        """enc.ustart, or (no starts, a sparse plan) the device-computed ones."""
        if enc.ustart is not None or self.dense:
            return enc
        return Encoded(enc.idx, enc.vals, enc.mn, enc.scale, self.unit_starts(enc.idx, stream))

    def decode(self, enc, base=None, out=None, stream=None, events=None):
        """Decode Encoded -> dense flat fp32[span] (+ base, fused). Asynchronous on `stream`.

        enc.ustart: the wire v2 per-unit starts; without them (a v1 payload) they are computed on the device first
        (unit_starts). events: 3 timing events (coalac_decode_ev: [1] / [2] bracket the decode kernel)."""
        self._check_encoded(enc)
        enc = self._starts_for(enc, stream)
        ust = self._check_encoded(enc)
        self._check_flat(base, "base")
        with _on(stream):
            if out is None:
                out = self.empty_flat() if base is None else torch.empty_like(base)
        self._check_flat(out, "output")
        args = (self._h, _idx_ptr(enc.idx), _ptr(enc.vals), _ptr(enc.mn), _ptr(enc.scale), ust, _ptr(base), _ptr(out),
                _stream_handle(stream))
        with torch.cuda.device(self.device):
            if events is None:
                rc = self._lib.coalac_decode(*args)
            else:
                rc = self._lib.coalac_decode_ev(*args, _event_array(events, 3))
        _lib.check(rc, "coalac_decode")
        return out

    def aggregate(self, enc, weights, total=None, base=None, out=None, mode="recip", stream=None, events=None,
                  avg_mask=None):
        """Fused decode + FedAvg of the plan's `clients` updates (coalac_aggregate).

        enc: the batched Encoded of all clients (client-major, as encode() produces). weights: one
        number per client (FedAvg weights, e.g. sample counts); total: their sum (default
        sum(weights)). Returns out fp32[span_per_client] indexed like client 0's segments:
        base + decoded_i averaged exactly as coala/server/strategies.py:6-29,57-90 would on the decoded
        modules — mode "recip" reproduces torch on the GPU (division by a host scalar becomes a multiply
        by its fp32 reciprocal), "div" torch on the CPU, "sum" stops before the division (weighted_sum,
        strategies.py:57-90: what a multi-GPU server hands to reduce_models, distributed.py:42-57).
        avg_mask: one bool per segment of a client (None: all True); a False segment is not averaged but
        takes client 0's decoded value — aggregation_content "parameters" (strategies.py:32-54, 93-124).
        enc.ustart: the clients' per-unit starts, concatenated (computed on the device when absent).
        """
        self._check_encoded(enc)
        if not getattr(self.table, "uniform", False):
            raise ValueError("fused aggregation needs a plan over copies of one layout (a SegmentTable)")
        if self.dense and enc.idx.numel() == 0:  # (the aggregate kernel reads explicit indices: the implied ones and
            with _on(stream):                      # the implied starts, both made once per plan)
                enc = Encoded(self.implied_indices(), enc.vals, enc.mn, enc.scale,
                              self.implied_starts() if enc.ustart is None else enc.ustart)
        if enc.ustart is None:
            enc = Encoded(enc.idx, enc.vals, enc.mn, enc.scale, self.unit_starts(enc.idx, stream))
        ust = self._check_encoded(enc)
        C = self.table.clients
        if len(weights) != C:
            raise ValueError(f"need {C} weights, got {len(weights)}")
        modes = {"recip": _lib.COALAC_AGG_RECIP, "div": _lib.COALAC_AGG_DIV, "sum": _lib.COALAC_AGG_SUM}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, got {mode!r}")
        n_out = self.table.span_per_client
        if base is not None:
            self._check_flat(base, "base", n_out)
        with _on(stream):
            out = torch.empty(n_out, dtype=torch.float32, device=self.device) if out is None else out
            w = torch.tensor([float(x) for x in weights], dtype=torch.float64).to(torch.float32).to(self.device)
            m = None
            if avg_mask is not None:
                if len(avg_mask) != len(self.table.sizes):
                    raise ValueError(f"avg_mask: need {len(self.table.sizes)} entries, got {len(avg_mask)}")
                m = torch.tensor([1 if x else 0 for x in avg_mask], dtype=torch.uint8).to(self.device)
        # (the kernel writes the segments' elements only: an output that ends with the last segment suffices,
        # e.g. a decoded module's buffer, which has no trailing alignment pad)
        self._check_flat(out, "output", self.table.offsets[-1] + self.table.sizes[-1] if self.table.sizes else 0)
        total = float(sum(weights)) if total is None else float(total)
        args = (self._h, C, _ptr(enc.idx), _ptr(enc.vals), _ptr(enc.mn), _ptr(enc.scale), ust, _ptr(w),
                ctypes.c_float(total), modes[mode], _ptr(m), _ptr(base), _ptr(out), _stream_handle(stream))
        with torch.cuda.device(self.device):
            if events is None:
                rc = self._lib.coalac_aggregate(*args)
            else:
                rc = self._lib.coalac_aggregate_ev(*args, _event_array(events, 3))
        _lib.check(rc, "coalac_aggregate")
        return out  # w / m were allocated on the launch stream: their memory is reused only after the kernel

    AGG_DENSE_KINDS = {"codes": _lib.COALAC_AGGD_CODES, "packed": _lib.COALAC_AGGD_PACKED,
                       "block": _lib.COALAC_AGGD_BLOCK}

    def aggregate_dense(self, codes, mns, scales, weights, total=None, base=None, out=None, mode="recip",
                        avg_mask=None, kind="codes", stream=None, _block=UNIT):
        """Fused decode + FedAvg of C ratio-1 uploads of THIS plan's layout (a one-client dense plan), each read from
        its own buffers (coalac_aggregate_dense): no concatenation, no `clients`-copies plan, no implied
        indices. codes / mns / scales: lists of C tensors, one per upload —

            kind "codes":  uint8[total_k] codes,                    mn / scale fp32[n_segments]
            kind "packed": uint32[dense_packed_words] (wire v4),    mn / scale fp32[n_segments]
            kind "block":  uint32[dense_packed_words],              mn / scale fp32[n_units] (wire v5: per block)

        weights, total, base, mode, avg_mask and the result as aggregate(): out fp32[span] indexed by the plan's
        segments, bit-identical to decode / decode_packed / decode_block of every upload followed by the reference's
        weighted sum and division. The pointer arrays, the weights and the mask go up in small copies on the launch
        stream. Asynchronous on `stream`."""
        self._need_dense("aggregate_dense")
        if kind not in self.AGG_DENSE_KINDS:
            raise ValueError(f"kind must be one of {sorted(self.AGG_DENSE_KINDS)}, got {kind!r}")
        modes = {"recip": _lib.COALAC_AGG_RECIP, "div": _lib.COALAC_AGG_DIV, "sum": _lib.COALAC_AGG_SUM}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, got {mode!r}")
        C = len(codes)
        if C < 1 or len(mns) != C or len(scales) != C or len(weights) != C:
            raise ValueError(f"aggregate_dense: need one codes / mn / scale tensor and one weight per upload, got "
                             f"{C} / {len(mns)} / {len(scales)} / {len(weights)}")
        stream_kind = kind != "codes"
        n_range = self.block_count(_block) if kind == "block" else self.n_segments  # (_block: aggregate_dense_g's)
        for i, (c, m, s) in enumerate(zip(codes, mns, scales)):
            if stream_kind:
                self._check_dense_packed(c, f"upload {i}: packed stream")
            else:
                self._check_codes(c, f"upload {i}: codes")
            if c.data_ptr() % 4:
                raise ValueError(f"upload {i}: the code storage must be 4-byte aligned")
            for t in (m, s):
                if t.device != self.device or t.dtype != torch.float32 or not t.is_contiguous() or \
                        t.numel() < n_range or t.data_ptr() % 4:
                    raise ValueError(f"upload {i}: need mn / scale as float32[{n_range}] on {self.device}, got "
                                     f"{t.dtype}[{t.numel()}] on {t.device}")
        if avg_mask is not None and len(avg_mask) != self.n_segments:
            raise ValueError(f"avg_mask: need {self.n_segments} entries, got {len(avg_mask)}")
        self._check_flat(base, "base")
        sizes = self.table.segs
        n_out = int((sizes[:, 0] + sizes[:, 1]).max()) if len(sizes) else 0  # (an output may end with the last segment)
        with _on(stream):
            if out is None:
                out = self.empty_flat() if base is None else torch.empty_like(base)
            # one table: the three pointer arrays, C pointers each
            ptrs = torch.tensor([t.data_ptr() for ts in (codes, mns, scales) for t in ts],
                                dtype=torch.int64).to(self.device)
            w = torch.tensor([float(x) for x in weights], dtype=torch.float64).to(torch.float32).to(self.device)
            m = None
            if avg_mask is not None:
                m = torch.tensor([1 if x else 0 for x in avg_mask], dtype=torch.uint8).to(self.device)
        self._check_flat(out, "output", n_out)
        total = float(sum(weights)) if total is None else float(total)
        code_bytes = min(c.numel() * c.element_size() for c in codes)
        p = ptrs.data_ptr()
        rest = (ctypes.c_void_p(p), ctypes.c_uint64(code_bytes), ctypes.c_void_p(p + 8 * C), ctypes.c_void_p(p + 16 * C),
                _ptr(w), ctypes.c_float(total), modes[mode], _ptr(m), _ptr(base), _ptr(out), _stream_handle(stream))
        with _device_ctx(self.device):
            if _block != UNIT:
                rc = self._lib.coalac_aggregate_dense_g(self._h, C, ctypes.c_uint32(_block), *rest)
            else:
                rc = self._lib.coalac_aggregate_dense(self._h, C, self.AGG_DENSE_KINDS[kind], *rest)
        _lib.check(rc, "coalac_aggregate_dense")
        return out  # ptrs / w / m were allocated on the launch stream: their memory is reused only after the kernel

    AGG_UPLOAD_KINDS = {"entries": _lib.COALAC_AGGS_ENTRIES, "compact": _lib.COALAC_AGGS_COMPACT}

    def aggregate_uploads(self, idxs, packeds, vals, mns, scales, ustarts, weights, total=None, base=None, out=None,
                          mode="recip", avg_mask=None, kind="entries", stream=None):
        """aggregate() of C sparse uploads of THIS plan's layout (a one-client sparse plan), each read from its own
        buffers (coalac_aggregate_uploads): no concatenation, no `clients`-copies plan. Lists of C
        tensors, one per upload (a list the kind does not read may be None) —

            kind "entries": idxs int32[total_k], vals uint8[total_k] (bits 32: fp32[total_k])      (wire v2)
            kind "compact": packeds uint32[packed_words], the wire v3 stream; vals fp32[total_k] at bits 32 only

        mns / scales: fp32[n_segments] each (not read at bits 32, may be None); ustarts: int32[n_units] each, the
        per-unit starts. weights, total, base, mode, avg_mask and the result as aggregate(): out fp32[span] indexed by
        the plan's segments, bit-identical to unpack (compact) and aggregate on the concatenated uploads. The pointer
        arrays, the weights and the mask go up in small copies on the launch stream. Asynchronous on `stream`."""
        if self.dense:
            raise ValueError("aggregate_uploads: a dense plan's uploads are aggregate_dense's")
        if kind not in self.AGG_UPLOAD_KINDS:
            raise ValueError(f"kind must be one of {sorted(self.AGG_UPLOAD_KINDS)}, got {kind!r}")
        modes = {"recip": _lib.COALAC_AGG_RECIP, "div": _lib.COALAC_AGG_DIV, "sum": _lib.COALAC_AGG_SUM}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, got {mode!r}")
        raw, compact = self.bits == 32, kind == "compact"
        # the lists the kernel reads, in the pointer table's order
        lists = [("idx", None if compact else idxs, torch.int32, self.total_k),
                 ("packed", packeds if compact else None, torch.uint32, self.packed_words if compact else 0),
                 ("vals", vals if raw or not compact else None, self.vals_dtype, self.total_k),
                 ("mn", None if raw else mns, torch.float32, self.n_segments),
                 ("scale", None if raw else scales, torch.float32, self.n_segments),
                 ("ustart", ustarts, torch.int32, self.n_units)]
        required = {"ustart", "packed" if compact else "idx"} | (set() if raw else {"mn", "scale"}) | \
            ({"vals"} if raw or not compact else set())
        C = len(weights)
        for name, ts, dt, n in lists:
            if name in required and (ts is None or len(ts) != C):
                raise ValueError(f"aggregate_uploads: need one {name} tensor per upload ({C} weights), got "
                                 f"{'none' if ts is None else len(ts)}")
        if C < 1:
            raise ValueError("aggregate_uploads: need at least one upload")
        for name, ts, dt, n in lists:
            if name not in required:
                continue
            for i, t in enumerate(ts):
                if name == "packed":
                    self._check_packed(t, f"upload {i}: packed stream")
                elif name in ("mn", "scale"):
                    self._check_ranges(f"upload {i}", n, "mn / scale", t)
                elif t.device != self.device or t.dtype != dt or not t.is_contiguous() or t.numel() < n or \
                        (name == "ustart" and t.numel() != n):
                    raise ValueError(f"upload {i}: need {name} as {dt}[{n}] on {self.device}, got "
                                     f"{t.dtype}[{t.numel()}] on {t.device}")
                if t.data_ptr() % 4:
                    raise ValueError(f"upload {i}: the {name} storage must be 4-byte aligned")
        if avg_mask is not None and len(avg_mask) != self.n_segments:
            raise ValueError(f"avg_mask: need {self.n_segments} entries, got {len(avg_mask)}")
        self._check_flat(base, "base")
        sizes = self.table.segs
        n_out = int((sizes[:, 0] + sizes[:, 1]).max()) if len(sizes) else 0  # (an output may end with the last segment)
        with _on(stream):
            if out is None:
                out = self.empty_flat() if base is None else torch.empty_like(base)
            # one table: the pointer arrays the kind reads, C pointers each
            used = [(name, ts) for name, ts, _, _ in lists if name in required]
            ptrs = torch.tensor([t.data_ptr() for _, ts in used for t in ts], dtype=torch.int64).to(self.device)
            w = torch.tensor([float(x) for x in weights], dtype=torch.float64).to(torch.float32).to(self.device)
            m = None
            if avg_mask is not None:
                m = torch.tensor([1 if x else 0 for x in avg_mask], dtype=torch.uint8).to(self.device)
        self._check_flat(out, "output", n_out)
        total = float(sum(weights)) if total is None else float(total)
        at = {name: ctypes.c_void_p(ptrs.data_ptr() + 8 * C * j) for j, (name, _) in enumerate(used)}
        arr = lambda name: at.get(name, ctypes.c_void_p(None))  # noqa: E731
        packed_bytes = min(4 * t.numel() for t in packeds) if compact else 0
        with _device_ctx(self.device):
            rc = self._lib.coalac_aggregate_uploads(
                self._h, C, self.AGG_UPLOAD_KINDS[kind], arr("idx"), arr("packed"), ctypes.c_uint64(packed_bytes),
                arr("vals"), arr("mn"), arr("scale"), arr("ustart"), _ptr(w), ctypes.c_float(total), modes[mode],
                _ptr(m), _ptr(base), _ptr(out), _stream_handle(stream))
        _lib.check(rc, "coalac_aggregate_uploads")
        return out  # ptrs / w / m were allocated on the launch stream: their memory is reused only after the kernel

    def implied_indices(self):
        """A dense plan's indices (0..n-1 per segment, every client) as a device int32 tensor, made once."""
        t = self.__dict__.get("_implied")
        if t is None:
            one = torch.cat([torch.arange(n, dtype=torch.int32) for n in self.table.segs[:, 1].tolist()])
            t = self._implied = one.to(self.device)
        return t

    def implied_starts(self):
        """A dense plan's per-unit starts (unit j of a segment starts at entry 4096 j: every element is kept), every
        client, as a device int32 tensor, made once (recomputed by a device searchsorted per call)."""
        t = self.__dict__.get("_implied_starts")
        if t is None:
            one = torch.cat([torch.arange(0, n, UNIT, dtype=torch.int32) for n in self.table.segs[:, 1].tolist()])
            t = self._implied_starts = one.to(self.device)
        return t

    def fallbacks(self, workspace, stream=None):
        """Segments of the last encode with this workspace whose sampled bracket missed (synchronises)."""
        c = ctypes.c_int()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.coalac_workspace_fallbacks(self._h, _ptr(workspace), _stream_handle(stream),
                                                            ctypes.byref(c)), "coalac_workspace_fallbacks")
        return c.value


def _event_array(events, n):
    """torch.cuda.Event list -> void*[n] of hipEvent_t (events must have been recorded once or be
    created with enable_timing; torch creates the HIP event lazily on first record)."""
    arr = (ctypes.c_void_p * n)()
    for i, e in enumerate(events[:n]):
        if e is not None:
            arr[i] = ctypes.c_void_p(e.cuda_event)
    return arr
