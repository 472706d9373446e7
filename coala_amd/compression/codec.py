"""Update codec over state_dicts: flatten -> HIP encode -> picklable carrier -> HIP decode -> module.

This is the host-side mirror of what COALA's empty compression package would provide
(/root/reference/coala/compression/__init__.py is 0 bytes). What the reference DOES pin, and this module
honours:
  * the carrier is whatever object the hook leaves in `self.model`; the reference deep-copies it and
    pickles it into UploadContent.data (/root/reference/coala/client/base.py:363,
    /root/reference/coala/protocol/codec.py:4-9), so CompressedUpdate pickles to a compact blob;
  * the server hands the decoded object to FedAvg, which iterates `state_dict()` of full modules
    including int64 `num_batches_tracked` buffers (/root/reference/coala/server/strategies.py:57-90),
    so decode returns a full nn.Module; non-fp32 entries travel raw (passthrough);
  * `calculate_model_size` calls `.parameters()` on whatever is in `self.model`
    (/root/reference/coala/client/base.py:155,474-487), so the carrier has a parameters() that reports
    its real payload size.

State / layout description: state.py; blob validation: validate.py; decoded-module clone and recycling: clone.py
(their public names are re-exported here).
"""
import ctypes
import math
import os
import threading
from collections import OrderedDict

import numpy as np
import torch
from torch import nn

from . import _lib, wire
from ._cache import IdentityCache
from .clone import _recipe, _reuse_after, _segment_views, module_with_state, release_decode_pool
from .plan import CodecPlan, Encoded
from .spec import RAW_BITS, UNIT, VALID_BITS, sr_call_seed
from .state import (FlatState, RawState, as_numpy, describe_state, describe_tensors,  # noqa: F401 (re-exported)
                    flatten_state, layout_of, module_tensors)
from .state import (_check_same_layout, _data_ptr, _decode_layout, _dense_elements, _describe, _get_device,
                    _is_contig, _layout, _layout_walk, _module_walk, _raw_snapshot, _to_host)
from .validate import MODES, validate


class HipBackend:
    """Default backend: hand-written HIP kernels behind the C ABI (coala_amd/csrc/coalac.hip)."""

    name = "hip"

    def __init__(self):
        self._gather_ptrs = IdentityCache(16)  # keyed by value: the scalars' pointers -> the same on the device

    @property
    def block_error_feedback(self):
        """Block-wise quantisation with error feedback: whether the loaded library exports
        coalac_encode_block_ef (an ABI-11 build from before it loads without the symbol)."""
        return hasattr(_lib.load(), "coalac_encode_block_ef")

    def default_device(self):
        return torch.device("cuda", torch.cuda.current_device())

    def runs_on(self, device):
        return torch.device(device).type == "cuda"

    def make_plan(self, sizes, ratio, bits, device, clients=1):
        if device.type != "cuda":
            raise RuntimeError(f"the HIP codec runs on GPU tensors only; got tensors on {device} "
                               "(there is no CPU fallback)")
        return CodecPlan(sizes, ratio, bits, clients=clients, device=device)

    def gather_scalars(self, ts, described=None):
        """One contiguous copy of the one-element tensors ts (one dtype, one GPU) in a single launch
        (coalac_gather), or None when they do not qualify (the caller then stacks them with torch).
        described: the _Described these tensors came from (their pointers; the checks run once per layout)."""
        t0 = ts[0]
        if described is not None and described.raw_ok is False:
            return None
        if t0.device.type != "cuda":
            return None
        dev, size = t0.device, t0.element_size()
        if size not in (1, 2, 4, 8):  # (coalac_gather copies 1/2/4/8-byte elements; complex128 is stacked)
            return None
        ptrs = tuple(map(_data_ptr, ts)) if described is None else described.raw_ptrs
        if described is None or described.raw_ok is None:
            ok = list(map(_get_device, ts)) == [dev.index] * len(ts) and not any(p % size for p in ptrs)
            if described is not None:
                described.raw_ok = ok
            if not ok:
                return None
        d = self._gather_ptrs.get((), ptrs, lambda: torch.tensor(ptrs, dtype=torch.int64).to(dev))
        st = torch.cuda.current_stream(dev)
        d.record_stream(st)  # (an eviction from the cache never hands its memory to a kernel still reading it)
        out = torch.empty(len(ts), dtype=t0.dtype, device=dev)
        lib = _lib.load()
        _lib.check(lib.coalac_gather(ctypes.c_void_p(d.data_ptr()), len(ts), size, ctypes.c_void_p(out.data_ptr()),
                                     ctypes.c_void_p(st.cuda_stream)), "coalac_gather")
        return out


_PACKED_HEADERS = IdentityCache(16)  # (layout entries; header fields, raw sizes) -> header JSON bytes


def _raw_nbytes(raw):
    """Bytes of an update's passthrough entries (a RawState, or a plain {name: tensor})."""
    return raw.nbytes if isinstance(raw, RawState) else sum(t.numel() * t.element_size() for t in raw.values())


class CompressedUpdate:
    """Picklable carrier of one compressed client update (what `compression()` leaves in self.model).

    Holds the encoded buffers (device tensors right after encode; CPU tensors after unpickling) and the
    raw passthrough entries. Pickles to the COALAQ1 blob (wire.py). A compact carrier (header "compact": wire
    v3) also holds the packed entry stream, `packed`, and ships that instead of idx and the uint8 codes. A block-wise
    carrier (header "blockwise": wire v5) holds one mn / scale per 4096-element block and the bit-packed code stream;
    its uint8 codes exist only where a blob was unpacked on the host.
    """

    def __init__(self, header, encoded, raw, blob=None, packed=None):
        self.header, self.encoded, self.raw = header, encoded, raw
        # a compact carrier's packed entry stream (uint32[P]): the device buffer the encode packed, or None until
        # first asked for (encoded buffers on the CPU, or a backend without pack); shared by every deep copy
        self._packed = [packed]
        # the packed COALAQ1 bytes, built on first pickle and shared by every deep copy: the reference
        # pickles copy.deepcopy(self.model) (client/base.py:363), so the payload is packed once
        self._blob = [blob]

    def __deepcopy__(self, memo):
        # The encoded payload is immutable after encode: a deep copy shares it (and the packed blob, and the header's
        # "entries" list, never mutated) instead of a D2H + pack + unpack round trip through __getstate__/__setstate__.
        other = memo[id(self)] = CompressedUpdate.__new__(CompressedUpdate)
        other.__dict__.update(self.__dict__, header=dict(self.header))
        return other

    @property
    def packed(self):
        """A compact carrier's packed entry stream (wire.py, version 3), or a dense-packed carrier's bit-packed code
        stream (version 4), as a uint32 tensor; else None. Packed on the GPU right after the encode where the plan can
        (CodecPlan.pack / pack_dense); otherwise on the host, on first use (a received carrier: its blob's section)."""
        stream, bits = wire.format_of(self.header).stream, self.header["bits"]
        if stream is None:
            return None
        if self._packed[0] is None:
            blob = self._blob[0]
            if stream == "entries":
                words = wire.pack_entries(*_to_host(self.encoded.idx, self.encoded.vals), bits)
            elif blob is not None:
                o, n = wire.sections(blob, self.header)[1]["packed"]
                words = np.frombuffer(blob, dtype="<u4", count=n // 4, offset=o).copy()
            else:
                words = wire.pack_dense_codes(_to_host(self.encoded.vals)[0], self._seg_sizes(), bits)
            self._packed[0] = torch.from_numpy(words)
        return self._packed[0]

    def _seg_sizes(self):
        return _decode_layout(self.header["entries"]).sizes

    @property
    def signature(self):
        """(ratio, bits, mode, wire version): what updates must share, next to their layout, to be aggregated as one."""
        h = self.header
        return h["ratio"], h["bits"], h["mode"], wire.format_of(h).version

    # -- size accounting (client/base.py:155, 474-487) -------------------------------------------
    @property
    def nbytes(self):
        """The payload's bytes: its array sections (wire.section_list) and the raw passthrough entries."""
        return sum(n * dt.itemsize for _, dt, n in wire.section_list(self.header)) + _raw_nbytes(self.raw)

    def parameters(self):
        """One meta tensor whose numel * 32 bit equals the payload size, so the reference's
        calculate_model_size reports the real upload size even without the plugin's override."""
        yield torch.empty(int(math.ceil(self.nbytes / 4)), device="meta")

    # -- wire -------------------------------------------------------------------------------------
    def to_bytes(self):
        if self._blob[0] is None:
            self._blob[0] = self._pack()
        return self._blob[0]

    def _pack(self):
        h = self.header
        raw = self.raw
        rawb = raw.entry_bytes() if isinstance(raw, RawState) else {
            n: (t.cpu().contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b"")
            for n, t in raw.items()}
        wh = dict(h, dense=True) if wire.is_dense(h) else h  # the header as the blob spells it

        def header_json():
            entries, pos = [], 0
            for e in h["entries"]:
                if e["kind"] == "raw":
                    nb = len(rawb[e["name"]])
                    e = dict(e, off=pos, nbytes=nb)
                    pos += nb
                entries.append(e)
            return wire.encode_header(dict(wh, entries=entries))
        # its JSON (with each raw entry's blob offset) depends on the layout and the raw byte counts only
        hjson = _PACKED_HEADERS.get(h["entries"], (self.signature, h["n_segments"], h.get("total_k"), h.get("n_units"),
                                                   h.get("n_blocks"), h.get("blockwise"), h.get("rotate"),
                                                   tuple(map(len, rawb.values()))), header_json)
        # ONE device-to-host copy, of the buffers the format ships (wire.section_list) and no other: where a packed
        # stream travels, idx and the uint8 codes stay where they are
        enc = self.encoded
        names = [name for name, _, _ in wire.section_list(h)]
        arrs = dict(zip(names, _to_host(*(self.packed.to(enc.mn.device) if name == "packed" else getattr(enc, name)
                                          for name in names))))
        rawbytes = b"".join(rawb[e["name"]] for e in h["entries"] if e["kind"] == "raw")
        return wire.pack(wh, arrs["mn"], arrs["scale"], arrs.get("idx"), arrs.get("vals"), rawbytes, header_json=hjson,
                         ustart=arrs.get("ustart"), packed=arrs.get("packed"))

    def encoded_to(self, device, staging=None, plan=None, keep_packed=False):
        """The encoded buffers on `device`. An unpickled update (the server side of a remote upload,
        coala/server/service.py:81-111) is moved with ONE host-to-device copy of the blob's mn / scale /
        idx / vals region through `staging` (a pinned host buffer: staging(nbytes) -> uint8 tensor), so
        the copy is asynchronous on the caller's stream; device tensors are typed views into it. A compact
        blob's region (mn ... ustart) holds the packed stream: idx / vals are then materialised on the device by
        `plan`.unpack (the decoding plan of this update; without one, the host-unpacked buffers are copied). A
        dense-packed blob (wire v4) for a plan that decodes the stream (decode_packed): its mn ... packed region, the
        stream staying packed on the device; a block-wise blob (wire v5) likewise, always: its decode (decode_block)
        reads nothing but the stream.
        keep_packed: a compact update stays compact — an Encoded whose `packed` is the entry stream on `device`, idx
        empty and vals None (bits 32: the fp32 values), for a reader of the stream itself (CodecPlan.aggregate_uploads,
        kind "compact"); a blob's staged mn ... ustart region is all there is, with no unpack and no room for idx /
        vals. A carrier that has neither its stream on `device` nor a blob (stream_for), and every other format, is
        handed out as without the keyword."""
        device = torch.device(device)
        cuda, blob, enc = device.type == "cuda", self._blob[0], self.encoded
        fmt = wire.format_of(self.header)
        if keep_packed and self.stream_for(device):
            f32 = self.header["bits"] == RAW_BITS
            pk = self._packed[0]
            if pk is not None and pk.device == device and enc.mn.device == device:
                # a local carrier: its buffers as they are, with the stream the encode packed
                return Encoded(enc.idx, enc.vals, enc.mn, enc.scale, enc.ustart, pk)
            no_idx = torch.empty(0, dtype=torch.int32, device=device)
            if staging is None or not cuda:
                to = lambda t: t.to(device, non_blocking=True)  # noqa: E731
                return Encoded(no_idx, to(enc.vals) if f32 else None, to(enc.mn), to(enc.scale), to(enc.ustart),
                               to(self._blob_stream()))
            view, _ = self._staged_sections(device, staging)
            return Encoded(no_idx, view("vals", torch.float32) if f32 else None, view("mn", torch.float32),
                           view("scale", torch.float32), view("ustart", torch.int32), view("packed", torch.uint32))
        if fmt.stream == "dense" and (fmt.per_block or (cuda and getattr(plan, "decode_packed", None) is not None)):
            # for a plan that reads the stream: an Encoded whose `packed` is the bit-packed stream on `device`, with no
            # uint8 codes there (vals None: CodecPlan.unpack_dense makes them for who needs them); a carrier whose
            # buffers are on the device already is handed out as it is
            if enc.mn.device == device:
                return Encoded(enc.idx, enc.vals, enc.mn, enc.scale, None, self.packed.to(device, non_blocking=True))
            no_idx = torch.empty(0, dtype=torch.int32, device=device)
            if blob is None or staging is None or not cuda:
                return Encoded(no_idx, None, enc.mn.to(device, non_blocking=True),
                               enc.scale.to(device, non_blocking=True), None, self.packed.to(device, non_blocking=True))
            view, _ = self._staged_sections(device, staging)
            return Encoded(no_idx, None, view("mn", torch.float32), view("scale", torch.float32), None,
                           view("packed", torch.uint32))
        compact = fmt.stream == "entries"
        if (staging is None or not cuda or blob is None or wire.is_dense(self.header)
                or enc.idx.device == device or (compact and getattr(plan, "unpack", None) is None)):
            return enc.to(device, non_blocking=True)
        K, f32 = int(self.header["total_k"]), self.header["bits"] == RAW_BITS
        vdt = torch.float32 if f32 else torch.uint8
        # a compact blob: idx (and the uint8 codes) are unpacked behind the region
        view, room = self._staged_sections(device, staging, 4 * K + (0 if f32 else K) if compact else 0)
        mn, scale, ustart = view("mn", torch.float32), view("scale", torch.float32), view("ustart", torch.int32)
        if compact:
            idx = room[:4 * K].view(torch.int32)
            vals = view("vals", vdt) if f32 else room[4 * K:]
            plan.unpack(view("packed", torch.uint32), ustart, out=(idx, vals))
            return Encoded(idx, vals, mn, scale, ustart)
        return Encoded(view("idx", torch.int32), view("vals", vdt), mn, scale, ustart)

    def stream_for(self, device):
        """A compact (wire v3) update whose entry stream a reader on `device` can have without packing anything: the
        one the encode packed there, or the blob's own section."""
        if wire.format_of(self.header).stream != "entries" or wire.is_dense(self.header):
            return False
        pk = self._packed[0]
        return self._blob[0] is not None or (pk is not None and pk.device == torch.device(device)
                                             and self.encoded.mn.device == pk.device)

    def _blob_stream(self):
        """The blob's packed section as a uint32 tensor (a copy: the blob's bytes are read-only)."""
        o, n = wire.sections(self._blob[0], self.header)[1]["packed"]
        return torch.from_numpy(np.frombuffer(self._blob[0], dtype="<u4", count=n // 4, offset=o).copy())

    def _staged_sections(self, device, staging, room=0):
        """ONE host-to-device copy of the blob's array sections (they lie back to back: wire.sections) through the pinned
        buffer staging(nbytes) into one allocation on `device`, with `room` more bytes behind them (16-byte aligned) ->
        (view(name, torch dtype): that section there, or None where the format has none; the room)."""
        blob = self._blob[0]
        sec = wire.sections(blob, self.header)[1]
        lo, (o, n) = sec["mn"][0], sec[next(reversed(sec))]
        size = o + n - lo
        stage = staging(size)
        stage[:size].numpy()[:] = np.frombuffer(blob, dtype=np.uint8, count=size, offset=lo)
        behind = (size + 15) // 16 * 16
        dev = torch.empty(behind + room, dtype=torch.uint8, device=device)
        dev[:size].copy_(stage[:size], non_blocking=True)

        def view(name, dt):
            o, n = sec.get(name, (None, 0))
            return None if o is None else dev[o - lo:o - lo + n].view(dt)
        return view, dev[behind:]

    @classmethod
    def from_bytes(cls, blob):
        h, mn, scale, idx, vals, rawb, ustart = wire.unpack(blob)
        validate(h, idx, ustart)
        raw = RawState.from_entries([e for e in h["entries"] if e["kind"] == "raw"], rawb)
        enc = Encoded(torch.from_numpy(idx.copy()), torch.from_numpy(vals.copy()),
                      torch.from_numpy(mn.copy()), torch.from_numpy(scale.copy()),
                      None if ustart is None else torch.from_numpy(ustart.copy()))
        return cls(h, enc, raw, blob=bytes(blob))

    def __getstate__(self):
        return {"blob": self.to_bytes()}

    def __setstate__(self, state):
        other = CompressedUpdate.from_bytes(state["blob"])
        self.__dict__.update(other.__dict__)

    @property
    def compression_ratio(self):
        """Dense fp32 (+ raw) bytes of the update / its payload bytes."""
        return (4 * _dense_elements(self.header["entries"]) + _raw_nbytes(self.raw)) / max(1, self.nbytes)

    def __repr__(self):
        h = self.header
        return (f"CompressedUpdate(mode={h['mode']}, ratio={h['ratio']}, bits={h['bits']}, "
                f"segments={h['n_segments']}, kept={h['total_k']}, bytes={self.nbytes})")


def _all_kept(plan):
    """Every segment of the plan keeps all its elements (the library's dense codec: nothing to pack)."""
    dense = getattr(plan, "dense", None)
    if dense is None:
        segs = plan.table.segs
        dense = bool(len(segs)) and bool((segs[:, 1] == segs[:, 2]).all())
    return dense


def _delta_base(mode, entries, base, device, missing):
    """A delta-mode update's base on `device` — the flat fp32 buffer of the global-model snapshot `base`, which
    must be there (else ValueError(missing)) and of the update's layout — or None in "weights" mode."""
    if mode != "delta":
        return None
    if base is None:
        raise ValueError(missing)
    _check_same_layout(entries, base.entries)
    # the snapshot may have been taken where the global model arrived (the reference client's
    # set_model runs before pretrain moves the model to its device, client/base.py:138 vs :245)
    return base.flat_on(device)


def _copy_raw_groups(raw, into, non_blocking=False):
    """An update's passthrough groups copied into a recycled skeleton's raw buffers."""
    for dst, (src, _) in zip(into.raws, raw._groups):
        dst.copy_(src, non_blocking=non_blocking)


class UpdateCodec:
    """Encode / decode model updates with CodecSpec v1.

    Args:
        ratio: top-k ratio per tensor, (0, 1].
        bits:  1..8 -> uint8 min/max codes; 32 -> raw fp32 values (lossless at ratio 1).
        mode:  "delta" encodes w_local - w_global (decode adds w_global back, fused in the kernel);
               "weights" encodes the weights themselves.
        backend: object with make_plan(sizes, ratio, bits, device); default HipBackend.
        recycle: decode_module / aggregate decode into a module this codec returned earlier once nothing
               outside the codec references it (_TreeRecipe.idle_skeleton); False builds a new module
               every call. release_pool() drops every pooled module.
        compact: sparse uploads travel in the compact payload format (wire v3): every kept entry as one
               (12 + bits)-bit field instead of an int32 index and a whole uint8 code — 2.5 bytes per entry at 8 bits,
               2 at 4 bits, instead of 5. Lossless (the decoded result is bit-identical) and self-describing (a decoder
               needs no switch). A dense plan or ratio 1 keeps the dense format. Off by default.
        pack_dense: ratio-1 (dense) updates with bits below 8 travel with their codes bit-packed (wire v4, DESIGN.md
               §13): `bits` bits per element instead of a whole byte — the download direction's payload, or a
               pure-quantisation upload. Lossless and self-describing, as compact is. At bits 8 or 32, or below ratio
               1, the payload is what it is without the option. Off by default.
        blockwise: ratio-1 (dense) updates with bits 1..8 are quantised block-wise (wire v5): one
               min / scale pair per 4096-element block instead of one per tensor, so a single large weight no longer
               sets the step of its whole tensor; the codes always travel bit-packed, and the encode is one pass over
               the update. Applies where pack_dense applies (and wins over it when both are set); below ratio 1 or at
               bits 32 it is ignored. With error feedback (residual=) the encode is the fused one-pass form of
               DESIGN.md §19 (plan.encode_block_ef; a backend without it: ValueError). Off by default.
        block_size: the block size of blockwise: 4096 (the default), 1024 or 256 elements. A smaller
               block isolates an outlier better — about 0.6x / 0.4x the RMS error of 4096 on heavy-tailed updates at 1024
               / 256 — for 8 more bytes per block (+6 % of the payload at 4 bits and 256). The header names the size, so
               a decoder and aggregate(..., dense_kernel=True) have no switch. Below 4096 the encode rounds to nearest
               only: stochastic=True, a residual=, or a backend whose plan lacks encode_block_g is a ValueError.
        stochastic: ratio-1 (dense) updates with bits 1..8 — per-tensor or block-wise — are quantised with stochastic
               (unbiased) rounding: a code is floor(t) or floor(t) + 1 with probability equal to the
               fraction, so the decoded value is an unbiased estimate and the error of an average of C such updates
               falls as 1 / sqrt(C) instead of staying at the round-to-nearest bias. The payload formats do not change
               (rounding mode is not on the wire). Only the dense family has it: a ratio below 1, bits 32, a residual=
               or a backend without the stochastic encodes is a ValueError, not silently ignored. Off by default.
        seed:  the 64-bit seed of the stochastic rounding; the n-th stochastic encode of this codec uses
               spec.sr_call_seed(seed, n). None draws it from os.urandom once per codec.
        rotate: block-wise updates (blockwise=True, ratio 1, bits 1..8, block size 4096) are rotated before they are
               quantised (wire v6): every full 4096-element block is multiplied by a pseudo-random sign
               diagonal and the orthonormal Walsh-Hadamard transform, its coefficients quantised, and the decoder
               applies the inverse. The coefficients of a heavy-tailed block are close to Gaussian, so one outlier no
               longer sets the step: about 0.27x the RMS error on Student-t(3) data at 1..4 bits, at the same payload
               size; on Gaussian data it is neutral (1.01x), and a block whose error is one huge value among small ones
               is worse at 1 / 2 bits (§22 has the table). Works with stochastic=True. Without blockwise, below ratio 1,
               at bits 32 or with another block size it is a ValueError here; with a residual=, or on a backend whose
               plan lacks encode_block_rot, a ValueError at encode. The header carries the seed: a decoder has no switch.
               Off by default.
        rotate_seed: the 64-bit seed of the rotation; the n-th rotated encode of this codec uses
               spec.sr_call_seed(rotate_seed ^ ROTATE_DOMAIN, n), so successive rounds and different clients rotate
               differently, and the call's rotation seed differs from its stochastic-rounding seed also where
               rotate_seed == seed. None draws it from os.urandom once per codec.
    """

    # the domain separation of the rotation's call seeds from the stochastic rounding's (both are sr_call_seed over
    # the same counter): the first 64 fractional bits of sqrt(2)
    ROTATE_DOMAIN = 0x6A09E667F3BCC908

    def __init__(self, ratio=0.01, bits=8, mode="delta", backend=None, recycle=True, compact=False, pack_dense=False,
                 blockwise=False, stochastic=False, seed=None, block_size=UNIT, rotate=False, rotate_seed=None):
        if not (0.0 < float(ratio) <= 1.0):
            raise ValueError(f"ratio must be in (0, 1], got {ratio}")
        if bits not in VALID_BITS:
            raise ValueError(f"bits must be one of {VALID_BITS}, got {bits}")
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode}")
        self.ratio, self.bits, self.mode = float(ratio), int(bits), mode
        self.recycle = bool(recycle)
        self.compact = bool(compact)
        self.pack_dense = bool(pack_dense)
        self.blockwise = bool(blockwise)
        self.stochastic = bool(stochastic)
        self.block_size = wire.check_block_size(block_size)
        if self.block_size != UNIT and self.stochastic:
            raise ValueError(f"block_size {self.block_size} rounds to nearest only: stochastic rounding is defined for "
                             f"{UNIT}-element blocks (DESIGN.md §20)")
        if self.stochastic:
            if self.ratio < 1.0:
                raise ValueError(f"stochastic rounding covers the dense quantisers only (ratio 1), got ratio {ratio}: "
                                 "the sparse top-k emit rounds to nearest")
            if self.bits == RAW_BITS:
                raise ValueError("stochastic rounding needs bits 1..8: bits 32 carries the fp32 values, nothing is rounded")
        self.seed = (int.from_bytes(os.urandom(8), "little") if seed is None else int(seed)) & ((1 << 64) - 1)
        self._sr_calls = 0  # stochastic encodes so far (under _lock: a server encodes from several threads)
        self.rotate = bool(rotate)
        if self.rotate:
            if not self.blockwise:
                raise ValueError("rotate=True needs blockwise=True: the rotation is defined for block-wise payloads")
            if self.ratio < 1.0:
                raise ValueError(f"rotate=True covers block-wise dense updates only (ratio 1), got ratio {ratio}")
            if self.bits == RAW_BITS:
                raise ValueError("rotate=True needs bits 1..8: bits 32 carries the fp32 values, nothing is quantised")
            if self.block_size != UNIT:
                raise ValueError(f"rotate=True is defined for {UNIT}-element blocks, not block_size {self.block_size} "
                                 "(DESIGN.md §22)")
        self.rotate_seed = (int.from_bytes(os.urandom(8), "little") if rotate_seed is None
                            else int(rotate_seed)) & ((1 << 64) - 1)
        self._rot_calls = 0  # rotated encodes so far (under _lock)
        self.backend = backend if backend is not None else HipBackend()
        self._plans = {}
        self._plan_fast = IdentityCache(32)  # (sizes object; ratio, bits, clients, device) -> plan
        self._checked_ptrs = {}  # id(plan) -> the segment pointers of the last in-place encode that passed the checks
        self._ws = OrderedDict()
        self._lock = threading.Lock()
        self._tls = threading.local()

    def plan_for(self, sizes, device, ratio=None, bits=None, clients=1):
        # (per sizes OBJECT — a layout's cached tuple — no hash of a 161-entry tuple per hook call)
        return self._plan_fast.get((sizes,), (ratio, bits, clients, device),
                                   self._plan_for, sizes, device, ratio, bits, clients)

    def _plan_for(self, sizes, device, ratio, bits, clients):
        ratio = self.ratio if ratio is None else float(ratio)
        bits = self.bits if bits is None else int(bits)
        key = (tuple(sizes), ratio, bits, str(device), int(clients))
        with self._lock:
            p = self._plans.get(key)
            if p is None:
                p = self.backend.make_plan(list(sizes), ratio, bits, device, clients=clients)
                self._plans[key] = p
        return p

    def _next_sr_seed(self):
        """The seed of this codec's next stochastic encode: sr_call_seed(seed, n), n counted under the lock."""
        with self._lock:
            n = self._sr_calls
            self._sr_calls = n + 1
        return sr_call_seed(self.seed, n)

    def _next_rot_seed(self):
        """The rotation seed of this codec's next rotated encode: sr_call_seed(rotate_seed ^ ROTATE_DOMAIN, n). With
        stochastic rounding every encode draws both seeds, so the two counters agree, and the two call seeds differ
        also where rotate_seed == seed (sr_call_seed is a bijection of seed + (n + 1) * its constant)."""
        with self._lock:
            n = self._rot_calls
            self._rot_calls = n + 1
        return sr_call_seed(self.rotate_seed ^ self.ROTATE_DOMAIN, n)

    @staticmethod
    def release_pool():
        """Drop every pooled decoded module (of every template): their storage is freed once their holders
        drop them too. For a server that ends training or changes its model; the pool also evicts trees
        unused for a while (_TreeRecipe.idle_skeleton) and is bounded by the device's memory."""
        release_decode_pool()

    # -- encode -----------------------------------------------------------------------------------
    def encode(self, state, base=None, device=None, residual=None):
        """state_dict -> CompressedUpdate. `base` (delta mode): FlatState of w_global (same layout).
        `device`: where to flatten and encode (default: where the state lives if the backend runs there,
        else the backend's default device — a model trained on the CPU is encoded on the GPU).
        `residual` (delta mode only): this client's error-feedback memory (new_residual), updated in place:
        the update encoded is (state - base) + residual, and what the payload does not carry of it stays in
        the residual for the next round. The payload is an ordinary delta-mode one."""
        if device is None:
            device = self._device_for(state.values())
        L, segs, raw = _describe(state)
        return self._encode(L, segs, raw, base, device, lambda: state, residual=residual)

    def new_residual(self, module_or_state, device=None):
        """A zeroed error-feedback memory for a model of this layout: fp32[span] (the flat layout of its fp32
        entries, 4 bytes per parameter) on the encode device."""
        if isinstance(module_or_state, nn.Module):
            names, tensors, walk = _module_walk(module_or_state)
            L = _layout_walk(names, tensors, walk)[0].L
        else:
            tensors = list(module_or_state.values())
            L = _layout(module_or_state)
        if device is None:
            device = self._device_for(tensors)
        if not L.sizes:
            return torch.zeros(0, dtype=torch.float32, device=device)
        device = torch.device(device)
        return torch.zeros(int(self.plan_for(L.sizes_key, device).table.span), dtype=torch.float32, device=device)

    def encode_module(self, module, base=None, device=None, residual=None):
        """module -> CompressedUpdate of its state_dict (what CompressionClientMixin.compression() runs): the
        same result as encode(module.state_dict(), ...), with the state read through a cached walk of the
        module tree (module_tensors) instead of building the state_dict. residual: as encode()."""
        names, tensors, walk = _module_walk(module)
        if device is None:
            device = self._device_for(tensors)
        d, segs = _layout_walk(names, tensors, walk)
        gather = getattr(self.backend, "gather_scalars", None)
        # the passthrough snapshot is taken after the encode's launches (stream order: the same values), so
        # the GPU starts on the segments one gather launch earlier
        return self._encode(d.L, segs, lambda: _raw_snapshot(d, tensors, gather), base, device,
                            lambda: OrderedDict(zip(names, tensors)), d.seg_ptrs, residual=residual)

    def _encode(self, L, segs, raw, base, device, state_fn, ptrs=None, residual=None):
        """raw: the RawState, or a function that takes it (called once the encode is enqueued)."""
        if residual is not None and self.mode != "delta":
            raise ValueError(f"error feedback (residual=) needs mode 'delta', not {self.mode!r}: the memory holds "
                             "what earlier updates dropped, which only adds to an update, never to the weights")
        need_base = "delta mode needs the global-model snapshot (base)"
        if self.mode == "delta" and base is None:  # (also of a state without fp32 entries, which returns below)
            raise ValueError(need_base)
        entries, sizes = L.entries, L.sizes
        header = {"ratio": self.ratio, "bits": self.bits, "mode": self.mode, "n_segments": len(sizes),
                  "entries": entries}
        if not sizes:
            header["total_k"] = 0
            raw = raw() if callable(raw) else raw
            z = torch.zeros(0)
            return CompressedUpdate(header, Encoded(z.int(), z.to(torch.uint8), z, z), raw)
        device = torch.device(device)
        base_flat = _delta_base(self.mode, entries, base, device, need_base)
        plan = self.plan_for(L.sizes_key, device)
        blockwise = self.blockwise and self.ratio >= 1.0 and self.bits != RAW_BITS and _all_kept(plan)
        if blockwise:
            if residual is not None and (getattr(plan, "encode_block_ef", None) is None
                                         or not getattr(plan, "has_block_ef", True)):
                raise ValueError(f"the {getattr(self.backend, 'name', type(self.backend).__name__)!r} backend's plan "
                                 "has no encode_block_ef: block-wise quantisation cannot be combined with error "
                                 "feedback (residual=) on it")
            if getattr(plan, "encode_block", None) is None:
                raise RuntimeError(f"the {getattr(self.backend, 'name', type(self.backend).__name__)!r} backend's plan "
                                   "has no encode_block: block-wise quantisation is not available on it")
            if self.block_size != UNIT:
                if residual is not None:
                    raise ValueError(f"block_size {self.block_size} cannot be combined with error feedback (residual=): "
                                     f"the one-pass error feedback is defined for {UNIT}-element blocks (DESIGN.md §20)")
                _block_methods(self.backend, plan, self.block_size, "block-wise quantisation")
        rotate = self.rotate and blockwise
        if self.rotate:
            if residual is not None:
                raise ValueError("rotate=True cannot be combined with error feedback (residual=): the one-pass error "
                                 "feedback is defined for unrotated blocks (DESIGN.md §22)")
            if not blockwise or getattr(plan, "encode_block_rot", None) is None \
                    or not getattr(plan, "has_block_rot", True):
                raise ValueError(f"the {getattr(self.backend, 'name', type(self.backend).__name__)!r} backend's plan "
                                 "has no encode_block_rot: the rotation is not available on it")
        sr_seed = None
        if self.stochastic:
            if residual is not None:
                raise ValueError("stochastic rounding cannot be combined with error feedback (residual=): the residual "
                                 "already returns the quantisation error to the client")
            need = "encode_block_sr" if blockwise else "encode_sr"
            if getattr(plan, need, None) is None or not _all_kept(plan):
                raise ValueError(f"the {getattr(self.backend, 'name', type(self.backend).__name__)!r} backend's plan "
                                 f"has no {need}: stochastic rounding is not available on it")
            sr_seed = self._next_sr_seed()
        if residual is not None:
            # (a block-wise plan's error feedback is its own one-pass encode, checked above)
            if not blockwise and (getattr(plan, "ef_accumulate", None) is None
                                  or getattr(plan, "ef_commit", None) is None):
                raise RuntimeError(f"the {getattr(self.backend, 'name', type(self.backend).__name__)!r} backend's plan "
                                   "has no ef_accumulate / ef_commit: error feedback is not available on it")
            if residual.dtype != torch.float32 or residual.device != device or residual.dim() != 1 or \
                    residual.numel() != int(plan.table.span):
                raise ValueError(f"residual: need float32[{int(plan.table.span)}] on {device} (new_residual), got "
                                 f"{residual.dtype}{list(residual.shape)} on {residual.device}")
        cur = torch.cuda.current_stream(device) if device.type == "cuda" else None  # (looked up once per call)
        ws = None if blockwise else self._workspace(plan, cur)
        dev_index = device.index if device.type == "cuda" else -1  # (Tensor.get_device(): -1 on the CPU)
        in_place = getattr(plan, "encode_segments", None) is not None
        if in_place:  # every segment on the plan's device, contiguous, 16-B aligned (one pass per property)
            if ptrs is None:
                ptrs = tuple(map(_data_ptr, segs))
            # (the same storage as an encode that passed the checks: a model's parameters do not move between
            # rounds; contiguity is re-read every call — a parameter re-strided in place keeps its start,
            # `p.data = p.data.t()`, and would otherwise be read in storage order)
            last = self._checked_ptrs.get(id(plan))
            if (last is ptrs or last == ptrs) and not all(map(_is_contig, segs)):
                self._checked_ptrs.pop(id(plan), None)
                last = None
            if last is not ptrs and last != ptrs:
                in_place = (all(map(_is_contig, segs)) and list(map(_get_device, segs)) == [dev_index] * len(segs)
                            and not any(p & 15 for p in ptrs))
                if in_place:
                    self._checked_ptrs[id(plan)] = ptrs
        if blockwise:
            # wire v5: one pass — ranges per block, the bit-packed stream written directly (no workspace, no codes)
            # (with a residual: the fused error feedback of DESIGN.md §19, still one launch and the same carrier)
            block, how = (plan.encode_block, {}) if sr_seed is None else (plan.encode_block_sr, {"seed": sr_seed})
            if residual is not None:
                block, how = plan.encode_block_ef, {"residual": residual}
            if self.block_size != UNIT:
                block, how = plan.encode_block_g, {"block": self.block_size}
            if rotate:  # wire v6: the same triple, the full blocks' codes those of their coefficients
                rot_seed = self._next_rot_seed()
                block, how = plan.encode_block_rot, {"rot_seed": rot_seed, "seed": sr_seed}
                header["rotate"] = rot_seed
            if in_place:
                bmn, bscale, packed = block(tensors=segs, base=base_flat, stream=cur, checked=True, ptrs=ptrs, **how)
            else:
                bmn, bscale, packed = block(flat=flatten_state(state_fn(), device=device).flat, base=base_flat,
                                            stream=cur, **how)
            header.update(total_k=int(plan.table.total_k), blockwise=self.block_size,
                          n_blocks=int(plan.table.n_units) if self.block_size == UNIT
                          else wire.block_count(sizes, self.block_size))
            enc = Encoded(torch.empty(0, dtype=torch.int32, device=bmn.device), None, bmn, bscale, None, packed)
            return CompressedUpdate(header, enc, raw() if callable(raw) else raw, packed=packed)
        if residual is not None:
            # error feedback, in stream order: residual = (state - base) + residual; the plain encode of that; then
            # residual -= what the payload reconstructs, at its kept entries
            if in_place:
                plan.ef_accumulate(residual, tensors=segs, base=base_flat, stream=cur, checked=True, ptrs=ptrs)
            else:
                plan.ef_accumulate(residual, flat=flatten_state(state_fn(), device=device).flat, base=base_flat)
            enc = plan.encode(residual, base=None, workspace=ws)
            plan.ef_commit(enc, residual)
        elif sr_seed is not None:  # the dense encode with stochastic rounding, from the same two sources
            if in_place:
                enc = plan.encode_sr(tensors=segs, base=base_flat, seed=sr_seed, workspace=ws, stream=cur, checked=True,
                                     ptrs=ptrs)
            else:
                enc = plan.encode_sr(flat=flatten_state(state_fn(), device=device).flat, base=base_flat, seed=sr_seed,
                                     workspace=ws, stream=cur)
        elif in_place:  # read the parameters where they live: no flattening copy (+8 B/element of traffic)
            # (dtype and sizes hold by construction: the plan was made from this layout's segments)
            enc = plan.encode_segments(segs, base=base_flat, workspace=ws, checked=True, ptrs=ptrs, launch=cur)
        else:
            fs = flatten_state(state_fn(), device=device)
            enc = plan.encode(fs.flat, base=base_flat, workspace=ws)
        header["total_k"] = int(plan.table.total_k)
        if enc.ustart is not None and self.ratio < 1.0:  # wire v2 (a dense download implies its starts)
            header["n_units"] = int(plan.table.n_units)
        packed = None
        if self.compact and "n_units" in header and not _all_kept(plan):
            # wire v3: the entries repacked on the encode's stream, directly after it (a plan without pack — the test
            # backends — or buffers on the CPU: the carrier packs on the host when it is pickled)
            header["compact"] = True
            pack = getattr(plan, "pack", None)
            if pack is not None and enc.idx.device.type == "cuda":
                packed = pack(enc, stream=cur)
        elif self.pack_dense and self.ratio >= 1.0 and self.bits < 8 and _all_kept(plan):
            # wire v4: the dense codes bit-packed on the encode's stream, directly after it (and after the error
            # feedback's commit, which reads the uint8 codes); a plan without pack_dense packs on the host, as above
            header["dense_packed"] = True
            pack = getattr(plan, "pack_dense", None)
            if pack is not None and enc.vals.device.type == "cuda":
                packed = pack(enc, stream=cur)
        return CompressedUpdate(header, enc, raw() if callable(raw) else raw, packed=packed)

    def _thread_stream(self, device):
        """One HIP stream per (thread, device): concurrent decodes from several threads overlap on the GPU
        instead of queueing on one stream."""
        streams = getattr(self._tls, "streams", None)
        if streams is None:
            streams = self._tls.streams = {}
        key = str(device)
        s = streams.get(key)
        if s is None:
            s = streams[key] = torch.cuda.Stream(device)
        return s

    def _staging(self, nbytes):
        """This thread's pinned host staging buffer of at least nbytes (grown by doubling). Reused only once
        the copy out of it that the previous decode enqueued has completed (its event, _staged)."""
        ev = getattr(self._tls, "staging_event", None)
        if ev is not None:
            ev.synchronize()
            self._tls.staging_event = None
        buf = getattr(self._tls, "staging", None)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 2 * (buf.numel() if buf is not None else 0), 1 << 20),
                              dtype=torch.uint8, pin_memory=True)
            self._tls.staging = buf
        self._tls.staging_used = True
        return buf

    def _staged(self, stream):
        """After encoded_to: if it staged through this thread's pinned buffer, mark the copy's completion."""
        if getattr(self._tls, "staging_used", False):
            self._tls.staging_used = False
            ev = torch.cuda.Event()
            ev.record(stream)
            self._tls.staging_event = ev

    WS_CACHE = 16  # encode workspaces kept per codec (one per plan and launch stream in use)

    def _workspace(self, plan, stream=None):
        """The encode workspace of `plan` for this thread and `stream` (default: the current one), reused across
        calls (kernels on one stream run in order, so consecutive encodes of one thread can share it). Keyed by thread
        too: two threads encoding on one stream (e.g. both on the default stream) interleave their launches, since
        the ctypes call releases the GIL, and one encode's select would read the other's scan results. A bounded
        LRU: an evicted workspace was allocated on its stream, whose later allocations are the only ones that can
        reuse it (stream-ordered)."""
        if not hasattr(plan, "empty_workspace"):
            return None
        if stream is None:
            stream = torch.cuda.current_stream(plan.device) if plan.device.type == "cuda" else None
        key = (id(plan), threading.get_ident(), None if stream is None else stream.cuda_stream)
        with self._lock:
            hit = self._ws.get(key)
            if hit is not None and hit[0] is plan:
                self._ws.move_to_end(key)
                return hit[1]
            ws = plan.empty_workspace()
            self._ws[key] = (plan, ws)
            self._ws.move_to_end(key)
            while len(self._ws) > self.WS_CACHE:
                self._ws.popitem(last=False)
        return ws

    def _device_for(self, tensors):
        for t in tensors:
            if t.dtype == torch.float32 and t.numel() > 0:
                runs = getattr(self.backend, "runs_on", None)
                return t.device if runs is None or runs(t.device) else self.backend.default_device()
        return None

    def snapshot(self, module_or_state, device=None):
        """FlatState of a model (the w_global snapshot for delta mode), flattened on `device` (default:
        where the codec will run: the state's own device if the backend runs there, else the backend's
        default device)."""
        state = module_or_state.state_dict() if isinstance(module_or_state, nn.Module) else module_or_state
        return flatten_state(state, device=device if device is not None else self._device_for(state.values()))

    # -- decode -----------------------------------------------------------------------------------
    def decode_state(self, update, base=None, device=None):
        """CompressedUpdate -> OrderedDict state (fp32 entries are views into one fresh flat buffer).

        On a GPU the decode runs on this thread's own stream (the remote server decodes from one thread per
        upload, coala/server/service.py:74), after a pinned H2D of a received payload; the caller's current
        stream waits for it (no host synchronisation), so the returned tensors are ready for any work the
        caller enqueues next."""
        return self._decode(update, base, device)[0]

    def _decode(self, update, base=None, device=None, into=None):
        """decode_state's work: (state, flat buffer, raw group buffers). `into` (a recycled skeleton, see
        decode_module): decode into its flat buffer and copy the passthrough entries into its raw buffers
        instead of allocating — state is then None."""
        h = update.header  # self-describing: decode with the blob's own ratio/bits/mode
        D, fmt = _decode_layout(h["entries"]), wire.format_of(h)
        flat = plan = None
        raw = update.raw
        if D.sizes:
            if device is None:
                device = self.backend.default_device()
            base_flat = _delta_base(h["mode"], h["entries"], base, device,
                                    "delta-mode update needs the global model (base) to decode")
            plan = self.plan_for(D.sizes, device, ratio=h["ratio"], bits=h["bits"])
            if device.type == "cuda":
                cur = torch.cuda.current_stream(device)
                side = self._thread_stream(device)
                side.wait_stream(cur)
                if into is not None:  # a recycled tree: after its previous holder's work (_reuse_after)
                    _reuse_after(into, side, cur)
                # (the caller's stream's pool)
                out = into.flat if into is not None else torch.empty(plan.span, dtype=torch.float32, device=device)
                with torch.cuda.stream(side):
                    enc = update.encoded_to(device, staging=self._staging, plan=plan)
                    self._staged(side)
                    flat = _decode_encoded(plan, fmt, enc, base_flat, out, side, block=_block_size(h),
                                           rotate=h.get("rotate"))
                    if into is not None:
                        _copy_raw_groups(raw, into, non_blocking=True)
                cur.wait_stream(side)
            else:
                if into is not None:
                    _reuse_after(into, None, None)
                # (off the GPU only a block-wise update is read from its stream: a dense-packed one decodes from its codes)
                enc = update.encoded_to(device) if fmt.per_block else update.encoded.to(device, non_blocking=True)
                flat = _decode_encoded(plan, fmt, enc, base_flat, None if into is None else into.flat,
                                       block=_block_size(h), rotate=h.get("rotate"))
                if into is not None:
                    _copy_raw_groups(raw, into)
        elif into is not None:
            _copy_raw_groups(raw, into)
        if into is not None:
            return None, flat, into.raws
        vals = [None] * len(D.names)
        if D.sizes:
            for pos, v in zip(D.seg_pos, _segment_views(flat, plan.table, h["entries"])):
                vals[pos] = v
        raws = None
        if D.raw:
            if isinstance(raw, RawState):
                raws, raw = raw.fresh_groups(device)
            else:
                raw = {n: (t.to(device) if device is not None else t).clone() for n, t in raw.items()}
            for pos, name in D.raw:
                vals[pos] = raw[name]
        return OrderedDict(zip(D.names, vals)), flat, raws

    def decode_module(self, update, template, base=None):
        """CompressedUpdate -> new nn.Module shaped like `template` holding the decoded state.

        No parameter data is copied: the new module's parameters/buffers are views into the decode
        output. `template` is never aliased. Decoded modules are RECYCLED: once nothing outside this codec
        references a module it returned — none of its submodules, parameters or buffers (the reference server
        drops a round's uploads when the next round's replace them in client_uploads, coala/server/base.py:
        377-381, 562-571) — a later call of the same layout decodes straight into that module's storage and
        returns it, instead of building a module tree again (the Python of ~130 modules and ~160 Parameters
        for a ResNet-50 was most of a decompression(model) call)."""
        D = _decode_layout(update.header["entries"])
        recipe = _recipe(template)
        device = self.backend.default_device() if D.sizes else None
        # (the root comes back taken under the pool lock: no other thread can be handed this tree)
        sk, root = recipe.idle_skeleton(D, update.raw, device) if self.recycle else (None, None)
        if sk is not None:
            self._decode(update, base, device, into=sk)
            recipe.refresh(sk)
            return root
        box = [None]
        box[0], flat, raws = self._decode(update, base, device)  # (the state lives in `box` only)
        return recipe.build_and_adopt(box, D, flat, raws, update.raw, device, adopt=self.recycle)

    # -- fused server-side aggregation ------------------------------------------------------------
    def dense_aggregate_plan(self, header, device=None):
        """The one-layout plan whose aggregate_dense serves a round of updates with this header (aggregate(...,
        dense_kernel=True)), or None where that route does not apply: ratio below 1, bits 32, no fp32 entries, or a
        backend whose plans do not offer the method."""
        sizes = _decode_layout(header["entries"]).sizes
        if not sizes or header["ratio"] < 1.0 or header["bits"] == RAW_BITS:
            return None
        device = self.backend.default_device() if device is None else torch.device(device)
        plan = self.plan_for(sizes, device, ratio=header["ratio"], bits=header["bits"])
        return plan if getattr(plan, "aggregate_dense", None) is not None else None

    def _aggregate_dense(self, plan, updates, weights, total, base_flat, mode, avg_mask, device, out):
        """aggregate()'s fp32 entries by the dense kernel: every upload on the device in its own encoded_to() form
        (uint8 codes, the packed stream, or a block-wise mn ... packed region; a received one through the pinned
        staging buffer), then ONE launch over the uploads' own buffers, on the current stream."""
        cuda = device.type == "cuda"
        cur = torch.cuda.current_stream(device) if cuda else None
        encs = []
        for u in updates:
            encs.append(u.encoded_to(device, staging=self._staging if cuda else None, plan=plan))
            if cuda:
                self._staged(cur)
        kind = _dense_kind(updates[0].header, encs[0])
        if any(_dense_kind(u.header, e) != kind for u, e in zip(updates[1:], encs[1:])):
            raise ValueError("dense aggregation needs every upload in the same form on the device")
        codes = [e.vals if kind == "codes" else e.packed for e in encs]
        block = _block_size(updates[0].header)
        if kind == "block" and block != UNIT:  # (one block size per round: _uniform)
            _block_methods(self.backend, plan, block, "the dense aggregate")
            return plan.aggregate_dense_g(block, codes, [e.mn for e in encs], [e.scale for e in encs], weights,
                                          total=total, base=base_flat, out=out, mode=mode, avg_mask=avg_mask)
        return plan.aggregate_dense(codes, [e.mn for e in encs], [e.scale for e in encs], weights, total=total,
                                    base=base_flat, out=out, mode=mode, avg_mask=avg_mask, kind=kind)

    def sparse_uploads_plan(self, updates, device=None):
        """The one-layout plan whose aggregate_uploads serves this round (aggregate(..., sparse_uploads=True)), or None
        where that route does not apply: no fp32 entries, uploads without per-unit starts (wire v1), a dense, dense-
        packed or block-wise round, a plan whose every segment keeps everything, or a backend whose plans do not
        offer the method. (Mixed formats are not a uniform round: aggregate() rejects them either way.)"""
        h0 = updates[0].header
        fmt = wire.format_of(h0)
        sizes = _decode_layout(h0["entries"]).sizes
        if not sizes or wire.is_dense(h0) or fmt.stream == "dense" or not _uniform(updates) or \
                any(u.encoded.ustart is None for u in updates):
            return None
        device = self.backend.default_device() if device is None else torch.device(device)
        plan = self.plan_for(sizes, device, ratio=h0["ratio"], bits=h0["bits"])
        return plan if getattr(plan, "aggregate_uploads", None) is not None and not _all_kept(plan) else None

    def _aggregate_uploads(self, plan, updates, weights, total, base_flat, mode, avg_mask, device, out):
        """aggregate()'s fp32 entries from the uploads' own buffers: every upload on the device in its encoded_to() form
        (a received blob: ONE pinned copy of its mn ... ustart region, a compact one staying compact; a local carrier
        where it is), then ONE launch, on the current stream."""
        cuda = device.type == "cuda"
        cur = torch.cuda.current_stream(device) if cuda else None
        # a compact round is read from the streams where every upload has its stream for `device` (stream_for: a
        # received blob brings it, a local carrier holds the one its encode packed there), else from unpacked entries
        compact = all(u.stream_for(device) for u in updates)
        encs = []
        for u in updates:
            encs.append(u.encoded_to(device, staging=self._staging if cuda else None, plan=plan, keep_packed=compact))
            if cuda:
                self._staged(cur)
        col = lambda f: [getattr(e, f) for e in encs]  # noqa: E731
        return plan.aggregate_uploads(col("idx"), col("packed"), col("vals"), col("mn"), col("scale"), col("ustart"),
                                      weights, total=total, base=base_flat, out=out, mode=mode, avg_mask=avg_mask,
                                      kind="compact" if compact else "entries")

    def aggregate(self, updates, weights, template, base=None, mode="recip", device=None, params_only=False,
                  dense_kernel=False, sparse_uploads=False):
        """Fused decode + FedAvg of several CompressedUpdates of one layout -> nn.Module (recycled from the
        decode pool once idle, as decode_module's are: a dropped earlier result is aggregated into).

        Equivalent to decode_module() of every update followed by the reference's
        strategies.federated_averaging(models, weights) (coala/server/strategies.py:6-29, 57-90), with
        the fp32 entries decoded and averaged in ONE kernel (coalac_aggregate) instead of C dense
        modules. mode "recip": torch-on-GPU division semantics (the decoded modules live on the GPU);
        "div": torch-on-CPU; "sum": strategies.weighted_sum (:57-90) — no division, the module a
        multi-GPU server passes to reduce_models (coala/distributed/distributed.py:42-57). Non-fp32
        entries (int64 BatchNorm counters) are combined with the same torch ops as the reference, on the
        output device. Weights follow federated_averaging / weighted_sum: empty or all-zero weights
        become 1 per update. params_only (aggregation_content "parameters", coala/server/base.py:588-591):
        only the template's parameters are averaged (federated_averaging_only_params /
        weighted_sum_only_params, strategies.py:32-54, 93-124); every buffer keeps update 0's decoded value,
        as the reference's deepcopy(models[0]) does.
        dense_kernel: ratio-1 updates with bits 1..8 — plain uint8 codes, bit-packed (wire v4) or
        block-wise (wire v5) — are aggregated by the dense kernel (CodecPlan.aggregate_dense) where the backend's plan
        offers it: every upload is read from its own encoded_to() copy, with no concatenation, no unpacking to a byte
        per element and no implied indices, and block-wise updates are accepted. Everything else (ratio below 1, bits
        32, a backend without the method) takes the route above, as with False.
        sparse_uploads: a round of sparse uploads that carry their per-unit starts — plain (wire v2) or
        compact (wire v3), bits 32 included — is aggregated from the uploads' own buffers (CodecPlan.aggregate_uploads)
        where the backend's plan offers it: one pinned copy per received blob, a compact stream read as it is, no
        concatenation, no unpack launch, no plan per client count. Everything else (wire v1, a dense round, a backend
        without the method) takes the route above, as with False.
        """
        if not updates:
            return None
        weights = list(weights) if weights is not None else []
        if not weights or sum(weights) == 0:
            weights = [1 for _ in updates]
        if len(weights) != len(updates):
            raise ValueError("one weight per update")
        total = sum(weights)
        h0, fmt = updates[0].header, wire.format_of(updates[0].header)
        if not _uniform(updates):
            raise ValueError("fused aggregation needs updates of one layout / ratio / bits / mode / payload format")
        sizes = [e["n"] for e in h0["entries"] if e["kind"] == "seg"]
        device = self.backend.default_device() if device is None else torch.device(device)
        # the one-layout plan whose aggregate_dense reads the uploads, when this round takes that route
        one = self.dense_aggregate_plan(h0, device) if dense_kernel else None
        ups = self.sparse_uploads_plan(updates, device) if sparse_uploads and one is None else None
        if fmt.per_block and one is None:
            raise ValueError("fused aggregation reads per-segment codes: block-wise updates are decoded one by one "
                             "(decode_module), or aggregated by the dense kernel (dense_kernel=True)")
        base_flat = _delta_base(h0["mode"], h0["entries"], base, device,
                                "delta-mode updates need the global model (base) to aggregate")
        state = OrderedDict()
        flat = None
        # the output module is recycled like decode_module's (the same pool: modules this codec returned that
        # nothing outside it references any more); not for params_only, whose buffers are update 0's values
        recipe = D = sk = root = None
        if self.recycle and not params_only and isinstance(updates[0].raw, RawState):
            D = _decode_layout(h0["entries"])
            recipe = _recipe(template)
            sk, root = recipe.idle_skeleton(D, updates[0].raw, device)  # (root taken under the pool lock)
            if sk is not None:
                cur = torch.cuda.current_stream(device) if device.type == "cuda" else None
                _reuse_after(sk, cur, cur)  # the kernel runs on the current stream
        if params_only:
            pnames = {n for n, _ in template.named_parameters(remove_duplicate=False)}
        accs = []
        raw_avg = _aggregate_raw(updates, weights, total, mode, device,
                                 keep=(lambda n: n not in pnames) if params_only else None, accs=accs)
        if raw_avg is None:  # (the passthrough entries are combined one by one below: nothing to recycle into)
            recipe = sk = root = None
        avg_mask = None
        if sizes and params_only:
            avg_mask = [e["name"] in pnames for e in h0["entries"] if e["kind"] == "seg"]
        if one is not None:
            plan = one
            flat = self._aggregate_dense(one, updates, weights, total, base_flat, mode, avg_mask, device,
                                         None if sk is None else sk.flat)
            if sk is not None and flat.data_ptr() != sk.flat.data_ptr():  # a backend that returns its own buffer
                sk = root = None
        elif ups is not None:
            plan = ups
            flat = self._aggregate_uploads(ups, updates, weights, total, base_flat, mode, avg_mask, device,
                                           None if sk is None else sk.flat)
            if sk is not None and flat.data_ptr() != sk.flat.data_ptr():  # a backend that returns its own buffer
                sk = root = None
        elif sizes:
            C = len(updates)
            plan = self.plan_for(sizes, device, ratio=h0["ratio"], bits=h0["bits"], clients=C)
            one = self.plan_for(sizes, device, ratio=h0["ratio"], bits=h0["bits"]) if fmt.stream == "dense" else None
            unpack = getattr(one, "unpack_dense", None)

            def on_device(u):
                e = u.encoded
                if unpack is None or e.vals.device == device:
                    return e.to(device, non_blocking=True)
                # a dense-packed upload whose codes are not on the device: the bit stream is moved instead, and the
                # codes the kernel reads are unpacked there
                return Encoded(e.idx.to(device), unpack(u.packed.to(device, non_blocking=True)),
                               e.mn.to(device, non_blocking=True), e.scale.to(device, non_blocking=True), None)
            encs = [on_device(u) for u in updates]
            batched = Encoded(*(torch.cat([getattr(e, f) for e in encs]) for f in ("idx", "vals", "mn", "scale")),
                              torch.cat([e.ustart for e in encs]) if all(e.ustart is not None for e in encs) else None)
            flat = plan.aggregate(batched, weights, total=total, base=base_flat, mode=mode, avg_mask=avg_mask,
                                  out=None if sk is None else sk.flat)
            if sk is not None and flat.data_ptr() != sk.flat.data_ptr():  # a backend that returns its own buffer
                sk = root = None
        if sk is not None:
            for dst, acc in zip(sk.raws, accs):
                dst.copy_(acc, non_blocking=True)
            recipe.refresh(sk)
            return root
        # the fp32 entries: one split of the output (_segment_views), not a slice + view per entry
        seg_views = iter(_segment_views(flat, plan.table, h0["entries"])) if sizes else None
        for e in h0["entries"]:
            if e["kind"] == "seg":
                state[e["name"]] = next(seg_views)
            elif raw_avg is not None:
                state[e["name"]] = raw_avg[e["name"]]
            elif params_only and e["name"] not in pnames:  # a buffer: update 0's (deepcopy(models[0]))
                state[e["name"]] = updates[0].raw[e["name"]].to(device).clone()
            else:  # restated weighted_sum (+ torch.div) on the raw entries
                acc = updates[0].raw[e["name"]].to(device).clone()
                acc *= weights[0]
                for i in range(1, len(updates)):
                    acc += updates[i].raw[e["name"]].to(device) * weights[i]
                state[e["name"]] = acc if mode == "sum" else torch.div(acc, total).to(acc.dtype)
        if recipe is not None:
            # no view of the output may outlive this frame beside the module's own: the pool's idle
            # fingerprint is taken inside build_and_adopt
            box = [state]
            del state, seg_views, raw_avg
            return recipe.build_and_adopt(box, D, flat, accs, updates[0].raw, device)
        return module_with_state(template, state)


def _dense_kind(header, enc):
    """What CodecPlan.aggregate_dense reads of a ratio-1 upload: its block-wise stream, its bit-packed stream where
    the upload's encoded_to() left one on the device, else its uint8 codes."""
    if wire.format_of(header).per_block:
        return "block"
    return "packed" if enc.packed is not None else "codes"


def _uniform(updates):
    """Updates of one layout, ratio, bits, mode and payload format (block-wise ones: of one block size): what one fused
    aggregation takes. A round that holds a rotated upload (wire v6) is not uniform: no fused kernel
    applies the inverse rotation, so such a round is decoded upload by upload, as a round of mixed formats is."""
    u0 = updates[0]
    if any("rotate" in u.header for u in updates):
        return False
    return all(u.signature == u0.signature and u.header["entries"] == u0.header["entries"]
               and u.header.get("blockwise") == u0.header.get("blockwise") for u in updates[1:])


def _block_size(header):
    """The block size of a block-wise (wire v5) header, else UNIT."""
    return int(header.get("blockwise", UNIT))


def _block_methods(backend, plan, block, who):
    """ValueError unless `plan` serves `block`-element blocks below 4096: the plan's encode_block_g /
    decode_block_g / aggregate_dense_g, on a library that exports their entry points."""
    if getattr(plan, "encode_block_g", None) is None or not getattr(plan, "has_block_g", True):
        raise ValueError(f"the {getattr(backend, 'name', type(backend).__name__)!r} backend's plan has no "
                         f"encode_block_g: {who} needs it for block size {block} (only {UNIT} is available on it)")


def _decode_encoded(plan, fmt, enc, base, out, stream=None, block=UNIT, rotate=None):
    """The plan's decode of an update in the form encoded_to() left it in: a block-wise update from its stream with
    each block's own range (block: its block size, the header's; rotate: a wire v6 header's rotation seed), a
    dense-packed one whose stream is on the device from the stream itself, else from its idx / vals."""
    if rotate is not None:
        if getattr(plan, "decode_block_rot", None) is None or not getattr(plan, "has_block_rot", True):
            raise ValueError("this backend's plan has no decode_block_rot: a rotated (wire v6) update cannot be decoded "
                             "on it")
        return plan.decode_block_rot(enc.packed, enc.mn, enc.scale, rotate, base=base, out=out, stream=stream)
    if fmt.per_block and block != UNIT:
        return plan.decode_block_g(block, enc.packed, enc.mn, enc.scale, base=base, out=out, stream=stream)
    if fmt.per_block:
        return plan.decode_block(enc.packed, enc.mn, enc.scale, base=base, out=out, stream=stream)
    if enc.packed is not None:
        return plan.decode_packed(enc.packed, enc.mn, enc.scale, base=base, out=out, stream=stream)
    return plan.decode(enc, base=base, out=out, stream=stream)


def _aggregate_raw(updates, weights, total, mode, device, keep=None, accs=None):
    """The passthrough entries of several updates combined as the per-entry loop in UpdateCodec.aggregate
    does — acc = x_0 * w_0; acc += x_i * w_i in update order; then torch.div(acc, total) cast back (not in
    mode "sum"); entries for which keep(name) is true take update 0's value — but with the same elementwise
    ops on each dtype group's flat tensor at once (a BatchNorm model's 53 counters: 2 ops per update instead
    of 2 per update and counter). None when the updates' RawStates are not grouped alike. accs (a list):
    receives each dtype group's result buffer, the storage the returned entries view."""
    raws = [u.raw for u in updates]
    if not all(isinstance(r, RawState) for r in raws):
        return None
    g0 = raws[0]._groups
    sig = raws[0].signature()
    if any(r.signature() != sig for r in raws[1:]):
        return None
    out = {}
    int_weights = all(type(w) is int and -(1 << 62) < w < (1 << 62) for w in weights)
    for gi, (f0, members) in enumerate(g0):
        if int_weights and f0.dtype in (torch.int64, torch.int32) and len(raws) > 2:
            # integer entries, integer weights: two's-complement sums do not depend on their order, so the
            # update-order loop is one stacked product and sum (3 launches instead of 2 per update), cast back
            # to the entry dtype (the loop's in-place ops wrap the same way)
            X = torch.stack([r._groups[gi][0].to(device) for r in raws])
            W = torch.tensor(weights, dtype=torch.int64, device=device)
            acc = (X.to(torch.int64) * W[:, None]).sum(0).to(f0.dtype)
        else:
            acc = f0.to(device, copy=True)
            acc *= weights[0]
            for i in range(1, len(raws)):
                acc += raws[i]._groups[gi][0].to(device) * weights[i]
        if mode != "sum":
            acc = torch.div(acc, total).to(acc.dtype)
        if accs is not None:
            accs.append(acc)
        first = f0.to(device, copy=True) if keep is not None else None
        views = raws[0]._make_views([(acc, members)])
        firsts = raws[0]._make_views([(first, members)]) if first is not None else None
        for n, _, _ in members:
            out[n] = firsts[n] if keep is not None and keep(n) else views[n]
    return out
