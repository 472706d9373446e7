"""Self-describing wire format of a compressed update ("COALAQ1").

The blob rides inside the pickled carrier that COALA puts into UploadContent.data
(/root/reference/coala/client/base.py:363 -> protos/coala/pb/server_service.proto:13-24). It must be
self-describing because remote clients never receive new config keys (OperateConfig has fixed fields,
/root/reference/protos/coala/pb/client_service.proto:24-39).

Layout (little-endian):
    0   8B   magic b"COALAQ1\\0"
    8   u32  format version (5 when the header has "blockwise", 4 when it has "dense_packed", 3 when it has "compact",
             2 when it has "n_units" only, else 1)
    12  u32  header length H
    16  H    UTF-8 JSON header: ratio, bits, mode, n_segments, total_k, [n_units], entries[]
             entry = {"name", "dtype", "shape", "kind": "seg", "seg": i, "n", "k", "out_off"}
                   | {"name", "dtype", "shape", "kind": "raw", "off", "nbytes"}
    then, each section starting at a 16-byte boundary:
         mn f32[T] | scale f32[T] | idx i32[K] | vals (u8[K], or f32[K] if bits == 32) | [ustart i32[U]] | raw bytes
    ustart (version 2): per 4096-element unit of every fp32 segment, in segment order, the segment-relative
    index of the unit's first kept entry — what the encoder's k_select computed anyway, so the decoder (and the
    server's fused aggregate) finds each unit's entries without searching the idx lists. U = "n_units".
    A header with "dense": true (ratio 1: every segment keeps all n elements, idx = 0..n-1 per segment)
    carries an empty idx section, and unpack returns an empty idx: the indices stay implied all the way into
    the GPU's dense decode (coalac.hip k_dense_deq), never materialised. This is the download-direction
    default (dense 8-bit weights, ~4x smaller than fp32 instead of 5 B per element with explicit indices).

Version 3, the COMPACT payload (opt-in, sparse uploads only; header key "compact": true, "n_units" mandatory):
         mn f32[T] | scale f32[T] | packed u32[P] | [vals f32[K] only when bits == 32] | ustart i32[U] | raw bytes
    For K = total_k entry positions and code width b (b = bits when bits <= 8; b = 0 when bits == 32, whose fp32
    values stay in their own section), every entry is one field of w = 12 + b bits (12 <= w <= 20):
        field_j = (idx[j] & 0xFFF) | (code_j << 12)          j: the position in the idx / vals arrays
    The packed section is a little-endian bit stream of uint32 words: field j occupies bits [j*w, (j+1)*w), bit t
    of the stream is bit t % 32 of word t // 32. It is P = ceil(K*w / 32) words long and all padding bits are zero,
    so equal payloads give equal bytes. Only the low 12 bits of an index travel: the upper bits are the number of
    its 4096-element unit, which ustart already says. Unit u of segment s, the u_s-th unit of that segment, owns
    the segment-relative entries [ustart[u], ustart[u+1]) (the segment's last unit ends at k_s), clamped to
    [0, k_s] with begin <= end (and to at most the unit's element count: a unit keeps no more entries than it has
    elements), exactly as the decode kernels clamp. For each owned entry e: j = out_off_s + e,
        idx[j] = (u_s << 12) | (field_j & 0xFFF)      vals[j] = field_j >> 12
    pack_entries / unpack_entries below are this format on the host (numpy); the GPU's k_pack / k_unpack
    (coalac.hip) produce and read the same bytes.

Version 4, BIT-PACKED DENSE CODES (opt-in, "dense" updates with bits 1..7 only; header keys "dense": true and
"dense_packed": true, no "n_units"):
         mn f32[T] | scale f32[T] | packed u32[P] | raw bytes
    With code width b = bits, segment s (in header order) owns W_s = ceil(n_s * b / 32) uint32 words at word offset
    pw_s = sum of W_t for t < s; the stream is P = sum of W_s words, and an empty segment owns none. Entry e of segment
    s — the code of its element e — occupies bits [e*b, (e+1)*b) of the segment's sub-stream, a little-endian bit
    stream as in version 3 (bit t is bit t % 32 of word t // 32). The padding bits of a segment's last word are zero,
    so equal payloads give equal bytes; a receiver ignores them. Every segment — and so every 4096-element unit of it,
    unit u_s at word pw_s + 128*b*u_s — starts on a word boundary. Any b-bit field is a legal code (<= 2^b - 1), so an
    untrusted stream can mis-decode but cannot produce an out-of-range code. At bits 8 the stream would be as long as
    the codes and at bits 32 there are none: neither is ever packed, and a header that says so is rejected.
    dense_packed_words / pack_dense_codes / unpack_dense_codes below are this format on the host (numpy); the GPU's
    k_pack_dense / k_unpack_dense / k_dense_deq_packed (coalac.hip) produce and read the same bytes. unpack() of a
    version-4 blob returns the rebuilt uint8 codes, so validate() and every consumer of codes sees what it sees for
    a version-1 / 2 dense blob.

Version 5, BLOCK-WISE DENSE QUANTISATION (opt-in, "dense" updates with bits 1..8; header keys "dense": true,
"blockwise": 4096 and "n_blocks": U):
         mn f32[U] | scale f32[U] | packed u32[P] | raw bytes
    One quantisation range per 4096-element block instead of one per segment. Block index = unit index: segment by
    segment in header order, ceil(n_s / 4096) blocks each, U = their sum; block u, the u_s-th of segment s, covers the
    segment's elements [4096 u_s, min(n_s, 4096 (u_s + 1))). CodecSpec v1 applies to the block as if it were a segment
    of its own with k = n: mn_u / mx_u its NaN-ignoring min / max (+ 0.0f), scale_u = 0 if mx_u == mn_u else
    (mx_u - mn_u) / L, the same quantise, decode mn_u + float(q) * scale_u. The code stream is version 4's, bit for bit
    (also at bits 8, where it is simply the codes): the same W_s, pw_s, field order and zero padding, so a block starts
    at word pw_s + 128*b*u_s. The blob is 8 U + 4 P + raw payload bytes (plus header and alignment). unpack() returns
    mn / scale of length U and the rebuilt uint8 codes. block_count / block_table below are the block order on the host.
"""
import json
import struct
import threading
from collections import OrderedDict

import numpy as np

from .spec import RAW_BITS, UNIT, VALID_BITS, k_for

MAGIC = b"COALAQ1\0"
VERSION = 1     # mn | scale | idx | vals | raw
VERSION_2 = 2   # ... | vals | ustart | raw
VERSION_3 = 3   # mn | scale | packed | [vals f32] | ustart | raw  (header "compact": true)
VERSION_4 = 4   # mn | scale | packed | raw  (header "dense": true, "dense_packed": true)
VERSION_5 = 5   # mn[U] | scale[U] | packed | raw  (header "dense": true, "blockwise": 4096, "n_blocks": U)
INDEX_BITS = 12  # low index bits in a packed field: log2(UNIT), the position inside the entry's 4096-element unit


def _pad16(n):
    return (16 - n % 16) % 16


def packed_words(total_k, bits):
    """uint32 words of the packed entry stream of total_k entries: ceil(total_k * (12 + code bits) / 32)."""
    return (int(total_k) * field_bits(bits) + 31) // 32


def field_bits(bits):
    """Width w of a packed field: 12 index bits + the code (none at bits 32, whose values are not packed)."""
    return INDEX_BITS + (0 if int(bits) == RAW_BITS else int(bits))


def pack_entries(idx, vals, bits):
    """idx int32[K], vals (uint8[K] codes; ignored at bits 32) -> the packed stream, uint32[ceil(K*w/32)]: field j =
    (idx[j] & 0xFFF) | (code_j << 12) at bits [j*w, (j+1)*w) of a little-endian bit stream, padding bits zero."""
    w = field_bits(bits)
    f = np.asarray(idx).astype(np.uint32) & np.uint32(UNIT - 1)
    if w > INDEX_BITS:
        f |= (np.asarray(vals).astype(np.uint32) & np.uint32((1 << (w - INDEX_BITS)) - 1)) << np.uint32(INDEX_BITS)
    K = f.size
    stream = np.zeros(packed_words(K, bits) * 32, dtype=np.uint8)
    stream[:K * w] = ((f[:, None] >> np.arange(w, dtype=np.uint32)) & np.uint32(1)).astype(np.uint8).reshape(-1)
    return np.packbits(stream, bitorder="little").view("<u4")


def unpack_entries(packed, ustart, segs_n, segs_k, bits):
    """The packed stream + per-unit starts -> (idx int32[K], vals uint8[K]) for segments of segs_n elements keeping
    segs_k entries each, laid out back to back (out_off = the running sum of k), K = sum(segs_k). The ranges the
    starts give are clamped as the kernels clamp them, so any starts reconstruct in range; positions no unit owns
    stay 0 (never with a valid payload). At bits 32 vals is all zero (the fp32 values are their own section)."""
    w = field_bits(bits)
    n = np.asarray(segs_n, dtype=np.int64).reshape(-1)
    k = np.asarray(segs_k, dtype=np.int64).reshape(-1)
    if n.size != k.size or np.any(n < 0) or np.any(k < 0) or np.any(k > n):
        raise ValueError("COALAQ1: bad segment sizes for a packed stream")
    K = int(k.sum())
    packed = np.ascontiguousarray(packed, dtype="<u4")
    if packed.size < packed_words(K, bits):
        raise ValueError("COALAQ1: truncated packed section")
    nu = (n + UNIT - 1) // UNIT
    ustart = np.asarray(ustart).astype(np.uint32).astype(np.int64)  # (the kernels read the starts as unsigned)
    if ustart.size != int(nu.sum()):
        raise ValueError("COALAQ1: per-unit start count mismatch")
    # every field: the one or two words that hold it, as one 64-bit value
    bit = np.arange(K, dtype=np.int64) * w
    wd, sh = bit >> 5, (bit & 31).astype(np.uint64)
    words = np.concatenate([packed[:packed_words(K, bits)], np.zeros(1, dtype="<u4")]).astype(np.uint64)
    f = (((words[wd] | (words[wd + 1] << np.uint64(32))) >> sh) & np.uint64((1 << w) - 1)).astype(np.uint32)
    # every unit: its segment, its number inside the segment, its clamped entry range
    seg = np.repeat(np.arange(n.size), nu)
    first_unit = np.cumsum(nu) - nu
    u_s = np.arange(ustart.size, dtype=np.int64) - first_unit[seg]
    ks = k[seg]
    last = u_s == nu[seg] - 1
    ulen = np.minimum(UNIT, n[seg] - u_s * UNIT)
    lo = np.minimum(ustart, ks)
    nxt = np.append(ustart[1:], 0)
    hi = np.maximum(lo, np.minimum(np.minimum(np.where(last, ks, nxt), ks), lo + ulen))
    cnt = hi - lo
    out_off = (np.cumsum(k) - k)[seg]
    owned = int(cnt.sum())
    j = np.repeat(out_off + lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(owned, dtype=np.int64)
    idx = np.zeros(K, dtype=np.int32)
    vals = np.zeros(K, dtype=np.uint8)
    idx[j] = ((np.repeat(u_s, cnt) << INDEX_BITS) | (f[j] & np.uint32(UNIT - 1))).astype(np.int32)
    vals[j] = (f[j] >> np.uint32(INDEX_BITS)).astype(np.uint8)
    return idx, vals


def _segment_words(sizes, bits):
    """(W_s per segment, b) of a dense-packed stream; bits must be a code width."""
    b = int(bits)
    if not 1 <= b <= 8:
        raise ValueError(f"COALAQ1: dense codes are packed at 1..8 bits, not {bits}")
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if np.any(n < 0):
        raise ValueError("COALAQ1: bad segment sizes for a dense-packed stream")
    return (n * b + 31) // 32, b


def dense_packed_words(sizes, bits):
    """uint32 words P of the bit-packed stream of dense segments of `sizes` elements: the sum of ceil(n * bits / 32)."""
    return int(_segment_words(sizes, bits)[0].sum())


def _group_shifts(b):
    """For each of the 32 entries of a group (b whole words): (word, shift, bits that spill into the next word)."""
    return [((i * b) >> 5, (i * b) & 31, max(0, ((i * b) & 31) + b - 32)) for i in range(32)]


def pack_dense_codes(vals, sizes, bits, out_off=None):
    """uint8 codes -> the bit-packed dense stream, uint32[dense_packed_words(sizes, bits)]. Segment s holds sizes[s]
    codes at vals[out_off[s]:] (default: back to back, the running sum of sizes); entry e of it lands at bits
    [e*b, (e+1)*b) of the segment's own words, which start at word pw_s; padding bits are zero."""
    W, b = _segment_words(sizes, bits)
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    off = np.cumsum(n) - n if out_off is None else np.asarray(out_off, dtype=np.int64).reshape(-1)
    vals = np.asarray(vals).reshape(-1)
    out = np.zeros(int(W.sum()), dtype="<u4")
    shifts, mask, pw = _group_shifts(b), np.uint64((1 << b) - 1), 0
    for ns, ws, o in zip(n.tolist(), W.tolist(), off.tolist()):
        if not ns:
            continue
        if o < 0 or o + ns > vals.size:
            raise ValueError("COALAQ1: segment codes past the end of vals")
        G = (ns + 31) // 32  # 32-entry groups = b words each; the last one zero-padded
        c = np.zeros(G * 32, dtype=np.uint64)
        c[:ns] = vals[o:o + ns]
        c = (c & mask).reshape(G, 32)
        words = np.zeros((G, b + 1), dtype=np.uint64)
        for i, (wd, sh, spill) in enumerate(shifts):
            words[:, wd] |= (c[:, i] << np.uint64(sh)) & np.uint64(0xFFFFFFFF)
            if spill:
                words[:, wd + 1] |= c[:, i] >> np.uint64(b - spill)
        out[pw:pw + ws] = words[:, :b].reshape(-1)[:ws].astype("<u4")
        pw += ws
    return out


def unpack_dense_codes(packed, sizes, bits, out_off=None, out=None):
    """The bit-packed dense stream -> uint8 codes (the inverse of pack_dense_codes; padding bits are ignored). out: a
    uint8 array to write into (default: a new one of sum(sizes), or of max(out_off + sizes)); only the segments' own
    positions are written. A stream shorter than dense_packed_words(sizes, bits) is a ValueError."""
    W, b = _segment_words(sizes, bits)
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    off = np.cumsum(n) - n if out_off is None else np.asarray(out_off, dtype=np.int64).reshape(-1)
    packed = np.ascontiguousarray(packed, dtype="<u4").reshape(-1)
    if packed.size < int(W.sum()):
        raise ValueError("COALAQ1: truncated packed section")
    if out is None:
        out = np.zeros(int((off + n).max()) if n.size else 0, dtype=np.uint8)
    shifts, mask, pw = _group_shifts(b), np.uint64((1 << b) - 1), 0
    for ns, ws, o in zip(n.tolist(), W.tolist(), off.tolist()):
        if not ns:
            continue
        G = (ns + 31) // 32
        words = np.zeros(G * b + 1, dtype=np.uint64)  # (+ 1: the word after the last, for a field that would spill)
        words[:ws] = packed[pw:pw + ws]
        lo, hi = words[:G * b].reshape(G, b), words[1:G * b + 1].reshape(G, b)
        c = np.empty((G, 32), dtype=np.uint8)
        for i, (wd, sh, spill) in enumerate(shifts):
            v = lo[:, wd] >> np.uint64(sh)
            if spill:
                v = v | (hi[:, wd] << np.uint64(32 - sh))
            c[:, i] = (v & mask).astype(np.uint8)
        out[o:o + ns] = c.reshape(-1)[:ns]
        pw += ws
    return out


def _seg_sizes(header):
    return [int(e["n"]) for e in header["entries"] if e["kind"] == "seg"]


def block_count(sizes):
    """Blocks U of dense segments of `sizes` elements: the sum of ceil(n / 4096) (an empty segment has none)."""
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    return int(((n + UNIT - 1) // UNIT).sum())


def block_table(sizes):
    """The block-wise format's view of dense segments laid out back to back: one row (offset, length) per block, in
    block order — what a decoder applies mn[u] / scale[u] to. int64[U, 2]."""
    rows, off = [], 0
    for n in (int(x) for x in sizes):
        rows += [(off + a, min(UNIT, n - a)) for a in range(0, n, UNIT)]
        off += n
    return np.asarray(rows, dtype=np.int64).reshape(-1, 2)


def _check_blockwise(header, layout=True):
    """The header rules of a block-wise (version 5) payload; returns (segment sizes, U). layout=False: the format keys
    only (pack() is handed a header that may hold nothing else; the full header travels as header_json)."""
    if not header.get("dense"):
        raise ValueError("COALAQ1: \"blockwise\" needs a \"dense\" payload")
    if isinstance(header["blockwise"], bool) or int(header["blockwise"]) != UNIT:
        raise ValueError(f"COALAQ1: block size {header['blockwise']!r} (only {UNIT} is defined)")
    if header.get("dense_packed") or header.get("compact") or "n_units" in header:
        raise ValueError("COALAQ1: \"blockwise\" excludes \"dense_packed\", \"compact\" and per-unit starts")
    if "bits" in header and not 1 <= int(header["bits"]) <= 8:
        raise ValueError(f"COALAQ1: block-wise codes are 1..8 bits wide, not {header['bits']}")
    if not layout:
        return None, int(header.get("n_blocks", -1))
    if "bits" not in header:
        raise ValueError("COALAQ1: header without bits")
    ns = _seg_sizes(header)
    if sum(ns) != int(header["total_k"]):
        raise ValueError("COALAQ1: dense header with k != n")
    if "n_blocks" not in header or int(header["n_blocks"]) != block_count(ns):
        raise ValueError("COALAQ1: header n_blocks is not the layout's block count")
    return ns, int(header["n_blocks"])


def pack(header, mn, scale, idx, vals, raw, header_json=None, ustart=None, packed=None):
    """numpy arrays + raw bytes -> blob (bytes). A "dense" header drops idx (it is implied). header_json: the
    header's JSON encoding, if the caller has it already. ustart: the per-unit starts (version 2; the header
    must then carry "n_units" = len(ustart)). packed: the packed entry stream (version 3, which needs ustart and a
    header with "compact": true): it stands where idx stood, and vals is the fp32 values at bits 32, else None.
    A header with "dense" and "dense_packed" (version 4): packed is the bit-packed dense stream, the only section
    after mn and scale (idx, vals and ustart are not written). A header with "blockwise" (version 5): mn / scale hold
    one entry per block ("n_blocks" of them) and packed is the same stream."""
    if header.get("blockwise"):
        _, U = _check_blockwise(header, layout=False)
        if packed is None or ustart is not None or len(mn) != U or len(scale) != U:
            raise ValueError("COALAQ1: a block-wise payload needs the packed stream and one mn / scale per block")
        return _pack_stream(VERSION_5, header, header_json, mn, scale, packed, raw)
    if header.get("dense_packed"):
        if not header.get("dense") or packed is None or ustart is not None or "n_units" in header:
            raise ValueError("COALAQ1: a dense-packed payload needs \"dense\", the packed stream and no per-unit starts")
        return _pack_stream(VERSION_4, header, header_json, mn, scale, packed, raw)
    if header.get("dense"):
        idx = np.zeros(0, dtype=np.int32)
    if (ustart is not None) != ("n_units" in header) or (ustart is not None and len(ustart) != header["n_units"]):
        raise ValueError("COALAQ1: ustart section and header n_units disagree")
    if (packed is not None) != bool(header.get("compact")) or (packed is not None and ustart is None):
        raise ValueError("COALAQ1: a compact payload needs the packed stream, the per-unit starts and \"compact\"")
    h = header_json if header_json is not None else encode_header(header)
    ver = VERSION_3 if packed is not None else VERSION if ustart is None else VERSION_2
    parts = [MAGIC, struct.pack("<II", ver, len(h)), h]
    size = 16 + len(h)
    arrays = [np.ascontiguousarray(mn, "<f4"), np.ascontiguousarray(scale, "<f4")]
    if packed is not None:
        arrays.append(np.ascontiguousarray(packed, "<u4"))
        if vals is not None:
            arrays.append(np.ascontiguousarray(vals, "<f4"))
    else:
        arrays += [np.ascontiguousarray(idx, "<i4"), np.ascontiguousarray(vals)]
    if ustart is not None:
        arrays.append(np.ascontiguousarray(ustart, "<i4"))
    for arr in arrays:
        p = _pad16(size)
        parts.append(b"\0" * p)
        b = arr.tobytes()
        parts.append(b)
        size += p + len(b)
    p = _pad16(size)
    parts.append(b"\0" * p)
    parts.append(bytes(raw))
    return b"".join(parts)


def _pack_stream(ver, header, header_json, mn, scale, packed, raw):
    """mn | scale | packed | raw, each 16-byte aligned, behind the header: the layout versions 4 and 5 share."""
    h = header_json if header_json is not None else encode_header(header)
    parts, size = [MAGIC, struct.pack("<II", ver, len(h)), h], 16 + len(h)
    for arr in (np.ascontiguousarray(mn, "<f4"), np.ascontiguousarray(scale, "<f4"), np.ascontiguousarray(packed, "<u4")):
        b = arr.tobytes()
        parts += [b"\0" * _pad16(size), b]
        size += _pad16(size) + len(b)
    parts += [b"\0" * _pad16(size), bytes(raw)]
    return b"".join(parts)


_HEADERS = OrderedDict()  # header JSON bytes -> parsed header (the same layout arrives round after round)
_HEADERS_LOCK = threading.Lock()


def _parse_header(mv, hl):
    """The blob's JSON header, parsed once per distinct header text (LRU of 32): a SHALLOW copy of the
    cached dict is returned — its "entries" list is shared and must never be mutated (nothing does)."""
    key = bytes(mv[16:16 + hl])
    with _HEADERS_LOCK:
        h = _HEADERS.get(key)
        if h is not None:
            _HEADERS.move_to_end(key)
    if h is None:
        h = json.loads(key.decode())
        with _HEADERS_LOCK:
            _HEADERS[key] = h
            while len(_HEADERS) > 32:
                _HEADERS.popitem(last=False)
    return dict(h)


def encode_header(header):
    return json.dumps(header, separators=(",", ":"), sort_keys=True).encode()


def sections(blob, header=None):
    """(header, {name: (byte offset, byte count)}) of the mn / scale / idx / vals (/ ustart) sections in `blob` — a
    compact or dense-packed blob: `packed` where idx (and the uint8 codes) stood — which lie back to back (each
    16-byte aligned): one host-to-device copy moves all of them."""
    mv = memoryview(blob)
    if bytes(mv[:8]) != MAGIC:
        raise ValueError("not a COALAQ1 blob (bad magic)")
    ver, hl = struct.unpack_from("<II", mv, 8)
    if header is None:
        header = _parse_header(mv, hl)
    T, K = int(header["n_segments"]), int(header["total_k"])
    bits = int(header["bits"])
    vsz = 4 if bits == RAW_BITS else 1
    pos = 16 + hl
    out = {}
    if header.get("blockwise"):  # version 5: per-block ranges, then version 4's stream
        U = int(header["n_blocks"])
        names = [("mn", 4 * U), ("scale", 4 * U), ("packed", 4 * dense_packed_words(_seg_sizes(header), bits))]
    elif header.get("dense_packed"):  # version 4: the bit-packed dense stream, nothing else
        names = [("mn", 4 * T), ("scale", 4 * T), ("packed", 4 * dense_packed_words(_seg_sizes(header), bits))]
    elif header.get("compact"):  # version 3: the packed stream where idx stood; the values only as fp32
        names = [("mn", 4 * T), ("scale", 4 * T), ("packed", 4 * packed_words(K, bits))]
        if bits == RAW_BITS:
            names.append(("vals", 4 * K))
    else:
        names = [("mn", 4 * T), ("scale", 4 * T), ("idx", 0 if header.get("dense") else 4 * K), ("vals", vsz * K)]
    if "n_units" in header:
        names.append(("ustart", 4 * int(header["n_units"])))
    for name, n in names:
        pos += _pad16(pos)
        out[name] = (pos, n)
        pos += n
    return header, out


def _unpack_blockwise(mv, pos, header):
    """unpack() of a version-5 blob: mn / scale per block, the uint8 codes rebuilt from the stream."""
    ns, U = _check_blockwise(header)
    bits = int(header["bits"])
    out = []
    for dt, n in ((np.dtype("<f4"), U), (np.dtype("<f4"), U), (np.dtype("<u4"), dense_packed_words(ns, bits))):
        pos += _pad16(pos)
        if pos + n * dt.itemsize > len(mv):
            raise ValueError("COALAQ1: truncated blob")
        out.append(np.frombuffer(mv, dtype=dt, count=n, offset=pos))
        pos += n * dt.itemsize
    pos += _pad16(pos)
    return (header, out[0], out[1], np.zeros(0, dtype="<i4"), unpack_dense_codes(out[2], ns, bits), bytes(mv[pos:]), None)


def unpack(blob):
    """blob -> (header dict, mn, scale, idx, vals, raw bytes, ustart or None). Arrays are read-only views of
    blob; a "dense" blob's idx is empty (implied). A compact (version 3) blob's idx and uint8 vals are rebuilt
    from its packed stream (unpack_entries, with every segment's k = k_for(n, ratio) as validate() expects). A
    block-wise (version 5) blob's mn / scale have one entry per block."""
    mv = memoryview(blob)
    if bytes(mv[:8]) != MAGIC:
        raise ValueError("not a COALAQ1 blob (bad magic)")
    ver, hl = struct.unpack_from("<II", mv, 8)
    if ver not in (VERSION, VERSION_2, VERSION_3, VERSION_4, VERSION_5):
        raise ValueError(f"unsupported COALAQ1 version {ver}")
    header = _parse_header(mv, hl)
    if (ver == VERSION_5) != ("blockwise" in header):
        raise ValueError("COALAQ1: version and header blockwise disagree")
    if ver == VERSION_5:
        return _unpack_blockwise(mv, 16 + hl, header)
    compact = ver == VERSION_3
    if compact != bool(header.get("compact")):
        raise ValueError("COALAQ1: version and header compact disagree")
    if (ver in (VERSION_2, VERSION_3)) != ("n_units" in header):
        raise ValueError("COALAQ1: version and header n_units disagree")
    dense_packed = ver == VERSION_4
    if dense_packed != bool(header.get("dense_packed")):
        raise ValueError("COALAQ1: version and header dense_packed disagree")
    T, K = int(header["n_segments"]), int(header["total_k"])
    bits = int(header["bits"])
    vdt = np.dtype("<f4") if bits == RAW_BITS else np.dtype("u1")
    pos = 16 + hl
    out = []
    dense = bool(header.get("dense"))
    if dense_packed:
        if not dense or not 1 <= bits <= 7 or K < 0:
            raise ValueError("COALAQ1: bad dense_packed header (needs \"dense\" and bits 1..7)")
        ns = _seg_sizes(header)
        if sum(ns) != K:
            raise ValueError("COALAQ1: dense header with k != n")
        layout = [(np.dtype("<f4"), T), (np.dtype("<f4"), T), (np.dtype("<u4"), dense_packed_words(ns, bits))]
    elif compact:
        if dense or bits not in VALID_BITS or K < 0:
            raise ValueError("COALAQ1: bad compact header")
        layout = [(np.dtype("<f4"), T), (np.dtype("<f4"), T), (np.dtype("<u4"), packed_words(K, bits)),
                  (vdt, K if bits == RAW_BITS else 0)]
    else:
        layout = [(np.dtype("<f4"), T), (np.dtype("<f4"), T), (np.dtype("<i4"), 0 if dense else K), (vdt, K)]
    if ver in (VERSION_2, VERSION_3):
        layout.append((np.dtype("<i4"), int(header["n_units"])))
    for dt, n in layout:
        pos += _pad16(pos)
        if n < 0 or pos + n * dt.itemsize > len(mv):
            raise ValueError("COALAQ1: truncated blob")
        out.append(np.frombuffer(mv, dtype=dt, count=n, offset=pos))
        pos += n * dt.itemsize
    pos += _pad16(pos)
    raw = bytes(mv[pos:])
    if dense and K != sum(int(e["n"]) for e in header["entries"] if e["kind"] == "seg"):
        raise ValueError("COALAQ1: dense header with k != n")
    if dense_packed:  # the uint8 codes, rebuilt: what a version-1 dense blob carries
        return (header, out[0], out[1], np.zeros(0, dtype="<i4"), unpack_dense_codes(out[2], ns, bits), raw, None)
    ustart = out[4] if ver != VERSION else None
    if compact:
        ns = [int(e["n"]) for e in header["entries"] if e["kind"] == "seg"]
        ks = [k_for(n, float(header["ratio"])) for n in ns]
        if sum(ks) != K:
            raise ValueError("COALAQ1: kept-entry count mismatch")
        idx, codes = unpack_entries(out[2], ustart, ns, ks, bits)
        out[2], out[3] = idx, (out[3] if bits == RAW_BITS else codes)
    return (header, *out[:4], raw, ustart)
