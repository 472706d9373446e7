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
    k_pack_dense / k_unpack_dense / k_dense_deq_stream (coalac.hip) produce and read the same bytes. unpack() of a
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
    "blockwise" may also be 256 or 1024: the same format with blocks of G = that many elements —
    ceil(n_s / G) blocks per segment, "n_blocks" their sum NB, block g_s of segment s covering its elements
    [G g_s, min(n_s, G (g_s + 1))), mn / scale of length NB; the code stream does not change. A blob with
    "blockwise": 4096 is byte for byte what it was before the other two sizes existed. No other size is defined.

Version 6, ROTATED BLOCK-WISE QUANTISATION (opt-in; header keys "dense": true, "blockwise": 4096, "n_blocks": U and
"rotate": the call's rotation seed, an integer in [0, 2^64)):
         mn f32[U] | scale f32[U] | packed u32[P] | raw bytes
    Version 5's sections at block size 4096, byte for byte in layout and length; what differs is what the codes mean.
    Every block of exactly 4096 elements holds the codes of its Walsh-Hadamard coefficients under the sign diagonal of
    the "rotate" seed, and a decoder applies the inverse after dequantising; a shorter block (a
    segment's ragged end, a small tensor) is version 5's. It is a version of its own, not a version-5 blob with one
    more key, because a reader from before it would decode the coefficients as values and return garbage without a
    word: the version word makes it refuse. "rotate" is rejected without "blockwise", with a block size other than 4096,
    with a seed that is not an integer (a bool is not) in range, and with "dense_packed", "compact" or "n_units".
    unpack() returns mn / scale of length U and the rebuilt uint8 codes of the coefficients.

The executable form of the above is the table FORMATS below: one record per version with the version's ordered
sections (name, dtype, element count) and its header rules. format_of(header) picks the record — nothing else in the
package reads the format keys — and is_dense(header) says whether the indices are implied. pack, sections and unpack are
one walk each over section_list(header), so they cannot disagree on a layout; CompressedUpdate (codec.py) takes its byte
count, the buffers it ships and its staging region from the same list.
"""
import json
import struct
import threading
from collections import OrderedDict, namedtuple

import numpy as np

from ._cache import IdentityCache
from .spec import RAW_BITS, UNIT, VALID_BITS, k_for

MAGIC = b"COALAQ1\0"
VERSION = 1     # mn | scale | idx | vals | raw
VERSION_2 = 2   # ... | vals | ustart | raw
VERSION_3 = 3   # mn | scale | packed | [vals f32] | ustart | raw  (header "compact": true)
VERSION_4 = 4   # mn | scale | packed | raw  (header "dense": true, "dense_packed": true)
VERSION_5 = 5   # mn[U] | scale[U] | packed | raw  (header "dense": true, "blockwise": 256 | 1024 | 4096, "n_blocks": U)
VERSION_6 = 6   # version 5's sections at "blockwise": 4096, the full blocks rotated (header "rotate": the seed)
BLOCK_SIZES = (256, 1024, UNIT)  # the block sizes "blockwise" may name
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


_SIZES = IdentityCache(64)  # entries list -> its fp32 segment sizes (headers of one layout share the list)


def _entry_sizes(entries):
    return [int(e["n"]) for e in entries if e["kind"] == "seg"]


def _seg_sizes(header):
    return _SIZES.get(header["entries"], (), _entry_sizes, header["entries"])


def check_block_size(block):
    """`block` as an int if it is one of BLOCK_SIZES (a bool is not a size), else ValueError."""
    if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or int(block) not in BLOCK_SIZES:
        raise ValueError(f"COALAQ1: block size {block!r} (only {', '.join(map(str, BLOCK_SIZES))} are defined)")
    return int(block)


def block_count(sizes, block=UNIT):
    """Blocks U of dense segments of `sizes` elements: the sum of ceil(n / block) (an empty segment has none)."""
    n = np.asarray(sizes, dtype=np.int64).reshape(-1)
    return int(((n + block - 1) // block).sum())


def block_table(sizes, block=UNIT):
    """The block-wise format's view of dense segments laid out back to back: one row (offset, length) per block of
    `block` elements, in block order — what a decoder applies mn[u] / scale[u] to. int64[U, 2]."""
    rows, off = [], 0
    for n in (int(x) for x in sizes):
        rows += [(off + a, min(block, n - a)) for a in range(0, n, block)]
        off += n
    return np.asarray(rows, dtype=np.int64).reshape(-1, 2)


# -- the format table -----------------------------------------------------------------------------------------------
# One record per wire version: what travels between the JSON header and the raw bytes, and what a header of that
# version must say. sections(header, dense) -> the ordered [(name, numpy dtype, element count)]; rules(header, dense,
# layout) raises ValueError (None: no rules of its own; layout False: the format keys only, for pack(), whose header
# may hold no entries to check counts against). stream: what the "packed" section holds ("entries": version 3's
# fields, "dense": version 4's code stream, None: there is none); per_block: mn / scale hold one entry per block.
Format = namedtuple("Format", "version stream per_block sections rules")
_F4, _U4, _I4, _U1 = np.dtype("<f4"), np.dtype("<u4"), np.dtype("<i4"), np.dtype("u1")


def _ranges(count):
    return [("mn", _F4, count), ("scale", _F4, count)]


def _v1_sections(h, dense):
    K = int(h["total_k"])
    return _ranges(int(h["n_segments"])) + [("idx", _I4, 0 if dense else K),
                                            ("vals", _F4 if int(h["bits"]) == RAW_BITS else _U1, K)]


def _v2_sections(h, dense):
    return _v1_sections(h, dense) + [("ustart", _I4, int(h["n_units"]))]


def _v3_sections(h, dense):
    K, bits = int(h["total_k"]), int(h["bits"])
    return (_ranges(int(h["n_segments"])) + [("packed", _U4, packed_words(K, bits))]
            + ([("vals", _F4, K)] if bits == RAW_BITS else []) + [("ustart", _I4, int(h["n_units"]))])


def _code_stream(h):
    return ("packed", _U4, dense_packed_words(_seg_sizes(h), h["bits"]))


def _v4_sections(h, dense):
    return _ranges(int(h["n_segments"])) + [_code_stream(h)]


def _v5_sections(h, dense):
    return _ranges(int(h["n_blocks"])) + [_code_stream(h)]


def _need_code_bits(h, layout, widest, what):
    """bits in 1..widest; a header without bits passes only where the layout is not checked (layout=False)."""
    if (layout or "bits" in h) and not 1 <= int(h.get("bits", 0)) <= widest:
        raise ValueError(f"COALAQ1: {what} codes are 1..{widest} bits wide, not {h.get('bits')}")


def _v3_rules(h, dense, layout):
    if dense or "n_units" not in h:
        raise ValueError("COALAQ1: a compact payload is sparse and carries its per-unit starts (\"n_units\")")
    if layout and (h.get("bits") not in VALID_BITS or int(h["total_k"]) < 0):
        raise ValueError("COALAQ1: bad compact header")


def _v4_rules(h, dense, layout):
    if not dense or h.get("compact") or "n_units" in h:
        raise ValueError("COALAQ1: a dense-packed payload needs \"dense\" and excludes \"compact\" and per-unit starts")
    _need_code_bits(h, layout, 7, "dense-packed")


def _v5_rules(h, dense, layout):
    if not dense:
        raise ValueError("COALAQ1: \"blockwise\" needs a \"dense\" payload")
    block = check_block_size(h["blockwise"])
    if h.get("dense_packed") or h.get("compact") or "n_units" in h:
        raise ValueError("COALAQ1: \"blockwise\" excludes \"dense_packed\", \"compact\" and per-unit starts")
    _need_code_bits(h, layout, 8, "block-wise")
    if layout and int(h.get("n_blocks", -1)) != block_count(_seg_sizes(h), block):
        raise ValueError("COALAQ1: header n_blocks is not the layout's block count")


def check_rotate_seed(seed):
    """`seed` as an int if it is an integer in [0, 2^64) (a bool is not a seed), else ValueError."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
        raise ValueError(f"COALAQ1: \"rotate\" is the rotation seed, an integer in [0, 2^64), not {seed!r}")
    return int(seed)


def _v6_rules(h, dense, layout):
    if "blockwise" not in h:
        raise ValueError("COALAQ1: \"rotate\" needs a \"blockwise\" payload")
    _v5_rules(h, dense, layout)
    if h["blockwise"] != UNIT:
        raise ValueError(f"COALAQ1: \"rotate\" is defined for {UNIT}-element blocks only, not {h['blockwise']}")
    check_rotate_seed(h["rotate"])


FORMATS = (Format(VERSION, None, False, _v1_sections, None),
           Format(VERSION_2, None, False, _v2_sections, None),
           Format(VERSION_3, "entries", False, _v3_sections, _v3_rules),
           Format(VERSION_4, "dense", False, _v4_sections, _v4_rules),
           Format(VERSION_5, "dense", True, _v5_sections, _v5_rules),
           Format(VERSION_6, "dense", True, _v5_sections, _v6_rules))


def format_of(header):
    """The Format a header describes: the one place that reads the format keys, in their order of precedence."""
    if "rotate" in header:
        return FORMATS[5]
    if "blockwise" in header:
        return FORMATS[4]
    if header.get("dense_packed"):
        return FORMATS[3]
    if header.get("compact"):
        return FORMATS[2]
    return FORMATS[1] if "n_units" in header else FORMATS[0]


def is_dense(header, on_wire=False):
    """Implied indices (0..n-1 per segment, an empty idx section). A header in a blob says so itself ("dense": true);
    a carrier's in-memory header (UpdateCodec._encode) has no such key and is dense at ratio 1. on_wire: the header
    is one read from, or written into, a blob, where the key alone counts: a ratio-1 blob without it ships its
    indices (the payloads of before the key existed)."""
    return bool(header.get("dense")) or (not on_wire and header.get("ratio", 0.0) >= 1.0)


def section_list(header, on_wire=False):
    """The ordered (name, numpy dtype, element count) of every array section of a payload with this header, between
    the JSON header and the raw bytes: the layouts of the module docstring, stated once."""
    return format_of(header).sections(header, is_dense(header, on_wire))


def check_header(header, on_wire=False):
    """The header rules of the header's format, counts checked against its entries (ValueError)."""
    fmt, dense = format_of(header), is_dense(header, on_wire)
    if fmt.rules is not None:
        fmt.rules(header, dense, True)
    if dense and int(header["total_k"]) != sum(_seg_sizes(header)):
        raise ValueError("COALAQ1: dense header with k != n")


def _section_offsets(secs, pos):
    """([(name, dtype, count, byte offset)], offset of the raw bytes) of a section_list behind a header that ends at
    byte pos: every section, and the raw bytes, at the next 16-byte boundary."""
    out = []
    for name, dt, n in secs:
        pos += _pad16(pos)
        out.append((name, dt, n, pos))
        pos += n * dt.itemsize
    return out, pos + _pad16(pos)


def pack(header, mn, scale, idx, vals, raw, header_json=None, ustart=None, packed=None):
    """numpy arrays + raw bytes -> blob (bytes): the sections the header's format lists (section_list), each taken from
    the argument of its name, which must hold as many elements as the header says; arguments the format has no section
    for are ignored (idx and uint8 vals next to a packed stream), except that ustart and packed must be None then. A
    "dense" header's idx is implied and not written. header_json: the header's JSON encoding, if the caller has it
    already; `header` then needs only what names the format and counts its sections."""
    fmt, dense = format_of(header), is_dense(header, on_wire=True)
    if fmt.rules is not None:  # (layout=False, the format keys only: this header may hold no entries to count)
        fmt.rules(header, dense, False)
    h = header_json if header_json is not None else encode_header(header)
    given = {"mn": mn, "scale": scale, "idx": idx, "vals": vals, "ustart": ustart, "packed": packed}
    secs, end = _section_offsets(fmt.sections(header, dense), 16 + len(h))
    names = [s[0] for s in secs]
    if (ustart is not None and "ustart" not in names) or (packed is not None and "packed" not in names):
        raise ValueError("COALAQ1: per-unit starts or a packed stream where the header describes none")
    parts, size = [MAGIC, struct.pack("<II", fmt.version, len(h)), h], 16 + len(h)
    for name, dt, n, off in secs:
        implied = given[name] is None or (name == "idx" and n == 0)  # (a dense header: whatever idx holds stays home)
        arr = np.zeros(0, dt) if implied else np.ascontiguousarray(given[name], dt).reshape(-1)
        if arr.size != n:
            raise ValueError(f"COALAQ1: section {name} holds {arr.size} elements, the header says {n}")
        parts += [b"\0" * (off - size), arr.tobytes()]
        size = off + arr.nbytes
    parts += [b"\0" * (end - size), bytes(raw)]
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


def _open(blob, header=None):
    """(memoryview, version word, header, end of the header) of a blob; header: parsed already (the caller's own)."""
    mv = memoryview(blob)
    if bytes(mv[:8]) != MAGIC:
        raise ValueError("not a COALAQ1 blob (bad magic)")
    ver, hl = struct.unpack_from("<II", mv, 8)
    return mv, ver, _parse_header(mv, hl) if header is None else header, 16 + hl


def sections(blob, header=None):
    """(header, {name: (byte offset, byte count)}) of the array sections in `blob`, in blob order (section_list): they
    lie back to back, each 16-byte aligned, so one host-to-device copy moves all of them. header: the blob's own,
    parsed already, or its carrier's in-memory one (CompressedUpdate.header)."""
    mv, _, h, pos = _open(blob, header)
    return h, {name: (off, n * dt.itemsize) for name, dt, n, off in _section_offsets(section_list(h, header is None), pos)[0]}


def unpack(blob):
    """blob -> (header dict, mn, scale, idx, vals, raw bytes, ustart or None). Arrays are read-only views of
    blob; a "dense" blob's idx is empty (implied). A compact (version 3) blob's idx and uint8 vals are rebuilt
    from its packed stream (unpack_entries, with every segment's k = k_for(n, ratio) as validate() expects), a
    version-4 / 5 blob's uint8 codes from its own (unpack_dense_codes). A block-wise (version 5) blob's mn / scale
    have one entry per block."""
    mv, ver, header, pos = _open(blob)
    fmt = format_of(header)
    if fmt.version != ver:
        raise ValueError(f"COALAQ1: version word {ver}, but the header's keys (\"rotate\", \"blockwise\", \"dense_packed\", "
                         f"\"compact\", \"n_units\") describe version {fmt.version}")
    check_header(header, on_wire=True)
    secs, raw_at = _section_offsets(section_list(header, on_wire=True), pos)
    out = {}
    for name, dt, n, off in secs:
        if n < 0 or off + n * dt.itemsize > len(mv):
            raise ValueError("COALAQ1: truncated blob")
        out[name] = np.frombuffer(mv, dtype=dt, count=n, offset=off)
    idx, vals, bits = out.get("idx"), out.get("vals"), int(header["bits"])
    if fmt.stream == "entries":
        ns = _seg_sizes(header)
        ks = [k_for(n, float(header["ratio"])) for n in ns]
        if sum(ks) != int(header["total_k"]):
            raise ValueError("COALAQ1: kept-entry count mismatch")
        idx, codes = unpack_entries(out["packed"], out["ustart"], ns, ks, bits)
        vals = vals if bits == RAW_BITS else codes
    elif fmt.stream == "dense":  # the uint8 codes, rebuilt: what a version-1 dense blob carries
        idx, vals = np.zeros(0, dtype="<i4"), unpack_dense_codes(out["packed"], _seg_sizes(header), bits)
    return header, out["mn"], out["scale"], idx, vals, bytes(mv[raw_at:]), out.get("ustart")
