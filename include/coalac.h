/*
 * coalac.h — C ABI of the MI355X (gfx950) model-update codec (CodecSpec v1: per-tensor top-k + 8-bit
 * quantise). This is the drop-in boundary for COALA's compression plugin surface.
 *
 * The reference (SonyResearch/COALA) is 100 % Python and has NO codec and NO FFI: coala/compression/
 * __init__.py is 0 bytes. The entry points below replace the work the reference's empty hooks would do:
 *
 *   coalac_encode  <- BaseClient.compression()          /root/reference/coala/client/base.py:330-332
 *                     (called from run_train, base.py:153; its output rides in UploadContent.data via
 *                      codec.marshal, base.py:363 / coala/protocol/codec.py:4-5)
 *                     and BaseServer.compression()        /root/reference/coala/server/base.py:347-349
 *   coalac_decode  <- BaseServer.decompression(model)   /root/reference/coala/server/base.py:558-560
 *                     (called at server/base.py:376 and server/service.py:106,125)
 *                     and BaseClient.decompression()      /root/reference/coala/client/base.py:203-205
 *   coalac_plan_*  <- no counterpart: a tensor layout (segment table) is fixed for a whole FL task, so
 *                     the device-side metadata is built once per layout and reused every round.
 *
 * Conventions
 *   - Every d_* pointer is a DEVICE pointer owned by the caller (e.g. torch tensor storage).
 *   - All work is enqueued on the caller's HIP stream (`stream`, a hipStream_t; NULL = default stream)
 *     and returns immediately. No host synchronisation, no allocation inside encode/decode.
 *   - Re-entrant: no global mutable state. A plan is immutable after creation and may be shared by
 *     threads; each concurrent encode needs its own workspace.
 *   - Errors: return value 0 = OK, negative = error code below; nothing throws across the ABI. The
 *     message of the last failed call on the calling thread is in coalac_last_error().
 */
#ifndef COALAC_H
#define COALAC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COALAC_ABI_VERSION 11

enum {
  COALAC_OK = 0,
  COALAC_EINVAL = -1,      /* invalid argument (bad segment table, null pointer, misaligned offset) */
  COALAC_EBITS = -2,       /* unsupported bit width (valid: 1..8, or 32 = raw fp32 values) */
  COALAC_EWORKSPACE = -3,  /* workspace smaller than coalac_plan_query() says */
  COALAC_EHIP = -4,        /* a HIP runtime call or kernel launch failed */
  COALAC_EDEVICE = -5,     /* called with a different current device than the plan was created on */
  COALAC_ENOMEM = -6       /* device allocation for the plan failed */
};

enum {
  COALAC_FLAG_FORCE_EXACT = 1,    /* test hook: re-select every large segment exactly (no sampling) */
  COALAC_FLAG_GENERIC_SELECT = 2, /* test hook: resolve the k-th key with the multi-pass select only */
  COALAC_FLAG_STAMPS = 4,         /* diagnostics: record per-block phase timestamps of k_select */
  COALAC_FLAG_NO_FORK = 8         /* encode small segments inside k_scan, never on the plan's side stream
                                     (for callers that run several plans concurrently themselves) */
};
/* (ABI 3 dropped ABI 2's COALAC_FLAG_ONE_LAUNCH / FRONT_LAUNCH / ITEM_STAMPS: the one-launch encode variants
 * measured slower than the kernel sequence, DESIGN.md §6c. ABI 4 added the per-unit starts d_ustart to encode,
 * decode and aggregate: wire v2. ABI 5 makes them required by the sparse decode and the aggregate — a host that
 * receives a version-1 payload computes them (coala_amd/compression/plan.py) — and drops the decode workspace,
 * the k_bounds / k_fill / k_scatter kernels and the staged (_sched) entry points; plans whose every segment keeps
 * all its elements run the dense codec, with the indices implied. ABI 6 adds the error-feedback pair
 * coalac_ef_accumulate / coalac_ef_commit — a client-side residual memory around an unchanged encode; no existing
 * entry point changes. ABI 7 adds the compact payload's coalac_plan_packed_bytes / coalac_pack / coalac_unpack — a
 * lossless repacking of idx / vals after an unchanged encode and before an unchanged decode; again no existing entry
 * point, plan query or workspace size changes. ABI 8 adds the bit-packed dense codes' coalac_plan_dense_packed_bytes /
 * coalac_pack_dense / coalac_unpack_dense / coalac_decode_packed — the same kind of lossless repacking for a dense
 * plan's uint8 codes (wire v4); once more nothing that existed changes. ABI 9 adds the block-wise dense pair
 * coalac_encode_block / coalac_decode_block — one quantisation range per 4096-element unit of a dense plan, encoded in
 * one pass into the wire v4 code stream (wire v5); every existing entry point, query and size is as it was. ABI 10 adds
 * the one entry point coalac_aggregate_dense — the fused decode + FedAvg of ratio-1 uploads read from their own uint8
 * codes, wire v4 streams or block-wise (wire v5) streams; nothing that existed changes. ABI 11 adds the one entry point
 * coalac_aggregate_uploads — the sparse fused decode + FedAvg read from each upload's own idx / vals arrays or wire v3
 * stream; nothing that existed changes. Still ABI 11: the stochastic-rounding pair coalac_encode_sr /
 * coalac_encode_block_sr is purely additive — two new symbols beside their deterministic twins, no existing entry
 * point, flag, query, workspace size or payload changes — so the version a loader checks stays what it was; a caller
 * that needs the pair looks the symbols up. The same holds for coalac_encode_block_ef, the block-wise encode with error
 * feedback in one pass: one more symbol, nothing that existed changes.) */

/* One fp32 segment (= one flattened tensor of the state_dict). Offsets are in ELEMENTS.
 *   in_off : start of the segment in the flat input / dense output buffer; must be a multiple of 4
 *   n      : element count, 0 <= n < 2^31
 *   k      : kept elements, 0 if n == 0 else 1 <= k <= n (host computes max(1, min(n, ceil(n*ratio)))). Any
 *            1 <= k <= n is accepted per segment, independently of the other segments' (k = 1, n - 1 and n of a
 *            large segment inside a sparse plan included), and tested so: tests/test_gpu_high_ratio.py.
 *   out_off: start of this segment's k entries in the idx / vals arrays                              */
typedef struct coalac_seg {
  uint64_t in_off;
  uint64_t n;
  uint64_t k;
  uint64_t out_off;
} coalac_seg_t;

typedef struct coalac_plan* coalac_plan_t;

int coalac_version(void);
const char* coalac_last_error(void);

/* Build the device metadata for a segment table (HOST pointer) on the current device.
 * bits: 1..8 -> uint8 codes (vals is uint8_t[total_k]); 32 -> raw fp32 values (vals is float[total_k]). */
int coalac_plan_create(const coalac_seg_t* h_segs, int nseg, int bits, coalac_plan_t* out);
int coalac_plan_destroy(coalac_plan_t plan);

/* ws_bytes: the workspace coalac_encode needs (decode and aggregate need none);
 * total_k: length of idx/vals;
 * span: max(in_off + n) = the minimum length (elements) of the input/output flat buffers;
 * n_units: 4096-element work units (segment by segment: ceil(n / 4096) each) = the length of the per-unit
 * starts array (ustart). Any output pointer may be NULL. */
int coalac_plan_query(coalac_plan_t plan, uint64_t* ws_bytes, uint64_t* total_k, uint64_t* span, uint64_t* n_units);

/* Encode d_in (fp32[span]) into idx (int32[total_k], segment-relative, ascending per segment),
 * vals (uint8[total_k] codes or fp32[total_k]), mn (fp32[nseg]) and scale (fp32[nseg]).
 * d_ustart (uint32[n_units], or NULL = not written): per 4096-element unit, the index (segment-relative, into
 * the segment's idx list) of its first kept entry — the wire v2 section that lets a decoder find every unit's
 * entries without searching the idx lists (coalac_decode / coalac_aggregate d_ustart).
 * d_base != NULL selects delta mode: the codec encodes (d_in - d_base).
 * A DENSE plan (every segment's k == n: ratio 1, the download direction's default) runs the dense codec: a
 * per-segment min / max pass, then one quantise stream; its indices are implied (0..n-1 per segment) and d_idx /
 * d_ustart may be NULL (given, they are written too). */
int coalac_encode(coalac_plan_t plan, const float* d_in, const float* d_base, int32_t* d_idx,
                  void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes,
                  unsigned flags, void* stream);

/* Encode with every segment read from its OWN device pointer: d_seg_in is a DEVICE array of nseg
 * pointers, d_seg_in[s] -> fp32[n_s], 16-byte aligned (e.g. the data pointers of a model's parameters:
 * the plugin encodes the trained state in place, with no flattening copy — client compression(),
 * coala/client/base.py:330-332). d_base (delta mode) stays a flat buffer indexed by in_off. Outputs,
 * workspace, flags and stream as coalac_encode. */
int coalac_encode_segptr(coalac_plan_t plan, const float* const* d_seg_in, const float* d_base, int32_t* d_idx,
                         void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes,
                         unsigned flags, void* stream);

/* Decode into the dense d_out (fp32[span]); only positions inside segments are written.
 * d_ustart: the encoder's per-unit starts (wire v2; required unless the plan is dense — a host holding a v1
 * payload computes them: for unit u of a segment, the number of the segment's kept indices below u * 4096).
 * d_base != NULL: d_out = d_base + decoded (fused; d_out may alias d_base). The encoded arrays may come from an
 * untrusted blob: out-of-range or unsorted indices, or wrong starts, can mis-decode but never write outside the
 * unit (still, validate blobs on the host; coala_amd/compression/codec.py validate() does). A dense plan decodes
 * positionally (d_idx / d_ustart are not read). */
int coalac_decode(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                  const float* d_scale, const uint32_t* d_ustart, const float* d_base, float* d_out, void* stream);

/* Error feedback for a top-k upload (EF-SGD / "sparsified SGD with memory"): what an encode drops is kept in a
 * per-client residual d_resid (fp32[span], the plan's flat input layout, 16-byte aligned, zero at the start) and added
 * to the next round's update. One round, all on one stream:
 *
 *   coalac_ef_accumulate(plan, d_in | d_seg_in, d_base, d_resid, stream)   r[i] = (x[i] - base[i]) + r[i]
 *   coalac_encode(plan, d_resid, NULL, ...same stream...)                  the payload of `r` as a plain input
 *   coalac_ef_commit(plan, idx, vals, mn, scale, ustart, d_resid, stream)  r[pos] = r[pos] - xhat at every kept entry
 *
 * accumulate: fp32 subtract, then fp32 add (d_base NULL: r[i] = x[i] + r[i]), for every element of every segment;
 * the padding between segments is not written. Exactly one of d_in (flat, indexed by in_off) and d_seg_in (a DEVICE
 * array of per-segment pointers, as coalac_encode_segptr takes) is non-NULL; both or neither is COALAC_EINVAL (checked
 * before the plan is used).
 * commit: xhat is what coalac_decode writes for the entry — mn + float(q) * scale, fp32 multiply then fp32 add, or the
 * stored fp32 value (bits 32) — so the residual is exactly what the server did not reconstruct; a result that is NaN
 * or +-Inf is stored as +0.0f. Positions that were not kept are left as they are: they hold the accumulated value,
 * which is their residual. A sparse plan needs d_idx and d_ustart (NULL: COALAC_EINVAL); a dense plan takes every
 * position as a kept entry and reads neither.
 * Both are one asynchronous launch: no allocation, no workspace, no host synchronisation; they follow the plan's unit
 * table, so batched (`clients` copies) and explicit-row plans work alike. Stream order suffices between the three
 * calls: coalac_encode may fork small segments to the plan's side stream, but it makes `stream` wait for that
 * stream's join event before it returns (launch_encode), so work enqueued on `stream` afterwards sees every output of
 * the encode. The payload is an ordinary one: with d_base given to accumulate, the server decodes it as delta mode. */
int coalac_ef_accumulate(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                         float* d_resid, void* stream);
int coalac_ef_commit(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                     const float* d_scale, const uint32_t* d_ustart, float* d_resid, void* stream);

/* Compact payload (wire v3): entry j of the plan's idx / vals arrays as one w-bit field, w = 12 + b, where b = bits
 * (1..8) or 0 at bits 32 (the fp32 values then stay in d_vals and are neither packed nor unpacked):
 *
 *   field_j = (idx[j] & 0xFFF) | (code_j << 12)
 *
 * in a little-endian bit stream of uint32 words: field j occupies bits [j w, (j + 1) w), bit t of the stream is bit
 * t % 32 of word t / 32; the stream is ceil(total_k w / 32) words long and its padding bits are zero. j is the position
 * in idx / vals, so out_off, batched and explicit-row plans are honoured (an explicit-row plan packs every position
 * below its total_k, its own or not). The upper bits of an index are its 4096-element unit's number, which the per-unit
 * starts (d_ustart) already say: unit u of a segment, its u_s-th, owns the segment-relative entries
 * [ustart[u], ustart[u + 1]) (the segment's last unit ends at k), clamped to [0, k] with begin <= end exactly as
 * coalac_decode clamps; for each owned entry e, j = out_off + e, idx[j] = (u_s << 12) | (field_j & 0xFFF) and
 * vals[j] = field_j >> 12. Whatever the starts say, unpack writes only idx[j] / vals[j] with
 * out_off <= j < out_off + k of the unit's own segment.
 * Each call is one asynchronous launch on `stream`: no allocation, no workspace, no host synchronisation. Any NULL
 * pointer, a packed_bytes below coalac_plan_packed_bytes, or a dense plan (every k == n: its indices are implied and
 * wire v2 carries it) is COALAC_EINVAL. coalac_pack needs d_idx and d_vals 16-byte aligned. */
int coalac_plan_packed_bytes(coalac_plan_t plan, uint64_t* bytes);
int coalac_pack(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, void* d_packed, uint64_t packed_bytes,
                void* stream);
int coalac_unpack(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const uint32_t* d_ustart,
                  int32_t* d_idx, void* d_vals, void* stream);

/* Bit-packed dense codes (wire v4): the uint8 codes of a DENSE plan (every k == n) with code width b = bits, 1 <= b <= 8
 * (the host packs only b <= 7: at 8 the stream is as long as the codes), as b-bit fields:
 *
 *   segment s, in the plan's row order, owns W_s = ceil(n_s b / 32) uint32 words at word offset pw_s = sum of W_t, t < s
 *   (an empty segment owns none; pw_s does not depend on out_off); the stream is P = sum of W_s words;
 *   entry e of segment s — its code vals[out_off_s + e] — occupies bits [e b, (e + 1) b) of the segment's sub-stream,
 *   little-endian as above (bit t is bit t % 32 of word t / 32); the padding bits of a segment's last word are zero.
 *
 * Every 4096-element unit of a segment therefore starts on a word (unit u_s at word pw_s + 128 b u_s), and one wave per
 * unit owns whole words. coalac_pack_dense writes only the words [pw_s, pw_s + W_s) of the plan's segments;
 * coalac_unpack_dense, its inverse, only vals[out_off_s + [0, n_s)) — the adapter for every consumer of uint8 codes
 * (coalac_decode, coalac_aggregate, coalac_ef_commit). coalac_decode_packed is coalac_decode of a dense plan reading the
 * stream itself, with no byte-per-element intermediate: d_out (and d_base, fused: d_out = d_base + decoded) as
 * coalac_decode takes them, the result bit-identical to coalac_unpack_dense followed by coalac_decode. Any b-bit field
 * is a legal code, so an untrusted stream can mis-decode but not produce a code above 2^b - 1; padding bits are ignored.
 * Each call is one asynchronous launch on `stream`: no allocation, no workspace, no host synchronisation. Any NULL
 * pointer (d_base excepted), a sparse plan, a plan with bits == 32, or a packed_bytes below
 * coalac_plan_dense_packed_bytes (= 4 P) is COALAC_EINVAL; d_packed and d_vals are 4-byte aligned. Here and in the
 * block-wise entry points below every COALAC_EINVAL case is checked before the first device call, and before a plan
 * without units returns COALAC_OK. */
int coalac_plan_dense_packed_bytes(coalac_plan_t plan, uint64_t* bytes);
int coalac_pack_dense(coalac_plan_t plan, const void* d_vals, void* d_packed, uint64_t packed_bytes, void* stream);
int coalac_unpack_dense(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, void* d_vals, void* stream);
int coalac_decode_packed(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_mn,
                         const float* d_scale, const float* d_base, float* d_out, void* stream);

/* Block-wise dense quantisation (wire v5): a DENSE plan (every k == n) with bits 1..8, every 4096-element unit of it
 * (the plan's unit table: segment by segment ceil(n / 4096) each, row after row; coalac_plan_query's n_units = U of
 * them) quantised over its OWN range. Unit u, the u_s-th of segment s, covers the segment's elements
 * [4096 u_s, min(n_s, 4096 (u_s + 1))), and CodecSpec v1 applies to it as if it were a segment with k = n:
 *
 *   bmn[u]    = the NaN-ignoring min of the unit's values (x, or x - base in delta mode), + 0.0f
 *   bscale[u] = 0 if max == min else (max - min) / (2^bits - 1)          (max likewise NaN-ignoring, + 0.0f)
 *   code      = coalac_encode's quantise with (bmn[u], bscale[u]);  decoded = bmn[u] + float(code) * bscale[u]
 *               (fp32 multiply, then fp32 add; + base, fused, as coalac_decode)
 *
 * The codes leave and arrive as the wire v4 stream above, bit for bit its layout and length (coalac_plan_dense_packed_
 * bytes; at 8 bits the stream is the codes): segment s owns the words [pw_s, pw_s + W_s), unit u_s starts at word
 * pw_s + 128 b u_s, padding bits are written as zero and ignored on decode. coalac_encode_block reads the update once
 * (no min / max pre-pass, no per-segment reduction, no byte-per-element codes) and writes bmn[U], bscale[U] and only
 * the stream words of the plan's segments; exactly one of d_in (flat fp32[span], indexed by in_off) and d_seg_in (a
 * DEVICE array of per-segment pointers, as coalac_encode_segptr takes) is non-NULL, d_base != NULL selects delta mode.
 * coalac_decode_block is coalac_decode_packed with each unit's own range. Each call is one asynchronous launch on
 * `stream`: no allocation, no workspace, no host synchronisation. COALAC_EINVAL: both or neither of d_in / d_seg_in, a
 * sparse plan, bits == 32 (nothing to scale), a NULL pointer other than d_base, a packed_bytes below
 * coalac_plan_dense_packed_bytes, d_in / d_base / d_out not 16-byte or d_bmn / d_bscale / d_packed not 4-byte
 * aligned. A plan without units returns COALAC_OK and launches nothing. */
int coalac_encode_block(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                        float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, void* stream);
int coalac_decode_block(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_bmn,
                        const float* d_bscale, const float* d_base, float* d_out, void* stream);

/* Stochastic (unbiased) rounding for the dense quantisers. The range of every segment
 * (coalac_encode_sr) or 4096-element unit (coalac_encode_block_sr) is computed exactly as by the deterministic twin;
 * only the code of an element changes: with t = (v - mn) / scale (the IEEE fp32 quotient) it is floor(t) or
 * floor(t) + 1, the latter when u < t - floor(t), where u in [0, 1) holds 24 bits hashed from `seed` and the element's
 * flat position in_off_s + e (a pure function of the two: the same seed gives the same payload, with d_seg_in as with
 * d_in). 0 where !(scale > 0) or !(t > 0), 2^bits - 1 where t >= it; an integer t is kept. The decoded value is an
 * unbiased estimate of v, so the error of an average of C uploads encoded with different seeds falls as 1 / sqrt(C).
 * The outputs are ordinary: coalac_decode*, coalac_pack_dense and coalac_aggregate_dense read them as they are.
 *
 * coalac_encode_sr is the dense encode of coalac_encode / coalac_encode_segptr: exactly one of d_in (flat fp32[span])
 * and d_seg_in (a DEVICE array of per-segment pointers) is non-NULL, d_base != NULL selects delta mode, d_vals
 * uint8[total_k], d_mn / d_scale fp32[nseg], the workspace is coalac_encode's; the indices and per-unit starts are
 * implied and not written. coalac_encode_block_sr is coalac_encode_block plus the seed. Errors (COALAC_EINVAL): a
 * sparse plan, bits == 32, both or neither input, and the NULL-pointer, size and alignment cases of the twins
 * (COALAC_EWORKSPACE for a short workspace). A plan without segments (units) returns COALAC_OK and launches nothing. */
int coalac_encode_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                     void* d_vals, float* d_mn, float* d_scale, void* d_ws, uint64_t ws_bytes, uint64_t seed,
                     unsigned flags, void* stream);
int coalac_encode_block_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                           float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t seed,
                           void* stream);

/* Error feedback for a block-wise upload in one pass (an addition to CodecSpec v1, bit for bit).
 * coalac_encode_block of a = (x - base) + r with the residual r (d_resid: fp32[span], the plan's flat input layout,
 * indexed by in_off, 16-byte aligned, zero at the start) read and rewritten in the same launch. Per 4096-element unit u:
 *
 *   a[i]      = (x[i] - base[i]) + r[i]        fp32 subtract, then fp32 add (d_base NULL: x[i] + r[i]) — exactly
 *                                              coalac_ef_accumulate's arithmetic
 *   bmn[u], bscale[u], code                    coalac_encode_block's, of the unit's a (a code past a ragged unit's end
 *                                              is 0)
 *   xhat      = bmn[u] + float(code) * bscale[u]   what coalac_decode_block writes without a base: fp32 multiply, then add
 *   r[i]      = a[i] - xhat, stored as +0.0f where that is NaN or +-Inf (coalac_ef_commit's rule)
 *
 * Only the elements of segments are written to r: the padding between segments and everything past the last segment
 * stay as they were. For any input, bmn, bscale, the stream and r equal the result of coalac_ef_accumulate(plan, x,
 * base, r); coalac_encode_block(plan, d_in = r, no base); r[i] = r[i] - d[i] (+0.0f where not finite), d being
 * coalac_decode_block of that payload without a base. The payload is an ordinary delta-mode wire v5 payload:
 * coalac_decode_block and coalac_aggregate_dense (kind BLOCK) read it as any other. d_resid must not alias any other
 * argument. One asynchronous launch on `stream`: no workspace, no allocation, no host synchronisation. COALAC_EINVAL
 * (all checked before the first device call): every case coalac_encode_block rejects, d_resid NULL, d_resid not
 * 16-byte aligned. A plan without units returns COALAC_OK and launches nothing. There is no stochastic variant
 * (the residual already returns the rounding error to the client). */
int coalac_encode_block_ef(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                           float* d_resid, float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes,
                           void* stream);

/* Profiling variants: identical work, plus hipEventRecord(events[i], stream) between kernels.
 * encode: [0] before k_sample, [1] after k_sample, [2] after k_scan, [3] after the select kernels
 *         (k_ghist, k_gwin, k_select), [4] after k_emit (recorded even if the plan has no large segment);
 *         dense plans: [1] after the min / max pass, [2] after the quantise stream;
 * decode: [0] at the start, [1] before the decode kernel, [2] after it. NULL array or NULL entries are skipped. */
int coalac_encode_ev(coalac_plan_t plan, const float* d_in, const float* d_base, int32_t* d_idx,
                     void* d_vals, float* d_mn, float* d_scale, uint32_t* d_ustart, void* d_ws, uint64_t ws_bytes,
                     unsigned flags, void* stream, void* const* events);
int coalac_decode_ev(coalac_plan_t plan, const int32_t* d_idx, const void* d_vals, const float* d_mn,
                     const float* d_scale, const uint32_t* d_ustart, const float* d_base, float* d_out, void* stream,
                     void* const* events);

/* Fused server-side decode + FedAvg of the `clients` updates the plan batches.
 * Replaces, on the server, decompression of every upload (coala/server/base.py:558-560, called :376)
 * followed by strategies.federated_averaging (coala/server/strategies.py:6-29, 57-90) on the decoded
 * modules, for the fp32 entries. The plan's table must be `clients` copies of one layout at constant
 * input / output strides (client-major, as a batched encode uses). Per element of client 0's layout:
 *   x_i = d_base + decoded_i   (decoded_i = +0.0f where client i did not keep the element; without a
 *                               base x_i = decoded_i: exactly what coalac_decode writes)
 *   acc = x_0 * w_0;  acc = acc + (x_i * w_i) for i = 1.. in client order (fp32, no FMA)
 *   d_out = acc / total               (mode COALAC_AGG_DIV: torch's CPU division by a scalar)
 *         = acc * (1.0f / total)      (mode COALAC_AGG_RECIP: torch's GPU division by a host scalar)
 *         = acc                       (mode COALAC_AGG_SUM: strategies.weighted_sum, :57-90 — the
 *                                      multi-GPU server's per-rank sum before reduce_models'
 *                                      all_reduce + division, coala/server/base.py:595-598)
 * d_avg_mask: DEVICE uint8[segments per client] or NULL (= every segment averaged). A segment whose byte
 * is 0 is not averaged: d_out = x_0, client 0's decoded value — aggregation_content "parameters"
 * (coala/server/base.py:588-591), where strategies.weighted_sum_only_params / federated_averaging_only_params
 * average the parameters only and keep models[0]'s buffers (coala/server/strategies.py:32-54, 93-124).
 * d_weights: DEVICE fp32[clients] = float(w_i); total: float(sum of the weights). d_out / d_base are
 * indexed like client 0's segments. d_ustart: the clients' per-unit starts, concatenated in client order
 * (uint32[n_units]; required). Only the elements of client 0's segments are written to d_out: the alignment pads
 * between segments and anything after the last segment are left as they are, so a d_out that ends with the last
 * segment suffices. The encoded arrays may come from untrusted blobs: out-of-range or unsorted indices, or wrong
 * starts, can mis-aggregate but never write outside the unit — every unit's entry range is clamped and every entry
 * bounds-checked exactly as coalac_decode does, so the result is still decode-each followed by the weighted sum.
 * Events (the _ev variant): [0] at the start, [1] before k_aggregate, [2] after. */
enum { COALAC_AGG_DIV = 0, COALAC_AGG_RECIP = 1, COALAC_AGG_SUM = 2 };
int coalac_aggregate(coalac_plan_t plan, int clients, const int32_t* d_idx, const void* d_vals,
                     const float* d_mn, const float* d_scale, const uint32_t* d_ustart, const float* d_weights,
                     float total, int mode, const uint8_t* d_avg_mask, const float* d_base, float* d_out,
                     void* stream);
int coalac_aggregate_ev(coalac_plan_t plan, int clients, const int32_t* d_idx, const void* d_vals,
                        const float* d_mn, const float* d_scale, const uint32_t* d_ustart, const float* d_weights,
                        float total, int mode, const uint8_t* d_avg_mask, const float* d_base, float* d_out,
                        void* stream, void* const* events);

/* Fused decode + FedAvg of `clients` ratio-1 (dense) uploads, each read where it lies. `plan` is a
 * ONE-LAYOUT dense plan (every k == n, bits 1..8): the layout is the plan's own table, and d_out / d_base are indexed by
 * its in_off. Per element of every segment, in client order — coalac_aggregate's contract, bit for bit:
 *   x_i = d_base + decoded_i (without a base: decoded_i);  decoded_i = mn + float(q_i) * scale (fp32 multiply, then add)
 *   acc = x_0 * w_0;  acc = acc + (x_i * w_i), i = 1..clients-1 (fp32, no FMA);  d_out = acc / total | acc * (1.0f /
 *   total) | acc by `mode` (COALAC_AGG_DIV | RECIP | SUM); a segment whose d_avg_mask byte is 0 gets d_out = x_0.
 * So the result equals coalac_decode / coalac_decode_packed / coalac_decode_block of every upload followed by the
 * reference's weighted_sum and division (coala/server/strategies.py:6-29, 57-90), without the `clients` dense copies.
 * kind says what client i's buffers hold:
 *   COALAC_AGGD_CODES   d_codes[i]: uint8 codes, entry e of segment s at out_off_s + e (wire v2 dense); mn / scale fp32[nseg]
 *   COALAC_AGGD_PACKED  d_codes[i]: the wire v4 stream of the plan (coalac_pack_dense's layout);     mn / scale fp32[nseg]
 *   COALAC_AGGD_BLOCK   d_codes[i]: the same stream; mn / scale fp32[n_units], one pair per 4096-element unit (wire v5,
 *                       coalac_encode_block's bmn / bscale)
 * d_codes, d_mn, d_scale: DEVICE arrays of `clients` device pointers (as coalac_encode_segptr takes d_seg_in): every
 * upload stays where it was copied to — no concatenation, no batched `clients`-copies plan, no implied indices.
 * code_bytes: the length of EACH client's code buffer, at least total_k (CODES) or coalac_plan_dense_packed_bytes (the
 * stream kinds). d_weights: DEVICE fp32[clients]; total: float(sum of the weights); d_avg_mask: DEVICE uint8[nseg] or
 * NULL (every segment averaged). Only the segments' elements of d_out are written. One asynchronous launch on `stream`:
 * no allocation, no workspace, no host synchronisation; any `clients` >= 1.
 * COALAC_EINVAL (with a coalac_last_error message): a sparse plan, bits == 32, clients < 1, a bad kind or mode, a NULL
 * pointer other than d_base / d_avg_mask, a code_bytes below the above, d_out / d_base not 16-byte aligned. A plan
 * without units returns COALAC_OK and launches nothing. The CONTENTS of the three pointer arrays live on the device and
 * cannot be checked here: every d_codes[i] must be 4-byte aligned and code_bytes long, every d_mn[i] / d_scale[i] hold
 * nseg (BLOCK: n_units) floats — the caller's duty (coala_amd/compression/plan.py aggregate_dense checks each tensor). An
 * untrusted stream can mis-decode but not make the kernel read outside [d_codes[i], d_codes[i] + code_bytes): loads are
 * range-checked to each unit's own codes or words, and padding bits are ignored. */
enum { COALAC_AGGD_CODES = 0, COALAC_AGGD_PACKED = 1, COALAC_AGGD_BLOCK = 2 };
int coalac_aggregate_dense(coalac_plan_t plan, int clients, int kind, const void* const* d_codes, uint64_t code_bytes,
                           const float* const* d_mn, const float* const* d_scale, const float* d_weights, float total,
                           int mode, const uint8_t* d_avg_mask, const float* d_base, float* d_out, void* stream);

/* Block-wise dense quantisation with 256- and 1024-element blocks (an addition to CodecSpec v1, bit for
 * bit). `block` is the block size G: 256, 1024 or 4096. With G = 4096 every entry point below gives its twin's result
 * bit for bit (coalac_encode_block, coalac_decode_block, coalac_aggregate_dense with kind COALAC_AGGD_BLOCK). `plan` is a
 * dense plan (every k == n), bits 1..8.
 *
 *   blocks       block g_s of segment s covers its elements [G g_s, min(n_s, G (g_s + 1))); blocks are numbered segment by
 *                segment in the plan's row order, ceil(n_s / G) each (an empty segment has none): NB = sum of
 *                ceil(n_s / G) — coalac_plan_block_count. The first block of segment s is gb_s = sum over t < s of
 *                ceil(n_t / G); the block of row group j of the segment's 4096-element unit u_s is gb_s + u_s (4096 / G) + j
 *   per block    exactly what coalac_encode_block does per unit: bmn the NaN-ignoring min + 0.0f, bscale CodecSpec v1's
 *                range, the code the deterministic round-to-nearest code under the block's own range, a code past a
 *                ragged block's end 0; decoded value bmn + float(code) * bscale (fp32 multiply, then add; + base)
 *   code stream  wire v4's, unchanged in layout and length; d_bmn / d_bscale: fp32[NB] (not fp32[n_units])
 *
 * The ranges are indexed from the plan, never from the payload: a block that does not exist has no range written or
 * read, and an untrusted stream can only mis-decode. coalac_encode_block_g is deterministic: there is no stochastic
 * and no error-feedback variant below 4096. Arguments are the twins', plus `block`; each call is one asynchronous launch
 * on `stream`: no allocation, no workspace, no host synchronisation. coalac_aggregate_dense_g is kind COALAC_AGGD_BLOCK
 * with every d_mn[i] / d_scale[i] holding NB floats.
 * COALAC_EINVAL (all checked before the first device call): every case the twin rejects, and a `block` other than 256,
 * 1024 or 4096; coalac_plan_block_count: a NULL plan or output, a sparse plan, bits == 32, such a `block`. A plan without
 * units returns COALAC_OK and launches nothing. */
int coalac_plan_block_count(coalac_plan_t plan, uint32_t block, uint64_t* n_blocks);
int coalac_encode_block_g(coalac_plan_t plan, uint32_t block, const float* d_in, const float* const* d_seg_in,
                          const float* d_base, float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes,
                          void* stream);
int coalac_decode_block_g(coalac_plan_t plan, uint32_t block, const void* d_packed, uint64_t packed_bytes,
                          const float* d_bmn, const float* d_bscale, const float* d_base, float* d_out, void* stream);
int coalac_aggregate_dense_g(coalac_plan_t plan, int clients, uint32_t block, const void* const* d_codes,
                             uint64_t code_bytes, const float* const* d_mn, const float* const* d_scale,
                             const float* d_weights, float total, int mode, const uint8_t* d_avg_mask,
                             const float* d_base, float* d_out, void* stream);

/* Rotated block-wise quantisation (an addition to CodecSpec v1, bit for bit; additive symbols, the ABI
 * version does not step). `plan` is a dense plan (every k == n), bits 1..8. Unit u — the u_s-th of segment s, `len`
 * elements, its first at flat position c0 = in_off_s + 4096 u_s — is
 *
 *   len < 4096   not rotated: exactly coalac_encode_block / coalac_encode_block_sr / coalac_decode_block (a ragged last
 *                unit, every small tensor). Which units are rotated is a function of the plan alone.
 *   len == 4096  a[e] = x[e] (- base[e], fp32); s[e] = a[e] with its sign bit inverted where bit 23 of the 24-bit draw of
 *                position c0 + e under `rot_seed` is set (the hash of coalac_encode_sr's contract; an XOR on the bit
 *                pattern, also of +-0, +-Inf and NaN); then for h = 1, 2, 4, ..., 2048, in this order, every pair
 *                (i, i + h) with i & h == 0 becomes (t[i] + t[i+h], t[i] - t[i+h]), all fp32, and y[e] = t[e] * 2^-6 (the
 *                orthonormal Walsh-Hadamard transform). y is quantised exactly as coalac_encode_block quantises x: bmn[u],
 *                bscale[u] from its NaN-ignoring min / max, the round-to-nearest code, or (_rot_sr) the stochastic code
 *                of coalac_encode_block_sr with the draw of position c0 + e under `seed`.
 *   decode       yq[e] = bmn[u] + float(code) * bscale[u] (multiply, then add); the same transform and * 2^-6, the same
 *                sign inversion, + base[e] when given. The transform and the signs are their own inverses, so the error of
 *                the decoded unit is the quantisation error of y, rotated.
 *   code stream  wire v4's, unchanged in layout and length; d_bmn / d_bscale: fp32[n_units]
 *
 * bmn, bscale and the stream are bit-exact against the host model for any input, non-finite values included (every
 * intermediate's class follows from IEEE add and subtract); decoded values too, except that a NaN's sign and payload are
 * not specified. A stream decoded with another rot_seed, or without the rotation, is wrong but never out of bounds.
 * Arguments, sizes, alignment and COALAC_EINVAL cases are the twins' (coalac_encode_block, coalac_encode_block_sr,
 * coalac_decode_block), all checked before the first device call; a plan without units returns COALAC_OK and launches
 * nothing. Each call is one asynchronous launch on `stream`: no allocation, no workspace, no host synchronisation. */
int coalac_encode_block_rot(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                            float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t rot_seed,
                            void* stream);
int coalac_encode_block_rot_sr(coalac_plan_t plan, const float* d_in, const float* const* d_seg_in, const float* d_base,
                               float* d_bmn, float* d_bscale, void* d_packed, uint64_t packed_bytes, uint64_t rot_seed,
                               uint64_t seed, void* stream);
int coalac_decode_block_rot(coalac_plan_t plan, const void* d_packed, uint64_t packed_bytes, const float* d_bmn,
                            const float* d_bscale, uint64_t rot_seed, const float* d_base, float* d_out, void* stream);

/* coalac_aggregate from each SPARSE upload's own buffers. `plan` is a ONE-LAYOUT sparse plan (not dense;
 * bits 1..8 or 32): d_out / d_base are indexed by its in_off. The arithmetic is coalac_aggregate's contract bit for bit
 * (x_i = base + d_i, +0.0f where client i kept nothing; acc = x_0 * w_0, acc = acc + x_i * w_i in client order, no FMA;
 * DIV | RECIP | SUM; an unmasked segment gets x_0; the forms for a -0.0f or NaN base carry over). kind says what client
 * i's entries are:
 *   COALAC_AGGS_ENTRIES  d_idx[i]: int32[total_k], d_vals[i]: uint8[total_k] codes (bits 1..8) or fp32[total_k] (bits 32)
 *                        — an upload as coalac_encode wrote it (wire v2); d_packed is ignored
 *   COALAC_AGGS_COMPACT  d_packed[i]: the wire v3 stream above (packed_bytes long each): for unit u and every entry
 *                        position j = out_off_s + e, e in the unit's clamped range [ustart[u], ustart[u + 1]) (the clamp
 *                        coalac_decode, coalac_unpack and coalac_aggregate share), the field's in-unit position is
 *                        field_j & 0xFFF and its code field_j >> 12; the field's second word is read only inside
 *                        packed_bytes. d_idx is ignored (may be NULL); d_vals[i]: fp32[total_k] at bits 32, else ignored
 * An entry whose position lies outside the unit's elements is dropped (both kinds). On any payload validate() accepts the
 * result equals coalac_unpack of every upload followed by coalac_aggregate on their concatenation.
 * d_idx, d_packed, d_vals, d_mn, d_scale, d_ustart: DEVICE arrays of `clients` device pointers, as
 * coalac_aggregate_dense takes them; d_mn[i] / d_scale[i]: fp32[nseg] (bits 32: unused, may be NULL); d_ustart[i]:
 * uint32[n_units], required. d_weights: DEVICE fp32[clients]; d_avg_mask: DEVICE uint8[nseg] or NULL. Only the segments'
 * elements of d_out are written. One asynchronous launch on `stream`: no allocation, no workspace, no host
 * synchronisation; any `clients` >= 1.
 * COALAC_EINVAL (with a coalac_last_error message): a dense plan (coalac_aggregate_dense's), clients < 1, a bad kind or
 * mode, a required array NULL, a packed_bytes below coalac_plan_packed_bytes (COMPACT), d_out / d_base not 16-byte
 * aligned. A plan without units returns COALAC_OK and launches nothing. The CONTENTS of the pointer arrays are the
 * caller's duty: every pointer 4-byte aligned and its array as long as stated (coala_amd/compression/plan.py
 * aggregate_uploads checks each tensor). An untrusted upload can mis-aggregate, but the kernel never writes outside the
 * unit's elements and never reads outside [d_packed[i], + packed_bytes), idx / vals [0, total_k), mn / scale [0, nseg) or
 * ustart [0, n_units). */
enum { COALAC_AGGS_ENTRIES = 0, COALAC_AGGS_COMPACT = 1 };
int coalac_aggregate_uploads(coalac_plan_t plan, int clients, int kind, const int32_t* const* d_idx,
                             const void* const* d_packed, uint64_t packed_bytes, const void* const* d_vals,
                             const float* const* d_mn, const float* const* d_scale, const uint32_t* const* d_ustart,
                             const float* d_weights, float total, int mode, const uint8_t* d_avg_mask,
                             const float* d_base, float* d_out, void* stream);

/* Snapshot n scalars of elem_bytes (1, 2, 4 or 8) each, read through the DEVICE pointer array d_src (each pointer
 * aligned to elem_bytes), into the contiguous d_out, in one launch on `stream`: the passthrough entries of an
 * update — BatchNorm's int64 num_batches_tracked, one per layer — that the carrier takes with the encoded tensors
 * (client compression(), coala/client/base.py:330-332; they travel raw, CodecSpec v1). */
int coalac_gather(const void* const* d_src, int n, int elem_bytes, void* d_out, void* stream);

/* Diagnostics: number of segments whose sampled thresholds were rejected and re-selected exactly in
 * the last encode that used workspace d_ws (synchronises `stream`). */
int coalac_workspace_fallbacks(coalac_plan_t plan, const void* d_ws, void* stream, int* out);

/* Diagnostics: copy up to n phase timestamps (32 per segment row: k_sample, k_ghist, k_gwin, k_select phases, 100 MHz
 * ticks; 0 = phase not reached) of the last COALAC_FLAG_STAMPS encode with d_ws to host (synchronises
 * `stream`). Returns the count copied or a negative error. */
int coalac_debug_stamps(coalac_plan_t plan, const void* d_ws, void* stream, uint64_t* host, int n);

/* Diagnostics: copy the sampled brackets {T_lo, T_hi} of the first n large units (plan order: the large segments'
 * units, segment after segment) of the last encode with d_ws to host (synchronises `stream`). T_lo carries the tie
 * flag (bit 31) of a tie-mode segment. Returns the count copied or a negative error. */
int coalac_debug_brackets(coalac_plan_t plan, const void* d_ws, void* stream, uint32_t* host_tlo, uint32_t* host_thi,
                          int n);

#ifdef __cplusplus
}
#endif

#endif /* COALAC_H */
