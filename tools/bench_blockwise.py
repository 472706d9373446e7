"""Cost of block-wise dense quantisation: one ResNet-50 global model at ratio 1, weights mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up of every shape, with the windows' min and max), per code width in --bits:

  encode_block / decode_block   the two new kernels, with their algorithmic bytes (4N + N b / 8 + 8U for the encode,
                      N b / 8 + 8U + 4N for the decode) against the 8 TB/s HBM peak
  encode / decode     this library's plain dense encode and decode (the unchanged defaults)
  parent_*            with --parent-lib (a build of the parent commit's coalac.hip), that library called through its
                      C ABI on the same buffers: its plain encode, its encode + coalac_pack_dense, its plain decode and
                      its coalac_decode_packed — what the conditions of §14 are stated against
  hooks               host wall time (time.perf_counter, synchronised) of the carrier's to_bytes() on the sender and
                      encoded_to() on the receiver, block-wise and bit-packed per-tensor, and the payload sizes

    python tools/bench_blockwise.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/blockwise_step.json]
"""
import argparse
import ctypes
import json
import os
import pickle
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
PARENT_SYMBOLS = ("coalac_plan_create", "coalac_plan_query", "coalac_encode", "coalac_decode", "coalac_pack_dense",
                  "coalac_decode_packed")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--bits", type=int, nargs="+", default=[4, 6])
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--hook-reps", type=int, default=9)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from coala_amd.compression import CodecPlan, UpdateCodec, _lib
    from coala_amd.layouts import build_module, fp32_sizes
    from coala_amd.workload import synth_batch

    dev = torch.device("cuda", 0)
    sizes = fp32_sizes(a.layout)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        """Median over the windows of the time per call (ms), and the spread (min, max)."""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(a.windows):
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            per.append(t0.elapsed_time(t1) / a.steps)
        return {"ms": round(statistics.median(per), 5), "min": round(min(per), 5), "max": round(max(per), 5)}

    def roof(r, nbytes):
        gbs = nbytes / (r["ms"] * 1e-3) / 1e9
        r.update({"alg_bytes": int(nbytes), "achieved_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_GBS, 4)})
        return r

    def parent_calls(plan, x, out, ws, flat, packed):
        """The parent commit's library on the same buffers (its own plan of the table)."""
        lib = ctypes.CDLL(a.parent_lib)
        for name, res, args in _lib.SIGNATURES:
            if name in PARENT_SYMBOLS:
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        wsb = ctypes.c_uint64()
        assert lib.coalac_plan_query(h, ctypes.byref(wsb), None, None, None) == 0 and wsb.value <= ws.numel()
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        N = ctypes.c_void_p(0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pb = ctypes.c_uint64(4 * packed.numel())

        def enc():
            assert lib.coalac_encode(h, P(x), N, N, P(out.vals), P(out.mn), P(out.scale), N, P(ws), wsb, 0, st) == 0

        def enc_pack():
            enc()
            assert lib.coalac_pack_dense(h, P(out.vals), P(packed), pb, st) == 0

        def dec():
            assert lib.coalac_decode(h, N, P(out.vals), P(out.mn), P(out.scale), N, N, P(flat), st) == 0

        def dec_packed():
            assert lib.coalac_decode_packed(h, P(packed), pb, P(out.mn), P(out.scale), N, P(flat), st) == 0
        return enc, enc_pack, dec, dec_packed

    def overlap(x, y):
        return not (x["max"] < y["min"] or y["max"] < x["min"])

    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        ws, out, flat = plan.empty_workspace(), plan.empty_encoded(), plan.empty_flat()
        plan.encode(x, out=out, workspace=ws)
        packed = plan.pack_dense(out)
        blk = plan.empty_block_encoded()
        plan.encode_block(flat=x, out=blk)
        N, U, Pw = int(plan.total_k), int(plan.n_units), int(plan.dense_packed_words)
        r.update({"elements": N, "blocks": U, "packed_bytes": 4 * Pw, "range_bytes": 8 * U})
        r["encode_block"] = roof(window(lambda: plan.encode_block(flat=x, out=blk)), 4 * N + 4 * Pw + 8 * U)
        r["decode_block"] = roof(window(lambda: plan.decode_block(blk[2], blk[0], blk[1], out=flat)), 4 * Pw + 8 * U + 4 * N)
        r["encode"] = window(lambda: plan.encode(x, out=out, workspace=ws))
        r["decode"] = window(lambda: plan.decode(out, out=flat))
        if a.parent_lib:
            enc, enc_pack, dec, dec_packed = parent_calls(plan, x, out, ws, flat, packed)
            r["parent_encode"] = window(enc)
            r["parent_encode_pack"] = window(enc_pack)
            r["parent_decode"] = window(dec)
            r["parent_decode_packed"] = window(dec_packed)
            # once more, interleaved after the parent's: the run-to-run spread of the same kernels
            r["encode_block_again"] = window(lambda: plan.encode_block(flat=x, out=blk))
            r["decode_block_again"] = window(lambda: plan.decode_block(blk[2], blk[0], blk[1], out=flat))
            r["encode_again"] = window(lambda: plan.encode(x, out=out, workspace=ws))
            r["decode_again"] = window(lambda: plan.decode(out, out=flat))
            eb, pe, pep = r["encode_block"], r["parent_encode"], r["parent_encode_pack"]
            db, pdp = r["decode_block"], r["parent_decode_packed"]
            r["encode_block_over_parent_encode_pack"] = round(eb["ms"] / pep["ms"], 3)
            r["encode_block_over_parent_encode"] = round(eb["ms"] / pe["ms"], 3)
            r["decode_block_over_parent_decode_packed"] = round(db["ms"] / pdp["ms"], 3)
            r["conditions"] = {
                "encode_faster_than_parent_encode_pack_windows_disjoint": eb["max"] < pep["min"],
                "encode_below_parent_plain_encode": eb["ms"] < pe["ms"],
                "decode_within_parent_decode_packed_spread_plus_5pct": db["ms"] <= pdp["max"] * 1.05,
                "plain_encode_windows_overlap_parent": overlap(r["encode"], pe) or overlap(r["encode_again"], pe),
                "plain_decode_windows_overlap_parent": overlap(r["decode"], r["parent_decode"])
                or overlap(r["decode_again"], r["parent_decode"])}
        # the hooks: sender to_bytes() (D2H + blob), receiver encoded_to() (H2D of the payload's arrays)
        model = build_module(a.layout, seed=1).to(dev)
        hooks = r["hooks"] = {}
        for name, kw in (("blockwise", {"blockwise": True}), ("packed", {"pack_dense": True})):
            if name == "packed" and bits >= 8:
                continue
            codec = UpdateCodec(1.0, bits, "weights", **kw)
            tb, et, up = [], [], None
            for _ in range(a.hook_reps):
                up = codec.encode_module(model)
                torch.cuda.synchronize()
                s = time.perf_counter()
                blob = up.to_bytes()
                tb.append((time.perf_counter() - s) * 1e3)
            back = pickle.loads(pickle.dumps(up))
            cplan = codec.plan_for(tuple(sizes), dev, ratio=1.0, bits=bits)
            for _ in range(a.hook_reps):
                torch.cuda.synchronize()
                s = time.perf_counter()
                back.encoded_to(dev, staging=codec._staging, plan=cplan)
                torch.cuda.synchronize()
                et.append((time.perf_counter() - s) * 1e3)
                codec._staged(torch.cuda.current_stream(dev))
            hooks[name] = {"to_bytes_ms": round(statistics.median(tb), 4), "encoded_to_ms": round(statistics.median(et), 4),
                           "nbytes": int(up.nbytes), "blob_bytes": len(blob)}
    doc = {"what": "block-wise dense quantisation: coalac_encode_block / coalac_decode_block beside the parent "
                   "library's encode (+ pack_dense) and decode_packed, the unchanged plain encode / decode, the hooks",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": 1.0, "mode": "weights",
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the "
                     f"windows' spread); hooks: host wall time, median of {a.hook_reps}",
           "hbm_peak_GBs": HBM_GBS, "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
