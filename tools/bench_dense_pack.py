"""Cost and gain of the bit-packed dense codes: one ResNet-50 global model at ratio 1, weights mode —
the download direction's payload.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each,
after a warm-up of every shape), per code width in --bits:

  k_pack_dense / k_unpack_dense   each kernel alone, with its algorithmic bytes (the uint8 codes on one side, the
                      stream on the other) against the 8 TB/s HBM peak
  decode_packed       the dense decode reading the stream (k_dense_deq_stream), and unpack_dense followed by the
                      plain decode, which writes and re-reads one byte per element in between
  encode / decode     the plain dense encode and decode; with --parent-lib (a build of the parent commit's
                      coalac.hip) also those of that library, called through its C ABI directly on the same buffers
                      (the entry points are the same in both)
  encode_pack         the encode followed by the pack on the same stream
  hooks               host wall time (time.perf_counter, synchronised) of the carrier's to_bytes() on the sender and
                      encoded_to() on the receiver, plain and packed, and the payload sizes

    python tools/bench_dense_pack.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/dense_pack_step.json]
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

    def parent_calls(plan, x, out, ws, flat):
        """The plain encode and decode of the parent commit's library on the same buffers (its own plan of the table)."""
        lib = ctypes.CDLL(a.parent_lib)
        for name, res, args in _lib.SIGNATURES:
            if name in ("coalac_plan_create", "coalac_encode", "coalac_decode", "coalac_plan_query"):
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

        def enc():
            assert lib.coalac_encode(h, P(x), N, N, P(out.vals), P(out.mn), P(out.scale), N, P(ws), wsb, 0, st) == 0

        def dec():
            assert lib.coalac_decode(h, N, P(out.vals), P(out.mn), P(out.scale), N, N, P(flat), st) == 0
        return enc, dec

    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        ws, out, flat = plan.empty_workspace(), plan.empty_encoded(), plan.empty_flat()
        plan.encode(x, out=out, workspace=ws)
        packed = plan.pack_dense(out)
        vals2 = plan.unpack_dense(packed)
        a1 = plan.decode(out).clone()
        a2 = plan.decode_packed(packed, out.mn, out.scale)
        N, Pw = int(plan.total_k), int(plan.dense_packed_words)
        r.update({"elements": N, "codes_bytes": N, "packed_bytes": 4 * Pw,
                  "round_trip_equal": bool(torch.equal(vals2, out.vals)),
                  "decode_packed_equal": bool(torch.equal(a1.view(torch.int32), a2.view(torch.int32)))})
        r["k_pack_dense"] = roof(window(lambda: plan.pack_dense(out, out=packed)), N + 4 * Pw)
        r["k_unpack_dense"] = roof(window(lambda: plan.unpack_dense(packed, out=vals2)), N + 4 * Pw)
        r["decode_packed"] = roof(window(lambda: plan.decode_packed(packed, out.mn, out.scale, out=flat)), 4 * Pw + 4 * N)

        def unpack_decode():
            plan.unpack_dense(packed, out=vals2)
            plan.decode(out, out=flat)
        r["unpack_then_decode"] = window(unpack_decode)
        r["encode"] = roof(window(lambda: plan.encode(x, out=out, workspace=ws)), 8 * N + N)
        r["decode"] = roof(window(lambda: plan.decode(out, out=flat)), N + 4 * N)

        def enc_pack():
            plan.encode(x, out=out, workspace=ws)
            plan.pack_dense(out, out=packed)
        r["encode_pack"] = window(enc_pack)
        r["pack_over_encode"] = round(r["encode_pack"]["ms"] / r["encode"]["ms"], 3)
        r["decode_packed_over_decode"] = round(r["decode_packed"]["ms"] / r["decode"]["ms"], 3)
        if a.parent_lib:
            enc, dec = parent_calls(plan, x, out, ws, flat)
            r["parent_encode"] = window(enc)
            r["parent_decode"] = window(dec)
            # once more, interleaved after the parent's: the run-to-run spread of the same library
            r["encode_again"] = window(lambda: plan.encode(x, out=out, workspace=ws))
            r["decode_again"] = window(lambda: plan.decode(out, out=flat))
            r["decode_packed_over_parent_decode"] = round(r["decode_packed"]["ms"] / r["parent_decode"]["ms"], 3)
        # the hooks: sender to_bytes() (D2H + blob), receiver encoded_to() (H2D of the payload's arrays)
        model = build_module(a.layout, seed=1).to(dev)
        hooks = r["hooks"] = {}
        for pack in (False, True):
            codec = UpdateCodec(1.0, bits, "weights", pack_dense=pack)
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
            hooks["packed" if pack else "plain"] = {
                "to_bytes_ms": round(statistics.median(tb), 4), "encoded_to_ms": round(statistics.median(et), 4),
                "nbytes": int(up.nbytes), "blob_bytes": len(blob)}
        hooks["nbytes_ratio"] = round(hooks["packed"]["nbytes"] / hooks["plain"]["nbytes"], 4)
    doc = {"what": "bit-packed dense codes: k_pack_dense / k_unpack_dense / decode_packed, the plain dense encode and "
                   "decode beside the parent library's, and the hooks' copies",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": 1.0, "mode": "weights",
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls; hooks: host wall "
                     f"time, median of {a.hook_reps}",
           "hbm_peak_GBs": HBM_GBS, "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
