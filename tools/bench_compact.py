"""Cost and gain of the compact upload payload: ResNet-50 updates, ratio 0.01, delta mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each,
after a warm-up of every shape), per code width in --bits:

  k_pack / k_unpack   each kernel alone, for one update and for a --clients batch, with its algorithmic bytes
                      (pack reads idx + codes and writes the stream; unpack reads the stream and the starts and
                      writes idx + codes) against the 8 TB/s HBM peak
  encode / encode+pack  the plain encode and the encode followed by the pack on the same stream; with --parent-lib
                      (a build of the parent commit's coalac.hip) also the plain encode of that library, called
                      through its C ABI directly (the encode entry point is the same in both)
  hooks               host wall time (time.perf_counter, synchronised) of the carrier's to_bytes() on the client and
                      encoded_to() on the server, with and without compact, and the payload sizes

    python tools/bench_compact.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/compact_step.json]
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
    p.add_argument("--ratio", type=float, default=0.01)
    p.add_argument("--bits", type=int, nargs="+", default=[8, 4])
    p.add_argument("--clients", type=int, default=16)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--hook-reps", type=int, default=15)
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

    def parent_encode(plan, x, base, out, ws):
        """The plain encode of the parent commit's library on the same buffers (its own plan of the same table)."""
        lib = ctypes.CDLL(a.parent_lib)
        for name, res, args in _lib.SIGNATURES:
            if name in ("coalac_plan_create", "coalac_encode", "coalac_plan_query"):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        wsb = ctypes.c_uint64()
        assert lib.coalac_plan_query(h, ctypes.byref(wsb), None, None, None) == 0 and wsb.value <= ws.numel()
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def run():
            rc = lib.coalac_encode(h, P(x), P(base), P(out.idx), P(out.vals), P(out.mn), P(out.scale), P(out.ustart),
                                   P(ws), wsb, 0, st)
            assert rc == 0
        return run

    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        vb = 4 if bits == 32 else 1
        for C in (1, a.clients):
            plan = CodecPlan(sizes, a.ratio, bits, clients=C, device=dev)
            x = synth_batch(plan.table, dev, client_ids=list(range(C)))
            base = synth_batch(plan.table, dev, client_ids=[999] * C)
            ws, out = plan.empty_workspace(), plan.empty_encoded()
            plan.encode(x, base=base, out=out, workspace=ws)
            packed = plan.pack(out)
            idx2, vals2 = plan.unpack(packed, out.ustart)
            same = bool(torch.equal(idx2, out.idx) and (bits == 32 or torch.equal(vals2, out.vals)))
            K, U, Pw = int(plan.total_k), int(plan.n_units), int(plan.packed_words)
            codes = 0 if bits == 32 else K
            c = r[f"clients{C}"] = {"entries": K, "units": U, "packed_bytes": 4 * Pw, "idx_vals_bytes": (4 + vb) * K,
                                    "round_trip_equal": same}
            c["k_pack"] = roof(window(lambda: plan.pack(out, out=packed)), 4 * K + codes + 4 * Pw)
            c["k_unpack"] = roof(window(lambda: plan.unpack(packed, out.ustart, out=(idx2, vals2))),
                                 4 * Pw + (32 + 4) * U + 4 * K + codes)
            c["encode"] = window(lambda: plan.encode(x, base=base, out=out, workspace=ws))

            def enc_pack():
                plan.encode(x, base=base, out=out, workspace=ws)
                plan.pack(out, out=packed)
            c["encode_pack"] = window(enc_pack)
            c["pack_over_encode"] = round(c["encode_pack"]["ms"] / c["encode"]["ms"], 3)
            if a.parent_lib:
                c["parent_encode"] = window(parent_encode(plan, x, base, out, ws))
                c["encode_pack_over_parent_encode"] = round(c["encode_pack"]["ms"] / c["parent_encode"]["ms"], 3)
        # the hooks: client to_bytes() (D2H + blob), server encoded_to() (pinned H2D [+ unpack])
        trained, glob = build_module(a.layout, seed=1).to(dev), build_module(a.layout, seed=2).to(dev)
        hooks = r["hooks"] = {}
        for compact in (False, True):
            codec = UpdateCodec(a.ratio, bits, "delta", compact=compact)
            snap = codec.snapshot(glob)
            tb, et, up = [], [], None
            for _ in range(a.hook_reps):
                up = codec.encode_module(trained, base=snap)
                torch.cuda.synchronize()
                s = time.perf_counter()
                blob = up.to_bytes()
                tb.append((time.perf_counter() - s) * 1e3)
            back = pickle.loads(pickle.dumps(up))
            plan = codec.plan_for(tuple(sizes), dev, ratio=a.ratio, bits=bits)
            for _ in range(a.hook_reps):
                torch.cuda.synchronize()
                s = time.perf_counter()
                back.encoded_to(dev, staging=codec._staging, plan=plan)
                torch.cuda.synchronize()
                et.append((time.perf_counter() - s) * 1e3)
                codec._staged(torch.cuda.current_stream(dev))
            hooks["compact" if compact else "plain"] = {
                "to_bytes_ms": round(statistics.median(tb), 4), "encoded_to_ms": round(statistics.median(et), 4),
                "nbytes": int(up.nbytes), "blob_bytes": len(blob)}
        hooks["nbytes_ratio"] = round(hooks["compact"]["nbytes"] / hooks["plain"]["nbytes"], 4)
    doc = {"what": "compact upload payload: k_pack / k_unpack, encode + pack vs encode, and the hooks' copies",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": a.ratio, "mode": "delta",
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
