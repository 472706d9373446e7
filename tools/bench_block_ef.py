"""Cost of error feedback for block-wise uploads: one ResNet-50 update at ratio 1, delta mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up, with the windows' min and max), per code width in --bits:

  (a) encode_block                 the block-wise encode alone (no error feedback)
  (b) encode_block_ef              the fused call: encode and residual update in one launch
  (c) composed                     the same round from the calls that existed before: ef_accumulate, encode_block of
                                   the residual, decode_block to a temporary, torch subtract
  (d) --nt-lib                     a build of this source with BLOCK_EF_STORE_AUX = 2 (tools/build_variant.sh NAME
                                   -DBLOCK_EF_STORE_AUX=2): its encode_block_ef through the C ABI on the same buffers,
                                   interleaved with this build's (each side twice) — the store-policy A/B
  --parent-lib                     a build of the parent commit's coalac.hip: its encode_block on the same buffers,
                                   interleaved with this build's (each side twice): it must not have moved

(the residual of (b), (c) and (d) is zeroed before every window, so no run drifts into non-finite values)

    python tools/bench_block_ef.py [--parent-lib PATH] [--nt-lib PATH] [--out profiles/block_ef_step.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OTHER_SYMBOLS = ("coalac_plan_create", "coalac_encode_block", "coalac_encode_block_ef")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--bits", type=int, nargs="+", default=[2, 4, 8])
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--nt-lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from coala_amd.compression import CodecPlan, _lib
    from coala_amd.layouts import fp32_sizes
    from coala_amd.workload import synth_batch

    dev = torch.device("cuda", 0)
    sizes = fp32_sizes(a.layout)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn, before=None):
        """Median over the windows of the time per call (ms), and the spread (min, max)."""
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(a.windows):
            if before is not None:
                before()
            t0.record()
            for _ in range(a.steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            per.append(t0.elapsed_time(t1) / a.steps)
        return {"ms": round(statistics.median(per), 5), "min": round(min(per), 5), "max": round(max(per), 5)}

    def other_library(path, plan):
        """Another build of the library (its own plan of the table) -> (lib, plan handle)."""
        lib = ctypes.CDLL(path)
        for name, res, args in _lib.SIGNATURES:
            if name in OTHER_SYMBOLS and hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        return lib, h

    def overlap(x, y):
        return not (x["max"] < y["min"] or y["max"] < x["min"])

    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    N = ctypes.c_void_p(0)
    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        base = synth_batch(plan.table, dev, client_ids=[1])
        resid = torch.zeros(plan.span, device=dev)
        tmp = torch.zeros(plan.span, device=dev)
        blk = plan.empty_block_encoded()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pb = ctypes.c_uint64(4 * blk[2].numel())
        r.update({"elements": int(plan.total_k), "blocks": int(plan.n_units)})
        zero = lambda: resid.zero_()  # noqa: E731
        enc_block = lambda: plan.encode_block(flat=x, base=base, out=blk)  # noqa: E731
        enc_ef = lambda: plan.encode_block_ef(resid, flat=x, base=base, out=blk)  # noqa: E731

        def composed():
            plan.ef_accumulate(resid, flat=x, base=base)
            plan.encode_block(flat=resid, out=blk)
            plan.decode_block(blk[2], blk[0], blk[1], out=tmp)
            resid.sub_(tmp)
        for tag in ("", "_again"):
            r["encode_block" + tag] = window(enc_block)
            r["encode_block_ef" + tag] = window(enc_ef, zero)
            r["composed" + tag] = window(composed, zero)
        best = lambda name: min(r[name]["ms"], r[name + "_again"]["ms"])  # noqa: E731
        spread = lambda name: abs(r[name]["ms"] - r[name + "_again"]["ms"]) / best(name)  # noqa: E731
        r["ef_over_encode_block"] = round(best("encode_block_ef") / best("encode_block"), 3)
        r["composed_over_ef"] = round(best("composed") / best("encode_block_ef"), 3)
        r["pass_to_pass_spread"] = {k: round(spread(k), 4) for k in ("encode_block", "encode_block_ef", "composed")}
        if a.nt_lib:
            lib, h = other_library(a.nt_lib, plan)

            def nt_ef():
                assert lib.coalac_encode_block_ef(h, P(x), N, P(base), P(resid), P(blk[0]), P(blk[1]), P(blk[2]), pb, st) == 0
            r["nt_ef"], r["ab_plain_ef"] = window(nt_ef, zero), window(enc_ef, zero)
            r["nt_ef_again"], r["ab_plain_ef_again"] = window(nt_ef, zero), window(enc_ef, zero)
            r["nt_over_plain_stores"] = round(statistics.median([r["nt_ef"]["ms"], r["nt_ef_again"]["ms"]])
                                              / statistics.median([r["ab_plain_ef"]["ms"], r["ab_plain_ef_again"]["ms"]]), 3)
            r["nt_windows_overlap_plain"] = any(overlap(m, t) for m in (r["ab_plain_ef"], r["ab_plain_ef_again"])
                                                for t in (r["nt_ef"], r["nt_ef_again"]))
        if a.parent_lib:
            lib, h = other_library(a.parent_lib, plan)

            def parent_block():
                assert lib.coalac_encode_block(h, P(x), N, P(base), P(blk[0]), P(blk[1]), P(blk[2]), pb, st) == 0
            r["parent_encode_block"], r["ab_encode_block"] = window(parent_block), window(enc_block)
            r["parent_encode_block_again"], r["ab_encode_block_again"] = window(parent_block), window(enc_block)
            mine = [r["ab_encode_block"], r["ab_encode_block_again"]]
            theirs = [r["parent_encode_block"], r["parent_encode_block_again"]]
            r["encode_block_over_parent"] = round(statistics.median(m["ms"] for m in mine)
                                                  / statistics.median(t["ms"] for t in theirs), 4)
            # the yardstick: how far two passes of ONE library lie apart in this run
            same = lambda ws: abs(ws[0]["ms"] - ws[1]["ms"]) / min(w["ms"] for w in ws)  # noqa: E731
            r["same_library_pass_spread"] = round(max(same(mine), same(theirs)), 4)
            r["encode_block_windows_overlap_parent"] = any(overlap(m, t) for m in mine for t in theirs)
    doc = {"what": "error feedback for block-wise uploads: coalac_encode_block_ef beside encode_block alone, beside the "
                   "same round composed from the earlier calls, with non-temporal residual stores, and encode_block "
                   "beside the parent commit's library",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": 1.0, "mode": "delta",
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "nt_library": os.path.basename(a.nt_lib) if a.nt_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the "
                     "windows' spread)", "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
