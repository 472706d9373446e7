"""Cost of block-wise dense quantisation with 256- and 1024-element blocks: one ResNet-50 update at
ratio 1, weights mode, and 16 uploads of it for the aggregate.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after a
warm-up of every shape, with the windows' min and max), per code width in --bits:

  encode_block_g / decode_block_g / aggregate_dense_g   at G = 256 and 1024, beside the 4096 paths of the same build
                      (encode_block / decode_block / aggregate_dense kind "block"), each with its algorithmic bytes —
                      4 + b / 8 + 8 / G per element on the encode — against the 8 TB/s HBM peak, and its ratio to 4096
  unchanged_vs_parent with --parent-lib (a build of the parent commit's coalac.hip): coalac_encode_block,
                      coalac_decode_block and coalac_aggregate_dense (BLOCK) of this build and of that library, both
                      called through the C ABI on the same buffers, interleaved (this, parent, this, parent): the unchanged
                      paths are expected to lie inside the parent's own run-to-run spread; the spread and the ratio are
                      reported, whatever they are

    python tools/bench_subblock.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/subblock_step.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
PARENT_SYMBOLS = ("coalac_plan_create", "coalac_encode_block", "coalac_decode_block", "coalac_aggregate_dense")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--bits", type=int, nargs="+", default=[2, 4])
    p.add_argument("--blocks", type=int, nargs="+", default=[256, 1024])
    p.add_argument("--clients", type=int, default=16)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from coala_amd.compression import CodecPlan, _lib
    from coala_amd.layouts import fp32_sizes
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

    def overlap(x, y):
        return not (x["max"] < y["min"] or y["max"] < x["min"])

    def abi_calls(path, plan, x, blk, flat, table, w, C):
        """The library at `path` called through its C ABI on the same buffers (its own plan of the table): the parent
        commit's, and this build's the same way, so that both sides of the comparison pay the same host time."""
        lib = ctypes.CDLL(path)
        for name, res, args in _lib.SIGNATURES:
            if name in PARENT_SYMBOLS:
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        N = ctypes.c_void_p(0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pb = ctypes.c_uint64(4 * blk[2].numel())
        tp = table.data_ptr()

        def enc():
            assert lib.coalac_encode_block(h, P(x), N, N, P(blk[0]), P(blk[1]), P(blk[2]), pb, st) == 0

        def dec():
            assert lib.coalac_decode_block(h, P(blk[2]), pb, P(blk[0]), P(blk[1]), N, P(flat), st) == 0

        def agg():
            assert lib.coalac_aggregate_dense(h, C, _lib.COALAC_AGGD_BLOCK, ctypes.c_void_p(tp), pb,
                                              ctypes.c_void_p(tp + 8 * C), ctypes.c_void_p(tp + 16 * C), P(w),
                                              ctypes.c_float(float(C)), _lib.COALAC_AGG_RECIP, N, N, P(flat), st) == 0
        return enc, dec, agg

    res = {}
    C = a.clients
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        flat = plan.empty_flat()
        N, Pw = int(plan.total_k), int(plan.dense_packed_words)
        weights = [1] * C
        r.update({"elements": N, "packed_bytes": 4 * Pw, "clients": C})
        ups = {}
        for G in [4096] + list(a.blocks):
            NB = plan.block_count(G)
            # C uploads: the same update scaled per client (distinct ranges and codes)
            ups[G] = [plan.encode_block_g(G, flat=x * (1.0 + 0.01 * c)) for c in range(C)]
            blk = ups[G][0]
            g = r[f"G{G}"] = {"blocks": NB, "range_bytes": 8 * NB,
                              "payload_bytes_per_element": round((4 * Pw + 8 * NB) / N, 4)}
            g["encode"] = roof(window(lambda: plan.encode_block_g(G, flat=x, out=blk)), 4 * N + 4 * Pw + 8 * NB)
            g["decode"] = roof(window(lambda: plan.decode_block_g(G, blk[2], blk[0], blk[1], out=flat)),
                               4 * Pw + 8 * NB + 4 * N)
            cs, ms, ss = ([u[i] for u in ups[G]] for i in (2, 0, 1))
            g["aggregate"] = roof(window(lambda: plan.aggregate_dense_g(G, cs, ms, ss, weights, out=flat)),
                                  C * (4 * Pw + 8 * NB) + 4 * N)
        for G in a.blocks:
            for what in ("encode", "decode", "aggregate"):
                r[f"G{G}"][f"{what}_over_4096"] = round(r[f"G{G}"][what]["ms"] / r["G4096"][what]["ms"], 3)
        if a.parent_lib:
            blk = ups[4096][0]
            cs, ms, ss = ([u[i] for u in ups[4096]] for i in (2, 0, 1))
            table = torch.tensor([t.data_ptr() for ts in (cs, ms, ss) for t in ts], dtype=torch.int64).to(dev)
            w = torch.ones(C, dtype=torch.float32, device=dev)
            names = ("encode", "decode", "aggregate")
            mine = dict(zip(names, abi_calls(_lib.lib_path(), plan, x, blk, flat, table, w, C)))
            theirs = dict(zip(names, abi_calls(a.parent_lib, plan, x, blk, flat, table, w, C)))
            ab = r["unchanged_vs_parent"] = {}
            for what in ("encode", "decode", "aggregate"):
                # interleaved: this build, the parent, this build, the parent
                runs = [window(f) for f in (mine[what], theirs[what], mine[what], theirs[what])]
                lo, hi = min(runs[1]["min"], runs[3]["min"]), max(runs[1]["max"], runs[3]["max"])
                med = statistics.median([runs[0]["ms"], runs[2]["ms"]])
                pmed = statistics.median([runs[1]["ms"], runs[3]["ms"]])
                ab[what] = {"this": [runs[0], runs[2]], "parent": [runs[1], runs[3]],
                            "parent_spread": [lo, hi], "ratio_to_parent": round(med / pmed, 4),
                            "inside_parent_spread": lo <= med <= hi,
                            "windows_overlap": overlap(runs[0], runs[1]) or overlap(runs[2], runs[3])}
    doc = {"what": "block-wise dense quantisation with 256- and 1024-element blocks: coalac_encode_block_g / "
                   "coalac_decode_block_g / coalac_aggregate_dense_g beside the 4096 paths of the same build, and the "
                   "unchanged 4096 entry points interleaved with the parent library's",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": 1.0, "mode": "weights", "clients": C,
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the "
                     "windows' spread)",
           "hbm_peak_GBs": HBM_GBS, "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
