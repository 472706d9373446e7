"""Cost of stochastic rounding in the dense quantisers: one ResNet-50 update at ratio 1, weights mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up, with the windows' min and max), per code width in --bits:

  encode_sr / encode              the stochastic per-tensor encode beside this library's deterministic one
  encode_block_sr / encode_block  the same for the block-wise encode
  parent_encode / parent_encode_block
                                  with --parent-lib (a build of the parent commit's coalac.hip; COALAC_LIB names the same
                                  kind of library for the whole binding), that library's deterministic encodes through
                                  its C ABI on the same buffers, interleaved A/B with this build's (each side twice):
                                  the deterministic instantiations must not have moved

    python tools/bench_sr.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/sr_step.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_SYMBOLS = ("coalac_plan_create", "coalac_plan_query", "coalac_encode", "coalac_encode_block")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--bits", type=int, nargs="+", default=[4, 8])
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

    def parent_calls(plan, x, out, ws, blk):
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
        pb = ctypes.c_uint64(4 * blk[2].numel())

        def enc():
            assert lib.coalac_encode(h, P(x), N, N, P(out.vals), P(out.mn), P(out.scale), N, P(ws), wsb, 0, st) == 0

        def enc_block():
            assert lib.coalac_encode_block(h, P(x), N, N, P(blk[0]), P(blk[1]), P(blk[2]), pb, st) == 0
        return enc, enc_block

    def overlap(x, y):
        return not (x["max"] < y["min"] or y["max"] < x["min"])

    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        ws, out, blk = plan.empty_workspace(), plan.empty_encoded(with_idx=False), plan.empty_block_encoded()
        r.update({"elements": int(plan.total_k), "blocks": int(plan.n_units)})
        seed = [0x5EED]

        def enc_sr():
            seed[0] += 1
            plan.encode_sr(flat=x, seed=seed[0], out=out, workspace=ws)

        def enc_block_sr():
            seed[0] += 1
            plan.encode_block_sr(flat=x, seed=seed[0], out=blk)
        enc = lambda: plan.encode(x, out=out, workspace=ws)  # noqa: E731
        enc_block = lambda: plan.encode_block(flat=x, out=blk)  # noqa: E731
        r["encode"], r["encode_sr"] = window(enc), window(enc_sr)
        r["encode_block"], r["encode_block_sr"] = window(enc_block), window(enc_block_sr)
        r["encode_again"], r["encode_sr_again"] = window(enc), window(enc_sr)
        r["encode_block_again"], r["encode_block_sr_again"] = window(enc_block), window(enc_block_sr)
        r["encode_sr_over_encode"] = round(min(r["encode_sr"]["ms"], r["encode_sr_again"]["ms"])
                                           / min(r["encode"]["ms"], r["encode_again"]["ms"]), 3)
        r["encode_block_sr_over_encode_block"] = round(
            min(r["encode_block_sr"]["ms"], r["encode_block_sr_again"]["ms"])
            / min(r["encode_block"]["ms"], r["encode_block_again"]["ms"]), 3)
        if a.parent_lib:
            penc, penc_block = parent_calls(plan, x, out, ws, blk)
            # interleaved A/B, each side twice: parent, this build, parent, this build
            r["parent_encode"], r["ab_encode"] = window(penc), window(enc)
            r["parent_encode_again"], r["ab_encode_again"] = window(penc), window(enc)
            r["parent_encode_block"], r["ab_encode_block"] = window(penc_block), window(enc_block)
            r["parent_encode_block_again"], r["ab_encode_block_again"] = window(penc_block), window(enc_block)
            for name in ("encode", "encode_block"):
                mine = [r[f"ab_{name}"], r[f"ab_{name}_again"], r[name], r[f"{name}_again"]]
                theirs = [r[f"parent_{name}"], r[f"parent_{name}_again"]]
                r[f"{name}_over_parent"] = round(statistics.median(m["ms"] for m in mine[:2])
                                                 / statistics.median(t["ms"] for t in theirs), 3)
                r[f"{name}_windows_overlap_parent"] = any(overlap(m, t) for m in mine for t in theirs)
    doc = {"what": "stochastic rounding: coalac_encode_sr / coalac_encode_block_sr beside the deterministic encodes of "
                   "this build and of the parent commit's library",
           "layout": a.layout, "elements": int(sum(sizes)), "ratio": 1.0, "mode": "weights",
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the "
                     "windows' spread)", "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
