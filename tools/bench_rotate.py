"""Cost of the rotation in the block-wise quantisers: one ResNet-50 update at ratio 1, weights mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up, with the windows' min and max), per code width in --bits:

  encode_block_rot / encode_block          the rotated round-to-nearest encode beside this library's unrotated one
  encode_block_rot_sr / encode_block_sr    the same with stochastic rounding
  decode_block_rot / decode_block          the rotated decode beside the unrotated one
  parent_encode_block / parent_encode_block_sr / parent_decode_block
                                           with --parent-lib (a build of the parent commit's coalac.hip), that library's
                                           entry points and this build's, both through the C ABI on the same buffers,
                                           interleaved (this, parent, this, parent): the unchanged entry points must lie
                                           inside the parent's own [min, max] window spread

    python tools/bench_rotate.py [--layout resnet50_tv] [--parent-lib PATH] [--out profiles/rotate_step.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_SYMBOLS = ("coalac_plan_create", "coalac_encode_block", "coalac_encode_block_sr", "coalac_decode_block")
TWINS = (("encode_block_rot", "encode_block"), ("encode_block_rot_sr", "encode_block_sr"),
         ("decode_block_rot", "decode_block"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--bits", type=int, nargs="+", default=[2, 4])
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

    def raw_calls(path, plan, x, blk, out):
        """The unchanged entry points of the library at `path` through its C ABI, on the same buffers (its own plan of
        the table): the parent's library and this build's are called the same way, so the host cost per call is equal."""
        lib = ctypes.CDLL(path)
        for name, res, args in _lib.SIGNATURES:
            if name in PARENT_SYMBOLS:
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        N = ctypes.c_void_p(0)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        pb = ctypes.c_uint64(4 * blk[2].numel())

        def enc():
            assert lib.coalac_encode_block(h, P(x), N, N, P(blk[0]), P(blk[1]), P(blk[2]), pb, st) == 0

        def enc_sr():
            assert lib.coalac_encode_block_sr(h, P(x), N, N, P(blk[0]), P(blk[1]), P(blk[2]), pb,
                                              ctypes.c_uint64(0x5EED), st) == 0

        def dec():
            assert lib.coalac_decode_block(h, P(blk[2]), pb, P(blk[0]), P(blk[1]), N, P(out), st) == 0
        return {"encode_block": enc, "encode_block_sr": enc_sr, "decode_block": dec}

    res = {}
    for bits in a.bits:
        r = res[f"bits{bits}"] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        x = synth_batch(plan.table, dev, client_ids=[0])
        blk, rot, out = plan.empty_block_encoded(), plan.empty_block_encoded(), plan.empty_flat()
        full = int(sum(n // 4096 for n in sizes))
        r.update({"elements": int(plan.total_k), "blocks": int(plan.n_units), "rotated_blocks": full})
        seed = [0x5EED]

        def bump():
            seed[0] += 1
            return seed[0]
        plan.encode_block(flat=x, out=blk)
        plan.encode_block_rot(flat=x, rot_seed=7, out=rot)
        calls = {
            "encode_block": lambda: plan.encode_block(flat=x, out=blk),
            "encode_block_sr": lambda: plan.encode_block_sr(flat=x, seed=bump(), out=blk),
            "decode_block": lambda: plan.decode_block(blk[2], blk[0], blk[1], out=out),
            "encode_block_rot": lambda: plan.encode_block_rot(flat=x, rot_seed=bump(), out=rot),
            "encode_block_rot_sr": lambda: plan.encode_block_rot(flat=x, rot_seed=bump(), seed=bump(), out=rot),
            "decode_block_rot": lambda: plan.decode_block_rot(rot[2], rot[0], rot[1], 7, out=out),
        }
        for new, old in TWINS:  # twin, rotated, twin, rotated
            r[old], r[new] = window(calls[old]), window(calls[new])
            r[old + "_again"], r[new + "_again"] = window(calls[old]), window(calls[new])
            r[f"{new}_over_{old}"] = round(min(r[new]["ms"], r[new + "_again"]["ms"])
                                           / min(r[old]["ms"], r[old + "_again"]["ms"]), 3)
            # bytes the call moves (input or output fp32, the stream, the ranges) over its time: against HBM's rate
            moved = 4 * plan.total_k + 4 * plan.dense_packed_words + 8 * plan.n_units
            r[new + "_gb_per_s"] = round(moved / min(r[new]["ms"], r[new + "_again"]["ms"]) / 1e6, 1)
            r[old + "_gb_per_s"] = round(moved / min(r[old]["ms"], r[old + "_again"]["ms"]) / 1e6, 1)
        if a.parent_lib:
            parent = raw_calls(a.parent_lib, plan, x, blk, out)
            this = raw_calls(_lib.lib_path(), plan, x, blk, out)
            for _, name in TWINS:  # interleaved A/B, each side twice: this, parent, this, parent
                r["ab_" + name], r["parent_" + name] = window(this[name]), window(parent[name])
                r["ab_" + name + "_again"], r["parent_" + name + "_again"] = window(this[name]), window(parent[name])
                mine = [r["ab_" + name], r["ab_" + name + "_again"]]
                theirs = [r["parent_" + name], r["parent_" + name + "_again"]]
                lo, hi = min(t["min"] for t in theirs), max(t["max"] for t in theirs)
                r[name + "_over_parent"] = round(statistics.median(m["ms"] for m in mine)
                                                 / statistics.median(t["ms"] for t in theirs), 3)
                r[name + "_inside_parent_spread"] = all(lo <= m["ms"] <= hi for m in mine)
    doc = {"what": "rotated block-wise quantisation: coalac_encode_block_rot / _rot_sr / coalac_decode_block_rot beside "
                   "the unrotated entry points of this build and of the parent commit's library",
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
