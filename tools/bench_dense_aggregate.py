"""Cost of the dense fused aggregate: --clients ResNet-50 uploads at ratio 1, weights and delta mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up, with the windows' min and max), for block-wise at 4 bits, bit-packed at 4 bits and plain at 8 bits:

  (a) new        coalac_aggregate_dense on the uploads' own buffers, with its algorithmic bytes
                 C N b / 8 + 4N (+ 4N with a base) + 8 C R against the 8 TB/s HBM peak; with --variant-lib, the same
                 call on builds with other AGD_SPLIT / AGD_DEPTH (the A/B of the split and the depth)
  (b) replaced   the route it replaces, on --parent-lib (a build of the parent commit's coalac.hip) through its C ABI
                 on the same buffers — block-wise: C x coalac_decode_block + torch's weighted sum and division; packed:
                 C x coalac_unpack_dense + coalac_aggregate with implied indices; plain: coalac_aggregate with implied
                 indices — and the extra device memory each route holds
  (c) unchanged  this library's coalac_aggregate (sparse, ratio 0.01), coalac_decode_block and coalac_decode_packed
                 beside the parent's, window against window
  (d) hook       server.aggregate() host wall time (synchronised), the switch on and off, median of --hook-reps

    python tools/bench_dense_aggregate.py --parent-lib PATH [--variant-lib NAME=PATH ...] [--out profiles/dense_aggregate_step.json]
"""
import argparse
import copy
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
FORMATS = (("block4", "block", 4), ("packed4", "packed", 4), ("plain8", "codes", 8))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--clients", type=int, default=16)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--hook-reps", type=int, default=9)
    p.add_argument("--hook-layout", default=None, help="layout of the server hook's round (default: --layout)")
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--variant-lib", action="append", default=[], help="NAME=PATH of another build of this source")
    p.add_argument("--skip", nargs="*", default=[], choices=["replaced", "unchanged", "hook"])
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from coala_amd.compression import CodecPlan, CompressionServerMixin, UpdateCodec, _lib
    from coala_amd.compression.spec import SegmentTable
    from coala_amd.fl import LoopbackServer
    from coala_amd.layouts import build_module, fp32_sizes
    from coala_amd.workload import synth_batch

    dev = torch.device("cuda", 0)
    sizes = fp32_sizes(a.layout)
    C = a.clients
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    NUL = ctypes.c_void_p(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def window(fn, steps=None):
        steps = a.steps if steps is None else steps
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        per = []
        for _ in range(a.windows):
            t0.record()
            for _ in range(steps):
                fn()
            t1.record()
            torch.cuda.synchronize()
            per.append(t0.elapsed_time(t1) / steps)
        return {"ms": round(statistics.median(per), 5), "min": round(min(per), 5), "max": round(max(per), 5)}

    def roof(r, nbytes):
        gbs = nbytes / (r["ms"] * 1e-3) / 1e9
        r.update({"alg_bytes": int(nbytes), "achieved_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_GBS, 4)})
        return r

    def overlap(x, y):
        return not (x["max"] < y["min"] or y["max"] < x["min"])

    def bind(path):
        lib = ctypes.CDLL(path)
        for name, res, args in _lib.SIGNATURES:
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = res, args
        return lib

    def lib_plan(lib, plan):
        segs = plan.table.segs
        arr = (_lib.SegDesc * len(segs))(*[_lib.SegDesc(*r) for r in segs.tolist()])
        h = ctypes.c_void_p()
        assert lib.coalac_plan_create(arr, len(segs), plan.bits, ctypes.byref(h)) == 0
        return h

    parent = bind(a.parent_lib) if a.parent_lib else None
    variants = {n: bind(q) for n, q in (v.split("=", 1) for v in a.variant_lib)}
    res = {}

    def write(res, final=True):
        """The result document: printed once at the end, written to --out after every section."""
        doc = document(a, sizes, variants, res)
        if final:
            print(json.dumps(doc), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    one_table = SegmentTable(sizes, 1.0, 1)
    base = synth_batch(one_table, dev, client_ids=[99])
    w_host = [1 + (i * 7) % 13 for i in range(C)]  # (sample counts: integers, as the int64 counters need)
    total = float(sum(w_host))
    wdev = torch.tensor(w_host, dtype=torch.float32, device=dev)

    for tag, kind, bits in FORMATS:
        r = res[tag] = {}
        plan = CodecPlan(sizes, 1.0, bits, device=dev)
        N, U, T, Pw = int(plan.total_k), int(plan.n_units), int(plan.n_segments), int(plan.dense_packed_words)
        R = U if kind == "block" else T
        codes, mns, scs = [], [], []
        for c in range(C):  # every upload in its own buffers, as encoded_to() leaves them
            x = synth_batch(one_table, dev, client_ids=[c])
            if kind == "block":
                bm, bs, st = plan.encode_block(flat=x)
                codes.append(st.clone()), mns.append(bm.clone()), scs.append(bs.clone())
            else:
                e = plan.encode(x)
                codes.append(plan.pack_dense(e).clone() if kind == "packed" else e.vals.clone())
                mns.append(e.mn.clone()), scs.append(e.scale.clone())
            del x
        out = plan.empty_flat()
        code_b = (4 * Pw) if kind != "codes" else N
        r.update({"elements": N, "clients": C, "ranges_per_client": R, "code_bytes_per_client": code_b})
        ptrs = torch.tensor([t.data_ptr() for ts in (codes, mns, scs) for t in ts], dtype=torch.int64).to(dev)
        pp = ptrs.data_ptr()
        kid = plan.AGG_DENSE_KINDS[kind]

        def dense_call(lib, h, b):
            def f():
                assert lib.coalac_aggregate_dense(h, C, kid, ctypes.c_void_p(pp), ctypes.c_uint64(code_b),
                                                  ctypes.c_void_p(pp + 8 * C), ctypes.c_void_p(pp + 16 * C), P(wdev),
                                                  ctypes.c_float(total), _lib.COALAC_AGG_RECIP, NUL,
                                                  NUL if b is None else P(b), P(out), stream()) == 0
            return f
        for mode, b in (("weights", None), ("delta", base)):
            alg = C * code_b + 4 * N + (4 * N if b is not None else 0) + 8 * C * R
            r[f"new_{mode}"] = roof(window(dense_call(plan._lib, plan._h, b)), alg)
            r[f"new_{mode}_wrapper"] = window(lambda: plan.aggregate_dense(codes, mns, scs, w_host, total=total, base=b,
                                                                           out=out, kind=kind))
            for name, lib in variants.items():
                r[f"new_{mode}_{name}"] = roof(window(dense_call(lib, lib_plan(lib, plan), b)), alg)
        r["extra_device_bytes_new"] = 0

        if parent is not None and "replaced" not in a.skip:
            ph = lib_plan(parent, plan)
            if kind == "block":
                dense = [plan.empty_flat() for _ in range(C)]
                r["extra_device_bytes_replaced"] = C * 4 * int(plan.span)

                def replaced(b):
                    def f():
                        for c in range(C):
                            assert parent.coalac_decode_block(ph, P(codes[c]), ctypes.c_uint64(4 * Pw), P(mns[c]), P(scs[c]),
                                                              NUL if b is None else P(b), P(dense[c]), stream()) == 0
                        acc = dense[0] * w_host[0]
                        for c in range(1, C):
                            acc += dense[c] * w_host[c]
                        torch.div(acc, total, out=out)
                    return f
            else:
                batched = CodecPlan(sizes, 1.0, bits, clients=C, device=dev)
                bh = lib_plan(parent, batched)
                idx, ust = batched.implied_indices(), batched.implied_starts()
                vals = torch.empty(C * N, dtype=torch.uint8, device=dev)
                mn, sc = torch.cat(mns), torch.cat(scs)
                if kind == "codes":
                    vals.copy_(torch.cat(codes))
                r["extra_device_bytes_replaced"] = int(idx.numel() * 4 + ust.numel() * 4 + vals.numel())

                def replaced(b):
                    def f():
                        if kind == "packed":
                            for c in range(C):
                                assert parent.coalac_unpack_dense(ph, P(codes[c]), ctypes.c_uint64(4 * Pw),
                                                                  ctypes.c_void_p(vals.data_ptr() + c * N), stream()) == 0
                        assert parent.coalac_aggregate(bh, C, P(idx), P(vals), P(mn), P(sc), P(ust), P(wdev),
                                                       ctypes.c_float(total), _lib.COALAC_AGG_RECIP, NUL,
                                                       NUL if b is None else P(b), P(out), stream()) == 0
                    return f
            for mode, b in (("weights", None), ("delta", base)):
                r[f"replaced_{mode}"] = window(replaced(b))
                new, old = r[f"new_{mode}"], r[f"replaced_{mode}"]
                r[f"new_over_replaced_{mode}"] = round(new["ms"] / old["ms"], 4)
                r[f"new_faster_windows_disjoint_{mode}"] = new["max"] < old["min"]
            if kind == "block":
                del dense
            else:
                del batched, idx, ust, vals
        del codes, mns, scs, out, plan
        torch.cuda.empty_cache()
        write(res, final=False)

    if parent is not None and "unchanged" not in a.skip:
        u = res["unchanged"] = {}
        # the sparse aggregate: C uploads at ratio 0.01, 8 bits
        sp = CodecPlan(sizes, 0.01, 8, clients=C, device=dev)
        x = synth_batch(sp.table, dev)
        enc = sp.encode(x)
        del x
        sout = torch.empty(sp.table.span_per_client, dtype=torch.float32, device=dev)
        sph = lib_plan(parent, sp)

        def sparse(lib, h):
            return lambda: lib.coalac_aggregate(h, C, P(enc.idx), P(enc.vals), P(enc.mn), P(enc.scale), P(enc.ustart),
                                                P(wdev), ctypes.c_float(total), _lib.COALAC_AGG_RECIP, NUL, NUL, P(sout),
                                                stream())
        plan = CodecPlan(sizes, 1.0, 4, device=dev)
        x = synth_batch(one_table, dev, client_ids=[0])
        bm, bs, st = plan.encode_block(flat=x)
        e = plan.encode(x)
        pk = plan.pack_dense(e)
        flat = plan.empty_flat()
        ph = lib_plan(parent, plan)
        pb = ctypes.c_uint64(4 * pk.numel())
        pairs = {
            "aggregate_sparse": (sparse(sp._lib, sp._h), sparse(parent, sph)),
            "decode_block": (lambda: plan._lib.coalac_decode_block(plan._h, P(st), pb, P(bm), P(bs), NUL, P(flat), stream()),
                             lambda: parent.coalac_decode_block(ph, P(st), pb, P(bm), P(bs), NUL, P(flat), stream())),
            "decode_packed": (lambda: plan._lib.coalac_decode_packed(plan._h, P(pk), pb, P(e.mn), P(e.scale), NUL, P(flat), stream()),
                              lambda: parent.coalac_decode_packed(ph, P(pk), pb, P(e.mn), P(e.scale), NUL, P(flat), stream())),
        }
        for name, (mine, theirs) in pairs.items():
            assert mine() == 0 and theirs() == 0
            ws = [window(mine), window(theirs), window(mine), window(theirs)]  # interleaved: the run-to-run spread
            u[name] = {"this": ws[0], "parent": ws[1], "this_again": ws[2], "parent_again": ws[3],
                       "windows_overlap": any(overlap(m, t) for m in (ws[0], ws[2]) for t in (ws[1], ws[3]))}
        del sp, enc, sout, plan, flat
        torch.cuda.empty_cache()
        write(res, final=False)

    if "hook" not in a.skip:
        hk = res["hook"] = {}
        layout = a.hook_layout or a.layout
        g = build_module(layout, seed=5).to(dev)
        for tag, kind, bits in FORMATS:
            kw = {"block": dict(blockwise=True), "packed": dict(pack_dense=True), "codes": {}}[kind]
            codec = UpdateCodec(1.0, bits, "weights", **kw)
            ups = []
            for s in range(C):
                m = build_module(layout, seed=s + 1).to(dev)
                ups.append(pickle.loads(pickle.dumps(codec.encode_module(m))))
                del m
            hk[tag] = {"layout": layout, "clients": C}
            for dense in (True, False):
                class Server(CompressionServerMixin, LoopbackServer):
                    codec_ratio, codec_bits, codec_mode = 1.0, bits, "weights"
                    codec_fused_aggregate = True
                    codec_fused_dense_aggregate = dense
                srv = Server(copy.deepcopy(g), [])
                ts = []
                for _ in range(a.hook_reps + 1):
                    torch.cuda.synchronize()
                    s = time.perf_counter()
                    agg = srv.aggregate(list(ups), w_host)
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - s) * 1e3)
                    del agg
                hk[tag]["switch_on_ms" if dense else "switch_off_ms"] = round(statistics.median(ts[1:]), 3)
                del srv
            del ups
            torch.cuda.empty_cache()

    write(res)


def document(a, sizes, variants, res):
    return {"what": "dense fused aggregate: coalac_aggregate_dense on the uploads' own buffers beside the routes it "
                   "replaces (on the parent library), the unchanged kernels, and the server hook",
           "layout": a.layout, "elements": int(sum(sizes)), "clients": a.clients, "ratio": 1.0,
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "variants": sorted(variants),
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the windows' "
                     f"spread); hook: host wall time, median of {a.hook_reps}",
           "byte_model": "C N b / 8 + 4N (+ 4N with a base) + 8 C R", "hbm_peak_GBs": HBM_GBS, "results": res}


if __name__ == "__main__":
    main()
