"""Cost of the sparse fused aggregate from the uploads' own buffers: --clients ResNet-50 uploads at
ratio 0.01, delta mode, bits 8 and 4.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each, after
a warm-up, with the windows' min and max):

  (a) parent     coalac_aggregate on the concatenated uploads, on --parent-lib (a build of the parent commit's
                 coalac.hip), twice (its run-to-run spread), and this library's coalac_aggregate beside it
  (b) entries    coalac_aggregate_uploads, kind ENTRIES, on the uploads' own idx / vals arrays
  (c) compact    coalac_aggregate_uploads, kind COMPACT, on the uploads' own wire v3 streams
  (d) unpack     the --clients coalac_unpack launches that (c) replaces
  (e) hook       UpdateCodec.aggregate() from --clients received blobs, host wall time (synchronised), sparse_uploads
                 off and on, for plain (wire v2) and compact (wire v3) blobs, median of --hook-reps

    python tools/bench_sparse_aggregate.py --parent-lib PATH [--out profiles/sparse_aggregate_step.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--clients", type=int, default=16)
    p.add_argument("--ratio", type=float, default=0.01)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--hook-reps", type=int, default=9)
    p.add_argument("--parent-lib", default=None)
    p.add_argument("--skip", nargs="*", default=[], choices=["hook"])
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch

    from coala_amd.compression import CodecPlan, CompressedUpdate, UpdateCodec, _lib
    from coala_amd.compression.spec import SegmentTable
    from coala_amd.layouts import build_module, fp32_sizes
    from coala_amd.workload import synth_batch

    dev = torch.device("cuda", 0)
    sizes = fp32_sizes(a.layout)
    C = a.clients
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    NUL = ctypes.c_void_p(0)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def window(fn):
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
    res = {}
    one_table = SegmentTable(sizes, a.ratio, 1)
    base = synth_batch(one_table, dev, client_ids=[99])
    w_host = [1 + (i * 7) % 13 for i in range(C)]
    total = float(sum(w_host))
    wdev = torch.tensor(w_host, dtype=torch.float32, device=dev)

    for bits in (8, 4):
        r = res[f"bits{bits}"] = {}
        one = CodecPlan(sizes, a.ratio, bits, device=dev)
        many = CodecPlan(sizes, a.ratio, bits, clients=C, device=dev)
        K, Pw = int(one.total_k), int(one.packed_words)
        ups = []
        for c in range(C):  # every upload in its own buffers, as encoded_to() leaves them
            e = one.encode(synth_batch(one_table, dev, client_ids=[c]), base=base)
            ups.append((e.idx.clone(), e.vals.clone(), e.mn.clone(), e.scale.clone(), e.ustart.clone(), one.pack(e).clone()))
        cat = [torch.cat([u[i] for u in ups]) for i in range(5)]
        out = one.empty_flat()
        r.update({"entries_per_client": K, "stream_bytes_per_client": 4 * Pw, "entry_bytes_per_client": 5 * K})
        ptrs = torch.tensor([u[i].data_ptr() for i in (0, 5, 1, 2, 3, 4) for u in ups], dtype=torch.int64).to(dev)
        at = lambda j: ctypes.c_void_p(ptrs.data_ptr() + 8 * C * j)  # noqa: E731

        def batched(lib, h):
            return lambda: lib.coalac_aggregate(h, C, P(cat[0]), P(cat[1]), P(cat[2]), P(cat[3]), P(cat[4]), P(wdev),
                                                ctypes.c_float(total), _lib.COALAC_AGG_RECIP, NUL, P(base), P(out),
                                                stream())

        def uploads(kind):
            return lambda: one._lib.coalac_aggregate_uploads(
                one._h, C, kind, at(0), at(1), ctypes.c_uint64(4 * Pw), at(2), at(3), at(4), at(5), P(wdev),
                ctypes.c_float(total), _lib.COALAC_AGG_RECIP, NUL, P(base), P(out), stream())
        scratch = (torch.empty(K, dtype=torch.int32, device=dev), torch.empty(K, dtype=torch.uint8, device=dev))

        def unpacks():
            for u in ups:
                one._lib.coalac_unpack(one._h, P(u[5]), ctypes.c_uint64(4 * Pw), P(u[4]), P(scratch[0]), P(scratch[1]),
                                       stream())
        mine = batched(many._lib, many._h)
        ent, com = uploads(_lib.COALAC_AGGS_ENTRIES), uploads(_lib.COALAC_AGGS_COMPACT)
        assert mine() == 0 and ent() == 0 and com() == 0
        ref = out.clone()
        for f in (mine, ent):  # the three forms compute the same bits
            out.zero_()
            f()
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        if parent is not None:
            theirs = batched(parent, lib_plan(parent, many))
            assert theirs() == 0
            r["a_parent_aggregate"] = window(theirs)
        r["a_this_aggregate"] = window(mine)
        r["b_uploads_entries"] = window(ent)
        r["c_uploads_compact"] = window(com)
        r["d_unpack_x_clients"] = window(unpacks)
        if parent is not None:
            r["a_parent_aggregate_again"] = window(theirs)
            pa = (r["a_parent_aggregate"], r["a_parent_aggregate_again"])
            r["parent_spread_ms"] = [min(x["min"] for x in pa), max(x["max"] for x in pa)]
            for k in ("a_this_aggregate", "b_uploads_entries", "c_uploads_compact"):
                r[k]["within_parent_spread"] = any(overlap(r[k], x) for x in pa)
                r[k]["over_parent_median"] = round(r[k]["ms"] / statistics.median(x["ms"] for x in pa), 4)
        del ups, cat, out, one, many
        torch.cuda.empty_cache()

    if "hook" not in a.skip:
        hk = res["hook"] = {}
        g = build_module(a.layout, seed=5).to(dev)
        for bits in (8, 4):
            for compact in (False, True):
                client = UpdateCodec(a.ratio, bits, "delta", compact=compact)
                snap = client.snapshot(g)
                blobs = []
                for s in range(C):
                    m = build_module(a.layout, seed=s + 1).to(dev)
                    blobs.append(client.encode_module(m, base=snap).to_bytes())
                    del m
                server = UpdateCodec(a.ratio, bits, "delta")
                h = hk[f"bits{bits}_{'compact' if compact else 'plain'}"] = {"blob_bytes": len(blobs[0])}
                for on in (False, True):
                    ts = []
                    for _ in range(a.hook_reps + 1):
                        ups = [CompressedUpdate.from_bytes(b) for b in blobs]  # (received: not timed)
                        torch.cuda.synchronize()
                        s = time.perf_counter()
                        agg = server.aggregate(ups, w_host, g, base=snap, sparse_uploads=on)
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - s) * 1e3)
                        del agg, ups
                    h["sparse_uploads_on_ms" if on else "sparse_uploads_off_ms"] = {
                        "ms": round(statistics.median(ts[1:]), 3), "min": round(min(ts[1:]), 3), "max": round(max(ts[1:]), 3)}
                del blobs
                torch.cuda.empty_cache()

    doc = {"what": "sparse fused aggregate from the uploads' own buffers: coalac_aggregate_uploads (entries, compact) "
                   "beside coalac_aggregate on the concatenation (parent build and this one), the unpack launches the "
                   "compact kind replaces, and UpdateCodec.aggregate from received blobs",
           "layout": a.layout, "elements": int(sum(sizes)), "clients": C, "ratio": a.ratio, "mode": "delta",
           "parent_library": os.path.basename(a.parent_lib) if a.parent_lib else None,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls (min, max: the windows' "
                     f"spread); hook: host wall time, median of {a.hook_reps}",
           "results": res}
    print(json.dumps(doc), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
