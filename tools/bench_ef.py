"""Cost of error feedback on one upload: one ResNet-50 update, ratio 0.01, 8 bits, delta mode.

Timed with HIP events over windows of back-to-back calls (the median of --windows windows of --steps calls each,
after a warm-up of every shape):

  (a) plain     the encode without error feedback: plan.encode(x, base)
  (b) ef        accumulate + encode(residual) + commit: the three launches of an error-feedback round
  (c) torch     the same result composed from the public operations that existed before the two kernels:
                r.add_(x - base); enc = plan.encode(r); r.sub_(plan.decode(enc))
  and each new kernel alone, with its algorithmic bytes against the 8 TB/s HBM peak: accumulate moves 16 B per
  element (12 without a base); commit reads its entries (idx + code) and reads and writes the 64-byte sectors of
  the residual they fall in.

    python tools/bench_ef.py [--layout resnet50_tv] [--out profiles/ef_step.json] [--label plain-stores]

COALAC_LIB selects an A/B build of the library (tools/build_variant.sh, e.g. -DEF_STORE_AUX=2).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--layout", default="resnet50_tv")
    p.add_argument("--ratio", type=float, default=0.01)
    p.add_argument("--bits", type=int, default=8)
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--windows", type=int, default=9)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--label", default="")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch

    from coala_amd.compression import CodecPlan
    from coala_amd.layouts import fp32_sizes
    from coala_amd.workload import synth_batch

    dev = torch.device("cuda", 0)
    sizes = fp32_sizes(a.layout)
    plan = CodecPlan(sizes, a.ratio, a.bits, device=dev)
    base = synth_batch(plan.table, dev, client_ids=[999])
    x = synth_batch(plan.table, dev, client_ids=[0])
    ws, out = plan.empty_workspace(), plan.empty_encoded()
    r = torch.zeros_like(x)  # the flat layout's length (its last segment padded to the alignment)
    dense = torch.empty_like(x)
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

    def plain():
        plan.encode(x, base=base, out=out, workspace=ws)

    def ef():
        plan.ef_accumulate(r, flat=x, base=base)
        plan.encode(r, out=out, workspace=ws)
        plan.ef_commit(out, r)

    def composed():
        r.add_(x - base)
        plan.encode(r, out=out, workspace=ws)
        r.sub_(plan.decode(out, out=dense))

    # the two flows give the same residual and payload (finite data: the non-finite rule never applies)
    r.zero_()
    ef()
    ef()
    r_ef, idx_ef = r.clone(), out.idx.clone()
    r.zero_()
    composed()
    composed()
    same = bool(torch.equal(r_ef.view(torch.int32), r.view(torch.int32)) and torch.equal(idx_ef, out.idx))

    res = {"plain_encode": window(plain)}
    r.zero_()
    res["ef_encode"] = window(ef)
    r.zero_()
    res["torch_composition"] = window(composed)
    r.zero_()
    res["k_ef_accumulate"] = window(lambda: plan.ef_accumulate(r, flat=x, base=base))
    r.zero_()
    res["k_ef_accumulate_no_base"] = window(lambda: plan.ef_accumulate(r, flat=x))
    r.zero_()
    ef()
    res["k_ef_commit"] = window(lambda: plan.ef_commit(out, r))

    N, K, U = int(sum(sizes)), int(plan.total_k), int(plan.n_units)
    vb = 4 if a.bits == 32 else 1
    segs = plan.table.segs.astype(np.int64)
    idx = out.idx.cpu().numpy().astype(np.int64)
    pos = np.concatenate([off + idx[oo:oo + k] for off, n, k, oo in segs])
    sectors = int(np.unique(pos // 16).size)  # 64-byte sectors of the residual that hold a kept entry

    def roof(name, nbytes):
        ms = res[name]["ms"]
        gbs = nbytes / (ms * 1e-3) / 1e9
        res[name].update({"alg_bytes": int(nbytes), "achieved_GBs": round(gbs, 1), "frac_of_hbm_peak": round(gbs / HBM_GBS, 4)})

    roof("k_ef_accumulate", 16 * N + 32 * U)
    roof("k_ef_accumulate_no_base", 12 * N + 32 * U)
    roof("k_ef_commit", (4 + vb) * K + 2 * 64 * sectors + (32 + 4) * U)
    res["k_ef_commit"].update({"entries": K, "sectors_64B": sectors})
    doc = {"what": "error-feedback encode of one update vs the plain encode and the torch composition",
           "layout": a.layout, "elements": N, "ratio": a.ratio, "bits": a.bits, "mode": "delta",
           "library": os.path.basename(os.environ.get("COALAC_LIB", "")) or "in-tree", "label": a.label,
           "timing": f"HIP events, median of {a.windows} windows of {a.steps} back-to-back calls",
           "hbm_peak_GBs": HBM_GBS, "results": res,
           "ef_over_plain": round(res["ef_encode"]["ms"] / res["plain_encode"]["ms"], 3),
           "torch_over_ef": round(res["torch_composition"]["ms"] / res["ef_encode"]["ms"], 3),
           "ef_equals_torch_composition": same}
    line = json.dumps(doc)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")


if __name__ == "__main__":
    main()
