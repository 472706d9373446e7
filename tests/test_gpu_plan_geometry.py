"""Plan geometry and workspace bounds of the codec library.

The workspace size, the payload size, the span and the unit count of a plan (coalac_plan_query) are pinned to
literals recorded from the library of commit 2089ce0 (the parent of the change that made the workspace and the plan
tables one walk each) on an MI355X: the walk must place every array where the four hand-kept lists did. The tables are
the smallest that reach each branch of the layout code. The encode must stay inside the workspace the plan asks for:
a guard after it survives, and the payload is the oracle's.
"""
import ctypes

import numpy as np
import pytest
import torch

from coala_amd.compression import CodecPlan
from coala_amd.compression._lib import COALAC_FLAG_STAMPS
from oracle import codec_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 300, 1024, 1025, 4096, 4097, 70001]  # around the small-segment limits and the unit size, one multi-unit
DENSE = [0, 5, 5000]                             # ratio 1, with an empty segment
OVER_LATENCY = [4096 * 8200, 300]                # more than LATENCY_PLAN_UNITS (8192) units
FORK_CLASS = [4096 * 16384, 300]                 # FORK_MIN_LUNITS (16384) large units beside a small segment

# (sizes, ratio, bits, clients, environment) -> (ws_bytes, total_k, span, n_units), from commit 2089ce0's library
GEOMETRY = {
    ("sizes", 0.01, 8, 1, ""): (99072, 809, 80657, 25),
    ("sizes", 0.01, 8, 2, ""): (193536, 1618, 161329, 50),
    ("sizes", 0.01, 32, 1, ""): (99072, 809, 80657, 25),
    ("sizes", 0.01, 32, 2, ""): (193536, 1618, 161329, 50),
    ("sizes", 0.3, 8, 1, ""): (411648, 24167, 80657, 25),
    ("sizes", 0.3, 8, 2, ""): (818688, 48334, 161329, 50),
    ("sizes", 0.3, 32, 1, ""): (411648, 24167, 80657, 25),
    ("sizes", 0.3, 32, 2, ""): (818688, 48334, 161329, 50),
    ("dense", 1.0, 8, 1, ""): (256, 5005, 5032, 3),
    ("dense", 1.0, 32, 1, ""): (256, 5005, 5032, 3),
    ("over_latency", 0.01, 8, 1, ""): (29858816, 335875, 33587500, 8201),
    ("fork_class", 0.01, 8, 1, ""): (59645696, 671092, 67109164, 16385),
    ("sizes", 0.01, 8, 1, "COALAC_SMALL_MAX=4096"): (83968, 809, 80657, 25),
    ("sizes", 0.01, 8, 1, "COALAC_CCAP=512"): (90624, 809, 80657, 25),
    ("sizes", 0.3, 8, 1, "COALAC_SMALL_MAX=4096"): (368128, 24167, 80657, 25),
    ("sizes", 0.3, 8, 1, "COALAC_CCAP=512"): (90624, 24167, 80657, 25),
}

# the same commit's coalac_debug_stamps / coalac_debug_brackets counts for SIZES at ratio 0.3 (asked for 4096 each)
STAMP_COUNT, BRACKET_COUNT = 224, 22


def geometry_cases():
    cases = [("sizes", r, b, c, "") for r in (0.01, 0.3) for b in (8, 32) for c in (1, 2)]
    cases += [("dense", 1.0, b, 1, "") for b in (8, 32)]
    cases += [("over_latency", 0.01, 8, 1, ""), ("fork_class", 0.01, 8, 1, "")]
    cases += [("sizes", r, 8, 1, env) for r in (0.01, 0.3) for env in ("COALAC_SMALL_MAX=4096", "COALAC_CCAP=512")]
    return cases


TABLES = {"sizes": SIZES, "dense": DENSE, "over_latency": OVER_LATENCY, "fork_class": FORK_CLASS}


def query(name, ratio, bits, clients, env, monkeypatch):
    if env:
        monkeypatch.setenv(*env.split("="))
    plan = CodecPlan(TABLES[name], ratio, bits, clients=clients)
    got = (plan.ws_bytes, plan.total_k, plan.span, plan.n_units)
    plan.close()
    return got


@pytest.mark.parametrize("name,ratio,bits,clients,env", geometry_cases())
def test_plan_geometry_is_the_parents(cuda, monkeypatch, name, ratio, bits, clients, env):
    got = query(name, ratio, bits, clients, env, monkeypatch)
    print("GEOMETRY", repr((name, ratio, bits, clients, env)), got)
    assert got == GEOMETRY[(name, ratio, bits, clients, env)]


GUARD = 4096


def guarded_encode(sizes, ratio, bits, flags=0):
    """One encode into a workspace of exactly ws_bytes followed by a guard; returns the plan, the workspace, the
    inputs and the encoded buffers after asserting that the guard is intact."""
    plan = CodecPlan(sizes, ratio, bits)
    t = plan.table
    rng = np.random.default_rng(len(sizes) * 100 + bits)
    flat = np.zeros(t.span, np.float32)
    for off, n in zip(t.offsets, sizes):
        flat[off:off + n] = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    ws = torch.full((plan.ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    enc = plan.encode(torch.from_numpy(flat).cuda(), workspace=ws, flags=flags, out=plan.empty_encoded(with_idx=True))
    torch.cuda.synchronize()
    guard = ws[plan.ws_bytes:].cpu().numpy()
    assert guard.size == GUARD and np.all(guard == 0xA5), np.flatnonzero(guard != 0xA5)[:8]
    return plan, ws, flat, enc


def assert_payload_is_the_oracles(plan, flat, enc, bits):
    segs = plan.table.segs.astype(np.int64)
    idx, vals, mn, sc = O.encode(flat, segs, bits)
    np.testing.assert_array_equal(enc.idx.cpu().numpy(), idx)
    np.testing.assert_array_equal(enc.vals.cpu().numpy().view(np.uint8), vals.view(np.uint8))
    np.testing.assert_array_equal(enc.mn.cpu().numpy().view(np.uint32), mn.view(np.uint32))
    np.testing.assert_array_equal(enc.scale.cpu().numpy().view(np.uint32), sc.view(np.uint32))
    np.testing.assert_array_equal(enc.ustart.cpu().numpy(), O.unit_starts(idx, segs))


@pytest.mark.parametrize("bits", [8, 32])
@pytest.mark.parametrize("name,ratio", [("sizes", 0.3), ("dense", 1.0)])
def test_encode_stays_inside_its_workspace(cuda, name, ratio, bits):
    plan, ws, flat, enc = guarded_encode(TABLES[name], ratio, bits)
    assert_payload_is_the_oracles(plan, flat, enc, bits)


def test_stamped_encode_stays_inside_its_workspace(cuda):
    """COALAC_FLAG_STAMPS: the kernels also write the workspace's stamp rows; the diagnostics read them and the
    brackets back from where the encode put them."""
    plan, ws, flat, enc = guarded_encode(SIZES, 0.3, 8, flags=COALAC_FLAG_STAMPS)
    assert_payload_is_the_oracles(plan, flat, enc, 8)
    n = 4096
    stamps = (ctypes.c_uint64 * n)()
    lo, hi = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
    p = ctypes.c_void_p(ws.data_ptr())
    got_stamps = plan._lib.coalac_debug_stamps(plan._h, p, None, stamps, n)
    got_brackets = plan._lib.coalac_debug_brackets(plan._h, p, None, lo, hi, n)
    print("STAMP_COUNT, BRACKET_COUNT =", got_stamps, got_brackets)
    assert (got_stamps, got_brackets) == (STAMP_COUNT, BRACKET_COUNT)
    # a stamped encode wrote clock ticks into some rows, and every upper bracket is a key (not the 0xA5 fill)
    assert np.count_nonzero(np.frombuffer(stamps, np.uint64)[:got_stamps] != 0xA5A5A5A5A5A5A5A5) > 0
    assert np.all(np.frombuffer(hi, np.uint32)[:got_brackets] <= 0x7FFFFFFF)
