"""The kernels' own sr_u24 / sr_code (coalac.hip, their __host__ side) against the numpy model (tests/sr_model.py), and
the argument checks of coalac_encode_sr / coalac_encode_block_sr, without Python in the process and without a GPU:
tests/sr_host_checks.hip (a stand-alone program that includes coalac.hip) is built with the host sanitizers and
-ffp-contract=off, and run as a child process over a table of draws and codes this test writes from the model —
seeds, positions on both sides of 2^32, quotients at and next to integers, NaN, infinities and the ends of the range.
The device code in the binary is never run (built at -O0 to keep the compile short)."""
import numpy as np

from tests import sr_model as M
from tests.host_program import build_and_run


def _table(path):
    rng = np.random.default_rng(18)
    seeds = [0, 1, 0xDEADBEEFCAFEF00D, (1 << 64) - 1] + [int(x) for x in rng.integers(0, 1 << 63, 4)]
    pos = np.concatenate([np.arange(8), (1 << 32) + np.arange(-4, 5), (1 << 45) + np.arange(3), (5 << 32) - 1 + np.arange(3),
                          rng.integers(0, 1 << 46, 24)]).astype(np.uint64)
    rows = []
    for s in seeds:
        rows += [f"u {s:x} {int(c):x} {int(u):x}" for c, u in zip(pos, M.sr_u24(s, pos))]
    for levels in (1, 3, 15, 127, 255):
        L = np.float32(levels)
        t = (rng.random(400) * levels).astype(np.float32)
        ints = np.arange(0, levels + 1, max(1, levels // 16)).astype(np.float32)
        near = np.concatenate([(ints.view(np.int32) + d).view(np.float32) for d in (-2, -1, 1, 2)])
        edge = np.array([0.0, -0.0, -1.5, np.nan, np.inf, -np.inf, 1e-45, 2.0 ** -30, 2.0 ** -24, 2.0 ** -23, L, L * 2,
                         np.nextafter(L, np.float32(0)), 0.5, 0.99999994], np.float32)
        t = np.concatenate([t, ints, near, edge]).astype(np.float32)
        u = rng.integers(0, 1 << 24, t.size).astype(np.uint32)
        u[::7] = 0
        u[3::7] = (1 << 24) - 1
        codes = M.codes_of(t, u, levels)
        rows += [f"c {int(b):x} {int(x):x} {levels:x} {int(c):x}" for b, x, c in zip(t.view(np.uint32), u, codes)]
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


def test_kernel_source_matches_the_model_and_checks_its_arguments(tmp_path):
    table = str(tmp_path / "table.txt")
    _table(table)
    built, run = build_and_run("sr_host_checks", tmp_path, table)
    assert built.returncode == 0, built.stderr[-4000:]
    assert run.returncode == 0 and "sr host checks: ok" in run.stdout, (run.stdout[-4000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr, run.stderr[-4000:]
