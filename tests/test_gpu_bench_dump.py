"""bench.py --dump-outputs on the GPU: the arrays of the last timed step of a small headline workload (3 LeNet
clients as 2 sub-batches), whole and as the seeded sample, against the oracle; a plain run's result carries the
headline figure and none of the --full measurements."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from oracle import codec_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("idx", "vals", "mn", "scale", "ustart", "decoded")


@pytest.fixture(scope="module")
def dumped(cuda, tmp_path_factory):
    """One small plain run (2 timed steps), dumped whole and again with every array above its cap."""
    mp = pytest.MonkeyPatch()
    whole, sampled = (str(tmp_path_factory.mktemp(n)) for n in ("whole", "sampled"))
    mp.setattr(sys, "argv", ["bench.py", "--layout", "lenet", "--clients", "3", "--steps", "2", "--warmup", "1"])
    try:
        a = bench.parse()
        W = bench.setup_workload("C3", a, cuda, 0, headline=True)
        bench.warm_workload(W, a)
        res = bench.time_workload(W, a, cuda, 1, dump_dir=whole)
        mp.setattr(bench, "DUMP_CAPS", {n: 8 for n in NAMES})
        bench.dump_outputs(W, a, sampled)
        t = W["table"]
        flat = W["flats"][0].cpu().numpy()
        bench.release_workload(W)
    finally:
        mp.undo()
    segs = t.segs.astype(np.int64)
    idx, vals, mn, sc = O.encode(flat, segs, 8)
    dec = O.decode(idx, vals, mn, sc, segs, 8, t.span)
    ref = {"idx": idx, "vals": vals, "mn": mn, "scale": sc, "ustart": O.unit_starts(idx, segs),
           "decoded": np.concatenate([dec[off:off + n] for off, n in segs[:, :2]])}
    return res, whole, sampled, ref


def expected(ref, cap):
    """What dump_outputs keeps of an array: all of it up to `cap` elements, else the seeded sample of positions."""
    if ref.size <= cap:
        return ref
    return ref[np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, ref.size, cap))]


def test_dump_outputs_default_caps_match_the_oracle(dumped):
    """The encoded arrays whole, `decoded` (19.8 M elements, above its cap) as its sample; under 64 MB in all."""
    _, whole, _, ref = dumped
    assert sorted(os.listdir(whole)) == sorted(n + ".npy" for n in NAMES)
    assert ref["decoded"].size > bench.DUMP_CAPS["decoded"] and ref["idx"].size <= bench.DUMP_CAPS["idx"]
    for n in NAMES:
        x = np.load(os.path.join(whole, n + ".npy"))
        assert x.dtype == (np.float64 if n in ("idx", "ustart") else np.float32), n
        want = expected(ref[n], bench.DUMP_CAPS[n])
        assert x.shape == want.shape, n
        np.testing.assert_array_equal(x, want.astype(x.dtype), err_msg=n)
        assert np.count_nonzero(x) > 0, n
    sizes = {"idx": 8, "ustart": 8}
    assert sum(bench.DUMP_CAPS[n] * sizes.get(n, 4) for n in NAMES) <= 64e6


def test_dump_outputs_sample_is_seeded(dumped):
    """Every array above its cap (8 elements here): the same seeded positions, idx and vals paired."""
    _, _, sampled, ref = dumped
    for n in NAMES:
        x = np.load(os.path.join(sampled, n + ".npy"))
        assert ref[n].size > 8 and x.shape == (8,), n
        np.testing.assert_array_equal(x, expected(ref[n], 8).astype(x.dtype), err_msg=n)


def test_plain_result_has_the_headline_figure_only(dumped):
    res = dumped[0]
    assert res["ms_per_step"] > 0 and res["value"] > 0
    for k in ("roofline", "stages_ms", "repeat_windows"):
        assert k not in res
