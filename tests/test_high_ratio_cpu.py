"""The expected values of tests/test_gpu_high_ratio.py, checked without the kernel: the oracle's fast top-k at the
extreme ranks (its argpartition pivot n - k is 1 at k = n - 1 and n - 1 at k = 1; k = n returns every index), and the
sampler model's open
brackets — T_lo = 0 once ceil(p m + 6 sqrt(p m) + 8) >= m (the sampled lower rank does not exist), T_hi = KEY_MAX while
floor(p m - 6 sqrt(p m) - 8) < 1."""
import numpy as np
import pytest

from coala_amd.compression.spec import k_for
from oracle import codec_oracle as O
from tests.high_ratio_inputs import KINDS, SIZES, extreme_ks, layout, mixed_ks
from tests.sampler_model import KEY_MAX, TIE_FLAG, bracket, ccap_for, takes_raw_path


@pytest.mark.parametrize("kind", KINDS + ("one",))
def test_oracle_topk_at_extreme_ranks(kind):
    """O.topk_indices (argpartition on key << 32 | ~index) equals the full stable sort on every segment of the small
    layout at k in {1, 2, n - 1, n, n // 2 + 1}: ties (zeros, equal |x|, grid levels) go to the lower index."""
    for x in layout(kind):
        n = x.size
        for k in sorted({1, min(2, n), max(1, n - 1), n, n // 2 + 1}):
            got, want = O.topk_indices(x, k), O.topk_indices_bruteforce(x, k)
            assert got.dtype == np.int32 and got.size == k
            np.testing.assert_array_equal(got, want, err_msg=f"{kind} n={n} k={k}")


@pytest.mark.parametrize("i,ratio", [(0, 0.9), (1, 0.9), (5, 0.97)])
def test_model_opens_the_lower_bracket(i, ratio):
    """(n = 1025, 0.9), (n = 4097, 0.9): m = 1024 sampled keys, rlo = ceil(921.6 + 182.2 + 8) >= 1024;
    (n = 2^20, 0.97): m = 8192, rlo = ceil(7946.2 + 534.9 + 8) >= 8192. The bracket then starts at key 0 without the
    tie flag, keeps a sampled upper edge, and holds the k-th key with room in a unit's record slots (no raw path)."""
    x = layout("gauss")[i]
    k = k_for(x.size, ratio)
    tlo, thi, outcome = bracket(x, k, i)
    assert tlo == 0 and not tlo & TIE_FLAG and outcome == "none"
    assert 0 < thi < KEY_MAX
    assert not takes_raw_path(x, k, tlo, thi, ccap_for([ratio]))
    # ... and one step below the formula's threshold the lower rank exists again
    lo_ratio = {1025: 0.8, 4097: 0.8, 1 << 20: 0.9}[x.size]
    assert bracket(x, k_for(x.size, lo_ratio), i)[0] > 0


@pytest.mark.parametrize("k", [1, 2])
def test_model_opens_the_upper_bracket_at_tiny_k(k):
    """k = 1 and k = 2 of 2^20 elements: p m < 0.02, so rhi < 1 and T_hi stays KEY_MAX; the lower rank is
    ceil(6 sqrt(p m) + 8 + p m) = 9 or 10 of the 8192 sampled keys."""
    x = layout("gauss")[5]
    tlo, thi, _ = bracket(x, k, 5)
    assert thi == KEY_MAX and 0 < tlo < KEY_MAX
    assert not takes_raw_path(x, k, tlo, thi, ccap_for([k / x.size]))


def test_explicit_k_tables():
    ks = extreme_ks()
    assert [ks[i] for i in range(6)] == [1, 2, SIZES[2] - 1, SIZES[3], SIZES[4] // 2 + 1, k_for(1 << 20, 0.001)]
    assert extreme_ks(1)[5] == 1 and extreme_ks(1)[0] == 2
    assert ks[6:] == [700, 1] and all(1 <= k <= n for k, n in zip(ks, SIZES))
    mk = mixed_ks()
    assert max(k / n for k, n in zip(mk[:6], SIZES[:6])) > 0.475 and ccap_for([mk[3] / SIZES[3]]) == 4096
    assert any(k != n for k, n in zip(mk, SIZES))
