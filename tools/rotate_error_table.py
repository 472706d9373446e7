"""The error table of DESIGN.md §22, from the committed model (tests/rot_model.py; no GPU): RMS error of
decode(encode(x)) against x on 2^18 elements, rotated 4096-element blocks beside unrotated blocks of 4096 and 256.

    python tools/rotate_error_table.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import rot_model as RM  # noqa: E402
from tests import subblock_model as SB  # noqa: E402


def main():
    rng = np.random.default_rng(22)
    n = 1 << 18
    spike = rng.standard_normal(n).astype(np.float32)
    spike[rng.integers(0, 4096, n // 4096) + np.arange(0, n, 4096)] = 1000.0  # one value of 1000 per block
    data = {"student_t3": rng.standard_t(3, n).astype(np.float32), "laplace": rng.laplace(size=n).astype(np.float32),
            "normal": rng.standard_normal(n).astype(np.float32), "normal_spike1000": spike}
    print("data bits rot4096/plain4096 rot4096/plain256")
    for name, x in data.items():
        for bits in (1, 2, 4):
            rot, p4096, p256 = RM.rms_error(x, bits, rot_seed=7), RM.rms_error(x, bits), SB.rms_error(x, bits, 256)
            print(f"{name} {bits} {rot / p4096:.3f} {rot / p256:.3f}")
    x = data["student_t3"][:1 << 16]
    for bits in (1, 2, 4):
        rot = np.mean([RM.roundtrip(x, bits, 100 + c, 200 + c).astype(np.float64) for c in range(16)], axis=0)
        plain = np.mean([RM.roundtrip(x, bits, None, 200 + c).astype(np.float64) for c in range(16)], axis=0)
        print(f"student_t3 mean-of-16-SR {bits} {np.sqrt(np.mean((rot - x) ** 2)) / np.sqrt(np.mean((plain - x) ** 2)):.3f}")


if __name__ == "__main__":
    main()
