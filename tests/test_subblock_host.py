"""The argument checks of the block-size entry points — coalac_plan_block_count, coalac_encode_block_g,
coalac_decode_block_g, coalac_aggregate_dense_g — without Python in the process and without a GPU:
tests/subblock_host_checks.hip (a stand-alone program that includes coalac.hip) is built with the host sanitizers and run
as a child process. Every COALAC_EINVAL case returns before the first device call, so plans in host memory serve; the
device code in the binary is never run (built at -O0 to keep the compile short)."""
import os
import subprocess

from coala_amd import _build

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "subblock_host_checks.hip")
SANITIZE = "-fsanitize=address,undefined"


def test_entry_points_check_their_arguments_before_any_device_call(tmp_path):
    exe = str(tmp_path / "subblock_host_checks")
    cmd = [_build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", f"--offload-arch={_build.ARCH}",
           "-Xarch_device", "-O0", "-Xarch_device", "-g0", "-Xarch_host", SANITIZE,
           "-Xarch_host", "-fno-sanitize-recover=undefined", SANITIZE,  # (the last one: the link's runtime)
           "-Wno-option-ignored", "-Wno-pass-failed", "-o", exe, SRC]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert run.returncode == 0 and "subblock host checks: ok" in run.stdout, (run.stdout[-4000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr, run.stderr[-4000:]
