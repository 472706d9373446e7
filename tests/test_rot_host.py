"""The argument checks of the rotated block-wise entry points — coalac_encode_block_rot,
coalac_encode_block_rot_sr, coalac_decode_block_rot — without Python in the process and without a GPU:
tests/rot_host_checks.hip (a stand-alone program that includes coalac.hip) is built with the host sanitizers and run as
a child process. Every COALAC_EINVAL case returns before the first device call, so plans in host memory serve; the
device code in the binary is never run (built at -O0 to keep the compile short)."""
from tests.host_program import build_and_run


def test_entry_points_check_their_arguments_before_any_device_call(tmp_path):
    built, run = build_and_run("rot_host_checks", tmp_path)
    assert built.returncode == 0, built.stderr[-4000:]
    assert run.returncode == 0 and "rot host checks: ok" in run.stdout, (run.stdout[-4000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr, run.stderr[-4000:]
