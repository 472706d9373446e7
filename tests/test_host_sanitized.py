"""The codec's host code under AddressSanitizer + UndefinedBehaviorSanitizer, without Python in the process and
without a GPU: tests/host_checks.hip (a stand-alone program that includes coalac.hip) is built with the host
sanitizers and run as a child process (tests/host_program.py). It covers what returns before any device call — plan
validation, the NULL-argument cases of every entry point, every COALAC_EINVAL case of coalac_pack_dense,
coalac_unpack_dense and coalac_decode_packed — and the workspace / plan-table walks on host buffers of exactly the
measured size."""
from tests.host_program import build_and_run


def test_host_code_is_clean_under_sanitizers(tmp_path):
    built, run = build_and_run("host_checks", tmp_path)
    assert built.returncode == 0, built.stderr[-4000:]
    assert run.returncode == 0 and "host checks: ok" in run.stdout, (run.stdout[-4000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error:" not in run.stderr, run.stderr[-4000:]
