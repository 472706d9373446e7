"""Build one of the stand-alone host-check programs (tests/*.hip: a main() over the included coalac.hip) with
AddressSanitizer + UndefinedBehaviorSanitizer on the host side, and run it as a child process: no Python and no GPU in
that process. The device code in the binary is never run (built at -O0 to keep the compile short). The assertions stay
with the tests that call this."""
import os
import subprocess

from coala_amd import _build

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZE = "-fsanitize=address,undefined"


def build_and_run(name, tmp_path, *args):
    """Compile tests/<name>.hip into tmp_path and, if that worked, run it with `args`: (the build's CompletedProcess,
    the run's or None)."""
    exe = str(tmp_path / name)
    cmd = [_build.hipcc(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", f"--offload-arch={_build.ARCH}",
           "-Xarch_device", "-O0", "-Xarch_device", "-g0", "-Xarch_host", SANITIZE,
           "-Xarch_host", "-fno-sanitize-recover=undefined", SANITIZE,  # (the last one: the link's runtime)
           "-Wno-option-ignored", "-Wno-pass-failed", "-o", exe, os.path.join(HERE, name + ".hip")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0:
        return built, None
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return built, subprocess.run([exe, *args], capture_output=True, text=True, env=env, timeout=120)
