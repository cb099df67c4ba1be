"""CPU: the host helpers the query entries share (csrc/host_pack.hpp: ImuSamples, check_frame, check_count, gate_scatter), compiled with
g++ as a program of its own (tests/host_querypack_check.cpp): the IMU sample streams of 2 queries of 1 and 3 samples accepted and rejected
once per error string, and the status table of the two leave-one-out gates for every status x failed factorisation.  The program runs
once plainly and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"
SRC = os.path.join(HERE, "host_querypack_check.cpp")
HDRS = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]


def _build(out, flags):
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", ROCM_INC] + flags + ["-o", out, SRC, "-pthread"])
    return out


def _run(exe, **env):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert p.returncode == 0 and "QUERYPACK_OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-3000:])


def test_own_cases():
    _run(_build(os.path.join(HERE, "_build", "host_querypack_check"), []))


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer + UBSan linked in, as a plain executable."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    _run(_build(str(tmp_path / "querypack_asan"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
         ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
