"""CPU: the slice planner of ctvio_visual_gate_batch (csrc/host_pack.hpp: plan_gate_slices), compiled with g++ as a program of its own
(tests/host_gateslice_check.cpp).  Given cases through its arguments: budgets that give one slice, many slices, one window per slice, an
oversize window, empty windows; every window lands in exactly one slice and the order is preserved.  The program's own cases run once
plainly and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"
SRC = os.path.join(HERE, "host_gateslice_check.cpp")
HDRS = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]


def _build(out, flags):
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", ROCM_INC] + flags + ["-o", out, SRC, "-pthread"])
    return out


@pytest.fixture(scope="module")
def exe():
    return _build(os.path.join(HERE, "_build", "host_gateslice_check"), [])


def slices(exe, budget, n, wbeg=0, wend=None):
    wend = len(n) if wend is None else wend
    p = subprocess.run([exe, str(budget), str(wbeg), str(wend)] + [str(x) for x in n], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)
    return [tuple(int(x) for x in line.split()) for line in p.stdout.splitlines()]


CASES = [
    ("one slice", 65536, [64, 128, 64, 256], [(0, 4, 512)]),
    ("many slices", 192, [64, 128, 64, 256], [(0, 2, 192), (2, 3, 64), (3, 4, 256)]),
    ("one window per slice", 64, [64, 64, 64, 64], [(0, 1, 64), (1, 2, 64), (2, 3, 64), (3, 4, 64)]),
    ("an oversize window", 128, [64, 1024, 64], [(0, 1, 64), (1, 2, 1024), (2, 3, 64)]),
    ("empty windows", 64, [0, 0, 64, 0, 64, 0], [(0, 4, 64), (4, 6, 64)]),
    ("only empty windows", 64, [0, 0, 0], [(0, 3, 0)]),
]


@pytest.mark.parametrize("what,budget,n,want", CASES, ids=[c[0] for c in CASES])
def test_given_cases(exe, what, budget, n, want):
    got = slices(exe, budget, n)
    assert got == want
    assert [w for a, b, _ in got for w in range(a, b)] == list(range(len(n)))      # every window once, in order
    assert all(s == sum(n[a:b]) for a, b, s in got)
    assert all(s <= budget or sum(1 for x in n[a:b] if x) == 1 for a, b, s in got)


def test_sub_range(exe):
    """The single-window entry and a sub-range of the batch."""
    assert slices(exe, 128, [64, 128, 64, 256], 1, 3) == [(1, 2, 128), (2, 3, 64)]
    assert slices(exe, 1, [64, 128, 64, 256], 2, 3) == [(2, 3, 64)]
    assert slices(exe, 64, [64], 0, 0) == []


def test_own_cases(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "GATESLICE_OK 2009 cases" in p.stdout, (p.returncode, p.stdout[-500:])


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer + UBSan linked in, as a plain executable."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    exe = _build(str(tmp_path / "gateslice_asan"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1"))
    assert p.returncode == 0 and "GATESLICE_OK 2009 cases" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
