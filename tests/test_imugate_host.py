"""CPU: the host-buildable parts of ctvio_imu_gate_batch, compiled with g++ as a program of its own (tests/host_imugate_check.cpp): the
6 x 6 step of the epilogue (csrc/imugate6.hpp -- the function the device runs) on random symmetric A with eigenvalues in [0, 0.99], A = 0,
repeated eigenvalues and lambda_max above 1 - min_redundancy, against NumPy results passed through the program's arguments at the step's
own rounding (redundancy absolute 64 * 2^-53; chi2 and cov36 relative 64 * 2^-53 / redundancy); the slot map and the tile / slice planning
(csrc/host_pack.hpp) for odd M, M = 0 and an oversize window.  The program's own cases run once plainly and once under AddressSanitizer +
UBSan, as a plain executable."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"
SRC = os.path.join(HERE, "host_imugate_check.cpp")
HDRS = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp", "imugate6.hpp", "so3.hpp")] + \
       [os.path.join(HERE, "..", "include", "ctvio.h")]


def _build(out, flags):
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", ROCM_INC] + flags + ["-o", out, SRC, "-pthread"])
    return out


@pytest.fixture(scope="module")
def exe():
    return _build(os.path.join(HERE, "_build", "host_imugate_check"), [])


def sym(rng, ev):
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    A = (Q * np.asarray(ev, float)) @ Q.T
    return 0.5 * (A + A.T)


def step(exe, A, r, env=None):
    """Runs the program on (A, r) with NumPy's results as the expected values; returns its stdout."""
    M = np.eye(6) - A
    red = float(np.linalg.eigvalsh(M)[0])
    Mi = np.linalg.inv(M)
    cov = 0.5 * (Mi + Mi.T) - np.eye(6)
    chi = float(r @ np.linalg.solve(M, r))
    a21 = [A[i, j] for i in range(6) for j in range(i + 1)]
    args = [repr(float(x)) for x in a21 + list(r) + [red, chi] + list(cov.reshape(-1))]
    p = subprocess.run([exe, "step"] + args, capture_output=True, text=True, timeout=60, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr[-2000:], np.linalg.eigvalsh(A))
    return p.stdout, red


def test_step_random_spectra(exe):
    """Eigenvalues drawn from [0, 0.99]: 40 matrices; the worst use of each margin is printed."""
    rng = np.random.default_rng(3)
    worst = np.zeros(3)
    for _ in range(40):
        out, _ = step(exe, sym(rng, rng.uniform(0.0, 0.99, 6)), rng.standard_normal(6) * 3)
        assert "IMUGATE_STEP_OK" in out, out
        worst = np.maximum(worst, [float(x) for x in out.split("IMUGATE_STEP_OK")[1].split()])
    print(f"worst use of the margins (redundancy, chi2, cov36): {worst}")


@pytest.mark.parametrize("ev", [(0, 0, 0, 0, 0, 0), (0.5,) * 6, (0.3, 0.3, 0.3, 0.7, 0.7, 0.7), (0, 0, 0.98, 0.98, 0.5, 0.5), (0.2, 0.2, 0.2, 0.2, 0.2, 0.9),
                                (0.1, 0.2, 0.3, 0.4, 0.5, 0.98999), (1e-9, 1e-6, 1e-3, 0.1, 0.5, 0.9)],
                         ids=["zero", "six-fold", "two triples", "pairs at the ends", "five-fold", "near the threshold", "spread"])
def test_step_special_spectra(exe, ev):
    rng = np.random.default_rng(4)
    A = np.zeros((6, 6)) if not any(ev) else sym(rng, ev)
    out, _ = step(exe, A, rng.standard_normal(6))
    assert "IMUGATE_STEP_OK" in out, out
    out, _ = step(exe, np.diag(np.asarray(ev, float)), rng.standard_normal(6))      # (diagonal: nothing to rotate)
    assert "IMUGATE_STEP_OK" in out, out


@pytest.mark.parametrize("top", [0.995, 0.99999, 1.0, 1.0 + 1e-12])
def test_step_above_the_threshold(exe, top):
    """lambda_max(A) above 1 - min_redundancy, up to a not quite positive definite I - A (the weak sample of the GPU test: -1.6e-12): the
    redundancy alone is compared, and is below min_redundancy."""
    rng = np.random.default_rng(5)
    out, red = step(exe, sym(rng, (0.1, 0.3, 0.5, 0.7, 0.9, top)), rng.standard_normal(6))
    assert red < 0.01 and "redundancy" in out and "IMUGATE_STEP_OK" not in out, out


TILE_CASES = [
    ("odd M", 49152, [7], [(0, 1, 7, 4)], {0: 0}),
    ("M = 0 between windows", 49152, [80, 0, 501], [(0, 3, 581, 291)], {0: 0, 1: 40, 2: 40}),
    ("an oversize window", 128, [64, 1001, 64], [(0, 1, 64, 32), (1, 2, 1001, 501), (2, 3, 64, 32)], {0: 0, 1: 0, 2: 0}),
    ("only M = 0", 64, [0, 0], [(0, 2, 0, 0)], {0: 0, 1: 0}),
    ("slices of whole windows", 8, [5, 0, 3, 0, 0, 9], [(0, 5, 8, 5), (5, 6, 9, 5)], {0: 0, 1: 3, 2: 3, 3: 5, 4: 5, 5: 0}),
]


@pytest.mark.parametrize("what,budget,M,want,first", TILE_CASES, ids=[c[0] for c in TILE_CASES])
def test_tiles(exe, what, budget, M, want, first):
    """The slices (whole windows within the budget, an oversize window alone), each slice's tile count -- ceil(M / 2) per window, no tile
    straddles a window -- and every window's first tile; the program itself walks every tile through the device's lookup and checks that
    every sample is covered exactly once."""
    p = subprocess.run([exe, "tiles", str(budget)] + [str(x) for x in M], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = [x.split() for x in p.stdout.splitlines()]
    got = [tuple(int(v) for v in x) for x in lines if x[0] != "w"]
    got_first = {int(x[1]): int(x[2]) for x in lines if x[0] == "w"}
    assert got == want and got_first == first
    assert all(t == sum((m + 1) // 2 for m in M[a:b]) for a, b, _, t in got)


def test_own_cases(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "IMUGATE_HOST_OK 1017 cases" in p.stdout, (p.returncode, p.stdout[-500:])


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same program with AddressSanitizer + UBSan linked in, as a plain executable: its own cases and one step."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not installed")
    exe = _build(str(tmp_path / "imugate_asan"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "IMUGATE_HOST_OK 1017 cases" in p.stdout, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    rng = np.random.default_rng(6)
    out, _ = step(exe, sym(rng, rng.uniform(0.0, 0.99, 6)), rng.standard_normal(6), env)
    assert "IMUGATE_STEP_OK" in out
