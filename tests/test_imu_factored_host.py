"""CPU: the staged IMU functions of ctrl-vio_amd/csrc/factors.hpp that the fast body of k_imu_linearize_f64 is made of -- compact rows in
pair-log coordinates, accelerometer rows rotated into the world frame, the group transform T^T G^ T, the lamA-weighted sums of the position
columns -- compiled with g++ for the test only (tests/host_imufactored_check.cpp), assembled into the 32 x 32 group tile and compared with
the tile accumulated directly from imu_eval_core's Jacobian: every entry scaled by sqrt(H_ii H_jj), bound 1e-10 (the project's bound for
normal equations in fp64).  Random groups of 1 .. 130 samples, isotropic accelerometer weights, knot-pair logs up to 0.49 rad."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_imufactored_check.cpp")
HDRS = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("so3.hpp", "factors.hpp")]


@pytest.fixture(scope="module")
def hf():
    out = os.path.join(HERE, "_build", "libhostimufactored.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", out, SRC])
    lib = C.CDLL(out)
    lib.hm_imufactored_case.argtypes = [C.c_uint64, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    lib.hm_imufactored_case.restype = C.c_double
    return lib


def test_factored_tile_matches_direct_accumulation(hf):
    worst, at = 0.0, None
    seed = 1000
    for n in (1, 2, 3, 4, 5, 17, 63, 64, 65, 100, 128, 129, 130):
        for max_log in (1e-9, 0.01, 0.1, 0.3, 0.49):
            for _ in range(3):
                seed += 1
                new, ref = np.zeros((32, 32)), np.zeros((32, 32))
                e = hf.hm_imufactored_case(seed, n, max_log, new.ctypes.data_as(C.c_void_p), ref.ctypes.data_as(C.c_void_p))
                # the same figure from the two tiles, so that the bound does not rest on the C side's arithmetic alone
                sc = np.sqrt(np.diag(ref)[:31])
                assert (sc > 0).all()
                e2 = np.abs((new[:31, :31] - ref[:31, :31]) / np.outer(sc, sc)).max()
                assert e == pytest.approx(e2, rel=1e-6, abs=1e-18)
                assert np.array_equal(new, new.T)
                assert not new[31].any() and not new[:, 31].any()
                if e2 > worst:
                    worst, at = e2, (n, max_log, seed)
    # knot columns are differences of two pair terms (-M_i JrI_i^T + M_(i-1) JrI_(i-1)): the margin the transform leaves
    print(f"worst scaled difference {worst:.3g} at (samples, log, seed) = {at}")
    assert worst <= 1e-10


def test_stand_alone_program_under_sanitizers(tmp_path):
    """The same cases as a program of its own with AddressSanitizer and UBSan (the staged functions index small fixed arrays)."""
    exe = str(tmp_path / "imufactored_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DIMUFACTORED_MAIN",
                           "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
