"""CPU: the packer writes every staged byte.  The host-only steps of a batch upload (csrc/host_pack.hpp: plan, offsets, input-arena layout,
fill -- the functions SolverImpl::pack_and_upload calls), compiled with g++ for the test only (tests/host_staging_check.cpp), pack the batch
over 0x00 and over 0xFF: the staging arena is reused, so a byte the packer leaves alone would carry the previous batch to the device, and
the filled extent of every segment must agree between the two packs.  (On the GPU the upload runs the same check under CTVIO_POISON.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROCM_INC = "/opt/rocm/include"
VIS_STAGE = 8 * 116 * 9 * 8 + 8 * 2 * 8 * 4      # kernels_assemble.hpp: vis_stage_bytes(8, 8)


@pytest.fixture(scope="module")
def hs():
    if not os.path.isdir(ROCM_INC):
        pytest.skip("HIP headers not found")
    out = os.path.join(HERE, "_build", "libhoststaging.so")
    src = os.path.join(HERE, "host_staging_check.cpp")
    hdrs = [os.path.join(HERE, "..", "ctrl-vio_amd", "csrc", f) for f in ("host_pack.hpp", "device_types.hpp")] + [os.path.join(HERE, "..", "include", "ctvio.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(f) > os.path.getmtime(out) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-I", ROCM_INC, "-o", out, src, "-L/opt/rocm/lib", "-lamdhip64",
                               "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    lib = C.CDLL(out)
    lib.hs_pack.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_int] + [C.c_void_p] * 5 + [C.c_char_p, C.c_int]
    return lib


def pack(hs, cv, wins, deterministic2=False, dense=False, threads=4):
    """-> (rc, message, walk, [(name, offset, filled bytes, hash)])"""
    keep = []
    arr = (cv.capi.CWindow * len(wins))(*[cv.capi.to_cwindow(w, keep) for w in wins])
    n = hs.hs_nseg()
    name = (C.c_char_p * n)(); off = np.zeros(n, np.uint64); nbytes = np.zeros(n, np.uint64); h = np.zeros(n, np.uint64)
    walk = C.c_int32(); err = C.create_string_buffer(256)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    rc = hs.hs_pack(len(wins), C.cast(arr, C.c_void_p), int(deterministic2), int(dense), VIS_STAGE, threads, C.cast(name, C.c_void_p), p(off), p(nbytes), p(h),
                    C.byref(walk), err, 256)
    return rc, err.value.decode(), walk.value, [(name[i].decode(), int(off[i]), int(nbytes[i]), int(h[i])) for i in range(n)]


def _without_imu(w):
    w.imu_t = w.imu_t[:0]; w.imu_gyro = w.imu_gyro[:0]; w.imu_acc = w.imu_acc[:0]; w.imu_bias = w.imu_bias[:0]
    w.normalize()
    return w


def _without_blocks(w):
    z = lambda a: a[:0]
    w.v_lm, w.v_ti, w.v_tj, w.v_rowi, w.v_rowj, w.v_pi, w.v_pj = z(w.v_lm), z(w.v_ti), z(w.v_tj), z(w.v_rowi), z(w.v_rowj), z(w.v_pi), z(w.v_pj)
    w.normalize()
    return w


def _cases(cv):
    mk = cv.synth.make_window
    return {
        "tiny": ([mk("tiny", seed=3)], {}),
        "config1": ([mk("config1", seed=1001)], {}),
        "config2": ([mk("config2", seed=1000)], {}),
        "prior_free": ([mk("config1", seed=1002, with_prior=False)], {}),
        "no_imu": ([_without_imu(mk("config1", seed=1003))], {}),
        "no_blocks": ([_without_blocks(mk("config1", seed=1004))], {}),
        "config5_row_walk": ([mk("config5", seed=1011)], dict(deterministic2=True)),
        "mixed3": ([mk("tiny", seed=42, with_prior=False), _without_blocks(mk("config1", seed=1005)), mk("config1", seed=1200, F=10, dt_ns=40_000_000)],
                   dict(deterministic2=True)),
    }


CASES = ["tiny", "config1", "config2", "prior_free", "no_imu", "no_blocks", "config5_row_walk", "mixed3"]


@pytest.mark.parametrize("case", CASES)
def test_packer_writes_every_staged_byte(hs, cv, case):
    wins, kw = _cases(cv)[case]
    rc, msg, walk, segs = pack(hs, cv, wins, **kw)
    assert rc == 0, msg
    # the layout: 256-byte aligned segments, in list order, the filled extent inside the segment
    names = [s[0] for s in segs]
    assert len(set(names)) == len(names) and names[0] == "meta" and names[-1] == "vrow_off"
    for (_, o, nb, _), nxt in zip(segs, segs[1:]):
        assert o % 256 == 0 and o + nb <= nxt[1]
    by = {s[0]: s for s in segs}
    if case == "no_imu":
        assert wins[0].M == 0 and by["imu_u"][2] == 0 and by["groups"][2] == 0
    if case == "no_blocks":
        assert wins[0].V == 0 and by["v_win"][2] == 0 and by["vitems"][2] == 0
    if case == "prior_free":
        assert by["pH"][2] == 0 and by["pcol"][2] == 0
    # the row walk is packed exactly when deterministic = 2 meets a window beyond the LDS-resident Hessian (K > 25)
    assert walk == int(bool(kw.get("deterministic2")) and max(w.K for w in wins) > 25)
    assert (by["vrow"][2] > 0) == bool(walk) and (by["vrow_off"][2] > 0) == bool(walk)
    # the pack does not depend on how the windows are spread over the host threads
    rc1, msg1, _, segs1 = pack(hs, cv, wins, threads=1, **kw)
    assert rc1 == 0 and segs1 == segs
