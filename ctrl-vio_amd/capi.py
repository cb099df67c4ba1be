"""ctypes binding of libctvio.so (include/ctvio.h) -- plumbing only: every computation happens in the
HIP library.  There is NO CPU fallback: if the library is missing or no GPU is present, construction
raises (the product path must fail loudly, never silently compute elsewhere).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CTVIO_LIB_PATH") or os.path.join(_HERE, "libctvio.so")   # (CTVIO_LIB_PATH: another build of the same source -- compiler-flag A/B runs)
import glob
SRC = [os.path.join(_HERE, "csrc", "ctvio.hip")] + sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hpp")))   # every header is a dependency
HDR = os.path.join(os.path.dirname(_HERE), "include", "ctvio.h")

FP64 = 1   # the only precision (ctvio.h: the mixed fp32 mode was removed)
TERMINATION = {0: "max-iterations", 1: "gradient-tolerance", 2: "parameter-tolerance", 3: "function-tolerance", 4: "min-radius", 5: "failure"}


def hipcc_command(out: str, src: str) -> list:
    """The one hipcc line for device code of this project: libctvio.so and the test-only probe of the device math (tests/devprobe.py)
    are built with it, so a flag change reaches both."""
    return ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize",
            "-o", out, src]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc cross-compiles for gfx950 without a GPU; the .so is kept in-tree so it ships with the repo snapshot."""
    deps = SRC + [HDR]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(f) for f in deps):
        return LIB_PATH
    cmd = hipcc_command(LIB_PATH, SRC[0])
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return LIB_PATH


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("precision", C.c_int32), ("use_mfma", C.c_int32), ("check_every", C.c_int32),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_consecutive_invalid_steps", C.c_int32), ("deterministic", C.c_int32), ("host_threads", C.c_int32),
                ("use_graph", C.c_int32), ("line_search", C.c_int32)]


class CWindow(C.Structure):
    _fields_ = [
        ("K", C.c_int32), ("F", C.c_int32), ("L", C.c_int32), ("M", C.c_int32), ("NB", C.c_int32), ("V", C.c_int32),
        ("pn", C.c_int32), ("pnb", C.c_int32),
        ("t0_ns", C.c_int64), ("dt_ns", C.c_int64),
        ("quat", C.c_void_p), ("pos", C.c_void_p), ("bias", C.c_void_p), ("rho", C.c_void_p),
        ("ld", C.c_double), ("ld_lo", C.c_double), ("ld_hi", C.c_double),
        ("fix_ld", C.c_int32), ("lock_bg", C.c_int32), ("lock_ba", C.c_int32), ("fixed_upto", C.c_int32),
        ("q_CI", C.c_double * 4), ("p_CI", C.c_double * 3), ("gravity", C.c_double * 3), ("imu_w", C.c_double * 6),
        ("img_w", C.c_double), ("cauchy_a", C.c_double),
        ("imu_t", C.c_void_p), ("imu_gyro", C.c_void_p), ("imu_acc", C.c_void_p), ("imu_bias", C.c_void_p),
        ("bc_i", C.c_void_p), ("bc_j", C.c_void_p), ("bc_w", C.c_void_p),
        ("v_lm", C.c_void_p), ("v_ti", C.c_void_p), ("v_tj", C.c_void_p), ("v_rowi", C.c_void_p), ("v_rowj", C.c_void_p),
        ("v_pi", C.c_void_p), ("v_pj", C.c_void_p),
        ("pJ0", C.c_void_p), ("pr0", C.c_void_p), ("p_kind", C.c_void_p), ("p_index", C.c_void_p), ("p_off", C.c_void_p),
        ("p_x0", C.c_void_p), ("v_cauchy", C.c_void_p), ("knot_const", C.c_void_p),
    ]


class Summary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("num_successful", C.c_int32), ("num_unsuccessful", C.c_int32),
                ("termination", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_radius", C.c_double), ("num_line_search_steps", C.c_int32), ("num_line_search_reduced", C.c_int32)]

    def as_dict(self):
        return dict(iterations=self.iterations, num_successful=self.num_successful, num_unsuccessful=self.num_unsuccessful,
                    termination=TERMINATION.get(self.termination, "?"), initial_cost=self.initial_cost,
                    final_cost=self.final_cost, final_radius=self.final_radius,
                    num_line_search_steps=self.num_line_search_steps, num_line_search_reduced=self.num_line_search_reduced)


class TriangulateOptions(C.Structure):
    _fields_ = [("row_times", C.c_int32), ("only_unset", C.c_int32), ("apply", C.c_int32), ("min_depth", C.c_double), ("init_depth", C.c_double)]


class ImuNoise(C.Structure):
    _fields_ = [("gyr_n", C.c_double), ("acc_n", C.c_double), ("gyr_w", C.c_double), ("acc_w", C.c_double)]


class RowModel(C.Structure):
    _fields_ = [("fy", C.c_double), ("cy", C.c_double), ("rows", C.c_int32), ("iterations", C.c_int32)]


class GateOptions(C.Structure):
    _fields_ = [("min_redundancy", C.c_double)]


class CullOptions(C.Structure):
    _fields_ = [("min_redundancy", C.c_double), ("chi2_max", C.c_double), ("mean_error_max", C.c_double),
                ("worst_only", C.c_int32), ("drop_uncomputable", C.c_int32)]


# every symbol include/ctvio.h declares (tests check the .so exports all of them)
SYMBOLS = ["ctvio_default_options", "ctvio_status_string", "ctvio_last_error", "ctvio_device_count", "ctvio_create",
           "ctvio_destroy", "ctvio_clear", "ctvio_add_window", "ctvio_upload", "ctvio_set_batch", "ctvio_num_windows", "ctvio_solve",
           "ctvio_get_state", "ctvio_get_batch_state", "ctvio_set_state", "ctvio_snapshot_state", "ctvio_restore_state", "ctvio_linearize", "ctvio_cost", "ctvio_lm_step", "ctvio_spline_eval", "ctvio_sensor_pose", "ctvio_gauge_restore", "ctvio_marginalize", "ctvio_marginalize_batch", "ctvio_residual_summary",
           "ctvio_last_timing", "ctvio_set_profiling", "ctvio_stream", "ctvio_solve_sharded", "ctvio_sharded_release", "ctvio_shard_of",
           "ctvio_shard_count", "ctvio_shards_used", "ctvio_spline_eval_batch", "ctvio_graph_captures", "ctvio_marginalize_ran_on_host",
           "ctvio_covariance_batch", "ctvio_covariance", "ctvio_pose_covariance_batch", "ctvio_pose_covariance",
           "ctvio_landmark_points_batch", "ctvio_landmark_points", "ctvio_nav_state_batch", "ctvio_nav_state",
           "ctvio_relative_pose_batch", "ctvio_relative_pose", "ctvio_project_landmarks_batch", "ctvio_project_landmarks",
           "ctvio_default_imu_noise", "ctvio_imu_predict_batch", "ctvio_imu_predict", "ctvio_body_rates_batch", "ctvio_body_rates",
           "ctvio_predict_landmarks_batch", "ctvio_predict_landmarks",
           "ctvio_default_gate_options", "ctvio_visual_gate_batch", "ctvio_visual_gate", "ctvio_imu_gate_batch", "ctvio_imu_gate",
           "ctvio_set_visual_active_batch", "ctvio_set_visual_active", "ctvio_get_visual_active_batch", "ctvio_get_visual_active",
           "ctvio_default_cull_options", "ctvio_cull_visual_batch", "ctvio_cull_visual",
           "ctvio_default_triangulate_options", "ctvio_triangulate_batch", "ctvio_triangulate", "ctvio_shift_anchor_batch"]

_lib = None


def load_library():
    """dlopen libctvio.so (raises if it has not been built -- no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
        lib = C.CDLL(LIB_PATH)
        lib.ctvio_status_string.restype = C.c_char_p
        lib.ctvio_last_error.restype = C.c_char_p
        lib.ctvio_stream.restype = C.c_void_p
        lib.ctvio_create.argtypes = [C.POINTER(Options), C.POINTER(C.c_void_p)]
        lib.ctvio_destroy.argtypes = [C.c_void_p]
        for name in ("ctvio_clear", "ctvio_upload", "ctvio_num_windows", "ctvio_snapshot_state", "ctvio_restore_state"):
            getattr(lib, name).argtypes = [C.c_void_p]
        lib.ctvio_add_window.argtypes = [C.c_void_p, C.POINTER(CWindow), C.POINTER(C.c_int32)]
        lib.ctvio_set_batch.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ctvio_get_batch_state.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        lib.ctvio_solve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ctvio_get_state.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
        lib.ctvio_set_state.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_double]
        lib.ctvio_linearize.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
        lib.ctvio_cost.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ctvio_lm_step.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
        lib.ctvio_spline_eval.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        lib.ctvio_sensor_pose.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
        lib.ctvio_marginalize.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_double] + [C.c_void_p] * 4
        lib.ctvio_marginalize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 4
        lib.ctvio_residual_summary.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        lib.ctvio_gauge_restore.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4
        lib.ctvio_last_timing.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        lib.ctvio_set_profiling.argtypes = [C.c_void_p, C.c_int32]
        lib.ctvio_stream.argtypes = [C.c_void_p]
        lib.ctvio_graph_captures.argtypes = [C.c_void_p]
        lib.ctvio_marginalize_ran_on_host.argtypes = [C.c_void_p]
        lib.ctvio_solve_sharded.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 6
        lib.ctvio_shard_of.argtypes = [C.c_int32, C.c_int32]
        lib.ctvio_shard_count.argtypes = [C.c_int32, C.c_int32, C.c_int32]
        lib.ctvio_shards_used.argtypes = [C.c_int32, C.c_int32]
        lib.ctvio_spline_eval_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 7
        lib.ctvio_covariance_batch.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        lib.ctvio_covariance.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4
        lib.ctvio_pose_covariance_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        lib.ctvio_pose_covariance.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        lib.ctvio_landmark_points_batch.argtypes = [C.c_void_p] + [C.c_void_p] * 3
        lib.ctvio_landmark_points.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 3
        lib.ctvio_nav_state_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6
        lib.ctvio_nav_state.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        lib.ctvio_body_rates_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
        lib.ctvio_body_rates.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
        lib.ctvio_relative_pose_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 8
        lib.ctvio_relative_pose.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7
        lib.ctvio_project_landmarks_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.POINTER(RowModel)] + [C.c_void_p] * 6
        lib.ctvio_project_landmarks.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.POINTER(RowModel)] + [C.c_void_p] * 6
        lib.ctvio_default_imu_noise.argtypes = [C.POINTER(ImuNoise)]
        lib.ctvio_default_imu_noise.restype = None
        lib.ctvio_imu_predict_batch.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.POINTER(ImuNoise), C.c_int32] + [C.c_void_p] * 3
        lib.ctvio_imu_predict.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.POINTER(ImuNoise), C.c_int32] + [C.c_void_p] * 3
        lib.ctvio_predict_landmarks_batch.argtypes = ([C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.POINTER(ImuNoise), C.c_int64] + [C.c_void_p] * 3 +
                                                      [C.POINTER(RowModel)] + [C.c_void_p] * 7)
        lib.ctvio_predict_landmarks.argtypes = ([C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.POINTER(ImuNoise), C.c_int32] +
                                                [C.c_void_p] * 2 + [C.POINTER(RowModel)] + [C.c_void_p] * 7)
        lib.ctvio_default_gate_options.argtypes = [C.POINTER(GateOptions)]
        lib.ctvio_default_gate_options.restype = None
        lib.ctvio_visual_gate_batch.argtypes = [C.c_void_p, C.POINTER(GateOptions)] + [C.c_void_p] * 9
        lib.ctvio_visual_gate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GateOptions)] + [C.c_void_p] * 9
        lib.ctvio_imu_gate_batch.argtypes = [C.c_void_p, C.POINTER(GateOptions)] + [C.c_void_p] * 6
        lib.ctvio_imu_gate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(GateOptions)] + [C.c_void_p] * 6
        lib.ctvio_set_visual_active_batch.argtypes = [C.c_void_p, C.c_void_p]
        lib.ctvio_set_visual_active.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ctvio_get_visual_active_batch.argtypes = [C.c_void_p, C.c_void_p]
        lib.ctvio_get_visual_active.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.ctvio_default_cull_options.argtypes = [C.POINTER(CullOptions)]
        lib.ctvio_default_cull_options.restype = None
        lib.ctvio_cull_visual_batch.argtypes = [C.c_void_p, C.POINTER(CullOptions), C.c_void_p, C.c_void_p]
        lib.ctvio_cull_visual.argtypes = [C.c_void_p, C.c_int32, C.POINTER(CullOptions), C.c_void_p, C.c_void_p]
        lib.ctvio_default_triangulate_options.argtypes = [C.POINTER(TriangulateOptions)]
        lib.ctvio_default_triangulate_options.restype = None
        lib.ctvio_triangulate_batch.argtypes = [C.c_void_p, C.POINTER(TriangulateOptions), C.c_void_p, C.c_void_p]
        lib.ctvio_triangulate.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TriangulateOptions), C.c_void_p, C.c_void_p]
        lib.ctvio_shift_anchor_batch.argtypes = [C.c_void_p, C.POINTER(TriangulateOptions), C.c_int64] + [C.c_void_p] * 6
        _lib = lib
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def to_cwindow(w, keep):
    """Window (ctrl-vio_amd/window.py) -> ctvio_window.  `keep` collects arrays that must outlive the call."""
    w.normalize()
    pJ0_cm = np.asfortranarray(w.pJ0)
    keep.append(pJ0_cm)
    c = CWindow()
    c.K, c.F, c.L, c.M, c.NB, c.V = w.K, w.F, w.L, w.M, w.NB, w.V
    c.pn, c.pnb = w.pn, int(w.p_kind.shape[0])
    c.t0_ns, c.dt_ns = w.t0_ns, w.dt_ns
    c.quat, c.pos, c.bias, c.rho = _p(w.quat), _p(w.pos), _p(w.bias), _p(w.rho)
    c.ld, c.ld_lo, c.ld_hi = w.ld, w.ld_lo, w.ld_hi
    c.fix_ld, c.lock_bg, c.lock_ba, c.fixed_upto = int(w.fix_ld), int(w.lock_bg), int(w.lock_ba), int(w.fixed_upto)
    c.q_CI[:] = w.q_CI.tolist(); c.p_CI[:] = w.p_CI.tolist(); c.gravity[:] = w.gravity.tolist(); c.imu_w[:] = w.imu_w.tolist()
    c.img_w, c.cauchy_a = w.img_w, w.cauchy_a
    c.imu_t, c.imu_gyro, c.imu_acc, c.imu_bias = _p(w.imu_t), _p(w.imu_gyro), _p(w.imu_acc), _p(w.imu_bias)
    c.bc_i, c.bc_j, c.bc_w = _p(w.bc_i), _p(w.bc_j), _p(w.bc_w)
    c.v_lm, c.v_ti, c.v_tj = _p(w.v_lm), _p(w.v_ti), _p(w.v_tj)
    c.v_rowi, c.v_rowj, c.v_pi, c.v_pj = _p(w.v_rowi), _p(w.v_rowj), _p(w.v_pi), _p(w.v_pj)
    c.pJ0 = pJ0_cm.ctypes.data_as(C.c_void_p) if w.pn else None
    c.pr0, c.p_kind, c.p_index, c.p_off, c.p_x0 = _p(w.pr0), _p(w.p_kind), _p(w.p_index), _p(w.p_off), _p(w.p_x0)
    c.v_cauchy = _p(w.v_cauchy) if w.v_cauchy is not None else None
    c.knot_const = _p(w.knot_const) if w.knot_const is not None else None
    return c


class CtvioError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        lib = load_library()
        raise CtvioError(f"{lib.ctvio_status_string(rc).decode()} ({rc}): {lib.ctvio_last_error().decode()}")
