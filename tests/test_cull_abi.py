"""CPU: the visual-block flags and ctvio_cull_visual are part of the C ABI (declared, exported, listed in capi.SYMBOLS, with prototypes;
ctvio_cull_options is 32 bytes with the header's field order on both sides, its defaults), and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ctvio_set_visual_active_batch", "ctvio_set_visual_active", "ctvio_get_visual_active_batch", "ctvio_get_visual_active",
           "ctvio_cull_visual_batch", "ctvio_cull_visual")

TU = """
#include <cstddef>
#include "ctvio.h"
static_assert(sizeof(ctvio_cull_options) == 32, "ctvio_cull_options");
static_assert(offsetof(ctvio_cull_options, min_redundancy) == 0 && offsetof(ctvio_cull_options, chi2_max) == 8 &&
              offsetof(ctvio_cull_options, mean_error_max) == 16 && offsetof(ctvio_cull_options, worst_only) == 24 &&
              offsetof(ctvio_cull_options, drop_uncomputable) == 28, "ctvio_cull_options field order");
int32_t (*const set_batch)(ctvio_solver *, const uint8_t *) = &ctvio_set_visual_active_batch;
int32_t (*const set_one)(ctvio_solver *, int32_t, const uint8_t *) = &ctvio_set_visual_active;
int32_t (*const get_batch)(ctvio_solver *, uint8_t *) = &ctvio_get_visual_active_batch;
int32_t (*const get_one)(ctvio_solver *, int32_t, uint8_t *) = &ctvio_get_visual_active;
int32_t (*const cull_batch)(ctvio_solver *, const ctvio_cull_options *, int32_t *, uint8_t *) = &ctvio_cull_visual_batch;
int32_t (*const cull_one)(ctvio_solver *, int32_t, const ctvio_cull_options *, int32_t *, uint8_t *) = &ctvio_cull_visual;
void (*const defaults)(ctvio_cull_options *) = &ctvio_default_cull_options;
"""


def test_symbols_exported_and_struct_mirrored(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    hdr = open(os.path.join(ROOT, "include", "ctvio.h")).read()
    for name in ENTRIES:
        assert name in cv.capi.SYMBOLS
        assert f"int32_t {name}(ctvio_solver *s" in hdr, name
        assert hasattr(lib, name), name
    assert "ctvio_default_cull_options" in cv.capi.SYMBOLS and hasattr(lib, "ctvio_default_cull_options")
    body = re.search(r"typedef struct ctvio_cull_options \{(.*?)\} ctvio_cull_options;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(double|int32_t)\s+(\w+);", body, re.M)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(cv.capi.CullOptions._fields_)
    assert C.sizeof(cv.capi.CullOptions) == 32
    co = C.POINTER(cv.capi.CullOptions)
    assert lib.ctvio_cull_visual_batch.argtypes == [C.c_void_p, co, C.c_void_p, C.c_void_p]
    assert lib.ctvio_cull_visual.argtypes == [C.c_void_p, C.c_int32, co, C.c_void_p, C.c_void_p]
    for f in ("set_visual_active", "visual_active", "cull_visual"):
        assert callable(getattr(cv.Solver, f)), f


def test_defaults(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    o = cv.capi.CullOptions(-1.0, -1.0, -1.0, 7, 7)
    lib.ctvio_default_cull_options(C.byref(o))
    assert (o.min_redundancy, o.chi2_max, o.mean_error_max, o.worst_only, o.drop_uncomputable) == (0.01, 9.21, 0.0, 0, 1)
    lib.ctvio_default_cull_options(None)      # (a null pointer is ignored)


def test_null_solver_is_refused_without_a_device(cv):
    cv.capi.build_library()
    lib = cv.capi.load_library()
    o = cv.capi.CullOptions()
    lib.ctvio_default_cull_options(C.byref(o))
    assert lib.ctvio_cull_visual_batch(None, C.byref(o), None, None) == 1
    assert lib.ctvio_cull_visual(None, 0, None, None, None) == 1
    assert lib.ctvio_set_visual_active_batch(None, None) == 1 and lib.ctvio_set_visual_active(None, 0, None) == 1
    assert lib.ctvio_get_visual_active_batch(None, None) == 1 and lib.ctvio_get_visual_active(None, 0, None) == 1


def test_header_compiles_standalone(tmp_path):
    src = tmp_path / "cull_tu.cpp"
    src.write_text(TU)
    for f in (str(src), os.path.join(ROOT, "tests", "cull_demo.cpp"), os.path.join(ROOT, "tests", "cull_adaptor_demo.cpp")):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), f])
