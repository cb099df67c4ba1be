"""CPU: the line-search interpolation of the device (ctrl-vio_amd/csrc/ls_poly.hpp: ls_minimize_interpolating, ls_root_real_parts,
ls_poly_eval), compiled with g++ for the test only (tests/host_lspoly_check.cpp) and compared with NumPy's solve / roots in the convention of
tests/test_oracle_linesearch.py::test_interpolating_polynomial_minimiser, which checks the oracle's copy of the algorithm.  The same cases
run on the gfx950 build in tests/test_gpu_device_math.py (tests/ls_cases.py holds them)."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def host():
    import devprobe
    return devprobe.Host()


@pytest.mark.parametrize("ns", [2, 3])
def test_interpolating_minimiser_matches_numpy(host, ns):
    """300 seeded cases: lo <= x <= hi and |p(x) - best| <= 1e-9 max(1, |best|)."""
    import ls_cases
    ls_cases.check_against_reference(host, ns, *ls_cases.random_cases(ns), label=f"host, {ns} samples")


def test_interpolating_minimiser_edges(host):
    """Coincident abscissae (singular system: the midpoint exactly), lo == hi, constant data (the derivative trimmed to nothing), a nearly
    degenerate quadratic derivative, a derivative with a complex pair, a quintic with four real critical points inside the interval."""
    import ls_cases
    ls_cases.check_edges(host, "host")


def test_exactly_quadratic_data_trims_the_derivative(host):
    """The cubic's leading coefficient is an exact zero, the derivative is trimmed to a line and the result is that line's root, to the bit."""
    import ls_cases
    ls_cases.check_trimming(host, "host")


def test_root_real_parts(host):
    """ls_root_real_parts directly: trimming, deg == 1, both orders of the quadratic formula, Durand-Kerner, against numpy.roots."""
    import ls_cases
    ls_cases.check_roots(host, "host")
