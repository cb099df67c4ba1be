"""The cases of the line-search interpolation (ctrl-vio_amd/csrc/ls_poly.hpp: ls_minimize_interpolating) and their check against NumPy's
solve / roots, written once for the g++ build (tests/test_ls_poly_host.py) and the gfx950 build (tests/test_gpu_device_math.py).  `impl` is
devprobe.Host or devprobe.Device.  The polynomial's VALUE at the returned abscissa is compared with the reference's best value, never the
abscissa itself: it is ill-conditioned wherever the polynomial is flat."""
import numpy as np

from test_oracle_linesearch import _ref_step

RTOL = 1e-9   # |p(x) - best| <= RTOL max(1, |best|): the convention of test_oracle_linesearch.py::test_interpolating_polynomial_minimiser


def random_cases(ns, n=300):
    """the generator of test_interpolating_polynomial_minimiser: samples at 0 and at ns - 1 decreasing abscissae, the interval of a contraction"""
    rng = np.random.default_rng(ns)
    x, v, g, lo, hi = [], [], [], [], []
    for _ in range(n):
        xi = np.concatenate([[0.0], np.sort(rng.uniform(0.05, 1.0, ns - 1))[::-1]])
        x.append(xi); v.append(rng.normal(size=ns)); g.append(rng.normal(size=ns))
        lo.append(1e-3 * xi[1]); hi.append(0.6 * xi[1])
    return np.array(x), np.array(v), np.array(g), np.array(lo), np.array(hi)


def check_against_reference(impl, ns, x, v, g, lo, hi, label):
    got = impl.ls_minimize(ns, x, v, g, lo, hi)
    worst = 0.0
    for i in range(len(lo)):
        c, best = _ref_step(x[i], v[i], g[i], lo[i], hi[i])
        assert lo[i] <= got[i] <= hi[i], (label, i, got[i], lo[i], hi[i])
        worst = max(worst, abs(np.polyval(c, got[i]) - best) / (RTOL * max(1.0, abs(best))))
    print(f"{label}: worst |p(x) - best| over bound {worst:.3g}")
    assert worst <= 1.0, (label, worst)
    return worst


def _samples(coef, xs):
    """values and gradients of the polynomial (highest power first) at xs: the data its interpolant reproduces"""
    xs = np.array(xs, float)
    return xs, np.polyval(coef, xs), np.polyval(np.polyder(coef), xs)


def edge_cases():
    """(name, ns, x, v, g, lo, hi)"""
    cases = []
    rng = np.random.default_rng(11)
    # lo == hi: the only admissible abscissa
    cases.append(("lo == hi, 2 samples", 2, np.array([0.0, 0.8]), rng.normal(size=2), rng.normal(size=2), 0.2, 0.2))
    cases.append(("lo == hi, 3 samples", 3, np.array([0.0, 0.8, 0.5]), rng.normal(size=3), rng.normal(size=3), 0.3, 0.3))
    # two samples of a constant: every coefficient but the last vanishes and ls_root_real_parts trims the derivative to nothing.  (The
    # exactly quadratic data whose cubic coefficient comes out as an exact zero, so that the derivative is trimmed to a line, has a check
    # of its own: check_trimming.)  Sampled at 0 and 0.5 the same quadratic leaves a cubic coefficient of -1.2e-15 (the elimination's factor
    # is 1 / 6): a nearly degenerate quadratic for the deg == 2 formula, whose other root lies at 1e15
    cases.append(("constant data", 2, np.array([0.0, 0.75]), np.array([1.5, 1.5]), np.zeros(2), 0.05, 0.7))
    cases.append(("nearly degenerate quadratic derivative" + AT_ROOT, 2) + _samples(QUADRATIC, [0.0, 0.5]) + (0.05, 0.4))
    # a derivative with a complex pair: a monotone cubic (two samples: the quadratic formula's D < 0 branch), and a quintic whose quartic
    # derivative (x^2 + 1)(x - 0.3)(x - 0.6) has two real and two complex roots (three samples: Durand-Kerner)
    cases.append(("cubic, complex pair", 2) + _samples([1.0, 0.0, 1.0, 0.0], [0.0, 1.0]) + (0.1, 0.9))
    # (the interval starts past the maximum at 0.3: the minimum over it is the root 0.6, not an end)
    d4 = np.polymul([1.0, 0.0, 1.0], np.polymul([1.0, -0.3], [1.0, -0.6]))
    cases.append(("quintic, complex pair" + AT_ROOT, 3) + _samples(np.polyint(d4), [0.0, 1.0, 0.5]) + (0.25, 0.9))
    # a quintic whose derivative has all four real roots inside the interval: minima at 0.4 and 0.8 (the lower one), and with the sign
    # flipped at 0.2 (the lower one) and 0.6; the intervals and samples keep the ends and the samples above the lower minimum
    d4 = 30.0 * np.poly([0.2, 0.4, 0.6, 0.8])
    cases.append(("quintic, four real roots inside" + AT_ROOT, 3) + _samples(np.polyint(d4), [0.0, 1.0, 0.5]) + (0.15, 0.9))
    cases.append(("quintic, four real roots inside, sign flipped" + AT_ROOT, 3) + _samples(np.polyint(-d4), [0.0, 1.0, 0.3]) + (0.1, 0.85))
    return cases


AT_ROOT = " (minimum at a root)"
QUADRATIC = [2.0, -1.0, 0.5]   # 2 x^2 - x + 0.5: minimum 0.375 at 0.25


def check_edges(impl, label):
    worst = 0.0
    for name, ns, x, v, g, lo, hi in edge_cases():
        if name.endswith(AT_ROOT):   # the case is about the roots: no other candidate (midpoint, ends, samples) may come near the minimum
            c, best = _ref_step(x, v, g, lo, hi)
            others = [0.5 * (lo + hi), lo, hi] + [xi for xi in x if lo <= xi <= hi]
            assert best < min(np.polyval(c, z) for z in others) - 5e-5, name
        worst = max(worst, check_against_reference(impl, ns, x[None], v[None], g[None], np.array([lo]), np.array([hi]), f"{label}, {name}"))
    # coincident abscissae: the 2 ns x 2 ns system is singular (two pairs of equal rows cancel to exact zeros in the elimination) and the
    # minimiser falls back to the midpoint of the interval, exactly
    for ns, x in ((2, [0.3, 0.3]), (3, [0.0, 0.4, 0.4])):
        rng = np.random.default_rng(ns)
        v, g = rng.normal(size=ns), rng.normal(size=ns)
        v[-1], g[-1] = v[-2], g[-2]
        got = impl.ls_minimize(ns, np.array([x]), v[None], g[None], np.array([0.01]), np.array([0.25]))
        assert got[0] == 0.5 * (0.01 + 0.25), (label, ns, got)
    return worst


def check_trimming(impl, label):
    """Exactly quadratic data at abscissae for which the elimination is exact in fp64 (dyadic data, dyadic factors: also under fma): the
    interpolating cubic's leading coefficient is an exact zero, the derivative [0, 4, -1] is trimmed to the line 4 x - 1, and the result is
    that line's root -(-1) / 4 to the bit.  The coefficients come back from the implementation itself, so the case shows that the trimming
    ran and cannot degrade into the deg == 2 formula unnoticed."""
    for x1 in (0.75, 1.0, 1.5, 3.0):
        x, v, g = _samples(QUADRATIC, [0.0, x1])
        got, coef = impl.ls_minimize(2, x[None], v[None], g[None], np.array([0.05]), np.array([0.4]), coef=True)
        assert np.array_equal(coef[0], [0.0, 2.0, -1.0, 0.5, 0.0, 0.0]), (label, x1, coef[0])
        assert got[0] == 0.25, (label, x1, got[0])
    print(f"{label}: exactly quadratic data: cubic coefficient 0, result the trimmed line's root 0.25, to the bit")


def check_roots(impl, label):
    """ls_root_real_parts on its own, every branch: leading zeros trimmed to nothing, to a constant, to a line (deg == 1: -p1 / p0, exact
    for dyadic data), to a quadratic (both orders of the stable formula, and a complex pair: the real part twice); Durand-Kerner for
    cubics and quartics, with and without complex pairs, against numpy.roots at 1e-12 of the largest root (simple, well separated
    roots: the iteration stops at a change of 1e-15 of the root bound)."""
    def run(p):
        cnt, re = impl.ls_roots(np.array([p], float))
        return int(cnt[0]), re[0]
    for p in ([0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 5.0], [7.0]):
        assert run(p)[0] == 0, (label, p)
    for p, root in (([0.0, 4.0, -1.0], 0.25), ([0.0, 0.0, 0.0, -2.0, 3.0], 1.5), ([8.0, 1.0], -0.125)):   # a wrong sign in deg == 1 fails here
        n, re = run(p)
        assert n == 1 and re[0] == root and np.isnan(re[1:]).all(), (label, p, n, re)
    worst = 0.0
    polys = [[0.0, 2.0, -3.0, 1.0], [0.0, 0.0, 1.0, 3.0, 2.0], [1.0, -3.0, 2.0], [1.0, 2.0, 5.0],                       # quadratics: b < 0, b > 0, D < 0
             list(np.poly([0.2, 0.5, 0.9])), list(np.poly([-1.5, 0.25, 2.0])), list(np.polymul([1.0, 0.0, 1.0], [1.0, -0.4])),   # cubics
             [0.0] + list(np.poly([0.1, 0.7, 3.0])),                                                                             # a trimmed cubic
             list(np.poly([0.2, 0.4, 0.6, 0.8])), list(np.polymul([1.0, -1.0, 2.5], np.poly([0.3, 0.6]))),
             list(np.polymul([1.0, 0.0, 1.0], [1.0, 1.0, 4.0])), list(-3.0 * np.poly([-2.0, -0.5, 1.0, 4.0]))]                 # quartics
    for p in polys:
        n, re = run(p)
        ref = np.sort(np.roots(p).real)
        assert n == len(ref) and np.isnan(re[n:]).all(), (label, p, n, re)
        worst = max(worst, np.abs(np.sort(re[:n]) - ref).max() / (1e-12 * np.abs(np.roots(p)).max()))
    print(f"{label}: ls_root_real_parts against numpy.roots, worst error over bound {worst:.3g}")
    assert worst <= 1.0, (label, worst)
    return worst
