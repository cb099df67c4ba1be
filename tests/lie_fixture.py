"""The high-precision fixture of the Lie primitives of ctrl-vio_amd/csrc/so3.hpp (tests/golden/lie_edge_grid.npz): its inputs, its expected
values (mpmath at 50 digits, rounded once to fp64; written by `python tests/golden/make_golden.py lie`) and the one check both builds of the
header run against it (tests/devprobe.py: Host, Device).

Rotation vectors: 23 axes (the coordinate axes and 20 seeded random ones) at each of the angles ANGLES and at the three doubles around the
series / closed-form switch of so3_exp, Jr and Jr^-1 (dot(phi, phi) just below, on and just above 0.25).  Angles within 0.1 of pi are not
in the grid: the closed form of Jr^-1 loses about 1e-16 / (pi - theta)^2 there (6e-10 at pi - 1e-9 on the host build), the reference's has
the same loss, and no usable spline has such a knot pair.

Bounds (the family of tests/test_device_math_host.py::test_lie_primitives): exp 1e-13, Jr 2e-13, Jr^-1 4e-13 of its largest entry,
log(exp) 4e-13 max(1, theta), quaternion products and basis rows 1e-13 of the largest output."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "golden", "lie_edge_grid.npz")
ANGLES = (0.0, 1e-300, 1e-160, 1e-20, 1e-9, 1e-4, 0.1, 1.0, 2.0, 3.0)
DIGITS = 50
EXPECTED = ("exp", "Jr", "Jr_inv", "log_exp", "log", "qmul", "basis")   # the arrays expected_values() computes


# ------------------------------------------------------------------------------------------------ inputs
def _axes():
    rng = np.random.default_rng(20)
    a = rng.normal(size=(20, 3))
    return np.concatenate([np.eye(3), a / np.linalg.norm(a, axis=1, keepdims=True)])


def _switch_rows(axis):
    """three multiples of the axis whose fp64 dot(phi, phi) (plain products and sums, no fma) is the largest below 0.25, 0.25 itself (or,
    where no multiple hits it, the smallest above) and the next above that, among the 129 doubles around 0.5 / |axis|"""
    s = 0.5 / np.linalg.norm(axis)
    for _ in range(64):
        s = np.nextafter(s, 0.0)
    cand = []
    for _ in range(129):
        phi = s * axis
        cand.append((phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], phi))
        s = np.nextafter(s, 1.0)
    below = max((c for c in cand if c[0] < 0.25), key=lambda c: c[0])
    on = min((c for c in cand if c[0] >= 0.25), key=lambda c: c[0])
    above = min((c for c in cand if c[0] > on[0]), key=lambda c: c[0])
    return [below[1], on[1], above[1]]


def _unit_rows(rng, n):
    """unit quaternions to rounding: normalised in fp64"""
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def knot_spacings():
    """dt_ns of the `tiny` and `config1` windows of ctrl-vio_amd/synth.py, read from the generator (both 50 ms today, idt = 20), and 30 ms:
    idt = 33.33..., not a double, so that idt^D carries rounding into the basis rows"""
    import importlib
    import sys
    root = os.path.dirname(HERE)
    if root not in sys.path:
        sys.path.insert(0, root)
    synth = importlib.import_module("ctrl-vio_amd").synth
    return [int(synth.make_window(cfg, seed=seed).dt_ns) for cfg, seed in (("tiny", 7), ("config1", 1003))] + [30_000_000]


def inputs():
    dt_ns = knot_spacings()
    axes = _axes()
    phi = [ang * a for ang in ANGLES for a in axes]
    for k in range(3):
        phi += [_switch_rows(a)[k] for a in axes]
    phi = np.array(phi)
    rng = np.random.default_rng(21)
    # so3_log on quaternions directly (x, y, z, w): the other cover (w < 0) at several angles; |v| on both sides of 1e-10 with w = +-1; |w| on
    # both sides of 1e-10 with either sign
    lq = []
    for ang in (1e-4, 0.1, 1.0, 2.0, 3.0):
        for a in axes[[0, 3, 4, 5]]:
            lq.append(-np.concatenate([np.sin(0.5 * ang) * a, [np.cos(0.5 * ang)]]))
    for n in (0.999e-10, 1.001e-10, 1e-12, 1e-9):
        for a, w in ((axes[1], 1.0), (axes[6], 1.0), (axes[7], -1.0)):
            lq.append(np.concatenate([n * a, [w]]))
    for wabs in (0.999e-10, 1.001e-10, 1e-12, 1e-9):
        for a, sgn in ((axes[2], 1.0), (axes[8], 1.0), (axes[9], -1.0), (axes[2], -1.0)):
            w = sgn * wabs
            lq.append(np.concatenate([np.sqrt(1.0 - w * w) * a, [w]]))
    u = np.array([0.0, 2.0 ** -52, 0.5, 1.0 - 2.0 ** -53])
    return dict(phi=phi, log_q=np.array(lq), qmul_a=_unit_rows(rng, 40), qmul_b=_unit_rows(rng, 40),
                basis_u=np.tile(u, len(dt_ns)), basis_idt=np.repeat([1e9 / d for d in dt_ns], len(u)))


# ------------------------------------------------------------------------------------------------ expected values (needs mpmath)
def expected_values(inp):
    """Every output from its definition at DIGITS digits (closed forms, with enough further working digits for their cancellation at small
    angles), rounded once to fp64.  One exception: so3_log below its two 1e-10 thresholds is compared with the limit the function itself
    uses there, see below."""
    import mpmath as mp

    def work_digits(theta):
        # (1 - cos t) / t^2, (t - sin t) / t^3 and 1 / t^2 - (1 + cos t) / (2 t sin t) cancel 2, 3 and 2 times the digits of 1 / t
        return DIGITS + 10 + (0 if theta >= 1 else int(3 * -mp.log10(theta)) + 3)

    def hat(v):
        return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    def f64(m):
        return np.array([float(x) for x in m], np.float64)

    n = len(inp["phi"])
    out = dict(exp=np.zeros((n, 4)), Jr=np.zeros((n, 3, 3)), Jr_inv=np.zeros((n, 3, 3)), log_exp=np.array(inp["phi"], np.float64).copy())
    for i, phi in enumerate(inp["phi"]):
        mp.mp.dps = DIGITS
        v = [mp.mpf(float(x)) for x in phi]
        theta = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
        if theta == 0:
            im, re, a, b, c = mp.mpf(1) / 2, mp.mpf(1), mp.mpf(1) / 2, mp.mpf(1) / 6, mp.mpf(1) / 12
        else:
            mp.mp.dps = work_digits(theta)
            theta = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
            im, re = mp.sin(theta / 2) / theta, mp.cos(theta / 2)
            a = (1 - mp.cos(theta)) / theta ** 2
            b = (theta - mp.sin(theta)) / theta ** 3
            c = 1 / theta ** 2 - (1 + mp.cos(theta)) / (2 * theta * mp.sin(theta))
        H = hat(v)
        H2 = H * H
        out["exp"][i] = f64([im * v[0], im * v[1], im * v[2], re])
        out["Jr"][i] = f64(mp.eye(3) - a * H + b * H2).reshape(3, 3)
        out["Jr_inv"][i] = f64(mp.eye(3) + H / 2 + c * H2).reshape(3, 3)
    mp.mp.dps = DIGITS
    # so3_log by its own definition: 2 atan(n / w) / n times the vector part, with the function's two limits below its 1e-10 thresholds
    # (2 / w - 2 n^2 / w^3 for n < 1e-10; +-pi / n for |w| < 1e-10, which is the atan form to 2 |w| / n^2).  The rows stay 1e-3 relative away
    # from either threshold, so the branch is the one the fp64 code takes.
    lg = np.zeros((len(inp["log_q"]), 3))
    for i, q in enumerate(inp["log_q"]):
        x, y, z, w = [mp.mpf(float(t)) for t in q]
        nn = mp.sqrt(x * x + y * y + z * z)
        if nn < mp.mpf("1e-10"):
            f = 2 / w - 2 * nn * nn / w ** 3
        elif abs(w) < mp.mpf("1e-10"):
            f = (mp.pi if w > 0 else -mp.pi) / nn
        else:
            f = 2 * mp.atan(nn / w) / nn
        lg[i] = f64([f * x, f * y, f * z])
    out["log"] = lg
    # qmul: Hamilton product times 2 / (1 + |.|^2); qmul_unit is the same function to (|.|^2 - 1)^3 / 8
    qm = np.zeros((len(inp["qmul_a"]), 4))
    for i, (qa, qb) in enumerate(zip(inp["qmul_a"], inp["qmul_b"])):
        ax, ay, az, aw = [mp.mpf(float(t)) for t in qa]
        bx, by, bz, bw = [mp.mpf(float(t)) for t in qb]
        o = [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
             aw * bw - ax * bx - ay * by - az * bz]
        s = 2 / (1 + sum(t * t for t in o))
        qm[i] = f64([s * t for t in o])
    out["qmul"] = qm
    # basis<CUMULATIVE, D>(u, idt^D): idt^D / 6 times M b_D(u); rows: cumulative D = 0, 1, 2, then the plain basis D = 0, 1, 2
    Mc = mp.matrix([[6, 0, 0, 0], [5, 3, -3, 1], [1, 3, 3, -2], [0, 0, 0, 1]])
    Mb = mp.matrix([[1, -3, 3, -1], [4, 0, -6, 3], [1, 3, 3, -3], [0, 0, 0, 1]])
    bs = np.zeros((len(inp["basis_u"]), 6, 4))
    for i, (u, idt) in enumerate(zip(inp["basis_u"], inp["basis_idt"])):
        u, idt = mp.mpf(float(u)), mp.mpf(float(idt))
        mono = [mp.matrix([1, u, u * u, u ** 3]), mp.matrix([0, 1, 2 * u, 3 * u * u]), mp.matrix([0, 0, 2, 6 * u])]
        for k, M in enumerate((Mc, Mb)):
            for D in range(3):
                bs[i, 3 * k + D] = f64(idt ** D / 6 * (M * mono[D]))
    out["basis"] = bs
    return out


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ the check
def check(fx, impl, label):
    """impl: devprobe.Host or devprobe.Device.  Asserts every bound, prints and returns the worst error over bound per output."""
    tol = 1e-13
    worst = {}

    def see(name, err, bound):
        ratio = np.max(np.asarray(err) / np.asarray(bound))
        worst[name] = max(worst.get(name, 0.0), float(ratio))

    phi = fx["phi"]
    theta = np.linalg.norm(phi, axis=1)
    q, Jr, Ji, lg = impl.so3(phi)
    see("exp", np.abs(q - fx["exp"]).max(axis=1), tol)
    see("Jr", np.abs(Jr - fx["Jr"]).max(axis=(1, 2)), 2 * tol)
    see("Jr_inv", np.abs(Ji - fx["Jr_inv"]).max(axis=(1, 2)), 4 * tol * np.abs(fx["Jr_inv"]).max(axis=(1, 2)))
    see("log_exp", np.abs(lg - fx["log_exp"]).max(axis=1), 4 * tol * np.maximum(1.0, theta))
    small = theta < 0.5
    assert small.sum() >= 7 * 23 and (~small).sum() >= 3 * 23
    qs, Js = impl.so3_small(phi[small])
    see("exp_small", np.abs(qs - fx["exp"][small]).max(axis=1), tol)
    see("Jr_small", np.abs(Js - fx["Jr"][small]).max(axis=(1, 2)), 2 * tol)
    lq = impl.so3_log(fx["log_q"])
    see("log", np.abs(lq - fx["log"]).max(axis=1), 4 * tol * np.maximum(1.0, np.linalg.norm(fx["log"], axis=1)))
    o, ou = impl.qmul(fx["qmul_a"], fx["qmul_b"])
    see("qmul", np.abs(o - fx["qmul"]).max(axis=1), tol * np.abs(fx["qmul"]).max(axis=1))
    see("qmul_unit", np.abs(ou - fx["qmul"]).max(axis=1), tol * np.abs(fx["qmul"]).max(axis=1))
    c = impl.basis(fx["basis_u"], fx["basis_idt"])
    see("basis", np.abs(c - fx["basis"]).max(axis=2), tol * np.abs(fx["basis"]).max(axis=2))
    print(f"{label}: worst error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad
    return worst
