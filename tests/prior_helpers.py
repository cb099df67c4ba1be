"""Dense marginalisation priors for the tests (MarginalizationFactor: r = r0 + J0 dx over the kept blocks).

synth.make_window's prior is the gauge anchor of bench.py's windows: J0 = 1e3 I, r0 = 0, ROT / POS of knots 0..3 in canonical
offset order, linearised at the truth.  A transposed J0, a wrong column map of the bias / line-delay blocks, a broken quaternion sign
fix or wrong per-window offsets all pass unnoticed with it.  `make_prior` builds the opposite: every block kind, blocks listed in a
shuffled order at offsets that are a random permutation of the block slots, J0 = diag(sigma) U with U orthogonal and sigma log-uniform
in [1, 1e3] (neither symmetric nor diagonal), r0 ~ N(0, 0.1), x0 = the current state slightly perturbed, and at least one ROT block
that stores the NEGATED quaternion of its x0 (the same rotation, dq.w < 0: the sign fix of marginalization_factor.cpp:346-350).
"""
from __future__ import annotations

import numpy as np

PK_ROT, PK_POS, PK_BG, PK_BA, PK_LD = 0, 1, 2, 3, 4
BLOCK_SIZE = {PK_ROT: 3, PK_POS: 3, PK_BG: 3, PK_BA: 3, PK_LD: 1}


def unknown_of(w, kind, idx):
    """First unknown of a kept block in the package's ordering (window.py): knot k rot 6k / pos 6k+3, bias f bg 6K+6f / ba 6K+6f+3,
    line delay 6K+6F."""
    K, F = w.K, w.F
    return {PK_ROT: 6 * idx, PK_POS: 6 * idx + 3, PK_BG: 6 * K + 6 * idx, PK_BA: 6 * K + 6 * idx + 3, PK_LD: 6 * K + 6 * F}[kind]


def prior_columns(w):
    """col[i] = the unknown that prior dimension i belongs to."""
    col = np.full(w.pn, -1, np.int64)
    for kind, idx, off in zip(w.p_kind, w.p_index, w.p_off):
        u0 = unknown_of(w, int(kind), int(idx))
        for k in range(BLOCK_SIZE[int(kind)]):
            col[off + k] = u0 + k
    return col


def _qexp(v):
    th = np.linalg.norm(v)
    if th < 1e-12:
        q = np.array([0.5 * v[0], 0.5 * v[1], 0.5 * v[2], 1.0])
    else:
        s = np.sin(0.5 * th) / th
        q = np.array([s * v[0], s * v[1], s * v[2], np.cos(0.5 * th)])
    return q / np.linalg.norm(q)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def constant_knots(w):
    kc = np.zeros(w.K, bool)
    kc[: max(int(w.fixed_upto) + 1, 0)] = True
    if w.knot_const is not None:
        kc |= np.asarray(w.knot_const, bool)
    return kc


def make_prior(w, seed, *, full=False, with_const=False, n_knots=4, n_bias=3, negate=None):
    """Prior arrays (pJ0, pr0, p_kind, p_index, p_off, p_x0) for window w (not modified).

    full:       every pose unknown (ROT + POS of every knot, BG + BA of every bias state, LD): pn = P, the largest a valid window has.
    with_const: the blocks include the window's constant ones -- every knot held constant (fixed_upto, knot_const), and the bias /
                line-delay blocks even when lock_bg / lock_ba / fix_ld hold them.
    otherwise:  ROT + POS of a run of n_knots knots, BG + BA of n_bias bias states, LD.
    negate:     how many ROT blocks store -x0 (default: about a third, at least one)."""
    rng = np.random.default_rng(seed)
    K, F = w.K, w.F
    if full:
        knots, biases = list(range(K)), list(range(F))
    else:
        k0 = int(rng.integers(0, K - n_knots + 1))
        knots = list(range(k0, k0 + n_knots))
        biases = sorted(rng.choice(F, size=min(n_bias, F), replace=False).tolist())
        if with_const:
            kc = np.flatnonzero(constant_knots(w)).tolist()
            assert kc, "with_const needs a window with constant knots"
            knots = sorted(set(knots) | set(kc))
    blocks = [(PK_ROT, k) for k in knots] + [(PK_POS, k) for k in knots]
    blocks += [(PK_BG, f) for f in biases] + [(PK_BA, f) for f in biases] + [(PK_LD, 0)]
    nb = len(blocks)
    pn = sum(BLOCK_SIZE[k] for k, _ in blocks)
    # offsets: the block slots laid out in a random order; the blocks listed in another random order
    layout = rng.permutation(nb)
    off = np.zeros(nb, np.int32)
    o = 0
    for b in layout:
        off[b] = o
        o += BLOCK_SIZE[blocks[b][0]]
    assert o == pn
    order = rng.permutation(nb)
    blocks = [blocks[b] for b in order]
    off = off[order]
    # x0: the current state, perturbed
    rot_blocks = [i for i, (k, _) in enumerate(blocks) if k == PK_ROT]
    nneg = max(1, len(rot_blocks) // 3) if negate is None else int(negate)
    neg = set(rng.choice(rot_blocks, size=min(nneg, len(rot_blocks)), replace=False).tolist())
    x0 = np.zeros((nb, 4))
    for i, (kind, idx) in enumerate(blocks):
        if kind == PK_ROT:
            q = _qmul(w.quat[idx], _qexp(rng.normal(0.0, 1e-3, 3)))
            x0[i] = -q if i in neg else q
        elif kind == PK_POS:
            x0[i, :3] = w.pos[idx] + rng.normal(0.0, 1e-2, 3)
        elif kind == PK_BG:
            x0[i, :3] = w.bias[idx, :3] + rng.normal(0.0, 1e-2, 3)
        elif kind == PK_BA:
            x0[i, :3] = w.bias[idx, 3:] + rng.normal(0.0, 1e-2, 3)
        else:
            x0[i, 0] = w.ld + rng.normal(0.0, 1e-6)
    # J0 = diag(sigma) U
    Q, R = np.linalg.qr(rng.normal(size=(pn, pn)))
    U = Q * np.sign(np.diag(R))
    sigma = np.exp(rng.uniform(0.0, np.log(1e3), pn))
    J0 = sigma[:, None] * U
    r0 = rng.normal(0.0, 0.1, pn)
    return dict(pJ0=J0, pr0=r0, p_kind=np.array([k for k, _ in blocks], np.int32), p_index=np.array([i for _, i in blocks], np.int32),
                p_off=off, p_x0=x0)


def with_prior(w, pr):
    """A copy of w carrying prior `pr` (a dict from make_prior; None: no prior)."""
    w = w.copy()
    if pr is None:
        pr = dict(pJ0=np.zeros((0, 0)), pr0=np.zeros(0), p_kind=np.zeros(0, np.int32), p_index=np.zeros(0, np.int32),
                  p_off=np.zeros(0, np.int32), p_x0=np.zeros((0, 4)))
    for k, v in pr.items():
        setattr(w, k, np.array(v, copy=True))
    return w.normalize()


def dense_prior_window(w, seed, **kw):
    """w with a make_prior prior (replacing the gauge anchor synth puts on it)."""
    return with_prior(w, make_prior(w, seed, **kw))


def duplicate_block(w, kind):
    """w with its first prior block of `kind` listed a second time, at a new offset behind the others (an invalid window: the host
    refuses it)."""
    b = int(np.flatnonzero(w.p_kind == kind)[0])
    n, sz = w.pn, BLOCK_SIZE[kind]
    J0 = 10.0 * np.eye(n + sz)
    J0[:n, :n] = w.pJ0
    return with_prior(w, dict(pJ0=J0, pr0=np.zeros(n + sz), p_kind=np.append(w.p_kind, kind), p_index=np.append(w.p_index, w.p_index[b]),
                              p_off=np.append(w.p_off, n), p_x0=np.vstack([w.p_x0, w.p_x0[b]])))


def has_negated_rotation(w):
    """Some ROT block's x0 is the negated neighbour of its knot (dq.w < 0 at the current state)."""
    for kind, idx, x0 in zip(w.p_kind, w.p_index, w.p_x0):
        if kind == PK_ROT and np.dot(x0, w.quat[idx]) < 0:
            return True
    return False
