"""Multi-shift CG (cgx_cg_solve_shifted) restated in numpy.

The base recurrence is cg_model.cg's loop on A from x = 0 in float64 (its
spmv and dot, every intermediate rounded, nothing contracted); the shifts run
the statements of cgx.h / cgx_shift.h shift_step with the same parentheses.
The shifted updates add no dot, so a run's dots that are not clear are the
base loop's: `choices` and `trajectories` work as cg_model's do, and the
engine must equal one trajectory.

numpy and the standard library only.
"""
from __future__ import annotations

import sys
from collections import namedtuple

import numpy as np

from tests import cg_model
from tests.cg_model import MAX_UNCLEAR, TooManyUnclear, Unclear, _NeedChoice

DBL_MIN = sys.float_info.min
F = np.float64

# X (n, S); per shift: bodies, code (1 frozen by the rule, 2 cap), zeta after
# its last body, |zeta| sqrt(r.r) after its last body; the dots that were not
# clear; the base alpha and beta of every body; per shift the zeta_{n+1} of
# every body it ran
Run = namedtuple("Run", "X bodies codes zeta res unclear alphas betas zetas")


def shift_step(a, bt, ap, bp, sigma, zc, zp, rxr, tol):
    """cgx_shift.h shift_step on float64 scalars -> (zn, as, bs, stop)."""
    with np.errstate(all="ignore"):
        t1 = (a * bp) * (zp - zc)
        t2 = (zp * ap) * (F(1) + sigma * a)
        zn = ((zc * zp) * ap) / (t1 + t2)
        q = zn / zc
        as_ = a * q
        bs = (bt * q) * q
        stop = bool(np.isnan(rxr)) or bool(np.abs(zc) * np.sqrt(rxr) <= tol) \
            or not bool(np.abs(zn) >= DBL_MIN)
    assert all(type(t) is F for t in (t1, t2, zn, q, as_, bs))
    return zn, as_, bs, stop


def zeta_sequence(alphas, betas, sigma, rxr=None, tol=0.0):
    """The zeta_{n+1} a shift forms from recorded base scalars, body by body
    (rxr: r.r at the start of each body, for the freeze rule; None: only the
    underflow term can freeze). Stops after the body that freezes."""
    ap, bp, zc, zp = F(1), F(0), F(1), F(1)
    out = []
    for n, (a, bt) in enumerate(zip(alphas, betas)):
        r = F(1) if rxr is None else F(rxr[n])
        zn, _, _, stop = shift_step(F(a), F(bt), ap, bp, F(sigma), zc, zp, r, F(tol))
        out.append(zn)
        zp, zc, ap, bp = zc, zn, F(a), F(bt)
        if stop:
            break
    return out


def cg_shifted(rp, cl, v, b, sigmas, tol, max_bodies, choices=(), _cache=None, _branch=False):
    """The loop. tol and max_bodies as cgx_cg_solve_shifted's. -> Run."""
    v = np.asarray(v, F)
    b = np.asarray(b, F)
    n, S = len(b), len(sigmas)
    sig = [F(s) for s in sigmas]
    cap = n + 1 if max_bodies < 0 else min(n + 1, max(int(max_bodies), 1))
    tol = F(tol)
    unclear = []
    seq = [0]
    cache = {} if _cache is None else _cache

    def d(name, body, a, c):
        i = seq[0]
        seq[0] += 1
        key = (i, tuple(float(q.taken) for q in unclear))
        if key not in cache:
            cache[key] = cg_model.dot(a, c)
        val, clear, lo, hi, margin = cache[key]
        if not clear:
            k = len(unclear)
            if k < len(choices):
                val = hi if choices[k] else lo
            elif _branch:
                raise _NeedChoice()
            unclear.append(Unclear(i, name, body, lo, hi, val, margin))
        return val

    def A(y):
        key = ("A", seq[0], tuple(float(q.taken) for q in unclear))
        if key not in cache:
            cache[key] = cg_model.spmv(rp, cl, v, y)
        return cache[key]

    with np.errstate(all="ignore"):
        r = b - np.zeros(n, F)
        p = r.copy()
        rxr = d("r.r", 0, r, r)
        X = [np.zeros(n, F) for _ in range(S)]
        P = [b.copy() for _ in range(S)]
        zc, zp = [F(1)] * S, [F(1)] * S
        active = [True] * S
        bodies, codes, rrs = [0] * S, [0] * S, [F(0)] * S
        zetas = [[] for _ in range(S)]
        ap, bp = F(1), F(0)
        alphas, betas = [], []
        m = 0
        while True:
            Ap = A(p)
            pAp = d("p.Ap", m + 1, p, Ap)
            a = rxr / pAp
            r = r - a * Ap
            rr = d("r.r", m + 1, r, r)
            bt = rr / rxr
            m += 1
            for s in range(S):
                if not active[s]:
                    continue
                zn, as_, bs, stop = shift_step(a, bt, ap, bp, sig[s], zc[s], zp[s], rxr, tol)
                X[s] = X[s] + as_ * P[s]
                P[s] = zn * r + bs * P[s]
                zp[s], zc[s] = zc[s], zn
                zetas[s].append(zn)
                bodies[s], rrs[s] = m, rr
                if stop:
                    codes[s], active[s] = 1, False
                elif m >= cap:
                    codes[s] = 2
            p = r + bt * p
            alphas.append(a)
            betas.append(bt)
            ap, bp, rxr = a, bt, rr
            if not any(active) or m >= cap:
                break
        res = [np.abs(zc[s]) * np.sqrt(rrs[s]) for s in range(S)]
        return Run(np.stack(X, axis=1), bodies, codes, list(zc), res, unclear, alphas, betas,
                   zetas)


def trajectories(*args, max_unclear=MAX_UNCLEAR, **kw):
    """Every run of cg_shifted(*args, **kw) over the combinations of choices
    at its dots that are not clear -> [(choices, Run)]."""
    cache, out, stack = {}, [], [()]
    while stack:
        ch = stack.pop()
        try:
            out.append((ch, cg_shifted(*args, choices=ch, _cache=cache, _branch=True, **kw)))
        except _NeedChoice:
            if len(ch) >= max_unclear:
                raise TooManyUnclear(f"more than {max_unclear} dots are not clear "
                                     f"(choices so far {ch})") from None
            stack += [ch + (1,), ch + (0,)]
    return out
