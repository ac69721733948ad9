"""The engine's CG loop restated in numpy, in any dtype (float32 or float64).

Every intermediate is rounded to `dtype`, statement for statement as the
kernels compute it (cgx_kernels.hip is built with -ffp-contract=off, so no
product is fused into an addition):

  spmv    the per-row loop from 0, entries in CSR order, each product rounded
          before it is added (VectorOperations.hpp:438-466);
  dot     the loop's dots are double-length sums (cgx_dd.h): their value is
          the exact sum S of the dtype-rounded products t_i to within about
          n u^2 sum|t_i| (u the unit roundoff), rounded once. Here S is summed
          exactly (the value math.fsum would round, kept as an integer so that
          its distance to a rounding boundary is exact too) and rounded once;
  cg      CG.hpp's loop with stop rule Q5, plain or with a diagonal
          preconditioner (cgx.h, "diagonal preconditioning").

A dot is *clear* when S lies farther than the guard g = 4 n u^2 sum|t_i| from
every midpoint between adjacent dtype values: whatever the order the device
sums in, it then rounds to the same value. A dot that is not clear may round
to either of the two values that bracket S; `choices` picks one, and
`trajectories` enumerates every combination. The guard is cgx_dd.h's stated
accuracy times 4, not a fitted number.

numpy and the standard library only.
"""
from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

# x, bodies run, r.r before the first body, r.r after each body, r.z after each
# body (preconditioned; else empty), the dots that were not clear, x after
# each body (keep_x=True; else empty)
Run = namedtuple("Run", "x bodies rr0 rr rz unclear xs")
# one dot that was not clear: its number in the run (0 = the initial r.r), its
# name, the body it belongs to (0 = init), the bracketing values, the one
# taken, and the distance to the boundary in guards (< 1)
Unclear = namedtuple("Unclear", "index name body lo hi taken margin")

MAX_UNCLEAR = 3  # per committed case: at most 2^3 trajectories


class TooManyUnclear(RuntimeError):
    pass


class _NeedChoice(Exception):
    pass


def spmv(rp, cl, v, x):
    """y = A x, the reference's per-row loop, vectorised over "the j-th entry
    of every row that has one"."""
    n = len(rp) - 1
    dt = x.dtype
    v = np.asarray(v, dt)
    rp = np.asarray(rp, np.int64)
    deg = np.diff(rp)
    order = np.argsort(-deg, kind="stable")  # rows by falling length
    sdeg = deg[order[::-1]]                  # ascending
    y = np.zeros(n, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(deg.max()) if n else 0):
            cnt = n - int(np.searchsorted(sdeg, j, side="right"))  # rows with > j entries
            if cnt == n:
                k = rp[:-1] + j
                y = y + v[k] * x[cl[k]]
            else:
                r = order[:cnt]
                k = rp[r] + j
                y[r] = y[r] + v[k] * x[cl[k]]
    return y


def _exact_sum(t):
    """The exact sum of a finite float array as a Fraction. Each value is
    m 2^e with a 53-bit integer m, split into halves of 26 and 27 bits; the
    halves are summed per exponent in float64, where every partial sum is an
    integer below 2^53 and so exact in any order."""
    assert t.size < (1 << 26)
    m, e = np.frexp(t.astype(np.float64))
    big = np.ldexp(m, 53)                    # integer-valued, |big| < 2^53
    hi = np.trunc(np.ldexp(big, -27))
    lo = big - np.ldexp(hi, 27)
    e0 = int(e.min()) if t.size else 0
    idx = (e - e0).astype(np.int64)
    sh = np.bincount(idx, weights=hi)
    sl = np.bincount(idx, weights=lo)
    total = 0
    for k in np.nonzero((sh != 0) | (sl != 0))[0]:
        total += ((int(sh[k]) << 27) + int(sl[k])) << int(k)
    return Fraction(total) * Fraction(2) ** (e0 - 53)


def dot(a, b):
    """-> (value, clear, lo, hi, margin): the exact sum of fl(a_i b_i) rounded
    once to the arrays' dtype; whether it is clear (module docstring); the two
    dtype values that bracket the exact sum; distance to the nearest rounding
    boundary divided by the guard (inf where the guard is 0)."""
    dt = a.dtype.type
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = a * b
    assert t.dtype == a.dtype == b.dtype
    if not np.isfinite(t).all():             # NaN / Inf: nothing to round
        with np.errstate(invalid="ignore", over="ignore"):
            s = dt(np.sum(t))
        return s, True, s, s, math.inf
    S = _exact_sum(t)
    A = S if (t >= 0).all() else _exact_sum(np.abs(t))
    if A == 0:
        z = dt(0)
        return z, True, z, z, math.inf
    u = float(np.finfo(dt).eps) / 2
    guard = Fraction(4 * t.size) * Fraction(u) ** 2 * A
    big = np.finfo(dt).max
    assert abs(S) < Fraction(float(big))
    c = dt(S.numerator / S.denominator)      # near S; the neighbours settle the rest
    cand = [np.nextafter(c, dt(-np.inf)), c, np.nextafter(c, dt(np.inf))]
    fr = [Fraction(float(q)) for q in cand]
    lo = max(i for i in range(3) if fr[i] <= S)
    hi = min(i for i in range(3) if fr[i] >= S)
    if lo == hi:  # S is a dtype value: the nearer boundary is half a gap away
        i = lo
        val = cand[i]
        dn = (fr[i] - Fraction(float(np.nextafter(val, dt(-np.inf))))) / 2
        up = (Fraction(float(np.nextafter(val, dt(np.inf)))) - fr[i]) / 2
        dist = min(dn, up)
        if dn <= up:
            blo, bhi = np.nextafter(val, dt(-np.inf)), val
        else:
            blo, bhi = val, np.nextafter(val, dt(np.inf))
    else:
        blo, bhi = cand[lo], cand[hi]
        mid = (fr[lo] + fr[hi]) / 2
        dist = abs(S - mid)
        if S < mid:
            val = blo
        elif S > mid:
            val = bhi
        else:  # a tie: to even
            even = (blo.view(np.uint32 if dt == np.float32 else np.uint64) & 1) == 0
            val = blo if even else bhi
    return val, dist > guard, blo, bhi, float(dist / guard)


def _dot_plain(a, b):
    """(teeth) the dot as a plain index-order sum in dtype."""
    t = a * b
    return np.cumsum(t, dtype=t.dtype)[-1]


def _dot_unrounded(a, b):
    """(teeth) the dot with its products left unrounded (f32 only: the f64
    products of f32 values are exact)."""
    assert a.dtype == np.float32
    return np.float32(math.fsum((a.astype(np.float64) * b.astype(np.float64)).tolist()))


def cg(rp, cl, v, b, tol, max_bodies, x0=None, minv=None, dtype=np.float32, choices=(),
       keep_x=False, wrong=None, _cache=None, _branch=False):
    """The loop. tol and max_bodies as cgx_cg_begin's (cap min(N + 1,
    max_bodies), N + 1 when max_bodies < 0); minv: the diagonal m of the
    preconditioned loop. choices[i] = 0 / 1 takes the lower / upper
    bracketing value at the i-th dot that is not clear; past the end of
    `choices` such a dot takes its rounded value. -> Run.

    wrong (the CPU tests' deliberately wrong variants): "fma_r" forms the r
    update with one rounding, "pap_unrounded" sums p.Ap over unrounded
    products, "plain_dots" sums every dot in index order in dtype."""
    dt = np.dtype(dtype).type
    v = np.asarray(v, dt)
    b = np.asarray(b, dt)
    n = len(b)
    cap = n + 1 if max_bodies < 0 else min(n + 1, max(int(max_bodies), 1))
    tol = dt(tol)
    unclear = []
    seq = [0]
    cache = {} if _cache is None else _cache

    def d(name, body, a, c):
        i = seq[0]
        seq[0] += 1
        if wrong == "plain_dots":
            return _dot_plain(a, c)
        if wrong == "pap_unrounded" and name == "p.Ap":
            return _dot_unrounded(a, c)
        key = (i, tuple(float(q.taken) for q in unclear))  # the run so far is a function of these
        if key not in cache:
            cache[key] = dot(a, c)
        val, clear, lo, hi, margin = cache[key]
        if not clear:
            k = len(unclear)
            if k < len(choices):
                val = hi if choices[k] else lo
            elif _branch:
                raise _NeedChoice()
            unclear.append(Unclear(i, name, body, lo, hi, val, margin))
        return val

    def A(y):  # (shared between trajectories like the dots)
        key = ("A", seq[0], tuple(float(q.taken) for q in unclear))
        if key not in cache:
            cache[key] = spmv(rp, cl, v, y)
        return cache[key]

    with np.errstate(all="ignore"):
        x = np.zeros(n, dt) if x0 is None else np.array(x0, dt)
        r = b - (np.zeros(n, dt) if x0 is None else A(x))  # A 0 = +0 in every row
        rxr = d("r.r", 0, r, r)
        rr0 = rxr
        if minv is None:
            p = r.copy()
            rz = None
        else:
            m = np.asarray(minv, dt)
            p = m * r
            rz = d("r.z", 0, r, p)
        bodies, rrs, rzs, xs = 0, [], [], []
        while True:
            Ap = A(p)
            pAp = d("p.Ap", bodies + 1, p, Ap)
            alpha = (rxr if minv is None else rz) / pAp
            if wrong == "fma_r":
                r = (r.astype(np.float64) - np.float64(alpha) * Ap.astype(np.float64)).astype(dt)
            else:
                r = r - alpha * Ap
            rr_new = d("r.r", bodies + 1, r, r)
            x = x + alpha * p
            if minv is None:
                beta = rr_new / rxr
                p = r + beta * p
            else:
                z = m * r
                rz_new = d("r.z", bodies + 1, r, z)
                beta = rz_new / rz
                p = z + beta * p
                rz = rz_new
                rzs.append(rz)
            bodies += 1
            stop = bool(np.isnan(rxr)) or bool(np.sqrt(rxr) <= tol)  # Q5: the r.r it started with
            rxr = rr_new
            rrs.append(rxr)
            if keep_x:
                xs.append(x)
            if stop or bodies >= cap:
                assert type(alpha) is dt and type(beta) is dt and x.dtype == r.dtype == p.dtype == dt
                return Run(x, bodies, rr0, rrs, rzs, unclear, xs)


def trajectories(*args, max_unclear=MAX_UNCLEAR, **kw):
    """Every run of cg(*args, **kw) over the 2^k combinations of choices at
    its dots that are not clear -> [(choices, Run)]. The runs share the dots
    of their common prefixes. TooManyUnclear past max_unclear on any path."""
    cache, out, stack = {}, [], [()]
    while stack:
        ch = stack.pop()
        try:
            out.append((ch, cg(*args, choices=ch, _cache=cache, _branch=True, **kw)))
        except _NeedChoice:
            if len(ch) >= max_unclear:
                raise TooManyUnclear(f"more than {max_unclear} dots are not clear "
                                     f"(choices so far {ch})") from None
            stack += [ch + (1,), ch + (0,)]
    return out
