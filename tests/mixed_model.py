"""The mixed-precision solve (cgx_mixed_solve; cgx.h "cgx_mixed", DESIGN.md
§5d) restated in numpy on tests/cg_model.py: the outer loop in float64
(cg_model.spmv, cg_model.dot), the inner solves the float32 model
(cg_model.cg), the two casts numpy's.

  r = b - A x; rr = dot(r, r) (exact sum of the rounded squares, rounded once)
  record (rr, bodies and final f32 r.r of the inner solve before; 0, 0 first)
  rr NaN / Inf -> 4; sqrt(rr) <= tol -> 1; sqrt(rr) > 0.5 prev -> 3;
  o == max_outer or tot >= cap -> 2
  nr = f 2^e (frexp), s = 2^-e; r32 = float32(r s); tol_in = max(inner_reduction, 0.5 tol s)
  d32 = f32 CG on A32 d = r32 from 0, cap min(n + 1, inner_cap, cap - tot)
  final inner r.r NaN -> 4, no correction; else x += float64(d32) 2^e, tot += bodies

A dot that is not clear (cg_model's guard) may round either way on the
device: `choices` picks, over the outer dots and the inner solves' dots in
the order they occur, and `trajectories` enumerates every combination.

numpy and the standard library only.
"""
from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests import cg_model

F32 = np.float32

# x, status (1 tol, 2 cap / max_outer, 3 stagnated, 4 NaN), corrections applied,
# inner bodies counted, the last f64 r.r, [(rr, inner bodies, inner final r.r)]
# per residual evaluation, the dots that were not clear (outer and inner)
Result = namedtuple("Result", "x status outer inner_bodies rxr history unclear")

DEFAULTS = dict(inner_reduction=1e-5, max_outer=8, inner_cap=-1)


def cast_matrix(vl):
    """A32's values; raises where cgx_mixed_create refuses."""
    vl = np.asarray(vl, np.float64)
    with np.errstate(over="ignore", under="ignore"):
        v32 = vl.astype(F32)
    bad = np.isinf(v32) | ((v32 == 0) & (vl != 0))
    if bad.any():
        raise ValueError(f"{int(bad.sum())} values overflow or underflow in f32; first {int(np.argmax(bad))}")
    return v32


def jacobi32(rp, cl, v32):
    """cgx_csr_diag_inv on A32: the f32 sums of each row's col == row entries, 1 / them in f32."""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    on = rows == cl
    d = np.zeros(n, F32)
    np.add.at(d, rows[on], np.asarray(v32, F32)[on])
    return F32(1) / d


def _trunc32(a):
    """(teeth) float64 -> float32 rounded toward zero."""
    with np.errstate(over="ignore", under="ignore"):
        f = a.astype(F32)
    over = np.abs(f.astype(np.float64)) > np.abs(a)
    f[over] = np.nextafter(f[over], F32(0))
    return f


def refine(rp, cl, vl, b, tol, max_bodies=-1, x0=None, precond=None, inner_reduction=0,
           max_outer=0, inner_cap=0, choices=(), wrong=None, _branch=False):
    """-> Result. precond: None, "jacobi" or n float64 values (the caller's
    diagonal, cast to f32). 0 for the three knobs keeps the defaults, as
    cgx_mixed_config. wrong (the CPU tests' deliberately wrong variants):
    "trunc_cast" casts r s toward zero, "fma_scale" scales by 1 / nr (not a
    power of two) and forms the up-add with one rounding, "plain_rr" sums the
    outer r.r in index order, "flush" casts f32 subnormals to 0."""
    rp = np.asarray(rp, np.int64)
    cl = np.asarray(cl, np.int64)
    vl = np.asarray(vl, np.float64)
    b = np.asarray(b, np.float64)
    n = len(b)
    v32 = cast_matrix(vl)
    inner_reduction = inner_reduction or DEFAULTS["inner_reduction"]
    max_outer = max_outer or DEFAULTS["max_outer"]
    icap = n + 1 if (inner_cap or -1) < 0 else min(n + 1, int(inner_cap))
    cap = n + 1 if max_bodies < 0 else min(n + 1, max(int(max_bodies), 1))
    if precond is None:
        m32 = None
    elif isinstance(precond, str):
        assert precond == "jacobi"
        m32 = jacobi32(rp, cl, v32)
    else:
        with np.errstate(over="ignore", under="ignore"):
            m32 = np.asarray(precond, np.float64).astype(F32)
        assert (np.isfinite(m32) & (m32 > 0)).all()
    x = np.zeros(n) if x0 is None else np.array(x0, np.float64)
    used, unclear, history = 0, [], []
    tot, prev, last = 0, math.inf, (0, 0.0)
    o = 0
    with np.errstate(all="ignore"):
        while True:
            r = b - cg_model.spmv(rp, cl, vl, x)
            if wrong == "plain_rr":
                rr = cg_model._dot_plain(r, r)
            else:
                rr, clear, lo, hi, margin = cg_model.dot(r, r)
                if not clear:
                    if used < len(choices):
                        rr = hi if choices[used] else lo
                    elif _branch:
                        raise cg_model._NeedChoice()
                    used += 1
                    unclear.append(cg_model.Unclear(o, "outer r.r", o, lo, hi, rr, margin))
            rr = float(rr)
            history.append((rr, last[0], last[1]))
            nr = math.sqrt(rr) if rr >= 0 else math.nan
            if not math.isfinite(rr):
                status = 4
            elif nr <= tol:
                status = 1
            elif nr > 0.5 * prev:
                status = 3
            elif o == max_outer or tot >= cap:
                status = 2
            else:
                status = 0
            if status:
                return Result(x, status, o, tot, rr, history, unclear)
            prev = nr
            _, e = math.frexp(nr)
            s, sinv = math.ldexp(1.0, -e), math.ldexp(1.0, e)
            if wrong == "fma_scale":
                s, sinv = 1.0 / nr, nr
            r32 = _trunc32(r * s) if wrong == "trunc_cast" else (r * s).astype(F32)
            if wrong == "flush":
                r32[np.abs(r32) < np.finfo(F32).tiny] = 0
            tol_in = max(inner_reduction, 0.5 * tol * s)
            run = cg_model.cg(rp, cl, v32, r32, tol_in, min(icap, cap - tot), minv=m32, dtype=F32,
                              choices=tuple(choices[used:]), _branch=_branch)
            used += len(run.unclear)
            unclear += run.unclear
            irxr = float(run.rr[-1])
            if math.isnan(irxr):
                return Result(x, 4, o, tot, rr, history, unclear)
            if wrong == "fma_scale":
                fs = Fraction(sinv)
                x = np.array([float(Fraction(float(a)) + Fraction(float(d)) * fs)
                              for a, d in zip(x, run.x)])
            else:
                x = x + run.x.astype(np.float64) * sinv
            tot += run.bodies
            last = (run.bodies, irxr)
            o += 1


def trajectories(*args, max_unclear=cg_model.MAX_UNCLEAR, **kw):
    """Every run of refine(*args, **kw) over the combinations of choices at its
    dots that are not clear -> [(choices, Result)]. TooManyUnclear past
    max_unclear on any path."""
    out, stack = [], [()]
    while stack:
        ch = stack.pop()
        try:
            out.append((ch, refine(*args, choices=ch, _branch=True, **kw)))
        except cg_model._NeedChoice:
            if len(ch) >= max_unclear:
                raise cg_model.TooManyUnclear(
                    f"more than {max_unclear} dots are not clear (choices so far {ch})") from None
            stack += [ch + (1,), ch + (0,)]
    return out
