"""The systems of the wave-per-system tests (cgx_many_set_form, DESIGN.md §5e,
"A wave per system"): one definition for tests/test_many_wave_cpu.py, which
checks with tests/cg_model.py that every one of them has no dot that is not
clear under the plain loop, JACOBI and DIAGONAL, and for
tests/test_gpu_many_wave.py, which compares them bit for bit on the device.

The sets are built from tests/many_systems.py's helpers and have its shape:
(rowptr, col, vals (nsys, nnz), B (nsys, n), tol, X0 or None, max_bodies).

  w63x41    poisson2d(9, 7),  41 systems   R = 1, its upper edge with n64
  w65x21    poisson2d(13, 5), 21 systems   R = 2, its lower edge
  w255x13   poisson2d(17, 15), 13 systems  R = 4
  n128      poisson2d(16, 8),  3 systems   R = 2, its upper edge
  n129      irregular_spd(129), 3 systems  R = 4, its lower edge

No system count is a multiple of 4 (a workgroup's waves), and the body counts
of the w sets differ between the waves of one workgroup. Width 1.0 would send
systems of w63x41 and w65x21 to their cap, 0.5 does not; for n129 the seeds
329 to 334 send system 2 to the cap in the plain loop, 335 is the first that
does not.

A set's preconditioner follows tests/many_pcg_systems.precond's recipe:
JACOBI m = 1 / d, DIAGONAL m = (1 / d) U(0.5, 2) from
default_rng(DIAG_SEED + s).

numpy only.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import many_pcg_systems as P
from tests import many_systems as M
from tests.util import irregular_spd

NONE, JACOBI, DIAGONAL = P.NONE, P.JACOBI, P.DIAGONAL
KINDS = P.KINDS
DIAG_SEED = P.DIAG_SEED

# name -> (pattern, nsys, seed of variants, width)
_SETS = {
    "w63x41": (lambda: M.poisson2d(9, 7), 41, 61, 0.5),
    "w65x21": (lambda: M.poisson2d(13, 5), 21, 62, 0.5),
    "w255x13": (lambda: M.poisson2d(17, 15), 13, 63, 0.5),
    "n128": (lambda: M.poisson2d(16, 8), 3, 328, 0.25),
    "n129": (lambda: irregular_spd(129, seed=7), 3, 335, 0.25),
}
W_SETS = ("w63x41", "w65x21", "w255x13")
ALL_SETS = tuple(_SETS)

# bodies over a set's systems (min, max), (plain, JACOBI, DIAGONAL): cg_model's, recorded
BODIES = {
    "w63x41": ((26, 40), (26, 28), (29, 37)),
    "w65x21": ((26, 40), (26, 29), (29, 37)),
    "w255x13": ((52, 76), (48, 57), (58, 74)),
    "n128": ((38, 40), (36, 40), (43, 51)),
    "n129": ((75, 123), (38, 44), (45, 55)),
}


@functools.lru_cache(maxsize=None)
def system_set(name):
    """-> (rp, cl, vals, B, tol, X0, max_bodies), as many_systems.system_set;
    the names of many_systems' own sets pass through."""
    if name not in _SETS:
        return M.system_set(name)
    pattern, nsys, seed, width = _SETS[name]
    rp, cl, vl = pattern()
    vals, B = M.variants(rp, cl, vl, nsys, seed=seed, width=width)
    return rp, cl, vals, B, M._tol(B), None, -1


@functools.lru_cache(maxsize=None)
def precond(name, kind):
    """The (nsys, n) m of set `name` under `kind` (JACOBI or DIAGONAL)."""
    rp, cl, vals = system_set(name)[:3]
    out = []
    for s in range(len(vals)):
        d, _ = P.diagonal_of(rp, cl, vals[s])
        m = 1.0 / d
        if kind == DIAGONAL:
            m = m * np.random.default_rng(DIAG_SEED + s).uniform(0.5, 2.0, len(d))
        out.append(m)
    return np.stack(out)
