"""The systems and preconditioners of the preconditioned many-systems tests
(cgx_many_set_precond): one definition for
tests/test_many_pcg_cpu.py, which checks with tests/cg_model.py that every
one of them has no dot that is not clear, and for tests/test_gpu_many_pcg.py,
which compares them bit for bit on the device.

The sets are tests/many_systems.py's, but for n = 1 and 2, whose seeds do not
carry over (below). A set's preconditioner is an (nsys, n) array m:

  JACOBI    m = 1 / d with d the system's own diagonal, the entries with
            col == row summed from 0 in entry order (k_diag_inv's expression);
  DIAGONAL  m = (1 / d) U(0.5, 2), drawn per system from seed DIAG_SEED + s.
            The `empty` set has no diagonal entry in row 31: its m is 1 there.

numpy only.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import many_systems as M

NONE, JACOBI, DIAGONAL = 0, 1, 2
KINDS = {"jacobi": JACOBI, "diagonal": DIAGONAL}
DIAG_SEED = 900
EMPTY_ROW = 31

# n = 1, 2: a dot of one or two products often lies on a rounding boundary
# (the sum of two doubles of one exponent is a tie half of the time), and the
# seeds many_systems.py found for the plain loop do not stay clear under a
# preconditioner. (matrix seed of dense_spd, seed of variants):
#   n = 1  many_systems' matrix; the first variants seed from 215 up whose
#          three runs have no dot that is not clear under JACOBI and DIAGONAL;
#   n = 2  system 0 (the matrix itself, b = 1, 2) does not depend on the
#          variants seed and is not clear under DIAGONAL on many_systems'
#          matrix (seed 102), so the matrix seed moves too: the first from
#          102 up for which a variants seed in 215..254 leaves all three runs
#          clear under both kinds, and the first such variants seed.
# tests/test_many_pcg_cpu.py checks both. x may be NaN: a small system is
# solved exactly before the stop rule sees it, and the next body forms 0 / 0
# as the single solve does; NAN_X pins which (set, kind) -> systems those are.
SMALL_SEEDS = {1: (101, 215), 2: (109, 228)}
NAN_X = {("n1", "jacobi"): (0, 1, 2), ("n1", "diagonal"): (1,), ("n2", "diagonal"): (0,)}


@functools.lru_cache(maxsize=None)
def system_set(name):
    """-> (rp, cl, vals, B, tol, X0, max_bodies), as many_systems.system_set"""
    if name in ("n1", "n2"):
        n = int(name[1:])
        mseed, vseed = SMALL_SEEDS[n]
        rp, cl, vl = M.dense_spd(n, mseed)
        vals, B = M.variants(rp, cl, vl, 3, seed=vseed, width=0.25)
        return rp, cl, vals, B, M._tol(B), None, -1
    return M.system_set(name)


def diagonal_of(rp, cl, vl):
    """d_i: row i's entries with col == i summed from 0 in entry order (0
    where there is none), and whether the row has one."""
    n = len(rp) - 1
    rows = M.row_of(rp)
    idx = np.nonzero(np.asarray(cl) == rows)[0]
    d = np.zeros(n)
    np.add.at(d, rows[idx], np.asarray(vl, np.float64)[idx])  # unbuffered: in entry order
    found = np.zeros(n, bool)
    found[rows[idx]] = True
    return d, found


@functools.lru_cache(maxsize=None)
def precond(name, kind):
    """The (nsys, n) m of set `name` under `kind` (JACOBI or DIAGONAL). JACOBI
    of `empty` holds inf in row 31: that set is refused under JACOBI."""
    rp, cl, vals = system_set(name)[:3]
    out = []
    for s in range(len(vals)):
        d, found = diagonal_of(rp, cl, vals[s])
        with np.errstate(divide="ignore"):
            m = 1.0 / d
        if kind == DIAGONAL:
            m = m * np.random.default_rng(DIAG_SEED + s).uniform(0.5, 2.0, len(d))
            m[~found] = 1.0
        out.append(m)
    return np.stack(out)


ALL_SETS = M.ALL_SETS
SIZES = M.SIZES
