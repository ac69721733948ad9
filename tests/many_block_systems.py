"""The systems of the block-preconditioned many-systems tests
(cgx_many_set_block_precond): one definition for
tests/test_many_block_pcg_cpu.py, which checks with tests/bj_model.py that
every one of them has no dot that is not clear, and for
tests/test_gpu_many_block_pcg.py, which compares them bit for bit on the
device.

A set's pattern is the leading principal submatrix of
workloads.node_mixed(nx, ny, bs, 1.5, seed) cut to n rows: still SPD, and the
cut makes the partial last block. Its systems are many_systems.variants of
that matrix (system 0 the matrix itself with b = 1..n, the others scaled with
a random b). A set's preconditioner is an (nsys, n, bs) array W:

  JACOBI  W = bj_model.csr_block_inverse of the system's own values;
  GIVEN   the same, each block scaled by its own factor in [0.5, 2) drawn from
          seed GIVEN_SEED + s (still symmetric positive definite, and not what
          JACOBI builds).

SEEDS[name] = (matrix seed, variants seed): the first pair, matrix seed from 7
up and variants seed from 300 up (the variants seed moves first), for which
every system of the set has no unclear dot under both kinds; search() is the
search that found them, and the CPU test asserts the condition for each.

numpy only.
"""
from __future__ import annotations

import functools

import numpy as np

from conjugategradient_amd.workloads import node_mixed
from tests import bj_model
from tests import many_systems as M

NONE, JACOBI, GIVEN = 0, 1, 2
KINDS = {"jacobi": JACOBI, "given": GIVEN}
E = 1.5
GIVEN_SEED = 1100
FIRST_MATRIX_SEED, FIRST_VARIANTS_SEED, VARIANTS_SEEDS = 7, 300, 12

# name: (nx, ny, bs, n, nsys, width of the variants' scaling, max_bodies, with x0)
SETS = {
    # the workgroup form
    "n257b3": (10, 9, 3, 257, 3, 0.25, -1, False),    # block {255, 256} wraps thread 255 -> 0
    "n396b3": (12, 11, 3, 396, 3, 0.25, -1, False),   # 2 rows per thread
    "n1023b7": (13, 12, 7, 1023, 3, 0.25, -1, False),  # 4 rows per thread, a partial block of 1
    "n4096b8": (32, 16, 8, 4096, 3, 0.25, 12, False),  # 16 rows per thread; capped
    "n4096b5": (29, 29, 5, 4096, 3, 0.25, 12, False),  # the same, a partial block of 1; capped
    # the wave form (and, up to 64 rows, both)
    "n60b3": (5, 4, 3, 60, 3, 0.25, -1, False),       # small whole blocks
    "n65b3": (6, 4, 3, 65, 3, 0.25, -1, False),       # block {63, 64} wraps lane 63 -> 0
    "n255b8": (8, 4, 8, 255, 3, 0.25, -1, False),     # 4 rows per lane, a partial block of 7
    "n256b8": (8, 4, 8, 256, 3, 0.25, -1, False),     # 4 rows per lane, whole blocks
    # a single partial block
    "n1b3": (1, 1, 3, 1, 3, 0.25, -1, False),
    "n2b3": (1, 1, 3, 2, 3, 0.25, -1, False),
    "n7b8": (1, 1, 8, 7, 3, 0.25, -1, False),
    # several systems per workgroup and per wave; a non-zero x0 with a cap of 5
    "multi11": (5, 4, 3, 60, 11, 0.5, -1, False),
    "n396b3x0": (12, 11, 3, 396, 5, 0.25, 5, True),
}
# the search's result (search(name)); n <= 2 as many_pcg_systems.SMALL_SEEDS
SEEDS = {
    "n257b3": (7, 300), "n396b3": (7, 300), "n1023b7": (7, 300), "n4096b8": (7, 300),
    "n4096b5": (7, 300), "n60b3": (7, 300), "n65b3": (7, 300), "n255b8": (7, 300),
    "n256b8": (7, 300), "n1b3": (7, 300), "n2b3": (19, 300), "n7b8": (7, 305),
    "multi11": (7, 300), "n396b3x0": (7, 300),
}
# (set, kind) -> the systems whose x holds a NaN: a system of one block is
# solved exactly by its first body, and the next body forms 0 / 0, as the
# single solve does
NAN_X = {("n1b3", "jacobi"): (0, 2), ("n2b3", "jacobi"): (0,)}


def cut(rp, cl, vl, n):
    """The leading principal n x n submatrix of a CSR matrix."""
    rows = M.row_of(rp)
    keep = (rows < n) & (np.asarray(cl) < n)
    cnt = np.bincount(rows[keep], minlength=len(rp) - 1)[:n]
    rp2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    return rp2, np.asarray(cl)[keep].astype(np.int32), np.asarray(vl, np.float64)[keep]


@functools.lru_cache(maxsize=None)
def build(name, seeds=None):
    """-> (rp, cl, vals (nsys, nnz), B (nsys, n), tol, X0 or None, max_bodies, bs)"""
    nx, ny, bs, n, nsys, width, max_bodies, with_x0 = SETS[name]
    mseed, vseed = SEEDS[name] if seeds is None else seeds
    rp, cl, vl = cut(*node_mixed(nx, ny, bs, E, mseed), n)
    vals, B = M.variants(rp, cl, vl, nsys, seed=vseed, width=width)
    X0 = np.random.default_rng(vseed + 1).standard_normal(B.shape) if with_x0 else None
    return rp, cl, vals, B, M._tol(B), X0, max_bodies, bs


def system_set(name):
    return build(name)


@functools.lru_cache(maxsize=None)
def precond(name, kind, seeds=None):
    """The (nsys, n, bs) W of set `name` under `kind` (JACOBI or GIVEN)."""
    rp, cl, vals, B, tol, X0, mb, bs = build(name, seeds)
    n = len(rp) - 1
    out = []
    for s in range(len(vals)):
        W, bad = bj_model.csr_block_inverse(rp, cl, vals[s], bs)
        assert not bad
        if kind == GIVEN:
            f = np.random.default_rng(GIVEN_SEED + s).uniform(0.5, 2.0, -(-n // bs))
            W = W * np.repeat(f, bs)[:n, None]
        out.append(W)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def model_runs(name, kind, seeds=None):
    """bj_model.cg of every system of the set under `kind` ("jacobi", "given")."""
    rp, cl, vals, B, tol, X0, mb, bs = build(name, seeds)
    W = precond(name, KINDS[kind], seeds)
    return [bj_model.cg(rp, cl, vals[s], B[s], tol, mb, W[s], x0=None if X0 is None else X0[s])
            for s in range(len(vals))]


def clear(name, seeds):
    """Every system of the set, under both kinds, has no unclear dot."""
    return all(not run.unclear for kind in KINDS for run in model_runs(name, kind, seeds))


def search(name):
    """The first (matrix seed, variants seed) whose set is clear."""
    for mseed in range(FIRST_MATRIX_SEED, FIRST_MATRIX_SEED + 40):
        for vseed in range(FIRST_VARIANTS_SEED, FIRST_VARIANTS_SEED + VARIANTS_SEEDS):
            if clear(name, (mseed, vseed)):
                return mseed, vseed
    raise LookupError(name)


ALL_SETS = tuple(SETS)
