"""The systems the block-Jacobi GPU tests compare bit for bit with
tests/bj_model.py, shared with the CPU test that checks every one of them is
ended by the stop rule below its cap with no unclear dot (cg_model's guard),
which is what makes the comparison exact whatever order the device sums in.

A case is a node_mixed matrix (conjugategradient_amd.workloads), a block size
and a kind; b_i = i + 1 normalised, x0 = 0, tol 1e-8. Its matrix seed is the
first one from FIRST_SEED on whose model run is clear: SEEDS records the
search, tests/test_block_pcg_cpu.py repeats it.

  nm396     12 x 11 nodes x 3: blocks = nodes, one workgroup tile
  nm1035    23 x 15 nodes x 3, 1035 rows (odd; no multiple of 2, 4, 6, 7 or
            8): three tiles of update_r, so both sweep directions run and a
            512-row boundary would cut a block for bs = 3, 5, 7; bs = 7 and 8
            leave a partial last block
"""
from __future__ import annotations

import functools

import numpy as np

from conjugategradient_amd.workloads import node_mixed
from tests import bj_model

JACOBI, GIVEN = 1, 2
FIRST_SEED = 7
TOL = 1e-8
E = 1.5

# name: (nx, ny, nodal unknowns, block size, kind)
CASES = {
    "nm396-j3": (12, 11, 3, 3, JACOBI),
    "nm396-g3": (12, 11, 3, 3, GIVEN),
    "nm396-j2": (12, 11, 3, 2, JACOBI),
    "nm1035-j3": (23, 15, 3, 3, JACOBI),
    "nm1035-g5": (23, 15, 3, 5, GIVEN),
    "nm1035-j7": (23, 15, 3, 7, JACOBI),
    "nm1035-j8": (23, 15, 3, 8, JACOBI),
}
# the search's result (first clear seed from FIRST_SEED on)
SEEDS = {
    "nm396-j3": 7, "nm396-g3": 7, "nm396-j2": 7, "nm1035-j3": 7, "nm1035-g5": 7,
    "nm1035-j7": 7, "nm1035-j8": 7,
}


def rhs(n):
    b = np.arange(1, n + 1, dtype=np.float64)
    return b / np.linalg.norm(b)


def given_blocks(rp, cl, vl, bs, seed):
    """A caller's W: the block inverses, each block scaled by its own factor
    in [0.5, 2) (still symmetric positive definite, and not what JACOBI
    builds)."""
    W, bad = bj_model.csr_block_inverse(rp, cl, vl, bs)
    assert not bad
    n = len(rp) - 1
    s = np.random.default_rng(1000 + seed).uniform(0.5, 2.0, -(-n // bs))
    return W * np.repeat(s, bs)[:n, None]


@functools.lru_cache(maxsize=None)
def build(name, seed=None):
    """-> (rp, cl, vl, b, bs, kind, W): W the model's preconditioner (JACOBI:
    what cgx_csr_block_inv must give; GIVEN: what the caller passes)."""
    nx, ny, nu, bs, kind = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    rp, cl, vl = node_mixed(nx, ny, nu, E, seed)
    n = len(rp) - 1
    if kind == JACOBI:
        W, bad = bj_model.csr_block_inverse(rp, cl, vl, bs)
        assert not bad
    else:
        W = given_blocks(rp, cl, vl, bs, seed)
    return rp, cl, vl, rhs(n), bs, kind, W


@functools.lru_cache(maxsize=None)
def model_run(name, seed=None, max_bodies=-1):
    rp, cl, vl, b, bs, kind, W = build(name, seed)
    return bj_model.cg(rp, cl, vl, b, TOL, max_bodies, W)


def clear(name, seed):
    run = model_run(name, seed)
    n = len(build(name, seed)[3])
    return not run.unclear and run.bodies < n + 1
