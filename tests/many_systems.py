"""The systems of the many-systems tests (cgx_many): one
definition for tests/test_many_cpu.py, which checks with tests/cg_model.py
that every one of them has no dot that is not clear, and for
tests/test_gpu_many.py, which compares them bit for bit on the device.

A *set* is (rowptr, col, vals (nsys, nnz), B (nsys, n), tol (nsys) -> one
float, X0 or None, max_bodies): one cgx_many_solve call. The call takes one
absolute tolerance, so a set's tol is 1e-6 of its smallest ||b||.

numpy only.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.util import irregular_spd


def poisson2d(nx, ny):
    """5-point Dirichlet Poisson, x fastest, columns ascending (diag 4, off -1)."""
    n = nx * ny
    i = np.arange(n)
    ix, iy = i % nx, i // nx
    rows = [i[iy > 0], i[ix > 0], i, i[ix < nx - 1], i[iy < ny - 1]]
    cols = [i[iy > 0] - nx, i[ix > 0] - 1, i, i[ix < nx - 1] + 1, i[iy < ny - 1] + nx]
    vals = [np.full(len(r), -1.0) for r in rows]
    vals[2] = np.full(n, 4.0)
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    order = np.lexsort((c, r))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, r + 1, 1)
    return np.cumsum(rp).astype(np.int32), c[order].astype(np.int32), v[order]


def dense_spd(n, seed):
    m = np.random.default_rng(seed).standard_normal((n, n))
    a = m @ m.T + n * np.eye(n)
    rp = np.arange(0, n * n + 1, n, dtype=np.int32)
    cl = np.tile(np.arange(n, dtype=np.int32), n)
    return rp, cl, a.ravel().copy()


def row_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def scaled(rp, cl, vl, d):
    """D A D: symmetric, SPD with A."""
    return d[row_of(rp)] * vl * d[cl]


def variants(rp, cl, vl, nsys, seed, width=1.0):
    """nsys systems on one pattern: system 0 plain with b = 1..n, system s > 0
    scaled by d = 10^(w_s U(0,1)), w_s rising to `width`, with a random b: the
    body counts rise with w_s."""
    n = len(rp) - 1
    rng = np.random.default_rng(seed)
    vals, B = [vl.copy()], [np.arange(1, n + 1, dtype=np.float64)]
    for s in range(1, nsys):
        w = width * s / (nsys - 1)
        d = 10.0 ** (w * rng.uniform(0.0, 1.0, n))
        vals.append(scaled(rp, cl, vl, d))
        B.append(rng.standard_normal(n))
    return np.stack(vals), np.stack(B)


def _tol(B):
    return 1e-6 * float(np.min(np.linalg.norm(B, axis=1)))


def pattern_for(n):
    """The sizes test's pattern: dense SPD up to 5 rows, 2-D Poisson where n
    factors, irregular_spd where it does not."""
    grids = {63: (9, 7), 64: (8, 8), 65: (13, 5), 255: (17, 15), 256: (16, 16), 1023: (33, 31),
             4096: (64, 64)}
    if n <= 5:
        return dense_spd(n, 100 + n)
    if n in grids:
        return poisson2d(*grids[n])
    return irregular_spd(n, seed=7)


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4096)


@functools.lru_cache(maxsize=None)
def system_set(name):
    """-> (rp, cl, vals, B, tol, X0, max_bodies)"""
    if name == "multi":  # 37 systems on the 33 x 31 pattern, body counts from 91 up
        rp, cl, vl = poisson2d(33, 31)
        vals, B = variants(rp, cl, vl, 37, seed=41)
        return rp, cl, vals, B, _tol(B), None, -1
    if name == "multi5":  # the first 5 of them from a non-zero x0, 5 bodies
        rp, cl, vals, B, tol, _, _ = system_set("multi")
        X0 = np.random.default_rng(43).standard_normal((5, B.shape[1]))
        return rp, cl, vals[:5].copy(), B[:5].copy(), tol, X0, 5
    if name == "n1025x9":  # 8 rows per thread, which no size reaches: 9 systems, 41 x 25
        rp, cl, vl = poisson2d(41, 25)
        vals, B = variants(rp, cl, vl, 9, seed=1225, width=0.5)
        return rp, cl, vals, B, _tol(B), None, -1
    if name.startswith("n"):  # the sizes: 3 systems each
        n = int(name[1:])
        rp, cl, vl = pattern_for(n)
        # (n = 1, 2: a dot of one or two products often lies exactly on a
        # rounding boundary, which cg_model counts as not clear; these seeds
        # are the first from 215 up whose three runs have none and a finite x.
        # The narrower scaling keeps the small systems below their cap.)
        seed = {1: 216, 2: 217}.get(n, 200 + n)
        vals, B = variants(rp, cl, vl, 3, seed=seed, width=0.25 if n <= 257 else 1.0)
        return rp, cl, vals, B, _tol(B), None, -1
    if name == "hub":  # a 300-entry row; the milder scaling stays below the cap
        rp, cl, vl = irregular_spd(1000, hub=300, seed=3)
        vals, B = variants(rp, cl, vl, 3, seed=47, width=0.25)
        return rp, cl, vals, B, _tol(B), None, -1
    if name == "empty":  # row (and column) 31 of the 9 x 7 pattern without entries, b_31 = 0
        rp, cl, vl = poisson2d(9, 7)
        k = 31
        keep = (row_of(rp) != k) & (cl != k)
        cnt = np.bincount(row_of(rp)[keep], minlength=len(rp) - 1)
        rp2 = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        vals, B = variants(rp2, cl[keep], vl[keep], 3, seed=53, width=0.25)
        B[:, k] = 0.0
        return rp2, cl[keep], vals, B, _tol(B), None, -1
    raise KeyError(name)


ALL_SETS = ("multi", "multi5", "hub", "empty", "n1025x9") + tuple(f"n{n}" for n in SIZES)
