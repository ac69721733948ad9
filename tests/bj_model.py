"""Block-Jacobi preconditioned CG restated in numpy (cgx.h "block-Jacobi
preconditioning"), on top of tests/cg_model.py's spmv and dot.

  block_inverse      the inverse of one dense SPD block by LDL^T without
                     pivoting, in scalar float64 statements (Python floats are
                     IEEE doubles and nothing here is fused); k_block_inv
                     follows it statement by statement;
  csr_block_inverse  the matrix read (lower triangle of each diagonal block,
                     duplicates summed from 0 in entry order) and W as the
                     n x bs array the engine stores;
  block_apply        z_i = sum_j W[i, j] r[b bs + j], from +0.0 in ascending j
                     over the block's real columns, each product rounded;
  cg                 cg_model.cg's preconditioned loop with z = block_apply.

numpy and the standard library only.
"""
from __future__ import annotations

import numpy as np

from tests import cg_model as M


def _ok(d):
    """pc_ok: positive and finite (False for NaN)."""
    return d > 0.0 and d <= 1.7976931348623157e308


def block_inverse(B):
    """B: m x m (only its lower triangle is read). -> (W, ok): W = L^-T D^-1
    L^-1 as an m x m float64 array, exactly symmetric (the lower triangle is
    computed and mirrored); ok False when a pivot is not positive and finite
    (W then holds whatever the statements give)."""
    m = len(B)
    B = [[float(B[i][j]) for j in range(m)] for i in range(m)]
    L = [[0.0] * m for _ in range(m)]
    Mi = [[0.0] * m for _ in range(m)]
    D = [0.0] * m
    E = [0.0] * m
    ok = True
    for j in range(m):
        s = B[j][j]
        for k in range(j):
            s = s - L[j][k] * (L[j][k] * D[k])
        D[j] = s
        if not _ok(s):
            ok = False
        for i in range(j + 1, m):
            t = B[i][j]
            for k in range(j):
                t = t - L[i][k] * (L[j][k] * D[k])
            L[i][j] = _div(t, s)
        E[j] = _div(1.0, s)
    for i in range(1, m):          # Mi = L^-1, unit lower triangle
        for j in range(i):
            s = L[i][j]
            for k in range(j + 1, i):
                s = s + L[i][k] * Mi[k][j]
            Mi[i][j] = -s
    W = np.zeros((m, m))
    for i in range(m):             # W = Mi^T D^-1 Mi, lower triangle, mirrored
        for j in range(i + 1):
            s = E[i] if j == i else Mi[i][j] * E[i]
            for k in range(i + 1, m):
                s = s + (Mi[k][i] * E[k]) * (Mi[k][i] if j == i else Mi[k][j])
            W[i, j] = s
            W[j, i] = s
    return W, ok


def _div(a, b):
    """IEEE division (Python raises on a zero divisor)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def csr_blocks(rp, cl, vl, bs):
    """The diagonal blocks as the engine reads them: for row i of block b the
    entries of CSR row i with b bs <= col <= i, duplicates summed from 0 in
    entry order (the upper triangle is ignored and left 0 here)."""
    n = len(rp) - 1
    out = []
    for b0 in range(0, n, bs):
        m = min(bs, n - b0)
        B = [[0.0] * m for _ in range(m)]
        for i in range(m):
            for k in range(int(rp[b0 + i]), int(rp[b0 + i + 1])):
                c = int(cl[k]) - b0
                if 0 <= c <= i:
                    B[i][c] = B[i][c] + float(vl[k])
        out.append(B)
    return out


def csr_block_inverse(rp, cl, vl, bs):
    """-> (W, bad): W the n x bs float64 array of cgx_csr_block_inv (the columns
    past a partial last block +0.0), bad the indices of the bad blocks."""
    n = len(rp) - 1
    W = np.zeros((n, bs))
    bad = []
    for b, B in enumerate(csr_blocks(rp, cl, vl, bs)):
        Wb, ok = block_inverse(B)
        m = len(B)
        W[b * bs:b * bs + m, :m] = Wb
        if not ok:
            bad.append(b)
    return W, bad


def block_apply(W, r):
    """z = M^-1 r for W n x bs."""
    n, bs = W.shape
    nb = -(-n // bs)
    rp = np.zeros(nb * bs, r.dtype)
    rp[:n] = r
    R = np.repeat(rp.reshape(nb, bs), bs, axis=0)[:n]    # row i: its block's r
    real = (np.arange(n) // bs * bs)[:, None] + np.arange(bs)[None, :] < n
    z = np.zeros(n, r.dtype)
    with np.errstate(all="ignore"):
        for j in range(bs):
            t = z + W[:, j] * R[:, j]
            z = np.where(real[:, j], t, z)
    return z


def cg(rp, cl, v, b, tol, max_bodies, W, x0=None, keep_x=False):
    """cg_model.cg's preconditioned loop (float64) with z = block_apply(W, r).
    Every dot takes its rounded value; those that are not clear are listed in
    Run.unclear. -> cg_model.Run."""
    dt = np.float64
    v = np.asarray(v, dt)
    b = np.asarray(b, dt)
    W = np.asarray(W, dt)
    n = len(b)
    cap = n + 1 if max_bodies < 0 else min(n + 1, max(int(max_bodies), 1))
    tol = dt(tol)
    unclear = []
    seq = [0]

    def d(name, body, a, c):
        i = seq[0]
        seq[0] += 1
        val, clear, lo, hi, margin = M.dot(a, c)
        if not clear:
            unclear.append(M.Unclear(i, name, body, lo, hi, val, margin))
        return val

    with np.errstate(all="ignore"):
        x = np.zeros(n, dt) if x0 is None else np.array(x0, dt)
        r = b - (np.zeros(n, dt) if x0 is None else M.spmv(rp, cl, v, x))
        rxr = d("r.r", 0, r, r)
        rr0 = rxr
        p = block_apply(W, r)
        rz = d("r.z", 0, r, p)
        bodies, rrs, rzs, xs = 0, [], [], []
        while True:
            Ap = M.spmv(rp, cl, v, p)
            pAp = d("p.Ap", bodies + 1, p, Ap)
            alpha = rz / pAp
            r = r - alpha * Ap
            rr_new = d("r.r", bodies + 1, r, r)
            x = x + alpha * p
            z = block_apply(W, r)
            rz_new = d("r.z", bodies + 1, r, z)
            beta = rz_new / rz
            p = z + beta * p
            rz = rz_new
            rzs.append(rz)
            bodies += 1
            stop = bool(np.isnan(rxr)) or bool(np.sqrt(rxr) <= tol)
            rxr = rr_new
            rrs.append(rxr)
            if keep_x:
                xs.append(x)
            if stop or bodies >= cap:
                return M.Run(x, bodies, rr0, rrs, rzs, unclear, xs)
