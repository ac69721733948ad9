"""Block-Jacobi preconditioning (cgx_cg_set_block_precond), the
parts that need no device: the model (tests/bj_model.py) pinned to
tests/cg_model.py where the two must agree, the block inverse's properties
and accuracy, the node_mixed generator, the convergence the feature exists
for, the condition that makes the GPU tests' bit comparisons exact (no
unclear dot, ended by the stop rule below the cap), and the refusals,
exports, bindings and the C++ example's compilation.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from conjugategradient_amd.workloads import node_mixed, node_mixed_blocks
from tests import bj_model, cg_model
from tests import block_pcg_systems as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
NEW_SYMBOLS = ["cgx_csr_block_inv", "cgx_cg_set_block_precond", "cgx_cg_get_block_precond"]
B = cga.BlockPreconditioner


def _err():
    return cga.lib().cgx_last_error().decode()


def _diag(rp, cl, vl):
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    d = np.zeros(n)
    np.add.at(d, rows[rows == cl], vl[rows == cl])
    return d


def _dense(rp, cl, vl):
    n = len(rp) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rp)), cl] = vl
    return A


# -- exports, bindings, refusals ------------------------------------------------
def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    assert [int(k) for k in (B.None_, B.Jacobi, B.Given)] == [0, 1, 2]
    assert hasattr(cga.CG, "setBlockPreconditioner") and hasattr(cga.Matrix, "block_inv")
    assert "BlockPreconditioner" in cga.__all__
    hdr = open(os.path.join(ROOT, "include", "cgx.h")).read()
    assert "CGX_BLOCK_NONE = 0, CGX_BLOCK_JACOBI = 1, CGX_BLOCK_GIVEN = 2" in hdr
    for s in NEW_SYMBOLS:  # each declaration says what it replaces in the reference
        doc = hdr[:hdr.index(f"int {s}(")]
        assert doc.rstrip().endswith("Replaces nothing in the reference. */"), s


def test_refusals_need_no_device():
    """The handle is NULL or made up: a refusal must come before anything
    reads it."""
    L = cga.lib()
    fake = 0x5000  # never dereferenced: every call below is refused first
    assert L.cgx_cg_set_block_precond(None, B.Jacobi, 3, None) == EINVAL
    assert "NULL" in _err()
    for kind in (-1, 3, 17):
        assert L.cgx_cg_set_block_precond(fake, kind, 3, 0x1000) == EINVAL
        assert f"kind {kind}" in _err()
    for bs in (0, -2, 9):
        for kind, d in ((B.Jacobi, None), (B.Given, 0x1000)):
            assert L.cgx_cg_set_block_precond(fake, kind, bs, d) == EINVAL
            assert f"block size {bs}" in _err()
        assert L.cgx_csr_block_inv(fake, bs, 0x1000) == EINVAL
        assert f"block size {bs}" in _err()
    assert L.cgx_cg_set_block_precond(fake, B.Given, 3, None) == EINVAL
    assert "needs d_w" in _err()
    assert L.cgx_cg_set_block_precond(fake, B.Given, 3, 0x1008) == EINVAL
    assert "16-byte aligned" in _err()
    assert L.cgx_csr_block_inv(None, 3, 0x1000) == EINVAL
    assert L.cgx_csr_block_inv(fake, 3, None) == EINVAL
    kind, bs = C.c_int(7), C.c_int(7)
    assert L.cgx_cg_get_block_precond(None, C.byref(kind), C.byref(bs)) == EINVAL
    assert (kind.value, bs.value) == (7, 7)


def test_python_class_refuses_before_any_device_call():
    cg = object.__new__(cga.CG)  # no queue, no solver: a device call would raise
    cg.dtype = np.dtype(np.float64)
    cg._cg = None
    cg.A = object.__new__(cga.Matrix)
    cg.A._N = 12
    with pytest.raises(ValueError, match="unknown block preconditioner kind"):
        cg.setBlockPreconditioner(5, 3)
    for bs in (0, 9):
        with pytest.raises(ValueError, match="block_size"):
            cg.setBlockPreconditioner(B.Jacobi, bs)
    with pytest.raises(ValueError, match="needs blocks"):
        cg.setBlockPreconditioner(B.Given, 3)
    with pytest.raises(ValueError, match="blocks has shape"):
        cg.setBlockPreconditioner(B.Given, 3, np.ones(36))
    with pytest.raises(ValueError, match="blocks has shape"):
        cg.setBlockPreconditioner(B.Given, 3, np.ones((12, 4)))
    with pytest.raises(ValueError, match="blocks has 10 rows"):
        cg.setBlockPreconditioner(B.Given, 3, np.ones((10, 3)))
    cg.setBlockPreconditioner(B.Given, 3, np.ones((12, 3)))
    assert (cg._blk, cg._blk_bs) == (B.Given, 3) and cg._precond == cga.Preconditioner.None_
    cg.setPreconditioner(cga.Preconditioner.Jacobi)  # replaces the block one
    assert cg._blk == B.None_ and cg._precond == cga.Preconditioner.Jacobi
    cg.dtype = np.dtype(np.float32)
    with pytest.raises(TypeError, match="float64"):
        cg.setBlockPreconditioner(B.Jacobi, 3)
    m = object.__new__(cga.Matrix)
    with pytest.raises(ValueError, match="block_size"):
        m.block_inv(9)


def test_block_pcg_check_compiles(tmp_path):
    out = str(tmp_path / "block_pcg_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "block_pcg_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# -- the model against cg_model -------------------------------------------------
def _same_run(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    assert a.bodies == b.bodies and a.rr0 == b.rr0
    assert a.rr == b.rr


@pytest.mark.parametrize("bs", [1, 3, 8])
def test_model_with_a_diagonal_only_w_is_cg_models_diagonal_loop(bs):
    rp, cl, vl = node_mixed(6, 5, 3, 1.0, 7)
    n = len(rp) - 1
    b = S.rhs(n)
    m = 1.0 / _diag(rp, cl, vl)
    W = np.zeros((n, bs))
    W[np.arange(n), np.arange(n) % bs] = m
    ours = bj_model.cg(rp, cl, vl, b, S.TOL, 40, W)
    ref = cg_model.cg(rp, cl, vl, b, S.TOL, 40, minv=m, dtype=np.float64)
    _same_run(ours, ref)
    assert ours.rz == ref.rz and ours.bodies == 40


def test_model_with_identity_w_is_the_plain_loop():
    rp, cl, vl = node_mixed(6, 5, 3, 1.0, 7)
    n = len(rp) - 1
    b = S.rhs(n)
    W = np.zeros((n, 4))
    W[np.arange(n), np.arange(n) % 4] = 1.0
    ours = bj_model.cg(rp, cl, vl, b, S.TOL, 40, W)
    ref = cg_model.cg(rp, cl, vl, b, S.TOL, 40, dtype=np.float64)
    _same_run(ours, ref)
    assert ours.rz == ours.rr  # r.z is r.r under the identity


def test_block_apply_skips_the_columns_past_a_partial_block():
    """n = 7, bs = 3: the last block has one row; its W row holds NaN in the
    two columns that do not exist, and they must not reach z."""
    W = np.arange(1.0, 22.0).reshape(7, 3)
    W[6, 1:] = np.nan
    r = np.arange(1.0, 8.0)
    z = bj_model.block_apply(W, r)
    want = [W[i, 0] * r[i // 3 * 3] + W[i, 1] * r[i // 3 * 3 + 1] + W[i, 2] * r[i // 3 * 3 + 2]
            for i in range(6)] + [W[6, 0] * r[6]]
    np.testing.assert_array_equal(z, want)


# -- the block inverse ----------------------------------------------------------
# max |I - W B| over the diagonal blocks of three node_mixed matrices, per
# block size: the model's and np.linalg.inv's, measured when the test was
# written (both are at the level of cond(B) * eps, cond up to 1e3):
#   bs     1        2        3        4        5        6        7        8
#   model  1.1e-16  1.7e-14  3.4e-14  3.6e-14  3.9e-14  5.3e-14  4.5e-14  5.4e-14
#   numpy  1.1e-16  3.4e-14  8.1e-14  2.5e-13  8.1e-13  4.3e-12  1.4e-12  1.8e-12
# The bar is numpy's error on the same blocks times 4, a small factor for the
# different algorithm (LDL^T with an explicit triangular inverse against LU
# with partial pivoting and a solve).
INV_MATS = [(12, 11, 3), (23, 15, 3), (7, 5, 8)]


@pytest.mark.parametrize("bs", range(1, 9))
def test_block_inverse_symmetric_and_as_accurate_as_numpys(bs):
    em = en = 0.0
    for nx, ny, nu in INV_MATS:
        rp, cl, vl = node_mixed(nx, ny, nu, S.E, 7)
        for Bl in bj_model.csr_blocks(rp, cl, vl, bs):
            A = np.tril(np.array(Bl))
            A = A + np.tril(A, -1).T
            W, ok = bj_model.block_inverse(Bl)
            assert ok
            np.testing.assert_array_equal(W, W.T)
            eye = np.eye(len(A))
            em = max(em, np.abs(eye - W @ A).max())
            en = max(en, np.abs(eye - np.linalg.inv(A) @ A).max())
    print(f"bs {bs}: max |I - W B| model {em:.3e}, numpy {en:.3e}")
    assert em <= 4 * en


def test_block_inverse_of_one_row_is_the_reciprocal():
    rp, cl, vl = node_mixed(12, 11, 3, S.E, 7)
    W, bad = bj_model.csr_block_inverse(rp, cl, vl, 1)
    assert not bad
    np.testing.assert_array_equal(W[:, 0], 1.0 / _diag(rp, cl, vl))


@pytest.mark.parametrize("pivot", [0.0, -1.0, float("nan"), float("inf")])
def test_block_inverse_flags_a_bad_pivot(pivot):
    Bl = [[4.0, 0.0, 0.0], [1.0, 3.0, 0.0], [0.5, 0.25, 2.0]]
    assert bj_model.block_inverse(Bl)[1]
    Bl[1][1] = pivot + 1.0 / 4.0  # d_1 = B11 - L10^2 d_0 = B11 - 1/4
    assert not bj_model.block_inverse(Bl)[1]


def test_matrix_read_takes_the_lower_triangle_and_sums_duplicates():
    # row 1 of block 0: col 0 twice (1.0, then 0.5), the diagonal, an upper
    # entry (ignored) and a column of the next block (ignored); unsorted
    rp = np.array([0, 1, 6, 7])
    cl = np.array([0, 2, 0, 1, 0, 1, 2])
    vl = np.array([4.0, 9.0, 1.0, 3.0, 0.5, 0.0, 2.0])
    blocks = bj_model.csr_blocks(rp, cl, vl, 2)
    assert blocks == [[[4.0, 0.0], [1.5, 3.0]], [[2.0]]]


# -- node_mixed -------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(12, 11, 3), (23, 15, 3), (9, 7, 4), (7, 5, 8), (6, 5, 2)])
def test_node_mixed_is_exactly_symmetric_and_positive_definite(dims):
    rp, cl, vl = node_mixed(*dims, S.E, 7)
    A = _dense(rp, cl, vl)
    assert len(rp) - 1 == dims[0] * dims[1] * dims[2]
    np.testing.assert_array_equal(A, A.T)
    assert np.diff(rp).max() <= 5 * dims[2]
    assert np.linalg.eigvalsh(A).min() > 0


def test_node_mixed_sparse_build_is_the_dense_formula():
    nx, ny, bs = 12, 11, 3
    rp, cl, vl = node_mixed(nx, ny, bs, S.E, 7)
    T = node_mixed_blocks(nx * ny, bs, S.E, 7)
    nn = nx * ny
    Lap = np.zeros((nn, nn))
    for k in range(nn):
        Lap[k, k] = 4.0
        if k % nx < nx - 1:
            Lap[k, k + 1] = Lap[k + 1, k] = -1.0
        if k // nx < ny - 1:
            Lap[k, k + nx] = Lap[k + nx, k] = -1.0
    D = np.zeros((nn * bs, nn * bs))
    for k in range(nn):
        D[k * bs:(k + 1) * bs, k * bs:(k + 1) * bs] = T[k]
    K = np.kron(Lap, np.eye(bs))
    want = D.T @ K @ D
    # both sum the same bs products per entry in some order: the difference is
    # bounded by a few roundings of the sum of their magnitudes
    bound = 8 * bs * np.finfo(float).eps * (np.abs(D.T) @ np.abs(K) @ np.abs(D))
    got = _dense(rp, cl, vl)
    assert (np.abs(got - want) <= bound).all()
    assert ((got != 0) == (np.abs(D.T) @ np.abs(K) @ np.abs(D) != 0)).all()
    sv = np.linalg.svd(T, compute_uv=False)
    assert sv.min() >= 1.0 - 1e-12 and sv.max() <= 10.0 ** S.E * (1 + 1e-12)


# -- what the feature is for ----------------------------------------------------
def test_block_jacobi_needs_a_third_of_jacobis_bodies():
    """node_mixed(12, 11, 3, 1.5, 7), b_i = i + 1 normalised, tol 1e-8, the
    model's counts when the test was written: block-Jacobi 49 bodies, Jacobi
    308, plain CG 397 = the cap n + 1 (residual 7.9e-6)."""
    rp, cl, vl = node_mixed(12, 11, 3, S.E, 7)
    n = len(rp) - 1
    b = S.rhs(n)
    W, bad = bj_model.csr_block_inverse(rp, cl, vl, 3)
    assert not bad
    blk = bj_model.cg(rp, cl, vl, b, S.TOL, -1, W)
    jac = cg_model.cg(rp, cl, vl, b, S.TOL, -1, minv=1.0 / _diag(rp, cl, vl), dtype=np.float64)
    plain = cg_model.cg(rp, cl, vl, b, S.TOL, -1, dtype=np.float64)
    print(f"bodies: block-Jacobi {blk.bodies}, Jacobi {jac.bodies}, plain {plain.bodies} "
          f"(cap {n + 1}, residual {np.sqrt(plain.rr[-1]):.2e})")
    assert 3 * blk.bodies <= jac.bodies < n + 1
    assert plain.bodies == n + 1
    A = _dense(rp, cl, vl)
    assert np.linalg.norm(b - A @ blk.x) <= 2e-8


# -- the GPU tests' systems -----------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_committed_systems_are_the_first_clear_ones(name):
    """The search block_pcg_systems.SEEDS records, run again: the first
    matrix seed from FIRST_SEED on whose model run has no unclear dot and is
    ended by the stop rule below the cap n + 1."""
    found = next(s for s in range(S.FIRST_SEED, S.FIRST_SEED + 40) if S.clear(name, s))
    assert S.SEEDS[name] == found
    run = S.model_run(name)
    n = len(S.build(name)[3])
    print(f"{name}: {run.bodies} bodies of at most {n + 1}")
    assert not run.unclear and run.bodies < n + 1
    assert np.sqrt(run.rr[-2]) <= S.TOL  # the stop rule saw this r.r
