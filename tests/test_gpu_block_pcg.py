"""Block-Jacobi preconditioning on the device (cgx_cg_set_block_precond;
DESIGN.md §5f): k_block_inv, k_block_check, k_pc_init_blk, k_update_r_blk,
k_update_xp_blk and k_update_p_defer_blk against tests/bj_model.py, bit for
bit (every comparison of x, bodies, r.r, r.z and stop code is exact: the
systems of tests/block_pcg_systems.py have no unclear dot), cross-pinned to
the diagonal and the plain solver, and the driver, error, switching and
refusal behaviour around them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from conjugategradient_amd.workloads import node_mixed
from tests import bj_model, cg_model
from tests import block_pcg_systems as S
from tests.test_gpu_pcg import _tridiag5

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "block_pcg_check")
P, B = cga.Preconditioner, cga.BlockPreconditioner
EINVAL, ESTATE, EUNSUPPORTED = 1, 4, 6


def _err():
    return lib().cgx_last_error().decode()


class Solver:
    """A raw cgx_cg on a Matrix, with the arrays a solve needs kept alive."""

    def __init__(self, queue, m, mode=0, poll=0, graph=-1):
        self.queue, self.m, self.n = queue, m, m.N()
        self.dtype = m.dtype
        self.h = C.c_void_p()
        check(lib().cgx_cg_create(queue.handle, m.schedule(), C.byref(self.h)))
        check(lib().cgx_cg_set_mode(self.h, mode))
        check(lib().cgx_cg_config(self.h, poll, graph))
        self.keep = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        lib().cgx_cg_destroy(self.h)
        self.h = None

    def dev(self, a):
        d = cga.DeviceArray(self.queue, np.size(a), self.dtype).upload(np.ravel(a))
        self.keep.append(d)
        return d

    def block_rc(self, kind, bs=0, W=None):
        return lib().cgx_cg_set_block_precond(self.h, int(kind), bs,
                                              self.dev(W).ptr if W is not None else None)

    def block(self, kind, bs=0, W=None):
        check(self.block_rc(kind, bs, W))
        return self

    def diag(self, kind, m=None):
        check(lib().cgx_cg_set_precond(self.h, int(kind),
                                       self.dev(m).ptr if m is not None else None))
        return self

    def kinds(self):
        k, bk, bs = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        check(lib().cgx_cg_get_precond(self.h, C.byref(k)))
        check(lib().cgx_cg_get_block_precond(self.h, C.byref(bk), C.byref(bs)))
        return k.value, bk.value, bs.value

    def mode(self):
        v = C.c_int(-1)
        check(lib().cgx_cg_get_mode(self.h, C.byref(v)))
        return v.value

    def solve(self, b, tol=0.0, cap=-1, x0=None, split=None, rz=True):
        """(x, bodies, stop code, r.r, r.z) of begin + run(s); split: the
        bodies of the first cgx_cg_run calls."""
        n = self.n
        db, dx = self.dev(b), self.dev(np.zeros(n) if x0 is None else x0)
        check(lib().cgx_cg_begin(self.h, db.ptr, dx.ptr, tol, cap))
        total, stopped, rxr, rzv = C.c_int64(), C.c_int(), C.c_double(), C.c_double(np.nan)
        for k in list(split or []) + [n + 1]:
            check(lib().cgx_cg_run(self.h, k, C.byref(total), C.byref(stopped)))
        check(lib().cgx_cg_rxr(self.h, C.byref(rxr)))
        if rz:
            check(lib().cgx_cg_rz(self.h, C.byref(rzv)))
        out = (dx.download(), total.value, stopped.value, rxr.value, rzv.value)
        self.keep.clear()
        return out


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(np.array(a[1:]), np.array(b[1:]))


def _model_out(run, stopped=1):
    return (run.x, run.bodies, stopped, float(run.rr[-1]), float(run.rz[-1]))


_mats = {}


def _matrix(queue, key):
    """One device Matrix per node_mixed configuration (or case name), shared."""
    if key not in _mats:
        if isinstance(key, str):
            rp, cl, vl = S.build(key)[:3]
        else:
            rp, cl, vl = node_mixed(*key)
        _mats[key] = (cga.Matrix(queue, vl, cl, rp), rp, cl, vl)
    return _mats[key]


# 1 -- cgx_csr_block_inv --------------------------------------------------------
def _dense_spd(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, n))
    A = G @ G.T + n * np.eye(n)
    A = np.triu(A) + np.triu(A, 1).T
    r, c = np.nonzero(np.ones((n, n)))
    rp = np.arange(0, n * n + 1, n).astype(np.int32)
    return rp, c.astype(np.int32), A[r, c]


def _shuffled_split(rp, cl, vl, bs_max=8):
    """Every row's entries reversed, and each entry within bs_max columns of
    the diagonal split in two parts (0.25 of it first in the row, the rest
    where it was): unsorted rows with duplicates inside every diagonal block."""
    rows, cols, vals = [0], [], []
    for i in range(len(rp) - 1):
        c, v = cl[rp[i]:rp[i + 1]][::-1], vl[rp[i]:rp[i + 1]][::-1]
        near = np.abs(c - i) < bs_max
        cols.append(np.concatenate([c[near], c]))
        vals.append(np.concatenate([0.25 * v[near], np.where(near, v - 0.25 * v, v)]))
        rows.append(rows[-1] + len(cols[-1]))
    return np.array(rows, np.int32), np.concatenate(cols).astype(np.int32), np.concatenate(vals)


INV_CASES = {"n1": lambda: _dense_spd(1, 1), "n2": lambda: _dense_spd(2, 2),
             "n7": lambda: _dense_spd(7, 3), "n396": lambda: node_mixed(12, 11, 3, S.E, 7),
             "n1035": lambda: node_mixed(23, 15, 3, S.E, 7),
             "shuffled-split": lambda: _shuffled_split(*node_mixed(6, 5, 3, S.E, 7))}


@pytest.mark.parametrize("name", list(INV_CASES))
def test_block_inv_is_the_models_bit_for_bit(queue, name):
    """bs = 1..8 on n = 1, 2, 7 (n < bs: one partial block), 396, 1035 (not a
    multiple of 2, 4, 6, 7 or 8) and on unsorted rows with duplicate entries."""
    rp, cl, vl = INV_CASES[name]()
    if name == "shuffled-split":
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        assert (np.bincount(rows[rows == cl]) == 2).all() and (np.diff(cl[:4]) < 0).any()
    m = cga.Matrix(queue, vl, cl, rp)
    for bs in range(1, 9):
        W, bad = bj_model.csr_block_inverse(rp, cl, vl, bs)
        assert not bad
        got = m.block_inv(bs)
        assert got.shape == W.shape
        np.testing.assert_array_equal(got, W, err_msg=f"{name} bs {bs}")
        np.testing.assert_array_equal(np.signbit(got), np.signbit(W))  # -0.0 is not +0.0
        last = (len(rp) - 1) // bs * bs  # the partial block's padding columns are +0.0
        pad = got[last:, len(rp) - 1 - last:]
        assert not pad.any() and not np.signbit(pad).any()
    np.testing.assert_array_equal(m.block_inv(1)[:, 0], m.diag_inv())


# 2 -- solves against the model -------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("name", list(S.CASES))
def test_solve_is_the_models_bit_for_bit(queue, name, mode):
    rp, cl, vl, b, bs, kind, W = S.build(name)
    m = _matrix(queue, name)[0]
    want = _model_out(S.model_run(name))
    with Solver(queue, m, mode) as s:
        s.block(kind, bs, W if kind == S.GIVEN else None)
        assert s.kinds() == (P.None_, kind, bs) and s.mode() == mode
        got = s.solve(b, S.TOL)
    print(f"{name} mode {mode}: {got[1]} bodies, r.r {got[3]:.17g}, r.z {got[4]:.17g}")
    _same(got, want)


# 3 -- cross-pins that need no model -------------------------------------------
# the matrices of test_gpu_pcg.py::test_tiny_systems
TINY = [np.array([[4.0]]), np.array([[4.0, 1.0], [1.0, 3.0]]), _tridiag5()]


@pytest.mark.parametrize("bs", range(2, 9))
def test_given_diagonal_w_is_the_diagonal_solver_and_identity_the_plain_one(queue, bs):
    """GIVEN with a W whose only entries are its diagonal is
    cgx_cg_set_precond(DIAGONAL) with that diagonal, and with the identity the
    plain solver, bit for bit, on finite systems: z_i = +0.0 + w r_i + 0 r_j +
    ... equals m_i r_i unless r_i is -0.0 (the sum from +0.0 turns it into
    +0.0): the one case where the bits could differ, which needs an r entry of
    exactly zero and does not occur on these systems."""
    m, rp, cl, vl = _matrix(queue, (23, 15, 3, S.E, 7))
    n = m.N()
    b = S.rhs(n)
    d = np.random.default_rng(bs).uniform(0.5, 2.0, n) * m.diag_inv()
    Wd = np.zeros((n, bs))
    Wd[np.arange(n), np.arange(n) % bs] = d
    Wi = (Wd != 0).astype(np.float64)
    for mode in (1, 3):
        with Solver(queue, m, mode) as s:
            blk = s.block(B.Given, bs, Wd).solve(b, 0.0, 45)
            ident = s.block(B.Given, bs, Wi).solve(b, 0.0, 45)
            dia = s.diag(P.Diagonal, d).solve(b, 0.0, 45)
            plain = s.diag(P.None_).solve(b, 0.0, 45, rz=False)
        assert blk[1] == 45 and blk[2] == 2
        _same(blk, dia)
        _same(ident[:4], plain[:4])
        assert ident[4] == ident[3]  # r.z is r.r


def _start_residuals(rp, cl, vl, b, W, bodies):
    """r at the start of bodies 1 .. `bodies`, by bj_model.cg's statements."""
    r = np.array(b, np.float64)
    p = bj_model.block_apply(W, r)
    rz = cg_model.dot(r, p)[0]
    out = []
    for _ in range(bodies):
        out.append(r)
        Ap = cg_model.spmv(rp, cl, vl, p)
        r = r - (rz / cg_model.dot(p, Ap)[0]) * Ap
        z = bj_model.block_apply(W, r)
        rzn = cg_model.dot(r, z)[0]
        p = z + (rzn / rz) * p
        rz = rzn
    return out


@pytest.mark.parametrize("dense", TINY, ids=["n1", "n2", "n5"])
@pytest.mark.parametrize("mode", [1, 3])
def test_tiny_systems_given_diagonal_w_and_identity(queue, dense, mode):
    """The cross-pins of the test above on test_gpu_pcg.py::test_tiny_systems'
    matrices (n = 1, 2, 5; b_i = i + 1), bs = 1, 2, 3 (n = 1, 2: one partial
    block), 1 .. n bodies: the vector kernels' n >> 1 == 0 clamped loads and
    their odd-n tail with z read from the z buffer. No body starts from an r
    with a zero entry (asserted on the model's r), so no -0.0 can differ."""
    n = len(dense)
    r, c = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    cl, vl = c.astype(np.int32), dense[r, c]
    m = cga.Matrix(queue, vl, cl, rp)
    b = np.arange(1, n + 1, dtype=np.float64)
    d = np.random.default_rng(n).uniform(0.5, 2.0, n) / np.diag(dense)
    with Solver(queue, m, mode) as s:
        for bs in (1, 2, 3):
            Wd = np.zeros((n, bs))
            Wd[np.arange(n), np.arange(n) % bs] = d
            Wi = (Wd != 0).astype(np.float64)
            for W in (Wd, Wi):
                assert all((rk != 0).all() for rk in _start_residuals(rp, cl, vl, b, W, n))
            for bodies in range(1, n + 1):
                blk = s.block(B.Given, bs, Wd).solve(b, 0.0, bodies)
                ident = s.block(B.Given, bs, Wi).solve(b, 0.0, bodies)
                dia = s.diag(P.Diagonal, d).solve(b, 0.0, bodies)
                plain = s.diag(P.None_).solve(b, 0.0, bodies, rz=False)
                assert blk[1] == bodies
                _same(blk, dia)
                _same(ident[:4], plain[:4])
                assert ident[4] == ident[3]  # r.z is r.r


def test_block_jacobi_of_one_row_is_jacobi(queue):
    for key in ((23, 15, 3, S.E, 7), (12, 11, 3, S.E, 7)):
        m = _matrix(queue, key)[0]
        b = S.rhs(m.N())
        for mode in (1, 3):
            with Solver(queue, m, mode) as s:
                blk = s.block(B.Jacobi, 1).solve(b, S.TOL)
                jac = s.diag(P.Jacobi).solve(b, S.TOL)
            assert blk[2] == 1
            _same(blk, jac)


# 4 -- driver behaviour ---------------------------------------------------------
@pytest.mark.parametrize("bodies", [29, 30, 31, 32])
def test_deferred_x_group_boundaries(queue, bodies):
    rp, cl, vl, b, bs, kind, W = S.build("nm1035-j3")
    m = _matrix(queue, "nm1035-j3")[0]
    want = S.model_run("nm1035-j3", None, bodies)
    assert want.bodies == bodies
    for mode in (1, 3):
        with Solver(queue, m, mode) as s:
            _same(s.block(B.Jacobi, bs).solve(b, S.TOL, bodies), _model_out(want, 2))


def test_graph_eager_poll_interval_and_split_runs(queue):
    rp, cl, vl, b, bs, kind, W = S.build("nm1035-j3")
    m = _matrix(queue, "nm1035-j3")[0]
    want = _model_out(S.model_run("nm1035-j3"))
    for graph, poll in ((1, 5), (0, 5), (1, 1), (0, 32)):
        with Solver(queue, m, 3, poll, graph) as s:
            _same(s.block(B.Jacobi, bs).solve(b, S.TOL), want)
    for mode in (1, 3):
        with Solver(queue, m, mode) as s:
            s.block(B.Jacobi, bs)
            _same(s.solve(b, S.TOL, split=[1, 2, 7, 30]), want)
            _same(s.solve(b, S.TOL), want)  # the same solver again


def test_warm_start_with_a_cap(queue):
    rp, cl, vl, b, bs, kind, W = S.build("nm396-g3")
    m = _matrix(queue, "nm396-g3")[0]
    x0 = 0.5 * S.model_run("nm396-g3").x
    want = bj_model.cg(rp, cl, vl, b, S.TOL, 20, W, x0=x0)
    assert want.bodies == 20 and not want.unclear
    for mode in (1, 3):
        with Solver(queue, m, mode) as s:
            _same(s.block(B.Given, bs, W).solve(b, S.TOL, 20, x0=x0), _model_out(want, 2))


# 5 -- errors -------------------------------------------------------------------
def _with_diagonal(rp, cl, vl, row, how):
    rp, cl, vl = rp.copy(), cl.copy(), vl.copy()
    k = rp[row] + int(np.nonzero(cl[rp[row]:rp[row + 1]] == row)[0][0])
    if how == "missing":
        cl, vl = np.delete(cl, k), np.delete(vl, k)
        rp[row + 1:] -= 1
    else:
        vl[k] = {"zero": 0.0, "negative": -1.0, "nan": np.nan}[how]
    return rp, cl, vl


@pytest.mark.parametrize("how", ["zero", "negative", "nan", "missing"])
def test_bad_block_is_einval_naming_the_block(queue, how):
    """Row 21 = row 0 of block 7 (bs = 3): its diagonal entry is the block's
    first pivot. zero and missing give d = 0, and the model agrees."""
    rp, cl, vl = _with_diagonal(*node_mixed(6, 5, 3, S.E, 7), 21, how)
    assert bj_model.csr_block_inverse(rp, cl, vl, 3)[1] == [7]
    m = cga.Matrix(queue, vl, cl, rp)
    L = lib()
    out = cga.DeviceArray(queue, m.N() * 3)
    assert L.cgx_csr_block_inv(m.schedule(), 3, out.ptr) == EINVAL
    msg = _err()
    assert "1 block" in msg and "block 7" in msg and "row 21" in msg, msg
    with pytest.raises(cga.CgxError, match="block 7"):
        m.block_inv(3)
    with Solver(queue, m) as s:
        s.diag(P.Diagonal, np.ones(m.N()))
        assert s.block_rc(B.Jacobi, 3) == EINVAL and "block 7" in _err()
        assert s.kinds() == (P.Diagonal, B.None_, 0)  # the solver keeps what it had


def test_given_w_is_checked(queue):
    m = _matrix(queue, (12, 11, 3, S.E, 7))[0]
    n = m.N()
    W0 = m.block_inv(3)
    with Solver(queue, m) as s:
        s.block(B.Jacobi, 2)
        for bad, at in ((np.nan, (40, 1)), (np.inf, (40, 0)), (0.0, (40, 1)), (-1.0, (40, 1)),
                        (np.nan, (40, 2))):
            W = W0.copy()
            W[at] = bad  # row 40 is row 1 of block 13: column 1 is its diagonal entry
            assert s.block_rc(B.Given, 3, W) == EINVAL, (bad, at)
            assert "row 40" in _err() and "block 13" in _err(), _err()
            assert s.kinds() == (P.None_, B.Jacobi, 2)
        # the columns past a partial block are not read: n = 396, bs = 5
        W = np.zeros((n, 5))
        W[np.arange(n), np.arange(n) % 5] = 1.0
        W[395, 1:] = np.nan
        s.block(B.Given, 5, W)
        assert s.kinds() == (P.None_, B.Given, 5)


# 6 -- switching ----------------------------------------------------------------
def test_switching_preconditioners_on_one_solver(queue):
    m = _matrix(queue, (23, 15, 3, S.E, 7))[0]
    b = S.rhs(m.N())
    d = m.diag_inv()

    def fresh(setup, rz=True):
        with Solver(queue, m) as s:
            setup(s)
            return s.solve(b, S.TOL, 60, rz=rz)

    with Solver(queue, m) as s:
        rzv = C.c_double()
        assert lib().cgx_cg_rz(s.h, C.byref(rzv)) == ESTATE
        s.diag(P.Diagonal, d)
        assert s.kinds() == (P.Diagonal, B.None_, 0) and s.mode() == 3
        _same(s.solve(b, S.TOL, 60), fresh(lambda t: t.diag(P.Jacobi)))
        s.block(B.Jacobi, 3)
        assert s.kinds() == (P.None_, B.Jacobi, 3) and s.mode() == 3
        _same(s.solve(b, S.TOL, 60), fresh(lambda t: t.block(B.Jacobi, 3)))
        s.block(B.None_)
        assert s.kinds() == (P.None_, B.None_, 0)
        _same(s.solve(b, S.TOL, 60, rz=False), fresh(lambda t: None, rz=False))
        assert lib().cgx_cg_rz(s.h, C.byref(rzv)) == ESTATE
        s.block(B.Jacobi, 5)
        s.diag(P.Jacobi)  # replaces the block one
        assert s.kinds() == (P.Jacobi, B.None_, 0)
        _same(s.solve(b, S.TOL, 60), fresh(lambda t: t.diag(P.Jacobi)))
        s.block(B.Jacobi, 5)
        s.diag(P.None_)  # and so does NONE
        assert s.kinds() == (P.None_, B.None_, 0)


# 7 -- refusals -----------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 4, 5, 6, 7])
def test_other_modes_refuse_a_block_preconditioner(queue, monkeypatch, mode):
    if mode == 6:  # needs the lean stencil walk
        monkeypatch.setenv("CGX_SPMV_VARIANT", "33554432:0")
        m = cga.Matrix.poisson(queue, 3, 128, 48, 40)
    elif mode == 7:  # the smallest shape the ring form of the tile walk takes
        m = cga.Matrix.poisson(queue, 3, 256, 128, 128)
    else:
        m = cga.Matrix.poisson(queue, 2, 30, 30)
    with Solver(queue, m) as s:  # the mode first, then the preconditioner
        check(lib().cgx_cg_set_mode(s.h, mode))  # the mode itself runs on this matrix
        assert s.block_rc(B.Jacobi, 2) == EUNSUPPORTED
        assert "modes 1 and 3" in _err() and "block" in _err()
        assert s.mode() == mode and s.kinds() == (P.None_, B.None_, 0)
    with Solver(queue, m) as s:  # the preconditioner first, then the mode
        s.block(B.Jacobi, 2)
        assert s.mode() == 3  # auto with a preconditioner
        assert lib().cgx_cg_set_mode(s.h, mode) == EUNSUPPORTED
        assert "modes 1 and 3" in _err() and "block" in _err()
        assert s.mode() == 3
        check(lib().cgx_cg_set_mode(s.h, 1))
        assert s.mode() == 1 and s.kinds() == (P.None_, B.Jacobi, 2)


def test_f32_mixed_and_the_fused_batch_refuse(queue):
    rp, cl, vl = node_mixed(6, 5, 3, S.E, 7)
    n = len(rp) - 1
    m32 = cga.Matrix(queue, vl, cl, rp, dtype=np.float32)
    with Solver(queue, m32) as s:
        assert s.block_rc(B.Jacobi, 3) == EUNSUPPORTED and "f32" in _err()
        assert s.kinds() == (P.None_, B.None_, 0)
    out = cga.DeviceArray(queue, 3 * n, np.float32)
    assert lib().cgx_csr_block_inv(m32.schedule(), 3, out.ptr) == EUNSUPPORTED and "f32" in _err()
    cg = cga.CG(queue)
    cg.setMatrix(cga.Matrix(queue, vl, cl, rp))
    cg.setTarget(S.rhs(n))
    cg.setBlockPreconditioner(B.Jacobi, 3)
    with pytest.raises(cga.CgxError, match="f32"):
        cg.solve_mixed(S.TOL)
    cg.batch_form = 1
    with pytest.raises(cga.CgxError, match="preconditioner is set"):
        cg.solve_batch(np.ones((n, 3)))


def test_sequential_batch_is_three_single_solves(queue):
    rp, cl, vl, b, bs, kind, W = S.build("nm396-j3")
    n = len(b)
    Bm = np.stack([b, b[::-1].copy(), np.cos(np.arange(n))], axis=1)
    cg = cga.CG(queue)
    cg.setMatrix(_matrix(queue, "nm396-j3")[0])
    cg.setBlockPreconditioner(B.Jacobi, bs)
    cg.batch_form = 2
    X = cg.solve_batch(Bm, improvement=S.TOL)
    assert cg.batch_info()[0] == 2
    for c in range(3):
        one = cga.CG(queue)
        one.setMatrix(_matrix(queue, "nm396-j3")[0])
        one.setTarget(Bm[:, c].copy())
        one.setBlockPreconditioner(B.Jacobi, bs)
        one.solve(S.TOL)
        np.testing.assert_array_equal(X[:, c], one.extract())
        assert cg.iterations_batch[c] == one.iterations
        assert cg.final_rxr_batch[c] == one.final_rxr and cg.stopped_batch[c] == 1
    assert cg.iterations_batch[0] == S.model_run("nm396-j3").bodies


# 8 -- bindings -----------------------------------------------------------------
def test_python_class(queue):
    for name in ("nm396-g3", "nm1035-j7"):
        rp, cl, vl, b, bs, kind, W = S.build(name)
        want = S.model_run(name)
        cg = cga.CG(queue)
        cg.setMatrix(vl, cl, rp)
        cg.setTarget(b)
        cg.setBlockPreconditioner(kind, bs, W if kind == S.GIVEN else None)
        cg.solve(S.TOL)  # the solver is built here, after the call
        np.testing.assert_array_equal(cg.extract(), want.x)
        assert (cg.iterations, cg.final_rxr, cg.final_rz) == (want.bodies, want.rr[-1],
                                                             want.rz[-1])
        cg.setPreconditioner(P.Jacobi)  # on the live solver: replaces the block one
        cg.setInital(np.zeros(len(b)))
        cg.solve(S.TOL)
        assert cg.iterations > want.bodies
        cg.setBlockPreconditioner(kind, bs, W if kind == S.GIVEN else None)
        cg.setInital(np.zeros(len(b)))
        cg.solve(S.TOL)
        np.testing.assert_array_equal(cg.extract(), want.x)
        assert cg.iterations == want.bodies


def test_cpp_block_preconditioners(tmp_path):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)
    rp, cl, vl, b, bs, kind, W = S.build("nm1035-j3")
    n = len(b)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([n, len(vl), bs], np.int64).tofile(f)
        rp.astype(np.int32).tofile(f)
        cl.astype(np.int32).tofile(f)
        vl.astype(np.float64).tofile(f)
        b.tofile(f)
        W.tofile(f)
        np.array([S.TOL], np.float64).tofile(f)
    p = subprocess.run([EXE, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    runs = np.fromfile(out, np.float64).reshape(3, 2 + n)
    want = S.model_run("nm1035-j3")
    for run in runs[:2]:  # block-Jacobi, and its W moved in as Given: the same bits
        assert (int(run[0]), run[1]) == (want.bodies, want.rr[-1])
        np.testing.assert_array_equal(run[2:], want.x)
    assert int(runs[2][0]) >= 3 * want.bodies  # Jacobi after the switch back
