"""Multi-shift CG (cgx_cg_solve_shifted): (A + sigma_s I) x_s = b
for up to 8 shifts from one Krylov space.

Expected values are never the shifted solve itself: the single mode-1 solve
through the C ABI (the sigma = 0 anchor, bit for bit), the numpy model
tests/shift_model.py (every x_s, body count, code, residual and zeta equal to
one of its trajectories, bit for bit), and scipy's sparse direct solve.

Matrix and right-hand side: irregular_spd(4097, hub=300, seed=3) with variant
13 forced (17+ row blocks, an odd n, so column 1 of X at ldx = n is not
16-byte aligned and takes the 8-byte accesses, and the last row goes through
the odd-n tail), b = default_rng(21).standard_normal(n). Under tol = 1e-6 the
shifts 0, 1e-3, 0.05, 1, 30 freeze after 185 / 184 / 138 / 49 / 12 bodies in
the model; shift counts 1, 3, 5 and 8 take the three instantiated widths
(2, 4, 8 shifts per thread).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests import shift_model
from tests.test_gpu_batch import SENTINEL, Solver, columns, device_matrix, host_matrix

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "shift_check")
EINVAL, ESTATE, EUNSUPPORTED = 1, 4, 6
SIGMAS = (0.0, 1e-3, 0.05, 1.0, 30.0)
MODEL_BODIES = [185, 184, 138, 49, 12]  # tests/shift_model.py at tol 1e-6


def rhs(n):
    return np.random.default_rng(21).standard_normal(n)


def matrix_of(name):
    if name == "even":
        from tests.util import irregular_spd
        return irregular_spd(6001 + 1, seed=9)
    if name == "p3d":
        return None
    return host_matrix(name)


_even = {}


def dev(queue, name, variant=0):
    if name == "even":
        if "m" not in _even:
            rp, cl, vl = matrix_of("even")
            _even["m"] = cga.Matrix(queue, vl, cl, rp)
        return _even["m"]
    return device_matrix(queue, name, variant)


def shifted_rc(s, b, sigmas, tol=0.0, max_iter=-1, ld=None, ldarg=None, k=None, offset=0):
    """The return code of cgx_cg_solve_shifted on Solver s and its outputs:
    (X, bodies, res, codes, zeta, gaps). X is uploaded as SENTINEL."""
    n, kk = s.n, len(sigmas)
    ld = n if ld is None else ld
    db = cga.DeviceArray(s.queue, n, np.float64).upload(np.asarray(b, np.float64))
    dX = cga.DeviceArray(s.queue, kk * ld, np.float64).upload(np.full(kk * ld, SENTINEL))
    k = kk if k is None else k
    sg = (C.c_double * 8)(*list(sigmas))
    bodies, res, codes = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_int * 8)()
    rc = lib().cgx_cg_solve_shifted(s.h, k, sg, db.ptr, dX.ptr, ld if ldarg is None else ldarg,
                                    tol, max_iter, bodies, res, codes)
    if rc:
        return rc, None
    zeta = (C.c_double * 8)()
    check(lib().cgx_cg_shifted_zeta(s.h, zeta))
    host = dX.download().reshape(kk, ld)
    return 0, (np.ascontiguousarray(host[:, :n].T), list(bodies[:kk]), np.array(res[:kk]),
               list(codes[:kk]), np.array(zeta[:kk]), host[:, n:])


def shifted(s, b, sigmas, **kw):
    rc, out = shifted_rc(s, b, sigmas, **kw)
    assert rc == 0, lib().cgx_last_error()
    return out


@functools.lru_cache(maxsize=None)
def model(name, sigmas, tol, max_iter, nan_at=-1):
    """Every trajectory of the model on matrix `name` (computed once)."""
    rp, cl, vl = matrix_of(name)
    b = rhs(len(rp) - 1)
    if nan_at >= 0:
        b[nan_at] = np.nan
    tr = shift_model.trajectories(rp, cl, vl, b, list(sigmas), tol, max_iter)
    assert 1 <= len(tr) <= 2 ** shift_model.MAX_UNCLEAR
    return tr


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def same(a, b):
    """Bit for bit; a NaN equals a NaN whatever its sign and payload (which
    NaN an invalid operation such as 0 / 0 yields differs between the device
    and numpy: dense n = 1, whose second body divides 0 by 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) \
        and np.array_equal(bits(a[~na]), bits(b[~nb]))


def equals_run(out, run):
    X, bodies, res, codes, zeta = out[:5]
    return (bodies == list(run.bodies) and codes == list(run.codes)
            and same(zeta, run.zeta) and same(res, run.res) and same(X, run.X))


def assert_is_a_trajectory(out, tr):
    if any(equals_run(out, run) for _, run in tr):
        return
    run = tr[0][1]  # say where the first one differs
    X, bodies, res, codes, zeta = out[:5]
    assert bodies == list(run.bodies), f"bodies {bodies} != {run.bodies}"
    assert codes == list(run.codes), f"codes {codes} != {run.codes}"
    np.testing.assert_array_equal(zeta, np.array(run.zeta), err_msg="zeta")
    np.testing.assert_array_equal(res, np.array(run.res), err_msg="res")
    for c in range(X.shape[1]):
        np.testing.assert_array_equal(X[:, c], run.X[:, c], err_msg=f"x of shift {c}")
    raise AssertionError("no trajectory of the model equals the engine")


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("irr", 13), ("c16", 133), ("hub", 13), ("p3d", 0)])
def test_sigma_zero_is_the_single_solve(queue, name, variant):
    m = dev(queue, name, variant)
    b = rhs(m.N())
    with Solver(queue, m) as one, Solver(queue, m) as s:
        for tol, cap in ((0.0, 40), (1e-6, -1)):
            xr, kr, _, sr = one.single(b, None, tol, cap)
            for sig, c in (([0.0], 0), ([0.05, 0.0, 1.0], 1)):
                X, bodies, res, codes, zeta, _ = shifted(s, b, sig, tol=tol, max_iter=cap)
                np.testing.assert_array_equal(X[:, c], xr, err_msg=f"{name} tol {tol} {sig}")
                assert (bodies[c], codes[c]) == (kr, sr)
                assert zeta[c] == 1.0
                assert np.isfinite(X).all()
                if len(sig) == 3:  # larger shifts converge no later
                    assert bodies[2] <= bodies[0] <= bodies[1]


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol,cap", [(0.0, 40), (1e-6, -1)])
def test_model_identity(queue, tol, cap):
    m = dev(queue, "irr", 13)
    tr = model("irr", SIGMAS, tol, cap)
    with Solver(queue, m) as s:
        out = shifted(s, rhs(m.N()), SIGMAS, tol=tol, max_iter=cap)
    print("bodies", out[1], "codes", out[3], "zeta", out[4], "res", out[2])
    assert_is_a_trajectory(out, tr)
    if tol:
        assert out[1] == MODEL_BODIES and out[3] == [1] * 5
        assert len(set(out[1])) == 5
    else:
        assert out[1] == [40] * 5 and out[3] == [2] * 5


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
def test_every_shift_count(queue, k):
    """1..8 shifts run the kernels built for 2, 4 and 8; duplicates allowed."""
    sig = (0.0, 0.05, 0.05, 1.0, 1e-3, 30.0, 2.0, 0.0)[:k]
    m = dev(queue, "irr", 13)
    with Solver(queue, m) as s:
        out = shifted(s, rhs(m.N()), sig, tol=0.0, max_iter=21)
    assert_is_a_trajectory(out, model("irr", sig, 0.0, 21))
    if k >= 3:
        np.testing.assert_array_equal(out[0][:, 1], out[0][:, 2])


# 3 ---------------------------------------------------------------------------
def test_frozen_shifts_stay_put(queue):
    m = dev(queue, "irr", 13)
    b = rhs(m.N())
    cap = MODEL_BODIES[4]
    with Solver(queue, m) as s:
        full = shifted(s, b, SIGMAS, tol=1e-6)
        short = shifted(s, b, SIGMAS, tol=1e-6, max_iter=cap)
    assert short[1] == [cap] * 5 and short[3] == [2, 2, 2, 2, 1]
    assert full[1][4] == cap and full[3][4] == 1
    np.testing.assert_array_equal(full[0][:, 4], short[0][:, 4])
    assert full[2][4] == short[2][4] and full[4][4] == short[4][4]
    assert_is_a_trajectory(short, model("irr", SIGMAS, 1e-6, cap))


# 4 ---------------------------------------------------------------------------
def test_underflow_freeze(queue):
    sig = (0.0, 1e3, 1e5)
    m = dev(queue, "irr", 13)
    with Solver(queue, m) as s:
        out = shifted(s, rhs(m.N()), sig, tol=0.0, max_iter=60)
    tr = model("irr", sig, 0.0, 60)
    print("bodies", out[1], "codes", out[3], "zeta", out[4])
    assert_is_a_trajectory(out, tr)
    assert np.isfinite(out[0]).all()
    assert out[3] == [2, 2, 1] and out[1][:2] == [60, 60] and out[1][2] < 60
    assert not abs(out[4][2]) >= shift_model.DBL_MIN


# 5 ---------------------------------------------------------------------------
def test_independent_correctness(queue):
    """Against scipy's sparse direct solve of A + sigma I: the error of x_s is
    within 10 times the error of the single cgx_cg_solve on the explicitly
    shifted matrix at the same tol (the margin covers the two solves stopping
    at different bodies under the same residual rule)."""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl

    rp, cl, vl = host_matrix("irr")
    n = len(rp) - 1
    b = rhs(n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    diag = np.nonzero(rows == cl)[0]
    assert len(diag) == n
    with Solver(queue, dev(queue, "irr", 13)) as s:
        X = shifted(s, b, SIGMAS, tol=1e-6)[0]
    for c, sg in enumerate(SIGMAS):
        vs = vl.copy()
        vs[diag] += sg
        xstar = spl.spsolve(sp.csr_matrix((vs, cl, rp), shape=(n, n)).tocsc(), b)
        ms = cga.Matrix(queue, vs, cl, rp)
        with Solver(queue, ms) as one:
            xr = one.single(b, None, 1e-6, -1)[0]
        e = np.linalg.norm(X[:, c] - xstar) / np.linalg.norm(xstar)
        e_ref = np.linalg.norm(xr - xstar) / np.linalg.norm(xstar)
        print(f"sigma {sg}: e {e:.3e} e_ref {e_ref:.3e} ratio {e / e_ref:.3f}")
        assert e <= 10 * e_ref, (sg, e, e_ref)


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257])
def test_tiny_systems(queue, n):
    name = f"dense{n}"
    sig = (0.0, 0.5, 7.0)
    with Solver(queue, dev(queue, name)) as s:
        out = shifted(s, rhs(n), sig, tol=1e-10)
    assert_is_a_trajectory(out, model(name, sig, 1e-10, -1))
    assert out[3] == [1, 1, 1]


# 7 ---------------------------------------------------------------------------
def test_leading_dimension(queue):
    m = dev(queue, "irr", 13)
    n = m.N()
    tr = model("irr", SIGMAS, 0.0, 40)
    with Solver(queue, m) as s:
        out = shifted(s, rhs(n), SIGMAS, tol=0.0, max_iter=40, ld=n + 3)
    assert_is_a_trajectory(out, tr)
    assert out[5].shape == (5, 3) and np.all(out[5] == SENTINEL)
    # an even n with ldx = n + 1: every odd column is not 16-byte aligned
    me = dev(queue, "even")
    ne = me.N()
    assert ne % 2 == 0
    sig = (0.05, 0.0, 1.0, 30.0)
    with Solver(queue, me) as s:
        out = shifted(s, rhs(ne), sig, tol=0.0, max_iter=25, ld=ne + 1)
    assert_is_a_trajectory(out, model("even", sig, 0.0, 25))
    assert out[5].shape == (4, 1) and np.all(out[5] == SENTINEL)


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("poll_every,use_graph", [(1, 1), (5, 1), (32, 1), (1, 0), (5, 0), (32, 0)])
def test_chunking(queue, poll_every, use_graph):
    m = dev(queue, "irr", 13)
    b = rhs(m.N())
    with Solver(queue, m) as plain:
        want40 = shifted(plain, b, SIGMAS, tol=0.0, max_iter=40)
    assert_is_a_trajectory(want40, model("irr", SIGMAS, 0.0, 40))
    with Solver(queue, m, poll_every=poll_every, use_graph=use_graph) as s:
        for cap in (40, 41, 42, 43):  # runs that end in every slot
            out = shifted(s, b, SIGMAS, tol=0.0, max_iter=cap)
            assert out[1] == [cap] * 5
            assert_is_a_trajectory(out, model("irr", SIGMAS, 0.0, cap))
            if cap == 40:
                for a, w in zip(out[:5], want40[:5]):
                    np.testing.assert_array_equal(np.asarray(a), np.asarray(w))


# 9 ---------------------------------------------------------------------------
def test_nan_ends_every_shift(queue):
    m = dev(queue, "irr", 13)
    b = rhs(m.N())
    b[100] = np.nan
    with Solver(queue, m) as s:
        _, kr, _, sr = s.single(b, None, 1e-6, -1)
        out = shifted(s, b, (0.0, 0.05, 1.0), tol=1e-6)
    assert sr == 1 and kr <= 3
    assert out[1] == [kr] * 3 and out[3] == [1, 1, 1]


# 10 --------------------------------------------------------------------------
def test_state_interleaves_with_single_and_batch(queue):
    m = dev(queue, "irr", 13)
    n = m.N()
    b = rhs(n)
    B = columns(n, 3)
    with Solver(queue, m) as s:
        one0 = s.single(b, None, 0.0, 40)
        bat0 = s.batch(B, tol=0.0, max_iter=40, form=1)
        sh0 = shifted(s, b, SIGMAS, tol=0.0, max_iter=40)
        one1 = s.single(b, None, 0.0, 40)  # a single solve after a shifted one
        sh1 = shifted(s, b, SIGMAS, tol=0.0, max_iter=40)
        bat1 = s.batch(B, tol=0.0, max_iter=40, form=1)  # a batch after a shifted one
        sh2 = shifted(s, b, SIGMAS[:3], tol=0.0, max_iter=40)  # another shift count
        np.testing.assert_array_equal(one0[0], one1[0])
        assert one0[1:] == one1[1:]
        for a, w in zip(bat0[:4], bat1[:4]):
            np.testing.assert_array_equal(a, w)
        for other in (sh1,):
            for a, w in zip(sh0[:5], other[:5]):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(w))
        np.testing.assert_array_equal(sh2[0], sh0[0][:, :3])
        np.testing.assert_array_equal(sh0[0][:, 0], one0[0])
        # the shifted call ended the single solve: cgx_cg_run needs a new begin
        s.single(b, None, 0.0, 3)
        shifted(s, b, [0.5], tol=0.0, max_iter=3)
        total, stopped = C.c_int64(), C.c_int()
        assert lib().cgx_cg_run(s.h, 1, C.byref(total), C.byref(stopped)) == ESTATE
        # ... and the batch in progress
        dB, dX = s.upload(B[:, :2], n), s.upload(np.zeros((n, 2)), n)
        check(lib().cgx_cg_begin_batch(s.h, 2, dB.ptr, n, dX.ptr, n, 0.0, 40))
        shifted(s, b, [0.5], tol=0.0, max_iter=3)
        tot = (C.c_int64 * 8)()
        assert lib().cgx_cg_run_batch(s.h, 1, tot, C.byref(stopped)) != 0


def test_refusals(queue):
    m = dev(queue, "irr", 13)
    n = m.N()
    b = rhs(n)
    with Solver(queue, m) as s:
        zeta = (C.c_double * 8)()
        assert lib().cgx_cg_shifted_zeta(s.h, zeta) == ESTATE  # before any shifted solve
        assert shifted_rc(s, b, [0.5], k=0)[0] == EINVAL
        assert shifted_rc(s, b, [0.5] * 8, k=9)[0] == EINVAL
        assert shifted_rc(s, b, [0.5, 1.0], ldarg=n - 1)[0] == EINVAL
        for bad in (-1e-300, np.nan, np.inf, -np.inf):
            assert shifted_rc(s, b, [0.5, bad])[0] == EINVAL
            assert b"finite and not negative" in lib().cgx_last_error()
        sg = (C.c_double * 8)(0.5)
        db = cga.DeviceArray(queue, n, np.float64).upload(b)
        dX = cga.DeviceArray(queue, n, np.float64)
        bo, ro = (C.c_int64 * 8)(), (C.c_double * 8)()
        L = lib()
        assert L.cgx_cg_solve_shifted(s.h, 1, None, db.ptr, dX.ptr, n, 0.0, 5, bo, ro, None) == EINVAL
        assert L.cgx_cg_solve_shifted(s.h, 1, sg, None, dX.ptr, n, 0.0, 5, bo, ro, None) == EINVAL
        assert L.cgx_cg_solve_shifted(s.h, 1, sg, db.ptr, None, n, 0.0, 5, bo, ro, None) == EINVAL
        assert L.cgx_cg_solve_shifted(s.h, 1, sg, db.ptr, dX.ptr, n, 0.0, 5, None, ro, None) == EINVAL
        assert L.cgx_cg_solve_shifted(s.h, 1, sg, db.ptr, dX.ptr, n, 0.0, 5, bo, None, None) == EINVAL
        # stopped_out may be NULL
        assert L.cgx_cg_solve_shifted(s.h, 1, sg, db.ptr, dX.ptr, n, 0.0, 5, bo, ro, None) == 0
        assert bo[0] == 5
        # a preconditioner of either family
        check(L.cgx_cg_set_precond(s.h, 1, None))  # Jacobi
        assert shifted_rc(s, b, [0.5])[0] == EUNSUPPORTED
        assert b"preconditioner" in L.cgx_last_error()
        check(L.cgx_cg_set_precond(s.h, 0, None))
        check(L.cgx_cg_set_block_precond(s.h, 1, 4, None))  # block-Jacobi
        assert shifted_rc(s, b, [0.5])[0] == EUNSUPPORTED
        assert b"preconditioner" in L.cgx_last_error()
        check(L.cgx_cg_set_block_precond(s.h, 0, 0, None))
        # the solver's mode does not matter
        want = shifted(s, b, SIGMAS[:3], tol=0.0, max_iter=20)
    for mode in (0, 3):
        with Solver(queue, m, mode=mode) as s:
            out = shifted(s, b, SIGMAS[:3], tol=0.0, max_iter=20)
            for a, w in zip(out[:5], want[:5]):
                np.testing.assert_array_equal(np.asarray(a), np.asarray(w))
    m32 = cga.Matrix(queue, *[host_matrix("irr")[i] for i in (2, 1, 0)], dtype=np.float32)
    with Solver(queue, m32, dtype=np.float32) as s:
        assert shifted_rc(s, b, [0.5])[0] == EUNSUPPORTED
        assert b"f32" in lib().cgx_last_error()


def test_partitioned_matrix_is_refused():
    """A one-rank world over the host transport (callbacks that copy): the
    matrix is partitioned, and the shifted solve says so."""
    from conjugategradient_amd.hostcomm import AG, AR, EX

    L = lib()
    q = cga.Queue(0)
    cbs = (AG(lambda user, send, nbytes, recv: C.memmove(recv, send, nbytes) and 0),
           AR(lambda user, vals, count: 0),
           EX(lambda user, n, peers, send, sbytes, recv, rbytes: 0))
    try:
        check(L.cgx_dist_init_host(q.handle, 0, 1, *[C.cast(f, C.c_void_p) for f in cbs], None))
        rp, cl, vl = host_matrix("dense63")
        n = 63
        rows = cga.DeviceArray(q, n + 1, np.int32).upload(rp.astype(np.int32))
        cols = cga.DeviceArray(q, len(cl), np.int32).upload(cl.astype(np.int32))
        vals = cga.DeviceArray(q, len(vl), np.float64).upload(vl)
        A = C.c_void_p()
        check(L.cgx_csr_create_dist(q.handle, n, 0, n, len(vl), rows.ptr, cols.ptr, vals.ptr, 0,
                                    C.byref(A)))
        cg = C.c_void_p()
        check(L.cgx_cg_create(q.handle, A, C.byref(cg)))
        db = cga.DeviceArray(q, n, np.float64).upload(rhs(n))
        dX = cga.DeviceArray(q, n, np.float64)
        sg = (C.c_double * 8)(0.5)
        bo, ro = (C.c_int64 * 8)(), (C.c_double * 8)()
        assert L.cgx_cg_solve_shifted(cg, 1, sg, db.ptr, dX.ptr, n, 0.0, 5, bo, ro, None) \
            == EUNSUPPORTED
        assert b"partitioned" in L.cgx_last_error()
        L.cgx_cg_destroy(cg)
        L.cgx_csr_destroy(A)
    finally:
        q.close()


# 11 --------------------------------------------------------------------------
def test_python_layer(queue, monkeypatch):
    monkeypatch.setenv("CGX_SPMV_VARIANT", "13")
    rp, cl, vl = host_matrix("irr")
    n = len(rp) - 1
    b = rhs(n)
    with Solver(queue, dev(queue, "irr", 13)) as s:
        want = shifted(s, b, SIGMAS, tol=1e-6)
    cg = cga.CG(queue)
    cg.setMatrix(vl, cl, rp)
    cg.setTarget(b)
    X = cg.solve_shifted(SIGMAS, improvement=1e-6)
    assert X.shape == (n, 5)
    np.testing.assert_array_equal(X, want[0])
    assert list(cg.iterations_shifted) == want[1] and list(cg.stopped_shifted) == want[3]
    np.testing.assert_array_equal(cg.residual_shifted, want[2])
    X = cg.solve_shifted([0.05], max_iter=10)
    with Solver(queue, dev(queue, "irr", 13)) as s:
        np.testing.assert_array_equal(X, shifted(s, b, [0.05], tol=0.0, max_iter=10)[0])
    assert list(cg.iterations_shifted) == [10]
    for bad in ([], [0.1] * 9, [-1.0], [np.nan]):
        with pytest.raises(ValueError):
            cg.solve_shifted(bad)


def test_cpp_layer(queue, tmp_path):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)
    rp, cl, vl = host_matrix("irr")
    n, k = len(rp) - 1, len(SIGMAS)
    b = rhs(n)
    # the C++ layer's matrix keeps its production variant: the ABI run too
    with Solver(queue, dev(queue, "irr", 0)) as s:
        want = shifted(s, b, SIGMAS, tol=1e-6)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([n, len(vl), k, -1], np.int64).tofile(f)
        rp.astype(np.int32).tofile(f)
        cl.astype(np.int32).tofile(f)
        vl.astype(np.float64).tofile(f)
        b.tofile(f)
        np.array(SIGMAS, np.float64).tofile(f)
        np.array([1e-6], np.float64).tofile(f)
    p = subprocess.run([EXE, str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.fromfile(out, np.float64).reshape(k, 3 + n)
    for c in range(k):
        assert (int(res[c, 0]), res[c, 1], int(res[c, 2])) == (want[1][c], want[2][c], want[3][c])
        np.testing.assert_array_equal(res[c, 3:], want[0][:, c])
