"""Diagonal preconditioning on the device (cgx_cg_set_precond):
the preconditioned update kernels of modes 1 and 3 (k_update_r_pc,
k_update_xp_pc, k_update_p_defer_pc, k_pc_init) and the diagonal extraction
(k_diag_inv), against the numpy PCG of tests/test_pcg_cpu.py on the scaled
matrices plain CG does not solve. The engine's double-length dots lie between
the checker's np.dot and fsum variants, which differ by < 1e-15 after 30
bodies (test_pcg_cpu.py), so x is held to 1e-13 there."""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests.test_pcg_cpu import CASES, case, diag_of, jacobi_ref, pcg, residual
from tests.util import irregular_spd, rel

pytestmark = pytest.mark.gpu

P = cga.Preconditioner
EINVAL, ESTATE, EUNSUPPORTED = 1, 4, 6


def _matrix(queue, name, dtype=np.float64):
    rp, cl, vl, _ = case(name)
    return cga.Matrix(queue, vl, cl, rp, dtype=dtype)


def _cg(queue, m, b, mode, kind=P.None_, diag=None, dtype=np.float64, poll=32, graph=True):
    cg = cga.CG(queue, dtype)
    cg.mode = mode
    cg.poll_every = poll
    cg.use_graph = graph
    cg.setMatrix(m)
    cg.setTarget(b)
    cg.setPreconditioner(kind, diag)
    return cg


def _run(cg, tol, max_iter=-1, x0=None, in_place=False):
    if in_place and cg.x.ptr() is not None:  # the same x: captured graphs stay valid
        cg.x.data().fill(0.0)
    else:
        cg.setInital(np.zeros(cg.getDimension()) if x0 is None else x0)
    cg.solve(tol, max_iter=max_iter)
    return cg.extract(), cg.iterations, cg.final_rxr, cg.final_rz


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1:] == b[1:], (a[1:], b[1:])


def _mode(cg):
    v = C.c_int(-1)
    check(lib().cgx_cg_get_mode(cg._solver(), C.byref(v)))
    return v.value


# 1 -------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("p2d", None), ("irr", None), ("p3d", None),
                                          ("p3d", 13)],
                         ids=["p2d", "irr", "p3d", "p3d-csr-stream"])
def test_jacobi_30_bodies_against_checker(queue, monkeypatch, name, variant):
    if variant is not None:
        monkeypatch.setenv("CGX_SPMV_VARIANT", str(variant))
    m = _matrix(queue, name)
    b = case(name)[3]
    xr, kr, rr, rz = jacobi_ref(name, 0.0, 30)
    out = {mode: _run(_cg(queue, m, b, mode, P.Jacobi), 0.0, 30) for mode in (1, 3)}
    for mode, (x, k, rxr, rzz) in out.items():
        d = rel(x, xr)
        print(f"{name} mode {mode}: rel {d:.3e}, r.r {rxr:.17g} (checker {rr:.17g}), "
              f"r.z {rzz:.17g} (checker {rz:.17g})")
        assert k == kr == 30
        assert d <= 1e-13
        assert rxr == pytest.approx(rr, rel=1e-9) and rzz == pytest.approx(rz, rel=1e-9)
    _same(out[3], out[1])


# 2 -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["p2d", "irr"])
def test_jacobi_converges_where_plain_cg_hits_the_cap(queue, name):
    m = _matrix(queue, name)
    b = case(name)[3]
    n = len(b)
    tol = 1e-8 * float(np.linalg.norm(b))
    xr, kr, _, _ = jacobi_ref(name, 1e-8, -1)
    assert kr == CASES[name]
    cg = _cg(queue, m, b, 0, P.Jacobi)
    assert _mode(cg) == 3
    first = _run(cg, tol)
    x, k = first[:2]
    print(f"{name}: Jacobi {k} bodies (checker {kr}), rel {rel(x, xr):.3e}, "
          f"residual {residual(name, x):.3e}")
    assert abs(k - kr) <= 2
    assert rel(x, xr) <= 1e-10
    assert residual(name, x) <= 2e-8
    # the same solver without the preconditioner: the reason the feature exists
    cg.setPreconditioner(P.None_)
    x0, k0, _, rz0 = _run(cg, tol, in_place=True)
    print(f"{name}: plain {k0} bodies, residual {residual(name, x0):.3e}")
    assert k0 == n + 1
    assert residual(name, x0) > 1e-4
    assert np.isnan(rz0)
    # ... and back: the graphs captured for the plain bodies are gone
    cg.setPreconditioner(P.Jacobi)
    _same(_run(cg, tol, in_place=True), first)


# 3 -------------------------------------------------------------------------
IDENTITY = [("3d-rule", (3, 20, 18, 17), None), ("2d-rule", (2, 70, 66, 1), None),
            ("3d-lean", (3, 128, 48, 40), "33554432:0"), ("irr", None, None)]


@pytest.mark.parametrize("name,dims,variant", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_unit_diagonal_is_the_plain_solver_bit_for_bit(queue, monkeypatch, name, dims, variant):
    if variant is not None:
        monkeypatch.setenv("CGX_SPMV_VARIANT", variant)
    if dims is None:
        rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
        m = cga.Matrix(queue, vl, cl, rp)
    else:
        m = cga.Matrix.poisson(queue, *dims)
    if name == "3d-lean":
        v = C.c_int(0)
        check(lib().cgx_csr_variant(m.schedule(), C.byref(v)))
        assert v.value & 33554432
    n = m.N()
    b = np.arange(1, n + 1, dtype=np.float64)
    for mode in (1, 3):
        x0, k0, r0, _ = _run(_cg(queue, m, b, mode), 0.0, 45)
        x1, k1, r1, z1 = _run(_cg(queue, m, b, mode, P.Diagonal, np.ones(n)), 0.0, 45)
        assert k0 == k1 == 45
        np.testing.assert_array_equal(x1, x0)
        assert r1 == r0 and z1 == r1


# 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("bodies", [29, 30, 31, 32])
def test_deferred_x_group_boundaries(queue, bodies):
    m = _matrix(queue, "p2d")
    b = case("p2d")[3]
    one = _run(_cg(queue, m, b, 1, P.Jacobi), 0.0, bodies)
    assert one[1] == bodies
    _same(_run(_cg(queue, m, b, 3, P.Jacobi), 0.0, bodies), one)


def test_poll_interval_graph_and_warm_start(queue):
    m = _matrix(queue, "p2d")
    rp, cl, vl, b = case("p2d")
    ref = _run(_cg(queue, m, b, 3, P.Jacobi), 0.0, 30)
    for graph in (True, False):
        _same(_run(_cg(queue, m, b, 3, P.Jacobi, poll=5, graph=graph), 0.0, 30), ref)
    x0 = 0.5 * jacobi_ref("p2d", 1e-8, -1)[0]
    xr, kr, _, _ = pcg(rp, cl, vl, b, 1.0 / diag_of(rp, cl, vl), 0.0, True, 30, x0)
    out = {mode: _run(_cg(queue, m, b, mode, P.Jacobi), 0.0, 30, x0) for mode in (1, 3)}
    for mode, (x, k, _, _) in out.items():
        print(f"warm start, mode {mode}: rel {rel(x, xr):.3e}")
        assert k == kr == 30 and rel(x, xr) <= 1e-13
    _same(out[3], out[1])


@pytest.mark.parametrize("name", ["p2d", "p3d"])
def test_non_temporal_loads_of_m_give_the_same_bits(queue, monkeypatch, name):
    """$CGX_PCG_M_NT=1 (read by cgx_cg_set_precond) only changes how m is loaded."""
    m = _matrix(queue, name)
    b = case(name)[3]
    for mode in (1, 3):
        monkeypatch.delenv("CGX_PCG_M_NT", raising=False)
        ref = _run(_cg(queue, m, b, mode, P.Jacobi), 0.0, 31)
        monkeypatch.setenv("CGX_PCG_M_NT", "1")
        _same(_run(_cg(queue, m, b, mode, P.Jacobi), 0.0, 31), ref)


# 5 -------------------------------------------------------------------------
def _tridiag5():
    d = np.array([1.0, 10.0, 100.0, 1e3, 1e4])
    o = -0.3 * np.sqrt(d[:-1] * d[1:])  # D^-1/2 A D^-1/2 = tridiag(-0.3, 1, -0.3): SPD
    return np.diag(d) + np.diag(o, 1) + np.diag(o, -1)


@pytest.mark.parametrize("dense", [np.array([[4.0]]), np.array([[4.0, 1.0], [1.0, 3.0]]),
                                   _tridiag5()], ids=["n1", "n2", "n5"])
@pytest.mark.parametrize("mode", [1, 3])
def test_tiny_systems(queue, dense, mode):
    """The exact solution within n + 1 bodies. The body count is capped from
    outside: once r is exactly 0 (n = 1 after one body) the next body divides
    0 by 0, as the plain solver and the reference do (Q5)."""
    n = len(dense)
    r, c = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    m = cga.Matrix(queue, dense[r, c], c.astype(np.int32), rp)
    b = np.arange(1, n + 1, dtype=np.float64)
    want = np.linalg.solve(dense, b)
    np.testing.assert_array_equal(m.diag_inv(), 1.0 / np.diag(dense))
    errs = []
    for bodies in range(1, n + 2):
        x, k, _, _ = _run(_cg(queue, m, b, mode, P.Jacobi), 0.0, bodies)
        assert k == bodies
        errs.append(rel(x, want))
        if errs[-1] <= 1e-12:
            break
    print(f"n = {n} mode {mode}: rel by bodies {errs}")
    assert errs[-1] <= 1e-12


# 6 -------------------------------------------------------------------------
def test_callers_diagonal_gives_jacobis_bits(queue):
    m = _matrix(queue, "p2d")
    rp, cl, vl, b = case("p2d")
    minv = 1.0 / diag_of(rp, cl, vl)
    for mode in (1, 3):
        jac = _run(_cg(queue, m, b, mode, P.Jacobi), 0.0, 30)
        _same(_run(_cg(queue, m, b, mode, P.Diagonal, minv), 0.0, 30), jac)
        # a device Vector the caller built
        v = cga.Vector(queue, minv)
        _same(_run(_cg(queue, m, b, mode, P.Diagonal, v), 0.0, 30), jac)


def _shuffled_with_split_diagonal():
    """poisson 5 x 4 with every row's entries reversed and its diagonal entry
    split in two (1.5 first in the row, the rest last): unsorted, duplicated."""
    from oracle import oracle as O
    rp, cl, vl = (np.asarray(a) for a in O.poisson(2, 5, 4, 1))
    rows, cols, vals = [], [], []
    for i in range(len(rp) - 1):
        c, v = cl[rp[i]:rp[i + 1]][::-1], vl[rp[i]:rp[i + 1]][::-1].astype(np.float64)
        k = int(np.nonzero(c == i)[0][0])
        rest = v[k] * (1.0 + 0.1 * i) - 1.5  # diagonals differ row to row
        c = np.concatenate([[i], np.delete(c, k), [i]])
        v = np.concatenate([[1.5], np.delete(v, k), [rest]])
        rows.append(len(c))
        cols.append(c)
        vals.append(v)
    rp2 = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return rp2, np.concatenate(cols).astype(np.int32), np.concatenate(vals)


def test_diag_inv_is_numpys_bit_for_bit(queue):
    for name in CASES:
        rp, cl, vl, _ = case(name)
        np.testing.assert_array_equal(_matrix(queue, name).diag_inv(),
                                      1.0 / diag_of(rp, cl, vl))
    rp, cl, vl = _shuffled_with_split_diagonal()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    on = rows == cl
    assert (np.bincount(rows[on], minlength=n) == 2).all() and (np.diff(cl[:3]) < 0).any()
    np.testing.assert_array_equal(cga.Matrix(queue, vl, cl, rp).diag_inv(),
                                  1.0 / diag_of(rp, cl, vl))
    f = cga.Matrix(queue, vl, cl, rp, dtype=np.float32).diag_inv()
    d32 = np.zeros(n, np.float32)
    np.add.at(d32, rows[on], vl.astype(np.float32)[on])  # f32 sums, entry order
    assert f.dtype == np.float32
    np.testing.assert_array_equal(f, np.float32(1) / d32)


# 7 -------------------------------------------------------------------------
def _raw_solver(queue, m):
    h = C.c_void_p()
    check(lib().cgx_cg_create(queue.handle, m.schedule(), C.byref(h)))
    return h


@pytest.mark.parametrize("how", ["zero", "missing"])
def test_bad_diagonal_is_einval_naming_the_row(queue, how):
    from oracle import oracle as O
    rp, cl, vl = (np.array(a) for a in O.poisson(2, 6, 5, 1))
    k = rp[7] + int(np.nonzero(cl[rp[7]:rp[8]] == 7)[0][0])
    if how == "zero":
        vl[k] = 0.0
    else:
        cl, vl = np.delete(cl, k), np.delete(vl, k)
        rp = rp.copy()
        rp[8:] -= 1
    m = cga.Matrix(queue, vl, cl, rp)
    L = lib()
    out = cga.DeviceArray(queue, m.N())
    assert L.cgx_csr_diag_inv(m.schedule(), out.ptr) == EINVAL
    msg = L.cgx_last_error().decode()
    assert "row 7" in msg and "1 row" in msg, msg
    with pytest.raises(cga.CgxError, match="row 7"):
        m.diag_inv()
    h = _raw_solver(queue, m)
    try:
        assert L.cgx_cg_set_precond(h, P.Jacobi, None) == EINVAL
        assert "row 7" in L.cgx_last_error().decode()
        kind = C.c_int(-1)
        check(L.cgx_cg_get_precond(h, C.byref(kind)))
        assert kind.value == P.None_  # the solver keeps what it had
    finally:
        L.cgx_cg_destroy(h)


def test_callers_diagonal_is_checked(queue):
    m = cga.Matrix.poisson(queue, 2, 30, 30)
    n = m.N()
    L = lib()
    h = _raw_solver(queue, m)
    try:
        for bad in (-1.0, float("nan"), 0.0, float("inf")):
            v = np.ones(n)
            v[11] = bad
            d = cga.Vector(queue, v)
            assert L.cgx_cg_set_precond(h, P.Diagonal, d.ptr()) == EINVAL, bad
            assert "entry 11" in L.cgx_last_error().decode()
        assert L.cgx_cg_set_precond(h, P.Diagonal, None) == EINVAL
        assert L.cgx_cg_set_precond(h, 3, None) == EINVAL
        rz = C.c_double()
        assert L.cgx_cg_rz(h, C.byref(rz)) == ESTATE  # no preconditioner
        assert "without a preconditioner" in L.cgx_last_error().decode()
    finally:
        L.cgx_cg_destroy(h)


@pytest.mark.parametrize("mode", [2, 4, 5, 6])
def test_other_modes_refuse_a_preconditioner(queue, monkeypatch, mode):
    if mode == 6:  # needs the lean stencil walk
        monkeypatch.setenv("CGX_SPMV_VARIANT", "33554432:0")
        m = cga.Matrix.poisson(queue, 3, 128, 48, 40)
    else:
        m = cga.Matrix.poisson(queue, 2, 30, 30)
    L = lib()
    got = C.c_int(-1)
    # the mode first, then the preconditioner
    h = _raw_solver(queue, m)
    try:
        check(L.cgx_cg_set_mode(h, mode))  # the mode itself runs on this matrix
        assert L.cgx_cg_set_precond(h, P.Jacobi, None) == EUNSUPPORTED
        msg = L.cgx_last_error().decode()
        assert "modes 1 and 3" in msg, msg
        check(L.cgx_cg_get_mode(h, C.byref(got)))
        assert got.value == mode
        check(L.cgx_cg_get_precond(h, C.byref(got)))
        assert got.value == P.None_
    finally:
        L.cgx_cg_destroy(h)
    # the preconditioner first, then the mode
    h = _raw_solver(queue, m)
    try:
        check(L.cgx_cg_set_precond(h, P.Jacobi, None))
        check(L.cgx_cg_get_mode(h, C.byref(got)))
        assert got.value == 3  # auto with a preconditioner
        assert L.cgx_cg_set_mode(h, mode) == EUNSUPPORTED
        msg = L.cgx_last_error().decode()
        assert "modes 1 and 3" in msg, msg
        check(L.cgx_cg_get_mode(h, C.byref(got)))
        assert got.value == 3
        check(L.cgx_cg_set_mode(h, 1))
        check(L.cgx_cg_get_mode(h, C.byref(got)))
        assert got.value == 1
    finally:
        L.cgx_cg_destroy(h)


# 8 -------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 3])
def test_f32_jacobi(queue, mode):
    m = _matrix(queue, "p2d", np.float32)
    b = case("p2d")[3]
    n = len(b)
    tol = 1e-3 * float(np.linalg.norm(b))
    x, k, _, _ = _run(_cg(queue, m, b, mode, P.Jacobi, dtype=np.float32), tol)
    res = residual("p2d", x.astype(np.float64))
    print(f"f32 mode {mode}: Jacobi {k} bodies, f64 residual {res:.3e}")
    assert x.dtype == np.float32
    assert k < 200  # stopped by the rule, far below the cap n + 1
    assert res <= 3e-3
    x0, k0, _, _ = _run(_cg(queue, m, b, mode, dtype=np.float32), tol)
    print(f"f32 mode {mode}: plain {k0} bodies, f64 residual "
          f"{residual('p2d', x0.astype(np.float64)):.3e}")
    assert k0 == n + 1
