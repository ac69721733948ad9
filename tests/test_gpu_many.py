"""Many small systems (cgx_many_solve): one workgroup runs a
whole CG solve, init and every body, and then takes the next system.

Every expected value is a single solve in mode 1 through the C ABI (one
cgx_csr and cgx_cg per system, cgx_cg_begin / cgx_cg_run on that system's own
values, b and x0) or tests/cg_model.cg; never the kernel under test. The
comparison is bit for bit (assert_array_equal): each system keeps the single
kernels' per-element expressions and per-row sum order, and the two dots are
double-length sums whose rounded value does not depend on how rows are dealt
to threads wherever the dot is clear of a rounding boundary (cgx_dd.h), which
tests/test_many_cpu.py checks for every system used here
(tests/many_systems.py). The hub row's system is pinned to cg_model: the
single solve tree-sums a row longer than a tile, one thread here sums it in
entry order.

Sizes: n = 1, 2 (fewer rows than a wave), 63 / 64 / 65 (the last partial wave
of the 1-row-per-thread form), 255 / 256 / 257 (1 to 2 rows per thread), 1,023
(4 rows per thread, a last stride of 255) and 4,096 (16 rows per thread, the
most); 4,097 is refused. 1,025 (8 rows per thread) has a test of its own.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import F64, check, lib
from tests import cg_model
from tests import many_systems as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "many_check")
EINVAL, EUNSUPPORTED = 1, 6
SENTINEL = -7.25e11
PAD = 8  # elements in front of every device block (keeps it 8-byte aligned)


def single(queue, rp, cl, vl, b, x0, tol, max_bodies):
    """(x, bodies, rxr, stopped) of cgx_cg_begin / cgx_cg_run in mode 1 on a
    matrix of this system's own."""
    m = cga.Matrix(queue, vl, cl, rp)
    n = m.N()
    h = C.c_void_p()
    check(lib().cgx_cg_create(queue.handle, m.schedule(), C.byref(h)))
    try:
        check(lib().cgx_cg_set_mode(h, 1))
        db = cga.DeviceArray(queue, n, np.float64).upload(b)
        dx = cga.DeviceArray(queue, n, np.float64).upload(np.zeros(n) if x0 is None else x0)
        check(lib().cgx_cg_begin(h, db.ptr, dx.ptr, tol, max_bodies))
        cap = n + 1 if max_bodies < 0 else min(n + 1, max(max_bodies, 1))
        total, stopped, rxr = C.c_int64(), C.c_int(), C.c_double()
        check(lib().cgx_cg_run(h, cap, C.byref(total), C.byref(stopped)))
        check(lib().cgx_cg_rxr(h, C.byref(rxr)))
        return dx.download(), total.value, rxr.value, stopped.value
    finally:
        lib().cgx_cg_destroy(h)


_refs = {}


def references(queue, name):
    """The single solves of a set's systems, computed once and shared."""
    if name not in _refs:
        rp, cl, vals, B, tol, X0, mb = M.system_set(name)
        _refs[name] = [single(queue, rp, cl, vals[s], B[s], None if X0 is None else X0[s], tol, mb)
                       for s in range(len(vals))]
    return _refs[name]


def block(queue, rows, ld, dtype=np.float64):
    """A device block of len(rows) rows at leading dimension ld behind PAD
    sentinels, every gap a sentinel -> (array, pointer to row 0, host image)."""
    k, w = rows.shape
    host = np.full(PAD + k * ld + PAD, SENTINEL, dtype=dtype)
    body = host[PAD:PAD + k * ld].reshape(k, ld)
    body[:, :w] = rows
    d = cga.DeviceArray(queue, host.size, dtype).upload(host)
    return d, d.ptr + PAD * np.dtype(dtype).itemsize, host


class Many:
    """A cgx_many on device copies of a set, driven through the C ABI."""

    def __init__(self, queue, rp, cl, vals, ldv=None):
        self.queue = queue
        self.nsys, self.nnz = vals.shape
        self.n = len(rp) - 1
        self.ldv = self.nnz if ldv is None else ldv
        self.rp = cga.DeviceArray(queue, self.n + 1, np.int32).upload(rp)
        self.cl = cga.DeviceArray(queue, self.nnz, np.int32).upload(cl)
        self.vals, self.vptr, self.vhost = block(queue, vals, self.ldv)
        h = C.c_void_p()
        check(lib().cgx_many_create(queue.handle, F64, self.nsys, self.n, self.nnz, self.rp.ptr,
                                    self.cl.ptr, self.vptr, self.ldv, C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().cgx_many_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        wg, r, lds = C.c_int(), C.c_int(), C.c_int64()
        check(lib().cgx_many_info(self.h, C.byref(wg), C.byref(r), C.byref(lds)))
        return wg.value, r.value, lds.value

    def solve(self, B, X0=None, tol=0.0, max_bodies=-1, ld=None, max_workgroups=0):
        """-> X, bodies, rxr, stopped, and the host images before / after of B and X"""
        ld = self.n if ld is None else ld
        dB, pB, hB = block(self.queue, B, ld)
        dX, pX, hX = block(self.queue, np.zeros_like(B) if X0 is None else X0, ld)
        check(lib().cgx_many_config(self.h, max_workgroups))
        ns = self.nsys
        bodies, rxr, stopped = (C.c_int64 * ns)(), (C.c_double * ns)(), (C.c_int * ns)()
        check(lib().cgx_many_solve(self.h, pB, ld, pX, ld, tol, max_bodies, bodies, rxr, stopped))
        aX, aB = dX.download(), dB.download()
        X = aX[PAD:PAD + ns * ld].reshape(ns, ld)[:, :self.n].copy()
        return (X, np.array(bodies[:]), np.array(rxr[:]), np.array(stopped[:]),
                (hB, aB), (hX, aX))


def assert_systems_equal(out, refs, which=None):
    X, bodies, rxr, stopped = out[:4]
    for s, (xr, kr, rr, sr) in enumerate(refs):
        if which is not None and s not in which:
            continue
        np.testing.assert_array_equal(X[s], xr, err_msg=f"system {s}: x")
        np.testing.assert_array_equal(bodies[s], kr, err_msg=f"system {s}: bodies")
        np.testing.assert_array_equal(rxr[s], rr, err_msg=f"system {s}: r.r")
        np.testing.assert_array_equal(stopped[s], sr, err_msg=f"system {s}: stop code")


def test_several_systems_per_workgroup(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("multi")
    refs = references(queue, "multi")
    with Many(queue, rp, cl, vals) as m:
        three = m.solve(B, tol=tol, max_workgroups=3)  # 12 or 13 systems per workgroup
        check(lib().cgx_many_config(m.h, 3))
        assert m.info()[0] == 3
        full = m.solve(B, tol=tol)
        wg, r, lds = m.info()
        assert 3 < wg <= 37 and r == 4 and lds >= 4 * 256 * 8
    for a, b in zip(three[:4], full[:4]):
        np.testing.assert_array_equal(a, b)
    assert_systems_equal(three, refs)
    assert_systems_equal(full, refs)
    assert len(set(three[1].tolist())) >= 3, three[1]
    assert (three[3] == 1).all() and (three[1] < 1024).all()


@pytest.mark.parametrize("n", M.SIZES)
def test_sizes(queue, n):
    name = f"n{n}"
    rp, cl, vals, B, tol, _, _ = M.system_set(name)
    with Many(queue, rp, cl, vals) as m:
        out = m.solve(B, tol=tol)
        assert m.info()[1] == next(r for r in (1, 2, 4, 8, 16) if n <= 256 * r)
    assert_systems_equal(out, references(queue, name))
    assert (out[3] == 1).all()


def test_eight_rows_per_thread(queue):
    """n = 1,025: k_many_cg<8, kManyPlain>, which no size above reaches; 9
    systems, all on one workgroup."""
    rp, cl, vals, B, tol, _, _ = M.system_set("n1025x9")
    with Many(queue, rp, cl, vals) as m:
        out = m.solve(B, tol=tol, max_workgroups=1)
        assert m.info()[:2] == (1, 8)
    assert_systems_equal(out, references(queue, "n1025x9"))
    assert (out[3] == 1).all()


def test_hub_row_against_the_model(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("hub")
    with Many(queue, rp, cl, vals) as m:
        X, bodies, rxr, stopped = m.solve(B, tol=tol)[:4]
    for s in range(len(vals)):
        run = cg_model.cg(rp, cl, vals[s], B[s], tol, -1, dtype=np.float64)
        np.testing.assert_array_equal(X[s], run.x, err_msg=f"system {s}: x")
        np.testing.assert_array_equal(bodies[s], run.bodies)
        np.testing.assert_array_equal(rxr[s], run.rr[-1])
        np.testing.assert_array_equal(stopped[s], 1)


def test_empty_row(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("empty")
    with Many(queue, rp, cl, vals) as m:
        out = m.solve(B, tol=tol)
    assert_systems_equal(out, references(queue, "empty"))


def test_leading_dimensions_and_sentinels(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("n65")
    n, nnz = 65, vals.shape[1]
    with Many(queue, rp, cl, vals, ldv=nnz + 5) as m:
        out = m.solve(B, tol=tol, ld=n + 37)
        vafter = m.vals.download()
    assert_systems_equal(out, references(queue, "n65"))
    np.testing.assert_array_equal(vafter, m.vhost)          # values and their gaps: untouched
    (hB, aB), (hX, aX) = out[4], out[5]
    np.testing.assert_array_equal(aB, hB)                   # B and its gaps: untouched
    ld = n + 37
    gaps = np.ones(aX.size, bool)
    for s in range(3):
        gaps[PAD + s * ld:PAD + s * ld + n] = False
    assert gaps.sum() == 2 * PAD + 3 * 37
    np.testing.assert_array_equal(aX[gaps], np.full(gaps.sum(), SENTINEL))
    # (ld < n is refused)
    with Many(queue, rp, cl, vals) as m:
        dB, pB, _ = block(queue, B, n)
        out3 = (C.c_int64 * 3)(), (C.c_double * 3)()
        assert lib().cgx_many_solve(m.h, pB, n - 1, pB, n, 0.0, -1, *out3, None) == EINVAL
        assert b"ldb" in lib().cgx_last_error()
        assert lib().cgx_many_solve(m.h, pB, n, pB, n - 1, 0.0, -1, *out3, None) == EINVAL
        assert lib().cgx_many_solve(m.h, pB + 4, n, pB, n, 0.0, -1, *out3, None) == EINVAL
        assert b"8-byte" in lib().cgx_last_error()
        assert lib().cgx_many_solve(m.h, None, n, pB, n, 0.0, -1, *out3, None) == EINVAL
        assert lib().cgx_many_config(m.h, -1) == EINVAL


def test_nonzero_x0_and_a_cap_of_five(queue):
    rp, cl, vals, B, tol, X0, mb = M.system_set("multi5")
    with Many(queue, rp, cl, vals) as m:
        out = m.solve(B, X0=X0, tol=tol, max_bodies=mb)
    assert_systems_equal(out, references(queue, "multi5"))
    np.testing.assert_array_equal(out[1], np.full(5, 5))
    np.testing.assert_array_equal(out[3], np.full(5, 2))


def test_nan_and_inf_stay_in_their_system(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("multi")
    vals, B = vals[:8].copy(), B[:8].copy()
    refs = references(queue, "multi")[:8]
    B[2, 5] = np.nan
    vals[5, 17] = np.inf
    with Many(queue, rp, cl, vals) as m:
        out = m.solve(B, tol=tol, max_workgroups=2)  # the two share workgroups with the rest
    others = [s for s in range(8) if s not in (2, 5)]
    assert_systems_equal(out, refs, which=others)
    for s in (2, 5):
        xr, kr, rr, sr = single(queue, rp, cl, vals[s], B[s], None, tol, -1)
        assert np.isnan(rr) and sr == 1
        np.testing.assert_array_equal(out[1][s], kr)
        np.testing.assert_array_equal(out[3][s], sr)
        np.testing.assert_array_equal(out[2][s], rr)
        np.testing.assert_array_equal(out[0][s], xr)


def test_python_class_and_values_overwritten_in_place(queue):
    rp, cl, vals, B, tol, _, _ = M.system_set("n255")
    refs = references(queue, "n255")
    m = cga.ManyCG(queue, rp, cl, vals)
    try:
        X = m.solve(B, improvement=tol)
        assert X.shape == B.shape and m.info()[1] == 1
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped), refs)
        # system s now takes the values of system 2 - s: no new create
        m.set_values(vals[::-1])
        X = m.solve(B, improvement=tol)
        swapped = [single(queue, rp, cl, vals[2 - s], B[s], None, tol, -1) for s in (0, 2)]
        assert_systems_equal((X[[0, 2]], m.bodies[[0, 2]], m.rxr[[0, 2]], m.stopped[[0, 2]]),
                             swapped)
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped), refs, which=[1])
        assert not np.array_equal(X[0], refs[0][0])
    finally:
        m.close()


def test_pattern_refusals(queue):
    rp, cl, vl = M.poisson2d(5, 4)
    vals = np.tile(vl, (2, 1))

    def rc_of(rp_, cl_, n=None, nnz=None):
        d_rp = cga.DeviceArray(queue, len(rp_), np.int32).upload(rp_)
        d_cl = cga.DeviceArray(queue, len(cl_), np.int32).upload(cl_)
        d_v = cga.DeviceArray(queue, vals.size, np.float64).upload(vals.ravel())
        h = C.c_void_p()
        rc = lib().cgx_many_create(queue.handle, F64, 2, len(rp_) - 1 if n is None else n,
                                   len(cl_) if nnz is None else nnz, d_rp.ptr, d_cl.ptr, d_v.ptr,
                                   len(vl), C.byref(h))
        assert rc or h.value
        if h.value:
            lib().cgx_many_destroy(h)
        return rc, lib().cgx_last_error()

    assert rc_of(rp, cl)[0] == 0
    bad = rp.copy()
    bad[0] = 1
    rc, msg = rc_of(bad, cl)
    assert rc == EINVAL and b"rowptr" in msg
    bad = rp.copy()
    bad[-1] -= 1
    rc, msg = rc_of(bad, cl)
    assert rc == EINVAL and b"rowptr" in msg
    bad = rp.copy()
    bad[3], bad[4] = rp[4], rp[3]
    rc, msg = rc_of(bad, cl)
    assert rc == EINVAL and b"rowptr" in msg
    for v in (-1, 20):
        bad = cl.copy()
        bad[7] = v
        rc, msg = rc_of(rp, bad)
        assert rc == EINVAL and b"column" in msg
    h = C.c_void_p()
    d = cga.DeviceArray(queue, 4098, np.float64)
    rc = lib().cgx_many_create(queue.handle, F64, 1, 4097, 4097, d.ptr, d.ptr, d.ptr, 4097,
                               C.byref(h))
    assert rc == EUNSUPPORTED and b"cgx_cg_solve" in lib().cgx_last_error()
    rc = lib().cgx_many_create(queue.handle, 1, 1, 20, len(cl), d.ptr, d.ptr, d.ptr, len(cl),
                               C.byref(h))
    assert rc == EUNSUPPORTED and b"f32" in lib().cgx_last_error()


def test_many_check_example():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "5 agree" in r.stdout and "agreement" in r.stdout
