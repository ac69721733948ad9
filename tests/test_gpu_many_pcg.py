"""Diagonal preconditioning inside the many-systems kernel
(cgx_many_set_precond): JACOBI formed from the values each
solve reads, or a caller's DIAGONAL, in k_many_cg<R, true>.

Every expected value is a single solve in mode 1 through the C ABI with
cgx_cg_set_precond on that system's own matrix (x, bodies, cgx_cg_rxr,
cgx_cg_rz, stop code) or tests/cg_model.cg with minv; never the kernel under
test. The comparison is bit for bit (assert_array_equal), which
tests/test_many_pcg_cpu.py makes exact: no dot of any system used here is
closer than its guard to a rounding boundary. The hub row's system is pinned
to cg_model, as in tests/test_gpu_many.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests import cg_model
from tests import many_pcg_systems as P
from tests import test_gpu_many as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "many_pcg_check")
EINVAL, ESTATE = 1, 4
PAD, SENTINEL = G.PAD, G.SENTINEL
KINDS = list(P.KINDS)


def single(queue, rp, cl, vl, b, x0, tol, max_bodies, kind, m):
    """(x, bodies, rxr, stopped, rz) of cgx_cg_begin / cgx_cg_run in mode 1 with
    cgx_cg_set_precond(kind) on a matrix of this system's own."""
    A = cga.Matrix(queue, vl, cl, rp)
    n = A.N()
    h = C.c_void_p()
    check(lib().cgx_cg_create(queue.handle, A.schedule(), C.byref(h)))
    try:
        check(lib().cgx_cg_set_mode(h, 1))
        dm = None
        if kind == P.DIAGONAL:
            dm = cga.DeviceArray(queue, n, np.float64).upload(m)
        check(lib().cgx_cg_set_precond(h, kind, dm.ptr if dm is not None else None))
        db = cga.DeviceArray(queue, n, np.float64).upload(b)
        dx = cga.DeviceArray(queue, n, np.float64).upload(np.zeros(n) if x0 is None else x0)
        check(lib().cgx_cg_begin(h, db.ptr, dx.ptr, tol, max_bodies))
        cap = n + 1 if max_bodies < 0 else min(n + 1, max(max_bodies, 1))
        total, stopped, rxr, rz = C.c_int64(), C.c_int(), C.c_double(), C.c_double()
        check(lib().cgx_cg_run(h, cap, C.byref(total), C.byref(stopped)))
        check(lib().cgx_cg_rxr(h, C.byref(rxr)))
        check(lib().cgx_cg_rz(h, C.byref(rz)))
        return dx.download(), total.value, rxr.value, stopped.value, rz.value
    finally:
        lib().cgx_cg_destroy(h)


_refs = {}


def references(queue, name, kind):
    """The single preconditioned solves of a set's systems, computed once and shared."""
    if (name, kind) not in _refs:
        rp, cl, vals, B, tol, X0, mb = P.system_set(name)
        m = P.precond(name, P.KINDS[kind])
        _refs[name, kind] = [single(queue, rp, cl, vals[s], B[s], None if X0 is None else X0[s],
                                    tol, mb, P.KINDS[kind], m[s]) for s in range(len(vals))]
    return _refs[name, kind]


class PMany(G.Many):
    """tests/test_gpu_many.py's Many with a preconditioner."""

    def set_precond(self, kind, m=None, ldm=None):
        """m: (nsys, n) host values, placed at leading dimension ldm between sentinels"""
        self.ldm = self.n if ldm is None else ldm
        self.dM = self.pM = self.hM = None
        if m is not None:
            self.dM, self.pM, self.hM = G.block(self.queue, m, self.ldm)
        check(lib().cgx_many_set_precond(self.h, kind, self.pM, self.ldm))

    def set(self, name, kind, ldm=None):
        k = P.KINDS[kind]
        self.set_precond(k, P.precond(name, k) if k == P.DIAGONAL else None, ldm)

    def kind(self):
        k = C.c_int(-1)
        check(lib().cgx_many_get_precond(self.h, C.byref(k)))
        return k.value

    def rz(self):
        out = (C.c_double * self.nsys)()
        check(lib().cgx_many_rz(self.h, out))
        return np.array(out[:])

    def psolve(self, *a, **kw):
        """solve's tuple with rz appended"""
        return self.solve(*a, **kw) + (self.rz(),)


def assert_systems_equal(out, refs, which=None):
    G.assert_systems_equal(out, [r[:4] for r in refs], which)
    for s, ref in enumerate(refs):
        if which is None or s in which:
            np.testing.assert_array_equal(out[6][s], ref[4], err_msg=f"system {s}: r.z")


@pytest.mark.parametrize("kind", KINDS)
def test_several_systems_per_workgroup(queue, kind):
    rp, cl, vals, B, tol, _, _ = P.system_set("multi")
    refs = references(queue, "multi", kind)
    with PMany(queue, rp, cl, vals) as m:
        plain_lds = m.info()[2]
        m.set("multi", kind)
        assert m.kind() == P.KINDS[kind]
        three = m.psolve(B, tol=tol, max_workgroups=3)  # 12 or 13 systems per workgroup
        full = m.psolve(B, tol=tol)
        wg, r, lds = m.info()
        assert 3 < wg <= 37 and r == 4
        assert lds >= 2 * 4 * 256 * 8 and plain_lds < 2 * 4 * 256 * 8  # m is a second p
    for a, b in zip(three[:4] + three[6:], full[:4] + full[6:]):
        np.testing.assert_array_equal(a, b)
    assert_systems_equal(three, refs)
    assert_systems_equal(full, refs)
    assert len(set(three[1].tolist())) >= 3, three[1]
    assert (three[3] == 1).all() and (three[1] <= 150).all()


@pytest.mark.parametrize("n,kind", [(n, "jacobi") for n in P.SIZES] + [(257, "diagonal"),
                                                                       (4096, "diagonal")])
def test_sizes(queue, n, kind):
    name = f"n{n}"
    rp, cl, vals, B, tol, _, _ = P.system_set(name)
    with PMany(queue, rp, cl, vals) as m:
        m.set(name, kind)
        out = m.psolve(B, tol=tol)
        assert m.info()[1] == next(r for r in (1, 2, 4, 8, 16) if n <= 256 * r)
    assert_systems_equal(out, references(queue, name, kind))
    assert (out[3] == 1).all()
    nan_x = [s for s in range(3) if np.isnan(out[0][s]).any()]
    assert tuple(nan_x) == P.NAN_X.get((name, kind), ())


def test_eight_rows_per_thread(queue):
    """n = 1,025: k_many_cg<8, kManyDiag>, which no size above reaches; 9
    systems, all on one workgroup."""
    rp, cl, vals, B, tol, _, _ = P.system_set("n1025x9")
    with PMany(queue, rp, cl, vals) as m:
        m.set("n1025x9", "jacobi")
        out = m.psolve(B, tol=tol, max_workgroups=1)
        assert m.info()[:2] == (1, 8)
    assert_systems_equal(out, references(queue, "n1025x9", "jacobi"))
    assert (out[3] == 1).all()


@pytest.mark.parametrize("kind", KINDS)
def test_hub_row_against_the_model(queue, kind):
    rp, cl, vals, B, tol, _, _ = P.system_set("hub")
    mm = P.precond("hub", P.KINDS[kind])
    with PMany(queue, rp, cl, vals) as m:
        m.set("hub", kind)
        X, bodies, rxr, stopped, _, _, rz = m.psolve(B, tol=tol)
    for s in range(len(vals)):
        run = cg_model.cg(rp, cl, vals[s], B[s], tol, -1, minv=mm[s], dtype=np.float64)
        np.testing.assert_array_equal(X[s], run.x, err_msg=f"system {s}: x")
        np.testing.assert_array_equal(bodies[s], run.bodies)
        np.testing.assert_array_equal(rxr[s], run.rr[-1])
        np.testing.assert_array_equal(rz[s], run.rz[-1])
        np.testing.assert_array_equal(stopped[s], 1)


def test_diagonal_of_ones_is_the_plain_solve(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("n1023")
    with PMany(queue, rp, cl, vals) as m:
        plain = m.solve(B, tol=tol)
        assert lib().cgx_many_rz(m.h, (C.c_double * 3)()) == ESTATE  # no preconditioner
        m.set_precond(P.DIAGONAL, np.ones_like(B))
        assert lib().cgx_many_rz(m.h, (C.c_double * 3)()) == ESTATE  # no solve under it yet
        ones = m.psolve(B, tol=tol)
    for a, b in zip(plain[:4], ones[:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ones[6], ones[2])  # rz == rxr


def test_empty_row(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("empty")
    X0 = np.random.default_rng(5).standard_normal(B.shape)
    with PMany(queue, rp, cl, vals) as m:
        m.set("empty", "jacobi")  # row 31 has no diagonal entry: every system is refused
        out = m.psolve(B, X0=X0, tol=tol)
        np.testing.assert_array_equal(out[0], X0)
        np.testing.assert_array_equal(out[5][1], out[5][0])  # the whole X image, gaps included
        np.testing.assert_array_equal(out[1], np.zeros(3))
        np.testing.assert_array_equal(out[3], np.full(3, 3))
        assert np.isnan(out[2]).all() and np.isnan(out[6]).all()
        m.set("empty", "diagonal")  # m = 1 at row 31: no diagonal entry is needed
        out = m.psolve(B, tol=tol)
    assert_systems_equal(out, references(queue, "empty", "diagonal"))
    assert (out[3] == 1).all()


def test_leading_dimensions_and_sentinels(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("n65")
    n, nnz = 65, vals.shape[1]
    with PMany(queue, rp, cl, vals, ldv=nnz + 5) as m:
        m.set("n65", "diagonal", ldm=n + 11)
        out = m.psolve(B, tol=tol, ld=n + 37)
        vafter, mafter = m.vals.download(), m.dM.download()
        # refusals that need an object; the object keeps what it had
        assert lib().cgx_many_set_precond(m.h, P.DIAGONAL, m.pM, n - 1) == EINVAL
        assert b"ldm" in lib().cgx_last_error()
        assert lib().cgx_many_set_precond(m.h, 9, m.pM, n) == EINVAL
        assert lib().cgx_many_set_precond(m.h, P.DIAGONAL, m.pM + 4, n) == EINVAL
        assert lib().cgx_many_set_precond(m.h, P.DIAGONAL, None, n) == EINVAL
        assert m.kind() == P.DIAGONAL
        np.testing.assert_array_equal(m.rz(), out[6])
        again = m.psolve(B, tol=tol, ld=n + 37)
    assert_systems_equal(out, references(queue, "n65", "diagonal"))
    assert_systems_equal(again, references(queue, "n65", "diagonal"))
    np.testing.assert_array_equal(vafter, m.vhost)          # values and their gaps: untouched
    np.testing.assert_array_equal(mafter, m.hM)             # m and its gaps: untouched
    (hB, aB), (hX, aX) = out[4], out[5]
    np.testing.assert_array_equal(aB, hB)                   # B and its gaps: untouched
    ld = n + 37
    gaps = np.ones(aX.size, bool)
    for s in range(3):
        gaps[PAD + s * ld:PAD + s * ld + n] = False
    assert gaps.sum() == 2 * PAD + 3 * 37
    np.testing.assert_array_equal(aX[gaps], np.full(gaps.sum(), SENTINEL))


@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_x0_and_a_cap_of_five(queue, kind):
    rp, cl, vals, B, tol, X0, mb = P.system_set("multi5")
    with PMany(queue, rp, cl, vals) as m:
        m.set("multi5", kind)
        out = m.psolve(B, X0=X0, tol=tol, max_bodies=mb)
    assert_systems_equal(out, references(queue, "multi5", kind))
    np.testing.assert_array_equal(out[1], np.full(5, 5))
    np.testing.assert_array_equal(out[3], np.full(5, 2))


def _assert_refused_alone(out, X0, refs):
    """system 1 refused with its X as given, systems 0 and 2 equal to refs"""
    np.testing.assert_array_equal(out[3][1], 3)
    np.testing.assert_array_equal(out[1][1], 0)
    assert np.isnan(out[2][1]) and np.isnan(out[6][1])
    np.testing.assert_array_equal(out[0][1], X0[1])
    assert_systems_equal(out, refs, which=[0, 2])


@pytest.mark.parametrize("bad", ["negative", "zero", "nan", "inf"])
def test_bad_diagonal_stops_its_own_system(queue, bad):
    rp, cl, vals, B, tol, _, _ = P.system_set("n63")
    e = int(rp[0] + np.nonzero(cl[rp[0]:rp[1]] == 0)[0][0])  # a_00's entry
    value = lambda v: {"negative": -abs(v), "zero": 0.0, "nan": np.nan, "inf": np.inf}[bad]  # noqa: E731
    X0 = np.zeros_like(B)
    X0[1] = SENTINEL / 3 + np.arange(63)  # system 1's guess: must come back untouched
    # JACOBI: a_00 of system 1
    v2 = vals.copy()
    v2[1, e] = value(vals[1, e])
    with PMany(queue, rp, cl, v2) as m:
        m.set_precond(P.JACOBI)
        out = m.psolve(B, X0=X0, tol=tol, max_workgroups=1)  # one workgroup runs all three
        _assert_refused_alone(out, X0, references(queue, "n63", "jacobi"))
        out = m.psolve(B, X0=X0, tol=tol)
        _assert_refused_alone(out, X0, references(queue, "n63", "jacobi"))
    # DIAGONAL: m_0 of system 1
    mm = P.precond("n63", P.DIAGONAL).copy()
    mm[1, 0] = value(mm[1, 0])
    with PMany(queue, rp, cl, vals) as m:
        m.set_precond(P.DIAGONAL, mm)
        out = m.psolve(B, X0=X0, tol=tol, max_workgroups=1)
        _assert_refused_alone(out, X0, references(queue, "n63", "diagonal"))


def test_nan_in_b_stays_in_its_system(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("multi")
    vals, B = vals[:8].copy(), B[:8].copy()
    refs = references(queue, "multi", "jacobi")[:8]
    B[2, 5] = np.nan
    with PMany(queue, rp, cl, vals) as m:
        m.set_precond(P.JACOBI)
        out = m.psolve(B, tol=tol, max_workgroups=2)  # it shares a workgroup with three others
    assert_systems_equal(out, refs, which=[s for s in range(8) if s != 2])
    ref = single(queue, rp, cl, vals[2], B[2], None, tol, -1, P.JACOBI, None)
    assert np.isnan(ref[2]) and ref[3] == 1
    assert_systems_equal((out[0][2:3], out[1][2:3], out[2][2:3], out[3][2:3], None, None,
                          out[6][2:3]), [ref])


def test_python_class_and_values_overwritten_in_place(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("n255")
    refs = references(queue, "n255", "jacobi")
    m = cga.ManyCG(queue, rp, cl, vals)
    try:
        plain = m.solve(B, improvement=tol)
        assert m.rz is None
        plain_out = (plain, m.bodies, m.rxr, m.stopped)
        m.set_preconditioner(cga.Preconditioner.Jacobi)
        X = m.solve(B, improvement=tol)
        assert X.shape == B.shape and m.info()[1] == 1 and m.info()[2] >= 2 * 256 * 8
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz), refs)
        # system s now takes the values of system 2 - s: the diagonal must follow
        m.set_values(vals[::-1])
        X = m.solve(B, improvement=tol)
        swapped = [single(queue, rp, cl, vals[2 - s], B[s], None, tol, -1, P.JACOBI, None)
                   for s in range(3)]
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz), swapped)
        assert not np.array_equal(X[0], refs[0][0])
        # the caller's diagonal through the class, then back to the plain loop
        m.set_values(vals)
        m.set_preconditioner(cga.Preconditioner.Diagonal, P.precond("n255", P.DIAGONAL))
        X = m.solve(B, improvement=tol)
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz),
                             references(queue, "n255", "diagonal"))
        m.set_preconditioner(cga.Preconditioner.None_)
        X = m.solve(B, improvement=tol)
        assert m.rz is None
        for a, b in zip((X, m.bodies, m.rxr, m.stopped), plain_out):
            np.testing.assert_array_equal(a, b)
    finally:
        m.close()


def test_set_precond_between_solves(queue):
    rp, cl, vals, B, tol, _, _ = P.system_set("n257")
    with PMany(queue, rp, cl, vals) as m:
        assert m.kind() == P.NONE
        first = m.solve(B, tol=tol)
        m.set_precond(P.JACOBI)
        jac = m.psolve(B, tol=tol)
        m.set_precond(P.NONE)
        assert m.kind() == P.NONE
        assert lib().cgx_many_rz(m.h, (C.c_double * 3)()) == ESTATE
        assert b"no preconditioner" in lib().cgx_last_error()
        last = m.solve(B, tol=tol)
    assert_systems_equal(jac, references(queue, "n257", "jacobi"))
    for a, b in zip(first[:4], last[:4]):
        np.testing.assert_array_equal(a, b)


def test_many_pcg_check_example():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "5 agree" in r.stdout and "isolated" in r.stdout and ": agreement" in r.stdout
