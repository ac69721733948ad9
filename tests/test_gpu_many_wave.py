"""A wave per system in the many-systems solve (cgx_many_set_form, DESIGN.md
§5e): k_many_cg_wave<R, PC>, R = 1, 2, 4 rows per lane for n <= 256, four
independent solves per workgroup and no workgroup barrier.

Every expected value is a single solve in mode 1 through the C ABI (with
cgx_cg_set_precond under a preconditioner), as in tests/test_gpu_many.py and
tests/test_gpu_many_pcg.py, whose helpers and cached references this module
shares; never the kernel under test. Everything is compared bit for bit
(assert_array_equal), which tests/test_many_cpu.py, tests/test_many_pcg_cpu.py
and tests/test_many_wave_cpu.py make exact: no dot of any system used here is
closer than its guard to a rounding boundary. The workgroup form of the same
object is compared as well; for n <= 64 it must agree clear or not, NaN
systems included (cgx.h).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests import many_wave_systems as W
from tests import test_gpu_many as G
from tests import test_gpu_many_pcg as GP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "many_wave_check")
EINVAL, EUNSUPPORTED = 1, 6
AUTO, WORKGROUP, WAVE = 0, 1, 2
PAD, SENTINEL = G.PAD, G.SENTINEL
KINDS = list(W.KINDS)

_refs = {}


def references(queue, name, kind=None):
    """The single solves of a set's systems (kind: None plain, "jacobi" or
    "diagonal"), computed once and shared; the older modules' caches serve
    their own sets."""
    if name not in W.ALL_SETS:
        return G.references(queue, name) if kind is None else GP.references(queue, name, kind)
    if (name, kind) not in _refs:
        rp, cl, vals, B, tol, _, mb = W.system_set(name)
        if kind is None:
            _refs[name, kind] = [G.single(queue, rp, cl, vals[s], B[s], None, tol, mb)
                                 for s in range(len(vals))]
        else:
            m = W.precond(name, W.KINDS[kind])
            _refs[name, kind] = [GP.single(queue, rp, cl, vals[s], B[s], None, tol, mb,
                                           W.KINDS[kind], m[s]) for s in range(len(vals))]
    return _refs[name, kind]


class WMany(GP.PMany):
    """tests/test_gpu_many_pcg.py's PMany with the form calls."""

    def set_form(self, form):
        check(lib().cgx_many_set_form(self.h, form))

    def form(self):
        req, eff = C.c_int(-1), C.c_int(-1)
        check(lib().cgx_many_get_form(self.h, C.byref(req), C.byref(eff)))
        return req.value, eff.value

    def both(self, *a, pc=False, **kw):
        """-> the solve in the wave form and in the workgroup form, the object
        left in the wave form"""
        run = self.psolve if pc else self.solve
        self.set_form(WAVE)
        wave = run(*a, **kw)
        self.set_form(WORKGROUP)
        wg = run(*a, **kw)
        self.set_form(WAVE)
        return wave, wg


def assert_same(a, b, pc=False):
    """x, bodies, r.r, stop code (and r.z) of two solve tuples"""
    for u, v in zip(a[:4] + (a[6:] if pc else ()), b[:4] + (b[6:] if pc else ())):
        np.testing.assert_array_equal(u, v)


def rows_per_lane(n):
    return next(r for r in (1, 2, 4) if n <= 64 * r)


@pytest.mark.parametrize("name", ["n1", "n2", "n63", "n64", "empty", "n65", "n128", "n129",
                                  "n255", "n256"])
def test_sizes(queue, name):
    rp, cl, vals, B, tol, _, _ = W.system_set(name)
    n = len(rp) - 1
    with WMany(queue, rp, cl, vals) as m:
        wave, wg = m.both(B, tol=tol)
        assert m.form() == (WAVE, WAVE)
        grid, r, lds = m.info()
        assert r == rows_per_lane(n) and lds == 4 * r * 64 * 8 and grid == 1
        m.set_form(WORKGROUP)
        assert m.form() == (WORKGROUP, WORKGROUP) and m.info()[1] == 1
    G.assert_systems_equal(wave, references(queue, name))
    assert_same(wave, wg)
    assert (wave[3] == 1).all()


@pytest.mark.parametrize("name", W.W_SETS)
def test_several_systems_per_wave_and_waves_that_finish_apart(queue, name):
    rp, cl, vals, B, tol, _, _ = W.system_set(name)
    nsys = len(vals)
    refs = references(queue, name)
    with WMany(queue, rp, cl, vals) as m:
        m.set_form(WAVE)
        three = m.solve(B, tol=tol, max_workgroups=3)  # 12 waves, 3 to 4 systems per wave
        check(lib().cgx_many_config(m.h, 3))
        assert m.info()[0] == 3
        full = m.solve(B, tol=tol)
        assert m.info()[0] == -(-nsys // 4)  # (far below the resident workgroups)
    assert_same(three, full)
    G.assert_systems_equal(three, refs)
    G.assert_systems_equal(full, refs)
    assert len(set(three[1].tolist())) >= 3, three[1]
    assert (three[3] == 1).all()


def test_one_system(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("w63x41")
    with WMany(queue, rp, cl, vals[:1]) as m:  # three idle waves
        wave, wg = m.both(B[:1], tol=tol)
        assert m.info()[0] == 1
    G.assert_systems_equal(wave, references(queue, "w63x41")[:1])
    assert_same(wave, wg)


def test_leading_dimensions_and_sentinels(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("n65")
    n, nnz = 65, vals.shape[1]
    with WMany(queue, rp, cl, vals, ldv=nnz + 5) as m:
        m.set_form(WAVE)
        out = m.solve(B, tol=tol, ld=n + 37)
        assert m.info()[1] == 2
        vafter = m.vals.download()
    G.assert_systems_equal(out, references(queue, "n65"))
    np.testing.assert_array_equal(vafter, m.vhost)          # values and their gaps: untouched
    (hB, aB), (hX, aX) = out[4], out[5]
    np.testing.assert_array_equal(aB, hB)                   # B and its gaps: untouched
    ld = n + 37
    gaps = np.ones(aX.size, bool)
    for s in range(3):
        gaps[PAD + s * ld:PAD + s * ld + n] = False
    assert gaps.sum() == 2 * PAD + 3 * 37
    np.testing.assert_array_equal(aX[gaps], np.full(gaps.sum(), SENTINEL))


def test_nonzero_x0_and_a_cap_of_five(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("w63x41")
    vals, B = vals[:5].copy(), B[:5].copy()
    X0 = np.random.default_rng(43).standard_normal(B.shape)
    with WMany(queue, rp, cl, vals) as m:
        wave, wg = m.both(B, X0=X0, tol=tol, max_bodies=5)
    refs = [G.single(queue, rp, cl, vals[s], B[s], X0[s], tol, 5) for s in range(5)]
    G.assert_systems_equal(wave, refs)
    assert_same(wave, wg)
    np.testing.assert_array_equal(wave[1], np.full(5, 5))
    np.testing.assert_array_equal(wave[3], np.full(5, 2))


def test_nan_and_inf_stay_in_their_system(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("w63x41")
    vals, B = vals[:8].copy(), B[:8].copy()
    refs = references(queue, "w63x41")[:8]
    B[2, 5] = np.nan
    vals[5, 17] = np.inf
    with WMany(queue, rp, cl, vals) as m:
        wave, wg = m.both(B, tol=tol, max_workgroups=1)  # the two share a workgroup with the rest
    G.assert_systems_equal(wave, refs, which=[s for s in range(8) if s not in (2, 5)])
    for s in (2, 5):
        xr, kr, rr, sr = G.single(queue, rp, cl, vals[s], B[s], None, tol, -1)
        assert np.isnan(rr) and sr == 1
        np.testing.assert_array_equal(wave[1][s], kr)
        np.testing.assert_array_equal(wave[3][s], sr)
        np.testing.assert_array_equal(wave[2][s], rr)
        np.testing.assert_array_equal(wave[0][s], xr)
    assert_same(wave, wg)  # n <= 64: the same bits, NaN systems included


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", W.W_SETS)
def test_preconditioned(queue, name, kind):
    rp, cl, vals, B, tol, _, _ = W.system_set(name)
    n = len(rp) - 1
    k = W.KINDS[kind]
    refs = references(queue, name, kind)
    with WMany(queue, rp, cl, vals) as m:
        m.set_precond(k, W.precond(name, k) if k == W.DIAGONAL else None)
        wave, wg = m.both(B, pc=True, tol=tol, max_workgroups=3)
        r = rows_per_lane(n)
        assert m.info()[1:] == (r, 2 * 4 * r * 64 * 8)
        full = m.psolve(B, tol=tol)
    GP.assert_systems_equal(wave, refs)
    assert_same(wave, wg, pc=True)
    assert_same(wave, full, pc=True)
    assert (wave[3] == 1).all()


def test_diagonal_of_ones_is_the_plain_wave_solve(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("w65x21")
    with WMany(queue, rp, cl, vals) as m:
        m.set_form(WAVE)
        plain = m.solve(B, tol=tol)
        m.set_precond(W.DIAGONAL, np.ones_like(B))
        ones = m.psolve(B, tol=tol)
    assert_same(plain, ones)
    np.testing.assert_array_equal(ones[6], ones[2])  # rz == rxr


def test_jacobi_follows_values_overwritten_in_place(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("n128")
    nnz = vals.shape[1]
    with WMany(queue, rp, cl, vals) as m:
        m.set_form(WAVE)
        m.set_precond(W.JACOBI)
        first = m.psolve(B, tol=tol)
        host = m.vhost.copy()  # system s now takes the values of system 2 - s: no new create
        host[PAD:PAD + 3 * nnz].reshape(3, nnz)[:] = vals[::-1]
        m.vals.upload(host)
        second = m.psolve(B, tol=tol)
    GP.assert_systems_equal(first, references(queue, "n128", "jacobi"))
    swapped = [GP.single(queue, rp, cl, vals[2 - s], B[s], None, tol, -1, W.JACOBI, None)
               for s in range(3)]
    GP.assert_systems_equal(second, swapped)
    assert not np.array_equal(second[0][0], first[0][0])


@pytest.mark.parametrize("case", ["jacobi-negative", "jacobi-zero", "diagonal-nan"])
def test_bad_diagonal_stops_its_own_system(queue, case):
    rp, cl, vals, B, tol, _, _ = W.system_set("w63x41")
    vals, B = vals[:8].copy(), B[:8].copy()
    kind, bad_s = case.split("-")[0], 5
    refs = references(queue, "w63x41", kind)[:8]
    X0 = np.zeros_like(B)
    X0[bad_s] = SENTINEL / 3 + np.arange(63)  # its guess: must come back untouched
    mm = None
    if kind == "jacobi":
        e = int(rp[9] + np.nonzero(cl[rp[9]:rp[10]] == 9)[0][0])  # a_99's entry
        vals[bad_s, e] = {"negative": -vals[bad_s, e], "zero": 0.0}[case.split("-")[1]]
    else:
        mm = W.precond("w63x41", W.DIAGONAL)[:8].copy()
        mm[bad_s, 9] = np.nan
    with WMany(queue, rp, cl, vals) as m:
        m.set_precond(W.KINDS[kind], mm)
        wave, wg = m.both(B, pc=True, X0=X0, tol=tol, max_workgroups=1)  # one workgroup runs all
    np.testing.assert_array_equal(wave[3][bad_s], 3)
    np.testing.assert_array_equal(wave[1][bad_s], 0)
    assert np.isnan(wave[2][bad_s]) and np.isnan(wave[6][bad_s])
    np.testing.assert_array_equal(wave[0][bad_s], X0[bad_s])
    GP.assert_systems_equal(wave, refs, which=[s for s in range(8) if s != bad_s])
    assert_same(wave, wg, pc=True)


def test_form_api(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("n257")
    with WMany(queue, rp, cl, vals) as m:
        assert m.form() == (AUTO, WORKGROUP)
        assert lib().cgx_many_set_form(m.h, WAVE) == EUNSUPPORTED
        msg = lib().cgx_last_error()
        assert b"256" in msg and b"workgroup form" in msg
        assert m.form() == (AUTO, WORKGROUP)
        m.set_form(WORKGROUP)
        assert lib().cgx_many_set_form(m.h, 3) == EINVAL
        assert lib().cgx_many_set_form(m.h, -1) == EINVAL
        assert m.form() == (WORKGROUP, WORKGROUP) and m.info()[1] == 2
        out = m.solve(B, tol=tol)  # after the refused calls: the form it had
    G.assert_systems_equal(out, references(queue, "n257"))
    # auto: the wave form up to 64 rows, the workgroup form above
    for name, eff in (("n64", WAVE), ("n65", WORKGROUP), ("n256", WORKGROUP)):
        rp, cl, vals, B, tol, _, _ = W.system_set(name)
        with WMany(queue, rp, cl, vals) as m:
            assert m.form() == (AUTO, eff) and m.info()[1] == 1
    # both ways between solves on one object
    rp, cl, vals, B, tol, _, _ = W.system_set("n65")
    refs = references(queue, "n65")
    with WMany(queue, rp, cl, vals) as m:
        for form, r in ((WAVE, 2), (WORKGROUP, 1), (WAVE, 2), (AUTO, 1)):
            m.set_form(form)
            assert m.form()[0] == form and m.info()[1] == r
            assert lib().cgx_many_set_form(m.h, 7) == EINVAL
            assert m.form()[0] == form
            G.assert_systems_equal(m.solve(B, tol=tol), refs)


def test_python_class(queue):
    rp, cl, vals, B, tol, _, _ = W.system_set("n63")
    refs = references(queue, "n63")
    m = cga.ManyCG(queue, rp, cl, vals)
    try:
        assert m.form[0] == cga.MANY_FORM_AUTO
        m.set_form(cga.ManyCG.FORM_WAVE)
        assert m.form == (WAVE, WAVE) and m.info()[1:] == (1, 2048)
        X = m.solve(B, improvement=tol)
        G.assert_systems_equal((X, m.bodies, m.rxr, m.stopped), refs)
        m.set_form(cga.MANY_FORM_WORKGROUP)
        assert m.form == (WORKGROUP, WORKGROUP)
        X2 = m.solve(B, improvement=tol)
        np.testing.assert_array_equal(X2, X)
        with pytest.raises(ValueError, match="unknown form"):
            m.set_form(5)
        assert m.form == (WORKGROUP, WORKGROUP)
    finally:
        m.close()
    rp, cl, vals = W.system_set("n257")[:3]
    m = cga.ManyCG(queue, rp, cl, vals)
    try:
        with pytest.raises(cga.CgxError, match="256"):
            m.set_form(cga.MANY_FORM_WAVE)
        assert m.form == (AUTO, WORKGROUP)
    finally:
        m.close()


def test_many_wave_check_example():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "plain identical" in r.stdout and "Jacobi identical" in r.stdout
    assert ": agreement" in r.stdout
