"""Block-Jacobi preconditioning inside the many-systems kernels
(cgx_many_set_block_precond): k_many_block_inv,
k_many_block_check and the block variants of k_many_cg and k_many_cg_wave.

Every expected value is a single solve in mode 1 through the C ABI with
cgx_cg_set_block_precond on that system's own matrix (x, bodies, cgx_cg_rxr,
cgx_cg_rz, stop code) and tests/bj_model.cg; never the kernel under test. The
comparison is bit for bit (assert_array_equal), which
tests/test_many_block_pcg_cpu.py makes exact: no dot of any system used here
(tests/many_block_systems.py) is closer than its guard to a rounding boundary.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests import bj_model
from tests import many_block_systems as S
from tests import many_pcg_systems as P
from tests import test_gpu_many as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "many_block_pcg_check")
EINVAL, ESTATE = 1, 4
PAD, SENTINEL = G.PAD, G.SENTINEL
KINDS = list(S.KINDS)
WORKGROUP, WAVE = 1, 2


def single(queue, rp, cl, vl, b, x0, tol, max_bodies, kind, bs, W):
    """(x, bodies, rxr, stopped, rz) of cgx_cg_begin / cgx_cg_run in mode 1 with
    cgx_cg_set_block_precond(kind, bs, W) on a matrix of this system's own."""
    A = cga.Matrix(queue, vl, cl, rp)
    n = A.N()
    h = C.c_void_p()
    check(lib().cgx_cg_create(queue.handle, A.schedule(), C.byref(h)))
    try:
        check(lib().cgx_cg_set_mode(h, 1))
        dw = None
        if kind == S.GIVEN:
            dw = cga.DeviceArray(queue, n * bs, np.float64).upload(np.ravel(W))
        check(lib().cgx_cg_set_block_precond(h, kind, bs, dw.ptr if dw is not None else None))
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
    """The single block-preconditioned solves of a set's systems, computed once
    and shared; each is first held to the model's run."""
    if (name, kind) not in _refs:
        rp, cl, vals, B, tol, X0, mb, bs = S.system_set(name)
        W = S.precond(name, S.KINDS[kind])
        refs = [single(queue, rp, cl, vals[s], B[s], None if X0 is None else X0[s], tol, mb,
                       S.KINDS[kind], bs, W[s]) for s in range(len(vals))]
        for s, (ref, run) in enumerate(zip(refs, S.model_runs(name, kind))):
            np.testing.assert_array_equal(ref[0], run.x, err_msg=f"{name}[{s}] {kind}: x")
            np.testing.assert_array_equal(np.array([ref[1], ref[2], ref[4]]),
                                          np.array([run.bodies, run.rr[-1], run.rz[-1]]),
                                          err_msg=f"{name}[{s}] {kind}: bodies, r.r, r.z")
        _refs[name, kind] = refs
    return _refs[name, kind]


class BMany(G.Many):
    """tests/test_gpu_many.py's Many with the block preconditioner's calls."""

    def set_block(self, kind, bs=0, W=None, ldw=None):
        """W: (nsys, n, bs) host values, placed at leading dimension ldw between sentinels"""
        self.ldw = self.n * bs if ldw is None else ldw
        self.dW = self.pW = self.hW = None
        if W is not None:
            self.dW, self.pW, self.hW = G.block(self.queue, W.reshape(len(W), -1), self.ldw)
        check(lib().cgx_many_set_block_precond(self.h, kind, bs, self.pW, self.ldw))

    def set(self, name, kind, ldw=None):
        k, bs = S.KINDS[kind], S.system_set(name)[7]
        self.set_block(k, bs, S.precond(name, k) if k == S.GIVEN else None, ldw)

    def set_diag(self, kind):
        check(lib().cgx_many_set_precond(self.h, kind, None, self.n))

    def set_form(self, form):
        check(lib().cgx_many_set_form(self.h, form))

    def kinds(self):
        k, bk, bs = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        check(lib().cgx_many_get_precond(self.h, C.byref(k)))
        check(lib().cgx_many_get_block_precond(self.h, C.byref(bk), C.byref(bs)))
        return k.value, bk.value, bs.value

    def rz(self):
        out = (C.c_double * self.nsys)()
        check(lib().cgx_many_rz(self.h, out))
        return np.array(out[:])

    def psolve(self, *a, **kw):
        """solve's tuple with rz appended"""
        return self.solve(*a, **kw) + (self.rz(),)

    def block_inv(self, bs, ldw=None):
        """-> W (nsys, n, bs), n_bad, first_bad, the whole device image, its host image before"""
        ldw = self.n * bs if ldw is None else ldw
        d, ptr, host = G.block(self.queue, np.zeros((self.nsys, 0)), ldw)
        nb, fb = C.c_int64(-5), C.c_int64(-5)
        check(lib().cgx_many_block_inv(self.h, bs, ptr, ldw, C.byref(nb), C.byref(fb)))
        after = d.download()
        W = after[PAD:PAD + self.nsys * ldw].reshape(self.nsys, ldw)[:, :self.n * bs]
        return W.reshape(self.nsys, self.n, bs).copy(), nb.value, fb.value, after, host


def assert_systems_equal(out, refs, which=None):
    G.assert_systems_equal(out, [r[:4] for r in refs], which)
    for s, ref in enumerate(refs):
        if which is None or s in which:
            np.testing.assert_array_equal(out[6][s], ref[4], err_msg=f"system {s}: r.z")


# 1 -- cgx_many_block_inv --------------------------------------------------------
def M_dense(n, seed):
    from tests import many_systems as M

    return M.dense_spd(n, seed)


def _inv_pattern(n):
    if n <= 7:
        return M_dense(n, 100 + n)
    nx, ny = {65: (6, 4), 257: (10, 9)}[n]
    from conjugategradient_amd.workloads import node_mixed

    return S.cut(*node_mixed(nx, ny, 3, S.E, 7), n)


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


def _variants3(rp, cl, vl):
    from tests import many_systems as M

    return M.variants(rp, cl, vl, 3, seed=77, width=0.25)[0]


@pytest.mark.parametrize("n", [1, 2, 7, 65, 257, "shuffled-split"])
def test_block_inv_is_the_models_bit_for_bit(queue, n):
    """bs = 1..8 on n = 1, 2, 7 (n < bs: one partial block), 65, 257, and on
    unsorted rows with duplicate entries; the sentinels in [n bs, ldw) and
    around the array stay."""
    if n == "shuffled-split":
        rp, cl, vl = _shuffled_split(*_inv_pattern(65))
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
        assert (np.bincount(rows[rows == cl]) == 2).all() and (np.diff(cl[:4]) < 0).any()
    else:
        rp, cl, vl = _inv_pattern(n)
    vals = _variants3(rp, cl, vl)
    nn = len(rp) - 1
    with BMany(queue, rp, cl, vals) as m:
        for bs in range(1, 9):
            got, nb, fb, after, before = m.block_inv(bs, ldw=nn * bs + 3)
            assert (nb, fb) == (0, -1)
            for s in range(3):
                W, bad = bj_model.csr_block_inverse(rp, cl, vals[s], bs)
                assert not bad
                np.testing.assert_array_equal(got[s], W, err_msg=f"n {n} bs {bs} system {s}")
                np.testing.assert_array_equal(np.signbit(got[s]), np.signbit(W))
            gaps = np.ones(after.size, bool)
            for s in range(3):
                gaps[PAD + s * (nn * bs + 3):PAD + s * (nn * bs + 3) + nn * bs] = False
            assert gaps.sum() == 2 * PAD + 9
            np.testing.assert_array_equal(after[gaps], before[gaps])


def test_block_inv_counts_the_bad_systems(queue):
    """System 1 made indefinite in block 7 (bs = 3): a_21,21 negated."""
    rp, cl, vl = _inv_pattern(65)
    vals = _variants3(rp, cl, vl).copy()
    e = int(rp[21] + np.nonzero(cl[rp[21]:rp[22]] == 21)[0][0])
    vals[1, e] = -vals[1, e]
    assert bj_model.csr_block_inverse(rp, cl, vals[1], 3)[1] == [7]
    with BMany(queue, rp, cl, vals) as m:
        assert lib().cgx_many_block_bad(m.h, (C.c_int * 3)()) == ESTATE  # no block_inv yet
        got, nb, fb, _, _ = m.block_inv(3)
        assert (nb, fb) == (1, 1)
        for s in range(3):  # a bad block's W holds whatever the statements give
            np.testing.assert_array_equal(got[s], bj_model.csr_block_inverse(rp, cl, vals[s], 3)[0])
        assert m.block_inv(1)[1:3] == (1, 1)
        verdicts = (C.c_int * 3)(7, 7, 7)
        check(lib().cgx_many_block_bad(m.h, verdicts))
        assert verdicts[:] == [0, 1, 0]
        assert lib().cgx_many_block_inv(m.h, 3, None, 65 * 3, None, None) == EINVAL
        assert lib().cgx_many_block_inv(m.h, 9, m.vptr, 65 * 9, None, None) == EINVAL
        assert lib().cgx_many_block_inv(m.h, 3, m.vptr, 65 * 3 - 1, None, None) == EINVAL
        assert b"ldw" in lib().cgx_last_error()


# 2 -- solves against the single solver and the model ---------------------------
WG_SETS = ["n257b3", "n396b3", "n1023b7", "n4096b8", "n4096b5"]
WAVE_SETS = ["n60b3", "n65b3", "n255b8", "n256b8"]
TINY_SETS = ["n1b3", "n2b3", "n7b8"]


def _solve_set(queue, name, kind, form):
    rp, cl, vals, B, tol, X0, mb, bs = S.system_set(name)
    with BMany(queue, rp, cl, vals) as m:
        m.set_form(form)
        m.set(name, kind)
        assert m.kinds() == (P.NONE, S.KINDS[kind], bs)
        out = m.psolve(B, X0=X0, tol=tol, max_bodies=mb)
        info = m.info()
    print(f"{name} {kind} form {form}: bodies {out[1].tolist()}")
    return out, info


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", WG_SETS)
def test_workgroup_form(queue, name, kind):
    n, mb = S.SETS[name][3], S.SETS[name][6]
    out, (wg, r, lds) = _solve_set(queue, name, kind, WORKGROUP)
    assert r == next(k for k in (1, 2, 4, 8, 16) if n <= 256 * k)
    # p, the staged r with the 8 doubles a partial block's reads may run over, the reduction words
    assert lds == (2 * r * 256 + 8 + 32) * 8
    assert_systems_equal(out, references(queue, name, kind))
    assert (out[3] == (1 if mb < 0 else 2)).all()


def test_eight_rows_per_thread(queue):
    """n = 1,025, bs = 3 (a partial block of 2): k_many_cg<8, kManyBlock>, which
    no set of many_block_systems reaches; 9 systems, all on one workgroup. The
    set is built as many_block_systems.build builds its own, with the first
    variants seed from 300 up (301) that leaves no dot of the model's runs
    unclear, which is asserted here."""
    from conjugategradient_amd.workloads import node_mixed
    from tests import many_systems as M

    bs, n, nsys = 3, 1025, 9
    rp, cl, vl = S.cut(*node_mixed(19, 18, bs, S.E, 7), n)
    vals, B = M.variants(rp, cl, vl, nsys, seed=301, width=0.25)
    tol = M._tol(B)
    refs = []
    for s in range(nsys):
        W, bad = bj_model.csr_block_inverse(rp, cl, vals[s], bs)
        run = bj_model.cg(rp, cl, vals[s], B[s], tol, -1, W)
        assert not bad and not run.unclear, s
        ref = single(queue, rp, cl, vals[s], B[s], None, tol, -1, S.JACOBI, bs, None)
        np.testing.assert_array_equal(ref[0], run.x, err_msg=f"system {s}: x")
        np.testing.assert_array_equal(np.array([ref[1], ref[2], ref[4]]),
                                      np.array([run.bodies, run.rr[-1], run.rz[-1]]))
        refs.append(ref)
    with BMany(queue, rp, cl, vals) as m:
        m.set_block(S.JACOBI, bs)
        out = m.psolve(B, tol=tol, max_workgroups=1)
        assert m.info()[:2] == (1, 8)
    assert_systems_equal(out, refs)
    assert (out[3] == 1).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", WAVE_SETS)
def test_wave_form(queue, name, kind):
    n = S.SETS[name][3]
    out, (wg, r, lds) = _solve_set(queue, name, kind, WAVE)
    assert r == next(k for k in (1, 2, 4) if n <= 64 * k) and lds == (2 * 4 * r * 64 + 8) * 8
    assert_systems_equal(out, references(queue, name, kind))
    assert (out[3] == 1).all()


@pytest.mark.parametrize("form", [WORKGROUP, WAVE])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", TINY_SETS)
def test_a_single_partial_block(queue, name, kind, form):
    out, _ = _solve_set(queue, name, kind, form)
    assert_systems_equal(out, references(queue, name, kind))
    assert (out[3] == 1).all()
    nan_x = tuple(s for s in range(3) if np.isnan(out[0][s]).any())
    assert nan_x == S.NAN_X.get((name, kind), ())


# 3 -- pins -----------------------------------------------------------------------
@pytest.mark.parametrize("form", [WORKGROUP, WAVE])
def test_one_row_blocks_are_the_in_kernel_jacobi(queue, form):
    rp, cl, vals, B, tol, _, _, _ = S.system_set("n65b3")
    with BMany(queue, rp, cl, vals) as m:
        m.set_form(form)
        m.set_diag(P.JACOBI)
        jac = m.psolve(B, tol=tol)
        m.set_block(S.JACOBI, 1)
        blk = m.psolve(B, tol=tol)
    for a, b in zip(jac[:4] + jac[6:], blk[:4] + blk[6:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("name,bs", [("n257b3", 3), ("n60b3", 8)])
def test_identity_blocks_are_the_plain_solve(queue, name, bs):
    rp, cl, vals, B, tol, _, _, _ = S.system_set(name)
    n = len(rp) - 1
    W = np.zeros((3, n, bs))
    W[:, np.arange(n), np.arange(n) % bs] = 1.0
    with BMany(queue, rp, cl, vals) as m:
        plain = m.solve(B, tol=tol, max_bodies=40)
        m.set_block(S.GIVEN, bs, W)
        ident = m.psolve(B, tol=tol, max_bodies=40)
    for a, b in zip(plain[:4], ident[:4]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(ident[6], ident[2])  # rz == rxr


@pytest.mark.parametrize("kind", KINDS)
def test_the_two_forms_agree_at_60_rows(queue, kind):
    a, _ = _solve_set(queue, "n60b3", kind, WAVE)
    b, _ = _solve_set(queue, "n60b3", kind, WORKGROUP)
    for u, v in zip(a[:4] + a[6:], b[:4] + b[6:]):
        np.testing.assert_array_equal(u, v)


# 4 -- other cases ----------------------------------------------------------------
@pytest.mark.parametrize("form", [WORKGROUP, WAVE])
@pytest.mark.parametrize("kind", KINDS)
def test_several_systems_per_workgroup_and_per_wave(queue, kind, form):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("multi11")
    refs = references(queue, "multi11", kind)
    with BMany(queue, rp, cl, vals) as m:
        m.set_form(form)
        m.set("multi11", kind)
        two = m.psolve(B, tol=tol, max_workgroups=2)  # 5 or 6 systems a workgroup, 1 or 2 a wave
        check(lib().cgx_many_config(m.h, 2))
        assert m.info()[0] == 2
        full = m.psolve(B, tol=tol)
    assert_systems_equal(two, refs)
    assert_systems_equal(full, refs)
    assert len(set(two[1].tolist())) >= 2, two[1]


@pytest.mark.parametrize("form", [WORKGROUP, WAVE])
def test_leading_dimensions_and_sentinels(queue, form):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("n65b3")
    n, nnz = 65, vals.shape[1]
    refs = references(queue, "n65b3", "given")
    with BMany(queue, rp, cl, vals, ldv=nnz + 5) as m:
        m.set_form(form)
        m.set("n65b3", "given", ldw=n * bs + 13)
        out = m.psolve(B, tol=tol, ld=n + 37)
        vafter, wafter = m.vals.download(), m.dW.download()
        # the refusals that need an object; the object keeps what it had
        assert lib().cgx_many_set_block_precond(m.h, S.GIVEN, bs, m.pW, n * bs - 1) == EINVAL
        assert b"ldw" in lib().cgx_last_error()
        assert lib().cgx_many_set_block_precond(m.h, 9, bs, m.pW, n * bs) == EINVAL
        assert lib().cgx_many_set_block_precond(m.h, S.GIVEN, 9, m.pW, n * 9) == EINVAL
        assert lib().cgx_many_set_block_precond(m.h, S.GIVEN, bs, m.pW + 4, n * bs) == EINVAL
        assert lib().cgx_many_set_block_precond(m.h, S.GIVEN, bs, None, n * bs) == EINVAL
        assert m.kinds() == (P.NONE, S.GIVEN, bs)
        np.testing.assert_array_equal(m.rz(), out[6])
        again = m.psolve(B, tol=tol, ld=n + 37)
    assert_systems_equal(out, refs)
    assert_systems_equal(again, refs)
    np.testing.assert_array_equal(vafter, m.vhost)  # values and their gaps: untouched
    np.testing.assert_array_equal(wafter, m.hW)     # W and its gaps: untouched
    (hB, aB), (hX, aX) = out[4], out[5]
    np.testing.assert_array_equal(aB, hB)           # B and its gaps: untouched
    ld = n + 37
    gaps = np.ones(aX.size, bool)
    for s in range(3):
        gaps[PAD + s * ld:PAD + s * ld + n] = False
    assert gaps.sum() == 2 * PAD + 3 * 37
    np.testing.assert_array_equal(aX[gaps], np.full(gaps.sum(), SENTINEL))


@pytest.mark.parametrize("kind", KINDS)
def test_nonzero_x0_and_a_cap_of_five(queue, kind):
    out, _ = _solve_set(queue, "n396b3x0", kind, WORKGROUP)
    assert_systems_equal(out, references(queue, "n396b3x0", kind))
    np.testing.assert_array_equal(out[1], np.full(5, 5))
    np.testing.assert_array_equal(out[3], np.full(5, 2))


def _assert_refused_alone(out, X0, refs):
    """system 1 refused with its X as given, systems 0 and 2 equal to refs"""
    np.testing.assert_array_equal(out[3][1], 3)
    np.testing.assert_array_equal(out[1][1], 0)
    assert np.isnan(out[2][1]) and np.isnan(out[6][1])
    np.testing.assert_array_equal(out[0][1], X0[1])
    assert_systems_equal(out, refs, which=[0, 2])


@pytest.mark.parametrize("form", [WORKGROUP, WAVE])
def test_bad_block_stops_its_own_system(queue, form):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("n65b3")
    n = 65
    X0 = np.zeros_like(B)
    X0[1] = SENTINEL / 3 + np.arange(n)  # system 1's guess: must come back untouched
    # JACOBI: a_21,21 of system 1 negated, the first pivot of block 7
    e = int(rp[21] + np.nonzero(cl[rp[21]:rp[22]] == 21)[0][0])
    v2 = vals.copy()
    v2[1, e] = -v2[1, e]
    with BMany(queue, rp, cl, v2) as m:
        m.set_form(form)
        m.set_block(S.JACOBI, bs)
        out = m.psolve(B, X0=X0, tol=tol, max_workgroups=1)  # one workgroup runs all three
        _assert_refused_alone(out, X0, references(queue, "n65b3", "jacobi"))
        out = m.psolve(B, X0=X0, tol=tol)
        _assert_refused_alone(out, X0, references(queue, "n65b3", "jacobi"))
    # GIVEN: a NaN off the diagonal, and a W[i, i] that is not positive, in system 1
    for at, value in (((1, 22, 0), np.nan), ((1, 22, 1), 0.0), ((1, 64, 1), -1.0)):
        W = S.precond("n65b3", S.GIVEN).copy()
        W[at] = value  # row 22 is row 1 of block 7; row 64 row 1 of the partial block
        with BMany(queue, rp, cl, vals) as m:
            m.set_form(form)
            m.set_block(S.GIVEN, bs, W)
            out = m.psolve(B, X0=X0, tol=tol, max_workgroups=1)
            _assert_refused_alone(out, X0, references(queue, "n65b3", "given"))
    # the columns past the partial block are not read
    W = S.precond("n65b3", S.GIVEN).copy()
    W[:, 63:, 2] = np.nan
    with BMany(queue, rp, cl, vals) as m:
        m.set_form(form)
        m.set_block(S.GIVEN, bs, W)
        assert_systems_equal(m.psolve(B, tol=tol), references(queue, "n65b3", "given"))


def test_nan_in_b_stays_in_its_system(queue):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("multi11")
    refs = references(queue, "multi11", "jacobi")
    B = B.copy()
    B[2, 5] = np.nan
    with BMany(queue, rp, cl, vals) as m:
        m.set_form(WORKGROUP)
        m.set_block(S.JACOBI, bs)
        out = m.psolve(B, tol=tol, max_workgroups=2)  # it shares a workgroup with others
    assert_systems_equal(out, refs, which=[s for s in range(11) if s != 2])
    ref = single(queue, rp, cl, vals[2], B[2], None, tol, -1, S.JACOBI, bs, None)
    assert np.isnan(ref[2]) and ref[3] == 1
    assert_systems_equal((out[0][2:3], out[1][2:3], out[2][2:3], out[3][2:3], None, None,
                          out[6][2:3]), [ref])


def test_values_overwritten_in_place_and_the_python_class(queue):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("n257b3")
    refs = references(queue, "n257b3", "jacobi")
    m = cga.ManyCG(queue, rp, cl, vals)
    try:
        m.set_block_preconditioner(cga.BlockPreconditioner.Jacobi, bs)
        X = m.solve(B, improvement=tol)
        assert m.info()[1] == 2 and m.info()[2] == (2 * 2 * 256 + 8 + 32) * 8
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz), refs)
        # system s now takes the values of system 2 - s: W must follow
        m.set_values(vals[::-1])
        X = m.solve(B, improvement=tol)
        swapped = [single(queue, rp, cl, vals[2 - s], B[s], None, tol, -1, S.JACOBI, bs, None)
                   for s in range(3)]
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz), swapped)
        assert not np.array_equal(X[1], X[1] * 0) and not np.array_equal(X[0], refs[0][0])
        # block_inv, and its W moved in as Given: the same bits as Jacobi
        m.set_values(vals)
        W, bad = m.block_inv(bs)
        assert W.shape == (3, 257, bs) and len(bad) == 0
        np.testing.assert_array_equal(W, S.precond("n257b3", S.JACOBI))
        m.set_block_preconditioner(cga.BlockPreconditioner.Given, bs, W)
        X = m.solve(B, improvement=tol)
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz), refs)
        # the caller's blocks, flat; then the diagonal one replaces it, then none
        m.set_block_preconditioner(2, bs, S.precond("n257b3", S.GIVEN).reshape(3, -1))
        X = m.solve(B, improvement=tol)
        assert_systems_equal((X, m.bodies, m.rxr, m.stopped, None, None, m.rz),
                             references(queue, "n257b3", "given"))
        m.set_preconditioner(cga.Preconditioner.Jacobi)
        m.solve(B, improvement=tol)
        assert (m.bodies > np.array([r[1] for r in refs])).all() and m.rz is not None
        m.set_block_preconditioner(cga.BlockPreconditioner.Jacobi, bs)
        m.set_block_preconditioner(cga.BlockPreconditioner.None_)
        m.solve(B, improvement=tol)
        assert m.rz is None
    finally:
        m.close()


def test_switching_between_solves_and_the_exclusion(queue):
    rp, cl, vals, B, tol, _, _, bs = S.system_set("n257b3")
    refs = references(queue, "n257b3", "jacobi")
    with BMany(queue, rp, cl, vals) as m:
        assert m.kinds() == (P.NONE, S.NONE, 0)
        first = m.solve(B, tol=tol)
        m.set_diag(P.JACOBI)
        assert m.kinds() == (P.JACOBI, S.NONE, 0)
        jac = m.psolve(B, tol=tol)
        m.set_block(S.JACOBI, bs)
        assert m.kinds() == (P.NONE, S.JACOBI, bs)  # get_precond reports NONE under a block one
        assert lib().cgx_many_rz(m.h, (C.c_double * 3)()) == ESTATE  # no solve under it yet
        blk = m.psolve(B, tol=tol)
        m.set_diag(P.JACOBI)  # replaces the block one
        assert m.kinds() == (P.JACOBI, S.NONE, 0)
        jac2 = m.psolve(B, tol=tol)
        m.set_block(S.JACOBI, 5)
        m.set_diag(P.NONE)  # and so does NONE
        assert m.kinds() == (P.NONE, S.NONE, 0)
        m.set_diag(P.JACOBI)
        m.set_block(S.NONE)  # and the block NONE the diagonal one
        assert m.kinds() == (P.NONE, S.NONE, 0)
        assert lib().cgx_many_rz(m.h, (C.c_double * 3)()) == ESTATE
        last = m.solve(B, tol=tol)
    assert_systems_equal(blk, refs)
    for a, b in zip(first[:4], last[:4]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(jac[:4] + jac[6:], jac2[:4] + jac2[6:]):
        np.testing.assert_array_equal(a, b)
    assert (blk[1] < jac[1]).all()


def test_many_block_pcg_check_example():
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "agree bit for bit" in r.stdout and "fewer bodies" in r.stdout
