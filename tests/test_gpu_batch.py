"""Batched CG (cgx_cg_solve_batch): k independent solves on one
matrix, the fused form serving every column from one pass over the CSR arrays.

Every expected value is a single-RHS solve in mode 1 through the C ABI
(cgx_cg_begin / cgx_cg_run on the column's own b and x0), or
oracle.cg_solve_dd; never the batch itself. The comparison is bit for bit:
each column keeps the single kernels' per-element expressions and per-row sum
order, and the two dots are double-length sums whose rounded value does not
depend on how rows are dealt to threads (cgx_dd.h).

Columns (rng = default_rng(21)): i + 1, 1e-3 N(0,1), 1e3 N(0,1), N(0,1), then
further N(0,1) columns up to 8. Under tol = 1e-6 the first four stop at
different bodies, far below the cap (CPU run of the same loop):
irregular_spd(4097, hub=300, seed=3) 230 / 130 / 231 / 183 (the engine, with
its double-length dots: 229 / 131 / 232 / 184),
irregular_spd(20000, seed=5, hub=5000) 237 / 123 / 222 / 176,
16^3 Poisson 68 / 45 / 79 / 62.

Sizes are the smallest at which the kernels can go wrong: 4,097 rows are 17+
row blocks (more than one workgroup, a last block of one row), roughly every
other block starts at an odd entry (the paired loads' element before k0), the
300-entry hub row fills most of a block, the 5,000-entry hub row is longer
than a tile, and k = 1, 3, 5 are not instantiated widths (2, 4, 8).
"""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests.util import irregular_spd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "batch_check")
EINVAL, EUNSUPPORTED = 1, 6
SENTINEL = -7.25e11


def columns(n, k=8):
    rng = np.random.default_rng(21)
    cols = [np.arange(1, n + 1, dtype=np.float64), 1e-3 * rng.standard_normal(n),
            1e3 * rng.standard_normal(n), rng.standard_normal(n)]
    cols += [rng.standard_normal(n) for _ in range(4)]
    return np.stack(cols[:k], axis=1)


@functools.lru_cache(maxsize=None)
def host_matrix(name):
    if name == "irr":
        return irregular_spd(4097, hub=300, seed=3)
    if name == "hub":
        return irregular_spd(20000, seed=5, hub=5000)
    if name == "c16":
        return irregular_spd(6001, seed=9)
    if name.startswith("dense"):
        n = int(name[5:])
        m = np.random.default_rng(100 + n).standard_normal((n, n))
        a = m @ m.T + n * np.eye(n)
        rp = np.arange(0, n * n + 1, n, dtype=np.int32)
        cl = np.tile(np.arange(n, dtype=np.int32), n)
        return rp, cl, a.ravel().copy()
    raise KeyError(name)


_matrices = {}


def device_matrix(queue, name, variant=0):
    """One device matrix per (name, forced variant), shared by the tests."""
    key = (name, variant)
    if key not in _matrices:
        if name == "p3d":
            m = cga.Matrix.poisson(queue, 3, 16, 16, 16)
        else:
            rp, cl, vl = host_matrix(name)
            m = cga.Matrix(queue, vl, cl, rp)
        if variant:
            check(lib().cgx_csr_set_variant(m.schedule(), variant))
            got = C.c_int()
            check(lib().cgx_csr_variant(m.schedule(), C.byref(got)))
            assert got.value == variant
        _matrices[key] = m
    return _matrices[key]


class Solver:
    """A cgx_cg on a matrix, driven through the C ABI."""

    def __init__(self, queue, m, dtype=np.float64, mode=1, poll_every=0, use_graph=-1):
        self.queue, self.m, self.dtype = queue, m, np.dtype(dtype)
        self.n = m.N()
        h = C.c_void_p()
        check(lib().cgx_cg_create(queue.handle, m.schedule(), C.byref(h)))
        self.h = h
        check(lib().cgx_cg_set_mode(h, mode))
        check(lib().cgx_cg_config(h, poll_every, use_graph))

    def close(self):
        if self.h:
            lib().cgx_cg_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def single(self, b, x0=None, tol=0.0, max_iter=-1):
        """(x, bodies, rxr, stopped) of cgx_cg_begin / cgx_cg_run on one column."""
        n = self.n
        db = cga.DeviceArray(self.queue, n, self.dtype).upload(b)
        dx = cga.DeviceArray(self.queue, n, self.dtype).upload(np.zeros(n) if x0 is None else x0)
        check(lib().cgx_cg_begin(self.h, db.ptr, dx.ptr, tol, max_iter))
        cap = n + 1 if max_iter < 0 else min(n + 1, max(max_iter, 1))
        total, stopped, rxr = C.c_int64(), C.c_int(), C.c_double()
        check(lib().cgx_cg_run(self.h, cap, C.byref(total), C.byref(stopped)))
        check(lib().cgx_cg_rxr(self.h, C.byref(rxr)))
        return dx.download(), total.value, rxr.value, stopped.value

    def upload(self, M, ld):
        """Column-major device block with leading dimension ld, gaps = SENTINEL."""
        n, k = M.shape
        host = np.full((k, ld), SENTINEL, dtype=self.dtype)
        host[:, :n] = M.T
        return cga.DeviceArray(self.queue, k * ld, self.dtype).upload(host.ravel())

    def download(self, d, k, ld):
        host = d.download().reshape(k, ld)
        return np.ascontiguousarray(host[:, : self.n].T), host[:, self.n:]

    def batch_rc(self, B, X0=None, tol=0.0, max_iter=-1, form=1, ld=None, k=None, ldarg=None):
        """The return code of cgx_cg_solve_batch and its outputs."""
        n, kk = B.shape
        ld = n if ld is None else ld
        dB = self.upload(B, ld)
        dX = self.upload(np.zeros_like(B) if X0 is None else X0, ld)
        check(lib().cgx_cg_set_batch_form(self.h, form))
        k = kk if k is None else k
        bodies, rxr, stopped = (C.c_int64 * 8)(), (C.c_double * 8)(), (C.c_int * 8)()
        lda = ld if ldarg is None else ldarg
        rc = lib().cgx_cg_solve_batch(self.h, k, dB.ptr, lda, dX.ptr, lda, tol, max_iter, bodies,
                                      rxr, stopped)
        if rc:
            return rc, None
        X, gapx = self.download(dX, kk, ld)
        _, gapb = self.download(dB, kk, ld)
        return 0, (X, np.array(bodies[:kk]), np.array(rxr[:kk]), np.array(stopped[:kk]), gapx, gapb)

    def batch(self, B, **kw):
        rc, out = self.batch_rc(B, **kw)
        assert rc == 0, lib().cgx_last_error()
        return out

    def info(self, form=None):
        if form is not None:
            check(lib().cgx_cg_set_batch_form(self.h, form))
        f, w = C.c_int(), C.c_int()
        check(lib().cgx_cg_batch_info(self.h, C.byref(f), C.byref(w)))
        return f.value, w.value


_refs = {}


def reference(queue, name, variant, tol, max_iter, k=8, x0col=None):
    """The single mode-1 solves of the first k standard columns, computed once
    per (matrix, tol, cap) on a solver of their own and shared."""
    key = (name, variant, tol, max_iter)
    m = device_matrix(queue, name, variant)
    if key not in _refs:
        _refs[key] = {}
    have = _refs[key]
    B = columns(m.N())
    missing = [c for c in range(k) if c not in have]
    if missing:
        with Solver(queue, m) as s:
            for c in missing:
                have[c] = s.single(B[:, c], None, tol, max_iter)
    return [have[c] for c in range(k)]


def assert_columns_equal(out, refs, cols=None):
    X, bodies, rxr, stopped = out[:4]
    for j, ref in enumerate(refs):
        if cols is not None and j not in cols:
            continue
        xr, kr, rr, sr = ref
        np.testing.assert_array_equal(X[:, j], xr, err_msg=f"column {j}: x")
        assert bodies[j] == kr, f"column {j}: bodies {bodies[j]} != {kr}"
        assert rxr[j] == rr or (np.isnan(rxr[j]) and np.isnan(rr)), \
            f"column {j}: r.r {rxr[j]!r} != {rr!r}"
        assert stopped[j] == sr, f"column {j}: stop code {stopped[j]} != {sr}"


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
def test_fused_bit_identity(queue, oracle, k):
    m = device_matrix(queue, "irr", 13)
    refs = reference(queue, "irr", 13, 0.0, 40, k)
    B = columns(m.N(), k)
    with Solver(queue, m) as s:
        out = s.batch(B, tol=0.0, max_iter=40)
        assert s.info() == (1, {1: 2, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8}[k])
    assert_columns_equal(out, refs)
    assert list(out[1]) == [40] * k and list(out[3]) == [2] * k
    if k == 4:
        rp, cl, vl = host_matrix("irr")
        for c in range(k):
            xo, res = oracle.cg_solve_dd(rp, cl, vl, B[:, c].copy(), 0.0, max_iter=40)
            assert res.iterations == 40
            np.testing.assert_array_equal(out[0][:, c], xo)


# 2 ---------------------------------------------------------------------------
def test_per_column_stop_and_freeze(queue):
    m = device_matrix(queue, "irr", 13)
    refs = reference(queue, "irr", 13, 1e-6, -1, 4)
    B = columns(m.N(), 4)
    with Solver(queue, m) as s:
        out = s.batch(B, tol=1e-6)
        assert_columns_equal(out, refs)
        counts = [int(b) for b in out[1]]
        print("stop bodies", counts)
        assert len(set(counts)) == 4 and max(counts) < m.N() // 4
        assert list(out[3]) == [1, 1, 1, 1]
        # the same solve through begin / run in pieces of 7 bodies
        n = m.N()
        dB, dX = s.upload(B, n), s.upload(np.zeros_like(B), n)
        check(lib().cgx_cg_begin_batch(s.h, 4, dB.ptr, n, dX.ptr, n, 1e-6, -1))
        total, done = (C.c_int64 * 8)(), C.c_int(0)
        frozen = {}
        pieces = 0
        while not done.value:
            check(lib().cgx_cg_run_batch(s.h, 7, total, C.byref(done)))
            pieces += 1
            assert pieces <= max(counts) // 7 + 2
            X, _ = s.download(dX, 4, n)
            for c in range(4):
                if c in frozen:  # stopped in an earlier piece: not touched since
                    np.testing.assert_array_equal(X[:, c], frozen[c])
                elif total[c] == counts[c] and total[c] < 7 * pieces:
                    frozen[c] = X[:, c].copy()
        assert [total[c] for c in range(4)] == counts
        for c in range(4):
            np.testing.assert_array_equal(X[:, c], refs[c][0])


# 3 ---------------------------------------------------------------------------
def test_nan_and_inf_stay_in_their_column(queue):
    m = device_matrix(queue, "irr", 13)
    refs = reference(queue, "irr", 13, 1e-6, -1, 5)
    n = m.N()
    B = columns(n, 5).copy()
    X0 = np.zeros_like(B)
    B[100, 1] = np.nan
    X0[7, 3] = np.inf
    with Solver(queue, m) as s:
        out = s.batch(B, X0=X0, tol=1e-6)
    # the NaN rule's stop code (CG.hpp:396-404 on a NaN r.r), long before the others stop
    assert out[3][1] == 1 and out[3][3] == 1
    print("bodies", list(out[1]))
    assert out[1][1] <= 3 and out[1][3] <= 3
    assert_columns_equal(out, refs, cols={0, 2, 4})


# 4 ---------------------------------------------------------------------------
def test_row_longer_than_a_tile(queue):
    m = device_matrix(queue, "hub", 13)
    assert np.diff(host_matrix("hub")[0]).max() > 2046
    refs = reference(queue, "hub", 13, 0.0, 30, 3)
    with Solver(queue, m) as s:
        out = s.batch(columns(m.N(), 3), tol=0.0, max_iter=30)
    assert_columns_equal(out, refs)


# 5 ---------------------------------------------------------------------------
def test_16_bit_column_deltas(queue):
    m = device_matrix(queue, "c16", 133)
    refs = reference(queue, "c16", 133, 0.0, 30, 3)
    with Solver(queue, m) as s:
        out = s.batch(columns(m.N(), 3), tol=0.0, max_iter=30)
    assert_columns_equal(out, refs)


# 6 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 257])
def test_tiny_systems(queue, n):
    name = f"dense{n}"
    m = device_matrix(queue, name)
    refs = reference(queue, name, 0, 1e-9, -1, 3)
    with Solver(queue, m) as s:
        out = s.batch(columns(n, 3), tol=1e-9)
    assert_columns_equal(out, refs)


# 7 ---------------------------------------------------------------------------
def test_other_spmv_families(queue):
    m = device_matrix(queue, "p3d")
    refs = reference(queue, "p3d", 0, 1e-6, -1, 4)
    B = columns(m.N(), 4)
    with Solver(queue, m) as s:
        assert s.info(0) == (2, 0)  # a SELL matrix: auto stays sequential
        assert_columns_equal(s.batch(B, tol=1e-6, form=1), refs)
        assert s.info() == (1, 4)
        assert_columns_equal(s.batch(B, tol=1e-6, form=2), refs)  # the solver is in mode 1
        out = s.batch(B, tol=1e-6, form=0)
        assert_columns_equal(out, refs)
        assert len(set(int(b) for b in out[1])) == 4
    # the sequential form in the solver's auto mode (what the Python and C++
    # layers run by default on this matrix): each column is that solver's own
    # single solve, bit for bit
    with Solver(queue, m, mode=0) as s:
        mode = C.c_int()
        check(lib().cgx_cg_get_mode(s.h, C.byref(mode)))
        assert mode.value != 1
        want = [s.single(B[:, c], None, 1e-6, -1) for c in range(3)]
        assert s.info(0) == (2, 0)
        assert_columns_equal(s.batch(B[:, :3], tol=1e-6, form=0), want)
    irr = device_matrix(queue, "irr", 13)
    with Solver(queue, irr) as s:
        assert s.info(0)[0] == 1  # a CSR-stream matrix: auto takes fused ...
        B = columns(irr.N(), 2)
        refs = reference(queue, "irr", 13, 0.0, 40, 2)
        assert_columns_equal(s.batch(B, tol=0.0, max_iter=40, form=0), refs)
        assert s.info() == (1, 2)
        # ... for two or more columns; one alone stays sequential (cgx.h)
        assert_columns_equal(s.batch(B[:, :1], tol=0.0, max_iter=40, form=0), refs[:1])
        assert s.info() == (2, 0)


# 8 ---------------------------------------------------------------------------
def test_leading_dimension_gaps(queue):
    m = device_matrix(queue, "irr", 13)
    refs = reference(queue, "irr", 13, 0.0, 40, 4)
    n = m.N()
    with Solver(queue, m) as s:
        out = s.batch(columns(n, 4), tol=0.0, max_iter=40, ld=n + 37)
    assert_columns_equal(out, refs)
    assert out[4].shape == (4, 37) and np.all(out[4] == SENTINEL) and np.all(out[5] == SENTINEL)
    # the sequential form on an odd ld: columns 1 and 3 are not 16-byte aligned
    # and go through its aligned copy
    with Solver(queue, m) as s:
        out = s.batch(columns(n, 4), tol=0.0, max_iter=40, ld=n + 38, form=2)
    assert_columns_equal(out, refs)
    assert out[4].shape == (4, 38) and np.all(out[4] == SENTINEL) and np.all(out[5] == SENTINEL)


# 9 ---------------------------------------------------------------------------
@pytest.mark.parametrize("poll_every,use_graph", [(1, 1), (32, 1), (32, 0), (5, 1)])
def test_chunking(queue, poll_every, use_graph):
    m = device_matrix(queue, "irr", 13)
    B = columns(m.N(), 3)
    for cap in (40, 41, 42, 43):  # runs that end in every slot
        refs = reference(queue, "irr", 13, 0.0, cap, 3)
        with Solver(queue, m, poll_every=poll_every, use_graph=use_graph) as s:
            assert_columns_equal(s.batch(B, tol=0.0, max_iter=cap), refs)


# 10 --------------------------------------------------------------------------
def test_refusals(queue):
    m = device_matrix(queue, "irr", 13)
    n = m.N()
    B = columns(n, 8)
    refs = reference(queue, "irr", 13, 0.0, 40, 2)
    with Solver(queue, m) as s:
        assert s.batch_rc(B[:, :1], k=0)[0] == EINVAL
        assert s.batch_rc(B, k=9)[0] == EINVAL
        assert s.batch_rc(B[:, :2], ldarg=n - 1)[0] == EINVAL
        check(lib().cgx_cg_set_precond(s.h, 1, None))  # Jacobi
        assert s.batch_rc(B[:, :2], form=1)[0] == EUNSUPPORTED
        assert b"preconditioner" in lib().cgx_last_error()
        with Solver(queue, m) as pc:  # the single preconditioned solves, mode 1
            check(lib().cgx_cg_set_precond(pc.h, 1, None))
            want = [pc.single(B[:, c], None, 1e-6, -1) for c in range(2)]
        assert_columns_equal(s.batch(B[:, :2], tol=1e-6, form=2), want)
        check(lib().cgx_cg_set_precond(s.h, 0, None))
        # begin / run are the fused form's
        check(lib().cgx_cg_set_batch_form(s.h, 2))
        dB, dX = s.upload(B[:, :2], n), s.upload(np.zeros((n, 2)), n)
        assert lib().cgx_cg_begin_batch(s.h, 2, dB.ptr, n, dX.ptr, n, 0.0, 40) == EUNSUPPORTED
        tot, done = (C.c_int64 * 8)(), C.c_int()
        assert lib().cgx_cg_run_batch(s.h, 1, tot, C.byref(done)) == EUNSUPPORTED
        assert_columns_equal(s.batch(B[:, :2], tol=0.0, max_iter=40, form=1), refs)
    m32 = cga.Matrix(queue, *[host_matrix("irr")[i] for i in (2, 1, 0)], dtype=np.float32)
    with Solver(queue, m32, dtype=np.float32) as s:
        assert s.batch_rc(B[:, :2].astype(np.float32), form=1)[0] == EUNSUPPORTED
        assert b"f32" in lib().cgx_last_error()
        rc, out = s.batch_rc(B[:, :2].astype(np.float32), tol=0.0, max_iter=10, form=2)
        assert rc == 0 and list(out[1]) == [10, 10]


def test_single_and_batch_interleave(queue):
    m = device_matrix(queue, "irr", 13)
    B = columns(m.N(), 3)
    refs = reference(queue, "irr", 13, 0.0, 40, 3)
    with Solver(queue, m) as s:
        first = s.batch(B, tol=0.0, max_iter=40)
        one = s.single(B[:, 1], None, 0.0, 40)  # a single solve after a batch
        np.testing.assert_array_equal(one[0], refs[1][0])
        assert one[1:] == refs[1][1:]
        again = s.batch(B, tol=0.0, max_iter=40)  # a batch after a single solve
        assert_columns_equal(again, refs)
        np.testing.assert_array_equal(again[0], first[0])
        # a batch call ends the single solve: cgx_cg_run needs a new begin
        total, stopped = C.c_int64(), C.c_int()
        assert lib().cgx_cg_run(s.h, 1, C.byref(total), C.byref(stopped)) != 0
        # and cgx_cg_begin ends the batch
        s.single(B[:, 0], None, 0.0, 3)
        tot = (C.c_int64 * 8)()
        assert lib().cgx_cg_run_batch(s.h, 1, tot, C.byref(stopped)) != 0


# 11 --------------------------------------------------------------------------
def test_python_layer(queue, monkeypatch):
    monkeypatch.setenv("CGX_SPMV_VARIANT", "13")
    rp, cl, vl = host_matrix("irr")
    refs = reference(queue, "irr", 13, 0.0, 40, 3)
    B = columns(len(rp) - 1, 3)
    cg = cga.CG(queue)
    cg.setMatrix(vl, cl, rp)
    cg.batch_form = 1
    Xc = cg.solve_batch(np.ascontiguousarray(B), improvement=0.0, max_iter=40)
    assert cg.batch_info() == (1, 4)
    Xf = cg.solve_batch(np.asfortranarray(B), improvement=0.0, max_iter=40)
    np.testing.assert_array_equal(Xc, Xf)
    assert Xc.shape == B.shape
    for c in range(3):
        np.testing.assert_array_equal(Xc[:, c], refs[c][0])
    assert list(cg.iterations_batch) == [40, 40, 40] and list(cg.stopped_batch) == [2, 2, 2]
    assert list(cg.final_rxr_batch) == [r[2] for r in refs]
    X0 = 0.5 * columns(len(rp) - 1, 3)[:, ::-1]
    with Solver(queue, device_matrix(queue, "irr", 13)) as s:
        want = [s.single(B[:, c], X0[:, c], 0.0, 10)[0] for c in range(3)]
    got = cg.solve_batch(B, X0=X0, max_iter=10)
    for c in range(3):
        np.testing.assert_array_equal(got[:, c], want[c])


def test_cpp_layer(queue, tmp_path):
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)
    rp, cl, vl = host_matrix("irr")
    n, k = len(rp) - 1, 3
    B = columns(n, k)
    # the C++ layer's matrix keeps its production variant: the reference too
    refs = reference(queue, "irr", 0, 1e-6, -1, k)
    inp, out = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(inp, "wb") as f:
        np.array([n, len(vl), k, -1], np.int64).tofile(f)
        rp.astype(np.int32).tofile(f)
        cl.astype(np.int32).tofile(f)
        vl.astype(np.float64).tofile(f)
        np.ascontiguousarray(B.T).tofile(f)
        np.array([1e-6], np.float64).tofile(f)
    p = subprocess.run([EXE, str(inp), str(out), "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = np.fromfile(out, np.float64).reshape(k, 3 + n)
    for c in range(k):
        xr, kr, rr, sr = refs[c]
        assert (int(res[c, 0]), res[c, 1], int(res[c, 2])) == (kr, rr, sr)
        np.testing.assert_array_equal(res[c, 3:], xr)
