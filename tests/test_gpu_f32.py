"""The T = float instantiation of the engine, bit for bit.

The f32 kernels are the f64 templates with other shapes: the update kernels
walk float2 pairs (n >> 1 pairs and an odd-n tail), clamp their first loads
onto a slack element at n = 1, run a 4-deep unrolled trip before a strided
remainder, and switch to non-temporal loads and stores above 8,388,608
elements (twice the f64 threshold). Everything here is an equality:

  - the vector operations against numpy's f32 expressions with rounded
    products; dot_acc / norm_acc on integer inputs whose sum is exact in any
    order (one random-valued case per size carries the file's only tolerance,
    the bound that holds for any summation order);
  - SpMV on every row against tests/cg_model.spmv;
  - the CG loop (x after every body, every r.r and r.z, the body count)
    against tests/cg_model.cg: the exact-dot model, which
    tests/test_cg_model_cpu.py pins to the f64 oracle. Where a dot's exact sum
    lies within the documented accuracy of the double-length sums of a
    rounding boundary the model branches (at most 8 trajectories per case,
    asserted on the CPU), and the device must be one of them.

Division and square root: alpha, beta and the stop rule's sqrt are f32
operations in the kernels, correctly rounded as hipcc compiles them without
fast-math; the model uses numpy's.
"""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import DeviceArray, Matrix, Scalar, Vector, VectorOperations
from conjugategradient_amd import _native as N
from conjugategradient_amd._native import check, lib
from tests import cg_model
from tests.test_cg_model_cpu import CASES, KVL, inputs, model
from tests.util import irregular_spd

pytestmark = pytest.mark.gpu

F32 = np.float32
EUNSUPPORTED = 6
SIZES = [1, 2, 3, 255, 256, 257, 4097, 100_001]


def _ops(queue, n):
    ops = VectorOperations(queue, F32)
    ops.setVectorSize(n)
    return ops


def _vec(queue, a):
    return Vector(queue, a, dtype=F32)


# ---------------------------------------------------------------------------
# vector operations

@pytest.mark.parametrize("n", SIZES)
def test_axpy_family_bitexact(queue, n):
    rng = np.random.default_rng(11 + n)
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    a, b = F32(0.7310585786300049), F32(-1.3862943611198906)
    ops = _ops(queue, n)
    xv, yv, rv = _vec(queue, x), _vec(queue, y), Vector(queue, n, dtype=F32)
    sa, sb = Scalar(queue, a, F32), Scalar(queue, b, F32)
    want = {"sapbx": x + b * y, "sambx": x - b * y, "saxpby": a * x + b * y}
    assert all(w.dtype == F32 for w in want.values())
    ops.sapbx(xv, yv, sb, rv)
    np.testing.assert_array_equal(rv.to_numpy(), want["sapbx"])
    ops.sambx(xv, yv, sb, rv)
    np.testing.assert_array_equal(rv.to_numpy(), want["sambx"])
    ops.saxpby(xv, yv, sa, sb, rv)
    np.testing.assert_array_equal(rv.to_numpy(), want["saxpby"])
    for name in want:  # in place: res = x, then res = y (fresh operands each time)
        xa, ya = _vec(queue, x), _vec(queue, y)
        args = (xa, ya, sa, sb) if name == "saxpby" else (xa, ya, sb)
        getattr(ops, name)(*args, xa)
        np.testing.assert_array_equal(xa.to_numpy(), want[name], err_msg=f"{name}, res = x")
        np.testing.assert_array_equal(ya.to_numpy(), y)
        xa = _vec(queue, x)
        args = (xa, ya, sa, sb) if name == "saxpby" else (xa, ya, sb)
        getattr(ops, name)(*args, ya)
        np.testing.assert_array_equal(ya.to_numpy(), want[name], err_msg=f"{name}, res = y")
        np.testing.assert_array_equal(xa.to_numpy(), x)


@pytest.mark.parametrize("num,den", [(1.0, 3.0), (7.0, 2.0), (0.1, 0.7), (-5.0, 1e-30), (0.0, 0.0)])
def test_scalar_div_bitexact(queue, num, den):
    sn, sd, so = Scalar(queue, num, F32), Scalar(queue, den, F32), Scalar(queue, 9.0, F32)
    check(lib().cgx_scalar_div(queue.handle, N.F32, sn.ptr(), sd.ptr(), so.ptr()))
    with np.errstate(all="ignore"):
        want = F32(num) / F32(den)
    got = so._v.download()[0]
    if (num, den) == (1.0, 3.0):  # an inexact quotient: not the f64 quotient
        assert float(want) != 1.0 / 3.0
    np.testing.assert_array_equal(got, want)
    assert got.dtype == F32


@pytest.mark.parametrize("n", SIZES)
def test_fill_every_element(queue, n):
    d = DeviceArray(queue, n + 2, F32)
    d.upload(np.full(n + 2, 7.0, F32))
    check(lib().cgx_fill(queue.handle, N.F32, d.ptr, 0.1, n))
    got = d.download()
    np.testing.assert_array_equal(got[:n], np.full(n, F32(0.1)))
    np.testing.assert_array_equal(got[n:], [7.0, 7.0])  # nothing past n


def _iota(queue, n, offset):
    d = DeviceArray(queue, n, F32)
    check(lib().cgx_iota(queue.handle, N.F32, d.ptr, n, float(offset)))
    return d.download()


def test_iota_every_element(queue):
    n = 4097
    want = (np.arange(n, dtype=np.float64) + 1 + 0.5).astype(F32)
    np.testing.assert_array_equal(_iota(queue, n, 0.5), want)


def test_iota_where_f32_rounds(queue):
    n = (1 << 24) + 9  # i + 1 needs 25 bits at the end: b_i = fl32(i + 1)
    want = (np.arange(n, dtype=np.float64) + 1 + 0.0).astype(F32)
    assert (want[-8:].astype(np.float64) != np.arange(n - 8, n) + 1.0).any()
    np.testing.assert_array_equal(_iota(queue, n, 0.0), want)


DOT_SIZES = [1, 2, 3, 255, 256, 257, 4097, 100_001, 1_000_003]


@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_and_norm_accumulate_exact_on_integers(queue, n):
    """k_dot_acc is a plain f32 sum in grid order. With x_i, y_i integers in
    [-3, 3] every product and every partial sum is an integer below 9 n + 5 <
    2^24, so exact in any order: one dropped or doubled element shows."""
    rng = np.random.default_rng(n)
    x = rng.integers(-3, 4, n).astype(F32)
    y = rng.integers(-3, 4, n).astype(F32)
    assert 9 * n + 5 < 1 << 24
    ops = _ops(queue, n)
    xv, yv = _vec(queue, x), _vec(queue, y)
    s = Scalar(queue, 5.0, F32)  # accumulate semantics (Q4)
    ops.dot_product_trivial(xv, yv, s)
    assert s.get() == 5 + int(np.dot(x.astype(np.int64), y.astype(np.int64)))
    ops.dot_product_trivial(xv, yv, s)  # ... and again on top
    assert s.get() == 5 + 2 * int(np.dot(x.astype(np.int64), y.astype(np.int64)))
    s2 = Scalar(queue, -4.0, F32)
    ops.norm(xv, s2)
    assert s2.get() == -4 + int(np.dot(x.astype(np.int64), x.astype(np.int64)))


@pytest.mark.parametrize("n", DOT_SIZES)
def test_dot_and_norm_accumulate_random_any_order_bound(queue, n):
    """The bound of a recursive sum in ANY order (Higham, Accuracy and
    Stability, 4.2: (n - 1) u sum|t_i| to first order) plus one rounding per
    product and one for the final add onto *res: (n + 2) u (|init| + sum |x_i
    y_i|), u = 2^-24."""
    rng = np.random.default_rng(n + 1)
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    ops = _ops(queue, n)
    xv, yv = _vec(queue, x), _vec(queue, y)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for init, a, b, run in ((5.0, x64, y64, lambda s: ops.dot_product_trivial(xv, yv, s)),
                            (0.25, x64, x64, lambda s: ops.norm(xv, s))):
        s = Scalar(queue, init, F32)
        run(s)
        want = init + float(np.sum(a * b))
        bound = (n + 2) * 2.0 ** -24 * (abs(init) + float(np.sum(np.abs(a * b))))
        print(f"n = {n}: |got - want| = {abs(s.get() - want):.3e}, bound {bound:.3e}")
        assert abs(s.get() - want) <= bound


# ---------------------------------------------------------------------------
# SpMV, every row

def _spmv(queue, m, x):
    n = m.N()
    y = Vector(queue, n, dtype=F32)
    _ops(queue, n).spmv(m, _vec(queue, x), y, m.NNZ(), count=n)
    return y.to_numpy()


def _variant(m):
    v = C.c_int()
    check(lib().cgx_csr_variant(m.schedule(), C.byref(v)))
    return v.value


@pytest.fixture(scope="module")
def irregular():
    rp, cl, vl = irregular_spd(50_000, seed=3)
    n = len(rp) - 1
    assert np.diff(rp).max() <= 2042  # no row long enough for the tree path
    x = np.random.default_rng(7).standard_normal(n).astype(F32)
    # non-finite and signed-zero values at a few rows
    x[[0, 1, 777, n // 2, n - 2, n - 1]] = [np.inf, -0.0, np.nan, -np.inf, 0.0, -0.0]
    v32 = vl.astype(F32)
    return rp, cl, v32, x, cg_model.spmv(rp, cl, v32, x)


@pytest.mark.parametrize("variant", [None, 0, 5, 13, 15, 133], ids=lambda v: f"v{v}")
def test_spmv_irregular_every_row(queue, irregular, variant):
    rp, cl, v32, x, want = irregular
    m = Matrix(queue, v32, cl, rp, dtype=F32)
    if variant is not None:
        check(lib().cgx_csr_set_variant(m.schedule(), variant))
        if variant:
            assert _variant(m) == variant
    assert np.isnan(want).any() and np.isinf(want).any()
    np.testing.assert_array_equal(_spmv(queue, m, x), want, err_msg=f"variant {_variant(m)}")


def test_spmv_poisson_and_single_row(queue, oracle):
    rp, cl, vl = oracle.poisson(2, 128, 128, 1)
    x = np.random.default_rng(2).standard_normal(len(rp) - 1).astype(F32)
    m = Matrix(queue, vl, cl, rp, dtype=F32)
    np.testing.assert_array_equal(_spmv(queue, m, x), cg_model.spmv(rp, cl, vl.astype(F32), x))
    rp, cl, vl = np.array([0, 3], np.int32), np.array([0, 0, 0], np.int32), np.ones(3)
    x = np.array([0.1], F32)
    m = Matrix(queue, vl, cl, rp, dtype=F32)
    want = cg_model.spmv(rp, cl, vl.astype(F32), x)
    assert want[0] == (F32(0.1) + F32(0.1)) + F32(0.1)
    np.testing.assert_array_equal(_spmv(queue, m, x), want)


# ---------------------------------------------------------------------------
# the loop

def _matrix(queue, name, monkeypatch):
    c = inputs(name)
    mat, extras = CASES[name][0], CASES[name][5]
    if "lean" in extras:  # the walk forced at creation (its first grid candidate)
        monkeypatch.setenv("CGX_SPMV_VARIANT", f"{KVL}:0")
    if mat[0] == "poisson" and len(c["b"]) > 100_000:  # generated on the device
        m = Matrix.poisson(queue, *mat[1:], dtype=F32)
        assert m.N() == len(c["b"]) and m.NNZ() == len(c["vl"])
    else:
        m = Matrix(queue, c["vl"], c["cl"], c["rp"], dtype=F32)
    if "lean" in extras:
        assert _variant(m) & KVL
    return m


def _x0(queue, c):
    n = len(c["b"])
    return _vec(queue, np.zeros(n, F32) if c["x0"] is None else c["x0"])


def _stepwise(queue, m, c, mode, jacobi):
    """begin, then run(1) until the solver stops: x, r.r (and r.z) after
    every body. -> (bodies, [r.r], [r.z], [x]) or the refusal of the mode."""
    L = lib()
    h = C.c_void_p()
    check(L.cgx_cg_create(queue.handle, m.schedule(), C.byref(h)))
    try:
        rc = L.cgx_cg_set_mode(h, mode)
        if rc:
            return rc, L.cgx_last_error().decode()
        if jacobi:
            check(L.cgx_cg_set_precond(h, cga.Preconditioner.Jacobi, None))
        bv, xv = _vec(queue, c["b"]), _x0(queue, c)
        check(L.cgx_cg_begin(h, bv.ptr(), xv.ptr(), c["tol"], c["cap"]))
        tot, st, val = C.c_int64(0), C.c_int(0), C.c_double(0)
        rr, rz, xs = [], [], []
        limit = len(c["b"]) + 1
        while not st.value and tot.value < limit:
            check(L.cgx_cg_run(h, 1, C.byref(tot), C.byref(st)))
            assert tot.value == len(rr) + 1
            check(L.cgx_cg_rxr(h, C.byref(val)))
            rr.append(val.value)
            if jacobi:
                check(L.cgx_cg_rz(h, C.byref(val)))
                rz.append(val.value)
            xs.append(xv.to_numpy())
        assert st.value in (1, 2)
        return tot.value, rr, rz, xs
    finally:
        L.cgx_cg_destroy(h)


def _solve(queue, m, c, mode, jacobi, graph, poll):
    cg = cga.CG(queue, F32)
    cg.mode, cg.use_graph, cg.poll_every = mode, graph, poll
    cg.setMatrix(m)
    cg.setTarget(_vec(queue, c["b"]))
    cg.setInitial(_x0(queue, c))
    if jacobi:
        cg.setPreconditioner(cga.Preconditioner.Jacobi)
    cg.solve(c["tol"], max_iter=c["cap"])
    return cg.extract(), cg.iterations, cg.final_rxr, cg.final_rz


def _same(a, b):
    """Equality of f32 scalars / sequences / arrays, NaNs in equal places equal."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def _report(runs, bodies, rr, rz, xs):
    """Where the device left the model: against the trajectory it follows
    longest, the first body whose r.r (r.z, x) differs and how many elements
    of the final x do: which launch of which body to read."""
    def first(a, b):
        k = 0
        while k < min(len(a), len(b)) and _same(a[k], b[k]):
            k += 1
        return k
    best = max(runs, key=lambda cr: first(rr, cr[1].rr))
    ch, run = best
    out = [f"no trajectory of {len(runs)} matches; closest is choices {ch}: bodies {bodies} "
           f"(model {run.bodies})"]
    k = first(rr, run.rr)
    if k < max(len(rr), len(run.rr)):
        out.append(f"first body whose r.r differs: {k + 1} (device {rr[k] if k < len(rr) else None!r}, "
                   f"model {float(run.rr[k]) if k < len(run.rr) else None!r})")
    if rz:
        k = first(rz, run.rz)
        if k < max(len(rz), len(run.rz)):
            out.append(f"first body whose r.z differs: {k + 1}")
    if xs:
        k = first(xs, run.xs)
        if k < max(len(xs), len(run.xs)):
            out.append(f"first body whose x differs: {k + 1} "
                       f"({int(np.count_nonzero(xs[k] != run.xs[k])) if k < min(len(xs), len(run.xs)) else '-'} elements)")
        if xs[-1].shape == run.x.shape:
            out.append(f"elements of the final x that differ: "
                       f"{int(np.count_nonzero(~((xs[-1] == run.x) | (np.isnan(xs[-1]) & np.isnan(run.x)))))}"
                       f" of {run.x.size}")
    return "; ".join(out)


LOOP = [(name, mode) for name in CASES for mode in CASES[name][1]]


@pytest.mark.parametrize("name,mode", LOOP, ids=[f"{n}-mode{m}" for n, m in LOOP])
def test_loop_is_a_model_trajectory_bit_for_bit(queue, monkeypatch, name, mode):
    c = inputs(name)
    jacobi = "jacobi" in CASES[name][5]
    m = _matrix(queue, name, monkeypatch)
    if jacobi:  # the model's m is the device's
        np.testing.assert_array_equal(m.diag_inv(), c["minv"])
    step = _stepwise(queue, m, c, mode, jacobi)
    if len(step) == 2:  # the mode refused: only mode 2, only for want of a fused kernel
        rc, msg = step
        assert mode == 2 and rc == EUNSUPPORTED, (rc, msg)
        assert "mode 2 needs a production SpMV format" in msg, msg
        print(f"{name}: mode 2 is unsupported for variant {_variant(m)}: {msg}")
        return
    bodies, rr, rz, xs = step
    runs = model(name)
    hit = [ch for ch, run in runs
           if run.bodies == bodies and _same(rr, run.rr) and _same(rz, run.rz)
           and all(_same(a, b) for a, b in zip(xs, run.xs))]
    assert hit, _report(runs, bodies, rr, rz, xs)
    # (two trajectories can be equal in everything observable: a quotient
    # often rounds the same for both neighbours of an unclear p.Ap)
    run = dict(runs)[hit[0]]
    assert xs[-1].dtype == F32
    np.testing.assert_array_equal(xs[-1], run.x)
    print(f"{name} mode {mode}: {bodies} bodies, trajectory {hit} of {len(runs)} "
          f"({len(run.unclear)} dots not clear)")
    # one uninterrupted solve (graph replay, default poll), and eager launches polled every 4
    for graph, poll in ((True, 32), (False, 4)):
        x, k, rxr, rzz = _solve(queue, m, c, mode, jacobi, graph, poll)
        what = f"solve(graph={graph}, poll={poll})"
        assert k == bodies, what
        assert _same(x, xs[-1]), f"{what}: {int(np.count_nonzero(x != xs[-1]))} elements of x differ"
        assert _same(rxr, rr[-1]), what
        if jacobi:
            assert _same(rzz, rz[-1]), what

