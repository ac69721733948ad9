"""The mixed-precision solve (cgx_mixed) on the device, bit for
bit against tests/mixed_model.py: x, every history record (the f64 r.r, the
inner bodies, the inner solve's final f32 r.r), the outer count, the body count
and the status must be those of one trajectory of the model (the model
branches where a dot's exact sum lies within the double-length sums' accuracy
of a rounding boundary; tests/test_mixed_cpu.py holds every case to at most 8
trajectories). Everything here is an equality.

The cases come from tests/test_mixed_cpu.CASES: the table's systems in inner
modes 1 and 3, a caller's diagonal, a non-zero x0, the dense systems, the
lean walk's size in inner auto mode, the four statuses, the kernels' tails
(n = 1, 3, 5, 1,023 with an odd nnz, one inner body) and a right-hand side
whose scaled components reach into the f32 subnormals.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import Matrix, Vector
from conjugategradient_amd._native import check, lib
from tests.test_cg_model_cpu import KVL
from tests.test_mixed_cpu import CASES, inputs, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "examples", "mixed_check")
EINVAL, EUNSUPPORTED = 1, 6
F32 = np.float32


class Mixed:
    """A cgx_mixed handle on a device Matrix."""

    def __init__(self, queue, m):
        self.q, self.m = queue, m
        self.h = C.c_void_p()
        check(lib().cgx_mixed_create(queue.handle, m.schedule(), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().cgx_mixed_destroy(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def inner_mode(self):
        cg, mode = C.c_void_p(), C.c_int(-1)
        check(lib().cgx_mixed_inner(self.h, None, C.byref(cg)))
        check(lib().cgx_cg_get_mode(cg, C.byref(mode)))
        return mode.value

    def solve(self, b, tol, x0=None, max_bodies=-1):
        """-> dict(x, outer, bodies, rxr, status, history)."""
        L = lib()
        n = len(b)
        bv = Vector(self.q, np.asarray(b, np.float64))
        xv = Vector(self.q, np.zeros(n) if x0 is None else np.asarray(x0, np.float64))
        outer, bodies, rxr, status = C.c_int(-1), C.c_int64(-1), C.c_double(-1), C.c_int(-1)
        check(L.cgx_mixed_solve(self.h, bv.ptr(), xv.ptr(), float(tol), int(max_bodies),
                                C.byref(outer), C.byref(bodies), C.byref(rxr), C.byref(status)))
        cnt = C.c_int(0)
        check(L.cgx_mixed_history(self.h, None, None, None, 0, C.byref(cnt)))
        k = cnt.value
        rr, ib, ir = (C.c_double * k)(), (C.c_int64 * k)(), (C.c_double * k)()
        check(L.cgx_mixed_history(self.h, rr, ib, ir, k, C.byref(cnt)))
        return dict(x=xv.to_numpy(), outer=outer.value, bodies=bodies.value, rxr=rxr.value,
                    status=status.value, history=[(rr[i], ib[i], ir[i]) for i in range(k)])


def _configure(mx, name, mode, queue):
    """The case's options on a handle; -> the keyword arguments of solve."""
    c = inputs(name)
    kw = c["kw"]
    L = lib()
    check(L.cgx_mixed_set_mode(mx.h, mode))
    keep = None
    if isinstance(kw.get("precond"), str):
        check(L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Jacobi, None))
    elif kw.get("precond") is not None:
        keep = Vector(queue, kw["precond"])
        check(L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Diagonal, keep.ptr()))
        keep = None  # the object owns an f32 copy: the caller's vector may go
    check(L.cgx_mixed_config(mx.h, 0.0, int(kw.get("max_outer", 0)), int(kw.get("inner_cap", 0))))
    return dict(x0=kw.get("x0"), max_bodies=kw.get("max_bodies", -1))


def _match(name, got):
    """The trajectories of the model the device's run equals in everything."""
    runs = model(name)
    hit = [ch for ch, r in runs
           if r.status == got["status"] and r.outer == got["outer"]
           and r.inner_bodies == got["bodies"] and r.history == got["history"]
           and r.rxr == got["rxr"] and np.array_equal(r.x, got["x"])]
    if not hit:
        r = runs[0][1]
        k = 0
        while k < min(len(r.history), len(got["history"])) and r.history[k] == got["history"][k]:
            k += 1
        pytest.fail(f"{name}: no trajectory of {len(runs)} matches. device: status {got['status']}, "
                    f"outer {got['outer']}, bodies {got['bodies']}, history {got['history']}; model "
                    f"(first trajectory): status {r.status}, outer {r.outer}, bodies "
                    f"{r.inner_bodies}, history {r.history}; first record that differs: {k}; "
                    f"elements of x that differ: {int(np.count_nonzero(r.x != got['x']))} of {r.x.size}")
    return hit


def _matrix(queue, name, monkeypatch=None):
    c = inputs(name)
    mat = CASES[name][0]
    if name == "lean":  # generated on the device, the walk forced at creation (A and A32)
        monkeypatch.setenv("CGX_SPMV_VARIANT", f"{KVL}:0")
        m = Matrix.poisson(queue, *mat[1:])
        assert m.N() == len(c["b"]) and m.NNZ() == len(c["vl"])
        return m
    return Matrix(queue, c["vl"], c["cl"], c["rp"])


BITWISE = [(n, m) for n in ("p2d", "p3d", "irr", "jacobi", "diag", "x0", "tiny2", "tiny3", "tiny5",
                            "stagnate", "cap", "edge1", "edge3", "edge5", "edge1023", "subnormal")
           for m in CASES[n][2]]


@pytest.mark.parametrize("name,mode", BITWISE, ids=[f"{n}-mode{m}" for n, m in BITWISE])
def test_a_model_trajectory_bit_for_bit(queue, name, mode):
    c = inputs(name)
    with Mixed(queue, _matrix(queue, name)) as mx:
        kw = _configure(mx, name, mode, queue)
        assert mx.inner_mode() == mode  # cgx_mixed_inner's solver reports the mode that was set
        got = mx.solve(c["b"], c["tol"], **kw)
        hit = _match(name, got)
        print(f"{name} mode {mode}: status {got['status']}, {got['outer']} outer steps, inner "
              f"bodies {[h[1] for h in got['history'][1:]]}, trajectory {hit}")
        # a second solve on the same handle (its inner graphs now captured) is the same
        again = mx.solve(c["b"], c["tol"], **kw)
        assert again["history"] == got["history"] and np.array_equal(again["x"], got["x"])
        if name in ("p2d", "p3d", "irr", "jacobi", "diag", "x0"):
            assert got["status"] == 1
            r = c["b"] - _spmv64(c, got["x"])
            assert np.linalg.norm(r) <= c["tol"] * (1 + 1e-12)  # numpy's norm, another sum order


def _spmv64(c, x):
    from tests import cg_model
    return cg_model.spmv(c["rp"], c["cl"], c["vl"], x)


def test_status_4_at_n_1_leaves_x(queue):
    c = inputs("nan1")
    x0 = np.array([0.125])
    with Mixed(queue, _matrix(queue, "nan1")) as mx:
        got = mx.solve(c["b"], c["tol"], x0=x0)
    assert (got["status"], got["outer"], got["bodies"]) == (4, 0, 0)
    np.testing.assert_array_equal(got["x"], x0)
    assert got["history"] == [(float((c["b"][0] - c["vl"][0] * x0[0]) ** 2), 0, 0.0)]


def test_lean_walk_in_inner_auto_mode(queue, monkeypatch):
    """Poisson 128 x 64 x 40 with the lean walk forced on A and A32: auto
    resolves to mode 6 inside; inner_cap 6 and max_outer 2 give 12 bodies and
    status 2."""
    c = inputs("lean")
    m = _matrix(queue, "lean", monkeypatch)
    with Mixed(queue, m) as mx:
        kw = _configure(mx, "lean", 0, queue)
        a32, v = C.c_void_p(), C.c_int(0)
        check(lib().cgx_mixed_inner(mx.h, C.byref(a32), None))
        check(lib().cgx_csr_variant(a32, C.byref(v)))
        assert v.value & KVL and mx.inner_mode() == 6
        got = mx.solve(c["b"], c["tol"], **kw)
        assert (got["status"], got["outer"], got["bodies"]) == (2, 2, 12)
        assert [h[1] for h in got["history"]] == [0, 6, 6]
        _match("lean", got)


def test_body_cap_over_the_whole_call(queue):
    """max_bodies counts inner bodies over the call: 100 on p2d ends the second
    inner solve at 19 bodies, status 2."""
    c = inputs("p2d")
    from tests import mixed_model
    want = mixed_model.refine(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], max_bodies=100)
    assert want.status == 2 and [h[1] for h in want.history] == [0, 81, 19] and not want.unclear
    with Mixed(queue, _matrix(queue, "p2d")) as mx:
        check(lib().cgx_mixed_set_mode(mx.h, 1))
        got = mx.solve(c["b"], c["tol"], max_bodies=100)
    assert (got["status"], got["outer"], got["bodies"]) == (2, 2, 100)
    assert got["history"] == want.history and np.array_equal(got["x"], want.x)


# ---------------------------------------------------------------------------
# refusals

def test_refuses_an_f32_matrix(queue):
    c = inputs("p2d")
    m = Matrix(queue, c["vl"], c["cl"], c["rp"], dtype=F32)
    h = C.c_void_p()
    assert lib().cgx_mixed_create(queue.handle, m.schedule(), C.byref(h)) == EINVAL
    assert "f32" in lib().cgx_last_error().decode() and not h.value


def test_refuses_a_partitioned_matrix():
    """One rank over the host transport on a queue of its own."""
    from conjugategradient_amd.hostcomm import AG, AR, EX
    c = inputs("p2d")
    n, nnz = len(c["b"]), len(c["vl"])
    q = cga.Queue(0)
    cbs = (AG(lambda *a: 0), AR(lambda *a: 0), EX(lambda *a: 0))
    L = lib()
    try:
        check(L.cgx_dist_init_host(q.handle, 0, 1, C.cast(cbs[0], C.c_void_p),
                                   C.cast(cbs[1], C.c_void_p), C.cast(cbs[2], C.c_void_p), None))
        m = Matrix(q, c["vl"], c["cl"], c["rp"])
        a, h = C.c_void_p(), C.c_void_p()
        check(L.cgx_csr_create_dist(q.handle, n, 0, n, nnz, m.rows().ptr, m.columns().ptr,
                                    m.data().ptr, 0, C.byref(a)))
        try:
            assert L.cgx_mixed_create(q.handle, a, C.byref(h)) == EUNSUPPORTED
            assert "partitioned" in L.cgx_last_error().decode() and not h.value
        finally:
            L.cgx_csr_destroy(a)
            del m
    finally:
        q.close()


def test_refuses_values_outside_f32(queue):
    c = inputs("p2d")
    vl = c["vl"].copy()
    vl[[7, 100, 101]] = [1e300, -1e-60, -np.inf]
    m = Matrix(queue, vl, c["cl"], c["rp"])
    h = C.c_void_p()
    assert lib().cgx_mixed_create(queue.handle, m.schedule(), C.byref(h)) == EINVAL
    msg = lib().cgx_last_error().decode()
    assert "3 values" in msg and "entry 7" in msg, msg


def test_refuses_a_bad_diagonal_and_bad_config(queue):
    c = inputs("p2d")
    n = len(c["b"])
    L = lib()
    with Mixed(queue, _matrix(queue, "p2d")) as mx:
        d = np.ones(n)
        d[41] = 1e-60  # positive and finite in f64, 0 after the cast
        dv = Vector(queue, d)
        assert L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Diagonal, dv.ptr()) == EINVAL
        assert "entry 41" in L.cgx_last_error().decode()
        d[41] = 1e60   # inf after the cast
        dv = Vector(queue, d)
        assert L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Diagonal, dv.ptr()) == EINVAL
        assert "entry 41" in L.cgx_last_error().decode()
        kind = C.c_int(-1)
        cg = C.c_void_p()
        check(L.cgx_mixed_inner(mx.h, None, C.byref(cg)))
        check(L.cgx_cg_get_precond(cg, C.byref(kind)))
        assert kind.value == cga.Preconditioner.None_  # it keeps what it had
        for args in ((-1.0, 0, 0), (float("nan"), 0, 0), (float("inf"), 0, 0), (0.0, -1, 0),
                     (0.0, 0, -1)):
            assert L.cgx_mixed_config(mx.h, *args) == EINVAL, args
        check(L.cgx_mixed_config(mx.h, 0.0, 0, 0))
        # a mode that refuses a preconditioner fails as cgx_cg_set_precond does
        assert L.cgx_mixed_set_mode(mx.h, 2) in (0, EUNSUPPORTED)
        if mx.inner_mode() == 2:
            assert L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Jacobi, None) == EUNSUPPORTED
        check(L.cgx_mixed_set_mode(mx.h, 1))
        check(L.cgx_mixed_set_precond(mx.h, cga.Preconditioner.Jacobi, None))
        assert L.cgx_mixed_set_mode(mx.h, 6) == EUNSUPPORTED
        # the defaults still solve
        got = mx.solve(c["b"], c["tol"])
        assert got["status"] == 1


def test_bytes_cover_the_f32_values_and_vectors(queue):
    c = inputs("p3d")
    n, nnz = len(c["b"]), len(c["vl"])
    with Mixed(queue, _matrix(queue, "p3d")) as mx:
        by = C.c_int64(0)
        check(lib().cgx_mixed_bytes(mx.h, C.byref(by)))
    own = 4 * nnz + 2 * 8 * n + 2 * 4 * n  # val32, r and Ax, r32 and d32
    inner = 3 * 4 * n                       # the inner solver's r, p, Ap at the least
    print(f"cgx_mixed_bytes: {by.value} (n = {n}, nnz = {nnz}; own {own}, inner >= {inner})")
    assert by.value >= own + inner


# ---------------------------------------------------------------------------
# the bindings

def _cg(queue, name):
    c = inputs(name)
    cg = cga.CG(queue)
    cg.setMatrix(c["vl"], c["cl"], c["rp"])
    cg.setTarget(c["b"])
    return cg


def test_python_solve_mixed(queue):
    c = inputs("jacobi")
    cg = _cg(queue, "jacobi")
    cg.mode = 3
    cg.setPreconditioner(cga.Preconditioner.Jacobi)
    cg.solve_mixed(c["tol"])
    got = dict(x=cg.extract(), outer=cg.outer_steps, bodies=cg.iterations, rxr=cg.final_rxr,
               status=cg.mixed_status, history=cg.mixed_history)
    _match("jacobi", got)
    assert cg.mixed_status == 1 and cg.is_solved


def test_python_fallback_continues_in_f64(queue):
    """tol 0: the mixed solve stagnates (status 3); with fallback the f64 solve
    goes on from its x. Equal to a plain f64 solve warm-started from that x."""
    c = inputs("stagnate")
    cg = _cg(queue, "stagnate")
    cg.mode = 1
    cg.solve_mixed(0.0, fallback=False)
    assert cg.mixed_status == 3
    xm, km = cg.extract(), cg.iterations
    _match("stagnate", dict(x=xm, outer=cg.outer_steps, bodies=km, rxr=cg.final_rxr, status=3,
                            history=cg.mixed_history))
    plain = _cg(queue, "stagnate")
    plain.mode = 1
    plain.setInitial(xm)
    plain.solve(0.0)
    both = _cg(queue, "stagnate")
    both.mode = 1
    both.solve_mixed(0.0, fallback=True)
    assert both.mixed_status == 3 and both.outer_steps == 4
    assert both.iterations == km + plain.iterations
    np.testing.assert_array_equal(both.extract(), plain.extract())  # (NaNs in equal places equal)
    np.testing.assert_equal(both.final_rxr, plain.final_rxr)


def test_mixed_check_runs():
    if not os.path.exists(EXE):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "examples")], check=True)
    p = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr[-2000:]
    assert "agreement to 1e-10" in p.stdout and "NO agreement" not in p.stdout
