"""The sweep directions of the CG bodies (cgx_sweep.h, cgx_cg_sweep_dirs): the
two-kernel bodies on one device (modes 4 and 7) launch 0, 1 in every slot, so
the launches alternate strictly in stream order, where they used to run
0,1 | 1,0 | 0,1 | 1,0; the three-kernel bodies (modes 3 and 6) keep
slot & 1, 1 - (slot & 1), slot & 1. A direction changes the order a launch
walks its rows in and with it the order of its dot's partial sums, which the
double-length dots make invisible: x stays mode 3's and the double-length
oracle's (oracle.cg_solve_dd), bit for bit. Mode 3 runs the directions it
always ran, so it and the oracle are the references; neither is code this
schedule touches.

Shapes: 256 x 128 x 128 is the smallest the ring walk takes
(tests/test_gpu_lean_ring.py); 256 x 132 x 128 has x-lines that do not divide
into workgroups and keeps the per-wave first kernel. The lean walk is forced
at creation ($CGX_SPMV_VARIANT, as tests/test_gpu_fullsize.py does), so modes
4, 6 and 7 run their lean kernels whatever the autotune measures on the day.
b_i = i + 1 throughout."""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib

pytestmark = pytest.mark.gpu

KVL = 33554432
MAIN = (3, 256, 128, 128)
ODD = (3, 256, 132, 128)


def _forms(m):
    t, r = C.c_int(0), C.c_int(0)
    check(lib().cgx_csr_lean_ring(m.schedule(), C.byref(t), C.byref(r)))
    return t.value, r.value


def _mode(h):
    v = C.c_int(-1)
    check(lib().cgx_cg_get_mode(h, C.byref(v)))
    return v.value


def _dirs(h, slot):
    d, n = (C.c_int * 4)(9, 9, 9, 9), C.c_int(-1)
    check(lib().cgx_cg_sweep_dirs(h, slot, d, 4, C.byref(n)))
    return [d[k] for k in range(n.value)]


def _solve(queue, m, b, mode, bodies, tol=0.0):
    cg = cga.CG(queue)
    cg.mode = mode
    cg.setMatrix(m)
    cg.setTarget(b)
    cg.solve(tol, max_iter=bodies)
    assert _mode(cg._solver()) == mode
    return cg.extract(), cg.iterations


class _Run:
    """One cgx_cg_begin, then cgx_cg_run in chunks of `poll` bodies, each chunk
    a graph captured from the slot it starts in."""

    def __init__(self, queue, m, b, mode, poll, cap):
        L = lib()
        n = m.N()
        self.q = queue
        self.b = cga.DeviceArray(queue, n, np.float64).upload(b)
        self.x = cga.DeviceArray(queue, n, np.float64)
        self.x.fill(0.0)
        self.cg = C.c_void_p()
        check(L.cgx_cg_create(queue.handle, m.schedule(), C.byref(self.cg)))
        try:
            check(L.cgx_cg_config(self.cg, poll, 1))
            check(L.cgx_cg_set_mode(self.cg, mode))
            assert _mode(self.cg) == mode
            check(L.cgx_cg_begin(self.cg, self.b.ptr, self.x.ptr, 0.0, cap))
        except Exception:
            self.close()
            raise

    def run(self, bodies):
        tot, st, rxr = C.c_int64(), C.c_int(), C.c_double()
        check(lib().cgx_cg_run(self.cg, bodies, C.byref(tot), C.byref(st)))
        check(lib().cgx_sync(self.q.handle))
        check(lib().cgx_cg_rxr(self.cg, C.byref(rxr)))
        return self.x.download(), tot.value, rxr.value

    def close(self):
        if self.cg:
            lib().cgx_cg_destroy(self.cg)
            self.cg = C.c_void_p()


class _Case:
    """A shape's matrix (the lean walk forced), right-hand side and
    references, computed once and left unchanged."""

    def __init__(self, queue, oracle, dims):
        self.queue, self.oracle, self.dims = queue, oracle, dims
        self.csr = oracle.poisson(*dims)
        n = len(self.csr[0]) - 1
        self.b = np.arange(1, n + 1, dtype=np.float64)
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("CGX_SPMV_VARIANT", f"{KVL}:0")
            self.m = cga.Matrix.poisson(queue, *dims)
            v = C.c_int(0)
            check(lib().cgx_csr_variant(self.m.schedule(), C.byref(v)))
        assert v.value & KVL, (dims, v.value)
        self._dd, self._m3 = {}, {}

    def dd(self, bodies):
        if bodies not in self._dd:
            x, _ = self.oracle.cg_solve_dd(*self.csr, self.b, 0.0, threads=16, max_iter=bodies)
            x.setflags(write=False)
            self._dd[bodies] = x
        return self._dd[bodies]

    def mode3(self, bodies, tol=0.0):
        key = (bodies, tol)
        if key not in self._m3:
            x, it = _solve(self.queue, self.m, self.b, 3, bodies, tol)
            x.setflags(write=False)
            self._m3[key] = (x, it)
        return self._m3[key]


@pytest.fixture(scope="module")
def cases(queue, oracle):
    made = {}

    def get(dims):
        if dims not in made:
            made[dims] = _Case(queue, oracle, dims)
        return made[dims]

    return get


def test_schedule(cases):
    """Slots 0 - 7: modes 4 and 7 alternate strictly in stream order; modes 3
    and 6 are launched as they always were (the rule written out)."""
    c = cases(MAIN)
    assert _forms(c.m) == (1, 1)
    for mode in (4, 7, 3, 6):
        cg = cga.CG(c.queue)
        cg.mode = mode
        cg.setMatrix(c.m)
        h = cg._solver()
        assert _mode(h) == mode
        per_slot = [_dirs(h, slot) for slot in range(8)]
        if mode in (4, 7):
            assert all(len(d) == 2 for d in per_slot), (mode, per_slot)
            seq = [v for d in per_slot for v in d]
            assert seq[0] == 0
            assert all(seq[i] == 1 - seq[i - 1] for i in range(1, len(seq))), (mode, seq)
        else:
            for slot, d in enumerate(per_slot):
                par = slot & 1
                rpar = 1 - par
                assert d == [par, rpar, par], (mode, slot, d)


@pytest.mark.parametrize("mode", [7, 4])
def test_bit_identical_to_mode3_and_dd_oracle(cases, mode):
    """9 bodies end in slot 0: a one-body partial group to flush after two
    folded flushes; 12 bodies end with a folded flush."""
    c = cases(MAIN)
    assert _forms(c.m) == (1, 1)
    for bodies in (9, 12):
        x, it = _solve(c.queue, c.m, c.b, mode, bodies)
        assert it == bodies
        x3, it3 = c.mode3(bodies)
        assert it3 == bodies
        assert np.array_equal(x, x3), (mode, bodies, float(np.max(np.abs(x - x3))))
        assert np.array_equal(x, c.dd(bodies)), (mode, bodies,
                                                 float(np.max(np.abs(x - c.dd(bodies)))))


def test_split_run(cases):
    """Mode 7, one solver: runs of 3 then 6 bodies in chunks of 3 (graphs
    captured from slots 0, 3 and 2) against another solver's single chunk of
    9 from slot 0: x and r.r equal, and x is mode 3's."""
    c = cases(MAIN)
    assert _forms(c.m) == (1, 1)
    whole = _Run(c.queue, c.m, c.b, 7, 9, 9)
    try:
        xw, totw, rxrw = whole.run(9)
    finally:
        whole.close()
    split = _Run(c.queue, c.m, c.b, 7, 3, 9)
    try:
        x1, tot1, _ = split.run(3)
        assert tot1 == 3
        assert np.array_equal(x1, c.mode3(3)[0])
        xs, tots, rxrs = split.run(6)
    finally:
        split.close()
    assert totw == tots == 9
    assert np.array_equal(xs, xw)
    assert rxrs == rxrw
    assert np.array_equal(xs, c.mode3(9)[0])


def test_stop_inside_a_group(cases):
    """A tolerance mode 3 reaches after a body count that is no multiple of 4
    (tightened once if the first lands on one): mode 7 stops after the same
    count with the same x."""
    c = cases(MAIN)
    assert _forms(c.m) == (1, 1)
    tol = 1e-2 * float(np.linalg.norm(c.b))
    x3, it3 = c.mode3(-1, tol)
    if it3 % 4 == 0:
        tol *= 0.7
        x3, it3 = c.mode3(-1, tol)
    print(f"mode 3 stops after {it3} bodies at tol {tol:.6e}")
    assert it3 > 4 and it3 % 4 != 0, it3
    x7, it7 = _solve(c.queue, c.m, c.b, 7, -1, tol)
    assert it7 == it3
    assert np.array_equal(x7, x3), float(np.max(np.abs(x7 - x3)))


def test_per_wave_first_kernel(cases):
    """256 x 132 x 128: lean_ring_ok is false, mode 7's first kernel is the
    per-wave tile walk under the same schedule."""
    c = cases(ODD)
    assert _forms(c.m) == (1, 0)
    x, it = _solve(c.queue, c.m, c.b, 7, 6)
    assert it == 6
    x3, it3 = c.mode3(6)
    assert it3 == 6
    assert np.array_equal(x, x3), float(np.max(np.abs(x - x3)))
    assert np.array_equal(x, c.dd(6)), float(np.max(np.abs(x - c.dd(6))))
