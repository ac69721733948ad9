"""Mode 7 with the group's x flush folded into slot 3's second kernel
(k_spmv_lean_updr_rule_flush). It changes no value: x is mode 3's and the
double-length oracle's (oracle.cg_solve_dd), bit for bit, for runs that end
in every slot with the group finished or not, for runs resumed inside a
group, for a warm start, for a run stopped by the tolerance, on a second
workgroup count per plane and with the per-wave first kernel
($CGX_LEAN_RING=0 and the shape whose x-lines do not divide into workgroups).
The last three cases were written for a clamp of the tile and ring walks'
loads past a part's last plane, which measured no gain and is not in the
tree; they stay as checks of modes 6 and 7 on those paths.

Shapes: 256 x 128 x 128 is the smallest the ring walk takes; 256 x 132 x 128
takes the per-wave first kernel with the same second kernel; 256 x 160 x 128
has another number of workgroups per plane. b_i = i + 1 throughout."""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib

pytestmark = pytest.mark.gpu

KVL = 33554432
MAIN = (3, 256, 128, 128)
OTHER = (3, 256, 160, 128)
ODD = (3, 256, 132, 128)
BODIES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)
POLL = 8
CHUNKS = ((3, 1, 4), (4, 4), (2, 5, 2), (6, 3), (1, 1, 1, 1, 4))


def _forms(m):
    t, r = C.c_int(0), C.c_int(0)
    check(lib().cgx_csr_lean_ring(m.schedule(), C.byref(t), C.byref(r)))
    return t.value, r.value


def _lean_whole(m):
    c, s, g, d, a, ch = C.c_int(), C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().cgx_csr_lean_info(m.schedule(), C.byref(c), C.byref(s), C.byref(g), C.byref(d),
                                  C.byref(a), C.byref(ch)))
    v = C.c_int(0)
    check(lib().cgx_csr_variant(m.schedule(), C.byref(v)))
    return bool(v.value & KVL) and g.value > 0 and ch.value == 0, (g.value, d.value, a.value)


def _solve(queue, m, b, mode, bodies, tol=0.0, x0=None):
    cg = cga.CG(queue)
    cg.mode = mode
    cg.setMatrix(m)
    cg.setTarget(b)
    if x0 is not None:
        cg.setInital(x0)
    cg.solve(tol, max_iter=bodies)
    return cg.extract(), cg.iterations


class _Run:
    """A solver driven through the C ABI: one cgx_cg_begin, then cgx_cg_run
    in chunks, x downloaded after each (cgx_cg_run leaves no x update pending)."""

    def __init__(self, queue, m, b, mode, graph, cap):
        L = lib()
        n = m.N()
        self.q = queue
        self.b = cga.DeviceArray(queue, n, np.float64).upload(b)
        self.x = cga.DeviceArray(queue, n, np.float64)
        self.x.fill(0.0)
        self.cg = C.c_void_p()
        check(L.cgx_cg_create(queue.handle, m.schedule(), C.byref(self.cg)))
        try:
            check(L.cgx_cg_config(self.cg, POLL, 1 if graph else 0))
            check(L.cgx_cg_set_mode(self.cg, mode))
            check(L.cgx_cg_begin(self.cg, self.b.ptr, self.x.ptr, 0.0, cap))
        except Exception:
            self.close()
            raise

    def run(self, bodies):
        tot, st = C.c_int64(), C.c_int()
        check(lib().cgx_cg_run(self.cg, bodies, C.byref(tot), C.byref(st)))
        check(lib().cgx_sync(self.q.handle))
        return self.x.download(), tot.value, st.value

    def close(self):
        if self.cg:
            lib().cgx_cg_destroy(self.cg)
            self.cg = C.c_void_p()


class _Case:
    """A shape's matrix, right-hand side and references, computed once."""

    def __init__(self, queue, oracle, dims):
        self.queue, self.oracle, self.dims = queue, oracle, dims
        self.csr = oracle.poisson(*dims)
        n = len(self.csr[0]) - 1
        self.b = np.arange(1, n + 1, dtype=np.float64)
        self.m = cga.Matrix.poisson(queue, *dims)
        self._dd, self._m3 = {}, {}

    def dd(self, bodies):
        if bodies not in self._dd:
            x, _ = self.oracle.cg_solve_dd(*self.csr, self.b, 0.0, threads=16, max_iter=bodies)
            x.setflags(write=False)
            self._dd[bodies] = x
        return self._dd[bodies]

    def mode3(self, bodies, x0=None):
        key = bodies if x0 is None else (bodies, "warm")
        if key not in self._m3:
            x, it = _solve(self.queue, self.m, self.b, 3, bodies, x0=x0)
            assert it == bodies
            x.setflags(write=False)
            self._m3[key] = x
        return self._m3[key]

    def need_tile(self, ring):
        whole, info = _lean_whole(self.m)
        tile, r = _forms(self.m)
        if not (whole and tile):
            pytest.skip(f"{self.dims}: the plane-per-step layout did not take it {info}")
        assert r == ring, (self.dims, info)


@pytest.fixture(scope="module")
def cases(queue, oracle):
    made = {}

    def get(dims):
        if dims not in made:
            made[dims] = _Case(queue, oracle, dims)
        return made[dims]

    return get


@pytest.mark.parametrize("graph", [1, 0], ids=["graph", "nograph"])
@pytest.mark.parametrize("bodies", BODIES)
def test_runs_end_in_every_slot(cases, bodies, graph):
    """Cap = bodies. A run of exactly that many bodies ends in slot bodies mod
    4 with the group finished (4, 8, 12) or not; a run of whole poll intervals
    past the cap also launches the bodies after the stop, so with caps 5, 6
    and 7 the slot-3 launch finds its body inactive and a partial group
    pending (the fused kernel's inactive path)."""
    c = cases(MAIN)
    c.need_tile(1)
    for ask in (bodies, -(-bodies // POLL) * POLL):
        run = _Run(c.queue, c.m, c.b, 7, graph, bodies)
        try:
            x, tot, st = run.run(ask)
        finally:
            run.close()
        assert tot == bodies and st == 2, (ask, tot, st)
        assert np.array_equal(x, c.mode3(bodies)), (ask, float(np.max(np.abs(x - c.mode3(bodies)))))
        assert np.array_equal(x, c.dd(bodies)), (ask, float(np.max(np.abs(x - c.dd(bodies)))))


@pytest.mark.parametrize("graph", [1, 0], ids=["graph", "nograph"])
@pytest.mark.parametrize("chunks", CHUNKS, ids=["+".join(map(str, ch)) for ch in CHUNKS])
def test_resumed_runs(cases, chunks, graph):
    """One begin (cap 12), runs resumed inside and at the ends of groups:
    after every chunk x is mode 3's after the same number of bodies."""
    c = cases(MAIN)
    c.need_tile(1)
    run = _Run(c.queue, c.m, c.b, 7, graph, 12)
    try:
        done = 0
        for ch in chunks:
            x, tot, _ = run.run(ch)
            done += ch
            assert tot == done, (chunks, ch, tot)
            assert np.array_equal(x, c.mode3(done)), (chunks, done)
    finally:
        run.close()


def test_warm_start(cases):
    c = cases(MAIN)
    c.need_tile(1)
    x0 = np.random.default_rng(7).standard_normal(c.b.size)
    for bodies in (7, 8):
        x, it = _solve(c.queue, c.m, c.b, 7, bodies, x0=x0.copy())
        assert it == bodies
        assert np.array_equal(x, c.mode3(bodies, x0=x0.copy())), bodies


def test_stop_by_tolerance(cases):
    """To 1e-8 ||b||: the body count and x equal the dd oracle's."""
    c = cases(MAIN)
    c.need_tile(1)
    tol = 1e-8 * float(np.linalg.norm(c.b))
    want, res = c.oracle.cg_solve_dd(*c.csr, c.b, tol, threads=16)
    assert res.stopped_by_tol
    x, it = _solve(c.queue, c.m, c.b, 7, -1, tol=tol)
    assert it == res.iterations
    assert np.array_equal(x, want), float(np.max(np.abs(x - want)))


@pytest.mark.parametrize("mode", [6, 7])
def test_other_workgroup_count(cases, mode):
    """256 x 160 x 128: modes 6 (tile walk) and 7 (ring walk) equal mode 3."""
    c = cases(OTHER)
    c.need_tile(1)
    for bodies in (5, 6, 7, 8):
        x, it = _solve(c.queue, c.m, c.b, mode, bodies)
        assert it == bodies
        assert np.array_equal(x, c.mode3(bodies)), (mode, bodies)


def test_per_wave_walk_under_the_switch(cases, monkeypatch):
    """$CGX_LEAN_RING=0: mode 7's first kernel is the per-wave tile walk."""
    c = cases(MAIN)
    c.need_tile(1)
    want = {bodies: c.mode3(bodies) for bodies in (5, 6, 7, 8)}
    monkeypatch.setenv("CGX_LEAN_RING", "0")
    assert _forms(c.m) == (1, 0)
    for bodies, w in want.items():
        x, it = _solve(c.queue, c.m, c.b, 7, bodies)
        assert it == bodies
        assert np.array_equal(x, w), bodies


def test_lines_not_whole_workgroups(cases):
    """256 x 132 x 128: the per-wave first kernel, the same fused second one."""
    c = cases(ODD)
    c.need_tile(0)
    for bodies in (5, 6, 7, 8):
        x, it = _solve(c.queue, c.m, c.b, 7, bodies)
        assert it == bodies
        assert np.array_equal(x, c.mode3(bodies)), bodies
