"""The ring form of the tile walk (spmv_lean_ring, lean_ring_ok; mode 7's
first kernel): a workgroup shares a plane's formed center lines through LDS,
so a wave's +-a pairs and x-line edge values come from its neighbours'
centers instead of from loads of its own. The per-row sums are the tile
walk's products in the same order, so x is bit-identical to mode 3 (the
4-wave walk's body), to the per-wave tile form, and to the oracle's
double-length model (oracle.cg_solve_dd). Mode 6's first kernel keeps the
per-wave tile form (its ring form measured no faster and was not kept, so
there is no f32 ring kernel: mode 7 is f64 only); it runs beside mode 7 here.

Shapes: 256 x 128 x 128 is the smallest the plane-per-step layout takes (4 ny
workgroups within the grid's bounds, 16 planes per XCD group); 256 x 160 x 128
has another number of workgroups per plane; 256 x 132 x 128 has x-lines that
do not divide into workgroups, and keeps the per-wave form."""
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
BODIES = (5, 6, 7, 8)  # runs end in every slot of a group, both sweep directions


def _forms(m):
    """(tile, ring): the tile walk applies; mode 7's first kernel runs the ring form."""
    t, r = C.c_int(0), C.c_int(0)
    check(lib().cgx_csr_lean_ring(m.schedule(), C.byref(t), C.byref(r)))
    return t.value, r.value


def _auto_mode(queue, m):
    cg = cga.CG(queue)
    cg.setMatrix(m)
    v = C.c_int(-1)
    check(lib().cgx_cg_get_mode(cg._solver(), C.byref(v)))
    return v.value


def _lean_whole(m):
    c, s, g, d, a, ch = C.c_int(), C.c_int64(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
    check(lib().cgx_csr_lean_info(m.schedule(), C.byref(c), C.byref(s), C.byref(g), C.byref(d),
                                  C.byref(a), C.byref(ch)))
    v = C.c_int(0)
    check(lib().cgx_csr_variant(m.schedule(), C.byref(v)))
    return bool(v.value & KVL) and g.value > 0 and ch.value == 0, (g.value, d.value, a.value)


def _solve(queue, m, b, mode, bodies, tol=0.0, dtype=np.float64):
    cg = cga.CG(queue, dtype) if dtype != np.float64 else cga.CG(queue)
    cg.mode = mode
    cg.setMatrix(m)
    cg.setTarget(b.astype(dtype))
    cg.solve(tol, max_iter=bodies)
    return cg.extract(), cg.iterations


class _Case:
    """A shape's matrix, right-hand side and references, computed once."""

    def __init__(self, queue, oracle, dims):
        self.queue, self.oracle, self.dims = queue, oracle, dims
        self.csr = oracle.poisson(*dims)
        n = len(self.csr[0]) - 1
        self.b = np.arange(1, n + 1, dtype=np.float64)  # Tester.cpp:27-30
        self.m = cga.Matrix.poisson(queue, *dims)
        self._dd, self._m3 = {}, {}

    def dd(self, bodies):
        if bodies not in self._dd:
            x, _ = self.oracle.cg_solve_dd(*self.csr, self.b, 0.0, threads=16, max_iter=bodies)
            x.setflags(write=False)
            self._dd[bodies] = x
        return self._dd[bodies]

    def mode3(self, bodies):
        if bodies not in self._m3:
            x, it = _solve(self.queue, self.m, self.b, 3, bodies)
            assert it == bodies
            x.setflags(write=False)
            self._m3[bodies] = x
        return self._m3[bodies]

    def need_ring(self):
        whole, info = _lean_whole(self.m)
        tile, ring = _forms(self.m)
        if not (whole and tile):
            pytest.skip(f"{self.dims}: the plane-per-step layout did not take it {info}")
        assert ring == 1, (self.dims, info)


@pytest.fixture(scope="module")
def cases(queue, oracle):
    made = {}

    def get(dims):
        if dims not in made:
            made[dims] = _Case(queue, oracle, dims)
        return made[dims]

    return get


@pytest.mark.parametrize("dims", [MAIN, OTHER], ids=["256x128x128", "256x160x128"])
@pytest.mark.parametrize("mode", [6, 7])
def test_ring_bit_identical_to_dd_oracle_and_mode3(cases, mode, dims):
    c = cases(dims)
    c.need_ring()
    for bodies in BODIES:
        x, it = _solve(c.queue, c.m, c.b, mode, bodies)
        assert it == bodies
        assert np.array_equal(x, c.dd(bodies)), (bodies, float(np.max(np.abs(x - c.dd(bodies)))))
        assert np.array_equal(x, c.mode3(bodies)), bodies


@pytest.fixture(scope="module")
def to_tol(cases):
    c = cases(MAIN)
    tol = 1e-8 * float(np.linalg.norm(c.b))
    want, res = c.oracle.cg_solve_dd(*c.csr, c.b, tol, threads=16)
    want.setflags(write=False)
    return tol, want, res


@pytest.mark.parametrize("mode", [6, 7])
def test_ring_stop_rule_bodies_exact(cases, to_tol, mode):
    """To 1e-8 ||b||: the body count and x equal the dd oracle's."""
    c = cases(MAIN)
    c.need_ring()
    tol, want, res = to_tol
    assert res.stopped_by_tol
    x, it = _solve(c.queue, c.m, c.b, mode, -1, tol=tol)
    assert it == res.iterations
    assert np.array_equal(x, want), float(np.max(np.abs(x - want)))


def test_lines_not_whole_workgroups_keep_the_tile_form(cases):
    """256 x 132 x 128: lean_tile_ok holds, 132 x-lines do not divide into
    workgroups; the per-wave tile form runs and x is mode 3's."""
    c = cases(ODD)
    whole, info = _lean_whole(c.m)
    tile, ring = _forms(c.m)
    if not (whole and tile):
        pytest.skip(f"{ODD}: the plane-per-step layout did not take it {info}")
    assert ring == 0
    assert _auto_mode(c.queue, c.m) == 6
    for mode in (6, 7):
        for bodies in (7, 8):
            x, it = _solve(c.queue, c.m, c.b, mode, bodies)
            assert it == bodies
            assert np.array_equal(x, c.mode3(bodies)), (mode, bodies)


def test_switch_forces_the_tile_form_same_x(cases, monkeypatch):
    """$CGX_LEAN_RING=0 (read at each call) keeps the per-wave tile form and
    auto at mode 6: x is the ring form's, bit for bit, in modes 6 and 7.
    (256 x 160 x 128: above the 4 M rows up to which auto takes mode 4.)"""
    c = cases(OTHER)
    c.need_ring()
    assert _auto_mode(c.queue, c.m) == 7
    new = {mode: _solve(c.queue, c.m, c.b, mode, 8) for mode in (0, 6, 7)}
    monkeypatch.setenv("CGX_LEAN_RING", "0")
    assert _forms(c.m) == (1, 0)
    assert _auto_mode(c.queue, c.m) == 6
    old = {mode: _solve(c.queue, c.m, c.b, mode, 8) for mode in (0, 6, 7)}
    monkeypatch.delenv("CGX_LEAN_RING")
    assert _forms(c.m) == (1, 1)
    for mode in (0, 6, 7):
        assert new[mode][1] == old[mode][1] == 8
        assert np.array_equal(old[mode][0], new[mode][0]), mode
    assert np.array_equal(new[0][0], c.mode3(8))
