"""The loop's dots as double-length sums (round 6; cgx_dd.h): x does not
depend on the SpMV form the autotune picks, the iteration mode, the sweep
direction or the launch grids — and it equals, bit for bit, the oracle's
model of that arithmetic (oracle.cg_solve_dd: the reference iteration with
each dot a double-length sum, rounded once, on OpenMP threads), at the
BASELINE configs' full sizes.

The reference's own summation order (sycl::reduction) stays unpinned; these
tests pin the engine's arithmetic, every other value of which is rounded as
in the reference's expressions (no FMA). Up to round 5 the iterates moved
at the rounding level with the form a timing comparison picked
(VERDICT r5, weak #1)."""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import check, lib
from tests.util import irregular_spd

pytestmark = pytest.mark.gpu

BODIES = 40
KVL = 33554432
KIL = 67108864


def _record(m):
    """The autotune's timed forms (cgx_csr_autotune_record): variant, kind."""
    L = lib()
    n = C.c_int(0)
    L.cgx_csr_autotune_record(m.schedule(), None, None, None, 0, C.byref(n))
    v, k, us = (C.c_int * n.value)(), (C.c_int * n.value)(), (C.c_float * n.value)()
    check(L.cgx_csr_autotune_record(m.schedule(), v, k, us, n.value, C.byref(n)))
    return [(v[i], k[i]) for i in range(n.value)]


def _variant(m):
    v = C.c_int(0)
    check(lib().cgx_csr_variant(m.schedule(), C.byref(v)))
    return v.value


def _solve(queue, m, b, mode, bodies=BODIES, tol=0.0):
    cg = cga.CG(queue)
    cg.mode = mode
    cg.setMatrix(m)
    cg.setTarget(b)
    cg.solve(tol, max_iter=bodies)
    return cg.extract(), cg.iterations


def _forms(m, extra=()):
    """Every form the autotune timed as a loop SpMV (k_spmv_dot over the
    matrix, the lean walk), in its record's order, and `extra`."""
    seen = []
    for v, kind in _record(m):
        if kind in (0, 3) and v not in seen:
            seen.append(v)
    for v in extra:
        if v not in seen:
            seen.append(v)
    return seen


def _check_forms(queue, m, b, want, forms, modes=(3,)):
    prod = _variant(m)
    ran = []
    for v in forms:
        check(lib().cgx_csr_set_variant(m.schedule(), v))
        for mode in modes:
            x, it = _solve(queue, m, b, mode)
            assert it == BODIES
            assert np.array_equal(x, want), (v, mode, float(np.max(np.abs(x - want))))
            ran.append((v, mode))
    check(lib().cgx_csr_set_variant(m.schedule(), prod))
    return ran


def test_256cubed_every_form_and_mode_bit_identical_to_dd_oracle(queue, oracle):
    rp, cl, vl = oracle.poisson(3, 256, 256, 256)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)  # Tester.cpp:27-30
    want, _ = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, threads=16, max_iter=BODIES)
    m = cga.Matrix.poisson(queue, 3, 256, 256, 256)
    forms = _forms(m, extra=(15 | KIL,))
    # the production form (the lean walk) in modes 1, 3, 4, 6 (Ap recomputed
    # by a second walk instead of stored) and 7 (mode 4's formed p_k with Ap
    # recomputed, the tile walk); the rest in mode 3
    assert _variant(m) & KVL
    ran = _check_forms(queue, m, b, want, [_variant(m)], modes=(1, 3, 4, 6, 7))
    ran += _check_forms(queue, m, b, want, [v for v in forms if not v & KVL])
    print("256^3 forms x modes, x bit-identical to the dd oracle:", ran)
    assert len(ran) >= 8, ran  # CSR-stream, SELL, SELL-P, value codes, templates, lean


def test_256cubed_stop_rule_bodies_exact(queue, oracle):
    """To tolerance (1e-8 ||b||, ~890 bodies, auto mode): the body count and x
    equal the dd oracle's exactly — the stop rule (CG.hpp:396-404, 436)
    reads the same r.r bits on both sides."""
    rp, cl, vl = oracle.poisson(3, 256, 256, 256)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    tol = 1e-8 * float(np.linalg.norm(b))
    want, res = oracle.cg_solve_dd(rp, cl, vl, b, tol, threads=16)
    m = cga.Matrix.poisson(queue, 3, 256, 256, 256)
    x, it = _solve(queue, m, b, 0, bodies=-1, tol=tol)
    assert res.stopped_by_tol
    assert it == res.iterations
    assert np.array_equal(x, want), float(np.max(np.abs(x - want)))


def test_tile_walk_other_shape_bit_identical_to_dd_oracle(queue, oracle):
    """The tile walk (modes 6 and 7's p.Ap walk, lean_tile_ok) on a second
    shape it takes: 256 x 128 x 256 (a = 2 slices, 256 slices per plane, 16
    planes per wave at two parts per XCD group), x equal to the dd oracle bit
    for bit in modes 6 and 7, and to mode 3 (the 4-wave walk's body)."""
    dims = (3, 256, 128, 256)
    rp, cl, vl = oracle.poisson(*dims)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    want, _ = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, threads=16, max_iter=BODIES)
    m = cga.Matrix.poisson(queue, *dims)
    assert _variant(m) & KVL
    ran = _check_forms(queue, m, b, want, [_variant(m)], modes=(3, 6, 7))
    print("256x128x256:", ran)


def test_tile_walk_f32(queue, oracle):
    """The tile walk in f32 (mode 6's p.Ap kernel, T = float): 20 bodies at
    256 x 128 x 256 against mode 3 (the 4-wave walk's body) and the f64 dd
    oracle. f32 dots keep f32 pairs, which are not split-independent (§6),
    so the bars are tolerances: a wrong neighbour or edge would be far
    outside them. (The f32 loop's arithmetic, mode 6's second walk included,
    is held bit for bit to the exact-dot model at smaller sizes in
    tests/test_gpu_f32.py.)"""
    dims = (3, 256, 128, 256)
    rp, cl, vl = oracle.poisson(*dims)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    want, _ = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, threads=16, max_iter=20)
    m = cga.Matrix.poisson(queue, *dims, dtype=np.float32)
    xs = {}
    for mode in (3, 6):
        cg = cga.CG(queue, np.float32)
        cg.mode = mode
        cg.setMatrix(m)
        cg.setTarget(b.astype(np.float32))
        cg.solve(0.0, max_iter=20)
        assert cg.iterations == 20
        xs[mode] = cg.extract().astype(np.float64)
    d36 = float(np.linalg.norm(xs[6] - xs[3]) / np.linalg.norm(xs[3]))
    d6 = float(np.linalg.norm(xs[6] - want) / np.linalg.norm(want))
    print("f32 tile walk: mode 6 vs 3", d36, "vs f64 dd oracle", d6)
    assert d36 <= 1e-5 and d6 <= 1e-4, (d36, d6)


@pytest.mark.parametrize("mode", [6, 7])
def test_256cubed_stop_rule_bodies_exact_recomputed(queue, oracle, mode):
    """Modes 6 and 7 to tolerance: the same bodies and x as the dd oracle
    (mode 7's stop rule runs in its kernel 2, as mode 4's update_r)."""
    rp, cl, vl = oracle.poisson(3, 256, 256, 256)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    tol = 1e-8 * float(np.linalg.norm(b))
    want, res = oracle.cg_solve_dd(rp, cl, vl, b, tol, threads=16)
    m = cga.Matrix.poisson(queue, 3, 256, 256, 256)
    x, it = _solve(queue, m, b, mode, bodies=-1, tol=tol)
    assert it == res.iterations
    assert np.array_equal(x, want), float(np.max(np.abs(x - want)))


def test_4096squared_forms_bit_identical_to_dd_oracle(queue, oracle):
    rp, cl, vl = oracle.poisson(2, 4096, 4096, 1)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    want, _ = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, threads=16, max_iter=BODIES)
    m = cga.Matrix.poisson(queue, 2, 4096, 4096, 1)
    ran = _check_forms(queue, m, b, want, [_variant(m)], modes=(1, 3, 4))
    ran += _check_forms(queue, m, b, want, [v for v in _forms(m) if v != _variant(m)][:6])
    print("4096^2:", ran)


def test_g3_standin_every_form_bit_identical_to_dd_oracle(queue, oracle):
    """The ill-conditioned irregular case, where plain summation orders
    diverge (the oracle on 16 against 8 threads: ~3e-8 after 40 bodies):
    every CSR-stream form the autotune can pick, modes 1 and 3, equals the
    dd oracle bit for bit."""
    rp, cl, vl = irregular_spd(1_585_478, mean_deg=3.83, seed=12345)
    n = len(rp) - 1
    b = np.arange(1, n + 1, dtype=np.float64)
    want, _ = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, threads=16, max_iter=BODIES)
    m = cga.Matrix(queue, vl, cl, rp)
    forms = _forms(m, extra=(0, 5, 13, 15, 133, 265, 13 | KIL))
    ran = _check_forms(queue, m, b, want, forms, modes=(1, 3))
    print("G3 stand-in:", ran)
