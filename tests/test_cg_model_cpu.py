"""tests/cg_model.py, the numpy model the f32 engine is held to bit for bit
(tests/test_gpu_f32.py), checked without a device:

  - at float64 it is oracle.cg_solve_dd (the engine's f64 model) bit for bit,
    and its preconditioned branch is tests/test_pcg_cpu.pcg(exact=True), so
    the model cannot be bent to fit the device;
  - every loop case the GPU file runs (CASES, imported from here) has at most
    cg_model.MAX_UNCLEAR dots that are not clear, on every trajectory. This is
    a condition on the inputs (seed, body count), met by the model alone;
  - on those inputs three deliberately wrong variants of the model differ from
    it in at least one bit of x: the evidence that the bit comparison on the
    device separates an FMA in the r update, unrounded products in p.Ap and
    dots that are not double-length sums.
"""
import functools

import numpy as np
import pytest

from tests import cg_model
from tests.test_pcg_cpu import case as pcg_case, diag_of, pcg
from tests.util import irregular_spd, rel

F32 = np.float32
KVL = 33554432  # the lean stencil walk's variant bit


def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


def _dense_csr(dense):
    n = len(dense)
    r, c = np.nonzero(dense)
    rp = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int32)
    return rp, c.astype(np.int32), dense[r, c].astype(np.float64)


def _tridiag(d):
    d = np.asarray(d, np.float64)
    o = -0.3 * np.sqrt(d[:-1] * d[1:])  # D^-1/2 A D^-1/2 = tridiag(-0.3, 1, -0.3): SPD
    return np.diag(d) + np.diag(o, 1) + np.diag(o, -1)


TINY = {1: np.array([[4.0]]), 2: np.array([[4.0, 1.0], [1.0, 3.0]]),
        3: _tridiag([1.0, 10.0, 100.0]), 5: _tridiag([1.0, 10.0, 100.0, 1e3, 1e4])}

# name: (matrix, modes, max_bodies, relative tol, seed of b, extras)
#   matrix: ("poisson", dim, nx, ny, nz) | ("irr",) | ("tiny", n) | ("pcg", name)
#   extras: "x0" a non-zero initial guess, "jacobi" 1 / diag(A) as m, "lean"
#   the lean walk forced at creation
CASES = {
    "p2d": (("poisson", 2, 33, 31, 1), (1, 2, 3), 12, 0.0, 3, ()),
    "p2d-tol": (("poisson", 2, 33, 31, 1), (1, 2, 3), -1, 1e-3, 3, ()),
    "irr": (("irr",), (1, 2, 3), 12, 0.0, 3, ()),
    "p3d": (("poisson", 3, 48, 48, 30), (1, 3), 12, 0.0, 4, ()),
    "tiny1": (("tiny", 1), (1, 3), -1, 0.0, 3, ()),
    "tiny2": (("tiny", 2), (1, 3), -1, 0.0, 4, ()),
    "tiny3": (("tiny", 3), (1, 3), -1, 0.0, 4, ()),
    "tiny5": (("tiny", 5), (1, 3), -1, 0.0, 3, ()),
    "lean": (("poisson", 3, 128, 64, 40), (3, 6), 6, 0.0, 3, ("lean",)),
    "x0": (("poisson", 2, 33, 31, 1), (1, 3), 12, 0.0, 3, ("x0",)),
    "jacobi-p2d": (("pcg", "p2d"), (1, 3), 12, 0.0, 3, ("jacobi",)),
    "jacobi-irr": (("pcg", "irr"), (1, 3), 12, 0.0, 3, ("jacobi",)),
    "nt": (("poisson", 2, 4096, 2050, 1), (1, 3), 1, 0.0, 3, ()),
}
# the cases whose guard is below 0.02 ulp (up to ~70k rows): no dot may be unclear
SMALL = [c for c in CASES if c not in ("lean", "nt")]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(rp, cl, vl (f64), b (f32), x0, minv (f32 or None), tol, cap)."""
    mat, _, cap, tol_rel, seed, extras = CASES[name]
    if mat[0] == "poisson":
        rp, cl, vl = _oracle().poisson(*mat[1:])
    elif mat[0] == "irr":
        rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
    elif mat[0] == "tiny":
        rp, cl, vl = _dense_csr(TINY[mat[1]])
    else:
        rp, cl, vl, _ = pcg_case(mat[1])  # the scaled matrix
    n = len(rp) - 1
    b = np.random.default_rng(seed).standard_normal(n).astype(F32)
    x0 = None
    if "x0" in extras:
        x0 = (0.5 * np.random.default_rng(seed + 100).standard_normal(n)).astype(F32)
    minv = None
    if "jacobi" in extras:  # cgx_csr_diag_inv's values (test_diag_inv_is_numpys_bit_for_bit)
        rows = np.repeat(np.arange(n), np.diff(rp))
        on = rows == cl
        d32 = np.zeros(n, F32)
        np.add.at(d32, rows[on], np.asarray(vl, F32)[on])
        minv = F32(1) / d32
    tol = tol_rel * float(np.linalg.norm(b.astype(np.float64)))
    out = dict(rp=np.asarray(rp, np.int32), cl=np.asarray(cl, np.int32),
               vl=np.asarray(vl, np.float64), b=b, x0=x0, minv=minv, tol=tol, cap=cap)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model(name):
    """Every trajectory of the f32 model on a case: [(choices, Run)], with x
    after each body kept. Computed once."""
    c = inputs(name)
    return cg_model.trajectories(c["rp"], c["cl"], c["vl"].astype(F32), c["b"], c["tol"], c["cap"],
                                 x0=c["x0"], minv=c["minv"], dtype=F32, keep_x=True)


# ---------------------------------------------------------------------------
# the model against the oracle, float64

SHAPES = [(2, 48, 40, 1), (3, 12, 11, 10), (2, 129, 65, 1)]


def _b64(n):
    return np.random.default_rng(3).standard_normal(n)


@pytest.mark.parametrize("dims", SHAPES, ids=["48x40", "12x11x10", "129x65"])
def test_f64_model_is_the_dd_oracle_bit_for_bit(oracle, dims):
    rp, cl, vl = oracle.poisson(*dims)
    b = _b64(len(rp) - 1)
    run = cg_model.cg(rp, cl, vl, b, 0.0, 12, dtype=np.float64)
    x, res = oracle.cg_solve_dd(rp, cl, vl, b, 0.0, max_iter=12)
    print(f"{dims}: 12 bodies, r.r {run.rr[-1]!r} (oracle {res.rxr!r}), "
          f"{len(run.unclear)} dots not clear")
    assert run.bodies == res.iterations == 12
    np.testing.assert_array_equal(run.x, x)
    assert float(run.rr[-1]) == res.rxr and float(run.rr0) == res.rxr0
    assert run.x.dtype == np.float64 and not run.unclear


def test_f64_model_to_a_tolerance_and_from_an_initial_guess(oracle):
    rp, cl, vl = oracle.poisson(2, 48, 40, 1)
    b = _b64(len(rp) - 1)
    tol = 1e-8 * float(np.linalg.norm(b))
    run = cg_model.cg(rp, cl, vl, b, tol, -1, dtype=np.float64)
    x, res = oracle.cg_solve_dd(rp, cl, vl, b, tol)
    print(f"to 1e-8 ||b||: {run.bodies} bodies (oracle {res.iterations}), "
          f"{len(run.unclear)} dots not clear")
    assert res.stopped_by_tol and 12 < run.bodies == res.iterations < len(b)
    np.testing.assert_array_equal(run.x, x)
    assert float(run.rr[-1]) == res.rxr
    x0 = 0.5 * x + np.random.default_rng(4).standard_normal(len(b))
    run = cg_model.cg(rp, cl, vl, b, tol, 20, x0=x0, dtype=np.float64)
    x, res = oracle.cg_solve_dd(rp, cl, vl, b, tol, max_iter=20, x0=x0)
    assert run.bodies == res.iterations == 20
    np.testing.assert_array_equal(run.x, x)
    assert float(run.rr[-1]) == res.rxr and float(run.rr0) == res.rxr0


def test_model_spmv_is_the_oracles(oracle):
    for rp, cl, vl in (oracle.poisson(3, 12, 11, 10), irregular_spd(4097, hub=300, seed=3),
                       (np.array([0, 3], np.int32), np.array([0, 0, 0], np.int32), np.ones(3))):
        x = np.random.default_rng(7).standard_normal(len(rp) - 1)
        np.testing.assert_array_equal(cg_model.spmv(rp, cl, vl, x), oracle.spmv(rp, cl, vl, x))


@pytest.mark.parametrize("name", ["p2d", "irr"])
def test_f64_preconditioned_model_against_the_pcg_checker(name):
    """The checker's own bar for two restatements of the loop is 1e-13 after
    30 bodies (test_checker_variants_agree_after_30_bodies); its exact-dot
    variant is the model's arithmetic, so they are also equal bit for bit."""
    rp, cl, vl, b = pcg_case(name)
    m = 1.0 / diag_of(rp, cl, vl)
    x, k, rr, rz = pcg(rp, cl, vl, b, m, 0.0, exact=True, max_bodies=30)
    run = cg_model.cg(rp, cl, vl, b, 0.0, 30, minv=m, dtype=np.float64)
    print(f"{name}: rel {rel(run.x, x):.3e}, r.r {run.rr[-1]!r} / {rr!r}, r.z {run.rz[-1]!r} / {rz!r}")
    assert run.bodies == k == 30
    assert rel(run.x, x) <= 1e-13
    np.testing.assert_array_equal(run.x, x)
    assert float(run.rr[-1]) == rr and float(run.rz[-1]) == rz


def test_dot_reports_a_sum_on_a_rounding_boundary():
    # 1 + 2^-24 is the midpoint of 1 and 1 + 2^-23: not clear, the bracket is those two
    a = np.array([1.0, 2.0 ** -24], F32)
    val, clear, lo, hi, margin = cg_model.dot(a, np.ones(2, F32))
    assert not clear and margin == 0.0 and (lo, hi) == (F32(1), np.nextafter(F32(1), F32(2)))
    assert val == F32(1)  # the tie goes to even
    # far from a boundary, across a binade edge, cancelling terms
    a = np.array([2.0, -2.0 ** -23, 2.0 ** -26], F32)
    val, clear, lo, hi, _ = cg_model.dot(a, np.ones(3, F32))
    assert clear and lo == val == np.nextafter(F32(2), F32(0)) and hi == F32(2)
    assert cg_model.dot(np.zeros(3, F32), np.ones(3, F32))[:2] == (F32(0), True)


# ---------------------------------------------------------------------------
# the committed f32 cases

@pytest.mark.parametrize("name", list(CASES))
def test_unclear_dots_within_the_cap(name):
    runs = model(name)  # raises TooManyUnclear past the cap on any path
    worst = max(len(r.unclear) for _, r in runs)
    first = runs[0][1]
    n = len(inputs(name)["b"])
    margins = [f"{u.name}@{u.body}:{u.margin:.2f}g" for u in first.unclear]
    print(f"{name}: n = {n}, {first.bodies} bodies, {len(runs)} trajectories, "
          f"at most {worst} dots not clear {margins}")
    assert worst <= cg_model.MAX_UNCLEAR and len(runs) <= 2 ** cg_model.MAX_UNCLEAR
    if name in SMALL:
        assert worst == 0 and len(runs) == 1
    assert all(r.x.dtype == F32 for _, r in runs)
    mat, _, cap, tol_rel, _, _ = CASES[name]
    if tol_rel > 0:  # stopped by the rule, in f32, well below the cap
        assert 12 < first.bodies < n // 4
        # the body after the first r.r at or below tol^2 is the last (Q5)
        tol = F32(inputs(name)["tol"])
        below = [k for k, v in enumerate([first.rr0] + first.rr) if np.sqrt(v) <= tol]
        assert below[0] + 1 == first.bodies
    elif cap < 0:
        assert first.bodies <= n + 1
    else:
        assert first.bodies == cap


WRONG = ["fma_r", "pap_unrounded", "plain_dots"]
# The tiny systems are there for the kernels' edge loads: with one to five
# products per dot they cannot separate summation orders. nt runs one body,
# after which x = x0 + alpha p has not yet seen the r update, and its guard is
# wider than an ulp, so both neighbours of every dot are trajectories: it is
# there for the element-wise non-temporal paths (x after the body, bit for
# bit), not for the dots.
TEETH = [c for c in CASES if not c.startswith("tiny") and c != "nt"]
# Leaving p.Ap's products unrounded moves the sum by about u sqrt(sum t_i^2)
# ~ u sum|t_i| / sqrt(n). The guard is 4 n u^2 sum|t_i|: from n ~ (4 u)^(-2/3) ~
# 26,000 rows on it is the wider of the two, so a dot such a shift can flip
# is a dot that is not clear, and both its values are trajectories. At 69,120
# and 327,680 rows the comparison therefore cannot separate this variant by
# construction (4,000 seeds of p3d swept with the model: no clear dot
# flipped); it is separated at the small sizes, 0.02 ulp of shift per dot
# against a guard of 2e-4 ulp, on the CSR-stream and SELL forms those run.
RARE = {"p3d": ["pap_unrounded"], "lean": ["pap_unrounded"]}


@pytest.mark.parametrize("name", TEETH)
def test_wrong_variants_differ_in_x(name):
    """A wrong variant must differ from EVERY trajectory the device may match."""
    c = inputs(name)
    runs = model(name)
    diffs = {}
    for w in WRONG:
        run = cg_model.cg(c["rp"], c["cl"], c["vl"].astype(F32), c["b"], c["tol"], c["cap"],
                          x0=c["x0"], minv=c["minv"], dtype=F32, wrong=w)
        diffs[w] = min(int(np.count_nonzero(run.x != r.x)) if run.bodies == r.bodies else -1
                       for _, r in runs)
    print(f"{name}: elements of x that differ (-1: another body count): {diffs}")
    assert all(d != 0 for w, d in diffs.items() if w not in RARE.get(name, ())), diffs
