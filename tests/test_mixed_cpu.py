"""The mixed-precision solve (cgx_mixed), the parts that need no
device: tests/mixed_model.py, the numpy model the device is held to bit for
bit (tests/test_gpu_mixed.py), on the committed cases (CASES, imported from
here):

  - every case has at most cg_model.MAX_UNCLEAR dots that are not clear,
    counted over the outer r.r and every inner solve, on every trajectory;
  - the model reaches the tolerance in the outer steps and inner bodies
    recorded here (DESIGN.md §5d's table), and the plain f64 model's body count
    stands beside them;
  - the three other statuses: stagnation at tol 0, the body cap on the scaled
    matrix without a preconditioner, NaN at n = 1 with x untouched;
  - three deliberately wrong variants (the cast truncated, the up-add fused
    with a scale that is not a power of two, r.r summed in index order) change
    x or the history, so the bit comparison on the device separates them;
  - the entry points are declared and exported, solve_mixed's argument errors
    come before any device call, examples/mixed_check.cpp compiles.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from tests import cg_model, mixed_model
from tests.test_cg_model_cpu import TINY, _dense_csr, _tridiag
from tests.test_pcg_cpu import case as pcg_case, diag_of
from tests.util import irregular_spd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cgx_mixed_create", "cgx_mixed_destroy", "cgx_mixed_config", "cgx_mixed_set_mode",
               "cgx_mixed_set_precond", "cgx_mixed_solve", "cgx_mixed_history", "cgx_mixed_inner",
               "cgx_mixed_bytes"]

# name: (matrix, relative tol, inner modes the GPU file runs, options)
#   matrix: ("poisson", dim, nx, ny, nz) | ("irr",) | ("tiny", n) | ("pcg", name)
#   options: precond "jacobi" | "diag" (the caller's 1 / diag(A) in f64), x0,
#   max_bodies, inner_cap, max_outer
CASES = {
    "p2d": (("poisson", 2, 33, 31, 1), 1e-8, (1, 3), {}),
    "p3d": (("poisson", 3, 24, 20, 16), 1e-8, (1, 3), {}),
    "irr": (("irr",), 1e-8, (1,), {}),
    "jacobi": (("pcg", "p2d"), 1e-8, (1, 3), {"precond": "jacobi"}),
    "diag": (("pcg", "p2d"), 1e-8, (1, 3), {"precond": "diag"}),
    "x0": (("poisson", 2, 33, 31, 1), 1e-8, (1,), {"x0": True}),
    "tiny2": (("tiny", 2), 1e-12, (1,), {}),
    "tiny3": (("tiny", 3), 1e-12, (1,), {}),
    "tiny5": (("tiny", 5), 1e-12, (1,), {}),
    # the other statuses
    "stagnate": (("poisson", 2, 33, 31, 1), 0.0, (1,), {}),
    "cap": (("pcg", "p2d"), 1e-8, (1,), {}),
    "nan1": (("tiny", 1), 1e-8, (1,), {}),
    # the lean walk's size, inner auto mode (6): two inner solves of 6 bodies, then max_outer.
    # b = A g, g standard normal: rough enough that 6 bodies more than halve the residual
    # (from b = 1..n they raise it: status 3 after one step); the seed is one whose 29 dots
    # at 327,680 rows are all clear (a condition on the inputs, met by the model alone)
    "lean": (("poisson", 3, 128, 64, 40), 1e-8, (0,),
             {"inner_cap": 6, "max_outer": 2, "b": ("Ag", 36)}),
    # the kernels' tails: one residual, one cast, one inner body, one up-add, one residual.
    # Values, b and x0 with 53 random bits, so every cast rounds; nnz = 3 n - 2 is odd
    "edge1": (("tri", 1), 0.0, (1,), {"inner_cap": 1, "max_outer": 1, "x0": True, "b": ("rand", 5)}),
    "edge3": (("tri", 3), 0.0, (1,), {"inner_cap": 1, "max_outer": 1, "x0": True, "b": ("rand", 5)}),
    "edge5": (("tri", 5), 0.0, (1,), {"inner_cap": 1, "max_outer": 1, "x0": True, "b": ("rand", 5)}),
    "edge1023": (("tri", 1023), 0.0, (1, 3),
                 {"inner_cap": 1, "max_outer": 1, "x0": True, "b": ("rand", 5)}),
    # r s spans 2^-140 .. 1: the components below 2^-126 are f32 subnormals
    "subnormal": (("tri", 67), 0.0, (1,), {"inner_cap": 1, "max_outer": 1, "b": ("span", 140)}),
}
# f64 CG bodies, outer steps, inner bodies per step (DESIGN.md §5d's table)
TABLE = {
    "p2d": (108, 2, [81, 59]),
    "p3d": (89, 2, [59, 41]),
    "irr": (181, 2, [160, 139]),
    "jacobi": (128, 2, [98, 71]),
}
# dots that are not clear, at most, over every trajectory
UNCLEAR = {"p2d": 0, "p3d": 0, "jacobi": 0, "x0": 0, "irr": 2, "diag": 2,
           "tiny2": 0, "tiny3": 0, "tiny5": 0, "lean": 0}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> dict(rp, cl, vl, b, tol, kw): kw the keyword arguments of mixed_model.refine."""
    mat, tol_rel, _, opt = CASES[name]
    if mat[0] == "poisson":
        from oracle import oracle as O
        rp, cl, vl = O.poisson(*mat[1:])
    elif mat[0] == "irr":
        rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
    elif mat[0] == "tiny":
        rp, cl, vl = _dense_csr(TINY[mat[1]])
    elif mat[0] == "tri":  # D^1/2 tridiag(-0.3, 1, -0.3) D^1/2, d uniform in [1, 2): SPD
        d = 1.0 + np.random.default_rng(mat[1]).random(mat[1])
        rp, cl, vl = _dense_csr(_tridiag(d))
    else:
        rp, cl, vl, _ = pcg_case(mat[1])
    rp, cl = np.asarray(rp, np.int32), np.asarray(cl, np.int32)
    vl = np.array(vl, np.float64)
    n = len(rp) - 1
    kind, arg = opt.get("b", ("iota", 0))
    if kind == "iota":
        b = np.arange(1, n + 1, dtype=np.float64)
    elif kind == "rand":
        b = np.random.default_rng(arg).standard_normal(n)
    elif kind == "Ag":
        b = cg_model.spmv(rp, cl, vl, np.random.default_rng(arg).standard_normal(n))
    else:  # "span": random mantissas, exponents falling evenly from 0 to -arg
        m = 1.0 + np.random.default_rng(9).random(n)
        b = np.ldexp(m, -np.round(np.linspace(0, arg, n)).astype(np.int64))
    kw = {}
    if opt.get("precond") == "jacobi":
        kw["precond"] = "jacobi"
    elif opt.get("precond") == "diag":
        kw["precond"] = 1.0 / diag_of(rp, cl, vl)
    if opt.get("x0"):
        kw["x0"] = 0.5 * np.random.default_rng(103).standard_normal(n)
    for k in ("max_bodies", "inner_cap", "max_outer"):
        if k in opt:
            kw[k] = opt[k]
    for a in (rp, cl, vl, b):
        a.setflags(write=False)
    return dict(rp=rp, cl=cl, vl=vl, b=b, tol=tol_rel * float(np.linalg.norm(b)), kw=kw)


@functools.lru_cache(maxsize=None)
def model(name):
    """Every trajectory of the model on a case: [(choices, Result)]. Computed once."""
    c = inputs(name)
    return mixed_model.trajectories(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], **c["kw"])


def _show(name, runs):
    r = runs[0][1]
    nb = np.linalg.norm(inputs(name)["b"])
    print(f"{name}: n = {len(r.x)}, status {r.status}, {r.outer} outer steps, inner bodies "
          f"{[h[1] for h in r.history[1:]]}, rel. residuals "
          f"{['%.2e' % (np.sqrt(h[0]) / nb) for h in r.history]}, "
          f"{len(runs)} trajectories, at most {max(len(q.unclear) for _, q in runs)} dots not clear")


@pytest.mark.parametrize("name", list(CASES))
def test_unclear_dots_within_the_cap(name):
    runs = model(name)  # raises TooManyUnclear past the cap on any path
    _show(name, runs)
    worst = max(len(r.unclear) for _, r in runs)
    assert worst <= cg_model.MAX_UNCLEAR and len(runs) <= 2 ** cg_model.MAX_UNCLEAR
    if name in UNCLEAR:
        assert worst == UNCLEAR[name]
    assert all(r.x.dtype == np.float64 for _, r in runs)


@pytest.mark.parametrize("name", list(TABLE))
def test_reaches_tol_in_the_recorded_steps(name):
    c = inputs(name)
    f64_bodies, outer, inner = TABLE[name]
    # the table's row: every dot rounded to nearest, not clear or not
    r = mixed_model.refine(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], **c["kw"])
    assert [h[1] for h in r.history[1:]] == inner and r.inner_bodies == sum(inner)
    for _, r in model(name):  # every trajectory the device may take gets there
        assert r.status == 1 and r.outer == outer
        assert np.sqrt(r.rxr) <= c["tol"] and r.history[-1][0] == r.rxr
        # the true residual of the x returned, in plain numpy
        assert np.linalg.norm(c["b"] - cg_model.spmv(c["rp"], c["cl"], c["vl"], r.x)) <= c["tol"]
    m = None
    if c["kw"].get("precond") == "jacobi":
        m = 1.0 / diag_of(c["rp"], c["cl"], c["vl"])
    run = cg_model.cg(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], -1, minv=m, dtype=np.float64)
    print(f"{name}: f64 CG {run.bodies} bodies; mixed {inner} in {outer} outer steps "
          f"({sum(inner) / run.bodies:.2f} x)")
    assert run.bodies == f64_bodies


def test_status_3_at_tol_0():
    (_, r), = model("stagnate")
    rel = [np.sqrt(h[0]) / np.linalg.norm(inputs("stagnate")["b"]) for h in r.history]
    assert r.status == 3 and r.outer == 4 and len(r.history) == 5
    assert rel[-1] > 0.5 * rel[-2] and rel[-1] < 1e-13


def test_status_2_at_the_body_cap():
    """The scaled matrix without a preconditioner: f32 CG does not reach 1e-5
    within n + 1 bodies, so the one inner solve spends the whole cap."""
    (_, r), = model("cap")
    n = len(r.x)
    assert r.status == 2 and r.outer == 1 and r.inner_bodies == n + 1
    assert [h[1] for h in r.history] == [0, n + 1]


def test_status_4_at_n_1_leaves_x():
    c = inputs("nan1")
    x0 = np.array([0.125])
    r = mixed_model.refine(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], x0=x0)
    assert r.status == 4 and r.outer == 0 and r.inner_bodies == 0 and len(r.history) == 1
    np.testing.assert_array_equal(r.x, x0)
    (_, r0), = model("nan1")
    assert r0.status == 4 and (r0.x == 0).all()


def _differs(name, wrong):
    c = inputs(name)
    (_, good), = model(name)
    bad = mixed_model.refine(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], wrong=wrong, **c["kw"])
    dx = int(np.count_nonzero(bad.x != good.x))
    dh = bad.history != good.history
    print(f"{name}, {wrong}: {dx} elements of x differ, history differs: {dh}")
    return bool(dx or dh)


@pytest.mark.parametrize("wrong", ["trunc_cast", "fma_scale", "plain_rr"])
def test_wrong_variants_change_x_or_the_history(wrong):
    """On Poisson 33 x 31 from a non-zero x0 (random, 53 bits). The run from
    x0 = 0 cannot separate the cast or the summation order, to 1e-8 ||b|| or
    to stagnation: with b = 1..n and A's entries 4 and -1, x is a short sum of
    f32 vectors times powers of two, A x and b - A x are exact in f64, and the
    residual, cancelled to the size of the last correction's error, fits 24
    bits; its cast is exact whatever the rounding and its squares sum exactly
    in any order (the next test). The fused up-add shows on both."""
    assert _differs("x0", wrong)


def test_from_x0_zero_the_casts_of_p2d_are_exact():
    c = inputs("p2d")
    r = mixed_model.refine(c["rp"], c["cl"], c["vl"], c["b"], c["tol"], max_outer=1)
    res = c["b"] - cg_model.spmv(c["rp"], c["cl"], c["vl"], r.x)
    assert (res.astype(np.float32).astype(np.float64) == res).all()
    assert not _differs("p2d", "trunc_cast") and not _differs("p2d", "plain_rr")
    assert _differs("p2d", "fma_scale")


def test_subnormal_case_separates_a_flushing_cast():
    c = inputs("subnormal")
    nr = float(np.sqrt(cg_model.dot(c["b"], c["b"])[0]))
    r32 = (c["b"] * 2.0 ** -np.frexp(nr)[1]).astype(np.float32)
    sub = (r32 != 0) & (np.abs(r32) < np.finfo(np.float32).tiny)
    print(f"subnormal: {int(sub.sum())} of {len(r32)} components of r32 are subnormal, "
          f"the smallest {float(np.abs(r32).min()):.3e}")
    assert sub.sum() >= 5 and (r32 != 0).all()
    assert _differs("subnormal", "flush")


def test_cast_refusals_of_the_model():
    with pytest.raises(ValueError, match="1 values.*first 2"):
        mixed_model.cast_matrix([1.0, 2.0, 1e300])
    with pytest.raises(ValueError, match="2 values.*first 0"):
        mixed_model.cast_matrix([1e-60, -1e39, 0.0])


# ---------------------------------------------------------------------------
# the interface, without a device

def test_new_symbols_exported():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
    text = open(os.path.join(ROOT, "include", "cgx.h")).read()
    block = text[text.index("---- cgx_mixed"):text.index("/* CG::accuracy")]
    assert block.count("Replaces nothing in the reference") >= len(NEW_SYMBOLS)


def test_solve_mixed_argument_errors_touch_no_device():
    cg = cga.CG(None, np.float32)  # no queue: anything that reached the device would raise otherwise
    with pytest.raises(TypeError, match="float64"):
        cg.solve_mixed(1e-8)
    cg = cga.CG(None)
    for kw in ({"inner_reduction": -1.0}, {"inner_reduction": float("nan")},
               {"inner_reduction": float("inf")}, {"max_outer": -1}, {"inner_cap": -2}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            cg.solve_mixed(1e-8, **kw)
    with pytest.raises(RuntimeError, match="No right hand side"):
        cg.solve_mixed(1e-8)
    assert cg.mixed_status is None and cg.mixed_history is None and cg.outer_steps == 0


def test_mixed_check_compiles(tmp_path):
    out = str(tmp_path / "mixed_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "mixed_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
