"""Multi-shift CG (cgx_cg_solve_shifted), the parts that need no
device: the ABI's symbols, the scalar step (cgx_shift.h, the function the
kernel calls) against the model's scalars bit for bit, the model
(tests/shift_model.py) against direct solves and against cg_model, and the
Python layer's refusals.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from tests import cg_model, shift_model
from tests.util import irregular_spd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["cgx_cg_solve_shifted", "cgx_cg_shifted_zeta"]
EINVAL = 1
SIGMAS = [0.0, 1e-3, 0.05, 1.0, 30.0]


def dense_spd(n):
    m = np.random.default_rng(100 + n).standard_normal((n, n))
    a = m @ m.T + n * np.eye(n)
    rp = np.arange(0, n * n + 1, n, dtype=np.int32)
    cl = np.tile(np.arange(n, dtype=np.int32), n)
    return rp, cl, a.ravel().copy(), a


@functools.lru_cache(maxsize=None)
def irr_run():
    rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
    b = np.random.default_rng(21).standard_normal(len(rp) - 1)
    return shift_model.cg_shifted(rp, cl, vl, b, SIGMAS + [1e3, 1e5], 0.0, 60)


def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    hdr = open(os.path.join(ROOT, "include", "cgx.h")).read()
    assert "enum { CGX_SHIFT_MAX = 8 };" in hdr
    doc = hdr[:hdr.index("int cgx_cg_solve_shifted(")]
    doc = doc[doc.rindex("/* ----"):]
    assert "replaces\n * nothing in the reference" in doc or "replaces nothing in the reference" in doc
    for line in ("t1 = (a * bp) * (zp - zc)", "t2 = (zp * ap) * (1 + sigma * a)",
                 "zn = ((zc * zp) * ap) / (t1 + t2)", "bs = (bt * q) * q"):
        assert line in doc
    assert hasattr(cga.CG, "solve_shifted") and cga.CG.MAX_SHIFTS == 8
    cpp = open(os.path.join(ROOT, "include", "CG.hpp")).read()
    for name in ("solveShifted", "shiftedIterations", "shiftedResidual", "shiftedStopped"):
        assert name in cpp


def test_refusals_need_no_device():
    """NULL or made-up handles: the refusal comes before anything reads them."""
    L = cga.lib()
    sg = (_native.C.c_double * 8)(*([0.5] * 8))
    out_b, out_r = (_native.C.c_int64 * 8)(), (_native.C.c_double * 8)()
    assert L.cgx_cg_solve_shifted(None, 1, sg, 0x1000, 0x1000, 8, 0.0, -1, out_b, out_r, None) \
        == EINVAL
    fake = 0x5000  # never dereferenced: nshift is checked first
    for k in (0, -1, 9):
        assert L.cgx_cg_solve_shifted(fake, k, sg, 0x1000, 0x1000, 8, 0.0, -1, out_b, out_r,
                                      None) == EINVAL
        assert b"1 to 8 shifts" in L.cgx_last_error()
    assert L.cgx_cg_shifted_zeta(None, out_r) == EINVAL


def test_python_class_refuses_before_any_device_call():
    cg = object.__new__(cga.CG)  # no queue, no solver: a device call would raise
    cg.dtype = np.dtype(np.float64)
    for bad in ([], [0.1] * 9, [[0.1, 0.2]]):
        with pytest.raises(ValueError, match="1 to 8 shifts"):
            cg.solve_shifted(bad)
    for bad in ([-1e-300], [0.0, np.nan], [np.inf], [1.0, -0.5]):
        with pytest.raises(ValueError, match="finite and not negative"):
            cg.solve_shifted(bad)


def test_shift_step_check_equals_the_models_scalars(tmp_path):
    """examples/shift_step_check.cpp (g++, no contraction) on the alpha, beta
    and r.r sequences the model recorded: every zeta of every shift, bit for
    bit, and the body that freezes it."""
    exe = str(tmp_path / "shift_step_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "conjugategradient_amd", "csrc"),
                        os.path.join(ROOT, "examples", "shift_step_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    run = irr_run()
    sig = SIGMAS + [1e3, 1e5]
    nb = len(run.alphas)
    assert nb == 60
    # r.r at the start of body n: recovered exactly, beta_n = rr_n / rxr_n is
    # not invertible, so the model's own sequence is rebuilt from a rerun
    rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
    b = np.random.default_rng(21).standard_normal(len(rp) - 1)
    base = cg_model.cg(rp, cl, vl, b, 0.0, 60, dtype=np.float64)
    rxr = [base.rr0] + list(base.rr[:-1])
    for tol in (0.0, 1e-3):
        inp = tmp_path / f"in{tol}.bin"
        with open(inp, "wb") as f:
            np.array([nb, len(sig)], np.int64).tofile(f)
            np.array(run.alphas, np.float64).tofile(f)
            np.array(run.betas, np.float64).tofile(f)
            np.array(rxr, np.float64).tofile(f)
            np.array(sig, np.float64).tofile(f)
            np.array([tol], np.float64).tofile(f)
        p = subprocess.run([exe, str(inp)], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr
        lines = p.stdout.strip().split("\n")
        assert len(lines) == len(sig)
        for s, line in enumerate(lines):
            *hexes, state = line.split()
            got = np.array([int(h, 16) for h in hexes], np.uint64).view(np.float64)
            want = np.array(shift_model.zeta_sequence(run.alphas, run.betas, sig[s], rxr, tol))
            np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
            if tol == 0.0:  # the full run's own zetas
                full = np.array(run.zetas[s])
                np.testing.assert_array_equal(got.view(np.uint64), full.view(np.uint64))
                assert state == ("stop" if run.codes[s] == 1 else "run")
    # sigma = 0: zeta stays 1 exactly; sigma = 1e5 leaves the normal range
    assert all(z == 1.0 for z in run.zetas[0])
    assert run.codes[6] == 1 and run.bodies[6] < 60 and not abs(run.zetas[6][-1]) >= shift_model.DBL_MIN
    assert np.isfinite(run.X).all()


@pytest.mark.parametrize("n", [63, 257])
def test_model_agrees_with_direct_solves(n):
    rp, cl, vl, a = dense_spd(n)
    b = np.random.default_rng(21).standard_normal(n)
    sig = [0.0, 0.5, 7.0, 300.0]
    run = shift_model.cg_shifted(rp, cl, vl, b, sig, 1e-10, -1)
    assert run.codes == [1] * len(sig)
    for s, sg in enumerate(sig):
        want = np.linalg.solve(a + sg * np.eye(n), b)
        # the shift froze on |zeta| ||r|| <= 1e-10; the true residual follows
        # the recurrence's to rounding (some 1e-13 here), so 2e-10 bounds it,
        # and A = M M^T + n I puts every eigenvalue of A + sigma I above
        # n + sigma: ||x - x*|| <= ||residual|| / (n + sigma)
        true = np.linalg.norm(b - (a + sg * np.eye(n)) @ run.X[:, s])
        assert true <= 2e-10, (sg, true)
        assert np.linalg.norm(run.X[:, s] - want) <= 2e-10 / (n + sg), sg
    assert run.bodies[0] >= run.bodies[1] >= run.bodies[2] >= run.bodies[3]


def test_sigma_zero_column_is_cg_models_x():
    for n in (1, 2, 63):
        rp, cl, vl, _ = dense_spd(n)
        b = np.random.default_rng(21).standard_normal(n)
        ref = cg_model.cg(rp, cl, vl, b, 1e-10, -1, dtype=np.float64)
        run = shift_model.cg_shifted(rp, cl, vl, b, [0.05, 0.0, 1.0], 1e-10, -1)
        np.testing.assert_array_equal(run.X[:, 1], ref.x)
        assert run.bodies[1] == ref.bodies
    rp, cl, vl = irregular_spd(4097, hub=300, seed=3)
    b = np.random.default_rng(21).standard_normal(len(rp) - 1)
    ref = cg_model.cg(rp, cl, vl, b, 0.0, 60, dtype=np.float64)
    run = irr_run()
    np.testing.assert_array_equal(run.X[:, 0], ref.x)
    assert run.bodies[0] == ref.bodies == 60 and run.codes[0] == 2
    assert len(run.unclear) == len(ref.unclear) == 0
