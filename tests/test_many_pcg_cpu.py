"""Diagonal preconditioning of the many-systems solve (cgx_many_set_precond;
DESIGN.md §5e), the parts that need no device: the entry points are declared,
exported and bound, the C ABI and the Python class refuse bad arguments before
they touch a device, the C++ example compiles, and every system the GPU tests
compare bit for bit (tests/many_pcg_systems.py) meets the condition that makes
that comparison exact: in the numpy restatement of the preconditioned loop
(tests/cg_model.py with minv, float64) no dot is closer than its guard to a
rounding boundary, and the run ends by the stop rule below its cap.

A system of n <= 2 rows cannot end below its cap (tests/test_many_cpu.py);
those sets are held to "ended by the stop rule", where a NaN r.r counts, as
in the kernels: a small system can be solved exactly before the rule sees it,
and the next body then forms 0 / 0. many_pcg_systems.NAN_X lists those.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from tests import cg_model
from tests import many_pcg_systems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESTATE = 1, 4
NEW_SYMBOLS = ["cgx_many_set_precond", "cgx_many_get_precond", "cgx_many_rz"]

# bodies over a set's systems, (JACOBI, DIAGONAL): the model's, recorded
BODIES = {"multi": ((91, 116), (105, 150)), "multi5": ((5, 5), (5, 5)),
          "hub": ((51, 61), (65, 79)), "n1023": ((96, 116), (115, 150)),
          "n4096": ((167, 197), (220, 315))}
MID = ((22, 58), (30, 75))  # n63 ... n257


def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    assert hasattr(cga.ManyCG, "set_preconditioner")


def _err():
    return cga.lib().cgx_last_error().decode()


def test_set_precond_refusals_need_no_device():
    """The handle is NULL or made up: a refusal must come before anything
    reads it. (ldm < n needs a real object: tests/test_gpu_many_pcg.py.)"""
    L = cga.lib()
    fake = 0x5000  # never dereferenced: every call below is refused first
    for kind in (-1, 3, 17):
        assert L.cgx_many_set_precond(fake, kind, 0x1000, 10) == EINVAL
        assert f"unknown kind {kind}" in _err()
    assert L.cgx_many_set_precond(fake, P.DIAGONAL, None, 10) == EINVAL
    assert "NULL" in _err() and "d_M" in _err()
    assert L.cgx_many_set_precond(fake, P.DIAGONAL, 0x1004, 10) == EINVAL
    assert "8-byte aligned" in _err()
    for kind, d in ((P.NONE, None), (P.JACOBI, None), (P.DIAGONAL, 0x1000)):
        assert L.cgx_many_set_precond(None, kind, d, 10) == EINVAL
        assert "NULL handle" in _err()


def test_get_precond_and_rz_refuse_null():
    L = cga.lib()
    kind, rz = C.c_int(7), (C.c_double * 3)()
    assert L.cgx_many_get_precond(None, C.byref(kind)) == EINVAL
    assert L.cgx_many_get_precond(0x5000, None) == EINVAL
    assert kind.value == 7
    assert L.cgx_many_rz(None, rz) == EINVAL
    assert L.cgx_many_rz(0x5000, None) == EINVAL
    assert ESTATE == 4  # (cgx_many_rz's state refusals need an object: the GPU tests)


def test_python_class_refuses_before_any_device_call():
    m = object.__new__(cga.ManyCG)
    m.nsys, m.n, m.nnz, m._h = 3, 12, 40, None  # no queue, no handle: a device call would raise
    with pytest.raises(ValueError, match="unknown preconditioner kind"):
        m.set_preconditioner(5)
    with pytest.raises(ValueError, match="needs diag"):
        m.set_preconditioner(cga.Preconditioner.Diagonal)
    with pytest.raises(ValueError, match="diag has shape"):
        m.set_preconditioner(cga.Preconditioner.Diagonal, np.ones((12, 3)))
    with pytest.raises(ValueError, match="diag has shape"):
        m.set_preconditioner(P.DIAGONAL, np.ones(36))
    # solve's shape checks still work on such an object
    with pytest.raises(ValueError, match="B has shape"):
        m.solve(np.ones((12, 3)))


def test_many_pcg_check_compiles(tmp_path):
    out = str(tmp_path / "many_pcg_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "many_pcg_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _small_clear(n, mseed, vseed):
    from tests import many_systems as M

    rp, cl, vl = M.dense_spd(n, mseed)
    vals, B = M.variants(rp, cl, vl, 3, seed=vseed, width=0.25)
    for kind in (P.JACOBI, P.DIAGONAL):
        for s in range(3):
            m = 1.0 / P.diagonal_of(rp, cl, vals[s])[0]
            if kind == P.DIAGONAL:
                m = m * np.random.default_rng(P.DIAG_SEED + s).uniform(0.5, 2.0, n)
            if cg_model.cg(rp, cl, vals[s], B[s], M._tol(B), -1, minv=m, dtype=np.float64).unclear:
                return False
    return True


def test_small_seeds_are_the_first_clear_ones():
    """The search many_pcg_systems.SMALL_SEEDS records, run again."""
    assert P.SMALL_SEEDS[1] == (101, next(v for v in range(215, 255) if _small_clear(1, 101, v)))
    found = next((ms, vs) for ms in range(102, 140) for vs in range(215, 255)
                 if _small_clear(2, ms, vs))
    assert P.SMALL_SEEDS[2] == found


def _runs(name, kind):
    rp, cl, vals, B, tol, X0, max_bodies = P.system_set(name)
    m = P.precond(name, P.KINDS[kind])
    return [cg_model.cg(rp, cl, vals[s], B[s], tol, max_bodies,
                        x0=None if X0 is None else X0[s], minv=m[s], dtype=np.float64)
            for s in range(len(vals))]


@pytest.mark.parametrize("kind", list(P.KINDS))
@pytest.mark.parametrize("name", P.ALL_SETS)
def test_committed_systems_have_no_unclear_dot(name, kind):
    rp, cl, vals, B, tol, X0, max_bodies = P.system_set(name)
    n = len(rp) - 1
    m = P.precond(name, P.KINDS[kind])
    assert m.shape == B.shape
    if name == "empty":
        assert (np.diff(rp) == 0).sum() == 1 and np.diff(rp)[P.EMPTY_ROW] == 0
        if kind == "jacobi":  # refused on the device (code 3): nothing to model
            assert np.isinf(m[:, P.EMPTY_ROW]).all()
            return
        assert (m[:, P.EMPTY_ROW] == 1.0).all()
    assert np.isfinite(m).all() and (m > 0).all()
    bodies, nan_x = [], []
    for s, run in enumerate(_runs(name, kind)):
        assert not run.unclear, f"{name}[{s}] {kind}: {len(run.unclear)} dots are not clear"
        assert len(run.rz) == run.bodies
        if np.isnan(run.x).any():
            nan_x.append(s)
        began = ([run.rr0] + run.rr)[-2]  # the r.r the last body began with
        by_rule = bool(np.isnan(began)) or bool(np.sqrt(began) <= tol)
        if max_bodies >= 0:
            assert run.bodies == max_bodies and not by_rule, f"{name}[{s}]: not ended by the cap"
        else:
            assert by_rule, f"{name}[{s}] {kind}: not ended by the stop rule"
            assert run.bodies < n + 1 or n <= 2, f"{name}[{s}]: {run.bodies} bodies, the cap"
        bodies.append(run.bodies)
    assert tuple(nan_x) == P.NAN_X.get((name, kind), ()), (name, kind, nan_x)
    k = 0 if kind == "jacobi" else 1
    if name in BODIES:
        assert (min(bodies), max(bodies)) == BODIES[name][k], bodies
    elif name[1:].isdigit() and 63 <= int(name[1:]) <= 257:
        assert MID[k][0] <= min(bodies) and max(bodies) <= MID[k][1], bodies


def test_jacobi_m_is_the_diagonal_summed_in_entry_order():
    rp = np.array([0, 3, 5], np.int32)
    cl = np.array([0, 1, 0, 1, 0], np.int32)       # row 0 holds its diagonal twice
    vl = np.array([1.0, 9.0, 2.0 ** -60, 4.0, 7.0])
    d, found = P.diagonal_of(rp, cl, vl)
    assert found.all() and d[0] == 1.0 + 2.0 ** -60 == 1.0 and d[1] == 4.0
    d, found = P.diagonal_of(rp, np.array([1, 1, 1, 1, 0], np.int32), vl)
    assert not found[0] and d[0] == 0.0 and found[1] and d[1] == 4.0
