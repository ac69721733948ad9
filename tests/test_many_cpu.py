"""Many small systems (cgx_many), the parts that need no device:
the entry points are declared, exported and bound, the C ABI and the Python
class refuse bad arguments before they touch a device, the C++ example
compiles, and every system the GPU tests compare bit for bit
(tests/many_systems.py) meets the condition that makes that comparison
exact: in the numpy restatement of the loop (tests/cg_model.py, float64) no
dot is closer than its guard to a rounding boundary, so its rounded value does
not depend on how the rows are dealt to threads, and the run ends by the stop
rule below its cap.

A system of n <= 2 rows cannot end below its cap: CG needs n bodies and stop
rule Q5 tests the r.r a body began with, so the body that finds it small is
body n + 1, the cap. Those sets are held to "ended by the stop rule" instead.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from tests import cg_model
from tests import many_systems as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = 1, 6
NEW_SYMBOLS = ["cgx_many_create", "cgx_many_destroy", "cgx_many_config", "cgx_many_solve",
               "cgx_many_info"]


def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    assert cga.ManyCG is cga.core.ManyCG and "ManyCG" in cga.__all__


def _create(dtype=_native.F64, nsys=3, n=10, nnz=28, ldv=28, ctx=None, rp=0x1000, cl=0x2000,
            vl=0x3000, out=True):
    """cgx_many_create's return code and message. The pointers are made up:
    a refusal must come before anything reads them (ctx is NULL, so a call
    that passed every argument check ends at the NULL check)."""
    h = C.c_void_p()
    rc = cga.lib().cgx_many_create(ctx, dtype, nsys, n, nnz, rp, cl, vl, ldv,
                                   C.byref(h) if out else None)
    assert not h.value
    return rc, cga.lib().cgx_last_error().decode()


def test_create_refusals_need_no_device():
    rc, msg = _create(dtype=_native.F32)
    assert rc == EUNSUPPORTED and "f32" in msg
    rc, msg = _create(n=4097, nnz=4097, ldv=4097)
    assert rc == EUNSUPPORTED and "4096" in msg and "cgx_cg_solve" in msg
    rc, msg = _create(n=0)
    assert rc == EINVAL and "n 0" in msg
    rc, msg = _create(ldv=27)
    assert rc == EINVAL and "ldv 27" in msg and "nnz 28" in msg
    for nsys in (0, -4):
        rc, msg = _create(nsys=nsys)
        assert rc == EINVAL and f"nsys {nsys}" in msg
    rc, msg = _create(vl=0x3004)
    assert rc == EINVAL and "8-byte aligned" in msg
    rc, msg = _create(rp=0x1002)
    assert rc == EINVAL and "4-byte aligned" in msg
    for kw in ({"rp": None}, {"cl": None}, {"vl": None}, {}):  # ({}: ctx is NULL)
        rc, msg = _create(**kw)
        assert rc == EINVAL and "NULL" in msg
    rc, msg = _create(out=False)
    assert rc == EINVAL and "NULL" in msg
    # n = 4096 is supported: the call gets as far as the NULL context
    rc, msg = _create(n=4096, nnz=4096, ldv=4096)
    assert rc == EINVAL and "NULL" in msg


def test_null_handle_refusals():
    L = cga.lib()
    assert L.cgx_many_config(None, 0) == EINVAL
    assert L.cgx_many_info(None, None, None, None) == EINVAL
    assert L.cgx_many_solve(None, 0x1000, 10, 0x2000, 10, 0.0, -1, None, None, None) == EINVAL
    assert L.cgx_many_destroy(None) == 0


def test_python_class_refuses_before_any_device_call():
    rp, cl, vl = M.poisson2d(4, 3)
    nnz = len(vl)
    vals = np.tile(vl, (3, 1))
    mk = lambda **kw: cga.ManyCG(None, kw.get("rp", rp), kw.get("cl", cl), kw.get("vals", vals),  # noqa: E731
                                 kw.get("g", 0))  # no queue: a device call would raise otherwise
    with pytest.raises(TypeError, match="float64"):
        mk(vals=vals.astype(np.float32))
    with pytest.raises(ValueError, match="2-D"):
        mk(vals=vl)
    with pytest.raises(ValueError, match="at least 1"):
        mk(vals=np.empty((0, nnz)))
    with pytest.raises(ValueError, match="cols has"):
        mk(cl=cl[:-1])
    with pytest.raises(ValueError, match="0 to nnz"):
        mk(rp=rp + 1)
    with pytest.raises(ValueError, match="negative"):
        mk(g=-1)
    big = np.arange(4098, dtype=np.int32)
    with pytest.raises(ValueError, match="1 to 4096 rows"):
        cga.ManyCG(None, big, big[:-1], np.ones((2, 4097)))
    # solve's shape checks, on an object that never reached a device
    m = object.__new__(cga.ManyCG)
    m.nsys, m.n, m.nnz, m._h = 3, 12, nnz, None
    with pytest.raises(ValueError, match="B has shape"):
        m.solve(np.ones((12, 3)))
    with pytest.raises(ValueError, match="X0 has shape"):
        m.solve(np.ones((3, 12)), X0=np.ones((3, 11)))
    with pytest.raises(ValueError, match="vals has shape"):
        m.set_values(np.ones((3, nnz + 1)))


def test_many_check_compiles(tmp_path):
    out = str(tmp_path / "many_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "many_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", M.ALL_SETS)
def test_committed_systems_have_no_unclear_dot(name):
    rp, cl, vals, B, tol, X0, max_bodies = M.system_set(name)
    n = len(rp) - 1
    assert vals.shape == (len(B), len(cl)) and B.shape[1] == n and rp[-1] == len(cl)
    bodies = []
    for s in range(len(vals)):
        run = cg_model.cg(rp, cl, vals[s], B[s], tol, max_bodies,
                          x0=None if X0 is None else X0[s], dtype=np.float64)
        assert not run.unclear, f"{name}[{s}]: {len(run.unclear)} dots are not clear"
        assert np.isfinite(run.x).all()
        by_rule = bool(np.sqrt(([run.rr0] + run.rr)[-2]) <= tol)  # the r.r the last body began with
        if max_bodies >= 0:
            assert run.bodies == max_bodies and not by_rule, f"{name}[{s}]: not ended by the cap"
        else:
            assert by_rule, f"{name}[{s}]: not ended by the stop rule"
            assert run.bodies < n + 1 or n <= 2, f"{name}[{s}]: {run.bodies} bodies, the cap"
        bodies.append(run.bodies)
    if name == "multi":
        assert len(vals) == 37 and len(set(bodies)) >= 3, bodies
    if name == "hub":
        assert np.diff(rp).max() >= 300
    if name == "empty":
        assert (np.diff(rp) == 0).sum() == 1
