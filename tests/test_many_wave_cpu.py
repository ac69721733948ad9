"""A wave per system in the many-systems solve (cgx_many_set_form; DESIGN.md
§5e), the parts that need no device: the entry points are declared, exported
and bound, the C ABI and the Python class refuse bad arguments before they
touch a device, the C++ example compiles, and every new system the GPU tests
compare bit for bit (tests/many_wave_systems.py) meets the condition that makes
that comparison exact: in the numpy restatement of the loop (tests/cg_model.py,
float64; plain, JACOBI and DIAGONAL) no dot is closer than its guard to a
rounding boundary, so its rounded value does not depend on how the rows are
dealt to lanes, x is finite, and the run ends by the stop rule below its cap.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd import _native
from tests import cg_model
from tests import many_wave_systems as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
NEW_SYMBOLS = ["cgx_many_set_form", "cgx_many_get_form"]


def test_new_symbols_exported_and_bound():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"
        assert s in _native._SIGS, f"{s} has no ctypes signature"
    assert hasattr(cga.ManyCG, "set_form") and isinstance(cga.ManyCG.form, property)
    assert (cga.MANY_FORM_AUTO, cga.MANY_FORM_WORKGROUP, cga.MANY_FORM_WAVE) == (0, 1, 2)
    assert (cga.ManyCG.FORM_AUTO, cga.ManyCG.FORM_WORKGROUP, cga.ManyCG.FORM_WAVE) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "cgx.h")).read()
    for name, v in (("AUTO", 0), ("WORKGROUP", 1), ("WAVE", 2)):
        assert f"CGX_MANY_FORM_{name} = {v}" in header


def _err():
    return cga.lib().cgx_last_error().decode()


def test_form_calls_refuse_null_and_unknown_without_a_device():
    L = cga.lib()
    assert L.cgx_many_set_form(None, 2) == EINVAL
    assert "NULL handle" in _err()
    req, eff = C.c_int(7), C.c_int(7)
    assert L.cgx_many_get_form(None, C.byref(req), C.byref(eff)) == EINVAL
    assert (req.value, eff.value) == (7, 7)
    fake = 0x5000  # never dereferenced: an unknown form is refused first
    for form in (-1, 3, 17):
        assert L.cgx_many_set_form(fake, form) == EINVAL
        assert f"unknown form {form}" in _err()


def test_python_class_refuses_an_unknown_form_before_any_device_call():
    m = object.__new__(cga.ManyCG)
    m.nsys, m.n, m.nnz, m._h = 3, 12, 40, None  # no handle: a device call would fail
    for form in (-1, 3, "wave", None, 2.0, True):
        with pytest.raises(ValueError, match="unknown form"):
            m.set_form(form)


def test_many_wave_check_compiles(tmp_path):
    out = str(tmp_path / "many_wave_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "many_wave_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_sets_have_the_sizes_the_wave_form_branches_on():
    sizes = {name: (len(W.system_set(name)[0]) - 1, len(W.system_set(name)[2]))
             for name in W.ALL_SETS}
    assert sizes == {"w63x41": (63, 41), "w65x21": (65, 21), "w255x13": (255, 13),
                     "n128": (128, 3), "n129": (129, 3)}
    assert all(nsys % 4 for _, nsys in sizes.values())


@pytest.mark.parametrize("kind", ["plain"] + list(W.KINDS))
@pytest.mark.parametrize("name", W.ALL_SETS)
def test_committed_systems_have_no_unclear_dot(name, kind):
    rp, cl, vals, B, tol, X0, max_bodies = W.system_set(name)
    n = len(rp) - 1
    assert X0 is None and max_bodies == -1
    assert vals.shape == (len(B), len(cl)) and B.shape[1] == n and rp[-1] == len(cl)
    m = None
    if kind != "plain":
        m = W.precond(name, W.KINDS[kind])
        assert m.shape == B.shape and np.isfinite(m).all() and (m > 0).all()
    bodies = []
    for s in range(len(vals)):
        run = cg_model.cg(rp, cl, vals[s], B[s], tol, -1, minv=None if m is None else m[s],
                          dtype=np.float64)
        assert not run.unclear, f"{name}[{s}] {kind}: {len(run.unclear)} dots are not clear"
        assert np.isfinite(run.x).all()
        began = ([run.rr0] + run.rr)[-2]  # the r.r the last body began with
        assert bool(np.sqrt(began) <= tol), f"{name}[{s}] {kind}: not ended by the stop rule"
        assert run.bodies < n + 1, f"{name}[{s}] {kind}: {run.bodies} bodies, the cap"
        bodies.append(run.bodies)
    k = ["plain", "jacobi", "diagonal"].index(kind)
    assert (min(bodies), max(bodies)) == W.BODIES[name][k], bodies
    if name in W.W_SETS and kind == "plain":  # waves of one workgroup finish apart
        assert len(set(bodies)) >= 3, bodies
        assert any(len(set(bodies[i:i + 4])) > 1 for i in range(0, len(bodies) - 3, 4))
    if name == "n129" and kind == "plain":
        assert bodies == [75, 105, 123]
