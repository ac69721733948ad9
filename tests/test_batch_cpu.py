"""Batched CG (cgx_cg_solve_batch), the parts that need no
device: the new entry points are declared and exported, the Python mirror
refuses bad shapes before it touches a device, and the C++ drop-in's
extension compiles."""
import os
import subprocess

import numpy as np
import pytest

import conjugategradient_amd as cga

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["cgx_cg_solve_batch", "cgx_cg_begin_batch", "cgx_cg_run_batch",
               "cgx_cg_set_batch_form", "cgx_cg_batch_info"]


def test_new_symbols_exported():
    syms = cga.header_symbols()
    L = cga.lib()
    for s in NEW_SYMBOLS:
        assert s in syms, f"{s} not declared in include/cgx.h"
        assert hasattr(L, s), f"{s} not exported by libcgx.so"


def test_solve_batch_shape_errors_touch_no_device():
    cg = cga.CG(None)  # no queue: anything that reached the device would raise otherwise
    cg.A._N = 10
    with pytest.raises(ValueError, match="2-D"):
        cg.solve_batch(np.ones(10))
    with pytest.raises(ValueError, match="9 rows"):
        cg.solve_batch(np.ones((9, 2)))
    with pytest.raises(ValueError, match="1 to 8"):
        cg.solve_batch(np.ones((10, 0)))
    with pytest.raises(ValueError, match="1 to 8"):
        cg.solve_batch(np.ones((10, 9)))
    with pytest.raises(ValueError, match="X0 has shape"):
        cg.solve_batch(np.ones((10, 3)), X0=np.ones((10, 2)))
    with pytest.raises(ValueError, match="X0 has shape"):
        cg.solve_batch(np.ones((10, 3), order="F"), X0=np.ones(10))
    assert cg.iterations_batch is None and cg.final_rxr_batch is None
    assert cg.stopped_batch is None and cg.batch_form == 0


def test_batch_check_compiles(tmp_path):
    out = str(tmp_path / "batch_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                        "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", "batch_check.cpp"), "-o", out,
                        "-L" + os.path.join(ROOT, "conjugategradient_amd"), "-lcgx",
                        "-Wl,-rpath," + os.path.join(ROOT, "conjugategradient_amd")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
