"""bench.py --dump-outputs: the files hold what the timed run's
caller has after its last step: x with every deferred update applied, and
r.r, as float64 .npy; a long x is written as the fixed sample dump_sample
names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import F64, check, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu


# 22 bodies: the window ends inside a group of four deferred x updates
@pytest.mark.parametrize("mode,sample", [(1, None), (3, None), (3, 1000)])
def test_dump_outputs_holds_x_and_rxr(queue, oracle, tmp_path, monkeypatch, mode, sample):
    L = lib()
    nx = 24
    A = cga.Matrix.poisson(queue, 3, nx, nx, nx)
    n = A.N()
    b = cga.DeviceArray(queue, n, np.float64)
    x = cga.DeviceArray(queue, n, np.float64)
    check(L.cgx_iota(queue.handle, F64, b.ptr, n, 0.0))
    x.fill(0.0)
    if sample:  # a vector longer than the sample: the seeded positions only
        monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    cg = C.c_void_p()
    check(L.cgx_cg_create(queue.handle, A.schedule(), C.byref(cg)))
    try:
        check(L.cgx_cg_config(cg, 8, 1))
        check(L.cgx_cg_set_mode(cg, mode))
        check(L.cgx_cg_begin(cg, b.ptr, x.ptr, 0.0, 22))
        tot, st = C.c_int64(), C.c_int()
        check(L.cgx_cg_run(cg, 22, C.byref(tot), C.byref(st)))
        assert tot.value == 22
        bench.dump_outputs(L, cg, x, str(tmp_path / "out"), 0, 1)
        rxr = C.c_double()
        check(L.cgx_cg_rxr(cg, C.byref(rxr)))
    finally:
        L.cgx_cg_destroy(cg)
    assert sorted(os.listdir(tmp_path / "out")) == ["rxr.npy", "x.npy"]
    xd, rd = np.load(tmp_path / "out" / "x.npy"), np.load(tmp_path / "out" / "rxr.npy")
    assert xd.dtype == np.float64 and rd.dtype == np.float64 and rd.shape == (1,)
    full = x.download()
    idx = bench.dump_sample(n)
    assert (idx is None) == (sample is None)
    np.testing.assert_array_equal(xd, full if idx is None else full[idx])
    assert xd.shape == ((n,) if sample is None else (sample,))
    assert rd[0] == rxr.value and rd[0] > 0.0
    # and it is the solver's x after 22 bodies: the oracle's iteration
    rp, cl, vl = oracle.poisson(3, nx, nx, nx)
    x_ref, res = oracle.cg_solve(rp, cl, vl, np.arange(1, n + 1, dtype=np.float64), 0.0,
                                 max_iter=22)
    assert res.iterations == 22
    assert np.linalg.norm(full - x_ref) <= 1e-10 * np.linalg.norm(x_ref)
