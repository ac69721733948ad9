"""Per-kernel timing (cgx_cg_set_kernel_timing): every timed
kernel launch takes the start / stop events its dispatch records
(hipExtLaunchKernel), the kernel's own duration as rocprofv3 reports it,
beside the event pair around the launch (dispatch latency included). bench.py
prices the roofline on the former. The timed run's x equals an untimed
(graph-replayed) run's bit for bit: the events change no kernel.

The launches of every mode's body are pinned through the timing counts: 24
bodies in chunks of 8 under a cap of 25 (tol 0, so every body is active) give
one init launch and, per kernel id, the launches the driver makes for 24
bodies. Mode 7 ends the body of every fourth slot with the walk that also
applies the group's x updates, counted under id 3: 18 and 6. Mode 5 makes one
launch per chunk of 64 bodies."""
import ctypes as C

import numpy as np
import pytest

import conjugategradient_amd as cga
from conjugategradient_amd._native import F64, check, lib

pytestmark = pytest.mark.gpu

KVL = 33554432  # the lean stencil walk's variant bit
CALLS = {1: [1, 24, 24, 24], 3: [1, 24, 24, 24], 6: [1, 24, 24, 24],
         2: [1, 24, 24, 0], 4: [1, 24, 24, 0],
         7: [1, 24, 18, 6],
         5: [1, 1, 0, 0]}


def _run(L, q, A, mode, timing, bodies=24):
    n = A.N()
    b = cga.DeviceArray(q, n, np.float64)
    x = cga.DeviceArray(q, n, np.float64)
    check(L.cgx_iota(q.handle, F64, b.ptr, n, 0.0))
    x.fill(0.0)
    cg = C.c_void_p()
    check(L.cgx_cg_create(q.handle, A.schedule(), C.byref(cg)))
    try:
        check(L.cgx_cg_config(cg, 8, 1))
        check(L.cgx_cg_set_mode(cg, mode))
        check(L.cgx_cg_set_kernel_timing(cg, 1 if timing else 0))
        check(L.cgx_cg_begin(cg, b.ptr, x.ptr, 0.0, bodies + 1))
        tot, st = C.c_int64(), C.c_int()
        check(L.cgx_cg_run(cg, bodies, C.byref(tot), C.byref(st)))
        check(L.cgx_sync(q.handle))
        assert tot.value == bodies and st.value == 0, (tot.value, st.value)
        d, dc = (C.c_double * 4)(), (C.c_int64 * 4)()
        e, ec = (C.c_double * 4)(), (C.c_int64 * 4)()
        check(L.cgx_cg_kernel_times(cg, d, dc))
        check(L.cgx_cg_kernel_exec_times(cg, e, ec))
        return x.download(), list(d), list(dc), list(e), list(ec)
    finally:
        L.cgx_cg_destroy(cg)


def _matrix(L, queue, mode):
    if mode == 5:  # the persistent body: a small 2-D problem
        return cga.Matrix.poisson(queue, 2, 128, 128)
    if mode == 7:  # the smallest shape the ring walk takes, the lean walk forced
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("CGX_SPMV_VARIANT", f"{KVL}:0")
            return cga.Matrix.poisson(queue, 3, 256, 128, 128)
    A = cga.Matrix.poisson(queue, 3, 128, 128, 64)
    if mode == 6:  # (Ap recomputed: the lean walk's mode; forced at this size)
        check(L.cgx_csr_set_variant(A.schedule(), KVL))
    return A


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5, 6, 7])
def test_dispatch_recorded_kernel_times(queue, mode):
    L = lib()
    A = _matrix(L, queue, mode)
    x_t, d, dc, e, ec = _run(L, queue, A, mode, True)
    x_g, *_ = _run(L, queue, A, mode, False)
    np.testing.assert_array_equal(x_t, x_g)
    print(f"mode {mode}: launches {dc}, dispatch-recorded {ec}")
    assert dc == CALLS[mode], (mode, dc)
    if mode in (2, 5, 7):  # which of their launches record a pair of their own is not pinned
        return
    kernels = (1, 2) if mode == 4 else (1, 2, 3)
    for k in kernels:
        # every timed launch of the body's kernels recorded its own pair
        assert dc[k] > 0 and ec[k] == dc[k], (k, dc, ec)
        # the kernel alone takes no longer than the launch around it
        assert 0.0 < e[k] <= d[k] * 1.0001, (k, d, e)
