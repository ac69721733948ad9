"""conjugategradient_amd — MI355X-native conjugate-gradient solver.

A from-scratch gfx950 engine (libcgx.so: HIP kernels + C ABI, include/cgx.h)
behind the interfaces of XeniaHerr/ConjugateGradient:

* C++: include/CG.hpp, include/VectorOperations.hpp,
  include/LinearAlgebraTypes.hpp (drop-in for src/*.hpp);
* Python: the same classes in ``conjugategradient_amd.core``; the
  Matrix-Market loader (test/mm_reader.cpp read_file) in ``.mtx``.
"""
from ._native import (MANY_FORM_AUTO, MANY_FORM_WAVE, MANY_FORM_WORKGROUP,  # noqa: F401
                      CgxError, device_count, header_symbols, lib)
from .core import (CG, BlockPreconditioner, DeviceArray, Debuglevel, Event,  # noqa: F401
                   ManyCG, Matrix, Preconditioner, Queue, Scalar, Vector, VectorOperations)
from .mtx import read_file, write_mtx_lower  # noqa: F401

__all__ = ["BlockPreconditioner", "CG", "CgxError", "Debuglevel", "DeviceArray", "Event",
           "MANY_FORM_AUTO", "MANY_FORM_WAVE", "MANY_FORM_WORKGROUP", "ManyCG", "Matrix",
           "Preconditioner", "Queue", "Scalar", "Vector", "VectorOperations", "device_count", "header_symbols", "lib",
           "read_file", "write_mtx_lower"]
