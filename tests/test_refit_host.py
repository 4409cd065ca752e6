"""CPU tests of the refit entry point's boundary (rt_refit_mesh_device / Renderer.refit_mesh_device): the library exports and
binds it, a NULL context is refused without a GPU, and the Python wrapper refuses what is not a float32 device tensor before
it calls the library.  The refit itself is tested on the GPU (tests/test_gpu_refit.py)."""
import ctypes as C

import numpy as np
import pytest

import raytracing_engine_amd as R
from raytracing_engine_amd import _lib


def test_refit_is_exported_and_bound():
    lib = R.load()
    assert "rt_refit_mesh_device" in _lib.PROTOTYPES
    assert lib.rt_refit_mesh_device(None, None, 0) == -1  # RT_ERR_INVALID: no context, nothing touched
    assert lib.rt_refit_mesh_device(None, C.c_void_p(16), 1) == -1


def test_refit_wrapper_checks_its_tensor_before_the_library():
    torch = pytest.importorskip("torch")
    r = R.Renderer.__new__(R.Renderer)  # no context: every argument below must be refused before the library is called
    r._lib, r._ctx, r.device = None, None, 0
    v = np.zeros((4, 9), np.float32)
    for bad in (v, torch.from_numpy(v), torch.from_numpy(v).double(), torch.from_numpy(v).t(), torch.zeros(4, 8)):
        with pytest.raises(ValueError):
            r.refit_mesh_device(bad)
