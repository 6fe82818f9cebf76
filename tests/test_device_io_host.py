"""Device arrays (mg3d_upload_device, mg3d_download_device, mg3d_step_set_source_device, mg3d_ctx_set_coefficient_device)
without a GPU: the exports, the argument errors that need no device, the new kernel timer's name, the descriptor
array_desc builds from a torch tensor, and that importing the package still does not import torch."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_F32, MG3D_F64, array_desc, mg3d_array

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MG3D_ERR_ARG = 1
NEW = ("mg3d_upload_device", "mg3d_download_device", "mg3d_step_set_source_device", "mg3d_ctx_set_coefficient_device")


def test_the_library_exports_the_four_entry_points():
    L = C.CDLL(M.lib_path())
    for name in NEW:
        assert hasattr(L, name), name


def test_null_context_is_a_bad_argument():
    L = M.lib()
    buf = (C.c_double * 27)()
    a = mg3d_array(C.addressof(buf), MG3D_F64, (C.c_longlong * 3)(9, 3, 1))
    assert L.mg3d_upload_device(None, 0, 0, C.byref(a), None) == MG3D_ERR_ARG
    assert L.mg3d_download_device(None, 0, 0, C.byref(a), None) == MG3D_ERR_ARG
    assert L.mg3d_step_set_source_device(None, C.byref(a), None) == MG3D_ERR_ARG
    assert L.mg3d_ctx_set_coefficient_device(None, C.byref(a), None) == MG3D_ERR_ARG
    assert L.mg3d_step_set_source_device(None, None, None) == MG3D_ERR_ARG
    assert L.mg3d_ctx_set_coefficient_device(None, None, None) == MG3D_ERR_ARG
    assert L.mg3d_last_error()


def test_the_pack_timer_has_a_name():
    L = M.lib()
    names, k = [], 0
    while L.mg3d_kernel_name(k) != b"?":
        names.append(L.mg3d_kernel_name(k).decode())
        k += 1
    assert names[-1] == "pack" and names[-2] == "step_rhs"  # appended at the end: the older timers keep their numbers


def test_array_desc_codes_and_strides():
    import torch
    x = torch.zeros(6, 5, 4, dtype=torch.float64)
    a = array_desc(x)
    assert isinstance(a, mg3d_array)
    assert (a.ptr, a.dtype, list(a.stride)) == (x.data_ptr(), MG3D_F64, [20, 4, 1])
    p = x.permute(2, 1, 0)
    a = array_desc(p, shape=(4, 5, 6))
    assert (a.ptr, a.dtype, list(a.stride)) == (x.data_ptr(), MG3D_F64, [1, 4, 20])
    y = torch.zeros(6, 5, 4, dtype=torch.float32)
    v = y[::2, :, 1:]
    a = array_desc(v, writable=True, shape=(3, 5, 3))
    assert (a.ptr, a.dtype, list(a.stride)) == (y.data_ptr() + 4, MG3D_F32, [40, 4, 1])
    e = torch.tensor(2.5, dtype=torch.float64).expand(7, 7, 7)
    a = array_desc(e)
    assert (a.ptr, a.dtype, list(a.stride)) == (e.data_ptr(), MG3D_F64, [0, 0, 0])


def test_array_desc_refuses_what_the_library_cannot_read():
    import torch
    for bad in (torch.zeros(3, 3, 3, dtype=torch.int64), torch.zeros(3, 3, 3, dtype=torch.float16),
                torch.zeros(3, 3, dtype=torch.float64), [[[1.0]]]):
        with pytest.raises(TypeError):
            array_desc(bad)
    with pytest.raises(ValueError):
        array_desc(torch.zeros(3, 3, 4, dtype=torch.float64), shape=(3, 3, 3))
    e = torch.tensor(1.0).expand(3, 3, 3)
    with pytest.raises(ValueError):
        array_desc(e, writable=True)
    with pytest.raises(ValueError):
        array_desc(torch.zeros(3, 1, 3).expand(3, 3, 3), writable=True)


def test_importing_the_package_does_not_import_torch():
    code = ("import sys; import multigrid_parallel_amd as M; from multigrid_parallel_amd.binding import array_desc; "
            "assert 'torch' not in sys.modules, 'torch was imported'; print('ok')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
