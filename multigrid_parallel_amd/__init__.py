"""multigrid_parallel_amd -- MI355X-native 3D geometric multigrid V-cycle behind the C call surface of
knram06/multigrid_parallel's mg_3d.h.

The product is the C-ABI shared library ``lib/libmg3d.so`` (hand-written HIP for gfx950 + C host side,
sources in ``csrc/``, ABI in ``include/mg3d.h``, drop-in headers ``include/mg_3d.h`` / ``postprocess.h``).
This Python package is only the thin ctypes mirror used by the tests and by bench.py.
"""
from .binding import Solver, Solver32, DistSolver, DistSolver32, EsParams, Mg3dError, lib, lib_path  # noqa: F401
from .binding import MG3D_F32, MG3D_F64, array_desc, mg3d_array, mg3d_vec, vec_desc  # noqa: F401  (device arrays; torch is imported on use only)
from .binding import (MG3D_FATE_ALIVE, MG3D_FATE_FACE, MG3D_FATE_INVALID, MG3D_FATE_SLOTS, MG3D_I32,  # noqa: F401
                      MG3D_PERMUTE_MAX_VECS, mg3d_push_params)  # the particle push and the reorder
