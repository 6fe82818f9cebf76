#!/usr/bin/env python3
"""The device-array entry points against the host forms: python tools/device_io_bench.py [c,L ...]
(default 9,7 and 9,6: 513^3 and 257^3, constant operator, Dirichlet faces, V(2,2), theta = 1, dt = 1e-3).

Per size, STEPS steps per timed run, RUNS runs after a warm-up, median (min .. max):
  host    ms per step of a loop that replaces the source every step: step_set_source(numpy) + step_advance(1, cycles=2)
  tensor  the same loop through step_set_source_tensor (two tensors on the GPU, alternating) + step_advance(1, cycles=2)
  fixed   ms per step of step_advance(STEPS, cycles=2) with a source that stays: the floor of the two loops
  pack    ms per launch of the pack and of the unpack kernel from the library's "pack" kernel timer (timing mode 3, in runs
          of their own: the markers cost idle queue time), for a contiguous float64, a contiguous float32 and a
          permute(2,1,0) float64 tensor
  copy2d  ms per hipMemcpy2DAsync device to device of the same shape (dense rows into the padded pitch), REPS copies
          between one event pair: what the host forms do, applied device to device
and the decision the contiguous-float64 pack rests on: kernel against copy2d."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the HIP runtime is torch's

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_parallel_amd as M
from multigrid_parallel_amd.binding import MG3D_R, MG3D_U

RUNS = int(os.environ.get("RUNS", "5"))
STEPS = int(os.environ.get("STEPS", "20"))
REPS = int(os.environ.get("REPS", "10"))
DT = 1e-3


def guess(N):
    x = np.sin(np.pi * np.linspace(0.0, 1.0, N))
    return np.ascontiguousarray(x[:, None, None] * x[None, :, None] * x[None, None, :])


def spread(ts, unit=1e3):
    return f"{statistics.median(ts) * unit:9.3f} ms (min {min(ts) * unit:.3f}, max {max(ts) * unit:.3f}, {len(ts)} runs)"


def timed(fn, per):
    fn()  # warm-up: first launches, chunk tuning
    out = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) / per)
    return out


def pack_ms(s):
    calls, secs = s.kernel_times().get((s.num_levels - 1, "pack"), (0, 0.0))
    return secs / calls if calls else float("nan")


def kernel_runs(s, call):
    """RUNS x (REPS launches under the kernel timer) -> seconds per launch of each run"""
    call()
    s.sync()
    out = []
    for _ in range(RUNS):
        s.timing_enable(3)
        s.timing_reset()
        for _ in range(REPS):
            call()
        out.append(pack_ms(s))
        s.timing_enable(0)
    return out


def hip_runtime():
    """the HIP runtime this process already uses (torch's), by its path in the process map"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    if not paths:
        raise RuntimeError("no libamdhip64 in this process")
    rt = C.CDLL(paths[0])
    rt.hipMemcpy2DAsync.restype = C.c_int
    rt.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    return rt


def copy2d_runs(rt, N):
    pitch = (N + 15) & ~15
    src = torch.rand(N, N, N, dtype=torch.float64, device="cuda")
    dst = torch.zeros(N * N * pitch, dtype=torch.float64, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = rt.hipMemcpy2DAsync(dst.data_ptr(), pitch * 8, src.data_ptr(), N * 8, N * 8, N * N, 3, stream)  # 3: device to device
        if rc != 0:
            raise RuntimeError(f"hipMemcpy2DAsync: {rc}")

    copy()
    torch.cuda.synchronize()
    assert torch.equal(dst.view(N, N, pitch)[:, :, :N], src)
    out = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            copy()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / REPS)
    return out


def main():
    cases = [tuple(int(v) for v in a.split(",")) for a in sys.argv[1:]] or [(9, 7), (9, 6)]
    rt = hip_runtime()
    for c, L in cases:
        with M.Solver(c, L, 2) as s:
            N, top = s.N, L - 1
            s.get_details()
            s.step_setup(DT, 1.0)
            u0 = guess(N)
            rng = np.random.default_rng(N)
            src_h = [rng.uniform(-1, 1, (N, N, N)) for _ in range(2)]
            src_d = [torch.from_numpy(a).cuda() for a in src_h]
            print(f"{N}^3 V(2,2), constant, Dirichlet faces, dt = {DT}, theta = 1, {STEPS} steps per run, 2 cycles per step:")

            def host_loop():
                for n in range(STEPS):
                    s.step_set_source(src_h[n & 1])
                    s.step_advance(1, cycles=2)
                s.sync()

            def tensor_loop():
                for n in range(STEPS):
                    s.step_set_source_tensor(src_d[n & 1])
                    s.step_advance(1, cycles=2)
                s.sync()

            def fixed():
                s.step_advance(STEPS, cycles=2)
                s.sync()

            t = {}
            for name, fn, label in (("host", host_loop, "step_set_source(numpy) + step_advance(1)"),
                                    ("tensor", tensor_loop, "step_set_source_tensor + step_advance(1)"),
                                    ("fixed", fixed, f"step_advance({STEPS}), the source stays")):
                s.upload(MG3D_U, top, u0)
                s.step_set_source(src_h[0])
                t[name] = timed(fn, STEPS)
                print(f"  {name:7s}{label:44s}{spread(t[name])} per step")
            m = {k: statistics.median(v) * 1e3 for k, v in t.items()}
            # the kernels, under the event pairs
            f64 = src_d[0]
            views = (("contiguous float64", f64), ("contiguous float32", f64.float()),
                     ("permute(2,1,0) float64", f64.permute(2, 1, 0)))
            k = {}
            for label, v in views:
                k[label, "pack"] = kernel_runs(s, lambda: s.upload_tensor(MG3D_R, top, v))
                k[label, "unpack"] = kernel_runs(s, lambda: s.download_tensor(MG3D_R, top, out=v))
                for what in ("pack", "unpack"):
                    print(f"  {what:7s}{label:44s}{spread(k[label, what])} per launch")
            cp = copy2d_runs(rt, N)
            print(f"  copy2d {'hipMemcpy2DAsync device to device':44s}{spread(cp)} per copy")
            pk, c2 = statistics.median(k["contiguous float64", "pack"]) * 1e3, statistics.median(cp) * 1e3
            print(f"  tensor - fixed = {m['tensor'] - m['fixed']:.3f} ms per step (one pack launch: {pk:.3f} ms); "
                  f"host / tensor = {m['host'] / m['tensor']:.1f}")
            print(f"  contiguous float64: pack kernel {pk:.3f} ms, copy2d {c2:.3f} ms -> "
                  f"{'the kernel stays' if pk <= c2 else 'copy2d is faster'}", flush=True)


if __name__ == "__main__":
    main()
