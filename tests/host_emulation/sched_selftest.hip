// TEST INFRASTRUCTURE, host emulation only (tests/emu_backend.py compiles this file into the emulation library; it is no part of
// pointcept_amd and is never built for or run on a GPU).  Two kernels that pin what the emulator's schedules (hip/hip_runtime.h,
// PTC_EMU_SCHED) can and cannot see -- tests/test_emulation_wave_skew_cpu.py.
//
// One workgroup of WAVES waves, ITERS iterations.  In iteration `it` every wave writes its LDS row (value 1000 (it + 1) + 64 wave + lane),
// the workgroup meets, and every wave reads the row of its neighbour (wave + 1) % WAVES; the value passes through a shuffle (a wave
// collective, as the MFMAs between a real kernel's LDS read and its next write are) and goes to out[it][wave][lane ^ 1].
//   BARRIER = true   the workgroup meets again at the end of the iteration: the neighbour's row cannot change under the read.
//   BARRIER = false  it does not: a wave that is ahead writes its row of iteration it + 1 while its neighbour has yet to read that of `it`.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SST_WAVES 4
#define SST_ITERS 2

template <bool BARRIER>
__global__ void sched_selftest_kernel(int32_t* out) {
  __shared__ int32_t row[SST_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int it = 0; it < SST_ITERS; ++it) {
    row[wave][lane] = 1000 * (it + 1) + 64 * wave + lane;
    __syncthreads();
    const int32_t v = row[(wave + 1) % SST_WAVES][lane];
    out[(it * SST_WAVES + wave) * 64 + (lane ^ 1)] = __shfl_xor(v, 1);
    if (BARRIER) __syncthreads();
  }
}

// out: int32 [SST_ITERS][SST_WAVES][64]
extern "C" int emu_sched_selftest(int with_barrier, int32_t* out) {
  if (with_barrier) hipLaunchKernelGGL(sched_selftest_kernel<true>, dim3(1), dim3(SST_WAVES * 64), 0, nullptr, out);
  else hipLaunchKernelGGL(sched_selftest_kernel<false>, dim3(1), dim3(SST_WAVES * 64), 0, nullptr, out);
  return 0;
}
