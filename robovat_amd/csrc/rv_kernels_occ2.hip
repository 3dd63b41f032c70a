// rv_kernels_occ2.hip — the env kernel compiled for two waves per SIMD (see rv_env_kernel.h).
// gfx950 only; built with hipcc --offload-arch=gfx950 into librovat_hip.so next to rv_kernels.hip.
#define RV_ENV_OCCUPANCY_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))      // at most 256 registers per wave
#define RV_SEGMENTS_NOINLINE 1      // the loop inlined into the kernel, the segments of the env program out of line: see env_program
#define k_env k_env_occ2
#include "rv_env_kernel.h"

void rv_launch_k_env_occ2(int mode, const EnvKernelArgs& a, int n_grid, hipStream_t stream) {
  rv_launch_k_env_here(mode, a, n_grid, stream);
}
int rv_k_env_occ2_blocks_per_cu() { return rv_k_env_blocks_per_cu_here(); }
