// podworker device code — built on its own as a plain gfx950 ELF code object
// (hipcc --cuda-device-only --no-gpu-bundle-output) and embedded in the host
// program, which loads it through the ROCr loader and dispatches it with AQL
// packets (see podworker.hip).
//
// The host fills in no hidden kernel arguments, so neither kernel may read
// blockDim/gridDim: the workgroup size is fixed at 256 and the index comes
// from the workgroup-id and workitem-id registers alone.

#include <hip/hip_runtime.h>

#define PW_BLOCK 256

static __device__ __forceinline__ int pw_global_index() {
  return static_cast<int>(__builtin_amdgcn_workgroup_id_x()) * PW_BLOCK +
         static_cast<int>(__builtin_amdgcn_workitem_id_x());
}

// out[i] = 2*i + 1 (mod 2^32) for i < n.
extern "C" __global__ void __launch_bounds__(PW_BLOCK)
touch_kernel(unsigned int* out, int n) {
  int i = pw_global_index();
  if (i < n) out[i] = static_cast<unsigned int>(i) * 2u + 1u;
}

// dst[j] = src[idx[j]] for j < m: brings the sampled words back to
// host-visible memory without a copy call.
extern "C" __global__ void __launch_bounds__(PW_BLOCK)
gather_kernel(const unsigned int* src, const int* idx, unsigned int* dst,
              int m) {
  int j = pw_global_index();
  if (j < m) dst[j] = src[idx[j]];
}
