// vr_shared.h -- the device helpers that both sides of the library use: the march kernels (vr_kernels.h and the headers behind
// vr_launch.h, compiled once per arithmetic mode) and the kernels of the C ABI's translation unit (the auxiliary kernels and the
// voxel tools).  None of them has a multiply-add of the per-sample kind, so they exist once, in namespace vr.
#pragma once
#include <hip/hip_runtime.h>

namespace vr {

// The wavefront's lane mask of a condition.  (HIP's __ballot takes an int: the condition becomes 0 / 1 in a register and is
// compared again -- v_cndmask + v_cmp and a scalar wait on the vector compare -- where the builtin takes the condition's own mask.)
__device__ __forceinline__ unsigned long long vr_ballot(bool x) { return __builtin_amdgcn_ballot_w64(x); }

// Orders a wavefront's LDS writes before its following LDS reads of the SAME wave-private region (and the reads of one
// tile before the next tile load overwrites them).  A wavefront's LDS instructions execute in issue order, so no s_barrier
// is needed; this only stops the compiler from moving memory operations across it.
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// column-major mat4 * (x,y,z,1), summed left to right
__device__ __forceinline__ void mat4_mul_point(const float* m, float x, float y, float z, float w, float out[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = ((m[0 + r] * x + m[4 + r] * y) + m[8 + r] * z) + m[12 + r] * w;
}

}  // namespace vr
