// What the loss kernels of loss_optim.hip and focal.hip share: the target loader, the 256-thread block sum (block_sum_256 of
// volume_common.h, which the volume ops use too) and the finaliser of a streaming pass that leaves one partial per block. Included after
// gfx950_dialect.h and include/mi355_unet3d.h.
#pragma once
#include "volume_common.h"

// y of class c at voxel v of sample n, for the three target kinds: fp32 / uint8 of the logits' shape [N][C][V], or an int32 label map [N][V]
__device__ __forceinline__ float loss_target(const void* target, int kind, long long V, int C, long long n, int c, long long v) {
  if (kind == MI355_DICE_TARGET_LABELS) return ((const int*)target)[(size_t)n * V + v] == c ? 1.f : 0.f;
  const size_t i = ((size_t)n * C + c) * V + v;
  return kind == MI355_DICE_TARGET_U8 ? (float)((const unsigned char*)target)[i] : ((const float*)target)[i];
}

// One block of 256: the B block partials of a streaming pass, summed in double in index order (no floating-point atomics), scaled, then
// written to loss[0] or added to it: loss[0] (+)= (float)(sum * inv_count) * weight.
static __global__ void loss_finalize_kernel(const float* part, int B, double inv_count, float weight, float* loss, int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int b = threadIdx.x; b < B; b += blockDim.x) s += (double)part[b];
  block_sum_256(red, s);
  if (threadIdx.x == 0) {
    const float v = (float)(red[0] * inv_count) * weight;
    loss[0] = accumulate ? loss[0] + v : v;
  }
}
