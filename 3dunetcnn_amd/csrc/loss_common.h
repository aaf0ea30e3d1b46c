// What the loss kernels of loss_optim.hip and focal.hip share: the target loader, the 256-thread block sum and the finaliser of a streaming
// pass that leaves one partial per block. Included after gfx950_dialect.h and include/mi355_unet3d.h.
#pragma once

// y of class c at voxel v of sample n, for the three target kinds: fp32 / uint8 of the logits' shape [N][C][V], or an int32 label map [N][V]
__device__ __forceinline__ float loss_target(const void* target, int kind, long long V, int C, long long n, int c, long long v) {
  if (kind == MI355_DICE_TARGET_LABELS) return ((const int*)target)[(size_t)n * V + v] == c ? 1.f : 0.f;
  const size_t i = ((size_t)n * C + c) * V + v;
  return kind == MI355_DICE_TARGET_U8 ? (float)((const unsigned char*)target)[i] : ((const float*)target)[i];
}

// Sum of v over the 256 threads of the block, left in red[0] for thread 0 to read. The order is fixed -- s = 128, 64, ... 1 over
// red[t] += red[t + s] -- so a sum has the same bits on every call. A caller that reuses `red` puts a barrier before the next sum.
template <typename T>
__device__ __forceinline__ void block_sum_256(T* red, T v) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
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
