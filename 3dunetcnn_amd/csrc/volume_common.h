// What the volume ops either side of the network share (prepost.hip, augment.hip, components.hip, metrics.hip, intensity.hip): host checks
// and launch arithmetic, wave and block reductions, numpy's linear percentile rule with the radix pick, the sampling set-up and the
// shifted z-score moments. One copy of each. Included after gfx950_dialect.h and include/mi355_unet3d.h.
// The rules all these ops keep: NO WORKGROUP EVER WAITS FOR ANOTHER (no flag, no spin, no grid-wide barrier: what one launch hands to the
// next crosses a kernel boundary); every loop is bounded by an extent; no allocation, copy or host wait; a fixed number of launches.
// Workgroups meet only in INTEGER atomics (order-independent). Floating sums are never atomic: a workgroup adds its own voxels in a
// fixed order into its own slot, and one thread (or one fixed tree) adds the slots -- two calls on the same input give the same bits.
#pragma once

// ---- host side ---------------------------------------------------------------------------------------------------------------------
#define VOL_MAX_VOXELS 2147483646ll         // voxel indices, counts and labels (1 + index) stay in int32

static inline unsigned vol_blocks(long long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

static inline int vol_check_dims(int32_t c, int64_t voxels) { return (c < 1 || c > 65535 || voxels < 1 || voxels > VOL_MAX_VOXELS) ? MI355_EINVAL : MI355_OK; }
static inline int vol_check_dims(int32_t c, int32_t d, int32_t h, int32_t w) { return (d < 1 || h < 1 || w < 1) ? MI355_EINVAL : vol_check_dims(c, (int64_t)d * h * w); }

// a contiguous slice of `per` voxels (a multiple of `granule`) per workgroup, at most max_wg workgroups per channel; *nb = how many
static inline long long vol_slice(long long V, int granule, int max_wg, int* nb) {
  long long per = (V + max_wg - 1) / max_wg;
  per = (per + granule - 1) / granule * granule;
  *nb = (int)((V + per - 1) / per);
  return per;
}

// Only for a source that defines VOL_ZERO_WORDS before the include (hipcc emits a __global__ function whether or not it is launched).
// static: every such source has its own copy (the emulator links all sources into one library).
#ifdef VOL_ZERO_WORDS
static __global__ void zero_words_kernel(int* p, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0;
}
#endif

// ---- wave and block reductions -----------------------------------------------------------------------------------------------------
template <class T> __device__ __forceinline__ T wave_sum(T v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);   // a + b == b + a: every lane ends with the same bits
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned ov = __shfl_xor(v, o); v = ov > v ? ov : v; }
  return v;
}

// Sum of v over the 256 threads of the block, left in red[0] for thread 0 to read. The order is fixed -- s = 128, 64, ... 1 over
// red[t] += red[t + s] -- so a sum has the same bits on every call. A caller that reuses `red` puts a barrier before the next sum.
template <typename T> __device__ __forceinline__ void block_sum_256(T* red, T v) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
}
// ... and of two values at once (the two moments of a z-score), each array in that same order, on one set of barriers
template <typename T> __device__ __forceinline__ void block_sum_256(T* r0, T* r1, T v0, T v1) {
  r0[threadIdx.x] = v0; r1[threadIdx.x] = v1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) { r0[threadIdx.x] += r0[threadIdx.x + s]; r1[threadIdx.x] += r1[threadIdx.x + s]; }
    __syncthreads();
  }
}

// ---- numpy's default ("linear") percentile over a radix select ------------------------------------------------------------------------
// position p = q / 100 * (n - 1); the two ranks are floor(p) and floor(p) + 1 (clamped to n - 1); the value lo + (p - floor(p)) * (hi - lo)
__device__ __forceinline__ double linear_position(double q, int n) { return q / 100.0 * (double)(n - 1); }
__device__ __forceinline__ int linear_rank(double q, int n, bool upper) {
  long long lo = (long long)floor(linear_position(q, n));
  lo = lo < 0 ? 0 : (lo > n - 1 ? n - 1 : lo);
  return (int)(upper && lo + 1 <= n - 1 ? lo + 1 : lo);
}
__device__ __forceinline__ double linear_blend(double lo, double hi, double frac) {
  return hi == lo ? lo : lo + frac * (hi - lo);              // (equal, infinite ones included: no inf - inf)
}
// the bin of a 256-bin histogram that holds rank k (bin 255 if none does); `below` = the count of the bins before it
__device__ __forceinline__ int radix_pick(const int* hist, int k, int& below) {
  int sum = 0, bin = 255;
  for (int b = 0; b < 256; ++b) {
    const int here = hist[b];
    if (k < sum + here) { bin = b; break; }
    sum += here;
  }
  below = sum; return bin;
}

// ---- sampling a source volume of extent (sd, sh, sw) at voxel coordinates (cz, cy, cx) -------------------------------------------------
__device__ __forceinline__ int clamp_index(int v, int n) { return v < 0 ? 0 : (v < n ? v : n - 1); }
__device__ __forceinline__ float clamp_coord(float v, float hi) { return v < 0.f ? 0.f : (v > hi ? hi : v); }

// the nearest source voxel (rintf: half to even; floor_mode: floorf): its linear offset, clamped into the volume; `inside` = it was there
__device__ __forceinline__ size_t nearest_source(float cz, float cy, float cx, bool floor_mode, int sd, int sh, int sw, bool& inside) {
  const float rz = !floor_mode ? rintf(cz) : floorf(cz), ry = !floor_mode ? rintf(cy) : floorf(cy);
  const float rx = !floor_mode ? rintf(cx) : floorf(cx);
  const int iz = (int)rz, iy = (int)ry, ix = (int)rx;
  inside = iz >= 0 && iy >= 0 && ix >= 0 && iz < sd && iy < sh && ix < sw;
  return ((size_t)clamp_index(iz, sd) * sh + clamp_index(iy, sh)) * sw + clamp_index(ix, sw);
}

// The eight corners (k = 4 * dz + 2 * dy + dx) of the cell that holds the point: weights and clamped linear offsets. padding 0 (border):
// the coordinates are clamped into the volume first, which leaves only weight-0 corners outside; padding 1 (zeros): a corner outside
// the volume gets weight 0. Returns whether the three fractions are all zero (the point IS source voxel 0 of the cell).
// wgt / off are the caller's registers: plain force-inlined functions only (a closure put such arrays in scratch). augment_resample_kernel
// writes this loop out: hipcc optimises the helper before inlining it, and that kernel then takes 107 VGPRs for 99 and runs 0.5 % slower.
__device__ __forceinline__ bool trilinear_setup(float cz, float cy, float cx, int sd, int sh, int sw, int padding, float wgt[8], size_t off[8]) {
  if (padding == 0) { cz = clamp_coord(cz, (float)(sd - 1)); cy = clamp_coord(cy, (float)(sh - 1)); cx = clamp_coord(cx, (float)(sw - 1)); }
  const float fz = floorf(cz), fy = floorf(cy), fx = floorf(cx);
  const float lz = cz - fz, ly = cy - fy, lx = cx - fx;
  const int z0 = (int)fz, y0 = (int)fy, x0 = (int)fx;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int a = k >> 2, b = (k >> 1) & 1, e = k & 1;
    int iz = z0 + a, iy = y0 + b, ix = x0 + e;
    float w = (a ? lz : 1.f - lz) * (b ? ly : 1.f - ly) * (e ? lx : 1.f - lx);
    const bool inside = iz >= 0 && iy >= 0 && ix >= 0 && iz < sd && iy < sh && ix < sw;
    if (!inside) {
      if (padding == 1) w = 0.f;
      iz = clamp_index(iz, sd); iy = clamp_index(iy, sh); ix = clamp_index(ix, sw);
    }
    wgt[k] = w; off[k] = ((size_t)iz * sh + iy) * sw + ix;
  }
  return lz == 0.f && ly == 0.f && lx == 0.f;
}
// x pairs first, then y, then z: (v00 + v01) + (v10 + v11), each vXY one product-sum pair
__device__ __forceinline__ float trilinear_blend(const float* s, const float wgt[8], const size_t off[8]) {
  const float v00 = wgt[0] * s[off[0]] + wgt[1] * s[off[1]], v01 = wgt[2] * s[off[2]] + wgt[3] * s[off[3]];
  const float v10 = wgt[4] * s[off[4]] + wgt[5] * s[off[5]], v11 = wgt[6] * s[off[6]] + wgt[7] * s[off[7]];
  return (v00 + v01) + (v10 + v11);
}

// ---- shifted z-score moments ------------------------------------------------------------------------------------------------------
// s0 = sum(x - K), s1 = sum((x - K)^2) over n values, K = the channel's first voxel (the sums carry deviations, not the level):
// mean = K + s0 / n, population variance (torch.std(unbiased=False)) clamped at 0, divisor 0 -> 1 (MONAI NormalizeIntensity)
__device__ __forceinline__ void shifted_mean_rstd(double K, double s0, double s1, double n, float& mean, float& rstd) {
  const double m = K + s0 / n;
  double var = (s1 - s0 * s0 / n) / n; if (var < 0.0) var = 0.0;
  double sd = sqrt(var); if (sd == 0.0) sd = 1.0;
  const float r = (float)(1.0 / sd);
  mean = (float)m; rstd = r;
}
