// Intensity normalisation on the device: exact per-channel percentiles of a dense, signed fp32 volume, the three window forms built on
// them (clamp, rescale, shift-and-floor), the z-score over a selected set of voxels, and the any-channel threshold mask.
//
// The rules at the top of volume_common.h hold. Every buffer is the caller's and has a closed-form size; everything is enqueued on
// `stream`; a fixed number of launches whatever the data: percentiles 10, window 1, zscore_select 3, threshold_any 1. The integer atomics
// are the histogram bins and the NaN counter; the floating sums are per-workgroup doubles that one thread adds in index order.
//
//   percentiles   radix select over the ORDER-PRESERVING KEY of the fp32 bit pattern (negatives: all bits flipped, the others: the sign
//                 bit flipped; unsigned key order = value order, -0 just below +0, -NaN below -inf, +NaN above +inf): 4 passes of 8 bits
//                 for up to 2 * nq ranks at once. pct_hist_kernel<0> histograms the top byte of every participating voxel (one
//                 histogram serves all ranks) and counts the NaNs; pct_pick_kernel walks the 256 bins to the one that holds each rank;
//                 passes 1..3 histogram the next byte of the voxels whose higher bits equal a rank's prefix. Ranks that still share
//                 their prefix share ONE histogram (the pick kernel names the first such rank their leader), so a voxel matches at
//                 most one histogram and costs at most one LDS atomic per pass, however many ranks are asked for.
//                 THE DOMINANT BIN: a skull-stripped MR channel is more than half exact zeros, and one LDS atomic per voxel would
//                 serialise the whole wave on one address. Before the atomic, the wave takes the bin of its first pending lane,
//                 ballots the lanes that hold the same bin, and that one lane adds their count (PCT_PEEL rounds); only what is left
//                 goes to the LDS lane by lane. On random data a round retires a lane or two and costs two ballots and a broadcast;
//                 on a run of equal values it retires the whole wave with one atomic.
//   window        one launch, 16 bytes per thread where the channel bases allow, element by element elsewhere.
//   zscore_select partials (count, sum and sum of squares of x - pivot in DOUBLE, pivot = the channel's first voxel if finite: the
//                 shifted form loses nothing when the mean is far larger than the spread), a finaliser per channel, and the apply pass,
//                 which forms (x - mean) / std in double and rounds once.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#define VOL_ZERO_WORDS                      // this source launches zero_words_kernel
#include "volume_common.h"

#define IN_WG 1024                          // most workgroups per channel of the streaming kernels = slots of partial sums
#define PCT_PASSES 4                        // radix select: 4 passes of 8 bits over the key
#define PCT_RANKS (2 * MI355_PERCENTILE_MAX_Q)
#define PCT_PEEL 2                          // wave-aggregation rounds before the lane-by-lane LDS atomics

struct PctScratch {                         // per channel
  int hist[PCT_PASSES][PCT_RANKS][256];     // a histogram per pass and leader rank (pass 0: [0][0] only); nothing is zeroed between launches
  unsigned prefix[PCT_RANKS];               // the key bits of each order statistic selected so far
  int rank[PCT_RANKS];                      // its rank among the values that share the prefix
  int leader[PCT_RANKS];                    // the first rank with the same prefix: the owner of the histogram both are read from
  int n, nan;                               // participating values (NaNs included), participating NaNs
  int pad[6];
};
static_assert(sizeof(PctScratch) == MI355_PERCENTILE_SCRATCH_BYTES, "MI355_PERCENTILE_SCRATCH_BYTES is the size of PctScratch");

struct ZsScratch {                          // per channel
  double sum[IN_WG], sumsq[IN_WG];          // per-workgroup sums of (x - pivot) and (x - pivot)^2 over the selected voxels
  int count[IN_WG];
  double mean, std;                         // written by the finaliser, read by the apply pass
  int n, pad[3];
};
static_assert(sizeof(ZsScratch) == MI355_ZSCORE_SELECT_SCRATCH_BYTES, "MI355_ZSCORE_SELECT_SCRATCH_BYTES is the size of ZsScratch");

// four consecutive voxels of a channel: one 16-byte load where the address allows; `valid` = how many lie below `stop`
__device__ __forceinline__ int in_load4(const float* x, long long i, long long stop, float v[4]) {
  if (i + 4 <= stop && (uintptr_t)(x + i) % 16 == 0) {
    const float4 f = *reinterpret_cast<const float4*>(x + i);
    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    return 4;
  }
  int valid = 0;
  for (int k = 0; k < 4; ++k) {
    v[k] = 0.f;
    if (i + k < stop) { v[k] = x[i + k]; valid = k + 1; }
  }
  return valid;
}

// ---- a. percentiles -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pct_key(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float pct_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// the value a named lane holds, the lane index being the same in all lanes: v_readlane_b32, no LDS traffic
#ifdef MI355_EMU
#define LANE_VALUE(v, lane) __shfl((v), (lane))
#else
#define LANE_VALUE(v, lane) __builtin_amdgcn_readlane((v), (lane))
#endif

// lh[slot] += 1 for every lane with `todo`; the whole wave calls this together (see THE DOMINANT BIN at the top)
__device__ __forceinline__ void pct_add(int* lh, bool todo, int slot, int lane) {
  for (int r = 0; r < PCT_PEEL; ++r) {
    const LaneMask pending = LANE_MASK(todo);
    if (pending == 0ull) return;                              // (the whole wave)
    const int first = __builtin_ctzll(pending);
    const int common = LANE_VALUE(slot, first);
    const bool same = todo && slot == common;
    const LaneMask m = LANE_MASK(same);
    if (lane == first) atomicAdd(&lh[common], (int)__builtin_popcountll(m));
    todo = todo && !same;
  }
  if (todo) atomicAdd(&lh[slot], 1);
}

// PASS 0: the top byte of every participating voxel into hist[0][0], and the NaN count. PASS 1..3: bits [high - 8, high) of the voxels
// whose bits above `high` equal the prefix of a leader rank into that rank's hist[PASS][rank].
template <int PASS>
__global__ void __launch_bounds__(256) pct_hist_kernel(const float* x, const float* above, long long V, long long per, int ranks,
                                                       PctScratch* scratch) {
  __shared__ int lh[(PASS == 0 ? 1 : PCT_RANKS) * 256];
  __shared__ int wnan[4];
  constexpr int SLOTS = PASS == 0 ? 1 : PCT_RANKS;
  PctScratch* S = scratch + blockIdx.y;
  for (int k = 0; k < SLOTS; ++k) lh[k * 256 + threadIdx.x] = 0;
  const int lane = threadIdx.x & 63;
  constexpr int high = 32 - 8 * PASS;
  unsigned prefix[PCT_RANKS];
  bool leads[PCT_RANKS];
  for (int r = 0; r < PCT_RANKS; ++r) {
    prefix[r] = 0u; leads[r] = false;
    if (PASS > 0 && r < ranks) { prefix[r] = S->prefix[r]; leads[r] = S->leader[r] == r; }
  }
  const bool has_nan = PASS > 0 && S->nan != 0;                // the answer is NaN already: nothing to select (uniform)
  __syncthreads();
  const long long start = (long long)blockIdx.x * per, stop = start + per < V ? start + per : V;
  const float* xc = x + (size_t)blockIdx.y * V;
  const bool masked = above != nullptr;
  const float thr = masked ? above[blockIdx.y] : 0.f;
  int nans = 0;
  for (long long i0 = start; i0 < stop && !has_nan; i0 += 1024) {          // (the bounds are the workgroup's: every wave makes every trip)
    float v[4];
    const int valid = in_load4(xc, i0 + 4 * (long long)threadIdx.x, stop, v);
    for (int k = 0; k < 4; ++k) {
      bool todo = k < valid && (!masked || v[k] > thr);       // (a NaN voxel or a NaN threshold compares false)
      const unsigned key = pct_key(v[k]);
      int slot = 0;
      if (PASS == 0) {
        nans += todo && v[k] != v[k];
        slot = (int)(key >> 24);
      } else {
        bool hit = false;
        for (int r = 0; r < PCT_RANKS; ++r)
          if (leads[r] && (key >> (high % 32)) == prefix[r]) { hit = true; slot = r * 256 + (int)((key >> (high - 8)) & 255u); }
        todo = todo && hit;
      }
      pct_add(lh, todo, slot, lane);
    }
  }
  if (PASS == 0) {
    nans = wave_sum(nans);
    if (lane == 0) wnan[threadIdx.x >> 6] = nans;
  }
  __syncthreads();
  for (int k = 0; k < SLOTS; ++k)
    if (lh[k * 256 + threadIdx.x] != 0) atomicAdd(&S->hist[PASS][k][threadIdx.x], lh[k * 256 + threadIdx.x]);
  if (PASS == 0 && threadIdx.x == 0) {
    const int t = wnan[0] + wnan[1] + wnan[2] + wnan[3];
    if (t != 0) atomicAdd(&S->nan, t);
  }
}

struct PctQ { double q[MI355_PERCENTILE_MAX_Q]; };

// thread r < ranks owns rank r = 2 * (index of q) + (0: lower, 1: upper) of numpy's linear rule (linear_rank)
__global__ void pct_pick_kernel(int pass, PctQ qs, int ranks, PctScratch* scratch) {
  __shared__ unsigned chosen[PCT_RANKS];
  PctScratch* S = scratch + blockIdx.x;
  const int r = threadIdx.x;
  const bool mine = r < ranks;
  int n = 0;
  if (pass == 0) {
    if (r == 0) {
      for (int b = 0; b < 256; ++b) n += S->hist[0][0][b];
      S->n = n;
    }
    __syncthreads();
    n = S->n;
  } else {
    n = S->n;
  }
  const bool live = mine && n > 0 && S->nan == 0;
  unsigned next = 0u;
  if (live) {
    int k;
    unsigned prefix = 0u;
    int owner = 0;
    if (pass == 0) {
      k = linear_rank(qs.q[r >> 1], n, (r & 1) != 0);
    } else {
      k = S->rank[r];
      prefix = S->prefix[r];
      owner = S->leader[r];
    }
    int below;
    next = (prefix << 8) | (unsigned)radix_pick(S->hist[pass][owner], k, below);
    S->rank[r] = k - below;
  }
  if (threadIdx.x < PCT_RANKS) chosen[threadIdx.x] = next;
  __syncthreads();                                           // every histogram of this pass has been read; the prefixes are all chosen
  if (live) {
    int first = r;
    for (int j = r - 1; j >= 0; --j)
      if (chosen[j] == next) first = j;
    S->prefix[r] = next;
    S->leader[r] = first;
  }
}

__global__ void pct_final_kernel(PctQ qs, int nq, const PctScratch* scratch, float* out, float* ranks_out, int* n_out) {
  const PctScratch* S = scratch + blockIdx.x;
  const int j = threadIdx.x;
  const int n = S->n;
  if (j == 0) n_out[blockIdx.x] = n;
  if (j >= nq) return;
  float lo = __uint_as_float(0x7fc00000u), hi = lo, val = lo;
  if (n > 0 && S->nan == 0) {
    lo = pct_value(S->prefix[2 * j]); hi = pct_value(S->prefix[2 * j + 1]);
    const double p = linear_position(qs.q[j], n);
    val = (float)linear_blend((double)lo, (double)hi, p - floor(p));
  }
  out[(size_t)blockIdx.x * nq + j] = val;
  if (ranks_out) {
    ranks_out[((size_t)blockIdx.x * nq + j) * 2] = lo;
    ranks_out[((size_t)blockIdx.x * nq + j) * 2 + 1] = hi;
  }
}

extern "C" int mi355_percentiles(const float* x, int32_t c, int64_t voxels, const double* q, int32_t nq, const float* above, float* out,
                                 float* ranks, int32_t* n, void* scratch, void* stream) {
  if (!x || !q || !out || !n || !scratch || (uintptr_t)scratch % 8 != 0) return MI355_EINVAL;
  int rc = vol_check_dims(c, voxels); if (rc) return rc;
  if (nq < 1 || nq > MI355_PERCENTILE_MAX_Q) return MI355_EINVAL;
  PctQ qs;
  for (int i = 0; i < MI355_PERCENTILE_MAX_Q; ++i) {
    qs.q[i] = i < nq ? q[i] : 0.0;
    if (!(qs.q[i] >= 0.0 && qs.q[i] <= 100.0)) return MI355_EINVAL;
  }
  const long long V = voxels;
  int nb;
  const long long per = vol_slice(V, 1024, IN_WG, &nb);
  const int nr = 2 * nq;
  PctScratch* S = (PctScratch*)scratch;
  const long long words = (long long)c * (long long)(sizeof(PctScratch) / 4);
  LAUNCH(zero_words_kernel, dim3(vol_blocks(words, 256)), dim3(256), 0, stream, (int*)scratch, words);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_hist_kernel<0>, dim3(nb, c), dim3(256), 0, stream, x, above, V, per, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_pick_kernel, dim3(c), dim3(64), 0, stream, 0, qs, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_hist_kernel<1>, dim3(nb, c), dim3(256), 0, stream, x, above, V, per, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_pick_kernel, dim3(c), dim3(64), 0, stream, 1, qs, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_hist_kernel<2>, dim3(nb, c), dim3(256), 0, stream, x, above, V, per, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_pick_kernel, dim3(c), dim3(64), 0, stream, 2, qs, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_hist_kernel<3>, dim3(nb, c), dim3(256), 0, stream, x, above, V, per, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_pick_kernel, dim3(c), dim3(64), 0, stream, 3, qs, nr, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(pct_final_kernel, dim3(c), dim3(64), 0, stream, qs, (int)nq, (const PctScratch*)S, out, ranks, (int*)n);
  return LAUNCH_CHECK();
}

// ---- b. windows -----------------------------------------------------------------------------------------------------------------------
template <int MODE> __device__ __forceinline__ float win_one(float x, float lo, float hi, float floor_v, float ceiling) {
  if (MODE == MI355_WINDOW_CLAMP) {                           // torch.clamp: a NaN voxel or bound gives NaN; lo > hi gives hi
    if (x != x) return x;
    if (lo != lo) return lo;
    if (hi != hi) return hi;
    const float t = x < lo ? lo : x;
    return t > hi ? hi : t;
  }
  if (MODE == MI355_WINDOW_RESCALE) {                         // window_data: a NaN t fails both comparisons and stays
    float t = (x - lo) / (hi - lo);
    t = t < floor_v ? floor_v : t;
    return t > ceiling ? ceiling : t;
  }
  return x <= lo ? floor_v : x - lo;                          // SHIFT_FLOOR
}

template <int MODE>
__global__ void __launch_bounds__(256) win_kernel(const float* x, int x_channels, float* y, long long V, const float* lo, const float* hi,
                                                  float floor_v, float ceiling) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= V) return;
  const float* xc = x + (x_channels == 1 ? (size_t)0 : (size_t)blockIdx.y * V);
  float* yc = y + (size_t)blockIdx.y * V;
  const float l = lo[blockIdx.y], h = MODE == MI355_WINDOW_SHIFT_FLOOR ? 0.f : hi[blockIdx.y];
  float v[4];
  const int valid = in_load4(xc, i, V, v);
  for (int k = 0; k < 4; ++k) v[k] = win_one<MODE>(v[k], l, h, floor_v, ceiling);
  if (valid == 4 && (uintptr_t)(yc + i) % 16 == 0) {
    *reinterpret_cast<float4*>(yc + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < valid; ++k) yc[i + k] = v[k];
  }
}

extern "C" int mi355_window(const float* x, int32_t x_channels, float* y, int32_t c, int64_t voxels, const float* lo, const float* hi,
                            int32_t mode, float floor_v, float ceiling, void* stream) {
  if (!x || !y || !lo) return MI355_EINVAL;
  int rc = vol_check_dims(c, voxels); if (rc) return rc;
  if (x_channels != c && x_channels != 1) return MI355_EINVAL;
  if (mode != MI355_WINDOW_CLAMP && mode != MI355_WINDOW_RESCALE && mode != MI355_WINDOW_SHIFT_FLOOR) return MI355_EINVAL;
  if (mode != MI355_WINDOW_SHIFT_FLOOR && !hi) return MI355_EINVAL;
  const long long V = voxels;
  const dim3 grid(vol_blocks(V, 1024), c);
  if (mode == MI355_WINDOW_CLAMP) LAUNCH(win_kernel<MI355_WINDOW_CLAMP>, grid, dim3(256), 0, stream, x, (int)x_channels, y, V, lo, hi, floor_v, ceiling);
  else if (mode == MI355_WINDOW_RESCALE) LAUNCH(win_kernel<MI355_WINDOW_RESCALE>, grid, dim3(256), 0, stream, x, (int)x_channels, y, V, lo, hi, floor_v, ceiling);
  else LAUNCH(win_kernel<MI355_WINDOW_SHIFT_FLOOR>, grid, dim3(256), 0, stream, x, (int)x_channels, y, V, lo, hi, floor_v, ceiling);
  return LAUNCH_CHECK();
}

// ---- c. z-score over a selected set ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool zs_selected(float x, int select, float threshold) {
  if (select == MI355_SELECT_NONZERO) return x != 0.f;
  if (select == MI355_SELECT_ABS_ABOVE) return fabsf(x) > threshold;
  return true;
}
__device__ __forceinline__ double zs_pivot(const float* xc) {
  const float p = xc[0];
  return (p - p == 0.f) ? (double)p : 0.0;                   // the channel's first voxel if it is finite
}

__global__ void __launch_bounds__(256) zs_partial_kernel(const float* x, long long V, long long per, int select, float threshold,
                                                         ZsScratch* scratch) {
  __shared__ double ws[2][4];
  __shared__ int wn[4];
  ZsScratch* S = scratch + blockIdx.y;
  const float* xc = x + (size_t)blockIdx.y * V;
  const double pivot = zs_pivot(xc);
  const long long start = (long long)blockIdx.x * per, stop = start + per < V ? start + per : V;
  double s = 0.0, ss = 0.0;
  int n = 0;
  for (long long i0 = start; i0 < stop; i0 += 1024) {
    float v[4];
    const int valid = in_load4(xc, i0 + 4 * (long long)threadIdx.x, stop, v);
    for (int k = 0; k < valid; ++k) {
      if (zs_selected(v[k], select, threshold)) {
        const double d = (double)v[k] - pivot;
        s += d; ss += d * d; ++n;
      }
    }
  }
  s = wave_sum(s); ss = wave_sum(ss); n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = s; ws[1][threadIdx.x >> 6] = ss; wn[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    S->sum[blockIdx.x] = ((ws[0][0] + ws[0][1]) + ws[0][2]) + ws[0][3];
    S->sumsq[blockIdx.x] = ((ws[1][0] + ws[1][1]) + ws[1][2]) + ws[1][3];
    S->count[blockIdx.x] = wn[0] + wn[1] + wn[2] + wn[3];
  }
}

__global__ void zs_final_kernel(const float* x, long long V, int nb, int center, int ddof, int zero_std_to_one, ZsScratch* scratch, int* n_out) {
#pragma clang fp contract(off)                              // ss - s * m of a single value is exactly 0 only if the product is rounded as ss was
  if (threadIdx.x != 0) return;
  ZsScratch* S = scratch + blockIdx.x;
  double s = 0.0, ss = 0.0;
  long long n = 0;
  for (int i = 0; i < nb; ++i) { s += S->sum[i]; ss += S->sumsq[i]; n += S->count[i]; }      // index order
  const double pivot = zs_pivot(x + (size_t)blockIdx.x * V);
  const double dn = (double)n, m = s / dn;                   // mean of x - pivot (n == 0: NaN, and nothing is selected to use it)
  const double dof = dn - (double)ddof;                      // sum (d - m)^2 = ss - s^2 / n; no degree of freedom left: NaN, as torch
  double var = dof > 0.0 ? (ss - s * m) / dof : (double)__uint_as_float(0x7fc00000u);
  if (var < 0.0) var = 0.0;                                  // (rounding of an all-equal set; NaN stays NaN)
  double sd = sqrt(var);
  if (zero_std_to_one && sd == 0.0) sd = 1.0;
  S->mean = center ? m + pivot : 0.0;
  S->std = sd;
  S->n = (int)n;
  n_out[blockIdx.x] = (int)n;
}

__global__ void __launch_bounds__(256) zs_apply_kernel(const float* x, float* y, long long V, int select, float threshold,
                                                       const ZsScratch* scratch) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= V) return;
  const ZsScratch* S = scratch + blockIdx.y;
  const float* xc = x + (size_t)blockIdx.y * V;
  float* yc = y + (size_t)blockIdx.y * V;
  const double mean = S->mean, sd = S->std;
  float v[4];
  const int valid = in_load4(xc, i, V, v);
  for (int k = 0; k < 4; ++k)
    if (zs_selected(v[k], select, threshold)) v[k] = (float)(((double)v[k] - mean) / sd);      // unselected: the bits as they were
  if (valid == 4 && (uintptr_t)(yc + i) % 16 == 0) {
    *reinterpret_cast<float4*>(yc + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < valid; ++k) yc[i + k] = v[k];
  }
}

extern "C" int mi355_zscore_select(const float* x, float* y, int32_t c, int64_t voxels, int32_t select, float threshold, int32_t center,
                                   int32_t ddof, int32_t zero_std_to_one, int32_t* n, void* scratch, void* stream) {
  if (!x || !y || !n || !scratch || (uintptr_t)scratch % 8 != 0) return MI355_EINVAL;
  int rc = vol_check_dims(c, voxels); if (rc) return rc;
  if (select != MI355_SELECT_ALL && select != MI355_SELECT_NONZERO && select != MI355_SELECT_ABS_ABOVE) return MI355_EINVAL;
  if (ddof != 0 && ddof != 1) return MI355_EINVAL;
  if (select == MI355_SELECT_ABS_ABOVE && threshold != threshold) return MI355_EINVAL;
  const long long V = voxels;
  int nb;
  const long long per = vol_slice(V, 1024, IN_WG, &nb);
  ZsScratch* S = (ZsScratch*)scratch;
  LAUNCH(zs_partial_kernel, dim3(nb, c), dim3(256), 0, stream, x, V, per, (int)select, threshold, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(zs_final_kernel, dim3(c), dim3(64), 0, stream, x, V, nb, (int)(center != 0), (int)ddof, (int)(zero_std_to_one != 0), S, (int*)n);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(zs_apply_kernel, dim3(vol_blocks(V, 1024), c), dim3(256), 0, stream, x, y, V, (int)select, threshold, (const ZsScratch*)S);
  return LAUNCH_CHECK();
}

// ---- d. any channel above its threshold ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) thr_any_kernel(const float* x, int c, long long V, const float* thr, unsigned char* out) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= V) return;
  bool any[4] = {false, false, false, false};
  int valid = 0;
  for (int ch = 0; ch < c; ++ch) {
    float v[4];
    valid = in_load4(x + (size_t)ch * V, i, V, v);
    const float t = thr[ch];
    for (int k = 0; k < 4; ++k) any[k] = any[k] || v[k] > t;
  }
  if (valid == 4 && (uintptr_t)(out + i) % 4 == 0) {
    *reinterpret_cast<unsigned*>(out + i) = (unsigned)any[0] | ((unsigned)any[1] << 8) | ((unsigned)any[2] << 16) | ((unsigned)any[3] << 24);
  } else {
    for (int k = 0; k < valid; ++k) out[i + k] = any[k] ? 1 : 0;
  }
}

extern "C" int mi355_threshold_any(const float* x, int32_t c, int64_t voxels, const float* thr, uint8_t* out, void* stream) {
  if (!x || !thr || !out) return MI355_EINVAL;
  int rc = vol_check_dims(c, voxels); if (rc) return rc;
  LAUNCH(thr_any_kernel, dim3(vol_blocks(voxels, 1024)), dim3(256), 0, stream, x, (int)c, (long long)voxels, thr, (unsigned char*)out);
  return LAUNCH_CHECK();
}
