// Scoring a mask against the ground truth, on the device: overlap counts, mask edges, the exact Euclidean distance transform and the
// surface-distance statistics (Hausdorff, percentile Hausdorff, average surface distance) that BraTS and SPPIN are ranked by.
//
// The rules at the top of volume_common.h hold. The loops are bounded by a line length, a chunk, 256 bins or the fixed number of partials;
// the integer atomics are adds on counters and histogram bins and max on the bit pattern of a non-negative float; the sums of distances
// are per-workgroup doubles that one thread adds in index order.
// Every op makes a fixed number of launches, whatever the data: seg_counts 2, mask_edges 1, edt 3, surface_stats 10.
//
//   seg_counts_kernel   4096 voxels per workgroup, 16 bytes per thread; three per-thread counts (pred, truth, both) reduced through the
//                       wave and the LDS, then one atomicAdd per workgroup and counter (TP, FP, FN, TN).
//   mask_edges_kernel   one thread per voxel: foreground with at least one of the six face neighbours background (outside = background).
//   edt_x_kernel        one wave per x-row, 64 voxels at a time: the ballot of the site bits gives every lane its nearest site at or
//                       below it (sweep up, the last site of earlier chunks carried along) and at or above it (sweep down).
//   edt_line_kernel     the y and the z pass: min_j(g[j] + (s * (i - j))^2) by BRUTE FORCE. One workgroup owns a bundle of 64 x-adjacent
//                       lines; EDT_CHUNK elements of the bundle are staged in the LDS (every lane reads its own column: no bank
//                       conflict, every global access a full 256-byte row), and every output voxel scans the staged chunk. A thread
//                       keeps 32 outputs in registers, so one LDS read feeds 32 candidates. Lines longer than a stage are streamed:
//                       for every chunk of outputs, every chunk of inputs. O(V * (H + D)) candidates -- 240 x 240 x 155: 8.9 M voxels x
//                       395 = 3.5 G, four vector instructions each -- branch-free, exact, no lower-envelope stack whose depth
//                       depends on the data, and the emulator runs it unchanged.
//                       +inf marks "no site in this line so far": inf + finite = inf and min() drops it; inf - inf is never formed.
//   surf_*              see mi355_surface_stats below.
//
// Exactness of the EDT: with spacing (1, 1, 1) every term is an integer; all of them are exact in fp32 while
// (D-1)^2 + (H-1)^2 + (W-1)^2 < 2^24, and the minimum of exact candidates is exact. Other spacings: each of the three terms carries at
// most two roundings and each sum one: relative error < 5 * 2^-24.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#define VOL_ZERO_WORDS                      // this source launches zero_words_kernel
#include "volume_common.h"

#define CNT_PER_WG 4096                     // voxels per workgroup of seg_counts_kernel
#define EDT_CHUNK 128                       // line elements per LDS stage of edt_line_kernel (x 64 columns x 4 bytes = 32 KiB)
#define EDT_SEGS 4                          // 256 threads = 64 columns x 4 segments of the output chunk
#define EDT_PER (EDT_CHUNK / EDT_SEGS)      // outputs a thread keeps in registers
#define SURF_WG 1024                        // most workgroups per channel of the surf_* streaming kernels = slots of partial sums
#define SURF_PASSES 4                       // radix select: 4 passes of 8 bits over the fp32 bit pattern

// per channel; [2] = direction (0: edges of A measured in the field of B, 1: the reverse), [2][2] = (direction, lower / upper rank)
struct SurfScratch {
  double sums[2][SURF_WG];                  // per-workgroup sums of sqrt(dist2), written by their owners only
  int hist[SURF_PASSES][2][2][256];         // a histogram per pass: nothing is zeroed between launches
  unsigned long long maxbits[2];            // max of the dist2 bit patterns (non-negative floats: bit order = value order)
  int n[2];                                 // edge voxels per direction
  unsigned prefix[2][2];                    // the bits of the order statistic selected so far
  int rank[2][2];                           // its rank among the values that share the prefix
  int pad[2];
};
static_assert(sizeof(SurfScratch) == MI355_SURFACE_SCRATCH_BYTES, "MI355_SURFACE_SCRATCH_BYTES is the size of SurfScratch");

// ---- a. overlap counts --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void count_word(unsigned a, unsigned b, int& np, int& nt, int& tp) {
  for (int k = 0; k < 4; ++k) {
    const int p = ((a >> (8 * k)) & 255u) != 0u, t = ((b >> (8 * k)) & 255u) != 0u;
    np += p; nt += t; tp += p & t;
  }
}

__global__ void __launch_bounds__(256) seg_counts_kernel(const unsigned char* pred, const unsigned char* truth, long long V, int* counts) {
  __shared__ int part[3][4];
  const unsigned char* p = pred + (size_t)blockIdx.y * V;
  const unsigned char* t = truth + (size_t)blockIdx.y * V;
  const long long block0 = (long long)blockIdx.x * CNT_PER_WG, start = block0 + (long long)threadIdx.x * 16;
  int np = 0, nt = 0, tp = 0;
  if (start + 16 <= V && (uintptr_t)(p + start) % 16 == 0 && (uintptr_t)(t + start) % 16 == 0) {
    const uint4 a = *reinterpret_cast<const uint4*>(p + start), b = *reinterpret_cast<const uint4*>(t + start);
    count_word(a.x, b.x, np, nt, tp); count_word(a.y, b.y, np, nt, tp); count_word(a.z, b.z, np, nt, tp); count_word(a.w, b.w, np, nt, tp);
  } else {
    for (int k = 0; k < 16; ++k) {
      if (start + k < V) { const int pp = p[start + k] != 0, tt = t[start + k] != 0; np += pp; nt += tt; tp += pp & tt; }
    }
  }
  for (int o = 32; o > 0; o >>= 1) { np += __shfl_xor(np, o); nt += __shfl_xor(nt, o); tp += __shfl_xor(tp, o); }
  if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = np; part[1][threadIdx.x >> 6] = nt; part[2][threadIdx.x >> 6] = tp; }
  __syncthreads();
  if (threadIdx.x == 0) {
    np = part[0][0] + part[0][1] + part[0][2] + part[0][3];
    nt = part[1][0] + part[1][1] + part[1][2] + part[1][3];
    tp = part[2][0] + part[2][1] + part[2][2] + part[2][3];
    const long long left = V - block0;
    const int here = (int)(left < CNT_PER_WG ? left : CNT_PER_WG);
    int* out = counts + 4 * blockIdx.y;
    atomicAdd(out + 0, tp);
    atomicAdd(out + 1, np - tp);
    atomicAdd(out + 2, nt - tp);
    atomicAdd(out + 3, here - np - nt + tp);
  }
}

extern "C" int mi355_seg_counts(const uint8_t* pred, const uint8_t* truth, int32_t c, int32_t d, int32_t h, int32_t w, int32_t* counts,
                                void* stream) {
  if (!pred || !truth || !counts) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  const long long V = (long long)d * h * w;
  LAUNCH(zero_words_kernel, dim3(vol_blocks(4ll * c, 256)), dim3(256), 0, stream, (int*)counts, 4ll * c);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(seg_counts_kernel, dim3(vol_blocks(V, CNT_PER_WG), c), dim3(256), 0, stream, (const unsigned char*)pred, (const unsigned char*)truth,
         V, (int*)counts);
  return LAUNCH_CHECK();
}

// ---- b. edges ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) mask_edges_kernel(const unsigned char* mask, int D, int H, int W, unsigned char* edges) {
  const long long V = (long long)D * H * W;
  const long long vv = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vv >= V) return;
  const unsigned char* m = mask + (size_t)blockIdx.y * V;
  const int v = (int)vv, hw = H * W;
  const int x = v % W, y = (v / W) % H, z = v / hw;
  bool edge = false;
  if (m[v] != 0) {
    const bool inside = x > 0 && x + 1 < W && y > 0 && y + 1 < H && z > 0 && z + 1 < D;
    // (short-circuit: a neighbour is read only when it lies in the volume)
    edge = !(inside && m[v - 1] != 0 && m[v + 1] != 0 && m[v - W] != 0 && m[v + W] != 0 && m[v - hw] != 0 && m[v + hw] != 0);
  }
  edges[(size_t)blockIdx.y * V + v] = edge ? 1 : 0;
}

extern "C" int mi355_mask_edges(const uint8_t* mask, int32_t c, int32_t d, int32_t h, int32_t w, uint8_t* edges, void* stream) {
  if (!mask || !edges) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  LAUNCH(mask_edges_kernel, dim3(vol_blocks((long long)d * h * w, 256), c), dim3(256), 0, stream, (const unsigned char*)mask, (int)d, (int)h,
         (int)w, (unsigned char*)edges);
  return LAUNCH_CHECK();
}

// ---- c. exact squared Euclidean distance transform ---------------------------------------------------------------------------------------
// out[x] = (sx * |x - nearest site of the row|)^2, +inf for a row without sites. The same lane writes out[x] in the sweep up and reads it
// back in the sweep down (x = chunk * 64 + lane in both).
__global__ void __launch_bounds__(256) edt_x_kernel(const unsigned char* sites, int invert, long long rows, int W, float sx, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= rows) return;                                  // the whole wave
  const size_t base = ((size_t)blockIdx.y * rows + row) * W;
  const int chunks = (W + 63) / 64;
  const bool want = invert == 0;
  int last = -1;                                            // the last site of the chunks below (wave-uniform)
  for (int ch = 0; ch < chunks; ++ch) {
    const int x = ch * 64 + lane;
    const bool site = x < W && (sites[base + x] != 0) == want;
    const unsigned long long bits = LANE_MASK(site);
    const unsigned long long at_or_below = bits & (lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1ull));
    const int near = at_or_below ? ch * 64 + 63 - __builtin_clzll(at_or_below) : last;
    if (x < W) out[base + x] = near >= 0 ? (float)(x - near) : INFINITY;
    if (bits) last = ch * 64 + 63 - __builtin_clzll(bits);
  }
  int next = -1;                                            // the first site of the chunks above
  for (int ch = chunks - 1; ch >= 0; --ch) {
    const int x = ch * 64 + lane;
    const bool site = x < W && (sites[base + x] != 0) == want;
    const unsigned long long bits = LANE_MASK(site);
    const unsigned long long at_or_above = bits & (~0ull << lane);
    const int near = at_or_above ? ch * 64 + __builtin_ctzll(at_or_above) : next;
    if (x < W) {
      const float below = out[base + x], above = near >= 0 ? (float)(near - x) : INFINITY;
      const float t = sx * fminf(below, above);
      out[base + x] = t * t;
    }
    if (bits) next = ch * 64 + __builtin_ctzll(bits);
  }
}

// out[i] = min_j(in[j] + (sp * (i - j))^2) along a line of L elements `step` apart; blockIdx.x = (line bundle of 64 columns, index along
// the other axis, `other` elements apart). Thread (lane, seg) owns outputs seg * EDT_PER .. + EDT_PER - 1 of every output chunk.
__global__ void __launch_bounds__(256) edt_line_kernel(const float* in, float* out, int L, long long step, long long other, int tiles_x, int W,
                                                       long long V, float sp) {
  __shared__ float stage[EDT_CHUNK][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int bx = blockIdx.x % tiles_x, o = blockIdx.x / tiles_x;
  const int x = bx * 64 + lane;
  const bool inb = x < W;
  const size_t base = (size_t)blockIdx.y * V + (size_t)o * other + x;
  const int chunks = (L + EDT_CHUNK - 1) / EDT_CHUNK;
  for (int oc = 0; oc < chunks; ++oc) {
    const int i0 = oc * EDT_CHUNK + seg * EDT_PER;
    float acc[EDT_PER];
#pragma unroll
    for (int k = 0; k < EDT_PER; ++k) acc[k] = INFINITY;
    for (int jc = 0; jc < chunks; ++jc) {
      const int j0 = jc * EDT_CHUNK;
      const int rows = L - j0 < EDT_CHUNK ? L - j0 : EDT_CHUNK;
      __syncthreads();                                      // the readers of the previous stage are done
      for (int r = seg; r < rows; r += EDT_SEGS) stage[r][lane] = inb ? in[base + (size_t)(j0 + r) * step] : INFINITY;
      __syncthreads();
      if (i0 < L) {                                         // (the whole wave: seg is the wave index)
        const float d0 = (float)(i0 - j0);
        for (int r = 0; r < rows; ++r) {
          const float g = stage[r][lane], d = d0 - (float)r;             // i0 - j: a small integer, exact
#pragma unroll
          for (int k = 0; k < EDT_PER; ++k) {
            const float t = sp * (d + (float)k);
            acc[k] = fminf(acc[k], t * t + g);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EDT_PER; ++k)
      if (inb && i0 + k < L) out[base + (size_t)(i0 + k) * step] = acc[k];
  }
}

static bool mt_bad_spacing(float s) { return !(s > 0.f) || !std::isfinite(s); }

extern "C" int mi355_edt(const uint8_t* sites, int32_t invert, int32_t c, int32_t d, int32_t h, int32_t w, float sz, float sy, float sx,
                         float* dist2, float* tmp, void* stream) {
  if (!sites || !dist2 || !tmp || dist2 == tmp) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  if (mt_bad_spacing(sz) || mt_bad_spacing(sy) || mt_bad_spacing(sx)) return MI355_EINVAL;
  const long long V = (long long)d * h * w, rows = (long long)d * h;
  const int tiles_x = ceil_div(w, 64);
  LAUNCH(edt_x_kernel, dim3(vol_blocks(rows, 4), c), dim3(256), 0, stream, (const unsigned char*)sites, (int)(invert != 0), rows, (int)w, sx, dist2);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(edt_line_kernel, dim3((unsigned)((long long)tiles_x * d), c), dim3(256), 0, stream, (const float*)dist2, tmp, (int)h, (long long)w,
         (long long)h * w, tiles_x, (int)w, V, sy);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(edt_line_kernel, dim3((unsigned)((long long)tiles_x * h), c), dim3(256), 0, stream, (const float*)tmp, dist2, (int)d, (long long)h * w,
         (long long)w, tiles_x, (int)w, V, sz);
  return LAUNCH_CHECK();
}

// ---- d. surface-distance statistics -----------------------------------------------------------------------------------------------------
// Per channel and direction, over the edge voxels of the source set: the maximum (atomicMax on the bits of dist2; sqrt is monotone, so
// the root of the largest dist2 is the largest distance), the sum of sqrtf(dist2) (per-workgroup partials in fixed order, see the top),
// and two order statistics of dist2 by radix select: pass p histograms bits 31-8p .. 24-8p of the values whose higher bits equal the
// prefix chosen so far (surf_stats_kernel is pass 0 for both ranks at once; surf_hist_kernel passes 1..3, a histogram per rank, since the
// two ranks may have parted), and surf_pick_kernel walks the 256 bins to the one that holds the rank. No compaction, no sort.
// A workgroup owns a contiguous slice of `per` voxels (a multiple of 256): thread t adds voxels t, t + 256, ... of the slice in order.
__global__ void __launch_bounds__(256) surf_stats_kernel(const unsigned char* edges_a, const unsigned char* edges_b, const float* d2_ab,
                                                         const float* d2_ba, long long V, long long per, SurfScratch* scratch) {
  __shared__ int lh[2][256];
  __shared__ double wsum[2][4];
  __shared__ int wn[2][4];
  __shared__ unsigned wmax[2][4];
  SurfScratch* S = scratch + blockIdx.y;
  lh[0][threadIdx.x] = 0; lh[1][threadIdx.x] = 0;
  __syncthreads();
  const long long start = (long long)blockIdx.x * per, stop = start + per < V ? start + per : V;
  const size_t cb = (size_t)blockIdx.y * V;
  double s[2] = {0.0, 0.0};
  int n[2] = {0, 0};
  unsigned mx[2] = {0u, 0u};
  for (long long i = start + threadIdx.x; i < stop; i += 256) {
    for (int dir = 0; dir < 2; ++dir) {
      if ((dir ? edges_b : edges_a)[cb + i] != 0) {
        const float d2 = (dir ? d2_ba : d2_ab)[cb + i];
        const unsigned b = __float_as_uint(d2);
        s[dir] += (double)sqrtf(d2);
        ++n[dir];
        mx[dir] = b > mx[dir] ? b : mx[dir];
        atomicAdd(&lh[dir][b >> 24], 1);
      }
    }
  }
  for (int dir = 0; dir < 2; ++dir) {
    const double ws = wave_sum(s[dir]);
    const int wc = wave_sum(n[dir]);
    const unsigned wm = wave_max(mx[dir]);
    if ((threadIdx.x & 63) == 0) { wsum[dir][threadIdx.x >> 6] = ws; wn[dir][threadIdx.x >> 6] = wc; wmax[dir][threadIdx.x >> 6] = wm; }
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int dir = threadIdx.x;
    double t = wsum[dir][0]; int c = wn[dir][0]; unsigned m = wmax[dir][0];
    for (int i = 1; i < 4; ++i) { t += wsum[dir][i]; c += wn[dir][i]; m = wmax[dir][i] > m ? wmax[dir][i] : m; }
    S->sums[dir][blockIdx.x] = t;
    if (c > 0) { atomicAdd(&S->n[dir], c); atomicMax(&S->maxbits[dir], (unsigned long long)m); }
  }
  for (int dir = 0; dir < 2; ++dir)
    if (lh[dir][threadIdx.x] != 0) atomicAdd(&S->hist[0][dir][0][threadIdx.x], lh[dir][threadIdx.x]);
}

__global__ void __launch_bounds__(256) surf_hist_kernel(const unsigned char* edges_a, const unsigned char* edges_b, const float* d2_ab,
                                                        const float* d2_ba, long long V, long long per, int pass, SurfScratch* scratch) {
  __shared__ int lh[2][2][256];
  SurfScratch* S = scratch + blockIdx.y;
  for (int k = 0; k < 4; ++k) lh[k >> 1][k & 1][threadIdx.x] = 0;
  __syncthreads();
  const long long start = (long long)blockIdx.x * per, stop = start + per < V ? start + per : V;
  const size_t cb = (size_t)blockIdx.y * V;
  const int high = 32 - 8 * pass, low = 24 - 8 * pass;      // pass 1..3: high = 24, 16, 8
  unsigned prefix[2][2];
  for (int k = 0; k < 4; ++k) prefix[k >> 1][k & 1] = S->prefix[k >> 1][k & 1];
  for (long long i = start + threadIdx.x; i < stop; i += 256) {
    for (int dir = 0; dir < 2; ++dir) {
      if ((dir ? edges_b : edges_a)[cb + i] != 0) {
        const unsigned b = __float_as_uint((dir ? d2_ba : d2_ab)[cb + i]);
        for (int r = 0; r < 2; ++r)
          if ((b >> high) == prefix[dir][r]) atomicAdd(&lh[dir][r][(b >> low) & 255u], 1);
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k)
    if (lh[k >> 1][k & 1][threadIdx.x] != 0) atomicAdd(&S->hist[pass][k >> 1][k & 1][threadIdx.x], lh[k >> 1][k & 1][threadIdx.x]);
}

// thread (dir, r) of a channel: rank r (0: lower, 1: upper; linear_rank) of direction dir, one byte further per pass
__global__ void surf_pick_kernel(int pass, double percentile, SurfScratch* scratch) {
  SurfScratch* S = scratch + blockIdx.x;
  if (threadIdx.x >= 4) return;
  const int dir = threadIdx.x >> 1, r = threadIdx.x & 1;
  const int n = S->n[dir];
  if (n == 0) return;
  int k;
  unsigned prefix = 0u;
  if (pass == 0) {
    k = linear_rank(percentile, n, r != 0);
  } else {
    k = S->rank[dir][r];
    prefix = S->prefix[dir][r];
  }
  int below;
  const int bin = radix_pick(S->hist[pass][dir][pass == 0 ? 0 : r], k, below);
  S->prefix[dir][r] = (prefix << 8) | (unsigned)bin;
  S->rank[dir][r] = k - below;
}

__global__ void surf_final_kernel(int nb, double percentile, const SurfScratch* scratch, float* out, int* n_out) {
  __shared__ double total[2];
  const SurfScratch* S = scratch + blockIdx.x;
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int i = 0; i < nb; ++i) t += S->sums[threadIdx.x][i];                  // index order
    total[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float* o = out + 8 * blockIdx.x;
  const int na = S->n[0], nbv = S->n[1];
  n_out[2 * blockIdx.x] = na; n_out[2 * blockIdx.x + 1] = nbv;
  if (na == 0 || nbv == 0) {
    const float v = (na == 0 && nbv == 0) ? 0.f : INFINITY;
    for (int i = 0; i < 8; ++i) o[i] = v;
    return;
  }
  float hd[2], pct[2];
  for (int dir = 0; dir < 2; ++dir) {
    const int n = dir ? nbv : na;
    hd[dir] = sqrtf(__uint_as_float((unsigned)S->maxbits[dir]));
    const double lo = (double)sqrtf(__uint_as_float(S->prefix[dir][0])), hi = (double)sqrtf(__uint_as_float(S->prefix[dir][1]));
    const double p = linear_position(percentile, n);
    pct[dir] = (float)linear_blend(lo, hi, p - floor(p));
  }
  o[0] = hd[0] > hd[1] ? hd[0] : hd[1];
  o[1] = pct[0] > pct[1] ? pct[0] : pct[1];
  o[2] = (float)((total[0] + total[1]) / ((double)na + (double)nbv));
  o[3] = hd[0]; o[4] = hd[1]; o[5] = pct[0]; o[6] = pct[1];
  o[7] = (float)(total[0] / (double)na);
}

extern "C" int mi355_surface_stats(const uint8_t* edges_a, const uint8_t* edges_b, const float* dist2_ab, const float* dist2_ba, int32_t c,
                                   int64_t voxels, double percentile, float* out, int32_t* n, void* scratch, void* stream) {
  if (!edges_a || !edges_b || !dist2_ab || !dist2_ba || !out || !n || !scratch || (uintptr_t)scratch % 8 != 0) return MI355_EINVAL;
  if (vol_check_dims(c, voxels) || !(percentile >= 0.0 && percentile <= 100.0)) return MI355_EINVAL;
  const long long V = voxels;
  int nb;                                                   // <= SURF_WG
  const long long per = vol_slice(V, 256, SURF_WG, &nb);
  SurfScratch* S = (SurfScratch*)scratch;
  const unsigned char *ea = (const unsigned char*)edges_a, *eb = (const unsigned char*)edges_b;
  const long long words = (long long)c * (long long)(sizeof(SurfScratch) / 4);
  LAUNCH(zero_words_kernel, dim3(vol_blocks(words, 256)), dim3(256), 0, stream, (int*)scratch, words);
  int rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(surf_stats_kernel, dim3(nb, c), dim3(256), 0, stream, ea, eb, dist2_ab, dist2_ba, V, per, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(surf_pick_kernel, dim3(c), dim3(64), 0, stream, 0, percentile, S);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  for (int pass = 1; pass < SURF_PASSES; ++pass) {
    LAUNCH(surf_hist_kernel, dim3(nb, c), dim3(256), 0, stream, ea, eb, dist2_ab, dist2_ba, V, per, pass, S);
    rc = LAUNCH_CHECK(); if (rc) return rc;
    LAUNCH(surf_pick_kernel, dim3(c), dim3(64), 0, stream, pass, percentile, S);
    rc = LAUNCH_CHECK(); if (rc) return rc;
  }
  LAUNCH(surf_final_kernel, dim3(c), dim3(64), 0, stream, nb, percentile, (const SurfScratch*)S, out, (int*)n);
  return LAUNCH_CHECK();
}
