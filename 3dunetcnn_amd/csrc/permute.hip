// Signed axis permutations of a volume batch on the device: the 48 rotations and reflections of the reference's unet3d/utils/augment.py
// (permute_data and its inverse) as ONE launch each way, and the inverse fused with the activation and the running mean of a
// permutation ensemble.
//
// The rules at the top of volume_common.h hold: every buffer is the caller's, everything is enqueued on `stream`, one launch whatever the
// data, no atomics at all -- one thread owns one output voxel, so a second call gives the same bits.
//
//   the code     one int per sample: s0 | s1 << 2 | s2 << 4 | f0 << 6 | f1 << 7 | f2 << 8. Output axis a (0 = D, 1 = H, 2 = W) reads source
//                axis s_a, backwards with f_a: out[v0, v1, v2] = in[u], u[s_a] = f_a ? out_extent[a] - 1 - v_a : v_a. The host checks the
//                codes and hands them to the kernel IN ITS ARGUMENTS (PermCodes): no device table, no copy, no wait. A workgroup decodes
//                its sample's code into a base offset and one signed source stride per OUTPUT axis (PermMap): the source offset of an
//                output voxel is base + v0 * step[0] + v1 * step[1] + v2 * step[2], in 64 bits.
//   two routes   chosen per workgroup from its sample's code.
//                ROWS (s2 == 2): a row of W stays a row, possibly reversed. A thread copies 16 bytes where the row length and both
//                pointers allow (a reversed row: the 16 bytes are loaded from the mirrored place and their elements reversed in registers),
//                one element elsewhere; neighbouring threads take neighbouring addresses either way.
//                TILE (W moves): source W becomes output axis b (0 or 1) and output W reads source axis s2. A workgroup owns a
//                PT x PT tile of the (b, W) plane of the OUTPUT at one coordinate of the remaining axis: it reads the tile with lanes
//                along source W, parks it in the LDS one element per dword, and writes it with lanes along output W. Both global
//                sides are coalesced; a flipped axis only reverses the order of the lanes' addresses.
//   the LDS pad  the tile is unsigned[PT][PT + 1]. It is written by rows (lane -> consecutive dwords: ds_write_b32, bank = dword % 32,
//                conflict-free) and read by columns (lane -> dword lane * (PT + 1) + const). ds_read_b32 is served in two 32-lane
//                halves over 32 banks: with the row padded by ONE access width (PT + 1 = 65 = 1 mod 32) the 32 lanes of a half hit 32
//                different banks; unpadded (64 = 0 mod 32) they would all hit one (32-way). Padding by 2, 4 or 8 would leave a 2-, 4- or
//                8-way conflict.
//   accumulate   mi355_unpermute_accumulate is the same walk with the INVERSE code (source = the permuted prediction, output = the
//                un-permuted fp32 accumulator) and an epilogue: acc = (init ? 0 : acc) + weight * p, p = the value, its sigmoid or the
//                softmax over the voxel's channels (the expressions of postprocess_kernel in prepost.hip). A thread walks the channels of
//                its voxels. Softmax on the TILE route: the maximum and the sum of a voxel are formed by the thread that loads it
//                (first walk over the channels, registers), then every channel is loaded again (the tile's logits are in the L2 by then),
//                normalised and transposed through the one LDS tile.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#include "volume_common.h"

#define PT MI355_PERMUTE_TILE
#define PT_ROWS (PT * PT / 256)            // tile elements per thread
#define PERM_MAX_C 16                       // softmax channels, as the loss family and postprocess
static_assert(PT == 64 && PT_ROWS == 16, "256 threads: 64 lanes along a tile row, 4 rows per step");

struct PermCodes { unsigned short code[MI355_PERMUTE_MAX_BATCH]; };

// ---- the code ----------------------------------------------------------------------------------------------------------------------------
static inline bool perm_code_ok(int code) {
  if (code < 0 || (code >> 9) != 0) return false;
  const int s0 = code & 3, s1 = (code >> 2) & 3, s2 = (code >> 4) & 3;
  return s0 < 3 && s1 < 3 && s2 < 3 && s0 != s1 && s0 != s2 && s1 != s2;
}
// out_extent[a] = E[s_a]
static inline void perm_out_extents(int code, const int E[3], int O[3]) {
  for (int a = 0; a < 3; ++a) O[a] = E[(code >> (2 * a)) & 3];
}
// the code of the inverse map: output axis k of the inverse reads the axis a with s_a == k, backwards exactly when a did
static inline int perm_inverse(int code) {
  int inv = 0;
  for (int a = 0; a < 3; ++a) {
    const int k = (code >> (2 * a)) & 3;
    inv |= a << (2 * k);
    inv |= ((code >> (6 + a)) & 1) << (6 + k);
  }
  return inv;
}
// workgroups a sample needs per (n, c) volume (permute) or per n (accumulate) on its route; vec = elements per 16-byte thread, or 1
static inline long long perm_units(int code, const int O[3], int vec) {
  if (((code >> 4) & 3) == 2) return ((long long)O[0] * O[1] * O[2] / vec + 255) / 256;
  const int b = (code & 3) == 2 ? 0 : 1;
  return (long long)((O[b] + PT - 1) / PT) * ((O[2] + PT - 1) / PT) * O[1 - b];
}

struct PermMap {
  int O[3];                                 // output extents
  long long step[3];                        // signed source stride of each output axis, in elements
  long long base;                           // source offset of output voxel (0, 0, 0)
  bool rows;                                // s2 == 2
  int b;                                    // TILE route: the output axis that runs along source W
};
__device__ __forceinline__ int pick3(int i, int a0, int a1, int a2) { return i == 0 ? a0 : (i == 1 ? a1 : a2); }
__device__ __forceinline__ PermMap perm_map(int code, int e0, int e1, int e2) {
  PermMap m;
  m.base = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int s = (code >> (2 * a)) & 3;
    m.O[a] = pick3(s, e0, e1, e2);
    const long long stride = s == 0 ? (long long)e1 * e2 : (s == 1 ? (long long)e2 : 1ll);
    const bool flip = ((code >> (6 + a)) & 1) != 0;
    m.step[a] = flip ? -stride : stride;
    if (flip) m.base += (long long)(m.O[a] - 1) * stride;
  }
  m.rows = ((code >> 4) & 3) == 2;
  m.b = (code & 3) == 2 ? 0 : 1;
  return m;
}

// the elements of 16 bytes in reverse order (elem = their size in bytes)
__device__ __forceinline__ unsigned perm_rev_word(unsigned x, int elem) {
  if (elem == 2) return (x >> 16) | (x << 16);
  if (elem == 1) return __builtin_bswap32(x);
  return x;
}
__device__ __forceinline__ uint4 perm_rev16(uint4 v, int elem) {
  return make_uint4(perm_rev_word(v.w, elem), perm_rev_word(v.z, elem), perm_rev_word(v.y, elem), perm_rev_word(v.x, elem));
}

// ---- a. the permutation -------------------------------------------------------------------------------------------------------------------
// grid (workgroups per volume on the longest route, c, n); T = an unsigned integer of the element's size
template <class T>
__global__ void __launch_bounds__(256) permute_kernel(const T* src, T* dst, int e0, int e1, int e2, PermCodes codes, int per_sample, int vec_ok) {
  __shared__ unsigned tile[PT][PT + 1];
  const PermMap m = perm_map(codes.code[per_sample ? blockIdx.z : 0], e0, e1, e2);
  const long long V = (long long)e0 * e1 * e2;
  const size_t vol = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * (size_t)V;
  const T* s = src + vol;
  T* d = dst + vol;
  if (m.rows) {
    constexpr int VEC = 16 / (int)sizeof(T);
    const int W = m.O[2];
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (vec_ok) {
      const int per_row = W / VEC;
      if (item >= V / VEC) return;
      const long long row = item / per_row;
      const int x0 = (int)(item - row * per_row) * VEC;
      const int v0 = (int)(row / m.O[1]), v1 = (int)(row - (long long)v0 * m.O[1]);
      const long long from = m.base + v0 * m.step[0] + v1 * m.step[1];
      const bool flip = m.step[2] < 0;                                        // (from + x * step[2], x = x0 + VEC - 1, is the lowest address)
      const long long lo = flip ? from - (long long)(x0 + VEC - 1) : from + x0;
      uint4 v = *reinterpret_cast<const uint4*>(s + lo);
      if (flip) v = perm_rev16(v, (int)sizeof(T));
      *reinterpret_cast<uint4*>(d + row * W + x0) = v;
    } else {
      if (item >= V) return;
      const long long row = item / W;
      const int x = (int)(item - row * W);
      const int v0 = (int)(row / m.O[1]), v1 = (int)(row - (long long)v0 * m.O[1]);
      d[item] = s[m.base + v0 * m.step[0] + v1 * m.step[1] + x * m.step[2]];
    }
    return;
  }
  const int b = m.b, r = 1 - b;
  const int Ob = pick3(b, m.O[0], m.O[1], 0), Or = pick3(r, m.O[0], m.O[1], 0), O2 = m.O[2];
  const long long step_b = b == 0 ? m.step[0] : m.step[1], step_r = r == 0 ? m.step[0] : m.step[1];
  const int tiles_b = (Ob + PT - 1) / PT, tiles_2 = (O2 + PT - 1) / PT;
  const long long unit = blockIdx.x;
  if (unit >= (long long)tiles_b * tiles_2 * Or) return;                      // (the whole workgroup: the grid is sized for the longest route)
  const int tb = (int)(unit % tiles_b), t2 = (int)((unit / tiles_b) % tiles_2), vr = (int)(unit / ((long long)tiles_b * tiles_2));
  const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
  {
    const int vb = tb * PT + tx;                                              // lanes along source W
    const long long from = m.base + vr * step_r + vb * step_b;
    for (int k = 0; k < PT_ROWS; ++k) {
      const int i2 = ty + 4 * k, v2 = t2 * PT + i2;
      if (vb < Ob && v2 < O2) tile[i2][tx] = (unsigned)s[from + v2 * m.step[2]];
    }
  }
  __syncthreads();
  {
    const int v2 = t2 * PT + tx;                                              // lanes along output W
    for (int k = 0; k < PT_ROWS; ++k) {
      const int jb = ty + 4 * k, vb = tb * PT + jb;
      if (vb < Ob && v2 < O2) {
        const long long row = b == 0 ? (long long)vb * m.O[1] + vr : (long long)vr * m.O[1] + vb;
        d[row * O2 + v2] = (T)tile[tx][jb];
      }
    }
  }
}

// n_codes codes checked and spread over n samples; EINVAL where the ABI says so. O = the output extents every sample shares.
static int perm_gather_codes(const int32_t* codes, int32_t n_codes, int32_t n, const int E[3], PermCodes& pc, int O[3]) {
  if (!codes || n < 1 || n > 65535 || (n_codes != 1 && n_codes != n) || n_codes > MI355_PERMUTE_MAX_BATCH) return MI355_EINVAL;
  for (int i = 0; i < MI355_PERMUTE_MAX_BATCH; ++i) pc.code[i] = 0;
  for (int i = 0; i < n_codes; ++i) {
    if (!perm_code_ok(codes[i])) return MI355_EINVAL;
    int Oi[3];
    perm_out_extents(codes[i], E, Oi);
    if (i == 0) { O[0] = Oi[0]; O[1] = Oi[1]; O[2] = Oi[2]; }
    else if (Oi[0] != O[0] || Oi[1] != O[1] || Oi[2] != O[2]) return MI355_EINVAL;
    pc.code[i] = (unsigned short)codes[i];
  }
  return MI355_OK;
}

extern "C" int mi355_permute3d(const void* src, void* dst, int32_t n, int32_t c, int32_t d, int32_t h, int32_t w, int32_t elem_bytes,
                               const int32_t* codes, int32_t n_codes, void* stream) {
  if (!src || !dst || src == dst) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) return MI355_EINVAL;
  const int E[3] = {d, h, w};
  int O[3];
  PermCodes pc;
  rc = perm_gather_codes(codes, n_codes, n, E, pc, O); if (rc) return rc;
  const int vec = 16 / elem_bytes;
  const int vec_ok = (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0 && O[2] % vec == 0;      // (ROWS: O[2] is the source's W too)
  long long units = 0;
  for (int i = 0; i < n_codes; ++i) {
    const long long u = perm_units(pc.code[i], O, vec_ok ? vec : 1);
    units = u > units ? u : units;
  }
  const dim3 grid((unsigned)units, c, n);
  const int per_sample = n_codes > 1;
  if (elem_bytes == 1) LAUNCH(permute_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)src, (uint8_t*)dst, (int)d, (int)h, (int)w, pc, per_sample, vec_ok);
  else if (elem_bytes == 2) LAUNCH(permute_kernel<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t*)src, (uint16_t*)dst, (int)d, (int)h, (int)w, pc, per_sample, vec_ok);
  else LAUNCH(permute_kernel<uint32_t>, grid, dim3(256), 0, stream, (const uint32_t*)src, (uint32_t*)dst, (int)d, (int)h, (int)w, pc, per_sample, vec_ok);
  return LAUNCH_CHECK();
}

// ---- b. the inverse, the activation and the running mean in one pass ------------------------------------------------------------------------
__device__ __forceinline__ float perm_value(const void* src, int src_elem, size_t i) {
  if (src_elem == MI355_ACT_F32) return reinterpret_cast<const float*>(src)[i];
  const unsigned h = reinterpret_cast<const unsigned short*>(src)[i];
  return src_elem == MI355_ACT_BF16 ? bf16lo_to_f32(h) : f16lo_to_f32(h);
}
// four consecutive values from element i (aligned to four elements), in reverse order with `flip`
__device__ __forceinline__ void perm_value4(const void* src, int src_elem, size_t i, bool flip, float v[4]) {
  float t[4];
  if (src_elem == MI355_ACT_F32) {
    const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(src) + i);
    t[0] = f.x; t[1] = f.y; t[2] = f.z; t[3] = f.w;
  } else {
    const uint2 p = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(src) + i);
    if (src_elem == MI355_ACT_BF16) { t[0] = bf16lo_to_f32(p.x); t[1] = bf16hi_to_f32(p.x); t[2] = bf16lo_to_f32(p.y); t[3] = bf16hi_to_f32(p.y); }
    else { t[0] = f16lo_to_f32(p.x); t[1] = f16hi_to_f32(p.x); t[2] = f16lo_to_f32(p.y); t[3] = f16hi_to_f32(p.y); }
  }
  for (int k = 0; k < 4; ++k) v[k] = flip ? t[3 - k] : t[k];
}
__device__ __forceinline__ float perm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
// acc = (init ? 0 : acc) + weight * p: one product, or one fused multiply-add (a single rounding)
__device__ __forceinline__ float perm_fold(float old, float p, float weight, int init) { return init ? weight * p : fmaf(weight, p, old); }

// acc[0 .. VEC) = (init ? 0 : acc) + weight * p; init never reads acc
template <int VEC> __device__ __forceinline__ void unperm_store(float* a, const float p[VEC], float weight, int init) {
  if (VEC == 4) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!init) o = *reinterpret_cast<const float4*>(a);
    *reinterpret_cast<float4*>(a) = make_float4(perm_fold(o.x, p[0], weight, init), perm_fold(o.y, p[1], weight, init),
                                                perm_fold(o.z, p[2], weight, init), perm_fold(o.w, p[3], weight, init));
  } else {
    a[0] = perm_fold(init ? 0.f : a[0], p[0], weight, init);
  }
}
template <int VEC> __device__ __forceinline__ void unperm_load(const void* src, int src_elem, size_t at, bool flip, float v[VEC]) {
  if (VEC == 4) perm_value4(src, src_elem, at, flip, v);
  else v[0] = perm_value(src, src_elem, at);
}

// ROWS route: VEC consecutive voxels of acc per thread, every channel. from = source offset of the first (flip: of the LAST) of them,
// to = accumulator offset of the first, both within a channel.
template <int ACT, int VEC>
__device__ __forceinline__ void unperm_rows(const void* src, int src_elem, float* acc, int c, long long V, size_t sample, long long from,
                                            bool flip, long long to, float weight, int init) {
  if (ACT == MI355_ACT_SOFTMAX) {
    float x[PERM_MAX_C][VEC], mx[VEC], sum[VEC];
    for (int k = 0; k < VEC; ++k) { mx[k] = -3.0e38f; sum[k] = 0.f; }
#pragma unroll
    for (int ch = 0; ch < PERM_MAX_C; ++ch) {
      if (ch < c) {
        unperm_load<VEC>(src, src_elem, (sample * c + ch) * (size_t)V + (size_t)from, flip, x[ch]);
        for (int k = 0; k < VEC; ++k) mx[k] = x[ch][k] > mx[k] ? x[ch][k] : mx[k];
      }
    }
#pragma unroll
    for (int ch = 0; ch < PERM_MAX_C; ++ch)
      if (ch < c)
        for (int k = 0; k < VEC; ++k) { x[ch][k] = expf(x[ch][k] - mx[k]); sum[k] += x[ch][k]; }
#pragma unroll
    for (int ch = 0; ch < PERM_MAX_C; ++ch) {
      if (ch < c) {
        float p[VEC];
        for (int k = 0; k < VEC; ++k) p[k] = x[ch][k] / sum[k];
        unperm_store<VEC>(acc + (sample * c + ch) * (size_t)V + (size_t)to, p, weight, init);
      }
    }
  } else {
    for (int ch = 0; ch < c; ++ch) {
      float p[VEC];
      unperm_load<VEC>(src, src_elem, (sample * c + ch) * (size_t)V + (size_t)from, flip, p);
      if (ACT == MI355_ACT_SIGMOID)
        for (int k = 0; k < VEC; ++k) p[k] = perm_sigmoid(p[k]);
      unperm_store<VEC>(acc + (sample * c + ch) * (size_t)V + (size_t)to, p, weight, init);
    }
  }
}

// grid (workgroups per sample on the longest route, n). (e0, e1, e2) = extents of src; the codes are the INVERSE ones: acc is the output.
template <int ACT>
__global__ void __launch_bounds__(256) unpermute_accumulate_kernel(const void* src, int src_elem, float* acc, int c, int e0, int e1, int e2,
                                                                   PermCodes codes, int per_sample, int vec_ok, float weight, int init) {
  __shared__ float tile[PT][PT + 1];
  const PermMap m = perm_map(codes.code[per_sample ? blockIdx.y : 0], e0, e1, e2);
  const long long V = (long long)e0 * e1 * e2;
  const size_t sample = blockIdx.y;
  if (m.rows) {
    const int W = m.O[2];
    const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
    if (item >= (vec_ok ? V / 4 : V)) return;
    const int per_row = vec_ok ? W / 4 : W;
    const long long row = item / per_row;
    const int x0 = (int)(item - row * per_row) * (vec_ok ? 4 : 1);
    const int v0 = (int)(row / m.O[1]), v1 = (int)(row - (long long)v0 * m.O[1]);
    const long long from = m.base + v0 * m.step[0] + v1 * m.step[1];
    const bool flip = m.step[2] < 0;
    if (vec_ok) unperm_rows<ACT, 4>(src, src_elem, acc, c, V, sample, flip ? from - (long long)(x0 + 3) : from + x0, flip, row * W + x0, weight, init);
    else unperm_rows<ACT, 1>(src, src_elem, acc, c, V, sample, from + x0 * m.step[2], false, row * W + x0, weight, init);
    return;
  }
  const int b = m.b, r = 1 - b;
  const int Ob = pick3(b, m.O[0], m.O[1], 0), Or = pick3(r, m.O[0], m.O[1], 0), O2 = m.O[2];
  const long long step_b = b == 0 ? m.step[0] : m.step[1], step_r = r == 0 ? m.step[0] : m.step[1];
  const int tiles_b = (Ob + PT - 1) / PT, tiles_2 = (O2 + PT - 1) / PT;
  const long long unit = blockIdx.x;
  if (unit >= (long long)tiles_b * tiles_2 * Or) return;
  const int tb = (int)(unit % tiles_b), t2 = (int)((unit / tiles_b) % tiles_2), vr = (int)(unit / ((long long)tiles_b * tiles_2));
  const int tx = threadIdx.x & (PT - 1), ty = threadIdx.x / PT;
  const int vb_in = tb * PT + tx;                                             // loading: lanes along source W
  const long long from = m.base + vr * step_r + vb_in * step_b;
  const int v2_out = t2 * PT + tx;                                            // storing: lanes along the accumulator's W
  float mx[PT_ROWS], sum[PT_ROWS];
  if (ACT == MI355_ACT_SOFTMAX) {
#pragma unroll
    for (int k = 0; k < PT_ROWS; ++k) {
      const int v2 = t2 * PT + ty + 4 * k;
      mx[k] = -3.0e38f; sum[k] = 0.f;
      if (vb_in < Ob && v2 < O2) {
        for (int ch = 0; ch < c; ++ch) {
          const float xv = perm_value(src, src_elem, (sample * c + ch) * (size_t)V + (size_t)(from + v2 * m.step[2]));
          mx[k] = xv > mx[k] ? xv : mx[k];
        }
        for (int ch = 0; ch < c; ++ch)
          sum[k] += expf(perm_value(src, src_elem, (sample * c + ch) * (size_t)V + (size_t)(from + v2 * m.step[2])) - mx[k]);
      }
    }
  }
  for (int ch = 0; ch < c; ++ch) {
    const size_t vol = (sample * c + ch) * (size_t)V;
#pragma unroll
    for (int k = 0; k < PT_ROWS; ++k) {
      const int i2 = ty + 4 * k, v2 = t2 * PT + i2;
      if (vb_in < Ob && v2 < O2) {
        float p = perm_value(src, src_elem, vol + (size_t)(from + v2 * m.step[2]));
        if (ACT == MI355_ACT_SIGMOID) p = perm_sigmoid(p);
        if (ACT == MI355_ACT_SOFTMAX) p = expf(p - mx[k]) / sum[k];
        tile[i2][tx] = p;
      }
    }
    __syncthreads();
    for (int k = 0; k < PT_ROWS; ++k) {
      const int jb = ty + 4 * k, vb = tb * PT + jb;
      if (vb < Ob && v2_out < O2) {
        const long long row = b == 0 ? (long long)vb * m.O[1] + vr : (long long)vr * m.O[1] + vb;
        float* a = acc + vol + (size_t)(row * O2 + v2_out);
        a[0] = perm_fold(init ? 0.f : a[0], tile[tx][jb], weight, init);
      }
    }
    __syncthreads();                                                         // the tile is free for the next channel
  }
}

extern "C" int mi355_unpermute_accumulate(const void* src, int32_t src_elem, float* acc, int32_t n, int32_t c, int32_t d, int32_t h, int32_t w,
                                          const int32_t* codes, int32_t n_codes, int32_t activation, float weight, int32_t init, void* stream) {
  if (!src || !acc || src == (const void*)acc) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  if (src_elem != MI355_ACT_F32 && src_elem != MI355_ACT_BF16 && src_elem != MI355_ACT_F16) return MI355_EINVAL;
  if (activation != MI355_ACT_NONE && activation != MI355_ACT_SIGMOID && activation != MI355_ACT_SOFTMAX) return MI355_EINVAL;
  if (activation == MI355_ACT_SOFTMAX && c > PERM_MAX_C) return MI355_EINVAL;
  if (weight != weight) return MI355_EINVAL;
  const int E[3] = {d, h, w};
  int P[3];                                                   // the extents of src: what the forward codes make of (d, h, w)
  PermCodes fwd, inv;
  rc = perm_gather_codes(codes, n_codes, n, E, fwd, P); if (rc) return rc;
  for (int i = 0; i < MI355_PERMUTE_MAX_BATCH; ++i) inv.code[i] = (unsigned short)(i < n_codes ? perm_inverse(fwd.code[i]) : 0);
  const int src_bytes = src_elem == MI355_ACT_F32 ? 4 : 2;
  const int vec_ok = (uintptr_t)src % (4 * src_bytes) == 0 && (uintptr_t)acc % 16 == 0 && w % 4 == 0;
  long long units = 0;
  for (int i = 0; i < n_codes; ++i) {
    const long long u = perm_units(inv.code[i], E, vec_ok ? 4 : 1);
    units = u > units ? u : units;
  }
  const dim3 grid((unsigned)units, n);
  const int per_sample = n_codes > 1;
  const int in = init != 0;
  if (activation == MI355_ACT_NONE) LAUNCH(unpermute_accumulate_kernel<MI355_ACT_NONE>, grid, dim3(256), 0, stream, src, (int)src_elem, acc, (int)c, P[0], P[1], P[2], inv, per_sample, vec_ok, weight, in);
  else if (activation == MI355_ACT_SIGMOID) LAUNCH(unpermute_accumulate_kernel<MI355_ACT_SIGMOID>, grid, dim3(256), 0, stream, src, (int)src_elem, acc, (int)c, P[0], P[1], P[2], inv, per_sample, vec_ok, weight, in);
  else LAUNCH(unpermute_accumulate_kernel<MI355_ACT_SOFTMAX>, grid, dim3(256), 0, stream, src, (int)src_elem, acc, (int)c, P[0], P[1], P[2], inv, per_sample, vec_ok, weight, in);
  return LAUNCH_CHECK();
}
