// Residual block of DynUNet (MONAI UnetResBlock, restated from memory -- see 3dunetcnn_amd/dynunet.py):
//   out = lrelu(norm1(conv1(x)));  out = norm2(conv2(out));  res = norm3(conv3(x));  out = lrelu(out + res)
// The engine keeps conv outputs RAW and folds each norm into a per-(n, c) scale / shift pair. The block's output is a function of TWO raw
// tensors with two sets of statistics, which no conv prologue expresses, so it is materialised here:
//   res_join_fwd_kernel     A = lrelu(sc2 * r2 + sh2 + sc3 * r3 + sh3)                                         2 reads, 1 write, 1 launch
//   res_join_bwd            g = dA * (A > 0 ? 1 : slope); both InstanceNorm backwards under the same g          8 reads, 2 writes, 3 launches
// and the shortcut of the down-sampling blocks, Conv3d(k = 1, stride = 2, no bias): r3[n, z, y, x, :] = W3 x[n, 2z, 2y, 2x, :]
//   c1s2_gemm_kernel<T, 1>  forward: gathers the even voxels of x
//   c1s2_gemm_kernel<T, 0>  data gradient, ADDED into the even voxels of an existing fine gradient (one voxel in eight)
//   c1s2_wgrad_kernel       dW3[co][ci] = sum d_r3 * x(even voxels): per-split partial matrices + a fixed-order reduce
// Every reduction is per-workgroup partials combined in a fixed order (double): no floating-point atomics, two runs give the same bits.
// The shortcut's arithmetic is fp32 fma on the vector ALU in every precision mode (under 1 % of the block's flops).
#include "gfx950_dialect.h"
#include <cstdlib>
#include "../../include/mi355_unet3d.h"
#include "act_io.h"

#define RJ_MAX_BLOCKS_PER_SAMPLE 1024     // workgroups (= partial records) per sample of the backward's first pass
#define RJ_MIN_VOXELS_PER_BLOCK 16
#define C1S2_MAX_C 384                    // channel cap of the shortcut conv, either side (BraTS bottleneck: 256 -> 384)
#define C1S2_TV 32                        // coarse voxels per tile of the forward / data-gradient kernel
#define C1S2_WT 64                        // edge of the weight-gradient tile (co x ci)
#define C1S2_MAX_SPLITS 256
#define C1S2_SPLIT_VOXELS 256             // coarse voxels per split, at least
#define C1S2_MAX_WS_FLOATS (4u << 20)     // partial matrices of the weight gradient: at most 16 MiB

// ---- join ------------------------------------------------------------------------------------------------------------------------------
// grid (B, N), Q * R threads: a thread keeps ONE channel run q = tid % Q (its scale / shift in registers) and walks the voxels
// vb + r, vb + r + R, ... of its block's share.
template <typename T, int VW>
__global__ __launch_bounds__(256) void res_join_fwd_kernel(const T* r2, int r2ld, const T* r3, int r3ld, T* a, int ald, long long V, int C, int Q,
                                                           int R, const float* sc2, const float* sh2, const float* sc3, const float* sh3,
                                                           float slope) {
  const int tid = threadIdx.x, q = tid % Q, r = tid / Q, c = VW * q;
  const int n = blockIdx.y, B = gridDim.x;
  const long long per = (V + B - 1) / B, vb = (long long)blockIdx.x * per, ve = vb + per < V ? vb + per : V;
  float s2[VW], s3[VW], h[VW], t[VW];
  ldv<VW>(sc2 + (size_t)n * C + c, s2);
  ldv<VW>(sc3 + (size_t)n * C + c, s3);
  ldv<VW>(sh2 + (size_t)n * C + c, h);
  ldv<VW>(sh3 + (size_t)n * C + c, t);
#pragma unroll
  for (int e = 0; e < VW; ++e) h[e] += t[e];
  const size_t nb = (size_t)n * V;
#pragma unroll 2
  for (long long v = vb + r; v < ve; v += R) {
    float x2[VW], x3[VW], o[VW];
    ldv<VW>(r2 + (nb + v) * r2ld + c, x2);
    ldv<VW>(r3 + (nb + v) * r3ld + c, x3);
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const float u = fmaf(s3[e], x3[e], fmaf(s2[e], x2[e], h[e]));
      o[e] = fmaxf(u, u * slope);                       // 0 <= slope <= 1
    }
    stv<VW>(a + (nb + v) * ald + c, o);
  }
}

// first pass of the backward: per (n, block, c) the sums (g, g * xhat2, g * xhat3), xhat_b = (r_b - mean_b) * rstd_b.
// The backward's arithmetic is DOUBLE from here to the store of d_r2 / d_r3: gamma rstd (g - mean(g) - xhat mean(g xhat)) cancels -- completely
// for a plane of two voxels, to ~eps / var of its terms -- and fp32 products would leave 2^-24 of the TERMS in a result that small. Both
// passes stay bound by their eight tensor reads (about ten fp64 operations per element against 16 / 8 bytes moved).
template <typename T, int VW>
__global__ __launch_bounds__(256) void res_join_bwd_partial_kernel(const T* a, int ald, const T* da, int dald, const T* r2, int r2ld, const T* r3,
                                                                   int r3ld, long long V, int C, int Q, int R, float slope, const float* mr2,
                                                                   const float* mr3, double* part) {
  DYN_LDS(lds);
  double* rj_lds = reinterpret_cast<double*>(lds);  // [R][Q][3 VW]
  const int tid = threadIdx.x, q = tid % Q, r = tid / Q, c = VW * q;
  const int n = blockIdx.y, blk = blockIdx.x, B = gridDim.x;
  const long long per = (V + B - 1) / B, vb = (long long)blk * per, ve = vb + per < V ? vb + per : V;
  double m2[VW], i2[VW], m3[VW], i3[VW], s0[VW], s2[VW], s3[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    const size_t k = ((size_t)n * C + c + e) * 2;
    m2[e] = (double)mr2[k]; i2[e] = (double)mr2[k + 1]; m3[e] = (double)mr3[k]; i3[e] = (double)mr3[k + 1];
    s0[e] = 0.0; s2[e] = 0.0; s3[e] = 0.0;
  }
  const double dslope = (double)slope;
  const size_t nb = (size_t)n * V;
  for (long long v = vb + r; v < ve; v += R) {
    float av[VW], dv[VW], x2[VW], x3[VW];
    ldv<VW>(a + (nb + v) * ald + c, av);
    ldv<VW>(da + (nb + v) * dald + c, dv);
    ldv<VW>(r2 + (nb + v) * r2ld + c, x2);
    ldv<VW>(r3 + (nb + v) * r3ld + c, x3);
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const double g = av[e] > 0.f ? (double)dv[e] : (double)dv[e] * dslope;
      s0[e] += g; s2[e] += g * (((double)x2[e] - m2[e]) * i2[e]); s3[e] += g * (((double)x3[e] - m3[e]) * i3[e]);
    }
  }
  double* my = rj_lds + (size_t)tid * (3 * VW);
#pragma unroll
  for (int e = 0; e < VW; ++e) { my[e] = s0[e]; my[VW + e] = s2[e]; my[2 * VW + e] = s3[e]; }
  __syncthreads();
  if (r == 0) {
    double t[3 * VW];
#pragma unroll
    for (int e = 0; e < 3 * VW; ++e) t[e] = 0.0;
    for (int rr = 0; rr < R; ++rr) {
      const double* o = rj_lds + (size_t)(rr * Q + q) * (3 * VW);
#pragma unroll
      for (int e = 0; e < 3 * VW; ++e) t[e] += o[e];
    }
    double* dst = part + (((size_t)n * B + blk) * C + c) * 3;
#pragma unroll
    for (int e = 0; e < VW; ++e) { dst[3 * e] = t[e]; dst[3 * e + 1] = t[VW + e]; dst[3 * e + 2] = t[2 * VW + e]; }
  }
}

// 32 channels x 8 slices of the record range per workgroup, samples in turn: per (n, c) the coefficients of both branches,
//   d_r = k0 * g + k1 + k2 * (r - mean),  k0 = gamma rstd, k1 = -k0 sum(g) / V, k2 = -k0 rstd sum(g xhat) / V
// coef[n][c][6] = branch 2 | branch 3 (double), and dgamma_b[c] = sum_n sum(g xhat_b), dbeta_b[c] = sum_n sum(g). Fixed order.
__global__ __launch_bounds__(256) void res_join_bwd_finalize_kernel(const double* part, int B, int C, int N, long long V, const float* gamma2,
                                                                    const float* mr2, const float* gamma3, const float* mr3, double* coef,
                                                                    float* dgamma2, float* dbeta2, float* dgamma3, float* dbeta3) {
  __shared__ double p0[256], p1[256], p2[256];
  const int tid = threadIdx.x, ci = tid & 31, sl = tid >> 5;
  const int c = blockIdx.x * 32 + ci;
  double dg2 = 0.0, dg3 = 0.0, db = 0.0;
  for (int n = 0; n < N; ++n) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (c < C)
      for (int blk = sl; blk < B; blk += 8) {
        const double* r = part + (((size_t)n * B + blk) * C + c) * 3;
        a0 += r[0]; a1 += r[1]; a2 += r[2];
      }
    p0[tid] = a0; p1[tid] = a1; p2[tid] = a2;
    __syncthreads();
    if (sl == 0 && c < C) {
      double s0 = 0.0, s2 = 0.0, s3 = 0.0;
      for (int k = 0; k < 8; ++k) { s0 += p0[k * 32 + ci]; s2 += p1[k * 32 + ci]; s3 += p2[k * 32 + ci]; }
      const size_t m = ((size_t)n * C + c) * 2;
      double* k = coef + ((size_t)n * C + c) * 6;
      const double ga2 = gamma2 ? (double)gamma2[c] : 1.0, ga3 = gamma3 ? (double)gamma3[c] : 1.0;
      const double rs2 = (double)mr2[m + 1], rs3 = (double)mr3[m + 1], dV = (double)V;
      k[0] = ga2 * rs2; k[1] = -ga2 * rs2 * s0 / dV; k[2] = -ga2 * rs2 * rs2 * s2 / dV;
      k[3] = ga3 * rs3; k[4] = -ga3 * rs3 * s0 / dV; k[5] = -ga3 * rs3 * rs3 * s3 / dV;
      db += s0; dg2 += s2; dg3 += s3;
    }
    __syncthreads();
  }
  if (sl == 0 && c < C) {
    dgamma2[c] = (float)dg2; dbeta2[c] = (float)db; dgamma3[c] = (float)dg3; dbeta3[c] = (float)db;
  }
}

// second pass: the same thread map as the forward; d_r2 may be dA itself (each element is read, then written, by one thread)
template <typename T, int VW>
__global__ __launch_bounds__(256) void res_join_bwd_apply_kernel(const T* a, int ald, const T* da, int dald, const T* r2, int r2ld, const T* r3,
                                                                 int r3ld, T* d2, int d2ld, T* d3, int d3ld, long long V, int C, int Q, int R,
                                                                 float slope, const float* mr2, const float* mr3, const double* coef) {
  const int tid = threadIdx.x, q = tid % Q, r = tid / Q, c = VW * q;
  const int n = blockIdx.y, B = gridDim.x;
  const long long per = (V + B - 1) / B, vb = (long long)blockIdx.x * per, ve = vb + per < V ? vb + per : V;
  double k[VW][6], m2[VW], m3[VW];
#pragma unroll
  for (int e = 0; e < VW; ++e) {
    const double* src = coef + ((size_t)n * C + c + e) * 6;
#pragma unroll
    for (int j = 0; j < 6; ++j) k[e][j] = src[j];
    m2[e] = (double)mr2[((size_t)n * C + c + e) * 2]; m3[e] = (double)mr3[((size_t)n * C + c + e) * 2];
  }
  const double dslope = (double)slope;
  const size_t nb = (size_t)n * V;
  for (long long v = vb + r; v < ve; v += R) {
    float av[VW], dv[VW], x2[VW], x3[VW], o2[VW], o3[VW];
    ldv<VW>(a + (nb + v) * ald + c, av);
    ldv<VW>(da + (nb + v) * dald + c, dv);
    ldv<VW>(r2 + (nb + v) * r2ld + c, x2);
    ldv<VW>(r3 + (nb + v) * r3ld + c, x3);
#pragma unroll
    for (int e = 0; e < VW; ++e) {
      const double g = av[e] > 0.f ? (double)dv[e] : (double)dv[e] * dslope;
      o2[e] = (float)(k[e][0] * g + k[e][1] + k[e][2] * ((double)x2[e] - m2[e]));
      o3[e] = (float)(k[e][3] * g + k[e][4] + k[e][5] * ((double)x3[e] - m3[e]));
    }
    stv<VW>(d2 + (nb + v) * d2ld + c, o2);
    stv<VW>(d3 + (nb + v) * d3ld + c, o3);
  }
}

static long long rj_voxels(const mi355_act* t) { return (long long)t->d * t->h * t->w; }

static int rj_partial_blocks(long long V) {
  long long b = V / RJ_MIN_VOXELS_PER_BLOCK;
  if (b < 1) b = 1;
  if (b > RJ_MAX_BLOCKS_PER_SAMPLE) b = RJ_MAX_BLOCKS_PER_SAMPLE;
  return (int)b;
}

// blocks per sample of the two streaming passes: at least 8 voxels per thread where the tensor allows, at most ~16K workgroups per launch
static int rj_stream_blocks(long long V, int R, int N) {
  long long b = (V + (long long)R * 8 - 1) / ((long long)R * 8);
  const long long cap = (16384 + N - 1) / N;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

static int rj_same_view(const mi355_act* ref, const mi355_act* t) {
  return act_view_ok(t) && t->n == ref->n && t->d == ref->d && t->h == ref->h && t->w == ref->w && t->c == ref->c;
}

// 0, or the status of a set of views that is not one (n, d, h, w, c) in one storage type
static int rj_check(const mi355_act* ref, const mi355_act* const* others, int count) {
  if (!act_view_ok(ref) || ref->n < 1 || ref->d < 1 || ref->h < 1 || ref->w < 1) return MI355_EINVAL;
  for (int i = 0; i < count; ++i)
    if (!rj_same_view(ref, others[i])) return MI355_EINVAL;
  for (int i = 0; i < count; ++i)
    if (others[i]->dtype != ref->dtype) return MI355_EUNSUPPORTED;
  if (ref->c / 4 > 256 || ref->n > 65535) return MI355_EUNSUPPORTED;
  return 0;
}

extern "C" size_t mi355_res_join_scratch_bytes(const mi355_act* a) {
  if (!a) return 0;
  return ((size_t)a->n * rj_partial_blocks(rj_voxels(a)) * a->c * 3 + (size_t)a->n * a->c * 6) * sizeof(double);
}

extern "C" int mi355_res_join_fwd(const mi355_act* r2, const mi355_act* r3, const float* scale2, const float* shift2, const float* scale3,
                                  const float* shift3, float act_slope, const mi355_act* a, void* stream) {
  const mi355_act* others[2] = {r3, a};
  int rc = rj_check(r2, others, 2);
  if (rc) return rc;
  if (!scale2 || !shift2 || !scale3 || !shift3) return MI355_EINVAL;
  if (((uintptr_t)scale2 | (uintptr_t)shift2 | (uintptr_t)scale3 | (uintptr_t)shift3) & 15) return MI355_EINVAL;
  if (!(act_slope >= 0.f && act_slope <= 1.f)) return MI355_EINVAL;
  const long long V = rj_voxels(r2);
  const int C = r2->c, N = r2->n;
  if (act_vw8(r2) && act_vw8(r3) && act_vw8(a)) {
    const int Q = C / 8, R = 256 / Q > 0 ? 256 / Q : 1;
    ACT_TYPED_LP16(r2->dtype, T, LAUNCH((res_join_fwd_kernel<T, 8>), dim3(rj_stream_blocks(V, R, N), N), dim3(Q * R), 0, stream, (const T*)r2->p, r2->ld,
                                        (const T*)r3->p, r3->ld, (T*)a->p, a->ld, V, C, Q, R, scale2, shift2, scale3, shift3, act_slope));
  } else {
    const int Q = C / 4, R = 256 / Q > 0 ? 256 / Q : 1;
    ACT_TYPED(r2->dtype, T, LAUNCH((res_join_fwd_kernel<T, 4>), dim3(rj_stream_blocks(V, R, N), N), dim3(Q * R), 0, stream, (const T*)r2->p, r2->ld,
                                   (const T*)r3->p, r3->ld, (T*)a->p, a->ld, V, C, Q, R, scale2, shift2, scale3, shift3, act_slope));
  }
  return LAUNCH_CHECK();
}

extern "C" int mi355_res_join_bwd(const mi355_act* a, const mi355_act* da, const mi355_act* r2, const mi355_act* r3, float act_slope,
                                  const float* gamma2, const float* mean_rstd2, const float* gamma3, const float* mean_rstd3,
                                  const mi355_act* d_r2, const mi355_act* d_r3, float* dgamma2, float* dbeta2, float* dgamma3, float* dbeta3,
                                  void* ws, size_t ws_bytes, void* stream) {
  const mi355_act* others[5] = {da, r2, r3, d_r2, d_r3};
  int rc = rj_check(a, others, 5);
  if (rc) return rc;
  if (!mean_rstd2 || !mean_rstd3 || !dgamma2 || !dbeta2 || !dgamma3 || !dbeta3 || !ws || ((uintptr_t)ws & 15)) return MI355_EINVAL;
  if (!(act_slope >= 0.f && act_slope <= 1.f)) return MI355_EINVAL;
  // d_r2 may BE dA (same base, same leading dimension); any other overlap of an output with a tensor this call reads is refused
  if (d_r2->p == da->p && d_r2->ld != da->ld) return MI355_EINVAL;
  if (d_r3->p == da->p || d_r3->p == a->p || d_r3->p == r2->p || d_r3->p == r3->p || d_r3->p == d_r2->p || d_r2->p == a->p || d_r2->p == r2->p ||
      d_r2->p == r3->p)
    return MI355_EINVAL;
  if (ws_bytes < mi355_res_join_scratch_bytes(a)) return MI355_EWORKSPACE;
  const long long V = rj_voxels(a);
  const int C = a->c, N = a->n, B = rj_partial_blocks(V);
  double* part = (double*)ws;
  double* coef = part + (size_t)N * B * C * 3;
  const bool vw8 = act_vw8(a) && act_vw8(da) && act_vw8(r2) && act_vw8(r3) && act_vw8(d_r2) && act_vw8(d_r3);
  const int VW = vw8 ? 8 : 4, Q = C / VW, R = 256 / Q > 0 ? 256 / Q : 1;
  if (vw8)
    ACT_TYPED_LP16(a->dtype, T, LAUNCH((res_join_bwd_partial_kernel<T, 8>), dim3(B, N), dim3(Q * R), (size_t)Q * R * 24 * sizeof(double), stream, (const T*)a->p,
                                       a->ld, (const T*)da->p, da->ld, (const T*)r2->p, r2->ld, (const T*)r3->p, r3->ld, V, C, Q, R, act_slope, mean_rstd2,
                                       mean_rstd3, part));
  else
    ACT_TYPED(a->dtype, T, LAUNCH((res_join_bwd_partial_kernel<T, 4>), dim3(B, N), dim3(Q * R), (size_t)Q * R * 12 * sizeof(double), stream, (const T*)a->p,
                                  a->ld, (const T*)da->p, da->ld, (const T*)r2->p, r2->ld, (const T*)r3->p, r3->ld, V, C, Q, R, act_slope, mean_rstd2,
                                  mean_rstd3, part));
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(res_join_bwd_finalize_kernel, dim3(ceil_div(C, 32)), dim3(256), 0, stream, (const double*)part, B, C, N, V, gamma2, mean_rstd2, gamma3,
         mean_rstd3, coef, dgamma2, dbeta2, dgamma3, dbeta3);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  const int B2 = rj_stream_blocks(V, R, N);
  if (vw8)
    ACT_TYPED_LP16(a->dtype, T, LAUNCH((res_join_bwd_apply_kernel<T, 8>), dim3(B2, N), dim3(Q * R), 0, stream, (const T*)a->p, a->ld, (const T*)da->p, da->ld,
                                       (const T*)r2->p, r2->ld, (const T*)r3->p, r3->ld, (T*)d_r2->p, d_r2->ld, (T*)d_r3->p, d_r3->ld, V, C, Q, R, act_slope,
                                       mean_rstd2, mean_rstd3, (const double*)coef));
  else
    ACT_TYPED(a->dtype, T, LAUNCH((res_join_bwd_apply_kernel<T, 4>), dim3(B2, N), dim3(Q * R), 0, stream, (const T*)a->p, a->ld, (const T*)da->p, da->ld,
                                  (const T*)r2->p, r2->ld, (const T*)r3->p, r3->ld, (T*)d_r2->p, d_r2->ld, (T*)d_r3->p, d_r3->ld, V, C, Q, R, act_slope,
                                  mean_rstd2, mean_rstd3, (const double*)coef));
  return LAUNCH_CHECK();
}

// ---- 1x1x1 stride-2 shortcut conv --------------------------------------------------------------------------------------------------------
// element offset (in voxels) of the fine voxel (2z, 2y, 2x) of sample n, from the coarse voxel's linear index over [N][Dc][Hc][Wc]
__device__ __forceinline__ size_t c1s2_fine_voxel(long long cv, int Dc, int Hc, int Wc) {
  const long long x = cv % Wc, t = cv / Wc, y = t % Hc, u = t / Hc, z = u % Dc, n = u / Dc;
  return (size_t)(((n * (2LL * Dc) + 2 * z) * (2LL * Hc) + 2 * y) * (2LL * Wc) + 2 * x);
}

// out[v][o] (+)= sum_k in[v][k] * W(k, o) over tiles of C1S2_TV coarse voxels. FWD: `in` is the fine tensor read at its even voxels, `out`
// the coarse one, W(k, o) = w[o * K + k] (k = ci, o = co). Otherwise: `in` is the coarse gradient, `out` the fine gradient whose even
// voxels are read, added to and written back, W(k, o) = w[k * O + o] (k = co, o = ci). A thread owns 4 voxels x 4 output channels of a
// tile; the tile's input rows are staged in LDS once (whole rows, 16-byte loads of fp32 / 8-byte loads of 16-bit elements).
template <typename T, int FWD>
__global__ __launch_bounds__(256) void c1s2_gemm_kernel(const T* in, int inld, const float* w, T* out, int outld, long long NV, int Dc, int Hc, int Wc,
                                                        int K, int O) {
  DYN_LDS(lds);                    // fine-voxel offsets [C1S2_TV] (8 bytes each) | input rows [C1S2_TV][K + 4]
  long long* lo = reinterpret_cast<long long*>(lds);
  float* lin = lds + 2 * C1S2_TV;
  const int KS = K + 4, KQ = K / 4, OQ = O / 4, tid = threadIdx.x;
  const long long ntiles = (NV + C1S2_TV - 1) / C1S2_TV;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long v0 = tile * C1S2_TV;
    __syncthreads();
    if (tid < C1S2_TV) lo[tid] = v0 + tid < NV ? (long long)c1s2_fine_voxel(v0 + tid, Dc, Hc, Wc) : -1;
    __syncthreads();
    for (int i = tid; i < C1S2_TV * KQ; i += 256) {
      const int v = i / KQ, kq = i % KQ;
      float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lo[v] >= 0) val = ld4(in + (FWD ? (size_t)lo[v] : (size_t)(v0 + v)) * inld + 4 * kq);
      *reinterpret_cast<float4*>(lin + v * KS + 4 * kq) = val;
    }
    __syncthreads();
    for (int item = tid; item < (C1S2_TV / 4) * OQ; item += 256) {
      const int oq = item % OQ, vg = item / OQ;
      float acc[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = 0.f;
      for (int k = 0; k < K; k += 4) {
        float wb[4][4];            // [kk][e] = W(k + kk, 4 oq + e)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if constexpr (FWD) {
            const float4 t = *reinterpret_cast<const float4*>(w + (size_t)(4 * oq + i) * K + k);
            wb[0][i] = t.x; wb[1][i] = t.y; wb[2][i] = t.z; wb[3][i] = t.w;
          } else {
            const float4 t = *reinterpret_cast<const float4*>(w + (size_t)(k + i) * O + 4 * oq);
            wb[i][0] = t.x; wb[i][1] = t.y; wb[i][2] = t.z; wb[i][3] = t.w;
          }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 xi = *reinterpret_cast<const float4*>(lin + (4 * vg + j) * KS + k);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            acc[j][e] = fmaf(xi.w, wb[3][e], fmaf(xi.z, wb[2][e], fmaf(xi.y, wb[1][e], fmaf(xi.x, wb[0][e], acc[j][e]))));
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int v = 4 * vg + j;
        if (lo[v] < 0) continue;
        T* d = out + (FWD ? (size_t)(v0 + v) : (size_t)lo[v]) * outld + 4 * oq;
        float4 r = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        if constexpr (!FWD) { const float4 old = ld4(d); r.x += old.x; r.y += old.y; r.z += old.z; r.w += old.w; }
        st4(d, r);
      }
    }
  }
}

// grid (co tiles * ci tiles, splits): the split's share of the coarse voxels, 32 at a time: dy rows [32][64] and x rows [32][64] in LDS, a
// thread owns 4 co x 4 ci of the 64 x 64 tile. ws[split][cout][cin]; a split past the last voxel writes zeros.
template <typename T>
__global__ __launch_bounds__(256) void c1s2_wgrad_kernel(const T* x, int xld, const T* dy, int dyld, float* ws, long long NV, int Dc, int Hc, int Wc,
                                                         int Cin, int Cout, int tiles_ci) {
  __shared__ __attribute__((aligned(16))) float ld_[C1S2_TV][C1S2_WT + 4];
  __shared__ __attribute__((aligned(16))) float lx_[C1S2_TV][C1S2_WT + 4];
  __shared__ long long lo[C1S2_TV];
  const int tid = threadIdx.x, tci = tid & 15, tco = tid >> 4;
  const int ci0 = (blockIdx.x % tiles_ci) * C1S2_WT, co0 = (blockIdx.x / tiles_ci) * C1S2_WT;
  const int S = gridDim.y, s = blockIdx.y;
  const long long per = (NV + S - 1) / S, vb = (long long)s * per, ve = vb + per < NV ? vb + per : NV;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
  for (long long v0 = vb; v0 < ve; v0 += C1S2_TV) {
    __syncthreads();
    if (tid < C1S2_TV) lo[tid] = v0 + tid < ve ? (long long)c1s2_fine_voxel(v0 + tid, Dc, Hc, Wc) : -1;
    __syncthreads();
    for (int i = tid; i < C1S2_TV * (C1S2_WT / 4); i += 256) {
      const int v = i / (C1S2_WT / 4), cq = i % (C1S2_WT / 4);
      float4 dv = make_float4(0.f, 0.f, 0.f, 0.f), xv = dv;
      if (lo[v] >= 0) {
        if (co0 + 4 * cq < Cout) dv = ld4(dy + (size_t)(v0 + v) * dyld + co0 + 4 * cq);
        if (ci0 + 4 * cq < Cin) xv = ld4(x + (size_t)lo[v] * xld + ci0 + 4 * cq);
      }
      *reinterpret_cast<float4*>(&ld_[v][4 * cq]) = dv;
      *reinterpret_cast<float4*>(&lx_[v][4 * cq]) = xv;
    }
    __syncthreads();
    for (int v = 0; v < C1S2_TV; ++v) {
      const float4 dv = *reinterpret_cast<const float4*>(&ld_[v][4 * tco]);
      const float4 xv = *reinterpret_cast<const float4*>(&lx_[v][4 * tci]);
      const float d4[4] = {dv.x, dv.y, dv.z, dv.w}, x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(d4[i], x4[j], acc[i][j]);
    }
  }
  const int co = co0 + 4 * tco, ci = ci0 + 4 * tci;
  if (co < Cout && ci < Cin) {
    float* dst = ws + ((size_t)s * Cout + co) * Cin + ci;
#pragma unroll
    for (int i = 0; i < 4; ++i) st4(dst + (size_t)i * Cin, make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
  }
}

__global__ __launch_bounds__(256) void c1s2_wgrad_reduce_kernel(const float* ws, int S, int E, float* dw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double t = 0.0;
  for (int s = 0; s < S; ++s) t += (double)ws[(size_t)s * E + e];
  dw[e] = (float)t;
}

// 0, or the status of a (fine, coarse) pair that is not the two sides of a 1x1x1 stride-2 conv
static int c1s2_check(const mi355_act* fine, const mi355_act* coarse) {
  if (!act_view_ok(fine) || !act_view_ok(coarse)) return MI355_EINVAL;
  if (fine->n < 1 || fine->d < 1 || fine->h < 1 || fine->w < 1 || ((fine->d | fine->h | fine->w) & 1)) return MI355_EINVAL;     // even extents only
  if (coarse->n != fine->n || 2 * (long long)coarse->d != fine->d || 2 * (long long)coarse->h != fine->h || 2 * (long long)coarse->w != fine->w) return MI355_EINVAL;
  if (fine->c > C1S2_MAX_C || coarse->c > C1S2_MAX_C || fine->dtype != coarse->dtype) return MI355_EUNSUPPORTED;
  return 0;
}

static long long c1s2_voxels(const mi355_act* coarse) { return (long long)coarse->n * coarse->d * coarse->h * coarse->w; }

static int c1s2_splits(const mi355_act* x, const mi355_act* dy) {
  const long long NV = c1s2_voxels(dy);
  long long s = (NV + C1S2_SPLIT_VOXELS - 1) / C1S2_SPLIT_VOXELS;
  const long long cap = C1S2_MAX_WS_FLOATS / ((long long)x->c * dy->c);
  if (s > cap) s = cap;
  if (s > C1S2_MAX_SPLITS) s = C1S2_MAX_SPLITS;
  if (s < 1) s = 1;
  return (int)s;
}

static unsigned c1s2_grid(long long NV) {
  const long long t = (NV + C1S2_TV - 1) / C1S2_TV;
  return (unsigned)(t > 65536 ? 65536 : t);
}

extern "C" size_t mi355_conv1x1_s2_scratch_bytes(const mi355_act* x, const mi355_act* dy) {
  if (!x || !dy || x->c < 1 || dy->c < 1) return 0;
  return (size_t)c1s2_splits(x, dy) * x->c * dy->c * sizeof(float);
}

extern "C" int mi355_conv1x1_s2_fwd(const mi355_act* x, const float* w, const mi355_act* y, void* stream) {
  int rc = c1s2_check(x, y);
  if (rc) return rc;
  if (!w || ((uintptr_t)w & 15)) return MI355_EINVAL;
  const long long NV = c1s2_voxels(y);
  const size_t lds = ((size_t)2 * C1S2_TV + (size_t)C1S2_TV * (x->c + 4)) * sizeof(float);
  ACT_TYPED(x->dtype, T, LAUNCH((c1s2_gemm_kernel<T, 1>), dim3(c1s2_grid(NV)), dim3(256), lds, stream, (const T*)x->p, x->ld, w, (T*)y->p, y->ld, NV, y->d, y->h,
                                y->w, x->c, y->c));
  return LAUNCH_CHECK();
}

extern "C" int mi355_conv1x1_s2_dgrad_add(const mi355_act* dy, const float* w, const mi355_act* dx, void* stream) {
  int rc = c1s2_check(dx, dy);
  if (rc) return rc;
  if (!w || ((uintptr_t)w & 15)) return MI355_EINVAL;
  const long long NV = c1s2_voxels(dy);
  const size_t lds = ((size_t)2 * C1S2_TV + (size_t)C1S2_TV * (dy->c + 4)) * sizeof(float);
  ACT_TYPED(dy->dtype, T, LAUNCH((c1s2_gemm_kernel<T, 0>), dim3(c1s2_grid(NV)), dim3(256), lds, stream, (const T*)dy->p, dy->ld, w, (T*)dx->p, dx->ld, NV, dy->d,
                                 dy->h, dy->w, dy->c, dx->c));
  return LAUNCH_CHECK();
}

extern "C" int mi355_conv1x1_s2_wgrad(const mi355_act* x, const mi355_act* dy, float* dw, void* ws, size_t ws_bytes, void* stream) {
  int rc = c1s2_check(x, dy);
  if (rc) return rc;
  if (!dw || !ws || ((uintptr_t)dw & 3) || ((uintptr_t)ws & 15)) return MI355_EINVAL;
  if (ws_bytes < mi355_conv1x1_s2_scratch_bytes(x, dy)) return MI355_EWORKSPACE;
  const long long NV = c1s2_voxels(dy);
  const int S = c1s2_splits(x, dy), tiles_ci = ceil_div(x->c, C1S2_WT), tiles_co = ceil_div(dy->c, C1S2_WT), E = x->c * dy->c;
  ACT_TYPED(x->dtype, T, LAUNCH((c1s2_wgrad_kernel<T>), dim3(tiles_ci * tiles_co, S), dim3(256), 0, stream, (const T*)x->p, x->ld, (const T*)dy->p, dy->ld,
                                (float*)ws, NV, dy->d, dy->h, dy->w, x->c, dy->c, tiles_ci));
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(c1s2_wgrad_reduce_kernel, dim3(ceil_div(E, 256)), dim3(256), 0, stream, (const float*)ws, S, E, dw);
  return LAUNCH_CHECK();
}
