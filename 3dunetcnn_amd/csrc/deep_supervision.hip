// Deep-supervision heads of DynUNet (MONAI DynUNet(deep_supervision=True), restated from memory -- see 3dunetcnn_amd/dynunet.py):
//   head_i = UnetOutBlock(filters[i + 1] -> out_channels, k = 1, bias) on the activated output of the up block at level i + 1,
//   torch.stack([out] + [F.interpolate(head_i, out.shape[2:])], dim=1)          (interpolation "nearest": src = floor(dst / 2^(i + 1)))
// Forward: 1x1x1 projection of a coarse NDHWC tensor whose result lands nearest-up-sampled by `factor` in a contiguous fp32 NCDHW slot of the
// stacked output. Backward: the slot's gradient is read once, every factor^3 block summed to the coarse gradient dz, from which dw / dbias
// (per-workgroup partials + a fixed-order reduce: bitwise reproducible) and wT dz, ADDED to the decoder level's gradient, follow.
// The projection itself is the few-class one of pointwise.hip (same prologue, same tile scheme) with a 32-voxel tile, so that 320 input
// channels fit the 64 KiB LDS window.
#include "gfx950_dialect.h"
#include <cstdlib>
#include "../../include/mi355_unet3d.h"
#include "act_io.h"

#define DS_MAX_COUT 8
#define DS_MAX_CIN 320            // MONAI's default filter cap for spatial_dims == 3
#define DS_TV 32                  // coarse voxels per tile (256 threads = 32 voxels x 8 classes)
#define DS_MAX_BLOCKS 512         // workgroups of the backward = partial tables of dw / dbias
#define DS_MAX_PART ((DS_MAX_COUT * DS_MAX_CIN + DS_MAX_COUT + 255) / 256)

// fused prologue act(scale[n,c] * x + shift[n,c]) applied while staging the x tile (proj_prologue of pointwise.hip)
__device__ __forceinline__ float4 ds_prologue(float4 v, const float* sc, const float* sh, float slope, int n, int Cin, int c) {
  if (!sc) return v;
  const float4 s4 = *reinterpret_cast<const float4*>(sc + (size_t)n * Cin + c);
  const float4 h4 = *reinterpret_cast<const float4*>(sh + (size_t)n * Cin + c);
  v.x = v.x * s4.x + h4.x; v.y = v.y * s4.y + h4.y; v.z = v.z * s4.z + h4.z; v.w = v.w * s4.w + h4.w;
  v.x = fmaxf(v.x, v.x * slope); v.y = fmaxf(v.y, v.y * slope); v.z = fmaxf(v.z, v.z * slope); v.w = fmaxf(v.w, v.w * slope);   // 0 <= slope <= 1
  return v;
}

// the tile's activated input [DS_TV][Cin + 1] (rows past the volume: 0) and, per coarse voxel, the offset of its first fine voxel inside one
// (n, class) volume of the fine tensor (-1 past the volume)
template <typename T>
__device__ __forceinline__ void ds_stage_tile(const T* x, int xld, const float* sc, const float* sh, float slope, int n, long long v0, long long V,
                                              int H, int W, int Cin, int lf, float* lx, long long* lo) {
  const int tid = threadIdx.x, Q = Cin / 4, XS = Cin + 1;
  for (int i = tid; i < DS_TV * Q; i += 256) {
    const int v = i / Q, q = i % Q;
    float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v0 + v < V) val = ds_prologue(ld4(x + ((size_t)n * V + v0 + v) * xld + 4 * q), sc, sh, slope, n, Cin, 4 * q);
    float* d = lx + v * XS + 4 * q; d[0] = val.x; d[1] = val.y; d[2] = val.z; d[3] = val.w;
  }
  if (tid < DS_TV) {
    const long long v = v0 + tid;
    long long o = -1;
    if (v < V) {
      const long long xq = v % W, r = v / W, y = r % H, z = r / H;
      const long long Hf = (long long)H << lf, Wf = (long long)W << lf;
      o = ((z << lf) * Hf + (y << lf)) * Wf + (xq << lf);
    }
    lo[tid] = o;
  }
}

// VW floats per store: 4 (16 bytes) where factor >= 4, 2 for factor 2. A unit of the store phase is one such store; consecutive units walk
// (piece of a coarse voxel's run, coarse voxel) first, so a wavefront covers the contiguous fine rows of consecutive coarse voxels.
template <typename T, int VW>
__global__ __launch_bounds__(256) void ds_head_fwd_kernel(const T* x, int xld, const float* sc, const float* sh, float slope, const float* w,
                                                          const float* bias, float* out, int N, int D, int H, int W, int Cin, int Cout, int lf) {
  DYN_LDS(lds);                    // fine offsets [DS_TV] (8 bytes each) | x tile [DS_TV][Cin+1] | w [Cout][Cin] | z [Cout][DS_TV]
  const int XS = Cin + 1;
  long long* lo = reinterpret_cast<long long*>(lds);
  float* lx = lds + 2 * DS_TV; float* lw = lx + DS_TV * XS; float* lz = lw + Cout * Cin;
  const int tid = threadIdx.x;
  for (int i = tid; i < Cout * Cin; i += 256) lw[i] = w[i];
  const long long V = (long long)D * H * W, Vf = V << (3 * lf);
  const long long Hf = (long long)H << lf, Wf = (long long)W << lf;
  const long long tilesPerN = (V + DS_TV - 1) / DS_TV, ntiles = (long long)N * tilesPerN;
  const int f = 1 << lf, cqb = lf - (VW == 4 ? 2 : 1);            // 2^cqb stores per coarse voxel and fine row
  const int units = Cout << (2 * lf + 5 + cqb);
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = (int)(tile / tilesPerN); const long long v0 = (tile % tilesPerN) * DS_TV;
    __syncthreads();
    ds_stage_tile(x, xld, sc, sh, slope, n, v0, V, H, W, Cin, lf, lx, lo);
    __syncthreads();
    {
      const int v = tid & (DS_TV - 1), co = tid >> 5;
      if (co < Cout) {
        float acc = bias ? bias[co] : 0.f;
        for (int ci = 0; ci < Cin; ++ci) acc += lx[v * XS + ci] * lw[co * Cin + ci];
        lz[co * DS_TV + v] = acc;
      }
    }
    __syncthreads();
    for (int u = tid; u < units; u += 256) {
      const int cq = u & ((1 << cqb) - 1), v = (u >> cqb) & (DS_TV - 1), b = (u >> (cqb + 5)) & (f - 1), a = (u >> (cqb + 5 + lf)) & (f - 1);
      const int co = u >> (cqb + 5 + 2 * lf);
      const long long base = lo[v];
      if (base < 0) continue;
      const float val = lz[co * DS_TV + v];
      float* p = out + ((size_t)n * Cout + co) * Vf + base + ((long long)a * Hf + b) * Wf + cq * VW;
      if constexpr (VW == 4) st4(p, make_float4(val, val, val, val));
      else *reinterpret_cast<float2*>(p) = make_float2(val, val);
    }
  }
}

// dz tile (the factor^3 block sums of the fine gradient) + dx += wT dz + per-block partial dw / dbias
template <typename T, int VW>
__global__ __launch_bounds__(256) void ds_head_bwd_kernel(const T* x, int xld, const float* sc, const float* sh, float slope, const float* w,
                                                          const float* dout, T* dx, int dxld, float* ws, int N, int D, int H, int W, int Cin,
                                                          int Cout, int lf) {
  DYN_LDS(lds);                    // fine offsets [DS_TV] | x tile [DS_TV][Cin+1] | w [Cout][Cin] | dz [Cout][DS_TV] | run sums [Cout][DS_TV][2^cqb]
  const int XS = Cin + 1;
  long long* lo = reinterpret_cast<long long*>(lds);
  float* lx = lds + 2 * DS_TV; float* lw = lx + DS_TV * XS; float* lz = lw + Cout * Cin; float* lp = lz + DS_MAX_COUT * DS_TV;
  const int tid = threadIdx.x, Q = Cin / 4;
  for (int i = tid; i < Cout * Cin; i += 256) lw[i] = w[i];
  const int npairs = Cout * Cin + Cout;     // dw entries then dbias entries
  float part[DS_MAX_PART];
#pragma unroll
  for (int k = 0; k < DS_MAX_PART; ++k) part[k] = 0.f;
  const long long V = (long long)D * H * W, Vf = V << (3 * lf);
  const long long Hf = (long long)H << lf, Wf = (long long)W << lf;
  const long long tilesPerN = (V + DS_TV - 1) / DS_TV, ntiles = (long long)N * tilesPerN;
  const int f = 1 << lf, cqb = lf - (VW == 4 ? 2 : 1);
  const int combos = Cout << (5 + cqb);     // (class, coarse voxel, piece of its fine run): each summed over the f x f fine rows by one thread
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n = (int)(tile / tilesPerN); const long long v0 = (tile % tilesPerN) * DS_TV;
    __syncthreads();
    ds_stage_tile(x, xld, sc, sh, slope, n, v0, V, H, W, Cin, lf, lx, lo);
    __syncthreads();
    // consecutive threads read consecutive pieces of the fine rows of consecutive coarse voxels; fixed order: (a: (b: 4 values pairwise))
    for (int c = tid; c < combos; c += 256) {
      const int cq = c & ((1 << cqb) - 1), v = (c >> cqb) & (DS_TV - 1), co = c >> (cqb + 5);
      const long long base = lo[v];
      float s = 0.f;
      if (base >= 0) {
        const float* p0 = dout + ((size_t)n * Cout + co) * Vf + base + cq * VW;
        for (int a = 0; a < f; ++a) {
          float sa = 0.f;
          for (int b = 0; b < f; ++b) {
            const float* p = p0 + ((long long)a * Hf + b) * Wf;
            if constexpr (VW == 4) { const float4 g = ld4(p); sa += (g.x + g.y) + (g.z + g.w); }
            else { const float2 g = *reinterpret_cast<const float2*>(p); sa += g.x + g.y; }
          }
          s += sa;
        }
      }
      lp[c] = s;
    }
    __syncthreads();
    for (int i = tid; i < Cout * DS_TV; i += 256) {
      float t = 0.f;
      for (int cq = 0; cq < (1 << cqb); ++cq) t += lp[(i << cqb) + cq];
      lz[i] = t;
    }
    __syncthreads();
    // partial dw / dbias: entry e -> (co, ci) or bias co
#pragma unroll
    for (int k = 0; k < DS_MAX_PART; ++k) {
      const int e = tid + 256 * k;
      if (e < npairs) {
        float s = 0.f;
        if (e < Cout * Cin) {
          const int co = e / Cin, ci = e % Cin;
          for (int v = 0; v < DS_TV; ++v) s += lz[co * DS_TV + v] * lx[v * XS + ci];
        } else {
          const int co = e - Cout * Cin;
          for (int v = 0; v < DS_TV; ++v) s += lz[co * DS_TV + v];
        }
        part[k] += s;
      }
    }
    // dx of this tile: thread (v, quad) adds 4 channels of wT dz to what the level's gradient already holds, in fp32, one rounding on store
    if (dx) {
      for (int i = tid; i < DS_TV * Q; i += 256) {
        const int v = i / Q, q = i % Q;
        if (v0 + v >= V) continue;
        T* d = dx + ((size_t)n * V + v0 + v) * dxld + 4 * q;
        const float4 old = ld4(d);
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        for (int co = 0; co < Cout; ++co) {
          const float g = lz[co * DS_TV + v];
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] += g * lw[co * Cin + 4 * q + e];
        }
        st4(d, make_float4(old.x + o[0], old.y + o[1], old.z + o[2], old.w + o[3]));
      }
    }
  }
#pragma unroll
  for (int k = 0; k < DS_MAX_PART; ++k) {
    const int e = tid + 256 * k;
    if (e < npairs) ws[(size_t)blockIdx.x * npairs + e] = part[k];
  }
}

// 8 output elements per workgroup x 32 lanes striding the per-block partials; lanes combined through LDS in a fixed order
__global__ __launch_bounds__(256) void ds_head_reduce_kernel(const float* ws, int nblocks, int npairs, int ndw, float* dw, float* dbias) {
  __shared__ double part[8][32];
  const int l = threadIdx.x & 31, k = threadIdx.x >> 5;
  const int e = blockIdx.x * 8 + k;
  double s = 0.0;
  if (e < npairs)
    for (int b = l; b < nblocks; b += 32) s += (double)ws[(size_t)b * npairs + e];
  part[k][l] = s;
  __syncthreads();
  if (l == 0 && e < npairs) {
    double t = 0.0;
    for (int i = 0; i < 32; ++i) t += part[k][i];
    if (e < ndw) dw[e] = (float)t;
    else if (dbias) dbias[e - ndw] = (float)t;
  }
}

static long long ds_tiles(const mi355_act* x) {
  const long long V = (long long)x->d * x->h * x->w;
  return (long long)x->n * ((V + DS_TV - 1) / DS_TV);
}

static int ds_bwd_blocks(const mi355_act* x) {
  const long long t = ds_tiles(x);
  return (int)(t > DS_MAX_BLOCKS ? DS_MAX_BLOCKS : (t < 1 ? 1 : t));
}

// log2(factor) for a power of two in [2, 32]; -1 otherwise
static int ds_log2_factor(int32_t factor) {
  for (int lf = 1; lf <= 5; ++lf)
    if (factor == (1 << lf)) return lf;
  return -1;
}

// what both entry points ask of (x, prologue, w, the fine tensor, cout, factor)
static int ds_args_ok(const mi355_act* x, const float* in_scale, const float* in_shift, float act_slope, const float* w, const float* fine,
                      int32_t cout, int32_t factor) {
  if (!act_view_ok(x) || !w || !fine || ((uintptr_t)fine & 15) || cout < 1 || cout > DS_MAX_COUT || x->c > DS_MAX_CIN) return 0;
  if (x->n < 1 || x->d < 1 || x->h < 1 || x->w < 1 || ds_log2_factor(factor) < 0) return 0;
  if ((long long)x->d * factor > 0x7fffffffLL || (long long)x->h * factor > 0x7fffffffLL || (long long)x->w * factor > 0x7fffffffLL) return 0;
  if ((in_scale == nullptr) != (in_shift == nullptr)) return 0;
  if (((uintptr_t)in_scale & 15) || ((uintptr_t)in_shift & 15) || ((uintptr_t)w & 3)) return 0;      // the prologue reads 4 channels per load
  if (in_scale && !(act_slope >= 0.f && act_slope <= 1.f)) return 0;       // act(u) = max(u, slope * u)
  return 1;
}

extern "C" size_t mi355_ds_head_scratch_bytes(const mi355_act* x, int32_t cout) {
  if (!x) return 0;
  return (size_t)ds_bwd_blocks(x) * ((size_t)cout * x->c + cout) * sizeof(float);
}

extern "C" int mi355_ds_head_fwd(const mi355_act* x, const float* in_scale, const float* in_shift, float act_slope, const float* w,
                                 const float* bias, float* out_ncdhw, int32_t cout, int32_t factor, void* stream) {
  if (!ds_args_ok(x, in_scale, in_shift, act_slope, w, out_ncdhw, cout, factor) || ((uintptr_t)bias & 3)) return MI355_EINVAL;
  const int lf = ds_log2_factor(factor);
  const size_t lds = ((size_t)2 * DS_TV + (size_t)DS_TV * (x->c + 1) + (size_t)cout * x->c + (size_t)cout * DS_TV) * sizeof(float);
  long long grid = ds_tiles(x); if (grid > 8 * DS_MAX_BLOCKS) grid = 8 * DS_MAX_BLOCKS;
  if (lf >= 2)
    ACT_TYPED(x->dtype, T, LAUNCH((ds_head_fwd_kernel<T, 4>), dim3((unsigned)grid), dim3(256), lds, stream, (const T*)x->p, x->ld, in_scale, in_shift, act_slope,
                                  w, bias, out_ncdhw, x->n, x->d, x->h, x->w, x->c, cout, lf));
  else
    ACT_TYPED(x->dtype, T, LAUNCH((ds_head_fwd_kernel<T, 2>), dim3((unsigned)grid), dim3(256), lds, stream, (const T*)x->p, x->ld, in_scale, in_shift, act_slope,
                                  w, bias, out_ncdhw, x->n, x->d, x->h, x->w, x->c, cout, lf));
  return LAUNCH_CHECK();
}

extern "C" int mi355_ds_head_bwd(const mi355_act* x, const float* in_scale, const float* in_shift, float act_slope, const float* w,
                                 const float* dout_ncdhw, const mi355_act* dx, float* dw, float* dbias, int32_t cout, int32_t factor,
                                 void* ws, size_t ws_bytes, void* stream) {
  if (!ds_args_ok(x, in_scale, in_shift, act_slope, w, dout_ncdhw, cout, factor) || !dw || !ws) return MI355_EINVAL;
  if (((uintptr_t)dw & 3) || ((uintptr_t)dbias & 3) || ((uintptr_t)ws & 3)) return MI355_EINVAL;
  if (dx && (!act_view_ok(dx) || dx->n != x->n || dx->d != x->d || dx->h != x->h || dx->w != x->w || dx->c != x->c)) return MI355_EINVAL;
  if (dx && dx->dtype != x->dtype) return MI355_EUNSUPPORTED;
  if (ws_bytes < mi355_ds_head_scratch_bytes(x, cout)) return MI355_EWORKSPACE;
  const int lf = ds_log2_factor(factor);
  const int cqb = lf - (lf >= 2 ? 2 : 1);
  const size_t lds = ((size_t)2 * DS_TV + (size_t)DS_TV * (x->c + 1) + (size_t)cout * x->c + (size_t)DS_MAX_COUT * DS_TV +
                      ((size_t)cout * DS_TV << cqb)) * sizeof(float);
  const int nb = ds_bwd_blocks(x);
  const int npairs = cout * x->c + cout;
  if (lf >= 2)
    ACT_TYPED(x->dtype, T, LAUNCH((ds_head_bwd_kernel<T, 4>), dim3(nb), dim3(256), lds, stream, (const T*)x->p, x->ld, in_scale, in_shift, act_slope, w, dout_ncdhw,
                                  dx ? (T*)dx->p : (T*)nullptr, dx ? dx->ld : 0, (float*)ws, x->n, x->d, x->h, x->w, x->c, cout, lf));
  else
    ACT_TYPED(x->dtype, T, LAUNCH((ds_head_bwd_kernel<T, 2>), dim3(nb), dim3(256), lds, stream, (const T*)x->p, x->ld, in_scale, in_shift, act_slope, w, dout_ncdhw,
                                  dx ? (T*)dx->p : (T*)nullptr, dx ? dx->ld : 0, (float*)ws, x->n, x->d, x->h, x->w, x->c, cout, lf));
  int rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(ds_head_reduce_kernel, dim3(ceil_div(npairs, 8)), dim3(256), 0, stream, (const float*)ws, nb, npairs, cout * x->c, dw, dbias);
  return LAUNCH_CHECK();
}
