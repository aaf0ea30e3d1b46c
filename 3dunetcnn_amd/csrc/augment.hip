// Training augmentation of a whole batch on the device (unet3d/datasets/segmentation.py:75-94: spatial augmentations on image and label
// together, then intensity normalisation, then intensity augmentations on the image) -- two launches per batch.
//
//  pass A (augment_resample_kernel): one workgroup = one brick of 64 (x) * 4 (y) * 16 (z) OUTPUT voxels of one sample; a wave owns one
//         64-voxel row at a time (x across the lanes: every store is one full 256-byte row, and the eight source corners of neighbouring
//         lanes of a slightly rotated row share cache lines) and walks the brick's 16 z. Per voxel the map M_n is evaluated once; the
//         image channels are blended from it (trilinear), the label channels picked (nearest, round half to even). With `normalize` it
//         leaves one (sum, sum of squares) record per (brick, channel) of the values it wrote, shifted by K = the channel's first SOURCE
//         voxel (shifted_mean_rstd of volume_common.h: the fp32 sums then carry deviations, not the level).
//  pass B (augment_finalize_kernel): every workgroup folds the records of its (sample, channel) in one fixed order (fp64), then applies
//         (x - mean) * rstd * gain + offset in place with 16-byte accesses.
//  No atomics anywhere: two runs give the same bits. Without `normalize` pass B does not run: gain and offset (if given) go into pass A's
//  store. A map whose coordinates are integers (flips, crops, identity) copies source voxels bit for bit.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#include "volume_common.h"

#define AUG_BX 64
#define AUG_BY 4
#define AUG_BZ 16
#define AUG_CG 4                     // image channels carried per walk of the brick (their sums live in registers)
#define AUG_B_THREADS 256
#define AUG_B_ITERS 32               // pass B: 256 threads * 4 floats * 32 = 32768 values per workgroup

struct AugArgs {
  const float* img; float* out;
  const void* lbl; void* lbl_out;
  const float* m; const float* gain; const float* offset;
  float* rec;
  int n, ci, cl, lbl_f32;
  int sd, sh, sw, dd, dh, dw;
  int nbx, nby, nbz;
  int padding, normalize;
};

__global__ __launch_bounds__(AUG_BX * AUG_BY) void augment_resample_kernel(AugArgs a) {
  __shared__ float red[AUG_BY][AUG_CG][2];
  const int lane = threadIdx.x, wave = threadIdx.y;
  const int n = blockIdx.y;
  int b = blockIdx.x;
  const int bx = b % a.nbx; b /= a.nbx;
  const int by = b % a.nby, bz = b / a.nby;
  const int x = bx * AUG_BX + lane, y = by * AUG_BY + wave, z0 = bz * AUG_BZ;
  const bool live = x < a.dw && y < a.dh;
  const long long SV = (long long)a.sd * a.sh * a.sw, DV = (long long)a.dd * a.dh * a.dw;
  const float* M = a.m + (size_t)n * 12;
  // the part of the map that does not change along z
  const float bz_ = M[1] * (float)y + M[2] * (float)x + M[3], mzz = M[0];
  const float by_ = M[5] * (float)y + M[6] * (float)x + M[7], myz = M[4];
  const float bx_ = M[9] * (float)y + M[10] * (float)x + M[11], mxz = M[8];
  const int nz = (a.dd - z0) < AUG_BZ ? (a.dd - z0) : AUG_BZ;
  const bool affine = !a.normalize && (a.gain || a.offset);
  const int ngroups = (a.ci + AUG_CG - 1) / AUG_CG;

  for (int g = 0; g < ngroups; ++g) {
    const int c0 = g * AUG_CG;
    float s0[AUG_CG], s1[AUG_CG], K[AUG_CG], ga[AUG_CG], of[AUG_CG];
    const float* sc[AUG_CG]; float* dc[AUG_CG];
#pragma unroll
    for (int j = 0; j < AUG_CG; ++j) {
      const int c = (c0 + j < a.ci) ? c0 + j : a.ci - 1;     // a short last group repeats its last channel (never stored, never recorded)
      sc[j] = a.img + ((size_t)n * a.ci + c) * SV;
      dc[j] = a.out + ((size_t)n * a.ci + c) * DV;
      s0[j] = 0.f; s1[j] = 0.f;
      K[j] = a.normalize ? sc[j][0] : 0.f;
      ga[j] = (affine && a.gain) ? a.gain[(size_t)n * a.ci + c] : 1.f;
      of[j] = (affine && a.offset) ? a.offset[(size_t)n * a.ci + c] : 0.f;
    }
    if (live) {
      for (int k = 0; k < nz; ++k) {
        const int z = z0 + k;
        const float fzv = (float)z;
        const float cz0 = mzz * fzv + bz_, cy0 = myz * fzv + by_, cx0 = mxz * fzv + bx_;
        const size_t v = ((size_t)z * a.dh + y) * a.dw + x;
        if (g == 0 && a.lbl) {
          // labels: the nearest source voxel of the same coordinates (rintf: half to even)
          bool inside;
          const size_t o = nearest_source(cz0, cy0, cx0, false, a.sd, a.sh, a.sw, inside);
          const bool zero = a.padding == 1 && !inside;
          if (a.lbl_f32) {
            const float* ls = (const float*)a.lbl + (size_t)n * a.cl * SV; float* ld = (float*)a.lbl_out + (size_t)n * a.cl * DV;
            for (int c = 0; c < a.cl; ++c) ld[(size_t)c * DV + v] = zero ? 0.f : ls[(size_t)c * SV + o];
          } else {
            const unsigned char* ls = (const unsigned char*)a.lbl + (size_t)n * a.cl * SV;
            unsigned char* ld = (unsigned char*)a.lbl_out + (size_t)n * a.cl * DV;
            for (int c = 0; c < a.cl; ++c) ld[(size_t)c * DV + v] = zero ? (unsigned char)0 : ls[(size_t)c * SV + o];
          }
        }
        float cz = cz0, cy = cy0, cx = cx0;           // trilinear_setup of volume_common.h written out: see there (the helper costs eight VGPRs here)
        if (a.padding == 0) { cz = clamp_coord(cz, (float)(a.sd - 1)); cy = clamp_coord(cy, (float)(a.sh - 1)); cx = clamp_coord(cx, (float)(a.sw - 1)); }
        const float fz = floorf(cz), fy = floorf(cy), fx = floorf(cx);
        const float lz = cz - fz, ly = cy - fy, lx = cx - fx;
        const int iz0 = (int)fz, iy0 = (int)fy, ix0 = (int)fx;
        const bool exact = lz == 0.f && ly == 0.f && lx == 0.f;        // the output voxel IS a source voxel: copied, not blended
        float wgt[8]; size_t off[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int qa = q >> 2, qb = (q >> 1) & 1, qe = q & 1;
          int iz = iz0 + qa, iy = iy0 + qb, ix = ix0 + qe;
          float w = (qa ? lz : 1.f - lz) * (qb ? ly : 1.f - ly) * (qe ? lx : 1.f - lx);
          const bool inside = iz >= 0 && iy >= 0 && ix >= 0 && iz < a.sd && iy < a.sh && ix < a.sw;
          if (!inside) {
            if (a.padding == 1) w = 0.f;           // zeros outside; with border padding the clamp above leaves only weight-0 corners outside
            iz = clamp_index(iz, a.sd); iy = clamp_index(iy, a.sh); ix = clamp_index(ix, a.sw);
          }
          wgt[q] = w; off[q] = ((size_t)iz * a.sh + iy) * a.sw + ix;
        }
#pragma unroll
        for (int j = 0; j < AUG_CG; ++j) {
          if (c0 + j >= a.ci) continue;
          float val;
          if (exact) val = wgt[0] != 0.f ? sc[j][off[0]] : 0.f;
          else val = trilinear_blend(sc[j], wgt, off);
          const float t = val - K[j];
          s0[j] += t; s1[j] += t * t;
          dc[j][v] = affine ? val * ga[j] + of[j] : val;
        }
      }
    }
    if (a.normalize) {
      // lanes -> wave by cross-lane adds, waves -> workgroup through LDS in wave order
#pragma unroll
      for (int j = 0; j < AUG_CG; ++j) {
        float p0 = s0[j], p1 = s1[j];
        for (int d = 32; d > 0; d >>= 1) { p0 += __shfl_down(p0, d, 64); p1 += __shfl_down(p1, d, 64); }
        if (lane == 0) { red[wave][j][0] = p0; red[wave][j][1] = p1; }
      }
      __syncthreads();
      if (wave == 0 && lane < AUG_CG && c0 + lane < a.ci) {
        float r0 = 0.f, r1 = 0.f;
        for (int w = 0; w < AUG_BY; ++w) { r0 += red[w][lane][0]; r1 += red[w][lane][1]; }
        float* r = a.rec + (((size_t)n * a.ci + c0 + lane) * gridDim.x + blockIdx.x) * 2;
        r[0] = r0; r[1] = r1;
      }
      __syncthreads();
    }
  }
}

// grid (chunks of a channel, n * ci). rec: [n * ci][nrec][2]; K as in pass A.
__global__ __launch_bounds__(AUG_B_THREADS) void augment_finalize_kernel(float* out, const float* img, const float* rec, const float* gain,
                                                                        const float* offset, int nrec, long long SV, long long DV, int vec) {
  __shared__ double r0[AUG_B_THREADS], r1[AUG_B_THREADS];
  __shared__ float stat[2];
  const int nc = blockIdx.y, t = threadIdx.x;
  const float* r = rec + (size_t)nc * nrec * 2;
  double a0 = 0.0, a1 = 0.0;
  for (int i = t; i < nrec; i += AUG_B_THREADS) { a0 += (double)r[2 * i]; a1 += (double)r[2 * i + 1]; }
  block_sum_256(r0, r1, a0, a1);
  if (t == 0) shifted_mean_rstd((double)img[(size_t)nc * SV], r0[0], r1[0], (double)DV, stat[0], stat[1]);
  __syncthreads();
  const float mean = stat[0];
  const float sc = stat[1] * (gain ? gain[nc] : 1.f), of = offset ? offset[nc] : 0.f;
  float* o = out + (size_t)nc * DV;
  const long long chunk = (long long)AUG_B_THREADS * 4 * AUG_B_ITERS;
  const long long lo = (long long)blockIdx.x * chunk;
  const long long hi = lo + chunk < DV ? lo + chunk : DV;
  if (vec) {                       // DV % 4 == 0 and a 16-byte aligned tensor: every channel starts on a 16-byte boundary
    for (long long i = lo + 4 * t; i < hi; i += 4 * AUG_B_THREADS) {
      float4 q = *reinterpret_cast<float4*>(o + i);
      q.x = (q.x - mean) * sc + of; q.y = (q.y - mean) * sc + of; q.z = (q.z - mean) * sc + of; q.w = (q.w - mean) * sc + of;
      *reinterpret_cast<float4*>(o + i) = q;
    }
  } else {
    for (long long i = lo + t; i < hi; i += AUG_B_THREADS) o[i] = (o[i] - mean) * sc + of;
  }
}

static inline long long aug_bricks(int dd, int dh, int dw) {
  return (long long)ceil_div(dw, AUG_BX) * ceil_div(dh, AUG_BY) * ceil_div(dd, AUG_BZ);
}

extern "C" size_t mi355_augment_batch_workspace(int32_t n, int32_t ci, int32_t dd, int32_t dh, int32_t dw) {
  if (n < 1 || ci < 1 || dd < 1 || dh < 1 || dw < 1) return 0;
  return (size_t)n * ci * (size_t)aug_bricks(dd, dh, dw) * 2 * sizeof(float);
}

extern "C" int mi355_augment_batch(const float* image, float* out, const void* label, void* label_out, int32_t label_dtype, int32_t n,
                                   int32_t ci, int32_t cl, int32_t sd, int32_t sh, int32_t sw, int32_t dd, int32_t dh, int32_t dw,
                                   const float* m, const float* gain, const float* offset, int32_t padding, int32_t normalize, void* ws,
                                   size_t ws_bytes, void* stream) {
  if (!image || !out || !m || n < 1 || ci < 1 || sd < 1 || sh < 1 || sw < 1 || dd < 1 || dh < 1 || dw < 1) return MI355_EINVAL;
  if (padding < 0 || padding > 1) return MI355_EINVAL;
  if ((label != nullptr) != (label_out != nullptr)) return MI355_EINVAL;
  if (label && (cl < 1 || (label_dtype != MI355_LABEL_U8 && label_dtype != MI355_LABEL_F32))) return MI355_EINVAL;
  const long long bricks = aug_bricks(dd, dh, dw);
  if (bricks > 0x7fffffffLL || n > 65535 || (long long)n * ci > 65535) return MI355_EUNSUPPORTED;
  if (normalize) {
    if (!ws) return MI355_EINVAL;
    if (ws_bytes < mi355_augment_batch_workspace(n, ci, dd, dh, dw)) return MI355_EWORKSPACE;
  }
  AugArgs a;
  a.img = image; a.out = out; a.lbl = label; a.lbl_out = label_out; a.m = m; a.gain = gain; a.offset = offset; a.rec = (float*)ws;
  a.n = n; a.ci = ci; a.cl = label ? cl : 0; a.lbl_f32 = label_dtype == MI355_LABEL_F32;
  a.sd = sd; a.sh = sh; a.sw = sw; a.dd = dd; a.dh = dh; a.dw = dw;
  a.nbx = ceil_div(dw, AUG_BX); a.nby = ceil_div(dh, AUG_BY); a.nbz = ceil_div(dd, AUG_BZ);
  a.padding = padding; a.normalize = normalize ? 1 : 0;
  LAUNCH(augment_resample_kernel, dim3((unsigned)bricks, n), dim3(AUG_BX, AUG_BY), 0, stream, a);
  int rc = LAUNCH_CHECK();
  if (rc || !normalize) return rc;
  const long long SV = (long long)sd * sh * sw, DV = (long long)dd * dh * dw;
  const long long chunk = (long long)AUG_B_THREADS * 4 * AUG_B_ITERS;
  const int vec = DV % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
  LAUNCH(augment_finalize_kernel, dim3((unsigned)((DV + chunk - 1) / chunk), n * ci), dim3(AUG_B_THREADS), 0, stream, out, image,
         (const float*)ws, gain, offset, (int)bricks, SV, DV, vec);
  return LAUNCH_CHECK();
}
