// Focal loss (monai.losses.FocalLoss, and the focal term of DiceFocalLoss): value and d/dlogits in one streaming pass over the logits,
// on the pattern of mi355_ce_fwd_bwd (loss_optim.hip): one partial per block into the workspace, a single-block finaliser
// (loss_finalize_kernel, loss_common.h) that sums them in double in index order (no floating-point atomics: two calls on the same inputs give the same bits), `weight` /
// `accumulate_loss` / `accumulate_grad` / `grad_scale` so that the term lands on top of a Dice term the way the CE term does.
//
// Formulas (include/mi355_unet3d.h states them in full). w_c: class weight, a: the alpha factor, g: gamma.
//   sigmoid form, per element:  B = max(z,0) - z y + log1p(exp(-|z|));  u = -z (2y - 1);  M = exp(g logsigmoid(u));
//                               l = w_c a B M;   dl/dz = w_c a M [ (sigmoid(z) - y) - g B sigmoid(-u) (2y - 1) ]
//   softmax form, per voxel:    ls = log_softmax(z) over the counted channels;  l_c = -w_c a_c y_c (1 - exp(ls_c))^g ls_c;
//                               G_c = dl_c/dls_c = w_c a_c y_c [ -(1-p_c)^g + g p_c ls_c (1-p_c)^(g-1) ];  dL/dz_j = G_j - p_j sum_c G_c
// Every exponential takes a non-positive argument, so z = +-80 (and beyond) stays finite; (1-p)^g and its derivative are 0 at p == 1
// for every g > 0 (the limit), never 0 * inf.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#include "loss_common.h"

#define FOCAL_BLOCKS 1024
#define FOCAL_MAX_C 16
static_assert(FOCAL_BLOCKS * sizeof(float) == MI355_FOCAL_SCRATCH_BYTES, "MI355_FOCAL_SCRATCH_BYTES is one float per block");

struct FocalArgs {
  int N, C, c0, kind, has_alpha, accumulate;
  long long V;
  float gamma, alpha, gscale;
  const float* class_w;
};

// e = exp(-|x|) given: log(1 + exp(-|x|)) and sigmoid(x) without a second exponential
__device__ __forceinline__ float sigmoid_from(float x, float e) { const float r = 1.f / (1.f + e); return x >= 0.f ? r : e * r; }

// SOFTMAX is a template argument: the sigmoid form (the one DiceFocalLoss runs by default) keeps no per-channel arrays
template <int SOFTMAX>
__global__ void focal_kernel(const float* z, const void* target, FocalArgs a, float* dz, float* part) {
  __shared__ float red[256];
  float local = 0.f;
  const long long V = a.V, NV = (long long)a.N * V;
  const int C = a.C, c0 = a.c0, Ce = C - c0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < NV; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / V, v = i - n * V;
    const size_t base = (size_t)n * C * V + v;
    if (dz && c0 && !a.accumulate) dz[base] = 0.f;                 // include_background == 0: channel 0 takes no gradient from this term
    if constexpr (!SOFTMAX) {
      for (int c = c0; c < C; ++c) {
        const float zz = z[base + (size_t)c * V];
        const float y = loss_target(target, a.kind, V, C, n, c, v);
        const float s = 2.f * y - 1.f, u = -zz * s;
        const float ez = expf(-fabsf(zz)), l1z = log1pf(ez);
        float eu = ez, l1u = l1z;                                  // a hard target (y = 0 or 1): |u| == |z|, the same two values
        if (fabsf(s) != 1.f) { eu = expf(-fabsf(u)); l1u = log1pf(eu); }
        const float B = (zz > 0.f ? zz : 0.f) - zz * y + l1z;
        const float logsig_u = (u < 0.f ? u : 0.f) - l1u;
        const float M = expf(a.gamma * logsig_u);
        float k = a.class_w ? a.class_w[c - c0] : 1.f;
        if (a.has_alpha) k *= a.alpha * y + (1.f - a.alpha) * (1.f - y);
        local += k * B * M;
        if (dz) {
          const float g = k * M * ((sigmoid_from(zz, ez) - y) - a.gamma * B * sigmoid_from(-u, eu) * s) * a.gscale;
          float* d = dz + base + (size_t)c * V;
          *d = a.accumulate ? *d + g : g;
        }
      }
    } else {
      float zc[FOCAL_MAX_C], G[FOCAL_MAX_C];
      float mx = -3.4e38f;
#pragma unroll
      for (int j = 0; j < FOCAL_MAX_C; ++j)
        if (j < Ce) { zc[j] = z[base + (size_t)(c0 + j) * V]; mx = zc[j] > mx ? zc[j] : mx; }
      float se = 0.f;
#pragma unroll
      for (int j = 0; j < FOCAL_MAX_C; ++j)
        if (j < Ce) se += expf(zc[j] - mx);
      const float lse = mx + logf(se);
      float Gsum = 0.f;
#pragma unroll
      for (int j = 0; j < FOCAL_MAX_C; ++j)
        if (j < Ce) {
          const float y = loss_target(target, a.kind, V, C, n, c0 + j, v);
          const float ls = zc[j] - lse;
          const float q = -expm1f(ls);                             // 1 - p, exact 0 only where ls == 0
          float k = (a.class_w ? a.class_w[j] : 1.f) * y;
          if (a.has_alpha) k *= (c0 + j == 0) ? 1.f - a.alpha : a.alpha;
          float F = 1.f, dF = 0.f;                                 // (1-p)^g and g (1-p)^(g-1)
          if (a.gamma > 0.f) {
            F = q > 0.f ? expf(a.gamma * logf(q)) : 0.f;
            dF = q > 0.f ? a.gamma * F / q : 0.f;
          }
          local -= k * F * ls;
          G[j] = k * (dF * (1.f - q) * ls - F);
          Gsum += G[j];
        }
      if (dz) {
#pragma unroll
        for (int j = 0; j < FOCAL_MAX_C; ++j)
          if (j < Ce) {
            const float g = (G[j] - expf(zc[j] - lse) * Gsum) * a.gscale;
            float* d = dz + base + (size_t)(c0 + j) * V;
            *d = a.accumulate ? *d + g : g;
          }
      }
    }
  }
  block_sum_256(red, local);
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

extern "C" int mi355_focal_fwd_bwd(const mi355_focal_opts* o, const float* logits, const void* target, int32_t n, int32_t c, int64_t voxels,
                                   float weight, float* loss, int32_t accumulate_loss, float* dlogits, int32_t accumulate_grad,
                                   float grad_scale, void* ws, size_t ws_bytes, void* stream) {
  if (!o || !logits || !target || !loss || !ws || n <= 0 || c <= 0 || voxels <= 0) return MI355_EINVAL;
  if (o->mode != MI355_FOCAL_SIGMOID && o->mode != MI355_FOCAL_SOFTMAX) return MI355_EINVAL;
  if (o->target_kind < MI355_DICE_TARGET_F32 || o->target_kind > MI355_DICE_TARGET_LABELS) return MI355_EINVAL;
  if (o->reduction != MI355_DICE_REDUCE_MEAN && o->reduction != MI355_DICE_REDUCE_SUM) return MI355_EINVAL;
  if (!(o->gamma >= 0.f) || o->gamma > 3.0e38f) return MI355_EINVAL;                               // negative, NaN or infinite
  if (o->has_alpha && !(o->alpha >= 0.f && o->alpha <= 1.f)) return MI355_EINVAL;
  if (!o->include_background && c < 2) return MI355_EINVAL;
  if (c > FOCAL_MAX_C) return MI355_EUNSUPPORTED;
  if (ws_bytes < MI355_FOCAL_SCRATCH_BYTES) return MI355_EWORKSPACE;
  const int c0 = o->include_background ? 0 : 1, ce = c - c0;
  const long long NV = (long long)n * voxels;
  // MEAN: over every counted element. SUM: sum over (n, counted c) of the spatial mean -- the scale of the Dice term's "sum".
  const double count = o->reduction == MI355_DICE_REDUCE_MEAN ? (double)NV * ce : (double)voxels;
  long long g = (NV + 255) / 256; if (g > FOCAL_BLOCKS) g = FOCAL_BLOCKS;
  FocalArgs a;
  a.N = n; a.C = c; a.c0 = c0; a.kind = o->target_kind;
  a.has_alpha = o->has_alpha ? 1 : 0; a.accumulate = accumulate_grad ? 1 : 0; a.V = (long long)voxels;
  a.gamma = o->gamma; a.alpha = o->alpha; a.gscale = (float)((double)weight * (double)grad_scale / count); a.class_w = o->class_weight;
  if (o->mode == MI355_FOCAL_SOFTMAX && ce > 1)
    LAUNCH((focal_kernel<1>), dim3((unsigned)g), dim3(256), 0, stream, logits, target, a, dlogits, (float*)ws);
  else
    LAUNCH((focal_kernel<0>), dim3((unsigned)g), dim3(256), 0, stream, logits, target, a, dlogits, (float*)ws);
  int rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(loss_finalize_kernel, dim3(1), dim3(256), 0, stream, (const float*)ws, (int)g, 1.0 / count, weight, loss, accumulate_loss);
  return LAUNCH_CHECK();
}
