// The internal interface of the convolution sources (conv3d_*.hip), host code only: every function one of them defines and another calls,
// and the small answers they share (a padded channel count, whether a grid fits a launch, a well-formed norm prologue). A new cross-file
// function of the conv family is declared HERE and nowhere else: a declaration that drifts from its definition then fails to compile or link.
// (Not for conv3d_bf16_zring.hip / conv3d_lp.h: the plane-ring launches are declared in conv3d_lp.h, beside the ConvBArgs they take.)
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/mi355_unet3d.h"
struct GnFuseArgs;      // gn_fuse.h

// ---- cross-file functions -----------------------------------------------------------------------------------------------------------
// conv3d_fwd.hip: the one validation and copy of a call's statistics request (moments_out / mi355_gn_bwd_fuse) into a kernel's arguments
int mi355_fill_gn_fuse(GnFuseArgs& g, const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
// conv3d_bf16.hip: the 3x3x3 stride-1 forward on 16-bit operands
int mi355_conv3d_fwd_bf16_impl(const mi355_act* x, const void* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream);
int mi355_conv3d_bf16_kernel_name(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d, char* out, size_t n);
int32_t mi355_conv3d_bf16_stats_blocks(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
// conv3d_c4.hip: the first-layer kernels (4 input channels) and the <= 4 output channel forward
int mi355_conv3d_c4_ok(const mi355_act* x, const mi355_conv_desc* d);
int mi355_conv3d_c4_fwd_impl(const mi355_act* x, const float* w, const mi355_act* y, const mi355_conv_desc* d, void* stream);
size_t mi355_conv3d_c4_wgrad_workspace(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
int mi355_conv3d_c4_wgrad_impl(const mi355_act* x, const mi355_act* dy, float* dw, const mi355_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
void conv3d_c4_wgrad_reduce_launch(const float* ws, float* dw, int Cout, int splits, void* stream);
int mi355_conv3d_narrow_ok(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
int mi355_conv3d_narrow_impl(const mi355_act* x, const float* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream);
// conv3d_s2.hip: the z-marching 32 -> 32 channel stride-2 forward, data gradient and weight gradient
int mi355_conv3d_s2c32_ok(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
int32_t mi355_conv3d_s2c32_stats_blocks(const mi355_act* y);
int mi355_conv3d_s2c32_fwd_impl(const mi355_act* x, const float* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream);
int mi355_conv3d_s2c32_dgrad_ok(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
int mi355_conv3d_s2c32_dgrad_impl(const mi355_act* x, const float* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream);
int mi355_conv3d_s2c32_wgrad_ok(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
size_t mi355_conv3d_s2c32_wgrad_workspace(const mi355_act* dy);
int mi355_conv3d_s2c32_wgrad_impl(const mi355_act* x, const mi355_act* dy, float* dw, const mi355_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
// conv3d_k1_stream.hip: 1x1x1 forward / data gradient of bf16 tensors as wave streams
int mi355_conv3d_k1_stream_ok(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d);
int mi355_conv3d_k1_stream_impl(const mi355_act* x, const float* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream);
// conv3d_wgrad.hip: partial slabs of a weight gradient -> dw
int mi355_wgrad_reduce_launch(const float* ws, float* dw, int Cout, int Cin, int T, int SL, int ciTiles, void* stream);
// conv3d_wgrad_bf16.hip: the 3x3x3 stride-1 weight gradient on 16-bit operands
size_t mi355_conv3d_wgrad_bf16_workspace(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
int mi355_conv3d_wgrad_bf16_impl(const mi355_act* x, const mi355_act* dy, float* dw, const mi355_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
// conv3d_wgrad_lp.hip: the z-marching 3x3x3 and the streaming 1x1x1 weight gradient of 16-bit tensors
int mi355_conv3d_wgrad_lp_tr_ok(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
size_t mi355_conv3d_wgrad_lp_tr_workspace(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
int mi355_conv3d_wgrad_lp_tr_impl(const mi355_act* x, const mi355_act* dy, float* dw, const mi355_conv_desc* d, void* ws, size_t ws_bytes, void* stream);
int mi355_conv3d_wgrad_k1_lp_ok(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
size_t mi355_conv3d_wgrad_k1_lp_workspace(const mi355_act* x, const mi355_act* dy, const mi355_conv_desc* d);
int mi355_conv3d_wgrad_k1_lp_impl(const mi355_act* x, const mi355_act* dy, float* dw, const mi355_conv_desc* d, void* ws, size_t ws_bytes, void* stream);

// ---- shared host answers --------------------------------------------------------------------------------------------------------------
// channel counts as the packs and kernels pad them: to the 32-channel output tile, the 8-channel fp32 chunk, the 16-channel 16-bit chunk
static inline int pad32(int c) { return (c + 31) / 32 * 32; }
static inline int pad8(int c) { return (c + 7) / 8 * 8; }
static inline int pad16(int c) { return (c + 15) / 16 * 16; }
// a workgroup count a one-dimensional grid takes
static inline bool grid_fits(long long blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }
// epilogue records per sample, or 0: this call cannot fuse statistics
static inline int32_t records_or_0(long long b) { return grid_fits(b) ? (int32_t)b : 0; }
// grid of a weight-pack launch (256 threads, grid-stride): one thread per item, at most 4096 workgroups
static inline int pack_grid(size_t items) { const int grid = (int)((items + 255) / 256); return grid > 4096 ? 4096 : grid; }
// the norm prologue of a descriptor is well formed: scale and shift present, act(u) = max(u, slope * u) with 0 <= slope <= 1 (not NaN)
static inline bool affine_prologue_ok(const mi355_conv_desc* d) {
  return d->in_mode != MI355_IN_AFFINE_ACT || (d->in_scale && d->in_shift && d->act_slope >= 0.f && d->act_slope <= 1.f);
}
