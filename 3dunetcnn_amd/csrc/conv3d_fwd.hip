// conv3d forward / dgrad / transposed-conv forward on gfx950 fp32 MFMA (v_mfma_f32_32x32x2_f32).
//
// Replaces torch.nn.Conv3d (reference: unet3d/models/pytorch/classification/resnet.py:12-22, called from
// myronenko.py:17-21) with the GroupNorm-apply+ReLU prologue (myronenko.py:18-19), the residual add
// (myronenko.py:56), Dropout3d scale (myronenko.py:78-79), F.pad window (segmentation/unet.py:34-40) and the
// channel-slice write of torch.cat (unet.py:42) fused in.
//
// Formulation: im2col-free implicit GEMM. M = output voxels (32 per MFMA tile), N = output channels,
// K = taps x input channels. A workgroup stages the (haloed) input tile of KC input channels in LDS once per
// channel chunk -- normalised, activated and zero-padded on the way in -- and every tap reads it at a shifted
// LDS address. Weights are pre-packed [tap][ci/4][co][4] so each lane fetches the B fragments of 4 consecutive
// MFMA k-steps with one 16-byte global load (L2 resident, software-prefetched one tap ahead).
// K ordering inside an 8-channel group: lanes 0-31 own channels 0..3, lanes 32-63 channels 4..7, k-step s uses
// (s, 4+s); A and B use the same permutation so the sum is unchanged.
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#include "gn_fuse.h"
#include "pack_values.h"
#include "act_io.h"
#include "conv_internal.h"

struct ConvArgs {
  const float* x; int xld;
  const float* wp;
  float* y; int yld;
  const float* res; int resld;
  const float* in_scale; const float* in_shift; float slope;
  const float* out_chscale; const float* bias;
  int N, Di, Hi, Wi, Cin, CinP;
  int Do, Ho, Wo, Cout, CoutP;   // logical output extent
  int yD, yH, yW, offz, offy, offx;  // destination buffer extent and window shift
  int pad;
  int tilesZ, tilesY, tilesX, coTiles;
  bool residual_or_chscale() const { return res != nullptr || out_chscale != nullptr; }
  const float* in_slope;   // per-input-channel negative slope (NULL: scalar slope)
  int outmode;             // MI355_OUT_*
  int cD, cH, cW, fC;      // IN_S2D / OUT_D2S (1x1x1 only): coarse grid extents and the fine tensor's channel count
  GnFuseArgs g;            // norm statistics fused into the epilogue (gn_fuse.h); both pointers NULL: nothing extra
};

// FULLJ: CinP is a multiple of KC, so every chunk has all KC/8 k-groups and the tap loop contains no data-dependent branch
// (with a runtime k-group count the compiler keeps the accumulators in VGPRs across the branches and copies all of them to
// and from AGPRs around every group of MFMAs).
// FUSE: the epilogue also reduces norm statistics of what it stores (gn_fuse.h): 1 = moments of the output (forward), 2 = the
// norm-backward partial sums (dgrad). Separate instantiations so that the plain kernels keep their register budget (the extra
// live values cost a wave of occupancy per SIMD in several configurations).
// Waves per SIMD the register allocator must fit (512 registers / waves, accumulators in AGPRs included): several instantiations sit
// one or two VGPRs above a boundary otherwise and lose a wave for it.
// The two-level (TL) form keeps a second accumulator set; of those with 2 tiles per wave only the 2x2-wave layout fits 4 waves.
constexpr int conv_min_waves(int tiles, bool tl, int wn, bool fullj) {
  if (!tl) return tiles <= 2 ? 4 : tiles <= 4 ? 3 : 2;
  return tiles == 1 ? 4 : tiles == 2 ? (wn == 2 ? 4 : fullj ? 3 : 2) : 2;
}

// TA: storage type of x, y, the residual and the normalised tensor of the norm-backward sums (act_io.h: float, or bf16_t / f16_t for the
// HBM-bound forms a network with 16-bit activation storage runs here: 1x1x1, stride 2, zero-insert). The 16-bit forms keep fp32 MFMA
// operands -- the staged values are widened on load -- and round once, on store; statistics are taken over the values as stored.
template <int KD, int STRIDE, int TZ, int TY, int TX, int KC, int PADV, int WM, int WN, int MT, int NT, int INMODE, bool TL = false, bool FULLJ = false, int FUSE = 0,
          typename TA = float>
__global__ __launch_bounds__(256) MIN_WAVES_PER_SIMD(conv_min_waves(MT * NT, TL, WN, FULLJ))
void conv3d_mfma(ConvArgs a) {
  const TA* const ax = reinterpret_cast<const TA*>(a.x);
  TA* const ay = reinterpret_cast<TA*>(a.y);
  const TA* const ares = reinterpret_cast<const TA*>(a.res);
  const TA* const agx = reinterpret_cast<const TA*>(a.g.gx);
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert(TZ * TY * TX == 32 * WM * MT, "tile voxels must equal 32*WM*MT");
  static_assert(KC % 8 == 0, "channel chunk is a multiple of 8");
  static_assert(KD * KD * KD == 1 || (KD * KD * KD) % 3 == 0, "the tap loop is unrolled by three");
  constexpr int HZ = (TZ - 1) * STRIDE + KD, HY = (TY - 1) * STRIDE + KD, HX = (TX - 1) * STRIDE + KD;
  constexpr int HV = HZ * HY * HX;
  constexpr int VS = KC + PADV;
  constexpr int Q = KC / 4;
  constexpr bool ROWSTAGE = KD == 3 && HX * Q <= 256 && (INMODE == MI355_IN_PLAIN || INMODE == MI355_IN_AFFINE_ACT);
  constexpr int J = KC / 8;
  constexpr int T = KD * KD * KD;
  DYN_LDS(lds);

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, li = lane & 31;
  const int wm = wave / WN, wn = wave % WN;
  // Zero-insert mode (dgrad of a stride-2 conv / ConvTranspose3d(k3,s2,p1)): 7 of 8 positions of the up-sampled input are
  // zeros, and WHICH taps see a non-zero depends only on the output voxel's parity per axis: an even coordinate uses tap 1,
  // an odd one taps 0 and 2. With ZIP the 8 M tiles of the 4x8x8 output tile are the 8 parity classes (32 same-parity voxels
  // each), so a tile issues MFMAs for its own 1/2/4/8 taps only instead of all 27 (27/8 taps per voxel on average). A wave
  // owns the two classes that differ in x; the (z, y) class is rotated with the workgroup index because the classes carry
  // 3/6/6/12 taps and would otherwise load the 4 SIMDs unevenly.
  constexpr bool ZIP = INMODE == MI355_IN_ZERO_INSERT && KD == 3 && STRIDE == 1 && TZ == 4 && TY == 8 && TX == 8 && WM == 4 && MT == 2;
  constexpr int ZCZ = TZ / 2 + 1, ZCY = TY / 2 + 1, ZCX = TX / 2 + 1, ZHV = ZCZ * ZCY * ZCX;   // coarse tile of the ZIP form
  const int zcls = ZIP ? ((wm + (int)blockIdx.x) & 3) : 0;     // (az, ay) = (zcls >> 1, zcls & 1)

  int b = blockIdx.x;
  const int cot = b % a.coTiles; b /= a.coTiles;
  const int tx0 = (b % a.tilesX) * TX; b /= a.tilesX;
  const int ty0 = (b % a.tilesY) * TY; b /= a.tilesY;
  const int tz0 = (b % a.tilesZ) * TZ; b /= a.tilesZ;
  const int n = b;
  const int co_base = cot * (32 * WN * NT) + wn * (32 * NT);

  // A fragment base addresses (floats) for this lane's voxel of each M tile.
  int abase[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int tv = (wm * MT + mt) * 32 + li;
    int tz = tv / (TY * TX), ty = (tv / TX) % TY, tx = tv % TX;
    abase[mt] = (((tz * STRIDE) * HY + ty * STRIDE) * HX + tx * STRIDE) * VS + half * 4;
    // ZIP: LDS holds only the COARSE voxels the tile can see (CZ x CY x CX = 3 x 5 x 5 instead of the 6 x 10 x 10 zero-inserted
    // halo, 7/8 of which would be zeros). Lane li of a parity-class tile is output voxel (2*(li>>4)+az, 2*((li>>2)&3)+ay,
    // 2*(li&3)+ax); a tap d it uses reads coarse voxel (li>>4) + (d>>1) along each axis, whatever the class.
    if (ZIP) abase[mt] = ((((li >> 4) * ZCY) + ((li >> 2) & 3)) * ZCX + (li & 3)) * VS + half * 4;
  }

  // Two-level accumulation (TL, selected for Cin >= 4 chunks): the MFMAs of one channel chunk (27*KC products) chain into
  // `accc`, which is folded into `acc` at the end of the chunk. Keeps the sequential fp32 chain at <= 864 terms instead of
  // 27*Cin (6912 at Cin = 256), which brings the roundoff of the deep layers down to that of a blocked CPU convolution.
  // Without TL both names are the same accumulator (single chain).
  f32x16 acc[MT][NT], accc[TL ? MT : 1][TL ? NT : 1];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[mt][nt][r] = 0.f; if (TL) accc[mt][nt][r] = 0.f; }

  const int CQ = a.CinP / 4;
  const float4* wp4 = reinterpret_cast<const float4*>(a.wp);
  const int sq = tid % Q;       // this thread's channel quad inside the chunk (fixed: 256 % Q == 0)
  const int sv0 = tid / Q;

  // B fragments (packed weights [tap][ci/4][co][4]) are addressed as (wave-uniform slab pointer, in SGPRs) + (this lane's fixed 32-bit
  // byte offset inside a slab): no per-lane 64-bit index arithmetic in the tap loop. SQ counters
  // (profiles/r2_sq_counters_conv_kernels.txt) show MFMA-busy % + 4 x VALU-instruction % ~ 94 % of the SIMD cycles in these kernels:
  // vector-ALU instructions are paid in matrix time.
  const unsigned lane_b = (unsigned)(half * a.CoutP + co_base + li) * 16u;
  const size_t tap_slab = (size_t)CQ * a.CoutP;
  auto load_b = [&](float4 (&bf)[J][NT], const float4* slab, int jn_) {      // slab: tap and chunk applied, wave-uniform
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        bf[j][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < jn_)
          bf[j][nt] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(slab + (size_t)(2 * j) * a.CoutP + nt * 32) + lane_b);
      }
  };

  for (int c0 = 0; c0 < a.CinP; c0 += KC) {
    // k-groups of this chunk that exist (CinP is a multiple of 8 but not necessarily of KC); wave-uniform
    const int jn = FULLJ ? J : ((a.CinP - c0) / 8 < J ? (a.CinP - c0) / 8 : J);
    const float4* wpc = wp4 + (size_t)(c0 / 4) * a.CoutP;      // this chunk's channel quads inside every tap slab
    // 3x3x3: the first tap's B fragments are requested before the tile is staged, their latency hides under the staging loads
    // (0.3-0.6 % per layer); the 1x1x1 kernels measured 5-13 % faster asking after the barrier (fewer registers while staging)
    float4 b0[ZIP ? 1 : J][ZIP ? 1 : NT];
    if constexpr (!ZIP && T > 1) load_b(b0, wpc, jn);
    // ---- stage the haloed input tile for channels [c0, c0+KC) ----
    __syncthreads();
    {
      const int c = c0 + 4 * sq;
      const bool cvalid = c < a.Cin;
      float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 sl = make_float4(a.slope, a.slope, a.slope, a.slope);
      if (INMODE == MI355_IN_AFFINE_ACT && cvalid) {
        sc = *reinterpret_cast<const float4*>(a.in_scale + (size_t)n * a.Cin + c);
        sh = *reinterpret_cast<const float4*>(a.in_shift + (size_t)n * a.Cin + c);
        if (a.in_slope) sl = *reinterpret_cast<const float4*>(a.in_slope + c);
      }
      if (INMODE == MI355_IN_S2D) {
        // 1x1x1 over the space-to-depth view of a fine tensor: logical channel c = p*fC + k, p = 4a+2b+e
        const int p = cvalid ? c / a.fC : 0, k = c - p * a.fC;
        const int pa = p >> 2, pb = (p >> 1) & 1, pe = p & 1;
        for (int hv = sv0; hv < HV; hv += 256 / Q) {
          const int v = tx0 + hv;
          float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
          if (cvalid && v < a.Wi) {
            const int xx = v % a.cW, yy = (v / a.cW) % a.cH, zz = v / (a.cW * a.cH);
            const size_t fv = (((size_t)n * (2 * a.cD) + 2 * zz + pa) * (2 * a.cH) + 2 * yy + pb) * (2 * a.cW) + 2 * xx + pe;
            val = ld4(ax + fv * a.xld + k);
          }
          *reinterpret_cast<float4*>(lds + hv * VS + 4 * sq) = val;
        }
      } else if constexpr (ZIP) {
        // coarse voxel (cz, cy, cx) of the tile = input voxel (tz0/2 + cz, ty0/2 + cy, tx0/2 + cx) (tile origins are even, pad is 1)
        constexpr int UP = (ZHV * Q + 255) / 256;
        float4 ld[UP];
#pragma unroll
        for (int k = 0; k < UP; ++k) {
          int hv = sv0 + k * (256 / Q);
          if (hv >= ZHV) hv = ZHV - 1;
          int iz = tz0 / 2 + hv / (ZCY * ZCX), iy = ty0 / 2 + (hv / ZCX) % ZCY, ix = tx0 / 2 + hv % ZCX;
          iz = iz < a.Di ? iz : a.Di - 1; iy = iy < a.Hi ? iy : a.Hi - 1; ix = ix < a.Wi ? ix : a.Wi - 1;
          ld[k] = ld4(ax + ((((size_t)n * a.Di + iz) * a.Hi + iy) * a.Wi + ix) * a.xld + (cvalid ? c : 0));
        }
#pragma unroll
        for (int k = 0; k < UP; ++k) {
          const int hv = sv0 + k * (256 / Q);
          if (hv >= ZHV) continue;
          const int iz = tz0 / 2 + hv / (ZCY * ZCX), iy = ty0 / 2 + (hv / ZCX) % ZCY, ix = tx0 / 2 + hv % ZCX;
          const bool ok = cvalid && iz < a.Di && iy < a.Hi && ix < a.Wi;
          *reinterpret_cast<float4*>(lds + hv * VS + 4 * sq) = ok ? ld[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      } else if constexpr (ROWSTAGE) {
        // Row-structured staging (3x3x3, plain / norm-prologue inputs): a thread owns one (halo x, channel quad) pair and walks the
        // (z, y) rows of the halo, RP rows at a time. Its x coordinate, x clamp / validity and channel offset are per-thread
        // constants, a row costs an add-with-carry for (hz, hy), two clamps and ONE 64-bit multiply-add for the address, and the LDS
        // address is a per-thread base plus a compile-time offset -- ~35 vector-ALU instructions per staged float4 instead of ~60
        // (flat voxel index -> two divisions, three clamps and the voxel index chain, all done twice). SQ counters after the tap-loop
        // work (profiles/r2_sq_counters_conv_kernels_after.txt): staging arithmetic is what is left of the vector-ALU share. Measured:
        // 32->32 @128^3 -1.5...-2 %, the other layers +-0.5 % (profiles/r2_ab_experiments.txt, section 9).
        constexpr int TPR = HX * Q, RP = 256 / TPR, NR = HZ * HY, UP = (NR + RP - 1) / RP, UB = 4;
        const bool tact = tid < RP * TPR;                        // 240 of 256 threads stage (10 x 4 quads x 6 rows)
        const int rt = tact ? tid / TPR : 0, xt = tid % TPR;
        const int hx = xt / Q, q4 = xt % Q;
        const int cr = c0 + 4 * q4;
        const bool crv = cr < a.Cin;
        float4 rsc = make_float4(1.f, 1.f, 1.f, 1.f), rsh = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 rsl = make_float4(a.slope, a.slope, a.slope, a.slope);
        if (INMODE == MI355_IN_AFFINE_ACT && crv) {
          rsc = *reinterpret_cast<const float4*>(a.in_scale + (size_t)n * a.Cin + cr);
          rsh = *reinterpret_cast<const float4*>(a.in_shift + (size_t)n * a.Cin + cr);
          if (a.in_slope) rsl = *reinterpret_cast<const float4*>(a.in_slope + cr);
        }
        const int ix = tx0 * STRIDE - a.pad + hx;
        const bool xok = tact && crv && ix >= 0 && ix < a.Wi;
        const int ixc = ix < 0 ? 0 : (ix < a.Wi ? ix : a.Wi - 1);
        const TA* colp = ax + (size_t)ixc * a.xld + (crv ? cr : 0);      // this thread's column: row offset added per unit
        const unsigned rowpitch = (unsigned)a.Wi * (unsigned)a.xld;           // floats per (z, y) row
        const int hz0 = rt / HY, hy0 = rt % HY;
        float* ldst = lds + ((rt * HX + hx) * VS + 4 * q4);                  // + k * RP * HX * VS per unit: an immediate
#pragma unroll
        for (int k0 = 0; k0 < UP; k0 += UB) {
          float4 ld[UB];
          bool ok[UB];
#pragma unroll
          for (int kk = 0; kk < UB; ++kk) {
            if (k0 + kk >= UP) continue;
            const int k = k0 + kk;
            int hy = hy0 + (k * RP) % HY, hz = hz0 + (k * RP) / HY;
            if (hy >= HY) { hy -= HY; hz += 1; }
            if (hz >= HZ) hz = HZ - 1;                            // the ragged last round re-reads a valid row (not stored)
            const int iz = tz0 * STRIDE - a.pad + hz, iy = ty0 * STRIDE - a.pad + hy;
            const int izc = iz < 0 ? 0 : (iz < a.Di ? iz : a.Di - 1), iyc = iy < 0 ? 0 : (iy < a.Hi ? iy : a.Hi - 1);
            ok[kk] = xok && iz >= 0 && iz < a.Di && iy >= 0 && iy < a.Hi;
            ld[kk] = ld4(colp + (size_t)(unsigned)((n * a.Di + izc) * a.Hi + iyc) * rowpitch);
          }
#pragma unroll
          for (int kk = 0; kk < UB; ++kk) {
            if (k0 + kk >= UP) continue;
            const int k = k0 + kk;
            if ((UP * RP > NR && k == UP - 1 && rt + k * RP >= NR) || !tact) continue;
            float4 v = ld[kk];
            if (INMODE == MI355_IN_AFFINE_ACT) {
              v.x = v.x * rsc.x + rsh.x; v.y = v.y * rsc.y + rsh.y; v.z = v.z * rsc.z + rsh.z; v.w = v.w * rsc.w + rsh.w;
              v.x = fmaxf(v.x, v.x * rsl.x); v.y = fmaxf(v.y, v.y * rsl.y); v.z = fmaxf(v.z, v.z * rsl.z); v.w = fmaxf(v.w, v.w * rsl.w);
            }
            if (!ok[kk]) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(ldst + k * (RP * HX * VS)) = v;
          }
        }
      } else {
        // Batches of UB staging units: all loads of a batch are issued from clamped, always-valid addresses before the first
        // use (no branch around a load, so they are in flight together instead of one dependent round trip each), then
        // masked / normalised and written to LDS.
        constexpr int UP = (HV * Q + 255) / 256, UB = 4;
#pragma unroll
        for (int k0 = 0; k0 < UP; k0 += UB) {
          float4 ld[UB];
#pragma unroll
          for (int kk = 0; kk < UB; ++kk) {
            if (k0 + kk >= UP) continue;
            int hv = sv0 + (k0 + kk) * (256 / Q);
            if (hv >= HV) hv = HV - 1;
            const int hz = hv / (HY * HX), hy = (hv / HX) % HY, hx = hv % HX;
            int iz = tz0 * STRIDE - a.pad + hz, iy = ty0 * STRIDE - a.pad + hy, ix = tx0 * STRIDE - a.pad + hx;
            if (INMODE == MI355_IN_ZERO_INSERT) { iz >>= 1; iy >>= 1; ix >>= 1; }
            iz = iz < 0 ? 0 : (iz < a.Di ? iz : a.Di - 1);
            iy = iy < 0 ? 0 : (iy < a.Hi ? iy : a.Hi - 1);
            ix = ix < 0 ? 0 : (ix < a.Wi ? ix : a.Wi - 1);
            ld[kk] = ld4(ax + ((((size_t)n * a.Di + iz) * a.Hi + iy) * a.Wi + ix) * a.xld + (cvalid ? c : 0));
          }
#pragma unroll
          for (int kk = 0; kk < UB; ++kk) {
            if (k0 + kk >= UP) continue;
            const int hv = sv0 + (k0 + kk) * (256 / Q);
            if (hv >= HV) continue;
            const int hz = hv / (HY * HX), hy = (hv / HX) % HY, hx = hv % HX;
            int iz = tz0 * STRIDE - a.pad + hz, iy = ty0 * STRIDE - a.pad + hy, ix = tx0 * STRIDE - a.pad + hx;
            bool ok = cvalid;
            if (INMODE == MI355_IN_ZERO_INSERT) {
              ok = ok && iz >= 0 && iy >= 0 && ix >= 0 && ((iz | iy | ix) & 1) == 0;
              iz >>= 1; iy >>= 1; ix >>= 1;
              ok = ok && iz < a.Di && iy < a.Hi && ix < a.Wi;
            } else {
              ok = ok && iz >= 0 && iy >= 0 && ix >= 0 && iz < a.Di && iy < a.Hi && ix < a.Wi;
            }
            float4 v = ld[kk];
            if (INMODE == MI355_IN_AFFINE_ACT) {
              v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
              // act(u) = max(u, slope * u) for 0 <= slope <= 1 (ReLU, LeakyReLU, identity): no compare / select
              v.x = fmaxf(v.x, v.x * sl.x); v.y = fmaxf(v.y, v.y * sl.y); v.z = fmaxf(v.z, v.z * sl.z); v.w = fmaxf(v.w, v.w * sl.w);
            }
            if (!ok) v = make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(lds + hv * VS + 4 * sq) = v;
          }
        }
      }
    }
    __syncthreads();

    // ---- 27 taps x KC/8 k-groups, B fragments prefetched one tap ahead ----
    if constexpr (!ZIP && T == 1) load_b(b0, wpc, jn);
    if constexpr (ZIP) {
      const int az = zcls >> 1, ay = zcls & 1;
      const int ny = ay ? 2 : 1, ncomb = (az ? 2 : 1) * ny;
#pragma unroll 1
      for (int cb = 0; cb < ncomb; ++cb) {
        const int dz = az ? 2 * (cb / ny) : 1, dy = ay ? 2 * (cb % ny) : 1;
        float4 b3[3][J][NT];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int j = 0; j < J; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              b3[dx][j][nt] = make_float4(0.f, 0.f, 0.f, 0.f);
              if (j < jn) b3[dx][j][nt] = wp4[((size_t)(((dz * 3 + dy) * 3 + dx) * CQ + c0 / 4 + half + 2 * j)) * a.CoutP + co_base + nt * 32 + li];
            }
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int mt = (dx & 1) ? 0 : 1;          // even x (class ax = 0 = M tile 0) uses tap 1, odd x taps 0 and 2
          const int toff = (((dz >> 1) * ZCY + (dy >> 1)) * ZCX + (dx >> 1)) * VS;
#pragma unroll
          for (int j = 0; j < J; ++j) {
            if (j >= jn) continue;
            const float4 af = *reinterpret_cast<const float4*>(lds + abase[mt] + toff + j * 8);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              f32x16& ac = TL ? accc[TL ? mt : 0][TL ? nt : 0] : acc[mt][nt];
              ac = MFMA_32x32x2(af.x, b3[dx][j][nt].x, ac);
              ac = MFMA_32x32x2(af.y, b3[dx][j][nt].y, ac);
              ac = MFMA_32x32x2(af.z, b3[dx][j][nt].z, ac);
              ac = MFMA_32x32x2(af.w, b3[dx][j][nt].w, ac);
            }
          }
        }
      }
    } else {
      auto run_tap = [&](const float4 (&bf)[J][NT], int tap) {
        const int dz = tap / (KD * KD), dy = (tap / KD) % KD, dx = tap % KD;      // wave-uniform: scalar ALU
        const int toff = ((dz * HY + dy) * HX + dx) * VS;
#pragma unroll
        for (int j = 0; j < J; ++j) {
          if (j >= jn) continue;
          float4 af[MT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const float4*>(lds + abase[mt] + toff + j * 8);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
              f32x16& ac = TL ? accc[TL ? mt : 0][TL ? nt : 0] : acc[mt][nt];
              ac = MFMA_32x32x2(af[mt].x, bf[j][nt].x, ac);
              ac = MFMA_32x32x2(af[mt].y, bf[j][nt].y, ac);
              ac = MFMA_32x32x2(af[mt].z, bf[j][nt].z, ac);
              ac = MFMA_32x32x2(af[mt].w, bf[j][nt].w, ac);
            }
        }
      };
      // B fragments run one tap ahead of the MFMAs that use them. Two forms, chosen per tile shape by measurement
      // (tools/bench_conv_layers.py, profiles/r2_ab_experiments.txt):
      //  * three register sets rotating through an unroll-by-three body (27 = 9 x 3; a peeled odd tap made the compiler keep a
      //    second copy of every accumulator): no "current = next" moves -- 4-6 % faster where a wave holds up to two tiles;
      //  * two sets with the move: what the 4-tile (2 x 2) waves and the 2 x 2-wave layout prefer (the third set costs them the
      //    registers their A fragments were read ahead in).
      constexpr bool ROT3 = !(MT * NT == 4 || (WM == 2 && WN == 2 && MT * NT == 2));
      if constexpr (T == 1) {
        run_tap(b0, 0);
      } else if constexpr (ROT3) {
        float4 b1[J][NT], b2[J][NT];
#pragma unroll 1
        for (int tap = 0; tap < T; tap += 3) {
          load_b(b1, wpc + tap_slab * (tap + 1), jn);
          SCHED_BARRIER();      // the B loads of the NEXT tap stay above this tap's MFMAs (the scheduler otherwise sinks them to their use)
          run_tap(b0, tap);
          load_b(b2, wpc + tap_slab * (tap + 2), jn);
          SCHED_BARRIER();
          run_tap(b1, tap + 1);
          if (tap + 3 < T) load_b(b0, wpc + tap_slab * (tap + 3), jn);      // wave-uniform branch
          SCHED_BARRIER();
          run_tap(b2, tap + 2);
        }
      } else {
        float4 b1[J][NT];
#pragma unroll 1
        for (int tap = 0; tap < T; ++tap) {
          load_b(b1, wpc + tap_slab * (tap + 1 < T ? tap + 1 : tap), jn);
          SCHED_BARRIER();
          run_tap(b0, tap);
#pragma unroll
          for (int j = 0; j < J; ++j)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) b0[j][nt] = b1[j][nt];
        }
      }
    }
    if (TL) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int r = 0; r < 16; ++r) { acc[mt][nt][r] += accc[TL ? mt : 0][TL ? nt : 0][r]; accc[TL ? mt : 0][TL ? nt : 0][r] = 0.f; }
    }
  }

  // ---- epilogue, interior tiles (everything but the ragged edge of a layer): accumulator register r of M tile m is voxel
  // tv = 32 m + (r & 3) + 8 (r >> 2) + 4 half of the tile, i.e. x = 4 half + (r & 3) and 8-voxel row 4 m + (r >> 2): one base
  // pointer per lane and tile plus wave-uniform offsets. The general path below spends ~30 vector-ALU instructions per stored
  // value on the lane map, the bound checks and two 64-bit voxel indices. ----
  // (not for the 4-tile waves with the norm-backward sums: both paths in one kernel spill there; same speed either way)
  if constexpr (!ZIP && ((TX == 8 && TY % 4 == 0) || (KD == 1 && TX == 256 && TY == 1 && TZ == 1)) && !(FUSE == 2 && MT * NT >= 4)) {
    const bool interior = tz0 + TZ <= a.Do && ty0 + TY <= a.Ho && tx0 + TX <= a.Wo && a.offz == 0 && a.offy == 0 && a.offx == 0 &&
                          a.yD == a.Do && a.yH == a.Ho && a.yW == a.Wo && !(KD == 1 && a.outmode == MI355_OUT_D2S);      // workgroup-uniform
    if (interior) {
      constexpr int K = FUSE == 1 ? 3 : 2;
      float vals[NT][K];
      const size_t rowstep = TX == 8 ? (size_t)a.Wo : 8;      // voxels between accumulator rows r and r + 4 (1x1x1 tiles are flat)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int co = co_base + nt * 32 + li;
        const bool cov = co < a.Cout;
        const int coc = cov ? co : a.Cout - 1;
        float bs = 0.f, cs = 1.f;
        if (a.bias) bs = a.bias[coc];
        if (a.out_chscale) cs = a.out_chscale[(size_t)n * a.Cout + coc];
        float K0 = 0.f, s0 = 0.f, s1 = 0.f, gsc = 1.f, gsh = 0.f, gmean = 0.f, grstd = 1.f;
        if constexpr (FUSE == 2) {
          const int grp = coc / (a.Cout / a.g.ggroups);
          gsc = a.g.gscale[(size_t)n * a.Cout + coc]; gsh = a.g.gshift[(size_t)n * a.Cout + coc];
          gmean = a.g.gmr[((size_t)n * a.g.ggroups + grp) * 2]; grstd = a.g.gmr[((size_t)n * a.g.ggroups + grp) * 2 + 1];
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int tv0 = (wm * MT + mt) * 32 + 4 * half;      // this lane's voxel for r = 0
          const size_t v0 = (((size_t)n * a.Do + tz0 + tv0 / (TY * TX)) * a.Ho + ty0 + (tv0 / TX) % TY) * a.Wo + tx0 + tv0 % TX;
          TA* yp = ay + v0 * a.yld + coc;
          const TA* rp = a.res ? ares + v0 * a.resld + coc : nullptr;
          // FUSE 2: the 16 reads of the normalised tensor of this tile go out ahead of their use
          constexpr int GB = 16;
          const TA* gp = FUSE == 2 ? agx + v0 * a.g.gxld + coc : nullptr;
#pragma unroll
          for (int r0 = 0; r0 < 16; r0 += GB) {
            float gxv[GB];
            if constexpr (FUSE == 2) {
#pragma unroll
              for (int r = r0; r < r0 + GB; ++r) gxv[r - r0] = ld1(gp + ((size_t)(r >> 2) * rowstep + (r & 3)) * a.g.gxld);
            }
#pragma unroll
            for (int r = r0; r < r0 + GB; ++r) {
              const size_t eo = (size_t)(r >> 2) * rowstep + (r & 3);      // wave-uniform
              float v = acc[mt][nt][r] + bs;
              if (a.res) v += ld1(rp + eo * a.resld);
              v *= cs;
              if (cov) st1(yp + eo * a.yld, v);
              if constexpr (FUSE != 0) v = as_stored(yp, v);
              if constexpr (FUSE == 1) {
                if (mt == 0 && r == 0) K0 = v;
                const float t = v - K0;
                s0 += t; s1 += t * t;
              } else if constexpr (FUSE == 2) {
                const float xv = gxv[r - r0];
                const float u = xv * gsc + gsh;
                const float du = u > 0.f ? v : v * a.g.gslope;
                s0 += du; s1 += du * ((xv - gmean) * grstd);
              }
            }
          }
        }
        if constexpr (FUSE == 1) {
          const float c = cov ? (float)(MT * 16) : 0.f;
          const float m2 = s1 - s0 * s0 / (float)(MT * 16);
          vals[nt][0] = c; vals[nt][1] = cov ? s0 + c * K0 : 0.f; vals[nt][2] = (cov && m2 > 0.f) ? m2 : 0.f;
        } else if constexpr (FUSE == 2) {
          vals[nt][0] = cov ? s0 : 0.f; vals[nt][1] = cov ? s1 : 0.f;
        }
      }
      if constexpr (FUSE != 0) {
        const int tile = ((tz0 / TZ) * a.tilesY + ty0 / TY) * a.tilesX + tx0 / TX;
        const size_t rec = (size_t)n * ((size_t)a.tilesZ * a.tilesY * a.tilesX) + tile;
        float* dst = (FUSE == 1 ? a.g.mom : a.g.gnb) + rec * a.Cout * K;
        gn_fuse_reduce_store<K, NT, WM, WN>(vals, lds, wm, wn, half, li, tid, dst, cot * (32 * WN * NT), a.Cout);
      }
      return;
    }
  }

  // ---- epilogue: bias, residual, dropout scale, windowed store ----
  if constexpr (FUSE == 0) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
        const int tv = (wm * MT + mt) * 32 + row;
        int oz = tz0 + tv / (TY * TX), oy = ty0 + (tv / TX) % TY, ox = tx0 + tv % TX;
        if (ZIP) { oz = tz0 + 2 * (row >> 4) + (zcls >> 1); oy = ty0 + 2 * ((row >> 2) & 3) + (zcls & 1); ox = tx0 + 2 * (row & 3) + mt; }
        if (oz >= a.Do || oy >= a.Ho || ox >= a.Wo) continue;
        if (KD == 1 && a.outmode == MI355_OUT_D2S) {
          // ConvTranspose3d(k2,s2): logical channel p*fC + k of coarse voxel ox (flat) -> fine voxel (2z+a, 2y+b, 2x+e), channel k
          const int xx = ox % a.cW, yy = (ox / a.cW) % a.cH, zz = ox / (a.cW * a.cH);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const int co = co_base + nt * 32 + li;
            if (co >= a.Cout) continue;
            const int p = co / a.fC, k = co - p * a.fC;
            const size_t fv = (((size_t)n * (2 * a.cD) + 2 * zz + (p >> 2)) * (2 * a.cH) + 2 * yy + ((p >> 1) & 1)) * (2 * a.cW) + 2 * xx + (p & 1);
            float v = acc[mt][nt][r];
            if (a.bias) v += a.bias[k];
            st1(ay + fv * a.yld + k, v);
          }
          continue;
        }
        const int sz = oz + a.offz, sy = oy + a.offy, sx = ox + a.offx;
        if (sz < 0 || sy < 0 || sx < 0 || sz >= a.yD || sy >= a.yH || sx >= a.yW) continue;
        const size_t ovox = (((size_t)n * a.Do + oz) * a.Ho + oy) * a.Wo + ox;
        const size_t svox = (((size_t)n * a.yD + sz) * a.yH + sy) * a.yW + sx;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int co = co_base + nt * 32 + li;
          if (co >= a.Cout) continue;
          float v = acc[mt][nt][r];
          if (a.bias) v += a.bias[co];
          if (a.res) v += ld1(ares + ovox * a.resld + co);
          if (a.out_chscale) v *= a.out_chscale[(size_t)n * a.Cout + co];
          st1(ay + svox * a.yld + co, v);
        }
      }
    }
  } else {
    // ---- the same epilogue + norm statistics of what it stores (gn_fuse.h). The host only selects these instantiations for
    // un-windowed plain outputs (stats_fusable), so the stored voxel IS the logical one. One N tile at a time: the running sums of a
    // single channel column are live, not NT of them (the 4-tile configurations sit at their register limit).
    constexpr int K = FUSE == 1 ? 3 : 2;
    float vals[NT][K];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = co_base + nt * 32 + li;
      const bool cov = co < a.Cout;
      const int coc = cov ? co : a.Cout - 1;
      float bs = 0.f, cs = 1.f;
      if (a.bias) bs = a.bias[coc];
      if (a.out_chscale) cs = a.out_chscale[(size_t)n * a.Cout + coc];
      // FUSE 1: one-pass moments about K0 = the lane's first stored value of this channel (a sample of the data: no cancellation)
      // FUSE 2: sum du, sum du * xhat with du = dA * act'(scale * gx + shift), xhat = (gx - mean) * rstd
      float K0 = 0.f, s0 = 0.f, s1 = 0.f, gsc = 1.f, gsh = 0.f, gmean = 0.f, grstd = 1.f;
      int cnt = 0;
      if constexpr (FUSE == 2) {
        const int grp = coc / (a.Cout / a.g.ggroups);
        gsc = a.g.gscale[(size_t)n * a.Cout + coc]; gsh = a.g.gshift[(size_t)n * a.Cout + coc];
        gmean = a.g.gmr[((size_t)n * a.g.ggroups + grp) * 2]; grstd = a.g.gmr[((size_t)n * a.g.ggroups + grp) * 2 + 1];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        // FUSE 2: the 16 reads of the normalised tensor of this tile are issued first, from clamped (always valid) addresses --
        // inside the loop below every one of them was a dependent round trip behind the stores (0.2-0.4 ms per 128^3 launch)
        float gxv[16];
        if constexpr (FUSE == 2) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int tv = (wm * MT + mt) * 32 + row;
            int oz = tz0 + tv / (TY * TX), oy = ty0 + (tv / TX) % TY, ox = tx0 + tv % TX;
            oz = oz < a.Do ? oz : a.Do - 1; oy = oy < a.Ho ? oy : a.Ho - 1; ox = ox < a.Wo ? ox : a.Wo - 1;
            gxv[r] = ld1(agx + ((((size_t)n * a.Do + oz) * a.Ho + oy) * a.Wo + ox) * a.g.gxld + coc);
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * half;
          const int tv = (wm * MT + mt) * 32 + row;
          const int oz = tz0 + tv / (TY * TX), oy = ty0 + (tv / TX) % TY, ox = tx0 + tv % TX;
          if (oz >= a.Do || oy >= a.Ho || ox >= a.Wo || !cov) continue;
          const size_t ovox = (((size_t)n * a.Do + oz) * a.Ho + oy) * a.Wo + ox;
          float v = acc[mt][nt][r] + bs;
          if (a.res) v += ld1(ares + ovox * a.resld + co);
          v *= cs;
          st1(ay + ovox * a.yld + co, v);
          v = as_stored(ay, v);
          if constexpr (FUSE == 1) {
            if (cnt == 0) K0 = v;
            const float t = v - K0;
            s0 += t; s1 += t * t;
          } else {
            const float xv = gxv[r];
            const float u = xv * gsc + gsh;
            const float du = u > 0.f ? v : v * a.g.gslope;
            s0 += du; s1 += du * ((xv - gmean) * grstd);
          }
          ++cnt;
        }
      }
      if constexpr (FUSE == 1) {
        const float c = (float)cnt;
        const float m2 = cnt > 0 ? s1 - s0 * s0 / c : 0.f;
        vals[nt][0] = c; vals[nt][1] = s0 + c * K0; vals[nt][2] = m2 > 0.f ? m2 : 0.f;
      } else {
        vals[nt][0] = s0; vals[nt][1] = s1;
      }
    }
    const int tile = ((tz0 / TZ) * a.tilesY + ty0 / TY) * a.tilesX + tx0 / TX;
    const size_t rec = (size_t)n * ((size_t)a.tilesZ * a.tilesY * a.tilesX) + tile;
    float* dst = (FUSE == 1 ? a.g.mom : a.g.gnb) + rec * a.Cout * K;
    gn_fuse_reduce_store<K, NT, WM, WN>(vals, lds, wm, wn, half, li, tid, dst, cot * (32 * WN * NT), a.Cout);
  }
}

// ---- weight packing ---------------------------------------------------------------------------
// mode 0: w OIDHW [cout][cin][T]              -> wp[t][ciP/4][coP][4]           (forward)
// mode 1: same w, dgrad pack: roles swapped: "out" = ci, "in" = co, tap flipped  (dgrad of Conv3d)
// mode 2: ConvTranspose3d weight IODHW [cin][cout][T], forward = correlation of the zero-inserted input with
//         flipped taps: wp[t'][ci][co] = w[ci][co][flip(t')]
// mode 3: ConvTranspose3d dgrad = plain stride-2 correlation of dy: "in" = co, "out" = ci, taps not flipped.
__global__ void pack_weight_kernel(const float* w, float* wp, int cout, int cin, int T, int coutP, int cinP, int mode) {
  // logical packed dims: O (out), I (in); the element definition is pack_values.h: pack_f32_value
  const size_t total = (size_t)T * (cinP / 4) * coutP * 4;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x)
    wp[idx] = pack_f32_value(w, idx, cout, cin, T, coutP, cinP, mode);
}

// Every pack of a training step in ONE launch. The tasks differ by three orders of magnitude (a 4 -> 32 first layer against a
// 256 -> 256 Winograd pack of 3.1 M elements), so the grid is cut into equal CHUNKS of MI355_PACK_CHUNK work items: workgroup b
// finds its task by bisection over the cumulative `first_chunk` column (a grid of (blocks per task) x tasks, the first version, left
// the large tasks to too few workgroups: 0.92 ms for 0.55 GB of traffic).
__global__ __launch_bounds__(256) void pack_batch_kernel(const mi355_pack_task* tasks, int ntasks) {
  int lo = 0, hi = ntasks - 1;
  const int chunk = blockIdx.x;
  while (lo < hi) {                                          // last task whose first_chunk <= chunk (workgroup-uniform)
    const int mid = (lo + hi + 1) >> 1;
    if (tasks[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  const mi355_pack_task t = tasks[lo];
  const bool lp = t.kind >= MI355_PACK_LP;                  // 16-bit operand pack of precision t.kind - MI355_PACK_LP
  const int coutP = (t.cout + 31) / 32 * 32, cinP = lp ? (t.cin + 15) / 16 * 16 : (t.kind == MI355_PACK_WINO3 ? (t.cin + 3) / 4 * 4 : (t.cin + 7) / 8 * 8);
  const int T = t.kd * t.kd * t.kd;
  // work items: an fp32 / 16-bit pack element, or one (dz, ci, co) of a Winograd pack (16 outputs from 9 weights, pack_values.h)
  // ... or one (ci, co) of a 3-D Winograd pack (64 outputs from 27 weights)
  const size_t items = t.kind == MI355_PACK_WINO ? (size_t)3 * cinP * coutP : (t.kind == MI355_PACK_WINO3 ? (size_t)cinP * coutP : (size_t)T * cinP * coutP);
  const size_t base = (size_t)(chunk - t.first_chunk) * MI355_PACK_CHUNK;
  const int prec = t.kind - MI355_PACK_LP;
  const int ns = prec == MI355_PREC_BF16X3 ? 2 : (prec == MI355_PREC_BF16X6 ? 3 : 1);
#pragma unroll 2
  for (int k = 0; k < MI355_PACK_CHUNK / 256; ++k) {
    const size_t idx = base + (size_t)k * 256 + threadIdx.x;
    if (idx >= items) break;
    if (lp) pack_lp_item(t.w, reinterpret_cast<unsigned short*>(t.out), idx, t.cout, t.cin, T, coutP, cinP, t.mode, ns, prec == MI355_PREC_F16);
    else if (t.kind == MI355_PACK_WINO) pack_wino_item(t.w, t.out, idx, t.cout, t.cin, coutP, cinP, t.mode);
    else if (t.kind == MI355_PACK_WINO3) pack_wino3_item(t.w, t.out, idx, t.cout, t.cin, coutP, cinP, t.mode);
    else t.out[idx] = pack_f32_value(t.w, idx, t.cout, t.cin, T, coutP, cinP, t.mode);
  }
}

// tasks: DEVICE array of ntasks records with `first_chunk` filled in (cumulative ceil(work items / MI355_PACK_CHUNK) of the tasks before);
// total_chunks: the sum over all tasks. The caller builds the table once: the pointers of a training loop do not change from step to step.
extern "C" int mi355_pack_weights_batch(const mi355_pack_task* tasks, int32_t ntasks, int32_t total_chunks, void* stream) {
  if (!tasks || ntasks <= 0 || ntasks > 65535 || total_chunks <= 0) return MI355_EINVAL;
  LAUNCH(pack_batch_kernel, dim3((unsigned)total_chunks), dim3(256), 0, stream, tasks, (int)ntasks);
  return LAUNCH_CHECK();
}

extern "C" size_t mi355_packed_weight_elems(int32_t cout, int32_t cin, int32_t kd, int32_t mode) {
  (void)mode;
  const int coutP = pad32(cout), cinP = pad8(cin);
  return (size_t)kd * kd * kd * cinP * coutP;
}

// cout/cin are the PACKED roles (for dgrad packs pass cout := original cin, cin := original cout).
extern "C" int mi355_pack_conv_weight(const float* w, float* wp, int32_t cout, int32_t cin, int32_t kd, int32_t mode, void* stream) {
  if (!w || !wp || cout <= 0 || cin <= 0 || (kd != 1 && kd != 3) || mode < 0 || mode > 3) return MI355_EINVAL;
  const int coutP = pad32(cout), cinP = pad8(cin);
  const int T = kd * kd * kd;
  const size_t total = (size_t)T * cinP * coutP;
  LAUNCH(pack_weight_kernel, dim3(pack_grid(total)), dim3(256), 0, stream, w, wp, cout, cin, T, coutP, cinP, mode);
  return LAUNCH_CHECK();
}

// ---- dispatch ---------------------------------------------------------------------------------
// Configuration table of the generic kernel conv3d_mfma (ids are stable; select_cfg picks one, mi355_conv3d_fwd launches the
// instantiation of the same row, mi355_conv3d_fwd_config prints its template arguments):
//  0/1: 1x1x1, 256-voxel flat tiles, 64/32 output channels per workgroup
//  2/3: 3x3x3 stride 2 (also the zero-insert form with stride template 1), 4x4x8 tiles, KC=8
//  4/5: 3x3x3 stride 1, 4x8x8 tiles, KC=16 (large volumes: >= 131072 output voxels in the batch)
//  6/7: 3x3x3 stride 1, 2x4x8 / 4x4x8 tiles, KC=32 (small volumes, so the grid still covers 256 CUs)
//  8:   3x3x3 stride 1, 4x4x8 tiles x 64 output channels, KC=16, 2 M tiles per wave (32768 .. 131071 output voxels, > 32 output
//       channels: each B fragment feeds two MFMA tiles; +10 % over configuration 6 on the 32^3-level layers)
struct MfmaCfg { int kc, tiles, tz, ty, tx; const char* args; };      // tiles = MT * NT; args = TZ .. NT as the trace prints them
static const MfmaCfg kMfmaCfg[9] = {
    {32, 4, 1, 1, 256, "1, 1, 256, 32, 4, 4, 1, 2, 2"}, {32, 2, 1, 1, 256, "1, 1, 256, 32, 4, 4, 1, 2, 1"},
    {8, 2, 4, 4, 8, "4, 4, 8, 8, 0, 4, 1, 1, 2"},      {8, 1, 4, 4, 8, "4, 4, 8, 8, 0, 4, 1, 1, 1"},
    {16, 4, 4, 8, 8, "4, 8, 8, 16, 4, 4, 1, 2, 2"},    {16, 2, 4, 8, 8, "4, 8, 8, 16, 4, 4, 1, 2, 1"},
    {32, 1, 2, 4, 8, "2, 4, 8, 32, 4, 2, 2, 1, 1"},    {32, 1, 4, 4, 8, "4, 4, 8, 32, 4, 4, 1, 1, 1"},
    {16, 2, 4, 4, 8, "4, 4, 8, 16, 4, 2, 2, 2, 1"}};
static int select_cfg(int kd, int stride, long long vox, int cout, int in_mode) {
  if (kd == 1) return cout > 32 ? 0 : 1;
  if (stride == 2) return cout > 32 ? 2 : 3;
  if (vox >= 256LL * 512 || in_mode == MI355_IN_ZERO_INSERT) return cout > 32 ? 4 : 5;   // zero-insert: parity-class tiles need 4x8x8
  if (cout > 32 && vox >= 64LL * 512) return 8;
  return cout > 32 ? 6 : 7;
}

// can this call fuse norm statistics into its epilogue? (plain, un-windowed output: what is stored IS the logical tensor)
static bool stats_fusable(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d) {
  if (!x || !y || !d || d->out_mode != MI355_OUT_PLAIN || d->in_mode == MI355_IN_S2D) return false;
  if (d->off_z || d->off_y || d->off_x || d->out_d != y->d || d->out_h != y->h || d->out_w != y->w) return false;
  if ((d->kd != 1 && d->kd != 3) || (d->stride != 1 && d->stride != 2)) return false;
  return true;
}

extern "C" int mi355_conv3d_uses_bf16(const mi355_conv_desc* d) {
  return d && d->precision != MI355_PREC_F32 && d->kd == 3 && d->stride == 1 &&
         (d->in_mode == MI355_IN_PLAIN || d->in_mode == MI355_IN_AFFINE_ACT);
}

// ---- routing: one plan per call -------------------------------------------------------------------
// mi355_conv3d_fwd launches the route, mi355_conv3d_stats_blocks and mi355_conv3d_fwd_config read it: the three cannot disagree.
enum FwdRoute { FWD_REFUSED, FWD_C4, FWD_NARROW, FWD_LP16, FWD_S2C32, FWD_S2C32_DGRAD, FWD_K1_STREAM, FWD_MFMA };
// rc: the status of a refused call; cfg, tl, fullj (FWD_MFMA): row of kMfmaCfg, two-level accumulation, whole channel chunks; fuse: 1 moments
// epilogue, 2 norm-backward sums; stats_blocks: epilogue records per sample (0: this call cannot fuse statistics)
struct FwdPlan { FwdRoute route; int rc, cfg; bool tl, fullj; int fuse; int32_t stats_blocks; };

static FwdPlan plan_fwd(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d) {
  FwdPlan p; memset(&p, 0, sizeof(p));
  p.rc = MI355_EUNSUPPORTED;
  if (!x || !y || !d) { p.rc = MI355_EINVAL; return p; }
  p.fuse = d->moments_out ? 1 : (d->gn_bwd ? 2 : 0);
  const bool fusable = stats_fusable(x, y, d);
  long long b = 0;
  if (d->wformat == MI355_W_OIDHW4) {
    p.route = FWD_C4;
    if (fusable && mi355_conv3d_c4_ok(x, d)) b = (long long)ceil_div(y->d, 4) * ceil_div(y->h, 8) * ceil_div(y->w, 8);
  } else if (d->wformat == MI355_W_PACKED_F32_NARROW || (d->wformat == MI355_W_PACKED && d->precision == MI355_PREC_F32 && mi355_conv3d_narrow_ok(x, y, d))) {
    p.route = FWD_NARROW;
  } else if (d->wformat != MI355_W_PACKED) {
    p.rc = MI355_EINVAL;
  } else if (mi355_conv3d_uses_bf16(d)) {
    p.route = FWD_LP16;
    if (fusable) p.stats_blocks = mi355_conv3d_bf16_stats_blocks(x, y, d);
  } else if (d->in_mode == MI355_IN_ZERO_INSERT && (d->stride != 1 || d->kd != 3 || d->pad != 1)) {
    p.rc = MI355_EINVAL;
  } else if (mi355_conv3d_s2c32_ok(x, y, d)) {
    p.route = FWD_S2C32;
    if (fusable) p.stats_blocks = mi355_conv3d_s2c32_stats_blocks(y);
  } else if (mi355_conv3d_s2c32_dgrad_ok(x, y, d)) {
    p.route = FWD_S2C32_DGRAD;
  } else if (mi355_conv3d_k1_stream_ok(x, y, d)) {
    p.route = FWD_K1_STREAM;
  } else if (x->dtype == y->dtype) {      // one storage type per call here (the first-layer kernels above take fp32 x with either y)
    p.route = FWD_MFMA;
    p.cfg = select_cfg(d->kd, d->stride, (long long)d->out_d * d->out_h * d->out_w * x->n,
                       (d->kd == 1 && d->out_mode == MI355_OUT_D2S) ? 8 * y->c : y->c, d->in_mode);
    const MfmaCfg& c = kMfmaCfg[p.cfg];
    // two-level accumulation: always for >= 4 channel chunks; for the 1-tile-per-wave configurations (16 accumulator
    // registers, deep layers) already from 2 chunks, where it is free
    // (not for the 4-tile configuration: 64 more live registers would cost a wave of occupancy per SIMD)
    const int cinP = pad8(x->c), cinL = d->in_mode == MI355_IN_S2D ? 8 * x->c : x->c;
    p.tl = d->kd == 3 && c.tiles <= 2 && (cinP >= 4 * c.kc || (c.tiles == 1 && cinP >= 2 * c.kc));
    p.fullj = pad8(cinL) % c.kc == 0;
    // only the 3x3x3 kernels reading a plain / normalised input carry the fused-statistics epilogue
    if (fusable && d->kd == 3 && (d->in_mode == MI355_IN_PLAIN || d->in_mode == MI355_IN_AFFINE_ACT))
      b = (long long)ceil_div(y->d, c.tz) * ceil_div(y->h, c.ty) * ceil_div(y->w, c.tx);
  }
  if (grid_fits(b)) p.stats_blocks = (int32_t)b;
  return p;
}

// the forms that exist for 16-bit activation storage: what a UNet3D or a DynUNet with 16-bit activation storage sends here (their 3x3x3
// stride-1 convolutions run on the 16-bit-operand kernels of conv3d_bf16*.hip): 1x1x1 on a plain, normalised or space-to-depth input
// (DynUNet's ConvTranspose3d(k2, s2) and its data gradient), 3x3x3 stride 2 on a plain or normalised input (with or without the moments
// epilogue), and the zero-insert form (stride-2 dgrad, ConvTranspose3d(k3, s2))
template <typename TA> constexpr bool act_form_exists(int kd, int stride, int im, int fuse) {
  return std::is_same<TA, float>::value || (kd == 1 && im != MI355_IN_ZERO_INSERT && fuse == 0) ||
         (kd == 3 && stride == 2 && (im == MI355_IN_PLAIN || im == MI355_IN_AFFINE_ACT) && fuse <= 1) ||
         (kd == 3 && im == MI355_IN_ZERO_INSERT && fuse == 0);
}

template <int KD, int STRIDE, int TZ, int TY, int TX, int KC, int PADV, int WM, int WN, int MT, int NT, typename TA = float>
static int launch_cfg(ConvArgs& a, int in_mode, const FwdPlan& p, void* stream) {
  constexpr int HZ = (TZ - 1) * STRIDE + KD, HY = (TY - 1) * STRIDE + KD, HX = (TX - 1) * STRIDE + KD;
  constexpr size_t lds = (size_t)HZ * HY * HX * (KC + PADV) * sizeof(float);
  static_assert(lds <= 64 * 1024, "LDS tile must fit the default 64 KiB dynamic window");
  a.tilesZ = ceil_div(a.Do, TZ); a.tilesY = ceil_div(a.Ho, TY); a.tilesX = ceil_div(a.Wo, TX);
  a.coTiles = ceil_div(a.Cout, 32 * WN * NT);
  const long long blocks = (long long)a.N * a.tilesZ * a.tilesY * a.tilesX * a.coTiles;
  if (!grid_fits(blocks)) return MI355_EINVAL;
  const bool tl = p.tl, fullj = p.fullj;
  const int fuse = p.fuse;
  if (fuse && (KD != 3 || (in_mode != MI355_IN_PLAIN && in_mode != MI355_IN_AFFINE_ACT))) return MI355_EUNSUPPORTED;
#define MI355_LAUNCH_CONV4(SS, IM, LDSB, FU)                                                                                         \
  do {                                                                                                                         \
    if constexpr (!act_form_exists<TA>(KD, STRIDE, IM, FU)) return MI355_EUNSUPPORTED;                                          \
    else if (tl && fullj) LAUNCH((conv3d_mfma<KD, SS, TZ, TY, TX, KC, PADV, WM, WN, MT, NT, IM, KD == 3, true, FU, TA>), dim3((unsigned)blocks), dim3(256), (LDSB), stream, a);  \
    else if (tl) LAUNCH((conv3d_mfma<KD, SS, TZ, TY, TX, KC, PADV, WM, WN, MT, NT, IM, KD == 3, false, FU, TA>), dim3((unsigned)blocks), dim3(256), (LDSB), stream, a);      \
    else if (fullj) LAUNCH((conv3d_mfma<KD, SS, TZ, TY, TX, KC, PADV, WM, WN, MT, NT, IM, false, true, FU, TA>), dim3((unsigned)blocks), dim3(256), (LDSB), stream, a);       \
    else LAUNCH((conv3d_mfma<KD, SS, TZ, TY, TX, KC, PADV, WM, WN, MT, NT, IM, false, false, FU, TA>), dim3((unsigned)blocks), dim3(256), (LDSB), stream, a);                 \
  } while (0)
#define MI355_LAUNCH_CONV(SS, IM, LDSB)                                                                                              \
  do {                                                                                                                         \
    if constexpr (KD == 3 && (IM == MI355_IN_PLAIN || IM == MI355_IN_AFFINE_ACT)) {                                            \
      if (fuse == 1) MI355_LAUNCH_CONV4(SS, IM, LDSB, 1);                                                                      \
      else if (fuse == 2) { if constexpr (IM == MI355_IN_PLAIN) MI355_LAUNCH_CONV4(SS, IM, LDSB, 2); else return MI355_EUNSUPPORTED; } \
      else MI355_LAUNCH_CONV4(SS, IM, LDSB, 0);                                                                                \
    } else MI355_LAUNCH_CONV4(SS, IM, LDSB, 0);                                                                                \
  } while (0)
  if (in_mode == MI355_IN_PLAIN) {
    MI355_LAUNCH_CONV(STRIDE, MI355_IN_PLAIN, lds);
  } else if (in_mode == MI355_IN_AFFINE_ACT) {
    MI355_LAUNCH_CONV(STRIDE, MI355_IN_AFFINE_ACT, lds);
  } else if (in_mode == MI355_IN_S2D) {
    if constexpr (KD == 1) {
      MI355_LAUNCH_CONV(1, MI355_IN_S2D, lds);
    } else return MI355_EUNSUPPORTED;
  } else {
    if constexpr (KD == 3) {
      if (STRIDE != 1) return MI355_EUNSUPPORTED;
      // parity-class form (4x8x8 tiles, 2 M tiles per wave): LDS holds the 3x5x5 coarse voxels only
      constexpr bool zip = TZ == 4 && TY == 8 && TX == 8 && WM == 4 && MT == 2;
      constexpr size_t lds_zi = zip ? (size_t)(TZ / 2 + 1) * (TY / 2 + 1) * (TX / 2 + 1) * (KC + PADV) * sizeof(float) : lds;
      MI355_LAUNCH_CONV(1, MI355_IN_ZERO_INSERT, lds_zi);
    } else return MI355_EUNSUPPORTED;
  }
#undef MI355_LAUNCH_CONV
#undef MI355_LAUNCH_CONV4
  return LAUNCH_CHECK();
}


// the instantiation of configuration p.cfg (kMfmaCfg) for storage type TA; 16-bit storage: the 1x1x1 and the stride-2 / zero-insert forms only
// (with exact-fp32 3x3x3 stride-1 arithmetic: no such kernel, act_form_exists)
template <typename TA>
static int launch_mfma(ConvArgs& a, int im, const FwdPlan& p, void* stream) {
  constexpr bool f32 = std::is_same<TA, float>::value;
  switch (p.cfg) {
    case 0: return launch_cfg<1, 1, 1, 1, 256, 32, 4, 4, 1, 2, 2, TA>(a, im, p, stream);
    case 1: return launch_cfg<1, 1, 1, 1, 256, 32, 4, 4, 1, 2, 1, TA>(a, im, p, stream);
    case 2: return launch_cfg<3, 2, 4, 4, 8, 8, 0, 4, 1, 1, 2, TA>(a, im, p, stream);
    case 3: return launch_cfg<3, 2, 4, 4, 8, 8, 0, 4, 1, 1, 1, TA>(a, im, p, stream);
    case 4: return launch_cfg<3, 1, 4, 8, 8, 16, 4, 4, 1, 2, 2, TA>(a, im, p, stream);
    case 5: return launch_cfg<3, 1, 4, 8, 8, 16, 4, 4, 1, 2, 1, TA>(a, im, p, stream);
    case 6: if constexpr (f32) return launch_cfg<3, 1, 2, 4, 8, 32, 4, 2, 2, 1, 1>(a, im, p, stream); break;
    case 7: if constexpr (f32) return launch_cfg<3, 1, 4, 4, 8, 32, 4, 4, 1, 1, 1>(a, im, p, stream); break;
    case 8: if constexpr (f32) return launch_cfg<3, 1, 4, 4, 8, 16, 4, 2, 2, 2, 1>(a, im, p, stream); break;
  }
  return MI355_EUNSUPPORTED;
}

extern "C" int32_t mi355_conv3d_stats_blocks(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d) {
  return plan_fwd(x, y, d).stats_blocks;
}

// the one validation and copy of a statistics request (also the 16-bit forward's, conv3d_bf16.hip, and the Winograd kernels', wino_common.h)
int mi355_fill_gn_fuse(GnFuseArgs& g, const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d) {
  memset(&g, 0, sizeof(g));
  if (!d->moments_out && !d->gn_bwd) return 0;
  if (d->moments_out && d->gn_bwd) return MI355_EUNSUPPORTED;      // a call is a forward (moments) or a dgrad (norm-backward sums), not both
  if (!stats_fusable(x, y, d)) return MI355_EUNSUPPORTED;
  g.mom = d->moments_out;
  if (d->gn_bwd) {
    const mi355_gn_bwd_fuse* f = d->gn_bwd;
    if (!f->gx || !f->scale || !f->shift || !f->mean_rstd || !f->partials_out || f->groups <= 0 || y->c % f->groups || f->gx_ld < y->c)
      return MI355_EINVAL;
    g.gnb = f->partials_out; g.gx = (const float*)f->gx; g.gxld = f->gx_ld; g.gscale = f->scale; g.gshift = f->shift; g.gmr = f->mean_rstd;
    g.ggroups = f->groups; g.gslope = f->act_slope;
  }
  return 0;
}

extern "C" int mi355_conv3d_fwd(const mi355_act* x, const float* wp, const mi355_act* y, const mi355_conv_desc* d, void* stream) {
  if (!x || !y || !wp || !d || !x->p || !y->p) return MI355_EINVAL;
  if ((d->kd != 1 && d->kd != 3) || (d->stride != 1 && d->stride != 2)) return MI355_EUNSUPPORTED;
  if (x->c % 4 || x->ld % 4 || x->ld < x->c || y->ld < y->c || x->n != y->n || !act_dtype_ok(x) || !act_dtype_ok(y)) return MI355_EINVAL;
  if (((uintptr_t)x->p & act_align_mask(x->dtype)) || ((uintptr_t)wp & 15)) return MI355_EINVAL;
  if (!affine_prologue_ok(d)) return MI355_EINVAL;
  if (d->in_mode < 0 || d->in_mode > 3) return MI355_EINVAL;
  if ((d->in_mode == MI355_IN_S2D || d->out_mode == MI355_OUT_D2S) && d->kd != 1) return MI355_EUNSUPPORTED;
  if (d->in_mode == MI355_IN_S2D && d->out_mode == MI355_OUT_D2S) return MI355_EUNSUPPORTED;
  if (d->out_mode != MI355_OUT_PLAIN && d->out_mode != MI355_OUT_D2S) return MI355_EINVAL;
  if (d->precision < MI355_PREC_F32 || d->precision > MI355_PREC_F16) return MI355_EINVAL;
  const FwdPlan p = plan_fwd(x, y, d);
  switch (p.route) {
    case FWD_REFUSED: return p.rc;
    case FWD_C4: return mi355_conv3d_c4_fwd_impl(x, wp, y, d, stream);
    case FWD_NARROW: return p.fuse ? MI355_EUNSUPPORTED : mi355_conv3d_narrow_impl(x, wp, y, d, stream);
    case FWD_LP16:
      if (d->out_d <= 0 || d->out_h <= 0 || d->out_w <= 0) return MI355_EINVAL;
      return mi355_conv3d_fwd_bf16_impl(x, wp, y, d, stream);
    case FWD_S2C32: return mi355_conv3d_s2c32_fwd_impl(x, wp, y, d, stream);
    case FWD_S2C32_DGRAD: return mi355_conv3d_s2c32_dgrad_impl(x, wp, y, d, stream);
    case FWD_K1_STREAM: return mi355_conv3d_k1_stream_impl(x, wp, y, d, stream);
    case FWD_MFMA: break;
  }
  if (act_is_lp16(x->dtype) && (y->c % 4 || y->ld % 4 || ((uintptr_t)y->p & 7))) return MI355_EINVAL;
  ConvArgs a;
  a.x = (const float*)x->p; a.xld = x->ld; a.wp = wp; a.y = (float*)y->p; a.yld = y->ld;
  a.res = (const float*)d->residual; a.resld = d->residual_ld;
  a.in_scale = d->in_scale; a.in_shift = d->in_shift; a.slope = d->act_slope;
  a.out_chscale = d->out_chscale; a.bias = d->bias;
  a.N = x->n; a.Di = x->d; a.Hi = x->h; a.Wi = x->w; a.Cin = x->c; a.CinP = pad8(x->c);
  a.Do = d->out_d; a.Ho = d->out_h; a.Wo = d->out_w; a.Cout = y->c; a.CoutP = pad32(y->c);
  a.yD = y->d; a.yH = y->h; a.yW = y->w; a.offz = d->off_z; a.offy = d->off_y; a.offx = d->off_x;
  a.pad = d->pad;
  a.in_slope = d->in_slope; a.outmode = d->out_mode; a.cD = a.cH = a.cW = 1; a.fC = 4;
  if (a.Do <= 0 || a.Ho <= 0 || a.Wo <= 0) return MI355_EINVAL;
  { const int rcg = mi355_fill_gn_fuse(a.g, x, y, d); if (rcg) return rcg; }
  if (a.res && a.resld < a.Cout) return MI355_EINVAL;
  const int im = d->in_mode;
  // 1x1x1: flatten (d,h,w) along x so tiles are 256 consecutive voxels (no halo); n stays separate for the per-(n,c) affine prologue.
  ConvArgs f = a;
  if (d->kd == 1) {
    if (d->stride != 1 || im == MI355_IN_ZERO_INSERT) return MI355_EUNSUPPORTED;
    long long vin = (long long)a.Di * a.Hi * a.Wi, vout = (long long)a.Do * a.Ho * a.Wo;
    long long vy = (long long)a.yD * a.yH * a.yW;
    if (im == MI355_IN_S2D) {
      // x is the fine tensor: the conv runs on the coarse grid (= y's grid) with 8*x->c logical input channels
      if (x->d != 2 * y->d || x->h != 2 * y->h || x->w != 2 * y->w || a.residual_or_chscale()) return MI355_EINVAL;
      f.cD = y->d; f.cH = y->h; f.cW = y->w; f.fC = x->c; f.Cin = 8 * x->c; f.CinP = pad8(f.Cin);
      vin = vout;
    } else if (d->out_mode == MI355_OUT_D2S) {
      // y is the fine tensor: the conv runs on x's grid with 8*y->c logical output channels
      if (y->d != 2 * x->d || y->h != 2 * x->h || y->w != 2 * x->w || a.residual_or_chscale()) return MI355_EINVAL;
      if (d->out_d != x->d || d->out_h != x->h || d->out_w != x->w || y->c % 4) return MI355_EINVAL;
      f.cD = x->d; f.cH = x->h; f.cW = x->w; f.fC = y->c; f.Cout = 8 * y->c; f.CoutP = f.Cout;
      vy = vout;
    }
    if (vin != vout || vy != vout || a.offz || a.offy || a.offx || vin > 0x7fffffffLL) return MI355_EUNSUPPORTED;
    f.Di = f.Hi = 1; f.Wi = (int)vin; f.Do = f.Ho = 1; f.Wo = (int)vout; f.yD = f.yH = 1; f.yW = (int)vy; f.pad = 0;
  }
  int rc;
  ACT_TYPED(x->dtype, TA, rc = launch_mfma<TA>(f, im, p, stream));
  return rc;
}

// Name of the kernel instantiation mi355_conv3d_fwd launches for this problem, as it appears (demangled) in a
// rocprofv3 kernel trace -- lets bench.py attribute HIP-event timings to the same symbol the profile reports.
extern "C" int mi355_conv3d_fwd_config(const mi355_act* x, const mi355_act* y, const mi355_conv_desc* d, char* out, size_t n) {
  if (!x || !y || !d || !out || n < 8) return MI355_EINVAL;
  const FwdPlan p = plan_fwd(x, y, d);
  switch (p.route) {
    case FWD_REFUSED: return p.rc;
    case FWD_C4: snprintf(out, n, d->precision == MI355_PREC_F32 ? "conv3d_c4_fwd" : "conv3d_c4_fwd_bf16"); return 0;
    case FWD_NARROW: snprintf(out, n, "conv3d_c4_dgrad"); return 0;
    case FWD_LP16: return mi355_conv3d_bf16_kernel_name(x, y, d, out, n);
    case FWD_S2C32: snprintf(out, n, "conv3d_s2c32_fwd"); return 0;
    case FWD_S2C32_DGRAD: snprintf(out, n, "conv3d_s2c32_dgrad"); return 0;
    case FWD_K1_STREAM: snprintf(out, n, "conv3d_k1_stream_bf16"); return 0;
    case FWD_MFMA: break;
  }
  snprintf(out, n, "conv3d_mfma<%d, %d, %s, %d, %s, %s>", d->kd, d->stride, kMfmaCfg[p.cfg].args, d->in_mode, p.tl ? "true" : "false",
           p.fullj ? "true" : "false");
  return 0;
}
