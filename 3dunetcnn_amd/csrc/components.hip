// After the network, on the device: ensemble mean + threshold, connected-component labelling, largest-component / minimum-size cleanup.
//
//  examples/sppin/process.py:258-274 averages the cross-validation models' sigmoid outputs (np.mean(np.stack(...), axis=0)), thresholds
//  the mean (SimpleITK.BinaryThreshold(lowerThreshold=0.5): inclusive), labels the components (SimpleITK.ConnectedComponent: faces),
//  sorts them by size (RelabelComponent(sortByObjectSize=True)) and keeps the largest (== 1).
//
// Labelling is union-find over ONE int32 array: labels[v] = 1 + index of v's parent (0 = background). A link always points to a SMALLER
// linear index, so every chain strictly decreases, every tree's root is the smallest index it holds, and the final label
// (1 + smallest linear index of the component) does not depend on the order in which anything ran.
//
//   cc_local_kernel    one workgroup per 64 x 4 x 4 tile (x fastest): a wave owns an x-row, the ballot bitmap of the row gives every run
//                      of foreground voxels its first index (no x-direction unions at all); runs of neighbouring rows are united in LDS;
//                      labels = global index of the tile-local root.
//   cc_merge_kernel    every pair of neighbouring foreground voxels that lies in two tiles: unite the two trees in global memory.
//   cc_flatten_kernel  every voxel follows its chain to the root.
//
// NO WORKGROUP EVER WAITS FOR ANOTHER. There is no flag, no spin on a value somebody else must write, no grid-wide barrier: every loop
// below either walks a strictly decreasing chain (at most as long as the index it starts from) or is the union loop, whose `a` strictly
// decreases each time round. Workgroups of cc_merge_kernel talk only through the RETURNED value of atomicMin (an agent-scope
// read-modify-write, executed where all eight XCDs agree); everything else crosses a kernel boundary.
//
// Why a stale read cannot produce a wrong label (the XCDs' L2s are not coherent with each other, and a CU's L1 is never refreshed by
// another CU's stores): in cc_merge_kernel the only words that change are roots' words, only through atomicMin, only downwards, and a
// foreground word never becomes 0. g_find() may therefore return a vertex that was a root once and is not any more -- still a member
// of the same tree. The union loop then asks the authoritative copy: `old = atomicMin(&L[a], b)`. old == a: a WAS a root at that instant
// and now hangs under b (b < a, so no cycle): united. old != a: somebody lowered L[a] first; L[a] is now min(old, b), both members of
// trees that must end up united, and the loop goes on with the pair (old, b), old < a. Every step keeps "same tree => same component"
// and "the pair this thread was given ends in one tree"; the partition after the launch is the closure of all pairs, whatever was
// stale. g_find() reads with relaxed agent-scope loads (L1 bypassed) so that chains are usually fresh; correctness does not need it.
// No path compression with plain stores happens during the merge launch. cc_flatten_kernel does store while others read, but it runs
// after the kernel boundary, stores only `root + 1`, and both the old and the new word are ancestors of the voxel.
//
// Sizes (cc_sizes_kernel): NOT one global atomic per voxel onto the root -- a 9 M-voxel component would put 9 M adds on one address.
// A workgroup sums 1024 consecutive voxels per label in an LDS hash table (one insert per run of equal labels along x) and issues one
// global atomicAdd per (workgroup, label).
#include "gfx950_dialect.h"
#include "../../include/mi355_unet3d.h"
#include "volume_common.h"

#define CC_TX 64
#define CC_TY 4
#define CC_TZ 4
#define CC_ROWS (CC_TY * CC_TZ)
#define CC_TILE (CC_TX * CC_ROWS)
#define CC_HASH 1024                        // slots of the per-workgroup size table: a workgroup inserts at most 512 runs

#ifdef MI355_EMU
static inline int ld_agent(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
static inline int ld_lds(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
#else
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
#endif

// ---- a. ensemble mean + threshold -------------------------------------------------------------------------------------------------
__global__ void ensemble_threshold_kernel(const float* probs, int M, long long n, float thr, float* mean, unsigned char* mask, int vec) {
  const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const float fm = (float)M;
  if (vec) {                                               // 16-byte loads: n % 4 == 0 and every pointer suitably aligned
    const long long n4 = n >> 2;
    for (long long i = first; i < n4; i += stride) {
      float4 s = *reinterpret_cast<const float4*>(probs + 4 * i);
      for (int m = 1; m < M; ++m) {                        // index order 0 .. M-1
        const float4 q = *reinterpret_cast<const float4*>(probs + (size_t)m * n + 4 * i);
        s.x += q.x; s.y += q.y; s.z += q.z; s.w += q.w;
      }
      s.x = s.x / fm; s.y = s.y / fm; s.z = s.z / fm; s.w = s.w / fm;
      if (mean) *reinterpret_cast<float4*>(mean + 4 * i) = s;
      if (mask) reinterpret_cast<unsigned*>(mask)[i] = (s.x >= thr ? 1u : 0u) | (s.y >= thr ? 0x100u : 0u) | (s.z >= thr ? 0x10000u : 0u) |
                                                       (s.w >= thr ? 0x1000000u : 0u);
    }
    return;
  }
  for (long long i = first; i < n; i += stride) {
    float s = probs[i];
    for (int m = 1; m < M; ++m) s += probs[(size_t)m * n + i];
    s = s / fm;
    if (mean) mean[i] = s;
    if (mask) mask[i] = s >= thr ? 1 : 0;
  }
}

extern "C" int mi355_ensemble_threshold(const float* probs, int32_t m, int64_t elems, float threshold, float* mean, uint8_t* mask,
                                        void* stream) {
  if (!probs || m < 1 || elems <= 0 || (!mean && !mask)) return MI355_EINVAL;
  const int vec = (elems % 4 == 0) && ((uintptr_t)probs % 16 == 0) && ((uintptr_t)mean % 16 == 0) && ((uintptr_t)mask % 4 == 0);
  long long g = ((vec ? elems / 4 : elems) + 255) / 256;
  if (g > 16384) g = 16384;
  LAUNCH(ensemble_threshold_kernel, dim3((unsigned)g), dim3(256), 0, stream, probs, (int)m, (long long)elems, threshold, mean,
         (unsigned char*)mask, vec);
  return LAUNCH_CHECK();
}

// ---- b. connected components --------------------------------------------------------------------------------------------------------
// tile-local union-find in LDS: p[i] = parent of local voxel i (row * 64 + x), -1 = background
__device__ __forceinline__ int lds_find(const int* p, int a) {
  for (;;) { const int q = ld_lds(p + a); if (q == a) return a; a = q; }      // q < a: strictly decreasing
}
__device__ __forceinline__ void lds_unite(int* p, int a, int b) {
  for (;;) {
    a = lds_find(p, a); b = lds_find(p, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&p[a], b);
    if (old == a) return;
    a = old;                                                                    // old < a
  }
}

__global__ void __launch_bounds__(256) cc_local_kernel(const unsigned char* mask, int D, int H, int W, int tiles_x, int tiles_y, int conn26,
                                                       int* labels) {
  __shared__ int parent[CC_TILE];
  __shared__ unsigned long long rowbits[CC_ROWS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int t = blockIdx.x;
  const int tx = t % tiles_x; t /= tiles_x;
  const int ty = t % tiles_y, tz = t / tiles_y;
  const long long V = (long long)D * H * W;
  const unsigned char* m = mask + (size_t)blockIdx.y * V;
  int* L = labels + (size_t)blockIdx.y * V;
  const int x = tx * CC_TX + lane;
  // rows wave * 4 .. wave * 4 + 3 of the tile (row = local z * 4 + local y): bitmap of the row, first index of every run
  for (int k = 0; k < 4; ++k) {
    const int row = wave * 4 + k, z = tz * CC_TZ + (row >> 2), y = ty * CC_TY + (row & 3);
    const bool inb = x < W && y < H && z < D;
    const bool fg = inb && m[((long long)z * H + y) * W + x] != 0;
    const unsigned long long bits = LANE_MASK(fg);
    const unsigned long long below = ~bits & ((1ull << lane) - 1ull);           // background lanes below this one
    const int start = below ? 64 - __builtin_clzll(below) : 0;
    parent[row * CC_TX + lane] = fg ? row * CC_TX + start : -1;
    if (lane == 0) rowbits[row] = bits;
  }
  __syncthreads();
  // unite with the runs of the rows that come earlier in raster order: (dz, dy) = (0, -1), (-1, 0) and, for 26, (-1, -1), (-1, 1).
  // A pair (x, x) is skipped when (x-1, x-1) exists too: the two runs are the same two runs. Diagonal pairs (x, x +- 1) are needed only
  // where (x, x) is background in the other row: otherwise x +- 1 there belongs to the run of x.
  for (int k = 0; k < 4; ++k) {
    const int row = wave * 4 + k, lz = row >> 2, ly = row & 3, me = row * CC_TX + lane;
    const unsigned long long mine = rowbits[row];
    if (!((mine >> lane) & 1ull)) continue;
    const bool prev_me = lane > 0 && ((mine >> (lane - 1)) & 1ull);
    for (int j = 0; j < (conn26 ? 4 : 2); ++j) {
      const int nlz = lz - (j == 0 ? 0 : 1), nly = ly + (j == 0 ? -1 : (j == 1 ? 0 : (j == 2 ? -1 : 1)));
      if (nlz < 0 || nly < 0 || nly >= CC_TY) continue;
      const int nrow = nlz * 4 + nly;
      const unsigned long long nb = rowbits[nrow];
      if ((nb >> lane) & 1ull) {
        if (!(prev_me && ((nb >> (lane - 1)) & 1ull))) lds_unite(parent, me, nrow * CC_TX + lane);
      } else if (conn26) {
        if (lane > 0 && ((nb >> (lane - 1)) & 1ull)) lds_unite(parent, me, nrow * CC_TX + lane - 1);
        if (lane < 63 && ((nb >> (lane + 1)) & 1ull)) lds_unite(parent, me, nrow * CC_TX + lane + 1);
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int row = wave * 4 + k, z = tz * CC_TZ + (row >> 2), y = ty * CC_TY + (row & 3);
    if (!(x < W && y < H && z < D)) continue;
    int lab = 0;
    if (parent[row * CC_TX + lane] >= 0) {
      const int r = lds_find(parent, row * CC_TX + lane), rr = r >> 6;
      // the local order (z, y, x) is the global raster order: the local root is the smallest global index of the local component
      lab = 1 + (int)(((long long)(tz * CC_TZ + (rr >> 2)) * H + (ty * CC_TY + (rr & 3))) * W + tx * CC_TX + (r & 63));
    }
    L[((long long)z * H + y) * W + x] = lab;
  }
}

// global union-find on L[v] = 1 + parent(v). See the comment at the top of the file: g_find may be stale, atomicMin's return value is not.
__device__ __forceinline__ int g_find(const int* L, int a) {
  for (;;) { const int q = ld_agent(L + a) - 1; if (q == a) return a; a = q; }  // q < a: strictly decreasing
}
__device__ __forceinline__ void g_unite(int* L, int a, int b) {
  for (;;) {
    a = g_find(L, a); b = g_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b + 1) - 1;
    if (old == a) return;
    a = old;                                                                    // old < a
  }
}

// One thread per voxel; a foreground voxel handles the pairs it forms with EARLIER neighbours (raster order) in another tile. The skip
// rules of cc_local_kernel hold here as well: the pairs they lean on are united by that kernel (same tile) or by this one (other tile).
__global__ void __launch_bounds__(256) cc_merge_kernel(int D, int H, int W, int conn26, int* labels) {
  const long long V = (long long)D * H * W;
  const long long vv = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vv >= V) return;
  int* L = labels + (size_t)blockIdx.y * V;
  const int v = (int)vv;
  const int x = v % W, y = (v / W) % H, z = v / (W * H);
  const int lx = x & (CC_TX - 1), ly = y & (CC_TY - 1), lz = z & (CC_TZ - 1);
  if (!(lx == 0 || ly == 0 || lz == 0 || (conn26 && (lx == CC_TX - 1 || ly == CC_TY - 1)))) return;   // no earlier neighbour in another tile
  if (L[v] == 0) return;                                    // (0 never changes and nothing becomes 0: a plain load decides it)
  const bool prev_me = x > 0 && L[v - 1] != 0;
  if (lx == 0 && prev_me) g_unite(L, v, v - 1);
  for (int j = 0; j < (conn26 ? 4 : 2); ++j) {
    const int nz = z - (j == 0 ? 0 : 1), ny = y + (j == 0 ? -1 : (j == 1 ? 0 : (j == 2 ? -1 : 1)));
    if (nz < 0 || ny < 0 || ny >= H) continue;
    const bool row_crosses = (ny >> 2) != (y >> 2) || (nz >> 2) != (z >> 2);
    const int base = (int)(((long long)nz * H + ny) * W);
    if (L[base + x] != 0) {
      if (row_crosses && !(prev_me && L[base + x - 1] != 0)) g_unite(L, v, base + x);
    } else if (conn26) {
      if (x > 0 && (row_crosses || lx == 0) && L[base + x - 1] != 0) g_unite(L, v, base + x - 1);
      if (x + 1 < W && (row_crosses || lx == CC_TX - 1) && L[base + x + 1] != 0) g_unite(L, v, base + x + 1);
    }
  }
}

__global__ void __launch_bounds__(256) cc_flatten_kernel(long long V, int* labels) {
  const long long vv = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (vv >= V) return;
  int* L = labels + (size_t)blockIdx.y * V;
  int a = L[vv];
  if (a == 0) return;
  // plain loads: a word another thread of THIS launch rewrites holds an ancestor of the voxel before and after
  for (;;) { const int q = L[a - 1]; if (q == a) break; a = q; }
  L[vv] = a;
}

extern "C" int mi355_cc_label(const uint8_t* mask, int32_t c, int32_t d, int32_t h, int32_t w, int32_t connectivity, int32_t* labels,
                              void* stream) {
  if (!mask || !labels || (connectivity != 6 && connectivity != 26)) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  const long long V = (long long)d * h * w;
  const int tiles_x = ceil_div(w, CC_TX), tiles_y = ceil_div(h, CC_TY), tiles_z = ceil_div(d, CC_TZ), conn26 = connectivity == 26;
  LAUNCH(cc_local_kernel, dim3((unsigned)((long long)tiles_x * tiles_y * tiles_z), c), dim3(256), 0, stream, (const unsigned char*)mask,
         (int)d, (int)h, (int)w, tiles_x, tiles_y, conn26, (int*)labels);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_merge_kernel, dim3(vol_blocks(V, 256), c), dim3(256), 0, stream, (int)d, (int)h, (int)w, conn26, (int*)labels);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_flatten_kernel, dim3(vol_blocks(V, 256), c), dim3(256), 0, stream, V, (int*)labels);
  return LAUNCH_CHECK();
}

// ---- c. sizes, largest component, output mask -----------------------------------------------------------------------------------------
// workspace: [c] packed best (size << 32 | ~label: the maximum is the largest size, ties -> the smaller label), [c] component counts,
// [c][V] sizes (only the words at roots are ever touched)
static size_t cc_small_bytes(int32_t c) { return (size_t)c * 8 + (((size_t)c * 4 + 7) & ~(size_t)7); }
extern "C" size_t mi355_cc_workspace(int32_t c, int32_t d, int32_t h, int32_t w) {
  if (vol_check_dims(c, d, h, w)) return 0;
  return cc_small_bytes(c) + (size_t)c * d * h * w * 4;
}

__global__ void cc_zero_kernel(unsigned long long* best, int* count, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) { best[i] = 0ull; count[i] = 0; }
}

__global__ void __launch_bounds__(256) cc_roots_kernel(const int* labels, long long V, int* sizes) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  if (labels[(size_t)blockIdx.y * V + v] == (int)v + 1) sizes[(size_t)blockIdx.y * V + v] = 0;
}

__global__ void __launch_bounds__(256) cc_sizes_kernel(const int* labels, long long V, int* sizes) {
  __shared__ int keys[CC_HASH];
  __shared__ int vals[CC_HASH];
  const int lane = threadIdx.x & 63;
  const int* L = labels + (size_t)blockIdx.y * V;
  int* S = sizes + (size_t)blockIdx.y * V;
  for (int k = 0; k < CC_HASH / 256; ++k) { keys[threadIdx.x + 256 * k] = 0; vals[threadIdx.x + 256 * k] = 0; }
  __syncthreads();
  const long long base = (long long)blockIdx.x * 1024;
  for (int k = 0; k < 4; ++k) {
    const long long v = base + k * 256 + threadIdx.x;
    const int lab = v < V ? L[v] : 0;
    const int prev = __shfl(lab, (lane + 63) & 63);
    const bool start = lane == 0 || lab != prev;                                // first lane of a run of equal labels
    const unsigned long long sm = LANE_MASK(start);
    const unsigned long long above = lane == 63 ? 0ull : sm >> (lane + 1);
    const int len = above ? __builtin_ctzll(above) + 1 : 64 - lane;
    if (start && lab != 0) {
      unsigned s = ((unsigned)lab * 2654435761u) >> 22;                         // 10 bits
      for (;;) {                                                                // at most 512 keys in 1024 slots: an empty one is found
        const int old = atomicCAS(&keys[s], 0, lab);
        if (old == 0 || old == lab) { atomicAdd(&vals[s], len); break; }
        s = (s + 1) & (CC_HASH - 1);
      }
    }
  }
  __syncthreads();
  for (int k = 0; k < CC_HASH / 256; ++k) {
    const int s = threadIdx.x + 256 * k;
    if (keys[s] != 0) atomicAdd(&S[keys[s] - 1], vals[s]);                      // one add per (workgroup, component)
  }
}

__global__ void __launch_bounds__(256) cc_select_kernel(const int* labels, long long V, const int* sizes, unsigned long long* best, int* count) {
  __shared__ unsigned long long wbest[4];
  __shared__ int wcount[4];
  const int* L = labels + (size_t)blockIdx.y * V;
  const int* S = sizes + (size_t)blockIdx.y * V;
  const long long base = (long long)blockIdx.x * 1024;
  unsigned long long b = 0ull;
  int n = 0;
  for (int k = 0; k < 4; ++k) {
    const long long v = base + k * 256 + threadIdx.x;
    if (v < V && L[v] == (int)v + 1) {
      const unsigned long long key = ((unsigned long long)(unsigned)S[v] << 32) | (unsigned long long)(0xffffffffu - (unsigned)(v + 1));
      b = key > b ? key : b;
      ++n;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long ob = __shfl_xor(b, o);
    const int on = __shfl_xor(n, o);
    b = ob > b ? ob : b; n += on;
  }
  if ((threadIdx.x & 63) == 0) { wbest[threadIdx.x >> 6] = b; wcount[threadIdx.x >> 6] = n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < 4; ++i) { b = wbest[i] > b ? wbest[i] : b; n += wcount[i]; }
    if (n > 0) { atomicMax(&best[blockIdx.y], b); atomicAdd(&count[blockIdx.y], n); }
  }
}

__global__ void __launch_bounds__(256) cc_write_kernel(const unsigned char* mask, const int* labels, long long V, const int* sizes,
                                                       const unsigned long long* best, const int* count, int keep_largest,
                                                       long long min_size, unsigned char* out, int* stats) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= V) return;
  const size_t i = (size_t)blockIdx.y * V + v;
  const unsigned long long b = best[blockIdx.y];
  const int winner = b ? (int)(0xffffffffu - (unsigned)(b & 0xffffffffull)) : 0;
  if (v == 0 && stats) { stats[3 * blockIdx.y] = count[blockIdx.y]; stats[3 * blockIdx.y + 1] = (int)(b >> 32); stats[3 * blockIdx.y + 2] = winner; }
  const int lab = labels[i];
  bool keep = mask[i] != 0 && lab != 0;
  if (keep) keep = (long long)sizes[(size_t)blockIdx.y * V + lab - 1] >= min_size && (!keep_largest || lab == winner);
  out[i] = keep ? 1 : 0;
}

extern "C" int mi355_cc_filter(const uint8_t* mask, const int32_t* labels, int32_t c, int32_t d, int32_t h, int32_t w, int32_t keep_largest,
                               int64_t min_size, uint8_t* out, int32_t* stats, void* ws, size_t ws_bytes, void* stream) {
  if (!mask || !labels || !out || !ws) return MI355_EINVAL;
  int rc = vol_check_dims(c, d, h, w); if (rc) return rc;
  if (ws_bytes < mi355_cc_workspace(c, d, h, w)) return MI355_EWORKSPACE;
  const long long V = (long long)d * h * w;
  unsigned long long* best = (unsigned long long*)ws;
  int* count = (int*)((char*)ws + (size_t)c * 8);
  int* sizes = (int*)((char*)ws + cc_small_bytes(c));
  const int* L = (const int*)labels;
  LAUNCH(cc_zero_kernel, dim3(vol_blocks(c, 256)), dim3(256), 0, stream, best, count, (int)c);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_roots_kernel, dim3(vol_blocks(V, 256), c), dim3(256), 0, stream, L, V, sizes);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_sizes_kernel, dim3(vol_blocks(V, 1024), c), dim3(256), 0, stream, L, V, sizes);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_select_kernel, dim3(vol_blocks(V, 1024), c), dim3(256), 0, stream, L, V, (const int*)sizes, best, count);
  rc = LAUNCH_CHECK(); if (rc) return rc;
  LAUNCH(cc_write_kernel, dim3(vol_blocks(V, 256), c), dim3(256), 0, stream, (const unsigned char*)mask, L, V, (const int*)sizes,
         (const unsigned long long*)best, (const int*)count, (int)keep_largest, (long long)min_size, (unsigned char*)out, (int*)stats);
  return LAUNCH_CHECK();
}
