// TEST INFRASTRUCTURE ONLY -- see emu.h.
#include "emu.h"
#include <mutex>
#include <string>

namespace emu {

thread_local BlockState* g_bs = nullptr;
thread_local emu_dim3 g_threadIdx, g_blockIdx, g_blockDim, g_gridDim;

void fiber_entry() {
  BlockState* bs = g_bs;
  int me = bs->cur;
  bs->body();
  bs->fibers[me].done = true;
  swapcontext(&bs->fibers[me].ctx, &bs->sched);
}

void run_block(BlockState& bs) {
  bs.bar_count = 0; bs.bar_gen = 0;
  const unsigned nwaves = (bs.nthreads + 63) / 64;
  bs.dma_log.assign(nwaves, {}); bs.dma_wait_log.assign(nwaves, {});
  bs.dma_pending.assign(bs.nthreads, {}); bs.dma_cursor.assign(bs.nthreads, 0); bs.dma_waits.assign(bs.nthreads, 0);
  memset(bs.wbar_count, 0, sizeof(bs.wbar_count));
  memset(bs.wbar_gen, 0, sizeof(bs.wbar_gen));
  for (unsigned i = 0; i < bs.nthreads; ++i) {
    Fiber& f = bs.fibers[i];
    f.done = false;
    getcontext(&f.ctx);
    f.ctx.uc_stack.ss_sp = f.stack;
    f.ctx.uc_stack.ss_size = 128 * 1024;
    f.ctx.uc_link = nullptr;
    makecontext(&f.ctx, (void (*)())fiber_entry, 0);
  }
  unsigned remaining = bs.nthreads;
  while (remaining) {
    for (unsigned i = 0; i < bs.nthreads; ++i) {
      Fiber& f = bs.fibers[i];
      if (f.done) continue;
      bs.cur = (int)i;
      set_tid((int)i);
      swapcontext(&bs.sched, &f.ctx);
      if (f.done) --remaining;
    }
  }
}

static std::mutex g_launch_mu;
static std::string g_launches, g_geometry;

void record_launch(const char* kernel) {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  g_launches += kernel;
  g_launches += '\n';
}

void record_geometry(emu_dim3 grid, emu_dim3 block, size_t lds_bytes) {
  char line[128];
  snprintf(line, sizeof(line), "%u %u %u %u %u %u %zu\n", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds_bytes);
  std::lock_guard<std::mutex> lock(g_launch_mu);
  g_geometry += line;
}

}  // namespace emu

// The kernel expressions LAUNCHed since the previous call, one per line (as written in the source: "(conv3d_mfma<KD, ...>)"), into
// out[0, n); returns the length of the full record and clears it. (Not an mi355_ symbol: the library's C ABI is unaffected.)
extern "C" size_t emu_take_launches(char* out, size_t n) {
  std::lock_guard<std::mutex> lock(emu::g_launch_mu);
  const size_t len = emu::g_launches.size();
  if (out && n) snprintf(out, n, "%s", emu::g_launches.c_str());
  emu::g_launches.clear();
  return len;
}

// The geometry of the same launches, one line each ("gx gy gz bx by bz lds_bytes"), read and cleared like emu_take_launches and
// independently of it.
extern "C" size_t emu_take_geometry(char* out, size_t n) {
  std::lock_guard<std::mutex> lock(emu::g_launch_mu);
  const size_t len = emu::g_geometry.size();
  if (out && n) snprintf(out, n, "%s", emu::g_geometry.c_str());
  emu::g_geometry.clear();
  return len;
}
