// Internal helpers shared by the .hip translation units of liborigin_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/origin_hip.h"

// kernel classes timed by the built-in HIP-event profiler (origin_prof_*)
enum OriginKernelId {
  K_DCT_FIT = 0,
  K_DCT_SUMS,
  K_DCT_STANDARDIZE,
  K_DCT_CONTINUUM,
  K_O2,
  K_PCA_SELECT,
  K_PCA_BMEAN,
  K_PCA_GATHER,
  K_PCA_PROJECT,
  K_PCA_GRAM,
  K_PCA_EIG,
  K_PCA_UVEC,
  K_PCA_DEFLATE_DOT,
  K_PCA_DEFLATE_UPDATE,
  K_PCA_FLUSH,
  K_GLR_SPATIAL,
  K_GLR_SPECTRAL,
  K_GLR_BORDER,
  K_GLR_TABLES,
  K_LOCAL_MAX,
  K_SMALL,
  K_PCA_TOTAL,  // the whole greedy PCA as one scope (level 1; its kernels are level-2 scopes)
  K_LINES_GATHER,   // line estimation (lines.hip): gather / standardise / centre, and the clean pass
  K_LINES_UVEC,     // u = A v / |A v| and the DCT denoising of u
  K_LINES_PROJECT,  // t = A^T u (column reduction over z)
  K_LINES_LS,       // residual + weighted least-squares deconvolution, one wave per row
  K_LINES_SELECT,   // peakdet / flux / mse per grid offset and the winner of each detection
  K_MERGE_BIN,       // spatio-spectral merging (merge.hip): rows binned by spaxel
  K_MERGE_COMP,      // components of the near graph (hook / compress rounds, labels)
  K_MERGE_STAGE1,    // seeds and their groups, one workgroup per component
  K_MERGE_RENUMBER,  // seed ranks, group ids, the largest area of a group
  K_MERGE_STAGE2,    // z bitmaps and the cu / otg walk, one wave per area label
  K_STATS,           // moments of a cube (stats.hip): the streaming pass and its final wave
  K_SEGMAP_MASK,     // segmentation maps (segmap.hip): threshold, erosion, dilation, disc, union
  K_SEGMAP_LABEL,    // connected components: tiles, seams, flatten, scan, ranks, labels
  K_MATCH_BIN,       // matching of point lists (match.hip): B binned into 3-D cells
  K_MATCH_QUERY,     // every point of A against the cells around it
  K_COUNT
};

struct OriginProfEvent {
  hipEvent_t a, b;
  int id;
};

constexpr int ORIGIN_TIMER_SLOTS = 64;

// a device buffer that only grows (origin_grow)
struct GrowBuffer {
  void *p = nullptr;
  size_t bytes = 0;
};

// A second stream beside the context's main one, made on first use.  begin: the stream waits for
// what the main stream has been given so far; end: `join` is recorded behind the work enqueued
// since and `pending` set; join: the main stream waits for `join` (no host sync); wait: the host
// does.  The last two clear `pending` and do nothing where nothing is pending.
struct ForkStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  bool pending = false;
};

struct AllocCache;  // ctx.hip

struct origin_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_start[ORIGIN_TIMER_SLOTS] = {};
  hipEvent_t ev_stop[ORIGIN_TIMER_SLOTS] = {};
  bool ev_made[ORIGIN_TIMER_SLOTS] = {};
  GrowBuffer scratch;  // partial reductions of the main stream's kernels
  int num_cu = 0;
  // cached DCT cosine table (dct.hip)
  double *ctab = nullptr;
  int ctab_nz = 0, ctab_order = 0;
  // per-kernel-class timing with HIP events on the stream the kernels run on
  int prof_level = 0;  // 0 off, 1 coarse (one scope per large kernel / per PCA run), 2 + every PCA kernel
  std::vector<OriginProfEvent> prof_pending;
  std::vector<hipEvent_t> prof_free;
  double prof_ms[K_COUNT] = {};
  long prof_n[K_COUNT] = {};
  // persistent workspace of origin_pca_run (owned by pca.hip)
  void *pca_ws = nullptr;
  void (*pca_ws_free)(void *) = nullptr;
  // Auxiliary stream, of the lowest priority: an HBM-bound pass nothing downstream waits for (the
  // cont_dct cube of origin_dct_cont_std_async) runs here in the shadow of the greedy PCA's
  // latency-bound kernels, with a scratch of its own (the PCA uses the main one).
  // origin_aux_join() makes the main stream wait for it, origin_sync() waits for every stream.
  ForkStream aux;
  GrowBuffer aux_scratch;
  // Side stream of the row-band GLR (origin_glr_run_rows with ORIGIN_GLR_SIDE): restricted to the
  // first num_cu - reserve compute units, so that a band started while the greedy PCA still
  // iterates over its last areas leaves CUs to the PCA's small kernels.  Its join event is
  // recorded behind the band; origin_glr_run_finish / origin_sync wait for it.
  ForkStream side;
  // pinned staging of every host copy of 32 MiB or more (origin_h2d, origin_d2h) and of the two
  // conversions (origin_d2h_f32_as_f64, origin_h2d_f64_as_f32): two 64 MiB buffers and two events,
  // made by the first such call on this context (all or nothing) and freed with it
  char *stage_buf[2] = {nullptr, nullptr};
  hipEvent_t stage_ev[2] = {nullptr, nullptr};
  bool stage_ready = false;
  // greedy PCA: called once, when at most pca_tail_max areas still iterate, after the areas that
  // have finished were written to the output (origin_pca_set_tail_hook, pca.hip)
  void (*pca_tail_hook)(void *user, int n_active, const int *areas) = nullptr;
  void *pca_tail_user = nullptr;
  int pca_tail_max = 0;
  // device blocks released by origin_free and kept for the next origin_malloc of their size
  // (ctx.hip: a hipMalloc of a 5 GB cube takes ~40 ms, a hipFree synchronises the device)
  AllocCache *alloc_cache = nullptr;
};

// forked-stream plumbing (ctx.hip); `create` makes the stream on first use
int origin_make_aux_stream(origin_ctx *ctx, hipStream_t *out);
int origin_make_side_stream(origin_ctx *ctx, hipStream_t *out);
int origin_fork_begin(origin_ctx *ctx, ForkStream &f, int (*create)(origin_ctx *, hipStream_t *));
int origin_fork_end(ForkStream &f);
int origin_fork_join(origin_ctx *ctx, ForkStream &f);
int origin_fork_wait(ForkStream &f);

// An event pair costs ~10 us of stream time on this hardware (barrier packets): 13 scopes in each
// of the 56 PCA iterations add 5 ms to a 95 ms step.  Scopes therefore carry a level; bench.py
// times its steps at level 1 (a handful of pairs per step) and takes the per-kernel PCA detail
// from an extra, untimed step at level 2.
int origin_prof_begin(origin_ctx *ctx, int id);  // returns the entry index
void origin_prof_end(origin_ctx *ctx, int entry);

// RAII: times everything enqueued on ctx->stream during its lifetime as kernel class `id`
struct ProfScope {
  origin_ctx *ctx;
  int entry;
  ProfScope(origin_ctx *c, int id, int level = 1) : ctx(c), entry(-1) {
    if (ctx->prof_level >= level) entry = origin_prof_begin(ctx, id);
  }
  // close the scope and open a new one of class `id` (same level)
  void next(int id) {
    if (entry >= 0) {
      origin_prof_end(ctx, entry);
      entry = origin_prof_begin(ctx, id);
    }
  }
  ~ProfScope() {
    if (entry >= 0) origin_prof_end(ctx, entry);
  }
};

void origin_set_error(const char *fmt, ...);
// at least `bytes` of b; before a smaller buffer is freed, `sync` (the stream that used it) drains
int origin_grow(GrowBuffer &b, size_t bytes, hipStream_t sync, void **out);
static inline int origin_scratch(origin_ctx *ctx, size_t bytes, void **out) {
  return origin_grow(ctx->scratch, bytes, ctx->stream, out);
}

// glr_spatial_mfma.hip: matrix-core spatial GLR stage (one field, or one weighted field of a
// mosaic: W its weight map, accf = add to what the fields before left in out)
int origin_spatial_mfma_ok(int Ny, int Nx, int P);
// (ry0, nry / rx0, nrx: rows / columns of 64 x 64 regions to run, <= 0 = all of them)
int origin_spatial_mfma_launch(origin_ctx *ctx, int terms, const float *A, const float *W,
                               const float *taps, int Nz, int Ny, int Nx, int P, int accf,
                               float *out, int ry0 = 0, int nry = 0, int rx0 = 0, int nrx = 0);
long origin_spatial_mfma_count(int terms, int Nz, int Ny, int Nx, int P);

// An origin_malloc'd block that is freed with its scope, and the host drivers' way to lay a
// workspace out in one (merge.hip, lines.hip): the pieces are listed once, in a layout function.
struct DevMem {
  origin_ctx *ctx;
  void *p = nullptr;
  explicit DevMem(origin_ctx *c) : ctx(c) {}
  int alloc(size_t bytes) { return origin_malloc(ctx, std::max(bytes, (size_t)256), &p); }
  ~DevMem() {
    if (p) (void)origin_free(ctx, p);
  }
};

struct Carver {  // consecutive 256-byte aligned pieces of one block; null base: sizes only
  size_t off = 0;
  char *base = nullptr;
  template <class T>
  T *take(size_t n) {
    T *r = base ? (T *)(base + off) : nullptr;
    off += (n * sizeof(T) + 255) & ~(size_t)255;
    return r;
  }
};

// `layout(Carver &)` takes its pieces and stores their pointers: once without a block, for the
// size; then `mem` is allocated and the layout runs again on it.  The allocation's ORIGIN_* code.
template <class Layout>
int carve_block(origin_ctx *ctx, DevMem &mem, Layout &&layout) {
  Carver c;
  layout(c);
  const int rc = mem.alloc(c.off);
  if (rc) return rc;
  c.off = 0, c.base = (char *)mem.p;
  layout(c);
  return ORIGIN_OK;
}

// Streamed file I/O (fits.hip, ingest.hip): a data unit moves in chunks of at most this many
// bytes through two pinned host buffers, each with the event that says its copy has drained.
constexpr long IO_CHUNK_BYTES = 64l << 20;

struct IoStage {
  void *h[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~IoStage() {
    for (int i = 0; i < 2; ++i) {
      if (h[i]) (void)hipHostFree(h[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
  }
};

template <class T>
int put(origin_ctx *ctx, T *d, const std::vector<T> &h) {
  return origin_h2d(ctx, d, h.data(), h.size() * sizeof(T));
}

#define ORIGIN_CHECK_ARG(cond, ...)       \
  do {                                    \
    if (!(cond)) {                        \
      origin_set_error(__VA_ARGS__);      \
      return ORIGIN_E_ARG;                \
    }                                     \
  } while (0)

#define ORIGIN_HIP(call)                                                              \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess) {                                                           \
      origin_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                       __LINE__);                                                     \
      return e_ == hipErrorOutOfMemory ? ORIGIN_E_NOMEM : ORIGIN_E_HIP;               \
    }                                                                                 \
  } while (0)

#define ORIGIN_LAUNCH_CHECK() ORIGIN_HIP(hipGetLastError())

static inline int origin_use(origin_ctx *ctx) {
  if (!ctx) {
    origin_set_error("null context");
    return ORIGIN_E_ARG;
  }
  ORIGIN_HIP(hipSetDevice(ctx->device));
  return ORIGIN_OK;
}

#define ORIGIN_USE(ctx)            \
  do {                             \
    int r_ = origin_use(ctx);      \
    if (r_ != ORIGIN_OK) return r_; \
  } while (0)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// a[0..L) -> its exclusive prefix sums in place, a[L] = the total; ONE workgroup of THREADS,
// thread t takes the chunk [t * per, (t + 1) * per) (merge.hip, segmap.hip, match.hip)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void origin_scan_kernel(int L, int *a) {
  __shared__ int part[THREADS];
  const int t = threadIdx.x;
  const int per = (L + THREADS - 1) / THREADS;
  const int lo = min(L, t * per), hi = min(L, lo + per);
  int s = 0;
  for (int i = lo; i < hi; ++i) s += a[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = part[t] - s;
  for (int i = lo; i < hi; ++i) {
    const int v = a[i];
    a[i] = base;
    base += v;
  }
  if (t == THREADS - 1) a[L] = part[t];
}

// hipFuncSetAttribute (the dynamic-LDS ceiling of a kernel) holds per DEVICE, and a process may
// drive several devices from several threads (origin_amd/session.py: one context and one thread
// per GPU): the statements run once per device, under a lock -- a second thread on the same device
// must not launch before the attribute is there.  They may leave through ORIGIN_HIP.
struct OriginPerDeviceOnce {
  std::mutex mu;
  unsigned long long done = 0;
};
#define ORIGIN_ONCE_PER_DEVICE(ctx, state, ...)                          \
  do {                                                                   \
    std::lock_guard<std::mutex> lk_((state).mu);                         \
    const unsigned long long bit_ = 1ull << ((ctx)->device & 63);        \
    if (!((state).done & bit_)) {                                        \
      __VA_ARGS__;                                                       \
      (state).done |= bit_;                                              \
    }                                                                    \
  } while (0)
