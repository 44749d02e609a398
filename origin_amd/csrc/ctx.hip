// Context, device memory, copies and HIP-event timers of liborigin_hip.so.
#include <sys/mman.h>

#include <algorithm>
#include <cstdlib>
#include <map>
#include <unordered_map>

#include <functional>

#include <cstring>
#include "common.h"

void origin_host_pool_run(int n, const std::function<void(int)> &task);  // thresh.hip (C++ linkage)

static thread_local char g_err[1024] = "";

// Blocks of at least 1 MiB that origin_free releases are kept (up to ORIGIN_ALLOC_CACHE_GB, default
// 96, 0 = off) and handed to the next origin_malloc that asks for their size or up to an eighth
// less.  The Step seam allocates every output of every step afresh (the reference's steps return
// new arrays): at 3681 x 600 x 600 that was 27 allocations of up to 5.3 GB at ~40 ms each -- 1.2 s
// of a 3.2 s pass (tools/e2e_profile.py) -- and a device-wide synchronisation per release.  Reuse
// is ordered by the context's stream: origin_free makes it wait for the auxiliary and side streams,
// and every kernel of the library runs on one of the three.
struct AllocCache {
  std::mutex mu;
  std::unordered_map<void *, size_t> live;     // blocks handed out (>= ALLOC_MIN): their sizes
  std::multimap<size_t, void *> spare;         // released blocks by size
  size_t spare_bytes = 0, cap_bytes = 0;
};
constexpr size_t ALLOC_MIN = (size_t)1 << 20;

static size_t alloc_cache_spare(AllocCache *c) {
  std::lock_guard<std::mutex> lk(c->mu);
  return c->spare_bytes;
}

static void alloc_cache_release(origin_ctx *ctx, bool destroy) {
  AllocCache *c = ctx->alloc_cache;
  if (!c) return;
  {
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->spare.empty()) (void)hipStreamSynchronize(ctx->stream);
    for (auto &kv : c->spare) (void)hipFree(kv.second);
    c->spare.clear();
    c->spare_bytes = 0;
  }
  if (destroy) {
    delete c;
    ctx->alloc_cache = nullptr;
  }
}

// strided (nz, ny, rowbytes) box copy, device to device; 16 bytes per thread when aligned
__global__ __launch_bounds__(256) void copy_box_kernel(char *__restrict__ dst, long dpy, long dpz,
                                                       const char *__restrict__ src, long spy,
                                                       long spz, int ny, long rowbytes, int vec) {
  const int z = blockIdx.z;
  const int y = blockIdx.y;
  const long x = ((long)blockIdx.x * 256 + threadIdx.x) * vec;
  if (y >= ny || x >= rowbytes) return;
  const char *s = src + (long)z * spz + (long)y * spy + x;
  char *d = dst + (long)z * dpz + (long)y * dpy + x;
  if (vec == 16) {
    *reinterpret_cast<uint4 *>(d) = *reinterpret_cast<const uint4 *>(s);
  } else if (vec == 4) {
    *reinterpret_cast<unsigned *>(d) = *reinterpret_cast<const unsigned *>(s);
  } else {
    *d = *s;
  }
}

void origin_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int origin_grow(GrowBuffer &b, size_t bytes, hipStream_t sync, void **out) {
  if (bytes > b.bytes) {
    if (b.p) {
      if (sync) ORIGIN_HIP(hipStreamSynchronize(sync));
      ORIGIN_HIP(hipFree(b.p));
      b.p = nullptr;
      b.bytes = 0;
    }
    const size_t want = bytes + bytes / 4 + (1 << 20);
    ORIGIN_HIP(hipMalloc(&b.p, want));
    b.bytes = want;
  }
  *out = b.p;
  return ORIGIN_OK;
}

// The side stream: every CU but the last `reserve` (ORIGIN_GLR_SIDE_RESERVE, default an eighth of
// the chip: 32 of 256).  Measured at 3681 x 600 x 600 with the GLR's early bands beside the greedy
// PCA's tail (tools/tail_overlap_tune.sh, profiles/r03_tail_overlap_tune.txt): step 55.8 ms with
// no reserve (the PCA's small kernels wait for a GLR workgroup to leave a CU: no better than
// running the two in sequence, 55.9), 53.8 / 53.3 / 53.1 with 8 / 16 / 24 CUs, 51.9 with 32,
// 52.4 / 52.7 / 53.0 with 40 / 64 / 96.
int origin_make_side_stream(origin_ctx *ctx, hipStream_t *out) {
  const char *e = getenv("ORIGIN_GLR_SIDE_RESERVE");
  const int ncu = ctx->num_cu > 0 ? std::min(ctx->num_cu, 256) : 256;
  int reserve = e ? atoi(e) : ncu / 8;
  reserve = std::max(0, std::min(reserve, ncu - 8));
  uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < ncu - reserve; ++i) mask[i >> 5] |= 1u << (i & 31);
  if (hipExtStreamCreateWithCUMask(out, 8, mask) != hipSuccess) {
    // (no CU masks on this runtime: a stream of the lowest priority still gives correct results,
    // only less of an overlap -- the main stream's small kernels wait for CUs)
    (void)hipGetLastError();
    return origin_make_aux_stream(ctx, out);
  }
  return ORIGIN_OK;
}

// The aux stream has the lowest priority the device offers: its thousands of HBM-bound workgroups
// must not sit in front of the one-block kernels of the PCA.
int origin_make_aux_stream(origin_ctx *, hipStream_t *out) {
  int lo = 0, hi = 0;
  ORIGIN_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));  // lo = least urgent
  ORIGIN_HIP(hipStreamCreateWithPriority(out, hipStreamNonBlocking, lo));
  return ORIGIN_OK;
}

// Work enqueued on the stream afterwards starts behind everything the main stream has been given
// so far.
int origin_fork_begin(origin_ctx *ctx, ForkStream &f, int (*create)(origin_ctx *, hipStream_t *)) {
  if (!f.stream) {
    if (int rc = create(ctx, &f.stream)) return rc;
    ORIGIN_HIP(hipEventCreateWithFlags(&f.fork, hipEventDisableTiming));
    ORIGIN_HIP(hipEventCreateWithFlags(&f.join, hipEventDisableTiming));
  }
  ORIGIN_HIP(hipEventRecord(f.fork, ctx->stream));
  ORIGIN_HIP(hipStreamWaitEvent(f.stream, f.fork, 0));
  return ORIGIN_OK;
}

int origin_fork_end(ForkStream &f) {
  ORIGIN_HIP(hipEventRecord(f.join, f.stream));
  f.pending = true;
  return ORIGIN_OK;
}

int origin_fork_join(origin_ctx *ctx, ForkStream &f) {
  if (f.stream && f.pending) {
    ORIGIN_HIP(hipStreamWaitEvent(ctx->stream, f.join, 0));
    f.pending = false;
  }
  return ORIGIN_OK;
}

int origin_fork_wait(ForkStream &f) {
  if (f.stream && f.pending) {
    ORIGIN_HIP(hipStreamSynchronize(f.stream));
    f.pending = false;
  }
  return ORIGIN_OK;
}

static hipEvent_t prof_event(origin_ctx *ctx) {
  if (!ctx->prof_free.empty()) {
    hipEvent_t e = ctx->prof_free.back();
    ctx->prof_free.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

static void prof_drain(origin_ctx *ctx) {
  for (auto &p : ctx->prof_pending) {
    float ms = 0.f;
    if (p.a && p.b && hipEventSynchronize(p.b) == hipSuccess &&
        hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
      ctx->prof_ms[p.id] += ms;
      ctx->prof_n[p.id] += 1;
    }
    if (p.a) ctx->prof_free.push_back(p.a);
    if (p.b) ctx->prof_free.push_back(p.b);
  }
  ctx->prof_pending.clear();
}

int origin_prof_begin(origin_ctx *ctx, int id) {
  OriginProfEvent p;
  p.a = prof_event(ctx);
  p.b = nullptr;
  p.id = id;
  if (p.a) (void)hipEventRecord(p.a, ctx->stream);
  ctx->prof_pending.push_back(p);
  return (int)ctx->prof_pending.size() - 1;
}

void origin_prof_end(origin_ctx *ctx, int entry) {
  if (entry < 0 || entry >= (int)ctx->prof_pending.size()) return;
  OriginProfEvent &p = ctx->prof_pending[entry];
  p.b = prof_event(ctx);
  if (p.b) (void)hipEventRecord(p.b, ctx->stream);
}

static const char *kKernelNames[K_COUNT] = {
    "dct_fit",         "dct_plane_sums",     "dct_standardize", "dct_continuum", "o2",
    "pca_select",      "pca_bmean",          "pca_gather",      "pca_project",   "pca_gram",
    "pca_eig",         "pca_uvec",
    "pca_deflate_dot", "pca_deflate_finish", "pca_flush", "glr_spatial",     "glr_spectral",  "glr_border", "glr_tables",
    "local_max",       "small",              "pca_total",
    "lines_gather",    "lines_uvec",         "lines_project",   "lines_ls",      "lines_select",
    "merge_bin",       "merge_components",   "merge_stage1",    "merge_renumber", "merge_stage2",
    "cube_moments",    "segmap_mask",        "segmap_label",    "match_bin",     "match_query"};

extern "C" {

int origin_prof_enable(origin_ctx *ctx, int on) {
  ORIGIN_USE(ctx);
  prof_drain(ctx);
  ctx->prof_level = on < 0 ? 0 : (on > 2 ? 2 : on);
  return ORIGIN_OK;
}

int origin_prof_reset(origin_ctx *ctx) {
  ORIGIN_USE(ctx);
  prof_drain(ctx);
  memset(ctx->prof_ms, 0, sizeof(ctx->prof_ms));
  memset(ctx->prof_n, 0, sizeof(ctx->prof_n));
  return ORIGIN_OK;
}

int origin_prof_count(void) { return K_COUNT; }

int origin_prof_get(origin_ctx *ctx, int id, const char **name, double *total_ms, long *launches) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(id >= 0 && id < K_COUNT, "kernel id out of range");
  prof_drain(ctx);
  if (name) *name = kKernelNames[id];
  if (total_ms) *total_ms = ctx->prof_ms[id];
  if (launches) *launches = ctx->prof_n[id];
  return ORIGIN_OK;
}

const char *origin_last_error(void) { return g_err; }

int origin_abi_version(void) { return 1; }

int origin_device_count(int *count) {
  ORIGIN_CHECK_ARG(count, "count is null");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    origin_set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
    return ORIGIN_E_NODEVICE;
  }
  *count = n;
  return ORIGIN_OK;
}

int origin_ctx_create(int device, origin_ctx **out) {
  ORIGIN_CHECK_ARG(out, "out is null");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    origin_set_error("no HIP device visible");
    return ORIGIN_E_NODEVICE;
  }
  ORIGIN_CHECK_ARG(device >= 0 && device < n, "device %d out of range [0,%d)", device, n);
  ORIGIN_HIP(hipSetDevice(device));
  origin_ctx *ctx = new origin_ctx();
  ctx->device = device;
  hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ctx;
    origin_set_error("hipStreamCreate: %s", hipGetErrorString(e));
    return ORIGIN_E_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->num_cu = prop.multiProcessorCount;
  if (ctx->num_cu <= 0) ctx->num_cu = 256;
  ctx->alloc_cache = new AllocCache();
  const char *gb = getenv("ORIGIN_ALLOC_CACHE_GB");
  ctx->alloc_cache->cap_bytes = (size_t)((gb ? atof(gb) : 96.0) * 1e9);
  *out = ctx;
  return ORIGIN_OK;
}

int origin_ctx_destroy(origin_ctx *ctx) {
  if (!ctx) return ORIGIN_OK;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  for (int i = 0; i < ORIGIN_TIMER_SLOTS; ++i)
    if (ctx->ev_made[i]) {
      hipEventDestroy(ctx->ev_start[i]);
      hipEventDestroy(ctx->ev_stop[i]);
    }
  for (ForkStream *f : {&ctx->aux, &ctx->side})
    if (f->stream) {
      hipStreamSynchronize(f->stream);
      hipStreamDestroy(f->stream);
      hipEventDestroy(f->fork);
      hipEventDestroy(f->join);
    }
  if (ctx->stage_ready) {
    for (int b = 0; b < 2; ++b) {
      hipHostFree(ctx->stage_buf[b]);
      hipEventDestroy(ctx->stage_ev[b]);
    }
  }
  alloc_cache_release(ctx, true);
  if (ctx->aux_scratch.p) hipFree(ctx->aux_scratch.p);
  if (ctx->scratch.p) hipFree(ctx->scratch.p);
  if (ctx->ctab) hipFree(ctx->ctab);
  if (ctx->pca_ws && ctx->pca_ws_free) ctx->pca_ws_free(ctx->pca_ws);
  prof_drain(ctx);
  for (hipEvent_t e : ctx->prof_free) hipEventDestroy(e);
  hipStreamDestroy(ctx->stream);
  delete ctx;
  return ORIGIN_OK;
}

int origin_sync(origin_ctx *ctx) {
  ORIGIN_USE(ctx);
  if (int rc = origin_fork_wait(ctx->side)) return rc;
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return origin_fork_wait(ctx->aux);
}

int origin_aux_join(origin_ctx *ctx) {
  ORIGIN_USE(ctx);
  return origin_fork_join(ctx, ctx->aux);
}

int origin_device_name(origin_ctx *ctx, char *buf, int buflen) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(buf && buflen > 0, "bad buffer");
  hipDeviceProp_t prop;
  ORIGIN_HIP(hipGetDeviceProperties(&prop, ctx->device));
  snprintf(buf, buflen, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return ORIGIN_OK;
}

int origin_mem_info(origin_ctx *ctx, size_t *free_bytes, size_t *total_bytes) {
  ORIGIN_USE(ctx);
  size_t f = 0, t = 0;
  ORIGIN_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f + alloc_cache_spare(ctx->alloc_cache);  // (spare blocks go back when memory runs out)
  if (total_bytes) *total_bytes = t;
  return ORIGIN_OK;
}

int origin_stream(origin_ctx *ctx, void **stream) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(stream, "stream is null");
  *stream = (void *)ctx->stream;
  return ORIGIN_OK;
}

int origin_malloc(origin_ctx *ctx, size_t bytes, void **d_ptr) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_ptr, "d_ptr is null");
  *d_ptr = nullptr;
  if (bytes == 0) bytes = 16;
  AllocCache *c = ctx->alloc_cache;
  if (bytes >= ALLOC_MIN && c->cap_bytes > 0) {
    std::lock_guard<std::mutex> lk(c->mu);
    auto it = c->spare.lower_bound(bytes);
    if (it != c->spare.end() && it->first - bytes <= bytes / 8) {
      *d_ptr = it->second;
      c->live[it->second] = it->first;
      c->spare_bytes -= it->first;
      c->spare.erase(it);
      return ORIGIN_OK;
    }
  }
  hipError_t e = hipMalloc(d_ptr, bytes);
  if (e == hipErrorOutOfMemory && alloc_cache_spare(c) > 0) {  // give the spare blocks back and try again
    (void)hipGetLastError();
    alloc_cache_release(ctx, false);
    e = hipMalloc(d_ptr, bytes);
  }
  if (e != hipSuccess) {
    origin_set_error("hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? ORIGIN_E_NOMEM : ORIGIN_E_HIP;
  }
  if (bytes >= ALLOC_MIN && c->cap_bytes > 0) {
    std::lock_guard<std::mutex> lk(c->mu);
    c->live[*d_ptr] = bytes;
  }
  return ORIGIN_OK;
}

int origin_free(origin_ctx *ctx, void *d_ptr) {
  ORIGIN_USE(ctx);
  if (!d_ptr) return ORIGIN_OK;
  AllocCache *c = ctx->alloc_cache;
  {
    std::unique_lock<std::mutex> lk(c->mu);
    auto it = c->live.find(d_ptr);
    if (it != c->live.end()) {
      const size_t sz = it->second;
      c->live.erase(it);
      if (c->spare_bytes + sz <= c->cap_bytes) {
        // whoever gets the block next uses it behind everything enqueued so far, on any stream
        lk.unlock();
        if (int rc = origin_fork_join(ctx, ctx->aux)) return rc;
        if (int rc = origin_fork_join(ctx, ctx->side)) return rc;
        lk.lock();
        c->spare.emplace(sz, d_ptr);
        c->spare_bytes += sz;
        return ORIGIN_OK;
      }
    }
  }
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  ORIGIN_HIP(hipFree(d_ptr));
  return ORIGIN_OK;
}

int origin_memset(origin_ctx *ctx, void *d_ptr, int byte, size_t bytes) {
  ORIGIN_USE(ctx);
  ORIGIN_HIP(hipMemsetAsync(d_ptr, byte, bytes, ctx->stream));
  return ORIGIN_OK;
}

constexpr size_t STAGED_MIN = (size_t)32 << 20;   // plain copies of at least this go through pinned staging
constexpr size_t STAGED_CH = (size_t)64 << 20;    // bytes per staging buffer
constexpr size_t STAGED_PIECE = (size_t)1 << 20;  // staging bytes per task of the host pool

// The staging buffers: owned by the context (its device, its stream), marked ready only when both
// buffers and both events exist; a partial failure is rolled back.
static int stage_create(origin_ctx *ctx) {
  if (ctx->stage_ready) return ORIGIN_OK;
  char *st[2] = {nullptr, nullptr};
  hipEvent_t ev[2];
  int nev = 0;
  hipError_t e = hipSuccess;
  for (int b = 0; b < 2 && e == hipSuccess; ++b)
    e = hipHostMalloc((void **)&st[b], STAGED_CH, hipHostMallocDefault);
  for (int b = 0; b < 2 && e == hipSuccess; ++b) {
    e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
    if (e == hipSuccess) ++nev;
  }
  for (int b = 0; b < 2 && e == hipSuccess; ++b) e = hipEventRecord(ev[b], ctx->stream);
  if (e != hipSuccess) {
    for (int b = 0; b < nev; ++b) (void)hipEventDestroy(ev[b]);
    for (int b = 0; b < 2; ++b)
      if (st[b]) (void)hipHostFree(st[b]);
    origin_set_error("conversion staging: %s", hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? ORIGIN_E_NOMEM : ORIGIN_E_HIP;
  }
  for (int b = 0; b < 2; ++b) ctx->stage_buf[b] = st[b], ctx->stage_ev[b] = ev[b];
  ctx->stage_ready = true;
  return ORIGIN_OK;
}

// What the host pool does to a piece of n elements between the caller's pages and a staging buffer.
typedef void (*StagePiece)(void *__restrict__ dst, const void *__restrict__ src, size_t n);
static void piece_copy(void *__restrict__ dst, const void *__restrict__ src, size_t n) {
  memcpy(dst, src, n);
}
static void piece_widen(void *__restrict__ dst, const void *__restrict__ src, size_t n) {
  for (size_t i = 0; i < n; ++i) ((double *)dst)[i] = (double)((const float *)src)[i];
}
static void piece_narrow(void *__restrict__ dst, const void *__restrict__ src, size_t n) {
  for (size_t i = 0; i < n; ++i) ((float *)dst)[i] = (float)((const double *)src)[i];
}

// the m elements of a chunk, spread over the host pool in pieces of `per` elements
static void stage_pieces(StagePiece piece, char *dst, size_t dst_el, const char *src, size_t src_el,
                         size_t m, size_t per) {
  origin_host_pool_run((int)((m + per - 1) / per), [&](int p) {
    const size_t a = (size_t)p * per, b = std::min(m, a + per);
    piece(dst + a * dst_el, src + a * src_el, b - a);
  });
}

// Large copies between pageable host memory and the device, in 64 MiB chunks through the context's
// two pinned staging buffers, with the host side of every chunk -- `piece` between the caller's
// pages and the staging buffer, over elements of host_el bytes there and dev_el bytes on the
// device -- spread over the host worker pool while the other buffer is on the bus.  A pageable
// hipMemcpy does its memcpy on one runtime thread: 21-30 GB/s, and 22 GB/s into a fresh
// destination whose pages fault one by one (tools/pagefault_probe.py); this reaches 45 GB/s into
// fresh pages.  The conversions replace a single-threaded astype on top of that.
static int staged_h2d(origin_ctx *ctx, char *d_dst, const char *h_src, size_t n, size_t dev_el,
                      size_t host_el, StagePiece piece) {
  char *const *stage = ctx->stage_buf;
  hipEvent_t *ev = ctx->stage_ev;
  const size_t CH = STAGED_CH / dev_el;
  const size_t nch = (n + CH - 1) / CH;
  for (size_t c = 0; c < nch; ++c) {
    const size_t o = c * CH, m = std::min(CH, n - o);
    ORIGIN_HIP(hipEventSynchronize(ev[c & 1]));  // the copy that last read this buffer is done
    stage_pieces(piece, stage[c & 1], dev_el, h_src + o * host_el, host_el, m, STAGED_PIECE / dev_el);
    ORIGIN_HIP(hipMemcpyAsync(d_dst + o * dev_el, stage[c & 1], m * dev_el, hipMemcpyHostToDevice,
                              ctx->stream));
    ORIGIN_HIP(hipEventRecord(ev[c & 1], ctx->stream));
  }
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

// (while chunk c + 1 is in flight the host pool works on chunk c)
static int staged_d2h(origin_ctx *ctx, char *h_dst, const char *d_src, size_t n, size_t dev_el,
                      size_t host_el, StagePiece piece) {
  char *const *stage = ctx->stage_buf;
  hipEvent_t *ev = ctx->stage_ev;
  const size_t CH = STAGED_CH / dev_el;
  const size_t nch = (n + CH - 1) / CH;
  ORIGIN_HIP(hipEventSynchronize(ev[0]));  // (an upload may still be reading the buffers)
  ORIGIN_HIP(hipEventSynchronize(ev[1]));
  auto issue = [&](size_t c) -> int {
    const size_t o = c * CH, m = std::min(CH, n - o);
    ORIGIN_HIP(hipMemcpyAsync(stage[c & 1], d_src + o * dev_el, m * dev_el, hipMemcpyDeviceToHost,
                              ctx->stream));
    ORIGIN_HIP(hipEventRecord(ev[c & 1], ctx->stream));
    return ORIGIN_OK;
  };
  int rc = issue(0);
  if (rc) return rc;
  for (size_t c = 0; c < nch; ++c) {
    ORIGIN_HIP(hipEventSynchronize(ev[c & 1]));
    if (c + 1 < nch && (rc = issue(c + 1))) return rc;
    const size_t o = c * CH, m = std::min(CH, n - o);
    stage_pieces(piece, h_dst + o * host_el, host_el, stage[c & 1], dev_el, m, STAGED_PIECE / dev_el);
  }
  return ORIGIN_OK;
}

// a large destination is usually a fresh np.empty: every 4 KiB page of it faults on its first
// write (23 against 56 GB/s for a pageable copy of 1.3 GB, tools/pagefault_probe.py).  Ask for
// transparent huge pages on the part that covers whole 2 MiB pages -- a hint, ignored where the
// system does not offer them
static void hint_huge_pages(void *dst, size_t bytes) {
  if (bytes < ((size_t)8 << 20)) return;
  const uintptr_t m = ((uintptr_t)2 << 20) - 1;
  const uintptr_t a = ((uintptr_t)dst + m) & ~m, b = ((uintptr_t)dst + bytes) & ~m;
  if (b > a) (void)madvise((void *)a, (size_t)(b - a), MADV_HUGEPAGE);
}

int origin_h2d(origin_ctx *ctx, void *d_dst, const void *h_src, size_t bytes) {
  ORIGIN_USE(ctx);
  if (bytes == 0) return ORIGIN_OK;
  if (bytes >= STAGED_MIN) {
    if (int rc = stage_create(ctx)) return rc;
    return staged_h2d(ctx, (char *)d_dst, (const char *)h_src, bytes, 1, 1, piece_copy);
  }
  ORIGIN_HIP(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

// Reads of device arrays by the host first make the main stream wait for pending work of the
// auxiliary stream (cont_dct / ima_dct of origin_dct_cont_std_async: origin_fork_join on ctx->aux):
// a caller that forgot origin_aux_join would otherwise get a half-written array without any error.
int origin_d2h(origin_ctx *ctx, void *h_dst, const void *d_src, size_t bytes) {
  ORIGIN_USE(ctx);
  if (bytes == 0) return ORIGIN_OK;
  if (int rc = origin_fork_join(ctx, ctx->aux)) return rc;
  hint_huge_pages(h_dst, bytes);
  if (bytes >= STAGED_MIN) {
    if (int rc = stage_create(ctx)) return rc;
    return staged_d2h(ctx, (char *)h_dst, (const char *)d_src, bytes, 1, 1, piece_copy);
  }
  ORIGIN_HIP(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

// Device float32 -> host float64 (the reference's arrays are float64: every cube that leaves
// through the function seam or a LazyCube is widened)
int origin_d2h_f32_as_f64(origin_ctx *ctx, double *h_dst, const float *d_src, size_t n) {
  ORIGIN_USE(ctx);
  if (n == 0) return ORIGIN_OK;
  ORIGIN_CHECK_ARG(h_dst && d_src, "null pointer");
  if (int rc = stage_create(ctx)) return rc;
  if (int rc = origin_fork_join(ctx, ctx->aux)) return rc;
  hint_huge_pages(h_dst, n * sizeof(double));
  return staged_d2h(ctx, (char *)h_dst, (const char *)d_src, n, sizeof(float), sizeof(double),
                    piece_widen);
}

// Host float64 -> device float32 (the reference hands float64 cubes to the function seam)
int origin_h2d_f64_as_f32(origin_ctx *ctx, float *d_dst, const double *h_src, size_t n) {
  ORIGIN_USE(ctx);
  if (n == 0) return ORIGIN_OK;
  ORIGIN_CHECK_ARG(d_dst && h_src, "null pointer");
  if (int rc = stage_create(ctx)) return rc;
  return staged_h2d(ctx, (char *)d_dst, (const char *)h_src, n, sizeof(float), sizeof(double),
                    piece_narrow);
}

int origin_d2d(origin_ctx *ctx, void *d_dst, const void *d_src, size_t bytes) {
  ORIGIN_USE(ctx);
  if (bytes == 0) return ORIGIN_OK;
  ORIGIN_HIP(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return ORIGIN_OK;
}

int origin_copy_box(origin_ctx *ctx, int kind, void *dst, long dst_pitch_y, long dst_pitch_z,
                    const void *src, long src_pitch_y, long src_pitch_z, int nz, int ny,
                    int nx, int elem) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(kind >= 0 && kind <= 2, "kind must be 0 (h2d), 1 (d2h) or 2 (d2d)");
  ORIGIN_CHECK_ARG(elem == 1 || elem == 2 || elem == 4 || elem == 8, "elem must be 1,2,4,8");
  ORIGIN_CHECK_ARG(nz >= 0 && ny >= 0 && nx >= 0, "negative extent");
  ORIGIN_CHECK_ARG(dst_pitch_y >= nx && src_pitch_y >= nx, "row pitch smaller than nx");
  ORIGIN_CHECK_ARG(dst_pitch_z >= dst_pitch_y * (long)(ny > 0 ? 1 : 0) &&
                       src_pitch_z >= src_pitch_y * (long)(ny > 0 ? 1 : 0),
                   "plane pitch smaller than a row");
  if (nz == 0 || ny == 0 || nx == 0) return ORIGIN_OK;
  if (kind == 1) {
    int rca = origin_fork_join(ctx, ctx->aux);
    if (rca) return rca;
  }
  hipMemcpyKind k = kind == 0   ? hipMemcpyHostToDevice
                    : kind == 1 ? hipMemcpyDeviceToHost
                                : hipMemcpyDeviceToDevice;
  if (kind == 2 && nz <= 65535 && ny <= 65535) {
    const long rowbytes = (long)nx * elem;
    const long dpy = dst_pitch_y * elem, dpz = dst_pitch_z * elem;
    const long spy = src_pitch_y * elem, spz = src_pitch_z * elem;
    auto aligned = [&](long a) {
      return ((uintptr_t)dst % a) == 0 && ((uintptr_t)src % a) == 0 && rowbytes % a == 0 &&
             dpy % a == 0 && dpz % a == 0 && spy % a == 0 && spz % a == 0;
    };
    const int vec = aligned(16) ? 16 : aligned(4) ? 4 : 1;
    dim3 grid((unsigned)((rowbytes / vec + 255) / 256), ny, nz);
    hipLaunchKernelGGL(copy_box_kernel, grid, dim3(256), 0, ctx->stream, (char *)dst, dpy, dpz,
                       (const char *)src, spy, spz, ny, rowbytes, vec);
    ORIGIN_LAUNCH_CHECK();
    return ORIGIN_OK;
  }
  // one 2-D copy per plane: rows of nx*elem bytes at the given pitches
  for (int z = 0; z < nz; ++z) {
    const char *s = (const char *)src + (size_t)z * src_pitch_z * elem;
    char *d = (char *)dst + (size_t)z * dst_pitch_z * elem;
    ORIGIN_HIP(hipMemcpy2DAsync(d, (size_t)dst_pitch_y * elem, s, (size_t)src_pitch_y * elem,
                                (size_t)nx * elem, ny, k, ctx->stream));
  }
  if (kind != 2) ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

int origin_timer_start(origin_ctx *ctx, int slot) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(slot >= 0 && slot < ORIGIN_TIMER_SLOTS, "timer slot out of range");
  if (!ctx->ev_made[slot]) {
    ORIGIN_HIP(hipEventCreate(&ctx->ev_start[slot]));
    ORIGIN_HIP(hipEventCreate(&ctx->ev_stop[slot]));
    ctx->ev_made[slot] = true;
  }
  ORIGIN_HIP(hipEventRecord(ctx->ev_start[slot], ctx->stream));
  return ORIGIN_OK;
}

int origin_timer_stop(origin_ctx *ctx, int slot) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(slot >= 0 && slot < ORIGIN_TIMER_SLOTS && ctx->ev_made[slot], "timer slot not started");
  ORIGIN_HIP(hipEventRecord(ctx->ev_stop[slot], ctx->stream));
  return ORIGIN_OK;
}

int origin_timer_ms(origin_ctx *ctx, int slot, float *ms) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(slot >= 0 && slot < ORIGIN_TIMER_SLOTS && ctx->ev_made[slot] && ms, "timer slot not started");
  ORIGIN_HIP(hipEventSynchronize(ctx->ev_stop[slot]));
  ORIGIN_HIP(hipEventElapsedTime(ms, ctx->ev_start[slot], ctx->ev_stop[slot]));
  return ORIGIN_OK;
}

}  // extern "C"
