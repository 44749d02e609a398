// Fixed-radius matching of two point lists -- DESIGN.md section 3l.
//
// "Is there a point of B within r of this point of A" is what the reference asks of two cKDTrees
// and query_ball_tree in two places: compute_true_purity (lib_origin.py:2383-2399: the local
// maxima above a threshold against the lines of a reference catalogue, once per threshold) and
// Detection.run (steps.py:983-992: the std detections against the correl detections).  Here it is
// one call on two host tables.
//
// The predicate is part of the interface (include/origin_hip.h): d2 = (dx*dx + dy*dy) + dz*dz with
// every difference, product and sum a separately rounded float64 operation in this order, compared
// with r2 = r*r rounded once on the host.  That is what NumPy evaluates; no FMA is formed
// (contraction is off: see dist2).
//
// Binning: 3-D cells over the joint bounding box of A and B (reference lines may lie outside the
// field or at negative pixel coordinates, so the cube's shape is not used).  3-D cells rather than
// (y, x) cells with members ordered by z: a bright source puts hundreds of detections into one
// spaxel column, and with cells cut along z as well a query sees only the members within 2 sides of
// its own z without any ordering inside a cell -- slot order inside a cell comes from atomics and
// nothing depends on it.  The cells of one (z, y) row are consecutive, so are their slots: a query
// reads 9 slot ranges, not 27.
//
// Cell side h >= r * (1 + 2^-20), and the cell of a coordinate c on an axis is
// floor(fl(fl(c - lo) / h)) clamped to [0, cells - 1].  A pair that passes the predicate has
// |a - b| <= r * (1 + 4u) on every axis (u = 2^-53: the rounding of the difference, the square and
// the two sums, all of non-negative terms).  The two quotients carry a relative error of at most
// 2u + u^2 each and are at most the number of cells of the axis, <= 2^20, so they differ by at
// most (1 + 4u) / (1 + 2^-20) + 2^20 * 5u < 1 - 2^-21 + 2^-30 < 1: the floors differ by at most
// one, and clamping is monotone.  So every pair within r lies in neighbouring cells, whatever the
// rounding of the bin index does.  The number of cells is capped (MT_MAX_CELLS, and twice the
// number of B points): the side grows when the box is large or r is tiny, and when r exceeds the
// box there is one cell.
//
// Launch sequence of one call (every loop is bounded by n, m or a cell's size; no workgroup waits
// for another; plain vector stores and integer atomics only):
//   bin     histogram of B per cell, exclusive scan (origin_scan_kernel), scatter of B's
//           coordinates and row numbers into cell order with a cursor per cell
//   query   one lane per point of A walks the 3 x 3 rows of cells around its own: a_hit is a plain
//           store by that lane, b_hit an atomicOr into a bit per B row, b_max an atomicMax on an
//           integer key that orders like the float (as sparse_zmax_kernel); neither depends on the
//           order of arrival, so the outputs are the same from run to run
//           (with a_hit alone asked for, a lane stops at its first partner)
#pragma clang fp contract(off)
#include <cmath>

#include "common.h"

namespace {

constexpr int MT_BLOCK = 256;
constexpr int MT_SCAN = 1024;
constexpr long MT_MAX_CELLS = 1l << 20;
constexpr int MT_KEY_NEG_INF = (int)0x807fffffu;  // fkey(-inf)

// floats as integers that order like them (negative floats: the magnitude bits flipped)
__host__ __device__ __forceinline__ int fkey_bits(int b) { return b >= 0 ? b : b ^ 0x7fffffff; }

struct Grid {
  double lo[3], h;
  int nc[3];  // cells along x, y, z
};

// The predicate's left-hand side.  Plain operators under the file's contract(off): the
// __dmul_rn / __dadd_rn of the HIP headers are inline products and sums compiled with the headers'
// own contraction setting, and fuse once inlined.
__device__ __forceinline__ double dist2(double dx, double dy, double dz) {
#pragma clang fp contract(off)
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ int cell_axis(double c, double lo, double h, int n) {
#pragma clang fp contract(off)
  const double t = (c - lo) / h;
  if (!(t > 0.0)) return 0;
  if (t >= (double)n) return n - 1;
  return (int)t;
}

__device__ __forceinline__ int aload(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------ bin
__global__ __launch_bounds__(MT_BLOCK) void hist_kernel(int m, const double *bx, const double *by,
                                                        const double *bz, Grid g, int *key,
                                                        int *cnt) {
  for (int j = blockIdx.x * MT_BLOCK + threadIdx.x; j < m; j += gridDim.x * MT_BLOCK) {
    const int cx = cell_axis(bx[j], g.lo[0], g.h, g.nc[0]);
    const int cy = cell_axis(by[j], g.lo[1], g.h, g.nc[1]);
    const int cz = cell_axis(bz[j], g.lo[2], g.h, g.nc[2]);
    const int k = (cz * g.nc[1] + cy) * g.nc[0] + cx;
    key[j] = k;
    atomicAdd(&cnt[k], 1);
  }
}

__global__ __launch_bounds__(MT_BLOCK) void scatter_kernel(int m, const double *bx,
                                                           const double *by, const double *bz,
                                                           const int *key, int *cursor, double *sx,
                                                           double *sy, double *sz, int *sj) {
  for (int j = blockIdx.x * MT_BLOCK + threadIdx.x; j < m; j += gridDim.x * MT_BLOCK) {
    const int p = atomicAdd(&cursor[key[j]], 1);
    sx[p] = bx[j], sy[p] = by[j], sz[p] = bz[j], sj[p] = j;
  }
}

// ---------------------------------------------------------------------------------------- query
struct QueryArgs {
  int n;
  const double *ax, *ay, *az;
  const float *aval;  // or null
  Grid g;
  double r2;
  const int *start;
  const double *sx, *sy, *sz;
  const int *sj;
  uint8_t *ahit;    // [n] or null
  unsigned *bbits;  // [cdiv(m, 32)] or null
  int *bkey;        // [m] or null (with aval)
};

__global__ __launch_bounds__(MT_BLOCK) void query_kernel(QueryArgs a) {
  const int nx = a.g.nc[0], ny = a.g.nc[1], nz = a.g.nc[2];
  for (int i = blockIdx.x * MT_BLOCK + threadIdx.x; i < a.n; i += gridDim.x * MT_BLOCK) {
    const double x = a.ax[i], y = a.ay[i], z = a.az[i];
    const int cx = cell_axis(x, a.g.lo[0], a.g.h, nx);
    const int cy = cell_axis(y, a.g.lo[1], a.g.h, ny);
    const int cz = cell_axis(z, a.g.lo[2], a.g.h, nz);
    const int vkey = a.bkey ? fkey_bits(__float_as_int(a.aval[i])) : 0;
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, nx - 1);
    int hit = 0, done = 0;  // done: a_hit alone is asked for and the first partner was found
    for (int qz = max(cz - 1, 0); qz <= min(cz + 1, nz - 1) && !done; ++qz)
      for (int qy = max(cy - 1, 0); qy <= min(cy + 1, ny - 1) && !done; ++qy) {
        const int row = (qz * ny + qy) * nx;
        const int p0 = a.start[row + x0], p1 = a.start[row + x1 + 1];
        for (int p = p0; p < p1 && !done; ++p) {
          if (!(dist2(x - a.sx[p], y - a.sy[p], z - a.sz[p]) <= a.r2)) continue;
          hit = 1;
          done = !a.bbits && !a.bkey;
          const int j = a.sj[p];
          // both words only ever grow: a stale read can only lead to an atomic too many
          if (a.bbits) {
            const unsigned bit = 1u << (j & 31);
            if (!((unsigned)aload((const int *)a.bbits + (j >> 5)) & bit))
              atomicOr(&a.bbits[j >> 5], bit);
          }
          if (a.bkey && aload(a.bkey + j) < vkey) atomicMax(&a.bkey[j], vkey);
        }
      }
    if (a.ahit) a.ahit[i] = (uint8_t)hit;
  }
}

// ------------------------------------------------------------------------------------ host side
inline int grid_for(long n) {
  return (int)std::max(1l, std::min((n + MT_BLOCK - 1) / MT_BLOCK, 4096l));
}

#define MT_LAUNCH(kernel, grid, block, ...)                                          \
  do {                                                                               \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, ctx->stream, __VA_ARGS__); \
    ORIGIN_LAUNCH_CHECK();                                                           \
  } while (0)

// The cells for the box [lo, hi] of both lists: side h >= r * (1 + 2^-20), at most `cap` cells.
// An axis whose extent is not a finite number has one cell.
Grid choose_grid(const double lo[3], const double hi[3], double r, long cap) {
  Grid g;
  double ext[3], emax = 0.0;
  for (int k = 0; k < 3; ++k) {
    g.lo[k] = lo[k];
    ext[k] = hi[k] - lo[k];
    if (!std::isfinite(ext[k]) || !(ext[k] > 0.0)) ext[k] = 0.0;
    emax = std::max(emax, ext[k]);
  }
  double h = r * (1.0 + 0x1p-20);
  h = std::max(h, emax / (double)cap);
  if (!(h > 0.0)) h = 1.0;
  bool fits = false;
  for (int it = 0; it < 1024 && !fits; ++it) {  // (cells <= (cap + 1)^3 and shrink every round)
    double cells = 1.0;
    for (int k = 0; k < 3; ++k) cells *= std::floor(ext[k] / h) + 1.0;
    fits = cells <= (double)cap;
    if (!fits) h *= 1.25;
  }
  g.h = h;
  for (int k = 0; k < 3; ++k) g.nc[k] = fits ? (int)std::floor(ext[k] / h) + 1 : 1;
  return g;
}

// finite coordinates; widens [lo, hi]
int check_points(const char *name, long n, const double *const c[3], double lo[3], double hi[3]) {
  for (int k = 0; k < 3; ++k)
    for (long i = 0; i < n; ++i) {
      const double v = c[k][i];
      ORIGIN_CHECK_ARG(std::isfinite(v), "point %ld of %s has a coordinate that is not finite",
                       i, name);
      lo[k] = std::min(lo[k], v), hi[k] = std::max(hi[k], v);
    }
  return ORIGIN_OK;
}

}  // namespace

extern "C" {

int origin_ball_match(origin_ctx *ctx, long n, const double *h_ax, const double *h_ay,
                      const double *h_az, const float *h_aval, long m, const double *h_bx,
                      const double *h_by, const double *h_bz, double r, uint8_t *h_a_hit,
                      uint8_t *h_b_hit, float *h_b_max) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(n >= 0 && n < (1l << 30) && m >= 0 && m < (1l << 30), "n or m out of range");
  ORIGIN_CHECK_ARG(std::isfinite(r) && r >= 0.0, "the radius must be finite and not negative");
  ORIGIN_CHECK_ARG(!h_b_max || h_aval, "b_max needs a_val");
  ORIGIN_CHECK_ARG(n == 0 || (h_ax && h_ay && h_az), "null pointer (A)");
  ORIGIN_CHECK_ARG(m == 0 || (h_bx && h_by && h_bz), "null pointer (B)");
  const double *const A[3] = {h_ax, h_ay, h_az}, *const B[3] = {h_bx, h_by, h_bz};
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int rc;
  if ((rc = check_points("A", n, A, lo, hi)) || (rc = check_points("B", m, B, lo, hi))) return rc;
  if (h_aval)
    for (long i = 0; i < n; ++i)
      ORIGIN_CHECK_ARG(!std::isnan(h_aval[i]), "a_val[%ld] is NaN", i);
  if (n == 0 || m == 0) {
    if (h_a_hit) memset(h_a_hit, 0, (size_t)n);
    if (h_b_hit) memset(h_b_hit, 0, (size_t)m);
    if (h_b_max) std::fill(h_b_max, h_b_max + m, -INFINITY);
    return ORIGIN_OK;
  }
  const int N = (int)n, M = (int)m, W = cdiv(m, 32);
  const bool want_b = h_b_hit || h_b_max;
  const Grid g = choose_grid(lo, hi, r, std::min(MT_MAX_CELLS, std::max(64l, 2 * m)));
  const int C = g.nc[0] * g.nc[1] * g.nc[2];

  DevMem mem(ctx);
  double *ax, *ay, *az, *bx, *by, *bz, *sx, *sy, *sz;
  float *aval;
  int *key, *start, *cursor, *sj, *bkey;
  unsigned *bbits;
  uint8_t *ahit;
  rc = carve_block(ctx, mem, [&](Carver &c) {
    ax = c.take<double>(N), ay = c.take<double>(N), az = c.take<double>(N);
    bx = c.take<double>(M), by = c.take<double>(M), bz = c.take<double>(M);
    sx = c.take<double>(M), sy = c.take<double>(M), sz = c.take<double>(M);
    aval = c.take<float>(h_b_max ? N : 0);
    key = c.take<int>(M), sj = c.take<int>(M);
    start = c.take<int>(C + 1), cursor = c.take<int>(C + 1);
    bkey = c.take<int>(h_b_max ? M : 0), bbits = c.take<unsigned>(want_b ? W : 0);
    ahit = c.take<uint8_t>(h_a_hit ? N : 0);
  });
  if (rc) return rc;
  const size_t na = (size_t)N * sizeof(double), nb = (size_t)M * sizeof(double);
  if ((rc = origin_h2d(ctx, ax, h_ax, na)) || (rc = origin_h2d(ctx, ay, h_ay, na)) ||
      (rc = origin_h2d(ctx, az, h_az, na)) || (rc = origin_h2d(ctx, bx, h_bx, nb)) ||
      (rc = origin_h2d(ctx, by, h_by, nb)) || (rc = origin_h2d(ctx, bz, h_bz, nb)))
    return rc;
  if (h_b_max && (rc = origin_h2d(ctx, aval, h_aval, (size_t)N * sizeof(float)))) return rc;
  {
    ProfScope ps(ctx, K_MATCH_BIN);
    ORIGIN_HIP(hipMemsetAsync(start, 0, (size_t)(C + 1) * sizeof(int), ctx->stream));
    MT_LAUNCH(hist_kernel, grid_for(M), MT_BLOCK, M, bx, by, bz, g, key, start);
    MT_LAUNCH(origin_scan_kernel<MT_SCAN>, 1, MT_SCAN, C, start);
    ORIGIN_HIP(hipMemcpyAsync(cursor, start, (size_t)(C + 1) * sizeof(int),
                              hipMemcpyDeviceToDevice, ctx->stream));
    MT_LAUNCH(scatter_kernel, grid_for(M), MT_BLOCK, M, bx, by, bz, key, cursor, sx, sy, sz, sj);
  }
  {
    ProfScope ps(ctx, K_MATCH_QUERY);
    if (want_b) ORIGIN_HIP(hipMemsetAsync(bbits, 0, (size_t)W * sizeof(unsigned), ctx->stream));
    if (h_b_max)
      ORIGIN_HIP(hipMemsetD32Async((hipDeviceptr_t)bkey, MT_KEY_NEG_INF, (size_t)M, ctx->stream));
    QueryArgs q = {N,  ax, ay, az, h_b_max ? aval : nullptr, g, r * r, start, sx, sy, sz, sj,
                   h_a_hit ? ahit : nullptr, want_b ? bbits : nullptr, h_b_max ? bkey : nullptr};
    MT_LAUNCH(query_kernel, grid_for(N), MT_BLOCK, q);
  }
  if (h_a_hit && (rc = origin_d2h(ctx, h_a_hit, ahit, (size_t)N))) return rc;
  if (want_b) {
    std::vector<unsigned> bits(W);
    if ((rc = origin_d2h(ctx, bits.data(), bbits, (size_t)W * sizeof(unsigned)))) return rc;
    if (h_b_hit)
      for (long j = 0; j < m; ++j) h_b_hit[j] = (bits[j >> 5] >> (j & 31)) & 1u;
    if (h_b_max) {
      std::vector<int> keys(M);
      if ((rc = origin_d2h(ctx, keys.data(), bkey, (size_t)M * sizeof(int)))) return rc;
      for (long j = 0; j < m; ++j) {
        // (a row nobody reached keeps the key of -inf; the flip is its own inverse)
        const bool hit = (bits[j >> 5] >> (j & 31)) & 1u;
        const int b = fkey_bits(hit ? keys[j] : MT_KEY_NEG_INF);
        memcpy(&h_b_max[j], &b, sizeof(float));
      }
    }
  }
  return origin_sync(ctx);
}

}  // extern "C"
