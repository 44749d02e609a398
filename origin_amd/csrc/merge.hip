// Spatio-spectral merging of step 7 (reference lib_origin.py:1259-1387: itersrc and
// spatiospectral_merging) -- DESIGN.md section 3h.
//
// The reference is a recursive host function that evaluates np.hypot against the whole table for
// every detection it visits.  Restated: seeds are the unmatched rows in
// ascending order; the group of a seed is what a breadth-first walk over *near* steps reaches among
// the rows that are still unmatched and *eligible* for that seed.  Groups never leave a connected
// component of the near graph, so the components run side by side, one workgroup each, and only
// the seed loop inside a component is sequential.  The second stage (groups of one segmap label
// whose lines come within tol_spec of each other) is independent per label: one wave each, the
// z-sets of the groups as bitmaps over Nz and "min |dz| <= dzmax" as "the bitmap dilated by dzmax
// meets the other".
//
// Every predicate is an integer test: the host evaluates np.hypot itself into two small tables
// (near / far over |dx|, |dy| < R) and passes dzmax = ceil(tol_spec) - 1.  There is no floating
// point in this file.
//
// Launch sequence of one call (every kernel loop is bounded by n, the spaxel count, a component's or
// an area's size; no workgroup waits on another):
//   bin         histogram of the rows per spaxel, exclusive scan, scatter (slot order inside a
//               spaxel comes from atomics; nothing below depends on it)
//   components  union-find over the occupied spaxels: hook (atomicMin of the larger root onto the
//               smaller) and compress, repeated while a hook changed something (every such round
//               removes a root: at most n rounds); the host reads the flag
//   (host)      rows ordered by component, largest component first, rows ascending: O(n) bookkeeping
//   stage 1     one workgroup per component: first unmatched member = seed, level-synchronous
//               expansion with the frontier in a global queue segment of the component's size
//   renumber    flag-scan of the seeds, group ids, integer atomicMax of the area per group
//   (host)      groups per area label > 0; labels with one group are done
//   stage 2     bitmaps by atomicOr, then one wave per label walks cu / otg exactly as the reference
#include <algorithm>
#include <climits>
#include <numeric>

#include "common.h"

namespace {

constexpr int MG_BLOCK = 256;
constexpr int MG_SCAN = 1024;
constexpr int MG_MAXR = 64;            // predicate tables up to 64 x 64 (tol_spat up to ~43)
constexpr int MG_S2_LDS = 64 * 1024;   // alive bits of one area's groups

__device__ __forceinline__ int aload(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------ bin
__global__ void hist_kernel(int n, const int *x, const int *y, int Nx, int *key, int *cnt) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const int k = y[r] * Nx + x[r];
    key[r] = k;
    atomicAdd(&cnt[k], 1);
  }
}

__global__ void scatter_kernel(int n, const int *key, int *cursor, int *binrows) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    binrows[atomicAdd(&cursor[key[r]], 1)] = r;
}

// ----------------------------------------------------------------------------------- components
// parent[sp] <= sp for an occupied spaxel (-1 for an empty one): a forest whose roots are the
// smallest spaxel of their tree.
__global__ void parent_init_kernel(int S, const int *start, int *parent, int *complow) {
  for (int sp = blockIdx.x * blockDim.x + threadIdx.x; sp < S; sp += gridDim.x * blockDim.x) {
    parent[sp] = start[sp + 1] > start[sp] ? sp : -1;
    complow[sp] = INT_MAX;
  }
}

__device__ __forceinline__ int find_root(const int *parent, int p, int S) {
  for (int i = 0; i < S; ++i) {  // (parents strictly decrease)
    const int q = aload(parent + p);
    if (q == p) break;
    p = q;
  }
  return p;
}

__global__ void hook_kernel(int Ny, int Nx, int R, int wr, const uint8_t *near_t, int *parent,
                            int *changed) {
  const int S = Ny * Nx;
  for (int sp = blockIdx.x * blockDim.x + threadIdx.x; sp < S; sp += gridDim.x * blockDim.x) {
    if (aload(parent + sp) < 0) continue;
    const int sx = sp % Nx, sy = sp / Nx;
    // the half of the window in front of sp: every edge is seen from its larger end
    for (int dy = -wr; dy <= 0; ++dy)
      for (int dx = -wr; dx <= wr; ++dx) {
        if (dy == 0 && dx >= 0) break;
        if (!near_t[abs(dx) * R + abs(dy)]) continue;
        const int xx = sx + dx, yy = sy + dy;
        if (xx < 0 || xx >= Nx || yy < 0) continue;
        const int nb = yy * Nx + xx;
        if (aload(parent + nb) < 0) continue;
        const int ra = find_root(parent, sp, S), rb = find_root(parent, nb, S);
        if (ra != rb) {
          atomicMin(&parent[max(ra, rb)], min(ra, rb));
          *changed = 1;
        }
      }
  }
}

__global__ void compress_kernel(int S, int *parent) {
  for (int sp = blockIdx.x * blockDim.x + threadIdx.x; sp < S; sp += gridDim.x * blockDim.x)
    if (aload(parent + sp) >= 0) {
      const int r = find_root(parent, sp, S);
      atomicMin(&parent[sp], r);
    }
}

// lowest row of every component, then that label for every row
__global__ void complow_kernel(int n, const int *key, const int *parent, int *complow) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    atomicMin(&complow[parent[key[r]]], r);
}
__global__ void comp_kernel(int n, const int *key, const int *parent, const int *complow,
                            int *comp) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    comp[r] = complow[parent[key[r]]];
}

// -------------------------------------------------------------------------------------- stage 1
struct Stage1Args {
  int nc;                // components, largest first
  const int *comp_off;   // [nc + 1] into members
  const int *members;    // rows of each component, ascending
  const int *x, *y, *z;
  const int *start, *binrows;
  int Ny, Nx, R, wr, dzmax;
  const uint8_t *near_t, *far_t;
  int *imatch;           // -1 = unmatched, else the seed row
  int *queue;            // [n]: a component uses its own members' range
};

__global__ __launch_bounds__(MG_BLOCK) void stage1_kernel(Stage1Args a) {
  __shared__ uint8_t s_near[MG_MAXR * MG_MAXR], s_far[MG_MAXR * MG_MAXR];
  __shared__ int s_first, s_tail;
  const int t = threadIdx.x, R = a.R;
  for (int i = t; i < R * R; i += MG_BLOCK) s_near[i] = a.near_t[i], s_far[i] = a.far_t[i];
  const int win = 2 * a.wr + 1, win2 = win * win;
  for (int c = blockIdx.x; c < a.nc; c += gridDim.x) {
    const int off = a.comp_off[c], m = a.comp_off[c + 1] - off;
    const int *mem = a.members + off;
    int *queue = a.queue + off;
    int tail = 0, base = 0;
    __syncthreads();
    if (t == 0) s_tail = 0;
    // at most cdiv(m, MG_BLOCK) empty chunks and m seeds
    for (long it = 0; it < 2l * m + 2 && base < m; ++it) {
      if (t == 0) s_first = INT_MAX;
      __syncthreads();
      if (base + t < m && aload(a.imatch + mem[base + t]) < 0) atomicMin(&s_first, base + t);
      __syncthreads();
      const int first = s_first;
      if (first == INT_MAX) {
        base += MG_BLOCK;
        __syncthreads();
        continue;
      }
      const int s = mem[first];
      const int xs = a.x[s], ys = a.y[s], zs = a.z[s];
      int head = tail;
      if (t == 0) {
        atomicExch(&a.imatch[s], s);
        queue[tail] = s;
        s_tail = tail + 1;
      }
      __syncthreads();
      for (int lvl = 0; lvl < m; ++lvl) {  // a level takes at least one row off the queue
        const int end = s_tail;
        __syncthreads();
        if (end == head) break;
        const long items = (long)(end - head) * win2;
        for (long w = t; w < items; w += MG_BLOCK) {
          const int row = queue[head + (int)(w / win2)], k = (int)(w % win2);
          const int dx = k % win - a.wr, dy = k / win - a.wr;
          if (!s_near[abs(dx) * R + abs(dy)]) continue;
          const int xx = a.x[row] + dx, yy = a.y[row] + dy;
          if (xx < 0 || xx >= a.Nx || yy < 0 || yy >= a.Ny) continue;
          const int sp = yy * a.Nx + xx;
          const int p0 = a.start[sp], p1 = a.start[sp + 1];
          if (p0 == p1) continue;
          // eligible for the seed: not far from it, or spectrally close
          const int ax = abs(xx - xs), ay = abs(yy - ys);
          const bool far = ax >= R || ay >= R || s_far[ax * R + ay];
          for (int p = p0; p < p1; ++p) {
            const int j = a.binrows[p];
            if (aload(a.imatch + j) >= 0) continue;
            if (far && abs(a.z[j] - zs) > a.dzmax) continue;
            if (atomicCAS(&a.imatch[j], -1, s) == -1) queue[atomicAdd(&s_tail, 1)] = j;
          }
        }
        __syncthreads();
        head = end;
      }
      tail = s_tail;
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------------------------- renumber
__global__ void seed_flag_kernel(int n, const int *imatch, int *rank) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x)
    rank[r] = imatch[r] == r;
}
// pass 0: a seed starts its group's area; pass 1: every row raises it; pass 2: every row takes it
template <int PASS>
__global__ void group_kernel(int n, const int *imatch, const int *rank, const int *area, int *gid,
                             int *garea, int *area_out) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const int im = imatch[r];
    if (im < 0 || im >= n) continue;  // (never: stage 1 matches every row; the host checks gid)
    const int g = rank[im];
    if (PASS == 0) {
      gid[r] = g;
      if (im == r) garea[g] = area[r];
    } else if (PASS == 1) {
      atomicMax(&garea[g], area[r]);
    } else {
      area_out[r] = garea[g];
    }
  }
}

// -------------------------------------------------------------------------------------- stage 2
// B: the channels of a group's rows; D: those channels widened by dzmax on both sides
__global__ void bitmap_kernel(int n, const int *z, const int *rowslot, int Nz, int W, int dzmax,
                              unsigned *B, unsigned *D) {
  for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    const int slot = rowslot[r];
    if (slot < 0) continue;
    const int zc = z[r];
    const size_t o = (size_t)slot * W;
    atomicOr(&B[o + (zc >> 5)], 1u << (zc & 31));
    const int lo = max(0, zc - dzmax), hi = min(Nz - 1, zc + dzmax);
    if (lo > hi) continue;
    for (int w = lo >> 5; w <= (hi >> 5); ++w) {
      const int b0 = max(lo, w * 32) - w * 32, b1 = min(hi, w * 32 + 31) - w * 32;
      const unsigned mask = (b1 - b0 == 31) ? ~0u : (((1u << (b1 - b0 + 1)) - 1u) << b0);
      atomicOr(&D[o + w], mask);
    }
  }
}

// One wave per area label.  Slots aoff[a] .. aoff[a + 1] are the label's groups in ascending id.
// link[slot]: index (inside the area) of the group that absorbed it, itself while alive; root:
// the same followed to the survivor.
__global__ __launch_bounds__(64) void stage2_kernel(const int *aoff, int W, unsigned *B,
                                                    unsigned *D, int *link, int *root) {
  extern __shared__ unsigned s_alive[];
  const int base = aoff[blockIdx.x], k = aoff[blockIdx.x + 1] - base, lane = threadIdx.x;
  for (int w = lane; w < (k + 31) / 32; w += 64) s_alive[w] = ~0u;
  for (int j = lane; j < k; j += 64) link[base + j] = j;
  __syncthreads();
  int nalive = k;
  for (int i = 0; i < k && nalive > 1; ++i) {
    if (!((s_alive[i >> 5] >> (i & 31)) & 1u)) continue;
    unsigned *Bi = B + (size_t)(base + i) * W, *Di = D + (size_t)(base + i) * W;
    for (int j = 0; j < k; ++j) {
      if (j == i || !((s_alive[j >> 5] >> (j & 31)) & 1u)) continue;
      const unsigned *Bj = B + (size_t)(base + j) * W, *Dj = D + (size_t)(base + j) * W;
      int hit = 0;
      for (int w = lane; w < W; w += 64) hit |= (Di[w] & Bj[w]) != 0u;
      if (__ballot(hit) == 0ull) continue;
      for (int w = lane; w < W; w += 64) Bi[w] |= Bj[w], Di[w] |= Dj[w];  // (a lane's own words)
      if (lane == 0) {
        s_alive[j >> 5] &= ~(1u << (j & 31));
        link[base + j] = i;
      }
      --nalive;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int j = lane; j < k; j += 64) {
    int f = j;
    for (int s = 0; s < k; ++s) {
      const int nf = aload(link + base + f);
      if (nf == f) break;
      f = nf;
    }
    root[base + j] = f;
  }
}

// ------------------------------------------------------------------------------------ host side
inline int grid_for(long n) { return (int)std::max(1l, std::min((n + MG_BLOCK - 1) / MG_BLOCK, 4096l)); }

#define MG_LAUNCH(kernel, grid, block, lds, ...)                                   \
  do {                                                                             \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, ctx->stream, __VA_ARGS__); \
    ORIGIN_LAUNCH_CHECK();                                                         \
  } while (0)

// (host) rows ordered by component (a component's label is its lowest row), largest component
// first, rows ascending: `members`, and comp_off[0 .. nc] into it
void order_by_component(const std::vector<int> &comp, std::vector<int> &members,
                        std::vector<int> &comp_off) {
  const int N = (int)comp.size();
  std::vector<int> size(N, 0), order, slot(N);
  for (int r = 0; r < N; ++r) ++size[comp[r]];
  for (int r = 0; r < N; ++r)
    if (size[r]) order.push_back(r);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return size[a] > size[b]; });
  const int nc = (int)order.size();
  comp_off.assign(nc + 1, 0);
  for (int i = 0; i < nc; ++i) slot[order[i]] = i, comp_off[i + 1] = comp_off[i] + size[order[i]];
  std::vector<int> cur(comp_off.begin(), comp_off.end() - 1);
  members.resize(N);
  for (int r = 0; r < N; ++r) members[cur[slot[comp[r]]]++] = r;
}

// (host) groups per area label > 0, labels ascending; a label with one group is done.  slot_group:
// the other labels' groups, aoff[0 .. na] into it; gslot: a group's slot or -1.  Returns kmax,
// the most groups of one label.
int label_groups(int N, const int *gid, const int *area, std::vector<int> &slot_group,
                 std::vector<int> &aoff, std::vector<int> &gslot) {
  int ng = 0;
  for (int r = 0; r < N; ++r) ng = std::max(ng, gid[r] + 1);
  std::vector<int> garea_h(ng, 0), glist;
  for (int r = 0; r < N; ++r) garea_h[gid[r]] = area[r];
  for (int g = 0; g < ng; ++g)
    if (garea_h[g] > 0) glist.push_back(g);
  std::stable_sort(glist.begin(), glist.end(),
                   [&](int a, int b) { return garea_h[a] < garea_h[b]; });
  slot_group.clear(), aoff.assign(1, 0), gslot.assign(ng, -1);
  int kmax = 0;
  for (size_t i = 0; i < glist.size();) {
    size_t j = i;
    while (j < glist.size() && garea_h[glist[j]] == garea_h[glist[i]]) ++j;
    if (j - i > 1) {
      for (size_t q = i; q < j; ++q) gslot[glist[q]] = (int)slot_group.size(), slot_group.push_back(glist[q]);
      aoff.push_back((int)slot_group.size());
      kmax = std::max(kmax, (int)(j - i));
    }
    i = j;
  }
  return kmax;
}

// One call: the sizes, the call's block and stage 2's with their pieces, and one method per stage
// of the launch sequence in the header.
struct MergeRun {
  origin_ctx *ctx;
  const int N, S, Ny, Nx, Nz, R, wr, dzmax;  // wr: half-width of the near window
  const size_t nb;                           // bytes of a column
  const int gn, gs;
  DevMem mem, mem2;
  int *x, *y, *z, *area, *key, *binrows, *start, *cursor, *parent, *complow, *comp, *members,
      *comp_off, *imatch, *queue, *rank, *gid, *garea, *area_out, *flag;
  uint8_t *near_t, *far_t;
  int *d_rowslot, *d_aoff, *link, *root;
  unsigned *B, *D;

  MergeRun(origin_ctx *c, int n, int ny, int nx, int nz, int r, int w, int dz)
      : ctx(c), N(n), S(ny * nx), Ny(ny), Nx(nx), Nz(nz), R(r), wr(w), dzmax(dz),
        nb((size_t)n * sizeof(int)), gn(grid_for(n)), gs(grid_for(ny * nx)), mem(c), mem2(c) {}

  int setup(const int *h_x, const int *h_y, const int *h_z, const int *h_area,
            const uint8_t *h_near, const uint8_t *h_far) {
    int rc = carve_block(ctx, mem, [&](Carver &c) {
      x = c.take<int>(N), y = c.take<int>(N), z = c.take<int>(N), area = c.take<int>(N);
      key = c.take<int>(N), binrows = c.take<int>(N);
      start = c.take<int>(S + 1), cursor = c.take<int>(S + 1);
      parent = c.take<int>(S), complow = c.take<int>(S), comp = c.take<int>(N);
      members = c.take<int>(N), comp_off = c.take<int>(N + 1);
      imatch = c.take<int>(N), queue = c.take<int>(N), rank = c.take<int>(N + 1);
      gid = c.take<int>(N), garea = c.take<int>(N), area_out = c.take<int>(N);
      flag = c.take<int>(1);
      near_t = c.take<uint8_t>(R * R), far_t = c.take<uint8_t>(R * R);
    });
    if (rc) return rc;
    if ((rc = origin_h2d(ctx, x, h_x, nb)) || (rc = origin_h2d(ctx, y, h_y, nb)) ||
        (rc = origin_h2d(ctx, z, h_z, nb)) || (rc = origin_h2d(ctx, area, h_area, nb)) ||
        (rc = origin_h2d(ctx, near_t, h_near, (size_t)R * R)))
      return rc;
    return origin_h2d(ctx, far_t, h_far, (size_t)R * R);
  }

  int bin() {
    ProfScope ps(ctx, K_MERGE_BIN);
    ORIGIN_HIP(hipMemsetAsync(start, 0, (size_t)(S + 1) * sizeof(int), ctx->stream));
    MG_LAUNCH(hist_kernel, gn, MG_BLOCK, 0, N, x, y, Nx, key, start);
    MG_LAUNCH(origin_scan_kernel<MG_SCAN>, 1, MG_SCAN, 0, S, start);
    ORIGIN_HIP(hipMemcpyAsync(cursor, start, (size_t)(S + 1) * sizeof(int),
                              hipMemcpyDeviceToDevice, ctx->stream));
    MG_LAUNCH(scatter_kernel, gn, MG_BLOCK, 0, N, key, cursor, binrows);
    return ORIGIN_OK;
  }

  // components of the near graph; hcomp: the label of every row, a row not above it
  int components(std::vector<int> &hcomp) {
    MG_LAUNCH(parent_init_kernel, gs, MG_BLOCK, 0, S, start, parent, complow);
    int rc, changed = 1;
    for (long round = 0; changed; ++round) {
      if (round > (long)N + 1) {  // (every round that changes something removes a root)
        origin_set_error("component labelling did not converge in %ld rounds", round);
        return ORIGIN_E_STATE;
      }
      {
        ProfScope ps(ctx, K_MERGE_COMP);
        ORIGIN_HIP(hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
        MG_LAUNCH(hook_kernel, gs, MG_BLOCK, 0, Ny, Nx, R, wr, near_t, parent, flag);
        MG_LAUNCH(compress_kernel, gs, MG_BLOCK, 0, S, parent);
      }
      if ((rc = origin_d2h(ctx, &changed, flag, sizeof(int)))) return rc;
    }
    {
      ProfScope ps(ctx, K_MERGE_COMP);
      MG_LAUNCH(complow_kernel, gn, MG_BLOCK, 0, N, key, parent, complow);
      MG_LAUNCH(comp_kernel, gn, MG_BLOCK, 0, N, key, parent, complow, comp);
    }
    hcomp.resize(N);
    if ((rc = origin_d2h(ctx, hcomp.data(), comp, nb))) return rc;
    for (int r = 0; r < N; ++r)
      if (hcomp[r] < 0 || hcomp[r] > r) {
        origin_set_error("component label %d of row %d is not a lower row", hcomp[r], r);
        return ORIGIN_E_STATE;
      }
    return ORIGIN_OK;
  }

  int stage1(const std::vector<int> &h_members, const std::vector<int> &h_comp_off) {
    const int nc = (int)h_comp_off.size() - 1;
    int rc;
    if ((rc = put(ctx, members, h_members)) || (rc = put(ctx, comp_off, h_comp_off))) return rc;
    ProfScope ps(ctx, K_MERGE_STAGE1);
    ORIGIN_HIP(hipMemsetAsync(imatch, 0xff, nb, ctx->stream));
    Stage1Args a = {nc, comp_off, members, x, y, z, start, binrows, Ny, Nx, R, wr, dzmax,
                    near_t, far_t, imatch, queue};
    MG_LAUNCH(stage1_kernel, std::min(nc, 4 * std::max(ctx->num_cu, 1)), MG_BLOCK, 0, a);
    return ORIGIN_OK;
  }

  // rank of the seed among the seeds = group id, the group's largest area
  int renumber(int *h_gid, int *h_area_out) {
    {
      ProfScope ps(ctx, K_MERGE_RENUMBER);
      ORIGIN_HIP(hipMemsetAsync(gid, 0xff, nb, ctx->stream));
      MG_LAUNCH(seed_flag_kernel, gn, MG_BLOCK, 0, N, imatch, rank);
      MG_LAUNCH(origin_scan_kernel<MG_SCAN>, 1, MG_SCAN, 0, N, rank);
      MG_LAUNCH(group_kernel<0>, gn, MG_BLOCK, 0, N, imatch, rank, area, gid, garea, area_out);
      MG_LAUNCH(group_kernel<1>, gn, MG_BLOCK, 0, N, imatch, rank, area, gid, garea, area_out);
      MG_LAUNCH(group_kernel<2>, gn, MG_BLOCK, 0, N, imatch, rank, area, gid, garea, area_out);
    }
    int rc;
    if ((rc = origin_d2h(ctx, h_gid, gid, nb)) || (rc = origin_d2h(ctx, h_area_out, area_out, nb)))
      return rc;
    for (int r = 0; r < N; ++r)
      if (h_gid[r] < 0 || h_gid[r] > r) {
        origin_set_error("row %d was left without a group", r);
        return ORIGIN_E_STATE;
      }
    return ORIGIN_OK;
  }

  // the slots' groups that merge; h_imatch: a row's group, replaced by the group's survivor
  int stage2(const std::vector<int> &slot_group, const std::vector<int> &aoff,
             const std::vector<int> &gslot, int kmax, const int *h_gid, int *h_imatch) {
    const int na = (int)aoff.size() - 1, nslots = (int)slot_group.size();
    const size_t lds = (size_t)((kmax + 31) / 32) * sizeof(unsigned);
    ORIGIN_CHECK_ARG(lds <= MG_S2_LDS, "an area label holds %d groups (limit %d)", kmax,
                     MG_S2_LDS * 8);
    const int W = (Nz + 31) / 32;
    std::vector<int> rowslot(N), root_h(nslots);
    for (int r = 0; r < N; ++r) rowslot[r] = gslot[h_gid[r]];
    int rc = carve_block(ctx, mem2, [&](Carver &c) {
      d_rowslot = c.take<int>(N), d_aoff = c.take<int>(na + 1);
      link = c.take<int>(nslots), root = c.take<int>(nslots);
      B = c.take<unsigned>((size_t)nslots * W), D = c.take<unsigned>((size_t)nslots * W);
    });
    if (rc) return rc;
    if ((rc = put(ctx, d_rowslot, rowslot)) || (rc = put(ctx, d_aoff, aoff))) return rc;
    {
      ProfScope ps(ctx, K_MERGE_STAGE2);
      // (B and D are adjacent pieces of one block)
      ORIGIN_HIP(hipMemsetAsync(B, 0, (size_t)((char *)D - (char *)B) + (size_t)nslots * W * sizeof(unsigned),
                                ctx->stream));
      MG_LAUNCH(bitmap_kernel, gn, MG_BLOCK, 0, N, z, d_rowslot, Nz, W, dzmax, B, D);
      MG_LAUNCH(stage2_kernel, na, 64, lds, d_aoff, W, B, D, link, root);
    }
    if ((rc = origin_d2h(ctx, root_h.data(), root, (size_t)nslots * sizeof(int)))) return rc;
    std::vector<int> final_gid(nslots);  // a slot's survivor, as a group id
    for (int a = 0; a < na; ++a)
      for (int s = aoff[a]; s < aoff[a + 1]; ++s) {
        if (root_h[s] < 0 || root_h[s] >= aoff[a + 1] - aoff[a]) {
          origin_set_error("spectral stage: group slot %d has no survivor", s);
          return ORIGIN_E_STATE;
        }
        final_gid[s] = slot_group[aoff[a] + root_h[s]];
      }
    for (int r = 0; r < N; ++r)
      if (rowslot[r] >= 0) h_imatch[r] = final_gid[rowslot[r]];
    return ORIGIN_OK;
  }
};

}  // namespace

extern "C" {

int origin_merge_detections(origin_ctx *ctx, long n, const int *h_x, const int *h_y, const int *h_z,
                            const int *h_area, int Ny, int Nx, int Nz, int R,
                            const uint8_t *h_near, const uint8_t *h_far, int dzmax, int *h_comp,
                            int *h_area_out, int *h_imatch2, int *h_imatch) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(n >= 0 && n < (1l << 30), "n out of range");
  if (n == 0) return ORIGIN_OK;
  ORIGIN_CHECK_ARG(h_x && h_y && h_z && h_area && h_near && h_far && h_area_out && h_imatch2 &&
                       h_imatch,
                   "null pointer");
  ORIGIN_CHECK_ARG(Ny > 0 && Nx > 0 && Nz > 0 && (long)Ny * Nx < (1l << 30), "bad cube shape");
  ORIGIN_CHECK_ARG(R >= 1 && R <= MG_MAXR, "predicate tables must be between 1 and %d wide",
                   MG_MAXR);
  ORIGIN_CHECK_ARG(h_near[0], "tol_spat must be positive (a detection is near itself)");
  for (long r = 0; r < n; ++r)
    ORIGIN_CHECK_ARG(h_x[r] >= 0 && h_x[r] < Nx && h_y[r] >= 0 && h_y[r] < Ny && h_z[r] >= 0 &&
                         h_z[r] < Nz,
                     "detection %ld lies outside the (%d, %d, %d) cube", r, Nz, Ny, Nx);
  dzmax = std::max(-1, std::min(dzmax, Nz));
  int wr = 0;  // half-width of the near window
  for (int a = 0; a < R; ++a)
    for (int b = 0; b < R; ++b)
      if (h_near[a * R + b]) wr = std::max(wr, std::max(a, b));
  MergeRun run(ctx, (int)n, Ny, Nx, Nz, R, wr, dzmax);
  std::vector<int> hcomp, members, comp_off, slot_group, aoff, gslot;
  int rc;
  if ((rc = run.setup(h_x, h_y, h_z, h_area, h_near, h_far)) || (rc = run.bin()) ||
      (rc = run.components(hcomp)))
    return rc;
  if (h_comp) memcpy(h_comp, hcomp.data(), run.nb);
  order_by_component(hcomp, members, comp_off);
  if ((rc = run.stage1(members, comp_off)) || (rc = run.renumber(h_imatch2, h_area_out))) return rc;
  memcpy(h_imatch, h_imatch2, run.nb);
  const int kmax = label_groups(run.N, h_imatch2, h_area_out, slot_group, aoff, gslot);
  if (aoff.size() == 1) return ORIGIN_OK;  // every label has one group
  return run.stage2(slot_group, aoff, gslot, kmax, h_imatch2, h_imatch);
}

}  // extern "C"
