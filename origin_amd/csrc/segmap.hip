// Segmentation maps of steps 1 and 6 (reference lib_origin.py:243-280, compute_segmap_gauss, and
// the two ndi.label calls on unions of label maps, steps.py:487 and :869) -- DESIGN.md section 3k.
//
// The reference thresholds a float64 map, erodes and dilates the mask once with the 4-neighbour
// cross (scipy binary_erosion with border_value=1, binary_dilation with border 0), widens it with a
// disc through fftconvolve, and numbers the 4-connected components with ndi.label.  Everything here
// is a comparison or an integer operation; results are bit-identical to the host code.
//
// The one place where the device evaluates directly what the reference evaluates through an FFT:
// `fftconvolve(mask, disc, 'same') > 1e-9` with disc = (hypot(dy, dx) < f), f = int(fwhm) // 2.  The
// exact convolution of two 0/1 images is an integer count, 0 or >= 1, and the FFT's rounding error
// (3e-15 at 600 x 600) lies six orders below the 1e-9 cut, so the result is "some mask pixel lies at
// an integer offset with dy^2 + dx^2 < f^2", outside the image counting as 0.  disc_kernel loops over
// those offsets.  f = 0 has no offset and gives the empty mask (the reference's all-False disc does
// the same), f = 1 is the identity.
//
// Labels: 1..n in raster order of each component's first pixel (its smallest flat index), which is
// scipy.ndimage.label's numbering.  A forest over the pixels, parent[p] <= p inside a component
// (-1 for background), is only ever changed by hooking a larger root under a smaller index
// (atomicMin), so the final root of a component is its smallest flat index whatever the order of
// the atomics: the labels are the same from run to run.
//
// Launch sequence of origin_segmap_label (all on the context's main stream; no workgroup or thread
// waits for another, there is no flag to spin on and no host round trip before the final count):
//   tile     one workgroup per 32 x 32 tile: union-find in LDS (a pixel starts at the first pixel of
//            its horizontal run, then unites with the pixel above), parent[p] = flat global index
//            of the tile-local root
//   seam     one thread per pixel pair facing each other across a tile edge: unite their trees
//   flatten  root[p] = the root of p; per block of 256 pixels the number of roots (root[p] == p)
//   scan     one workgroup: exclusive scan of the block counts, the total behind them
//   rank     rank[p] = roots before p in raster order (block-local scan + the block's base)
//   label    labels[p] = rank[root[p]] + 1, 0 for background
// Loops, and why each ends:
//   uf_find    follows parent links while they strictly decrease and stay >= 0: at most p steps
//   uf_unite   every round either returns or replaces the larger of its two indices by a strictly
//              smaller one (the value the atomicMin read, or a root below it): max(a, b) strictly
//              decreases, at most max(a, b) rounds.  No round waits for another thread's store.
//   run start  walks left inside the tile: at most 31 steps
//   disc       offsets clipped to the image: at most Ny * Nx
//   scans      log2(256) Hillis-Steele steps; a thread's chunk of the block counts
#include "common.h"

namespace {

constexpr int SG_MT = 16;                 // mask tile (16 x 16 threads), apron of 2
constexpr int SG_TW = 32, SG_TH = 32;     // labeller tile
constexpr int SG_BLOCK = 256;
constexpr int SG_SCAN = 256;              // threads of the scan workgroup = pixels of a count block

#define SG_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define SG_AGENT __HIP_MEMORY_SCOPE_AGENT

// ---------------------------------------------------------------------------------------- masks
// stage 1: m0 = map > gamma (float64; NaN and -inf are False); 2: eroded, outside = 1; 3: dilated,
// outside = 0
__global__ __launch_bounds__(SG_MT *SG_MT) void mask_kernel(const double *__restrict__ map, int Ny,
                                                           int Nx, double gamma, int stage,
                                                           uint8_t *__restrict__ out) {
  constexpr int W0 = SG_MT + 4, W1 = SG_MT + 2;
  __shared__ uint8_t s0[W0 * W0];  // 0 / 1, 2 = outside the image
  __shared__ uint8_t s1[W1 * W1];
  const int t = threadIdx.y * SG_MT + threadIdx.x;
  const int y0 = blockIdx.y * SG_MT, x0 = blockIdx.x * SG_MT;
  for (int i = t; i < W0 * W0; i += SG_MT * SG_MT) {
    const int yy = y0 - 2 + i / W0, xx = x0 - 2 + i % W0;
    const bool in = yy >= 0 && yy < Ny && xx >= 0 && xx < Nx;
    s0[i] = in ? (uint8_t)(map[(size_t)yy * Nx + xx] > gamma) : (uint8_t)2;
  }
  __syncthreads();
  for (int i = t; i < W1 * W1; i += SG_MT * SG_MT) {
    const int c = (i / W1 + 1) * W0 + i % W1 + 1;
    // (a pixel outside the image is 1 for its neighbours' erosion and 0 for their dilation)
    s1[i] = s0[c] == 1 && s0[c - 1] && s0[c + 1] && s0[c - W0] && s0[c + W0];
  }
  __syncthreads();
  const int y = y0 + threadIdx.y, x = x0 + threadIdx.x;
  if (y >= Ny || x >= Nx) return;
  const int c1 = (threadIdx.y + 1) * W1 + threadIdx.x + 1;
  uint8_t v;
  if (stage == 1)
    v = s0[(threadIdx.y + 2) * W0 + threadIdx.x + 2];
  else if (stage == 2)
    v = s1[c1];
  else
    v = s1[c1] | s1[c1 - 1] | s1[c1 + 1] | s1[c1 - W1] | s1[c1 + W1];
  out[(size_t)y * Nx + x] = v;
}

// out[y][x] = OR of in[y + dy][x + dx] over dy^2 + dx^2 < f^2 inside the image
__global__ void disc_kernel(const uint8_t *__restrict__ in, int Ny, int Nx, int f,
                            uint8_t *__restrict__ out) {
  const long S = (long)Ny * Nx, f2 = (long)f * f;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < S; p += (long)gridDim.x * blockDim.x) {
    const int y = (int)(p / Nx), x = (int)(p % Nx);
    const int ya = max(0, y - (f - 1)), yb = (int)min((long)Ny - 1, (long)y + f - 1);
    const int xa = max(0, x - (f - 1)), xb = (int)min((long)Nx - 1, (long)x + f - 1);
    uint8_t hit = 0;
    for (int yy = ya; yy <= yb && !hit; ++yy) {
      const long dy2 = (long)(yy - y) * (yy - y);
      for (int xx = xa; xx <= xb; ++xx)
        if (dy2 + (long)(xx - x) * (xx - x) < f2 && in[(size_t)yy * Nx + xx]) {
          hit = 1;
          break;
        }
    }
    out[p] = hit;
  }
}

__global__ void union_kernel(const int *__restrict__ a, const int *__restrict__ b, long n,
                             uint8_t *__restrict__ out) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x)
    out[p] = a[p] > 0 || b[p] > 0;
}

// ------------------------------------------------------------------------------------- labeller
template <int SCOPE>
__device__ __forceinline__ int uf_load(const int *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// the root of foreground pixel p (parents strictly decrease)
template <int SCOPE>
__device__ __forceinline__ int uf_find(const int *parent, int p) {
  for (;;) {
    const int q = uf_load<SCOPE>(parent + p);
    if (q >= p || q < 0) return p;
    p = q;
  }
}

// the same, and p linked straight to it (a smaller index of its own tree)
template <int SCOPE>
__device__ __forceinline__ int uf_find_compress(int *parent, int p) {
  const int r = uf_find<SCOPE>(parent, p);
  if (r != p) __hip_atomic_fetch_min(parent + p, r, __ATOMIC_RELAXED, SCOPE);
  return r;
}

// Lock-free union: the larger root goes under the smaller.  Where the atomicMin finds that `a` was
// no root any more, the link it read (old) is either kept (old < b) or replaced by b: both times
// old and b are still to be united, and the loop goes on from the value read.
template <int SCOPE>
__device__ __forceinline__ void uf_unite(int *parent, int a, int b) {
  for (;;) {
    a = uf_find_compress<SCOPE>(parent, a);
    b = uf_find_compress<SCOPE>(parent, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b, b = s;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;
    a = old;  // old < a and b < a: max(a, b) strictly decreases
  }
}

__global__ __launch_bounds__(SG_BLOCK) void tile_kernel(const uint8_t *__restrict__ mask, int Ny,
                                                        int Nx, int *__restrict__ parent) {
  constexpr int T = SG_TW * SG_TH;
  __shared__ int s[T];
  __shared__ uint8_t fg[T];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * SG_TW, y0 = blockIdx.y * SG_TH;
  for (int i = t; i < T; i += SG_BLOCK) {
    const int y = y0 + i / SG_TW, x = x0 + i % SG_TW;
    fg[i] = y < Ny && x < Nx && mask[(size_t)y * Nx + x] != 0;
  }
  __syncthreads();
  for (int i = t; i < T; i += SG_BLOCK) {
    int r = -1;
    if (fg[i]) {
      r = i;
      for (int lx = i % SG_TW; lx > 0 && fg[r - 1]; --lx) --r;  // first pixel of the run
    }
    s[i] = r;
  }
  __syncthreads();
  for (int i = t + SG_TW; i < T; i += SG_BLOCK)
    if (fg[i] && fg[i - SG_TW]) uf_unite<SG_WG>(s, i, i - SG_TW);
  __syncthreads();
  for (int i = t; i < T; i += SG_BLOCK) {
    const int y = y0 + i / SG_TW, x = x0 + i % SG_TW;
    if (y >= Ny || x >= Nx) continue;
    int g = -1;
    if (fg[i]) {
      const int r = uf_find<SG_WG>(s, i);
      g = (y0 + r / SG_TW) * Nx + x0 + r % SG_TW;
    }
    parent[(size_t)y * Nx + x] = g;
  }
}

// pairs across vertical tile edges first (nv of them: x = k * SG_TW against x - 1, every y), then
// across horizontal ones (y = k * SG_TH against y - 1, every x)
__global__ void seam_kernel(int Ny, int Nx, long nv, long nh, int *parent) {
  for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < nv + nh;
       k += (long)gridDim.x * blockDim.x) {
    int p, q;
    if (k < nv) {
      const int x = (int)(k / Ny + 1) * SG_TW, y = (int)(k % Ny);
      p = y * Nx + x, q = p - 1;
    } else {
      const long j = k - nv;
      const int y = (int)(j / Nx + 1) * SG_TH, x = (int)(j % Nx);
      p = y * Nx + x, q = p - Nx;
    }
    if (uf_load<SG_AGENT>(parent + p) >= 0 && uf_load<SG_AGENT>(parent + q) >= 0)
      uf_unite<SG_AGENT>(parent, p, q);
  }
}

__global__ __launch_bounds__(SG_SCAN) void flatten_kernel(int S, const int *__restrict__ parent,
                                                          int *__restrict__ root,
                                                          int *__restrict__ counts) {
  const int p = blockIdx.x * SG_SCAN + threadIdx.x;
  int r = -1;
  if (p < S) {
    if (parent[p] >= 0) r = uf_find<SG_AGENT>(parent, p);
    root[p] = r;
  }
  const int c = __syncthreads_count(p < S && r == p);
  if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(SG_SCAN) void rank_kernel(int S, const int *__restrict__ root,
                                                       const int *__restrict__ base,
                                                       int *__restrict__ rank) {
  __shared__ int part[SG_SCAN];
  const int t = threadIdx.x, p = blockIdx.x * SG_SCAN + t;
  const int flag = p < S && root[p] == p;
  part[t] = flag;
  __syncthreads();
  for (int off = 1; off < SG_SCAN; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  if (p < S) rank[p] = base[blockIdx.x] + part[t] - flag;
}

__global__ void label_kernel(int S, const int *__restrict__ root, const int *__restrict__ rank,
                             int *__restrict__ labels) {
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < S; p += gridDim.x * blockDim.x) {
    const int r = root[p];
    labels[p] = r >= 0 ? rank[r] + 1 : 0;
  }
}

inline int grid_for(long n) {
  return (int)std::max(1l, std::min((n + SG_BLOCK - 1) / SG_BLOCK, 4096l));
}

#define SG_LAUNCH(kernel, grid, block, ...)                                    \
  do {                                                                         \
    hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, __VA_ARGS__);      \
    ORIGIN_LAUNCH_CHECK();                                                     \
  } while (0)

int check_image(int Ny, int Nx) {
  ORIGIN_CHECK_ARG(Ny > 0 && Nx > 0 && (long)Ny * Nx < (1l << 30), "bad image shape (%d, %d)", Ny,
                   Nx);
  ORIGIN_CHECK_ARG(cdiv(Ny, SG_MT) <= 65535 && cdiv(Ny, SG_TH) <= 65535,
                   "image of %d rows is too tall", Ny);
  return ORIGIN_OK;
}

}  // namespace

extern "C" {

int origin_label_tile(int *tw, int *th) {
  ORIGIN_CHECK_ARG(tw && th, "null pointer");
  *tw = SG_TW, *th = SG_TH;
  return ORIGIN_OK;
}

int origin_label_scan_span(void) { return SG_SCAN * SG_SCAN; }

int origin_segmap_mask(origin_ctx *ctx, const double *d_map, int Ny, int Nx, double gamma, int f,
                       int stage, uint8_t *d_mask) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_map && d_mask, "null pointer");
  ORIGIN_CHECK_ARG(stage >= 1 && stage <= 4, "stage must be 1..4");
  int rc = check_image(Ny, Nx);
  if (rc) return rc;
  const dim3 grid(cdiv(Nx, SG_MT), cdiv(Ny, SG_MT)), block(SG_MT, SG_MT);
  const long S = (long)Ny * Nx;
  ProfScope ps(ctx, K_SEGMAP_MASK);
  if (stage < 4 || f < 0) {
    SG_LAUNCH(mask_kernel, grid, block, d_map, Ny, Nx, gamma, std::min(stage, 3), d_mask);
    return ORIGIN_OK;
  }
  if (f == 0) {  // no offset: the empty mask
    ORIGIN_HIP(hipMemsetAsync(d_mask, 0, (size_t)S, ctx->stream));
    return ORIGIN_OK;
  }
  void *tmp = nullptr;  // the mask before the disc, in the main stream's scratch
  if ((rc = origin_scratch(ctx, (size_t)S, &tmp))) return rc;
  SG_LAUNCH(mask_kernel, grid, block, d_map, Ny, Nx, gamma, 3, (uint8_t *)tmp);
  SG_LAUNCH(disc_kernel, dim3(grid_for(S)), dim3(SG_BLOCK), (const uint8_t *)tmp, Ny, Nx, f,
            d_mask);
  return ORIGIN_OK;
}

int origin_segmap_union(origin_ctx *ctx, const int *d_a, const int *d_b, long n, uint8_t *d_mask) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_a && d_b && d_mask && n > 0, "bad arguments");
  ProfScope ps(ctx, K_SEGMAP_MASK);
  SG_LAUNCH(union_kernel, dim3(grid_for(n)), dim3(SG_BLOCK), d_a, d_b, n, d_mask);
  return ORIGIN_OK;
}

int origin_segmap_label(origin_ctx *ctx, const uint8_t *d_mask, int Ny, int Nx, int *d_labels,
                        int *h_n) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_mask && d_labels && h_n, "null pointer");
  int rc = check_image(Ny, Nx);
  if (rc) return rc;
  const int S = Ny * Nx, nblk = cdiv(S, SG_SCAN);
  const int tx = cdiv(Nx, SG_TW), ty = cdiv(Ny, SG_TH);
  const long nv = (long)(tx - 1) * Ny, nh = (long)(ty - 1) * Nx;
  // the work arrays are pieces of the main stream's scratch: laid out once for the size, once on it
  int *parent, *root, *rank, *counts;
  auto layout = [&](Carver &c) {
    parent = c.take<int>(S), root = c.take<int>(S), rank = c.take<int>(S);
    counts = c.take<int>(nblk + 1);
  };
  Carver c;
  layout(c);
  void *scr = nullptr;
  if ((rc = origin_scratch(ctx, c.off, &scr))) return rc;
  c.off = 0, c.base = (char *)scr;
  layout(c);
  {
    ProfScope ps(ctx, K_SEGMAP_LABEL);
    SG_LAUNCH(tile_kernel, dim3(tx, ty), dim3(SG_BLOCK), d_mask, Ny, Nx, parent);
    if (nv + nh > 0)
      SG_LAUNCH(seam_kernel, dim3(grid_for(nv + nh)), dim3(SG_BLOCK), Ny, Nx, nv, nh, parent);
    SG_LAUNCH(flatten_kernel, dim3(nblk), dim3(SG_SCAN), S, parent, root, counts);
    SG_LAUNCH(origin_scan_kernel<SG_SCAN>, dim3(1), dim3(SG_SCAN), nblk, counts);
    SG_LAUNCH(rank_kernel, dim3(nblk), dim3(SG_SCAN), S, root, counts, rank);
    SG_LAUNCH(label_kernel, dim3(grid_for(S)), dim3(SG_BLOCK), S, root, rank, d_labels);
  }
  return origin_d2h(ctx, h_n, counts + nblk, sizeof(int));
}

}  // extern "C"
