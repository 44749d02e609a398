// Moments of a device cube: the two np.std calls that open add_tglr_stat
// (reference muse_origin/lib_origin.py:2127-2129, called by CleanResults.run, steps.py:1155-1160)
//
//   std_correl = np.std(correl);  std_std = np.std(std)
//
// over the two full float64 host cubes.  Here the cube stays in HBM as float32 and one streaming
// pass gives (n, sum(x - shift), sum((x - shift)^2)) over the voxels of the kept spaxels; only the
// three scalars cross PCIe.  np.std is two such passes (shift = 0 for the mean, shift = mean for
// M2: kernels.cube_std).
//
// Every voxel is widened to float64 before the subtraction and all sums are float64, in a fixed
// order (the discipline of lines.hip: no floating-point atomics, so the same input gives the same
// bits on every call):
//   lane   : SM_VEC accumulators, one per element of its 16-byte loads; the lane visits its vectors
//            in ascending address order (grid stride), then adds (a0 + a1) + (a2 + a3)
//   wave   : xor butterfly, 32 .. 1
//   block  : the four wave sums, ((w0 + w1) + (w2 + w3)), plus -- in block 0 only -- the head and
//            tail voxels in ascending address order
//   grid   : block partials in a workspace; a second kernel of one wave adds them, lane l taking
//            blocks l, l + 64, ... in ascending order, then the same butterfly
// The grid is a function of the voxel count alone (at most SM_MAX_BLOCKS blocks), never of the
// device, so the order -- and the result -- is the same on every gfx950 part.
//
// The cube pointer needs float alignment only: the voxels before the first 16-byte boundary
// (head) and those behind the last whole vector (tail) are read as scalars.  S need not be a
// multiple of anything: the spaxel of a voxel is carried along the grid stride (one 64-bit
// remainder per lane, then additions), not recomputed per voxel.  A voxel of an excluded spaxel is
// not read into the sums at all (select, not multiply): a NaN there does not propagate, a NaN in a
// kept spaxel does, as in NumPy.
#include "common.h"

namespace {

constexpr int SM_THREADS = 256;       // lanes per block
constexpr int SM_VEC = 4;             // voxels per load
constexpr int SM_UNROLL = 4;          // loads in flight per lane
constexpr int SM_MAX_BLOCKS = 1024;   // 4 blocks (16 waves) per CU of a 256-CU part: 64 KiB of
                                      // loads in flight per CU with SM_UNROLL = 4

typedef float f32x4s __attribute__((ext_vector_type(4)));

struct Moments {
  double n, s1, s2;
};

__device__ __forceinline__ double sm_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// one voxel into one accumulator triple
__device__ __forceinline__ void sm_add(float x, bool k, double shift, int &n, double &s1,
                                       double &s2) {
  const double d = k ? (double)x - shift : 0.0;
  n += k;
  s1 += d;
  s2 = fma(d, d, s2);
}

template <bool KEEP>
__global__ __launch_bounds__(SM_THREADS) void moments_kernel(
    const float *__restrict__ cube, const uint8_t *__restrict__ keep, long n, long S, long head,
    long nvec, long stepmod, double shift, double *__restrict__ part) {
  __shared__ double red[3][SM_THREADS / 64];
  const f32x4s *vec = reinterpret_cast<const f32x4s *>(cube + head);
  const long stride = (long)gridDim.x * SM_THREADS;
  long v = (long)blockIdx.x * SM_THREADS + threadIdx.x;
  // spaxel of the first voxel of vector v; advanced by stepmod = (stride * SM_VEC) % S per step
  long sp = KEEP ? (head + v * SM_VEC) % S : 0;
  int cnt[SM_VEC] = {};
  double a1[SM_VEC] = {}, a2[SM_VEC] = {};

  auto take = [&](const f32x4s q) {
#pragma unroll
    for (int e = 0; e < SM_VEC; ++e) {
      bool k = true;
      if (KEEP) {
        long se = sp + e;
        while (se >= S) se -= S;   // (at most once unless S < SM_VEC)
        k = keep[se] != 0;
      }
      sm_add(q[e], k, shift, cnt[e], a1[e], a2[e]);
    }
    if (KEEP) {
      sp += stepmod;
      if (sp >= S) sp -= S;
    }
  };

  for (; v + (SM_UNROLL - 1) * stride < nvec; v += SM_UNROLL * stride) {
    f32x4s q[SM_UNROLL];
#pragma unroll
    for (int u = 0; u < SM_UNROLL; ++u) q[u] = vec[v + u * stride];
#pragma unroll
    for (int u = 0; u < SM_UNROLL; ++u) take(q[u]);
  }
  for (; v < nvec; v += stride) take(vec[v]);

  double t[3];
  t[0] = (double)((cnt[0] + cnt[1]) + (cnt[2] + cnt[3]));
  t[1] = (a1[0] + a1[1]) + (a1[2] + a1[3]);
  t[2] = (a2[0] + a2[1]) + (a2[2] + a2[3]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    t[j] = sm_wave_sum(t[j]);
    if (lane == 0) red[j][wave] = t[j];
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  Moments m;
  m.n = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  m.s1 = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  m.s2 = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  if (blockIdx.x == 0) {  // head [0, head) and tail [head + nvec * SM_VEC, n): fewer than 4 each
    const long tail0 = head + nvec * SM_VEC;
    for (long i = 0; i < n; ++i) {
      if (i == head) i = tail0;
      if (i >= n) break;
      int c = 0;
      double s1 = 0.0, s2 = 0.0;
      sm_add(cube[i], !KEEP || keep[i % S] != 0, shift, c, s1, s2);
      m.n += c;
      m.s1 += s1;
      m.s2 += s2;
    }
  }
  part[3 * blockIdx.x + 0] = m.n;
  part[3 * blockIdx.x + 1] = m.s1;
  part[3 * blockIdx.x + 2] = m.s2;
}

// out[j] = sum over the blocks of part[3 * b + j]: one wave, lane l takes b = l, l + 64, ...
__global__ __launch_bounds__(64) void moments_final_kernel(const double *__restrict__ part,
                                                           int nblk, double *__restrict__ out) {
  double t[3] = {0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nblk; b += 64)
#pragma unroll
    for (int j = 0; j < 3; ++j) t[j] += part[3 * b + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) t[j] = sm_wave_sum(t[j]);
  if (threadIdx.x == 0) out[0] = t[0], out[1] = t[1], out[2] = t[2];
}

}  // namespace

extern "C" {

int origin_cube_moments_blocks(long n_voxels) {
  const long nvec = n_voxels / SM_VEC;
  long b = (nvec + SM_THREADS - 1) / SM_THREADS;
  return (int)(b < 1 ? 1 : b > SM_MAX_BLOCKS ? SM_MAX_BLOCKS : b);
}

int origin_cube_moments(origin_ctx *ctx, const float *d_cube, const uint8_t *d_keep, int Nz, long S,
                        double shift, double *h_out) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_cube && h_out && Nz > 0 && S > 0, "bad arguments");
  ORIGIN_CHECK_ARG(((uintptr_t)d_cube & 3) == 0, "d_cube must be float aligned");
  const long n = (long)Nz * S;
  // voxels before the first 16-byte boundary, whole vectors behind them, the rest is the tail
  long head = (long)((16 - ((uintptr_t)d_cube & 15)) & 15) / (long)sizeof(float);
  if (head > n) head = n;
  const long nvec = (n - head) / SM_VEC;
  const int nblk = origin_cube_moments_blocks(n);
  const long stepmod = ((long)nblk * SM_THREADS * SM_VEC) % S;
  // [block partials: nblk x 3 x float64 | result: 3 x float64]
  void *scr = nullptr;
  int rc = origin_scratch(ctx, (size_t)(nblk + 1) * 3 * sizeof(double), &scr);
  if (rc) return rc;
  double *d_part = (double *)scr, *d_out = d_part + 3 * (size_t)nblk;
  {
    ProfScope ps(ctx, K_STATS);
    if (d_keep)
      hipLaunchKernelGGL(moments_kernel<true>, dim3(nblk), dim3(SM_THREADS), 0, ctx->stream, d_cube,
                         d_keep, n, S, head, nvec, stepmod, shift, d_part);
    else
      hipLaunchKernelGGL(moments_kernel<false>, dim3(nblk), dim3(SM_THREADS), 0, ctx->stream,
                         d_cube, d_keep, n, S, head, nvec, stepmod, shift, d_part);
    hipLaunchKernelGGL(moments_final_kernel, dim3(1), dim3(64), 0, ctx->stream, d_part, nblk,
                       d_out);
  }
  ORIGIN_LAUNCH_CHECK();
  ORIGIN_HIP(hipMemcpyAsync(h_out, d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

}  // extern "C"
