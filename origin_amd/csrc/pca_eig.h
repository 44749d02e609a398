// What pca.hip and pca_eig.hip share: the eigen-solver's launch and the sizes its caller lays
// buffers out by, and the wave reduction both files' kernels use.  And what pca.hip and lines.hip
// share: the K-split of a Gram launch, which lines.hip sizes its Gram groups by.
#pragma once
#include "common.h"

// K-split of a Gram launch over `ntiles` tiles, so that small problems still put >= ~8 waves on
// every CU.  The one copy of the rule: gram_launch (pca.hip) splits by it, and lines.hip keeps its
// Gram groups small enough to get the split of a single problem.
inline int pca_gram_ksplit(int num_cu, long ntiles, int Nz) {
  int ksplit = (int)(((long)num_cu * 8 + ntiles - 1) / ntiles);
  if (ksplit < 1) ksplit = 1;
  if (ksplit > 32) ksplit = 32;
  if (ksplit > Nz / 64) ksplit = Nz / 64 > 0 ? Nz / 64 : 1;
  return ksplit;
}

typedef double double4_t __attribute__((ext_vector_type(4)));

// Sum of a double over the 64 lanes of a wave, returned in every lane.  Within each row of
// 16 lanes the exchange uses DPP moves (quad_perm / row_ror: a few cycles each) instead of
// ds_bpermute; the four row sums are then combined through v_readlane.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum_d(double v) {
  v += dpp_mov_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_mov_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_mov_d<0x124>(v);  // row_ror:4
  v += dpp_mov_d<0x128>(v);  // row_ror:8  -> every lane holds the sum of its row of 16
  const int lo = __double2loint(v), hi = __double2hiint(v);
  double t = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
    t += __hiloint2double(__builtin_amdgcn_readlane(hi, 16 * r),
                          __builtin_amdgcn_readlane(lo, 16 * r));
  return t;
}

constexpr int LANCZOS_M = 48;    // matrices of up to this many columns: the small-matrix solver
constexpr int EIG_QROWS = 194;   // basis rows per matrix in the scratch d_q

// Leading eigenvector of nmat symmetric PSD matrices on ctx->stream: matrix k is d_n[k] columns
// at d_G + d_g_off[k] with row stride d_ld[k] (ldmax = the largest stride, which picks the
// kernel), its vector goes to d_v + d_v_off[k], its basis scratch is EIG_QROWS * ld doubles at
// d_q + d_q_off[k].  d_info (may be null): per matrix (theta, residual, restarts).  d_slab: the
// K-split slabs of gram_kernel when every matrix has at most LANCZOS_M columns and the solver sums
// them itself.  d_dbg (may be null): per matrix steps and time, then phase times.
int origin_pca_eig_launch(origin_ctx *ctx, int nmat, long ldmax, const double *d_G,
                          const long *d_g_off, const long *d_ld, const long *d_n, double *d_q,
                          const long *d_q_off, double *d_v, const long *d_v_off, double *d_info,
                          const double *d_slab = nullptr, long slab_stride = 0, int ksplit = 0,
                          double *d_dbg = nullptr);
