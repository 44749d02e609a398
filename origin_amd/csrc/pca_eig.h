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

// A batch of symmetric PSD matrices for the eigen-solver: matrix k is n[k] columns at G + g_off[k]
// with row stride ld[k], its leading eigenvector goes to v + v_off[k], its basis scratch is
// EIG_QROWS * ld[k] doubles at Q + q_off[k].  info (may be null): per matrix (theta, residual,
// restarts).  dbg (may be null): per matrix steps and time, then phase times.
struct EigBatch {
  int nmat;
  const double *G;
  const long *g_off, *ld, *n;
  double *Q;
  const long *q_off;
  double *v;
  const long *v_off;
  double *info, *dbg;
};

// The K-split slabs of gram_kernel (slab s of matrix k at ptr + s * stride + g_off[k]), given when
// every matrix has at most LANCZOS_M columns: the solver then sums them itself instead of reading G.
struct EigSlabs {
  const double *ptr = nullptr;
  long stride = 0;
  int ksplit = 0;
};

// Leading eigenvector of every matrix of the batch, one launch on ctx->stream; ldmax = the largest
// row stride, which picks the kernel (the size classes are listed at the top of pca_eig.hip).
int origin_pca_eig_launch(origin_ctx *ctx, const EigBatch &batch, long ldmax, EigSlabs slabs = {});
