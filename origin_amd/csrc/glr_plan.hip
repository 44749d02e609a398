// GLR matched filter: the plan (glr.hip has the algebra and the runs).  A plan holds what depends on
// the PSFs, the weight maps and the profiles alone: the taps in the layouts of every kernel, the
// border-class normalisation tables of an unweighted field, the FOLD tables and their eps test,
// and the norm cube of a weighted one.  It also says what a plan runs (glr_paths_at) and holds the
// launch geometry the two matrix-core spectral kernels share: the spaxels of a range, the z chunks
// and the rows of the partial maps.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <vector>

#include "glr_plan.h"

namespace {

// ------------------------------------------------------------------------------------
// border-class normalisation tables (mode 0)
// ------------------------------------------------------------------------------------
// normcls[z][cy][cx] = sum over the in-field part of the window of k_z^2
__global__ __launch_bounds__(256) void norm_classes_kernel(const float *__restrict__ k2, int Nz,
                                                           int P, double *__restrict__ ncls) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = (long)Nz * P * P;
  if (i >= n) return;
  const int z = (int)(i / (P * P));
  const int cls = (int)(i - (long)z * P * P);
  const int cy = cls / P, cx = cls - cy * P;
  const int c = P / 2;
  // class id t <-> window clipped to dy in [max(0,c-t), min(P-1, P-1+c-t)]
  const int dy0 = max(0, c - cy), dy1 = min(P - 1, P - 1 + c - cy);
  const int dx0 = max(0, c - cx), dx1 = min(P - 1, P - 1 + c - cx);
  const float *kz = k2 + (long)z * P * P;
  double acc = 0.0;
  for (int dy = dy0; dy <= dy1; ++dy)
    for (int dx = dx0; dx <= dx1; ++dx) acc += (double)kz[dy * P + dx];
  ncls[i] = acc;
}

// eps of the FOLD form on an explicit norm cube (NORMW): over every voxel of the channels
// [zf0, zf1) and every profile, |sqrt(den_k / (norm sum_j p_k[j]^2)) - 1| with den_k the true
// smoothed norm (lib_origin.py:1055: conv of norm_fsf with p_k^2); a spaxel no field covers has
// norm = 0 and den = 0 in both forms.  norm: channel 0 of the padded cube.  A thread takes
// NE_ZT consecutive channels of one spaxel (their common window in registers), the squared taps
// sit in LDS as dense 65-slot rows (slot u = channel offset u - 32); float bits through atomicMax
// (values >= 0).  Runs once per plan (glr_plan_prepare): ~0.1 s at 3681 x 600 x 600.
constexpr int NE_ZT = 4;
__global__ __launch_bounds__(256) void normw_eps_kernel(const float *__restrict__ norm,
                                                        const float *__restrict__ taps2,
                                                        const int *__restrict__ tap_off, int K,
                                                        long S, int zf0, int zf1,
                                                        unsigned *__restrict__ eps_bits) {
  __shared__ float tt[MF_MAX_K][65];
  __shared__ float ts2[MF_MAX_K];
  for (int i = threadIdx.x; i < K * 65; i += 256) {
    const int k = i / 65, u = i - 65 * k;
    const int o = tap_off[k], L = tap_off[k + 1] - o, lw = (L - 1) / 2;
    const int j = 32 + lw - u;  // window slot u = channel z - 32 + u = z + lw - j
    tt[k][u] = (j >= 0 && j < L) ? taps2[o + j] : 0.0f;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    float a = 0.0f;
    for (int u = 0; u < 65; ++u) a += tt[threadIdx.x][u];
    ts2[threadIdx.x] = a;
  }
  __syncthreads();
  const long sp = (long)blockIdx.x * 256 + threadIdx.x;
  const int z = zf0 + NE_ZT * (int)blockIdx.y;
  float eps = 0.0f;
  if (sp < S) {
    float w[64 + NE_ZT];  // channels z - 32 .. z + NE_ZT + 31 (the pads of the cube cover the ends)
#pragma unroll
    for (int j = 0; j < 64 + NE_ZT; ++j) w[j] = norm[(long)(z - 32 + j) * S + sp];
    for (int k = 0; k < K; ++k) {
      float den[NE_ZT];
#pragma unroll
      for (int c = 0; c < NE_ZT; ++c) den[c] = 0.0f;
#pragma unroll
      for (int u = 0; u < 65; ++u) {
        const float t = tt[k][u];
#pragma unroll
        for (int c = 0; c < NE_ZT; ++c) den[c] += t * w[u + c];
      }
#pragma unroll
      for (int c = 0; c < NE_ZT; ++c) {
        if (z + c >= zf1) continue;
        const float ref = w[32 + c] * ts2[k];
        const float e = ref > 0.0f ? fabsf(sqrtf(den[c] / ref) - 1.0f)
                                   : (den[c] > 0.0f ? INFINITY : 0.0f);
        eps = fmaxf(eps, e);
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) eps = fmaxf(eps, __shfl_xor(eps, o));
  if ((threadIdx.x & 63) == 0 && eps > 0.0f) atomicMax(eps_bits, __float_as_uint(eps));
}

// FOLD tables of the matrix-core spectral stage (glr_spectral_mfma.hip): rden_fold = rden / a_k,
// s[cls][z] = the middle of its range over k, eps = the largest half width of that range relative
// to s over the FOLD channels [zf0, zf1) (float bits, atomicMax: every value is >= 0)
__global__ __launch_bounds__(256) void fold_tables_kernel(const float *__restrict__ rden,
                                                          const float *__restrict__ ainv, int K,
                                                          int PP, int NzP, int zf0, int zf1,
                                                          float *__restrict__ rden_fold,
                                                          float *__restrict__ sden,
                                                          unsigned *__restrict__ eps_bits) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)PP * NzP) return;
  const int cls = (int)(i / NzP), z = (int)(i % NzP);
  float lo = INFINITY, hi = 0.0f;
  for (int k = 0; k < K; ++k) {
    const long j = ((long)cls * K + k) * NzP + z;
    const float v = rden[j] * ainv[k];
    rden_fold[j] = v;
    lo = fminf(lo, v), hi = fmaxf(hi, v);
  }
  sden[i] = 0.5f * (lo + hi);
  if (z >= zf0 && z < zf1) {
    const float eps = lo > 0.0f ? (hi - lo) / (hi + lo) : INFINITY;
    atomicMax(eps_bits, __float_as_uint(eps));
  }
}

// rden[cls][k][z] = 1/sqrt(sum_j p_k[j]^2 normcls[z + lw - j][cls])   (0 if den <= 0 or z >= Nz)
// z is the fastest axis (stride NzP, a multiple of 32): a lane of the matrix-core kernel
// fetches the four consecutive channels of an accumulator group with one 16-byte load.
__global__ __launch_bounds__(256) void rden_kernel(const double *__restrict__ ncls,
                                                   const float *__restrict__ taps2,
                                                   const int *__restrict__ tap_off, int K, int Nz,
                                                   int PP, int NzP, float *__restrict__ rden) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long n = (long)PP * K * NzP;
  if (i >= n) return;
  const int z = (int)(i % NzP);
  const int k = (int)((i / NzP) % K);
  const int cls = (int)(i / ((long)NzP * K));
  if (z >= Nz) {
    rden[i] = 0.0f;
    return;
  }
  const int off = tap_off[k], L = tap_off[k + 1] - off, lw = (L - 1) / 2;
  double den = 0.0;
  for (int j = 0; j < L; ++j) {
    const int zz = z + lw - j;
    if (zz >= 0 && zz < Nz) den += (double)taps2[off + j] * ncls[(long)zz * PP + cls];
  }
  rden[i] = den > 0.0 ? (float)(1.0 / sqrt(den)) : 0.0f;
}

// ------------------------------------------------------------------------------------
// spectral stage on the matrix cores: operand layout (the kernel is glr_spectral_mfma.hip).
//
// num_k[z] = sum_j p_k[j] x[z + lw_k - j] is a banded Toeplitz product: for a tile of 32 output
// channels z0..z0+31 and the 96-channel window x[z0-32 .. z0+63],
//     num_k[z0+m, s] = sum_{i=0}^{95} A_k[m][i] X[i][s],   A_k[m][i] = p_k[m + lw_k + 32 - i]
// (zero outside the band), i.e. a [32 x 96] x [96 x N] GEMM per profile whose B operand -- the
// data -- is shared by all K profiles.  fp32 MFMA runs at the vector rate, so the product is
// evaluated with v_mfma_f32_32x32x16_f16 (16x that rate) on a two-term split of both
// operands: y = x * 2^e (e per tile, from the tile's max |x|, so any input range is safe and
// scaling the cube by a power of two scales the result exactly), y = yh + yl with yh = f16(y),
// yl = f16(y - yh) -- 22 significant bits -- likewise the taps, and
//     num = Ah Bh + Ah Bl + Al Bh      (the dropped Al Bl term is 2^-22 relative)
// accumulated in fp32 by the matrix core.  Error vs float64: ~3e-7 of sum |p x|, the same
// order as the fp32 FMA chain of spectral3_kernel (~1e-7); origin_glr_plan_set_precision
// selects that kernel instead.
//
// A wave owns 32 consecutive spaxels (one 32-column B tile, fragments loaded straight from
// global memory: lane (r, h) holds X[16 ks + 8 h + j][r], 128-byte segments per half wave) and
// marches z in tiles of 32.  The A fragments of a Toeplitz matrix are 8 consecutive entries of
// one padded tap array G_k[e] = p_k[lw_k + 63 - e] starting at e = 16 ks + 8 h - m + 31; LDS
// holds, per profile, 8 copies of G_k shifted by 0..7 elements (hi and lo halves, 320-byte
// copies: conflict-free for the lane groups of ds_read_b128) so that every fragment is ONE
// aligned ds_read_b128 at a per-lane base plus an immediate offset.  Profiles whose half width
// is <= 16 only touch window blocks 1..4 (4 of the 6 k-steps).
// Normalisation: 1/sqrt(den) of the lane's border class, exact for every spaxel (no fix-up
// pass behind this kernel).
// ------------------------------------------------------------------------------------

template <typename T>
int upload(origin_ctx *ctx, const std::vector<T> &h, T **d, size_t *bytes) {
  void *p = nullptr;
  const size_t n = std::max<size_t>(h.size(), 1) * sizeof(T);
  ORIGIN_HIP(hipMalloc(&p, n));
  *d = (T *)p;
  *bytes += n;
  if (!h.empty()) {
    ORIGIN_HIP(hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice,
                              ctx->stream));
    ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  }
  return ORIGIN_OK;
}

// a device allocation that lives for one step of plan creation
struct DevTmp {
  void *p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp &) = delete;
  DevTmp &operator=(const DevTmp &) = delete;
  ~DevTmp() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};

// a plan under construction: a step that fails just returns, the plan goes with it
struct PlanDeleter {
  void operator()(origin_glr_plan *pl) const { origin_glr_plan_destroy(pl); }
};

// the profiles as every kernel takes them: odd lengths 2 lw + 1, centred on tap lw
struct Profiles {
  std::vector<float> taps, taps2;  // concatenated; taps2 = squares
  std::vector<int> off;            // [K+1]
  int len(int k) const { return off[k + 1] - off[k]; }
  int lw(int k) const { return (len(k) - 1) / 2; }
};

// zero-mean PSF per channel and field: psf -= psf.mean()      (lib_origin.py:1033-1034)
int prepare_psfs(origin_glr_plan *pl, const double *h_psf, const double *h_weights) {
  const size_t PP = (size_t)pl->P * pl->P, planes = (size_t)pl->nfields * pl->Nz;
  std::vector<float> k(planes * PP), k2(k.size());
  for (size_t i = 0; i < planes; ++i) {
    const double *src = h_psf + i * PP;
    double m = 0.0;
    for (size_t j = 0; j < PP; ++j) m += src[j];
    m /= (double)PP;
    for (size_t j = 0; j < PP; ++j) {
      const double v = src[j] - m;
      k[i * PP + j] = (float)v;
      k2[i * PP + j] = (float)(v * v);  // psf **= 2                            (lib :1040)
    }
  }
  if (int rc = upload(pl->ctx, k, &pl->d_k, &pl->bytes)) return rc;
  if (int rc = upload(pl->ctx, k2, &pl->d_k2, &pl->bytes)) return rc;
  if (h_weights) {
    std::vector<float> w((size_t)pl->nfields * pl->Ny * pl->Nx);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (float)h_weights[i];
    if (int rc = upload(pl->ctx, w, &pl->d_w, &pl->bytes)) return rc;
  }
  return ORIGIN_OK;
}

// profiles: every kernel centres a profile of length 2*lw+1 on tap lw.  The reference centres
// on startind = (L-1)//2 (lib :1179-1181), which for an even L is L/2 - 1: an even profile
// therefore gets a LEADING zero tap, p' = [0, p_0 .. p_{L-1}], lw' = L/2, so that
// sum_j p'[j] x[z + lw' - j] = sum_j p[j] x[z + L/2 - 1 - j]  (a trailing zero would shift the
// output by one channel)
int prepare_profiles(origin_glr_plan *pl, const double *h_taps, const int *h_tap_off,
                     Profiles *prof) {
  const int K = pl->K;
  prof->off.assign(K + 1, 0);
  for (int kk = 0; kk < K; ++kk) {
    const int L = h_tap_off[kk + 1] - h_tap_off[kk];
    if (!(L & 1)) {
      prof->taps.push_back(0.f);
      prof->taps2.push_back(0.f);
    }
    for (int j = 0; j < L; ++j) {
      const double v = h_taps[h_tap_off[kk] + j];
      prof->taps.push_back((float)v);
      prof->taps2.push_back((float)(v * v));
    }
    prof->off[kk + 1] = (int)prof->taps.size();
    pl->lwmax = std::max(pl->lwmax, prof->lw(kk));
  }
  // scalar loads may read a few taps past the end of a profile row: pad
  prof->taps.resize(prof->taps.size() + 64, 0.f);
  prof->taps2.resize(prof->taps2.size() + 64, 0.f);
  if (int rc = upload(pl->ctx, prof->taps, &pl->d_taps, &pl->bytes)) return rc;
  if (int rc = upload(pl->ctx, prof->taps2, &pl->d_taps2, &pl->bytes)) return rc;
  return upload(pl->ctx, prof->off, &pl->d_tap_off, &pl->bytes);
}

// half profiles (exactly symmetric profiles -- the Gaussian dictionaries are -- allow
// p[c+d] (w[c+d] + w[c-d])) and the fixed-length rows of spectral3_kernel
int build_half_taps_and_rows(origin_glr_plan *pl, const Profiles &prof) {
  const int K = pl->K;
  std::vector<float> htaps;
  std::vector<int> hoff(K + 1, 0);
  pl->symmetric = 1;
  for (int kk = 0; kk < K; ++kk) {
    const float *p = &prof.taps[prof.off[kk]];
    const int lw = prof.lw(kk);
    for (int d = 0; d <= lw; ++d) {
      if (p[lw + d] != p[lw - d]) pl->symmetric = 0;
      htaps.push_back(p[lw + d]);
    }
    hoff[kk + 1] = (int)htaps.size();
  }
  htaps.resize(htaps.size() + 64, 0.f);
  if (int rc = upload(pl->ctx, htaps, &pl->d_htaps, &pl->bytes)) return rc;
  if (int rc = upload(pl->ctx, hoff, &pl->d_htap_off, &pl->bytes)) return rc;
  if (pl->lwmax > 32) return ORIGIN_OK;
  const int lwmax = pl->lwmax;
  const int lwt = lwmax <= 8 ? 8 : lwmax <= 16 ? 16 : lwmax <= 24 ? 24 : lwmax <= 29 ? 29 : 32;
  const int RL = (2 * lwt + 1 + 15) / 16 * 16 + 16;  // [lw | taps padded to 16s]
  std::vector<float> rows((size_t)(K + 2) * RL, 0.f);
  for (int kk = 0; kk < K; ++kk) {
    const int L = prof.len(kk), lw = prof.lw(kk);
    memcpy(&rows[(size_t)kk * RL], &lw, sizeof(int));
    for (int j = 0; j < L; ++j) rows[(size_t)kk * RL + 1 + j] = prof.taps[prof.off[kk] + j];
  }
  if (int rc = upload(pl->ctx, rows, &pl->d_rows, &pl->bytes)) return rc;
  pl->lwt = lwt;
  return ORIGIN_OK;
}

unsigned short to_bf16(float v) {  // round to nearest even
  unsigned u;
  memcpy(&u, &v, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);
  return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// matrix-core spectral stage: padded tap arrays G_k[e] = p_k[lw_k + 63 - e], 8 copies shifted
// by 0..7 elements (glr_tables.h), profiles in processing order (narrow ones -- half width
// <= 16: window blocks 1..4 -- first, so that the kernel's profile pairs are narrow/narrow,
// at most one narrow/wide, wide/wide); f16 hi + lo (times 2^MF_TAP_SCALE_LOG2) and bf16.
// fold_a: a_k = 1/sqrt(sum p_k^2) of the FOLD tables.
int build_mfma_tap_tables(origin_glr_plan *pl, const Profiles &prof, std::vector<double> *fold_a) {
  const int K = pl->K;
  std::vector<int> order(K), pinfo(K, 0);
  for (int kk = 0; kk < K; ++kk) order[kk] = kk;
  std::stable_sort(order.begin(), order.end(),
                   [&](int a, int b) { return (prof.lw(a) > 16) < (prof.lw(b) > 16); });
  constexpr size_t PROF = MF_PROF_BYTES / 2, COPY = MF_COPY_BYTES / 2, LO = 8 * COPY;  // in halves
  std::vector<_Float16> at(K * PROF, (_Float16)0.0f);
  std::vector<_Float16> at2(pl->mode == 1 ? at.size() : 0, (_Float16)0.0f);
  std::vector<unsigned short> ab(K * PROF, 0);
  // FOLD: the same tables with the taps times a_k (plans with an explicit norm cube use them
  // too: NORMW, glr_spectral_mfma.hip)
  std::vector<_Float16> atf(mf_fold_fits(K) ? at.size() : 0, (_Float16)0.0f);
  std::vector<unsigned short> abf(mf_fold_fits(K) ? ab.size() : 0, 0);
  fold_a->assign(K, 1.0);
  for (int kk = 0; kk < K; ++kk) {
    double s2 = 0.0;
    for (int j = prof.off[kk]; j < prof.off[kk + 1]; ++j) s2 += (double)prof.taps[j] * prof.taps[j];
    if (s2 > 0.0) (*fold_a)[kk] = 1.0 / std::sqrt(s2);
  }
  const float tscale = (float)(1 << MF_TAP_SCALE_LOG2);
  auto split = [&](float g, _Float16 *dst) {  // two-term f16 split: hi here, lo in the lo copies
    const _Float16 gh = (_Float16)g;
    dst[0] = gh;
    dst[LO] = (_Float16)(g - (float)gh);
  };
  for (int slot = 0; slot < K; ++slot) {
    const int kk = order[slot];
    const int L = prof.len(kk), lw = prof.lw(kk);
    pinfo[slot] = kk | ((lw > 16) << 8);
    for (int c = 0; c < 8; ++c)
      for (int q = 0; q < MF_GROUPS; ++q)
        for (int j = 0; j < 8; ++j) {
          const int e = 8 * q + c + j, ti = lw + 63 - e;
          const float t = (ti >= 0 && ti < L) ? prof.taps[prof.off[kk] + ti] : 0.0f;
          const size_t base = slot * PROF + c * COPY + (size_t)q * 8 + j;
          split(t * tscale, &at[base]);
          ab[base] = to_bf16(t);
          if (!atf.empty()) {
            const float tf = (float)((double)t * (*fold_a)[kk]);
            split(tf * tscale, &atf[base]);
            abf[base] = to_bf16(tf);
          }
          // squared taps (float32 squares, as d_taps2) for the denominator
          if (!at2.empty()) split((t * t) * tscale, &at2[base]);
        }
  }
  origin_ctx *ctx = pl->ctx;
  if (int rc = upload(ctx, at, (_Float16 **)&pl->d_atab, &pl->bytes)) return rc;
  if (int rc = upload(ctx, ab, (unsigned short **)&pl->d_atab_bf16, &pl->bytes)) return rc;
  if (!at2.empty())
    if (int rc = upload(ctx, at2, (_Float16 **)&pl->d_atab2, &pl->bytes)) return rc;
  if (!atf.empty()) {
    if (int rc = upload(ctx, atf, (_Float16 **)&pl->d_atab_fold, &pl->bytes)) return rc;
    if (int rc = upload(ctx, abf, (unsigned short **)&pl->d_atab_bf16_fold, &pl->bytes)) return rc;
  }
  if (int rc = upload(ctx, pinfo, &pl->d_pwide, &pl->bytes)) return rc;
  pl->n_narrow = 0;
  for (int slot = 0; slot < K; ++slot) pl->n_narrow += (pinfo[slot] >> 8) == 0;
  pl->order_ident = 1;
  for (int slot = 0; slot < K; ++slot) pl->order_ident &= order[slot] == slot;
  pl->h_order = order;
  return ORIGIN_OK;
}

// the norm cube of a weighted plan (padded like cube_fsf: MF_PAD_FRONT zero channels in front,
// MF_PAD_BACK behind) is a constant of the plan: allocated HERE, where the callers' memory
// checks run and plan->bytes is read, and filled by glr_plan_prepare (the first run, or
// origin_glr_plan_prepare ahead of it)
int alloc_norm_cube(origin_glr_plan *pl) {
  const size_t padded =
      ((size_t)pl->Nz + MF_PAD_FRONT + MF_PAD_BACK) * (size_t)pl->Ny * pl->Nx * sizeof(float);
  ORIGIN_HIP(hipMalloc((void **)&pl->d_normc, padded));
  ORIGIN_HIP(hipMemsetAsync(pl->d_normc, 0, padded, pl->ctx->stream));
  pl->bytes += padded;
  return ORIGIN_OK;
}

// mode 0: the list of border spaxels, 1/sqrt(den) per border class, its interior slice
int build_border_tables(origin_glr_plan *pl) {
  origin_ctx *ctx = pl->ctx;
  const int Nz = pl->Nz, Ny = pl->Ny, Nx = pl->Nx, P = pl->P, K = pl->K, NzP = pl->NzP;
  const size_t PP = (size_t)P * P;
  std::vector<int> border;
  const int c = P / 2;
  for (int y = 0; y < Ny; ++y)
    for (int x = 0; x < Nx; ++x)
      if (y < c || y > Ny - 1 - c || x < c || x > Nx - 1 - c) border.push_back(y * Nx + x);
  pl->nborder = (int)border.size();
  if (int rc = upload(ctx, border, &pl->d_border, &pl->bytes)) return rc;
  DevTmp ncls;
  const size_t ncls_n = (size_t)Nz * PP, rn = PP * (size_t)K * NzP;
  ORIGIN_HIP(ncls.alloc(ncls_n * sizeof(double)));
  ORIGIN_HIP(hipMalloc((void **)&pl->d_rden, rn * sizeof(float)));
  pl->bytes += rn * sizeof(float);
  hipLaunchKernelGGL(norm_classes_kernel, dim3(cdiv((long)ncls_n, 256)), dim3(256), 0, ctx->stream,
                     pl->d_k2, Nz, P, (double *)ncls.p);
  hipLaunchKernelGGL(rden_kernel, dim3(cdiv((long)rn, 256)), dim3(256), 0, ctx->stream,
                     (const double *)ncls.p, pl->d_taps2, pl->d_tap_off, K, Nz, (int)PP, NzP,
                     pl->d_rden);
  ORIGIN_LAUNCH_CHECK();
  // the interior class is a slice of the table
  pl->d_rdi = pl->d_rden + (size_t)((P / 2) * P + P / 2) * K * NzP;
  if (!pl->h_order.empty()) {  // the same slice in the kernel's processing order
    ORIGIN_HIP(hipMalloc((void **)&pl->d_rdi_s, (size_t)K * NzP * sizeof(float)));
    pl->bytes += (size_t)K * NzP * sizeof(float);
    for (int slot = 0; slot < K; ++slot)
      ORIGIN_HIP(hipMemcpyAsync(pl->d_rdi_s + (size_t)slot * NzP,
                                pl->d_rdi + (size_t)pl->h_order[slot] * NzP, NzP * sizeof(float),
                                hipMemcpyDeviceToDevice, ctx->stream));
  }
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));  // (ncls goes with this scope)
  return ORIGIN_OK;
}

// mode 0: the FOLD tables and their eps test; a plan that fails it (or has no FOLD range) drops them
int build_fold_tables(origin_glr_plan *pl, const std::vector<double> &fold_a) {
  origin_ctx *ctx = pl->ctx;
  const int K = pl->K, NzP = pl->NzP;
  const size_t PP = (size_t)pl->P * pl->P, rn = PP * (size_t)K * NzP, sn = PP * (size_t)NzP;
  int zf0, zf1;
  mf_fold_range(pl->Nz, &zf0, &zf1);
  if (pl->d_atab_fold && zf1 > zf0 && mf_fold_fits(K)) {
    std::vector<float> ainv(K + 1, 0.0f);  // 1/a_k, then the word the kernel's atomicMax starts from
    for (int kk = 0; kk < K; ++kk) ainv[kk] = (float)(1.0 / fold_a[kk]);
    DevTmp tmp;
    ORIGIN_HIP(tmp.alloc(ainv.size() * sizeof(float)));
    float *d_ainv = (float *)tmp.p;
    unsigned *d_eps = (unsigned *)(d_ainv + K), eps_bits = 0;
    ORIGIN_HIP(hipMemcpyAsync(d_ainv, ainv.data(), ainv.size() * sizeof(float),
                              hipMemcpyHostToDevice, ctx->stream));
    ORIGIN_HIP(hipMalloc((void **)&pl->d_rden_fold, rn * sizeof(float)));
    ORIGIN_HIP(hipMalloc((void **)&pl->d_sden, sn * sizeof(float)));
    hipLaunchKernelGGL(fold_tables_kernel, dim3(cdiv((long)sn, 256)), dim3(256), 0, ctx->stream,
                       pl->d_rden, d_ainv, K, (int)PP, NzP, zf0, zf1, pl->d_rden_fold, pl->d_sden,
                       d_eps);
    ORIGIN_LAUNCH_CHECK();
    ORIGIN_HIP(hipMemcpyAsync(&eps_bits, d_eps, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(&pl->fold_eps, &eps_bits, sizeof(float));
  }
  if (pl->d_rden_fold && pl->fold_eps <= MF_FOLD_EPS) {
    pl->bytes += (rn + sn) * sizeof(float);
  } else {  // no FOLD for this plan
    for (void **q : {(void **)&pl->d_atab_fold, (void **)&pl->d_atab_bf16_fold,
                     (void **)&pl->d_rden_fold, (void **)&pl->d_sden}) {
      if (*q) (void)hipFree(*q);
      *q = nullptr;
    }
  }
  return ORIGIN_OK;
}

}  // namespace

// ---- the launch geometry the two matrix-core spectral kernels share
int glr_range_resolve(const GlrRange &rg, int Ny, int Nx, int waves, GlrSpaxels *sp) {
  const GlrRange r = rg.y1 > 0 ? rg : GlrRange{0, Ny, 0, Nx};
  const bool rect = r.x0 > 0 || r.x1 < Nx;
  const long s_first = (long)r.y0 * Nx, s_end = (long)r.y1 * Nx;
  if (r.y0 < 0 || r.y0 >= r.y1 || r.y1 > Ny || (!rect && s_first % 32 != 0)) {
    origin_set_error("spectral MFMA stage: bad spaxel range");
    return ORIGIN_E_ARG;
  }
  if (r.x0 < 0 || r.x0 >= r.x1 || r.x1 > Nx) {
    origin_set_error("spectral MFMA stage: bad rectangle");
    return ORIGIN_E_ARG;
  }
  // columns (32 spaxels x one z chunk): one per wave
  const long ncols = rect ? (long)(r.y1 - r.y0) * cdiv(r.x1 - r.x0, 32) : cdiv(s_end - s_first, 32);
  *sp = {s_first, s_end, cdiv(ncols, waves), rect ? r.x0 : 0, rect ? r.x1 : 0};
  return ORIGIN_OK;
}

// One block per CU at a time (LDS): the number of z chunks is picked so that the blocks fill whole
// rounds of the chip -- useful channel slots / (rounds x CUs x (chunk length + ~one tile of
// start-up per block)); chunks are whole 32-channel tiles, at most 64 of them (partial maps).
GlrChunks glr_z_chunks(int num_cu, int Nz, long S, int waves) {
  const long bx = cdiv(S, 32 * waves);
  const int ncu = std::max(1, num_cu);
  int nzm = 1;
  double best_eff = 0.0;
  for (int n = 1; n <= std::min(64, std::max(1, cdiv(Nz, 64))); ++n) {
    const int zc = (cdiv(Nz, n) + 31) / 32 * 32;
    const long blocks = bx * cdiv(Nz, zc);
    const long rounds = (blocks + ncu - 1) / ncu;
    const double eff = (double)bx * Nz / ((double)rounds * ncu * (zc + 32));
    if (eff > best_eff * 1.0001) best_eff = eff, nzm = n;
  }
  const int zcm = (cdiv(Nz, nzm) + 31) / 32 * 32;
  return {cdiv(Nz, zcm), zcm};
}

int glr_part_rows(const origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form) {
  const long S = (long)pl->Ny * pl->Nx;
  if (form == GLR_SPEC_NORM_MFMA) return glr_z_chunks(ctx->num_cu, pl->Nz, S, NM_WAVES).n;
  int rows = glr_z_chunks(ctx->num_cu, pl->Nz, S, MF_WAVES).n;
  if (form == GLR_SPEC_NORMW) {
    int zf0, zf1;
    mf_fold_range(pl->Nz, &zf0, &zf1);
    rows += cdiv(zf0, 32) + cdiv(pl->Nz - zf1, 32);
  }
  return rows;
}

GlrPaths glr_paths_at(const origin_glr_plan *pl, int precision, bool no_fold) {
  GlrPaths p;
  p.prepared = pl->mode == 0 || (pl->normc_ready && pl->normw_checked);
  // the matrix-core stages need the plan's tap tables (weights=None) or its weight maps (a norm
  // cube without weight maps -- a field smaller than the PSF -- stays on the fp32 kernels)
  const bool mc = precision >= 1 && (pl->mode == 0 ? pl->d_atab != nullptr : pl->d_w != nullptr);
  p.spatial_mfma = mc && origin_spatial_mfma_ok(pl->Ny, pl->Nx, pl->P);
  // explicit norm cube: second Toeplitz product on the matrix cores
  const bool norm_tables = mc && pl->mode == 1 && pl->d_atab && pl->d_atab2 &&
                           pl->K <= origin_spectral_norm_mfma_max_k();
  // NORMW: the FOLD form of the table kernel on the norm cube where the plan's eps allows it (bf16
  // plans too: one bf16 MFMA per product), the two-product kernel (f16 split) for the 32 channels
  // at either end of the cube; the partial maps of both must fit their 64 rows
  int zf0, zf1;
  mf_fold_range(pl->Nz, &zf0, &zf1);
  const bool normw =
      norm_tables && pl->normw_checked && pl->fold_eps <= MF_FOLD_EPS && pl->d_atab_fold &&
      zf1 > zf0 && !no_fold && pl->K > 2 &&  // (the FOLD pair loop peels two pairs)
      glr_part_rows(pl->ctx, pl, GLR_SPEC_NORMW) <= 64;
  if (normw) p.spectral = GLR_SPEC_NORMW;
  else if (norm_tables && precision == 1) p.spectral = GLR_SPEC_NORM_MFMA;
  else if (mc && pl->mode == 0 && pl->d_rdi) p.spectral = GLR_SPEC_TABLE;
  else if (pl->mode == 0 && ((long)pl->Ny * pl->Nx & 1) == 0 && pl->lwt) p.spectral = GLR_SPEC_PACKED;
  else p.spectral = pl->lwmax <= 32 ? GLR_SPEC_FP32 : GLR_SPEC_GENERIC;
  return p;
}

// eps of the FOLD form on the norm cube (channel 0 at norm) the plan has just made
static int measure_normw_eps(origin_ctx *ctx, origin_glr_plan *pl, const float *norm) {
  pl->normw_checked = 1;
  pl->fold_eps = INFINITY;
  int zf0, zf1;
  mf_fold_range(pl->Nz, &zf0, &zf1);
  if (zf1 <= zf0 || pl->lwmax > 32) return ORIGIN_OK;
  const long S = (long)pl->Ny * pl->Nx;
  void *scr = nullptr;
  if (int rc = origin_scratch(ctx, 256, &scr)) return rc;
  unsigned *d_eps = (unsigned *)scr, bits = 0x7f800000u;
  ORIGIN_HIP(hipMemsetAsync(d_eps, 0, sizeof(unsigned), ctx->stream));
  hipLaunchKernelGGL(normw_eps_kernel, dim3((unsigned)cdiv(S, 256), (unsigned)cdiv(zf1 - zf0, NE_ZT)),
                     dim3(256), 0, ctx->stream, norm, pl->d_taps2, pl->d_tap_off, pl->K, S, zf0, zf1,
                     d_eps);
  ORIGIN_LAUNCH_CHECK();
  ORIGIN_HIP(hipMemcpyAsync(&bits, d_eps, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  memcpy(&pl->fold_eps, &bits, sizeof(float));
  return ORIGIN_OK;
}

int glr_plan_prepare(origin_ctx *ctx, origin_glr_plan *pl) {
  if (pl->mode != 1) return ORIGIN_OK;
  const int Nz = pl->Nz, Ny = pl->Ny, Nx = pl->Nx, P = pl->P;
  const size_t S = (size_t)Ny * Nx;
  float *norm = pl->d_normc + (size_t)MF_PAD_FRONT * S;
  if (!pl->normc_ready) {
    // norm_fsf depends on the PSFs and the weight maps only: made once, into the cube the plan
    // keeps (padded like cube_fsf; alloc_norm_cube zeroed the pads)
    ProfScope ps(ctx, K_GLR_SPATIAL);
    for (int f = 0; f < pl->nfields; ++f) {
      const float *wf = pl->d_w ? pl->d_w + (size_t)f * S : nullptr;
      const float *k2f = pl->d_k2 + (size_t)f * Nz * P * P;
      if (int rc = glr_fp32_spatial(ctx, nullptr, wf, k2f, Nz, Ny, Nx, P, f > 0, norm)) return rc;
    }
    pl->normc_ready = 1;
  }
  // NORMW: eps of the FOLD form, measured on that cube (plans without folded taps run the exact
  // forms whatever it would be)
  if (!pl->normw_checked) {
    if (pl->d_atab_fold) return measure_normw_eps(ctx, pl, norm);
    pl->normw_checked = 1;
  }
  return ORIGIN_OK;
}

extern "C" {

int origin_glr_plan_prepare(origin_ctx *ctx, origin_glr_plan *plan) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(plan && plan->ctx == ctx, "plan does not belong to this context");
  return glr_plan_prepare(ctx, plan);
}

int origin_glr_plan_destroy(origin_glr_plan *plan) {
  if (!plan) return ORIGIN_OK;
  (void)hipSetDevice(plan->ctx->device);
  (void)hipStreamSynchronize(plan->ctx->stream);
  for (void *p : {(void *)plan->d_k, (void *)plan->d_k2, (void *)plan->d_w, (void *)plan->d_taps,
                  (void *)plan->d_taps2, (void *)plan->d_tap_off, (void *)plan->d_rden,
                  (void *)plan->d_htaps, (void *)plan->d_htap_off, (void *)plan->d_rows,
                  (void *)plan->d_border, (void *)plan->d_atab, (void *)plan->d_atab_bf16,
                  (void *)plan->d_pwide, (void *)plan->d_rdi_s, (void *)plan->d_normc,
                  (void *)plan->d_atab2, (void *)plan->d_atab_fold, (void *)plan->d_atab_bf16_fold,
                  (void *)plan->d_rden_fold, (void *)plan->d_sden})
    if (p) (void)hipFree(p);
  delete plan;
  return ORIGIN_OK;
}

int origin_glr_plan_create(origin_ctx *ctx, int Nz, int Ny, int Nx, int nfields, int P,
                           const double *h_psf, const double *h_weights, int K,
                           const double *h_taps, const int *h_tap_off,
                           origin_glr_plan **out) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(out, "out is null");
  *out = nullptr;
  ORIGIN_CHECK_ARG(Nz > 0 && Ny > 0 && Nx > 0, "bad cube shape (%d,%d,%d)", Nz, Ny, Nx);
  ORIGIN_CHECK_ARG(nfields >= 1 && h_psf, "need at least one PSF");
  ORIGIN_CHECK_ARG(P >= 1 && (P & 1) && P <= 63, "PSF size %d unsupported (odd, <= 63)", P);
  ORIGIN_CHECK_ARG(K >= 1 && K <= 255 && h_taps && h_tap_off,
                   "need 1..255 profiles (profile index is uint8)");
  ORIGIN_CHECK_ARG(h_weights || nfields == 1, "several fields need weight maps");
  for (int k = 0; k < K; ++k)
    ORIGIN_CHECK_ARG(h_tap_off[k + 1] > h_tap_off[k], "profile %d is empty", k);

  std::unique_ptr<origin_glr_plan, PlanDeleter> owner(new origin_glr_plan());
  origin_glr_plan *pl = owner.get();
  pl->ctx = ctx;
  pl->Nz = Nz, pl->Ny = Ny, pl->Nx = Nx, pl->nfields = nfields, pl->P = P, pl->K = K;
  pl->mode = (h_weights == nullptr && Ny >= P && Nx >= P) ? 0 : 1;
  pl->NzP = (Nz + 31) / 32 * 32 + 32;  // the matrix-core spectral kernel reads whole 32-channel tiles
  pl->Kp = pl->NzP;

  Profiles prof;
  std::vector<double> fold_a;
  if (int rc = prepare_psfs(pl, h_psf, h_weights)) return rc;
  if (int rc = prepare_profiles(pl, h_taps, h_tap_off, &prof)) return rc;
  if (int rc = build_half_taps_and_rows(pl, prof)) return rc;
  if (pl->lwmax <= 32 && K <= MF_MAX_K && (pl->mode == 0 || h_weights)) {
    if (int rc = build_mfma_tap_tables(pl, prof, &fold_a)) return rc;
    pl->precision = 1;
  }
  // a mosaic of weighted fields: its spatial stage runs on the matrix cores too (per-field
  // accumulation, glr_spatial_mfma.hip) where its profiles leave the spectral stage in fp32
  if (h_weights && origin_spatial_mfma_ok(Ny, Nx, P)) pl->precision = 1;
  if (pl->mode == 1) {
    if (int rc = alloc_norm_cube(pl)) return rc;
  } else {
    ProfScope ps(ctx, K_GLR_TABLES);
    if (int rc = build_border_tables(pl)) return rc;
    if (int rc = build_fold_tables(pl, fold_a)) return rc;
  }
  *out = owner.release();
  return ORIGIN_OK;
}

int origin_glr_plan_set_precision(origin_glr_plan *plan, int precision) {
  ORIGIN_CHECK_ARG(plan && precision >= 0 && precision <= 2, "precision must be 0, 1 or 2");
  // eligible: at precision 1 some stage of the plan runs on the matrix cores
  const GlrPaths at1 = glr_paths_at(plan, 1, false);
  plan->precision = at1.spatial_mfma || at1.spectral_mfma() ? precision : 0;
  return ORIGIN_OK;
}

int origin_glr_plan_get_precision(origin_glr_plan *plan, int *precision) {
  ORIGIN_CHECK_ARG(plan && precision, "null argument");
  *precision = plan->precision;
  return ORIGIN_OK;
}

int origin_glr_plan_fold_eps(origin_glr_plan *plan, float *eps, int *active) {
  ORIGIN_CHECK_ARG(plan && eps && active, "null argument");
  *eps = plan->fold_eps;
  // (a plan with a norm cube measures eps in its first run or in origin_glr_plan_prepare: +inf
  // and inactive before that.  `active` is the verdict of the eps test, not the form that runs: glr_paths keeps a plan whose
  // eps passes on the exact kernels when it has one profile pair only, or -- with a norm cube --
  // when the partial maps of NORMW's three launches would not fit their 64 rows)
  *active = (plan->mode == 0 ? plan->d_rden_fold != nullptr
                             : plan->normw_checked && plan->d_atab_fold != nullptr &&
                                   plan->fold_eps <= MF_FOLD_EPS) &&
            !glr_no_fold();
  return ORIGIN_OK;
}

int origin_glr_plan_mfma_count(origin_glr_plan *plan, long *spatial, long *spectral) {
  ORIGIN_CHECK_ARG(plan && spatial && spectral, "null argument");
  const origin_glr_plan *pl = plan;
  *spatial = *spectral = 0;
  // (the counts model the table kernels: a plan with a norm cube reports none)
  const GlrPaths paths = glr_paths(pl, glr_no_fold());
  const int terms = pl->precision == 2 ? 1 : 3;
  if (pl->mode == 0 && paths.spatial_mfma)
    *spatial = origin_spatial_mfma_count(terms, pl->Nz, pl->Ny, pl->Nx, pl->P);
  if (paths.spectral == GLR_SPEC_TABLE)
    *spectral = origin_spectral_mfma_count(pl->ctx->num_cu, terms, pl->K, pl->n_narrow, pl->Nz,
                                           pl->Ny, pl->Nx);
  return ORIGIN_OK;
}

int origin_glr_mfma_count_model(int num_cu, int terms, int K, int n_narrow, int Nz, int Ny, int Nx,
                                int P, long *spatial, long *spectral) {
  ORIGIN_CHECK_ARG(spatial && spectral && num_cu > 0 && (terms == 1 || terms == 3) && K > 0 &&
                       n_narrow >= 0 && n_narrow <= K && Nz > 0 && Ny > 0 && Nx > 0 && P > 0,
                   "bad arguments");
  *spatial = origin_spatial_mfma_ok(Ny, Nx, P) ? origin_spatial_mfma_count(terms, Nz, Ny, Nx, P) : 0;
  *spectral = origin_spectral_mfma_count(num_cu, terms, K, n_narrow, Nz, Ny, Nx);
  return ORIGIN_OK;
}

int origin_glr_plan_paths(origin_glr_plan *plan, int *spatial_mfma, int *spectral, int *lwt,
                          int *lwmax, int *nborder) {
  ORIGIN_CHECK_ARG(plan && spatial_mfma && spectral && lwt && lwmax && nborder, "null argument");
  const GlrPaths paths = glr_paths(plan, glr_no_fold());
  *spatial_mfma = paths.spatial_mfma ? 1 : 0;
  *spectral = (int)paths.spectral;
  *lwt = plan->lwt;
  *lwmax = plan->lwmax;
  *nborder = plan->nborder;
  return ORIGIN_OK;
}

int origin_glr_plan_bytes(origin_glr_plan *plan, size_t *bytes) {
  ORIGIN_CHECK_ARG(plan && bytes, "null argument");
  *bytes = plan->bytes;
  return ORIGIN_OK;
}

int origin_glr_work_elems(origin_glr_plan *plan, size_t *elems) {
  ORIGIN_CHECK_ARG(plan && elems, "null argument");
  // (the norm cube of mode 1 belongs to the plan)
  *elems = GlrWork::elems(plan);
  return ORIGIN_OK;
}

int origin_glr_rows_supported(origin_glr_plan *plan, int *ok) {
  ORIGIN_CHECK_ARG(plan && ok, "null argument");
  *ok = glr_paths(plan, glr_no_fold()).rows_ok() ? 1 : 0;
  return ORIGIN_OK;
}

}  // extern "C"
