// GLR matched-filter correlation  (SURVEY.md 2.2 rows k8-k12).
//
// Replaces Correlation_GLR_test (reference muse_origin/lib_origin.py:1070-1217, helpers
// _convolve_fsf :1027-1043 and _convolve_profile :1046-1060) and the dense lines of
// ComputeTGLR.run (steps.py:781-793).  The reference evaluates everything with FFTs; the
// kernels below evaluate the same algebra directly (verified against the
// reference to 1e-15 by oracle/gen_golden.py "direct algebra"):
//
//   cube_fsf[z,y,x] = sum_f sum_{dy,dx} k_fz[dy,dx] (w_f cube)[z, y+dy-c, x+dx-c]
//   norm_fsf[z,y,x] = sum_f sum_{dy,dx} k_fz[dy,dx]^2 w_f[y+dy-c, x+dx-c]
//   num_k[z] = sum_j p_k[j] cube_fsf[z + lw_k - j]
//   den_k[z] = sum_j p_k[j]^2 norm_fsf[z + lw_k - j]
//   T_k = num_k / sqrt(den_k)   (den_k <= 0 -> 0);  correl = max_k, correl_min = min_k,
//   profile = first argmax_k
//
// with k = PSF - mean(PSF), c = P/2 and zeros outside the cube.
//
// Normalisation.  With weights=None, norm_fsf[z,y,x] depends on (y,x) only through how the
// PSF window is clipped by the field border: P*P "border classes" (class (c,c) = interior).
// The plan tabulates 1/sqrt(den_k[z]) per class once, so the hot kernel never touches a
// second cube.  With field weights (or fields smaller than the PSF) norm_fsf is a real
// cube, produced by the same stencil kernel, and den_k is convolved next to num_k.
//
// glr_plan.hip builds the plan and says which kernels a plan runs (glr_paths); the fp32 kernels are
// in glr_fp32.hip, the matrix-core ones in glr_spatial_mfma.hip, glr_spectral_mfma.hip and
// glr_spectral_norm_mfma.hip.  This file holds the runs.
#include <algorithm>

#include "glr_plan.h"

namespace {

__global__ __launch_bounds__(256) void maxmap_final_kernel(const float *__restrict__ part_max,
                                                           const float *__restrict__ part_min,
                                                           int nzc, long S,
                                                           float *__restrict__ maxmap,
                                                           float *__restrict__ minmap) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  float a = -INFINITY, b = INFINITY;
  for (int k = 0; k < nzc; ++k) {
    a = fmaxf(a, part_max[(long)k * S + s]);
    b = fminf(b, part_min[(long)k * S + s]);
  }
  if (maxmap) maxmap[s] = a;
  if (minmap) minmap[s] = b;
}

int launch_maxmap_final(origin_ctx *ctx, const GlrSpectralIO &io, long S, float *d_maxmap,
                        float *d_minmap) {
  hipLaunchKernelGGL(maxmap_final_kernel, dim3(cdiv(S, 256)), dim3(256), 0, ctx->stream, io.pmax,
                     io.pmin, io.nzc, S, d_maxmap, d_minmap);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// the zero channels around cube_fsf
int zero_pads(origin_ctx *ctx, const origin_glr_plan *pl, float *d_work, const GlrWork &w) {
  const size_t S = (size_t)pl->Ny * pl->Nx;
  ORIGIN_HIP(hipMemsetAsync(d_work, 0, MF_PAD_FRONT * S * sizeof(float), ctx->stream));
  ORIGIN_HIP(hipMemsetAsync(w.back_pad, 0, MF_PAD_BACK * S * sizeof(float), ctx->stream));
  return ORIGIN_OK;
}

// spatial stage over the whole field (regions: the 64 x 64 regions ry0 .. / rx0 .. of the matrix-core
// kernel, nry <= 0 = all): cube_fsf, the fields of a weighted mosaic accumulated one by one
int run_spatial(origin_ctx *ctx, origin_glr_plan *pl, bool on_mfma, const float *d_cube, float *fsf,
                int ry0 = 0, int nry = 0, int rx0 = 0, int nrx = 0) {
  const int Nz = pl->Nz, Ny = pl->Ny, Nx = pl->Nx, P = pl->P;
  const size_t S = (size_t)Ny * Nx;
  for (int f = 0; f < pl->nfields; ++f) {
    ProfScope ps(ctx, K_GLR_SPATIAL);
    const float *kf = pl->d_k + (size_t)f * Nz * P * P;
    const float *wf = pl->d_w ? pl->d_w + (size_t)f * S : nullptr;
    // matrix cores, two-term f16 split (glr_spatial_mfma.hip); weighted fields accumulate
    int rc = on_mfma
                 ? origin_spatial_mfma_launch(ctx, pl->precision == 2 ? 1 : 3, d_cube, wf, kf, Nz,
                                              Ny, Nx, P, wf && f > 0, fsf, ry0, nry, rx0, nrx)
                 : glr_fp32_spatial(ctx, d_cube, wf, kf, Nz, Ny, Nx, P, f > 0, fsf);
    if (rc) return rc;
  }
  return ORIGIN_OK;
}

// NORMW: rows of each partial map -- the table kernel's z chunks, then the 32-channel end tiles
int normw_part_rows(const origin_ctx *ctx, const origin_glr_plan *pl) {
  int zf0, zf1;
  mf_fold_range(pl->Nz, &zf0, &zf1);
  return origin_spectral_mfma_chunks(ctx->num_cu, pl->Nz, pl->Ny, pl->Nx) + cdiv(zf0, 32) +
         cdiv(pl->Nz - zf1, 32);
}

// NORMW: the FOLD form of the table kernel between the ends of the cube, the two-product kernel
// for the 32 channels at either end; the partial maps of the ends follow those of the middle.
// rg: the spaxels of a band or rectangle (the rows of the partial maps are the whole field's)
int run_spectral_normw(origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectralIO *io,
                       const NmRange &rg) {
  int zf0, zf1;
  mf_fold_range(pl->Nz, &zf0, &zf1);
  SpectralMfmaArgs a = glr_spectral_mfma_args(pl, io, true);
  a.rden = a.rdi_s = a.rden_fold = a.sden = nullptr;  // (no class tables: the norm cube instead)
  a.normc = io->norm;
  a.part_rows = normw_part_rows(ctx, pl);
  a.s_first = rg.s_first, a.s_count = rg.s_count, a.rx0 = rg.rx0, a.rx1 = rg.rx1;
  if (int rc = origin_spectral_mfma_launch(ctx, a)) return rc;
  int got = 0;
  int rc = origin_spectral_norm_mfma_launch_ends(
      ctx, io->fsf, io->norm, pl->d_atab, pl->d_atab2, pl->d_pwide, pl->K, pl->Nz, pl->Ny, pl->Nx,
      io->mask, io->correl, io->profile, io->correl_min, io->pmax, io->pmin, zf0, zf1, io->nzc, &got,
      rg);
  io->nzc += got;
  return rc;
}

// the matrix-core spectral stage of the plan's form over the spaxels of rg
int run_spectral_mfma(origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form, bool no_fold,
                      GlrSpectralIO *io, const NmRange &rg) {
  switch (form) {
    case GLR_SPEC_NORMW:
      return run_spectral_normw(ctx, pl, io, rg);
    case GLR_SPEC_NORM_MFMA:
      return origin_spectral_norm_mfma_launch(ctx, io->fsf, io->norm, pl->d_atab, pl->d_atab2,
                                              pl->d_pwide, pl->K, pl->Nz, pl->Ny, pl->Nx, io->mask,
                                              io->correl, io->profile, io->correl_min, io->part,
                                              io->want_maps, &io->nzc, &io->pmax, &io->pmin, rg);
    default: {
      SpectralMfmaArgs a = glr_spectral_mfma_args(pl, io, !no_fold);
      a.s_first = rg.s_first, a.s_count = rg.s_count, a.rx0 = rg.rx0, a.rx1 = rg.rx1;
      return origin_spectral_mfma_launch(ctx, a);
    }
  }
}

}  // namespace

SpectralMfmaArgs glr_spectral_mfma_args(const origin_glr_plan *pl, GlrSpectralIO *io, bool fold) {
  const bool b16 = pl->precision == 2;
  SpectralMfmaArgs a;
  a.io = io;
  a.terms = b16 ? 1 : 3;
  a.atab = b16 ? pl->d_atab_bf16 : pl->d_atab;
  a.atab_fold = !fold ? nullptr : b16 ? pl->d_atab_bf16_fold : pl->d_atab_fold;
  a.rden = pl->d_rden, a.rdi_s = pl->d_rdi_s;
  a.rden_fold = fold ? pl->d_rden_fold : nullptr, a.sden = fold ? pl->d_sden : nullptr;
  a.pinfo = pl->d_pwide;
  a.NzP = pl->NzP, a.K = pl->K, a.n_narrow = pl->n_narrow, a.ident = pl->order_ident;
  a.Nz = pl->Nz, a.Ny = pl->Ny, a.Nx = pl->Nx, a.P = pl->P;
  return a;
}

extern "C" {

int origin_glr_run_rows(origin_ctx *ctx, origin_glr_plan *pl, const float *d_cube,
                        const uint8_t *d_mask, float *d_work, float *d_correl, uint8_t *d_profile,
                        float *d_correl_min, int y0, int y1, int flags) {
  return origin_glr_run_rect(ctx, pl, d_cube, d_mask, d_work, d_correl, d_profile, d_correl_min, y0,
                             y1, 0, pl ? pl->Nx : 0, flags);
}

// ---- a GLR run in row bands (plans whose two stages run on the matrix cores; a plan with a norm
// cube after origin_glr_plan_prepare: the band makes neither the cube nor its eps)
int origin_glr_run_rect(origin_ctx *ctx, origin_glr_plan *pl, const float *d_cube,
                        const uint8_t *d_mask, float *d_work, float *d_correl, uint8_t *d_profile,
                        float *d_correl_min, int y0, int y1, int x0, int x1, int flags) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(pl && pl->ctx == ctx, "plan does not belong to this context");
  ORIGIN_CHECK_ARG(d_cube && d_work && d_correl && d_profile && d_correl_min, "null pointer");
  const int Ny = pl->Ny, Nx = pl->Nx;
  ORIGIN_CHECK_ARG(y0 >= 0 && y0 < y1 && y1 <= Ny && y0 % 64 == 0 && (y1 % 64 == 0 || y1 == Ny),
                   "row band must start at a multiple of 64 and end at one or at Ny");
  ORIGIN_CHECK_ARG(x0 >= 0 && x0 < x1 && x1 <= Nx && x0 % 64 == 0 && (x1 % 64 == 0 || x1 == Nx),
                   "column range must start at a multiple of 64 and end at one or at Nx");
  const bool whole_rows = x0 == 0 && x1 == Nx;  // (then the waves are those of a run over the field)
  const bool no_fold = glr_no_fold();
  const GlrPaths paths = glr_paths(pl, no_fold);
  if (!paths.prepared) {
    origin_set_error("origin_glr_run_rows: a plan with a norm cube runs in bands after "
                     "origin_glr_plan_prepare");
    return ORIGIN_E_STATE;
  }
  if (!paths.rows_ok()) {
    origin_set_error("origin_glr_run_rows: the plan's stages do not run the matrix-core kernels");
    return ORIGIN_E_STATE;
  }
  const GlrWork work(pl, d_work);
  const bool side = (flags & ORIGIN_GLR_SIDE) != 0;
  if (flags & ORIGIN_GLR_FIRST)  // (main stream: before any band)
    if (int rc = zero_pads(ctx, pl, d_work, work)) return rc;
  // the launch functions enqueue on ctx->stream: the side stream takes its place for this band
  if (side) {
    if (int rc = origin_fork_begin(ctx, ctx->side, origin_make_side_stream)) return rc;
    std::swap(ctx->stream, ctx->side.stream);
  }
  int rc = run_spatial(ctx, pl, true, d_cube, work.fsf, y0 / 64, cdiv(y1 - y0, 64), x0 / 64,
                       cdiv(x1 - x0, 64));
  if (rc == ORIGIN_OK) {
    ProfScope ps(ctx, K_GLR_SPECTRAL);
    const float *norm = pl->mode == 1 ? pl->d_normc + (size_t)MF_PAD_FRONT * Ny * Nx : nullptr;
    GlrSpectralIO io = {work.fsf, norm, d_mask, d_correl, d_profile, d_correl_min, work.part, true};
    NmRange rg;
    rg.s_first = (long)y0 * Nx, rg.s_count = (long)(y1 - y0) * Nx;
    if (!whole_rows) rg.rx0 = x0, rg.rx1 = x1;
    rc = run_spectral_mfma(ctx, pl, paths.spectral, no_fold, &io, rg);
  }
  if (side) {
    std::swap(ctx->stream, ctx->side.stream);
    if (rc == ORIGIN_OK) rc = origin_fork_end(ctx->side);
  }
  return rc;
}

int origin_glr_run_finish(origin_ctx *ctx, origin_glr_plan *pl, float *d_work, float *d_maxmap,
                          float *d_minmap) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(pl && pl->ctx == ctx && d_work, "bad argument");
  if (int rc = origin_fork_join(ctx, ctx->side)) return rc;  // bands on the side stream
  if (!d_maxmap && !d_minmap) return ORIGIN_OK;
  const long S = (long)pl->Ny * pl->Nx;
  GlrSpectralIO io = {};
  // the rows of each partial map: those of the form the bands ran
  switch (glr_paths(pl, glr_no_fold()).spectral) {
    case GLR_SPEC_NORMW:
      io.nzc = normw_part_rows(ctx, pl);
      break;
    case GLR_SPEC_NORM_MFMA:
      io.nzc = origin_spectral_norm_mfma_chunks(ctx->num_cu, pl->Nz, pl->Ny, pl->Nx);
      break;
    default:
      io.nzc = origin_spectral_mfma_chunks(ctx->num_cu, pl->Nz, pl->Ny, pl->Nx);
  }
  io.pmax = GlrWork(pl, d_work).part;
  io.pmin = io.pmax + (size_t)io.nzc * S;
  ProfScope ps(ctx, K_SMALL);
  return launch_maxmap_final(ctx, io, S, d_maxmap, d_minmap);
}

int origin_glr_run(origin_ctx *ctx, origin_glr_plan *pl, const float *d_cube,
                   const uint8_t *d_mask, float *d_work, float *d_correl,
                   uint8_t *d_profile, float *d_correl_min, float *d_maxmap,
                   float *d_minmap) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(pl && pl->ctx == ctx, "plan does not belong to this context");
  ORIGIN_CHECK_ARG(d_cube && d_work && d_correl && d_profile && d_correl_min, "null pointer");
  const long S = (long)pl->Ny * pl->Nx;
  const bool no_fold = glr_no_fold();
  const GlrWork work(pl, d_work);
  // a plan with a norm cube: its first run makes the cube and measures eps of the FOLD form on it
  // (nothing once origin_glr_plan_prepare or an earlier run has)
  if (int rc = glr_plan_prepare(ctx, pl)) return rc;
  const float *norm = pl->mode == 1 ? pl->d_normc + (size_t)MF_PAD_FRONT * S : nullptr;
  // (asked now: the eps just measured decides between NORMW and two products)
  const GlrPaths paths = glr_paths(pl, no_fold);
  if (int rc = zero_pads(ctx, pl, d_work, work)) return rc;
  if (int rc = run_spatial(ctx, pl, paths.spatial_mfma, d_cube, work.fsf)) return rc;

  // ---- spectral stage
  GlrSpectralIO io = {work.fsf, norm, d_mask, d_correl, d_profile, d_correl_min, work.part,
                      d_maxmap || d_minmap};
  {
    ProfScope ps(ctx, K_GLR_SPECTRAL);
    int rc = paths.spectral_mfma()
                 ? run_spectral_mfma(ctx, pl, paths.spectral, no_fold, &io, NmRange())
                 : glr_fp32_spectral(ctx, pl, paths.spectral, &io, &ps);
    if (rc) return rc;
  }
  if (!io.want_maps) return ORIGIN_OK;
  ProfScope ps(ctx, K_SMALL);
  if (int rc = launch_maxmap_final(ctx, io, S, d_maxmap, d_minmap)) return rc;
  if (paths.spectral == GLR_SPEC_PACKED && pl->nborder > 0)
    return glr_fp32_border_maps(ctx, pl, d_correl, d_correl_min, d_maxmap, d_minmap);
  return ORIGIN_OK;
}

}  // extern "C"
