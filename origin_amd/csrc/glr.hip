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

// spatial stage over the 64 x 64 regions that hold rg (the whole field on the fp32 kernel):
// cube_fsf, the fields of a weighted mosaic accumulated one by one
int run_spatial(origin_ctx *ctx, origin_glr_plan *pl, bool on_mfma, const float *d_cube, float *fsf,
                const GlrRange &rg) {
  const int Nz = pl->Nz, Ny = pl->Ny, Nx = pl->Nx, P = pl->P;
  const size_t S = (size_t)Ny * Nx;
  for (int f = 0; f < pl->nfields; ++f) {
    ProfScope ps(ctx, K_GLR_SPATIAL);
    const float *kf = pl->d_k + (size_t)f * Nz * P * P;
    const float *wf = pl->d_w ? pl->d_w + (size_t)f * S : nullptr;
    // matrix cores, two-term f16 split (glr_spatial_mfma.hip); weighted fields accumulate
    // (regions ry0, nry, rx0, nrx; none = all)
    int rc = on_mfma
                 ? origin_spatial_mfma_launch(ctx, pl->precision == 2 ? 1 : 3, d_cube, wf, kf, Nz,
                                              Ny, Nx, P, wf && f > 0, fsf, rg.y0 / 64,
                                              cdiv(rg.y1 - rg.y0, 64), rg.x0 / 64,
                                              cdiv(rg.x1 - rg.x0, 64))
                 : glr_fp32_spatial(ctx, d_cube, wf, kf, Nz, Ny, Nx, P, f > 0, fsf);
    if (rc) return rc;
  }
  return ORIGIN_OK;
}

// the partial maps of a run of `form` in io.part: glr_part_rows rows of maxima, then of minima
void lay_out_maps(const origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form,
                  GlrSpectralIO *io) {
  io->nzc = glr_part_rows(ctx, pl, form);
  io->pmax = io->want_maps ? io->part : nullptr;
  io->pmin = io->want_maps ? io->part + (size_t)io->nzc * pl->Ny * pl->Nx : nullptr;
}

// the matrix-core spectral stage of the plan's form over the spaxels of rg (a band or rectangle:
// the rows of the partial maps are the whole field's)
int run_spectral_mfma(origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form, bool no_fold,
                      GlrSpectralIO *io, const GlrRange &rg) {
  lay_out_maps(ctx, pl, form, io);
  if (form == GLR_SPEC_NORM_MFMA) return origin_spectral_norm_mfma_launch(ctx, pl, *io, rg);
  const bool normw = form == GLR_SPEC_NORMW;
  SpectralMfmaArgs a = glr_spectral_mfma_args(pl, io, normw || !no_fold);
  a.range = rg;
  if (!normw) return origin_spectral_mfma_launch(ctx, a);
  // NORMW: the FOLD form of the table kernel between the ends of the cube, the two-product kernel
  // for the 32 channels at either end; the partial maps of the ends follow those of the middle
  a.rden = a.rdi_s = a.rden_fold = a.sden = nullptr;  // (no class tables: the norm cube instead)
  a.normc = io->norm;
  if (int rc = origin_spectral_mfma_launch(ctx, a)) return rc;
  return origin_spectral_norm_mfma_launch_ends(ctx, pl, *io, rg,
                                               glr_part_rows(ctx, pl, GLR_SPEC_TABLE));
}

}  // namespace

SpectralMfmaArgs glr_spectral_mfma_args(const origin_glr_plan *pl, const GlrSpectralIO *io,
                                        bool fold) {
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
  const GlrRange rg = {y0, y1, x0, x1};
  int rc = run_spatial(ctx, pl, true, d_cube, work.fsf, rg);
  if (rc == ORIGIN_OK) {
    ProfScope ps(ctx, K_GLR_SPECTRAL);
    const float *norm = pl->mode == 1 ? pl->d_normc + (size_t)MF_PAD_FRONT * Ny * Nx : nullptr;
    GlrSpectralIO io = {work.fsf, norm, d_mask, d_correl, d_profile, d_correl_min, work.part, true};
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
  io.part = GlrWork(pl, d_work).part, io.want_maps = true;
  lay_out_maps(ctx, pl, glr_paths(pl, glr_no_fold()).spectral, &io);  // (the form the bands ran)
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
  const GlrRange whole;
  if (int rc = run_spatial(ctx, pl, paths.spatial_mfma, d_cube, work.fsf, whole)) return rc;

  // ---- spectral stage
  GlrSpectralIO io = {work.fsf, norm, d_mask, d_correl, d_profile, d_correl_min, work.part,
                      d_maxmap || d_minmap};
  {
    ProfScope ps(ctx, K_GLR_SPECTRAL);
    int rc = paths.spectral_mfma() ? run_spectral_mfma(ctx, pl, paths.spectral, no_fold, &io, whole)
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
