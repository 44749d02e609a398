// The GLR plan, the table of what a plan runs, and the launch functions of the GLR stages: shared
// by glr_plan.hip (plan), glr.hip (runs), glr_fp32.hip and the matrix-core kernels.
#pragma once
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "glr_tables.h"

struct origin_glr_plan {
  origin_ctx *ctx = nullptr;
  int Nz = 0, Ny = 0, Nx = 0, nfields = 0, P = 0, K = 0;
  int mode = 0;   // 0 = border-class table (weights=None), 1 = explicit norm cube
  int lwmax = 0;  // largest profile half width
  float *d_k = nullptr;     // [F][Nz][P][P]  zero-mean PSF
  float *d_k2 = nullptr;    // [F][Nz][P][P]  its square
  float *d_w = nullptr;     // [F][Ny][Nx] or null
  float *d_taps = nullptr;  // concatenated profiles (odd lengths; even ones padded with a 0 tap)
  float *d_taps2 = nullptr; // squares
  int *d_tap_off = nullptr; // [K+1]
  float *d_rden = nullptr;  // mode 0: [P*P][K][NzP]  1/sqrt(den) per border class (0 for z >= Nz)
  int Kp = 0;               // z stride of d_rden (= NzP)
  int symmetric = 0;   // every prepared profile is exactly symmetric about its centre
  float *d_htaps = nullptr;  // symmetric case: half profiles h_k[d] = p_k[lw_k + d], d = 0..lw_k
  int *d_htap_off = nullptr; // [K+1]
  float *d_rows = nullptr;   // [K+1][RL] rows (lw, p[0..2 lw]) for spectral3_kernel<LWT>
  float *d_rdi = nullptr;    // mode 0: interior-class slice of d_rden, [K][NzP] (not owned)
  int *d_border = nullptr;   // mode 0: flat indices of the spaxels whose border class is not interior
  int nborder = 0;
  int lwt = 0;         // template half width chosen for d_rows (8, 16, 24, 29 or 32; 0 = none)
  int NzP = 0;
  uint4 *d_atab = nullptr;   // matrix-core spectral stage: shifted hi/lo f16 tap copies (glr_tables.h)
  uint4 *d_atab_bf16 = nullptr;  // the same with bf16 taps (precision 2)
  uint4 *d_atab2 = nullptr;      // the squared taps in the same layout (plans with an explicit norm cube)
  int *d_pwide = nullptr;  // [K] processing order, narrow first: original index | (half width > 16) << 8
  int n_narrow = 0;    // number of narrow profiles (the first n_narrow slots)
  int order_ident = 0; // the processing order is the caller's order (slot = index)
  float *d_rdi_s = nullptr;  // interior-class 1/sqrt(den) in processing order [slot][NzP]
  // FOLD (glr_spectral_mfma.hip): taps times a_k = 1/sqrt(sum p_k^2), the table 1/(a_k sqrt(den))
  // [P*P][K][NzP], the class factors s [P*P][NzP]; fold_eps = max |1/(a_k sqrt(den)) / s - 1| over
  // the FOLD channels (the tables are dropped when it exceeds MF_FOLD_EPS; +inf: not measured)
  uint4 *d_atab_fold = nullptr, *d_atab_bf16_fold = nullptr;
  float *d_rden_fold = nullptr, *d_sden = nullptr;
  float fold_eps = INFINITY;
  // mode 1 (explicit norm cube): 1 once glr_plan_prepare has measured eps on the norm cube (then
  // fold_eps holds it) -- NORMW runs where it is <= MF_FOLD_EPS
  int normw_checked = 0;
  std::vector<int> h_order;  // processing order on the host (empty: no matrix-core tap tables)
  int precision = 0;  // 0 = fp32 FMA kernels, 1 = split-f16 MFMA stages, 2 = bf16 MFMA stages
  float *d_normc = nullptr;  // mode 1: norm_fsf [Nz][Ny][Nx], a constant of the plan (PSFs and weight
                             // maps only): allocated with the plan, computed by glr_plan_prepare and kept
  int normc_ready = 0;
  size_t bytes = 0;
};

// ---- what a plan runs: the ONE place that decides it (run, row bands, MFMA counts, precision)
enum GlrSpectral {
  GLR_SPEC_TABLE,      // matrix cores, 1/sqrt(den) from the border-class tables (FOLD where it holds)
  GLR_SPEC_NORMW,      // norm cube: FOLD form of the table kernel, two-product kernel at the ends
  GLR_SPEC_NORM_MFMA,  // norm cube: two Toeplitz products on the matrix cores
  GLR_SPEC_PACKED,     // fp32, two spaxels per lane, interior class + border pass
  GLR_SPEC_FP32,       // fp32, register window of half width 8 / 16 / 32
  GLR_SPEC_GENERIC     // fp32, plain loops (profiles wider than 32)
};
struct GlrPaths {
  bool spatial_mfma;  // the spatial stage runs on the matrix cores
  GlrSpectral spectral;
  bool prepared;  // no norm cube, or the plan has made it and measured its eps (glr_plan_prepare)
  bool spectral_mfma() const { return spectral <= GLR_SPEC_NORM_MFMA; }
  // runs in row bands / rectangles: both stages on the matrix cores, and whatever the spectral
  // stage reads besides cube_fsf exists before the first band
  bool rows_ok() const { return prepared && spatial_mfma && spectral_mfma(); }
};
// ORIGIN_GLR_NO_FOLD=1: the exact form everywhere (read per call: tests set it within a process)
inline bool glr_no_fold() { return getenv("ORIGIN_GLR_NO_FOLD") != nullptr; }
GlrPaths glr_paths_at(const origin_glr_plan *pl, int precision, bool no_fold);  // at a precision
inline GlrPaths glr_paths(const origin_glr_plan *pl, bool no_fold) {
  return glr_paths_at(pl, pl->precision, no_fold);
}

// ---- the work buffer of a run: [pad | cube_fsf | pad | partial maps]; the pads are MF_PAD_FRONT
// and MF_PAD_BACK zero channels, the partial maps <= 64 rows each of maxima and minima
struct GlrWork {
  float *fsf, *back_pad, *part;
  GlrWork(const origin_glr_plan *pl, float *d_work) {
    const size_t S = (size_t)pl->Ny * pl->Nx;
    fsf = d_work + MF_PAD_FRONT * S;
    back_pad = fsf + (size_t)pl->Nz * S;
    part = back_pad + MF_PAD_BACK * S;
  }
  static size_t elems(const origin_glr_plan *pl) {
    const size_t S = (size_t)pl->Ny * pl->Nx;
    return (size_t)pl->Nz * S + 2 * 64 * S + (MF_PAD_FRONT + MF_PAD_BACK) * S;
  }
};

// glr_plan.hip: what a plan with a norm cube owes before its spectral form is known -- the norm
// cube, then eps of the FOLD form on it -- on the main stream (the eps read-back synchronises it);
// once per plan, nothing for the others.  origin_glr_plan_prepare and origin_glr_run.
int glr_plan_prepare(origin_ctx *ctx, origin_glr_plan *pl);

// ---- glr_fp32.hip: the fp32 FMA kernels
// out (+)= corr2(A * B, taps) per channel; A == NULL: the norm of the weights B
int glr_fp32_spatial(origin_ctx *ctx, const float *A, const float *B, const float *taps, int Nz,
                     int Ny, int Nx, int P, int accumulate, float *out);
// what the spectral stage reads and writes, whatever kernel runs it.  The partial maps: nzc rows
// each at pmax / pmin (null without want_maps) -- the matrix-core forms get them from the driver
// before their launches (glr_part_rows), the fp32 forms report their own
struct GlrSpectralIO {
  const float *fsf, *norm;  // padded cubes, channel 0 (norm: plans with a norm cube)
  const uint8_t *mask;
  float *correl;
  uint8_t *profile;
  float *correl_min;
  float *part;
  bool want_maps;
  int nzc = 0;
  float *pmax = nullptr, *pmin = nullptr;
};
// forms PACKED (with its border pass, timed as K_GLR_BORDER), FP32 and GENERIC
int glr_fp32_spectral(origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form,
                      GlrSpectralIO *io, ProfScope *ps);
// PACKED: the maps of the border spaxels from the final cubes (behind maxmap_final_kernel)
int glr_fp32_border_maps(origin_ctx *ctx, const origin_glr_plan *pl, const float *correl,
                         const float *correl_min, float *maxmap, float *minmap);

// ---- the matrix-core spectral stage (glr_spectral_mfma.hip, glr_spectral_norm_mfma.hip)
// The spaxels of a launch: rows y0 .. y1 - 1 and columns x0 .. x1 - 1 of the field, as
// origin_glr_run_rect takes them; y1 == 0: the whole field.  The spatial stage runs the 64 x 64
// regions that hold them, the spectral stage what glr_range_resolve makes of them.
struct GlrRange {
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
};
// What a spectral kernel is given: with whole rows the spaxels [s_first, s_end) -- the waves hold
// the 32 spaxels they hold in a launch over the field, so s_first is a multiple of 32 -- and
// rx0 = rx1 = 0; with a proper column range a rectangle, columns rx0 .. rx1 - 1 of the rows
// s_first / Nx .. s_end / Nx - 1, a wave holding 32 consecutive columns of one row.  bx: blocks of
// `waves` waves along x.
struct GlrSpaxels {
  long s_first, s_end, bx;
  int rx0, rx1;
};
int glr_range_resolve(const GlrRange &rg, int Ny, int Nx, int waves, GlrSpaxels *sp);
// z chunks of a launch over all channels, for blocks of `waves` waves of 32 spaxels: n chunks of
// len channels.  Those of the WHOLE field of S spaxels, whatever part of it a launch takes: the
// partial maps of all parts of a run share their layout and a band's z tiles are the whole run's.
struct GlrChunks {
  int n, len;
};
GlrChunks glr_z_chunks(int num_cu, int Nz, long S, int waves);
// rows of each partial map of a run of this form: the kernel's z chunks; NORMW: the table
// kernel's, then the 32-channel end tiles of the two-product kernel
int glr_part_rows(const origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form);

// glr_spectral_mfma.hip
struct SpectralMfmaArgs {
  // cube and outputs
  const GlrSpectralIO *io;
  // tables (fold: nullptr = the exact form everywhere)
  int terms;  // 3: f16 split, 1: bf16
  const uint4 *atab, *atab_fold;
  const float *rden, *rdi_s, *rden_fold, *sden;
  const int *pinfo;
  int NzP, K, n_narrow, ident;
  // geometry
  int Nz, Ny, Nx, P;
  GlrRange range;
  // NORMW: the norm cube
  const float *normc = nullptr;
};
// the tables of the plan's precision; fold: bring the folded tables too
SpectralMfmaArgs glr_spectral_mfma_args(const origin_glr_plan *pl, const GlrSpectralIO *io,
                                        bool fold);
int origin_spectral_mfma_launch(origin_ctx *ctx, const SpectralMfmaArgs &a);
long origin_spectral_mfma_count(int num_cu, int terms, int K, int n_narrow, int Nz, int Ny,
                                int Nx);

// glr_spectral_norm_mfma.hip: the same stage for plans with an explicit norm cube
int origin_spectral_norm_mfma_max_k();
int origin_spectral_norm_mfma_launch(origin_ctx *ctx, const origin_glr_plan *pl,
                                     const GlrSpectralIO &io, const GlrRange &rg);
// the end tiles [0, zf0) and [zf1, Nz) of a plan whose other channels run NORMW (mf_fold_range);
// their partial maps from row prow0 on
int origin_spectral_norm_mfma_launch_ends(origin_ctx *ctx, const origin_glr_plan *pl,
                                          const GlrSpectralIO &io, const GlrRange &rg, int prow0);
