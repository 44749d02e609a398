// Line estimation of step 8: estimation_line / GridAnalysis / method_PCA_wgt / LS_deconv_wgt /
// conv_wgt / peakdet (reference lib_origin.py:1482-1938) for many detections at once.
//
// A PROBLEM is one (detection, grid offset) pair: an (Nz, P, P) column of raw and var around
// (cy, cx) = (y0 + dy, x0 + dx).  Its float64 work matrix A is Nz x ld, ld = P^2 rounded up to 16
// (slack columns zero), the layout origin_pca_gram / origin_pca_eig take.  Per batch of problems:
//
//   gather<0>     A = ds - rowmean(ds), ds = data / sqrt(var)                    (:1575-1579)
//   leading       G = A^T A (origin_pca_gram), v = leading eigenvector (origin_pca_eig),
//                 u = A v / |A v|: svds(k=1) of :1580 up to the sign, which the projection drops
//   colsum<0>     t = A^T u                                                      (:1583)
//   ls            deconv[z] = varest[z] sum_p psf (ds - u t^T) / sqrt(var)       (:1584-1587, :1504-1508)
//   gather<1>     A = (data - psf deconv (|psf| > 0)) / sqrt(var), centred       (:1590-1597)
//   leading       second vector                                                  (:1598)
//   dct           u <- D0 (D0^T u)                                               (:1600-1603)
//   colsum<1>     t = ds^T u with the UNCENTRED ds (the reference's asymmetry)   (:1606)
//   ls            estimated_line, estimated_var                                  (:1607-1611)
//   select        peakdet, flux, mse per grid offset, the winner of a detection  (:1693-1790)
//
// ds is never stored: wherever the uncentred value is needed it is recomputed from the cubes.
// Every sum has a fixed order (per-lane sequences, xor butterflies, slabs in ascending order):
// no atomics, and nothing depends on which other problems share the batch.  All loops have
// bounds that do not depend on the data.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "pca_eig.h"

namespace {

constexpr int LN_MAXCAND = 128;  // grid offsets per detection: size_grid <= 5
constexpr int LN_SLAB = 32;      // channels per partial of the column reduction
constexpr int LN_MAXDCT = 1024;  // order_dct + 1

// what every kernel needs to recompute an element of a problem's window
struct Field {
  const float *raw, *var;
  const double *psf;  // [nf][Nz][P2]
  const double *wgt;  // [nf][Ny][Nx] or null
  int Nz, Ny, Nx, P, P2, ld, nf;
};

struct Elem {
  double d, v, psf;
  bool bad;
};

// data (0 outside the field), var (+inf outside: lib :1884-1888) and the effective PSF
// sum_n w_n[y, x] psf_n[z, p] (:1713-1717; w_n = 0 outside the field, :1895-1896) of window
// element p of channel z around (cy, cx).  bad: a non-finite raw value, a var that is NaN or <= 0.
__device__ __forceinline__ Elem load_elem(const Field &f, int cy, int cx, int z, int p) {
  const int py = p / f.P, px = p - py * f.P;
  const int y = cy - f.P / 2 + py, x = cx - f.P / 2 + px;
  const bool in = y >= 0 && y < f.Ny && x >= 0 && x < f.Nx;
  Elem e;
  e.d = 0.0;
  e.v = INFINITY;
  e.bad = false;
  if (in) {
    const long i = ((long)z * f.Ny + y) * f.Nx + x;
    e.d = (double)f.raw[i];
    e.v = (double)f.var[i];
    e.bad = !isfinite(e.d) || !(e.v > 0.0);
  }
  if (!f.wgt) {
    e.psf = f.psf[(long)z * f.P2 + p];
  } else {
    double s = 0.0;
    for (int n = 0; n < f.nf; ++n) {
      const double w = in ? f.wgt[((long)n * f.Ny + y) * f.Nx + x] : 0.0;
      s += w * f.psf[((long)n * f.Nz + z) * f.P2 + p];
    }
    e.psf = s;
  }
  return e;
}

// sum over the 64 lanes, the same value (bit for bit) in every lane
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

// MODE 0: A = ds - rowmean(ds).  MODE 1: A = cleaned data, centred (dec = first deconvolution).
// The mean is over the P2 window elements, those outside the field (zeros) included (:1579).
// A row that holds a bad element, or (MODE 0) whose sum psf^2 / var is not positive, is written
// as zeros and flags its problem.     grid (ceil(Nz/4), nprob), block (64, 4): one wave per row
template <int MODE>
__global__ __launch_bounds__(256) void gather_kernel(Field f, const int *__restrict__ cen,
                                                     const double *__restrict__ dec,
                                                     double *__restrict__ A,
                                                     double *__restrict__ mean_out,
                                                     int *__restrict__ flag) {
  const int q = blockIdx.y, z = blockIdx.x * 4 + threadIdx.y, lane = threadIdx.x;
  if (z >= f.Nz) return;
  const int cy = cen[2 * q], cx = cen[2 * q + 1];
  const long row = (long)q * f.Nz + z;
  const double dz = MODE ? dec[row] : 0.0;
  bool bad = MODE ? flag[q] != 0 : false;
  double s = 0.0, sp = 0.0;
  for (int p = lane; p < f.P2; p += 64) {
    const Elem e = load_elem(f, cy, cx, z, p);
    bad |= e.bad;
    const double conv = fabs(e.psf) > 0.0 ? e.psf * dz : 0.0;
    s += (MODE ? e.d - conv : e.d) / sqrt(e.v);
    sp += e.psf * e.psf / e.v;
  }
  bad = __ballot(bad) != 0ull;
  s = wave_sum(s);
  sp = wave_sum(sp);
  if (!MODE && !(sp > 0.0)) bad = true;
  const double mean = s / (double)f.P2;
  double *Ar = A + row * f.ld;
  for (int p = lane; p < f.ld; p += 64) {
    double val = 0.0;
    if (p < f.P2 && !bad) {
      const Elem e = load_elem(f, cy, cx, z, p);
      const double conv = fabs(e.psf) > 0.0 ? e.psf * dz : 0.0;
      val = (MODE ? e.d - conv : e.d) / sqrt(e.v) - mean;
    }
    Ar[p] = val;
  }
  if (lane == 0) {
    if (mean_out) mean_out[row] = bad ? 0.0 : mean;
    if (!MODE && bad) flag[q] = 1;
  }
}

// whole matrices (and row means) of flagged problems become zero     grid (64, nprob), block 256
__global__ __launch_bounds__(256) void zero_flagged_kernel(const int *__restrict__ flag, long per,
                                                           int Nz, double *__restrict__ A,
                                                           double *__restrict__ mean_out) {
  const int q = blockIdx.y;
  if (!flag[q]) return;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per; i += (long)gridDim.x * 256)
    A[(long)q * per + i] = 0.0;
  if (mean_out)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < Nz; i += (long)gridDim.x * 256)
      mean_out[(long)q * Nz + i] = 0.0;
}

// y[z] = sum_p A[z][p] v[p]     grid (ceil(Nz/4), nprob), block (64, 4)
__global__ __launch_bounds__(256) void av_kernel(const double *__restrict__ A,
                                                 const double *__restrict__ v, int Nz, int ld,
                                                 double *__restrict__ y) {
  const int q = blockIdx.y, z = blockIdx.x * 4 + threadIdx.y, lane = threadIdx.x;
  if (z >= Nz) return;
  const double *Ar = A + ((long)q * Nz + z) * ld, *vq = v + (long)q * ld;
  double s = 0.0;
  for (int p = lane; p < ld; p += 64) s += Ar[p] * vq[p];
  s = wave_sum(s);
  if (lane == 0) y[(long)q * Nz + z] = s;
}

// sum over the block in a fixed order; every thread gets the total     block 256
__device__ __forceinline__ double block_sum(double x, double *sh) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  const double tot = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return tot;
}

// u = y / |y|, u = 0 where |y| == 0 (or not finite)     grid nprob, block 256
__global__ __launch_bounds__(256) void unorm_kernel(int Nz, double *__restrict__ y) {
  __shared__ double sh[4];
  double *yq = y + (long)blockIdx.x * Nz;
  double s = 0.0;
  for (int z = threadIdx.x; z < Nz; z += 256) s += yq[z] * yq[z];
  const double nrm = sqrt(block_sum(s, sh));
  const bool ok = nrm > 0.0 && isfinite(nrm);
  for (int z = threadIdx.x; z < Nz; z += 256) yq[z] = ok ? yq[z] / nrm : 0.0;
}

// u <- D (D^T u), D = DCTMAT(Nz, K - 1) as [Nz][K] (lib :127-147, :1602-1603; not renormalised)
// grid nprob, block 256
__global__ __launch_bounds__(256) void dct_kernel(int Nz, int K, const double *__restrict__ D,
                                                  double *__restrict__ u) {
  __shared__ double c[LN_MAXDCT];
  double *uq = u + (long)blockIdx.x * Nz;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = w; k < K; k += 4) {
    double s = 0.0;
    for (int z = lane; z < Nz; z += 64) s += D[(long)z * K + k] * uq[z];
    s = wave_sum(s);
    if (lane == 0) c[k] = s;
  }
  __syncthreads();
  for (int z = threadIdx.x; z < Nz; z += 256) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += D[(long)z * K + k] * c[k];
    uq[z] = s;
  }
}

// tpart[slab][p] = sum_{z in slab} M[z][p] u[z]; SRC 0: M = A, SRC 1: M = the uncentred ds
// grid (nslab, nprob), block 256
template <int SRC>
__global__ __launch_bounds__(256) void colsum_kernel(Field f, const int *__restrict__ cen,
                                                     const int *__restrict__ flag,
                                                     const double *__restrict__ A,
                                                     const double *__restrict__ u, int nslab,
                                                     double *__restrict__ tpart) {
  const int q = blockIdx.y, sl = blockIdx.x;
  const int z0 = sl * LN_SLAB, z1 = min(f.Nz, z0 + LN_SLAB);
  const int cy = cen[2 * q], cx = cen[2 * q + 1];
  const bool dead = flag[q] != 0;
  const double *uq = u + (long)q * f.Nz;
  for (int p = threadIdx.x; p < f.ld; p += 256) {
    double acc = 0.0;
    if (!dead && (SRC == 0 || p < f.P2)) {
      for (int z = z0; z < z1; ++z) {
        double m;
        if (SRC == 0) {
          m = A[((long)q * f.Nz + z) * f.ld + p];
        } else {
          const Elem e = load_elem(f, cy, cx, z, p);
          m = e.d / sqrt(e.v);
        }
        acc += m * uq[z];
      }
    }
    tpart[((long)q * nslab + sl) * f.ld + p] = acc;
  }
}

// t[p] = sum_slab tpart[slab][p], slabs in ascending order     grid (ceil(ld/256), nprob)
__global__ __launch_bounds__(256) void colreduce_kernel(const double *__restrict__ tpart, int nslab,
                                                        int ld, double *__restrict__ t) {
  const int q = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ld) return;
  double acc = 0.0;
  for (int s = 0; s < nslab; ++s) acc += tpart[((long)q * nslab + s) * ld + p];
  t[(long)q * ld + p] = acc;
}

// LS_deconv_wgt on residual = ds - u t^T (lib :1504-1508):
//   varest[z] = 1 / sum_p psf^2 / var,  dec[z] = varest[z] sum_p psf residual / sqrt(var)
// grid (ceil(Nz/4), nprob), block (64, 4)
__global__ __launch_bounds__(256) void ls_kernel(Field f, const int *__restrict__ cen,
                                                 const int *__restrict__ flag,
                                                 const double *__restrict__ u,
                                                 const double *__restrict__ t,
                                                 double *__restrict__ dec,
                                                 double *__restrict__ varest) {
  const int q = blockIdx.y, z = blockIdx.x * 4 + threadIdx.y, lane = threadIdx.x;
  if (z >= f.Nz) return;
  const long row = (long)q * f.Nz + z;
  if (flag[q]) {
    if (lane == 0) dec[row] = 0.0, varest[row] = 0.0;
    return;
  }
  const int cy = cen[2 * q], cx = cen[2 * q + 1];
  const double uz = u[row];
  const double *tq = t + (long)q * f.ld;
  double s1 = 0.0, s2 = 0.0;
  for (int p = lane; p < f.P2; p += 64) {
    const Elem e = load_elem(f, cy, cx, z, p);
    const double sd = sqrt(e.v);
    const double res = e.d / sd - uz * tq[p];
    s1 += e.psf * e.psf / e.v;
    s2 += e.psf * res / sd;
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) {
    const double ve = 1.0 / s1;
    varest[row] = ve;
    dec[row] = s2 * ve;
  }
}

// v[start:stop] of a length-n array as Python slices it (a negative bound counts from the end)
__device__ __forceinline__ void py_slice(long start, long stop, int n, int &a, int &b) {
  if (start < 0) start = start + n < 0 ? 0 : start + n;
  if (stop < 0) stop = stop + n < 0 ? 0 : stop + n;
  if (start > n) start = n;
  if (stop > n) stop = n;
  a = (int)start;
  b = (int)(stop > start ? stop : start);
}

// sum((r1 - LC)^2) / sum(r1^2) over channels [a, b) and the central (2 hp + 1)^2 of the window,
// LC = conv_wgt(dec, psf) (lib :1736-1746, :1529-1531); 0/0 = NaN for an empty range, as NumPy
__device__ double mse_of(const Field &f, int cy, int cx, const double *v, int a, int b, int hp) {
  double num = 0.0, den = 0.0;
  const int c = f.P / 2;
  for (int z = a; z < b; ++z)
    for (int iy = c - hp; iy <= c + hp; ++iy)
      for (int ix = c - hp; ix <= c + hp; ++ix) {
        const Elem e = load_elem(f, cy, cx, z, iy * f.P + ix);
        const double lc = fabs(e.psf) > 0.0 ? e.psf * v[z] : 0.0;
        num += (e.d - lc) * (e.d - lc);
        den += e.d * e.d;
      }
  return num / den;
}

// GridAnalysis after method_PCA_wgt (lib :1693-1790), one block per detection, one thread per grid
// offset.  det: (z0, y0, x0, first problem, problems) per detection; the problems of a detection
// are its valid grid offsets in np.where order (dy major).  (The `z_est == 0: break` of :1723
// cannot be taken: peakdet returns an interior index or size // 2, and the window holds at least
// two channels for Nz >= 2.)  The first best offset wins a tie.  Fallback row (:1760-1769) when
// every offset is flagged or the criterion of an offset is NaN / of the winner not finite.
// grid ndet, block 64
__global__ __launch_bounds__(64) void select_kernel(Field f, const int *__restrict__ det,
                                                    const int *__restrict__ cen,
                                                    const int *__restrict__ flag,
                                                    const double *__restrict__ dec,
                                                    const double *__restrict__ varest,
                                                    int use_mse, int hp, int horiz,
                                                    double *__restrict__ o_line,
                                                    double *__restrict__ o_var,
                                                    double *__restrict__ o_flux,
                                                    double *__restrict__ o_mse,
                                                    int *__restrict__ o_yxz,
                                                    int *__restrict__ o_status) {
  __shared__ double crit[LN_MAXCAND], f05[LN_MAXCAND], m5[LN_MAXCAND];
  __shared__ int zest[LN_MAXCAND], ok[LN_MAXCAND], win;
  const int d = blockIdx.x, Nz = f.Nz;
  const int z0 = det[5 * d], y0 = det[5 * d + 1], x0 = det[5 * d + 2];
  const int first = det[5 * d + 3], nc = det[5 * d + 4];
  for (int c = threadIdx.x; c < nc; c += 64) {
    const int q = first + c;
    ok[c] = !flag[q];
    crit[c] = f05[c] = m5[c] = 0.0;
    zest[c] = 0;
    if (!ok[c]) continue;
    const double *v = dec + (long)q * Nz;
    const int cy = cen[2 * q], cx = cen[2 * q + 1];
    // peakdet(v[ind_max]) (:1793-1801): the strict local maximum closest to the middle
    const int lo = max(0, z0 - 5), hi = min(Nz, z0 + 6), L = hi - lo;
    int zi = L / 2;
    long bestd = -1;
    for (int i = 1; i + 1 < L; ++i)
      if (v[lo + i] > v[lo + i - 1] && v[lo + i] > v[lo + i + 1]) {
        const long dd = (long)(i - L / 2) * (i - L / 2);
        if (bestd < 0 || dd < bestd) bestd = dd, zi = i;
      }
    const int maxz = z0 - 5 + zi;  // (:1726, also where z0 < 5)
    zest[c] = maxz;
    int a, b;
    py_slice((long)maxz - horiz, (long)maxz + horiz + 1, Nz, a, b);  // ind_hrz (:1734)
    const int a5 = max(0, maxz - 5), b5 = max(a5, min(maxz + 6, Nz));  // ind_z5 (:1742)
    double s = 0.0;
    for (int z = a5; z < b5; ++z) s += v[z];
    f05[c] = s;
    m5[c] = mse_of(f, cy, cx, v, a5, b5, hp);
    if (use_mse) {
      crit[c] = mse_of(f, cy, cx, v, a, b, hp);
    } else {
      s = 0.0;
      for (int z = a; z < b; ++z) s += v[z];
      crit[c] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int best = -1;
    bool nan = false;
    for (int c = 0; c < nc; ++c) {
      if (!ok[c]) continue;
      if (crit[c] != crit[c]) nan = true;
      if (best < 0 || (use_mse ? crit[c] < crit[best] : crit[c] > crit[best])) best = c;
    }
    if (best >= 0 && (nan || !isfinite(crit[best]))) best = -1;
    win = best;
    o_flux[d] = best < 0 ? 0.0 : f05[best];
    o_mse[d] = best < 0 ? 1.0e6 : m5[best];
    o_yxz[3 * d] = best < 0 ? y0 : cen[2 * (first + best)];
    o_yxz[3 * d + 1] = best < 0 ? x0 : cen[2 * (first + best) + 1];
    o_yxz[3 * d + 2] = best < 0 ? z0 : zest[best];
    o_status[d] = best < 0 ? 1 : 0;
  }
  __syncthreads();
  const int best = win;
  for (int z = threadIdx.x; z < Nz; z += 64) {
    o_line[(long)d * Nz + z] = best < 0 ? 0.0 : dec[(long)(first + best) * Nz + z];
    o_var[(long)d * Nz + z] = best < 0 ? 0.0 : varest[(long)(first + best) * Nz + z];
  }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct Problems {
  std::vector<int> cen;  // (cy, cx) per problem
  std::vector<int> det;  // (z0, y0, x0, first problem, problems) per detection
};

// the valid grid offsets of every detection in np.where order (lib :1703-1706)
void list_problems(const int *h_det, int ndet, int size_grid, int Ny, int Nx, Problems &pr) {
  for (int d = 0; d < ndet; ++d) {
    const int z0 = h_det[3 * d], y0 = h_det[3 * d + 1], x0 = h_det[3 * d + 2];
    const int first = (int)(pr.cen.size() / 2);
    for (int dy = -size_grid; dy <= size_grid; ++dy)
      for (int dx = -size_grid; dx <= size_grid; ++dx) {
        const int y = y0 + dy, x = x0 + dx;
        if (y < 0 || y >= Ny || x < 0 || x >= Nx) continue;
        pr.cen.push_back(y);
        pr.cen.push_back(x);
      }
    const int n = (int)(pr.cen.size() / 2) - first;
    const int row[5] = {z0, y0, x0, first, n};
    pr.det.insert(pr.det.end(), row, row + 5);
  }
}

int check_shapes(const void *d_raw, int Nz, int Ny, int Nx, int nf, int P, const double *h_psf) {
  ORIGIN_CHECK_ARG(d_raw && h_psf, "null cube or PSF");
  ORIGIN_CHECK_ARG(Nz >= 2 && Ny > 0 && Nx > 0 && nf >= 1, "bad cube shape or field count");
  ORIGIN_CHECK_ARG(P >= 1 && P <= 41 && (P & 1), "PSF size must be odd and at most 41");
  return ORIGIN_OK;
}

int check_dets(const int *h_det, int ndet, int Nz, int Ny, int Nx, int size_grid, int hp, int horiz,
               int P) {
  ORIGIN_CHECK_ARG(h_det && ndet > 0, "no detections");
  ORIGIN_CHECK_ARG(size_grid >= 0 && (2 * size_grid + 1) * (2 * size_grid + 1) <= LN_MAXCAND,
                   "size_grid must be in 0..5");
  ORIGIN_CHECK_ARG(hp >= 0 && hp <= P / 2 && horiz >= 0, "bad horiz_psf / horiz");
  for (int d = 0; d < ndet; ++d)
    ORIGIN_CHECK_ARG(h_det[3 * d] >= 0 && h_det[3 * d] < Nz && h_det[3 * d + 1] >= 0 &&
                         h_det[3 * d + 1] < Ny && h_det[3 * d + 2] >= 0 && h_det[3 * d + 2] < Nx,
                     "detection %d lies outside the cube", d);
  return ORIGIN_OK;
}

// device copies of the PSFs and the weight maps
struct Tables {
  DevMem psf, wgt;
  explicit Tables(origin_ctx *c) : psf(c), wgt(c) {}
  int upload(origin_ctx *ctx, Field &f, const double *h_psf, const double *h_wgt) {
    const size_t pb = (size_t)f.nf * f.Nz * f.P2 * sizeof(double);
    int rc = psf.alloc(pb);
    if (rc) return rc;
    if ((rc = origin_h2d(ctx, psf.p, h_psf, pb))) return rc;
    f.psf = (const double *)psf.p;
    f.wgt = nullptr;
    if (h_wgt) {
      const size_t wb = (size_t)f.nf * f.Ny * f.Nx * sizeof(double);
      if ((rc = wgt.alloc(wb))) return rc;
      if ((rc = origin_h2d(ctx, wgt.p, h_wgt, wb))) return rc;
      f.wgt = (const double *)wgt.p;
    }
    return ORIGIN_OK;
  }
};

Field make_field(const float *d_raw, const float *d_var, int Nz, int Ny, int Nx, int nf, int P) {
  Field f;
  f.raw = d_raw, f.var = d_var, f.psf = nullptr, f.wgt = nullptr;
  f.Nz = Nz, f.Ny = Ny, f.Nx = Nx, f.P = P, f.P2 = P * P, f.ld = (P * P + 15) / 16 * 16, f.nf = nf;
  return f;
}

// pieces of the batch workspace; sized for `nb` problems and `nd` detections
struct Work {
  double *A, *mean, *G, *v, *u, *tpart, *t, *dec, *varest, *o_line, *o_var, *o_flux, *o_mse;
  long *xp_off, *g_off, *ld, *n, *q_off, *v_off, *gx_off, *gg_off;
  int *ti, *tj, *ta, *cen, *det, *flag, *o_yxz, *o_status;
  int nslab, gmax, tpp;
  void layout(Carver &c, const Field &f, long nb, long nd) {
    const long Nz = f.Nz, ld = f.ld;
    A = c.take<double>(nb * Nz * ld), mean = c.take<double>(nb * Nz);
    G = c.take<double>(nb * ld * ld), v = c.take<double>(nb * ld), u = c.take<double>(nb * Nz);
    tpart = c.take<double>(nb * nslab * ld), t = c.take<double>(nb * ld);
    dec = c.take<double>(nb * Nz), varest = c.take<double>(nb * Nz);
    o_line = c.take<double>(nd * Nz), o_var = c.take<double>(nd * Nz);
    o_flux = c.take<double>(nd), o_mse = c.take<double>(nd);
    xp_off = c.take<long>(nb), g_off = c.take<long>(nb), this->ld = c.take<long>(nb);
    n = c.take<long>(nb), q_off = c.take<long>(nb), v_off = c.take<long>(nb);
    gx_off = c.take<long>(gmax), gg_off = c.take<long>(gmax);
    ti = c.take<int>((long)gmax * tpp), tj = c.take<int>((long)gmax * tpp);
    ta = c.take<int>((long)gmax * tpp);
    cen = c.take<int>(2 * nb), det = c.take<int>(5 * nd), flag = c.take<int>(nb);
    o_yxz = c.take<int>(3 * nd), o_status = c.take<int>(nd);
  }
};

// Gram product, leading eigenvector and u = A v / |A v| of the nb matrices in W.A.  The Gram
// launches cover groups of at most W.gmax problems: every group size up to gmax gives gram_launch
// the K-split of a single problem, so a matrix is summed the same way whatever shares its batch.
int leading_vectors(origin_ctx *ctx, const Field &f, Work &W, int nb) {
  const long Nz = f.Nz, ld = f.ld;
  for (int s = 0; s < nb; s += W.gmax) {
    const int k = std::min(W.gmax, nb - s);
    int rc = origin_pca_gram(ctx, W.A + s * Nz * ld, W.gx_off, W.ld, f.Nz, k * W.tpp, W.ti, W.tj,
                             W.ta, (long)k * ld * ld, W.G + s * ld * ld, W.gg_off);
    if (rc) return rc;
  }
  int rc = origin_pca_eig(ctx, W.G, W.g_off, W.ld, W.n, nb, (long)nb * origin_pca_eig_qrows() * ld,
                          W.q_off, W.v, W.v_off, nullptr);
  if (rc) return rc;
  ProfScope ps(ctx, K_LINES_UVEC);
  hipLaunchKernelGGL(av_kernel, dim3(cdiv(Nz, 4), nb), dim3(64, 4), 0, ctx->stream, W.A, W.v, f.Nz,
                     f.ld, W.u);
  hipLaunchKernelGGL(unorm_kernel, dim3(nb), dim3(256), 0, ctx->stream, f.Nz, W.u);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// t = M^T u (SRC as colsum_kernel), then the least-squares pass into W.dec / W.varest
template <int SRC>
int project_and_deconvolve(origin_ctx *ctx, const Field &f, Work &W, int nb) {
  {
    ProfScope ps(ctx, K_LINES_PROJECT);
    hipLaunchKernelGGL(colsum_kernel<SRC>, dim3(W.nslab, nb), dim3(256), 0, ctx->stream, f, W.cen,
                       W.flag, W.A, W.u, W.nslab, W.tpart);
    hipLaunchKernelGGL(colreduce_kernel, dim3(cdiv(f.ld, 256), nb), dim3(256), 0, ctx->stream,
                       W.tpart, W.nslab, f.ld, W.t);
  }
  ProfScope ps(ctx, K_LINES_LS);
  hipLaunchKernelGGL(ls_kernel, dim3(cdiv(f.Nz, 4), nb), dim3(64, 4), 0, ctx->stream, f, W.cen,
                     W.flag, W.u, W.t, W.dec, W.varest);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

int run_gather(origin_ctx *ctx, const Field &f, int nb, const int *cen, double *A, double *mean,
               int *flag) {
  ProfScope ps(ctx, K_LINES_GATHER);
  ORIGIN_HIP(hipMemsetAsync(flag, 0, (size_t)nb * sizeof(int), ctx->stream));
  hipLaunchKernelGGL(gather_kernel<0>, dim3(cdiv(f.Nz, 4), nb), dim3(64, 4), 0, ctx->stream, f, cen,
                     (const double *)nullptr, A, mean, flag);
  hipLaunchKernelGGL(zero_flagged_kernel, dim3(64, nb), dim3(256), 0, ctx->stream, flag,
                     (long)f.Nz * f.ld, f.Nz, A, mean);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// what the batches of a call share: how a detection's winner is picked, the DCT denoising of u
// (DCTMAT(Nz, K - 1) on the device, K == 0: none) and the caller's arrays, one row per detection
struct Call {
  int criteria, horiz_psf, horiz, K;
  const double *dct;
  double *line, *var, *flux, *mse;
  int *yxz, *status;
};

int run_select(origin_ctx *ctx, const Field &f, Work &W, int nd, const Call &c) {
  ProfScope ps(ctx, K_LINES_SELECT);
  hipLaunchKernelGGL(select_kernel, dim3(nd), dim3(64), 0, ctx->stream, f, W.det, W.cen, W.flag,
                     W.dec, W.varest, c.criteria, c.horiz_psf, c.horiz, W.o_line, W.o_var, W.o_flux,
                     W.o_mse, W.o_yxz, W.o_status);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// results of nd detections, starting at detection d0 of the caller's arrays
int fetch_results(origin_ctx *ctx, const Field &f, Work &W, int d0, int nd, const Call &h) {
  const size_t lb = (size_t)nd * f.Nz * sizeof(double);
  int rc;
  if ((rc = origin_d2h(ctx, h.line + (size_t)d0 * f.Nz, W.o_line, lb))) return rc;
  if ((rc = origin_d2h(ctx, h.var + (size_t)d0 * f.Nz, W.o_var, lb))) return rc;
  if ((rc = origin_d2h(ctx, h.flux + d0, W.o_flux, nd * sizeof(double)))) return rc;
  if ((rc = origin_d2h(ctx, h.mse + d0, W.o_mse, nd * sizeof(double)))) return rc;
  if ((rc = origin_d2h(ctx, h.yxz + 3 * (size_t)d0, W.o_yxz, 3 * nd * sizeof(int)))) return rc;
  return origin_d2h(ctx, h.status + d0, W.o_status, nd * sizeof(int));
}

// DCTMAT(Nz, K - 1) (lib :127-147) as [Nz][K] on the device, built once per call; K == 0: none
int upload_dct(origin_ctx *ctx, int Nz, int K, DevMem &dct) {
  if (K <= 0) return ORIGIN_OK;
  std::vector<double> D((size_t)Nz * K);
  for (int z = 0; z < Nz; ++z)
    for (int k = 0; k < K; ++k) {
      const double c = std::sqrt(2.0 / Nz) * std::cos((z + 0.5) * (M_PI / Nz) * k);
      D[(size_t)z * K + k] = k == 0 ? c * (1.0 / std::sqrt(2.0)) : c;
    }
  const int rc = dct.alloc(D.size() * sizeof(double));
  return rc ? rc : origin_h2d(ctx, dct.p, D.data(), D.size() * sizeof(double));
}

// the largest Gram group that keeps ks1, a single problem's K-split, within 256 MiB of slabs
int gram_group(int num_cu, int tpp, int Nz, long ld, int ks1) {
  int g = 1;
  while (g < 1024 && pca_gram_ksplit(num_cu, (long)(g + 1) * tpp, Nz) == ks1 &&
         (size_t)ks1 * (g + 1) * ld * ld * sizeof(double) <= ((size_t)256 << 20))
    ++g;
  return g;
}

// problems per batch (whole detections): from the free memory unless the caller says
long batch_capacity(size_t free_b, const Field &f, Work &W, int ks1, int size_grid, int max_prob) {
  const int ncand_max = (2 * size_grid + 1) * (2 * size_grid + 1);
  Carver one;  // (sizes only: a null base)
  W.layout(one, f, 1, 1);
  const size_t per_problem = one.off + (size_t)origin_pca_eig_qrows() * f.ld * 8 +
                             (size_t)ks1 * f.ld * f.ld * 8;
  long cap = (long)(free_b / 2 / per_problem);
  cap = std::max((long)ncand_max, std::min(cap, 8192l));
  if (max_prob > 0) cap = std::max((long)ncand_max, std::min(cap, (long)max_prob));
  return cap;
}

// descriptors of origin_pca_gram (one group, reused by every group) and origin_pca_eig
int upload_descriptors(origin_ctx *ctx, const Field &f, Work &W, long cap) {
  const long Nz = f.Nz, ld = f.ld;
  const int nt = (int)((ld + 31) / 32);
  std::vector<long> xo(cap), go(cap), lds(cap, ld), ns(cap, f.P2), qo(cap), vo(cap);
  for (long i = 0; i < cap; ++i) {
    xo[i] = i * Nz * ld, go[i] = i * ld * ld, vo[i] = i * ld;
    qo[i] = i * origin_pca_eig_qrows() * ld;
  }
  std::vector<int> ti, tj, ta;
  for (int a = 0; a < W.gmax; ++a)
    for (int i = 0; i < nt; ++i)
      for (int j = i; j < nt; ++j) ti.push_back(i), tj.push_back(j), ta.push_back(a);
  int rc;
  if ((rc = put(ctx, W.xp_off, xo)) || (rc = put(ctx, W.g_off, go)) || (rc = put(ctx, W.ld, lds)) ||
      (rc = put(ctx, W.n, ns)) || (rc = put(ctx, W.q_off, qo)) || (rc = put(ctx, W.v_off, vo)) ||
      (rc = put(ctx, W.ti, ti)) || (rc = put(ctx, W.tj, tj)) || (rc = put(ctx, W.ta, ta)))
    return rc;
  xo.resize(W.gmax), go.resize(W.gmax);
  if ((rc = put(ctx, W.gx_off, xo))) return rc;
  return put(ctx, W.gg_off, go);
}

// detections [d0, d1) of the call, nb problems: the header's steps on one batch
int estimate_batch(origin_ctx *ctx, const Field &f, Work &W, const Problems &pr, int d0, int d1,
                   int nb, const Call &c) {
  const int nd = d1 - d0, p0 = pr.det[5 * d0 + 3];
  std::vector<int> det(pr.det.begin() + 5 * d0, pr.det.begin() + 5 * d1);
  for (int d = 0; d < nd; ++d) det[5 * d + 3] -= p0;
  int rc;
  if ((rc = origin_h2d(ctx, W.cen, pr.cen.data() + 2 * (size_t)p0, 2 * (size_t)nb * sizeof(int))))
    return rc;
  if ((rc = put(ctx, W.det, det))) return rc;
  if ((rc = run_gather(ctx, f, nb, W.cen, W.A, W.mean, W.flag))) return rc;
  if ((rc = leading_vectors(ctx, f, W, nb))) return rc;
  if ((rc = project_and_deconvolve<0>(ctx, f, W, nb))) return rc;
  {
    ProfScope ps(ctx, K_LINES_GATHER);
    hipLaunchKernelGGL(gather_kernel<1>, dim3(cdiv(f.Nz, 4), nb), dim3(64, 4), 0, ctx->stream, f,
                       W.cen, W.dec, W.A, (double *)nullptr, W.flag);
    ORIGIN_LAUNCH_CHECK();
  }
  if ((rc = leading_vectors(ctx, f, W, nb))) return rc;
  if (c.K > 0) {
    ProfScope ps(ctx, K_LINES_UVEC);
    hipLaunchKernelGGL(dct_kernel, dim3(nb), dim3(256), 0, ctx->stream, f.Nz, c.K, c.dct, W.u);
    ORIGIN_LAUNCH_CHECK();
  }
  if ((rc = project_and_deconvolve<1>(ctx, f, W, nb))) return rc;
  if ((rc = run_select(ctx, f, W, nd, c))) return rc;
  return fetch_results(ctx, f, W, d0, nd, c);
}

}  // namespace

extern "C" {

int origin_lines_gather(origin_ctx *ctx, const float *d_raw, const float *d_var, int Nz, int Ny,
                        int Nx, int nfields, int P, const double *h_psf, const double *h_weights,
                        int nprob, const int *h_centres, double *d_A, double *d_mean, int *d_flag) {
  ORIGIN_USE(ctx);
  int rc = check_shapes(d_raw, Nz, Ny, Nx, nfields, P, h_psf);
  if (rc) return rc;
  ORIGIN_CHECK_ARG(d_var && nprob > 0 && h_centres && d_A && d_mean && d_flag, "bad arguments");
  Field f = make_field(d_raw, d_var, Nz, Ny, Nx, nfields, P);
  Tables tab(ctx);
  if ((rc = tab.upload(ctx, f, h_psf, h_weights))) return rc;
  DevMem cen(ctx);
  if ((rc = cen.alloc((size_t)2 * nprob * sizeof(int)))) return rc;
  if ((rc = origin_h2d(ctx, cen.p, h_centres, (size_t)2 * nprob * sizeof(int)))) return rc;
  if ((rc = run_gather(ctx, f, nprob, (const int *)cen.p, d_A, d_mean, d_flag))) return rc;
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

int origin_lines_select(origin_ctx *ctx, const float *d_raw, int Nz, int Ny, int Nx, int nfields,
                        int P, const double *h_psf, const double *h_weights, int ndet,
                        const int *h_det, int size_grid, int criteria, int horiz_psf, int horiz,
                        const double *h_deconv, const double *h_varest, const int *h_flag,
                        double *h_line, double *h_var, double *h_flux5, double *h_mse5, int *h_yxz,
                        int *h_status) {
  ORIGIN_USE(ctx);
  int rc = check_shapes(d_raw, Nz, Ny, Nx, nfields, P, h_psf);
  if (rc) return rc;
  if ((rc = check_dets(h_det, ndet, Nz, Ny, Nx, size_grid, horiz_psf, horiz, P))) return rc;
  ORIGIN_CHECK_ARG((criteria == 0 || criteria == 1) && h_deconv && h_varest && h_flag && h_line &&
                       h_var && h_flux5 && h_mse5 && h_yxz && h_status,
                   "bad arguments");
  Field f = make_field(d_raw, d_raw, Nz, Ny, Nx, nfields, P);  // (var is not read by the selection)
  Tables tab(ctx);
  if ((rc = tab.upload(ctx, f, h_psf, h_weights))) return rc;
  Problems pr;
  list_problems(h_det, ndet, size_grid, Ny, Nx, pr);
  const int nb = (int)(pr.cen.size() / 2);
  Work W = {};
  DevMem mem(ctx);
  rc = carve_block(ctx, mem, [&](Carver &c) {  // only the pieces the selection touches
    W.dec = c.take<double>((long)nb * Nz), W.varest = c.take<double>((long)nb * Nz);
    W.o_line = c.take<double>((long)ndet * Nz), W.o_var = c.take<double>((long)ndet * Nz);
    W.o_flux = c.take<double>(ndet), W.o_mse = c.take<double>(ndet);
    W.cen = c.take<int>(2 * nb), W.det = c.take<int>(5 * ndet), W.flag = c.take<int>(nb);
    W.o_yxz = c.take<int>(3 * ndet), W.o_status = c.take<int>(ndet);
  });
  if (rc) return rc;
  const size_t db = (size_t)nb * Nz * sizeof(double);
  if ((rc = origin_h2d(ctx, W.dec, h_deconv, db))) return rc;
  if ((rc = origin_h2d(ctx, W.varest, h_varest, db))) return rc;
  if ((rc = origin_h2d(ctx, W.flag, h_flag, (size_t)nb * sizeof(int)))) return rc;
  if ((rc = put(ctx, W.cen, pr.cen)) || (rc = put(ctx, W.det, pr.det))) return rc;
  const Call call = {criteria, horiz_psf, horiz, 0, nullptr,  // (no DCT in the selection)
                     h_line, h_var, h_flux5, h_mse5, h_yxz, h_status};
  if ((rc = run_select(ctx, f, W, ndet, call))) return rc;
  return fetch_results(ctx, f, W, 0, ndet, call);
}

int origin_lines_estimate(origin_ctx *ctx, const float *d_raw, const float *d_var, int Nz, int Ny,
                          int Nx, int nfields, int P, const double *h_psf, const double *h_weights,
                          int ndet, const int *h_det, int size_grid, int criteria, int order_dct,
                          int horiz_psf, int horiz, int max_problems, double *h_line, double *h_var,
                          double *h_flux5, double *h_mse5, int *h_yxz, int *h_status,
                          int *h_nbatch) {
  ORIGIN_USE(ctx);
  int rc = check_shapes(d_raw, Nz, Ny, Nx, nfields, P, h_psf);
  if (rc) return rc;
  if ((rc = check_dets(h_det, ndet, Nz, Ny, Nx, size_grid, horiz_psf, horiz, P))) return rc;
  ORIGIN_CHECK_ARG(d_var && (criteria == 0 || criteria == 1) && h_line && h_var && h_flux5 &&
                       h_mse5 && h_yxz && h_status && max_problems >= 0,
                   "bad arguments");
  ORIGIN_CHECK_ARG(order_dct >= -1 && order_dct < LN_MAXDCT, "order_dct must be below %d",
                   LN_MAXDCT);
  ORIGIN_CHECK_ARG(!h_weights || size_grid == 0, "weighted fields need size_grid == 0");
  Field f = make_field(d_raw, d_var, Nz, Ny, Nx, nfields, P);
  Tables tab(ctx);
  if ((rc = tab.upload(ctx, f, h_psf, h_weights))) return rc;
  DevMem dct(ctx);
  if ((rc = upload_dct(ctx, Nz, order_dct + 1, dct))) return rc;
  Problems pr;
  list_problems(h_det, ndet, size_grid, Ny, Nx, pr);
  const int nt = (f.ld + 31) / 32;
  Work W = {};
  W.nslab = cdiv(Nz, LN_SLAB);
  W.tpp = nt * (nt + 1) / 2;
  const int ks1 = pca_gram_ksplit(ctx->num_cu, W.tpp, Nz);
  W.gmax = gram_group(ctx->num_cu, W.tpp, Nz, f.ld, ks1);
  size_t free_b = 0, total_b = 0;
  if ((rc = origin_mem_info(ctx, &free_b, &total_b))) return rc;
  const long cap = batch_capacity(free_b, f, W, ks1, size_grid, max_problems);
  W.gmax = (int)std::min((long)W.gmax, cap);
  DevMem mem(ctx);
  const long nd_cap = std::min((long)ndet, cap);
  if ((rc = carve_block(ctx, mem, [&](Carver &c) { W.layout(c, f, cap, nd_cap); }))) return rc;
  if ((rc = upload_descriptors(ctx, f, W, cap))) return rc;

  const Call call = {criteria, horiz_psf, horiz, order_dct + 1, (const double *)dct.p,
                     h_line, h_var, h_flux5, h_mse5, h_yxz, h_status};
  int nbatch = 0;
  for (int d0 = 0; d0 < ndet; ++nbatch) {
    int d1 = d0;
    long nb = 0;
    while (d1 < ndet && nb + pr.det[5 * d1 + 4] <= cap) nb += pr.det[5 * d1 + 4], ++d1;
    if ((rc = estimate_batch(ctx, f, W, pr, d0, d1, (int)nb, call))) return rc;
    d0 = d1;
  }
  if (h_nbatch) *h_nbatch = nbatch;
  return ORIGIN_OK;
}

}  // extern "C"
