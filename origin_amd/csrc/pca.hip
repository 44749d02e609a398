// Greedy PCA  (SURVEY.md 2.2 rows k5-k7): the whole loop of Compute_GreedyPCA
// (reference muse_origin/lib_origin.py:848-954) for all areas of a cube that stays in
// place in HBM as (Nz, S), S = Ny*Nx.
//
// Per iteration and per area (lib :899-949):
//   nuisance set   pypx = {test > thr}; mapO2[pypx] += 1; itermax guard        (:889,:901-905)
//   background     the nb = 1 + int(n_bg / Noise_population) lowest-O2 spectra  (:908-917)
//   b   = mean of the background spectra                                       (:917)
//   Xp  = X_nuis - b (b^T X_nuis)            [un-normalised projection]        (:920-923)
//   u   = leading left singular vector of Xp (ARPACK svds(k=1, tol=0))         (:940)
//   F  -= u (u^T F) over the whole area; test = mean_z F^2                     (:943-946)
//
// Coefficient form.  The cube is NOT rewritten every iteration.  With X the input (cube_std)
// the deflated cube after t iterations is  F_t = X - sum_{k<t} u_k c_k^T,  c_k = F_{k-1}^T u_k,
// so the library keeps the vectors U (per area) and the coefficient rows C (per spaxel) and
// evaluates columns of F_t on the fly where an iteration needs them (background mean, nuisance
// block).  One iteration then reads the area once (c_t = X^T u_t - C^T (U^T u_t)) instead of
// reading it twice and writing it once, and the O2 test follows from Pythagoras:
// |F_t|^2 = |F_{t-1}|^2 - c_t^2 exactly (u_t has unit norm).  The cube itself is produced by
// one final pass F = X - U C (single float32 rounding instead of one per iteration).
//
// All areas advance in lock step (they are independent, lib :806-819), every kernel is
// batched over the areas still iterating, and the control flow (which spaxels are
// nuisances, which background spectra feed the mean, when an area stops) runs on the device:
// per iteration the host reads back two ints per area to size the launches.
//
// u comes from the Gram matrix G = Xp^T Xp (float64 MFMA, the only matrix-shaped
// contraction of the path): its leading eigenvector v, converged until the residual is at
// rounding level, gives u = Xp v / |Xp v|.  pca_eig.hip picks the solver by the size of the
// iteration's largest matrix: up to 96 columns repeated squaring on the matrix cores
// (eig_power_kernel), up to 512 plain Lanczos with the matrix resident on the CU
// (lanczos_plain_kernel), above that restarted Lanczos with full re-orthogonalisation
// (lanczos_kernel).  SURVEY.md section 7 (hard part 1): the loop is threshold driven, so the
// eigen-solve must be converged; everything that feeds it is float64, only the cube is f32.
//
// A block never straddles two areas, so per-area vectors (b, u) are wave-uniform.
//
// The driver (origin_pca_run_into, at the end of the file) is a loop over the members of PcaRun:
//   select()               the selection kernel, its hand-shake, the counts n / nb per area
//   maybe_fire_tail_hook() few stragglers left: write the finished areas, tell the caller
//   build_work_list()      descriptors, Gram tiles and slot table of the areas with n >= 2, uploaded
//   enqueue_chain()        cbar_kernel ... deflate_finish_kernel; the eigen-solvers are in pca_eig.hip
//   flush()                F = X - U C: when an area is out of vector slots, and at the end
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <vector>

#include "common.h"
#include "pca_eig.h"

namespace {

// descriptor fields of the per-iteration work list (int64 [DF_COUNT][nw])
enum {
  DF_AREA = 0, DF_LIST0, DF_N, DF_NB, DF_LD, DF_XP, DF_C, DF_G, DF_Q, DF_NS, DF_CBASE,
  DF_T,    // vectors already removed from this area (rows of C / columns of U in use)
  DF_CN,   // offset of the gathered coefficient block Cn[T][ld] of this area
  DF_FBOLD,  // offset of this area's nuisance block of the previous iteration (-1: none)
  DF_LDOLD,  // its row stride
  DF_NOLD,   // its number of columns
  DF_SVALID,  // 1: the running column sum of the area's background set is usable (bmean_kernel)
  DF_COUNT
};
constexpr int PCA_CAP = 64;  // vectors kept per area before the cube is flushed (F = X - U C)
#define DSC(f, k) (D[(long)(f) * nw + (k)])

// ------------------------------------------------------------------------------------
// selection: nuisance list, background list, iteration bookkeeping.  One block per area.
// ------------------------------------------------------------------------------------
struct BlockScan {
  int *wtot;  // LDS [16]
  __device__ __forceinline__ int exclusive(bool f, int &total) {
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rank = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // previous users of wtot are done
    if (lane == 0) wtot[wave] = __popcll(b);
    __syncthreads();
    int pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      const int c = wtot[w];
      pre += (w < wave) ? c : 0;
      tot += c;
    }
    total = tot;
    return pre + rank;
  }
};

// What a selection launch works on: the area lists, the O2 values and thresholds, the per-area
// state, the lists it writes and where the counts go.  One block per area.
struct SelectArgs {
  const int *spx;       // spaxel lists of the areas, area a at [spx_off[a], spx_off[a + 1])
  const long *spx_off;
  const double *test, *thr;
  double noise_pop;
  int itermax;
  int *active, *nbiter, *nstop, *mapO2;
  int *nuis, *bg, *nuis_pos, *bg_pos;  // nuisance / background spaxels and their list positions
  int *n_out, *nb_out;
  // changes of the background set against the previous iteration (bmean_kernel), kept by the
  // register-resident kernel only: membership flags, signed list of changes, their number per area
  uint8_t *inB;
  int *dlist, *ndiff;
  // select_publish: mapped host memory for the counts, the device counter of finished blocks and
  // the generation of this launch
  int *host_out;
  unsigned *counter;
  int gen;
};

// ---- the rules both selection kernels share (side effects by thread 0, in the reference's order)
// the area stops iterating
__device__ __forceinline__ void select_stop(const SelectArgs &s, int a) {
  if (threadIdx.x == 0) s.active[a] = 0, s.n_out[a] = 0, s.nb_out[a] = 0;
}

// entry: an area that has stopped reports zero counts; returns whether the area still iterates
__device__ __forceinline__ bool select_enter(const SelectArgs &s, int a) {
  if (s.active[a]) return true;
  if (threadIdx.x == 0) s.n_out[a] = 0, s.nb_out[a] = 0;
  return false;
}

// nbiter += 1; if nbiter > itermax: nstop += 1; break                            (lib :900-905)
// (mapO2[pypx] += 1 comes before it, lib :901.)  s_it: an int in LDS; returns whether the area stops.
__device__ __forceinline__ bool select_itermax_stop(const SelectArgs &s, int a, int *s_it) {
  if (threadIdx.x == 0) {
    const int it = s.nbiter[a] + 1;
    s.nbiter[a] = it;
    *s_it = it;
  }
  __syncthreads();
  if (*s_it <= s.itermax) return false;
  if (threadIdx.x == 0) atomicAdd(s.nstop, 1);
  select_stop(s, a);
  return true;
}

// nb = 1 + int(len(nind) / Noise_population), clipped by the slice [:nb]         (lib :914-917)
__device__ __forceinline__ int select_nb(int ncand, double noise_pop) {
  const int nb = 1 + (int)floor((double)ncand / noise_pop);
  return nb > ncand ? ncand : nb;
}

// One radix pass's pick, by wave 0: the bucket of hist[256] that holds rank *s_remaining, through a
// 64-lane prefix scan of four buckets per lane.  Leaves the rank inside that bucket in
// *s_remaining and `prefix` with the bucket's digit at `shift` in *s_prefix; s_done (may be null):
// whether the bucket holds a single element, which is then the answer.
__device__ __forceinline__ void select_pick_bucket(const int *hist, unsigned long long prefix,
                                                   int shift, int *s_remaining,
                                                   unsigned long long *s_prefix, int *s_done) {
  const int lane = threadIdx.x;
  const int rem0 = *s_remaining;
  const int h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2],
            h3 = hist[4 * lane + 3];
  const int mine = h0 + h1 + h2 + h3;
  int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int excl = incl - mine;
  if (rem0 >= excl && rem0 < incl) {  // exactly one lane
    int rem = rem0 - excl, b = 4 * lane, hb = h0;
    if (rem >= h0) {
      rem -= h0, ++b, hb = h1;
      if (rem >= h1) {
        rem -= h1, ++b, hb = h2;
        if (rem >= h2) rem -= h2, ++b, hb = h3;
      }
    }
    *s_remaining = rem;
    *s_prefix = prefix | ((unsigned long long)b << shift);
    if (s_done) *s_done = hb == 1;  // (then rem == 0)
  }
}

// the counts of an area that goes on; if x_red.shape[1] == 1: break              (lib :927-928)
__device__ __forceinline__ void select_finish(const SelectArgs &s, int a, int n, int nb) {
  if (threadIdx.x != 0) return;
  s.nb_out[a] = nb;
  if (n == 1) s.active[a] = 0;
  s.n_out[a] = n == 1 ? 0 : n;
}

// The general kernel, for areas of any size: the O2 values are streamed from memory in every pass,
// one block scan per 1024-entry chunk.
__device__ __forceinline__ void pca_select_body(const SelectArgs &s) {
  __shared__ int wtot[16];
  __shared__ int hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_remaining, s_it;
  const int a = blockIdx.x;
  const int tid = threadIdx.x;
  const long o0 = s.spx_off[a];
  const int ns = (int)(s.spx_off[a + 1] - o0);
  if (!select_enter(s, a)) return;
  const double thr = s.thr[a];
  BlockScan scan{wtot};
  auto tval = [&](int i) -> double { return s.test[s.spx[o0 + i]]; };

  // ---- pass 1: nuisance compaction in index order (np.where(test > thr)), candidates count
  int n = 0, ncand = 0;
  for (int c0 = 0; c0 < ns; c0 += 1024) {
    const int i = c0 + tid;
    const bool valid = i < ns;
    const double t = valid ? tval(i) : 0.0;
    const bool isn = valid && (t > thr);
    const int sp = isn ? s.spx[o0 + i] : 0;
    const bool cand = valid && (t > 0.0) && (t <= thr);
    int tot;
    const int r = scan.exclusive(isn, tot);
    if (isn) {
      s.nuis[o0 + n + r] = sp;
      s.nuis_pos[o0 + n + r] = (int)(o0 + i);
      s.mapO2[sp] += 1;  // mapO2[pypx] += 1                                     (lib :901)
    }
    n += tot;
    int tc;
    scan.exclusive(cand, tc);
    ncand += tc;
  }
  if (n == 0) {  // while len(pypx) > 0                                           (lib :899)
    select_stop(s, a);
    return;
  }
  __syncthreads();
  if (select_itermax_stop(s, a, &s_it)) return;
  const int nb = select_nb(ncand, s.noise_pop);

  if (nb > 0) {
    // ---- radix select of the nb-th smallest candidate (keys: bits of positive doubles)
    if (tid == 0) s_prefix = 0ull, s_remaining = nb - 1;
    unsigned long long maskbits = 0ull;
    for (int pass = 7; pass >= 0; --pass) {
      const int shift = pass * 8;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
      for (int i = tid; i < ns; i += 1024) {
        const double t = tval(i);
        if ((t > 0.0) && (t <= thr)) {
          const unsigned long long key = (unsigned long long)__double_as_longlong(t);
          if ((key & maskbits) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
        }
      }
      __syncthreads();
      if (tid < 64) select_pick_bucket(hist, prefix, shift, &s_remaining, &s_prefix, nullptr);
      maskbits |= 255ull << shift;
      __syncthreads();
    }
    const unsigned long long tau = s_prefix;
    const int need_equal = s_remaining + 1;
    // ---- emit the background columns.  The reference indexes the *filtered* vector
    // test[test > 0] and uses those indices on the unfiltered columns (lib :908-917): the
    // column of a selected element is its rank among the elements with test > 0.
    int nfilt = 0, neq = 0, nemit = 0;
    for (int c0 = 0; c0 < ns; c0 += 1024) {
      const int i = c0 + tid;
      const bool valid = i < ns;
      const double t = valid ? tval(i) : 0.0;
      const bool pos = valid && (t > 0.0);
      const bool cand = pos && (t <= thr);
      const unsigned long long key = (unsigned long long)__double_as_longlong(t);
      int tf, te, tm;
      const int rf = scan.exclusive(pos, tf);
      const bool eq = cand && key == tau;
      const int re = scan.exclusive(eq, te);
      const bool emit = cand && (key < tau || (eq && (neq + re) < need_equal));
      const int rm = scan.exclusive(emit, tm);
      if (emit) {
        s.bg[o0 + nemit + rm] = s.spx[o0 + nfilt + rf];
        s.bg_pos[o0 + nemit + rm] = (int)(o0 + nfilt + rf);
      }
      nfilt += tf;
      neq += te;
      nemit += tm;
    }
  }
  select_finish(s, a, n, nb);
}

// Same selection for areas of at most 1024 * SEL_EPT spaxels (every 100 x 100 area), built for
// the latency of a one-block kernel: thread t owns the SEL_EPT consecutive list entries
// [t*E, (t+1)*E) in registers, so index order is (thread, local) order and each compaction is ONE
// block scan of per-thread counts instead of one scan per 1024-entry chunk (3 scans + a few
// radix passes instead of ~50 scans).  Results are identical to pca_select_kernel.
constexpr int SEL_EPT = 12;

__device__ __forceinline__ unsigned long long block_scan_u64(unsigned long long v,
                                                             unsigned long long *wsum,
                                                             unsigned long long &total) {
  // inclusive scan inside the wave, exclusive across waves; returns the exclusive prefix
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  __syncthreads();  // previous users of wsum are done
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  unsigned long long pre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const unsigned long long c = wsum[w];
    pre += (w < wave) ? c : 0ull;
    tot += c;
  }
  total = tot;
  return pre + incl - v;
}

__device__ __forceinline__ void pca_select_fast_body(const SelectArgs &s) {
  __shared__ unsigned long long wsum[16], wmax[16];
  __shared__ unsigned bmap[1024 * SEL_EPT / 32];  // list positions emitted as background
  __shared__ int hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_remaining, s_it, s_done;
  extern __shared__ int scache[];  // spaxel index of every list entry (for the filtered-index quirk)
  const int a = blockIdx.x;
  const int tid = threadIdx.x;
  const long o0 = s.spx_off[a];
  const int ns = (int)(s.spx_off[a + 1] - o0);
  if (!select_enter(s, a)) return;
  const double thr = s.thr[a];
  const int E = (ns + 1023) / 1024;  // entries per thread (<= SEL_EPT)
  const int i0 = tid * E;
  // two batches of independent loads: indices, then values
  int sp[SEL_EPT];
  double tv[SEL_EPT];
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e) sp[e] = (e < E && i0 + e < ns) ? s.spx[o0 + i0 + e] : -1;
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e) tv[e] = sp[e] >= 0 ? s.test[sp[e]] : 0.0;
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e)
    if (sp[e] >= 0) scache[i0 + e] = sp[e];
  // membership of the previous iteration's background set (see the end of this function)
  unsigned oldmask = 0;
  {
    uint8_t ob[SEL_EPT];
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e) ob[e] = sp[e] >= 0 ? s.inB[o0 + i0 + e] : (uint8_t)0;
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e) oldmask |= (unsigned)(ob[e] != 0) << e;
    // (the mask is formed here: left to itself the compiler carries the loaded flags to the end
    // of the kernel, twelve registers more than the 128 a block of 1024 threads has)
    asm volatile("" : "+v"(oldmask));
    for (int i = tid; i < 1024 * SEL_EPT / 32; i += 1024) bmap[i] = 0u;
  }

  // ---- counts: nuisance (t > thr), candidates (0 < t <= thr), positive (t > 0)
  unsigned long long cnt = 0;  // [nuis | cand | pos] x 20 bits
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e) {
    const bool v = sp[e] >= 0;
    const bool isn = v && tv[e] > thr, pos = v && tv[e] > 0.0, cand = pos && tv[e] <= thr;
    cnt += ((unsigned long long)isn << 40) + ((unsigned long long)cand << 20) + (unsigned long long)pos;
  }
  unsigned long long tot;
  const unsigned long long pre = block_scan_u64(cnt, wsum, tot);
  const int n = (int)(tot >> 40), ncand = (int)((tot >> 20) & 0xfffff);
  if (n == 0) {  // while len(pypx) > 0                                           (lib :899)
    select_stop(s, a);
    return;
  }
  {  // nuisance compaction in index order (np.where(test > thr)); mapO2[pypx] += 1   (lib :901, before the itermax test)
    int rn = (int)(pre >> 40);
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e)
      if (sp[e] >= 0 && tv[e] > thr) {
        s.nuis[o0 + rn] = sp[e];
        s.nuis_pos[o0 + rn] = (int)(o0 + i0 + e);
        s.mapO2[sp[e]] += 1;
        ++rn;
      }
  }
  if (select_itermax_stop(s, a, &s_it)) return;
  const int nb = select_nb(ncand, s.noise_pop);

  if (nb > 0) {
    // ---- radix select of the nb-th smallest candidate (keys: bits of positive doubles).
    // The O2 values of an area sit in a narrow range around 1, so the leading bytes of all
    // keys coincide and a histogram over them is one LDS counter hit by every thread.  The
    // digits are therefore taken from key - min(key), most significant bit of the RANGE first
    // (8 bits per pass), and the passes stop as soon as the bucket holding the wanted rank has
    // a single element -- typically after two or three passes instead of eight.
    unsigned long long kmin = ~0ull, kmax = 0ull;
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e)
      if (sp[e] >= 0 && tv[e] > 0.0 && tv[e] <= thr) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(tv[e]);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
      }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o1 = __shfl_xor(kmin, off, 64), o2 = __shfl_xor(kmax, off, 64);
      kmin = o1 < kmin ? o1 : kmin;
      kmax = o2 > kmax ? o2 : kmax;
    }
    __syncthreads();  // previous users of wsum are done
    if ((tid & 63) == 0) wsum[tid >> 6] = kmin, wmax[tid >> 6] = kmax;
    if (tid == 0) s_prefix = 0ull, s_remaining = nb - 1, s_done = 0;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      kmin = wsum[w] < kmin ? wsum[w] : kmin;
      kmax = wmax[w] > kmax ? wmax[w] : kmax;
    }
    const unsigned long long range = kmax - kmin;  // nb > 0: there is at least one candidate
    int hi_bit = range ? 64 - __clzll((long long)range) : 0;  // digits below this bit
    while (hi_bit > 0) {
      const int lo_bit = hi_bit > 8 ? hi_bit - 8 : 0;
      const unsigned long long above = hi_bit >= 64 ? 0ull : ~0ull << hi_bit;  // decided bits
      const unsigned dmask = (1u << (hi_bit - lo_bit)) - 1u;
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      const unsigned long long prefix = s_prefix;
#pragma unroll
      for (int e = 0; e < SEL_EPT; ++e)
        if (sp[e] >= 0 && tv[e] > 0.0 && tv[e] <= thr) {
          const unsigned long long key =
              (unsigned long long)__double_as_longlong(tv[e]) - kmin;
          if ((key & above) == prefix) atomicAdd(&hist[(int)((unsigned)(key >> lo_bit) & dmask)], 1);
        }
      __syncthreads();
      if (tid < 64) select_pick_bucket(hist, prefix, lo_bit, &s_remaining, &s_prefix, &s_done);
      __syncthreads();
      hi_bit = lo_bit;
      if (s_done) break;
    }
    if (hi_bit > 0) {  // stopped early: the one candidate matching the decided bits
      const unsigned long long above = ~0ull << hi_bit, prefix = s_prefix;
      __syncthreads();  // everyone has read s_prefix
#pragma unroll
      for (int e = 0; e < SEL_EPT; ++e)
        if (sp[e] >= 0 && tv[e] > 0.0 && tv[e] <= thr) {
          const unsigned long long key =
              (unsigned long long)__double_as_longlong(tv[e]) - kmin;
          if ((key & above) == prefix) s_prefix = key;
        }
      __syncthreads();
    }
    const unsigned long long tau = s_prefix + kmin;
    const int need_equal = s_remaining + 1;
    // ---- emit the background columns.  The reference indexes the *filtered* vector
    // test[test > 0] and uses those indices on the unfiltered columns (lib :908-917): the
    // column of a selected element is its rank among the elements with test > 0.
    unsigned long long ce = 0;  // [eq | below] x 20 bits
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e)
      if (sp[e] >= 0 && tv[e] > 0.0 && tv[e] <= thr) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(tv[e]);
        ce += ((unsigned long long)(key == tau) << 20) + (unsigned long long)(key < tau);
      }
    unsigned long long tot2;
    const unsigned long long pre2 = block_scan_u64(ce, wsum, tot2);
    // emitted before this thread: all smaller keys before it + the first equal ones (index order)
    int eq_before = (int)(pre2 >> 20);
    int emit_before = (int)(pre2 & 0xfffff) + min(eq_before, need_equal);
    int rp = (int)(pre & 0xfffff);  // rank among the positive elements
#pragma unroll
    for (int e = 0; e < SEL_EPT; ++e) {
      if (sp[e] < 0 || !(tv[e] > 0.0)) continue;
      if (tv[e] <= thr) {
        const unsigned long long key = (unsigned long long)__double_as_longlong(tv[e]);
        const bool eq = key == tau;
        const bool emit = key < tau || (eq && eq_before < need_equal);
        if (emit) {
          s.bg[o0 + emit_before] = scache[rp];
          s.bg_pos[o0 + emit_before] = (int)(o0 + rp);
          atomicOr(&bmap[rp >> 5], 1u << (rp & 31));
          ++emit_before;
        }
        eq_before += eq;
      }
      ++rp;
    }
  }
  // The background set changes by a few columns per iteration (the O2 tests move slowly), so
  // its mean is updated from the columns that entered or left it instead of re-gathered
  // (bmean_kernel).  Here: the changes of membership in list order -- +(spaxel+1) entered,
  // -(spaxel+1) left -- and the new membership flags.
  __syncthreads();  // bmap complete
  unsigned newmask = 0;
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e)
    if (sp[e] >= 0) newmask |= ((bmap[(i0 + e) >> 5] >> ((i0 + e) & 31)) & 1u) << e;
  const unsigned diff = newmask ^ oldmask;
  unsigned long long tot3;
  int r = (int)block_scan_u64((unsigned long long)__popc(diff), wsum, tot3);
#pragma unroll
  for (int e = 0; e < SEL_EPT; ++e)
    if ((diff >> e) & 1u) {
      const bool in = (newmask >> e) & 1u;
      s.dlist[o0 + r++] = in ? sp[e] + 1 : -(sp[e] + 1);
      s.inB[o0 + i0 + e] = (uint8_t)in;
    }
  if (tid == 0) s.ndiff[a] = (int)tot3;
  select_finish(s, a, n, nb);
}

// The host sizes every launch of an iteration from n / nb of each area.  Instead of a D2H copy
// and a stream synchronisation (~30 us of wake-up latency per iteration), each block stores its
// two numbers straight into mapped, coherent host memory; the last block to finish (device
// counter) raises the generation flag the host spins on.
__device__ __forceinline__ void select_publish(const SelectArgs &s) {
  if (threadIdx.x != 0) return;
  if (!s.host_out) return;
  const int a = blockIdx.x, na = gridDim.x;
  s.host_out[a] = s.n_out[a];
  s.host_out[na + a] = s.nb_out[a];
  __threadfence_system();
  const unsigned old = atomicAdd(s.counter, 1u);
  if (old + 1u == (unsigned)na * (unsigned)s.gen) {
    __threadfence_system();
    __hip_atomic_store(s.host_out + 2 * na, s.gen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(1024) void pca_select_kernel(SelectArgs s) {
  pca_select_body(s);
  select_publish(s);
}

__global__ __launch_bounds__(1024) void pca_select_fast_kernel(SelectArgs s) {
  pca_select_fast_body(s);
  select_publish(s);
}

// ------------------------------------------------------------------------------------
// cbar_k[q] = mean_{i in bg_k} C[q][bg_pos_i], q < T_k           grid (nw), block 1024
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void cbar_kernel(const double *__restrict__ C, long ntot,
                                                    const int *__restrict__ bg_pos,
                                                    const long *__restrict__ D, int nw,
                                                    double *__restrict__ cbar) {
  const int k = blockIdx.x;
  const int T = (int)DSC(DF_T, k);
  const int nb = (int)DSC(DF_NB, k);
  const long o0 = DSC(DF_LIST0, k);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // every read below is an L2 round trip (~0.7 us): fetch the positions once, then keep the
  // gathers of a row independent (first 8 positions per lane from registers)
  int pos[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pos[e] = lane + 64 * e < nb ? bg_pos[o0 + lane + 64 * e] : -1;
  for (int q = wave; q < T; q += 16) {
    const double *row = C + (long)q * ntot;
    double v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = pos[e] >= 0 ? row[pos[e]] : 0.0;
    double acc = 0.0;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += v[e];  // same order as the plain loop
    for (int i = lane + 512; i < nb; i += 64) acc += row[bg_pos[o0 + i]];
    acc = wave_sum_d(acc);
    if (lane == 0) cbar[(long)k * PCA_CAP + q] = acc / (double)nb;
  }
}

// ------------------------------------------------------------------------------------
// b_k[z] = mean_{i in bg_k} F_t[z, bg_i] = mean_i X[z, bg_i] - sum_q U[z][q] cbar[q]
// grid (ceil(Nz/4), nw), block (64,4).  U layout: [area][z][PCA_CAP].
// A background column is a scattered gather (a 64-byte sector per sample), and the set moves by
// a few columns per iteration: with Ssum (float64 [area][Nz], the sum over the set as the
// previous iteration left it) and DF_SVALID the sum is updated from the columns that entered /
// left (dlist, signed, in list order: a fixed summation order) instead of re-gathered.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bmean_kernel(const float *__restrict__ X, int Nz, long S,
                                                    const int *__restrict__ bg,
                                                    const long *__restrict__ D, int nw,
                                                    const double *__restrict__ U,
                                                    const double *__restrict__ cbar,
                                                    double *__restrict__ b,
                                                    const int *__restrict__ dlist,
                                                    const int *__restrict__ ndiff,
                                                    double *__restrict__ Ssum) {
  const int k = blockIdx.y;
  const int z = blockIdx.x * 4 + threadIdx.y;
  if (z >= Nz) return;
  const long o0 = DSC(DF_LIST0, k);
  const int nb = (int)DSC(DF_NB, k), T = (int)DSC(DF_T, k);
  const int a = (int)DSC(DF_AREA, k);
  const float *row = X + (long)z * S;
  double part = 0.0;
  const bool delta = Ssum && DSC(DF_SVALID, k);
  if (delta) {
    const int nd = ndiff[a];
    for (int i = threadIdx.x; i < nd; i += 64) {
      const int e = dlist[o0 + i];
      const double v = (double)row[(e > 0 ? e : -e) - 1];
      part += e > 0 ? v : -v;
    }
  } else {
    for (int i = threadIdx.x; i < nb; i += 64) part += (double)row[bg[o0 + i]];
  }
  double tot = wave_sum_d(part);
  if (delta) tot += Ssum[(long)a * Nz + z];
  if (Ssum && threadIdx.x == 0) Ssum[(long)a * Nz + z] = tot;
  double acc = 0.0;
  if ((int)threadIdx.x < T)  // T <= PCA_CAP == 64 lanes
    acc = U[((long)a * Nz + z) * PCA_CAP + threadIdx.x] * cbar[(long)k * PCA_CAP + threadIdx.x];
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) b[(long)k * Nz + z] = tot / (double)nb - acc;
}

// ------------------------------------------------------------------------------------
// Nuisance block of F_t (float64, [Nz][ld]):  Fb[z][j] = F_t[z, col_j]
// and the partial c_j = b^T Fb_j of the block's z slice.
// The nuisance set only shrinks (the O2 tests only decrease), so the columns of iteration t are
// a subsequence of those of iteration t-1: when the previous block of the area is at hand
// (DF_FBOLD >= 0) column j is its old column (found by the list position, binary search) minus
// the one deflation since,  F_t = F_{t-1} - u_{t-1} c_{t-1}^T  -- no read of the cube (a
// scattered column costs a 64-byte sector per 4-byte sample).  Otherwise (first iteration of an
// area, or after a flush)  Fb[z][j] = X[z, col_j] - sum_q U[z][q] C[q][pos_j].
// grid (ceil(ldmax/64), nw, z slices), block (64 columns, 16 waves over z)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void gather_xp_kernel(
    const float *__restrict__ X, int Nz, long S, const int *__restrict__ nuis,
    const int *__restrict__ nuis_pos, const int *__restrict__ nuis_pos_old,
    const long *__restrict__ D, int nw, const double *__restrict__ b,
    const double *__restrict__ U, const double *__restrict__ C, long ntot,
    const double *__restrict__ Fold, double *__restrict__ Fb, double *__restrict__ cpart,
    long ctot, int zper) {
  __shared__ double red[16][64];
  __shared__ double Cn[PCA_CAP][64];  // coefficients of this block's 64 columns
  const int k = blockIdx.y;
  const int ld = (int)DSC(DF_LD, k);
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (blockIdx.x * 64 >= ld) return;  // whole block out of range (uniform)
  const int n = (int)DSC(DF_N, k), T = (int)DSC(DF_T, k);
  const bool live = j < n;   // real nuisance column
  const bool inld = j < ld;  // padded column (stored as zeros)
  const long list0 = DSC(DF_LIST0, k);
  const long col = live ? (long)nuis[list0 + j] : 0;
  const long pos = live ? (long)nuis_pos[list0 + j] : 0;
  const double *bk = b + (long)k * Nz;
  const double *Ua = U + (long)DSC(DF_AREA, k) * Nz * PCA_CAP;
  double *Fk = Fb + DSC(DF_XP, k);
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.y);
  const int z0 = blockIdx.z * zper, z1 = min(Nz, z0 + zper);
  const long fbold = DSC(DF_FBOLD, k);
  double acc = 0.0;
  if (fbold >= 0) {
    // ---- from the previous block: column with the same list position
    const int nold = (int)DSC(DF_NOLD, k), ldold = (int)DSC(DF_LDOLD, k);
    int io = 0;
    if (live) {
      int lo = 0, hi = nold - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long)nuis_pos_old[list0 + mid] < pos) lo = mid + 1;
        else hi = mid;
      }
      io = lo;
    }
    const double cprev = live ? C[(long)(T - 1) * ntot + pos] : 0.0;
    const double *Fo = Fold + fbold;
    // four channels per trip with their loads issued together (each is an L2 round trip)
    for (int z = z0 + w; z < z1; z += 64) {
      double fo[4], uu[4], bb[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int zz = z + 16 * s;
        const long zc = zz < z1 ? zz : z0;
        fo[s] = live ? Fo[zc * ldold + io] : 0.0;
        uu[s] = Ua[zc * PCA_CAP + (T - 1)];
        bb[s] = bk[zc];
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int zz = z + 16 * s;
        if (zz < z1) {
          const double v = live ? fma(-uu[s], cprev, fo[s]) : 0.0;
          if (inld) Fk[(long)zz * ld + j] = v;
          acc = fma(bb[s], v, acc);
        }
      }
    }
  } else {
    for (int q = w; q < T; q += 16) Cn[q][threadIdx.x] = live ? C[(long)q * ntot + pos] : 0.0;
    __syncthreads();
    for (int z = z0 + w; z < z1; z += 16) {
      double v = live ? (double)X[(long)z * S + col] : 0.0;
      const double *uz = Ua + (long)z * PCA_CAP;  // wave-uniform row of U -> scalar loads
      for (int q = 0; q < T; ++q) v = fma(-uz[q], Cn[q][threadIdx.x], v);
      if (inld) Fk[(long)z * ld + j] = v;
      acc = fma(bk[z], v, acc);
    }
  }
  red[threadIdx.y][threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.y == 0 && inld) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += red[q][threadIdx.x];
    cpart[(long)blockIdx.z * ctot + DSC(DF_C, k) + j] = t;
  }
}

// Xp[z][j] = Fb[z][j] - b[z] c[j]       grid (ceil(Nz/16), nw), block 256 (lanes over columns)
// (out of place: Fb stays as the next iteration's source)
__global__ __launch_bounds__(256) void project_xp_kernel(const double *__restrict__ b, int Nz,
                                                         const long *__restrict__ D, int nw,
                                                         const double *__restrict__ Fb,
                                                         double *__restrict__ Xp,
                                                         const double *__restrict__ cpart,
                                                         long ctot, int nzb) {
  const int k = blockIdx.y;
  const int ld = (int)DSC(DF_LD, k);
  const double *F = Fb + DSC(DF_XP, k);
  double *X = Xp + DSC(DF_XP, k);
  const double *c = cpart + DSC(DF_C, k);
  const double *bk = b + (long)k * Nz;
  const int z0 = blockIdx.x * 16, z1 = min(Nz, z0 + 16);
  for (int j = threadIdx.x; j < ld; j += 256) {
    // all loads of the column first (independent), then the arithmetic
    double cq[16], f[16], bz[16];  // nzb <= 16, 16 channels per block
#pragma unroll
    for (int q = 0; q < 16; ++q) cq[q] = q < nzb ? c[(long)q * ctot + j] : 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int z = z0 + e < z1 ? z0 + e : z0;
      f[e] = F[(long)z * ld + j];
      bz[e] = bk[z];
    }
    double cj = 0.0;  // c_j = b^T F_j, summed over the z slices of the gather in fixed order
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (q < nzb) cj += cq[q];
#pragma unroll
    for (int e = 0; e < 16; ++e)
      if (z0 + e < z1) X[(long)(z0 + e) * ld + j] = fma(-bz[e], cj, f[e]);
  }
}

// ------------------------------------------------------------------------------------
// G = Xp^T Xp with v_mfma_f64_16x16x4_f64.
// One wave computes a 32x32 tile (2x2 MFMA tiles) of the upper triangle for one K-slice of
// the channels; slabs are summed in fixed order by gram_reduce_kernel and mirrored.
//   A operand (16x4): lane l holds A[i = l&15][k = l>>4] = Xp[k0 + (l>>4)][i0 + (l&15)]
//   B operand (4x16): lane l holds B[k = l>>4][j = l&15] = Xp[k0 + (l>>4)][j0 + (l&15)]
//   D (16x16): lane l, reg r holds D[row = (l>>4) + 4r][col = l&15]
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void gram_kernel(const double *__restrict__ Xp,
                                                  const long *__restrict__ xp_off,
                                                  const long *__restrict__ ld_,
                                                  const int *__restrict__ tile_i,
                                                  const int *__restrict__ tile_j,
                                                  const int *__restrict__ tile_a, int Nz,
                                                  int ksplit, double *__restrict__ slab,
                                                  const long *__restrict__ g_off,
                                                  long slab_stride,
                                                  const long *__restrict__ n_) {
  const int t = blockIdx.x;
  const int a = tile_a[t];
  if (n_ && n_[a] < 2) return;  // the area finished with this iteration's selection
  const int ld = (int)ld_[a];
  const int i0 = tile_i[t] * 32, j0 = tile_j[t] * 32;
  const int ks = blockIdx.y;
  const int zper = ((Nz + ksplit - 1) / ksplit + 3) & ~3;
  const int z0 = ks * zper, z1 = min(Nz, z0 + zper);
  const double *X = Xp + xp_off[a];
  const int lane = threadIdx.x;
  const int r16 = lane & 15, kq = lane >> 4;
  // columns beyond ld (ld is a multiple of 16, tiles are 32 wide) are clamped and zeroed
  const bool ia0 = i0 + r16 < ld, ia1 = i0 + 16 + r16 < ld;
  const bool jb0 = j0 + r16 < ld, jb1 = j0 + 16 + r16 < ld;
  double4_t acc00 = {0, 0, 0, 0}, acc01 = {0, 0, 0, 0}, acc10 = {0, 0, 0, 0}, acc11 = {0, 0, 0, 0};
  // eight k-steps (32 channels) per trip: the 32 loads are issued together -- a trip with one
  // k-step waits a whole L2 round trip (~0.7 us) for four loads
  for (int z = z0; z < z1; z += 32) {
    double a0[8], a1[8], b0[8], b1[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int zz = z + 4 * s + kq;
      const bool zin = zz < z1;
      const double *row = X + (long)(zin ? zz : z0) * ld;
      a0[s] = (zin && ia0) ? row[i0 + r16] : 0.0;
      a1[s] = (zin && ia1) ? row[i0 + 16 + r16] : 0.0;
      b0[s] = (zin && jb0) ? row[j0 + r16] : 0.0;
      b1[s] = (zin && jb1) ? row[j0 + 16 + r16] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      acc00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b0[s], acc00, 0, 0, 0);
      acc01 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s], b1[s], acc01, 0, 0, 0);
      acc10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b0[s], acc10, 0, 0, 0);
      acc11 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s], b1[s], acc11, 0, 0, 0);
    }
  }
  double *G = slab + (long)ks * slab_stride + g_off[a];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = kq + 4 * r;
    const int gi0 = i0 + row, gi1 = i0 + 16 + row;
    const int gj0 = j0 + r16, gj1 = j0 + 16 + r16;
    if (gi0 < ld && gj0 < ld) G[(long)gi0 * ld + gj0] = acc00[r];
    if (gi0 < ld && gj1 < ld) G[(long)gi0 * ld + gj1] = acc01[r];
    if (gi1 < ld && gj0 < ld) G[(long)gi1 * ld + gj0] = acc10[r];
    if (gi1 < ld && gj1 < ld) G[(long)gi1 * ld + gj1] = acc11[r];
  }
}

// G[i][j] = sum_ks slab[ks][i][j] for tile (ti <= tj), mirrored into the lower triangle
__global__ __launch_bounds__(256) void gram_reduce_kernel(const double *__restrict__ slab,
                                                          long slab_stride, int ksplit,
                                                          const long *__restrict__ ld_,
                                                          const int *__restrict__ tile_i,
                                                          const int *__restrict__ tile_j,
                                                          const int *__restrict__ tile_a,
                                                          double *__restrict__ G,
                                                          const long *__restrict__ g_off,
                                                          const long *__restrict__ n_) {
  const int t = blockIdx.x;
  const int a = tile_a[t];
  if (n_ && n_[a] < 2) return;
  const int ld = (int)ld_[a];
  const int i0 = tile_i[t] * 32, j0 = tile_j[t] * 32;
  double *Ga = G + g_off[a];
  for (int e = threadIdx.x; e < 1024; e += 256) {
    const int i = i0 + (e >> 5), j = j0 + (e & 31);
    if (i >= ld || j >= ld) continue;
    double acc = 0.0;
    for (int ks = 0; ks < ksplit; ++ks)
      acc += slab[(long)ks * slab_stride + g_off[a] + (long)i * ld + j];
    Ga[(long)i * ld + j] = acc;
    Ga[(long)j * ld + i] = acc;
  }
}

// ------------------------------------------------------------------------------------
// u = Xp v, then normalised and appended to U.     grid (ceil(Nz/4), nw), block (64,4)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void xv_kernel(const double *__restrict__ Xp,
                                                 const long *__restrict__ D, int nw, int Nz,
                                                 const double *__restrict__ v,
                                                 double *__restrict__ u) {
  const int k = blockIdx.y;
  const int z = blockIdx.x * 4 + threadIdx.y;
  if (z >= Nz) return;
  const int ld = (int)DSC(DF_LD, k), n = (int)DSC(DF_N, k);
  const double *row = Xp + DSC(DF_XP, k) + (long)z * ld;
  const double *vk = v + DSC(DF_C, k);
  double acc = 0.0;
  for (int j = threadIdx.x; j < n; j += 64) acc = fma(row[j], vk[j], acc);
  acc = wave_sum_d(acc);
  if (threadIdx.x == 0) u[(long)k * Nz + z] = acc;
}

// w_k[q] = u_k . U[:, q] (q < T_k) and |u_k|^2 of the not yet normalised u_k, as partial sums over
// UW_SLICES slices of z: grid (UW_SLICES, nw), block 256; lanes over q, waves over the rows of a
// slice.  part[(k * UW_SLICES + b) * (PCA_CAP + 1) + q], entry PCA_CAP = the slice's sum of squares.
constexpr int UW_SLICES = 32;
__global__ __launch_bounds__(256) void uw_partial_kernel(const double *__restrict__ u, int Nz,
                                                         const long *__restrict__ D, int nw,
                                                         const double *__restrict__ U,
                                                         double *__restrict__ part) {
  __shared__ double wred[4][PCA_CAP + 1];
  const int k = blockIdx.y, b = blockIdx.x;
  const int T = (int)DSC(DF_T, k);
  const double *uk = u + (long)k * Nz;
  const double *Ua = U + (long)DSC(DF_AREA, k) * Nz * PCA_CAP;
  const int zs = (Nz + UW_SLICES - 1) / UW_SLICES;
  const int z0 = b * zs, z1 = min(Nz, z0 + zs);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double a = 0.0, s2 = 0.0;
  for (int z = z0 + wave; z < z1; z += 4) {
    const double uz = uk[z];
    s2 = fma(uz, uz, s2);
    if (lane < T) a = fma(uz, Ua[(long)z * PCA_CAP + lane], a);
  }
  wred[wave][lane] = a;
  if (lane == 0) wred[wave][PCA_CAP] = s2;
  __syncthreads();
  if (threadIdx.x <= PCA_CAP) {
    const int q = threadIdx.x;
    part[((long)k * UW_SLICES + b) * (PCA_CAP + 1) + q] =
        ((wred[0][q] + wred[1][q]) + wred[2][q]) + wred[3][q];
  }
}

// normalise u_k, store it as column T_k of U, and w_k[q] = u_k . U[:, q] for q < T_k
__global__ __launch_bounds__(1024) void normalize_kernel(double *__restrict__ u, int Nz,
                                                         const long *__restrict__ D, int nw,
                                                         double *__restrict__ U,
                                                         const double *__restrict__ part,
                                                         double *__restrict__ wq) {
  __shared__ double s_inv;
  const int k = blockIdx.x;
  const int T = (int)DSC(DF_T, k);
  double *uk = u + (long)k * Nz;
  double *Ua = U + (long)DSC(DF_AREA, k) * Nz * PCA_CAP;
  const double *pk = part + (long)k * UW_SLICES * (PCA_CAP + 1);
  double acc = 0.0;
  if (threadIdx.x <= PCA_CAP) {  // fixed-order sums over the slices
#pragma unroll 8
    for (int b = 0; b < UW_SLICES; ++b) acc += pk[(long)b * (PCA_CAP + 1) + threadIdx.x];
    if (threadIdx.x == PCA_CAP) s_inv = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
  }
  __syncthreads();
  const double inv = s_inv;
  if ((int)threadIdx.x < T) wq[(long)k * PCA_CAP + threadIdx.x] = acc * inv;
  for (int z = threadIdx.x; z < Nz; z += 1024) {
    const double x = uk[z] * inv;
    uk[z] = x;
    Ua[(long)z * PCA_CAP + T] = x;
  }
}

// ------------------------------------------------------------------------------------
// deflation of whole areas in coefficient form.
//   dot    : cpart[zs][i] = sum_{z in slice zs} u_k[z] X[z, spx[i]]
//   finish : c_i = sum_zs cpart - sum_q w[q] C[q][i] (= u^T F_{t-1,i});  C[T][i] = c_i;
//            test[spx[i]] -= c_i^2 / Nz          (|F_t|^2 = |F_{t-1}|^2 - c^2, |u| = 1)
// grid (ceil(nsmax/256), ZS, nw) / (ceil(nsmax/256), nw); 256 lanes over the area's list
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void deflate_dot_kernel(const float *__restrict__ F, int Nz,
                                                          long S, const int *__restrict__ spx,
                                                          const long *__restrict__ D, int nw,
                                                          const double *__restrict__ u, int zper,
                                                          double *__restrict__ cpart, long ntot) {
  const int k = blockIdx.z;
  const int ns = (int)DSC(DF_NS, k);
  const int li = blockIdx.x * 256 + threadIdx.x;
  if (blockIdx.x * 256 >= ns) return;
  const bool live = li < ns;
  const long col = spx[DSC(DF_LIST0, k) + (live ? li : ns - 1)];
  const double *uk = u + (long)k * Nz;
  const int z0 = blockIdx.y * zper, z1 = min(Nz, z0 + zper);
  double acc = 0.0;
#pragma unroll 4
  for (int z = z0; z < z1; ++z) acc = fma(uk[z], (double)F[(long)z * S + col], acc);
  if (live) cpart[(long)blockIdx.y * ntot + DSC(DF_CBASE, k) + li] = acc;
}

// The same dot products with the block -> memory mapping of the cube instead of the areas':
// 256 consecutive spaxels of the flattened (Ny, Nx) plane per block, each lane looking up its
// area (area_of), the area's slot in this iteration's work list (kidx, -1: not iterating) and
// its list position (pos_of).  An area row of 100 float32 cuts the 128-byte lines at both ends,
// and with one block set per area every cut line is fetched twice (measured: 4.7 TB/s of
// algorithmic bytes with 100-wide areas against 6.3 TB/s with 128-wide ones); here every line
// is fetched once, whole.  Same z slices and summation order as deflate_dot_kernel: identical partial sums.
// Used while the iterating areas cover most of the field.  grid (ceil(S/256), ZS)
__global__ __launch_bounds__(256) void deflate_dot_rows_kernel(
    const float *__restrict__ F, int Nz, long S, const int *__restrict__ area_of,
    const int *__restrict__ pos_of, const int *__restrict__ kidx, const long *__restrict__ D,
    int nw, const double *__restrict__ u, int zper, double *__restrict__ cpart, long ntot) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  int k = -1;
  if (s < S) {
    const int a = area_of[s];
    if (a >= 0) k = kidx[a];
  }
  if (!__any(k >= 0)) return;  // nothing of this wave's 64 spaxels iterates (no block barrier used)
  const long sc = k >= 0 ? s : (long)blockIdx.x * 256;  // idle lanes re-read the block's first spaxel
  const double *uk = u + (long)(k >= 0 ? k : 0) * Nz;  // per-lane load; lanes of one area share it
  const int z0 = blockIdx.y * zper, z1 = min(Nz, z0 + zper);
  double acc = 0.0;
#pragma unroll 4
  for (int z = z0; z < z1; ++z) acc = fma(uk[z], (double)F[(long)z * S + sc], acc);
  if (k >= 0)
    cpart[(long)blockIdx.y * ntot + DSC(DF_CBASE, k) + (pos_of[s] - DSC(DF_LIST0, k))] = acc;
}

// area_of[s] / pos_of[s]: the area (index) holding spaxel s and its position in the
// concatenated lists; area_of is preset to -1.   grid (ceil(nsmax/256), na)
__global__ __launch_bounds__(256) void invert_lists_kernel(const int *__restrict__ spx,
                                                           const long *__restrict__ spx_off,
                                                           int *__restrict__ area_of,
                                                           int *__restrict__ pos_of) {
  const int a = blockIdx.y;
  const long o0 = spx_off[a];
  const long i = o0 + (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= spx_off[a + 1]) return;
  const int s = spx[i];
  area_of[s] = a;
  pos_of[s] = (int)i;
}

__global__ __launch_bounds__(256) void deflate_finish_kernel(const int *__restrict__ spx,
                                                             const long *__restrict__ D, int nw,
                                                             int nzs, int Nz, long cb_tot,
                                                             const double *__restrict__ cpart,
                                                             const double *__restrict__ wq,
                                                             double *__restrict__ C, long ntot,
                                                             double *__restrict__ test) {
  const int k = blockIdx.y;
  const int ns = (int)DSC(DF_NS, k);
  const int li = blockIdx.x * 256 + threadIdx.x;
  if (li >= ns) return;
  const int T = (int)DSC(DF_T, k);
  const long pos = DSC(DF_LIST0, k) + li;
  const long ci = DSC(DF_CBASE, k) + li;
  double c = 0.0;
  {  // loads of a batch are independent (L2 latency), the sums keep their order
    int q = 0;
    for (; q + 8 <= nzs; q += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = cpart[(long)(q + e) * cb_tot + ci];
#pragma unroll
      for (int e = 0; e < 8; ++e) c += v[e];
    }
    for (; q < nzs; ++q) c += cpart[(long)q * cb_tot + ci];
  }
  const double *w = wq + (long)k * PCA_CAP;
  {
    int q = 0;
    for (; q + 8 <= T; q += 8) {
      double v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = C[(long)(q + e) * ntot + pos];
#pragma unroll
      for (int e = 0; e < 8; ++e) c = fma(-w[q + e], v[e], c);
    }
    for (; q < T; ++q) c = fma(-w[q], C[(long)q * ntot + pos], c);
  }
  C[(long)T * ntot + pos] = c;
  const long sp = spx[pos];
  test[sp] = test[sp] - c * c / (double)Nz;
}

// ------------------------------------------------------------------------------------
// flush: F[z, s] = X[z, s] - sum_{q < T_a} U[z][q] C[q][i]  (X may alias F; one float32 rounding)
// 1-D grid over (spaxel chunk, channel block, area), see the decoding below; thread = one spaxel x
// 32 channels, U rows in LDS
// ------------------------------------------------------------------------------------
constexpr int FLUSH_ZB = 32;  // channels per block
__global__ __launch_bounds__(256, 4) void flush_kernel(const float *X, float *F, int Nz, long S,
                                                    const int *__restrict__ spx,
                                                    const long *__restrict__ FD, int nf,
                                                    const double *__restrict__ U,
                                                    const double *__restrict__ C, long ntot,
                                                    int nxb, int nzb, int out_nx, long out_py,
                                                    long out_pz) {
  // out_nx > 0: F is a box inside a larger cube (the halo-extended tile of the tiled path):
  // spaxel col = y * out_nx + x of the (Nz, S) input goes to F[z * out_pz + y * out_py + x]
  // FD: [4][nf] = area, list0, ns, T
  __shared__ double Us[FLUSH_ZB][PCA_CAP];  // this block's rows of U (zero beyond T / Nz)
  // 1-D grid decoded so that the blocks of neighbouring areas for the same rows and channels
  // are 8 workgroup ids apart: same XCD (id mod 8), a few dispatches apart in time.  An area
  // row of 100 float32 cuts the 128-byte lines at both ends; when the two halves of a cut line
  // are written while the line is still in that XCD's L2 it goes to memory once, whole,
  // instead of as two partial writes (a read-modify-write each).
  const long id = blockIdx.x;
  const int low = (int)(id & 7);
  const long rest = id >> 3;
  const int k = (int)(rest % nf);
  const long cz = (rest / nf) * 8 + low;  // index over (spaxel chunk, channel block)
  if (cz >= (long)nxb * nzb) return;
  const int bx = (int)(cz % nxb), by = (int)(cz / nxb);
  const int ns = (int)FD[(long)2 * nf + k], T = (int)FD[(long)3 * nf + k];
  const int li = bx * 256 + threadIdx.x;
  if (bx * 256 >= ns) return;
  const bool live = li < ns;
  const long pos = FD[(long)1 * nf + k] + (live ? li : ns - 1);
  const long col = spx[pos];
  const long fcol = out_nx > 0 ? (col / out_nx) * out_py + (col % out_nx) : col;
  const long fS = out_nx > 0 ? out_pz : S;
  const double *Ua = U + FD[k] * (long)Nz * PCA_CAP;
  const int z0 = by * FLUSH_ZB;
  for (int i = threadIdx.x; i < FLUSH_ZB * PCA_CAP; i += 256) {
    const int r = i / PCA_CAP, q = i - r * PCA_CAP;
    Us[r][q] = (z0 + r < Nz && q < T) ? Ua[(long)(z0 + r) * PCA_CAP + q] : 0.0;
  }
  __syncthreads();
  // Register budget: 4 waves per SIMD (128 VGPRs) keep enough loads in flight for this pass to
  // stream; left alone the compiler hoists all 128 LDS reads of a coefficient batch (250 VGPRs,
  // 2 waves per SIMD, 2.9 TB/s).  Hence two rows of U per scheduling group, and the X column
  // loaded after the coefficient loop.
  double acc[FLUSH_ZB];
#pragma unroll
  for (int r = 0; r < FLUSH_ZB; ++r) acc[r] = 0.0;
  for (int q0 = 0; q0 < T; q0 += 8) {
    double c[8];  // independent loads; entries beyond T multiply zero rows of Us
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = q0 + e < T ? C[(long)(q0 + e) * ntot + pos] : 0.0;
#pragma unroll
    for (int r = 0; r < FLUSH_ZB; r += 2) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[r] = fma(Us[r][q0 + e], c[e], acc[r]);
        acc[r + 1] = fma(Us[r + 1][q0 + e], c[e], acc[r + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  float xv[FLUSH_ZB];
#pragma unroll
  for (int r = 0; r < FLUSH_ZB; ++r) xv[r] = X[(long)min(z0 + r, Nz - 1) * S + col];
  if (live) {
#pragma unroll
    for (int r = 0; r < FLUSH_ZB; ++r) {
      const int z = z0 + r;
      if (z < Nz) F[(long)z * fS + fcol] = (float)((double)xv[r] - acc[r]);
    }
  }
}

// ------------------------------------------------------------------------------------
// host helpers
// ------------------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int reserve(origin_ctx *ctx, size_t want) {
    if (want <= bytes) return ORIGIN_OK;
    if (p) {
      ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
      ORIGIN_HIP(hipFree(p));
      p = nullptr;
      bytes = 0;
    }
    const size_t n = want + want / 4 + 4096;
    ORIGIN_HIP(hipMalloc(&p, n));
    bytes = n;
    return ORIGIN_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  ~DevBuf() { release(); }
};

// pinned host memory that lives as long as the workspace (hipHostMalloc / hipHostFree cost
// hundreds of microseconds and the free waits for the device)
struct HostBuf {
  void *p = nullptr;
  size_t bytes = 0;
  unsigned flags = 0;
  int reserve(size_t want, unsigned fl) {
    if (want <= bytes && fl == flags) return ORIGIN_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    const size_t n = want + want / 2 + 256;
    ORIGIN_HIP(hipHostMalloc(&p, n, fl));
    bytes = n;
    flags = fl;
    return ORIGIN_OK;
  }
  ~HostBuf() {
    if (p) (void)hipHostFree(p);
  }
};

struct PcaWorkspace {
  DevBuf state, lists, test, desc, xp, g, cv, bu, part, cpart, info, U, C, small, fd;
  DevBuf fb[2];   // nuisance blocks of this / the previous iteration
  DevBuf bgsum;   // running background sums and the lists that update them
  DevBuf invert;  // spaxel -> (area, list position)
  DevBuf work;    // contiguous work cube of a strided run that flushes before its end
  HostBuf h_nnb, h_stage;
};

int gram_launch(origin_ctx *ctx, const double *d_Xp, const long *d_xp_off, const long *d_ld, int Nz,
                int ntiles, const int *d_ti, const int *d_tj, const int *d_ta, long g_total,
                double *d_G, const long *d_g_off, bool skip_reduce = false,
                const double **slab_out = nullptr, int *ksplit_out = nullptr,
                const long *d_n = nullptr) {
  const int ksplit = pca_gram_ksplit(ctx->num_cu, ntiles, Nz);
  void *scr = nullptr;
  int rc = origin_scratch(ctx, (size_t)ksplit * g_total * sizeof(double), &scr);
  if (rc) return rc;
  ProfScope ps(ctx, K_PCA_GRAM, 2);
  hipLaunchKernelGGL(gram_kernel, dim3(ntiles, ksplit), dim3(64), 0, ctx->stream, d_Xp, d_xp_off,
                     d_ld, d_ti, d_tj, d_ta, Nz, ksplit, (double *)scr, d_g_off, g_total, d_n);
  if (slab_out) *slab_out = (const double *)scr;
  if (ksplit_out) *ksplit_out = ksplit;
  // the small-matrix eigen-solver sums the slabs itself when every matrix of the launch is small
  if (!skip_reduce)
    hipLaunchKernelGGL(gram_reduce_kernel, dim3(ntiles), dim3(256), 0, ctx->stream,
                       (const double *)scr, g_total, ksplit, d_ld, d_ti, d_tj, d_ta, d_G, d_g_off,
                       d_n);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// sizes of one iteration's work list (build_work_list)
struct PcaWork {
  int nw = 0;                          // areas iterating = slots of the list
  long xp = 0, c = 0, g = 0, q = 0;    // elements of the nuisance blocks, vectors, Gram matrices, bases
  long cb = 0;                         // spaxels of the iterating areas
  int ldmax = 0, nsmax = 0, ntiles = 0;
};

// One run of the greedy PCA: the arguments of origin_pca_run_into, the device state carved from
// the context's workspace and the host's bookkeeping per area.
struct PcaRun {
  origin_ctx *ctx;
  PcaWorkspace &W;
  hipStream_t st;
  const float *d_X;
  float *d_F;
  int Nz;
  long S;
  int na;
  const int *d_spx;
  const long *h_spx_off;
  double noise_pop;
  int itermax;
  int *d_mapO2;
  int out_nx;  // > 0: d_F is a box inside a larger cube
  long out_py, out_pz;
  const int nsmax_all;      // spaxels of the largest area
  // Every area fits the register-resident selection (pca_select_fast_kernel).  Only that kernel
  // keeps the changes of the background set, so it also decides whether bmean_kernel updates
  // running sums (d_ssum, DF_SVALID) or gathers the background columns afresh.
  const bool sel_resident;

  long ntot;                // list entries of all areas
  const float *src;         // where the not-yet-deflated cube is read from
  float *d_work = nullptr;  // work cube of a strided run, once a mid-run flush has made it
  bool debug;               // ORIGIN_PCA_DEBUG: eigen-solver statistics per iteration
  // state
  double *d_thr;
  long *d_spx_off;
  int *d_active, *d_nbiter, *d_n, *d_nb, *d_nstop;
  unsigned *d_selcnt;  // blocks of all selections that have finished
  // lists
  int *d_nuis, *d_bg, *d_bg_pos, *d_npos[2];  // (nuisance positions: ping-pong)
  // Running sum of the background columns of each area (bmean_kernel): float64 [na][Nz], then
  // the signed list of columns that entered / left the set [ntot], their number per area [na]
  // and the membership flag of every list position [ntot].  In use when sel_resident.
  double *d_ssum;
  int *d_dlist, *d_ndiff;
  uint8_t *d_inb;
  // spaxel -> (area, list position) for the kernel that walks the cube in memory order
  // (deflate_dot_rows_kernel); the per-iteration area -> work-list slot table travels with the
  // descriptors
  int *d_area_of, *d_pos_of;
  double *d_test;
  double *d_U, *d_C;  // removed vectors U[area][z][PCA_CAP], coefficient rows C[PCA_CAP][list position]
  int *h_nnb;         // read-back [2*na] + [1] generation flag (mapped host memory)
  int *d_hostout;     // its device address
  int iters = 0;
  int gen = 1;  // selections launched so far + 1
  // host bookkeeping per area
  std::vector<int> counts;  // [2][na]: n and nb of the selection just read back
  std::vector<int> T;       // vectors held since the last flush
  std::vector<long> fb_off, fb_ld, fb_n;  // nuisance block as the previous iteration left it
  std::vector<char> s_valid;  // the running background sum is usable
  std::vector<char> flushed;  // written to d_F ahead of the final flush (tail hook): left alone then
  std::vector<long> D;        // this iteration's work list (descriptors)
  bool tail_fired = false;
  int tail_run = 0, tail_n0 = 0;  // iterations in a row with few areas; their nuisance count at the first

  int ns_of(int a) const { return (int)(h_spx_off[a + 1] - h_spx_off[a]); }
  int setup(const double *d_test0, const double *h_thr);
  int flush(bool final, bool only_done = false);
  int select();
  int active_areas(bool *full) const;
  int maybe_fire_tail_hook(int nw, bool full);
  int build_work_list(int nw, PcaWork &w, long *h_trace, int trace_cap);
  int enqueue_chain(const PcaWork &w);
  int report_debug(int nw, const double *d_info);
  void advance(const PcaWork &w);
};

// Workspace buffers that do not depend on the iteration, and the initial uploads.
int PcaRun::setup(const double *d_test0, const double *h_thr) {
  int rc;
  const size_t st_bytes = (size_t)na * (sizeof(double) + 4 * sizeof(int)) + sizeof(int) * 2 +
                          (size_t)(na + 1) * sizeof(long) + 64;
  if ((rc = W.state.reserve(ctx, st_bytes))) return rc;
  d_thr = (double *)W.state.p;
  d_spx_off = (long *)(d_thr + na);
  d_active = (int *)(d_spx_off + na + 1);
  d_nbiter = d_active + na;
  d_n = d_nbiter + na;  // n and nb are contiguous: one read-back
  d_nb = d_n + na;
  d_nstop = d_nb + na;
  d_selcnt = (unsigned *)(d_nstop + 1);  // (zeroed together with d_nstop)
  std::vector<int> ones(na, 1);
  ORIGIN_HIP(hipMemcpyAsync(d_thr, h_thr, (size_t)na * sizeof(double), hipMemcpyHostToDevice, st));
  ORIGIN_HIP(hipMemcpyAsync(d_spx_off, h_spx_off, (size_t)(na + 1) * sizeof(long),
                            hipMemcpyHostToDevice, st));
  ORIGIN_HIP(hipMemcpyAsync(d_active, ones.data(), (size_t)na * sizeof(int), hipMemcpyHostToDevice,
                            st));
  ORIGIN_HIP(hipMemsetAsync(d_nbiter, 0, (size_t)na * sizeof(int), st));
  ORIGIN_HIP(hipMemsetAsync(d_nstop, 0, 2 * sizeof(int), st));
  ORIGIN_HIP(hipStreamSynchronize(st));  // `ones` goes out of use
  if ((rc = W.lists.reserve(ctx, (size_t)5 * ntot * sizeof(int)))) return rc;
  d_nuis = (int *)W.lists.p;
  d_bg = d_nuis + ntot;
  d_bg_pos = d_bg + ntot;
  d_npos[0] = d_bg_pos + ntot;
  d_npos[1] = d_npos[0] + ntot;
  fb_off.assign(na, -1);
  fb_ld.assign(na, 0);
  fb_n.assign(na, 0);
  if ((rc = W.bgsum.reserve(ctx, (size_t)na * Nz * sizeof(double) +
                                     (size_t)(ntot + na) * sizeof(int) + (size_t)ntot)))
    return rc;
  d_ssum = (double *)W.bgsum.p;
  d_dlist = (int *)(d_ssum + (size_t)na * Nz);
  d_ndiff = d_dlist + ntot;
  d_inb = (uint8_t *)(d_ndiff + na);
  ORIGIN_HIP(hipMemsetAsync(d_inb, 0, (size_t)ntot, st));
  s_valid.assign(na, 0);
  if ((rc = W.invert.reserve(ctx, (size_t)2 * S * sizeof(int)))) return rc;
  d_area_of = (int *)W.invert.p;
  d_pos_of = d_area_of + S;
  ORIGIN_HIP(hipMemsetAsync(d_area_of, 0xFF, (size_t)S * sizeof(int), st));
  if (nsmax_all > 0)
    hipLaunchKernelGGL(invert_lists_kernel, dim3(cdiv(nsmax_all, 256), na), dim3(256), 0, st, d_spx,
                       d_spx_off, d_area_of, d_pos_of);
  if ((rc = W.test.reserve(ctx, (size_t)S * sizeof(double)))) return rc;
  d_test = (double *)W.test.p;
  ORIGIN_HIP(hipMemcpyAsync(d_test, d_test0, (size_t)S * sizeof(double), hipMemcpyDeviceToDevice,
                            st));
  if ((rc = W.U.reserve(ctx, (size_t)na * Nz * PCA_CAP * sizeof(double)))) return rc;
  if ((rc = W.C.reserve(ctx, (size_t)PCA_CAP * ntot * sizeof(double)))) return rc;
  d_U = (double *)W.U.p, d_C = (double *)W.C.p;
  T.assign(na, 0);
  flushed.assign(na, 0);
  counts.assign(2 * (size_t)na, 0);

  // read-back buffer: mapped, coherent host memory the selection kernel writes into directly
  if ((rc = W.h_nnb.reserve((size_t)(2 * na + 1) * sizeof(int),
                            hipHostMallocMapped | hipHostMallocCoherent)))
    return rc;
  h_nnb = (int *)W.h_nnb.p;
  memset(h_nnb, 0, (size_t)(2 * na + 1) * sizeof(int));
  ORIGIN_HIP(hipHostGetDevicePointer((void **)&d_hostout, h_nnb, 0));
  return ORIGIN_OK;
}

// F = X - U C for every area that holds vectors (every area at all when the output is a
// different buffer and has not been written yet); afterwards T = 0 and the cube is read
// from d_F.
// (Flushing the areas that have finished at once, on a second low-priority or CU-masked stream
// in the shadow of the iterations that go on, was built and measured: no gain -- 25.4-25.5 ms
// against 25.0-25.1; the one-block kernels of the chain slow down by what the flush overlaps.)
// (strided output: a flush in the middle of the run -- an area used up its PCA_CAP slots -- goes
// to a contiguous work cube the later passes read; only the final one writes d_F)
// only_done (tail hook): write just the areas that are not in the work list any more
// (counts[a] < 2) -- they have stopped iterating for good and the final flush leaves them alone;
// nothing else changes (src, T of the others).
int PcaRun::flush(bool final, bool only_done) {
  const bool strided = out_nx > 0;
  float *dst = d_F;
  if (strided && !final) {
    int rw = W.work.reserve(ctx, (size_t)Nz * S * sizeof(float));
    if (rw) return rw;
    if (!d_work && ntot < S)
      ORIGIN_HIP(hipMemcpyAsync(W.work.p, d_X, (size_t)Nz * S * sizeof(float),
                                hipMemcpyDeviceToDevice, st));
    d_work = (float *)W.work.p;
    dst = d_work;
  }
  const bool to_strided = strided && final;
  const bool all = src != dst;
  std::vector<int> areas;  // the areas written now
  for (int a = 0; a < na; ++a) {
    if (flushed[a] || (only_done && counts[a] >= 2)) continue;
    if ((all || T[a] > 0) && ns_of(a) > 0) areas.push_back(a);
  }
  const int nf = (int)areas.size();
  if (nf > 0) {
    std::vector<long> fd((size_t)4 * nf);  // descriptors [4][nf] = area, list0, ns, T
    int nsmax = 0;
    for (int k = 0; k < nf; ++k) {
      const int a = areas[k];
      fd[k] = a;
      fd[(size_t)nf + k] = h_spx_off[a];
      fd[(size_t)2 * nf + k] = ns_of(a);
      fd[(size_t)3 * nf + k] = T[a];
      nsmax = std::max(nsmax, ns_of(a));
    }
    int r;
    if ((r = W.fd.reserve(ctx, fd.size() * sizeof(long)))) return r;
    ORIGIN_HIP(hipMemcpyAsync(W.fd.p, fd.data(), fd.size() * sizeof(long), hipMemcpyHostToDevice,
                              st));
    ORIGIN_HIP(hipStreamSynchronize(st));
    ProfScope ps(ctx, K_PCA_FLUSH, 2);
    // (Round 3 measured two more forms of this pass at 3681 x 600 x 600 and dropped them: the
    // cube's memory order with one pass per area present in a wave, 3.39 ms; two / four spaxels
    // per lane so that one LDS read of U serves several products, 3.0 / 3.8 ms; this form 2.83.
    // Round 4: 16 / 24 / 8 channels per block instead of 32 (80 / 96 / 64 VGPRs, six / five / eight
    // waves per SIMD): 3.01 / 2.93 / 3.61 ms against 3.04 in the same session -- not occupancy.)
    const int nxb = cdiv(nsmax, 256), nzb = cdiv(Nz, FLUSH_ZB);
    const long ngroups = ((long)nxb * nzb + 7) / 8;  // groups of 8 (spaxel chunk, channel block)
    hipLaunchKernelGGL(flush_kernel, dim3((unsigned)(ngroups * nf * 8)), dim3(256), 0, st, src, dst,
                       Nz, S, d_spx, (const long *)W.fd.p, nf, d_U, d_C, ntot, nxb, nzb,
                       to_strided ? out_nx : 0, out_py, out_pz);
    ORIGIN_LAUNCH_CHECK();
  }
  if (only_done) {  // the areas that still iterate keep their vectors and go on reading src
    for (int a = 0; a < na; ++a)
      if (counts[a] < 2) flushed[a] = 1, T[a] = 0;
    return ORIGIN_OK;
  }
  for (int a = 0; a < na; ++a) T[a] = 0;
  std::fill(fb_off.begin(), fb_off.end(), -1L);  // (blocks refer to columns of U)
  std::fill(s_valid.begin(), s_valid.end(), (char)0);  // (sums refer to the cube read so far)
  src = dst;
  return ORIGIN_OK;
}

// The selection of this iteration, and its counts.  n / nb arrive in mapped host memory; wait for
// the generation flag of this selection (everything enqueued before it on the stream is complete
// by then).  Fall back to a stream synchronisation after 5 s (a faulted kernel never raises the
// flag).
int PcaRun::select() {
  {
    ProfScope ps(ctx, K_PCA_SELECT, 2);
    const SelectArgs sel{d_spx, d_spx_off, d_test, d_thr, noise_pop, itermax, d_active, d_nbiter,
                         d_nstop, d_mapO2, d_nuis, d_bg, d_npos[iters & 1], d_bg_pos, d_n, d_nb,
                         d_inb, d_dlist, d_ndiff, d_hostout, d_selcnt, gen};
    if (sel_resident)  // dynamic LDS: the spaxel index of every list entry
      hipLaunchKernelGGL(pca_select_fast_kernel, dim3(na), dim3(1024),
                         (size_t)nsmax_all * sizeof(int), st, sel);
    else
      hipLaunchKernelGGL(pca_select_kernel, dim3(na), dim3(1024), 0, st, sel);
  }
  ORIGIN_LAUNCH_CHECK();
  int *flag = h_nnb + 2 * na;
  const auto t_start = std::chrono::steady_clock::now();
  long polls = 0;
  while (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != gen) {
    __builtin_ia32_pause();
    if ((++polls & 0xfffff) == 0 &&
        std::chrono::steady_clock::now() - t_start > std::chrono::seconds(5)) {
      ORIGIN_HIP(hipStreamSynchronize(st));
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != gen) {
        origin_set_error("greedy PCA: the selection kernel did not report back");
        return ORIGIN_E_HIP;
      }
    }
  }
  ++gen;
  memcpy(counts.data(), h_nnb, 2 * (size_t)na * sizeof(int));
  return ORIGIN_OK;
}

// areas that iterate (n >= 2); *full: one of them has used up its PCA_CAP vector slots
int PcaRun::active_areas(bool *full) const {
  int nw = 0;
  *full = false;
  for (int a = 0; a < na; ++a)
    if (counts[a] >= 2) {
      ++nw;
      *full = *full || T[a] >= PCA_CAP;
    }
  return nw;
}

// Tail hook: once, when few areas are left.  The areas that are done are written to d_F now
// (the pass they would have had at the end), then the caller learns which areas go on -- it may
// start the next stage on everything that does not depend on them (origin_glr_run_rows on the
// side stream).  Needs no work cube between the input and d_F.
// It fires only when the few areas left look like stragglers: three iterations in a row with
// at most pca_tail_max areas, whose nuisance count has not fallen below 0.6 of what it was at
// the first of them.  (Bench fields, (areas, nuisance spaxels) per iteration: 600^2 ... (3,50)
// (2,31) (2,28) (1,24) (1,21) (1,20) and 44 more down to (1,12); 200^2 ... (2,74) (2,58) (1,52)
// (1,51) and 34 more; 300^2 ... (7,93) (1,23) (1,13) (1,3), end -- there the run is over
// before anything started beside it could pay: 17.5 ms per step with the hook at the first
// iteration with one area, 16.3 without it.)
int PcaRun::maybe_fire_tail_hook(int nw, bool full) {
  int n_active_sum = 0;
  for (int a = 0; a < na; ++a)
    if (counts[a] >= 2) n_active_sum += counts[a];
  if (nw <= ctx->pca_tail_max && iters >= 1) {
    if (tail_run++ == 0) tail_n0 = n_active_sum;
  } else {
    tail_run = 0;
  }
  if (!ctx->pca_tail_hook || tail_fired || tail_run < 3 ||
      10 * (long)n_active_sum < 6 * (long)tail_n0 || d_work || full)
    return ORIGIN_OK;
  tail_fired = true;
  int rc = flush(true, true);
  if (rc) return rc;
  std::vector<int> act;
  for (int a = 0; a < na; ++a)
    if (counts[a] >= 2) act.push_back(a);
  ctx->pca_tail_hook(ctx->pca_tail_user, (int)act.size(), act.data());
  return ORIGIN_OK;
}

// The work list of this iteration: one slot per area with n >= 2 in the selection just read back,
// so no kernel of the chain meets a slot that has finished.  Fills D, the Gram tile lists and kidx
// and sends them to the device.
int PcaRun::build_work_list(int nw, PcaWork &w, long *h_trace, int trace_cap) {
  w = PcaWork();
  w.nw = nw;
  D.assign((size_t)DF_COUNT * nw, 0);
  std::vector<int> ti, tj, ta;  // Gram tiles (i, j, slot)
  std::vector<int> kidx(na, -1);  // area -> slot of this iteration (-1: not iterating)
  int k = 0;
  long nsum = 0;
  for (int a = 0; a < na; ++a) {
    const int n = counts[a];
    if (n < 2) continue;
    const int ld = (n + 15) / 16 * 16;
    const int ns = ns_of(a);
    D[(size_t)DF_AREA * nw + k] = a;
    D[(size_t)DF_LIST0 * nw + k] = h_spx_off[a];
    D[(size_t)DF_N * nw + k] = n;
    D[(size_t)DF_NB * nw + k] = counts[na + a];
    D[(size_t)DF_LD * nw + k] = ld;
    D[(size_t)DF_XP * nw + k] = w.xp;
    D[(size_t)DF_C * nw + k] = w.c;
    D[(size_t)DF_G * nw + k] = w.g;
    D[(size_t)DF_Q * nw + k] = w.q;
    D[(size_t)DF_NS * nw + k] = ns;
    D[(size_t)DF_CBASE * nw + k] = w.cb;
    D[(size_t)DF_T * nw + k] = T[a];
    // previous nuisance block of the area, usable while at least one vector is held
    const bool have = fb_off[a] >= 0 && T[a] >= 1;
    D[(size_t)DF_FBOLD * nw + k] = have ? fb_off[a] : -1;
    D[(size_t)DF_LDOLD * nw + k] = fb_ld[a];
    D[(size_t)DF_NOLD * nw + k] = fb_n[a];
    D[(size_t)DF_SVALID * nw + k] = sel_resident && s_valid[a];
    s_valid[a] = sel_resident;  // this iteration's bmean_kernel leaves the sum behind
    w.xp += (long)Nz * ld;
    w.c += ld;
    w.g += (long)ld * ld;
    w.q += (long)EIG_QROWS * ld;
    w.cb += ns;
    w.ldmax = std::max(w.ldmax, ld);
    w.nsmax = std::max(w.nsmax, ns);
    nsum += n;
    const int Tt = (ld + 31) / 32;
    for (int i = 0; i < Tt; ++i)
      for (int j = i; j < Tt; ++j) ti.push_back(i), tj.push_back(j), ta.push_back(k);
    kidx[a] = k;
    ++k;
  }
  const int ntiles = w.ntiles = (int)ti.size();
  if (h_trace && iters < trace_cap) {
    h_trace[2 * iters] = nw;
    h_trace[2 * iters + 1] = nsum;
  }
  // descriptors, tile lists and kidx go up in ONE asynchronous copy from pinned staging (free
  // again: the selection that has just reported back is behind every earlier upload)
  const size_t dbytes = D.size() * sizeof(long), tbytes = (size_t)3 * ntiles * sizeof(int);
  const size_t kbytes = (size_t)na * sizeof(int);
  int rc;
  if ((rc = W.desc.reserve(ctx, dbytes + tbytes + kbytes))) return rc;
  if (dbytes + tbytes + kbytes > W.h_stage.bytes &&
      (rc = W.h_stage.reserve((dbytes + tbytes + kbytes) * 2, hipHostMallocDefault)))
    return rc;
  char *h_stage = (char *)W.h_stage.p;
  memcpy(h_stage, D.data(), dbytes);
  int *ht = (int *)(h_stage + dbytes);
  memcpy(ht, ti.data(), (size_t)ntiles * sizeof(int));
  memcpy(ht + ntiles, tj.data(), (size_t)ntiles * sizeof(int));
  memcpy(ht + 2 * (size_t)ntiles, ta.data(), (size_t)ntiles * sizeof(int));
  memcpy(ht + 3 * (size_t)ntiles, kidx.data(), kbytes);
  ORIGIN_HIP(hipMemcpyAsync(W.desc.p, h_stage, dbytes + tbytes + kbytes, hipMemcpyHostToDevice, st));
  return ORIGIN_OK;
}

// Enqueues one iteration behind the upload of its work list: background mean, nuisance block,
// projection, Gram matrix, eigenvector, u, deflation of the iterating areas.
int PcaRun::enqueue_chain(const PcaWork &w) {
  int rc;
  const int nw = w.nw, ntiles = w.ntiles;
  const size_t dbytes = D.size() * sizeof(long);
  const long *dD = (const long *)W.desc.p;
  const int *d_ti = (const int *)((char *)W.desc.p + dbytes), *d_tj = d_ti + ntiles,
            *d_ta = d_tj + ntiles, *d_kidx = d_ta + ntiles;
  const long *dLD = dD + (size_t)DF_LD * nw, *dXP = dD + (size_t)DF_XP * nw;
  const long *dG = dD + (size_t)DF_G * nw, *dQ = dD + (size_t)DF_Q * nw;
  const long *dN = dD + (size_t)DF_N * nw, *dC = dD + (size_t)DF_C * nw;

  DevBuf &fb_new = W.fb[iters & 1], &fb_old = W.fb[(iters & 1) ^ 1];
  if ((rc = W.xp.reserve(ctx, (size_t)w.xp * sizeof(double)))) return rc;
  if ((rc = fb_new.reserve(ctx, (size_t)w.xp * sizeof(double)))) return rc;
  if ((rc = W.g.reserve(ctx, (size_t)w.g * sizeof(double)))) return rc;
  if ((rc = W.cv.reserve(ctx, (size_t)w.c * sizeof(double)))) return rc;
  if ((rc = W.bu.reserve(ctx, (size_t)2 * nw * Nz * sizeof(double)))) return rc;
  if ((rc = W.small.reserve(ctx, ((size_t)2 * nw * PCA_CAP +
                                  (size_t)nw * UW_SLICES * (PCA_CAP + 1)) * sizeof(double))))
    return rc;
  double *d_Xp = (double *)W.xp.p, *d_Fb = (double *)fb_new.p, *d_G = (double *)W.g.p;
  double *d_v = (double *)W.cv.p;
  double *d_b = (double *)W.bu.p, *d_u = d_b + (size_t)nw * Nz;
  double *d_cbar = (double *)W.small.p, *d_wq = d_cbar + (size_t)nw * PCA_CAP;
  double *d_uwpart = d_wq + (size_t)nw * PCA_CAP;

  {
    ProfScope ps(ctx, K_PCA_BMEAN, 2);
    hipLaunchKernelGGL(cbar_kernel, dim3(nw), dim3(1024), 0, st, d_C, ntot, d_bg_pos, dD, nw,
                       d_cbar);
    hipLaunchKernelGGL(bmean_kernel, dim3(cdiv(Nz, 4), nw), dim3(64, 4), 0, st, src, Nz, S, d_bg,
                       dD, nw, d_U, d_cbar, d_b, d_dlist, d_ndiff, sel_resident ? d_ssum : nullptr);
  }
  // z slices of the gather: enough blocks to fill the chip even when few areas iterate
  int nzb = (int)(((long)ctx->num_cu * 2 + (long)cdiv(w.ldmax, 64) * nw - 1) /
                  ((long)cdiv(w.ldmax, 64) * nw));
  nzb = std::max(1, std::min(nzb, 16));
  const int gzper = (cdiv(Nz, nzb) + 15) / 16 * 16;
  nzb = cdiv(Nz, gzper);
  if ((rc = W.cpart.reserve(ctx, (size_t)nzb * w.c * sizeof(double)))) return rc;
  double *d_cpart = (double *)W.cpart.p;
  {
    ProfScope ps(ctx, K_PCA_GATHER, 2);
    hipLaunchKernelGGL(gather_xp_kernel, dim3(cdiv(w.ldmax, 64), nw, nzb), dim3(64, 16), 0, st, src,
                       Nz, S, d_nuis, d_npos[iters & 1], d_npos[(iters & 1) ^ 1], dD, nw, d_b, d_U,
                       d_C, ntot, (const double *)fb_old.p, d_Fb, d_cpart, w.c, gzper);
  }
  {
    ProfScope ps(ctx, K_PCA_PROJECT, 2);
    hipLaunchKernelGGL(project_xp_kernel, dim3(cdiv(Nz, 16), nw), dim3(256), 0, st, d_b, Nz, dD, nw,
                       d_Fb, d_Xp, d_cpart, w.c, nzb);
  }
  ORIGIN_LAUNCH_CHECK();
  const bool all_small = w.ldmax <= LANCZOS_M;  // (ld is n rounded up to 16: n <= 48)
  const double *d_slab = nullptr;
  int gram_ksplit = 0;
  if ((rc = gram_launch(ctx, d_Xp, dXP, dLD, Nz, ntiles, d_ti, d_tj, d_ta, w.g, d_G, dG, all_small,
                        &d_slab, &gram_ksplit, dN)))
    return rc;
  if ((rc = W.part.reserve(ctx, (size_t)w.q * sizeof(double)))) return rc;
  double *d_info = nullptr;
  if (debug) {
    if ((rc = W.info.reserve(ctx, (size_t)13 * nw * sizeof(double)))) return rc;
    d_info = (double *)W.info.p;
  }
  {
    ProfScope ps(ctx, K_PCA_EIG, 2);
    const EigBatch batch{nw, d_G, dG, dLD, dN, (double *)W.part.p, dQ, d_v, dC, d_info,
                         debug ? d_info + (size_t)3 * nw : nullptr};
    const EigSlabs slabs = all_small ? EigSlabs{d_slab, w.g, gram_ksplit} : EigSlabs{};
    if ((rc = origin_pca_eig_launch(ctx, batch, w.ldmax, slabs)))
      return rc;
  }
  if (debug && (rc = report_debug(nw, d_info))) return rc;
  {
    ProfScope ps(ctx, K_PCA_UVEC, 2);
    hipLaunchKernelGGL(xv_kernel, dim3(cdiv(Nz, 4), nw), dim3(64, 4), 0, st, d_Xp, dD, nw, Nz, d_v,
                       d_u);
    hipLaunchKernelGGL(uw_partial_kernel, dim3(UW_SLICES, nw), dim3(256), 0, st, d_u, Nz, dD, nw,
                       d_U, d_uwpart);
    hipLaunchKernelGGL(normalize_kernel, dim3(nw), dim3(1024), 0, st, d_u, Nz, dD, nw, d_U,
                       d_uwpart, d_wq);
  }
  ORIGIN_LAUNCH_CHECK();
  // ---- deflation (coefficient form): one read pass over the iterating areas
  const long blocks = (long)cdiv(w.nsmax, 256) * nw;
  int nzs = (int)(((long)ctx->num_cu * 8 + blocks - 1) / blocks);
  nzs = std::max(1, std::min(nzs, 32));
  nzs = std::min(nzs, Nz);
  const int zper = cdiv(Nz, nzs);
  nzs = cdiv(Nz, zper);
  void *scr = nullptr;
  if ((rc = origin_scratch(ctx, (size_t)nzs * w.cb * sizeof(double), &scr))) return rc;
  double *cpart = (double *)scr;
  {
    ProfScope ps(ctx, K_PCA_DEFLATE_DOT, 2);
    if (2 * w.cb >= S)  // the iterating areas cover at least half of the field
      hipLaunchKernelGGL(deflate_dot_rows_kernel, dim3(cdiv(S, 256), nzs), dim3(256), 0, st, src, Nz,
                         S, d_area_of, d_pos_of, d_kidx, dD, nw, d_u, zper, cpart, w.cb);
    else
      hipLaunchKernelGGL(deflate_dot_kernel, dim3(cdiv(w.nsmax, 256), nzs, nw), dim3(256), 0, st,
                         src, Nz, S, d_spx, dD, nw, d_u, zper, cpart, w.cb);
  }
  {
    ProfScope ps(ctx, K_PCA_DEFLATE_UPDATE, 2);
    hipLaunchKernelGGL(deflate_finish_kernel, dim3(cdiv(w.nsmax, 256), nw), dim3(256), 0, st, d_spx,
                       dD, nw, nzs, Nz, w.cb, cpart, d_wq, d_C, ntot, d_test);
  }
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// ORIGIN_PCA_DEBUG: reads the eigen-solver's statistics of this iteration back (a host
// synchronisation) and prints them; ORIGIN_PCA_DEBUG_EIG adds a line per matrix.
int PcaRun::report_debug(int nw, const double *d_info) {
  std::vector<double> info((size_t)13 * nw, 0.0);
  ORIGIN_HIP(hipMemcpyAsync(info.data(), d_info, info.size() * sizeof(double),
                            hipMemcpyDeviceToHost, st));
  ORIGIN_HIP(hipStreamSynchronize(st));
  if (getenv("ORIGIN_PCA_DEBUG_EIG")) {  // per matrix: n:steps:restarts:us
    fprintf(stderr, "[pca-eig] iter %d:", iters);
    for (int w = 0; w < nw; ++w)
      fprintf(stderr, " %d:%.0f:%.0f:%.0f", (int)D[(size_t)DF_N * nw + w], info[3 * nw + 2 * w],
              info[3 * w + 2], info[3 * nw + 2 * w + 1]);
    fprintf(stderr, "\n");
    // phases (us) of the slowest plain-Lanczos block: setup, mat-vec, vector part, checks, final
    int ws_ = -1;
    for (int w = 0; w < nw; ++w)
      if (info[3 * nw + 2 * w] > 0 && (ws_ < 0 || info[3 * nw + 2 * w + 1] > info[3 * nw + 2 * ws_ + 1]))
        ws_ = w;
    if (ws_ >= 0) {
      const double *t = &info[5 * (size_t)nw + 8 * (size_t)ws_];
      fprintf(stderr, "[pca-eig]   slowest n %d steps %.0f: setup %.1f matvec %.1f vector %.1f checks %.1f "
              "(prep %.1f rounds %.1f vector %.1f) final %.1f us\n",
              (int)D[(size_t)DF_N * nw + ws_], info[3 * nw + 2 * ws_], t[0] * 0.01, t[1] * 0.01,
              t[2] * 0.01, t[3] * 0.01, t[5] * 0.01, t[6] * 0.01, t[7] * 0.01, t[4] * 0.01);
    }
  }
  double rmax = 0, rsum = 0, resmax = 0;
  int nmax = 0;
  for (int w = 0; w < nw; ++w) {
    rmax = std::max(rmax, info[3 * w + 2]);
    rsum += info[3 * w + 2];
    resmax = std::max(resmax, info[3 * w + 1] / std::max(info[3 * w], 1e-300));
    nmax = std::max(nmax, (int)D[(size_t)DF_N * nw + w]);
  }
  fprintf(stderr, "[pca] iter %3d areas %3d nmax %4d restarts max %2.0f mean %.2f relres max %.1e\n",
          iters, nw, nmax, rmax, rsum / nw, resmax);
  return ORIGIN_OK;
}

// every area of the work list now holds one more vector; its block becomes the next gather's source
void PcaRun::advance(const PcaWork &w) {
  for (int k = 0; k < w.nw; ++k) {
    const int a = (int)D[(size_t)DF_AREA * w.nw + k];
    T[a] += 1;
    fb_off[a] = D[(size_t)DF_XP * w.nw + k];
    fb_ld[a] = D[(size_t)DF_LD * w.nw + k];
    fb_n[a] = counts[a];
  }
  ++iters;
}

}  // namespace

extern "C" {

// Stand-alone Gram product (used by tests): nmat matrices, offsets/ld as int64 arrays.
int origin_pca_gram(origin_ctx *ctx, const double *d_Xp, const long *d_xp_off, const long *d_ld,
                    int Nz, int ntiles, const int *d_tile_i, const int *d_tile_j,
                    const int *d_tile_a, long g_total, double *d_G, const long *d_g_off) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_Xp && d_xp_off && d_ld && d_tile_i && d_tile_j && d_tile_a && d_G &&
                       d_g_off && Nz > 0 && ntiles > 0 && g_total > 0,
                   "bad arguments");
  return gram_launch(ctx, d_Xp, d_xp_off, d_ld, Nz, ntiles, d_tile_i, d_tile_j, d_tile_a, g_total,
                     d_G, d_g_off);
}

int origin_pca_set_tail_hook(origin_ctx *ctx, void (*hook)(void *, int, const int *), void *user,
                             int max_active) {
  ORIGIN_CHECK_ARG(ctx && max_active >= 0, "bad argument");
  ctx->pca_tail_hook = hook;
  ctx->pca_tail_user = user;
  ctx->pca_tail_max = max_active;
  return ORIGIN_OK;
}

// The whole greedy PCA of `na` areas; d_F receives cube_faint.  out_nx > 0: d_F is the first
// element of an (Nz, S / out_nx, out_nx) box inside a larger cube with row pitch out_py and plane
// pitch out_pz (elements) -- the interior of a halo-extended tile, so that the tiled path needs no
// copy between the PCA and the halo exchange; d_X must then be a different, contiguous cube.
int origin_pca_run_into(origin_ctx *ctx, const float *d_X, float *d_F, int Nz, long S, int na,
                        const int *d_spx, const long *h_spx_off, const double *d_test0,
                        const double *h_thr, double noise_pop, int itermax, int *d_mapO2,
                        int *h_nstop, int *h_iters, long *h_trace, int trace_cap, int out_nx,
                        long out_py, long out_pz) {
  ORIGIN_USE(ctx);
  const bool strided = out_nx > 0;
  ORIGIN_CHECK_ARG(!strided || (d_X && d_X != d_F && S % out_nx == 0 && out_py >= out_nx &&
                                out_pz >= (S / out_nx) * out_py),
                   "strided output needs a separate contiguous input and consistent pitches");
  ORIGIN_CHECK_ARG(d_F && d_spx && h_spx_off && d_test0 && h_thr && d_mapO2 && h_nstop &&
                       Nz > 0 && S > 0 && na > 0,
                   "bad arguments");
  ORIGIN_CHECK_ARG(noise_pop > 0 && itermax >= 0, "bad Noise_population / itermax");
  ProfScope ps_total(ctx, K_PCA_TOTAL, 1);
  if (!d_X) d_X = d_F;
  const long ntot = h_spx_off[na];
  ORIGIN_CHECK_ARG(ntot >= 0 && ntot <= S, "area lists longer than the field");
  hipStream_t st = ctx->stream;
  if (h_iters) *h_iters = 0;
  *h_nstop = 0;
  ORIGIN_HIP(hipMemsetAsync(d_mapO2, 0, (size_t)S * sizeof(int), st));
  if (d_X != d_F && ntot < S) {  // spaxels outside every area are simply copied
    if (strided) {
      int rcb = origin_copy_box(ctx, 2, d_F, out_py, out_pz, d_X, out_nx, S, Nz, (int)(S / out_nx),
                                out_nx, (int)sizeof(float));
      if (rcb) return rcb;
    } else {
      ORIGIN_HIP(hipMemcpyAsync(d_F, d_X, (size_t)Nz * S * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
  }
  if (ntot == 0) return ORIGIN_OK;

  // device buffers are kept in the context between calls (hipMalloc/hipFree of a few hundred
  // MB per call cost milliseconds)
  if (!ctx->pca_ws) {
    ctx->pca_ws = new PcaWorkspace();
    ctx->pca_ws_free = [](void *p) { delete (PcaWorkspace *)p; };
  }
  int nsmax_all = 0;
  for (int a = 0; a < na; ++a)
    nsmax_all = std::max(nsmax_all, (int)(h_spx_off[a + 1] - h_spx_off[a]));
  PcaRun R{ctx, *(PcaWorkspace *)ctx->pca_ws, st, d_X, d_F, Nz, S, na, d_spx, h_spx_off,
           noise_pop, itermax, d_mapO2, out_nx, out_py, out_pz, nsmax_all,
           nsmax_all <= 1024 * SEL_EPT};
  R.ntot = ntot;
  R.src = d_X;
  R.debug = getenv("ORIGIN_PCA_DEBUG") != nullptr;
  int rc;
  if ((rc = R.setup(d_test0, h_thr))) return rc;

  // Per iteration: selection, hand-shake, exact work list, chain.  (The host running one selection
  // ahead of the device was built and measured at 3681 x 600 x 600, 57 iterations: 26.0-26.3
  // against 25.7-25.9 ms for this order -- the loop is bound by the device, the hand-shake hides
  // behind the chain either way.  The 120 us gaps per tail iteration in rocprofv3 timelines are
  // per-dispatch profiler overhead: the unprofiled tail runs at its kernels' busy time, ~125 us
  // per iteration.)
  // host-side phase times of the loop (ORIGIN_PCA_TIMING): selection + building the list, enqueueing
  double t_build = 0, t_enq = 0;
  using Clock = std::chrono::steady_clock;
  for (;;) {
    const auto tp0 = Clock::now();
    if ((rc = R.select())) return rc;
    bool full;
    const int nw = R.active_areas(&full);
    if (nw == 0) break;
    if ((rc = R.maybe_fire_tail_hook(nw, full))) return rc;
    if (full && (rc = R.flush(false))) return rc;  // an area used up its PCA_CAP slots
    PcaWork work;
    if ((rc = R.build_work_list(nw, work, h_trace, trace_cap))) return rc;
    const auto tp1 = Clock::now();
    if ((rc = R.enqueue_chain(work))) return rc;
    R.advance(work);
    t_build += std::chrono::duration<double>(tp1 - tp0).count();
    t_enq += std::chrono::duration<double>(Clock::now() - tp1).count();
  }
  if (getenv("ORIGIN_PCA_TIMING"))
    fprintf(stderr, "[pca] host loop: %d iterations, build %.2f ms, enqueue %.2f ms\n", R.iters,
            1e3 * t_build, 1e3 * t_enq);
  if ((rc = R.flush(true))) return rc;
  ORIGIN_HIP(hipMemcpyAsync(R.h_nnb, R.d_nstop, sizeof(int), hipMemcpyDeviceToHost, st));
  ORIGIN_HIP(hipStreamSynchronize(st));
  *h_nstop = R.h_nnb[0];
  if (h_iters) *h_iters = R.iters;
  return ORIGIN_OK;
}

int origin_pca_run(origin_ctx *ctx, const float *d_X, float *d_F, int Nz, long S, int na,
                   const int *d_spx, const long *h_spx_off, const double *d_test0,
                   const double *h_thr, double noise_pop, int itermax, int *d_mapO2, int *h_nstop,
                   int *h_iters, long *h_trace, int trace_cap) {
  return origin_pca_run_into(ctx, d_X, d_F, Nz, S, na, d_spx, h_spx_off, d_test0, h_thr, noise_pop,
                             itermax, d_mapO2, h_nstop, h_iters, h_trace, trace_cap, 0, 0, 0);
}

}  // extern "C"
