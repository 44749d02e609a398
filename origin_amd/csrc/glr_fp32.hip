// GLR matched filter: the fp32 FMA kernels (glr.hip has the algebra).  They serve
// origin_glr_plan_set_precision(plan, 0), the shapes the matrix-core kernels do not take (PSF sizes
// outside 5 .. 41, profiles wider than 32 channels, more than 26 profiles, fields smaller than the
// PSF) and the norm cube of a weighted plan.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "glr_plan.h"

namespace {

// ------------------------------------------------------------------------------------
// spatial stage: out[z] (+)= corr2(A[z] * B, taps[z]),  zero padded, 'same'
// block (64,4): tile 64 x 16 outputs, each thread 4 rows (ty, ty+4, ty+8, ty+12)
// ------------------------------------------------------------------------------------
constexpr int TX = 64, TY = 16;

__global__ __launch_bounds__(256) void spatial_kernel(const float *__restrict__ A,
                                                      const float *__restrict__ B,
                                                      const float *__restrict__ taps, int Ny,
                                                      int Nx, int P, int accumulate,
                                                      float *__restrict__ out) {
  extern __shared__ float tile[];  // [(TY+P-1)][pitch]
  const int c = P / 2;
  const int pitch = TX + P - 1;
  const int rows = TY + P - 1;
  const int z = blockIdx.z;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const long S = (long)Ny * Nx;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  for (int i = tid; i < rows * pitch; i += 256) {
    const int ry = i / pitch, rx = i - ry * pitch;
    const int y = y0 + ry - c, x = x0 + rx - c;
    float v = 0.0f;
    if (y >= 0 && y < Ny && x >= 0 && x < Nx) {
      const long p = (long)y * Nx + x;
      v = A ? A[(long)z * S + p] : 1.0f;
      if (B) v *= B[p];
    }
    tile[i] = v;
  }
  __syncthreads();
  const float *kz = taps + (long)z * P * P;  // uniform -> scalar loads
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const int tx = threadIdx.x, ty = threadIdx.y;
  for (int dy = 0; dy < P; ++dy) {
    const float *r0 = tile + (ty + dy) * pitch + tx;
    for (int dx = 0; dx < P; ++dx) {
      const float kv = kz[dy * P + dx];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = fmaf(kv, r0[(4 * r) * pitch + dx], acc[r]);
    }
  }
  const int x = x0 + tx;
  if (x < Nx) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = y0 + ty + 4 * r;
      if (y < Ny) {
        const long o = (long)z * S + (long)y * Nx + x;
        out[o] = accumulate ? out[o] + acc[r] : acc[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// spatial stage, register-tiled: block 256 threads = 16 x 16, every thread owns a 4 x 4
// patch of outputs (tile 64 x 64).  For each of the 4+P-1 input rows of its patch a thread
// reads the row segment it needs once from LDS (ds_read_b128, conflict free because the
// pitch is a multiple of 16 floats) and feeds up to 4 output rows x P taps x 4 columns of
// FMAs from registers; the taps are wave-uniform and come from scalar loads.
// ------------------------------------------------------------------------------------
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int P, bool VEC, bool HAS_B>
__global__ __launch_bounds__(256) void spatial4x4_kernel(const float *__restrict__ A,
                                                         const float *__restrict__ B,
                                                         const float *__restrict__ taps, int Nz,
                                                         int Ny, int Nx, int zper, int accumulate,
                                                         float *__restrict__ out) {
  constexpr int H = P - 1;
  constexpr int W = 64 + H;                  // tile width in floats (multiple of 4: P odd)
  constexpr int W4 = (W + 3) / 4;            // float4 per tile row
  constexpr int PITCH = (W + 15) / 16 * 16;  // multiple of 16 floats: conflict-free b128 reads
  constexpr int ROWS = 64 + H;
  constexpr int NV = (4 + H + 3) / 4;        // float4 per row segment a thread consumes
  constexpr int RPT = 256 / W4;               // tile rows staged per pass by the block
  constexpr int NQ = (ROWS + RPT - 1) / RPT;  // staged float4 per thread
  static_assert(60 + 4 * NV <= PITCH && 4 * W4 <= PITCH, "row segment exceeds the LDS pitch");
  __shared__ __attribute__((aligned(16))) float tile[ROWS * PITCH];
  constexpr int c = P / 2;
  const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
  const long S = (long)Ny * Nx;
  const int tid = threadIdx.x;
  const int z0 = blockIdx.z * zper, z1 = min(Nz, z0 + zper);

  // Register staging of the next plane's tile (issue early, write to LDS late).  Thread
  // (sr, sc4) stages the float4 column sc4 of tile rows sr, sr+RPT, sr+2 RPT, ...
  const int sr = tid / W4, sc4 = tid - sr * W4;
  const bool stager = sr < RPT;
  const int sx = x0 - c + 4 * sc4;  // first field column of the staged float4
  // VEC: Nx % 4 == 0 and sx % 4 == 0, so a float4 is either fully inside or fully outside
  const bool xin = sx >= 0 && sx + 3 < Nx;
  float4 stage[NQ];
  auto load_tile = [&](int z) {
    const float *Az = A + (long)z * S;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int ry = sr + RPT * j;
      const int y = y0 - c + ry;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (stager && ry < ROWS && y >= 0 && y < Ny) {
        const long p = (long)y * Nx + sx;
        if constexpr (VEC) {
          if (xin) {
            v = *reinterpret_cast<const float4 *>(Az + p);
            if constexpr (HAS_B) {
              const float4 w = *reinterpret_cast<const float4 *>(B + p);
              v.x *= w.x, v.y *= w.y, v.z *= w.z, v.w *= w.w;
            }
          }
        } else {
          float e[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int xx = sx + t;
            float u = 0.f;
            if (xx >= 0 && xx < Nx) {
              u = Az[p + t];
              if constexpr (HAS_B) u *= B[p + t];
            }
            e[t] = u;
          }
          v = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
      stage[j] = v;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      const int ry = sr + RPT * j;
      if (stager && ry < ROWS)
        *reinterpret_cast<float4 *>(tile + ry * PITCH + 4 * sc4) = stage[j];
    }
  };

  const int tx = tid & 15, ty = tid >> 4;
  load_tile(z0);
  for (int z = z0; z < z1; ++z) {
    __syncthreads();  // every wave is done reading the previous tile
    store_tile();
    __syncthreads();
    if (z + 1 < z1) load_tile(z + 1);  // in flight while this plane is computed
    const float *kz = taps + (long)z * P * P;  // uniform -> scalar loads
    // Full-rate fp32 on gfx950 needs v_pk_fma_f32, whose 64-bit operands are even-aligned
    // register pairs: keep the row segment twice, as pairs starting at even (rowE) and at
    // odd (rowO) columns, so that every (column, column+1) pair is a ready-made operand.
    f32x2 acc[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a][0] = acc[a][1] = (f32x2){0.f, 0.f};
#pragma unroll 1
    for (int i = 0; i < 4 + H; ++i) {
      const float *rbase = tile + (4 * ty + i) * PITCH + 4 * tx;
      const float4 *rp = reinterpret_cast<const float4 *>(rbase);
      f32x2 rowE[2 * NV], rowO[2 * NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const float4 v = rp[q];
        rowE[2 * q] = (f32x2){v.x, v.y};
        rowE[2 * q + 1] = (f32x2){v.z, v.w};
      }
      // odd-aligned pairs (2q+1, 2q+2) are assembled from neighbouring even pairs in
      // registers (one v_pk_mov_b32 each): reading them from LDS with ds_read2_b32 costs
      // 8-way bank conflicts and made the LDS, not the VALU, the bottleneck
#pragma unroll
      for (int q = 0; q + 1 < 2 * NV; ++q)
        rowO[q] = __builtin_shufflevector(rowE[q], rowE[q + 1], 1, 2);
      rowO[2 * NV - 1] = (f32x2){rowE[2 * NV - 1].y, 0.0f};
      // output rows are processed in pairs so that four independent accumulators are in
      // flight (a packed FMA then never waits for the previous one on the same register)
      auto single = [&](int ry) {
        const float *kr = kz + (i - ry) * P;
#pragma unroll
        for (int dx = 0; dx < P; ++dx) {
          const float kv = kr[dx];
          const f32x2 k2 = (f32x2){kv, kv};
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int j = 2 * h + dx;  // first column of the pair
            const f32x2 in = (j & 1) ? rowO[j >> 1] : rowE[j >> 1];
            acc[ry][h] = __builtin_elementwise_fma(k2, in, acc[ry][h]);
          }
        }
      };
#pragma unroll
      for (int rp = 0; rp < 4; rp += 2) {
        const int dya = i - rp, dyb = i - rp - 1;
        const bool va = dya >= 0 && dya < P, vb = dyb >= 0 && dyb < P;  // wave-uniform
        if (va && vb) {
          const float *ka = kz + dya * P, *kb = kz + dyb * P;
#pragma unroll
          for (int dx = 0; dx < P; ++dx) {
            const f32x2 a2 = (f32x2){ka[dx], ka[dx]}, b2 = (f32x2){kb[dx], kb[dx]};
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int j = 2 * h + dx;
              const f32x2 in = (j & 1) ? rowO[j >> 1] : rowE[j >> 1];
              acc[rp][h] = __builtin_elementwise_fma(a2, in, acc[rp][h]);
              acc[rp + 1][h] = __builtin_elementwise_fma(b2, in, acc[rp + 1][h]);
            }
          }
        } else {
          if (va) single(rp);
          if (vb) single(rp + 1);
        }
      }
    }
    const int xo = x0 + 4 * tx;
#pragma unroll
    for (int ry = 0; ry < 4; ++ry) {
      const int y = y0 + 4 * ty + ry;
      if (y >= Ny) continue;
      float *o = out + (long)z * S + (long)y * Nx + xo;
      if (VEC && xo + 3 < Nx) {
        float4 v = make_float4(acc[ry][0].x, acc[ry][0].y, acc[ry][1].x, acc[ry][1].y);
        if (accumulate) {
          const float4 old = *reinterpret_cast<float4 *>(o);
          v.x += old.x, v.y += old.y, v.z += old.z, v.w += old.w;
        }
        *reinterpret_cast<float4 *>(o) = v;
      } else {
        const float r4[4] = {acc[ry][0].x, acc[ry][0].y, acc[ry][1].x, acc[ry][1].y};
#pragma unroll
        for (int rx = 0; rx < 4; ++rx)
          if (xo + rx < Nx) o[rx] = accumulate ? o[rx] + r4[rx] : r4[rx];
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// spectral stage.  One lane per spaxel, marching z with a register window of the last
// 2*LWMAX+1 channels; the taps of a profile are wave-uniform (scalar loads), the window
// index of every FMA is a compile-time constant (switch on the half width).
// ------------------------------------------------------------------------------------
template <int LWMAX, int LW>
__device__ __forceinline__ float conv_lw(const float (&w)[2 * LWMAX + 1],
                                         const float *__restrict__ p) {
  float acc = 0.0f;
#pragma unroll
  for (int j = 0; j <= 2 * LW; ++j) acc = fmaf(p[j], w[LWMAX + LW - j], acc);
  return acc;
}

#define CASE_LW(N)                   \
  case N:                            \
    if constexpr (N <= LWMAX) return conv_lw<LWMAX, (N <= LWMAX ? N : 0)>(w, p); \
    break;

template <int LWMAX>
__device__ __forceinline__ float conv_sel(const float (&w)[2 * LWMAX + 1],
                                          const float *__restrict__ p, int lw) {
  switch (lw) {
    CASE_LW(0) CASE_LW(1) CASE_LW(2) CASE_LW(3) CASE_LW(4) CASE_LW(5) CASE_LW(6) CASE_LW(7)
    CASE_LW(8) CASE_LW(9) CASE_LW(10) CASE_LW(11) CASE_LW(12) CASE_LW(13) CASE_LW(14)
    CASE_LW(15) CASE_LW(16) CASE_LW(17) CASE_LW(18) CASE_LW(19) CASE_LW(20) CASE_LW(21)
    CASE_LW(22) CASE_LW(23) CASE_LW(24) CASE_LW(25) CASE_LW(26) CASE_LW(27) CASE_LW(28)
    CASE_LW(29) CASE_LW(30) CASE_LW(31) CASE_LW(32)
    default:
      break;
  }
  return 0.0f;
}
#undef CASE_LW

__device__ __forceinline__ int border_class(int t, int N, int P) {
  const int c = P / 2;
  return t < c ? t : (t > N - 1 - c ? P - 1 - (N - 1 - t) : c);
}

template <int LWMAX, bool GENERAL>
__global__ __launch_bounds__(256) void spectral_kernel(
    const float *__restrict__ fsf, const float *__restrict__ norm,
    const float *__restrict__ rden, const float *__restrict__ taps,
    const float *__restrict__ taps2, const int *__restrict__ tap_off, int K, int Kp, int Nz,
    int Ny, int Nx, int P, int zchunk, const uint8_t *__restrict__ mask,
    float *__restrict__ correl,
    uint8_t *__restrict__ profile, float *__restrict__ correl_min,
    float *__restrict__ part_max, float *__restrict__ part_min,
    const int *__restrict__ list, int nlist) {
  // with `list` the kernel only (re)computes the listed spaxels (border fix-up pass)
  constexpr int W = 2 * LWMAX + 1;
  const long S = (long)Ny * Nx;
  const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = list ? i0 < nlist : i0 < S;
  const long s = list ? (long)list[live ? i0 : 0] : i0;
  const long sc = live ? s : S - 1;
  const int z0 = blockIdx.y * zchunk;
  const int z1 = min(Nz, z0 + zchunk);

  const float *rd = nullptr;
  if constexpr (!GENERAL) {
    const int y = (int)(sc / Nx), x = (int)(sc - (long)y * Nx);
    const int cls = border_class(y, Ny, P) * P + border_class(x, Nx, P);
    rd = rden + (long)cls * K * Kp;  // Kp: z stride of the table
  }

  float w[W];
  float wn[GENERAL ? W : 1];
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const int zz = z0 - LWMAX + i;
    const bool in = zz >= 0 && zz < Nz;
    w[i] = in ? fsf[(long)zz * S + sc] : 0.0f;
    if constexpr (GENERAL) wn[i] = in ? norm[(long)zz * S + sc] : 0.0f;
  }

  float vmax = -INFINITY, vmin = INFINITY;
  for (int z = z0; z < z1; ++z) {
    float best = -INFINITY, worst = INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
      const int off = tap_off[k];
      const int lw = (tap_off[k + 1] - off - 1) >> 1;
      const float num = conv_sel<LWMAX>(w, taps + off, lw);
      float T;
      if constexpr (GENERAL) {
        const float den = conv_sel<LWMAX>(wn, taps2 + off, lw);
        T = den > 0.0f ? num / sqrtf(den) : 0.0f;  // den <= 0 -> inf -> T = 0  (lib :1057)
      } else {
        T = num * rd[(long)k * Kp + z];
      }
      if (T > best) {  // strict '>' : first maximum wins                      (lib :1210)
        best = T;
        bk = k;
      }
      worst = fminf(worst, T);
    }
    const long idx = (long)z * S + sc;
    if (mask && mask[idx]) {  // correl[mask] = 0 ; profile[mask] = 0   (steps.py:781,788)
      best = 0.0f;
      bk = 0;
    }
    if (live) {
      correl[idx] = best;
      profile[idx] = (uint8_t)bk;
      correl_min[idx] = worst;
    }
    vmax = fmaxf(vmax, best);
    vmin = fminf(vmin, worst);
    // slide the window by one channel
#pragma unroll
    for (int i = 0; i < W - 1; ++i) {
      w[i] = w[i + 1];
      if constexpr (GENERAL) wn[i] = wn[i + 1];
    }
    const int zn = z + 1 + LWMAX;
    const bool in = zn < Nz;
    w[W - 1] = in ? fsf[(long)zn * S + sc] : 0.0f;
    if constexpr (GENERAL) wn[W - 1] = in ? norm[(long)zn * S + sc] : 0.0f;
  }
  if (live && part_max) {
    part_max[(long)blockIdx.y * S + s] = vmax;
    part_min[(long)blockIdx.y * S + s] = vmin;
  }
}

// ------------------------------------------------------------------------------------
// spectral stage, packed and z-blocked.  One lane owns TWO adjacent spaxels (float2 loads,
// v_pk_fma_f32: the only way to the full fp32 rate on gfx950) and produces SPEC_ZC
// consecutive channels per step from a register window of 2*LWMAX + SPEC_ZC float2.
// Profiles are the OUTER loop of a step: the constants of profile k come as one fixed-length
// row  [lw_k (int bits), p_k[0], ..., p_k[2 lw_k], 0 ...]  fetched by a few wide scalar loads
// and then feed SPEC_ZC * (2 lw_k + 1) packed FMAs, so the scalar-load latency is amortised
// over hundreds of cycles of arithmetic.  The kernel normalises EVERY spaxel with the
// interior-class 1/sqrt(den) (wave-uniform, scalar loads); the spaxels within P/2 of the field
// border, whose normalisation differs, are recomputed afterwards by spectral_kernel on the
// plan's border list (a few percent of the field).
// ------------------------------------------------------------------------------------
constexpr int SPEC_ZC = 4;

template <int LWMAX, int LW>
__device__ __forceinline__ void conv3_one(const f32x2 (&w)[2 * LWMAX + SPEC_ZC],
                                          const float *__restrict__ taps,  // wave-uniform
                                          f32x2 (&num)[SPEC_ZC]) {
  constexpr int NT = 2 * LW + 1;         // taps of this profile
  constexpr int NCH = (NT + 15) / 16;    // chunks of 16 scalars
#pragma unroll
  for (int o = 0; o < SPEC_ZC; ++o) num[o] = (f32x2){0.f, 0.f};
  // Taps are consumed in chunks of 16 scalars from two alternating SGPR sets: the chunk
  // c+1 is requested right after chunk c has arrived and before the 64 packed FMAs of chunk c
  // are issued, so the scalar-load latency hides behind them.  Scalar loads return out of
  // order, hence the explicit lgkmcnt(0) / sched_barrier fences that pin this order.
  float ta[16], tb[16];
  auto load = [&](float (&t)[16], int c) {
#pragma unroll
    for (int i = 0; i < 16; ++i) t[i] = taps[16 * c + i];
  };
  auto fmas = [&](const float (&t)[16], int c, int i0, int i1) {
#pragma unroll
    for (int i = i0; i < i1; ++i) {
      const int j = 16 * c + i;
      if (j < NT) {
        const f32x2 pj = (f32x2){t[i], t[i]};
#pragma unroll
        for (int o = 0; o < SPEC_ZC; ++o)
          num[o] = __builtin_elementwise_fma(pj, w[LWMAX + o + LW - j], num[o]);
      }
    }
  };
  // hipcc's own waitcnt insertion puts lgkmcnt(0) in front of the first use of a chunk, so
  // the first tap of chunk c is consumed BEFORE chunk c+1 is requested: the wait then covers
  // only chunk c, and the request for c+1 flies during the remaining 15 x SPEC_ZC FMAs.
  load(ta, 0);
#pragma unroll
  for (int c = 0; c < NCH; c += 2) {
    fmas(ta, c, 0, 1);
    __builtin_amdgcn_sched_barrier(0);
    if (c + 1 < NCH) load(tb, c + 1);
    __builtin_amdgcn_sched_barrier(0);
    fmas(ta, c, 1, 16);
    if (c + 1 < NCH) {
      __builtin_amdgcn_sched_barrier(0);
      fmas(tb, c + 1, 0, 1);
      __builtin_amdgcn_sched_barrier(0);
      if (c + 2 < NCH) load(ta, c + 2);
      __builtin_amdgcn_sched_barrier(0);
      fmas(tb, c + 1, 1, 16);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

#define CASE3(N)                                                              \
  case N:                                                                     \
    if constexpr (N <= LWMAX) conv3_one<LWMAX, (N <= LWMAX ? N : 0)>(w, taps, num); \
    break;

template <int LWMAX>
__device__ __forceinline__ void conv3_sel(const f32x2 (&w)[2 * LWMAX + SPEC_ZC],
                                          const float *__restrict__ taps, int lw,
                                          f32x2 (&num)[SPEC_ZC]) {
  switch (lw) {
    CASE3(0) CASE3(1) CASE3(2) CASE3(3) CASE3(4) CASE3(5) CASE3(6) CASE3(7) CASE3(8) CASE3(9)
    CASE3(10) CASE3(11) CASE3(12) CASE3(13) CASE3(14) CASE3(15) CASE3(16) CASE3(17) CASE3(18)
    CASE3(19) CASE3(20) CASE3(21) CASE3(22) CASE3(23) CASE3(24) CASE3(25) CASE3(26) CASE3(27)
    CASE3(28) CASE3(29) CASE3(30) CASE3(31) CASE3(32)
    default:
#pragma unroll
      for (int o = 0; o < SPEC_ZC; ++o) num[o] = (f32x2){0.f, 0.f};
      break;
  }
}
#undef CASE3

template <int LWMAX>
__global__ __launch_bounds__(256) void spectral3_kernel(
    const float *__restrict__ fsf, const float *__restrict__ rdi, int NzP,
    const float *__restrict__ rows, int K, int Nz, int Ny, int Nx, int zchunk,
    const uint8_t *__restrict__ mask, float *__restrict__ correl,
    uint8_t *__restrict__ profile, float *__restrict__ correl_min, float *__restrict__ part_max,
    float *__restrict__ part_min) {
  constexpr int ZC = SPEC_ZC;
  constexpr int RL = (2 * LWMAX + 1 + 15) / 16 * 16 + 16;
  constexpr int W = 2 * LWMAX + ZC;
  const long S = (long)Ny * Nx;  // even
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  const bool live = 2 * t < S;
  const long s0 = live ? 2 * t : S - 2;
  const int z0 = blockIdx.y * zchunk;  // multiple of ZC
  const int z1 = min(Nz, z0 + zchunk);

  auto load2 = [&](int zz) -> f32x2 {
    if (zz < 0 || zz >= Nz) return (f32x2){0.f, 0.f};
    return *reinterpret_cast<const f32x2 *>(fsf + (long)zz * S + s0);
  };

  f32x2 w[W];
#pragma unroll
  for (int i = 0; i < W; ++i) w[i] = load2(z0 - LWMAX + i);

  f32x2 vmax = (f32x2){-INFINITY, -INFINITY}, vmin = (f32x2){INFINITY, INFINITY};
  for (int zb = z0; zb < z1; zb += ZC) {
    // request the planes that enter the window at the end of this step now: the loads have
    // the whole step (K profiles) to land
    f32x2 incoming[ZC];
#pragma unroll
    for (int o = 0; o < ZC; ++o) incoming[o] = load2(zb + ZC + LWMAX + o);
    unsigned short mk[ZC];  // mask bytes of the two spaxels, also requested a step ahead
#pragma unroll
    for (int o = 0; o < ZC; ++o)
      mk[o] = (mask && zb + o < z1)
                  ? *reinterpret_cast<const unsigned short *>(mask + (long)(zb + o) * S + s0)
                  : (unsigned short)0;
    f32x2 best[ZC], worst[ZC];
    int bk0[ZC], bk1[ZC];
#pragma unroll
    for (int o = 0; o < ZC; ++o) {
      best[o] = (f32x2){-INFINITY, -INFINITY};
      worst[o] = (f32x2){INFINITY, INFINITY};
      bk0[o] = bk1[o] = 0;
    }
    int lw_next = __float_as_int(rows[0]);
    for (int k = 0; k < K; ++k) {
      const float *rk = rows + (long)k * RL;  // wave-uniform -> wide scalar loads
      const int lw = lw_next;
      lw_next = __float_as_int(rk[RL]);  // rows has K+1 entries; used by the next iteration
      float rdu[ZC];
      {
        const float *ru = rdi + (long)k * NzP + zb;  // NzP >= Nz + ZC: no bound check
#pragma unroll
        for (int o = 0; o < ZC; ++o) rdu[o] = ru[o];
      }
      f32x2 num[ZC];
      conv3_sel<LWMAX>(w, rk + 1, lw, num);
#pragma unroll
      for (int o = 0; o < ZC; ++o) {
        const f32x2 T = num[o] * (f32x2){rdu[o], rdu[o]};
        // strict '>' : the first maximum wins                             (lib :1210)
        if (T.x > best[o].x) best[o].x = T.x, bk0[o] = k;
        if (T.y > best[o].y) best[o].y = T.y, bk1[o] = k;
        worst[o].x = fminf(worst[o].x, T.x);
        worst[o].y = fminf(worst[o].y, T.y);
      }
    }
#pragma unroll
    for (int o = 0; o < ZC; ++o) {
      const int zz = zb + o;
      if (zz < z1) {
        const long idx = (long)zz * S + s0;
        f32x2 b = best[o];
        int k0 = bk0[o], k1 = bk1[o];
        // correl[mask] = 0 ; profile[mask] = 0                        (steps.py:781,788)
        if (mk[o] & 0x00ff) b.x = 0.0f, k0 = 0;
        if (mk[o] & 0xff00) b.y = 0.0f, k1 = 0;
        if (live) {
          *reinterpret_cast<f32x2 *>(correl + idx) = b;
          *reinterpret_cast<f32x2 *>(correl_min + idx) = worst[o];
          *reinterpret_cast<unsigned short *>(profile + idx) = (unsigned short)(k0 | (k1 << 8));
        }
        vmax.x = fmaxf(vmax.x, b.x), vmax.y = fmaxf(vmax.y, b.y);
        vmin.x = fminf(vmin.x, worst[o].x), vmin.y = fminf(vmin.y, worst[o].y);
      }
    }
    // slide the window by ZC channels
#pragma unroll
    for (int i = 0; i < W - ZC; ++i) w[i] = w[i + ZC];
#pragma unroll
    for (int o = 0; o < ZC; ++o) w[W - ZC + o] = incoming[o];
  }
  if (live && part_max) {
    *reinterpret_cast<f32x2 *>(part_max + (long)blockIdx.y * S + s0) = vmax;
    *reinterpret_cast<f32x2 *>(part_min + (long)blockIdx.y * S + s0) = vmin;
  }
}

// fallback for profiles wider than the register window: plain loops over global memory
template <bool GENERAL>
__global__ __launch_bounds__(256) void spectral_generic_kernel(
    const float *__restrict__ fsf, const float *__restrict__ norm,
    const float *__restrict__ rden, const float *__restrict__ taps,
    const float *__restrict__ taps2, const int *__restrict__ tap_off, int K, int Kp, int Nz,
    int Ny, int Nx, int P, int zchunk, const uint8_t *__restrict__ mask,
    float *__restrict__ correl,
    uint8_t *__restrict__ profile, float *__restrict__ correl_min,
    float *__restrict__ part_max, float *__restrict__ part_min,
    const int *__restrict__ list, int nlist) {
  const long S = (long)Ny * Nx;
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  (void)list;
  (void)nlist;
  if (s >= S) return;
  const int z0 = blockIdx.y * zchunk;
  const int z1 = min(Nz, z0 + zchunk);
  const float *rd = nullptr;
  if constexpr (!GENERAL) {
    const int y = (int)(s / Nx), x = (int)(s - (long)y * Nx);
    rd = rden + (long)(border_class(y, Ny, P) * P + border_class(x, Nx, P)) * K * Kp;
  }
  float vmax = -INFINITY, vmin = INFINITY;
  for (int z = z0; z < z1; ++z) {
    float best = -INFINITY, worst = INFINITY;
    int bk = 0;
    for (int k = 0; k < K; ++k) {
      const int off = tap_off[k], L = tap_off[k + 1] - off, lw = (L - 1) >> 1;
      float num = 0.0f, den = 0.0f;
      for (int j = 0; j < L; ++j) {
        const int zz = z + lw - j;
        if (zz >= 0 && zz < Nz) {
          num = fmaf(taps[off + j], fsf[(long)zz * S + s], num);
          if constexpr (GENERAL) den = fmaf(taps2[off + j], norm[(long)zz * S + s], den);
        }
      }
      float T;
      if constexpr (GENERAL)
        T = den > 0.0f ? num / sqrtf(den) : 0.0f;
      else
        T = num * rd[(long)k * Kp + z];
      if (T > best) {
        best = T;
        bk = k;
      }
      worst = fminf(worst, T);
    }
    const long idx = (long)z * S + s;
    if (mask && mask[idx]) {
      best = 0.0f;
      bk = 0;
    }
    correl[idx] = best;
    profile[idx] = (uint8_t)bk;
    correl_min[idx] = worst;
    vmax = fmaxf(vmax, best);
    vmin = fminf(vmin, worst);
  }
  if (part_max) {
    part_max[(long)blockIdx.y * S + s] = vmax;
    part_min[(long)blockIdx.y * S + s] = vmin;
  }
}

// maxmap / minmap of the listed spaxels straight from the final cubes (border fix-up).
// Lanes run over list entries (border rows are contiguous in memory), z is cut in slices
// whose partial extrema are merged with ordered-int atomics (max/min are order independent,
// so the result is deterministic).
__device__ __forceinline__ void atomic_max_f(float *addr, float v) {
  if (v >= 0.0f)
    atomicMax(reinterpret_cast<int *>(addr), __float_as_int(v));
  else
    atomicMin(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}
__device__ __forceinline__ void atomic_min_f(float *addr, float v) {
  if (v >= 0.0f)
    atomicMin(reinterpret_cast<int *>(addr), __float_as_int(v));
  else
    atomicMax(reinterpret_cast<unsigned *>(addr), __float_as_uint(v));
}

__global__ __launch_bounds__(256) void list_maps_init_kernel(const int *__restrict__ list, int nlist,
                                                             float *__restrict__ maxmap,
                                                             float *__restrict__ minmap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nlist) return;
  if (maxmap) maxmap[list[i]] = -INFINITY;
  if (minmap) minmap[list[i]] = INFINITY;
}

__global__ __launch_bounds__(256) void list_maps_kernel(const float *__restrict__ correl,
                                                        const float *__restrict__ correl_min,
                                                        int Nz, long S, int zper,
                                                        const int *__restrict__ list, int nlist,
                                                        float *__restrict__ maxmap,
                                                        float *__restrict__ minmap) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nlist) return;
  const long s = list[i];
  const int z0 = blockIdx.y * zper, z1 = min(Nz, z0 + zper);
  float a = -INFINITY, b = INFINITY;
  for (int z = z0; z < z1; ++z) {
    a = fmaxf(a, correl[(long)z * S + s]);
    b = fminf(b, correl_min[(long)z * S + s]);
  }
  if (maxmap) atomic_max_f(maxmap + s, a);
  if (minmap) atomic_min_f(minmap + s, b);
}

int spectral_zchunks(origin_ctx *ctx, long S, int Nz, int lwmax) {
  const long blocks = (S + 255) / 256;
  long want = ((long)ctx->num_cu * 8 + blocks - 1) / blocks;
  // the window warm-up reads 2*lwmax extra channels per chunk: keep chunks >= 4 windows
  const long maxc = std::max(1L, (long)Nz / (8L * lwmax + 8));
  if (want > maxc) want = maxc;
  if (want < 1) want = 1;
  return (int)want;
}

}  // namespace

template <int P>
static void launch_spatial4x4(origin_ctx *ctx, dim3 grid, bool vec, const float *A, const float *B,
                              const float *taps, int Nz, int Ny, int Nx, int zper, int acc,
                              float *out) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, A, B, taps, Nz, Ny, Nx, zper, acc,
                       out);
  };
  if (vec && B) go(spatial4x4_kernel<P, true, true>);
  else if (vec) go(spatial4x4_kernel<P, true, false>);
  else if (B) go(spatial4x4_kernel<P, false, true>);
  else go(spatial4x4_kernel<P, false, false>);
}

int glr_fp32_spatial(origin_ctx *ctx, const float *A, const float *B, const float *taps, int Nz,
                     int Ny, int Nx, int P, int accumulate, float *out) {
  // each block marches `zper` channels of one 64x64 tile, prefetching the next plane
  const long tiles = (long)cdiv(Nx, 64) * cdiv(Ny, 64);
  int nzb = (int)(((long)ctx->num_cu * 16 + tiles - 1) / tiles);
  nzb = std::max(1, std::min(nzb, Nz));
  const int zper = cdiv(Nz, nzb);
  dim3 g4(cdiv(Nx, 64), cdiv(Ny, 64), cdiv(Nz, zper));
  const bool vec = (Nx & 3) == 0 && ((P / 2) & 3) == 0;
  switch (A ? P : 0) {  // A == NULL (norm of the weights) takes the generic kernel
    case 7:
      launch_spatial4x4<7>(ctx, g4, vec, A, B, taps, Nz, Ny, Nx, zper, accumulate, out);
      break;
    case 9:
      launch_spatial4x4<9>(ctx, g4, vec, A, B, taps, Nz, Ny, Nx, zper, accumulate, out);
      break;
    case 25:
      launch_spatial4x4<25>(ctx, g4, vec, A, B, taps, Nz, Ny, Nx, zper, accumulate, out);
      break;
    default: {  // any other odd PSF size: generic LDS-tiled kernel
      dim3 sgrid(cdiv(Nx, TX), cdiv(Ny, TY), Nz), sblock(64, 4);
      const size_t lds = (size_t)(TY + P - 1) * (TX + P - 1) * sizeof(float);
      hipLaunchKernelGGL(spatial_kernel, sgrid, sblock, lds, ctx->stream, A, B, taps, Ny, Nx, P,
                         accumulate, out);
    }
  }
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

// the border spaxels of the packed form: exact per-class normalisation
static void launch_border_pass(origin_ctx *ctx, const origin_glr_plan *pl, const GlrSpectralIO &io) {
  // few spaxels: cut z finer so that the pass still fills the chip (its maps are redone from the
  // final cubes by glr_fp32_border_maps, so it writes no partials)
  const int Nz = pl->Nz;
  const long bb = cdiv(pl->nborder, 256);
  int nzb = (int)(((long)ctx->num_cu * 12 + bb - 1) / bb);
  nzb = std::max(1, std::min(nzb, Nz / (4 * std::max(pl->lwmax, 1) + 4)));
  const int zcb = cdiv(Nz, nzb);
  dim3 gb((unsigned)bb, cdiv(Nz, zcb));
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, gb, dim3(256), 0, ctx->stream, io.fsf, io.norm, pl->d_rden, pl->d_taps,
                       pl->d_taps2, pl->d_tap_off, pl->K, pl->Kp, Nz, pl->Ny, pl->Nx, pl->P, zcb,
                       io.mask, io.correl, io.profile, io.correl_min, (float *)nullptr,
                       (float *)nullptr, pl->d_border, pl->nborder);
  };
  if (pl->lwmax <= 8) go(spectral_kernel<8, false>);
  else if (pl->lwmax <= 16) go(spectral_kernel<16, false>);
  else go(spectral_kernel<32, false>);
}

int glr_fp32_spectral(origin_ctx *ctx, const origin_glr_plan *pl, GlrSpectral form,
                      GlrSpectralIO *io, ProfScope *ps) {
  const int Nz = pl->Nz, Ny = pl->Ny, Nx = pl->Nx, K = pl->K;
  const long S = (long)Ny * Nx;
  int nzc = std::min(64, spectral_zchunks(ctx, S, Nz, std::max(pl->lwmax, 1)));
  int zchunk = cdiv(Nz, nzc);
  zchunk = (zchunk + SPEC_ZC - 1) / SPEC_ZC * SPEC_ZC;  // the packed kernel steps SPEC_ZC channels
  nzc = cdiv(Nz, zchunk);
  io->nzc = nzc;
  io->pmax = io->want_maps ? io->part : nullptr;
  io->pmin = io->want_maps ? io->part + (size_t)nzc * S : nullptr;
  const bool gen = pl->mode == 1;
  auto go = [&](auto general, auto specific) {
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(cdiv(S, 256), nzc), dim3(256), 0, ctx->stream, io->fsf,
                         io->norm, pl->d_rden, pl->d_taps, pl->d_taps2, pl->d_tap_off, K, pl->Kp, Nz,
                         Ny, Nx, pl->P, zchunk, io->mask, io->correl, io->profile, io->correl_min,
                         io->pmax, io->pmin, (const int *)nullptr, 0);
    };
    if (gen) launch(general);
    else launch(specific);
  };
  if (form == GLR_SPEC_PACKED) {
    // one lane = two adjacent spaxels, SPEC_ZC channels per step
    auto go3 = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, dim3(cdiv(S / 2, 256), nzc), dim3(256), 0, ctx->stream, io->fsf,
                         pl->d_rdi, pl->NzP, pl->d_rows, K, Nz, Ny, Nx, zchunk, io->mask, io->correl,
                         io->profile, io->correl_min, io->pmax, io->pmin);
    };
    switch (pl->lwt) {
      case 8: go3(spectral3_kernel<8>); break;
      case 16: go3(spectral3_kernel<16>); break;
      case 24: go3(spectral3_kernel<24>); break;
      case 29: go3(spectral3_kernel<29>); break;
      default: go3(spectral3_kernel<32>); break;
    }
    if (pl->nborder > 0) {
      ps->next(K_GLR_BORDER);
      launch_border_pass(ctx, pl, *io);
    }
  } else if (form == GLR_SPEC_GENERIC) {
    go(spectral_generic_kernel<true>, spectral_generic_kernel<false>);
  } else if (pl->lwmax <= 8) {
    go(spectral_kernel<8, true>, spectral_kernel<8, false>);
  } else if (pl->lwmax <= 16) {
    go(spectral_kernel<16, true>, spectral_kernel<16, false>);
  } else {
    go(spectral_kernel<32, true>, spectral_kernel<32, false>);
  }
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

int glr_fp32_border_maps(origin_ctx *ctx, const origin_glr_plan *pl, const float *correl,
                         const float *correl_min, float *maxmap, float *minmap) {
  const int zper = 64;
  const long S = (long)pl->Ny * pl->Nx;
  hipLaunchKernelGGL(list_maps_init_kernel, dim3(cdiv(pl->nborder, 256)), dim3(256), 0, ctx->stream,
                     pl->d_border, pl->nborder, maxmap, minmap);
  hipLaunchKernelGGL(list_maps_kernel, dim3(cdiv(pl->nborder, 256), cdiv(pl->Nz, zper)), dim3(256),
                     0, ctx->stream, correl, correl_min, pl->Nz, S, zper, pl->d_border, pl->nborder,
                     maxmap, minmap);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}
