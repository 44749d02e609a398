// Step 0 on the device: the DATA and STAT data units of a MUSE cube file become the three
// arrays every step starts from, and the white image, in one pass.
//
// ORIGIN.__init__ opens the file with mpdaf's Cube (origin.py:213), which reads both units as
// float64 and masks the voxels where either is not finite; cube_raw / var / mask (origin.py:262-274)
// are then data.filled(0), var.filled(inf) and the mask, and ima_white (origin.py:240) is the
// masked mean over z.  Here the file's big-endian bytes are copied to HBM as they are, and one
// kernel swaps, narrows, masks and fills them and adds the planes to the per-spaxel sums.  The
// planes may be whole or one rank's band of rows (origin_cube_read_rows), and a DQ unit, where
// the caller gives one, masks the voxels whose element is not zero.
//
// Pure byte work, HBM bound: per voxel |BITPIX| / 8 bytes of each unit in, 4 + 4 + 1 bytes out;
// the sums (8 + 4 bytes per spaxel) move once per launch, not once per plane.
#include <errno.h>
#include <unistd.h>

#include "common.h"

namespace {

// N consecutive file elements from element index e on, as float32 bit patterns.  BITPIX -32 is
// a byte swap; -64 a swap and the rounding (float) of the float64 value: beyond the float32
// range that gives inf, below it 0.  N == 4 reads 16 bytes at a time.
template <int BITPIX, int N>
__device__ __forceinline__ void load_be(const uint8_t *__restrict__ src, long e, unsigned (&bits)[N]) {
  if (BITPIX == -32) {
    if constexpr (N == 4) {
      const uint4 q = *(const uint4 *)(src + e * 4);
      bits[0] = __builtin_bswap32(q.x), bits[1] = __builtin_bswap32(q.y);
      bits[2] = __builtin_bswap32(q.z), bits[3] = __builtin_bswap32(q.w);
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) bits[i] = __builtin_bswap32(((const unsigned *)src)[e + i]);
    }
  } else {
    if constexpr (N == 4) {
      const uint4 a = *(const uint4 *)(src + e * 8), b = *(const uint4 *)(src + e * 8 + 16);
      const unsigned w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const unsigned long long v = ((unsigned long long)__builtin_bswap32(w[2 * i]) << 32) |
                                     __builtin_bswap32(w[2 * i + 1]);
        bits[i] = __float_as_uint((float)__longlong_as_double((long long)v));
      }
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const unsigned long long v = __builtin_bswap64(((const unsigned long long *)src)[e + i]);
        bits[i] = __float_as_uint((float)__longlong_as_double((long long)v));
      }
    }
  }
}

__device__ __forceinline__ bool finite_bits(unsigned b) { return (b & 0x7f800000u) != 0x7f800000u; }

// The DQ flags of N consecutive voxels from element index e on: f[i] != 0 where the element is
// not zero.  That test needs no byte swap, so the big-endian bytes are looked at as they lie:
// N == 4 reads the four elements with one 4- (BITPIX 8), 8- (16) or 16-byte (32) load.
template <int BQ, int N>
__device__ __forceinline__ void load_dq(const uint8_t *__restrict__ src, long e, unsigned (&f)[N]) {
  if constexpr (N == 4) {
    if constexpr (BQ == 8) {
      const unsigned q = *(const unsigned *)(src + e);
      f[0] = q & 0xffu, f[1] = q & 0xff00u, f[2] = q & 0xff0000u, f[3] = q & 0xff000000u;
    } else if constexpr (BQ == 16) {
      const uint2 q = *(const uint2 *)(src + e * 2);
      f[0] = q.x & 0xffffu, f[1] = q.x & 0xffff0000u, f[2] = q.y & 0xffffu, f[3] = q.y & 0xffff0000u;
    } else {
      const uint4 q = *(const uint4 *)(src + e * 4);
      f[0] = q.x, f[1] = q.y, f[2] = q.z, f[3] = q.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (BQ == 8) f[i] = src[e + i];
      else if constexpr (BQ == 16) f[i] = ((const unsigned short *)src)[e + i];
      else f[i] = ((const unsigned *)src)[e + i];
    }
  }
}

// A lane owns N consecutive voxels of a plane (N == 4: 16-byte loads and stores, one 4-byte mask
// store; N == 1 where S % 4 != 0 or a base is not 16-byte aligned) and marches the chunk's planes
// with the sums of its spaxels in registers: read once, one plane added after the other, written
// once.  No other lane of the launch touches those spaxels, and launches are ordered on the stream.
// BQ: BITPIX of the DQ unit (8, 16, 32) whose non-zero elements are masked too; 0: no DQ unit.
template <int BD, int BS, int BQ, int N>
__global__ __launch_bounds__(64) void cube_ingest_kernel(
    const uint8_t *__restrict__ data_be, const uint8_t *__restrict__ stat_be,
    const uint8_t *__restrict__ dq_be, int nplanes, long S,
    float *__restrict__ raw, float *__restrict__ var, uint8_t *__restrict__ mask,
    double *__restrict__ wsum, int *__restrict__ wcnt) {
  const long groups = S / N;
  const long stride = (long)gridDim.x * 64;
  for (long g = (long)blockIdx.x * 64 + threadIdx.x; g < groups; g += stride) {
    const long s = g * N;
    double sum[N];
    int cnt[N];
    if constexpr (N == 4) {
      const double2 s0 = *(const double2 *)(wsum + s), s1 = *(const double2 *)(wsum + s + 2);
      const int4 c = *(const int4 *)(wcnt + s);
      sum[0] = s0.x, sum[1] = s0.y, sum[2] = s1.x, sum[3] = s1.y;
      cnt[0] = c.x, cnt[1] = c.y, cnt[2] = c.z, cnt[3] = c.w;
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) sum[i] = wsum[s + i], cnt[i] = wcnt[s + i];
    }
#pragma unroll 2
    for (int p = 0; p < nplanes; ++p) {
      const long e = (long)p * S + s;
      unsigned d[N], v[N], m[N];
      load_be<BD, N>(data_be, e, d);
      load_be<BS, N>(stat_be, e, v);
      if constexpr (BQ != 0) load_dq<BQ, N>(dq_be, e, m);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        if constexpr (BQ != 0)
          m[i] = !(finite_bits(d[i]) && finite_bits(v[i])) || m[i] != 0;
        else
          m[i] = !(finite_bits(d[i]) && finite_bits(v[i]));
        d[i] = m[i] ? 0u : d[i];
        v[i] = m[i] ? 0x7f800000u : v[i];
        // (a masked voxel adds +0.0, as NumPy's sum of data.filled(0) does; a lone -0.0 too
        // sums to +0.0 there, since np.add.reduce starts from its identity +0.0 as the sums do)
        sum[i] += (double)__uint_as_float(d[i]);
        cnt[i] += m[i] ? 0 : 1;
      }
      if constexpr (N == 4) {
        *(uint4 *)(raw + e) = make_uint4(d[0], d[1], d[2], d[3]);
        *(uint4 *)(var + e) = make_uint4(v[0], v[1], v[2], v[3]);
        *(unsigned *)(mask + e) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          ((unsigned *)raw)[e + i] = d[i];
          ((unsigned *)var)[e + i] = v[i];
          mask[e + i] = (uint8_t)m[i];
        }
      }
    }
    if constexpr (N == 4) {
      *(double2 *)(wsum + s) = make_double2(sum[0], sum[1]);
      *(double2 *)(wsum + s + 2) = make_double2(sum[2], sum[3]);
      *(int4 *)(wcnt + s) = make_int4(cnt[0], cnt[1], cnt[2], cnt[3]);
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) wsum[s + i] = sum[i], wcnt[s + i] = cnt[i];
    }
  }
}

template <int BD, int BS, int BQ>
void launch_ingest(origin_ctx *ctx, bool vec, const uint8_t *d, const uint8_t *s, const uint8_t *q,
                   int nplanes, long S, float *raw, float *var, uint8_t *mask, double *wsum,
                   int *wcnt) {
  const long groups = vec ? S / 4 : S;
  const int grid = (int)std::min<long>((groups + 63) / 64, (long)ctx->num_cu * 32);
  if (vec)
    hipLaunchKernelGGL((cube_ingest_kernel<BD, BS, BQ, 4>), dim3(grid), dim3(64), 0, ctx->stream, d,
                       s, q, nplanes, S, raw, var, mask, wsum, wcnt);
  else
    hipLaunchKernelGGL((cube_ingest_kernel<BD, BS, BQ, 1>), dim3(grid), dim3(64), 0, ctx->stream, d,
                       s, q, nplanes, S, raw, var, mask, wsum, wcnt);
}

template <int BD, int BS, class... A>
void launch_ingest_dq(int bitpix_dq, A... a) {
  switch (bitpix_dq) {
    case 0: return launch_ingest<BD, BS, 0>(a...);
    case 8: return launch_ingest<BD, BS, 8>(a...);
    case 16: return launch_ingest<BD, BS, 16>(a...);
    default: return launch_ingest<BD, BS, 32>(a...);
  }
}

bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int pread_all(int fd, char *p, size_t bytes, off_t off) {
  while (bytes) {
    const ssize_t r = ::pread(fd, p, bytes, off);
    if (r < 0 && errno == EINTR) continue;
    if (r <= 0) {
      origin_set_error(r == 0 ? "unexpected end of file" : "read failed: %s", strerror(errno));
      return ORIGIN_E_STATE;
    }
    p += r, off += r;
    bytes -= (size_t)r;
  }
  return ORIGIN_OK;
}

}  // namespace

extern "C" {

int origin_cube_ingest_planes_dq(origin_ctx *ctx, const void *d_data_be, int bitpix_data,
                                 const void *d_stat_be, int bitpix_stat, const void *d_dq_be,
                                 int bitpix_dq, int nplanes, long S, float *d_raw, float *d_var,
                                 uint8_t *d_mask, double *d_white_sum, int *d_white_cnt) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(d_data_be && d_stat_be && d_raw && d_var && d_mask && d_white_sum && d_white_cnt,
                   "null pointer");
  ORIGIN_CHECK_ARG(nplanes > 0 && S > 0, "bad shape: %d planes of %ld spaxels", nplanes, S);
  ORIGIN_CHECK_ARG((bitpix_data == -32 || bitpix_data == -64) &&
                       (bitpix_stat == -32 || bitpix_stat == -64),
                   "BITPIX %d / %d: only -32 and -64 are ingested", bitpix_data, bitpix_stat);
  ORIGIN_CHECK_ARG(d_dq_be ? (bitpix_dq == 8 || bitpix_dq == 16 || bitpix_dq == 32) : bitpix_dq == 0,
                   "DQ BITPIX %d: 8, 16 or 32 with a DQ unit, 0 without one", bitpix_dq);
  ORIGIN_CHECK_ARG(aligned(d_data_be, 8) && aligned(d_stat_be, 8), "file bytes must be 8-byte aligned");
  ORIGIN_CHECK_ARG(!d_dq_be || aligned(d_dq_be, bitpix_dq / 8),
                   "DQ bytes must be aligned to their %d-byte elements", bitpix_dq / 8);
  ORIGIN_CHECK_ARG(aligned(d_raw, 4) && aligned(d_var, 4) && aligned(d_white_sum, 8) &&
                       aligned(d_white_cnt, 4),
                   "misaligned output");
  // (the four DQ elements of a lane are one load of 4 * bitpix_dq / 8 bytes)
  const bool vec = S % 4 == 0 && aligned(d_data_be, 16) && aligned(d_stat_be, 16) &&
                   (!d_dq_be || aligned(d_dq_be, bitpix_dq / 2)) && aligned(d_raw, 16) &&
                   aligned(d_var, 16) && aligned(d_mask, 4) && aligned(d_white_sum, 16) &&
                   aligned(d_white_cnt, 16);
  const uint8_t *d = (const uint8_t *)d_data_be, *s = (const uint8_t *)d_stat_be,
                *q = (const uint8_t *)d_dq_be;
  if (bitpix_data == -32 && bitpix_stat == -32)
    launch_ingest_dq<-32, -32>(bitpix_dq, ctx, vec, d, s, q, nplanes, S, d_raw, d_var, d_mask,
                               d_white_sum, d_white_cnt);
  else if (bitpix_data == -32)
    launch_ingest_dq<-32, -64>(bitpix_dq, ctx, vec, d, s, q, nplanes, S, d_raw, d_var, d_mask,
                               d_white_sum, d_white_cnt);
  else if (bitpix_stat == -32)
    launch_ingest_dq<-64, -32>(bitpix_dq, ctx, vec, d, s, q, nplanes, S, d_raw, d_var, d_mask,
                               d_white_sum, d_white_cnt);
  else
    launch_ingest_dq<-64, -64>(bitpix_dq, ctx, vec, d, s, q, nplanes, S, d_raw, d_var, d_mask,
                               d_white_sum, d_white_cnt);
  ORIGIN_LAUNCH_CHECK();
  return ORIGIN_OK;
}

int origin_cube_ingest_planes(origin_ctx *ctx, const void *d_data_be, int bitpix_data,
                              const void *d_stat_be, int bitpix_stat, int nplanes, long S,
                              float *d_raw, float *d_var, uint8_t *d_mask, double *d_white_sum,
                              int *d_white_cnt) {
  return origin_cube_ingest_planes_dq(ctx, d_data_be, bitpix_data, d_stat_be, bitpix_stat, nullptr,
                                      0, nplanes, S, d_raw, d_var, d_mask, d_white_sum,
                                      d_white_cnt);
}

// The stream behind both readers: spaxels [first, first + S) of every plane of `plane` spaxels.
// A band of whole rows is one contiguous byte range of a plane, and the whole plane one of the
// unit, so a chunk of whole planes is one pread per unit and a chunk of bands one per plane and
// unit; in the pinned buffer the chunk's planes lie packed: DATA, STAT, DQ (each 256-byte aligned).
static int read_band(origin_ctx *ctx, int fd, long off_data, int bitpix_data, long off_stat,
                     int bitpix_stat, long off_dq, int bitpix_dq, int Nz, long plane, long first,
                     long S, int planes_per_chunk, float *d_raw, float *d_var, uint8_t *d_mask,
                     double *d_white_sum, int *d_white_cnt) {
  const long w[3] = {-bitpix_data / 8, -bitpix_stat / 8, off_dq < 0 ? 0 : bitpix_dq / 8};
  const long off[3] = {off_data, off_stat, off_dq};
  long ppc = planes_per_chunk ? planes_per_chunk
                              : std::max(1l, IO_CHUNK_BYTES / (S * (w[0] + w[1] + w[2])));
  ppc = std::min<long>(ppc, Nz);
  size_t at[4] = {0, 0, 0, 0};
  for (int u = 0; u < 3; ++u) at[u + 1] = (at[u] + (size_t)(ppc * S * w[u]) + 255) & ~(size_t)255;
  const size_t buf = at[3];
  void *scr = nullptr;
  int rc = origin_scratch(ctx, 2 * buf, &scr);
  if (rc) return rc;
  IoStage st;
  for (int i = 0; i < 2; ++i) {
    ORIGIN_HIP(hipHostMalloc(&st.h[i], buf, hipHostMallocDefault));
    ORIGIN_HIP(hipEventCreateWithFlags(&st.ev[i], hipEventDisableTiming));
  }
  ORIGIN_HIP(hipMemsetAsync(d_white_sum, 0, (size_t)S * sizeof(double), ctx->stream));
  ORIGIN_HIP(hipMemsetAsync(d_white_cnt, 0, (size_t)S * sizeof(int), ctx->stream));
  const long nchunks = (Nz + ppc - 1) / ppc;
  for (long k = 0; k < nchunks; ++k) {
    const long z0 = k * ppc, np = std::min(ppc, Nz - z0);
    char *h = (char *)st.h[k & 1], *d = (char *)scr + (k & 1) * buf;
    if (k >= 2) ORIGIN_HIP(hipEventSynchronize(st.ev[k & 1]));  // buffer free again
    for (int u = 0; u < 3 && !rc; ++u) {
      if (!w[u]) continue;
      if (S == plane) {
        rc = pread_all(fd, h + at[u], (size_t)(np * S * w[u]), (off_t)(off[u] + z0 * S * w[u]));
      } else {
        for (long z = z0; z < z0 + np && !rc; ++z)
          rc = pread_all(fd, h + at[u] + (size_t)((z - z0) * S * w[u]), (size_t)(S * w[u]),
                         (off_t)(off[u] + (z * plane + first) * w[u]));
      }
    }
    if (rc) {
      (void)hipStreamSynchronize(ctx->stream);
      return rc;
    }
    for (int u = 0; u < 3; ++u)
      if (w[u])
        ORIGIN_HIP(hipMemcpyAsync(d + at[u], h + at[u], (size_t)(np * S * w[u]),
                                  hipMemcpyHostToDevice, ctx->stream));
    ORIGIN_HIP(hipEventRecord(st.ev[k & 1], ctx->stream));
    rc = origin_cube_ingest_planes_dq(ctx, d, bitpix_data, d + at[1], bitpix_stat,
                                      w[2] ? d + at[2] : nullptr, w[2] ? bitpix_dq : 0, (int)np, S,
                                      d_raw + z0 * S, d_var + z0 * S, d_mask + z0 * S, d_white_sum,
                                      d_white_cnt);
    if (rc) {
      (void)hipStreamSynchronize(ctx->stream);
      return rc;
    }
  }
  ORIGIN_HIP(hipStreamSynchronize(ctx->stream));
  return ORIGIN_OK;
}

int origin_cube_read(origin_ctx *ctx, int fd, long off_data, int bitpix_data, long off_stat,
                     int bitpix_stat, int Nz, long S, int planes_per_chunk, float *d_raw,
                     float *d_var, uint8_t *d_mask, double *d_white_sum, int *d_white_cnt) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(fd >= 0 && off_data >= 0 && off_stat >= 0 && Nz > 0 && S > 0 &&
                       planes_per_chunk >= 0,
                   "bad arguments");
  ORIGIN_CHECK_ARG((bitpix_data == -32 || bitpix_data == -64) &&
                       (bitpix_stat == -32 || bitpix_stat == -64),
                   "BITPIX %d / %d: only -32 and -64 are ingested", bitpix_data, bitpix_stat);
  return read_band(ctx, fd, off_data, bitpix_data, off_stat, bitpix_stat, -1, 0, Nz, S, 0, S,
                   planes_per_chunk, d_raw, d_var, d_mask, d_white_sum, d_white_cnt);
}

int origin_cube_read_rows(origin_ctx *ctx, int fd, long off_data, int bitpix_data, long off_stat,
                          int bitpix_stat, long off_dq, int bitpix_dq, int Nz, int Ny, int Nx,
                          int y0, int y1, int planes_per_chunk, float *d_raw, float *d_var,
                          uint8_t *d_mask, double *d_white_sum, int *d_white_cnt) {
  ORIGIN_USE(ctx);
  ORIGIN_CHECK_ARG(fd >= 0 && off_data >= 0 && off_stat >= 0 && planes_per_chunk >= 0,
                   "bad arguments");
  ORIGIN_CHECK_ARG(d_raw && d_var && d_mask && d_white_sum && d_white_cnt, "null pointer");
  ORIGIN_CHECK_ARG(Nz > 0 && Ny > 0 && Nx > 0 && 0 <= y0 && y0 < y1 && y1 <= Ny,
                   "bad shape: rows [%d, %d) of a %d x %d x %d cube", y0, y1, Nz, Ny, Nx);
  ORIGIN_CHECK_ARG((bitpix_data == -32 || bitpix_data == -64) &&
                       (bitpix_stat == -32 || bitpix_stat == -64),
                   "BITPIX %d / %d: only -32 and -64 are ingested", bitpix_data, bitpix_stat);
  ORIGIN_CHECK_ARG(off_dq < 0 || bitpix_dq == 8 || bitpix_dq == 16 || bitpix_dq == 32,
                   "DQ BITPIX %d: only 8, 16 and 32 are read", bitpix_dq);
  return read_band(ctx, fd, off_data, bitpix_data, off_stat, bitpix_stat, off_dq, bitpix_dq, Nz,
                   (long)Ny * Nx, (long)y0 * Nx, (long)(y1 - y0) * Nx, planes_per_chunk, d_raw,
                   d_var, d_mask, d_white_sum, d_white_cnt);
}

}  // extern "C"
