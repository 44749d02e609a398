/*
 * origin_hip.h -- C ABI of liborigin_hip.so, the MI355X (gfx950) implementation of
 * ORIGIN's dense hot path.
 *
 * The reference (musevlt/origin) has no FFI: its hot path is four Python functions in
 * muse_origin/lib_origin.py that Step.run bodies in muse_origin/steps.py resolve by
 * name (steps.py:19-41).  This ABI is what those functions are re-implemented on; each
 * entry point cites the reference interface it replaces.  The Python binding is
 * origin_amd/_capi.py (ctypes); INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success or a negative ORIGIN_E_* code; the message of
 *     the last failure on the calling thread is origin_last_error().  Nothing aborts.
 *   - cubes are C-order (Nz, Ny, Nx), x fastest, float32; masks / profile indices uint8.
 *   - pointers named d_* are DEVICE pointers obtained from origin_malloc (or any HIP
 *     allocation on the context's device); h_* are host pointers.  The library never
 *     keeps a caller pointer after the call returns, except plan objects that own
 *     private device copies of what they were given.
 *   - all work is enqueued on the context's stream; calls that return host values
 *     synchronise, the others are asynchronous (origin_sync to wait).
 *   - one host thread per context; a context is not re-entrant.
 */
#ifndef ORIGIN_HIP_H
#define ORIGIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORIGIN_OK 0
#define ORIGIN_E_ARG (-1)      /* bad argument / unsupported size            */
#define ORIGIN_E_NOMEM (-2)    /* device allocation failed                    */
#define ORIGIN_E_HIP (-3)      /* a HIP runtime call or kernel launch failed  */
#define ORIGIN_E_NODEVICE (-4) /* no usable GPU                               */
#define ORIGIN_E_STATE (-5)    /* call order / plan mismatch                  */

typedef struct origin_ctx origin_ctx;
typedef struct origin_glr_plan origin_glr_plan;

/* ---- context, memory, timing ------------------------------------------------------ */
const char *origin_last_error(void);
int origin_abi_version(void);
int origin_device_count(int *count);
int origin_ctx_create(int device, origin_ctx **out);
int origin_ctx_destroy(origin_ctx *ctx);
int origin_sync(origin_ctx *ctx); /* main stream and, if work is pending there, the aux stream */
/* Work enqueued through an *_async entry point runs on the context's low-priority auxiliary
 * stream, ordered after everything enqueued on the main stream before the call.  Its inputs
 * must stay untouched and its outputs unread until origin_aux_join (the main stream waits for
 * it; no host synchronisation) or origin_sync. */
int origin_aux_join(origin_ctx *ctx);
int origin_device_name(origin_ctx *ctx, char *buf, int buflen);
int origin_mem_info(origin_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
/* the hipStream_t of the context, as an opaque pointer (for interop / RCCL) */
int origin_stream(origin_ctx *ctx, void **stream);

/* origin_free keeps blocks of at least 1 MiB (up to ORIGIN_ALLOC_CACHE_GB, default 96; 0 = off) for
 * the next origin_malloc of their size: the steps of the reference return fresh arrays, and a
 * hipMalloc of a 5 GB cube takes ~40 ms.  Reuse is ordered by the context's streams; origin_mem_info
 * counts the kept blocks as free (they are released when an allocation would fail). */
int origin_malloc(origin_ctx *ctx, size_t bytes, void **d_ptr);
int origin_free(origin_ctx *ctx, void *d_ptr);
int origin_memset(origin_ctx *ctx, void *d_ptr, int byte, size_t bytes);
int origin_h2d(origin_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int origin_d2h(origin_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* Device float32 -> host float64, n elements: the widening the reference's float64 interface
 * needs (cubes leaving through the function seam, steps.py store_cube), chunked through pinned
 * staging and widened by the host worker pool while the next chunk is in flight. */
int origin_d2h_f32_as_f64(origin_ctx *ctx, double *h_dst, const float *d_src, size_t n);
/* The other direction: host float64 -> device float32 (round to nearest even, as
 * ndarray.astype(float32)), narrowed by the host worker pool into pinned staging. */
int origin_h2d_f64_as_f32(origin_ctx *ctx, float *d_dst, const double *h_src, size_t n);
int origin_d2d(origin_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* strided 3-D box copy of `elem`-byte elements between (Nz, Ny, Nx)-shaped arrays; kind:
 * 0 = host->device, 1 = device->host, 2 = device->device.  Pitches in elements.  Used
 * for tile upload/download and halo strips. */
int origin_copy_box(origin_ctx *ctx, int kind, void *dst, long dst_pitch_y, long dst_pitch_z,
                    const void *src, long src_pitch_y, long src_pitch_z, int nz, int ny,
                    int nx, int elem);
/* Spaxel-list moves (csrc/columns.hip): packed[z][i] = cube[z][idx[i]] and back, for `elem`-byte
 * elements (1 or 4) of an (Nz, S) cube and a contiguous (Nz, n) buffer; idx: n int32 spaxel
 * indices on the device, each < S.  What the tiled path exchanges when PCA areas (irregular sets of
 * spaxels, steps.py:492-569) are handed to ranks as wholes: the spaxels a rank's GLR reads around
 * its own (lib_origin.py:1027-1043) are a list, not a rectangle.  Asynchronous on the stream. */
int origin_gather_columns(origin_ctx *ctx, const void *d_cube, int Nz, long S, const int *d_idx,
                          long n, int elem, void *d_packed);
int origin_scatter_columns(origin_ctx *ctx, void *d_cube, int Nz, long S, const int *d_idx, long n,
                           int elem, const void *d_packed);

/* ---- purity threshold reductions -----------------------------------
 * Device side of Compute_threshold_purity (lib_origin.py:1391-1479, called by
 * ComputePurityThreshold.run, steps.py:874-890): the default threshold list needs the
 * per-spaxel maxima of the local-maximum cubes (:1437-1442), the purity curve the number of
 * voxels above each threshold (:1444-1452).  d_keep: uint8 [Ny*Nx] or NULL, 0 = spaxel
 * excluded (cube_local_min * (segmap == 0), :1430). */
int origin_zmax_map(origin_ctx *ctx, const float *d_cube, const uint8_t *d_keep, int Nz, long S,
                    float *d_map /* [S] */);
/* h_counts[t] = #{ voxels : (double) value > h_thr[t] }, thresholds in any order, nthr <= 1024 */
int origin_count_above(origin_ctx *ctx, const float *d_cube, const uint8_t *d_keep, int Nz, long S,
                       int nthr, const double *h_thr, long *h_counts);

/* ---- detection thresholding (the consumer of the local-maximum cubes) -------------------
 * Detection.run, steps.py:956-974 (and det_correl_min, :935-939):
 *     z, y, x = np.where(cube > thr);  T_GLR = cube[z, y, x];  profile = cube_profile[z, y, x]
 * as an ordered stream compaction on the device: positions in C order (z slowest, x fastest, the
 * order np.where returns), compared in float64 (NaN is never above).  d_aux: uint8 cube gathered at
 * the same positions (cube_profile) or NULL.  *h_count receives the TOTAL number of voxels above
 * thr; the first min(cap, total) of them are written to d_z / d_y / d_x (int32) and, where given,
 * d_val (float32) and d_auxout (uint8) -- call again with a larger cap when total > cap; cap = 0
 * only counts.  d_cube must be 16-byte aligned.  Synchronises the stream. */
int origin_where_above(origin_ctx *ctx, const float *d_cube, const uint8_t *d_aux, int Nz, int Ny,
                       int Nx, double thr, long cap, int *d_z, int *d_y, int *d_x, float *d_val,
                       uint8_t *d_auxout, long *h_count);

/* ---- cube statistics (step 9) ----------------------------------------------------------
 * add_tglr_stat opens with np.std(correl) and np.std(std) over the two full host cubes
 * (lib_origin.py:2127-2129, called by CleanResults.run, steps.py:1155-1160).  One streaming pass
 * over a float32 device cube:
 *     h_out = (n, sum(x - shift), sum((x - shift)^2))   over the voxels whose spaxel is kept
 * d_keep: uint8 [S] or NULL, 0 = spaxel excluded (origin_count_above's contract).  Every voxel is
 * widened to float64 before the subtraction; all sums are float64, in a fixed order (no
 * floating-point atomics: the same input gives the same bits on every call).  np.std is two calls:
 * shift = 0 gives the mean, shift = mean gives M2 (origin_amd/kernels.py: cube_std).  d_cube needs
 * float alignment only, S no particular divisor.  Non-finite input propagates as in NumPy.
 * Synchronises the stream. */
int origin_cube_moments(origin_ctx *ctx, const float *d_cube, const uint8_t *d_keep, int Nz, long S,
                        double shift, double *h_out /* [3] */);
/* blocks origin_cube_moments launches for a cube of n_voxels (256 lanes x 4 voxels each per
 * sweep of the grid): a function of the voxel count alone */
int origin_cube_moments_blocks(long n_voxels);

/* ---- FITS data units ------------------------------------------------
 * Step.dump / Step.load (steps.py:301-352) write and reload every cube / image of a step as a
 * FITS image extension through mpdaf (Cube.write(convert_float32=False) -> float64; lazy
 * reload in DataObj.__get__, steps.py:131-160).  A FITS data unit is the array in big-endian
 * byte order, IEEE-754 for BITPIX < 0.  These two calls convert between a device array and
 * the bytes of a data unit (widening / narrowing included), replacing the host-side dtype and
 * byte-order pass of astropy.io.fits; origin_amd/fitsio.py writes the headers around them.
 * element types: 0 = float32, 1 = uint8, 2 = int32, 3 = float64.
 * bitpix: -64, -32, 8, 16, 32, 64.  d_dst of encode / d_src of decode: n * |bitpix| / 8 bytes,
 * 8-byte aligned.  Asynchronous on the context's stream. */
int origin_fits_encode(origin_ctx *ctx, const void *d_src, int src_type, long n, int bitpix,
                       void *d_dst);
int origin_fits_decode(origin_ctx *ctx, const void *d_src, int bitpix, long n, int dst_type,
                       void *d_dst);
/* The same conversions streamed to / from an open file descriptor at its current offset
 * (sequential write() / read()): conversion, PCIe copy through two pinned buffers and file
 * I/O overlap chunk by chunk.  The caller writes the header blocks and the padding of the
 * data unit to a multiple of 2880 bytes.  Both return when the file / the device array is
 * complete. */
int origin_fits_write_data(origin_ctx *ctx, const void *d_src, int src_type, long n, int bitpix,
                           int fd);
int origin_fits_read_data(origin_ctx *ctx, int fd, int bitpix, long n, int dst_type, void *d_dst);

/* ---- step 0: a MUSE cube file becomes cube_raw / var / mask and the white image ----------
 * ORIGIN.__init__ reads the cube through mpdaf (origin.py:210-219), whose Cube masks the voxels
 * where DATA or STAT is not finite, and derives from it (origin.py:262-274, :240)
 *     cube_raw = cube.data.filled(0);  var = cube.var.filled(inf);  mask = cube._mask
 *     ima_white = cube.mean(axis=0)
 * origin_cube_ingest_planes is that pass for `nplanes` consecutive planes whose big-endian file
 * bytes (BITPIX -32 or -64 each; 8-byte aligned) already sit on the device.  Per voxel, with d / s
 * the DATA / STAT value as float32 (-64: rounded, so a value beyond the float32 range is inf):
 *     m = !isfinite(d) || !isfinite(s);  raw = m ? 0 : d;  var = m ? inf : s;  mask = m
 * finite values bit for bit.  d_raw / d_var / d_mask point at the first of the planes.
 * d_white_sum[S] (float64) / d_white_cnt[S] (int32) are running: sum += (double) raw plane after
 * plane in increasing z, cnt += !m -- the plane-by-plane float64 sum of NumPy, however the planes
 * are split into calls.  The caller zeroes both before the first plane (origin_memset).
 * 16-byte accesses where S % 4 == 0 and every pointer is 16-byte aligned (d_mask: 4).
 * Asynchronous on the context's stream. */
int origin_cube_ingest_planes(origin_ctx *ctx, const void *d_data_be, int bitpix_data,
                              const void *d_stat_be, int bitpix_stat, int nplanes, long S,
                              float *d_raw, float *d_var, uint8_t *d_mask, double *d_white_sum,
                              int *d_white_cnt);
/* The same with a DQ unit: `nplanes` planes of big-endian integers, BITPIX 8, 16 or 32, aligned to
 * their element size (the 16-byte form: to four elements).  A voxel whose DQ element is not zero
 * is masked as well:
 *     m = !isfinite(d) || !isfinite(s) || dq != 0
 * and everything after m is as above.  d_dq_be == NULL with bitpix_dq == 0: no DQ unit, which is
 * origin_cube_ingest_planes. */
int origin_cube_ingest_planes_dq(origin_ctx *ctx, const void *d_data_be, int bitpix_data,
                                 const void *d_stat_be, int bitpix_stat, const void *d_dq_be,
                                 int bitpix_dq, int nplanes, long S, float *d_raw, float *d_var,
                                 uint8_t *d_mask, double *d_white_sum, int *d_white_cnt);
/* The same from an open file (replaces the float64 host read of Cube(filename), origin.py:213):
 * pread at the byte offsets of the two data units into two pinned buffers, chunk by chunk a whole
 * number of planes, H2D copy then kernel, file reads overlapping both as in origin_fits_read_data.
 * planes_per_chunk == 0: as many planes as fit 64 MiB of file bytes, at least 1.  Zeroes the sums
 * itself.  A short read gives ORIGIN_E_STATE after the stream has drained.  Returns when the
 * arrays are complete. */
int origin_cube_read(origin_ctx *ctx, int fd, long off_data, int bitpix_data, long off_stat,
                     int bitpix_stat, int Nz, long S, int planes_per_chunk, float *d_raw,
                     float *d_var, uint8_t *d_mask, double *d_white_sum, int *d_white_cnt);
/* Rows [y0, y1) of every plane of a (Nz, Ny, Nx) cube file -- one rank's band of a field cut into
 * bands of whole rows -- by the same loop: one pread per plane and unit at
 * off + ((z * Ny + y0) * Nx) * width, the band's planes packed in the pinned buffer (DATA, STAT,
 * DQ, each section 256-byte aligned), H2D copies, the kernel with S = (y1 - y0) * Nx.  The outputs
 * are band-shaped: (Nz, y1 - y0, Nx) cubes, (y1 - y0, Nx) sums.  off_dq < 0: no DQ unit; otherwise
 * its non-zero elements (bitpix_dq 8, 16 or 32) are masked as in origin_cube_ingest_planes_dq.
 * planes_per_chunk == 0: as many planes as fit 64 MiB of the band's file bytes.  y0 = 0, y1 = Ny
 * without DQ is origin_cube_read. */
int origin_cube_read_rows(origin_ctx *ctx, int fd, long off_data, int bitpix_data, long off_stat,
                          int bitpix_stat, long off_dq, int bitpix_dq, int Nz, int Ny, int Nx,
                          int y0, int y1, int planes_per_chunk, float *d_raw, float *d_var,
                          uint8_t *d_mask, double *d_white_sum, int *d_white_cnt);

/* ---- inter-GPU exchange (one process per GPU; RCCL over xGMI on the context's stream) ----
 * The reference has no multi-GPU path (its only parallelism is the joblib pool of
 * lib_origin.py:1150-1160); these serve the spatial tiling of origin_amd/multigpu.py.
 * librccl.so is opened on first use.  origin_comm_unique_id is called on ONE rank and the
 * ORIGIN_COMM_ID_BYTES blob handed to every rank by any host channel; origin_comm_create is
 * collective.  allreduce / exchange are asynchronous on the context's stream. */
#define ORIGIN_COMM_ID_BYTES 128
typedef struct origin_comm origin_comm;
int origin_comm_unique_id(char *id /* [ORIGIN_COMM_ID_BYTES] */);
int origin_comm_create(origin_ctx *ctx, const char *id, int rank, int world, origin_comm **out);
int origin_comm_destroy(origin_comm *comm);
/* in-place sum over all ranks of n float64 (per-channel sum / count, steps.py:442) */
int origin_comm_allreduce_f64(origin_comm *comm, double *d_buf, long n);
/* grouped point-to-point: contiguous device buffers, sizes in bytes; every rank posts all
 * its receives and sends in one group (halo strips of cube_faint before the GLR) */
int origin_comm_exchange(origin_comm *comm, int nsend, const int *send_peer,
                         const void *const *d_send, const long *send_bytes, int nrecv,
                         const int *recv_peer, void *const *d_recv, const long *recv_bytes);

/* HIP-event timers on the context's stream: slot in [0, 64). */
int origin_timer_start(origin_ctx *ctx, int slot);
int origin_timer_stop(origin_ctx *ctx, int slot);
int origin_timer_ms(origin_ctx *ctx, int slot, float *ms); /* synchronises on the stop */

/* Built-in per-kernel-class profiler: when enabled, every kernel launch of the library is
 * bracketed by HIP events on the context's stream; totals are kept per class
 * (id in [0, origin_prof_count())).  origin_prof_get synchronises on pending events. */
int origin_prof_enable(origin_ctx *ctx, int on);
int origin_prof_reset(origin_ctx *ctx);
int origin_prof_count(void);
int origin_prof_get(origin_ctx *ctx, int id, const char **name, double *total_ms,
                    long *launches);

/* ---- A. DCT continuum + standardisation -------------------------------------------
 * Replaces dct_residual (lib_origin.py:150-240) and the dense lines of
 * Preprocessing.run (steps.py:431-450, :463-465). */

/* Per-spaxel fit of order+1 DCT-II atoms (lib_origin.py:127-146): weighted LSQ
 * D (D^T S^-1 D)^-1 D^T S^-1 s for spaxels without masked voxels (:226-235), plain
 * D D^T s otherwise or when approx != 0 (:191-194, :237).  d_coef: float64 [(order+1)][S]. */
int origin_dct_fit(origin_ctx *ctx, const float *d_raw, const float *d_var,
                   const uint8_t *d_mask, int Nz, int Ny, int Nx, int order, int approx,
                   double *d_coef);
/* origin_dct_fit followed by origin_dct_resid_sums (below), as one call: the per-channel sums
 * of raw over the unmasked spaxels are taken inside the fit's moments pass, which reads raw and
 * mask anyway, so the separate 5 B/voxel plane pass disappears (masked voxels are visited once
 * more, mask bytes only, in the spaxel groups that have any).  Same d_coef, d_zsum, d_zcnt as
 * the two calls (summation order differs: agreement to a few ulp of float64). */
int origin_dct_fit_sums(origin_ctx *ctx, const float *d_raw, const float *d_var,
                        const uint8_t *d_mask, int Nz, int Ny, int Nx, int order, int approx,
                        double *d_coef, double *d_zsum, double *d_zcnt);
/* Continuum cube D c (what dct_residual returns), float32. */
int origin_dct_continuum(origin_ctx *ctx, const double *d_coef, int Nz, int Ny, int Nx,
                         int order, float *d_cont);
/* Per-channel sum and count over unmasked spaxels of (raw - cont): the two halves of
 * nanmean(data, axis=(1,2)) (steps.py:434-442).  d_zsum, d_zcnt: float64 [Nz].  Across
 * GPUs these are all-reduced by the host before origin_dct_standardize. */
int origin_dct_resid_sums(origin_ctx *ctx, const float *d_raw, const uint8_t *d_mask,
                          const double *d_coef, int Nz, int Ny, int Nx, int order,
                          double *d_zsum, double *d_zcnt);
/* cube_std = (raw - cont - zsum/zcnt) / sqrt(var), 0 where masked; cont_dct = cont / sqrt(var)
 * (steps.py:439-446, :463); optional per-spaxel images (may be NULL): ima_std = mean_z
 * cube_std (:450), ima_dct = mean_z cont_dct (:465), o2 = mean_z cube_std^2 (O2test,
 * lib_origin.py:957-974).  d_cont_dct may be NULL. */
int origin_dct_standardize(origin_ctx *ctx, const float *d_raw, const float *d_var,
                           const uint8_t *d_mask, const double *d_coef,
                           const double *d_zsum, const double *d_zcnt, int Nz, int Ny,
                           int Nx, int order, float *d_cube_std, float *d_cont_dct,
                           float *d_ima_std, float *d_ima_dct, double *d_o2);
/* cont_dct (and ima_dct, may be NULL) alone, for callers that pass NULL for both above: nothing
 * downstream of the O2 map waits for the continuum cube, so it can be enqueued after the O2
 * map has been fetched and run while the host fits the thresholds (lib_origin.py:977-1024).
 * Same values as origin_dct_standardize gives. */
int origin_dct_cont_std(origin_ctx *ctx, const float *d_var, const double *d_coef, int Nz, int Ny,
                        int Nx, int order, float *d_cont_dct, float *d_ima_dct);
/* the same on the auxiliary stream (see origin_aux_join): nothing downstream of the O2 map needs
 * cont_dct, so the pass can hide behind the greedy PCA's latency-bound kernels */
int origin_dct_cont_std_async(origin_ctx *ctx, const float *d_var, const double *d_coef, int Nz,
                              int Ny, int Nx, int order, float *d_cont_dct, float *d_ima_dct);

/* ---- B. O2 test and greedy PCA ---------------------------------------------------- */

/* O2test (lib_origin.py:957-974): out[s] = mean_z cube[z, s]^2, float64 [S]. */
int origin_o2(origin_ctx *ctx, const float *d_cube, int Nz, long S, double *d_out);

/* Compute_GreedyPCA_area / Compute_GreedyPCA (lib_origin.py:769-821, :848-954): the whole
 * greedy loop for `na` areas: d_X (float32 (Nz, S), S = Ny*Nx) is cube_std, d_F receives
 * cube_faint; d_X == d_F or d_X == NULL means in place.  All areas advance in lock step,
 * control flow on the device, cube kept in coefficient form F = X - U C until the end.
 *   d_spx      int32 device: concatenated flat spaxel indices s = y*Nx + x of the areas, each
 *              in the column order of cube[:, areamap == i]; h_spx_off: host int64 [na+1].
 *   d_test0    float64 device [S]: O2 test per spaxel (testO2, lib :840) -- not modified.
 *   h_thr      host float64 [na]: thresholds (thresO2).
 *   d_mapO2    int32 device [S]: out, iterations per spaxel (zero outside the areas).
 *   h_nstop    out: number of areas stopped by itermax (:902-905); h_iters (may be NULL):
 *              lock-step iterations executed; h_trace (may be NULL): per iteration
 *              (areas iterating, total nuisance spaxels), int64 [2*trace_cap].
 * Per iteration (lib :899-949): nuisance/background selection (:889-917, including the
 * filtered-index quirk of :908-917), b = mean background (:917), Xp = X - b(b^T X)
 * (:920-923; the division by sum(b^2) at :924 only rescales Xp), G = Xp^T Xp with
 * v_mfma_f64_16x16x4_f64 and its leading eigenvector (repeated squaring on the f64 matrix
 * cores up to 96 columns; above, Lanczos with the matrix resident in the registers and LDS of
 * one CU, converged to a Ritz residual of 1e-14 and verified against G) in place of svds(k=1)
 * (:940), u = Xp v/|Xp v|, F -= u u^T F and the new O2 test (:943-946). */
int origin_pca_run(origin_ctx *ctx, const float *d_X, float *d_F, int Nz, long S, int na,
                   const int *d_spx,
                   const long *h_spx_off, const double *d_test0, const double *h_thr,
                   double noise_pop, int itermax, int *d_mapO2, int *h_nstop, int *h_iters,
                   long *h_trace, int trace_cap);
/* Tail hook of the greedy PCA: `hook(user, n_active, areas)` is called ONCE per run, from inside
 * origin_pca_run / origin_pca_run_into on the calling thread, once at most max_active areas have
 * been iterating for three iterations in a row without their nuisance count falling below 0.6 of
 * what it was at the first of them (stragglers; a run that is about to end does not call).  Before the call the areas that have
 * finished -- they never iterate again -- are written to d_F (the pass they would have had at the
 * end, on the context's stream); `areas` lists the indices of those that go on.  The caller may
 * enqueue the next stage for everything that does not depend on them (origin_glr_run_rows with
 * ORIGIN_GLR_SIDE).  hook = NULL removes it.  Results of the PCA are unchanged. */
int origin_pca_set_tail_hook(origin_ctx *ctx, void (*hook)(void *user, int n_active, const int *areas),
                             void *user, int max_active);
/* The same with cube_faint written into a box of a larger cube: d_F is the box's first element,
 * spaxel y * out_nx + x of the (Nz, S) input goes to d_F[z * out_pz + y * out_py + x].  The tiled
 * path (origin_amd/multigpu.py) points it at the interior of the halo-extended tile the GLR
 * reads, so that no copy stands between the greedy PCA and the halo exchange.  d_X must be a
 * separate contiguous cube.  out_nx == 0: identical to origin_pca_run. */
int origin_pca_run_into(origin_ctx *ctx, const float *d_X, float *d_F, int Nz, long S, int na,
                        const int *d_spx, const long *h_spx_off, const double *d_test0,
                        const double *h_thr, double noise_pop, int itermax, int *d_mapO2,
                        int *h_nstop, int *h_iters, long *h_trace, int trace_cap, int out_nx,
                        long out_py, long out_pz);

/* Pieces of the above exposed for unit tests.  gram: G_a = X_a^T X_a for `nmat` float64
 * matrices X_a ([Nz][ld_a] at d_Xp + xp_off[a], ld_a a multiple of 16); the caller lists the
 * 32x32 upper-triangle tiles (tile_i <= tile_j, matrix tile_a); g_total = sum ld_a^2.
 * eig: leading eigenvector (unit norm) of symmetric PSD matrices G_a (n_a x n_a, row stride
 * ld_a); scratch rows: q_off[a] into a buffer of q_total = sum origin_pca_eig_qrows()*ld_a
 * doubles; d_info (may be NULL): (eigenvalue, Ritz residual, restarts) per matrix. */
int origin_pca_gram(origin_ctx *ctx, const double *d_Xp, const long *d_xp_off, const long *d_ld,
                    int Nz, int ntiles, const int *d_tile_i, const int *d_tile_j,
                    const int *d_tile_a, long g_total, double *d_G, const long *d_g_off);
int origin_pca_eig(origin_ctx *ctx, const double *d_G, const long *d_g_off, const long *d_ld,
                   const long *d_n, int nmat, long q_total, const long *d_q_off, double *d_v,
                   const long *d_v_off, double *d_info);
int origin_pca_eig_qrows(void);

/* Host-only helper of Compute_PCA_threshold (lib_origin.py:999-1002): data > 0, sigma clip
 * (median / std, <= maxiters iterations), np.histogram(bins='fd', density=True).  h_hist gets
 * *nbins values, h_edges *nbins + 1; cap_bins = capacity of h_hist.  No GPU involved. */
int origin_o2_histogram(const double *h_data, long n, double sigclip, int maxiters,
                        double *h_hist, double *h_edges, long cap_bins, long *nbins,
                        long *nkept);

/* the same for `na` areas (values of area a at h_data[h_off[a] .. h_off[a+1])) on host threads;
 * results of area a start at a * (cap_bins + 1) in h_hist / h_edges. */
int origin_o2_histogram_batch(const double *h_data, const long *h_off, int na, double sigclip,
                              int maxiters, double *h_hist, double *h_edges, long cap_bins,
                              long *h_nbins);

/* Gaussian fit of one histogram half (lib_origin.py:1014-1018: astropy LevMarLSQFitter on
 * Gaussian1D = MINPACK lmder, analytic Jacobian, xtol 1e-7, maxfev 100): h_p[3] = (amplitude,
 * mean, stddev), start values in, solution out; *info = MINPACK's termination code. */
int origin_gauss_fit(const double *h_x, const double *h_y, long m, double *h_p, int *info,
                     int *nfev);

/* Threshold of every area from the histograms origin_o2_histogram_batch left (same layout):
 * mode, half-maximum width, bin centres left of mode + fwhm/2, Gaussian fit, thresO2 = mean -
 * stddev * coef with coef = norm.ppf(pfa) (lib_origin.py:1004-1022).  h_res[a] = (thresO2,
 * mean, stddev); h_status[a] = 0 ok, 1 = histogram maximum in the first bin (the reference's
 * argmin over an empty slice raises), 2 = fewer than three bins to fit.  Host threads only. */
int origin_o2_threshold_batch(const double *h_hist, const double *h_edges, const long *h_nbins,
                              int na, long cap_bins, double coef, double *h_res, int *h_status);

/* ComputePCAThreshold.run for every area in one pass over the host worker pool (steps.py:610-631,
 * lib_origin.py:977-1024): gather the area's O2 values from the map (h_map float64 [S]; h_idx =
 * concatenated flat spaxel indices, area a at [h_off[a], h_off[a+1])) into h_data (the
 * reference's testO2, same layout), then origin_o2_histogram and the threshold fit of
 * origin_o2_threshold_batch.  Outputs as those two; h_status[a] = 3 if the histogram failed. */
int origin_o2_areas_fit(const double *h_map, const int *h_idx, const long *h_off, int na,
                        double sigclip, int maxiters, double coef, double *h_data, double *h_hist,
                        double *h_edges, long cap_bins, long *h_nbins, double *h_res,
                        int *h_status);

/* ---- C. GLR correlation ------------------------------------------------------------
 * Replaces Correlation_GLR_test (lib_origin.py:1070-1217) and the dense lines of
 * ComputeTGLR.run (steps.py:781-793).
 *
 * A plan owns device copies of the zero-mean PSFs k_fz = PSF_fz - mean (lib :1033-1034),
 * the optional field weights, the prepared profiles (trimmed / normalised / mean
 * subtracted by the host exactly as lib :1155-1165) and the derived normalisation
 * tables.  h_psf: float64 [nfields][Nz][P][P] (P odd, as the reference holds them);
 * h_weights: float64 [nfields][Ny][Nx] or NULL (weights=None); h_taps: float64
 * concatenated taps of the K prepared profiles, h_tap_off: int [K+1]. */
int origin_glr_plan_create(origin_ctx *ctx, int Nz, int Ny, int Nx, int nfields, int P,
                           const double *h_psf, const double *h_weights, int K,
                           const double *h_taps, const int *h_tap_off,
                           origin_glr_plan **out);
int origin_glr_plan_destroy(origin_glr_plan *plan);
/* bytes of device memory the plan holds */
/* Arithmetic of the GLR stages when the plan is eligible for the matrix cores: 1 (default) =
 * two-term f16 split of data and taps, three MFMAs per product, fp32 accumulation (~3e-7 of
 * sum |p x| from float64: fp32 class); 2 = bf16 operands, one MFMA per product (BASELINE config 4
 * "bf16 GLR"; |dT| ~1e-2); 0 = fp32 FMA chain (~1e-7).  Eligible: the spatial stage for odd PSF
 * sizes 5..41 (27..41: three k-steps per window row, one block per CU for the f16 split; one
 * field, or a mosaic of weighted fields: per-field accumulation); the spectral
 * stage for profile half widths <= 32 and K <= 26 -- through the border-class table without
 * weight maps, through the plan's norm cube with them (that cube, [Nz + 96][Ny][Nx] float32, is
 * allocated with the plan and filled by its first run or by origin_glr_plan_prepare): the FOLD form where the cube is smooth along z
 * (origin_glr_plan_fold_eps; precision 1 or 2), else a second Toeplitz product (precision 1 only).
 * A stage that is not eligible runs the fp32 kernels; plans where neither stage is (a field
 * smaller than the PSF without weight maps, longer / more profiles) always report 0.  get
 * returns the plan's setting. */
int origin_glr_plan_set_precision(origin_glr_plan *plan, int precision);
int origin_glr_plan_get_precision(origin_glr_plan *plan, int *precision);
int origin_glr_plan_bytes(origin_glr_plan *plan, size_t *bytes);
/* Matrix-core instructions (v_mfma_f32_32x32x16_{f16,bf16}: 32768 flop each) ONE run of the plan
 * issues in its spatial / spectral stage -- what rocprofv3's SQ_INSTS_MFMA counts per launch
 * (partial edge tiles included); 0 for a stage that runs the fp32 kernels or the weighted forms.
 * bench.py prices `roofline.executed` with it (measurement). */
int origin_glr_plan_mfma_count(origin_glr_plan *plan, long *spatial, long *spectral);
/* FOLD of the matrix-core spectral stage (plans without weight maps): away from the cube's first
 * and last 32 channels 1/sqrt(den_k[z]) = a_k s(z) (1 + e_k(z)) with a_k = 1/sqrt(sum p_k^2) and s
 * a factor of the spaxel's border class alone; *eps = the plan's max |e| (measured on its own
 * tables at creation; +inf for plans the stage does not serve).  Where eps <= 2e-6 (and K <= 24)
 * the stage compares the profiles through accumulators that carry a_k and applies s(z) to the
 * maximum and the minimum (*active = 1): correl and correl_min carry a relative error <= eps, the
 * profile index is that of a maximum up to the same eps.
 * Plans with weight maps (an explicit norm cube): den_k[z, s] = norm[z, s] sum p_k^2 (1 + e)^2; eps
 * is measured by the first run or by prepare (origin_glr_plan_prepare) on the norm cube either
 * makes (+inf and inactive before), and
 * where it passes the stage is the same FOLD kernel with rsq(norm) of each voxel behind the loop
 * instead of a second Toeplitz product (the 32 channels at either end keep the two-product
 * kernel); bf16 plans included.
 * ORIGIN_GLR_NO_FOLD=1 in the environment runs the exact form everywhere. */
int origin_glr_plan_fold_eps(origin_glr_plan *plan, float *eps, int *active);
/* What a plan with weight maps (an explicit norm cube) owes before the form of its spectral stage is
 * known, done now instead of inside its first run: the norm cube (PSFs and weight maps only), then
 * eps of the FOLD form measured on it.  On the context's main stream; the eps read-back
 * synchronises it, so call it where a wait is harmless -- never from a PCA tail hook.  Idempotent;
 * nothing to do for plans without a norm cube.  origin_glr_run calls it itself; row bands and
 * rectangles (origin_glr_run_rows) need it called first. */
int origin_glr_plan_prepare(origin_ctx *ctx, origin_glr_plan *plan);
/* The same arithmetic without a plan or a device (host only: num_cu compute units, `terms` = 3
 * for the f16 split, 1 for bf16; n_narrow = profiles of half width <= 16): lets the CPU tests
 * check bench.py's `executed` against the counter passes committed under profiles/. */
int origin_glr_mfma_count_model(int num_cu, int terms, int K, int n_narrow, int Nz, int Ny, int Nx,
                                int P, long *spatial, long *spectral);
/* Which kernels the plan's next run takes, as the run itself decides it (read only; a weighted
 * plan answers for the FOLD verdict it has now, which its first run measures): *spatial_mfma = 1
 * if the spatial stage runs on the matrix cores; *spectral = the form of the spectral stage,
 * 0 table, 1 normw, 2 norm_mfma (matrix cores), 3 packed, 4 fp32, 5 generic (fp32 FMA kernels,
 * csrc/glr_fp32.hip); *lwt = the register-window half width of the packed form's tap rows (8, 16,
 * 24, 29 or 32; 0: half widths above 32), *lwmax = the largest profile half width, *nborder = the
 * spaxels within P/2 of the field's border (0 for a plan with a norm cube).  The tests use it to
 * assert the kernel they were written for. */
int origin_glr_plan_paths(origin_glr_plan *plan, int *spatial_mfma, int *spectral, int *lwt,
                          int *lwmax, int *nborder);

/* A GLR run in ROW BANDS: the same results as origin_glr_run, written band by band -- so that the
 * bands whose input is final can start while the greedy PCA still iterates over its last areas
 * (origin_pca_set_tail_hook).  A band is the rows [y0, y1) of the field, y0 a multiple of 64, y1 a
 * multiple of 64 or Ny; its spatial stage reads cube rows [y0 - P/2, y1 + P/2).  flags:
 * ORIGIN_GLR_FIRST on the first band of a run (zeroes the pad channels of the work cube, on the main
 * stream), ORIGIN_GLR_SIDE to enqueue the band on the context's side stream (all compute units but
 * ORIGIN_GLR_SIDE_RESERVE, default an eighth of them; it starts behind everything the main stream was given before
 * the call).  origin_glr_run_finish makes the main stream wait for the side bands and writes the
 * maps (NULL: none).  Only plans whose two stages run on the matrix cores (precision 1 or 2, odd
 * PSF 5..41, profile half widths <= 32, K <= 26): one field without weight maps (the table kernel),
 * or a mosaic of weighted fields AFTER origin_glr_plan_prepare -- the FOLD form on the norm cube
 * where its eps passes, the two-product kernel otherwise (precision 1); a band never makes the
 * norm cube or measures eps (that synchronises the stream).  origin_glr_rows_supported tells: 0
 * for a weighted plan that is not prepared, whose bf16 eps test failed or that runs the fp32
 * kernels.  Others return ORIGIN_E_STATE (naming origin_glr_plan_prepare where that is what is
 * missing). */
#define ORIGIN_GLR_FIRST 1
#define ORIGIN_GLR_SIDE 2
int origin_glr_rows_supported(origin_glr_plan *plan, int *ok);
int origin_glr_run_rows(origin_ctx *ctx, origin_glr_plan *plan, const float *d_cube,
                        const uint8_t *d_mask, float *d_work, float *d_correl, uint8_t *d_profile,
                        float *d_correl_min, int y0, int y1, int flags);
/* The same for a RECTANGLE of the field: rows [y0, y1), columns [x0, x1), each a multiple of 64 or
 * the field's end (origin_glr_run_rows = all columns).  A tile of a tiled field runs the rectangles
 * that stay clear of its halo while the halo strips are on their way (origin_amd/multigpu.py).
 * With x0 > 0 or x1 < Nx a wave of the spectral stage holds 32 columns of ONE row (rows are not
 * multiples of 32 long in general): results agree with origin_glr_run to rounding, not bit for bit. */
int origin_glr_run_rect(origin_ctx *ctx, origin_glr_plan *plan, const float *d_cube,
                        const uint8_t *d_mask, float *d_work, float *d_correl, uint8_t *d_profile,
                        float *d_correl_min, int y0, int y1, int x0, int x1, int flags);
int origin_glr_run_finish(origin_ctx *ctx, origin_glr_plan *plan, float *d_work, float *d_maxmap,
                          float *d_minmap);

/* correl = max_k T_k, profile = first argmax_k, correl_min = min_k T_k (lib :1205-1212).
 * If d_mask != NULL the ComputeTGLR glue is fused: correl[mask] = 0, profile[mask] = 0
 * (steps.py:781, :788) before maxmap = amax_z correl, minmap = amin_z correl_min (:792-793).
 * d_maxmap / d_minmap may be NULL.  d_work: float32 workspace of
 * origin_glr_work_elems(plan) elements. */
int origin_glr_work_elems(origin_glr_plan *plan, size_t *elems);
int origin_glr_run(origin_ctx *ctx, origin_glr_plan *plan, const float *d_cube,
                   const uint8_t *d_mask, float *d_work, float *d_correl,
                   uint8_t *d_profile, float *d_correl_min, float *d_maxmap,
                   float *d_minmap);

/* ---- D. local maxima ---------------------------------------------------------------
 * compute_local_max (lib_origin.py:1220-1256): size^3 maximum_filter (scipy 'reflect'
 * border == clamped window for a max), keep voxels equal to their window maximum and
 * not masked, zero elsewhere; same on -correl_min. */
int origin_local_max(origin_ctx *ctx, const float *d_correl, const float *d_correl_min,
                     const uint8_t *d_mask, int Nz, int Ny, int Nx, int size,
                     float *d_local_max, float *d_local_min);

/* Sparse form of the same pass (size 3, Nx % 4 == 0): the two cubes are > 98 % zeros, and the
 * consumers of cube_local_max / cube_local_min (Compute_threshold_purity lib_origin.py:1391-1479,
 * Detection.run steps.py:935-974) only ever count or pick the non-zero voxels.  Instead of two
 * dense float32 cubes (8 of the pass's 17 B per voxel) the pass appends (linear index z*Ny*Nx +
 * y*Nx + x, value) of every non-zero output to per-wave segments: segment w of `seg_cap` entries
 * starts at w * seg_cap in idx / val, counts[w] (maxima of correl) and counts[nseg + w] (maxima of
 * -correl_min) say how many it holds.  A count above seg_cap means the segment overflowed (entries
 * beyond it were dropped): use the dense form.  origin_local_max_sparse_plan gives nseg and seg_cap
 * for a shape (nseg 0: no sparse form for it); order inside and across segments is the march order
 * of the waves, not np.where's -- consumers that need an order sort what they keep.  The values are
 * bit for bit those of origin_local_max. */
int origin_local_max_sparse_plan(origin_ctx *ctx, int Nz, int Ny, int Nx, long *nseg, int *seg_cap);
int origin_local_max_sparse(origin_ctx *ctx, const float *d_correl, const float *d_correl_min,
                            const uint8_t *d_mask, int Nz, int Ny, int Nx, long nseg, int seg_cap,
                            long long *d_idx_max, float *d_val_max, long long *d_idx_min,
                            float *d_val_min, int *d_counts);
/* consumers: the dense cube of n voxels (zeros + entries); counts above each of nthr thresholds
 * (origin_count_above's contract; keep: uint8 per spaxel, 0 = excluded, or NULL); the entries
 * above a threshold in no particular order (the first `cap`; *h_count = how many there are; aux:
 * a uint8 cube gathered at the hits, or NULL); per-spaxel maximum over z, 0 where a column has no
 * positive entry (the dense cube's columns always hold zeros). */
int origin_sparse_to_dense(origin_ctx *ctx, const long long *d_idx, const float *d_val,
                           const int *d_counts, long nseg, int seg_cap, float *d_dense, long n);
int origin_sparse_count_above(origin_ctx *ctx, const long long *d_idx, const float *d_val,
                              const int *d_counts, long nseg, int seg_cap, const uint8_t *d_keep,
                              long S, int nthr, const double *h_thr, long *h_counts);
int origin_sparse_where_above(origin_ctx *ctx, const long long *d_idx, const float *d_val,
                              const int *d_counts, long nseg, int seg_cap, double threshold,
                              const uint8_t *d_aux, long cap, long long *d_out_idx,
                              float *d_out_val, uint8_t *d_out_aux, long *h_count);
int origin_sparse_zmax_map(origin_ctx *ctx, const long long *d_idx, const float *d_val,
                           const int *d_counts, long nseg, int seg_cap, const uint8_t *d_keep,
                           long S, float *d_map);

/* ---- E. line estimation -------------------------------------------------------------
 * estimation_line (lib_origin.py:1805-1938, called by ComputeSpectra.run, steps.py:1082-1096)
 * with GridAnalysis (:1620-1790), method_PCA_wgt (:1535-1617), LS_deconv_wgt (:1482-1510),
 * conv_wgt (:1513-1532) and peakdet (:1793-1801), for `ndet` detections in batches sized from
 * origin_mem_info (max_problems > 0: at most that many (detection, grid offset) problems per
 * batch, whole detections; results do not depend on it).  float64 after the gather.
 *   d_raw, d_var  float32 device cubes (Nz, Ny, Nx);
 *   h_psf         float64 [nfields][Nz][P][P] (P odd, <= 41); h_weights float64 [nfields][Ny][Nx]
 *                 or NULL (weights=None).  With weights the PSF of a problem is sum_n w_n[window]
 *                 psf_n[z] (:1713-1717) and size_grid must be 0;
 *   h_det         int32 [ndet][3]: z0, y0, x0, inside the cube;
 *   size_grid     0..5; criteria 0 = 'flux', 1 = 'mse'; order_dct -1 = None (PCA LS only);
 *   h_line, h_var float64 [ndet][Nz]: estimated line / variance of the winning grid offset;
 *   h_flux5, h_mse5 float64 [ndet]; h_yxz int32 [ndet][3]: y, x, z; h_status int32 [ndet]: 1 =
 *                 the fallback row (0.0, 1e6, [0], [0], y0, x0, z0) of :1760-1769 (line / var
 *                 zero), given where every grid offset is degenerate or the criterion is not finite;
 *   h_nbatch      (may be NULL) batches run.
 * Deviations from the reference: a window with a non-finite raw value, a
 * var that is NaN or <= 0, or a channel whose sum psf^2/var is 0 never reaches the eigen-solver
 * (fallback row instead of ARPACK on NaN); grid offsets outside the field do not compete; the
 * first best offset wins a tie.  Synchronises. */
int origin_lines_estimate(origin_ctx *ctx, const float *d_raw, const float *d_var, int Nz, int Ny,
                          int Nx, int nfields, int P, const double *h_psf, const double *h_weights,
                          int ndet, const int *h_det, int size_grid, int criteria, int order_dct,
                          int horiz_psf, int horiz, int max_problems, double *h_line, double *h_var,
                          double *h_flux5, double *h_mse5, int *h_yxz, int *h_status,
                          int *h_nbatch);
/* Pieces of the above exposed for unit tests.  gather: the standardised, centred work matrices of
 * :1575-1579 for `nprob` windows centred at h_centres (int32 [nprob][2]: y, x; any position, the
 * part outside the field is data 0 / var +inf, :1884-1888): d_A float64 [nprob][Nz][ld], ld = P*P
 * rounded up to 16, slack columns zero; d_mean float64 [nprob][Nz] the row means that were
 * subtracted; d_flag int32 [nprob]: 1 = degenerate (matrix and means zero).
 * select: the grid analysis of :1693-1790 on given deconvolutions: h_deconv / h_varest float64
 * [nprob][Nz] and h_flag int32 [nprob] for the problems of the detections in order -- per
 * detection its grid offsets inside the field, dy major (np.where order); outputs as above. */
int origin_lines_gather(origin_ctx *ctx, const float *d_raw, const float *d_var, int Nz, int Ny,
                        int Nx, int nfields, int P, const double *h_psf, const double *h_weights,
                        int nprob, const int *h_centres, double *d_A, double *d_mean, int *d_flag);
int origin_lines_select(origin_ctx *ctx, const float *d_raw, int Nz, int Ny, int Nx, int nfields,
                        int P, const double *h_psf, const double *h_weights, int ndet,
                        const int *h_det, int size_grid, int criteria, int horiz_psf, int horiz,
                        const double *h_deconv, const double *h_varest, const int *h_flag,
                        double *h_line, double *h_var, double *h_flux5, double *h_mse5, int *h_yxz,
                        int *h_status);

/* ---- F. spatio-spectral merging ------------------------------------------------------
 * spatiospectral_merging with itersrc (lib_origin.py:1259-1387, called by Detection.run,
 * steps.py:1014) for n detections given as host arrays in table order.
 *   h_x, h_y, h_z  int32 [n] inside the (Nz, Ny, Nx) cube; h_area int32 [n] segmap labels;
 *   h_near, h_far  uint8 [R][R] over (|dx|, |dy|), R <= 64: np.hypot(dx, dy) < tol_spat and
 *                  np.hypot(dx, dy) > tol_spat * np.sqrt(2) as NumPy evaluates them; outside the
 *                  tables nothing is near and everything is far.  h_near[0] must be set;
 *   dzmax          ceil(tol_spec) - 1: |dz| < tol_spec is |dz| <= dzmax;
 *   h_comp         (may be NULL) lowest row of the row's connected component of the near graph;
 *   h_area_out     the largest area label of the row's group; h_imatch2 / h_imatch the 0-based
 *                  group id before / after the spectral stage; all int32 [n] in input row order
 *                  (the reference returns its table sorted by imatch).
 * No floating point on the device; results are the same from run to run.  n = 0 is valid.
 * Synchronises. */
int origin_merge_detections(origin_ctx *ctx, long n, const int *h_x, const int *h_y,
                            const int *h_z, const int *h_area, int Ny, int Nx, int Nz, int R,
                            const uint8_t *h_near, const uint8_t *h_far, int dzmax, int *h_comp,
                            int *h_area_out, int *h_imatch2, int *h_imatch);

/* ---- G. segmentation maps ------------------------------------------------------------
 * compute_segmap_gauss (lib_origin.py:243-280, called by Preprocessing.run, steps.py:473 and :481,
 * and by ComputePurityThreshold.run, steps.py:862) behind its threshold fit, and the label of the
 * union of two label maps (steps.py:487, :869): DESIGN.md section 3k.  Comparisons and integer
 * work only; every result is bit-identical to the reference's.
 *
 * origin_segmap_mask: the mask of lib_origin.py:268-278 for a float64 device map (Ny, Nx):
 *   stage 1  map > gamma, compared in float64 (NaN and -inf are 0)                        (:268)
 *   stage 2  + binary_erosion, 4-neighbour cross, pixels outside the image count as 1     (:269)
 *   stage 3  + binary_dilation, same cross, outside counts as 0                           (:270)
 *   stage 4  + the disc of :273-278 when f >= 0: f = int(fwhm_fsf) // 2, a pixel is set where the
 *            stage-3 mask has a pixel at an integer offset with dy^2 + dx^2 < f^2 (outside: 0).
 *            That is fftconvolve(mask, disc, 'same') > 1e-9 evaluated directly: the convolution
 *            is an integer count and the FFT's error is ~1e-15.  f = 0 gives the empty mask, f = 1
 *            the identity; f is not capped.  f < 0: no disc (fwhm_fsf <= 0), the stage-3 mask.
 * d_mask: uint8 [Ny*Nx], 0 / 1.  The stages below 4 exist for the unit tests.  Asynchronous.
 * origin_segmap_union: d_mask[i] = d_a[i] > 0 || d_b[i] > 0 for two int32 label maps of n pixels
 * (the argument of ndi.label at steps.py:487, :869).  Asynchronous.
 * origin_segmap_label: scipy.ndimage.label(mask)[0] with the default 4-connected structure (:280):
 * int32 labels 1..n in raster order of each component's first pixel, 0 for background; *h_n = n.
 * Ny * Nx < 2^30.  No workgroup waits for another; the labels are the same from run to run.
 * Synchronises. */
int origin_segmap_mask(origin_ctx *ctx, const double *d_map, int Ny, int Nx, double gamma, int f,
                       int stage, uint8_t *d_mask);
int origin_segmap_union(origin_ctx *ctx, const int *d_a, const int *d_b, long n, uint8_t *d_mask);
int origin_segmap_label(origin_ctx *ctx, const uint8_t *d_mask, int Ny, int Nx, int *d_labels,
                        int *h_n);
/* host-only geometry of the labeller: a workgroup builds the components of one tw x th tile; the
 * roots of more than origin_label_scan_span() pixels are counted in more than one pass of the
 * scan's one workgroup.  The tests derive their shapes from these. */
int origin_label_tile(int *tw, int *th);
int origin_label_scan_span(void);

/* ---- H. matching of point lists ------------------------------------------------------
 * "Which points of A have a point of B within r, and the other way round" for two host tables:
 * what the reference asks of two cKDTrees and query_ball_tree in compute_true_purity
 * (lib_origin.py:2383-2399, once per threshold) and in Detection.run (steps.py:983-992): DESIGN.md
 * section 3l.
 *   h_ax, h_ay, h_az  float64 [n] host columns of A; h_bx, h_by, h_bz float64 [m] those of B;
 *   r                 finite, >= 0;
 *   h_aval            (may be NULL) float32 [n], a value per point of A, no NaN;
 *   h_a_hit           (may be NULL) uint8 [n]: 1 where some B_j has d2(A_i, B_j) <= r*r;
 *   h_b_hit           (may be NULL) uint8 [m]: the same, seen from B;
 *   h_b_max           (may be NULL; needs h_aval) float32 [m]: the largest h_aval[i] over the A_i
 *                     within r of B_j, -inf where there is none (-0 orders below +0).
 * The predicate is part of the interface: with dx = ax - bx, dy = ay - by, dz = az - bz,
 *   d2 = (dx*dx + dy*dy) + dz*dz <= r*r
 * where every difference, product and sum is one separately rounded float64 operation in exactly
 * this order (no fused multiply-add) and r*r is one rounded product made once on the host.  This
 * is what NumPy computes for the same expression, so the outputs can be compared bit for bit.
 * ORIGIN_E_ARG with a message for: a coordinate that is not finite, r negative or not finite,
 * h_b_max without h_aval, a NaN in h_aval.  n == 0 or m == 0 launches nothing and fills the outputs
 * (zeros, -inf).  The outputs do not depend on the order in which lanes arrive (integer atomicOr /
 * atomicMax): they are the same from run to run, and a permutation of B's rows permutes h_b_hit /
 * h_b_max and nothing else.  Synchronises. */
int origin_ball_match(origin_ctx *ctx, long n, const double *h_ax, const double *h_ay,
                      const double *h_az, const float *h_aval, long m, const double *h_bx,
                      const double *h_by, const double *h_bz, double r, uint8_t *h_a_hit,
                      uint8_t *h_b_hit, float *h_b_max);

#ifdef __cplusplus
}
#endif
#endif /* ORIGIN_HIP_H */
