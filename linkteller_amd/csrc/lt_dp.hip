// LapGraph cell selection on the device (reference worker.py:302-335).
//
// The reference adds an N x N Laplace noise matrix (strict lower triangle) to the adjacency and keeps the n_keep largest
// cells, with a 50-way np.argpartition over the flattened float64 matrix.  The noise itself has to stay numpy's (a given
// --noise-seed must give the reference's graph), so the host draws it and uploads it; everything after the draw runs here:
//   k_lap_add_edges   cell(i, j) += 1.0 for the edges j < i            (the fp64 add of worker.py:299, same rounding)
//   k_lap_hist        one radix pass of a top-k SELECT over the order-preserving 64-bit keys of the cells j < i: histogram
//                     of the next 8 bits among the cells whose higher bits match the prefix found so far
//   k_lap_pick        walks the 256 bins from the top and fixes the next 8 bits of the threshold (no host round trip)
//   k_lap_collect     cells above the threshold, then as many cells EQUAL to it as are still missing
// The selected SET is what np.argpartition returns whenever the n_keep-th largest value is not tied (continuous noise:
// ties occur with probability zero; cells of the upper triangle are exact zeros in the reference and are never reached
// because n_keep is far below the number of positive cells -- a threshold <= 0 is refused, the reference asserts there).
#include <string.h>

#include "lt_internal.h"

// order-preserving map double -> uint64 (larger double <=> larger key)
__device__ __forceinline__ unsigned long long lap_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__global__ void k_lap_add_edges(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                double *__restrict__ cells) {
    const int i = blockIdx.x;
    for (int e = rowptr[i] + threadIdx.x; e < rowptr[i + 1]; e += blockDim.x) {
        const int j = col[e];
        if (j < i) cells[(size_t)i * n + j] += 1.0;
    }
}

// state[0] = prefix (the bits of the threshold key fixed so far, in place), state[1] = cells still to take inside the prefix
// bucket, state[2] = output cursor.  `shift` = position of the digit this pass histograms (56, 48, ..., 0).
__global__ __launch_bounds__(256) void k_lap_hist(int n, const double *__restrict__ cells, int shift,
                                                  const unsigned long long *__restrict__ state,
                                                  unsigned *__restrict__ hist) {
    __shared__ unsigned sh[256];
    sh[threadIdx.x] = 0;
    __syncthreads();
    const unsigned long long prefix = state[0];
    const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    for (int i = blockIdx.x + 1; i < n; i += gridDim.x) {          // row i holds the cells j < i
        const double *row = cells + (size_t)i * n;
        for (int j = threadIdx.x; j < i; j += 256) {
            const unsigned long long k = lap_key(row[j]);
            if ((k & himask) == (prefix & himask)) atomicAdd(&sh[(unsigned)(k >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sh[threadIdx.x]);
}

__global__ void k_lap_pick(int shift, unsigned long long *__restrict__ state, unsigned *__restrict__ hist) {
    // single thread: 256 bins
    unsigned long long need = state[1];
    int d = 255;
    for (; d > 0; --d) {
        const unsigned c = hist[d];
        if (c >= need) break;
        need -= c;
    }
    state[0] |= (unsigned long long)d << shift;
    state[1] = need;                       // cells to take among those whose key matches the prefix so far
    for (int i = 0; i < 256; ++i) hist[i] = 0;
}

__global__ __launch_bounds__(256) void k_lap_collect(int n, const double *__restrict__ cells,
                                                     unsigned long long *__restrict__ state, long long k_total,
                                                     long long *__restrict__ out, int pass) {
    const unsigned long long thr = state[0];
    for (int i = blockIdx.x + 1; i < n; i += gridDim.x) {
        const double *row = cells + (size_t)i * n;
        for (int j = threadIdx.x; j < i; j += 256) {
            const unsigned long long k = lap_key(row[j]);
            if (pass == 0 ? k > thr : k == thr) {
                const unsigned long long p = atomicAdd(&state[2], 1ull);
                if ((long long)p < k_total) out[p] = (long long)i * n + j;
            }
        }
    }
}

// cells: [n, n] float64 on the device, holding the noise (only j < i is read); overwritten with adjacency + noise.
// lower_rowptr / lower_col: device CSR of the adjacency (any entries with j >= i are ignored).  out_idx: [n_keep] int64
// on the device, the flat indices i * n + j of the selected cells in no particular order.  work: >= 4096 bytes of
// device scratch.  threshold_out (host, optional): the n_keep-th largest cell value.  Synchronises (it returns a value).
extern "C" int lt_lapgraph_select(int32_t n, const int32_t *lower_rowptr, const int32_t *lower_col, double *cells,
                                  int64_t n_keep, int64_t *out_idx, void *work, size_t work_bytes,
                                  double *threshold_out, void *stream) {
    LT_REQUIRE(n > 1 && lower_rowptr && lower_col && cells && out_idx && work, "lt_lapgraph_select: NULL argument or n < 2");
    LT_REQUIRE(work_bytes >= 4096 && ((uintptr_t)work % 8) == 0, "lt_lapgraph_select: work needs 4096 bytes, 8-byte aligned");
    const long long total = (long long)n * (n - 1) / 2;
    LT_REQUIRE(n_keep > 0 && n_keep <= total, "lt_lapgraph_select: n_keep=%lld outside [1, %lld]", (long long)n_keep, total);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *state = (unsigned long long *)work;          // [0] prefix, [1] remaining, [2] cursor
    unsigned *hist = (unsigned *)((char *)work + 64);                // 256 bins
    LT_HIP(hipMemsetAsync(work, 0, 4096, st));
    const unsigned long long init[3] = {0ull, (unsigned long long)n_keep, 0ull};
    LT_HIP(hipMemcpyAsync(state, init, sizeof(init), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_lap_add_edges, dim3((unsigned)n), dim3(64), 0, st, n, lower_rowptr, lower_col, cells);
    LT_CHECK_LAUNCH();
    const unsigned grid = (unsigned)(n - 1 < 4096 ? n - 1 : 4096);
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_lap_hist, dim3(grid), dim3(256), 0, st, n, cells, shift, state, hist);
        hipLaunchKernelGGL(k_lap_pick, dim3(1), dim3(1), 0, st, shift, state, hist);
        LT_CHECK_LAUNCH();
    }
    // state[0] = key of the n_keep-th largest cell, state[1] = how many cells equal to it belong to the selection
    hipLaunchKernelGGL(k_lap_collect, dim3(grid), dim3(256), 0, st, n, cells, state, (long long)n_keep, (long long *)out_idx, 0);
    hipLaunchKernelGGL(k_lap_collect, dim3(grid), dim3(256), 0, st, n, cells, state, (long long)n_keep, (long long *)out_idx, 1);
    LT_CHECK_LAUNCH();
    unsigned long long fin[3];
    LT_HIP(hipMemcpyAsync(fin, state, sizeof(fin), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    unsigned long long u = fin[0];
    u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    double thr;
    memcpy(&thr, &u, sizeof(thr));
    if (threshold_out) *threshold_out = thr;
    if (!(thr > 0.0))
        return lt_set_error(LT_ERR_UNSUPPORTED, "lt_lapgraph_select: the %lld-th largest cell is %g <= 0: the selection would reach "
                                                "the zero cells of the upper triangle (the reference asserts there, worker.py:326)",
                            (long long)n_keep, thr);
    if ((long long)fin[2] < n_keep)
        return lt_set_error(LT_ERR_INVALID, "lt_lapgraph_select: collected %llu of %lld cells", fin[2], (long long)n_keep);
    return LT_OK;
}

// =====================================================================================================================
// The Philox cell stream (include/linkteller_hip.h, "edge-DP noise from a counter-based stream"): LapGraph and EdgeRand
// without an N x N matrix.  Cell (i, j), j < i, has the linear index t = i (i - 1) / 2 + j; cells 2q and 2q + 1 share the
// Philox block with counter (q lo, q hi, stream, 0).  The noise is evaluated where it is needed and never stored:
//   k_phx_flat<0>     LapGraph, the streaming pass: a grid-stride loop over the Philox blocks of a row range.  The rank key
//                     of a non-edge cell is g(k), non-decreasing in the cell's 52-bit integer k, so "key >= key_min" is the
//                     integer test k >= k_min with k_min found once on the host (phx_k_min): no fp64 work per cell.  A hit
//                     (rare: the caller asks for a few times n_keep of the n (n - 1) / 2 cells) recovers (i, j) from t by
//                     an integer square root and is dropped if the adjacency holds it, by a binary search in row i --
//   k_phx_edges       -- because the edge cells, whose key carries the factor c = exp(eps2), are evaluated by this second
//                     kernel over the CSR entries j < i, a wave per row.
//   k_phx_flat<1>     EdgeRand: the same loop over stream 2, a hit is k < floor(s 2^52); reports the cell and its coin.
// All three append through a wave-aggregated cursor (one atomic per wave and cell slot with a hit); the cursor keeps
// counting past the capacity, nothing is written there.
//   lt_lapgraph_philox  chooses key_min from the closed-form tail of the key distribution, scans into a candidate buffer of
//                     3 n_keep + 4096 entries, rescans with a moved key_min when fewer than n_keep or more than the buffer
//                     came back, then selects exactly: k_phx_hist / k_phx_pick, eight digit passes over the key bits and
//                     eight over the complemented cell index among the cells tied at the threshold key (the total order is
//                     key descending, then cell ascending), and k_phx_collect.
// =====================================================================================================================
#include <math.h>

#include "lt_philox.hip.h"

#define PHX_BLOCK 256
#define PHX_MAX_BLOCKS 2048     // 256 CUs x 8 blocks of 4 waves
#define PHX_K_END (1ull << 52)  // one past the largest k

// cells in front of row i
__host__ __device__ static inline unsigned long long phx_tri(unsigned long long i) { return i ? i * (i - 1) / 2 : 0ull; }

// the rank key of a non-edge cell from its 52-bit integer: u = (2k + 1) 2^-53 (exact), g = 2u below one half, else
// 1 / (2 (1 - u)); every step but the divide is exact, the divide is correctly rounded
__host__ __device__ static inline double phx_g(unsigned long long k) {
    const double u = (double)(2 * k + 1) * 0x1p-53;
    return k < (1ull << 51) ? 2.0 * u : 1.0 / (2.0 * (1.0 - u));
}

// smallest k with phx_g(k) >= key_min (PHX_K_END: none); phx_g is non-decreasing
static unsigned long long phx_k_min(double key_min) {
    unsigned long long lo = 0, hi = PHX_K_END;
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (phx_g(mid) >= key_min) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// row and column of cell t
__device__ __forceinline__ void phx_row_col(unsigned long long t, unsigned long long &i, unsigned long long &j) {
    unsigned long long r = (unsigned long long)sqrt(2.0 * (double)t);     // i - 1 .. i + 1
    if (r < 1) r = 1;
    while (phx_tri(r) > t) --r;
    while (phx_tri(r + 1) <= t) ++r;
    i = r;
    j = t - phx_tri(r);
}

// one atomic for the hits of a wave: returns this lane's position (valid where `hit`).  Every lane of the wave calls it.
__device__ __forceinline__ unsigned long long phx_wave_claim(bool hit, unsigned long long *count) {
    const unsigned long long m = __ballot(hit);
    if (!m) return 0;
    const unsigned lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(m));
    const unsigned lo = __shfl((unsigned)base, leader), hi = __shfl((unsigned)(base >> 32), leader);
    return (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// MODE 0: the non-edge cells of LapGraph's stream 0 with k >= k_thr; MODE 1: EdgeRand's stream 2, cells with k < k_thr.
// Cells [t0, t1), t0 < t1.  The loop bounds are the same for the 64 lanes of a wave (the ballots need whole waves).
template <int MODE>
__global__ __launch_bounds__(PHX_BLOCK) void k_phx_flat(int n, unsigned long long t0, unsigned long long t1,
                                                        const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                        uint2 key, unsigned long long k_thr, long long *__restrict__ out_cell,
                                                        double *__restrict__ out_key, unsigned char *__restrict__ out_coin,
                                                        long long cap, unsigned long long *count) {
    const unsigned long long q0 = t0 >> 1, nq = ((t1 - 1) >> 1) - q0 + 1;
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long stride = (unsigned long long)gridDim.x * PHX_BLOCK;
    for (unsigned long long base = (unsigned long long)blockIdx.x * PHX_BLOCK + (threadIdx.x & ~63u); base < nq; base += stride) {
        const bool live = base + lane < nq;
        const unsigned long long q = q0 + base + lane;
        const uint4 w = lt_philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), MODE ? 2u : 0u, 0u), key);
        const unsigned long long k0 = ((unsigned long long)w.x << 20) | (w.y >> 12);
        const unsigned long long k1 = ((unsigned long long)w.z << 20) | (w.w >> 12);
        const bool in0 = live && 2 * q >= t0, in1 = live && 2 * q + 1 < t1;     // 2q < t1 and 2q + 1 >= t0 hold for every live q
        const bool h0 = in0 && (MODE ? k0 < k_thr : k0 >= k_thr);
        const bool h1 = in1 && (MODE ? k1 < k_thr : k1 >= k_thr);
        if (!__ballot(h0 || h1)) continue;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            bool h = c ? h1 : h0;
            const unsigned long long k = c ? k1 : k0;
            long long cell = 0;
            if (h) {
                unsigned long long i, j;
                phx_row_col(2 * q + c, i, j);
                if (MODE == 0) {       // an edge cell belongs to k_phx_edges
                    int a = rowptr[i], b = rowptr[i + 1];
                    while (a < b) {
                        const int mid = a + ((b - a) >> 1);
                        if ((unsigned long long)col[mid] < j) a = mid + 1; else b = mid;
                    }
                    if (a < rowptr[i + 1] && (unsigned long long)col[a] == j) h = false;
                }
                cell = (long long)(i * (unsigned long long)n + j);
            }
            const unsigned long long pos = phx_wave_claim(h, count);
            if (h && pos < (unsigned long long)cap) {
                out_cell[pos] = cell;
                if (MODE == 0) out_key[pos] = phx_g(k);
                else out_coin[pos] = (unsigned char)((c ? w.w : w.y) & 1u);
            }
        }
    }
}

// the edge cells (i, j), j < i, of rows [row_begin, row_end): key = g c.  A wave per row, 64 entries a trip.
__global__ __launch_bounds__(PHX_BLOCK) void k_phx_edges(int row_begin, int row_end, int n, const int32_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ col, uint2 key, double c, double key_min,
                                                         long long *__restrict__ out_cell, double *__restrict__ out_key,
                                                         long long cap, unsigned long long *count) {
    const unsigned lane = threadIdx.x & 63u;
    const long long wave = ((long long)blockIdx.x * PHX_BLOCK + threadIdx.x) >> 6, n_waves = (long long)gridDim.x * (PHX_BLOCK / 64);
    for (long long i = row_begin + wave; i < row_end; i += n_waves) {
        const int e0 = rowptr[i], e1 = rowptr[i + 1];
        for (int eb = e0; eb < e1; eb += 64) {
            const int e = eb + (int)lane;
            bool h = false;
            long long cell = 0;
            double v = 0.0;
            if (e < e1) {
                const long long j = col[e];
                if (j >= 0 && j < i) {
                    const unsigned long long t = phx_tri((unsigned long long)i) + (unsigned long long)j, q = t >> 1;
                    const uint4 w = lt_philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), 0u, 0u), key);
                    const unsigned long long k = (t & 1) ? ((unsigned long long)w.z << 20) | (w.w >> 12)
                                                         : ((unsigned long long)w.x << 20) | (w.y >> 12);
                    v = phx_g(k) * c;
                    h = v >= key_min;
                    cell = i * n + j;
                }
            }
            const unsigned long long pos = phx_wave_claim(h, count);
            if (h && pos < (unsigned long long)cap) {
                out_cell[pos] = cell;
                out_key[pos] = v;
            }
        }
    }
}

static unsigned phx_flat_grid(unsigned long long t0, unsigned long long t1) {
    const unsigned long long nq = ((t1 - 1) >> 1) - (t0 >> 1) + 1, blocks = (nq + PHX_BLOCK - 1) / PHX_BLOCK;
    return (unsigned)(blocks < PHX_MAX_BLOCKS ? blocks : PHX_MAX_BLOCKS);
}

// clears *d_count and enqueues the two kernels of a LapGraph scan (arguments checked by the callers)
static int phx_scan_launch(int32_t n, int32_t row_begin, int32_t row_end, const int32_t *d_rowptr, const int32_t *d_col, uint64_t seed,
                           double edge_factor, double key_min, int64_t *out_cell, double *out_key, int64_t capacity,
                           int64_t *d_count, hipStream_t st) {
    LT_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
    const unsigned long long t0 = phx_tri((unsigned long long)row_begin), t1 = phx_tri((unsigned long long)row_end);
    if (t0 >= t1) return LT_OK;
    const uint2 key = make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
    const unsigned long long k_thr = phx_k_min(key_min);
    if (k_thr < PHX_K_END) {
        hipLaunchKernelGGL(k_phx_flat<0>, dim3(phx_flat_grid(t0, t1)), dim3(PHX_BLOCK), 0, st, n, t0, t1, d_rowptr, d_col, key, k_thr,
                           (long long *)out_cell, out_key, (unsigned char *)nullptr, (long long)capacity, (unsigned long long *)d_count);
        LT_CHECK_LAUNCH();
    }
    const int rows = row_end - row_begin, blocks = (rows + PHX_BLOCK / 64 - 1) / (PHX_BLOCK / 64);
    hipLaunchKernelGGL(k_phx_edges, dim3((unsigned)(blocks < PHX_MAX_BLOCKS ? blocks : PHX_MAX_BLOCKS)), dim3(PHX_BLOCK), 0, st, row_begin,
                       row_end, n, d_rowptr, d_col, key, edge_factor, key_min, (long long *)out_cell, out_key, (long long)capacity,
                       (unsigned long long *)d_count);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_philox_cells_scan(int32_t n, int32_t row_begin, int32_t row_end, const int32_t *d_rowptr, const int32_t *d_col,
                                    uint64_t seed, double edge_factor, double key_min, int64_t *out_cell, double *out_key,
                                    int64_t capacity, int64_t *d_count, void *stream) {
    LT_REQUIRE(n > 1 && d_rowptr && d_col && out_cell && out_key && d_count, "lt_philox_cells_scan: NULL argument or n < 2");
    LT_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n, "lt_philox_cells_scan: rows [%d, %d) outside 0 <= row_begin <= row_end <= %d",
               row_begin, row_end, n);
    LT_REQUIRE(capacity >= 0, "lt_philox_cells_scan: capacity=%lld is negative", (long long)capacity);
    LT_REQUIRE(edge_factor >= 0.0 && isfinite(edge_factor) && key_min >= 0.0, "lt_philox_cells_scan: edge_factor=%g must be finite and >= 0, key_min=%g >= 0",
               edge_factor, key_min);
    return phx_scan_launch(n, row_begin, row_end, d_rowptr, d_col, seed, edge_factor, key_min, out_cell, out_key, capacity, d_count,
                           (hipStream_t)stream);
}

extern "C" int lt_edgerand_philox(int32_t n, int32_t row_begin, int32_t row_end, uint64_t seed, uint64_t s_threshold, int64_t *out_cell,
                                  uint8_t *out_coin, int64_t capacity, int64_t *d_count, void *stream) {
    LT_REQUIRE(n > 1 && out_cell && out_coin && d_count, "lt_edgerand_philox: NULL argument or n < 2");
    LT_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n, "lt_edgerand_philox: rows [%d, %d) outside 0 <= row_begin <= row_end <= %d",
               row_begin, row_end, n);
    LT_REQUIRE(capacity >= 0, "lt_edgerand_philox: capacity=%lld is negative", (long long)capacity);
    LT_REQUIRE(s_threshold <= PHX_K_END, "lt_edgerand_philox: s_threshold=%llu above 2^52", (unsigned long long)s_threshold);
    hipStream_t st = (hipStream_t)stream;
    LT_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
    const unsigned long long t0 = phx_tri((unsigned long long)row_begin), t1 = phx_tri((unsigned long long)row_end);
    if (t0 >= t1 || s_threshold == 0) return LT_OK;
    hipLaunchKernelGGL(k_phx_flat<1>, dim3(phx_flat_grid(t0, t1)), dim3(PHX_BLOCK), 0, st, n, t0, t1, (const int32_t *)nullptr,
                       (const int32_t *)nullptr, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)), (unsigned long long)s_threshold,
                       (long long *)out_cell, (double *)nullptr, (unsigned char *)out_coin, (long long)capacity, (unsigned long long *)d_count);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- the exact selection among the candidates -------------------------------------------------------------------------------
// state (uint64): [0] the threshold key's bits fixed so far, [1] cells still to take inside that prefix, [2] / [3] the same for
// the complemented cell index among the cells tied at the threshold key, [4] output cursor, [5] cells above the threshold key,
// [6] cells tied at it, [7] the scan's counter.  Passes 0 .. 7 fix the key, 8 .. 15 the index; keys are >= +0.0, so their
// bit patterns order as the values do.
#define PHX_HEADER_BYTES 4096
#define PHX_HIST_OFFSET 512

__global__ __launch_bounds__(256) void k_phx_hist(const unsigned long long *__restrict__ keys, const long long *__restrict__ cells,
                                                  unsigned long long cnt, int pass, const unsigned long long *__restrict__ state,
                                                  unsigned long long *__restrict__ hist) {
    __shared__ unsigned sh[256];
    sh[threadIdx.x] = 0;
    __syncthreads();
    const int second = pass >> 3, shift = 56 - 8 * (pass & 7);
    const unsigned long long prefix = state[second ? 2 : 0], thr = state[0];
    const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
    for (unsigned long long x = (unsigned long long)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (unsigned long long)gridDim.x * 256) {
        const unsigned long long kb = keys[x];
        if (second && kb != thr) continue;
        const unsigned long long v = second ? ~(unsigned long long)cells[x] : kb;
        if ((v & himask) == (prefix & himask)) atomicAdd(&sh[(unsigned)(v >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (sh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)sh[threadIdx.x]);
}

__global__ void k_phx_pick(int pass, unsigned long long n_keep, unsigned long long *__restrict__ state, unsigned long long *__restrict__ hist) {
    const int second = pass >> 3, shift = 56 - 8 * (pass & 7);
    unsigned long long need = state[second ? 3 : 1];
    int d = 255;
    for (; d > 0; --d) {
        const unsigned long long c = hist[d];
        if (c >= need) break;
        need -= c;
    }
    state[second ? 2 : 0] |= (unsigned long long)d << shift;
    state[second ? 3 : 1] = need;
    if (pass == 7) {       // the key is whole: `need` of the hist[d] cells tied at it belong to the selection
        state[3] = need;
        state[5] = n_keep - need;
        state[6] = hist[d];
    }
    for (int i = 0; i < 256; ++i) hist[i] = 0;
}

__global__ __launch_bounds__(256) void k_phx_collect(const unsigned long long *__restrict__ keys, const long long *__restrict__ cells,
                                                     unsigned long long cnt, unsigned long long n_keep, unsigned long long *__restrict__ state,
                                                     long long *__restrict__ out) {
    const unsigned long long thr = state[0], last = state[2];
    for (unsigned long long x = (unsigned long long)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (unsigned long long)gridDim.x * 256) {
        const unsigned long long kb = keys[x];
        const long long cell = cells[x];
        if (kb > thr || (kb == thr && ~(unsigned long long)cell >= last)) {
            const unsigned long long p = atomicAdd(&state[4], 1ull);
            if (p < n_keep) out[p] = cell;
        }
    }
}

static int64_t phx_capacity(int64_t n_keep) { return 3 * n_keep + 4096; }
#define PHX_MAX_KEEP ((int64_t)1 << 56)     // 16-byte candidates: the workspace stays below 2^62 bytes

extern "C" int lt_lapgraph_philox_workspace(int32_t n, int64_t nnz, int64_t n_keep, size_t *bytes) {
    LT_REQUIRE(bytes, "lt_lapgraph_philox_workspace: NULL argument");
    *bytes = 0;
    LT_REQUIRE(n > 1 && nnz >= 0, "lt_lapgraph_philox_workspace: n=%d < 2 or nnz=%lld < 0", n, (long long)nnz);
    const long long total = (long long)n * (n - 1) / 2;
    LT_REQUIRE(n_keep > 0 && n_keep <= total && n_keep < PHX_MAX_KEEP, "lt_lapgraph_philox_workspace: n_keep=%lld outside [1, %lld]",
               (long long)n_keep, total);
    *bytes = PHX_HEADER_BYTES + (size_t)phx_capacity(n_keep) * 16;
    return LT_OK;
}

// share of the non-edge keys that are >= x
static double phx_tail(double x) { return x <= 0.0 ? 1.0 : x < 1.0 ? 1.0 - 0.5 * x : 0.5 / x; }

// the largest key_min at which about `target` cells are expected: bisection over the bit patterns of the non-negative doubles
static double phx_model_key_min(double cells_plain, double cells_edge, double c, double target) {
    uint64_t lo = 0, hi = 0x7ff0000000000000ull;       // expected(lo) >= target > expected(hi) = 0
    if (cells_plain + cells_edge <= target) return 0.0;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        double x;
        memcpy(&x, &mid, sizeof(x));
        const double expect = cells_plain * phx_tail(x) + cells_edge * (c > 0.0 ? phx_tail(x / c) : 0.0);
        if (expect >= target) lo = mid; else hi = mid;
    }
    double x;
    memcpy(&x, &lo, sizeof(x));
    return x;
}

extern "C" int lt_lapgraph_philox(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, uint64_t seed, double edge_factor,
                                  int64_t n_keep, double key_hint, int64_t *out_idx, int64_t *info, void *ws, size_t ws_bytes,
                                  void *stream) {
    LT_REQUIRE(n > 1 && d_rowptr && d_col && out_idx && info && ws, "lt_lapgraph_philox: NULL argument or n < 2");
    const long long total = (long long)n * (n - 1) / 2;
    LT_REQUIRE(n_keep > 0 && n_keep <= total && n_keep < PHX_MAX_KEEP, "lt_lapgraph_philox: n_keep=%lld outside [1, %lld]", (long long)n_keep, total);
    LT_REQUIRE(edge_factor >= 0.0 && isfinite(edge_factor), "lt_lapgraph_philox: edge_factor=%g must be finite and >= 0", edge_factor);
    const int64_t cap = phx_capacity(n_keep);
    LT_REQUIRE(ws_bytes >= PHX_HEADER_BYTES + (size_t)cap * 16 && ((uintptr_t)ws % 8) == 0,
               "lt_lapgraph_philox: workspace needs %zu bytes (lt_lapgraph_philox_workspace), 8-byte aligned", PHX_HEADER_BYTES + (size_t)cap * 16);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *state = (unsigned long long *)ws;
    unsigned long long *hist = (unsigned long long *)((char *)ws + PHX_HIST_OFFSET);
    int64_t *cand_cell = (int64_t *)((char *)ws + PHX_HEADER_BYTES);
    double *cand_key = (double *)(cand_cell + cap);
    int64_t *d_count = (int64_t *)&state[7];

    int32_t nnz = 0;
    LT_HIP(hipMemcpyAsync(&nnz, d_rowptr + n, sizeof(nnz), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    LT_REQUIRE(nnz >= 0, "lt_lapgraph_philox: rowptr[n]=%d is negative", nnz);
    // a symmetric adjacency holds each edge twice, once below the diagonal; the estimate only steers the first key_min
    const double edges = 0.5 * nnz < (double)total ? 0.5 * nnz : (double)total;
    const double target = 1.5 * (double)n_keep + 64.0;
    const double model = phx_model_key_min((double)total - edges, edges, edge_factor, target);

    // lo: a key_min known to report >= n_keep cells (0 reports them all), hi: one known to report fewer
    uint64_t lo = 0, hi = 0x7ff0000000000001ull;
    double x = key_hint > 0.0 ? key_hint : model;
    bool hinted = key_hint > 0.0;
    int64_t cnt = 0;
    int passes = 0;
    for (;;) {
        ++passes;
        int rc = phx_scan_launch(n, 0, n, d_rowptr, d_col, seed, edge_factor, x, cand_cell, cand_key, cap, d_count, st);
        if (rc != LT_OK) return rc;
        LT_HIP(hipMemcpyAsync(&cnt, d_count, sizeof(cnt), hipMemcpyDeviceToHost, st));
        LT_HIP(hipStreamSynchronize(st));
        if (cnt >= n_keep && cnt <= cap) break;
        uint64_t xb;
        memcpy(&xb, &x, sizeof(xb));
        if (cnt > cap) lo = xb; else hi = xb;
        if (hi - lo <= 1)
            return lt_set_error(LT_ERR_UNSUPPORTED, "lt_lapgraph_philox: %lld cells share the key %g around the %lld-th largest: more than "
                                "the candidate buffer of %lld holds", (long long)cnt, x, (long long)n_keep, (long long)cap);
        // the tail is ~ 1 / x: scale by the count seen; from the sixth pass on (or outside the bracket) bisect the bit patterns
        double next = hinted ? model : (passes < 6 && cnt > 0) ? x * ((double)cnt / target) : -1.0;
        hinted = false;
        uint64_t nb = 0;
        if (next >= 0.0) memcpy(&nb, &next, sizeof(nb));
        if (!(next >= 0.0) || nb <= lo || nb >= hi) nb = lo + (hi - lo) / 2;
        memcpy(&x, &nb, sizeof(x));
    }

    LT_HIP(hipMemsetAsync(ws, 0, PHX_HEADER_BYTES, st));
    const unsigned long long init[2] = {0ull, (unsigned long long)n_keep};
    LT_HIP(hipMemcpyAsync(state, init, sizeof(init), hipMemcpyHostToDevice, st));
    const unsigned long long blocks = ((unsigned long long)cnt + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
    for (int pass = 0; pass < 16; ++pass) {
        hipLaunchKernelGGL(k_phx_hist, dim3(grid), dim3(256), 0, st, (const unsigned long long *)cand_key, (const long long *)cand_cell,
                           (unsigned long long)cnt, pass, state, hist);
        hipLaunchKernelGGL(k_phx_pick, dim3(1), dim3(1), 0, st, pass, (unsigned long long)n_keep, state, hist);
        LT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_phx_collect, dim3(grid), dim3(256), 0, st, (const unsigned long long *)cand_key, (const long long *)cand_cell,
                       (unsigned long long)cnt, (unsigned long long)n_keep, state, (long long *)out_idx);
    LT_CHECK_LAUNCH();
    unsigned long long fin[8];
    LT_HIP(hipMemcpyAsync(fin, state, sizeof(fin), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    uint64_t xb;
    memcpy(&xb, &x, sizeof(xb));
    info[0] = (int64_t)fin[0];
    info[1] = cnt;
    info[2] = passes;
    info[3] = (int64_t)fin[5];
    info[4] = n_keep - (int64_t)fin[5];
    info[5] = (int64_t)fin[6];
    info[6] = (int64_t)xb;
    info[7] = 0;
    if ((long long)fin[4] != n_keep)
        return lt_set_error(LT_ERR_INVALID, "lt_lapgraph_philox: collected %llu of %lld cells", fin[4], (long long)n_keep);
    return LT_OK;
}
