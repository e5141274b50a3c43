// The baseline attacks' scores on the device (reference attacker.py:287-375, LSA2-post / LSA2-attr): the correlation of mean-centred
// rows of an fp32 matrix V [n, ldv],
//     corr(u, v) = <x_u - m, x_v - m> / ||x_u - m|| / ||x_v - m||,
// as a k x k square over a node sample (m = the column mean over the k listed rows) or as a list of pairs (m = the column mean
// over all n rows).  fp32 inputs are widened exactly; the mean, the centring, every product and every sum are fp64; ONE rounding
// to fp32 happens at the store.  No floating-point atomics: every sum has one fixed order, two calls give equal bits.
//
//   k_corr_colsum       rows in a FIXED partition (corr_parts(rows): a function of the row count alone); one thread per column adds
//                       its partition's rows in row order.  Block column 0 of a partition also counts its bad node ids.
//   k_corr_mean         mean[c] = (part[0][c] + part[1][c] + ...) / valid rows, partition order.
//   k_corr_gram         SYRK on v_mfma_f64_16x16x4_f64: one block per (lower 64 x 64 tile, K slice).  Rows V[nodes[i]] are gathered,
//                       widened and centred while the operands are staged into LDS -- no k x D fp64 copy of the centred rows exists.
//                       The K tail (D % 16 of the last step) is zero in LDS, never read from memory.  K slices: corr_slices(k, D),
//                       a function of (k, D) alone; each slice writes its own 64 x 64 partial.
//   k_corr_finish       one block per lower tile: the slices' partials are added in slice order; the norms are the square roots of
//                       the reduced Gram's own diagonal; s = g / n_i / n_j is rounded once into an LDS tile and stored at (i, j)
//                       AND (j, i), both as row segments: the square is symmetric bit for bit.  Diagonal tiles compute their
//                       lower half only.
//   k_corr_rownorm      (pair lists) ||x_r - m|| for all n rows: a wave per row for D > 64, eight lanes per row below.
//   k_corr_pairs        (pair lists) a wave per pair for D > 64, eight lanes per pair below (posteriors have 2 .. 7 columns).
// A node id outside [0, n) is never used as an address: its row is staged as zeros, its cells are NaN, info[1] counts it (and the
// square's mean is taken over the valid listed rows).  A row whose centred vector is zero has norm 0: its cells are NaN, info[0]
// counts it.
#include <math.h>

#include "lt_internal.h"

namespace {

typedef double cr_f64x4 __attribute__((ext_vector_type(4)));

constexpr int CR_BM = 64;            // tile edge (rows of the sample)
constexpr int CR_BK = 16;            // columns of V per staging step
constexpr int CR_LD = CR_BK + 1;     // LDS row stride in doubles (odd: the 16 rows a fragment read touches land in distinct banks)
constexpr int CR_TILE = CR_BM * CR_BM;
constexpr int CR_TARGET_BLOCKS = 512;      // (tile, slice) blocks the split aims at: two per CU
constexpr int CR_MAX_SLICES = 16;
constexpr int CR_PART_ROWS = 32;           // rows per column-sum partition, at least
constexpr int CR_MAX_PARTS = 1024;         // beyond CR_PART_ROWS * this many rows the partitions grow instead of their number
constexpr int CR_PACK = 8;                 // lanes per row / per pair on the packed route
constexpr int CR_PACK_MAX_D = 64;          // D <= this: the packed route

struct corr_part_plan { int parts, rows_per; };
corr_part_plan corr_parts(long rows) {
    corr_part_plan p;
    long per = (rows + CR_MAX_PARTS - 1) / CR_MAX_PARTS;
    if (per < CR_PART_ROWS) per = CR_PART_ROWS;
    p.rows_per = (int)per;
    p.parts = rows > 0 ? (int)((rows + per - 1) / per) : 0;
    return p;
}

struct corr_slice_plan { int tiles_edge, slices, steps_per; long tiles; };
corr_slice_plan corr_slices(int k, int D) {
    corr_slice_plan p;
    p.tiles_edge = (k + CR_BM - 1) / CR_BM;
    p.tiles = (long)p.tiles_edge * (p.tiles_edge + 1) / 2;
    const int steps = (D + CR_BK - 1) / CR_BK;
    long want = p.tiles > 0 ? (CR_TARGET_BLOCKS + p.tiles - 1) / p.tiles : 1;
    if (want > CR_MAX_SLICES) want = CR_MAX_SLICES;
    if (want > steps) want = steps;
    if (want < 1) want = 1;
    p.steps_per = (int)((steps + want - 1) / want);
    if (p.steps_per < 1) p.steps_per = 1;
    p.slices = (steps + p.steps_per - 1) / p.steps_per;      // (no empty slice; the last one may be shorter)
    if (p.slices < 1) p.slices = 1;
    return p;
}

size_t corr_round2(size_t words) { return (words + 1) & ~(size_t)1; }
size_t corr_square_words(int D, int k) {
    if (k <= 0) return 0;
    const corr_part_plan pp = corr_parts(k);
    const corr_slice_plan sp = corr_slices(k, D);
    return corr_round2((size_t)D) + corr_round2((size_t)pp.parts * D) + (size_t)sp.slices * sp.tiles * CR_TILE;
}
size_t corr_pairs_words(int n, int D, long m) {
    if (m <= 0) return 0;
    const corr_part_plan pp = corr_parts(n);
    return corr_round2((size_t)D) + corr_round2((size_t)pp.parts * D) + (size_t)n;
}

// ---- (a) column sums ---------------------------------------------------------------------------------------------------------------
// grid (ceil(D / 256), parts).  nodes == NULL: row r of the partition is row r of V.
__global__ __launch_bounds__(256) void k_corr_colsum(const float *__restrict__ V, long ldv, int n, int D,
                                                     const int32_t *__restrict__ nodes, int rows, int rows_per,
                                                     double *__restrict__ part, unsigned long long *__restrict__ info) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int r0 = blockIdx.y * rows_per;
    const int r1 = r0 + rows_per < rows ? r0 + rows_per : rows;
    if (nodes && blockIdx.x == 0) {
        int bad = 0;
        for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) {
            const int id = nodes[r];
            bad += (id < 0 || id >= n) ? 1 : 0;
        }
        if (bad) atomicAdd(&info[1], (unsigned long long)bad);       // (an integer count: order does not show)
    }
    if (c >= D) return;
    double acc = 0.0;
    for (int r = r0; r < r1; ++r) {
        const int id = nodes ? nodes[r] : r;
        if (id < 0 || id >= n) continue;
        acc += (double)V[(size_t)id * ldv + c];
    }
    part[(size_t)blockIdx.y * D + c] = acc;
}

// bad_from_info: the valid rows are rows - info[1] (the square); else all rows count (the pair lists)
__global__ __launch_bounds__(256) void k_corr_mean(const double *__restrict__ part, int parts, int D, long rows, int bad_from_info,
                                                   const unsigned long long *__restrict__ info, double *__restrict__ mean) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    double acc = 0.0;
    for (int p = 0; p < parts; ++p) acc += part[(size_t)p * D + c];
    const long valid = rows - (bad_from_info ? (long)info[1] : 0);
    mean[c] = acc / (double)valid;
}

// ---- (b) the Gram of the centred rows ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void corr_tile_of(long t, int *ti, int *tj) {
    // t = ti (ti + 1) / 2 + tj, tj <= ti
    long i = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (i * (i + 1) / 2 > t) --i;
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    *ti = (int)i;
    *tj = (int)(t - i * (i + 1) / 2);
}

// grid: tiles * slices blocks, block b = slice * tiles + tile.  gram[(slice * tiles + tile) * 4096 + r * 64 + c].
__global__ __launch_bounds__(256) void k_corr_gram(const float *__restrict__ V, long ldv, int n, int D,
                                                   const int32_t *__restrict__ nodes, int k, const double *__restrict__ mean,
                                                   long tiles, int steps_per, double *__restrict__ gram) {
    __shared__ double As[CR_BM * CR_LD];
    __shared__ double Bs[CR_BM * CR_LD];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const long tile = (long)blockIdx.x % tiles;
    const int slice = (int)((long)blockIdx.x / tiles);
    int ti, tj;
    corr_tile_of(tile, &ti, &tj);
    const int steps = (D + CR_BK - 1) / CR_BK;
    const int s0 = slice * steps_per;
    const int s1 = s0 + steps_per < steps ? s0 + steps_per : steps;
    // staging: thread -> row tid >> 2 of both tiles, columns (tid & 3) * 4 .. + 3 of the step
    const int a_row = tid >> 2, a_col = (tid & 3) * 4;
    const int gi = ti * CR_BM + a_row, gj = tj * CR_BM + a_row;
    int id_i = gi < k ? nodes[gi] : -1, id_j = gj < k ? nodes[gj] : -1;
    if (id_i < 0 || id_i >= n) id_i = -1;
    if (id_j < 0 || id_j >= n) id_j = -1;
    const float *pa = V + (size_t)(id_i < 0 ? 0 : id_i) * ldv;
    const float *pb = V + (size_t)(id_j < 0 ? 0 : id_j) * ldv;
    const int a_frag = (wr * 32 + (lane & 15)) * CR_LD + (lane >> 4);
    const int b_frag = (wc * 32 + (lane & 15)) * CR_LD + (lane >> 4);
    cr_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = cr_f64x4{0.0, 0.0, 0.0, 0.0};
    double ra[4], rb[4];
    // a step's operands: widened, centred; columns >= D (the K tail) and rows without a valid node stay zero, nothing is loaded
    auto stage = [&](int step) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = step * CR_BK + a_col + j;
            ra[j] = 0.0;
            rb[j] = 0.0;
            if (c < D) {
                const double mc = mean[c];
                if (id_i >= 0) ra[j] = (double)pa[c] - mc;
                if (id_j >= 0) rb[j] = (double)pb[c] - mc;
            }
        }
    };
    if (s0 < s1) stage(s0);
    for (int step = s0; step < s1; ++step) {
        __syncthreads();      // the previous step's fragment reads are done
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            As[a_row * CR_LD + a_col + j] = ra[j];
            Bs[a_row * CR_LD + a_col + j] = rb[j];
        }
        __syncthreads();
        if (step + 1 < s1) stage(step + 1);      // the next step's loads fly under this step's MFMAs
#pragma unroll
        for (int kk = 0; kk < CR_BK; kk += 4) {
            // A operand: lane holds A[row lane & 15][k = lane >> 4]; B operand: B[k = lane >> 4][col lane & 15] = d_j[col][k]
            const double a0 = As[a_frag + kk], a1 = As[a_frag + 16 * CR_LD + kk];
            const double b0 = Bs[b_frag + kk], b1 = Bs[b_frag + 16 * CR_LD + kk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    // f64 C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg.  The whole 64 x 64 partial is written (pad rows hold zeros).
    double *dst = gram + ((size_t)slice * tiles + tile) * CR_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = wc * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = wr * 32 + i * 16 + (lane >> 4) + 4 * reg;
                dst[r * CR_BM + c] = acc[i][j][reg];
            }
        }
}

// ---- (c) finish: slices in order, norms from the diagonal, divide, round once, store and mirror ------------------------------------------
__global__ __launch_bounds__(256) void k_corr_finish(const double *__restrict__ gram, long tiles, int slices, int n,
                                                     const int32_t *__restrict__ nodes, int k, float *__restrict__ out, long ldo,
                                                     unsigned long long *__restrict__ info) {
    __shared__ double nrm[2 * CR_BM];      // [0, 64): rows of tile ti, [64, 128): rows of tile tj; NaN marks a bad node id
    const int tid = threadIdx.x;
    int ti, tj;
    corr_tile_of((long)blockIdx.x, &ti, &tj);
    if (tid < 2 * CR_BM) {
        const int tt = tid < CR_BM ? ti : tj, r = tid & (CR_BM - 1);
        const int g = tt * CR_BM + r;
        double v = nan("");
        if (g < k) {
            const int id = nodes[g];
            if (id >= 0 && id < n) {
                const long td = (long)tt * (tt + 1) / 2 + tt;
                double d = 0.0;
                for (int s = 0; s < slices; ++s) d += gram[((size_t)s * tiles + td) * CR_TILE + r * CR_BM + r];
                v = sqrt(d);
                if (ti == tj && tid < CR_BM && v == 0.0) atomicAdd(&info[0], 1ull);      // (each row once: its diagonal tile)
            }
        }
        nrm[tid] = v;
    }
    __syncthreads();
    // the rounded tile goes through LDS so that the cell AND its mirror leave as row segments (a mirror stored straight from the
    // registers put consecutive lanes ldo floats apart: 2 M scattered 4-byte stores at k = 2000)
    __shared__ float tile[CR_BM * (CR_BM + 1)];
    const size_t t0 = (size_t)blockIdx.x * CR_TILE;
    for (int e = tid; e < CR_TILE; e += 256) {
        const int r = e >> 6, c = e & 63;
        const int gi = ti * CR_BM + r, gj = tj * CR_BM + c;
        if (gi >= k || gj >= k || (ti == tj && c > r)) continue;
        double g = 0.0;
        for (int s = 0; s < slices; ++s) g += gram[(size_t)s * tiles * CR_TILE + t0 + e];
        const double ni = nrm[r], nj = nrm[CR_BM + c];
        float v;
        if (ni != ni || nj != nj || ni == 0.0 || nj == 0.0) v = __uint_as_float(0x7fc00000u);
        else v = (float)(g / ni / nj);
        tile[r * (CR_BM + 1) + c] = v;
        if (ti == tj) tile[c * (CR_BM + 1) + r] = v;      // a diagonal tile's upper half: the very same bits
    }
    __syncthreads();
    for (int e = tid; e < CR_TILE; e += 256) {
        const int r = e >> 6, c = e & 63;      // lanes along c: a row segment of out in both stores
        const int gi = ti * CR_BM + r, gj = tj * CR_BM + c;
        if (gi < k && gj < k) out[(size_t)gi * ldo + gj] = tile[r * (CR_BM + 1) + c];
        if (ti != tj) {                        // the mirror tile: row tj * 64 + r, column ti * 64 + c, the very same bits
            const int mi = tj * CR_BM + r, mj = ti * CR_BM + c;
            if (mi < k && mj < k) out[(size_t)mi * ldo + mj] = tile[c * (CR_BM + 1) + r];
        }
    }
}

// ---- (d) pair lists ------------------------------------------------------------------------------------------------------------------
// G lanes share one row / one pair: lane `sub` of the group adds columns sub, sub + G, ... in order, then a butterfly over the group.
template <int G>
__device__ __forceinline__ double corr_group_sum(double v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G>
__global__ __launch_bounds__(256) void k_corr_rownorm(const float *__restrict__ V, long ldv, int n, int D,
                                                      const double *__restrict__ mean, double *__restrict__ norm) {
    const long item = ((long)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = item < n;                       // (whole groups: every lane of a group agrees)
    double acc = 0.0;
    if (live) {
        const float *p = V + (size_t)item * ldv;
        for (int c = sub; c < D; c += G) {
            const double d = (double)p[c] - mean[c];
            acc += d * d;
        }
    }
    acc = corr_group_sum<G>(acc);
    if (live && sub == 0) norm[item] = sqrt(acc);
}

template <int G>
__global__ __launch_bounds__(256) void k_corr_pairs(const float *__restrict__ V, long ldv, int n, int D,
                                                    const int32_t *__restrict__ u, const int32_t *__restrict__ v, long m,
                                                    const double *__restrict__ mean, const double *__restrict__ norm,
                                                    float *__restrict__ out, unsigned long long *__restrict__ info) {
    const long item = ((long)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = item < m;
    int iu = -1, iv = -1;
    if (live) { iu = u[item]; iv = v[item]; }
    const bool bu = iu < 0 || iu >= n, bv = iv < 0 || iv >= n;
    const bool ok = live && !bu && !bv;
    double acc = 0.0;
    if (ok) {
        const float *pu = V + (size_t)iu * ldv, *pv = V + (size_t)iv * ldv;
        for (int c = sub; c < D; c += G) {
            const double mc = mean[c];
            acc += ((double)pu[c] - mc) * ((double)pv[c] - mc);
        }
    }
    acc = corr_group_sum<G>(acc);
    if (live && sub == 0) {
        float s = __uint_as_float(0x7fc00000u);
        if (!ok) {
            atomicAdd(&info[1], (unsigned long long)((bu ? 1 : 0) + (bv ? 1 : 0)));
        } else {
            const double nu = norm[iu], nv = norm[iv];
            if (nu == 0.0 || nv == 0.0) atomicAdd(&info[0], 1ull);
            else s = (float)(acc / nu / nv);
        }
        out[item] = s;
    }
}

}  // namespace

extern "C" size_t lt_corr_workspace_bytes(int32_t n, int32_t D, int32_t k, int64_t n_pairs) {
    if (n < 1 || D < 1 || k < 0 || n_pairs < 0 || n_pairs > 0x7fffffffll) return 0;
    const size_t a = corr_square_words(D, k), b = corr_pairs_words(n, D, (long)n_pairs);
    const size_t w = a > b ? a : b;
    return (w > 2 ? w : 2) * sizeof(double);
}

extern "C" int lt_corr_square(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, float *out,
                              int64_t ldo, int64_t *info, void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(V && nodes && out && info && ws, "lt_corr_square: NULL pointer");
    LT_REQUIRE(n >= 1 && D >= 1 && k >= 0, "lt_corr_square: n=%d, D=%d, k=%d: n and D are >= 1, k >= 0", n, D, k);
    LT_REQUIRE(ldv >= D, "lt_corr_square: ldv=%lld smaller than D=%d", (long long)ldv, D);
    LT_REQUIRE(ldo >= k, "lt_corr_square: ldo=%lld smaller than k=%d", (long long)ldo, k);
    const size_t need = lt_corr_workspace_bytes(n, D, k, 0);
    LT_REQUIRE(ws_bytes >= need && ((uintptr_t)ws % 8) == 0, "lt_corr_square: workspace needs %zu bytes (got %zu), 8-byte aligned", need,
               ws_bytes);
    if (k == 0) return LT_OK;
    hipStream_t st = (hipStream_t)stream;
    const corr_part_plan pp = corr_parts(k);
    const corr_slice_plan sp = corr_slices(k, D);
    double *mean = (double *)ws;
    double *part = mean + corr_round2((size_t)D);
    double *gram = part + corr_round2((size_t)pp.parts * D);
    unsigned long long *inf = (unsigned long long *)info;
    LT_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    const unsigned cb = (unsigned)((D + 255) / 256);
    hipLaunchKernelGGL(k_corr_colsum, dim3(cb, (unsigned)pp.parts), dim3(256), 0, st, V, (long)ldv, n, D, nodes, k, pp.rows_per, part, inf);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_mean, dim3(cb), dim3(256), 0, st, part, pp.parts, D, (long)k, 1, inf, mean);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_gram, dim3((unsigned)(sp.tiles * sp.slices)), dim3(256), 0, st, V, (long)ldv, n, D, nodes, k, mean, sp.tiles,
                       sp.steps_per, gram);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_finish, dim3((unsigned)sp.tiles), dim3(256), 0, st, gram, sp.tiles, sp.slices, n, nodes, k, out, (long)ldo,
                       inf);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_corr_pairs(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *u, const int32_t *v, int64_t m,
                             float *out, int64_t *info, void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(V && u && v && out && info && ws, "lt_corr_pairs: NULL pointer");
    LT_REQUIRE(n >= 1 && D >= 1, "lt_corr_pairs: n=%d, D=%d: both are >= 1", n, D);
    LT_REQUIRE(m >= 0 && m <= 0x7fffffffll, "lt_corr_pairs: m=%lld outside [0, 2^31 - 1]", (long long)m);
    LT_REQUIRE(ldv >= D, "lt_corr_pairs: ldv=%lld smaller than D=%d", (long long)ldv, D);
    const size_t need = lt_corr_workspace_bytes(n, D, 0, m);
    LT_REQUIRE(ws_bytes >= need && ((uintptr_t)ws % 8) == 0, "lt_corr_pairs: workspace needs %zu bytes (got %zu), 8-byte aligned", need,
               ws_bytes);
    if (m == 0) return LT_OK;
    hipStream_t st = (hipStream_t)stream;
    const corr_part_plan pp = corr_parts(n);
    double *mean = (double *)ws;
    double *part = mean + corr_round2((size_t)D);
    double *norm = part + corr_round2((size_t)pp.parts * D);
    unsigned long long *inf = (unsigned long long *)info;
    LT_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    const unsigned cb = (unsigned)((D + 255) / 256);
    hipLaunchKernelGGL(k_corr_colsum, dim3(cb, (unsigned)pp.parts), dim3(256), 0, st, V, (long)ldv, n, D, (const int32_t *)nullptr, n,
                       pp.rows_per, part, inf);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_mean, dim3(cb), dim3(256), 0, st, part, pp.parts, D, (long)n, 0, inf, mean);
    LT_CHECK_LAUNCH();
    if (D > CR_PACK_MAX_D) {
        hipLaunchKernelGGL((k_corr_rownorm<64>), dim3((unsigned)(((long)n * 64 + 255) / 256)), dim3(256), 0, st, V, (long)ldv, n, D, mean, norm);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_corr_pairs<64>), dim3((unsigned)((m * 64 + 255) / 256)), dim3(256), 0, st, V, (long)ldv, n, D, u, v, (long)m,
                           mean, norm, out, inf);
        LT_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL((k_corr_rownorm<CR_PACK>), dim3((unsigned)(((long)n * CR_PACK + 255) / 256)), dim3(256), 0, st, V, (long)ldv, n, D,
                           mean, norm);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL((k_corr_pairs<CR_PACK>), dim3((unsigned)((m * CR_PACK + 255) / 256)), dim3(256), 0, st, V, (long)ldv, n, D, u, v,
                           (long)m, mean, norm, out, inf);
        LT_CHECK_LAUNCH();
    }
    return LT_OK;
}
