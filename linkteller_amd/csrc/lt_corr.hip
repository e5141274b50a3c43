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
//   k_corr_rows_norm    (row bands, prepare) the Gram's diagonal tiles only, the slices in order inside the block -> the norms.
//   k_corr_rows         (row bands) the tile body at (band row block, column block) origins; a plan of one slice finishes in the
//                       epilogue, else k_corr_rows_finish adds the band's partials in slice order.  Same bits as the square's cells.
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

// One K slice (staging steps [s0, s1)) of a 64 x 64 tile with ARBITRARY origins: rows nodes[row0 + r] against columns nodes[col0 + c],
// r, c < 64, accumulated onto acc.  List positions at or past row_end / col_end, and ids outside [0, n), are staged as zeros and
// never loaded.  A cell's value depends on its two rows, the mean and (s0, s1) alone -- not on the origins, and not on which of the
// two rows is the A operand (the products commute, the K order is the same): the square's tiles and the row bands' give equal bits.
// Opens with a barrier, so it may be called again on the same LDS (the next slice) without one in between.
__device__ __forceinline__ void corr_tile_slice(const float *__restrict__ V, long ldv, int n, int D, const int32_t *__restrict__ nodes,
                                                const double *__restrict__ mean, int row0, int row_end, int col0, int col_end, int s0,
                                                int s1, double *As, double *Bs, cr_f64x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    // staging: thread -> row tid >> 2 of both tiles, columns (tid & 3) * 4 .. + 3 of the step
    const int a_row = tid >> 2, a_col = (tid & 3) * 4;
    const int gi = row0 + a_row, gj = col0 + a_row;
    int id_i = gi < row_end ? nodes[gi] : -1, id_j = gj < col_end ? nodes[gj] : -1;
    if (id_i < 0 || id_i >= n) id_i = -1;
    if (id_j < 0 || id_j >= n) id_j = -1;
    const float *pa = V + (size_t)(id_i < 0 ? 0 : id_i) * ldv;
    const float *pb = V + (size_t)(id_j < 0 ? 0 : id_j) * ldv;
    const int a_frag = (wr * 32 + (lane & 15)) * CR_LD + (lane >> 4);
    const int b_frag = (wc * 32 + (lane & 15)) * CR_LD + (lane >> 4);
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
}

__device__ __forceinline__ void corr_acc_zero(cr_f64x4 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = cr_f64x4{0.0, 0.0, 0.0, 0.0};
}

// grid: tiles * slices blocks, block b = slice * tiles + tile.  gram[(slice * tiles + tile) * 4096 + r * 64 + c].
__global__ __launch_bounds__(256) void k_corr_gram(const float *__restrict__ V, long ldv, int n, int D,
                                                   const int32_t *__restrict__ nodes, int k, const double *__restrict__ mean,
                                                   long tiles, int steps_per, double *__restrict__ gram) {
    __shared__ double As[CR_BM * CR_LD];
    __shared__ double Bs[CR_BM * CR_LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const long tile = (long)blockIdx.x % tiles;
    const int slice = (int)((long)blockIdx.x / tiles);
    int ti, tj;
    corr_tile_of(tile, &ti, &tj);
    const int steps = (D + CR_BK - 1) / CR_BK;
    const int s0 = slice * steps_per;
    const int s1 = s0 + steps_per < steps ? s0 + steps_per : steps;
    cr_f64x4 acc[2][2];
    corr_acc_zero(acc);
    corr_tile_slice(V, ldv, n, D, nodes, mean, ti * CR_BM, k, tj * CR_BM, k, s0, s1, As, Bs, acc);
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

// ---- (c') row bands of the square: lt_corr_rows_prepare / lt_corr_rows -----------------------------------------------------------------
// A cell's bits are the square's: the same tile body, the slice plan of the WHOLE list (corr_slices(k, D)), every slice from a zero
// accumulator, the slices added in slice order from 0.0, the norms from the diagonal formed that way, one rounding.  The two divisions
// each round, and (g / a) / b is not (g / b) / a: the square forms a cell in its LOWER position only -- g / n_row / n_col with
// row >= col -- and mirrors those bits, so a cell above the diagonal divides by the norm of its COLUMN (the larger list position) first.
__device__ __forceinline__ float corr_cell(double g, int gi, int gj, const double *__restrict__ norm) {
    const double n_hi = norm[gi >= gj ? gi : gj], n_lo = norm[gi >= gj ? gj : gi];
    if (n_hi != n_hi || n_lo != n_lo || n_hi == 0.0 || n_lo == 0.0) return __uint_as_float(0x7fc00000u);
    return (float)(g / n_hi / n_lo);
}

// prepare: one block per DIAGONAL tile, the slices one after the other in the block.  norm[g] = sqrt of the diagonal cell; NaN marks a
// bad node id.  Only the waves on the tile's diagonal (wr == wc) hold diagonal cells, all four stage.
__global__ __launch_bounds__(256) void k_corr_rows_norm(const float *__restrict__ V, long ldv, int n, int D,
                                                        const int32_t *__restrict__ nodes, int k, const double *__restrict__ mean,
                                                        int steps_per, int slices, double *__restrict__ norm,
                                                        unsigned long long *__restrict__ info) {
    __shared__ double As[CR_BM * CR_LD];
    __shared__ double Bs[CR_BM * CR_LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int row0 = blockIdx.x * CR_BM;
    const int steps = (D + CR_BK - 1) / CR_BK;
    double tot[2][4];      // the diagonal sub-tiles (i == j) only
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) tot[i][reg] = 0.0;
    for (int s = 0; s < slices; ++s) {
        const int s0 = s * steps_per;
        const int s1 = s0 + steps_per < steps ? s0 + steps_per : steps;
        cr_f64x4 acc[2][2];
        corr_acc_zero(acc);
        corr_tile_slice(V, ldv, n, D, nodes, mean, row0, k, row0, k, s0, s1, As, Bs, acc);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) tot[i][reg] += acc[i][i][reg];
    }
    if (wr != wc) return;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            if ((lane & 15) != (lane >> 4) + 4 * reg) continue;      // C/D layout: col = lane & 15, row = (lane >> 4) + 4 * reg
            const int g = row0 + wr * 32 + i * 16 + (lane & 15);
            if (g >= k) continue;
            const int id = nodes[g];
            double v = nan("");
            if (id >= 0 && id < n) {
                v = sqrt(tot[i][reg]);
                if (v == 0.0) atomicAdd(&info[0], 1ull);      // (an integer count, each listed row once)
            }
            norm[g] = v;
        }
}

// rows: grid (column blocks of [0, n_cols), row blocks of the band, FUSED ? 1 : slices).  The band's row blocks start at row_begin,
// not on a multiple of 64.  FUSED (a plan of one slice): the finish is the epilogue, nothing is stored but the scores.  Else the
// slice's 64 x 64 partial goes to part[((slice * row blocks + rb) * column blocks + cb) * 4096 + r * 64 + c] for k_corr_rows_finish.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_corr_rows(const float *__restrict__ V, long ldv, int n, int D,
                                                   const int32_t *__restrict__ nodes, const double *__restrict__ mean,
                                                   const double *__restrict__ norm, int row_begin, int n_rows, int n_cols,
                                                   int steps_per, float *__restrict__ out, long ldo, double *__restrict__ part) {
    __shared__ double As[CR_BM * CR_LD];
    __shared__ double Bs[CR_BM * CR_LD];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int row0 = row_begin + (int)blockIdx.y * CR_BM, row_end = row_begin + n_rows;
    const int col0 = (int)blockIdx.x * CR_BM;
    const int steps = (D + CR_BK - 1) / CR_BK;
    const int s0 = FUSED ? 0 : (int)blockIdx.z * steps_per;
    const int s1 = FUSED ? steps : (s0 + steps_per < steps ? s0 + steps_per : steps);
    cr_f64x4 acc[2][2];
    corr_acc_zero(acc);
    corr_tile_slice(V, ldv, n, D, nodes, mean, row0, row_end, col0, n_cols, s0, s1, As, Bs, acc);
    double *dst = FUSED ? nullptr : part + (((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * CR_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = wc * 32 + j * 16 + (lane & 15);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = wr * 32 + i * 16 + (lane >> 4) + 4 * reg;
                if (FUSED) {
                    const int gi = row0 + r, gj = col0 + c;
                    if (gi < row_end && gj < n_cols)
                        out[(size_t)(gi - row_begin) * ldo + gj] = corr_cell(0.0 + acc[i][j][reg], gi, gj, norm);
                } else {
                    dst[r * CR_BM + c] = acc[i][j][reg];
                }
            }
        }
}

// grid (column blocks, row blocks): the slices' partials in slice order, divide, round once, store as row segments
__global__ __launch_bounds__(256) void k_corr_rows_finish(const double *__restrict__ part, int slices, const double *__restrict__ norm,
                                                          int row_begin, int n_rows, int n_cols, float *__restrict__ out, long ldo) {
    const int row0 = row_begin + (int)blockIdx.y * CR_BM, row_end = row_begin + n_rows;
    const int col0 = (int)blockIdx.x * CR_BM;
    const size_t t0 = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * CR_TILE;
    const size_t per_slice = (size_t)gridDim.y * gridDim.x * CR_TILE;
    for (int e = threadIdx.x; e < CR_TILE; e += 256) {
        const int gi = row0 + (e >> 6), gj = col0 + (e & 63);
        if (gi >= row_end || gj >= n_cols) continue;
        double g = 0.0;
        for (int s = 0; s < slices; ++s) g += part[(size_t)s * per_slice + t0 + e];
        out[(size_t)(gi - row_begin) * ldo + gj] = corr_cell(g, gi, gj, norm);
    }
}

// the rows calls' workspace: mean | column-sum partitions | norms (the head, what prepare leaves) | a band's partials
size_t corr_rows_head_words(int D, int k) {
    return corr_round2((size_t)D) + corr_round2((size_t)corr_parts(k).parts * D) + corr_round2((size_t)k);
}
size_t corr_rows_part_words(int D, int k, int rows) {
    if (k <= 0 || rows <= 0) return 0;
    const corr_slice_plan sp = corr_slices(k, D);
    if (sp.slices == 1) return 0;
    return (size_t)sp.slices * ((rows + CR_BM - 1) / CR_BM) * sp.tiles_edge * CR_TILE;
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

extern "C" size_t lt_corr_rows_workspace_bytes(int32_t n, int32_t D, int32_t k, int32_t max_rows) {
    if (n < 1 || D < 1 || k < 0 || max_rows < 0) return 0;
    const size_t w = corr_rows_head_words(D, k) + corr_rows_part_words(D, k, max_rows);
    return (w > 2 ? w : 2) * sizeof(double);
}

extern "C" int lt_corr_rows_prepare(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, int64_t *info,
                                    void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(V && nodes && info && ws, "lt_corr_rows_prepare: NULL pointer");
    LT_REQUIRE(n >= 1 && D >= 1 && k >= 0, "lt_corr_rows_prepare: n=%d, D=%d, k=%d: n and D are >= 1, k >= 0", n, D, k);
    LT_REQUIRE(ldv >= D, "lt_corr_rows_prepare: ldv=%lld smaller than D=%d", (long long)ldv, D);
    const size_t need = lt_corr_rows_workspace_bytes(n, D, k, 0);
    LT_REQUIRE(ws_bytes >= need && ((uintptr_t)ws % 8) == 0, "lt_corr_rows_prepare: workspace needs %zu bytes (got %zu), 8-byte aligned",
               need, ws_bytes);
    if (k == 0) return LT_OK;      // (as lt_corr_square: nothing is enqueued, info is left alone)
    hipStream_t st = (hipStream_t)stream;
    const corr_part_plan pp = corr_parts(k);
    const corr_slice_plan sp = corr_slices(k, D);
    double *mean = (double *)ws;
    double *part = mean + corr_round2((size_t)D);
    double *norm = part + corr_round2((size_t)pp.parts * D);
    unsigned long long *inf = (unsigned long long *)info;
    LT_HIP(hipMemsetAsync(info, 0, 4 * sizeof(int64_t), st));
    const unsigned cb = (unsigned)((D + 255) / 256);
    hipLaunchKernelGGL(k_corr_colsum, dim3(cb, (unsigned)pp.parts), dim3(256), 0, st, V, (long)ldv, n, D, nodes, k, pp.rows_per, part, inf);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_mean, dim3(cb), dim3(256), 0, st, part, pp.parts, D, (long)k, 1, inf, mean);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_corr_rows_norm, dim3((unsigned)sp.tiles_edge), dim3(256), 0, st, V, (long)ldv, n, D, nodes, k, mean, sp.steps_per,
                       sp.slices, norm, inf);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_corr_rows(const float *V, int64_t ldv, int32_t n, int32_t D, const int32_t *nodes, int32_t k, int32_t row_begin,
                            int32_t n_rows, int32_t n_cols, float *out, int64_t ldo, void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(V && nodes && out && ws, "lt_corr_rows: NULL pointer");
    LT_REQUIRE(n >= 1 && D >= 1 && k >= 0, "lt_corr_rows: n=%d, D=%d, k=%d: n and D are >= 1, k >= 0", n, D, k);
    LT_REQUIRE(ldv >= D, "lt_corr_rows: ldv=%lld smaller than D=%d", (long long)ldv, D);
    LT_REQUIRE(row_begin >= 0 && n_rows >= 0 && (int64_t)row_begin + n_rows <= k,
               "lt_corr_rows: rows [%d, %d + %d) outside the %d listed", row_begin, row_begin, n_rows, k);
    LT_REQUIRE(n_cols >= 0 && n_cols <= k, "lt_corr_rows: n_cols=%d outside [0, %d]", n_cols, k);
    LT_REQUIRE(n_rows <= 65535 * CR_BM, "lt_corr_rows: n_rows=%d above %d a call", n_rows, 65535 * CR_BM);
    LT_REQUIRE(ldo >= n_cols, "lt_corr_rows: ldo=%lld smaller than n_cols=%d", (long long)ldo, n_cols);
    // (a band longer than the max_rows the workspace was sized for is a short workspace)
    const size_t need = lt_corr_rows_workspace_bytes(n, D, k, n_rows);
    LT_REQUIRE(ws_bytes >= need && ((uintptr_t)ws % 8) == 0,
               "lt_corr_rows: %d rows need a workspace of %zu bytes (got %zu: n_rows above its max_rows?), 8-byte aligned", n_rows, need,
               ws_bytes);
    if (n_rows == 0 || n_cols == 0) return LT_OK;
    hipStream_t st = (hipStream_t)stream;
    const corr_part_plan pp = corr_parts(k);
    const corr_slice_plan sp = corr_slices(k, D);
    const double *mean = (const double *)ws;
    const double *norm = mean + corr_round2((size_t)D) + corr_round2((size_t)pp.parts * D);
    double *part = (double *)norm + corr_round2((size_t)k);
    // column blocks right of the last needed column are not launched
    const dim3 grid((unsigned)((n_cols + CR_BM - 1) / CR_BM), (unsigned)((n_rows + CR_BM - 1) / CR_BM), 1);
    if (sp.slices == 1) {
        hipLaunchKernelGGL(k_corr_rows<true>, grid, dim3(256), 0, st, V, (long)ldv, n, D, nodes, mean, norm, row_begin, n_rows, n_cols,
                           sp.steps_per, out, (long)ldo, (double *)nullptr);
        LT_CHECK_LAUNCH();
    } else {
        hipLaunchKernelGGL(k_corr_rows<false>, dim3(grid.x, grid.y, (unsigned)sp.slices), dim3(256), 0, st, V, (long)ldv, n, D, nodes, mean,
                           norm, row_begin, n_rows, n_cols, sp.steps_per, out, (long)ldo, part);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_corr_rows_finish, grid, dim3(256), 0, st, part, sp.slices, norm, row_begin, n_rows, n_cols, out, (long)ldo);
        LT_CHECK_LAUNCH();
    }
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
