// A DP graph stays on the device (include/linkteller_hip.h, "a DP graph stays on the device"):
//   lt_sym_csr_from_cells   the lower-triangle cells of lt_lapgraph_philox / lt_edgerand_philox -> a symmetric CSR, merged with a base
//   lt_normalize_csr        the six normalisers on a unit pattern, in the host's float64 arithmetic, narrowed once to float32
// Both only enqueue.  The only atomics are integer counts of d_info; every position that is written is a function of the input.
#include <stdint.h>

#include "lt_internal.h"
#include "lt_radix.hip.h"

namespace {

#define DG_TILE 1024        // entries of the flag scan per block: 256 threads x 4

struct dg_plan {
    int64_t L, total;       // directed entries 2 m; base_nnz + L
    int rounds, nblk;       // the radix sort's cut of L
    int64_t sblk;           // blocks of the flag scan over total + 1 words
    size_t key[2], pay[2], hist, lptr, mc, flag, bsum, bytes;
};

bool dg_make_plan(int32_t n, int64_t base_nnz, int64_t m, dg_plan *p) {
    if (n < 2 || base_nnz < 0 || m < 0 || m >= ((int64_t)1 << 30) || base_nnz + 2 * m >= (int64_t)INT32_MAX) return false;
    p->L = 2 * m;
    p->total = base_nnz + p->L;
    lt_radix_plan(p->L > 0 ? p->L : 1, &p->rounds, &p->nblk);
    p->sblk = (p->total + 1 + DG_TILE - 1) / DG_TILE;
    size_t at = 0;
    auto take = [&at](size_t words) { const size_t o = at; at += lt_align_up(words * sizeof(int32_t), 8); return o; };
    for (int x = 0; x < 2; ++x) { p->key[x] = take((size_t)p->L); p->pay[x] = take((size_t)p->L); }
    p->hist = take((size_t)256 * p->nblk);
    p->lptr = take((size_t)n + 1);
    p->mc = take((size_t)p->total);
    p->flag = take((size_t)p->total + 1);
    p->bsum = take((size_t)p->sblk);
    p->bytes = at;
    return true;
}

// (row, col) of the directed entry e of the cell list: entry 2 k is (i, j), entry 2 k + 1 is (j, i); a cell that is no strict-lower
// cell of an n x n matrix (or an e outside the list) gives (n, n), which sorts behind every row
__device__ __forceinline__ void dg_entry(const long long *__restrict__ cells, int n, long long L, int e, int &row, int &col) {
    int i = n, j = n;
    if (e >= 0 && e < L) {
        const long long c = cells[e >> 1];
        if (c >= 0 && c < (long long)n * n) {
            i = (int)(c / n);
            j = (int)(c - (long long)i * n);
            if (j >= i) i = j = n;
        }
    }
    row = (e & 1) ? j : i;
    col = (e & 1) ? i : j;
}
__device__ __forceinline__ int dg_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }
// the base's row offset, clamped; 0 without a base
__device__ __forceinline__ int dg_brp(const int32_t *__restrict__ brp, int r, int base_nnz) { return brp ? dg_clamp(brp[r], base_nnz) : 0; }

}  // namespace

// ---- the sort's inputs ---------------------------------------------------------------------------------------------------------
// one thread per cell: the column keys of its two directed entries, and the count of the cells that are none
static __global__ __launch_bounds__(256) void k_dg_expand(const long long *__restrict__ cells, long long m, int n, int32_t *__restrict__ key,
                                                          unsigned long long *__restrict__ info) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    int row, col;
    dg_entry(cells, n, 2 * m, (int)(2 * k), row, col);
    key[2 * k] = col;
    key[2 * k + 1] = row;
    if (row == n) atomicAdd(&info[1], 1ull);
}
// after the sort by column: the row of every entry, the key of the second sort
static __global__ __launch_bounds__(256) void k_dg_rowkey(const long long *__restrict__ cells, long long L, int n, const int32_t *__restrict__ pay,
                                                          int32_t *__restrict__ key) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    int row, col;
    dg_entry(cells, n, L, pay[p], row, col);
    key[p] = row;
}
// after the sort by row: col * 2 + coin of every entry, in (row, col) order
static __global__ __launch_bounds__(256) void k_dg_colcoin(const long long *__restrict__ cells, const uint8_t *__restrict__ coins, long long L, int n,
                                                           const int32_t *__restrict__ pay, uint32_t *__restrict__ cc) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const int e = pay[p];
    int row, col;
    dg_entry(cells, n, L, e, row, col);
    const unsigned coin = (coins && e >= 0 && e < L) ? (coins[e >> 1] != 0) : 1u;
    cc[p] = (uint32_t)col * 2u + coin;
}
// lptr[r] = the first sorted entry whose row is >= r, r in [0, n]: lptr[n] entries belong to rows of the matrix
static __global__ __launch_bounds__(256) void k_dg_listptr(const int32_t *__restrict__ rows, long long L, int n, int32_t *__restrict__ lptr) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > n) return;
    long long lo = 0, hi = L;                              // rows[lo - 1] < r <= rows[hi]
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (rows[mid] < r) lo = mid + 1; else hi = mid;
    }
    lptr[r] = (int32_t)lo;
}

// ---- the merge: every entry finds its place in its row's merged order (base entry first where the columns are equal) ------------
// A listed entry (r, c, coin) at sorted position p stands behind the base columns <= c of row r; it is kept when the coin sets a
// pair the base does not hold.  An entry that repeats its left neighbour is dropped and, on the lower-triangle side, counted.
static __global__ __launch_bounds__(256) void k_dg_place_list(const int32_t *__restrict__ rows, const uint32_t *__restrict__ cc, long long L, int n,
                                                              const int32_t *__restrict__ lptr, const int32_t *__restrict__ brp,
                                                              const int32_t *__restrict__ bcol, int base_nnz, long long total,
                                                              int32_t *__restrict__ mc, int32_t *__restrict__ flag,
                                                              unsigned long long *__restrict__ info) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= L) return;
    const int r = rows[p];
    if (r < 0 || r >= n) return;
    const int c = (int)(cc[p] >> 1);
    const unsigned coin = cc[p] & 1u;
    const int b = dg_brp(brp, r, base_nnz);
    int e = dg_brp(brp, r + 1, base_nnz);
    if (e < b) e = b;
    int lo = b, hi = e;                                    // base columns of [b, lo) are <= c, those of [hi, e) are > c
    while (lo < hi) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (bcol[mid] <= c) lo = mid + 1; else hi = mid;
    }
    const bool found = lo > b && bcol[lo - 1] == c;
    const bool dup = p > lptr[r] && (int)(cc[p - 1] >> 1) == c;
    if (dup && r > c) atomicAdd(&info[2], 1ull);
    const long long pos = p + lo;                          // (b + lptr[r]) + (p - lptr[r]) + (lo - b)
    if (pos < total) {
        mc[pos] = c;
        flag[pos] = (coin && !found && !dup) ? 1 : 0;
    }
}
// A base entry (r, c) at k stands behind the listed columns < c of row r; it is kept unless the list clears the pair.
static __global__ __launch_bounds__(256) void k_dg_place_base(const int32_t *__restrict__ brp, const int32_t *__restrict__ bcol, int base_nnz, int n,
                                                              const int32_t *__restrict__ lptr, const uint32_t *__restrict__ cc,
                                                              long long total, int32_t *__restrict__ mc, int32_t *__restrict__ flag) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= base_nnz) return;
    int lo = 0, hi = n;                                    // brp[lo] <= k < brp[hi]
    while (hi - lo > 1) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (dg_brp(brp, mid, base_nnz) <= k) lo = mid; else hi = mid;
    }
    const int r = lo, c = bcol[k];
    const int l0 = lptr[r], l1 = lptr[r + 1];
    int a = l0, z = l1;                                    // listed columns of [l0, a) are < c, those of [z, l1) are >= c
    while (a < z) {
        const int mid = (int)(((long long)a + z) >> 1);
        if ((long long)(cc[mid] >> 1) < (long long)c) a = mid + 1; else z = mid;
    }
    const bool cleared = a < l1 && (int)(cc[a] >> 1) == c && (cc[a] & 1u) == 0u;
    const long long pos = k + a;                           // (brp[r] + l0) + (k - brp[r]) + (a - l0)
    if (pos < total) {
        mc[pos] = c;
        flag[pos] = cleared ? 0 : 1;
    }
}

// ---- the ordered compaction: flag[0 .. N) -> its exclusive prefix sums in place, in three launches ----------------------------------
static __global__ __launch_bounds__(256) void k_dg_tile_sums(const int32_t *__restrict__ flag, long long N, int32_t *__restrict__ bsum) {
    __shared__ int s_part[4];
    const long long at = (long long)blockIdx.x * DG_TILE + 4 * threadIdx.x;
    int s = 0;
    for (int x = 0; x < 4; ++x) if (at + x < N) s += flag[at + x];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}
static __global__ __launch_bounds__(256) void k_dg_tile_scan(int32_t *__restrict__ flag, long long N, const int32_t *__restrict__ bsum) {
    __shared__ int s_scan[256];
    const int t = threadIdx.x;
    const long long at = (long long)blockIdx.x * DG_TILE + 4 * t;
    int v[4], s = 0;
    for (int x = 0; x < 4; ++x) { v[x] = at + x < N ? flag[at + x] : 0; s += v[x]; }
    s_scan[t] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    int run = bsum[blockIdx.x] + s_scan[t] - s;
    for (int x = 0; x < 4; ++x) {
        if (at + x < N) flag[at + x] = run;
        run += v[x];
    }
}
// scan[x + 1] != scan[x]: merged entry x is kept and lands at scan[x]; a row starts where its merged range starts
static __global__ __launch_bounds__(256) void k_dg_write(const int32_t *__restrict__ scan, const int32_t *__restrict__ mc, long long total, int n,
                                                         const int32_t *__restrict__ brp, int base_nnz, const int32_t *__restrict__ lptr,
                                                         int32_t *__restrict__ out_rowptr, int32_t *__restrict__ out_col, long long capacity,
                                                         long long *__restrict__ info) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x < total) {
        const int s = scan[x];
        if (scan[x + 1] != s && s >= 0 && s < capacity) out_col[s] = mc[x];
    }
    if (x <= n) {
        long long start = (long long)dg_brp(brp, (int)x, base_nnz) + lptr[x];
        if (start > total) start = total;
        out_rowptr[x] = scan[start];
    }
    if (x == 0) { info[0] = scan[total]; info[3] = 0; }
}

extern "C" size_t lt_sym_csr_workspace_bytes(int32_t n, int64_t base_nnz, int64_t m) {
    dg_plan p;
    return dg_make_plan(n, base_nnz, m, &p) ? p.bytes : 0;
}

extern "C" int lt_sym_csr_from_cells(int32_t n, const int32_t *base_rowptr_or_null, const int32_t *base_col_or_null, int64_t base_nnz,
                                     const int64_t *cells, const uint8_t *coins_or_null, int64_t m, int32_t *out_rowptr, int32_t *out_col,
                                     int64_t out_capacity, int64_t *d_info, void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(cells && out_rowptr && out_col && d_info && ws, "lt_sym_csr_from_cells: NULL pointer");
    LT_REQUIRE((base_rowptr_or_null != nullptr) == (base_col_or_null != nullptr),
               "lt_sym_csr_from_cells: the base needs both rowptr and col, or neither");
    LT_REQUIRE(n >= 2, "lt_sym_csr_from_cells: n=%d < 2", n);
    LT_REQUIRE(m >= 0 && base_nnz >= 0, "lt_sym_csr_from_cells: negative size (m=%lld base_nnz=%lld)", (long long)m, (long long)base_nnz);
    LT_REQUIRE(base_rowptr_or_null || base_nnz == 0, "lt_sym_csr_from_cells: base_nnz=%lld without a base", (long long)base_nnz);
    LT_REQUIRE(out_capacity >= 0, "lt_sym_csr_from_cells: negative capacity %lld", (long long)out_capacity);
    dg_plan p;
    LT_REQUIRE(dg_make_plan(n, base_nnz, m, &p), "lt_sym_csr_from_cells: base_nnz + 2 m = %lld + 2 * %lld does not fit int32 row pointers",
               (long long)base_nnz, (long long)m);
    LT_REQUIRE(ws_bytes >= p.bytes && ((uintptr_t)ws % 8) == 0,
               "lt_sym_csr_from_cells: workspace needs %zu bytes (got %zu), 8-byte aligned", p.bytes, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    int32_t *key[2] = {(int32_t *)(w + p.key[0]), (int32_t *)(w + p.key[1])};
    int32_t *pay[2] = {(int32_t *)(w + p.pay[0]), (int32_t *)(w + p.pay[1])};
    int32_t *hist = (int32_t *)(w + p.hist), *lptr = (int32_t *)(w + p.lptr), *mc = (int32_t *)(w + p.mc);
    int32_t *flag = (int32_t *)(w + p.flag), *bsum = (int32_t *)(w + p.bsum);
    const long long L = p.L, total = p.total;
    const int cL = (int)L, cbase = (int)base_nnz;
    auto blocks = [](long long count) { return dim3((unsigned)((count + 255) / 256)); };

    LT_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), st));
    LT_HIP(hipMemsetAsync(flag, 0, ((size_t)total + 1) * sizeof(int32_t), st));
    const int32_t *rows = key[0];
    const uint32_t *cc = (const uint32_t *)key[1];
    if (L > 0) {
        hipLaunchKernelGGL(k_dg_expand, blocks(m), dim3(256), 0, st, (const long long *)cells, (long long)m, n, key[0],
                           (unsigned long long *)d_info);
        LT_CHECK_LAUNCH();
        // two stable sorts, by column and then by row; keys run to n (the entries of cells that are none)
        const int passes = lt_radix_passes(n);
        int cur = 0;                                       // key[cur] holds the keys of the next pass
        const int32_t *pin = nullptr;
        for (int half = 0; half < 2; ++half) {
            for (int q = 0; q < passes; ++q) {
                hipLaunchKernelGGL(k_gb_radix_hist, dim3((unsigned)p.nblk), dim3(256), 0, st, key[cur], cL, 8 * q, p.rounds, p.nblk, hist);
                LT_CHECK_LAUNCH();
                hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, hist, (long long)256 * p.nblk);
                LT_CHECK_LAUNCH();
                hipLaunchKernelGGL(k_gb_radix_scatter, dim3((unsigned)p.nblk), dim3(256), 0, st, key[cur], pin, cL, 8 * q, p.rounds, p.nblk,
                                   hist, key[cur ^ 1], pay[cur ^ 1]);
                LT_CHECK_LAUNCH();
                cur ^= 1;
                pin = pay[cur];
            }
            if (half == 0) {                               // the sorted columns are done with: their buffer takes the row keys
                hipLaunchKernelGGL(k_dg_rowkey, blocks(L), dim3(256), 0, st, (const long long *)cells, L, n, pin, key[cur]);
                LT_CHECK_LAUNCH();
            }
        }
        rows = key[cur];
        cc = (const uint32_t *)key[cur ^ 1];
        hipLaunchKernelGGL(k_dg_colcoin, blocks(L), dim3(256), 0, st, (const long long *)cells, coins_or_null, L, n, pin, (uint32_t *)key[cur ^ 1]);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dg_listptr, blocks((long long)n + 1), dim3(256), 0, st, rows, L, n, lptr);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_dg_place_list, blocks(L), dim3(256), 0, st, rows, cc, L, n, lptr, base_rowptr_or_null, base_col_or_null, cbase,
                           total, mc, flag, (unsigned long long *)d_info);
        LT_CHECK_LAUNCH();
    } else {
        LT_HIP(hipMemsetAsync(lptr, 0, ((size_t)n + 1) * sizeof(int32_t), st));
    }
    if (base_nnz > 0) {
        hipLaunchKernelGGL(k_dg_place_base, blocks(base_nnz), dim3(256), 0, st, base_rowptr_or_null, base_col_or_null, cbase, n, lptr, cc,
                           total, mc, flag);
        LT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_dg_tile_sums, dim3((unsigned)p.sblk), dim3(256), 0, st, flag, total + 1, bsum);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, bsum, (long long)p.sblk);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_dg_tile_scan, dim3((unsigned)p.sblk), dim3(256), 0, st, flag, total + 1, bsum);
    LT_CHECK_LAUNCH();
    const long long span = total > (long long)n + 1 ? total : (long long)n + 1;
    hipLaunchKernelGGL(k_dg_write, blocks(span), dim3(256), 0, st, flag, mc, total, n, base_rowptr_or_null, cbase, lptr, out_rowptr, out_col,
                       (long long)out_capacity, (long long *)d_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- lt_normalize_csr -----------------------------------------------------------------------------------------------------------
// A quarter wave (16 lanes) per row.  Pass 1: the row's length in the output (its entries, plus the diagonal where the form adds the
// identity and the row has none) and the check of its columns; a one-block scan; pass 2 writes columns and values.
#define NM_LANES 16
#define NM_ROWS (256 / NM_LANES)

static __device__ __forceinline__ int nm_sum16(int v) {
    for (int off = NM_LANES / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, NM_LANES);
    return v;
}

static __global__ __launch_bounds__(256) void k_nm_lengths(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz,
                                                           int add_diag, int32_t *__restrict__ out_rowptr, unsigned long long *__restrict__ info) {
    const long long r = (long long)blockIdx.x * NM_ROWS + threadIdx.x / NM_LANES;
    const int sub = threadIdx.x % NM_LANES;
    int b = 0, e = 0;
    if (r < n) {
        b = dg_clamp(rowptr[r], nnz);
        e = dg_clamp(rowptr[r + 1], nnz);
        if (e < b) e = b;
    }
    int bad = 0, diag = 0;
    for (int k = b + sub; k < e; k += NM_LANES) {
        const int c = col[k];
        if (c < 0 || c >= n || (k > b && col[k - 1] >= c)) bad = 1;
        if (c == r) diag = 1;
    }
    bad = nm_sum16(bad);
    diag = nm_sum16(diag);
    if (sub != 0 || r > n) return;
    out_rowptr[r] = r < n ? (e - b) + ((add_diag && !diag) ? 1 : 0) : 0;
    if (bad) atomicAdd(&info[1], 1ull);
}

static __global__ __launch_bounds__(256) void k_nm_fill(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz,
                                                        int aug, int plus1, int sym, const double *__restrict__ inv_pow,
                                                        const int32_t *__restrict__ out_rowptr, int32_t *__restrict__ out_col,
                                                        float *__restrict__ out_val, long long capacity, long long *__restrict__ info) {
    const long long r = (long long)blockIdx.x * NM_ROWS + threadIdx.x / NM_LANES;
    const int sub = threadIdx.x % NM_LANES;
    if (r == 0 && sub == 0) info[0] = out_rowptr[n];
    int b = 0, e = 0;
    if (r < n) {
        b = dg_clamp(rowptr[r], nnz);
        e = dg_clamp(rowptr[r + 1], nnz);
        if (e < b) e = b;
    }
    int less = 0, diag = 0;
    for (int k = b + sub; k < e; k += NM_LANES) {
        const int c = col[k];
        less += c < r;
        diag |= c == r;
    }
    less = nm_sum16(less);
    diag = nm_sum16(diag);
    if (r >= n) return;
    const int ins = ((aug || plus1) && !diag) ? 1 : 0;     // the identity adds an entry of its own
    const long long o = out_rowptr[r];
    const long long top = (long long)n + 1;                // inv_pow has n + 2 entries
    const long long s_r = (long long)(e - b) + aug;
    const double d_r = inv_pow[s_r < top ? s_r : top];
    for (int k = b + sub; k < e; k += NM_LANES) {
        const int c = col[k];
        double v = d_r * ((aug && c == r) ? 2.0 : 1.0);
        if (sym) {
            double d_c = 0.0;
            if (c >= 0 && c < n) {
                const int cb = dg_clamp(rowptr[c], nnz), ce = dg_clamp(rowptr[c + 1], nnz);
                const long long s_c = (long long)(ce > cb ? ce - cb : 0) + aug;
                d_c = inv_pow[s_c < top ? s_c : top];
            }
            v = v * d_c;
        }
        if (plus1 && c == r) v = v + 1.0;
        const long long pos = o + (k - b) + ((ins && c > r) ? 1 : 0);
        if (pos >= 0 && pos < capacity) {
            out_col[pos] = c;
            out_val[pos] = (float)v;
        }
    }
    if (ins && sub == 0) {
        double v = 0.0;
        if (aug) {
            v = d_r * 1.0;
            if (sym) v = v * d_r;
        }
        if (plus1) v = v + 1.0;
        const long long pos = o + less;
        if (pos >= 0 && pos < capacity) {
            out_col[pos] = (int32_t)r;
            out_val[pos] = (float)v;
        }
    }
}

extern "C" int lt_normalize_csr(int32_t n, const int32_t *rowptr, const int32_t *col, int64_t nnz, int32_t norm, const double *inv_pow,
                                int32_t *out_rowptr, int32_t *out_col, float *out_val, int64_t out_capacity, int64_t *d_info,
                                void *stream) {
    LT_REQUIRE(rowptr && col && inv_pow && out_rowptr && out_col && out_val && d_info, "lt_normalize_csr: NULL pointer");
    LT_REQUIRE(n >= 1, "lt_normalize_csr: n=%d < 1", n);
    LT_REQUIRE(nnz >= 0 && nnz < (int64_t)INT32_MAX - n, "lt_normalize_csr: nnz=%lld is negative or nnz + n does not fit int32 row pointers",
               (long long)nnz);
    LT_REQUIRE(norm >= LT_NORM_FIRST_ORDER_GCN && norm <= LT_NORM_AUG_NORM_ADJ, "lt_normalize_csr: unknown norm %d", norm);
    LT_REQUIRE(out_capacity >= 0, "lt_normalize_csr: negative capacity %lld", (long long)out_capacity);
    hipStream_t st = (hipStream_t)stream;
    const int aug = norm == LT_NORM_BINGGE || norm == LT_NORM_AUG_RWALK || norm == LT_NORM_AUG_NORM_ADJ;
    const int plus1 = norm == LT_NORM_FIRST_ORDER_GCN || norm == LT_NORM_BINGGE;
    const int sym = norm != LT_NORM_RWALK && norm != LT_NORM_AUG_RWALK;
    const dim3 grid((unsigned)(((long long)n + 1 + NM_ROWS - 1) / NM_ROWS));
    LT_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_nm_lengths, grid, dim3(256), 0, st, n, rowptr, col, (int)nnz, aug || plus1, out_rowptr, (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, out_rowptr, (long long)n + 1);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_nm_fill, grid, dim3(256), 0, st, n, rowptr, col, (int)nnz, aug, plus1, sym, inv_pow, out_rowptr, out_col, out_val,
                       (long long)out_capacity, (long long *)d_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}
