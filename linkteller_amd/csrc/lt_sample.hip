// The attack's node pairs on the device (include/linkteller_hip.h, "the attack's node pairs"):
//   lt_sample_square_labels     all pairs of a node sample: the label triangle and the index of their score cells
//   lt_group_pairs              a pair list grouped by probe, the layout of lt_influence_pairs
//   lt_upper_edge_count         E = the stored entries with col > row
//   lt_sample_balanced_philox   those E edges and the first E accepted non-edge draws of Philox stream 3
// The adjacency is a device CSR whose rows are sorted and unique; a stored entry counts whatever its value.  The only atomics are
// integer counts; every position that is written is a function of the input.
#include <stdint.h>

#include "lt_internal.h"
#include "lt_philox.hip.h"
#include "lt_radix.hip.h"

namespace {

#define SM_TILE 1024        // words of the flag scan per block: 256 threads x 4

__device__ __forceinline__ int sm_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the extent [b, e) of row r, clamped to the stored entries
__device__ __forceinline__ void sm_row(const int32_t *__restrict__ rowptr, int r, int nnz, int &b, int &e) {
    b = sm_clamp(rowptr[r], nnz);
    e = sm_clamp(rowptr[r + 1], nnz);
    if (e < b) e = b;
}
// the first entry of [b, e) whose column is >= c (the row is sorted)
__device__ __forceinline__ int sm_lower_bound(const int32_t *__restrict__ col, int b, int e, int c) {
    while (b < e) {
        const int mid = (int)(((long long)b + e) >> 1);
        if (col[mid] < c) b = mid + 1; else e = mid;
    }
    return b;
}
// is c stored in row r?  (r, c in [0, n))
__device__ __forceinline__ bool sm_stored(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz, int r, int c) {
    int b, e;
    sm_row(rowptr, r, nnz, b, e);
    const int at = sm_lower_bound(col, b, e, c);
    return at < e && col[at] == c;
}
__device__ __forceinline__ unsigned long long sm_block_sum(unsigned long long v, unsigned long long *s_part) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

}  // namespace

// ---- the ordered compaction's scan: a[0 .. N) -> its exclusive prefix sums in place, in three launches ---------------------------
static __global__ __launch_bounds__(256) void k_sm_tile_sums(const int32_t *__restrict__ a, long long N, int32_t *__restrict__ bsum) {
    __shared__ int s_part[4];
    const long long at = (long long)blockIdx.x * SM_TILE + 4 * threadIdx.x;
    int s = 0;
    for (int x = 0; x < 4; ++x) if (at + x < N) s += a[at + x];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}
static __global__ __launch_bounds__(256) void k_sm_tile_scan(int32_t *__restrict__ a, long long N, const int32_t *__restrict__ bsum) {
    __shared__ int s_scan[256];
    const int t = threadIdx.x;
    const long long at = (long long)blockIdx.x * SM_TILE + 4 * t;
    int v[4], s = 0;
    for (int x = 0; x < 4; ++x) { v[x] = at + x < N ? a[at + x] : 0; s += v[x]; }
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
        if (at + x < N) a[at + x] = run;
        run += v[x];
    }
}
static inline long long sm_scan_blocks(long long N) { return (N + SM_TILE - 1) / SM_TILE; }
// (bsum: sm_scan_blocks(N) words)
static int sm_scan(int32_t *a, long long N, int32_t *bsum, hipStream_t st) {
    const long long sblk = sm_scan_blocks(N);
    hipLaunchKernelGGL(k_sm_tile_sums, dim3((unsigned)sblk), dim3(256), 0, st, a, N, bsum);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, bsum, sblk);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sm_tile_scan, dim3((unsigned)sblk), dim3(256), 0, st, a, N, bsum);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- lt_sample_square_labels ------------------------------------------------------------------------------------------------------
// pos[node] = the node's position in the sample, -1 for the others: cleared, scattered (the last position of a repeated node wins)
// and checked back.
static __global__ __launch_bounds__(256) void k_sq_scatter(const int32_t *__restrict__ nodes, int k, int n, int32_t *__restrict__ pos,
                                                           unsigned long long *__restrict__ info) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= k) return;
    const int v = nodes[t];
    if (v < 0 || v >= n) atomicAdd(&info[1], 1ull);
    else atomicMax(&pos[v], (int)t);
}
static __global__ __launch_bounds__(256) void k_sq_check(const int32_t *__restrict__ nodes, int k, int n, const int32_t *__restrict__ pos,
                                                         unsigned long long *__restrict__ info) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= k) return;
    const int v = nodes[t];
    if (v >= 0 && v < n && pos[v] != (int)t) atomicAdd(&info[2], 1ull);      // one per occurrence beyond a node's first
}
// One block per position i < k - 1.  It owns the slots [p0, p0 + k - 1 - i) of the pairs (i, j), j > i: it clears their labels and
// writes their index, coalesced; after the barrier it walks row nodes[i] and sets the label of every column that sits at a later
// position of the sample.  A hub row is walked by the whole block.
static __global__ __launch_bounds__(256) void k_sq_labels(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz, int n,
                                                          const int32_t *__restrict__ nodes, int k, long long lds,
                                                          const int32_t *__restrict__ pos, uint8_t *__restrict__ labels,
                                                          long long *__restrict__ index, unsigned long long *__restrict__ info) {
    __shared__ unsigned long long s_part[4];
    const int i = blockIdx.x;
    const long long p0 = (long long)i * (2ll * k - i - 1) / 2;
    const int len = k - 1 - i;
    for (int q = threadIdx.x; q < len; q += 256) {
        labels[p0 + q] = 0;
        if (index) index[p0 + q] = (long long)(i + 1 + q) * lds + i;
    }
    __syncthreads();
    const int u = nodes[i];
    unsigned long long found = 0;
    if (u >= 0 && u < n) {
        int b, e;
        sm_row(rowptr, u, nnz, b, e);
        for (int x = b + threadIdx.x; x < e; x += 256) {
            const int c = col[x];
            if (c < 0 || c >= n) continue;
            const int j = pos[c];
            if (j > i && j < k) {
                labels[p0 + (j - i - 1)] = 1;
                ++found;
            }
        }
    }
    found = sm_block_sum(found, s_part);
    if (threadIdx.x == 0 && found) atomicAdd(&info[0], found);
}

extern "C" size_t lt_sample_square_workspace_bytes(int32_t n, int32_t k) {
    if (n < 1 || k < 2) return 0;
    return lt_align_up((size_t)n * sizeof(int32_t), 8);
}

extern "C" int lt_sample_square_labels(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, const int32_t *nodes,
                                       int32_t k, int64_t lds, uint8_t *out_labels, int64_t *out_index_or_null, int64_t *d_info,
                                       void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(d_rowptr && d_col && nodes && out_labels && d_info && ws, "lt_sample_square_labels: NULL pointer");
    LT_REQUIRE(n >= 1, "lt_sample_square_labels: n=%d < 1", n);
    LT_REQUIRE(k >= 2, "lt_sample_square_labels: k=%d < 2", k);
    LT_REQUIRE(lds >= k, "lt_sample_square_labels: lds=%lld < k=%d", (long long)lds, k);
    LT_REQUIRE(nnz >= 0 && nnz < (int64_t)INT32_MAX, "lt_sample_square_labels: nnz=%lld outside [0, 2^31 - 1)", (long long)nnz);
    const size_t need = lt_sample_square_workspace_bytes(n, k);
    LT_REQUIRE(ws_bytes >= need && ((uintptr_t)ws % 8) == 0, "lt_sample_square_labels: workspace needs %zu bytes (got %zu), 8-byte aligned",
               need, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    int32_t *pos = (int32_t *)ws;
    LT_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), st));
    LT_HIP(hipMemsetAsync(pos, 0xff, (size_t)n * sizeof(int32_t), st));
    const dim3 kb((unsigned)(((long long)k + 255) / 256));
    hipLaunchKernelGGL(k_sq_scatter, kb, dim3(256), 0, st, nodes, k, n, pos, (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sq_check, kb, dim3(256), 0, st, nodes, k, n, (const int32_t *)pos, (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sq_labels, dim3((unsigned)(k - 1)), dim3(256), 0, st, d_rowptr, d_col, (int)nnz, n, nodes, k, (long long)lds,
                       (const int32_t *)pos, out_labels, (long long *)out_index_or_null, (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- lt_group_pairs -------------------------------------------------------------------------------------------------------------
namespace {
struct gp_plan {
    int rounds, nblk;
    long long sblk;
    size_t key[2], pay[2], hist, flag, bsum, bytes;
};
bool gp_make_plan(int64_t m, gp_plan *p) {
    if (m < 1 || m > (int64_t)INT32_MAX - 1) return false;
    lt_radix_plan(m, &p->rounds, &p->nblk);
    p->sblk = sm_scan_blocks(m + 1);
    size_t at = 0;
    auto take = [&at](size_t words) { const size_t o = at; at += lt_align_up(words * sizeof(int32_t), 8); return o; };
    for (int x = 0; x < 2; ++x) { p->key[x] = take((size_t)m); p->pay[x] = take((size_t)m); }
    p->hist = take((size_t)256 * p->nblk);
    p->flag = take((size_t)m + 1);
    p->bsum = take((size_t)p->sblk);
    p->bytes = at;
    return true;
}
}  // namespace

static __global__ __launch_bounds__(256) void k_gp_range(const int32_t *__restrict__ probe, const int32_t *__restrict__ observed, long long m, int n,
                                                         unsigned long long *__restrict__ info) {
    __shared__ unsigned long long s_part[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bad = 0;
    if (p < m) bad = (unsigned long long)(probe[p] < 0 || probe[p] >= n) + (unsigned long long)(observed[p] < 0 || observed[p] >= n);
    bad = sm_block_sum(bad, s_part);
    if (threadIdx.x == 0 && bad) atomicAdd(&info[1], bad);
}
// after the sort: the order, the observed ids in that order, and the flag of every pair that starts a probe's group (flag[m] = 0)
static __global__ __launch_bounds__(256) void k_gp_heads(const int32_t *__restrict__ key, const int32_t *__restrict__ pay,
                                                         const int32_t *__restrict__ observed, long long m, int32_t *__restrict__ out_order,
                                                         int32_t *__restrict__ out_obs, int32_t *__restrict__ flag) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p > m) return;
    if (p == m) { flag[p] = 0; return; }
    int src = pay[p];
    if (src < 0 || src >= m) src = 0;
    out_order[p] = src;
    out_obs[p] = observed[src];
    flag[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}
// scan[p + 1] != scan[p]: pair p starts group scan[p]
static __global__ __launch_bounds__(256) void k_gp_write(const int32_t *__restrict__ scan, const int32_t *__restrict__ key, long long m,
                                                         int32_t *__restrict__ out_nodes, long long *__restrict__ out_ptr,
                                                         long long *__restrict__ info) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p > m) return;
    const int g = scan[p];
    if (p == m) {
        if (g >= 0 && g <= m) out_ptr[g] = m;
        info[0] = g;
        return;
    }
    if (scan[p + 1] != g && g >= 0 && g < m) {
        out_nodes[g] = key[p];
        out_ptr[g] = p;
    }
}

extern "C" size_t lt_group_pairs_workspace_bytes(int64_t m) {
    gp_plan p;
    return gp_make_plan(m, &p) ? p.bytes : 0;
}

extern "C" int lt_group_pairs(int32_t n, const int32_t *probe, const int32_t *observed, int64_t m, int32_t *out_nodes, int64_t *out_ptr,
                              int32_t *out_obs, int32_t *out_order, int64_t *d_info, void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(probe && observed && out_nodes && out_ptr && out_obs && out_order && d_info && ws, "lt_group_pairs: NULL pointer");
    LT_REQUIRE(n >= 1, "lt_group_pairs: n=%d < 1", n);
    gp_plan p;
    LT_REQUIRE(gp_make_plan(m, &p), "lt_group_pairs: m=%lld outside [1, 2^31 - 2]", (long long)m);
    LT_REQUIRE(ws_bytes >= p.bytes && ((uintptr_t)ws % 8) == 0, "lt_group_pairs: workspace needs %zu bytes (got %zu), 8-byte aligned",
               p.bytes, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    int32_t *key[2] = {(int32_t *)(w + p.key[0]), (int32_t *)(w + p.key[1])};
    int32_t *pay[2] = {(int32_t *)(w + p.pay[0]), (int32_t *)(w + p.pay[1])};
    int32_t *hist = (int32_t *)(w + p.hist), *flag = (int32_t *)(w + p.flag), *bsum = (int32_t *)(w + p.bsum);
    const int cm = (int)m;
    auto blocks = [](long long count) { return dim3((unsigned)((count + 255) / 256)); };

    LT_HIP(hipMemsetAsync(d_info, 0, 4 * sizeof(int64_t), st));
    hipLaunchKernelGGL(k_gp_range, blocks(m), dim3(256), 0, st, probe, observed, (long long)m, n, (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    // the stable sort by probe; the first pass reads the caller's array and takes the pair's index as its payload
    const int passes = lt_radix_passes((int64_t)n - 1);
    const int32_t *kin = probe, *pin = nullptr;
    int cur = 1;                                           // key[cur ^ 1] / pay[cur ^ 1] take the next pass's output
    for (int q = 0; q < passes; ++q) {
        hipLaunchKernelGGL(k_gb_radix_hist, dim3((unsigned)p.nblk), dim3(256), 0, st, kin, cm, 8 * q, p.rounds, p.nblk, hist);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, hist, (long long)256 * p.nblk);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gb_radix_scatter, dim3((unsigned)p.nblk), dim3(256), 0, st, kin, pin, cm, 8 * q, p.rounds, p.nblk, hist,
                           key[cur ^ 1], pay[cur ^ 1]);
        LT_CHECK_LAUNCH();
        cur ^= 1;
        kin = key[cur];
        pin = pay[cur];
    }
    hipLaunchKernelGGL(k_gp_heads, blocks(m + 1), dim3(256), 0, st, kin, pin, observed, (long long)m, out_order, out_obs, flag);
    LT_CHECK_LAUNCH();
    const int rc = sm_scan(flag, m + 1, bsum, st);
    if (rc != LT_OK) return rc;
    hipLaunchKernelGGL(k_gp_write, blocks(m + 1), dim3(256), 0, st, (const int32_t *)flag, kin, (long long)m, out_nodes,
                       (long long *)out_ptr, (long long *)d_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- lt_upper_edge_count, lt_sample_balanced_philox -----------------------------------------------------------------------------
// The entries of a sorted row with col > row are its tail: their number comes from one bisection.  ucnt: [n + 1] or NULL.
static __global__ __launch_bounds__(256) void k_bp_upper(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz, int n,
                                                         int32_t *__restrict__ ucnt, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long s_part[4];
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    if (r < n) {
        int b, e;
        sm_row(rowptr, (int)r, nnz, b, e);
        cnt = e - sm_lower_bound(col, b, e, (int)r + 1);
    }
    if (ucnt && r <= n) ucnt[r] = cnt;
    const unsigned long long sum = sm_block_sum((unsigned long long)cnt, s_part);
    if (total && threadIdx.x == 0 && sum) atomicAdd(total, sum);
}
// one thread per stored entry: an entry of its row's tail goes to the row's stretch of the edge list, at its place in the tail
static __global__ __launch_bounds__(256) void k_bp_edges(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz, int n,
                                                         const int32_t *__restrict__ uoff, long long E, int32_t *__restrict__ out_u,
                                                         int32_t *__restrict__ out_v) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= nnz) return;
    int lo = 0, hi = n;                                    // rowptr[lo] <= x < rowptr[hi]
    while (hi - lo > 1) {
        const int mid = (int)(((long long)lo + hi) >> 1);
        if (sm_clamp(rowptr[mid], nnz) <= x) lo = mid; else hi = mid;
    }
    const int r = lo, c = col[x];
    int b, e;
    sm_row(rowptr, r, nnz, b, e);
    if (x < b || x >= e || c <= r) return;
    const int cnt = uoff[r + 1] - uoff[r];
    const long long at = (long long)uoff[r] + (x - (e - cnt));
    if (x >= e - cnt && at >= 0 && at < E) {
        out_u[at] = r;
        out_v[at] = c;
    }
}
// draw t of stream 3
__device__ __forceinline__ void bp_draw(unsigned long long t, uint2 key, unsigned n, int &u, int &v) {
    const uint4 w = lt_philox4x32_10(make_uint4((uint32_t)t, (uint32_t)(t >> 32), 3u, 0u), key);
    u = (int)(((unsigned long long)w.x * n) >> 32);
    v = (int)(((unsigned long long)w.y * n) >> 32);
}
// the round's draws t0 + x, x < cnt: the pair and whether it is accepted (flag[cnt] = 0)
static __global__ __launch_bounds__(256) void k_bp_flags(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int nnz, int n,
                                                         unsigned long long t0, long long cnt, uint2 key, int32_t *__restrict__ du,
                                                         int32_t *__restrict__ dv, int32_t *__restrict__ flag) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x > cnt) return;
    if (x == cnt) { flag[x] = 0; return; }
    int u, v;
    bp_draw(t0 + (unsigned long long)x, key, (unsigned)n, u, v);
    du[x] = u;
    dv[x] = v;
    flag[x] = (!sm_stored(rowptr, col, nnz, u, v) && !sm_stored(rowptr, col, nnz, v, u)) ? 1 : 0;
}
// the accepted draws go behind the `have` of the earlier rounds, in draw order, while they fit.  state: [0] accepted and written so
// far, [1] t of the last written draw + 1, [2] written draws with u == v
static __global__ __launch_bounds__(256) void k_bp_write(const int32_t *__restrict__ scan, const int32_t *__restrict__ du,
                                                         const int32_t *__restrict__ dv, unsigned long long t0, long long cnt, long long have,
                                                         long long E, int32_t *__restrict__ out_u, int32_t *__restrict__ out_v,
                                                         unsigned long long *__restrict__ state) {
    __shared__ unsigned long long s_part[4];
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long self = 0;
    if (x < cnt) {
        const int s = scan[x];
        const long long at = have + s;
        if (scan[x + 1] != s && s >= 0 && at < E) {
            out_u[E + at] = du[x];
            out_v[E + at] = dv[x];
            self = du[x] == dv[x];
            if (at == E - 1) state[1] = t0 + (unsigned long long)x + 1ull;
        }
    }
    if (x == 0) {
        const long long got = have + scan[cnt];
        state[0] = (unsigned long long)(got < E ? got : E);
    }
    self = sm_block_sum(self, s_part);
    if (threadIdx.x == 0 && self) atomicAdd(&state[2], self);
}

namespace {
#define BP_ROUND_MAX ((int64_t)1 << 24)
struct bp_plan {
    int64_t R;
    size_t uoff, du, dv, flag, bsum, state, bytes;
};
bool bp_make_plan(int32_t n, int64_t E, int64_t round_draws, bp_plan *p) {
    if (n < 1 || E < 0 || E >= ((int64_t)1 << 30) || round_draws < 0 || round_draws > BP_ROUND_MAX) return false;
    int64_t R = round_draws;
    if (R == 0) {                                          // one round usually does: E draws and the share a sparse graph refuses
        R = (E + E / 8 + 4096 + 1023) / 1024 * 1024;
        if (R > ((int64_t)1 << 22)) R = (int64_t)1 << 22;
    }
    p->R = R;
    const int64_t span = R > (int64_t)n ? R : (int64_t)n;  // the scan's array serves the rows' counts first, the rounds' flags then
    size_t at = 0;
    auto take = [&at](size_t words) { const size_t o = at; at += lt_align_up(words * sizeof(int32_t), 8); return o; };
    p->uoff = take((size_t)n + 1);
    p->du = take((size_t)R);
    p->dv = take((size_t)R);
    p->flag = take((size_t)R + 1);
    p->bsum = take((size_t)sm_scan_blocks(span + 1));
    p->state = take(8);
    p->bytes = at;
    return true;
}
}  // namespace

extern "C" int lt_upper_edge_count(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, int64_t *d_count, void *stream) {
    LT_REQUIRE(d_rowptr && d_col && d_count, "lt_upper_edge_count: NULL pointer");
    LT_REQUIRE(n >= 1, "lt_upper_edge_count: n=%d < 1", n);
    LT_REQUIRE(nnz >= 0 && nnz < (int64_t)INT32_MAX, "lt_upper_edge_count: nnz=%lld outside [0, 2^31 - 1)", (long long)nnz);
    hipStream_t st = (hipStream_t)stream;
    LT_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(k_bp_upper, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, st, d_rowptr, d_col, (int)nnz, n,
                       (int32_t *)nullptr, (unsigned long long *)d_count);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" size_t lt_sample_balanced_workspace_bytes(int32_t n, int64_t E, int64_t round_draws) {
    bp_plan p;
    return bp_make_plan(n, E, round_draws, &p) ? p.bytes : 0;
}

extern "C" int lt_sample_balanced_philox(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, int64_t nnz, int64_t E, uint64_t seed,
                                         int64_t max_draws, int64_t round_draws, int32_t *out_u, int32_t *out_v, int64_t *info,
                                         void *ws, size_t ws_bytes, void *stream) {
    LT_REQUIRE(d_rowptr && d_col && out_u && out_v && info && ws, "lt_sample_balanced_philox: NULL pointer");
    LT_REQUIRE(n >= 1, "lt_sample_balanced_philox: n=%d < 1", n);
    LT_REQUIRE(nnz >= 0 && nnz < (int64_t)INT32_MAX, "lt_sample_balanced_philox: nnz=%lld outside [0, 2^31 - 1)", (long long)nnz);
    LT_REQUIRE(max_draws >= 0, "lt_sample_balanced_philox: max_draws=%lld < 0", (long long)max_draws);
    bp_plan p;
    LT_REQUIRE(bp_make_plan(n, E, round_draws, &p), "lt_sample_balanced_philox: E=%lld outside [0, 2^30) or round_draws=%lld outside [0, 2^24]",
               (long long)E, (long long)round_draws);
    LT_REQUIRE(ws_bytes >= p.bytes && ((uintptr_t)ws % 8) == 0,
               "lt_sample_balanced_philox: workspace needs %zu bytes (got %zu), 8-byte aligned", p.bytes, ws_bytes);
    hipStream_t st = (hipStream_t)stream;
    char *w = (char *)ws;
    int32_t *uoff = (int32_t *)(w + p.uoff), *du = (int32_t *)(w + p.du), *dv = (int32_t *)(w + p.dv);
    int32_t *flag = (int32_t *)(w + p.flag), *bsum = (int32_t *)(w + p.bsum);
    unsigned long long *state = (unsigned long long *)(w + p.state);
    auto blocks = [](long long count) { return dim3((unsigned)((count + 255) / 256)); };
    for (int x = 0; x < 8; ++x) info[x] = 0;

    // the rows' tails -> their offsets in the edge list; the total must be the caller's E
    hipLaunchKernelGGL(k_bp_upper, blocks((long long)n + 1), dim3(256), 0, st, d_rowptr, d_col, (int)nnz, n, uoff, (unsigned long long *)nullptr);
    LT_CHECK_LAUNCH();
    int rc = sm_scan(uoff, (long long)n + 1, bsum, st);
    if (rc != LT_OK) return rc;
    int32_t found = 0;
    LT_HIP(hipMemcpyAsync(&found, uoff + n, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    LT_REQUIRE((int64_t)found == E, "lt_sample_balanced_philox: E=%lld, but the graph stores %lld entries with col > row", (long long)E,
               (long long)found);
    info[0] = E;
    if (E == 0) return LT_OK;
    if (nnz > 0) {
        hipLaunchKernelGGL(k_bp_edges, blocks(nnz), dim3(256), 0, st, d_rowptr, d_col, (int)nnz, n, (const int32_t *)uoff, (long long)E, out_u,
                           out_v);
        LT_CHECK_LAUNCH();
    }
    const unsigned long long cap = max_draws ? (unsigned long long)max_draws : 64ull * (unsigned long long)E + 4096ull;
    const uint2 key = make_uint2((uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
    LT_HIP(hipMemsetAsync(state, 0, 4 * sizeof(unsigned long long), st));
    unsigned long long host_state[4] = {0, 0, 0, 0};
    unsigned long long t0 = 0;
    long long have = 0, rounds = 0;
    while (have < E && t0 < cap) {
        const long long cnt = (long long)(cap - t0 < (unsigned long long)p.R ? cap - t0 : (unsigned long long)p.R);
        hipLaunchKernelGGL(k_bp_flags, blocks(cnt + 1), dim3(256), 0, st, d_rowptr, d_col, (int)nnz, n, t0, cnt, key, du, dv, flag);
        LT_CHECK_LAUNCH();
        rc = sm_scan(flag, cnt + 1, bsum, st);
        if (rc != LT_OK) return rc;
        hipLaunchKernelGGL(k_bp_write, blocks(cnt), dim3(256), 0, st, (const int32_t *)flag, (const int32_t *)du, (const int32_t *)dv, t0, cnt,
                           have, (long long)E, out_u, out_v, state);
        LT_CHECK_LAUNCH();
        LT_HIP(hipMemcpyAsync(host_state, state, sizeof(host_state), hipMemcpyDeviceToHost, st));
        LT_HIP(hipStreamSynchronize(st));
        have = (long long)host_state[0];
        t0 += (unsigned long long)cnt;
        ++rounds;
    }
    info[2] = rounds;
    info[3] = (int64_t)host_state[2];
    if (have < E) {
        info[1] = (int64_t)t0;
        return lt_set_error(LT_ERR_UNSUPPORTED, "lt_sample_balanced_philox: %lld of %lld non-edges accepted within %llu draws (a graph this "
                            "dense leaves too few pairs that are adjacent in neither direction)", have, (long long)E, t0);
    }
    info[1] = (int64_t)host_state[1];
    return LT_OK;
}
