// lt_graph_create_device: the tables of lt_graph_create (lt_core.hip) built from a CSR that already lies in device memory, and
// lt_graph_table, the read-back that lets a test hold the two builders against each other word for word.
//
// What runs where.  Every array of nnz entries or of record words is formed by the kernels below and never leaves the device.
// The host sees rowptr (n + 1 words), the column totals (n words), the first column of every segment of a long row and the four
// counts per node of the incidence records; from those it forms what lt_graph_create forms with the same loops: max_row / max_col,
// hot_frac, tptr, the two segment tables, the work items and the record offsets.
//
// Nothing depends on the order in which atomics land: the atomics below are integer counts (column totals, local entries, touched
// nodes through a bitmap), one atomicMin (the first offending entry) and one LDS cursor whose slots a sort by unique keys reorders.
#include <string.h>

#include <algorithm>
#include <functional>
#include <new>
#include <vector>

#include "lt_internal.h"
#include "lt_radix.hip.h"

namespace {

// device scratch of one build, released on every way out
struct dev_tmp {
    std::vector<void *> held;
    ~dev_tmp() { for (void *q : held) (void)hipFree(q); }
    template <class T> hipError_t get(T **out, size_t count) {
        void *q = nullptr;
        *out = nullptr;
        hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        held.push_back(q);      // (may throw bad_alloc: the caller's handler reports it; q is then lost with the failed build)
        *out = (T *)q;
        return hipSuccess;
    }
};
// the graph under construction: freed unless the build hands it over (after the stream has drained: kernels may still write it)
struct graph_guard {
    lt_graph *g;
    hipStream_t st;
    ~graph_guard() {
        if (!g) return;
        (void)hipStreamSynchronize(st);
        free_graph(g);
    }
};
struct gb_flags {
    unsigned bad_k;             // smallest entry index that breaks a rule (0xffffffff: none)
    int too_big;                // a node passed LT_DL_MAX_T incidences
    unsigned long long n_local; // entries within LT_LOCAL_WINDOW of the diagonal
};

}  // namespace

// ---- validation: one thread per entry of the rows [0, nrows), whose offsets the host has checked ------------------------------
// Finds the entry's row by bisection of rowptr (kept in erow for the transpose), tests the column against [0, n) and against its
// left neighbour, and counts: the column totals, the local entries.  An entry that breaks a rule is never used as an index.
static __global__ __launch_bounds__(256) void k_gb_validate(const int32_t *__restrict__ rowptr, int nrows, int n,
                                                            const int32_t *__restrict__ col, int kend, int32_t *__restrict__ erow,
                                                            int32_t *__restrict__ colcnt, gb_flags *__restrict__ flags) {
    __shared__ int s_local;
    if (threadIdx.x == 0) s_local = 0;
    __syncthreads();
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < kend) {
        int lo = 0, hi = nrows;                     // rowptr[lo] <= k < rowptr[hi]
        while (hi - lo > 1) {
            const int mid = (int)(((long long)lo + hi) >> 1);
            if (rowptr[mid] <= k) lo = mid; else hi = mid;
        }
        const int r = lo, c = col[k];
        erow[k] = r;
        if (c < 0 || c >= n) atomicMin(&flags->bad_k, (unsigned)k);
        else if (k != rowptr[r] && col[k - 1] >= c) atomicMin(&flags->bad_k, (unsigned)k);
        else {
            atomicAdd(&colcnt[c], 1);
            if ((c >= r ? c - r : r - c) <= LT_LOCAL_WINDOW) atomicAdd(&s_local, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_local) atomicAdd(&flags->n_local, (unsigned long long)s_local);
}

// ---- transpose: a stable LSD radix sort of the row-major entries by column, 8 bits a pass (lt_radix.hip.h) -------------------
// Entry order inside a digit is kept, so after the last pass the entries of a column stand in row order -- the host's counting
// sort.  The payload is the entry's CSR index.
// the CSC arrays from the sorted entry indices: row, value and position inside the row travel with each entry
static __global__ __launch_bounds__(256) void k_gb_transpose_fill(const int32_t *__restrict__ src, int count, const int32_t *__restrict__ erow,
                                                                  const int32_t *__restrict__ rowptr, const float *__restrict__ val,
                                                                  int32_t *__restrict__ trow, float *__restrict__ tval,
                                                                  int32_t *__restrict__ tpos) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    const int k = src[p];
    if ((unsigned)k >= (unsigned)count) return;
    const int r = erow[k];
    trow[p] = r;
    tval[p] = val[k];
    if (tpos) tpos[p] = k - rowptr[r];
}
static __global__ __launch_bounds__(256) void k_gb_gather(const int32_t *__restrict__ src, long long src_n, const int32_t *__restrict__ idx,
                                                          int m, int32_t *__restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int k = idx[i];
    out[i] = (k >= 0 && k < src_n) ? src[k] : 0;
}

// ---- incidence records (lt_items.hip.h "INCIDENCE RECORD"; the host's build_delta_records) ------------------------------------
// Pass 1, one block per node v: its items (the column of v), its incidences (the column lengths of its items' rows, summed) and the
// nodes it touches (distinct rows over those columns: a bitmap of n bits in LDS, a node counts when its bit was clear).
static __global__ __launch_bounds__(256) void k_gb_rec_count(int n, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                             int4 *__restrict__ meta, gb_flags *__restrict__ flags) {
    extern __shared__ unsigned bm[];                      // (n + 31) / 32 words
    __shared__ unsigned long long s_inc;
    __shared__ int s_touched;
    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int b = tptr[v], e = tptr[v + 1];
    if (t == 0) { s_inc = 0; s_touched = 0; }
    for (int x = t; x < (n + 31) / 32; x += 256) bm[x] = 0u;
    __syncthreads();
    unsigned long long inc = 0;
    for (int i = b + t; i < e; i += 256) {
        const int r = trow[i];
        if ((unsigned)r < (unsigned)n) inc += (unsigned long long)(tptr[r + 1] - tptr[r]);
    }
    if (inc) atomicAdd(&s_inc, inc);
    __syncthreads();
    inc = s_inc;
    if (inc > LT_DL_MAX_T) {                              // the whole graph goes without records
        if (t == 0) { flags->too_big = 1; meta[v] = make_int4(0, e - b, 0, LT_DL_MAX_T + 1); }
        return;
    }
    int touched = 0;
    for (int i = b + w; i < e; i += 4) {                  // a wave per item, its lanes over the column of the item's row
        const int r = trow[i];
        if ((unsigned)r >= (unsigned)n) continue;
        for (int q = tptr[r] + lane; q < tptr[r + 1]; q += 64) {
            const int u = trow[q];
            if ((unsigned)u >= (unsigned)n) continue;
            const unsigned bit = 1u << (u & 31);
            if (!(atomicOr(&bm[u >> 5], bit) & bit)) ++touched;
        }
    }
    if (touched) atomicAdd(&s_touched, touched);
    __syncthreads();
    if (t == 0) meta[v] = make_int4(0, e - b, s_touched, (int)inc);
}
// Pass 3, one block per node: gathers the node's incidences (key = u << 16 | position in row u, ik = item << 16 | position, a) into
// LDS through a cursor, sorts them by key (bitonic, padded with 0xffffffff to a power of two; the keys of a node are unique, so the
// result is the host's std::sort whatever order the cursor gave), and writes items / (u, first | count << 16) / (a, ik).
// LDS: 12 bytes per slot, `cap` slots = the graph's largest incidence count rounded up to a power of two (at most 48 KB).
static __global__ __launch_bounds__(256) void k_gb_rec_fill(int n, const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                            const float *__restrict__ tval, const int32_t *__restrict__ tpos,
                                                            const int4 *__restrict__ meta, int32_t *__restrict__ rec, long long rec_words,
                                                            int cap) {
    extern __shared__ unsigned gb_slots[];                // [3 * cap]
    unsigned *skey = gb_slots;
    int *sik = (int *)(gb_slots + cap);
    float *sa = (float *)(gb_slots + 2 * (size_t)cap);
    __shared__ int s_cur;
    __shared__ int s_scan[256];
    const int v = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int4 m = meta[v];
    const int b = tptr[v], e = tptr[v + 1];
    const int ni = m.y, nt = m.z, ninc = m.w;
    if (ni != e - b || nt < 0 || ninc < 0 || ninc > cap || m.x < 0 || (long long)m.x + 2ll * ((long long)ni + nt + ninc) > rec_words) return;
    int32_t *items = rec + m.x, *list = items + 2 * ni, *ent = list + 2 * nt;
    int P = 1;
    while (P < ninc) P <<= 1;
    for (int j = t; j < P; j += 256) skey[j] = 0xffffffffu;
    if (t == 0) s_cur = 0;
    __syncthreads();
    for (int i = b + w; i < e; i += 4) {
        const int r = trow[i], item = i - b;
        if (lane == 0) { items[2 * item] = r; items[2 * item + 1] = __float_as_int(tval[i]); }
        if ((unsigned)r >= (unsigned)n) continue;
        for (int q = tptr[r] + lane; q < tptr[r + 1]; q += 64) {
            const int slot = atomicAdd(&s_cur, 1);
            if (slot < ninc) {
                skey[slot] = ((unsigned)trow[q] << 16) | (unsigned)tpos[q];
                sik[slot] = (item << 16) | tpos[q];
                sa[slot] = tval[q];
            }
        }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = t; x < P; x += 256) {
                const int y = x ^ j;
                if (y > x) {
                    const unsigned kx = skey[x], ky = skey[y];
                    if ((kx > ky) == ((x & k) == 0)) {
                        skey[x] = ky; skey[y] = kx;
                        const int ix = sik[x]; sik[x] = sik[y]; sik[y] = ix;
                        const float ax = sa[x]; sa[x] = sa[y]; sa[y] = ax;
                    }
                }
            }
            __syncthreads();
        }
    for (int x = t; x < ninc; x += 256) { ent[2 * x] = __float_as_int(sa[x]); ent[2 * x + 1] = sik[x]; }
    // the touched nodes: a group of equal u starts where u changes; its index is the number of starts before it
    const int per = (ninc + 255) / 256;
    const int lo = t * per < ninc ? t * per : ninc, hi = lo + per < ninc ? lo + per : ninc;
    int heads = 0;
    for (int x = lo; x < hi; ++x) heads += (x == 0 || (skey[x] >> 16) != (skey[x - 1] >> 16));
    s_scan[t] = heads;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int add = t >= off ? s_scan[t - off] : 0;
        __syncthreads();
        s_scan[t] += add;
        __syncthreads();
    }
    int nl = s_scan[t] - heads;
    for (int x = lo; x < hi; ++x) {
        const unsigned u = skey[x] >> 16;
        if (x != 0 && u == (skey[x - 1] >> 16)) continue;
        int f = x + 1;
        while (f < ninc && (skey[f] >> 16) == u) ++f;
        if (nl < nt) { list[2 * nl] = (int)u; list[2 * nl + 1] = x | ((f - x) << 16); }
        ++nl;
    }
}

// ---- the build --------------------------------------------------------------------------------------------------------------
#define GB_SYNC() LT_HIP(hipStreamSynchronize(st))
template <class T> static int gb_upload(T **dst, const std::vector<T> &src, hipStream_t st) {
    LT_HIP(hipMalloc((void **)dst, src.size() * sizeof(T)));
    LT_HIP(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st));
    return LT_OK;
}

static int gb_build(int32_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_col, const float *d_val, hipStream_t st,
                    lt_graph **out) {
    // host vectors that asynchronous copies read stay alive until the last synchronisation of this function
    std::vector<int32_t> rp((size_t)n + 1), cnt, tptr, segcol, w_e0, w_cnt, w_dst, meta;
    std::vector<int32_t> lrow, lptr(1, 0), slong, sbeg, qrow, qptr(1, 0), qlong, qbeg;
    dev_tmp tmp;
    graph_guard guard{new (std::nothrow) lt_graph(), st};
    lt_graph *g = guard.g;
    if (!g) return lt_set_error(LT_ERR_NOMEM, "lt_graph_create_device: out of host memory");
    g->n = n;
    g->nnz = nnz;
    const size_t pb = ((size_t)n + 1) * sizeof(int32_t);
    const size_t ib = ((size_t)nnz + LT_CSR_PAD) * sizeof(int32_t);
    const size_t fb = ((size_t)nnz + LT_CSR_PAD) * sizeof(float);
    const int cnnz = (int)nnz;

    // rowptr: checked completely on the host before any kernel reads col / val through it
    LT_HIP(hipMalloc((void **)&g->rowptr, pb));
    LT_HIP(hipMemcpyAsync(g->rowptr, d_rowptr, pb, hipMemcpyDeviceToDevice, st));
    LT_HIP(hipMemcpyAsync(rp.data(), d_rowptr, pb, hipMemcpyDeviceToHost, st));
    GB_SYNC();
    LT_REQUIRE(rp[0] == 0, "lt_graph_create_device: rowptr[0]=%d, expected 0", rp[0]);
    LT_REQUIRE((int64_t)rp[n] == nnz, "lt_graph_create_device: rowptr[n]=%d != nnz=%lld", rp[n], (long long)nnz);
    int32_t rbad = n, max_row = 0;                       // the first row whose offsets are out of range or decreasing
    for (int32_t r = 0; r < n; ++r) {
        const int32_t b = rp[r], e = rp[r + 1];
        if (b < 0 || (int64_t)e > nnz || b > e) { rbad = r; break; }
        if (e - b > max_row) max_row = e - b;
    }
    const int kend = rbad < n ? rp[rbad] : cnnz;         // the entries of the rows in front of it

    LT_HIP(hipMalloc((void **)&g->col, ib));
    LT_HIP(hipMalloc((void **)&g->val, fb));
    LT_HIP(hipMemsetAsync(g->col, 0, ib, st));
    LT_HIP(hipMemsetAsync(g->val, 0, fb, st));
    if (nnz > 0) {
        LT_HIP(hipMemcpyAsync(g->col, d_col, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        LT_HIP(hipMemcpyAsync(g->val, d_val, (size_t)nnz * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    int32_t *erow = nullptr, *colcnt = nullptr;
    gb_flags *flags = nullptr;
    LT_HIP(tmp.get(&erow, (size_t)nnz));
    LT_HIP(tmp.get(&colcnt, (size_t)n));
    LT_HIP(tmp.get(&flags, 1));
    LT_HIP(hipMemsetAsync(colcnt, 0, (size_t)(n > 0 ? n : 1) * sizeof(int32_t), st));
    LT_HIP(hipMemsetAsync(flags, 0, sizeof(gb_flags), st));
    LT_HIP(hipMemsetAsync(&flags->bad_k, 0xff, sizeof(unsigned), st));
    if (kend > 0) {
        hipLaunchKernelGGL(k_gb_validate, dim3((unsigned)(((long long)kend + 255) / 256)), dim3(256), 0, st, g->rowptr, rbad, n, g->col, kend, erow,
                           colcnt, flags);
        LT_CHECK_LAUNCH();
    }
    gb_flags hf;
    LT_HIP(hipMemcpyAsync(&hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st));
    GB_SYNC();
    if (hf.bad_k != 0xffffffffu) {                        // the first offending entry lies in front of row rbad
        const int k = (int)hf.bad_k;
        const int32_t r = (int32_t)(std::upper_bound(rp.begin(), rp.begin() + rbad + 1, k) - rp.begin()) - 1;
        int32_t c = 0;
        LT_HIP(hipMemcpyAsync(&c, g->col + k, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GB_SYNC();
        if (c < 0 || c >= n) return lt_set_error(LT_ERR_INVALID, "lt_graph_create_device: column %d out of range at row %d", c, r);
        return lt_set_error(LT_ERR_INVALID, "lt_graph_create_device: columns of row %d are not strictly increasing", r);
    }
    if (rbad < n) return lt_set_error(LT_ERR_INVALID, "lt_graph_create_device: rowptr not monotone at row %d", rbad);

    // column totals -> hot_frac, max_col, tptr (the host's loops)
    cnt.resize((size_t)n);
    if (n > 0) LT_HIP(hipMemcpyAsync(cnt.data(), colcnt, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    GB_SYNC();
    double hot_frac = 1.0;
    if (n > LT_HOT_COLUMNS && nnz > 0) {
        std::vector<int32_t> indeg(cnt);
        std::nth_element(indeg.begin(), indeg.begin() + LT_HOT_COLUMNS, indeg.end(), std::greater<int32_t>());
        int64_t hot = 0;
        for (int i = 0; i < LT_HOT_COLUMNS; ++i) hot += indeg[i];
        hot_frac = (double)hot / (double)nnz;
    }
    int32_t max_col = 0;
    tptr.assign((size_t)n + 1, 0);
    for (int32_t c = 0; c < n; ++c) {
        if (cnt[c] > max_col) max_col = cnt[c];
        tptr[(size_t)c + 1] = tptr[c] + cnt[c];
    }
    g->max_row_nnz = max_row;
    g->max_col_nnz = max_col;
    g->local_frac = nnz > 0 ? (float)((double)(int64_t)hf.n_local / (double)nnz) : 1.f;
    g->hot_frac = (float)hot_frac;
    LT_HIP(hipMalloc((void **)&g->tptr, pb));
    LT_HIP(hipMemcpyAsync(g->tptr, tptr.data(), pb, hipMemcpyHostToDevice, st));
    LT_HIP(hipMalloc((void **)&g->trow, ib));
    LT_HIP(hipMalloc((void **)&g->tval, fb));
    if (n <= 65534) {
        LT_HIP(hipMalloc((void **)&g->tpos, ib));
        LT_HIP(hipMemsetAsync(g->tpos, 0, ib, st));
    }

    // the transpose
    if (nnz > 0) {
        int bits = 1;
        while (bits < 31 && ((int64_t)1 << bits) < (int64_t)n) ++bits;
        const int passes = (bits + 7) / 8;
        int rounds, nblk;                                 // entries per block = 256 * rounds: at most 4096 blocks
        lt_radix_plan(nnz, &rounds, &nblk);
        int32_t *key[2] = {nullptr, nullptr}, *pay[2] = {nullptr, nullptr}, *hist = nullptr;
        for (int x = 0; x < 2; ++x) {
            LT_HIP(tmp.get(&key[x], (size_t)nnz));
            LT_HIP(tmp.get(&pay[x], (size_t)nnz));
        }
        LT_HIP(tmp.get(&hist, (size_t)256 * nblk));
        const int32_t *kin = g->col, *pin = nullptr;
        for (int p = 0; p < passes; ++p) {
            hipLaunchKernelGGL(k_gb_radix_hist, dim3((unsigned)nblk), dim3(256), 0, st, kin, cnnz, 8 * p, rounds, nblk, hist);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, hist, (long long)256 * nblk);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_gb_radix_scatter, dim3((unsigned)nblk), dim3(256), 0, st, kin, pin, cnnz, 8 * p, rounds, nblk, hist,
                               key[p & 1], pay[p & 1]);
            LT_CHECK_LAUNCH();
            kin = key[p & 1];
            pin = pay[p & 1];
        }
        hipLaunchKernelGGL(k_gb_transpose_fill, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, pin, cnnz, erow, g->rowptr, g->val,
                           g->trow, g->tval, g->tpos);
        LT_CHECK_LAUNCH();
    }

    // segment table of the long rows, the fp64 row kernel's own, and the work items of the tiled SpMM: lt_graph_create's loops
    for (int32_t r = 0; r < n; ++r) {
        if (rp[r + 1] - rp[r] <= LT_ROW_SEG) continue;
        const int32_t li = (int32_t)lrow.size();
        lrow.push_back(r);
        for (int32_t b = rp[r]; b < rp[r + 1]; b += LT_ROW_SEG) { slong.push_back(li); sbeg.push_back(b); }
        lptr.push_back((int32_t)sbeg.size());
    }
    g->p_n_long = (int32_t)lrow.size();
    g->p_n_seg = (int32_t)sbeg.size();
    if (g->p_n_long > 0) {
        int rc;
        if ((rc = gb_upload(&g->p_long_row, lrow, st)) || (rc = gb_upload(&g->p_long_segptr, lptr, st)) ||
            (rc = gb_upload(&g->p_seg_long, slong, st)) || (rc = gb_upload(&g->p_seg_begin, sbeg, st))) return rc;
        LT_HIP(hipMalloc((void **)&g->p_seg_scratch, (size_t)g->p_n_seg * LT_MAX_H * sizeof(float)));
        // the first column of every segment: the key its work item is sorted by
        int32_t *d_segcol = nullptr;
        LT_HIP(tmp.get(&d_segcol, sbeg.size()));
        hipLaunchKernelGGL(k_gb_gather, dim3((unsigned)((sbeg.size() + 255) / 256)), dim3(256), 0, st, g->col, (long long)nnz, g->p_seg_begin,
                           g->p_n_seg, d_segcol);
        LT_CHECK_LAUNCH();
        segcol.resize(sbeg.size());
        LT_HIP(hipMemcpyAsync(segcol.data(), d_segcol, sbeg.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        GB_SYNC();
    }
    for (int32_t r = 0; r < n; ++r) {
        if (rp[r + 1] - rp[r] <= LT_F64_LONG) continue;
        const int32_t li = (int32_t)qrow.size();
        qrow.push_back(r);
        for (int32_t b = rp[r]; b < rp[r + 1]; b += LT_F64_SEG) { qlong.push_back(li); qbeg.push_back(b); }
        qptr.push_back((int32_t)qbeg.size());
    }
    g->q_n_long = (int32_t)qrow.size();
    g->q_n_seg = (int32_t)qbeg.size();
    if (g->q_n_long > 0) {
        int rc;
        if ((rc = gb_upload(&g->q_long_row, qrow, st)) || (rc = gb_upload(&g->q_long_segptr, qptr, st)) ||
            (rc = gb_upload(&g->q_seg_long, qlong, st)) || (rc = gb_upload(&g->q_seg_begin, qbeg, st))) return rc;
    }
    {
        struct item { int32_t e0, cnt, dst; };
        std::vector<item> items;
        items.reserve((size_t)n + sbeg.size());
        for (size_t sg = 0; sg < sbeg.size(); ++sg) {
            const int32_t r = lrow[slong[sg]];
            const int32_t left = rp[r + 1] - sbeg[sg];
            items.push_back({sbeg[sg], left < LT_ROW_SEG ? left : LT_ROW_SEG, n + (int32_t)sg});
        }
        const int32_t *sc = segcol.data();
        std::stable_sort(items.begin(), items.end(), [sc, n](const item &a, const item &b) { return sc[a.dst - n] < sc[b.dst - n]; });
        const size_t nseg_items = items.size();
        constexpr int NCLS = LT_ROW_SEG / 16 + 1;
        size_t cls_n[NCLS] = {};
        for (int32_t r = 0; r < n; ++r) {
            const int32_t d = rp[r + 1] - rp[r];
            if (d <= LT_ROW_SEG) cls_n[(d + 15) / 16]++;
        }
        size_t cls_at[NCLS], at = nseg_items;
        for (int k = NCLS - 1; k >= 0; --k) { cls_at[k] = at; at += cls_n[k]; }
        items.resize(at);
        for (int32_t r = 0; r < n; ++r) {
            const int32_t d = rp[r + 1] - rp[r];
            if (d <= LT_ROW_SEG) items[cls_at[(d + 15) / 16]++] = {rp[r], d, r};
        }
        g->w_n = (int32_t)items.size();
        if (g->w_n > 0) {
            w_e0.resize(items.size()); w_cnt.resize(items.size()); w_dst.resize(items.size());
            for (size_t i = 0; i < items.size(); ++i) { w_e0[i] = items[i].e0; w_cnt[i] = items[i].cnt; w_dst[i] = items[i].dst; }
            int rc;
            if ((rc = gb_upload(&g->w_e0, w_e0, st)) || (rc = gb_upload(&g->w_cnt, w_cnt, st)) || (rc = gb_upload(&g->w_dst, w_dst, st))) return rc;
        }
    }
    GB_SYNC();
    lt_graph_build_cv(g);

    // the fused DELTA route's records, under the host's conditions; running out of device memory only means "no records"
    if (g->p_n_long == 0 && g->tpos && n >= 1 && n <= 65534 && max_col < 32768) {
        int4 *d_meta = nullptr;
        int32_t *d_rec = nullptr;
        bool ok = hipMalloc((void **)&d_meta, (size_t)n * sizeof(int4)) == hipSuccess;
        int64_t words = 0;
        int32_t max_t = 0, max_tu = 0;
        int64_t touched = 0;
        if (ok) {
            const size_t bm_bytes = (size_t)((n + 31) / 32) * sizeof(unsigned);
            hipLaunchKernelGGL(k_gb_rec_count, dim3((unsigned)n), dim3(256), bm_bytes, st, n, g->tptr, g->trow, d_meta, flags);
            meta.resize((size_t)n * 4);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyAsync(meta.data(), d_meta, (size_t)n * sizeof(int4), hipMemcpyDeviceToHost, st) == hipSuccess &&
                 hipMemcpyAsync(&hf, flags, sizeof(hf), hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
        if (ok) ok = hf.too_big == 0;
        if (ok) {                                          // offsets, with the host's arithmetic
            for (int32_t v = 0; v < n && ok; ++v) {
                int32_t *m = &meta[(size_t)v * 4];
                if (words > LT_DL_MAX_WORDS) { ok = false; break; }
                m[0] = (int32_t)words;
                words += 2 * ((int64_t)m[1] + m[2] + m[3]);
                if (m[3] > max_t) max_t = m[3];
                if (m[2] > max_tu) max_tu = m[2];
                touched += m[2];
            }
            if (words > LT_DL_MAX_WORDS) ok = false;
        }
        if (ok) ok = hipMalloc((void **)&d_rec, ((size_t)words + 4) * sizeof(int32_t)) == hipSuccess;
        if (ok) ok = hipMemsetAsync(d_rec, 0, ((size_t)words + 4) * sizeof(int32_t), st) == hipSuccess &&
                     hipMemcpyAsync(d_meta, meta.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            int cap = 1;
            while (cap < max_t) cap <<= 1;                 // max_t <= LT_DL_MAX_T: at most 48 KB of slots
            hipLaunchKernelGGL(k_gb_rec_fill, dim3((unsigned)n), dim3(256), (size_t)cap * 12, st, n, g->tptr, g->trow, g->tval, g->tpos,
                               d_meta, d_rec, (long long)words, cap);
            ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
        }
        if (ok) {
            g->dl_meta = d_meta;
            g->dl_rec = d_rec;
            g->dl_max_t = max_t;
            g->dl_max_tu = max_tu;
            g->dl_touch_frac = (double)touched / ((double)n * n);
        } else {
            (void)hipGetLastError();
            (void)hipStreamSynchronize(st);
            (void)hipFree(d_meta);
            (void)hipFree(d_rec);
        }
    }
    GB_SYNC();
    guard.g = nullptr;
    *out = g;
    return LT_OK;
}

extern "C" int lt_graph_create_device(int32_t n, int64_t nnz, const int32_t *d_rowptr, const int32_t *d_col, const float *d_val,
                                      void *stream, lt_graph **out) {
    LT_REQUIRE(out != nullptr, "lt_graph_create_device: out is NULL");
    *out = nullptr;
    LT_REQUIRE(n >= 0 && nnz >= 0, "lt_graph_create_device: negative size (n=%d nnz=%lld)", n, (long long)nnz);
    LT_REQUIRE(nnz < (int64_t)INT32_MAX, "lt_graph_create_device: nnz=%lld does not fit int32 row pointers", (long long)nnz);
    LT_REQUIRE(d_rowptr != nullptr, "lt_graph_create_device: rowptr is NULL");
    LT_REQUIRE(nnz == 0 || (d_col != nullptr && d_val != nullptr), "lt_graph_create_device: col/val is NULL");
    try {
        return gb_build(n, nnz, d_rowptr, d_col, d_val, (hipStream_t)stream, out);
    } catch (const std::bad_alloc &) {
        return lt_set_error(LT_ERR_NOMEM, "lt_graph_create_device: host allocation for %d rows failed", n);
    }
}

// ---- lt_graph_table: a table of the graph, copied to host memory ------------------------------------------------------------
extern "C" int lt_graph_table(const lt_graph *g, int32_t which, void *dst, int64_t capacity_bytes, int64_t *bytes) {
    LT_REQUIRE(g != nullptr, "lt_graph_table: graph is NULL");
    LT_REQUIRE(bytes != nullptr, "lt_graph_table: bytes is NULL");
    LT_REQUIRE(which >= 0 && which < LT_TABLE_COUNT, "lt_graph_table: which=%d", which);
    LT_REQUIRE(dst == nullptr || capacity_bytes >= 0, "lt_graph_table: negative capacity");
    const int64_t n = g->n, nnz = g->nnz, w = sizeof(int32_t);
    double scalars[LT_TABLE_SCALAR_COUNT] = {
        (double)g->n, (double)g->nnz, (double)g->max_row_nnz, (double)g->max_col_nnz, (double)g->local_frac, (double)g->hot_frac,
        (double)g->p_n_long, (double)g->p_n_seg, (double)g->q_n_long, (double)g->q_n_seg, (double)g->w_n, (double)g->dl_max_t,
        (double)g->dl_max_tu, g->dl_touch_frac, g->tpos ? 1.0 : 0.0, g->cv ? 1.0 : 0.0, (g->dl_meta && g->dl_rec) ? 1.0 : 0.0};
    const void *src = nullptr;
    int64_t size = 0;
    bool host = false;
    switch (which) {
    case LT_TABLE_ROWPTR: src = g->rowptr; size = (n + 1) * w; break;
    case LT_TABLE_COL: src = g->col; size = (nnz + LT_CSR_PAD) * w; break;
    case LT_TABLE_VAL: src = g->val; size = (nnz + LT_CSR_PAD) * w; break;
    case LT_TABLE_TPTR: src = g->tptr; size = (n + 1) * w; break;
    case LT_TABLE_TROW: src = g->trow; size = nnz * w; break;
    case LT_TABLE_TVAL: src = g->tval; size = nnz * w; break;
    case LT_TABLE_TPOS: src = g->tpos; size = (nnz + LT_CSR_PAD) * w; break;
    case LT_TABLE_CV: src = g->cv; size = (nnz + LT_CSR_PAD) * 2 * w; break;
    case LT_TABLE_DL_META: src = (g->dl_meta && g->dl_rec) ? g->dl_meta : nullptr; size = n * 4 * w; break;
    case LT_TABLE_DL_REC:
        if (g->dl_meta && g->dl_rec && n > 0) {             // the last node's record ends the array (+ 4 zero words)
            int32_t m[4];
            LT_HIP(hipMemcpy(m, g->dl_meta + (n - 1), sizeof(m), hipMemcpyDeviceToHost));
            src = g->dl_rec;
            size = ((int64_t)m[0] + 2 * ((int64_t)m[1] + m[2] + m[3]) + 4) * w;
        }
        break;
    case LT_TABLE_P_LONG_ROW: src = g->p_long_row; size = (int64_t)g->p_n_long * w; break;
    case LT_TABLE_P_LONG_SEGPTR: src = g->p_long_segptr; size = ((int64_t)g->p_n_long + 1) * w; break;
    case LT_TABLE_P_SEG_LONG: src = g->p_seg_long; size = (int64_t)g->p_n_seg * w; break;
    case LT_TABLE_P_SEG_BEGIN: src = g->p_seg_begin; size = (int64_t)g->p_n_seg * w; break;
    case LT_TABLE_Q_LONG_ROW: src = g->q_long_row; size = (int64_t)g->q_n_long * w; break;
    case LT_TABLE_Q_LONG_SEGPTR: src = g->q_long_segptr; size = ((int64_t)g->q_n_long + 1) * w; break;
    case LT_TABLE_Q_SEG_LONG: src = g->q_seg_long; size = (int64_t)g->q_n_seg * w; break;
    case LT_TABLE_Q_SEG_BEGIN: src = g->q_seg_begin; size = (int64_t)g->q_n_seg * w; break;
    case LT_TABLE_W_E0: src = g->w_e0; size = (int64_t)g->w_n * w; break;
    case LT_TABLE_W_CNT: src = g->w_cnt; size = (int64_t)g->w_n * w; break;
    case LT_TABLE_W_DST: src = g->w_dst; size = (int64_t)g->w_n * w; break;
    default: src = scalars; size = sizeof(scalars); host = true; break;      // LT_TABLE_SCALARS
    }
    if (!src) size = 0;                                      // an absent optional table
    *bytes = size;
    if (!dst || size == 0) return LT_OK;
    if (capacity_bytes < size)
        return lt_set_error(LT_ERR_WORKSPACE, "lt_graph_table: %lld bytes given, %lld needed", (long long)capacity_bytes, (long long)size);
    if (host) memcpy(dst, src, (size_t)size);
    else LT_HIP(hipMemcpy(dst, src, (size_t)size, hipMemcpyDeviceToHost));
    return LT_OK;
}
