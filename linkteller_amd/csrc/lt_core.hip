// liblinkteller_hip: error plumbing + the device-resident graph handle.
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "lt_internal.h"

static thread_local char g_err[512] = "";

int lt_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" const char *lt_last_error(void) { return g_err; }

// ---- tuning knobs -------------------------------------------------------------------------------
static long long env_ll(const char *name, long long dflt) {
    const char *e = getenv(name);
    return (e && *e) ? atoll(e) : dflt;
}
static lt_tuning tuning_defaults() {
    lt_tuning t;
    t.tiled_min_bytes = env_ll("LT_SPMM_TILED_MIN_BYTES", (long long)32 << 20);
    t.chunk_budget = env_ll("LT_CHUNK_BUDGET_BYTES", (long long)1 << 30);
    if (t.chunk_budget <= 0) t.chunk_budget = (long long)1 << 30;
    const long long p = env_ll("LT_FULL_P", 0);
    t.full_p = (p == 8 || p == 16 || p == 32) ? (int)p : 0;
    t.long_par = getenv("LT_LONG_PAR") ? (env_ll("LT_LONG_PAR", 0) != 0 ? 1 : 0) : -1;
    t.overlap = env_ll("LT_OVERLAP", 1) != 0 ? 1 : 0;
    t.item_bits = env_ll("LT_ITEM_BITS", 1) != 0 ? 1 : 0;
    const long long w = env_ll("LT_WIDE_MIN_HP", 24);
    t.wide_min_hp = w > 0 ? (int)w : 24;
    const long long pk = env_ll("LT_PROBE_KSLICE", 0);
    t.probe_kslice = pk > 0 ? (int)pk : 0;
    t.pair_marks = env_ll("LT_PAIR_MARKS", (long long)1 << 22);
    t.hub_short_side = getenv("LT_HUB_SHORT_SIDE") ? (env_ll("LT_HUB_SHORT_SIDE", 0) != 0 ? 1 : 0) : -1;
    t.bits_max_bytes = env_ll("LT_BITS_MAX_BYTES", (long long)128 << 20);
    t.tiled_big = 0;
    t.stageb_rows = env_ll("LT_STAGEB_ROWS", 1) != 0 ? 1 : 0;
    t.defer_cref = env_ll("LT_DEFER_CREF", 1) != 0 ? 1 : 0;
    t.s1_f32 = env_ll("LT_S1_F32", 1) != 0 ? 1 : 0;
    t.z_on_demand = getenv("LT_Z_ON_DEMAND") ? (env_ll("LT_Z_ON_DEMAND", 0) != 0 ? 1 : 0) : -1;
    t.aggregate_first = getenv("LT_AGGREGATE_FIRST") ? (env_ll("LT_AGGREGATE_FIRST", 0) != 0 ? 1 : 0) : -1;
    t.feature_delta = getenv("LT_FEATURE_DELTA") ? (env_ll("LT_FEATURE_DELTA", 0) != 0 ? 1 : 0) : -1;
    t.delta_fused = env_ll("LT_DELTA_FUSED", 1) != 0 ? 1 : 0;
    t.records_early = env_ll("LT_RECORDS_EARLY", 1) != 0 ? 1 : 0;
    t.feature_ring = env_ll("LT_FEATURE_RING", 0) != 0 ? (env_ll("LT_FEATURE_RING", 0) < 0 ? -1 : 1) : 0;
    t.feature_flags = env_ll("LT_FEATURE_FLAGS", 1) != 0 ? 1 : 0;
    t.feature_lists = env_ll("LT_FEATURE_LISTS", 1) != 0 ? 1 : 0;
    t.export_sparse = env_ll("LT_EXPORT_SPARSE", 1) != 0 ? 1 : 0;
    t.pair_list = env_ll("LT_PAIR_LIST", 1) != 0 ? 1 : 0;
    t.i8_split = env_ll("LT_I8_SPLIT", 1) != 0 ? 1 : 0;
    t.gcn3_product_gather = env_ll("LT_GCN3_PRODUCT_GATHER", 1) != 0 ? 1 : 0;
    t.export_zero_blocks = (int)std::min<long long>(4096, std::max<long long>(1, env_ll("LT_EXPORT_ZERO_BLOCKS", 16)));
    t.export_zero_inflight = (int)std::min<long long>(64, std::max<long long>(1, env_ll("LT_EXPORT_ZERO_INFLIGHT", 4)));
    t.export_zero_share2 = (int)std::min<long long>(100, std::max<long long>(0, env_ll("LT_EXPORT_ZERO_SHARE2", 15)));
    t.export_zero_share = (int)std::min<long long>(100, std::max<long long>(0, env_ll("LT_EXPORT_ZERO_SHARE", 35)));
    t.export_compact = (int)std::min<long long>(2, std::max<long long>(0, env_ll("LT_EXPORT_COMPACT", 1)));
    t.export_early = (int)std::min<long long>(2, std::max<long long>(0, env_ll("LT_EXPORT_EARLY", 0)));
    t.host_poll = env_ll("LT_HOST_POLL", 1) != 0 ? 1 : 0;
    t.host_poll_sentinel = (long long)LT_LANDING_SENTINEL;
    t.feature_stagger = (int)env_ll("LT_FEATURE_STAGGER", 0);
    const long long xb = env_ll("LT_XF64_BLOCKS", 96);
    t.xf64_blocks = xb > 0 && xb <= 4096 ? (int)xb : 96;
    const long long frm = env_ll("LT_FEATURE_RING_MIN_ROWS", 1024);
    t.feature_ring_min_rows = frm > 2 ? (int)(frm > (1 << 30) ? (1 << 30) : frm) : 2;
    t.profile_every = 1;
    return t;
}
lt_tuning &lt_tune() {
    static lt_tuning t = tuning_defaults();
    return t;
}
extern "C" int lt_set_tuning(const char *key, long long value) {
    LT_REQUIRE(key != nullptr, "lt_set_tuning: key is NULL");
    lt_tuning &t = lt_tune();
    const lt_tuning d = tuning_defaults();
    const bool reset = value == LT_TUNING_DEFAULT;
    if (!strcmp(key, "tiled_min_bytes")) t.tiled_min_bytes = reset ? d.tiled_min_bytes : value;
    else if (!strcmp(key, "chunk_budget_bytes")) {
        LT_REQUIRE(reset || value > 0, "lt_set_tuning: chunk_budget_bytes must be positive");
        t.chunk_budget = reset ? d.chunk_budget : value;
    } else if (!strcmp(key, "full_p")) {
        LT_REQUIRE(reset || value == 0 || value == 8 || value == 16 || value == 32, "lt_set_tuning: full_p must be 0, 8, 16 or 32");
        t.full_p = reset ? d.full_p : (int)value;
    } else if (!strcmp(key, "long_par")) {
        LT_REQUIRE(reset || value == 0 || value == 1, "lt_set_tuning: long_par must be 0 or 1");
        t.long_par = reset ? d.long_par : (int)value;
    } else if (!strcmp(key, "overlap")) t.overlap = reset ? d.overlap : (value != 0);
    else if (!strcmp(key, "item_bits")) t.item_bits = reset ? d.item_bits : (value != 0);
    else if (!strcmp(key, "wide_min_hp")) {
        LT_REQUIRE(reset || value > 0, "lt_set_tuning: wide_min_hp must be positive");
        t.wide_min_hp = reset ? d.wide_min_hp : (int)value;
    } else if (!strcmp(key, "pair_marks")) t.pair_marks = reset ? d.pair_marks : value;
    else if (!strcmp(key, "hub_short_side")) t.hub_short_side = reset ? d.hub_short_side : (value < 0 ? -1 : (value != 0));
    else if (!strcmp(key, "bits_max_bytes")) t.bits_max_bytes = reset ? d.bits_max_bytes : value;
    else if (!strcmp(key, "tiled_big")) t.tiled_big = reset ? 0 : (value != 0);
    else if (!strcmp(key, "s1_f32")) t.s1_f32 = reset ? d.s1_f32 : (value != 0);
    else if (!strcmp(key, "defer_cref")) t.defer_cref = reset ? d.defer_cref : (value != 0);
    else if (!strcmp(key, "delta_fused")) t.delta_fused = reset ? d.delta_fused : (value != 0);
    else if (!strcmp(key, "records_early")) t.records_early = reset ? d.records_early : (value != 0);
    else if (!strcmp(key, "profile_every")) t.profile_every = reset ? 1 : (value >= 1 ? (int)(value > 1000000 ? 1000000 : value) : 1);
    else if (!strcmp(key, "z_on_demand")) t.z_on_demand = reset ? d.z_on_demand : (value < 0 ? -1 : (value != 0));
    else if (!strcmp(key, "stageb_rows")) t.stageb_rows = reset ? d.stageb_rows : (value != 0);
    else if (!strcmp(key, "aggregate_first")) t.aggregate_first = reset ? d.aggregate_first : (value < 0 ? -1 : (value != 0));
    else if (!strcmp(key, "feature_delta")) t.feature_delta = reset ? d.feature_delta : (value < 0 ? -1 : (value != 0));
    else if (!strcmp(key, "feature_ring")) t.feature_ring = reset ? d.feature_ring : (value < 0 ? -1 : (value != 0));
    else if (!strcmp(key, "feature_flags")) t.feature_flags = reset ? d.feature_flags : (value != 0);
    else if (!strcmp(key, "feature_lists")) t.feature_lists = reset ? d.feature_lists : (value != 0);
    else if (!strcmp(key, "pair_list")) t.pair_list = reset ? d.pair_list : (value != 0);
    else if (!strcmp(key, "i8_split")) t.i8_split = reset ? d.i8_split : (value != 0);
    else if (!strcmp(key, "gcn3_product_gather")) t.gcn3_product_gather = reset ? d.gcn3_product_gather : (value != 0);
    else if (!strcmp(key, "export_sparse")) t.export_sparse = reset ? d.export_sparse : (value != 0);
    else if (!strcmp(key, "export_zero_share2")) t.export_zero_share2 = reset ? d.export_zero_share2 : (int)std::min<long long>(100, std::max<long long>(0, value));
    else if (!strcmp(key, "export_zero_share")) t.export_zero_share = reset ? d.export_zero_share : (int)std::min<long long>(100, std::max<long long>(0, value));
    else if (!strcmp(key, "export_zero_inflight")) t.export_zero_inflight = reset ? d.export_zero_inflight : (int)std::min<long long>(64, std::max<long long>(1, value));
    else if (!strcmp(key, "export_compact")) {
        LT_REQUIRE(reset || (value >= 0 && value <= 2), "lt_set_tuning: export_compact must be 0, 1 or 2");
        t.export_compact = reset ? d.export_compact : (int)value;
    }
    else if (!strcmp(key, "export_early")) {
        LT_REQUIRE(reset || (value >= 0 && value <= 2), "lt_set_tuning: export_early must be 0, 1 or 2");
        t.export_early = reset ? d.export_early : (int)value;
    }
    else if (!strcmp(key, "host_poll")) {
        LT_REQUIRE(reset || value == 0 || value == 1, "lt_set_tuning: host_poll must be 0 or 1");
        t.host_poll = reset ? d.host_poll : (int)value;
    }
    else if (!strcmp(key, "host_poll_sentinel")) {
        LT_REQUIRE(reset || (value >= 0 && value <= 0xffffffffLL), "lt_set_tuning: host_poll_sentinel must be a 32-bit pattern");
        t.host_poll_sentinel = reset ? d.host_poll_sentinel : value;
    }
    else if (!strcmp(key, "export_zero_blocks")) t.export_zero_blocks = reset ? d.export_zero_blocks : (int)std::min<long long>(4096, std::max<long long>(1, value));
    else if (!strcmp(key, "feature_stagger")) {
        LT_REQUIRE(reset || (value >= 0 && value < (1 << 24)), "lt_set_tuning: feature_stagger out of range");
        t.feature_stagger = reset ? d.feature_stagger : (int)value;
    }
    else if (!strcmp(key, "xf64_blocks")) {
        LT_REQUIRE(reset || (value >= 1 && value <= 4096), "lt_set_tuning: xf64_blocks must be in [1, 4096]");
        t.xf64_blocks = reset ? d.xf64_blocks : (int)value;
    }
    else if (!strcmp(key, "feature_ring_min_rows")) {
        LT_REQUIRE(reset || value >= 2, "lt_set_tuning: feature_ring_min_rows must be >= 2");
        t.feature_ring_min_rows = reset ? d.feature_ring_min_rows : (int)(value > (1 << 30) ? (1 << 30) : value);
    } else if (!strcmp(key, "probe_kslice")) {
        LT_REQUIRE(reset || (value >= 0 && value <= 1 << 20), "lt_set_tuning: probe_kslice must be >= 0");
        t.probe_kslice = reset ? d.probe_kslice : (int)value;
    } else return lt_set_error(LT_ERR_INVALID, "lt_set_tuning: unknown key '%s'", key);
    return LT_OK;
}
extern "C" int lt_abi_version(void) { return LT_ABI_VERSION; }

extern "C" int lt_device_count(int *count) {
    LT_REQUIRE(count != nullptr, "lt_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // clear the sticky "no device" state
        n = 0;
    }
    *count = n;
    return LT_OK;
}

static __global__ void k_interleave_cv(const int32_t *__restrict__ col, const float *__restrict__ val, long long total, int2 *__restrict__ cv) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) cv[i] = make_int2(col[i], __float_as_int(val[i]));
}

// (col, val) interleaved for the tiled SpMM, on the graphs that take it (a failure to allocate only means the kernel reads the two streams)
void lt_graph_build_cv(lt_graph *g) {
    const int64_t nnz = g->nnz;
    if (lt_tiled_wanted(g, 256) && nnz > 0) {
        int2 *cv = nullptr;
        if (hipMalloc((void **)&cv, ((size_t)nnz + LT_CSR_PAD) * sizeof(int2)) == hipSuccess) {
            hipLaunchKernelGGL(k_interleave_cv, dim3((unsigned)(((size_t)nnz + LT_CSR_PAD + 255) / 256)), dim3(256), 0, 0, g->col, g->val,
                               (long long)nnz + LT_CSR_PAD, cv);
            if (hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess) g->cv = cv;
            else (void)hipFree(cv);
        } else {
            (void)hipGetLastError();
        }
    }
}

// The fused DELTA route's per-node incidence records (lt_items.hip.h "INCIDENCE RECORD"; lt_influence.hip k_delta_probe_finish):
// for node v, its items (the CSC column of v) and the entries (u, position in row u) that hold an item, grouped by u ascending,
// a node's entries in entry order.  Sum over the nodes of |R_v| * column lengths entries -- 1.6 M at twitch size, 25 MB; built on
// the host from the CSC arrays lt_graph_create has in hand.  Only for graphs whose largest record stays small (no hub rows).
struct dl_host {
    std::vector<int32_t> meta, rec;
    int32_t max_t = 0, max_tu = 0;
};
static bool build_delta_records(int32_t n, const int32_t *tptr, const int32_t *trow, const float *tval, const int32_t *tpos,
                                int32_t max_col, dl_host &out) {
    if (n < 1 || n > 65534 || max_col >= 32768 || tpos == nullptr) return false;
    unsigned T = std::thread::hardware_concurrency();
    if (T < 1) T = 1;
    if (T > 8) T = 8;
    if ((int64_t)n < 4096) T = 1;
    auto run = [&](auto &&fn) {
        if (T == 1) { fn(0u); return; }
        struct joiner {
            std::vector<std::thread> th;
            ~joiner() { for (auto &x : th) if (x.joinable()) x.join(); }
        } j;
        j.th.reserve(T);
        for (unsigned t = 0; t < T; ++t) j.th.emplace_back(fn, t);
    };
    out.meta.assign((size_t)n * 4, 0);
    std::vector<int> too_big(T, 0);
    // pass 1: items, incidences and touched nodes of every node
    run([&](unsigned t) {
        std::vector<int32_t> stamp((size_t)n, -1);
        const int32_t v0 = (int32_t)((int64_t)n * t / T), v1 = (int32_t)((int64_t)n * (t + 1) / T);
        for (int32_t v = v0; v < v1; ++v) {
            int64_t inc = 0;
            int32_t touched = 0;
            for (int32_t i = tptr[v]; i < tptr[v + 1] && inc <= LT_DL_MAX_T; ++i) {
                const int32_t r = trow[i];
                inc += tptr[r + 1] - tptr[r];
                if (inc > LT_DL_MAX_T) break;
                for (int32_t q = tptr[r]; q < tptr[r + 1]; ++q)
                    if (stamp[trow[q]] != v) { stamp[trow[q]] = v; ++touched; }
            }
            if (inc > LT_DL_MAX_T) { too_big[t] = 1; return; }
            out.meta[(size_t)v * 4 + 1] = tptr[v + 1] - tptr[v];
            out.meta[(size_t)v * 4 + 2] = touched;
            out.meta[(size_t)v * 4 + 3] = (int32_t)inc;
        }
    });
    for (unsigned t = 0; t < T; ++t) if (too_big[t]) return false;
    int64_t words = 0;
    for (int32_t v = 0; v < n; ++v) {
        int32_t *m = &out.meta[(size_t)v * 4];
        if (words > LT_DL_MAX_WORDS) return false;
        m[0] = (int32_t)words;
        words += 2 * ((int64_t)m[1] + m[2] + m[3]);
        if (m[3] > out.max_t) out.max_t = m[3];
        if (m[2] > out.max_tu) out.max_tu = m[2];
    }
    if (words > LT_DL_MAX_WORDS) return false;
    out.rec.assign((size_t)words + 4, 0);
    // pass 2: the records
    run([&](unsigned t) {
        struct inc_t { uint32_t key; int32_t ik; float a; };
        std::vector<inc_t> buf;
        buf.reserve(LT_DL_MAX_T);
        const int32_t v0 = (int32_t)((int64_t)n * t / T), v1 = (int32_t)((int64_t)n * (t + 1) / T);
        for (int32_t v = v0; v < v1; ++v) {
            const int32_t *m = &out.meta[(size_t)v * 4];
            int32_t *items = &out.rec[(size_t)m[0]], *list = items + 2 * m[1], *ent = list + 2 * m[2];
            buf.clear();
            for (int32_t i = tptr[v]; i < tptr[v + 1]; ++i) {
                const int32_t r = trow[i], item = i - tptr[v];
                items[2 * item] = r;
                memcpy(&items[2 * item + 1], &tval[i], sizeof(float));
                for (int32_t q = tptr[r]; q < tptr[r + 1]; ++q)
                    buf.push_back({((uint32_t)trow[q] << 16) | (uint32_t)tpos[q], (item << 16) | tpos[q], tval[q]});
            }
            std::sort(buf.begin(), buf.end(), [](const inc_t &x, const inc_t &y) { return x.key < y.key; });
            int32_t nl = 0;
            for (size_t e = 0; e < buf.size();) {
                size_t f = e;
                const uint32_t u = buf[e].key >> 16;
                while (f < buf.size() && (buf[f].key >> 16) == u) ++f;
                list[2 * nl] = (int32_t)u;
                list[2 * nl + 1] = (int32_t)e | ((int32_t)(f - e) << 16);
                ++nl;
                e = f;
            }
            for (size_t e = 0; e < buf.size(); ++e) {
                memcpy(&ent[2 * e], &buf[e].a, sizeof(float));
                ent[2 * e + 1] = buf[e].ik;
            }
        }
    });
    return true;
}

extern "C" int lt_graph_create(int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                               const float *val, lt_graph **out) {
    LT_REQUIRE(out != nullptr, "lt_graph_create: out is NULL");
    *out = nullptr;
    LT_REQUIRE(n >= 0 && nnz >= 0, "lt_graph_create: negative size (n=%d nnz=%lld)", n, (long long)nnz);
    LT_REQUIRE(nnz < (int64_t)INT32_MAX, "lt_graph_create: nnz=%lld does not fit int32 row pointers", (long long)nnz);
    LT_REQUIRE(rowptr != nullptr, "lt_graph_create: rowptr is NULL");
    LT_REQUIRE(nnz == 0 || (col != nullptr && val != nullptr), "lt_graph_create: col/val is NULL");
    LT_REQUIRE(rowptr[0] == 0, "lt_graph_create: rowptr[0]=%d, expected 0", rowptr[0]);
    LT_REQUIRE((int64_t)rowptr[n] == nnz, "lt_graph_create: rowptr[n]=%d != nnz=%lld", rowptr[n], (long long)nnz);

    // validate + build the transpose on the host: a counting sort that keeps the rows ascending inside each column,
    // split over threads by contiguous row ranges (thread t counts / fills its rows; its cursors start behind the
    // entries of the threads with lower rows, so the result does not depend on the thread count).  A 77 M-entry graph:
    // ~1 s single-threaded, most of it the scattered fill.
    std::vector<int32_t> tptr;
    std::unique_ptr<int32_t[]> trow;     // (uninitialised: the threads of the fill touch the pages, not a zeroing pass)
    std::unique_ptr<float[]> tval;
    std::unique_ptr<int32_t[]> tpos;     // small graphs only (lt_graph::tpos)
    int32_t max_row = 0, max_col = 0;
    int64_t n_local = 0;
    double hot_frac = 1.0;
    try {
        tptr.assign((size_t)n + 1, 0);
        unsigned T = 1;
        if (nnz >= (1 << 20)) {
            T = std::thread::hardware_concurrency();
            if (T < 1) T = 1;
            if (T > 16) T = 16;
            while (T > 1 && (size_t)T * (size_t)n > ((size_t)1 << 28)) --T;   // <= 1 GiB of per-thread counters
            if ((int64_t)T > (int64_t)n) T = n > 0 ? (unsigned)n : 1;
        }
        // row ranges with about nnz / T entries each
        std::vector<int32_t> rb(T + 1, n);
        rb[0] = 0;
        for (unsigned t = 1; t < T; ++t) {
            const int64_t want = nnz / T * t;
            // (on a malformed, non-monotone rowptr the search lands anywhere in [0, n]; the pass below reports the row)
            rb[t] = (int32_t)(std::lower_bound(rowptr, rowptr + n, (int32_t)want) - rowptr);
            if (rb[t] < rb[t - 1]) rb[t] = rb[t - 1];
        }
        struct part { int64_t n_local = 0; int32_t max_row = 0; int32_t bad_row = -1, bad_col = 0; int bad_kind = 0; };
        std::vector<part> parts(T);
        std::vector<std::vector<int32_t>> cnt(T);
        for (unsigned t = 0; t < T; ++t) cnt[t].assign((size_t)n, 0);
        auto run = [&](auto &&fn) {
            if (T == 1) { fn(0u); return; }
            // (a std::thread constructor may throw std::system_error: the threads already running are joined before
            // it travels on -- destroying a joinable std::thread would call std::terminate)
            struct joiner {
                std::vector<std::thread> th;
                ~joiner() { for (auto &x : th) if (x.joinable()) x.join(); }
            } j;
            j.th.reserve(T);
            for (unsigned t = 0; t < T; ++t) j.th.emplace_back(fn, t);
        };
        run([&](unsigned t) {
            part &pt = parts[t];
            int32_t *ct = cnt[t].data();
            for (int32_t r = rb[t]; r < rb[t + 1]; ++r) {
                const int32_t b = rowptr[r], e = rowptr[r + 1];
                // (each thread starts in the middle of rowptr: every offset is range-checked before col[] is read)
                if (b < 0 || (int64_t)e > nnz || b > e) { pt.bad_row = r; pt.bad_kind = 1; return; }
                if (e - b > pt.max_row) pt.max_row = e - b;
                for (int32_t k = b; k < e; ++k) {
                    const int32_t c = col[k];
                    if (c < 0 || c >= n) { pt.bad_row = r; pt.bad_col = c; pt.bad_kind = 2; return; }
                    if (k != b && col[k - 1] >= c) { pt.bad_row = r; pt.bad_kind = 3; return; }
                    pt.n_local += (c >= r ? c - r : r - c) <= LT_LOCAL_WINDOW;
                    ct[c]++;
                }
            }
        });
        for (unsigned t = 0; t < T; ++t) {       // the first offending row, as a single pass would report it
            const part &pt = parts[t];
            if (pt.bad_kind == 1) return lt_set_error(LT_ERR_INVALID, "lt_graph_create: rowptr not monotone at row %d", pt.bad_row);
            if (pt.bad_kind == 2) return lt_set_error(LT_ERR_INVALID, "lt_graph_create: column %d out of range at row %d", pt.bad_col, pt.bad_row);
            if (pt.bad_kind == 3) return lt_set_error(LT_ERR_INVALID, "lt_graph_create: columns of row %d are not strictly increasing", pt.bad_row);
            n_local += pt.n_local;
            if (pt.max_row > max_row) max_row = pt.max_row;
        }
        // column totals -> tptr; the per-thread counters become per-thread cursors (column ranges in parallel)
        run([&](unsigned t) {
            const int32_t c0 = (int32_t)((int64_t)n * t / T), c1 = (int32_t)((int64_t)n * (t + 1) / T);
            for (int32_t c = c0; c < c1; ++c) {
                int32_t tot = 0;
                for (unsigned u = 0; u < T; ++u) tot += cnt[u][c];
                tptr[(size_t)c + 1] = tot;
            }
        });
        if (n > LT_HOT_COLUMNS && nnz > 0) {   // entries that read the LT_HOT_COLUMNS most-read columns
            std::vector<int32_t> indeg(tptr.begin() + 1, tptr.end());
            std::nth_element(indeg.begin(), indeg.begin() + LT_HOT_COLUMNS, indeg.end(), std::greater<int32_t>());
            int64_t hot = 0;
            for (int i = 0; i < LT_HOT_COLUMNS; ++i) hot += indeg[i];
            hot_frac = (double)hot / (double)nnz;
        }
        for (int32_t c = 0; c < n; ++c) {
            if (tptr[(size_t)c + 1] > max_col) max_col = tptr[(size_t)c + 1];
            tptr[(size_t)c + 1] += tptr[c];
        }
        run([&](unsigned t) {
            const int32_t c0 = (int32_t)((int64_t)n * t / T), c1 = (int32_t)((int64_t)n * (t + 1) / T);
            for (int32_t c = c0; c < c1; ++c) {
                int32_t at = tptr[c];
                for (unsigned u = 0; u < T; ++u) { const int32_t k = cnt[u][c]; cnt[u][c] = at; at += k; }
            }
        });
        trow.reset(new int32_t[(size_t)nnz + 1]);
        tval.reset(new float[(size_t)nnz + 1]);
        int32_t *trow_p = trow.get();
        float *tval_p = tval.get();
        if (n <= 65534) tpos.reset(new int32_t[(size_t)nnz + 1]);
        int32_t *tpos_p = tpos.get();
        run([&](unsigned t) {
            int32_t *cur = cnt[t].data();
            for (int32_t r = rb[t]; r < rb[t + 1]; ++r)
                for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
                    const int32_t p = cur[col[k]]++;
                    trow_p[p] = r;
                    tval_p[p] = val[k];
                    if (tpos_p) tpos_p[p] = k - rowptr[r];
                }
        });
    } catch (const std::bad_alloc &) {
        return lt_set_error(LT_ERR_NOMEM, "lt_graph_create: host allocation for %lld entries failed", (long long)nnz);
    } catch (const std::system_error &) {
        return lt_set_error(LT_ERR_NOMEM, "lt_graph_create: could not start the host threads");
    }

    lt_graph *g = new (std::nothrow) lt_graph();
    if (!g) return lt_set_error(LT_ERR_NOMEM, "lt_graph_create: out of host memory");
    g->n = n;
    g->nnz = nnz;
    g->max_row_nnz = max_row;
    g->max_col_nnz = max_col;
    g->local_frac = nnz > 0 ? (float)((double)n_local / (double)nnz) : 1.f;
    g->hot_frac = (float)hot_frac;
    const size_t pb = ((size_t)n + 1) * sizeof(int32_t);
    // +LT_CSR_PAD zero entries: the LDS-ring probe kernel reads (col, val) in 4-entry scalar bursts that
    // may run past a row's (and so the array's) end; padded columns are 0 (a valid node), values 0
    const size_t ib = ((size_t)nnz + LT_CSR_PAD) * sizeof(int32_t);
    const size_t fb = ((size_t)nnz + LT_CSR_PAD) * sizeof(float);
#define G_HIP(call)                                                                        \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) {                                                            \
            free_graph(g);                                                                 \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                  \
    } while (0)
    G_HIP(hipMalloc((void **)&g->rowptr, pb));
    G_HIP(hipMalloc((void **)&g->col, ib));
    G_HIP(hipMalloc((void **)&g->val, fb));
    G_HIP(hipMemset(g->col, 0, ib));
    G_HIP(hipMemset(g->val, 0, fb));
    G_HIP(hipMalloc((void **)&g->tptr, pb));
    G_HIP(hipMalloc((void **)&g->trow, ib));
    G_HIP(hipMalloc((void **)&g->tval, fb));
    G_HIP(hipMemcpy(g->rowptr, rowptr, pb, hipMemcpyHostToDevice));
    G_HIP(hipMemcpy(g->tptr, tptr.data(), pb, hipMemcpyHostToDevice));
    if (nnz > 0) {
        G_HIP(hipMemcpy(g->col, col, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        G_HIP(hipMemcpy(g->val, val, (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
        G_HIP(hipMemcpy(g->trow, trow.get(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        G_HIP(hipMemcpy(g->tval, tval.get(), (size_t)nnz * sizeof(float), hipMemcpyHostToDevice));
    }
    if (tpos) {
        G_HIP(hipMalloc((void **)&g->tpos, ib));
        G_HIP(hipMemset(g->tpos, 0, ib));
        if (nnz > 0) G_HIP(hipMemcpy(g->tpos, tpos.get(), (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    // segment table of the long rows (LT_ROW_SEG entries per segment)
    {
        std::vector<int32_t> lrow, lptr(1, 0), slong, sbeg;
        for (int32_t r = 0; r < n; ++r) {
            if (rowptr[r + 1] - rowptr[r] <= LT_ROW_SEG) continue;
            const int32_t li = (int32_t)lrow.size();
            lrow.push_back(r);
            for (int32_t b = rowptr[r]; b < rowptr[r + 1]; b += LT_ROW_SEG) {
                slong.push_back(li);
                sbeg.push_back(b);
            }
            lptr.push_back((int32_t)sbeg.size());
        }
        g->p_n_long = (int32_t)lrow.size();
        g->p_n_seg = (int32_t)sbeg.size();
        if (g->p_n_long > 0) {
            G_HIP(hipMalloc((void **)&g->p_long_row, lrow.size() * sizeof(int32_t)));
            G_HIP(hipMalloc((void **)&g->p_long_segptr, lptr.size() * sizeof(int32_t)));
            G_HIP(hipMalloc((void **)&g->p_seg_long, slong.size() * sizeof(int32_t)));
            G_HIP(hipMalloc((void **)&g->p_seg_begin, sbeg.size() * sizeof(int32_t)));
            G_HIP(hipMemcpy(g->p_long_row, lrow.data(), lrow.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            G_HIP(hipMemcpy(g->p_long_segptr, lptr.data(), lptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            G_HIP(hipMemcpy(g->p_seg_long, slong.data(), slong.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            G_HIP(hipMemcpy(g->p_seg_begin, sbeg.data(), sbeg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            G_HIP(hipMalloc((void **)&g->p_seg_scratch, (size_t)g->p_n_seg * LT_MAX_H * sizeof(float)));
        }
        {   // the fp64 row kernel's own segment table (lt_internal.h: LT_F64_LONG / LT_F64_SEG)
            std::vector<int32_t> qrow, qptr(1, 0), qlong, qbeg;
            for (int32_t r = 0; r < n; ++r) {
                if (rowptr[r + 1] - rowptr[r] <= LT_F64_LONG) continue;
                const int32_t li = (int32_t)qrow.size();
                qrow.push_back(r);
                for (int32_t b_ = rowptr[r]; b_ < rowptr[r + 1]; b_ += LT_F64_SEG) {
                    qlong.push_back(li);
                    qbeg.push_back(b_);
                }
                qptr.push_back((int32_t)qbeg.size());
            }
            g->q_n_long = (int32_t)qrow.size();
            g->q_n_seg = (int32_t)qbeg.size();
            if (g->q_n_long > 0) {
                G_HIP(hipMalloc((void **)&g->q_long_row, qrow.size() * sizeof(int32_t)));
                G_HIP(hipMalloc((void **)&g->q_long_segptr, qptr.size() * sizeof(int32_t)));
                G_HIP(hipMalloc((void **)&g->q_seg_long, qlong.size() * sizeof(int32_t)));
                G_HIP(hipMalloc((void **)&g->q_seg_begin, qbeg.size() * sizeof(int32_t)));
                G_HIP(hipMemcpy(g->q_long_row, qrow.data(), qrow.size() * sizeof(int32_t), hipMemcpyHostToDevice));
                G_HIP(hipMemcpy(g->q_long_segptr, qptr.data(), qptr.size() * sizeof(int32_t), hipMemcpyHostToDevice));
                G_HIP(hipMemcpy(g->q_seg_long, qlong.data(), qlong.size() * sizeof(int32_t), hipMemcpyHostToDevice));
                G_HIP(hipMemcpy(g->q_seg_begin, qbeg.data(), qbeg.size() * sizeof(int32_t), hipMemcpyHostToDevice));
            }
        }
        // work items of the tiled SpMM: segments by first column, then short rows by length class (16 entries)
        struct item { int32_t e0, cnt, dst; };
        std::vector<item> items;
        try {
            items.reserve((size_t)n + sbeg.size());
            for (size_t sg = 0; sg < sbeg.size(); ++sg) {
                const int32_t r = lrow[slong[sg]];
                const int32_t left = rowptr[r + 1] - sbeg[sg];
                items.push_back({sbeg[sg], left < LT_ROW_SEG ? left : LT_ROW_SEG, n + (int32_t)sg});
            }
            std::stable_sort(items.begin(), items.end(), [col](const item &a, const item &b) { return col[a.e0] < col[b.e0]; });
            // the short rows by length class (16 entries), longest first, row order kept inside a class: a counting sort
            const size_t nseg_items = items.size();
            constexpr int NCLS = LT_ROW_SEG / 16 + 1;
            size_t cls_n[NCLS] = {};
            for (int32_t r = 0; r < n; ++r) {
                const int32_t d = rowptr[r + 1] - rowptr[r];
                if (d <= LT_ROW_SEG) cls_n[(d + 15) / 16]++;
            }
            size_t cls_at[NCLS], at = nseg_items;
            for (int k = NCLS - 1; k >= 0; --k) { cls_at[k] = at; at += cls_n[k]; }
            items.resize(at);
            for (int32_t r = 0; r < n; ++r) {
                const int32_t d = rowptr[r + 1] - rowptr[r];
                if (d <= LT_ROW_SEG) items[cls_at[(d + 15) / 16]++] = {rowptr[r], d, r};
            }
        } catch (const std::bad_alloc &) {
            free_graph(g);
            return lt_set_error(LT_ERR_NOMEM, "lt_graph_create: host allocation of the work list failed");
        }
        g->w_n = (int32_t)items.size();
        if (g->w_n > 0) {
            std::vector<int32_t> tmp(items.size());
            const size_t wb = items.size() * sizeof(int32_t);
            G_HIP(hipMalloc((void **)&g->w_e0, wb));
            G_HIP(hipMalloc((void **)&g->w_cnt, wb));
            G_HIP(hipMalloc((void **)&g->w_dst, wb));
            for (size_t i = 0; i < items.size(); ++i) tmp[i] = items[i].e0;
            G_HIP(hipMemcpy(g->w_e0, tmp.data(), wb, hipMemcpyHostToDevice));
            for (size_t i = 0; i < items.size(); ++i) tmp[i] = items[i].cnt;
            G_HIP(hipMemcpy(g->w_cnt, tmp.data(), wb, hipMemcpyHostToDevice));
            for (size_t i = 0; i < items.size(); ++i) tmp[i] = items[i].dst;
            G_HIP(hipMemcpy(g->w_dst, tmp.data(), wb, hipMemcpyHostToDevice));
        }
    }
    lt_graph_build_cv(g);
    // the fused DELTA route's per-node records (graphs without hub rows; a failure to build them only means the route is not taken)
    if (g->p_n_long == 0 && tpos) {
        try {
            dl_host dl;
            if (build_delta_records(n, tptr.data(), trow.get(), tval.get(), tpos.get(), max_col, dl)) {
                // (not G_HIP: device memory that does not suffice for the records must not fail the whole create -- the buffers
                // are released, the error cleared and the graph simply has no records: the item kernels serve it)
                hipError_t e = hipMalloc((void **)&g->dl_meta, (size_t)n * sizeof(int4));
                if (e == hipSuccess) e = hipMalloc((void **)&g->dl_rec, dl.rec.size() * sizeof(int32_t));
                if (e == hipSuccess) e = hipMemcpy(g->dl_meta, dl.meta.data(), (size_t)n * sizeof(int4), hipMemcpyHostToDevice);
                if (e == hipSuccess) e = hipMemcpy(g->dl_rec, dl.rec.data(), dl.rec.size() * sizeof(int32_t), hipMemcpyHostToDevice);
                if (e == hipSuccess) {
                    g->dl_max_t = dl.max_t;
                    g->dl_max_tu = dl.max_tu;
                    double touched = 0.0;
                    for (int32_t v = 0; v < n; ++v) touched += dl.meta[(size_t)v * 4 + 2];
                    g->dl_touch_frac = touched / ((double)n * n);
                } else {
                    (void)hipGetLastError();
                    (void)hipFree(g->dl_meta); (void)hipFree(g->dl_rec);
                    g->dl_meta = nullptr; g->dl_rec = nullptr;
                }
            }
        } catch (const std::bad_alloc &) {
        } catch (const std::system_error &) {
        }
    }
#undef G_HIP
    *out = g;
    return LT_OK;
}

extern "C" int lt_graph_destroy(lt_graph *g) {
    free_graph(g);
    return LT_OK;
}

// Host only: the incidence records of a CSR, as lt_graph_create would build them (tests/test_records.py).  The transpose is
// formed here by a plain counting pass (lt_graph_create's threaded one is validated against the same CSR on the device side).
extern "C" int lt_graph_records_host(int32_t n, int64_t nnz, const int32_t *rowptr, const int32_t *col, const float *val,
                                     int32_t *meta, int32_t *rec, int64_t rec_capacity, int64_t *rec_words) {
    LT_REQUIRE(n >= 1 && nnz >= 0 && rowptr && (nnz == 0 || (col && val)) && meta && rec_words,
               "lt_graph_records_host: n=%d nnz=%lld or a NULL argument", n, (long long)nnz);
    LT_REQUIRE(rowptr[0] == 0 && (int64_t)rowptr[n] == nnz, "lt_graph_records_host: rowptr[0] / rowptr[n] do not frame %lld entries",
               (long long)nnz);
    try {
        std::vector<int32_t> tptr((size_t)n + 1, 0), trow((size_t)nnz + 1), tpos((size_t)nnz + 1);
        std::vector<float> tval((size_t)nnz + 1);
        int32_t max_row = 0, max_col = 0;
        for (int32_t r = 0; r < n; ++r) {
            LT_REQUIRE(rowptr[r + 1] >= rowptr[r], "lt_graph_records_host: rowptr is not monotone at row %d", r);
            max_row = std::max(max_row, rowptr[r + 1] - rowptr[r]);
            for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
                LT_REQUIRE(col[k] >= 0 && col[k] < n, "lt_graph_records_host: column %d out of range in row %d", col[k], r);
                ++tptr[(size_t)col[k] + 1];
            }
        }
        for (int32_t c = 0; c < n; ++c) {
            max_col = std::max(max_col, tptr[(size_t)c + 1]);
            tptr[(size_t)c + 1] += tptr[c];
        }
        std::vector<int32_t> cur(tptr.begin(), tptr.end() - 1);
        for (int32_t r = 0; r < n; ++r)
            for (int32_t k = rowptr[r]; k < rowptr[r + 1]; ++k) {
                const int32_t p = cur[col[k]]++;
                trow[p] = r;
                tval[p] = val[k];
                tpos[p] = k - rowptr[r];
            }
        dl_host dl;
        if (max_row > LT_ROW_SEG || !build_delta_records(n, tptr.data(), trow.data(), tval.data(), tpos.data(), max_col, dl))
            return lt_set_error(LT_ERR_UNSUPPORTED, "lt_graph_records_host: this graph gets no incidence records");
        const int64_t words = (int64_t)dl.rec.size() - 4;          // (the builder pads its buffer by 4 words)
        *rec_words = words;
        memcpy(meta, dl.meta.data(), (size_t)n * 4 * sizeof(int32_t));
        if (rec) {
            if (rec_capacity < words)
                return lt_set_error(LT_ERR_WORKSPACE, "lt_graph_records_host: %lld words given, %lld needed", (long long)rec_capacity,
                                    (long long)words);
            memcpy(rec, dl.rec.data(), (size_t)words * sizeof(int32_t));
        }
    } catch (const std::bad_alloc &) {
        return lt_set_error(LT_ERR_NOMEM, "lt_graph_records_host: host allocation failed");
    } catch (const std::system_error &) {
        return lt_set_error(LT_ERR_NOMEM, "lt_graph_records_host: could not start the host threads");
    }
    return LT_OK;
}

extern "C" int lt_graph_info(const lt_graph *g, int32_t *n, int64_t *nnz, int32_t *max_row_nnz) {
    LT_REQUIRE(g != nullptr, "lt_graph_info: graph is NULL");
    if (n) *n = g->n;
    if (nnz) *nnz = g->nnz;
    if (max_row_nnz) *max_row_nnz = g->max_row_nnz;
    return LT_OK;
}

// ---- lt_graph_reached_rows: the rows of at least min_entries entries that a list of probe nodes reaches in one hop -----------
// (R_v = {r : A_hat[r, v] != 0} over the probes' CSC columns.)  What the ranks of a multi-GPU run agree on before they split the
// shared hub rows of the on-demand pre-activation (lt_baseline_form_rows_fp64): every rank runs this on the WHOLE probe list.
// The list comes out in no particular order (a flag word per row, first arrival appends): sort it before use.
static __global__ __launch_bounds__(256) void k_reached_rows(const int32_t *__restrict__ probes, int n_probe, int n,
                                                             const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow,
                                                             const int32_t *__restrict__ rowptr, int min_entries,
                                                             int32_t *__restrict__ flags, int32_t *__restrict__ rows,
                                                             int32_t *__restrict__ count) {
    // one wave per probe: its column's entries in strides of 64
    const int wave = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= n_probe) return;
    const int v = probes[wave];
    if ((unsigned)v >= (unsigned)n) return;
    for (int e = tptr[v] + lane; e < tptr[v + 1]; e += 64) {
        const int r = trow[e];
        if (rowptr[r + 1] - rowptr[r] < min_entries) continue;
        if (atomicExch(&flags[r], 1) == 0) rows[atomicAdd(count, 1)] = r;
    }
}
extern "C" int lt_graph_reached_rows(const lt_graph *g, const int32_t *probes, int32_t n_probe, int32_t min_entries, int32_t *flags,
                                     int32_t *rows, int32_t *count, void *stream) {
    LT_REQUIRE(g != nullptr, "lt_graph_reached_rows: graph is NULL");
    LT_REQUIRE(n_probe >= 0 && (n_probe == 0 || probes != nullptr), "lt_graph_reached_rows: bad probe list");
    LT_REQUIRE(flags && rows && count, "lt_graph_reached_rows: NULL output / scratch pointer");
    hipStream_t st = (hipStream_t)stream;
    LT_HIP(hipMemsetAsync(flags, 0, (size_t)(g->n > 0 ? g->n : 1) * sizeof(int32_t), st));
    LT_HIP(hipMemsetAsync(count, 0, sizeof(int32_t), st));
    if (n_probe == 0 || g->n == 0) return LT_OK;
    hipLaunchKernelGGL(k_reached_rows, dim3((unsigned)((n_probe + 3) / 4)), dim3(256), 0, st, probes, n_probe, g->n, g->tptr, g->trow,
                       g->rowptr, min_entries, flags, rows, count);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// ---- node ids out of range: the flag words the kernels raise (include/linkteller_hip.h, lt_node_check) -------------------------
// Two words of mapped host memory per process (portable: every device writes through its own alias): [0] a probe list,
// [1] an observed list held an id outside [0, n).  Coherent, said explicitly (what the default means depends on the environment):
// a host-landed call that placed its values by look reads the words WITHOUT a stream wait, on the argument that the launches
// that raise them had ended before the finish launch began.  That holds only if a kernel's plain store to this memory is in host
// memory when the kernel has ended -- true of fine-grained memory (never cached in the L2 past the end-of-kernel release), not
// promised for coarse-grained memory between two kernels of one stream.
namespace {
int32_t *g_node_err_host = nullptr;
bool g_node_err_tried = false;
}
int32_t *lt_node_err_dev() {
    if (!g_node_err_tried) {
        g_node_err_tried = true;
        if (hipHostMalloc((void **)&g_node_err_host, 2 * sizeof(int32_t), hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) == hipSuccess)
            g_node_err_host[0] = g_node_err_host[1] = 0;
        else { g_node_err_host = nullptr; (void)hipGetLastError(); }
    }
    if (!g_node_err_host) return nullptr;
    int32_t *dev = nullptr;
    if (hipHostGetDevicePointer((void **)&dev, g_node_err_host, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return dev;
}
extern "C" int lt_node_check(int32_t *bad_probe, int32_t *bad_observe) {
    int p = 0, o = 0;
    if (g_node_err_host) {
        volatile int32_t *w = g_node_err_host;
        p = w[0] != 0; o = w[1] != 0;
        w[0] = 0; w[1] = 0;
    }
    if (bad_probe) *bad_probe = p;
    if (bad_observe) *bad_observe = o;
    if (p || o)
        return lt_set_error(LT_ERR_INDEX, "node id out of range in the %s of an earlier call (its rows are meaningless)",
                            p && o ? "probe and observed lists" : (p ? "probe list" : "observed list"));
    return LT_OK;
}
// (what the probe primitives call on entry: a flag raised by an earlier call's kernels is reported now, nothing is enqueued)
int lt_node_err_pending() {
    if (!g_node_err_host) return LT_OK;
    volatile int32_t *w = g_node_err_host;
    if (w[0] == 0 && w[1] == 0) return LT_OK;
    return lt_node_check(nullptr, nullptr);
}

// ---- lt_export_rows_f64: the finished rows -> float64, straight into host memory ------------------------------------------
// The reference fills influence_val (np.zeros -> float64, attacker.py:216) with n_test^2 `.norm().item()` round trips
// (attacker.py:227-229).  Here the matrix leaves the device ONCE, already widened: one lane reads two scores and stores two
// doubles, a wave instruction writes 1 KiB of contiguous bytes -- into device memory, or over PCIe into pinned host memory
// (hipHostMalloc / hipHostRegister: the kernel writes through the device-side alias of the buffer, no staging copy, no
// second launch; the bytes are the caller's once the stream has drained).
static __global__ __launch_bounds__(256) void k_export_rows_f64(const float *__restrict__ src, long lds, int rows, int cols,
                                                                 double *__restrict__ dst, long ldd) {
    const int half = (cols + 1) >> 1;
    const long total = (long)rows * half;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) {
        const int r = (int)(k / half), c = (int)(k % half) * 2;
        const float *s = src + r * lds + c;
        double *d = dst + r * ldd + c;
        if (c + 1 < cols) {
            const float a = s[0], b = s[1];
            if ((reinterpret_cast<uintptr_t>(d) & 15) == 0) *reinterpret_cast<double2 *>(d) = make_double2((double)a, (double)b);
            else { d[0] = (double)a; d[1] = (double)b; }
        } else d[0] = (double)s[0];
    }
}

// dst may be host memory: only pinned (device-mapped) memory can be written by a kernel -- resolve its device-side alias and
// refuse pageable pointers instead of faulting
int lt_export_resolve(double *dst, double **dev, const char *who, bool *is_host) {
    hipPointerAttribute_t at;
    hipError_t e = hipPointerGetAttributes(&at, dst);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return lt_set_error(LT_ERR_INVALID, "%s: dst is neither device memory nor pinned host memory (%s)", who, hipGetErrorString(e));
    }
    *dev = dst;
    if (is_host) *is_host = at.type == hipMemoryTypeHost;
    if (at.type == hipMemoryTypeHost) {
        LT_REQUIRE(at.devicePointer != nullptr, "%s: pinned dst has no device-side alias", who);
        *dev = (double *)at.devicePointer;
    } else if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged) {
        return lt_set_error(LT_ERR_INVALID, "%s: dst is pageable host memory (pin it: hipHostMalloc / hipHostRegister)", who);
    }
    return LT_OK;
}
int lt_export_rows_dev(const float *src, int64_t lds, int32_t rows, int32_t cols, double *d, int64_t ldd, hipStream_t stream) {
    const long total = (long)rows * ((cols + 1) / 2);
    if (total <= 0) return LT_OK;
    long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_export_rows_f64, dim3((unsigned)blocks), dim3(256), 0, stream, src, (long)lds, rows, cols, d, (long)ldd);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_export_rows_f64(const float *src, int64_t lds, int32_t rows, int32_t cols, double *dst, int64_t ldd,
                                  void *stream) {
    LT_REQUIRE(rows >= 0 && cols >= 0, "lt_export_rows_f64: negative shape");
    if (rows == 0 || cols == 0) return LT_OK;
    LT_REQUIRE(src && dst, "lt_export_rows_f64: NULL pointer");
    LT_REQUIRE(lds >= cols && ldd >= cols, "lt_export_rows_f64: leading dimension smaller than the row");
    double *d = nullptr;
    const int rc = lt_export_resolve(dst, &d, "lt_export_rows_f64");
    if (rc) return rc;
    return lt_export_rows_dev(src, lds, rows, cols, d, ldd, (hipStream_t)stream);
}

// ---- per-kernel event timing ------------------------------------------------------------------
unsigned g_lt_profile_mask = 0;   // bit k set: kernel class k is bracketed by events
namespace {
struct prof_rec { int id; hipEvent_t a, b; };
std::vector<prof_rec> g_recs;
std::vector<hipEvent_t> g_free;
hipEvent_t g_open[LT_K_COUNT];
unsigned g_tick[LT_K_COUNT];
// "profile_every" samples whole CALLS of the probe primitive, not single scopes: a class that opens several scopes per call (a
// chunked call, the three sites of the fp64 product) would otherwise alias to one of them; scopes outside any call keep a
// tick per class
int g_call_depth = 0;
bool g_call_sampled = true;
unsigned g_call_tick = 0;
int64_t g_calls_sampled = 0;
hipEvent_t take_event() {
    if (!g_free.empty()) { hipEvent_t e = g_free.back(); g_free.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}
}  // namespace

bool lt_profile_sample(int id) {
    if (g_call_depth > 0) return g_call_sampled;
    const unsigned every = (unsigned)lt_tune().profile_every;
    return every <= 1u || (g_tick[id]++ % every) == 0u;
}
void lt_profile_call_begin() {
    if (g_call_depth++ > 0 || !g_lt_profile_mask) return;
    const unsigned every = (unsigned)lt_tune().profile_every;
    g_call_sampled = every <= 1u || (g_call_tick++ % every) == 0u;
    if (g_call_sampled) ++g_calls_sampled;
}
void lt_profile_call_end() { if (g_call_depth > 0) --g_call_depth; }
void lt_profile_begin(int id, hipStream_t st) {
    hipEvent_t e = take_event();
    (void)hipEventRecord(e, st);
    g_open[id] = e;
}
void lt_profile_end(int id, hipStream_t st) {
    hipEvent_t e = take_event();
    (void)hipEventRecord(e, st);
    g_recs.push_back({id, g_open[id], e});
}

extern "C" int lt_profile_reset(void) {
    for (auto &r : g_recs) { g_free.push_back(r.a); g_free.push_back(r.b); }
    g_recs.clear();
    return LT_OK;
}
extern "C" int lt_profile_enable(int mask) {
    lt_profile_reset();
    for (auto &t : g_tick) t = 0;
    g_call_tick = 0;
    g_calls_sampled = 0;
    g_lt_profile_mask = (unsigned)mask;
    return LT_OK;
}
extern "C" int lt_profile_calls(int64_t *calls_sampled) {
    if (calls_sampled) *calls_sampled = g_calls_sampled;
    return LT_OK;
}
extern "C" int lt_profile_summary(int kernel_id, double *total_ms, int64_t *launches) {
    LT_REQUIRE(kernel_id >= 0 && kernel_id < LT_K_COUNT, "lt_profile_summary: kernel_id=%d", kernel_id);
    double tot = 0.0;
    int64_t cnt = 0;
    for (auto &r : g_recs) {
        if (r.id != kernel_id) continue;
        LT_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        LT_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        tot += ms;
        ++cnt;
    }
    if (total_ms) *total_ms = tot;
    if (launches) *launches = cnt;
    return LT_OK;
}
