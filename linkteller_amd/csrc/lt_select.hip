// Edge recovery on the device: the m first cells of the strict lower triangle of an fp32 score matrix (reference
// attack_stats_all.py:106-116: n_pos = ceil(ratio * n_total), np.argpartition(pred, -n_pos)[-n_pos:] over the saved score list).
//
// The cells (i, j), j < i, of scores[n, lds] are ranked by the TOTAL order "value descending, then flat index i * n + j
// ascending" (-0.0 counts as +0.0), so the answer is a pure function of the input even when the m-th value is tied -- the normal
// case here: >= 90 % of an influence matrix is exact +0.  A radix select over order-preserving 32-bit keys finds the m-th key,
// then an ORDERED compaction writes the selection in ascending flat index:
//   k_sel_hist    x 4  one 8-bit digit each, top digit first: histogram of the digit among the cells whose higher digits match
//                      the prefix fixed so far.  The pick of the previous digit is the launch's prologue (every block walks the
//                      256 bins of the previous histogram itself; block 0 records the state for the launches behind it).
//   k_sel_count        prologue: the last pick -> threshold key, cells to take among the tied ones, out_info.  Then (above, tied)
//                      per block.
//   k_sel_scan         one block: exclusive scans of the blocks' tied cells and of the cells each block takes.
//   k_sel_write        a cell is taken if key > threshold, or key == threshold and its rank among the tied cells (in flat
//                      order, exclusive) < tied-taken; it goes to out[block offset + rank among the block's taken cells].
// Every block owns a contiguous range of the FLATTENED triangle (row i holds i cells: ranges are balanced by cells, not rows),
// the same range in every launch.  Stream order is the only barrier between blocks: no block waits on another inside a kernel,
// nothing spins, the host is not asked between passes, the call does not synchronise.
//
// Loads: lane k of a tile reads triangle cell base + k, i.e. consecutive addresses along a row (256 contiguous bytes per wave
// instruction, broken only where a row ends).  The cells of row i start at word i * lds of the matrix, the flattened triangle at
// cell i (i - 1) / 2: the two never share a 16-byte phase for more than one row in four, so wider per-lane loads would need a
// per-row realignment that the ordered compaction could not keep; four independent dword loads per lane are in flight instead.
#include <math.h>

#include "lt_internal.h"
#include "lt_radix.hip.h"

namespace {

constexpr int SEL_THREADS = 256;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr long long SEL_MIN_CHUNK = 2048;   // cells per block, at least
constexpr long long SEL_MAX_BLOCKS = 4096;  // beyond SEL_MIN_CHUNK * this many cells the ranges grow instead of the grid

// workspace layout (8-byte words): [0, 1024) four histograms of 256 bins; [1024, 1032) the state after each pick
// (prefix, cells still to take inside the prefix bucket); then per block: (above, tied) packed, tied-before, out-offset
constexpr size_t SEL_HIST_WORDS = 4 * 256;
constexpr size_t SEL_STATE_WORDS = 8;
constexpr size_t SEL_HEAD_WORDS = SEL_HIST_WORDS + SEL_STATE_WORDS;

struct sel_plan { long long total, chunk; int blocks; };

bool sel_make_plan(int32_t n, int64_t m, sel_plan *p) {
    if (n < 2) return false;
    const long long total = (long long)n * (n - 1) / 2;
    if (m < 1 || m > total) return false;
    long long chunk = (total + SEL_MAX_BLOCKS - 1) / SEL_MAX_BLOCKS;
    if (chunk < SEL_MIN_CHUNK) chunk = SEL_MIN_CHUNK;
    chunk = (chunk + SEL_THREADS - 1) / SEL_THREADS * SEL_THREADS;
    p->total = total;
    p->chunk = chunk;
    p->blocks = (int)((total + chunk - 1) / chunk);
    return true;
}

// order-preserving map float bits -> uint32 (larger value <=> larger key).  -0.0 is keyed as +0.0: the integer form of
// `v + 0.0f`, which leaves subnormals alone whatever the kernel's denormal mode is.
__device__ __forceinline__ unsigned sel_key(unsigned bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits >> 31) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ unsigned sel_unkey(unsigned key) { return (key >> 31) ? (key ^ 0x80000000u) : ~key; }

// triangle cell t -> (row i, column j): i (i - 1) / 2 <= t < (i + 1) i / 2
__device__ __forceinline__ void sel_cell(long long t, long long *i_out, long long *j_out) {
    long long i = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
    if (i < 1) i = 1;
    while (i * (i - 1) / 2 > t) --i;
    while ((i + 1) * i / 2 <= t) ++i;
    *i_out = i;
    *j_out = t - i * (i - 1) / 2;
}
__device__ __forceinline__ void sel_advance(long long *i, long long *j, long long step) {
    long long jj = *j + step, ii = *i;
    while (jj >= ii) { jj -= ii; ++ii; }
    *i = ii;
    *j = jj;
}

struct sel_state { unsigned prefix; unsigned long long need, tied_total; };

// The pick behind histogram `pass - 1` (pass = 1 .. 4), by every thread of the block: walks the bins from the top to the one that
// holds the need-th cell.  Leaves (prefix, cells still to take inside that bin, the bin's count) in *out (shared memory).
__device__ void sel_resolve(int pass, long long m, const unsigned long long *__restrict__ ws, unsigned long long *suf /* [256] shared */,
                            sel_state *out /* shared */) {
    const int tid = threadIdx.x;
    unsigned prev_prefix = 0u;
    unsigned long long need = (unsigned long long)m;
    if (pass >= 2) {
        prev_prefix = (unsigned)ws[SEL_HIST_WORDS + 2 * (pass - 2)];
        need = ws[SEL_HIST_WORDS + 2 * (pass - 2) + 1];
    }
    suf[tid] = ws[256 * (pass - 1) + tid];
    if (tid == 0) { out->prefix = prev_prefix; out->need = need; out->tied_total = 0ull; }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {      // suf[d] <- cells in the bins >= d
        unsigned long long v = suf[tid];
        if (tid + off < 256) v += suf[tid + off];
        __syncthreads();
        suf[tid] = v;
        __syncthreads();
    }
    const unsigned long long ge = suf[tid], gt = tid < 255 ? suf[tid + 1] : 0ull;
    if (gt < need && need <= ge) {                 // exactly one bin
        out->prefix = prev_prefix | ((unsigned)tid << (32 - 8 * pass));
        out->need = need - gt;
        out->tied_total = ge - gt;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SEL_THREADS) void k_sel_hist(const float *__restrict__ scores, long long lds, long long total,
                                                          long long chunk, int pass, long long m, unsigned long long *__restrict__ ws) {
    __shared__ unsigned sh[256];
    __shared__ unsigned long long suf[256];
    __shared__ sel_state st;
    const int tid = threadIdx.x, lane = tid & 63;
    sh[tid] = 0u;
    unsigned prefix = 0u, himask = 0u;
    if (pass > 0) {
        sel_resolve(pass, m, ws, suf, &st);
        prefix = st.prefix;
        himask = ~0u << (32 - 8 * pass);
        if (blockIdx.x == 0 && tid == 0) {
            ws[SEL_HIST_WORDS + 2 * (pass - 1)] = prefix;
            ws[SEL_HIST_WORDS + 2 * (pass - 1) + 1] = st.need;
        }
    } else {
        __syncthreads();
    }
    const int shift = 24 - 8 * pass;
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < total ? t0 + chunk : total;
    long long i = 1, j = 0;
    if (t0 + tid < t1) sel_cell(t0 + tid, &i, &j);
    for (long long t = t0 + tid; t - tid < t1; t += 4 * SEL_THREADS) {      // (uniform trip count: the ballots below want whole waves)
        unsigned bits[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = t + u * SEL_THREADS < t1;
            bits[u] = 0u;
            if (ok[u]) {
                bits[u] = __float_as_uint(scores[i * lds + j]);
                sel_advance(&i, &j, SEL_THREADS);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned key = sel_key(bits[u]);
            const bool match = ok[u] && (key & himask) == prefix;
            const unsigned bin = (key >> shift) & 255u;
            // one bin takes nearly every increment (the +0 cells): the lanes that share the first matching lane's bin are counted
            // by a ballot and added once, the others add for themselves
            const unsigned long long act = __ballot(match);
            if (act) {
                const int leader = __ffsll((long long)act) - 1;
                const unsigned lbin = (unsigned)__shfl((int)bin, leader);
                const unsigned long long same = __ballot(match && bin == lbin);
                if (lane == leader) atomicAdd(&sh[lbin], (unsigned)__popcll(same));
                else if (match && bin != lbin) atomicAdd(&sh[bin], 1u);
            }
        }
    }
    __syncthreads();
    if (sh[tid]) atomicAdd(&ws[256 * pass + tid], (unsigned long long)sh[tid]);
}

__global__ __launch_bounds__(SEL_THREADS) void k_sel_count(const float *__restrict__ scores, long long lds, long long total,
                                                           long long chunk, long long m, unsigned long long *__restrict__ ws,
                                                           long long *__restrict__ out_info) {
    __shared__ unsigned long long suf[256];
    __shared__ sel_state st;
    __shared__ unsigned w_above[SEL_WAVES], w_tied[SEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    sel_resolve(4, m, ws, suf, &st);
    const unsigned thr = st.prefix;
    if (blockIdx.x == 0 && tid == 0) {
        ws[SEL_HIST_WORDS + 6] = thr;
        ws[SEL_HIST_WORDS + 7] = st.need;
        out_info[0] = (long long)sel_unkey(thr);
        out_info[1] = m - (long long)st.need;
        out_info[2] = (long long)st.need;
        out_info[3] = (long long)st.tied_total;
    }
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < total ? t0 + chunk : total;
    long long i = 1, j = 0;
    if (t0 + tid < t1) sel_cell(t0 + tid, &i, &j);
    unsigned above = 0u, tied = 0u;
    for (long long t = t0 + tid; t < t1; t += SEL_THREADS) {
        const unsigned key = sel_key(__float_as_uint(scores[i * lds + j]));
        above += key > thr;
        tied += key == thr;
        sel_advance(&i, &j, SEL_THREADS);
    }
    for (int off = 32; off > 0; off >>= 1) {
        above += (unsigned)__shfl_down((int)above, off);
        tied += (unsigned)__shfl_down((int)tied, off);
    }
    if (lane == 0) { w_above[wave] = above; w_tied[wave] = tied; }
    __syncthreads();
    if (tid == 0) {
        unsigned a = 0u, e = 0u;
        for (int w = 0; w < SEL_WAVES; ++w) { a += w_above[w]; e += w_tied[w]; }
        ws[SEL_HEAD_WORDS + 3 * (size_t)blockIdx.x] = ((unsigned long long)a << 32) | e;
    }
}

// one block: per block of the other launches, the tied cells in front of it and where its taken cells start in the output
__global__ __launch_bounds__(SEL_THREADS) void k_sel_scan(int blocks, unsigned long long *__restrict__ ws) {
    __shared__ unsigned long long part[SEL_THREADS];
    const int tid = threadIdx.x;
    const int per = (blocks + SEL_THREADS - 1) / SEL_THREADS;
    const int b0 = tid * per, b1 = b0 + per < blocks ? b0 + per : blocks;
    const unsigned long long tied_taken = ws[SEL_HIST_WORDS + 7];
    unsigned long long *rec = ws + SEL_HEAD_WORDS;
    unsigned long long s = 0ull;
    for (int b = b0; b < b1; ++b) s += rec[3 * (size_t)b] & 0xffffffffull;
    part[tid] = s;
    __syncthreads();
    unsigned long long tied_before = 0ull;
    for (int k = 0; k < tid; ++k) tied_before += part[k];
    __syncthreads();
    s = 0ull;
    for (int b = b0; b < b1; ++b) {
        const unsigned long long c = rec[3 * (size_t)b];
        const unsigned long long tied = c & 0xffffffffull, above = c >> 32;
        const unsigned long long left = tied_taken > tied_before ? tied_taken - tied_before : 0ull;
        const unsigned long long taken = above + (tied < left ? tied : left);
        rec[3 * (size_t)b + 1] = tied_before;
        rec[3 * (size_t)b + 2] = taken;       // (its exclusive scan below)
        tied_before += tied;
        s += taken;
    }
    part[tid] = s;
    __syncthreads();
    unsigned long long off = 0ull;
    for (int k = 0; k < tid; ++k) off += part[k];
    for (int b = b0; b < b1; ++b) {
        const unsigned long long taken = rec[3 * (size_t)b + 2];
        rec[3 * (size_t)b + 2] = off;
        off += taken;
    }
}

__global__ __launch_bounds__(SEL_THREADS) void k_sel_write(const float *__restrict__ scores, long long lds, long long n, long long total,
                                                           long long chunk, long long m, const unsigned long long *__restrict__ ws,
                                                           long long *__restrict__ out_idx, float *__restrict__ out_score) {
    __shared__ unsigned w_tied[SEL_WAVES], w_take[SEL_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned thr = (unsigned)ws[SEL_HIST_WORDS + 6];
    const unsigned long long tied_taken = ws[SEL_HIST_WORDS + 7];
    unsigned long long run_tied = ws[SEL_HEAD_WORDS + 3 * (size_t)blockIdx.x + 1];
    unsigned long long run_out = ws[SEL_HEAD_WORDS + 3 * (size_t)blockIdx.x + 2];
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < total ? t0 + chunk : total;
    long long i = 1, j = 0;
    if (t0 + tid < t1) sel_cell(t0 + tid, &i, &j);
    unsigned next = (t0 + tid < t1) ? __float_as_uint(scores[i * lds + j]) : 0u;
    for (long long t = t0 + tid; t - tid < t1; t += SEL_THREADS) {      // tile by tile, in flat order; uniform trip count
        const bool ok = t < t1;
        const unsigned bits = next;
        const long long ci = i, cj = j;
        if (t + SEL_THREADS < t1) {                                     // the next tile's load goes out before this tile's barriers
            sel_advance(&i, &j, SEL_THREADS);
            next = __float_as_uint(scores[i * lds + j]);
        }
        const unsigned key = sel_key(bits);
        const bool is_tied = ok && key == thr;
        const unsigned long long bt = __ballot(is_tied);
        if (lane == 0) w_tied[wave] = (unsigned)__popcll(bt);
        __syncthreads();
        unsigned long long rank = run_tied + (unsigned long long)__popcll(bt & below);
        unsigned tile_tied = 0u;
        for (int w = 0; w < SEL_WAVES; ++w) {
            if (w < wave) rank += w_tied[w];
            tile_tied += w_tied[w];
        }
        const bool take = ok && (key > thr || (is_tied && rank < tied_taken));
        const unsigned long long bk = __ballot(take);
        if (lane == 0) w_take[wave] = (unsigned)__popcll(bk);
        __syncthreads();
        unsigned long long pos = run_out + (unsigned long long)__popcll(bk & below);
        unsigned tile_take = 0u;
        for (int w = 0; w < SEL_WAVES; ++w) {
            if (w < wave) pos += w_take[w];
            tile_take += w_take[w];
        }
        if (take && pos < (unsigned long long)m) {
            out_idx[pos] = ci * n + cj;
            out_score[pos] = __uint_as_float(bits);
        }
        run_tied += tile_tied;
        run_out += tile_take;
    }
}

}  // namespace

extern "C" size_t lt_top_pairs_workspace_bytes(int32_t n, int64_t m) {
    sel_plan p;
    if (!sel_make_plan(n, m, &p)) return 0;
    return (SEL_HEAD_WORDS + 3 * (size_t)p.blocks) * sizeof(unsigned long long);
}

extern "C" int lt_top_pairs_lower(const float *scores, int64_t lds, int32_t n, int64_t m, int64_t *out_idx, float *out_score,
                                  int64_t *out_info, void *workspace, size_t workspace_bytes, void *stream) {
    LT_REQUIRE(scores && out_idx && out_score && out_info && workspace, "lt_top_pairs_lower: NULL pointer");
    LT_REQUIRE(n >= 2, "lt_top_pairs_lower: n=%d: a strict lower triangle needs n >= 2", n);
    LT_REQUIRE(lds >= n, "lt_top_pairs_lower: lds=%lld smaller than n=%d", (long long)lds, n);
    sel_plan p;
    LT_REQUIRE(sel_make_plan(n, m, &p), "lt_top_pairs_lower: m=%lld outside [1, %lld]", (long long)m, (long long)n * (n - 1) / 2);
    const size_t need = lt_top_pairs_workspace_bytes(n, m);
    LT_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace % 8) == 0,
               "lt_top_pairs_lower: workspace needs %zu bytes (got %zu), 8-byte aligned", need, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ws = (unsigned long long *)workspace;
    const dim3 grid((unsigned)p.blocks), block(SEL_THREADS);
    {
        lt_prof_scope prof(LT_K_SELECT_HIST, st);
        LT_HIP(hipMemsetAsync(ws, 0, SEL_HEAD_WORDS * sizeof(unsigned long long), st));
        for (int pass = 0; pass < 4; ++pass) {
            hipLaunchKernelGGL(k_sel_hist, grid, block, 0, st, scores, (long long)lds, p.total, p.chunk, pass, (long long)m, ws);
            LT_CHECK_LAUNCH();
        }
    }
    {
        lt_prof_scope prof(LT_K_SELECT_COLLECT, st);
        hipLaunchKernelGGL(k_sel_count, grid, block, 0, st, scores, (long long)lds, p.total, p.chunk, (long long)m, ws,
                           (long long *)out_info);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_sel_scan, dim3(1), block, 0, st, p.blocks, ws);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_sel_write, grid, block, 0, st, scores, (long long)lds, (long long)n, p.total, p.chunk, (long long)m, ws,
                           (long long *)out_idx, out_score);
        LT_CHECK_LAUNCH();
    }
    return LT_OK;
}

// ---- the same selection over rows that arrive in chunks: lt_top_stream_* -------------------------------------------------------
// The matrix never exists: lt_top_stream_push is handed rows [row_begin, row_begin + n_rows) as the probe primitive wrote them and
// the handle keeps O(m + slack) state.  Held entries are (stored bits, flat index i * n + j) in one of two candidate buffers of
// capacity m + slack; the total order and the outputs are those of lt_top_pairs_lower above (same sel_key, same digit picks).
//   k_str_scan      a slab of whole rows: lane k reads triangle cell base + k of the slab (consecutive addresses along a row), and
//                   every cell that can still be among the m first is appended through ONE cursor add per wave (str_wave_claim).
//                   Until a compaction has set a threshold every cell qualifies; behind it only key > threshold does: a cell tied
//                   at the threshold has a larger flat index than every held cell (rows ascend), so it ranks behind the m-th.
//   the chain       in front of EVERY slab, always enqueued: k_str_gate (one block) looks at the device-side count and raises the
//                   fire word when it exceeds m + slack / 2; the launches behind it -- 4 + P k_str_hist digit passes (4 over the key,
//                   P = the bytes of n * n - 1 over the complemented flat index among the cells tied at the threshold key: ties are
//                   cut at ascending flat index) and k_str_compact -- return at once when it is down.  The pick of each digit is the
//                   prologue of the next launch, as above.  k_str_compact copies exactly the m first held entries to the other
//                   buffer, which becomes the current one, and records the threshold key.  5 + P launches + the gate per slab
//                   (8 .. 14); an idle chain is that many launches of blocks that read one word.
//   finish          the chain once more, forced, leaves exactly m entries; they are sorted by (row, column) with the stable LSD
//                   passes of lt_radix.hip.h (column digits, then row digits) and written in ascending flat index.
// Why the candidate buffer cannot overflow: push cuts its rows into slabs of whole rows holding at most slack / 2 cells (a row has
// at most n - 1 <= slack / 2 of them).  The chain in front of a slab leaves count <= m + slack / 2: either the gate found it so, or
// the compaction left exactly m.  The slab appends at most its own cells, so count <= m + slack = capacity behind it -- decided on
// the device, the host is never asked.  (Every append is bounds-checked against the capacity all the same.)
// Cells tied at the final threshold that were dropped on the way are counted (word STR_W_TIEDDROP: reset when the threshold
// rises, added to while it stays), which makes out_info[3] the count over the whole triangle.
// Device bytes (lt_top_stream_bytes), A(x) = x rounded up to 256:
//   25600 + A(8 cap) + A(16 cap) + 4 A(4 m) + A(1024 nblk(m)),  cap = m + slack, nblk(m) = the blocks lt_radix_plan gives m entries
// i.e. two buffers of 12-byte entries, the sort's two key / payload pairs and its digit counts: nothing of it grows with n beyond
// the minimum slack 2 (n - 1), nothing with max_push_rows.
namespace {

constexpr int STR_W_CNT = 0;        // [2] entries held in each buffer
constexpr int STR_W_CUR = 2;        // the buffer the scans append to
constexpr int STR_W_SRC = 3;        // the buffer a fired chain selects from
constexpr int STR_W_FIRE = 4;
constexpr int STR_W_THR = 5;        // threshold key, valid when STR_W_THRSET
constexpr int STR_W_THRSET = 6;
constexpr int STR_W_TIEDDROP = 7;   // cells tied at the threshold key that are no longer held
constexpr int STR_W_SEEN = 8;       // cells scanned
constexpr int STR_W_FIRED = 9;      // [2] chains that fired in front of the first slab of a push / of a later slab
constexpr int STR_W_SLABS = 11;
constexpr int STR_W_SLOT = 16;      // 12 x (prefix, need, tied_total): the state after each pick
constexpr int STR_W_HIST = 64;      // 12 x 256 bins
constexpr int STR_MAX_PASS = 12;
constexpr size_t STR_HEAD_WORDS = 3200;
constexpr long long STR_MAX_M = 1ll << 30;
constexpr long long STR_MAX_SLACK = 1ll << 31;
constexpr long long STR_DEFAULT_SLACK = 1ll << 22;

struct str_pick { unsigned long long prefix, need, tied_total; };

// phx_wave_claim of lt_dp.hip: one atomic for the appends of a wave; every lane of the wave calls it
__device__ __forceinline__ unsigned long long str_wave_claim(bool hit, unsigned long long *count) {
    const unsigned long long mk = __ballot(hit);
    if (!mk) return 0;
    const unsigned lane = threadIdx.x & 63u;
    const int leader = __ffsll((long long)mk) - 1;
    unsigned long long base = 0;
    if ((int)lane == leader) base = atomicAdd(count, (unsigned long long)__popcll(mk));
    const unsigned lo = __shfl((unsigned)base, leader), hi = __shfl((unsigned)(base >> 32), leader);
    return (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(mk & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ int str_shift(int p, int P) { return p < 4 ? 24 - 8 * p : 8 * (P - 1 - (p - 4)); }
__device__ __forceinline__ unsigned long long str_imask(int P) { return P >= 8 ? ~0ull : (1ull << (8 * P)) - 1ull; }

// the pick behind histogram p (0 .. 3 key digits, 4 .. 3 + P index digits), by every thread of the block (sel_resolve's walk)
__device__ void str_resolve(int p, int P, long long m, const unsigned long long *__restrict__ ws, unsigned long long *suf, str_pick *out) {
    const int tid = threadIdx.x;
    unsigned long long prev = 0ull, need = (unsigned long long)m;
    if (p == 4) need = ws[STR_W_SLOT + 3 * 3 + 1];
    else if (p > 0) { prev = ws[STR_W_SLOT + 3 * (p - 1)]; need = ws[STR_W_SLOT + 3 * (p - 1) + 1]; }
    suf[tid] = ws[STR_W_HIST + 256 * p + tid];
    if (tid == 0) { out->prefix = prev; out->need = need; out->tied_total = 0ull; }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        unsigned long long v = suf[tid];
        if (tid + off < 256) v += suf[tid + off];
        __syncthreads();
        suf[tid] = v;
        __syncthreads();
    }
    const unsigned long long ge = suf[tid], gt = tid < 255 ? suf[tid + 1] : 0ull;
    if (gt < need && need <= ge) {
        out->prefix = prev | ((unsigned long long)tid << str_shift(p, P));
        out->need = need - gt;
        out->tied_total = ge - gt;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SEL_THREADS) void k_str_gate(unsigned long long *__restrict__ ws, unsigned long long limit, int force, int inside) {
    __shared__ int fire;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const unsigned long long cur = ws[STR_W_CUR] & 1ull;
        const int f = force || ws[STR_W_CNT + cur] > limit;
        ws[STR_W_FIRE] = (unsigned long long)f;
        if (f) {
            ws[STR_W_SRC] = cur;
            ws[STR_W_CUR] = cur ^ 1ull;
            ws[STR_W_CNT + (cur ^ 1ull)] = 0ull;
            if (!force) ws[STR_W_FIRED + (inside ? 1 : 0)] += 1ull;
        }
        fire = f;
    }
    __syncthreads();
    if (fire)
        for (int k = tid; k < STR_MAX_PASS * 256; k += SEL_THREADS) ws[STR_W_HIST + k] = 0ull;
}

// digit pass q of a fired chain over the entries of the source buffer
__global__ __launch_bounds__(SEL_THREADS) void k_str_hist(const unsigned *__restrict__ bits2, const long long *__restrict__ idx2, long long cap,
                                                          int q, int P, long long m, unsigned long long *__restrict__ ws) {
    __shared__ unsigned sh[256];
    __shared__ unsigned long long suf[256];
    __shared__ str_pick st;
    if (!ws[STR_W_FIRE]) return;
    const int tid = threadIdx.x, lane = tid & 63;
    sh[tid] = 0u;
    unsigned long long prefix = 0ull, himask = 0ull;
    unsigned thr = 0u;
    if (q > 0) {
        str_resolve(q - 1, P, m, ws, suf, &st);
        if (blockIdx.x == 0 && tid == 0) {
            ws[STR_W_SLOT + 3 * (q - 1)] = st.prefix;
            ws[STR_W_SLOT + 3 * (q - 1) + 1] = st.need;
            ws[STR_W_SLOT + 3 * (q - 1) + 2] = st.tied_total;
        }
        if (q < 4) {
            prefix = st.prefix;
            himask = (~0ull << (32 - 8 * q)) & 0xffffffffull;
        } else if (q == 4) {
            thr = (unsigned)st.prefix;
        } else {
            thr = (unsigned)ws[STR_W_SLOT + 3 * 3];
            prefix = st.prefix;
            himask = ~0ull << (str_shift(q, P) + 8);
        }
    } else {
        __syncthreads();
    }
    const bool second = q >= 4;
    const int shift = str_shift(q, P);
    const unsigned long long imask = str_imask(P);
    const unsigned long long src = ws[STR_W_SRC] & 1ull;
    unsigned long long cnt = ws[STR_W_CNT + src];
    if (cnt > (unsigned long long)cap) cnt = (unsigned long long)cap;
    const unsigned *bits = bits2 + src * cap;
    const long long *idx = idx2 + src * cap;
    for (unsigned long long x0 = (unsigned long long)blockIdx.x * SEL_THREADS; x0 < cnt; x0 += (unsigned long long)gridDim.x * SEL_THREADS) {
        const unsigned long long x = x0 + tid;
        const bool ok = x < cnt;
        const unsigned key = ok ? sel_key(bits[x]) : 0u;
        unsigned long long v = key;
        bool match = ok;
        if (second) {
            match = ok && key == thr;
            v = match ? (~(unsigned long long)idx[x]) & imask : 0ull;
        }
        match = match && (v & himask) == prefix;
        const unsigned bin = (unsigned)(v >> shift) & 255u;
        const unsigned long long act = __ballot(match);
        if (act) {       // (k_sel_hist's aggregation: one bin takes nearly every increment)
            const int leader = __ffsll((long long)act) - 1;
            const unsigned lbin = (unsigned)__shfl((int)bin, leader);
            const unsigned long long same = __ballot(match && bin == lbin);
            if (lane == leader) atomicAdd(&sh[lbin], (unsigned)__popcll(same));
            else if (match && bin != lbin) atomicAdd(&sh[bin], 1u);
        }
    }
    __syncthreads();
    if (sh[tid]) atomicAdd(&ws[STR_W_HIST + 256 * q + tid], (unsigned long long)sh[tid]);
}

// the last pick, then the m first entries of the source buffer go to the current one; block 0 records the threshold
__global__ __launch_bounds__(SEL_THREADS) void k_str_compact(unsigned *__restrict__ bits2, long long *__restrict__ idx2, long long cap, int P,
                                                             long long m, unsigned long long *__restrict__ ws, long long *__restrict__ out_info) {
    __shared__ unsigned long long suf[256];
    __shared__ str_pick st;
    if (!ws[STR_W_FIRE]) return;
    const int tid = threadIdx.x;
    str_resolve(3 + P, P, m, ws, suf, &st);
    const unsigned long long last = st.prefix;
    const unsigned thr = (unsigned)ws[STR_W_SLOT + 3 * 3];
    const unsigned long long imask = str_imask(P);
    if (blockIdx.x == 0 && tid == 0) {
        const unsigned long long need = ws[STR_W_SLOT + 3 * 3 + 1], tied = ws[STR_W_SLOT + 3 * 3 + 2];
        const unsigned long long extra = tied > need ? tied - need : 0ull;
        const bool same = ws[STR_W_THRSET] && (unsigned)ws[STR_W_THR] == thr;
        const unsigned long long dropped = same ? ws[STR_W_TIEDDROP] + extra : extra;
        ws[STR_W_TIEDDROP] = dropped;
        ws[STR_W_THR] = thr;
        ws[STR_W_THRSET] = 1ull;
        if (out_info) {
            out_info[0] = (long long)sel_unkey(thr);
            out_info[1] = m - (long long)need;
            out_info[2] = (long long)need;
            out_info[3] = (long long)(need + dropped);
        }
    }
    const unsigned long long src = ws[STR_W_SRC] & 1ull, dst = src ^ 1ull;
    unsigned long long cnt = ws[STR_W_CNT + src];
    if (cnt > (unsigned long long)cap) cnt = (unsigned long long)cap;
    for (unsigned long long x0 = (unsigned long long)blockIdx.x * SEL_THREADS; x0 < cnt; x0 += (unsigned long long)gridDim.x * SEL_THREADS) {
        const unsigned long long x = x0 + tid;
        const bool ok = x < cnt;
        unsigned b = 0u;
        long long c = 0;
        bool take = false;
        if (ok) {
            b = bits2[src * cap + x];
            c = idx2[src * cap + x];
            const unsigned key = sel_key(b);
            take = key > thr || (key == thr && ((~(unsigned long long)c) & imask) >= last);
        }
        const unsigned long long pos = str_wave_claim(take, &ws[STR_W_CNT + dst]);
        if (take && pos < (unsigned long long)cap) {
            bits2[dst * cap + pos] = b;
            idx2[dst * cap + pos] = c;
        }
    }
}

// a slab: the cells of rows [a, b), flattened; `tbase` = a (a - 1) / 2, the slab's first cell in the flattened triangle; rows holds
// row `row_begin` of the matrix at its start
__global__ __launch_bounds__(SEL_THREADS) void k_str_scan(const float *__restrict__ rows, long long lds, long long n, long long row_begin,
                                                          long long tbase, long long cells, long long chunk, unsigned *__restrict__ bits2,
                                                          long long *__restrict__ idx2, long long cap, unsigned long long *__restrict__ ws) {
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long cur = ws[STR_W_CUR] & 1ull;
    const bool thr_set = ws[STR_W_THRSET] != 0ull;
    const unsigned thr = (unsigned)ws[STR_W_THR];
    unsigned *bits = bits2 + cur * cap;
    long long *idx = idx2 + cur * cap;
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < cells ? t0 + chunk : cells;
    long long i = 1, j = 0;
    if (t0 + tid < t1) sel_cell(tbase + t0 + tid, &i, &j);
    unsigned tied = 0u;                                                     // (lane 0 of each wave)
    for (long long t = t0 + tid; t - tid < t1; t += 4 * SEL_THREADS) {      // uniform trip count: whole waves at the ballots
        unsigned b[4];
        long long c[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ok[u] = t + u * SEL_THREADS < t1;
            b[u] = 0u;
            c[u] = 0;
            if (ok[u]) {
                b[u] = __float_as_uint(rows[(i - row_begin) * lds + j]);
                c[u] = i * n + j;
                sel_advance(&i, &j, SEL_THREADS);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned key = sel_key(b[u]);
            const bool take = ok[u] && (!thr_set || key > thr);
            const unsigned long long bt = __ballot(ok[u] && thr_set && key == thr);
            if (lane == 0) tied += (unsigned)__popcll(bt);
            const unsigned long long pos = str_wave_claim(take, &ws[STR_W_CNT + cur]);
            if (take && pos < (unsigned long long)cap) {
                bits[pos] = b[u];
                idx[pos] = c[u];
            }
        }
    }
    if (lane == 0 && tied) atomicAdd(&ws[STR_W_TIEDDROP], (unsigned long long)tied);
    if (blockIdx.x == 0 && tid == 0) {
        atomicAdd(&ws[STR_W_SEEN], (unsigned long long)cells);
        atomicAdd(&ws[STR_W_SLABS], 1ull);
    }
}

// finish: the sort keys of the m held entries (column first, the row after the column passes), and the ordered output
__global__ __launch_bounds__(256) void k_str_cols(const long long *__restrict__ idx2, long long cap, const unsigned long long *__restrict__ ws,
                                                  long long n, int m, int32_t *__restrict__ key) {
    const long long *idx = idx2 + (ws[STR_W_CUR] & 1ull) * cap;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < m) {
        const long long c = idx[x];
        key[x] = (c >= 0 && c < n * n) ? (int32_t)(c % n) : 0;
    }
}
__global__ __launch_bounds__(256) void k_str_rowkeys(const long long *__restrict__ idx2, long long cap, const unsigned long long *__restrict__ ws,
                                                     long long n, int m, const int32_t *__restrict__ pay, int32_t *__restrict__ key) {
    const long long *idx = idx2 + (ws[STR_W_CUR] & 1ull) * cap;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < m) {
        const unsigned p = (unsigned)pay[x];
        const long long c = p < (unsigned)m ? idx[p] : 0;
        key[x] = (c >= 0 && c < n * n) ? (int32_t)(c / n) : 0;
    }
}
__global__ __launch_bounds__(256) void k_str_out(const unsigned *__restrict__ bits2, const long long *__restrict__ idx2, long long cap,
                                                 const unsigned long long *__restrict__ ws, long long n, int m, const int32_t *__restrict__ pay,
                                                 long long *__restrict__ out_idx, float *__restrict__ out_score) {
    const unsigned long long cur = ws[STR_W_CUR] & 1ull;
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x < m) {
        unsigned p = (unsigned)pay[x];
        if (p >= (unsigned)m) p = 0u;
        long long c = idx2[cur * cap + p];
        if (c < 0 || c >= n * n) c = n;                 // (cell (1, 0): only a buffer that does not hold m entries gets here)
        out_idx[x] = c;
        out_score[x] = __uint_as_float(bits2[cur * cap + p]);
    }
}

__global__ __launch_bounds__(256) void k_pairs_present(int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const int32_t *__restrict__ u, const int32_t *__restrict__ v, long long m,
                                                       unsigned char *__restrict__ out, unsigned long long *__restrict__ info) {
    for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < m; k += (long long)gridDim.x * 256) {
        const int a0 = u[k], c = v[k];
        unsigned char hit = 0;
        if (a0 < 0 || a0 >= n || c < 0 || c >= n) {
            atomicAdd(&info[0], 1ull);
        } else {
            int a = rowptr[a0], b = rowptr[a0 + 1];
            const int end = b;
            while (a < b) {
                const int mid = a + ((b - a) >> 1);
                if (col[mid] < c) a = mid + 1; else b = mid;
            }
            hit = a < end && col[a] == c;
        }
        out[k] = hit;
    }
}

struct str_layout { size_t bits, idx, key[2], pay[2], hist, total; int rounds, nblk; };

void str_make_layout(int64_t m, int64_t cap, str_layout *L) {
    lt_radix_plan(m, &L->rounds, &L->nblk);
    size_t at = STR_HEAD_WORDS * sizeof(unsigned long long);
    auto take = [&at](size_t bytes) { const size_t o = at; at += lt_align_up(bytes, 256); return o; };
    L->bits = take(8 * (size_t)cap);
    L->idx = take(16 * (size_t)cap);
    for (int x = 0; x < 2; ++x) { L->key[x] = take(4 * (size_t)m); L->pay[x] = take(4 * (size_t)m); }
    L->hist = take(1024 * (size_t)L->nblk);
    L->total = at;
}

}  // namespace

struct lt_top_stream {
    int32_t n = 0, max_rows = 0, next_row = 0;
    int64_t m = 0, slack = 0, cap = 0;
    int P = 0;
    bool finished = false;
    char *dev = nullptr;
    str_layout L;
};

extern "C" int lt_top_stream_create(int32_t n, int64_t m, int32_t max_push_rows, int64_t slack_cells, lt_top_stream **out) {
    LT_REQUIRE(out, "lt_top_stream_create: NULL pointer");
    *out = nullptr;
    LT_REQUIRE(n >= 2, "lt_top_stream_create: n=%d: a strict lower triangle needs n >= 2", n);
    const long long total = (long long)n * (n - 1) / 2;
    LT_REQUIRE(m >= 1 && m <= total, "lt_top_stream_create: m=%lld outside [1, %lld]", (long long)m, total);
    LT_REQUIRE(m <= STR_MAX_M, "lt_top_stream_create: m=%lld beyond %lld", (long long)m, STR_MAX_M);
    LT_REQUIRE(max_push_rows >= 1, "lt_top_stream_create: max_push_rows=%d < 1", max_push_rows);
    const long long least = 2ll * (n - 1);
    if (slack_cells == 0) slack_cells = least > STR_DEFAULT_SLACK ? least : STR_DEFAULT_SLACK;
    LT_REQUIRE(slack_cells >= least && slack_cells <= STR_MAX_SLACK, "lt_top_stream_create: slack_cells=%lld outside [2 (n - 1) = %lld, %lld]",
               (long long)slack_cells, least, STR_MAX_SLACK);
    lt_top_stream *s = new lt_top_stream;
    s->n = n;
    s->m = m;
    s->max_rows = max_push_rows;
    s->slack = slack_cells;
    s->cap = m + slack_cells;
    unsigned long long span = (unsigned long long)n * (unsigned long long)n - 1ull;
    s->P = 0;
    while (span) { ++s->P; span >>= 8; }
    str_make_layout(m, s->cap, &s->L);
    hipError_t e = hipMalloc((void **)&s->dev, s->L.total);
    if (e == hipSuccess) e = hipMemset(s->dev, 0, STR_HEAD_WORDS * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        const size_t wanted = s->L.total;
        (void)hipFree(s->dev);
        delete s;
        return lt_set_error(LT_ERR_HIP, "lt_top_stream_create: %zu device bytes: %s", wanted, hipGetErrorString(e));
    }
    *out = s;
    return LT_OK;
}

extern "C" int lt_top_stream_bytes(const lt_top_stream *s, size_t *device_bytes) {
    LT_REQUIRE(s && device_bytes, "lt_top_stream_bytes: NULL pointer");
    *device_bytes = s->L.total;
    return LT_OK;
}

extern "C" int lt_top_stream_reset(lt_top_stream *s, void *stream) {
    LT_REQUIRE(s, "lt_top_stream_reset: NULL handle");
    LT_HIP(hipMemsetAsync(s->dev, 0, STR_HEAD_WORDS * sizeof(unsigned long long), (hipStream_t)stream));
    s->next_row = 0;
    s->finished = false;
    return LT_OK;
}

extern "C" int lt_top_stream_destroy(lt_top_stream *s) {
    if (!s) return LT_OK;
    (void)hipFree(s->dev);
    delete s;
    return LT_OK;
}

// the chain in front of a slab (force = 0) or of finish (force = 1, out_info set)
static int str_chain(lt_top_stream *s, int force, int inside, long long *out_info, hipStream_t st) {
    unsigned long long *ws = (unsigned long long *)s->dev;
    unsigned *bits = (unsigned *)(s->dev + s->L.bits);
    long long *idx = (long long *)(s->dev + s->L.idx);
    long long blocks = (s->cap + 1023) / 1024;
    if (blocks > 1024) blocks = 1024;
    const dim3 grid((unsigned)blocks), block(SEL_THREADS);
    hipLaunchKernelGGL(k_str_gate, dim3(1), block, 0, st, ws, (unsigned long long)(s->m + s->slack / 2), force, inside);
    LT_CHECK_LAUNCH();
    for (int q = 0; q < 4 + s->P; ++q) {
        hipLaunchKernelGGL(k_str_hist, grid, block, 0, st, (const unsigned *)bits, (const long long *)idx, (long long)s->cap, q, s->P,
                           (long long)s->m, ws);
        LT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_str_compact, grid, block, 0, st, bits, idx, (long long)s->cap, s->P, (long long)s->m, ws, out_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_top_stream_push(lt_top_stream *s, const float *rows, int64_t lds, int32_t row_begin, int32_t n_rows, void *stream) {
    LT_REQUIRE(s && rows, "lt_top_stream_push: NULL pointer");
    LT_REQUIRE(!s->finished, "lt_top_stream_push: the stream was finished (lt_top_stream_reset starts another matrix)");
    LT_REQUIRE(n_rows >= 1 && n_rows <= s->max_rows, "lt_top_stream_push: n_rows=%d outside [1, max_push_rows = %d]", n_rows, s->max_rows);
    LT_REQUIRE(row_begin == s->next_row, "lt_top_stream_push: row_begin=%d, the next row is %d (rows arrive in order, once)", row_begin,
               s->next_row);
    LT_REQUIRE((long long)row_begin + n_rows <= s->n, "lt_top_stream_push: rows [%d, %lld) beyond n=%d", row_begin,
               (long long)row_begin + n_rows, s->n);
    LT_REQUIRE(lds >= (long long)row_begin + n_rows - 1, "lt_top_stream_push: lds=%lld smaller than row_begin + n_rows - 1 = %lld",
               (long long)lds, (long long)row_begin + n_rows - 1);
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *ws = (unsigned long long *)s->dev;
    unsigned *bits = (unsigned *)(s->dev + s->L.bits);
    long long *idx = (long long *)(s->dev + s->L.idx);
    const long long end = (long long)row_begin + n_rows, limit = s->slack / 2;
    int slab = 0;
    for (long long a = row_begin > 1 ? row_begin : 1; a < end; ++slab) {       // (row 0 holds no cell)
        long long b = a, cells = 0;
        while (b < end && cells + b <= limit) { cells += b; ++b; }           // whole rows, at most slack / 2 cells (row a alone fits)
        int rc = str_chain(s, 0, slab > 0, nullptr, st);
        if (rc != LT_OK) return rc;
        long long chunk = (cells + SEL_MAX_BLOCKS - 1) / SEL_MAX_BLOCKS;
        if (chunk < SEL_MIN_CHUNK) chunk = SEL_MIN_CHUNK;
        chunk = (chunk + SEL_THREADS - 1) / SEL_THREADS * SEL_THREADS;
        hipLaunchKernelGGL(k_str_scan, dim3((unsigned)((cells + chunk - 1) / chunk)), dim3(SEL_THREADS), 0, st, rows, (long long)lds,
                           (long long)s->n, (long long)row_begin, a * (a - 1) / 2, cells, chunk, bits, idx, (long long)s->cap, ws);
        LT_CHECK_LAUNCH();
        a = b;
    }
    s->next_row = (int32_t)end;
    return LT_OK;
}

extern "C" int lt_top_stream_finish(lt_top_stream *s, int64_t *out_idx, float *out_score, int64_t *out_info, void *stream) {
    LT_REQUIRE(s && out_idx && out_score && out_info, "lt_top_stream_finish: NULL pointer");
    LT_REQUIRE(s->next_row == s->n, "lt_top_stream_finish: %d of %d rows were pushed", s->next_row, s->n);
    LT_REQUIRE(!s->finished, "lt_top_stream_finish: already finished (lt_top_stream_reset starts another matrix)");
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long *ws = (const unsigned long long *)s->dev;
    const unsigned *bits = (const unsigned *)(s->dev + s->L.bits);
    const long long *idx = (const long long *)(s->dev + s->L.idx);
    int32_t *key[2] = {(int32_t *)(s->dev + s->L.key[0]), (int32_t *)(s->dev + s->L.key[1])};
    int32_t *pay[2] = {(int32_t *)(s->dev + s->L.pay[0]), (int32_t *)(s->dev + s->L.pay[1])};
    int32_t *hist = (int32_t *)(s->dev + s->L.hist);
    s->finished = true;
    int rc = str_chain(s, 1, 0, (long long *)out_info, st);
    if (rc != LT_OK) return rc;
    const int m = (int)s->m;
    const dim3 mgrid((unsigned)((s->m + 255) / 256));
    hipLaunchKernelGGL(k_str_cols, mgrid, dim3(256), 0, st, idx, (long long)s->cap, ws, (long long)s->n, m, key[0]);
    LT_CHECK_LAUNCH();
    const int passes = lt_radix_passes(s->n - 1);
    int cur = 0;
    const int32_t *pin = nullptr;
    for (int half = 0; half < 2; ++half) {
        for (int q = 0; q < passes; ++q) {
            hipLaunchKernelGGL(k_gb_radix_hist, dim3((unsigned)s->L.nblk), dim3(256), 0, st, (const int32_t *)key[cur], m, 8 * q, s->L.rounds,
                               s->L.nblk, hist);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, hist, (long long)256 * s->L.nblk);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_gb_radix_scatter, dim3((unsigned)s->L.nblk), dim3(256), 0, st, (const int32_t *)key[cur], pin, m, 8 * q,
                               s->L.rounds, s->L.nblk, (const int32_t *)hist, key[cur ^ 1], pay[cur ^ 1]);
            LT_CHECK_LAUNCH();
            cur ^= 1;
            pin = pay[cur];
        }
        if (half == 0) {       // the sorted columns are done with: their buffer takes the row keys, in the order reached so far
            hipLaunchKernelGGL(k_str_rowkeys, mgrid, dim3(256), 0, st, idx, (long long)s->cap, ws, (long long)s->n, m, pin, key[cur]);
            LT_CHECK_LAUNCH();
        }
    }
    hipLaunchKernelGGL(k_str_out, mgrid, dim3(256), 0, st, bits, idx, (long long)s->cap, ws, (long long)s->n, m, pin, (long long *)out_idx,
                       out_score);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_top_stream_stats(const lt_top_stream *s, int64_t *d_out, void *stream) {
    LT_REQUIRE(s && d_out, "lt_top_stream_stats: NULL pointer");
    LT_HIP(hipMemcpyAsync(d_out, s->dev, 16 * sizeof(int64_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

extern "C" int lt_pairs_present(int32_t n, const int32_t *d_rowptr, const int32_t *d_col, const int32_t *u, const int32_t *v, int64_t m,
                                uint8_t *out, int64_t *d_info, void *stream) {
    LT_REQUIRE(d_rowptr && d_info && n >= 1, "lt_pairs_present: NULL pointer or n=%d < 1", n);
    LT_REQUIRE(m >= 0, "lt_pairs_present: m=%lld < 0", (long long)m);
    hipStream_t st = (hipStream_t)stream;
    LT_HIP(hipMemsetAsync(d_info, 0, sizeof(int64_t), st));
    if (m == 0) return LT_OK;
    LT_REQUIRE(d_col && u && v && out, "lt_pairs_present: NULL pointer");
    long long blocks = (m + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_pairs_present, dim3((unsigned)blocks), dim3(256), 0, st, (int)n, d_rowptr, d_col, u, v, (long long)m, out,
                       (unsigned long long *)d_info);
    LT_CHECK_LAUNCH();
    return LT_OK;
}
