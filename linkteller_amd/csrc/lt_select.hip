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
