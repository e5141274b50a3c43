// Attack metrics on the device: the table behind the reference's roc_curve / precision_recall_curve / average_precision_score
// calls (attacker.py:378-389) -- for each distinct score, in descending order, how many positives and how many negatives score
// at least that much -- and the two numbers the attack prints, AUC (as the exact integer Mann-Whitney sum) and AP.
//
// Item k has label labels[k] in {0, 1} and score scores[index[k]] (scores[k] without an index).  Values are ordered as
// lt_top_pairs_lower orders them (lt_select.hip sel_key: -0.0 counts as +0.0, subnormals stay distinct whatever the kernel's
// denormal mode is); the sort key is the COMPLEMENT of that key, so that ascending key order is descending score order:
//   k_mc_keys          gather, key, label; counts non-finite scores, indices outside [0, n_scores) (replaced by 0 BEFORE the load,
//                      as k_check_nodes does with node ids) and labels > 1 (taken as 1)
//   x 4, low digit first (an LSD radix sort, 8 bits a pass, the label as payload; the pattern of lt_graph_build.hip's transpose):
//   k_mc_hist          digit counts per block, hist[digit * blocks + block]
//   k_mc_scan          one block per digit: exclusive scan of the digit's counts over the blocks, and the digit's total
//   k_mc_scatter       prologue: the scan of the 256 totals (every block repeats it in LDS) = where each digit starts; then the block
//                      walks its keys tile by tile and places every key behind the keys of its digit before it
//   then, on the sorted keys (a run = the items of one distinct value; its end is the last of them):
//   k_mc_count         positives and run ends per block
//   k_mc_block_scan    one block: exclusive scans of both over the blocks; D = the run ends, P = the positives
//   k_mc_write         at the run end at position i, the d-th of them: thresholds[d] = the value, tps[d] = positives in [0, i],
//                      fps[d] = i + 1 - tps[d]
//   k_mc_terms         per block of d: the integer sum of neg_d (2 tps[d - 1] + pos_d) and the float64 sum of
//                      (pos_d / P) (tps[d] / (tps[d] + fps[d])), each thread its own d's in ascending order, the threads' sums
//                      added in thread order
//   k_mc_summary       the blocks' sums added in block order; summary[0 .. 8)
// Every output is a function of the MULTISET of (value, label) pairs -- tps / fps are read at run ends only, where every member of
// the tie has been counted -- so the sort need not be stable and neither the order of the items nor the order inside a tie shows.
// The integer sums are exact in any order; the float64 sum has ONE order.  Two calls give identical bytes.
// Every block owns a contiguous range of `chunk` positions, the same range in every launch.  Stream order is the only barrier
// between blocks: no block waits on another inside a kernel, nothing spins, the host is not asked between passes, the call does
// not synchronise.  Every loop is bounded by an argument passed by value.
#include "lt_internal.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_WAVES = MC_THREADS / 64;
constexpr long long MC_MIN_CHUNK = 512;    // positions per block and pass, at least
constexpr long long MC_MAX_BLOCKS = 512;   // beyond MC_MIN_CHUNK * this many items the ranges grow instead of the grid
// (k_mc_scan, k_mc_block_scan: MC_THREADS threads over the blocks, each a contiguous stretch of them)

// workspace: [0, MC_HEAD_WORDS) 8-byte words: non-finite scores, bad indices, bad labels, D, P; then MC_BLOCK_WORDS per block:
// positives (-> those in front of the block), run ends (-> those in front), the block's integer sum, its float64 sum; then the
// digit counters (32-bit; 256 rows of one entry per block, then the 256 row sums), two key arrays (32-bit) and two label arrays (bytes)
constexpr size_t MC_HEAD_WORDS = 8;
constexpr size_t MC_BLOCK_WORDS = 4;

struct mc_plan {
    long long n, chunk;
    int blocks, rounds;
    size_t off_hist, off_tot, off_key[2], off_lab[2], bytes;
};

bool mc_make_plan(int64_t n_items, mc_plan *p) {
    if (n_items < 1 || n_items > 0x7fffffffLL) return false;
    long long chunk = ((long long)n_items + MC_MAX_BLOCKS - 1) / MC_MAX_BLOCKS;
    if (chunk < MC_MIN_CHUNK) chunk = MC_MIN_CHUNK;
    chunk = (chunk + MC_THREADS - 1) / MC_THREADS * MC_THREADS;
    p->n = (long long)n_items;
    p->chunk = chunk;
    p->blocks = (int)((p->n + chunk - 1) / chunk);
    p->rounds = (int)(chunk / MC_THREADS);
    size_t off = (MC_HEAD_WORDS + MC_BLOCK_WORDS * (size_t)p->blocks) * 8;
    p->off_hist = off;
    off += lt_align_up((size_t)256 * p->blocks * 4, 8);
    p->off_tot = off;
    off += 256 * 4;
    for (int x = 0; x < 2; ++x) { p->off_key[x] = off; off += lt_align_up((size_t)p->n * 4, 8); }
    for (int x = 0; x < 2; ++x) { p->off_lab[x] = off; off += lt_align_up((size_t)p->n, 8); }
    p->bytes = off;
    return true;
}

// lt_select.hip sel_key / sel_unkey: order-preserving map float bits -> uint32 (larger value <=> larger key), -0.0 keyed as +0.0
__device__ __forceinline__ unsigned mc_key(unsigned bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits >> 31) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ unsigned mc_unkey(unsigned key) { return (key >> 31) ? (key ^ 0x80000000u) : ~key; }

__global__ __launch_bounds__(MC_THREADS) void k_mc_keys(const float *__restrict__ scores, long long n_scores,
                                                        const long long *__restrict__ index, const unsigned char *__restrict__ labels,
                                                        long long n, long long chunk, unsigned *__restrict__ key_out,
                                                        unsigned char *__restrict__ lab_out, unsigned long long *__restrict__ head) {
    __shared__ unsigned bad[3];
    const int tid = threadIdx.x;
    if (tid < 3) bad[tid] = 0u;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < n ? t0 + chunk : n;
    unsigned nonfinite = 0u, bad_index = 0u, bad_label = 0u;
    for (long long t = t0 + tid; t < t1; t += MC_THREADS) {
        long long s = index ? index[t] : t;
        if ((unsigned long long)s >= (unsigned long long)n_scores) { ++bad_index; s = 0; }
        const unsigned bits = __float_as_uint(scores[s]);
        nonfinite += (bits & 0x7f800000u) == 0x7f800000u;
        unsigned char y = labels[t];
        if (y > 1) { ++bad_label; y = 1; }
        key_out[t] = ~mc_key(bits);
        lab_out[t] = y;
    }
    if (nonfinite) atomicAdd(&bad[0], nonfinite);
    if (bad_index) atomicAdd(&bad[1], bad_index);
    if (bad_label) atomicAdd(&bad[2], bad_label);
    __syncthreads();
    if (tid < 3 && bad[tid]) atomicAdd(&head[tid], (unsigned long long)bad[tid]);
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_hist(const unsigned *__restrict__ key, long long n, long long chunk, int shift, int nblk,
                                                        unsigned *__restrict__ hist) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x, lane = tid & 63;
    h[tid] = 0u;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < n ? t0 + chunk : n;
    for (long long t = t0 + tid; t - tid < t1; t += MC_THREADS) {      // (uniform trip count: the ballots below want whole waves)
        const bool ok = t < t1;
        const unsigned bin = ok ? (key[t] >> shift) & 255u : 0u;
        // one bin takes nearly every increment (the +0 scores): the lanes that share the first lane's bin are counted by a
        // ballot and added once, the others add for themselves (lt_select.hip k_sel_hist)
        const unsigned long long act = __ballot(ok);
        if (act) {
            const int leader = __ffsll((long long)act) - 1;
            const unsigned lbin = (unsigned)__shfl((int)bin, leader);
            const unsigned long long same = __ballot(ok && bin == lbin);
            if (lane == leader) atomicAdd(&h[lbin], (unsigned)__popcll(same));
            else if (ok && bin != lbin) atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    hist[(size_t)tid * nblk + blockIdx.x] = h[tid];
}

// one block per digit: row d of hist (the blocks' counts of digit d, contiguous) -> its exclusive prefix sums over the blocks, and
// tot[d] = the row's sum.  Each thread a contiguous stretch of the row; the stretch sums scanned in LDS.
__global__ __launch_bounds__(MC_THREADS) void k_mc_scan(unsigned *__restrict__ hist, int nblk, unsigned *__restrict__ tot) {
    __shared__ unsigned part[MC_THREADS];
    const int t = threadIdx.x;
    unsigned *row = hist + (size_t)blockIdx.x * nblk;
    const int per = (nblk + MC_THREADS - 1) / MC_THREADS;
    const int lo = t * per < nblk ? t * per : nblk, hi = lo + per < nblk ? lo + per : nblk;
    unsigned s = 0u;
    for (int i = lo; i < hi; ++i) s += row[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < MC_THREADS; off <<= 1) {
        const unsigned v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned run = part[t] - s;
    for (int i = lo; i < hi; ++i) { const unsigned v = row[i]; row[i] = run; run += v; }
    if (t == MC_THREADS - 1) tot[blockIdx.x] = part[t];
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_scatter(const unsigned *__restrict__ key_in, const unsigned char *__restrict__ lab_in,
                                                           long long n, long long chunk, int rounds, int shift, int nblk,
                                                           const unsigned *__restrict__ offs, const unsigned *__restrict__ tot,
                                                           unsigned *__restrict__ key_out, unsigned char *__restrict__ lab_out) {
    __shared__ unsigned base[256];
    __shared__ unsigned wcnt[MC_WAVES][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    // where digit t starts: the keys of the lower digits (a 256-entry scan every block repeats in LDS -- cheaper than a one-block
    // launch between k_mc_scan and this one) + the keys of digit t in the blocks in front of this one
    const unsigned mine = tot[t];
    base[t] = mine;
    for (int x = 0; x < MC_WAVES; ++x) wcnt[x][t] = 0u;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned v = t >= off ? base[t - off] : 0u;
        __syncthreads();
        base[t] += v;
        __syncthreads();
    }
    base[t] = base[t] - mine + offs[(size_t)t * nblk + blockIdx.x];
    __syncthreads();
    const long long first = (long long)blockIdx.x * chunk;
    for (int r = 0; r < rounds; ++r) {
        const long long g0 = first + (long long)r * MC_THREADS;
        if (g0 >= n) break;                                       // (the whole block leaves together)
        const long long i = g0 + t;
        const bool valid = i < n;
        const unsigned key = valid ? key_in[i] : 0u;
        const unsigned char y = valid ? lab_in[i] : (unsigned char)0;
        const unsigned d = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);                // the valid lanes of this wave that hold digit d
        for (int b = 0; b < 8; ++b) {
            const int bit = (int)((d >> b) & 1u);
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wcnt[w][d] = (unsigned)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned pos = base[d] + rank;
            for (int x = 0; x < w; ++x) pos += wcnt[x][d];
            if ((long long)pos < n) {
                key_out[pos] = key;
                lab_out[pos] = y;
            }
        }
        __syncthreads();
        unsigned add = 0u;
        for (int x = 0; x < MC_WAVES; ++x) { add += wcnt[x][t]; wcnt[x][t] = 0u; }
        base[t] += add;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_count(const unsigned *__restrict__ key, const unsigned char *__restrict__ lab, long long n,
                                                         long long chunk, unsigned long long *__restrict__ rec) {
    __shared__ unsigned w_pos[MC_WAVES], w_end[MC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < n ? t0 + chunk : n;
    unsigned pos = 0u, ends = 0u;
    for (long long t = t0 + tid; t < t1; t += MC_THREADS) {
        pos += lab[t];
        ends += (t == n - 1) || key[t] != key[t + 1];
    }
    for (int off = 32; off > 0; off >>= 1) {
        pos += (unsigned)__shfl_down((int)pos, off);
        ends += (unsigned)__shfl_down((int)ends, off);
    }
    if (lane == 0) { w_pos[wave] = pos; w_end[wave] = ends; }
    __syncthreads();
    if (tid == 0) {
        unsigned a = 0u, e = 0u;
        for (int w = 0; w < MC_WAVES; ++w) { a += w_pos[w]; e += w_end[w]; }
        rec[MC_BLOCK_WORDS * (size_t)blockIdx.x] = a;
        rec[MC_BLOCK_WORDS * (size_t)blockIdx.x + 1] = e;
    }
}

// one block: per block of the other launches, the positives and the run ends in front of it; head[3] = D, head[4] = P
__global__ __launch_bounds__(MC_THREADS) void k_mc_block_scan(int blocks, unsigned long long *__restrict__ head) {
    __shared__ unsigned long long part_p[MC_THREADS], part_e[MC_THREADS];
    const int tid = threadIdx.x;
    const int per = (blocks + MC_THREADS - 1) / MC_THREADS;
    const int b0 = tid * per < blocks ? tid * per : blocks, b1 = b0 + per < blocks ? b0 + per : blocks;
    unsigned long long *rec = head + MC_HEAD_WORDS;
    unsigned long long sp = 0ull, se = 0ull;
    for (int b = b0; b < b1; ++b) {
        sp += rec[MC_BLOCK_WORDS * (size_t)b];
        se += rec[MC_BLOCK_WORDS * (size_t)b + 1];
    }
    part_p[tid] = sp;
    part_e[tid] = se;
    __syncthreads();
    unsigned long long run_p = 0ull, run_e = 0ull;
    for (int k = 0; k < tid; ++k) { run_p += part_p[k]; run_e += part_e[k]; }
    for (int b = b0; b < b1; ++b) {
        const unsigned long long p = rec[MC_BLOCK_WORDS * (size_t)b], e = rec[MC_BLOCK_WORDS * (size_t)b + 1];
        rec[MC_BLOCK_WORDS * (size_t)b] = run_p;
        rec[MC_BLOCK_WORDS * (size_t)b + 1] = run_e;
        run_p += p;
        run_e += e;
    }
    if (tid == MC_THREADS - 1) { head[3] = run_e; head[4] = run_p; }      // (the last thread's stretch ends the list, or is empty)
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_write(const unsigned *__restrict__ key, const unsigned char *__restrict__ lab, long long n,
                                                         long long chunk, const unsigned long long *__restrict__ head,
                                                         float *__restrict__ thresholds, long long *__restrict__ tps,
                                                         long long *__restrict__ fps) {
    __shared__ unsigned w_pos[MC_WAVES], w_end[MC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull, upto = (2ull << lane) - 1ull;
    const unsigned long long *rec = head + MC_HEAD_WORDS + MC_BLOCK_WORDS * (size_t)blockIdx.x;
    unsigned long long run_pos = rec[0], run_end = rec[1];
    const long long t0 = (long long)blockIdx.x * chunk;
    const long long t1 = t0 + chunk < n ? t0 + chunk : n;
    for (long long t = t0 + tid; t - tid < t1; t += MC_THREADS) {      // tile by tile, in sorted order; uniform trip count
        const bool ok = t < t1;
        const unsigned k = ok ? key[t] : 0u;
        const bool y = ok && lab[t] != 0;
        const bool end = ok && (t == n - 1 || key[t + 1] != k);
        const unsigned long long by = __ballot(y), be = __ballot(end);
        if (lane == 0) { w_pos[wave] = (unsigned)__popcll(by); w_end[wave] = (unsigned)__popcll(be); }
        __syncthreads();
        unsigned long long tp = run_pos + (unsigned long long)__popcll(by & upto);       // positives in [0, t]
        unsigned long long d = run_end + (unsigned long long)__popcll(be & below);       // run ends in [0, t)
        unsigned tile_pos = 0u, tile_end = 0u;
        for (int w = 0; w < MC_WAVES; ++w) {
            if (w < wave) { tp += w_pos[w]; d += w_end[w]; }
            tile_pos += w_pos[w];
            tile_end += w_end[w];
        }
        if (end && d < (unsigned long long)n) {
            thresholds[d] = __uint_as_float(mc_unkey(~k));
            tps[d] = (long long)tp;
            fps[d] = t + 1 - (long long)tp;
        }
        run_pos += tile_pos;
        run_end += tile_end;
        __syncthreads();
    }
}

__global__ __launch_bounds__(MC_THREADS) void k_mc_terms(const long long *__restrict__ tps, const long long *__restrict__ fps, long long n,
                                                         long long chunk, unsigned long long *__restrict__ head) {
    __shared__ unsigned long long s_a[MC_THREADS];
    __shared__ double s_ap[MC_THREADS];
    const int tid = threadIdx.x;
    long long D = (long long)head[3];
    if (D > n) D = n;
    const double P = (double)head[4];
    const long long t0 = (long long)blockIdx.x * chunk;
    unsigned long long a = 0ull;
    double ap = 0.0;
    for (long long d = t0 + tid; d < t0 + chunk; d += MC_THREADS) {
        if (d >= D) break;
        const long long tp = tps[d], fp = fps[d];
        const long long tp_prev = d ? tps[d - 1] : 0, fp_prev = d ? fps[d - 1] : 0;
        const long long pos = tp - tp_prev, neg = fp - fp_prev;
        a += (unsigned long long)neg * (unsigned long long)(2 * tp_prev + pos);
        if (P > 0.0) ap += ((double)pos / P) * ((double)tp / (double)(tp + fp));
    }
    s_a[tid] = a;
    s_ap[tid] = ap;
    __syncthreads();
    if (tid == 0) {
        unsigned long long sa = 0ull;
        double sp = 0.0;
        for (int k = 0; k < MC_THREADS; ++k) { sa += s_a[k]; sp += s_ap[k]; }      // thread order
        unsigned long long *rec = head + MC_HEAD_WORDS + MC_BLOCK_WORDS * (size_t)blockIdx.x;
        rec[2] = sa;
        rec[3] = (unsigned long long)__double_as_longlong(sp);
    }
}

__global__ __launch_bounds__(64) void k_mc_summary(int blocks, long long n, long long chunk, const unsigned long long *__restrict__ head,
                                                   long long *__restrict__ summary) {
    if (threadIdx.x != 0) return;
    const long long D = (long long)head[3], P = (long long)head[4];
    unsigned long long sa = 0ull;
    double sp = 0.0;
    for (int b = 0; b < blocks; ++b) {                                     // block order; the blocks past D hold zeros
        if ((long long)b * chunk >= D) break;
        const unsigned long long *rec = head + MC_HEAD_WORDS + MC_BLOCK_WORDS * (size_t)b;
        sa += rec[2];
        sp += __longlong_as_double((long long)rec[3]);
    }
    summary[0] = D;
    summary[1] = P;
    summary[2] = n - P;
    summary[3] = (long long)sa;
    summary[4] = P > 0 ? __double_as_longlong(sp) : 0ll;
    summary[5] = (long long)head[0];
    summary[6] = (long long)head[1];
    summary[7] = (long long)head[2];
}

}  // namespace

extern "C" size_t lt_score_curve_workspace_bytes(int64_t n_items) {
    mc_plan p;
    if (!mc_make_plan(n_items, &p)) return 0;
    return p.bytes;
}

extern "C" int lt_score_curve(const float *scores, int64_t n_scores, const int64_t *index_or_null, const uint8_t *labels, int64_t n_items,
                              float *thresholds, int64_t *tps, int64_t *fps, int64_t *summary, void *workspace, size_t workspace_bytes,
                              void *stream) {
    LT_REQUIRE(scores && labels && thresholds && tps && fps && summary && workspace, "lt_score_curve: NULL pointer");
    mc_plan p;
    LT_REQUIRE(mc_make_plan(n_items, &p), "lt_score_curve: n_items=%lld outside [1, 2^31 - 1]", (long long)n_items);
    LT_REQUIRE(n_scores >= 1, "lt_score_curve: n_scores=%lld: the scores hold no element", (long long)n_scores);
    LT_REQUIRE(index_or_null || n_scores >= n_items, "lt_score_curve: n_scores=%lld smaller than n_items=%lld without an index",
               (long long)n_scores, (long long)n_items);
    LT_REQUIRE(workspace_bytes >= p.bytes && ((uintptr_t)workspace % 8) == 0,
               "lt_score_curve: workspace needs %zu bytes (got %zu), 8-byte aligned", p.bytes, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *wsb = (unsigned char *)workspace;
    unsigned long long *head = (unsigned long long *)workspace;
    unsigned *hist = (unsigned *)(wsb + p.off_hist), *tot = (unsigned *)(wsb + p.off_tot);
    unsigned *key[2] = {(unsigned *)(wsb + p.off_key[0]), (unsigned *)(wsb + p.off_key[1])};
    unsigned char *lab[2] = {wsb + p.off_lab[0], wsb + p.off_lab[1]};
    const dim3 grid((unsigned)p.blocks), block(MC_THREADS);
    {
        lt_prof_scope prof(LT_K_METRICS_SORT, st);
        LT_HIP(hipMemsetAsync(head, 0, MC_HEAD_WORDS * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_mc_keys, grid, block, 0, st, scores, (long long)n_scores, (const long long *)index_or_null,
                           (const unsigned char *)labels, p.n, p.chunk, key[0], lab[0], head);
        LT_CHECK_LAUNCH();
        for (int pass = 0; pass < 4; ++pass) {                              // the sorted keys end in key[0] / lab[0]
            const int in = pass & 1, out = in ^ 1;
            hipLaunchKernelGGL(k_mc_hist, grid, block, 0, st, key[in], p.n, p.chunk, 8 * pass, p.blocks, hist);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_mc_scan, dim3(256), block, 0, st, hist, p.blocks, tot);
            LT_CHECK_LAUNCH();
            hipLaunchKernelGGL(k_mc_scatter, grid, block, 0, st, key[in], lab[in], p.n, p.chunk, p.rounds, 8 * pass, p.blocks, hist,
                               tot, key[out], lab[out]);
            LT_CHECK_LAUNCH();
        }
    }
    {
        lt_prof_scope prof(LT_K_METRICS_CURVE, st);
        hipLaunchKernelGGL(k_mc_count, grid, block, 0, st, key[0], lab[0], p.n, p.chunk, head + MC_HEAD_WORDS);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mc_block_scan, dim3(1), block, 0, st, p.blocks, head);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mc_write, grid, block, 0, st, key[0], lab[0], p.n, p.chunk, head, thresholds, (long long *)tps,
                           (long long *)fps);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mc_terms, grid, block, 0, st, (const long long *)tps, (const long long *)fps, p.n, p.chunk, head);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_mc_summary, dim3(1), dim3(64), 0, st, p.blocks, p.n, p.chunk, head, (long long *)summary);
        LT_CHECK_LAUNCH();
    }
    return LT_OK;
}
