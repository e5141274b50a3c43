// A stable LSD radix sort of int32 keys with an int32 payload, 8 bits a pass, and the one-block scan it needs.  Shared by the
// transpose of lt_graph_create_device (lt_graph_build.hip) and by the cell sort of lt_sym_csr_from_cells (lt_dp_graph.hip).
//
// A block owns `rounds` consecutive groups of 256 entries.  Pass: (1) digit counts per block, hist[digit * nblk + block];
// (2) exclusive scan of hist in that order = where each block's entries of each digit start; (3) the block walks its groups in
// order and places every entry behind the entries of its digit that came before it: in earlier groups (base), in lower waves of the
// group (wcnt), in lower lanes of the wave (a ballot per digit bit).  Entry order inside a digit is kept.  The payload of the first
// pass may be absent (pay_in == NULL): it is then the entry's index.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

static __global__ __launch_bounds__(256) void k_gb_radix_hist(const int32_t *__restrict__ key, int count, int shift, int rounds, int nblk,
                                                              int32_t *__restrict__ hist) {
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * rounds * 256;
    for (int r = 0; r < rounds; ++r) {
        const long long i = base + (long long)r * 256 + threadIdx.x;
        if (i < count) atomicAdd(&h[(key[i] >> shift) & 255], 1);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * nblk + blockIdx.x] = h[threadIdx.x];
}
// one block: a[0 .. N) -> its exclusive prefix sums (each thread a contiguous stretch; the stretch sums scanned in LDS)
static __global__ __launch_bounds__(1024) void k_gb_scan(int32_t *__restrict__ a, long long N) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const long long per = (N + 1023) / 1024;
    const long long lo = (long long)t * per < N ? (long long)t * per : N, hi = lo + per < N ? lo + per : N;
    int s = 0;
    for (long long i = lo; i < hi; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (long long i = lo; i < hi; ++i) { const int v = a[i]; a[i] = run; run += v; }
}
static __global__ __launch_bounds__(256) void k_gb_radix_scatter(const int32_t *__restrict__ key_in, const int32_t *__restrict__ pay_in,
                                                                 int count, int shift, int rounds, int nblk,
                                                                 const int32_t *__restrict__ offs, int32_t *__restrict__ key_out,
                                                                 int32_t *__restrict__ pay_out) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    base[t] = offs[(size_t)t * nblk + blockIdx.x];
    for (int x = 0; x < 4; ++x) wcnt[x][t] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * rounds * 256;
    for (int r = 0; r < rounds; ++r) {
        const long long g0 = first + (long long)r * 256;
        if (g0 >= count) break;                                   // (the whole block leaves together)
        const long long i = g0 + t;
        const bool valid = i < count;
        const int key = valid ? key_in[i] : 0;
        const int d = (key >> shift) & 255;
        unsigned long long same = __ballot(valid);                // the valid lanes of this wave that hold digit d
        for (int b = 0; b < 8; ++b) {
            const int bit = (d >> b) & 1;
            const unsigned long long bal = __ballot(bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[w][d] = __popcll(same);
        __syncthreads();
        if (valid) {
            int pos = base[d] + rank;
            for (int x = 0; x < w; ++x) pos += wcnt[x][d];
            if ((unsigned)pos < (unsigned)count) {
                key_out[pos] = key;
                pay_out[pos] = pay_in ? pay_in[i] : (int32_t)i;
            }
        }
        __syncthreads();
        base[t] += wcnt[0][t] + wcnt[1][t] + wcnt[2][t] + wcnt[3][t];
        for (int x = 0; x < 4; ++x) wcnt[x][t] = 0;
        __syncthreads();
    }
}

// entries per block = 256 * rounds, chosen so that a sort of `count` entries takes at most 4096 blocks
static inline void lt_radix_plan(int64_t count, int *rounds, int *nblk) {
    int r = 4;
    while (r < (1 << 20) && (count + 256ll * r - 1) / (256ll * r) > 4096) r <<= 1;
    *rounds = r;
    *nblk = (int)((count + 256ll * r - 1) / (256ll * r));
}
// the digit passes that order keys of [0, limit]
static inline int lt_radix_passes(int64_t limit) {
    int bits = 1;
    while (bits < 31 && ((int64_t)1 << bits) <= limit) ++bits;
    return (bits + 7) / 8;
}
