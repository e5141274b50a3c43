// The probe primitive for the 3-layer model (GCN3, gcn/models.py:28-46; reached with --n-layer 3,
// gcn_trainer.py:81-86):   out = A (relu(A (relu(A (X W1) + b1) W2) + b2) W3) + b3
//
// Same idea as the 2-layer SPARSE mode, one hop deeper.  X + pert_v differs from X in row v only, so
//   S1 = X W1              changes in row v,
//   H1 = relu(A S1 + b1)   changes on R1 = {r : A[r,v] != 0},          S2 = H1 W2 on the same rows,
//   H2 = relu(A S2 + b2)   changes on R2 = {r2 : A[r2,r] != 0, r in R1}, S3 = H2 W3 on the same rows,
//   out = A S3 + b3        changes on the 3-hop set; only the observed rows are formed.
// Per probe chunk (no read-back: the GEMM's row count stays on the device, lt_launch_gemm_mdev):  level-1 items (b, r in R1) -> H1x rows (k3_rows_relu with row v substituted) -> one MFMA GEMM
// S2x = H1x W2 -> R2 by marking (k3_mark2: the thread that flips a bit appends the item) -> level-2 items (b, r2):
// k3_stageB runs the layer-2 chain of row r2 with the rows of R1 looked up in S2x (bitmap with positions), relu,
// . W3 -> S3x[b][r2] -> k3_stageC: layer-3 row of each observed node with the rows of R2 looked up in S3x, minus the
// baseline logits, / delta, L2 norm.
//
// Arithmetic = the fp32 finite difference of the reference (attacker.py:105-106), evaluated only where it can be
// non-zero: every recomputed row goes through the SAME device functions as the baseline forward below (row_dot chains
// started from the bias, relu_w2_partial + group_sum, row2_dot), so rows a probe cannot reach difference to exactly 0
// and rows it can reach carry only the perturbation and fp32 rounding -- the reference's noise class.
//
// A WIDE class layer (lt_baseline3_create_wide: 9 .. 256 classes, reddit / ppi) is served in LT_MODE_DELTA alone: the class width
// enters behind the layer-2 kink test, so the chain is the narrow one up to dH2 and the last two steps have wide forms (k3w_* /
// k3dw_* below).  Its level-2 tables are sized by n rows per probe, as S3x is: large graphs get small probe chunks.
//
// A LIST of (probe, observed) pairs (lt_influence3_pairs) takes the same chunk loop: only the last step reads the observed list, so
// levels 1 and 2 are launched as above and the observed-row kernels have a list form (k*_stageC_pairs) that runs the rectangle's
// per-cell device function (k3_cellC / k3d_cellC / k3dw_cellC) for pair k -- the bits of the rectangle by construction.
//
// The 2-LAYER model with a wide class layer (lt_baseline2w, at the end of this file) is the wide chain with one level removed and
// shares its kernels: k3d_items1, the MFMA product over the items, k3dw_stageC / k3dw_stageC_pairs over the level-1 tables.
#include <new>

#include "lt_items.hip.h"

#define LT_BLOCK 256
#define LT3_GRID 2048

struct lt_baseline3 {
    const lt_graph *g = nullptr;
    int32_t n = 0, F = 0, H1 = 0, H2 = 0, C = 0, Hp1 = 0, Hp2 = 0;
    const float *X = nullptr;
    int64_t ldx = 0;
    const float *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr, *W3 = nullptr, *b3 = nullptr;
    // owned
    float *S1 = nullptr;    // [n, Hp1]  X W1
    float *Act1 = nullptr;  // [n, Hp1]  H1 = relu(A S1 + b1)
    float *S2 = nullptr;    // [n, Hp2]  H1 W2
    float *Z2 = nullptr;    // [n, Hp2]  A S2 + b2
    float *S3 = nullptr;    // [n, C]    relu(Z2) W3
    float *OUT = nullptr;   // [n, C]    A S3 + b3
    float *b1p = nullptr, *b2p = nullptr, *W3p = nullptr;   // zero-padded to Hp1 / Hp2 / [Hp2, C]
    float *slabs = nullptr;     // split-K partials of X W1
    float *seg_part = nullptr;  // [g->p_n_seg, Hp2] segment sums of the hub rows (layer 2)
    // fp64 baseline for the exact (delta) propagation, lt_baseline3_enable_fp64: the layer-1 pre-activation Z1d lives in an
    // inner 2-layer baseline handle (its fp64 routes: feature rows / matrix cores), the layer-2 one here
    lt_baseline *l1 = nullptr;
    double *S2d = nullptr;      // [n, Hp2]  relu(Z1d) W2
    double *Z2d = nullptr;      // [n, Hp2]  A S2d + b2
    double *seg2d = nullptr;    // [lt_f64_seg_rows(g), Hp2]
    bool fp64_fresh = false;
    // lt_baseline3_refresh launches nothing (round 6, as lt_baseline_refresh since ABI 2): the padded parameters and the fp32 forward
    // are recomputed on the stream of the first call that reads them -- a LT_MODE_DELTA build reads no fp32 layer at all
    bool pad_fresh = false, fp32_fresh = false;
    // lt_baseline3_create_wide (C <= 256; LT_MODE_DELTA only): the class rows S3 / OUT have the stride Cp = C rounded up to 4 and
    // the last layer of the fp32 forward goes through the unfused product / SpMM
    bool wide = false;
    int32_t Cp = 0;
    float *b3p = nullptr;       // b3 zero-padded to Cp (an aligned bias for the SpMM's 16-byte path)
};

// h[dst] = relu(A[r,:] S + bias): all rows (items == NULL), or the level-1 items of a probe chunk, whose row reads
// Sp[b] in place of S[v] (the perturbed row of probe b)
template <int LPR>
__global__ __launch_bounds__(LT_BLOCK) void k3_rows_relu(
    int n_rows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S, int Hp, const float *__restrict__ biasp, float *__restrict__ out,
    const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const int32_t *__restrict__ probes, int nb,
    const int32_t *__restrict__ off, const float *__restrict__ Sp) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1);
    const int coff = 4 * gl;
    const bool active = coff < Hp;
    const bool items = off != nullptr;
    const int total = items ? off[nb] : n_rows;
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    for (int base = wave0 * RPW; base < total; base += nwaves * RPW) {
        const int it = base + lane / LPR;
        if (it >= total || !active) continue;
        int r = it, v = -1;
        const float *sub = nullptr;
        if (items) {
            const int b = find_probe(off, nb, it);
            v = probes[b];
            r = trow[tptr[v] + (it - off[b])];
            sub = Sp + (size_t)b * Hp;
        }
        const f32x4 z = row_dot<8>(col, val, rowptr[r], rowptr[r + 1], S, Hp, coff, true, v, sub, ld4(biasp + coff));
        f32x4 h;
        h.x = fmaxf(z.x, 0.f); h.y = fmaxf(z.y, 0.f); h.z = fmaxf(z.z, 0.f); h.w = fmaxf(z.w, 0.f);
        *reinterpret_cast<f32x4 *>(out + (size_t)it * Hp + coff) = h;
    }
}

// R2 of every probe: for each level-1 item (b, r) the rows r2 that read row r (CSC column r) are marked in the probe's bitmap
// (k3_mark2); k3_list2 then turns every probe's bitmap row into its level-2 items (b, r2) (order irrelevant: every item is
// computed on its own and lands in S3x[b][r2]).
// (Up to round 5 the thread that flipped a bit appended the item itself: one add per wave and trip on ONE word -- 9 K of them at
// twitch size, which that word's L2 channel serves one after the other: 105 us of a 0.35 ms GCN3 build.  Now the marks are
// fire-and-forget and the list costs one add per 256 bitmap words that hold anything.)
__global__ __launch_bounds__(LT_BLOCK) void k3_mark2(
    const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const int32_t *__restrict__ probes, int nb,
    const int32_t *__restrict__ off, int words, uint32_t *__restrict__ bits2, int32_t *__restrict__ n_items2) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_items2 = 0;      // (k3_list2's cursor: cleared here instead of by a memset of its own)
    const int total = off[nb];
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    for (int it = wave0; it < total; it += nwaves) {
        const int b = find_probe(off, nb, it);
        const int v = probes[b];
        const int r = trow[tptr[v] + (it - off[b])];
        for (int t = tptr[r] + lane; t < tptr[r + 1]; t += 64) {
            const int r2 = trow[t];
            atomicOr(&bits2[(size_t)b * words + (r2 >> 5)], 1u << (r2 & 31));
        }
    }
}
// one block per probe: its bitmap row, 256 words at a time -> items2 (a place per set bit behind one add per stretch)
__global__ __launch_bounds__(LT_BLOCK) void k3_list2(int words, const uint32_t *__restrict__ bits2, int2 *__restrict__ items2,
                                                     int32_t *__restrict__ n_items2) {
    __shared__ int s_wave[LT_BLOCK / 64];
    __shared__ int s_base;
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t *row = bits2 + (size_t)b * words;
    for (int w0 = 0; w0 < words; w0 += LT_BLOCK) {          // (block-uniform)
        const int w = w0 + threadIdx.x;
        uint32_t m = w < words ? row[w] : 0u;
        const int cnt = __popc(m);
        int incl = cnt;                                      // inclusive prefix over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wid] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < LT_BLOCK / 64; ++k) {
            before += k < wid ? s_wave[k] : 0;
            all += s_wave[k];
        }
        if (all > 0 && threadIdx.x == 0) s_base = atomicAdd(n_items2, all);
        __syncthreads();
        if (cnt > 0) {
            int pos = s_base + before + incl - cnt;
            while (m) {
                const int bit = __ffs((int)m) - 1;
                m &= m - 1u;
                items2[pos++] = make_int2(b, w * 32 + bit);
            }
        }
        __syncthreads();                                     // (s_wave / s_base are rewritten by the next stretch)
    }
}

// One CSR row against S2 with the rows of R1(b) replaced by their perturbed versions (S2x, found through the probe's
// bitmap with positions): row_dot's canonical order -- 128-entry fmaf chains, the first started from `init`, their
// sums added in segment order -- so an unperturbed row gives the bits of the baseline kernel.
__device__ __forceinline__ f32x4 row_dot_lookup(const int32_t *__restrict__ col, const float *__restrict__ val, int e0,
                                                int e1, const float *__restrict__ S, int ld, int coff,
                                                const uint2 *__restrict__ mb, const float *__restrict__ items, f32x4 init) {
    f32x4 total = init;
    for (int s0 = e0; s0 < e1 || s0 == e0; s0 += LT_ROW_SEG) {
        const int s1 = min(e1, s0 + LT_ROW_SEG);
        f32x4 acc = s0 == e0 ? init : f32x4{0.f, 0.f, 0.f, 0.f};
        int e = s0;
        for (; e + 4 <= s1; e += 4) {
            float a[4];
            f32x4 s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = col[e + k];
                a[k] = val[e + k];
                const int p = bits_pos(mb, c);
                s[k] = ld4((p >= 0 ? items + (size_t)p * ld : S + (size_t)c * ld) + coff);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = fma4(a[k], s[k], acc);
        }
        for (; e < s1; ++e) {
            const int c = col[e];
            const int p = bits_pos(mb, c);
            acc = fma4(val[e], ld4((p >= 0 ? items + (size_t)p * ld : S + (size_t)c * ld) + coff), acc);
        }
        if (s0 == e0) total = acc;
        else { total.x += acc.x; total.y += acc.y; total.z += acc.z; total.w += acc.w; }
        if (s1 >= e1) break;
    }
    return total;
}

// level-2 items: S3x[b][r2] = relu(A[r2,:] S2' + b2) . W3
template <int LPR, int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3_stageB(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S2, int Hp2, const float *__restrict__ b2p, const float *__restrict__ W3p, int C,
    const int32_t *__restrict__ off, const float *__restrict__ S2x, const uint2 *__restrict__ bits1, int words,
    const int2 *__restrict__ items2, const int32_t *__restrict__ n_items2, int n, float *__restrict__ S3x) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1);
    const int coff = 4 * gl;
    const bool active = coff < Hp2;
    const int total = *n_items2;
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    for (int base = wave0 * RPW; base < total; base += nwaves * RPW) {
        const int it = base + lane / LPR;
        const bool live = it < total;   // group-uniform; dead groups still join the shuffles
        float part[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) part[c] = 0.f;
        int b = 0, r2 = 0;
        if (live) {
            const int2 w = items2[it];
            b = w.x; r2 = w.y;
            if (active) {
                const f32x4 z = row_dot_lookup(col, val, rowptr[r2], rowptr[r2 + 1], S2, Hp2, coff,
                                               bits1 + (size_t)b * words, S2x + (size_t)off[b] * Hp2, ld4(b2p + coff));
                relu_w2_partial<CP>(z, W3p + (size_t)coff * C, C, part);
            }
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) part[c] = group_sum<LPR>(part[c]);
        if (live && gl == 0) {
#pragma unroll
            for (int c = 0; c < CP; ++c)
                if (c < C) S3x[((size_t)b * n + r2) * C + c] = part[c];
        }
    }
}

// The list form of the observed-row kernels (lt_influence3_pairs): a lane group owns pair k of the chunk instead of cell (b, j).  Its
// probe is the last b with pair_ptr[b] <= k (probes without pairs repeat an offset): a binary search in the chunk's slice of the device
// copy of the offsets, at most 16 steps (a chunk holds up to 65 534 probes) over lines that every group of the wave shares.  k is the
// same in all lanes of a group, so the search and everything behind it is group-uniform.
__device__ __forceinline__ int pair_owner(const int64_t *__restrict__ pair_ptr, int nb, long k) {
    int lo = 0, hi = nb;      // pair_ptr[lo] <= k < pair_ptr[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (pair_ptr[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

// observed rows: out[b][j] = || (A[u,:] S3' + b3 - OUT[u]) / delta ||, 8 lanes per (probe, observed node).  The cell (probe b of the
// chunk, observed node u) is ONE function for the rectangle and the list kernel: the two differ in how a group finds (b, u) and where
// lane 0 stores the value, nothing else.
template <int CP>
__device__ __forceinline__ float k3_cellC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S3, int C, const float *__restrict__ b3, const float *__restrict__ OUT, int n,
    const float *__restrict__ S3x, const uint32_t *__restrict__ bits2, int words, float delta, int b, int u, int q) {
    const uint32_t *mb = bits2 + (size_t)b * words;
    const float *mine = S3x + (size_t)b * n * C;
    const int e0 = rowptr[u], e1 = rowptr[u + 1];
    auto member = [&](int c) { return ((mb[c >> 5] >> (c & 31)) & 1u) != 0u; };
    bool touch = false;
    for (int e = e0 + q; e < e1; e += LT_L2_LANES) touch |= member(col[e]);
    int t = touch ? 1 : 0;
#pragma unroll
    for (int m = LT_L2_LANES / 2; m >= 1; m >>= 1) t |= __shfl_xor(t, m, 64);
    float res = 0.f;
    if (t) {
        float acc[CP];
        row2_dot<CP>(col, val, e0, e1, q, C,
                     [&](int c, int) { return member(c) ? mine + (size_t)c * C : S3 + (size_t)c * C; }, acc);
        res = diff_norm<CP>(acc, b3, OUT + (size_t)u * C, C, delta);
    }
    return res;
}
template <int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3_stageC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S3, int C, const float *__restrict__ b3, const float *__restrict__ OUT, int nb, int n,
    const float *__restrict__ S3x, const uint32_t *__restrict__ bits2, int words, const int32_t *__restrict__ observe,
    int n_obs, float delta, float *__restrict__ out, long ldo) {
    const long gid = ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LT_L2_LANES;
    const int q = threadIdx.x & (LT_L2_LANES - 1);
    if (gid >= (long)nb * n_obs) return;
    const int b = (int)(gid / n_obs), j = (int)(gid % n_obs);
    const float res = k3_cellC<CP>(rowptr, col, val, S3, C, b3, OUT, n, S3x, bits2, words, delta, b, observe[j], q);
    if (q == 0) out[(long)b * ldo + j] = res;
}
// the list form: pairs k0 .. k1 of the call are the chunk's (pair_ptr = the chunk's slice of the offsets, nb + 1 of them)
template <int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3_stageC_pairs(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S3, int C, const float *__restrict__ b3, const float *__restrict__ OUT, int nb, int n,
    const float *__restrict__ S3x, const uint32_t *__restrict__ bits2, int words, const int64_t *__restrict__ pair_ptr, long k0,
    long k1, const int32_t *__restrict__ pair_obs, float delta, float *__restrict__ out) {
    const long k = k0 + ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LT_L2_LANES;
    const int q = threadIdx.x & (LT_L2_LANES - 1);
    if (k >= k1) return;                                            // (group-uniform)
    const int b = pair_owner(pair_ptr, nb, k);
    const float res = k3_cellC<CP>(rowptr, col, val, S3, C, b3, OUT, n, S3x, bits2, words, delta, b, pair_obs[k], q);
    if (q == 0) out[k] = res;
}

// ---- exact propagation (LT_MODE_DELTA) for three layers ---------------------------------------------------------------
// The perturbation itself is pushed through the layers: dS1[v] = d * S1[v]; on the level-1 items dZ1[r] = A[r,v] dS1[v] and
// dH1 = relu(Z1 + dZ1) - relu(Z1) evaluated piecewise on the fp64 pre-activation (the kink test of the 2-layer delta mode);
// dS2 = dH1 W2 (the MFMA GEMM over the items); on the level-2 items dZ2[q] = sum over the members r of R1 in row q of
// A[q,r] dS2[r], dH2 likewise on the fp64 layer-2 pre-activation Z2d, dS3 = dH2 W3; the observed rows sum A[u,q] dS3[q] over
// the members of R2.  No subtraction of nearly equal numbers anywhere.
__device__ __forceinline__ float relu_diff(double z, float dz) {
    const double z1 = z + (double)dz;
    return z > 0.0 ? (z1 > 0.0 ? dz : (float)(-z)) : (z1 > 0.0 ? (float)z1 : 0.f);
}
template <int LPR>
__global__ __launch_bounds__(LT_BLOCK) void k3d_items1(
    const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const float *__restrict__ tval,
    const int32_t *__restrict__ probes, int nb, const int32_t *__restrict__ off, const double *__restrict__ Spd,
    const double *__restrict__ Z1d, int Hp, float delta, float *__restrict__ dH1x) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int coff = 4 * (lane & (LPR - 1));
    const int total = off[nb];
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    for (int base = wave0 * RPW; base < total; base += nwaves * RPW) {
        const int it = base + lane / LPR;
        if (it >= total || coff >= Hp) continue;
        const int b = find_probe(off, nb, it);
        const int v = probes[b];
        const int t = tptr[v] + (it - off[b]);
        const int r = trow[t];
        const float arv = tval[t];
        const double *sp = Spd + (size_t)b * Hp + coff, *zp = Z1d + (size_t)r * Hp + coff;
        f32x4 dh;
#pragma unroll
        for (int k = 0; k < 4; ++k) dh[k] = relu_diff(zp[k], arv * (delta * (float)sp[k]));
        *reinterpret_cast<f32x4 *>(dH1x + (size_t)it * Hp + coff) = dh;
    }
}

template <int LPR, int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3d_stageB(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const double *__restrict__ Z2d, int Hp2, const float *__restrict__ W3p, int C, const int32_t *__restrict__ off,
    const float *__restrict__ dS2x, const uint2 *__restrict__ bits1, int words, const int2 *__restrict__ items2,
    const int32_t *__restrict__ n_items2, int n, float *__restrict__ dS3x) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1);
    const int coff = 4 * gl;
    const bool active = coff < Hp2;
    const int total = *n_items2;
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    // (the lane's rows of W3 do not depend on the item: read once)
    float w3r[4][CP];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < CP; ++c) w3r[k][c] = (active && c < C) ? W3p[(size_t)(coff + k) * C + c] : 0.f;
    for (int base = wave0 * RPW; base < total; base += nwaves * RPW) {
        const int it = base + lane / LPR;
        const bool live = it < total;   // group-uniform; dead groups still join the shuffles
        float part[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) part[c] = 0.f;
        int b = 0, q = 0;
        if (live) {
            const int2 w = items2[it];
            b = w.x; q = w.y;
            const uint2 *mb = bits1 + (size_t)b * words;
            const float *items = dS2x + (size_t)off[b] * Hp2;
            f32x4 dz = {0.f, 0.f, 0.f, 0.f};
            // (the row's fp64 pre-activation goes out in front of the look-ups: nothing in them depends on it)
            double zq[4] = {0.0, 0.0, 0.0, 0.0};
            if (active) {
                const double2 z01 = *reinterpret_cast<const double2 *>(Z2d + (size_t)q * Hp2 + coff);
                const double2 z23 = *reinterpret_cast<const double2 *>(Z2d + (size_t)q * Hp2 + coff + 2);
                zq[0] = z01.x; zq[1] = z01.y; zq[2] = z23.x; zq[3] = z23.y;
            }
            // (round 6) the group's lanes look up LPR entries of the row side by side (column, membership word: two trips for the
            // stretch instead of two per entry -- the 18 dependent pairs of an average row were this launch's 94 us), then the members'
            // items are added in entry order: the same chain
            const int e_end = rowptr[q + 1], gbase = lane & ~(LPR - 1);
            for (int e0 = rowptr[q]; e0 < e_end; e0 += LPR) {            // (group-uniform)
                const int e = e0 + gl;
                int p = -1;
                float a = 0.f;
                if (e < e_end) {
                    p = bits_pos(mb, col[e]);
                    a = val[e];
                }
                unsigned long long hits = __ballot(p >= 0) >> gbase;
                if (LPR < 64) hits &= (1ull << LPR) - 1ull;
                while (hits) {                                           // members of R1 only, in entry order (group-uniform)
                    const int k = __ffsll((long long)hits) - 1;
                    hits &= hits - 1ull;
                    const int pk = __shfl(p, gbase + k, 64);
                    const float ak = __shfl(a, gbase + k, 64);
                    if (active) dz = fma4(ak, ld4(items + (size_t)pk * Hp2 + coff), dz);
                }
            }
            if (active) {
                float dh[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) dh[k] = relu_diff(zq[k], dz[k]);
#pragma unroll
                for (int c = 0; c < CP; ++c)
                    if (c < C) {
                        float pr = dh[0] * w3r[0][c];
                        pr = fmaf(dh[1], w3r[1][c], pr);
                        pr = fmaf(dh[2], w3r[2][c], pr);
                        pr = fmaf(dh[3], w3r[3][c], pr);
                        part[c] = pr;
                    }
            }
        }
#pragma unroll
        for (int c = 0; c < CP; ++c) part[c] = group_sum<LPR>(part[c]);
        if (live && gl == 0) {
#pragma unroll
            for (int c = 0; c < CP; ++c)
                if (c < C) dS3x[((size_t)b * n + q) * C + c] = part[c];
        }
    }
}

// (the cell is one function for the rectangle and the list kernel, as k3_cellC)
template <int CP>
__device__ __forceinline__ float k3d_cellC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int n,
    const float *__restrict__ dS3x, const uint32_t *__restrict__ bits2, int words, float delta, int b, int u, int q) {
    const uint32_t *mb = bits2 + (size_t)b * words;
    const float *mine = dS3x + (size_t)b * n * C;
    const int e0 = rowptr[u], e1 = rowptr[u + 1];
    auto member = [&](int c) { return ((mb[c >> 5] >> (c & 31)) & 1u) != 0u; };
    // (round 6: no pass over the row in front that only asks whether any entry is a member -- three hops reach most pairs at twitch
    // size, and a pair nothing reaches comes out of the sums as +0 all the same: 0 / delta, fma, sqrt)
    float acc[CP];
    row2_dot<CP>(col, val, e0, e1, q, C,
                 [&](int c, int) { return member(c) ? mine + (size_t)c * C : (const float *)nullptr; }, acc);
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) {
            const float d = acc[c] / delta;
            ss = fmaf(d, d, ss);
        }
    return sqrtf(ss);
}
template <int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3d_stageC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int nb, int n,
    const float *__restrict__ dS3x, const uint32_t *__restrict__ bits2, int words, const int32_t *__restrict__ observe,
    int n_obs, float delta, float *__restrict__ out, long ldo) {
    const long gid = ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LT_L2_LANES;
    const int q = threadIdx.x & (LT_L2_LANES - 1);
    if (gid >= (long)nb * n_obs) return;
    const int b = (int)(gid / n_obs), j = (int)(gid % n_obs);
    const float res = k3d_cellC<CP>(rowptr, col, val, C, n, dS3x, bits2, words, delta, b, observe[j], q);
    if (q == 0) out[(long)b * ldo + j] = res;
}
template <int CP>
__global__ __launch_bounds__(LT_BLOCK) void k3d_stageC_pairs(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int nb, int n,
    const float *__restrict__ dS3x, const uint32_t *__restrict__ bits2, int words, const int64_t *__restrict__ pair_ptr, long k0,
    long k1, const int32_t *__restrict__ pair_obs, float delta, float *__restrict__ out) {
    const long k = k0 + ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LT_L2_LANES;
    const int q = threadIdx.x & (LT_L2_LANES - 1);
    if (k >= k1) return;                                            // (group-uniform)
    const int b = pair_owner(pair_ptr, nb, k);
    const float res = k3d_cellC<CP>(rowptr, col, val, C, n, dS3x, bits2, words, delta, b, pair_obs[k], q);
    if (q == 0) out[k] = res;
}

// ---- LT_MODE_DELTA with a wide class layer (lt_baseline3_create_wide, C <= 256) ------------------------------------------------------
// The class width only enters behind the layer-2 kink test, so levels 1 and 2 are the chain above; the last two steps change:
// k3d_stageB's  . W3  in registers (CP <= 8 columns per lane) becomes one MFMA product over the level-2 items, dS3x = dH2x W3
// (row count on the device, as level 1), and k3d_stageC's 8 lanes x CP columns become a lane group ACROSS the class columns.
// For the product the level-2 items need a place each, known to the readers: k3w_rank2 turns a probe's marks (k3_mark2) into
// a bitmap row with positions, (mask, members of the probe below this word) -- what bits1 is for level 1 --, k3w_list2 adds
// the probes' offsets (off2[b] = members of the probes before b; off2[nb] = the chunk's count, which stays on the device) and
// lists the items: item (b, r2) sits at off2[b] + bits_pos(row_b, r2), a probe's items ascending in r2, the probes in order.
// Nothing here depends on which thread came first: a cell's value is a function of (probe, observed, model, graph) alone.
__global__ __launch_bounds__(LT_BLOCK) void k3w_rank2(int words, const uint32_t *__restrict__ bits2, uint2 *__restrict__ rank2,
                                                      int32_t *__restrict__ cnt2) {
    __shared__ int s_wave[LT_BLOCK / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t *row = bits2 + (size_t)b * words;
    int run = 0;                                             // members in the words before this stretch (the same in every thread)
    for (int w0 = 0; w0 < words; w0 += LT_BLOCK) {          // (block-uniform)
        const int w = w0 + threadIdx.x;
        const uint32_t m = w < words ? row[w] : 0u;
        const int cnt = __popc(m);
        int incl = cnt;                                      // inclusive prefix over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) s_wave[wid] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < LT_BLOCK / 64; ++k) {
            before += k < wid ? s_wave[k] : 0;
            all += s_wave[k];
        }
        if (w < words) rank2[(size_t)b * words + w] = make_uint2(m, (unsigned)(run + before + incl - cnt));
        run += all;
        __syncthreads();                                     // (s_wave is rewritten by the next stretch)
    }
    if (threadIdx.x == 0) cnt2[b] = run;
}
// one block per probe: its offset (every block sums the counts in front of it, as k_item_bits does for level 1), its items
__global__ __launch_bounds__(LT_BLOCK) void k3w_list2(int nb, int words, const uint2 *__restrict__ rank2,
                                                      const int32_t *__restrict__ cnt2, int32_t *__restrict__ off2,
                                                      int2 *__restrict__ items2) {
    __shared__ int32_t red[LT_BLOCK / 64];
    const int b = blockIdx.x;
    int part = 0;
    for (int i = threadIdx.x; i < b; i += LT_BLOCK) part += cnt2[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    int my_off = 0;
#pragma unroll
    for (int k = 0; k < LT_BLOCK / 64; ++k) my_off += red[k];
    if (threadIdx.x == 0) {
        off2[b] = my_off;
        if (b == nb - 1) off2[nb] = my_off + cnt2[b];
    }
    for (int w = threadIdx.x; w < words; w += LT_BLOCK) {
        const uint2 e = rank2[(size_t)b * words + w];
        uint32_t m = e.x;
        int pos = my_off + (int)e.y;
        while (m) {
            const int bit = __ffs((int)m) - 1;
            m &= m - 1u;
            items2[pos++] = make_int2(b, w * 32 + bit);
        }
    }
}

// level-2 items: k3d_stageB up to the kink test -- the same entry-order chain over the members of R1 in row q, the same
// relu_diff on the fp64 pre-activation -- and the row dH2x[item, 0 .. Hp2) stored instead of multiplied by W3
template <int LPR>
__global__ __launch_bounds__(LT_BLOCK) void k3dw_stageB(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const double *__restrict__ Z2d, int Hp2, const int32_t *__restrict__ off, const float *__restrict__ dS2x,
    const uint2 *__restrict__ bits1, int words, const int2 *__restrict__ items2, const int32_t *__restrict__ n_items2,
    float *__restrict__ dH2x) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1);
    const int coff = 4 * gl;
    const bool active = coff < Hp2;
    const int total = *n_items2;
    const int wave0 = (blockIdx.x * LT_BLOCK + threadIdx.x) >> 6;
    const int nwaves = gridDim.x * (LT_BLOCK / 64);
    for (int base = wave0 * RPW; base < total; base += nwaves * RPW) {
        const int it = base + lane / LPR;
        if (it >= total) continue;      // (group-uniform: the shuffles below stay inside the group)
        const int2 w = items2[it];
        const int b = w.x, q = w.y;
        const uint2 *mb = bits1 + (size_t)b * words;
        const float *items = dS2x + (size_t)off[b] * Hp2;
        f32x4 dz = {0.f, 0.f, 0.f, 0.f};
        double zq[4] = {0.0, 0.0, 0.0, 0.0};
        if (active) {
            const double2 z01 = *reinterpret_cast<const double2 *>(Z2d + (size_t)q * Hp2 + coff);
            const double2 z23 = *reinterpret_cast<const double2 *>(Z2d + (size_t)q * Hp2 + coff + 2);
            zq[0] = z01.x; zq[1] = z01.y; zq[2] = z23.x; zq[3] = z23.y;
        }
        const int e_end = rowptr[q + 1], gbase = lane & ~(LPR - 1);
        for (int e0 = rowptr[q]; e0 < e_end; e0 += LPR) {            // (group-uniform)
            const int e = e0 + gl;
            int p = -1;
            float a = 0.f;
            if (e < e_end) {
                p = bits_pos(mb, col[e]);
                a = val[e];
            }
            unsigned long long hits = __ballot(p >= 0) >> gbase;
            if (LPR < 64) hits &= (1ull << LPR) - 1ull;
            while (hits) {                                           // members of R1 only, in entry order (group-uniform)
                const int k = __ffsll((long long)hits) - 1;
                hits &= hits - 1ull;
                const int pk = __shfl(p, gbase + k, 64);
                const float ak = __shfl(a, gbase + k, 64);
                if (active) dz = fma4(ak, ld4(items + (size_t)pk * Hp2 + coff), dz);
            }
        }
        if (active) {
            f32x4 dh;
#pragma unroll
            for (int k = 0; k < 4; ++k) dh[k] = relu_diff(zq[k], dz[k]);
            *reinterpret_cast<f32x4 *>(dH2x + (size_t)it * Hp2 + coff) = dh;
        }
    }
}

// observed rows: one lane group per (probe, observed) cell, a lane per 4 class columns.  The entries of row u are walked in
// entry order (the group looks LPR of them up side by side, as stage B does), the members of R2 add fma(a, dS3x[pos][c], acc);
// then d = acc / delta, the lane's squares in column order, the lanes by the fixed butterfly, sqrt.  A cell no path reaches
// sums nothing: 0 / delta, fma, sqrt = +0.  (Columns C .. Cp of dS3x are never written: what they hold is carried along and
// left out of the squares.)
// (The cell is one function for the rectangle and the list kernel, as k3_cellC; every lane of the group returns the group's value.)
template <int LPR>
__device__ __forceinline__ float k3dw_cellC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int Cp,
    const float *__restrict__ dS3x, const uint2 *__restrict__ rank2, int words, const int32_t *__restrict__ off2, float delta, int b,
    int u, int gl, int gbase) {
    const int coff = 4 * gl;
    const bool active = coff < Cp;
    const uint2 *mb = rank2 + (size_t)b * words;
    const float *mine = dS3x + (size_t)off2[b] * Cp;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int e_end = rowptr[u + 1];
    for (int e0 = rowptr[u]; e0 < e_end; e0 += LPR) {               // (group-uniform)
        const int e = e0 + gl;
        int p = -1;
        float a = 0.f;
        if (e < e_end) {
            p = bits_pos(mb, col[e]);
            a = val[e];
        }
        unsigned long long hits = __ballot(p >= 0) >> gbase;
        if (LPR < 64) hits &= (1ull << LPR) - 1ull;
        while (hits) {                                              // members of R2 only, in entry order (group-uniform)
            const int k = __ffsll((long long)hits) - 1;
            hits &= hits - 1ull;
            const int pk = __shfl(p, gbase + k, 64);
            const float ak = __shfl(a, gbase + k, 64);
            if (active) acc = fma4(ak, ld4(mine + (size_t)pk * Cp + coff), acc);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (active && coff + k < C) {
            const float d = acc[k] / delta;
            ss = fmaf(d, d, ss);
        }
    ss = group_sum<LPR>(ss);
    return sqrtf(ss);
}
template <int LPR>
__global__ __launch_bounds__(LT_BLOCK) void k3dw_stageC(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int Cp, int nb,
    const float *__restrict__ dS3x, const uint2 *__restrict__ rank2, int words, const int32_t *__restrict__ off2,
    const int32_t *__restrict__ observe, int n_obs, float delta, float *__restrict__ out, long ldo) {
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1), gbase = lane & ~(LPR - 1);
    const long cell = ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LPR;
    if (cell >= (long)nb * n_obs) return;                           // (group-uniform)
    const int b = (int)(cell / n_obs), j = (int)(cell % n_obs);
    const float res = k3dw_cellC<LPR>(rowptr, col, val, C, Cp, dS3x, rank2, words, off2, delta, b, observe[j], gl, gbase);
    if (gl == 0) out[(long)b * ldo + j] = res;
}
template <int LPR>
__global__ __launch_bounds__(LT_BLOCK) void k3dw_stageC_pairs(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val, int C, int Cp, int nb,
    const float *__restrict__ dS3x, const uint2 *__restrict__ rank2, int words, const int32_t *__restrict__ off2,
    const int64_t *__restrict__ pair_ptr, long k0, long k1, const int32_t *__restrict__ pair_obs, float delta,
    float *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1), gbase = lane & ~(LPR - 1);
    const long k = k0 + ((long)blockIdx.x * LT_BLOCK + threadIdx.x) / LPR;
    if (k >= k1) return;                                            // (group-uniform)
    const int b = pair_owner(pair_ptr, nb, k);
    const float res = k3dw_cellC<LPR>(rowptr, col, val, C, Cp, dS3x, rank2, words, off2, delta, b, pair_obs[k], gl, gbase);
    if (gl == 0) out[k] = res;
}

__global__ void k3w_pad_b3(const float *__restrict__ b3, int C, int Cp, float *__restrict__ b3p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Cp) b3p[i] = i < C ? b3[i] : 0.f;
}

__global__ void k3_pad(const float *__restrict__ b1, int H1, int Hp1, const float *__restrict__ b2, int H2, int Hp2,
                       const float *__restrict__ W3, int C, float *__restrict__ b1p, float *__restrict__ b2p,
                       float *__restrict__ W3p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Hp1) b1p[i] = i < H1 ? b1[i] : 0.f;
    if (i < Hp2) b2p[i] = i < H2 ? b2[i] : 0.f;
    if (i < Hp2 * C) W3p[i] = (i / C) < H2 ? W3[i] : 0.f;
}

// ------------------------------------------------------------------------------------------------
static void free_baseline3(lt_baseline3 *b) {
    if (!b) return;
    (void)hipFree(b->S1); (void)hipFree(b->Act1); (void)hipFree(b->S2); (void)hipFree(b->Z2); (void)hipFree(b->S3);
    (void)hipFree(b->OUT); (void)hipFree(b->b1p); (void)hipFree(b->b2p); (void)hipFree(b->W3p); (void)hipFree(b->slabs);
    (void)hipFree(b->seg_part); (void)hipFree(b->b3p);
    (void)hipFree(b->S2d); (void)hipFree(b->Z2d); (void)hipFree(b->seg2d);
    if (b->l1) (void)lt_baseline_destroy(b->l1);
    delete b;
}

static inline unsigned blocks_for(long n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

extern "C" int lt_baseline3_refresh(lt_baseline3 *b, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_baseline3_refresh: baseline is NULL");
    b->fp64_fresh = b->pad_fresh = b->fp32_fresh = false;
    if (b->l1) (void)lt_baseline_refresh(b->l1, stream);
    return LT_OK;
}

extern "C" int lt_baseline3_features_changed(lt_baseline3 *b, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_baseline3_features_changed: baseline is NULL");
    b->fp64_fresh = b->pad_fresh = b->fp32_fresh = false;
    return b->l1 ? lt_baseline_features_changed(b->l1, stream) : LT_OK;
}

// b1 / b2 / W3 zero-padded to the padded widths (read by the fp32 forward, the fp64 layer-2 pre-activation and the probes' kernels)
static int ensure3_pad(const lt_baseline3 *cb, hipStream_t st) {
    lt_baseline3 *b = const_cast<lt_baseline3 *>(cb);   // cache state only
    if (b->pad_fresh || b->n == 0) return LT_OK;
    const int mx = (b->Hp1 > b->Hp2 * b->C ? b->Hp1 : b->Hp2 * b->C);
    hipLaunchKernelGGL(k3_pad, dim3((mx + 255) / 256), dim3(256), 0, st, b->b1, b->H1, b->Hp1, b->b2, b->H2, b->Hp2, b->W3,
                       b->C, b->b1p, b->b2p, b->W3p);
    LT_CHECK_LAUNCH();
    if (b->wide) {
        hipLaunchKernelGGL(k3w_pad_b3, dim3((b->Cp + 255) / 256), dim3(256), 0, st, b->b3, b->C, b->Cp, b->b3p);
        LT_CHECK_LAUNCH();
    }
    b->pad_fresh = true;
    return LT_OK;
}

// the unperturbed fp32 forward (the fp32 finite difference's baseline, lt_baseline3_logits)
static int ensure3_fp32(const lt_baseline3 *cb, hipStream_t st) {
    lt_baseline3 *b = const_cast<lt_baseline3 *>(cb);   // cache state only
    if (b->fp32_fresh || b->n == 0) return LT_OK;
    int rc = ensure3_pad(b, st);
    if (rc) return rc;
    const lt_graph *g = b->g;
    const int n = b->n;
    // S1 = X W1 (pad columns zero)
    if (b->Hp1 != b->H1) LT_HIP(hipMemsetAsync(b->S1, 0, (size_t)n * b->Hp1 * sizeof(float), st));
    rc = b->slabs ? lt_launch_gemm_splitk(b->X, b->ldx, b->W1, b->H1, b->S1, b->Hp1, n, b->H1, b->F,
                                          lt_gemm_pick_kslice(n, b->H1, b->F), b->slabs, st)
                  : lt_launch_gemm(b->X, b->ldx, b->W1, b->H1, b->S1, b->Hp1, n, b->H1, b->F, st);
    if (rc) return rc;
    // H1 = relu(A S1 + b1)
    const int lpr1 = lt_lpr_for(b->Hp1);
    LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k3_rows_relu<LPR_>), dim3(blocks_for(n, (LT_BLOCK / 64) * (64 / lpr1))),
                                             dim3(LT_BLOCK), 0, st, n, g->rowptr, g->col, g->val, b->S1, b->Hp1, b->b1p, b->Act1,
                                             (const int32_t *)nullptr, (const int32_t *)nullptr, (const int32_t *)nullptr, 0,
                                             (const int32_t *)nullptr, (const float *)nullptr));
    LT_CHECK_LAUNCH();
    // S2 = H1 W2
    if (b->Hp2 != b->H2) LT_HIP(hipMemsetAsync(b->S2, 0, (size_t)n * b->Hp2 * sizeof(float), st));
    rc = lt_launch_gemm(b->Act1, b->Hp1, b->W2, b->H2, b->S2, b->Hp2, n, b->H2, b->H1, st);
    if (rc) return rc;
    if (b->wide) {
        // the class layer unfused: H2 = relu(A S2 + b2) (into Z2), S3 = H2 W3, OUT = A S3 + b3 -- the SpMM's wide row kernels,
        // the MFMA product; rows of stride Cp
        rc = lt_spmm_csr_f32(g, b->S2, b->Hp2, b->Hp2, b->b2p, 1, b->Z2, b->Hp2, st);
        if (rc) return rc;
        rc = lt_launch_gemm(b->Z2, b->Hp2, b->W3, b->C, b->S3, b->Cp, n, b->C, b->H2, st);
        if (rc) return rc;
        rc = lt_spmm_csr_f32(g, b->S3, b->Cp, b->C, b->b3p, 0, b->OUT, b->Cp, st);
        if (rc) return rc;
        b->fp32_fresh = true;
        return LT_OK;
    }
    // S3 = relu(A S2 + b2) W3, OUT = A S3 + b3: the fused layer kernels of the 2-layer path
    rc = lt_launch_layer1(g, b->S2, b->Hp2, b->b2p, b->W3p, b->C, b->Z2, b->S3, st, b->seg_part);
    if (rc) return rc;
    rc = lt_launch_layer2(g, b->S3, b->C, b->b3, b->OUT, st);
    if (rc) return rc;
    b->fp32_fresh = true;
    return LT_OK;
}

#define LT3_WIDE_MAX_C 256     // classes of a wide handle: one lane group of k3dw_stageC (64 lanes x 4 columns)
// `fn` = the entry point's name in the messages; max_c = LT_MAX_C (the fused class layer) or LT3_WIDE_MAX_C (a wide handle)
static int baseline3_create(const char *fn, bool wide, const lt_graph *g, const float *X, int64_t ldx, int32_t F, const float *W1,
                            const float *b1, int32_t H1, const float *W2, const float *b2, int32_t H2, const float *W3,
                            const float *b3, int32_t C, void *stream, lt_baseline3 **out) {
    const int max_c = wide ? LT3_WIDE_MAX_C : LT_MAX_C;
    LT_REQUIRE(out != nullptr, "%s: out is NULL", fn);
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "%s: graph is NULL", fn);
    LT_REQUIRE(F > 0 && H1 > 0 && H2 > 0 && C > 0, "%s: F=%d H1=%d H2=%d C=%d must be positive", fn, F, H1, H2, C);
    if (H1 > LT_MAX_H || H2 > LT_MAX_H || C > max_c)
        return lt_set_error(LT_ERR_UNSUPPORTED, "%s: H1=%d H2=%d C=%d (supported: H <= %d, C <= %d)", fn, H1, H2, C, LT_MAX_H, max_c);
    LT_REQUIRE(X && W1 && b1 && W2 && b2 && W3 && b3, "%s: NULL tensor pointer", fn);
    LT_REQUIRE(ldx >= F, "%s: ldx=%lld < F=%d", fn, (long long)ldx, F);
    (void)lt_node_err_dev();      // (allocated outside any stream capture)
    lt_baseline3 *b = new (std::nothrow) lt_baseline3();
    if (!b) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", fn);
    b->g = g; b->n = g->n; b->F = F; b->H1 = H1; b->H2 = H2; b->C = C;
    b->Hp1 = lt_round_up(H1, 4); b->Hp2 = lt_round_up(H2, 4);
    b->wide = wide; b->Cp = lt_round_up(C, 4);
    const size_t ldc = wide ? (size_t)b->Cp : (size_t)C;      // row stride of S3 / OUT
    b->X = X; b->ldx = ldx; b->W1 = W1; b->b1 = b1; b->W2 = W2; b->b2 = b2; b->W3 = W3; b->b3 = b3;
    const size_t n1 = (size_t)(b->n > 0 ? b->n : 1);
#define B3_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            free_baseline3(b);                                                              \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)
    B3_HIP(hipMalloc((void **)&b->S1, n1 * b->Hp1 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->Act1, n1 * b->Hp1 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->S2, n1 * b->Hp2 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->Z2, n1 * b->Hp2 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->S3, n1 * ldc * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->OUT, n1 * ldc * sizeof(float)));
    if (wide) B3_HIP(hipMalloc((void **)&b->b3p, (size_t)b->Cp * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->b1p, (size_t)b->Hp1 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->b2p, (size_t)b->Hp2 * sizeof(float)));
    B3_HIP(hipMalloc((void **)&b->W3p, (size_t)b->Hp2 * C * sizeof(float)));
    if (g->p_n_seg > 0) B3_HIP(hipMalloc((void **)&b->seg_part, (size_t)g->p_n_seg * b->Hp2 * sizeof(float)));
    const size_t sb = lt_gemm_splitk_slab_bytes(b->n, H1, F, lt_gemm_pick_kslice(b->n, H1, F));
    if (sb) B3_HIP(hipMalloc((void **)&b->slabs, sb));
#undef B3_HIP
    const int rc = lt_baseline3_refresh(b, stream);
    if (rc) {
        free_baseline3(b);
        return rc;
    }
    *out = b;
    return LT_OK;
}

extern "C" int lt_baseline3_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const float *W1,
                                   const float *b1, int32_t H1, const float *W2, const float *b2, int32_t H2,
                                   const float *W3, const float *b3, int32_t C, void *stream, lt_baseline3 **out) {
    return baseline3_create("lt_baseline3_create", false, g, X, ldx, F, W1, b1, H1, W2, b2, H2, W3, b3, C, stream, out);
}

// The same handle for a class layer of up to LT3_WIDE_MAX_C columns: LT_MODE_DELTA only (the wide chain above), logits through
// the unfused class layer.  C <= LT_MAX_C is allowed and takes the wide kernels all the same.
extern "C" int lt_baseline3_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const float *W1,
                                        const float *b1, int32_t H1, const float *W2, const float *b2, int32_t H2,
                                        const float *W3, const float *b3, int32_t C, void *stream, lt_baseline3 **out) {
    return baseline3_create("lt_baseline3_create_wide", true, g, X, ldx, F, W1, b1, H1, W2, b2, H2, W3, b3, C, stream, out);
}

extern "C" int lt_baseline3_destroy(lt_baseline3 *b) {
    free_baseline3(b);
    return LT_OK;
}

extern "C" int lt_baseline3_logits(const lt_baseline3 *b, float *dst, void *stream) {
    LT_REQUIRE(b != nullptr && dst != nullptr, "lt_baseline3_logits: NULL argument");
    if (b->n == 0) return LT_OK;
    { const int rc = ensure3_fp32(b, (hipStream_t)stream); if (rc) return rc; }
    if (b->wide && b->Cp != b->C) {      // rows of stride Cp -> the caller's dense [n, C]
        LT_HIP(hipMemcpy2DAsync(dst, (size_t)b->C * sizeof(float), b->OUT, (size_t)b->Cp * sizeof(float), (size_t)b->C * sizeof(float),
                                (size_t)b->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return LT_OK;
    }
    LT_HIP(hipMemcpyAsync(dst, b->OUT, (size_t)b->n * b->C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

// fp64 baseline of the first two layers (the kink tests of LT_MODE_DELTA): Z1d through an inner 2-layer handle over the
// same borrowed X / W1 / b1 (so that it takes the fp64 product routes of lt_fp64.hip), S2d = relu(Z1d) W2 and
// Z2d = A S2d + b2 here.  Costs one more copy of the layer-1 buffers; redone after every lt_baseline3_refresh when next needed.
extern "C" int lt_baseline3_enable_fp64(lt_baseline3 *b, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_baseline3_enable_fp64: baseline is NULL");
    if (b->Z2d) return LT_OK;
    lt_baseline *l1 = nullptr;
    // (W2 / b2 of the inner handle are never used for arithmetic: only its fp64 pre-activation is read; C = 1 keeps its
    // padding kernel inside W2's first H1 floats)
    int rc = lt_baseline_create(b->g, b->X, b->ldx, b->F, b->W1, b->b1, b->H1, b->W2, b->b2, 1, stream, &l1);
    if (rc) return rc;
    l1->no_agg = true;
    rc = lt_baseline_enable_fp64(l1, stream);
    if (rc) { (void)lt_baseline_destroy(l1); return rc; }
    const size_t n1 = (size_t)(b->n > 0 ? b->n : 1);
    double *s2d = nullptr, *z2d = nullptr, *seg = nullptr;
    hipError_t e = hipMalloc((void **)&s2d, n1 * b->Hp2 * sizeof(double));
    if (e == hipSuccess) e = hipMemsetAsync(s2d, 0, n1 * b->Hp2 * sizeof(double), (hipStream_t)stream);   // pad columns stay zero
    if (e == hipSuccess) e = hipMalloc((void **)&z2d, n1 * b->Hp2 * sizeof(double));
    if (e == hipSuccess && lt_f64_seg_rows(b->g) > 0) e = hipMalloc((void **)&seg, (size_t)lt_f64_seg_rows(b->g) * b->Hp2 * sizeof(double));
    if (e != hipSuccess) {
        (void)hipFree(s2d); (void)hipFree(z2d); (void)hipFree(seg); (void)lt_baseline_destroy(l1);
        return lt_set_error(LT_ERR_HIP, "lt_baseline3_enable_fp64: hipMalloc failed: %s", hipGetErrorString(e));
    }
    b->l1 = l1; b->S2d = s2d; b->Z2d = z2d; b->seg2d = seg;
    b->fp64_fresh = false;
    return LT_OK;
}

static int ensure3_fp64(const lt_baseline3 *cb, hipStream_t st) {
    lt_baseline3 *b = const_cast<lt_baseline3 *>(cb);   // cache state only
    if (b->fp64_fresh || b->n == 0) return LT_OK;
    int rc = ensure3_pad(b, st);                        // (b2p below)
    if (rc) return rc;
    rc = lt_fp64_form_all(b->l1, st);                   // Z1d, every row
    if (rc) return rc;
    rc = lt_launch_gemm_f64_dense(b->l1->Z1d, (long)b->Hp1, b->n, b->W2, (long)b->H2, b->H2, b->H1, nullptr, b->S2d, (long)b->Hp2, 1, st);
    if (rc) return rc;
    rc = lt_launch_spmm_f64(b->g, b->S2d, b->Hp2, b->b2p, b->Z2d, b->seg2d, st);
    if (rc) return rc;
    b->fp64_fresh = true;
    return LT_OK;
}

// ---- workspace ------------------------------------------------------------------------------
struct infl3_ws {
    float *Sp, *slabs, *H1x, *S2x, *S3x;
    double *Spd;            // delta: fp64 product rows of the chunk's probes [chunk, Hp1]
    int32_t *off, *n_items2;
    uint2 *bits1;
    uint32_t *bits2;
    int2 *items2;
    int32_t *probes_s, *obs_s;    // the call's lists, every id checked against [0, n) (lt_items.hip.h k_check_nodes)
    int64_t *pair_ptr;            // lt_influence3_pairs: the device copy of pair_ptr [n_probe + 1] (obs_s is then [n_pairs])
    // a wide handle (delta only; S3x = dS3x [items2, Cp]): the level-2 bitmap with positions, the probes' counts and offsets, dH2x
    uint2 *rank2;
    int32_t *cnt2, *off2;
    float *dH2x;
    size_t bytes;
    int chunk;
};

static int probe_kslice3(const lt_baseline3 *b) { return lt_gemm_pick_kslice(b->n, b->H1, b->F); }

// n_pairs >= 0: the carve of lt_influence3_pairs (n_obs = 0) -- the checked observed list is sized by the pair list and the offsets'
// device copy follows it; the chunk and every per-chunk table are those of the rows call
static infl3_ws carve3(void *base, const lt_baseline3 *b, int n_probe, int n_obs, int64_t n_pairs = -1) {
    infl3_ws w = {};
    const size_t n = (size_t)b->n, C = (size_t)b->C, Hp1 = (size_t)b->Hp1, Hp2 = (size_t)b->Hp2;
    const size_t maxc = (size_t)(b->g->max_col_nnz > 0 ? b->g->max_col_nnz : 1);
    const size_t words = (n + 31) / 32;
    const size_t splitk = (((size_t)b->F + probe_kslice3(b) - 1) / probe_kslice3(b)) * (size_t)b->H1;
    // (a wide handle: no fp32 product rows, and the level-2 tables -- dH2x, dS3x, the items -- by the upper bound of n rows per
    // probe, as S3x is for a narrow one: a large graph gets small chunks)
    const size_t Cp = (size_t)b->Cp;
    const size_t per_probe_wide = Hp1 * sizeof(double) + (maxc * (Hp1 + Hp2) + n * (Hp2 + Cp)) * sizeof(float) + n * sizeof(int2) +
                                  words * (2 * sizeof(uint2) + sizeof(uint32_t)) + 3 * sizeof(int32_t);
    const size_t per_probe = b->wide ? per_probe_wide :
                             (Hp1 + splitk + maxc * (Hp1 + Hp2) + n * C) * sizeof(float) + n * sizeof(int2) +
                             words * (sizeof(uint2) + sizeof(uint32_t)) + sizeof(int32_t);
    size_t chunk = (size_t)lt_tune().chunk_budget / per_probe;
    if (chunk < 1) chunk = 1;
    if (chunk > 65534) chunk = 65534;
    if (chunk > (size_t)(n_probe > 0 ? n_probe : 1)) chunk = (size_t)(n_probe > 0 ? n_probe : 1);
    w.chunk = (int)chunk;
    size_t offb = 0;
    char *p = (char *)base;
    auto take = [&](size_t bytes) {
        void *q = p ? (void *)(p + offb) : nullptr;
        offb += lt_align_up(bytes ? bytes : 1, 256);
        return q;
    };
    if (b->wide) {
        w.Spd = (double *)take(chunk * Hp1 * sizeof(double));
        w.off = (int32_t *)take((chunk + 1) * sizeof(int32_t));
        w.n_items2 = (int32_t *)take(sizeof(int32_t));
        w.H1x = (float *)take(chunk * maxc * Hp1 * sizeof(float));
        w.S2x = (float *)take(chunk * maxc * Hp2 * sizeof(float));
        w.bits1 = (uint2 *)take(chunk * words * sizeof(uint2));
        w.bits2 = (uint32_t *)take(chunk * words * sizeof(uint32_t));
        w.rank2 = (uint2 *)take(chunk * words * sizeof(uint2));
        w.cnt2 = (int32_t *)take(chunk * sizeof(int32_t));
        w.off2 = (int32_t *)take((chunk + 1) * sizeof(int32_t));
        w.items2 = (int2 *)take(chunk * n * sizeof(int2));
        w.dH2x = (float *)take(chunk * n * Hp2 * sizeof(float));
        w.S3x = (float *)take(chunk * n * Cp * sizeof(float));
        w.probes_s = (int32_t *)take((size_t)(n_probe > 0 ? n_probe : 1) * sizeof(int32_t));
        w.obs_s = (int32_t *)take((n_pairs >= 0 ? (size_t)n_pairs : (size_t)(n_obs > 0 ? n_obs : 1)) * sizeof(int32_t));
        if (n_pairs >= 0) w.pair_ptr = (int64_t *)take(((size_t)n_probe + 1) * sizeof(int64_t));
        w.bytes = offb;
        return w;
    }
    w.Sp = (float *)take(chunk * Hp1 * sizeof(float));
    w.Spd = (double *)take(chunk * Hp1 * sizeof(double));
    w.slabs = (float *)take(lt_gemm_splitk_slab_bytes((int)chunk, b->H1, b->F, probe_kslice3(b)));
    w.off = (int32_t *)take((chunk + 1) * sizeof(int32_t));
    w.n_items2 = (int32_t *)take(sizeof(int32_t));
    w.H1x = (float *)take(chunk * maxc * Hp1 * sizeof(float));
    w.S2x = (float *)take(chunk * maxc * Hp2 * sizeof(float));
    w.bits1 = (uint2 *)take(chunk * words * sizeof(uint2));
    w.bits2 = (uint32_t *)take(chunk * words * sizeof(uint32_t));
    w.items2 = (int2 *)take(chunk * n * sizeof(int2));
    w.S3x = (float *)take(chunk * n * C * sizeof(float));
    w.probes_s = (int32_t *)take((size_t)(n_probe > 0 ? n_probe : 1) * sizeof(int32_t));
    w.obs_s = (int32_t *)take((n_pairs >= 0 ? (size_t)n_pairs : (size_t)(n_obs > 0 ? n_obs : 1)) * sizeof(int32_t));
    if (n_pairs >= 0) w.pair_ptr = (int64_t *)take(((size_t)n_probe + 1) * sizeof(int64_t));
    w.bytes = offb;
    return w;
}

extern "C" size_t lt_influence3_workspace_bytes(const lt_baseline3 *b, int32_t n_probe, int32_t n_obs) {
    if (!b || n_probe < 0 || n_obs < 0) return 0;
    return carve3(nullptr, b, n_probe, n_obs).bytes;
}

// ---- what the rows and pairs calls of lt_baseline3 and lt_baseline2w share (influence3_impl, influence3_wide_chunks, influence2w_impl) ----
// The front of a call: everything that refuses it before its first launch.  fn: the entry point that was called; serves(): the handle's
// own word on a known mode (a return code).  A pair list (pj; lt_internal.h) brings the observed ids of the call.  *go = false with
// LT_OK: an empty list, nothing to do.
template <class Serves>
static int probe_front(const char *fn, int32_t n, int32_t mode, Serves serves, const int32_t *probe_nodes, int32_t n_probe,
                       const int32_t **observe_nodes, int32_t n_obs, float delta, const float *out, int64_t ldo, const void *workspace,
                       size_t workspace_bytes, size_t need, const lt_pairs_job *pj, bool *go) {
    *go = false;
    LT_REQUIRE(mode == LT_MODE_SPARSE || mode == LT_MODE_FULL || mode == LT_MODE_DELTA, "%s: unknown mode %d", fn, mode);
    { const int rc = serves(); if (rc) return rc; }
    LT_REQUIRE(n_probe >= 0 && n_obs >= 0, "%s: negative count", fn);
    LT_REQUIRE(delta != 0.f && delta == delta, "%s: delta must be a non-zero number", fn);
    if (n_probe == 0 || (pj ? pj->n_pairs == 0 : n_obs == 0)) return LT_OK;
    if (pj) *observe_nodes = pj->obs;
    LT_REQUIRE(probe_nodes && *observe_nodes && out, "%s: NULL pointer", fn);
    LT_REQUIRE(pj || ldo >= n_obs, "%s: ldo=%lld < n_obs=%d", fn, (long long)ldo, n_obs);
    LT_REQUIRE(n > 0, "%s: empty graph", fn);
    { const int rc = lt_node_err_pending(); if (rc) return rc; }     // an earlier call's list held an id out of range
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % 256))
        return lt_set_error(LT_ERR_WORKSPACE, "%s: workspace needs %zu bytes, 256-byte aligned", fn, need);
    *go = true;
    return LT_OK;
}

// Every chunk's grid limits, before anything is enqueued: the lane groups of the chunk's last launch (`lanes` per cell) and the launches
// over the chunk's items (at most rows_max per probe; 0: the carve keeps that product an int).  A chunk of a pair list whose probes own
// no pair launches nothing.
static int probe_chunk_limits(const char *fn, int n_probe, int chunk, int n_obs, const lt_pairs_job *pj, int lanes, long rows_max) {
    for (int p0 = 0; p0 < n_probe; p0 += chunk) {
        const int nb = (n_probe - p0) < chunk ? (n_probe - p0) : chunk;
        const long cells = pj ? (long)(pj->ptr[p0 + nb] - pj->ptr[p0]) : (long)nb * n_obs;
        if (pj && cells == 0) continue;
        LT_REQUIRE((cells * lanes + LT_BLOCK - 1) / LT_BLOCK < 2147483647L, "%s: %ld cells per chunk of %d probes exceed the grid limit",
                   fn, cells, nb);
        LT_REQUIRE((long)nb * rows_max < 2147483647L, "%s: %d probes x %ld rows per chunk exceed the grid limit", fn, nb, rows_max);
    }
    return LT_OK;
}

// Node ids: both lists checked into the workspace, which the call reads from then on (the first reader is a GEMM that gathers
// X[probes]).  A pair list: pair_obs is the observed list of the check -- LT_PAIRS_MAX keeps the two counts' sum an int -- and the
// offsets go to the device behind it by one stream-ordered copy.
static int probe_check_nodes(int n, const int32_t **probe_nodes, int n_probe, const int32_t **observe_nodes, int n_obs,
                             const lt_pairs_job *pj, int32_t *probes_s, int32_t *obs_s, int64_t *pair_ptr_dev, hipStream_t st) {
    const long n_list = pj ? (long)pj->n_pairs : (long)n_obs, tot = (long)n_probe + n_list;
    hipLaunchKernelGGL(k_check_nodes, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, *probe_nodes, n_probe, *observe_nodes,
                       (int)n_list, n, probes_s, obs_s, lt_node_err_dev());
    LT_CHECK_LAUNCH();
    *probe_nodes = probes_s;
    *observe_nodes = obs_s;
    if (pj) LT_HIP(hipMemcpyAsync(pair_ptr_dev, pj->ptr, ((size_t)n_probe + 1) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    return LT_OK;
}

// Level 1 of the exact chain for a chunk's probes, over the inner baseline l1 of (X, W1, b1): the probes' own product rows in fp64
// (dS1[v] = d * S1[v]) -- read off the inner baseline's product where it holds one (formed for every row: the 2-layer stage A reads a
// probe's row the same way; X[probes] W1 over again on the f64 cores was 0.40 of the 0.87 ms this build took at twitch size, round 6),
// formed here on the aggregate-first route --, the level-1 bitmap with positions (bits1, off) and dH1x on the fp64 pre-activation.
static int exact_level1(const lt_graph *g, const lt_baseline *l1, const float *X, int64_t ldx, const float *W1, int F, int H, int Hp,
                        int lpr1, const int32_t *probes, int nb, int words, double *Spd, uint2 *bits1, int32_t *off, float delta,
                        float *dH1x, hipStream_t st) {
    int rc = lt_tune().gcn3_product_gather != 0 ? lt_fp64_product_rows_gather(l1, probes, nb, Spd, (long)Hp, st) : 1;
    if (rc == 1) {
        if (Hp != H) LT_HIP(hipMemsetAsync(Spd, 0, (size_t)nb * Hp * sizeof(double), st));
        rc = lt_launch_gemm_f64_gather(X, (long)ldx, probes, nb, W1, (long)H, H, F, Spd, (long)Hp, st);
    }
    if (rc) return rc;
    hipLaunchKernelGGL(k_item_bits, dim3(nb), dim3(256), 0, st, g->tptr, g->trow, probes, nb, words, bits1, off, (int2 *)nullptr, (uint2 *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
    LT_CHECK_LAUNCH();
    LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k3d_items1<LPR_>), dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->tptr, g->trow, g->tval, probes,
                                             nb, off, Spd, l1->Z1d, Hp, delta, dH1x));
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// The last launch of a wide chunk, the observed rows: the cells of probes [p0, p0 + nb) x the observed list into the rectangle, or the
// chunk's pairs [k0, k1) into out[k], over the tables (dSx, rank, off) of the level in front (k3dw_stageC / k3dw_stageC_pairs).
static int wide_observed_rows(const lt_graph *g, int C, int Cp, int lprc, int p0, int nb, const float *dSx, const uint2 *rank, int words,
                              const int32_t *off, const lt_pairs_job *pj, const int64_t *pair_ptr_dev, long k0, long k1,
                              const int32_t *observe_nodes, int n_obs, float delta, float *out, int64_t ldo, hipStream_t st) {
    const long cells = pj ? k1 - k0 : (long)nb * n_obs;
    const unsigned gridC = (unsigned)((cells * lprc + LT_BLOCK - 1) / LT_BLOCK);
    if (pj) {
        LT_DISPATCH_LPR(lprc, hipLaunchKernelGGL((k3dw_stageC_pairs<LPR_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col,
                                                 g->val, C, Cp, nb, dSx, rank, words, off, pair_ptr_dev + p0, k0, k1, observe_nodes,
                                                 delta, out));
    } else {
        LT_DISPATCH_LPR(lprc, hipLaunchKernelGGL((k3dw_stageC<LPR_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val,
                                                 C, Cp, nb, dSx, rank, words, off, observe_nodes, n_obs, delta,
                                                 out + (int64_t)p0 * ldo, (long)ldo));
    }
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// The probe chunks of a wide handle (LT_MODE_DELTA; the lists are the checked ones, the fp64 pre-activations are fresh, the grid limits
// hold): level 1 as for a narrow handle, then the wide forms of the last two steps (k3w_rank2 ... k3dw_stageC above).  Enqueue only.
static int influence3_wide_chunks(const lt_baseline3 *b, const infl3_ws &w, const int32_t *probe_nodes, int n_probe,
                                  const int32_t *observe_nodes, int n_obs, float delta, float *out, int64_t ldo, hipStream_t st,
                                  const lt_pairs_job *pj) {
    const lt_graph *g = b->g;
    const int n = b->n, C = b->C, Cp = b->Cp, Hp1 = b->Hp1, Hp2 = b->Hp2;
    const int lpr1 = lt_lpr_for(Hp1), lpr2 = lt_lpr_for(Hp2), lprc = lt_lpr_for(Cp);
    const int words = (n + 31) / 32;
    const long maxc = g->max_col_nnz > 0 ? g->max_col_nnz : 1;
    for (int p0 = 0; p0 < n_probe; p0 += w.chunk) {
        const int nb = (n_probe - p0) < w.chunk ? (n_probe - p0) : w.chunk;
        const int32_t *probes = probe_nodes + p0;
        // (a pair list: the chunk's pairs by value; a chunk whose probes own none is skipped whole, levels 1 and 2 included)
        const long k0 = pj ? (long)pj->ptr[p0] : 0L, k1 = pj ? (long)pj->ptr[p0 + nb] : 0L;
        if (pj && k0 == k1) continue;
        const long m_bound = (long)nb * maxc, m2_bound = (long)nb * n;
        // level 1 (the narrow chain's), then dS2x = dH1x W2
        int rc = exact_level1(g, b->l1, b->X, b->ldx, b->W1, b->F, b->H1, Hp1, lpr1, probes, nb, words, w.Spd, w.bits1, w.off, delta, w.H1x, st);
        if (rc) return rc;
        if (Hp2 != b->H2) LT_HIP(hipMemsetAsync(w.S2x, 0, (size_t)m_bound * Hp2 * sizeof(float), st));
        rc = lt_launch_gemm_mdev(w.H1x, Hp1, b->W2, b->H2, w.S2x, Hp2, (int)m_bound, w.off + nb, b->H2, b->H1, st);
        if (rc) return rc;
        // level 2: R2 by marking, then every member's place
        LT_HIP(hipMemsetAsync(w.bits2, 0, (size_t)nb * words * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k3_mark2, dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->tptr, g->trow, probes, nb, w.off, words, w.bits2,
                           w.n_items2);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k3w_rank2, dim3((unsigned)nb), dim3(LT_BLOCK), 0, st, words, w.bits2, w.rank2, w.cnt2);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k3w_list2, dim3((unsigned)nb), dim3(LT_BLOCK), 0, st, nb, words, w.rank2, w.cnt2, w.off2, w.items2);
        LT_CHECK_LAUNCH();
        LT_DISPATCH_LPR(lpr2, hipLaunchKernelGGL((k3dw_stageB<LPR_>), dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val,
                                                 b->Z2d, Hp2, w.off, w.S2x, w.bits1, words, w.items2, w.off2 + nb, w.dH2x));
        LT_CHECK_LAUNCH();
        // dS3x = dH2x W3 over the items (the count on the device); W3 as the caller holds it: the product reads K = H2 rows of it
        // and N = C columns, and leaves the pad columns of both operands alone
        rc = lt_launch_gemm_mdev(w.dH2x, Hp2, b->W3, C, w.S3x, Cp, (int)m2_bound, w.off2 + nb, C, b->H2, st);
        if (rc) return rc;
        // level 3: the observed rows
        rc = wide_observed_rows(g, C, Cp, lprc, p0, nb, w.S3x, w.rank2, words, w.off2, pj, w.pair_ptr, k0, k1, observe_nodes, n_obs, delta, out,
                                ldo, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_influence3_rows(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe,
                                  const int32_t *observe_nodes, int32_t n_obs, float delta, float *out, int64_t ldo,
                                  void *workspace, size_t workspace_bytes, void *stream) {
    return lt_influence3_rows_mode(b, probe_nodes, n_probe, observe_nodes, n_obs, delta, LT_MODE_SPARSE, out, ldo, workspace,
                                   workspace_bytes, stream);
}

static int influence3_impl(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe, const int32_t *observe_nodes,
                           int32_t n_obs, float delta, int32_t mode, float *out, int64_t ldo, void *workspace, size_t workspace_bytes,
                           void *stream, const lt_pairs_job *pj);

extern "C" int lt_influence3_rows_mode(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe,
                                       const int32_t *observe_nodes, int32_t n_obs, float delta, int32_t mode, float *out,
                                       int64_t ldo, void *workspace, size_t workspace_bytes, void *stream) {
    return influence3_impl(b, probe_nodes, n_probe, observe_nodes, n_obs, delta, mode, out, ldo, workspace, workspace_bytes, stream,
                           nullptr);
}

// ---- lt_influence3_pairs (include/linkteller_hip.h): the scores of a LIST of (probe, observed) pairs, grouped by probe -----------
extern "C" size_t lt_influence3_pairs_workspace_bytes(const lt_baseline3 *b, int32_t n_probe, int64_t n_pairs) {
    if (!b || n_probe < 0 || n_pairs < 0 || n_pairs > LT_PAIRS_MAX) return 0;
    return carve3(nullptr, b, n_probe, 0, n_pairs).bytes;
}
extern "C" int lt_influence3_pairs(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe, const int64_t *pair_ptr,
                                   const int32_t *pair_obs, int64_t n_pairs, float delta, int32_t mode, float *out,
                                   void *workspace, size_t workspace_bytes, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_influence3_pairs: baseline is NULL");
    { const int rc = lt_pairs_check("lt_influence3_pairs", n_probe, pair_ptr, n_pairs); if (rc) return rc; }
    // (FULL names the quantity SPARSE computes for this model: lt_influence3_rows_mode evaluates both by the same launches)
    const lt_pairs_job pj = {pair_ptr, pair_obs, n_pairs};
    return influence3_impl(b, probe_nodes, n_probe, nullptr, 0, delta, mode, out, 0, workspace, workspace_bytes, stream, &pj);
}

static int influence3_impl(const lt_baseline3 *b, const int32_t *probe_nodes, int32_t n_probe, const int32_t *observe_nodes,
                           int32_t n_obs, float delta, int32_t mode, float *out, int64_t ldo, void *workspace, size_t workspace_bytes,
                           void *stream, const lt_pairs_job *pj) {
    const char *fn = pj ? "lt_influence3_pairs" : "lt_influence3_rows";
    LT_REQUIRE(b != nullptr, "%s: baseline is NULL", fn);
    lt_prof_call prof_call_;
    const bool exact = mode == LT_MODE_DELTA;
    {
        const size_t need = pj ? lt_influence3_pairs_workspace_bytes(b, n_probe, pj->n_pairs) : lt_influence3_workspace_bytes(b, n_probe, n_obs);
        bool go;
        const int rc = probe_front(fn, b->n, mode, [&]() {
            if (b->wide && !exact)
                return lt_set_error(LT_ERR_UNSUPPORTED, "%s: a wide handle (lt_baseline3_create_wide, C=%d) serves LT_MODE_DELTA only; the "
                                    "fp32 finite difference of this shape is the caller's loop over the unfused layers", fn, b->C);
            LT_REQUIRE(!exact || b->Z2d != nullptr, "%s: LT_MODE_DELTA needs lt_baseline3_enable_fp64", fn);
            return (int)LT_OK;
        }, probe_nodes, n_probe, &observe_nodes, n_obs, delta, out, ldo, workspace, workspace_bytes, need, pj, &go);
        if (rc || !go) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const lt_graph *g = b->g;
    const infl3_ws w = carve3(workspace, b, n_probe, n_obs, pj ? pj->n_pairs : (int64_t)-1);
    const int n = b->n, C = b->C, Hp1 = b->Hp1, Hp2 = b->Hp2, cp = lt_cp_for(C);
    const long maxc = g->max_col_nnz > 0 ? g->max_col_nnz : 1;
    {   // (a wide handle's level-2 tables run over up to n rows per probe)
        const int rc = probe_chunk_limits(fn, n_probe, w.chunk, n_obs, pj, b->wide ? lt_lpr_for(b->Cp) : LT_L2_LANES,
                                          b->wide && n > maxc ? (long)n : maxc);
        if (rc) return rc;
    }
    { const int rc = probe_check_nodes(n, &probe_nodes, n_probe, &observe_nodes, n_obs, pj, w.probes_s, w.obs_s, w.pair_ptr, st); if (rc) return rc; }
    const int lpr1 = lt_lpr_for(Hp1), lpr2 = lt_lpr_for(Hp2);
    const int words = (n + 31) / 32;
    {   // the baseline the mode reads: the fp64 pre-activations of the first two layers, or the fp32 forward
        const int rc = exact ? ensure3_fp64(b, st) : ensure3_fp32(b, st);
        if (rc) return rc;
    }
    if (b->wide) return influence3_wide_chunks(b, w, probe_nodes, n_probe, observe_nodes, n_obs, delta, out, ldo, st, pj);
    for (int p0 = 0; p0 < n_probe; p0 += w.chunk) {
        const int nb = (n_probe - p0) < w.chunk ? (n_probe - p0) : w.chunk;
        const int32_t *probes = probe_nodes + p0;
        float *orow = out + (int64_t)p0 * ldo;
        // (a pair list: the chunk's pairs by value; a chunk whose probes own none is skipped whole, levels 1 and 2 included)
        const long k0 = pj ? (long)pj->ptr[p0] : 0L, k1 = pj ? (long)pj->ptr[p0 + nb] : 0L;
        if (pj && k0 == k1) continue;
        const long cells = pj ? k1 - k0 : (long)nb * n_obs;
        const long m_bound = (long)nb * maxc;
        int rc;
        // level 1: H1x rows (sparse: recomputed with row v substituted; delta: the change dH1), then S2x = H1x W2 (M = number of
        // items, only known on the device: the GEMM runs over the chunk's upper bound nb * max column length, the tiles
        // past the count exit -- no read-back, no host synchronisation)
        if (!exact) {
            // perturbed rows: Sp = (X[v] + X[v] d) W1, the slicing of the baseline product          attacker.py:101-105
            if (Hp1 != b->H1) LT_HIP(hipMemsetAsync(w.Sp, 0, (size_t)nb * Hp1 * sizeof(float), st));
            rc = lt_launch_gemm_splitk(b->X, b->ldx, b->W1, b->H1, w.Sp, Hp1, nb, b->H1, b->F, probe_kslice3(b), w.slabs, st,
                                       probes, delta);
            if (rc) return rc;
            hipLaunchKernelGGL(k_item_bits, dim3(nb), dim3(256), 0, st, g->tptr, g->trow, probes, nb, words, w.bits1, w.off, (int2 *)nullptr, (uint2 *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
            LT_CHECK_LAUNCH();
            LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k3_rows_relu<LPR_>), dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, 0, g->rowptr,
                                                     g->col, g->val, b->S1, Hp1, b->b1p, w.H1x, g->tptr, g->trow, probes, nb, w.off,
                                                     w.Sp));
            LT_CHECK_LAUNCH();
        } else {
            rc = exact_level1(g, b->l1, b->X, b->ldx, b->W1, b->F, b->H1, Hp1, lpr1, probes, nb, words, w.Spd, w.bits1, w.off, delta, w.H1x, st);
            if (rc) return rc;
        }
        if (Hp2 != b->H2) LT_HIP(hipMemsetAsync(w.S2x, 0, (size_t)m_bound * Hp2 * sizeof(float), st));
        rc = lt_launch_gemm_mdev(w.H1x, Hp1, b->W2, b->H2, w.S2x, Hp2, (int)m_bound, w.off + nb, b->H2, b->H1, st);
        if (rc) return rc;
        // level 2: R2 and its items
        LT_HIP(hipMemsetAsync(w.bits2, 0, (size_t)nb * words * sizeof(uint32_t), st));
        hipLaunchKernelGGL(k3_mark2, dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->tptr, g->trow, probes, nb, w.off, words, w.bits2,
                           w.n_items2);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k3_list2, dim3((unsigned)nb), dim3(LT_BLOCK), 0, st, words, w.bits2, w.items2, w.n_items2);
        LT_CHECK_LAUNCH();
        const unsigned gridC = (unsigned)((cells * LT_L2_LANES + LT_BLOCK - 1) / LT_BLOCK);
        if (!exact) {
            LT_DISPATCH_LPR(lpr2, LT_DISPATCH_CP(cp,
                hipLaunchKernelGGL((k3_stageB<LPR_, CP_>), dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val, b->S2,
                                   Hp2, b->b2p, b->W3p, C, w.off, w.S2x, w.bits1, words, w.items2, w.n_items2, n, w.S3x)));
            LT_CHECK_LAUNCH();
            // level 3: observed rows
            if (pj) {
                LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k3_stageC_pairs<CP_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col,
                                                      g->val, b->S3, C, b->b3, b->OUT, nb, n, w.S3x, w.bits2, words, w.pair_ptr + p0,
                                                      k0, k1, observe_nodes, delta, out));
            } else {
                LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k3_stageC<CP_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val,
                                                      b->S3, C, b->b3, b->OUT, nb, n, w.S3x, w.bits2, words, observe_nodes, n_obs,
                                                      delta, orow, (long)ldo));
            }
        } else {
            LT_DISPATCH_LPR(lpr2, LT_DISPATCH_CP(cp,
                hipLaunchKernelGGL((k3d_stageB<LPR_, CP_>), dim3(LT3_GRID), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val, b->Z2d,
                                   Hp2, b->W3p, C, w.off, w.S2x, w.bits1, words, w.items2, w.n_items2, n, w.S3x)));
            LT_CHECK_LAUNCH();
            if (pj) {
                LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k3d_stageC_pairs<CP_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col,
                                                      g->val, C, nb, n, w.S3x, w.bits2, words, w.pair_ptr + p0, k0, k1, observe_nodes,
                                                      delta, out));
            } else {
                LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k3d_stageC<CP_>), dim3(gridC), dim3(LT_BLOCK), 0, st, g->rowptr, g->col, g->val,
                                                      C, nb, n, w.S3x, w.bits2, words, observe_nodes, n_obs, delta, orow, (long)ldo));
            }
        }
        LT_CHECK_LAUNCH();
    }
    return LT_OK;
}

// ---- the 2-layer model with a wide class layer (lt_baseline2w: H <= 256, 1 <= C <= 256; LT_MODE_DELTA alone) --------------------------
//   logits = A (relu(A (X W1) + b1) W2) + b2
// For two layers the class width enters only behind the single kink test, so the chain is the wide chain above with one level removed:
// the probes' fp64 product rows, the level-1 bitmap with positions (k_item_bits: bits1, off), dH1x on the fp64 pre-activation
// (k3d_items1), dS2x = dH1x W2 as one MFMA product over the items (count on the device, rows of stride Cp) -- and the observed rows are
// k3dw_stageC / k3dw_stageC_pairs themselves, handed the level-1 tables where the 3-layer chain hands them the level-2 ones: a probe's
// item (b, r) sits at off[b] + bits_pos(bits1 row of b, r), which is all k3dw_cellC asks of (rank2, off2, dS3x).  No level-2 table, so
// the per-probe tables are sized by the longest column, not by n: chunks are large.
// The handle owns an inner 2-layer baseline over (X, W1, b1) for the fp64 pre-activation Z1d and the probes' product rows (what
// lt_baseline3_enable_fp64 builds: C = 1, no_agg), from creation; the fp32 forward exists only for lt_baseline2w_logits and is
// allocated by its first call.
struct lt_baseline2w {
    const lt_graph *g = nullptr;
    int32_t n = 0, F = 0, H = 0, C = 0, Hp = 0, Cp = 0;
    const float *X = nullptr;
    int64_t ldx = 0;
    const float *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;
    lt_baseline *l1 = nullptr;      // owned: Z1d, the product rows
    // owned, lt_baseline2w_logits only
    float *S1 = nullptr;    // [n, Hp]  X W1
    float *Act1 = nullptr;  // [n, Hp]  relu(A S1 + b1)
    float *S2 = nullptr;    // [n, Cp]  H1 W2
    float *OUT = nullptr;   // [n, Cp]  A S2 + b2
    float *b1p = nullptr, *b2p = nullptr;   // zero-padded to Hp / Cp
    bool fp32_fresh = false;
};

static void free_baseline2w(lt_baseline2w *b) {
    if (!b) return;
    (void)hipFree(b->S1); (void)hipFree(b->Act1); (void)hipFree(b->S2); (void)hipFree(b->OUT); (void)hipFree(b->b1p); (void)hipFree(b->b2p);
    if (b->l1) (void)lt_baseline_destroy(b->l1);
    delete b;
}

extern "C" int lt_baseline2w_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const float *W1, const float *b1,
                                    int32_t H, const float *W2, const float *b2, int32_t C, void *stream, lt_baseline2w **out) {
    LT_REQUIRE(out != nullptr, "lt_baseline2w_create: out is NULL");
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "lt_baseline2w_create: graph is NULL");
    LT_REQUIRE(F > 0 && H > 0 && C > 0, "lt_baseline2w_create: F=%d H=%d C=%d must be positive", F, H, C);
    if (H > LT_MAX_H || C > LT3_WIDE_MAX_C)
        return lt_set_error(LT_ERR_UNSUPPORTED, "lt_baseline2w_create: H=%d C=%d (supported: H <= %d, C <= %d)", H, C, LT_MAX_H,
                            LT3_WIDE_MAX_C);
    LT_REQUIRE(X && W1 && b1 && W2 && b2, "lt_baseline2w_create: NULL tensor pointer");
    LT_REQUIRE(ldx >= F, "lt_baseline2w_create: ldx=%lld < F=%d", (long long)ldx, F);
    (void)lt_node_err_dev();      // (allocated outside any stream capture)
    lt_baseline2w *b = new (std::nothrow) lt_baseline2w();
    if (!b) return lt_set_error(LT_ERR_NOMEM, "lt_baseline2w_create: out of host memory");
    b->g = g; b->n = g->n; b->F = F; b->H = H; b->C = C;
    b->Hp = lt_round_up(H, 4); b->Cp = lt_round_up(C, 4);
    b->X = X; b->ldx = ldx; b->W1 = W1; b->b1 = b1; b->W2 = W2; b->b2 = b2;
    // (W2 / b2 of the inner handle are never used for arithmetic: only its fp64 pre-activation and product rows are read; C = 1
    // keeps its padding kernel inside W2's first H floats)
    int rc = lt_baseline_create(g, X, ldx, F, W1, b1, H, W2, b2, 1, stream, &b->l1);
    if (rc == LT_OK) {
        b->l1->no_agg = true;
        rc = lt_baseline_enable_fp64(b->l1, stream);
    }
    if (rc) {
        free_baseline2w(b);
        return rc;
    }
    *out = b;
    return LT_OK;
}

extern "C" int lt_baseline2w_refresh(lt_baseline2w *b, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_baseline2w_refresh: baseline is NULL");
    b->fp32_fresh = false;
    return lt_baseline_refresh(b->l1, stream);
}

extern "C" int lt_baseline2w_features_changed(lt_baseline2w *b, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_baseline2w_features_changed: baseline is NULL");
    b->fp32_fresh = false;
    return lt_baseline_features_changed(b->l1, stream);
}

extern "C" int lt_baseline2w_destroy(lt_baseline2w *b) {
    free_baseline2w(b);
    return LT_OK;
}

// the unperturbed fp32 forward on the unfused layers (the product, the SpMM's row kernels), rows of stride Hp / Cp
static int ensure2w_fp32(const lt_baseline2w *cb, hipStream_t st) {
    lt_baseline2w *b = const_cast<lt_baseline2w *>(cb);   // cache state only
    if (b->fp32_fresh || b->n == 0) return LT_OK;
    const size_t n = (size_t)b->n;
    // (each buffer once: a call that failed half-way leaves what it got to the next call and to destroy)
    if (!b->S1) LT_HIP(hipMalloc((void **)&b->S1, n * b->Hp * sizeof(float)));
    if (!b->Act1) LT_HIP(hipMalloc((void **)&b->Act1, n * b->Hp * sizeof(float)));
    if (!b->S2) LT_HIP(hipMalloc((void **)&b->S2, n * b->Cp * sizeof(float)));
    if (!b->OUT) LT_HIP(hipMalloc((void **)&b->OUT, n * b->Cp * sizeof(float)));
    if (!b->b1p) LT_HIP(hipMalloc((void **)&b->b1p, (size_t)b->Hp * sizeof(float)));
    if (!b->b2p) LT_HIP(hipMalloc((void **)&b->b2p, (size_t)b->Cp * sizeof(float)));
    hipLaunchKernelGGL(k3w_pad_b3, dim3((b->Hp + 255) / 256), dim3(256), 0, st, b->b1, b->H, b->Hp, b->b1p);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k3w_pad_b3, dim3((b->Cp + 255) / 256), dim3(256), 0, st, b->b2, b->C, b->Cp, b->b2p);
    LT_CHECK_LAUNCH();
    if (b->Hp != b->H) LT_HIP(hipMemsetAsync(b->S1, 0, n * b->Hp * sizeof(float), st));
    int rc = lt_launch_gemm(b->X, b->ldx, b->W1, b->H, b->S1, b->Hp, b->n, b->H, b->F, st);
    if (rc) return rc;
    rc = lt_spmm_csr_f32(b->g, b->S1, b->Hp, b->Hp, b->b1p, 1, b->Act1, b->Hp, st);
    if (rc) return rc;
    rc = lt_launch_gemm(b->Act1, b->Hp, b->W2, b->C, b->S2, b->Cp, b->n, b->C, b->H, st);
    if (rc) return rc;
    rc = lt_spmm_csr_f32(b->g, b->S2, b->Cp, b->C, b->b2p, 0, b->OUT, b->Cp, st);
    if (rc) return rc;
    b->fp32_fresh = true;
    return LT_OK;
}

extern "C" int lt_baseline2w_logits(const lt_baseline2w *b, float *dst, void *stream) {
    LT_REQUIRE(b != nullptr && dst != nullptr, "lt_baseline2w_logits: NULL argument");
    if (b->n == 0) return LT_OK;
    { const int rc = ensure2w_fp32(b, (hipStream_t)stream); if (rc) return rc; }
    LT_HIP(hipMemcpy2DAsync(dst, (size_t)b->C * sizeof(float), b->OUT, (size_t)b->Cp * sizeof(float), (size_t)b->C * sizeof(float),
                            (size_t)b->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

struct infl2w_ws {
    double *Spd;            // fp64 product rows of the chunk's probes [chunk, Hp]
    int32_t *off;           // [chunk + 1] the probes' item offsets; off[nb] = the chunk's item count (stays on the device)
    uint2 *bits1;           // [chunk, words] the level-1 bitmap with positions
    float *dH1x, *dS2x;     // [chunk * maxc, Hp] / [chunk * maxc, Cp]
    int32_t *probes_s, *obs_s;
    int64_t *pair_ptr;      // lt_influence2w_pairs: the device copy of the offsets (obs_s is then [n_pairs])
    size_t bytes;
    int chunk;
};

// n_pairs >= 0: the carve of lt_influence2w_pairs (n_obs = 0); the chunk and every per-chunk table are those of the rows call
static infl2w_ws carve2w(void *base, const lt_baseline2w *b, int n_probe, int n_obs, int64_t n_pairs = -1) {
    infl2w_ws w = {};
    const size_t Hp = (size_t)b->Hp, Cp = (size_t)b->Cp;
    const size_t maxc = (size_t)(b->g->max_col_nnz > 0 ? b->g->max_col_nnz : 1);
    const size_t words = ((size_t)b->n + 31) / 32;
    const size_t per_probe = Hp * sizeof(double) + maxc * (Hp + Cp) * sizeof(float) + words * sizeof(uint2) + sizeof(int32_t);
    size_t chunk = (size_t)lt_tune().chunk_budget / per_probe;
    if (chunk > 65534) chunk = 65534;
    if (chunk > (size_t)2147483646 / maxc) chunk = (size_t)2147483646 / maxc;      // (the items' upper bound chunk * maxc stays an int)
    if (chunk > (size_t)(n_probe > 0 ? n_probe : 1)) chunk = (size_t)(n_probe > 0 ? n_probe : 1);
    if (chunk < 1) chunk = 1;
    w.chunk = (int)chunk;
    size_t offb = 0;
    char *p = (char *)base;
    auto take = [&](size_t bytes) {
        void *q = p ? (void *)(p + offb) : nullptr;
        offb += lt_align_up(bytes ? bytes : 1, 256);
        return q;
    };
    w.Spd = (double *)take(chunk * Hp * sizeof(double));
    w.off = (int32_t *)take((chunk + 1) * sizeof(int32_t));
    w.bits1 = (uint2 *)take(chunk * words * sizeof(uint2));
    w.dH1x = (float *)take(chunk * maxc * Hp * sizeof(float));
    w.dS2x = (float *)take(chunk * maxc * Cp * sizeof(float));
    w.probes_s = (int32_t *)take((size_t)(n_probe > 0 ? n_probe : 1) * sizeof(int32_t));
    w.obs_s = (int32_t *)take((n_pairs >= 0 ? (size_t)n_pairs : (size_t)(n_obs > 0 ? n_obs : 1)) * sizeof(int32_t));
    if (n_pairs >= 0) w.pair_ptr = (int64_t *)take(((size_t)n_probe + 1) * sizeof(int64_t));
    w.bytes = offb;
    return w;
}

extern "C" size_t lt_influence2w_workspace_bytes(const lt_baseline2w *b, int32_t n_probe, int32_t n_obs) {
    if (!b || n_probe < 0 || n_obs < 0) return 0;
    return carve2w(nullptr, b, n_probe, n_obs).bytes;
}
extern "C" size_t lt_influence2w_pairs_workspace_bytes(const lt_baseline2w *b, int32_t n_probe, int64_t n_pairs) {
    if (!b || n_probe < 0 || n_pairs < 0 || n_pairs > LT_PAIRS_MAX) return 0;
    return carve2w(nullptr, b, n_probe, 0, n_pairs).bytes;
}

// rows (pj == NULL) and pairs: everything but the last launch of a chunk is the same
static int influence2w_impl(const lt_baseline2w *b, const int32_t *probe_nodes, int32_t n_probe, const int32_t *observe_nodes, int32_t n_obs,
                            float delta, int32_t mode, float *out, int64_t ldo, void *workspace, size_t workspace_bytes, void *stream,
                            const lt_pairs_job *pj) {
    const char *fn = pj ? "lt_influence2w_pairs" : "lt_influence2w_rows";
    lt_prof_call prof_call_;
    {
        const size_t need = pj ? lt_influence2w_pairs_workspace_bytes(b, n_probe, pj->n_pairs) : lt_influence2w_workspace_bytes(b, n_probe, n_obs);
        bool go;
        const int rc = probe_front(fn, b->n, mode, [&]() {
            if (mode != LT_MODE_DELTA)
                return lt_set_error(LT_ERR_UNSUPPORTED, "%s: a lt_baseline2w handle (C=%d) serves LT_MODE_DELTA only; the fp32 finite "
                                    "difference of this shape is lt_influence_rows_vec + lt_wide_combine over class slices", fn, b->C);
            return (int)LT_OK;
        }, probe_nodes, n_probe, &observe_nodes, n_obs, delta, out, ldo, workspace, workspace_bytes, need, pj, &go);
        if (rc || !go) return rc;
    }
    hipStream_t st = (hipStream_t)stream;
    const lt_graph *g = b->g;
    const infl2w_ws w = carve2w(workspace, b, n_probe, n_obs, pj ? pj->n_pairs : (int64_t)-1);
    const int n = b->n, C = b->C, Cp = b->Cp, Hp = b->Hp;
    const int lpr1 = lt_lpr_for(Hp), lprc = lt_lpr_for(Cp);
    const int words = (n + 31) / 32;
    const long maxc = g->max_col_nnz > 0 ? g->max_col_nnz : 1;
    { const int rc = probe_chunk_limits(fn, n_probe, w.chunk, n_obs, pj, lprc, 0); if (rc) return rc; }
    { const int rc = probe_check_nodes(n, &probe_nodes, n_probe, &observe_nodes, n_obs, pj, w.probes_s, w.obs_s, w.pair_ptr, st); if (rc) return rc; }
    { const int rc = lt_fp64_form_all(b->l1, st); if (rc) return rc; }      // Z1d, every row (nothing when it is current)
    for (int p0 = 0; p0 < n_probe; p0 += w.chunk) {
        const int nb = (n_probe - p0) < w.chunk ? (n_probe - p0) : w.chunk;
        const int32_t *probes = probe_nodes + p0;
        // (a pair list: the chunk's pairs by value; a chunk whose probes own none launches nothing)
        const long k0 = pj ? (long)pj->ptr[p0] : 0L, k1 = pj ? (long)pj->ptr[p0 + nb] : 0L;
        if (pj && k0 == k1) continue;
        const long m_bound = (long)nb * maxc;       // (< 2^31: carve2w)
        int rc = exact_level1(g, b->l1, b->X, b->ldx, b->W1, b->F, b->H, Hp, lpr1, probes, nb, words, w.Spd, w.bits1, w.off, delta, w.dH1x, st);
        if (rc) return rc;
        // dS2x = dH1x W2 over the items; W2 as the caller holds it (K = H rows, N = C columns: the pad columns of both operands
        // are left alone)
        rc = lt_launch_gemm_mdev(w.dH1x, Hp, b->W2, C, w.dS2x, Cp, (int)m_bound, w.off + nb, C, b->H, st);
        if (rc) return rc;
        // the observed rows: the wide chain's cell over the level-1 tables
        rc = wide_observed_rows(g, C, Cp, lprc, p0, nb, w.dS2x, w.bits1, words, w.off, pj, w.pair_ptr, k0, k1, observe_nodes, n_obs, delta, out,
                                ldo, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_influence2w_rows(const lt_baseline2w *b, const int32_t *probe_nodes, int32_t n_probe, const int32_t *observe_nodes,
                                   int32_t n_obs, float delta, int32_t mode, float *out, int64_t ldo, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_influence2w_rows: baseline is NULL");
    return influence2w_impl(b, probe_nodes, n_probe, observe_nodes, n_obs, delta, mode, out, ldo, workspace, workspace_bytes, stream,
                            nullptr);
}

extern "C" int lt_influence2w_pairs(const lt_baseline2w *b, const int32_t *probe_nodes, int32_t n_probe, const int64_t *pair_ptr,
                                    const int32_t *pair_obs, int64_t n_pairs, float delta, int32_t mode, float *out, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    LT_REQUIRE(b != nullptr, "lt_influence2w_pairs: baseline is NULL");
    { const int rc = lt_pairs_check("lt_influence2w_pairs", n_probe, pair_ptr, n_pairs); if (rc) return rc; }
    const lt_pairs_job pj = {pair_ptr, pair_obs, n_pairs};
    return influence2w_impl(b, probe_nodes, n_probe, nullptr, 0, delta, mode, out, 0, workspace, workspace_bytes, stream, &pj);
}
