// Training of the 2-layer GCN: one epoch of GCNTrainer.train_one_epoch on a transfer dataset (reference gcn_trainer.py:144-170,
// gcn/models.py:19-24, F.cross_entropy, torch.optim.Adam), as stream-ordered launches with no host synchronisation.
//
//   S1 = X W1                   lt_launch_gemm(_splitk)        the forward's product, same slicing: same bits
//   Z1 = A S1 + b1              lt_launch_layer1 (Z1 stored)   the forward's chains
//   H1d = dropout(relu(Z1)),    k_tr_dropout                   Philox4x32-10 mask; S2 with relu_w2_partial's order
//   S2 = H1d W2
//   Z2 = A S2 + b2              lt_launch_layer2               the forward's layer 2: with p = 0, Z2 IS gcn2_forward's output
//   loss, dZ2, correct          k_tr_ce, k_tr_ce_reduce        per-row CE head, then one block: mean loss, count, db2
//   dS2 = A^T dZ2               k_tr_spmm_t_narrow             CSC rows (A is not symmetric in general)
//   dZ1, db1 / dW2 partials     k_tr_bwd_rows                  dZ1 = [H1d > 0] (dS2 W2^T) / (1 - p); fixed-order row blocks
//   db1, dW2                    k_tr_colsum                    the blocks' partials in block order
//   dS1 = A^T dZ1               k_tr_spmm_t_wide               row_dot chains over the CSC
//   dW1 = X^T dS1               k_gemm_tn_mfma + k_sum_slabs   v_mfma_f32_32x32x2_f32, A^T staged through LDS, split-K
//   Adam                        k_tr_adam                      one launch over W1 | b1 | W2 | b2
//
// Every reduction has a fixed order (no float atomics): two trainings with the same inputs give the same bits.
// Built with -ffp-contract=off: the only fused operations are explicit fmaf calls and the MFMAs.
#include <math.h>

#include <new>

#include "lt_rows.hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

#define TR_BLOCK 256
#define TR_ROWS_PER_BLOCK 32   // k_tr_bwd_rows: rows summed by one block (its partial is one slab of the column sums)

// --------------------------------------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): counter (c0, c1, c2, c3), key (k0, k1)
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint4 lt_philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k.x += 0x9E3779B9u; k.y += 0xBB67AE85u; }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    }
    return c;
}

// word (i & 3) of Philox(counter (q lo, q hi, epoch, 0), key (seed lo, seed hi)), q = i >> 2
__device__ __forceinline__ uint4 lt_drop_block(uint64_t q, uint32_t epoch, uint64_t seed) {
    return lt_philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), epoch, 0u),
                            make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

struct lt_drop_args {
    int on;              // 0: p == 0, no RNG call
    uint64_t thresh;     // keep iff u >= thresh = floor(p * 2^32)  (2^32 for p == 1: nothing is kept)
    float scale;         // 1 / (1 - p), rounded once from double
    uint32_t epoch;
    uint64_t seed;
};

// --------------------------------------------------------------------------------------------
// H1d = dropout(relu(Z1)) and S2 = H1d W2 (lane layout and summation order of k_layer1: with p = 0 these are its S2 bits)
// --------------------------------------------------------------------------------------------
template <int LPR, int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_dropout(int n, const float *__restrict__ Z1, int Hp, int H,
                                                         const float *__restrict__ W2p, int C, lt_drop_args d,
                                                         float *__restrict__ H1d, float *__restrict__ S2) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * TR_BLOCK + threadIdx.x) >> 6;
    const int gl = lane & (LPR - 1);
    int r = wave * RPW + lane / LPR;
    if (LPR == 64) r = __builtin_amdgcn_readfirstlane(r);
    if (r >= n) return;
    const int coff = 4 * gl;
    const bool active = coff < Hp;
    float part[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) part[c] = 0.f;
    if (active) {
        const f32x4 z = ld4(Z1 + (size_t)r * Hp + coff);
        f32x4 h = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
        if (d.on) {
            const uint64_t i0 = (uint64_t)r * H + coff;
            uint32_t u[4];
            if ((H & 3) == 0) {    // the 4 columns are the 4 words of one Philox block
                const uint4 w = lt_drop_block(i0 >> 2, d.epoch, d.seed);
                u[0] = w.x; u[1] = w.y; u[2] = w.z; u[3] = w.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint64_t i = i0 + j;
                    const uint4 w = lt_drop_block(i >> 2, d.epoch, d.seed);
                    const uint32_t sel = (uint32_t)(i & 3);
                    u[j] = sel == 0 ? w.x : sel == 1 ? w.y : sel == 2 ? w.z : w.w;
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool keep = coff + j < H && (uint64_t)u[j] >= d.thresh;
                h[j] = keep ? h[j] * d.scale : 0.f;
            }
        }
        *reinterpret_cast<f32x4 *>(H1d + (size_t)r * Hp + coff) = h;
        relu_w2_partial<CP>(h, W2p + (size_t)coff * C, C, part);   // h >= 0: the relu is the identity
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) part[c] = group_sum<LPR>(part[c]);
    if (gl == 0) {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) S2[(size_t)r * C + c] = part[c];
    }
}

// --------------------------------------------------------------------------------------------
// softmax cross-entropy head, one thread per row: loss_r = logsumexp(z) - z[y], dZ2 = (softmax(z) - onehot(y)) / n,
// correct = (first argmax == y)
// --------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_ce(int n, const float *__restrict__ Z2, int C,
                                                    const int32_t *__restrict__ labels, float inv_n,
                                                    float *__restrict__ loss_r, int32_t *__restrict__ corr_r,
                                                    float *__restrict__ dZ2) {
    const int r = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (r >= n) return;
    const int y = labels[r];
    float z[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) z[c] = c < C ? Z2[(size_t)r * C + c] : -INFINITY;
    float mx = z[0];
    int arg = 0;
#pragma unroll
    for (int c = 1; c < CP; ++c)
        if (c < C && z[c] > mx) { mx = z[c]; arg = c; }
    float e[CP], s = 0.f, zy = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        e[c] = c < C ? expf(z[c] - mx) : 0.f;
        s += e[c];
        if (c == y) zy = z[c];
    }
    loss_r[r] = (mx + logf(s)) - zy;
    corr_r[r] = arg == y ? 1 : 0;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) dZ2[(size_t)r * C + c] = (e[c] / s - (c == y ? 1.f : 0.f)) * inv_n;
}

// One block: mean loss and correct count into the epoch's record, db2 = sum_r dZ2 -- thread t sums rows t, t + 256, ...
// in row order, then a fixed tree over the threads.
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_ce_reduce(int n, int C, const float *__restrict__ loss_r,
                                                           const int32_t *__restrict__ corr_r,
                                                           const float *__restrict__ dZ2, float *__restrict__ record,
                                                           float *__restrict__ db2) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int sc[TR_BLOCK];
    __shared__ float sd[CP][TR_BLOCK];
    const int t = threadIdx.x;
    float l = 0.f, d[CP];
    int k = 0;
#pragma unroll
    for (int c = 0; c < CP; ++c) d[c] = 0.f;
    for (int r = t; r < n; r += TR_BLOCK) {
        l += loss_r[r];
        k += corr_r[r];
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) d[c] += dZ2[(size_t)r * C + c];
    }
    sl[t] = l;
    sc[t] = k;
#pragma unroll
    for (int c = 0; c < CP; ++c) sd[c][t] = d[c];
    __syncthreads();
    for (int w = TR_BLOCK / 2; w >= 1; w >>= 1) {
        if (t < w) {
            sl[t] += sl[t + w];
            sc[t] += sc[t + w];
#pragma unroll
            for (int c = 0; c < CP; ++c) sd[c][t] += sd[c][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        record[0] = sl[0] / (float)n;
        record[1] = (float)sc[0];
    }
    if (t < C) db2[t] = sd[t < CP ? t : 0][0];
}

// --------------------------------------------------------------------------------------------
// A^T products over the CSC (tptr / trow / tval = CSR of A^T)
// --------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_spmm_t_narrow(int n, const int32_t *__restrict__ tptr,
                                                               const int32_t *__restrict__ trow,
                                                               const float *__restrict__ tval,
                                                               const float *__restrict__ D, int C,
                                                               float *__restrict__ OUT) {
    const int gid = (blockIdx.x * TR_BLOCK + threadIdx.x) / LT_L2_LANES;
    const int q = threadIdx.x & (LT_L2_LANES - 1);
    if (gid >= n) return;
    float acc[CP];
    row2_dot<CP>(trow, tval, tptr[gid], tptr[gid + 1], q, C, [&](int c, int) { return D + (size_t)c * C; }, acc);
    if (q == 0) {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) OUT[(size_t)gid * C + c] = acc[c];
    }
}

template <int LPR>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_spmm_t_wide(int n, const int32_t *__restrict__ tptr,
                                                             const int32_t *__restrict__ trow,
                                                             const float *__restrict__ tval,
                                                             const float *__restrict__ D, int Hp,
                                                             float *__restrict__ OUT) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * TR_BLOCK + threadIdx.x) >> 6;
    const int gl = lane & (LPR - 1);
    int r = wave * RPW + lane / LPR;
    if (LPR == 64) r = __builtin_amdgcn_readfirstlane(r);
    if (r >= n) return;
    const int coff = 4 * gl;
    const bool active = coff < Hp;
    const f32x4 z = row_dot<8>(trow, tval, tptr[r], tptr[r + 1], D, Hp, coff, active, -1, nullptr);
    if (active) *reinterpret_cast<f32x4 *>(OUT + (size_t)r * Hp + coff) = z;
}

// --------------------------------------------------------------------------------------------
// dZ1 = [H1d > 0] (dS2 W2^T) * scale, written; and per block of TR_ROWS_PER_BLOCK rows the partial sums of db1 = sum_r dZ1
// and dW2 = H1d^T dS2 into slab blockIdx.x ([H | H * C] floats).  Thread (s, h): column h, rows s, s + G, ... of the
// block's rows (G = 256 / W sub-rows, W = pow2 >= Hp); the sub-rows' sums are then added in sub-row order.
// --------------------------------------------------------------------------------------------
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_bwd_rows(int n, int H, int Hp, int W, int C,
                                                          const float *__restrict__ H1d, const float *__restrict__ dS2,
                                                          const float *__restrict__ W2p, float scale,
                                                          float *__restrict__ dZ1, float *__restrict__ part) {
    __shared__ float red[TR_BLOCK][CP + 1];
    const int t = threadIdx.x;
    const int h = t & (W - 1), s = t / W, G = TR_BLOCK / W;
    const int r0 = blockIdx.x * TR_ROWS_PER_BLOCK, r1 = min(n, r0 + TR_ROWS_PER_BLOCK);
    float w2[CP], dw[CP], db = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        w2[c] = (h < Hp && c < C) ? W2p[(size_t)h * C + c] : 0.f;
        dw[c] = 0.f;
    }
    if (h < Hp) {
        for (int r = r0 + s; r < r1; r += G) {
            const float a = H1d[(size_t)r * Hp + h];
            float ds[CP];
#pragma unroll
            for (int c = 0; c < CP; ++c) ds[c] = c < C ? dS2[(size_t)r * C + c] : 0.f;
            float gsum = ds[0] * w2[0];
#pragma unroll
            for (int c = 1; c < CP; ++c)
                if (c < C) gsum = fmaf(ds[c], w2[c], gsum);
            const float dz = a > 0.f ? gsum * scale : 0.f;
            dZ1[(size_t)r * Hp + h] = dz;
            db += dz;
#pragma unroll
            for (int c = 0; c < CP; ++c) dw[c] = fmaf(a, ds[c], dw[c]);
        }
    }
    red[t][0] = db;
#pragma unroll
    for (int c = 0; c < CP; ++c) red[t][c + 1] = dw[c];
    __syncthreads();
    if (s == 0 && h < H) {
        for (int k = 1; k < G; ++k) {
            db += red[k * W + h][0];
#pragma unroll
            for (int c = 0; c < CP; ++c) dw[c] += red[k * W + h][c + 1];
        }
        float *p = part + (size_t)blockIdx.x * ((size_t)H + (size_t)H * C);
        p[h] = db;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) p[H + (size_t)h * C + c] = dw[c];
    }
}

// out[o] = sum over the slabs of part[slab * L + o], in slab order: lane group k (of 4) sums slabs k, k + 4, ..., the four
// sums are added in group order.  64 outputs per block.
__global__ __launch_bounds__(TR_BLOCK) void k_tr_colsum(const float *__restrict__ part, int slabs, int L,
                                                        float *__restrict__ out) {
    __shared__ float red[4][64];
    const int o = blockIdx.x * 64 + (threadIdx.x & 63), k = threadIdx.x >> 6;
    float acc = 0.f;
    if (o < L) {
        int z = k;
        for (; z + 12 < slabs; z += 16) {
            const float a0 = part[(size_t)z * L + o], a1 = part[(size_t)(z + 4) * L + o];
            const float a2 = part[(size_t)(z + 8) * L + o], a3 = part[(size_t)(z + 12) * L + o];
            acc += a0; acc += a1; acc += a2; acc += a3;
        }
        for (; z < slabs; z += 4) acc += part[(size_t)z * L + o];
    }
    red[k][threadIdx.x & 63] = acc;
    __syncthreads();
    if (k == 0 && o < L) out[o] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// --------------------------------------------------------------------------------------------
// C[M, N] = A^T B with A [K, M] (row-major, lda), B [K, N] (ldb): the backward's dW1 = X^T dS1 (M = F, N = H, K = n).
// The block / wave / fold structure of k_gemm_f32_mfma (lt_gemm.hip): 64 x 64 block tile, four waves of one 32 x 32
// v_mfma_f32_32x32x2_f32 tile, 16-deep k-tiles through LDS with a register prefetch; only the A tile is loaded as
// k-rows of 64 consecutive m and transposed on its way into LDS (rows padded to 17 floats, so both the transposing
// stores and the MFMA operand reads hit distinct banks).  blockIdx.z owns K slice z and writes slab z.
// --------------------------------------------------------------------------------------------
#define TN_BM 64
#define TN_BN 64
#define TN_BK 16
#define TN_LDA (TN_BK + 1)
#define TN_FOLD 128
__global__ __launch_bounds__(256) void k_gemm_tn_mfma(const float *__restrict__ A, long lda,
                                                      const float *__restrict__ B, long ldb, float *__restrict__ C,
                                                      long ldc, int M, int N, int K, int kslice, long slab_stride) {
    __shared__ __attribute__((aligned(16))) float As[2][TN_BM * TN_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][TN_BK * TN_BN];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int m0 = blockIdx.x * TN_BM;
    const int n0 = blockIdx.y * TN_BN;
    const int a_k = tid >> 4, a_m = (tid & 15) * 4;   // A^T tile: k-row a_k, m columns a_m .. a_m + 3
    const int b_row = tid >> 4, b_col = (tid & 15) * 4;
    const bool a_full = (m0 + a_m + 3) < M;
    const bool b_full = (n0 + b_col + 3) < N;
    const float *a_ptr = A + (long)a_k * lda + m0 + a_m;
    const float *b_ptr = B + (long)b_row * ldb + n0 + b_col;
    const int kb = blockIdx.z * kslice;
    const int ke = min(K, kb + kslice);
    C += (long)blockIdx.z * slab_stride;

    f32x4 ra, rb;
    auto load_tiles = [&](int k0) {
        ra = f32x4{0.f, 0.f, 0.f, 0.f};
        rb = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k0 + a_k < ke) {
            const float *p = a_ptr + (long)k0 * lda;
            if (a_full) {
                ra = *reinterpret_cast<const f32x4u *>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (m0 + a_m + j < M) ra[j] = p[j];
            }
        }
        if (k0 + b_row < ke) {
            const float *p = b_ptr + (long)k0 * ldb;
            if (b_full) {
                rb = *reinterpret_cast<const f32x4u *>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (n0 + b_col + j < N) rb[j] = p[j];
            }
        }
    };
    auto store_tiles = [&](int buf) {
        float *as = &As[buf][a_m * TN_LDA + a_k];
        as[0] = ra.x; as[TN_LDA] = ra.y; as[2 * TN_LDA] = ra.z; as[3 * TN_LDA] = ra.w;
        *reinterpret_cast<f32x4 *>(&Bs[buf][b_row * TN_BN + b_col]) = rb;
    };

    f32x16 acc, total;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; total[i] = 0.f; }
    const int nk = (ke - kb + TN_BK - 1) / TN_BK;
    if (nk > 0) {
        load_tiles(kb);
        store_tiles(0);
    }
    __syncthreads();
    const int a_frag = (wr * 32 + (lane & 31)) * TN_LDA + (lane >> 5);
    const int b_frag = (lane >> 5) * TN_BN + wc * 32 + (lane & 31);
    constexpr int FOLD_TILES = TN_FOLD / TN_BK;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles(kb + (kt + 1) * TN_BK);
        const float *as = &As[buf][a_frag];
        const float *bs = &Bs[buf][b_frag];
#pragma unroll
        for (int kk = 0; kk < TN_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk], bs[kk * TN_BN], acc, 0, 0, 0);
        if ((kt + 1) % FOLD_TILES == 0) {
            total += acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        }
        if (kt + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }
    total += acc;
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int cn = n0 + wc * 32 + (lane & 31);
    if (cn < N) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int cm = m0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (cm < M) C[(long)cm * ldc + cn] = total[reg];
        }
    }
}

// --------------------------------------------------------------------------------------------
// Adam (torch/optim/adam.py _single_tensor_adam, weight decay added to the gradient), op by op in fp32 with the rounding of
// torch's CPU kernels: the weight-decay add, lerp_ and addcmul_ are fused multiply-adds there (vec::fmadd), so they are
// explicit fmaf calls here; sqrt and division are correctly rounded.  The Python scalars arrive as torch converts them
// (formed in double on the host, rounded once to float):
//   g = fma(p, wd, g);  m = fma(w1, g - m, m)  (lerp_, weight w1 = 1 - beta1 < 0.5);  v = v * beta2;  v = fma(w2 * g, g, v)
//   denom = sqrt(v) / bc2_sqrt + eps;  p = p + (neg_step * m) / denom
// --------------------------------------------------------------------------------------------
struct lt_adam_scalars {
    float wd, w1, beta2, w2, bc2_sqrt, eps, neg_step;
    int decay;
};

static lt_adam_scalars adam_scalars(int64_t step, double lr, double beta1, double beta2, double eps, double wd) {
    lt_adam_scalars s;
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    s.wd = (float)wd;
    s.decay = wd != 0.0;
    s.w1 = (float)(1.0 - beta1);
    s.beta2 = (float)beta2;
    s.w2 = (float)(1.0 - beta2);
    s.bc2_sqrt = (float)pow(bc2, 0.5);   // Python's bc2 ** 0.5 is pow(), which may differ from sqrt() in the last bit
    s.eps = (float)eps;
    s.neg_step = (float)(-(lr / bc1));
    return s;
}

__device__ __forceinline__ float adam_elem(float p, float g, float &m, float &v, const lt_adam_scalars &s) {
    if (s.decay) g = fmaf(p, s.wd, g);
    const float d = __fsub_rn(g, m);
    m = s.w1 < 0.5f ? fmaf(s.w1, d, m) : fmaf(__fsub_rn(s.w1, 1.f), d, g);
    v = __fmul_rn(v, s.beta2);
    v = fmaf(__fmul_rn(s.w2, g), g, v);
    // sqrtf and '/' are correctly rounded in fp32 (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt); the header's
    // __fsqrt_rn is the native approximation unless OCML_BASIC_ROUNDED_OPERATIONS is defined
    const float denom = __fadd_rn(sqrtf(v) / s.bc2_sqrt, s.eps);
    return __fadd_rn(p, (__fmul_rn(s.neg_step, m)) / denom);
}

__global__ void k_adam(int64_t n, float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                       float *__restrict__ v, lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float mi = m[i], vi = v[i];
    p[i] = adam_elem(p[i], g[i], mi, vi, s);
    m[i] = mi;
    v[i] = vi;
}

// The four parameter tensors in one launch: index i of the concatenation W1 | b1 | W2 | b2 (the layout of the gradient and
// moment buffers).  The b1 / W2 copies the row kernels read (b1p [Hp], W2p [Hp, C], zero-padded) follow the update.
__global__ void k_tr_adam(int64_t total, int64_t o1, int64_t o2, int64_t o3, float *__restrict__ W1,
                          float *__restrict__ b1, float *__restrict__ W2, float *__restrict__ b2,
                          const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                          float *__restrict__ b1p, float *__restrict__ W2p, lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float *p = i < o1 ? W1 + i : i < o2 ? b1 + (i - o1) : i < o3 ? W2 + (i - o2) : b2 + (i - o3);
    float mi = m[i], vi = v[i];
    const float np = adam_elem(*p, g[i], mi, vi, s);
    *p = np;
    m[i] = mi;
    v[i] = vi;
    if (i >= o1 && i < o2) b1p[i - o1] = np;
    else if (i >= o2 && i < o3) W2p[i - o2] = np;
}

__global__ void k_tr_pad(const float *__restrict__ b1, const float *__restrict__ W2, int H, int Hp, int C,
                         float *__restrict__ b1p, float *__restrict__ W2p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Hp) b1p[i] = i < H ? b1[i] : 0.f;
    const int j = i - Hp;
    if (j >= 0 && j < Hp * C) W2p[j] = (j / C) < H ? W2[j] : 0.f;
}

extern "C" int lt_adam_step(int64_t n, float *p, const float *g, float *m, float *v, int64_t step, double lr,
                            double beta1, double beta2, double eps, double weight_decay, void *stream) {
    LT_REQUIRE(n >= 0, "lt_adam_step: n=%lld", (long long)n);
    LT_REQUIRE(step >= 1, "lt_adam_step: step=%lld, must be >= 1 (the count after this update)", (long long)step);
    if (n == 0) return LT_OK;
    LT_REQUIRE(p && g && m && v, "lt_adam_step: NULL pointer");
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, p, g, m, v,
                       adam_scalars(step, lr, beta1, beta2, eps, weight_decay));
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// --------------------------------------------------------------------------------------------
// trainer state
// --------------------------------------------------------------------------------------------
struct lt_gcn2_trainer {
    const lt_graph *g = nullptr;
    int32_t n = 0, F = 0, H = 0, C = 0, Hp = 0;
    const float *X = nullptr;
    int64_t ldx = 0;
    const int32_t *labels = nullptr;
    float *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr;
    double lr = 0, wd = 0, p = 0;
    uint64_t seed = 0;
    int64_t epoch = 0;            // epochs run since creation (= Adam's step count)
    int32_t kslice = 0;           // split-K slicing of X W1 (the forward's)
    int32_t tn_kslice = 0, tn_splits = 0;
    int32_t n_part = 0;           // row blocks of k_tr_bwd_rows
    float *S1 = nullptr, *Z1 = nullptr, *H1d = nullptr, *dZ1 = nullptr, *dS1 = nullptr;   // [n, Hp]
    float *S2 = nullptr, *Z2 = nullptr, *dZ2 = nullptr, *dS2 = nullptr;                   // [n, C]
    float *loss_r = nullptr;
    int32_t *corr_r = nullptr;
    float *b1p = nullptr, *W2p = nullptr;
    float *slabs = nullptr, *tn_slabs = nullptr, *part = nullptr, *seg_part = nullptr;
    float *grad = nullptr, *m = nullptr, *v = nullptr;   // [F*H | H | H*C | C]
    int64_t n_param = 0;
};

static void free_trainer(lt_gcn2_trainer *t) {
    if (!t) return;
    float *bufs[] = {t->S1, t->Z1, t->H1d, t->dZ1, t->dS1, t->S2, t->Z2, t->dZ2, t->dS2, t->loss_r, t->b1p, t->W2p,
                     t->slabs, t->tn_slabs, t->part, t->seg_part, t->grad, t->m, t->v};
    for (float *b : bufs) (void)hipFree(b);
    (void)hipFree(t->corr_r);
    delete t;
}

static int tn_pick_splits(int M, int N, int K) {
    // about two blocks per CU over the 256 CUs, slices of at least 256 rows
    const long tiles = (long)((M + TN_BM - 1) / TN_BM) * ((N + TN_BN - 1) / TN_BN);
    long s = (512 + tiles - 1) / tiles;
    s = s < 1 ? 1 : s > 16 ? 16 : s;
    while (s > 1 && (K + s - 1) / s < 256) --s;
    return (int)s;
}

extern "C" int lt_gcn2_trainer_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const int32_t *labels,
                                      int32_t H, int32_t C, float *W1, float *b1, float *W2, float *b2, double lr,
                                      double weight_decay, double dropout, uint64_t seed, void *stream,
                                      lt_gcn2_trainer **out) {
    LT_REQUIRE(out != nullptr, "lt_gcn2_trainer_create: out is NULL");
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "lt_gcn2_trainer_create: graph is NULL");
    LT_REQUIRE(F > 0 && H > 0 && C > 0, "lt_gcn2_trainer_create: F=%d H=%d C=%d must be positive", F, H, C);
    LT_REQUIRE(H <= LT_MAX_H && C <= LT_MAX_C, "lt_gcn2_trainer_create: H=%d C=%d (supported: H <= %d, C <= %d)", H, C,
               LT_MAX_H, LT_MAX_C);
    LT_REQUIRE(X && labels && W1 && b1 && W2 && b2, "lt_gcn2_trainer_create: NULL tensor pointer");
    LT_REQUIRE(ldx >= F, "lt_gcn2_trainer_create: ldx=%lld < F=%d", (long long)ldx, F);
    LT_REQUIRE(dropout >= 0.0 && dropout <= 1.0, "lt_gcn2_trainer_create: dropout=%g outside [0, 1]", dropout);
    LT_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "lt_gcn2_trainer_create: lr=%g weight_decay=%g", lr, weight_decay);
    LT_REQUIRE(g->n > 0, "lt_gcn2_trainer_create: empty graph");
    lt_gcn2_trainer *t = new (std::nothrow) lt_gcn2_trainer();
    if (!t) return lt_set_error(LT_ERR_NOMEM, "lt_gcn2_trainer_create: out of host memory");
    t->g = g; t->n = g->n; t->F = F; t->H = H; t->C = C; t->Hp = lt_round_up(H, 4);
    t->X = X; t->ldx = ldx; t->labels = labels;
    t->W1 = W1; t->b1 = b1; t->W2 = W2; t->b2 = b2;
    t->lr = lr; t->wd = weight_decay; t->p = dropout; t->seed = seed;
    t->kslice = lt_gemm_pick_kslice(t->n, H, F);
    t->tn_splits = tn_pick_splits(F, H, t->n);
    t->tn_kslice = lt_round_up((t->n + t->tn_splits - 1) / t->tn_splits, TN_BK);
    t->tn_splits = (t->n + t->tn_kslice - 1) / t->tn_kslice;
    t->n_part = (t->n + TR_ROWS_PER_BLOCK - 1) / TR_ROWS_PER_BLOCK;
    t->n_param = (int64_t)F * H + H + (int64_t)H * C + C;
    const size_t nh = (size_t)t->n * t->Hp * sizeof(float), nc = (size_t)t->n * C * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
#define T_HIP(call)                                                                         \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            free_trainer(t);                                                                \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)
    float **hbufs[] = {&t->S1, &t->Z1, &t->H1d, &t->dZ1, &t->dS1};
    for (float **b : hbufs) T_HIP(hipMalloc((void **)b, nh));
    float **cbufs[] = {&t->S2, &t->Z2, &t->dZ2, &t->dS2};
    for (float **b : cbufs) T_HIP(hipMalloc((void **)b, nc));
    T_HIP(hipMalloc((void **)&t->loss_r, (size_t)t->n * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->corr_r, (size_t)t->n * sizeof(int32_t)));
    T_HIP(hipMalloc((void **)&t->b1p, (size_t)t->Hp * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->W2p, (size_t)t->Hp * C * sizeof(float)));
    const size_t sb = lt_gemm_splitk_slab_bytes(t->n, H, F, t->kslice);
    if (sb) T_HIP(hipMalloc((void **)&t->slabs, sb));
    if (t->tn_splits > 1) T_HIP(hipMalloc((void **)&t->tn_slabs, (size_t)t->tn_splits * F * H * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->part, (size_t)t->n_part * ((size_t)H + (size_t)H * C) * sizeof(float)));
    if (g->p_n_seg > 0) T_HIP(hipMalloc((void **)&t->seg_part, (size_t)g->p_n_seg * t->Hp * sizeof(float)));
    float **pbufs[] = {&t->grad, &t->m, &t->v};
    for (float **b : pbufs) T_HIP(hipMalloc((void **)b, (size_t)t->n_param * sizeof(float)));
    // pad columns of S1 (the GEMM writes H of them) and the moments start at zero
    T_HIP(hipMemsetAsync(t->S1, 0, nh, st));
    T_HIP(hipMemsetAsync(t->m, 0, (size_t)t->n_param * sizeof(float), st));
    T_HIP(hipMemsetAsync(t->v, 0, (size_t)t->n_param * sizeof(float), st));
#undef T_HIP
    *out = t;
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_destroy(lt_gcn2_trainer *t) {
    free_trainer(t);
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_epoch(const lt_gcn2_trainer *t, int64_t *epoch) {
    LT_REQUIRE(t != nullptr && epoch != nullptr, "lt_gcn2_trainer_epoch: NULL argument");
    *epoch = t->epoch;
    return LT_OK;
}

static unsigned rows_grid(int n, int rows_per_block) { return (unsigned)((n + rows_per_block - 1) / rows_per_block); }

static int run_epoch(lt_gcn2_trainer *t, float *record, hipStream_t st) {
    const lt_graph *g = t->g;
    const int n = t->n, F = t->F, H = t->H, C = t->C, Hp = t->Hp;
    const int lpr = lt_lpr_for(Hp), cp = lt_cp_for(C);
    const int rpb = (TR_BLOCK / 64) * (64 / lpr);
    int rc;
    // forward: the launches of lt_gcn2_forward
    if (t->slabs)
        rc = lt_launch_gemm_splitk(t->X, t->ldx, t->W1, H, t->S1, Hp, n, H, F, t->kslice, t->slabs, st);
    else
        rc = lt_launch_gemm(t->X, t->ldx, t->W1, H, t->S1, Hp, n, H, F, st);
    if (rc) return rc;
    rc = lt_launch_layer1(g, t->S1, Hp, t->b1p, t->W2p, C, t->Z1, t->S2, st, t->seg_part);
    if (rc) return rc;
    lt_drop_args d;
    d.on = t->p > 0.0;
    d.thresh = (uint64_t)floor(t->p * 4294967296.0);
    d.scale = t->p < 1.0 ? (float)(1.0 / (1.0 - t->p)) : 0.f;
    d.epoch = (uint32_t)t->epoch;
    d.seed = t->seed;
    LT_DISPATCH_LPR(lpr, LT_DISPATCH_CP(cp,
        hipLaunchKernelGGL((k_tr_dropout<LPR_, CP_>), dim3(rows_grid(n, rpb)), dim3(TR_BLOCK), 0, st, n, t->Z1, Hp, H, t->W2p,
                           C, d, t->H1d, t->S2)));
    LT_CHECK_LAUNCH();
    rc = lt_launch_layer2(g, t->S2, C, t->b2, t->Z2, st);
    if (rc) return rc;
    // loss head
    float *gW1 = t->grad, *gb1 = gW1 + (size_t)F * H, *gW2 = gb1 + H, *gb2 = gW2 + (size_t)H * C;
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce<CP_>), dim3(rows_grid(n, TR_BLOCK)), dim3(TR_BLOCK), 0, st, n, t->Z2, C,
                                          t->labels, 1.0f / (float)n, t->loss_r, t->corr_r, t->dZ2));
    LT_CHECK_LAUNCH();
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce_reduce<CP_>), dim3(1), dim3(TR_BLOCK), 0, st, n, C, t->loss_r, t->corr_r,
                                          t->dZ2, record, gb2));
    LT_CHECK_LAUNCH();
    // backward
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_spmm_t_narrow<CP_>), dim3(rows_grid(n, TR_BLOCK / LT_L2_LANES)),
                                          dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZ2, C, t->dS2));
    LT_CHECK_LAUNCH();
    int W = 1;
    while (W < Hp) W <<= 1;
    const float scale = t->p > 0.0 ? (t->p < 1.0 ? (float)(1.0 / (1.0 - t->p)) : 0.f) : 1.f;
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_bwd_rows<CP_>), dim3((unsigned)t->n_part), dim3(TR_BLOCK), 0, st, n, H, Hp, W,
                                          C, t->H1d, t->dS2, t->W2p, scale, t->dZ1, t->part));
    LT_CHECK_LAUNCH();
    const int L = H + H * C;   // db1 | dW2: adjacent in the gradient buffer
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((L + 63) / 64)), dim3(TR_BLOCK), 0, st, t->part, t->n_part, L, gb1);
    LT_CHECK_LAUNCH();
    LT_DISPATCH_LPR(lpr, hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, rpb)), dim3(TR_BLOCK), 0, st, n,
                                            g->tptr, g->trow, g->tval, t->dZ1, Hp, t->dS1));
    LT_CHECK_LAUNCH();
    {
        const bool split = t->tn_splits > 1;
        dim3 grid((unsigned)((F + TN_BM - 1) / TN_BM), (unsigned)((H + TN_BN - 1) / TN_BN), (unsigned)t->tn_splits);
        hipLaunchKernelGGL(k_gemm_tn_mfma, grid, dim3(256), 0, st, t->X, (long)t->ldx, t->dS1, (long)Hp,
                           split ? t->tn_slabs : gW1, (long)H, F, H, n, t->tn_kslice, (long)F * H);
        LT_CHECK_LAUNCH();
        if (split) {
            rc = lt_launch_sum_slabs(t->tn_slabs, (long)F * H, t->tn_splits, F, H, (long)H, gW1, (long)H, st);
            if (rc) return rc;
        }
    }
    // Adam
    const int64_t step = t->epoch + 1;
    const int64_t o1 = (int64_t)F * H, o2 = o1 + H, o3 = o2 + (int64_t)H * C;
    hipLaunchKernelGGL(k_tr_adam, dim3((unsigned)((t->n_param + 255) / 256)), dim3(256), 0, st, t->n_param, o1, o2, o3,
                       t->W1, t->b1, t->W2, t->b2, t->grad, t->m, t->v, t->b1p, t->W2p,
                       adam_scalars(step, t->lr, 0.9, 0.999, 1e-8, t->wd));
    LT_CHECK_LAUNCH();
    t->epoch = step;
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_run(lt_gcn2_trainer *t, int32_t n_epochs, float *record, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_run: trainer is NULL");
    LT_REQUIRE(n_epochs >= 0, "lt_gcn2_trainer_run: n_epochs=%d", n_epochs);
    if (n_epochs == 0) return LT_OK;
    LT_REQUIRE(record != nullptr, "lt_gcn2_trainer_run: record is NULL");
    LT_REQUIRE(t->epoch + n_epochs <= (int64_t)UINT32_MAX, "lt_gcn2_trainer_run: epoch counter would pass 2^32");
    hipStream_t st = (hipStream_t)stream;
    // the borrowed parameters may have changed since the last run: b1p / W2p from them (Adam keeps them current after that)
    hipLaunchKernelGGL(k_tr_pad, dim3((t->Hp * (t->C + 1) + 255) / 256), dim3(256), 0, st, t->b1, t->W2, t->H, t->Hp, t->C,
                       t->b1p, t->W2p);
    LT_CHECK_LAUNCH();
    for (int32_t j = 0; j < n_epochs; ++j) {
        const int rc = run_epoch(t, record + 2 * (size_t)j, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_grads(const lt_gcn2_trainer *t, float *dW1, float *db1, float *dW2, float *db2, void *stream) {
    LT_REQUIRE(t != nullptr && dW1 && db1 && dW2 && db2, "lt_gcn2_trainer_grads: NULL argument");
    hipStream_t st = (hipStream_t)stream;
    const size_t fh = (size_t)t->F * t->H, hc = (size_t)t->H * t->C;
    LT_HIP(hipMemcpyAsync(dW1, t->grad, fh * sizeof(float), hipMemcpyDeviceToDevice, st));
    LT_HIP(hipMemcpyAsync(db1, t->grad + fh, (size_t)t->H * sizeof(float), hipMemcpyDeviceToDevice, st));
    LT_HIP(hipMemcpyAsync(dW2, t->grad + fh + t->H, hc * sizeof(float), hipMemcpyDeviceToDevice, st));
    LT_HIP(hipMemcpyAsync(db2, t->grad + fh + t->H + hc, (size_t)t->C * sizeof(float), hipMemcpyDeviceToDevice, st));
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_logits(const lt_gcn2_trainer *t, float *Z2, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr && Z2 != nullptr, "lt_gcn2_trainer_logits: NULL argument");
    LT_REQUIRE(ldz >= t->C, "lt_gcn2_trainer_logits: ldz=%lld < C=%d", (long long)ldz, t->C);
    LT_HIP(hipMemcpy2DAsync(Z2, (size_t)ldz * sizeof(float), t->Z2, (size_t)t->C * sizeof(float), (size_t)t->C * sizeof(float),
                            (size_t)t->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}
