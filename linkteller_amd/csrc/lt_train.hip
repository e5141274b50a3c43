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
// The 3-layer GCN's epoch (lt_gcn3_trainer_*) is built from the same kernels further down, with its own launch table.
//
// Every reduction has a fixed order (no float atomics): two trainings with the same inputs give the same bits.
// Built with -ffp-contract=off: the only fused operations are explicit fmaf calls and the MFMAs.
#include <math.h>

#include <new>

#include "lt_philox.hip.h"
#include "lt_rows.hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

#define TR_BLOCK 256
#define TR_ROWS_PER_BLOCK 32   // k_tr_bwd_rows: rows summed by one block (its partial is one slab of the column sums)

// --------------------------------------------------------------------------------------------
// The dropout mask: Philox4x32-10 (lt_philox.hip.h)
// --------------------------------------------------------------------------------------------
// word (i & 3) of Philox(counter (q lo, q hi, epoch, layer), key (seed lo, seed hi)), q = i >> 2
__device__ __forceinline__ uint4 lt_drop_block(uint64_t q, uint32_t epoch, uint64_t seed, uint32_t layer) {
    return lt_philox4x32_10(make_uint4((uint32_t)q, (uint32_t)(q >> 32), epoch, layer),
                            make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

struct lt_drop_args {
    int on;              // 0: p == 0, no RNG call
    uint64_t thresh;     // keep iff u >= thresh = floor(p * 2^32)  (2^32 for p == 1: nothing is kept)
    float scale;         // 1 / (1 - p), rounded once from double
    uint32_t epoch;
    uint64_t seed;
    uint32_t layer = 0;  // counter word 3: the hidden layer the mask belongs to (the 2-layer trainer has one: 0)
};

// columns coff .. coff + 3 of row r of a [n, H] hidden layer (h >= 0 already): kept elements scaled, the others and the
// pad columns zero
__device__ __forceinline__ f32x4 lt_drop4(f32x4 h, int r, int coff, int H, const lt_drop_args &d) {
    const uint64_t i0 = (uint64_t)r * H + coff;
    uint32_t u[4];
    if ((H & 3) == 0) {    // the 4 columns are the 4 words of one Philox block
        const uint4 w = lt_drop_block(i0 >> 2, d.epoch, d.seed, d.layer);
        u[0] = w.x; u[1] = w.y; u[2] = w.z; u[3] = w.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t i = i0 + j;
            const uint4 w = lt_drop_block(i >> 2, d.epoch, d.seed, d.layer);
            const uint32_t sel = (uint32_t)(i & 3);
            u[j] = sel == 0 ? w.x : sel == 1 ? w.y : sel == 2 ? w.z : w.w;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool keep = coff + j < H && (uint64_t)u[j] >= d.thresh;
        h[j] = keep ? h[j] * d.scale : 0.f;
    }
    return h;
}

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
        if (d.on) h = lt_drop4(h, r, coff, H, d);
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
// Validation (reference gcn_trainer.py:167-174 + utils/early_stopping.py): the evaluation head in two kernels, the
// early-stopping state in device memory, the predicated snapshot of the parameters.
// --------------------------------------------------------------------------------------------
// Row stage: k_tr_ce's per-row arithmetic (the same operations in the same order: the same row losses and argmax), one
// thread per row.  Block b leaves the tree sum of its 256 row losses in part_loss[b] and its C x C confusion cells
// (true class, predicted class) in part_cnt[b, C * C]; a label outside [0, C) counts in no cell.
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_val_rows(int n, const float *__restrict__ Z, long ldz, int C,
                                                       const int32_t *__restrict__ labels, float *__restrict__ part_loss,
                                                       int32_t *__restrict__ part_cnt) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int sc[CP * CP];
    const int t = threadIdx.x;
    const int r = blockIdx.x * TR_BLOCK + t;
    if (t < CP * CP) sc[t] = 0;
    __syncthreads();
    float l = 0.f;
    if (r < n) {
        const int y = labels[r];
        float z[CP];
#pragma unroll
        for (int c = 0; c < CP; ++c) z[c] = c < C ? Z[(size_t)r * ldz + c] : -INFINITY;
        float mx = z[0];
        int arg = 0;
#pragma unroll
        for (int c = 1; c < CP; ++c)
            if (c < C && z[c] > mx) { mx = z[c]; arg = c; }
        float s = 0.f, zy = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float e = c < C ? expf(z[c] - mx) : 0.f;
            s += e;
            if (c == y) zy = z[c];
        }
        l = (mx + logf(s)) - zy;
        if ((unsigned)y < (unsigned)C) atomicAdd(&sc[y * C + arg], 1);   // integer LDS atomics: the counts do not depend on order
    }
    sl[t] = l;
    __syncthreads();
    for (int w = TR_BLOCK / 2; w >= 1; w >>= 1) {
        if (t < w) sl[t] += sl[t + w];
        __syncthreads();
    }
    if (t == 0) part_loss[blockIdx.x] = sl[0];
    if (t < C * C) part_cnt[(size_t)blockIdx.x * (C * C) + t] = sc[t];
}

// Row stage over a list: entry i = blockIdx.x * 256 + t scores logits row rows[i] against labels[rows[i]] with k_val_rows'
// per-row arithmetic (the same operations in the same order), the same block tree and the same partials, so the list
// 0 .. n - 1 leaves k_val_rows' bits.  An id outside [0, n) is never dereferenced: its entry adds 0 to the loss and counts in
// no cell; each block adds its number of such entries to *n_bad (an integer atomic: the total does not depend on order).
template <int CP>
__global__ __launch_bounds__(TR_BLOCK) void k_val_rows_list(int n, int m, const int32_t *__restrict__ rows,
                                                            const float *__restrict__ Z, long ldz, int C,
                                                            const int32_t *__restrict__ labels, float *__restrict__ part_loss,
                                                            int32_t *__restrict__ part_cnt, int32_t *n_bad) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int sc[CP * CP];
    __shared__ int sbad;
    const int t = threadIdx.x;
    const int i = blockIdx.x * TR_BLOCK + t;
    if (t < CP * CP) sc[t] = 0;
    if (t == 0) sbad = 0;
    __syncthreads();
    float l = 0.f;
    if (i < m) {
        const int r = rows[i];
        if ((unsigned)r < (unsigned)n) {
            const int y = labels[r];
            float z[CP];
#pragma unroll
            for (int c = 0; c < CP; ++c) z[c] = c < C ? Z[(size_t)r * ldz + c] : -INFINITY;
            float mx = z[0];
            int arg = 0;
#pragma unroll
            for (int c = 1; c < CP; ++c)
                if (c < C && z[c] > mx) { mx = z[c]; arg = c; }
            float s = 0.f, zy = 0.f;
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const float e = c < C ? expf(z[c] - mx) : 0.f;
                s += e;
                if (c == y) zy = z[c];
            }
            l = (mx + logf(s)) - zy;
            if ((unsigned)y < (unsigned)C) atomicAdd(&sc[y * C + arg], 1);
        } else if (n_bad) {
            atomicAdd(&sbad, 1);
        }
    }
    sl[t] = l;
    __syncthreads();
    for (int w = TR_BLOCK / 2; w >= 1; w >>= 1) {
        if (t < w) sl[t] += sl[t + w];
        __syncthreads();
    }
    if (t == 0) part_loss[blockIdx.x] = sl[0];
    if (t < C * C) part_cnt[(size_t)blockIdx.x * (C * C) + t] = sc[t];
    if (t == 0 && n_bad && sbad) atomicAdd(n_bad, sbad);
}

// The early-stopping state: 8 words of device memory.
#define VAL_STATE_WORDS 8
enum { VS_BEST_LOSS = 0, VS_BEST_EPOCH = 1, VS_COUNTER = 2, VS_STOP_EPOCH = 3, VS_IMPROVED = 4, VS_SEEN = 5 };

// EarlyStopping.__call__ with delta = 0 on the loss itself (score = -loss: `score < best_score` is `loss > best`, false for
// a tie and for a NaN on either side).  patience 0: never stops.
__device__ __forceinline__ void val_state_update(int32_t *s, float loss, int patience, int epoch) {
    if (s[VS_STOP_EPOCH] >= 0) {
        s[VS_IMPROVED] = 0;
        return;
    }
    const float best = __int_as_float(s[VS_BEST_LOSS]);
    if (s[VS_SEEN] > 0 && loss > best) {
        const int c = s[VS_COUNTER] + 1;
        s[VS_COUNTER] = c;
        s[VS_IMPROVED] = 0;
        if (patience > 0 && c >= patience) s[VS_STOP_EPOCH] = epoch;
    } else {
        s[VS_BEST_LOSS] = __float_as_int(loss);
        s[VS_BEST_EPOCH] = epoch;
        s[VS_COUNTER] = 0;
        s[VS_IMPROVED] = 1;
    }
    s[VS_SEEN] = 1;
}

// Finish stage, one block: thread t adds the partial losses t, t + 256, ... in ascending block order, then the fixed tree;
// the cells are integers (lane group k of 4 takes the partials k, k + 4, ...).  Thread 0 writes the mean loss and, when a
// state block is given, applies the epoch to it.
__global__ __launch_bounds__(TR_BLOCK) void k_val_finish(int n_blk, int n, int C, const float *__restrict__ part_loss,
                                                         const int32_t *__restrict__ part_cnt, float *__restrict__ loss_out,
                                                         int32_t *__restrict__ conf_out, int32_t *state, int patience,
                                                         int epoch) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int sc[4][64];
    const int t = threadIdx.x, cc = C * C;
    float l = 0.f;
    for (int b = t; b < n_blk; b += TR_BLOCK) l += part_loss[b];
    sl[t] = l;
    const int cell = t & 63, grp = t >> 6;
    int k = 0;
    if (cell < cc)
        for (int b = grp; b < n_blk; b += 4) k += part_cnt[(size_t)b * cc + cell];
    sc[grp][cell] = k;
    __syncthreads();
    for (int w = TR_BLOCK / 2; w >= 1; w >>= 1) {
        if (t < w) sl[t] += sl[t + w];
        __syncthreads();
    }
    if (t < cc) conf_out[t] = (sc[0][t] + sc[1][t]) + (sc[2][t] + sc[3][t]);
    if (t == 0) {
        const float mean = sl[0] / (float)n;
        *loss_out = mean;
        if (state) val_state_update(state, mean, patience, epoch);
    }
}

__global__ void k_val_state(const float *__restrict__ loss, int32_t *state, int patience, int epoch) {
    if (blockIdx.x == 0 && threadIdx.x == 0) val_state_update(state, *loss, patience, epoch);
}

__global__ void k_val_state_reset(int32_t *state) {
    const int t = threadIdx.x;
    if (t < VAL_STATE_WORDS) state[t] = (t == VS_BEST_EPOCH || t == VS_STOP_EPOCH) ? -1 : 0;
}

// Predicated copy between the live parameter tensors (segment k = elements [o[k - 1], o[k]) of the concatenation) and the
// contiguous snapshot: every thread reads *flag, a word an earlier launch on the stream wrote, and returns when it is 0.
// V floats per thread: the host picks the widest V for which every pointer is V * 4-byte aligned and every segment starts
// at a multiple of V; a vector that would cross its segment's end (the last one only, then) is copied element by element.
struct lt_snap_segs {
    float *p[6];
    int64_t o[6];
};

template <int V>
__global__ __launch_bounds__(256) void k_val_snapshot(lt_snap_segs T, float *__restrict__ snap,
                                                      const int32_t *__restrict__ flag, int to_live) {
    if (*flag == 0) return;
    const int64_t e0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    if (e0 >= T.o[5]) return;
    const int k = e0 < T.o[0] ? 0 : e0 < T.o[1] ? 1 : e0 < T.o[2] ? 2 : e0 < T.o[3] ? 3 : e0 < T.o[4] ? 4 : 5;
    const int64_t end = T.o[k], j = k ? e0 - T.o[k - 1] : e0;
    float *p;      // a switch over constant indices, as in k_tr3_adam
    switch (k) {
        case 0: p = T.p[0]; break;
        case 1: p = T.p[1]; break;
        case 2: p = T.p[2]; break;
        case 3: p = T.p[3]; break;
        case 4: p = T.p[4]; break;
        default: p = T.p[5]; break;
    }
    float *live = p + j, *kept = snap + e0;
    float *dst = to_live ? live : kept;
    const float *src = to_live ? kept : live;
    typedef float fvec __attribute__((ext_vector_type(V)));
    if (e0 + V <= end) {
        *reinterpret_cast<fvec *>(dst) = *reinterpret_cast<const fvec *>(src);
    } else {
        for (int i = 0; i < V && e0 + i < end; ++i) dst[i] = src[i];
    }
}

static int snap_width(const lt_snap_segs &T, const float *snap) {
    int V = 4;
    for (; V > 1; V >>= 1) {
        bool ok = ((uintptr_t)snap % (V * sizeof(float))) == 0;
        for (int k = 0; k < 6 && ok; ++k) {
            const int64_t b = k ? T.o[k - 1] : 0;
            if (T.o[k] == b) continue;      // an empty segment (the 2-layer trainer has four)
            ok = (b % V) == 0 && ((uintptr_t)T.p[k] % (V * sizeof(float))) == 0;
        }
        if (ok) break;
    }
    return V;
}

static int launch_snapshot(const lt_snap_segs &T, float *snap, const int32_t *flag, int to_live, hipStream_t st) {
    const int V = snap_width(T, snap);
    const int64_t threads = (T.o[5] + V - 1) / V;
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (V == 4) hipLaunchKernelGGL((k_val_snapshot<4>), grid, dim3(256), 0, st, T, snap, flag, to_live);
    else if (V == 2) hipLaunchKernelGGL((k_val_snapshot<2>), grid, dim3(256), 0, st, T, snap, flag, to_live);
    else hipLaunchKernelGGL((k_val_snapshot<1>), grid, dim3(256), 0, st, T, snap, flag, to_live);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// What a trainer with validation attached owns: the forward's buffers at the validation graph's size, the head's partials,
// the state block and (keep_best) the snapshot.
struct lt_val {
    const lt_graph *g = nullptr;
    int32_t n = 0;
    const float *X = nullptr;
    int64_t ldx = 0;
    const int32_t *labels = nullptr;
    const int32_t *rows = nullptr;         // attach_validation_rows: the head scores these m rows (borrowed); NULL: all n
    int32_t m = 0;
    int32_t keep_best = 0, patience = 0;
    int32_t kslice = 0;           // split-K slicing of X2 W1, chosen for n2 (the forward's choice at that size)
    int32_t n_blk = 0;            // blocks of k_val_rows (of k_val_rows_list with a row list)
    float *S1 = nullptr, *Z1 = nullptr;    // [n2, Hp1]; Z1 only feeds the tiled layer-1 route (2-layer model)
    float *H1 = nullptr;                   // [n2, Hp1] 3-layer model: relu(A S1 + b1)
    float *S2 = nullptr, *Z2 = nullptr;    // [n2, Hp2] 3-layer model
    float *Sc = nullptr, *Z = nullptr;     // [n2, C]: the last product and the validation logits
    float *slabs = nullptr, *seg_part = nullptr;
    float *part_loss = nullptr;            // [n_blk]
    int32_t *part_cnt = nullptr;           // [n_blk, C * C]
    int32_t *state = nullptr;              // [VAL_STATE_WORDS]
    float *snap = nullptr;                 // [n_param] (keep_best)
};

static void free_val(lt_val *v) {
    if (!v) return;
    float *bufs[] = {v->S1, v->Z1, v->H1, v->S2, v->Z2, v->Sc, v->Z, v->slabs, v->seg_part, v->part_loss, v->snap};
    for (float *b : bufs) (void)hipFree(b);
    (void)hipFree(v->part_cnt);
    (void)hipFree(v->state);
    delete v;
}

static size_t val_head_bytes(int n, int C) {
    const size_t n_blk = (size_t)((n + TR_BLOCK - 1) / TR_BLOCK);
    return n_blk * (1 + (size_t)C * C) * sizeof(float);
}

static int launch_val_head(const float *Z, long ldz, const int32_t *labels, int n, int C, float *part_loss,
                           int32_t *part_cnt, float *loss_out, int32_t *conf_out, int32_t *state, int patience, int epoch,
                           hipStream_t st) {
    const int n_blk = (n + TR_BLOCK - 1) / TR_BLOCK;
    LT_DISPATCH_CP(lt_cp_for(C), hipLaunchKernelGGL((k_val_rows<CP_>), dim3((unsigned)n_blk), dim3(TR_BLOCK), 0, st, n, Z, ldz,
                                                    C, labels, part_loss, part_cnt));
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_val_finish, dim3(1), dim3(TR_BLOCK), 0, st, n_blk, n, C, part_loss, part_cnt, loss_out, conf_out,
                       state, patience, epoch);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// the head over a row list: k_val_rows_list over ceil(m / 256) blocks, then the finish stage with m as the divisor
static int launch_val_head_rows(const float *Z, long ldz, const int32_t *labels, int n, int C, const int32_t *rows, int m,
                                float *part_loss, int32_t *part_cnt, float *loss_out, int32_t *conf_out, int32_t *n_bad,
                                int32_t *state, int patience, int epoch, hipStream_t st) {
    const int n_blk = (m + TR_BLOCK - 1) / TR_BLOCK;
    LT_DISPATCH_CP(lt_cp_for(C), hipLaunchKernelGGL((k_val_rows_list<CP_>), dim3((unsigned)n_blk), dim3(TR_BLOCK), 0, st, n, m,
                                                    rows, Z, ldz, C, labels, part_loss, part_cnt, n_bad));
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_val_finish, dim3(1), dim3(TR_BLOCK), 0, st, n_blk, m, C, part_loss, part_cnt, loss_out, conf_out,
                       state, patience, epoch);
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
    lt_val *val = nullptr;        // lt_gcn2_trainer_attach_validation (owned)
};

static void free_trainer(lt_gcn2_trainer *t) {
    if (!t) return;
    free_val(t->val);
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

// ============================================================================================
// Training of the 3-layer GCN (reference gcn/models.py:28-46): the 2-layer epoch one layer up.
//
//   S1 = X W1                      lt_launch_gemm(_splitk)        the 2-layer trainer's product
//   H1d = drop_0(relu(A S1 + b1))  k_tr3_layer1 (+ _long)         row_dot chains from the bias, ReLU and the Philox mask (layer
//                                                                 word 0) as the epilogue: Z1 never exists in memory
//   S2 = H1d W2                    lt_launch_gemm
//   Z2 = A S2 + b2                 lt_launch_layer1 (Z2 stored)
//   H2d = drop_1(relu(Z2)), S3     k_tr_dropout, layer word 1
//   Z3 = A S3 + b3                 lt_launch_layer2
//   loss, dZ3, db3, correct        k_tr_ce, k_tr_ce_reduce
//   dS3 = A^T dZ3                  k_tr_spmm_t_narrow
//   dZ2, db2 | dW3                 k_tr_bwd_rows(H2d, dS3, W3p) + k_tr_colsum
//   dS2 = A^T dZ2                  k_tr_spmm_t_wide
//   dW2 = H1d^T dS2                k_gemm_tn_mfma + k_sum_slabs
//   dZ1 = [H1d > 0] scale (dS2 W2^T), db1 slabs     k_tr3_dz_mfma, then k_tr_colsum
//   dS1 = A^T dZ1; dW1 = X^T dS1   k_tr_spmm_t_wide, k_gemm_tn_mfma + k_sum_slabs
//   Adam                           k_tr3_adam                     one launch over W1 | b1 | W2 | b2 | W3 | b3 and the padded copies
// ============================================================================================

// H1d[r] = drop(relu(A[r, :] S + bias)) for every row.  The launch's first seg_blocks blocks take the SEGMENTS of the hub rows
// (k_layer1's scheme: row_dot's canonical order, the first segment's chain started from the bias); k_tr3_layer1_long adds
// them in segment order and applies the same epilogue.
template <int LPR>
__global__ __launch_bounds__(TR_BLOCK) void k_tr3_layer1(
    int n, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
    const float *__restrict__ S, int Hp, int H, const float *__restrict__ biasp, lt_drop_args d, float *__restrict__ Hd,
    int skip_long, int seg_blocks, int n_seg, const int32_t *__restrict__ seg_long, const int32_t *__restrict__ seg_begin,
    const int32_t *__restrict__ long_row, float *__restrict__ seg_part) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int gl = lane & (LPR - 1);
    const int coff = 4 * gl;
    const bool active = coff < Hp;
    if ((int)blockIdx.x < seg_blocks) {
        int sg = ((blockIdx.x * TR_BLOCK + threadIdx.x) >> 6) * RPW + lane / LPR;
        if (LPR == 64) sg = __builtin_amdgcn_readfirstlane(sg);
        if (sg >= n_seg) return;
        const int rs = long_row[seg_long[sg]];
        const int s0 = seg_begin[sg], s1 = min(rowptr[rs + 1], s0 + LT_ROW_SEG);
        const f32x4 init = (active && s0 == rowptr[rs]) ? ld4(biasp + coff) : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 zs = seg_chain<16>(col, val, s0, s1, S, Hp, coff, active, -1, nullptr, init);
        if (active) *reinterpret_cast<f32x4 *>(seg_part + (size_t)sg * Hp + coff) = zs;
        return;
    }
    const int wave = (((int)blockIdx.x - seg_blocks) * TR_BLOCK + threadIdx.x) >> 6;
    int r = wave * RPW + lane / LPR;
    if (LPR == 64) r = __builtin_amdgcn_readfirstlane(r);
    if (r >= n) return;
    if (skip_long && rowptr[r + 1] - rowptr[r] > LT_ROW_SEG) return;
    const f32x4 bv = active ? ld4(biasp + coff) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 z = row_dot<8>(col, val, rowptr[r], rowptr[r + 1], S, Hp, coff, active, -1, nullptr, bv);
    if (active) {
        f32x4 h = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
        if (d.on) h = lt_drop4(h, r, coff, H, d);
        *reinterpret_cast<f32x4 *>(Hd + (size_t)r * Hp + coff) = h;
    }
}

template <int LPR>
__global__ __launch_bounds__(TR_BLOCK) void k_tr3_layer1_long(int n_long, const int32_t *__restrict__ long_row,
                                                              const int32_t *__restrict__ long_segptr,
                                                              const float *__restrict__ part, int Hp, int H, lt_drop_args d,
                                                              float *__restrict__ Hd) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * TR_BLOCK + threadIdx.x) >> 6;
    const int gl = lane & (LPR - 1);
    int li = wave * RPW + lane / LPR;
    if (LPR == 64) li = __builtin_amdgcn_readfirstlane(li);
    if (li >= n_long) return;
    const int coff = 4 * gl;
    if (coff >= Hp) return;
    const int r = long_row[li];
    const int s0 = long_segptr[li], s1 = long_segptr[li + 1];
    f32x4 z = ld4(part + (size_t)s0 * Hp + coff);
    for (int s = s0 + 1; s < s1; ++s) {
        const f32x4 t = ld4(part + (size_t)s * Hp + coff);
        z.x += t.x; z.y += t.y; z.z += t.z; z.w += t.w;
    }
    f32x4 h = {fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
    if (d.on) h = lt_drop4(h, r, coff, H, d);
    *reinterpret_cast<f32x4 *>(Hd + (size_t)r * Hp + coff) = h;
}

// --------------------------------------------------------------------------------------------
// dZ[M, N] = [Hd > 0] * scale * (A W^T) with A = dS2 [M = n, K = H2] and the weight W = W2 [N = H1, K = H2] read as it
// lies: its 64 x 16 tile is loaded as rows of 4 consecutive k and transposed on its way into LDS (rows of the LDS tile
// padded to 65 floats).  (A transposed mirror of W2 kept current by the Adam launch and read with the NN tile shape
// measured the same per epoch and was removed: NOTES.md section 13.)
// Block / wave structure of k_gemm_f32_mfma: 64 x 64 block tile, four waves of one 32 x 32 v_mfma_f32_32x32x2_f32 tile,
// 16-deep k-tiles with a register prefetch.  K <= 256: one pass, no split-K.  Epilogue: the mask and the scale, the store,
// and the block's column sums (a lane's 16 rows in register order, the two half-waves, the two row waves) into slab
// blockIdx.x of part [gridDim.x, N]: k_tr_colsum adds the slabs in order for db1.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tr3_dz_mfma(const float *__restrict__ A, long lda, const float *__restrict__ B,
                                                     long ldb, const float *__restrict__ Hd, float *__restrict__ dZ,
                                                     long ldz, int M, int N, int K, float scale,
                                                     float *__restrict__ part) {
    constexpr int LDB = TN_BN + 1;
    __shared__ __attribute__((aligned(16))) float As[2][TN_BM * TN_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][TN_BK * LDB];
    __shared__ float red[2][TN_BN];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int m0 = blockIdx.x * TN_BM;
    const int n0 = blockIdx.y * TN_BN;
    const int a_row = tid >> 2, a_col = (tid & 3) * 4;          // A tile 64 x 16: row tid / 4, 4 consecutive k
    const bool a_row_ok = (m0 + a_row) < M;
    const float *a_ptr = A + (long)(m0 + a_row) * lda + a_col;
    const int b_row = tid >> 2, b_col = (tid & 3) * 4;          // W2 tile 64 x 16: n-row tid / 4, 4 consecutive k
    const float *b_ptr = B + (long)(n0 + b_row) * ldb + b_col;

    f32x4 ra, rb;
    auto load_tiles = [&](int k0) {
        ra = f32x4{0.f, 0.f, 0.f, 0.f};
        rb = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a_row_ok) {
            if (k0 + a_col + 3 < K) {
                ra = *reinterpret_cast<const f32x4u *>(a_ptr + k0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + a_col + j < K) ra[j] = a_ptr[k0 + j];
            }
        }
        if (n0 + b_row < N) {
            if (k0 + b_col + 3 < K) {
                rb = *reinterpret_cast<const f32x4u *>(b_ptr + k0);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + b_col + j < K) rb[j] = b_ptr[k0 + j];
            }
        }
    };
    auto store_tiles = [&](int buf) {
        float *as = &As[buf][a_row * TN_LDA + a_col];
        as[0] = ra.x; as[1] = ra.y; as[2] = ra.z; as[3] = ra.w;
        float *bs = &Bs[buf][b_col * LDB + b_row];
        bs[0] = rb.x; bs[LDB] = rb.y; bs[2 * LDB] = rb.z; bs[3 * LDB] = rb.w;
    };

    f32x16 acc, total;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; total[i] = 0.f; }
    const int nk = (K + TN_BK - 1) / TN_BK;
    load_tiles(0);
    store_tiles(0);
    __syncthreads();
    const int a_frag = (wr * 32 + (lane & 31)) * TN_LDA + (lane >> 5);
    const int b_frag = (lane >> 5) * LDB + wc * 32 + (lane & 31);
    constexpr int FOLD_TILES = TN_FOLD / TN_BK;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles((kt + 1) * TN_BK);
        const float *as = &As[buf][a_frag];
        const float *bs = &Bs[buf][b_frag];
#pragma unroll
        for (int kk = 0; kk < TN_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk], bs[kk * LDB], acc, 0, 0, 0);
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
    float cs = 0.f;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int cm = m0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        float dz = 0.f;
        if (cm < M && cn < N) {
            dz = Hd[(long)cm * ldz + cn] > 0.f ? total[reg] * scale : 0.f;
            dZ[(long)cm * ldz + cn] = dz;
        }
        cs += dz;
    }
    cs += __shfl_xor(cs, 32, 64);
    if (lane < 32) red[wr][wc * 32 + lane] = cs;
    __syncthreads();
    if (tid < TN_BN && n0 + tid < N) part[(size_t)blockIdx.x * N + n0 + tid] = red[0][tid] + red[1][tid];
}

// The six parameter tensors in one launch: index i of the concatenation W1 | b1 | W2 | b2 | W3 | b3 (o[k] = where tensor
// k ends).  The copies the row kernels read follow the update: b1p [Hp1], b2p [Hp2], W3p [Hp2, C] (zero-padded).
struct lt_tr3_tensors {
    float *p[6];
    int64_t o[6];
    float *b1p, *b2p, *W3p;
};

__global__ void k_tr3_adam(lt_tr3_tensors T, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                           lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.o[5]) return;
    const int k = i < T.o[0] ? 0 : i < T.o[1] ? 1 : i < T.o[2] ? 2 : i < T.o[3] ? 3 : i < T.o[4] ? 4 : 5;
    const int64_t j = k ? i - T.o[k - 1] : i;
    float *p;      // a switch over constant indices: T.p[k] with a run-time k would move the argument struct to scratch
    switch (k) {
        case 0: p = T.p[0]; break;
        case 1: p = T.p[1]; break;
        case 2: p = T.p[2]; break;
        case 3: p = T.p[3]; break;
        case 4: p = T.p[4]; break;
        default: p = T.p[5]; break;
    }
    float mi = m[i], vi = v[i];
    const float np = adam_elem(p[j], g[i], mi, vi, s);
    p[j] = np;
    m[i] = mi;
    v[i] = vi;
    if (k == 1) T.b1p[j] = np;
    else if (k == 3) T.b2p[j] = np;
    else if (k == 4) T.W3p[j] = np;
}

__global__ void k_tr3_pad(const float *__restrict__ b1, int H1, int Hp1, const float *__restrict__ b2, int H2, int Hp2, const float *__restrict__ W3, int C,
                          float *__restrict__ b1p, float *__restrict__ b2p, float *__restrict__ W3p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Hp1) b1p[i] = i < H1 ? b1[i] : 0.f;
    if (i < Hp2) b2p[i] = i < H2 ? b2[i] : 0.f;
    if (i < Hp2 * C) W3p[i] = (i / C) < H2 ? W3[i] : 0.f;
}

struct lt_gcn3_trainer {
    const lt_graph *g = nullptr;
    int32_t n = 0, F = 0, H1 = 0, H2 = 0, C = 0, Hp1 = 0, Hp2 = 0;
    const float *X = nullptr;
    int64_t ldx = 0;
    const int32_t *labels = nullptr;
    float *P[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // W1, b1, W2, b2, W3, b3 (borrowed)
    int64_t off[6] = {0, 0, 0, 0, 0, 0};                                    // where each ends in grad / m / v
    double lr = 0, wd = 0, p = 0;
    uint64_t seed = 0;
    int64_t epoch = 0;
    int32_t kslice = 0;                       // split-K slicing of X W1 (the forward's)
    int32_t tn1_kslice = 0, tn1_splits = 0;   // dW1 = X^T dS1
    int32_t tn2_kslice = 0, tn2_splits = 0;   // dW2 = H1d^T dS2
    int32_t n_part = 0;                       // row blocks of k_tr_bwd_rows (layer 2)
    int32_t n_mblk = 0;                       // row blocks of k_tr3_dz_mfma
    float *S1 = nullptr, *H1d = nullptr, *dZ1 = nullptr, *dS1 = nullptr;                        // [n, Hp1]
    float *S2 = nullptr, *Z2 = nullptr, *H2d = nullptr, *dZ2 = nullptr, *dS2 = nullptr;         // [n, Hp2]
    float *S3 = nullptr, *Z3 = nullptr, *dZ3 = nullptr, *dS3 = nullptr;                         // [n, C]
    float *loss_r = nullptr;
    int32_t *corr_r = nullptr;
    float *b1p = nullptr, *b2p = nullptr, *W3p = nullptr;
    float *slabs = nullptr, *tn1_slabs = nullptr, *tn2_slabs = nullptr, *part = nullptr, *part1 = nullptr, *seg_part = nullptr;
    float *grad = nullptr, *m = nullptr, *v = nullptr;
    lt_val *val = nullptr;                    // lt_gcn3_trainer_attach_validation (owned)
};

static void free_trainer3(lt_gcn3_trainer *t) {
    if (!t) return;
    free_val(t->val);
    float *bufs[] = {t->S1, t->H1d, t->dZ1, t->dS1, t->S2, t->Z2, t->H2d, t->dZ2, t->dS2, t->S3, t->Z3, t->dZ3, t->dS3,
                     t->loss_r, t->b1p, t->b2p, t->W3p, t->slabs, t->tn1_slabs, t->tn2_slabs, t->part, t->part1,
                     t->seg_part, t->grad, t->m, t->v};
    for (float *b : bufs) (void)hipFree(b);
    (void)hipFree(t->corr_r);
    delete t;
}

extern "C" int lt_gcn3_trainer_create(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const int32_t *labels,
                                      int32_t H1, int32_t H2, int32_t C, float *W1, float *b1, float *W2, float *b2,
                                      float *W3, float *b3, double lr, double weight_decay, double dropout, uint64_t seed,
                                      void *stream, lt_gcn3_trainer **out) {
    LT_REQUIRE(out != nullptr, "lt_gcn3_trainer_create: out is NULL");
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "lt_gcn3_trainer_create: graph is NULL");
    LT_REQUIRE(F > 0 && H1 > 0 && H2 > 0 && C > 0, "lt_gcn3_trainer_create: F=%d H1=%d H2=%d C=%d must be positive", F, H1,
               H2, C);
    LT_REQUIRE(H1 <= LT_MAX_H && H2 <= LT_MAX_H && C <= LT_MAX_C,
               "lt_gcn3_trainer_create: H1=%d H2=%d C=%d (supported: H1, H2 <= %d, C <= %d)", H1, H2, C, LT_MAX_H, LT_MAX_C);
    LT_REQUIRE(X && labels && W1 && b1 && W2 && b2 && W3 && b3, "lt_gcn3_trainer_create: NULL tensor pointer");
    LT_REQUIRE(ldx >= F, "lt_gcn3_trainer_create: ldx=%lld < F=%d", (long long)ldx, F);
    LT_REQUIRE(dropout >= 0.0 && dropout <= 1.0, "lt_gcn3_trainer_create: dropout=%g outside [0, 1]", dropout);
    LT_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "lt_gcn3_trainer_create: lr=%g weight_decay=%g", lr, weight_decay);
    LT_REQUIRE(g->n > 0, "lt_gcn3_trainer_create: empty graph");
    lt_gcn3_trainer *t = new (std::nothrow) lt_gcn3_trainer();
    if (!t) return lt_set_error(LT_ERR_NOMEM, "lt_gcn3_trainer_create: out of host memory");
    const int n = g->n;
    t->g = g; t->n = n; t->F = F; t->H1 = H1; t->H2 = H2; t->C = C;
    t->Hp1 = lt_round_up(H1, 4); t->Hp2 = lt_round_up(H2, 4);
    t->X = X; t->ldx = ldx; t->labels = labels;
    float *ps[6] = {W1, b1, W2, b2, W3, b3};
    const int64_t sizes[6] = {(int64_t)F * H1, H1, (int64_t)H1 * H2, H2, (int64_t)H2 * C, C};
    int64_t end = 0;
    for (int k = 0; k < 6; ++k) { t->P[k] = ps[k]; end += sizes[k]; t->off[k] = end; }
    t->lr = lr; t->wd = weight_decay; t->p = dropout; t->seed = seed;
    t->kslice = lt_gemm_pick_kslice(n, H1, F);
    t->tn1_splits = tn_pick_splits(F, H1, n);
    t->tn1_kslice = lt_round_up((n + t->tn1_splits - 1) / t->tn1_splits, TN_BK);
    t->tn1_splits = (n + t->tn1_kslice - 1) / t->tn1_kslice;
    t->tn2_splits = tn_pick_splits(H1, H2, n);
    t->tn2_kslice = lt_round_up((n + t->tn2_splits - 1) / t->tn2_splits, TN_BK);
    t->tn2_splits = (n + t->tn2_kslice - 1) / t->tn2_kslice;
    t->n_part = (n + TR_ROWS_PER_BLOCK - 1) / TR_ROWS_PER_BLOCK;
    t->n_mblk = (n + TN_BM - 1) / TN_BM;
    const size_t nh1 = (size_t)n * t->Hp1 * sizeof(float), nh2 = (size_t)n * t->Hp2 * sizeof(float);
    const size_t nc = (size_t)n * C * sizeof(float), np_bytes = (size_t)end * sizeof(float);
    const int hpm = t->Hp1 > t->Hp2 ? t->Hp1 : t->Hp2;
    hipStream_t st = (hipStream_t)stream;
#define T_HIP(call)                                                                         \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            free_trainer3(t);                                                               \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)
    float **h1bufs[] = {&t->S1, &t->H1d, &t->dZ1, &t->dS1};
    for (float **b : h1bufs) T_HIP(hipMalloc((void **)b, nh1));
    float **h2bufs[] = {&t->S2, &t->Z2, &t->H2d, &t->dZ2, &t->dS2};
    for (float **b : h2bufs) T_HIP(hipMalloc((void **)b, nh2));
    float **cbufs[] = {&t->S3, &t->Z3, &t->dZ3, &t->dS3};
    for (float **b : cbufs) T_HIP(hipMalloc((void **)b, nc));
    T_HIP(hipMalloc((void **)&t->loss_r, (size_t)n * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->corr_r, (size_t)n * sizeof(int32_t)));
    T_HIP(hipMalloc((void **)&t->b1p, (size_t)t->Hp1 * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->b2p, (size_t)t->Hp2 * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->W3p, (size_t)t->Hp2 * C * sizeof(float)));
    const size_t sb = lt_gemm_splitk_slab_bytes(n, H1, F, t->kslice);
    if (sb) T_HIP(hipMalloc((void **)&t->slabs, sb));
    if (t->tn1_splits > 1) T_HIP(hipMalloc((void **)&t->tn1_slabs, (size_t)t->tn1_splits * F * H1 * sizeof(float)));
    if (t->tn2_splits > 1) T_HIP(hipMalloc((void **)&t->tn2_slabs, (size_t)t->tn2_splits * H1 * H2 * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->part, (size_t)t->n_part * ((size_t)H2 + (size_t)H2 * C) * sizeof(float)));
    T_HIP(hipMalloc((void **)&t->part1, (size_t)t->n_mblk * H1 * sizeof(float)));
    if (g->p_n_seg > 0) T_HIP(hipMalloc((void **)&t->seg_part, (size_t)g->p_n_seg * hpm * sizeof(float)));
    float **pbufs[] = {&t->grad, &t->m, &t->v};
    for (float **b : pbufs) T_HIP(hipMalloc((void **)b, np_bytes));
    // pad columns of S1 / S2 (the GEMMs write H of them) and of dZ1 (its product writes H1 of them) stay zero
    T_HIP(hipMemsetAsync(t->S1, 0, nh1, st));
    T_HIP(hipMemsetAsync(t->S2, 0, nh2, st));
    T_HIP(hipMemsetAsync(t->dZ1, 0, nh1, st));
    T_HIP(hipMemsetAsync(t->m, 0, np_bytes, st));
    T_HIP(hipMemsetAsync(t->v, 0, np_bytes, st));
#undef T_HIP
    *out = t;
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_destroy(lt_gcn3_trainer *t) {
    free_trainer3(t);
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_epoch(const lt_gcn3_trainer *t, int64_t *epoch) {
    LT_REQUIRE(t != nullptr && epoch != nullptr, "lt_gcn3_trainer_epoch: NULL argument");
    *epoch = t->epoch;
    return LT_OK;
}

static int launch_tn(const float *A, long lda, const float *B, long ldb, float *C, int M, int N, int K, int kslice, int splits,
                     float *slabs, hipStream_t st) {
    const bool split = splits > 1;
    dim3 grid((unsigned)((M + TN_BM - 1) / TN_BM), (unsigned)((N + TN_BN - 1) / TN_BN), (unsigned)splits);
    hipLaunchKernelGGL(k_gemm_tn_mfma, grid, dim3(256), 0, st, A, lda, B, ldb, split ? slabs : C, (long)N, M, N, K, kslice,
                       (long)M * N);
    LT_CHECK_LAUNCH();
    if (split) return lt_launch_sum_slabs(slabs, (long)M * N, splits, M, N, (long)N, C, (long)N, st);
    return LT_OK;
}

static int run_epoch3(lt_gcn3_trainer *t, float *record, hipStream_t st) {
    const lt_graph *g = t->g;
    const int n = t->n, F = t->F, H1 = t->H1, H2 = t->H2, C = t->C, Hp1 = t->Hp1, Hp2 = t->Hp2;
    const int lpr1 = lt_lpr_for(Hp1), lpr2 = lt_lpr_for(Hp2), cp = lt_cp_for(C);
    const int rpb1 = (TR_BLOCK / 64) * (64 / lpr1), rpb2 = (TR_BLOCK / 64) * (64 / lpr2);
    float *W1 = t->P[0], *W2 = t->P[2], *b3 = t->P[5];
    float *gW1 = t->grad, *gb1 = t->grad + t->off[0], *gW2 = t->grad + t->off[1], *gb2 = t->grad + t->off[2],
          *gb3 = t->grad + t->off[4];
    int rc;
    lt_drop_args d;
    d.on = t->p > 0.0;
    d.thresh = (uint64_t)floor(t->p * 4294967296.0);
    d.scale = t->p < 1.0 ? (float)(1.0 / (1.0 - t->p)) : 0.f;
    d.epoch = (uint32_t)t->epoch;
    d.seed = t->seed;
    const float scale = t->p > 0.0 ? d.scale : 1.f;
    // layer 1
    if (t->slabs)
        rc = lt_launch_gemm_splitk(t->X, t->ldx, W1, H1, t->S1, Hp1, n, H1, F, t->kslice, t->slabs, st);
    else
        rc = lt_launch_gemm(t->X, t->ldx, W1, H1, t->S1, Hp1, n, H1, F, st);
    if (rc) return rc;
    {
        const int have_long = g->p_n_long > 0 ? 1 : 0;
        const unsigned seg_blocks = have_long ? rows_grid(g->p_n_seg, rpb1) : 0u;
        d.layer = 0;
        LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k_tr3_layer1<LPR_>), dim3(rows_grid(n, rpb1) + seg_blocks), dim3(TR_BLOCK), 0,
                                                 st, n, g->rowptr, g->col, g->val, t->S1, Hp1, H1, t->b1p, d, t->H1d, have_long,
                                                 (int)seg_blocks, g->p_n_seg, g->p_seg_long, g->p_seg_begin, g->p_long_row,
                                                 t->seg_part));
        LT_CHECK_LAUNCH();
        if (have_long) {
            LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k_tr3_layer1_long<LPR_>), dim3(rows_grid(g->p_n_long, rpb1)),
                                                     dim3(TR_BLOCK), 0, st, g->p_n_long, g->p_long_row, g->p_long_segptr,
                                                     t->seg_part, Hp1, H1, d, t->H1d));
            LT_CHECK_LAUNCH();
        }
    }
    // layers 2 and 3: the 2-layer trainer's chain
    rc = lt_launch_gemm(t->H1d, Hp1, W2, H2, t->S2, Hp2, n, H2, H1, st);
    if (rc) return rc;
    rc = lt_launch_layer1(g, t->S2, Hp2, t->b2p, t->W3p, C, t->Z2, t->S3, st, t->seg_part);
    if (rc) return rc;
    d.layer = 1;
    LT_DISPATCH_LPR(lpr2, LT_DISPATCH_CP(cp,
        hipLaunchKernelGGL((k_tr_dropout<LPR_, CP_>), dim3(rows_grid(n, rpb2)), dim3(TR_BLOCK), 0, st, n, t->Z2, Hp2, H2, t->W3p,
                           C, d, t->H2d, t->S3)));
    LT_CHECK_LAUNCH();
    rc = lt_launch_layer2(g, t->S3, C, b3, t->Z3, st);
    if (rc) return rc;
    // loss head
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce<CP_>), dim3(rows_grid(n, TR_BLOCK)), dim3(TR_BLOCK), 0, st, n, t->Z3, C,
                                          t->labels, 1.0f / (float)n, t->loss_r, t->corr_r, t->dZ3));
    LT_CHECK_LAUNCH();
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce_reduce<CP_>), dim3(1), dim3(TR_BLOCK), 0, st, n, C, t->loss_r, t->corr_r,
                                          t->dZ3, record, gb3));
    LT_CHECK_LAUNCH();
    // backward through layer 3
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_spmm_t_narrow<CP_>), dim3(rows_grid(n, TR_BLOCK / LT_L2_LANES)),
                                          dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZ3, C, t->dS3));
    LT_CHECK_LAUNCH();
    int W = 1;
    while (W < Hp2) W <<= 1;
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_bwd_rows<CP_>), dim3((unsigned)t->n_part), dim3(TR_BLOCK), 0, st, n, H2, Hp2, W,
                                          C, t->H2d, t->dS3, t->W3p, scale, t->dZ2, t->part));
    LT_CHECK_LAUNCH();
    const int L = H2 + H2 * C;   // db2 | dW3: adjacent in the gradient buffer
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((L + 63) / 64)), dim3(TR_BLOCK), 0, st, t->part, t->n_part, L, gb2);
    LT_CHECK_LAUNCH();
    // backward through layer 2
    LT_DISPATCH_LPR(lpr2, hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, rpb2)), dim3(TR_BLOCK), 0, st, n,
                                             g->tptr, g->trow, g->tval, t->dZ2, Hp2, t->dS2));
    LT_CHECK_LAUNCH();
    rc = launch_tn(t->H1d, (long)Hp1, t->dS2, (long)Hp2, gW2, H1, H2, n, t->tn2_kslice, t->tn2_splits, t->tn2_slabs, st);
    if (rc) return rc;
    {
        dim3 grid((unsigned)t->n_mblk, (unsigned)((H1 + TN_BN - 1) / TN_BN));
        hipLaunchKernelGGL(k_tr3_dz_mfma, grid, dim3(256), 0, st, t->dS2, (long)Hp2, W2, (long)H2, t->H1d, t->dZ1, (long)Hp1, n,
                           H1, H2, scale, t->part1);
        LT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((H1 + 63) / 64)), dim3(TR_BLOCK), 0, st, t->part1, t->n_mblk, H1, gb1);
    LT_CHECK_LAUNCH();
    // backward through layer 1
    LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, rpb1)), dim3(TR_BLOCK), 0, st, n,
                                             g->tptr, g->trow, g->tval, t->dZ1, Hp1, t->dS1));
    LT_CHECK_LAUNCH();
    rc = launch_tn(t->X, (long)t->ldx, t->dS1, (long)Hp1, gW1, F, H1, n, t->tn1_kslice, t->tn1_splits, t->tn1_slabs, st);
    if (rc) return rc;
    // Adam
    const int64_t step = t->epoch + 1;
    lt_tr3_tensors T;
    for (int k = 0; k < 6; ++k) { T.p[k] = t->P[k]; T.o[k] = t->off[k]; }
    T.b1p = t->b1p; T.b2p = t->b2p; T.W3p = t->W3p;
    hipLaunchKernelGGL(k_tr3_adam, dim3((unsigned)((t->off[5] + 255) / 256)), dim3(256), 0, st, T, t->grad, t->m, t->v,
                       adam_scalars(step, t->lr, 0.9, 0.999, 1e-8, t->wd));
    LT_CHECK_LAUNCH();
    t->epoch = step;
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_run(lt_gcn3_trainer *t, int32_t n_epochs, float *record, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_run: trainer is NULL");
    LT_REQUIRE(n_epochs >= 0, "lt_gcn3_trainer_run: n_epochs=%d", n_epochs);
    if (n_epochs == 0) return LT_OK;
    LT_REQUIRE(record != nullptr, "lt_gcn3_trainer_run: record is NULL");
    LT_REQUIRE(t->epoch + n_epochs <= (int64_t)UINT32_MAX, "lt_gcn3_trainer_run: epoch counter would pass 2^32");
    hipStream_t st = (hipStream_t)stream;
    // the borrowed parameters may have changed since the last run: the mirrors from them (Adam keeps them current after that)
    const int mx = t->Hp1 > t->Hp2 * t->C ? t->Hp1 : t->Hp2 * t->C;
    hipLaunchKernelGGL(k_tr3_pad, dim3((mx + 255) / 256), dim3(256), 0, st, t->P[1], t->H1, t->Hp1, t->P[3], t->H2, t->Hp2,
                       t->P[4], t->C, t->b1p, t->b2p, t->W3p);
    LT_CHECK_LAUNCH();
    for (int32_t j = 0; j < n_epochs; ++j) {
        const int rc = run_epoch3(t, record + 2 * (size_t)j, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_grads(const lt_gcn3_trainer *t, float *dW1, float *db1, float *dW2, float *db2, float *dW3,
                                     float *db3, void *stream) {
    LT_REQUIRE(t != nullptr && dW1 && db1 && dW2 && db2 && dW3 && db3, "lt_gcn3_trainer_grads: NULL argument");
    float *dst[6] = {dW1, db1, dW2, db2, dW3, db3};
    for (int k = 0; k < 6; ++k) {
        const int64_t b = k ? t->off[k - 1] : 0;
        LT_HIP(hipMemcpyAsync(dst[k], t->grad + b, (size_t)(t->off[k] - b) * sizeof(float), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
    }
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_logits(const lt_gcn3_trainer *t, float *Z3, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr && Z3 != nullptr, "lt_gcn3_trainer_logits: NULL argument");
    LT_REQUIRE(ldz >= t->C, "lt_gcn3_trainer_logits: ldz=%lld < C=%d", (long long)ldz, t->C);
    LT_HIP(hipMemcpy2DAsync(Z3, (size_t)ldz * sizeof(float), t->Z3, (size_t)t->C * sizeof(float), (size_t)t->C * sizeof(float),
                            (size_t)t->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_hidden(const lt_gcn3_trainer *t, int32_t layer, float *dst, int64_t ld, void *stream) {
    LT_REQUIRE(t != nullptr && dst != nullptr, "lt_gcn3_trainer_hidden: NULL argument");
    LT_REQUIRE(layer == 1 || layer == 2, "lt_gcn3_trainer_hidden: layer=%d, must be 1 or 2", layer);
    const int H = layer == 1 ? t->H1 : t->H2, Hp = layer == 1 ? t->Hp1 : t->Hp2;
    LT_REQUIRE(ld >= H, "lt_gcn3_trainer_hidden: ld=%lld < H%d=%d", (long long)ld, layer, H);
    LT_HIP(hipMemcpy2DAsync(dst, (size_t)ld * sizeof(float), layer == 1 ? t->H1d : t->H2d, (size_t)Hp * sizeof(float),
                            (size_t)H * sizeof(float), (size_t)t->n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

// ============================================================================================
// Validation: the standalone head and state update, and per-epoch validation inside both trainers.
// ============================================================================================
extern "C" size_t lt_eval_head_workspace_bytes(int32_t n, int32_t C) {
    if (n <= 0 || C <= 0 || C > LT_MAX_C) return 0;
    return val_head_bytes(n, C);
}

extern "C" int lt_eval_head(const float *Z, int64_t ldz, const int32_t *labels, int32_t n, int32_t C, float *loss,
                            int32_t *confusion, void *workspace, size_t workspace_bytes, void *stream) {
    LT_REQUIRE(n > 0, "lt_eval_head: n=%d, must be positive", n);
    LT_REQUIRE(C > 0 && C <= LT_MAX_C, "lt_eval_head: C=%d (supported: 1 .. %d)", C, LT_MAX_C);
    LT_REQUIRE(Z && labels && loss && confusion, "lt_eval_head: NULL pointer");
    LT_REQUIRE(ldz >= C, "lt_eval_head: ldz=%lld < C=%d", (long long)ldz, C);
    if (!workspace || workspace_bytes < val_head_bytes(n, C) || ((uintptr_t)workspace % sizeof(float)))
        return lt_set_error(LT_ERR_WORKSPACE, "lt_eval_head: workspace needs %zu bytes, 4-byte aligned", val_head_bytes(n, C));
    const int n_blk = (n + TR_BLOCK - 1) / TR_BLOCK;
    float *part_loss = (float *)workspace;
    return launch_val_head(Z, (long)ldz, labels, n, C, part_loss, (int32_t *)(part_loss + n_blk), loss, confusion, nullptr, 0, 0,
                           (hipStream_t)stream);
}

extern "C" size_t lt_eval_head_rows_workspace_bytes(int32_t m, int32_t C) {
    if (m <= 0 || C <= 0 || C > LT_MAX_C) return 0;
    return val_head_bytes(m, C);
}

extern "C" int lt_eval_head_rows(const float *Z, int64_t ldz, const int32_t *labels, int32_t n, int32_t C, const int32_t *rows,
                                 int32_t m, float *loss, int32_t *confusion, int32_t *n_bad, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    LT_REQUIRE(m > 0, "lt_eval_head_rows: m=%d, must be positive", m);
    LT_REQUIRE(n > 0, "lt_eval_head_rows: n=%d, must be positive", n);
    LT_REQUIRE(C > 0 && C <= LT_MAX_C, "lt_eval_head_rows: C=%d (supported: 1 .. %d)", C, LT_MAX_C);
    LT_REQUIRE(Z && labels && rows && loss && confusion, "lt_eval_head_rows: NULL pointer");
    LT_REQUIRE(ldz >= C, "lt_eval_head_rows: ldz=%lld < C=%d", (long long)ldz, C);
    if (!workspace || workspace_bytes < val_head_bytes(m, C) || ((uintptr_t)workspace % sizeof(float)))
        return lt_set_error(LT_ERR_WORKSPACE, "lt_eval_head_rows: workspace needs %zu bytes, 4-byte aligned",
                            val_head_bytes(m, C));
    hipStream_t st = (hipStream_t)stream;
    if (n_bad) LT_HIP(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
    const int n_blk = (m + TR_BLOCK - 1) / TR_BLOCK;
    float *part_loss = (float *)workspace;
    return launch_val_head_rows(Z, (long)ldz, labels, n, C, rows, m, part_loss, (int32_t *)(part_loss + n_blk), loss, confusion,
                                n_bad, nullptr, 0, 0, st);
}

extern "C" int lt_early_stop_reset(int32_t *state, void *stream) {
    LT_REQUIRE(state != nullptr, "lt_early_stop_reset: state is NULL");
    hipLaunchKernelGGL(k_val_state_reset, dim3(1), dim3(64), 0, (hipStream_t)stream, state);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

extern "C" int lt_early_stop_update(const float *loss, int32_t patience, int32_t epoch, int32_t *state, void *stream) {
    LT_REQUIRE(loss != nullptr && state != nullptr, "lt_early_stop_update: NULL pointer");
    LT_REQUIRE(patience >= 0, "lt_early_stop_update: patience=%d, must be >= 0 (0: never stop)", patience);
    LT_REQUIRE(epoch >= 0, "lt_early_stop_update: epoch=%d, must be >= 0", epoch);
    hipLaunchKernelGGL(k_val_state, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, state, patience, epoch);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// the device a pointer's memory lives on, -1 for anything that is not device memory
static int ptr_device(const void *p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return at.type == hipMemoryTypeDevice ? at.device : -1;
}

// Everything lt_gcn*_trainer_attach_validation checks and allocates.  Hp2 = 0: the 2-layer model.
static int val_attach(const char *who, lt_val **slot, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                      const int32_t *labels2, int32_t keep_best, int32_t patience, const float *X, int F, int H1, int Hp1,
                      int Hp2, int C, int64_t n_param, hipStream_t st, int with_rows = 0, const int32_t *rows = nullptr,
                      int32_t m = 0) {
    LT_REQUIRE(*slot == nullptr, "%s: validation is already attached to this trainer", who);
    LT_REQUIRE(g2 != nullptr && X2 != nullptr && labels2 != nullptr, "%s: NULL argument", who);
    LT_REQUIRE(g2->n > 0, "%s: empty graph", who);
    LT_REQUIRE(n2 == g2->n, "%s: X2 has %d rows, the graph %d nodes", who, n2, g2->n);
    LT_REQUIRE(ldx2 >= F, "%s: ldx2=%lld < F=%d", who, (long long)ldx2, F);
    LT_REQUIRE(keep_best == 0 || keep_best == 1, "%s: keep_best=%d, must be 0 or 1", who, keep_best);
    LT_REQUIRE(patience >= 0, "%s: patience=%d, must be >= 0 (0: never stop)", who, patience);
    const int dev = ptr_device(X);
    LT_REQUIRE(dev >= 0 && ptr_device(X2) == dev && ptr_device(g2->rowptr) == dev && ptr_device(labels2) == dev,
               "%s: the validation graph, X2 and labels2 must live on the trainer's device (%d)", who, dev);
    if (with_rows) {
        LT_REQUIRE(rows != nullptr, "%s: rows is NULL", who);
        LT_REQUIRE(m > 0, "%s: m=%d, must be positive", who, m);
        LT_REQUIRE(ptr_device(rows) == dev, "%s: rows must live on the trainer's device (%d)", who, dev);
    }
    {
        int32_t *host = new (std::nothrow) int32_t[(size_t)n2];
        if (!host) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
        hipError_t e = hipMemcpyAsync(host, labels2, (size_t)n2 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        int bad = -1;
        if (e == hipSuccess)
            for (int i = 0; i < n2 && bad < 0; ++i)
                if (host[i] < 0 || host[i] >= C) bad = i;
        const int bad_label = bad >= 0 ? host[bad] : 0;
        delete[] host;
        if (e != hipSuccess) return lt_set_error(LT_ERR_HIP, "%s: reading labels2 failed: %s", who, hipGetErrorString(e));
        LT_REQUIRE(bad < 0, "%s: labels2[%d]=%d outside [0, %d)", who, bad, bad_label, C);
    }
    if (with_rows) {      // the list is read back once and checked here: the head then never meets an id outside [0, n2)
        int32_t *host = new (std::nothrow) int32_t[(size_t)m];
        if (!host) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
        hipError_t e = hipMemcpyAsync(host, rows, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        int bad = -1;
        if (e == hipSuccess)
            for (int i = 0; i < m && bad < 0; ++i)
                if (host[i] < 0 || host[i] >= n2) bad = i;
        const int bad_row = bad >= 0 ? host[bad] : 0;
        delete[] host;
        if (e != hipSuccess) return lt_set_error(LT_ERR_HIP, "%s: reading rows failed: %s", who, hipGetErrorString(e));
        LT_REQUIRE(bad < 0, "%s: rows[%d]=%d outside [0, %d)", who, bad, bad_row, n2);
    }
    lt_val *v = new (std::nothrow) lt_val();
    if (!v) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
    v->g = g2; v->n = n2; v->X = X2; v->ldx = ldx2; v->labels = labels2;
    v->keep_best = keep_best; v->patience = patience;
    v->kslice = lt_gemm_pick_kslice(n2, H1, F);
    v->rows = with_rows ? rows : nullptr;
    v->m = with_rows ? m : 0;
    v->n_blk = ((with_rows ? m : n2) + TR_BLOCK - 1) / TR_BLOCK;
    const size_t nh1 = (size_t)n2 * Hp1 * sizeof(float), nh2 = (size_t)n2 * Hp2 * sizeof(float);
    const size_t nc = (size_t)n2 * C * sizeof(float);
    const int hpm = Hp1 > Hp2 ? Hp1 : Hp2;
#define V_HIP(call)                                                                         \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            free_val(v);                                                                    \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)
    V_HIP(hipMalloc((void **)&v->S1, nh1));
    V_HIP(hipMemsetAsync(v->S1, 0, nh1, st));      // the GEMM writes H of the Hp columns
    if (Hp2 == 0) {
        V_HIP(hipMalloc((void **)&v->Z1, nh1));
    } else {
        V_HIP(hipMalloc((void **)&v->H1, nh1));
        V_HIP(hipMalloc((void **)&v->S2, nh2));
        V_HIP(hipMalloc((void **)&v->Z2, nh2));
        V_HIP(hipMemsetAsync(v->S2, 0, nh2, st));
    }
    V_HIP(hipMalloc((void **)&v->Sc, nc));
    V_HIP(hipMalloc((void **)&v->Z, nc));
    const size_t sb = lt_gemm_splitk_slab_bytes(n2, H1, F, v->kslice);
    if (sb) V_HIP(hipMalloc((void **)&v->slabs, sb));
    if (g2->p_n_seg > 0) V_HIP(hipMalloc((void **)&v->seg_part, (size_t)g2->p_n_seg * hpm * sizeof(float)));
    V_HIP(hipMalloc((void **)&v->part_loss, (size_t)v->n_blk * sizeof(float)));
    V_HIP(hipMalloc((void **)&v->part_cnt, (size_t)v->n_blk * C * C * sizeof(int32_t)));
    V_HIP(hipMalloc((void **)&v->state, VAL_STATE_WORDS * sizeof(int32_t)));
    if (keep_best) V_HIP(hipMalloc((void **)&v->snap, (size_t)n_param * sizeof(float)));
#undef V_HIP
    hipLaunchKernelGGL(k_val_state_reset, dim3(1), dim3(64), 0, st, v->state);
    {
        hipError_t e_ = hipGetLastError();
        if (e_ != hipSuccess) {
            free_val(v);
            return lt_set_error(LT_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e_));
        }
    }
    *slot = v;
    return LT_OK;
}

// head, state and snapshot behind a validation forward; e = the epoch just trained (0-based, since creation)
static int val_finish_epoch(lt_val *v, int C, const lt_snap_segs &T, int64_t e, float *val_loss, int32_t *val_counts,
                            hipStream_t st) {
    int rc = v->rows ? launch_val_head_rows(v->Z, (long)C, v->labels, v->n, C, v->rows, v->m, v->part_loss, v->part_cnt, val_loss,
                                            val_counts, nullptr, v->state, v->patience, (int)e, st)
                     : launch_val_head(v->Z, (long)C, v->labels, v->n, C, v->part_loss, v->part_cnt, val_loss, val_counts,
                                       v->state, v->patience, (int)e, st);
    if (rc) return rc;
    if (v->keep_best) return launch_snapshot(T, v->snap, v->state + VS_IMPROVED, 0, st);
    return LT_OK;
}

static int val_read_state(const char *who, const lt_val *v, int32_t *state_host, hipStream_t st) {
    LT_REQUIRE(v != nullptr, "%s: no validation attached", who);
    LT_REQUIRE(state_host != nullptr, "%s: state is NULL", who);
    LT_HIP(hipMemcpyAsync(state_host, v->state, VAL_STATE_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    return LT_OK;
}

static int val_copy_logits(const char *who, const lt_val *v, int C, float *Z, int64_t ldz, hipStream_t st) {
    LT_REQUIRE(v != nullptr, "%s: no validation attached", who);
    LT_REQUIRE(Z != nullptr, "%s: Z is NULL", who);
    LT_REQUIRE(ldz >= C, "%s: ldz=%lld < C=%d", who, (long long)ldz, C);
    LT_HIP(hipMemcpy2DAsync(Z, (size_t)ldz * sizeof(float), v->Z, (size_t)C * sizeof(float), (size_t)C * sizeof(float),
                            (size_t)v->n, hipMemcpyDeviceToDevice, st));
    return LT_OK;
}

// ---- the 2-layer trainer ----
static lt_snap_segs snap_segs2(const lt_gcn2_trainer *t) {
    lt_snap_segs T;
    const int64_t o1 = (int64_t)t->F * t->H, o2 = o1 + t->H, o3 = o2 + (int64_t)t->H * t->C;
    float *ps[6] = {t->W1, t->b1, t->W2, t->b2, nullptr, nullptr};
    const int64_t os[6] = {o1, o2, o3, t->n_param, t->n_param, t->n_param};
    for (int k = 0; k < 6; ++k) { T.p[k] = ps[k]; T.o[k] = os[k]; }
    return T;
}

// the forward of run_epoch on the validation graph, dropout off: lt_gcn2_forward's launches at n2 (its logits' bits)
static int val_forward2(lt_gcn2_trainer *t, hipStream_t st) {
    lt_val *v = t->val;
    const int F = t->F, H = t->H, C = t->C, Hp = t->Hp;
    int rc;
    if (v->slabs)
        rc = lt_launch_gemm_splitk(v->X, v->ldx, t->W1, H, v->S1, Hp, v->n, H, F, v->kslice, v->slabs, st);
    else
        rc = lt_launch_gemm(v->X, v->ldx, t->W1, H, v->S1, Hp, v->n, H, F, st);
    if (rc) return rc;
    rc = lt_launch_layer1(v->g, v->S1, Hp, t->b1p, t->W2p, C, lt_tiled_wanted(v->g, Hp) ? v->Z1 : nullptr, v->Sc, st,
                          v->seg_part);
    if (rc) return rc;
    return lt_launch_layer2(v->g, v->Sc, C, t->b2, v->Z, st);
}

extern "C" int lt_gcn2_trainer_attach_validation(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                 int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                 void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_attach_validation: trainer is NULL");
    return val_attach("lt_gcn2_trainer_attach_validation", &t->val, g2, X2, ldx2, n2, labels2, keep_best, patience, t->X, t->F,
                      t->H, t->Hp, 0, t->C, t->n_param, (hipStream_t)stream);
}

extern "C" int lt_gcn2_trainer_attach_validation_rows(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                      const int32_t *rows, int32_t m, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_attach_validation_rows: trainer is NULL");
    return val_attach("lt_gcn2_trainer_attach_validation_rows", &t->val, g2, X2, ldx2, n2, labels2, keep_best, patience, t->X,
                      t->F, t->H, t->Hp, 0, t->C, t->n_param, (hipStream_t)stream, 1, rows, m);
}

extern "C" int lt_gcn2_trainer_run_validated(lt_gcn2_trainer *t, int32_t n_epochs, float *record, float *val_loss,
                                             int32_t *val_counts, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_run_validated: trainer is NULL");
    LT_REQUIRE(t->val != nullptr, "lt_gcn2_trainer_run_validated: no validation attached");
    LT_REQUIRE(n_epochs >= 0, "lt_gcn2_trainer_run_validated: n_epochs=%d", n_epochs);
    if (n_epochs == 0) return LT_OK;
    LT_REQUIRE(record && val_loss && val_counts, "lt_gcn2_trainer_run_validated: NULL output");
    LT_REQUIRE(t->epoch + n_epochs <= (int64_t)INT32_MAX, "lt_gcn2_trainer_run_validated: epoch counter would pass 2^31");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_tr_pad, dim3((t->Hp * (t->C + 1) + 255) / 256), dim3(256), 0, st, t->b1, t->W2, t->H, t->Hp, t->C,
                       t->b1p, t->W2p);
    LT_CHECK_LAUNCH();
    const lt_snap_segs T = snap_segs2(t);
    const size_t cc = (size_t)t->C * t->C;
    for (int32_t j = 0; j < n_epochs; ++j) {
        const int64_t e = t->epoch;
        int rc = run_epoch(t, record + 2 * (size_t)j, st);
        if (rc) return rc;
        rc = val_forward2(t, st);
        if (rc) return rc;
        rc = val_finish_epoch(t->val, t->C, T, e, val_loss + j, val_counts + cc * (size_t)j, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_val_state(const lt_gcn2_trainer *t, int32_t *state, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_val_state: trainer is NULL");
    return val_read_state("lt_gcn2_trainer_val_state", t->val, state, (hipStream_t)stream);
}

extern "C" int lt_gcn2_trainer_restore_best(lt_gcn2_trainer *t, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_restore_best: trainer is NULL");
    LT_REQUIRE(t->val != nullptr && t->val->keep_best, "lt_gcn2_trainer_restore_best: no validation with keep_best attached");
    return launch_snapshot(snap_segs2(t), t->val->snap, t->val->state + VS_SEEN, 1, (hipStream_t)stream);
}

extern "C" int lt_gcn2_trainer_val_logits(const lt_gcn2_trainer *t, float *Z, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn2_trainer_val_logits: trainer is NULL");
    return val_copy_logits("lt_gcn2_trainer_val_logits", t->val, t->C, Z, ldz, (hipStream_t)stream);
}

// ---- the 3-layer trainer ----
static lt_snap_segs snap_segs3(const lt_gcn3_trainer *t) {
    lt_snap_segs T;
    for (int k = 0; k < 6; ++k) { T.p[k] = t->P[k]; T.o[k] = t->off[k]; }
    return T;
}

// the forward of run_epoch3 on the validation graph, dropout off (k_tr_dropout with no mask only repeats layer 1's S3 bits,
// so it is not launched)
static int val_forward3(lt_gcn3_trainer *t, hipStream_t st) {
    lt_val *v = t->val;
    const lt_graph *g = v->g;
    const int n = v->n, F = t->F, H1 = t->H1, H2 = t->H2, C = t->C, Hp1 = t->Hp1, Hp2 = t->Hp2;
    const int lpr1 = lt_lpr_for(Hp1);
    const int rpb1 = (TR_BLOCK / 64) * (64 / lpr1);
    int rc;
    if (v->slabs)
        rc = lt_launch_gemm_splitk(v->X, v->ldx, t->P[0], H1, v->S1, Hp1, n, H1, F, v->kslice, v->slabs, st);
    else
        rc = lt_launch_gemm(v->X, v->ldx, t->P[0], H1, v->S1, Hp1, n, H1, F, st);
    if (rc) return rc;
    lt_drop_args d;
    d.on = 0; d.thresh = 0; d.scale = 1.f; d.epoch = 0; d.seed = 0; d.layer = 0;
    const int have_long = g->p_n_long > 0 ? 1 : 0;
    const unsigned seg_blocks = have_long ? rows_grid(g->p_n_seg, rpb1) : 0u;
    LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k_tr3_layer1<LPR_>), dim3(rows_grid(n, rpb1) + seg_blocks), dim3(TR_BLOCK), 0, st,
                                             n, g->rowptr, g->col, g->val, v->S1, Hp1, H1, t->b1p, d, v->H1, have_long,
                                             (int)seg_blocks, g->p_n_seg, g->p_seg_long, g->p_seg_begin, g->p_long_row,
                                             v->seg_part));
    LT_CHECK_LAUNCH();
    if (have_long) {
        LT_DISPATCH_LPR(lpr1, hipLaunchKernelGGL((k_tr3_layer1_long<LPR_>), dim3(rows_grid(g->p_n_long, rpb1)), dim3(TR_BLOCK),
                                                 0, st, g->p_n_long, g->p_long_row, g->p_long_segptr, v->seg_part, Hp1, H1, d,
                                                 v->H1));
        LT_CHECK_LAUNCH();
    }
    rc = lt_launch_gemm(v->H1, Hp1, t->P[2], H2, v->S2, Hp2, n, H2, H1, st);
    if (rc) return rc;
    rc = lt_launch_layer1(g, v->S2, Hp2, t->b2p, t->W3p, C, v->Z2, v->Sc, st, v->seg_part);
    if (rc) return rc;
    return lt_launch_layer2(g, v->Sc, C, t->P[5], v->Z, st);
}

extern "C" int lt_gcn3_trainer_attach_validation(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                 int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                 void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_attach_validation: trainer is NULL");
    return val_attach("lt_gcn3_trainer_attach_validation", &t->val, g2, X2, ldx2, n2, labels2, keep_best, patience, t->X, t->F,
                      t->H1, t->Hp1, t->Hp2, t->C, t->off[5], (hipStream_t)stream);
}

extern "C" int lt_gcn3_trainer_attach_validation_rows(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                      const int32_t *rows, int32_t m, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_attach_validation_rows: trainer is NULL");
    return val_attach("lt_gcn3_trainer_attach_validation_rows", &t->val, g2, X2, ldx2, n2, labels2, keep_best, patience, t->X,
                      t->F, t->H1, t->Hp1, t->Hp2, t->C, t->off[5], (hipStream_t)stream, 1, rows, m);
}

extern "C" int lt_gcn3_trainer_run_validated(lt_gcn3_trainer *t, int32_t n_epochs, float *record, float *val_loss,
                                             int32_t *val_counts, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_run_validated: trainer is NULL");
    LT_REQUIRE(t->val != nullptr, "lt_gcn3_trainer_run_validated: no validation attached");
    LT_REQUIRE(n_epochs >= 0, "lt_gcn3_trainer_run_validated: n_epochs=%d", n_epochs);
    if (n_epochs == 0) return LT_OK;
    LT_REQUIRE(record && val_loss && val_counts, "lt_gcn3_trainer_run_validated: NULL output");
    LT_REQUIRE(t->epoch + n_epochs <= (int64_t)INT32_MAX, "lt_gcn3_trainer_run_validated: epoch counter would pass 2^31");
    hipStream_t st = (hipStream_t)stream;
    const int mx = t->Hp1 > t->Hp2 * t->C ? t->Hp1 : t->Hp2 * t->C;
    hipLaunchKernelGGL(k_tr3_pad, dim3((mx + 255) / 256), dim3(256), 0, st, t->P[1], t->H1, t->Hp1, t->P[3], t->H2, t->Hp2,
                       t->P[4], t->C, t->b1p, t->b2p, t->W3p);
    LT_CHECK_LAUNCH();
    const lt_snap_segs T = snap_segs3(t);
    const size_t cc = (size_t)t->C * t->C;
    for (int32_t j = 0; j < n_epochs; ++j) {
        const int64_t e = t->epoch;
        int rc = run_epoch3(t, record + 2 * (size_t)j, st);
        if (rc) return rc;
        rc = val_forward3(t, st);
        if (rc) return rc;
        rc = val_finish_epoch(t->val, t->C, T, e, val_loss + j, val_counts + cc * (size_t)j, st);
        if (rc) return rc;
    }
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_val_state(const lt_gcn3_trainer *t, int32_t *state, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_val_state: trainer is NULL");
    return val_read_state("lt_gcn3_trainer_val_state", t->val, state, (hipStream_t)stream);
}

extern "C" int lt_gcn3_trainer_restore_best(lt_gcn3_trainer *t, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_restore_best: trainer is NULL");
    LT_REQUIRE(t->val != nullptr && t->val->keep_best, "lt_gcn3_trainer_restore_best: no validation with keep_best attached");
    return launch_snapshot(snap_segs3(t), t->val->snap, t->val->state + VS_SEEN, 1, (hipStream_t)stream);
}

extern "C" int lt_gcn3_trainer_val_logits(const lt_gcn3_trainer *t, float *Z, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr, "lt_gcn3_trainer_val_logits: trainer is NULL");
    return val_copy_logits("lt_gcn3_trainer_val_logits", t->val, t->C, Z, ldz, (hipStream_t)stream);
}
