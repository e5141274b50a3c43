// Training of the 2-layer GCN and the 3-layer GCN3: one epoch of GCNTrainer.train_one_epoch (reference gcn_trainer.py:144-170,
// gcn/models.py:19-46, F.cross_entropy, torch.optim.Adam), as stream-ordered launches with no host synchronisation.  Both
// models run ONE epoch (run_epoch): the "top chain" -- the last hidden layer, the class layer, the loss head and their
// backward -- behind an optional FRONT layer, which only GCN3 has.  S is the product the top chain starts from, b the bias of
// its hidden layer, Wc / bc the class layer's parameters.
//
//   front layer (GCN3)
//   S1 = X W1                      lt_launch_gemm(_splitk)        the forward's product, same slicing: same bits
//   Hf = drop_0(relu(A S1 + b1))   k_tr3_layer1 (+ _long)         row_dot chains from the bias, ReLU and the Philox mask (layer
//                                                                 word 0) as the epilogue: Z1 never exists in memory
//   S = Hf W2                      lt_launch_gemm
//   top chain (without a front layer: S = X W1, the product above)
//   Z = A S + b                    lt_launch_layer1 (Z stored)    the forward's chains
//   Hd = drop(relu(Z)), Sc = Hd Wc k_tr_dropout                   Philox4x32-10 mask, layer word = hidden layers in front of
//                                                                 it (0 or 1); Sc with relu_w2_partial's order
//   Zc = A Sc + bc                 lt_launch_layer2               the forward's last layer: with p = 0, Zc IS the forward's output
//   loss, dZc, correct, dbc        k_tr_ce, k_tr_ce_reduce        per-row CE head, then one block: mean loss, count, dbc
//   dSc = A^T dZc                  k_tr_spmm_t_narrow             CSC rows (A is not symmetric in general)
//   dZ, db | dWc partials          k_tr_bwd_rows                  dZ = [Hd > 0] (dSc Wc^T) / (1 - p); fixed-order row blocks
//   db, dWc                        k_tr_colsum                    the blocks' partials in block order
//   dS = A^T dZ                    k_tr_spmm_t_wide               row_dot chains over the CSC
//   front layer's backward (GCN3)
//   dW2 = Hf^T dS                  k_gemm_tn_mfma + k_sum_slabs
//   dZ1 = [Hf > 0] scale (dS W2^T), db1 slabs       k_tr3_dz_mfma, then k_tr_colsum
//   dS1 = A^T dZ1                  k_tr_spmm_t_wide
//   both
//   dW1 = X^T dS1                  k_gemm_tn_mfma + k_sum_slabs   v_mfma_f32_32x32x2_f32, A^T staged through LDS, split-K
//   Adam                           k_tr_adam / k_tr3_adam         one launch over W1 | b1 | W2 | b2 (| W3 | b3) and the padded copies
//
// With the wide head (lt_gcn*_trainer_create_wide; lt_train_wide.hip.h, included below) the top chain is launch_wide_forward,
// launch_trw_head and launch_wide_backward instead: the class layer as matrix products at the padded width, the hidden layer's
// backward a k_tr3_dz_mfma stage (GCN3 then runs two: dZ2 here, dZ1 in the front layer's backward), Adam by k_tr3_adam over
// four segments or, for GCN3, k_tr3w_adam over six.
//
// Every reduction has a fixed order (no float atomics): two trainings with the same inputs give the same bits.
// Built with -ffp-contract=off: the only fused operations are explicit fmaf calls and the MFMAs.
#include <math.h>

#include <new>

#include "lt_philox.hip.h"
#include "lt_rows.hip.h"
#include "lt_train_common.hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

#define TR_BLOCK 256
#define TR_ROWS_PER_BLOCK 32   // k_tr_bwd_rows: rows summed by one block (its partial is one slab of the column sums)

// (the dropout mask -- lt_drop_block, lt_drop_args, lt_drop4 -- and Adam's element update live in lt_train_common.hip.h, which
// the minibatch MLP trainer shares)

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
// LIST (lt_gcn*_trainer_set_train_rows): one thread per list POSITION k < n, row r = rows[k] (the library checked the list:
// distinct ids inside the graph); loss_r / corr_r are indexed by k, dZ2 is written at row r and nowhere else -- the other
// rows keep the zeros they got when the list was set -- and inv_n = 1 / (the list's length).  The same operations in the same
// order: the list 0 .. n - 1 leaves the bits of the launch without one.  Without LIST rows is not read.
// --------------------------------------------------------------------------------------------
template <int CP, bool LIST>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_ce(int n, const int32_t *__restrict__ rows, const float *__restrict__ Z2, int C,
                                                    const int32_t *__restrict__ labels, float inv_n,
                                                    float *__restrict__ loss_r, int32_t *__restrict__ corr_r,
                                                    float *__restrict__ dZ2) {
    const int k = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int r = LIST ? rows[k] : k;
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
    loss_r[k] = (mx + logf(s)) - zy;
    corr_r[k] = arg == y ? 1 : 0;
#pragma unroll
    for (int c = 0; c < CP; ++c)
        if (c < C) dZ2[(size_t)r * C + c] = (e[c] / s - (c == y ? 1.f : 0.f)) * inv_n;
}

// One block: mean loss and correct count into the epoch's record, db2 = sum_r dZ2 -- thread t sums rows t, t + 256, ...
// in row order, then a fixed tree over the threads.  LIST: positions t, t + 256, ... of the n listed rows, dZ2 read through
// the list.
template <int CP, bool LIST>
__global__ __launch_bounds__(TR_BLOCK) void k_tr_ce_reduce(int n, const int32_t *__restrict__ rows, int C,
                                                           const float *__restrict__ loss_r,
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
    for (int i = t; i < n; i += TR_BLOCK) {
        const int r = LIST ? rows[i] : i;
        l += loss_r[i];
        k += corr_r[i];
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
// (lt_adam_scalars, adam_scalars and adam_elem: lt_train_common.hip.h)

__global__ void k_adam(int64_t n, float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m,
                       float *__restrict__ v, lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float mi = m[i], vi = v[i];
    p[i] = adam_elem(p[i], g[i], mi, vi, s);
    m[i] = mi;
    v[i] = vi;
}

// A model's parameter tensors as six segments of one concatenation W1 | b1 | W2 | b2 | W3 | b3, the layout of the gradient,
// moment and snapshot buffers: segment k is p[k], o[k] is where it ends.  The 2-layer model has four: o[4] = o[5] = o[3].
struct lt_snap_segs {
    float *p[6];
    int64_t o[6];
};

// The row kernels read zero-padded copies of some parameters (a bias [H] as [Hp], a weight [H, C] as [Hp, C]): the 2-layer
// model of b1 and W2 (b1p, W2p), GCN3 of b1, b2 and W3.  The Adam launch keeps them current and a pad launch rebuilds them
// from the borrowed parameters.  Each model has its own pair of kernels: one pair over the six-segment table measured 0.3 %
// slower per epoch for the 2-layer model at H = 256 (NOTES.md, the trainer-core entry), so the two were kept.

// The four parameter tensors of the 2-layer model in one launch: index i of the concatenation W1 | b1 | W2 | b2.
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

// GCN3's six tensors in one launch: the segment table and the copies b1p [Hp1], b2p [Hp2], W3p [Hp2, C].
struct lt_tr3_tensors {
    lt_snap_segs s;
    float *b1p, *b2p, *W3p;
};

__global__ void k_tr3_adam(lt_tr3_tensors T, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                           lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.s.o[5]) return;
    const int k = i < T.s.o[0] ? 0 : i < T.s.o[1] ? 1 : i < T.s.o[2] ? 2 : i < T.s.o[3] ? 3 : i < T.s.o[4] ? 4 : 5;
    const int64_t j = k ? i - T.s.o[k - 1] : i;
    float *p;      // a switch over constant indices: T.s.p[k] with a run-time k would move the argument struct to scratch
    switch (k) {
        case 0: p = T.s.p[0]; break;
        case 1: p = T.s.p[1]; break;
        case 2: p = T.s.p[2]; break;
        case 3: p = T.s.p[3]; break;
        case 4: p = T.s.p[4]; break;
        default: p = T.s.p[5]; break;
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

__global__ void k_tr3_pad(const float *__restrict__ b1, int H1, int Hp1, const float *__restrict__ b2, int H2, int Hp2,
                          const float *__restrict__ W3, int C, float *__restrict__ b1p, float *__restrict__ b2p,
                          float *__restrict__ W3p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Hp1) b1p[i] = i < H1 ? b1[i] : 0.f;
    if (i < Hp2) b2p[i] = i < H2 ? b2[i] : 0.f;
    if (i < Hp2 * C) W3p[i] = (i / C) < H2 ? W3[i] : 0.f;
}

// GCN3 with the wide head: the six segments and the three bias copies b1p [Hp1], b2p [Hp2], b3p [Cp].  No W3p: both products
// read W3 as it lies.  A sibling of k_tr3_adam / k_tr3_pad, not a generalisation of them (NOTES.md, 2026-10-20, "Left out").
struct lt_tr3w_tensors {
    lt_snap_segs s;
    float *b1p, *b2p, *b3p;
};

__global__ void k_tr3w_adam(lt_tr3w_tensors T, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                            lt_adam_scalars s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.s.o[5]) return;
    const int k = i < T.s.o[0] ? 0 : i < T.s.o[1] ? 1 : i < T.s.o[2] ? 2 : i < T.s.o[3] ? 3 : i < T.s.o[4] ? 4 : 5;
    const int64_t j = k ? i - T.s.o[k - 1] : i;
    float *p;      // a switch over constant indices, as in k_tr3_adam
    switch (k) {
        case 0: p = T.s.p[0]; break;
        case 1: p = T.s.p[1]; break;
        case 2: p = T.s.p[2]; break;
        case 3: p = T.s.p[3]; break;
        case 4: p = T.s.p[4]; break;
        default: p = T.s.p[5]; break;
    }
    float mi = m[i], vi = v[i];
    const float np = adam_elem(p[j], g[i], mi, vi, s);
    p[j] = np;
    m[i] = mi;
    v[i] = vi;
    if (k == 1) T.b1p[j] = np;
    else if (k == 3) T.b2p[j] = np;
    else if (k == 5) T.b3p[j] = np;
}

__global__ void k_tr3w_pad(const float *__restrict__ b1, int H1, int Hp1, const float *__restrict__ b2, int H2, int Hp2,
                           const float *__restrict__ b3, int C, int Cp, float *__restrict__ b1p, float *__restrict__ b2p,
                           float *__restrict__ b3p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Hp1) b1p[i] = i < H1 ? b1[i] : 0.f;
    if (i < Hp2) b2p[i] = i < H2 ? b2[i] : 0.f;
    if (i < Cp) b3p[i] = i < C ? b3[i] : 0.f;
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
// LIST: entry i = blockIdx.x * 256 + t scores logits row rows[i] against labels[rows[i]], i < m, so the list 0 .. n - 1
// leaves the bits of the launch without one.  An id outside [0, n) is never dereferenced: its entry adds 0 to the loss and
// counts in no cell; each block adds its number of such entries to *n_bad (an integer atomic: the total does not depend on
// order).  Without LIST, m, rows and n_bad are not read.
template <int CP, bool LIST>
__global__ __launch_bounds__(TR_BLOCK) void k_val_rows(int n, int m, const int32_t *__restrict__ rows,
                                                       const float *__restrict__ Z, long ldz, int C,
                                                       const int32_t *__restrict__ labels, float *__restrict__ part_loss,
                                                       int32_t *__restrict__ part_cnt, int32_t *n_bad) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int sc[CP * CP];
    __shared__ int sbad;
    const int t = threadIdx.x;
    int r = blockIdx.x * TR_BLOCK + t;
    if (t < CP * CP) sc[t] = 0;
    if constexpr (LIST)
        if (t == 0) sbad = 0;
    __syncthreads();
    bool scored = r < (LIST ? m : n);
    if constexpr (LIST) {
        if (scored) {
            r = rows[r];
            scored = (unsigned)r < (unsigned)n;
            if (!scored && n_bad) atomicAdd(&sbad, 1);
        }
    }
    float l = 0.f;
    if (scored) {
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
    if constexpr (LIST)
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
    int64_t ldy = 0;                       // wide BCE head: leading dimension of the uint8 labels
    int32_t keep_best = 0, patience = 0;
    int32_t kslice = 0;           // split-K slicing of X2 W1, chosen for n2 (the forward's choice at that size)
    int32_t n_blk = 0;            // blocks of k_val_rows
    float *fS = nullptr, *fH = nullptr;    // [n2, Hp of the front layer] GCN3: X2 W1 and relu(A fS + b1)
    float *S = nullptr, *Z = nullptr;      // [n2, Hp of the top chain]; without a front layer Z only feeds the tiled layer-1 route
    float *Sc = nullptr, *Zc = nullptr;    // [n2, C]: the last product and the validation logits
    float *slabs = nullptr, *seg_part = nullptr;
    float *part_loss = nullptr;            // [n_blk]
    int32_t *part_cnt = nullptr;           // [n_blk, C * C]
    int32_t *state = nullptr;              // [VAL_STATE_WORDS]
    float *snap = nullptr;                 // [n_param] (keep_best)
};

static void free_val(lt_val *v) {
    if (!v) return;
    float *bufs[] = {v->fS, v->fH, v->S, v->Z, v->Sc, v->Zc, v->slabs, v->seg_part, v->part_loss, v->snap};
    for (float *b : bufs) (void)hipFree(b);
    (void)hipFree(v->part_cnt);
    (void)hipFree(v->state);
    delete v;
}

static size_t val_head_bytes(int n, int C) {
    const size_t n_blk = (size_t)((n + TR_BLOCK - 1) / TR_BLOCK);
    return n_blk * (1 + (size_t)C * C) * sizeof(float);
}

// The head: the row stage over all n rows (rows == NULL) or over the m listed ones, then the finish stage with the number
// of scored entries as the divisor.
static int launch_val_head(const float *Z, long ldz, const int32_t *labels, int n, int C, const int32_t *rows, int m,
                           float *part_loss, int32_t *part_cnt, float *loss_out, int32_t *conf_out, int32_t *n_bad,
                           int32_t *state, int patience, int epoch, hipStream_t st) {
    const int cnt = rows ? m : n, n_blk = (cnt + TR_BLOCK - 1) / TR_BLOCK;
    const dim3 grid((unsigned)n_blk), block(TR_BLOCK);
    if (rows) {
        LT_DISPATCH_CP(lt_cp_for(C), hipLaunchKernelGGL((k_val_rows<CP_, true>), grid, block, 0, st, n, m, rows, Z, ldz, C, labels,
                                                        part_loss, part_cnt, n_bad));
    } else {
        LT_DISPATCH_CP(lt_cp_for(C), hipLaunchKernelGGL((k_val_rows<CP_, false>), grid, block, 0, st, n, m, rows, Z, ldz, C, labels,
                                                        part_loss, part_cnt, n_bad));
    }
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_val_finish, dim3(1), dim3(TR_BLOCK), 0, st, n_blk, cnt, C, part_loss, part_cnt, loss_out, conf_out,
                       state, patience, epoch);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// --------------------------------------------------------------------------------------------
// The front layer of GCN3 and its backward
// --------------------------------------------------------------------------------------------

// H1d[r] = drop(relu(A[r, :] S + bias)) for every row.  The launch's first seg_blocks blocks take the SEGMENTS of the hub rows
// (k_layer1's scheme: row_dot's canonical order, the first segment's chain started from the bias); k_tr3_layer1_long adds
// them in segment order and applies the same epilogue.  ACT = false: no ReLU and no mask, the row is stored as it is summed (the
// wide head's class layer Z2 = A S2 + b2).
template <int LPR, bool ACT = true>
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
        f32x4 h = z;
        if constexpr (ACT) {
            h = f32x4{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
            if (d.on) h = lt_drop4(h, r, coff, H, d);
        }
        *reinterpret_cast<f32x4 *>(Hd + (size_t)r * Hp + coff) = h;
    }
}

template <int LPR, bool ACT = true>
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
    f32x4 h = z;
    if constexpr (ACT) {
        h = f32x4{fmaxf(z.x, 0.f), fmaxf(z.y, 0.f), fmaxf(z.z, 0.f), fmaxf(z.w, 0.f)};
        if (d.on) h = lt_drop4(h, r, coff, H, d);
    }
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

// The wide head's kernels and launcher.  Included here, not at the top: it uses TR_BLOCK, val_state_update and the row helpers
// of lt_rows.hip.h defined above, and the trainer below uses its trw_plan / trw_parts / launch_trw_head.
#include "lt_train_wide.hip.h"

// --------------------------------------------------------------------------------------------
// trainer state: one struct behind both public handles
// --------------------------------------------------------------------------------------------
struct lt_tn {                    // one dW = A^T B product over K = n rows
    int32_t kslice = 0, splits = 0;
    float *slabs = nullptr;       // [splits, M, N] when splits > 1
};

struct lt_trainer {
    const lt_graph *g = nullptr;
    int32_t layers = 0;           // 2 (GCN) or 3 (GCN3); top = layers - 2 is the number of hidden layers in front of the top chain
    int32_t n = 0, F = 0, C = 0;
    int32_t H[2] = {0, 0}, Hp[2] = {0, 0};   // hidden widths in model order, and rounded up to 4; the top chain's is [top]
    const float *X = nullptr;
    int64_t ldx = 0;
    const int32_t *labels = nullptr;
    float *P[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // W1, b1, W2, b2, W3, b3 (borrowed)
    int64_t off[6] = {0, 0, 0, 0, 0, 0};                                    // where each ends in grad / m / v; off[5]: all of them
    double lr = 0, wd = 0, p = 0;
    uint64_t seed = 0;
    int64_t epoch = 0;            // epochs run since creation (= Adam's step count)
    int32_t kslice = 0;           // split-K slicing of X W1 (the forward's)
    lt_tn tn[3];                  // dW1 = X^T dS1; GCN3: dW2 = Hf^T dS; the wide head: tn[top + 1], dWc = Hd^T dSc
    int32_t n_part = 0;           // row blocks of k_tr_bwd_rows
    int32_t n_mblk = 0;           // row blocks of k_tr3_dz_mfma
    int32_t n_seg = 0;            // the graph's hub-row segments at creation (g->p_n_seg): the rows of seg_part
    float *S = nullptr, *Z = nullptr, *Hd = nullptr, *dZ = nullptr, *dS = nullptr;    // top chain, [n, Hp[top]]
    float *Sc = nullptr, *Zc = nullptr, *dZc = nullptr, *dSc = nullptr;               // top chain, [n, C]
    float *fS = nullptr, *fHd = nullptr, *fdZ = nullptr, *fdS = nullptr;              // front layer (GCN3), [n, Hp[0]]
    float *loss_r = nullptr;
    int32_t *corr_r = nullptr;
    // owned: mir[k] is the zero-padded copy of segment k the row kernels read, mir_len[k] floats (b1, and the top chain's
    // b and Wc); NULL / 0 for the other segments
    float *mir[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int32_t mir_len[6] = {0, 0, 0, 0, 0, 0};
    float *slabs = nullptr, *part = nullptr, *part1 = nullptr, *seg_part = nullptr;
    float *part2 = nullptr;       // GCN3 with the wide head: the db2 slabs [n_mblk, H2] of the top chain's k_tr3_dz_mfma stage
    float *grad = nullptr, *m = nullptr, *v = nullptr;   // [off[5]]
    lt_val *val = nullptr;        // lt_gcn*_trainer_attach_validation (owned)
    // The wide head (lt_gcn*_trainer_create_wide; lt_train_wide.hip.h): the class layer as matrix products at the padded width
    // Cp, Sc / Zc / dZc / dSc [n, Cp] with zero pad columns, `labels` int32 [n] (CE) or uint8 [n, ldy] (BCE), mir[2 top + 3] = the
    // class bias at Cp (b2 of the 2-layer model, b3 of GCN3, whose mir[3] is b2 at Hp2).
    int32_t wide = 0, loss_kind = 0, Cp = 0;
    int64_t ldy = 0;
    float *whead = nullptr;       // the head's partials (trw_part_bytes) and, behind them, the last epoch's counts [C, 3]
    // lt_gcn*_trainer_set_train_rows (owned, NULL / 0 without a list): the m listed row ids on the device and, for the wide
    // head, its partials at the list's length (trw_part_bytes(m): a shorter list can be cut into MORE blocks than n rows are)
    int32_t *train_rows = nullptr;
    int32_t n_train = 0;
    float *lhead = nullptr;
};
// widest padded row a segment scratch holds: the hidden widths and, for the wide head, the class layer's Cp
static inline int trainer_hpm(const lt_trainer *t) {
    const int h = t->Hp[0] > t->Hp[1] ? t->Hp[0] : t->Hp[1];
    return t->wide && t->Cp > h ? t->Cp : h;
}
static inline int trainer_ldc(const lt_trainer *t) { return t->wide ? t->Cp : t->C; }      // leading dimension of the [n, C] buffers
static inline int32_t *trainer_counts(const lt_trainer *t) {      // behind the all-rows head's partials, with a list too
    return (int32_t *)((char *)t->whead + trw_parts(t->whead, t->n, t->C, true).bytes);
}
// the training head's partials: over all n rows, or over the list
static inline lt_trw_parts trainer_head_parts(const lt_trainer *t) {
    return t->train_rows ? trw_parts(t->lhead, t->n_train, t->C, true) : trw_parts(t->whead, t->n, t->C, true);
}
struct lt_gcn2_trainer : lt_trainer {};
struct lt_gcn3_trainer : lt_trainer {};

// Every device buffer a trainer owns: where its pointer lives, its size (0: not allocated) and whether it starts at zero.
// create walks the table to allocate, free to release.
struct lt_buf {
    void **slot;
    size_t bytes;
    bool zero;
};
#define TR_MAX_BUFS 40

// Fills b[TR_MAX_BUFS] from the trainer's own fields (the borrowed graph is not read: destroy may come after the graph's) and
// returns the number of entries, -1 if the table does not hold them all.
static int trainer_bufs(lt_trainer *t, lt_buf *b) {
    const int top = t->layers - 2, C = t->C, hpm = trainer_hpm(t);
    const size_t f4 = sizeof(float), n = (size_t)t->n;
    const bool w = t->wide != 0;      // the wide head: no Z, no row-loss arrays, no k_tr_bwd_rows slabs; its own partials
    const size_t nt = n * t->Hp[top] * f4, nf = top ? n * t->Hp[0] * f4 : 0, nc = n * trainer_ldc(t) * f4, np = (size_t)t->off[5] * f4;
    int k = 0;
    auto add = [&](auto *slot, size_t bytes, bool zero = false) {
        if (k < TR_MAX_BUFS) b[k] = lt_buf{(void **)slot, bytes, zero};
        ++k;
    };
    // pad columns of the products (the GEMMs write H of them) and of the front layer's dZ (its product writes H of them) stay
    // zero; the moments start at zero
    add(&t->fS, nf, true); add(&t->S, nt, true); add(&t->fdZ, nf, true);
    add(&t->fHd, nf); add(&t->fdS, nf);
    // (wide: the class product writes C of the Cp columns of Sc, the dZ product H of the Hp columns of dZ)
    add(&t->Z, w ? 0 : nt); add(&t->Hd, nt); add(&t->dZ, nt, w); add(&t->dS, nt);
    add(&t->Sc, nc, w); add(&t->Zc, nc); add(&t->dZc, nc); add(&t->dSc, nc);
    add(&t->loss_r, w ? 0 : n * f4); add(&t->corr_r, w ? 0 : n * sizeof(int32_t));
    for (int s = 0; s < 6; ++s) add(&t->mir[s], (size_t)t->mir_len[s] * f4);
    add(&t->slabs, lt_gemm_splitk_slab_bytes(t->n, t->H[0], t->F, t->kslice));
    add(&t->tn[0].slabs, t->tn[0].splits > 1 ? (size_t)t->tn[0].splits * t->F * t->H[0] * f4 : 0);
    add(&t->tn[1].slabs, t->tn[1].splits > 1 ? (size_t)t->tn[1].splits * t->H[0] * (top ? t->H[1] : C) * f4 : 0);
    add(&t->tn[2].slabs, t->tn[2].splits > 1 ? (size_t)t->tn[2].splits * t->H[1] * C * f4 : 0);
    add(&t->part, w ? 0 : (size_t)t->n_part * ((size_t)t->H[top] + (size_t)t->H[top] * C) * f4);
    add(&t->part1, top || w ? (size_t)t->n_mblk * t->H[0] * f4 : 0);
    add(&t->part2, top && w ? (size_t)t->n_mblk * t->H[1] * f4 : 0);
    add(&t->whead, w ? trw_part_bytes(t->n, C, true) + 3 * (size_t)C * sizeof(int32_t) : 0);
    add(&t->seg_part, (size_t)t->n_seg * hpm * f4);
    add(&t->grad, np); add(&t->m, np, true); add(&t->v, np, true);
    return k <= TR_MAX_BUFS ? k : -1;
}

static void free_trainer(lt_trainer *t) {
    if (!t) return;
    free_val(t->val);
    lt_buf b[TR_MAX_BUFS];
    const int nb = trainer_bufs(t, b);
    for (int k = 0; k < nb; ++k) (void)hipFree(*b[k].slot);
    (void)hipFree(t->train_rows);
    (void)hipFree(t->lhead);
    if (t->layers == 3) delete static_cast<lt_gcn3_trainer *>(t);
    else delete static_cast<lt_gcn2_trainer *>(t);
}

static int tn_pick_splits(int M, int N, int K) {
    // about two blocks per CU over the 256 CUs, slices of at least 256 rows
    const long tiles = (long)((M + TN_BM - 1) / TN_BM) * ((N + TN_BN - 1) / TN_BN);
    long s = (512 + tiles - 1) / tiles;
    s = s < 1 ? 1 : s > 16 ? 16 : s;
    while (s > 1 && (K + s - 1) / s < 256) --s;
    return (int)s;
}

static void tn_plan(lt_tn *tn, int M, int N, int K) {
    tn->splits = tn_pick_splits(M, N, K);
    tn->kslice = lt_round_up((K + tn->splits - 1) / tn->splits, TN_BK);
    tn->splits = (K + tn->kslice - 1) / tn->kslice;
}

// What both lt_gcn*_trainer_create share, behind the checks whose wording names the model's widths.  Hs: the hidden widths
// (Hs[1] = 0 for the 2-layer model), ps: the 2 * layers parameter tensors.
static int trainer_create(const char *who, int layers, const lt_graph *g, const float *X, int64_t ldx, int32_t F,
                          const int32_t *labels, const int32_t *Hs, int32_t C, float *const *ps, double lr, double weight_decay,
                          double dropout, uint64_t seed, void *stream, lt_trainer **out, int wide = 0, int loss_kind = 0,
                          int64_t ldy = 0) {
    LT_REQUIRE(ldx >= F, "%s: ldx=%lld < F=%d", who, (long long)ldx, F);
    LT_REQUIRE(dropout >= 0.0 && dropout <= 1.0, "%s: dropout=%g outside [0, 1]", who, dropout);
    LT_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "%s: lr=%g weight_decay=%g", who, lr, weight_decay);
    LT_REQUIRE(g->n > 0, "%s: empty graph", who);
    lt_trainer *t = layers == 3 ? static_cast<lt_trainer *>(new (std::nothrow) lt_gcn3_trainer())
                                : static_cast<lt_trainer *>(new (std::nothrow) lt_gcn2_trainer());
    if (!t) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
    const int n = g->n, top = layers - 2;
    t->g = g; t->layers = layers; t->n = n; t->F = F; t->C = C;
    t->X = X; t->ldx = ldx; t->labels = labels;
    t->wide = wide; t->loss_kind = loss_kind; t->ldy = ldy; t->Cp = lt_round_up(C, 4);
    const int dims[4] = {F, Hs[0], top ? Hs[1] : C, C};      // layer l maps dims[l] to dims[l + 1] columns
    int64_t end = 0;
    for (int l = 0; l < 3; ++l) {
        const bool have = l < layers;
        if (l <= top) { t->H[l] = dims[l + 1]; t->Hp[l] = lt_round_up(dims[l + 1], 4); }
        t->P[2 * l] = have ? ps[2 * l] : nullptr;
        t->off[2 * l] = end += have ? (int64_t)dims[l] * dims[l + 1] : 0;
        t->P[2 * l + 1] = have ? ps[2 * l + 1] : nullptr;
        t->off[2 * l + 1] = end += have ? dims[l + 1] : 0;
    }
    t->lr = lr; t->wd = weight_decay; t->p = dropout; t->seed = seed;
    t->kslice = lt_gemm_pick_kslice(n, t->H[0], F);
    tn_plan(&t->tn[0], F, t->H[0], n);
    if (top) tn_plan(&t->tn[1], t->H[0], t->H[1], n);
    if (wide) tn_plan(&t->tn[top + 1], t->H[top], C, n);      // dWc = Hd^T dSc (dW2 of the 2-layer model, dW3 of GCN3)
    t->n_part = (n + TR_ROWS_PER_BLOCK - 1) / TR_ROWS_PER_BLOCK;
    t->n_mblk = (n + TN_BM - 1) / TN_BM;
    t->n_seg = g->p_n_seg > 0 ? g->p_n_seg : 0;
    t->mir_len[1] = t->Hp[0];
    if (wide) {      // the class weight is read as it lies by the products
        t->mir_len[2 * top + 1] = t->Hp[top];
        t->mir_len[2 * top + 3] = t->Cp;
    } else {
        t->mir_len[2 * top + 1] = t->Hp[top];
        t->mir_len[2 * top + 2] = t->Hp[top] * C;
    }
    hipStream_t st = (hipStream_t)stream;
    lt_buf b[TR_MAX_BUFS];
    const int nb = trainer_bufs(t, b);
    if (nb < 0) {      // nothing is allocated yet
        free_trainer(t);
        return lt_set_error(LT_ERR_INVALID, "%s: the buffer table holds %d entries, the trainer has more", who, TR_MAX_BUFS);
    }
    hipError_t e = hipSuccess;
    const char *what = "hipMalloc";
    for (int k = 0; k < nb && e == hipSuccess; ++k)
        if (b[k].bytes) e = hipMalloc(b[k].slot, b[k].bytes);
    if (e == hipSuccess) what = "hipMemsetAsync";
    for (int k = 0; k < nb && e == hipSuccess; ++k)
        if (b[k].bytes && b[k].zero) e = hipMemsetAsync(*b[k].slot, 0, b[k].bytes, st);
    if (e != hipSuccess) {
        free_trainer(t);
        return lt_set_error(LT_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
    }
    *out = t;
    return LT_OK;
}

// --------------------------------------------------------------------------------------------
// the launches of one epoch, in pieces the validation forward shares
// --------------------------------------------------------------------------------------------
static unsigned rows_grid(int n, int rows_per_block) { return (unsigned)((n + rows_per_block - 1) / rows_per_block); }
static int wide_rows_per_block(int Hp) { return (TR_BLOCK / 64) * (64 / lt_lpr_for(Hp)); }

// the mask of the epoch about to run (layer word 0)
static lt_drop_args drop_args(const lt_trainer *t) {
    lt_drop_args d;
    d.on = t->p > 0.0;
    d.thresh = (uint64_t)floor(t->p * 4294967296.0);
    d.scale = t->p < 1.0 ? (float)(1.0 / (1.0 - t->p)) : 0.f;
    d.epoch = (uint32_t)t->epoch;
    d.seed = t->seed;
    return d;
}

// S1 = X W1 over the n rows of X, through split-K slabs where the forward slices
static int launch_xw1(const lt_trainer *t, const float *X, int64_t ldx, int n, int kslice, float *slabs, float *S1,
                      hipStream_t st) {
    const int H = t->H[0];
    if (slabs) return lt_launch_gemm_splitk(X, ldx, t->P[0], H, S1, t->Hp[0], n, H, t->F, kslice, slabs, st);
    return lt_launch_gemm(X, ldx, t->P[0], H, S1, t->Hp[0], n, H, t->F, st);
}

// out = A S + bias for every row of g at the padded width Hp, through k_tr3_layer1 (+ _long for the hub rows); ACT: with the
// ReLU and the mask d
template <bool ACT>
static int launch_rows_layer(const lt_graph *g, const float *S, int Hp, int H, const float *biasp, const lt_drop_args &d,
                             float *out, float *seg_part, hipStream_t st) {
    const int n = g->n, lpr = lt_lpr_for(Hp), rpb = wide_rows_per_block(Hp);
    const int have_long = g->p_n_long > 0 ? 1 : 0;
    const unsigned seg_blocks = have_long ? rows_grid(g->p_n_seg, rpb) : 0u;
    LT_DISPATCH_LPR(lpr, hipLaunchKernelGGL((k_tr3_layer1<LPR_, ACT>), dim3(rows_grid(n, rpb) + seg_blocks), dim3(TR_BLOCK), 0, st,
                                            n, g->rowptr, g->col, g->val, S, Hp, H, biasp, d, out, have_long, (int)seg_blocks,
                                            g->p_n_seg, g->p_seg_long, g->p_seg_begin, g->p_long_row, seg_part));
    LT_CHECK_LAUNCH();
    if (have_long) {
        LT_DISPATCH_LPR(lpr, hipLaunchKernelGGL((k_tr3_layer1_long<LPR_, ACT>), dim3(rows_grid(g->p_n_long, rpb)), dim3(TR_BLOCK),
                                                0, st, g->p_n_long, g->p_long_row, g->p_long_segptr, seg_part, Hp, H, d, out));
        LT_CHECK_LAUNCH();
    }
    return LT_OK;
}

// GCN3's front layer on graph g: Hf = drop(relu(A S1 + b1)), then the top chain's input S = Hf W2
static int launch_front(const lt_trainer *t, const lt_graph *g, const float *S1, const lt_drop_args &d, float *Hf,
                        float *seg_part, float *S, hipStream_t st) {
    const int rc = launch_rows_layer<true>(g, S1, t->Hp[0], t->H[0], t->mir[1], d, Hf, seg_part, st);
    if (rc) return rc;
    return lt_launch_gemm(Hf, t->Hp[0], t->P[2], t->H[1], S, t->Hp[1], g->n, t->H[1], t->H[0], st);
}

static lt_drop_args drop_off() {
    lt_drop_args off;
    off.on = 0; off.thresh = 0; off.scale = 1.f; off.epoch = 0; off.seed = 0;
    return off;
}

// The wide route's forward on graph g from the top chain's product S (X W1; GCN3: Hf W2): Hd = drop(relu(A S + b)) with the
// mask d, Sc = Hd Wc (C of the Cp columns; the others stay zero), Zc = A Sc + bc at width Cp.  The chain's tensors by the
// trainer's depth: top = layers - 2 hidden layers lie in front of it.
static int launch_wide_forward(const lt_trainer *t, const lt_graph *g, const float *S, const lt_drop_args &d, float *Hd,
                               float *Sc, float *Zc, float *seg_part, hipStream_t st) {
    const int top = t->layers - 2, H = t->H[top], Hp = t->Hp[top], C = t->C, Cp = t->Cp;
    int rc = launch_rows_layer<true>(g, S, Hp, H, t->mir[2 * top + 1], d, Hd, seg_part, st);
    if (rc) return rc;
    rc = lt_launch_gemm(Hd, Hp, t->P[2 * top + 2], C, Sc, Cp, g->n, C, H, st);
    if (rc) return rc;
    return launch_rows_layer<false>(g, Sc, Cp, C, t->mir[2 * top + 3], drop_off(), Zc, seg_part, st);
}

static int launch_tn(const float *A, long lda, const float *B, long ldb, float *C, int M, int N, int K, const lt_tn &tn,
                     hipStream_t st);

// The wide route's backward from dZc down to the top chain's dS: the gradients of the class layer and of the hidden layer's
// bias.  The hidden layer's k_tr3_dz_mfma stage leaves its bias slabs in part1, or, behind a front layer whose own stage
// uses part1, in part2.
static int launch_wide_backward(const lt_trainer *t, float scale, hipStream_t st) {
    const lt_graph *g = t->g;
    const int top = t->layers - 2, n = t->n, H = t->H[top], Hp = t->Hp[top], C = t->C, Cp = t->Cp;
    float *bslabs = top ? t->part2 : t->part1;
    const lt_trw_parts parts = trainer_head_parts(t);
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((C + 63) / 64)), dim3(TR_BLOCK), 0, st, parts.db, parts.n_blk, C,
                       t->grad + t->off[2 * top + 2]);                                            // dbc
    LT_CHECK_LAUNCH();
    LT_DISPATCH_LPR(lt_lpr_for(Cp), hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, wide_rows_per_block(Cp))),
                                                       dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZc, Cp, t->dSc));
    LT_CHECK_LAUNCH();
    int rc = launch_tn(t->Hd, (long)Hp, t->dSc, (long)Cp, t->grad + t->off[2 * top + 1], H, C, n, t->tn[top + 1], st);      // dWc
    if (rc) return rc;
    dim3 grid((unsigned)t->n_mblk, (unsigned)((H + TN_BN - 1) / TN_BN));
    hipLaunchKernelGGL(k_tr3_dz_mfma, grid, dim3(256), 0, st, t->dSc, (long)Cp, t->P[2 * top + 2], (long)C, t->Hd, t->dZ, (long)Hp,
                       n, H, C, scale, bslabs);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((H + 63) / 64)), dim3(TR_BLOCK), 0, st, bslabs, t->n_mblk, H,
                       t->grad + t->off[2 * top]);                                                // db of the hidden layer
    LT_CHECK_LAUNCH();
    LT_DISPATCH_LPR(lt_lpr_for(Hp), hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, wide_rows_per_block(Hp))),
                                                       dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZ, Hp, t->dS));
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// The top chain's forward on graph g: Z = A S + b with layer 1's own Sc = relu(Z) Wc, then (d != NULL) Hd = drop(relu(Z)) and
// Sc = Hd Wc, then Zc = A Sc + bc.  d == NULL, the validation forward: with no mask k_tr_dropout would only repeat layer 1's
// Sc bits, so it is not launched.  Z may be NULL where layer 1 does not need it.
static int launch_top_forward(const lt_trainer *t, const lt_graph *g, const float *S, float *Z, const lt_drop_args *d, float *Hd,
                              float *Sc, float *Zc, float *seg_part, hipStream_t st) {
    const int top = t->layers - 2, n = g->n, H = t->H[top], Hp = t->Hp[top], C = t->C;
    const float *bp = t->mir[2 * top + 1], *Wcp = t->mir[2 * top + 2];
    int rc = lt_launch_layer1(g, S, Hp, bp, Wcp, C, Z, Sc, st, seg_part);
    if (rc) return rc;
    if (d) {
        LT_DISPATCH_LPR(lt_lpr_for(Hp), LT_DISPATCH_CP(lt_cp_for(C),
            hipLaunchKernelGGL((k_tr_dropout<LPR_, CP_>), dim3(rows_grid(n, wide_rows_per_block(Hp))), dim3(TR_BLOCK), 0, st, n, Z,
                               Hp, H, Wcp, C, *d, Hd, Sc)));
        LT_CHECK_LAUNCH();
    }
    return lt_launch_layer2(g, Sc, C, t->P[2 * top + 3], Zc, st);
}

// loss head: the epoch's record, dZc and dbc; with a list of training rows (LIST), over its positions
template <bool LIST>
static int launch_loss_head(const lt_trainer *t, float *record, hipStream_t st) {
    const int C = t->C, cp = lt_cp_for(C), cnt = LIST ? t->n_train : t->n;
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce<CP_, LIST>), dim3(rows_grid(cnt, TR_BLOCK)), dim3(TR_BLOCK), 0, st, cnt,
                                          t->train_rows, t->Zc, C, t->labels, 1.0f / (float)cnt, t->loss_r, t->corr_r, t->dZc));
    LT_CHECK_LAUNCH();
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_ce_reduce<CP_, LIST>), dim3(1), dim3(TR_BLOCK), 0, st, cnt, t->train_rows, C,
                                          t->loss_r, t->corr_r, t->dZc, record, t->grad + t->off[2 * (t->layers - 2) + 2]));
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// The top chain's backward: dSc = A^T dZc, dZ and the gradients of the hidden layer's bias and of Wc (adjacent in the
// gradient buffer), dS = A^T dZ.
static int launch_top_backward(const lt_trainer *t, float scale, hipStream_t st) {
    const lt_graph *g = t->g;
    const int top = t->layers - 2, n = t->n, H = t->H[top], Hp = t->Hp[top], C = t->C, cp = lt_cp_for(C);
    const float *Wcp = t->mir[2 * top + 2];
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_spmm_t_narrow<CP_>), dim3(rows_grid(n, TR_BLOCK / LT_L2_LANES)),
                                          dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZc, C, t->dSc));
    LT_CHECK_LAUNCH();
    int W = 1;
    while (W < Hp) W <<= 1;
    LT_DISPATCH_CP(cp, hipLaunchKernelGGL((k_tr_bwd_rows<CP_>), dim3((unsigned)t->n_part), dim3(TR_BLOCK), 0, st, n, H, Hp, W,
                                          C, t->Hd, t->dSc, Wcp, scale, t->dZ, t->part));
    LT_CHECK_LAUNCH();
    const int L = H + H * C;
    hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((L + 63) / 64)), dim3(TR_BLOCK), 0, st, t->part, t->n_part, L,
                       t->grad + t->off[2 * top]);
    LT_CHECK_LAUNCH();
    LT_DISPATCH_LPR(lt_lpr_for(Hp), hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, wide_rows_per_block(Hp))),
                                                       dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->dZ, Hp, t->dS));
    LT_CHECK_LAUNCH();
    return LT_OK;
}

// C [M, N] = A^T B over K rows, through the product's slabs when it is split
static int launch_tn(const float *A, long lda, const float *B, long ldb, float *C, int M, int N, int K, const lt_tn &tn,
                     hipStream_t st) {
    const bool split = tn.splits > 1;
    dim3 grid((unsigned)((M + TN_BM - 1) / TN_BM), (unsigned)((N + TN_BN - 1) / TN_BN), (unsigned)tn.splits);
    hipLaunchKernelGGL(k_gemm_tn_mfma, grid, dim3(256), 0, st, A, lda, B, ldb, split ? tn.slabs : C, (long)N, M, N, K, tn.kslice,
                       (long)M * N);
    LT_CHECK_LAUNCH();
    if (split) return lt_launch_sum_slabs(tn.slabs, (long)M * N, tn.splits, M, N, (long)N, C, (long)N, st);
    return LT_OK;
}

static lt_snap_segs snap_segs(const lt_trainer *t) {
    lt_snap_segs T;
    for (int k = 0; k < 6; ++k) { T.p[k] = t->P[k]; T.o[k] = t->off[k]; }
    return T;
}

static int run_epoch(lt_trainer *t, float *record, hipStream_t st) {
    const lt_graph *g = t->g;
    const int n = t->n, F = t->F, top = t->layers - 2, H1 = t->H[0], Hp1 = t->Hp[0];
    lt_drop_args d = drop_args(t);
    const float scale = t->p > 0.0 ? d.scale : 1.f;
    // forward
    int rc = launch_xw1(t, t->X, t->ldx, n, t->kslice, t->slabs, top ? t->fS : t->S, st);
    if (rc) return rc;
    if (top) {
        rc = launch_front(t, g, t->fS, d, t->fHd, t->seg_part, t->S, st);
        if (rc) return rc;
    }
    d.layer = (uint32_t)top;
    if (t->wide) {      // the class layer as matrix products, the wide head, and their backward
        rc = launch_wide_forward(t, g, t->S, d, t->Hd, t->Sc, t->Zc, t->seg_part, st);
        if (rc) return rc;
        rc = launch_trw_head(t->loss_kind, t->Zc, (long)t->Cp, t->labels, (long)t->ldy, n, t->C, t->train_rows, t->n_train, t->dZc,
                             t->train_rows ? t->lhead : t->whead, record, record + 1, trainer_counts(t), nullptr, nullptr, 0, 0,
                             st);
        if (rc) return rc;
        rc = launch_wide_backward(t, scale, st);
        if (rc) return rc;
    } else {
        rc = launch_top_forward(t, g, t->S, t->Z, &d, t->Hd, t->Sc, t->Zc, t->seg_part, st);
        if (rc) return rc;
        rc = t->train_rows ? launch_loss_head<true>(t, record, st) : launch_loss_head<false>(t, record, st);
        if (rc) return rc;
        // backward
        rc = launch_top_backward(t, scale, st);
        if (rc) return rc;
    }
    if (top) {      // through the middle weight and the front layer: dW2, dZ1 and db1, dS1
        const int H2 = t->H[1], Hp2 = t->Hp[1];
        rc = launch_tn(t->fHd, (long)Hp1, t->dS, (long)Hp2, t->grad + t->off[1], H1, H2, n, t->tn[1], st);
        if (rc) return rc;
        dim3 grid((unsigned)t->n_mblk, (unsigned)((H1 + TN_BN - 1) / TN_BN));
        hipLaunchKernelGGL(k_tr3_dz_mfma, grid, dim3(256), 0, st, t->dS, (long)Hp2, t->P[2], (long)H2, t->fHd, t->fdZ, (long)Hp1,
                           n, H1, H2, scale, t->part1);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_tr_colsum, dim3((unsigned)((H1 + 63) / 64)), dim3(TR_BLOCK), 0, st, t->part1, t->n_mblk, H1,
                           t->grad + t->off[0]);
        LT_CHECK_LAUNCH();
        LT_DISPATCH_LPR(lt_lpr_for(Hp1), hipLaunchKernelGGL((k_tr_spmm_t_wide<LPR_>), dim3(rows_grid(n, wide_rows_per_block(Hp1))),
                                                            dim3(TR_BLOCK), 0, st, n, g->tptr, g->trow, g->tval, t->fdZ, Hp1,
                                                            t->fdS));
        LT_CHECK_LAUNCH();
    }
    rc = launch_tn(t->X, (long)t->ldx, top ? t->fdS : t->dS, (long)Hp1, t->grad, F, H1, n, t->tn[0], st);
    if (rc) return rc;
    // Adam
    const int64_t step = t->epoch + 1;
    const lt_adam_scalars s = adam_scalars(step, t->lr, 0.9, 0.999, 1e-8, t->wd);
    const dim3 adam_grid((unsigned)((t->off[5] + 255) / 256));
    if (top && t->wide) {
        const lt_tr3w_tensors T = {snap_segs(t), t->mir[1], t->mir[3], t->mir[5]};
        hipLaunchKernelGGL(k_tr3w_adam, adam_grid, dim3(256), 0, st, T, t->grad, t->m, t->v, s);
    } else if (top || t->wide) {      // (wide: segments W1 | b1 | W2 | b2, the mirrors b1p and b2p; no fifth segment, so no W3p)
        const lt_tr3_tensors T = {snap_segs(t), t->mir[1], t->mir[3], t->mir[4]};
        hipLaunchKernelGGL(k_tr3_adam, adam_grid, dim3(256), 0, st, T, t->grad, t->m, t->v, s);
    } else {
        hipLaunchKernelGGL(k_tr_adam, adam_grid, dim3(256), 0, st, t->off[5], t->off[0], t->off[1], t->off[2], t->P[0], t->P[1],
                           t->P[2], t->P[3], t->grad, t->m, t->v, t->mir[1], t->mir[2], s);
    }
    LT_CHECK_LAUNCH();
    t->epoch = step;
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
    return launch_val_head(Z, (long)ldz, labels, n, C, nullptr, 0, part_loss, (int32_t *)(part_loss + n_blk), loss, confusion,
                           nullptr, nullptr, 0, 0, (hipStream_t)stream);
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
    return launch_val_head(Z, (long)ldz, labels, n, C, rows, m, part_loss, (int32_t *)(part_loss + n_blk), loss, confusion, n_bad,
                           nullptr, 0, 0, st);
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

// Everything lt_gcn*_trainer_attach_validation(_rows) checks and allocates.
static int val_attach(const char *who, lt_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2, int32_t n2,
                      const int32_t *labels2, int32_t keep_best, int32_t patience, void *stream, int with_rows = 0,
                      const int32_t *rows = nullptr, int32_t m = 0, int want_wide = 0, int64_t ldy2 = 0) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    LT_REQUIRE(t->wide == want_wide, "%s: the trainer has the %s head; attach with lt_gcn%d_trainer_attach_validation%s", who,
               t->wide ? "wide" : "narrow", t->layers, t->wide ? "_wide" : " or _attach_validation_rows");
    const int F = t->F, C = t->C, top = t->layers - 2;
    const bool bce = t->wide && t->loss_kind == TRW_BCE;
    if (bce) LT_REQUIRE(ldy2 >= C, "%s: ldy2=%lld < C=%d", who, (long long)ldy2, C);
    hipStream_t st = (hipStream_t)stream;
    LT_REQUIRE(t->val == nullptr, "%s: validation is already attached to this trainer", who);
    LT_REQUIRE(g2 != nullptr && X2 != nullptr && labels2 != nullptr, "%s: NULL argument", who);
    LT_REQUIRE(g2->n > 0, "%s: empty graph", who);
    LT_REQUIRE(n2 == g2->n, "%s: X2 has %d rows, the graph %d nodes", who, n2, g2->n);
    LT_REQUIRE(ldx2 >= F, "%s: ldx2=%lld < F=%d", who, (long long)ldx2, F);
    LT_REQUIRE(keep_best == 0 || keep_best == 1, "%s: keep_best=%d, must be 0 or 1", who, keep_best);
    LT_REQUIRE(patience >= 0, "%s: patience=%d, must be >= 0 (0: never stop)", who, patience);
    const int dev = ptr_device(t->X);
    LT_REQUIRE(dev >= 0 && ptr_device(X2) == dev && ptr_device(g2->rowptr) == dev && ptr_device(labels2) == dev,
               "%s: the validation graph, X2 and labels2 must live on the trainer's device (%d)", who, dev);
    if (with_rows) {
        LT_REQUIRE(rows != nullptr, "%s: rows is NULL", who);
        LT_REQUIRE(m > 0, "%s: m=%d, must be positive", who, m);
        LT_REQUIRE(ptr_device(rows) == dev, "%s: rows must live on the trainer's device (%d)", who, dev);
    }
    if (!bce) {      // (the BCE head reads bytes: any value other than 0 is a 1)
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
    v->kslice = lt_gemm_pick_kslice(n2, t->H[0], F);
    v->rows = with_rows ? rows : nullptr;
    v->m = with_rows ? m : 0;
    v->n_blk = ((with_rows ? m : n2) + TR_BLOCK - 1) / TR_BLOCK;
    v->ldy = ldy2;
    const size_t nf = (size_t)n2 * t->Hp[0] * sizeof(float), nt = (size_t)n2 * t->Hp[top] * sizeof(float);
    const size_t nc = (size_t)n2 * trainer_ldc(t) * sizeof(float);
    const int hpm = trainer_hpm(t);
#define V_HIP(call)                                                                         \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            free_val(v);                                                                    \
            return lt_set_error(LT_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
        }                                                                                   \
    } while (0)
    if (top) {
        V_HIP(hipMalloc((void **)&v->fS, nf));
        V_HIP(hipMemsetAsync(v->fS, 0, nf, st));      // the GEMMs write H of the Hp columns
        V_HIP(hipMalloc((void **)&v->fH, nf));
    }
    V_HIP(hipMalloc((void **)&v->S, nt));
    V_HIP(hipMemsetAsync(v->S, 0, nt, st));
    V_HIP(hipMalloc((void **)&v->Z, nt));
    V_HIP(hipMalloc((void **)&v->Sc, nc));
    if (t->wide) V_HIP(hipMemsetAsync(v->Sc, 0, nc, st));      // the class product writes C of the Cp columns
    V_HIP(hipMalloc((void **)&v->Zc, nc));
    const size_t sb = lt_gemm_splitk_slab_bytes(n2, t->H[0], F, v->kslice);
    if (sb) V_HIP(hipMalloc((void **)&v->slabs, sb));
    if (g2->p_n_seg > 0) V_HIP(hipMalloc((void **)&v->seg_part, (size_t)g2->p_n_seg * hpm * sizeof(float)));
    if (t->wide) {      // the wide head's partials in one block (launch_trw_head)
        V_HIP(hipMalloc((void **)&v->part_loss, trw_part_bytes(with_rows ? m : n2, C, false)));
    } else {
        V_HIP(hipMalloc((void **)&v->part_loss, (size_t)v->n_blk * sizeof(float)));
        V_HIP(hipMalloc((void **)&v->part_cnt, (size_t)v->n_blk * C * C * sizeof(int32_t)));
    }
    V_HIP(hipMalloc((void **)&v->state, VAL_STATE_WORDS * sizeof(int32_t)));
    if (keep_best) V_HIP(hipMalloc((void **)&v->snap, (size_t)t->off[5] * sizeof(float)));
#undef V_HIP
    hipLaunchKernelGGL(k_val_state_reset, dim3(1), dim3(64), 0, st, v->state);
    {
        hipError_t e_ = hipGetLastError();
        if (e_ != hipSuccess) {
            free_val(v);
            return lt_set_error(LT_ERR_HIP, "%s: kernel launch failed: %s", who, hipGetErrorString(e_));
        }
    }
    t->val = v;
    return LT_OK;
}

// The epoch's forward on the validation graph with dropout off: the forward's launches at n2, its logits' bits.
static int val_forward(lt_trainer *t, hipStream_t st) {
    lt_val *v = t->val;
    const bool front = t->layers == 3;
    int rc = launch_xw1(t, v->X, v->ldx, v->n, v->kslice, v->slabs, front ? v->fS : v->S, st);
    if (rc) return rc;
    if (t->wide) {      // v->Z: the top chain's hidden layer
        if (front) {
            rc = launch_front(t, v->g, v->fS, drop_off(), v->fH, v->seg_part, v->S, st);
            if (rc) return rc;
        }
        return launch_wide_forward(t, v->g, v->S, drop_off(), v->Z, v->Sc, v->Zc, v->seg_part, st);
    }
    float *Z = v->Z;
    if (front) {
        lt_drop_args off;
        off.on = 0; off.thresh = 0; off.scale = 1.f; off.epoch = 0; off.seed = 0;
        rc = launch_front(t, v->g, v->fS, off, v->fH, v->seg_part, v->S, st);
        if (rc) return rc;
    } else if (!lt_tiled_wanted(v->g, t->Hp[0])) {
        Z = nullptr;      // only the tiled layer-1 route needs it
    }
    return launch_top_forward(t, v->g, v->S, Z, nullptr, nullptr, v->Sc, v->Zc, v->seg_part, st);
}

// head, state and snapshot behind a validation forward; e = the epoch just trained (0-based, since creation)
static int val_finish_epoch(const lt_trainer *t, lt_val *v, int C, const lt_snap_segs &T, int64_t e, float *val_loss,
                            int32_t *val_counts, hipStream_t st) {
    const int rc = t->wide ? launch_trw_head(t->loss_kind, v->Zc, (long)t->Cp, v->labels, (long)v->ldy, v->n, C, v->rows, v->m,
                                             nullptr, v->part_loss, val_loss, nullptr, val_counts, nullptr, v->state, v->patience,
                                             (int)e, st)
                           : launch_val_head(v->Zc, (long)C, v->labels, v->n, C, v->rows, v->m, v->part_loss, v->part_cnt, val_loss,
                                             val_counts, nullptr, v->state, v->patience, (int)e, st);
    if (rc) return rc;
    if (v->keep_best) return launch_snapshot(T, v->snap, v->state + VS_IMPROVED, 0, st);
    return LT_OK;
}

// --------------------------------------------------------------------------------------------
// the entry points' bodies; `who` is the public name the messages carry
// --------------------------------------------------------------------------------------------
// lt_gcn*_trainer_run (val_loss == val_counts == NULL, validated = false) and _run_validated
static int trainer_run(const char *who, lt_trainer *t, int32_t n_epochs, float *record, bool validated, float *val_loss,
                       int32_t *val_counts, void *stream) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    if (validated) {
        LT_REQUIRE(t->val != nullptr, "%s: no validation attached", who);
    }
    LT_REQUIRE(n_epochs >= 0, "%s: n_epochs=%d", who, n_epochs);
    if (n_epochs == 0) return LT_OK;
    if (validated) {
        LT_REQUIRE(record && val_loss && val_counts, "%s: NULL output", who);
        LT_REQUIRE(t->epoch + n_epochs <= (int64_t)INT32_MAX, "%s: epoch counter would pass 2^31", who);
    } else {
        LT_REQUIRE(record != nullptr, "%s: record is NULL", who);
        LT_REQUIRE(t->epoch + n_epochs <= (int64_t)UINT32_MAX, "%s: epoch counter would pass 2^32", who);
    }
    hipStream_t st = (hipStream_t)stream;
    const lt_snap_segs T = snap_segs(t);
    // the borrowed parameters may have changed since the last run: the padded copies from them (Adam keeps them current after that)
    if (t->wide && t->layers == 3) {
        const int mh = t->Hp[0] > t->Hp[1] ? t->Hp[0] : t->Hp[1], mx = mh > t->Cp ? mh : t->Cp;
        hipLaunchKernelGGL(k_tr3w_pad, dim3((mx + 255) / 256), dim3(256), 0, st, t->P[1], t->H[0], t->Hp[0], t->P[3], t->H[1],
                           t->Hp[1], t->P[5], t->C, t->Cp, t->mir[1], t->mir[3], t->mir[5]);
    } else if (t->wide) {      // b1 at Hp and b2 at Cp: k_tr3_pad's first two copies (its third, over Hp2 * 0 elements, is empty)
        const int mx = t->Hp[0] > t->Cp ? t->Hp[0] : t->Cp;
        hipLaunchKernelGGL(k_tr3_pad, dim3((mx + 255) / 256), dim3(256), 0, st, t->P[1], t->H[0], t->Hp[0], t->P[3], t->C, t->Cp,
                           nullptr, 0, t->mir[1], t->mir[3], nullptr);
    } else if (t->layers == 3) {
        const int mx = t->Hp[0] > t->Hp[1] * t->C ? t->Hp[0] : t->Hp[1] * t->C;
        hipLaunchKernelGGL(k_tr3_pad, dim3((mx + 255) / 256), dim3(256), 0, st, t->P[1], t->H[0], t->Hp[0], t->P[3], t->H[1],
                           t->Hp[1], t->P[4], t->C, t->mir[1], t->mir[3], t->mir[4]);
    } else {
        hipLaunchKernelGGL(k_tr_pad, dim3((t->Hp[0] * (t->C + 1) + 255) / 256), dim3(256), 0, st, t->P[1], t->P[2], t->H[0],
                           t->Hp[0], t->C, t->mir[1], t->mir[2]);
    }
    LT_CHECK_LAUNCH();
    const size_t cc = t->wide ? 3 * (size_t)t->C : (size_t)t->C * t->C;      // an epoch's val_counts
    for (int32_t j = 0; j < n_epochs; ++j) {
        const int64_t e = t->epoch;
        int rc = run_epoch(t, record + 2 * (size_t)j, st);
        if (rc == LT_OK && validated) rc = val_forward(t, st);
        if (rc == LT_OK && validated) rc = val_finish_epoch(t, t->val, t->C, T, e, val_loss + j, val_counts + cc * (size_t)j, st);
        if (rc) return rc;
    }
    return LT_OK;
}

// the last epoch's gradients: dst[k] takes segment k of the gradient buffer
static int trainer_grads(const lt_trainer *t, float *const *dst, void *stream) {
    for (int k = 0; k < 2 * t->layers; ++k) {
        const int64_t b = k ? t->off[k - 1] : 0;
        LT_HIP(hipMemcpyAsync(dst[k], t->grad + b, (size_t)(t->off[k] - b) * sizeof(float), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
    }
    return LT_OK;
}

// rows of width floats from a trainer buffer of leading dimension lds into dst [n, ld]
static int copy_rows(float *dst, int64_t ld, const float *src, int lds, int width, int n, void *stream) {
    LT_HIP(hipMemcpy2DAsync(dst, (size_t)ld * sizeof(float), src, (size_t)lds * sizeof(float), (size_t)width * sizeof(float),
                            (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

static int trainer_logits(const char *who, const lt_trainer *t, float *Z, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr && Z != nullptr, "%s: NULL argument", who);
    LT_REQUIRE(ldz >= t->C, "%s: ldz=%lld < C=%d", who, (long long)ldz, t->C);
    return copy_rows(Z, ldz, t->Zc, trainer_ldc(t), t->C, t->n, stream);
}

static int trainer_epoch(const char *who, const lt_trainer *t, int64_t *epoch) {
    LT_REQUIRE(t != nullptr && epoch != nullptr, "%s: NULL argument", who);
    *epoch = t->epoch;
    return LT_OK;
}

static int trainer_val_state(const char *who, const lt_trainer *t, int32_t *state_host, void *stream) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    LT_REQUIRE(t->val != nullptr, "%s: no validation attached", who);
    LT_REQUIRE(state_host != nullptr, "%s: state is NULL", who);
    hipStream_t st = (hipStream_t)stream;
    LT_HIP(hipMemcpyAsync(state_host, t->val->state, VAL_STATE_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    LT_HIP(hipStreamSynchronize(st));
    return LT_OK;
}

static int trainer_restore_best(const char *who, lt_trainer *t, void *stream) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    LT_REQUIRE(t->val != nullptr && t->val->keep_best, "%s: no validation with keep_best attached", who);
    return launch_snapshot(snap_segs(t), t->val->snap, t->val->state + VS_SEEN, 1, (hipStream_t)stream);
}

static int trainer_val_logits(const char *who, const lt_trainer *t, float *Z, int64_t ldz, void *stream) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    LT_REQUIRE(t->val != nullptr, "%s: no validation attached", who);
    LT_REQUIRE(Z != nullptr, "%s: Z is NULL", who);
    LT_REQUIRE(ldz >= t->C, "%s: ldz=%lld < C=%d", who, (long long)ldz, t->C);
    return copy_rows(Z, ldz, t->val->Zc, trainer_ldc(t), t->C, t->val->n, stream);
}

// lt_gcn*_trainer_set_train_rows.  Everything that can refuse comes first -- the checks of the host list, the allocations, the
// copy -- so a refused call leaves the trainer as it was.  Then dZc is zeroed (the listed head writes listed rows only, and
// the backward reads every row) and the new list replaces the old one.
static int trainer_set_train_rows(const char *who, lt_trainer *t, const int32_t *rows, int32_t m, void *stream) {
    LT_REQUIRE(t != nullptr, "%s: trainer is NULL", who);
    LT_REQUIRE(m >= 0, "%s: m=%d, must be >= 0 (0: all rows)", who, m);
    LT_REQUIRE(m <= t->n, "%s: m=%d ids, the graph has n=%d rows", who, m, t->n);
    hipStream_t st = (hipStream_t)stream;
    // an old list may still be read by epochs in flight on any stream: wait for the device before it is replaced and freed
    // (before anything is allocated, so a failure here leaves nothing behind)
    if (t->train_rows) LT_HIP(hipDeviceSynchronize());
    int32_t *drows = nullptr;
    float *lhead = nullptr;
    if (m > 0) {
        LT_REQUIRE(rows != nullptr, "%s: rows is NULL with m=%d", who, m);
        const int n = t->n;
        uint8_t *seen = new (std::nothrow) uint8_t[(size_t)n]();
        if (!seen) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
        int bad = -1, rep = -1;
        for (int i = 0; i < m && bad < 0 && rep < 0; ++i) {
            const int32_t r = rows[i];
            if (r < 0 || r >= n) bad = i;
            else if (seen[r]) rep = i;
            else seen[r] = 1;
        }
        delete[] seen;
        LT_REQUIRE(bad < 0, "%s: rows[%d]=%d outside [0, %d)", who, bad, bad >= 0 ? rows[bad] : 0, n);
        LT_REQUIRE(rep < 0, "%s: rows[%d]=%d repeats an earlier id", who, rep, rep >= 0 ? rows[rep] : 0);
        hipError_t e = hipMalloc((void **)&drows, (size_t)m * sizeof(int32_t));
        if (e == hipSuccess && t->wide) e = hipMalloc((void **)&lhead, trw_part_bytes(m, t->C, true));
        if (e == hipSuccess) e = hipMemcpyAsync(drows, rows, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);      // the caller's array is its own again when this returns
        if (e == hipSuccess) e = hipMemsetAsync(t->dZc, 0, (size_t)n * trainer_ldc(t) * sizeof(float), st);
        if (e != hipSuccess) {
            (void)hipFree(drows);
            (void)hipFree(lhead);
            return lt_set_error(LT_ERR_HIP, "%s: setting up the list failed: %s", who, hipGetErrorString(e));
        }
    }
    (void)hipFree(t->train_rows);
    (void)hipFree(t->lhead);
    t->train_rows = drows;
    t->lhead = lhead;
    t->n_train = m;
    return LT_OK;
}

// ---- the 2-layer trainer ----
extern "C" int lt_gcn2_trainer_set_train_rows(lt_gcn2_trainer *t, const int32_t *rows, int32_t m, void *stream) {
    return trainer_set_train_rows("lt_gcn2_trainer_set_train_rows", t, rows, m, stream);
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
    const int32_t Hs[2] = {H, 0};
    float *const ps[4] = {W1, b1, W2, b2};
    lt_trainer *t = nullptr;
    const int rc = trainer_create("lt_gcn2_trainer_create", 2, g, X, ldx, F, labels, Hs, C, ps, lr, weight_decay, dropout, seed,
                                  stream, &t);
    *out = static_cast<lt_gcn2_trainer *>(t);
    return rc;
}

extern "C" int lt_gcn2_trainer_destroy(lt_gcn2_trainer *t) {
    free_trainer(t);
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_epoch(const lt_gcn2_trainer *t, int64_t *epoch) {
    return trainer_epoch("lt_gcn2_trainer_epoch", t, epoch);
}

extern "C" int lt_gcn2_trainer_run(lt_gcn2_trainer *t, int32_t n_epochs, float *record, void *stream) {
    return trainer_run("lt_gcn2_trainer_run", t, n_epochs, record, false, nullptr, nullptr, stream);
}

extern "C" int lt_gcn2_trainer_grads(const lt_gcn2_trainer *t, float *dW1, float *db1, float *dW2, float *db2, void *stream) {
    LT_REQUIRE(t != nullptr && dW1 && db1 && dW2 && db2, "lt_gcn2_trainer_grads: NULL argument");
    float *const dst[4] = {dW1, db1, dW2, db2};
    return trainer_grads(t, dst, stream);
}

extern "C" int lt_gcn2_trainer_logits(const lt_gcn2_trainer *t, float *Z2, int64_t ldz, void *stream) {
    return trainer_logits("lt_gcn2_trainer_logits", t, Z2, ldz, stream);
}

extern "C" int lt_gcn2_trainer_attach_validation(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                 int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                 void *stream) {
    return val_attach("lt_gcn2_trainer_attach_validation", t, g2, X2, ldx2, n2, labels2, keep_best, patience, stream);
}

extern "C" int lt_gcn2_trainer_attach_validation_rows(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                      const int32_t *rows, int32_t m, void *stream) {
    return val_attach("lt_gcn2_trainer_attach_validation_rows", t, g2, X2, ldx2, n2, labels2, keep_best, patience, stream, 1, rows,
                      m);
}

extern "C" int lt_gcn2_trainer_run_validated(lt_gcn2_trainer *t, int32_t n_epochs, float *record, float *val_loss,
                                             int32_t *val_counts, void *stream) {
    return trainer_run("lt_gcn2_trainer_run_validated", t, n_epochs, record, true, val_loss, val_counts, stream);
}

extern "C" int lt_gcn2_trainer_val_state(const lt_gcn2_trainer *t, int32_t *state, void *stream) {
    return trainer_val_state("lt_gcn2_trainer_val_state", t, state, stream);
}

extern "C" int lt_gcn2_trainer_restore_best(lt_gcn2_trainer *t, void *stream) {
    return trainer_restore_best("lt_gcn2_trainer_restore_best", t, stream);
}

extern "C" int lt_gcn2_trainer_val_logits(const lt_gcn2_trainer *t, float *Z, int64_t ldz, void *stream) {
    return trainer_val_logits("lt_gcn2_trainer_val_logits", t, Z, ldz, stream);
}

// ---- the 2-layer trainer with the wide head ----
extern "C" int lt_gcn2_trainer_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const void *labels,
                                           int64_t ldy, int32_t loss_kind, int32_t H, int32_t C, float *W1, float *b1, float *W2,
                                           float *b2, double lr, double weight_decay, double dropout, uint64_t seed, void *stream,
                                           lt_gcn2_trainer **out) {
    LT_REQUIRE(out != nullptr, "lt_gcn2_trainer_create_wide: out is NULL");
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "lt_gcn2_trainer_create_wide: graph is NULL");
    LT_REQUIRE(F > 0 && H > 0 && C > 0, "lt_gcn2_trainer_create_wide: F=%d H=%d C=%d must be positive", F, H, C);
    LT_REQUIRE(H <= LT_MAX_H, "lt_gcn2_trainer_create_wide: H=%d (supported: H <= %d)", H, LT_MAX_H);
    LT_REQUIRE(C <= LT_MAX_H, "lt_gcn2_trainer_create_wide: C=%d (supported: C <= %d)", C, LT_MAX_H);
    LT_REQUIRE(loss_kind == LT_LOSS_CE || loss_kind == LT_LOSS_BCE,
               "lt_gcn2_trainer_create_wide: loss_kind=%d, must be LT_LOSS_CE (0) or LT_LOSS_BCE (1)", loss_kind);
    if (loss_kind == LT_LOSS_BCE) LT_REQUIRE(ldy >= C, "lt_gcn2_trainer_create_wide: ldy=%lld < C=%d", (long long)ldy, C);
    LT_REQUIRE(X && labels && W1 && b1 && W2 && b2, "lt_gcn2_trainer_create_wide: NULL tensor pointer");
    const int32_t Hs[2] = {H, 0};
    float *const ps[4] = {W1, b1, W2, b2};
    lt_trainer *t = nullptr;
    const int rc = trainer_create("lt_gcn2_trainer_create_wide", 2, g, X, ldx, F, static_cast<const int32_t *>(labels), Hs, C, ps, lr,
                                  weight_decay, dropout, seed, stream, &t, 1, loss_kind, ldy);
    *out = static_cast<lt_gcn2_trainer *>(t);
    return rc;
}

static int trainer_counts_out(const char *who, const lt_trainer *t, int32_t *counts, void *stream) {
    LT_REQUIRE(t != nullptr && counts != nullptr, "%s: NULL argument", who);
    LT_REQUIRE(t->wide, "%s: the trainer has the narrow head, which keeps no per-class counts", who);
    LT_REQUIRE(t->epoch > 0, "%s: no epoch has run", who);
    LT_HIP(hipMemcpyAsync(counts, trainer_counts(t), 3 * (size_t)t->C * sizeof(int32_t), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return LT_OK;
}

extern "C" int lt_gcn2_trainer_counts(const lt_gcn2_trainer *t, int32_t *counts, void *stream) {
    return trainer_counts_out("lt_gcn2_trainer_counts", t, counts, stream);
}

extern "C" int lt_gcn2_trainer_hidden(const lt_gcn2_trainer *t, float *H1d, int64_t ld, void *stream) {
    LT_REQUIRE(t != nullptr && H1d != nullptr, "lt_gcn2_trainer_hidden: NULL argument");
    LT_REQUIRE(ld >= t->H[0], "lt_gcn2_trainer_hidden: ld=%lld < H=%d", (long long)ld, t->H[0]);
    return copy_rows(H1d, ld, t->Hd, t->Hp[0], t->H[0], t->n, stream);
}

extern "C" int lt_gcn2_trainer_attach_validation_wide(lt_gcn2_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const void *labels2, int64_t ldy2, int32_t keep_best,
                                                      int32_t patience, const int32_t *rows, int32_t m, void *stream) {
    return val_attach("lt_gcn2_trainer_attach_validation_wide", t, g2, X2, ldx2, n2, static_cast<const int32_t *>(labels2),
                      keep_best, patience, stream, rows != nullptr, rows, m, 1, ldy2);
}

extern "C" size_t lt_eval_head_wide_workspace_bytes(int32_t m, int32_t C) {
    if (m <= 0 || C <= 0 || C > LT_MAX_H) return 0;
    return trw_part_bytes(m, C, false);
}

extern "C" int lt_eval_head_wide(const float *Z, int64_t ldz, const void *labels, int64_t ldy, int32_t n, int32_t C,
                                 int32_t loss_kind, const int32_t *rows, int32_t m, float *loss, int32_t *counts, int32_t *n_bad,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    LT_REQUIRE(n > 0, "lt_eval_head_wide: n=%d, must be positive", n);
    LT_REQUIRE(C > 0 && C <= LT_MAX_H, "lt_eval_head_wide: C=%d (supported: 1 .. %d)", C, LT_MAX_H);
    LT_REQUIRE(loss_kind == LT_LOSS_CE || loss_kind == LT_LOSS_BCE,
               "lt_eval_head_wide: loss_kind=%d, must be LT_LOSS_CE (0) or LT_LOSS_BCE (1)", loss_kind);
    LT_REQUIRE(Z && labels && loss && counts, "lt_eval_head_wide: NULL pointer");
    LT_REQUIRE(ldz >= C, "lt_eval_head_wide: ldz=%lld < C=%d", (long long)ldz, C);
    if (loss_kind == LT_LOSS_BCE) LT_REQUIRE(ldy >= C, "lt_eval_head_wide: ldy=%lld < C=%d", (long long)ldy, C);
    if (rows) LT_REQUIRE(m > 0, "lt_eval_head_wide: m=%d, must be positive", m);
    const size_t need = trw_part_bytes(rows ? m : n, C, false);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace % sizeof(float)))
        return lt_set_error(LT_ERR_WORKSPACE, "lt_eval_head_wide: workspace needs %zu bytes, 4-byte aligned", need);
    hipStream_t st = (hipStream_t)stream;
    if (n_bad) LT_HIP(hipMemsetAsync(n_bad, 0, sizeof(int32_t), st));
    return launch_trw_head(loss_kind, Z, (long)ldz, labels, (long)ldy, n, C, rows, m, nullptr, (float *)workspace, loss, nullptr,
                           counts, n_bad, nullptr, 0, 0, st);
}

// ---- the 3-layer trainer ----
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
    const int32_t Hs[2] = {H1, H2};
    float *const ps[6] = {W1, b1, W2, b2, W3, b3};
    lt_trainer *t = nullptr;
    const int rc = trainer_create("lt_gcn3_trainer_create", 3, g, X, ldx, F, labels, Hs, C, ps, lr, weight_decay, dropout, seed,
                                  stream, &t);
    *out = static_cast<lt_gcn3_trainer *>(t);
    return rc;
}

// ---- the 3-layer trainer with the wide head ----
extern "C" int lt_gcn3_trainer_create_wide(const lt_graph *g, const float *X, int64_t ldx, int32_t F, const void *labels,
                                           int64_t ldy, int32_t loss_kind, int32_t H1, int32_t H2, int32_t C, float *W1, float *b1,
                                           float *W2, float *b2, float *W3, float *b3, double lr, double weight_decay,
                                           double dropout, uint64_t seed, void *stream, lt_gcn3_trainer **out) {
    LT_REQUIRE(out != nullptr, "lt_gcn3_trainer_create_wide: out is NULL");
    *out = nullptr;
    LT_REQUIRE(g != nullptr, "lt_gcn3_trainer_create_wide: graph is NULL");
    LT_REQUIRE(F > 0 && H1 > 0 && H2 > 0 && C > 0, "lt_gcn3_trainer_create_wide: F=%d H1=%d H2=%d C=%d must be positive", F, H1,
               H2, C);
    LT_REQUIRE(H1 <= LT_MAX_H && H2 <= LT_MAX_H, "lt_gcn3_trainer_create_wide: H1=%d H2=%d (supported: H1, H2 <= %d)", H1, H2,
               LT_MAX_H);
    LT_REQUIRE(C <= LT_MAX_H, "lt_gcn3_trainer_create_wide: C=%d (supported: C <= %d)", C, LT_MAX_H);
    LT_REQUIRE(loss_kind == LT_LOSS_CE || loss_kind == LT_LOSS_BCE,
               "lt_gcn3_trainer_create_wide: loss_kind=%d, must be LT_LOSS_CE (0) or LT_LOSS_BCE (1)", loss_kind);
    if (loss_kind == LT_LOSS_BCE) LT_REQUIRE(ldy >= C, "lt_gcn3_trainer_create_wide: ldy=%lld < C=%d", (long long)ldy, C);
    LT_REQUIRE(X && labels && W1 && b1 && W2 && b2 && W3 && b3, "lt_gcn3_trainer_create_wide: NULL tensor pointer");
    const int32_t Hs[2] = {H1, H2};
    float *const ps[6] = {W1, b1, W2, b2, W3, b3};
    lt_trainer *t = nullptr;
    const int rc = trainer_create("lt_gcn3_trainer_create_wide", 3, g, X, ldx, F, static_cast<const int32_t *>(labels), Hs, C, ps, lr,
                                  weight_decay, dropout, seed, stream, &t, 1, loss_kind, ldy);
    *out = static_cast<lt_gcn3_trainer *>(t);
    return rc;
}

extern "C" int lt_gcn3_trainer_counts(const lt_gcn3_trainer *t, int32_t *counts, void *stream) {
    return trainer_counts_out("lt_gcn3_trainer_counts", t, counts, stream);
}

extern "C" int lt_gcn3_trainer_attach_validation_wide(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const void *labels2, int64_t ldy2, int32_t keep_best,
                                                      int32_t patience, const int32_t *rows, int32_t m, void *stream) {
    return val_attach("lt_gcn3_trainer_attach_validation_wide", t, g2, X2, ldx2, n2, static_cast<const int32_t *>(labels2),
                      keep_best, patience, stream, rows != nullptr, rows, m, 1, ldy2);
}

extern "C" int lt_gcn3_trainer_set_train_rows(lt_gcn3_trainer *t, const int32_t *rows, int32_t m, void *stream) {
    return trainer_set_train_rows("lt_gcn3_trainer_set_train_rows", t, rows, m, stream);
}

extern "C" int lt_gcn3_trainer_destroy(lt_gcn3_trainer *t) {
    free_trainer(t);
    return LT_OK;
}

extern "C" int lt_gcn3_trainer_epoch(const lt_gcn3_trainer *t, int64_t *epoch) {
    return trainer_epoch("lt_gcn3_trainer_epoch", t, epoch);
}

extern "C" int lt_gcn3_trainer_run(lt_gcn3_trainer *t, int32_t n_epochs, float *record, void *stream) {
    return trainer_run("lt_gcn3_trainer_run", t, n_epochs, record, false, nullptr, nullptr, stream);
}

extern "C" int lt_gcn3_trainer_grads(const lt_gcn3_trainer *t, float *dW1, float *db1, float *dW2, float *db2, float *dW3,
                                     float *db3, void *stream) {
    LT_REQUIRE(t != nullptr && dW1 && db1 && dW2 && db2 && dW3 && db3, "lt_gcn3_trainer_grads: NULL argument");
    float *const dst[6] = {dW1, db1, dW2, db2, dW3, db3};
    return trainer_grads(t, dst, stream);
}

extern "C" int lt_gcn3_trainer_logits(const lt_gcn3_trainer *t, float *Z3, int64_t ldz, void *stream) {
    return trainer_logits("lt_gcn3_trainer_logits", t, Z3, ldz, stream);
}

extern "C" int lt_gcn3_trainer_hidden(const lt_gcn3_trainer *t, int32_t layer, float *dst, int64_t ld, void *stream) {
    LT_REQUIRE(t != nullptr && dst != nullptr, "lt_gcn3_trainer_hidden: NULL argument");
    LT_REQUIRE(layer == 1 || layer == 2, "lt_gcn3_trainer_hidden: layer=%d, must be 1 or 2", layer);
    const int H = t->H[layer - 1];
    LT_REQUIRE(ld >= H, "lt_gcn3_trainer_hidden: ld=%lld < H%d=%d", (long long)ld, layer, H);
    return copy_rows(dst, ld, layer == 1 ? t->fHd : t->Hd, t->Hp[layer - 1], H, t->n, stream);
}

extern "C" int lt_gcn3_trainer_attach_validation(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                 int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                 void *stream) {
    return val_attach("lt_gcn3_trainer_attach_validation", t, g2, X2, ldx2, n2, labels2, keep_best, patience, stream);
}

extern "C" int lt_gcn3_trainer_attach_validation_rows(lt_gcn3_trainer *t, const lt_graph *g2, const float *X2, int64_t ldx2,
                                                      int32_t n2, const int32_t *labels2, int32_t keep_best, int32_t patience,
                                                      const int32_t *rows, int32_t m, void *stream) {
    return val_attach("lt_gcn3_trainer_attach_validation_rows", t, g2, X2, ldx2, n2, labels2, keep_best, patience, stream, 1, rows,
                      m);
}

extern "C" int lt_gcn3_trainer_run_validated(lt_gcn3_trainer *t, int32_t n_epochs, float *record, float *val_loss,
                                             int32_t *val_counts, void *stream) {
    return trainer_run("lt_gcn3_trainer_run_validated", t, n_epochs, record, true, val_loss, val_counts, stream);
}

extern "C" int lt_gcn3_trainer_val_state(const lt_gcn3_trainer *t, int32_t *state, void *stream) {
    return trainer_val_state("lt_gcn3_trainer_val_state", t, state, stream);
}

extern "C" int lt_gcn3_trainer_restore_best(lt_gcn3_trainer *t, void *stream) {
    return trainer_restore_best("lt_gcn3_trainer_restore_best", t, stream);
}

extern "C" int lt_gcn3_trainer_val_logits(const lt_gcn3_trainer *t, float *Z, int64_t ldz, void *stream) {
    return trainer_val_logits("lt_gcn3_trainer_val_logits", t, Z, ldz, stream);
}
