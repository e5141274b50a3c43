// The feature-only baselines: OneLayerMLP / SingleHiddenLayerMLP (reference gcn/models.py:91-120) trained as MLPTrainer
// (mlp_trainer.py) trains them -- Adam on minibatches of an epoch's row order -- as stream-ordered launches with no host
// synchronisation.  The rows of a batch are read out of X through the row list; X_b never exists in memory.
//
//   one step over the b rows `rows[0 .. b)` of the epoch's order (j = position inside the batch), depth 2:
//   Z1 slabs = X[rows] W1          k_mlp_gemm_gather     v_mfma_f32_32x32x2_f32, 64 x 64 tiles, A rows gathered on their way into
//                                                        LDS; K in slices of MLP_KSLICE columns, one slab per slice
//   H1d = drop(relu(Z1 + b1)),     k_mlp_rows_fwd        MLP_RPB rows per block: the slabs in slice order, then the bias; the Philox
//   Z2 = H1d W2 + b2,                                    mask of element (j, h) of step s; the class layer as one fmaf chain per
//   loss, tp, dZ2                                        (row, class); the head a wave per row (the row arithmetic of lt_train_common.hip.h)
//   dZ1 = [H1d > 0] (dZ2 W2^T) / (1 - p)   k_mlp_rows_bwd   one fmaf chain over the classes per (row, hidden unit)
//   dW2, db2, db1 slabs            k_mlp_colgrads        one thread per output, the rows of a chunk of MLP_CHUNK in four interleaved
//                                                        chains
//   dW1 slabs = X[rows]^T dZ1      k_mlp_gemm_tn_gather  k_gemm_tn_mfma's structure (lt_train.hip), the k-rows gathered; one slab per chunk
//   grads, Adam, the step's record k_mlp_adam            the chunks' slabs in chunk order, adam_elem; block 0 adds the loss partials
//   depth 1: Z = X[rows] W + b through the same kernels (no hidden stage, no dZ1; dW = X[rows]^T dZ).
//
// Every sum has a fixed order and the cut of every launch is a function of the step's shapes alone (no float atomics): two
// trainers agree bit for bit and run(a + b) equals run(a); run(b).  lt_mlp_forward runs the first two kernels with the mask off:
// its logits of a row are the bits a p = 0 step forms for that row.
// Built with -ffp-contract=off: the only fused operations are explicit fmaf calls and the MFMAs.
#include <math.h>

#include <new>

#include "lt_radix.hip.h"
#include "lt_train_common.hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

#define MLP_BLOCK 256
#define MLP_RPB 16        // rows of a batch per block of the row passes
#define MLP_LD 256        // their LDS rows: LT_MAX_H = the widest class layer
#define MLP_CHUNK 512     // rows of a batch per gradient slab
#define MLP_KSLICE 512    // columns of X per forward slab (a multiple of the k-tile)

// row j of a batch: the node it names.  An id outside [0, n) is never an address: row 0 stands in and the flag word is raised.
__device__ __forceinline__ int mlp_row(const int32_t *rows, int j, int n, int32_t *err) {
    if (!rows) return j;
    int r = rows[j];
    if ((unsigned)r >= (unsigned)n) {
        if (err) *err = 1;
        r = 0;
    }
    return r;
}

// --------------------------------------------------------------------------------------------
// C[M, N] (slab blockIdx.z) = A[rows[0 .. M), kb .. ke) B[kb .. ke, N): the forward's product over gathered rows
// --------------------------------------------------------------------------------------------
#define MG_BM 64
#define MG_BN 64
#define MG_BK 16
#define MG_LDA (MG_BK + 1)
__global__ __launch_bounds__(256) void k_mlp_gemm_gather(const float *__restrict__ A, long lda, const int32_t *__restrict__ rows,
                                                         int n_a, int32_t *err, const float *__restrict__ B, long ldb,
                                                         float *__restrict__ C, long ldc, int M, int N, int K, int kslice,
                                                         long slab_stride) {
    __shared__ __attribute__((aligned(16))) float As[2][MG_BM * MG_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][MG_BK * MG_BN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int m0 = blockIdx.x * MG_BM, n0 = blockIdx.y * MG_BN;
    const int a_m = tid >> 2, a_k = (tid & 3) * 4;      // A tile: row a_m, k columns a_k .. a_k + 3
    const int b_row = tid >> 4, b_col = (tid & 15) * 4;
    const bool a_ok = m0 + a_m < M;
    const bool b_full = (n0 + b_col + 3) < N;
    const int ar = a_ok ? mlp_row(rows, m0 + a_m, n_a, (blockIdx.y | blockIdx.z) == 0 ? err : nullptr) : 0;
    const float *a_ptr = A + (long)ar * lda + a_k;
    const float *b_ptr = B + (long)b_row * ldb + n0 + b_col;
    const int kb = blockIdx.z * kslice;
    const int ke = min(K, kb + kslice);
    C += (long)blockIdx.z * slab_stride;

    f32x4 ra, rb;
    auto load_tiles = [&](int k0) {
        ra = f32x4{0.f, 0.f, 0.f, 0.f};
        rb = f32x4{0.f, 0.f, 0.f, 0.f};
        if (a_ok) {
            const float *p = a_ptr + k0;
            if (k0 + a_k + 3 < ke) {
                ra = *reinterpret_cast<const f32x4u *>(p);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + a_k + j < ke) ra[j] = p[j];
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
        float *as = &As[buf][a_m * MG_LDA + a_k];
        as[0] = ra.x; as[1] = ra.y; as[2] = ra.z; as[3] = ra.w;
        *reinterpret_cast<f32x4 *>(&Bs[buf][b_row * MG_BN + b_col]) = rb;
    };

    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    const int nk = (ke - kb + MG_BK - 1) / MG_BK;
    if (nk > 0) {
        load_tiles(kb);
        store_tiles(0);
    }
    __syncthreads();
    const int a_frag = (wr * 32 + (lane & 31)) * MG_LDA + (lane >> 5);
    const int b_frag = (lane >> 5) * MG_BN + wc * 32 + (lane & 31);
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles(kb + (kt + 1) * MG_BK);
        const float *as = &As[buf][a_frag];
        const float *bs = &Bs[buf][b_frag];
#pragma unroll
        for (int kk = 0; kk < MG_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk], bs[kk * MG_BN], acc, 0, 0, 0);
        if (kt + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }
    // C/D layout of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const int cn = n0 + wc * 32 + (lane & 31);
    if (cn < N) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int cm = m0 + wr * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
            if (cm < M) C[(long)cm * ldc + cn] = acc[reg];
        }
    }
}

// --------------------------------------------------------------------------------------------
// C[M, N] (slab blockIdx.z) = A[rows[kb .. ke), M]^T B[kb .. ke, N): dW1 = X_b^T dZ1 over gathered rows (M = F, K = b)
// --------------------------------------------------------------------------------------------
#define MT_FOLD 128
__global__ __launch_bounds__(256) void k_mlp_gemm_tn_gather(const float *__restrict__ A, long lda,
                                                            const int32_t *__restrict__ rows, int n_a,
                                                            const float *__restrict__ B, long ldb, float *__restrict__ C, long ldc,
                                                            int M, int N, int K, int kslice, long slab_stride) {
    __shared__ __attribute__((aligned(16))) float As[2][MG_BM * MG_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][MG_BK * MG_BN];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;
    const int m0 = blockIdx.x * MG_BM, n0 = blockIdx.y * MG_BN;
    const int a_k = tid >> 4, a_m = (tid & 15) * 4;   // A^T tile: k-row a_k, m columns a_m .. a_m + 3
    const int b_row = tid >> 4, b_col = (tid & 15) * 4;
    const bool a_full = (m0 + a_m + 3) < M;
    const bool b_full = (n0 + b_col + 3) < N;
    const float *b_ptr = B + (long)b_row * ldb + n0 + b_col;
    const int kb = blockIdx.z * kslice;
    const int ke = min(K, kb + kslice);
    C += (long)blockIdx.z * slab_stride;

    f32x4 ra, rb;
    auto load_tiles = [&](int k0) {
        ra = f32x4{0.f, 0.f, 0.f, 0.f};
        rb = f32x4{0.f, 0.f, 0.f, 0.f};
        if (k0 + a_k < ke) {
            const float *p = A + (long)mlp_row(rows, k0 + a_k, n_a, nullptr) * lda + m0 + a_m;
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
        float *as = &As[buf][a_m * MG_LDA + a_k];
        as[0] = ra.x; as[MG_LDA] = ra.y; as[2 * MG_LDA] = ra.z; as[3 * MG_LDA] = ra.w;
        *reinterpret_cast<f32x4 *>(&Bs[buf][b_row * MG_BN + b_col]) = rb;
    };

    f32x16 acc, total;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[i] = 0.f; total[i] = 0.f; }
    const int nk = (ke - kb + MG_BK - 1) / MG_BK;
    if (nk > 0) {
        load_tiles(kb);
        store_tiles(0);
    }
    __syncthreads();
    const int a_frag = (wr * 32 + (lane & 31)) * MG_LDA + (lane >> 5);
    const int b_frag = (lane >> 5) * MG_BN + wc * 32 + (lane & 31);
    constexpr int FOLD_TILES = MT_FOLD / MG_BK;
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) load_tiles(kb + (kt + 1) * MG_BK);
        const float *as = &As[buf][a_frag];
        const float *bs = &Bs[buf][b_frag];
#pragma unroll
        for (int kk = 0; kk < MG_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(as[kk], bs[kk * MG_BN], acc, 0, 0, 0);
        if ((kt + 1) % FOLD_TILES == 0) {
            total += acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        }
        if (kt + 1 < nk) store_tiles(buf ^ 1);
        __syncthreads();
    }
    total += acc;
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
// The forward's row pass: hidden layer, class layer, loss head
// --------------------------------------------------------------------------------------------
struct lt_mlp_fwd_args {
    int b, n, depth, H, C, nslab;
    long slab_stride;
    const float *slabs;        // [nslab][b, H] (depth 2) / [nslab][b, C] (depth 1)
    const float *b1, *W2, *b2; // depth 1: b2 is the layer's bias, the others are not read
    lt_drop_args d;            // d.epoch carries the step
    float *H1d;                // [b, H] or NULL
    float *Z;                  // logits [b, ldz] or NULL
    long ldz;
    // the head (labels == NULL: none)
    const int32_t *rows;
    const void *labels;
    long ldy;
    float inv;                 // 1 / b (CE), 1 / (b C) (BCE)
    float *dZ;                 // [b, C]
    float *part_loss;          // [blocks]
    int32_t *part_tp;          // [blocks]
};

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int LOSS>
__global__ __launch_bounds__(MLP_BLOCK) void k_mlp_rows_fwd(lt_mlp_fwd_args a) {
    __shared__ float sh[MLP_RPB * MLP_LD];
    __shared__ float sz[MLP_RPB * MLP_LD];
    __shared__ float sl[MLP_RPB];
    __shared__ int stp[MLP_RPB];
    const int t = threadIdx.x, j0 = blockIdx.x * MLP_RPB;
    const int nr = min(MLP_RPB, a.b - j0);
    const int H = a.H, C = a.C;
    if (a.depth == 2) {
        for (int idx = t; idx < nr * H; idx += MLP_BLOCK) {
            const int r = idx / H, h = idx - r * H;
            const size_t e = (size_t)(j0 + r) * H + h;
            float z = a.slabs[e];
            for (int s = 1; s < a.nslab; ++s) z += a.slabs[(size_t)s * a.slab_stride + e];
            z += a.b1[h];
            float v = fmaxf(z, 0.f);
            if (a.d.on) {
                const uint4 w = lt_drop_block((uint64_t)e >> 2, a.d.epoch, a.d.seed, 0u);
                const uint32_t sel = (uint32_t)(e & 3);
                const uint32_t u = sel == 0 ? w.x : sel == 1 ? w.y : sel == 2 ? w.z : w.w;
                v = (uint64_t)u >= a.d.thresh ? v * a.d.scale : 0.f;
            }
            if (a.H1d) a.H1d[e] = v;
            sh[r * MLP_LD + h] = v;
        }
        __syncthreads();
        for (int idx = t; idx < nr * C; idx += MLP_BLOCK) {
            const int r = idx / C, c = idx - r * C;
            const float *hr = &sh[r * MLP_LD];
            float acc = 0.f;
            for (int h = 0; h < H; ++h) acc = fmaf(hr[h], a.W2[(size_t)h * C + c], acc);
            sz[r * MLP_LD + c] = acc + a.b2[c];
        }
    } else {
        for (int idx = t; idx < nr * C; idx += MLP_BLOCK) {
            const int r = idx / C, c = idx - r * C;
            const size_t e = (size_t)(j0 + r) * C + c;
            float z = a.slabs[e];
            for (int s = 1; s < a.nslab; ++s) z += a.slabs[(size_t)s * a.slab_stride + e];
            sz[r * MLP_LD + c] = z + a.b2[c];
        }
    }
    __syncthreads();
    if (a.Z) {
        for (int idx = t; idx < nr * C; idx += MLP_BLOCK) {
            const int r = idx / C, c = idx - r * C;
            a.Z[(size_t)(j0 + r) * a.ldz + c] = sz[r * MLP_LD + c];
        }
    }
    if (!a.labels) return;
    const int lane = t & 63;
    for (int r = t >> 6; r < MLP_RPB; r += MLP_BLOCK / 64) {      // a wave per row; r is uniform over the wave
        float l = 0.f;
        int tp = 0;
        if (r < nr) {
            const int j = j0 + r;
            const int node = mlp_row(a.rows, j, a.n, nullptr);
            const float *zr = &sz[r * MLP_LD];
            float *dz = a.dZ + (size_t)j * C;
            if constexpr (LOSS == LT_LOSS_CE) {
                const int y = static_cast<const int32_t *>(a.labels)[node];
                float mx = -INFINITY;
                int arg = 0x7fffffff;
                for (int c = lane; c < C; c += 64) {
                    const float v = zr[c];
                    if (v > mx || arg == 0x7fffffff) { mx = v; arg = c; }
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const float omx = __shfl_xor(mx, m, 64);
                    const int oarg = __shfl_xor(arg, m, 64);
                    lt_argmax_merge(mx, arg, omx, oarg);
                }
                float s = 0.f;
                for (int c = lane; c < C; c += 64) s += expf(zr[c] - mx);
                s = wave_sum(s);
                const bool y_ok = (unsigned)y < (unsigned)C;
                l = lt_ce_row_loss(mx, s, y_ok ? zr[y] : 0.f);
                for (int c = lane; c < C; c += 64) dz[c] = lt_ce_grad(expf(zr[c] - mx), s, c == y, a.inv);
                tp = y_ok && arg == y;
            } else {
                const uint8_t *yr = static_cast<const uint8_t *>(a.labels) + (size_t)node * a.ldy;
                for (int c = lane; c < C; c += 64) {
                    const float zj = zr[c];
                    const bool yb = yr[c] != 0;
                    float sig;
                    l += lt_bce_elem(zj, yb, sig);
                    dz[c] = (sig - (yb ? 1.f : 0.f)) * a.inv;
                    tp += (zj > 0.f && yb) ? 1 : 0;
                }
                l = wave_sum(l);
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) tp += __shfl_xor(tp, m, 64);
            }
        }
        if (lane == 0) { sl[r] = l; stp[r] = tp; }
    }
    __syncthreads();
    if (t == 0) {
        float ls = 0.f;
        int tp = 0;
#pragma unroll
        for (int r = 0; r < MLP_RPB; ++r) { ls += sl[r]; tp += stp[r]; }
        a.part_loss[blockIdx.x] = ls;
        a.part_tp[blockIdx.x] = tp;
    }
}

// dZ1 = [H1d > 0] (dZ2 W2^T) scale
__global__ __launch_bounds__(MLP_BLOCK) void k_mlp_rows_bwd(int b, int H, int C, const float *__restrict__ dZ2,
                                                            const float *__restrict__ W2, const float *__restrict__ H1d,
                                                            float scale, float *__restrict__ dZ1) {
    __shared__ float sd[MLP_RPB * MLP_LD];
    const int t = threadIdx.x, j0 = blockIdx.x * MLP_RPB;
    const int nr = min(MLP_RPB, b - j0);
    for (int idx = t; idx < nr * C; idx += MLP_BLOCK) {
        const int r = idx / C, c = idx - r * C;
        sd[r * MLP_LD + c] = dZ2[(size_t)(j0 + r) * C + c];
    }
    __syncthreads();
    for (int idx = t; idx < nr * H; idx += MLP_BLOCK) {
        const int r = idx / H, h = idx - r * H;
        const float *w = W2 + (size_t)h * C;
        const float *dr = &sd[r * MLP_LD];
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(dr[c], w[c], acc);
        const size_t e = (size_t)(j0 + r) * H + h;
        dZ1[e] = H1d[e] > 0.f ? acc * scale : 0.f;
    }
}

// the column gradients of rows [chunk * MLP_CHUNK, ...) of the batch, one thread per output: dW2 = H1d^T dZ2, db2 and db1 the
// column sums of dZ2 and dZ1 (depth 1: db alone).  Row j adds into chain j & 3; the four chains are added as (0 + 1) + (2 + 3).
__global__ __launch_bounds__(MLP_BLOCK) void k_mlp_colgrads(int b, int depth, int H, int C, const float *__restrict__ H1d,
                                                            const float *__restrict__ dZ2, const float *__restrict__ dZ1,
                                                            float *__restrict__ slabs, long total, long o_b1, long o_W2,
                                                            long o_b2) {
    const int i = blockIdx.x * MLP_BLOCK + threadIdx.x;
    const int n_w2 = depth == 2 ? H * C : 0, n_out = depth == 2 ? n_w2 + C + H : C;
    if (i >= n_out) return;
    const int jb = blockIdx.y * MLP_CHUNK, je = min(b, jb + MLP_CHUNK);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    long out;
    if (i < n_w2) {
        const int h = i / C, c = i - h * C;
        const float *hp = H1d + h, *dp = dZ2 + c;
        int j = jb;
        for (; j + 3 < je; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmaf(hp[(size_t)(j + u) * H], dp[(size_t)(j + u) * C], acc[u]);
        }
        for (int u = 0; j < je; ++j, ++u) acc[u] = fmaf(hp[(size_t)j * H], dp[(size_t)j * C], acc[u]);
        out = o_W2 + i;
    } else {
        const bool is_b2 = i < n_w2 + C;
        const int col = is_b2 ? i - n_w2 : i - n_w2 - C, ld = is_b2 ? C : H;
        const float *p = (is_b2 ? dZ2 : dZ1) + col;
        int j = jb;
        for (; j + 3 < je; j += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] += p[(size_t)(j + u) * ld];
        }
        for (int u = 0; j < je; ++j, ++u) acc[u] += p[(size_t)j * ld];
        out = (is_b2 ? o_b2 : o_b1) + col;
    }
    slabs[(size_t)blockIdx.y * total + out] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// gradient = the chunks' slabs in chunk order (kept in G: the test accessor's view, before weight decay), then Adam; block 0
// also adds the head's partials (four interleaved chains over the blocks) into the step's record.
struct lt_mlp_adam_args {
    long total, o1, o2, o3;      // [0, o1) P0 | [o1, o2) P1 | [o2, o3) P2 | [o3, total) P3
    float *P0, *P1, *P2, *P3;
    const float *slabs;
    int nch;
    float *G, *m, *v;
    lt_adam_scalars s;
    int nblk;
    const float *part_loss;
    const int32_t *part_tp;
    float divisor;
    float *record;
};
__global__ __launch_bounds__(MLP_BLOCK) void k_mlp_adam(lt_mlp_adam_args a) {
    const long i = (long)blockIdx.x * MLP_BLOCK + threadIdx.x;
    if (i < a.total) {
        float g = a.slabs[i];
        for (int ch = 1; ch < a.nch; ++ch) g += a.slabs[(size_t)ch * a.total + i];
        a.G[i] = g;
        float *p = i < a.o1 ? a.P0 + i : i < a.o2 ? a.P1 + (i - a.o1) : i < a.o3 ? a.P2 + (i - a.o2) : a.P3 + (i - a.o3);
        float mi = a.m[i], vi = a.v[i];
        *p = adam_elem(*p, g, mi, vi, a.s);
        a.m[i] = mi;
        a.v[i] = vi;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float ls[4] = {0.f, 0.f, 0.f, 0.f};
        int tp = 0;
        for (int k = 0; k < a.nblk; ++k) {
            ls[k & 3] += a.part_loss[k];
            tp += a.part_tp[k];
        }
        a.record[0] = ((ls[0] + ls[1]) + (ls[2] + ls[3])) / a.divisor;
        a.record[1] = (float)tp;
    }
}

// the shuffle's keys: word 0 of Philox4x32-10, counter (r, 0, epoch, 2)
__global__ void k_mlp_keys(int n, uint32_t epoch, uint64_t seed, int32_t *__restrict__ key) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    key[r] = (int32_t)lt_philox4x32_10(make_uint4((uint32_t)r, 0u, epoch, 2u), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32))).x;
}

// --------------------------------------------------------------------------------------------
// host side
// --------------------------------------------------------------------------------------------
struct lt_mlp_trainer {
    int n = 0, F = 0, H = 0, C = 0, depth = 0, B = 0, bmax = 0, loss = 0;
    const float *X = nullptr;
    int64_t ldx = 0, ldy = 0;
    const void *labels = nullptr;
    float *P[4] = {nullptr, nullptr, nullptr, nullptr};
    long o1 = 0, o2 = 0, o3 = 0, total = 0;
    double lr = 0, wd = 0, p = 0;
    uint64_t seed = 0;
    int64_t steps = 0, epochs = 0;
    int last_b = 0, nslab = 0, nch_max = 0, nblk_max = 0, N1 = 0;      // N1: width of the first product (H, or C at depth 1)
    bool have_order = false;
    float *fslabs = nullptr, *H1d = nullptr, *Z = nullptr, *dZ2 = nullptr, *dZ1 = nullptr, *gslabs = nullptr, *G = nullptr,
          *m = nullptr, *v = nullptr, *part_loss = nullptr, *rec = nullptr;
    int32_t *part_tp = nullptr, *key[2] = {nullptr, nullptr}, *pay[2] = {nullptr, nullptr}, *hist = nullptr;
    int rounds = 0, rblk = 0;
};

static void mlp_free(lt_mlp_trainer *t) {
    if (!t) return;
    void *bufs[] = {t->fslabs, t->H1d, t->Z, t->dZ2, t->dZ1, t->gslabs, t->G, t->m, t->v, t->part_loss, t->rec, t->part_tp,
                    t->key[0], t->key[1], t->pay[0], t->pay[1], t->hist};
    for (void *b : bufs) (void)hipFree(b);
    delete t;
}

static lt_drop_args mlp_drop(double p, uint64_t seed, int64_t step, bool on) {
    lt_drop_args d;
    d.on = on && p > 0.0;
    d.thresh = (uint64_t)floor(p * 4294967296.0);
    d.scale = p < 1.0 ? (float)(1.0 / (1.0 - p)) : 0.f;
    d.epoch = (uint32_t)step;
    d.seed = seed;
    return d;
}

static int mlp_nslab(int F) { return (F + MLP_KSLICE - 1) / MLP_KSLICE; }

// the forward of m rows (rows == NULL: rows 0 .. m - 1): the gathered product, then the row pass whose arguments the caller began
static int mlp_launch_forward(const float *X, int64_t ldx, int n, int F, int depth, int N1, const float *W1, const int32_t *rows,
                              int m, float *fslabs, long slab_stride, int32_t *err, int loss, lt_mlp_fwd_args &a,
                              hipStream_t st) {
    const int nslab = mlp_nslab(F);
    const dim3 grid((unsigned)((m + MG_BM - 1) / MG_BM), (unsigned)((N1 + MG_BN - 1) / MG_BN), (unsigned)nslab);
    hipLaunchKernelGGL(k_mlp_gemm_gather, grid, dim3(256), 0, st, X, (long)ldx, rows, n, err, W1, (long)N1, fslabs, (long)N1, m, N1,
                       F, MLP_KSLICE, slab_stride);
    LT_CHECK_LAUNCH();
    a.b = m; a.n = n; a.depth = depth; a.nslab = nslab; a.slab_stride = slab_stride; a.slabs = fslabs; a.rows = rows;
    const dim3 rgrid((unsigned)((m + MLP_RPB - 1) / MLP_RPB));
    if (loss == LT_LOSS_BCE) hipLaunchKernelGGL(k_mlp_rows_fwd<LT_LOSS_BCE>, rgrid, dim3(MLP_BLOCK), 0, st, a);
    else hipLaunchKernelGGL(k_mlp_rows_fwd<LT_LOSS_CE>, rgrid, dim3(MLP_BLOCK), 0, st, a);
    LT_CHECK_LAUNCH();
    return LT_OK;
}

static int mlp_check_model(const char *who, int32_t F, int32_t depth, int32_t H, int32_t C) {
    LT_REQUIRE(depth == 1 || depth == 2, "%s: depth=%d (1 or 2)", who, depth);
    LT_REQUIRE(F >= 1, "%s: F=%d", who, F);
    LT_REQUIRE(depth == 1 || (H >= 1 && H <= LT_MAX_H), "%s: H=%d outside [1, %d]", who, H, LT_MAX_H);
    LT_REQUIRE(C >= 1 && C <= MLP_LD, "%s: C=%d outside [1, %d]", who, C, MLP_LD);
    return LT_OK;
}

extern "C" int lt_mlp_trainer_create(const float *X, int64_t ldx, int32_t n, int32_t F, const void *labels, int64_t ldy,
                                     int32_t loss_kind, int32_t depth, int32_t H, int32_t C, float *W1, float *b1, float *W2,
                                     float *b2, int32_t batch_size, double lr, double weight_decay, double dropout, uint64_t seed,
                                     void *stream, lt_mlp_trainer **out) {
    const char *who = "lt_mlp_trainer_create";
    LT_REQUIRE(out, "%s: out is NULL", who);
    *out = nullptr;
    if (int rc = mlp_check_model(who, F, depth, H, C)) return rc;
    LT_REQUIRE(X && labels && W1 && b1 && (depth == 1 || (W2 && b2)), "%s: NULL pointer", who);
    LT_REQUIRE(n >= 1, "%s: n=%d", who, n);
    LT_REQUIRE(ldx >= F, "%s: ldx=%lld < F=%d", who, (long long)ldx, F);
    LT_REQUIRE(batch_size >= 1, "%s: batch_size=%d < 1", who, batch_size);
    LT_REQUIRE(loss_kind == LT_LOSS_CE || loss_kind == LT_LOSS_BCE, "%s: loss_kind=%d", who, loss_kind);
    LT_REQUIRE(loss_kind == LT_LOSS_CE || ldy >= C, "%s: ldy=%lld < C=%d", who, (long long)ldy, C);
    LT_REQUIRE(dropout >= 0.0 && dropout <= 1.0, "%s: dropout=%g outside [0, 1]", who, dropout);
    LT_REQUIRE(lr >= 0.0 && weight_decay >= 0.0, "%s: lr=%g weight_decay=%g", who, lr, weight_decay);
    lt_mlp_trainer *t = new (std::nothrow) lt_mlp_trainer();
    if (!t) return lt_set_error(LT_ERR_NOMEM, "%s: out of host memory", who);
    t->n = n; t->F = F; t->H = depth == 2 ? H : 0; t->C = C; t->depth = depth; t->B = batch_size; t->loss = loss_kind;
    t->bmax = batch_size < n ? batch_size : n;
    t->X = X; t->ldx = ldx; t->labels = labels; t->ldy = ldy;
    t->P[0] = W1; t->P[1] = b1; t->P[2] = depth == 2 ? W2 : nullptr; t->P[3] = depth == 2 ? b2 : nullptr;
    t->N1 = depth == 2 ? H : C;
    t->o1 = (long)F * t->N1;
    if (depth == 2) { t->o2 = t->o1 + H; t->o3 = t->o2 + (long)H * C; t->total = t->o3 + C; }
    else { t->total = t->o1 + C; t->o2 = t->o3 = t->total; }
    t->lr = lr; t->wd = weight_decay; t->p = dropout; t->seed = seed;
    t->nslab = mlp_nslab(F);
    t->nch_max = (t->bmax + MLP_CHUNK - 1) / MLP_CHUNK;
    t->nblk_max = (t->bmax + MLP_RPB - 1) / MLP_RPB;
    lt_radix_plan(n, &t->rounds, &t->rblk);
    const size_t bm = (size_t)t->bmax, f4 = sizeof(float);
    struct { void **slot; size_t bytes; bool zero; } bufs[] = {
        {(void **)&t->fslabs, (size_t)t->nslab * bm * t->N1 * f4, false},
        {(void **)&t->H1d, depth == 2 ? bm * H * f4 : 0, false},
        {(void **)&t->dZ1, depth == 2 ? bm * H * f4 : 0, false},
        {(void **)&t->Z, bm * C * f4, false},
        {(void **)&t->dZ2, bm * C * f4, false},
        {(void **)&t->gslabs, (size_t)t->nch_max * t->total * f4, false},
        {(void **)&t->G, (size_t)t->total * f4, true},
        {(void **)&t->m, (size_t)t->total * f4, true},
        {(void **)&t->v, (size_t)t->total * f4, true},
        {(void **)&t->part_loss, (size_t)t->nblk_max * f4, false},
        {(void **)&t->part_tp, (size_t)t->nblk_max * sizeof(int32_t), false},
        {(void **)&t->rec, 2 * f4, true},
        {(void **)&t->key[0], (size_t)n * sizeof(int32_t), false},
        {(void **)&t->key[1], (size_t)n * sizeof(int32_t), false},
        {(void **)&t->pay[0], (size_t)n * sizeof(int32_t), false},
        {(void **)&t->pay[1], (size_t)n * sizeof(int32_t), false},
        {(void **)&t->hist, (size_t)256 * t->rblk * sizeof(int32_t), false},
    };
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipSuccess;
    const char *what = "hipMalloc";
    for (auto &b : bufs)
        if (b.bytes && e == hipSuccess) e = hipMalloc(b.slot, b.bytes);
    if (e == hipSuccess) what = "hipMemsetAsync";
    for (auto &b : bufs)
        if (b.bytes && b.zero && e == hipSuccess) e = hipMemsetAsync(*b.slot, 0, b.bytes, st);
    if (e != hipSuccess) {
        mlp_free(t);
        return lt_set_error(e == hipErrorOutOfMemory ? LT_ERR_NOMEM : LT_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
    }
    *out = t;
    return LT_OK;
}

extern "C" int lt_mlp_trainer_destroy(lt_mlp_trainer *t) {
    mlp_free(t);
    return LT_OK;
}

// one optimiser step over the b rows rows[0 .. b)
static int mlp_step(lt_mlp_trainer *t, const int32_t *rows, int b, float *record, hipStream_t st) {
    const int H = t->H, C = t->C, F = t->F, depth = t->depth, N1 = t->N1;
    lt_mlp_fwd_args a = {};
    a.H = H; a.C = C;
    a.b1 = depth == 2 ? t->P[1] : nullptr;
    a.W2 = t->P[2];
    a.b2 = depth == 2 ? t->P[3] : t->P[1];
    a.d = mlp_drop(t->p, t->seed, t->steps, depth == 2);
    a.H1d = t->H1d; a.Z = t->Z; a.ldz = C;
    a.labels = t->labels; a.ldy = t->ldy;
    const double terms = t->loss == LT_LOSS_BCE ? (double)b * C : (double)b;
    a.inv = t->loss == LT_LOSS_BCE ? (float)(1.0 / terms) : 1.0f / (float)b;
    a.dZ = t->dZ2; a.part_loss = t->part_loss; a.part_tp = t->part_tp;
    if (int rc = mlp_launch_forward(t->X, t->ldx, t->n, F, depth, N1, t->P[0], rows, b, t->fslabs, (long)t->bmax * N1,
                                    lt_node_err_dev(), t->loss, a, st))
        return rc;
    const unsigned nblk = (unsigned)((b + MLP_RPB - 1) / MLP_RPB), nch = (unsigned)((b + MLP_CHUNK - 1) / MLP_CHUNK);
    if (depth == 2) {
        hipLaunchKernelGGL(k_mlp_rows_bwd, dim3(nblk), dim3(MLP_BLOCK), 0, st, b, H, C, t->dZ2, t->P[2], t->H1d,
                           t->p < 1.0 ? (float)(1.0 / (1.0 - t->p)) : 0.f, t->dZ1);
        LT_CHECK_LAUNCH();
    }
    const int n_out = depth == 2 ? H * C + C + H : C;
    hipLaunchKernelGGL(k_mlp_colgrads, dim3((unsigned)((n_out + MLP_BLOCK - 1) / MLP_BLOCK), nch), dim3(MLP_BLOCK), 0, st, b, depth,
                       H, C, t->H1d, t->dZ2, t->dZ1, t->gslabs, t->total, t->o1, t->o2, depth == 2 ? t->o3 : t->o1);
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_mlp_gemm_tn_gather, dim3((unsigned)((F + MG_BM - 1) / MG_BM), (unsigned)((N1 + MG_BN - 1) / MG_BN), nch),
                       dim3(256), 0, st, t->X, (long)t->ldx, rows, t->n, depth == 2 ? t->dZ1 : t->dZ2, (long)N1, t->gslabs, (long)N1,
                       F, N1, b, MLP_CHUNK, t->total);
    LT_CHECK_LAUNCH();
    lt_mlp_adam_args g;
    g.total = t->total; g.o1 = t->o1; g.o2 = t->o2; g.o3 = t->o3;
    g.P0 = t->P[0]; g.P1 = t->P[1]; g.P2 = t->P[2]; g.P3 = t->P[3];
    g.slabs = t->gslabs; g.nch = (int)nch; g.G = t->G; g.m = t->m; g.v = t->v;
    g.s = adam_scalars(t->steps + 1, t->lr, 0.9, 0.999, 1e-8, t->wd);
    g.nblk = (int)nblk; g.part_loss = t->part_loss; g.part_tp = t->part_tp; g.divisor = (float)terms;
    g.record = record ? record : t->rec;
    hipLaunchKernelGGL(k_mlp_adam, dim3((unsigned)((t->total + MLP_BLOCK - 1) / MLP_BLOCK)), dim3(MLP_BLOCK), 0, st, g);
    LT_CHECK_LAUNCH();
    t->steps += 1;
    t->last_b = b;
    return LT_OK;
}

// the epoch's Philox order into pay[0]: keys, then four stable 8-bit passes (ties keep the row order)
static int mlp_shuffle(lt_mlp_trainer *t, hipStream_t st) {
    const int n = t->n;
    hipLaunchKernelGGL(k_mlp_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (uint32_t)t->epochs, t->seed, t->key[0]);
    LT_CHECK_LAUNCH();
    int cur = 0;
    for (int q = 0; q < 4; ++q) {
        hipLaunchKernelGGL(k_gb_radix_hist, dim3((unsigned)t->rblk), dim3(256), 0, st, t->key[cur], n, 8 * q, t->rounds, t->rblk, t->hist);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gb_scan, dim3(1), dim3(1024), 0, st, t->hist, (long long)256 * t->rblk);
        LT_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_gb_radix_scatter, dim3((unsigned)t->rblk), dim3(256), 0, st, t->key[cur],
                           q ? (const int32_t *)t->pay[cur] : (const int32_t *)nullptr, n, 8 * q, t->rounds, t->rblk, t->hist,
                           t->key[cur ^ 1], t->pay[cur ^ 1]);
        LT_CHECK_LAUNCH();
        cur ^= 1;
    }
    t->have_order = true;
    return LT_OK;
}

extern "C" int lt_mlp_trainer_run(lt_mlp_trainer *t, int32_t n_epochs, const int32_t *order, float *record, void *stream) {
    const char *who = "lt_mlp_trainer_run";
    LT_REQUIRE(t, "%s: NULL trainer", who);
    LT_REQUIRE(n_epochs >= 0, "%s: n_epochs=%d", who, n_epochs);
    if (int rc = lt_node_err_pending()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int spe = (t->n + t->B - 1) / t->B;
    for (int e = 0; e < n_epochs; ++e) {
        const int32_t *rows = order ? order + (size_t)e * t->n : t->pay[0];
        if (!order)
            if (int rc = mlp_shuffle(t, st)) return rc;
        for (int s = 0; s < spe; ++s) {
            const int off = s * t->B, b = t->n - off < t->B ? t->n - off : t->B;
            if (int rc = mlp_step(t, rows + off, b, record ? record + 2 * ((size_t)e * spe + s) : nullptr, st)) return rc;
        }
        t->epochs += 1;
    }
    return LT_OK;
}

extern "C" int lt_mlp_trainer_step(lt_mlp_trainer *t, const int32_t *rows, int32_t b, float *record, void *stream) {
    const char *who = "lt_mlp_trainer_step";
    LT_REQUIRE(t && rows, "%s: NULL pointer", who);
    LT_REQUIRE(b >= 1 && b <= t->bmax, "%s: b=%d outside [1, min(batch_size, n) = %d]", who, b, t->bmax);
    if (int rc = lt_node_err_pending()) return rc;
    return mlp_step(t, rows, b, record, (hipStream_t)stream);
}

extern "C" int lt_mlp_trainer_counts(const lt_mlp_trainer *t, int64_t *steps, int64_t *epochs, int32_t *last_rows) {
    LT_REQUIRE(t, "lt_mlp_trainer_counts: NULL trainer");
    if (steps) *steps = t->steps;
    if (epochs) *epochs = t->epochs;
    if (last_rows) *last_rows = t->last_b;
    return LT_OK;
}

extern "C" int lt_mlp_trainer_grads(const lt_mlp_trainer *t, float *dW1, float *db1, float *dW2, float *db2, void *stream) {
    const char *who = "lt_mlp_trainer_grads";
    LT_REQUIRE(t && dW1 && db1 && (t->depth == 1 || (dW2 && db2)), "%s: NULL pointer", who);
    LT_REQUIRE(t->steps > 0, "%s: no step has run", who);
    hipStream_t st = (hipStream_t)stream;
    float *dst[4] = {dW1, db1, dW2, db2};
    const long off[5] = {0, t->o1, t->o2, t->o3, t->total};
    for (int k = 0; k < (t->depth == 2 ? 4 : 2); ++k) {
        const long end = t->depth == 2 ? off[k + 1] : (k == 0 ? t->o1 : t->total);
        LT_HIP(hipMemcpyAsync(dst[k], t->G + off[k], (size_t)(end - off[k]) * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    return LT_OK;
}

extern "C" int lt_mlp_trainer_logits(const lt_mlp_trainer *t, float *Z, int64_t ldz, void *stream) {
    const char *who = "lt_mlp_trainer_logits";
    LT_REQUIRE(t && Z, "%s: NULL pointer", who);
    LT_REQUIRE(t->steps > 0, "%s: no step has run", who);
    LT_REQUIRE(ldz >= t->C, "%s: ldz=%lld < C=%d", who, (long long)ldz, t->C);
    LT_HIP(hipMemcpy2DAsync(Z, (size_t)ldz * sizeof(float), t->Z, (size_t)t->C * sizeof(float), (size_t)t->C * sizeof(float),
                            (size_t)t->last_b, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

extern "C" int lt_mlp_trainer_order(const lt_mlp_trainer *t, int32_t *order, void *stream) {
    const char *who = "lt_mlp_trainer_order";
    LT_REQUIRE(t && order, "%s: NULL pointer", who);
    LT_REQUIRE(t->have_order, "%s: no epoch has run under the Philox order", who);
    LT_HIP(hipMemcpyAsync(order, t->pay[0], (size_t)t->n * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return LT_OK;
}

extern "C" size_t lt_mlp_forward_workspace_bytes(int32_t m, int32_t F, int32_t depth, int32_t H, int32_t C) {
    if (m < 1 || F < 1 || (depth != 1 && depth != 2) || C < 1 || C > MLP_LD || (depth == 2 && (H < 1 || H > LT_MAX_H))) return 0;
    return (size_t)mlp_nslab(F) * (size_t)m * (size_t)(depth == 2 ? H : C) * sizeof(float);
}

extern "C" int lt_mlp_forward(const float *X2, int64_t ldx2, int32_t n2, int32_t F, int32_t depth, int32_t H, int32_t C,
                              const float *W1, const float *b1, const float *W2, const float *b2, const int32_t *rows, int32_t m,
                              float *Z, int64_t ldz, void *workspace, size_t workspace_bytes, void *stream) {
    const char *who = "lt_mlp_forward";
    if (int rc = mlp_check_model(who, F, depth, H, C)) return rc;
    LT_REQUIRE(X2 && W1 && b1 && (depth == 1 || (W2 && b2)) && Z, "%s: NULL pointer", who);
    LT_REQUIRE(n2 >= 1 && ldx2 >= F && ldz >= C, "%s: n2=%d ldx2=%lld ldz=%lld", who, n2, (long long)ldx2, (long long)ldz);
    const int cnt = rows ? m : n2;
    LT_REQUIRE(cnt >= 1, "%s: m=%d", who, m);
    if (int rc = lt_node_err_pending()) return rc;
    const size_t need = lt_mlp_forward_workspace_bytes(cnt, F, depth, H, C);
    if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15))
        return lt_set_error(LT_ERR_WORKSPACE, "%s: workspace of %zu bytes (16-byte aligned) needed, %zu given", who, need, workspace_bytes);
    const int N1 = depth == 2 ? H : C;
    lt_mlp_fwd_args a = {};
    a.H = depth == 2 ? H : 0; a.C = C;
    a.b1 = depth == 2 ? b1 : nullptr; a.W2 = W2; a.b2 = depth == 2 ? b2 : b1;
    a.d = mlp_drop(0.0, 0, 0, false);
    a.Z = Z; a.ldz = ldz;
    return mlp_launch_forward(X2, ldx2, n2, F, depth, N1, W1, rows, cnt, (float *)workspace, (long)cnt * N1, lt_node_err_dev(),
                              LT_LOSS_CE, a, (hipStream_t)stream);
}
