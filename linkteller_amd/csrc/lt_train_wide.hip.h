// The wide loss head of the 2-layer trainer (lt_gcn2_trainer_create_wide, lt_eval_head_wide): class width 1 <= C <= 256 with
// either of the reference's two losses (gcn_trainer.py:27-28, 41-45: F.cross_entropy on a label per node,
// F.binary_cross_entropy_with_logits on C labels per node).  Included by lt_train.hip, which owns the trainer.
//
// k_trw_head<LOSS, LPR, GRAD, LIST>: a group of LPR lanes (8, 16, 32 or 64, from Cp = C rounded up to 4) per row, 4 columns per
// lane.  The row's logits are read once; with GRAD the gradient leaves as one float4 per lane (the pad columns zero).  A block
// takes `tiles_per_block` consecutive tiles of RPB = 256 / LPR rows and leaves, for its rows,
//   part_loss[b]          the sum of the row losses: rows of a tile in row order, tiles in order (one chain in thread 0)
//   part_cnt[b, C, 3]     (tp, fp, fn) per class, counted with integer LDS atomics
//   part_db[b, C]         GRAD: the column sums of its gradient rows, rows in order (thread c owns column c)
// k_trw_finish (one block) adds the blocks' partials: the losses by a fixed tree, the counts as integers.  No float atomics:
// every sum has a fixed order.
//
// Row arithmetic, fp32, -ffp-contract=off (the per-element functions live in lt_train_common.hip.h, shared with lt_mlp.hip):
//   CE   mx = max_c z_c (first argmax: ties go to the lower column), e_c = expf(z_c - mx), s = sum e_c (a lane's four in column
//        order, then the group butterfly), loss = (mx + logf(s)) - z_y, dZ = (e_c / s - [c == y]) / n.  k_tr_ce's operations; the
//        sum's association differs from its one-thread chain, so the two heads agree to rounding, not bit for bit.  A label
//        outside [0, C): z_y = 0 and no one-hot term, as in k_tr_ce; the row counts in no cell.
//   BCE  per element l = (max(z, 0) - z y) + log1pf(expf(-|z|)); sigma = z >= 0 ? 1 / (1 + e^-z) : e^z / (1 + e^z), both through
//        t = expf(-|z|) <= 1, so nothing overflows; dZ = (sigma - y) / (n C); loss = sum l / (n C).  A label byte other than 0
//        counts as 1.  Predicted positive iff z > 0: the reference's sigmoid(z) > 0.5 evaluated in fp32 differs from it only
//        where |z| < 2^-22 (there 1 / (1 + e^-z) rounds to 0.5 although z > 0).
#pragma once

enum { TRW_CE = 0, TRW_BCE = 1 };
#define TRW_MAX_BLOCKS 256     // blocks of the head: the finish stage is one block that reads one partial per thread

struct lt_trw_args {
    int n;                     // rows of Z and of the labels
    int cnt;                   // entries scored: n, or the list's m
    const int32_t *rows;       // LIST: [cnt] row ids
    const float *Z;
    long ldz;
    int C, Cp;
    const void *labels;        // CE: int32 [n]; BCE: uint8 [n, ldy]
    long ldy;
    float inv;                 // GRAD: 1 / cnt (CE), 1 / (cnt C) (BCE)
    float *dZ;                 // GRAD: [n, Cp]
    float *part_loss;          // [blocks]
    int32_t *part_cnt;         // [blocks, C, 3]
    float *part_db;            // GRAD: [blocks, C]
    int32_t *n_bad;            // LIST: entries outside [0, n) (may be NULL)
    int tiles_per_block;
};

template <int LOSS, int LPR, bool GRAD, bool LIST>
__global__ __launch_bounds__(TR_BLOCK) void k_trw_head(lt_trw_args a) {
    constexpr int RPW = 64 / LPR, RPB = (TR_BLOCK / 64) * RPW, TW = 4 * LPR;   // rows and columns of one tile
    __shared__ int sc[3 * LT_MAX_H];
    __shared__ float sl[RPB];
    __shared__ float sd[GRAD ? RPB * TW : 1];
    __shared__ int sbad;
    const int t = threadIdx.x, lane = t & 63, gl = lane & (LPR - 1), coff = 4 * gl;
    const int rt = (t >> 6) * RPW + lane / LPR;      // the group's row inside the tile
    const int C = a.C, Cp = a.Cp;
    const bool active = coff < Cp;
    for (int i = t; i < 3 * C; i += TR_BLOCK) sc[i] = 0;
    if (LIST && t == 0) sbad = 0;
    float lsum = 0.f, dsum = 0.f;
    const int ntiles = (a.cnt + RPB - 1) / RPB;
    const int tile0 = blockIdx.x * a.tiles_per_block, tile1 = min(ntiles, tile0 + a.tiles_per_block);
    for (int tile = tile0; tile < tile1; ++tile) {
        __syncthreads();      // the counters are cleared; the last tile's sl / sd have been read
        const int i = tile * RPB + rt;
        bool scored = i < a.cnt;
        int r = i;
        if constexpr (LIST) {
            if (scored) {
                r = a.rows[i];
                scored = (unsigned)r < (unsigned)a.n;      // an id outside [0, n) is never dereferenced
                if (!scored && gl == 0) atomicAdd(&sbad, 1);
            }
        }
        float l = 0.f;
        f32x4 dz = {0.f, 0.f, 0.f, 0.f};
        if (scored) {      // uniform over the row's lane group: the shuffles below stay inside it
            f32x4 z = {0.f, 0.f, 0.f, 0.f};
            const float *zr = a.Z + (size_t)r * a.ldz + coff;
            if constexpr (GRAD) {      // the trainer's own [n, Cp] buffer
                if (active) z = ld4(zr);
            } else {                   // a caller's view: any ldz >= C, any 4-byte aligned address
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (coff + j < C) z[j] = zr[j];
            }
            if constexpr (LOSS == TRW_CE) {
                const int y = static_cast<const int32_t *>(a.labels)[r];
                float mx = -INFINITY;
                int arg = coff;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = coff + j < C ? z[j] : -INFINITY;
                    if (j == 0 || v > mx) { mx = v; arg = coff + j; }
                }
#pragma unroll
                for (int m = LPR / 2; m >= 1; m >>= 1) {
                    const float omx = __shfl_xor(mx, m, 64);
                    const int oarg = __shfl_xor(arg, m, 64);
                    lt_argmax_merge(mx, arg, omx, oarg);
                }
                float e[4], s = 0.f, zy = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    e[j] = coff + j < C ? expf(z[j] - mx) : 0.f;
                    s += e[j];
                    if (coff + j == y && coff + j < C) zy = z[j];
                }
                s = group_sum<LPR>(s);
                zy = group_sum<LPR>(zy);      // one lane holds z_y, the others 0
                l = lt_ce_row_loss(mx, s, zy);
                if constexpr (GRAD) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (coff + j < C) dz[j] = lt_ce_grad(e[j], s, coff + j == y, a.inv);
                }
                if (gl == 0 && (unsigned)y < (unsigned)C) {      // integer LDS atomics: the counts do not depend on order
                    if (arg == y) {
                        atomicAdd(&sc[3 * y], 1);
                    } else {
                        atomicAdd(&sc[3 * arg + 1], 1);
                        atomicAdd(&sc[3 * y + 2], 1);
                    }
                }
            } else {
                const uint8_t *yr = static_cast<const uint8_t *>(a.labels) + (size_t)r * a.ldy + coff;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (coff + j < C) {
                        const float zj = z[j];
                        const bool yb = yr[j] != 0;
                        float sig;
                        l += lt_bce_elem(zj, yb, sig);
                        if constexpr (GRAD) dz[j] = (sig - (yb ? 1.f : 0.f)) * a.inv;
                        const bool pred = zj > 0.f;
                        if (pred || yb) atomicAdd(&sc[3 * (coff + j) + (pred ? (yb ? 0 : 1) : 2)], 1);
                    }
                }
                l = group_sum<LPR>(l);
            }
            if constexpr (GRAD)
                if (active) *reinterpret_cast<f32x4 *>(a.dZ + (size_t)r * Cp + coff) = dz;
        }
        if (gl == 0) sl[rt] = l;
        if constexpr (GRAD) *reinterpret_cast<f32x4 *>(&sd[rt * TW + coff]) = dz;
        __syncthreads();
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < RPB; ++k) lsum += sl[k];
        }
        if constexpr (GRAD) {
            if (t < C) {
#pragma unroll
                for (int k = 0; k < RPB; ++k) dsum += sd[k * TW + t];
            }
        }
    }
    __syncthreads();
    if (t == 0) a.part_loss[blockIdx.x] = lsum;
    if constexpr (GRAD)
        if (t < C) a.part_db[(size_t)blockIdx.x * C + t] = dsum;
    for (int i = t; i < 3 * C; i += TR_BLOCK) a.part_cnt[(size_t)blockIdx.x * (3 * C) + i] = sc[i];
    if constexpr (LIST)
        if (t == 0 && a.n_bad && sbad) atomicAdd(a.n_bad, sbad);
}

// Finish stage, one block: thread t takes partial loss t (n_blk <= 256), then the fixed tree; the count cells are integers
// (thread t sums cells t, t + 256, t + 512 over the blocks).  Thread 0 writes loss = sum / divisor and the sum of the tp
// column (as a float: the second word of the trainer's record; NULL for an evaluation) and, when a state block is given,
// applies the epoch to it.
__global__ __launch_bounds__(TR_BLOCK) void k_trw_finish(int n_blk, int C, float divisor, const float *__restrict__ part_loss,
                                                         const int32_t *__restrict__ part_cnt, float *__restrict__ loss_out,
                                                         float *__restrict__ tp_out, int32_t *__restrict__ counts,
                                                         int32_t *state, int patience, int epoch) {
    __shared__ float sl[TR_BLOCK];
    __shared__ int st[TR_BLOCK];
    const int t = threadIdx.x, cells = 3 * C;
    sl[t] = t < n_blk ? part_loss[t] : 0.f;
    int tp = 0;
    for (int cell = t; cell < cells; cell += TR_BLOCK) {
        int k = 0;
#pragma unroll 4      // (16 measured slower: 29 us against 19 at 256 blocks and 363 cells, NOTES)
        for (int b = 0; b < n_blk; ++b) k += part_cnt[(size_t)b * cells + cell];
        counts[cell] = k;
        if (cell % 3 == 0) tp += k;
    }
    st[t] = tp;
    __syncthreads();
    for (int w = TR_BLOCK / 2; w >= 1; w >>= 1) {
        if (t < w) {
            sl[t] += sl[t + w];
            st[t] += st[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float mean = sl[0] / divisor;
        *loss_out = mean;
        if (tp_out) *tp_out = (float)st[0];
        if (state) val_state_update(state, mean, patience, epoch);
    }
}

// How a head launch over cnt entries is cut: lane group, rows per tile, blocks and tiles per block.  A function of (cnt, C)
// alone, so two launches over as many entries sum in the same order.
struct lt_trw_plan {
    int lpr, rpb, n_blk, tpb;
};
static lt_trw_plan trw_plan(int cnt, int C) {
    lt_trw_plan p;
    p.lpr = lt_lpr_for(lt_round_up(C, 4));
    if (p.lpr < 8) p.lpr = 8;
    p.rpb = TR_BLOCK / p.lpr;
    const int ntiles = (cnt + p.rpb - 1) / p.rpb;
    p.tpb = (ntiles + TRW_MAX_BLOCKS - 1) / TRW_MAX_BLOCKS;
    if (p.tpb < 1) p.tpb = 1;
    p.n_blk = (ntiles + p.tpb - 1) / p.tpb;
    return p;
}

// A head's partials inside one block of memory: loss [n_blk] | cnt [n_blk, C, 3] | (grad) db [n_blk, C], and their size.  The
// one place that knows the layout (base may be NULL when only the size is wanted).
struct lt_trw_parts {
    int n_blk;
    float *loss;
    int32_t *cnt;
    float *db;
    size_t bytes;
};
static lt_trw_parts trw_parts(float *base, int cnt, int C, bool grad) {
    lt_trw_parts q;
    q.n_blk = trw_plan(cnt, C).n_blk;
    q.loss = base;
    q.cnt = base ? (int32_t *)(base + q.n_blk) : nullptr;
    q.db = base && grad ? (float *)(q.cnt + (size_t)q.n_blk * 3 * C) : nullptr;
    q.bytes = (size_t)q.n_blk * (1 + 3 * (size_t)C + (grad ? (size_t)C : 0)) * sizeof(float);
    return q;
}
static size_t trw_part_bytes(int cnt, int C, bool grad) { return trw_parts(nullptr, cnt, C, grad).bytes; }

#define TRW_DISPATCH(loss, lpr, ...)                                                              \
    do {                                                                                          \
        if ((loss) == TRW_CE) { constexpr int LOSS_ = TRW_CE; TRW_DISPATCH_LPR(lpr, __VA_ARGS__); } \
        else { constexpr int LOSS_ = TRW_BCE; TRW_DISPATCH_LPR(lpr, __VA_ARGS__); }               \
    } while (0)
#define TRW_DISPATCH_LPR(lpr, ...)                                        \
    switch (lpr) {                                                        \
        case 8: { constexpr int LPR_ = 8; __VA_ARGS__; } break;           \
        case 16: { constexpr int LPR_ = 16; __VA_ARGS__; } break;         \
        case 32: { constexpr int LPR_ = 32; __VA_ARGS__; } break;         \
        default: { constexpr int LPR_ = 64; __VA_ARGS__; } break;         \
    }

// The head over all n rows (rows == NULL) or the m listed ones, then the finish stage.  dZ != NULL: the training head, with
// the gradient and its column-sum slabs; with a list it writes the listed rows of dZ only (the trainer zeroed the others
// when the list was set), inv and the divisor from m, and the list 0 .. n - 1 leaves the bits of the launch without one.
// `part` holds trw_part_bytes(cnt, C, dZ != NULL).
static int launch_trw_head(int loss_kind, const float *Z, long ldz, const void *labels, long ldy, int n, int C,
                           const int32_t *rows, int m, float *dZ, float *part, float *loss_out, float *tp_out, int32_t *counts,
                           int32_t *n_bad, int32_t *state, int patience, int epoch, hipStream_t st) {
    const int cnt = rows ? m : n;
    const lt_trw_plan p = trw_plan(cnt, C);
    lt_trw_args a;
    a.n = n; a.cnt = cnt; a.rows = rows; a.Z = Z; a.ldz = ldz; a.C = C; a.Cp = lt_round_up(C, 4);
    a.labels = labels; a.ldy = ldy;
    const double rows_d = (double)cnt, terms = loss_kind == TRW_BCE ? rows_d * C : rows_d;
    a.inv = loss_kind == TRW_BCE ? (float)(1.0 / terms) : 1.0f / (float)cnt;
    a.dZ = dZ;
    const lt_trw_parts parts = trw_parts(part, cnt, C, dZ != nullptr);
    a.part_loss = parts.loss;
    a.part_cnt = parts.cnt;
    a.part_db = parts.db;
    a.n_bad = n_bad;
    a.tiles_per_block = p.tpb;
    const dim3 grid((unsigned)p.n_blk), block(TR_BLOCK);
    if (dZ && rows) TRW_DISPATCH(loss_kind, p.lpr, hipLaunchKernelGGL((k_trw_head<LOSS_, LPR_, true, true>), grid, block, 0, st, a));
    else if (dZ) TRW_DISPATCH(loss_kind, p.lpr, hipLaunchKernelGGL((k_trw_head<LOSS_, LPR_, true, false>), grid, block, 0, st, a));
    else if (rows) TRW_DISPATCH(loss_kind, p.lpr, hipLaunchKernelGGL((k_trw_head<LOSS_, LPR_, false, true>), grid, block, 0, st, a));
    else TRW_DISPATCH(loss_kind, p.lpr, hipLaunchKernelGGL((k_trw_head<LOSS_, LPR_, false, false>), grid, block, 0, st, a));
    LT_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_trw_finish, dim3(1), dim3(TR_BLOCK), 0, st, p.n_blk, C, (float)terms, a.part_loss, a.part_cnt, loss_out,
                       tp_out, counts, state, patience, epoch);
    LT_CHECK_LAUNCH();
    return LT_OK;
}
