// Device functions the trainers share: the Philox dropout mask, the Adam element update and the per-element arithmetic of the
// CE / BCE loss heads.  Included by lt_train.hip (the GCN trainers; lt_train_wide.hip.h's head) and lt_mlp.hip (the minibatch MLP
// trainer); one definition, so both take the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lt_philox.hip.h"
#include "lt_rows.hip.h"

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

// --------------------------------------------------------------------------------------------
// Row arithmetic of the loss heads (k_trw_head in lt_train_wide.hip.h, k_mlp_rows_fwd in lt_mlp.hip), fp32, one definition:
// the heads differ in how a row's columns are spread over lanes, not in what is computed per element.
// --------------------------------------------------------------------------------------------
// running (max, first argmax) of a row merged with another lane's: ties go to the lower column
__device__ __forceinline__ void lt_argmax_merge(float &mx, int &arg, float omx, int oarg) {
    if (omx > mx || (omx == mx && oarg < arg)) { mx = omx; arg = oarg; }
}
// CE: the row's loss from its max, the sum of exp(z - max) and the label's logit; one element of its gradient
__device__ __forceinline__ float lt_ce_row_loss(float mx, float s, float zy) { return (mx + logf(s)) - zy; }
__device__ __forceinline__ float lt_ce_grad(float e, float s, bool hit, float inv) { return (e / s - (hit ? 1.f : 0.f)) * inv; }
// BCE with logits, one element: returns its loss term, leaves sigmoid(z) in sig; both through t = expf(-|z|) <= 1, so nothing
// overflows.  The gradient is (sig - y) * inv.
__device__ __forceinline__ float lt_bce_elem(float z, bool yb, float &sig) {
    const float y = yb ? 1.f : 0.f;
    const float ez = expf(-fabsf(z));
    sig = z >= 0.f ? 1.f / (1.f + ez) : ez / (1.f + ez);
    return (fmaxf(z, 0.f) - z * y) + log1pf(ez);
}
