// sg3_ranger.hip -- one Ranger step (RAdam + lookahead + gradient centralisation; reference utils/ranger.py:79-165) of up to 32
// float32 tensors in one launch.
//
// A workgroup is one row of one tensor (a 1-D tensor is a single row).  Per row, in the order of the reference's tensor ops:
//   centralisation (2-D tensors when enabled)   mean = (sum of the row) / cols; each thread sums its columns tid, tid + 256, ...
//                                               in ascending order, the 256 partials are halved in LDS (128, 64, ... 1): a fixed
//                                               order; g = grad - mean is written back to grad, as the reference's in-place add_.
//   moments                                     v = v * beta2 + (1 - beta2) * g * g;   m = m * beta1 + (1 - beta1) * g
//   weight decay (when non-zero)                p = p - (weight_decay * lr) * p
//   step                                        adaptive: p = p - (step_size * lr) * m / (sqrt(v) + eps);  plain: p = p - (step_size * lr) * m
//   lookahead (every k-th step)                 slow = slow + alpha * (p - slow);  p = slow
// step_size, the branch and the lookahead flag are host scalars computed from the step count: nothing is read back from the device.
// Built without contraction so that each line above rounds as the corresponding torch op does.
#include "sg3_common.h"

namespace sg3 {

static constexpr int kRangerMax = 32;

struct RangerLaunch {
    sg3_ranger_tensor t[kRangerMax];
    int rowStart[kRangerMax + 1];      // first workgroup of tensor i; rowStart[count] = grid size
    int count;
    float beta1, beta2, oneMinusBeta1, oneMinusBeta2, eps, decay, stepLr, alpha;
    int adaptive, lookahead;
};

__global__ void __launch_bounds__(256)
ranger_kernel(RangerLaunch a) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    int i = 0;
    while (i + 1 < a.count && (int)blockIdx.x >= a.rowStart[i + 1]) i++;
    const sg3_ranger_tensor T = a.t[i];
    const size_t base = (size_t)((int)blockIdx.x - a.rowStart[i]) * (size_t)T.cols;

    float mean = 0.f;
    if (T.centralise) {
        float s = 0.f;
        for (int c = tid; c < T.cols; c += 256) s = __fadd_rn(s, T.grad[base + c]);
        red[tid] = s;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) red[tid] = __fadd_rn(red[tid], red[tid + o]);
            __syncthreads();
        }
        mean = __fdiv_rn(red[0], (float)T.cols);
    }
    for (int c = tid; c < T.cols; c += 256) {
        const size_t j = base + c;
        float g = T.grad[j];
        if (T.centralise) { g = __fsub_rn(g, mean); T.grad[j] = g; }
        const float v = __fadd_rn(__fmul_rn(T.expAvgSq[j], a.beta2), __fmul_rn(__fmul_rn(a.oneMinusBeta2, g), g));
        const float m = __fadd_rn(__fmul_rn(T.expAvg[j], a.beta1), __fmul_rn(a.oneMinusBeta1, g));
        T.expAvgSq[j] = v;
        T.expAvg[j] = m;
        float p = T.p[j];
        if (a.decay != 0.f) p = __fsub_rn(p, __fmul_rn(a.decay, p));
        if (a.adaptive) p = __fsub_rn(p, __fmul_rn(a.stepLr, __fdiv_rn(m, __fadd_rn(__fsqrt_rn(v), a.eps))));
        else p = __fsub_rn(p, __fmul_rn(a.stepLr, m));
        if (a.lookahead) {
            const float s = T.slow[j];
            p = __fadd_rn(s, __fmul_rn(a.alpha, __fsub_rn(p, s)));
            T.slow[j] = p;
        }
        T.p[j] = p;
    }
}

static bool ranger_overlaps(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

} // namespace sg3

extern "C" {

int sg3_ranger_step(const sg3_ranger_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p, "ranger_step: null params");
    SG3_REQUIRE(p->count >= 1 && p->count <= kRangerMax, "ranger_step: %d tensors (1..32 per call)", p->count);
    SG3_REQUIRE(p->beta1 >= 0.f && p->beta1 < 1.f && p->beta2 >= 0.f && p->beta2 < 1.f && p->eps > 0.f, "ranger_step: bad betas or eps");
    RangerLaunch a = {};
    a.count = p->count;
    int64_t rows = 0;
    for (int i = 0; i < p->count; i++) {
        const sg3_ranger_tensor& t = p->t[i];
        SG3_REQUIRE(t.p && t.grad && t.expAvg && t.expAvgSq && t.slow, "ranger_step: tensor %d has a null pointer", i);
        SG3_REQUIRE(t.rows > 0 && t.cols > 0, "ranger_step: tensor %d is %d x %d", i, t.rows, t.cols);
        SG3_REQUIRE((((uintptr_t)t.p | (uintptr_t)t.grad | (uintptr_t)t.expAvg | (uintptr_t)t.expAvgSq | (uintptr_t)t.slow) & 3) == 0,
                    "ranger_step: tensor %d is not 4-byte aligned", i);
        a.t[i] = t;
        a.rowStart[i] = (int)rows;
        rows += t.rows;
        SG3_REQUIRE(rows < (1ll << 30), "ranger_step: too many rows");
    }
    a.rowStart[p->count] = (int)rows;
    // every buffer is written: none may overlap another, of this tensor or of any other in the call
    for (int i = 0; i < 5 * p->count; i++)
        for (int j = 0; j < i; j++) {
            const sg3_ranger_tensor& u = p->t[i / 5];
            const sg3_ranger_tensor& v = p->t[j / 5];
            const float* const pu[5] = {u.p, u.grad, u.expAvg, u.expAvgSq, u.slow};
            const float* const pv[5] = {v.p, v.grad, v.expAvg, v.expAvgSq, v.slow};
            SG3_REQUIRE(!ranger_overlaps(pu[i % 5], (size_t)u.rows * u.cols * 4, pv[j % 5], (size_t)v.rows * v.cols * 4),
                        "ranger_step: buffer %d of tensor %d overlaps buffer %d of tensor %d", i % 5, i / 5, j % 5, j / 5);
        }
    a.beta1 = p->beta1; a.beta2 = p->beta2; a.oneMinusBeta1 = p->oneMinusBeta1; a.oneMinusBeta2 = p->oneMinusBeta2;
    a.eps = p->eps; a.decay = p->decay; a.stepLr = p->stepLr; a.alpha = p->alpha;
    a.adaptive = p->adaptive; a.lookahead = p->lookahead;
    hipLaunchKernelGGL(ranger_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a);
    SG3_LAUNCH_CHECK("ranger_kernel");
    return SG3_OK;
}

} // extern "C"
