// sg3_bn_train.hip -- training-mode BatchNorm2d of the encoder trunk: batch statistics, the element-wise apply, and the backward.
//
// Forward statistics (two launches): every workgroup takes one slice of one channel -- up to BN_SEG consecutive pixels of one
// sample -- and forms the slice's mean, then the sum of squared distances from THAT mean (a second read of a slice that is still
// in cache), both in float64.  A second launch merges the (count, mean, M2) triples of a channel in slice order (Chan's update)
// and derives   var = M2 / M (biased),  invstd = 1 / sqrt(var + eps),  a = gamma invstd,  b = beta - mean a.
// Nothing is ever formed as E[x^2] - E[x]^2, so a mean of 100 over a spread of 0.01 keeps the spread.
//
// The mean leaves as two floats, mean + meanLo: one float of a mean of 100 is off by up to 4e-6, which an invstd of 100 turns into 4e-4.
//
// Apply (one launch):  v = a[c] ((x - centre[c]) - centreLo[c]) + b[c]  (centre = NULL: v = a[c] x + b[c]);  pre = v (when asked);  y = PReLU(v; slope[c]).
// A BatchNorm in front of a convolution is never applied here: sg3_conv2d and sg3_conv2d_wgrad_sum take a and b as input affine.
//
// Backward reduce (two launches), per channel, float64 sums:   s1 = sum dy,   s2 = sum dy t,
//     t = (x - mean[c] - meanLo[c]) invstd[c]   (BatchNorm: s1 = dbeta, s2 = dgamma),    or    t = min(x, 0)   (PReLU: s2 = dslope, x = pre-activation;
//     the same pass can write masked = dy (x > 0 ? 1 : slope[c]), the gradient in front of the activation).
// Backward apply (one launch):  v = a[c] (dy - s1[c] / M - xhat s2[c] / M)  (+ addend through element strides);  raw = v (when asked);
//     dx = v (act > 0 ? 1 : slope[c])  when `act` is given (the PReLU in front of this BatchNorm whose pre-activation was saved).
//
// Every sum has a fixed order (strided per thread, a shuffle tree, four waves, slices in order): bit-identical on repeat.
#include "sg3_common.h"

namespace sg3 {

constexpr int BN_SEG = 8192;        // pixels of one sample per workgroup

__device__ __forceinline__ double bn_block_sum(double v, double* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    __syncthreads();
    return r;
}

// workgroup bid = c * P + n * segs + seg
__device__ __forceinline__ int bn_slice(int bid, int C, int HW, int segs, int P, int* c, size_t* offset) {
    *c = bid / P; const int pi = bid % P, n = pi / segs, seg = pi % segs;
    *offset = ((size_t)n * C + *c) * HW + (size_t)seg * BN_SEG;
    return min(BN_SEG, HW - seg * BN_SEG);
}

__global__ void __launch_bounds__(256)
bn_stats_partial_kernel(const float* x, double* partial, int C, int HW, int segs, int P) {
    __shared__ double sh[4];
    int c; size_t off;
    const int len = bn_slice(blockIdx.x, C, HW, segs, P, &c, &off);
    const float* base = x + off;
    double s = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) s += (double)base[i];
    const double mean = bn_block_sum(s, sh) / (double)len;
    double m2 = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) { const double d = (double)base[i] - mean; m2 += d * d; }
    m2 = bn_block_sum(m2, sh);
    if (threadIdx.x == 0) { partial[2 * (size_t)blockIdx.x] = mean; partial[2 * (size_t)blockIdx.x + 1] = m2; }
}

__global__ void __launch_bounds__(64)
bn_stats_finish_kernel(const double* partial, const float* gamma, const float* beta, float* mean, float* meanLo, float* var, float* invstd, float* a, float* b,
                       int C, int HW, int segs, int P, float eps) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double cnt = 0.0, mu = 0.0, m2 = 0.0;
    for (int pi = 0; pi < P; pi++) {
        const int seg = pi % segs;
        const double nb = (double)min(BN_SEG, HW - seg * BN_SEG);
        const double mb = partial[2 * ((size_t)c * P + pi)], qb = partial[2 * ((size_t)c * P + pi) + 1];
        const double tot = cnt + nb, delta = mb - mu;
        mu += delta * (nb / tot);
        m2 += qb + delta * delta * (cnt * nb / tot);
        cnt = tot;
    }
    const double v = m2 / cnt, is = 1.0 / sqrt(v + (double)eps);
    const double sa = (gamma ? (double)gamma[c] : 1.0) * is;
    mean[c] = (float)mu; meanLo[c] = (float)(mu - (double)(float)mu); var[c] = (float)v; invstd[c] = (float)is;
    a[c] = (float)sa; b[c] = (float)((beta ? (double)beta[c] : 0.0) - mu * sa);
}

__global__ void __launch_bounds__(256)
bn_apply_kernel(const float* x, const float* scale, const float* shift, const float* centre, const float* centreLo, const float* slope, float* y, float* pre,
                int C, int HW, int chunks) {
    const int plane = blockIdx.x / chunks, chunk = blockIdx.x % chunks, c = plane % C;
    const float a = scale[c], b = shift[c], m = centre ? centre[c] : 0.f, ml = centreLo ? centreLo[c] : 0.f, sl = slope ? slope[c] : 1.f;
    const size_t base = (size_t)plane * HW;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int i = chunk * 1024 + q * 256 + threadIdx.x;
        if (i < HW) {
            float v = fmaf((x[base + i] - m) - ml, a, b);
            if (pre) pre[base + i] = v;
            if (slope) v = v > 0.f ? v : v * sl;
            y[base + i] = v;
        }
    }
}

__global__ void __launch_bounds__(256)
bn_bwd_partial_kernel(const float* dy, const float* x, const float* mean, const float* meanLo, const float* invstd, const float* slope, float* masked, double* partial,
                      int C, int HW, int segs, int P, int mode) {
    __shared__ double sh[4];
    int c; size_t off;
    const int len = bn_slice(blockIdx.x, C, HW, segs, P, &c, &off);
    const double mu = mode == 0 ? (double)mean[c] + (meanLo ? (double)meanLo[c] : 0.0) : 0.0, is = mode == 0 ? (double)invstd[c] : 1.0;
    const float sl = masked ? slope[c] : 1.f;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < len; i += 256) {
        const double g = (double)dy[off + i], xv = (double)x[off + i];
        const double t = mode == 0 ? (xv - mu) * is : fmin(xv, 0.0);
        s1 += g; s2 += g * t;
        if (masked) masked[off + i] = x[off + i] > 0.f ? dy[off + i] : dy[off + i] * sl;
    }
    s1 = bn_block_sum(s1, sh); s2 = bn_block_sum(s2, sh);
    if (threadIdx.x == 0) { partial[2 * (size_t)blockIdx.x] = s1; partial[2 * (size_t)blockIdx.x + 1] = s2; }
}

__global__ void __launch_bounds__(64)
bn_bwd_finish_kernel(const double* partial, float* sum1, float* sum2, int C, int P) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int pi = 0; pi < P; pi++) { s1 += partial[2 * ((size_t)c * P + pi)]; s2 += partial[2 * ((size_t)c * P + pi) + 1]; }
    if (sum1) sum1[c] = (float)s1;
    sum2[c] = (float)s2;
}

struct BnBwdApply {
    const float* dy; const float* x; const float* mean; const float* meanLo; const float* invstd; const float* scale; const float* sum1; const float* sum2;
    const float* addend; const float* act; const float* slope; float* dx; float* raw;
    int64_t addStride[4];
    int C, H, W, chunks; float invM;
};

__global__ void __launch_bounds__(256)
bn_bwd_apply_kernel(BnBwdApply p) {
    const int HW = p.H * p.W;
    const int plane = blockIdx.x / p.chunks, chunk = blockIdx.x % p.chunks, c = plane % p.C, n = plane / p.C;
    const float mu = p.mean[c], ml = p.meanLo ? p.meanLo[c] : 0.f, is = p.invstd[c], a = p.scale[c], k1 = p.sum1[c] * p.invM, k2 = p.sum2[c] * p.invM;
    const float sl = p.act ? p.slope[c] : 1.f;
    const size_t base = (size_t)plane * HW;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int i = chunk * 1024 + q * 256 + threadIdx.x;
        if (i < HW) {
            const float xh = ((p.x[base + i] - mu) - ml) * is;
            float v = a * ((p.dy[base + i] - k1) - xh * k2);
            if (p.addend) {
                const int yy = i / p.W, xx = i % p.W;
                v += p.addend[(int64_t)n * p.addStride[0] + (int64_t)c * p.addStride[1] + (int64_t)yy * p.addStride[2] + (int64_t)xx * p.addStride[3]];
            }
            if (p.raw) p.raw[base + i] = v;
            if (p.act) v = p.act[base + i] > 0.f ? v : v * sl;
            p.dx[base + i] = v;
        }
    }
}

static bool bn_geometry(int N, int C, int H, int W, int* HW, int* segs, int* P, long long* blocks) {
    const long long hw = (long long)H * W, total = hw * N * C;
    if (N <= 0 || C <= 0 || hw <= 0 || total >= 0x7fffffffLL) return false;
    *HW = (int)hw; *segs = ceil_div(*HW, BN_SEG); *P = N * *segs; *blocks = (long long)*P * C;
    return *blocks <= 0x7fffffffLL;
}

} // namespace sg3

extern "C" {

int sg3_bn_train_partials(int N, int H, int W) {
    using namespace sg3;
    int HW, segs, P; long long blocks;
    if (!bn_geometry(N, 1, H, W, &HW, &segs, &P, &blocks)) return 0;
    return P;
}

int sg3_bn_train_stats(const sg3_bn_train_stats_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->partial && p->mean && p->meanLo && p->var && p->invstd && p->a && p->b, "bn_train_stats: null tensor");
    int HW, segs, P; long long blocks;
    SG3_REQUIRE(bn_geometry(p->N, p->C, p->H, p->W, &HW, &segs, &P, &blocks), "bn_train_stats: empty or too large tensor");
    SG3_REQUIRE((long long)p->N * HW > 1, "bn_train_stats: training-mode BatchNorm needs more than one value per channel");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_stats_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->x, p->partial, p->C, HW, segs, P);
    SG3_LAUNCH_CHECK("bn_stats_partial_kernel");
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((unsigned)ceil_div(p->C, 64)), dim3(64), 0, st, p->partial, p->gamma, p->beta, p->mean, p->meanLo, p->var,
                       p->invstd, p->a, p->b, p->C, HW, segs, P, p->eps);
    SG3_LAUNCH_CHECK("bn_stats_finish_kernel");
    return SG3_OK;
}

int sg3_bn_train_apply(const sg3_bn_train_apply_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->scale && p->shift && p->y, "bn_train_apply: null tensor");
    int HW, segs, P; long long blocks;
    SG3_REQUIRE(bn_geometry(p->N, p->C, p->H, p->W, &HW, &segs, &P, &blocks), "bn_train_apply: empty or too large tensor");
    const int chunks = ceil_div(HW, 1024);
    const long long grid = (long long)p->N * p->C * chunks;
    SG3_REQUIRE(grid <= 0x7fffffffLL, "bn_train_apply: grid too large");
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p->x, p->scale, p->shift, p->centre, p->centreLo, p->slope, p->y, p->pre,
                       p->C, HW, chunks);
    SG3_LAUNCH_CHECK("bn_apply_kernel");
    return SG3_OK;
}

int sg3_bn_train_bwd_reduce(const sg3_bn_train_bwd_reduce_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->dy && p->x && p->partial && p->sum2, "bn_train_bwd_reduce: null tensor");
    SG3_REQUIRE(p->mode == 0 || p->mode == 1, "bn_train_bwd_reduce: mode 0 (BatchNorm) or 1 (PReLU slope)");
    SG3_REQUIRE(p->mode == 1 || (p->mean && p->invstd), "bn_train_bwd_reduce: mean and invstd missing");
    SG3_REQUIRE(!p->masked || (p->mode == 1 && p->slope), "bn_train_bwd_reduce: the masked output belongs to mode 1 and needs the slopes");
    int HW, segs, P; long long blocks;
    SG3_REQUIRE(bn_geometry(p->N, p->C, p->H, p->W, &HW, &segs, &P, &blocks), "bn_train_bwd_reduce: empty or too large tensor");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_bwd_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, p->dy, p->x, p->mean, p->meanLo, p->invstd, p->slope, p->masked, p->partial, p->C, HW, segs, P, p->mode);
    SG3_LAUNCH_CHECK("bn_bwd_partial_kernel");
    hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((unsigned)ceil_div(p->C, 64)), dim3(64), 0, st, p->partial, p->sum1, p->sum2, p->C, P);
    SG3_LAUNCH_CHECK("bn_bwd_finish_kernel");
    return SG3_OK;
}

int sg3_bn_train_bwd_apply(const sg3_bn_train_bwd_apply_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->dy && p->x && p->mean && p->invstd && p->scale && p->sum1 && p->sum2 && p->dx, "bn_train_bwd_apply: null tensor");
    SG3_REQUIRE(!p->act || p->slope, "bn_train_bwd_apply: slope missing");
    int HW, segs, P; long long blocks;
    SG3_REQUIRE(bn_geometry(p->N, p->C, p->H, p->W, &HW, &segs, &P, &blocks), "bn_train_bwd_apply: empty or too large tensor");
    BnBwdApply q;
    q.dy = p->dy; q.x = p->x; q.mean = p->mean; q.meanLo = p->meanLo; q.invstd = p->invstd; q.scale = p->scale; q.sum1 = p->sum1; q.sum2 = p->sum2;
    q.addend = p->addend; q.act = p->act; q.slope = p->slope; q.dx = p->dx; q.raw = p->raw;
    for (int d = 0; d < 4; d++) q.addStride[d] = p->addStride[d];
    q.C = p->C; q.H = p->H; q.W = p->W; q.chunks = ceil_div(HW, 1024);
    q.invM = (float)(1.0 / ((double)p->N * HW));
    const long long grid = (long long)p->N * p->C * q.chunks;
    SG3_REQUIRE(grid <= 0x7fffffffLL, "bn_train_bwd_apply: grid too large");
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, q);
    SG3_LAUNCH_CHECK("bn_bwd_apply_kernel");
    return SG3_OK;
}

} // extern "C"
