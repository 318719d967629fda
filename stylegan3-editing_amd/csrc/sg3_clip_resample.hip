// sg3_clip_resample.hip -- the image preparation of the CLIP loss, forward and adjoint, one launch each and no intermediate.
//
// Reference: criteria/clip_loss.py `self.avg_pool(self.upsample(image))` with Upsample(scale_factor=7) (nearest) and
// AvgPool2d(stylegan_size // 32): at 1024 x 1024 torch writes a 7168 x 7168 plane per channel and reads it back.
//   y[oy][ox] = (1 / k^2) sum_{u in [oy k, oy k + k)} sum_{v in [ox k, ox k + k)} x[u / up][v / up]
// Along one axis the k upsampled pixels of a window come from the source pixels (oy k) / up .. (oy k + k - 1) / up, at most
// ceil(k / up) + 1 of them, and source pixel s contributes  c = |[s up, s up + up) n [oy k, oy k + k)|  of them: an integer.  So
// the box is separable with integer counts, y = (sum_s cy_s sum_t cx_t x[s][t]) / k^2.  AvgPool2d floors the output size; the
// upsampled rows and columns past oh k, ow k are in no window.
//
// The adjoint runs in gather form: source pixel s lies in the windows (s up) / k .. min((s up + up - 1) / k, oh - 1) -- two at
// most when k >= up -- with the same counts, so every thread sums what its own pixel receives: no atomics, one fixed order.
//
// Work split: one thread per written pixel and plane, consecutive threads along a row.
#include "sg3_common.h"

namespace sg3 {

static constexpr int kThreads = 256;

__device__ __forceinline__ int overlap(int a0, int a1, int b0, int b1) { return min(a1, b1) - max(a0, b0); }

__global__ void __launch_bounds__(kThreads)
clip_resample_kernel(sg3_clip_resample_params p) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t perPlane = (int64_t)p.oh * p.ow;
    if (g >= perPlane * p.B * p.C) return;
    const int plane = (int)(g / perPlane), r = (int)(g - plane * perPlane);
    const int b = plane / p.C, c = plane - b * p.C;
    const int oy = r / p.ow, ox = r - oy * p.ow;
    const float* x = p.x + (int64_t)b * p.xStride[0] + (int64_t)c * p.xStride[1];
    const int u0 = oy * p.k, v0 = ox * p.k;
    const int s0 = u0 / p.up, s1 = (u0 + p.k - 1) / p.up, t0 = v0 / p.up, t1 = (v0 + p.k - 1) / p.up;      // s1 <= H - 1, t1 <= W - 1: oh k <= up H
    float acc = 0.0f;
    for (int s = s0; s <= s1; s++) {
        const float* xr = x + (int64_t)s * p.xStride[2];
        float row = 0.0f;
        for (int t = t0; t <= t1; t++) row += (float)overlap(t * p.up, t * p.up + p.up, v0, v0 + p.k) * xr[(int64_t)t * p.xStride[3]];
        acc += (float)overlap(s * p.up, s * p.up + p.up, u0, u0 + p.k) * row;
    }
    p.y[(int64_t)b * p.yStride[0] + (int64_t)c * p.yStride[1] + (int64_t)oy * p.yStride[2] + (int64_t)ox * p.yStride[3]] = acc / (float)(p.k * p.k);
}

__global__ void __launch_bounds__(kThreads)
clip_resample_adjoint_kernel(sg3_clip_resample_params p) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t perPlane = (int64_t)p.H * p.W;
    if (g >= perPlane * p.B * p.C) return;
    const int plane = (int)(g / perPlane), r = (int)(g - plane * perPlane);
    const int b = plane / p.C, c = plane - b * p.C;
    const int s = r / p.W, t = r - s * p.W;
    const float* y = p.y + (int64_t)b * p.yStride[0] + (int64_t)c * p.yStride[1];
    const int u0 = s * p.up, v0 = t * p.up;
    const int oy0 = u0 / p.k, oy1 = min((u0 + p.up - 1) / p.k, p.oh - 1), ox0 = v0 / p.k, ox1 = min((v0 + p.up - 1) / p.k, p.ow - 1);
    float acc = 0.0f;
    for (int oy = oy0; oy <= oy1; oy++) {
        const float* yr = y + (int64_t)oy * p.yStride[2];
        float row = 0.0f;
        for (int ox = ox0; ox <= ox1; ox++) row += (float)overlap(v0, v0 + p.up, ox * p.k, ox * p.k + p.k) * yr[(int64_t)ox * p.yStride[3]];
        acc += (float)overlap(u0, u0 + p.up, oy * p.k, oy * p.k + p.k) * row;
    }
    p.x[(int64_t)b * p.xStride[0] + (int64_t)c * p.xStride[1] + (int64_t)s * p.xStride[2] + (int64_t)t * p.xStride[3]] = acc / (float)(p.k * p.k);
}

} // namespace sg3

extern "C" {

int sg3_clip_resample(const sg3_clip_resample_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->y, "clip_resample: null tensor");
    SG3_REQUIRE(p->B > 0 && p->C > 0 && p->H > 0 && p->W > 0, "clip_resample: sizes must be positive (B %d, C %d, %d x %d)", p->B, p->C, p->H, p->W);
    SG3_REQUIRE(p->up >= 1 && p->k >= 1 && p->up <= 1024 && p->k <= 1024, "clip_resample: up %d and k %d must be in 1 .. 1024", p->up, p->k);
    SG3_REQUIRE((int64_t)p->H * p->up < (1ll << 30) && (int64_t)p->W * p->up < (1ll << 30), "clip_resample: upsampled size too large");
    SG3_REQUIRE(p->oh == (int)((int64_t)p->H * p->up / p->k) && p->ow == (int)((int64_t)p->W * p->up / p->k) && p->oh > 0 && p->ow > 0,
                "clip_resample: output %d x %d is not floor(up * size / k) or is empty", p->oh, p->ow);
    const int64_t threads = (int64_t)p->B * p->C * (p->adjoint ? (int64_t)p->H * p->W : (int64_t)p->oh * p->ow);
    SG3_REQUIRE(threads / ((int64_t)p->B * p->C) < (1ll << 31) && (int64_t)p->B * p->C < (1ll << 31), "clip_resample: plane too large");
    const int64_t blocks = ceil_div64(threads, kThreads);
    SG3_REQUIRE(blocks < (1ll << 31), "clip_resample: batch too large for one launch");
    if (p->adjoint) hipLaunchKernelGGL(clip_resample_adjoint_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(clip_resample_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_resample_kernel");
    return SG3_OK;
}

} // extern "C"
