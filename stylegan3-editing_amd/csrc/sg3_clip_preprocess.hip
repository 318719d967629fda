// sg3_clip_preprocess.hip -- rendered float images -> the normalised 224 x 224 tensors CLIP's image encoder takes, in one launch.
//
// Reference: editing/styleclip_global_directions/preprocess/create_delta_i_c.py:53-56 `generate_images`:
//     F.interpolate(x, size=(224, 224), mode='bicubic', align_corners=True);  (y + 1) / 2;  clamp(0, 1);  Normalize(mean, std)
// five torch ops and four [B,3,224,224] intermediates per call there; one kernel and none here.
//   * Source coordinates are torch's, in float32: scale = float(in - 1) / float(out - 1), src = scale * dst, floorf, t = src - floor.
//     Double-precision coordinates differ from torch by up to 7e-4 in the result at 1024 -> 224, so they are not used.
//   * Taps: cubic convolution, A = -0.75, at floor - 1 .. floor + 2, indices clamped to the border; x first, then y, as torch's
//     device kernel orders them.
//   * This file is compiled with -ffp-contract=off (csrc/Makefile), so the compiler fuses nothing by itself and the rounding of
//     every operation is the one written here.  The tap polynomials and the four-product sums are written with fmaf: torch's
//     device kernel is built with contraction on and rounds those sums once per term, and with every product rounded on its own
//     this kernel missed the fp64 restatement by 1.3 - 2.6 x what torch's composite misses it by (measured),
//     beyond the factor of two its test allows at 1024 -> 224.  The coordinates, the clamp and the normalisation are not fused.
//   * The clamp is written with comparisons, which pass NaN through as torch.clamp does (fminf / fmaxf would drop it).
//   * Neither size changing is a copy in torch's device kernel (a NaN pixel stays one NaN pixel); so it is here.
//
// Work split: one thread per output pixel, all three channels (the coordinates and the eight tap weights are shared by them).
// Consecutive threads take consecutive ox, so stores are contiguous along a row; the 16-tap gathers of neighbouring outputs
// overlap and are served from cache (at 1024 -> 224 the stride between outputs is 4.6 input pixels).
#include "sg3_common.h"

namespace sg3 {

static constexpr int kThreads = 256;

struct Taps { int i[4]; float c[4]; };

// ((A + 2) x - (A + 3)) x x + 1 and ((A x - 5 A) x + 8 A) x - 4 A; exactly 1 and 0 at x = 0, 1, 2
__device__ __forceinline__ float cubic1(float x, float A) { return fmaf(fmaf(A + 2.0f, x, -(A + 3.0f)) * x, x, 1.0f); }
__device__ __forceinline__ float cubic2(float x, float A) { return fmaf(fmaf(fmaf(A, x, -5.0f * A), x, 8.0f * A), x, -4.0f * A); }

__device__ __forceinline__ Taps taps_for(int dst, float scale, int size) {
    const float A = -0.75f;
    const float src = scale * (float)dst;
    const float fl = floorf(src);
    const float t = src - fl;
    const int i0 = (int)fl;
    Taps r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.i[k] = min(max(i0 - 1 + k, 0), size - 1);
    const float u = 1.0f - t;
    r.c[0] = cubic2(t + 1.0f, A);
    r.c[1] = cubic1(t, A);
    r.c[2] = cubic1(u, A);
    r.c[3] = cubic2(u + 1.0f, A);
    return r;
}

__device__ __forceinline__ float interp4(float a, float b, float c, float d, const float* k) {
    return fmaf(d, k[3], fmaf(c, k[2], fmaf(b, k[1], a * k[0])));
}

__device__ __forceinline__ float finish(float v, float mean, float std) {
    float t = (v + 1.0f) * 0.5f;                              // x / 2 and x * 0.5f round identically
    t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);              // NaN fails both comparisons and stays
    return __fdiv_rn(t - mean, std);
}

__global__ void __launch_bounds__(kThreads)
clip_preprocess_kernel(sg3_clip_preprocess_params p, float scaleY, float scaleX) {
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t perImage = (int64_t)p.h * p.w;
    if (g >= perImage * p.B) return;
    const int b = (int)(g / perImage);
    const int r = (int)(g - b * perImage);
    const int oy = r / p.w, ox = r - oy * p.w;
    const float* xb = p.x + (int64_t)b * p.xStride[0];
    float* yb = p.y + (int64_t)b * p.yStride[0] + (int64_t)oy * p.yStride[2] + (int64_t)ox * p.yStride[3];
    if (p.H == p.h && p.W == p.w) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            yb[c * p.yStride[1]] = finish(xb[c * p.xStride[1] + (int64_t)oy * p.xStride[2] + (int64_t)ox * p.xStride[3]], p.mean[c], p.std[c]);
        return;
    }
    const Taps ty = taps_for(oy, scaleY, p.H);
    const Taps tx = taps_for(ox, scaleX, p.W);
    int64_t offX[4];
#pragma unroll
    for (int k = 0; k < 4; k++) offX[k] = (int64_t)tx.i[k] * p.xStride[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float* xc = xb + c * p.xStride[1];
        float rows[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float* xr = xc + (int64_t)ty.i[j] * p.xStride[2];
            rows[j] = interp4(xr[offX[0]], xr[offX[1]], xr[offX[2]], xr[offX[3]], tx.c);
        }
        yb[c * p.yStride[1]] = finish(interp4(rows[0], rows[1], rows[2], rows[3], ty.c), p.mean[c], p.std[c]);
    }
}

} // namespace sg3

extern "C" {

int sg3_clip_preprocess(const sg3_clip_preprocess_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->y, "clip_preprocess: null tensor");
    SG3_REQUIRE(p->C == 3, "clip_preprocess: x must have 3 channels, got %d", p->C);
    SG3_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0 && p->h > 0 && p->w > 0, "clip_preprocess: sizes must be positive (B %d, %d x %d -> %d x %d)",
                p->B, p->H, p->W, p->h, p->w);
    for (int c = 0; c < 3; c++)
        SG3_REQUIRE(p->std[c] != 0.0f && p->std[c] == p->std[c] && p->mean[c] == p->mean[c], "clip_preprocess: std[%d] must be non-zero, mean and std not NaN", c);
    SG3_REQUIRE(p->H <= (1 << 24) && p->W <= (1 << 24) && p->h <= (1 << 24) && p->w <= (1 << 24),
                "clip_preprocess: sizes beyond 2^24 are not exact in the float32 coordinates");
    const int64_t threads = (int64_t)p->B * p->h * p->w;
    const int64_t blocks = ceil_div64(threads, kThreads);
    SG3_REQUIRE(blocks < (1ll << 31), "clip_preprocess: batch too large for one launch");
    // torch's area_pixel_compute_scale with align_corners=True, in float32
    const float scaleY = p->h > 1 ? (float)(p->H - 1) / (float)(p->h - 1) : 0.0f;
    const float scaleX = p->w > 1 ? (float)(p->W - 1) / (float)(p->w - 1) : 0.0f;
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, *p, scaleY, scaleX);
    SG3_LAUNCH_CHECK("clip_preprocess_kernel");
    return SG3_OK;
}

} // extern "C"
