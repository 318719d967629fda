// sg3_face_pool.hip -- the image preparation of the identity loss, forward and adjoint, one launch each and no intermediate.
//
// Reference: criteria/id_loss.py extract_feats
//     if x.shape[2] != 256: x = AdaptiveAvgPool2d((256, 256))(x)
//     x = x[:, :, 35:223, 32:220]
//     x = AdaptiveAvgPool2d((112, 112))(x)
// Adaptive average pooling of n_in -> n_out samples averages, for output i, the window [floor(i n_in / n_out), ceil((i + 1) n_in / n_out)).
// Pool, crop and pool are together one separable linear map  out = Ay X Ax^T  per plane,
//     Ay[o][s] = (1 / |w112(o)|) sum_{j in w112(o)} [s in wsrc(off + j)] / |wsrc(off + j)|,
// w112 the windows of 188 -> 112, wsrc those of H -> 256 (or the single sample off + j when the reference skips the first pool:
// shape[2] == 256), off = 35 for rows and 32 for columns.  Nothing is tabulated: both kernels walk the windows, which keeps every
// index provably inside the tensors (forward: off + j <= 222, so the last source window ends at ceil(223 H / 256) <= H).
//
// The adjoint runs in gather form: every source pixel sums Ay[o][s] Ax[q][t] dy[o][q] over the few outputs whose windows contain it,
// in one fixed order (no atomics: bit-equal on repeat), and pixels outside the crop's footprint receive an exact zero.
//
// Work split: one thread per written pixel and plane, consecutive threads along a row.
#include "sg3_common.h"

namespace sg3 {

static constexpr int kFpThreads = 256;
static constexpr int kMid = 256, kCrop = 188, kOut = 112;

struct FpAxis { int in, pool, off; };

// source window of pooled sample r (0 <= r < 256)
__device__ __forceinline__ void fp_src_win(const FpAxis& a, int r, int& b, int& e) {
    if (!a.pool) { b = r; e = r + 1; return; }
    b = (int)(((int64_t)r * a.in) / kMid);
    e = (int)(((int64_t)(r + 1) * a.in + kMid - 1) / kMid);
}
// window of output o (0 <= o < 112) over the 188 cropped samples
__device__ __forceinline__ void fp_mid_win(int o, int& b, int& e) { b = (o * kCrop) / kOut; e = ((o + 1) * kCrop + kOut - 1) / kOut; }

// A[o][s] of one axis
__device__ __forceinline__ float fp_weight(const FpAxis& a, int o, int s) {
    int j0, j1;
    fp_mid_win(o, j0, j1);
    float w = 0.f;
    for (int j = j0; j < j1; j++) {
        int b, e;
        fp_src_win(a, a.off + j, b, e);
        if (s >= b && s < e) w += 1.f / (float)((e - b) * (j1 - j0));
    }
    return w;
}

// outputs [o0, o1] that can hold source sample s (a superset: fp_weight decides), empty when s is outside the crop's footprint
__device__ __forceinline__ void fp_out_range(const FpAxis& a, int s, int& o0, int& o1) {
    int r0, r1;
    if (!a.pool) { r0 = r1 = s; }
    else {
        r0 = max(0, (int)(((int64_t)s * kMid) / a.in) - 1);
        r1 = min(kMid - 1, (int)((((int64_t)s + 1) * kMid + a.in - 1) / a.in));
    }
    const int j0 = max(0, r0 - a.off), j1 = min(kCrop - 1, r1 - a.off);
    if (j1 < j0) { o0 = 0; o1 = -1; return; }
    o0 = max(0, (j0 * kOut) / kCrop - 1);
    o1 = min(kOut - 1, (j1 * kOut) / kCrop + 1);
}

__global__ void __launch_bounds__(kFpThreads)
face_pool_kernel(sg3_face_pool_params p) {
    const int64_t g = (int64_t)blockIdx.x * kFpThreads + threadIdx.x;
    const int perPlane = kOut * kOut;
    if (g >= (int64_t)perPlane * p.B * p.C) return;
    const int plane = (int)(g / perPlane), r = (int)(g - (int64_t)plane * perPlane);
    const int b = plane / p.C, c = plane - b * p.C;
    const int oy = r / kOut, ox = r - oy * kOut;
    const FpAxis ay = {p.H, p.pool, 35}, ax = {p.W, p.pool, 32};
    const float* x = p.x + (int64_t)b * p.xStride[0] + (int64_t)c * p.xStride[1];
    int jy0, jy1, jx0, jx1;
    fp_mid_win(oy, jy0, jy1);
    fp_mid_win(ox, jx0, jx1);
    float acc = 0.f;
    for (int jy = jy0; jy < jy1; jy++) {
        int sy0, sy1;
        fp_src_win(ay, ay.off + jy, sy0, sy1);
        float mid = 0.f;
        for (int sy = sy0; sy < sy1; sy++) {
            const float* xr = x + (int64_t)sy * p.xStride[2];
            float row = 0.f;
            for (int jx = jx0; jx < jx1; jx++) {
                int sx0, sx1;
                fp_src_win(ax, ax.off + jx, sx0, sx1);
                float s = 0.f;
                for (int sx = sx0; sx < sx1; sx++) s += xr[(int64_t)sx * p.xStride[3]];
                row += s / (float)(sx1 - sx0);
            }
            mid += row;
        }
        acc += mid / (float)(sy1 - sy0);
    }
    acc /= (float)((jy1 - jy0) * (jx1 - jx0));
    p.y[(int64_t)b * p.yStride[0] + (int64_t)c * p.yStride[1] + (int64_t)oy * p.yStride[2] + (int64_t)ox * p.yStride[3]] = acc;
}

__global__ void __launch_bounds__(kFpThreads)
face_pool_adjoint_kernel(sg3_face_pool_params p) {
    const int64_t g = (int64_t)blockIdx.x * kFpThreads + threadIdx.x;
    const int64_t perPlane = (int64_t)p.H * p.W;
    if (g >= perPlane * p.B * p.C) return;
    const int plane = (int)(g / perPlane), r = (int)(g - plane * perPlane);
    const int b = plane / p.C, c = plane - b * p.C;
    const int s = r / p.W, t = r - s * p.W;
    const FpAxis ay = {p.H, p.pool, 35}, ax = {p.W, p.pool, 32};
    const float* y = p.y + (int64_t)b * p.yStride[0] + (int64_t)c * p.yStride[1];
    int oy0, oy1, ox0, ox1;
    fp_out_range(ay, s, oy0, oy1);
    fp_out_range(ax, t, ox0, ox1);
    float acc = 0.f;
    // the column weights do not depend on the output row: taken once when the candidate range fits FP_HOIST registers (every
    // image of 64 columns or more), else inside the row loop; the sums are the same either way, term by term
    constexpr int FP_HOIST = 8;
    const bool hoist = ox1 - ox0 < FP_HOIST;
    float wxs[FP_HOIST];
#pragma unroll
    for (int k = 0; k < FP_HOIST; k++) wxs[k] = (hoist && ox0 + k <= ox1) ? fp_weight(ax, ox0 + k, t) : 0.f;
    if (ox1 >= ox0) {
        for (int oy = oy0; oy <= oy1; oy++) {
            const float wy = fp_weight(ay, oy, s);
            if (wy == 0.f) continue;
            const float* yr = y + (int64_t)oy * p.yStride[2];
            float row = 0.f;
            if (hoist) {
#pragma unroll
                for (int k = 0; k < FP_HOIST; k++)
                    if (wxs[k] != 0.f) row += wxs[k] * yr[(int64_t)(ox0 + k) * p.yStride[3]];
            } else {
                for (int ox = ox0; ox <= ox1; ox++) {
                    const float wx = fp_weight(ax, ox, t);
                    if (wx != 0.f) row += wx * yr[(int64_t)ox * p.yStride[3]];
                }
            }
            acc += wy * row;
        }
    }
    p.x[(int64_t)b * p.xStride[0] + (int64_t)c * p.xStride[1] + (int64_t)s * p.xStride[2] + (int64_t)t * p.xStride[3]] = acc;
}

} // namespace sg3

extern "C" {

int sg3_face_pool(const sg3_face_pool_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->y, "face_pool: null tensor");
    SG3_REQUIRE(p->B > 0 && p->C > 0 && p->H > 0 && p->W > 0, "face_pool: sizes must be positive (B %d, C %d, %d x %d)", p->B, p->C, p->H, p->W);
    SG3_REQUIRE(p->H <= (1 << 20) && p->W <= (1 << 20), "face_pool: image too large");
    SG3_REQUIRE(p->pool == (p->H != 256 ? 1 : 0), "face_pool: pool must be set exactly when H != 256 (the reference's rule)");
    SG3_REQUIRE(p->pool || p->W >= 220, "face_pool: an unpooled image needs at least 220 columns for the crop");
    const int64_t threads = (int64_t)p->B * p->C * (p->adjoint ? (int64_t)p->H * p->W : (int64_t)kOut * kOut);
    SG3_REQUIRE((int64_t)p->B * p->C < (1ll << 31), "face_pool: too many planes");
    const int64_t blocks = ceil_div64(threads, kFpThreads);
    SG3_REQUIRE(blocks < (1ll << 31), "face_pool: batch too large for one launch");
    if (p->adjoint) hipLaunchKernelGGL(face_pool_adjoint_kernel, dim3((unsigned)blocks), dim3(kFpThreads), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(face_pool_kernel, dim3((unsigned)blocks), dim3(kFpThreads), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("face_pool_kernel");
    return SG3_OK;
}

} // extern "C"
