// sg3_image_finish.hip -- rendered float images -> the uint8 tiles the editing scripts save, resized if asked, in one launch.
//
// Reference: utils/common.py:39-45 `tensor2im` (float32 numpy: (x + 1) / 2, clip to [0, 1], * 255, truncating astype(uint8)), then
// PIL `Image.resize((w, h))` (default BICUBIC, reducing_gap None) as inversion/scripts/inference_editing.py:82-85 does.  The result is
// bit-identical to `np.array(tensor2im(x[b]).resize((w, h)))`:
//   * the tensor2im arithmetic is the same IEEE single-precision operations in the same order; this file is compiled with
//     -ffp-contract=off (csrc/Makefile) and the products are written with __fmul_rn so that no FMA can fuse them.  NaN input is
//     outside the contract (fminf / fmaxf drop it where numpy's clip would propagate it).
//   * PIL's uint8 resampler is separable: a horizontal pass into an 8-bit intermediate, then a vertical pass, each output sample
//     `clip8((1 << 21) + sum_t u8[xmin + t] * k[t]) = clamp(ss >> 22, 0, 255)` with int32 fixed-point taps.  The taps are built on
//     the host in double precision by sg3_resample_coeffs (below) and checked there against the installed PIL
//     (tests/test_image_finish_cpu.py); the kernels only do integer multiply-adds.  A pass whose size does not change is skipped,
//     as PIL skips it; when neither changes PIL returns a copy and the copy kernel runs.
//
// Work split (DESIGN.md "InterFaceGAN editing"): resample_kernel takes one image and a band of TY output rows per workgroup.  The
// input rows the band needs are streamed through LDS CH rows at a time (float -> uint8 on the way in, planar per channel), the
// horizontal pass writes its 8-bit rows to a second LDS buffer, and the vertical pass reads that buffer and stores the band.  Each
// input float is read once per band that needs its row: 57 rows for 44 at 1024 -> 256 (TY = 11), the overlap served from cache.
// No workspace, one launch for all B images.  copy_kernel (no resize) converts 4 pixels per thread with 16-byte loads.
#include "sg3_common.h"
#include <cmath>
#include <vector>

namespace sg3 {

static constexpr int kPrecisionBits = 22;          // 32 - 8 - 2, as PIL's 8-bit resampler
static constexpr int kThreads = 256;
static constexpr int kStageRows = 4;               // CH: input rows in flight per workgroup step
static constexpr int kLdsBudget = 56 * 1024;       // three workgroups per CU (160 KiB)

__device__ __forceinline__ uint32_t to_u8(float v) {
    // tensor2im: np.clip((arr + 1) / 2, 0, 1) * 255 then astype(uint8).  x / 2 and x * 0.5f round identically.
    float t = __fmul_rn(__fadd_rn(v, 1.0f), 0.5f);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    return (uint32_t)(int)__fmul_rn(t, 255.0f);
}

__device__ __forceinline__ uint32_t clip8(int ss) {
    const int v = ss >> kPrecisionBits;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

struct FinishLaunch {
    sg3_image_finish_params p;
    int needH, needV;
    int TY;          // output rows per workgroup
    int rinMax;      // input rows a band may need (LDS rows of the horizontal result)
    int pitch;       // bytes per LDS row of the horizontal result (w * 3, rounded up to 4)
    int vecIn;       // x rows are 16-byte aligned float4 runs (stride-1 x, W % 4 == 0)
};

template <int KH>
__global__ void __launch_bounds__(kThreads)
resample_kernel(FinishLaunch L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const sg3_image_finish_params& p = L.p;
    const int b = blockIdx.y;
    const int oy0 = blockIdx.x * L.TY;
    const int oy1 = min(oy0 + L.TY, p.h);
    const int tid = threadIdx.x;
    int r0, r1;
    if (L.needV) { r0 = p.boundsV[2 * oy0]; r1 = p.boundsV[2 * (oy1 - 1)] + p.boundsV[2 * (oy1 - 1) + 1]; }
    else { r0 = oy0; r1 = oy1; }
    r1 = min(r1, r0 + L.rinMax);                                          // memory guard: the host sized rinMax from the same table
    unsigned char* hbuf = lds;                                            // [rinMax][pitch]: horizontal result, pixel-interleaved
    unsigned char* stage = lds + (size_t)L.rinMax * L.pitch;              // [CH][3][W]: tensor2im of the input rows, planar
    const float* xb = p.x + (int64_t)b * p.xStride[0];
    const int W = p.W, w = p.w;

    for (int ra = r0; ra < r1; ra += kStageRows) {
        const int nr = min(kStageRows, r1 - ra);
        // rows [ra, ra + nr): float -> uint8 into `stage` (or straight into hbuf when the width does not change)
        if (L.vecIn) {
            // all 3 * CH float4 loads of a thread are issued before the first is used
            const int W4 = W >> 2;
            for (int i = tid; i - tid < W4; i += kThreads) {
                float4 v[kStageRows * 3];
#pragma unroll
                for (int rc = 0; rc < kStageRows * 3; rc++) {
                    const int rr = rc / 3, c = rc % 3;
                    v[rc] = (rr < nr && i < W4)
                        ? reinterpret_cast<const float4*>(xb + c * p.xStride[1] + (int64_t)(ra + rr) * p.xStride[2])[i]
                        : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int rc = 0; rc < kStageRows * 3; rc++) {
                    const int rr = rc / 3, c = rc % 3;
                    if (rr < nr && i < W4) {
                        if (L.needH) {
                            const uint32_t q = to_u8(v[rc].x) | (to_u8(v[rc].y) << 8) | (to_u8(v[rc].z) << 16) | (to_u8(v[rc].w) << 24);
                            *reinterpret_cast<uint32_t*>(stage + (size_t)(rr * 3 + c) * W + 4 * i) = q;
                        } else {
                            unsigned char* d = hbuf + (size_t)(ra - r0 + rr) * L.pitch + 12 * i + c;
                            d[0] = (unsigned char)to_u8(v[rc].x); d[3] = (unsigned char)to_u8(v[rc].y);
                            d[6] = (unsigned char)to_u8(v[rc].z); d[9] = (unsigned char)to_u8(v[rc].w);
                        }
                    }
                }
            }
        } else {
            for (int rr = 0; rr < nr; rr++)
                for (int c = 0; c < 3; c++) {
                    const float* src = xb + c * p.xStride[1] + (int64_t)(ra + rr) * p.xStride[2];
                    for (int i = tid; i < W; i += kThreads) {
                        const uint32_t q = to_u8(src[(int64_t)i * p.xStride[3]]);
                        if (L.needH) stage[(size_t)(rr * 3 + c) * W + i] = (unsigned char)q;
                        else hbuf[(size_t)(ra - r0 + rr) * L.pitch + 3 * i + c] = (unsigned char)q;
                    }
                }
        }
        __syncthreads();
        if (L.needH) {
            for (int ox = tid; ox < w; ox += kThreads) {
                const int xmin = max(p.boundsH[2 * ox], 0), n = min(p.boundsH[2 * ox + 1], W - xmin);
                int k[KH];
#pragma unroll
                for (int t = 0; t < KH; t++) k[t] = t < n ? p.coeffsH[(size_t)ox * p.kH + t] : 0;
                for (int rr = 0; rr < nr; rr++) {
                    unsigned char* d = hbuf + (size_t)(ra - r0 + rr) * L.pitch + 3 * ox;
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const unsigned char* s = stage + (size_t)(rr * 3 + c) * W + xmin;
                        int ss = 1 << (kPrecisionBits - 1);
#pragma unroll
                        for (int t = 0; t < KH; t++)
                            if (t < n) ss += (int)s[t] * k[t];
                        d[c] = (unsigned char)clip8(ss);
                    }
                }
            }
            __syncthreads();                                            // stage is overwritten by the next rows
        }
    }
    if (!L.needH) __syncthreads();

    // vertical pass over the band: thread -> one byte (x, c) of an output row, so stores of a row are contiguous
    const int rowBytes = 3 * w;
    const int total = (oy1 - oy0) * rowBytes;
    unsigned char* yb = p.y + (int64_t)b * p.yStride[0];
    for (int idx = tid; idx < total; idx += kThreads) {
        const int oyl = idx / rowBytes;
        const int rem = idx - oyl * rowBytes;
        const int oy = oy0 + oyl;
        uint32_t v;
        if (L.needV) {
            const int ymin = max(p.boundsV[2 * oy] - r0, 0), n = min(p.boundsV[2 * oy + 1], r1 - r0 - ymin);
            const int* kv = p.coeffsV + (size_t)oy * p.kV;
            const unsigned char* s = hbuf + (size_t)ymin * L.pitch + rem;
            int ss = 1 << (kPrecisionBits - 1);
            for (int t = 0; t < n; t++) ss += (int)s[(size_t)t * L.pitch] * kv[t];
            v = clip8(ss);
        } else {
            v = hbuf[(size_t)oyl * L.pitch + rem];
        }
        const int ox = rem / 3, c = rem - 3 * (rem / 3);
        yb[(int64_t)oy * p.yStride[1] + (int64_t)ox * p.yStride[2] + (int64_t)c * p.yStride[3]] = (unsigned char)v;
    }
}

// no resize: thread -> 4 consecutive pixels of one row (VEC: three float4 loads, three 4-byte stores) or one pixel
template <bool VEC>
__global__ void __launch_bounds__(kThreads)
copy_kernel(sg3_image_finish_params p) {
    const int per = VEC ? 4 : 1;
    const int groups = p.W / per;
    const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t perImage = (int64_t)p.H * groups;
    if (g >= perImage * p.B) return;
    const int b = (int)(g / perImage);
    const int64_t r = g - b * perImage;
    const int yy = (int)(r / groups), x0 = (int)(r - (int64_t)yy * groups) * per;
    const float* xr = p.x + (int64_t)b * p.xStride[0] + (int64_t)yy * p.xStride[2];
    unsigned char* yr = p.y + (int64_t)b * p.yStride[0] + (int64_t)yy * p.yStride[1];
    if (VEC) {
        const float4 c0 = *reinterpret_cast<const float4*>(xr + x0);
        const float4 c1 = *reinterpret_cast<const float4*>(xr + p.xStride[1] + x0);
        const float4 c2 = *reinterpret_cast<const float4*>(xr + 2 * p.xStride[1] + x0);
        // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
        const uint32_t w0 = to_u8(c0.x) | (to_u8(c1.x) << 8) | (to_u8(c2.x) << 16) | (to_u8(c0.y) << 24);
        const uint32_t w1 = to_u8(c1.y) | (to_u8(c2.y) << 8) | (to_u8(c0.z) << 16) | (to_u8(c1.z) << 24);
        const uint32_t w2 = to_u8(c2.z) | (to_u8(c0.w) << 8) | (to_u8(c1.w) << 16) | (to_u8(c2.w) << 24);
        uint32_t* d = reinterpret_cast<uint32_t*>(yr + 3 * (int64_t)x0);
        d[0] = w0; d[1] = w1; d[2] = w2;
    } else {
        for (int c = 0; c < 3; c++)
            yr[(int64_t)x0 * p.yStride[2] + (int64_t)c * p.yStride[3]] =
                (unsigned char)to_u8(xr[(int64_t)c * p.xStride[1] + (int64_t)x0 * p.xStride[3]]);
    }
}

static double bicubic(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

} // namespace sg3

extern "C" {

int sg3_resample_coeffs(int32_t inSize, int32_t outSize, int32_t* bounds, int32_t* coeffs) {
    using namespace sg3;
    SG3_REQUIRE(inSize > 0 && outSize > 0 && inSize <= (1 << 20) && outSize <= (1 << 20), "resample_coeffs: sizes must be in [1, 2^20]");
    const double support0 = 2.0;                                    // bicubic
    const double scale = (double)inSize / outSize;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = support0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    if (!bounds && !coeffs) return ksize;
    SG3_REQUIRE(bounds && coeffs, "resample_coeffs: bounds and coeffs must both be given (or both NULL to query the tap count)");
    std::vector<double> k(ksize);
    for (int xx = 0; xx < outSize; xx++) {
        const double center = (xx + 0.5) * scale;
        const double ss = 1.0 / filterscale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inSize) xmax = inSize;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; x++) {
            const double v = bicubic((x + xmin - center + 0.5) * ss);
            k[x] = v;
            ww += v;
        }
        for (int x = 0; x < ksize; x++) {
            double v = x < xmax ? k[x] : 0.0;
            if (x < xmax && ww != 0.0) v /= ww;
            coeffs[(size_t)xx * ksize + x] = v < 0 ? (int32_t)(-0.5 + v * (1 << kPrecisionBits)) : (int32_t)(0.5 + v * (1 << kPrecisionBits));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

int sg3_image_finish(const sg3_image_finish_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->y, "image_finish: null tensor");
    SG3_REQUIRE(p->B > 0 && p->H > 0 && p->W > 0 && p->h > 0 && p->w > 0 && p->B <= 65535, "image_finish: bad shape");
    const int needH = p->w != p->W, needV = p->h != p->H;
    SG3_REQUIRE(!needH || (p->boundsH && p->coeffsH && p->kH > 0), "image_finish: the width changes but no horizontal table is given");
    SG3_REQUIRE(!needV || (p->boundsV && p->coeffsV && p->kV > 0), "image_finish: the height changes but no vertical table is given");
    hipStream_t st = (hipStream_t)stream;
    if (!needH && !needV) {
        const bool vec = p->xStride[3] == 1 && p->W % 4 == 0 && aligned16(p->x) && p->xStride[0] % 4 == 0 && p->xStride[1] % 4 == 0 &&
                         p->xStride[2] % 4 == 0 && p->yStride[3] == 1 && p->yStride[2] == 3 && ((uintptr_t)p->y & 3) == 0 &&
                         p->yStride[1] % 4 == 0 && p->yStride[0] % 4 == 0;
        const int64_t threads = (int64_t)p->B * p->H * (p->W / (vec ? 4 : 1));
        const int64_t blocks = ceil_div64(threads, kThreads);
        SG3_REQUIRE(blocks < (1ll << 31), "image_finish: batch too large for one launch");
        if (vec) hipLaunchKernelGGL(copy_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, st, *p);
        else hipLaunchKernelGGL(copy_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, *p);
        SG3_LAUNCH_CHECK("image_finish copy_kernel");
        return SG3_OK;
    }
    // the tables live on the device; their bounds are read back once per call only through the geometry below, which needs the
    // vertical windows: recompute them on the host (cheap, double precision, same function) instead of a device read
    std::vector<int32_t> bv;
    if (needV) {
        const int kv = sg3_resample_coeffs(p->H, p->h, nullptr, nullptr);
        SG3_REQUIRE(kv == p->kV, "image_finish: kV = %d does not match the table of %d -> %d rows (%d taps)", p->kV, p->H, p->h, kv);
        std::vector<int32_t> cv((size_t)p->h * kv);
        bv.resize(2 * (size_t)p->h);
        sg3_resample_coeffs(p->H, p->h, bv.data(), cv.data());
    }
    if (needH) {
        const int kh = sg3_resample_coeffs(p->W, p->w, nullptr, nullptr);
        SG3_REQUIRE(kh == p->kH, "image_finish: kH = %d does not match the table of %d -> %d columns (%d taps)", p->kH, p->W, p->w, kh);
        SG3_REQUIRE(kh <= 64, "image_finish: a %d -> %d width reduction needs %d taps (at most 64 supported)", p->W, p->w, kh);
    }
    FinishLaunch L;
    L.p = *p;
    L.needH = needH; L.needV = needV;
    L.pitch = (3 * p->w + 3) & ~3;
    L.vecIn = p->xStride[3] == 1 && p->W % 4 == 0 && aligned16(p->x) && p->xStride[0] % 4 == 0 && p->xStride[1] % 4 == 0 &&
              p->xStride[2] % 4 == 0;
    const size_t stageBytes = needH ? (size_t)kStageRows * 3 * p->W : 0;
    auto rows_for = [&](int ty) {
        int m = 0;
        for (int oy0 = 0; oy0 < p->h; oy0 += ty) {
            const int oy1 = oy0 + ty < p->h ? oy0 + ty : p->h;
            const int r = needV ? bv[2 * (oy1 - 1)] + bv[2 * (oy1 - 1) + 1] - bv[2 * oy0] : oy1 - oy0;
            m = r > m ? r : m;
        }
        return m;
    };
    L.TY = 0;
    for (int ty = 32; ty >= 1; ty--) {
        const int rin = rows_for(ty);
        if (stageBytes + (size_t)rin * L.pitch <= (size_t)kLdsBudget) { L.TY = ty; L.rinMax = rin; break; }
    }
    SG3_REQUIRE(L.TY > 0, "image_finish: %dx%d -> %dx%d does not fit the LDS budget of one workgroup", p->W, p->H, p->w, p->h);
    const size_t lds = stageBytes + (size_t)L.rinMax * L.pitch;
    const dim3 grid((unsigned)ceil_div(p->h, L.TY), (unsigned)p->B);
    if (!needH || p->kH <= 8) hipLaunchKernelGGL(resample_kernel<8>, grid, dim3(kThreads), lds, st, L);
    else if (p->kH <= 24) hipLaunchKernelGGL(resample_kernel<24>, grid, dim3(kThreads), lds, st, L);
    else hipLaunchKernelGGL(resample_kernel<64>, grid, dim3(kThreads), lds, st, L);
    SG3_LAUNCH_CHECK("image_finish resample_kernel");
    return SG3_OK;
}

} // extern "C"
