// sg3_flrelu_host.hip -- the host side of filtered_lrelu: the lookup from a plan entry to its streaming kernel, the launchers, the
// two small kernels (pointwise, finish-partials) and the C entry points.  The streaming kernel and its instantiations live in
// sg3_filtered_lrelu.hip, which is compiled in parts; what the two files share is sg3_flrelu_kernels.h.  Built with
// -fno-honor-nans like the kernel file (the two kernels here are compiled under it too).
#include "sg3_flrelu_kernels.h"
#include <atomic>
#include <utility>

namespace sg3 {

// ---------------------------------------------------------------------------
// up = down = 1, 1x1 filters: y = clamp(lrelu((x + b) * fu * gain)) * fd   (ToRGB layer: clamp(x + b))
struct PointParams {
    const void* x; void* y; const void* b;
    const float* fu; const float* fd;
    int N, C, H, W;
    long long xs[4], ys[4], bStride;
    int px0, py0, yH, yW;
    float gain, slope, clamp;
};

template <typename T>
__global__ void __launch_bounds__(256)
flrelu_pointwise_kernel(PointParams p) {
    const float fu = p.fu[0], fd = p.fd[0];
    const long long total = (long long)p.N * p.C * p.yH * p.yW;
    const long long gs = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gs) {
        const int ox = (int)(idx % p.yW); long long t = idx / p.yW;
        const int oy = (int)(t % p.yH); t /= p.yH;
        const int c = (int)(t % p.C); const int n = (int)(t / p.C);
        const int ix = ox - p.px0, iy = oy - p.py0;
        float v = 0.f;
        if ((unsigned)ix < (unsigned)p.W && (unsigned)iy < (unsigned)p.H)
            v = io<T>::ld((const T*)p.x + n * p.xs[0] + c * p.xs[1] + iy * p.xs[2] + ix * p.xs[3]) + (p.b ? io<T>::ld((const T*)p.b + c * p.bStride) : 0.f);
        v *= fu * p.gain;
        v = v < 0.f ? v * p.slope : v;
        v = fminf(fmaxf(v, -p.clamp), p.clamp);
        io<T>::st((T*)p.y + n * p.ys[0] + c * p.ys[1] + oy * p.ys[2] + ox * p.ys[3], v * fd);
    }
}

// ---------------------------------------------------------------------------
// Which kernel, how many launches and what grid a call takes: plan_filtered_lrelu, sg3_flrelu_plan.h.
//
// The up-4 separable plain forward has two forms that compute the same thing bit for bit: the default (up taps placed by hand, at
// most 128 VGPRs, four waves per SIMD) and the earlier one (`Stream`'s WIDE).  A process setting, seeded ONCE from the environment
// (SG3_FLRELU_UP4_WIDE=1: A/B timing) and changed only by an explicit sg3_filtered_lrelu_force_up4_wide call (the bit-identity test).
static std::atomic<int> g_up4_wide{[] { const char* e = getenv("SG3_FLRELU_UP4_WIDE"); return (e && e[0] == '1') ? 1 : 0; }()};

// The per-workgroup partial sums / maxima an adjoint launch left ([N][C][slots] each) -> the bias gradient db[c] = sum over (n, slot)
// and max |dx| = max over everything, in one small launch (as torch ops: a strided reduction and a max, ~19 us per layer and PTI step).
// One block: thread per channel, (n, slot) walked in order -- a fixed summation order, so db is reproducible.
__global__ void __launch_bounds__(256)
flrelu_finish_partials_kernel(const float* __restrict__ psum, const float* __restrict__ pmax, int N, int C, int slots,
                              float* __restrict__ db, float* __restrict__ amax) {
    __shared__ float red[4];
    float mx = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int n = 0; n < N; n++) {
            const size_t base = ((size_t)n * C + c) * slots;
            for (int k = 0; k < slots; k++) {
                s += psum[base + k];
                if (pmax) mx = __builtin_fmaxf(mx, pmax[base + k]);
            }
        }
        db[c] = s;
    }
    if (!amax) return;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) mx = __builtin_fmaxf(mx, __shfl_xor(mx, m));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) amax[0] = __builtin_fmaxf(__builtin_fmaxf(red[0], red[1]), __builtin_fmaxf(red[2], red[3]));
}

// The kernel of one plan entry: the 82 instantiations per tensor type (38 leaves of `stream_kernel_leaf`, each with the D vertical
// phases of its down factor), nullptr for coordinates none of them has.
template <typename T, int U, int D, int S, int G, int... R>
static StreamKernel stream_kernel_radial(int radial, int vph, std::integer_sequence<int, R...>) {
    StreamKernel f = nullptr;
    ((radial == R ? (void)(f = stream_kernel_leaf<T, U, D, R, S, G, 0>(vph)) : (void)0), ...);
    return f;
}
template <typename T>
static StreamKernel stream_kernel(const FlreluPlan& pl, int i) {
    typedef std::integer_sequence<int, 0, 1, 2, 5, 6> Forward;     // separable | 12x12 | 12x12 flipped | 12x12 with mirror-symmetric rows | the same, flipped
    typedef std::integer_sequence<int, 0, 3, 4> Adjoint;           // separable | 12x12 up filter | the same, flipped
    const int U = pl.U[i], D = pl.D[i], V = pl.VPH[i], R = pl.RADIAL[i], S = pl.SIGNS[i], G = pl.G[i];
    if (pl.WIDE[i]) {                                              // the earlier form of the up-4 separable plain forward
        if (U != 4 || D != 2 || R != 0 || S != 0) return nullptr;
        return G == 1 ? stream_kernel_leaf<T, 4, 2, 0, 0, 1, 1>(V) : G == 2 ? stream_kernel_leaf<T, 4, 2, 0, 0, 2, 1>(V) : nullptr;
    }
    if (S == 2) {                                                  // adjoint: up 2, one plane per wave
        if (U != 2 || G != 1) return nullptr;
        return D == 2 ? stream_kernel_radial<T, 2, 2, 2, 1>(R, V, Adjoint()) : D == 4 ? stream_kernel_radial<T, 2, 4, 2, 1>(R, V, Adjoint()) : nullptr;
    }
    if (D != 2 || (U != 2 && U != 4)) return nullptr;
    if (S == 1 && G == 1) return U == 2 ? stream_kernel_radial<T, 2, 2, 1, 1>(R, V, Forward()) : stream_kernel_radial<T, 4, 2, 1, 1>(R, V, Forward());
    if (S == 0 && G == 1) return U == 2 ? stream_kernel_radial<T, 2, 2, 0, 1>(R, V, Forward()) : stream_kernel_radial<T, 4, 2, 0, 1>(R, V, Forward());
    if (S == 0 && G == 2) return U == 2 ? stream_kernel_radial<T, 2, 2, 0, 2>(R, V, Forward()) : stream_kernel_radial<T, 4, 2, 0, 2>(R, V, Forward());
    return nullptr;
}
// the same for either tensor type, and what names the coordinates when there is none
static StreamKernel stream_kernel(int dtype, const FlreluPlan& pl, int i) {
    const StreamKernel kernel = dtype == SG3_F32 ? stream_kernel<float>(pl, i) : stream_kernel<_Float16>(pl, i);
    if (!kernel)
        set_error("filtered_lrelu: no flrelu_stream_kernel<U=%d, D=%d, VPH=%d, RADIAL=%d, SIGNS=%d, G=%d, WIDE=%d>", pl.U[i], pl.D[i], pl.VPH[i],
                  pl.RADIAL[i], pl.SIGNS[i], pl.G[i], pl.WIDE[i]);
    return kernel;
}

static int launch_stream(const sg3_filtered_lrelu_params& q, const FlreluPlan& pl, hipStream_t st) {
    StreamParams p;
    p.x = q.x; p.y = q.y; p.b = q.b; p.fu = q.fu; p.fd = q.fd;
    p.C = q.C; p.planes = q.N * q.C; p.xH = q.xH; p.xW = q.xW; p.yH = q.yH; p.yW = q.yW;
    p.xsN = q.xStride[0]; p.xsC = q.xStride[1]; p.xsH = q.xStride[2];
    p.ysN = q.yStride[0]; p.ysC = q.yStride[1]; p.ysH = q.yStride[2];
    p.bStride = q.bStride;
    p.px0 = q.px0; p.py0 = q.py0;
    p.gain = q.gain; p.slope = q.slope; p.clamp = q.clamp; p.flip = q.flip;
    p.fastAct = pl.fastAct;

    p.s = q.s; p.sH = q.sH; p.sWb = q.sWbytes; p.sx = q.sx; p.sy = q.sy;
    p.ysum = q.ySumPartial;
    p.ymax = q.yAbsMaxPartial;
#ifdef SG3_STAMPS
    p.stamps = g_stamps;
#endif
    p.nChunks = pl.nChunks; p.CH = pl.chunkRows;
    for (int i = 0; i < pl.launches; i++) {
        p.nStrips = pl.nStrips[i]; p.TW = pl.TW[i]; p.ox0Base = pl.ox0Base[i]; p.wideBlocks = pl.wideBlocks[i]; p.totalBlocks = pl.totalBlocks[i];
        const StreamKernel kernel = stream_kernel(q.dtype, pl, i);
        if (!kernel) return SG3_NO_KERNEL;             // sg3_filtered_lrelu_dispatch has checked: not reached through sg3_filtered_lrelu
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.totalBlocks), dim3(64), 0, st, p);
        SG3_LAUNCH_CHECK("flrelu_stream_kernel");
    }
    return SG3_OK;
}

template <typename T>
static int launch_pointwise(const sg3_filtered_lrelu_params& q, const FlreluPlan& pl, hipStream_t st) {
    PointParams p;
    p.x = q.x; p.y = q.y; p.b = q.b; p.fu = q.fu; p.fd = q.fd;
    p.N = q.N; p.C = q.C; p.H = q.xH; p.W = q.xW; p.yH = q.yH; p.yW = q.yW;
    for (int i = 0; i < 4; i++) { p.xs[i] = q.xStride[i]; p.ys[i] = q.yStride[i]; }
    p.bStride = q.bStride; p.px0 = q.px0; p.py0 = q.py0;
    p.gain = q.gain; p.slope = q.slope; p.clamp = q.clamp;
    hipLaunchKernelGGL((flrelu_pointwise_kernel<T>), dim3((unsigned)pl.totalBlocks[0]), dim3(256), 0, st, p);
    SG3_LAUNCH_CHECK("flrelu_pointwise_kernel");
    return SG3_OK;
}

} // namespace sg3

extern "C" {

int sg3_filtered_lrelu_has_kernel(int up, int down, int fuW, int fuH, int fdW, int fdH) {
    return (sg3::stream_supported(up, down, fuW, fuH, fdW, fdH) || sg3::pointwise_supported(up, down, fuW, fuH, fdW, fdH)) ? 1 : 0;
}

int sg3_filtered_lrelu_sum_slots(int N, int C, int yH, int yW, int down) {
    if (N <= 0 || C <= 0 || yH <= 0 || yW <= 0 || (down != 2 && down != 4)) return 0;
    int nStrips, TW, nChunks, CH;
    sg3::stream_grid(N, C, yH, yW, down, nStrips, TW, nChunks, CH);
    return nStrips * nChunks;
}

int sg3_filtered_lrelu_finish_partials(const float* sumPartial, const float* absMaxPartial, int N, int C, int slots, float* db, float* absMax, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(sumPartial && db && N > 0 && C > 0 && slots > 0, "filtered_lrelu_finish_partials: bad arguments");
    SG3_REQUIRE(!absMax == !absMaxPartial, "filtered_lrelu_finish_partials: absMaxPartial and absMax come together");
    hipLaunchKernelGGL(flrelu_finish_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sumPartial, absMaxPartial, N, C, slots, db, absMax);
    SG3_LAUNCH_CHECK("flrelu_finish_partials_kernel");
    return SG3_OK;
}

int sg3_filtered_lrelu_shape(int xH, int xW, int up, int down, int fuW, int fuH, int fdW, int fdH,
                             int px0, int px1, int py0, int py1, int* yH, int* yW, int* sH, int* sWbytes, int* swLimit) {
    using namespace sg3;
    SG3_REQUIRE(xH > 0 && xW > 0, "x is empty");
    SG3_REQUIRE(up >= 1 && down >= 1, "up and down must be at least 1");
    SG3_REQUIRE(fuW >= 1 && fdW >= 1, "fu and fd must not be empty");
    // separable filters have the same extent along both axes (reference :63-66 uses size(0) for the height)
    const int64_t fut_w = fuW - 1, fut_h = (fuH ? fuH : fuW) - 1;
    const int64_t fdt_w = fdW - 1, fdt_h = (fdH ? fdH : fdW) - 1;
    const int64_t cw = (int64_t)xW * up + (px0 + px1) - fut_w;
    const int64_t ch = (int64_t)xH * up + (py0 + py1) - fut_h;
    SG3_REQUIRE(cw > fdt_w && ch > fdt_h, "upsampled buffer must be at least the size of downsampling filter");
    SG3_REQUIRE(cw <= INT32_MAX && ch <= INT32_MAX, "upsampled buffer is too large");
    const int64_t ow = (cw - fdt_w + (down - 1)) / down;
    const int64_t oh = (ch - fdt_h + (down - 1)) / down;
    SG3_REQUIRE(ow > 0 && oh > 0, "output must be at least 1x1");
    const int64_t sw_active = ow * down - (down - 1) + fdt_w;
    const int64_t sh = oh * down - (down - 1) + fdt_h;
    const int64_t sw = (sw_active + 15) & ~(int64_t)15;
    SG3_REQUIRE(sh <= INT32_MAX && (sw >> 2) <= INT32_MAX, "signs is too large");
    if (yH) *yH = (int)oh;
    if (yW) *yW = (int)ow;
    if (sH) *sH = (int)sh;
    if (sWbytes) *sWbytes = (int)(sw >> 2);
    if (swLimit) *swLimit = (int)((sw_active + 3) >> 2);
    return SG3_OK;
}

float sg3_filtered_lrelu_fast_threshold(const float* fu, int fuW, int up, float gain, float slope, float clamp) {
    if (!fu || up < 1 || fuW < up) return -1.f;
    return sg3::fast_threshold(fu, fuW, up, gain, slope, clamp);
}

int sg3_filtered_lrelu_force_up4_wide(int wide) { return sg3::g_up4_wide.exchange(wide ? 1 : 0); }

// the plan of a call the older queries answer for: a tensor type the kernels have and a non-empty output, nothing else checked
static bool query_plan(const sg3_filtered_lrelu_params* p, sg3::FlreluPlan& pl) {
    if (!p || (p->dtype != SG3_F32 && p->dtype != SG3_F16) || p->N <= 0 || p->C <= 0 || p->yH <= 0 || p->yW <= 0) return false;
    pl = sg3::plan_filtered_lrelu(*p, sg3::FlreluKnobs::env(), sg3::g_up4_wide.load(std::memory_order_relaxed));
    return pl.kind == SG3_FLRELU_STREAM;
}

int sg3_filtered_lrelu_planes_per_wave(const sg3_filtered_lrelu_params* p) {
    sg3::FlreluPlan pl;
    return query_plan(p, pl) ? pl.planesPerWave : 0;
}

int sg3_filtered_lrelu_stream_grid(const sg3_filtered_lrelu_params* p, int* nStrips, int* stripW, int* nFullStrips, int* nChunks, int* chunkRows) {
    sg3::FlreluPlan pl;
    if (!query_plan(p, pl)) return 0;                                   // not a streaming-kernel call
    const bool mixed = pl.planesPerWave == 3;                           // launch 0 takes the full strips, one more strip follows them
    if (nStrips) *nStrips = pl.nStrips[0] + (mixed ? 1 : 0);
    if (stripW) *stripW = pl.TW[0];
    if (nFullStrips) *nFullStrips = mixed ? pl.nStrips[0] : 0;
    if (nChunks) *nChunks = pl.nChunks;
    if (chunkRows) *chunkRows = pl.chunkRows;
    return 1;
}

int sg3_filtered_lrelu_dispatch(const sg3_filtered_lrelu_params* p, sg3_filtered_lrelu_dispatch_info* out) {
    using namespace sg3;
    SG3_REQUIRE(p && out, "filtered_lrelu_dispatch: null argument");
    SG3_REQUIRE(p->N > 0 && p->C > 0 && p->xH > 0 && p->xW > 0, "filtered_lrelu: x is empty");
    SG3_REQUIRE(p->yH > 0 && p->yW > 0, "filtered_lrelu: output must be at least 1x1");
    SG3_REQUIRE(p->up >= 1 && p->down >= 1, "filtered_lrelu: up and down must be at least 1");
    SG3_REQUIRE(p->dtype == SG3_F32 || p->dtype == SG3_F16, "filtered_lrelu: x must be float16 or float32");
    SG3_REQUIRE(!(p->writeSigns && p->readSigns), "filtered_lrelu: cannot read and write signs in one call");
    *out = plan_filtered_lrelu(*p, FlreluKnobs::env(), g_up4_wide.load(std::memory_order_relaxed));
    if (out->kind == SG3_FLRELU_NONE) {
        set_error("filtered_lrelu: no fused kernel for up=%d down=%d fu=%dx%d fd=%dx%d signs=%d", p->up, p->down,
                  p->fuW, p->fuH, p->fdW, p->fdH, (int)(p->writeSigns || p->readSigns));
        return SG3_NO_KERNEL;
    }
    SG3_REQUIRE(out->launches > 0, "filtered_lrelu: grid too large");
    // every launch of the plan has its kernel in the library (host only: the pointers are looked up, not followed).  A coordinate the
    // plan chooses and no part of sg3_filtered_lrelu.hip instantiates is an error here, not a quiet trip through the generic composition
    for (int i = 0; out->kind == SG3_FLRELU_STREAM && i < out->launches; i++)
        if (!stream_kernel(p->dtype, *out, i)) return SG3_NO_KERNEL;
    return SG3_OK;
}

int sg3_filtered_lrelu(const sg3_filtered_lrelu_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->y && p->fu && p->fd, "filtered_lrelu: null tensor");
    FlreluPlan pl;
    const int rc = sg3_filtered_lrelu_dispatch(p, &pl);
    if (rc != SG3_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (pl.kind == SG3_FLRELU_POINTWISE) return p->dtype == SG3_F32 ? launch_pointwise<float>(*p, pl, st) : launch_pointwise<_Float16>(*p, pl, st);
    return launch_stream(*p, pl, st);
}

} // extern "C"
