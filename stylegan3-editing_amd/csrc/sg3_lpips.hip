// sg3_lpips.hip -- what the LPIPS (AlexNet) criterion needs besides sg3_conv2d / sg3_conv2d_dgrad (criteria/lpips):
//
//   sg3_lpips_prepare / _bwd   z-score + zero canvas + pixel-unshuffle by 4, so that the 11x11 stride-4 pad-2 first convolution is
//                              a VALID 3x3 stride-1 convolution over 48 channels (runs on sg3_conv2d / sg3_conv2d_dgrad), and the adjoint
//   sg3_conv2d_k5              5x5 stride-1 pad-2 convolution as an exact-fp32 MFMA implicit GEMM (the conv2d_mfma_kernel scheme of
//                              sg3_conv2d.hip with 25 taps); serves the forward (bias + ReLU) and, on transposed flipped weights, the
//                              data gradient
//   sg3_maxpool3s2 / _bwd      MaxPool2d(3, 2); the backward in gather form with the head's addend and the ReLU mask fused in
//   sg3_lpips_head             per layer: channel-unit-normalise both feature maps, squared difference, 1x1 `lin`, spatial mean;
//                              on request the closed-form gradient with respect to the first map
//
// No float atomics: every sum has a fixed order, so every result is bit-identical on repeat.
#include "sg3_igemm_f32.h"

namespace sg3 {

// ---------------------------------------------------------------------------------------------------------------------------
// prepare: canvas[n][c*16 + ry*4 + rx][py][px] = zscore(x[n][c][4 py + ry - 2][4 px + rx - 2]) inside the image, 0 outside
struct PrepP {
    float* x; long long xs[4]; float* canvas; const float* scale;
    int N, H, W, PH, PW;
    float mean[3], std[3];
};

__global__ void __launch_bounds__(256)
lpips_prepare_kernel(PrepP p) {
    const size_t total = (size_t)p.N * 48 * p.PH * p.PW;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int px = (int)(e % p.PW); size_t t = e / p.PW;
    const int py = (int)(t % p.PH); t /= p.PH;
    const int ch = (int)(t % 48); const int n = (int)(t / 48);
    const int c = ch >> 4, ry = (ch >> 2) & 3, rx = ch & 3;
    const int y = 4 * py + ry - 2, x = 4 * px + rx - 2;
    float v = 0.f;
    if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W)
        v = (p.x[n * p.xs[0] + c * p.xs[1] + y * p.xs[2] + x * p.xs[3]] - p.mean[c]) / p.std[c];
    p.canvas[e] = v;
}

// the adjoint: dx[n][c][y][x] = dcanvas[...] / std[c] (* scale[0]); image pixels beyond the canvas (never read by the convolution) get 0
__global__ void __launch_bounds__(256)
lpips_prepare_bwd_kernel(PrepP p) {
    const size_t total = (size_t)p.N * 3 * p.H * p.W;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % p.W); size_t t = e / p.W;
    const int y = (int)(t % p.H); t /= p.H;
    const int c = (int)(t % 3); const int n = (int)(t / 3);
    const int cy = y + 2, cx = x + 2;
    float v = 0.f;
    if ((cy >> 2) < p.PH && (cx >> 2) < p.PW) {
        const int ch = c * 16 + (cy & 3) * 4 + (cx & 3);
        v = p.canvas[(((size_t)n * 48 + ch) * p.PH + (cy >> 2)) * p.PW + (cx >> 2)] / p.std[c];
        if (p.scale) v *= p.scale[0];
    }
    p.x[n * p.xs[0] + c * p.xs[1] + y * p.xs[2] + x * p.xs[3]] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// 5x5 stride-1 pad-2 convolution: conv2d_mfma_kernel (sg3_conv2d.hip) with 25 taps.  Packed weights [O][ceil(I/8)][25][8]; the
// 8-channel (ROWS + 4) x 36 input patch in LDS channel-interleaved by 4; next chunk global->registers under the MFMA loop.
// BM = 64 output channels x (ROWS rows x 32 columns): the A image is 64 x 204 floats = 51 KB, with the patch 60 KB (4 rows) --
// two workgroups per CU in the 160 KB LDS, inside the 64 KB a workgroup gets without asking.
struct K5P {
    const float* x; const float* wp; const float* bias; float* out;
    int N, I, O, H, W, relu;
    int nch, xTiles, yTiles, mTiles, totalBlocks;
};

constexpr int K5_TAPS = 25, K5_KC = 8, K5_BM = 64;

template <int TN>
__global__ void __launch_bounds__(256)
conv2d_k5_kernel(K5P p) {
    constexpr int KS = 5, TAPS = K5_TAPS, KC = K5_KC, WM = 2, WN = 2;
    constexpr int BM = K5_BM;
    constexpr int ROWS = WN * TN;
    constexpr int PH = ROWS - 1 + KS, PW = 31 + KS;
    constexpr int AS = TAPS * KC + 4;
    constexpr int PLANE = PH * PW * 4;
    constexpr int NPL = KC / 4;
    constexpr int A_V4 = BM * TAPS * KC / 4;
    constexpr int A_PER = (A_V4 + 255) / 256;
    constexpr int B_EL = KC * PH * PW;
    constexpr int B_PER = (B_EL + 255) / 256;
    static_assert(BM == WM * 32 && (BM * AS + NPL * PLANE) * 4 <= 64 * 1024, "one 32-channel MFMA tile per wave row; static LDS");

    __shared__ __attribute__((aligned(16))) float smem[BM * AS + NPL * PLANE];
    float* sA = smem;
    float* sB = smem + BM * AS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    int bid = xcd_block(blockIdx.x, p.totalBlocks);
    const int mt = bid % p.mTiles; bid /= p.mTiles;
    const int xt = bid % p.xTiles; bid /= p.xTiles;
    const int yt = bid % p.yTiles; const int n = bid / p.yTiles;
    const int o0 = mt * BM, x0 = xt * 32, y0 = yt * ROWS;
    const float* xin = p.x + (size_t)n * p.I * p.H * p.W;

    f32x16 acc[TN];
#pragma unroll
    for (int b = 0; b < TN; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[b][r] = 0.f;

    f32x4 ra[A_PER];
    float rb[B_PER];

    auto fetch = [&](int ch) {
#pragma unroll
        for (int q = 0; q < A_PER; q++) {
            const int v = tid + 256 * q;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (A_V4 % 256 == 0 || v < A_V4) {
                const int row = v / (TAPS * KC / 4), col = v % (TAPS * KC / 4);
                if (o0 + row < p.O)
                    val = *reinterpret_cast<const f32x4*>(p.wp + ((size_t)(o0 + row) * p.nch + ch) * (TAPS * KC) + col * 4);
            }
            ra[q] = val;
        }
#pragma unroll
        for (int q = 0; q < B_PER; q++) {
            const int e = tid + 256 * q;
            float val = 0.f;
            if (B_EL % 256 == 0 || e < B_EL) {
                const int px = e % PW, t = e / PW, py = t % PH, c = t / PH;
                const int ci = ch * KC + c, gy = y0 - 2 + py, gx = x0 - 2 + px;
                if (ci < p.I && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W)
                    val = xin[((size_t)ci * p.H + gy) * p.W + gx];
            }
            rb[q] = val;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < A_PER; q++) {
            const int v = tid + 256 * q;
            if (A_V4 % 256 == 0 || v < A_V4) {
                const int row = v / (TAPS * KC / 4), col = v % (TAPS * KC / 4);
                *reinterpret_cast<f32x4*>(sA + row * AS + col * 4) = ra[q];
            }
        }
#pragma unroll
        for (int q = 0; q < B_PER; q++) {
            const int e = tid + 256 * q;
            if (B_EL % 256 == 0 || e < B_EL) {
                const int px = e % PW, t = e / PW, py = t % PH, c = t / PH;
                sB[(c >> 2) * PLANE + (py * PW + px) * 4 + (c & 3)] = rb[q];
            }
        }
    };

    fetch(0);
    for (int ch = 0; ch < p.nch; ch++) {
        __syncthreads();
        stage();
        __syncthreads();
        if (ch + 1 < p.nch) fetch(ch + 1);
#pragma unroll
        for (int tap = 0; tap < TAPS; tap++) {
            const int ky = tap / KS, kx = tap % KS;
            const f32x4 fa = *reinterpret_cast<const f32x4*>(sA + (wm * 32 + li) * AS + tap * KC + 4 * lh);
            f32x4 fb[TN];
#pragma unroll
            for (int b = 0; b < TN; b++)
                fb[b] = *reinterpret_cast<const f32x4*>(sB + lh * PLANE + ((wn * TN + b + ky) * PW + li + kx) * 4);
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int b = 0; b < TN; b++)
                    acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], fb[b][q], acc[b], 0, 0, 0);
        }
    }

    float* outp = p.out + (size_t)n * p.O * p.H * p.W;
    const int gx = x0 + li;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (o >= p.O) continue;
        const float bv = p.bias ? p.bias[o] : 0.f;
#pragma unroll
        for (int b = 0; b < TN; b++) {
            const int gy = y0 + wn * TN + b;
            if (gy < p.H && gx < p.W) {
                float v = acc[b][r] + bv;
                if (p.relu) v = v < 0.f ? 0.f : v;
                outp[((size_t)o * p.H + gy) * p.W + gx] = v;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
conv2d_k5_pack_kernel(const float* w, float* wp, int O, int I, int nch) {
    const int o = blockIdx.x;
    float* dst = wp + (size_t)o * nch * K5_TAPS * K5_KC;
    for (int j = threadIdx.x; j < nch * K5_TAPS * K5_KC; j += 256) {
        const int c = j % K5_KC, t = (j / K5_KC) % K5_TAPS, ch = j / (K5_KC * K5_TAPS);
        const int i = ch * K5_KC + c;
        dst[j] = i < I ? w[((size_t)o * I + i) * K5_TAPS + t] : 0.f;
    }
}

template <int TN>
static int launch_k5(const sg3_conv2d_k5_params& q, hipStream_t st) {
    K5P p;
    p.x = q.x; p.wp = q.wPacked; p.bias = q.bias; p.out = q.out;
    p.N = q.N; p.I = q.I; p.O = q.O; p.H = q.H; p.W = q.W; p.relu = q.relu;
    p.nch = ceil_div(q.I, K5_KC);
    p.xTiles = ceil_div(q.W, 32); p.yTiles = ceil_div(q.H, 2 * TN); p.mTiles = ceil_div(q.O, K5_BM);
    const long long total = (long long)p.xTiles * p.yTiles * p.mTiles * q.N;
    if (total > 0x7fffffffLL) { set_error("conv2d_k5: grid too large"); return SG3_BAD_ARG; }
    p.totalBlocks = (int)total;
    hipLaunchKernelGGL(conv2d_k5_kernel<TN>, dim3((unsigned)p.totalBlocks), dim3(256), 0, st, p);
    SG3_LAUNCH_CHECK("conv2d_k5_kernel");
    return SG3_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
struct PoolP {
    const float* x; const float* dy; const float* addend; float* out; long long os[4];
    int N, C, H, W, OH, OW, relu;
};

__global__ void __launch_bounds__(256)
maxpool3s2_kernel(PoolP p) {
    const size_t total = (size_t)p.N * p.C * p.OH * p.OW;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int ox = (int)(e % p.OW); size_t t = e / p.OW;
    const int oy = (int)(t % p.OH); const size_t plane = t / p.OH;
    const float* src = p.x + (plane * p.H + 2 * oy) * p.W + 2 * ox;
    float m = src[0];
#pragma unroll
    for (int j = 1; j < 9; j++) {
        const float v = src[(j / 3) * p.W + (j % 3)];
        if (v > m || v != v) m = v;
    }
    p.out[e] = m;
}

// gather form: input pixel (y, x) looks at the <= 4 windows that cover it and takes dy of those whose first maximum (row-major
// scan, as F.max_pool2d records it) it is; windows in ascending (oy, ox) order, then the addend, then the ReLU mask
__global__ void __launch_bounds__(256)
maxpool3s2_bwd_kernel(PoolP p) {
    const size_t total = (size_t)p.N * p.C * p.H * p.W;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int x = (int)(e % p.W); size_t t = e / p.W;
    const int y = (int)(t % p.H); const size_t plane = t / p.H;
    const int c = (int)(plane % p.C); const int n = (int)(plane / p.C);
    const float* xp = p.x + plane * p.H * p.W;
    const float* dyp = p.dy + plane * p.OH * p.OW;
    const float self = xp[(size_t)y * p.W + x];
    float v = 0.f;
    const int oy0 = y >= 2 ? (y - 1) >> 1 : 0, oy1 = min(y >> 1, p.OH - 1);
    const int ox0 = x >= 2 ? (x - 1) >> 1 : 0, ox1 = min(x >> 1, p.OW - 1);
    for (int oy = oy0; oy <= oy1; oy++)
        for (int ox = ox0; ox <= ox1; ox++) {
            const float* src = xp + (size_t)(2 * oy) * p.W + 2 * ox;
            float m = src[0]; int arg = 0;
#pragma unroll
            for (int j = 1; j < 9; j++) {
                const float u = src[(j / 3) * p.W + (j % 3)];
                if (u > m || u != u) { m = u; arg = j; }
            }
            if (arg == (y - 2 * oy) * 3 + (x - 2 * ox)) v += dyp[(size_t)oy * p.OW + ox];
        }
    if (p.addend) v += p.addend[e];
    if (p.relu && !(self > 0.f)) v = 0.f;
    p.out[n * p.os[0] + c * p.os[1] + y * p.os[2] + x * p.os[3]] = v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// head: a workgroup takes G groups of 64 pixels; lane = pixel, the four waves split the channels (c = wave, wave + 4, ...) and meet
// in LDS in a fixed order.  Per sample the nb workgroup partials are summed by the workgroup whose (integer) ticket is the last.
struct HeadP {
    const float* fx; const float* fy; const float* lin; float* value; float* dfx; float* partial; int* counter;
    int N, C, hw, G, nb, relu;
};

constexpr int HEAD_MAX_BLOCKS = 256;
static inline int head_groups(long long hw) { return (int)((hw + 64LL * HEAD_MAX_BLOCKS - 1) / (64LL * HEAD_MAX_BLOCKS)); }
static inline int head_blocks(long long hw) { const long long g = head_groups(hw); return (int)((hw + 64 * g - 1) / (64 * g)); }

__global__ void __launch_bounds__(256)
lpips_head_kernel(HeadP p) {
    __shared__ float red[2][4][64];
    __shared__ double blk[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x / p.nb, b = blockIdx.x % p.nb;
    const size_t base = (size_t)n * p.C * p.hw;
    const float* fx = p.fx + base;
    const float* fy = p.fy + base;
    float* dfx = p.dfx ? p.dfx + base : nullptr;
    const float invHw = 1.f / (float)p.hw;
    double pixels = 0.0;          // the value's long sums run in double: the float32 result then carries input rounding only
    for (int g = 0; g < p.G; g++) {
        const int px = (b * p.G + g) * 64 + lane;
        const bool in = px < p.hw;
        float sx = 0.f, sy = 0.f;
        if (in)
            for (int c = wave; c < p.C; c += 4) {
                const float u = fx[(size_t)c * p.hw + px], v = fy[(size_t)c * p.hw + px];
                sx += u * u; sy += v * v;
            }
        red[0][wave][lane] = sx; red[1][wave][lane] = sy;
        __syncthreads();
        sx = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        sy = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
        __syncthreads();
        const float rx = sqrtf(sx), ex = rx + 1e-10f, ey = sqrtf(sy) + 1e-10f;
        double vsum = 0.0;
        float s = 0.f;
        if (in)
            for (int c = wave; c < p.C; c += 4) {
                const float u = fx[(size_t)c * p.hw + px], v = fy[(size_t)c * p.hw + px], l = p.lin[c];
                const float d = u / ex - v / ey;
                vsum += (double)(l * d * d);
                s += (2.f * l * d * invHw) * u;
            }
        red[0][wave][lane] = (float)vsum; red[1][wave][lane] = s;
        __syncthreads();
        const float val = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
        s = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
        __syncthreads();
        pixels += (double)val;
        if (dfx && in) {
            // r = 0: every channel of the pixel sits at ReLU's zero; the reference's autograd gives NaN here, this path 0
            const bool zero = !(rx > 0.f);
            const float k = zero ? 0.f : s / rx / ex / ex;
            for (int c = wave; c < p.C; c += 4) {
                const float u = fx[(size_t)c * p.hw + px], v = fy[(size_t)c * p.hw + px], l = p.lin[c];
                float gr = 0.f;
                if (!zero) gr = (2.f * l * (u / ex - v / ey) * invHw) / ex - u * k;
                if (p.relu && !(u > 0.f)) gr = 0.f;
                dfx[(size_t)c * p.hw + px] = gr;
            }
        }
    }
    if (wave == 0) blk[lane] = pixels;
    __syncthreads();
    if (wave != 0) return;
    int last = 0;
    if (lane == 0) {
        double t = 0.0;
        for (int i = 0; i < 64; i++) t += blk[i];
        __hip_atomic_store(p.partial + (size_t)n * p.nb + b, (float)t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = __hip_atomic_fetch_add(p.counter + n, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == p.nb - 1;
    }
    last = __shfl(last, 0);
    if (!last) return;
    double t = 0.0;
    for (int j = lane; j < p.nb; j += 64) t += (double)__hip_atomic_load(p.partial + (size_t)n * p.nb + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int o = 32; o > 0; o >>= 1) t += __shfl_down(t, o);
    if (lane == 0) {
        p.value[n] = (float)(t / (double)p.hw);
        __hip_atomic_store(p.counter + n, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // ready for the next launch
    }
}

static int grid_1d(size_t total, unsigned& blocks) {
    const size_t b = (total + 255) / 256;
    if (b > 0x7fffffffULL) { set_error("lpips: tensor too large"); return SG3_BAD_ARG; }
    blocks = (unsigned)b;
    return SG3_OK;
}

static int prep_params(const sg3_lpips_prepare_params* q, PrepP& p) {
    SG3_REQUIRE(q && q->x && q->canvas, "lpips_prepare: null tensor");
    SG3_REQUIRE(q->N > 0 && q->H >= 7 && q->W >= 7, "lpips_prepare: the image must be at least 7 x 7");
    p.x = q->x; p.canvas = q->canvas; p.scale = q->scale;
    for (int i = 0; i < 4; i++) p.xs[i] = q->xStride[i];
    p.N = q->N; p.H = q->H; p.W = q->W;
    p.PH = (q->H - 7) / 4 + 3; p.PW = (q->W - 7) / 4 + 3;
    for (int i = 0; i < 3; i++) {
        SG3_REQUIRE(q->std[i] != 0.f, "lpips_prepare: std must not be zero");
        p.mean[i] = q->mean[i]; p.std[i] = q->std[i];
    }
    return SG3_OK;
}

} // namespace sg3

extern "C" {

int sg3_lpips_prepare(const sg3_lpips_prepare_params* q, void* stream) {
    using namespace sg3;
    PrepP p;
    int rc = prep_params(q, p);
    if (rc != SG3_OK) return rc;
    unsigned blocks;
    if ((rc = grid_1d((size_t)p.N * 48 * p.PH * p.PW, blocks)) != SG3_OK) return rc;
    hipLaunchKernelGGL(lpips_prepare_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    SG3_LAUNCH_CHECK("lpips_prepare_kernel");
    return SG3_OK;
}

int sg3_lpips_prepare_bwd(const sg3_lpips_prepare_params* q, void* stream) {
    using namespace sg3;
    PrepP p;
    int rc = prep_params(q, p);
    if (rc != SG3_OK) return rc;
    unsigned blocks;
    if ((rc = grid_1d((size_t)p.N * 3 * p.H * p.W, blocks)) != SG3_OK) return rc;
    hipLaunchKernelGGL(lpips_prepare_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    SG3_LAUNCH_CHECK("lpips_prepare_bwd_kernel");
    return SG3_OK;
}

int64_t sg3_conv2d_k5_packed_floats(int O, int I) {
    using namespace sg3;
    if (O <= 0 || I <= 0) return 0;
    return (int64_t)O * ceil_div(I, K5_KC) * K5_TAPS * K5_KC;
}

int sg3_conv2d_k5_pack(const float* w, float* wPacked, int O, int I, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(w && wPacked && O > 0 && I > 0, "conv2d_k5_pack: bad arguments");
    hipLaunchKernelGGL(conv2d_k5_pack_kernel, dim3(O), dim3(256), 0, (hipStream_t)stream, w, wPacked, O, I, ceil_div(I, K5_KC));
    SG3_LAUNCH_CHECK("conv2d_k5_pack_kernel");
    return SG3_OK;
}

int sg3_conv2d_k5(const sg3_conv2d_k5_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->wPacked && p->out, "conv2d_k5: null tensor");
    SG3_REQUIRE(p->N > 0 && p->I > 0 && p->O > 0 && p->H > 0 && p->W > 0, "conv2d_k5: empty tensor");
    // the 4-row tile, unless its grid leaves CUs without a workgroup: then twice the workgroups with 2 rows each
    const long long tiles4 = (long long)p->N * ceil_div(p->O, K5_BM) * ceil_div(p->H, 4) * ceil_div(p->W, 32);
    if (tiles4 < (long long)device_cu_count()) return launch_k5<1>(*p, (hipStream_t)stream);
    return launch_k5<2>(*p, (hipStream_t)stream);
}

int sg3_maxpool3s2(const sg3_maxpool3s2_params* q, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(q && q->x && q->y, "maxpool3s2: null tensor");
    SG3_REQUIRE(q->N > 0 && q->C > 0 && q->H >= 3 && q->W >= 3, "maxpool3s2: the input must be at least 3 x 3");
    PoolP p = {};
    p.x = q->x; p.out = q->y; p.N = q->N; p.C = q->C; p.H = q->H; p.W = q->W; p.OH = (q->H - 3) / 2 + 1; p.OW = (q->W - 3) / 2 + 1;
    unsigned blocks;
    const int rc = grid_1d((size_t)p.N * p.C * p.OH * p.OW, blocks);
    if (rc != SG3_OK) return rc;
    hipLaunchKernelGGL(maxpool3s2_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    SG3_LAUNCH_CHECK("maxpool3s2_kernel");
    return SG3_OK;
}

int sg3_maxpool3s2_bwd(const sg3_maxpool3s2_bwd_params* q, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(q && q->x && q->dy && q->dx, "maxpool3s2_bwd: null tensor");
    SG3_REQUIRE(q->N > 0 && q->C > 0 && q->H >= 3 && q->W >= 3, "maxpool3s2_bwd: the input must be at least 3 x 3");
    PoolP p = {};
    p.x = q->x; p.dy = q->dy; p.addend = q->addend; p.out = q->dx; p.relu = q->reluMask;
    for (int i = 0; i < 4; i++) p.os[i] = q->dxStride[i];
    p.N = q->N; p.C = q->C; p.H = q->H; p.W = q->W; p.OH = (q->H - 3) / 2 + 1; p.OW = (q->W - 3) / 2 + 1;
    unsigned blocks;
    const int rc = grid_1d((size_t)p.N * p.C * p.H * p.W, blocks);
    if (rc != SG3_OK) return rc;
    hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p);
    SG3_LAUNCH_CHECK("maxpool3s2_bwd_kernel");
    return SG3_OK;
}

int sg3_lpips_head_blocks(int h, int w) {
    using namespace sg3;
    if (h <= 0 || w <= 0) return 0;
    return head_blocks((long long)h * w);
}

int sg3_lpips_head(const sg3_lpips_head_params* q, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(q && q->fx && q->fy && q->lin && q->value && q->partial && q->counter, "lpips_head: null tensor");
    SG3_REQUIRE(q->N > 0 && q->C > 0 && q->h > 0 && q->w > 0, "lpips_head: empty tensor");
    SG3_REQUIRE((long long)q->h * q->w < 0x7fffffffLL && (long long)q->C * q->h * q->w < ((long long)1 << 40), "lpips_head: tensor too large");
    HeadP p;
    p.fx = q->fx; p.fy = q->fy; p.lin = q->lin; p.value = q->value; p.dfx = q->dfx; p.partial = q->partial; p.counter = q->counter;
    p.N = q->N; p.C = q->C; p.hw = q->h * q->w; p.relu = q->reluMask;
    p.G = head_groups(p.hw); p.nb = head_blocks(p.hw);
    SG3_REQUIRE((long long)p.N * p.nb < 0x7fffffffLL, "lpips_head: grid too large");
    hipLaunchKernelGGL(lpips_head_kernel, dim3((unsigned)(p.N * p.nb)), dim3(256), 0, (hipStream_t)stream, p);
    SG3_LAUNCH_CHECK("lpips_head_kernel");
    return SG3_OK;
}

} // extern "C"
