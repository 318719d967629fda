// sg3_conv2d_wgrad_sum.hip -- weight gradient of the encoder convolutions (sg3_conv2d.hip), summed over the batch, as an fp32-exact
// MFMA implicit GEMM.  This is what training the encoder trunk adds to the data gradient of sg3_conv2d_dgrad.hip.
//
//     dW[o][i][ky][kx] = sum_{n,oy,ox} dy[n][o][oy][ox] * xt[n][i][oy s + ky - pad][ox s + kx - pad],   k in {1, 3}, s in {1, 2}, pad = k / 2
//     xt = inScale[i] x + inShift[i] on real pixels (one fmaf), 0 in the padding: the train-mode BatchNorm in front of a unit's first
//     convolution is applied while the patch is staged, the normalised tensor never exists in memory.
//
// GEMM view: M = output channels (A = dy, rows), N = input channels (B = xt, columns), K = pixels of all samples.  One K chunk is one
// segment of P = 32 / s output pixels of one output row of one sample; the dy segment [64 o][P] and the input patch [64 i][k rows][(P - 1) s + k]
// it touches are staged in LDS, and every A fragment is used for all k x k taps (one accumulator tile per tap), so dy is read once.
// A workgroup owns a 64 x 64 (o, i) tile, four waves of 32 x 32, and a contiguous range of chunks; the next chunk is fetched
// global -> registers during the MFMA loop.  v_mfma_f32_32x32x2_f32 throughout: products are exact and every accumulator is one
// fmaf chain in chunk order, so |error| <= (chain + splits) 2^-24 (|dy| * |xt|) -- gradients here span 1e-2 .. 1e-9 and a
// split-precision operand would put an absolute floor under them.
//
// K is split over nSplit workgroup sets (sg3_conv2d_wgrad_sum_splits: host only, the same for every device so that results do not
// depend on the machine); each set writes its own partial [O][I][k][k] and a second small launch adds the partials in split order.
// No atomics anywhere: bit-identical on repeat.
#include "sg3_conv2d_plan.h"

namespace sg3 {

struct WgradSumParams {
    const float* x; const float* dy; float* out; const float* inScale; const float* inShift;
    int N, I, O, H, W, OH, OW, pad;
    int xSegs, nChunks, chunksPerSplit, oTiles, iTiles;
};

template <int KS, int STRIDE>
__global__ void __launch_bounds__(256)
conv2d_wgrad_sum_kernel(WgradSumParams p) {
    constexpr int TAPS = KS * KS, WS_PX = ws_px(STRIDE);
    constexpr int AS = WS_PX + 4;                              // dy row pitch: 16-byte rows, shifted banks
    constexpr int XW = (WS_PX - 1) * STRIDE + KS;              // input columns one segment touches
    constexpr int XWP = XW | 1;                                // odd pitch, and KS is odd: 32 channels on 32 banks
    constexpr int A_EL = WS_TILE * WS_PX, A_PER = A_EL / 256;
    constexpr int B_EL = WS_TILE * KS * XW, B_PER = (B_EL + 255) / 256;

    __shared__ __attribute__((aligned(16))) float sA[WS_TILE * AS];
    __shared__ float sB[WS_TILE * KS * XWP];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;

    int bid = blockIdx.x;
    const int it = bid % p.iTiles; bid /= p.iTiles;
    const int ot = bid % p.oTiles; const int split = bid / p.oTiles;
    const int o0 = ot * WS_TILE, i0 = it * WS_TILE;
    const int c0 = split * p.chunksPerSplit;
    const int c1 = min(c0 + p.chunksPerSplit, p.nChunks);

    f32x16 acc[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[t][r] = 0.f;

    float ra[A_PER], rb[B_PER];

    auto fetch = [&](int chunk) {
        const int xs = chunk % p.xSegs; const int t = chunk / p.xSegs;
        const int oy = t % p.OH, n = t / p.OH;
        const int x0 = xs * WS_PX;
#pragma unroll
        for (int q = 0; q < A_PER; q++) {
            const int e = tid + 256 * q;
            const int px = e % WS_PX, o = o0 + e / WS_PX;
            float v = 0.f;
            if (o < p.O && x0 + px < p.OW) v = p.dy[(((size_t)n * p.O + o) * p.OH + oy) * p.OW + x0 + px];
            ra[q] = v;
        }
#pragma unroll
        for (int q = 0; q < B_PER; q++) {
            const int e = tid + 256 * q;
            float v = 0.f;
            if (B_EL % 256 == 0 || e < B_EL) {
                const int ex = e % XW, u = e / XW, ey = u % KS, c = i0 + u / KS;
                const int gy = oy * STRIDE - p.pad + ey, gx = x0 * STRIDE - p.pad + ex;
                if (c < p.I && (unsigned)gy < (unsigned)p.H && (unsigned)gx < (unsigned)p.W) {
                    v = p.x[(((size_t)n * p.I + c) * p.H + gy) * p.W + gx];
                    if (p.inScale) v = fmaf(p.inScale[c], v, p.inShift[c]);
                }
            }
            rb[q] = v;
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int q = 0; q < A_PER; q++) {
            const int e = tid + 256 * q;
            sA[(e / WS_PX) * AS + e % WS_PX] = ra[q];
        }
#pragma unroll
        for (int q = 0; q < B_PER; q++) {
            const int e = tid + 256 * q;
            if (B_EL % 256 == 0 || e < B_EL) sB[(e / XW) * XWP + e % XW] = rb[q];
        }
    };

    if (c0 < c1) fetch(c0);
    for (int chunk = c0; chunk < c1; chunk++) {
        __syncthreads();
        stage();
        __syncthreads();
        if (chunk + 1 < c1) fetch(chunk + 1);
        const float* bRow = sB + (wn * 32 + li) * KS * XWP;
#pragma unroll
        for (int c8 = 0; c8 < WS_PX / 8; c8++) {
            // lane half lh holds pixel c8 * 8 + 4 lh + q of the chunk in MFMA q: k = lh
            const f32x4 fa = *reinterpret_cast<const f32x4*>(sA + (wm * 32 + li) * AS + c8 * 8 + 4 * lh);
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int tap = 0; tap < TAPS; tap++) {
                    const float b = bRow[(tap / KS) * XWP + (c8 * 8 + 4 * lh + q) * STRIDE + tap % KS];
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q], b, acc[tap], 0, 0, 0);
                }
        }
    }

    float* out = p.out + (size_t)split * p.O * p.I * TAPS;
    const int i = i0 + wn * 32 + li;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int o = o0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (o < p.O && i < p.I) {
#pragma unroll
            for (int tap = 0; tap < TAPS; tap++) out[((size_t)o * p.I + i) * TAPS + tap] = acc[tap][r];
        }
    }
}

// dw[e] = partial[0][e] + partial[1][e] + ... in split order
__global__ void __launch_bounds__(256)
conv2d_wgrad_sum_reduce_kernel(const float* partial, float* dw, int total, int nSplit) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    float s = partial[e];
    for (int j = 1; j < nSplit; j++) s += partial[(size_t)j * total + e];
    dw[e] = s;
}

template <int KS, int STRIDE>
static int launch_wgrad_sum(const sg3_conv2d_wgrad_sum_params& q, const Conv2dPlan& pl, hipStream_t st) {
    WgradSumParams p;
    p.x = q.x; p.dy = q.dy; p.inScale = q.inScale; p.inShift = q.inShift;
    p.out = pl.nSplit > 1 ? q.partial : q.dw;
    p.N = q.N; p.I = q.I; p.O = q.O; p.H = q.H; p.W = q.W; p.OH = pl.outH; p.OW = pl.outW; p.pad = KS / 2;
    p.xSegs = pl.xSegs; p.nChunks = pl.nChunks; p.chunksPerSplit = pl.chunksPerSplit; p.oTiles = pl.oTiles; p.iTiles = pl.iTiles;
    hipLaunchKernelGGL((conv2d_wgrad_sum_kernel<KS, STRIDE>), dim3((unsigned)pl.totalBlocks), dim3(pl.block), 0, st, p);
    SG3_LAUNCH_CHECK("conv2d_wgrad_sum_kernel");
    if (pl.nSplit > 1) {
        hipLaunchKernelGGL(conv2d_wgrad_sum_reduce_kernel, dim3((unsigned)pl.reduceGrid), dim3(256), 0, st, q.partial, q.dw, q.O * q.I * KS * KS, pl.nSplit);
        SG3_LAUNCH_CHECK("conv2d_wgrad_sum_reduce_kernel");
    }
    return SG3_OK;
}

} // namespace sg3

extern "C" {

// the checks and the plan of the launch
int sg3_conv2d_wgrad_sum_dispatch(const sg3_conv2d_wgrad_sum_params* p, sg3_conv2d_dispatch_info* out) {
    using namespace sg3;
    SG3_REQUIRE(out, "conv2d_wgrad_sum_dispatch: null argument");
    SG3_REQUIRE(p && p->x && p->dy && p->dw, "conv2d_wgrad_sum: null tensor");
    SG3_REQUIRE(p->N > 0 && p->I > 0 && p->O > 0 && p->H > 0 && p->W > 0, "conv2d_wgrad_sum: empty tensor");
    SG3_REQUIRE(p->k == 1 || p->k == 3, "conv2d_wgrad_sum: kernel size must be 1 or 3");
    SG3_REQUIRE(p->stride == 1 || p->stride == 2, "conv2d_wgrad_sum: stride must be 1 or 2");
    SG3_REQUIRE((p->inScale == nullptr) == (p->inShift == nullptr), "conv2d_wgrad_sum: inScale and inShift come together");
    *out = plan_conv2d_wgrad_sum(*p);
    SG3_REQUIRE(out->nChunks > 0, "conv2d_wgrad_sum: too many pixels");
    SG3_REQUIRE(out->nSplit == 1 || p->partial, "conv2d_wgrad_sum: %d splits need the partial scratch", out->nSplit);
    SG3_REQUIRE((long long)p->N * p->I * p->H * p->W < 0x7fffffffLL && (long long)p->N * p->O * out->outH * out->outW < 0x7fffffffLL &&
                (long long)out->nSplit * p->O * p->I * p->k * p->k < 0x7fffffffLL, "conv2d_wgrad_sum: tensor too large");
    SG3_REQUIRE(out->totalBlocks > 0, "conv2d_wgrad_sum: grid too large");
    return SG3_OK;
}

int sg3_conv2d_wgrad_sum_splits(int N, int I, int O, int H, int W, int k, int stride, int* nSplit, int* chunksPerSplit, int* xSegs) {
    float* const set = reinterpret_cast<float*>(16);          // the checks read pointers for presence only
    sg3_conv2d_wgrad_sum_params q = {set, set, nullptr, nullptr, set, set, N, I, O, H, W, k, stride};
    sg3::Conv2dPlan pl;
    const int rc = sg3_conv2d_wgrad_sum_dispatch(&q, &pl);
    if (rc != SG3_OK) return rc;
    if (nSplit) *nSplit = pl.nSplit;
    if (chunksPerSplit) *chunksPerSplit = pl.chunksPerSplit;
    if (xSegs) *xSegs = pl.xSegs;
    return SG3_OK;
}

int sg3_conv2d_wgrad_sum(const sg3_conv2d_wgrad_sum_params* p, void* stream) {
    using namespace sg3;
    Conv2dPlan pl;
    const int rc = sg3_conv2d_wgrad_sum_dispatch(p, &pl);
    if (rc != SG3_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->k == 3) return p->stride == 1 ? launch_wgrad_sum<3, 1>(*p, pl, st) : launch_wgrad_sum<3, 2>(*p, pl, st);
    return p->stride == 1 ? launch_wgrad_sum<1, 1>(*p, pl, st) : launch_wgrad_sum<1, 2>(*p, pl, st);
}

} // extern "C"
