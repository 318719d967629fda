// sg3_conv2d_dgrad.hip -- data gradient of the encoder convolutions (sg3_conv2d.hip) as an fp32-exact MFMA implicit GEMM.
//
// Forward:  y[n][o][oy][ox] = sum_{i,ky,kx} w[o][i][ky][kx] x[n][i][oy s - pad + ky][ox s - pad + kx],  k in {1, 3}, s in {1, 2}, pad = k / 2.
// Backward: dx[n][i][y][x]  = sum_{o,ky,kx} w[o][i][ky][kx] dy[n][o][(y + pad - ky) / s][(x + pad - kx) / s]   over the taps that divide.
// With s = 2 a tap reaches pixel (y, x) only when y + pad - ky and x + pad - kx are even, so the pixels of one parity class
// (y & 1, x & 1) all use the same taps: 1, 2, 2 and 4 of the nine for k = 3, one or none for k = 1.  Each class is a dense stride-1
// implicit GEMM over its own taps -- M = input channels, K = output channels x taps of the class, N = pixels of the class -- and a
// workgroup belongs to one class, so no inserted zero is ever multiplied.  Stride 1 is the single class with all taps.
//
// Operand staging follows conv2d_mfma_kernel: weights pre-packed [I][O/KC][tap][KC] (sg3_conv2d_pack of the transposed weight, so
// a per-input-channel scale -- the BatchNorm in front of the convolution -- is the pack's output scale), a dy patch of KC channels
// staged per K chunk in LDS, channel-interleaved by 4, with a one-pixel margin for the tap offsets -1 .. 1; the next chunk is
// fetched global -> registers during the MFMA loop.  v_mfma_f32_32x32x2_f32 throughout: products are exact, which the gradients
// here need (1e-4 .. 1e-9; a split-precision operand would carry an absolute floor near 2^-23).
//
// Epilogue, per written element:  v = acc (+ addend, through element strides);  v *= (act > 0 ? 1 : slope[i])  when `act` is given
// (the derivative of the PReLU whose saved output, or pre-activation, is `act`).  The input size H x W is a parameter: a stride-2
// output size does not determine it.  Every element of dx is written exactly once.
#include "sg3_conv2d_plan.h"

namespace sg3 {

struct DgradParams {
    const float* dy; const float* wp; float* dx; const float* act; const float* slope; const float* addend;
    int64_t addStride[4];
    int N, I, O, H, W, OH, OW, pad;
    int nch, xTiles, yTiles, mTiles, totalBlocks;
};

template <int KS, int STRIDE, int WM, int WN, int TM, int TN>
__global__ void __launch_bounds__(256)
conv2d_dgrad_kernel(DgradParams p) {
    constexpr int TAPS = ConvK<KS>::TAPS, KC = ConvK<KS>::KC;
    constexpr int BM = WM * TM * 32;
    constexpr int ROWS = WN * TN;
    constexpr int PH = ROWS + 2, PW = 34;              // class rows / columns of the tile plus the margin of one
    constexpr int AS = TAPS * KC + 4;
    constexpr int PLANE = PH * PW * 4;
    constexpr int NPL = KC / 4;
    constexpr int A_V4 = BM * TAPS * KC / 4;
    constexpr int A_PER = (A_V4 + 255) / 256;
    constexpr int B_EL = KC * PH * PW;
    constexpr int B_PER = (B_EL + 255) / 256;
    constexpr int SH = STRIDE == 2 ? 1 : 0;
    static_assert(WM * WN == 4, "4 waves per workgroup");

    __shared__ __attribute__((aligned(16))) float smem[BM * AS + NPL * PLANE];
    float* sA = smem;
    float* sB = smem + BM * AS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    int bid = blockIdx.x;
    const int mt = bid % p.mTiles; bid /= p.mTiles;
    const int xt = bid % p.xTiles; bid /= p.xTiles;
    const int yt = bid % p.yTiles; bid /= p.yTiles;
    const int cls = bid % (STRIDE * STRIDE); const int n = bid / (STRIDE * STRIDE);
    const int py = cls / STRIDE, px = cls % STRIDE;            // parity of the pixels this workgroup writes
    const int i0 = mt * BM, x0 = xt * 32, y0 = yt * ROWS;     // tile origin in class coordinates: pixel (y0 * STRIDE + py, x0 * STRIDE + px)
    const float* dyn = p.dy + (size_t)n * p.O * p.OH * p.OW;

    // Four accumulators per tile, one per k lane pair of the fragment (summed in the epilogue): a single accumulator would be a chain
    // of taps x O / 2 dependent additions, whose rounding error grows with its length and is several times that of a library GEMM
    // over O; four chains of a quarter the length also leave the matrix pipe no dependent back-to-back issue.
    f32x16 acc[4][TM][TN];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int a = 0; a < TM; a++)
#pragma unroll
            for (int b = 0; b < TN; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[q][a][b][r] = 0.f;

    // the taps of this class (workgroup-uniform); an empty class (k = 1, stride 2, odd pixels) only runs the epilogue
    bool any = false;
#pragma unroll
    for (int tap = 0; tap < TAPS; tap++)
        any = any || ((((py + p.pad - tap / KS) | (px + p.pad - tap % KS)) & (STRIDE - 1)) == 0);

    f32x4 ra[A_PER];
    float rb[B_PER];

    auto fetch = [&](int ch) {
#pragma unroll
        for (int q = 0; q < A_PER; q++) {
            const int v = tid + 256 * q;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (A_V4 % 256 == 0 || v < A_V4) {
                const int row = v / (TAPS * KC / 4), col = v % (TAPS * KC / 4);
                if (i0 + row < p.I)
                    val = *reinterpret_cast<const f32x4*>(p.wp + ((size_t)(i0 + row) * p.nch + ch) * (TAPS * KC) + col * 4);
            }
            ra[q] = val;
        }
#pragma unroll
        for (int q = 0; q < B_PER; q++) {
            const int e = tid + 256 * q;
            float val = 0.f;
            if (B_EL % 256 == 0 || e < B_EL) {
                const int ex = e % PW, t = e / PW, ey = t % PH, c = t / PH;
                const int oc = ch * KC + c, gy = y0 - 1 + ey, gx = x0 - 1 + ex;
                if (oc < p.O && (unsigned)gy < (unsigned)p.OH && (unsigned)gx < (unsigned)p.OW)
                    val = dyn[((size_t)oc * p.OH + gy) * p.OW + gx];
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
                const int ex = e % PW, t = e / PW, ey = t % PH, c = t / PH;
                sB[(c >> 2) * PLANE + (ey * PW + ex) * 4 + (c & 3)] = rb[q];
            }
        }
    };

    if (any) {
        fetch(0);
        for (int ch = 0; ch < p.nch; ch++) {
            __syncthreads();
            stage();
            __syncthreads();
            if (ch + 1 < p.nch) fetch(ch + 1);
#pragma unroll
            for (int tap = 0; tap < TAPS; tap++) {
                const int ty = py + p.pad - tap / KS, tx = px + p.pad - tap % KS;      // dy row = class row + ty / STRIDE
                if (((ty | tx) & (STRIDE - 1)) != 0) continue;                           // workgroup-uniform
                const int oy = (ty >> SH) + 1, ox = (tx >> SH) + 1;                      // 0 .. 2 inside the patch margin
#pragma unroll
                for (int c8 = 0; c8 < KC / 8; c8++) {
                    f32x4 fa[TM], fb[TN];
#pragma unroll
                    for (int a = 0; a < TM; a++)
                        fa[a] = *reinterpret_cast<const f32x4*>(sA + ((wm * TM + a) * 32 + li) * AS + tap * KC + c8 * 8 + 4 * lh);
#pragma unroll
                    for (int b = 0; b < TN; b++)
                        fb[b] = *reinterpret_cast<const f32x4*>(sB + (2 * c8 + lh) * PLANE + ((wn * TN + b + oy) * PW + li + ox) * 4);
#pragma unroll
                    for (int q = 0; q < 4; q++)
#pragma unroll
                        for (int a = 0; a < TM; a++)
#pragma unroll
                            for (int b = 0; b < TN; b++)
                                acc[q][a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[a][q], fb[b][q], acc[q][a][b], 0, 0, 0);
                }
            }
        }
    }

    const int gx = (x0 + li) * STRIDE + px;
#pragma unroll
    for (int a = 0; a < TM; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = i0 + (wm * TM + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (i >= p.I) continue;
            const float sl = p.act ? p.slope[i] : 1.f;
#pragma unroll
            for (int b = 0; b < TN; b++) {
                const int gy = (y0 + wn * TN + b) * STRIDE + py;
                if (gy < p.H && gx < p.W) {
                    const size_t at = (((size_t)n * p.I + i) * p.H + gy) * p.W + gx;
                    float v = (acc[0][a][b][r] + acc[1][a][b][r]) + (acc[2][a][b][r] + acc[3][a][b][r]);
                    if (p.addend) v += p.addend[(int64_t)n * p.addStride[0] + (int64_t)i * p.addStride[1] + (int64_t)gy * p.addStride[2] + (int64_t)gx * p.addStride[3]];
                    if (p.act) v = p.act[at] > 0.f ? v : v * sl;
                    p.dx[at] = v;
                }
            }
        }
}

template <int KS, int STRIDE, int WM, int WN, int TM, int TN>
static int launch_dgrad(const sg3_conv2d_dgrad_params& q, const Conv2dPlan& pl, hipStream_t st) {
    DgradParams p;
    p.dy = q.dy; p.wp = q.wPacked; p.dx = q.dx; p.act = q.act; p.slope = q.slope; p.addend = q.addend;
    for (int d = 0; d < 4; d++) p.addStride[d] = q.addStride[d];
    p.N = q.N; p.I = q.I; p.O = q.O; p.H = q.H; p.W = q.W; p.OH = q.OH; p.OW = q.OW; p.pad = KS / 2;
    p.nch = pl.nch; p.xTiles = pl.xTiles; p.yTiles = pl.yTiles; p.mTiles = pl.mTiles; p.totalBlocks = pl.totalBlocks;
    hipLaunchKernelGGL((conv2d_dgrad_kernel<KS, STRIDE, WM, WN, TM, TN>), dim3((unsigned)pl.totalBlocks), dim3(pl.block), 0, st, p);
    SG3_LAUNCH_CHECK("conv2d_dgrad_kernel");
    return SG3_OK;
}

// plan coordinates -> template instantiation: the two tiles per (KS, STRIDE)
template <int KS, int STRIDE>
static int launch_tile(const sg3_conv2d_dgrad_params& q, const Conv2dPlan& pl, hipStream_t st) {
    return pl.WM == 2 ? launch_dgrad<KS, STRIDE, 2, 2, 1, 1>(q, pl, st) : launch_dgrad<KS, STRIDE, 1, 4, 1, 1>(q, pl, st);
}

} // namespace sg3

extern "C" {

// the checks and the plan of the launch
int sg3_conv2d_dgrad_dispatch(const sg3_conv2d_dgrad_params* p, sg3_conv2d_dispatch_info* out) {
    using namespace sg3;
    SG3_REQUIRE(out, "conv2d_dgrad_dispatch: null argument");
    SG3_REQUIRE(p && p->dy && p->wPacked && p->dx, "conv2d_dgrad: null tensor");
    SG3_REQUIRE(p->N > 0 && p->I > 0 && p->O > 0 && p->H > 0 && p->W > 0, "conv2d_dgrad: empty tensor");
    SG3_REQUIRE(p->k == 1 || p->k == 3, "conv2d_dgrad: kernel size must be 1 or 3");
    SG3_REQUIRE(p->stride == 1 || p->stride == 2, "conv2d_dgrad: stride must be 1 or 2");
    SG3_REQUIRE(p->OH == (p->H + 2 * (p->k / 2) - p->k) / p->stride + 1 && p->OW == (p->W + 2 * (p->k / 2) - p->k) / p->stride + 1,
                "conv2d_dgrad: dy is %d x %d, but a %d x %d input with k %d, stride %d, padding k / 2 gives another size", p->OH, p->OW, p->H, p->W, p->k, p->stride);
    SG3_REQUIRE(!p->act || p->slope, "conv2d_dgrad: slope missing");
    SG3_REQUIRE((long long)p->N * p->I * p->H * p->W < 0x7fffffffLL && (long long)p->N * p->O * p->OH * p->OW < 0x7fffffffLL, "conv2d_dgrad: tensor too large");
    *out = plan_conv2d_dgrad(*p);
    SG3_REQUIRE(out->totalBlocks > 0, "conv2d_dgrad: grid too large");
    return SG3_OK;
}

int sg3_conv2d_dgrad(const sg3_conv2d_dgrad_params* p, void* stream) {
    using namespace sg3;
    Conv2dPlan pl;
    const int rc = sg3_conv2d_dgrad_dispatch(p, &pl);
    if (rc != SG3_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (p->k == 3) return p->stride == 1 ? launch_tile<3, 1>(*p, pl, st) : launch_tile<3, 2>(*p, pl, st);
    return p->stride == 1 ? launch_tile<1, 1>(*p, pl, st) : launch_tile<1, 2>(*p, pl, st);
}

} // extern "C"
