// sg3_se_bwd.hip -- backward of the squeeze-and-excitation tail of an IR-SE residual unit (sg3_se.hip), two launches like the forward.
//
// Forward:  m = mean_hw(res),  u = fc1 m,  h = relu(u),  z = fc2 h,  g = sigmoid(z),  out = shortcut + res * g.
// Backward, from dout and the saved res and m:
//     dg = sum_hw dout * res            se_dot_kernel, one wave per (n, c) plane
//     dz = dg g (1 - g),  dh = fc2^T dz,  du = dh [u > 0],  dm = fc1^T du
//     dres = dout g + dm / (H W)        se_bwd_apply_kernel: every workgroup recomputes the gate chain of its sample (three
//     dshortcut = dout                  C x C/16 products) and streams its 8 channels
// dshortcut is dout itself and is not written, except for the identity shortcut of a stride-2 unit (MaxPool2d(1, 2): the shortcut
// is x[:, :, ::2, ::2]), whose input gradient is dout at the even positions and zero elsewhere: `dscatter` [N][C][inH][inW].
#include "sg3_common.h"
#include <cmath>

namespace sg3 {

__global__ void __launch_bounds__(256)
se_dot_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ dot, int planes, int hw) {
    const int lane = threadIdx.x & 63;
    const int pl = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pl >= planes) return;
    const float* pa = a + (size_t)pl * hw;
    const float* pb = b + (size_t)pl * hw;
    float s = 0.f;
    for (int i = lane; i < hw; i += 64) s = __builtin_fmaf(pa[i], pb[i], s);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) dot[pl] = s;
}

constexpr int SEB_CG = 8;           // channels per workgroup of the apply kernel
constexpr int SEB_MAXC = 2048, SEB_MAXR = 128;

__global__ void __launch_bounds__(256)
se_bwd_apply_kernel(sg3_se_bwd_params p, int chunks, int rowsPer) {
    __shared__ float su[SEB_MAXR], sdu[SEB_MAXR];
    __shared__ float sdz[SEB_MAXC];
    __shared__ float sgate[SEB_CG], sdm[SEB_CG];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int bid = blockIdx.x;
    const int chunk = bid % chunks; bid /= chunks;
    const int groups = (p.C + SEB_CG - 1) / SEB_CG;
    const int cg = bid % groups, n = bid / groups;
    const float* mean = p.mean + (size_t)n * p.C;
    const float* dg = p.dg + (size_t)n * p.C;
    for (int r = wave; r < p.R; r += 4) {                                   // u = fc1 m
        const float* w = p.fc1 + (size_t)r * p.C;
        float s = 0.f;
        for (int i = lane; i < p.C; i += 64) s = __builtin_fmaf(w[i], mean[i], s);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) su[r] = s;
    }
    __syncthreads();
    for (int c = tid; c < p.C; c += 256) {                                  // g = sigmoid(fc2 relu(u)),  dz = dg g (1 - g)
        const float* w = p.fc2 + (size_t)c * p.R;
        float s = 0.f;
        for (int r = 0; r < p.R; r++) s = __builtin_fmaf(w[r], fmaxf(su[r], 0.f), s);
        const float g = 1.f / (1.f + expf(-s));
        sdz[c] = dg[c] * g * (1.f - g);
        if (c >= cg * SEB_CG && c < cg * SEB_CG + SEB_CG) sgate[c - cg * SEB_CG] = g;
    }
    __syncthreads();
    for (int r = wave; r < p.R; r += 4) {                                   // du = (fc2^T dz) [u > 0]
        float s = 0.f;
        for (int c = lane; c < p.C; c += 64) s = __builtin_fmaf(p.fc2[(size_t)c * p.R + r], sdz[c], s);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
        if (lane == 0) sdu[r] = su[r] > 0.f ? s : 0.f;
    }
    __syncthreads();
    if (tid < SEB_CG) {                                                     // dm = fc1^T du, for this workgroup's channels
        const int c = cg * SEB_CG + tid;
        float s = 0.f;
        if (c < p.C)
            for (int r = 0; r < p.R; r++) s = __builtin_fmaf(p.fc1[(size_t)r * p.C + c], sdu[r], s);
        sdm[tid] = s / (float)(p.H * p.W);
    }
    __syncthreads();
    const int hw = p.H * p.W;
    const int y0 = chunk * rowsPer, y1 = min(p.H, y0 + rowsPer);          // whole rows, so that a chunk's scatter owns whole input rows
    const int i0 = y0 * p.W, i1 = y1 * p.W;
    for (int k = 0; k < SEB_CG; k++) {
        const int c = cg * SEB_CG + k;
        if (c >= p.C) break;
        const float g = sgate[k], dm = sdm[k];
        const float* dout = p.dout + ((size_t)n * p.C + c) * hw;
        float* dres = p.dres + ((size_t)n * p.C + c) * hw;
        for (int i = i0 + tid; i < i1; i += 256) dres[i] = __builtin_fmaf(dout[i], g, dm);
        if (p.dscatter) {
            // rows [2 y0, 2 y1) of the input-sized plane; the last chunk also takes the odd last row of an even-sized input
            float* ds = p.dscatter + ((size_t)n * p.C + c) * p.inH * p.inW;
            const int r0 = 2 * y0, r1 = y1 == p.H ? p.inH : 2 * y1;
            for (int e = r0 * p.inW + tid; e < r1 * p.inW; e += 256) {
                const int y = e / p.inW, x = e - y * p.inW;
                ds[e] = ((y | x) & 1) ? 0.f : dout[(y >> 1) * p.W + (x >> 1)];
            }
        }
    }
}

} // namespace sg3

extern "C" int sg3_se_residual_bwd(const sg3_se_bwd_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->dout && p->res && p->mean && p->fc1 && p->fc2 && p->dg && p->dres, "se_residual_bwd: null tensor");
    SG3_REQUIRE(p->N > 0 && p->C > 0 && p->H > 0 && p->W > 0 && p->R > 0, "se_residual_bwd: empty tensor");
    SG3_REQUIRE(p->C <= SEB_MAXC && p->R <= SEB_MAXR, "se_residual_bwd: at most 2048 channels and 128 hidden units");
    SG3_REQUIRE((long long)p->N * p->C * p->H * p->W < 0x7fffffffLL, "se_residual_bwd: tensor too large");
    if (p->dscatter) {
        SG3_REQUIRE(p->H == (p->inH + 1) / 2 && p->W == (p->inW + 1) / 2, "se_residual_bwd: dscatter is %d x %d, not the stride-2 source of %d x %d", p->inH, p->inW, p->H, p->W);
        SG3_REQUIRE((long long)p->N * p->C * p->inH * p->inW < 0x7fffffffLL, "se_residual_bwd: tensor too large");
    }
    hipStream_t st = (hipStream_t)stream;
    const int planes = p->N * p->C, hw = p->H * p->W;
    hipLaunchKernelGGL(se_dot_kernel, dim3((unsigned)ceil_div(planes, 4)), dim3(256), 0, st, p->dout, p->res, p->dg, planes, hw);
    SG3_LAUNCH_CHECK("se_dot_kernel");
    // chunks cover whole rows, so that the scatter of a chunk owns whole rows of the input-sized plane
    int chunks = std::max(1, std::min(64, ceil_div(hw, 4096)));
    chunks = std::min(chunks, p->H);
    const int rowsPer = ceil_div(p->H, chunks);
    chunks = ceil_div(p->H, rowsPer);
    const long long blocks = (long long)p->N * ceil_div(p->C, SEB_CG) * chunks;
    hipLaunchKernelGGL(se_bwd_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, st, *p, chunks, rowsPer);
    SG3_LAUNCH_CHECK("se_bwd_apply_kernel");
    return SG3_OK;
}
