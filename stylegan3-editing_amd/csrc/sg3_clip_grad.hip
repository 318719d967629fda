// sg3_clip_grad.hip -- backward of CLIP's ViT image tower with respect to its input, beside the data-gradient epilogues of the GEMM
// in sg3_clip.hip: LayerNorm backward, attention backward and the per-sample power-of-two scale of the incoming gradient.
// Weights are frozen: nothing here produces a weight gradient.  No atomics and a fixed summation order everywhere, so a sample's
// gradient is bit-identical whatever batch it is in.
#include "sg3_common.h"
#include <math.h>

namespace sg3 {

static constexpr int kMaxL = 128;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm backward: one wave per row.  The statistics are the forward's (pivot = the row's first element, two passes), then
// with g = gamma dy and xhat = (d - mean d) rstd:  dx = rstd (g - mean(g) - xhat mean(g xhat)).  Every element of dy and dx is
// read and written by the same lane, so dx may be dy (ln_pre, in place on the gradient stream).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
clip_layernorm_bwd_kernel(sg3_clip_layernorm_bwd_params p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float* x = p.x + row * p.xRowStride;
    const float* dy = p.dy + row * p.dyRowStride;
    float* dx = p.dx + row * p.dxRowStride;
    const float n = (float)p.D;
    const float pivot = x[0];
    float s = 0.0f;
    for (int d = lane; d < p.D; d += 64) s += x[d] - pivot;
    const float md = wave_sum(s) / n;
    float q = 0.0f;
    for (int d = lane; d < p.D; d += 64) { const float t = (x[d] - pivot) - md; q += t * t; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / n + p.eps);
    float sg = 0.0f, sgx = 0.0f;
    for (int d = lane; d < p.D; d += 64) {
        const float g = p.gamma[d] * dy[d];
        sg += g;
        sgx += g * (((x[d] - pivot) - md) * rstd);
    }
    const float mg = wave_sum(sg) / n, mgx = wave_sum(sgx) / n;
    for (int d = lane; d < p.D; d += 64) {
        const float xhat = ((x[d] - pivot) - md) * rstd;
        const float v = rstd * ((p.gamma[d] * dy[d] - mg) - xhat * mgx);
        dx[d] = p.accumulate ? dx[d] + v : v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention backward: one workgroup per (sample, head), head dimension 64, L <= 128, non-causal.  Two sweeps over the same two
// LDS matrices (rows 66 halfs apart, as the forward keeps K):
//   sweep 1 holds K and V.  A wave takes query i: lane j recomputes the score s_ij (the forward's sum, in its order) and
//     dP_ij = dO_i . V_j, the wave takes the row's max, 1 / sum and delta_i = sum_j P_ij dP_ij, then dS_ij = P_ij (dP_ij - delta_i)
//     and lane d sums dQ_i[d] = sum_j dS_ij K_j[d] / 8 in ascending j.  max, 1 / sum and delta of every row stay in LDS.
//   sweep 2 holds Q and dO.  A wave takes key j: lane i recomputes s_ij (the same products in the same order, so the same
//     bits), P_ij and dS_ij from the saved row statistics, then lane d sums dV_j[d] = sum_i P_ij dO_i[d] and
//     dK_j[d] = sum_i dS_ij Q_i[d] / 8 in ascending i.
// The column sums dK and dV are made by recomputing the L x L matrices transposed, not by atomics and not by keeping two
// 128 x 128 float matrices in LDS: 34 KB of LDS per workgroup, four workgroups on a CU.
// ---------------------------------------------------------------------------------------------------------------------------
static constexpr int KP = 66;

__device__ __forceinline__ float dot64(const float* a, const _Float16* row) {
    float acc = 0.0f;
#pragma unroll 8
    for (int d = 0; d < 64; d += 2) {
        const uint32_t kk = *(const uint32_t*)&row[d];
        const _Float16* k2 = (const _Float16*)&kk;
        acc += a[d] * (float)k2[0];
        acc += a[d + 1] * (float)k2[1];
    }
    return acc;
}

__global__ void __launch_bounds__(256)
clip_attention_bwd_kernel(sg3_clip_attention_bwd_params p) {
    __shared__ __attribute__((aligned(16))) _Float16 sA[kMaxL * KP];      // K, then Q
    __shared__ __attribute__((aligned(16))) _Float16 sB[kMaxL * KP];      // V, then dO
    __shared__ float sR0[4][64];                                           // the wave's own row: q_i, then k_j
    __shared__ float sR1[4][64];                                           // dO_i, then v_j
    __shared__ float sP[4][kMaxL];
    __shared__ float sDS[4][kMaxL];
    __shared__ float sMax[kMaxL], sInv[kMaxL], sDelta[kMaxL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
    const int D = p.heads * 64, L = p.L;
    const _Float16* qkv = (const _Float16*)p.qkv + (int64_t)b * L * 3 * D + h * 64;
    const _Float16* dout = (const _Float16*)p.dout + (int64_t)b * L * D + h * 64;
    _Float16* dqkv = (_Float16*)p.dqkv + (int64_t)b * L * 3 * D + h * 64;

    for (int e = tid; e < L * 32; e += 256) {
        const int j = e >> 5, d2 = (e & 31) * 2;
        const _Float16* row = qkv + (int64_t)j * 3 * D;
        *(uint32_t*)&sA[j * KP + d2] = *(const uint32_t*)(row + D + d2);
        *(uint32_t*)&sB[j * KP + d2] = *(const uint32_t*)(row + 2 * D + d2);
    }
    __syncthreads();
    for (int i0 = 0; i0 < L; i0 += 4) {                         // every wave makes every trip (the barriers): a wave past the end redoes row L - 1
        const int i = min(i0 + wave, L - 1);
        sR0[wave][lane] = (float)qkv[(int64_t)i * 3 * D + lane];
        sR1[wave][lane] = (float)dout[(int64_t)i * D + lane];
        __syncthreads();
        float s[2], dp[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int j = lane + t * 64;
            s[t] = -INFINITY; dp[t] = 0.0f;
            if (j < L) {
                s[t] = dot64(sR0[wave], &sA[j * KP]) * 0.125f;
                dp[t] = dot64(sR1[wave], &sB[j * KP]);
            }
        }
        const float mx = wave_max(fmaxf(s[0], s[1]));
        const float e0 = lane < L ? expf(s[0] - mx) : 0.0f;
        const float e1 = lane + 64 < L ? expf(s[1] - mx) : 0.0f;
        const float inv = 1.0f / wave_sum(e0 + e1);
        const float p0 = e0 * inv, p1 = e1 * inv;
        const float delta = wave_sum(p0 * dp[0] + p1 * dp[1]);
        sDS[wave][lane] = p0 * (dp[0] - delta);
        sDS[wave][lane + 64] = p1 * (dp[1] - delta);
        if (lane == 0) { sMax[i] = mx; sInv[i] = inv; sDelta[i] = delta; }    // a wave redoing row L - 1 writes the same values
        __syncthreads();
        float dq = 0.0f;
        for (int j = 0; j < L; j++) dq += sDS[wave][j] * (float)sA[j * KP + lane];
        if (i0 + wave < L) dqkv[(int64_t)i * 3 * D + lane] = (_Float16)(dq * 0.125f);
        __syncthreads();
    }
    for (int e = tid; e < L * 32; e += 256) {
        const int j = e >> 5, d2 = (e & 31) * 2;
        *(uint32_t*)&sA[j * KP + d2] = *(const uint32_t*)(qkv + (int64_t)j * 3 * D + d2);
        *(uint32_t*)&sB[j * KP + d2] = *(const uint32_t*)(dout + (int64_t)j * D + d2);
    }
    __syncthreads();
    for (int j0 = 0; j0 < L; j0 += 4) {
        const int j = min(j0 + wave, L - 1);
        sR0[wave][lane] = (float)qkv[(int64_t)j * 3 * D + D + lane];
        sR1[wave][lane] = (float)qkv[(int64_t)j * 3 * D + 2 * D + lane];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int i = lane + t * 64;
            float pr = 0.0f, ds = 0.0f;
            if (i < L) {
                // q_i[d] * k_j[d] summed as in sweep 1: the product commutes, the order of the sum is the same
                const float sc = dot64(sR0[wave], &sA[i * KP]) * 0.125f;
                pr = expf(sc - sMax[i]) * sInv[i];
                ds = pr * (dot64(sR1[wave], &sB[i * KP]) - sDelta[i]);
            }
            sP[wave][i] = pr;
            sDS[wave][i] = ds;
        }
        __syncthreads();
        float dv = 0.0f, dk = 0.0f;
        for (int i = 0; i < L; i++) {
            dv += sP[wave][i] * (float)sB[i * KP + lane];
            dk += sDS[wave][i] * (float)sA[i * KP + lane];
        }
        if (j0 + wave < L) {
            dqkv[(int64_t)j * 3 * D + D + lane] = (_Float16)(dk * 0.125f);
            dqkv[(int64_t)j * 3 * D + 2 * D + lane] = (_Float16)dv;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Gradient scale: one workgroup per sample.  max|g| = m 2^e with 0.5 <= m < 1 gives scale 2^(4 - e): the largest scaled entry is
// in [8, 16), 2^12 below float16's overflow (the gradient grows through the blocks) and 2^17 above its smallest normal.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
clip_grad_scale_kernel(sg3_clip_grad_scale_params p) {
    __shared__ float sMaxW[4];
    const int tid = threadIdx.x, b = blockIdx.x;
    const float* g = p.g + (int64_t)b * p.E;
    float m = 0.0f;
    bool bad = false;
    for (int e = tid; e < p.E; e += 256) { const float v = fabsf(g[e]); bad |= !(v <= 3.0e38f); m = fmaxf(m, v); }
    m = wave_max(bad ? INFINITY : m);
    if ((tid & 63) == 0) sMaxW[tid >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(sMaxW[0], sMaxW[1]), fmaxf(sMaxW[2], sMaxW[3]));
    float scale = 1.0f;
    if (m > 0.0f && m <= 3.0e38f) {
        int e;
        frexpf(m, &e);
        scale = ldexpf(1.0f, min(max(4 - e, -100), 100));
    }
    _Float16* o = (_Float16*)p.out16 + (int64_t)b * p.E;
    for (int e = tid; e < p.E; e += 256) o[e] = (_Float16)(g[e] * scale);
    if (tid == 0) p.inv[b] = 1.0f / scale;
}

} // namespace sg3

extern "C" {

int sg3_clip_layernorm_bwd(const sg3_clip_layernorm_bwd_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->dy && p->x && p->gamma && p->dx, "clip_layernorm_bwd: null tensor");
    SG3_REQUIRE(p->rows > 0 && p->D > 0, "clip_layernorm_bwd: rows %d, D %d", p->rows, p->D);
    SG3_REQUIRE(p->dyRowStride >= p->D && p->xRowStride >= p->D && p->dxRowStride >= p->D, "clip_layernorm_bwd: row strides %lld, %lld, %lld below D %d",
                (long long)p->dyRowStride, (long long)p->xRowStride, (long long)p->dxRowStride, p->D);
    SG3_REQUIRE((const void*)p->dy != (const void*)p->dx || p->dyRowStride == p->dxRowStride, "clip_layernorm_bwd: in place needs equal row strides");
    SG3_REQUIRE((const void*)p->x != (const void*)p->dx, "clip_layernorm_bwd: dx must not be x");
    hipLaunchKernelGGL(clip_layernorm_bwd_kernel, dim3(ceil_div(p->rows, 4)), dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_layernorm_bwd_kernel");
    return SG3_OK;
}

int sg3_clip_attention_bwd(const sg3_clip_attention_bwd_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->qkv && p->dout && p->dqkv, "clip_attention_bwd: null tensor");
    SG3_REQUIRE(p->B > 0 && p->heads > 0 && p->L >= 1 && p->L <= kMaxL, "clip_attention_bwd: B %d, heads %d, L %d (at most %d)", p->B, p->heads, p->L, kMaxL);
    SG3_REQUIRE(p->causal == 0, "clip_attention_bwd: the causal backward is not built (the text tower has no backward)");
    SG3_REQUIRE(((uintptr_t)p->qkv & 3) == 0 && ((uintptr_t)p->dout & 3) == 0, "clip_attention_bwd: qkv and dout must be 4-byte aligned");
    SG3_REQUIRE(p->qkv != (const void*)p->dqkv && p->dout != (const void*)p->dqkv, "clip_attention_bwd: dqkv must not be an input");
    SG3_REQUIRE((int64_t)p->B * p->heads < (1ll << 31), "clip_attention_bwd: batch too large for one launch");
    hipLaunchKernelGGL(clip_attention_bwd_kernel, dim3((unsigned)(p->B * p->heads)), dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_attention_bwd_kernel");
    return SG3_OK;
}

int sg3_clip_grad_scale(const sg3_clip_grad_scale_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->g && p->out16 && p->inv, "clip_grad_scale: null tensor");
    SG3_REQUIRE(p->B > 0 && p->E > 0, "clip_grad_scale: B %d, E %d", p->B, p->E);
    hipLaunchKernelGGL(clip_grad_scale_kernel, dim3((unsigned)p->B), dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_grad_scale_kernel");
    return SG3_OK;
}

} // extern "C"
