// sg3_clip.hip -- the kernels of CLIP's ViT encoders (reference models/styleganxl/feature_networks/clip/model.py:153-236, :324-352):
// LayerNorm, a K-contiguous fp16 GEMM with fused epilogues, 64-wide-head attention and the text embedding.
//
// Numerics: the residual stream is fp32.  GEMM operands are fp16 (weights rounded once when they are prepared, activations
// rounded by the kernel that produces them), products accumulate in fp32 on v_mfma_f32_16x16x32_f16 in ascending k, one
// accumulator per output element: no split-K, no atomics, so an output row depends on its own input row only and a sample's
// features are bit-identical whatever batch it is in.  LayerNorm statistics, softmax and QuickGELU are fp32.
//
// GEMM: C[M,N] = A[M,K] . W[N,K]^T, both operands K-contiguous, so the 8 consecutive k a lane feeds to one MFMA are one 16-byte
// read: lane l holds A[row l & 15][k = 8 (l >> 4) + j] and W[col l & 15][the same k]; the result has its column on l & 15 and rows
// 4 (l >> 4) + r in register r.  A workgroup of four waves makes a 64 x 64 tile (32 x 32 per wave, 2 x 2 MFMA blocks) over 64-deep
// K stages (two MFMA steps of 32), staged through LDS with the next stage's global loads in flight during the MFMAs and two LDS
// buffers, one barrier per stage.  64 x 64 tiles keep the thin GEMMs of the sweep on every CU: M = 1600, N = 768 is 300
// workgroups.  LDS rows are 16 bytes longer than their data, which spreads the 16 rows of a ds_read_b128 fragment read over the
// banks.
//
// The patch-embedding form gathers A from the fp32 NCHW image: the convolution's stride equals its kernel, so row m is patch
// (sample, py, px) and k = (c * P + ky) * P + kx; 8 consecutive k are 8 consecutive pixels of one image row (P % 8 == 0).
//
// sg3_clip_gemm_grad is a second entry point of the same kernel for the recording forward and the backward of the image tower
// (the rest of that backward is sg3_clip_grad.hip): dX = dY . W on [in][out] copies of the matrices, with the epilogues
// residual-from-aux, QuickGELU + saved pre-activation, x QuickGELU'(u), and the patch-embedding adjoint, and with a float32 A
// operand (the gradient stream) rounded to float16 as it is loaded.
#include "sg3_common.h"

namespace sg3 {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

static constexpr int kMaxL = 128;        // attention keeps K and V of one (sample, head) in LDS

// ---------------------------------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row.  The row's first element is the pivot: d = x - x[0] is of the size of the row's spread even when
// the mean is large, so mean(d) and mean((d - mean(d))^2) lose nothing to cancellation (two passes, biased variance, as torch).
// Every element is read and written by the same lane, so out may be x itself.
// ---------------------------------------------------------------------------------------------------------------------------
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

template <typename OUT>
__global__ void __launch_bounds__(256)
clip_layernorm_kernel(sg3_clip_layernorm_params p) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const float* x = p.x + row * p.xRowStride;
    OUT* out = (OUT*)p.out + row * (int64_t)p.D;
    const float pivot = x[0];
    float s = 0.0f;
    for (int d = lane; d < p.D; d += 64) s += x[d] - pivot;
    const float md = wave_sum(s) / (float)p.D;
    float q = 0.0f;
    for (int d = lane; d < p.D; d += 64) { const float t = (x[d] - pivot) - md; q += t * t; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)p.D + p.eps);
    for (int d = lane; d < p.D; d += 64) {
        const float t = ((x[d] - pivot) - md) * rstd;
        out[d] = (OUT)(t * p.gamma[d] + p.beta[d]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// GEMM
// ---------------------------------------------------------------------------------------------------------------------------
#ifndef SG3_CLIP_TK
#define SG3_CLIP_TK 64      // measured against 32 on the ViT-B/32 shapes: 5 - 20 % less time per GEMM, DESIGN.md 3.9
#endif
static constexpr int TM = 64, TN = 64, TK = SG3_CLIP_TK, PITCH = TK + 8;      // PITCH in halfs: LDS rows 16 bytes longer than their data
static constexpr int SEGS = TK / 8;                      // 16-byte segments per row of a stage
static constexpr int LOADS = TM * SEGS / 256;            // segments per thread, per operand and stage
static_assert(TK % 32 == 0 && LOADS >= 1, "stage depth");

// the kernel's arguments: what sg3_clip_gemm_params and sg3_clip_gemm_grad_params hold between them (the epilogue is a template argument)
struct gemm_args {
    const void* a; const void* w; const float* bias; void* out; const float* pos; const float* cls; void* aux; const float* scale;
    int32_t M, K, N, P, R;
};

__device__ __forceinline__ uint4 halfs_of(const float* src) {
    const float4 lo = *(const float4*)src, hi = *(const float4*)(src + 4);
    half8 h = {(_Float16)lo.x, (_Float16)lo.y, (_Float16)lo.z, (_Float16)lo.w, (_Float16)hi.x, (_Float16)hi.y, (_Float16)hi.z, (_Float16)hi.w};
    return *(uint4*)&h;
}

// A32: a is float32 and rounded to float16 here (the gradient stream as an operand).  The patch adjoint reads token 1 + patch of
// each sample: row m of the product is row (m / g^2) (g^2 + 1) + 1 + m % g^2 of a.
template <int EPI, bool A32>
__device__ __forceinline__ uint4 load_a(const gemm_args& p, int m, int k) {
    uint4 r = make_uint4(0, 0, 0, 0);
    if (m >= p.M || k >= p.K) return r;
    if (EPI != SG3_CLIP_EPI_PATCH) {
        int64_t row = m;
        if (EPI == SG3_CLIP_EPI_PATCH_ADJOINT) { const int g = p.R / p.P, gg = g * g; row = (int64_t)(m / gg) * (gg + 1) + 1 + m % gg; }
        if (A32) return halfs_of((const float*)p.a + row * p.K + k);
        return *(const uint4*)((const _Float16*)p.a + row * p.K + k);
    }
    const int g = p.R / p.P, gg = g * g, PP = p.P * p.P;
    const int b = m / gg, pi = m - b * gg, py = pi / g, px = pi - py * g;
    const int c = k / PP, rem = k - c * PP, ky = rem / p.P, kx = rem - ky * p.P;
    const float* src = (const float*)p.a + (((int64_t)b * 3 + c) * p.R + (py * p.P + ky)) * p.R + (px * p.P + kx);
    return halfs_of(src);
}

__device__ __forceinline__ float quick_gelu(float v) { return v / (1.0f + __expf(-1.702f * v)); }
// d/du [u sigmoid(1.702 u)] = s (1 + 1.702 u (1 - s)); expf, not __expf: the derivative multiplies every gradient of the MLP branch
__device__ __forceinline__ float quick_gelu_grad(float u) {
    const float s = 1.0f / (1.0f + expf(-1.702f * u));
    return s * (1.0f + 1.702f * u * (1.0f - s));
}

template <int EPI, bool A32>
__global__ void __launch_bounds__(256)
clip_gemm_kernel(gemm_args p) {
    __shared__ __attribute__((aligned(16))) _Float16 sA[2][TM * PITCH];
    __shared__ __attribute__((aligned(16))) _Float16 sW[2][TN * PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * TM, n0 = blockIdx.x * TN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int fr = lane & 15, fk = (lane >> 4) * 8;

    floatx4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};

    // the 16-byte segments of a stage this thread moves: segment s is row (tid + 256 s) / SEGS, first k ((tid + 256 s) % SEGS) * 8.
    // N % 64 == 0, so every W row of the tile exists; a stage may reach past K (K % 32 == 0 only), where zeros are staged.
    uint4 ra[LOADS], rw[LOADS];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int s = 0; s < LOADS; s++) {
            const int e = tid + 256 * s, row = e / SEGS, k = k0 + (e % SEGS) * 8;
            ra[s] = load_a<EPI, A32>(p, m0 + row, k);
            rw[s] = k < p.K ? *(const uint4*)((const _Float16*)p.w + (int64_t)(n0 + row) * p.K + k) : make_uint4(0, 0, 0, 0);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int s = 0; s < LOADS; s++) {
            const int e = tid + 256 * s, o = (e / SEGS) * PITCH + (e % SEGS) * 8;
            *(uint4*)&sA[buf][o] = ra[s];
            *(uint4*)&sW[buf][o] = rw[s];
        }
    };

    const int nk = (p.K + TK - 1) / TK;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int cur = kt & 1;
        if (kt + 1 < nk) fetch((kt + 1) * TK);
#pragma unroll
        for (int kk = 0; kk < TK; kk += 32) {
            half8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; i++) a[i] = *(const half8*)&sA[cur][(wm + i * 16 + fr) * PITCH + kk + fk];
#pragma unroll
            for (int j = 0; j < 2; j++) b[j] = *(const half8*)&sW[cur][(wn + j * 16 + fr) * PITCH + kk + fk];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) stash(cur ^ 1);
        __syncthreads();
    }

    const int g = (EPI == SG3_CLIP_EPI_PATCH || EPI == SG3_CLIP_EPI_PATCH_ADJOINT) ? p.R / p.P : 1, gg = g * g;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
            if (m >= p.M) continue;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int n = n0 + wn + j * 16 + fr;
                float v = acc[i][j][r];
                if (p.bias) v += p.bias[n];
                const int64_t o = (int64_t)m * p.N + n;
                if (EPI == SG3_CLIP_EPI_F32) ((float*)p.out)[o] = v;
                else if (EPI == SG3_CLIP_EPI_F16) ((_Float16*)p.out)[o] = (_Float16)v;
                else if (EPI == SG3_CLIP_EPI_QUICKGELU_F16) ((_Float16*)p.out)[o] = (_Float16)quick_gelu(v);
                else if (EPI == SG3_CLIP_EPI_RESIDUAL) ((float*)p.out)[o] = (p.aux ? (const float*)p.aux : (const float*)p.out)[o] + v;
                else if (EPI == SG3_CLIP_EPI_QUICKGELU_SAVE_F16) {
                    ((_Float16*)p.aux)[o] = (_Float16)v;
                    ((_Float16*)p.out)[o] = (_Float16)quick_gelu(v);
                } else if (EPI == SG3_CLIP_EPI_DQUICKGELU_F16) ((_Float16*)p.out)[o] = (_Float16)(v * quick_gelu_grad((float)((const _Float16*)p.aux)[o]));
                else if (EPI == SG3_CLIP_EPI_PATCH_ADJOINT) {
                    const int PP = p.P * p.P;
                    const int b = m / gg, pi = m - b * gg, py = pi / g, px = pi - py * g;
                    const int c = n / PP, rem = n - c * PP, ky = rem / p.P, kx = rem - ky * p.P;
                    ((float*)p.out)[(((int64_t)b * 3 + c) * p.R + (py * p.P + ky)) * p.R + (px * p.P + kx)] = p.scale ? v * p.scale[b] : v;
                } else {
                    const int b = m / gg, pi = m - b * gg;
                    float* tok = (float*)p.out + ((int64_t)b * (gg + 1)) * p.N + n;
                    tok[(int64_t)(1 + pi) * p.N] = v + p.pos[(int64_t)(1 + pi) * p.N + n];
                    if (pi == 0) tok[0] = p.cls[n] + p.pos[n];
                }
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention: one workgroup per (sample, head), head dimension 64.  K and V of the head sit in LDS as fp16 (as the QKV GEMM wrote
// them; K rows 66 halfs apart so the 64 lanes that each walk their own key row hit 64 different banks).  A wave takes query rows
// wave, wave + 4, ...: lane j scores keys j and j + 64 (fp32 sum over the 64 dimensions, times 1/8), the row's max and sum
// go over the wave, then lane d sums p[j] * V[j][d] in ascending j.  causal: keys j <= i only.
// ---------------------------------------------------------------------------------------------------------------------------
static constexpr int KP = 66;

__global__ void __launch_bounds__(256)
clip_attention_kernel(sg3_clip_attention_params p) {
    __shared__ __attribute__((aligned(16))) _Float16 sK[kMaxL * KP];
    __shared__ __attribute__((aligned(16))) _Float16 sV[kMaxL * 64];
    __shared__ float sQ[4][64];
    __shared__ float sP[4][kMaxL];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / p.heads, h = blockIdx.x - b * p.heads;
    const int D = p.heads * 64, L = p.L;
    const _Float16* base = (const _Float16*)p.qkv + (int64_t)b * L * 3 * D + h * 64;
    for (int e = tid; e < L * 32; e += 256) {                   // half2 at a time
        const int j = e >> 5, d2 = (e & 31) * 2;
        const _Float16* row = base + (int64_t)j * 3 * D;
        *(uint32_t*)&sK[j * KP + d2] = *(const uint32_t*)(row + D + d2);
        *(uint32_t*)&sV[j * 64 + d2] = *(const uint32_t*)(row + 2 * D + d2);
    }
    __syncthreads();
    for (int i0 = 0; i0 < L; i0 += 4) {                         // every wave makes every trip (the barriers): a wave past the end redoes row L - 1
        const int i = min(i0 + wave, L - 1);
        sQ[wave][lane] = (float)base[(int64_t)i * 3 * D + lane];
        __syncthreads();
        const int nkeys = p.causal ? i + 1 : L;
        float s[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const int j = lane + t * 64;
            float a = 0.0f;
            if (j < nkeys) {
#pragma unroll 8
                for (int d = 0; d < 64; d += 2) {
                    const uint32_t kk = *(const uint32_t*)&sK[j * KP + d];
                    const _Float16* k2 = (const _Float16*)&kk;
                    a += sQ[wave][d] * (float)k2[0];
                    a += sQ[wave][d + 1] * (float)k2[1];
                }
                a *= 0.125f;
            } else a = -INFINITY;
            s[t] = a;
        }
        const float mx = wave_max(fmaxf(s[0], s[1]));             // key 0 is always attended: mx is finite
        const float e0 = lane < nkeys ? expf(s[0] - mx) : 0.0f;
        const float e1 = lane + 64 < nkeys ? expf(s[1] - mx) : 0.0f;
        const float inv = 1.0f / wave_sum(e0 + e1);
        sP[wave][lane] = e0 * inv;
        sP[wave][lane + 64] = e1 * inv;
        __syncthreads();
        float o = 0.0f;
        for (int j = 0; j < nkeys; j++) o += sP[wave][j] * (float)sV[j * 64 + lane];
        if (i0 + wave < L) ((_Float16*)p.out)[((int64_t)b * L + i) * D + h * 64 + lane] = (_Float16)o;
        __syncthreads();
    }
}

// text embedding: x[b, l, :] = table[token[b, l]] + pos[l]; a token outside the table is clamped to it (torch would assert)
__global__ void __launch_bounds__(256)
clip_embed_kernel(sg3_clip_embed_params p) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (int64_t)p.B * p.L) return;
    int64_t t = p.tokens[row];
    t = t < 0 ? 0 : (t >= p.vocab ? p.vocab - 1 : t);
    const float* e = p.table + t * p.D;
    const float* ps = p.pos + (row % p.L) * p.D;
    float* o = p.out + row * p.D;
    for (int d = threadIdx.x & 63; d < p.D; d += 64) o[d] = e[d] + ps[d];
}

static inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <int EPI, bool A32 = false>
static int launch_gemm(const gemm_args& p, hipStream_t s) {
    hipLaunchKernelGGL((clip_gemm_kernel<EPI, A32>), dim3(p.N / TN, ceil_div(p.M, TM)), dim3(256), 0, s, p);
    SG3_LAUNCH_CHECK("clip_gemm_kernel");
    return SG3_OK;
}

} // namespace sg3

extern "C" {

int sg3_clip_supported(int width, int heads, int L) {
    return width > 0 && heads > 0 && width == heads * 64 && L >= 1 && L <= sg3::kMaxL;
}

int sg3_clip_layernorm(const sg3_clip_layernorm_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->x && p->gamma && p->beta && p->out, "clip_layernorm: null tensor");
    SG3_REQUIRE(p->rows > 0 && p->D > 0 && p->xRowStride >= 0, "clip_layernorm: rows %d, D %d, row stride %lld", p->rows, p->D, (long long)p->xRowStride);
    SG3_REQUIRE(p->outDtype == SG3_F32 || p->outDtype == SG3_F16, "clip_layernorm: out must be float32 or float16");
    SG3_REQUIRE((const void*)p->x != p->out || (p->outDtype == SG3_F32 && p->xRowStride == p->D), "clip_layernorm: in place needs float32 out and dense rows");
    const dim3 grid(ceil_div(p->rows, 4));
    if (p->outDtype == SG3_F16) hipLaunchKernelGGL(clip_layernorm_kernel<_Float16>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    else hipLaunchKernelGGL(clip_layernorm_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_layernorm_kernel");
    return SG3_OK;
}

// what both GEMM entry points check: sizes, alignment, grid
#define SG3_CLIP_GEMM_COMMON(name)                                                                                                      \
    SG3_REQUIRE(p && p->a && p->w && p->out, name ": null tensor");                                                                     \
    SG3_REQUIRE(p->M > 0 && p->N > 0 && p->K > 0, name ": sizes must be positive (M %d, N %d, K %d)", p->M, p->N, p->K);                \
    SG3_REQUIRE(p->N % 64 == 0, name ": N %d is not a multiple of 64", p->N);                                                           \
    SG3_REQUIRE(p->K % 32 == 0, name ": K %d is not a multiple of 32", p->K)

int sg3_clip_gemm(const sg3_clip_gemm_params* p, void* stream) {
    using namespace sg3;
    SG3_CLIP_GEMM_COMMON("clip_gemm");
    SG3_REQUIRE(p->epilogue >= SG3_CLIP_EPI_F32 && p->epilogue <= SG3_CLIP_EPI_PATCH, "clip_gemm: unknown epilogue %d", p->epilogue);
    SG3_REQUIRE(aligned16(p->a) && aligned16(p->w), "clip_gemm: a and w must be 16-byte aligned");
    SG3_REQUIRE((int64_t)ceil_div(p->M, TM) <= 65535, "clip_gemm: M %d too large for one launch", p->M);
    if (p->epilogue == SG3_CLIP_EPI_PATCH) {
        SG3_REQUIRE(p->pos && p->cls, "clip_gemm: the patch embedding needs pos and cls");
        SG3_REQUIRE(p->P > 0 && p->P % 8 == 0 && p->R >= p->P && p->R % 4 == 0, "clip_gemm: patch %d (a multiple of 8), resolution %d (a multiple of 4)", p->P, p->R);
        SG3_REQUIRE(p->K == 3 * p->P * p->P, "clip_gemm: K %d is not 3 * patch^2", p->K);
        const int g = p->R / p->P;
        SG3_REQUIRE(p->M % (g * g) == 0, "clip_gemm: M %d is not a whole number of %d x %d patch grids", p->M, g, g);
    }
    const gemm_args q = {p->a, p->w, p->bias, p->out, p->pos, p->cls, nullptr, nullptr, p->M, p->K, p->N, p->P, p->R};
    hipStream_t s = (hipStream_t)stream;
    switch (p->epilogue) {
        case SG3_CLIP_EPI_F32:           return launch_gemm<SG3_CLIP_EPI_F32>(q, s);
        case SG3_CLIP_EPI_F16:           return launch_gemm<SG3_CLIP_EPI_F16>(q, s);
        case SG3_CLIP_EPI_QUICKGELU_F16: return launch_gemm<SG3_CLIP_EPI_QUICKGELU_F16>(q, s);
        case SG3_CLIP_EPI_RESIDUAL:      return launch_gemm<SG3_CLIP_EPI_RESIDUAL>(q, s);
        default:                         return launch_gemm<SG3_CLIP_EPI_PATCH>(q, s);
    }
}

int sg3_clip_gemm_grad(const sg3_clip_gemm_grad_params* p, void* stream) {
    using namespace sg3;
    SG3_CLIP_GEMM_COMMON("clip_gemm_grad");
    const int e = p->epilogue;
    const bool a32 = p->aF32 != 0;
    const bool reads_aux = e == SG3_CLIP_EPI_RESIDUAL || e == SG3_CLIP_EPI_DQUICKGELU_F16, writes_aux = e == SG3_CLIP_EPI_QUICKGELU_SAVE_F16;
    SG3_REQUIRE(e == SG3_CLIP_EPI_F32 || e == SG3_CLIP_EPI_F16 || reads_aux || writes_aux || e == SG3_CLIP_EPI_PATCH_ADJOINT, "clip_gemm_grad: unknown epilogue %d", e);
    SG3_REQUIRE(!a32 || e == SG3_CLIP_EPI_F16 || e == SG3_CLIP_EPI_DQUICKGELU_F16 || e == SG3_CLIP_EPI_PATCH_ADJOINT,
                "clip_gemm_grad: a float32 operand a is not built for epilogue %d", e);
    SG3_REQUIRE((p->aux != nullptr) == (reads_aux || writes_aux), "clip_gemm_grad: epilogue %d %s", e, p->aux ? "takes no aux" : "needs aux");
    SG3_REQUIRE(!writes_aux || (p->aux != p->out && p->aux != p->a), "clip_gemm_grad: aux must not be out or a");
    SG3_REQUIRE(!p->scale || e == SG3_CLIP_EPI_PATCH_ADJOINT, "clip_gemm_grad: epilogue %d takes no scale", e);
    SG3_REQUIRE(aligned16(p->a) && aligned16(p->w), "clip_gemm_grad: a and w must be 16-byte aligned");
    SG3_REQUIRE((int64_t)ceil_div(p->M, TM) <= 65535, "clip_gemm_grad: M %d too large for one launch", p->M);
    if (e == SG3_CLIP_EPI_PATCH_ADJOINT) {
        SG3_REQUIRE(p->P > 0 && p->P % 8 == 0 && p->R >= p->P, "clip_gemm_grad: patch %d (a multiple of 8), resolution %d", p->P, p->R);
        SG3_REQUIRE(p->N == 3 * p->P * p->P, "clip_gemm_grad: N %d is not 3 * patch^2", p->N);
        SG3_REQUIRE(!p->bias, "clip_gemm_grad: the patch adjoint takes no bias");
        const int g = p->R / p->P;
        SG3_REQUIRE(p->M % (g * g) == 0, "clip_gemm_grad: M %d is not a whole number of %d x %d patch grids", p->M, g, g);
    }
    const gemm_args q = {p->a, p->w, p->bias, p->out, nullptr, nullptr, p->aux, p->scale, p->M, p->K, p->N, p->P, p->R};
    hipStream_t s = (hipStream_t)stream;
    switch (e) {
        case SG3_CLIP_EPI_F32:                return launch_gemm<SG3_CLIP_EPI_F32>(q, s);
        case SG3_CLIP_EPI_F16:                return a32 ? launch_gemm<SG3_CLIP_EPI_F16, true>(q, s) : launch_gemm<SG3_CLIP_EPI_F16>(q, s);
        case SG3_CLIP_EPI_RESIDUAL:           return launch_gemm<SG3_CLIP_EPI_RESIDUAL>(q, s);
        case SG3_CLIP_EPI_QUICKGELU_SAVE_F16: return launch_gemm<SG3_CLIP_EPI_QUICKGELU_SAVE_F16>(q, s);
        case SG3_CLIP_EPI_DQUICKGELU_F16:     return a32 ? launch_gemm<SG3_CLIP_EPI_DQUICKGELU_F16, true>(q, s) : launch_gemm<SG3_CLIP_EPI_DQUICKGELU_F16>(q, s);
        default:                              return a32 ? launch_gemm<SG3_CLIP_EPI_PATCH_ADJOINT, true>(q, s) : launch_gemm<SG3_CLIP_EPI_PATCH_ADJOINT>(q, s);
    }
}

int sg3_clip_attention(const sg3_clip_attention_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->qkv && p->out, "clip_attention: null tensor");
    SG3_REQUIRE(p->B > 0 && p->heads > 0 && p->L >= 1 && p->L <= kMaxL, "clip_attention: B %d, heads %d, L %d (at most %d)", p->B, p->heads, p->L, kMaxL);
    SG3_REQUIRE(((uintptr_t)p->qkv & 3) == 0, "clip_attention: qkv must be 4-byte aligned");
    SG3_REQUIRE((int64_t)p->B * p->heads < (1ll << 31), "clip_attention: batch too large for one launch");
    hipLaunchKernelGGL(clip_attention_kernel, dim3((unsigned)(p->B * p->heads)), dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_attention_kernel");
    return SG3_OK;
}

int sg3_clip_embed(const sg3_clip_embed_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p && p->tokens && p->table && p->pos && p->out, "clip_embed: null tensor");
    SG3_REQUIRE(p->B > 0 && p->L > 0 && p->D > 0 && p->vocab > 0, "clip_embed: sizes must be positive");
    const int64_t blocks = ceil_div64((int64_t)p->B * p->L, 4);
    SG3_REQUIRE(blocks < (1ll << 31), "clip_embed: batch too large for one launch");
    hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, *p);
    SG3_LAUNCH_CHECK("clip_embed_kernel");
    return SG3_OK;
}

} // extern "C"
