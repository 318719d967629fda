// sg3_latent_mapper.hip -- StyleCLIP latent mapper forward (every group of a SingleMapper / LevelsMapper) in five launches.
//
// Reference: editing/styleclip_mapper/latent_mappers.py:9-25 (Mapper = PixelNorm + 4 x EqualLinear(512, 512, lr_mul=0.01,
// activation='fused_lrelu')), :46-78 (LevelsMapper: levels 0-4 / 5-7 / 8-15, a disabled group gives zeros), :136-137 (PixelNorm
// over dim 1, i.e. over the LEVELS of one sample), :117-127 (EqualLinear: leaky_relu(x @ (W * scale)^T + b * lr_mul, 0.2) * sqrt(2)),
// and scripts/inference.py:98 (w_hat = w + 0.1 * mapper(w)).
//
// Layout: activations stay [N][L][512] in two ping-pong scratch buffers, so a group is a level range plus a weight index and all
// groups of one layer are one launch.
//   pixelnorm_kernel   one thread per (n, feature): per group, x * rsqrt(mean over the group's levels of x^2 + 1e-8) -> scratch 0;
//                      levels outside every group get delta = 0 and out = x + alpha * 0 here.
//   layer_kernel x 4   a workgroup is (group, 32-row block of the group's N * Lg rows, 32-column block).  Its four waves each take
//                      one K quarter of 128 and run v_mfma_f32_32x32x2_f32 (fp32 products, fp32 accumulation) over it in a fixed
//                      order; the quarters are summed in LDS as ((q0 + q1) + q2) + q3.  Epilogue: + b * lr_mul, leaky_relu(0.2),
//                      * sqrt(2), each rounded separately as the reference's three elementwise ops; the last layer writes delta
//                      and out = x + alpha * delta (product and sum rounded separately, as `w + 0.1 * mapper(w)`).
// Every output element is the same sequence of operations whatever row block it lands in, so a latent's result does not depend
// on the batch it is in (batch invariance).  Layer boundaries are kernel boundaries: no hand-off between workgroups of a launch.
// Weights are the caller's prepared copy: (W * scale) in the stored [out][in] order (lane li of the MFMA B operand reads four
// consecutive inputs of output column li as one 16-byte load) and b * lr_mul.
//
// Training (sg3_latent_mapper_train_forward, sg3_latent_mapper_backward): the same two forward kernels writing h0..h3 into the
// caller's acts and h4 into delta, and a backward of at most ten launches, described above its kernels below.
#include "sg3_common.h"

namespace sg3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int kD = 512;            // latent width (the only one supported)
static constexpr int kTile = 32;          // rows and columns of one workgroup's output tile
static constexpr int kColBlocks = kD / kTile;
static constexpr int kQuarter = kD / 4;   // K range of one wave
static constexpr int kMaxGroups = 4;
static constexpr int kMaxLevels = 32;     // levels per latent (16 for StyleGAN3 W+)

struct MapperLaunch {
    const float* x;
    const float* weight;      // [G][4][512][512]
    const float* bias;        // [G][4][512]
    float* out;
    float* delta;
    const float* in;          // this layer's input  (scratch)
    float* dst;               // this layer's output (scratch; unused by the last layer)
    int N, L, G, layer;
    int begin[kMaxGroups], end[kMaxGroups];
    int tileStart[kMaxGroups + 1];   // first workgroup of group g; tileStart[G] = grid size
    float alpha;
};

__global__ void __launch_bounds__(256)
pixelnorm_kernel(MapperLaunch a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.N * kD) return;
    const int n = t / kD, k = t % kD;
    const size_t base = (size_t)n * a.L * kD + k;
    // every level of this (sample, feature) is loaded once, all loads in flight together
    float v[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) v[l] = l < a.L ? a.x[base + (size_t)l * kD] : 0.f;
    bool mapped[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) mapped[l] = false;
    for (int g = 0; g < a.G; g++) {
        float ss = 0.f;
#pragma unroll
        for (int l = 0; l < kMaxLevels; l++)
            if (l >= a.begin[g] && l < a.end[g]) ss = __fadd_rn(ss, __fmul_rn(v[l], v[l]));
        const float r = 1.0f / __fsqrt_rn(__fadd_rn(__fdiv_rn(ss, (float)(a.end[g] - a.begin[g])), 1e-8f));
#pragma unroll
        for (int l = 0; l < kMaxLevels; l++)
            if (l >= a.begin[g] && l < a.end[g]) { a.dst[base + (size_t)l * kD] = __fmul_rn(v[l], r); mapped[l] = true; }
    }
    // levels of a disabled group (or outside every group): delta = zeros, out = x + alpha * 0
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) {
        if (l >= a.L || mapped[l]) continue;
        if (a.delta) a.delta[base + (size_t)l * kD] = 0.f;
        if (a.out) a.out[base + (size_t)l * kD] = __fadd_rn(v[l], __fmul_rn(a.alpha, 0.f));
    }
}

template <bool LAST>
__global__ void __launch_bounds__(256)
layer_kernel(MapperLaunch a) {
    __shared__ float part[4][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int bid = blockIdx.x;
    int g = 0;
    while (g + 1 < a.G && bid >= a.tileStart[g + 1]) g++;
    const int local = bid - a.tileStart[g];
    const int cb = local % kColBlocks, rb = local / kColBlocks;
    const int l0 = a.begin[g], Lg = a.end[g] - a.begin[g];
    const int M = a.N * Lg;
    const float* W = a.weight + ((size_t)g * 4 + a.layer) * kD * kD;
    const float* B = a.bias + ((size_t)g * 4 + a.layer) * kD;

    // A operand: lane li = row m of the group (sample m / Lg, level l0 + m % Lg); B operand: lane li = output column
    const int m = rb * kTile + li;
    const bool rowOk = m < M;
    const float* arow = a.in + ((size_t)(rowOk ? m / Lg : 0) * a.L + l0 + (rowOk ? m % Lg : 0)) * kD + wave * kQuarter + 4 * lh;
    const float* wrow = W + (size_t)(cb * kTile + li) * kD + wave * kQuarter + 4 * lh;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    f32x4 fa[kQuarter / 8], fb[kQuarter / 8];
#pragma unroll
    for (int c = 0; c < kQuarter / 8; c++) {
        fb[c] = *reinterpret_cast<const f32x4*>(wrow + c * 8);
        fa[c] = rowOk ? *reinterpret_cast<const f32x4*>(arow + c * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < kQuarter / 8; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][q], fb[c][q], acc, 0, 0, 0);

#pragma unroll
    for (int r = 0; r < 16; r++) part[wave][r][lane] = acc[r];
    __syncthreads();

    // thread -> 4 of the tile's 1024 elements: register r = 4 * wave + j of lane `lane`
    const int col = cb * kTile + li;
    const float bv = B[col];
    const float sqrt2 = 1.41421356237309515f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = 4 * wave + j;
        const int row = rb * kTile + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row >= M) continue;
        float s = __fadd_rn(__fadd_rn(__fadd_rn(part[0][r][lane], part[1][r][lane]), part[2][r][lane]), part[3][r][lane]);
        float v = __fadd_rn(s, bv);
        v = v > 0.f ? v : __fmul_rn(v, 0.2f);
        v = __fmul_rn(v, sqrt2);
        const size_t i = ((size_t)(row / Lg) * a.L + l0 + row % Lg) * kD + col;
        if (LAST) {
            if (a.delta) a.delta[i] = v;
            if (a.out) a.out[i] = __fadd_rn(a.x[i], __fmul_rn(a.alpha, v));
        } else {
            a.dst[i] = v;
        }
    }
}

static bool overlaps(const void* p, size_t pb, const void* q, size_t qb) {
    if (!p || !q || !pb || !qb) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

// PixelNorm into h[0], then layer i reads h[i] and writes h[i + 1] (the last layer writes delta / out and no h).
static int run_forward(MapperLaunch a, float* const h[5], hipStream_t st) {
    a.dst = h[0];
    hipLaunchKernelGGL(pixelnorm_kernel, dim3((unsigned)ceil_div(a.N * kD, 256)), dim3(256), 0, st, a);
    SG3_LAUNCH_CHECK("latent_mapper pixelnorm_kernel");
    if (a.G == 0) return SG3_OK;
    const dim3 grid((unsigned)a.tileStart[a.G]);
    for (int layer = 0; layer < 4; layer++) {
        a.layer = layer;
        a.in = h[layer];
        a.dst = h[layer + 1];
        if (layer < 3) hipLaunchKernelGGL(layer_kernel<false>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(layer_kernel<true>, grid, dim3(256), 0, st, a);
        SG3_LAUNCH_CHECK("latent_mapper layer_kernel");
    }
    return SG3_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Backward.  With weight index w = 0..3 (h_w -> z_(w+1) -> h_(w+1)) and dz_(w+1) = dh_(w+1) * (h_(w+1) > 0 ? sqrt2 : 0.2 * sqrt2):
//   dz4_kernel           one thread per element of a mapped level: (dDelta + alpha * dOut) * slope(h4) -> dz buffer 0.
//   wgrad_kernel  x 4    a workgroup is (group, 32 output rows, 32 input columns) of dW[g][w] = dz_(w+1)^T @ h_w.  The reduction runs
//                        over the group's M = N * Lg rows: each wave takes one contiguous quarter (rounded up to even) in ascending
//                        order, two rows per v_mfma_f32_32x32x2_f32, a missing second row is a zero operand; the quarters are summed
//                        in LDS as ((q0 + q1) + q2) + q3, then * scale.  Both operands are read 32 consecutive floats per row.
//                        The workgroups of input block 0 also sum their dz operand per lane and write dB = (column sum) * lr_mul.
//   dgrad_kernel  x 4    the forward's tiling with the weight read K-major: lane li of the B operand is input column li, so one
//                        wave load is two full 128-byte row segments of W (coalesced, 4 bytes per lane); the A operand (dz) is read
//                        as the forward reads its activations.  Epilogue: the fixed-order sum of the four K quarters, times the
//                        slope of the saved h_w (w >= 1) -> the other dz buffer; w == 0 writes dh0 unchanged.
//   pixelnorm_bwd_kernel one thread per (sample, feature), recomputing r exactly as the forward does.
struct MapperBwdLaunch {
    const float* x;
    const float* weight;      // [G][4][512][512]
    const float* acts;        // [4][N][L][512]
    const float* delta;       // h4
    const float* dDelta;
    const float* dOut;
    float* dx;
    float* dW;
    float* dB;
    const float* dz;          // dz_(w+1) of this launch (dh0 for the PixelNorm backward)
    float* dst;               // dz_w / dh0
    int N, L, G, layer;       // layer = weight index w
    int begin[kMaxGroups], end[kMaxGroups];
    int tileStart[kMaxGroups + 1];
    float alpha;
    float wScale[kMaxGroups * 4], bScale[kMaxGroups * 4];
};

static constexpr float kSqrt2 = 1.41421356237309515f;
static constexpr float kSqrt2Neg = 0.2f * 1.41421356237309515f;   // rounded once, on the host

__global__ void __launch_bounds__(256)
dz4_kernel(MapperBwdLaunch a) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)a.N * a.L * kD) return;
    const int l = (int)((t / kD) % a.L);
    bool mapped = false;
    for (int g = 0; g < a.G; g++) mapped = mapped || (l >= a.begin[g] && l < a.end[g]);
    if (!mapped) return;
    float d = a.dDelta ? a.dDelta[t] : 0.f;
    if (a.dOut) {
        const float o = __fmul_rn(a.alpha, a.dOut[t]);
        d = a.dDelta ? __fadd_rn(d, o) : o;
    }
    a.dst[t] = __fmul_rn(d, a.delta[t] > 0.f ? kSqrt2 : kSqrt2Neg);
}

template <bool TO_H0>
__global__ void __launch_bounds__(256)
dgrad_kernel(MapperBwdLaunch a) {
    __shared__ float part[4][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int bid = blockIdx.x;
    int g = 0;
    while (g + 1 < a.G && bid >= a.tileStart[g + 1]) g++;
    const int local = bid - a.tileStart[g];
    const int cb = local % kColBlocks, rb = local / kColBlocks;
    const int l0 = a.begin[g], Lg = a.end[g] - a.begin[g];
    const int M = a.N * Lg;
    const float* W = a.weight + ((size_t)g * 4 + a.layer) * kD * kD;

    // A operand: lane li = row m of the group, k = output feature of the layer; B operand: lane li = input column, k-major reads
    const int m = rb * kTile + li;
    const bool rowOk = m < M;
    const float* arow = a.dz + ((size_t)(rowOk ? m / Lg : 0) * a.L + l0 + (rowOk ? m % Lg : 0)) * kD + wave * kQuarter + 4 * lh;
    const float* wcol = W + (size_t)(wave * kQuarter + 4 * lh) * kD + cb * kTile + li;

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    f32x4 fa[kQuarter / 8], fb[kQuarter / 8];
#pragma unroll
    for (int c = 0; c < kQuarter / 8; c++) {
#pragma unroll
        for (int q = 0; q < 4; q++) fb[c][q] = wcol[(size_t)(c * 8 + q) * kD];
        fa[c] = rowOk ? *reinterpret_cast<const f32x4*>(arow + c * 8) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < kQuarter / 8; c++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][q], fb[c][q], acc, 0, 0, 0);

#pragma unroll
    for (int r = 0; r < 16; r++) part[wave][r][lane] = acc[r];
    __syncthreads();

    const int col = cb * kTile + li;
    const float* hw = a.acts + (size_t)a.layer * a.N * a.L * kD;     // h_w, read only when w >= 1
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = 4 * wave + j;
        const int row = rb * kTile + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (row >= M) continue;
        float s = __fadd_rn(__fadd_rn(__fadd_rn(part[0][r][lane], part[1][r][lane]), part[2][r][lane]), part[3][r][lane]);
        const size_t i = ((size_t)(row / Lg) * a.L + l0 + row % Lg) * kD + col;
        if (!TO_H0) s = __fmul_rn(s, hw[i] > 0.f ? kSqrt2 : kSqrt2Neg);
        a.dst[i] = s;
    }
}

__global__ void __launch_bounds__(256)
wgrad_kernel(MapperBwdLaunch a) {
    __shared__ float part[4][16][64];
    __shared__ float bpart[8][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int g = blockIdx.x / (kColBlocks * kColBlocks);
    const int local = blockIdx.x % (kColBlocks * kColBlocks);
    const int ob = local / kColBlocks, ib = local % kColBlocks;
    const int l0 = a.begin[g], Lg = a.end[g] - a.begin[g];
    const int M = a.N * Lg;
    const int Q = ((M + 3) / 4 + 1) & ~1;             // rows per wave, even: a wave's pairs never straddle a quarter
    const int m0 = wave * Q, m1 = min(m0 + Q, M);
    const float* dzc = a.dz + ob * kTile + li;                                        // A: lane li = output feature, k = row
    const float* hc = a.acts + (size_t)a.layer * a.N * a.L * kD + ib * kTile + li;    // B: lane li = input feature,  k = row

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.f;
    float bsum = 0.f;
    for (int mm = m0; mm < m1; mm += 8) {             // four row pairs in flight; pairs past the quarter are zero operands
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int row = mm + 2 * u + lh;
            const bool ok = row < m1;                  // odd tail: the second row of the pair is a zero operand
            const size_t off = ok ? ((size_t)(row / Lg) * a.L + l0 + row % Lg) * kD : 0;
            av[u] = ok ? dzc[off] : 0.f;
            bv[u] = ok ? hc[off] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
            bsum = __fadd_rn(bsum, av[u]);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) part[wave][r][lane] = acc[r];
    if (ib == 0) bpart[2 * wave + lh][li] = bsum;
    __syncthreads();

    const size_t gl = (size_t)g * 4 + a.layer;
    const float ws = a.wScale[gl];
    float* dW = a.dW + gl * kD * kD;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int r = 4 * wave + j;
        const int orow = ob * kTile + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float s = __fadd_rn(__fadd_rn(__fadd_rn(part[0][r][lane], part[1][r][lane]), part[2][r][lane]), part[3][r][lane]);
        dW[(size_t)orow * kD + ib * kTile + li] = __fmul_rn(s, ws);
    }
    if (ib == 0 && tid < kTile) {
        float s = bpart[0][tid];
#pragma unroll
        for (int q = 1; q < 8; q++) s = __fadd_rn(s, bpart[q][tid]);
        a.dB[gl * kD + ob * kTile + tid] = __fmul_rn(s, a.bScale[gl]);
    }
}

__global__ void __launch_bounds__(256)
pixelnorm_bwd_kernel(MapperBwdLaunch a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.N * kD) return;
    const int n = t / kD, k = t % kD;
    const size_t base = (size_t)n * a.L * kD + k;
    float v[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) v[l] = l < a.L ? a.x[base + (size_t)l * kD] : 0.f;
    bool mapped[kMaxLevels];
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) mapped[l] = false;
    for (int g = 0; g < a.G; g++) {
        float ss = 0.f;
#pragma unroll
        for (int l = 0; l < kMaxLevels; l++)
            if (l >= a.begin[g] && l < a.end[g]) ss = __fadd_rn(ss, __fmul_rn(v[l], v[l]));
        const float lg = (float)(a.end[g] - a.begin[g]);
        const float r = 1.0f / __fsqrt_rn(__fadd_rn(__fdiv_rn(ss, lg), 1e-8f));     // the forward's r, operation for operation
        float d[kMaxLevels];
        float S = 0.f;
#pragma unroll
        for (int l = 0; l < kMaxLevels; l++) {
            d[l] = 0.f;
            if (l >= a.begin[g] && l < a.end[g]) { d[l] = a.dz[base + (size_t)l * kD]; S = __fadd_rn(S, __fmul_rn(d[l], v[l])); }
        }
        const float c = __fmul_rn(__fdiv_rn(__fmul_rn(__fmul_rn(r, r), r), lg), S);
#pragma unroll
        for (int l = 0; l < kMaxLevels; l++)
            if (l >= a.begin[g] && l < a.end[g]) {
                float dxv = __fsub_rn(__fmul_rn(r, d[l]), __fmul_rn(v[l], c));
                if (a.dOut) dxv = __fadd_rn(dxv, a.dOut[base + (size_t)l * kD]);
                a.dx[base + (size_t)l * kD] = dxv;
                mapped[l] = true;
            }
    }
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) {
        if (l >= a.L || mapped[l]) continue;
        a.dx[base + (size_t)l * kD] = a.dOut ? a.dOut[base + (size_t)l * kD] : 0.f;
    }
}

// the shape and group checks shared by the three entry points
static int check_shape(const char* who, int N, int L, int D, int groups, const int32_t* lb, const int32_t* le) {
    SG3_REQUIRE(D == kD, "%s: D = %d (only 512 is supported)", who, D);
    SG3_REQUIRE(N > 0 && L > 0 && L <= kMaxLevels, "%s: bad shape N = %d, L = %d (L <= 32)", who, N, L);
    SG3_REQUIRE((int64_t)N * L * kD * 2 < (1ll << 31), "%s: batch of %d too large", who, N);
    SG3_REQUIRE(groups >= 0 && groups <= kMaxGroups, "%s: %d groups (0..4 supported)", who, groups);
    for (int g = 0; g < groups; g++) {
        SG3_REQUIRE(lb[g] >= 0 && lb[g] < le[g] && le[g] <= L, "%s: group %d covers levels [%d, %d) of %d (empty or out of range)", who, g, lb[g], le[g], L);
        for (int h = 0; h < g; h++)
            SG3_REQUIRE(le[h] <= lb[g] || le[g] <= lb[h], "%s: groups %d and %d overlap", who, h, g);
    }
    return SG3_OK;
}

} // namespace sg3

extern "C" {

int sg3_latent_mapper(const sg3_latent_mapper_params* p, void* stream) {
    using namespace sg3;
    SG3_REQUIRE(p, "latent_mapper: null params");
    SG3_REQUIRE(p->x, "latent_mapper: null x");
    SG3_REQUIRE(p->out || p->delta, "latent_mapper: neither out nor delta is given");
    SG3_REQUIRE(p->D == kD, "latent_mapper: D = %d (only 512 is supported)", p->D);
    SG3_REQUIRE(p->N > 0 && p->L > 0 && p->L <= kMaxLevels, "latent_mapper: bad shape N = %d, L = %d (L <= 32)", p->N, p->L);
    SG3_REQUIRE((int64_t)p->N * p->L * kD * 2 < (1ll << 31), "latent_mapper: batch of %d too large", p->N);
    SG3_REQUIRE(p->groups >= 0 && p->groups <= kMaxGroups, "latent_mapper: %d groups (0..4 supported)", p->groups);
    for (int g = 0; g < p->groups; g++) {
        SG3_REQUIRE(p->levelBegin[g] >= 0 && p->levelBegin[g] < p->levelEnd[g] && p->levelEnd[g] <= p->L,
                    "latent_mapper: group %d covers levels [%d, %d) of %d (empty or out of range)", g, p->levelBegin[g], p->levelEnd[g], p->L);
        for (int h = 0; h < g; h++)
            SG3_REQUIRE(p->levelEnd[h] <= p->levelBegin[g] || p->levelEnd[g] <= p->levelBegin[h],
                        "latent_mapper: groups %d and %d overlap", h, g);
    }
    const size_t act = (size_t)p->N * p->L * kD * sizeof(float);
    const size_t wb = (size_t)p->groups * 4 * kD * kD * sizeof(float), bb = (size_t)p->groups * 4 * kD * sizeof(float);
    if (p->groups > 0) {
        SG3_REQUIRE(p->weight && p->bias && p->scratch, "latent_mapper: null weight, bias or scratch");
        SG3_REQUIRE(((uintptr_t)p->weight & 15) == 0 && ((uintptr_t)p->scratch & 15) == 0, "latent_mapper: weight and scratch must be 16-byte aligned");
    }
    const void* bufs[6] = {p->x, p->out, p->delta, p->groups ? p->scratch : nullptr, p->groups ? p->weight : nullptr, p->groups ? p->bias : nullptr};
    const size_t sizes[6] = {act, act, act, 2 * act, wb, bb};
    for (int i = 1; i < 4; i++)                    // written buffers overlap nothing else
        for (int j = 0; j < 6; j++)
            SG3_REQUIRE(i == j || !overlaps(bufs[i], sizes[i], bufs[j], sizes[j]), "latent_mapper: buffers %d and %d overlap", i, j);

    MapperLaunch a = {};
    a.x = p->x; a.weight = p->weight; a.bias = p->bias; a.out = p->out; a.delta = p->delta;
    a.N = p->N; a.L = p->L; a.G = p->groups; a.alpha = p->alpha;
    a.tileStart[0] = 0;
    for (int g = 0; g < p->groups; g++) {
        a.begin[g] = p->levelBegin[g]; a.end[g] = p->levelEnd[g];
        a.tileStart[g + 1] = a.tileStart[g] + ceil_div(p->N * (a.end[g] - a.begin[g]), kTile) * kColBlocks;
    }
    float* s0 = p->scratch;
    float* s1 = p->groups ? p->scratch + (size_t)p->N * p->L * kD : nullptr;
    float* const h[5] = {s0, s1, s0, s1, nullptr};
    return run_forward(a, h, (hipStream_t)stream);
}

int sg3_latent_mapper_train_forward(const sg3_latent_mapper_train_params* p, void* stream) {
    using namespace sg3;
    const char* who = "latent_mapper_train_forward";
    SG3_REQUIRE(p, "%s: null params", who);
    SG3_REQUIRE(p->x && p->delta, "%s: null x or delta", who);
    if (int rc = check_shape(who, p->N, p->L, p->D, p->groups, p->levelBegin, p->levelEnd)) return rc;
    const size_t act = (size_t)p->N * p->L * kD * sizeof(float);
    const size_t wb = (size_t)p->groups * 4 * kD * kD * sizeof(float), bb = (size_t)p->groups * 4 * kD * sizeof(float);
    if (p->groups > 0) {
        SG3_REQUIRE(p->weight && p->bias && p->acts, "%s: null weight, bias or acts", who);
        SG3_REQUIRE(((uintptr_t)p->weight & 15) == 0 && ((uintptr_t)p->acts & 15) == 0 && ((uintptr_t)p->delta & 15) == 0,
                    "%s: weight, acts and delta must be 16-byte aligned", who);
    }
    const void* bufs[6] = {p->x, p->out, p->delta, p->groups ? p->acts : nullptr, p->groups ? p->weight : nullptr, p->groups ? p->bias : nullptr};
    const size_t sizes[6] = {act, act, act, 4 * act, wb, bb};
    for (int i = 1; i < 4; i++)                    // written buffers overlap nothing else
        for (int j = 0; j < 6; j++)
            SG3_REQUIRE(i == j || !overlaps(bufs[i], sizes[i], bufs[j], sizes[j]), "%s: buffers %d and %d overlap", who, i, j);

    MapperLaunch a = {};
    a.x = p->x; a.weight = p->weight; a.bias = p->bias; a.out = p->out; a.delta = p->delta;
    a.N = p->N; a.L = p->L; a.G = p->groups; a.alpha = p->alpha;
    a.tileStart[0] = 0;
    for (int g = 0; g < p->groups; g++) {
        a.begin[g] = p->levelBegin[g]; a.end[g] = p->levelEnd[g];
        a.tileStart[g + 1] = a.tileStart[g] + ceil_div(p->N * (a.end[g] - a.begin[g]), kTile) * kColBlocks;
    }
    const size_t n = (size_t)p->N * p->L * kD;
    float* const h[5] = {p->acts, p->groups ? p->acts + n : nullptr, p->groups ? p->acts + 2 * n : nullptr, p->groups ? p->acts + 3 * n : nullptr, nullptr};
    return run_forward(a, h, (hipStream_t)stream);
}

int sg3_latent_mapper_backward(const sg3_latent_mapper_backward_params* p, void* stream) {
    using namespace sg3;
    const char* who = "latent_mapper_backward";
    SG3_REQUIRE(p, "%s: null params", who);
    SG3_REQUIRE(p->x, "%s: null x", who);
    if (int rc = check_shape(who, p->N, p->L, p->D, p->groups, p->levelBegin, p->levelEnd)) return rc;
    SG3_REQUIRE((p->dW != nullptr) == (p->dB != nullptr), "%s: dW and dB are given together or not at all", who);
    const bool wantW = p->groups > 0 && p->dW;
    SG3_REQUIRE(p->dx || wantW, "%s: nothing to compute (no dx, and no dW / dB of a group)", who);
    const size_t act = (size_t)p->N * p->L * kD * sizeof(float);
    const size_t wb = (size_t)p->groups * 4 * kD * kD * sizeof(float), bb = (size_t)p->groups * 4 * kD * sizeof(float);
    if (p->groups > 0) {
        SG3_REQUIRE(p->dDelta || p->dOut, "%s: neither dDelta nor dOut is given", who);
        SG3_REQUIRE(p->weight && p->acts && p->delta && p->scratch, "%s: null weight, acts, delta or scratch", who);
        SG3_REQUIRE(((uintptr_t)p->weight & 15) == 0 && ((uintptr_t)p->acts & 15) == 0 && ((uintptr_t)p->delta & 15) == 0 && ((uintptr_t)p->scratch & 15) == 0,
                    "%s: weight, acts, delta and scratch must be 16-byte aligned", who);
    }
    const bool on = p->groups > 0;
    // written: dx, dW, dB, scratch; read: x, weight, acts, delta, dDelta, dOut
    const void* bufs[10] = {p->dx, wantW ? p->dW : nullptr, wantW ? p->dB : nullptr, on ? p->scratch : nullptr,
                            p->x, on ? p->weight : nullptr, on ? p->acts : nullptr, on ? p->delta : nullptr, on ? p->dDelta : nullptr, p->dOut};
    const size_t sizes[10] = {act, wb, bb, 2 * act, act, wb, 4 * act, act, act, act};
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 10; j++)
            SG3_REQUIRE(i == j || !overlaps(bufs[i], sizes[i], bufs[j], sizes[j]), "%s: buffers %d and %d overlap", who, i, j);

    MapperBwdLaunch a = {};
    a.x = p->x; a.weight = p->weight; a.acts = p->acts; a.delta = p->delta; a.dDelta = p->dDelta; a.dOut = p->dOut;
    a.dx = p->dx; a.dW = p->dW; a.dB = p->dB;
    a.N = p->N; a.L = p->L; a.G = p->groups; a.alpha = p->alpha;
    a.tileStart[0] = 0;
    for (int g = 0; g < p->groups; g++) {
        a.begin[g] = p->levelBegin[g]; a.end[g] = p->levelEnd[g];
        a.tileStart[g + 1] = a.tileStart[g] + ceil_div(p->N * (a.end[g] - a.begin[g]), kTile) * kColBlocks;
        for (int w = 0; w < 4; w++) { a.wScale[4 * g + w] = p->wScale[4 * g + w]; a.bScale[4 * g + w] = p->bScale[4 * g + w]; }
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 perSample((unsigned)ceil_div(p->N * kD, 256));
    if (on) {
        float* cur = p->scratch;
        float* other = p->scratch + (size_t)p->N * p->L * kD;
        a.dst = cur;
        hipLaunchKernelGGL(dz4_kernel, dim3((unsigned)ceil_div(p->N * p->L * kD, 256)), dim3(256), 0, st, a);
        SG3_LAUNCH_CHECK("latent_mapper dz4_kernel");
        for (int w = 3; w >= 0; w--) {
            a.layer = w;
            a.dz = cur;
            if (wantW) {
                hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)(p->groups * kColBlocks * kColBlocks)), dim3(256), 0, st, a);
                SG3_LAUNCH_CHECK("latent_mapper wgrad_kernel");
            }
            if (w == 0 && !p->dx) break;
            a.dst = other;
            if (w > 0) hipLaunchKernelGGL(dgrad_kernel<false>, dim3((unsigned)a.tileStart[p->groups]), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(dgrad_kernel<true>, dim3((unsigned)a.tileStart[p->groups]), dim3(256), 0, st, a);
            SG3_LAUNCH_CHECK("latent_mapper dgrad_kernel");
            float* t = cur; cur = other; other = t;
        }
        a.dz = cur;       // dh0
    }
    if (p->dx) {
        hipLaunchKernelGGL(pixelnorm_bwd_kernel, perSample, dim3(256), 0, st, a);
        SG3_LAUNCH_CHECK("latent_mapper pixelnorm_bwd_kernel");
    }
    return SG3_OK;
}

} // extern "C"
