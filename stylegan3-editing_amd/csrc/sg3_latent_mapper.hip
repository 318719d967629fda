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
    hipStream_t st = (hipStream_t)stream;
    a.dst = s0;
    hipLaunchKernelGGL(pixelnorm_kernel, dim3((unsigned)ceil_div(p->N * kD, 256)), dim3(256), 0, st, a);
    SG3_LAUNCH_CHECK("latent_mapper pixelnorm_kernel");
    if (p->groups == 0) return SG3_OK;
    const dim3 grid((unsigned)a.tileStart[p->groups]);
    for (int layer = 0; layer < 4; layer++) {
        a.layer = layer;
        a.in = (layer & 1) ? s1 : s0;
        a.dst = (layer & 1) ? s0 : s1;
        if (layer < 3) hipLaunchKernelGGL(layer_kernel<false>, grid, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(layer_kernel<true>, grid, dim3(256), 0, st, a);
        SG3_LAUNCH_CHECK("latent_mapper layer_kernel");
    }
    return SG3_OK;
}

} // extern "C"
