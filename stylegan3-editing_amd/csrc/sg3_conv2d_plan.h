// sg3_conv2d_plan.h -- which kernel, tile and grid a call of the encoder's plain convolutions takes: three pure host functions
// (no HIP runtime call, no pointer followed; sg3_igemm_f32.h, where ConvK comes from, also holds device helpers of the kernels), each
// shared by its launch (sg3_conv2d, sg3_conv2d_dgrad, sg3_conv2d_wgrad_sum), the older host queries (sg3_conv2d_form,
// sg3_conv2d_wgrad_sum_splits) and the read-only ABI queries (sg3_conv2d*_dispatch, which tests read without a GPU).  They plan calls
// that have passed the entry point's argument checks.
#pragma once
#include "sg3_igemm_f32.h"

namespace sg3 {

// The plan IS the struct the ABI queries hand out (include/sg3_ops.h).  totalBlocks == 0: the grid does not fit a launch.
typedef sg3_conv2d_dispatch_info Conv2dPlan;

// conv2d_wgrad_sum_kernel: output pixels per K chunk, 32 at stride 1, 16 at stride 2 (the staged input patch is then 34 / 33 columns
// wide either way)
__host__ __device__ constexpr int ws_px(int stride) { return 32 / stride; }
constexpr int WS_TILE = 64;         // output / input channels per workgroup
constexpr int WS_BLOCKS = 512;      // workgroups the planner aims for (two per CU of an MI355X)

// 32 WM TM channels x (WN TN rows x 32 columns) per workgroup, over rows x cols pixels of `channels` channels, `copies` times
static inline void plan_tiles(Conv2dPlan& pl, int WM, int WN, int TM, int TN, int channels, int rows, int cols, long long copies) {
    pl.WM = WM; pl.WN = WN; pl.TM = TM; pl.TN = TN;
    pl.xTiles = ceil_div(cols, 32); pl.yTiles = ceil_div(rows, WN * TN); pl.mTiles = ceil_div(channels, WM * TM * 32);
    const long long total = (long long)pl.xTiles * pl.yTiles * pl.mTiles * copies;
    pl.totalBlocks = total > 0x7fffffffLL ? 0 : (int)total; pl.block = 256;
}

// sg3_conv2d.  `cus` decides one thing: forms 4 and 5.
static inline Conv2dPlan plan_conv2d(const sg3_conv2d_params& q, int cus) {
    Conv2dPlan pl = {};
    pl.KS = q.k; pl.STRIDE = q.stride;
    pl.outH = (q.H + 2 * q.pad - q.k) / q.stride + 1; pl.outW = (q.W + 2 * q.pad - q.k) / q.stride + 1;
    if (q.precision == SG3_CONV_F16X3) {
        // 64 channels x (4 rows x 32 columns): forms 0 .. 3 (1x1 stride 2 | 1, the projection shortcuts; 3x3 stride 2; 3x3 stride 1 on maps
        // of at most 16 rows) and 4; form 5 is 64 x (8 rows x 32).
        // The 8-row tile (230 registers: two workgroups per CU) needs a grid that offers every CU its two workgroups; the 32 x 32 maps
        // of a 16-frame batch (14 units of the IR-SE50 trunk, 28 launches) give 256 eight-row tiles = ONE four-wave workgroup per CU
        // (counters, round 4: 0.85 waves per SIMD, matrix pipes 0.32 busy at 2.45 GHz -- latency, not power).  Such grids take the
        // 4-row tile instead (153 registers, three workgroups per CU): twice the workgroups, each with half the rows.
        const long long tiles8 = (long long)q.N * ceil_div(q.O, 64) * ceil_div(pl.outH, 8) * ceil_div(pl.outW, 32);
        const int f = q.k == 1 ? (q.stride == 2 ? 0 : 1) : q.stride == 2 ? 2 : pl.outH <= 16 ? 3 : tiles8 < 2 * (long long)cus ? 4 : 5;
        pl.family = SG3_CONV2D_F16X3; pl.form = SG3_CONV2D_FORM_F16X3 + f; pl.kc = 16;
        plan_tiles(pl, 1, 4, 2, f == 5 ? 2 : 1, q.O, pl.outH, pl.outW, q.N);
        // conv2d_f16x3_kernel's LDS in halfs: sA [BM][taps x (hi | lo) x 16 + 8], sB 4 planes (hi | lo x channel octet) of the [PH][PW][8] patch
        const int ph = (pl.WN * pl.TN - 1) * q.stride + q.k, pw = 31 * q.stride + q.k;
        pl.ldsBytes = (pl.WM * pl.TM * 32 * (q.k * q.k * 32 + 8) + 4 * ph * pw * 8) * (int)sizeof(_Float16);
    } else {
        // four accumulators per tile (SG3_CONV_FP32_CHAINS): the 64- and 32-channel tiles only.  One: small feature maps (16x16 and
        // below) get the 4-row tile, large ones the 128-channel tile when O allows
        const bool chains = q.precision == SG3_CONV_FP32_CHAINS;
        const int tile = (!chains && q.O >= 128 && pl.outH >= 8) ? 0 : q.O > 32 ? 1 : 2;
        pl.family = SG3_CONV2D_FP32_MFMA; pl.CHAINS = chains ? 4 : 1; pl.kc = q.k == 3 ? ConvK<3>::KC : ConvK<1>::KC;
        pl.form = chains ? 11 + tile : ((q.k == 3 ? 2 : 0) + (q.stride == 2 ? 1 : 0)) * 3 + tile;
        if (tile == 0) plan_tiles(pl, 2, 2, 2, 2, q.O, pl.outH, pl.outW, q.N);            // 128 x (4 rows x 32)
        else if (tile == 1) plan_tiles(pl, 2, 2, 1, 1, q.O, pl.outH, pl.outW, q.N);       // 64 x (2 rows x 32)
        else plan_tiles(pl, 1, 4, 1, 1, q.O, pl.outH, pl.outW, q.N);                      // 32 x (4 rows x 32)
    }
    pl.nch = ceil_div(q.I, pl.kc);
    return pl;
}

// sg3_conv2d_dgrad: 64 channels x (2 rows x 32 columns) of one parity class per workgroup; the stem (3 input channels) takes
// 32 x (4 rows x 32)
static inline Conv2dPlan plan_conv2d_dgrad(const sg3_conv2d_dgrad_params& q) {
    Conv2dPlan pl = {};
    pl.family = SG3_CONV2D_DGRAD; pl.form = -1; pl.KS = q.k; pl.STRIDE = q.stride; pl.outH = q.OH; pl.outW = q.OW;
    pl.kc = q.k == 3 ? ConvK<3>::KC : ConvK<1>::KC; pl.nch = ceil_div(q.O, pl.kc); pl.classes = q.stride * q.stride;
    const bool wide = q.I > 32;
    plan_tiles(pl, wide ? 2 : 1, wide ? 2 : 4, 1, 1, q.I, ceil_div(q.H, q.stride), ceil_div(q.W, q.stride), (long long)q.N * pl.classes);
    return pl;
}

// sg3_conv2d_wgrad_sum: the K chunks and their split over workgroup sets (the same for every device, so that results do not depend on
// the machine), the 64 x 64 (o, i) tiles and the reduce launch.  nChunks == 0: more than 2^31 - 1 chunks.
static inline Conv2dPlan plan_conv2d_wgrad_sum(const sg3_conv2d_wgrad_sum_params& q) {
    Conv2dPlan pl = {};
    pl.family = SG3_CONV2D_WGRAD_SUM; pl.form = -1; pl.KS = q.k; pl.STRIDE = q.stride;
    pl.outH = (q.H + 2 * (q.k / 2) - q.k) / q.stride + 1; pl.outW = (q.W + 2 * (q.k / 2) - q.k) / q.stride + 1;
    pl.xSegs = ceil_div(pl.outW, ws_px(q.stride));
    const long long chunks = (long long)q.N * pl.outH * pl.xSegs;
    if (chunks <= 0 || chunks > 0x7fffffffLL) return pl;
    pl.nChunks = (int)chunks; pl.oTiles = ceil_div(q.O, WS_TILE); pl.iTiles = ceil_div(q.I, WS_TILE);
    const long long tiles = (long long)pl.oTiles * pl.iTiles;
    long long want = WS_BLOCKS / tiles; if (want < 1) want = 1; if (want > chunks) want = chunks;
    pl.chunksPerSplit = (int)ceil_div64(chunks, want);
    pl.nSplit = ceil_div(pl.nChunks, pl.chunksPerSplit);          // no empty split
    pl.totalBlocks = tiles * pl.nSplit > 0x7fffffffLL ? 0 : (int)(tiles * pl.nSplit); pl.block = 256;
    pl.reduceGrid = pl.nSplit > 1 ? (int)ceil_div64((long long)q.O * q.I * q.k * q.k, 256) : 0;
    return pl;
}

} // namespace sg3
