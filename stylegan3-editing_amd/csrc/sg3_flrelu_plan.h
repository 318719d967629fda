// sg3_flrelu_plan.h -- which kernel, how many launches and what grid a filtered_lrelu call takes: ONE pure host function,
// plan_filtered_lrelu, shared by the launch (sg3_filtered_lrelu), the older host queries (sg3_filtered_lrelu_planes_per_wave,
// sg3_filtered_lrelu_stream_grid) and the read-only ABI query (sg3_filtered_lrelu_dispatch, which tests read without a GPU).
// plan_filtered_lrelu makes no HIP runtime call and follows no pointer.  StreamCfg holds the tile constants the streaming kernel and
// the plan both read.
#pragma once
#include "sg3_common.h"
#include <cmath>
#include <cstdlib>

namespace sg3 {

template <int U, int D> struct StreamCfg {
    static constexpr int FU = 6 * U, FD = 6 * D;
    static constexpr int CPL = 4;                       // upsampled columns per lane
    static constexpr int GROUPS = CPL / U;              // column groups per lane that share one input window
    static constexpr int IWS = GROUPS * 64 + 6;         // input samples a wave needs per row (+ slack)
    static constexpr int NL = (IWS + 63) / 64;          // global loads per lane per row
    static constexpr int SIN = NL * 64;                 // LDS floats for the input row
    static constexpr int SOUT = 4 + 256 + 32;           // LDS floats for the output row (+ read-ahead of the last lanes)
    static constexpr int MAXTW = (256 - FD) / D;        // output columns a wave's 256 upsampled columns can complete
    // packed mode (two narrow planes per wave, 32 lanes each): input-row / output-row LDS segment of one plane, and the widest
    // output 32 lanes complete
    static constexpr int PSEG = GROUPS * 32 + 8;        // 72 (up 2) | 40 (up 4) input samples; 2 PSEG <= SIN
    static constexpr int POSEG = 4 * 32 + 16;           // 144 floats; 2 POSEG <= SOUT
    // output column 2l + 1 reads the exchanged row up to slot 4 + 4l + 13, and the 32 lanes write slots 4 - delta .. 131 - delta
    // (delta <= 3): l <= 26
    static constexpr int PACKTW = 2 * 27;               // 54 output columns (down 2)
    static_assert(2 * PSEG <= SIN && 2 * POSEG <= SOUT, "packed LDS rows fit the unpacked ones");
};

// The plan IS the struct the ABI query hands out (include/sg3_ops.h): kind of launch, the template coordinates and the work
// decomposition of up to two launches
typedef sg3_filtered_lrelu_dispatch_info FlreluPlan;

// The A/B switches of the plan
struct FlreluKnobs {
    bool pack = true;            // SG3_FLRELU_NOPACK=1 clears it: one plane per wave everywhere (A/B timing; read ONCE per process)
    bool fastAct = true;         // SG3_FLRELU_SLOWACT=1 clears it: lrelu + clamp everywhere (A/B timing and the parity tests; read on EVERY
                                 // call, so that a test can compare both forms in one process)
    static FlreluKnobs env() {
        static const bool pack = [] { const char* e = getenv("SG3_FLRELU_NOPACK"); return !(e && e[0] == '1'); }();
        const char* e = getenv("SG3_FLRELU_SLOWACT");
        FlreluKnobs v;
        v.pack = pack;
        v.fastAct = !(e && e[0] == '1');
        return v;
    }
};

static bool stream_supported(int up, int down, int fuW, int fuH, int fdW, int fdH) {
    if (fuH == 12) {
        // adjoint of the radial (config R) layers: 12x12 up filter, up 2, separable down 2 (12 taps) or 4 (24 taps)
        return up == 2 && fuW == 12 && fdH == 0 && ((down == 2 && fdW == 12) || (down == 4 && fdW == 24));
    }
    if (fuH != 0) return false;                               // otherwise a separable up filter
    if (fdH != 0 && fdH != 12) return false;                  // separable, or full 12x12 (radial) down filter
    if (down == 2 && fdW == 12) return (up == 2 && fuW == 12) || (up == 4 && fuW == 24);
    // adjoint of the up-4 layers: up 2 (12 taps), down 4 (24 taps), separable
    return down == 4 && fdW == 24 && fdH == 0 && up == 2 && fuW == 12;
}

// the streaming kernel evaluates lrelu as max(v, slope * v), valid for 0 <= slope <= 1 (every StyleGAN3 layer)
static bool stream_params_ok(const sg3_filtered_lrelu_params& q) {
    if (q.fdH != 0 && ((uintptr_t)q.fd & 15) != 0) return false;  // 2-D taps are fetched as 16-byte scalar quads
    if (q.fuH != 0 && (((uintptr_t)q.fu & 15) != 0 || !q.readSigns)) return false;       // 2-D up filter: adjoint passes only
    const bool signs = q.writeSigns || q.readSigns;
    if (signs && (!q.s || q.sH <= 0 || q.sWbytes <= 0)) return false;
    if (q.readSigns && q.fdH != 0) return false;                                          // adjoint passes: separable down filter
    if (q.readSigns && q.up != 2) return false;                                            // adjoint passes upsample by 2
    if (q.down == 4 && !q.readSigns) return false;                                         // down 4 exists for the adjoint only
    return q.slope >= 0.f && q.slope <= 1.f && q.xStride[3] == 1 && q.yStride[3] == 1 && !(q.clamp < 0.f);
}

static bool pointwise_supported(int up, int down, int fuW, int fuH, int fdW, int fdH) {
    return up == 1 && down == 1 && fuW == 1 && fdW == 1 && fuH <= 1 && fdH <= 1;
}

// Work decomposition of the streaming kernel: strips of equal width, as wide as a wave's 256 upsampled columns can complete
// (120 for down 2, 58 for down 4); row chunks: enough waves to fill 256 CUs x 16 waves a few times over, but chunks tall
// enough that the 11-row warm-up stays small.
static void stream_grid(int N, int C, int yH, int yW, int down, int& nStrips, int& TW, int& nChunks, int& CH) {
    const int maxTW = down == 2 ? StreamCfg<2, 2>::MAXTW : StreamCfg<2, 4>::MAXTW;
    nStrips = ceil_div(yW, maxTW);
    TW = ceil_div(yW, nStrips);
    const long long planes = (long long)N * C;
    const long long wantWaves = 256LL * 16 * 4;
    int n = (int)ceil_div64(wantWaves, planes * nStrips);
    const int maxChunks = max(1, yH / 48);
    if (n > maxChunks) n = maxChunks;
    if (n < 1) n = 1;
    CH = ceil_div(yH, n);
    nChunks = ceil_div(yH, CH);
}

// Two planes per wave (packed mode of the streaming kernel) for the plain forward on strips at most `width` columns wide: dense
// (n, c) planes (the second plane of a wave sits one channel stride after the first), offsets inside a 2 GB descriptor.
static bool stream_packs_planes(const sg3_filtered_lrelu_params& q, int width, const FlreluKnobs& knobs) {
    const long long esz = q.dtype == SG3_F32 ? 4 : 2;
    const long long xsC = q.xStride[1], ysC = q.yStride[1];
    return knobs.pack && !q.readSigns && !q.writeSigns && q.down == 2 && width <= StreamCfg<2, 2>::PACKTW &&
           q.xStride[0] == (long long)q.C * xsC && q.yStride[0] == (long long)q.C * ysC && xsC > 0 && ysC > 0 &&
           (xsC + q.xW) * esz < 0x7fffffffLL && (ysC + q.yW) * esz < 0x7fffffffLL;
}

// The one-instruction activation of the plain forward (StreamParams.fastAct): for a finite positive gain and a clamp that is a number.
static bool stream_fast_activation(const sg3_filtered_lrelu_params& q, const FlreluKnobs& knobs) {
    return knobs.fastAct && !q.readSigns && !q.writeSigns && q.gain > 0.f && q.gain < INFINITY && q.clamp >= 0.f;
}

// The up-4 separable plain forward has two forms that compute the same thing bit for bit: the default (up taps placed by hand, at
// most 128 VGPRs, four waves per SIMD) and the earlier one (`Stream`'s WIDE), taken where the process setting asks for it
static bool stream_up4_wide(const sg3_filtered_lrelu_params& q, int up4WideSetting) {
    return q.up == 4 && q.fdH == 0 && !q.readSigns && !q.writeSigns && up4WideSetting != 0;
}

// width of the full strips when a row is cut into full strips + a packed remainder, and their number (0: equal strips instead --
// no remainder, a remainder too wide to pack, or more waves than equal strips take)
constexpr int STREAM_FULL_TW = 120;
static int stream_full_strips(int yW, int nStripsEqual) {
    const int nFull = (yW - 1) / STREAM_FULL_TW, rem = yW - nFull * STREAM_FULL_TW;
    return (nFull >= 1 && nFull + 1 == nStripsEqual && rem <= StreamCfg<2, 2>::PACKTW) ? nFull : 0;
}

// The plan of one call whose dtype is fp32 / fp16 and whose N, C, yH, yW are positive.  Of the pointers it reads only whether s is
// there and the alignment of 2-D taps.  `up4WideSetting`: sg3_filtered_lrelu_force_up4_wide's setting.
// kind == SG3_FLRELU_NONE: no fused kernel.  kind == SG3_FLRELU_STREAM with launches == 0: the grid does not fit 2^31 - 1 workgroups
// (planesPerWave and the decomposition are filled in all the same).
static inline FlreluPlan plan_filtered_lrelu(const sg3_filtered_lrelu_params& q, const FlreluKnobs& knobs, int up4WideSetting) {
    FlreluPlan pl = {};
    pl.kind = SG3_FLRELU_NONE;
    const bool signs = q.writeSigns || q.readSigns;
    if (!signs && pointwise_supported(q.up, q.down, q.fuW, q.fuH, q.fdW, q.fdH)) {
        pl.kind = SG3_FLRELU_POINTWISE;
        pl.launches = 1;
        long long blocks = ceil_div64((long long)q.N * q.C * q.yH * q.yW, 256);
        if (blocks > 256 * 16) blocks = 256 * 16;
        pl.totalBlocks[0] = (int)blocks;
        return pl;
    }
    if (!(stream_supported(q.up, q.down, q.fuW, q.fuH, q.fdW, q.fdH) && stream_params_ok(q))) return pl;
    pl.kind = SG3_FLRELU_STREAM;
    pl.fastAct = stream_fast_activation(q, knobs) ? 1 : 0;
    int nStrips, TW;
    stream_grid(q.N, q.C, q.yH, q.yW, q.down, nStrips, TW, pl.nChunks, pl.chunkRows);
    const long long planes = (long long)q.N * q.C;
    const long long total = planes * nStrips * pl.nChunks;
    const long long packedBlocks = (planes + 1) / 2 * pl.nChunks;          // two planes per wave, one strip

    const bool packed = nStrips == 1 && stream_packs_planes(q, q.yW, knobs);    // the 36^2 .. 52^2 layers
    // Rows a little wider than a whole number of full strips (148 = 120 + 28, 276 = 2 x 120 + 36, 532 = 4 x 120 + 52 columns: the
    // 148^2 .. 532^2 layers): equal strips would leave 40 .. 57 of a wave's 64 lanes at work.  Instead the full-width strips go
    // first, one plane per wave, and the remainder strip follows in a second launch with two planes per wave:
    // nFull + 1/2 waves per plane and row chunk instead of nFull + 1.
    const int remFull = stream_full_strips(q.yW, nStrips);
    const bool mixed = !packed && remFull > 0 && stream_packs_planes(q, q.yW - remFull * STREAM_FULL_TW, knobs);
    // ONE launch of the two-plane kernel, whose first blocks take the full strips, where it holds as many waves per SIMD as the
    // one-plane kernel (separable: 120 / 124 registers at up 2, 104 / 111 at up 4 -- 142 / 147 in the WIDE form; 12x12 down filter at up 4: 153 .. 160 against
    // 148 .. 156, three waves either way).  12x12 down filter at up 2: two launches (135 registers against 128: three waves, not four)
    const bool oneLaunch = mixed && (q.fdH == 0 || q.up == 4);
    pl.planesPerWave = packed ? 2 : mixed ? 3 : 1;
    pl.sumSlots = q.readSigns ? nStrips * pl.nChunks : 0;

    // template coordinates: the same for both launches but G
    const int vph = (((q.py0 - (q.up - 1)) % q.down) + q.down) % q.down;
    int radial;
    if (q.readSigns) radial = q.fuH == 0 ? 0 : (q.flip ? 4 : 3);             // separable | 12x12 up filter | the same, flipped
    // separable | 12x12 | 12x12 flipped | 12x12 with mirror-symmetric rows | the same, flipped
    else radial = q.fdH == 0 ? 0 : (q.fdMirror ? (q.flip ? 6 : 5) : (q.flip ? 2 : 1));
    auto kernel = [&](int i, int G) {
        pl.U[i] = q.up; pl.D[i] = q.down; pl.VPH[i] = vph; pl.RADIAL[i] = radial; pl.G[i] = G;
        pl.SIGNS[i] = q.readSigns ? 2 : q.writeSigns ? 1 : 0;
        pl.WIDE[i] = stream_up4_wide(q, up4WideSetting) ? 1 : 0;
    };
    // launch 0: equal strips | one packed strip | the full strips (one launch: followed by the remainder's two-plane blocks)
    kernel(0, (packed || oneLaunch) ? 2 : 1);
    pl.nStrips[0] = mixed ? remFull : nStrips;
    pl.TW[0] = mixed ? STREAM_FULL_TW : TW;
    const long long fullBlocks = planes * remFull * pl.nChunks;
    const long long blocks0 = packed ? packedBlocks : !mixed ? total : oneLaunch ? fullBlocks + packedBlocks : fullBlocks;
    if (total > 0x7fffffffLL || blocks0 > 0x7fffffffLL) return pl;       // launches == 0
    pl.totalBlocks[0] = (int)blocks0;
    pl.launches = 1;
    if (oneLaunch) { pl.wideBlocks[0] = (int)fullBlocks; pl.ox0Base[0] = remFull * STREAM_FULL_TW; }
    // launch 1 (two-launch mixed form): the remainder strip, two planes per wave
    if (mixed && !oneLaunch) {
        pl.launches = 2;
        kernel(1, 2);
        pl.nStrips[1] = 1; pl.ox0Base[1] = remFull * STREAM_FULL_TW; pl.TW[1] = q.yW - pl.ox0Base[1];
        pl.totalBlocks[1] = (int)packedBlocks;
    }
    return pl;
}

} // namespace sg3
