// sg3_modconv_plan.h -- which kernel, tile and grid a modulated-convolution call takes: ONE pure host function, plan_modconv,
// shared by the launch (sg3_modulated_conv2d), the scratch query (sg3_modconv_split_scratch_floats) and the read-only ABI query
// (sg3_modconv_dispatch, which tests read without a GPU).  plan_modconv makes no HIP runtime call and follows no pointer (the
// header it takes ConvK from, sg3_igemm_f32.h, also holds device helpers of the kernels).
#pragma once
#include "sg3_igemm_f32.h"
#include <algorithm>
#include <cstdlib>

#ifndef SG3_TAILPACK
#define SG3_TAILPACK 1          // 0 compiles the tap-packed tail chunk of the 3x3 kernel out (A/B builds)
#endif

namespace sg3 {

// K chunk of the packed fp32 weights per kernel size (modconv_mfma_kernel): ConvK, sg3_igemm_f32.h
static inline int packed_kc(int k) { return k == 3 ? ConvK<3>::KC : ConvK<1>::KC; }
// 16-channel chunks of the f16x3 packing; 1x1 kernels stage two chunks per step, so their count is padded to even
static inline int f16x3_chunks(int I, int k) { const int c = (I + 15) / 16; return k == 1 ? (c + 1) / 2 * 2 : c; }

constexpr int FLAT_NPIX = 512;                 // modconv_flat_kernel: patch pixels staged per chunk (two per thread)

// The A/B switches of the dispatch, read from the environment ONCE per process (ConvKnobs::env)
struct ConvKnobs {
    bool conv3Flat = true;       // SG3_CONV3_ROWS=1 clears it: the narrow 3x3 layers stay on the row-tile kernel
    int  flatSplits = 0;         // SG3_FLAT_SPLITS: 1 = never split K, 2 .. 4 = always; 0 = by grid size
    bool tallF16 = true;         // SG3_CONV_F16_ROWS4=1 clears it: the plain fp16 3x3 form keeps four rows per wave
    bool conv1M16 = true;        // SG3_CONV1_MFMA32=1 clears it: the 1x1 kernels take the 32x32x16 form
    int  f23Rows = 0;            // SG3_F23_TN (4 | 5 | 7): seeds the forced rows per wave of the transform-domain kernel
                                 // (sg3_modconv_f23_force_rows owns the value afterwards)
    static const ConvKnobs& env() {
        static const ConvKnobs k = [] {
            auto is1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
            auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
            ConvKnobs v;
            v.conv3Flat = !is1("SG3_CONV3_ROWS");
            v.flatSplits = num("SG3_FLAT_SPLITS");
            v.tallF16 = !is1("SG3_CONV_F16_ROWS4");
            v.conv1M16 = !is1("SG3_CONV1_MFMA32");
            const int r = num("SG3_F23_TN");
            v.f23Rows = (r == 4 || r == 5 || r == 7) ? r : 0;
            return v;
        }();
        return k;
    }
};

// The plan IS the struct the ABI query hands out (include/sg3_ops.h): kernel family, template coordinates, launch and reduce geometry
typedef sg3_modconv_dispatch_info ConvPlan;

// K splits of a flat-kernel call with `tiles` workgroups and `nch` K chunks: none when the grid gives every CU a workgroup; else up to
// four, at least four chunks each
static inline int flat_k_splits(long long tiles, int nch, int cus, int forced) {
    if (forced >= 1) return std::min(forced, std::min(4, nch));
    if (tiles >= cus) return 1;
    const int s = (int)std::min<long long>(std::min<long long>(4, (2LL * cus) / tiles), nch / 4);
    return s >= 2 ? s : 1;
}

// does the patch of every RUN-pixel piece of an outH x outW plane fit FLAT_NPIX pixels?  rows touched <= (RUN - 2) / outW + 2
static inline bool flat_fits(int outW, int run) { return ((run - 2) / outW + 2 + 2) * (outW + 2) <= FLAT_NPIX; }

// workgroups per sample of the ToRGB kernel (`vec`: four pixels per thread)
static inline int torgb_blocks(int HW, bool vec) { return std::min(ceil_div(vec ? HW / 4 : HW, 256), 2048); }

// The plan of one VALID call (sg3_modulated_conv2d's checks passed) on a device with `cus` CUs.  Of the pointers it reads only
// whether dcoef, epilogueBias and splitScratch are there.  `f23ForcedRows`: sg3_modconv_f23_force_rows' setting (0 = cost model).
// family == SG3_MODCONV_NONE: the grid does not fit 2^31 - 1 workgroups.
static inline ConvPlan plan_modconv(const sg3_modconv_params& q, int cus, const ConvKnobs& knobs, int f23ForcedRows) {
    ConvPlan pl = {};
    pl.family = SG3_MODCONV_NONE;
    const int O = q.O;
    const int outH = q.H + 2 * q.pad - q.k + 1, outW = q.W + 2 * q.pad - q.k + 1;
    const long long elems = (long long)q.N * O * outH * outW;
    const bool fp32io = q.dtype == SG3_F32;
    pl.outPitch = q.outRowStride > 0 ? q.outRowStride : outW;
    pl.kSplits = 1; pl.gridY = 1; pl.block = 256;
    // grid = one workgroup per (tile, K split); false when that passes 2^31 - 1
    auto tiled = [&](int family) {
        const long long total = (long long)pl.xTiles * pl.yTiles * pl.mTiles * q.N * pl.kSplits;
        if (total > 0x7fffffffLL) return false;
        pl.totalBlocks = pl.gridX = (int)total;
        pl.reduceGrid = pl.kSplits > 1 ? (int)std::min<long long>((elems + 255) / 256, 4096) : 0;
        pl.family = family;
        return true;
    };
    // a split must fit the scratch on offer and a 32-bit grid
    auto split_fits = [&](int ksp, long long tiles) {
        return ksp > 1 && q.splitScratch && (long long)ksp * elems <= q.splitScratchFloats && (long long)ksp * tiles <= 0x7fffffffLL;
    };

    if (q.precision == SG3_CONV_F16X3_F23 || q.precision == SG3_CONV_F16_F23) {
        // rows per wave: one workgroup per CU, so the time goes with (rounds of 256 workgroups) x (rows per wave + per-chunk overhead)
        const long long per = (long long)q.N * ceil_div(O, 64) * ceil_div(outW, 32);
        int best = 7; double bestCost = 1e300;
        const int cands[3] = {7, 5, 4};
        for (int c = 0; c < 3; c++) {
            const int tn = cands[c];
            const long long wgs = per * ceil_div(outH, 2 * tn);
            const double rounds = wgs <= 1024 ? (double)ceil_div64(wgs, 256) : wgs / 256.0;
            const double cost = rounds * (tn + 0.6);
            if (cost < bestCost * 0.999) { bestCost = cost; best = tn; }
        }
        if (f23ForcedRows == 4 || f23ForcedRows == 5 || f23ForcedRows == 7) best = f23ForcedRows;      // tests, A/B timing
        pl.WM = 2; pl.WN = 4; pl.TM = 1; pl.TN = best; pl.SPLIT = fp32io;          // wave = (M block, transform point); TN rows x 2 row groups
        pl.nch = ceil_div(q.I, 16);
        pl.xTiles = ceil_div(outW, 32); pl.yTiles = ceil_div(outH, 2 * best); pl.mTiles = ceil_div(O, 64);
        const int imageBytes = 2 * (fp32io ? 16 : 8) * (2 * best + 2) * 256;
        pl.ldsBytes = std::max(imageBytes, 65536);               // double-buffered B image, at least the 64 KB exchange area
        pl.block = 512;
        if (!tiled(SG3_MODCONV_F23)) return pl;
#ifndef SG3_F23_ONE_TILE
        pl.gridX = (int)std::min<long long>(pl.totalBlocks, cus);        // one resident workgroup per CU walks the tiles
#endif
        return pl;
    }

    if (q.precision == SG3_CONV_F16X3 || q.precision == SG3_CONV_F16) {
        pl.SPLIT = q.precision == SG3_CONV_F16X3;
        if (q.k == 1) {
            // every staged input element is used once per output-channel tile, so the tile is as tall as the channel padding
            // allows: 256 rows (1024 -> 1024 @ 148^2 x 4: 0.88 ms against 1.05 ms with 128 rows and 1.25 ms with 64)
            // Few K stages (I <= 256: the 532^2 and 1044^2 layers of config R): HBM-bound, and ONE resident workgroup (100 KB of
            // double-buffered LDS) leaves the CU waiting on memory at the start and end of every tile.  These layers take the
            // 64-row tile with a single LDS image (42 KB, 110 registers): two workgroups per CU.  Measured at R-1024, batch 8:
            // L10 256->161 1232 -> 1099 us, L11 161->102 2600 -> 2358, L12 102->64 1373 -> 1103, L13 64->64 945 -> 808 (5.5 TB/s).
            // The 128-row tile needs 174 registers and spills under the two-workgroup bound.
            const bool thin = q.I <= 256;
            const int t128 = ceil_div(O, 128) * 128, t256 = ceil_div(O, 256) * 256;
            pl.NBUF = thin ? 1 : 2;
            if (thin || O <= 64) { pl.WM = 1; pl.WN = 8; pl.TM = 2; pl.TN = 1; }          //  64 x 256 pixels (thin: two workgroups per CU)
            else if (t256 <= t128) { pl.WM = 2; pl.WN = 4; pl.TM = 4; pl.TN = 2; }        // 256 x 256 pixels
            else { pl.WM = 2; pl.WN = 4; pl.TM = 2; pl.TN = 2; }                          // 128 x 256 pixels
            // the 16x16x32 form for the compute-bound tiles (R-1024, batch 8: 28.4 vs 32.2 ms over the 1024 .. 406-channel layers); the
            // thin HBM-bound layers keep 32x32x16: its stores are 128-byte row segments, the 16-wide blocks' 64-byte ones cost them 5 %
            pl.M16 = pl.NBUF == 2 && knobs.conv1M16;
            const int BM = pl.WM * pl.TM * 32, ROWS = pl.WN * pl.TN;
            pl.ldsBytes = pl.NBUF * (BM * (2 * 32 + 8) + (pl.SPLIT ? 8 : 4) * ROWS * 32 * 8) * 2;
            pl.block = 512;
            pl.nch = f16x3_chunks(q.I, 1) / 2;                  // stages of 32 channels
            pl.xTiles = ceil_div(q.H * q.W, ROWS * 32); pl.yTiles = 1; pl.mTiles = ceil_div(O, BM);     // flat 256-pixel tiles
            const long long total = (long long)pl.xTiles * pl.mTiles * q.N;
            // K split.  Precondition (what the scratch query has always required, so what every caller that sizes its scratch by the
            // query gets): fp32 tensors, more than 4 output channels, at least 8 stages of 32 channels and fewer than a quarter of a
            // 256-row tile per CU -- or SG3_FLAT_SPLITS >= 2.
            const long long P1 = (long long)q.H * q.W;
            const long long tiles1 = (long long)q.N * ceil_div(O, 256) * ceil_div((int)std::min<long long>(P1, 0x7fffffff), 256);
            const bool gate = fp32io && q.pad == 0 && O > 4 && (knobs.flatSplits >= 2 || (4 * tiles1 < cus && ceil_div(q.I, 32) >= 8));
            if (gate) {
                // this kernel's workgroups are eight waves with two resident per CU: measured neutral from ~100 tiles up (R-1024 batch 4: 15.1 vs
                // 15.0 ms), +1.7 % at 48, +5.6 % at 24 -- so it splits below a quarter of a tile per CU
                const int ksp = flat_k_splits(4 * total, pl.nch, cus, knobs.flatSplits);
                if (split_fits(ksp, total)) pl.kSplits = ksp;
            }
            tiled(SG3_MODCONV_GEMM1);
            return pl;
        }
        // Two row-streaming tiles, two workgroups per CU each.  The 64-channel tile stages the patch once for twice the
        // channels; the 32-channel tile pads the channel count less.  Measured at FFHQ-1024 (batch 8): O = 81 (96 vs 128
        // padded rows) 1.76 vs 2.10 ms, O = 203 (224 vs 256) 2.40 vs 2.54 ms, O = 323 (352 vs 384) 1.86 vs 1.77 ms: the
        // small tile wins when it saves at least ~10 % of the rows.
        const int t32 = ceil_div(O, 32) * 32, t64 = ceil_div(O, 64) * 64;
        // last K chunk with 1..4 channels (and at least one full chunk before it): the kernel packs its taps (PACK)
        const bool pack = SG3_TAILPACK && q.I > 16 && q.I % 16 >= 1 && q.I % 16 <= 4;
        // The plain fp16 form (one MFMA per K step) reads 0.75 LDS fragments per MFMA with four rows per wave -- LDS-bandwidth bound,
        // where the split form (0.5 per MFMA, three MFMAs per fragment pair) is not: its waves take taller stacks of rows (six: 0.61; five in the 32-channel tile: 0.67; eight rows spill).
        // SG3_CONV_F16_ROWS4=1 keeps four rows (A/B timing).
        const bool tall = !pl.SPLIT && knobs.tallF16 && outH >= 128;
        pl.nch = ceil_div(q.I, 16);
        auto rows = [&](int wm, int wn, int tn, bool pk) {
            pl.WM = wm; pl.WN = wn; pl.TM = 1; pl.TN = tn; pl.PACK = pk;
            const int BM = wm * 32, ROWS = wn * tn, PH = ROWS + 2, PW = 34;
            pl.ldsBytes = (BM * (9 * 32 + 8) + (pl.SPLIT ? 4 : 2) * PH * PW * 8) * 2;
            pl.xTiles = ceil_div(outW, 32); pl.yTiles = ceil_div(outH, ROWS); pl.mTiles = ceil_div(O, BM);
            tiled(SG3_MODCONV_ROWS);
            return pl;
        };
        if (O <= 32 || t32 * 10 <= t64 * 9) return rows(1, 4, tall ? 5 : 4, pack);                     //  32 x (16 | 20 rows x 32)
        if (tall) return rows(2, 2, 6, pack);                                                          //  64 x (12 rows x 32)
        // Narrow outputs with 64-channel tiles: runs of the flattened plane instead of 32-column row pieces (modconv_flat_kernel) when
        // that takes fewer rounds x MFMA blocks per wave than the best row tile.  SG3_CONV3_ROWS=1 keeps the row kernel.
        if (!pack && (q.outRowStride == 0 || q.outRowStride == outW) && knobs.conv3Flat) {
            const long long perM = (long long)q.N * ceil_div(O, 64);
            // time ~ rounds of 512 resident workgroups x (blocks per wave + staging); large grids are not quantised
            auto cost = [](long long wgs, int tn) { return (wgs <= 2048 ? (double)ceil_div64(wgs, 512) : wgs / 512.0) * (tn + 0.5); };
            const long long perRow = perM * ceil_div(outW, 32);
            const double rowCost = std::min(cost(perRow * ceil_div(outH, 8), 4), cost(perRow * ceil_div(outH, 10), 5));
            int best = 0; double bestCost = rowCost * 0.9;                       // the row kernel reads less LDS per MFMA: flat must save 10 %
            for (int tn = 4; tn >= 2; tn--) {
                if (!flat_fits(outW, 64 * tn)) continue;
                const double c = cost(perM * ceil_div(outH * outW, 64 * tn), tn);
                if (c < bestCost) { bestCost = c; best = tn; }
            }
            if (best) {
                pl.WM = 2; pl.WN = 2; pl.TM = 1; pl.TN = best;                   // 64 channels x runs of 64 TN pixels
                pl.ldsBytes = (64 * (9 * 32 + 8) + (pl.SPLIT ? 4 : 2) * FLAT_NPIX * 8) * 2;      // <= 80 KB: two workgroups per CU
                pl.xTiles = ceil_div(outH * outW, 64 * best); pl.yTiles = 1; pl.mTiles = ceil_div(O, 64);
                pl.outPitch = outW;
                const long long total = (long long)pl.xTiles * pl.mTiles * q.N;
                // K split.  Precondition (what the scratch query has always required, see the 1x1 form): dcoef present, rows of at most
                // 128 pixels, at least 8 chunks of 16 channels and fewer workgroups than CUs even with the smallest flat tile -- or
                // SG3_FLAT_SPLITS >= 2.
                const long long tiles = (long long)q.N * ceil_div(O, 64) * ceil_div(outH * outW, 128);
                const bool gate = q.dcoef && outW <= 128 && (knobs.flatSplits >= 2 || (tiles < cus && pl.nch >= 8));
                if (gate) {
                    const int ksp = flat_k_splits(total, pl.nch, cus, knobs.flatSplits);
                    if (split_fits(ksp, total)) pl.kSplits = ksp;
                }
                tiled(SG3_MODCONV_FLAT);
                return pl;
            }
        }
        if (!pack) {
            // Small grids (the 36^2 .. 52^2 layers): 512 workgroups are resident at once, so the time goes with the number of
            // ROUNDS times the rows a workgroup computes.  Ten-row tiles turn the 640 workgroups of a 38-row output (8 images
            // x 8 channel tiles x 2 x 5) into exactly 512: one round of 5 rows per wave instead of two rounds of 4.
            const long long per = (long long)q.N * ceil_div(O, 64) * ceil_div(outW, 32);
            const long long wg8 = per * ceil_div(outH, 8), wg10 = per * ceil_div(outH, 10);
            if (wg8 <= 2048 && ceil_div64(wg10, 512) * 5 < ceil_div64(wg8, 512) * 4) return rows(2, 2, 5, false);      //  64 x (10 rows x 32)
        }
        return rows(2, 2, 4, pack);                                                                                   //  64 x (8 rows x 32)
    }

    // exact fp32 products
    if (q.k == 1 && q.pad == 0 && O <= 4 && (size_t)q.I * 4 * sizeof(float) <= 48 * 1024) {
        // ToRGB: HBM-bound, no matrix cores; four pixels per thread when the plane allows (the launch falls back to one for
        // tensors off a 16-byte boundary and takes torgb_blocks(HW, false) workgroups per sample then)
        const int HW = q.H * q.W;
        pl.nch = ceil_div(q.I, ConvK<1>::KC);
        pl.xTiles = pl.yTiles = pl.mTiles = 1;
        pl.gridX = torgb_blocks(HW, HW % 4 == 0); pl.gridY = q.N;
        pl.ldsBytes = q.I * 4 * (int)sizeof(float);
        pl.family = SG3_MODCONV_TORGB;
        return pl;
    }
    {
        // M tile from the channel count: the smallest BM in {32,64,96,128} that wastes the least of the last tile
        int best = 128; double bestEff = 0.0;
        const int cands[4] = {128, 96, 64, 32};
        for (int c = 0; c < 4; c++) {
            const int bm = cands[c];
            const double eff = (double)O / (double)(ceil_div(O, bm) * bm);
            if (eff > bestEff + 1e-9) { bestEff = eff; best = bm; }
        }
        switch (best) {
            case 128: pl.WM = 2; pl.WN = 2; pl.TM = 2; pl.TN = 2; break;
            case 96:  pl.WM = 1; pl.WN = 4; pl.TM = 3; pl.TN = 1; break;
            case 64:  pl.WM = 1; pl.WN = 4; pl.TM = 2; pl.TN = 2; break;
            default:  pl.WM = 1; pl.WN = 4; pl.TM = 1; pl.TN = 4; break;
        }
        pl.nch = ceil_div(q.I, packed_kc(q.k));
        pl.xTiles = ceil_div(outW, 32); pl.yTiles = ceil_div(outH, pl.WN * pl.TN); pl.mTiles = ceil_div(O, best);
        tiled(SG3_MODCONV_FP32_MFMA);
        return pl;
    }
}

// the parameter-block fields every convolution kernel shares (ConvParams, F23Params)
template <typename P>
static inline void fill_params(P& p, const sg3_modconv_params& q, const ConvPlan& pl) {
    p.x = q.x; p.wp = q.wPacked; p.sIn = q.sIn; p.dcoef = q.dcoef; p.out = q.out;
    p.N = q.N; p.I = q.I; p.O = q.O; p.H = q.H; p.W = q.W; p.pad = q.pad;
    p.outH = q.H + 2 * q.pad - q.k + 1; p.outW = q.W + 2 * q.pad - q.k + 1;
    p.nch = pl.nch; p.xTiles = pl.xTiles; p.yTiles = pl.yTiles; p.mTiles = pl.mTiles;
    p.totalBlocks = pl.totalBlocks; p.outPitch = pl.outPitch;
}

} // namespace sg3
