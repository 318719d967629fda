// sg3_flrelu_kernels.h -- what the kernel file (sg3_filtered_lrelu.hip: the streaming kernel and its instantiations) and the host file
// (sg3_flrelu_host.hip: launchers, kernel lookup, C entry points) of filtered_lrelu share.  Only ordinary host functions cross that
// boundary: the kernel file takes its kernels' addresses itself and hands them out through `stream_kernel_leaf`.
#pragma once
#include "sg3_flrelu_plan.h"

namespace sg3 {

struct StreamParams {
    const void* x; void* y; const void* b; const float* fu; const float* fd;
    int C, xH, xW, yH, yW;
    int planes;                    // N * C
    long long xsN, xsC, xsH;      // element strides (innermost stride is 1)
    long long ysN, ysC, ysH;
    long long bStride;
    int px0, py0;
    int TW;                        // output columns per strip (<= 122)
    int ox0Base;                   // first output column of strip 0 (one-plane blocks) / of the packed strip (two-plane blocks)
    int wideBlocks;                // G = 2 kernels: the first wideBlocks (logical) blocks work on ONE plane each, strips of TW columns
                                   // from column 0; the others on two planes, columns ox0Base .. yW - 1
    int CH;                        // output rows per chunk
    int nStrips, nChunks;
    int totalBlocks;
    float gain, slope, clamp;
    int flip;
    int fastAct;                   // plain forward: 1 = try the one-instruction activation first (see `fast_threshold`), 0 = never
    float* ysum;                   // optional [N*C][nChunks*nStrips]: sum of this block's outputs (adjoint passes only: their bias gradient)
    float* ymax;                   // optional, same shape: max |output| of this block (adjoint passes only: the operand bound of the
                                   // convolution gradients that read the result next)
    unsigned char* s;              // sign tensor [N*C][sH][sWb] (2 bits per upsampled sample, 4 per byte), or null
    int sH, sWb, sx, sy;           // rows, bytes per row, offset of the upsampled buffer inside the sign tensor
#ifdef SG3_STAMPS
    unsigned long long* stamps;    // diagnostic build (tools/flrelu_clock.hip): per block {shader cycles, 100 MHz ticks} of the wave's life
#endif
};
#ifdef SG3_STAMPS
static unsigned long long* g_stamps = nullptr;
#endif

typedef void (*StreamKernel)(StreamParams);

// The kernels of one leaf of the lookup -- flrelu_stream_kernel<T, U, D, VPH, R, S, G, W> for VPH = 0 .. D - 1 -- or nullptr for a
// phase outside that range.  Defined by explicit instantiation in sg3_filtered_lrelu.hip, one per row of its part table; a leaf
// that no row names is a link error.
template <typename T, int U, int D, int R, int S, int G, int W> StreamKernel stream_kernel_leaf(int vph);

// Threshold of the one-instruction activation (plain forward).  The kernel forms every upsampled sample u from staged samples x
// (input + bias) through one phase of the separable up filter per direction, taps scaled by `up`: |u| <= hv * max |x| with
// hv = (up * max over phases of sum |f|)^2 (the phases map onto each other under flip).  For max |x| <= T, slope |u| <= clamp / gain
// holds -- with a 1e-4 margin over the rounding of the sums, of T and of u -- and |u| stays far below overflow.  -1: no fast path.
// Host and device run this same code (sg3_filtered_lrelu_fast_threshold exposes it to the CPU tests).
__host__ __device__ static inline float fast_threshold(const float* fu, int taps, int up, float gain, float slope, float clamp) {
    const float clampv = clamp / gain;                 // as the kernel forms it
    if (!(clampv > 0.f)) return -1.f;
    float hs = 0.f;
    for (int ph = 0; ph < up; ph++) {
        float s = 0.f;
        for (int k = ph; k < taps; k += up) s += fabsf(fu[k]);
        hs = fmaxf(hs, s);
    }
    hs *= (float)up;
    const float hv = hs * hs;
    return fminf(clampv / (slope * hv), 0x1p124f / fmaxf(hv, 1.f)) * 0.9999f;
}

} // namespace sg3
