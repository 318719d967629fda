// sg3_igemm_f32.h -- what the MFMA implicit-GEMM convolution kernels (sg3_modconv.hip, sg3_conv2d.hip, sg3_conv2d_dgrad.hip) share
// on the device: the vector types, the K chunk of the packed fp32 weights, the XCD block renumbering and the C-layout row of an
// accumulator register.  The exact-fp32 main loop itself (modconv_mfma_kernel, conv2d_mfma_kernel, conv2d_dgrad_kernel) is NOT
// here: each kernel keeps its own copy, see DESIGN.md 3.3.1.  The host-side plan of the encoder convolutions (sg3_conv2d_plan.h) takes
// ConvK from here.
#pragma once
#include "sg3_common.h"

namespace sg3 {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// K chunk of the packed fp32 weights per kernel size: [row][chunk][tap][KC]
template <int KS> struct ConvK { static_assert(KS == 1 || KS == 3, "kernel size 1 or 3"); static constexpr int TAPS = KS * KS, KC = (KS == 3) ? 8 : 16; };

// Hardware block id -> logical block id of a 1-D grid of nb blocks: the hardware deals consecutive ids round-robin to the 8 XCDs;
// renumbered, every XCD gets one run of consecutive logical ids (blocks that share operands share its L2).
// flrelu_stream_kernel (sg3_filtered_lrelu.hip, the kernel file of filtered_lrelu: its host side is sg3_flrelu_host.hip) spells the
// same two lines out on purpose: profiles/flrelu_traffic*.json carry the kernel file's hash (tests/test_tools_cpu.py), so an edit
// there means re-collecting them.
__device__ __forceinline__ int xcd_block(int bid, int nb) {
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

// C layout of the 32x32 MFMAs: register r of lane l holds column l & 31, row mfma_c_row(r) + 4 * (l >> 5).  The three exact-fp32
// kernels and two channel sums of modconv_f16x3_kernel spell the formula out: through the helper the index sum is associated
// differently and their instruction streams change; everywhere else the helper compiles to the same instructions.
__host__ __device__ constexpr int mfma_c_row(int r) { return (r & 3) + 8 * (r >> 2); }

} // namespace sg3
