// sg3_filtered_lrelu.hip -- fused bias -> upsample FIR -> gain*lrelu -> clamp -> downsample FIR for gfx950.
//
// Replaces filtered_lrelu_plugin.filtered_lrelu (reference torch_utils/ops/filtered_lrelu.cpp:16-209 and the
// tile kernel torch_utils/ops/filtered_lrelu.cu:139-1099).  The reference kernel is a CUDA thread-block tile
// pipeline (input tile -> 4 shared-memory passes, 512-1024 threads, warp-32 sign packing).  This one is built
// for CDNA4 from scratch around two observations:
//
//   * the op is on the fp32 VALU / HBM ridge (~21 FLOP/B), so the design goal is "nothing but FMAs
//     in the instruction stream": no halo recompute in the vertical direction, no LDS operand per FMA, no
//     workgroup barriers;
//   * both vertical FIR passes and the non-linearity are column-local, so they can live entirely in registers.
//
// Kernel `flrelu_stream_kernel` -- ONE WAVE (64 lanes) owns a strip of up to 120 output columns of one (n,c)
// plane and streams down a chunk of output rows:
//
//     global row i  --(+bias, zero outside the image)-->  LDS row  --H-up (polyphase, taps in SGPRs)-->
//     4 upsampled columns per lane, kept as a 6-row sliding window in VGPRs
//       --V-up (polyphase) --> U new upsampled rows in registers --> *gain, lrelu, clamp
//       --V-down: every upsampled row is scattered into 6 rotating accumulators (FD/D output rows in flight)
//     completed accumulator row --> LDS row --H-down (even/odd polyphase, ds_read_b64 pairs)--> global store
//
//   Per input row and lane that is 1 LDS row write + 8 LDS dword reads + 4 LDS writes + 24 LDS dword reads
//   against ~100 (U=2) / ~190 (U=4) VALU FMAs; the only data that ever touches LDS is one input row and one
//   output row, and because a wave only talks to itself there is no s_barrier anywhere (LDS executes a wave's
//   DS instructions in order; the compiler is held back with wavefront-scope fences).  The window / accumulator
//   rotation is resolved at compile time by unrolling 6 input rows per loop iteration.
//   Global reads are issued 3 rows ahead into registers; reads and writes are 256-B contiguous per instruction.
//   Grid = planes x row-chunks x strips, renumbered so that blocks sharing halo columns/rows sit on one XCD (L2).
//   Lane fill (plain forward): planes at most 54 columns wide run TWO per wave (template G = 2: lanes 0-31 / 32-63, own LDS
//   segments, own bias and gain); rows of 120 n + (1..54) columns are cut into n full strips, one plane per wave, plus the
//   remainder strip with two planes per wave -- in one launch of the G = 2 kernel (StreamParams.wideBlocks) where that costs
//   no occupancy, in two launches otherwise (`launch_stream`, sg3_flrelu_host.hip).
//
// Supported by the streaming kernel (`stream_supported` / `stream_params_ok`, sg3_flrelu_plan.h, are the authority): fp32 / fp16 I/O with
// unit innermost stride, slope in [0,1], and
//   forward, plain or sign-writing (training):  up 2 (12 taps) | up 4 (24 taps), separable;  down 2 with a separable 12-tap
//       filter (config T, and the critically sampled layers of config R) or a full 12x12 filter (radial layers of config R;
//       RADIAL 1|2, or 5|6 when the caller promises mirror-symmetric rows);
//   adjoint (sign-reading):  up 2 with a separable 12-tap filter or a full 12x12 filter (RADIAL 3|4: the radial layers' down
//       filter ends up on the up side), down 2 (12 taps) | down 4 (24 taps), separable.
// `flrelu_pointwise_kernel` (sg3_flrelu_host.hip) covers up = down = 1 with 1x1 filters (the ToRGB layer).  Anything else returns
// SG3_NO_KERNEL and the caller composes upfirdn2d + filtered_lrelu_act + upfirdn2d, exactly like the reference's rc = -1 path.
//
// Algorithmic traffic: C*(xH*xW + yH*yW)*sizeof(T) bytes per image -- the roofline figure bench.py uses.
//
// This file is the DEVICE side alone: the kernel template, and at its end the table of instantiations with the lookup that hands
// their addresses to the host side (sg3_flrelu_host.hip: launchers, the small kernels, the C entry points).  The table is cut into
// parts, -DSG3_FLRELU_PART=k compiles one of them, and the library is linked from all of them (csrc/Makefile); without the macro the
// file holds every kernel.  bench.py and tests/test_tools_cpu.py tie profiles/flrelu_traffic*.json to the sha256 of this file.
#include "sg3_flrelu_kernels.h"
#include <utility>

// rows of input the streaming kernel keeps in flight per wave (each costs NL registers per lane): three rows are ~3 x 1.5 us
// of work, several HBM latencies
#ifndef SG3_PREFETCH_ROWS
#define SG3_PREFETCH_ROWS 3
#endif
// 1: the plain forward keeps the reference's behaviour on non-finite input (a NaN activation stays a NaN through the clamp); 0
// compiles the guard out (A/B timing builds)
#ifndef SG3_NAN_GUARD
#define SG3_NAN_GUARD 1
#endif

namespace sg3 {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) float lds_f;          // explicit LDS address space: keeps ds_* instructions
typedef __attribute__((address_space(3))) v2f lds_v2f;
typedef __attribute__((address_space(3))) v4f lds_v4f;

__device__ __forceinline__ int to_sgpr_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float to_sgpr(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// A wave-uniform value the compiler must keep in a scalar register.  `to_sgpr` does not do that for a value formed by a vector
// instruction (a tap times `up`: gfx950 has no scalar float multiply): the compiler proves it uniform, folds the readfirstlane
// away and leaves the value in a VGPR for the whole kernel.  The s_nop is the wait state a v_readfirstlane needs after the vector
// instruction that wrote its source; the compiler inserts it around its own, not inside an asm statement.
__device__ __forceinline__ float pin_sgpr(float v) {
    float r;
    asm("s_nop 1\n\tv_readfirstlane_b32 %0, %1" : "=s"(r) : "v"(v));
    return r;
}

// Compiler-level ordering of this wave's LDS traffic (no instruction is emitted: a wave's DS ops execute in order).
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a + b as ONE v_add_f32, hidden from the SLP vectoriser (sg3_split.h `mul_single` is the same device for a multiply)
__device__ __forceinline__ float add_single(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// max(m, |a|, |b|) that PROPAGATES a NaN (IEEE 754-2019 maximum; v_max3_f32 returns the other operand).  asm: the file is built
// with -fno-honor-nans, under which the compiler may trade it for the form that drops the NaN
__device__ __forceinline__ float max3_abs_nan(float m, float a, float b) {
    float r;
    asm("v_maximum3_f32 %0, %1, |%2|, |%3|" : "=v"(r) : "v"(m), "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ v2f splat(float a) { return (v2f){a, a}; }

// acc + a * tap, where the tap is ONE half of a scalar-register pair (two taps per SGPR pair, no duplicates).
// The low half is expressible in C (the compiler emits op_sel_hi:[1,0,1]); the high half needs op_sel on the SGPR
// source, which hipcc never selects (it copies the tap to a fresh pair instead and runs out of SGPRs), hence the asm.
template <int HALF>
__device__ __forceinline__ v2f fma_tap(v2f a, v2f tapPair, v2f acc) {
    if (HALF == 0) return fma2(a, __builtin_shufflevector(tapPair, tapPair, 0, 0), acc);
    v2f r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(a), "s"(tapPair), "v"(acc));
    return r;
}
template <int HALF>
__device__ __forceinline__ v2f mul_tap(v2f a, v2f tapPair) {
    if (HALF == 0) return a * __builtin_shufflevector(tapPair, tapPair, 0, 0);
    v2f r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "s"(tapPair));
    return r;
}
// The same two operations with the register file of the tap pair stated (VREG: a vector register pair) and BOTH halves selected by
// op_sel.  Left to the compiler, the low half of a pair that sits in vector registers is splatted into a second register pair per
// tap: at up 4 the 24 up taps then hold 48 VGPRs, and the kernel loses its fourth wave per SIMD.
template <int HALF, bool VREG>
__device__ __forceinline__ v2f fma_tap_at(v2f a, v2f tapPair, v2f acc) {
    v2f r;
    if (HALF == 0 && VREG)  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "v"(tapPair), "v"(acc));
    if (HALF == 0 && !VREG) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(tapPair), "v"(acc));
    if (HALF == 1 && VREG)  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(a), "v"(tapPair), "v"(acc));
    if (HALF == 1 && !VREG) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(a), "s"(tapPair), "v"(acc));
    return r;
}
template <int HALF, bool VREG>
__device__ __forceinline__ v2f mul_tap_at(v2f a, v2f tapPair) {
    v2f r;
    if (HALF == 0 && VREG)  asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(tapPair));
    if (HALF == 0 && !VREG) asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "s"(tapPair));
    if (HALF == 1 && VREG)  asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(tapPair));
    if (HALF == 1 && !VREG) asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "s"(tapPair));
    return r;
}

// Radial (2-D) down filter taps: correlation taps g[k][x] = fd[flip ? k : 11-k][flip ? x : 11-x].  A filter row (12 taps)
// is fetched through the scalar cache into three SGPR quads; without flip the row sits reversed in memory and the
// packed FMA swaps the halves of its scalar pair (op_sel) instead of spending instructions on it.  The loads are
// explicit asm: left to the compiler they are hoisted (constant memory) and spill the scalar file.
struct TapRow { v4f a, b, c; };
__device__ __forceinline__ void radial_row_issue(TapRow& t, const float* fd, int row) {
    const float* src = fd + row * 12;
    asm volatile("s_load_dwordx4 %0, %3, 0x0\n\ts_load_dwordx4 %1, %3, 0x10\n\ts_load_dwordx4 %2, %3, 0x20"
                 : "=&s"(t.a), "=&s"(t.b), "=&s"(t.c) : "s"(src));
}
__device__ __forceinline__ void radial_row_wait(TapRow& t) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t.a), "+s"(t.b), "+s"(t.c));
}
// first half of a filter row (taps 0..5), all a mirror-symmetric row needs
struct TapHalf { v4f a; v2f b; };
__device__ __forceinline__ void radial_half_issue(TapHalf& t, const float* fd, int row) {
    const float* src = fd + row * 12;
    asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx2 %1, %2, 0x10" : "=&s"(t.a), "=&s"(t.b) : "s"(src));
}
__device__ __forceinline__ void radial_half_wait(TapHalf (&t)[6]) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(t[0].a), "+s"(t[0].b), "+s"(t[1].a), "+s"(t[1].b), "+s"(t[2].a), "+s"(t[2].b),
                                          "+s"(t[3].a), "+s"(t[3].b), "+s"(t[4].a), "+s"(t[4].b), "+s"(t[5].a), "+s"(t[5].b));
}
// pair (g[k][2q], g[k][2q+1]) of the row (memory pair q with flip; memory pair 5-q, halves swapped, without)
template <bool FLIP>
__device__ __forceinline__ v2f radial_pair(const TapRow& t, int q) {
    const int j = FLIP ? q : 5 - q;
    const v4f v = j < 2 ? t.a : (j < 4 ? t.b : t.c);
    return (j & 1) ? (v2f){v.z, v.w} : (v2f){v.x, v.y};
}
template <bool FLIP>
__device__ __forceinline__ v2f radial_fma(v2f a, v2f tq, v2f acc) {
    v2f r;
    if (FLIP) asm("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(tq), "v"(acc));
    else      asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(a), "s"(tq), "v"(acc));
    return r;
}
// a + (b.y, b.x)
__device__ __forceinline__ v2f add_swapped(v2f a, v2f b) {
    v2f r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <bool FLIP>
__device__ __forceinline__ v2f radial_mul(v2f a, v2f tq) {
    v2f r;
    if (FLIP) asm("v_pk_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "s"(tq));
    else      asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,0]" : "=v"(r) : "v"(a), "s"(tq));
    return r;
}

// 2-D UP filter (the adjoint of the radial layers: their 12x12 down filter becomes the up filter).  acc += x * (tap pair),
// x = one half of a register pair of adjacent input samples broadcast to both result lanes, the tap pair = one SGPR pair
// of a filter row, halves exchanged when SWAP (filter row stored in the opposite order).
template <int XHALF, bool SWAP>
__device__ __forceinline__ v2f fma_x_tap(v2f xpair, v2f tapPair, v2f acc) {
    v2f r;
    if (XHALF == 0 && !SWAP) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(xpair), "s"(tapPair), "v"(acc));
    if (XHALF == 1 && !SWAP) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "=v"(r) : "v"(xpair), "s"(tapPair), "v"(acc));
    if (XHALF == 0 && SWAP)  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(xpair), "s"(tapPair), "v"(acc));
    if (XHALF == 1 && SWAP)  asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1]" : "=v"(r) : "v"(xpair), "s"(tapPair), "v"(acc));
    return r;
}
// taps (G[k][2s+1], G[k][2s]) of the correlation-form filter row held in `t` (memory row k with flip, 11-k without):
// memory pair s with the halves exchanged (flip), memory pair 5-s as it stands (no flip)
template <bool FLIP>
__device__ __forceinline__ v2f up2d_pair(const TapRow& t, int s) {
    const int j = FLIP ? s : 5 - s;
    const v4f v = j < 2 ? t.a : (j < 4 ? t.b : t.c);
    return (j & 1) ? (v2f){v.z, v.w} : (v2f){v.x, v.y};
}

// StreamParams, the kernel's parameter block, and `fast_threshold`: sg3_flrelu_kernels.h (the host side fills / calls them too)
// StreamCfg<U, D>, the tile constants of the streaming kernel: sg3_flrelu_plan.h (the launch plan reads MAXTW and PACKTW)

// element <-> fp32 through raw buffer instructions: the hardware range check (offset >= num_records reads 0 /
// drops the store) replaces every per-lane bounds branch
template <typename T> struct bufio;
template <> struct bufio<float> {
    static __device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, int byteOff) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byteOff, 0, 0));
    }
    static __device__ __forceinline__ void st1(__amdgpu_buffer_rsrc_t r, int byteOff, float v) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byteOff, 0, 0);
    }
    static __device__ __forceinline__ void st2(__amdgpu_buffer_rsrc_t r, int byteOff, float a, float b) {
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        __builtin_amdgcn_raw_buffer_store_b64((u2){__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b)}, r, byteOff, 0, 0);
    }
};
template <> struct bufio<_Float16> {
    static __device__ __forceinline__ float ld(__amdgpu_buffer_rsrc_t r, int byteOff) {
        return (float)__builtin_bit_cast(_Float16, __builtin_amdgcn_raw_buffer_load_b16(r, byteOff, 0, 0));
    }
    static __device__ __forceinline__ void st1(__amdgpu_buffer_rsrc_t r, int byteOff, float v) {
        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (_Float16)v), r, byteOff, 0, 0);
    }
    static __device__ __forceinline__ void st2(__amdgpu_buffer_rsrc_t r, int byteOff, float a, float b) {
        const unsigned lo = __builtin_bit_cast(unsigned short, (_Float16)a), hi = __builtin_bit_cast(unsigned short, (_Float16)b);
        __builtin_amdgcn_raw_buffer_store_b32(lo | (hi << 16), r, byteOff, 0, 0);
    }
};

template <typename T, int U, int D>
struct WaveState {
    typedef StreamCfg<U, D> Cfg;
    v2f w[6][2];                  // sliding window of H-upsampled rows: [slot][column pair]
    v2f xw[6][4];                 // 2-D up filter: sliding window of RAW input rows, 8 samples per lane as adjacent pairs
    v2f acc[6][2];                // output rows in flight: [slot][column pair]
    float pre[SG3_PREFETCH_ROWS][Cfg::NL];   // prefetched input samples (+bias) for the next rows
    float bcol[Cfg::NL];          // bias where this lane's input column exists, else 0
    int coff[Cfg::NL];            // byte offset of this lane's input columns inside a row
    v2f tuP[Cfg::FU / 2];         // up taps (x U) in REVERSED pairs (tu[2m+1], tu[2m]): the H-up column-pair operands
                                  // as they stand, and the source of the V-up tap splats (odd tap = low half)
    v2f tdP[Cfg::FD / 2];         // down taps (td[2m], td[2m+1]): V-down splats and H-down even/odd pairs
    unsigned sg[SG3_PREFETCH_ROWS][U];       // sign-read mode: prefetched sign bytes (this lane's byte | next byte << 8) per upsampled row
    float osum;                   // running sum of the outputs this lane stored (only kept when p.ysum is given)
    float omax;                   // running max |output| (only kept when p.ymax is given)
    float xmax;                   // separable plain forward, fast pass: running max |staged sample| of this lane, NaN once it staged one
    int soff;                     // sign modes: byte offset, inside a sign row, of the byte holding this lane's first column
    int sq;                       // sign modes: position (0..3) of that column inside its byte (wave-uniform)
    int inBase, outBase;          // packed mode: this lane's window start in the input LDS row / its 4 samples' place in the output LDS row
    int ooff[2];                  // packed mode: byte offsets of this lane's two output columns from the first plane's row (out of range: none)
};

// SIGNS: 0 = plain forward; 1 = forward that also writes the sign tensor (training); 2 = adjoint pass: the stored signs
// replace the nonlinearity (gradient of lrelu + clamp).
// G: planes per wave.  2 = packed mode for narrow planes (yW <= PACKTW, one strip): lanes 0-31 work on plane 2k, lanes 32-63 on plane
// 2k + 1, with their own segments of the two LDS rows -- the 36^2 .. 52^2 layers use 21 .. 29 lanes of a wave otherwise, and the
// kernel's time there is its instruction count.  Plain forward only; tensors dense over (n, c) so that plane 2k + 1 sits one
// channel stride after plane 2k (also across the end of an image).
// WIDE: 1 = the up-4 separable plain forward as it was before its up taps were placed by hand (141 .. 147 VGPRs, three waves per
// SIMD): kept for A/B timing and the bit-identity test (`stream_up4_wide`).  The default form computes the same products in the same
// order from the same tap values; only the registers that hold the taps differ.
template <typename T, int U, int D, int VPH, int RADIAL, int SIGNS, int G = 1, int WIDE = 0>
struct Stream {
    typedef StreamCfg<U, D> Cfg;
    typedef WaveState<T, U, D> State;
    static_assert(WIDE == 0 || (U == 4 && RADIAL == 0 && SIGNS == 0), "WIDE: the up-4 separable plain forward only");
    // Up-4 separable plain forward: where the 12 up tap pairs live.  The scalar file has room for half of them next to the 6 down
    // tap pairs, the descriptors and the row bookkeeping (all 12: 51 .. 62 scalar spills, v_readlane in the row loop); the first
    // TU_PIN pairs are pinned there, the others sit in 12 VGPRs, one pair each, both halves read through op_sel.
    static constexpr bool PLACED = U == 4 && RADIAL == 0 && SIGNS == 0 && WIDE == 0;
    static constexpr int TU_PIN = PLACED ? 6 : 0;
    // separable plain forward (either up factor, one or two planes per wave): the forms whose bookkeeping is trimmed by hand
    static constexpr bool PLAIN = RADIAL == 0 && SIGNS == 0 && WIDE == 0;

    // issue the loads of input row `i` into st.pre[slot]; rows outside the image get a zero-length descriptor
    static __device__ __forceinline__ void prefetch(State& st, int slot, const StreamParams& p, const T* __restrict__ plane,
                                                    const unsigned char* __restrict__ splane, int i) {
        const bool rowOk = (unsigned)i < (unsigned)p.xH;
        const T* row = plane + (long long)i * p.xsH;
        // packed: the descriptor spans the same row of both planes (the lanes' offsets carry the plane and the column range check)
        const int rowBytes = (G > 1 ? (int)p.xsC + p.xW : p.xW) * (int)sizeof(T);
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)row, (short)0, rowOk ? rowBytes : 0, 0x00020000);
        float rowFlag = rowOk ? 1.f : 0.f;
        if (PLAIN) {
            // the flag as ONE scalar register (s_cselect on its bits) that the multiply-add reads as it stands.  Left visible, the
            // compiler selects the bias per lane instead (v_cndmask per load, and the add besides).  Same operation, same bits.
            int rowBits = rowOk ? 0x3f800000 : 0;
            asm("" : "+s"(rowBits));
            rowFlag = __builtin_bit_cast(float, rowBits);
        }
#pragma unroll
        for (int q = 0; q < Cfg::NL; q++) {
            if (PLAIN && q + 1 < Cfg::NL) {          // two loads, one packed multiply-add
                const v2f ld = {bufio<T>::ld(rs, st.coff[q]), bufio<T>::ld(rs, st.coff[q + 1])};
                const v2f r = fma2((v2f){st.bcol[q], st.bcol[q + 1]}, splat(rowFlag), ld);
                st.pre[slot][q] = r.x; st.pre[slot][q + 1] = r.y;
                q++;
                continue;
            }
            st.pre[slot][q] = __builtin_fmaf(st.bcol[q], rowFlag, bufio<T>::ld(rs, st.coff[q]));
        }
        if (SIGNS == 2) {
            // sign bytes of the U upsampled rows this input row will complete (rows / bytes outside the tensor read 0)
#pragma unroll
            for (int j = 0; j < U; j++) {
                const int sr = U * (i - 5) - (U - 1) + j + p.py0 + p.sy;
                const bool ok = (unsigned)sr < (unsigned)p.sH;
                const unsigned char* srow = splane + (ok ? (long long)sr * p.sWb : 0);
                const __amdgpu_buffer_rsrc_t ss = __builtin_amdgcn_make_buffer_rsrc((void*)srow, (short)0, ok ? p.sWb : 0, 0x00020000);
                const unsigned b0 = __builtin_amdgcn_raw_buffer_load_b8(ss, st.soff, 0, 0);
                const unsigned b1 = __builtin_amdgcn_raw_buffer_load_b8(ss, st.soff + 1, 0, 0);
                st.sg[slot][j] = b0 | (b1 << 8);
            }
        }
    }

    // one input row: H-up into window slot S, then U upsampled rows through lrelu into the down accumulators.  FAST (plain forward
    // only): the activation is the single med3(u, slope u, clamp), and a staged sample that fails |x| <= fastT is recorded -- in
    // st.xmax (separable forms), or by `liveGain` dropping to 0 from that row on (radial and WIDE forms) -- so that the outputs of
    // such a pass are rewritten by a pass with FAST = false
    template <int S, bool FAST>
    static __device__ __forceinline__ void step(State& st, const StreamParams& p, const T* __restrict__ plane, T* __restrict__ oplane,
                                                unsigned char* __restrict__ splane, lds_f* sIn, lds_f* sOut, int i, int delta, int lane,
                                                int oy0, int oy1, int ox0, int oxN, bool pairStore, float& liveGain, float& liveGain1, bool wide,
                                                float fastT) {
        constexpr bool RDOWN = RADIAL == 1 || RADIAL == 2 || RADIAL >= 5;   // full 12x12 DOWN filter (config R forward)
        constexpr bool FOLD = RADIAL >= 5;                         // ... whose rows read the same in both directions
        constexpr bool UP2D = RADIAL == 3 || RADIAL == 4;          // full 12x12 UP filter (adjoint of those layers)
        // ---- input row -> LDS -> this lane's H-upsampled samples ----
        wave_lds_sync();                 // the previous row's sIn reads precede this row's writes
        constexpr int PS = S % SG3_PREFETCH_ROWS;        // prefetch slot of this row
#pragma unroll
        for (int q = 0; q < Cfg::NL; q++) sIn[lane + 64 * q] = st.pre[PS][q];
        // Non-finite input.  v_med3 returns the MINIMUM of its operands when one is a NaN, so the clamp below turns a NaN activation
        // into -clamp, while the reference's `if (fabsf(v) > clamp) v = copysign(clamp, v)` (filtered_lrelu.cu:412-419) lets it
        // through; a NaN-preserving clamp costs an instruction per upsampled sample (8 %), and a wave-uniform branch to one cost 5 %
        // (measured: it fences the scheduler).  Instead every sample a lane stages is classified (one v_cmp_class per load: NaN or
        // infinity, which meets taps of both signs in the filter) and from the row a wave has met one on, its output gain -- one
        // scalar register, overwritten in place -- is NaN: every output it still writes in this strip is NaN.  That is a superset of the
        // reference's NaN footprint (a failure stays loud and stays where it happened), at no cost inside the nonlinearity.  The
        // last load of a row holds the strip's 6 halo samples, which the neighbouring strip classifies as its own: left out here.
        if (PLAIN && FAST) {
            // fast pass: the threshold test needs its answer only when the chunk is done (`run` reads it once), so a lane folds the
            // samples it stages -- the strip's halo included: it feeds this strip's upsampled samples -- into a running maximum of
            // magnitudes that keeps a NaN, two samples per instruction, instead of comparing each load against the threshold
#pragma unroll
            for (int q = 0; q < Cfg::NL; q += 2)
                st.xmax = max3_abs_nan(st.xmax, st.pre[PS][q], st.pre[PS][q + 1 < Cfg::NL ? q + 1 : q]);
        } else if (SIGNS == 0 && FAST) {
            // fast pass: every load a lane stages, the strip's halo included (it feeds this strip's upsampled samples), is tested
            // against the threshold: v_cmp_nle is true for |x| > T, NaN and infinity alike, and takes the place of the class test.
            // The radial forms have no scalar register to spare (a spill puts v_readlane into the row loop): T sits in a VGPR there.
#pragma unroll
            for (int q = 0; q < Cfg::NL; q++) {
                unsigned long long m;
                if (RADIAL) asm("v_cmp_nle_f32_e64 %0, |%1|, %2" : "=s"(m) : "v"(st.pre[PS][q]), "v"(fastT));
                else        asm("v_cmp_nle_f32_e64 %0, |%1|, %2" : "=s"(m) : "v"(st.pre[PS][q]), "s"(fastT));
                liveGain = m != 0ull ? 0.f : liveGain;
            }
        } else if (SIGNS == 0 && SG3_NAN_GUARD && G > 1) {
            // packed: every load is the wave's own (no neighbouring strip); staging lane e = lane + 64 q belongs to the first plane
            // while e < PSEG -- each plane has its own gain register
#pragma unroll
            for (int q = 0; q < Cfg::NL; q++) {
                unsigned long long m;
                asm("v_cmp_class_f32 %0, %1, %2" : "=s"(m) : "v"(st.pre[PS][q]), "s"(0x207));
                const int n0 = Cfg::PSEG - 64 * q;                                   // lanes of this load that stage the first plane
                const unsigned long long first = n0 >= 64 ? ~0ull : (n0 <= 0 ? 0ull : ((1ull << (n0 & 63)) - 1ull));
                // one-plane blocks: both registers follow the one plane, the last load (halo) left out as in the one-plane kernel
                const unsigned long long mw = q < Cfg::NL - 1 ? m : 0ull;
                liveGain = (wide ? mw : (m & first)) != 0ull ? __builtin_bit_cast(float, 0x7fc00000u) : liveGain;
                liveGain1 = (wide ? mw : (m & ~first)) != 0ull ? __builtin_bit_cast(float, 0x7fc00000u) : liveGain1;
            }
        } else if (SIGNS <= 1 && SG3_NAN_GUARD) {           // the sign-writing forward too: its outputs are the plain forward's
#pragma unroll
            for (int q = 0; q < Cfg::NL - 1; q++) {
                unsigned long long m;            // asm: the file is built with -fno-honor-nans, which folds the NaN classes away
                asm("v_cmp_class_f32 %0, %1, %2" : "=s"(m) : "v"(st.pre[PS][q]), "s"(0x207));
                // the output gain itself carries the state (one scalar register that is live anyway: the radial kernels have none to spare)
                liveGain = m != 0ull ? __builtin_bit_cast(float, 0x7fc00000u) : liveGain;
            }
        }
        unsigned sgNow[U];               // this row's sign bytes: the prefetch below reuses their slot
#pragma unroll
        for (int j = 0; j < U; j++) sgNow[j] = SIGNS == 2 ? st.sg[PS][j] : 0u;
        prefetch(st, PS, p, plane, splane, i + SG3_PREFETCH_ROWS);
        wave_lds_sync();
        if (U == 2) {
            float xs[8];
            // volatile: keeps four ds_read_b64 (2 LDS cycles each); merged into ds_read2_b64 they run at a quarter of that
            const volatile lds_v2f* src = reinterpret_cast<const volatile lds_v2f*>(sIn + (G > 1 ? st.inBase : 2 * lane));
#pragma unroll
            for (int q = 0; q < 4; q++) { v2f t = src[q]; xs[2 * q] = t.x; xs[2 * q + 1] = t.y; if (UP2D) st.xw[S][q] = t; }
#pragma unroll
            for (int g = 0; g < 2 && !UP2D; g++) {
                v2f a = splat(xs[g]) * st.tuP[0];
#pragma unroll
                for (int t = 1; t < 6; t++) a = fma2(splat(xs[g + t]), st.tuP[t], a);
                st.w[S][g] = a;
            }
        } else {  // U == 4: the lane's four columns are the four phases of one input window
            float xs[6];
#pragma unroll
            for (int t = 0; t < 6; t++) xs[t] = sIn[(G > 1 ? st.inBase : lane) + t];
            v2f a0 = splat(xs[0]) * st.tuP[1], a1 = splat(xs[0]) * st.tuP[0];
#pragma unroll
            for (int t = 1; t < 6; t++) {
                a0 = fma2(splat(xs[t]), st.tuP[2 * t + 1], a0);    // columns 0,1: phases 3,2
                a1 = fma2(splat(xs[t]), st.tuP[2 * t], a1);        // columns 2,3: phases 1,0
            }
            st.w[S][0] = a0; st.w[S][1] = a1;
        }
        // ---- U new upsampled rows ----
        const float slope = p.slope, clampv = p.clamp / p.gain, gain = p.gain;
        // the 2-D up filter's taps carry no up^2 factor
        const float gainOut = UP2D ? p.gain * (float)(U * U) :
                              ((SIGNS <= 1 && (SG3_NAN_GUARD || FAST) && !(PLAIN && FAST)) ? ((G > 1 && lane >= 32 && !FAST) ? liveGain1 : liveGain) : p.gain);
#pragma unroll
        for (int j = 0; j < U; j++) {
            const int kv = U - 1 - j;                          // vertical up phase of this row
            v2f u0, u1;
            // mirror-symmetric 12x12 down filter: the six half rows this upsampled row needs (36 taps) are requested now and
            // arrive under the vertical up filter and the nonlinearity
            TapHalf th[6];
            if (FOLD) {
                const int kp0 = (VPH + S * U + j) % D;
#pragma unroll
                for (int r = 0; r < 6; r++) radial_half_issue(th[r], p.fd, (RADIAL == 6) ? kp0 + r * D : 11 - (kp0 + r * D));
            }
            if (UP2D) {
                // 36 taps per upsampled sample: filter rows kv, kv + 2, .. against the six raw rows of the window; the rows
                // stream through the scalar cache like the radial down filter's, the next one loading under this one's FMAs
                constexpr bool FLIPU = RADIAL == 4;
                u0 = splat(0.f); u1 = splat(0.f);
                TapRow rowA, rowB;
                radial_row_issue(rowA, p.fu, FLIPU ? kv : 11 - kv);
#pragma unroll
                for (int t = 0; t < 6; t++) {
                    const int slot = (S + 1 + t) % 6;          // t = 0: oldest row (i - 5)
                    const int k = kv + 2 * t;
                    TapRow& cur = (t & 1) ? rowB : rowA;
                    TapRow& nxt = (t & 1) ? rowA : rowB;
                    radial_row_wait(cur);
                    if (t < 5) radial_row_issue(nxt, p.fu, FLIPU ? k + 2 : 11 - (k + 2));
#pragma unroll
                    for (int sx = 0; sx < 6; sx++) {
                        const v2f tq = up2d_pair<FLIPU>(cur, sx);
                        // column groups 0 / 1 read samples sx / sx + 1 of the row
                        u0 = (sx & 1) ? fma_x_tap<1, FLIPU>(st.xw[slot][sx / 2], tq, u0) : fma_x_tap<0, FLIPU>(st.xw[slot][sx / 2], tq, u0);
                        u1 = ((sx + 1) & 1) ? fma_x_tap<1, FLIPU>(st.xw[slot][(sx + 1) / 2], tq, u1) : fma_x_tap<0, FLIPU>(st.xw[slot][(sx + 1) / 2], tq, u1);
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 6 && !UP2D; t++) {
                const int slot = (S + 1 + t) % 6;              // t = 0: oldest row (i - 5)
                const int k = kv + U * t;
                // tap k lives in the reversed pair k/2: odd k = low half, even k = high half
                if (PLACED) {
                    const v2f tp = st.tuP[k / 2];
                    const bool vr = k / 2 >= TU_PIN;
                    if (t == 0) {
                        u0 = (k & 1) ? (vr ? mul_tap_at<0, true>(st.w[slot][0], tp) : mul_tap_at<0, false>(st.w[slot][0], tp))
                                     : (vr ? mul_tap_at<1, true>(st.w[slot][0], tp) : mul_tap_at<1, false>(st.w[slot][0], tp));
                        u1 = (k & 1) ? (vr ? mul_tap_at<0, true>(st.w[slot][1], tp) : mul_tap_at<0, false>(st.w[slot][1], tp))
                                     : (vr ? mul_tap_at<1, true>(st.w[slot][1], tp) : mul_tap_at<1, false>(st.w[slot][1], tp));
                    } else if (k & 1) {
                        u0 = vr ? fma_tap_at<0, true>(st.w[slot][0], tp, u0) : fma_tap_at<0, false>(st.w[slot][0], tp, u0);
                        u1 = vr ? fma_tap_at<0, true>(st.w[slot][1], tp, u1) : fma_tap_at<0, false>(st.w[slot][1], tp, u1);
                    } else {
                        u0 = vr ? fma_tap_at<1, true>(st.w[slot][0], tp, u0) : fma_tap_at<1, false>(st.w[slot][0], tp, u0);
                        u1 = vr ? fma_tap_at<1, true>(st.w[slot][1], tp, u1) : fma_tap_at<1, false>(st.w[slot][1], tp, u1);
                    }
                    continue;
                }
                if (t == 0) {
                    u0 = (k & 1) ? mul_tap<0>(st.w[slot][0], st.tuP[k / 2]) : mul_tap<1>(st.w[slot][0], st.tuP[k / 2]);
                    u1 = (k & 1) ? mul_tap<0>(st.w[slot][1], st.tuP[k / 2]) : mul_tap<1>(st.w[slot][1], st.tuP[k / 2]);
                } else if (k & 1) {
                    u0 = fma_tap<0>(st.w[slot][0], st.tuP[k / 2], u0);
                    u1 = fma_tap<0>(st.w[slot][1], st.tuP[k / 2], u1);
                } else {
                    u0 = fma_tap<1>(st.w[slot][0], st.tuP[k / 2], u0);
                    u1 = fma_tap<1>(st.w[slot][1], st.tuP[k / 2], u1);
                }
            }
            const int uy = U * (i - 5) - (U - 1) + j + p.py0;  // row of the upsampled buffer
            float a[4] = {u0.x, u0.y, u1.x, u1.y};
            if (SIGNS == 2) {
                // adjoint pass: the stored sign codes select the derivative of lrelu + clamp (1, slope or 0); the gain is
                // linear and applied once per output sample
                const unsigned bits = sgNow[j] >> (2 * st.sq);
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const unsigned code = bits >> (2 * c);
                    a[c] *= (code & 2u) ? 0.f : ((code & 1u) ? slope : 1.f);
                }
            }
            if (SIGNS == 1) {
                // training forward: the sign codes are decided in the reference's exact order (gain, lrelu, clamp; filtered_lrelu.cu
                // sign write) so that they agree with it: 1 = negative, 2 = clamped.  The output VALUES are formed below exactly as
                // the plain forward forms them (gain once per output sample), so that training reproduces inference bit for bit.
                // The code compares fl(gain * u) with clamp, the value clamps u at fl(clamp / gain): within a rounding of the
                // threshold a sample can carry the code "clamped" with an unclamped value or the reverse -- a difference of one
                // rounding of clamp in y, and a sample whose gradient multiplier is within rounding of its jump anyway.
                unsigned code = 0;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float v = a[c] * gain;
                    const bool neg = v < 0.f;
                    const float lv = neg ? v * slope : v;
                    const bool big = __builtin_fabsf(lv) > p.clamp;
                    code |= (big ? 2u : (neg ? 1u : 0u)) << (2 * c);
                }
                const int sr = uy + p.sy;
                if (uy >= oy0 * D && uy <= (oy1 - 1) * D + Cfg::FD - 1 && (unsigned)sr < (unsigned)p.sH) {    // wave-uniform
                    // a byte holds 4 consecutive columns; a lane's 4 columns start st.sq columns into a byte, so the byte is
                    // completed with the first st.sq columns of the next lane
                    const unsigned nxt = (unsigned)__shfl_down((int)code, 1);
                    const unsigned byte = st.sq == 0 ? code : ((code >> (2 * (4 - st.sq))) | (nxt << (2 * st.sq))) & 0xffu;
                    const int bofs = (st.sq == 0 || lane < 63) ? st.soff + (st.sq ? 1 : 0) : -1;
                    const __amdgpu_buffer_rsrc_t ss = __builtin_amdgcn_make_buffer_rsrc((void*)(splane + (long long)sr * p.sWb), (short)0, p.sWb, 0x00020000);
                    __builtin_amdgcn_raw_buffer_store_b8((unsigned char)byte, ss, bofs, 0, 0);
                }
            }
            if (SIGNS != 2 && FAST) {
                // lrelu + clamp in one instruction: med3(u, slope u, c) = med3(max(u, slope u), -c, c) whenever slope |u| <= c (u < 0:
                // slope u; 0 <= u <= c: u; u > c: c -- exact selections), which the threshold test on the staged samples guarantees
                const v2f s0 = u0 * splat(slope), s1 = u1 * splat(slope);
                a[0] = __builtin_amdgcn_fmed3f(u0.x, s0.x, clampv); a[1] = __builtin_amdgcn_fmed3f(u0.y, s0.y, clampv);
                a[2] = __builtin_amdgcn_fmed3f(u1.x, s1.x, clampv); a[3] = __builtin_amdgcn_fmed3f(u1.y, s1.y, clampv);
            } else if (SIGNS != 2) {
                // leaky ReLU (slope <= 1 so lrelu(v) = max(v, slope*v)) and clamp.  The activation gain g > 0 commutes with
                // both: clamp_c(lrelu(g*u)) = g * clamp_{c/g}(lrelu(u)), so g is applied once per OUTPUT sample after the
                // down filter instead of once per upsampled sample (clampv = clamp / gain here)
                const v2f s0 = u0 * splat(slope), s1 = u1 * splat(slope);
                a[0] = __builtin_fmaxf(u0.x, s0.x); a[1] = __builtin_fmaxf(u0.y, s0.y); a[2] = __builtin_fmaxf(u1.x, s1.x); a[3] = __builtin_fmaxf(u1.y, s1.y);
#pragma unroll
                for (int c = 0; c < 4; c++) a[c] = __builtin_amdgcn_fmed3f(a[c], -clampv, clampv);
            }
            const v2f r0 = {a[0], a[1]}, r1 = {a[2], a[3]};
            const int kp = (VPH + S * U + j) % D;              // down phase of this row (a trip starts at phase VPH)
            if (RDOWN) {
                // ---- full 2-D down filter (config R): the activated row is exchanged through LDS once (each lane reads
                // the 16 samples under its two output columns) and scattered into the six output rows it belongs to, one
                // even/odd polyphase pass per output row with that row's 12 taps.  The 144 taps do not fit the scalar
                // registers: they stream through the scalar cache (s_load) as SGPR pairs, off the LDS and VALU paths.
                lds_f* dstr = sOut + (4 - delta) + (G > 1 ? st.outBase : 4 * lane);
                dstr[0] = r0.x; dstr[1] = r0.y; dstr[2] = r1.x; dstr[3] = r1.y;
                wave_lds_sync();
                const lds_v4f* srcr = reinterpret_cast<const lds_v4f*>(sOut + 4 + (G > 1 ? st.outBase : 4 * lane));
                v2f pr[8];
#pragma unroll
                for (int q = 0; q < 4; q++) { const v4f t = srcr[q]; pr[2 * q] = (v2f){t.x, t.y}; pr[2 * q + 1] = (v2f){t.z, t.w}; }
                wave_lds_sync();
                const int headR = ((VPH + S * U + j) / D) % 6;
                constexpr bool FLIPPED = RADIAL == 2 || RADIAL == 6;
                // mirror-symmetric rows: the samples j and 11 - j under an output column share a tap, so they are added
                // first (three packed adds per column, the partner pair entering with its halves exchanged) and each of the
                // six output rows then costs three packed FMAs per column instead of six
                v2f fo[2][3];
#pragma unroll
                for (int q = 0; q < 3 && FOLD; q++) { fo[0][q] = add_swapped(pr[q], pr[5 - q]); fo[1][q] = add_swapped(pr[q + 1], pr[6 - q]); }
                if (FOLD) radial_half_wait(th);
#pragma unroll
                for (int r = 0; r < 6 && FOLD; r++) {
                    const int slot = (headR + 5 - r) % 6;          // r = 5: oldest output row (completes first)
                    const int k = kp + r * D;                      // filter row of this upsampled row in that output row
#pragma unroll
                    for (int q = 0; q < 3; q++) {
                        // memory order: taps (2q, 2q + 1) of the row
                        const v2f tq = q == 0 ? (v2f){th[r].a.x, th[r].a.y} : (q == 1 ? (v2f){th[r].a.z, th[r].a.w} : th[r].b);
                        if (k == 0 && q == 0) {
                            st.acc[slot][0] = radial_mul<true>(fo[0][0], tq);
                            st.acc[slot][1] = radial_mul<true>(fo[1][0], tq);
                        } else {
                            st.acc[slot][0] = radial_fma<true>(fo[0][q], tq, st.acc[slot][0]);
                            st.acc[slot][1] = radial_fma<true>(fo[1][q], tq, st.acc[slot][1]);
                        }
                    }
                }
                TapRow rowA, rowB;                                 // filter rows in flight: the next one loads under this one's FMAs
                if (!FOLD) radial_row_issue(rowA, p.fd, FLIPPED ? kp : 11 - kp);
#pragma unroll
                for (int r = 0; r < 6 && !FOLD; r++) {
                    const int slot = (headR + 5 - r) % 6;          // r = 5: oldest output row (completes first)
                    const int k = kp + r * D;                      // filter row of this upsampled row in that output row
                    TapRow& cur = (r & 1) ? rowB : rowA;
                    TapRow& nxt = (r & 1) ? rowA : rowB;
                    radial_row_wait(cur);
                    if (r < 5) radial_row_issue(nxt, p.fd, FLIPPED ? k + D : 11 - (k + D));
#pragma unroll
                    for (int q = 0; q < 6 && !FOLD; q++) {
                        const v2f tq = radial_pair<FLIPPED>(cur, q);
                        if (k == 0 && q == 0) {
                            st.acc[slot][0] = radial_mul<FLIPPED>(pr[0], tq);
                            st.acc[slot][1] = radial_mul<FLIPPED>(pr[1], tq);
                        } else {
                            st.acc[slot][0] = radial_fma<FLIPPED>(pr[q], tq, st.acc[slot][0]);
                            st.acc[slot][1] = radial_fma<FLIPPED>(pr[q + 1], tq, st.acc[slot][1]);
                        }
                    }
                }
                if (kp == D - 1) {
                    const int oy = (uy - (Cfg::FD - 1)) / D;       // exact
                    if (oy >= oy0 && oy < oy1) {                   // wave-uniform
                        const v2f y0 = st.acc[headR][0], y1 = st.acc[headR][1];
                        const float f0 = (y0.x + y0.y) * gainOut, f1 = (y1.x + y1.y) * gainOut;
                        if (SIGNS == 2) {
                            const float m0 = 2 * lane < oxN ? f0 : 0.f, m1 = 2 * lane + 1 < oxN ? f1 : 0.f;
                            st.osum += m0 + m1;
                            st.omax = __builtin_fmaxf(st.omax, __builtin_fmaxf(__builtin_fabsf(m0), __builtin_fabsf(m1)));
                        }
                        T* orow = oplane + (long long)oy * p.ysH + ox0;
                        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)orow, (short)0, (G > 1 ? (int)p.ysC + oxN : oxN) * (int)sizeof(T), 0x00020000);
                        if (pairStore) {
                            bufio<T>::st2(rs, G > 1 ? st.ooff[0] : 2 * lane * (int)sizeof(T), f0, f1);
                        } else {
                            bufio<T>::st1(rs, G > 1 ? st.ooff[0] : 2 * lane * (int)sizeof(T), f0);
                            bufio<T>::st1(rs, G > 1 ? st.ooff[1] : (2 * lane + 1) * (int)sizeof(T), f1);
                        }
                    }
                }
                continue;
            }
            // scatter into the FD/D output rows this upsampled row belongs to
            const int headNow = ((VPH + S * U + j) / D) % 6;   // output rows completed so far in this trip shift the head
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const int slot = (headNow + 5 - r) % 6;        // r = 5: oldest output row (completes first)
                const int k = kp + r * D;
                if (k == 0) {                                  // first contribution to a new output row: no zeroing needed
                    st.acc[slot][0] = mul_tap<0>(r0, st.tdP[0]);
                    st.acc[slot][1] = mul_tap<0>(r1, st.tdP[0]);
                } else if (k & 1) {
                    st.acc[slot][0] = fma_tap<1>(r0, st.tdP[k / 2], st.acc[slot][0]);
                    st.acc[slot][1] = fma_tap<1>(r1, st.tdP[k / 2], st.acc[slot][1]);
                } else {
                    st.acc[slot][0] = fma_tap<0>(r0, st.tdP[k / 2], st.acc[slot][0]);
                    st.acc[slot][1] = fma_tap<0>(r1, st.tdP[k / 2], st.acc[slot][1]);
                }
            }
            if (kp == D - 1) {
                // output row complete: H-down through LDS and store
                const int oy = (uy - (Cfg::FD - 1)) / D;       // exact
                if (oy >= oy0 && oy < oy1) {                   // wave-uniform
                    const v2f o0 = st.acc[headNow][0], o1 = st.acc[headNow][1];
                    lds_f* dst = sOut + (4 - delta) + (G > 1 ? st.outBase : 4 * lane);
                    dst[0] = o0.x; dst[1] = o0.y; dst[2] = o1.x; dst[3] = o1.y;
                    wave_lds_sync();
                    T* orow = oplane + (long long)oy * p.ysH + ox0;
                    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)orow, (short)0, (G > 1 ? (int)p.ysC + oxN : oxN) * (int)sizeof(T), 0x00020000);
                    const lds_v4f* src = reinterpret_cast<const lds_v4f*>(sOut + 4 + (G > 1 ? st.outBase : 4 * lane));
                    if (D == 2) {
                        // lane l -> output columns 2l, 2l+1: upsampled samples 4l .. 4l+13 (+4 pad), four aligned b128 reads
                        v2f pr[8];
#pragma unroll
                        for (int q = 0; q < 4; q++) { const v4f t = src[q]; pr[2 * q] = (v2f){t.x, t.y}; pr[2 * q + 1] = (v2f){t.z, t.w}; }
                        v2f y0 = pr[0] * st.tdP[0], y1 = pr[1] * st.tdP[0];
#pragma unroll
                        for (int q = 1; q < Cfg::FD / 2; q++) { y0 = fma2(pr[q], st.tdP[q], y0); y1 = fma2(pr[q + 1], st.tdP[q], y1); }
                        // even + odd phase of each column.  Written as y0.x + y0.y the two sums become one packed add whose operands
                        // are first re-packed across register pairs (three v_mov per output row); two plain adds need no move
                        const float e0 = PLAIN ? add_single(y0.x, y0.y) : y0.x + y0.y, e1 = PLAIN ? add_single(y1.x, y1.y) : y1.x + y1.y;
                        const float f0 = e0 * gainOut, f1 = e1 * gainOut;
                        if (SIGNS == 2) {
                            const float m0 = 2 * lane < oxN ? f0 : 0.f, m1 = 2 * lane + 1 < oxN ? f1 : 0.f;
                            st.osum += m0 + m1;
                            st.omax = __builtin_fmaxf(st.omax, __builtin_fmaxf(__builtin_fabsf(m0), __builtin_fabsf(m1)));
                        }
#ifdef SG3_FUSION_BOUND
                        // diagnostic builds of tools/flrelu_fusion_bound.hip ONLY (never in the product library): what a fusion of this
                        // layer with the ToRGB convolution behind it could cost at least.  1: the activation plane is not stored at all
                        // (the outputs are only kept alive); 2: instead, the wave's share of the three RGB partial sums -- three packed
                        // multiplies with wave-uniform weights and three 8-byte LDS writes per lane and row; the exchange between the
                        // waves of a pixel (LDS reads, adds, barrier) and the store of the partial image are NOT included.
                        if (SG3_FUSION_BOUND >= 2) {
                            lds_v2f* rgbx = reinterpret_cast<lds_v2f*>(sOut + Cfg::SOUT);
#pragma unroll
                            for (int k = 0; k < 3; k++) rgbx[k * 64 + lane] = (v2f){f0, f1} * splat(p.slope * (float)(k + 1));
                        } else {
                            asm volatile("" :: "v"(f0), "v"(f1));
                        }
                        if (false) {
#else
                        if (pairStore) {
#endif
                            bufio<T>::st2(rs, G > 1 ? st.ooff[0] : 2 * lane * (int)sizeof(T), f0, f1);
                        } else {
                            bufio<T>::st1(rs, G > 1 ? st.ooff[0] : 2 * lane * (int)sizeof(T), f0);
                            bufio<T>::st1(rs, G > 1 ? st.ooff[1] : (2 * lane + 1) * (int)sizeof(T), f1);
                        }
                    } else {
                        // D == 4: lane l -> output column l: upsampled samples 4l .. 4l+23, six aligned b128 reads
                        v2f pr[12];
#pragma unroll
                        for (int q = 0; q < 6; q++) { const v4f t = src[q]; pr[2 * q] = (v2f){t.x, t.y}; pr[2 * q + 1] = (v2f){t.z, t.w}; }
                        v2f y0 = pr[0] * st.tdP[0];
#pragma unroll
                        for (int q = 1; q < Cfg::FD / 2; q++) y0 = fma2(pr[q], st.tdP[q], y0);
                        const float f0 = (y0.x + y0.y) * gainOut;
                        if (SIGNS == 2) {
                            const float m0 = lane < oxN ? f0 : 0.f;
                            st.osum += m0;
                            st.omax = __builtin_fmaxf(st.omax, __builtin_fabsf(m0));
                        }
                        bufio<T>::st1(rs, lane * (int)sizeof(T), f0);
                    }
                    wave_lds_sync();
                }
            }
        }
    }

    // the chunk: zero window and accumulators, prefetch, then the rows 6 at a time
    template <bool FAST>
    static __device__ __forceinline__ void stream_chunk(State& st, const StreamParams& p, const T* __restrict__ plane, T* __restrict__ oplane,
                                                        unsigned char* __restrict__ splane, lds_f* sIn, lds_f* sOut, int iFirst, int nBlocks,
                                                        int delta, int lane, int oy0, int oy1, int ox0, int oxN, bool pairStore, float& liveGain,
                                                        float& liveGain1, bool wide, float fastT) {
#pragma unroll
        for (int s = 0; s < 6; s++) {
            st.w[s][0] = splat(0.f); st.w[s][1] = splat(0.f);
#pragma unroll
            for (int q = 0; q < 4; q++) st.xw[s][q] = splat(0.f);
            st.acc[s][0] = splat(0.f); st.acc[s][1] = splat(0.f);
            if (s < SG3_PREFETCH_ROWS) prefetch(st, s, p, plane, splane, iFirst + s);
        }

        int i = iFirst;
        for (int blk = 0; blk < nBlocks; blk++, i += 6) {
            step<0, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 0, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            step<1, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 1, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            step<2, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 2, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            step<3, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 3, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            step<4, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 4, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            step<5, FAST>(st, p, plane, oplane, splane, sIn, sOut, i + 5, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1, wide, fastT);
            if ((6 * U / D) % 6 != 0) {
                // a trip completes 6U/D output rows; when that is 3 (U = 2, D = 4) the ring of output rows has turned by
                // half: swap the halves so that the compile-time slot numbering holds for the next trip
#pragma unroll
                for (int r = 0; r < 3; r++)
#pragma unroll
                    for (int h = 0; h < 2; h++) { const v2f t = st.acc[r][h]; st.acc[r][h] = st.acc[r + 3][h]; st.acc[r + 3][h] = t; }
            }
        }
    }

    static __device__ __forceinline__ void run(const StreamParams& p) {
        static_assert((D == 2 || D == 4) && (6 * U) % D == 0, "streaming kernel: down is 2 or 4");
        constexpr bool RDOWN = RADIAL == 1 || RADIAL == 2 || RADIAL >= 5;
        constexpr bool UP2D = RADIAL == 3 || RADIAL == 4;
        static_assert(RADIAL >= 0 && RADIAL <= 6, "RADIAL: 0 separable, 1/2 12x12 down, 3/4 12x12 up, 5/6 12x12 down with mirror-symmetric rows");
        static_assert(!RDOWN || (D == 2 && SIGNS != 2), "radial down filter: forward passes (plain or sign-writing), down 2");
        static_assert(!UP2D || (U == 2 && SIGNS == 2), "2-D up filter: the adjoint pass, up 2");
        static_assert(G == 1 || (G == 2 && SIGNS == 0 && D == 2), "packed mode: plain forward, down 2, two planes");
#ifdef SG3_FUSION_BOUND
        __shared__ __attribute__((aligned(16))) float lds[Cfg::SIN + Cfg::SOUT + 3 * 128];      // + the diagnostic RGB rows
#else
        __shared__ __attribute__((aligned(16))) float lds[Cfg::SIN + Cfg::SOUT];
#endif
        lds_f* sIn = (lds_f*)lds;
        lds_f* sOut = (lds_f*)lds + Cfg::SIN;                               // row exchanged for the horizontal down pass
        const int lane = threadIdx.x;
#ifdef SG3_STAMPS
        const unsigned long long stampC = __builtin_amdgcn_s_memtime(), stampR = __builtin_amdgcn_s_memrealtime();
#endif

        // XCD-aware renumbering: consecutive logical blocks (adjacent strips / chunks of one plane) share an XCD's L2
        int bid = blockIdx.x;
        {
            const int nb = p.totalBlocks, q = nb >> 3, r = nb & 7, xcd = bid & 7, k = bid >> 3;
            bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
        }
        // a G = 2 kernel runs both forms: its first wideBlocks blocks take the full-width strips of the rows, one plane each, the
        // others the remainder strip (or the whole row, when it is narrow) of two planes each.  Wave-uniform.
        const bool wide = G > 1 && bid < p.wideBlocks;
        const bool two = G > 1 && !wide;
        const int pbid = two ? bid - p.wideBlocks : bid;
        const int strip = two ? 0 : pbid % p.nStrips;
        const int chunk = two ? pbid % p.nChunks : (pbid / p.nStrips) % p.nChunks;
        const int plane_id = two ? (pbid / p.nChunks) * 2 : pbid / (p.nStrips * p.nChunks);      // two: the first of this wave's planes
        const int n = plane_id / p.C, c = plane_id - n * p.C;

        const int ox0 = (G > 1 && wide) ? strip * p.TW : p.ox0Base + strip * p.TW;
        const int oxN = two ? p.yW - ox0 : min(p.TW, p.yW - ox0);
        const int oy0 = chunk * p.CH;
        const int oy1 = min(oy0 + p.CH, p.yH);

        const T* plane = (const T*)p.x + (long long)n * p.xsN + (long long)c * p.xsC;
        T* oplane = (T*)p.y + (long long)n * p.ysN + (long long)c * p.ysC;
        const float bias = p.b ? io<T>::ld((const T*)p.b + (long long)c * p.bStride) : 0.f;
        unsigned char* splane = SIGNS ? p.s + (long long)plane_id * p.sH * p.sWb : nullptr;
        // a pair store must not straddle the end of the row (and fp16 pairs must be dword aligned)
        const bool pairStore = ((oxN & 1) == 0) &&
            (sizeof(T) == 4 || (((((unsigned long long)oplane >> 1) + (unsigned long long)ox0) & 1) == 0 && (p.ysH & 1) == 0 && (G == 1 || (p.ysC & 1) == 0)));
        // packed: the second plane is the next one of the dense (n, c) order -- channel 0 of the next image after the last channel;
        // an odd number of planes leaves the last wave without one
        const bool second = two && plane_id + 1 < p.planes;
        const float bias1 = (second && p.b) ? io<T>::ld((const T*)p.b + (long long)(c + 1 == p.C ? 0 : c + 1) * p.bStride) : 0.f;

        State st;
        // taps -> scalar register pairs; effective correlation taps g[k] = f[flip ? k : taps-1-k]
        const float gU = (float)U;
#pragma unroll
        for (int m = 0; m < Cfg::FU / 2; m++) {
            if (UP2D) { st.tuP[m] = splat(0.f); continue; }          // 2-D up filter: rows stream from the scalar cache
            const float f1 = p.fu[p.flip ? 2 * m + 1 : Cfg::FU - 2 - 2 * m], f0 = p.fu[p.flip ? 2 * m : Cfg::FU - 1 - 2 * m];
            if (m < TU_PIN) st.tuP[m] = (v2f){pin_sgpr(f1 * gU), pin_sgpr(f0 * gU)};
            else st.tuP[m] = (v2f){to_sgpr(f1 * gU), to_sgpr(f0 * gU)};
        }
        if (RDOWN) {
#pragma unroll
            for (int m = 0; m < Cfg::FD / 2; m++) st.tdP[m] = splat(0.f);      // unused: the 12x12 taps stream from the scalar cache
        } else {
#pragma unroll
            for (int m = 0; m < Cfg::FD / 2; m++) {
                const float f0 = p.fd[p.flip ? 2 * m : Cfg::FD - 1 - 2 * m], f1 = p.fd[p.flip ? 2 * m + 1 : Cfg::FD - 2 - 2 * m];
                st.tdP[m] = (v2f){to_sgpr(f0), to_sgpr(f1)};
            }
        }

        // horizontal geometry: first upsampled column of the strip, shifted left by delta so that every lane's
        // U-column groups start at an upsampled position == 1 (mod U) and share one input window
        const int delta = ((D * ox0 - p.px0 - 1) % U + U) % U;
        const int uxs = D * ox0 - delta;
        const int ibase = floor_div(uxs - p.px0 - 1, U) + 1;
#pragma unroll
        for (int q = 0; q < Cfg::NL; q++) {
            if (G > 1) {
                // staging slot e of the LDS row: plane e / PSEG, sample e % PSEG of that plane's window
                // (one-plane blocks: the whole row is that plane's)
                const int e = lane + 64 * q, g = (two && e >= Cfg::PSEG) ? 1 : 0;
                const int ix = ibase + e - g * Cfg::PSEG;
                const bool ok = (wide || e < 2 * Cfg::PSEG) && (unsigned)ix < (unsigned)p.xW && (g == 0 || second);
                st.coff[q] = ok ? (g * (int)p.xsC + ix) * (int)sizeof(T) : (int)0x80000000;
                st.bcol[q] = ok ? (g ? bias1 : bias) : 0.f;
                continue;
            }
            const int ix = ibase + lane + 64 * q;
            st.coff[q] = ix * (int)sizeof(T);                  // negative / beyond the row -> out of range -> reads 0
            st.bcol[q] = ((unsigned)ix < (unsigned)p.xW) ? bias : 0.f;
        }
        if (G > 1) {
            const int g = two ? lane >> 5 : 0, ll = two ? lane & 31 : lane;
            st.inBase = g * Cfg::PSEG + Cfg::GROUPS * ll;
            st.outBase = g * Cfg::POSEG + 4 * ll;
            const bool mine = g == 0 || second;
            st.ooff[0] = (mine && 2 * ll < oxN) ? (g * (int)p.ysC + 2 * ll) * (int)sizeof(T) : (int)0x80000000;
            st.ooff[1] = (mine && 2 * ll + 1 < oxN) ? (g * (int)p.ysC + 2 * ll + 1) * (int)sizeof(T) : (int)0x80000000;
        }

        st.osum = 0.f;
        st.omax = 0.f;
        st.xmax = 0.f;
        float liveGain = p.gain;                  // the output gain; NaN from the row on in which this wave staged a non-finite sample
        float liveGain1 = p.gain;                 // packed mode: the second plane's
        if (SIGNS) {
            const int c0 = uxs + p.sx;                           // sign-tensor column of lane 0's first upsampled column
            st.sq = to_sgpr_i(((c0 % 4) + 4) % 4);
            st.soff = floor_div(c0, 4) + lane;
        } else {
            st.sq = 0; st.soff = 0;
        }

        // vertical geometry
        const int uyA = oy0 * D;
        const int uyB = (oy1 - 1) * D + Cfg::FD - 1;
        int iFirst = ceil_div_s(uyA - p.py0, U);                // first input row of the window that yields uyA
        if ((U * (iFirst - 5)) % D != 0) iFirst -= 1;           // trips start at down phase VPH: U * (iFirst - 5) = 0 (mod D)
        const int iLast = ceil_div_s(uyB - p.py0, U) + 5;       // step that yields uyB
        const int nBlocks = (iLast - iFirst + 1 + 5) / 6;

        // Plain forward: the chunk runs first with the one-instruction activation, every staged sample tested against the threshold
        // (a wave-uniform choice made once, before the row loop: a branch inside it costs 5 %); a wave that met a sample above it --
        // or a NaN, or an infinity -- runs the chunk again with lrelu + clamp and the NaN guard, rewriting every output it stored.
        // Either way the outputs are those of the second form, bit for bit.
        // The fast pass's flag: the lanes' running maximum |staged sample| against the threshold (separable forms); its output gain,
        // 0 from the row of a failed test on (radial and WIDE forms; fastAct promises a finite positive gain).
        bool slow = true;
        if constexpr (SIGNS == 0) {
            const float fastT = p.fastAct ? to_sgpr(fast_threshold(p.fu, Cfg::FU, U, p.gain, p.slope, p.clamp)) : -1.f;
            if (fastT > 0.f) {
                float fastGain = p.gain, unused = p.gain;
                stream_chunk<true>(st, p, plane, oplane, splane, sIn, sOut, iFirst, nBlocks, delta, lane, oy0, oy1, ox0, oxN, pairStore, fastGain,
                                   unused, wide, fastT);
                if (PLAIN) {
                    // |x| <= T on every sample every lane staged?  v_cmp_nle is true for a maximum above T, an infinity and a NaN alike
                    unsigned long long m;
                    asm("v_cmp_nle_f32_e64 %0, %1, %2" : "=s"(m) : "v"(st.xmax), "s"(fastT));
                    slow = m != 0ull;
                } else {
                    slow = fastGain != p.gain;
                }
            }
        }
        if (slow)
            stream_chunk<false>(st, p, plane, oplane, splane, sIn, sOut, iFirst, nBlocks, delta, lane, oy0, oy1, ox0, oxN, pairStore, liveGain, liveGain1,
                                wide, -1.f);
#ifdef SG3_STAMPS
        if (p.stamps && lane == 0) {
            p.stamps[2 * (long long)blockIdx.x] = __builtin_amdgcn_s_memtime() - stampC;
            p.stamps[2 * (long long)blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stampR;
        }
#endif
        if (SIGNS == 2 && p.ysum) {                         // bias gradient of the adjoint pass
            float v = st.osum;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
            if (lane == 0) p.ysum[(long long)plane_id * (p.nChunks * p.nStrips) + chunk * p.nStrips + strip] = v;
        }
        if (SIGNS == 2 && p.ymax) {                         // max |dx| of the adjoint pass
            float v = st.omax;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) v = __builtin_fmaxf(v, __shfl_xor(v, m));
            // the maximum of what was STORED: v is the largest fp32 result, and rounding to T is monotone, so its rounding is the largest
            // stored value (fp16 tensors: up to 2^-11 above v -- a reader that takes v for a bound on |dx| would be told too little)
            if (lane == 0) p.ymax[(long long)plane_id * (p.nChunks * p.nStrips) + chunk * p.nStrips + strip] = (float)(T)v;
        }
    }
};

template <typename T, int U, int D, int VPH, int RADIAL, int SIGNS, int G = 1, int WIDE = 0>
__global__ void __launch_bounds__(64)
flrelu_stream_kernel(StreamParams p) {
    Stream<T, U, D, VPH, RADIAL, SIGNS, G, WIDE>::run(p);
}

// ---------------------------------------------------------------------------
// The kernel of one plan entry.  This is where the kernels' addresses are taken, so this is where they are instantiated.
template <typename T, int U, int D, int R, int S, int G, int W, int... V>
static StreamKernel stream_kernel_vph(int vph, std::integer_sequence<int, V...>) {
    StreamKernel f = nullptr;
    ((vph == V ? (void)(f = flrelu_stream_kernel<T, U, D, V, R, S, G, W>) : (void)0), ...);
    return f;
}
// a trip starts at any of the D down phases
template <typename T, int U, int D, int R, int S, int G, int W>
StreamKernel stream_kernel_leaf(int vph) {
    return stream_kernel_vph<T, U, D, R, S, G, W>(vph, std::make_integer_sequence<int, D>());
}

// ---------------------------------------------------------------------------
// The part table: every leaf <T, U, D, R, S, G, W> the host's lookup can ask for (38 per tensor type, 82 kernels), each in exactly
// one part.  Part = 6 * (tensor type: float 0, half 1) + family:
//   0  plain forward, separable filters (both up factors, one and two planes per wave, the WIDE forms): the 24 kernels whose
//      assembly tests/test_flrelu_isa_budget_cpu.py and tests/test_flrelu_up4_resources_cpu.py read (parts 0 and 6)
//   1  plain forward, 12x12 down filter (RADIAL 1)
//   2  the same, flipped (RADIAL 2)
//   3  plain forward, 12x12 down filter with mirror-symmetric rows (RADIAL 5 | 6)
//   4  the adjoints, and the sign-writing forward with separable filters
//   5  the sign-writing forward with a 12x12 down filter
// cut by measured compile time: no part takes as long as sg3_modconv.hip; the whole file in one piece takes minutes.
//
// A kernel compiles to the same instructions in its part as in the whole file only while the part keeps the VARIETY of constants
// the whole file passes to the helpers that are not force-inlined -- floor_div / ceil_div_s (sg3_common.h) with b = U, and
// fast_threshold with (taps, up) = (6 U, U) from the plain forward.  They have internal linkage, so when every call in the
// translation unit passes the same constant, interprocedural constant propagation puts it into the helper's body before the
// inliner runs, and the prologue arithmetic comes out in another shape (the scalar registers behind it shift by one or two, a scalar
// spill appears or goes: 164 of 164 kernels differed when each leaf was compiled alone, none does with these parts).  Hence every
// part holds up-2 AND up-4 leaves, and a part that holds plain-forward leaves holds them of both up factors.
#ifndef SG3_FLRELU_PART
#define SG3_FLRELU_PART -1                       // every part: the tools and the dispatch recorder include this file as it stands
#endif
#define SG3_FLRELU_HERE(k) (SG3_FLRELU_PART < 0 || SG3_FLRELU_PART == (k))
#define LEAF(T, U, D, R, S, G, W) template StreamKernel stream_kernel_leaf<T, U, D, R, S, G, W>(int);
#define LEAVES_PLAIN_SEPARABLE(T) \
    LEAF(T, 4, 2, 0, 0, 1, 1) LEAF(T, 4, 2, 0, 0, 2, 1) LEAF(T, 2, 2, 0, 0, 1, 0) LEAF(T, 4, 2, 0, 0, 1, 0) LEAF(T, 2, 2, 0, 0, 2, 0) LEAF(T, 4, 2, 0, 0, 2, 0)
#define LEAVES_PLAIN_RADIAL(T, R) LEAF(T, 2, 2, R, 0, 1, 0) LEAF(T, 4, 2, R, 0, 1, 0) LEAF(T, 2, 2, R, 0, 2, 0) LEAF(T, 4, 2, R, 0, 2, 0)
#define LEAVES_ADJOINT_AND_SEPARABLE_SIGNS(T) \
    LEAF(T, 2, 2, 0, 2, 1, 0) LEAF(T, 2, 2, 3, 2, 1, 0) LEAF(T, 2, 2, 4, 2, 1, 0) LEAF(T, 2, 4, 0, 2, 1, 0) LEAF(T, 2, 4, 3, 2, 1, 0) LEAF(T, 2, 4, 4, 2, 1, 0) \
    LEAF(T, 2, 2, 0, 1, 1, 0) LEAF(T, 4, 2, 0, 1, 1, 0)
#define LEAVES_RADIAL_SIGNS(T) \
    LEAF(T, 2, 2, 1, 1, 1, 0) LEAF(T, 2, 2, 2, 1, 1, 0) LEAF(T, 2, 2, 5, 1, 1, 0) LEAF(T, 2, 2, 6, 1, 1, 0) \
    LEAF(T, 4, 2, 1, 1, 1, 0) LEAF(T, 4, 2, 2, 1, 1, 0) LEAF(T, 4, 2, 5, 1, 1, 0) LEAF(T, 4, 2, 6, 1, 1, 0)
#if SG3_FLRELU_HERE(0)
LEAVES_PLAIN_SEPARABLE(float)
#endif
#if SG3_FLRELU_HERE(1)
LEAVES_PLAIN_RADIAL(float, 1)
#endif
#if SG3_FLRELU_HERE(2)
LEAVES_PLAIN_RADIAL(float, 2)
#endif
#if SG3_FLRELU_HERE(3)
LEAVES_PLAIN_RADIAL(float, 5) LEAVES_PLAIN_RADIAL(float, 6)
#endif
#if SG3_FLRELU_HERE(4)
LEAVES_ADJOINT_AND_SEPARABLE_SIGNS(float)
#endif
#if SG3_FLRELU_HERE(5)
LEAVES_RADIAL_SIGNS(float)
#endif
#if SG3_FLRELU_HERE(6)
LEAVES_PLAIN_SEPARABLE(_Float16)
#endif
#if SG3_FLRELU_HERE(7)
LEAVES_PLAIN_RADIAL(_Float16, 1)
#endif
#if SG3_FLRELU_HERE(8)
LEAVES_PLAIN_RADIAL(_Float16, 2)
#endif
#if SG3_FLRELU_HERE(9)
LEAVES_PLAIN_RADIAL(_Float16, 5) LEAVES_PLAIN_RADIAL(_Float16, 6)
#endif
#if SG3_FLRELU_HERE(10)
LEAVES_ADJOINT_AND_SEPARABLE_SIGNS(_Float16)
#endif
#if SG3_FLRELU_HERE(11)
LEAVES_RADIAL_SIGNS(_Float16)
#endif
#if SG3_FLRELU_PART > 11
#error "sg3_filtered_lrelu.hip has parts 0 .. 11 (csrc/Makefile: FLRELU_PARTS)"
#endif
#undef LEAVES_RADIAL_SIGNS
#undef LEAVES_ADJOINT_AND_SEPARABLE_SIGNS
#undef LEAVES_PLAIN_RADIAL
#undef LEAVES_PLAIN_SEPARABLE
#undef LEAF

} // namespace sg3
