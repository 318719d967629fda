/*
 * sg3_ops.h -- C ABI of libsg3hip.so, the MI355X (gfx950) replacement for the
 * native plugins behind krylea/stylegan3-editing's `torch_utils.ops` package.
 *
 * Boundary rules (all entry points):
 *   - plain C: raw device pointers, sizes, strides; no torch / C++ types.
 *   - the CALLER owns and allocates every buffer (inputs, outputs, sign
 *     tensors) and computes their sizes with the sg3_*_shape helpers below
 *     (host-only, no GPU needed);
 *   - every launch is asynchronous on the `hipStream_t` passed as `void*
 *     stream` (NULL = the null stream); no call synchronises, allocates or
 *     keeps state between calls, so concurrent streams are safe (the
 *     reference keeps its taps in one global __constant__ buffer and is not:
 *     reference torch_utils/ops/filtered_lrelu.py:216-217);
 *   - return value: SG3_OK (0) on success, SG3_NO_KERNEL (-1) when no
 *     specialised kernel exists for the (up, down, taps) tuple -- the same
 *     meaning as the reference's rc (reference torch_utils/ops/
 *     filtered_lrelu.cpp:52-56) -- and < -1 for an invalid argument or a HIP
 *     launch error; sg3_last_error() returns a thread-local message.
 *
 * Each function cites the reference interface it replaces (paths relative to
 * the reference tree).
 */
#ifndef SG3_OPS_H
#define SG3_OPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG3_ABI_VERSION 1

/* exported from libsg3hip.so (the library is built with -fvisibility=hidden) */
#if defined(__GNUC__)
#define SG3_API __attribute__((visibility("default")))
#else
#define SG3_API
#endif

enum {
    SG3_OK          =  0,
    SG3_NO_KERNEL   = -1,  /* no specialised kernel: caller uses the generic composition */
    SG3_BAD_ARG     = -2,
    SG3_HIP_ERROR   = -3,
};

/* element types of activation tensors */
enum {
    SG3_F32 = 0,
    SG3_F16 = 1,
    SG3_F64 = 2,   /* bias_act / upfirdn2d / filtered_lrelu_act only */
};

SG3_API int         sg3_abi_version(void);
SG3_API const char* sg3_last_error(void);
/* number of HIP devices visible to the library (0 on a CPU-only host; never fails) */
SG3_API int         sg3_device_count(void);

/* ------------------------------------------------------------------------
 * filtered_lrelu  -- replaces filtered_lrelu_plugin.filtered_lrelu
 *   (torch_utils/ops/filtered_lrelu.cpp:16-209; parameter block
 *    torch_utils/ops/filtered_lrelu.h:14-53).
 *
 *   y = down_fd( clamp( lrelu( up_fu(x + b) * up^2 * gain ) ) )
 *
 * Shapes are NCHW; strides are in ELEMENTS (not bytes), order n,c,h,w.
 * fu/fd are float32 device arrays.  fuH == 0 (fdH == 0) means a separable
 * filter of fuW (fdW) taps applied along both axes; otherwise a full
 * fuH x fuW filter with row stride fuW.
 * signs: uint8 [N, C, sH, sWbytes], 2 bits per element of the upsampled
 * buffer (bit0 = negative, value 2 = clamped), 4 elements per byte along x
 * (torch_utils/ops/filtered_lrelu.cpp:87-94).  NULL when unused.
 * ---------------------------------------------------------------------- */
typedef struct sg3_filtered_lrelu_params {
    const void*    x;          /* [N,C,xH,xW] */
    void*          y;          /* [N,C,yH,yW] */
    const void*    b;          /* [C] bias, same dtype as x, or NULL (no bias) */
    uint8_t*       s;          /* sign tensor or NULL */
    const float*   fu;         /* upsampling taps */
    const float*   fd;         /* downsampling taps */
    int32_t        dtype;      /* SG3_F32 | SG3_F16 */
    int32_t        N, C;
    int32_t        xH, xW;
    int32_t        yH, yW;
    int64_t        xStride[4]; /* elements, n,c,h,w */
    int64_t        yStride[4];
    int64_t        bStride;
    int32_t        up, down;
    int32_t        fuW, fuH;   /* fuH == 0: separable */
    int32_t        fdW, fdH;
    int32_t        px0, py0;   /* left / top padding w.r.t. the upsampled image */
    int32_t        sH;         /* sign tensor height (rows) */
    int32_t        sWbytes;    /* sign tensor row pitch in bytes */
    int32_t        sx, sy;     /* offset between upsampled buffer and sign tensor */
    int32_t        swLimit;    /* active width of the sign tensor in bytes */
    float          gain;
    float          slope;
    float          clamp;      /* +inf = no clamp */
    int32_t        flip;       /* 1 = correlation (flip_filter=True) */
    int32_t        writeSigns;
    int32_t        readSigns;
    float*         ySumPartial; /* optional, readSigns calls only: [N*C, sg3_filtered_lrelu_sum_slots(...)] per-workgroup sums of
                                 * the outputs of each plane.  The caller adds them up: the bias gradient db = dx.sum([0,2,3])
                                 * of the adjoint pass (torch_utils/ops/filtered_lrelu.py:266-267) without re-reading dx */
    int32_t        fdMirror;    /* caller's promise about a 2-D down filter: fd[r][c] == fd[r][fdW-1-c] bit for bit (true of the
                                 * radial filters design_lowpass_filter builds, networks_stylegan3.py:370-391).  The kernel then
                                 * adds the two samples that share a tap before multiplying: 42 instead of 72 packed operations per
                                 * upsampled row and lane.  0 = no assumption */
    float*         yAbsMaxPartial; /* optional, readSigns calls only, same shape as ySumPartial: per-workgroup max |output| of the
                                 * values as STORED (fp16 tensors: after their rounding).  Their maximum is max |dx| of the adjoint
                                 * pass: the operand bound the split-precision gradient kernels of the convolution in front need
                                 * (sg3_conv2d_wgrad's amax mode), without a pass over dx */
} sg3_filtered_lrelu_params;

SG3_API int sg3_filtered_lrelu(const sg3_filtered_lrelu_params* p, void* stream);

/* number of partial sums per (n,c) plane that sg3_filtered_lrelu writes to ySumPartial for this output shape */
SG3_API int sg3_filtered_lrelu_sum_slots(int N, int C, int yH, int yW, int down);

/* db[c] = sum over (n, slot) of sumPartial[n][c][slot] (float32 [C]) and, when given, absMax[0] = max over absMaxPartial: the
 * per-workgroup values of one readSigns call folded in one small launch (fixed summation order) */
SG3_API int sg3_filtered_lrelu_finish_partials(const float* sumPartial, const float* absMaxPartial, int N, int C, int slots,
                                               float* db, float* absMax, void* stream);

/* Host-only query: how many (n,c) planes one wave of the streaming kernel works on for this call -- 2 for the plain forward on
 * narrow dense planes (output at most 54 columns wide, even C: the 36^2 .. 52^2 layers); 3 = mixed: rows cut into 120-column
 * strips with one plane per wave plus a remainder strip of at most 54 columns with two (the 148^2 .. 532^2 layers); 1 otherwise;
 * 0 when the call does not take the streaming kernel.  For tests and profiling; no reference counterpart. */
SG3_API int sg3_filtered_lrelu_planes_per_wave(const sg3_filtered_lrelu_params* p);

/* Diagnostic: the up-4 separable plain forward (fp32 / fp16) has two forms with bit-identical outputs -- the default, which holds
 * its up taps in scalar registers and single vector register pairs and runs four waves per SIMD, and the earlier, wider one (three
 * waves).  wide != 0 routes every later up-4 launch of the process to the earlier form, 0 back to the default; returns the previous
 * setting.  A process setting made by an explicit call (the bit-identity test, A/B timing) -- not an environment variable read per
 * launch, which could differ between a graph capture and a later eager call.  SG3_FLRELU_UP4_WIDE=1 in the environment seeds it once. */
SG3_API int sg3_filtered_lrelu_force_up4_wide(int wide);

/* Host-only query: the work decomposition `sg3_filtered_lrelu` launches for this call, from the functions the launch itself uses.
 * Output rows are cut into nChunks chunks of chunkRows rows (the last one shorter); output columns into nStrips strips: equal strips
 * of stripW columns (nFullStrips = 0), or nFullStrips strips of stripW = 120 columns, one plane per wave, followed by one remainder
 * strip with two planes per wave (planes_per_wave = 3).  ySumPartial / yAbsMaxPartial slot of a workgroup: chunk * nStrips + strip.
 * Returns 1, or 0 (nothing written) when the call does not take the streaming kernel.  For tests; no reference counterpart. */
SG3_API int sg3_filtered_lrelu_stream_grid(const sg3_filtered_lrelu_params* p, int* nStrips, int* stripW, int* nFullStrips, int* nChunks,
                                           int* chunkRows);

/* kinds of launch of sg3_filtered_lrelu */
enum {
    SG3_FLRELU_NONE      = 0,   /* no fused kernel (SG3_NO_KERNEL) */
    SG3_FLRELU_POINTWISE = 1,   /* flrelu_pointwise_kernel<T>: up = down = 1, 1x1 filters; totalBlocks[0] workgroups of 256 */
    SG3_FLRELU_STREAM    = 2,   /* flrelu_stream_kernel<T, U, D, VPH, RADIAL, SIGNS, G, WIDE>: workgroups of one wave */
};

/* What sg3_filtered_lrelu launches for a call: the kind, and per launch ([0], and [1] of the two-launch mixed form) the template
 * coordinates of the streaming kernel and its work decomposition. */
typedef struct sg3_filtered_lrelu_dispatch_info {
    int32_t        kind;          /* SG3_FLRELU_* */
    int32_t        launches;      /* 1 | 2; 0: none, or a grid that would pass 2^31 - 1 workgroups (SG3_BAD_ARG) */
    int32_t        planesPerWave; /* sg3_filtered_lrelu_planes_per_wave */
    int32_t        nChunks, chunkRows; /* output rows: nChunks chunks of chunkRows rows, both launches */
    int32_t        sumSlots;      /* readSigns calls: ySumPartial / yAbsMaxPartial values per plane (sg3_filtered_lrelu_sum_slots), else 0 */
    int32_t        fastAct;       /* 1: the plain forward tries the one-instruction activation first */
    int32_t        U[2], D[2], VPH[2], RADIAL[2], SIGNS[2], G[2], WIDE[2];
    int32_t        nStrips[2], TW[2];  /* strips of TW output columns */
    int32_t        ox0Base[2];    /* first output column of the two-plane strip */
    int32_t        wideBlocks[2]; /* G = 2: leading workgroups that take one plane each, on the full strips */
    int32_t        totalBlocks[2]; /* the grid */
} sg3_filtered_lrelu_dispatch_info;

/* The plan of a call, from the function the launch itself uses (host only: no launch, no pointer followed -- only whether s is set
 * and the alignment of 2-D taps is read, so placeholders do; x, y, fu and fd may be NULL).  Returns what sg3_filtered_lrelu would
 * return before launching: SG3_OK, SG3_NO_KERNEL, or SG3_BAD_ARG for a call it rejects. */
SG3_API int sg3_filtered_lrelu_dispatch(const sg3_filtered_lrelu_params* p, sg3_filtered_lrelu_dispatch_info* out);

/* host-only: the bound on |input + bias| under which the plain forward's streaming kernel evaluates lrelu + clamp as one
 * med3(u, slope*u, clamp/gain) -- the same computation the kernel makes from the separable up filter fu (fuW taps, HOST
 * memory here).  -1 when there is none (clamp/gain not positive). */
SG3_API float sg3_filtered_lrelu_fast_threshold(const float* fu, int fuW, int up, float gain, float slope, float clamp);

/* 1 when sg3_filtered_lrelu has a fused kernel for this tuple (host-only
 * query; mirrors the reference's choose_filtered_lrelu_kernel test call,
 * torch_utils/ops/filtered_lrelu.cpp:46-56). */
SG3_API int sg3_filtered_lrelu_has_kernel(int up, int down, int fuW, int fuH, int fdW, int fdH);

/* Output / sign-tensor geometry exactly as the reference host code derives it
 * (torch_utils/ops/filtered_lrelu.cpp:59-98).  Returns SG3_BAD_ARG when the
 * reference would raise.  Any out pointer may be NULL. */
SG3_API int sg3_filtered_lrelu_shape(int xH, int xW, int up, int down,
                             int fuW, int fuH, int fdW, int fdH,
                             int px0, int px1, int py0, int py1,
                             int* yH, int* yW,
                             int* sH, int* sWbytes, int* swLimit);

/* ------------------------------------------------------------------------
 * filtered_lrelu_act  -- replaces filtered_lrelu_plugin.filtered_lrelu_act_
 *   (torch_utils/ops/filtered_lrelu.cpp:213-290; filtered_lrelu.h:55-68).
 * In-place gain * lrelu * clamp on x with optional sign write / read.
 * sW is the sign tensor width in ELEMENTS (multiple of 16).
 * ---------------------------------------------------------------------- */
typedef struct sg3_filtered_lrelu_act_params {
    void*          x;          /* [N,C,H,W], modified in place */
    uint8_t*       s;          /* [N,C,sH,sW/4] or NULL */
    int32_t        dtype;      /* SG3_F32 | SG3_F16 | SG3_F64 */
    int32_t        N, C, H, W;
    int64_t        xStride[4]; /* elements */
    int32_t        sH, sW;
    int32_t        sx, sy;
    float          gain, slope, clamp;
    int32_t        writeSigns;
    int32_t        readSigns;
} sg3_filtered_lrelu_act_params;

SG3_API int sg3_filtered_lrelu_act(const sg3_filtered_lrelu_act_params* p, void* stream);

/* ------------------------------------------------------------------------
 * upfirdn2d  -- replaces upfirdn2d_plugin.upfirdn2d
 *   (torch_utils/ops/upfirdn2d.cpp:16-98; upfirdn2d.h:14-40).
 * f is a rank-2 float32 filter [fH, fW] with element strides fStride[2]
 * (h, w).  Separable filters are two calls, as in the reference Python
 * (torch_utils/ops/upfirdn2d.py:244-246).
 * ---------------------------------------------------------------------- */
typedef struct sg3_upfirdn2d_params {
    const void*    x;          /* [N,C,xH,xW] */
    const float*   f;          /* [fH,fW] */
    void*          y;          /* [N,C,yH,yW] */
    int32_t        dtype;      /* SG3_F32 | SG3_F16 | SG3_F64 */
    int32_t        N, C, xH, xW, yH, yW;
    int64_t        xStride[4];
    int64_t        yStride[4];
    int32_t        fH, fW;
    int64_t        fStride[2];
    int32_t        upx, upy, downx, downy;
    int32_t        padx0, pady0;
    int32_t        flip;
    float          gain;
} sg3_upfirdn2d_params;

SG3_API int sg3_upfirdn2d(const sg3_upfirdn2d_params* p, void* stream);

SG3_API int sg3_upfirdn2d_shape(int xH, int xW, int fH, int fW,
                        int upx, int upy, int downx, int downy,
                        int padx0, int padx1, int pady0, int pady1,
                        int* yH, int* yW);

/* ------------------------------------------------------------------------
 * bias_act  -- replaces bias_act_plugin.bias_act
 *   (torch_utils/ops/bias_act.cpp:32-92; bias_act.h:12-31; kernel semantics
 *    torch_utils/ops/bias_act.cu:23-147).
 * x is dense with `sizeX` elements; b (or NULL) has sizeB elements and
 * element i of x uses b[(i / stepB) % sizeB].  grad = 0 forward, 1 first
 * derivative, 2 second derivative.  act = 1..9 in the reference's order
 * (linear, relu, lrelu, tanh, sigmoid, elu, selu, softplus, swish).
 * clamp < 0 = none.
 * ---------------------------------------------------------------------- */
typedef struct sg3_bias_act_params {
    const void*    x;
    const void*    b;
    const void*    xref;
    const void*    yref;
    const void*    dy;
    void*          y;
    int32_t        dtype;      /* SG3_F32 | SG3_F16 | SG3_F64 */
    int32_t        grad;
    int32_t        act;
    float          alpha, gain, clamp;
    int64_t        sizeX;
    int32_t        sizeB;
    int32_t        stepB;
} sg3_bias_act_params;

SG3_API int sg3_bias_act(const sg3_bias_act_params* p, void* stream);

/* ------------------------------------------------------------------------
 * fourier_features -- the input features of SynthesisInput.forward
 *   (models/stylegan3/networks_stylegan3.py:236-241), channels-first:
 *
 *   out[n,c,y,x] = sin((grid[y,x,0]*freqs[n,c,0] + grid[y,x,1]*freqs[n,c,1]
 *                       + phases[n,c]) * 2*pi) * amps[n,c]
 *
 * `grid` is the sampling grid the caller built (F.affine_grid, :233-234),
 * `freqs` / `phases` / `amps` the transformed frequencies, phases and
 * amplitudes (:222-230).  Operation order as in the reference's torch ops,
 * so the result is bit-identical to them.  float32 only.
 * ---------------------------------------------------------------------- */
typedef struct sg3_fourier_params {
    const float*   grid;       /* [H,W,2] */
    const float*   freqs;      /* [N,C,2] */
    const float*   phases;     /* [N,C] */
    const float*   amps;       /* [N,C] */
    float*         out;        /* [N,C,H,W] */
    int32_t        N, C, H, W;
} sg3_fourier_params;

SG3_API int sg3_fourier_features(const sg3_fourier_params* p, void* stream);

/* ------------------------------------------------------------------------
 * input_transform -- the per-sample frequencies / phases / amplitudes of
 *   SynthesisInput.forward (models/stylegan3/networks_stylegan3.py:204-230): t' = t / |t[:2]| (when `normalise`; :206),
 *   M = R(t') @ T(t') @ user (:213-221), phases + freqs @ M[:2,2:], freqs @ M[:2,:2] (:224-225), amplitude fade-out (:228).
 *   One launch instead of ~35 small torch ops; products are formed k-ascending with one rounding per step like the
 *   reference's fp32 matmuls (differences, if any, are single roundings).  float32.
 * ---------------------------------------------------------------------- */
typedef struct sg3_input_transform_params {
    const float*   t;          /* [N,4] affine output (r_c, r_s, t_x, t_y) */
    const float*   user;       /* [3,3] (userStrideN = 0) or [N,3,3] (userStrideN = 9): SynthesisInput.transform */
    const float*   freqs;      /* [C,2] */
    const float*   phases;     /* [C] */
    float*         outFreqs;   /* [N,C,2] */
    float*         outPhases;  /* [N,C] */
    float*         outAmps;    /* [N,C] */
    int32_t        N, C;
    int32_t        normalise;  /* 1: divide t by |t[:2]| first (t straight from the affine layer) */
    int32_t        userStrideN;
    float          bandwidth, samplingRate;
} sg3_input_transform_params;

SG3_API int sg3_input_transform(const sg3_input_transform_params* p, void* stream);

/* ------------------------------------------------------------------------
 * affine_batch -- the affine layers (FullyConnectedLayer, linear activation) of every synthesis layer in one launch:
 *   out_j[n, i] = (ws[n, wsIndex[j], :] . weight[rowStart[j] + i, :] + bias[rowStart[j] + i]) * scale[rowStart[j] + i]
 *   (networks_stylegan3.py:88-96 per layer, called at :205 and :349; the ToRGB gain of :350-352 is `scale`).
 *   `weight` holds all layers' matrices one after the other with weight_gain already applied (`weight * weight_gain`, one
 *   rounding, as :89), `bias` likewise (`bias * bias_gain`).  Layer j's result is the dense block [N, C_j] at
 *   out + N * rowStart[j].  float32; the dot product is accumulated in another order than the BLAS call's (1e-7 relative).
 * ---------------------------------------------------------------------- */
typedef struct sg3_affine_batch_params {
    const float*   ws;         /* latents: element (n, l, k) at ws[n * wsStrideN + l * wsStrideL + k] */
    int64_t        wsStrideN, wsStrideL;
    const float*   weight;     /* [rows, wDim] */
    const float*   bias;       /* [rows] or NULL */
    const float*   scale;      /* [rows] or NULL (= 1) */
    const int32_t* rowStart;   /* [layers + 1] DEVICE array: first row of each layer, rowStart[layers] = rows */
    const int32_t* wsIndex;    /* [layers] DEVICE array: which latent each layer reads */
    float*         out;        /* [N * rows] */
    int32_t        N, wDim, layers, rows;
} sg3_affine_batch_params;

SG3_API int sg3_affine_batch(const sg3_affine_batch_params* p, void* stream);

/* ------------------------------------------------------------------------
 * modulated_conv2d -- replaces the grouped F.conv2d behind
 *   models/stylegan3/networks_stylegan3.py:24-63 (modulated_conv2d), reached
 *   through torch_utils/ops/conv2d_gradfix.py:36-39.
 *
 *   out[n,o,:,:] = dcoef[n,o] * sum_{i,ky,kx} wn[o,i,ky,kx] *
 *                  (x[n,i,:,:] * sIn[n,i]) (zero padded by `pad`)
 *
 * i.e. the per-sample modulation is applied to the INPUT channels and the
 * demodulation to the OUTPUT channels, so the whole batch shares one weight
 * matrix and runs as a single implicit GEMM (M = O, N = batch*pixels,
 * K = I*k*k) on the fp32 matrix cores (v_mfma_f32_32x32x2_f32, exact fp32).
 * Two calls:
 *   sg3_modulated_conv2d_prep  -> wPacked, sIn, dcoef   (tiny)
 *   sg3_modulated_conv2d       -> out
 * x / out are NCHW contiguous, dtype f32 or f16; accumulation is fp32.
 * outH = H + 2*pad - k + 1.  k is 1 or 3.
 * ---------------------------------------------------------------------- */

/* arithmetic of the implicit GEMM */
enum {
    SG3_CONV_FP32  = 0,  /* v_mfma_f32_32x32x2_f32: exact fp32 products */
    SG3_CONV_F16X3 = 1,  /* operands split x = hi + lo into two fp16 halves; hi*hi + hi*lo + lo*hi on
                          * v_mfma_f32_32x32x16_f16 with fp32 accumulation: every retained product is exact, the
                          * dropped lo*lo term is 2^-22 relative (fp32-equivalent), 5.3x the fp32 MFMA rate.
                          * needs a bound on |x| (xBound) to keep the halves in fp16 range */
    SG3_CONV_F16   = 2,  /* operands rounded to fp16 once, one v_mfma_f32_32x32x16_f16 per K step, fp32 accumulation:
                          * the arithmetic of the reference's fp16 layers (networks_stylegan3.py:59-62 with fp16 x and
                          * w.to(x.dtype)); same packing, xBound and power-of-two rescale as SG3_CONV_F16X3 */
    SG3_CONV_F16X3_F23 = 3, /* SG3_CONV_F16X3 in a transform domain along x (Winograd F(2,3): per pair of output columns four
                          * transform points of a 3-tap vertical filter instead of 2 x 9 taps): two thirds of the matrix
                          * instructions, the same split arithmetic on the transformed operands (inputs transformed in fp32 before
                          * the split, weights at pack time).  3x3 kernels on fp32 tensors with even W, pad and output row pitch
                          * only (sg3_modconv_f23_supported); its own packed layout, so prep and convolution must agree */
    SG3_CONV_FP32_CHAINS = 5, /* sg3_conv2d only: SG3_CONV_FP32 on the same packed weights with four accumulation chains per output
                          * (summed pairwise at the end) instead of one: a quarter of the rounding-error growth along K, for the
                          * recorded forward of encoder training; 64- and 32-channel tiles */
    SG3_CONV_F16_F23 = 4, /* SG3_CONV_F16 in the same transform domain, for fp16 tensors (the reference's `use_fp16` layers,
                          * networks_stylegan3.py:355-366): transformed inputs and weights rounded to fp16 once, one product per K step,
                          * fp32 accumulation, fp16 output.  Same shape rules; packed layout without lo fragments (half the size) */
};

/* 1 when sg3_modulated_conv2d takes this call with precision SG3_CONV_F16X3_F23 (dtype SG3_F32) / SG3_CONV_F16_F23 (dtype SG3_F16)
 * (host-only query, no launch) */
SG3_API int sg3_modconv_f23_supported(int dtype, int I, int O, int H, int W, int k, int pad, int outRowStride);

/* Diagnostic: force the rows-per-wave of the SG3_CONV_F16X3_F23 kernel (4 | 5 | 7; 0 = the launcher's own cost model, the default)
 * for every later launch of the process; returns the previous setting.  The tile height fixes the order of a tile's sums, so it is a
 * process setting made by an explicit call (tests walk all three heights; tools/ A/B runs) -- not an environment variable read per
 * launch, which could differ between a graph capture and a later eager call.  The environment variable SG3_F23_TN seeds it once. */
SG3_API int sg3_modconv_f23_force_rows(int rows);

/* number of floats (4-byte units) of the packed weight buffer for an [O,I,k,k] weight
 * (fp32: [O][ceil(I/KC)][k*k][KC] floats; f16x3 / f16: [O][chunks][k*k][hi|lo][16] halfs, chunks = ceil(I/16), rounded up to even for k = 1; zero padded). */
SG3_API int64_t sg3_modconv_packed_floats(int O, int I, int k, int precision);

/* Demodulation coefficients and input scales
 * (models/stylegan3/networks_stylegan3.py:39-56):
 *   wn    = w * rsqrt(mean(w^2 over I,k,k))          (per O)    -> wPacked
 *   sn    = s * rsqrt(mean(s^2 over N,I))
 *   dcoef = rsqrt( sum_{i,k} (wn[o,i,k] * sn[n,i])^2 + 1e-8 )   -> dcoef [N,O]
 *   sIn   = sn * inputGain                                      -> sIn [N,I]
 * With demodulate == 0: wn = w, sn = s, dcoef is not written.
 * inputGain is a DEVICE pointer (it derives from the magnitude_ema buffer,
 * :344) read according to inputGainMode: 0 none, 1 one scalar, 2 [I], 3 [N,I].
 * `wsq` is scratch [O,I] float32 (per-(o,i) sum over taps of wn^2).
 * ---------------------------------------------------------------------- */
typedef struct sg3_modconv_prep_params {
    const float*   w;          /* [O,I,k,k] */
    const float*   s;          /* [N,I] */
    float*         wPacked;    /* sg3_modconv_packed_floats(O,I,k) floats */
    float*         wsq;        /* [O,I] scratch */
    float*         sIn;        /* [N,I] */
    float*         dcoef;      /* [N,O] (NULL allowed when demodulate == 0) */
    const float*   inputGain;  /* device pointer or NULL */
    int32_t        inputGainMode;
    int32_t        N, I, O, k;
    int32_t        demodulate;
    int32_t        precision;  /* SG3_CONV_FP32 | SG3_CONV_F16X3 | SG3_CONV_F16 */
    float          xBound;     /* f16x3 only: max |x| the conv will see (> 0).  sIn is scaled by a power of two per
                                * sample so that |x * sIn| stays below 2^15, and dcoef (required, also without
                                * demodulation) carries the inverse */
    const float*   xBoundDev;  /* optional DEVICE pointer to that bound (overrides xBound when not NULL): lets a caller
                                * derive it on the device, e.g. max |dy| of a gradient, without a host round trip */
    int32_t        reuseWeights; /* 1: wPacked and wsq already hold the result of an earlier call with the same w, k, precision
                                  * and demodulate (inference with unchanged weights): only the style pass (sIn, dcoef) runs */
} sg3_modconv_prep_params;

SG3_API int sg3_modulated_conv2d_prep(const sg3_modconv_prep_params* p, void* stream);

/* The same for `count` independent (w, s) pairs -- the layers of one Generator.synthesis call, whose styles are all known
 * before the first convolution (networks_stylegan3.py:478-485 computes them layer by layer) -- in two launches instead of
 * 2 * count.  No reference counterpart: the reference folds this arithmetic into torch ops inside modulated_conv2d (:39-56). */
SG3_API int sg3_modulated_conv2d_prep_batch(const sg3_modconv_prep_params* list, int count, void* stream);

typedef struct sg3_modconv_params {
    const void*    x;          /* [N,I,H,W] */
    const float*   wPacked;    /* from sg3_modulated_conv2d_prep */
    const float*   sIn;        /* [N,I] */
    const float*   dcoef;      /* [N,O] or NULL (no demodulation) */
    void*          out;        /* [N,O,outH,outW] */
    int32_t        dtype;      /* SG3_F32 | SG3_F16 (x and out) */
    int32_t        N, I, O, H, W;
    int32_t        k;          /* 1 or 3 */
    int32_t        pad;
    int32_t        precision;  /* must match the prep call that produced wPacked */
    /* Optional epilogue of the ToRGB form only (k = 1, pad = 0, O <= 4, SG3_CONV_FP32): the bias + clamp that
     * SynthesisLayer.forward applies next through filtered_lrelu with up = down = 1, gain = 1, slope = 1
     * (networks_stylegan3.py:352-356), optionally followed by a scale such as SynthesisNetwork's output scale (:488-489):
     * out = clamp(conv + bias[o], +-epilogueClamp) * epilogueScale -- the same values without further passes over the
     * image.  epilogueBias NULL = no epilogue; epilogueClamp < 0 = no clamp; epilogueScale 0 = 1. */
    const float*   epilogueBias;
    float          epilogueClamp;
    float          epilogueScale;
    /* Row pitch of `out` in elements; 0 = dense (outW).  The caller may allocate [N,O,outH,pitch] with pitch a multiple of 128
     * bytes and hand the [..., :outW] view on: a 1046-float row is 4184 bytes, so every 128-byte store segment of a dense output
     * straddles two cache lines (3x3 split-precision / fp16 kernels only; other forms require 0 or outW). */
    int32_t        outRowStride;
    /* Optional scratch for small grids (batch 1 on the 36^2 .. 84^2 maps: fewer tiles than CUs): the flat 3x3 direct kernel and the 1x1
     * GEMM kernel (fp32 tensors) then split the input channels of a tile over up to four workgroups and a second launch adds their
     * partial sums in order.  A call splits only when ALL of this holds (sg3_modconv_dispatch reports the outcome as kSplits):
     *   3x3: dcoef present, outW <= 128, ceil(I/16) >= 8 and N * ceil(O/64) * ceil(outH*outW/128) (the workgroups of the smallest
     *        flat tile) below the CU count;
     *   1x1: fp32 tensors, pad 0, O > 4, ceil(I/32) >= 8 and 4 * N * ceil(O/256) * ceil(H*W/256) below the CU count;
     *   (SG3_FLAT_SPLITS >= 2 in the environment stands in for the channel and workgroup counts, A/B timing)
     * and the chosen kernel's own grid leaves CUs idle, and the scratch holds kSplits partial images.  NULL / too small = no split
     * (same result up to fp32 summation order).  sg3_modconv_split_scratch_floats gives the exact size. */
    float*         splitScratch;
    int64_t        splitScratchFloats;
} sg3_modconv_params;

SG3_API int sg3_modulated_conv2d(const sg3_modconv_params* p, void* stream);

/* floats of splitScratch with which this call splits its K loop: kSplits * N * O * outH * outW of the plan made as if scratch were
 * unlimited (0 = the call would not split) */
SG3_API int64_t sg3_modconv_split_scratch_floats(const sg3_modconv_params* p);

/* kernel families of sg3_modulated_conv2d */
enum {
    SG3_MODCONV_NONE      = -1, /* no launch: the grid would pass 2^31 - 1 workgroups */
    SG3_MODCONV_FP32_MFMA = 0,  /* modconv_mfma_kernel<T, k, WM, WN, TM, TN>: exact fp32 products */
    SG3_MODCONV_TORGB     = 1,  /* modconv_1x1_small_kernel: 1x1, O <= 4 */
    SG3_MODCONV_ROWS      = 2,  /* modconv_f16x3_kernel<T, WM, WN, TN, SPLIT, PACK>: 3x3, 32 WM channels x (WN TN rows x 32 columns) */
    SG3_MODCONV_FLAT      = 3,  /* modconv_flat_kernel<T, TN, SPLIT>: 3x3 on narrow planes, 64 channels x runs of 64 TN pixels */
    SG3_MODCONV_GEMM1     = 4,  /* modconv1_f16x3_kernel<T, WM, WN, TM, TN, SPLIT, NBUF, M16>: 1x1, 32 WM TM channels x 256 pixels */
    SG3_MODCONV_F23       = 5,  /* modconv_f23_kernel<TN, T>: 3x3 in the transform domain, TN rows per wave */
};

/* What sg3_modulated_conv2d launches for a call: kernel family, template coordinates (0 where the family has none), launch geometry. */
typedef struct sg3_modconv_dispatch_info {
    int32_t        family;     /* SG3_MODCONV_* */
    int32_t        WM, WN, TM, TN;
    int32_t        SPLIT;      /* fp16 hi/lo operands (three MFMAs per product) */
    int32_t        PACK;       /* ROWS: tap-packed last K chunk */
    int32_t        NBUF;       /* GEMM1: LDS images (1 = two workgroups per CU) */
    int32_t        M16;        /* GEMM1: the 16x16x32 MFMA form */
    int32_t        nch;        /* K chunks (GEMM1: stages of 32 channels) */
    int32_t        xTiles, yTiles, mTiles;
    int32_t        kSplits;    /* workgroups sharing a tile's input channels; > 1: a reduce launch follows */
    int32_t        totalBlocks; /* tiles x kSplits the grid walks (F23: persistent workgroups, gridX = min(totalBlocks, CUs)) */
    int32_t        gridX, gridY, block;
    int32_t        ldsBytes;   /* dynamic LDS of the launch */
    int32_t        outPitch;   /* elements between output rows */
    int32_t        reduceGrid; /* workgroups (of 256) of modconv_split_reduce_kernel, 0 without a split */
} sg3_modconv_dispatch_info;

/* The plan of a call, from the function the launch itself uses (host only: no launch, no pointer followed -- only whether dcoef,
 * epilogueBias and splitScratch are set is read, so placeholders do; x, wPacked, sIn and out may be NULL).  `cus` <= 0: the CU count
 * of the current device, 256 without one.  SG3_BAD_ARG for a call sg3_modulated_conv2d rejects. */
SG3_API int sg3_modconv_dispatch(const sg3_modconv_params* p, int cus, sg3_modconv_dispatch_info* out);

/* ------------------------------------------------------------------------
 * conv2d_wgrad -- per-sample weight gradient of the (modulated) convolution, the part of the backward of
 *   models/stylegan3/networks_stylegan3.py:59-62 (grouped F.conv2d) that PTI needs
 *   (inversion/scripts/run_pti_images.py:130-139):
 *
 *   dW[n,o,i,ky,kx] = sum_{y,x} dy[n,o,y,x] * x[n,i,y+ky-pad,x+kx-pad]
 *
 * The pixel (K) dimension is split over nBands x nSegGroups workgroup sets (sg3_conv2d_wgrad_splits proposes the
 * counts); each writes its partial sum to partial[band*nSegGroups+group][n][tap][o][i] and the caller adds them up
 * (deterministic; no float atomics).  Operands are multiplied by *scaleX / *scaleDy (device scalars, powers of two chosen
 * by the caller so that the scaled magnitudes peak near 2^15: fp16 hi/lo split inside) and the result by 1/(scaleX*scaleDy).
 * ---------------------------------------------------------------------- */
typedef struct sg3_wgrad_params {
    const void*    x;          /* [N,I,H,W] */
    const void*    dy;         /* [N,O,OH,OW], OH = H + 2*pad - k + 1 */
    float*         partial;    /* [nBands*nSegGroups, N, k*k, O, I] */
    const float*   scaleX;     /* device scalar */
    const float*   scaleDy;    /* device scalar */
    int32_t        dtype;      /* SG3_F32 | SG3_F16 (x and dy) */
    int32_t        N, I, O, H, W;
    int32_t        k;          /* 1 or 3 */
    int32_t        pad;
    int32_t        nBands, nSegGroups;
    int32_t        scalesAreAmax; /* 1: *scaleX / *scaleDy hold max |x| / max |dy| and the kernel derives the power-of-two scales
                                   * itself (2^-ceil(log2(amax / 2^15))): saves the caller eight tiny launches per layer */
} sg3_wgrad_params;

SG3_API int sg3_conv2d_wgrad_splits(int N, int I, int O, int H, int W, int k, int pad, int* nBands, int* nSegGroups);
SG3_API int sg3_conv2d_wgrad(const sg3_wgrad_params* p, void* stream);

/* ------------------------------------------------------------------------
 * conv2d -- the plain convolutions of the ReStyle encoder (IR-SE50 backbone and
 *   GradualStyleBlock heads): replaces the torch.nn.Conv2d / BatchNorm2d / PReLU /
 *   LeakyReLU module calls of models/setgan/encoder/encoders/helpers.py:98-120,
 *   restyle_psp_encoders.py:26-28 and map2style.py:15-19 for eval-mode inference.
 *
 *   out[n,o,y,x] = act( bias[o] + sum_{i,ky,kx} w[o,i,ky,kx] *
 *                       pre(x[n,i, y*stride+ky-pad, x*stride+kx-pad]) )
 *   pre(v) = v * inScale[i] + inShift[i] inside the image, 0 in the padding
 *            (an eval-mode BatchNorm in FRONT of the convolution, helpers.py:108);
 *   a BatchNorm BEHIND the convolution is folded into w / bias by the caller.
 *   act: 0 none, 1 PReLU with per-channel slope[o], 2 leaky ReLU with slope[0].
 * NCHW contiguous fp32 tensors, k in {1,3}, stride in {1,2}, pad 0 .. k/2 + 1.
 * SG3_CONV_FP32: exact fp32 matrix-core arithmetic (v_mfma_f32_32x32x2_f32).
 * SG3_CONV_F16X3: operands split into fp16 hi + lo.  Activations keep relative
 *   2^-21 plus up to ~2^-23 absolute (below |x| = 2^-3 the halves leave fp16's
 *   normal range; they are not rescaled).  Weights are lifted per output channel
 *   by a power of two at packing (wScale holds the inverse, applied exactly in the
 *   epilogue) and keep relative 2^-22 within 2^-17 of their channel's maximum.
 * wPacked comes from sg3_conv2d_pack (layout [O][ceil(I/KC)][k*k][KC]).
 * ---------------------------------------------------------------------- */
typedef struct sg3_conv2d_params {
    const float*   x;          /* [N,I,H,W] */
    const float*   wPacked;    /* sg3_modconv_packed_floats(O,I,k,precision) floats, written by sg3_conv2d_pack */
    const float*   inScale;    /* [I] or NULL */
    const float*   inShift;    /* [I] or NULL (NULL = 0) */
    const float*   bias;       /* [O] or NULL */
    const float*   slope;      /* act 1: [O]; act 2: [1]; else ignored */
    float*         out;        /* [N,O,outH,outW] */
    int32_t        N, I, O, H, W;
    int32_t        k, stride, pad;
    int32_t        act;
    int32_t        precision;  /* SG3_CONV_FP32 (exact) | SG3_CONV_F16X3 (1x1 / 3x3, stride 1 or 2: fp16 x 3 split, precision above) */
    int32_t*       rangeFlag;  /* f16x3: device int, OR-ed with 1 when an operand left the fp16 range (the result of that
                                * call is then invalid and the caller repeats it with SG3_CONV_FP32); never cleared here */
    const float*   wScale;     /* f16x3: [O], written by sg3_conv2d_pack with wPacked; ignored for SG3_CONV_FP32 */
} sg3_conv2d_params;

SG3_API int sg3_conv2d(const sg3_conv2d_params* p, void* stream);

/* Diagnostic: the kernel form sg3_conv2d launches for *p (same checks, nothing launched; negative status for invalid params): the
 * `form` field of sg3_conv2d_dispatch (below, with tile, grid and LDS of the launch) for the current device.
 *   SG3_CONV_FP32_CHAINS:  12 (64 ch x 2 rows) or 13 (32 ch x 4 rows)
 *   SG3_CONV_FP32:  ((k == 3) * 2 + (stride == 2)) * 3 + tile, tile 0 = 128 ch x 4 rows, 1 = 64 ch x 2 rows, 2 = 32 ch x 4 rows
 *                   (12 forms);
 *   SG3_CONV_F16X3: SG3_CONV2D_FORM_F16X3 + 0 (1x1 stride 2), 1 (1x1 stride 1), 2 (3x3 stride 2), 3 (3x3 stride 1, outH <= 16,
 *                   4-row tile), 4 (3x3 stride 1, 4-row tile: fewer 8-row tiles than two per CU), 5 (3x3 stride 1, 8-row tile). */
#define SG3_CONV2D_FORM_F16X3 16
SG3_API int sg3_conv2d_form(const sg3_conv2d_params* p);

/* w [O,I,k,k] (* outScale[o] when given: a folded BatchNorm) -> packed layout; SG3_CONV_F16X3 also writes wScale [O] */
SG3_API int sg3_conv2d_pack(const float* w, const float* outScale, float* wPacked, float* wScale, int O, int I, int k, int precision, void* stream);

/* ------------------------------------------------------------------------
 * modulation_backward -- dL/dw and dL/ds of modulated_conv2d's per-sample effective weights, given G = dL/dw_eff
 *   (the output of sg3_conv2d_wgrad).  The reference gets them from autograd through its weight algebra
 *   (models/stylegan3/networks_stylegan3.py:39-56: pre-normalisation of w and s, modulation, demodulation, input gain);
 *   this is the same chain in closed form, four launches instead of ~70 (see csrc/sg3_modgrad.hip).  float32, dense tensors.
 *   G is overwritten (it holds dL/dm afterwards).  The input gain is a constant here (a buffer in the reference).
 * ---------------------------------------------------------------------- */
typedef struct sg3_modgrad_params {
    float*         G;          /* [N,O,I,T] dL/dw_eff; scratch on return */
    const float*   w;          /* [O,I,T] raw weights */
    const float*   s;          /* [N,I] raw styles */
    const float*   inputGain;  /* as in sg3_modconv_prep_params, or NULL */
    int32_t        inputGainMode;
    float*         dW;         /* [O,I,T] */
    float*         dS;         /* [N,I] */
    float*         a;          /* [O] scratch */
    float*         dSn;        /* [N,I] scratch */
    int32_t        N, O, I, T; /* T = k * k taps */
    int32_t        demodulate;
} sg3_modgrad_params;

SG3_API int sg3_modulation_backward(const sg3_modgrad_params* p, void* stream);

/* The weights of the DATA-GRADIENT convolution of modulated_conv2d in one launch: the reference's backward runs the grouped
 * convolution's adjoint (autograd of networks_stylegan3.py:59-62), i.e. a convolution with the pre-normalised (:41-42, when
 * `normalise`), transposed and flipped weights:  wt[i][o][k-1-ky][k-1-kx] = w[o][i][ky][kx] * rsqrt(mean_{i,ky,kx} w[o]^2).
 * w [O,I,k,k] and wt [I,O,k,k] dense fp32.  Replaces six elementwise / reduction launches per layer and PTI step. */
SG3_API int sg3_modconv_transpose_weights(const float* w, float* wt, int O, int I, int k, int normalise, void* stream);

/* ------------------------------------------------------------------------
 * se_residual -- the tail of an IR-SE residual unit (models/setgan/encoder/encoders/helpers.py:57-73 SEModule and
 *   :117-120 bottleneck_IR_SE.forward):  out = shortcut + res * sigmoid(fc2 @ relu(fc1 @ mean_hw(res))).
 *   Two launches (plane means; gates + apply) instead of the seven of the torch op chain.  float32, res / out dense NCHW;
 *   the shortcut is addressed through element strides (the stride-2 units read a subsampled view of their input).
 * ---------------------------------------------------------------------- */
typedef struct sg3_se_params {
    const float*   res;        /* [N,C,H,W] dense: the residual branch (after its last BatchNorm) */
    const float*   shortcut;   /* [N,C,H,W] through scStride */
    int64_t        scStride[4];/* elements, n,c,h,w */
    const float*   fc1;        /* [R,C] */
    const float*   fc2;        /* [C,R] */
    float*         mean;       /* [N,C] scratch (holds mean_hw(res) afterwards) */
    float*         out;        /* [N,C,H,W] dense; may alias res */
    int32_t        N, C, H, W, R;
} sg3_se_params;

SG3_API int sg3_se_residual(const sg3_se_params* p, void* stream);

/* ----------------------------------------------------------------------
 * unfold3x3s2 -- the patch matrix of a 3x3, stride-2, padding-1 convolution, for the batched GEMMs of the GradualStyleBlock heads
 *   (models/setgan/encoder/encoders/map2style.py:8-25: Conv2d(3x3, stride 2, padding 1) + LeakyReLU per level;
 *   restyle_psp_encoders.py:26-50).  One launch per level instead of the pad / slice / stack / permute chain:
 *       dst[g][(n*OH + oy)*OW + ox][tap*C + c] = act(src[g,n,c, 2*oy + ky - 1, 2*ox + kx - 1]),  0 outside the map,
 *   tap = ky*3 + kx, OH = (IH+1)/2, OW = (IW+1)/2, act = LeakyReLU(slope) of the previous level (slope 1 = none).
 *   src is addressed through element strides, so it may be the channels-first strip a convolution wrote or the
 *   [g][n*pixels][c] rows of the previous level's GEMM.  float32.
 * ---------------------------------------------------------------------- */
typedef struct sg3_unfold_params {
    const float*   src;
    int64_t        srcStride[5];   /* elements: g, n, c, y, x */
    float*         dst;            /* [G][N*OH*OW][9*C] dense */
    int32_t        G, N, C, IH, IW;
    float          slope;
} sg3_unfold_params;

SG3_API int sg3_unfold3x3s2(const sg3_unfold_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Batched small-M GEMMs of the GradualStyleBlock heads (reference models/setgan/encoder/encoders/map2style.py:8-25: the 3x3
 * stride-2 convolutions of levels 2.. as GEMMs over unfolded patches, and the closing EqualLinear, models/stylegan2/model.py
 * EqualLinear.forward; restyle_psp_encoders.py:26-50 runs n_styles heads):
 *     c[g][m][n] = sum_k lrelu(a[g][m][k], slope) * w[g][k][n] + bias[g][n]
 *   float32 in and out, split-precision fp16 x 3 arithmetic on the matrix cores, weight-bandwidth bound; operand precision as
 *   for sg3_conv2d's SG3_CONV_F16X3 (weights: relative 2^-21 within 2^-17 of their column's maximum).
 *   sg3_head_gemm_pack writes w ([G][K][N] float32, K % 16 == 0, N % 32 == 0) as matrix-instruction fragments into `packed`
 *   (sg3_head_gemm_packed_halfs(G,K,N) fp16 elements, -1 for unsupported shapes), every column lifted by a power of two, and the
 *   inverse powers into colScale ([G][N] float32); *rangeFlag is OR-ed with 1 when a weight (pack) or an activation (gemm) lies
 *   outside the fp16 range: the caller then uses its fp32 path.  bias may be NULL.
 * ---------------------------------------------------------------------- */
typedef struct sg3_head_gemm_params {
    const float*   a;              /* [G][M][K] dense */
    const void*    wPacked;        /* from sg3_head_gemm_pack */
    const float*   colScale;       /* [G][N], from sg3_head_gemm_pack with wPacked */
    const float*   bias;           /* [G][N] or NULL */
    float*         c;              /* [G][M][N] dense */
    int32_t*       rangeFlag;
    int32_t        G, M, K, N;
    float          slope;          /* LeakyReLU applied to a on the way in; 1 = none */
} sg3_head_gemm_params;

SG3_API long long sg3_head_gemm_packed_halfs(int32_t G, int32_t K, int32_t N);
SG3_API int sg3_head_gemm_pack(const float* w, void* packed, float* colScale, int32_t G, int32_t K, int32_t N, int32_t* rangeFlag, void* stream);
SG3_API int sg3_head_gemm(const sg3_head_gemm_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Image finishing of the editing scripts (reference utils/common.py:39-45 tensor2im, then PIL Image.resize((w, h)) with its
 * default BICUBIC filter as inversion/scripts/inference_editing.py:82-85 uses it): for every image b of x [B,3,H,W] float32
 *     y[b] = np.array(tensor2im(x[b]).resize((w, h)))        uint8 [h,w,3], bit-identical (NaN input is outside the contract)
 * One launch for all B images.  Strides are in elements (x: n, c, y, x; y: n, y, x, c -- bytes), any layout, so y may be a
 * column band of a wider strip.  A dimension whose size changes needs its table from sg3_resample_coeffs, copied to the device
 * by the caller (boundsH / coeffsH for W -> w, boundsV / coeffsV for H -> h); unused tables may be NULL.  When neither changes,
 * the images are converted without filtering, as PIL returns a copy.
 * sg3_resample_coeffs (host only): PIL's fixed-point bicubic taps for in -> out samples: bounds [out][2] = (first input sample,
 * tap count), coeffs [out][ksize] int32 (22 fractional bits, normalised in double precision); returns ksize, or the ksize alone
 * when both arrays are NULL; < 0 on a bad size.
 * ---------------------------------------------------------------------- */
typedef struct sg3_image_finish_params {
    const float*   x;              /* [B,3,H,W] */
    int64_t        xStride[4];
    uint8_t*       y;              /* [B,h,w,3] */
    int64_t        yStride[4];
    int32_t        B, H, W, h, w;
    const int32_t* boundsH;        /* [w][2] */
    const int32_t* coeffsH;        /* [w][kH] */
    int32_t        kH;
    const int32_t* boundsV;        /* [h][2] */
    const int32_t* coeffsV;        /* [h][kV] */
    int32_t        kV;
} sg3_image_finish_params;

SG3_API int sg3_resample_coeffs(int32_t inSize, int32_t outSize, int32_t* bounds, int32_t* coeffs);
SG3_API int sg3_image_finish(const sg3_image_finish_params* p, void* stream);

/* ----------------------------------------------------------------------
 * StyleCLIP latent mapper forward (reference editing/styleclip_mapper/latent_mappers.py: Mapper = PixelNorm over dim 1 -- the
 * levels of one sample -- then 4 x EqualLinear(512, 512, lr_mul=0.01, activation='fused_lrelu'); LevelsMapper runs one Mapper per
 * level group, a disabled group gives zeros; scripts/inference.py: w_hat = w + 0.1 * mapper(w)).  For every group g and every
 * sample n, on the levels l of [levelBegin[g], levelEnd[g]):
 *     h0 = x[n,l,:] * rsqrt(mean over the group's levels of x[n,l,:]^2 + 1e-8)
 *     h(i+1) = leaky_relu(h(i) @ weight[g][i]^T + bias[g][i], 0.2) * sqrt(2)        i = 0..3
 *     delta[n,l,:] = h4,   out[n,l,:] = x[n,l,:] + alpha * delta[n,l,:]
 *   and on levels in no group delta = 0, out = x + alpha * 0.  weight [groups][4][512][512] is the prepared (W * scale) in the
 *   stored [out][in] order, bias [groups][4][512] is b * lr_mul; float32 throughout, fp32 products and fp32 accumulation in a fixed
 *   order, so a sample's result does not depend on the batch it is in.  x, out, delta are dense [N][L][D]; out or delta may be
 *   NULL (not both).  scratch: 2 * N * L * D floats (may be NULL when groups == 0).  weight and scratch 16-byte aligned; the written
 *   buffers overlap no other.  D must be 512, L at most 32, groups 0..4, groups non-empty and disjoint.  Five launches (one when groups == 0).
 * ---------------------------------------------------------------------- */
typedef struct sg3_latent_mapper_params {
    const float*   x;              /* [N][L][D] */
    const float*   weight;         /* [groups][4][D][D] */
    const float*   bias;           /* [groups][4][D] */
    float*         out;            /* [N][L][D] or NULL */
    float*         delta;          /* [N][L][D] or NULL */
    float*         scratch;        /* 2 * N * L * D floats */
    int32_t        N, L, D;
    int32_t        groups;
    int32_t        levelBegin[4];
    int32_t        levelEnd[4];
    float          alpha;
} sg3_latent_mapper_params;

SG3_API int sg3_latent_mapper(const sg3_latent_mapper_params* p, void* stream);

/* ----------------------------------------------------------------------
 * StyleCLIP latent mapper for training: the forward above with every activation kept, and its backward.
 *
 * sg3_latent_mapper_train_forward: the same two kernels, in the same order, as sg3_latent_mapper (so delta and out are bitwise
 *   equal to its results), writing h0..h3 into the caller's acts [4][N][L][D] and h4 into delta (required here) instead of a
 *   ping-pong scratch.  acts rows of levels in no group are not written.  Five launches (one when groups == 0).
 *
 * sg3_latent_mapper_backward: given dDelta and / or dOut (either may be NULL, not both when groups > 0; dOut adds alpha * dOut
 *   to dDelta and passes straight through to dx), with dz_i = dh_i * (h_i > 0 ? sqrt(2) : 0.2 * sqrt(2)) taken from the saved h_i:
 *     dh_(i-1) = dz_i @ weight[g][i-1]                                     i = 4..1   (fp32 MFMA, fixed order, batch invariant)
 *     dW[g][i-1] = (dz_i^T @ h_(i-1)) * wScale[4g+i-1]                     gradient of the STORED weight  [D][D]
 *     dB[g][i-1] = (sum over rows of dz_i) * bScale[4g+i-1]                gradient of the STORED bias    [D]
 *     dx[n,l,:]  = r * dh0_l - x_l * r^3 * (1/Lg) * sum_j dh0_j * x_j  (+ dOut[n,l,:])   over the group's levels,
 *   and dx = dOut (zero when NULL) on levels in no group.  dx may be NULL (then the last data gradient and the PixelNorm backward
 *   are skipped); dW and dB are both given or both NULL (then no weight gradient is launched).  x, acts, delta are what the
 *   forward read and wrote.  scratch: 2 * N * L * D floats.  At most ten launches: dz_4, 4 x data gradient, 4 x weight gradient,
 *   PixelNorm; every result is a fixed sequence of operations (no atomics), so two runs are bitwise equal.
 *   weight, acts, delta, scratch, dDelta 16-byte aligned; every written buffer overlaps no other; D == 512, L <= 32.
 * ---------------------------------------------------------------------- */
typedef struct sg3_latent_mapper_train_params {
    const float*   x;              /* [N][L][D] */
    const float*   weight;         /* [groups][4][D][D] */
    const float*   bias;           /* [groups][4][D] */
    float*         out;            /* [N][L][D] or NULL */
    float*         delta;          /* [N][L][D]  (h4) */
    float*         acts;           /* [4][N][L][D]  (h0..h3) */
    int32_t        N, L, D;
    int32_t        groups;
    int32_t        levelBegin[4];
    int32_t        levelEnd[4];
    float          alpha;
} sg3_latent_mapper_train_params;

typedef struct sg3_latent_mapper_backward_params {
    const float*   x;              /* [N][L][D] */
    const float*   weight;         /* [groups][4][D][D]  prepared, as in the forward */
    const float*   acts;           /* [4][N][L][D] */
    const float*   delta;          /* [N][L][D] */
    const float*   dDelta;         /* [N][L][D] or NULL */
    const float*   dOut;           /* [N][L][D] or NULL */
    float*         dx;             /* [N][L][D] or NULL */
    float*         dW;             /* [groups][4][D][D] or NULL */
    float*         dB;             /* [groups][4][D] or NULL */
    float*         scratch;        /* 2 * N * L * D floats */
    int32_t        N, L, D;
    int32_t        groups;
    int32_t        levelBegin[4];
    int32_t        levelEnd[4];
    float          alpha;
    float          wScale[16];     /* [groups][4]  EqualLinear.scale */
    float          bScale[16];     /* [groups][4]  EqualLinear.lr_mul */
} sg3_latent_mapper_backward_params;

SG3_API int sg3_latent_mapper_train_forward(const sg3_latent_mapper_train_params* p, void* stream);
SG3_API int sg3_latent_mapper_backward(const sg3_latent_mapper_backward_params* p, void* stream);

/* ----------------------------------------------------------------------
 * One Ranger step (RAdam + lookahead + gradient centralisation, reference utils/ranger.py:79-165) of up to 32 dense float32
 * tensors in one launch; one workgroup per row, a 1-D tensor is one row.  Per element, each line rounded as the torch op it restates:
 *     g = grad - mean(row)                 when centralise (written back to grad; the row sum has a fixed order)
 *     expAvgSq = expAvgSq * beta2 + oneMinusBeta2 * g * g;      expAvg = expAvg * beta1 + oneMinusBeta1 * g
 *     p = p - decay * p                    when decay (= weight_decay * lr) != 0
 *     p = p - stepLr * expAvg / (sqrt(expAvgSq) + eps)   when adaptive, else   p = p - stepLr * expAvg      (stepLr = step_size * lr)
 *     slow = slow + alpha * (p - slow);  p = slow        when lookahead
 * step_size, adaptive and lookahead come from the host's step count.  No buffer of the call may overlap another.
 * ---------------------------------------------------------------------- */
typedef struct sg3_ranger_tensor {
    float*         p;
    float*         grad;
    float*         expAvg;
    float*         expAvgSq;
    float*         slow;
    int32_t        rows, cols;
    int32_t        centralise;
    int32_t        reserved;
} sg3_ranger_tensor;

typedef struct sg3_ranger_params {
    sg3_ranger_tensor t[32];
    int32_t        count;
    float          beta1, beta2, oneMinusBeta1, oneMinusBeta2, eps, decay, stepLr, alpha;
    int32_t        adaptive, lookahead;
} sg3_ranger_params;

SG3_API int sg3_ranger_step(const sg3_ranger_params* p, void* stream);

/* ----------------------------------------------------------------------
 * CLIP image preprocessing of the StyleCLIP delta_i_c sweep (reference
 * editing/styleclip_global_directions/preprocess/create_delta_i_c.py:53-56), for x [B,3,H,W] float32:
 *     y = F.interpolate(x, size=(h, w), mode='bicubic', align_corners=True)
 *     y = ((y + 1) / 2).clamp(0, 1)
 *     y = (y - mean[c]) / std[c]                              float32 [B,3,h,w]
 * in one launch for all B images, one thread per output pixel over the three channels.  Source coordinates are torch's:
 * scale = float(in - 1) / float(out - 1) (0 when out == 1), src = scale * dst in float32, floorf, t = src - floor; taps are the
 * cubic convolution with A = -0.75 at floor - 1 .. floor + 2, indices clamped to the border; rows are filtered along x first, then
 * the four row results along y.  When neither size changes the pixels are copied without filtering, as torch's device kernel does.
 * The tap polynomials and the four-term sums are explicit fused multiply-adds, as torch's device kernel contracts them; nothing
 * else is fused (the library is built without contraction for this entry); NaN propagates through the clamp as it does through
 * torch.clamp.  Strides are in elements (n, c, y, x), any layout; y must not overlap x.  C must be 3, std non-zero.
 * ---------------------------------------------------------------------- */
typedef struct sg3_clip_preprocess_params {
    const float*   x;              /* [B,C,H,W] */
    int64_t        xStride[4];
    float*         y;              /* [B,C,h,w] */
    int64_t        yStride[4];
    int32_t        B, C, H, W, h, w;
    float          mean[3];
    float          std[3];
} sg3_clip_preprocess_params;

SG3_API int sg3_clip_preprocess(const sg3_clip_preprocess_params* p, void* stream);

/* ----------------------------------------------------------------------
 * CLIP ViT encoders (reference models/styleganxl/feature_networks/clip/model.py:153-236, :324-352): the kernels one
 * ResidualAttentionBlock and the two stems are made of.  The residual stream is float32 [rows][D]; GEMM operands are float16 with
 * float32 accumulation in ascending k, one accumulator per output element (no split-K, no atomics), so every output row depends
 * on its own input row only.  One launch per call, on `stream`; every argument check is made on the host before the launch.
 *
 * sg3_clip_supported (host only): 1 when these kernels run a transformer of this width, head count and sequence length
 * (width == 64 * heads, 1 <= L <= 128), else 0.
 *
 * sg3_clip_layernorm: out[r][:] = (x[r][:] - mean) / sqrt(var + eps) * gamma + beta, biased variance, float32 statistics taken
 *   relative to the row's first element (no cancellation on a large mean).  Row r of x starts at x + r * xRowStride (elements);
 *   out is dense [rows][D] in outDtype (SG3_F16 or SG3_F32); out == x is allowed for SG3_F32 with xRowStride == D.
 *
 * sg3_clip_gemm: C[M][N] = A[M][K] . W[N][K]^T (+ bias[N], float32, may be NULL); A and W float16, K contiguous, 16-byte aligned;
 *   W is nn.Linear's [out][in].  N % 64 == 0 and K % 32 == 0, else SG3_BAD_ARG; M is arbitrary.  epilogue:
 *     SG3_CLIP_EPI_F32            out float32 [M][N] = acc + bias
 *     SG3_CLIP_EPI_F16            out float16 [M][N] = acc + bias
 *     SG3_CLIP_EPI_QUICKGELU_F16  out float16 [M][N] = v * sigmoid(1.702 v), v = acc + bias, in float32
 *     SG3_CLIP_EPI_RESIDUAL       out float32 [M][N] += acc + bias (in place on the residual stream)
 *     SG3_CLIP_EPI_PATCH          the patch embedding: a is the dense float32 image [B][3][R][R], 16-byte aligned, R % 4 == 0; w is
 *                                 conv1.weight [N][3*P*P] in float16, P % 8 == 0, K == 3*P*P; with g = R / P, M == B*g*g and row
 *                                 m is patch (m / g^2, (m % g^2) / g, m % g).  out float32 [B][g*g + 1][N]: token 1 + patch =
 *                                 acc + bias + pos[1 + patch], token 0 = cls + pos[0]  (pos [g*g + 1][N], cls [N], float32).
 *
 * sg3_clip_attention: qkv float16 [B][L][3*D] as the in_proj GEMM writes it (q | k | v, head h in columns 64 h .. 64 h + 63 of
 *   each), D = 64 * heads.  out float16 [B][L][D] = softmax(q k^T / 8 (+ causal mask)) v per (sample, head); float32 scores,
 *   max-subtracted float32 softmax, float32 P.V.  causal != 0: query i attends keys j <= i (the reference's -inf upper triangle).
 *
 * sg3_clip_embed: out float32 [B][L][D] = table[tokens[b][l]][:] + pos[l][:]; tokens int64, a token outside [0, vocab) is
 *   clamped into it.
 * ---------------------------------------------------------------------- */
#define SG3_CLIP_EPI_F32           0
#define SG3_CLIP_EPI_F16           1
#define SG3_CLIP_EPI_QUICKGELU_F16 2
#define SG3_CLIP_EPI_RESIDUAL      3
#define SG3_CLIP_EPI_PATCH         4

typedef struct sg3_clip_layernorm_params {
    const float*   x;              /* row r at x + r * xRowStride */
    const float*   gamma;          /* [D] */
    const float*   beta;           /* [D] */
    void*          out;            /* [rows][D], outDtype */
    int64_t        xRowStride;
    int32_t        rows, D;
    int32_t        outDtype;       /* SG3_F16 or SG3_F32 */
    float          eps;
} sg3_clip_layernorm_params;

typedef struct sg3_clip_gemm_params {
    const void*    a;              /* float16 [M][K]; SG3_CLIP_EPI_PATCH: float32 [B][3][R][R] */
    const void*    w;              /* float16 [N][K] */
    const float*   bias;           /* [N] or NULL */
    void*          out;
    const float*   pos;            /* SG3_CLIP_EPI_PATCH: [g*g + 1][N] */
    const float*   cls;            /* SG3_CLIP_EPI_PATCH: [N] */
    int32_t        M, K, N;
    int32_t        epilogue;
    int32_t        P, R;           /* SG3_CLIP_EPI_PATCH: patch size, image resolution */
} sg3_clip_gemm_params;

typedef struct sg3_clip_attention_params {
    const void*    qkv;            /* float16 [B][L][3*64*heads] */
    void*          out;            /* float16 [B][L][64*heads] */
    int32_t        B, L, heads;
    int32_t        causal;
} sg3_clip_attention_params;

typedef struct sg3_clip_embed_params {
    const int64_t* tokens;         /* [B][L] */
    const float*   table;          /* [vocab][D] */
    const float*   pos;            /* [L][D] */
    float*         out;            /* [B][L][D] */
    int32_t        B, L, D, vocab;
} sg3_clip_embed_params;

SG3_API int sg3_clip_supported(int width, int heads, int L);
SG3_API int sg3_clip_layernorm(const sg3_clip_layernorm_params* p, void* stream);
SG3_API int sg3_clip_gemm(const sg3_clip_gemm_params* p, void* stream);
SG3_API int sg3_clip_attention(const sg3_clip_attention_params* p, void* stream);
SG3_API int sg3_clip_embed(const sg3_clip_embed_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Backward of the CLIP image tower with respect to its input (weights frozen: there is no weight gradient).  One launch per call, no atomics, fixed summation order: a row's result depends on that row's inputs only.
 *
 * sg3_clip_gemm_grad: the GEMM of sg3_clip_gemm (same kernel, same sizes and alignment rules, same accumulation order) with the
 *   epilogues of the recording forward and of the data-gradient pass; dX = dY . W is this kernel on a float16 [in][out] copy of
 *   the matrix.  epilogue is SG3_CLIP_EPI_F32, SG3_CLIP_EPI_F16 (as sg3_clip_gemm), or:
 *     SG3_CLIP_EPI_RESIDUAL            out float32 [M][N] = aux[m][n] + acc + bias: the residual is read from aux (float32 [M][N],
 *                                      required), so the stream before the block stays as the backward needs it
 *     SG3_CLIP_EPI_QUICKGELU_SAVE_F16  as SG3_CLIP_EPI_QUICKGELU_F16, and aux float16 [M][N] = v (the pre-activation)
 *     SG3_CLIP_EPI_DQUICKGELU_F16      out float16 [M][N] = v * QuickGELU'(u), u = aux[m][n] (float16, read),
 *                                      QuickGELU'(u) = s (1 + 1.702 u (1 - s)), s = sigmoid(1.702 u), in float32
 *     SG3_CLIP_EPI_PATCH_ADJOINT       the adjoint of SG3_CLIP_EPI_PATCH with respect to the image: a is the token gradient
 *                                      [B][g*g + 1][K] (row m of the product is token 1 + m % g^2 of sample m / g^2), w is
 *                                      conv1.weight transposed, float16 [N = 3*P*P][K]; out float32 [B][3][R][R], element
 *                                      (b, c, py*P + ky, px*P + kx) = v * (scale ? scale[b] : 1) with n = (c*P + ky)*P + kx.
 *                                      Patches do not overlap: every pixel of the g*P x g*P area is written once, no other is.
 *   aF32 != 0: a is float32 [M][K] (16-byte aligned) and rounded to float16 as it is loaded; allowed for SG3_CLIP_EPI_F16,
 *   SG3_CLIP_EPI_DQUICKGELU_F16 and SG3_CLIP_EPI_PATCH_ADJOINT (the float32 gradient stream is the operand).
 *
 * sg3_clip_layernorm_bwd: for y = LayerNorm(x) * gamma + beta and dy [rows][D] (row r at dy + r * dyRowStride),
 *   dx = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy, with the statistics of x taken as the forward takes them (relative to
 *   the row's first element).  Row r of x at x + r * xRowStride, of dx at dx + r * dxRowStride.  accumulate != 0: dx += result
 *   (the float32 gradient stream), else dx = result; dx == dy is allowed (every element is read and written by one lane).
 *
 * sg3_clip_attention_bwd: qkv float16 [B][L][3*D] as saved by the forward, dout float16 [B][L][D]; dqkv float16 [B][L][3*D].
 *   The probabilities are recomputed per (sample, head) in LDS; scores, softmax and its backward
 *   dS = P (dP - sum_j P dP) are float32.  L <= 128, head dimension 64.  causal != 0 is refused with SG3_BAD_ARG.
 *
 * sg3_clip_grad_scale: per row b of g float32 [B][E]: scale[b] = 2^(4 - e) with max|g[b]| = m 2^e, 0.5 <= m < 1 (1 for a zero or
 *   non-finite row), so that max|g[b]| scale[b] is in [8, 16); out16 float16 [B][E] = g scale[b]; inv[b] = 1 / scale[b] (exact).
 *   The gradients of a float16 backward are below float16's normal range at their natural size; the power of two is carried
 *   through the (linear) backward and divided out at the image.  Taken on the device: no host synchronisation.
 * ---------------------------------------------------------------------- */
#define SG3_CLIP_EPI_QUICKGELU_SAVE_F16 5
#define SG3_CLIP_EPI_DQUICKGELU_F16     6
#define SG3_CLIP_EPI_PATCH_ADJOINT      7

typedef struct sg3_clip_gemm_grad_params {
    const void*    a;              /* float16 [M][K], or float32 when aF32; SG3_CLIP_EPI_PATCH_ADJOINT: [B][g*g + 1][K] */
    const void*    w;              /* float16 [N][K] */
    const float*   bias;           /* [N] or NULL */
    void*          out;
    void*          aux;            /* see the epilogues; NULL for the others */
    const float*   scale;          /* SG3_CLIP_EPI_PATCH_ADJOINT: [B] or NULL */
    int32_t        M, K, N;
    int32_t        epilogue;
    int32_t        P, R;           /* SG3_CLIP_EPI_PATCH_ADJOINT: patch size, image resolution */
    int32_t        aF32;
} sg3_clip_gemm_grad_params;

typedef struct sg3_clip_layernorm_bwd_params {
    const float*   dy;
    const float*   x;
    const float*   gamma;          /* [D] */
    float*         dx;
    int64_t        dyRowStride, xRowStride, dxRowStride;
    int32_t        rows, D;
    int32_t        accumulate;
    float          eps;
} sg3_clip_layernorm_bwd_params;

typedef struct sg3_clip_attention_bwd_params {
    const void*    qkv;            /* float16 [B][L][3*64*heads] */
    const void*    dout;           /* float16 [B][L][64*heads] */
    void*          dqkv;           /* float16 [B][L][3*64*heads] */
    int32_t        B, L, heads;
    int32_t        causal;
} sg3_clip_attention_bwd_params;

typedef struct sg3_clip_grad_scale_params {
    const float*   g;              /* [B][E] */
    void*          out16;          /* float16 [B][E] */
    float*         inv;            /* [B] */
    int32_t        B, E;
} sg3_clip_grad_scale_params;

SG3_API int sg3_clip_gemm_grad(const sg3_clip_gemm_grad_params* p, void* stream);
SG3_API int sg3_clip_layernorm_bwd(const sg3_clip_layernorm_bwd_params* p, void* stream);
SG3_API int sg3_clip_attention_bwd(const sg3_clip_attention_bwd_params* p, void* stream);
SG3_API int sg3_clip_grad_scale(const sg3_clip_grad_scale_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Image preparation of the CLIP loss (reference criteria/clip_loss.py: AvgPool2d(k)(Upsample(scale_factor=up)(x)), nearest):
 *     y[oy][ox] = (1 / k^2) sum_{u in [oy k, oy k + k)} sum_{v in [ox k, ox k + k)} x[u / up][v / up],   oh = (up H) / k, ow = (up W) / k
 * as one launch with no intermediate: per axis the window covers at most ceil(k / up) + 1 source pixels, each with an integer
 * count of upsampled pixels inside the window.  adjoint != 0 runs the transpose in gather form: x is then the OUTPUT [B][C][H][W]
 * (the gradient of the source) and y the INPUT [B][C][oh][ow]; every source pixel sums the windows that overlap it (no atomics).
 * float32, strides in elements (n, c, y, x), any layout; the written tensor must not overlap the read one.
 * ---------------------------------------------------------------------- */
typedef struct sg3_clip_resample_params {
    float*         x;              /* [B][C][H][W]: read (forward) or written (adjoint) */
    int64_t        xStride[4];
    float*         y;              /* [B][C][oh][ow]: written (forward) or read (adjoint) */
    int64_t        yStride[4];
    int32_t        B, C, H, W, oh, ow;
    int32_t        up, k;
    int32_t        adjoint;
} sg3_clip_resample_params;

SG3_API int sg3_clip_resample(const sg3_clip_resample_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Image preparation of the identity loss (reference criteria/id_loss.py extract_feats): AdaptiveAvgPool2d(256) when H != 256,
 * crop [35:223, 32:220], AdaptiveAvgPool2d(112) -- one separable banded linear map per plane, out = Ay X Ax^T, as one launch that
 * reads the source once and writes no intermediate.  adjoint != 0 runs the transpose in gather form: x is then the OUTPUT
 * [B][C][H][W] (exact zeros outside the crop's footprint, no atomics) and y the INPUT [B][C][112][112].
 * float32, strides in elements (n, c, y, x), any layout; the written tensor must not overlap the read one.
 * `pool` must be 1 exactly when H != 256 (the reference's rule; the columns follow the rows); an unpooled image needs W >= 220.
 * ---------------------------------------------------------------------- */
typedef struct sg3_face_pool_params {
    float*         x;              /* [B][C][H][W]: read (forward) or written (adjoint) */
    int64_t        xStride[4];
    float*         y;              /* [B][C][112][112]: written (forward) or read (adjoint) */
    int64_t        yStride[4];
    int32_t        B, C, H, W;
    int32_t        pool;
    int32_t        adjoint;
} sg3_face_pool_params;

SG3_API int sg3_face_pool(const sg3_face_pool_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Data gradient of sg3_conv2d's convolutions (k in {1, 3}, stride in {1, 2}, padding k / 2) on the fp32 matrix cores:
 *     dx[n][i][y][x] = sum_{o,ky,kx} w[o][i][ky][kx] dy[n][o][(y + pad - ky) / stride][(x + pad - kx) / stride]   (taps that divide)
 * Stride 2 runs as four dense sub-convolutions, one per pixel parity, over the 1, 2, 2 and 4 taps that reach it.
 * wPacked: sg3_conv2d_pack(wT, outScale, ..., O = I, I = O, k, SG3_CONV_FP32) of the TRANSPOSED weight wT[i][o][ky][kx] (not
 * flipped); its outScale is then a per-input-channel scale of dx (a BatchNorm in front of the forward convolution).
 * H x W is the size of dx (a stride-2 output size does not determine it); OH x OW that of dy and must be the forward's output size.
 * Epilogue per element, in this order:  v = acc;  v += addend[n sN + i sC + y sH + x sW] (addend != NULL);
 * v *= (act[n][i][y][x] > 0 ? 1 : slope[i]) (act != NULL: the PReLU whose output -- or pre-activation, when a slope is negative --
 * was saved as act, contiguous like dx).  dy and dx are contiguous float32 and must not overlap.
 * ---------------------------------------------------------------------- */
typedef struct sg3_conv2d_dgrad_params {
    const float*   dy;             /* [N][O][OH][OW] */
    const float*   wPacked;
    float*         dx;             /* [N][I][H][W] */
    const float*   act;            /* [N][I][H][W] or NULL */
    const float*   slope;          /* [I], required with act */
    const float*   addend;         /* or NULL */
    int64_t        addStride[4];
    int32_t        N, I, O, H, W, OH, OW;
    int32_t        k, stride;
} sg3_conv2d_dgrad_params;

SG3_API int sg3_conv2d_dgrad(const sg3_conv2d_dgrad_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Backward of sg3_se_residual (out = shortcut + res * sigmoid(fc2 relu(fc1 mean_hw(res)))), two launches:
 *     dg = sum_hw dout res;  dz = dg g (1 - g);  dh = fc2^T dz;  du = dh [u > 0];  dm = fc1^T du;  dres = dout g + dm / (H W)
 * `res` is the forward's res input and `mean` what the forward left in its `mean`.  The shortcut's gradient is dout itself and is
 * not written; with dscatter != NULL (identity shortcut of a stride-2 unit) dscatter [N][C][inH][inW] receives dout at the even
 * positions and zero elsewhere, H = ceil(inH / 2), W = ceil(inW / 2).  All tensors contiguous float32; dg [N][C] is scratch.
 * ---------------------------------------------------------------------- */
typedef struct sg3_se_bwd_params {
    const float*   dout;           /* [N][C][H][W] */
    const float*   res;            /* [N][C][H][W] */
    const float*   mean;           /* [N][C] */
    const float*   fc1;            /* [R][C] */
    const float*   fc2;            /* [C][R] */
    float*         dg;             /* [N][C] scratch */
    float*         dres;           /* [N][C][H][W] */
    float*         dscatter;       /* [N][C][inH][inW] or NULL */
    int32_t        N, C, H, W, R;
    int32_t        inH, inW;
} sg3_se_bwd_params;

SG3_API int sg3_se_residual_bwd(const sg3_se_bwd_params* p, void* stream);

/* ----------------------------------------------------------------------
 * LPIPS (AlexNet) criterion (reference criteria/lpips): the pieces besides sg3_conv2d / sg3_conv2d_dgrad.  All float32, exact fp32
 * arithmetic, no float atomics: every result is bit-identical on repeat.  Tensors are contiguous unless strides are given.
 *
 * sg3_lpips_prepare: x [N][3][H][W] (element strides) -> canvas [N][48][OH+2][OW+2], OH = (H - 7) / 4 + 1 (OW likewise):
 *     canvas[n][c*16 + ry*4 + rx][py][px] = (x[n][c][4 py + ry - 2][4 px + rx - 2] - mean[c]) / std[c]   inside the image, else 0
 * Over it the 11x11 stride-4 pad-2 convolution is a VALID 3x3 stride-1 convolution of 48 channels whose weight is the 11x11 one
 * zero-extended to 12x12 and regrouped [O][3][3][4][3][4] -> [O][48][3][3].
 * sg3_lpips_prepare_bwd: the adjoint; x is then the OUTPUT (dx = dcanvas / std, times scale[0] when scale != NULL; exactly 0 for
 * image rows / columns beyond the canvas, which the convolution never reads) and canvas the INPUT.
 * ---------------------------------------------------------------------- */
typedef struct sg3_lpips_prepare_params {
    float*         x;              /* [N][3][H][W]: read (forward) or written (adjoint) */
    int64_t        xStride[4];
    float*         canvas;         /* [N][48][OH+2][OW+2]: written (forward) or read (adjoint) */
    const float*   scale;          /* adjoint only: device scalar multiplied into dx, or NULL */
    int32_t        N, H, W;
    float          mean[3];
    float          std[3];
} sg3_lpips_prepare_params;

SG3_API int sg3_lpips_prepare(const sg3_lpips_prepare_params* p, void* stream);
SG3_API int sg3_lpips_prepare_bwd(const sg3_lpips_prepare_params* p, void* stream);

/* 5x5 stride-1 pad-2 convolution on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): out = conv(x, w) (+ bias) (ReLU when relu != 0).
 * wPacked: sg3_conv2d_k5_pack of w [O][I][5][5] into [O][ceil(I/8)][25][8] (sg3_conv2d_k5_packed_floats floats).  The data gradient
 * of such a convolution is the same call on the transposed, spatially flipped weight wT[i][o][4-ky][4-kx]. */
typedef struct sg3_conv2d_k5_params {
    const float*   x;              /* [N][I][H][W] */
    const float*   wPacked;
    const float*   bias;           /* [O] or NULL */
    float*         out;            /* [N][O][H][W] */
    int32_t        N, I, O, H, W;
    int32_t        relu;
} sg3_conv2d_k5_params;

SG3_API int64_t sg3_conv2d_k5_packed_floats(int O, int I);
SG3_API int sg3_conv2d_k5_pack(const float* w, float* wPacked, int O, int I, void* stream);
SG3_API int sg3_conv2d_k5(const sg3_conv2d_k5_params* p, void* stream);

/* MaxPool2d(kernel 3, stride 2, no padding, floor): y [N][C][(H-3)/2+1][(W-3)/2+1], values bit-equal to the library's. */
typedef struct sg3_maxpool3s2_params {
    const float*   x;              /* [N][C][H][W] */
    float*         y;
    int32_t        N, C, H, W;
} sg3_maxpool3s2_params;

SG3_API int sg3_maxpool3s2(const sg3_maxpool3s2_params* p, void* stream);

/* Its backward in gather form: dx[pixel] = sum of dy over the (<= 4) windows whose first maximum in row-major order is that pixel,
 * + addend[pixel] (addend != NULL, contiguous like x), then times (x > 0) when reluMask != 0.  Pixels no window covers receive
 * only the addend.  dx is written through element strides (it may be the interior of a larger zeroed buffer). */
typedef struct sg3_maxpool3s2_bwd_params {
    const float*   x;              /* [N][C][H][W]: the forward's input */
    const float*   dy;             /* [N][C][OH][OW] */
    const float*   addend;         /* [N][C][H][W] or NULL */
    float*         dx;             /* [N][C][H][W] through dxStride */
    int64_t        dxStride[4];
    int32_t        N, C, H, W;
    int32_t        reluMask;
} sg3_maxpool3s2_bwd_params;

SG3_API int sg3_maxpool3s2_bwd(const sg3_maxpool3s2_bwd_params* p, void* stream);

/* One LPIPS layer:  value[n] = sum_hw sum_c lin[c] (a_c - b_c)^2 / (h w),  a = fx / (|fx| + 1e-10), b = fy / (|fy| + 1e-10), the
 * norms over channels per pixel.  dfx != NULL also receives d value[n] / d fx[n] in closed form:
 *     g_c = 2 lin[c] (a_c - b_c) / (h w),   dfx_c = g_c / (r + eps) - fx_c (sum_j g_j fx_j) / (r (r + eps)^2),   r = |fx|
 * and exactly 0 for every channel of a pixel with r = 0; with reluMask != 0 it is 0 wherever fx <= 0 as well.
 * partial: scratch of N * sg3_lpips_head_blocks(h, w) floats.  counter: N int32 that are ZERO on entry and are left zero. */
typedef struct sg3_lpips_head_params {
    const float*   fx;             /* [N][C][h][w] */
    const float*   fy;             /* [N][C][h][w] */
    const float*   lin;            /* [C] */
    float*         value;          /* [N] */
    float*         dfx;            /* [N][C][h][w] or NULL */
    float*         partial;
    int32_t*       counter;
    int32_t        N, C, h, w;
    int32_t        reluMask;
} sg3_lpips_head_params;

SG3_API int sg3_lpips_head_blocks(int h, int w);
SG3_API int sg3_lpips_head(const sg3_lpips_head_params* p, void* stream);

/* ----------------------------------------------------------------------
 * Training the encoder trunk: weight gradient of sg3_conv2d's convolutions summed over the batch, exact fp32 matrix products:
 *     dw[o][i][ky][kx] = sum_{n,oy,ox} dy[n][o][oy][ox] xt[n][i][oy stride + ky - k / 2][ox stride + kx - k / 2]
 *     xt = inScale[i] x + inShift[i] on real pixels (both NULL: xt = x), 0 in the padding; k in {1, 3}, stride in {1, 2}.
 * The K dimension is cut into chunks: chunk c = (n OH + oy) xSegs + xs is the output pixels [P xs, min(OW, P xs + P)) of row oy of
 * sample n, P = 32 / stride.  Split j of nSplit sums the chunks [j chunksPerSplit, min((j + 1) chunksPerSplit, N OH xSegs)) into its own partial, and a
 * second launch adds the partials in split order (one split: written to dw directly).  sg3_conv2d_wgrad_sum_splits is host only and does
 * not depend on the device.  partial: nSplit O I k k floats of scratch (may be NULL for one split).  All tensors contiguous float32.
 * ---------------------------------------------------------------------- */
typedef struct sg3_conv2d_wgrad_sum_params {
    const float*   x;              /* [N][I][H][W] */
    const float*   dy;             /* [N][O][OH][OW] */
    const float*   inScale;        /* [I] or NULL */
    const float*   inShift;        /* [I] or NULL */
    float*         dw;             /* [O][I][k][k] */
    float*         partial;
    int32_t        N, I, O, H, W;
    int32_t        k, stride;
} sg3_conv2d_wgrad_sum_params;

SG3_API int sg3_conv2d_wgrad_sum_splits(int N, int I, int O, int H, int W, int k, int stride, int* nSplit, int* chunksPerSplit, int* xSegs);
SG3_API int sg3_conv2d_wgrad_sum(const sg3_conv2d_wgrad_sum_params* p, void* stream);

/* ----------------------------------------------------------------------
 * What sg3_conv2d, sg3_conv2d_dgrad and sg3_conv2d_wgrad_sum launch for a call: kernel family, template coordinates, geometry and launch
 * values, from the functions the launches themselves use (csrc/sg3_conv2d_plan.h).  Fields a family has no use for are 0.
 * ---------------------------------------------------------------------- */
enum {
    SG3_CONV2D_FP32_MFMA = 0,  /* conv2d_mfma_kernel<KS, STRIDE, WM, WN, TM, TN, CHAINS>: exact fp32 products */
    SG3_CONV2D_F16X3     = 1,  /* conv2d_f16x3_kernel<KS, STRIDE, WM, WN, TM, TN>: fp16 hi/lo operands */
    SG3_CONV2D_DGRAD     = 2,  /* conv2d_dgrad_kernel<KS, STRIDE, WM, WN, TM, TN> */
    SG3_CONV2D_WGRAD_SUM = 3,  /* conv2d_wgrad_sum_kernel<KS, STRIDE>, then conv2d_wgrad_sum_reduce_kernel when nSplit > 1 */
};

typedef struct sg3_conv2d_dispatch_info {
    int32_t        family;     /* SG3_CONV2D_* */
    int32_t        form;       /* forward: what sg3_conv2d_form returns; -1 otherwise */
    int32_t        KS, STRIDE, WM, WN, TM, TN;   /* a workgroup takes 32 WM TM channels x (WN TN rows x 32 columns) */
    int32_t        CHAINS;     /* FP32_MFMA: accumulators per output (1 | 4) */
    int32_t        kc, nch;    /* channels per K chunk, K chunks (dgrad: of the output channels) */
    int32_t        outH, outW; /* size of the forward's output (dgrad, wgrad_sum: of dy) */
    int32_t        xTiles, yTiles, mTiles;
    int32_t        classes;    /* dgrad: pixel parity classes, stride^2, each with tiles of its own */
    int32_t        xSegs, nChunks, nSplit, chunksPerSplit;   /* wgrad_sum: as sg3_conv2d_wgrad_sum_splits describes them */
    int32_t        oTiles, iTiles;   /* wgrad_sum: 64 x 64 (o, i) tiles */
    int32_t        reduceGrid; /* wgrad_sum: workgroups (of 256) of the reduce launch, 0 with one split */
    int32_t        totalBlocks; /* the grid: xTiles yTiles mTiles N (x classes) | oTiles iTiles nSplit */
    int32_t        block;
    int32_t        ldsBytes;   /* dynamic LDS of the launch (0: the kernel's LDS is static) */
} sg3_conv2d_dispatch_info;

/* Host only: no launch, no pointer followed (only whether a pointer is set is read, so placeholders do).  SG3_BAD_ARG for a call the
 * launch rejects, a grid past 2^31 - 1 workgroups included.  `cus` <= 0: the CU count of the current device, 256 without one. */
SG3_API int sg3_conv2d_dispatch(const sg3_conv2d_params* p, int cus, sg3_conv2d_dispatch_info* out);
SG3_API int sg3_conv2d_dgrad_dispatch(const sg3_conv2d_dgrad_params* p, sg3_conv2d_dispatch_info* out);
SG3_API int sg3_conv2d_wgrad_sum_dispatch(const sg3_conv2d_wgrad_sum_params* p, sg3_conv2d_dispatch_info* out);

/* ----------------------------------------------------------------------
 * Training-mode BatchNorm2d (csrc/sg3_bn_train.hip).  Contiguous float32 [N][C][H][W]; per-channel vectors [C]; float64 sums in a
 * fixed order.  `partial` is scratch of 2 C sg3_bn_train_partials(N, H, W) doubles.
 *   stats:       mean (+ meanLo), var (biased), invstd = 1 / sqrt(var + eps), a = gamma invstd, b = beta - mean a   (gamma / beta NULL: 1 / 0)
 *   apply:       v = scale[c] (x - centre[c] - centreLo[c]) + shift[c] (NULL: 0);  pre = v (pre != NULL);  y = v > 0 ? v : v slope[c] (slope != NULL)
 *   bwd_reduce:  sum1[c] = sum dy,  sum2[c] = sum dy t;  mode 0: t = (x - mean[c] - meanLo[c]) invstd[c];  mode 1: t = min(x, 0), sum1 may be NULL,
 *                and masked = dy (x > 0 ? 1 : slope[c]) when asked
 *   bwd_apply:   v = scale[c] (dy - sum1[c] / M - xhat sum2[c] / M),  M = N H W;  v += addend (element strides);  raw = v (raw != NULL);
 *                dx = v (act > 0 ? 1 : slope[c])  (act != NULL: contiguous like dx)
 * ---------------------------------------------------------------------- */
typedef struct sg3_bn_train_stats_params {
    const float*   x;
    const float*   gamma;
    const float*   beta;
    double*        partial;
    float*         mean;
    float*         meanLo;         /* mean - (float)mean: the part of the float64 mean one float does not hold */
    float*         var;
    float*         invstd;
    float*         a;
    float*         b;
    int32_t        N, C, H, W;
    float          eps;
} sg3_bn_train_stats_params;

typedef struct sg3_bn_train_apply_params {
    const float*   x;
    const float*   scale;
    const float*   shift;
    const float*   centre;
    const float*   centreLo;       /* or NULL */
    const float*   slope;
    float*         y;
    float*         pre;
    int32_t        N, C, H, W;
} sg3_bn_train_apply_params;

typedef struct sg3_bn_train_bwd_reduce_params {
    const float*   dy;
    const float*   x;
    const float*   mean;
    const float*   meanLo;         /* or NULL */
    const float*   invstd;
    const float*   slope;          /* [C], with masked */
    float*         masked;         /* mode 1, or NULL: dy (x > 0 ? 1 : slope[c]) */
    double*        partial;
    float*         sum1;
    float*         sum2;
    int32_t        N, C, H, W;
    int32_t        mode;
} sg3_bn_train_bwd_reduce_params;

typedef struct sg3_bn_train_bwd_apply_params {
    const float*   dy;
    const float*   x;
    const float*   mean;
    const float*   meanLo;         /* or NULL */
    const float*   invstd;
    const float*   scale;
    const float*   sum1;
    const float*   sum2;
    const float*   addend;
    int64_t        addStride[4];
    const float*   act;
    const float*   slope;
    float*         dx;
    float*         raw;
    int32_t        N, C, H, W;
} sg3_bn_train_bwd_apply_params;

SG3_API int sg3_bn_train_partials(int N, int H, int W);
SG3_API int sg3_bn_train_stats(const sg3_bn_train_stats_params* p, void* stream);
SG3_API int sg3_bn_train_apply(const sg3_bn_train_apply_params* p, void* stream);
SG3_API int sg3_bn_train_bwd_reduce(const sg3_bn_train_bwd_reduce_params* p, void* stream);
SG3_API int sg3_bn_train_bwd_apply(const sg3_bn_train_bwd_apply_params* p, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SG3_OPS_H */
