"""ctypes binding of libsg3hip.so (C ABI declared in include/sg3_ops.h).

This is the only place that touches the shared library.  Tensors cross the boundary as raw device pointers +
sizes + element strides, launches go to the caller's current HIP stream.  There is NO fallback here: if the
library is missing, or a call fails, a RuntimeError is raised.
"""
import ctypes
import os

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# SG3_LIB: another build of the same library (same-box A/B timing of kernel variants from tools/); the product loads its own lib/ copy
LIB_PATH = os.environ.get('SG3_LIB') or os.path.join(_PKG_ROOT, 'lib', 'libsg3hip.so')

SG3_OK, SG3_NO_KERNEL, SG3_BAD_ARG, SG3_HIP_ERROR = 0, -1, -2, -3
SG3_F32, SG3_F16, SG3_F64 = 0, 1, 2
SG3_CONV_FP32, SG3_CONV_F16X3, SG3_CONV_F16, SG3_CONV_F16X3_F23, SG3_CONV_F16_F23, SG3_CONV_FP32_CHAINS = 0, 1, 2, 3, 4, 5
SG3_MODCONV_FP32_MFMA, SG3_MODCONV_TORGB, SG3_MODCONV_ROWS, SG3_MODCONV_FLAT, SG3_MODCONV_GEMM1, SG3_MODCONV_F23 = range(6)   # sg3_modconv_dispatch_info.family
SG3_FLRELU_NONE, SG3_FLRELU_POINTWISE, SG3_FLRELU_STREAM = range(3)                             # sg3_filtered_lrelu_dispatch_info.kind
SG3_CONV2D_FORM_F16X3 = 16          # sg3_conv2d_form: first f16x3 form (include/sg3_ops.h)
SG3_CONV2D_FP32_MFMA, SG3_CONV2D_F16X3, SG3_CONV2D_DGRAD, SG3_CONV2D_WGRAD_SUM = range(4)       # sg3_conv2d_dispatch_info.family
_DTYPE = {torch.float32: SG3_F32, torch.float16: SG3_F16, torch.float64: SG3_F64}

c_i32, c_i64, c_f32, c_vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


class FilteredLreluParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('y', c_vp), ('b', c_vp), ('s', c_vp), ('fu', c_vp), ('fd', c_vp),
                ('dtype', c_i32), ('N', c_i32), ('C', c_i32), ('xH', c_i32), ('xW', c_i32), ('yH', c_i32), ('yW', c_i32),
                ('xStride', c_i64 * 4), ('yStride', c_i64 * 4), ('bStride', c_i64),
                ('up', c_i32), ('down', c_i32), ('fuW', c_i32), ('fuH', c_i32), ('fdW', c_i32), ('fdH', c_i32),
                ('px0', c_i32), ('py0', c_i32), ('sH', c_i32), ('sWbytes', c_i32), ('sx', c_i32), ('sy', c_i32),
                ('swLimit', c_i32), ('gain', c_f32), ('slope', c_f32), ('clamp', c_f32),
                ('flip', c_i32), ('writeSigns', c_i32), ('readSigns', c_i32), ('ySumPartial', c_vp), ('fdMirror', c_i32), ('yAbsMaxPartial', c_vp)]


class FilteredLreluDispatchInfo(ctypes.Structure):
    PER_LAUNCH = ('U', 'D', 'VPH', 'RADIAL', 'SIGNS', 'G', 'WIDE', 'nStrips', 'TW', 'ox0Base', 'wideBlocks', 'totalBlocks')
    _fields_ = ([(n, c_i32) for n in ('kind', 'launches', 'planesPerWave', 'nChunks', 'chunkRows', 'sumSlots', 'fastAct')] +
                [(n, c_i32 * 2) for n in PER_LAUNCH])

    def as_dict(self):
        """the call-wide fields, and `launch`: one dict of PER_LAUNCH per launch"""
        d = {n: getattr(self, n) for n, t in self._fields_ if t is c_i32}
        d['launch'] = [{n: getattr(self, n)[i] for n in self.PER_LAUNCH} for i in range(self.launches)]
        return d


class FilteredLreluActParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('s', c_vp), ('dtype', c_i32), ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32),
                ('xStride', c_i64 * 4), ('sH', c_i32), ('sW', c_i32), ('sx', c_i32), ('sy', c_i32),
                ('gain', c_f32), ('slope', c_f32), ('clamp', c_f32), ('writeSigns', c_i32), ('readSigns', c_i32)]


class Upfirdn2dParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('f', c_vp), ('y', c_vp), ('dtype', c_i32),
                ('N', c_i32), ('C', c_i32), ('xH', c_i32), ('xW', c_i32), ('yH', c_i32), ('yW', c_i32),
                ('xStride', c_i64 * 4), ('yStride', c_i64 * 4), ('fH', c_i32), ('fW', c_i32), ('fStride', c_i64 * 2),
                ('upx', c_i32), ('upy', c_i32), ('downx', c_i32), ('downy', c_i32), ('padx0', c_i32), ('pady0', c_i32),
                ('flip', c_i32), ('gain', c_f32)]


class BiasActParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('b', c_vp), ('xref', c_vp), ('yref', c_vp), ('dy', c_vp), ('y', c_vp),
                ('dtype', c_i32), ('grad', c_i32), ('act', c_i32), ('alpha', c_f32), ('gain', c_f32), ('clamp', c_f32),
                ('sizeX', c_i64), ('sizeB', c_i32), ('stepB', c_i32)]


class ModconvParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('wPacked', c_vp), ('sIn', c_vp), ('dcoef', c_vp), ('out', c_vp), ('dtype', c_i32),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('k', c_i32), ('pad', c_i32), ('precision', c_i32),
                ('epilogueBias', c_vp), ('epilogueClamp', c_f32), ('epilogueScale', c_f32), ('outRowStride', c_i32),
                ('splitScratch', c_vp), ('splitScratchFloats', c_i64)]


class ModconvDispatchInfo(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ('family', 'WM', 'WN', 'TM', 'TN', 'SPLIT', 'PACK', 'NBUF', 'M16', 'nch', 'xTiles', 'yTiles', 'mTiles',
                                     'kSplits', 'totalBlocks', 'gridX', 'gridY', 'block', 'ldsBytes', 'outPitch', 'reduceGrid')]


class FourierParams(ctypes.Structure):
    _fields_ = [('grid', c_vp), ('freqs', c_vp), ('phases', c_vp), ('amps', c_vp), ('out', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32)]


class InputTransformParams(ctypes.Structure):
    _fields_ = [('t', c_vp), ('user', c_vp), ('freqs', c_vp), ('phases', c_vp), ('outFreqs', c_vp), ('outPhases', c_vp), ('outAmps', c_vp),
                ('N', c_i32), ('C', c_i32), ('normalise', c_i32), ('userStrideN', c_i32), ('bandwidth', c_f32), ('samplingRate', c_f32)]


class ModgradParams(ctypes.Structure):
    _fields_ = [('G', c_vp), ('w', c_vp), ('s', c_vp), ('inputGain', c_vp), ('inputGainMode', c_i32), ('dW', c_vp), ('dS', c_vp),
                ('a', c_vp), ('dSn', c_vp), ('N', c_i32), ('O', c_i32), ('I', c_i32), ('T', c_i32), ('demodulate', c_i32)]


class SeParams(ctypes.Structure):
    _fields_ = [('res', c_vp), ('shortcut', c_vp), ('scStride', c_i64 * 4), ('fc1', c_vp), ('fc2', c_vp), ('mean', c_vp), ('out', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('R', c_i32)]


class UnfoldParams(ctypes.Structure):
    _fields_ = [('src', c_vp), ('srcStride', c_i64 * 5), ('dst', c_vp), ('G', c_i32), ('N', c_i32), ('C', c_i32), ('IH', c_i32), ('IW', c_i32),
                ('slope', c_f32)]


class HeadGemmParams(ctypes.Structure):
    _fields_ = [('a', c_vp), ('wPacked', c_vp), ('colScale', c_vp), ('bias', c_vp), ('c', c_vp), ('rangeFlag', c_vp),
                ('G', c_i32), ('M', c_i32), ('K', c_i32), ('N', c_i32), ('slope', c_f32)]


class AffineBatchParams(ctypes.Structure):
    _fields_ = [('ws', c_vp), ('wsStrideN', c_i64), ('wsStrideL', c_i64), ('weight', c_vp), ('bias', c_vp), ('scale', c_vp),
                ('rowStart', c_vp), ('wsIndex', c_vp), ('out', c_vp), ('N', c_i32), ('wDim', c_i32), ('layers', c_i32), ('rows', c_i32)]


class ModconvPrepParams(ctypes.Structure):
    _fields_ = [('w', c_vp), ('s', c_vp), ('wPacked', c_vp), ('wsq', c_vp), ('sIn', c_vp), ('dcoef', c_vp),
                ('inputGain', c_vp), ('inputGainMode', c_i32),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('k', c_i32), ('demodulate', c_i32), ('precision', c_i32), ('xBound', c_f32),
                ('xBoundDev', c_vp), ('reuseWeights', c_i32)]


class WgradParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('dy', c_vp), ('partial', c_vp), ('scaleX', c_vp), ('scaleDy', c_vp), ('dtype', c_i32),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('k', c_i32), ('pad', c_i32),
                ('nBands', c_i32), ('nSegGroups', c_i32), ('scalesAreAmax', c_i32)]


class Conv2dParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('wPacked', c_vp), ('inScale', c_vp), ('inShift', c_vp), ('bias', c_vp), ('slope', c_vp), ('out', c_vp),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('k', c_i32), ('stride', c_i32), ('pad', c_i32),
                ('act', c_i32), ('precision', c_i32), ('rangeFlag', c_vp), ('wScale', c_vp)]


class ImageFinishParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('xStride', c_i64 * 4), ('y', c_vp), ('yStride', c_i64 * 4),
                ('B', c_i32), ('H', c_i32), ('W', c_i32), ('h', c_i32), ('w', c_i32),
                ('boundsH', c_vp), ('coeffsH', c_vp), ('kH', c_i32), ('boundsV', c_vp), ('coeffsV', c_vp), ('kV', c_i32)]


class LatentMapperParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('weight', c_vp), ('bias', c_vp), ('out', c_vp), ('delta', c_vp), ('scratch', c_vp),
                ('N', c_i32), ('L', c_i32), ('D', c_i32), ('groups', c_i32), ('levelBegin', c_i32 * 4), ('levelEnd', c_i32 * 4),
                ('alpha', c_f32)]


class LatentMapperTrainParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('weight', c_vp), ('bias', c_vp), ('out', c_vp), ('delta', c_vp), ('acts', c_vp),
                ('N', c_i32), ('L', c_i32), ('D', c_i32), ('groups', c_i32), ('levelBegin', c_i32 * 4), ('levelEnd', c_i32 * 4),
                ('alpha', c_f32)]


class LatentMapperBackwardParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('weight', c_vp), ('acts', c_vp), ('delta', c_vp), ('dDelta', c_vp), ('dOut', c_vp),
                ('dx', c_vp), ('dW', c_vp), ('dB', c_vp), ('scratch', c_vp),
                ('N', c_i32), ('L', c_i32), ('D', c_i32), ('groups', c_i32), ('levelBegin', c_i32 * 4), ('levelEnd', c_i32 * 4),
                ('alpha', c_f32), ('wScale', c_f32 * 16), ('bScale', c_f32 * 16)]


class RangerTensor(ctypes.Structure):
    _fields_ = [('p', c_vp), ('grad', c_vp), ('expAvg', c_vp), ('expAvgSq', c_vp), ('slow', c_vp),
                ('rows', c_i32), ('cols', c_i32), ('centralise', c_i32), ('reserved', c_i32)]


class RangerParams(ctypes.Structure):
    _fields_ = [('t', RangerTensor * 32), ('count', c_i32),
                ('beta1', c_f32), ('beta2', c_f32), ('oneMinusBeta1', c_f32), ('oneMinusBeta2', c_f32), ('eps', c_f32), ('decay', c_f32),
                ('stepLr', c_f32), ('alpha', c_f32), ('adaptive', c_i32), ('lookahead', c_i32)]


class ClipPreprocessParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('xStride', c_i64 * 4), ('y', c_vp), ('yStride', c_i64 * 4),
                ('B', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('h', c_i32), ('w', c_i32), ('mean', c_f32 * 3), ('std', c_f32 * 3)]


SG3_CLIP_EPI_F32, SG3_CLIP_EPI_F16, SG3_CLIP_EPI_QUICKGELU_F16, SG3_CLIP_EPI_RESIDUAL, SG3_CLIP_EPI_PATCH = 0, 1, 2, 3, 4
SG3_CLIP_EPI_QUICKGELU_SAVE_F16, SG3_CLIP_EPI_DQUICKGELU_F16, SG3_CLIP_EPI_PATCH_ADJOINT = 5, 6, 7


class ClipLayernormParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('gamma', c_vp), ('beta', c_vp), ('out', c_vp), ('xRowStride', c_i64), ('rows', c_i32), ('D', c_i32),
                ('outDtype', c_i32), ('eps', c_f32)]


class ClipGemmParams(ctypes.Structure):
    _fields_ = [('a', c_vp), ('w', c_vp), ('bias', c_vp), ('out', c_vp), ('pos', c_vp), ('cls', c_vp),
                ('M', c_i32), ('K', c_i32), ('N', c_i32), ('epilogue', c_i32), ('P', c_i32), ('R', c_i32)]


class ClipAttentionParams(ctypes.Structure):
    _fields_ = [('qkv', c_vp), ('out', c_vp), ('B', c_i32), ('L', c_i32), ('heads', c_i32), ('causal', c_i32)]


class ClipEmbedParams(ctypes.Structure):
    _fields_ = [('tokens', c_vp), ('table', c_vp), ('pos', c_vp), ('out', c_vp), ('B', c_i32), ('L', c_i32), ('D', c_i32), ('vocab', c_i32)]


class ClipGemmGradParams(ctypes.Structure):
    _fields_ = [('a', c_vp), ('w', c_vp), ('bias', c_vp), ('out', c_vp), ('aux', c_vp), ('scale', c_vp),
                ('M', c_i32), ('K', c_i32), ('N', c_i32), ('epilogue', c_i32), ('P', c_i32), ('R', c_i32), ('aF32', c_i32)]


class ClipLayernormBwdParams(ctypes.Structure):
    _fields_ = [('dy', c_vp), ('x', c_vp), ('gamma', c_vp), ('dx', c_vp), ('dyRowStride', c_i64), ('xRowStride', c_i64), ('dxRowStride', c_i64),
                ('rows', c_i32), ('D', c_i32), ('accumulate', c_i32), ('eps', c_f32)]


class ClipAttentionBwdParams(ctypes.Structure):
    _fields_ = [('qkv', c_vp), ('dout', c_vp), ('dqkv', c_vp), ('B', c_i32), ('L', c_i32), ('heads', c_i32), ('causal', c_i32)]


class ClipGradScaleParams(ctypes.Structure):
    _fields_ = [('g', c_vp), ('out16', c_vp), ('inv', c_vp), ('B', c_i32), ('E', c_i32)]


class ClipResampleParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('xStride', c_i64 * 4), ('y', c_vp), ('yStride', c_i64 * 4),
                ('B', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('oh', c_i32), ('ow', c_i32), ('up', c_i32), ('k', c_i32), ('adjoint', c_i32)]


class FacePoolParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('xStride', c_i64 * 4), ('y', c_vp), ('yStride', c_i64 * 4),
                ('B', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('pool', c_i32), ('adjoint', c_i32)]


class Conv2dDgradParams(ctypes.Structure):
    _fields_ = [('dy', c_vp), ('wPacked', c_vp), ('dx', c_vp), ('act', c_vp), ('slope', c_vp), ('addend', c_vp), ('addStride', c_i64 * 4),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('OH', c_i32), ('OW', c_i32), ('k', c_i32), ('stride', c_i32)]


class SeBwdParams(ctypes.Structure):
    _fields_ = [('dout', c_vp), ('res', c_vp), ('mean', c_vp), ('fc1', c_vp), ('fc2', c_vp), ('dg', c_vp), ('dres', c_vp), ('dscatter', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('R', c_i32), ('inH', c_i32), ('inW', c_i32)]


class LpipsPrepareParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('xStride', c_i64 * 4), ('canvas', c_vp), ('scale', c_vp), ('N', c_i32), ('H', c_i32), ('W', c_i32),
                ('mean', c_f32 * 3), ('std', c_f32 * 3)]


class Conv2dK5Params(ctypes.Structure):
    _fields_ = [('x', c_vp), ('wPacked', c_vp), ('bias', c_vp), ('out', c_vp),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('relu', c_i32)]


class Maxpool3s2Params(ctypes.Structure):
    _fields_ = [('x', c_vp), ('y', c_vp), ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32)]


class Maxpool3s2BwdParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('dy', c_vp), ('addend', c_vp), ('dx', c_vp), ('dxStride', c_i64 * 4),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('reluMask', c_i32)]


class LpipsHeadParams(ctypes.Structure):
    _fields_ = [('fx', c_vp), ('fy', c_vp), ('lin', c_vp), ('value', c_vp), ('dfx', c_vp), ('partial', c_vp), ('counter', c_vp),
                ('N', c_i32), ('C', c_i32), ('h', c_i32), ('w', c_i32), ('reluMask', c_i32)]


class Conv2dWgradSumParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('dy', c_vp), ('inScale', c_vp), ('inShift', c_vp), ('dw', c_vp), ('partial', c_vp),
                ('N', c_i32), ('I', c_i32), ('O', c_i32), ('H', c_i32), ('W', c_i32), ('k', c_i32), ('stride', c_i32)]


class Conv2dDispatchInfo(ctypes.Structure):
    _fields_ = [(n, c_i32) for n in ('family', 'form', 'KS', 'STRIDE', 'WM', 'WN', 'TM', 'TN', 'CHAINS', 'kc', 'nch', 'outH', 'outW', 'xTiles', 'yTiles',
                                     'mTiles', 'classes', 'xSegs', 'nChunks', 'nSplit', 'chunksPerSplit', 'oTiles', 'iTiles', 'reduceGrid', 'totalBlocks',
                                     'block', 'ldsBytes')]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BnTrainStatsParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('gamma', c_vp), ('beta', c_vp), ('partial', c_vp), ('mean', c_vp), ('meanLo', c_vp), ('var', c_vp), ('invstd', c_vp), ('a', c_vp), ('b', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('eps', c_f32)]


class BnTrainApplyParams(ctypes.Structure):
    _fields_ = [('x', c_vp), ('scale', c_vp), ('shift', c_vp), ('centre', c_vp), ('centreLo', c_vp), ('slope', c_vp), ('y', c_vp), ('pre', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32)]


class BnTrainBwdReduceParams(ctypes.Structure):
    _fields_ = [('dy', c_vp), ('x', c_vp), ('mean', c_vp), ('meanLo', c_vp), ('invstd', c_vp), ('slope', c_vp), ('masked', c_vp), ('partial', c_vp), ('sum1', c_vp), ('sum2', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('mode', c_i32)]


class BnTrainBwdApplyParams(ctypes.Structure):
    _fields_ = [('dy', c_vp), ('x', c_vp), ('mean', c_vp), ('meanLo', c_vp), ('invstd', c_vp), ('scale', c_vp), ('sum1', c_vp), ('sum2', c_vp),
                ('addend', c_vp), ('addStride', c_i64 * 4), ('act', c_vp), ('slope', c_vp), ('dx', c_vp), ('raw', c_vp),
                ('N', c_i32), ('C', c_i32), ('H', c_i32), ('W', c_i32)]


# every symbol include/sg3_ops.h declares: (name, restype, argtypes)
EXPORTS = [
    ('sg3_abi_version', ctypes.c_int, []),
    ('sg3_last_error', ctypes.c_char_p, []),
    ('sg3_device_count', ctypes.c_int, []),
    ('sg3_filtered_lrelu', ctypes.c_int, [ctypes.POINTER(FilteredLreluParams), c_vp]),
    ('sg3_filtered_lrelu_planes_per_wave', ctypes.c_int, [ctypes.POINTER(FilteredLreluParams)]),
    ('sg3_filtered_lrelu_dispatch', ctypes.c_int, [ctypes.POINTER(FilteredLreluParams), ctypes.POINTER(FilteredLreluDispatchInfo)]),
    ('sg3_filtered_lrelu_force_up4_wide', ctypes.c_int, [ctypes.c_int]),
    ('sg3_filtered_lrelu_stream_grid', ctypes.c_int, [ctypes.POINTER(FilteredLreluParams)] + [ctypes.POINTER(ctypes.c_int)] * 5),
    ('sg3_filtered_lrelu_fast_threshold', ctypes.c_float, [c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float]),
    ('sg3_filtered_lrelu_has_kernel', ctypes.c_int, [ctypes.c_int] * 6),
    ('sg3_filtered_lrelu_sum_slots', ctypes.c_int, [ctypes.c_int] * 5),
    ('sg3_filtered_lrelu_finish_partials', ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp, c_vp]),
    ('sg3_filtered_lrelu_shape', ctypes.c_int, [ctypes.c_int] * 12 + [ctypes.POINTER(ctypes.c_int)] * 5),
    ('sg3_filtered_lrelu_act', ctypes.c_int, [ctypes.POINTER(FilteredLreluActParams), c_vp]),
    ('sg3_upfirdn2d', ctypes.c_int, [ctypes.POINTER(Upfirdn2dParams), c_vp]),
    ('sg3_upfirdn2d_shape', ctypes.c_int, [ctypes.c_int] * 12 + [ctypes.POINTER(ctypes.c_int)] * 2),
    ('sg3_bias_act', ctypes.c_int, [ctypes.POINTER(BiasActParams), c_vp]),
    ('sg3_modconv_packed_floats', ctypes.c_int64, [ctypes.c_int] * 4),
    ('sg3_modulated_conv2d', ctypes.c_int, [ctypes.POINTER(ModconvParams), c_vp]),
    ('sg3_modconv_split_scratch_floats', ctypes.c_int64, [ctypes.POINTER(ModconvParams)]),
    ('sg3_modconv_dispatch', ctypes.c_int, [ctypes.POINTER(ModconvParams), ctypes.c_int, ctypes.POINTER(ModconvDispatchInfo)]),
    ('sg3_modconv_f23_supported', ctypes.c_int, [ctypes.c_int] * 8),
    ('sg3_modconv_f23_force_rows', ctypes.c_int, [ctypes.c_int]),
    ('sg3_fourier_features', ctypes.c_int, [ctypes.POINTER(FourierParams), c_vp]),
    ('sg3_input_transform', ctypes.c_int, [ctypes.POINTER(InputTransformParams), c_vp]),
    ('sg3_affine_batch', ctypes.c_int, [ctypes.POINTER(AffineBatchParams), c_vp]),
    ('sg3_se_residual', ctypes.c_int, [ctypes.POINTER(SeParams), c_vp]),
    ('sg3_unfold3x3s2', ctypes.c_int, [ctypes.POINTER(UnfoldParams), c_vp]),
    ('sg3_head_gemm_packed_halfs', ctypes.c_int64, [ctypes.c_int] * 3),
    ('sg3_head_gemm_pack', ctypes.c_int, [c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp, c_vp]),
    ('sg3_head_gemm', ctypes.c_int, [ctypes.POINTER(HeadGemmParams), c_vp]),
    ('sg3_modulation_backward', ctypes.c_int, [ctypes.POINTER(ModgradParams), c_vp]),
    ('sg3_modconv_transpose_weights', ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp]),
    ('sg3_modulated_conv2d_prep', ctypes.c_int, [ctypes.POINTER(ModconvPrepParams), c_vp]),
    ('sg3_modulated_conv2d_prep_batch', ctypes.c_int, [ctypes.POINTER(ModconvPrepParams), ctypes.c_int, c_vp]),
    ('sg3_conv2d', ctypes.c_int, [ctypes.POINTER(Conv2dParams), c_vp]),
    ('sg3_conv2d_form', ctypes.c_int, [ctypes.POINTER(Conv2dParams)]),
    ('sg3_conv2d_wgrad_splits', ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)] * 2),
    ('sg3_conv2d_wgrad', ctypes.c_int, [ctypes.POINTER(WgradParams), c_vp]),
    ('sg3_conv2d_pack', ctypes.c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, c_vp]),
    ('sg3_resample_coeffs', ctypes.c_int, [ctypes.c_int32, ctypes.c_int32, c_vp, c_vp]),
    ('sg3_image_finish', ctypes.c_int, [ctypes.POINTER(ImageFinishParams), c_vp]),
    ('sg3_latent_mapper', ctypes.c_int, [ctypes.POINTER(LatentMapperParams), c_vp]),
    ('sg3_latent_mapper_train_forward', ctypes.c_int, [ctypes.POINTER(LatentMapperTrainParams), c_vp]),
    ('sg3_latent_mapper_backward', ctypes.c_int, [ctypes.POINTER(LatentMapperBackwardParams), c_vp]),
    ('sg3_ranger_step', ctypes.c_int, [ctypes.POINTER(RangerParams), c_vp]),
    ('sg3_clip_preprocess', ctypes.c_int, [ctypes.POINTER(ClipPreprocessParams), c_vp]),
    ('sg3_clip_supported', ctypes.c_int, [ctypes.c_int] * 3),
    ('sg3_clip_layernorm', ctypes.c_int, [ctypes.POINTER(ClipLayernormParams), c_vp]),
    ('sg3_clip_gemm', ctypes.c_int, [ctypes.POINTER(ClipGemmParams), c_vp]),
    ('sg3_clip_attention', ctypes.c_int, [ctypes.POINTER(ClipAttentionParams), c_vp]),
    ('sg3_clip_embed', ctypes.c_int, [ctypes.POINTER(ClipEmbedParams), c_vp]),
    ('sg3_clip_gemm_grad', ctypes.c_int, [ctypes.POINTER(ClipGemmGradParams), c_vp]),
    ('sg3_clip_layernorm_bwd', ctypes.c_int, [ctypes.POINTER(ClipLayernormBwdParams), c_vp]),
    ('sg3_clip_attention_bwd', ctypes.c_int, [ctypes.POINTER(ClipAttentionBwdParams), c_vp]),
    ('sg3_clip_grad_scale', ctypes.c_int, [ctypes.POINTER(ClipGradScaleParams), c_vp]),
    ('sg3_clip_resample', ctypes.c_int, [ctypes.POINTER(ClipResampleParams), c_vp]),
    ('sg3_face_pool', ctypes.c_int, [ctypes.POINTER(FacePoolParams), c_vp]),
    ('sg3_conv2d_dgrad', ctypes.c_int, [ctypes.POINTER(Conv2dDgradParams), c_vp]),
    ('sg3_se_residual_bwd', ctypes.c_int, [ctypes.POINTER(SeBwdParams), c_vp]),
    ('sg3_lpips_prepare', ctypes.c_int, [ctypes.POINTER(LpipsPrepareParams), c_vp]),
    ('sg3_lpips_prepare_bwd', ctypes.c_int, [ctypes.POINTER(LpipsPrepareParams), c_vp]),
    ('sg3_conv2d_k5_packed_floats', ctypes.c_int64, [ctypes.c_int] * 2),
    ('sg3_conv2d_k5_pack', ctypes.c_int, [c_vp, c_vp, ctypes.c_int, ctypes.c_int, c_vp]),
    ('sg3_conv2d_k5', ctypes.c_int, [ctypes.POINTER(Conv2dK5Params), c_vp]),
    ('sg3_maxpool3s2', ctypes.c_int, [ctypes.POINTER(Maxpool3s2Params), c_vp]),
    ('sg3_maxpool3s2_bwd', ctypes.c_int, [ctypes.POINTER(Maxpool3s2BwdParams), c_vp]),
    ('sg3_lpips_head_blocks', ctypes.c_int, [ctypes.c_int] * 2),
    ('sg3_lpips_head', ctypes.c_int, [ctypes.POINTER(LpipsHeadParams), c_vp]),
    ('sg3_conv2d_wgrad_sum_splits', ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)] * 3),
    ('sg3_conv2d_wgrad_sum', ctypes.c_int, [ctypes.POINTER(Conv2dWgradSumParams), c_vp]),
    ('sg3_conv2d_dispatch', ctypes.c_int, [ctypes.POINTER(Conv2dParams), ctypes.c_int, ctypes.POINTER(Conv2dDispatchInfo)]),
    ('sg3_conv2d_dgrad_dispatch', ctypes.c_int, [ctypes.POINTER(Conv2dDgradParams), ctypes.POINTER(Conv2dDispatchInfo)]),
    ('sg3_conv2d_wgrad_sum_dispatch', ctypes.c_int, [ctypes.POINTER(Conv2dWgradSumParams), ctypes.POINTER(Conv2dDispatchInfo)]),
    ('sg3_bn_train_partials', ctypes.c_int, [ctypes.c_int] * 3),
    ('sg3_bn_train_stats', ctypes.c_int, [ctypes.POINTER(BnTrainStatsParams), c_vp]),
    ('sg3_bn_train_apply', ctypes.c_int, [ctypes.POINTER(BnTrainApplyParams), c_vp]),
    ('sg3_bn_train_bwd_reduce', ctypes.c_int, [ctypes.POINTER(BnTrainBwdReduceParams), c_vp]),
    ('sg3_bn_train_bwd_apply', ctypes.c_int, [ctypes.POINTER(BnTrainBwdApplyParams), c_vp]),
]

_lib = None
launch_count = 0      # number of successful kernel-launching ABI calls (bench / smoke assert the HIP path ran)


def load():
    """Load libsg3hip.so (after torch, so both share torch's libamdhip64.so.7).  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'libsg3hip.so not found at {LIB_PATH}: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                f'(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for GPU tensors.')
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, res, args in EXPORTS:
            fn = getattr(lib, name)          # AttributeError here = header / library mismatch
            fn.restype, fn.argtypes = res, args
        if lib.sg3_abi_version() != 1:
            raise RuntimeError(f'libsg3hip.so ABI version {lib.sg3_abi_version()} != 1')
        _lib = lib
    return _lib


def is_built():
    return os.path.exists(LIB_PATH)


def last_error():
    msg = load().sg3_last_error()
    return msg.decode() if msg else ''


def stream_ptr(device):
    return c_vp(torch.cuda.current_stream(device).cuda_stream)


def dtype_code(dtype):
    try:
        return _DTYPE[dtype]
    except KeyError:
        raise RuntimeError(f'unsupported dtype {dtype}') from None


def ptr(t):
    return c_vp(t.data_ptr()) if t is not None and t.numel() > 0 else c_vp(0)


def strides4(t):
    return (c_i64 * 4)(*[int(s) for s in t.stride()])


def check(rc, what, allow_no_kernel=False):
    """Translate an ABI return code: 0 ok; -1 passes through when allowed; everything else raises RuntimeError."""
    global launch_count
    if rc == SG3_OK:
        launch_count += 1
        return rc
    if rc == SG3_NO_KERNEL and allow_no_kernel:
        return rc
    raise RuntimeError(f'{what} failed (rc={rc}): {last_error()}')
