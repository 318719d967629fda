"""One full sg3_modulated_conv2d call per convolution kernel instantiation the launch plan can choose (csrc/sg3_modconv_plan.h).

TABLE is a literal: tools/find_modconv_variant_cases.py searched it on the CPU with sg3_modconv_dispatch(..., cus=256) and printed
it; nothing here or in the tests searches at run time.  tests/test_modconv_variant_cases_cpu.py holds every row to the plan it is
filed under and to the rules below; tests/test_gpu_modconv_variants.py runs every row on the GPU against float64.

A row is filed under a VARIANT = (dtype, k, family, WM, WN, TM, TN, SPLIT, PACK, NBUF, M16), the coordinates of
test_modconv_dispatch_cpu._variants(), and is one of these KINDS:

  variant  the smallest ragged call (below) the plan maps to the variant: one per variant of _variants()
  m16      the same for the twelve M16 = 0 kernels of the 1x1 GEMM, which need SG3_CONV1_MFMA32=1 in the environment (read once per
           process: these rows are planned and run in a child process)
  pad0     the 3x3 ROWS / FLAT / FP32_MFMA variants again at padding 0, the geometry of the data-gradient call (same output plane)
  padalt   one transform-domain variant per tensor type at the other padding it supports (0)
  ksplit   K split over 2 and 4 workgroups per tile (scratch on offer): FLAT for every (tensor type, SPLIT), GEMM1 for fp32 tensors
           and each SPLIT; the fp16 FLAT rows run modconv_split_reduce_kernel<_Float16>, the others <float>
  torgb    the ToRGB kernel at the other plane size class (H W divisible by 4: four pixels per thread; not: one)
  nodemod  one fp32-tensor row per family with demodulation off and styles x 1000 (the power-of-two rescale of the split forms);
           fp16 tensors cannot hold the undemodulated result

Which shape is "the smallest ragged call".  Among the shapes the plan maps to the variant, the one with the fewest multiply-adds
N I O outH outW k^2 that is

  RAGGED  O is no multiple of the tile's channels; outW no multiple of 32 (flat pixel tiles: the plane no multiple of the run);
          outH no multiple of the rows per workgroup; I no multiple of 16 (32 for the two-chunk stages of the 1x1 GEMM); PACK variants
          have I % 16 in 1 .. 4 by themselves.  ToRGB has no tile: O = 3, I % 16 != 0.
  SPANNING  along every tiled dimension there is a full tile AND a ragged one: O > tile channels, outW > 32 (plane > run), outH > rows
          per workgroup, I > one K step.  A one-tile shape is ragged too, but never multiplies a tile index by anything: the batch
          stride, the M-tile stride of the packed weights, the K-loop prefetch and the XCD renumbering of block ids would go unrun.

with N = 2 wherever the plan still picks the variant with two samples (batch stride, per-sample scales).  Where no such shape maps
to a variant the row says why in `exempt` and takes the nearest shape.  Every row stays below MAX_MACS multiply-adds.
"""

FP32_MFMA, TORGB, ROWS, FLAT, GEMM1, F23 = range(6)                  # sg3_modconv_dispatch_info.family
FAMILY_NAMES = ('mfma', 'torgb', 'rows', 'flat', 'gemm1', 'f23')
CONV_FP32, CONV_F16X3, CONV_F16, CONV_F16X3_F23, CONV_F16_F23 = range(5)       # sg3_modconv_params.precision
MAX_MACS = 2 * 10 ** 9
M16_ENV = ('SG3_CONV1_MFMA32', '1')

COLUMNS = ('kind', 'dtype', 'N', 'I', 'O', 'H', 'W', 'k', 'pad', 'precision', 'demodulate', 'scratch', 'forcedRows', 'kSplits', 'variant', 'exempt')

# fmt: off
TABLE = [
    ('variant', 0, 2, 17, 129, 17, 33, 1, 0, 0, 1, 0, 0, 0, (0, 1, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 33, 9, 33, 1, 0, 0, 1, 0, 0, 0, (0, 1, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 0, 2, 17, 161, 5, 33, 1, 0, 0, 1, 0, 0, 0, (0, 1, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 225, 5, 33, 1, 0, 0, 1, 0, 0, 0, (0, 1, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 129, 15, 31, 3, 2, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 33, 7, 31, 3, 2, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 0, 2, 17, 161, 3, 31, 3, 2, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 225, 3, 31, 3, 2, 0, 1, 0, 0, 0, (0, 3, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 129, 17, 33, 1, 0, 0, 1, 0, 0, 0, (1, 1, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 33, 9, 33, 1, 0, 0, 1, 0, 0, 0, (1, 1, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 1, 2, 17, 161, 5, 33, 1, 0, 0, 1, 0, 0, 0, (1, 1, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 225, 5, 33, 1, 0, 0, 1, 0, 0, 0, (1, 1, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 129, 15, 31, 3, 2, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 33, 7, 31, 3, 2, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 1, 2, 17, 161, 3, 31, 3, 2, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 225, 3, 31, 3, 2, 0, 1, 0, 0, 0, (1, 3, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 3, 33, 33, 1, 0, 0, 1, 0, 0, 0, (0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 3, 33, 33, 1, 0, 0, 1, 0, 0, 0, (1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 65, 15, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 65, 15, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 0, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 65, 15, 31, 3, 2, 1, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 65, 15, 31, 3, 2, 1, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 1, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 65, 126, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 5, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 65, 126, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 5, 0, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 97, 7, 99, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 97, 7, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 0, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 97, 7, 99, 3, 2, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 97, 7, 31, 3, 2, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 1, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 1345, 15, 99, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 5, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 1345, 15, 99, 3, 2, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 5, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 97, 126, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 6, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 17, 97, 126, 31, 3, 2, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 6, 0, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 15, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 65, 15, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 0, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 15, 31, 3, 2, 1, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 65, 15, 31, 3, 2, 1, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 1, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 126, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 5, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 65, 126, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 5, 0, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 97, 7, 99, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 97, 7, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 0, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 97, 7, 99, 3, 2, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 97, 7, 31, 3, 2, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 1, 1, 0, 0), ''),
    ('variant', 1, 2, 21, 1345, 15, 99, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 5, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 1345, 15, 99, 3, 2, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 5, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 97, 126, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 6, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 17, 97, 126, 31, 3, 2, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 6, 0, 1, 0, 0), ''),
    ('variant', 0, 2, 21, 97, 1, 41, 3, 2, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 97, 1, 41, 3, 2, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 2305, 12, 53, 3, 2, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 3, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 2305, 12, 53, 3, 2, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 3, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 2305, 31, 33, 3, 2, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 2305, 31, 33, 3, 2, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 97, 1, 41, 3, 2, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 97, 1, 41, 3, 2, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 2305, 12, 53, 3, 2, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 3, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 2305, 12, 53, 3, 2, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 3, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 2305, 31, 33, 3, 2, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 2305, 31, 33, 3, 2, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 33, 65, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 0, 0, 1, 0), ''),
    ('variant', 0, 2, 257, 33, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 0, 0, 2, 1), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 0, 2, 33, 65, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 1, 0, 1, 0), ''),
    ('variant', 0, 2, 257, 33, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 1, 0, 2, 1), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 0, 2, 257, 257, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 2, 4, 2, 2, 0, 0, 2, 1), ''),
    ('variant', 0, 2, 257, 257, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 2, 4, 2, 2, 1, 0, 2, 1), ''),
    ('variant', 0, 2, 257, 385, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 2, 4, 4, 2, 0, 0, 2, 1), ''),
    ('variant', 0, 2, 257, 385, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 2, 4, 4, 2, 1, 0, 2, 1), ''),
    ('variant', 1, 2, 33, 65, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 0, 0, 1, 0), ''),
    ('variant', 1, 2, 257, 33, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 0, 0, 2, 1), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 1, 2, 33, 65, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 1, 0, 1, 0), ''),
    ('variant', 1, 2, 257, 33, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 1, 0, 2, 1), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('variant', 1, 2, 257, 257, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 2, 4, 2, 2, 0, 0, 2, 1), ''),
    ('variant', 1, 2, 257, 257, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 2, 4, 2, 2, 1, 0, 2, 1), ''),
    ('variant', 1, 2, 257, 385, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 2, 4, 4, 2, 0, 0, 2, 1), ''),
    ('variant', 1, 2, 257, 385, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 2, 4, 4, 2, 1, 0, 2, 1), ''),
    ('variant', 0, 2, 21, 65, 7, 32, 3, 2, 3, 1, 0, 4, 0, (0, 3, 5, 2, 4, 1, 4, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 65, 9, 32, 3, 2, 3, 1, 0, 5, 0, (0, 3, 5, 2, 4, 1, 5, 1, 0, 0, 0), ''),
    ('variant', 0, 2, 21, 65, 13, 32, 3, 2, 3, 1, 0, 7, 0, (0, 3, 5, 2, 4, 1, 7, 1, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 7, 32, 3, 2, 4, 1, 0, 4, 0, (1, 3, 5, 2, 4, 1, 4, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 9, 32, 3, 2, 4, 1, 0, 5, 0, (1, 3, 5, 2, 4, 1, 5, 0, 0, 0, 0), ''),
    ('variant', 1, 2, 21, 65, 13, 32, 3, 2, 4, 1, 0, 7, 0, (1, 3, 5, 2, 4, 1, 7, 0, 0, 0, 0), ''),
    ('m16', 0, 2, 257, 33, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 0, 0, 2, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('m16', 0, 2, 257, 33, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 1, 0, 2, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('m16', 0, 2, 257, 257, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 2, 4, 2, 2, 0, 0, 2, 0), ''),
    ('m16', 0, 2, 257, 257, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 2, 4, 2, 2, 1, 0, 2, 0), ''),
    ('m16', 0, 2, 257, 385, 2, 129, 1, 0, 2, 1, 0, 0, 0, (0, 1, 4, 2, 4, 4, 2, 0, 0, 2, 0), ''),
    ('m16', 0, 2, 257, 385, 2, 129, 1, 0, 1, 1, 0, 0, 0, (0, 1, 4, 2, 4, 4, 2, 1, 0, 2, 0), ''),
    ('m16', 1, 2, 257, 33, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 0, 0, 2, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('m16', 1, 2, 257, 33, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 1, 8, 2, 1, 1, 0, 2, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('m16', 1, 2, 257, 257, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 2, 4, 2, 2, 0, 0, 2, 0), ''),
    ('m16', 1, 2, 257, 257, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 2, 4, 2, 2, 1, 0, 2, 0), ''),
    ('m16', 1, 2, 257, 385, 2, 129, 1, 0, 2, 1, 0, 0, 0, (1, 1, 4, 2, 4, 4, 2, 0, 0, 2, 0), ''),
    ('m16', 1, 2, 257, 385, 2, 129, 1, 0, 1, 1, 0, 0, 0, (1, 1, 4, 2, 4, 4, 2, 1, 0, 2, 0), ''),
    ('pad0', 0, 2, 17, 129, 19, 35, 3, 0, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 33, 11, 35, 3, 0, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('pad0', 0, 2, 17, 161, 7, 35, 3, 0, 0, 1, 0, 0, 0, (0, 3, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 225, 7, 35, 3, 0, 0, 1, 0, 0, 0, (0, 3, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 129, 19, 35, 3, 0, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 33, 11, 35, 3, 0, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 2, 2, 0, 0, 0, 0), 'the plan takes this tile for O <= 64 only: one M tile'),
    ('pad0', 1, 2, 17, 161, 7, 35, 3, 0, 0, 1, 0, 0, 0, (1, 3, 0, 1, 4, 3, 1, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 225, 7, 35, 3, 0, 0, 1, 0, 0, 0, (1, 3, 0, 2, 2, 2, 2, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 65, 19, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 65, 19, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 0, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 65, 19, 35, 3, 0, 1, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 1, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 65, 19, 35, 3, 0, 1, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 1, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 65, 130, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 5, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 65, 130, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 1, 4, 1, 5, 0, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 97, 11, 103, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 97, 11, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 0, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 97, 11, 103, 3, 0, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 97, 11, 35, 3, 0, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 4, 1, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 1345, 19, 103, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 5, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 1345, 19, 103, 3, 0, 1, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 5, 1, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 97, 130, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 6, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 17, 97, 130, 35, 3, 0, 2, 1, 0, 0, 0, (0, 3, 2, 2, 2, 1, 6, 0, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 65, 19, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 65, 19, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 0, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 65, 19, 35, 3, 0, 1, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 65, 19, 35, 3, 0, 1, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 4, 1, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 65, 130, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 5, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 65, 130, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 1, 4, 1, 5, 0, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 97, 11, 103, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 97, 11, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 0, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 97, 11, 103, 3, 0, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 97, 11, 35, 3, 0, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 4, 1, 1, 0, 0), ''),
    ('pad0', 1, 2, 21, 1345, 19, 103, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 5, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 1345, 19, 103, 3, 0, 1, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 5, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 97, 130, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 6, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 17, 97, 130, 35, 3, 0, 2, 1, 0, 0, 0, (1, 3, 2, 2, 2, 1, 6, 0, 1, 0, 0), ''),
    ('pad0', 0, 2, 21, 97, 5, 45, 3, 0, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 97, 5, 45, 3, 0, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 2305, 16, 57, 3, 0, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 3, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 2305, 16, 57, 3, 0, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 3, 1, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 2305, 35, 37, 3, 0, 2, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 0, 2, 21, 2305, 35, 37, 3, 0, 1, 1, 0, 0, 0, (0, 3, 3, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 97, 5, 45, 3, 0, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 97, 5, 45, 3, 0, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 2305, 16, 57, 3, 0, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 3, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 2305, 16, 57, 3, 0, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 3, 1, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 2305, 35, 37, 3, 0, 2, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 4, 0, 0, 0, 0), ''),
    ('pad0', 1, 2, 21, 2305, 35, 37, 3, 0, 1, 1, 0, 0, 0, (1, 3, 3, 2, 2, 1, 4, 1, 0, 0, 0), ''),
    ('padalt', 0, 2, 21, 65, 11, 36, 3, 0, 3, 1, 0, 4, 0, (0, 3, 5, 2, 4, 1, 4, 1, 0, 0, 0), ''),
    ('padalt', 1, 2, 21, 65, 11, 36, 3, 0, 4, 1, 0, 4, 0, (1, 3, 5, 2, 4, 1, 4, 0, 0, 0, 0), ''),
    ('ksplit', 0, 2, 117, 97, 3, 24, 3, 2, 2, 1, 1, 0, 2, (0, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('ksplit', 0, 2, 245, 97, 3, 24, 3, 2, 2, 1, 1, 0, 4, (0, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('ksplit', 0, 2, 117, 97, 3, 24, 3, 2, 1, 1, 1, 0, 2, (0, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('ksplit', 0, 2, 245, 97, 3, 24, 3, 2, 1, 1, 1, 0, 4, (0, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('ksplit', 1, 2, 117, 97, 3, 24, 3, 2, 2, 1, 1, 0, 2, (1, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('ksplit', 1, 2, 245, 97, 3, 24, 3, 2, 2, 1, 1, 0, 4, (1, 3, 3, 2, 2, 1, 2, 0, 0, 0, 0), ''),
    ('ksplit', 1, 2, 117, 97, 3, 24, 3, 2, 1, 1, 1, 0, 2, (1, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('ksplit', 1, 2, 245, 97, 3, 24, 3, 2, 1, 1, 1, 0, 4, (1, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('ksplit', 0, 2, 261, 257, 6, 43, 1, 0, 2, 1, 1, 0, 2, (0, 1, 4, 2, 4, 2, 2, 0, 0, 2, 1), ''),
    ('ksplit', 0, 2, 517, 257, 6, 43, 1, 0, 2, 1, 1, 0, 4, (0, 1, 4, 2, 4, 2, 2, 0, 0, 2, 1), ''),
    ('ksplit', 0, 2, 261, 257, 6, 43, 1, 0, 1, 1, 1, 0, 2, (0, 1, 4, 2, 4, 2, 2, 1, 0, 2, 1), ''),
    ('ksplit', 0, 2, 517, 257, 6, 43, 1, 0, 1, 1, 1, 0, 4, (0, 1, 4, 2, 4, 2, 2, 1, 0, 2, 1), ''),
    ('torgb', 0, 2, 17, 3, 34, 34, 1, 0, 0, 1, 0, 0, 0, (0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), ''),
    ('torgb', 1, 2, 17, 3, 34, 34, 1, 0, 0, 1, 0, 0, 0, (1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), ''),
    ('nodemod', 0, 2, 17, 129, 17, 33, 1, 0, 0, 0, 0, 0, 0, (0, 1, 0, 1, 4, 1, 4, 0, 0, 0, 0), ''),
    ('nodemod', 0, 2, 17, 3, 33, 33, 1, 0, 0, 0, 0, 0, 0, (0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0), ''),
    ('nodemod', 0, 2, 21, 65, 15, 31, 3, 2, 1, 0, 0, 0, 0, (0, 3, 2, 1, 4, 1, 4, 1, 0, 0, 0), ''),
    ('nodemod', 0, 2, 21, 97, 1, 41, 3, 2, 1, 0, 0, 0, 0, (0, 3, 3, 2, 2, 1, 2, 1, 0, 0, 0), ''),
    ('nodemod', 0, 2, 33, 65, 2, 129, 1, 0, 1, 0, 0, 0, 0, (0, 1, 4, 1, 8, 2, 1, 1, 0, 1, 0), ''),
    ('nodemod', 0, 2, 21, 65, 7, 32, 3, 2, 3, 0, 0, 4, 0, (0, 3, 5, 2, 4, 1, 4, 1, 0, 0, 0), ''),
]
# fmt: on


def _row(r):
    e = dict(zip(COLUMNS, r))
    assert len(r) == len(COLUMNS), r
    e['outRowStride'] = 0
    e['bias'] = 0
    e['dcoef'] = int(bool(e['demodulate']) or e['precision'] != CONV_FP32)      # the split / fp16 forms carry their power of two in dcoef
    v = e['variant']
    e['id'] = '%s-%s-%s-k%d-%d%d%d%d-s%dp%db%dm%d' % ((e['kind'], ('f32', 'f16')[e['dtype']], FAMILY_NAMES[v[2]], v[1]) + tuple(v[3:])) \
        + ('-ks%d' % e['kSplits'] if e['kind'] == 'ksplit' else '') + ('-pad%d' % e['pad'] if e['kind'] in ('pad0', 'padalt') else '') \
        + ('-hw%d' % (e['H'] * e['W'] % 4) if v[2] == TORGB else '')
    return e


ENTRIES = [_row(r) for r in TABLE]


def out_hw(e):
    return e['H'] + 2 * e['pad'] - e['k'] + 1, e['W'] + 2 * e['pad'] - e['k'] + 1


def macs(e):
    oh, ow = out_hw(e)
    return e['N'] * e['I'] * e['O'] * oh * ow * e['k'] ** 2


def variant_of(e, plan):
    """The coordinates a dispatch plan files call `e` under."""
    return (e['dtype'], e['k']) + tuple(plan[n] for n in ('family', 'WM', 'WN', 'TM', 'TN', 'SPLIT', 'PACK', 'NBUF', 'M16'))


def tile(variant):
    """(output channels, rows per workgroup or None, flat pixel run or None, channels per K step) of a variant's workgroup tile."""
    _, k, fam, wm, wn, tm, tn, _, _, _, _ = variant
    if fam == FP32_MFMA:
        return wm * tm * 32, wn * tn, None, 8 if k == 3 else 16
    if fam == TORGB:
        return None, None, None, 16
    if fam == ROWS:
        return wm * 32, wn * tn, None, 16
    if fam == FLAT:
        return 64, None, 64 * tn, 16
    if fam == GEMM1:
        return wm * tm * 32, None, wn * tn * 32, 32
    return 64, 2 * tn, None, 16                           # F23: two row groups of TN rows


def ragged_violations(e):
    """The RAGGED rules of the module docstring that call `e` breaks (empty: ragged)."""
    bm, rows, run, kc = tile(e['variant'])
    oh, ow = out_hw(e)
    bad = []
    if e['variant'][2] == TORGB:
        return (['O'] if e['O'] != 3 else []) + (['I'] if e['I'] % 16 == 0 else [])
    if e['O'] % bm == 0:
        bad.append('O')
    if run is not None:
        if oh * ow % run == 0:
            bad.append('plane')
    else:
        if ow % 32 == 0:
            bad.append('outW')
        if oh % rows == 0:
            bad.append('outH')
    if e['variant'][8]:                                   # PACK: the plan grants it for I % 16 in 1 .. 4 only
        if not 1 <= e['I'] % 16 <= 4:
            bad.append('I')
    elif e['I'] % (32 if e['variant'][2] == GEMM1 else 16) == 0:
        bad.append('I')
    return bad


def spanning_violations(e):
    """The SPANNING rules call `e` breaks (empty: a full and a ragged tile along every tiled dimension)."""
    bm, rows, run, kc = tile(e['variant'])
    oh, ow = out_hw(e)
    if e['variant'][2] == TORGB:
        return ['plane'] if e['H'] * e['W'] <= 1024 else []            # more than one workgroup of 256 threads x 4 pixels
    bad = []
    if e['O'] <= bm:
        bad.append('O')
    if run is not None:
        if oh * ow <= run:
            bad.append('plane')
    else:
        if ow <= 32:
            bad.append('outW')
        if oh <= rows:
            bad.append('outH')
    if e['I'] <= kc:
        bad.append('I')
    return bad


def crossed(variant):
    """A ROWS / FLAT / GEMM1 kernel whose tensor type and arithmetic no call of the Python op combines (_choose_form gives fp32
    tensors SPLIT = 1 and fp16 tensors SPLIT = 0): reachable through the C ABI alone."""
    return variant[2] in (ROWS, FLAT, GEMM1) and variant[0] == variant[7]


def sibling(e):
    """The same call on the other tensor type: the plan files it under the same template coordinates."""
    s = dict(e, dtype=1 - e['dtype'], variant=(1 - e['variant'][0],) + tuple(e['variant'][1:]))
    return s
