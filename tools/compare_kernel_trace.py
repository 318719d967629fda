"""Compares two rocprofv3 kernel traces (csv) launch by launch: the ordered sequences of (kernel name, grid, workgroup, LDS bytes)
of the kernels whose name contains --match must be equal.  Used to show that a change of the host side of an op launches exactly
what its parent commit launched:

    rocprofv3 --kernel-trace --output-format csv -d <dir A> -o t -- python -m pytest tests/test_gpu_ops.py tests/test_gpu_f23.py -q -k "modulated or modconv or f23"
    (the same at the other commit into <dir B>)
    python tools/compare_kernel_trace.py <dir A> <dir B> --match modconv
"""
import argparse
import collections
import csv
import glob
import os
import sys


def launches(path, match):
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, '**', '*kernel_trace.csv'), recursive=True))
    assert len(files) == 1, f'{path}: expected one kernel trace, found {files}'
    with open(files[0], newline='') as f:
        rows = list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    out = []
    for r in rows:
        if match in r['Kernel_Name']:
            out.append((r['Kernel_Name'], tuple(int(r['Grid_Size_' + a]) for a in 'XYZ'), tuple(int(r['Workgroup_Size_' + a]) for a in 'XYZ'),
                        int(r['LDS_Block_Size'])))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a'); ap.add_argument('b')
    ap.add_argument('--match', default='modconv')
    args = ap.parse_args()
    a, b = launches(args.a, args.match), launches(args.b, args.match)
    print(f'{len(a)} launches in A, {len(b)} in B ({args.match}), {len(set(x[0] for x in a))} distinct kernels in A')
    for name, n in sorted(collections.Counter(x[0].split('(')[0] for x in a).items()):
        print(f'{n:7d}  {name}')
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None and len(a) == len(b):
        print('EQUAL: the same kernels with the same grid, workgroup and LDS size, in the same order')
        return 0
    i = first if first is not None else min(len(a), len(b))
    print(f'DIFFERENT from launch {i}:\n  A: {a[i] if i < len(a) else None}\n  B: {b[i] if i < len(b) else None}')
    return 1


if __name__ == '__main__':
    sys.exit(main())
