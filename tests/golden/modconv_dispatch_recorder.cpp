// modconv_dispatch_recorder.cpp -- reads calls (one per line: dtype N I O H W k pad precision outRowStride dcoef bias scratch
// forcedRows) and prints, per call, the launches sg3_modulated_conv2d makes for it (see modconv_dispatch_recorder.h).
// `scratch` = 1 offers what sg3_modconv_split_scratch_floats asks for, as modulated_conv.py::_launch does.  No pointer is followed.
#include "modconv_dispatch_recorder.h"
#include "../../include/sg3_ops.h"
#include <cstdarg>

namespace sg3 { void set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vfprintf(stderr, fmt, a); va_end(a); fputc('\n', stderr); } }

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!f) return 2;
    int dtype, N, I, O, H, W, k, pad, prec, stride, dcoef, bias, scratch, rows;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &dtype, &N, &I, &O, &H, &W, &k, &pad, &prec, &stride, &dcoef, &bias, &scratch, &rows) == 14) {
        sg3_modconv_params q = {};
        float* const dummy = reinterpret_cast<float*>(0x1000);          // 16-byte aligned placeholder
        q.x = dummy; q.wPacked = dummy; q.sIn = dummy; q.out = dummy;
        q.dcoef = dcoef ? dummy : nullptr;
        q.epilogueBias = bias ? dummy : nullptr; q.epilogueClamp = 1.f; q.epilogueScale = 1.f;
        q.dtype = dtype; q.N = N; q.I = I; q.O = O; q.H = H; q.W = W; q.k = k; q.pad = pad; q.precision = prec; q.outRowStride = stride;
        long long need = 0;
        if (scratch) {
            need = sg3_modconv_split_scratch_floats(&q);
            if (need > 0) { q.splitScratch = dummy; q.splitScratchFloats = need; }
        }
        sg3_modconv_f23_force_rows(rows);
        rec::log().clear();
        const int rc = sg3_modulated_conv2d(&q, nullptr);
        printf("{\"call\":[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d],\"need\":%lld,\"rc\":%d,\"launches\":[%s]}\n",
               dtype, N, I, O, H, W, k, pad, prec, stride, dcoef, bias, scratch, rows, need, rc, rec::log().c_str());
    }
    return 0;
}
