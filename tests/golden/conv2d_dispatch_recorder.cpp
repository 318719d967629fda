// conv2d_dispatch_recorder.cpp -- reads calls (one per line: entry N I O H W k stride pad precision; the CALL_COLUMNS of
// make_conv2d_dispatch.py) and prints, per call, the launches sg3_conv2d (entry 0), sg3_conv2d_dgrad (1) or sg3_conv2d_wgrad_sum (2)
// makes for it (see modconv_dispatch_recorder.h) and what the older host queries answer (sg3_conv2d_form,
// sg3_conv2d_wgrad_sum_splits).  Tensors are placeholders: no pointer is followed.  The CU count is read once per process (REC_CUS).
#include "modconv_dispatch_recorder.h"
#include "../../include/sg3_ops.h"
#include <cstdarg>

namespace sg3 { void set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vfprintf(stderr, fmt, a); va_end(a); fputc('\n', stderr); } }

enum { FORWARD = 0, DGRAD = 1, WGRAD_SUM = 2 };

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!f) return 2;
    int entry, N, I, O, H, W, k, stride, pad, prec;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &entry, &N, &I, &O, &H, &W, &k, &stride, &pad, &prec) == 10) {
        float* const dummy = reinterpret_cast<float*>(0x1000);          // 16-byte aligned placeholder
        int rc = 0, form = 0, splitsRc = 0, s[3] = {0, 0, 0};
        rec::log().clear();
        if (entry == FORWARD) {
            sg3_conv2d_params q = {};
            q.x = dummy; q.wPacked = dummy; q.out = dummy; q.wScale = dummy; q.rangeFlag = reinterpret_cast<int32_t*>(dummy);
            q.N = N; q.I = I; q.O = O; q.H = H; q.W = W; q.k = k; q.stride = stride; q.pad = pad; q.precision = prec;
            form = sg3_conv2d_form(&q);
            rc = sg3_conv2d(&q, nullptr);
        } else if (entry == DGRAD) {
            sg3_conv2d_dgrad_params q = {};
            q.dy = dummy; q.wPacked = dummy; q.dx = dummy;
            q.N = N; q.I = I; q.O = O; q.H = H; q.W = W; q.k = k; q.stride = stride;
            q.OH = (H + 2 * (k / 2) - k) / stride + 1; q.OW = (W + 2 * (k / 2) - k) / stride + 1;
            rc = sg3_conv2d_dgrad(&q, nullptr);
        } else {
            sg3_conv2d_wgrad_sum_params q = {};
            q.x = dummy; q.dy = dummy; q.dw = dummy; q.partial = dummy;
            q.N = N; q.I = I; q.O = O; q.H = H; q.W = W; q.k = k; q.stride = stride;
            splitsRc = sg3_conv2d_wgrad_sum_splits(N, I, O, H, W, k, stride, &s[0], &s[1], &s[2]);
            rc = sg3_conv2d_wgrad_sum(&q, nullptr);
        }
        printf("{\"rc\":%d,\"form\":%d,\"splits\":[%d,%d,%d,%d],\"launches\":[%s]}\n", rc, form, splitsRc, s[0], s[1], s[2], rec::log().c_str());
    }
    return 0;
}
