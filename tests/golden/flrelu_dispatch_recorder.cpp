// flrelu_dispatch_recorder.cpp -- reads calls (one per line: the CALL_COLUMNS of make_flrelu_dispatch.py) and prints, per call, the
// launches sg3_filtered_lrelu makes for it (see modconv_dispatch_recorder.h) and what the older host queries answer
// (sg3_filtered_lrelu_planes_per_wave, sg3_filtered_lrelu_stream_grid).  Tensors are placeholders: no pointer is followed.
// SG3_FLRELU_NOPACK is read once per process, so the calls of that knob come in a run of their own with the variable set.
#include "modconv_dispatch_recorder.h"
#include "../../include/sg3_ops.h"
#include <cstdarg>

namespace sg3 { void set_error(const char* fmt, ...) { va_list a; va_start(a, fmt); vfprintf(stderr, fmt, a); va_end(a); fputc('\n', stderr); } }

enum { KNOB_NONE = 0, KNOB_NOPACK = 1, KNOB_SLOWACT = 2, KNOB_UP4_WIDE = 3 };
enum { DENSE = 0, CHANNELS_LAST = 1, EVERY_SECOND_SAMPLE = 2 };

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : stdin;
    if (!f) return 2;
    int dtype, N, C, xH, xW, yH, yW, up, down, fuW, fuH, fdW, fdH, px0, py0, sH, sWb, sx, sy, flip, write, read, partials, mirror, layout, fdOdd, sNull, knob;
    float gain, slope, clamp;
    while (fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %f %f %f %d %d %d %d %d %d %d %d %d", &dtype, &N, &C, &xH, &xW, &yH, &yW,
                  &up, &down, &fuW, &fuH, &fdW, &fdH, &px0, &py0, &sH, &sWb, &sx, &sy, &gain, &slope, &clamp, &flip, &write, &read, &partials, &mirror,
                  &layout, &fdOdd, &sNull, &knob) == 31) {
        sg3_filtered_lrelu_params q = {};
        char* const dummy = reinterpret_cast<char*>(0x1000);            // 16-byte aligned placeholder
        q.x = dummy; q.y = dummy; q.b = dummy; q.fu = reinterpret_cast<float*>(dummy);
        q.fd = reinterpret_cast<float*>(dummy + (fdOdd ? 4 : 0));
        q.s = ((write || read) && !sNull) ? reinterpret_cast<uint8_t*>(dummy) : nullptr;
        q.dtype = dtype; q.N = N; q.C = C; q.xH = xH; q.xW = xW; q.yH = yH; q.yW = yW;
        const long long xs[2][4] = {{(long long)C * xH * xW, (long long)xH * xW, xW, 1}, {(long long)C * xH * xW, 1, (long long)xW * C, C}};
        const long long ys[2][4] = {{(long long)C * yH * yW, (long long)yH * yW, yW, 1}, {(long long)C * yH * yW, 1, (long long)yW * C, C}};
        for (int i = 0; i < 4; i++) { q.xStride[i] = xs[layout == CHANNELS_LAST][i]; q.yStride[i] = ys[layout == CHANNELS_LAST][i]; }
        if (layout == EVERY_SECOND_SAMPLE) q.xStride[0] *= 2;           // x[::2] of a batch twice as large: planes not dense over (n, c)
        q.bStride = 1;
        q.up = up; q.down = down; q.fuW = fuW; q.fuH = fuH; q.fdW = fdW; q.fdH = fdH; q.px0 = px0; q.py0 = py0;
        q.sH = sH; q.sWbytes = sWb; q.sx = sx; q.sy = sy;
        q.gain = gain; q.slope = slope; q.clamp = clamp; q.flip = flip; q.writeSigns = write; q.readSigns = read; q.fdMirror = mirror;
        if (partials) { q.ySumPartial = reinterpret_cast<float*>(dummy); q.yAbsMaxPartial = reinterpret_cast<float*>(dummy); }
        if (knob == KNOB_SLOWACT) setenv("SG3_FLRELU_SLOWACT", "1", 1); else unsetenv("SG3_FLRELU_SLOWACT");
        sg3_filtered_lrelu_force_up4_wide(knob == KNOB_UP4_WIDE);
        int g[5] = {0, 0, 0, 0, 0};
        const int ppw = sg3_filtered_lrelu_planes_per_wave(&q);
        const int ok = sg3_filtered_lrelu_stream_grid(&q, &g[0], &g[1], &g[2], &g[3], &g[4]);
        rec::log().clear();
        const int rc = sg3_filtered_lrelu(&q, nullptr);
        printf("{\"rc\":%d,\"ppw\":%d,\"grid\":[%d,%d,%d,%d,%d,%d],\"launches\":[%s]}\n", rc, ppw, ok, g[0], g[1], g[2], g[3], g[4], rec::log().c_str());
    }
    return 0;
}
