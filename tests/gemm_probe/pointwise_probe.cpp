// Test-only probe of the norm / pointwise launchers (tests/test_pointwise_kernels.py, tests/pointwise_ref.py): flat C entries that call the
// mocha::launch_* functions of pointwise.hip (and launch_absmax of gemm_h2.hip) in libmocha_hip.so directly with caller-given device
// pointers, so that a test can put ANY shape the launchers' contracts allow on every kernel - the network only ever calls them with
// 90 tokens, 22 / 24 joints and whole windows.  Links against libmocha_hip.so as probe.cpp does; no product source is involved.
//
// Every entry first runs a sane() check of its own - PROBE_BAD_ARGUMENT for what no launcher checks and what would let a kernel touch
// memory the test did not describe (a missing pointer, a stride below the width, one of a pair of vectors, a phased final projection on
// anything but whole windows) - then the launcher, then synchronises the stream; it returns the first failing hipError_t (0 = hipSuccess).
// What a launcher itself must refuse (hipErrorInvalidValue) is passed through to it: those refusals are what the tests assert.
#include "../../mocha_sigasia2023_amd/csrc/kernels.h"

extern "C" {

enum { PROBE_UNSUPPORTED = -1, PROBE_BAD_ARGUMENT = -2 };

// launch_instnorm's arguments and every InormExtra field
struct pw_inorm {
    const float* x; float* out; float* mean_out; const float* gm; const float* gs; float* zn;
    const float* centre; float* zc; unsigned short* zc16; float* qstat;
    const float* table; const int32_t* row_idx; float* copy_out; unsigned short* kvimg; double* mean64;
    long long plane_stride, table_rows;
    int split_max, reverse, B, n;
};

}  // extern "C"

static int finish(hipError_t e, hipStream_t s) {
    const hipError_t es = hipStreamSynchronize(s);
    return (int)(e != hipSuccess ? e : es);
}

static bool sane(const pw_inorm& q) {
    if (q.B <= 0 || q.n <= 0 || q.n > 4096 || q.B > (1 << 20)) return false;
    if (!q.x && !q.row_idx) return false;                                   // the rows come from x or from the table
    if (q.zn && (!q.gm || !q.gs)) return false;                             // the z-score's vectors (no launcher check)
    if (q.plane_stride > 0 && q.plane_stride < (long long)q.B * q.n * 256) return false;      // plane 1 would overlap plane 0
    if (q.row_idx && q.table && q.table_rows < 1) return false;
    return true;
}

extern "C" {

int pw_instnorm(const pw_inorm* q, int use_extra, void* stream) {
    if (!q || !sane(*q)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    mocha::InormExtra ex;
    ex.centre = q->centre; ex.zc = q->zc; ex.zc16 = q->zc16; ex.plane_stride = q->plane_stride; ex.qstat = q->qstat;
    ex.table = q->table; ex.row_idx = q->row_idx; ex.table_rows = q->table_rows; ex.copy_out = q->copy_out;
    ex.kvimg = q->kvimg; ex.split_max = q->split_max; ex.mean64 = q->mean64; ex.reverse = q->reverse;
    return finish(mocha::launch_instnorm(q->x, q->out, q->mean_out, q->gm, q->gs, q->zn, q->B, q->n, s, use_extra ? &ex : nullptr), s);
}

int pw_adain(const float* x, const float* gb, int gb_stride, float* xad, float* qin, int B, int n, int closed, const int32_t* gb_idx,
             long long gb_rows, int split_max, int reverse, void* stream) {
    if (!x || !gb || !xad || !qin || B <= 0 || n <= 0 || n > 4096 || gb_stride <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_adain(x, gb, gb_stride, xad, qin, B, n, s, closed, gb_idx, gb_rows, split_max, reverse), s);
}

static bool sane_embed(const float* X, const float* W1, const float* b1, const float* AP, const float* out, int count, int V, int Cin,
                       const float* xmean, const float* xstd, int raw_root) {
    if (!X || !W1 || !b1 || !AP || !out || count <= 0 || V < 1 || Cin < 1 || V > 4096 || Cin > 4096) return false;
    if ((xmean == nullptr) != (xstd == nullptr) || raw_root < 0 || raw_root > 1) return false;
    return true;
}

int pw_embed_front(const float* X, const float* W1, const float* b1, const float* AP, float* out, int nframes, int V, int Cin,
                   const float* xmean, const float* xstd, int raw_root, int planes, int max_wgs, void* stream) {
    if (!sane_embed(X, W1, b1, AP, out, nframes, V, Cin, xmean, xstd, raw_root)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_embed_front(X, W1, b1, AP, out, nframes, V, Cin, xmean, xstd, raw_root, s, planes != 0, max_wgs), s);
}

int pw_embed_sums(const float* X, const float* W1, const float* b1, const float* AP, float* u, int nwin, int V, int Cin,
                  const float* xmean, const float* xstd, int raw_root, int max_wgs, int reverse, void* stream) {
    if (!sane_embed(X, W1, b1, AP, u, nwin, V, Cin, xmean, xstd, raw_root) || nwin > (1 << 20)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_embed_sums(X, W1, b1, AP, u, nwin, V, Cin, xmean, xstd, raw_root, s, max_wgs, reverse), s);
}

int pw_window_sums(const float* y, float* u, int rows, int channels, void* stream) {
    if (!y || !u || rows <= 0 || channels <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_window_sums(y, u, rows, channels, s), s);
}

int pw_body_front(const float* x, const float* A_b, float* out, int rows6, int reverse, void* stream) {
    if (!x || !A_b || !out || rows6 <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_body_front(x, A_b, out, rows6, s, reverse), s);
}

int pw_joint_expand(const float* g, const float* AU, float* out, int nframes15, int V, int reverse, void* stream) {
    if (!g || !AU || !out || nframes15 <= 0 || V < 1) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_joint_expand(g, AU, out, nframes15, V, s, reverse), s);
}

int pw_final_proj(const float* z, const float* W6, const float* b6, float* Y, int rows, int Cout, int V, const float* ymean,
                  const float* ystd, int phased, int reverse, void* stream) {
    if (!z || !W6 || !b6 || !Y || rows <= 0 || Cout < 1 || V < 1 || V > 4096) return PROBE_BAD_ARGUMENT;
    if ((ymean == nullptr) != (ystd == nullptr)) return PROBE_BAD_ARGUMENT;
    if (phased && rows % (60 * V) != 0) return PROBE_BAD_ARGUMENT;          // the phased row map is defined on whole windows of 60 frames
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_final_proj(z, W6, b6, Y, rows, Cout, V, ymean, ystd, s, phased, reverse), s);
}

int pw_linear_f64(const double* X, int ldx, int xcol, const double* W, const double* bias, double* y64, float* y32, int ldy, int M, int N,
                  int K, int L, int act, void* stream) {
    if (!X || !W || M <= 0 || N < 1 || K < 1 || L < 1 || xcol < 0) return PROBE_BAD_ARGUMENT;
    if ((long long)ldx < (long long)(L - 1) * xcol + K || (long long)ldy < (long long)L * N) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_linear_f64(X, ldx, xcol, W, bias, y64, y32, ldy, M, N, K, L, act, s), s);
}

int pw_rownorm2(const float* x, const float* sub, float* out, long long rows, int cols, int reverse, void* stream) {
    if (!x || !out || rows <= 0 || cols <= 0 || rows > (1ll << 30)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_rownorm2(x, sub, out, rows, cols, s, reverse), s);
}

int pw_sub_rows(const float* x, const float* sub, float* out, long long rows, int cols, void* stream) {
    if (!x || !sub || !out || rows <= 0 || cols <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_sub_rows(x, sub, out, rows, cols, s), s);
}

int pw_center_rows(const float* x, const float* centre, void* planes, int nplanes, float* out32, float* qstat, long long rows, int cols,
                   int reverse, void* stream) {
    if (!x || !centre || rows <= 0 || cols <= 0 || rows > (1ll << 30)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_center_rows(x, centre, planes, nplanes, out32, qstat, rows, cols, s, reverse), s);
}

long long pw_column_mean_scratch_doubles(int cols) { return cols > 0 ? (long long)mocha::column_mean_scratch_doubles(cols) : 0; }

int pw_column_mean(const float* x, long long N, int cols, float* mean, double* scratch, long long scratch_doubles, void* stream) {
    if (!x || !mean || !scratch || N <= 0 || cols <= 0) return PROBE_BAD_ARGUMENT;
    if (scratch_doubles < (long long)mocha::column_mean_scratch_doubles(cols)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_column_mean(x, N, cols, mean, scratch, s), s);
}

int pw_column_stats(const float* x, long long N, int cols, float* mean, float* sd, void* stream) {
    if (!x || !mean || N <= 0 || cols <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_column_stats(x, N, cols, mean, sd, s), s);
}

int pw_absmax(const float* x, long long nwin, long long per, float* out, float mul, float add, void* stream) {
    if (!x || !out || nwin <= 0 || per <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_absmax(x, nwin, per, out, s, mul, add), s);
}

}  // extern "C"
