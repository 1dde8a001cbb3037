// Test-only probe of the few-query scans and of the segmented matchers (tests/test_scan_kernels.py, tests/scan_ref.py): flat C entries that
// call the mocha::launch_* functions of match_stream.hip, match_scan8.hip, match_segmented.hip, match_seg_topk.hip and the two gathers of
// pointwise.hip in libmocha_hip.so directly with caller-given device pointers, so that a test can AUTHOR what the API always derives itself
// (the coarse keys, the scan's minima, rho, the mode words, the segment table) and put any shape the launchers' contracts allow on every
// kernel.  Links against libmocha_hip.so as match_probe.cpp does; no product source is involved and no kernel is defined here.
//
// Every entry first runs a check of its own - PROBE_BAD_ARGUMENT for what the kernels rely on and no launcher checks (the contract comment
// above the few-query and segmented launchers in csrc/kernels.h; a refusal launches nothing) - then, once per process,
// mocha::match_refine_init() and mocha::match_scan8_init() (dynamic LDS of the refine and of the adaptive scan; the library does it in
// mocha_create, which a probe never goes through), then the launcher, then synchronises the stream; it returns the first failing
// hipError_t (0 = hipSuccess).  What a launcher itself must refuse (hipErrorInvalidValue: D off the chunk, k out of range, a temperature
// that is not positive, out without enc, too many queries) is passed through to it.  Buffer sizes are what the CALLER says its buffers
// hold, in the units of the size helpers; a buffer smaller than the helper's figure is refused.
#include "../../mocha_sigasia2023_amd/csrc/kernels.h"

#include <vector>

extern "C" {
enum { PROBE_UNSUPPORTED = -1, PROBE_BAD_ARGUMENT = -2 };
}

static bool al(const void* p, unsigned a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static bool opt(const void* p, unsigned a) { return !p || ((uintptr_t)p & (a - 1)) == 0; }
static const long long MAX_N = 0x7ffffff0ll;

static int finish(hipError_t e, hipStream_t s) {
    const hipError_t es = hipStreamSynchronize(s);
    return (int)(e != hipSuccess ? e : es);
}

static hipError_t init_once() {
    static const hipError_t e = [] {
        const hipError_t a = mocha::match_refine_init();
        return a != hipSuccess ? a : mocha::match_scan8_init();
    }();
    return e;
}

// the arrival tickets of the refine (8 words behind the 8 x 64 slice winners of the scratch head) must be zero when a launch starts
static bool tickets_zero(const unsigned long long* scratch) {
    const size_t first = mocha::match_scan8_mode_word() - 8;
    unsigned long long h[8];
    if (hipMemcpy(h, scratch + first, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int i = 0; i < 8; ++i)
        if (h[i]) return false;
    return true;
}

// the few-query scans' operands: bank and queries on the 16-byte grid of their loads, a row count the 32-bit row of a key can hold
static bool sane_scan(const void* bank, const float* query, int Q, long long N, int D, const int32_t* idx) {
    return al(bank, 16) && al(query, 16) && al(idx, 4) && Q >= 1 && N >= 1 && N <= MAX_N && D > 0;
}

// the segment table: S + 1 device ints, non-decreasing from 0, NO EMPTY SEGMENT, the last one the bank's row count at most, the largest
// segment max_rows at most
static bool sane_segments(const int* seg_start, int S, long long max_rows, long long bank_rows) {
    if (!al(seg_start, 4) || S < 1 || S > (1 << 24) || max_rows < 1 || bank_rows < 1) return false;
    std::vector<int> h((size_t)S + 1);
    if (hipMemcpy(h.data(), seg_start, h.size() * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (h[0] != 0 || h[S] > bank_rows) return false;
    for (int s = 0; s < S; ++s) {
        const long long n = (long long)h[s + 1] - h[s];
        if (n < 1 || n > max_rows) return false;
    }
    return true;
}

extern "C" {

// ---- size helpers and constants
long long sp_stream_scratch(int Q, long long N) { return (long long)mocha::match_stream_scratch(Q, N); }
long long sp_scan16_scratch_words(long long N) { return (long long)mocha::match_scan16_scratch_words(N); }
long long sp_scan16_head_words() { return (long long)mocha::match_scan16_scratch_head_words(); }
long long sp_scan8_mode_word() { return (long long)mocha::match_scan8_mode_word(); }
long long sp_seg_scratch_words(int Q, long long max_rows) { return (long long)mocha::match_seg_scratch_words(Q, max_rows); }
long long sp_seg_plan_ints(int Q, int S) { return (long long)mocha::seg_plan_ints(Q, S); }
long long sp_seg_keys_words(long long max_rows) { return (long long)mocha::match_seg_keys_words(max_rows); }
int sp_seg_max_q() { return mocha::SEG_MAX_Q; }
int sp_seg_topk_q() { return mocha::SEG_TOPK_Q; }
int sp_seg_topk_max_k() { return mocha::SEG_TOPK_MAX_K; }

// ---- the streaming scan and its k-pass selection
int sp_match_stream(const void* bank, int bank_bf16, const float* query, int Q, long long N, int D, unsigned long long* partial,
                    long long partial_words, int32_t* idx, float* dist, void* stream) {
    if (!sane_scan(bank, query, Q, N, D, idx) || !al(partial, 8) || !opt(dist, 4) || partial_words < (long long)mocha::match_stream_scratch(Q, N))
        return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_stream(bank, bank_bf16, query, Q, N, D, partial, idx, dist, s), s);
}

int sp_match_topk(const void* bank, int bank_bf16, const float* query, int Q, long long N, int D, int k, unsigned long long* keys,
                  long long keys_words, int32_t* idx, float* dist, void* stream) {
    if (!sane_scan(bank, query, Q, N, D, idx) || !al(keys, 8) || !opt(dist, 4) || keys_words < 8 * N || k > (1 << 20)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_topk(bank, bank_bf16, query, Q, N, D, k, keys, idx, dist, s), s);
}

// ---- the gathers (src rows and out on the 16-byte grid)
int sp_gather_blend(const float* src, const int32_t* idx, const float* dist, float temperature, float* out, int Q, int k, int cols,
                    long long nrows, void* stream) {
    if (!al(src, 16) || !al(out, 16) || !al(idx, 4) || !al(dist, 4) || Q < 1 || cols <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_gather_blend(src, idx, dist, temperature, out, Q, k, cols, nrows, s), s);
}

int sp_gather_rows(const float* src, const int32_t* idx, float* out, int Q, int cols, long long nrows, void* stream) {
    if (!al(src, 16) || !al(out, 16) || !al(idx, 4) || Q < 1 || cols <= 0) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_gather_rows(src, idx, out, Q, cols, nrows, s), s);
}

// ---- the bf16-copy scan with its exact re-rank, the re-rank alone, the byte stage
int sp_match_scan16(const void* bank16, const float* rho, const float* bank, const float* qc, const float* query, int Q, long long N, int D,
                    unsigned long long* scratch, long long scratch_words, int32_t* idx, float* dist, void* stream) {
    if (!sane_scan(bank16, qc, Q, N, D, idx) || !al(bank, 16) || !al(query, 16) || !al(rho, 4) || !al(scratch, 8) || !opt(dist, 4) ||
        scratch_words < (long long)mocha::match_scan16_scratch_words(N) || !tickets_zero(scratch))
        return PROBE_BAD_ARGUMENT;
    const hipError_t init = init_once();
    if (init != hipSuccess) return (int)init;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_scan16(bank16, rho, bank, qc, query, Q, N, D, scratch, idx, dist, s), s);
}

// keys [nq][N], wgmin [nq][nwg], rho16 (and rho8) [N], mode 2 words or null, scratch: the head alone is enough
int sp_match_refine(const unsigned long long* keys, const unsigned long long* wgmin, int nwg, const float* rho16, const float* rho8, unsigned* mode,
                    const float* bank, const float* query, int nq, long long N, int D, int32_t* idx, float* dist, unsigned long long* scratch,
                    long long scratch_words, void* stream) {
    if (!al(keys, 8) || !al(wgmin, 8) || nwg < 1 || !al(rho16, 4) || !opt(rho8, 4) || !opt(mode, 4) || !al(bank, 16) || !al(query, 16) ||
        nq < 1 || nq > 8 || N < 1 || N > MAX_N || D < 256 || D % 256 || D > 23040 || !al(idx, 4) || !opt(dist, 4) || !al(scratch, 8) ||
        scratch_words < (long long)mocha::match_scan16_scratch_head_words() || !tickets_zero(scratch))
        return PROBE_BAD_ARGUMENT;
    const hipError_t init = init_once();
    if (init != hipSuccess) return (int)init;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_refine(keys, wgmin, nwg, rho16, rho8, mode, bank, query, nq, N, D, idx, dist, scratch, s), s);
}

int sp_match_scan8(const void* bank8, const float* scale8, const float* rho8, const void* bank16, const float* rho16, const float* bank,
                   const float* qc, const float* query, int Q, long long N, int D, unsigned long long* scratch, long long scratch_words,
                   int32_t* idx, float* dist, void* stream) {
    if (!sane_scan(bank8, qc, Q, N, D, idx) || !al(scale8, 4) || !al(rho8, 4) || !al(bank16, 16) || !al(rho16, 4) || !al(bank, 16) ||
        !al(query, 16) || !al(scratch, 8) || !opt(dist, 4) || scratch_words < (long long)mocha::match_scan16_scratch_words(N) || !tickets_zero(scratch))
        return PROBE_BAD_ARGUMENT;
    const hipError_t init = init_once();
    if (init != hipSuccess) return (int)init;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_scan8(bank8, scale8, rho8, bank16, rho16, bank, qc, query, Q, N, D, scratch, idx, dist, s), s);
}

// ---- the segmented matchers (bank_rows: rows the caller's bank - and enc - hold)
int sp_seg_plan(const int32_t* seg, int Q, int S, int* plan, long long plan_ints, void* stream) {
    if (!al(seg, 4) || !al(plan, 4) || (Q >= 1 && Q <= mocha::SEG_MAX_Q && S >= 1 && plan_ints < (long long)mocha::seg_plan_ints(Q, S)))
        return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_seg_plan(seg, Q, S, plan, s), s);
}

int sp_match_segmented(const void* bank, int bank_bf16, long long bank_rows, const float* query, const int32_t* seg, int Q, const int* seg_start,
                       int S, long long max_rows, int D, unsigned long long* partial, long long partial_words, int* plan, long long plan_ints,
                       int32_t* idx, int32_t* gidx, float* dist, void* stream) {
    if (!al(bank, 16) || !al(query, 16) || !al(seg, 4) || Q < 1 || D <= 0 || !al(partial, 8) || !al(plan, 4) || !opt(idx, 4) || !opt(gidx, 4) ||
        !opt(dist, 4))
        return PROBE_BAD_ARGUMENT;
    if (Q <= mocha::SEG_MAX_Q) {      // (more queries than that: the launcher's own refusal, whatever the table)
        if (!sane_segments(seg_start, S, max_rows, bank_rows) || partial_words < (long long)mocha::match_seg_scratch_words(Q, max_rows) ||
            plan_ints < (long long)mocha::seg_plan_ints(Q, S))
            return PROBE_BAD_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_segmented(bank, bank_bf16, query, seg, Q, seg_start, S, max_rows, D, partial, plan, idx, gidx, dist, s), s);
}

int sp_match_seg_topk(const void* bank, int bank_bf16, long long bank_rows, const float* query, const int32_t* seg, int Q, const int* seg_start,
                      int S, long long max_rows, int D, unsigned long long* keys, long long keys_words, int* plan, long long plan_ints,
                      const float* enc, int k, float temperature, int32_t* idx0, int32_t* idx_k, float* dist_k, float* w_k, float* out,
                      void* stream) {
    if (!al(bank, 16) || !al(query, 16) || !al(seg, 4) || Q < 1 || D <= 0 || !al(keys, 8) || !al(plan, 4) || !opt(enc, 16) || !opt(idx0, 4) ||
        !opt(idx_k, 4) || !opt(dist_k, 4) || !opt(w_k, 4) || !opt(out, 16))
        return PROBE_BAD_ARGUMENT;
    if (!sane_segments(seg_start, S, max_rows, bank_rows) || keys_words < (long long)mocha::match_seg_keys_words(max_rows) ||
        plan_ints < (long long)mocha::seg_plan_ints(mocha::SEG_TOPK_Q, S))
        return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    return finish(mocha::launch_match_seg_topk(bank, bank_bf16, query, seg, Q, seg_start, S, max_rows, D, keys, plan, enc, k, temperature, idx0, idx_k,
                                               dist_k, w_k, out, s), s);
}

}  // extern "C"
