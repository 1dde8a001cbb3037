// Test-only probe of the GEMM launchers (tests/test_gemm_instances.py): one flat C entry that fills a mocha::GemmParams from a plain struct
// and calls launch_gemm / launch_gemm_x3 / launch_gemm_h2 / launch_gemm_x3r of libmocha_hip.so directly, so that a test can put ANY
// gather / epilogue / tile configuration on any instance - the library's own C entry (mocha_linear) only builds plain rows + bias.
// Links against libmocha_hip.so (its mocha::launch_* symbols are exported); no product source is involved.
#include "../../mocha_sigasia2023_amd/csrc/kernels.h"

#include <algorithm>

extern "C" {

// mirrors every GemmParams field a kernel or a selection rule reads; the packed weight images, the weight scales and (unless a_amax is
// given) the activation bounds are made here, as mocha_linear does
struct probe_params {
    const float* A; const float* W; const float* wsub; float* C;
    const float* bias; const float* rowbias; const float* residual;
    const float* a_amax; float* c_amax;            // engine 3: a_amax null = measured here per window (launch_absmax)
    long long slab_stride;
    int M, N, K, lda, ldc, ldr, rb_mod, act, a_lrelu, gather;
    int T_out, V, ntaps, pad, stride, R, T_full, tshift, Cc, T_src, tstep;
    float ascale;
    int ksplit, persistent, persistent_max_n, tile64_below, rows_per_win;
    int x3r_grid;                                   // engine 4: workgroups (0 = the launcher's default)
};

enum { PROBE_UNSUPPORTED = -1, PROBE_BAD_ARGUMENT = -2 };

}  // extern "C"

static mocha::GemmParams to_params(const probe_params& q) {
    mocha::GemmParams p;
    p.A = q.A; p.W = q.W; p.wsub = q.wsub; p.C = q.C; p.bias = q.bias; p.rowbias = q.rowbias; p.residual = q.residual;
    p.M = q.M; p.N = q.N; p.K = q.K; p.lda = q.lda; p.ldc = q.ldc; p.ldr = q.ldr; p.rb_mod = q.rb_mod; p.act = q.act; p.a_lrelu = q.a_lrelu;
    p.gather = q.gather; p.T_out = q.T_out; p.V = q.V; p.ntaps = q.ntaps; p.pad = q.pad; p.stride = q.stride; p.R = q.R; p.T_full = q.T_full;
    p.tshift = q.tshift; p.Cc = q.Cc; p.T_src = q.T_src; p.tstep = q.tstep; p.ascale = q.ascale;
    p.ksplit = q.ksplit; p.slab_stride = q.slab_stride;
    p.persistent = q.persistent; p.persistent_max_n = q.persistent_max_n; p.tile64_below = q.tile64_below;
    p.a_amax = q.a_amax; p.c_amax = q.c_amax; p.rows_per_win = q.rows_per_win;
    return p;
}

static bool sane(const probe_params& q) {
    if (!q.A || !q.W || !q.C || q.M <= 0 || q.N <= 0 || q.K <= 0 || q.lda <= 0 || q.ldc < q.N || q.rb_mod <= 0 || q.ksplit < 1) return false;
    if (q.residual && q.ldr < q.N) return false;
    if (q.gather) {
        if (q.T_out <= 0 || q.V <= 0 || q.ntaps <= 0 || q.Cc <= 0 || q.T_src <= 0 || q.T_full <= 0 || q.R <= 0 || q.tshift < 0) return false;
        if (q.ntaps * q.Cc != q.K || q.lda < q.Cc || q.M % (q.T_out * q.V) != 0) return false;        // whole windows only
        // every reflected frame lies inside its window: one reflection at either end suffices and lands on a source frame
        const long long hi = (long long)(q.T_out - 1) * q.stride + (q.R - 1) + (long long)(q.ntaps - 1) * q.tstep - q.pad;
        if (q.stride < 0 || q.tstep < 0 || hi > 2ll * (q.T_full - 1) || q.pad > q.T_full - 1 || ((q.T_full - 1) >> q.tshift) >= q.T_src) return false;
    } else if (q.lda < q.K) return false;
    return true;
}

struct DevMem {
    void* p = nullptr;
    ~DevMem() { if (p) (void)hipFree(p); }
    hipError_t reserve(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 16)); }
};

extern "C" {

// out[7] = gemm_is_skinny16, gemm_is_skinny, gemm_is_small, gemm_is_narrow, gemm_x3_supports, gemm_h2_supports, gemm_x3r_supports (host code only)
int probe_select(const probe_params* q, int* out) {
    if (!q || !out) return PROBE_BAD_ARGUMENT;
    const mocha::GemmParams p = to_params(*q);
    out[0] = mocha::gemm_is_skinny16(p); out[1] = mocha::gemm_is_skinny(p); out[2] = mocha::gemm_is_small(p); out[3] = mocha::gemm_is_narrow(p);
    out[4] = mocha::gemm_x3_supports(p); out[5] = mocha::gemm_h2_supports(p); out[6] = mocha::gemm_x3r_supports(p);
    return 0;
}

// engine: 1 exact-f32 kernels (launch_gemm), 2 three bf16 planes (launch_gemm_x3), 3 two fp16 planes (launch_gemm_h2), 4 register-resident
// planes (launch_gemm_x3r).  Returns the hipError_t of the first failing call (0 = hipSuccess) after synchronising the stream,
// PROBE_UNSUPPORTED when the engine's *_supports() refuses the parameters, PROBE_BAD_ARGUMENT for parameters no launcher may see.
int probe_gemm(const probe_params* q, int engine, void* stream) {
    if (!q || engine < 1 || engine > 4 || !sane(*q)) return PROBE_BAD_ARGUMENT;
    hipStream_t s = (hipStream_t)stream;
    mocha::GemmParams p = to_params(*q);
    static bool init_done[5] = {false, false, false, false, false};
    hipError_t e = hipSuccess;
    if (!init_done[engine]) {
        e = engine == 1 ? mocha::gemm_init() : engine == 2 ? mocha::gemm_x3_init() : engine == 3 ? mocha::gemm_h2_init() : mocha::gemm_x3r_init();
        if (e != hipSuccess) return (int)e;
        init_done[engine] = true;
    }
    if (engine == 1) {
        e = mocha::launch_gemm(p, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        return (int)e;
    }
    DevMem img, aux;
    if (engine == 2 || engine == 4) {
        if (!(engine == 2 ? mocha::gemm_x3_supports(p) : mocha::gemm_x3r_supports(p))) return PROBE_UNSUPPORTED;
        e = img.reserve(mocha::gemm_x3_packed_elems(p.N, p.K) * sizeof(unsigned short));
        if (e == hipSuccess) e = mocha::launch_pack_x3(p.W, p.N, p.K, (unsigned short*)img.p, s);
        p.Wsplit = (const unsigned short*)img.p;
        if (e == hipSuccess) e = engine == 2 ? mocha::launch_gemm_x3(p, s) : mocha::launch_gemm_x3r(p, s, q->x3r_grid);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        else (void)hipStreamSynchronize(s);
        return (int)e;
    }
    // engine 3
    if (!mocha::gemm_h2_supports(p)) return PROBE_UNSUPPORTED;
    const int rpw = p.rows_per_win;
    const long long nwin = ((long long)p.M + rpw - 1) / rpw;
    const size_t n4 = ((size_t)p.N + 3) / 4 * 4;
    if (nwin > 65535) return PROBE_BAD_ARGUMENT;
    e = img.reserve(mocha::gemm_h2_packed_elems(p.N, p.K) * sizeof(unsigned short));
    if (e == hipSuccess) e = aux.reserve((n4 + (size_t)nwin) * sizeof(float));
    if (e != hipSuccess) return (int)e;
    float* w_inv = (float*)aux.p;
    float* amax = w_inv + n4;
    e = hipMemsetAsync(amax, 0, (size_t)nwin * sizeof(float), s);
    if (e == hipSuccess) e = mocha::launch_pack_h2(p.W, p.N, p.K, (unsigned short*)img.p, w_inv, s);
    if (e == hipSuccess && !p.a_amax) {
        // a window's bound = the largest magnitude of the source rows its output rows read (LeakyReLU on load does not raise it)
        if (p.gather) {
            if (rpw != p.T_out * p.V) { (void)hipStreamSynchronize(s); return PROBE_BAD_ARGUMENT; }      // a window of the launch = one (b) block of the gather
            e = mocha::launch_absmax(p.A, nwin, (long long)p.T_src * p.V * p.lda, amax, s);
        } else {
            const long long full = p.M / rpw;
            if (full > 0) e = mocha::launch_absmax(p.A, full, (long long)rpw * p.lda, amax, s);
            if (e == hipSuccess && full < nwin)
                e = mocha::launch_absmax(p.A + (size_t)full * rpw * p.lda, 1, (long long)(p.M - full * rpw - 1) * p.lda + p.K, amax + full, s);
        }
        p.a_amax = amax;
    }
    p.Wh2 = (const unsigned short*)img.p; p.w_inv = w_inv;
    if (e == hipSuccess) e = mocha::launch_gemm_h2(p, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    else (void)hipStreamSynchronize(s);
    return (int)e;
}

}  // extern "C"
