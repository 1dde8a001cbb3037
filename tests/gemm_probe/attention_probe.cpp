// Test-only probe of the attention launchers (tests/test_attention_kernels.py, tests/attention_ref.py): flat C entries that call
// mocha::launch_attention, launch_attention_x3 and launch_attention_x3_kv in libmocha_hip.so directly with caller-given device pointers,
// so that a test can put ANY shape, stride and head layout the launchers' contracts allow on every kernel instance - the network only
// ever calls them with 90 x 90 tokens (182 x 182, 90 x 181 in the CVAE) and whole batches.  Links against libmocha_hip.so as probe.cpp
// does; no product source is involved and no kernel is defined here.
//
// Every entry first runs a sane() check of its own - PROBE_BAD_ARGUMENT for what no launcher checks and what would let a kernel touch
// memory the test did not describe (a missing pointer, a head count below one, a stride below the width or off the 16-byte grid of the
// kernels' buffer loads, an index vector without a table size, a scale the max subtraction does not cover) - then, once per process,
// mocha::attention_x3_init() (the twelve-wave variant's dynamic LDS; the library does it in mocha_create, which a probe never goes
// through), then the launcher, then synchronises the stream; it returns the first failing hipError_t (0 = hipSuccess).
// What a launcher itself must refuse (hipErrorInvalidValue: token counts, head dims, the kv kernel's head counts) is passed through to
// it: those refusals are what the tests assert.
#include <cmath>
#include "../../mocha_sigasia2023_amd/csrc/kernels.h"

extern "C" {

enum { PROBE_UNSUPPORTED = -1, PROBE_BAD_ARGUMENT = -2 };
enum { AT_F32 = 0, AT_X3 = 1, AT_KV = 2 };

// AttnParams and AttnKvParams in one plain struct (kv: the image of launch_attention_x3_kv; k, v, kv_idx, hs*, split_max, reverse unused there)
struct at_params {
    const float* q; const float* k; const float* v; float* out;
    const int32_t* kv_idx; const unsigned short* kv;
    long long kv_rows;
    int ldq, ldk, ldv, ldo;
    int B, heads, dh, nq, nk;
    int hsk, hsv, split_max, reverse, pairs;
    float scale;
};

}  // extern "C"

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static bool stride_ok(int ld) { return ld > 0 && ld % 4 == 0 && ld <= (1 << 20); }

static bool sane(const at_params& a, int which) {
    if (which != AT_F32 && which != AT_X3 && which != AT_KV) return false;
    if (!a.q || !a.out || !aligned16(a.q) || !aligned16(a.out)) return false;
    if (a.B > (1 << 20) || a.heads > 64) return false;
    if (!(std::isfinite(a.scale) && a.scale > 0.f)) return false;
    if (!stride_ok(a.ldq) || !stride_ok(a.ldo)) return false;
    const long long width = (long long)(a.heads > 0 ? a.heads : 0) * (a.dh > 0 ? a.dh : 0);
    if (a.ldq < width || a.ldo < width) return false;
    if (which == AT_KV) return a.kv && aligned16(a.kv);      // the head count is the launcher's to refuse (even, >= 2)
    if (a.heads < 1) return false;                           // no launcher check: a grid of 0 workgroups, a division by 0
    if (!a.k || !a.v || !aligned16(a.k) || !aligned16(a.v) || !stride_ok(a.ldk) || !stride_ok(a.ldv)) return false;
    const long long hk = a.hsk < 0 ? a.dh : a.hsk, hv = a.hsv < 0 ? a.dh : a.hsv;      // as the kernels resolve them
    if (hk % 4 || hv % 4) return false;                      // a head's columns start on the 16-byte grid
    if (a.ldk < (a.heads - 1) * hk + a.dh || a.ldv < (a.heads - 1) * hv + a.dh) return false;
    if (a.kv_idx && a.kv_rows < 1) return false;
    return true;
}

static int finish(hipError_t e, hipStream_t s) {
    const hipError_t es = hipStreamSynchronize(s);
    return (int)(e != hipSuccess ? e : es);
}

extern "C" {

int at_kv_img_bytes() { return mocha::ATTN_KV_IMG_BYTES; }

// sane() alone (host code, no GPU): 0 or PROBE_BAD_ARGUMENT
int at_sane(const at_params* a, int which) { return a && sane(*a, which) ? 0 : PROBE_BAD_ARGUMENT; }

int at_attention(const at_params* a, int which, void* stream) {
    if (!a || !sane(*a, which)) return PROBE_BAD_ARGUMENT;
    static const hipError_t init = mocha::attention_x3_init();
    if (init != hipSuccess) return (int)init;
    hipStream_t s = (hipStream_t)stream;
    if (which == AT_KV) {
        mocha::AttnKvParams p{};
        p.q = a->q; p.out = a->out; p.kv = a->kv; p.ldq = a->ldq; p.ldo = a->ldo;
        p.B = a->B; p.heads = a->heads; p.dh = a->dh; p.nq = a->nq; p.nk = a->nk; p.scale = a->scale; p.pairs = a->pairs;
        return finish(mocha::launch_attention_x3_kv(p, s), s);
    }
    mocha::AttnParams p{};
    p.q = a->q; p.k = a->k; p.v = a->v; p.out = a->out;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.B = a->B; p.heads = a->heads; p.dh = a->dh; p.nq = a->nq; p.nk = a->nk; p.scale = a->scale;
    p.hsk = a->hsk; p.hsv = a->hsv; p.split_max = a->split_max;
    p.kv_idx = a->kv_idx; p.kv_rows = a->kv_rows; p.reverse = a->reverse;
    return finish(which == AT_F32 ? mocha::launch_attention(p, s) : mocha::launch_attention_x3(p, s), s);
}

}  // extern "C"
