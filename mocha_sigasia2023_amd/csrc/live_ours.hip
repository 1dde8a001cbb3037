// The CVAE ("Ours") branch inside the live step (mocha_live_step_ours; test_fullframework.py:290-298 for a stream's first frame,
// :446-457 after it): the per-stream autoregressive state lives in device memory and every decision of a frame is taken from device
// data, so that the whole step is one captured graph.
//
//  mocha_live_ours_condition   per stream a mode - 0 warming (the push left no effective character id), 1 seed (chain counter 0, or the
//                              character id differs from the one of the stream's last step), 2 chain - written into the counters, the
//                              sampler's condition rows for that mode, and the stream's noise row: copied from the caller (noise 1) or
//                              drawn here with Philox4x32-10 + Box-Muller (noise 2).
//  mocha_live_ours_update      after the sampler: the stream's character feature `prev` - the matched bank row (seed) or the de-normalised
//                              sample (chain) - and its counters.  A warming stream's state is not touched.
//
// The GROUPED instances (mocha_live_step_ours_grouped) serve one CVAE per CHARACTER from a weight bank: a stream's slot is
// cvae_of[eff[s]], its four statistics are the slot's (stats: (Cw, 4, 90, 256) = src_cnt mean / std, cha_encoded mean / std).  A stream
// whose character has no CVAE - cvae_of negative, >= Cw, or the slot not stored - is in mode 1 on EVERY valid frame: its condition rows
// are zeros, its character feature the matched bank row, seeded[s] = 1.  The condition kernel also writes slot[s], the `which` of the
// sampler's grouped launches: -1 for warming streams and for streams without a CVAE.
//
// Both are latency-bound at S <= 16 streams: one wave per 256-channel row, 16 bytes per lane, as mocha_cvae_latent.
#include "kernels.h"

namespace mocha {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int ours_mode(int chain, int last, int e, int nseg) {
    if (e < 0 || e >= nseg) return 0;
    return (chain == 0 || e != last) ? 1 : 2;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 24 random bits -> (0, 1]: ((x >> 8) + 0.5) 2^-24 in fp32 (round to nearest even: the top of the range gives exactly 1, never 0)
__device__ __forceinline__ float philox_u(uint32_t x) { return ((float)(x >> 8) + 0.5f) * 0x1p-24f; }

// rows per stream: 180 condition rows, then (noise != 0) the stream's noise row
template <bool GROUPED>
__global__ __launch_bounds__(256) void mocha_live_ours_condition(int32_t* __restrict__ counters, const int32_t* __restrict__ eff, int nseg,
                                                                 const float* __restrict__ cnt, const float* __restrict__ prev,
                                                                 const float* __restrict__ sm, const float* __restrict__ ss,
                                                                 const float* __restrict__ cm, const float* __restrict__ cs,
                                                                 float* __restrict__ cond, int noise, const float* __restrict__ eps_in,
                                                                 uint32_t key0, uint32_t key1, float* __restrict__ eps_out, int rps, int rows,
                                                                 OursGroup grp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), q = threadIdx.x & 63;
    if (row >= rows) return;
    const int s = row / rps, t = row - s * rps;
    const int chain = counters[s * 3], last = counters[s * 3 + 1];
    int mode = ours_mode(chain, last, eff[s], nseg);
    int slot = -1;
    if (GROUPED) {
        if (mode != 0) {                                        // (eff[s] is then inside the segment table)
            slot = grp.cvae_of[eff[s]];
            slot = (slot >= 0 && slot < grp.Cw && grp.stored[slot] != 0) ? slot : -1;
            if (slot < 0) mode = 1;                             // no CVAE: plain context matching on every valid frame
        }
        if (t == 0 && q == 0) grp.slot[s] = slot;
        if (slot >= 0) {
            const float* st = grp.stats + (size_t)slot * 4 * 90 * 256;
            sm = st; ss = st + 90 * 256; cm = st + 2 * 90 * 256; cs = st + 3 * 90 * 256;
        }
    }
    if (t == 0 && q == 0) counters[s * 3 + 2] = mode;
    if (t < 180) {
        const bool first = t < 90;
        const int tt = first ? t : t - 90;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if ((first ? mode != 0 : mode == 2) && (!GROUPED || slot >= 0)) {
            const f32x4 x = reinterpret_cast<const f32x4*>(first ? cnt : prev)[((size_t)s * 90 + tt) * 64 + q];
            const f32x4 m = reinterpret_cast<const f32x4*>(first ? sm : cm)[tt * 64 + q];
            const f32x4 sd = reinterpret_cast<const f32x4*>(first ? ss : cs)[tt * 64 + q];
            v = (x - m) / sd;
        }
        reinterpret_cast<f32x4*>(cond)[((size_t)s * 180 + t) * 64 + q] = v;
        return;
    }
    f32x4 e;
    if (noise == 1) {
        e = reinterpret_cast<const f32x4*>(eps_in)[(size_t)s * 64 + q];
    } else {
        // block q of the stream's frame: counter (q, chain counter, stream, 0) -> eps[4q .. 4q+3]
        uint32_t x[4];
        philox4x32_10((uint32_t)q, (uint32_t)chain, (uint32_t)s, 0u, key0, key1, x);
        const float two_pi = 6.283185307179586f;
        const float r0 = sqrtf(-2.f * logf(philox_u(x[0]))), a0 = two_pi * philox_u(x[1]);
        const float r1 = sqrtf(-2.f * logf(philox_u(x[2]))), a1 = two_pi * philox_u(x[3]);
        e[0] = r0 * cosf(a0); e[1] = r0 * sinf(a0);
        e[2] = r1 * cosf(a1); e[3] = r1 * sinf(a1);
    }
    reinterpret_cast<f32x4*>(eps_out)[(size_t)s * 64 + q] = e;
}

hipError_t launch_live_ours_condition(int32_t* counters, const int32_t* eff, int nseg, const float* cnt, const float* prev, const float* sm,
                                      const float* ss, const float* cm, const float* cs, float* cond, int noise, const float* eps_in,
                                      unsigned long long seed, float* eps_out, int S, hipStream_t s, const OursGroup* grp) {
    if (S <= 0) return hipSuccess;
    if (noise < 0 || noise > 2 || (noise == 1 && !eps_in) || (noise && !eps_out)) return hipErrorInvalidValue;
    if (grp && (!grp->cvae_of || !grp->stored || !grp->stats || !grp->slot || grp->Cw < 1)) return hipErrorInvalidValue;
    const int rps = 180 + (noise ? 1 : 0), rows = S * rps;
    if (grp)
        hipLaunchKernelGGL(mocha_live_ours_condition<true>, dim3((rows + 3) / 4), dim3(256), 0, s, counters, eff, nseg, cnt, prev, sm, ss, cm, cs,
                           cond, noise, eps_in, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), eps_out, rps, rows, *grp);
    else
        hipLaunchKernelGGL(mocha_live_ours_condition<false>, dim3((rows + 3) / 4), dim3(256), 0, s, counters, eff, nseg, cnt, prev, sm, ss, cm, cs,
                           cond, noise, eps_in, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), eps_out, rps, rows, OursGroup{});
    return hipGetLastError();
}

template <bool GROUPED>
__global__ __launch_bounds__(256) void mocha_live_ours_update(int32_t* __restrict__ counters, const int32_t* __restrict__ eff,
                                                              const float* __restrict__ vae, const float* __restrict__ cm,
                                                              const float* __restrict__ cs, const float* __restrict__ bank_enc,
                                                              const int32_t* __restrict__ gidx, long long bank_rows,
                                                              float* __restrict__ prev, int32_t* __restrict__ seeded, int rows /*S*90*/,
                                                              OursGroup grp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), q = threadIdx.x & 63;
    if (row >= rows) return;
    const int s = row / 90, t = row - s * 90;
    const int mode = counters[s * 3 + 2];                       // written by mocha_live_ours_condition; this kernel does not write it
    if (GROUPED && mode == 2) {                                 // the slot the condition kernel chose: a chaining stream always has one
        const int slot = grp.slot[s];
        const float* st = grp.stats + (size_t)(slot < 0 ? 0 : slot) * 4 * 90 * 256;
        cm = st + 2 * 90 * 256; cs = st + 3 * 90 * 256;
    }
    if (t == 0 && q == 0) {
        seeded[s] = mode == 1 ? 1 : 0;
        if (mode != 0) {
            const int chain = counters[s * 3];
            counters[s * 3] = chain == 0x7FFFFFFF ? 1 : chain + 1;
            counters[s * 3 + 1] = eff[s];
        }
    }
    if (mode == 2) {
        const f32x4 v = reinterpret_cast<const f32x4*>(vae)[(size_t)row * 64 + q];
        reinterpret_cast<f32x4*>(prev)[(size_t)row * 64 + q] =
            v * reinterpret_cast<const f32x4*>(cs)[t * 64 + q] + reinterpret_cast<const f32x4*>(cm)[t * 64 + q];
    } else if (mode == 1) {
        long long g = gidx[s];
        g = g < 0 ? 0 : (g >= bank_rows ? bank_rows - 1 : g);
        reinterpret_cast<f32x4*>(prev)[(size_t)row * 64 + q] = reinterpret_cast<const f32x4*>(bank_enc)[((size_t)g * 90 + t) * 64 + q];
    }
}

hipError_t launch_live_ours_update(int32_t* counters, const int32_t* eff, const float* vae, const float* cm, const float* cs,
                                   const float* bank_enc, const int32_t* gidx, long long bank_rows, float* prev, int32_t* seeded, int S,
                                   hipStream_t s, const OursGroup* grp) {
    if (S <= 0) return hipSuccess;
    if (bank_rows < 1) return hipErrorInvalidValue;
    if (grp && (!grp->stats || !grp->slot || grp->Cw < 1)) return hipErrorInvalidValue;
    const int rows = S * 90;
    if (grp)
        hipLaunchKernelGGL(mocha_live_ours_update<true>, dim3((rows + 3) / 4), dim3(256), 0, s, counters, eff, vae, cm, cs, bank_enc, gidx,
                           bank_rows, prev, seeded, rows, *grp);
    else
        hipLaunchKernelGGL(mocha_live_ours_update<false>, dim3((rows + 3) / 4), dim3(256), 0, s, counters, eff, vae, cm, cs, bank_enc, gidx,
                           bank_rows, prev, seeded, rows, OursGroup{});
    return hipGetLastError();
}

}  // namespace mocha
