// Character mixing on a MULTI-CHARACTER bank: a window is characterized by up to SEG_MIX_MAX_J (character, six body-part weights) components
// instead of exactly one character.  Every present component is matched exactly in its own character and the decoder reads, body part by
// body part, the weighted blend of the matched entries' encoded features: a strength dial (zombie 0.7, neutral 0.3), a cross-fade (a
// weight ramp) and a splice by body part (arms of A, legs of B) are one operation.  Tokens are (15 time patches x 6 body parts), token =
// t * 6 + v, so part v of every time patch takes component j's feature with the weight what[j][v].  Nothing is trained.
//
// ids, weights, the segment / slot table and (live steps) the push's gate are device data: a captured step replays with new ids and weights.
//
// 1. mocha_mix_prep (one workgroup, one thread per window): component j is PRESENT iff its id names a loaded character (inside the table,
//    on a resident bank a non-empty slot), at least one of its six weights is usable (0 < w <= FLT_MAX: NaN, negatives, zero and infinities
//    count as 0) and the window's gate is open.  Writes the Q x J EFFECTIVE ids (-1 where not present: the scan reads no bank row for them)
//    and the normalised weights: per part v, s_v = the sum of the usable weights of present components (fp32, j ascending); s_v > 0:
//    what[j][v] = w[j][v] / s_v (one IEEE division); otherwise the lowest present j gets 1.  In a live step it also rewrites valid[q]: a
//    stream none of whose components is present sits the step out as a warming one does.
// 2. The scan over the Q x J PSEUDO-queries: mocha_seg_plan on the effective ids, then the MIX instances of the ONE scan body and finish
//    body (match_seg_body.h), which map pseudo-query p to query row p / J - the J pseudo-queries of a window share its one query row,
//    nothing is replicated.  (Chosen over staging replicated rows: no J x 92 KB copy per window and no further scratch; the non-MIX
//    instances compile to the kernels they were.)  Index, tie rule, distance: launch_match_segmented's for (that query, that id), bit for bit.
//    Cost: sum over blocks (up to 8 pseudo-queries of one character) of that character's rows x D x bytes per value.
// 3. mocha_seg_mix_blend (15 workgroups per window, one per time patch: 6 tokens = 384 float4, the part of a float4 is its index >> 6):
//    out = sum_j what[j][v] * enc[row_j] with 16-byte loads and stores in mocha_seg_topk_blend's arithmetic - from 0 in fp32, j ascending,
//    every product and every sum rounded on its own (contraction off); a term whose weight is 0 is skipped and its row is not read, so one
//    effective component gives that entry's bits.  No component present: out = enc[0] (an in-bank row for the decoder, as an invalid id
//    in the hard and soft matchers).  The workgroups of time patch 0 also copy idx / dist (Q,J) out of the scratch.
#include "kernels.h"
#include "match_seg_body.h"

namespace mocha {

typedef float mx_f32x4 __attribute__((ext_vector_type(4)));

static constexpr int MIX_P = SEG_MIX_Q * SEG_MIX_MAX_J;          // pseudo-queries per launch
static constexpr int MIX_PATCHES = 15, MIX_PATCH4 = SEG_MIX_PARTS * 64;      // time patches; float4 per time patch (6 tokens x 64)

// iscr: effective ids | local rows | global rows (MIX_P each); fscr: normalised weights (MIX_P x 6) | distances (MIX_P)
size_t seg_mix_scratch_ints() { return 3 * (size_t)MIX_P; }
size_t seg_mix_scratch_floats() { return (size_t)MIX_P * (SEG_MIX_PARTS + 1); }

__device__ __forceinline__ bool mix_usable(float w) { return w > 0.f && w <= 3.402823466e+38f; }       // (false for a NaN)

template <bool PAIRS>
__global__ __launch_bounds__(64) void mocha_mix_prep(const int32_t* __restrict__ ids, const float* __restrict__ weights, int Q, int J,
                                                     const int* __restrict__ table, int S, const int32_t* __restrict__ gate,
                                                     int32_t* __restrict__ valid, int32_t* __restrict__ eff, float* __restrict__ what,
                                                     float* __restrict__ wnorm) {
    for (int q = threadIdx.x; q < Q; q += 64) {
        const bool open = !gate || gate[q] >= 0;
        const float* w = weights + (size_t)q * J * SEG_MIX_PARTS;
        bool present[SEG_MIX_MAX_J];
        int first = -1;                                               // the lowest present component
#pragma unroll
        for (int j = 0; j < SEG_MIX_MAX_J; ++j) {
            present[j] = false;
            if (j >= J) continue;
            const int id = ids[(size_t)q * J + j];
            bool p = open && id >= 0 && id < S;
            if (p) {                                                  // (the table is indexed with ids inside it only)
                long long lo, n;
                seg_extent<PAIRS>(table, id, lo, n);
                p = n > 0;
            }
            bool any = false;
            for (int v = 0; v < SEG_MIX_PARTS; ++v) any = any || mix_usable(w[j * SEG_MIX_PARTS + v]);
            p = p && any;
            present[j] = p;
            if (p && first < 0) first = j;
            eff[(size_t)q * J + j] = p ? id : -1;
        }
        if (valid) valid[q] = first >= 0 ? 1 : 0;
        for (int v = 0; v < SEG_MIX_PARTS; ++v) {
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < SEG_MIX_MAX_J; ++j)
                if (j < J && present[j] && mix_usable(w[j * SEG_MIX_PARTS + v])) sum += w[j * SEG_MIX_PARTS + v];
#pragma unroll
            for (int j = 0; j < SEG_MIX_MAX_J; ++j) {
                if (j >= J) continue;
                float r = 0.f;
                if (present[j]) {
                    if (sum > 0.f) r = mix_usable(w[j * SEG_MIX_PARTS + v]) ? __fdiv_rn(w[j * SEG_MIX_PARTS + v], sum) : 0.f;
                    else r = j == first ? 1.f : 0.f;
                }
                const size_t o = ((size_t)q * J + j) * SEG_MIX_PARTS + v;
                what[o] = r;
                if (wnorm) wnorm[o] = r;
            }
        }
    }
}

// the scan and the finish over pseudo-queries: the MIX instances of the one scan body and the one finish body (match_seg_body.h)
template <bool BF16, bool PAIRS>
__global__ __launch_bounds__(256) void mocha_match_seg_scan_mix(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                                const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ partial,
                                                                int mix_j) {
    seg_scan_workgroup<BF16, false, false, PAIRS, true>(bank, query, plan, seg_start, D, partial, (int)gridDim.x, SegAllow{}, mix_j);
}

template <bool BF16, bool PAIRS>
__global__ __launch_bounds__(256) void mocha_match_seg_finish_mix(const unsigned long long* __restrict__ partial, int pstride, const int32_t* __restrict__ eff,
                                                                  int S, const int* __restrict__ seg_start, const void* __restrict__ bank,
                                                                  const float* __restrict__ query, int D, int32_t* __restrict__ idx,
                                                                  int32_t* __restrict__ gidx, float* __restrict__ dist, int mix_j) {
    seg_finish_workgroup<BF16, PAIRS, true>(partial, pstride, eff, S, seg_start, bank, query, D, idx, gidx, dist, nullptr, nullptr, nullptr, mix_j);
}

// grid (windows, MIX_PATCHES).  eff / gidx_s / idx_s / dist_s / what: the launch's scratch; out (or null): (Q, 90 x 64) float4; idx (or
// null) / dist (or null): (Q,J).  Every row read is gidx_s's - a row inside the bank (0 for a component that is not present) - or row 0.
__global__ __launch_bounds__(256) void mocha_seg_mix_blend(const int32_t* __restrict__ eff, const int32_t* __restrict__ gidx_s,
                                                           const int32_t* __restrict__ idx_s, const float* __restrict__ dist_s,
                                                           const float* __restrict__ what, int J, const float* __restrict__ enc,
                                                           float* __restrict__ out, int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ float wl[SEG_MIX_MAX_J * SEG_MIX_PARTS];
    __shared__ long long rowl[SEG_MIX_MAX_J];
    __shared__ int anyl;
    const int q = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) {
        int any = 0;
        for (int j = 0; j < J; ++j) any |= eff[(size_t)q * J + j] >= 0;
        anyl = any;
    }
    if (tid < J) {
        rowl[tid] = gidx_s[(size_t)q * J + tid];
        if (t == 0) {
            if (idx) idx[(size_t)q * J + tid] = idx_s[(size_t)q * J + tid];
            if (dist) dist[(size_t)q * J + tid] = dist_s[(size_t)q * J + tid];
        }
    }
    if (tid < J * SEG_MIX_PARTS) wl[tid] = what[(size_t)q * J * SEG_MIX_PARTS + tid];
    if (!out) return;
    __syncthreads();
    constexpr size_t ROW4 = (size_t)MIX_PATCHES * MIX_PATCH4;        // float4 per encoded row
    const mx_f32x4* e = reinterpret_cast<const mx_f32x4*>(enc) + (size_t)t * MIX_PATCH4;
    mx_f32x4* o = reinterpret_cast<mx_f32x4*>(out) + (size_t)q * ROW4 + (size_t)t * MIX_PATCH4;
    if (!anyl) {                                      // no component present: the decoder reads row 0
        for (int i = tid; i < MIX_PATCH4; i += 256) o[i] = e[i];
        return;
    }
    for (int i = tid; i < MIX_PATCH4; i += 256) {
        // no contraction into fused multiply-adds (mocha_seg_topk_blend): a product rounded, then a sum rounded, which is what a staged
        // blend made of separate multiplies and adds computes
#pragma clang fp contract(off)
        const int v = i >> 6;                         // 64 float4 per token: the token's body part within its time patch
        mx_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < J; ++j) {
            const float w = wl[j * SEG_MIX_PARTS + v];
            if (w == 0.f) continue;
            const mx_f32x4 x = (e + (size_t)rowl[j] * ROW4)[i];
            const mx_f32x4 p = w * x;
            acc = acc + p;
        }
        o[i] = acc;
    }
}

hipError_t launch_match_seg_mix(const void* bank, int bank_bf16, const float* query, const int32_t* ids, const float* weights, int Q, int J,
                                const int* seg_start, int S, int64_t max_rows, int D, unsigned long long* partial, int* plan, int32_t* iscr,
                                float* fscr, const float* enc, const int32_t* gate, int32_t* valid, int32_t* idx, float* dist, float* wnorm,
                                float* out, hipStream_t s, int slot_table) {
    if (Q <= 0) return hipSuccess;
    if (slot_table && bank_bf16) return hipErrorInvalidValue;          // a resident bank is fp32
    if (Q > SEG_MIX_Q || J < 1 || J > SEG_MIX_MAX_J || S < 1 || max_rows < 1 || D != MIX_PATCHES * MIX_PATCH4 * 4 ||
        D % (bank_bf16 ? MS_CHUNK_BF16 : MS_CHUNK_F32) != 0 || !ids || !weights || !iscr || !fscr || (out && !enc))
        return hipErrorInvalidValue;
    const int P = Q * J;
    int32_t *eff = iscr, *idx_s = iscr + MIX_P, *gidx_s = iscr + 2 * MIX_P;
    float *what = fscr, *dist_s = dist ? fscr + (size_t)MIX_P * SEG_MIX_PARTS : nullptr;
    if (slot_table) hipLaunchKernelGGL(mocha_mix_prep<true>, dim3(1), dim3(64), 0, s, ids, weights, Q, J, seg_start, S, gate, valid, eff, what, wnorm);
    else hipLaunchKernelGGL(mocha_mix_prep<false>, dim3(1), dim3(64), 0, s, ids, weights, Q, J, seg_start, S, gate, valid, eff, what, wnorm);
    hipError_t e = launch_seg_plan(eff, P, S, plan, s);
    if (e != hipSuccess) return e;
    const unsigned gx = (unsigned)((max_rows + SEG_ROWS - 1) / SEG_ROWS);
    const unsigned gy = (unsigned)seg_blocks_bound(P, S);
    if (slot_table) {
        hipLaunchKernelGGL((mocha_match_seg_scan_mix<false, true>), dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, J);
        hipLaunchKernelGGL((mocha_match_seg_finish_mix<false, true>), dim3(P), dim3(256), 0, s, partial, (int)gx, eff, S, seg_start, bank, query, D, idx_s,
                           gidx_s, dist_s, J);
    } else if (bank_bf16) {
        hipLaunchKernelGGL((mocha_match_seg_scan_mix<true, false>), dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, J);
        hipLaunchKernelGGL((mocha_match_seg_finish_mix<true, false>), dim3(P), dim3(256), 0, s, partial, (int)gx, eff, S, seg_start, bank, query, D, idx_s,
                           gidx_s, dist_s, J);
    } else {
        hipLaunchKernelGGL((mocha_match_seg_scan_mix<false, false>), dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, J);
        hipLaunchKernelGGL((mocha_match_seg_finish_mix<false, false>), dim3(P), dim3(256), 0, s, partial, (int)gx, eff, S, seg_start, bank, query, D, idx_s,
                           gidx_s, dist_s, J);
    }
    hipLaunchKernelGGL(mocha_seg_mix_blend, dim3(Q, out ? MIX_PATCHES : 1), dim3(256), 0, s, eff, gidx_s, idx_s, dist_s, what, J, enc, out, idx, dist);
    return hipGetLastError();
}

}  // namespace mocha
