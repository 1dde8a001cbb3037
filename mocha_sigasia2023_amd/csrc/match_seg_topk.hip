// Soft context matching against a MULTI-CHARACTER bank: per query the k nearest rows of its OWN segment (1 <= k <= SEG_TOPK_MAX_K), exact,
// and the softmax-weighted blend of their encoded features - tree.query(q, k) of that character's BallTree plus the blend, on the device,
// segment ids as device data, nothing allocated: the matcher of the soft characterize / captured step / live step.
//
// Up to SEG_TOPK_Q = 16 queries per launch group (the key buffer holds 16 queries' keys); a larger batch walks its queries 16 at a time.
// 1. mocha_seg_plan (match_segmented.hip): the group's queries as blocks of up to 8 of one segment.
// 2. mocha_match_seg_keys: mocha_match_seg_scan's workgroup with the all-keys flag (match_seg_body.h: ONE body, the same lanes, sums and
//    order - every squared distance has the bits the 1-NN scan gives it).  Instead of one minimum per (query, workgroup) it writes the key
//    of each of the workgroup's 16 rows to keys[q][local row] (stride: the largest segment's rows rounded up to 16; ~0 past the segment's
//    end).  One pass over the rows of a segment per block, the bytes of the hard scan; + 8 B written per (row, query).
// 3. mocha_seg_topk_blend (one workgroup per query): ONE read of the query's keys - every thread keeps the 8 smallest it saw as a sorted
//    list in registers; k rounds of a workgroup minimum over the lists' heads (wave shuffles, then 4 words of LDS) pop the k smallest in
//    ascending order.  Keys are unique (the local row is their low word), so ties go to the lower row.  Then, per neighbour, the distance
//    the segmented calls report (seg_direct_dist2: for k = 1 the bits of mocha_match_seg_finish), the max-subtracted softmax of
//    -dist / temperature over the neighbours present (mocha_gather_blend's, with the distances subtracted before the scaling), and
//    out = sum_j w_j * encoded[seg start + idx_j] with 16-byte loads, j ascending, every product and sum rounded on its own (contraction
//    switched off: a staged blend of separate multiplies and adds in the same order has the same bits; w = {1} gives the row itself).
//    An id outside [0, S): idx -1, dist +inf, w 0, out = encoded[0] (an in-bank row for the decoder, as mocha_match_seg_finish's global
//    row 0).  No kernel indexes the bank with an id: only with rows inside [0, N).
// Action-constrained (a SegAllow, kernels.h): step 2 is mocha_match_seg_keys_allow - a row outside a constrained query's mask gets the key
// ~0, which step 3 already reads as "no row", and a workgroup of inadmissible rows writes its 16 x queries ~0 keys without reading the bank;
// step 3 also writes applied.  Fewer admissible rows than k: the missing neighbours are -1 / +inf / weight 0.
#include "kernels.h"
#include "match_seg_body.h"

namespace mocha {

typedef float st_f32x4 __attribute__((ext_vector_type(4)));

// PAIRS (here and below): seg_start is a resident bank's slot table (match_seg_body.h, seg_extent); an empty slot is an invalid id
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_match_seg_keys(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                            const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ keys, int kstride) {
    seg_scan_workgroup<BF16, true, false, PAIRS>(bank, query, plan, seg_start, D, keys, kstride);
}

// the all-keys scan of the action-constrained soft matcher: a row outside a constrained query's mask gets the key ~0 - to the selection
// below a missing row - and workgroups of inadmissible rows write their 16 x queries ~0 keys without reading the bank
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_match_seg_keys_allow(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                                  const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ keys, int kstride,
                                                                  SegAllow al) {
    seg_scan_workgroup<BF16, true, true, PAIRS>(bank, query, plan, seg_start, D, keys, kstride, al);
}

// keys: [group's queries][kstride]; idx0 (Q) / idx_k, dist_k, w_k (Q, k) / out (Q, cols4 x 4): each may be null
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_seg_topk_blend(const unsigned long long* __restrict__ keys, int kstride, const int32_t* __restrict__ seg, int S,
                                                            const int* __restrict__ seg_start, const void* __restrict__ bank,
                                                            const float* __restrict__ query, int D, const float* __restrict__ enc, int cols4, int k,
                                                            float inv_temp, int32_t* __restrict__ idx0, int32_t* __restrict__ idx_k,
                                                            float* __restrict__ dist_k, float* __restrict__ w_k, float* __restrict__ out,
                                                            const unsigned long long* __restrict__ allow, const unsigned long long* __restrict__ any,
                                                            int32_t* __restrict__ applied) {
    __shared__ unsigned long long wmin[MS_WAVES];
    __shared__ unsigned long long sel[SEG_TOPK_MAX_K];
    __shared__ float red[4];
    __shared__ float dj[SEG_TOPK_MAX_K], wj[SEG_TOPK_MAX_K];
    __shared__ long long rowj[SEG_TOPK_MAX_K];         // global row of neighbour j, -1 = missing
    const int q = blockIdx.x, tid = threadIdx.x;
    const int s = seg[q];
    st_f32x4* o = out ? reinterpret_cast<st_f32x4*>(out) + (size_t)q * cols4 : nullptr;
    bool none = s < 0 || s >= S;
    long long lo = 0, n = 0;
    if (!none) {
        seg_extent<PAIRS>(seg_start, s, lo, n);
        if (PAIRS) none = n == 0;
    }
    if (none) {                                   // an id outside the table (or an empty slot): no neighbour; the decoder reads row 0
        if (tid < k) {
            if (idx_k) idx_k[(size_t)q * k + tid] = -1;
            if (dist_k) dist_k[(size_t)q * k + tid] = __builtin_inff();
            if (w_k) w_k[(size_t)q * k + tid] = 0.f;
        }
        if (tid == 0 && idx0) idx0[q] = -1;
        if (tid == 0 && applied) applied[q] = 0;
        if (o) for (int i = tid; i < cols4; i += 256) o[i] = reinterpret_cast<const st_f32x4*>(enc)[i];
        return;
    }
    const long long n16 = (n + SEG_ROWS - 1) / SEG_ROWS * SEG_ROWS;          // what the scan wrote of this query's keys (<= kstride)
    const unsigned long long* kq = keys + (size_t)q * kstride;

    // the 8 smallest keys this thread sees, ascending
    unsigned long long l[SEG_TOPK_MAX_K];
#pragma unroll
    for (int j = 0; j < SEG_TOPK_MAX_K; ++j) l[j] = ~0ull;
    for (long long i = tid; i < n16; i += 256) {
        const unsigned long long v = kq[i];
        if (v < l[SEG_TOPK_MAX_K - 1]) {
#pragma unroll
            for (int j = SEG_TOPK_MAX_K - 1; j > 0; --j) l[j] = v < l[j - 1] ? l[j - 1] : (v < l[j] ? v : l[j]);
            l[0] = v < l[0] ? v : l[0];
        }
    }
    // k rounds: the workgroup's smallest head is the next neighbour; its owner pops it
    for (int r = 0; r < k; ++r) {
        unsigned long long m = l[0];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const unsigned long long t = __shfl_xor(m, off); m = t < m ? t : m; }
        if ((tid & 63) == 0) wmin[tid >> 6] = m;
        __syncthreads();
        unsigned long long best = wmin[0];
#pragma unroll
        for (int w = 1; w < MS_WAVES; ++w) best = wmin[w] < best ? wmin[w] : best;
        if (best != ~0ull && l[0] == best) {
#pragma unroll
            for (int j = 0; j < SEG_TOPK_MAX_K - 1; ++j) l[j] = l[j + 1];
            l[SEG_TOPK_MAX_K - 1] = ~0ull;
        }
        if (tid == 0) sel[r] = best;
        __syncthreads();
    }
    // the neighbours' rows and reported distances
    for (int j = 0; j < k; ++j) {
        const unsigned long long key = sel[j];
        const long long local = (long long)(key & 0xffffffffull);
        const bool have = key != ~0ull && local < n;         // fewer than k rows in the segment: missing
        float d = __builtin_inff();
        if (have) d = sqrtf(seg_direct_dist2<BF16>(bank, query + (size_t)q * D, (size_t)(lo + local), D, red));      // (uniform branch)
        if (tid == 0) { rowj[j] = have ? lo + local : -1; dj[j] = d; }
        __syncthreads();
    }
    if (tid == 0) {
        // max-subtracted softmax of -dist / temperature; the distances are subtracted BEFORE the scaling (an exact difference of two
        // nearby floats), so the exponent keeps its digits when the distances are large against the temperature
        float dmin = INFINITY;
        for (int j = 0; j < k; ++j) if (rowj[j] >= 0) dmin = fminf(dmin, dj[j]);
        float sum = 0.f;
        for (int j = 0; j < k; ++j) { wj[j] = rowj[j] >= 0 ? __expf((dmin - dj[j]) * inv_temp) : 0.f; sum += wj[j]; }
        for (int j = 0; j < k; ++j) {
            wj[j] = sum > 0.f ? wj[j] / sum : 0.f;
            if (idx_k) idx_k[(size_t)q * k + j] = rowj[j] >= 0 ? (int32_t)(rowj[j] - lo) : -1;
            if (dist_k) dist_k[(size_t)q * k + j] = dj[j];
            if (w_k) w_k[(size_t)q * k + j] = wj[j];
        }
        if (idx0) idx0[q] = rowj[0] >= 0 ? (int32_t)(rowj[0] - lo) : -1;
        if (applied) applied[q] = seg_allow_applied(allow[q], any[s]);
    }
    if (!o) return;
    __syncthreads();
    for (int i = tid; i < cols4; i += 256) {
        // no contraction into fused multiply-adds here (HIP's default would fuse, and __fmul_rn / __fadd_rn are plain operators to this
        // compiler): a product rounded, then a sum rounded, which is what a staged blend made of separate multiplies and adds computes
#pragma clang fp contract(off)
        st_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < k; ++j) {
            if (rowj[j] < 0) continue;
            const st_f32x4 x = (reinterpret_cast<const st_f32x4*>(enc) + (size_t)rowj[j] * cols4)[i];
            const st_f32x4 p = wj[j] * x;
            acc = acc + p;
        }
        o[i] = acc;
    }
}

static inline int seg_key_stride(int64_t max_rows) { return (int)((max_rows + SEG_ROWS - 1) / SEG_ROWS * SEG_ROWS); }

size_t match_seg_keys_words(int64_t max_rows) { return (size_t)SEG_TOPK_Q * (size_t)seg_key_stride(max_rows); }

int match_seg_key_stride(int64_t max_rows) { return seg_key_stride(max_rows); }

// steps 1 and 2 alone, on fp32 rows, for ONE group of up to SEG_TOPK_Q queries: the online path step reads the keys (match_path_step.hip)
hipError_t launch_match_seg_keys(const float* bank, const float* query, const int32_t* seg, int Q, const int* seg_start, int S, int64_t max_rows, int D,
                                 unsigned long long* keys, int* plan, hipStream_t s, int slot_table) {
    if (Q < 1 || Q > SEG_TOPK_Q || S < 1 || max_rows < 1 || max_rows > 0x7fffffff - SEG_ROWS || D % MS_CHUNK_F32 != 0) return hipErrorInvalidValue;
    const int kstride = seg_key_stride(max_rows);
    hipError_t e = launch_seg_plan(seg, Q, S, plan, s);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(kstride / SEG_ROWS), (unsigned)seg_blocks_bound(Q, S));
    if (slot_table) hipLaunchKernelGGL((mocha_match_seg_keys<false, true>), grid, dim3(256), 0, s, bank, query, plan, seg_start, D, keys, kstride);
    else hipLaunchKernelGGL(mocha_match_seg_keys<false>, grid, dim3(256), 0, s, bank, query, plan, seg_start, D, keys, kstride);
    return hipGetLastError();
}

hipError_t launch_match_seg_topk(const void* bank, int bank_bf16, const float* query, const int32_t* seg, int Q, const int* seg_start, int S,
                                 int64_t max_rows, int D, unsigned long long* keys, int* plan, const float* enc, int k, float temperature,
                                 int32_t* idx0, int32_t* idx_k, float* dist_k, float* w_k, float* out, hipStream_t s, const SegAllow* al,
                                 int slot_table) {
    if (Q <= 0) return hipSuccess;
    if (slot_table && bank_bf16) return hipErrorInvalidValue;          // a resident bank is fp32
    if (al && (!al->allow || !al->label || !al->any || !al->gran || !al->gran_start)) return hipErrorInvalidValue;
    if (S < 1 || max_rows < 1 || max_rows > 0x7fffffff - SEG_ROWS || D % (bank_bf16 ? MS_CHUNK_BF16 : MS_CHUNK_F32) != 0 || D % 4 != 0 || k < 1 ||
        k > SEG_TOPK_MAX_K || !(temperature > 0.f) || (out && !enc))
        return hipErrorInvalidValue;
    const int kstride = seg_key_stride(max_rows);
    const unsigned gx = (unsigned)(kstride / SEG_ROWS);
    const float inv_temp = 1.0f / temperature;
    for (int q0 = 0; q0 < Q; q0 += SEG_TOPK_Q) {        // the key buffer is reused group after group (same stream)
        const int n = (Q - q0) < SEG_TOPK_Q ? (Q - q0) : SEG_TOPK_Q;
        const float* qp = query + (size_t)q0 * D;
        const int32_t* sp = seg + q0;
        hipError_t e = launch_seg_plan(sp, n, S, plan, s);
        if (e != hipSuccess) return e;
        const unsigned gy = (unsigned)seg_blocks_bound(n, S);
        int32_t* i0 = idx0 ? idx0 + q0 : nullptr;
        int32_t* ik = idx_k ? idx_k + (size_t)q0 * k : nullptr;
        float* dk = dist_k ? dist_k + (size_t)q0 * k : nullptr;
        float* wk = w_k ? w_k + (size_t)q0 * k : nullptr;
        float* op = out ? out + (size_t)q0 * D : nullptr;
        SegAllow g{};                                   // this group's masks and report
        if (al) { g = *al; g.allow += q0; if (g.applied) g.applied += q0; }
        if (slot_table) {
            if (al) hipLaunchKernelGGL((mocha_match_seg_keys_allow<false, true>), dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride, g);
            else hipLaunchKernelGGL((mocha_match_seg_keys<false, true>), dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride);
            hipLaunchKernelGGL((mocha_seg_topk_blend<false, true>), dim3(n), dim3(256), 0, s, keys, kstride, sp, S, seg_start, bank, qp, D, enc, D / 4, k,
                               inv_temp, i0, ik, dk, wk, op, g.allow, g.any, g.applied);
        } else if (bank_bf16) {
            if (al) hipLaunchKernelGGL(mocha_match_seg_keys_allow<true>, dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride, g);
            else hipLaunchKernelGGL(mocha_match_seg_keys<true>, dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride);
            hipLaunchKernelGGL(mocha_seg_topk_blend<true>, dim3(n), dim3(256), 0, s, keys, kstride, sp, S, seg_start, bank, qp, D, enc, D / 4, k, inv_temp,
                               i0, ik, dk, wk, op, g.allow, g.any, g.applied);
        } else {
            if (al) hipLaunchKernelGGL(mocha_match_seg_keys_allow<false>, dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride, g);
            else hipLaunchKernelGGL(mocha_match_seg_keys<false>, dim3(gx, gy), dim3(256), 0, s, bank, qp, plan, seg_start, D, keys, kstride);
            hipLaunchKernelGGL(mocha_seg_topk_blend<false>, dim3(n), dim3(256), 0, s, keys, kstride, sp, S, seg_start, bank, qp, D, enc, D / 4, k, inv_temp,
                               i0, ik, dk, wk, op, g.allow, g.any, g.applied);
        }
    }
    return hipGetLastError();
}

}  // namespace mocha
