// The segmented bank scan's body and its plan layout (match_segmented.hip), shared with the all-keys scan of the soft matcher
// (match_seg_topk.hip): one body, so that both scans give every (row, query) the same squared distance to the bit.
#pragma once
#include "kernels.h"
#include "match_stream_body.h"

namespace mocha {

static constexpr int SEG_ROWS = MS_WAVES * MS_ROWS_PER_WAVE;     // rows per scan workgroup
static_assert(SEG_ROWS == SEG_GRANULE_ROWS, "the host builds one granule word per scan workgroup");

__host__ __device__ inline int seg_blocks_bound(int Q, int S) {      // sum_s ceil(c_s / 8) <= (Q + 7 min(S, Q)) / 8, and <= Q
    const int k = S < Q ? S : Q;
    const int b = (Q + 7 * k) / 8;
    return b < Q ? b : Q;
}

// plan layout (ints): [0] block count, then per block: segment, query count, 8 query indices
static constexpr int PLAN_STRIDE = 10;

// rows [row0, row0 + 4) of this wave, clamped to the segment's last row; qidx: the block's query indices (LDS)
// ALLKEYS (soft matching): every row's key goes to partial[query][local row] (pstride words per query; ~0 for the workgroup's rows past
// the segment's end) instead of one minimum per (query, workgroup) to partial[query][blockIdx.x]
// ALLOW (action-constrained matching): the distance loop is the plain one; at key time row r is a candidate of query q only if its label's
// bit is in eff[q] (LDS: the query's effective mask, all ones for an unconstrained query), else its key is ~0.  label: one byte per global
// row.  ALLOW = false reads neither.
// MIX (character mixing, match_seg_mix.hip): the block's entries are PSEUDO-queries - (window, component) pairs - whose query row is
// qrow[q] (LDS: pseudo-query / components per window) while keys still go to the pseudo-query's own words.  MIX = false never reads qrow.
template <int Q, bool BF16, bool ALLKEYS, bool ALLOW = false, bool MIX = false>
__device__ __forceinline__ void seg_scan_body(const void* __restrict__ bank, const float* __restrict__ query, const int* qidx, int nq,
                                              long long seg_lo, long long seg_n, long long row0, int D, float* __restrict__ qs,
                                              unsigned long long (*wbest)[8], unsigned long long* __restrict__ partial, int pstride,
                                              const unsigned long long* eff = nullptr, const unsigned char* __restrict__ label = nullptr,
                                              const int* qrow = nullptr) {
    constexpr int MS_CHUNK = BF16 ? MS_CHUNK_BF16 : MS_CHUNK_F32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* qsrc = MIX ? qrow : qidx;               // where query q of the block reads its row
    ms_f32x2 acc[MS_ROWS_PER_WAVE][Q];
#pragma unroll
    for (int r = 0; r < MS_ROWS_PER_WAVE; ++r)
#pragma unroll
        for (int q = 0; q < Q; ++q) acc[r][q] = ms_f32x2{0.f, 0.f};
    const int nchunks = D / MS_CHUNK;
    for (int ch = 0; ch < nchunks; ++ch) {
        __syncthreads();
        for (int i = tid; i < Q * (MS_CHUNK / 4); i += 256) {
            const int q = i / (MS_CHUNK / 4), o = i - q * (MS_CHUNK / 4);
            ms_f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < nq) v = reinterpret_cast<const ms_f32x4*>(query + (size_t)qsrc[q] * D + (size_t)ch * MS_CHUNK)[o];
            reinterpret_cast<ms_f32x4*>(qs)[i] = v;
        }
        __syncthreads();
        if (!BF16) {
            ms_f32x4 bv[MS_ROWS_PER_WAVE][5];
#pragma unroll
            for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
                long long row = row0 + r;
                row = seg_lo + (row < seg_n ? row : seg_n - 1);
                const ms_f32x4* bp = reinterpret_cast<const ms_f32x4*>(reinterpret_cast<const float*>(bank) + (size_t)row * D + (size_t)ch * MS_CHUNK);
#pragma unroll
                for (int i = 0; i < 5; ++i) bv[r][i] = __builtin_nontemporal_load(bp + lane + 64 * i);
            }
#pragma unroll
            for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const ms_f32x4 qv = reinterpret_cast<const ms_f32x4*>(qs)[q * (MS_CHUNK / 4) + lane + 64 * i];
#pragma unroll
                    for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
                        const ms_f32x4 d = bv[r][i] - qv;
                        const ms_f32x2 dl = {d[0], d[1]}, dh = {d[2], d[3]};
                        acc[r][q] = __builtin_elementwise_fma(dl, dl, acc[r][q]);
                        acc[r][q] = __builtin_elementwise_fma(dh, dh, acc[r][q]);
                    }
                }
        } else {
            ms_u32x4 bv[MS_ROWS_PER_WAVE][3];
#pragma unroll
            for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
                long long row = row0 + r;
                row = seg_lo + (row < seg_n ? row : seg_n - 1);
                const ms_u32x4* bp = reinterpret_cast<const ms_u32x4*>(reinterpret_cast<const unsigned short*>(bank) + (size_t)row * D + (size_t)ch * MS_CHUNK);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const int piece = lane + 64 * i;
                    ms_u32x4 z = {0u, 0u, 0u, 0u};
                    bv[r][i] = piece < MS_CHUNK / 8 ? __builtin_nontemporal_load(bp + piece) : z;
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int piece = lane + 64 * i;
                if (piece < MS_CHUNK / 8) {
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const ms_f32x4 q0 = reinterpret_cast<const ms_f32x4*>(qs)[q * (MS_CHUNK / 4) + piece * 2];
                        const ms_f32x4 q1 = reinterpret_cast<const ms_f32x4*>(qs)[q * (MS_CHUNK / 4) + piece * 2 + 1];
#pragma unroll
                        for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
                            const ms_u32x4 w = bv[r][i];
                            ms_f32x2 d;
                            d = ms_f32x2{__uint_as_float(w[0] << 16), __uint_as_float(w[0] & 0xffff0000u)} - ms_f32x2{q0[0], q0[1]};
                            acc[r][q] = __builtin_elementwise_fma(d, d, acc[r][q]);
                            d = ms_f32x2{__uint_as_float(w[1] << 16), __uint_as_float(w[1] & 0xffff0000u)} - ms_f32x2{q0[2], q0[3]};
                            acc[r][q] = __builtin_elementwise_fma(d, d, acc[r][q]);
                            d = ms_f32x2{__uint_as_float(w[2] << 16), __uint_as_float(w[2] & 0xffff0000u)} - ms_f32x2{q1[0], q1[1]};
                            acc[r][q] = __builtin_elementwise_fma(d, d, acc[r][q]);
                            d = ms_f32x2{__uint_as_float(w[3] << 16), __uint_as_float(w[3] & 0xffff0000u)} - ms_f32x2{q1[2], q1[3]};
                            acc[r][q] = __builtin_elementwise_fma(d, d, acc[r][q]);
                        }
                    }
                }
            }
        }
    }
    unsigned long long rbit[MS_ROWS_PER_WAVE];         // ALLOW: the label bit of each of this wave's rows (uniform per wave; 0 past the end)
    if (ALLOW) {
#pragma unroll
        for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
            const long long row = row0 + r;
            rbit[r] = row < seg_n ? 1ull << (label[seg_lo + row] & 63) : 0ull;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        unsigned long long kmin = ~0ull;
        const unsigned long long em = ALLOW ? eff[q] : 0ull;
#pragma unroll
        for (int r = 0; r < MS_ROWS_PER_WAVE; ++r) {
            const long long row = row0 + r;
            float v = acc[r][q][0] + acc[r][q][1];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            unsigned long long k = row < seg_n ? pack_key(v, (unsigned)row) : ~0ull;      // local row: ties to the lowest
            if (ALLOW) k = (rbit[r] & em) ? k : ~0ull;
            if (ALLKEYS) {
                // row < 16 (blockIdx.x + 1) <= the segment's rows rounded up to 16 <= pstride
                if (lane == 0 && q < nq) partial[(size_t)qidx[q] * pstride + row] = k;
            } else {
                kmin = k < kmin ? k : kmin;
            }
        }
        if (!ALLKEYS && lane == 0) wbest[wave][q] = kmin;
    }
    if (ALLKEYS) return;
    __syncthreads();
    if (tid < nq) {                                  // tid < nq <= Q
        unsigned long long k = wbest[0][tid];
#pragma unroll
        for (int w = 1; w < MS_WAVES; ++w) k = wbest[w][tid] < k ? wbest[w][tid] : k;
        partial[(size_t)qidx[tid] * pstride + blockIdx.x] = k;
    }
}

// The segment table's two forms (kernels.h): PAIRS = false, seg_start[S + 1] of contiguous segments; PAIRS = true, the slot table of a
// resident bank - {first row, rows} per slot, rows = 0 for an empty slot.  -> the segment's first global row and its row count
template <bool PAIRS>
__device__ __forceinline__ void seg_extent(const int* __restrict__ table, int s, long long& lo, long long& n) {
    if (PAIRS) {
        lo = table[2 * s];
        n = table[2 * s + 1];
    } else {
        lo = table[s];
        n = (long long)table[s + 1] - lo;
    }
}

// One scan workgroup: (x, y) scans rows [16 x, 16 x + 16) of block y's segment for the block's queries; a workgroup beyond the block count or
// past the end of its segment (every workgroup of an empty slot) returns at once.  pstride: words per query of `partial` (gridDim.x
// minima, or the key stride).
// ALLOW: al's masks and tables (kernels.h, SegAllow).  The workgroup forms its queries' effective masks in LDS, and when no query admits
// any label of its 16 rows (the granule word) it writes ~0 for each query - one minimum, or the 16 row keys, which the finish / top-k
// kernels read - and returns before the first bank row.
// MIX: the plan's entries are pseudo-queries, mix_j of them per query row (seg_scan_body); MIX = false ignores mix_j.
template <bool BF16, bool ALLKEYS, bool ALLOW = false, bool PAIRS = false, bool MIX = false>
__device__ __forceinline__ void seg_scan_workgroup(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                   const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ partial, int pstride,
                                                   SegAllow al = SegAllow{}, int mix_j = 1) {
    constexpr int MS_CHUNK = BF16 ? MS_CHUNK_BF16 : MS_CHUNK_F32;
    __shared__ __attribute__((aligned(16))) float qs[8 * MS_CHUNK];
    __shared__ unsigned long long wbest[MS_WAVES][8];
    __shared__ int qidx[8];
    __shared__ unsigned long long eff[ALLOW ? 8 : 1];
    __shared__ int qrow[MIX ? 8 : 1];
    const int b = blockIdx.y;
    if (b >= plan[0]) return;
    const int* e = plan + 1 + (size_t)b * PLAN_STRIDE;
    const int s = e[0], nq = e[1];
    long long lo, n;
    seg_extent<PAIRS>(seg_start, s, lo, n);
    const long long x0 = (long long)blockIdx.x * SEG_ROWS;
    if (x0 >= n) return;
    if (threadIdx.x < 8) qidx[threadIdx.x] = threadIdx.x < nq ? e[2 + threadIdx.x] : 0;
    if (MIX && threadIdx.x < 8) qrow[threadIdx.x] = threadIdx.x < nq ? e[2 + threadIdx.x] / mix_j : 0;
    // (the body's first barrier orders qidx before its use)
    const long long row0 = x0 + (long long)(threadIdx.x >> 6) * MS_ROWS_PER_WAVE;
    if (ALLOW) {
        if (threadIdx.x < 8) {                       // (the thread that wrote qidx[t]) a slot beyond nq admits nothing
            unsigned long long m = 0ull;
            if (threadIdx.x < nq) {
                m = al.allow[e[2 + threadIdx.x]];
                m = (m & al.any[s]) ? m : ~0ull;     // nothing asked, or no row of those labels: the whole segment
            }
            eff[threadIdx.x] = m;
        }
        __syncthreads();
        unsigned long long u = 0ull;
#pragma unroll
        for (int i = 0; i < 8; ++i) u |= eff[i];
        if (!(al.gran[al.gran_start[s] + blockIdx.x] & u)) {       // uniform: no row here is anybody's candidate
            if (ALLKEYS) {
                // row < 16 (blockIdx.x + 1) <= the segment's rows rounded up to 16 <= pstride
                if (threadIdx.x < SEG_ROWS * nq) partial[(size_t)qidx[threadIdx.x / SEG_ROWS] * pstride + x0 + threadIdx.x % SEG_ROWS] = ~0ull;
            } else if (threadIdx.x < nq) {
                partial[(size_t)qidx[threadIdx.x] * pstride + blockIdx.x] = ~0ull;
            }
            return;
        }
    }
    const unsigned char* lab = ALLOW ? al.label : nullptr;
    if (nq == 1) seg_scan_body<1, BF16, ALLKEYS, ALLOW, MIX>(bank, query, qidx, nq, lo, n, row0, D, qs, wbest, partial, pstride, eff, lab, qrow);
    else if (nq == 2) seg_scan_body<2, BF16, ALLKEYS, ALLOW, MIX>(bank, query, qidx, nq, lo, n, row0, D, qs, wbest, partial, pstride, eff, lab, qrow);
    else if (nq <= 4) seg_scan_body<4, BF16, ALLKEYS, ALLOW, MIX>(bank, query, qidx, nq, lo, n, row0, D, qs, wbest, partial, pstride, eff, lab, qrow);
    else seg_scan_body<8, BF16, ALLKEYS, ALLOW, MIX>(bank, query, qidx, nq, lo, n, row0, D, qs, wbest, partial, pstride, eff, lab, qrow);
}

// applied[q] of the finish / blend kernels: 1 constrained, 0 nothing asked, -1 the segment has no row of the asked labels (fell back)
__device__ __forceinline__ int seg_allow_applied(unsigned long long mask, unsigned long long any) {
    return mask == 0ull ? 0 : ((mask & any) ? 1 : -1);
}

// The squared distance the segmented calls REPORT for a matched row: the direct form summed by the whole workgroup (256 threads) in one
// fixed order, on every thread's return.  red: 4 floats of LDS; the caller puts a barrier between two calls.
template <bool BF16>
__device__ __forceinline__ float seg_direct_dist2(const void* __restrict__ bank, const float* __restrict__ query_row, size_t row, int D, float* red) {
    const int tid = threadIdx.x;
    float a = 0.f;
    for (int i = tid; i < D; i += 256) {
        float b;
        if (BF16) b = __uint_as_float((unsigned)reinterpret_cast<const unsigned short*>(bank)[row * D + i] << 16);
        else b = reinterpret_cast<const float*>(bank)[row * D + i];
        const float d = query_row[i] - b;
        a = fmaf(d, d, a);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((tid & 63) == 0) red[tid >> 6] = a;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// One finish workgroup (mocha_match_seg_finish, match_segmented.hip): query q's partial minima -> local row, global row (segment start +
// local row) and the direct-form distance; an id outside the table (or an empty slot): -1 / global row 0 / +inf.
// MIX (match_seg_mix.hip): q is a pseudo-query, its query row q / mix_j; MIX = false ignores mix_j.
template <bool BF16, bool PAIRS, bool MIX = false>
__device__ __forceinline__ void seg_finish_workgroup(const unsigned long long* __restrict__ partial, int pstride, const int32_t* __restrict__ seg, int S,
                                                     const int* __restrict__ seg_start, const void* __restrict__ bank, const float* __restrict__ query,
                                                     int D, int32_t* __restrict__ idx, int32_t* __restrict__ gidx, float* __restrict__ dist,
                                                     const unsigned long long* __restrict__ allow, const unsigned long long* __restrict__ any,
                                                     int32_t* __restrict__ applied, int mix_j = 1) {
    __shared__ unsigned long long kred[256];
    __shared__ float red[4];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int s = seg[q];
    bool none = s < 0 || s >= S;
    long long lo = 0, n = 0;
    if (!none) {
        seg_extent<PAIRS>(seg_start, s, lo, n);
        if (PAIRS) none = n == 0;
    }
    if (none) {                                   // an id outside the table (or an empty slot): no match; the decoder reads row 0
        if (tid == 0) {
            if (idx) idx[q] = -1;
            if (gidx) gidx[q] = 0;
            if (dist) dist[q] = __builtin_inff();
            if (applied) applied[q] = 0;
        }
        return;
    }
    const int nch = (int)((n + SEG_ROWS - 1) / SEG_ROWS);
    const unsigned long long* pq = partial + (size_t)q * pstride;
    unsigned long long k = ~0ull;
    for (int i = tid; i < nch; i += 256) k = pq[i] < k ? pq[i] : k;
    kred[tid] = k;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) kred[tid] = kred[tid + o] < kred[tid] ? kred[tid + o] : kred[tid];
        __syncthreads();
    }
    unsigned local = (unsigned)(kred[0] & 0xffffffffull);
    local = (long long)local < n ? local : 0u;     // (a NaN-only segment: the scan still wrote in-segment rows)
    const size_t row = (size_t)(lo + local);
    if (tid == 0) {
        if (idx) idx[q] = (int32_t)local;
        if (gidx) gidx[q] = (int32_t)row;
        if (applied) applied[q] = seg_allow_applied(allow[q], any[s]);
    }
    if (!dist) return;
    const float d2 = seg_direct_dist2<BF16>(bank, query + (size_t)(MIX ? q / mix_j : q) * D, row, D, red);
    if (tid == 0) dist[q] = sqrtf(d2);
}

}  // namespace mocha
