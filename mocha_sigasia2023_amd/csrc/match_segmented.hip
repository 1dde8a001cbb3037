// Context matching against a MULTI-CHARACTER bank: the bank is S row segments (one per character, mocha_bank_set_segments) and
// every query is matched, exactly, against its OWN segment only; the segment of each query is device data (seg[q]), so that a
// captured step can be replayed with new ids.
//
// exact 1-NN = argmin_{b in segment} sum_d (q_d - b_d)^2, in the DIRECT form as in match_stream.hip (same arithmetic: the rows'
// terms summed by the same lanes in the same order, two packed partial sums per (row, query), one wave reduction per row).
//
// 1. mocha_seg_plan (one workgroup): groups the queries by segment whatever order they come in - a stable sort by segment id
//    computed as ranks (O(Q^2) comparisons from LDS, no atomics, deterministic) - and forms BLOCKS of up to 8 queries of one
//    segment.  A query with an id outside [0, S) joins no block.
// 2. mocha_match_seg_scan: grid (row chunks of the LARGEST segment, an upper bound of the block count), both known on the host.
//    Workgroup (x, y) scans rows [16 x, 16 x + 16) of block y's segment for the block's queries and writes one partial minimum
//    per query; a workgroup beyond the block count or past the end of its segment returns at once.  Chosen over a persistent
//    grid that walks a device-built work list because the bound grid keeps the scan body that of match_stream.hip (a workgroup =
//    16 rows, every row read once per block, no per-item loop or list) and the bound is tight where it matters: with one query per
//    segment or 8 queries per segment every block is used; the idle workgroups cost a dispatch and one load each.  A pass costs
//    sum over blocks of rows(segment) x D x bytes per value.
//    The queries of a block are staged through LDS one D-chunk at a time and reused by every row; the bank rows stream once,
//    16 B per lane, straight to registers; candidates are 64-bit keys (order-preserving distance bits << 32 | local row), ties to
//    the lowest row.  The block's query count is device data: the workgroup takes the 1 / 2 / 4 / 8-query body by a uniform branch.
// 3. mocha_match_seg_finish (one workgroup per query): the query's partial minima -> local row, global row (segment start +
//    local row), and the Euclidean distance in the direct form.  An invalid id: local row -1, distance +inf, global row 0 (an
//    in-bank row for the decoder's gather).  No kernel ever indexes the bank with an id: only with rows inside [0, N).
// The bank may be fp32 rows or the centred bf16 copy (then with centred queries), as mocha_match_stream<f32|bf16>.
//
// Action-constrained matching (launch_match_segmented with a SegAllow, kernels.h): the scan is mocha_match_seg_scan_allow - the same
// grid, plan and partial minima; a workgroup first forms its queries' effective allow masks and reads ONE granule word (the label bits of
// its 16 rows): when no query admits any of them it writes ~0 minima and returns before its first bank row, otherwise it runs the plain
// distance loop and masks at key time.  With labels in runs a constrained pass reads about the admissible rows.  The finish kernel is the
// plain one and also writes applied (1 constrained / 0 nothing asked / -1 fell back).  The same three launches.
//
// A resident bank (launch_match_segmented with slot_table, kernels.h): the PAIRS = true instances of the scan and finish kernels read the
// segment as a {first row, rows} pair of a slot table instead of seg_start[s], seg_start[s + 1]; rows = 0 (an empty slot) is an invalid id.
// The plan kernel is the same (it only needs S).  The PAIRS = false instances are the kernels as they were.
//
// Character mixing (match_seg_mix.hip): the MIX form of the scan body and of the finish body (seg_finish_workgroup, match_seg_body.h) runs
// over (window, component) pseudo-queries that share their window's query row; the kernels here instantiate the MIX = false form.
#include "kernels.h"
#include "match_seg_body.h"

namespace mocha {

static constexpr int SEG_PLAN_T = 1024;

size_t seg_plan_ints(int Q, int S) { return 1 + (size_t)PLAN_STRIDE * seg_blocks_bound(Q, S); }

__global__ __launch_bounds__(SEG_PLAN_T) void mocha_seg_plan(const int32_t* __restrict__ seg, int Q, int S, int* __restrict__ plan) {
    __shared__ int sid[SEG_MAX_Q];          // id, or INT_MAX for an invalid one (sorts last, joins nothing)
    __shared__ int rnk[SEG_MAX_Q];          // position among the queries of the same segment (input order)
    const int tid = threadIdx.x;
    for (int q = tid; q < Q; q += SEG_PLAN_T) {
        const int s = seg[q];
        sid[q] = (s >= 0 && s < S) ? s : 0x7fffffff;
    }
    __syncthreads();
    for (int q = tid; q < Q; q += SEG_PLAN_T) {
        const int s = sid[q];
        int r = 0;
        for (int p = 0; p < q; ++p) r += sid[p] == s;
        rnk[q] = r;
    }
    __syncthreads();
    for (int q = tid; q < Q; q += SEG_PLAN_T) {
        const int s = sid[q];
        if (s == 0x7fffffff) continue;
        // block of q = blocks of all smaller segments (a query of rank 0 mod 8 opens one) + rank / 8
        int before = 0, cnt = 0;
        for (int p = 0; p < Q; ++p) {
            const int t = sid[p];
            before += (t < s) && (rnk[p] % 8 == 0);
            cnt += t == s;
        }
        const int r = rnk[q];
        const int b = before + r / 8;
        int* e = plan + 1 + (size_t)b * PLAN_STRIDE;
        e[2 + r % 8] = q;
        if (r % 8 == 0) {
            e[0] = s;
            e[1] = (cnt - r) < 8 ? (cnt - r) : 8;
        }
    }
    if (tid == 0) {                          // block count: one per (segment, 8 queries)
        int nb = 0;
        for (int p = 0; p < Q; ++p) nb += sid[p] != 0x7fffffff && rnk[p] % 8 == 0;
        plan[0] = nb;
    }
}

// partial: [Q][gridDim.x] (query-major, the query's chunks of its segment)
// PAIRS: seg_start is a resident bank's slot table (match_seg_body.h, seg_extent)
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_match_seg_scan(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                            const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ partial) {
    seg_scan_workgroup<BF16, false, false, PAIRS>(bank, query, plan, seg_start, D, partial, (int)gridDim.x);
}

// the action-constrained scan (match_seg_body.h, ALLOW): the same grid, the same partial minima; whole workgroups of inadmissible rows return
// before their first bank row
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_match_seg_scan_allow(const void* __restrict__ bank, const float* __restrict__ query, const int* __restrict__ plan,
                                                                  const int* __restrict__ seg_start, int D, unsigned long long* __restrict__ partial,
                                                                  SegAllow al) {
    seg_scan_workgroup<BF16, false, true, PAIRS>(bank, query, plan, seg_start, D, partial, (int)gridDim.x, al);
}

// allow / any / applied: the constrained match's masks and its per-query report (all null for the plain match); the body is
// seg_finish_workgroup (match_seg_body.h), shared with the mixing matcher's finish
// PAIRS (a resident bank's slot table): an empty slot is an invalid id
template <bool BF16, bool PAIRS = false>
__global__ __launch_bounds__(256) void mocha_match_seg_finish(const unsigned long long* __restrict__ partial, int pstride, const int32_t* __restrict__ seg, int S,
                                                              const int* __restrict__ seg_start, const void* __restrict__ bank, const float* __restrict__ query, int D,
                                                              int32_t* __restrict__ idx, int32_t* __restrict__ gidx, float* __restrict__ dist,
                                                              const unsigned long long* __restrict__ allow, const unsigned long long* __restrict__ any,
                                                              int32_t* __restrict__ applied) {
    seg_finish_workgroup<BF16, PAIRS>(partial, pstride, seg, S, seg_start, bank, query, D, idx, gidx, dist, allow, any, applied);
}

size_t match_seg_scratch_words(int Q, int64_t max_rows) {       // partial minima of Q queries against segments of up to max_rows rows
    return (size_t)Q * (size_t)((max_rows + SEG_ROWS - 1) / SEG_ROWS);
}

hipError_t launch_seg_plan(const int32_t* seg, int Q, int S, int* plan, hipStream_t s) {
    if (Q < 1 || Q > SEG_MAX_Q || S < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_seg_plan, dim3(1), dim3(SEG_PLAN_T), 0, s, seg, Q, S, plan);
    return hipGetLastError();
}

hipError_t launch_match_segmented(const void* bank, int bank_bf16, const float* query, const int32_t* seg, int Q, const int* seg_start, int S,
                                  int64_t max_rows, int D, unsigned long long* partial, int* plan, int32_t* idx, int32_t* gidx, float* dist,
                                  hipStream_t s, const SegAllow* al, int slot_table) {
    if (Q <= 0) return hipSuccess;
    if (al && (!al->allow || !al->label || !al->any || !al->gran || !al->gran_start)) return hipErrorInvalidValue;
    if (Q > SEG_MAX_Q || S < 1 || max_rows < 1 || D % (bank_bf16 ? MS_CHUNK_BF16 : MS_CHUNK_F32) != 0) return hipErrorInvalidValue;
    if (slot_table && bank_bf16) return hipErrorInvalidValue;          // a resident bank is fp32
    const unsigned gx = (unsigned)((max_rows + SEG_ROWS - 1) / SEG_ROWS);
    const unsigned gy = (unsigned)seg_blocks_bound(Q, S);
    hipLaunchKernelGGL(mocha_seg_plan, dim3(1), dim3(SEG_PLAN_T), 0, s, seg, Q, S, plan);
    const unsigned long long* am = al ? al->allow : nullptr;
    const unsigned long long* an = al ? al->any : nullptr;
    int32_t* ap = al ? al->applied : nullptr;
    if (slot_table) {
        if (al) hipLaunchKernelGGL((mocha_match_seg_scan_allow<false, true>), dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, *al);
        else hipLaunchKernelGGL((mocha_match_seg_scan<false, true>), dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial);
        hipLaunchKernelGGL((mocha_match_seg_finish<false, true>), dim3(Q), dim3(256), 0, s, partial, (int)gx, seg, S, seg_start, bank, query, D, idx, gidx,
                           dist, am, an, ap);
    } else if (bank_bf16) {
        if (al) hipLaunchKernelGGL(mocha_match_seg_scan_allow<true>, dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, *al);
        else hipLaunchKernelGGL(mocha_match_seg_scan<true>, dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial);
        hipLaunchKernelGGL(mocha_match_seg_finish<true>, dim3(Q), dim3(256), 0, s, partial, (int)gx, seg, S, seg_start, bank, query, D, idx, gidx, dist,
                           am, an, ap);
    } else {
        if (al) hipLaunchKernelGGL(mocha_match_seg_scan_allow<false>, dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial, *al);
        else hipLaunchKernelGGL(mocha_match_seg_scan<false>, dim3(gx, gy), dim3(256), 0, s, bank, query, plan, seg_start, D, partial);
        hipLaunchKernelGGL(mocha_match_seg_finish<false>, dim3(Q), dim3(256), 0, s, partial, (int)gx, seg, S, seg_start, bank, query, D, idx, gidx, dist,
                           am, an, ap);
    }
    return hipGetLastError();
}

}  // namespace mocha
