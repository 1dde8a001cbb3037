// Coherent context matching, the online form (include/mocha_hip.h, "coherent matching in live sessions"): ONE step of the path's forward
// recursion per stream, with the recursion's row R kept in caller-owned device memory between steps.
//
// The forward pass of match_path.hip re-bases R every window (a = R[i-1][j-1] - M[i-1]) and path[last] = m[last]: the row it holds after
// window t is the last row of the whole-clip path over windows 0..t.  A step therefore needs the previous R (one float64 per row of the
// stream's character), M and m, and nothing else.
//
// mocha_match_path_step: one workgroup of 1024 threads per stream, one launch for all streams; no word is shared between workgroups and
// nothing spins.  Thread t owns the STRIDED columns t, t + 1024, ... (at most MATCH_PATH_MAX_ROWS / 1024 = 16): the state and distance
// traffic is coalesced, and R_prev[j - 1] is read from the OTHER state buffer (two buffers switched by a parity word - R[j] needs
// R_prev[j - 1], which another thread owns), so there is no hand-over through LDS.  Within a thread the columns ascend, so the first of
// equal values stays; across threads the minimum is on (value, column): the wave butterfly and the LDS pass of mocha_match_path_forward.
// Ownership boundaries a tie can straddle: lanes 63 | 64 of neighbouring waves (columns 64 w - 1 | 64 w), thread 1023 | thread 0 of the
// next round (columns 1024 k - 1 | 1024 k), and one thread's own columns j | j + 1024.
//
// Two loaders of the one body: a row of fp32 distances with a leading dimension (mocha_match_path_advance), and the all-keys scan's key
// buffer (mocha_match_seg_keys: d = sqrtf of the key's high word, as mocha_match_dist_unpack takes it).
//
// Bounds: every column index is < n <= state_rows <= MATCH_PATH_MAX_ROWS, and n <= the loader's stride; a stream whose extent fails that
// sits the step out.  A start bit outside the table reads as "no start".
#include "kernels.h"
#include "match_seg_body.h"

namespace mocha {

static constexpr int MPS_T = 1024;
static_assert(sizeof(PathStepHdr) == PATH_STEP_HDR_BYTES, "the state header's size is part of mocha_path_state_bytes");

size_t path_step_state_bytes(int streams, int state_rows) {
    return (size_t)streams * PATH_STEP_HDR_BYTES + (size_t)streams * 2 * (size_t)state_rows * sizeof(double);
}

template <bool KEYS>
__device__ __forceinline__ float path_step_load(const PathStepArgs& a, int s, int j) {
    if (KEYS) {
        unsigned u = (unsigned)(a.keys[(size_t)s * a.kstride + j] >> 32);
        u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
        return sqrtf(__uint_as_float(u));
    }
    return a.dist[(size_t)s * a.ld + j];
}

__device__ __forceinline__ bool path_step_is_start(const PathStepArgs& a, long long bit) {
    if (!a.start_bits || bit < 0 || bit >= a.n_bits) return false;
    return (a.start_bits[bit >> 5] >> (bit & 31)) & 1u;
}

template <bool KEYS>
__global__ __launch_bounds__(MPS_T) void mocha_match_path_step(PathStepArgs a) {
    __shared__ double wmin[MPS_T / 64];
    __shared__ int wcol[MPS_T / 64];
    const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    PathStepHdr* h = reinterpret_cast<PathStepHdr*>(a.state) + s;
    double* Rbase = reinterpret_cast<double*>(static_cast<char*>(a.state) + (size_t)a.streams * PATH_STEP_HDR_BYTES) + (size_t)s * 2 * a.state_rows;
    const double INF = __builtin_huge_val();

    // the stream's effective id and its extent (uniform over the workgroup)
    const int e = a.ids[s];
    bool valid = e >= 0;
    long long lo = 0, n = 0;
    int epoch = 0;
    if (a.rows) {                                          // the pure form: rows per stream, first row 0
        if (valid) n = a.rows[s];
    } else {
        valid = valid && e < a.S;
        if (valid) {
            if (a.pairs) seg_extent<true>(a.seg_table, e, lo, n); else seg_extent<false>(a.seg_table, e, lo, n);
            if (a.epochs) epoch = (int)a.epochs[e];
        }
    }
    valid = valid && n >= 1 && n <= a.state_rows && n <= (KEYS ? (long long)a.kstride : a.ld) && lo >= 0;
    if (!valid) {                                          // sits out: the decoder reads global row 0, R is not touched
        if (t == 0) {
            if (a.idx) a.idx[s] = -1;
            if (a.gidx) a.gidx[s] = 0;
            if (a.dist_out) a.dist_out[s] = __builtin_inff();
            if (a.continued) a.continued[s] = 0;
            h->running = 0;
        }
        return;
    }
    const int rs = a.restart ? a.restart[s] : 0;
    const bool restart = !h->running || h->prev_id != e || h->prev_first != (int)lo || h->prev_rows != (int)n || h->prev_epoch != epoch || rs != 0;
    const int par = h->parity & 1, mprev = h->m_prev;
    const double Mprev = h->M;
    const double* __restrict__ Rp = Rbase + (size_t)par * a.state_rows;
    double* __restrict__ Rn = Rbase + (size_t)(par ^ 1) * a.state_rows;
    const long long bit0 = a.rows ? (a.bit_off ? (long long)a.bit_off[s] : 0ll) : lo;
    const double lambda = a.lambda;
    const int N = (int)n;

    double best = INF; int bj = 0x7fffffff;
    for (int j = t; j < N; j += MPS_T) {                   // at most state_rows / 1024 <= 16 rounds
        const float d = path_step_load<KEYS>(a, s, j);
        if (a.dist_row) a.dist_row[(size_t)s * a.ld_row + j] = d;
        double R;
        if (restart) {
            R = (double)d;
        } else {
            const bool pred = j > 0 && !path_step_is_start(a, bit0 + j);
            const double x = pred ? Rp[j - 1] - Mprev : INF;
            R = (double)d + (x < lambda ? x : lambda);     // strict: a tie jumps
        }
        Rn[j] = R;
        if (R < best) { best = R; bj = j; }                // ascending columns: the first of equal values stays
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int oj = __shfl_xor(bj, o);
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (lane == 0) { wmin[wave] = best; wcol[wave] = bj; }
    __syncthreads();                                       // (also: every thread has read the header and the restart word)
    if (t != 0) return;
    best = wmin[0]; bj = wcol[0];
    for (int w = 1; w < MPS_T / 64; ++w) {
        const double ob = wmin[w];
        const int oj = wcol[w];
        if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
    }
    if (bj < 0 || bj >= N) bj = 0;                         // (a row without any number that compares: the indices stay inside the extent)
    if (a.idx) a.idx[s] = bj;
    if (a.gidx) a.gidx[s] = (int32_t)(lo + bj);
    if (a.dist_out) a.dist_out[s] = path_step_load<KEYS>(a, s, bj);
    if (a.continued) a.continued[s] = (unsigned char)(!restart && bj == mprev + 1 && bj > 0 && !path_step_is_start(a, bit0 + bj));
    h->running = 1; h->prev_id = e; h->prev_first = (int)lo; h->prev_rows = N; h->prev_epoch = epoch;
    h->m_prev = bj; h->parity = par ^ 1; h->M = best;
    if (rs != 0) a.restart[s] = 0;                         // one-shot: the word this step consumed
}

hipError_t launch_match_path_step(const PathStepArgs& a, hipStream_t s) {
    if (a.streams < 1 || a.streams > PATH_STEP_MAX_STREAMS || a.state_rows < 1 || a.state_rows > MATCH_PATH_MAX_ROWS || !a.state || !a.ids ||
        !(a.lambda >= 0.0) || a.lambda > 1.7976931348623157e308)
        return hipErrorInvalidValue;
    if (!a.rows && (!a.seg_table || a.S < 1)) return hipErrorInvalidValue;
    if (a.dist_row && a.ld_row < a.state_rows) return hipErrorInvalidValue;
    if (a.keys) {
        if (a.kstride < 1) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mocha_match_path_step<true>, dim3(a.streams), dim3(MPS_T), 0, s, a);
    } else {
        if (!a.dist || a.ld < 1) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mocha_match_path_step<false>, dim3(a.streams), dim3(MPS_T), 0, s, a);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// bank starts: one bit per global bank row, "starts a clip", and a per-slot epoch word
// ---------------------------------------------------------------------------------------------------------------------
// bits of rows [first, first + rows) cleared (two characters of a resident bank may share a 32-bit word: atomic); epoch (or null) += 1
__global__ __launch_bounds__(256) void mocha_path_starts_clear(unsigned* __restrict__ bits, long long first, long long rows, unsigned* __restrict__ epoch) {
    const long long w0 = first >> 5, w1 = (first + rows + 31) >> 5;
    const long long w = w0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (w < w1) {
        const long long b0 = w << 5;
        unsigned mask = 0xffffffffu;
        if (b0 < first) mask &= 0xffffffffu << (unsigned)(first - b0);
        if (b0 + 32 > first + rows) mask &= 0xffffffffu >> (unsigned)(b0 + 32 - (first + rows));
        atomicAnd(bits + w, ~mask);
    }
    if (epoch && blockIdx.x == 0 && threadIdx.x == 0) *epoch += 1u;
}

// bit first + start[i] set for the n starts (each checked against [0, rows) again)
__global__ __launch_bounds__(256) void mocha_path_starts_set(const int32_t* __restrict__ start, int n, long long first, long long rows, unsigned* __restrict__ bits) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long long j = start[i];
    if (j < 0 || j >= rows) return;
    const long long b = first + j;
    atomicOr(bits + (b >> 5), 1u << (b & 31));
}

hipError_t launch_path_starts(unsigned* bits, int64_t n_bits, int64_t first, int64_t rows, const int32_t* start_dev, int n, unsigned* epoch, hipStream_t s) {
    if (!bits || first < 0 || rows < 0 || first + rows > n_bits || n < 0 || (n > 0 && !start_dev)) return hipErrorInvalidValue;
    if (rows > 0 || epoch) {
        const long long words = rows > 0 ? ((first + rows + 31) >> 5) - (first >> 5) : 0;
        hipLaunchKernelGGL(mocha_path_starts_clear, dim3((unsigned)std::max<long long>(1, (words + 255) / 256)), dim3(256), 0, s, bits, (long long)first,
                           (long long)rows, epoch);
    }
    if (n > 0) hipLaunchKernelGGL(mocha_path_starts_set, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, start_dev, n, (long long)first, (long long)rows, bits);
    return hipGetLastError();
}

}  // namespace mocha
