// Coherent context matching for clips (include/mocha_hip.h, "coherent context matching"): the matrix of exact distances between Q
// query windows and a range of bank rows, and the jump-penalised minimum-cost path through it.
//
// The reference's 'cm_' branch takes the nearest entry per frame and carries nothing from one frame to the next
// (test_fullframework.py:440-443); its banks are stride-1 windows of smooth clips (collect_CVAE_feature_action.py:119-125), so the right
// answer for consecutive source windows is almost always a run of consecutive bank rows.  The path pays lambda for every transition
// that is not "next row of the same clip".
//
// mocha_match_dist_scan / _unpack: entry (i, j) is bit for bit the distance mocha_match_topk reports for (query i, row j), because it
// comes from the same body (match_stream_body.h, the all-keys mode: 1 280-element chunks, float4 at lane + 64 i, two packed partial
// sums, x + y, the xor butterfly) and the same sqrtf - here with every group of 8 queries in ONE launch (blockIdx.y) instead of a scan
// and a finish launch per group.  A register tile of 16 queries per bank pass (acc[4][16] float2, 80 KB of LDS) was built and measured
// first and lost to this body at two of three shapes (profiles/r23/path_match_tile16.json).
//
// mocha_match_path_forward / _back: one workgroup per sequence, every loop bounded by the sequence's length or by N; no barrier between
// workgroups, no spin.  Thread t owns the c = ceil(N / 1024) columns [t c, (t + 1) c); the relative cost R is float64 in registers.
#include "kernels.h"
#include "match_stream_body.h"

namespace mocha {

static constexpr int MP_ROWS = MS_WAVES * MS_ROWS_PER_WAVE;

// the all-keys scan of match_stream.hip for EVERY group of 8 queries in one launch: blockIdx.y names the group, its keys go to
// keys[(8 y + q) * rows + row]
__global__ __launch_bounds__(256) void mocha_match_dist_scan(const float* __restrict__ bank /*row 0 of the range*/, const float* __restrict__ query,
                                                             int Q, int rows, int D, unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) float qs[8 * MS_CHUNK_F32];
    __shared__ unsigned long long wbest[MS_WAVES][8];
    const int q0 = blockIdx.y * 8;
    const int nq = Q - q0 < 8 ? Q - q0 : 8;
    match_stream_body<8, false>(bank, query + (size_t)q0 * D, nq, (long long)rows, D, keys + (size_t)q0 * rows, 1, nullptr, qs, wbest);
}

// keys -> distances: the square root mocha_match_topk_finish takes of the key's value
__global__ __launch_bounds__(256) void mocha_match_dist_unpack(const unsigned long long* __restrict__ keys, int Q, int rows, float* __restrict__ dist,
                                                               long long ld) {
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= rows || i >= Q) return;
    unsigned u = (unsigned)(keys[(size_t)i * rows + j] >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    dist[(size_t)i * ld + j] = sqrtf(__uint_as_float(u));
}

size_t match_dist_keys_words(int Q, int rows) { return (size_t)Q * rows; }

hipError_t launch_match_dist(const float* bank_rows, const float* query, int Q, int rows, int D, unsigned long long* keys, float* dist, int64_t ld,
                             hipStream_t s) {
    if (Q <= 0) return hipSuccess;
    if (rows < 1 || ld < rows || D % MS_CHUNK_F32 != 0) return hipErrorInvalidValue;
    const unsigned gx = (unsigned)((rows + MP_ROWS - 1) / MP_ROWS);
    for (int q0 = 0; q0 < Q; q0 += 8 * 65535) {          // (the grid's y limit: one launch up to 524 280 queries)
        const int nq = Q - q0 < 8 * 65535 ? Q - q0 : 8 * 65535;
        hipLaunchKernelGGL(mocha_match_dist_scan, dim3(gx, (unsigned)((nq + 7) / 8)), dim3(256), 0, s, bank_rows, query + (size_t)q0 * D, nq, rows, D,
                           keys + (size_t)q0 * rows);
    }
    for (int q0 = 0; q0 < Q; q0 += 65535) {
        const int nq = Q - q0 < 65535 ? Q - q0 : 65535;
        hipLaunchKernelGGL(mocha_match_dist_unpack, dim3((unsigned)((rows + 255) / 256), (unsigned)nq), dim3(256), 0, s, keys + (size_t)q0 * rows, nq,
                           rows, dist + (size_t)q0 * ld, (long long)ld);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// the path
// ---------------------------------------------------------------------------------------------------------------------
static constexpr int MPATH_T = 1024;            // threads at most, and 16-bit words of `cont` per window
static constexpr int MPATH_C = MATCH_PATH_MAX_ROWS / MPATH_T;      // columns a thread owns at most (16)

// one bit per bank row that starts a clip (bits zeroed by the caller)
__global__ void mocha_path_start_bits(const int32_t* __restrict__ start, int n, int N, unsigned* __restrict__ bits) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int j = start[i];
    if (j >= 0 && j < N) atomicOr(bits + (j >> 5), 1u << (j & 31));
}

// Forward pass of sequence blockIdx.x: windows [seq_start[b], seq_start[b + 1]).  m[i] = lowest column of the row minimum of R[i];
// cont[i][t] = thread t's continuation bits of window i (bit k: column t c + k).
__global__ __launch_bounds__(MPATH_T) void mocha_match_path_forward(const float* __restrict__ d, int N, long long ld,
                                                                    const int32_t* __restrict__ seq_start, const unsigned* __restrict__ start_bits,
                                                                    double lambda, int cpt, int32_t* __restrict__ m,
                                                                    unsigned short* __restrict__ cont) {
    __shared__ double edge[2][MPATH_T];          // R of every thread's last column, by step parity
    __shared__ double wmin[2][MPATH_T / 64];
    __shared__ int wcol[2][MPATH_T / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = blockDim.x >> 6;
    const int i0 = seq_start[blockIdx.x], i1 = seq_start[blockIdx.x + 1];
    const int j0 = t * cpt;
    const double INF = __builtin_huge_val();

    unsigned pred = 0;                           // bit k: column j0 + k has a predecessor
#pragma unroll
    for (int k = 0; k < MPATH_C; ++k) {
        const int j = j0 + k;
        if (k < cpt && j < N && j > 0 && !((start_bits[j >> 5] >> (j & 31)) & 1u)) pred |= 1u << k;
    }
    double R[MPATH_C];
    float dn[MPATH_C];
#pragma unroll
    for (int k = 0; k < MPATH_C; ++k) { R[k] = INF; dn[k] = 0.f; }
    if (i0 < i1) {
#pragma unroll
        for (int k = 0; k < MPATH_C; ++k)
            if (k < cpt && j0 + k < N) dn[k] = d[(size_t)i0 * ld + j0 + k];
    }
    double Mprev = 0.0;
    for (int i = i0; i < i1; ++i) {
        const int par = (i - i0) & 1;
        unsigned cbits = 0;
        if (i == i0) {
#pragma unroll
            for (int k = 0; k < MPATH_C; ++k)
                if (k < cpt && j0 + k < N) R[k] = (double)dn[k];
        } else {
            double left = t > 0 ? edge[par ^ 1][t - 1] : INF;      // R[i-1] of column j0 - 1
#pragma unroll
            for (int k = 0; k < MPATH_C; ++k) {
                if (k < cpt && j0 + k < N) {
                    const double a = ((pred >> k) & 1u) ? left - Mprev : INF;
                    const bool c = a < lambda;
                    left = R[k];
                    R[k] = (double)dn[k] + (c ? a : lambda);
                    cbits |= (unsigned)c << k;
                }
            }
        }
        if (i + 1 < i1) {                        // the next row's numbers are on their way while this one is reduced
#pragma unroll
            for (int k = 0; k < MPATH_C; ++k)
                if (k < cpt && j0 + k < N) dn[k] = d[(size_t)(i + 1) * ld + j0 + k];
        }
        double best = INF; int bj = 0x7fffffff;
        double last = INF;
#pragma unroll
        for (int k = 0; k < MPATH_C; ++k)
            if (k < cpt && j0 + k < N) {
                if (R[k] < best) { best = R[k]; bj = j0 + k; }      // ascending columns: the first of equal values stays
                last = R[k];
            }
        edge[par][t] = last;
        cont[(size_t)i * MPATH_T + t] = (unsigned short)cbits;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o);
            const int oj = __shfl_xor(bj, o);
            if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        if (lane == 0) { wmin[par][wave] = best; wcol[par][wave] = bj; }
        __syncthreads();
        best = wmin[par][0]; bj = wcol[par][0];
        for (int w = 1; w < nwaves; ++w) {
            const double ob = wmin[par][w];
            const int oj = wcol[par][w];
            if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
        }
        Mprev = best;
        if (t == 0) m[i] = bj;
    }
}

// Backtrack of sequence blockIdx.x, in a launch of its own (it reads what every thread of the forward pass wrote).  Sequential in
// the sequence's length: one dependent read per window.
__global__ __launch_bounds__(64) void mocha_match_path_back(const float* __restrict__ d, int N, long long ld, const int32_t* __restrict__ seq_start,
                                                            const unsigned* __restrict__ start_bits, int cpt, const int32_t* __restrict__ m,
                                                            const unsigned short* __restrict__ cont, int32_t* __restrict__ path,
                                                            float* __restrict__ dist_out, unsigned char* __restrict__ continued) {
    if (threadIdx.x != 0) return;
    const int i0 = seq_start[blockIdx.x], i1 = seq_start[blockIdx.x + 1];
    int next = -1;                               // path[i + 1]
    for (int i = i1 - 1; i >= i0; --i) {
        int j = m[i];
        if (i + 1 < i1) {
            const int tt = next / cpt, k = next - tt * cpt;
            if ((cont[(size_t)(i + 1) * MPATH_T + tt] >> k) & 1) j = next - 1;
            if (continued) {
                const bool has_pred = next > 0 && !((start_bits[next >> 5] >> (next & 31)) & 1u);
                continued[i + 1] = (unsigned char)(has_pred && next == j + 1);
            }
        }
        j = j < 0 ? 0 : (j >= N ? N - 1 : j);    // (never taken on a finite matrix: the indices stay inside the matrix whatever it holds)
        path[i] = j;
        if (dist_out) dist_out[i] = d[(size_t)i * ld + j];
        next = j;
    }
    if (continued && i0 < i1) continued[i0] = 0;
}

// out[i] = min_j d[i][j]: the unit of a relative jump penalty is the median of these
__global__ __launch_bounds__(256) void mocha_path_rowmin(const float* __restrict__ d, int N, long long ld, float* __restrict__ out) {
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    float v = __builtin_huge_valf();
    for (int j = tid; j < N; j += 256) v = fminf(v, d[(size_t)i * ld + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) out[i] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

hipError_t launch_path_rowmin(const float* d, int Q, int N, int64_t ld, float* out, hipStream_t s) {
    if (Q <= 0) return hipSuccess;
    if (N < 1 || ld < N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_path_rowmin, dim3(Q), dim3(256), 0, s, d, N, (long long)ld, out);
    return hipGetLastError();
}

size_t match_path_bits_words(int N) { return (size_t)(N + 31) / 32; }
size_t match_path_cont_words(int Q) { return (size_t)Q * MPATH_T; }      // 16-bit words

hipError_t launch_match_path(const float* d, int Q, int N, int64_t ld, const int32_t* seq_start_dev, int n_seq, const int32_t* bank_start_dev,
                             int n_b, double lambda, unsigned* start_bits, int32_t* m, unsigned short* cont, int32_t* path, float* dist_out,
                             unsigned char* continued, hipStream_t s) {
    if (Q <= 0 || n_seq <= 0) return hipSuccess;
    if (N < 1 || N > MATCH_PATH_MAX_ROWS || ld < N || !(lambda >= 0.0) || lambda > 1.7976931348623157e308) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(start_bits, 0, match_path_bits_words(N) * sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    if (n_b > 0) hipLaunchKernelGGL(mocha_path_start_bits, dim3((n_b + 255) / 256), dim3(256), 0, s, bank_start_dev, n_b, N, start_bits);
    const int cpt = (N + MPATH_T - 1) / MPATH_T;
    const int threads = (((N + cpt - 1) / cpt) + 63) / 64 * 64;
    hipLaunchKernelGGL(mocha_match_path_forward, dim3(n_seq), dim3(threads), 0, s, d, N, (long long)ld, seq_start_dev, start_bits, lambda, cpt, m,
                       cont);
    hipLaunchKernelGGL(mocha_match_path_back, dim3(n_seq), dim3(64), 0, s, d, N, (long long)ld, seq_start_dev, start_bits, cpt, m, cont, path,
                       dist_out, continued);
    return hipGetLastError();
}

}  // namespace mocha
