// fp32 GEMM on the bf16 matrix pipe of gfx950: C = epilogue(Aop · W^T) with both operands carried as three bf16 planes.
//
//   x = x0 + x1 + x2,  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1)       (round to nearest even; exact for practically every
//                                                                                       fp32 value, residual <= 2^-24 |x| otherwise)
//   a·b = a0b0 + (a0b1 + a1b0) + (a0b2 + a1b1 + a2b0) + (terms <= 2^-24 |ab|)
//
// Six v_mfma_f32_32x32x16_bf16 (fp32 accumulate, every bf16 x bf16 product exact in fp32) reproduce the fp32 product to the rounding
// of ONE fp32 operation (tests/test_plane_split_numerics.py) - far below what the fp32 accumulation of a K-long dot product rounds
// away, which is the same as in the exact-f32 kernel of gemm_f32.hip; measured against float64 the result is slightly MORE accurate
// than that kernel's (tests/test_gemm_engines.py).  The bf16 pipe runs 16x the fp32 MFMA rate, so six passes cost 0.375 of one v_mfma_f32_32x32x2_f32 pass.
//
// Structure:
//   * 128 x 128 tile per 256-thread workgroup, four waves of 64 x 64; K step 16 (one MFMA k): per step and wave 12 ds_read_b128
//     feed 24 MFMAs, i.e. half a read per MFMA (the LDS array sustains two).
//   * Weights are packed once (mocha_pack_x3) into the image the kernel consumes: [n tile][k step][plane][k half][128 rows][8 bf16],
//     12 KB per (tile, step), fetched straight into LDS by three buffer_load ... lds per thread (no VGPR staging, no ds_write).
//   * Activations stay fp32 in HBM (plain rows, or the temporal-conv gather of kernels.h); a thread fetches two 16-byte pieces per
//     step, splits them into the three planes (v_cvt_pk_bf16_f32 + a subtraction per level) and writes them with ds_write_b64.
//     The split of step s + 1 is interleaved by hand with the MFMAs of step s (two VALU instructions per MFMA, fenced), the fetch of
//     step s + 2 is issued once step s + 1's registers are free, so it has a whole step to land.
//   * Two LDS stages of 25.5 KB, one barrier per step: while step s is multiplied, step s + 1 is written into the other stage.
//     51 KB per workgroup -> three workgroups per CU cover each other's prologues, barriers and epilogues.
//   * LDS image per plane (both operands): [k half][row][8 bf16] - the 16 lanes a ds_read_b128 serves together read 256 contiguous
//     bytes; the halves are 64 bytes further apart than 2 KB so that the b64 plane stores of a 16-lane group (banked mod 32 dwords)
//     cover all banks once.
//   * Two more tile shapes from the same code (template parameters TM, TN): 64 x 128 for mid-size launches (twice the workgroups),
//     128 x 64 for N = 64 / 192 (one 64-row half of a packed block per stage; 44 split instructions over 12 MFMAs).
//   * K split over gridDim.z with raw partial sums per slab (the matcher's 23 040-long contraction).
//   * Operands swapped as in gemm_f32.hip (C^T accumulators), same epilogue: transposition through LDS, whole-line stores.
#include "kernels.h"
#include "device_utils.h"
#include <type_traits>
#include <algorithm>

namespace mocha {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#ifndef X3_MAXSUM
#define X3_MAXSUM 2         // products a_i b_j with i + j <= 2; tools/ builds an ablation with fewer (wrong results, timing only)
#endif
static constexpr int XN = 128, XK = 16;                  // tile width, K step; tile height = 64 TM rows
static constexpr int XA_HALF = 128 * 8 + 32;            // bf16 per k half of an A plane (2 KB + 64 B)
static constexpr int XA_PLANE = 2 * XA_HALF;            // 2176 bf16
static constexpr int XB_PLANE = 128 * 16;               // 2048 bf16, [k half][row][8]
static constexpr int XB_OFF = 3 * XA_PLANE;             // B planes follow the A planes of a stage
static constexpr int X_STAGE = XB_OFF + 3 * XA_PLANE;   // 13 056 bf16 = 26 112 B (the B planes use the padded A layout in LDS)
static constexpr int XW_BLOCK = 3 * XB_PLANE;           // packed weights per (n tile, k step): 6144 bf16 = 12 KB
// tile width 64 TN: the B planes of a stage hold 64 TN rows per k half (TN = 2: the layout above; TN = 1: one 64-row half of a packed block)
template <int TN> struct XT {
    static constexpr int TILE_N = 64 * TN;
    static constexpr int B_HALF = TILE_N * 8 + 32;
    static constexpr int B_PLANE = 2 * B_HALF;
    static constexpr int STAGE = XB_OFF + 3 * B_PLANE;
};
static_assert(XT<2>::STAGE == X_STAGE && XT<2>::B_HALF == XA_HALF, "TN = 2 is the 128-wide layout");

__device__ __forceinline__ float x3_lrelu(float x) { return x > 0.f ? x : 0.2f * x; }
__device__ __forceinline__ float x3_gelu(float x) { return mocha_gelu(x); }

// W [N][K] fp32 -> packed planes.  One workgroup per (n tile, k step) block: thread = (row, k half) reads 32 bytes and writes one
// 16-byte piece per plane, so every wave writes 512-byte runs of the 12 KB block (the image is written once per weight, but once per
// call for the matcher's transient bank).  wsub (K values, may be null) is subtracted from every row first (centred bank).
__global__ __launch_bounds__(256) void mocha_pack_x3(const float* __restrict__ W, const float* __restrict__ wsub, int N, int K, unsigned short* __restrict__ out, int reverse) {
    const int ksteps = K / XK;
    const int bx = reverse ? gridDim.x - 1 - blockIdx.x : blockIdx.x;          // reverse: the blocks, and with them the rows, from the last to the first
    const int nt = bx / ksteps, ks = bx - nt * ksteps;
    const int r = threadIdx.x >> 1, h = threadIdx.x & 1;
    const int n = nt * XN + r;
    const int k = ks * XK + 8 * h;
    f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (n < N) {
        lo = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k);
        hi = *reinterpret_cast<const f32x4*>(W + (size_t)n * K + k + 4);
        if (wsub) {
            lo -= *reinterpret_cast<const f32x4*>(wsub + k);
            hi -= *reinterpret_cast<const f32x4*>(wsub + k + 4);
        }
    }
    u32x2 a[3], b[3];
    plane_split4(lo, a); plane_split4(hi, b);
    unsigned short* blk = out + (size_t)bx * XW_BLOCK;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const u32x4 v = {a[q][0], a[q][1], b[q][0], b[q][1]};
        *reinterpret_cast<u32x4*>(blk + q * XB_PLANE + h * 1024 + r * 8) = v;
    }
}

size_t gemm_x3_packed_elems(int N, int K) { return (size_t)((N + XN - 1) / XN) * (K / XK) * XW_BLOCK; }

hipError_t launch_pack_x3(const float* W, int N, int K, unsigned short* out, hipStream_t s, const float* wsub, int reverse) {
    if (K % XK != 0) return hipErrorInvalidValue;
    const long long blocks = (long long)((N + XN - 1) / XN) * (K / XK);
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_pack_x3, dim3((unsigned)blocks), dim3(256), 0, s, W, wsub, N, K, out, reverse);
    return hipGetLastError();
}

// LRELU: LeakyReLU(0.2) on the activations as they are split; GATHER: temporal-conv gather (kernels.h) instead of plain rows.
// Compile-time so that a K step is one basic block the scheduler can interleave.
// TM: 32-row MFMA blocks per wave: 2 = the 128-row tile; 1 = a 64-row tile (four waves of 32 x 64) for mid-size launches
// (a few dozen to a few hundred windows), where 128-row tiles would leave most workgroup slots empty.
// TN: 32-column MFMA blocks per wave: 2 = the 128-wide tile; 1 = a 128 x 64 tile (waves of 64 x 32) for N = 64 / 192 (to_mot's joint
// block), where a padded 128-wide tile would idle half the pipe.  (A 128 x 256 tile, TN = 4, was measured and not kept:
// tools/experiments/gemm_x3_tile_128x256.patch.txt.)
template <bool LRELU, bool GATHER, int TM, int TN>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void mocha_gemm_x3(GemmParams p) {
    constexpr int TILE_M = TM * 64;
    constexpr int TILE_N = XT<TN>::TILE_N, B_HALF = XT<TN>::B_HALF, B_PLANE = XT<TN>::B_PLANE, STAGE = XT<TN>::STAGE;
    extern __shared__ __attribute__((aligned(16))) unsigned short x3_sm[];          // [2][STAGE]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    const int n_tiles = (p.N + TILE_N - 1) / TILE_N;
    const int m_tiles = (p.M + TILE_M - 1) / TILE_M;
    const int bid = blockIdx.x;
    int mt, nt;
    if (m_tiles >= 8) {                 // XCD-aware order: the n-tiles of one m-tile share an XCD (bid % 8)
        const int grp = bid / (8 * n_tiles);
        const int rem = bid - grp * 8 * n_tiles;
        mt = grp * 8 + (rem & 7);
        nt = rem >> 3;
    } else {
        mt = bid / n_tiles;
        nt = bid - mt * n_tiles;
    }
    if (mt >= m_tiles) return;
    if (p.reverse) mt = m_tiles - 1 - mt;         // GemmParams::reverse: the same workgroup slot, the mirrored row block
    const int m0 = mt * TILE_M, n0 = nt * TILE_N;
    // K split over gridDim.z (the matcher's 23 040-long contraction): this workgroup takes steps s0 .. s0 + nsteps - 1 and writes raw
    // partial sums to slab blockIdx.z; the host guarantees at least two steps per slab
    const int steps_total = p.K / XK;
    const int per = (steps_total + p.ksplit - 1) / p.ksplit;
    const int s0 = blockIdx.z * per;
    const int nsteps = (s0 + per) <= steps_total ? per : steps_total - s0;
#ifdef X3_EXP_STAMPS       // diagnostic build (tools/): cycle stamps per workgroup into the buffer passed as p.wsub
    long long stamp[4];
    stamp[3] = (long long)__builtin_amdgcn_s_memrealtime();      // 100 MHz, common to the chip
    stamp[0] = (long long)__builtin_amdgcn_s_memtime();
#define X3_STAMP(i) stamp[i] = (long long)__builtin_amdgcn_s_memtime()
#define X3_STAMP_OUT() do { if (tid == 0) { long long* d = (long long*)p.wsub + (size_t)bid * 6; d[0] = stamp[0]; d[1] = stamp[1]; d[2] = stamp[2]; d[3] = (long long)__builtin_amdgcn_s_memtime(); d[4] = stamp[3]; d[5] = (long long)__builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define X3_STAMP(i)
#define X3_STAMP_OUT()
#endif

    // ---- A loader: four lanes cover the 64-byte row segment of a step; a thread takes rows lrow and lrow + 64
    const int lrow = tid >> 2;
    const int lc = tid & 3;
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(GATHER ? p.A : p.A + (size_t)(m0 < p.M ? m0 : 0) * p.lda);
    int a_rb[TM], a_t[TM];
    unsigned a_off[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        int m = m0 + lrow + 64 * i;
        m = m < p.M ? m : p.M - 1;
        if (GATHER) {
            const int v = m % p.V;
            const int bt = m / p.V;
            a_t[i] = bt % p.T_out;
            a_rb[i] = (bt / p.T_out) * p.T_src * p.V + v;
            a_off[i] = 0;
        } else {
            a_rb[i] = m; a_t[i] = 0;
            a_off[i] = ((unsigned)(m - m0) * (unsigned)p.lda + lc * 4) * 4u;
        }
    }
    f32x4 rset[2][TM];                              // step t's activations wait in set t & 1, fetched two steps ahead
    auto load_a = [&](int s, f32x4 (&ra)[TM]) __attribute__((always_inline)) {
        const int k0 = (s0 + s) * XK;
        if (!GATHER) {
#pragma unroll
            for (int i = 0; i < TM; ++i) ra[i] = bload(rsA, a_off[i], (unsigned)k0 * 4u);
        } else {
            // the row of tap k0 / Cc, recomputed every step (a handful of VALU instructions hidden between the MFMAs; no branch)
            const int tap = k0 / p.Cc;
            const int cin = k0 - tap * p.Cc;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                int tf = a_t[i] * p.stride + tap * p.tstep - p.pad;
                tf = tf < 0 ? -tf : tf;
                tf = tf >= p.T_full ? 2 * (p.T_full - 1) - tf : tf;
                const unsigned off = ((unsigned)(a_rb[i] + (tf >> p.tshift) * p.V) * (unsigned)p.lda + lc * 4) * 4u;
                ra[i] = bload(rsA, off, (unsigned)cin * 4u);
            }
        }
    };
    // plane q of (row, piece lc): k half lc >> 1, 8 bytes at (lc & 1)
    const int a_wr = (lc >> 1) * XA_HALF + lrow * 8 + (lc & 1) * 4;
    auto split_store = [&](const f32x4 (&ra)[TM], unsigned short* st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            f32x4 v = ra[i];
            if (LRELU) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
            u32x2 pl[3];
            plane_split4(v, pl);
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x2*>(st + q * XA_PLANE + a_wr + i * 64 * 8) = pl[q];
        }
    };
    // ---- W: linear copy of the packed 12 KB block of (nt, step) into the stage
    const int wblock = TN == 1 ? nt >> 1 : nt;           // the packed image is in 128-column blocks; a 64-wide tile takes one half of one
    const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.Wsplit + ((size_t)wblock * steps_total + s0) * XW_BLOCK);
    auto dma_w = [&](int s, unsigned short* st) __attribute__((always_inline)) {
        if (TN == 2) {
#pragma unroll
            for (int j = 0; j < 3; ++j)
                // piece j * 4 + wave of the packed block = (plane, k half, 64-row half): same padded halves as the A planes
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(st + XB_OFF + ((j * 4 + wave) >> 2) * B_PLANE +
                                                         (((j * 4 + wave) >> 1) & 1) * B_HALF + ((j * 4 + wave) & 1) * 512), 16,
                                                         (unsigned)(j * 256 + tid) * 16u, (unsigned)s * (XW_BLOCK * 2u), 0, 0);
        } else {
            // six 1 KB pieces (plane, k half) of this tile's 64-row half: waves 0 and 1 copy two, waves 2 and 3 one
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int pc = j * 4 + wave;                 // (plane, k half) = (pc >> 1, pc & 1)
                if (pc < 6)                                  // wave-uniform
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(st + XB_OFF + (pc >> 1) * B_PLANE + (pc & 1) * B_HALF), 16,
                                                             (unsigned)(((pc >> 1) * 4 + (pc & 1) * 2 + (nt & 1)) * 64 + lane) * 16u, (unsigned)s * (XW_BLOCK * 2u), 0, 0);
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment of lane (row l31, k half hh): 16 bytes
    const int fa = hh * XA_HALF + (wm * TM * 32 + l31) * 8;
    const int fb = XB_OFF + hh * B_HALF + (wn * 32 * TN + l31) * 8;

    // prologue: step 0 into stage 0, step 1's activations into registers.  The counted waits below (and in the steps) rely on the
    // issue order of the copies relative to the register fetches; both are independent loads to the scheduler, so they are fenced.
    load_a(0, rset[0]);
    __builtin_amdgcn_sched_barrier(0);
    dma_w(0, x3_sm);
    __builtin_amdgcn_sched_barrier(0);
    split_store(rset[0], x3_sm);
    load_a(1, rset[1]);                             // K >= 32 (gemm_x3_supports)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(TM) : "memory");     // step 1's TM fetches stay in flight

    // One K step.  FETCH_W: step s + 1 exists (its weights are copied and its activations split into the other stage);
    // FETCH_A: step s + 2 exists (its activations are fetched).  The three variants are straight-line code, so the compiler's own
    // vmcnt bookkeeping for the activation registers is exact: the split waits for the two oldest fetches only, not for the copy.
    auto step = [&](int s, auto parity, auto fetch_w, auto fetch_a) __attribute__((always_inline)) {
        constexpr bool FETCH_W = decltype(fetch_w)::value, FETCH_A = decltype(fetch_a)::value;
        constexpr int P = decltype(parity)::value;      // s & 1
        unsigned short* cur = x3_sm + P * STAGE;
        unsigned short* nxt = x3_sm + (P ^ 1) * STAGE;
        if (FETCH_W) dma_w(s + 1, nxt);             // first thing after the barrier: a whole step to land
        __builtin_amdgcn_sched_barrier(0);          // ... and older than this step's register fetches (counted wait at the end)
        // step s + 2's activations into the set step s's came from (split during step s - 1): a whole step to land, not the
        // few MFMAs left when the fetch waited for step s + 1's registers to be free (the latency was exposed on every step)
        if (FETCH_A) load_a(s + 2, rset[P]);
        __builtin_amdgcn_sched_barrier(0);
        s16x8 a[3][TM], b[3][TN];
        auto rd_a = [&](int q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[q][i] = *reinterpret_cast<const s16x8*>(cur + q * XA_PLANE + fa + i * 32 * 8);
        };
        auto rd_b = [&](int q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TN; ++i) b[q][i] = *reinterpret_cast<const s16x8*>(cur + q * B_PLANE + fb + i * 32 * 8);
        };
        rd_a(0); rd_b(2); rd_a(1); rd_b(1); rd_a(2); rd_b(0);           // in the order the products below consume them
        // Hand-interleaved issue order (fenced so that the scheduler keeps it): after every MFMA two of the 44 VALU instructions that
        // split step s + 1's activations (an MFMA holds the vector issue port for 8 of its 32 cycles), the plane writes as soon as a
        // row's planes are complete, the fetch of step s + 2 when the registers are free.  Low-order products first, a0·b0 last.
        float x[4 * TM];
        unsigned pk[2 * TM][3], hi[2 * TM][2];
        if (FETCH_W) {
#pragma unroll
            for (int e = 0; e < 4 * TM; ++e) { x[e] = rset[P ^ 1][e >> 2][e & 3]; if (LRELU) x[e] = fmaxf(x[e], 0.2f * x[e]); }
        }
        auto split_op = [&](int k) __attribute__((always_inline)) {     // op k of 44: pair k / 11 (two values), step k % 11
            const int pr = k / 11, o = k % 11, lvl = o / 5;
            float& x0 = x[2 * pr]; float& x1 = x[2 * pr + 1];
            if (o == 10) { pk[pr][2] = cvt_pk_bf16(x0, x1); return; }
            switch (o % 5) {
                case 0: pk[pr][lvl] = cvt_pk_bf16(x0, x1); break;
                case 1: hi[pr][0] = pk[pr][lvl] << 16; break;
                case 2: hi[pr][1] = pk[pr][lvl] & 0xffff0000u; break;
                case 3: x0 -= __uint_as_float(hi[pr][0]); break;
                default: x1 -= __uint_as_float(hi[pr][1]); break;
            }
        };
        auto write_row = [&](int i) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const u32x2 v = {pk[2 * i][q], pk[2 * i + 1][q]};
                *reinterpret_cast<u32x2*>(nxt + q * XA_PLANE + a_wr + i * 64 * 8) = v;
            }
        };
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 6 * TM * TN; ++m) {
            const int pr = m / (TM * TN), pa = PLANE_PA[pr], pb = PLANE_PB[pr], i = (m % (TM * TN)) / TN, j = m % TN;
            if (X3_MAXSUM == 2 || pr == 5)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[pb][j], a[pa][i], acc[i][j], 0, 0, 0);       // C^T tile
            if (TN == 2) {                              // 22 TM split instructions over the first 11 TM MFMAs
                if (FETCH_W && m < 11 * TM) { split_op(2 * m); split_op(2 * m + 1); }
                if (FETCH_W && m == 10) write_row(0);
                if (FETCH_W && TM == 2 && m == 21) write_row(1);
            } else if (TM == 1) {                       // TN = 1, TM = 1 (round 5: the 64 x 64 tile of mid-size launches): 22 split instructions over 6 MFMAs
                if (FETCH_W) {
#pragma unroll
                    for (int k = 4 * m; k < 4 * m + 4; ++k)
                        if (k < 22) split_op(k);
                }
                if (FETCH_W && m == 5) write_row(0);
            } else {                                    // TN = 1, TM = 2: 44 split instructions over 11 of the 12 MFMAs
                if (FETCH_W && m < 11) { split_op(4 * m); split_op(4 * m + 1); split_op(4 * m + 2); split_op(4 * m + 3); }
                if (FETCH_W && m == 5) write_row(0);
                if (FETCH_W && m == 10) write_row(1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // the weights of step s + 1 have landed and this wave's plane writes are done; step s + 2's activations stay in flight
        // (__syncthreads() would drain them: its fence waits for vmcnt(0))
        if (FETCH_A) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(TM) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    X3_STAMP(1);
    using T = std::true_type; using F = std::false_type;
    using P0 = std::integral_constant<int, 0>; using P1 = std::integral_constant<int, 1>;
    for (int s = 0; s + 2 < nsteps; s += 2) {           // an even number of steps (gemm_x3_supports)
        step(s, P0{}, T{}, T{});
        step(s + 1, P1{}, T{}, T{});
    }
    step(nsteps - 2, P0{}, T{}, F{});
    step(nsteps - 1, P1{}, F{}, F{});
    X3_STAMP(2);

    // ---- epilogue: as in gemm_f32.hip (acc[i][j] = C^T of MFMA tile (i, j): lane & 31 = row, regs 4g..4g+3 = 4 columns)
    const bool vec_ok = ((p.ldc & 3) == 0) && (!p.residual || (p.ldr & 3) == 0) && ((p.N & 3) == 0);
    float* Cz = p.C + (size_t)blockIdx.z * p.slab_stride;
    const __amdgpu_buffer_rsrc_t rsC = make_rsrc(Cz + (size_t)m0 * p.ldc + n0);
    const __amdgpu_buffer_rsrc_t rsBias = make_rsrc(p.bias ? p.bias + n0 : p.A);
    const __amdgpu_buffer_rsrc_t rsRb = make_rsrc(p.rowbias ? p.rowbias + n0 : p.A);
    const __amdgpu_buffer_rsrc_t rsRes = make_rsrc(p.residual ? p.residual + (size_t)m0 * p.ldr + n0 : p.A);

    if (vec_ok && n0 + TILE_N <= p.N) {
        constexpr int LDP = TILE_N + 4;
        constexpr int C4 = TILE_N / 4;
        static_assert(64 * LDP * 4 <= 2 * STAGE * 2, "epilogue staging fits the operand stages");
        float* stage = reinterpret_cast<float*>(x3_sm);
        // epilogue operands are fetched ahead of their use and ahead of the stores before them (mocha_gemm_x3p's epilogue has the reasoning):
        // the bias quad once per tile, the residual (else the row-bias) rows two store iterations ahead
        static_assert(256 % C4 == 0, "a thread keeps its column quad over the iterations");
        constexpr int NIT = 64 * C4 / 256, RSTEP = 256 / C4;
        const int c4 = tid % C4, r0 = tid / C4;
        const unsigned cb = (unsigned)c4 * 16u;
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        const f32x4 bias4 = p.bias ? bload(rsBias, cb, 0u) : zero4;
        const bool pre_res = p.residual != nullptr, pre_rb = !pre_res && p.rowbias != nullptr;
        f32x4 pre[2];
        auto fetch_pre = [&](int k) __attribute__((always_inline)) {
            const int rloc = 64 * (k / NIT) + r0 + RSTEP * (k % NIT);
            int row = m0 + rloc;
            row = row < p.M ? row : p.M - 1;                                          // rows past M: any valid address, the value is not used
            if (pre_res) pre[k & 1] = bload(rsRes, (unsigned)(row - m0) * (unsigned)p.ldr * 4u + cb, 0u);
            else if (pre_rb) pre[k & 1] = bload(rsRb, (unsigned)(row % p.rb_mod) * (unsigned)p.N * 4u + cb, 0u);
        };
        if (pre_res || pre_rb) { fetch_pre(0); fetch_pre(1); }
        const bool plain_out = !p.bias && !p.rowbias && !p.residual;          // nothing to fetch: read the stage and store (A/B: the pipelined form below costs such launches 5 %)
#pragma unroll
        for (int h = 0; h < TM; ++h) {                // 64 rows of the tile per pass
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int rblk = wm * TM + i;           // this wave's 32-row block of the tile
                if ((rblk >> 1) != h) continue;         // wave-uniform
                float* srow = stage + ((rblk & 1) * 32 + l31) * LDP + wn * (32 * TN) + 4 * hh;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                        *reinterpret_cast<f32x4*>(srow + j * 32 + 8 * g) = v;
                    }
            }
            __syncthreads();
            if (plain_out) {
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int r = r0 + RSTEP * it;
                    const int rloc = 64 * h + r;
                    if (m0 + rloc < p.M) {
                        f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * LDP + c4 * 4);
                        if (p.act == 1) { v = mocha_gelu4(v); }
                        else if (p.act == 2) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
                        else if (p.act == 3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                        bstore(rsC, v, (unsigned)rloc * (unsigned)p.ldc * 4u + cb, 0u);
                    }
                }
            } else
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int r = r0 + RSTEP * it;
                const int rloc = 64 * h + r;
                f32x4 v = *reinterpret_cast<const f32x4*>(stage + r * LDP + c4 * 4) + bias4;
                if (pre_rb) v += pre[(NIT * h + it) & 1];
                else if (p.rowbias) v += bload(rsRb, (unsigned)((m0 + rloc) % p.rb_mod) * (unsigned)p.N * 4u + cb, 0u);   // a residual too: inline (2 GiB window)
                if (p.act == 1) { v = mocha_gelu4(v); }
                else if (p.act == 2) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
                else if (p.act == 3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                if (pre_res) v += pre[(NIT * h + it) & 1];
                if ((pre_res || pre_rb) && NIT * h + it + 2 < NIT * TM) fetch_pre(NIT * h + it + 2);      // ahead of this store
                if (m0 + rloc < p.M) bstore(rsC, v, (unsigned)rloc * (unsigned)p.ldc * 4u + cb, 0u);
            }
            if (h + 1 < TM) __syncthreads();
        }
        X3_STAMP_OUT();
        return;
    }

    // ragged tiles (N not a multiple of 128, unaligned leading dimensions): straight from the accumulators
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int row = m0 + (wm * TM + i) * 32 + l31;
        if (row >= p.M) continue;
        const float* rbrow = p.rowbias ? p.rowbias + (size_t)(row % p.rb_mod) * p.N : nullptr;
        const float* rsrow = p.residual ? p.residual + (size_t)row * p.ldr : nullptr;
        float* crow = Cz + (size_t)row * p.ldc;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c1 = n0 + wn * (32 * TN) + j * 32 + 8 * g + 4 * hh + e;
                    if (c1 >= p.N) continue;
                    float x = acc[i][j][4 * g + e];
                    if (p.bias) x += p.bias[c1];
                    if (rbrow) x += rbrow[c1];
                    if (p.act == 1) x = x3_gelu(x);
                    else if (p.act == 2) x = x3_lrelu(x);
                    else if (p.act == 3) x = fmaxf(x, 0.f);
                    if (rsrow) x += rsrow[c1];
                    crow[c1] = x;
                }
    }
}


// -----------------------------------------------------------------------------------------------------------------------------------
// Persistent instance (round 4): the K loop runs ACROSS tiles.  A workgroup walks tiles t = bid, bid + gridDim.x, ...;
// the last two steps of a tile do for the next tile's steps 0 and 1 exactly what every step does for its successors - fetch its
// activations two steps ahead, copy its weights and split its activations into the other LDS stage one step ahead - so a tile has no
// prologue: when its epilogue is over, step 0's operands are in LDS and step 1's activations in registers.  The epilogue stages the
// accumulators through the ONE stage the last step read from (32 rows per pass instead of 64), the other stage holds the next tile's step 0.
// Same arithmetic, same order per output element: results are bit-identical to mocha_gemm_x3.  128 x 128 tiles, ksplit = 1 only.
// -----------------------------------------------------------------------------------------------------------------------------------
// EPI: which epilogue operand is fetched ahead of the stores - 0 none (bias only), 1 the residual rows, 2 the row-bias rows (no residual)
template <bool LRELU, bool GATHER, int EPI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void mocha_gemm_x3p(GemmParams p) {
    constexpr int TM = 2, TN = 2;
    constexpr int TILE_M = 128, TILE_N = 128, B_HALF = XT<2>::B_HALF, B_PLANE = XT<2>::B_PLANE, STAGE = XT<2>::STAGE;
    extern __shared__ __attribute__((aligned(16))) unsigned short x3_sm[];          // [2][STAGE]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int n_tiles = (p.N + TILE_N - 1) / TILE_N;
    const int m_tiles = (p.M + TILE_M - 1) / TILE_M;
    const int m_pad = m_tiles >= 8 ? (m_tiles + 7) / 8 * 8 : m_tiles;
    const int total = m_pad * n_tiles;
    const int nsteps = p.K / XK;
    const int lrow = tid >> 2, lc = tid & 3;

    // a tile's loader state: base pointers stay uniform (SGPRs), per-lane offsets in a few VGPRs
    struct Tile { int m0, n0; int valid; int a_rb[TM], a_t[TM]; unsigned a_off[TM]; };       // no padding bytes: a bool here made every tile hand-over copy three of them through scratch
    auto make_tile = [&](int t) __attribute__((always_inline)) -> Tile {
        Tile T;
        int mt, nt;
        if (m_tiles >= 8) {                 // XCD-aware order as in mocha_gemm_x3: the n-tiles of one m-tile share an XCD (t % 8; gridDim.x % 8 == 0)
            const int grp = t / (8 * n_tiles);
            const int rem = t - grp * 8 * n_tiles;
            mt = grp * 8 + (rem & 7);
            nt = rem >> 3;
        } else {
            mt = t / n_tiles;
            nt = t - mt * n_tiles;
        }
        T.valid = mt < m_tiles;
        if (p.reverse) mt = m_tiles - 1 - mt;     // GemmParams::reverse: walk step t takes the mirrored row block, so does the successor the last two steps prefetch (padded m-tiles: negative, not valid)
        T.m0 = (T.valid ? mt : 0) * TILE_M; T.n0 = nt * TILE_N;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            int m = T.m0 + lrow + 64 * i;
            m = m < p.M ? m : p.M - 1;
            if (GATHER) {
                const int v = m % p.V;
                const int bt = m / p.V;
                T.a_t[i] = bt % p.T_out;
                T.a_rb[i] = (bt / p.T_out) * p.T_src * p.V + v;
                T.a_off[i] = 0;
            } else {
                T.a_rb[i] = m; T.a_t[i] = 0;
                T.a_off[i] = ((unsigned)(m - T.m0) * (unsigned)p.lda + lc * 4) * 4u;
            }
        }
        return T;
    };
    f32x4 rset[2][TM];
    auto load_a = [&](const Tile& T, int s, f32x4 (&ra)[TM]) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rsA = make_rsrc(GATHER ? p.A : p.A + (size_t)T.m0 * p.lda);
        const int k0 = s * XK;
        if (!GATHER) {
#pragma unroll
            for (int i = 0; i < TM; ++i) ra[i] = bload(rsA, T.a_off[i], (unsigned)k0 * 4u);
        } else {
            const int tap = k0 / p.Cc;
            const int cin = k0 - tap * p.Cc;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                int tf = T.a_t[i] * p.stride + tap * p.tstep - p.pad;
                tf = tf < 0 ? -tf : tf;
                tf = tf >= p.T_full ? 2 * (p.T_full - 1) - tf : tf;
                const unsigned off = ((unsigned)(T.a_rb[i] + (tf >> p.tshift) * p.V) * (unsigned)p.lda + lc * 4) * 4u;
                ra[i] = bload(rsA, off, (unsigned)cin * 4u);
            }
        }
    };
    const int a_wr = (lc >> 1) * XA_HALF + lrow * 8 + (lc & 1) * 4;
    auto split_store = [&](const f32x4 (&ra)[TM], unsigned short* st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            f32x4 v = ra[i];
            if (LRELU) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
            u32x2 pl[3];
            plane_split4(v, pl);
#pragma unroll
            for (int q = 0; q < 3; ++q) *reinterpret_cast<u32x2*>(st + q * XA_PLANE + a_wr + i * 64 * 8) = pl[q];
        }
    };
    auto dma_w = [&](const Tile& T, int s, unsigned short* st) __attribute__((always_inline)) {
        const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.Wsplit + ((size_t)(T.n0 / TILE_N) * nsteps) * XW_BLOCK);
#pragma unroll
        for (int j = 0; j < 3; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (__attribute__((address_space(3))) void*)(st + XB_OFF + ((j * 4 + wave) >> 2) * B_PLANE +
                                                     (((j * 4 + wave) >> 1) & 1) * B_HALF + ((j * 4 + wave) & 1) * 512), 16,
                                                     (unsigned)(j * 256 + tid) * 16u, (unsigned)s * (XW_BLOCK * 2u), 0, 0);
    };

    f32x16 acc[TM][TN];
    const int fa = hh * XA_HALF + (wm * TM * 32 + l31) * 8;
    const int fb = XB_OFF + hh * B_HALF + (wn * 32 * TN + l31) * 8;

    // One K step of tile `cur`.  FETCH_W: the step after this one exists - step s + 1 of this tile, or step 0 of the next tile (wt / ws) - its
    // weights are copied and its activations (waiting in rset[P ^ 1]) split into the other stage; FETCH_A: the step after that exists
    // (at / as) - its activations are fetched into rset[P].
    auto step = [&](auto parity, auto fetch_w, auto fetch_a, const Tile& wt, int ws, const Tile& at, int as) __attribute__((always_inline)) {
        constexpr bool FETCH_W = decltype(fetch_w)::value, FETCH_A = decltype(fetch_a)::value;
        constexpr int P = decltype(parity)::value;
        unsigned short* cur = x3_sm + P * STAGE;
        unsigned short* nxt = x3_sm + (P ^ 1) * STAGE;
        if (FETCH_W) dma_w(wt, ws, nxt);
        __builtin_amdgcn_sched_barrier(0);
        if (FETCH_A) load_a(at, as, rset[P]);
        __builtin_amdgcn_sched_barrier(0);
        s16x8 a[3][TM], b[3][TN];
        auto rd_a = [&](int q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TM; ++i) a[q][i] = *reinterpret_cast<const s16x8*>(cur + q * XA_PLANE + fa + i * 32 * 8);
        };
        auto rd_b = [&](int q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < TN; ++i) b[q][i] = *reinterpret_cast<const s16x8*>(cur + q * B_PLANE + fb + i * 32 * 8);
        };
        rd_a(0); rd_b(2); rd_a(1); rd_b(1); rd_a(2); rd_b(0);
        float x[4 * TM];
        unsigned pk[2 * TM][3], hi[2 * TM][2];
        if (FETCH_W) {
#pragma unroll
            for (int e = 0; e < 4 * TM; ++e) { x[e] = rset[P ^ 1][e >> 2][e & 3]; if (LRELU) x[e] = fmaxf(x[e], 0.2f * x[e]); }
        }
        auto split_op = [&](int k) __attribute__((always_inline)) {
            const int pr = k / 11, o = k % 11, lvl = o / 5;
            float& x0 = x[2 * pr]; float& x1 = x[2 * pr + 1];
            if (o == 10) { pk[pr][2] = cvt_pk_bf16(x0, x1); return; }
            switch (o % 5) {
                case 0: pk[pr][lvl] = cvt_pk_bf16(x0, x1); break;
                case 1: hi[pr][0] = pk[pr][lvl] << 16; break;
                case 2: hi[pr][1] = pk[pr][lvl] & 0xffff0000u; break;
                case 3: x0 -= __uint_as_float(hi[pr][0]); break;
                default: x1 -= __uint_as_float(hi[pr][1]); break;
            }
        };
        auto write_row = [&](int i) __attribute__((always_inline)) {
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const u32x2 v = {pk[2 * i][q], pk[2 * i + 1][q]};
                *reinterpret_cast<u32x2*>(nxt + q * XA_PLANE + a_wr + i * 64 * 8) = v;
            }
        };
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 6 * TM * TN; ++m) {
            const int pr = m / (TM * TN), pa = PLANE_PA[pr], pb = PLANE_PB[pr], i = (m % (TM * TN)) / TN, j = m % TN;
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[pb][j], a[pa][i], acc[i][j], 0, 0, 0);
            if (FETCH_W && m < 11 * TM) { split_op(2 * m); split_op(2 * m + 1); }
            if (FETCH_W && m == 10) write_row(0);
            if (FETCH_W && m == 21) write_row(1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (FETCH_A) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(TM) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    using TT = std::true_type;
    using P0 = std::integral_constant<int, 0>; using P1 = std::integral_constant<int, 1>;

    int t = blockIdx.x;
    if (t >= total) return;
    Tile cur = make_tile(t);
    while (!cur.valid) { t += gridDim.x; if (t >= total) return; cur = make_tile(t); }          // padded m-tiles of the XCD-aware order
    // the first tile's prologue (as in mocha_gemm_x3)
    load_a(cur, 0, rset[0]);
    __builtin_amdgcn_sched_barrier(0);
    dma_w(cur, 0, x3_sm);
    __builtin_amdgcn_sched_barrier(0);
    split_store(rset[0], x3_sm);
    load_a(cur, 1, rset[1]);
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(TM) : "memory");

    const bool vec_ok = ((p.ldc & 3) == 0) && (!p.residual || (p.ldr & 3) == 0) && ((p.N & 3) == 0);
    for (;;) {
        int tn = t + gridDim.x;
        Tile nxt = cur;
        bool has_next = false;
        while (tn < total) { nxt = make_tile(tn); if (nxt.valid) { has_next = true; break; } tn += gridDim.x; }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        for (int s = 0; s + 2 < nsteps; s += 2) {
            step(P0{}, TT{}, TT{}, cur, s + 1, cur, s + 2);
            step(P1{}, TT{}, TT{}, cur, s + 2, cur, s + 3);
        }
        // (the last tile of a workgroup prepares `cur` once more: the fetches stay inside the tile's buffers and nobody reads them)
        step(P0{}, TT{}, TT{}, cur, nsteps - 1, nxt, 0);              // next tile's step 0 activations into rset[0]
        step(P1{}, TT{}, TT{}, nxt, 0, nxt, 1);                       // its step 0 into stage 0, its step 1 activations into rset[1]

        // ---- epilogue of `cur` through stage 1 (the last step's operands are dead; stage 0 may hold the next tile's step 0): 32 rows per pass
        const int m0 = cur.m0, n0 = cur.n0;
        float* Cz = p.C;
        const __amdgpu_buffer_rsrc_t rsC = make_rsrc(Cz + (size_t)m0 * p.ldc + n0);
        const __amdgpu_buffer_rsrc_t rsBias = make_rsrc(p.bias ? p.bias + n0 : p.A);
        const __amdgpu_buffer_rsrc_t rsRb = make_rsrc(p.rowbias ? p.rowbias + n0 : p.A);
        const __amdgpu_buffer_rsrc_t rsRes = make_rsrc(p.residual ? p.residual + (size_t)m0 * p.ldr + n0 : p.A);
        if (vec_ok && n0 + TILE_N <= p.N) {
            constexpr int LDP = TILE_N + 4;
            constexpr int C4 = TILE_N / 4;
            static_assert(32 * LDP * 4 <= STAGE * 2, "a 32-row pass fits one stage");
            float* stage = reinterpret_cast<float*>(x3_sm + STAGE);
            // the epilogue's per-thread offsets do not depend on the tile: left alone, the compiler hoists all of them out of the tile loop and
            // keeps ~70 registers alive through the K steps (227 instead of 156 VGPRs: two waves per SIMD).  Derive them from a laundered
            // thread id so that they are recomputed here.
            int te = tid, l31e = l31, hhe = hh;
            asm volatile("" : "+v"(te), "+v"(l31e), "+v"(hhe));
            // Epilogue operands from global memory are fetched AHEAD of their use and ahead of the previous pass's stores: the vector-memory
            // counter retires in order, so a load issued after a store cannot be waited for without waiting for that store's acknowledgement
            // (the first build loaded bias and residual inside each of the 16 store iterations of a tile: 16 serial round trips, each behind
            // the previous store).  A thread's column quad is the same in every iteration (C4 = 32 divides 256): the bias is loaded once per
            // tile; `pre` holds the residual rows (or the row-bias rows where there is no residual) of the NEXT 32-row pass.
            static_assert(256 % C4 == 0, "a thread keeps its column quad over the iterations");
            constexpr int NIT = 32 * C4 / 256;
            const int c4 = te % C4, r0 = te / C4;
            const unsigned cb = (unsigned)c4 * 16u;
            const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
            const f32x4 bias4 = p.bias ? bload(rsBias, cb, 0u) : zero4;
            f32x4 pre[EPI ? 2 : 1];                              // the operand of store iterations k and k + 1 (k = 4 h + it), refilled two ahead
            auto fetch_pre = [&](int k) __attribute__((always_inline)) {
                const int rloc = 32 * (k / NIT) + r0 + (256 / C4) * (k % NIT);
                int row = m0 + rloc;
                row = row < p.M ? row : p.M - 1;                                      // rows past M: any valid address, the value is not used
                if constexpr (EPI == 1) pre[k & 1] = bload(rsRes, (unsigned)(row - m0) * (unsigned)p.ldr * 4u + cb, 0u);
                else if constexpr (EPI == 2) pre[k & 1] = bload(rsRb, (unsigned)(row % p.rb_mod) * (unsigned)p.N * 4u + cb, 0u);
            };
            if constexpr (EPI != 0) { fetch_pre(0); fetch_pre(1); }
#pragma unroll
            for (int h = 0; h < 2 * TM; ++h) {            // 32 rows of the tile per pass: MFMA row block h
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    if (wm * TM + i != h) continue;         // wave-uniform: the two waves that own row block h
                    float* srow = stage + l31e * LDP + wn * (32 * TN) + 4 * hhe;
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                            *reinterpret_cast<f32x4*>(srow + j * 32 + 8 * g) = v;
                        }
                }
                __syncthreads();
                if (EPI == 0 && !p.bias) {                  // nothing to fetch: read the stage and store (A/B: the pipelined form costs such launches 5 %)
#pragma unroll
                    for (int it = 0; it < NIT; ++it) {
                        const int rloc = 32 * h + r0 + (256 / C4) * it;
                        if (m0 + rloc < p.M) {
                            f32x4 v = *reinterpret_cast<const f32x4*>(stage + (r0 + (256 / C4) * it) * LDP + c4 * 4);
                            if (p.act == 1) { v = mocha_gelu4(v); }
                            else if (p.act == 2) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
                            else if (p.act == 3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                            bstore(rsC, v, (unsigned)rloc * (unsigned)p.ldc * 4u + cb, 0u);
                        }
                    }
                } else
#pragma unroll
                for (int it = 0; it < NIT; ++it) {         // one store iteration at a time: few live registers
                    const int rloc = 32 * h + r0 + (256 / C4) * it;
                    f32x4 v = *reinterpret_cast<const f32x4*>(stage + (r0 + (256 / C4) * it) * LDP + c4 * 4) + bias4;
                    if constexpr (EPI == 2) v += pre[(NIT * h + it) & 1];
                    else if (EPI == 1 && p.rowbias) v += bload(rsRb, (unsigned)((m0 + rloc) % p.rb_mod) * (unsigned)p.N * 4u + cb, 0u);   // a residual too: inline (2 GiB window)
                    if (p.act == 1) { v = mocha_gelu4(v); }
                    else if (p.act == 2) { v[0] = x3_lrelu(v[0]); v[1] = x3_lrelu(v[1]); v[2] = x3_lrelu(v[2]); v[3] = x3_lrelu(v[3]); }
                    else if (p.act == 3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
                    if constexpr (EPI == 1) v += pre[(NIT * h + it) & 1];
                    if constexpr (EPI != 0) { if (NIT * h + it + 2 < NIT * 2 * TM) fetch_pre(NIT * h + it + 2); }      // ahead of this store
                    if (m0 + rloc < p.M) bstore(rsC, v, (unsigned)rloc * (unsigned)p.ldc * 4u + cb, 0u);
                }
                __syncthreads();                          // the stage is rewritten by the next pass - or by the next tile's step 0
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = m0 + (wm * TM + i) * 32 + l31;
                if (row >= p.M) continue;
                const float* rbrow = p.rowbias ? p.rowbias + (size_t)(row % p.rb_mod) * p.N : nullptr;
                const float* rsrow = p.residual ? p.residual + (size_t)row * p.ldr : nullptr;
                float* crow = Cz + (size_t)row * p.ldc;
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int c1 = n0 + wn * (32 * TN) + j * 32 + 8 * g + 4 * hh + e;
                            if (c1 >= p.N) continue;
                            float x = acc[i][j][4 * g + e];
                            if (p.bias) x += p.bias[c1];
                            if (rbrow) x += rbrow[c1];
                            if (p.act == 1) x = x3_gelu(x);
                            else if (p.act == 2) x = x3_lrelu(x);
                            else if (p.act == 3) x = fmaxf(x, 0.f);
                            if (rsrow) x += rsrow[c1];
                            crow[c1] = x;
                        }
            }
        }
        if (!has_next) break;
        cur = nxt; t = tn;
    }
}

template <int TN> static constexpr size_t x3_lds_bytes() { return (size_t)2 * XT<TN>::STAGE * sizeof(unsigned short); }

template <bool L, bool G, int TM, int TN>
static hipError_t x3_attr() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3<L, G, TM, TN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<TN>());
}

hipError_t gemm_x3_init() {
    hipError_t e = x3_attr<false, false, 2, 2>();
    if (e == hipSuccess) e = x3_attr<true, false, 2, 2>();
    if (e == hipSuccess) e = x3_attr<false, true, 2, 2>();
    if (e == hipSuccess) e = x3_attr<true, true, 2, 2>();
    if (e == hipSuccess) e = x3_attr<false, false, 1, 2>();
    if (e == hipSuccess) e = x3_attr<true, false, 1, 2>();
    if (e == hipSuccess) e = x3_attr<false, true, 1, 2>();
    if (e == hipSuccess) e = x3_attr<true, true, 1, 2>();
    if (e == hipSuccess) e = x3_attr<false, false, 2, 1>();
    if (e == hipSuccess) e = x3_attr<true, false, 2, 1>();
    if (e == hipSuccess) e = x3_attr<false, true, 2, 1>();
    if (e == hipSuccess) e = x3_attr<true, true, 2, 1>();
    if (e == hipSuccess) e = x3_attr<false, false, 1, 1>();
    if (e == hipSuccess) e = x3_attr<true, false, 1, 1>();
    if (e == hipSuccess) e = x3_attr<false, true, 1, 1>();
    if (e == hipSuccess) e = x3_attr<true, true, 1, 1>();
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, false, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, false, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, false, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, false, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, true, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, true, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<false, true, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, true, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, true, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_gemm_x3p<true, true, 2>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)x3_lds_bytes<2>());
    return e;
}

// The 64 x 64 tile (round 5): four waves of 32 x 32, six MFMAs per wave and K step.
//  * mid-size launches whose width is a multiple of 64 but not of 128 (to_mot's joint block, N = 192, at a few dozen to a few hundred
//    windows) take it ALWAYS: their alternative was the exact-f32 engine (128 windows: 18.7 -> 13.4 us);
//  * mid-size launches of 128-multiples take it when they have fewer 64 x 128 tiles than p.tile64_below (option "gemm_tile64_below",
//    default 0 = never): measured NO gain - 128 windows, N = 256: K = 512 26.8 -> 27.5 us, K = 1024 47.2 -> 49.6 us; the whole 128-window
//    step 1.116 -> 1.150 ms (profiles/r05/c_tile64.txt) - a mid-size launch's time is its tiles' serial K loop, and a K step's floor
//    (barrier, LDS round trip, the activation split) does not shrink with the tile.
static bool x3_tile64(const GemmParams& p) {
    if (p.ksplit > 1 || p.N % 64 != 0 || !gemm_is_small(p)) return false;
    if (p.N % XN != 0) return true;
    const long long t64x128 = (long long)((p.M + 63) / 64) * ((p.N + 127) / 128);
    return t64x128 < p.tile64_below;
}

// shapes this engine takes; everything else stays on the exact-f32 kernels
bool gemm_x3_supports(const GemmParams& p) {
#ifndef X3_EXP_STAMPS
    if (p.wsub) return false;
#endif
    if (p.K % (2 * XK) != 0) return false;          // an even number of K steps (the register sets alternate)
    if (p.gather && (p.R != 1 || p.Cc % XK != 0)) return false;
    if (p.ksplit > 1) {
        // raw partial sums (the matcher): no epilogue operands, every K slab at least two steps, the 2 GiB window of the weight image
        if (p.bias || p.rowbias || p.residual || p.act || p.gather) return false;
        const int total = p.K / XK, per = (total + p.ksplit - 1) / p.ksplit;
        if ((per & 1) || total - (p.ksplit - 1) * per < 2 || ((total - (p.ksplit - 1) * per) & 1)) return false;   // every slab: an even number of steps, at least two
        return (long long)total * XW_BLOCK * 2 < (1ll << 31);
    }
    if (p.N % 64 != 0) return false;
    // N = 64 / 192 (to_mot's joint block): the 128 x 64 tile serves large launches, the 64 x 64 tile (round 5) the mid-size ones it is enabled for
    if (p.N % XN != 0 && gemm_is_small(p) && !x3_tile64(p)) return false;
    if (gemm_is_skinny(p)) return false;            // a handful of windows: latency-bound, mocha_gemm_skinny
    return true;
}

template <int TM, int TN>
static void x3_launch(const GemmParams& p, hipStream_t s) {
    const int m_tiles = (p.M + TM * 64 - 1) / (TM * 64);
    const int m_pad = m_tiles >= 8 ? (m_tiles + 7) / 8 * 8 : m_tiles;
    const dim3 grid(m_pad * ((p.N + 64 * TN - 1) / (64 * TN)), 1, p.ksplit > 1 ? p.ksplit : 1);
    if (p.a_lrelu) {
        if (p.gather) hipLaunchKernelGGL((mocha_gemm_x3<true, true, TM, TN>), grid, dim3(256), x3_lds_bytes<TN>(), s, p);
        else hipLaunchKernelGGL((mocha_gemm_x3<true, false, TM, TN>), grid, dim3(256), x3_lds_bytes<TN>(), s, p);
    } else {
        if (p.gather) hipLaunchKernelGGL((mocha_gemm_x3<false, true, TM, TN>), grid, dim3(256), x3_lds_bytes<TN>(), s, p);
        else hipLaunchKernelGGL((mocha_gemm_x3<false, false, TM, TN>), grid, dim3(256), x3_lds_bytes<TN>(), s, p);
    }
}

// Default: 768 workgroups (three per CU) walk the tiles of launches up to 512 columns wide - out_proj / ff1 / ff2 / the embedding and to_mot
// GEMMs 2-3 % faster, demo step 5.59 against 5.62 ms; the 1536-wide qkv projection is 5 % SLOWER that way and stays on mocha_gemm_x3
// (profiles/r04/d_persist_ab.txt, d_persist_selective_ab.txt)
// GemmParams::persistent (workgroups, a multiple of 8; 0 = never) / persistent_max_n: per context, options "gemm_persistent[_max_n]"

hipError_t launch_gemm_x3(const GemmParams& p, hipStream_t s) {
    if (p.M <= 0 || p.N <= 0) return hipSuccess;
    if (!p.Wsplit || !gemm_x3_supports(p)) return hipErrorInvalidValue;
    if (p.gather && (long long)p.M / p.T_out * p.T_src * p.lda * 4 >= (1ll << 31)) return hipErrorInvalidValue;
    if (128ll * p.lda * 4 >= (1ll << 31)) return hipErrorInvalidValue;
    // mid-size launches (fewer than 768 tiles of 128 x 64: a few dozen to a few hundred windows) take 64-row tiles, twice the workgroups;
    // N = 64 / 192 the 64-wide tile
    if (p.persistent > 0 && p.ksplit <= 1 && p.N % XN == 0 && p.N <= p.persistent_max_n && !gemm_is_small(p)) {
        // the persistent instance: p.persistent workgroups (a multiple of 8) walk the 128 x 128 tiles
        const int m_tiles = (p.M + 127) / 128, m_pad = m_tiles >= 8 ? (m_tiles + 7) / 8 * 8 : m_tiles;
        const long long total = (long long)m_pad * (p.N / XN);
        const unsigned grid = (unsigned)std::min<long long>(total, p.persistent);
        const int epi = p.residual ? 1 : p.rowbias ? 2 : 0;
#define X3P_LAUNCH(L, G)                                                                                                                  \
        do {                                                                                                                              \
            if (epi == 1) hipLaunchKernelGGL((mocha_gemm_x3p<L, G, 1>), dim3(grid), dim3(256), x3_lds_bytes<2>(), s, p);                 \
            else if (epi == 2) hipLaunchKernelGGL((mocha_gemm_x3p<L, G, 2>), dim3(grid), dim3(256), x3_lds_bytes<2>(), s, p);            \
            else hipLaunchKernelGGL((mocha_gemm_x3p<L, G, 0>), dim3(grid), dim3(256), x3_lds_bytes<2>(), s, p);                          \
        } while (0)
        if (p.a_lrelu) { if (p.gather) X3P_LAUNCH(true, true); else X3P_LAUNCH(true, false); }
        else { if (p.gather) X3P_LAUNCH(false, true); else X3P_LAUNCH(false, false); }
#undef X3P_LAUNCH
        return hipGetLastError();
    }
    if (x3_tile64(p)) x3_launch<1, 1>(p, s);
    else if (p.ksplit <= 1 && p.N % XN != 0) x3_launch<2, 1>(p, s);
    else if (p.ksplit <= 1 && gemm_is_small(p)) x3_launch<1, 2>(p, s);
    else x3_launch<2, 2>(p, s);
    return hipGetLastError();
}

}  // namespace mocha
