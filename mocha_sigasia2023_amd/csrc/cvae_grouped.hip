// The CVAE sampler with ONE WEIGHT SET PER GROUP OF ROWS, the set chosen by device data (mocha_cvae_sample_grouped, the grouped live step):
// a launch covers G groups of m consecutive rows, group g takes the weights of slot which[g] of a bank of Cw slots, and stored[slot] says
// whether that slot holds weights.  A group whose slot is outside [0, Cw) or not stored is INVALID: no weight, bias or residual of it is
// read and its output rows are written as zeros.  which / stored are read by every launch, so a captured graph follows them.
//
//  mocha_gemm_grouped           C[g] = act(A[g] W[slot]^T + bias[slot]) (+ R[g]), exact fp32 on v_mfma_f32_16x16x4_f32.  The structure of
//                               mocha_gemm_skinny16 (gemm_f32.hip): a 256-thread workgroup owns a 16 x 16 output tile, its four waves split K
//                               four ways, every load of a wave's K quarter is issued before its first MFMA, the four partial tiles are summed
//                               through LDS in a fixed order, fused epilogue.  Row tiles are cut PER GROUP (ceil(m / 16) per group, the last
//                               one partial), so a tile never needs two weight sets; the grid is (N / 16) x G x ceil(m / 16).
//                               The summation order of an output element is a function of K alone (which k groups a wave owns, the two
//                               alternating accumulators, the order of the four partial sums): a group's output is the same bits wherever
//                               it sits in whatever batch.  A group's weights are read once per 16 rows.
//  mocha_layernorm256_grouped   mocha_layernorm256 with weight / bias of the row's group's slot
//  mocha_cvae_prior_tokens_grouped   mocha_cvae_prior_tokens with mu_token / logvar_token of the clip's slot (the positional table is shared)
//
// Every store is a plain 16-byte vector store of a row the launch owns: nothing outside [C, C + G m ldc) is written.
#include "kernels.h"
#include "device_utils.h"

namespace mocha {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the slot of group g, or -1 for an invalid group (stored[] is only read for a slot inside the bank)
__device__ __forceinline__ int grouped_slot(const int32_t* __restrict__ which, const int32_t* __restrict__ stored, int Cw, int g) {
    const int slot = which[g];
    if (slot < 0 || slot >= Cw) return -1;
    return stored[slot] != 0 ? slot : -1;
}

//   lane l: A row m0 + (l & 15) of the group, W row n0 + (l & 15) of the slot, k sub-block l >> 4 (4 consecutive k per 16-byte load: element i
//   feeds MFMA i of the k group, the same k permutation on both operands);  acc[r] = C[m0 + (l & 15)][n0 + 4 (l >> 4) + r]  (W as the "A" operand).
__global__ __launch_bounds__(256) void mocha_gemm_grouped(GroupedGemmParams p) {
    __shared__ f32x4 red[3][64];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, kq = lane >> 4;
    const int n_tiles = p.N >> 4;
    const int tpg = (p.m + 15) >> 4;                // row tiles per group
    const int tile = blockIdx.x / n_tiles, nt = blockIdx.x - tile * n_tiles;
    const int g = tile / tpg, rt = tile - g * tpg;
    const int m0 = rt * 16, n0 = nt * 16;           // m0: row of the GROUP
    const int row = m0 + l15, col = n0 + 4 * kq;
    const size_t grow0 = (size_t)g * p.m;           // the group's first row of A / C / R

    const int slot = grouped_slot(p.which, p.stored, p.Cw, g);      // workgroup-uniform
    if (slot < 0) {
        if (wave == 0 && row < p.m) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(p.C + (grow0 + row) * p.ldc + col) = z;
        }
        return;
    }

    const int rowc = row < p.m ? row : p.m - 1;     // a partial tile's spare lanes re-read the group's last row
    const __amdgpu_buffer_rsrc_t rsA = make_rsrc(p.A + (grow0 + m0) * p.lda);
    const __amdgpu_buffer_rsrc_t rsW = make_rsrc(p.W + (size_t)slot * p.w_stride + (size_t)n0 * p.K);
    const unsigned a_off = ((unsigned)(rowc - m0) * (unsigned)p.lda + 4u * kq) * 4u;
    const unsigned w_off = ((unsigned)l15 * (unsigned)p.K + 4u * kq) * 4u;

    const int groups = p.K / 16;                    // k groups of 16 (4 per lane quarter)
    const int gper = (groups + 3) / 4;
    const int g_begin = wave * gper;
    const int g_end = (g_begin + gper) < groups ? (g_begin + gper) : groups;

    // epilogue operands of the wave that will use them, fetched before the K loop (their round trip hides under it)
    f32x4 ebias = {0.f, 0.f, 0.f, 0.f}, eres = {0.f, 0.f, 0.f, 0.f};
    if (wave == 0 && row < p.m) {
        if (p.bias) ebias = *reinterpret_cast<const f32x4*>(p.bias + (size_t)slot * p.b_stride + col);
        if (p.residual) eres = *reinterpret_cast<const f32x4*>(p.residual + (grow0 + row) * p.ldr + col);
    }

    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    constexpr int GMAX = 16;                        // k groups in flight per round: 2 x 16 x 16 B per lane (128 VGPRs)
    for (int g0 = g_begin; g0 < g_end; g0 += GMAX) {
        f32x4 a4[GMAX], b4[GMAX];
#pragma unroll
        for (int i = 0; i < GMAX; ++i) {
            const int kb = (g0 + i) * 16;            // wave-uniform
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            a4[i] = z; b4[i] = z;
            if (g0 + i < g_end) {
                a4[i] = bload(rsA, a_off, (unsigned)kb * 4u);
                b4[i] = bload(rsW, w_off, (unsigned)kb * 4u);
            }
        }
#pragma unroll
        for (int i = 0; i < GMAX; ++i) {
            if (g0 + i < g_end) {                   // wave-uniform
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[i][0], a4[i][0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[i][1], a4[i][1], acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[i][2], a4[i][2], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(b4[i][3], a4[i][3], acc1, 0, 0, 0);
            }
        }
    }
    f32x4 acc = acc0 + acc1;
    if (wave > 0) red[wave - 1][lane] = acc;
    __syncthreads();
    if (wave > 0) return;
    acc = ((acc + red[0][lane]) + red[1][lane]) + red[2][lane];
    if (row >= p.m) return;
    f32x4 v = acc + ebias;
    if (p.act == 3) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
    v += eres;
    *reinterpret_cast<f32x4*>(p.C + (grow0 + row) * p.ldc + col) = v;
}

hipError_t launch_gemm_grouped(const GroupedGemmParams& p, hipStream_t s) {
    if (!p.A || !p.W || !p.C || !p.which || !p.stored) return hipErrorInvalidValue;
    if (p.G < 0 || p.m < 1 || p.N < 16 || p.K < 16 || p.N % 16 != 0 || p.K % 16 != 0 || p.Cw < 1) return hipErrorInvalidValue;
    if (p.act != 0 && p.act != 3) return hipErrorInvalidValue;
    // 16-byte accesses at row * ld + 4 c floats; a row may not overlap the next one
    if (p.lda < p.K || p.ldc < p.N || (p.lda & 3) || (p.ldc & 3) || (p.residual && (p.ldr < p.N || (p.ldr & 3)))) return hipErrorInvalidValue;
    if (p.w_stride < (long long)p.N * p.K || (p.w_stride & 3) || (p.bias && (p.b_stride < p.N || (p.b_stride & 3)))) return hipErrorInvalidValue;
    // 32-bit buffer offsets inside a 16-row tile of A / W
    if (16ll * p.lda * 4 >= (1ll << 31) || 16ll * p.K * 4 >= (1ll << 31)) return hipErrorInvalidValue;
    if (p.G == 0) return hipSuccess;
    const long long tiles = (long long)p.G * ((p.m + 15) / 16) * (p.N / 16);
    if (tiles > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_gemm_grouped, dim3((unsigned)tiles), dim3(256), 0, s, p);
    return hipGetLastError();
}

// nn.LayerNorm(256) as mocha_layernorm256 (cvae.hip), the affine pair of the row's group's slot: w, b = (Cw) vectors `stride` floats apart
__global__ __launch_bounds__(256) void mocha_layernorm256_grouped(const float* __restrict__ x, const float* __restrict__ w,
                                                                  const float* __restrict__ b, long long stride,
                                                                  const int32_t* __restrict__ which, const int32_t* __restrict__ stored, int Cw,
                                                                  float* __restrict__ y, int m, int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int slot = grouped_slot(which, stored, Cw, row / m);      // wave-uniform
    if (slot < 0) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f32x4*>(y + (size_t)row * 256)[lane] = z;
        return;
    }
    const f32x4 v = reinterpret_cast<const f32x4*>(x + (size_t)row * 256)[lane];
    float s = (v[0] + v[1]) + (v[2] + v[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * (1.f / 256.f);
    const f32x4 d = v - mean;
    float q = (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
    const float rstd = 1.f / sqrtf(q * (1.f / 256.f) + 1e-5f);
    const f32x4 wv = reinterpret_cast<const f32x4*>(w + (size_t)slot * stride)[lane], bv = reinterpret_cast<const f32x4*>(b + (size_t)slot * stride)[lane];
    reinterpret_cast<f32x4*>(y + (size_t)row * 256)[lane] = d * rstd * wv + bv;
}

hipError_t launch_layernorm256_grouped(const float* x, const float* w, const float* b, long long stride, const int32_t* which,
                                       const int32_t* stored, int Cw, float* y, int G, int m, hipStream_t s) {
    if (!x || !w || !b || !which || !stored || !y || G < 0 || m < 1 || Cw < 1 || stride < 256 || (stride & 3) || (long long)G * m > 0x7fffffffll)
        return hipErrorInvalidValue;
    if (G == 0) return hipSuccess;
    const int rows = G * m;
    hipLaunchKernelGGL(mocha_layernorm256_grouped, dim3((rows + 3) / 4), dim3(256), 0, s, x, w, b, stride, which, stored, Cw, y, m, rows);
    return hipGetLastError();
}

// PriorNet.encode token assembly as mocha_cvae_prior_tokens (cvae.hip), the two learned tokens of the clip's slot
__global__ __launch_bounds__(256) void mocha_cvae_prior_tokens_grouped(const float* __restrict__ c, const float* __restrict__ mu_tok,
                                                                       const float* __restrict__ lv_tok, long long stride,
                                                                       const int32_t* __restrict__ which, const int32_t* __restrict__ stored,
                                                                       int Cw, const float* __restrict__ pe, float* __restrict__ out, int nc,
                                                                       int rows) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);        // (b, t) flattened; one wave per 256-channel row
    const int q = threadIdx.x & 63;
    if (row >= rows) return;
    const int ntok = nc + 2;
    const int b = row / ntok, t = row - b * ntok;
    const int slot = grouped_slot(which, stored, Cw, b);        // wave-uniform
    if (slot < 0) {
        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f32x4*>(out)[(size_t)row * 64 + q] = z;
        return;
    }
    f32x4 v;
    if (t == 0) v = reinterpret_cast<const f32x4*>(mu_tok + (size_t)slot * stride)[q];
    else if (t == 1) v = reinterpret_cast<const f32x4*>(lv_tok + (size_t)slot * stride)[q];
    else v = reinterpret_cast<const f32x4*>(c)[((size_t)b * nc + (t - 2)) * 64 + q];
    const f32x4 pv = reinterpret_cast<const f32x4*>(pe)[t * 64 + q];
    reinterpret_cast<f32x4*>(out)[(size_t)row * 64 + q] = v + pv;
}

hipError_t launch_cvae_prior_tokens_grouped(const float* c, const float* mu_tok, const float* lv_tok, long long stride, const int32_t* which,
                                            const int32_t* stored, int Cw, const float* pe, float* out, int B, int nc, hipStream_t s) {
    if (!c || !mu_tok || !lv_tok || !which || !stored || !pe || !out || B < 0 || nc < 1 || Cw < 1 || stride < 256 || (stride & 3) ||
        (long long)B * (nc + 2) > 0x7fffffffll)
        return hipErrorInvalidValue;
    if (B == 0) return hipSuccess;
    const int rows = B * (nc + 2);
    hipLaunchKernelGGL(mocha_cvae_prior_tokens_grouped, dim3((rows + 3) / 4), dim3(256), 0, s, c, mu_tok, lv_tok, stride, which, stored, Cw, pe, out,
                       nc, rows);
    return hipGetLastError();
}

// stored[slot] = value, one lane, an ordinary store: the LAST thing mocha_cvae_bank_store enqueues (as mocha_resident_publish)
__global__ __launch_bounds__(64) void mocha_cvae_bank_publish(int32_t* __restrict__ stored, int slot, int value) {
    if (threadIdx.x != 0) return;
    stored[slot] = value;
}

hipError_t launch_cvae_bank_publish(int32_t* stored, int slot, int Cw, int value, hipStream_t s) {
    if (!stored || slot < 0 || slot >= Cw) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_cvae_bank_publish, dim3(1), dim3(64), 0, s, stored, slot, value);
    return hipGetLastError();
}

}  // namespace mocha
