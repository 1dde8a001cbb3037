// The MOTION block of BVH files written on the device (mocha_bvh_format): bvh_pos / bvh_euler (F,V,3) float64, as mocha_postprocess
// leaves them, -> the text the reference's writer emits (motion/bvh.py:210-224): every number as "%f " and a '\n' behind the last space
// of a frame.  The reverse of bvh_parse.hip.
//
// A token is element (frame, column) of a virtual (F, C) matrix gathered from the two arrays (token_value); token t = frame * C + column.
// The clips of a call are concatenated along the frames and their text blocks lie back to back, so the text of the call is ONE run of
// tokens and a clip's block starts at the byte offset of the first token of its first frame.  Lane = token, workgroup = BVHW_BLOCK = 256
// consecutive tokens; rows do not align to workgroups (75 does not divide 256).  The launches, in order (launch_bvh_format):
//   0 mocha_bvhw_count   the bytes of every token (its length by fmt_f6.h, the space, the '\n' of a frame's last column), summed per
//                        workgroup by a wave prefix: counts[block].  The lane of a clip's first token leaves its in-block prefix in
//                        clip_begin[clip].  A refused value (NaN, +-inf, |x| >= 1e12) records its ordinal with atomicMin.
//   1 mocha_bvhw_scan    one workgroup: prefix = exclusive scan of counts, report.bytes = clip_begin[n_clips] = the total, and
//                        clip_begin[c] += prefix[the block of clip c's first token].
//   2 mocha_bvhw_write   every lane converts its token again and writes it, digit by digit, into the workgroup's LDS image at its in-block
//                        prefix.  The image is shifted by (destination address & 3) bytes, so LDS word w and the 4-byte-aligned global
//                        word w hold the same bytes: whole words go out as dwords, the up to three bytes in front of the first whole
//                        word and behind the last as bytes.  Nothing outside [text + prefix[block], text + prefix[block + 1]) is written.
// Conversion: fmt_f6.h - exact integer arithmetic, ties to even, the digit count taken after the rounding carry, the sign from the sign
// bit.  Divisions are by constants only.  No kernel keeps a per-thread array: nothing goes to scratch.  Plain vector stores only.
#include "kernels.h"
#include "fmt_f6.h"

namespace mocha {

namespace {
constexpr int STAGE_WORDS = (BVHW_BLOCK * (BVHW_MAX_TOKEN + 1) + 3 + 3) / 4;      // 256 tokens of at most 21 bytes + '\n', shifted by up to 3

__device__ inline unsigned wave_inclusive(unsigned v, unsigned lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += t;
    }
    return v;
}

// element (frame, col) of the writer's matrix.  save_positions = 0: columns 0..2 the root's position, 3 + 3i + k the angle ax[k] of joint
// visit[i].  save_positions = 1: 6i + k the position (k < 3) or the angle ax[k - 3] of joint visit[i].
__device__ inline double token_value(const BvhwParams& p, unsigned frame, unsigned col) {
    const size_t row = (size_t)frame * (size_t)p.V;
    if (p.save_positions) {
        const unsigned i = col / 6u, k = col % 6u;
        const size_t at = (row + (size_t)p.visit[i]) * 3;
        return k < 3 ? p.pos[at + k] : p.euler[at + (k == 3 ? p.ax[0] : k == 4 ? p.ax[1] : p.ax[2])];
    }
    if (col < 3) return p.pos[row * 3 + col];
    const unsigned i = (col - 3u) / 3u, k = (col - 3u) % 3u;
    return p.euler[(row + (size_t)p.visit[i]) * 3 + (k == 0 ? p.ax[0] : k == 1 ? p.ax[1] : p.ax[2])];
}

// the workgroup's exclusive prefix of n at this lane; *total = the workgroup's sum
__device__ inline unsigned block_exclusive(unsigned n, unsigned tid, unsigned* wave_sum, unsigned* total) {
    const unsigned lane = tid & 63, wave = tid >> 6;
    const unsigned incl = wave_inclusive(n, lane);
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned before = incl - n, all = 0;
    for (unsigned w = 0; w < BVHW_BLOCK / 64; ++w) { if (w < wave) before += wave_sum[w]; all += wave_sum[w]; }
    *total = all;
    return before;
}

__global__ __launch_bounds__(BVHW_BLOCK) void mocha_bvhw_count(BvhwParams p) {
    __shared__ unsigned wave_sum[BVHW_BLOCK / 64];
    const unsigned tid = threadIdx.x, t = blockIdx.x * BVHW_BLOCK + tid;
    unsigned n = 0, frame = 0, col = 0;
    if (t < p.T) {
        frame = t / (unsigned)p.C; col = t - frame * (unsigned)p.C;
        const fmt_f6::Fixed f = fmt_f6::to_fixed(token_value(p, frame, col));
        if (f.len == 0) atomicMin(&p.report->first_bad, (unsigned long long)t);
        n = (unsigned)f.len + 1u + (col + 1u == (unsigned)p.C ? 1u : 0u);
    }
    unsigned total;
    const unsigned before = block_exclusive(n, tid, wave_sum, &total);
    if (tid == 0) p.counts[blockIdx.x] = total;
    if (t < p.T && col == 0) {                                // the first token of a clip?  offsets[c] <= frame < offsets[c + 1]
        int lo = 0, hi = p.n_clips;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned)p.offsets[mid] <= frame) lo = mid; else hi = mid;
        }
        if ((unsigned)p.offsets[lo] == frame) p.clip_begin[lo] = (long long)before;
    }
}

constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void mocha_bvhw_scan(BvhwParams p) {
    __shared__ unsigned wave_sum[SCAN_THREADS / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned per = (p.nblocks + SCAN_THREADS - 1) / SCAN_THREADS;          // consecutive blocks per lane
    const unsigned lo = min(tid * per, p.nblocks), hi = min(lo + per, p.nblocks);
    unsigned mine = 0;
    for (unsigned b = lo; b < hi; ++b) mine += p.counts[b];
    const unsigned incl = wave_inclusive(mine, lane);
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned before = incl - mine;
    for (unsigned w = 0; w < wave; ++w) before += wave_sum[w];
    for (unsigned b = lo; b < hi; ++b) { p.prefix[b] = before; before += p.counts[b]; }
    if (tid == SCAN_THREADS - 1) {
        p.prefix[p.nblocks] = before;
        p.report->bytes = before;
        p.clip_begin[p.n_clips] = (long long)before;
    }
    __syncthreads();                                          // the prefixes are written: a clip adds the one of its first token's block
    for (unsigned c = tid; c < (unsigned)p.n_clips; c += SCAN_THREADS)
        p.clip_begin[c] += (long long)p.prefix[(unsigned)p.offsets[c] * (unsigned)p.C / BVHW_BLOCK];
}

__global__ __launch_bounds__(BVHW_BLOCK) void mocha_bvhw_write(BvhwParams p) {
    __shared__ unsigned stage[STAGE_WORDS];
    __shared__ unsigned wave_sum[BVHW_BLOCK / 64];
    const unsigned tid = threadIdx.x, t = blockIdx.x * BVHW_BLOCK + tid;
    unsigned n = 0;
    bool frame_end = false;
    fmt_f6::Fixed f;
    f.n = 0; f.neg = 0; f.len = 0;
    if (t < p.T) {
        const unsigned frame = t / (unsigned)p.C, col = t - frame * (unsigned)p.C;
        f = fmt_f6::to_fixed(token_value(p, frame, col));
        frame_end = col + 1u == (unsigned)p.C;
        n = (unsigned)f.len + 1u + (frame_end ? 1u : 0u);
    }
    unsigned total;
    const unsigned before = block_exclusive(n, tid, wave_sum, &total);
    const size_t base = p.prefix[blockIdx.x];
    const unsigned shift = (unsigned)(reinterpret_cast<uintptr_t>(p.text + base) & 3u);
    unsigned char* image = reinterpret_cast<unsigned char*>(stage);
    if (t < p.T && f.len) {                                   // (the call does not launch this kernel when a value was refused)
        unsigned char* b = image + shift + before;            // shift + before + n <= 3 + 256 * 22
        fmt_f6::put(f, b);
        b[f.len] = ' ';
        if (frame_end) b[f.len + 1] = '\n';
    }
    __syncthreads();
    // image bytes [shift, end) belong at (text + base - shift)[shift .. end): word w of the image is the aligned global word w
    const unsigned end = shift + total, w0 = (shift + 3u) >> 2, w1 = end >> 2;
    const unsigned head_end = min(w0 * 4u, end), tail_begin = max(w1 * 4u, head_end);
    unsigned char* dst = p.text + base;                       // byte i of the image goes to dst[i - shift]
    unsigned* dst_words = reinterpret_cast<unsigned*>(dst + (w0 * 4u - shift));      // aligned: the global word of image word w0
    for (unsigned w = w0 + tid; w < w1; w += BVHW_BLOCK) dst_words[w - w0] = stage[w];
    if (tid < 3u && shift + tid < head_end) dst[tid] = image[shift + tid];
    if (tid >= 64u && tid < 67u && tail_begin + (tid - 64u) < end) dst[tail_begin + (tid - 64u) - shift] = image[tail_begin + (tid - 64u)];
}
}  // namespace

hipError_t launch_bvh_format(const BvhwParams& p, int launch, hipStream_t s) {
    if (p.T == 0 || p.C < 1 || p.V < 1 || p.n_clips < 1 || p.nblocks != (p.T + BVHW_BLOCK - 1) / BVHW_BLOCK) return hipErrorInvalidValue;
    switch (launch) {
    case 0: hipLaunchKernelGGL(mocha_bvhw_count, dim3(p.nblocks), dim3(BVHW_BLOCK), 0, s, p); break;
    case 1: hipLaunchKernelGGL(mocha_bvhw_scan, dim3(1), dim3(SCAN_THREADS), 0, s, p); break;
    case 2:
        if (!p.text) return hipErrorInvalidValue;
        hipLaunchKernelGGL(mocha_bvhw_write, dim3(p.nblocks), dim3(BVHW_BLOCK), 0, s, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mocha
