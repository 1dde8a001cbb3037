// The MOTION block of BVH files on the device (mocha_bvh_motion): whitespace-separated decimal text -> the rot / pos arrays the
// reference's loader returns (motion/bvh.py:106-123), rounded once to fp32.  The text of all clips of a call is one buffer walked in
// blocks of BVH_BLOCK = 4096 bytes; a clip starts on a block boundary and the bytes between clips are '\n'.
//
// A token is a maximal run of bytes other than space, \t, \r, \n; it STARTS at a non-whitespace byte whose predecessor is whitespace
// (the byte before offset 0 counts as whitespace).  The launches, in order (launch_bvh_parse):
//   0 mocha_bvh_count   workgroup = block, lane = 16 bytes in one 16-byte load: the 16-bit mask of token starts, whose predecessor byte
//                       for a lane's first byte is the byte before it in the text - for lane 0 the last byte of the PREVIOUS block.
//                       counts[block] = the block's token starts.
//   1 mocha_bvh_scan    one workgroup: prefix = exclusive scan of counts, prefix[nblocks] = report.tokens = all tokens.
//   2 mocha_bvh_parse   workgroup = block.  The block and 80 bytes behind it are staged in LDS (a token is at most 64 bytes; 65 bytes
//                       decide that one is longer).  Token starts are compacted to an LDS list by a wave prefix of popcounts and dealt to
//                       the lanes round-robin.  Token t of the block has ordinal k = prefix[block] + t - prefix[first block of its clip]
//                       in its clip (the clip by bisection over the clips' first bytes), hence frame k / C and column k % C.  It starts a
//                       line when only spaces, tabs and \r lie between it and the last '\n' (or the clip's first byte).
//                       Violations record their byte with atomicMin: a token at or behind the clip's end (in a gap), a frame beyond the
//                       clip's, a token that starts a line with k % C != 0 or does not with k % C == 0, a token outside the grammar or
//                       longer than 64 bytes.  Values go out with plain stores, at most one per lane and token.
//   3 mocha_bvh_finish  lane = clip: fewer tokens than frames x C records the clip's end byte.  channels == 3: lane = (frame, output
//                       joint) fills the positions of every joint but the root's from off_out (bvh.py:97).
//   4 mocha_bvh_patch   only with slow tokens: lane = entry of the slow list, whose `at` word now holds the fp32 bits from the host.
//
// Conversion (parse_token): sign, then the significant digits accumulated in a uint64 with leading zeros skipped, and a decimal
// exponent (fractional digits count down, [eE] adds).  At most 15 significant digits (m < 10^15 < 2^53, exact as a double) and a net
// exponent within +-22 (10^22 = 2^22 5^22, 5^22 < 2^53: exact) take the fast path: double(m) * 10^e or double(m) / 10^-e is ONE IEEE
// operation on exact operands, so the float64 is the correctly rounded one Python's float() gives; the cast to fp32 rounds once more, as
// np.float32 does.  Float64 division is IEEE-rounded here (no fast-math); multiplying by a reciprocal instead would round twice.
// Any other token with m != 0 is listed for the host's strtod.  No kernel keeps a per-thread array: nothing goes to scratch.
#include "kernels.h"

namespace mocha {

namespace {
constexpr unsigned NL4 = 0x0a0a0a0au;
constexpr int HALO16 = 5;                                     // 16-byte words staged behind the block

__device__ const double BVH_P10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                       1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

__device__ inline bool is_ws(unsigned c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n'; }

// bit i = byte i of the 16 is whitespace (byte 0 = the low byte of x)
__device__ inline unsigned ws_mask(const uint4 v) {
    unsigned m = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned w = (i >> 2) == 0 ? v.x : (i >> 2) == 1 ? v.y : (i >> 2) == 2 ? v.z : v.w;
        m |= (is_ws((w >> ((i & 3) * 8)) & 0xffu) ? 1u : 0u) << i;
    }
    return m;
}

// the token-start mask of the 16 bytes at byte offset `at`: non-whitespace whose predecessor is whitespace
__device__ inline unsigned start_mask(const BvhParams& p, const uint4 v, long long at) {
    const unsigned w = ws_mask(v);
    const unsigned prev_ws = at == 0 ? 1u : (is_ws(p.text[at - 1]) ? 1u : 0u);      // lane 0: the previous block's last byte
    return ~w & ((w << 1) | prev_ws) & 0xffffu;
}

__device__ inline unsigned wave_inclusive(unsigned v, unsigned lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d);
        if (lane >= (unsigned)d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(256) void mocha_bvh_count(BvhParams p) {
    __shared__ unsigned total;
    const unsigned tid = threadIdx.x;
    if (tid == 0) total = 0;
    __syncthreads();
    const long long at = (long long)blockIdx.x * BVH_BLOCK + tid * 16;
    const uint4 v = reinterpret_cast<const uint4*>(p.text)[(size_t)blockIdx.x * 256 + tid];
    const unsigned n = wave_inclusive(__popc(start_mask(p, v, at)), tid & 63);
    if ((tid & 63) == 63) atomicAdd(&total, n);
    __syncthreads();
    if (tid == 0) p.counts[blockIdx.x] = total;
}

constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void mocha_bvh_scan(BvhParams p) {
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
    if (tid == SCAN_THREADS - 1) { p.prefix[p.nblocks] = before; p.report->tokens = before; }
}

// One token of at most 64 bytes at b[0 .. len): true when it follows the grammar [+-]? (digits [. digits?]? | . digits) ([eE] [+-]? digits)?.
// *fast: the value is *value; otherwise the host converts the token.
__device__ inline bool parse_token(const unsigned char* b, unsigned len, float* value, bool* fast) {
    auto ch = [&](unsigned i) -> unsigned { return i < len ? (unsigned)b[i] : 32u; };
    unsigned i = 0, c = ch(0);
    bool neg = false, digits = false;
    if (c == '+' || c == '-') { neg = c == '-'; c = ch(++i); }
    unsigned long long m = 0;
    int nd = 0, dexp = 0;
    while (c - '0' < 10u) {
        const unsigned d = c - '0';
        digits = true;
        if (m | d) {
            if (nd < 19) m = m * 10 + d; else ++dexp;
            ++nd;
        }
        c = ch(++i);
    }
    if (c == '.') {
        c = ch(++i);
        while (c - '0' < 10u) {
            const unsigned d = c - '0';
            digits = true;
            if (m | d) {
                if (nd < 19) { m = m * 10 + d; --dexp; }
                ++nd;
            } else {
                --dexp;
            }
            c = ch(++i);
        }
    }
    if (!digits) return false;
    if (c == 'e' || c == 'E') {
        c = ch(++i);
        bool eneg = false, edigits = false;
        if (c == '+' || c == '-') { eneg = c == '-'; c = ch(++i); }
        int e = 0;
        while (c - '0' < 10u) { edigits = true; e = min(e * 10 + (int)(c - '0'), 100000); c = ch(++i); }
        if (!edigits) return false;
        dexp += eneg ? -e : e;
    }
    if (i != len) return false;
    double v = 0.0;
    *fast = true;
    if (m != 0) {
        if (nd <= 15 && dexp >= -22 && dexp <= 22)
            v = dexp < 0 ? (double)m / BVH_P10[-dexp] : (double)m * BVH_P10[dexp];
        else
            *fast = false;
    }
    const float f = (float)v;
    *value = neg ? -f : f;
    return true;
}

__global__ __launch_bounds__(256) void mocha_bvh_parse(BvhParams p) {
    __shared__ uint4 stage[256 + HALO16];
    __shared__ unsigned short starts[BVH_BLOCK / 2];          // at most every second byte starts a token
    __shared__ unsigned wave_sum[4];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, block = blockIdx.x;
    const long long base = (long long)block * BVH_BLOCK;
    const uint4* src = reinterpret_cast<const uint4*>(p.text) + (size_t)block * 256;
    const uint4 v = src[tid];
    stage[tid] = v;
    if (tid < HALO16)                                         // nbytes is a multiple of the block: a 16-byte word is inside or outside
        stage[256 + tid] = base + BVH_BLOCK + tid * 16 < p.nbytes ? src[256 + tid] : make_uint4(NL4, NL4, NL4, NL4);
    unsigned mask = start_mask(p, v, base + tid * 16);
    const unsigned n = __popc(mask), incl = wave_inclusive(n, lane);
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    unsigned slot = incl - n, ntok = 0;
    for (unsigned w = 0; w < 4; ++w) { if (w < wave) slot += wave_sum[w]; ntok += wave_sum[w]; }
    while (mask) {
        starts[slot++] = (unsigned short)(tid * 16 + __ffs(mask) - 1);
        mask &= mask - 1;
    }
    __syncthreads();

    int lo = 0, hi = p.C;                                     // the block's clip: begin[c] <= base < begin[c+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.begin[mid] <= base) lo = mid; else hi = mid;
    }
    const int c = lo;
    const long long clip_begin = p.begin[c], clip_end = p.end[c];
    const unsigned k0 = p.prefix[block] - p.prefix[clip_begin / BVH_BLOCK];
    const unsigned frames = (unsigned)(p.offsets[c + 1] - p.offsets[c]);
    const size_t frame0 = (size_t)p.offsets[c];
    const unsigned char* bytes = reinterpret_cast<const unsigned char*>(stage);

    for (unsigned t = tid; t < ntok; t += 256) {
        const unsigned s = starts[t], k = k0 + t, frame = k / (unsigned)p.per_frame, col = k % (unsigned)p.per_frame;
        const long long at = base + s;
        bool line_start = true;                               // only spaces, tabs, \r back to the last '\n' or the clip's first byte
        for (long long q = at - 1; q >= clip_begin; --q) {
            const unsigned ch = q >= base ? bytes[q - base] : p.text[q];
            if (ch == '\n') break;
            if (!is_ws(ch)) { line_start = false; break; }
        }
        unsigned len = 0;
        while (len <= BVH_MAX_TOKEN && !is_ws(bytes[s + len])) ++len;      // s + 64 < 4096 + 80
        float value = 0.f;
        bool fast = true;
        bool ok = at < clip_end && frame < frames && line_start == (col == 0) && len <= BVH_MAX_TOKEN;
        ok = ok && parse_token(bytes + s, len, &value, &fast);
        if (!ok) { atomicMin(&p.report->first_bad, (unsigned long long)at); continue; }
        unsigned j, a;
        bool is_rot;
        if (p.channels == 3) {
            is_rot = col >= 3;
            j = is_rot ? (col - 3) / 3 : 0; a = col % 3;
        } else {
            j = col / 6; a = col % 3; is_rot = col % 6 >= 3;
        }
        const int vo = p.map[j];
        if (vo < 0) continue;
        const size_t dest = ((frame0 + frame) * (size_t)p.v_out + (size_t)vo) * 3 + a;
        if (fast) {
            (is_rot ? p.rot : p.pos)[dest] = value;
        } else {
            const unsigned e = atomicAdd(&p.report->slow, 1u);
            if (e < (unsigned)BVH_MAX_SLOW) p.slow[e] = BvhSlow{(unsigned long long)dest | (is_rot ? 1ull << 63 : 0ull), (unsigned long long)at};
        }
    }
}

__global__ __launch_bounds__(256) void mocha_bvh_finish(BvhParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)p.C) {
        const long long next = i + 1 < (size_t)p.C ? p.begin[i + 1] / BVH_BLOCK : (long long)p.nblocks;
        const unsigned have = p.prefix[next] - p.prefix[p.begin[i] / BVH_BLOCK];
        const unsigned long long want = (unsigned long long)(p.offsets[i + 1] - p.offsets[i]) * (unsigned)p.per_frame;
        if (have < want) atomicMin(&p.report->first_bad, (unsigned long long)p.end[i]);
    }
    if (p.channels == 3 && i < (size_t)p.F * p.v_out) {
        const int vo = (int)(i % p.v_out);
        if (vo != p.root_out)
            for (int a = 0; a < 3; ++a) p.pos[i * 3 + a] = p.off_out[vo * 3 + a];
    }
}

__global__ __launch_bounds__(256) void mocha_bvh_patch(BvhParams p) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned)p.n_patch) return;
    const BvhSlow e = p.slow[i];
    (e.dest >> 63 ? p.rot : p.pos)[e.dest & ~(1ull << 63)] = __uint_as_float((unsigned)e.at);
}
}  // namespace

hipError_t launch_bvh_parse(const BvhParams& p, int launch, hipStream_t s) {
    if (p.nblocks == 0 || p.C <= 0 || p.F <= 0) return hipSuccess;
    if (p.per_frame < 1 || p.v_out < 1 || (p.channels != 3 && p.channels != 6) || p.n_patch < 0 || p.n_patch > BVH_MAX_SLOW)
        return hipErrorInvalidValue;
    switch (launch) {
    case 0: hipLaunchKernelGGL(mocha_bvh_count, dim3(p.nblocks), dim3(256), 0, s, p); break;
    case 1: hipLaunchKernelGGL(mocha_bvh_scan, dim3(1), dim3(SCAN_THREADS), 0, s, p); break;
    case 2: hipLaunchKernelGGL(mocha_bvh_parse, dim3(p.nblocks), dim3(256), 0, s, p); break;
    case 3: {
        const size_t lanes = std::max<size_t>((size_t)p.C, p.channels == 3 ? (size_t)p.F * p.v_out : 0);
        hipLaunchKernelGGL(mocha_bvh_finish, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s, p);
        break;
    }
    case 4:
        if (p.n_patch == 0) return hipSuccess;
        hipLaunchKernelGGL(mocha_bvh_patch, dim3((p.n_patch + 255) / 256), dim3(256), 0, s, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace mocha
