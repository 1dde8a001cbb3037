// World-space poses and skinning palettes (mocha_world_pose, mocha_world_bind): what the reference's demo computes at its end with quat.fk
// over every output stream (test_fullframework.py:672-690) for animation_plot (:670).  Local rotations (n,V+1,4) w,x,y,z and positions
// (n,V+1,3), root bone first, float64 (what post-processing emits) or fp32 (what the mocap front end and the resampler emit; widened on
// load, the same code after that) -> gpos (n,V+1,3), grot (n,V+1,4) float64 and palette (n,V,12) fp32, each optional.
//   mocha_world_pose_k   workgroup = WORLD_FPB frames x 32 lanes, lane = (frame, bone).  A frame's rows are one contiguous run of every
//                        array and the workgroup's frames follow each other, so a frame's 32 lanes walk its run - consecutive lanes,
//                        consecutive 16-byte (rotations, palette) or 8- / 4-byte (positions) words, no division in the addressing -
//                        through LDS, where a frame's locals and globals live: forward kinematics indexes them by a run-time ancestor
//                        (the rule ingest_clip.hip states).
//   mocha_world_bind_k   one workgroup: the rest pose through the same functions, its rigid inverses and `pre` into the caller's bind.
// Forward kinematics: every lane folds down ITS OWN ancestor chain out of LDS (world_fk_bone) instead of the workgroup walking the tree
// one level per barrier as ingest_clip.hip's fk_levels does.  The chain costs a bone as many products as it has ancestors, where the level
// walk costs one - but a frame moves about 4 KB of HBM traffic against some hundred float64 products per bone (measured: DESIGN 8.22), the
// level walk holds all 256 lanes at max_depth barriers with most of them idle at every level, and the chain needs no depth table and no
// barrier between the load and the store phases.  A bone's result comes from one instruction sequence on its own chain, whatever call
// the frame arrives in: n frames in a call, each frame alone and the two input instances agree bit for bit (tests/test_world_pose_kernel.py).
// Rows whose valid entry is 0 are read but never written.  No allocation, no synchronisation.
#include "world_pose_body.h"

namespace mocha {

namespace {
constexpr int NB = MOCHA_MAX_BONES;

__device__ inline void load_rot(const double* __restrict__ src, size_t unit, double* __restrict__ dst) {      // unit: half a quaternion
    const double2 v = reinterpret_cast<const double2*>(src)[unit];
    dst[0] = v.x; dst[1] = v.y;
}
__device__ inline void load_rot(const float* __restrict__ src, size_t unit, double* __restrict__ dst) {       // unit: a quaternion
    const float4 v = reinterpret_cast<const float4*>(src)[unit];
    dst[0] = (double)v.x; dst[1] = (double)v.y; dst[2] = (double)v.z; dst[3] = (double)v.w;
}
}  // namespace

template <typename T>
__global__ __launch_bounds__(WORLD_FPB * NB) void mocha_world_pose_k(WorldPoseParams p) {
    __shared__ __attribute__((aligned(16))) double s_q[WORLD_FPB * NB * 4];      // locals, then globals
    __shared__ __attribute__((aligned(16))) double s_p[WORLD_FPB * NB * 3];
    __shared__ __attribute__((aligned(16))) float s_m[WORLD_FPB * NB * 12];      // palette rows of bones 1..V at slots 0..V-1
    __shared__ double s_b[(NB + 1) * 12];                                        // pre | inverse binds
    __shared__ int s_v[WORLD_FPB];
    constexpr int RU = sizeof(T) == 8 ? 2 : 1, RW = 4 / RU;                      // 16-byte units per quaternion, doubles per unit
    const int tid = threadIdx.x, J = p.V + 1, TH = WORLD_FPB * NB;
    const long long f0 = (long long)blockIdx.x * WORLD_FPB;
    const int nf = (int)(p.n - f0 < WORLD_FPB ? p.n - f0 : WORLD_FPB);           // >= 1: the grid covers n frames and no more
    const T* rot = static_cast<const T*>(p.rot);
    const T* pos = static_cast<const T*>(p.pos);
    const int fr = tid / NB, b = tid % NB;                                       // a frame's 32 lanes move that frame's rows
    const bool in = fr < nf;
    if (in) {
        for (int r = b; r < J * RU; r += NB) load_rot(rot, ((size_t)f0 + fr) * J * RU + r, s_q + fr * NB * 4 + r * RW);
        for (int r = b; r < J * 3; r += NB) s_p[fr * NB * 3 + r] = (double)pos[((size_t)f0 + fr) * J * 3 + r];
    }
    const bool pal = p.palette != nullptr;                                       // the host refused a palette without a bind
    if (pal)
        for (int i = tid; i < (J + 1) * 12; i += TH) s_b[i] = p.bind[i];
    if (tid < WORLD_FPB) s_v[tid] = tid < nf && (!p.valid || p.valid[f0 + tid] != 0);
    __syncthreads();

    const bool act = b < J && s_v[fr];
    dq G = {1.0, 0.0, 0.0, 0.0};
    d3 g = {0.0, 0.0, 0.0};
    float m[12];
    if (act) {
        world_fk_bone(reinterpret_cast<const dq*>(s_q) + fr * NB, reinterpret_cast<const d3*>(s_p) + fr * NB, p.anc[b], G, g);
        if (pal && b >= 1) world_palette(s_b, s_b + 12 * (1 + b), G, g, m);
    }
    __syncthreads();                                                             // every chain has read its locals
    if (act) {
        stq(s_q + (fr * NB + b) * 4, G);
        st3(s_p + (fr * NB + b) * 3, g);
        if (pal && b >= 1) {
            float4* o = reinterpret_cast<float4*>(s_m + (fr * NB + b - 1) * 12);
            o[0] = make_float4(m[0], m[1], m[2], m[3]);
            o[1] = make_float4(m[4], m[5], m[6], m[7]);
            o[2] = make_float4(m[8], m[9], m[10], m[11]);
        }
    }
    __syncthreads();

    if (in && s_v[fr]) {
        const size_t f = (size_t)f0 + fr;
        if (p.grot)
            for (int r = b; r < J * 2; r += NB)
                reinterpret_cast<double2*>(p.grot)[f * J * 2 + r] = *reinterpret_cast<const double2*>(s_q + fr * NB * 4 + r * 2);
        if (p.gpos)
            for (int r = b; r < J * 3; r += NB) p.gpos[f * J * 3 + r] = s_p[fr * NB * 3 + r];
        if (pal)
            for (int r = b; r < p.V * 3; r += NB)
                reinterpret_cast<float4*>(p.palette)[f * p.V * 3 + r] = *reinterpret_cast<const float4*>(s_m + fr * NB * 12 + r * 4);
    }
}

hipError_t launch_world_pose(const WorldPoseParams& p, hipStream_t s) {
    if (p.n <= 0) return hipSuccess;
    if (p.V < 1 || p.V + 1 > NB || !p.rot || !p.pos || (p.palette && !p.bind) || (!p.gpos && !p.grot && !p.palette)) return hipErrorInvalidValue;
    const long long blocks = (p.n + WORLD_FPB - 1) / WORLD_FPB;
    if (blocks > 0x7fffffffll) return hipErrorInvalidValue;
    if (p.in_f32) hipLaunchKernelGGL(mocha_world_pose_k<float>, dim3((unsigned)blocks), dim3(WORLD_FPB * NB), 0, s, p);
    else hipLaunchKernelGGL(mocha_world_pose_k<double>, dim3((unsigned)blocks), dim3(WORLD_FPB * NB), 0, s, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void mocha_world_bind_k(WorldBindParams p) {
    __shared__ dq s_q[NB];
    __shared__ d3 s_p[NB];
    const int b = threadIdx.x, J = p.V + 1;
    if (b < J) {
        dq q = {1.0, 0.0, 0.0, 0.0};
        if (p.rest_rot) {                                                        // quat.normalize (quat.py:15-16), once
            const dq r = ldq(p.rest_rot + b * 4);
            const double l = sqrt(r.w * r.w + r.x * r.x + r.y * r.y + r.z * r.z) + 1e-8;
            q = {r.w / l, r.x / l, r.y / l, r.z / l};
        }
        s_q[b] = q;
        s_p[b] = ld3(p.rest_pos + b * 3);
    }
    __syncthreads();
    if (b < 12) p.bind[b] = p.pre[b];
    if (b < J) {
        dq B;
        d3 c;
        world_fk_bone(s_q, s_p, p.anc[b], B, c);
        const aff34 inv = world_bind_inverse(B, c);
        for (int k = 0; k < 12; ++k) p.bind[12 * (1 + b) + k] = inv.m[k];
    }
}

hipError_t launch_world_bind(const WorldBindParams& p, hipStream_t s) {
    if (p.V < 1 || p.V + 1 > NB || !p.rest_pos || !p.bind) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_world_bind_k, dim3(1), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace mocha
