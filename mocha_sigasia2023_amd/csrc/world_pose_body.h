// One bone of one frame in world space: forward kinematics (quat.fk, motion/quat.py:166-173, with mul :112-120 and mul_vec :128-130) and
// the skinning palette entry  pre o [to_xform(G) | g] o inverse bind  (to_xform: quat.py:27-40).  mocha_world_pose_k (both input
// instances) and mocha_world_bind_k call these functions on a frame's locals in LDS, so what a frame gives does not depend on the call it
// arrives in, on its place in the batch, or on the width its inputs were stored in.
#pragma once
#include "kernels.h"
#include "quat64.h"

namespace mocha {

// a 3x4 affine map, row-major: m[4 i + j] = R[i][j], m[4 i + 3] = t[i]
struct aff34 { double m[12]; };

// G[b], g[b] of quat.fk from the frame's locals lq / lp (LDS, indexed by bone).  anc: bit a is set for b and for every ancestor a of b;
// parents precede their children, so the set bits in ascending order are the chain from the root down to b, and folding along it does
// the very operations quat.fk does for b, in its order:  g = mul_vec(G[par], p) + g[par],  G = mul(G[par], q).
__device__ inline void world_fk_bone(const dq* __restrict__ lq, const d3* __restrict__ lp, unsigned anc, dq& G, d3& g) {
    int a = __ffs(anc) - 1;
    anc &= anc - 1;
    G = lq[a];
    g = lp[a];
    while (anc) {
        a = __ffs(anc) - 1;
        anc &= anc - 1;
        g = qrot(G, lp[a]) + g;
        G = qmul(G, lq[a]);
    }
}

// quat.to_xform as written (quat.py:31-39), every product and sum rounded on its own: with an identity bind and an identity `pre` the
// palette is then to_xform of the float64 grot the same launch writes, bit for bit
__device__ inline void world_to_xform(dq q, double* __restrict__ R /*[9]*/) {
#pragma clang fp contract(off)
    const double x2 = q.x + q.x, y2 = q.y + q.y, z2 = q.z + q.z;
    const double xx = q.x * x2, yy = q.y * y2, wx = q.w * x2;
    const double xy = q.x * y2, yz = q.y * z2, wy = q.w * y2;
    const double xz = q.x * z2, zz = q.z * z2, wz = q.w * z2;
    R[0] = 1.0 - (yy + zz); R[1] = xy - wz;         R[2] = xz + wy;
    R[3] = xy + wz;         R[4] = 1.0 - (xx + zz); R[5] = yz - wx;
    R[6] = xz - wy;         R[7] = yz + wx;         R[8] = 1.0 - (xx + yy);
}

// a o b: rotation rows times columns summed k = 0, 1, 2; translation R_a t_b summed the same way, then + t_a
__device__ inline aff34 world_compose(const aff34& a, const aff34& b) {
    aff34 r;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) r.m[4 * i + j] = a.m[4 * i] * b.m[j] + a.m[4 * i + 1] * b.m[4 + j] + a.m[4 * i + 2] * b.m[8 + j];
        r.m[4 * i + 3] = (a.m[4 * i] * b.m[3] + a.m[4 * i + 1] * b.m[7] + a.m[4 * i + 2] * b.m[11]) + a.m[4 * i + 3];
    }
    return r;
}

__device__ inline aff34 world_affine(dq G, d3 g) {
    double R[9];
    world_to_xform(G, R);
    return {{R[0], R[1], R[2], g.x, R[3], R[4], R[5], g.y, R[6], R[7], R[8], g.z}};
}

// the rigid inverse (R^T, -R^T c) of a bind global
__device__ inline aff34 world_bind_inverse(dq B, d3 c) {
    double R[9];
    world_to_xform(B, R);
    return {{R[0], R[3], R[6], -(R[0] * c.x + R[3] * c.y + R[6] * c.z),
             R[1], R[4], R[7], -(R[1] * c.x + R[4] * c.y + R[7] * c.z),
             R[2], R[5], R[8], -(R[2] * c.x + R[5] * c.y + R[8] * c.z)}};
}

// (pre o [to_xform(G) | g]) o binv in float64, rounded once to fp32
__device__ inline void world_palette(const double* __restrict__ pre, const double* __restrict__ binv, dq G, d3 g, float* __restrict__ out) {
    aff34 P, I;
#pragma unroll
    for (int k = 0; k < 12; ++k) { P.m[k] = pre[k]; I.m[k] = binv[k]; }
    const aff34 r = world_compose(world_compose(P, world_affine(G, g)), I);
#pragma unroll
    for (int k = 0; k < 12; ++k) out[k] = (float)r.m[k];
}

}  // namespace mocha
