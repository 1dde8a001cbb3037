// The per-frame body of the demo's window featurisation (test_fullframework.py:141-185), shared by mocha_featurize (featurize.hip:
// finished windows in global memory) and mocha_live_push (live.hip: the window read out of a device-resident ring), so that both
// produce the same bits: forward kinematics with velocities over the bone tree (motion/quat.py:189-204), the window re-rooted on its
// last frame (:148-151), every bone expressed in that root frame (:154-158), features [pos 3 | rotation-matrix xy 6 | vel 3 | ang 3]
// (:180-185).  One thread per frame; the per-bone global transforms a thread needs for its children live in LDS
// ([bone][component][thread], conflict-free).  Quaternions are (w, x, y, z) as in the reference.
#pragma once
#include <hip/hip_runtime.h>

namespace mocha {

struct Q { float w, x, y, z; };
struct V3 { float x, y, z; };

__device__ __forceinline__ V3 crossv(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 addv(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 subv(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
// motion/quat.py:112-120: mul(x, y)
__device__ __forceinline__ Q qmul(Q x, Q y) {
    return {y.w * x.w - y.x * x.x - y.y * x.y - y.z * x.z,
            y.w * x.x + y.x * x.w - y.y * x.z + y.z * x.y,
            y.w * x.y + y.x * x.z + y.y * x.w - y.z * x.x,
            y.w * x.z - y.x * x.y + y.y * x.x + y.z * x.w};
}
__device__ __forceinline__ Q qinv(Q q) { return {q.w, -q.x, -q.y, -q.z}; }
// motion/quat.py:128-130: t = 2 cross(q.xyz, v); v + w t + cross(q.xyz, t)
__device__ __forceinline__ V3 qrot(Q q, V3 v) {
    const V3 u = {q.x, q.y, q.z};
    V3 t = crossv(u, v);
    t = {2.0f * t.x, 2.0f * t.y, 2.0f * t.z};
    const V3 c = crossv(u, t);
    return {v.x + q.w * t.x + c.x, v.y + q.w * t.y + c.y, v.z + q.w * t.z + c.z};
}

static constexpr int FT = 64;       // threads per workgroup
static constexpr int FC = 13;       // floats kept per bone: rot 4, pos 3, vel 3, ang 3
static constexpr int FEAT_MAX_BONES = 40;

// One frame: `load(i, lr, lp, lv, la)` hands over bone i's local rotation / offset / velocity / angular velocity, (Rr, Rp, Rv, Ra) is
// bone 0 of the window's last frame, o the frame's J x 15 output row, g the workgroup's LDS ([J][FC][FT] floats), tid the thread's column.
template <class Load>
__device__ __forceinline__ void featurize_frame(Load&& load, const int* __restrict__ parents, int J, Q Rr, V3 Rp, V3 Rv, V3 Ra,
                                                float* __restrict__ out, float* g, int tid) {
    const Q Ri = qinv(Rr);
    auto G = [&](int bone, int comp) -> float& { return g[(bone * FC + comp) * FT + tid]; };
    for (int i = 0; i < J; ++i) {
        Q lr; V3 lp, lv, la;
        load(i, lr, lp, lv, la);
        Q gr; V3 gp, gv, ga;
        if (i == 0) {
            gr = lr; gp = lp; gv = lv; ga = la;
        } else {
            const int p = parents[i];
            const Q pr = {G(p, 0), G(p, 1), G(p, 2), G(p, 3)};
            const V3 pp = {G(p, 4), G(p, 5), G(p, 6)}, pv = {G(p, 7), G(p, 8), G(p, 9)}, pa = {G(p, 10), G(p, 11), G(p, 12)};
            const V3 rp = qrot(pr, lp);
            gp = addv(rp, pp);
            gr = qmul(pr, lr);
            gv = addv(addv(qrot(pr, lv), crossv(pa, rp)), pv);
            ga = addv(qrot(pr, la), pa);
        }
        G(i, 0) = gr.w; G(i, 1) = gr.x; G(i, 2) = gr.y; G(i, 3) = gr.z;
        G(i, 4) = gp.x; G(i, 5) = gp.y; G(i, 6) = gp.z; G(i, 7) = gv.x; G(i, 8) = gv.y; G(i, 9) = gv.z;
        G(i, 10) = ga.x; G(i, 11) = ga.y; G(i, 12) = ga.z;
        // the root bone's own globals are replaced by the last frame's (test_fullframework.py:148-151)
        if (i == 0) { gr = Rr; gp = Rp; gv = Rv; ga = Ra; }
        const V3 xp = qrot(Ri, subv(gp, Rp));
        const Q xr = qmul(Ri, gr);
        const V3 xv = qrot(Ri, gv), xa = qrot(Ri, ga);
        // to_xform_xy, motion/quat.py:42-55
        const float x2 = xr.x + xr.x, y2 = xr.y + xr.y, z2 = xr.z + xr.z;
        const float xx = xr.x * x2, yy = xr.y * y2, wx = xr.w * x2;
        const float xy = xr.x * y2, yz = xr.y * z2, wy = xr.w * y2;
        const float xz = xr.x * z2, zz = xr.z * z2, wz = xr.w * z2;
        float* o = out + (size_t)i * 15;
        o[0] = xp.x; o[1] = xp.y; o[2] = xp.z;
        o[3] = 1.0f - (yy + zz); o[4] = xy - wz;
        o[5] = xy + wz;          o[6] = 1.0f - (xx + zz);
        o[7] = xz - wy;          o[8] = yz + wx;
        o[9] = xv.x; o[10] = xv.y; o[11] = xv.z;
        o[12] = xa.x; o[13] = xa.y; o[14] = xa.z;
    }
}

}  // namespace mocha
