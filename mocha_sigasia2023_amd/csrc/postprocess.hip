// Post-processing of decoded windows (test_fullframework.py:303-308, 338-437, 457-632, 665-697).
//
//  mocha_pose_heads    one 64-lane workgroup per window: last-frame pose (positions, 6-D rotation -> quaternion as
//                      motion/quat.py:96-107 / :69-94, velocities, angular velocities) and the mean hip speed over
//                      the window; float32 like the reference's NumPy on the float32 network output.
//  mocha_post_clip     the sequential frame loop of one clip per LANE (clips are the data-parallel axis): root
//                      integration, position blending, the foot-lock state machine (motion/Inertialization.py:300-377)
//                      and the two-bone IK (motion/quat.py:295-343), then the root merge + Euler channels the BVH
//                      writer consumes.  float64, because the reference's state arrays are NumPy float64.
//  mocha_inertialize   one 64-lane workgroup per stream, between the two above in a live step: the per-bone inertializers of
//                      motion/Inertialization.py:71-91 on the pose heads, so that a character switch decays instead of popping.
//
// Both kernels also serve the resumable form (launch_post_step, live sessions): ONE frame per clip and launch, the per-lane state (root
// transform, the bone's previous position, the contact record) loaded from and stored to device memory around it.
#include "kernels.h"
#include "quat64.h"

namespace mocha {

// ----------------------------------------------------------------------------------------------- heads
__device__ inline void cross3f(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(64) void mocha_pose_heads(const float* __restrict__ Y, float* __restrict__ heads,
                                                       float* __restrict__ speed, int T, int V) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const float* Yw = Y + (size_t)w * T * V * 15;
    float s = 0.f;
    for (int t = lane; t < T; t += 64) {
        const float* v = Yw + (size_t)t * V * 15 + 9;
        s += sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) speed[w] = s / (float)T;
    for (int j = lane; j < V; j += 64) {
        const float* f = Yw + ((size_t)(T - 1) * V + j) * 15;
        float* h = heads + ((size_t)w * V + j) * 13;
        // x (3,2) row-major: column 0 = f[3], f[5], f[7]; column 1 = f[4], f[6], f[8]
        const float c0[3] = {f[3], f[5], f[7]}, x1[3] = {f[4], f[6], f[8]};
        float c2[3], c1[3];
        cross3f(c0, x1, c2);
        float n = sqrtf(c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2]);
        c2[0] /= n; c2[1] /= n; c2[2] /= n;
        cross3f(c2, c0, c1);
        n = sqrtf(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
        c1[0] /= n; c1[1] /= n; c1[2] /= n;
        // ts[r][c]: columns c0, c1, c2
        const float t00 = c0[0], t10 = c0[1], t20 = c0[2], t01 = c1[0], t11 = c1[1], t21 = c1[2], t02 = c2[0], t12 = c2[1], t22 = c2[2];
        float q[4];
        if (t22 < 0.f) {
            if (t00 > t11) { q[0] = t21 - t12; q[1] = 1.f + t00 - t11 - t22; q[2] = t10 + t01; q[3] = t02 + t20; }
            else           { q[0] = t02 - t20; q[1] = t10 + t01; q[2] = 1.f - t00 + t11 - t22; q[3] = t21 + t12; }
        } else {
            if (t00 < -t11) { q[0] = t10 - t01; q[1] = t02 + t20; q[2] = t21 + t12; q[3] = 1.f - t00 - t11 + t22; }
            else            { q[0] = 1.f + t00 + t11 + t22; q[1] = t21 - t12; q[2] = t02 - t20; q[3] = t10 - t01; }
        }
        const float ql = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) + 1e-8f;
        h[0] = f[0]; h[1] = f[1]; h[2] = f[2];
        h[3] = q[0] / ql; h[4] = q[1] / ql; h[5] = q[2] / ql; h[6] = q[3] / ql;
        h[7] = f[9]; h[8] = f[10]; h[9] = f[11];
        h[10] = f[12]; h[11] = f[13]; h[12] = f[14];
    }
}

hipError_t launch_pose_heads(const float* Y, float* heads, float* speed, int B, int T, int V, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(mocha_pose_heads, dim3(B), dim3(64), 0, s, Y, heads, speed, T, V);
    return hipGetLastError();
}

// ----------------------------------------------------------------------------------------------- clip loop (float64)
// cross product of two vectors that may be the SAME vector, without fused multiply-adds: fma(a.y, b.z, -(a.z * b.y)) leaves the rounding
// error of one product where a x a is exactly 0, and normalize() divides that 1e-17 by its eps of 1e-8
__device__ inline d3 cross_unfused(d3 a, d3 b) {
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
struct ContactRec {
    bool state, lock;
    d3 position, velocity, point, target, off_x, off_v;
};
// State of one clip between two launches of the resumable form, POST_STATE_DOUBLES 8-byte words: [0] frames seen (int64; 0 = none: the
// next frame takes the first-frame branch, so all-zero bytes are a reset clip), [1..3] root position, [4..7] root rotation,
// [8 + 3 j ..] bone j's previous position, then per contact [flags (int64: bit 0 state, bit 1 lock) | position | velocity | point |
// target | off_x | off_v].
static constexpr int POST_STATE_CONTACT0 = 8 + MOCHA_MAX_BONES * 3, POST_STATE_CONTACT = 19;
static_assert(POST_STATE_CONTACT0 + MOCHA_MAX_CONTACT * POST_STATE_CONTACT == POST_STATE_DOUBLES, "post state layout");

// One WAVE per clip (round 3; the first version ran a clip in one lane, 64 clips per wave): the frame loop is sequential, but inside a
// frame the work has width - lane j owns bone j (its blended position is a per-bone recurrence over frames, kept in a register), lane 0
// also integrates the root, lane 32 + c runs contact c's state machine and two-bone IK - and everything a frame needs from memory (the
// bone's 13 head values, the root's source velocities, the contact flags) is fetched one frame AHEAD, so the per-frame critical path is
// the float64 arithmetic itself: root integration, then the chain and the IK of a contact, with one exchange through LDS between them.
// Every value is computed by the same expressions in the same order as before (and as the oracle): results are unchanged.
__global__ __launch_bounds__(64) void mocha_post_clip(PostParams p) {
    __shared__ double sh_pos[MOCHA_MAX_BONES * 3], sh_rot[MOCHA_MAX_BONES * 4];
    __shared__ double sh_w[6];                                   // wv, wa of the frame (the contact reset of frame 0 needs them)
    __shared__ double sh_ikq[MOCHA_MAX_CONTACT][2][4];
    __shared__ int sh_ikv[MOCHA_MAX_CONTACT];
    const int clip = blockIdx.x, lane = threadIdx.x;
    if (p.valid && p.valid[clip] == 0) return;                  // resumable form: a clip that is not stepped (uniform over the workgroup)
    const int V = p.V, J = V + 1, N = p.n_frames;
    const float* heads = p.heads + (size_t)clip * N * V * 13;
    const float* speed = p.speed + (size_t)clip * N;
    const float* rvel_s = p.src_rvel + (size_t)clip * N * 3;
    const float* rang_s = p.src_rang + (size_t)clip * N * 3;
    const float* sspeed = p.src_speed + (size_t)clip * N;
    const unsigned char* contact = p.contact + (size_t)clip * N * p.n_contact;
    double* POS = p.pos + (size_t)clip * N * J * 3;
    double* ROT = p.rot + (size_t)clip * N * J * 4;
    double* IKR = p.ik_rot + (size_t)clip * N * J * 4;
    double* BP = (p.bvh_pos && p.bvh_euler) ? p.bvh_pos + (size_t)clip * N * V * 3 : nullptr;
    const double dt = p.dt;
    const double ydamp = (4.0 * 0.6931471805599453) / (p.halflife + 1e-5) / 2.0;             // Inertialization.py:13-14, 40
    const double eydt = 1.0 / (1.0 + ydamp * dt + 0.48 * (ydamp * dt) * (ydamp * dt) + 0.235 * (ydamp * dt) * (ydamp * dt) * (ydamp * dt));

    const bool is_joint = lane < J, is_bone = lane >= 1 && lane < J;
    const int ci = lane - 32;
    const bool is_contact = ci >= 0 && ci < p.n_contact;
    // a contact lane's chain toe -> ... -> root (quat.py:241-273 recursion order, evaluated top-down), fixed for the clip
    int chain[MOCHA_MAX_CHAIN], depth = 0;
    if (is_contact)
        for (int b = p.contact_bones[ci]; b != -1 && depth < MOCHA_MAX_CHAIN; b = p.parents[b]) chain[depth++] = b;
    // which contacts write this bone's IK rotation (chain[3] the hip, chain[2] the knee), in contact order
    int ik_slot[MOCHA_MAX_CONTACT];
#pragma unroll
    for (int c = 0; c < MOCHA_MAX_CONTACT; ++c) {
        ik_slot[c] = -1;
        if (c < p.n_contact && is_joint) {
            int ch[MOCHA_MAX_CHAIN], d = 0;
            for (int b = p.contact_bones[c]; b != -1 && d < MOCHA_MAX_CHAIN; b = p.parents[b]) ch[d++] = b;
            if (d >= 5) { if (ch[3] == lane) ik_slot[c] = 0; else if (ch[2] == lane) ik_slot[c] = 1; }
        }
    }

    // per-lane state
    ContactRec cr;                                              // contact lanes
    d3 root_pos = {0, 0, 0};                                    // lane 0
    dq root_rot = {1, 0, 0, 0};
    d3 prev_p = {0, 0, 0};                                      // joint lanes: this bone's position in the previous frame
    // inputs of the frame about to be processed, fetched one frame ahead
    float hn[13];                                               // bone lanes
    float r_speed = 0.f, r_sspeed = 1.f, r_rv[3] = {0, 0, 0}, r_ra[3] = {0, 0, 0};            // lane 0
    unsigned char c_flag = 0;                                   // contact lanes
    // Resumable form (launch_post_step): the frames seen so far and the per-lane state come from / go back to device memory.  The
    // first-frame branch below is taken by frame 0 of a clip that has seen no frame yet; without a state that is frame 0 of the launch.
    double* S = p.state ? p.state + (size_t)clip * POST_STATE_DOUBLES : nullptr;
    double* cs = S ? S + POST_STATE_CONTACT0 + (is_contact ? ci : 0) * POST_STATE_CONTACT : nullptr;
    long long seen = 0;
    if (S) {
        seen = *reinterpret_cast<const long long*>(S);
        if (seen != 0) {
            if (lane == 0) { root_pos = ld3(S + 1); root_rot = ldq(S + 4); }
            if (is_joint) prev_p = ld3(S + 8 + lane * 3);
            if (is_contact) {
                const long long fl = *reinterpret_cast<const long long*>(cs);
                cr.state = (fl & 1) != 0; cr.lock = (fl & 2) != 0;
                cr.position = ld3(cs + 1); cr.velocity = ld3(cs + 4); cr.point = ld3(cs + 7);
                cr.target = ld3(cs + 10); cr.off_x = ld3(cs + 13); cr.off_v = ld3(cs + 16);
            }
        }
    }
    auto fetch = [&](int i) __attribute__((always_inline)) {
        if (i >= N) return;
        if (is_bone) {
            const float* hj = heads + ((size_t)i * V + (lane - 1)) * 13;
#pragma unroll
            for (int k = 0; k < 13; ++k) hn[k] = hj[k];
        }
        if (lane == 0) {
            r_speed = speed[i]; r_sspeed = sspeed[i];
            r_rv[0] = rvel_s[i * 3]; r_rv[1] = rvel_s[i * 3 + 1]; r_rv[2] = rvel_s[i * 3 + 2];
            r_ra[0] = rang_s[i * 3]; r_ra[1] = rang_s[i * 3 + 1]; r_ra[2] = rang_s[i * 3 + 2];
        }
        if (is_contact) c_flag = contact[(size_t)i * p.n_contact + ci];
    };
    fetch(0);

    for (int i = 0; i < N; ++i) {
        const bool first = i == 0 && seen == 0;
        // this frame's inputs into locals, the next frame's on their way
        float h[13];
#pragma unroll
        for (int k = 0; k < 13; ++k) h[k] = hn[k];
        const float f_speed = r_speed, f_sspeed = r_sspeed;
        const float f_rv[3] = {r_rv[0], r_rv[1], r_rv[2]}, f_ra[3] = {r_ra[0], r_ra[1], r_ra[2]};
        const bool in_state = c_flag != 0;
        fetch(i + 1);

        double* pos = POS + (size_t)i * J * 3;
        double* rot = ROT + (size_t)i * J * 4;
        double* ikr = IKR + (size_t)i * J * 4;
        d3 pj = {0, 0, 0}, vj = {0, 0, 0};
        dq rj = {1, 0, 0, 0};
        if (lane == 0) {
            // root-velocity ratio in float32, as NumPy computes it on float32 arrays (test_fullframework.py:492-496)
            float ratio = f_speed / f_sspeed;
            if (ratio > 3.0f || ratio < 0.33f) ratio = 1.0f;
            const d3 rv = {(double)(f_rv[0] * ratio), (double)(f_rv[1] * ratio), (double)(f_rv[2] * ratio)};
            const d3 ra = {(double)f_ra[0], (double)f_ra[1], (double)f_ra[2]};
            const d3 wv = qrot(root_rot, rv), wa = qrot(root_rot, ra);                         // :499-502
            root_pos = root_pos + wv * dt;
            root_rot = qmul(root_rot, from_scaled_angle_axis(wa * dt));
            pj = root_pos; vj = wv; rj = root_rot;
            st3(sh_w, wv); st3(sh_w + 3, wa);
            if (BP) st3(BP + (size_t)i * V * 3, root_pos);          // for mocha_post_bvh: the running (unblended) root of this frame
        } else if (is_bone) {
            pj = {(double)h[0], (double)h[1], (double)h[2]};
            rj = {(double)h[3], (double)h[4], (double)h[5], (double)h[6]};
            vj = {(double)h[7], (double)h[8], (double)h[9]};
        }
        if (is_joint) {
            // positions (blended with the previous frame's after the first one, :537/:627), rotations
            if (!first && p.blend_enabled) pj = (prev_p + vj * dt) * 0.5 + pj * 0.5;
            prev_p = pj;
            st3(pos + lane * 3, pj);
            stq(rot + lane * 4, rj);
            st3(sh_pos + lane * 3, pj);
            stq(sh_rot + lane * 4, rj);
        }
        if (lane < MOCHA_MAX_CONTACT) sh_ikv[lane] = 0;
        __syncthreads();

        if (is_contact) {
            if (first) {
                // contact reset with the global position / velocity of the toe (fk_vel_bone, quat.py:207-238)
                const d3 wv = ld3(sh_w), wa = ld3(sh_w + 3);
                d3 gv = {0, 0, 0}, ga = {0, 0, 0}, gpp = {0, 0, 0};
                dq grr = {1, 0, 0, 0};
                for (int k = depth - 1; k >= 0; --k) {
                    const int b = chain[k];
                    d3 lv, la;
                    if (b == 0) { lv = wv; la = wa; }
                    else {
                        const float* hb = heads + (size_t)(b - 1) * 13;                        // frame 0 (the reset happens in the launch's first frame only)
                        lv = {(double)hb[7], (double)hb[8], (double)hb[9]};
                        la = {(double)hb[10], (double)hb[11], (double)hb[12]};
                    }
                    const d3 lp = ld3(sh_pos + b * 3);
                    const dq lr = ldq(sh_rot + b * 4);
                    if (k == depth - 1) { gpp = lp; gv = lv; grr = lr; ga = la; }
                    else {
                        const d3 rp = qrot(grr, lp);
                        gv = gv + qrot(grr, lv) + cross(ga, rp);
                        ga = qrot(grr, la) + ga;
                        gpp = rp + gpp;
                        grr = qmul(grr, lr);
                    }
                }
                cr.state = false; cr.lock = false;
                cr.position = gpp; cr.velocity = gv; cr.point = gpp; cr.target = gpp;
                cr.off_x = {0, 0, 0}; cr.off_v = {0, 0, 0};
            } else if (p.ik_enabled && depth >= 5) {
                d3 gp[MOCHA_MAX_CHAIN];
                dq gr[MOCHA_MAX_CHAIN];
                for (int k = depth - 1; k >= 0; --k) {
                    const int b = chain[k];
                    const d3 lp = ld3(sh_pos + b * 3);
                    const dq lr = ldq(sh_rot + b * 4);
                    if (k == depth - 1) { gp[k] = lp; gr[k] = lr; }
                    else { gp[k] = qrot(gr[k + 1], lp) + gp[k + 1]; gr[k] = qmul(gr[k + 1], lr); }
                }
                // chain[0] toe, [1] heel, [2] knee, [3] hip, [4] the hip's parent
                ContactRec& c = cr;
                const d3 in_pos = gp[0];
                // Inertialization.py:300-377
                const d3 in_vel = (in_pos - c.target) * (1.0 / (dt + 1e-8));
                c.target = in_pos;
                {
                    const d3 j1 = c.off_v + c.off_x * ydamp;                                   // :39-54
                    c.off_x = eydt * (c.off_x + j1 * dt);
                    c.off_v = eydt * (c.off_v - j1 * (ydamp * dt));
                }
                if (c.lock) { c.position = c.point + c.off_x; c.velocity = c.off_v; }
                else { c.position = in_pos + c.off_x; c.velocity = in_vel + c.off_v; }
                const bool unlock = c.lock && len(c.point - in_pos) > p.unlock_radius;
                if (!c.state && in_state) {
                    c.lock = true;
                    c.point = c.position;
                    c.point.y = p.foot_height;
                    c.off_x = (in_pos + c.off_x) - c.point;
                    c.off_v = in_vel + c.off_v;
                } else if ((c.lock && c.state && !in_state) || unlock) {
                    c.lock = false;
                    c.off_x = (c.point + c.off_x) - in_pos;
                    c.off_v = c.off_v - in_vel;
                }
                c.state = in_state;
                if (c.position.y < p.foot_height) c.position.y = p.foot_height;                // test_fullframework.py:581-582
                // two-bone IK (quat.py:295-343): a hip, b knee, c heel
                const d3 a = gp[3], b = gp[2], e = gp[1];
                const d3 target = c.position + (gp[1] - gp[0]);
                const d3 fwd = qrot(gr[2], d3{0.0, 1.0, 0.0});
                const double max_ext = len(a - b) + len(b - e) - p.max_length_buffer;
                d3 t = target;
                if (len(target - a) > max_ext) t = a + max_ext * normalize(target - a);
                const d3 axis_rot = normalize(cross(normalize(e - a), fwd));
                const double lab = len(b - a), lcb = len(b - e), lat = len(t - a);
                const double ac_ab_0 = acos(clamp1(dot(normalize(e - a), normalize(b - a))));
                const double ba_bc_0 = acos(clamp1(dot(normalize(a - b), normalize(e - b))));
                const double ac_ab_1 = acos(clamp1((lab * lab + lat * lat - lcb * lcb) / (2.0 * lab * lat)));
                const double ba_bc_1 = acos(clamp1((lab * lab + lcb * lcb - lat * lat) / (2.0 * lab * lcb)));
                const dq r0 = from_angle_axis(ac_ab_1 - ac_ab_0, axis_rot);
                const dq r1 = from_angle_axis(ba_bc_1 - ba_bc_0, axis_rot);
                const d3 c_a = normalize(e - a), t_a = normalize(t - a);
                // a contact that has not locked yet has its target ON the heel: c_a and t_a may be the same bits (whenever toe + (heel - toe)
                // rounds to the heel), and their cross product then has to be the exact 0 the reference gets - r2 turns nothing
                const dq r2 = from_angle_axis(acos(clamp1(dot(c_a, t_a))), normalize(cross_unfused(c_a, t_a)));
                stq(&sh_ikq[ci][0][0], qmul(qinv(gr[4]), qmul(r2, qmul(r0, gr[3]))));          // the hip's (chain[3])
                stq(&sh_ikq[ci][1][0], qmul(qinv(gr[3]), qmul(r1, gr[2])));                    // the knee's (chain[2])
                sh_ikv[ci] = 1;
            }
        }
        __syncthreads();
        if (is_joint) {
            // the IK rotations: the bone's own rotation unless a contact replaced it (later contacts win, as in the sequential order)
            dq q = rj;
#pragma unroll
            for (int c = 0; c < MOCHA_MAX_CONTACT; ++c)
                if (ik_slot[c] >= 0 && sh_ikv[c]) q = ldq(&sh_ikq[c][ik_slot[c]][0]);
            stq(ikr + lane * 4, q);
        }
        __syncthreads();                                        // the LDS exchange is rewritten by the next frame
    }
    if (S) {
        if (lane == 0) {
            *reinterpret_cast<long long*>(S) = seen + N;
            st3(S + 1, root_pos); stq(S + 4, root_rot);
        }
        if (is_joint) st3(S + 8 + lane * 3, prev_p);
        if (is_contact) {
            *reinterpret_cast<long long*>(cs) = (cr.state ? 1 : 0) | (cr.lock ? 2 : 0);
            st3(cs + 1, cr.position); st3(cs + 4, cr.velocity); st3(cs + 7, cr.point);
            st3(cs + 10, cr.target); st3(cs + 13, cr.off_x); st3(cs + 16, cr.off_v);
        }
    }
}

// BVH channels (test_fullframework.py:677-681; quat.py:346-355): fold the synthetic root into bone 1, Euler angles in degrees.  No
// dependence between frames or bones - 3 float64 inverse trigonometric functions per bone, which the frame loop above used to
// evaluate one after the other in its single lane (72 per frame: most of its 46 us per frame for one clip).
__global__ __launch_bounds__(256) void mocha_post_bvh(PostParams p) {
    const int V = p.V, J = V + 1, N = p.n_frames;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long long)p.n_clips * N * V) return;
    const int j = (int)(t % V) + 1;
    const long long ci = t / V;                     // clip * N + frame
    if (p.valid && p.valid[ci / N] == 0) return;    // resumable form: a clip that is not stepped keeps its rows
    const double* pos = p.pos + (size_t)ci * J * 3;
    const double* ikr = p.ik_rot + (size_t)ci * J * 4;
    double* bp = p.bvh_pos + ((size_t)ci * V + (j - 1)) * 3;
    d3 pj = ld3(pos + j * 3);
    dq q = ldq(ikr + j * 4);
    if (j == 1) {
        const d3 root_pos = ld3(bp);                // parked by the frame loop
        const dq root_rot = ldq(p.rot + (size_t)ci * J * 4);       // ROT[frame][0]: the running root rotation (rotations are not blended)
        pj = qrot(root_rot, pj) + root_pos; q = qmul(root_rot, q);
    }
    st3(bp, pj);
    const double r2d = 57.29577951308232;
    d3 eu = {atan2(2 * (q.w * q.x + q.y * q.z), 1 - 2 * (q.x * q.x + q.y * q.y)), asin(clamp1(2 * (q.w * q.y - q.z * q.x))),
             atan2(2 * (q.w * q.z + q.x * q.y), 1 - 2 * (q.y * q.y + q.z * q.z))};
    st3(p.bvh_euler + ((size_t)ci * V + (j - 1)) * 3, eu * r2d);
}

hipError_t launch_post_clip(const PostParams& p, hipStream_t s) {
    if (p.n_clips <= 0 || p.n_frames <= 0) return hipSuccess;
    if (p.V + 1 > MOCHA_MAX_BONES || p.n_contact > MOCHA_MAX_CONTACT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_post_clip, dim3(p.n_clips), dim3(64), 0, s, p);
    if (p.bvh_pos && p.bvh_euler) {
        const long long n = (long long)p.n_clips * p.n_frames * p.V;
        hipLaunchKernelGGL(mocha_post_bvh, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
    }
    return hipGetLastError();
}

// The resumable form: the SAME two kernels on one frame per clip (p.n_frames = 1), the frame loop's state loaded from / stored to
// p.state around it and clips with valid[clip] == 0 skipped - so stepping a clip frame by frame executes, frame for frame, the
// instructions mocha_postprocess executes on the whole clip.
hipError_t launch_post_step(const PostParams& p, hipStream_t s) {
    if (p.n_frames != 1 || !p.state) return hipErrorInvalidValue;
    return launch_post_clip(p, s);
}

// ----------------------------------------------------------------------------------------------- inertialized character switches
// The reference's per-bone inertializers (motion/Inertialization.py:71-91, springs :10-37), which its demo never calls, applied to the
// pose heads between mocha_pose_heads and the post-processing frame: when a stream names another character, the decoder's pose has
// nothing to do with the previous one, and the difference is kept as an offset that decays with a critically damped spring.
//
// One 64-lane workgroup per stream, lane j owns non-root bone j (V + 1 <= MOCHA_MAX_BONES) and all 13 channels of its head row
// [pos 3 | quat wxyz 4 | vel 3 | ang 3].  The ROOT bone is not inertialized: the frame loop integrates it from its own previous output
// (test_fullframework.py:500-503), so it is continuous by construction.
//
// State of one stream, INERT_STATE_DOUBLES 8-byte words: [0] flags (int64: bit 0 seen, bit 1 active), [1] last id (int64), then
// INERT_BONE_DOUBLES planes of MOCHA_MAX_BONES words, word k of bone j at 2 + k * MOCHA_MAX_BONES + j: prev_in (13: the stream's previous
// valid INPUT heads, before offsets), off_pos, off_vel, off_ang (3 each), off_rot (4).  All-zero bytes are a reset stream: with seen == 0
// no offset is read, and the first valid frame writes them at rest (off_rot = identity).
//
// Per frame and stream, from device data alone:
//   not valid   valid given and valid[s] == 0 (the stream is warming): heads untouched, seen = active = 0.
//   first       seen == 0: prev_in = in, last_id = id, offsets at rest, seen = 1; out = in bit for bit.
//   transition  seen, and ids given with ids[s] != last_id, or trigger given with trigger[s] != 0: inertialize_transition_pos / _rot
//               (:71-74, :82-85, with quat.abs: w > 0.0 or negated) with src = prev_in and dst = in, then active = 1 and the update below in
//               the same frame (pose_transition followed by pose_update).  "src" is the stream's previous valid frame, NOT an extrapolation
//               of it to the switch frame: the function as the reference wrote it.
//   update      active: inertialize_update_pos / _rot (:76-80, :87-91): the offsets decay (fast_negexpf as the rational function written
//               there, halflife_to_damping with eps = 1e-5, quat.log / quat.exp with their eps = 1e-5 branches), out = in (+) offset;
//               out.rot = off_rot * in.rot is not renormalised, as in the reference.
//   not active  seen, no transition since the reset: out = in bit for bit (the words are copied: in + 0.0 would lose a -0.0).
//   always, for a valid frame: prev_in = in (the input, not the output), last_id = id.
// float64 arithmetic on the fp32 inputs, outputs rounded to fp32 once, offsets float64 across frames.
__global__ __launch_bounds__(64) void mocha_inertialize(double* __restrict__ state, const float* heads_in, float* heads_out,
                                                        const int32_t* __restrict__ ids, const int32_t* __restrict__ trigger,
                                                        const int32_t* __restrict__ valid, int V, double halflife, double dt) {
    const int s = blockIdx.x, lane = threadIdx.x;
    double* S = state + (size_t)s * INERT_STATE_DOUBLES;
    long long* F = reinterpret_cast<long long*>(S);
    if (valid && valid[s] == 0) {                               // uniform over the workgroup
        if (lane == 0) F[0] = 0;
        return;
    }
    const long long flags = F[0], last_id = F[1];
    const bool seen = (flags & 1) != 0;
    const long long id = ids ? (long long)ids[s] : (seen ? last_id : 0);
    const bool trans = seen && ((ids && id != last_id) || (trigger && trigger[s] != 0));
    const bool active = seen && (trans || (flags & 2) != 0);
    __syncthreads();                                            // every lane has read the flags before lane 0 rewrites them
    if (lane == 0) { F[0] = 1 | (active ? 2 : 0); F[1] = id; }
    if (lane >= V) return;
    double* B = S + 2 + lane;                                   // word k of this bone: B[k * MOCHA_MAX_BONES]
    const float* hin = heads_in + ((size_t)s * V + lane) * 13;
    float* hout = heads_out + ((size_t)s * V + lane) * 13;
    float h[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) h[k] = hin[k];
    auto W = [&](int k) -> double& { return B[k * MOCHA_MAX_BONES]; };
    if (!active) {
        if (!seen) {
#pragma unroll
            for (int k = 13; k < INERT_BONE_DOUBLES; ++k) W(k) = k == 22 ? 1.0 : 0.0;         // offsets at rest, off_rot = (1, 0, 0, 0)
        }
#pragma unroll
        for (int k = 0; k < 13; ++k) { W(k) = (double)h[k]; hout[k] = h[k]; }
        return;
    }
    const d3 in_p = {(double)h[0], (double)h[1], (double)h[2]}, in_v = {(double)h[7], (double)h[8], (double)h[9]},
             in_a = {(double)h[10], (double)h[11], (double)h[12]};
    const dq in_r = {(double)h[3], (double)h[4], (double)h[5], (double)h[6]};
    d3 off_p = {W(13), W(14), W(15)}, off_v = {W(16), W(17), W(18)}, off_a = {W(19), W(20), W(21)};
    dq off_r = {W(22), W(23), W(24), W(25)};
    if (trans) {
        const d3 src_p = {W(0), W(1), W(2)}, src_v = {W(7), W(8), W(9)}, src_a = {W(10), W(11), W(12)};
        const dq src_r = {W(3), W(4), W(5), W(6)};
        off_p = (src_p + off_p) - in_p;                                                        // Inertialization.py:72-73
        off_v = (src_v + off_v) - in_v;
        off_r = qmul(qmul(off_r, src_r), qinv(in_r));                                          // :83
        if (!(off_r.w > 0.0)) off_r = {-off_r.w, -off_r.x, -off_r.y, -off_r.z};                // quat.py:18-19
        off_a = (off_a + src_a) - in_a;                                                        // :84
    }
    const double y = (4.0 * 0.6931471805599453) / (halflife + 1e-5) / 2.0;                     // :13-14, 19
    const double ydt = y * dt;
    const double eydt = 1.0 / (1.0 + ydt + 0.48 * ydt * ydt + 0.235 * ydt * ydt * ydt);        // :10-11
    {
        const d3 j1 = off_v + off_p * y;                                                       // :18-26
        off_p = eydt * (off_p + j1 * dt);
        off_v = eydt * (off_v - (j1 * y) * dt);
    }
    {
        const d3 j0 = to_scaled_angle_axis(off_r);                                             // :28-37
        const d3 j1 = off_a + j0 * y;
        off_r = from_scaled_angle_axis(eydt * (j0 + j1 * dt));
        off_a = eydt * (off_a - (j1 * y) * dt);
    }
    const d3 out_p = in_p + off_p, out_v = in_v + off_v, out_a = off_a + in_a;                 // :78-79, 90
    const dq out_r = qmul(off_r, in_r);                                                        // :89
#pragma unroll
    for (int k = 0; k < 13; ++k) W(k) = (double)h[k];
    W(13) = off_p.x; W(14) = off_p.y; W(15) = off_p.z; W(16) = off_v.x; W(17) = off_v.y; W(18) = off_v.z;
    W(19) = off_a.x; W(20) = off_a.y; W(21) = off_a.z; W(22) = off_r.w; W(23) = off_r.x; W(24) = off_r.y; W(25) = off_r.z;
    hout[0] = (float)out_p.x; hout[1] = (float)out_p.y; hout[2] = (float)out_p.z;
    hout[3] = (float)out_r.w; hout[4] = (float)out_r.x; hout[5] = (float)out_r.y; hout[6] = (float)out_r.z;
    hout[7] = (float)out_v.x; hout[8] = (float)out_v.y; hout[9] = (float)out_v.z;
    hout[10] = (float)out_a.x; hout[11] = (float)out_a.y; hout[12] = (float)out_a.z;
}

hipError_t launch_inertialize(double* state, const float* heads_in, float* heads_out, const int32_t* ids, const int32_t* trigger,
                              const int32_t* valid, int n, int V, double halflife, double dt, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (V < 1 || V + 1 > MOCHA_MAX_BONES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_inertialize, dim3(n), dim3(64), 0, s, state, heads_in, heads_out, ids, trigger, valid, V, halflife, dt);
    return hipGetLastError();
}

}  // namespace mocha
