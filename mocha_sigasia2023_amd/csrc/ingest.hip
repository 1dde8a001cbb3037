// The mocap front end of a live session (mocha_live_ingest_step, mocha_live_step_raw): the reference's clip preparation
// (preprocess/generate_database.py:86-177 - root bone extraction, velocities, foot contacts) in streaming form, one raw frame per call.
//
// A stream has pushed raw frames r_0 .. r_{n-1}; L = lookahead (0..18).  Once n >= 31 (savgol_filter refuses a shorter clip) a call emits
// frame t = n-1-L of process_data applied to that prefix.  L = 18 gives the whole clip's frame, 0.3 s late; L = 0 gives the newest frame
// with the reference's clip-end rules applied at it: the polynomial edge fit of mode='interp', v[-1] = v[-2] + (v[-2] - v[-3]), and the
// 'nearest' padding of the median filter.
//
//  mocha_live_ingest   one 64-lane workgroup per stream, float64.  In order:
//    store    lane v < V: from_euler (quat.py:57-67; degrees -> radians as np.radians) or the quaternion as given, unrolled against the
//             bone's previous quaternion (quat.py:135-141: negate when the dot product is negative), positions x unit scale; lane 0 then
//             runs forward kinematics (quat.py:166-173) for the spine joint on xz and the projected, normalised across-direction
//             (:106, :112-119).  All of it goes into the stream's ring of INGEST_RING frames.
//    root     for the frames t-4 .. min(t+3, n-1), lane (frame, series): the 15-tap fit of the spine position and the 31-tap fit of the
//             direction (:107, :120), with the centre row, or - for a frame closer than half a window to an end of the prefix - that frame's
//             row over the first / last window.  Then per frame: renormalise, root rotation = normalize(between(z, direction)) (:121-124),
//             hips made root-local (:127-128).
//    vel/ang  for the frames t-3 .. min(t+2, n-1) and all V+1 bones: central differences (:138-151), the prefix's last frame extrapolated.
//    contact  lane (toe, frame): fk_vel (quat.py:189-204) down the toe's chain, speed < threshold (:162-169); the 6-tap median of the
//             boolean track (:173-177) is "at least 3 of the frames t-3 .. t+2, indices clamped to the prefix".
//    emit     frame t rounded to fp32 once; src_rvel / src_rang = inv_mul_vec(Yrot[0], Yvel[0] / Yang[0]) (test_fullframework.py:142-143)
//             and src_speed = mean |v| of bone 1 over the last 60 emitted frames (:493, v by :164-169; 0 before there are 60), all three
//             evaluated in float64 on the fp32 values the demo reads and rounded once - the demo evaluates them in fp32 NumPy, so they
//             may sit one fp32 ulp away from its values.
//
// The emitted frame reads the root at frames t-4 .. t+3 (contacts at t-3 read the velocity there, which reads the root at t-4), and the
// root direction at t-4 reads raw frames down to t-19 = n-38 at L = 18: hence a ring of 40.  Beyond the ring it depends only on the sign
// state of unroll, which is sequential from the first frame.
//
// State of one stream, INGEST_STATE_DOUBLES 8-byte words: [0] frames pushed (int64), [1] frames emitted (int64), the unroll reference
// quaternion per joint (MOCHA_MAX_BONES x 4), the ring (slot = frame % INGEST_RING: quaternions MOCHA_MAX_BONES x 4 | positions x 3 |
// spine xz | direction xz), then the last 60 emitted fp32 hips positions (slot = emitted % 60).  All-zero bytes = no frame seen.
//
// The frame-level arithmetic - the fit's row, the root from the fitted series, the central differences, the toe chain - is ingest_body.h,
// shared with the whole-clip form (ingest_clip.hip), which emits every frame of a clip and mirrors.
//
// Inherited from the reference: between([0,0,1], d) is singular for a character facing exactly -z; contacts flip at a hard threshold.
#include "ingest_body.h"

namespace mocha {

namespace {
constexpr int NB = MOCHA_MAX_BONES, RING = INGEST_RING;
constexpr int ST_REF = 2, ST_RING = ST_REF + NB * 4, ST_HIPS = ST_RING + RING * INGEST_FRAME_DOUBLES;
constexpr int FR_Q = 0, FR_P = NB * 4, FR_SP = NB * 7, FR_DIR = NB * 7 + 2;
static_assert(ST_HIPS + 180 == INGEST_STATE_DOUBLES, "ingest state layout");
constexpr int NROOT = 8, NVEL = 6;               // frames t-4 .. t+3 with a root, frames t-3 .. t+2 with velocities

// the fit of one series (word `off` of every ring frame) at frame j of a prefix of n frames: rows (W,W)
__device__ inline double fit(const double* __restrict__ rows, int W, const double* ring, int off, int j, int n) {
    int start, row;
    ingest_fit_row(W, j, n, start, row);
    double acc = 0.0;
    for (int k = 0; k < W; ++k) acc += rows[row * W + k] * ring[(size_t)((start + k) % RING) * INGEST_FRAME_DOUBLES + off];
    return acc;
}
}  // namespace

__global__ __launch_bounds__(64) void mocha_live_ingest(IngestParams p) {
    __shared__ dq s_q[NB];                       // store: the frame's local quaternions, then lane 0's global ones
    __shared__ d3 s_p[NB];
    __shared__ double s_fit[NROOT][4];
    __shared__ d3 s_rootp[NROOT], s_hipp[NROOT];
    __shared__ dq s_rootq[NROOT], s_hipq[NROOT];
    __shared__ d3 s_vel[NVEL][NB], s_ang[NVEL][NB];
    __shared__ int s_vote[MOCHA_MAX_CONTACT][NVEL];
    const int s = blockIdx.x, tid = threadIdx.x, V = p.V, J = p.V + 1;
    double* S = p.state + (size_t)s * INGEST_STATE_DOUBLES;
    long long* F = reinterpret_cast<long long*>(S);
    long long n0 = F[0], em = F[1];
    if (n0 < 0 || em < 0 || em > n0) { n0 = 0; em = 0; }         // a buffer that was never reset: start over
    double* ring = S + ST_RING;
    double* fr = ring + (size_t)(n0 % RING) * INGEST_FRAME_DOUBLES;
    __syncthreads();                                            // every lane has read the counters
    // ---- store
    if (tid < V) {
        dq q;
        if (p.euler) {
            const float* e = p.rot + ((size_t)s * V + tid) * 3;
            dq a[3];
            for (int k = 0; k < 3; ++k) {
                const double r = (double)e[k] * (3.141592653589793 / 180.0);
                const double c = cos(r / 2.0), sn = sin(r / 2.0);
                a[k] = {c, p.order[k] == 0 ? sn : 0.0, p.order[k] == 1 ? sn : 0.0, p.order[k] == 2 ? sn : 0.0};
            }
            q = qmul(a[0], qmul(a[1], a[2]));
        } else {
            const float* e = p.rot + ((size_t)s * V + tid) * 4;
            q = {(double)e[0], (double)e[1], (double)e[2], (double)e[3]};
        }
        double* ref = S + ST_REF + tid * 4;
        if (n0 > 0 && q.w * ref[0] + q.x * ref[1] + q.y * ref[2] + q.z * ref[3] < 0.0) q = {-q.w, -q.x, -q.y, -q.z};
        const float* x = p.pos + ((size_t)s * V + tid) * 3;
        const d3 lp = {(double)x[0] * p.scale, (double)x[1] * p.scale, (double)x[2] * p.scale};
        stq(ref, q);
        stq(fr + FR_Q + tid * 4, q);
        st3(fr + FR_P + tid * 3, lp);
        s_q[tid] = q; s_p[tid] = lp;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < V; ++v) {                            // parents[v] < v: checked on the host
            const int pa = p.parents[v];
            s_p[v] = qrot(s_q[pa], s_p[v]) + s_p[pa];
            s_q[v] = qmul(s_q[pa], s_q[v]);
        }
        const d3 sp = s_p[p.roles[0]];
        const d3 a = (s_p[p.roles[1]] - s_p[p.roles[2]]) + (s_p[p.roles[3]] - s_p[p.roles[4]]);
        const double dx = -a.z, dz = a.x;                        // [1,0,1] * cross(across, [0,1,0])
        const double l = sqrt(dx * dx + dz * dz);
        fr[FR_SP] = sp.x; fr[FR_SP + 1] = sp.z;
        fr[FR_DIR] = dx / l; fr[FR_DIR + 1] = dz / l;
        F[0] = n0 + 1;
        if (n0 + 1 < INGEST_FIRST) p.have[s] = 0;
    }
    if (n0 + 1 < INGEST_FIRST) return;                          // uniform: the stream is warming, its output rows stay
    __syncthreads();                                            // the new frame is visible to the workgroup
    // The prefix length as an int: every frame index below lies within RING of it and is only compared with it, with the window half
    // widths, and reduced modulo RING - so a long-running stream's count is folded to a small one congruent to it (100000 % RING == 0).
    static_assert(100000 % RING == 0, "fold keeps the ring slot");
    const int n = n0 + 1 < 100000 ? (int)(n0 + 1) : 100000 + (int)((n0 + 1 - 100000) % RING);
    const int t = n - 1 - p.lookahead, lo = t - 4, hi = min(t + 3, n - 1), nroot = hi - lo + 1;
    // ---- root: fits, then rotation and root-local hips per frame
    if (tid < nroot * 4) {
        const int k = tid >> 2, c = tid & 3;
        s_fit[k][c] = c < 2 ? fit(p.rows15, 15, ring, FR_SP + c, lo + k, n) : fit(p.rows31, 31, ring, FR_DIR + c - 2, lo + k, n);
    }
    __syncthreads();
    if (tid < nroot) {
        d3 rp;
        dq R;
        ingest_root(s_fit[tid][0], s_fit[tid][1], s_fit[tid][2], s_fit[tid][3], rp, R);
        const double* f = ring + (size_t)((lo + tid) % RING) * INGEST_FRAME_DOUBLES;
        const dq Ri = qinv(R);
        s_rootp[tid] = rp; s_rootq[tid] = R;
        s_hipp[tid] = qrot(Ri, ld3(f + FR_P) - rp);
        s_hipq[tid] = qmul(Ri, ldq(f + FR_Q));
    }
    __syncthreads();
    auto P = [&](int j, int b) -> d3 {
        return b == 0 ? s_rootp[j - lo] : b == 1 ? s_hipp[j - lo] : ld3(ring + (size_t)(j % RING) * INGEST_FRAME_DOUBLES + FR_P + (b - 1) * 3);
    };
    auto Q = [&](int j, int b) -> dq {
        return b == 0 ? s_rootq[j - lo] : b == 1 ? s_hipq[j - lo] : ldq(ring + (size_t)(j % RING) * INGEST_FRAME_DOUBLES + FR_Q + (b - 1) * 4);
    };
    // ---- velocities: frames t-3 .. min(t+2, n-1); the prefix's last frame is extrapolated from the two before it
    const int vlo = t - 3, vhi = min(t + 2, n - 1), vcen = min(vhi, n - 2);
    const double f60 = p.fps;
    for (int i = tid; i < (vcen - vlo + 1) * J; i += 64) {
        const int j = vlo + i / J, b = i % J;
        s_vel[j - vlo][b] = ingest_central_vel(P, j, b, f60);
        s_ang[j - vlo][b] = ingest_central_ang(Q, j, b, f60);
    }
    __syncthreads();
    if (vhi == n - 1) {                                          // lookahead <= 2: frames n-3, n-2 are in the window
        const int e = n - 1 - vlo;
        for (int b = tid; b < J; b += 64) {
            s_vel[e][b] = s_vel[e - 1][b] + (s_vel[e - 1][b] - s_vel[e - 2][b]);
            s_ang[e][b] = s_ang[e - 1][b] + (s_ang[e - 1][b] - s_ang[e - 2][b]);
        }
    }
    __syncthreads();
    // ---- contacts: lane (toe, frame of the vote)
    if (tid < p.n_contact * NVEL) {
        const int ci = tid / NVEL, j = min(t - 3 + tid % NVEL, n - 1);
        auto Vel = [&](int f, int b) -> d3 { return s_vel[f - vlo][b]; };
        auto Ang = [&](int f, int b) -> d3 { return s_ang[f - vlo][b]; };
        s_vote[ci][tid % NVEL] = ingest_toe_speed(p.parents, p.contact_bones[ci], j, P, Q, Vel, Ang) < p.threshold ? 1 : 0;
    }
    __syncthreads();
    // ---- emit frame t
    for (int b = tid; b < J; b += 64) {
        const d3 op = P(t, b), ov = s_vel[t - vlo][b], oa = s_ang[t - vlo][b];
        const dq oq = Q(t, b);
        float* yr = p.Yrot + ((size_t)s * J + b) * 4;
        float* yp = p.Ypos + ((size_t)s * J + b) * 3;
        float* yv = p.Yvel + ((size_t)s * J + b) * 3;
        float* ya = p.Yang + ((size_t)s * J + b) * 3;
        yr[0] = (float)oq.w; yr[1] = (float)oq.x; yr[2] = (float)oq.y; yr[3] = (float)oq.z;
        yp[0] = (float)op.x; yp[1] = (float)op.y; yp[2] = (float)op.z;
        yv[0] = (float)ov.x; yv[1] = (float)ov.y; yv[2] = (float)ov.z;
        ya[0] = (float)oa.x; ya[1] = (float)oa.y; ya[2] = (float)oa.z;
    }
    if (tid == 0) {
        for (int ci = 0; ci < p.n_contact; ++ci) {
            int votes = 0;
            for (int k = 0; k < NVEL; ++k) votes += s_vote[ci][k];
            p.contact[(size_t)s * p.n_contact + ci] = votes >= 3 ? 1 : 0;
        }
        const dq r32 = {(double)(float)s_rootq[t - lo].w, (double)(float)s_rootq[t - lo].x, (double)(float)s_rootq[t - lo].y,
                        (double)(float)s_rootq[t - lo].z};
        const d3 v0 = s_vel[t - vlo][0], a0 = s_ang[t - vlo][0];
        const d3 rv = qrot(qinv(r32), {(double)(float)v0.x, (double)(float)v0.y, (double)(float)v0.z});
        const d3 ra = qrot(qinv(r32), {(double)(float)a0.x, (double)(float)a0.y, (double)(float)a0.z});
        float* o = p.src_rvel + (size_t)s * 3;
        o[0] = (float)rv.x; o[1] = (float)rv.y; o[2] = (float)rv.z;
        o = p.src_rang + (size_t)s * 3;
        o[0] = (float)ra.x; o[1] = (float)ra.y; o[2] = (float)ra.z;
        // the window's own velocity of bone 1: the last 60 emitted fp32 hips positions, oldest first
        double* hips = S + ST_HIPS;
        const d3 hp = s_hipp[t - lo];
        double* slot = hips + (size_t)(em % 60) * 3;
        slot[0] = (double)(float)hp.x; slot[1] = (double)(float)hp.y; slot[2] = (double)(float)hp.z;
        const long long em1 = em + 1;
        double speed = 0.0;
        if (em1 >= 60) {
            auto H = [&](int k) -> d3 { return ld3(hips + (size_t)((em1 + k) % 60) * 3); };
            auto central = [&](int k) -> d3 { return 0.5 * (H(k + 1) - H(k)) * f60 + 0.5 * (H(k) - H(k - 1)) * f60; };
            const d3 first = central(1) - (central(3) - central(2));
            const d3 last = central(58) + (central(58) - central(57));
            speed = len(first);
            for (int k = 1; k < 59; ++k) speed += len(central(k));
            speed = (speed + len(last)) / 60.0;
        }
        p.src_speed[s] = (float)speed;
        F[1] = em1;
        p.have[s] = 1;
    }
}

hipError_t launch_live_ingest(const IngestParams& p, int S, hipStream_t s) {
    if (S <= 0) return hipSuccess;
    if (p.V < 1 || p.V + 1 > MOCHA_MAX_BONES || p.n_contact < 0 || p.n_contact > MOCHA_MAX_CONTACT || p.lookahead < 0 ||
        p.lookahead > INGEST_MAX_LOOKAHEAD)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_live_ingest, dim3(S), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace mocha
