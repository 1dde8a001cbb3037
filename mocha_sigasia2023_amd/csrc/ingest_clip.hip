// Whole mocap clips through the reference's clip preparation (mocha_ingest_clips) and its windowing (mocha_clip_windows):
// process_data of preprocess/generate_database.py:86-177 with mirror = False / True, and divide_clip(divide=True) (:57-84), parallel over
// frames.  The arithmetic per frame is that of the streaming form (ingest.hip), shared through ingest_body.h; what differs is where a frame's
// neighbours come from: the clip's own frames in a float64 workspace instead of a ring, so every frame of a clip is emitted - frame 0 with
// v[0] = v[1] - (v[3] - v[2]), the last with v[-1] = v[-2] + (v[-2] - v[-3]), the fits' first / last window rows at both ends.
//
// C clips share a call, concatenated along the frame axis; every kernel finds a frame's clip by bisection in the offsets and reads no
// frame outside it.  The launches, in order (launch_clip_ingest):
//   0 mocha_clip_quat     thread (frame, joint): from_euler (quat.py:57-67, degrees -> radians as np.radians) or the quaternion as given;
//                         positions x unit scale.
//   1 mocha_clip_unroll   workgroup (clip, joint): quat.unroll (quat.py:135-141) as a parity scan.  Negation is exact, so frame i is negated
//                         iff an odd number of the raw dot products dot(raw_k, raw_k-1), k <= i, is negative (a dot of exactly 0 does not
//                         flip).  A lane takes CLIP_SCAN_CHUNK consecutive frames, the wave combines the lanes' parities with a ballot and
//                         the popcount of the lower lanes, the workgroup carries the parity across its waves and across its passes of
//                         CLIP_SCAN_THREADS x CLIP_SCAN_CHUNK frames.
//   2 mocha_clip_mirror   mirrored clips only, lane (frame, joint): forward kinematics by tree depth in LDS, mirror_pos * gpos[map],
//                         from_xform(mirror_rot * to_xform(grot[map])) (quat.py:27-40, 69-94), quat.ik (:175-187) with the same parents.
//   3 mocha_clip_unroll   again, on the mirrored clips (generate_database.py:95).
//   4 mocha_clip_series   lane (frame, joint): forward kinematics, the spine joint on xz and the projected, normalised across-direction.
//   5 mocha_clip_root     lane (frame, series): the 15-tap / 31-tap cubic fit rows (first window, centre row, last window), then per frame
//                         renormalise, normalize(between(z, d)), hips made root-local.
//   6 mocha_clip_vel      lane (frame, bone of V+1): central differences and the quat.abs / to_scaled_angle_axis pair, a clip's first and
//                         last frame from recomputed neighbours; the fp32 outputs pos / vel / rot / ang; then lane (frame, toe): fk_vel down
//                         the toe chain on the float64 velocities in LDS, speed < threshold.
//   7 mocha_clip_vote     thread (frame, toe): at least 3 of the flags t-3 .. t+2, indices clamped to the clip.
// Per-joint state that forward kinematics indexes by a run-time parent lives in LDS, never in per-thread arrays.
#include "ingest_body.h"

namespace mocha {

namespace {
constexpr int NB = MOCHA_MAX_BONES, FPB = 8;     // frames per workgroup of the (frame, joint) kernels: 8 x 32 lanes

// the clip that holds frame f: offsets[c] <= f < offsets[c+1]
__device__ inline int clip_of(const int* __restrict__ off, int C, int f) {
    int lo = 0, hi = C;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (off[m] <= f) lo = m; else hi = m;
    }
    return lo;
}

// the fit of series `off` (a word of every frame's four) at frame j of a clip of n frames whose series start at `ser`: rows (W,W)
__device__ inline double fit(const double* __restrict__ rows, int W, const double* __restrict__ ser, int off, int j, int n) {
    int start, row;
    ingest_fit_row(W, j, n, start, row);
    double acc = 0.0;
    for (int k = 0; k < W; ++k) acc += rows[row * W + k] * ser[(size_t)(start + k) * 4 + off];
    return acc;
}

// forward kinematics (quat.py:166-173) of FPB frames in LDS, lanes = joints, one tree level per step; every lane of the workgroup calls
__device__ inline void fk_levels(dq (*sq)[NB], d3 (*sp)[NB], int fr, int v, bool act, const ClipParams& p) {
    for (int d = 1; d <= p.max_depth; ++d) {
        if (act && p.depth[v] == d) {
            const int pa = p.parents[v];
            sp[fr][v] = qrot(sq[fr][pa], sp[fr][v]) + sp[fr][pa];
            sq[fr][v] = qmul(sq[fr][pa], sq[fr][v]);
        }
        __syncthreads();
    }
}
}  // namespace

__global__ __launch_bounds__(256) void mocha_clip_quat(ClipParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.F * p.V) return;
    dq q;
    if (p.euler) {
        const float* e = p.rot + i * 3;
        dq a[3];
        for (int k = 0; k < 3; ++k) {
            const double r = (double)e[k] * (3.141592653589793 / 180.0);
            const double c = cos(r / 2.0), sn = sin(r / 2.0);
            a[k] = {c, p.order[k] == 0 ? sn : 0.0, p.order[k] == 1 ? sn : 0.0, p.order[k] == 2 ? sn : 0.0};
        }
        q = qmul(a[0], qmul(a[1], a[2]));
    } else {
        const float* e = p.rot + i * 4;
        q = {(double)e[0], (double)e[1], (double)e[2], (double)e[3]};
    }
    const float* x = p.pos + i * 3;
    stq(p.qraw + i * 4, q);
    st3(p.p + i * 3, {(double)x[0] * p.scale, (double)x[1] * p.scale, (double)x[2] * p.scale});
}

// grid (C, V): qraw -> q for one joint of one clip
__global__ __launch_bounds__(CLIP_SCAN_THREADS) void mocha_clip_unroll(ClipParams p, int mirrored_only) {
    constexpr int CH = CLIP_SCAN_CHUNK, NT = CLIP_SCAN_THREADS, NW = NT / 64;
    __shared__ unsigned s_wave[NW];
    const int c = blockIdx.x, v = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (mirrored_only && !(p.flags && p.flags[c])) return;      // uniform
    const int lo = p.offsets[c], n = p.offsets[c + 1] - lo;
    const double* src = p.qraw + ((size_t)lo * p.V + v) * 4;
    double* dst = p.q + ((size_t)lo * p.V + v) * 4;
    const size_t stride = (size_t)p.V * 4;
    unsigned carry = 0;                                          // parity of the flips before this pass
    for (int base = 0; base < n; base += NT * CH) {
        const int i0 = base + tid * CH;
        unsigned par = 0, bits = 0;                              // bit k: parity of the flips of frames i0 .. i0+k
        dq prev = {0.0, 0.0, 0.0, 0.0};
        if (i0 > 0 && i0 < n) prev = ldq(src + (size_t)(i0 - 1) * stride);
        for (int k = 0; k < CH; ++k) {
            const int i = i0 + k;
            if (i < n) {
                const dq cur = ldq(src + (size_t)i * stride);
                if (i > 0 && cur.w * prev.w + cur.x * prev.x + cur.y * prev.y + cur.z * prev.z < 0.0) par ^= 1u;
                bits |= par << k;
                prev = cur;
            }
        }
        const unsigned long long vote = __ballot(par != 0);
        const unsigned below = (unsigned)__popcll(vote & ((1ull << lane) - 1ull)) & 1u;
        if (lane == 0) s_wave[wave] = (unsigned)__popcll(vote) & 1u;
        __syncthreads();
        unsigned before = carry, total = 0;
        for (int w = 0; w < NW; ++w) { if (w < wave) before ^= s_wave[w]; total ^= s_wave[w]; }
        before ^= below;
        for (int k = 0; k < CH; ++k) {
            const int i = i0 + k;
            if (i < n) {
                const dq cur = ldq(src + (size_t)i * stride);
                const double sg = ((before ^ (bits >> k)) & 1u) ? -1.0 : 1.0;
                stq(dst + (size_t)i * stride, {sg * cur.w, sg * cur.x, sg * cur.y, sg * cur.z});
            }
        }
        carry ^= total;
        __syncthreads();                                         // s_wave is rewritten by the next pass
    }
}

// mirrored clips: q, p -> qraw, p (animation_mirror); the second unroll makes q of qraw
__global__ __launch_bounds__(FPB * NB) void mocha_clip_mirror(ClipParams p) {
    __shared__ dq s_q[FPB][NB], s_mq[FPB][NB];
    __shared__ d3 s_p[FPB][NB], s_mp[FPB][NB];
    const int fr = threadIdx.x / NB, v = threadIdx.x % NB, f = blockIdx.x * FPB + fr;
    bool act = f < p.F && v < p.V;
    if (act) act = p.flags[clip_of(p.offsets, p.C, f)] != 0;
    const size_t at = (size_t)f * p.V + v;
    if (act) { s_q[fr][v] = ldq(p.q + at * 4); s_p[fr][v] = ld3(p.p + at * 3); }
    __syncthreads();
    fk_levels(s_q, s_p, fr, v, act, p);
    if (act) {
        const int m = p.map[v];
        const d3 g = s_p[fr][m];
        s_mp[fr][v] = {-g.x, g.y, g.z};                          // mirror_pos = [-1, 1, 1]
        const dq r = s_q[fr][m];
        // to_xform (quat.py:27-40)
        const double x2 = r.x + r.x, y2 = r.y + r.y, z2 = r.z + r.z;
        const double xx = r.x * x2, yy = r.y * y2, wx = r.w * x2;
        const double xy = r.x * y2, yz = r.y * z2, wy = r.w * y2;
        const double xz = r.x * z2, zz = r.z * z2, wz = r.w * z2;
        // mirror_rot = [[-1,-1,1],[1,1,-1],[1,1,-1]], element by element
        const double m00 = -(1.0 - (yy + zz)), m01 = -(xy - wz), m02 = xz + wy;
        const double m10 = xy + wz, m11 = 1.0 - (xx + zz), m12 = -(yz - wx);
        const double m20 = xz - wy, m21 = yz + wx, m22 = -(1.0 - (xx + yy));
        dq o;                                                    // from_xform (quat.py:69-94)
        if (m22 < 0.0) {
            if (m00 > m11) o = {m21 - m12, 1.0 + m00 - m11 - m22, m10 + m01, m02 + m20};
            else o = {m02 - m20, m10 + m01, 1.0 - m00 + m11 - m22, m21 + m12};
        } else {
            if (m00 < -m11) o = {m10 - m01, m02 + m20, m21 + m12, 1.0 - m00 - m11 + m22};
            else o = {1.0 + m00 + m11 + m22, m21 - m12, m02 - m20, m10 - m01};
        }
        const double l = sqrt(o.w * o.w + o.x * o.x + o.y * o.y + o.z * o.z) + 1e-8;
        s_mq[fr][v] = {o.w / l, o.x / l, o.y / l, o.z / l};
    }
    __syncthreads();
    if (act) {                                                   // quat.ik
        dq lq = s_mq[fr][v];
        d3 lp = s_mp[fr][v];
        if (v > 0) {
            const int pa = p.parents[v];
            const dq pi = qinv(s_mq[fr][pa]);
            lq = qmul(pi, s_mq[fr][v]);
            lp = qrot(pi, s_mp[fr][v] - s_mp[fr][pa]);
        }
        stq(p.qraw + at * 4, lq);
        st3(p.p + at * 3, lp);
    }
}

__global__ __launch_bounds__(FPB * NB) void mocha_clip_series(ClipParams p) {
    __shared__ dq s_q[FPB][NB];
    __shared__ d3 s_p[FPB][NB];
    const int fr = threadIdx.x / NB, v = threadIdx.x % NB, f = blockIdx.x * FPB + fr;
    const bool act = f < p.F && v < p.V;
    const size_t at = (size_t)f * p.V + v;
    if (act) { s_q[fr][v] = ldq(p.q + at * 4); s_p[fr][v] = ld3(p.p + at * 3); }
    __syncthreads();
    fk_levels(s_q, s_p, fr, v, act, p);
    if (act && v == 0) {
        const d3 sp = s_p[fr][p.roles[0]];
        const d3 a = (s_p[fr][p.roles[1]] - s_p[fr][p.roles[2]]) + (s_p[fr][p.roles[3]] - s_p[fr][p.roles[4]]);
        const double dx = -a.z, dz = a.x;                        // [1,0,1] * cross(across, [0,1,0])
        const double l = sqrt(dx * dx + dz * dz);
        double* o = p.series + (size_t)f * 4;
        o[0] = sp.x; o[1] = sp.z; o[2] = dx / l; o[3] = dz / l;
    }
}

__global__ __launch_bounds__(256) void mocha_clip_root(ClipParams p) {
    __shared__ double s_fit[64][4];
    const int fr = threadIdx.x >> 2, c = threadIdx.x & 3, f = blockIdx.x * 64 + fr;
    int lo = 0;
    if (f < p.F) {
        const int ci = clip_of(p.offsets, p.C, f);
        lo = p.offsets[ci];
        const int n = p.offsets[ci + 1] - lo;
        const double* ser = p.series + (size_t)lo * 4;
        s_fit[fr][c] = c < 2 ? fit(p.rows15, 15, ser, c, f - lo, n) : fit(p.rows31, 31, ser, c, f - lo, n);
    }
    __syncthreads();
    if (f < p.F && c == 0) {
        d3 rp;
        dq R;
        ingest_root(s_fit[fr][0], s_fit[fr][1], s_fit[fr][2], s_fit[fr][3], rp, R);
        const dq Ri = qinv(R);
        double* o = p.root + (size_t)f * CLIP_ROOT_DOUBLES;
        o[0] = rp.x; o[1] = rp.z;
        stq(o + 2, R);
        st3(o + 6, qrot(Ri, ld3(p.p + (size_t)f * p.V * 3) - rp));
        stq(o + 9, qmul(Ri, ldq(p.q + (size_t)f * p.V * 4)));
    }
}

namespace {
// bone b of the (V+1)-bone skeleton at frame f: the root bone, the root-local hips, or a raw joint
__device__ inline d3 bone_p(const ClipParams& p, int f, int b) {
    const double* r = p.root + (size_t)f * CLIP_ROOT_DOUBLES;
    if (b == 0) return {r[0], 0.0, r[1]};
    if (b == 1) return ld3(r + 6);
    return ld3(p.p + ((size_t)f * p.V + (b - 1)) * 3);
}
__device__ inline dq bone_q(const ClipParams& p, int f, int b) {
    const double* r = p.root + (size_t)f * CLIP_ROOT_DOUBLES;
    if (b == 0) return ldq(r + 2);
    if (b == 1) return ldq(r + 9);
    return ldq(p.q + ((size_t)f * p.V + (b - 1)) * 4);
}
__device__ inline d3 central_v(const ClipParams& p, int f, int b) {
    return ingest_central_vel([&](int j, int k) -> d3 { return bone_p(p, j, k); }, f, b, p.fps);
}
__device__ inline d3 central_a(const ClipParams& p, int f, int b) {
    return ingest_central_ang([&](int j, int k) -> dq { return bone_q(p, j, k); }, f, b, p.fps);
}
}  // namespace

__global__ __launch_bounds__(FPB * NB) void mocha_clip_vel(ClipParams p) {
    __shared__ d3 s_vel[FPB][NB], s_ang[FPB][NB];
    const int fr = threadIdx.x / NB, b = threadIdx.x % NB, f = blockIdx.x * FPB + fr, J = p.V + 1;
    if (f < p.F && b < J) {
        const int ci = clip_of(p.offsets, p.C, f);
        const int lo = p.offsets[ci], hi = p.offsets[ci + 1] - 1;     // the clip's first and last frame: both >= 31 frames apart
        d3 v, a;
        if (f == lo) {
            v = central_v(p, lo + 1, b) - (central_v(p, lo + 3, b) - central_v(p, lo + 2, b));
            a = central_a(p, lo + 1, b) - (central_a(p, lo + 3, b) - central_a(p, lo + 2, b));
        } else if (f == hi) {
            const d3 v2 = central_v(p, hi - 1, b), a2 = central_a(p, hi - 1, b);
            v = v2 + (v2 - central_v(p, hi - 2, b));
            a = a2 + (a2 - central_a(p, hi - 2, b));
        } else {
            v = central_v(p, f, b);
            a = central_a(p, f, b);
        }
        s_vel[fr][b] = v; s_ang[fr][b] = a;
        const d3 op = bone_p(p, f, b);
        const dq oq = bone_q(p, f, b);
        const size_t at = (size_t)f * J + b;
        float* yr = p.out_rot + at * 4;
        float* yp = p.out_pos + at * 3;
        float* yv = p.out_vel + at * 3;
        float* ya = p.out_ang + at * 3;
        yr[0] = (float)oq.w; yr[1] = (float)oq.x; yr[2] = (float)oq.y; yr[3] = (float)oq.z;
        yp[0] = (float)op.x; yp[1] = (float)op.y; yp[2] = (float)op.z;
        yv[0] = (float)v.x; yv[1] = (float)v.y; yv[2] = (float)v.z;
        ya[0] = (float)a.x; ya[1] = (float)a.y; ya[2] = (float)a.z;
    }
    __syncthreads();
    // ---- toe speeds: lane (frame, toe), fk_vel (quat.py:189-204) down the toe's chain, the chain walked from the toe at every level
    if (threadIdx.x < FPB * p.n_contact) {
        const int cfr = threadIdx.x / p.n_contact, ci = threadIdx.x % p.n_contact, cf = blockIdx.x * FPB + cfr;
        if (cf < p.F) {
            const double speed = ingest_toe_speed(
                p.parents, p.contact_bones[ci], cf, [&](int j, int k) -> d3 { return bone_p(p, j, k); },
                [&](int j, int k) -> dq { return bone_q(p, j, k); }, [&](int, int k) -> d3 { return s_vel[cfr][k]; },
                [&](int, int k) -> d3 { return s_ang[cfr][k]; });
            p.below[(size_t)cf * MOCHA_MAX_CONTACT + ci] = speed < p.threshold ? 1 : 0;
        }
    }
}

__global__ __launch_bounds__(256) void mocha_clip_vote(ClipParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)p.F * p.n_contact) return;
    const int f = (int)(i / p.n_contact), ci = (int)(i % p.n_contact);
    const int c = clip_of(p.offsets, p.C, f);
    const int lo = p.offsets[c], hi = p.offsets[c + 1] - 1;
    int votes = 0;
    for (int k = -3; k <= 2; ++k) votes += p.below[(size_t)min(max(f + k, lo), hi) * MOCHA_MAX_CONTACT + ci];
    p.out_contact[i] = votes >= 3 ? 1 : 0;
}

hipError_t launch_clip_ingest(const ClipParams& p, int launch, hipStream_t s) {
    if (p.F <= 0 || p.C <= 0) return hipSuccess;
    if (p.V < 1 || p.V + 1 > MOCHA_MAX_BONES || p.n_contact < 0 || p.n_contact > MOCHA_MAX_CONTACT)
        return hipErrorInvalidValue;
    const unsigned per_joint = (unsigned)(((size_t)p.F * p.V + 255) / 256), per_frame = (unsigned)((p.F + FPB - 1) / FPB);
    switch (launch) {
    case 0: hipLaunchKernelGGL(mocha_clip_quat, dim3(per_joint), dim3(256), 0, s, p); break;
    case 1: case 3: hipLaunchKernelGGL(mocha_clip_unroll, dim3(p.C, p.V), dim3(CLIP_SCAN_THREADS), 0, s, p, launch == 3 ? 1 : 0); break;
    case 2: hipLaunchKernelGGL(mocha_clip_mirror, dim3(per_frame), dim3(FPB * NB), 0, s, p); break;
    case 4: hipLaunchKernelGGL(mocha_clip_series, dim3(per_frame), dim3(FPB * NB), 0, s, p); break;
    case 5: hipLaunchKernelGGL(mocha_clip_root, dim3((p.F + 63) / 64), dim3(256), 0, s, p); break;
    case 6: hipLaunchKernelGGL(mocha_clip_vel, dim3(per_frame), dim3(FPB * NB), 0, s, p); break;
    case 7:
        if (p.n_contact == 0) return hipSuccess;
        hipLaunchKernelGGL(mocha_clip_vote, dim3((unsigned)(((size_t)p.F * p.n_contact + 255) / 256)), dim3(256), 0, s, p);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// one thread per (window, frame of the window, bone): 13 floats, and the contacts with bone 0
__global__ __launch_bounds__(256) void mocha_clip_windows_k(ClipWindowParams p) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)p.B * p.window * p.J;
    if (i >= total) return;
    const int bone = (int)(i % p.J), t = (int)(i / p.J % p.window);
    const long long b = (long long)(i / ((size_t)p.J * p.window));
    int lo = 0, hi = p.C;                                        // wcum[c] <= b < wcum[c+1]; clips without a window repeat a value
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (p.wcum[m] <= b) lo = m; else hi = m;
    }
    const int c = lo, first = p.offsets[c], n = p.offsets[c + 1] - first;
    const int j = (int)(b - p.wcum[c]) * p.step, m = min(p.window, n - j);
    const int left = (p.window - m) / 2 + (p.window - m) % 2;
    const bool pad = t < left || t >= left + m;
    const size_t src = (size_t)(first + j + min(max(t - left, 0), m - 1));
    const size_t from = src * p.J + bone;
    for (int k = 0; k < 4; ++k) p.Yrot[i * 4 + k] = p.rot[from * 4 + k];
    for (int k = 0; k < 3; ++k) {
        p.Ypos[i * 3 + k] = p.pos[from * 3 + k];
        p.Yvel[i * 3 + k] = pad ? 0.f : p.vel[from * 3 + k];
        p.Yang[i * 3 + k] = pad ? 0.f : p.ang[from * 3 + k];
    }
    if (bone == 0)
        for (int k = 0; k < p.nc; ++k) p.Ycontact[((size_t)b * p.window + t) * p.nc + k] = p.contact[src * p.nc + k];
}

hipError_t launch_clip_windows(const ClipWindowParams& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    const size_t total = (size_t)p.B * p.window * p.J;
    if ((total + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_clip_windows_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mocha
