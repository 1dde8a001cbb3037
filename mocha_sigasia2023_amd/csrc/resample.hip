// The resampler in front of the mocap front end (mocha_resample_clips, mocha_resample_step): mocap at a source rate -> unit quaternions and
// positions at the rate the network, the 60-frame windows, the root fits and the bank are fixed to.  The reference has no resampler; the
// interpolation is composed of its own quaternion primitives (resample_body.h): between two source frames the rotation turns at the constant
// angular velocity that generate_database.py:148-149 assigns to the interval, positions move linearly.  Float64 on the fp32 inputs, rounded
// to fp32 once at the output.
//   mocha_clip_resample     thread (output frame, joint): the clip by bisection in the output offsets, t = k num in 64 bits, two unrolled
//                           quaternions and two positions of the workspace that mocha_clip_quat / mocha_clip_unroll (ingest_clip.hip) filled,
//                           one quaternion and one position out.  num / den per clip: files of different rates share a call.  An output
//                           that falls on a source frame (a == 0) is that frame and reads no other: the last output of a clip may sit
//                           on its last frame, and nothing crosses a clip boundary.
//   mocha_resample_step_k   workgroup = stream, lane = joint: converts the new frame as mocha_clip_quat does, unrolls it against the stored
//                           one, writes the outputs the host scheduled (k_first, count: integers alone) and keeps the new frame.
#include "resample_body.h"

namespace mocha {

namespace {
__device__ inline void store_joint(float* __restrict__ yr, float* __restrict__ yp, dq q, d3 x) {
    yr[0] = (float)q.w; yr[1] = (float)q.x; yr[2] = (float)q.y; yr[3] = (float)q.z;
    yp[0] = (float)x.x; yp[1] = (float)x.y; yp[2] = (float)x.z;
}
}  // namespace

__global__ __launch_bounds__(256) void mocha_clip_resample(ClipResampleParams p) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.F_out * p.V) return;
    const int f = (int)(idx / p.V), v = (int)(idx % p.V);
    int lo = 0, hi = p.C;                                        // out_off[c] <= f < out_off[c+1]
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (p.out_off[m] <= f) lo = m; else hi = m;
    }
    const int c = lo, first = p.in_off[c], n = p.in_off[c + 1] - first;
    long long i;
    double a;
    resample_at(f - p.out_off[c], p.num[c], p.den[c], i, a);
    if (i >= n) return;                                          // never: the host checked out_off against the output counts
    const size_t at = ((size_t)first + (size_t)i) * p.V + v;
    dq q = ldq(p.q + at * 4);
    d3 x = ld3(p.p + at * 3);
    if (a != 0.0 && i + 1 < n) {
        const size_t nx = at + p.V;
        const ResampledJoint r = resample_between(q, ldq(p.q + nx * 4), x, ld3(p.p + nx * 3), a);
        q = r.q; x = r.p;
    }
    store_joint(p.rot_out + idx * 4, p.pos_out + idx * 3, q, x);
}

hipError_t launch_clip_resample(const ClipResampleParams& p, hipStream_t s) {
    if (p.F_out <= 0 || p.C <= 0) return hipSuccess;
    if (p.V < 1 || p.V + 1 > MOCHA_MAX_BONES || p.F_out > 0x7fffffffll) return hipErrorInvalidValue;
    const size_t blocks = ((size_t)p.F_out * p.V + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_clip_resample, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void mocha_resample_step_k(ResampleStepParams p) {
    const int s = blockIdx.x, v = threadIdx.x;
    double* st = p.state + (size_t)s * RESAMPLE_STATE_DOUBLES;
    const bool fresh = st[0] != 0.0 || st[1] == 0.0;             // read by every lane before lane 0 rewrites the two words
    __syncthreads();
    if (v < p.V) {
        double* js = st + 2 + v * RESAMPLE_JOINT_DOUBLES;        // previous unrolled quaternion | position | unroll sign
        const size_t in = (size_t)s * p.V + v;
        const dq raw = resample_raw_quat(p.rot + in * (p.euler ? 3 : 4), p.euler, p.order[0], p.order[1], p.order[2]);
        const float* xp = p.pos + in * 3;
        const d3 p1 = {(double)xp[0], (double)xp[1], (double)xp[2]};
        const dq q0 = ldq(js);
        const d3 p0 = ld3(js + 4);
        double sg = 1.0;
        if (!fresh) {
            // mocha_clip_unroll negates a frame iff an odd number of the RAW dot products before it is negative; the stored frame is the
            // raw one times its sign, negation is exact, so the raw dot product's sign is this one's times the stored sign
            const double sg0 = js[7];
            const double d = raw.w * q0.w + raw.x * q0.x + raw.y * q0.y + raw.z * q0.z;
            const bool flip = sg0 < 0.0 ? d > 0.0 : d < 0.0;
            sg = flip ? -sg0 : sg0;
        }
        const dq q1 = {sg * raw.w, sg * raw.x, sg * raw.y, sg * raw.z};
        for (int e = 0; e < p.count; ++e) {
            long long i;
            double a;
            resample_at(p.k_first + e, p.num, p.den, i, a);
            dq q = q1;
            d3 x = p1;
            if (!fresh && a != 0.0) {                            // between the stored frame and the new one
                const ResampledJoint r = resample_between(q0, q1, p0, p1, a);
                q = r.q; x = r.p;
            }
            const size_t out = ((size_t)s * RESAMPLE_MAX_OUT + e) * p.V + v;
            store_joint(p.rot_out + out * 4, p.pos_out + out * 3, q, x);
        }
        stq(js, q1);
        st3(js + 4, p1);
        js[7] = sg;
    }
    if (v == 0) { st[0] = 0.0; st[1] = 1.0; }
}

hipError_t launch_resample_step(const ResampleStepParams& p, int S, hipStream_t s) {
    if (S < 1 || S > 16 || p.V < 1 || p.V + 1 > MOCHA_MAX_BONES || p.count < 0 || p.count > RESAMPLE_MAX_OUT) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mocha_resample_step_k, dim3(S), dim3(64), 0, s, p);
    return hipGetLastError();
}

}  // namespace mocha
