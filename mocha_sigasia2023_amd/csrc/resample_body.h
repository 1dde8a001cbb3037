// The resampler's arithmetic that its whole-clip form (mocha_clip_resample) and its streaming form (mocha_resample_step) share, both in
// resample.hip: where output k of a clip falls between two source frames, and the frame there.  resample_between is deliberately not
// inlined: both kernels call the same machine code, so a stream's outputs are the whole clip's bit for bit.
#pragma once
#include "kernels.h"
#include "quat64.h"

namespace mocha {

// output k at a step of num / den source frames: t = k num in 64 bits, source frame i = t div den, a = (t mod den) / den in [0, 1)
__device__ inline void resample_at(long long k, int num, int den, long long& i, double& a) {
    const long long t = k * (long long)num;
    i = t / den;
    a = (double)(t % den) / (double)den;
}

// the frame at a in (0, 1) between (q0, p0) and (q1, p1), q unrolled along time:
//   mul(from_scaled_angle_axis(a * to_scaled_angle_axis(abs(mul_inv(q1, q0)))), q0)      quat.py:18-19, 112-126, 149-164, eps = 1e-5
//   p0 + a * (p1 - p0)
// i.e. rotation at the constant angular velocity the reference's difference formula gives the interval (generate_database.py:148-149)
struct ResampledJoint { dq q; d3 p; };
__device__ inline __noinline__ ResampledJoint resample_between(dq q0, dq q1, d3 p0, d3 p1, double a) {
    dq d = qmul(q1, qinv(q0));
    if (!(d.w > 0.0)) d = {-d.w, -d.x, -d.y, -d.z};                                        // quat.abs
    return {qmul(from_scaled_angle_axis(a * to_scaled_angle_axis(d)), q0), p0 + a * (p1 - p0)};
}

// quat.from_euler(np.radians(e), order) as mocha_clip_quat writes it (ingest_clip.hip), or the quaternion as given
__device__ inline dq resample_axis_quat(float degrees, int axis) {
    const double r = (double)degrees * (3.141592653589793 / 180.0);
    const double c = cos(r / 2.0), sn = sin(r / 2.0);
    return {c, axis == 0 ? sn : 0.0, axis == 1 ? sn : 0.0, axis == 2 ? sn : 0.0};
}
__device__ inline dq resample_raw_quat(const float* __restrict__ e, int euler, int o0, int o1, int o2) {
    if (!euler) return {(double)e[0], (double)e[1], (double)e[2], (double)e[3]};
    return qmul(resample_axis_quat(e[0], o0), qmul(resample_axis_quat(e[1], o1), resample_axis_quat(e[2], o2)));
}

}  // namespace mocha
