// float64 vectors and quaternions (w,x,y,z) as motion/quat.py of the reference writes them: what the post-processing frame loop, the
// inertializer (postprocess.hip) and the mocap front end (ingest.hip) share.
#pragma once
#include <hip/hip_runtime.h>

namespace mocha {

struct d3 { double x, y, z; };
struct dq { double w, x, y, z; };

__device__ inline d3 operator+(d3 a, d3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ inline d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline d3 operator*(d3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ inline d3 operator*(double s, d3 a) { return {a.x * s, a.y * s, a.z * s}; }
__device__ inline double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ inline double len(d3 a) { return sqrt(dot(a, a)); }
__device__ inline d3 normalize(d3 a) { return a * (1.0 / (len(a) + 1e-8)); }                  // quat.py:15-16 (x / (|x| + eps))
__device__ inline dq qmul(dq x, dq y) {                                                        // quat.py:112-120
    return {y.w * x.w - y.x * x.x - y.y * x.y - y.z * x.z, y.w * x.x + y.x * x.w - y.y * x.z + y.z * x.y,
            y.w * x.y + y.x * x.z + y.y * x.w - y.z * x.x, y.w * x.z - y.x * x.y + y.y * x.x + y.z * x.w};
}
__device__ inline dq qinv(dq q) { return {q.w, -q.x, -q.y, -q.z}; }
__device__ inline d3 qrot(dq q, d3 v) {                                                        // quat.py:128-130
    const d3 u = {q.x, q.y, q.z};
    const d3 t = 2.0 * cross(u, v);
    return v + q.w * t + cross(u, t);
}
__device__ inline dq from_angle_axis(double angle, d3 axis) {                                  // quat.py:21-25
    const double c = cos(angle / 2.0), s = sin(angle / 2.0);
    return {c, s * axis.x, s * axis.y, s * axis.z};
}
__device__ inline dq from_scaled_angle_axis(d3 v) {                                            // quat.py:154-164
    const d3 x = v * 0.5;
    const double h = len(x);
    if (h < 1e-5) return {1.0, x.x, x.y, x.z};
    const double s = sin(h) / h;
    return {cos(h), s * x.x, s * x.y, s * x.z};
}
__device__ inline double clamp1(double x) { return x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x); }

__device__ inline d3 ld3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ inline dq ldq(const double* p) { return {p[0], p[1], p[2], p[3]}; }
__device__ inline void st3(double* p, d3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ inline void stq(double* p, dq q) { p[0] = q.w; p[1] = q.x; p[2] = q.y; p[3] = q.z; }
__device__ inline d3 to_scaled_angle_axis(dq q) {                                              // quat.py:149-152, 160-161
    const d3 v = {q.x, q.y, q.z};
    const double l = len(v);
    const double h = l < 1e-5 ? 1.0 : atan2(l, q.w) / l;
    return 2.0 * (v * h);
}

}  // namespace mocha
