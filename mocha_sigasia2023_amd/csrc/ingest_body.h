// Frame-level arithmetic of the mocap front end that its streaming form (ingest.hip: a ring of the last frames) and its whole-clip form
// (ingest_clip.hip: the clip's frames in a workspace) share, so that both evaluate the same expressions in the same order: the row of a
// cubic fit, the root bone from the four fitted series, the central differences and the toe chain of fk_vel.  Where a frame's neighbours
// live is the caller's business: bones are read through accessors P(frame, bone) -> d3 and Q(frame, bone) -> dq.
#pragma once
#include "kernels.h"
#include "quat64.h"

namespace mocha {

// savgol_filter(mode='interp') at sample j of n: the window's first sample and the row of the (W,W) fit matrix - the centre row inside,
// the first / last window's own rows within half a window of an end
__device__ inline void ingest_fit_row(int W, int j, int n, int& start, int& row) {
    const int h = W / 2;
    if (j < h) { start = 0; row = j; }
    else if (j > n - 1 - h) { start = n - W; row = j - (n - W); }
    else { start = j - h; row = h; }
}

// root position and rotation from the fitted spine xz and direction xz (generate_database.py:121-124): renormalise,
// normalize(between([0,0,1], d))
__device__ inline void ingest_root(double px, double pz, double dx, double dz, d3& rp, dq& R) {
    const double l = sqrt(dx * dx + dz * dz);
    dx /= l; dz /= l;
    const double w = sqrt(1.0 * (dx * dx + dz * dz)) + dz;       // between([0,0,1], d) = [sqrt(|z|^2 |d|^2) + z.d, cross(z, d)]
    const double m = sqrt(w * w + dx * dx) + 1e-8;               // normalize: x / (|x| + 1e-8)
    R = {w / m, 0.0, dx / m, 0.0};
    rp = {px, 0.0, pz};
}

// central differences at an inner frame j (generate_database.py:138-151)
template <class PF>
__device__ inline d3 ingest_central_vel(PF&& P, int j, int b, double fps) {
    const d3 p0 = P(j - 1, b), p1 = P(j, b), p2 = P(j + 1, b);
    return 0.5 * (p2 - p1) * fps + 0.5 * (p1 - p0) * fps;
}
template <class QF>
__device__ inline d3 ingest_central_ang(QF&& Q, int j, int b, double fps) {
    const dq q0 = Q(j - 1, b), q1 = Q(j, b), q2 = Q(j + 1, b);
    dq a = qmul(q2, qinv(q1)), c = qmul(q1, qinv(q0));
    if (!(a.w > 0.0)) a = {-a.w, -a.x, -a.y, -a.z};              // quat.abs
    if (!(c.w > 0.0)) c = {-c.w, -c.x, -c.y, -c.z};
    return 0.5 * to_scaled_angle_axis(a) * fps + 0.5 * to_scaled_angle_axis(c) * fps;
}

// fk_vel (quat.py:189-204) down the chain of bone `toe` of the (V+1)-bone skeleton at frame j, root bone first: the toe's global speed.
// parents: of the V raw joints.  VF / AF(j, bone): the float64 velocities.  The chain is walked from the toe at every level, so no
// per-thread array is indexed at run time.
template <class PF, class QF, class VF, class AF>
__device__ inline double ingest_toe_speed(const int* parents, int toe, int j, PF&& P, QF&& Q, VF&& Vel, AF&& Ang) {
    int depth = 0;
    for (int b = toe; b > 0 && depth < MOCHA_MAX_CHAIN; b = parents[b - 1] + 1) ++depth;
    d3 gv = Vel(j, 0), ga = Ang(j, 0);
    dq gr = Q(j, 0);
    for (int d = depth - 1; d >= 0; --d) {
        int b = toe;
        for (int u = 0; u < d; ++u) b = parents[b - 1] + 1;
        const d3 lp = qrot(gr, P(j, b));
        const d3 ngv = qrot(gr, Vel(j, b)) + cross(ga, lp) + gv;
        const d3 nga = qrot(gr, Ang(j, b)) + ga;
        gr = qmul(gr, Q(j, b)); gv = ngv; ga = nga;
    }
    return sqrt(gv.x * gv.x + gv.y * gv.y + gv.z * gv.z);
}

}  // namespace mocha
