// Window featurisation of the demo on the device (test_fullframework.py:141-185):
// forward kinematics with velocities over the bone tree (motion/quat.py:189-204), re-rooting of each
// window on its own last frame (:148-151), every bone expressed in that root frame (:154-158) and the
// features concatenated as [pos 3 | first two columns of the rotation matrix 6 | vel 3 | ang 3] (:180-185).
// One thread per (window, frame); the frame itself is featurize_frame (featurize_body.h, shared with the live ring of live.hip).
#include "kernels.h"
#include "device_utils.h"
#include "featurize_body.h"

namespace mocha {

// no packed fp32 instructions: LDS-fed v_pk_*_f32 with op_sel is the combination that misbehaved in mocha_body_front (pointwise.hip)
__global__ __launch_bounds__(FT) MOCHA_NO_PACKED_F32 void mocha_featurize(const float* __restrict__ Yrot, const float* __restrict__ Ypos,
                                                      const float* __restrict__ Yvel, const float* __restrict__ Yang,
                                                      const int* __restrict__ parents, float* __restrict__ X, int frames /*B*T*/,
                                                      int T, int J) {
    extern __shared__ float g[];                                  // [J][FC][FT]
    const int tid = threadIdx.x;
    const int f = blockIdx.x * FT + tid;
    if (f >= frames) return;
    const int b = f / T;
    const size_t last = ((size_t)b * T + (T - 1)) * J;             // bone 0 of the window's last frame
    const Q Rr = {Yrot[last * 4], Yrot[last * 4 + 1], Yrot[last * 4 + 2], Yrot[last * 4 + 3]};
    const V3 Rp = {Ypos[last * 3], Ypos[last * 3 + 1], Ypos[last * 3 + 2]};
    const V3 Rv = {Yvel[last * 3], Yvel[last * 3 + 1], Yvel[last * 3 + 2]};
    const V3 Ra = {Yang[last * 3], Yang[last * 3 + 1], Yang[last * 3 + 2]};
    featurize_frame([&](int i, Q& lr, V3& lp, V3& lv, V3& la) {
        const size_t e = (size_t)f * J + i;
        lr = {Yrot[e * 4], Yrot[e * 4 + 1], Yrot[e * 4 + 2], Yrot[e * 4 + 3]};
        lp = {Ypos[e * 3], Ypos[e * 3 + 1], Ypos[e * 3 + 2]};
        lv = {Yvel[e * 3], Yvel[e * 3 + 1], Yvel[e * 3 + 2]};
        la = {Yang[e * 3], Yang[e * 3 + 1], Yang[e * 3 + 2]};
    }, parents, J, Rr, Rp, Rv, Ra, X + (size_t)f * J * 15, g, tid);
}

hipError_t featurize_init() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_featurize), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(FEAT_MAX_BONES * FC * FT * sizeof(float)));
}

hipError_t launch_featurize(const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, const int* parents, float* X,
                            int B, int T, int J, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (J > FEAT_MAX_BONES || J < 1) return hipErrorInvalidValue;
    const int frames = B * T;
    hipLaunchKernelGGL(mocha_featurize, dim3((frames + FT - 1) / FT), dim3(FT), (size_t)J * FC * FT * sizeof(float), s, Yrot, Ypos, Yvel,
                       Yang, parents, X, frames, T, J);
    return hipGetLastError();
}

}  // namespace mocha
