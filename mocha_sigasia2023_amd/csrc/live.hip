// Device-resident window ring of a live session (mocha_live_step): per stream the last 60 frames of local bone data - the four arrays
// mocha_featurize takes, root bone first - with a head index and a fill count, all in device memory, so that a caller pushes ONE new
// frame per step instead of re-uploading the 59 it pushed before (test_fullframework.py:126-186 builds every window from the whole clip).
//
//  mocha_live_push     one 64-lane workgroup per stream: stores the new frame at the ring's head, advances head / fill, and writes the
//                      window "oldest ring frame ... newest ring frame" re-rooted on the newest frame as X_raw (60, J, 15) - thread t
//                      featurises window frame t through featurize_frame (featurize_body.h), the body of mocha_featurize, so the bits
//                      are those of mocha_featurize on the materialised window - plus the stream's effective character id (seg[s]
//                      once the ring holds 60 frames, -1 before: the segmented matcher reads no bank row for -1) and valid[s].
//                      With `have` (mocha_live_step_raw), a stream whose have[s] == 0 pushes nothing: counters and ring stay, eff = -1,
//                      valid = 0, its window is featurised as an empty ring's.
//
// Frames of a ring that is still filling are featurised as identity rotations and zeros: finite features, because the streams of a
// step share every later launch.
#include "kernels.h"
#include "device_utils.h"
#include "featurize_body.h"

namespace mocha {

// SLOTS: the step runs on a resident bank, whose slot table ({first row, rows} per slot, n_slots of them) says which ids name a character
// right now; SLOTS = false reads neither argument
template <bool SLOTS>
__global__ __launch_bounds__(FT) MOCHA_NO_PACKED_F32 void mocha_live_push(LiveRing r, const float* __restrict__ Yrot, const float* __restrict__ Ypos,
                                                      const float* __restrict__ Yvel, const float* __restrict__ Yang,
                                                      const int32_t* __restrict__ seg, const int* __restrict__ parents,
                                                      float* __restrict__ X, int32_t* __restrict__ eff, int32_t* __restrict__ valid, int J,
                                                      const int32_t* __restrict__ have, const int* __restrict__ slot_table, int n_slots) {
    extern __shared__ float g[];                                  // [J][FC][FT]
    const int s = blockIdx.x, tid = threadIdx.x;
    const int T = LIVE_WINDOW;
    int32_t* cnt = r.counters + s * 2;                            // {head: the slot the next frame goes to, fill: frames held (<= 60)}
    int head = cnt[0], fill = cnt[1];
    if (head < 0 || head >= T || fill < 0 || fill > T) { head = 0; fill = 0; }       // a buffer that was never reset: start over
    float* rot = r.rot + (size_t)s * T * J * 4;
    float* pos = r.pos + (size_t)s * T * J * 3;
    float* vel = r.vel + (size_t)s * T * J * 3;
    float* ang = r.ang + (size_t)s * T * J * 3;
    __syncthreads();                                              // every thread has read the counters
    const bool none = have && have[s] == 0;                       // uniform: no frame for this stream (mocha_live_step_raw's front end is warming)
    // the new frame into slot `head`
    for (int k = tid; !none && k < J * 4; k += FT) rot[(size_t)head * J * 4 + k] = Yrot[(size_t)s * J * 4 + k];
    for (int k = tid; !none && k < J * 3; k += FT) {
        pos[(size_t)head * J * 3 + k] = Ypos[(size_t)s * J * 3 + k];
        vel[(size_t)head * J * 3 + k] = Yvel[(size_t)s * J * 3 + k];
        ang[(size_t)head * J * 3 + k] = Yang[(size_t)s * J * 3 + k];
    }
    const int nhead = none ? head : head + 1 == T ? 0 : head + 1;
    const int nfill = none ? fill : fill < T ? fill + 1 : T;
    if (tid == 0) {
        if (!none) { cnt[0] = nhead; cnt[1] = nfill; }
        bool full = !none && nfill == T;
        if (SLOTS) {                                              // an empty slot: the frame is in the ring, the stream sits this step out
            const int id = seg[s];
            if (id >= 0 && id < n_slots && slot_table[2 * id + 1] == 0) full = false;
        }
        eff[s] = full ? seg[s] : -1;
        valid[s] = full ? 1 : 0;
    }
    __syncthreads();                                              // the new frame is visible to the workgroup
    if (tid >= T) return;
    // window frame tid (0 oldest .. 59 newest) has age 59 - tid; the frame of age a sits a + 1 slots behind the new head
    const int age = T - 1 - tid;
    const bool held = !none && age < nfill;
    int slot = nhead - 1 - age;
    if (slot < 0) slot += T;
    // bone 0 of the window's last frame: the frame just pushed
    const size_t last = (size_t)s * J;
    auto in = [&](const float* a, size_t i, float d) { return none ? d : a[i]; };       // no frame: the identity root, whatever the staging row holds
    const Q Rr = {in(Yrot, last * 4, 1.f), in(Yrot, last * 4 + 1, 0.f), in(Yrot, last * 4 + 2, 0.f), in(Yrot, last * 4 + 3, 0.f)};
    const V3 Rp = {in(Ypos, last * 3, 0.f), in(Ypos, last * 3 + 1, 0.f), in(Ypos, last * 3 + 2, 0.f)};
    const V3 Rv = {in(Yvel, last * 3, 0.f), in(Yvel, last * 3 + 1, 0.f), in(Yvel, last * 3 + 2, 0.f)};
    const V3 Ra = {in(Yang, last * 3, 0.f), in(Yang, last * 3 + 1, 0.f), in(Yang, last * 3 + 2, 0.f)};
    featurize_frame([&](int i, Q& lr, V3& lp, V3& lv, V3& la) {
        if (held) {
            const size_t e = (size_t)slot * J + i;
            lr = {rot[e * 4], rot[e * 4 + 1], rot[e * 4 + 2], rot[e * 4 + 3]};
            lp = {pos[e * 3], pos[e * 3 + 1], pos[e * 3 + 2]};
            lv = {vel[e * 3], vel[e * 3 + 1], vel[e * 3 + 2]};
            la = {ang[e * 3], ang[e * 3 + 1], ang[e * 3 + 2]};
        } else {
            lr = {1.f, 0.f, 0.f, 0.f}; lp = {0.f, 0.f, 0.f}; lv = {0.f, 0.f, 0.f}; la = {0.f, 0.f, 0.f};
        }
    }, parents, J, Rr, Rp, Rv, Ra, X + ((size_t)s * T + tid) * J * 15, g, tid);
}

hipError_t live_init() {
    const int lds = (int)(FEAT_MAX_BONES * FC * FT * sizeof(float));
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_live_push<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&mocha_live_push<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

hipError_t launch_live_push(const LiveRing& r, const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, const int32_t* seg,
                            const int* parents, float* X, int32_t* eff, int32_t* valid, int S, int J, hipStream_t s, const int32_t* have,
                            const int* slot_table, int n_slots) {
    if (S <= 0) return hipSuccess;
    if (J > FEAT_MAX_BONES || J < 1 || (slot_table && n_slots < 1)) return hipErrorInvalidValue;
    const size_t lds = (size_t)J * FC * FT * sizeof(float);
    if (slot_table)
        hipLaunchKernelGGL(mocha_live_push<true>, dim3(S), dim3(FT), lds, s, r, Yrot, Ypos, Yvel, Yang, seg, parents, X, eff, valid, J, have, slot_table,
                           n_slots);
    else
        hipLaunchKernelGGL(mocha_live_push<false>, dim3(S), dim3(FT), lds, s, r, Yrot, Ypos, Yvel, Yang, seg, parents, X, eff, valid, J, have, nullptr, 0);
    return hipGetLastError();
}

}  // namespace mocha
