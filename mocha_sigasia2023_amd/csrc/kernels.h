// Internal launcher interface between the host-side context (mocha_api.cpp) and the gfx950
// kernels (*.hip).  Not part of the C ABI (include/mocha_hip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mocha {

// ---------------------------------------------------------------------------------------
// fp32 MFMA GEMM:  C[M,N] = epilogue( Aop[M,K] · W[N,K]^T )
//
// Aop is either the plain row-major matrix A (lda) or an on-the-fly gather of a
// (batch, time, node, channel) activation tensor that realises a temporal convolution with
// reflect padding as a GEMM (net/blocks.py:112-118): for output row (b, t, v) and
// k = tap*Cc + c the operand is
//      ascale * sum_{j<R} src[(b, refl(t*stride + j + tap*tstep - pad, T_full) >> tshift, v), c]
// R = 4, stride = 4 additionally folds AvgPool2d((4,1)) (model.py:47) into the operand;
// tshift = 2 reads a nearest-x4-upsampled tensor (model.py:74) without materialising it; tstep = 4 with stride = 4 walks that tensor's
// SOURCE frames (taps a source frame apart; the reflection at the upsampled ends is then a clamp on source frames: mocha_api.cpp, fold_upsample).
// ---------------------------------------------------------------------------------------
struct GemmParams {
    const float* A = nullptr;     // source activations
    const float* W = nullptr;     // [N][K], k contiguous (nn.Linear / repacked conv layout)
    const float* wsub = nullptr;              // [K] vector subtracted from every W row while it is staged (centred bank)
    const unsigned short* Wsplit = nullptr;   // gemm_x3.hip: the packed three-plane image of W (launch_pack_x3)
    float* C = nullptr;
    const float* bias = nullptr;      // [N] or null
    const float* rowbias = nullptr;   // [rb_mod][N] or null, indexed by (row % rb_mod)
    const float* residual = nullptr;  // [M][ldr] or null, added after the activation
    int M = 0, N = 0, K = 0;
    int lda = 0, ldc = 0, ldr = 0;
    int rb_mod = 1;
    int act = 0;          // 0 none, 1 exact-erf GELU, 2 LeakyReLU(0.2), 3 ReLU
    int a_lrelu = 0;      // LeakyReLU(0.2) applied to the A operand as it is loaded
    int gather = 0;       // 0 plain rows, 1 temporal gather
    int T_out = 1, V = 1, ntaps = 1, pad = 0, stride = 1, R = 1, T_full = 1, tshift = 0, Cc = 0, T_src = 1;
    int tstep = 1;        // distance between taps on the T_full time line
    float ascale = 1.f;
    int ksplit = 1;               // >1: split K over gridDim.z, raw partial sums to C + z*slab_stride
    long long slab_stride = 0;
    // gemm_x3.hip, per context (options "gemm_persistent", "gemm_persistent_max_n"): workgroups of the persistent instance (0 = never; a
    // multiple of 8) and the widest launch, in columns, that takes it
    int persistent = 768, persistent_max_n = 512;
    int tile64_below = 0;         // gemm_x3.hip: mid-size launches with fewer 64 x 128 tiles than this take 64 x 64 tiles (option "gemm_tile64_below")
    // gemm_h2.hip (two fp16 planes, three passes; option "gemm_f16x2"): the packed two-plane image of W and 1 / S_w per row (launch_pack_h2);
    // rows_per_win: consecutive rows of the launch that form one WINDOW (the path's independent unit; >= 64); a_amax: per window a bound on
    // |A| (after a_lrelu), a vector in DEVICE memory - the window's activation scale comes from it; c_amax: null, or the vector where the
    // epilogue leaves, per window, the largest magnitude it stores (atomic max; zeroed by the caller) - a later launch's a_amax
    const unsigned short* Wh2 = nullptr;
    const float* w_inv = nullptr;
    const float* a_amax = nullptr;
    float* c_amax = nullptr;
    int rows_per_win = 0;
    // gemm_x3.hip (one-shot and persistent instances, ksplit = 1): the m-tiles are walked from the last row block to the first - the same
    // tiles, the same code per tile, the n-tiles of an m-tile on the same XCD; nothing but the order in which the rows are touched changes
    int reverse = 0;
};
hipError_t launch_gemm(const GemmParams& p, hipStream_t s);
bool gemm_is_narrow(const GemmParams& p);
bool gemm_is_small(const GemmParams& p);    // true: mid-size launch -> 64 x 64 tiles
bool gemm_is_skinny(const GemmParams& p);
bool gemm_is_skinny16(const GemmParams& p); // true: one or two windows -> mocha_gemm_skinny16 (16x16 tile per workgroup, every load of a wave's K quarter in flight at once)   // true: a handful of windows -> mocha_gemm_skinny (32x32 tile per workgroup, 4-way in-workgroup split-K)
hipError_t gemm_init();           // one-time function attributes (dynamic LDS size)
// fp32 GEMM on the bf16 matrix pipe (gemm_x3.hip): both operands as three bf16 planes, six MFMA passes, fp32-accurate.
// p.Wsplit = the packed image of W made by launch_pack_x3 (gemm_x3_packed_elems(N, K) bf16).
hipError_t gemm_x3_init();
bool gemm_x3_supports(const GemmParams& p);
size_t gemm_x3_packed_elems(int N, int K);
hipError_t launch_pack_x3(const float* W, int N, int K, unsigned short* out, hipStream_t s, const float* wsub = nullptr, int reverse = 0);   // wsub: K values subtracted from every row
hipError_t launch_gemm_x3(const GemmParams& p, hipStream_t s);
// the same engine with the activations resident in registers (gemm_x3r.hip, round 6): K = 256, N a multiple of 128 (>= 256), plain rows, bias / activation epilogue;
// bit-identical to launch_gemm_x3.  grid: workgroups (one per CU; 0 = 256)
hipError_t gemm_x3r_init();
bool gemm_x3r_supports(const GemmParams& p);
hipError_t launch_gemm_x3r(const GemmParams& p, hipStream_t s, int grid = 0);
// fp32 GEMM on the fp16 matrix pipe (gemm_h2.hip): both operands as two fp16 planes with power-of-two scales, three MFMA passes.
hipError_t gemm_h2_init();
bool gemm_h2_supports(const GemmParams& p);
size_t gemm_h2_packed_elems(int N, int K);
hipError_t launch_pack_h2(const float* W, int N, int K, unsigned short* out, float* w_inv /*N*/, hipStream_t s);
hipError_t launch_gemm_h2(const GemmParams& p, hipStream_t s);      // needs p.Wh2, p.w_inv, p.a_amax
hipError_t launch_absmax(const float* x, long long nwin, long long per, float* out /*nwin, zeroed by the caller*/, hipStream_t s, float mul = 1.f, float add = 0.f);   // out[w] = max(out[w], mul * max|window w of x| + add)
hipError_t launch_gather_f32(const float* table, const int32_t* idx, long long rows, float* out, int n, hipStream_t s);    // out[i] = table[clamp(idx[i])]


// ---------------------------------------------------------------------------------------
// Multi-head attention, nq queries x nk keys (<= 192), one workgroup per (window, head)
// (net/transformer.py:65-76; nn.MultiheadAttention in model_CVAE.py):
//   out[b, i, h*DH + d] = softmax_j(q_i·k_j * scale) v_j ;  batch b starts at row b*nq (q, out) / b*nk (k, v)
// What the kernels rely on and no launcher checks (tests/gemm_probe/attention_probe.cpp refuses it before a launch):
//   scale > 0 and finite (the row maximum is taken over the unscaled scores);
//   q, k, v, out (and the kv image) 16-byte aligned, ldq / ldk / ldv / ldo and an explicit hsk / hsv multiples of 4 floats: every operand
//   fetch and every store is 16 bytes at row * ld + 4c floats;
//   heads >= 1, ldq / ldo >= heads * dh, ldk / ldv >= (heads - 1) * hs + dh; a window's rows are all that is read (padded rows are
//   zero-filled or clamped to the window's last row), so the buffers may end with the last window's last row;
//   reverse is honoured only by the full-batch instances of launch_attention_x3 (B * heads > 256) and ignored elsewhere: the same windows
//   in another order, results identical to the bit either way.
// ---------------------------------------------------------------------------------------
struct AttnParams {
    const float* q; const float* k; const float* v; float* out;
    int ldq, ldk, ldv, ldo;       // row strides in floats
    int B, heads, dh, nq, nk;
    float scale;
    int hsk = -1, hsv = -1;       // column offset per head of k / v (default dh; 0 = all heads share the same rows)
    int split_max = 192;          // (window, head) pairs up to which the twelve-wave head-dim-256 variant is launched (0 = never)
    // launch_attention_x3 only (launch_attention refuses it): window b's keys / values are rows [kv_idx[b] * nk, +nk) of k / v (index clamped
    // to [0, kv_rows)) - the decoder reading IN(cha) and cha of the matched bank entries in place (test_fullframework.py:465), no gathered copy
    const int32_t* kv_idx = nullptr; long long kv_rows = 0;
    // launch_attention_x3, full-batch instances only: the windows are walked from the last to the first (GemmParams::reverse)
    int reverse = 0;
};
hipError_t launch_attention(const AttnParams& p, hipStream_t s);
// the same on the bf16 matrix pipe with exact three-plane operands (attention_x3.hip): nq, nk <= 96, dh = 128 / 256
hipError_t launch_attention_x3(const AttnParams& p, hipStream_t s);
hipError_t attention_x3_init();              // one-time function attributes (dynamic LDS of the twelve-wave small-batch variant)
// Cross-attention whose keys and values are the same for every head (the folded decoder: K = IN(cha), V = cha, dh = 256), from the
// pre-split bf16 plane images mocha_instnorm writes (InormExtra::kvimg; layout: attention_kv.hip).  One workgroup per (window, head pair).
static constexpr int ATTN_KV_STAGE_BYTES = 3 * 96 * 64;               // three planes x 96 rows x 32 bf16
static constexpr int ATTN_KV_IMG_BYTES = 16 * ATTN_KV_STAGE_BYTES;    // 8 K stages + 8 V stages per window: 294 912 B
struct AttnKvParams {
    const float* q; float* out; const unsigned short* kv;
    int ldq, ldo;                 // row strides in floats
    int B, heads, dh, nq, nk;
    float scale;
    int pairs = 0;                // 1: a six-wave workgroup per head pair even when the heads come in fours (diagnostic)
};
hipError_t launch_attention_x3_kv(const AttnKvParams& p, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Small bandwidth-bound kernels
// ---------------------------------------------------------------------------------------
// X (B,T,V,Cin) -> 1x1 conv Cin->64 + bias -> LeakyReLU -> hop-partitioned adjacency -> joint->part pool,
// written as rows (b,t,p) x (k*64+c)   [model.py:44-46 front half, net/blocks.py:57-66,131]
// raw_root = 1: X frames are (V+1, Cin) with the root bone first and are z-scored with xmean/xstd ((V+1)*Cin) on load
hipError_t launch_embed_front(const float* X, const float* W1, const float* b1, const float* AP /*3*V*6*/,
                              float* out, int nframes, int V, int Cin, const float* xmean, const float* xstd, int raw_root,
                              hipStream_t s, bool planes = false, int max_wgs = 512);
hipError_t launch_embed_sums(const float* X, const float* W1, const float* b1, const float* AP, float* u, int nwin, int V, int Cin,
                             const float* xmean, const float* xstd, int raw_root, hipStream_t s, int max_wgs = 512, int reverse = 0);      // reverse: row blocks from the last to the first (GemmParams::reverse), here and below; max_wgs: option "embed_front_max_wgs" (per context)
// rows (b,t,p) x 256 -> LeakyReLU -> body-part adjacency (2 hops) -> rows (b,t,w) x (k*256+c)
hipError_t launch_body_front(const float* x, const float* A_b /*2*6*6*/, float* out, int rows6 /*B*15*/, hipStream_t s, int reverse = 0);
// g rows (b,t',p) x (k*64+c) -> y2c rows (b,t',w) x 64 : sum_k sum_p AU[k][p][w] g[...]
hipError_t launch_joint_expand(const float* g, const float* AU /*3*6*V*/, float* out, int nframes15, int V, hipStream_t s, int reverse = 0);
// z rows x 64 -> LeakyReLU -> 1x1 conv 64->Cout + bias -> Y rows x Cout   [model.py:77-79]
// ymean/ystd ((V+1)*Cout, root row first) non-null: Y is de-normalised in the epilogue
hipError_t launch_final_proj(const float* z, const float* W6, const float* b6, float* Y, int rows, int Cout, int V,
                             const float* ymean, const float* ystd, hipStream_t s, int phased = 0, int reverse = 0);
// per (b, channel) instance norm over n tokens (net/transformer.py:13-20).
//   out = (x-mean)/(std+eps); mean_out (B,256) optional; zn = (out - gm)/gs optional
// optional extras of the instance norm: zc = zn - centre (the matcher's centred queries, bit-identical to mocha_sub_rows on zn);
// rows gathered from a table (x row of window b = table[clamp(row_idx[b])], the decoder's cha_encoded[frame_index]) and copied out
static constexpr int QSTAT_PARTS = 4;      // row statistics come in parts (one per workgroup of a window's channel quarter), added in order by mocha_match_select2
struct InormExtra {
    const float* centre = nullptr; float* zc = nullptr;      // zc: (z-score - centre), fp32
    unsigned short* zc16 = nullptr;                          // the same as bf16 (round to nearest even): the many-query bf16 pass's query plane
    // zc16 with plane_stride > 0: a SECOND plane bf16(zc - plane 0) at zc16 + plane_stride (elements) - the coarse pass then carries 16
    // significant bits of every query value; qstat (2 x QSTAT_PARTS floats per window, summed by the consumer in part order): ||zc||^2 and the squared norm of what the planes (zc16) leave out
    // - or, with zc alone, {||zc||^2, 0} - the selection's error bound (match_select2.hip) without a pass over the row
    long long plane_stride = 0; float* qstat = nullptr;
    const float* table = nullptr; const int32_t* row_idx = nullptr; long long table_rows = 0; float* copy_out = nullptr;
    // kvimg: per window the pre-split key / value images of launch_attention_x3_kv (ATTN_KV_IMG_BYTES each): K = the normalised rows,
    // V = the input rows, three bf16 planes each, rows n .. 95 zero
    unsigned short* kvimg = nullptr;
    int split_max = 1 << 30;             // windows up to which a window's channels go over four workgroups (per context: option "inorm_split_max")
    double* mean64 = nullptr;            // (B, 256) token mean summed in float64: the input of the float64 style MLP (launch_linear_f64)
    int reverse = 0;                     // windows from the last to the first (GemmParams::reverse)
};
hipError_t launch_instnorm(const float* x, float* out, float* mean_out, const float* gm, const float* gs, float* zn,
                           int B, int n, hipStream_t s, const InormExtra* ex = nullptr);
// AdaIN + the attention's mapping norm (net/transformer.py:108-113, 49-56):
//   xad = (1+gamma)*IN(x)+beta ; qin = IN(xad) ; gb (B,512) = [gamma | beta]
// closed != 0: qin from the first statistics in closed form (no cancellation against beta; pointwise.hip)
// gb_idx non-null: window b reads its gamma / beta at gb + clamp(gb_idx[b], gb_rows) * gb_stride (the bank's cached style constants)
hipError_t launch_adain(const float* x, const float* gb, int gb_stride /*floats between windows*/, float* xad, float* qin, int B, int n, hipStream_t s,
                        int closed = 1, const int32_t* gb_idx = nullptr, long long gb_rows = 0, int split_max = 1 << 30, int reverse = 0);
// Y = act(X W^T + bias) in float64, L independent column blocks (pointwise.hip: the decoder's style MLP)
// tiled != 0: the tiled kernel also for M <= 16 rows, which by default take a wave-reduction kernel whose summation order is another one
// (both tile sizes sum one fma chain over ascending k): a row's result then does not depend on how many rows the launch has
hipError_t launch_linear_f64(const double* X, int ldx, int xcol, const double* W, const double* bias, double* y64, float* y32, int ldy,
                             int M, int N, int K, int L, int act, hipStream_t s, int tiled = 0);
// u rows (b,t',p) x (dt*256+c) = 1/4 sum of the 4 reflect-indexed frames of tap dt (conv k=5 fused with AvgPool(4))
hipError_t launch_window_sums(const float* y, float* u, int rows, int channels /*256 or 192*/, hipStream_t s);
// ---- CVAE sampler pieces (cvae.hip; model_CVAE.py)
// y = LayerNorm(x) over 256 channels per row (eps 1e-5, biased variance), affine
hipError_t launch_layernorm256(const float* x, const float* w, const float* b, float* y, int rows, hipStream_t s);
// tokens (B,182,256) = [mu_token, logvar_token, c (B,180,256)] + pe[:182]          (model_CVAE.py:69-76)
hipError_t launch_cvae_prior_tokens(const float* c, const float* mu_tok, const float* lv_tok, const float* pe, float* out, int B, int nc, hipStream_t s);
// z = x[:,0] (+ eps * exp(0.5 x[:,1]));  mem (B,1+nc,256) = [z, c];  q (B,nq,256) = pe[:nq]   (model_CVAE.py:81-87,158-163)
hipError_t launch_cvae_latent(const float* x /*B,ntok,256*/, int ntok, const float* eps, const float* c, int nc, const float* pe, int nq,
                              float* mem, float* q, float* mu_out, float* logvar_out, int B, hipStream_t s);
// cond (B,2n,256) = cat[(src_cnt - sm)/ss, (prev - cm)/cs] over tokens; out = x*sd + mean   (test_fullframework.py:446-449)
hipError_t launch_cvae_condition(const float* src_cnt, const float* sm, const float* ss, const float* prev, const float* cm,
                                 const float* cs, float* cond, int B, int n, hipStream_t s);
hipError_t launch_scale_shift(const float* x, const float* mean, const float* sd, float* out, int B, int n, hipStream_t s);
// ---- the sampler with one weight set per group of rows (cvae_grouped.hip): G groups of m consecutive rows, group g on slot which[g] of a
// bank of Cw slots; stored[slot] != 0 says the slot holds weights.  which (G) and stored (Cw) are DEVICE int32 arrays read by every launch.
// A group whose slot is outside [0, Cw) or not stored reads no weight, bias or residual and its output rows are zeros.
// C[g] = act(A[g] W[slot]^T + bias[slot]) (+ R[g]), exact fp32 (v_mfma_f32_16x16x4_f32); W / bias of slot i start w_stride / b_stride
// floats after those of slot i - 1.  Any m >= 1, N % 16 == 0, K % 16 == 0; act 0 or 3 (ReLU); lda / ldc / ldr / the strides multiples of 4
// floats and every pointer 16-byte aligned (checked but for the alignment of the pointers).  The order of an output element's sum depends
// on K alone: a group's rows are the same bits at any position of any batch.
struct GroupedGemmParams {
    const float* A = nullptr;         // (G * m, lda)
    const float* W = nullptr;         // slot 0's [N][K], k contiguous
    const float* bias = nullptr;      // slot 0's [N], or null
    const int32_t* which = nullptr;   // device (G)
    const int32_t* stored = nullptr;  // device (Cw)
    float* C = nullptr;               // (G * m, ldc)
    const float* residual = nullptr;  // (G * m, ldr) or null, added after the activation
    int G = 0, m = 0, N = 0, K = 0, Cw = 0;
    int lda = 0, ldc = 0, ldr = 0;
    long long w_stride = 0, b_stride = 0;
    int act = 0;
};
hipError_t launch_gemm_grouped(const GroupedGemmParams& p, hipStream_t s);
// launch_layernorm256 / launch_cvae_prior_tokens with the affine pair / the two learned tokens of the group's slot (`stride` floats between slots)
hipError_t launch_layernorm256_grouped(const float* x, const float* w, const float* b, long long stride, const int32_t* which,
                                       const int32_t* stored, int Cw, float* y, int G, int m, hipStream_t s);
hipError_t launch_cvae_prior_tokens_grouped(const float* c, const float* mu_tok, const float* lv_tok, long long stride, const int32_t* which,
                                            const int32_t* stored, int Cw, const float* pe, float* out, int B, int nc, hipStream_t s);
// stored[slot] = value by one lane with an ordinary store (mocha_cvae_bank_store's last launch, mocha_cvae_bank_clear)
hipError_t launch_cvae_bank_publish(int32_t* stored, int slot, int Cw, int value, hipStream_t s);
// demo featurisation (featurize.hip): local bone features of B windows -> X (B,T,J,15) un-normalised, root bone included
hipError_t featurize_init();
hipError_t launch_featurize(const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, const int* parents /*J, device*/,
                            float* X, int B, int T, int J, hipStream_t s);
// live sessions (live.hip): per stream a ring of the last LIVE_WINDOW frames of local bone data (rot (S,60,J,4), pos / vel / ang (S,60,J,3))
// and counters (S,2) = {head, fill}, all device memory.  One call pushes the new frame (Yrot (S,J,4), Ypos / Yvel / Yang (S,J,3)) of
// every stream, writes X (S,60,J,15) bit-identical to launch_featurize on the materialised windows (frames a filling ring does not hold
// yet: identity / zeros), eff[s] = seg[s] once stream s holds 60 frames, else -1, and valid[s] = 1 / 0.
static constexpr int LIVE_WINDOW = 60;
struct LiveRing { int32_t* counters; float *rot, *pos, *vel, *ang; };
hipError_t live_init();
// have (S) or null: a stream with have[s] == 0 brought no frame - nothing is pushed, its counters stay, eff[s] = -1, valid[s] = 0 and its
// window is featurised as an empty ring's
// slot_table (n_slots pairs) or null: a resident bank's slot table (below); a stream that names an EMPTY slot pushes its frame as usual but
// gets eff[s] = -1, valid[s] = 0 - the step treats it as warming until the slot holds a character again
hipError_t launch_live_push(const LiveRing& r, const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, const int32_t* seg,
                            const int* parents /*J, device*/, float* X, int32_t* eff, int32_t* valid, int S, int J, hipStream_t s,
                            const int32_t* have = nullptr, const int* slot_table = nullptr, int n_slots = 0);
// the CVAE branch of a live step (live_ours.hip).  counters (S,3) = {chain: steps since the stream's seed frame, last: the character id of
// its last step, mode}; cnt / prev / vae (S,90,256), cond (S,180,256), eps (S,256); sm / ss / cm / cs (90,256) the CVAE's statistics.
// condition: mode[s] = 0 (eff[s] outside 0..nseg-1: warming) / 1 (chain == 0 or eff[s] != last: seed) / 2 (chain) into the counters;
//   cond[s] = 0 (mode 0), [(cnt - sm)/ss, 0] (mode 1), [(cnt - sm)/ss, (prev - cm)/cs] (mode 2); eps_out[s] = eps_in[s] (noise 1) or
//   Philox4x32-10 (key = the seed's low / high word, counter (block 0..63, chain, s, 0)) + Box-Muller (noise 2); noise 0: not written.
// update: mode 2: prev[s] = vae[s] * cs + cm; mode 1: prev[s] = bank_enc[gidx[s]]; modes 1, 2: chain + 1, last = eff[s]; seeded[s] = mode == 1.
// grp non-null: the GROUPED instances - one CVAE per character from a weight bank of Cw slots.  Stream s takes slot cvae_of[eff[s]]
// (cvae_of: one device int32 per segment / slot of the character bank) and that slot's statistics, stats (Cw, 4, 90, 256) = sm | ss | cm | cs;
// sm / ss / cm / cs are then ignored.  No CVAE (cvae_of negative or >= Cw, or stored[slot] == 0): mode 1 on every valid frame, cond[s] = 0.
// condition writes slot[s] (S) = the stream's slot, -1 for a warming stream or one without a CVAE; update reads it.
struct OursGroup {
    const int32_t* cvae_of = nullptr;
    const int32_t* stored = nullptr;
    const float* stats = nullptr;
    int Cw = 0;
    int32_t* slot = nullptr;
};
hipError_t launch_live_ours_condition(int32_t* counters, const int32_t* eff, int nseg, const float* cnt, const float* prev, const float* sm,
                                      const float* ss, const float* cm, const float* cs, float* cond, int noise, const float* eps_in,
                                      unsigned long long seed, float* eps_out, int S, hipStream_t s, const OursGroup* grp = nullptr);
hipError_t launch_live_ours_update(int32_t* counters, const int32_t* eff, const float* vae, const float* cm, const float* cs,
                                   const float* bank_enc, const int32_t* gidx, long long bank_rows, float* prev, int32_t* seeded, int S,
                                   hipStream_t s, const OursGroup* grp = nullptr);
// post-processing of decoded windows (postprocess.hip)
#define MOCHA_MAX_CONTACT 4
#define MOCHA_MAX_CHAIN 8
#define MOCHA_MAX_BONES 32
// The mocap front end of a live session (ingest.hip): ONE raw frame of S independent streams in - local rotations (V,4) wxyz or (V,3)
// Euler degrees, local positions (V,3), joint 0 the hips - and, once a stream has seen INGEST_FIRST frames, frame n-1-lookahead of the
// reference's process_data on the stream's prefix out: Yrot (S,V+1,4), Ypos / Yvel / Yang (S,V+1,3) root bone first, src_rvel / src_rang
// (S,3), src_speed (S), contact (S,n_contact), have (S) = 1 / 0.  state: (S, INGEST_STATE_DOUBLES) float64 words, all-zero = no frame seen.
// rows15 / rows31: the (15,15) and (31,31) cubic fit rows on the device.  One launch, no allocation, no synchronisation.
static constexpr int INGEST_FIRST = 31, INGEST_RING = 40, INGEST_MAX_LOOKAHEAD = 18;
static constexpr int INGEST_FRAME_DOUBLES = MOCHA_MAX_BONES * 7 + 4;      // quaternions | positions | spine xz | direction xz
static constexpr int INGEST_STATE_DOUBLES = 2 + MOCHA_MAX_BONES * 4 + INGEST_RING * INGEST_FRAME_DOUBLES + 60 * 3;
struct IngestParams {
    double* state;
    const double *rows15, *rows31;
    const float *rot, *pos;         // the raw frame: (S,V,4|3), (S,V,3)
    float *Yrot, *Ypos, *Yvel, *Yang, *src_rvel, *src_rang, *src_speed;
    unsigned char* contact;
    int32_t* have;
    int V, lookahead, euler, order[3], roles[5], n_contact;
    int parents[MOCHA_MAX_BONES];   // of the V raw joints
    int contact_bones[MOCHA_MAX_CONTACT];
    double scale, fps, threshold;
};
hipError_t launch_live_ingest(const IngestParams& p, int S, hipStream_t s);
// The same preparation for WHOLE clips (ingest_clip.hip): C clips concatenated along the frame axis, clip c = frames offsets[c] ..
// offsets[c+1]-1, every clip at least INGEST_FIRST frames; nothing crosses a clip boundary.  Parallel over frames; float64 on the fp32
// inputs, rounded to fp32 once at the output.  flags[c] != 0: the clip is mirrored (animation_mirror, generate_database.py:40-55) with the
// joint exchange `map` before the root bone is extracted.  The float64 workspace, per frame: raw quaternions | unrolled quaternions (V,4
// each) | positions (V,3) | spine xz, direction xz | root position xz, root rotation, root-local hips position and rotation
// (CLIP_ROOT_DOUBLES); `below`: the per-frame toe speed flags the vote reads.
static constexpr int CLIP_ROOT_DOUBLES = 13;
static constexpr int CLIP_SCAN_CHUNK = 32, CLIP_SCAN_THREADS = 128;       // unroll scan: frames per lane, lanes per workgroup
struct ClipParams {
    const float *rot, *pos;         // (F,V,4|3), (F,V,3)
    const int *offsets, *flags;     // device: (C+1), (C) or NULL
    const double *rows15, *rows31;
    double *qraw, *q, *p, *series, *root;
    unsigned char* below;           // (F, MOCHA_MAX_CONTACT)
    float *out_pos, *out_vel, *out_rot, *out_ang;
    unsigned char* out_contact;     // (F, n_contact)
    int F, C, V, euler, order[3], roles[5], n_contact, max_depth;
    int parents[MOCHA_MAX_BONES];   // of the V raw joints
    int depth[MOCHA_MAX_BONES];     // ancestors of a raw joint
    int map[MOCHA_MAX_BONES];       // the mirror exchange
    int contact_bones[MOCHA_MAX_CONTACT];
    double scale, fps, threshold;
};
// launch = 0 quaternions, 1 unroll (all clips), 2 mirror, 3 unroll (mirrored clips), 4 series, 5 root, 6 velocities + toe speed flags,
// 7 contact vote: one kernel each, so that the host layer can time every launch
hipError_t launch_clip_ingest(const ClipParams& p, int launch, hipStream_t s);
// divide_clip(divide=True) (generate_database.py:57-84) as one gather: window b of clip c (wcum[c] <= b < wcum[c+1]) starts at frame
// (b - wcum[c]) * step of the clip; a short slice is padded by its first / last frame, vel and ang padding zero
struct ClipWindowParams {
    const float *pos, *vel, *rot, *ang;   // (F,J,3|3|4|3)
    const unsigned char* contact;          // (F,nc)
    const int *offsets, *wcum;             // device: (C+1) each
    float *Yrot, *Ypos, *Yvel, *Yang;      // (B,window,J,.)
    unsigned char* Ycontact;               // (B,window,nc)
    int C, J, nc, window, step;
    long long B;
};
hipError_t launch_clip_windows(const ClipWindowParams& p, hipStream_t s);
// The resampler in front of the ingester (resample.hip): (rotations, positions) at a source rate -> (unit quaternions, positions) at the
// target rate.  The step between outputs is num / den source frames (1..RESAMPLE_MAX_TERM each); output k of a clip sits at t = k num:
// source frame i = t div den, a = (t mod den) / den; a == 0 gives frame i itself and frame i+1 is not read, else the frame between i and
// i+1 (resample_body.h).  Whole clips: q / p are the unrolled float64 quaternions and positions mocha_clip_quat (scale 1) and
// mocha_clip_unroll left in the workspace; clip c = source frames in_off[c] .. in_off[c+1]-1 -> outputs out_off[c] .. out_off[c+1]-1.
static constexpr int RESAMPLE_MAX_TERM = 4096, RESAMPLE_MAX_OUT = 4;
struct ClipResampleParams {
    const double *q, *p;                        // (F,V,4), (F,V,3)
    const int *in_off, *out_off, *num, *den;    // device: (C+1), (C+1), (C), (C)
    float *rot_out, *pos_out;                   // (F',V,4), (F',V,3)
    int C, V;
    long long F_out;
};
hipError_t launch_clip_resample(const ClipResampleParams& p, hipStream_t s);
// One source frame of S streams in lockstep: outputs k_first .. k_first+count-1 (the host's schedule for this push) of every stream into rot_out
// (S,RESAMPLE_MAX_OUT,V,4) / pos_out (S,RESAMPLE_MAX_OUT,V,3).  state: (S, RESAMPLE_STATE_DOUBLES) float64 words per stream = fresh | have
// | per joint: the previous unrolled quaternion, position and unroll sign; fresh != 0 or have == 0 (all-zero state): no predecessor,
// every output of the push is the new frame.
static constexpr int RESAMPLE_JOINT_DOUBLES = 8, RESAMPLE_STATE_DOUBLES = 2 + MOCHA_MAX_BONES * RESAMPLE_JOINT_DOUBLES;
struct ResampleStepParams {
    double* state;
    const float *rot, *pos;                     // (S,V,4|3), (S,V,3)
    float *rot_out, *pos_out;
    int V, euler, order[3], num, den, count;
    long long k_first;
};
hipError_t launch_resample_step(const ResampleStepParams& p, int S, hipStream_t s);
// World-space poses and skinning palettes (world_pose.hip): quat.fk over n frames of (V+1)-bone locals, float64 or fp32 in; gpos (n,V+1,3),
// grot (n,V+1,4) float64 and palette (n,V,12) fp32 = pre o [to_xform(grot) | gpos] o inverse bind, each may be null.  rot, grot and palette
// are 16-byte aligned.  bind: WORLD_BIND_DOUBLES(V) float64 words = pre (3x4 row-major) | the inverse bind of bones 0..V (3x4 each), written
// by launch_world_bind from a rest pose.  anc[b]: bit a set for b and every ancestor a of b.  Frames whose valid entry is 0 are not written.
static constexpr int WORLD_FPB = 8;                              // frames per workgroup, 32 lanes each
static constexpr int WORLD_BIND_DOUBLES(int V) { return (V + 2) * 12; }
struct WorldPoseParams {
    const void *rot, *pos;          // (n,V+1,4), (n,V+1,3): float64, or fp32 when in_f32
    const int32_t* valid;           // (n) or null
    const double* bind;
    double *gpos, *grot;
    float* palette;
    long long n;
    int V, in_f32;
    unsigned anc[MOCHA_MAX_BONES];
};
hipError_t launch_world_pose(const WorldPoseParams& p, hipStream_t s);
struct WorldBindParams {
    const double *rest_rot, *rest_pos;      // (V+1,4) or null = identity, (V+1,3)
    double* bind;
    int V;
    unsigned anc[MOCHA_MAX_BONES];
    double pre[12];
};
hipError_t launch_world_bind(const WorldBindParams& p, hipStream_t s);
// The MOTION blocks of BVH files as text -> rot / pos (F,v_out,3) fp32 (mocha_bvh_motion, bvh_parse.hip).  The text is walked in blocks
// of BVH_BLOCK bytes; clips start on block boundaries, so a clip's first token ordinal is the token prefix at its first block.
static constexpr int BVH_BLOCK = 4096, BVH_MAX_TOKEN = 64, BVH_MAX_SLOW = 4096;
struct BvhSlow { unsigned long long dest, at; };      // dest: element index, bit 63 set for rot; at: byte offset (the fp32 bits once patched)
struct BvhReport { unsigned long long first_bad; unsigned slow, tokens; };      // first_bad: ~0 = none
struct BvhParams {
    const unsigned char* text;          // nbytes = nblocks * BVH_BLOCK, 16-byte aligned
    long long nbytes;
    unsigned nblocks;
    const long long *begin, *end;       // device: (C) byte ranges of the clips
    const int *offsets, *map;           // device: (C+1) frame offsets, (n_joints) output joint or -1
    const float* off_out;               // device: (v_out,3) or NULL
    unsigned *counts, *prefix;          // device: (nblocks) token starts per block, (nblocks+1) their exclusive scan
    BvhReport* report;
    BvhSlow* slow;                      // device: BVH_MAX_SLOW entries
    float *rot, *pos;
    int C, n_joints, channels, v_out, per_frame, root_out, n_patch;
    long long F;
};
// launch = 0 count, 1 scan, 2 parse, 3 finish + fill, 4 patch (n_patch slow tokens converted on the host): one kernel each
hipError_t launch_bvh_parse(const BvhParams& p, int launch, hipStream_t s);
// The way back (mocha_bvh_format, bvh_format.hip): bvh_pos / bvh_euler (F,V,3) float64 -> the MOTION text of the reference's writer.
// Token t = frame * C + column of a virtual (F, C) matrix; the text is produced in blocks of BVHW_BLOCK tokens, one per lane.
static constexpr int BVHW_BLOCK = 256, BVHW_MAX_TOKEN = 21;
struct BvhwReport { unsigned long long first_bad, bytes; };      // first_bad: the smallest refused token ordinal, ~0 = none
struct BvhwParams {
    const double *pos, *euler;          // (F,V,3)
    const int *visit, *offsets;         // device: (V) joint of column group i, (n_clips+1) frame offsets
    unsigned *counts, *prefix;          // device: (nblocks) bytes per block, (nblocks+1) their exclusive scan
    long long* clip_begin;              // device: (n_clips+1) first byte of every clip's text, then the total
    BvhwReport* report;
    unsigned char* text;
    int ax[3];
    int V, C, save_positions, n_clips;
    unsigned T, nblocks;                // tokens = F * C, blocks of BVHW_BLOCK tokens
};
// launch = 0 count, 1 scan, 2 write: one kernel each
hipError_t launch_bvh_format(const BvhwParams& p, int launch, hipStream_t s);
static constexpr int POST_STATE_DOUBLES = 8 + MOCHA_MAX_BONES * 3 + MOCHA_MAX_CONTACT * 19;
struct PostParams {
    const float* heads;             // (clips, frames, V, 13)
    const float* speed;             // (clips, frames)
    const float* src_rvel;          // (clips, frames, 3)
    const float* src_rang;          // (clips, frames, 3)
    const float* src_speed;         // (clips, frames)
    const unsigned char* contact;   // (clips, frames, n_contact)
    double *pos, *rot, *ik_rot;     // (clips, frames, V+1, 3|4|4)
    double *bvh_pos, *bvh_euler;    // (clips, frames, V, 3) or null
    int n_clips, n_frames, V, n_contact, ik_enabled, blend_enabled;
    int parents[MOCHA_MAX_BONES];
    int contact_bones[MOCHA_MAX_CONTACT];
    double dt, max_length_buffer, foot_height, unlock_radius, halflife;
    double* state;                  // resumable form only: (clips, POST_STATE_DOUBLES), else null
    const int32_t* valid;           // resumable form only: (clips) or null; clips whose entry is 0 are skipped whole
};
hipError_t launch_pose_heads(const float* Y, float* heads, float* speed, int B, int T, int V, hipStream_t s);
hipError_t launch_post_clip(const PostParams& p, hipStream_t s);
// one frame per clip with the clip's state (p.state: POST_STATE_DOUBLES float64 words per clip, all-zero = no frame seen yet) in device
// memory: p as for launch_post_clip with n_frames = 1, the same kernels
hipError_t launch_post_step(const PostParams& p, hipStream_t s);
// Inertialization of the pose heads across a character switch (motion/Inertialization.py:71-91 per non-root bone), ONE frame of n
// independent streams: heads_in / heads_out (n, V, 13) fp32 (they may alias), state (n, INERT_STATE_DOUBLES) float64 words, all-zero =
// a reset stream; ids / trigger / valid (n) or null.  One launch, no allocation, no synchronisation.
static constexpr int INERT_BONE_DOUBLES = 13 + 3 + 3 + 3 + 4;      // prev_in | off_pos | off_vel | off_ang | off_rot
static constexpr int INERT_STATE_DOUBLES = 2 + MOCHA_MAX_BONES * INERT_BONE_DOUBLES;
hipError_t launch_inertialize(double* state, const float* heads_in, float* heads_out, const int32_t* ids, const int32_t* trigger,
                              const int32_t* valid, int n, int V, double halflife, double dt, hipStream_t s);
// per-column mean and population std over N rows (bank build: cnt_norm)
size_t column_mean_scratch_doubles(int cols);
hipError_t launch_column_mean(const float* x, int64_t N, int cols, float* mean, double* scratch, hipStream_t s);
hipError_t launch_column_stats(const float* x, int64_t N, int cols, float* mean, float* sd, hipStream_t s);
// bank row squared norms
hipError_t launch_rownorm2(const float* x, const float* sub /*or null*/, float* out, int64_t rows, int cols, hipStream_t s, int reverse = 0);
hipError_t launch_sub_rows(const float* x, const float* sub, float* out, int64_t rows, int cols, hipStream_t s);
// ---------------------------------------------------------------------------------------
// Context matching.  Every path is a cheap coarse stage, a pruning rule and an exact re-rank; the result is exact as long as the coarse
// stage's error stays inside the bound the rule assumes (stated with each kernel; held stage by stage by tests/test_match_kernels.py).
// What the kernels rely on and no launcher checks (tests/gemm_probe/match_probe.cpp refuses it before a launch):
//   pointers: every operand non-null and sized as stated; launch_to_bf16: x, sub 16-byte and y 8-byte aligned; launch_center_bf16: x,
//   centre, out 16-byte aligned; inputs finite (the bf16 conversions do not look for NaN);
//   coarse passes (launch_match_gemm_bf16, launch_match_pass256): qc16, bank16 and an image 16-byte aligned; S 16-byte aligned when
//   N % 4 == 0 (its stores are then 16 bytes); with planes = 2 the second plane EXACTLY Q * D elements after the first; the image of the full
//   match_tiled_elems / match_tile32_elems size (rows past N are part of it); tickets all zero at first use (they are left at zero);
//   K slice z covers the 64-k steps [z * per, (z + 1) * per) cut at D / 64, per = ceil(D / 64 / ksplit): a slice past the end is empty and its slab
//   is written as zeros; S is ksplit slabs of Q * N floats, every element of every slab written, nothing else;
//   selections (launch_match_select, launch_match_select2): exactly one of bank / bank16; query, centre and the bank 16-byte aligned (centre
//   is read in both bank modes by launch_match_select); lds >= N and slab_stride >= (Q - 1) * lds + N (ksplit > 1); S and bnorm 16-byte aligned
//   where lds, N and slab_stride are all multiples of 4 (the 16-byte score path; otherwise scalar loads); D >= 256 (D = 0 passes D % 256
//   and would read in front of the centre); NaN scores never qualify; a query without any finite score gets row 0, dist NaN from
//   launch_match_select2 and row 0's direct-form distance from launch_match_select;
//   few-query scans: rho / rho8 must be UPPER bounds of the copies' residual norms (an underestimate silently drops true winners); the
//   first match_scan16_scratch_head_words() words of the scratch zero at first use.
// ---------------------------------------------------------------------------------------
// many-query matcher (match_mfma.hip): centred bf16 queries, one-plane bf16 coarse scores S[z][q][n] (K split z), and the
// select kernel: per query, EVERY row whose coarse score ||b-c||^2 - 2 S lies within margin_rel * (2||q-c||^2 + ||b-c||^2 +
// ||b0-c||^2) of the best one (margin_rel >= 0 bounds the coarse pass's error; a negative value is rejected) is re-evaluated
// exactly in the direct form; the smallest exact distance wins, ties to the lowest row.
// bank = raw fp32 rows (exact distance sum (q - b)^2) or bank16 = centred bf16 rows (sum ((q - c) - b16)^2).
hipError_t match_mfma_init();
int match_bf16_ksplit(int Q, int64_t N);
hipError_t launch_center_bf16(const float* x, const float* centre, void* out, int64_t rows, int cols, hipStream_t s);
// row by row: planes[0] = bf16(x - centre) and, with nplanes = 2, planes[1] = bf16(x - centre - planes[0]) (stacked: plane 1 starts rows * cols
// elements after plane 0), or out32 = x - centre in fp32; qstat[row] = QSTAT_PARTS pairs whose sums are {||x - centre||^2, ||x - centre - planes||^2 (0 for fp32)} (all of it in part 0).  One
// workgroup per row, fixed summation order.  Exactly one of planes / out32 is non-null.
hipError_t launch_center_rows(const float* x, const float* centre, void* planes, int nplanes, float* out32, float* qstat, int64_t rows, int cols, hipStream_t s, int reverse = 0);
// planes = 2: qc16 holds two stacked bf16 planes of the queries (plane 1 starts Q * D elements after plane 0), S = (a0 + a1) b^T
// tiled: the bank as launch_tile_bf16 wrote it (match_tiled_elems(N, D) bf16), or null to read the row-major bank16
// nt_bank != 0: the bank's LDS-DMA loads carry the non-temporal hint
hipError_t launch_match_gemm_bf16(const void* qc16, const void* bank16, float* S, int Q, int64_t N, int D, int ksplit, hipStream_t s, int planes = 1,
                                  const void* tiled = nullptr, int nt_bank = 0, unsigned* tickets = nullptr);
// tickets (option "match_fold", round 6): ceil(Q / 128) * ceil(N / 128) zeroed words; the last-arriving K-slab workgroup of a tile leaves the slabs' sum in slab 0
// round 5 (match_pass.hip): 128 queries x 256 rows per workgroup, the bank straight into registers, only the queries through LDS;
// variant: bits 0-3 register prefetch depth in 64-k stages (0 = default), bit 4 non-temporal bank loads, bit 8 fill only (measurement)
int match_pass256_ksplit(int Q, int64_t N);
hipError_t launch_match_pass256(const void* qc16, const void* bank16, float* S, int Q, int64_t N, int D, int ksplit, hipStream_t s, int variant = 0,
                                int planes = 1, const void* tiled32 = nullptr);
// the bank in the pass's operand order (every wave-level load 1 KB contiguous): match_tile32_elems(N, D) bf16
size_t match_tile32_elems(int64_t N, int D);
hipError_t launch_tile32_bf16(const void* bank16, void* out, int64_t N, int D, hipStream_t s);
size_t match_tiled_elems(int64_t N, int D);
hipError_t launch_tile_bf16(const void* bank16, void* out, int64_t N, int D, hipStream_t s);
hipError_t launch_match_select(const float* S, int ksplit, long long slab_stride, int lds, const float* bnorm, const float* query,
                               const float* centre, const float* bank, const void* bank16, float margin_rel, int Q, int64_t N, int D,
                               int32_t* idx, float* dist, hipStream_t s);
// the same selection without the usually unnecessary work (match_select2.hip): the row statistics of the error bound come from the
// producer of the centred queries (qstat: 2 x QSTAT_PARTS floats per query - launch_center_rows, InormExtra::qstat), nothing is staged in LDS, and a
// query whose coarse minimum stands alone is answered without touching a bank row when dist == nullptr.  Otherwise the same arguments,
// bounds and result semantics as launch_match_select, but for a query without any finite score: row 0 from both, dist NaN here, row 0's
// direct-form distance there.
hipError_t launch_match_select2(const float* S, int ksplit, long long slab_stride, int lds, const float* bnorm, const float* query,
                                const float* centre, const float* bank, const void* bank16, const float* qstat, float margin_rel, int Q,
                                int64_t N, int D, int32_t* idx, float* dist, hipStream_t s);
// ---------------------------------------------------------------------------------------
// Few-query scans and segmented matchers (match_stream.hip, match_scan8.hip, match_segmented.hip, match_seg_topk.hip, the two gathers of
// pointwise.hip; held at the kernel boundary by tests/test_scan_kernels.py).  What the kernels rely on and no launcher checks
// (tests/gemm_probe/scan_probe.cpp refuses it before a launch):
//   pointers: every operand non-null unless stated optional, sized as stated; the bank (fp32, bf16 or byte rows), the queries (qc and
//   query), enc, src and the gathers' out 16-byte aligned (16-byte loads and stores, the refine's LDS-DMA of the query row); scratch,
//   partial and keys 8-byte aligned;
//   1 <= N <= 0x7ffffff0 (the row is the low word of a key; row N - 1 stands in for the rows past the end of the last workgroup) and
//   D > 0: D = 0 passes every D % chunk test.  D a multiple of the chunk - 1280 fp32, 1536 bf16, 2560 AND 1536 for the byte stage (so
//   7680 | D there) - is checked by the launchers; launch_match_scan16 / _scan8 also check D % 256 == 0 and D <= 23040 (the refine holds a
//   query row in LDS, match_refine_init), launch_match_refine checks NOTHING: 256 <= D <= 23040, D % 256 == 0, 1 <= nq <= 8, nwg >= 1 are
//   its caller's, and wgmin[q] must hold, per query, keys of that query whose minimum is the minimum of keys[q] (the scan's per-16-row minima);
//   scratch sizes: partial >= match_stream_scratch(Q, N) (whole groups of 8 queries), keys >= 8 * N for launch_match_topk, scratch >=
//   match_scan16_scratch_words(N) (the refine alone: the head), partial >= match_seg_scratch_words(Q, max_rows), plan >= seg_plan_ints(Q, S)
//   (the soft matcher: of SEG_TOPK_Q), keys >= match_seg_keys_words(max_rows); the scratch HEAD - match_scan16_scratch_head_words() words -
//   zero at first use: the arrival tickets must be zero when a launch starts (every completed launch leaves them so) and the byte stage's
//   two mode words start at {0, 0};
//   rho / rho8 UPPER bounds of the copies' residual norms (an underestimate silently drops true winners); a coarse key that is NaN never
//   qualifies for the re-rank; a query without any finite coarse key has every row re-ranked;
//   segment table: S + 1 device ints, seg_start[0] = 0, non-decreasing, seg_start[S] <= the bank's rows, and NO EMPTY SEGMENT
//   (mocha_bank_set_segments refuses one: the finish kernels would read row seg_start[s] of it, which for the last segment is past the
//   bank); max_rows >= the largest segment (rows beyond max_rows would never be scanned); Q <= SEG_MAX_Q for launch_seg_plan and
//   launch_match_segmented (checked); the ids seg[q] may be ANY int - outside [0, S): no block, -1 / row 0 / +inf / weights 0 / enc[0];
//   launch_gather_blend: k <= 64, cols % 4 == 0, temperature > 0 (checked); neighbours with idx outside [0, nrows) are left out;
//   launch_gather_rows: idx clamped into [0, nrows).
// ---------------------------------------------------------------------------------------
// streaming matcher for few queries against a large bank (HBM-bound): bank fp32 or bf16;
// partial = match_stream_scratch(Q, N) u64 words of scratch
size_t match_stream_scratch(int Q, int64_t N);
hipError_t launch_match_stream(const void* bank, int bank_bf16, const float* query, int Q, int64_t N, int D,
                               unsigned long long* partial, int32_t* idx, float* dist, hipStream_t s);
// k nearest rows per query, exact (every row's direct-form distance, then a k-pass selection); keys = 8 * N u64 words of scratch
hipError_t launch_match_topk(const void* bank, int bank_bf16, const float* query, int Q, int64_t N, int D, int k,
                             unsigned long long* keys, int32_t* idx, float* dist, hipStream_t s);
// Coherent context matching (match_path.hip).  launch_match_dist: dist[i * ld + j] = the distance launch_match_topk reports for query i
// and row j of the `rows` fp32 rows at bank_rows, bit for bit; nothing outside [0, Q) x [0, rows) is written.  launch_match_path: the
// jump-penalised path of include/mocha_hip.h through d (Q x N, leading dimension ld); seq_start_dev (n_seq + 1) and bank_start_dev (n_b)
// are device lists the caller validated; scratch: start_bits match_path_bits_words(N) 32-bit words, m Q ints, cont
// match_path_cont_words(Q) 16-bit words.  N <= MATCH_PATH_MAX_ROWS.
static constexpr int MATCH_PATH_MAX_ROWS = 16384;
size_t match_dist_keys_words(int Q, int rows);       // u64 words of `keys`
hipError_t launch_match_dist(const float* bank_rows, const float* query, int Q, int rows, int D, unsigned long long* keys, float* dist, int64_t ld,
                             hipStream_t s);
hipError_t launch_path_rowmin(const float* d, int Q, int N, int64_t ld, float* out /*Q*/, hipStream_t s);      // out[i] = min_j d[i][j]
size_t match_path_bits_words(int N);
size_t match_path_cont_words(int Q);
hipError_t launch_match_path(const float* d, int Q, int N, int64_t ld, const int32_t* seq_start_dev, int n_seq, const int32_t* bank_start_dev,
                             int n_b, double lambda, unsigned* start_bits, int32_t* m, unsigned short* cont, int32_t* path, float* dist_out,
                             unsigned char* continued, hipStream_t s);
// Coherent matching, the online form (match_path_step.hip): one step of the path's forward recursion per stream, the recursion's row in
// the caller's state buffer.  State: `streams` headers of PATH_STEP_HDR_BYTES, then per stream two buffers of state_rows float64 switched
// by the header's parity word; all zero = reset.  One launch of `streams` workgroups.
//   ids (S): the streams' effective ids; negative sits out.  The extent of id e: rows != null (the pure form) {0, rows[s]}, epoch 0; else
//   seg_table (S + 1 starts, or pairs != 0: a resident bank's slot table) with epochs[e] (or null: 0).  An id outside the table, an empty
//   slot, or an extent of more than state_rows rows (or more than the loader's stride) sits out: idx -1, gidx 0, dist_out +inf, continued 0,
//   running = 0, R untouched.
//   start_bits (or null): bit bit0 + j set = row j starts a clip, bit0 = bit_off[s] (or 0) in the pure form and the extent's first row
//   otherwise; a bit outside [0, n_bits) reads as not set.  restart (or null): S ints, a non-zero word restarts the stream and is cleared.
//   Loader: keys != null - the all-keys scan's buffer, stream s at keys + s * kstride - else dist + s * ld.
//   Outputs: idx (S) local rows; gidx, dist_out, continued, dist_row (S, ld_row >= state_rows: every d[j] of the step) may be null.
static constexpr int PATH_STEP_MAX_STREAMS = 16;
static constexpr int PATH_STEP_HDR_BYTES = 64;
struct PathStepHdr {
    int32_t running, prev_id, prev_first, prev_rows, prev_epoch, m_prev, parity, pad0;
    double M, pad1[3];
};
struct PathStepArgs {
    void* state; int streams; int state_rows;
    const int32_t* ids;
    const int32_t* rows;
    const int* seg_table; int S; int pairs; const unsigned* epochs;
    const unsigned* start_bits; long long n_bits; const int32_t* bit_off;
    int32_t* restart;
    double lambda;
    const float* dist; long long ld;
    const unsigned long long* keys; int kstride;
    int32_t* idx; int32_t* gidx; float* dist_out; unsigned char* continued; float* dist_row; long long ld_row;
};
size_t path_step_state_bytes(int streams, int state_rows);
hipError_t launch_match_path_step(const PathStepArgs& a, hipStream_t s);
// the start bits of rows [first, first + rows) of a table of n_bits bits cleared, then bit first + start_dev[i] set for the n device starts
// (each inside [0, rows)); epoch (or null): the word is incremented.  rows = 0 with an epoch: the increment alone.
hipError_t launch_path_starts(unsigned* bits, int64_t n_bits, int64_t first, int64_t rows, const int32_t* start_dev, int n, unsigned* epoch, hipStream_t s);
// out[q] = sum_j softmax_j(-dist[q][j] / temperature) * src[idx[q][j]] over the k neighbours of query q
hipError_t launch_gather_blend(const float* src, const int32_t* idx, const float* dist, float temperature, float* out, int Q, int k,
                               int cols, int64_t nrows, hipStream_t s);
hipError_t launch_to_bf16(const float* x, const float* sub /*per-column, or null*/, int cols, void* y, int64_t n, hipStream_t s);
// fp32 bank scanned through its centred bf16 copy, exact re-rank of what the rounding cannot exclude (match_stream.hip)
hipError_t match_refine_init();
size_t match_scan16_scratch_words(int64_t N);        // launch_match_scan16's scratch buffer, in 8-byte words; the first ..._head_words() must be zero at first use
size_t match_scan16_scratch_head_words();
// the one-byte first stage of the few-query scan (match_scan8.hip; option "scan8"): image + per-row scale + residual bound, the adaptive scan + refine
hipError_t launch_to_i8(const float* x, const float* centre, void* y, float* scale, float* rho, int64_t rows, int cols, hipStream_t s);
hipError_t match_scan8_init();
size_t match_scan8_mode_word();                      // word of the scan16 scratch head that holds the stage's two mode words {this call, next calls}
hipError_t launch_match_scan8(const void* bank8, const float* scale8, const float* rho8, const void* bank16, const float* rho16, const float* bank,
                              const float* qc, const float* query, int Q, int64_t N, int D, unsigned long long* scratch, int32_t* idx, float* dist, hipStream_t s);
hipError_t launch_match_refine(const unsigned long long* keys, const unsigned long long* wgmin, int nwg, const float* rho16, const float* rho8, unsigned* mode,
                               const float* bank, const float* query, int nq, int64_t N, int D, int32_t* idx, float* dist, unsigned long long* scratch, hipStream_t s);
hipError_t launch_rowresid(const float* x, const float* centre, const void* x16, float* rho, int64_t rows, int cols, hipStream_t s);
hipError_t launch_match_scan16(const void* bank16, const float* rho, const float* bank, const float* qc, const float* query, int Q, int64_t N,
                               int D, unsigned long long* scratch, int32_t* idx, float* dist, hipStream_t s);
hipError_t launch_rownorm2_bf16(const void* x, float* out, int64_t rows, int cols, hipStream_t s);
// multi-character bank (match_segmented.hip): every query's exact 1-NN within its own row segment [seg_start[seg[q]], seg_start[seg[q] + 1]),
// the segment chosen by device data; bank fp32 rows or the centred bf16 copy (then centred queries).  idx: local row (-1 for an id outside
// [0, S)), gidx: global row (0 for such an id), dist (or null): direct-form distance (+inf for such an id).  Q <= SEG_MAX_Q per launch;
// partial = match_seg_scratch_words(Q, largest segment) u64 words, plan = seg_plan_ints(Q, S) ints.
static constexpr int SEG_MAX_Q = 4096;
size_t match_seg_scratch_words(int Q, int64_t max_rows);
size_t seg_plan_ints(int Q, int S);
// Action-constrained matching (the ALLOW instances of the two scans): every bank row carries a label 0..63, every query a 64-bit allow
// mask.  any[s] = OR of 1 << label over segment s.  Query q of segment s is CONSTRAINED iff (allow[q] & any[s]) != 0: its candidates are
// the rows of s whose label bit is in allow[q]; otherwise (zero mask: nothing asked; no row of those labels: fall back) it takes the plain
// answer.  gran[gran_start[s] + x] = OR of the label bits of the segment's rows [16 x, 16 x + 16): a scan workgroup none of whose queries
// admits any of its rows writes ~0 keys and returns without reading a bank row.  applied[q] (or null) = 1 constrained / 0 nothing asked
// (or an id outside [0, S)) / -1 fell back, written by the finish / blend kernel.  All pointers but `applied` are required; label: one
// byte per GLOBAL row, any: S words, gran_start: S + 1 ints, gran: gran_start[S] words; allow / applied: Q entries, as idx.
static constexpr int SEG_GRANULE_ROWS = 16;      // rows per granule word = rows per scan workgroup (match_seg_body.h)
struct SegAllow {
    const unsigned long long* allow;
    const unsigned char* label;
    const unsigned long long* any;
    const unsigned long long* gran;
    const int* gran_start;
    int32_t* applied;
};
// slot_table != 0 (here and in launch_match_seg_topk; fp32 bank only): seg_start is not S + 1 starts but a RESIDENT bank's slot table - 2 S
// device ints, {first row, rows} per slot, first row a multiple of SEG_GRANULE_ROWS, the extents disjoint and inside the bank, rows <=
// max_rows; rows = 0 is an EMPTY slot, whose id is treated as an id outside [0, S) (and no row of it is read).  gran_start[s] is then
// first row / SEG_GRANULE_ROWS.  The table is device data a replayed graph reads: launch_resident_publish rewrites an entry in stream order.
hipError_t launch_match_segmented(const void* bank, int bank_bf16, const float* query, const int32_t* seg, int Q, const int* seg_start, int S,
                                  int64_t max_rows, int D, unsigned long long* partial, int* plan, int32_t* idx, int32_t* gidx, float* dist,
                                  hipStream_t s, const SegAllow* al = nullptr, int slot_table = 0);
// resident bank (bank_resident.hip): the label tables of the rows [first_row, first_row + n) of a new character - label bytes (labels[r] &
// 63, or 0 for null labels), the granule words from first_row / 16 on, and *any_slot - and the slot table entry {first_row, rows} with
// gran_start[slot], written last; rows = 0 empties the slot.  One workgroup each; first_row a multiple of 16 and first_row + n <= capacity_rows (checked).
hipError_t launch_resident_labels(const int32_t* labels, int64_t n, int64_t first_row, int64_t capacity_rows, unsigned char* label,
                                  unsigned long long* gran, unsigned long long* any_slot, hipStream_t s);
hipError_t launch_resident_publish(int* slots, int* gran_start, int slot, int n_slots, int64_t first_row, int64_t rows, int64_t capacity_rows,
                                   hipStream_t s);
hipError_t launch_seg_plan(const int32_t* seg, int Q, int S, int* plan, hipStream_t s);      // the matcher's first kernel alone (plan = seg_plan_ints(Q, S) ints)
// soft matching on a multi-character bank (match_seg_topk.hip): per query the k <= SEG_TOPK_MAX_K nearest rows of its own segment - idx_k
// (Q,k) local rows ascending by distance, ties to the lower row, -1 where the segment has fewer than k rows; dist_k (Q,k) the distance
// launch_match_segmented reports for that row (+inf); w_k (Q,k) = softmax_j(-dist / temperature) over the neighbours present (0) - and
// out (Q,D) = sum_j w_k[j] enc[segment start + idx_k[j]].  idx0 (Q) = column 0 of idx_k.  Any of the five outputs may be null.  An id
// outside [0, S): -1 / +inf / 0 and out = enc[0].  Any Q: the queries are walked SEG_TOPK_Q at a time through keys =
// match_seg_keys_words(largest segment) u64 words; plan = seg_plan_ints(SEG_TOPK_Q, S) ints.
static constexpr int SEG_TOPK_MAX_K = 8;
static constexpr int SEG_TOPK_Q = 16;
size_t match_seg_keys_words(int64_t max_rows);
hipError_t launch_match_seg_topk(const void* bank, int bank_bf16, const float* query, const int32_t* seg, int Q, const int* seg_start, int S,
                                 int64_t max_rows, int D, unsigned long long* keys, int* plan, const float* enc, int k, float temperature,
                                 int32_t* idx0, int32_t* idx_k, float* dist_k, float* w_k, float* out, hipStream_t s,
                                 const SegAllow* al = nullptr,         // al: rows outside a constrained query's mask count as missing
                                 int slot_table = 0);
// the plan and the all-keys scan alone, on fp32 rows, for one group of Q <= SEG_TOPK_Q queries: keys[q * match_seg_key_stride(max_rows) +
// local row] for every row of query q's segment (an id outside the table: nothing written for it)
int match_seg_key_stride(int64_t max_rows);
hipError_t launch_match_seg_keys(const float* bank, const float* query, const int32_t* seg, int Q, const int* seg_start, int S, int64_t max_rows, int D,
                                 unsigned long long* keys, int* plan, hipStream_t s, int slot_table = 0);
// character mixing on a multi-character bank (match_seg_mix.hip): window q carries J <= SEG_MIX_MAX_J components (ids[q][j], six body-part
// weights weights[q][j][v]); every PRESENT component - a loaded character and at least one weight in (0, FLT_MAX] - is matched exactly in
// its own character as launch_match_segmented matches (that query, that id); the weights are normalised per part over the present
// components (a part nobody weighs goes to the lowest present component) and out (Q,D) = sum_j what[j][token % 6] enc[row_j] in
// launch_match_seg_topk's blend arithmetic.  idx / dist (Q,J): local rows / distances, -1 / +inf where not present; wnorm (Q,J,6): the
// normalised weights (0); dist, wnorm, out may be null.  A window with no present component: out = enc[0].  gate (or null): Q ints, a
// window whose gate is negative has no present component (a live stream still warming); valid (or null, live steps): Q ints, rewritten to
// 1 where a component is present and 0 elsewhere.  Q <= SEG_MIX_Q per launch; partial = match_seg_scratch_words(SEG_MIX_Q * SEG_MIX_MAX_J,
// largest segment) words, plan = seg_plan_ints(SEG_MIX_Q * SEG_MIX_MAX_J, S) ints, iscr = seg_mix_scratch_ints() ints, fscr =
// seg_mix_scratch_floats() floats.  D = 90 x 256 (tokens t x 6 + part, 256 channels).
static constexpr int SEG_MIX_MAX_J = 4;
static constexpr int SEG_MIX_Q = 16;
static constexpr int SEG_MIX_PARTS = 6;
size_t seg_mix_scratch_ints();
size_t seg_mix_scratch_floats();
hipError_t launch_match_seg_mix(const void* bank, int bank_bf16, const float* query, const int32_t* ids, const float* weights, int Q, int J,
                                const int* seg_start, int S, int64_t max_rows, int D, unsigned long long* partial, int* plan, int32_t* iscr,
                                float* fscr, const float* enc, const int32_t* gate, int32_t* valid, int32_t* idx, float* dist, float* wnorm,
                                float* out, hipStream_t s, int slot_table = 0);
// out[q] = src[idx[q]] rows of `cols` floats
hipError_t launch_gather_rows(const float* src, const int32_t* idx, float* out, int Q, int cols, int64_t nrows, hipStream_t s);

}  // namespace mocha
