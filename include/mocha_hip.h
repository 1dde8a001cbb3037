/*
 * mocha_hip.h — C ABI of libmocha_hip.so: the MI355X (gfx950) implementation of the MOCHA
 * Generator hot path (motion encoder -> context matching -> body-part decoder).
 *
 * The reference (DK-Jang/MOCHA_SIGASIA2023) is pure Python and has no FFI of its own; the
 * boundary it offers is the attribute surface of its `Generator` module plus the
 * `gen_ema` state_dict key schema.  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference repository root).
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every tensor pointer is a DEVICE pointer to contiguous fp32 unless a comment says host;
 *   - layouts are the reference's: poses (B, T, V, C_in) channel-last, tokens (B, 90, 256)
 *     with token = t*6 + body_part (model.py:49), bank entries likewise;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it.  Steady-state calls do not synchronise
 *     the device and are graph-capture safe; device allocations (and the device synchronisation that replacing a
 *     buffer needs) only happen in mocha_finalize_weights, mocha_reserve, mocha_bank_set (both also size the match
 *     scratch for every query count the workspace admits), mocha_bank_set_segments (also the segmented calls' scratch),
 *     mocha_bank_broadcast, mocha_set_option and the first call
 *     with a batch larger than any before.  Each such replacement bumps mocha_generation(ctx): a caller that captured
 *     calls into its own HIP graph compares the generation before replaying (mocha_step_graph does so itself);
 *   - a NULL where a required device pointer belongs is MOCHA_ERR_ARG ("... null argument"), never a launch; with an empty batch
 *     (B == 0) the tensor pointers may be NULL and nothing is touched (tests/test_edge_cases.py);
 *   - functions return 0 on success, a negative mocha_status otherwise;
 *     mocha_last_error(ctx) gives the message.  The caller owns every in/out buffer; the
 *     context owns the device copies of the weights, the bank (unless borrowed) and the
 *     workspaces.  One context per device per host thread.
 *   - several contexts of one process may be driven concurrently from different streams (tests/test_runtime_gpu.py runs two whole
 *     pipelines side by side on same-priority and on different-priority streams and compares them bit for bit with the sequential
 *     results); a context itself serves one call at a time.
 *   - a platform hazard found in round 2, for applications that run THEIR OWN kernels on another stream while this library works:
 *     a kernel that issues ordinary VALU instructions between bf16 MFMAs (the plane engines do) was observed to corrupt the results
 *     of `v_pk_fma_f32 ... op_sel` (low result from a high VGPR) in OTHER kernels sharing its CU - lanes 48-63, value 0
 *     (tools/body_front_repro.hip reproduces it without this library's pipeline).  What is established by test, not by guess
 *     (tests/test_concurrency_stress.py, run on every GPU test pass): under that aggressor - large-batch plane GEMMs and plane
 *     attention streaming from a second context - the round-2 build of the affected kernel (kept as a test-only canary) differs
 *     from its solo result in more than half of 3 000 repetitions, while EVERY kernel class of this library, each repeated 1 000
 *     times on same- and different-priority streams, reproduces its solo result bit for bit - including the kernels that use
 *     packed fp32 arithmetic by design (mocha_match_stream) or by the compiler's choice (GEMM epilogues, window sums, norms).
 *     tools/isa_lint.py additionally keeps the one pattern that failed (low result from the HIGH register of a VGPR pair) out
 *     of the library's device code.  If foreign kernels must overlap with the library's calls and may contain that pattern,
 *     order them after the library's stream, or run with mocha_set_option "gemm_bf16x3" = 0 and "attention_bf16x3" = 0.
 *     Scope of this statement: ONE builder-written reproduction, observed on the boxes of this build's GPU pool - MI355X (gfx950:sramecc+:xnack-),
 *     kernel driver 6.18.51, ROCm runtime 7.0.2 (HIP 7.0.51831), code objects built with hipcc 7.2.26015, VBIOS 113-M355-01-1K1-020F,
 *     firmware MEC 44 / RLC 43 / SDMA 14 / SMC 04.86.15.106 (profiles/r05/c_versions.txt) - not a vendor erratum and not re-checked
 *     on any other driver / firmware; the canary test re-measures it on whatever box runs the GPU suite.
 */
#ifndef MOCHA_HIP_H
#define MOCHA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mocha_ctx mocha_ctx;

typedef enum {
    MOCHA_OK = 0,
    MOCHA_ERR_ARG = -1,      /* bad argument / unsupported configuration */
    MOCHA_ERR_HIP = -2,      /* a HIP runtime call failed */
    MOCHA_ERR_STATE = -3,    /* call order violated (weights not finalised, no bank, ...) */
    MOCHA_ERR_WEIGHT = -4    /* unknown weight name or wrong shape */
} mocha_status;

/* The 14 model dimensions Generator.__init__ reads (model.py:18-33, configs/config.yaml:13-31)
 * plus the skeleton layout (0 = 'mocha' 24 joints, 1 = 'mixamo' 22 joints; net/graph.py). */
typedef struct {
    int T, V, C_in, patch, dim;
    int enc_depth, enc_heads, enc_dim_head, enc_mlp;
    int dec_depth, dec_heads, dec_dim_head, dec_mlp;
    int layout;
} mocha_cfg;

/* Generator(cfg) construction, model.py:16-80 / trainer.py:22-23. */
int mocha_create(const mocha_cfg* cfg, int device, mocha_ctx** out);
void mocha_destroy(mocha_ctx* ctx);
const char* mocha_last_error(const mocha_ctx* ctx);   /* ctx may be NULL: last create error */

/* load_state_dict, trainer.py:239-240: one call per state_dict entry, `host` is HOST fp32.
 * Names are exactly the reference's ("mot_embedding.2.blk.gcn.conv.weight", ...).  The graph
 * buffers (A_j, A_b, pool/unpool weights) are accepted and cross-checked against the
 * regenerated constants. */
int mocha_load_weight(mocha_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
/* After the last mocha_load_weight: checks completeness, repacks weights into kernel layouts. */
int mocha_finalize_weights(mocha_ctx* ctx);

/* Pre-allocate workspaces for up to `max_batch` windows per internal chunk (larger B is
 * processed in chunks).  Optional; called lazily otherwise (not graph-capture safe then). */
int mocha_reserve(mocha_ctx* ctx, int max_batch);

/* model.pos_emb (model.py:40; test_fullframework.py:191): device pointer to (90, 256). */
int mocha_pos_emb(mocha_ctx* ctx, const float** dev_ptr);

/* model.mot_embedding(X), model.py:42-50 (test_fullframework.py:190).
 * X (B,T,V,C_in) -> tokens (B,90,256); add_pos != 0 fuses `+ pos_emb` (test_fullframework.py:191). */
int mocha_embed(mocha_ctx* ctx, const float* X, int B, float* tokens, int add_pos, void* stream);
/* model.encoder(tokens), model.py:53-59, net/transformer.py:90-95 (test_fullframework.py:192). */
int mocha_encoder(mocha_ctx* ctx, const float* tokens, int B, float* encoded, void* stream);
/* mean_variance_norm(encoded.permute(0,2,1)).permute(0,2,1), net/transformer.py:13-20
 * (test_fullframework.py:193).  If cnt_nm is non-NULL also writes cnt_nm = (cnt - cnt_mean) / cnt_std
 * (test_fullframework.py:293,297,442; cnt_mean / cnt_std (90,256) are then required).  cnt may be NULL when only cnt_nm is
 * wanted (at least one of the two must be given). */
int mocha_mvn(mocha_ctx* ctx, const float* encoded, int B, float* cnt,
              const float* cnt_mean, const float* cnt_std, float* cnt_nm, void* stream);
/* Fused demo encode sequence test_fullframework.py:190-193: embed, +pos_emb, encoder and - each when its pointer is non-NULL -
 * the cnt feature and its z-scored copy cnt_nm (as in mocha_mvn: cnt_nm needs cnt_mean / cnt_std, not cnt). */
int mocha_encode(mocha_ctx* ctx, const float* X, int B, float* encoded, float* cnt,
                 const float* cnt_mean, const float* cnt_std, float* cnt_nm, void* stream);
/* model.decoder(src_enc, cha_enc), model.py:62-68, net/transformer.py:90-121 (test_fullframework.py:301,455,465). */
int mocha_decoder(mocha_ctx* ctx, const float* src_enc, const float* cha_enc, int B, float* out, void* stream);
/* AdaIN's style constants of character features (net/transformer.py:98-107: AdaptiveAvgPool1d over the tokens, Linear 256->512,
 * LeakyReLU(0.2), Linear 512->512, of EVERY decoder layer): gb (B, 512 * decoder_depth) = [gamma_0 | beta_0 | gamma_1 | beta_1 | ...] for
 * cha_enc (B, 90, 256) - what model.decoder computes from its second argument before anything else, and what mocha_bank_set caches per
 * bank entry ("bank_dec_cache").  In float64 from a float64 token mean, rounded to fp32 once, unless "style_f64" = 0. */
int mocha_style_constants(mocha_ctx* ctx, const float* cha_enc, int B, float* gb, void* stream);

/* model.to_mot(tokens), model.py:71-80 (test_fullframework.py:302,456,466). */
int mocha_to_mot(mocha_ctx* ctx, const float* tokens, int B, float* Y, void* stream);
/* Generator.forward(src_X, cha_X), model.py:82-106. */
int mocha_forward(mocha_ctx* ctx, const float* src_X, const float* cha_X, int B, float* Y, void* stream);
/* Generator.forward(..., extract_feature=True), model.py:95-98. */
int mocha_forward_features(mocha_ctx* ctx, const float* src_X, const float* cha_X, int B,
                           float* src_enc, float* cha_enc, float* src_cnt, float* cha_cnt, void* stream);

/* Character feature bank = what BallTree(cha_cnt_nm) + cha_encoded hold in the demo
 * (test_fullframework.py:293-294, 298).  cnt_nm (N, 90*256) are the z-scored cnt features,
 * encoded (N, 90, 256) the features gathered for the decoder.  flags bit 0: borrow the
 * caller's buffers instead of copying (they must stay valid and unchanged). */
#define MOCHA_BANK_BORROW 1
/* flags bit 1: additionally keep a bf16 copy of cnt_nm (round-to-nearest-even) and match against it
 * (half the HBM bytes per bank scan; BASELINE configs[2]); indices then agree with the fp32 search
 * except where the two nearest distances differ by less than the bf16 rounding of the bank.
 * fp32 banks of up to 4096 rows additionally keep the packed three-plane image of the centred bank (6 bytes per value, made by
 * mocha_bank_set) that many-query matching multiplies on the bf16 pipe when "gemm_bf16x3" is on - exact planes, the same indices.
 * fp32 banks of at least 4096 rows additionally keep a centred bf16 copy (2 bytes per value) and one residual norm per row
 * (option "scan16", default 1): matching of up to 8 queries scans the copy - the scan is HBM-bound, half the bytes - and
 * re-evaluates on the fp32 rows, exactly, every row the copy's rounding cannot exclude (triangle inequality on the measured
 * residuals): the indices and distances of the fp32 search, not of a bf16 bank. */
#define MOCHA_BANK_BF16 2
/* flags bit 2: do not compute the per-entry decoder constants of option "bank_dec_cache" for this bank (+ 92 KB per entry saved; the decoder
 * then derives them per call, as with the option off) - the option itself is left as it is. */
#define MOCHA_BANK_NO_DEC_CACHE 4
int mocha_bank_set(mocha_ctx* ctx, const float* cnt_nm, const float* encoded, int64_t N, int flags, void* stream);
/* tree.query(q, k=1), test_fullframework.py:296,443: exact Euclidean 1-NN of each z-scored
 * query row (Q, 90*256) in the bank.  idx (Q,) int32; dist (Q,) fp32 Euclidean distance to the
 * winner (may be NULL). */
int mocha_match(mocha_ctx* ctx, const float* query_nm, int Q, int32_t* idx, float* dist, void* stream);
/* tree.query(q, k) for k > 1 (scikit-learn BallTree semantics; the reference only ever asks for k = 1, SURVEY.md §8f N4 lists
 * k > 1 as optional): the k nearest rows of every query, exact, distances ascending, ties to the lower row index.
 * idx (Q,k) int32 (-1 where the bank has fewer than k rows), dist (Q,k) fp32 or NULL.  One bank scan per 8 queries - a
 * convenience, not a fast path; allocates its scratch on first use.
 * mocha_bank_gather_blend: soft matching over those neighbours, out (Q,90,256) = sum_j softmax_j(-dist[q][j] / temperature) *
 * bank.encoded[idx[q][j]] (entries with idx < 0 left out; k <= 64, temperature > 0). */
int mocha_match_topk(mocha_ctx* ctx, const float* query_nm, int Q, int k, int32_t* idx, float* dist, void* stream);
int mocha_bank_gather_blend(mocha_ctx* ctx, const int32_t* idx, const float* dist, float temperature, int Q, int k, float* out,
                            void* stream);
/* cha_encoded[frame_index], test_fullframework.py:298,465: out (Q,90,256) = bank.encoded[idx[q]]. */
int mocha_bank_gather(mocha_ctx* ctx, const int32_t* idx, int Q, float* out, void* stream);

/* The NN ("cm_") branch of the demo, batched over all source windows
 * (test_fullframework.py:188-194, 288-302, 438-443, 465-467): encode src, match against the
 * current bank, gather, decode, to_mot.  Y (B,T,V,C_in); idx (B,) may be NULL. */
int mocha_characterize(mocha_ctx* ctx, const float* src_X, int B, const float* cnt_mean, const float* cnt_std,
                       float* Y, int32_t* idx, void* stream);

/* One streamed window per call (BASELINE configs[4]; the demo's per-frame loop test_fullframework.py:438-443, 465-467):
 * mocha_characterize with B = 1, captured into a HIP graph on first use and replayed afterwards (one graph launch
 * instead of ~45 kernel launches).  The graph is keyed on the five buffer pointers, `raw` and mocha_generation(ctx);
 * it is re-captured transparently when any of them changes (new bank, grown workspace, other buffers).  X1 (1,T,V,C_in)
 * [raw != 0: (1,T,V+1,C_in) un-normalised, after mocha_set_pose_norm], Y1 (1,T,V,C_in), idx (1,); all device memory
 * that stays valid between calls.  `stream` may be the null stream (capture runs on an internal stream). */
int mocha_step_graph(mocha_ctx* ctx, const float* X1, const float* cnt_mean, const float* cnt_std, float* Y1, int32_t* idx,
                     int raw, void* stream);
/* The same step on one of the context's LANES (mocha_set_option "lanes" = 1..3; lane 0 is mocha_step_graph).  Every lane has
 * its own workspace set, match scratch and captured graph, so the steps of up to three consecutive windows can be in flight
 * at once, each on its own stream: windows are independent (test_fullframework.py:148-158) and the step alternates a
 * latency-bound chain of small kernels (encode, decode) with an HBM-bound bank scan, so window i + 1's chains run under
 * window i's scan.  The caller gives every lane its own X1 / Y1 / idx buffers and stream; results of one lane are ordered by
 * that stream as usual.  Weights and the bank are shared and read-only. */
int mocha_step_graph_lane(mocha_ctx* ctx, int lane, const float* X1, const float* cnt_mean, const float* cnt_std, float* Y1,
                          int32_t* idx, int raw, void* stream);

/* Several characters served per call from ONE multi-character bank.  The characters' banks (each z-scored with the same global
 * cnt_mean / cnt_std) are concatenated into N rows; segment s = rows [seg_start[s], seg_start[s + 1]) is character s's bank.
 *   mocha_bank_set_segments : mocha_bank_set over the N rows (same flags, same derived data and decoder-constant cache), plus the segment
 *                             table.  seg_start (HOST, S + 1 entries) runs from 0 to N and every segment holds at least one row, else
 *                             MOCHA_ERR_ARG.  Sizes all the scratch of the segmented calls below (graph-capture safe: they never allocate).
 *                             mocha_bank_set and mocha_bank_broadcast clear the table; a segmented call without one is MOCHA_ERR_STATE.
 *                             Every other call on a segmented bank (mocha_match, mocha_match_topk, mocha_characterize, mocha_step_graph,
 *                             gathers) searches / reads the UNION of all rows, as after mocha_bank_set of the concatenation (the soft
 *                             calls further down are segmented).
 *   mocha_match_segmented   : exact 1-NN of each query (Q, 90*256) within its own segment seg[q] (DEVICE, Q int32): idx (Q,) the row LOCAL
 *                             to the segment (BallTree(that character's cnt_nm).query(k=1)), ties to the lowest row; dist (Q,) or NULL, the
 *                             Euclidean distance in the bank's arithmetic (fp32 rows; MOCHA_BANK_BF16: the bf16 copy centred on the union's
 *                             centroid, with centred queries).  An id outside [0, S): idx -1, dist +inf, and no bank row is read for it.
 *                             Cost: one pass over rows(segment) x 90*256 values per block of up to 8 queries sharing a segment.
 *   mocha_characterize_segmented : mocha_characterize (raw != 0: mocha_characterize_raw) with every window matched in its own segment;
 *                             idx (B,) local rows or NULL.  A window with an invalid id gets idx -1 and an unspecified Y (its decoder reads
 *                             row 0).
 *   mocha_step_graph_segmented : that call for S_w windows (1 <= S_w <= 16; X (S_w,T,V,C_in) device, one window per stream of the caller),
 *                             captured into a HIP graph on first use and replayed, as mocha_step_graph.  The graph is keyed on the buffer
 *                             pointers, S_w, raw and the generation; new ids written into seg between calls are read by the replay and do
 *                             not re-capture.  Uses workspace set 0 (as mocha_characterize and mocha_step_graph): drive the context from
 *                             one stream at a time. */
int mocha_bank_set_segments(mocha_ctx* ctx, const float* cnt_nm, const float* encoded, int64_t N, const int64_t* seg_start, int S, int flags,
                            void* stream);
int mocha_match_segmented(mocha_ctx* ctx, const float* query_nm, int Q, const int32_t* seg, int32_t* idx, float* dist, void* stream);
int mocha_characterize_segmented(mocha_ctx* ctx, const float* src_X, int B, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                                 float* Y, int32_t* idx, int raw, void* stream);
int mocha_step_graph_segmented(mocha_ctx* ctx, const float* X, int S_w, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                               float* Y, int32_t* idx, int raw, void* stream);

/* Soft context matching on a multi-character bank: the decoder's character feature as the softmax-weighted blend of the k nearest entries
 * of the window's OWN segment instead of the one nearest entry - tree.query(q, k) on that character's BallTree and a blend of
 * cha_encoded[frame_index[:, j]], which the reference (k = 1 only, test_fullframework.py:296,443) does not have.  With a hard 1-NN the
 * nearest row of a live stream flips whenever two entries are nearly equidistant and the pose pops; the blend moves continuously and needs
 * nothing trained.  1 <= k <= MOCHA_SOFT_MAX_K, temperature > 0 (else MOCHA_ERR_ARG, before anything is launched); a NULL required pointer is
 * MOCHA_ERR_ARG and a bank without a segment table MOCHA_ERR_STATE, as in the hard calls.  Nothing here allocates: mocha_bank_set_segments
 * also reserves the key buffer (16 queries x the largest segment's rows rounded up to 16, 8 bytes each, per workspace set: 2 MB at 16 384
 * rows).  The matcher therefore takes 16 queries at a time: a larger batch walks its windows 16 at a time inside the workspace chunk, ONE
 * PASS OVER THE QUERIES' SEGMENTS PER 16 WINDOWS at worst (the hard matcher: per 8 windows of one segment in a launch of up to 4 096).
 *   mocha_match_topk_segmented : replaces BallTree(character seg[q]'s cnt_nm).query(q, k) per character.  idx (Q,k) int32 rows LOCAL to the
 *                             segment, nearest first, ties to the lower row, -1 where the segment has fewer than k rows; dist (Q,k) or NULL,
 *                             the Euclidean distance in the bank's arithmetic as mocha_match_segmented reports it (column 0 is that call's
 *                             answer to the bit), +inf for a missing neighbour.  The order is that of the scan's squared distances, which
 *                             are mocha_match_segmented's to the bit (one scan body).  An id outside [0, S): idx -1, dist +inf, no bank row
 *                             read.  Cost: the scan of mocha_match_segmented (the same bytes; + 8 bytes written per row and query), one
 *                             read of the query's keys, and k bank rows re-read per query for the reported distances.
 *   mocha_characterize_soft_segmented : mocha_characterize_segmented with, per window, w = softmax_j(-dist_j / temperature) over the
 *                             neighbours present (max-subtracted as in mocha_bank_gather_blend: exp(-(dist_j - dist_min) / temperature), normalised) and the decoder run on
 *                             sum_j w_j encoded[segment start + idx_j] (j ascending, fp32, every product and sum rounded on its own).
 *                             idx_k / w_k (B,k) or NULL; a missing neighbour has weight 0.  k = 1 is mocha_characterize_segmented bit for bit
 *                             (weight 1).  A window with an invalid id: idx -1, w 0, an unspecified Y (its decoder reads row 0).  Cost over
 *                             the hard call: k encoded rows read per window for the blend, and the decoder's per-call flow (instance norm
 *                             and style MLP of the blended feature) - the bank's per-entry decoder constants do not apply to a blend.
 *   mocha_step_graph_soft_segmented : that call for 1 <= S_w <= 16 windows captured into a HIP graph and replayed, as
 *                             mocha_step_graph_segmented; idx_k / w_k required.  Keyed on the buffer pointers, S_w, raw, k, the temperature
 *                             and the generation: new k or temperature re-captures, new ids in seg are read by the replay.  Before a capture
 *                             the step runs once eagerly (first-use images of its kernels must exist before capture).
 *   mocha_live_step_soft    : mocha_live_step with that characterize in place of the hard one: the same session buffer, mocha_live_reset,
 *                             warming rule and refusals; idx (S) receives column 0 of idx_k (S,k); idx_k / w_k required, a warming stream
 *                             gets -1 / 0.  Its own captured graph, keyed as mocha_live_step's plus k, the temperature, idx_k and w_k. */
#define MOCHA_SOFT_MAX_K 8
int mocha_match_topk_segmented(mocha_ctx* ctx, const float* query_nm, int Q, const int32_t* seg, int k, int32_t* idx, float* dist, void* stream);
int mocha_characterize_soft_segmented(mocha_ctx* ctx, const float* src_X, int B, const int32_t* seg, int k, float temperature,
                                      const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int raw, void* stream);
int mocha_step_graph_soft_segmented(mocha_ctx* ctx, const float* X, int S_w, const int32_t* seg, int k, float temperature, const float* cnt_mean,
                                    const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int raw, void* stream);
/* (mocha_live_step_soft is declared below, after mocha_live_step.) */

/* Action-constrained context matching on a multi-character bank: "this character is crawling now".  The reference picks an action, keeps
 * the character's windows of that action and builds its BallTree over that subset (train_CVAE.py:181-211; one bank per action list in
 * collect_CVAE_feature_action.py:50-63,104-108).  Here every ROW carries an action label 0..63 and every QUERY a 64-bit allow mask (bit a
 * set: rows of action a are admissible), both device-side data of ONE bank:
 *   any[s] = OR of (1 << label) over the rows of segment s.  A query of character s with mask m is CONSTRAINED iff (m & any[s]) != 0: its
 *   answer is the exact nearest neighbour (or the k nearest) among the rows of segment s whose label bit is in m - ties to the lowest row,
 *   the index LOCAL to the segment and counting ALL its rows (not the subset's), the distance in the bank's arithmetic, missing neighbours
 *   -1 / +inf / weight 0, exactly as mocha_match_segmented / mocha_match_topk_segmented.  m == 0 (nothing asked) and (m & any[s]) == 0
 *   (the character has no entry of those actions: the match FALLS BACK to the whole segment) take the unconstrained answer to the bit.
 *   applied (int32 per query, or NULL): 1 constrained, 0 nothing asked, -1 fell back; an id outside [0, S): idx -1, dist +inf, applied 0.
 * A row's squared distance does not depend on the other rows, so on an fp32 bank a constrained answer has the bits the plain call gives on
 * a bank made of the admissible rows alone.  The scan skips every 16-row workgroup none of whose queries admits a label it holds, before
 * its first bank row: with labels in runs (one per clip range) a constrained match reads about the admissible share of the segment.  The
 * launch count is the plain match's.  The plain calls and their results are unchanged.
 *   mocha_bank_set_labels : labels (HOST, N int32) of the rows of the current segmented bank; MOCHA_ERR_STATE without a segment table,
 *                             MOCHA_ERR_ARG for a label outside 0..63 (the previous labels stay).  Builds the device tables (1 byte per
 *                             row, 8 bytes per segment and per 16 rows) and synchronises the stream; the constrained calls never allocate.
 *                             Moves the generation.  labels == NULL removes the labels.  mocha_bank_set, mocha_bank_set_segments and
 *                             mocha_bank_broadcast clear them, as they clear the segment table; a constrained call on a bank without
 *                             labels is MOCHA_ERR_STATE.
 *   mocha_match_segmented_allow : allow (DEVICE, Q uint64).  k == 1: mocha_match_segmented's idx (Q) / dist (Q) or NULL; 2 <= k <=
 *                             MOCHA_SOFT_MAX_K: mocha_match_topk_segmented's (Q,k) outputs (whose column 0 is the k == 1 answer to the
 *                             bit).  applied (Q) or NULL.
 *   mocha_characterize_segmented_allow : k == 0: mocha_characterize_segmented (idx_k holds B entries or is NULL, w_k may be NULL);
 *                             k >= 1: mocha_characterize_soft_segmented.  applied (B) or NULL.
 *   mocha_step_graph_segmented_allow : that call for 1 <= S_w <= 16 windows captured and replayed (idx_k required; w_k for k >= 1).  The
 *                             graph key gains the allow and applied pointers: new masks written into allow are read by the replay and do
 *                             not re-capture.
 *   mocha_live_step_allow / mocha_live_step_raw_allow (declared with the live calls below): the argument lists of mocha_live_step_inert /
 *                             mocha_live_step_raw (k == 0: hard; inert may be NULL), then allow (S uint64, DEVICE) and applied (S) or
 *                             NULL.  Each has its own captured graph; a warming stream gets applied 0.
 * NOT covered: the calls that search the union of all rows (mocha_match, mocha_characterize, mocha_step_graph), the seed match of
 * mocha_live_step_ours, and inertializing a CHANGE of the allowed actions (the inertializer triggers on a change of character only; soft
 * matching already softens a change of mask). */
int mocha_bank_set_labels(mocha_ctx* ctx, const int32_t* labels, void* stream);
int mocha_match_segmented_allow(mocha_ctx* ctx, const float* query_nm, int Q, const int32_t* seg, const uint64_t* allow, int k, int32_t* idx,
                                float* dist, int32_t* applied, void* stream);
int mocha_characterize_segmented_allow(mocha_ctx* ctx, const float* src_X, int B, const int32_t* seg, const uint64_t* allow, int k,
                                       float temperature, const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx_k, float* w_k,
                                       int32_t* applied, int raw, void* stream);
int mocha_step_graph_segmented_allow(mocha_ctx* ctx, const float* X, int S_w, const int32_t* seg, const uint64_t* allow, int k,
                                     float temperature, const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx_k, float* w_k,
                                     int32_t* applied, int raw, void* stream);

/* Resident multi-character bank: characters added and retired in place, while the captured steps keep replaying.
 * mocha_bank_set_segments fixes the set of characters: one more character means a concatenation of every character's rows, the whole
 * union's derived data over again, and a new generation - every captured segmented and live step is thrown away, and for the duration
 * the bank exists twice.  A resident bank reserves its storage, tables and scratch ONCE; a character then costs its own bytes and its own
 * style MLP, enqueued on the caller's stream, and mocha_generation() does not move.  Each character occupies a SLOT (its id in the
 * segmented and live calls, 0 .. max_characters - 1) and an extent of whole 16-row granules, first fit, never moved (no compaction).
 *   mocha_bank_resident_create : the context's current bank becomes an EMPTY resident bank for up to capacity_rows rows (rounded up to
 *                             16) in up to max_characters slots of up to max_rows_per_character rows each.  fp32 only and owned:
 *                             MOCHA_BANK_BF16 or MOCHA_BANK_BORROW is MOCHA_ERR_ARG; MOCHA_BANK_NO_DEC_CACHE is honoured.  Allocates,
 *                             zero-filled, the rows, the per-entry decoder constants (if the memory is not there the decoder computes them
 *                             per call, as for any bank), the label and slot tables and the segmented matcher's scratch of every workspace
 *                             set, sized by the two maxima.  Moves the generation once, as any new bank.  After it, add, retire and every
 *                             segmented or live call neither allocate, nor synchronise, nor move the generation; mocha_reserve re-sizes
 *                             the matcher's scratch itself (and moves the generation, as workspace growth does).  The scan grid of every
 *                             segmented call is sized by max_rows_per_character, not by the largest character loaded.
 *   mocha_bank_resident_add : the n rows cnt_nm / encoded (DEVICE, as mocha_bank_set_segments takes them) with labels (DEVICE, n int32, read
 *                             as label & 63; NULL: every row label 0) become the character of `slot` (-1: the lowest empty slot); the slot
 *                             taken goes to slot_out (HOST, or NULL).  Enqueues two row copies, the rows' decoder constants - the bits
 *                             of the style MLP's tiled float64 kernel, however few the rows are (what mocha_bank_set_segments computes for every
 *                             chunk of more than 16 rows; it walks a bank 4096 rows at a time, and a chunk of at most 16 rows - a bank
 *                             that small, or such a remainder - takes a wave-reduction kernel with another summation order) - their label
 *                             tables and, last, the slot's table entry.  Refused before anything is enqueued: a slot out of range, n < 1
 *                             or n > max_rows_per_character (MOCHA_ERR_ARG); an occupied slot, no empty slot, no free extent of n rows
 *                             (MOCHA_ERR_STATE; the message names the largest free extent).
 *   mocha_bank_resident_retire : the slot becomes empty (row count 0 in the table) and its extent free.  Its rows are not cleared: an empty
 *                             slot is never read.  Replacing a character is retire + add of the same slot on the same stream.  Ordering
 *                             is the stream's: a context is driven from one stream at a time, as for the graph steps.
 *   mocha_bank_resident_info : host-side.  slot >= 0: its first row and row count (0: empty); always: the free rows and the largest
 *                             free extent, in rows.  Any output may be NULL.  slot -1: the bank's figures only.
 * An id that names an EMPTY slot is treated as an id outside [0, S): idx -1, dist +inf, weights 0, applied 0, no bank row read for the
 * match.  In the live steps - on a resident bank only - a stream that names an empty slot is treated as WARMING: its frame goes into its
 * ring, valid[s] = 0, idx[s] = -1, its post state is not advanced and its output rows are left untouched; it resumes with the first frame
 * after the slot holds a character again.  The calls that search or read the union of all rows - mocha_match, mocha_match_topk,
 * mocha_characterize, mocha_step_graph[_lane], mocha_bank_gather[_blend], mocha_bank_export, mocha_bank_view, mocha_bank_broadcast - and
 * mocha_bank_set_labels are MOCHA_ERR_STATE on a resident bank (no centroid, norms or images are built; it is always labelled, through
 * add); mocha_bank_set* replaces it as it replaces any bank. */
int mocha_bank_resident_create(mocha_ctx* ctx, int64_t capacity_rows, int max_characters, int64_t max_rows_per_character, int flags,
                               void* stream);
int mocha_bank_resident_add(mocha_ctx* ctx, int slot, const float* cnt_nm, const float* encoded, int64_t n, const int32_t* labels,
                            int32_t* slot_out, void* stream);
int mocha_bank_resident_retire(mocha_ctx* ctx, int slot, void* stream);
int mocha_bank_resident_info(const mocha_ctx* ctx, int slot, int64_t* first_row, int64_t* rows, int64_t* free_rows, int64_t* largest_free);

/* Multi-GPU set-up: one process per GPU, windows sharded across ranks, the character bank replicated.
 * The reference has no counterpart (trainer.py:45-47 is nn.DataParallel); the only exchange on the path is this one-time
 * bank broadcast over RCCL / xGMI.  RCCL is loaded lazily (dlopen "librccl.so.1"); single-GPU callers never touch it.
 *   mocha_comm_unique_id : rank 0 obtains the 128-byte ncclUniqueId (HOST buffer) and ships it to the other ranks by any
 *                          means (torch.distributed, MPI, a file);
 *   mocha_comm_init      : every rank joins (ncclCommInitRank) — collective;
 *   mocha_bank_broadcast : the root's current bank (mocha_bank_set, N entries) becomes every rank's current bank.
 *                          cnt_nm and encoded travel as scatter (grouped ncclSend/ncclRecv of 1/world each) + in-place
 *                          ncclAllGather, so that every xGMI link of the root carries a share instead of one ring
 *                          neighbour carrying all of it; centroid, row norms and the optional bf16 copy (flags &
 *                          MOCHA_BANK_BF16) are recomputed locally.  `comm` = an ncclComm_t created by the same librccl,
 *                          or NULL for the context's own.  Collective.  Every rank first contributes a 16-byte header
 *                          {entries, bf16?} as it understands the call; the headers are all-gathered and checked by
 *                          every rank (one stream synchronisation), so a root without that bank, a flags mismatch or a
 *                          single rank naming another size fails on ALL ranks instead of hanging some of them; the
 *                          payload is then enqueued on `stream`.
 *   mocha_set_rccl_library: which librccl to resolve (before the first mocha_comm_* call; process-wide).  A process that
 *                          already holds an RCCL - PyTorch wheels bundle their own copy - should name that file, so that one
 *                          RCCL instance serves the process; NULL / never called: "librccl.so.1" from the loader path. */
int mocha_set_rccl_library(const char* path);
int mocha_comm_unique_id(mocha_ctx* ctx, void* id128);
int mocha_comm_init(mocha_ctx* ctx, const void* id128, int nranks, int rank);
int mocha_comm_destroy(mocha_ctx* ctx);
int mocha_bank_broadcast(mocha_ctx* ctx, void* comm, int root, int64_t N, int flags, void* stream);
/* The plan mocha_bank_broadcast follows for one tensor of `count` floats over `world` ranks (host-side, pure; exposed so
 * that the split can be tested without a GPU): out = {offset of this rank's chunk, chunk length, offset of the tail, tail
 * length}.  Chunk r is scattered root -> r and all-gathered; the count % world tail is broadcast whole. */
int mocha_bcast_plan(int64_t count, int world, int rank, int64_t out[4]);
/* What the context's communicator really is, for the bench line and for logs (bench.py's `rccl` record): ranks and this rank
 * as RCCL itself reports them (ncclCommCount / ncclCommUserRank on the communicator mocha_comm_init made - not the caller's
 * arguments), ncclGetVersion's code (major * 10000 + minor * 100 + patch), the file the RCCL entry points were resolved
 * from (dladdr on ncclCommInitRank: a stand-in or a second RCCL cannot pass unnoticed), the context's device ordinal and
 * its PCI bus id (hipDeviceGetPCIBusId).  MOCHA_ERR_STATE without a communicator.  Host-side, no synchronisation. */
typedef struct {
    int nranks, rank, rccl_version, device;
    char pci_bus_id[32];
    char library[512];
} mocha_comm_info_t;
int mocha_comm_info(mocha_ctx* ctx, mocha_comm_info_t* out);

/* Pose normalisation of the demo fused into the path: the four norm.npz
 * arrays of the reference (test_fullframework.py:64-71), HOST fp32, (V+1)*C_in each with the root bone
 * first.  Afterwards the *_raw entry points take un-normalised poses WITH the root bone,
 * X_raw (B,T,V+1,C_in), apply X = (X[:,:,1:] - X_mean[:,:,1:]) / X_std[:,:,1:] on load
 * (test_fullframework.py:186,269) and return Y * Y_std[0,:,1:] + Y_mean[0,:,1:] (test_fullframework.py:303,457). */
int mocha_set_pose_norm(mocha_ctx* ctx, const float* x_mean, const float* x_std, const float* y_mean, const float* y_std);
int mocha_encode_raw(mocha_ctx* ctx, const float* X_raw, int B, float* encoded, float* cnt,
                     const float* cnt_mean, const float* cnt_std, float* cnt_nm, void* stream);
int mocha_characterize_raw(mocha_ctx* ctx, const float* src_X_raw, int B, const float* cnt_mean, const float* cnt_std,
                           float* Y_denorm, int32_t* idx, void* stream);

/* The demo pair in one pass: the character clip (B_cha windows) becomes the bank, the B_src source windows are characterized
 * against it — mocha_encode(cha) + mocha_bank_set + mocha_characterize(src) with both clips sharing every launch of
 * mot_embedding / encoder / cnt (test_fullframework.py:188-194, 271-277 for the two clips; :293-296, 438-443, 465-467).
 * The bank is transient (it lives in the workspace during the call); the context's own bank is left untouched.  Optional
 * outputs cha_encoded / cha_cnt_nm (B_cha,90,256) receive the bank for later mocha_bank_set; idx (B_src) the matches.
 * B_src + B_cha must fit the workspace limit (default 1280 windows, mocha_reserve).  *_raw: as mocha_characterize_raw. */
int mocha_characterize_pair(mocha_ctx* ctx, const float* src_X, int B_src, const float* cha_X, int B_cha, const float* cnt_mean,
                            const float* cnt_std, float* Y, int32_t* idx, float* cha_encoded, float* cha_cnt_nm, void* stream);
int mocha_characterize_pair_raw(mocha_ctx* ctx, const float* src_X_raw, int B_src, const float* cha_X_raw, int B_cha,
                                const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx, float* cha_encoded,
                                float* cha_cnt_nm, void* stream);

/* Coherent context matching for clips: a jump-penalised path through the distance matrix instead of one arg-min per window.  The
 * reference's 'cm_' branch takes the nearest bank entry per frame and carries nothing from one frame to the next
 * (test_fullframework.py:440-443).  Its banks are stride-1 windows of smooth clips (collect_CVAE_feature_action.py:119-125), so the right
 * answer for consecutive source windows is almost always a run of consecutive bank rows; the independent arg-min leaves that run whenever
 * noise makes a far entry marginally nearer.  An extension the reference does not have; it needs nothing trained and changes no other call.
 * Definition.  d (Q x N) fp32: the Euclidean distance between z-scored query window i and bank row j, the direct-form sum of the library's
 * matchers (sqrtf of the fp32 squared distance).  Sequence starts 0 = s_0 < s_1 < ... < Q: windows of different sequences are independent.
 * Bank starts b in [0, N): a row j with j = 0 or j in b has no predecessor (the range_starts every bank file carries).  A jump penalty
 * lambda, finite and >= 0, in the units of d.  In float64 on the fp32 values of d, with the relative cost R re-based every step:
 *   first window of a sequence:  R[i][j] = d[i][j]
 *   otherwise:                   a = R[i-1][j-1] - M[i-1] if row j has a predecessor, else +inf;  cont(i, j) = (a < lambda), strict: a tie
 *                                jumps;  R[i][j] = d[i][j] + (cont ? a : lambda)
 *   M[i] = min_j R[i][j], m[i] the lowest j attaining it.
 *   backtrack per sequence:      path[last] = m[last];  path[i] = path[i+1] - 1 if cont(i+1, path[i+1]), else m[i].
 * This is the minimum over all row sequences of sum d[i][j_i] + lambda * (transitions that are not "next row of the same clip"), with the
 * tie rules fixed.  lambda = 0: nothing continues, R[i] = d[i], path[i] is the lowest-index arg-min of row i - the hard match.  Every step
 * is one float64 subtraction, one exact minimum and one float64 addition, so the device gives the sequential evaluation's path to the bit.
 *   mocha_match_dist_matrix : dist[i * ld + j] for Q queries (Q, 90*256; DEVICE) against rows [row0, row0 + rows) of the current bank's
 *                             fp32 rows (also when the bank keeps a bf16 copy), ld >= rows.  Entry (i, j) is bit for bit the distance
 *                             mocha_match_topk reports for (query i, row row0 + j) on an fp32 bank.  Only takes a row range: works on a
 *                             plain, a segmented and a resident bank.  Nothing outside [0, Q) x [0, rows) of dist is written.  The
 *                             all-keys scan behind mocha_match_topk with every group of 8 queries in one launch (ceil(Q / 8) passes over
 *                             the rows), then one launch that turns keys into distances; 8 bytes of context scratch per entry.
 *   mocha_match_path        : a pure function of a DEVICE matrix dist (Q x N, leading dimension ld); needs no bank.  seq_start (HOST,
 *                             n_seq + 1 int32) and bank_start (HOST, n_b int32, sorted; NULL / 0: only row 0 starts a clip) are uploaded
 *                             by the call.  Outputs (DEVICE): path (Q) int32; dist_out (Q) fp32 = dist[i][path[i]] or NULL; continued (Q)
 *                             uint8 or NULL: 1 where path[i] == path[i-1] + 1, that row has a predecessor and i is not a sequence start.
 *                             One workgroup per sequence: SEQUENTIAL in the sequence's length, one workgroup barrier per window, then a
 *                             backtrack launch with one dependent read per window.  N <= 16 384.
 *   mocha_characterize_path : mocha_characterize (raw != 0: mocha_characterize_raw) with the path over the whole bank in the matcher's
 *                             place: encode, z-score, matrix, path, then the decoder and to_mot on the path's rows.  idx (B) the path or
 *                             NULL; continued (B) or NULL.  A batch of more than one workspace chunk encodes twice (the path spans chunks).
 *                             lambda = 0 gives mocha_characterize's indices on tie-free data (ties: the lowest row) and its Y.
 *                             relative != 0: the penalty is lambda x the median over the B windows of their nearest distance (the lower
 *                             median of the matrix's row minima, taken from the call's own matrix; the call then waits for the stream).
 *   mocha_characterize_pair_path : mocha_characterize_pair[_raw] likewise, against the transient bank (bank starts index the B_cha rows).
 * Scratch (the scan's keys, the matrix of the characterize forms, m, the continuation bits - 2 KB per window -, the uploaded lists) is the context's own and
 * grows on first use; it does not move mocha_generation, so captured steps keep replaying.  These are BATCH calls: they allocate and copy
 * from host memory and are NOT capture-safe.  The scratch is one set per context whatever the stream: two of these calls on different
 * streams of one context must be ordered by the caller (as a context is driven from one stream at a time everywhere else).
 * Refusals, nothing launched: MOCHA_ERR_ARG for a NULL context or required pointer, Q < 0 (Q = 0 returns 0), rows < 1 or a range outside
 * the bank, ld < rows, lambda negative, NaN or infinite, starts that are unsorted or out of range, seq_start[0] != 0 or a last entry
 * != Q, more than 16 384 rows; MOCHA_ERR_STATE without a bank, and for mocha_characterize_path on a resident bank.
 * What it is not: no "stay" or "skip" transitions (time warping), one constant penalty.  These calls have no online form; the live one is
 * "coherent matching in live sessions" below. */
#define MOCHA_PATH_MAX_ROWS 16384
int mocha_match_dist_matrix(mocha_ctx* ctx, const float* query_nm, int Q, int64_t row0, int64_t rows, float* dist, int64_t ld, void* stream);
int mocha_match_path(mocha_ctx* ctx, const float* dist, int Q, int N, int64_t ld, const int32_t* seq_start, int n_seq,
                     const int32_t* bank_start, int n_b, double lambda, int32_t* path, float* dist_out, unsigned char* continued,
                     void* stream);
int mocha_characterize_path(mocha_ctx* ctx, const float* src_X, int B, const float* cnt_mean, const float* cnt_std, const int32_t* seq_start,
                            int n_seq, const int32_t* bank_start, int n_b, double lambda, int relative, float* Y, int32_t* idx,
                            unsigned char* continued, int raw, void* stream);
int mocha_characterize_pair_path(mocha_ctx* ctx, const float* src_X, int B_src, const float* cha_X, int B_cha, const float* cnt_mean,
                                 const float* cnt_std, const int32_t* seq_start, int n_seq, const int32_t* bank_start, int n_b,
                                 double lambda, int relative, float* Y, int32_t* idx, unsigned char* continued, float* cha_encoded,
                                 float* cha_cnt_nm, int raw, void* stream);

/* Coherent matching in live sessions: one step of the path per pushed frame, state on the device.  The forward recursion above is an
 * online algorithm with bounded state: R is re-based every step and path[last] = m[last], so the row the forward pass holds after window t
 * is, to the bit, the last row of mocha_match_path over windows 0..t.  A step needs the previous R (one float64 per row of the stream's
 * character), M and m.  The emitted row is this FILTERED row m[t] (no lookahead); it may differ from the whole-clip path's row t.
 * State, per stream, in caller-owned device memory (private layout, mocha_path_state_bytes): `running`, the previous character id, the
 * previous extent (first row, rows) and the slot epoch; the previously emitted row m_prev and M; two buffers of state_rows float64
 * switched by a parity word (64 bytes + 16 bytes per row per stream; 8-byte aligned).  A zeroed buffer is a reset state.
 * d[j]: the fp32 distance between the stream's z-scored query and row j of its character, bit for bit the entry mocha_match_dist_matrix
 * gives for that row; the fp32 rows are read whatever the bank's flags, as the matrix does.  lambda: finite, >= 0, in the units of d, by
 * value (part of a captured step's key).  One step of stream s with effective id e:
 *   e invalid (warming, no frame, id < 0 or outside the table, empty or retired slot): idx = -1, dist = +inf, continued = 0, running = 0;
 *            the decoder reads global row 0 (as mocha_match_segmented); the stream's R is not touched.
 *   restart  if !running, e != the previous id, the extent or the epoch changed, or restart[s] != 0:  R[j] = d[j].  restart: optional
 *            DEVICE int32 per stream, one-shot - the step clears the words it consumed (a stream that sits out consumes nothing).
 *   otherwise a = R_prev[j-1] - M_prev if row j has a predecessor, else +inf;  cont = (a < lambda), strict: a tie jumps;
 *            R[j] = d[j] + (cont ? a : lambda).
 *   M = min_j R[j], m its lowest column.  idx = m (local row); dist = d[m]; continued = 1 iff not a restart, m == m_prev + 1 and row m has
 *   a predecessor.
 * float64 on the fp32 d: one subtraction, one exact minimum, one addition - the device returns the sequential evaluation's row.
 * lambda = 0: the lowest-index arg-min of d, the hard match on an fp32 bank.
 * Row j has a predecessor iff j > 0 and j is not a bank start; row 0 of every character never has one.
 * Bank starts: one bit per global bank row and one epoch word per segment / slot, device data that exists, zeroed, from
 * mocha_bank_set_segments / mocha_bank_resident_create on (its pointer fixed for the bank's life).
 *   mocha_bank_set_starts          : starts (HOST, global rows, strictly increasing) of a segmented bank replace the table's bits.
 *   mocha_bank_resident_set_starts : starts (HOST, local rows of `slot`, strictly increasing) replace the bits of that character.
 *   Both only enqueue on `stream`, move no generation and re-capture nothing.  mocha_bank_resident_add / _retire clear the slot's bits
 *   and bump its epoch on the caller's stream, so a stream on a replaced character restarts even at the same extent.
 *   Refusals: MOCHA_ERR_ARG for unsorted starts or starts out of range; MOCHA_ERR_STATE without such a bank or for an empty slot.
 *   mocha_path_state_bytes   : bytes of a state for `streams` (1..16) streams of up to state_rows (1..MOCHA_PATH_MAX_ROWS) rows; < 0: refused.
 *   mocha_path_state_reset   : the streams named in `which` (HOST array of n stream ids; NULL: all) stop running: their next valid step
 *                              restarts.  Only enqueues memsets: graph-safe, like mocha_live_reset.
 *   mocha_match_path_advance : the pure form, needs no bank: one step on DEVICE rows dist (streams, ld) of distances.  ids (streams): < 0
 *                              sits out, a change restarts; rows (streams): the row count of each stream (outside 1..min(state_rows, ld):
 *                              sits out); start_bits (or NULL) a DEVICE table of n_bits bits, row j of stream s starts a clip iff bit
 *                              bit_off[s] + j (bit_off NULL: j) is set, bits outside the table read 0; restart as above (or NULL).
 *                              Outputs (DEVICE, per stream): idx int32; dist_out fp32 or NULL; continued uint8 or NULL.
 *   mocha_match_path_segmented : one step for z-scored queries (streams, 90*256) with ids seg (streams) against the current segmented or
 *                              resident bank: the plan, the all-keys scan of the fp32 rows (the soft matcher's, through its key buffer)
 *                              and the step kernel.  Capture-safe: no allocation, no host copy, no synchronisation.  dist_row (streams,
 *                              ld >= state_rows) or NULL: every d[j] of the step, for tests and tools.
 *   mocha_characterize_segmented_path : mocha_characterize_segmented with that matcher; B = the state's streams, 1..16 (window s is stream
 *                              s).  The decoder reads the matched row through the bank's per-entry constants, as the hard call does.
 *   mocha_live_step_path, mocha_live_step_raw_path : mocha_live_step / mocha_live_step_raw (hard matcher, no inertializer) with that
 *                              matcher, captured into graphs of their own, plus dist (streams) fp32 and continued (streams) uint8.
 *                              mocha_live_reset of a stream makes it warm up, so it sits out and then restarts.
 * Refusals, nothing launched: MOCHA_ERR_ARG for a NULL context or required pointer, streams outside 1..16, lambda negative, NaN or
 * infinite, state_rows < 1 or > MOCHA_PATH_MAX_ROWS, ld too small; MOCHA_ERR_STATE when the bank's largest character (for a resident bank
 * its reserved maximum) exceeds state_rows, without a bank or without a segment table.
 * What it is not: no fixed-lag smoothing (the emitted row is the filtered one); no "stay" or "skip" transitions; one penalty per call; not
 * combined with the soft, action-constrained, mix, inertialized or Ours steps; no streamed form; fp32 rows are read also on bf16 banks. */
int mocha_bank_set_starts(mocha_ctx* ctx, const int64_t* starts, int n, void* stream);
int mocha_bank_resident_set_starts(mocha_ctx* ctx, int slot, const int32_t* starts, int n, void* stream);
int64_t mocha_path_state_bytes(const mocha_ctx* ctx, int streams, int state_rows);
int mocha_path_state_reset(mocha_ctx* ctx, void* state, int streams, int state_rows, const int32_t* which, int n, void* stream);
int mocha_match_path_advance(mocha_ctx* ctx, void* state, int streams, int state_rows, const float* dist, int64_t ld, const int32_t* ids,
                             const int32_t* rows, const uint32_t* start_bits, int64_t n_bits, const int32_t* bit_off, int32_t* restart,
                             double lambda, int32_t* idx, float* dist_out, unsigned char* continued, void* stream);
int mocha_match_path_segmented(mocha_ctx* ctx, void* state, int streams, int state_rows, const float* query_nm, const int32_t* seg,
                               int32_t* restart, double lambda, int32_t* idx, float* dist, unsigned char* continued, float* dist_row, int64_t ld,
                               void* stream);
int mocha_characterize_segmented_path(mocha_ctx* ctx, const float* src_X, int B, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                                      void* path_state, int state_rows, double lambda, int32_t* restart, float* Y, int32_t* idx, float* dist,
                                      unsigned char* continued, int raw, void* stream);
/* (mocha_live_step_path and mocha_live_step_raw_path are declared with the live steps, below) */

/* CVAE character-feature sampler: CVAE.sample(c) of model_CVAE.py:44-46, i.e.
 * PriorNet (:49-92) then Decoder (:138-165).  Weights by their reference state_dict names
 * ("prior_net.encoder.layers.0.self_attn.in_proj_weight", ...; test_fullframework.py:52-58); the
 * posterior "encoder.*" entries and the pos_encoder.pe buffers of a checkpoint are accepted and ignored.
 * cond (B,180,256) -> out (B,90,256).  eps (B,256) is the reparameterisation noise
 * z = mu + eps*exp(0.5*logvar) (:81-87); eps == NULL is deterministic=True (z = mu).  mu/logvar (B,256) optional. */
int mocha_cvae_load_weight(mocha_ctx* ctx, const char* name, const float* host, const int64_t* shape, int ndim);
int mocha_cvae_finalize(mocha_ctx* ctx);
int mocha_cvae_sample(mocha_ctx* ctx, const float* cond, int B, float* out, float* mu, float* logvar, const float* eps, void* stream);

/* Conditioning glue of the demo's CVAE ("Ours") branch, test_fullframework.py:446-449, all (.., 90, 256):
 *   cond (B,180,256) = cat[(src_cnt - src_mean)/src_std , (prev_cha - cha_mean)/cha_std]  (token axis)
 *   out = x * std + mean                       (curr_cha_encoded = vae_output * cha_encoded_std + cha_encoded_mean) */
int mocha_cvae_condition(mocha_ctx* ctx, const float* src_cnt, const float* src_mean, const float* src_std, const float* prev_cha,
                         const float* cha_mean, const float* cha_std, int B, float* cond, void* stream);
int mocha_scale_shift(mocha_ctx* ctx, const float* x, const float* mean, const float* std_, int B, float* out, void* stream);

/* Window featurisation of the demo (test_fullframework.py:141-185): local bone features
 * of B windows — Yrot (B,T,V+1,4) quaternions (w,x,y,z), Ypos / Yvel / Yang (B,T,V+1,3), root bone first, as
 * process_data produces them (:126-139) — to the un-normalised features X_raw (B,T,V+1,15) that the *_raw
 * entry points consume: FK with velocities, re-rooting on each window's last frame, root-relative
 * position | rotation-matrix xy | velocity | angular velocity. */
int mocha_featurize(mocha_ctx* ctx, const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, int B,
                    float* X_raw, void* stream);

/* Post-processing of decoded windows.
 * mocha_pose_heads: Y (B,60,V,15) de-normalised -> heads (B,V,13) = [pos 3 | quat wxyz 4 | vel 3 | ang 3] of the last
 *   frame (test_fullframework.py:304-308: slices + quat.from_xform_xy) and speed (B) = mean_t |Y[t,0,9:12]| (:338).
 * mocha_postprocess: the sequential frame loop of the demo for n_clips independent clips of n_frames windows each
 *   (:338-437 first frame, :492-632 after it): root integration from the source's root-local velocities, position
 *   blending, foot-lock state machine (motion/Inertialization.py:300-377) and two-bone IK (motion/quat.py:295-343);
 *   optionally the root merge + Euler channels of the BVH writer (:677-681, 697).  State is float64 as in the
 *   reference.  heads (clips,frames,V,13), speed/src_speed (clips,frames), src_rvel/src_rang (clips,frames,3),
 *   contact (clips,frames,n_contact) uint8 -> pos (clips,frames,V+1,3), rot / ik_rot (clips,frames,V+1,4) wxyz,
 *   bvh_pos / bvh_euler (clips,frames,V,3; degrees; both NULL to skip).  cfg NULL = the demo's constants (:104-114). */
typedef struct mocha_post_cfg {
    double dt, ik_max_length_buffer, ik_foot_height, ik_unlock_radius, ik_blending_halflife;
    int ik_enabled, n_contact;
    int contact_bones[4];      /* toe bones, indices in the (V+1)-bone skeleton with the root bone in front */
    int blend_enabled;         /* 1 (default): positions blended with the previous frame's (:537, 627).  0 together with
                                * ik_enabled = 0 is the demo's context-matching "cm_" stream: decoded poses as they are, only
                                * the root integrated (test_fullframework.py:512-527, 637-641) */
} mocha_post_cfg;
void mocha_post_cfg_default(mocha_post_cfg* cfg);
int mocha_pose_heads(mocha_ctx* ctx, const float* Y, int B, float* heads, float* speed, void* stream);
int mocha_postprocess(mocha_ctx* ctx, const mocha_post_cfg* cfg, const float* heads, const float* speed, const float* src_rvel,
                      const float* src_rang, const float* src_speed, const unsigned char* contact, int n_clips, int n_frames,
                      double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, void* stream);

/* Resumable post-processing: ONE frame per clip and call, the loop's state in caller-owned device memory (the reference keeps it in
 * Python objects across the iterations of its frame loop, test_fullframework.py:338-437 for the first frame, :492-632 after it, and
 * :677-681 for the BVH channels - this call is one iteration of that loop).
 *   mocha_post_state_bytes : bytes of state per clip (private layout, float64; the same for every configuration of a context).
 *                            Host-side, no synchronisation.
 *   mocha_postprocess_step : heads (n_clips,V,13), speed / src_speed (n_clips), src_rvel / src_rang (n_clips,3), contact
 *                            (n_clips,n_contact) uint8 of the CURRENT frame -> pos (n_clips,V+1,3), rot / ik_rot (n_clips,V+1,4),
 *                            bvh_pos / bvh_euler (n_clips,V,3; both or neither) of that frame, and the state advanced by one frame.
 *                            state: n_clips * mocha_post_state_bytes device bytes.  ALL-ZERO BYTES MEAN "no frame seen yet": the next
 *                            call takes the first-frame branch (root from identity, contact reset from the toe's global position and
 *                            velocity, no blending, ik_rot = rot).  So a reset is a hipMemsetAsync of a clip's bytes and a snapshot /
 *                            rollback is a device copy.  The frame counter lives in the state, not in an argument: the call may be
 *                            captured into a HIP graph once and replayed for every frame, the first included.  The kernels are
 *                            mocha_postprocess's own, run on one frame with the state loaded and stored around it: stepping a clip
 *                            frame by frame from a zeroed state gives the bits of mocha_postprocess on the whole clip.  cfg as for mocha_postprocess, and
 *                            the same cfg must be passed for every frame of a clip.  n_clips == 0 is a no-op; a NULL required pointer
 *                            is MOCHA_ERR_ARG, never a launch.  No allocation, no synchronisation. */
int64_t mocha_post_state_bytes(const mocha_ctx* ctx);
int mocha_postprocess_step(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* state, const float* heads, const float* speed,
                           const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact, int n_clips,
                           double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, void* stream);

/* Live sessions: one mocap frame in, one characterized, root-integrated, foot-locked pose out, for 1..16 streams at once, every
 * stream against its own character of a multi-character bank.  The reference builds every 60-frame window from the whole loaded clip
 * (test_fullframework.py:126-186) and runs its frame loop over all windows afterwards (:338-437, 492-632, 677-681); here the window is
 * a device-resident ring per stream and the frame loop advances one iteration per call.
 *   mocha_live_state_bytes : bytes of the session buffer `live` for `streams` streams (caller-owned device memory, private layout: per
 *                            stream the ring of the last 60 frames of local bone data, its head / fill counters, the state of
 *                            mocha_postprocess_step, and the step's staging - X_raw, Y, heads, speed, effective ids).  Host-side.
 *   mocha_live_reset       : zeroes the ring counters and the post state of the streams named in `which` (HOST array of n stream ids;
 *                            NULL = all streams): they warm up again and their next valid frame takes the first-frame branch.
 *                            Enqueued on `stream`, graph-safe, no synchronisation.  A freshly zeroed buffer is a reset session.
 *   mocha_live_step        : pushes the NEW frame of every stream - Yrot (S,V+1,4) quaternions (w,x,y,z), Ypos / Yvel / Yang (S,V+1,3),
 *                            root bone first, the per-frame slices of what mocha_featurize takes - into its ring, featurises the window
 *                            "oldest ring frame ... newest ring frame" re-rooted on the newest one (bit-identical to mocha_featurize on
 *                            the materialised window), runs the segmented characterize of the S windows (mocha_step_graph_segmented's
 *                            kernels, raw = 1), mocha_pose_heads and one frame of mocha_postprocess_step with src_rvel / src_rang
 *                            (S,3), src_speed (S), contact (S,n_contact) of that frame.  seg (S) device: the character of each stream.
 *                            A stream whose ring holds fewer than 60 frames is WARMING: valid[s] = 0, idx[s] = -1 (it is matched against
 *                            no bank row), its post state is not advanced and its rows of pos / rot / ik_rot / bvh_* are left untouched;
 *                            its 60th push gives valid[s] = 1 and its first frame.  Otherwise idx[s] is the matched row local to the
 *                            character's segment.  The whole step is captured into a HIP graph on first use and replayed, keyed on every
 *                            pointer argument, `streams`, the contents of cfg (NULL = the demo's constants) and the generation: new ids
 *                            in seg, new frame data, resets and the warming -> running transition are device data and do not re-capture;
 *                            a new bank does.  While mocha_profile_start is active the step runs eagerly instead, launch by launch.
 *                            Needs mocha_set_pose_norm and a segment table (mocha_bank_set_segments; one segment serves a single
 *                            character), else MOCHA_ERR_STATE; streams outside 1..16 or a NULL required pointer (bvh_pos / bvh_euler:
 *                            both or neither) is MOCHA_ERR_ARG, and nothing is launched.  Uses workspace set 0 like the other graph
 *                            steps: one stream at a time per context. */
int64_t mocha_live_state_bytes(const mocha_ctx* ctx, int streams);
int mocha_live_reset(mocha_ctx* ctx, void* live, int streams, const int32_t* which, int n, void* stream);
int mocha_live_step(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                    const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                    const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, double* pos,
                    double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, void* stream);
/* mocha_live_step with the soft characterize (see "Soft context matching on a multi-character bank" above). */
int mocha_live_step_soft(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                         const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                         const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k, float temperature,
                         double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid,
                         int32_t* idx_k, float* w_k, void* stream);

/* Inertialized character switches.  A live stream may name another character on any frame; the decoder then reads a row of another
 * segment and mocha_pose_heads hands the post-processing frame a pose that has nothing to do with the previous one.  The reference holds
 * the remedy and never calls it: the per-bone inertializers of motion/Inertialization.py:71-91 (springs :10-37).  Here they run on the
 * pose heads, per stream and per non-root bone j = 0..V-1, on all 13 channels of a head row [pos 3 | quat wxyz 4 | vel 3 | ang 3] (fp32, as
 * mocha_pose_heads writes it).  The ROOT bone is not inertialized: the frame loop integrates it from its own previous output
 * (test_fullframework.py:500-503), so it is continuous by construction.
 *   mocha_inert_cfg        : halflife (seconds) and dt (seconds per frame).  NULL = {0.1, 1/60}.  halflife < 0, dt <= 0 or a non-finite
 *                            value is MOCHA_ERR_ARG; halflife == 0 is legal (the reference adds 1e-5).
 *   mocha_inert_state_bytes: bytes of state per stream (private layout, float64).  Host-side, no synchronisation.  The state holds the
 *                            flags `seen` and `active`, `last_id`, `prev_in` (the stream's previous valid input heads, before offsets)
 *                            and the offsets off_pos, off_vel, off_ang (3 each) and off_rot (a quaternion).  ALL-ZERO BYTES ARE A RESET
 *                            STREAM: a reset is a hipMemsetAsync, a snapshot / rollback a device copy, as for mocha_post_state_bytes.
 *   mocha_inertialize_step : ONE frame of n independent streams, heads_in (n,V,13) -> heads_out (n,V,13), which may be the same buffer;
 *                            state: n * mocha_inert_state_bytes device bytes; ids / trigger / valid (n) int32 device, each may be NULL
 *                            (valid NULL: every stream is valid).  Per stream, from device data alone:
 *                              not valid  - valid[s] == 0 (the stream is warming): its heads are untouched, its state is cleared
 *                                           (seen = active = 0, offsets at rest).  A stream reset with mocha_live_reset warms for 59
 *                                           frames, so it needs no reset call of its own.
 *                              first      - seen == 0: prev_in = in, last_id = id, seen = 1; the output is the input, bit for bit.
 *                              transition - seen, and ids given with ids[s] != last_id, or trigger given with trigger[s] != 0:
 *                                           off_pos, off_vel = inertialize_transition_pos(off_pos, off_vel, prev_in.pos, prev_in.vel,
 *                                           in.pos, in.vel) (:71-74); off_rot, off_ang = inertialize_transition_rot(off_rot, off_ang,
 *                                           prev_in.rot, prev_in.ang, in.rot, in.ang) (:82-85, with quat.abs: w > 0.0, negated
 *                                           otherwise); active = 1; then the update below IN THE SAME FRAME (pose_transition followed
 *                                           by pose_update).  "src" is the stream's previous valid frame, not an extrapolation of it
 *                                           to the switch frame: the function as the reference wrote it.
 *                              update     - active: out.pos, out.vel, off_pos, off_vel = inertialize_update_pos(off_pos, off_vel,
 *                                           in.pos, in.vel, halflife, dt) (:76-80, :18-26, :10-14: fast_negexpf is the rational
 *                                           function as written, halflife_to_damping uses eps = 1e-5); out.rot, out.ang, off_rot,
 *                                           off_ang = inertialize_update_rot(...) (:87-91, :28-37; quat.log and quat.exp keep their
 *                                           eps = 1e-5 branches; out.rot = off_rot (x) in.rot is not renormalised, as in the reference).
 *                              not active - seen and no transition since the reset: the output is the input bit for bit (the words
 *                                           are copied, no arithmetic: in + 0.0 would turn -0.0 into +0.0).
 *                              always, for a valid frame: prev_in = in (the input, not the output), last_id = id.
 *                            float64 arithmetic on the fp32 inputs, outputs rounded to fp32 once, offsets float64 across frames.
 *                            n == 0 is a no-op; a NULL required pointer or a bad cfg is MOCHA_ERR_ARG, never a launch.  One launch
 *                            (mocha_inertialize, one 64-lane workgroup per stream), no allocation, no synchronisation: capture-safe.
 *   mocha_live_step_inert  : the arguments of mocha_live_step_soft, then `inert` (streams * mocha_inert_state_bytes device bytes, the
 *                            caller's, zeroed = reset) and icfg.  k == 0 is the hard route of mocha_live_step (idx_k / w_k may be NULL),
 *                            k >= 1 the soft route.  The step is mocha_live_step's with ONE launch between mocha_pose_heads and the
 *                            post-processing frame: mocha_inertialize in place on the session's staged heads, ids = the step's
 *                            effective ids, valid = the step's valid.  A stream that never switches gets the bits of mocha_live_step /
 *                            _soft; mocha_live_state_bytes and the layout of `live` are unchanged.  Captured into its own HIP graph,
 *                            keyed as the live step's plus `inert` and the two doubles of icfg: a new id is device data and does not
 *                            capture again.  While mocha_profile_start is active the step runs eagerly, the launch named
 *                            mocha_inertialize, site live.inert.  Refusals as mocha_live_step / _soft; a NULL `inert` or a bad icfg is
 *                            MOCHA_ERR_ARG.  Nothing is launched on a refusal. */
typedef struct mocha_inert_cfg { double halflife, dt; } mocha_inert_cfg;
int64_t mocha_inert_state_bytes(const mocha_ctx* ctx);
int mocha_inertialize_step(mocha_ctx* ctx, const mocha_inert_cfg* cfg, void* state, const float* heads_in, float* heads_out,
                           const int32_t* ids, const int32_t* trigger, const int32_t* valid, int n, void* stream);
int mocha_live_step_inert(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                          const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                          const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                          float temperature, double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                          int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert, const mocha_inert_cfg* icfg);

/* The CVAE ("Ours") branch inside the live step (test_fullframework.py:446-457; a stream's first frame is :290-298): mocha_live_step
 * with the decoder's character feature sampled from the previous one instead of taken from the matched bank row.  The autoregressive
 * state of every stream lives in a second caller-owned device buffer `ours`, every decision of a frame is device data, and the noise can
 * be drawn on the device, so the step is ONE captured graph for 1..16 streams and needs no host arithmetic.
 *   mocha_live_ours_state_bytes : bytes of `ours` for `streams` streams (S below).  ALL-ZERO BYTES ARE A RESET BUFFER.  Sections in this
 *                            order, each starting on a 256-byte boundary:
 *                              counters (S,3) int32  {chain: steps since the stream's seed frame, last: the character id of its last
 *                                                     step, mode: what its latest step was - 0 warming, 1 seed, 2 chain}
 *                              prev    (S,90,256)    the stream's character feature: what the decoder of the latest step read
 *                              cnt     (S,90,256)    staging: the instance-normalised source feature of the step
 *                              cond    (S,180,256)   staging: the sampler's condition
 *                              vae     (S,90,256)    staging: the sampler's output
 *                              eps, mu, logvar (S,256 each)  staging: the noise used, the prior's mean and log-variance
 *                            The session buffer `live` of mocha_live_step is used as it is (same layout, same size).
 *   mocha_live_ours_reset  : mocha_live_reset plus zeroed counters of the named streams in `ours`: their next valid frame is a seed
 *                            frame.  Enqueued on `stream`, graph-safe.
 *   mocha_live_step_ours   : the arguments of mocha_live_step, plus `ours`, the CVAE's statistics and noise source, and seeded (S).
 *                            Per stream, from device data alone:
 *                              warming - the ring holds fewer than 60 frames (valid[s] = 0): the stream's counters and `prev` are not
 *                                        written and its `cond` rows are zeros, seeded[s] = 0, outputs untouched as in mocha_live_step
 *                                        (the staging sections cnt, vae, eps, mu, logvar are rewritten for EVERY stream on every step:
 *                                        the instance norm and the sampler run on the whole batch);
 *                              seed    - the stream's chain counter is 0 (first valid frame after a reset) or its character id differs
 *                                        from the one of its last step: the character feature is the matched bank row, i.e. the frame is
 *                                        mocha_live_step's frame; seeded[s] = 1.  The sampler still runs for the batch; the stream's
 *                                        sample is discarded;
 *                              chain   - cond = cat[(cnt - src_cnt_mean)/src_cnt_std, (prev - cha_encoded_mean)/cha_encoded_std],
 *                                        vae = CVAE.sample(cond), prev = vae * cha_encoded_std + cha_encoded_mean, decoder(encoded,
 *                                        prev); seeded[s] = 0.
 *                            idx[s] is the matched row of every valid frame (the reference searches on every frame).
 *                            noise 0: z = mu.  noise 1: eps (S,256) device, read on every step.  noise 2: drawn on the device with
 *                            Philox4x32-10, key = (low, high) 32-bit words of `seed`, counter = (j, chain counter of the stream, s, 0)
 *                            for j = 0..63; the block's words x0..x3 give u_k = ((x_k >> 8) + 0.5) * 2^-24, every operation in fp32
 *                            and rounded to nearest even (from 2^23 on the sum rounds to an integer: u_k lies in (0,1]), and, by Box-Muller,
 *                            eps[4j] = r cos(2 pi u1), eps[4j+1] = r sin(2 pi u1), r = sqrt(-2 log u0); eps[4j+2], eps[4j+3] likewise
 *                            from u2, u3.  A stream's noise depends on (seed, s, chain counter) alone: a replayed session repeats it.
 *                            ONE CVAE PER CONTEXT: its weights (mocha_cvae_load_weight / mocha_cvae_finalize ON THIS context, else
 *                            MOCHA_ERR_STATE) and the four statistics serve every stream - the reference trains one CVAE per target
 *                            character.  Streams may still name different segments; a seed row comes from the stream's own segment.
 *                            (One CVAE per CHARACTER, from a resident weight bank: mocha_live_step_ours_grouped below.)
 *                            Captured into its own HIP graph, keyed as mocha_live_step's plus `ours`, the pointers in ocfg, noise, seed
 *                            and seeded.  Other refusals as mocha_live_step; a NULL `ours`, ocfg or statistic, noise outside 0..2, or
 *                            noise 1 without eps is MOCHA_ERR_ARG, as are more streams than the workspace limit (mocha_reserve): the
 *                            branch runs its stages on all the streams in one piece.  Nothing is launched on a refusal. */
typedef struct mocha_ours_cfg {
    const float *src_cnt_mean, *src_cnt_std, *cha_encoded_mean, *cha_encoded_std;    /* device, (90,256) each */
    int noise;                 /* 0 none (z = mu), 1 eps given by the caller, 2 drawn on the device from seed */
    const float* eps;          /* device (S,256); noise 1 only */
    uint64_t seed;             /* noise 2 only */
} mocha_ours_cfg;
int64_t mocha_live_ours_state_bytes(const mocha_ctx* ctx, int streams);
int mocha_live_ours_reset(mocha_ctx* ctx, void* live, void* ours, int streams, const int32_t* which, int n, void* stream);
int mocha_live_step_ours(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                         const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                         const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, void* ours,
                         const mocha_ours_cfg* ocfg, double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler,
                         int32_t* idx, int32_t* valid, int32_t* seeded, void* stream);

/* One CVAE per character: a resident WEIGHT BANK of max_cvaes slots, each a whole CVAE (every tensor mocha_cvae_load_weight expects) with its
 * four statistics, one positional table for the bank, and a device word per slot that says whether the slot holds weights.  Which slot a
 * row of a sampler batch - or a stream of the live step - uses is DEVICE data, read by every launch: a captured step follows it.
 *   mocha_cvae_bank_create : allocates the bank, zero-filled: (max_cvaes, ...) for every sampler tensor (about 10.5 MB per slot), the
 *                            per-slot statistics (max_cvaes, 4, 90, 256) = src_cnt mean / std, cha_encoded mean / std, stored[max_cvaes] and
 *                            the shared sin / cos positional table.  Moves the generation once.  1 <= max_cvaes <= 4096, else MOCHA_ERR_ARG.
 *   mocha_cvae_bank_store  : writes the CVAE currently STAGED ON THE HOST by mocha_cvae_load_weight (mocha_cvae_finalize is not needed) into
 *                            `slot`, with its statistics (host, (90,256) each).  (Staging un-finalises the context's OWN CVAE, as every
 *                            mocha_cvae_load_weight does: mocha_cvae_finalize brings the staged one up as the context's.)  MOCHA_ERR_STATE without a bank or while a weight is missing
 *                            (the message names it).  One positional table per bank: a staged pos_encoder.pe becomes the bank's table when no
 *                            slot is stored; while one is, a staged table that differs from the bank's is MOCHA_ERR_ARG.  The copies
 *                            are enqueued on `stream` from a context-owned pinned buffer; the slot's stored word is written LAST, by a one-lane
 *                            kernel with an ordinary store.  NO generation move and no device-wide synchronisation: a captured grouped
 *                            step replays before and after, and a replay enqueued on the same stream after the store samples with the new
 *                            weights.  The call may wait for the PREVIOUS store's copies (they read the same pinned buffer), nothing else.
 *   mocha_cvae_bank_clear  : enqueues stored[slot] = 0; the weights stay.  Rows and streams on the slot then count as having no CVAE.
 *   mocha_cvae_bank_info   : host only: *capacity = max_cvaes; stored (capacity bytes, or NULL) = 1 / 0 per slot AS THE HOST ENQUEUED THEM.
 *   mocha_cvae_sample_grouped : mocha_cvae_sample with row b on slot which[b] (device, (B) int32).  A row whose slot is outside
 *                            [0, max_cvaes) or not stored reads no weight and gets zeros in out, mu and logvar; the other rows' bits do
 *                            not depend on it, nor on B or on their place in the batch.  MOCHA_ERR_STATE without a weight bank.
 *   mocha_linear_grouped   : the grouped GEMM alone on caller memory (all device), for tests and tooling, as mocha_linear is for the other
 *                            engines: y[g] = act(x[g] w_bank[which[g]]^T + bias_bank[which[g]]) (+ residual[g]) for G groups of m
 *                            consecutive rows; x (G*m, K), w_bank (Cw, N, K), bias_bank (Cw, N) or NULL, which (G) and stored (Cw) int32,
 *                            y (G*m, ldc), residual (G*m, ldr) or NULL; act 0 none / 3 ReLU.  m >= 1, N % 16 == 0, K % 16 == 0, ldc >= N
 *                            (and ldr >= N) multiples of 4, else MOCHA_ERR_ARG.  Exact fp32 (v_mfma_f32_16x16x4_f32); the order of an
 *                            element's sum depends on K alone.  A group with which[g] outside [0, Cw) or stored[which[g]] == 0: zeros.
 *   mocha_live_step_ours_grouped : mocha_live_step_ours's arguments plus cvae_of - device, one int32 per segment (or slot, on a resident
 *                            bank) of the CURRENT character bank: the weight-bank slot of that character's CVAE.  Read by every replay; a
 *                            producer may rewrite it in place.  The statistics pointers of ocfg are ignored and may be NULL: a stream's
 *                            four statistics are those of slot cvae_of[eff[s]].  A stream whose character has NO CVAE - cvae_of negative
 *                            or >= max_cvaes, or the slot not stored - is a SEED stream on every valid frame: its character feature is
 *                            the matched bank row, seeded[s] = 1, the frame is mocha_live_step's frame, its cond rows are zeros.  A
 *                            change of cvae_of[e] between frames does not reseed: `prev` is kept in de-normalised feature units and
 *                            simply meets the new statistics.  Streams without a CVAE and warming streams cost no weight traffic (the
 *                            sampler's stages still run for every stream of the batch).  No constrained seed match.  Its own captured
 *                            graph, keyed as mocha_live_step_ours's plus cvae_of; works on a multi-character bank and on a resident bank
 *                            alike.  Refusals as mocha_live_step_ours; in addition no weight bank is MOCHA_ERR_STATE and a NULL cvae_of
 *                            MOCHA_ERR_ARG.  Nothing is launched on a refusal. */
int mocha_cvae_bank_create(mocha_ctx* ctx, int max_cvaes);
int mocha_cvae_bank_store(mocha_ctx* ctx, int slot, const float* src_cnt_mean, const float* src_cnt_std, const float* cha_encoded_mean,
                          const float* cha_encoded_std /* host, (90,256) each */, void* stream);
int mocha_cvae_bank_clear(mocha_ctx* ctx, int slot, void* stream);
int mocha_cvae_bank_info(const mocha_ctx* ctx, int* capacity, unsigned char* stored);
int mocha_cvae_sample_grouped(mocha_ctx* ctx, const float* cond, int B, const int32_t* which /* device (B) */, float* out, float* mu,
                              float* logvar, const float* eps, void* stream);
int mocha_linear_grouped(mocha_ctx* ctx, const float* x, const float* w_bank, const float* bias_bank, const int32_t* which,
                         const int32_t* stored, float* y, int ldc, int G, int m, int N, int K, int Cw, int act, const float* residual, int ldr,
                         void* stream);
int mocha_live_step_ours_grouped(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                                 const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                                 const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, void* ours,
                                 const mocha_ours_cfg* ocfg, const int32_t* cvae_of, double* pos, double* rot, double* ik_rot, double* bvh_pos,
                                 double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* seeded, void* stream);

/* The mocap front end of a live session: RAW frames in.  What mocha_live_step takes per frame - Yrot / Ypos / Yvel / Yang with a synthetic
 * root bone, src_rvel / src_rang / src_speed, the foot contacts - is what the reference's process_data (preprocess/generate_database.py:
 * 86-177) makes of a whole clip with filters that read frames after the one they produce.  These calls are its streaming form, on the
 * device: a stream pushes ONE raw frame per call - the local rotations and local positions of its V joints, joint 0 the hips, as a mocap
 * device or one line of a BVH file holds them - and, once it has pushed 31 frames (the 31-tap filter refuses a shorter clip), every push
 * emits frame t = n-1-lookahead of process_data applied to the n frames pushed since the stream's reset.
 *   lookahead = 18 (0.3 s): the emitted frame is the whole clip's frame, contacts included (pos / vel / rot / ang already from 16 on).
 *   lookahead = 0: no added latency; the reference's clip-end rules are applied at every frame - the polynomial edge fit of
 *     savgol_filter(mode='interp'), v[-1] = v[-2] + (v[-2] - v[-3]), the 'nearest' padding of the median filter.
 * Per emitted frame: root position = 15-tap cubic fit of the spine joint on xz, root direction = 31-tap cubic fit of the projected
 * across-direction (shoulders + upper legs), renormalised before and after; root rotation = normalize(between(z, direction)); the hips
 * made root-local; velocities and angular velocities by central differences at `fps`; contacts = fk_vel down each toe chain, speed <
 * contact_velocity_threshold, then the 6-frame majority vote ("at least 3 of t-3 .. t+2").  src_rvel / src_rang = inv_mul_vec(Yrot[0],
 * Yvel[0] / Yang[0]) and src_speed = the mean speed of bone 1 over the last 60 emitted frames (test_fullframework.py:142-143, :164-169,
 * :493; 0 until 60 were emitted) are evaluated in float64 on the emitted fp32 values and rounded once: the demo evaluates them in fp32
 * NumPy, so they may sit one fp32 ulp away from its values.  Everything else is float64 on the fp32 inputs, rounded to fp32 once.
 * Inherited from the reference, not fixed: between([0,0,1], d) is singular for a character facing exactly -z; contacts flip at a hard
 * threshold.  A stream never emits the last `lookahead` frames of a clip and does not mirror: whole clips, mirrored or not, go through
 * mocha_ingest_clips below, which emits every frame.  BVH text is read by mocha_bvh_header / mocha_bvh_motion further down.
 *   mocha_ingest_cfg_default : the reference's constants (lookahead 0, Euler degrees in 'zyx' channel order, unit scale 0.01: cm -> m,
 *                            60 frames per second, threshold 0.5 m/s) and the role joints of `layout`: 0 ('mocha': Spine2 = 7, shoulders
 *                            9 / 16, upper legs 1 / 20), 1 ('mixamo' of this library's 22-joint table: 3, 6 / 10, 18 / 14).
 *   mocha_ingest_state_bytes : bytes of the front end's buffer for `streams` streams (caller-owned device memory, private layout: per
 *                            stream the frame counts, the sign state of quat.unroll, a ring of the last 40 raw frames and the last 60
 *                            emitted hips positions; then the staging mocha_live_step_raw hands to the live step).  ALL-ZERO BYTES = no
 *                            frame seen; a snapshot is a copy.
 *   mocha_ingest_reset     : zeroes the rows of the named streams (which NULL: all).  Enqueued on `stream`, graph-safe.
 *   mocha_live_ingest_step : the front end alone.  rot (S,V,4) quaternions w,x,y,z or (S,V,3) Euler degrees in the order of
 *                            cfg->euler_order (rot_format), pos (S,V,3); the toes are post->contact_bones (post NULL: the demo's).
 *                            Outputs Yrot (S,V+1,4), Ypos / Yvel / Yang (S,V+1,3), src_rvel / src_rang (S,3), src_speed (S), contact
 *                            (S,n_contact) uint8, have (S) int32: 1 where the stream emitted a frame.  Rows of a stream with have == 0 are
 *                            left untouched.  One launch (mocha_live_ingest, one 64-lane workgroup per stream), no allocation, no
 *                            synchronisation: capture-safe.
 *   mocha_live_step_raw    : mocha_live_ingest_step into the buffer's staging, then the live step on it, in ONE captured graph.  k == 0:
 *                            the hard step (idx_k / w_k may be NULL), k >= 1: the soft step; inert non-NULL: the inertialized step (icfg
 *                            NULL: its default).  A stream with have == 0 pushes nothing into its window ring: valid[s] = 0, its
 *                            outputs and its post state stay, exactly as for a warming stream - so valid first becomes 1 on push 90.
 *                            Keyed as the step it wraps plus `ingest`, the raw pointers and the CONTENTS of icfg_in; while profiling
 *                            the launch is named mocha_live_ingest, site live.ingest.
 * Refusals (MOCHA_ERR_ARG, nothing launched): a NULL required pointer, lookahead outside 0..18, rot_format outside 0..1, an Euler order
 * that is no permutation of 0..2, a role joint outside 0..V-1, unit_scale / fps / threshold not finite or fps <= 0, a skeleton whose
 * joints do not follow their parents, and what the post cfg refuses. */
typedef struct mocha_ingest_cfg {
    int lookahead;                       /* 0..18 frames */
    int rot_format;                      /* 0: quaternions (w,x,y,z), 1: Euler angles in degrees */
    int euler_order[3];                  /* axis index (0 x, 1 y, 2 z) of channel 0, 1, 2: quat.from_euler's `order` */
    double unit_scale, fps, contact_velocity_threshold;
    int spine, shoulder_l, shoulder_r, upleg_l, upleg_r;      /* raw joint indices */
} mocha_ingest_cfg;
void mocha_ingest_cfg_default(mocha_ingest_cfg* cfg, int layout);
int64_t mocha_ingest_state_bytes(const mocha_ctx* ctx, int streams);
int mocha_ingest_reset(mocha_ctx* ctx, void* ingest, int streams, const int32_t* which, int n, void* stream);
int mocha_live_ingest_step(mocha_ctx* ctx, const mocha_ingest_cfg* cfg, const mocha_post_cfg* post, void* ingest, int streams,
                           const float* rot, const float* pos, float* Yrot, float* Ypos, float* Yvel, float* Yang, float* src_rvel,
                           float* src_rang, float* src_speed, unsigned char* contact, int32_t* have, void* stream);
int mocha_live_step_raw(mocha_ctx* ctx, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                        const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                        float temperature, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler,
                        int32_t* idx, int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert,
                        const mocha_inert_cfg* icfg);
/* The action-constrained live steps (see mocha_bank_set_labels): mocha_live_step_inert's / mocha_live_step_raw's arguments - k == 0 the hard
 * matcher, inert may be NULL - then allow (streams uint64, DEVICE: read by every replay, a producer may write it in place) and applied
 * (streams int32, or NULL). */
int mocha_live_step_allow(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                          const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                          const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                          float temperature, double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                          int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert, const mocha_inert_cfg* icfg,
                          const uint64_t* allow, int32_t* applied);
int mocha_live_step_raw_allow(mocha_ctx* ctx, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                              const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                              float temperature, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler,
                              int32_t* idx, int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert,
                              const mocha_inert_cfg* icfg, const uint64_t* allow, int32_t* applied);

/* The live step with the online path in the hard matcher's place ("coherent matching in live sessions", above): mocha_live_step's /
 * mocha_live_step_raw's arguments (hard matcher, no inertializer), then path_state (mocha_path_state_bytes(ctx, streams, state_rows)),
 * state_rows, lambda, restart (DEVICE, streams int32, or NULL) and the outputs dist (streams) fp32 and continued (streams) uint8. */
int mocha_live_step_path(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                         const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                         const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, double* pos,
                         double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, void* stream,
                         void* path_state, int state_rows, double lambda, int32_t* restart, float* dist, unsigned char* continued);
int mocha_live_step_raw_path(mocha_ctx* ctx, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                             const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                             double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                             int32_t* valid, void* stream, void* path_state, int state_rows, double lambda, int32_t* restart, float* dist,
                             unsigned char* continued);

/* Character mixing on a multi-character bank: a window characterized by up to MOCHA_MIX_MAX (character, six body-part weights) components
 * instead of exactly one character - a strength dial ("70 % zombie, 30 % neutral"), a cross-fade (a weight ramp from a to b over n frames, in
 * feature space) and a splice by body part ("arms of A, legs of B") are ONE operation.  The model's tokens are 15 time patches x 6 body
 * parts, token = t * 6 + v (v in the column order of the layout's pool matrix, mocha_graph_constants); the decoder reads, part by part, the
 * weighted blend of the components' matched entries.  Nothing is trained, as for the soft calls.
 *   Window q carries ids[q][j] (int32) and weights[q][j][v] (fp32), j < J, 1 <= J <= MOCHA_MIX_MAX, v < MOCHA_MIX_PARTS; both DEVICE data.
 *   PRESENT: component j is present iff ids[q][j] names a loaded character (inside the table; on a resident bank a non-empty slot) and at
 *     least one of its six weights is usable.  A weight is usable iff 0 < w <= FLT_MAX: NaN, negatives, zero and infinities count as 0.
 *     A component that is not present reads no bank row and reports idx -1, dist +inf, weights 0: a ramp that reached 0 costs no scan.
 *   MATCH: a present component's row is the exact 1-NN of the window's query in that character - index, tie rule (lowest row), distance
 *     and bank arithmetic are mocha_match_segmented's for (that query, that id), bit for bit (fp32 rows, or the centred bf16 copy).
 *   NORMALISATION: per part v, s_v = the sum of the usable weights of present components (fp32, j ascending).  s_v > 0: wnorm[j][v] =
 *     w[j][v] / s_v (one IEEE division); otherwise the lowest present j gets 1 for that part, the others 0.
 *   FEATURE: F[t][v][c] = sum_j wnorm[j][v] * encoded[row_j][t][v][c] in the soft blend's arithmetic: from 0 in fp32, j ascending, every
 *     product and every sum rounded on its own; terms with wnorm == 0 are skipped and their row not read, so a window with one effective
 *     component gets that entry's bits.  The same id may appear in two components: both match the same row and their weights add.
 *   NO COMPONENT PRESENT: as an invalid id in the hard calls - idx -1, dist +inf, weights 0, the decoder reads row 0 (an unspecified Y).
 * NOT provided: mix together with soft (k > 1) or action-constrained matching per component, inertializing weight changes, the Ours
 * sessions, more than MOCHA_MIX_MAX components, more than 16 streams per step.
 * J outside 1..MOCHA_MIX_MAX and a NULL required pointer are MOCHA_ERR_ARG and a bank without a segment table MOCHA_ERR_STATE, before
 * anything is launched.  Nothing here allocates or synchronises: mocha_bank_set_segments, mocha_bank_resident_create and mocha_reserve also
 * reserve the scratch of 16 windows x 4 components per workspace set (64 x the largest segment's 16-row granules x 8 bytes, + 3 KB); a
 * larger batch walks its windows 16 at a time.  Launches per 16 windows: mocha_mix_prep, the plan, the scan and the finish over the Q x J
 * pseudo-queries (the J pseudo-queries of a window read its one query row), mocha_seg_mix_blend.  Scan cost: the sum over blocks (up to 8
 * pseudo-queries sharing a character) of that character's rows x 23 040 x bytes per value.
 *   mocha_match_mix_segmented : idx (Q,J) local rows; dist (Q,J), wnorm (Q,J,6), out (Q,90,256) or NULL.
 *   mocha_characterize_mix_segmented : mocha_characterize_segmented with the decoder run on F (the literal flow of the soft calls: the
 *                             bank's per-entry decoder constants do not apply to a blend).  idx (B,J) / wnorm (B,J,6) or NULL.
 *   mocha_step_graph_mix_segmented : that call for 1 <= S_w <= 16 windows captured into a HIP graph on first use and replayed; idx and wnorm
 *                             required.  Keyed on the buffer pointers, S_w, J, raw and the generation; the CONTENTS of ids and weights
 *                             are read by every replay and re-capture nothing.  Before a capture the step runs once eagerly.
 *   mocha_live_step_mix / mocha_live_step_raw_mix : mocha_live_step / mocha_live_step_raw with that characterize in place of the hard
 *                             one; ids (S,J) and weights (S,J,6) stand where seg stands, idx is (S,J) and wnorm (S,J,6) follows valid.
 *                             The session buffer, its size and layout, mocha_live_reset and the warming rule are unchanged.  A stream
 *                             none of whose components is present (every character retired, every weight 0) sits the step out as a
 *                             warming one: valid 0, its output rows untouched, its post state not advanced, idx -1, wnorm 0; it resumes
 *                             when a component is present again.  Each has its own captured graph and the eager pass before a capture. */
#define MOCHA_MIX_MAX 4
#define MOCHA_MIX_PARTS 6
int mocha_match_mix_segmented(mocha_ctx* ctx, const float* query_nm, int Q, const int32_t* ids, const float* weights, int J, int32_t* idx,
                              float* dist, float* wnorm, float* out, void* stream);
int mocha_characterize_mix_segmented(mocha_ctx* ctx, const float* src_X, int B, const int32_t* ids, const float* weights, int J,
                                     const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx, float* wnorm, int raw, void* stream);
int mocha_step_graph_mix_segmented(mocha_ctx* ctx, const float* X, int S_w, const int32_t* ids, const float* weights, int J,
                                   const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx, float* wnorm, int raw, void* stream);
int mocha_live_step_mix(mocha_ctx* ctx, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                        const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                        const unsigned char* contact, const int32_t* ids, const float* weights, int J, const float* cnt_mean,
                        const float* cnt_std, double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                        int32_t* valid, float* wnorm, void* stream);
int mocha_live_step_raw_mix(mocha_ctx* ctx, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                            const float* rot, const float* pos, const int32_t* ids, const float* weights, int J, const float* cnt_mean,
                            const float* cnt_std, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler,
                            int32_t* idx, int32_t* valid, float* wnorm, void* stream);

/* WHOLE clips through the same preparation, parallel over frames: process_data (preprocess/generate_database.py:86-177) with mirror =
 * False / True and divide_clip(divide=True) (:57-84), the first link of raw clip -> database.bin -> bank (generate_database_bin.py:96-208)
 * and of raw clip pair -> windows -> mocha_characterize_pair.  Every frame of a clip is emitted, frame 0 and the last included: the fits'
 * first / last window rows (savgol_filter mode='interp'), v[0] = v[1] - (v[3] - v[2]), v[-1] = v[-2] + (v[-2] - v[-3]), the median
 * filter's 'nearest' padding.  Float64 on the fp32 inputs, rounded to fp32 once at the output, as mocha_live_ingest_step.
 *   mocha_ingest_clips     : n_clips clips concatenated along the frame axis, clip c = frames clip_offsets[c] .. clip_offsets[c+1]-1 (host
 *                            array of n_clips + 1 values, clip_offsets[0] = 0); nothing crosses a clip boundary.  rot (F,V,4) quaternions
 *                            w,x,y,z or (F,V,3) Euler degrees (cfg->rot_format, cfg->euler_order), pos (F,V,3); cfg->lookahead is ignored.
 *                            mirror_flags (n_clips, host, or NULL): a clip with a non-zero flag goes through animation_mirror
 *                            (generate_database.py:40-55: forward kinematics, mirror_pos * gpos[map], from_xform(mirror_rot *
 *                            to_xform(grot[map])) with the four branches of quat.py:69-94, quat.ik) and a second quat.unroll (:95) first;
 *                            mirror_map (V, host): the joint exchange, map[map[v]] == v.  Outputs, root bone first: out_pos / out_vel /
 *                            out_ang (F,V+1,3), out_rot (F,V+1,4) fp32, out_contact (F,n_contact) uint8.  quat.unroll (quat.py:135-141)
 *                            runs as a parity scan per (clip, joint); six launches, eight with a mirrored clip.
 *                            NOT capture-safe: the call copies its tables to the device and waits for `stream` once before its launches,
 *                            and it may (re)allocate the context's float64 clip workspace (about 90 (V+1) bytes per frame, grow-only, does
 *                            not move mocha_generation()).
 *   mocha_clip_window_count: counts[c] = the windows divide_clip cuts from clip c: j = 0, step, 2 step, ... < n - window / 4 (:67).  Host
 *                            only; MOCHA_ERR_ARG for a NULL pointer, window < 4, step < 1 or offsets that do not increase.
 *   mocha_clip_windows     : the gather, ONE launch: window b of a clip starts at frame j = b * step of it; a slice of m < window frames
 *                            is padded on the left with (window-m)/2 + (window-m)%2 copies of its first frame and on the right with
 *                            (window-m)/2 copies of its last (:69-77), padding frames of vel / ang zero.  Inputs as mocha_ingest_clips
 *                            writes them; outputs Yrot (B,window,V+1,4), Ypos / Yvel / Yang (B,window,V+1,3) as mocha_featurize takes
 *                            them and Ycontact (B,window,n_contact), B = the sum of mocha_clip_window_count, clip after clip.
 *                            divide=False is not provided.  Not capture-safe, as above.
 *   mocha_mirror_map_default: the left / right exchange of `layout`: 0 ('mocha': Left* / Right* of the 24 joint names, legs 1-4 / 20-23,
 *                            arms 9-12 / 16-19), 1 ('mixamo' of this library's 22-joint table: arms 6-9 / 10-13, legs 14-17 / 18-21).
 * Refusals (MOCHA_ERR_ARG, nothing launched): everything mocha_live_ingest_step refuses (the lookahead apart); a clip shorter than 31 frames
 * (savgol_filter(window_length=31) raises there); clip_offsets that do not start at 0 or do not increase; a mirror flag set while
 * mirror_map is NULL; a mirror_map that is no involution or does not commute with the parents; window < 4 or step < 1.
 * Inherited from the reference: the singular -z heading; contacts flip at a hard threshold (generate_database_bin.py uses 0.2 m/s,
 * process_data 0.5: cfg->contact_velocity_threshold).  BVH text: mocha_bvh_header / mocha_bvh_motion below. */
int mocha_ingest_clips(mocha_ctx* ctx, const mocha_ingest_cfg* cfg, const mocha_post_cfg* post, const float* rot, const float* pos,
                       const int32_t* clip_offsets, int n_clips, const int32_t* mirror_map, const unsigned char* mirror_flags,
                       float* out_pos, float* out_vel, float* out_rot, float* out_ang, unsigned char* out_contact, void* stream);
int mocha_clip_window_count(const int32_t* clip_offsets, int n_clips, int window, int step, int64_t* counts);
int mocha_clip_windows(mocha_ctx* ctx, const float* pos, const float* vel, const float* rot, const float* ang,
                       const unsigned char* contact, int n_contact, const int32_t* clip_offsets, int n_clips, int window, int step,
                       float* Yrot, float* Ypos, float* Yvel, float* Yang, unsigned char* Ycontact, void* stream);
int mocha_mirror_map_default(int layout, int32_t* map);

/* RESAMPLING in front of the calls above: the network, the 60-frame windows, the 15- / 31-tap root fits and the bank are fixed to 60 frames
 * per second (generate_database.py:148-149, motion/bvh.py:179); cfg->fps only scales the finite differences.  These calls take (rotations,
 * positions) at a source rate to (unit quaternions w,x,y,z, positions) at the target rate: rot_out / pos_out are what mocha_ingest_clips and
 * mocha_live_ingest_step read with rot_format = 0 and fps = the target rate.  The reference has no resampler; the definition uses its
 * quaternion primitives only.  The step between outputs is num / den source frames: source_fps / target_fps reduced, each term 1..4096.
 *   count    a clip of n >= 1 source frames gives m = floor((n-1) den / num) + 1 outputs.
 *   output k t = k num in 64-bit integers, i = t div den, a = (double)(t mod den) / (double)den.  q: the clip's quaternions in float64 -
 *            quat.from_euler(np.radians(e), order) (quat.py:57-67) or the quaternions as given - sign-unrolled along time (quat.unroll,
 *            :135-141).  a == 0: the output is q[i], p[i] with no arithmetic, and frame i+1 is not read.  Otherwise the rotation is
 *            mul(from_scaled_angle_axis(a * to_scaled_angle_axis(abs(mul_inv(q[i+1], q[i])))), q[i]) (:18-19, 112-126, 149-164, the eps = 1e-5
 *            branches kept): the constant angular velocity the reference's difference formula gives the interval; it agrees with the
 *            textbook slerp to 2.3e-16 and is unit length to 3.4e-16.  The position is p[i] + a (p[i+1] - p[i]) in the file's units (no
 *            unit scale here: the ingester applies it).  Float64 on the fp32 inputs, rounded to fp32 once at the output.
 *   mocha_resample_frames     : HOST only.  m for one clip; negative (MOCHA_ERR_ARG) for n < 1, n >= 2^31 or a term outside 1..4096.  m may
 *                               exceed 2^31.
 *   mocha_resample_clips      : n_clips clips concatenated along the frame axis (offsets_in as clip_offsets above; a clip may have ONE frame);
 *                               num / den / offsets_out are host arrays, one ratio per clip, so files of different rates share a call.
 *                               offsets_out (n_clips + 1) must be the prefix sums of mocha_resample_frames.  rot (F,V,4) or (F,V,3) Euler
 *                               degrees (rot_format 0 / 1 and euler_order[3] as in mocha_ingest_cfg; euler_order may be NULL for
 *                               quaternions), pos (F,V,3); rot_out (F',V,4), pos_out (F',V,3), F' = offsets_out[n_clips].  Three launches:
 *                               the ingester's quaternion and unroll kernels on the context's clip workspace (60 V bytes per source frame),
 *                               then one thread per (output frame, joint).  Nothing crosses a clip boundary.  NOT capture-safe: waits for
 *                               `stream` once for its tables and may grow the workspace, as mocha_ingest_clips.
 *   mocha_resample_state_bytes: the size of the streaming state of `streams` streams: per joint the previous unrolled quaternion, its
 *                               position and its unroll sign in float64, and two words per stream (fresh, have).  All-zero = no frame seen.
 *   mocha_resample_reset      : the listed streams (which, n; NULL = all) have seen no frame.  Enqueued on `stream`.
 *   mocha_resample_step       : ONE source frame of `streams` streams in lockstep, rot (S,V,4|3), pos (S,V,3): push number push_index (from 0)
 *                               writes the outputs k with floor((push_index-1) den / num) < k <= floor(push_index den / num), the e-th of them
 *                               to rot_out[s][e] / pos_out[s][e] of rot_out (S,4,V,4), pos_out (S,4,V,3); *n_out = their number (0..4), the
 *                               same for every stream, computed on the host from the integers alone.  Rows e >= *n_out are not written.
 *                               A stream without a predecessor (after mocha_resample_reset, or an all-zero state) emits the new frame
 *                               for every output of that push.  The outputs of pushes 0, 1, 2, ... concatenated are mocha_resample_clips'
 *                               of the same frames BIT FOR BIT (both kernels call one device function).  One launch, no allocation, no
 *                               synchronisation, capture-safe (push_index, num, den are baked into a captured launch).
 * Refusals (MOCHA_ERR_ARG, nothing launched): a NULL required pointer; streams outside 1..16; num or den outside 1..4096; den > 4 num in
 * the step (more than four outputs per source frame: at a 60 fps target, sources below 15 fps); offsets_out that are not the prefix sums.
 * What it is not: linear / slerp only (no cubic interpolation), no low-pass filter before decimation, one rate per streaming state. */
int64_t mocha_resample_frames(int64_t n, int num, int den);
int mocha_resample_clips(mocha_ctx* ctx, int rot_format, const int* euler_order, const float* rot, const float* pos,
                         const int32_t* offsets_in, const int32_t* num, const int32_t* den, int n_clips, const int32_t* offsets_out,
                         float* rot_out, float* pos_out, void* stream);
int64_t mocha_resample_state_bytes(const mocha_ctx* ctx, int streams);
int mocha_resample_reset(mocha_ctx* ctx, void* state, int streams, const int32_t* which, int n, void* stream);
int mocha_resample_step(mocha_ctx* ctx, int rot_format, const int* euler_order, void* state, int streams, const float* rot, const float* pos,
                        int num, int den, int64_t push_index, float* rot_out, float* pos_out, int32_t* n_out, void* stream);

/* WORLD-SPACE POSES AND SKINNING PALETTES behind the calls above: what the reference's demo computes at its end - quat.fk over every output
 * stream (test_fullframework.py:672-690), the global positions going to animation_plot (:670) - and what an engine binds per skinned mesh.
 * Every pose the library emits or takes is LOCAL: rot (..,V+1,4) w,x,y,z and pos (..,V+1,3), parent-relative, the trajectory root bone first.
 *   fk       For a frame with locals q[b], p[b], b = 0..V, and the context's parents ([-1] + (joint parents + 1), test_fullframework.py:
 *            101-102: the table mocha_postprocess uses; par[b] < b):  G[0] = q[0], g[0] = p[0];  G[b] = mul(G[par b], q[b]);
 *            g[b] = mul_vec(G[par b], p[b]) + g[par b]  - quat.fk (motion/quat.py:166-173) with mul (:112-120) and mul_vec (:128-130), in
 *            float64.  Inputs are taken as given: NO normalisation of pose quaternions.
 *   palette  For bone b = 1..V (the engine's skeleton is the V bones without the trajectory root, as in the BVH writer's merge) the 3x4 matrix
 *            P[b] = pre o [to_xform(G[b]) | g[b]] o [to_xform(B[b]) | c[b]]^-1  with to_xform as quat.py:27-40; (B, c) = fk of a rest pose whose
 *            quaternions are normalised once with quat.normalize (:15-16); the inverse is the rigid one (R^T, -R^T c); pre is any 3x4 affine
 *            map (unit scale, axis swap, handedness).  Affine maps compose as (R1 R2 | R1 t2 + t1), sums over k = 0, 1, 2 in that order; the
 *            product is evaluated in float64 left to right as written, rounded ONCE to fp32 and stored row-major as 12 floats
 *            (r00 r01 r02 t0 | r10 .. | r20 ..).
 *   mocha_world_bind_bytes : HOST only.  The size of a bind: caller-owned device memory with a private layout (pre and V+1 inverse binds).
 *   mocha_world_bind       : rest_rot (V+1,4) float64 on the device or NULL = identity rotations, rest_pos (V+1,3) float64 on the device,
 *                            pre = 12 doubles row-major on the HOST or NULL = identity.  Computes the inverse bind globals on the device
 *                            with the fk function mocha_world_pose runs; one launch on `stream`.
 *   mocha_world_pose       : n frames.  rot (n,V+1,4) and pos (n,V+1,3) on the device, float64 (in_f32 = 0: what mocha_postprocess,
 *                            mocha_postprocess_step and mocha_live_step* emit; pass ik_rot or rot) or fp32 (in_f32 = 1: what
 *                            mocha_live_ingest_step, mocha_ingest_clips and mocha_resample_clips emit with their root bone; each value is
 *                            widened on load, the code is otherwise the same, so fp32 inputs give the bits of the same values passed as
 *                            float64).  Outputs, each may be NULL: gpos (n,V+1,3), grot (n,V+1,4) float64; palette (n,V,12) fp32, which needs
 *                            `bind`.  valid (n) int32 on the device or NULL: rows with valid[i] == 0 are NOT written (the live step's rule
 *                            for warming streams).  rot, grot and palette must be 16-byte aligned.  A frame's result does not depend on
 *                            n, on its index or on which outputs are asked for: n frames in one call are bit for bit the n calls of one
 *                            frame.  One launch, no allocation, no synchronisation, reads no context state that a later call changes and
 *                            does not move mocha_generation: capture-safe, and captured steps keep replaying.
 * Refusals (MOCHA_ERR_ARG, nothing launched): a NULL rot, pos, rest_pos or bind buffer; a palette without a bind; all three outputs NULL;
 * a pre that is not finite; n < 0; in_f32 outside 0..1; a misaligned array.  n == 0 is a no-op.
 * What it is not: no mesh skinning (the palette is what a vertex shader multiplies by); no global velocities (quat.fk_vel); no dual
 * quaternions; one bind per call; mocha_live_step* do not call it inside their captured graph - launch it behind them on the same stream. */
int64_t mocha_world_bind_bytes(const mocha_ctx* ctx);
int mocha_world_bind(mocha_ctx* ctx, const double* rest_rot, const double* rest_pos, const double* pre, void* bind, void* stream);
int mocha_world_pose(mocha_ctx* ctx, const void* rot, const void* pos, int in_f32, int64_t n, const int32_t* valid, const void* bind,
                     double* gpos, double* grot, float* palette, void* stream);

/* BVH TEXT in front of mocha_ingest_clips: what the reference's loader (motion/bvh.py:22-138) returns - Euler degrees in file channel
 * order and positions in file units per joint - as the two fp32 device arrays mocha_ingest_clips reads.  The hierarchy is read on the
 * host, the numbers of the MOTION block (over 99.9 % of a file) are parsed on the device.
 *   mocha_bvh_header       : HOST only, no context, no GPU.  Reads the HIERARCHY block and the Frames: / Frame Time: lines of `text`
 *                            (nbytes bytes, NOT NUL-terminated; nothing outside [text, text + nbytes) is read).  Joints are numbered in
 *                            file order as bvh.load numbers them (:43-49, :81-87); End Site offsets are ignored (:61-65); names are (byte
 *                            offset, length) into the text and may hold ':' (:43, :81).  channels = 3: the root has 6 channels, every
 *                            other joint 3 rotations; 6: every joint has 3 positions and 3 rotations (a root alone counts as 6).
 *                            order[i] = the axis (0 x, 1 y, 2 z) of rotation channel i.  [motion_begin, motion_end) = the numeric block:
 *                            from the first byte after the Frame Time: line to nbytes.  Line ends \n or \r\n, tabs and spaces.
 *                            Refused (MOCHA_ERR_ARG; error_offset = the first byte of the offending line, error = what is wrong, where
 *                            the reference reads silently and wrongly, :67-77, :112-118): 9-channel joints, position channels not in
 *                            X Y Z order, joints that disagree on the rotation order or on the channel count beyond the root / non-root
 *                            split, more than MOCHA_BVH_MAX_JOINTS joints, a missing MOTION, Frames: or Frame Time:, unbalanced braces,
 *                            text that ends inside the hierarchy, any other line in the hierarchy.
 *   mocha_bvh_motion       : the numeric blocks of n_clips files -> rot / pos (F,v_out,3) fp32, F = clip_offsets[n_clips], in exactly the
 *                            layout mocha_ingest_clips reads.
 *                            text_dev (DEVICE, 16-byte aligned, nbytes a multiple of MOCHA_BVH_ALIGN) holds ONLY the numeric blocks.
 *                            Packing rule: clip c occupies [clip_text_begin[c], clip_text_end[c]); clip_text_begin[0] = 0 and every begin
 *                            is a multiple of MOCHA_BVH_ALIGN; every byte between a clip's end and the next begin, and from the last end
 *                            to nbytes, is '\n'.  text_host (or NULL) is a host copy of the same bytes.  clip_text_begin / clip_text_end
 *                            (n_clips) and clip_offsets (n_clips + 1, as mocha_ingest_clips takes them) are HOST arrays; n_joints and
 *                            channels come from the header and hold for every clip of the call.  joint_map (HOST, n_joints, or NULL =
 *                            identity with v_out = n_joints): file joint j is written to output joint joint_map[j], -1 drops it; the
 *                            kept joints must cover 0..v_out-1 once each.  offsets_out (HOST, (v_out,3) fp32; required for channels ==
 *                            3): the positions of the joints that have no position channels (:97, :113).
 *                            A token is a maximal run of bytes other than space, \t, \r, \n; a frame is a non-empty line and holds
 *                            exactly C = 3 + 3 n_joints (channels 3) or 6 n_joints (channels 6) tokens; clip c holds exactly
 *                            (clip_offsets[c+1] - clip_offsets[c]) C tokens.  Grammar of a token, at most 64 bytes:
 *                            [+-]? (digits [. digits?]? | . digits) ([eE] [+-]? digits)?  - no nan, inf, hex or underscores.  Its value
 *                            is float(token) as Python reads it (:109, correctly rounded decimal -> float64), rounded once to fp32: bit
 *                            for bit, -0.000000 keeps its sign.  At most 15 significant digits and a net decimal exponent within +-22
 *                            (everything a %f writer emits) convert on the device: double(m) * 10^e or double(m) / 10^-e, one IEEE
 *                            operation on exact operands.  Any other token is a SLOW token: the device lists it (at most
 *                            MOCHA_BVH_MAX_SLOW per call), the call converts it with strtod from text_host and patches the outputs.
 *                            Four launches (mocha_bvh_count, mocha_bvh_scan, mocha_bvh_parse, mocha_bvh_finish), a fifth
 *                            (mocha_bvh_patch) only with slow tokens.  report (HOST, may be NULL): tokens found, slow tokens, first_bad =
 *                            the byte offset into text_dev of the first violation or -1.
 *                            MOCHA_ERR_STATE (first_bad set, outputs unspecified): a malformed or overlong token (its first byte), a
 *                            line whose first token is not a multiple of C into its clip or a token C into a line that does not start
 *                            one (that token), a token beyond the clip's frames or in a gap (that token), a clip with too few tokens
 *                            (its clip_text_end); also a slow token without text_host and more than MOCHA_BVH_MAX_SLOW slow tokens.
 *                            MOCHA_ERR_ARG, nothing launched: a NULL required pointer, a misaligned text_dev / nbytes / clip begin,
 *                            clip ranges that overlap or leave the buffer, nbytes >= 2^31, n_joints outside 1..MOCHA_BVH_MAX_JOINTS,
 *                            channels other than 3 or 6, a joint_map that is no such map, clip_offsets that do not increase from 0.
 *                            NOT capture-safe: the call uploads its tables, may (re)allocate the context's parse buffer (8 bytes per
 *                            4096 bytes of text plus 64 KiB, grow-only, does not move mocha_generation()) and waits for `stream` once
 *                            after its launches to read the report (a second time only to patch slow tokens). */
#define MOCHA_BVH_MAX_JOINTS 256
#define MOCHA_BVH_ALIGN 4096
#define MOCHA_BVH_MAX_SLOW 4096
typedef struct mocha_bvh_hdr {
    int32_t n_joints, channels;          /* channels: 3 or 6, see above */
    int32_t order[3], reserved;
    int64_t frames;
    double frame_time;
    int64_t motion_begin, motion_end;    /* byte range of the numeric block */
    int64_t error_offset;                /* -1, or the first byte of the refused line */
    char error[128];
    int32_t parents[MOCHA_BVH_MAX_JOINTS];
    int32_t name_length[MOCHA_BVH_MAX_JOINTS];
    int64_t name_offset[MOCHA_BVH_MAX_JOINTS];
    double offsets[MOCHA_BVH_MAX_JOINTS][3];
} mocha_bvh_hdr;
typedef struct mocha_bvh_report { int64_t tokens, slow, first_bad; } mocha_bvh_report;
int mocha_bvh_header(const char* text, int64_t nbytes, mocha_bvh_hdr* hdr);
int mocha_bvh_motion(mocha_ctx* ctx, const char* text_dev, int64_t nbytes, const char* text_host, const int64_t* clip_text_begin,
                     const int64_t* clip_text_end, const int32_t* clip_offsets, int n_clips, int n_joints, int channels,
                     const int32_t* joint_map, int v_out, const float* offsets_out, float* rot, float* pos, mocha_bvh_report* report,
                     void* stream);

/* BVH TEXT behind mocha_postprocess: the MOTION block the reference's writer emits (motion/bvh.py:210-224) for the float64 channels
 * mocha_postprocess leaves on the device, produced on the device.  The hierarchy lines stay with the host (a few hundred bytes).
 *   mocha_bvh_text_bound   : HOST only, no context, no GPU.  frames * (C * MOCHA_BVHW_MAX_TOKEN + 1): the most bytes frames frames can
 *                            take, C = 3 + 3 n_joints (save_positions 0) or 6 n_joints (1).  -1 for frames < 0 or n_joints < 1.
 *   mocha_bvh_format       : bvh_pos / bvh_euler (F,n_joints,3) float64 (DEVICE; F = clip_offsets[n_clips]; degrees) -> text_dev (DEVICE,
 *                            any alignment, capacity bytes).  A token is element (frame, column) of a virtual (F, C) matrix.
 *                            save_positions 0: columns 0..2 are pos[f, 0, :], column 3 + 3i + k is euler[f, visit[i], axes[k]].
 *                            save_positions 1: column 6i + k is pos[f, visit[i], k] for k < 3, else euler[f, visit[i], axes[k - 3]].
 *                            visit (HOST, n_joints): the joint of column group i - the writer's depth-first order; axes (HOST, 3): the
 *                            axis (0 x, 1 y, 2 z) of rotation channel k.  Every token is followed by one space, every frame ends with
 *                            '\n' behind its last space.  Clips are concatenated along the frames (clip_offsets: HOST, n_clips + 1,
 *                            increasing from 0, as mocha_ingest_clips takes them) and their text blocks lie back to back:
 *                            clip_text_begin (HOST, n_clips + 1, written by the call) holds the first byte of every clip's block and,
 *                            last, the total.
 *                            A token is Python's "%f" of the float64 (:215-222): the correctly rounded six-decimal expansion, ties to
 *                            even, in exact integer arithmetic (csrc/fmt_f6.h); the sign is the sign BIT (-0.0 and -1e-9 give
 *                            "-0.000000").  Admitted values are finite with |x| < 1e12 - a token then has at most 20 bytes,
 *                            MOCHA_BVHW_MAX_TOKEN with its space.  NaN, +-inf and |x| >= 1e12 are refused.
 *                            The call launches mocha_bvhw_count and mocha_bvhw_scan, then waits for `stream` ONCE to read the totals.
 *                            report (HOST, may be NULL): tokens = F C, bytes = the exact length of the text, first_bad = the SMALLEST
 *                            refused token ordinal (frame * C + column) or -1.
 *                            MOCHA_ERR_STATE: a value was refused; report.first_bad says which, text_dev is untouched.
 *                            MOCHA_ERR_ARG after the wait: capacity is below the exact total; report.bytes and clip_text_begin are set,
 *                            text_dev is untouched.  Otherwise the call enqueues mocha_bvhw_write and returns without a second wait;
 *                            no byte outside [text_dev, text_dev + report.bytes) is written.
 *                            MOCHA_ERR_ARG, nothing launched (judged before the context is looked at): a NULL required pointer,
 *                            n_joints outside 1..MOCHA_BVH_MAX_JOINTS, a visit or axes that is no permutation, clip_offsets that do
 *                            not increase from 0, a negative capacity, mocha_bvh_text_bound at or above 2^31 bytes, a NULL context.
 *                            NOT capture-safe: the call uploads its tables, may (re)allocate the context's format buffer (8 bytes per
 *                            256 tokens plus the tables, grow-only, does not move mocha_generation()) and waits for `stream`. */
#define MOCHA_BVHW_MAX_TOKEN 21   /* bytes, with the space */
typedef struct mocha_bvhw_report { int64_t tokens, bytes, first_bad; } mocha_bvhw_report;  /* first_bad: token ordinal or -1 */
int64_t mocha_bvh_text_bound(int64_t frames, int n_joints, int save_positions);
int mocha_bvh_format(mocha_ctx* ctx, const double* bvh_pos, const double* bvh_euler, const int32_t* clip_offsets, int n_clips,
                     int n_joints, const int32_t* visit, const int32_t axes[3], int save_positions, char* text_dev, int64_t capacity,
                     int64_t* clip_text_begin, mocha_bvhw_report* report, void* stream);

/* Bank build statistics: cnt_mean, cnt_std = np.mean(cnt, 0), np.std(cnt, 0) over the N bank entries
 * (compute_cnt_norm.py:174-175; population std), x (N, 90*256) -> mean, std (90*256). */
int mocha_column_stats(mocha_ctx* ctx, const float* x, int64_t N, float* mean, float* std_, void* stream);

/* Runtime options.  "dual_stream" (default 0): batches of at least "dual_min" (default 128) windows are split in two
 * halves that run concurrently on the caller's stream and on an internal stream (forked / joined with events, so
 * the call keeps stream semantics and stays graph-capturable); the two kernel chains fill each other's prologue /
 * epilogue / tail bubbles (+5 % on the demo step).  Results are unchanged except for the kernel choice per half.
 * "fold_decoder" (default 1): the decoder's key and value projections are folded into its query and output weights at
 * mocha_finalize_weights (possible because decoder_dim_head == dim; exact algebra, differences are fp32 rounding only),
 * which removes two of the four projection GEMMs per decoder layer; 0 runs the four projections as written in
 * net/transformer.py:62-76.
 * "gemm_bf16x3" (default 1): the large GEMM launches (every nn.Linear / conv-as-GEMM of the path whose batch fills the chip
 * and whose output width is a multiple of 64) run on the bf16 matrix pipe with both fp32 operands carried as three bf16
 * planes and six MFMA passes per product, fp32 accumulation (gemm_x3.hip): every bf16 x bf16 product is exact in fp32 and
 * the dropped cross terms are below 2^-26 of a product, so the result is as accurate as an fp32 FMA chain (measured against
 * float64: slightly more accurate than the exact-f32 MFMA kernel, tests/test_gemm_engines.py).  0 = every GEMM on
 * v_mfma_f32_32x32x2_f32 (gemm_f32.hip).
 * "attention_bf16x3" (default 1): the Generator's attention (net/transformer.py:65-76; 90 tokens, head dim 128 / 256) computes
 * QK^T and PV the same way - K, Q, V and the softmax probabilities as three bf16 planes each, six MFMA passes per product,
 * fp32 accumulation and an fp32 softmax (attention_x3.hip); 0 = v_mfma_f32_32x32x2_f32 (attention.hip).  The CVAE sampler's
 * attention (head dim 64) always uses attention.hip.
 * "attention_split_max" (default 192): up to this many (window, head) pairs the head-dim-256 attention
 * (the decoder's) gives each pair twelve waves - four groups contract a quarter of the head dim each, the partial score tiles are
 * summed through LDS in a fixed order, each group then writes a quarter of the output columns - because a one-window launch is
 * otherwise a serial chain of twelve staging steps per wave.  Same operands and products; the scores are summed in a different
 * association than the three-wave kernel's, so results agree to fp32 rounding.  0 = always the three-wave kernel.
 * "fold_joint" (default 1): the embedding joint block's 1x1 gcn conv folded into its k = 5 temporal conv at
 * mocha_finalize_weights (net/blocks.py:126-134 applies them back to back with nothing in between: one linear map, K = 5 x 192);
 * 0 runs the two convolutions as two GEMMs.  Differences are fp32 rounding only.
 * "lanes" (default 1, 1..3): workspace sets / captured graphs for mocha_step_graph_lane; changing it re-plans the workspaces.
 * "scan16" (default 1): see MOCHA_BANK_BF16 above - fp32 banks of >= 4096 rows are scanned through a centred bf16 copy with an
 * exact fp32 re-rank when at most 8 queries are matched; takes effect at the next mocha_bank_set; 0 scans the fp32 rows.
 * Round 4 (INTEGRATION.md section 6 has the table; PER CONTEXT since ABI 5 - round 4 kept five of them in process-wide variables):
 * "embed_sums" (default 1): mot_embedding's first stage and the joint
 * block's five-tap 4-frame sums in one kernel whose frame rows stay in LDS (0: two kernels, bit-identical); "embed_front_max_wgs"
 * (default 512): that kernel's persistent grid; "inorm_split_max" (default: every batch): windows up to
 * which the instance norms spread a window's channels over four workgroups (bit-identical either way); "gemm_persistent" (default 768
 * workgroups; 0 = off) and "gemm_persistent_max_n" (default 512): the plane GEMM's persistent instance, bit-identical; "select2"
 * (default 1) / "match_planes" (default 1; 2 = two bf16 query planes in the bf16 coarse pass): the many-query selection with
 * producer-side row statistics - the same exact result; "attention_kv", "attention_kv_pairs" (default 0): decoder attention from
 * pre-split key / value images, bit-identical; "bank_tiled" (default 0): bf16 banks, a tiled image for the many-query coarse pass;
 * "dual_min" (default 128): smallest batch that "dual_stream" splits over two streams (re-plans the workspaces).
 * "fold_upsample" (default 1): to_mot's k = 5 temporal conv over the nearest-x4-upsampled frames (model.py:74, net/blocks.py:112-118) as a
 * 3-tap conv over the 15 source frames with per-phase summed weights (exact algebra; differences are fp32 rounding of the weight sums);
 * "upsample_split_min" (default 256): windows from which it runs as two 2-tap launches.
 * Round 5 (ABI 5):
 * "adain_closed_form" (default 1): the decoder's AdaIN -> instance norm pair (net/transformer.py:108-113 then :49-56) from ONE set of
 * token statistics: with m, s the mean / unbiased std of x, AdaIN(x) = (1+g)(x-m)/(s+eps) + b has token mean exactly b and std
 * |1+g| s/(s+eps), so IN(AdaIN(x)) = (1+g)(x-m) / (|1+g| s + eps (s+eps)) - the same function in real arithmetic, without the
 * cancellation against b that costs the literal fp32 order (and the reference) the digits of every channel whose 1+g is small.
 * 0 = the literal two-pass order (A/B: tools/structured_matrix.py).
 * "style_f64" (default 1): the AdaIN style MLP (net/transformer.py:100-107; mean over tokens -> Linear -> LeakyReLU -> Linear) in
 * float64 from a float64 token mean, gamma / beta rounded to fp32 once; 0 = the fp32 GEMM engines.
 * "bank_dec_cache" (default 1): mocha_bank_set also computes what the decoder derives from a bank ENTRY alone - IN(entry) (the folded
 * decoder's keys) and every layer's gamma / beta - (+ 92 KB + 2 KB x decoder depth per entry), and mocha_characterize /
 * mocha_step_graph read them in place through frame_index instead of recomputing them per call from a gathered copy
 * (needs "style_f64", "fold_decoder", decoder_dim_head == dim, "attention_bf16x3", no "attention_kv"; otherwise, and with 0, the
 * per-call flow).  Takes effect at the next mocha_bank_set.
 * "match_pass" (default 0 = round 4's mocha_match_gemm_bf16_dma): 1 / 2 = the bf16 bank's coarse pass for up to "match_pass_max_q"
 * (default 256) queries as mocha_match_pass256 (match_pass.hip: 128 x 256 tiles, bank operands straight into registers, K split 16) on
 * the row-major bank / on an operand-order image built at the first such call (+ 2 B per bank value).  Same products summed over other K
 * slices: the selection's exact re-evaluation makes the answer the same.  Measured no faster at 128 queries, 13 us faster at 256 from the
 * image.  "match_pass_variant": that kernel's prefetch depth / non-temporal bit (diagnostic).
 * "match_nt" (default 1): the round-4 kernel's bank loads carry the non-temporal hint when a launch reads the bank once (Q <= 128).
 * "pair_overlap" (default 1): mocha_characterize_pair computes the transient bank's decoder constants on the context's internal stream
 * beside the matching chain (forked / joined with events; bit-identical, -0.6 % of the demo step).
 * "match_fold" (default 0; a measured negative kept reproducible): the bf16 many-query coarse pass's last-arriving
 * K-slab workgroup per tile adds the slabs up into slab 0 and the selection reads one slab; same indices, the pass 53 us slower.
 * "scan8" (default 0): mocha_bank_set also keeps the centred rows of an fp32 bank of >= 4 096 entries as biased bytes with a per-row scale and a
 * measured residual bound (+ N x 23 040 B); mocha_match with <= 4 queries then scans 1 B per value and re-evaluates exactly, on the fp32 rows,
 * every row the byte image cannot exclude - the result of the exact fp32 search - and falls back, by itself and on the device, to the bf16 scan
 * for banks / queries where the image excludes too little (independent N(0, 1) rows).  Takes effect at the next mocha_bank_set.
 * "gemm_x3r_min_n" (default 0 = never): K = 256 plane-GEMM launches of at least 8 192 rows and at least this many columns (a multiple of 256)
 * take the instance that keeps a wave's 32 activation rows resident in registers as planes for all n-tiles (gemm_x3r.hip, round 6):
 * bit-identical to the tiled instances; measured SLOWER inside the step (enc.qkv 404 -> 422 us, dec.q 144 -> 208, ff1 127 -> 166:
 * one wave per SIMD has nobody to hide behind; profiles/r06), so it stays an option.
 * "gemm_tile64_below" (default 0): mid-size plane-GEMM launches of 128-multiple width with fewer 64 x 128 tiles than this take 64 x 64
 * tiles (measured no gain); widths that are multiples of 64 only always do at mid size.
 * "gemm_f16x2" (default 0): the encoder's, decoder's and to_mot's batch-size GEMMs as TWO fp16 planes per operand and THREE
 * v_mfma_f32_32x32x16_f16 passes per product instead of three bf16 planes and six passes (gemm_h2.hip): x = fp16(S x) + fp16(residual)
 * carries 22 bits, a b ~ a0 b0 + a0 b1 + a1 b0, fp32 accumulation.  Per product 2^-22 instead of an fp32 multiply's 2^-24; a whole dot
 * product comes out CLOSER to float64 than on either fp32 engine (the accumulator's roundings dominate; tests/test_gemm_f16x2.py) at
 * 0.65-0.75 of the time.  Power-of-two scales: per weight row at pack time; per WINDOW for the activations, from bounds the producing
 * launch leaves in device memory (or that the arithmetic implies) - a window's result does not depend on the rest of the batch; rows more
 * than five decades below their window's largest magnitude keep fewer digits than fp32 would.  Launches without a bound (the raw-pose
 * embedding, calls of up to four windows) stay on the bf16 planes; the attention and the matcher always do.  The current bank's per-entry
 * bounds are taken at the next mocha_bank_set.
 * "walk" (default 1; changes results: no): the order in which the row-walking kernels of the batch path (plane GEMM, full-batch
 * attention, instance norm / AdaIN, the embedding's and to_mot's pointwise kernels, the matcher's centring, row norms and plane image)
 * touch their row blocks.  0 = every launch walks upwards; 1 = the tensor-producing steps of a call alternate - a consumer starts at the
 * rows its producer wrote last, the ones most likely still in the 256 MiB last-level cache; 2 = every eligible launch walks downwards
 * (tests).  Same tiles, same arithmetic per tile: bit-identical.  The direction is a function of the call's launch sequence alone (the
 * count starts over at every entry point and chunk), so a captured step bakes in what an eager call does.
 * Every option that changes which kernels a step launches bumps mocha_generation(ctx). */
int mocha_set_option(mocha_ctx* ctx, const char* name, int value);

/* y (M,N) = x (M,K) · w (N,K)^T + bias (N, may be NULL): nn.Linear (net/transformer.py:28-32, 57-61) as a stand-alone
 * operator on device pointers, for tests and tooling that want one of the two GEMM engines directly.
 * engine 0: the kernel the path would pick for this shape under the current options; 1: exact-f32 MFMA; 2: bf16 x 3 planes;
 * 3: fp16 x 2 planes / three passes (option "gemm_f16x2"'s engine; the activation bound is measured on every call; N % 64, K % 32)
 * (MOCHA_ERR_ARG if the shape is outside that engine: K % 32, N % 128, at least 768 row tiles ... see gemm_x3_supports).
 * With engine 2 (or 0 resolving to it) w is packed into the engine's image on every call (w may change between calls);
 * the call synchronises the stream once to free that image.  K % 32 == 0. */
int mocha_linear(mocha_ctx* ctx, const float* x, const float* w, const float* bias, float* y, int64_t M, int N, int K, int engine,
                 void* stream);

/* Introspection for tests and tooling. */
int mocha_abi_version(void);
/* Build provenance: the HIP toolchain libmocha_hip.so was compiled with ("hipcc HIP 7.2.26015-fc0010cf6a gfx950", static
 * string) and the HIP runtime version of the process that loaded it (hipRuntimeGetVersion; no device needed).  The built
 * library ships to the GPU box, whose ROCm may be older than the build container's: smoke() prints both. */
const char* mocha_build_info(void);
int mocha_runtime_version(void);
/* Monotonic counter, bumped whenever the context replaces a device buffer a captured graph may hold (workspaces, match
 * scratch, CVAE workspace) or its current bank changes.  Host-side; no synchronisation. */
int64_t mocha_generation(const mocha_ctx* ctx);
int mocha_graph_constants(mocha_ctx* ctx, float* A_j /*3*V*V host*/, float* A_b /*2*6*6 host*/,
                          float* pool /*V*6 host*/, float* unpool /*6*V host*/);

/* Copies of the current bank's rows into caller buffers, (N, 90*256) fp32 each, either may be NULL: what a rank that RECEIVED its bank
 * (mocha_bank_broadcast fills context-owned buffers) hands to further contexts of its process (mocha_bank_set ... MOCHA_BANK_BORROW on each:
 * BatchPipeline).  Enqueued on `stream`. */
int mocha_bank_export(mocha_ctx* ctx, float* cnt_nm, float* encoded, void* stream);

/* The current bank as the context holds it (device pointers, nothing is copied): the rows it matches against and gathers
 * from, and what the library derived from them - the centroid (90*256), the squared norms of the centred rows (N), the
 * centred bf16 copy (NULL for an fp32 bank).  Any out pointer may be NULL.  For tests that compare the ranks of a
 * mocha_bank_broadcast bit for bit. */
/* Option "scan8" (round 6; the matcher's one-byte first stage, match_scan8.hip): state[0] = 1 if the current bank carries the byte image,
 * state[1] = the stage's sticky mode word of workspace set `set` read back from the device (0: calls scan the byte image; 1: the refine
 * found the image's bounds useless for this bank / these queries and calls scan the bf16 copy; -1: no scratch yet).  Synchronises the device.
 * Replaces nothing in the reference (its BallTree has no such stage): introspection for tests and tooling. */
int mocha_scan_byte_state(mocha_ctx* ctx, int set, int32_t* state /*2*/, void* stream);
int mocha_bank_view(mocha_ctx* ctx, const float** cnt_nm, const float** encoded, const float** centroid, const float** row_norm2,
                    const void** cnt_bf16, int64_t* N);

/* Measurement support (bench.py roofline leg): between start and stop every kernel launch is
 * bracketed by a HIP event pair on its launch stream.  stop synchronises those events and
 * writes a JSON object {"kernels": {symbol: {launches, ms, flops, bytes}}, "sites": {...}} of
 * per-kernel totals (algorithmic flops/bytes of the launches) into `json` (capacity `cap`). */
int mocha_profile_start(mocha_ctx* ctx);
int mocha_profile_stop(mocha_ctx* ctx, char* json, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MOCHA_HIP_H */
