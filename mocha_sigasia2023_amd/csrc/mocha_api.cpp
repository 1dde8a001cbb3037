// Host side of libmocha_hip.so: context, weight loading / repacking, workspace management and
// the C-ABI entry points of include/mocha_hip.h.  Every function only enqueues work on the
// caller's stream.  Reference citations are relative to the reference repository root.
#include "../../include/mocha_hip.h"
#include "kernels.h"
#include "host_buffer.h"
#include "extent_alloc.h"

#include <rccl/rccl.h>      // types only: the RCCL entry points are resolved at run time (see Rccl below)
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <deque>
#include <map>
#include <tuple>
#include <string>
#include <vector>

using namespace mocha;

namespace {

thread_local std::string g_create_error;

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

// ------------------------------------------------------------------ skeleton constants (row a14)
// closed form of net/graph.py:116-131,290-312, computed in double
struct Skeleton {
    int V = 0;
    std::vector<int> parents, part_of;
    std::vector<double> A_j;   // [3][V][V]
    std::vector<double> A_b;   // [2][6][6]
    std::vector<double> pool;  // [V][6]
    std::vector<double> unpool;// [6][V]
};

static std::vector<double> distance_adjacency(const std::vector<int>& parents, int max_hop) {
    const int n = (int)parents.size();
    std::vector<std::vector<int>> nbr(n);
    for (int i = 0; i < n; ++i)
        if (parents[i] >= 0) { nbr[i].push_back(parents[i]); nbr[parents[i]].push_back(i); }
    std::vector<int> hop(n * n, 1 << 20);
    for (int s = 0; s < n; ++s) {
        std::deque<std::pair<int, int>> q;
        std::vector<char> seen(n, 0);
        hop[s * n + s] = 0; seen[s] = 1; q.push_back({s, 0});
        while (!q.empty()) {
            auto [v, d] = q.front(); q.pop_front();
            if (d == max_hop) continue;
            for (int u : nbr[v]) if (!seen[u]) { seen[u] = 1; hop[s * n + u] = d + 1; q.push_back({u, d + 1}); }
        }
    }
    std::vector<double> A((size_t)(max_hop + 1) * n * n, 0.0);
    for (int w = 0; w < n; ++w) {
        int cnt = 0;
        for (int v = 0; v < n; ++v) cnt += hop[v * n + w] <= max_hop;
        for (int v = 0; v < n; ++v) {
            const int h = hop[v * n + w];
            if (h <= max_hop) A[((size_t)h * n + v) * n + w] = 1.0 / (double)cnt;
        }
    }
    return A;
}

static bool make_skeleton(int layout, Skeleton& sk) {
    // net/graph.py:65-79,401-417 ('mocha'); :18-31,329-345 ('mixamo')
    static const int mocha_par[24] = {-1, 0, 1, 2, 3, 0, 5, 6, 7, 8, 9, 10, 11, 8, 13, 14, 8, 16, 17, 18, 0, 20, 21, 22};
    static const int mocha_part[24] = {0, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5};
    static const int mix_par[22] = {-1, 0, 1, 2, 3, 4, 3, 6, 7, 8, 3, 10, 11, 12, 0, 14, 15, 16, 0, 18, 19, 20};
    static const int mix_part[22] = {0, 0, 0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5};
    if (layout == 0) { sk.V = 24; sk.parents.assign(mocha_par, mocha_par + 24); sk.part_of.assign(mocha_part, mocha_part + 24); }
    else if (layout == 1) { sk.V = 22; sk.parents.assign(mix_par, mix_par + 22); sk.part_of.assign(mix_part, mix_part + 22); }
    else return false;
    sk.A_j = distance_adjacency(sk.parents, 2);
    sk.A_b = distance_adjacency({-1, 0, 0, 0, 0, 0}, 1);
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int v = 0; v < sk.V; ++v) cnt[sk.part_of[v]]++;
    sk.pool.assign((size_t)sk.V * 6, 0.0);
    sk.unpool.assign((size_t)6 * sk.V, 0.0);
    for (int v = 0; v < sk.V; ++v) {
        // the reference forms 1/|part| in float32 (net/graph.py:459-461): keep that rounding
        sk.pool[(size_t)v * 6 + sk.part_of[v]] = (double)(1.0f / (float)cnt[sk.part_of[v]]);
        sk.unpool[(size_t)sk.part_of[v] * sk.V + v] = 1.0;
    }
    return true;
}

// Scratch of workspace set k: the named workspaces of ensure_ws, the matchers' scratch (ensure_match_scratch, ensure_seg_scratch) and the
// two-plane fp16 engine's "output pointer -> its bound slot" notes
struct SetScratch {
    std::map<std::string, DeviceBuffer<float>> ws;
    DeviceBuffer<int32_t> idx_ws;                              // one index per window of the set: replaced with the workspaces (ensure_ws)
    DeviceBuffer<float> match_S{BUF_MOVES_GENERATION};         // the many-query GEMM's score slabs
    DeviceBuffer<float> match_qc{BUF_MOVES_GENERATION};        // queries minus the centroid
    DeviceBuffer<float> match_qstat{BUF_MOVES_GENERATION};     // row statistics of the round-4 selection (see select2 below)
    DeviceBuffer<unsigned long long> best_ws{BUF_MOVES_GENERATION};                    // the streaming scan's partial minima
    // every row's coarse key of 8 queries behind a head (slice winners, arrival tickets of mocha_match_refine) that starts at zero; the
    // tickets only ever count up
    DeviceBuffer<unsigned long long> scan_keys{BUF_MOVES_GENERATION | BUF_ZEROED};
    DeviceBuffer<unsigned> fold_tickets{BUF_MOVES_GENERATION | BUF_ZEROED};            // option "match_fold": arrival tickets per score tile
    // the segmented matcher's partial minima and plan for up to seg_q queries per launch (sized at mocha_bank_set_segments: the
    // segmented calls never allocate)
    DeviceBuffer<unsigned long long> seg_partial{BUF_MOVES_GENERATION};
    DeviceBuffer<int> seg_plan{BUF_MOVES_GENERATION};
    // the soft matcher's keys: every row's key of SEG_TOPK_Q queries against the largest segment (match_seg_topk.hip).  Reserved with the two
    // above and nowhere else, i.e. only by mocha_bank_set_segments, which moves the generation for the new bank anyway: BUF_PLAIN, so
    // that the generation counts what it counted before this buffer existed
    DeviceBuffer<unsigned long long> seg_keys;
    // the mixing matcher's scratch (match_seg_mix.hip) for 16 windows x 4 components: partial minima and plan of the 64 pseudo-queries,
    // effective ids / rows, normalised weights / distances, and 16 zero ids (the live mix step's push takes them: its gate is then "the
    // ring is full").  Reserved with seg_keys and nowhere else, BUF_PLAIN for the same reason
    DeviceBuffer<unsigned long long> mix_partial;
    DeviceBuffer<int> mix_plan;
    DeviceBuffer<int32_t> mix_i;
    DeviceBuffer<float> mix_f;
    DeviceBuffer<int32_t> mix_zero{BUF_ZEROED};
    const float* amax_enc_of = nullptr; float* amax_enc = nullptr;     // encoder output pointer -> its slot
    const float* amax_dec_of = nullptr; float* amax_dec = nullptr;     // decoder output pointer -> its slot
    const float* amax_tok_of = nullptr; float* amax_tok = nullptr;     // embedding output pointer -> its slot
};

// A character bank and everything mocha_bank_set derives from it.  The context keeps two: `bank`, the user's current bank, and `pair`,
// the transient bank of mocha_characterize_pair (centroid, row norms and plane image only).  None of these buffers moves the generation
// on its own: setting the current bank does.
struct Bank {
    const float* cnt = nullptr;                        // the rows matched against / the rows the decoder gathers: the caller's memory
    const float* enc = nullptr;                        // (MOCHA_BANK_BORROW, never freed here) or the owned copies below
    int64_t N = 0;
    DeviceBuffer<float> cnt_own, enc_own;
    bool is_bf16 = false;
    DeviceBuffer<float> norm;
    DeviceBuffer<float> center;                        // centroid of the bank (90*256), see do_match
    DeviceBuffer<unsigned short> bf16;                 // MOCHA_BANK_BF16: bf16(row - centroid)
    // the bf16 bank once more as the many-query coarse pass's own tiled image (contiguous 16 KB blocks), made at the first such match
    DeviceBuffer<unsigned short> tiled; bool tiled_valid = false;
    // match_pass = 2: mocha_match_pass256 reading the bank from its operand-order image (every wave-level load 1 KB contiguous), built at
    // the first such match (+ 2 B per bank value)
    DeviceBuffer<unsigned short> tile32; bool tile32_valid = false;
    // fp32 banks of up to X3_BANK_MAX rows also keep the plane engine's packed image of the centred bank (many-query matching)
    DeviceBuffer<unsigned short> x3; bool x3_valid = false;
    // fp32 banks of at least SCAN16_MIN rows also keep their centred bf16 copy and the rounding residual's norm per row: the
    // few-query matcher scans the copy (half the bytes) and re-ranks exactly what the rounding cannot exclude (match_stream.hip)
    DeviceBuffer<unsigned short> b16f; DeviceBuffer<float> rho; bool b16f_valid = false;
    // option "scan8" (default 0): the centred rows of an fp32 bank as biased bytes + per-row scale + residual bound - an adaptive 1 B / value first
    // stage of the few-query scan (match_scan8.hip); + N x 23 040 B
    DeviceBuffer<unsigned char> b8; DeviceBuffer<float> b8_scale, b8_rho; bool b8_valid = false;
    // Round 5: what the decoder derives from a bank ENTRY alone - IN(cha) (the folded decoder's keys, net/transformer.py:49-56) and every
    // layer's AdaIN gamma / beta (the style MLP of the entry's token mean, :98-107) - is computed once at mocha_bank_set, in float64 for
    // the MLP, and read through frame_index by the decoder (adain: gb_idx, attention: kv_idx) instead of being recomputed per step from
    // a gathered copy: + 92 KB + 4 KB per entry.  Option "bank_dec_cache" (0: recompute per call, the round-4 flow).
    DeviceBuffer<float> kin, gb; bool dec_valid = false;
    DeviceBuffer<float> amax; bool amax_ok = false;    // per entry: the largest magnitude of its encoded rows (two-plane fp16 engine)
    // multi-character bank (mocha_bank_set_segments): the rows as S segments, on the host and on the device; cleared by every other way
    // of setting the bank
    std::vector<int64_t> seg_start;                    // S + 1 entries; empty = no table
    int64_t seg_max_rows = 0;
    DeviceBuffer<int> seg_dev;
    // action labels of a multi-character bank's rows (mocha_bank_set_labels), cleared with the segment table: one byte per global row, the
    // OR of the label bits per segment (lab_any) and per 16 rows of a segment (lab_gran, segment s from word lab_gran_start[s]) - what the
    // action-constrained scans read (kernels.h, SegAllow)
    bool labelled = false;
    DeviceBuffer<unsigned char> lab_dev;
    DeviceBuffer<unsigned long long> lab_any, lab_gran;
    DeviceBuffer<int> lab_gran_start;
    // resident bank (mocha_bank_resident_create): N = the reserved capacity, owned rows, always labelled.  Characters live in `slot`s,
    // each an extent of whole granules handed out by `extents`; seg_dev then holds the slot table ({first row, rows} per slot, the
    // kernels' pair form), seg_start stays empty and seg_max_rows is the reserved maximum of rows per character.  add / retire rewrite
    // table entries in stream order; no pointer or launch shape a captured step bakes in changes while the bank is current.
    bool resident = false;
    struct Slot { int64_t first = 0, rows = 0; };      // rows = 0: empty
    std::vector<Slot> slot;                            // host mirror of the slot table
    ExtentAlloc extents;                               // units of SEG_GRANULE_ROWS rows
    // the online path's tables (mocha_bank_set_starts, mocha_bank_resident_set_starts): one bit per global row, "starts a clip", and
    // one epoch word per segment / slot, which add and retire bump.  They exist, zeroed, from mocha_bank_set_segments /
    // mocha_bank_resident_create on - calls that move the generation themselves - and are rewritten in stream order after that.
    DeviceBuffer<unsigned> start_bits, slot_epoch;
    DeviceBuffer<int32_t> start_list;                  // the uploaded list of a set_starts call

    bool segmented() const { return resident || !seg_start.empty(); }                 // the segmented calls serve this bank
    int segments() const { return resident ? (int)slot.size() : (int)seg_start.size() - 1; }
};

// The action constraint of a segmented call: per query a 64-bit allow mask (device) and, optionally, where the `applied` report goes.  A null
// AllowArg* is the plain call.
struct AllowArg {
    const unsigned long long* allow = nullptr;
    int32_t* applied = nullptr;
    AllowArg at(size_t q0) const { return AllowArg{allow + q0, applied ? applied + q0 : nullptr}; }
};

// The mix of a segmented call (match_seg_mix.hip): per window J component ids and J x 6 body-part weights (device), and where the (windows,
// J) local rows / distances and the (windows, J, 6) normalised weights go (each may be null).  gate / valid: the live steps' (per window).
struct MixArg {
    const int32_t* ids = nullptr;
    const float* weights = nullptr;
    int J = 0;
    int32_t* idx = nullptr;
    float* dist = nullptr;
    float* wnorm = nullptr;
    const int32_t* gate = nullptr;
    int32_t* valid = nullptr;
    MixArg at(size_t q0) const {
        return MixArg{ids + q0 * J, weights + q0 * J * 6, J, idx ? idx + q0 * J : nullptr, dist ? dist + q0 * J : nullptr,
                      wnorm ? wnorm + q0 * J * 6 : nullptr, gate ? gate + q0 : nullptr, valid ? valid + q0 : nullptr};
    }
};

// The online path of a segmented call (match_path_step.hip): window s of the call is stream s of the caller's state (streams = the call's
// windows, <= 16); the penalty by value; restart (device, one-shot words) and the per-stream outputs may be null.  dist_row (windows, ld):
// every distance of the step, for tests and tools.
struct PathStepArg {
    void* state = nullptr; int state_rows = 0; double lambda = 0.0;
    int32_t* restart = nullptr; float* dist = nullptr; unsigned char* continued = nullptr;
    float* dist_row = nullptr; int64_t ld = 0;
};

// The windows of a characterize: X (B windows, raw = with the root bone and un-normalised) -> Y
struct SegWindows {
    const float* X = nullptr; int B = 0; const float *cnt_mean = nullptr, *cnt_std = nullptr; float* Y = nullptr; bool raw = false;
};

// How a window of the segmented characterize gets its character feature (characterize_segmented_impl).  mix: the mixing matcher on mix->ids
// (`seg` unused).  Otherwise `seg` names the window's character, and k == 0 is the hard matcher (idx0: the local rows), k >= 1 the soft
// one (idx0: column 0, idx_k / w_k (B,k)); allow: its action constraint.  Every output may be null.
struct SegSelect {
    const int32_t* seg = nullptr;
    int k = 0; float temperature = 0.f;
    const AllowArg* allow = nullptr;
    const MixArg* mix = nullptr;
    const PathStepArg* path = nullptr;                 // the online path in the hard matcher's place (k == 0, no allow, no mix)
    int32_t *idx0 = nullptr, *idx_k = nullptr; float* w_k = nullptr;
    const int32_t* ids() const { return mix ? mix->ids : seg; }
    bool literal() const { return mix || k > 0; }      // the decoder runs on the blend in the "sel" workspace, not through the bank's rows
};

// The two configurations a captured live step carries by value, compared member by member (mocha_post_cfg has tail padding: no memcmp).
// A member added to either struct changes its size: the assertion then stops the build until the comparison next to it knows the member.
static_assert(sizeof(mocha_post_cfg) == 72, "mocha_post_cfg changed: update same_cfg(mocha_post_cfg) below, then this size");
bool same_cfg(const mocha_post_cfg& a, const mocha_post_cfg& b) {
    for (int i = 0; i < 4; ++i) if (a.contact_bones[i] != b.contact_bones[i]) return false;
    return a.dt == b.dt && a.ik_max_length_buffer == b.ik_max_length_buffer && a.ik_foot_height == b.ik_foot_height &&
           a.ik_unlock_radius == b.ik_unlock_radius && a.ik_blending_halflife == b.ik_blending_halflife &&
           a.ik_enabled == b.ik_enabled && a.n_contact == b.n_contact && a.blend_enabled == b.blend_enabled;
}
static_assert(sizeof(mocha_ingest_cfg) == 72, "mocha_ingest_cfg changed: update same_cfg(mocha_ingest_cfg) below, then this size");
bool same_cfg(const mocha_ingest_cfg& a, const mocha_ingest_cfg& b) {
    for (int i = 0; i < 3; ++i) if (a.euler_order[i] != b.euler_order[i]) return false;
    return a.lookahead == b.lookahead && a.rot_format == b.rot_format && a.unit_scale == b.unit_scale && a.fps == b.fps &&
           a.contact_velocity_threshold == b.contact_velocity_threshold && a.spine == b.spine && a.shoulder_l == b.shoulder_l &&
           a.shoulder_r == b.shoulder_r && a.upleg_l == b.upleg_l && a.upleg_r == b.upleg_r;
}

}  // namespace

struct mocha_ctx {
    mocha_cfg cfg{};
    int device = 0;
    std::string err;
    Skeleton sk;
    std::map<std::string, HostTensor> host_w;
    std::map<std::string, std::vector<int64_t>> expect;
    bool finalized = false;

    std::map<std::string, DeviceBuffer<float>> w;          // repacked device weights by short name (re-loading reuses the allocation)
    // Bumped whenever a device buffer that a captured graph may have baked in is replaced (workspaces, match scratch,
    // CVAE workspace) or the current bank changes: graph holders compare mocha_generation() before replaying.
    int64_t generation = 1;
    int ntok = 90, nT15 = 15, dim = 256, d4 = 64;

    // workspaces: sized for `chunk` windows; larger batches are processed chunk by chunk
    int chunk = 0;
    int max_chunk = 1280;
    // Two workspace sets: large batches are split in two halves that run on two HIP streams (the caller's and
    // `aux`), so that the prologue / epilogue / tail of one half's kernels overlaps the other half's MFMA phases
    // (+5..10 % measured); `cur` selects the set the pipelines below write to.
    static constexpr int MAX_SETS = 3;
    SetScratch sets[MAX_SETS];
    int cur = 0;
    // Lanes: up to three per-window steps in flight at once (mocha_step_graph_lane; BASELINE configs[4] pipelined).  Lane k
    // owns workspace set k (sets beyond the first are sized for a handful of windows unless dual_stream needs set 1 whole) and
    // its own captured graph; `lane` is the set the single-stream pipelines below write to.
    int lanes = 1, lane = 0;
    bool dual_stream = false; int dual_min = 128;     // opt-in: mocha_set_option(ctx, "dual_stream", 1) or MOCHA_DUAL_STREAM=1
    bool dual_ready = false;                          // ensure_ws allocated set 1 at full chunk size (a lane's set 1 holds 8 windows only)
    int attn_split_max = 192;                         // (window, head) pairs up to which the twelve-wave decoder attention is launched
    // folded decoder, larger batches: attention from pre-split key / value images (attention_kv.hip).  OFF by default: measured at the demo
    // step's 585 windows 197 us (twelve waves per window: three rounds of 256 workgroups) / 168 us (six waves per head pair) against 164 us
    // for mocha_attention_x3<256>, plus 18 us more in the instance norm that writes the images; it wins only where the windows fit one
    // round of CUs (256 windows: 75 against 89 us) - profiles/r04/b_attn_kv_ab.txt
    bool attn_kv = false;
    bool attn_kv_pairs = false;                       // ... with a six-wave workgroup per head pair instead of twelve waves per window (diagnostic)
    hipStream_t aux = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;

    Bank bank, pair;                                        // the user's current bank; the transient bank of mocha_characterize_pair
    DeviceBuffer<double> center_scratch;                    // fp64 partial column sums of launch_column_mean
    bool bank_dec_cache = true;                             // option "bank_dec_cache": see Bank::kin
    DeviceBuffer<double> style_scratch;                     // float64 token means + hidden activations of the style MLP, bank build
    // launch tuning, per context (round 4 kept these as process-wide globals: a second context, or another host thread, changed them underfoot)
    int inorm_split_max = 1 << 30, embed_max_wgs = 512, gemm_persistent = 768, gemm_persistent_max_n = 512; bool embed_sums = true;
    int gemm_x3r_min_n = 0;            // plane GEMM with the activations resident in registers (gemm_x3r.hip) for K = 256 launches at least this wide (0 = never); option "gemm_x3r_min_n"
    int gemm_tile64_below = 0;         // plane GEMM: 64 x 64 tiles for mid-size 128-multiple launches with fewer 64 x 128 tiles than this (measured: no gain; gemm_x3.hip)
    // Walk direction of the row-walking kernels of the batch path (option "walk"): 0 every launch walks its row blocks
    // upwards, 1 (default) the tensor-producing steps of a call alternate, so that a consumer meets its producer's newest rows first, 2 every
    // eligible launch walks downwards (tests).  walk_ord: eligible steps issued so far in this call (reset by every entry point and chunk):
    // a launch's direction is a pure function of the call's launch sequence, so a captured graph bakes in what an eager call does.
    int walk = 1, walk_ord = 0;
    bool pair_overlap = true;          // characterize_pair: the transient bank's decoder constants on the internal stream, beside the matching
    bool adain_closed = true;          // mocha_adain: qin from the first statistics in closed form (pointwise.hip); 0 = the literal two-pass order
    bool style_f64 = true;             // the style MLP in float64 (mocha_linear_f64); 0 = the fp32 GEMM engines
    std::map<std::string, DeviceBuffer<double>> w64;        // float64 copies of the style MLP's weights
    // CVAE sampler (row N1): weights under "cvae.<reference key>", workspace for cvae_B conditions
    std::map<std::string, std::vector<int64_t>> cvae_expect;
    std::map<std::string, HostTensor> cvae_host;
    std::map<std::string, DeviceBuffer<float>> cw;
    bool cvae_ready = false;
    int cvae_depth = 2, cvae_heads = 4, cvae_nc = 180, cvae_nq = 90;
    std::map<std::string, DeviceBuffer<float>> cws; int cvae_B = 0;
    // CVAE weight bank (mocha_cvae_bank_create): Cw slots of `slot_floats` floats, every tensor of cvae_expect at off[name] inside its
    // slot (so a grouped launch reads slot i's tensor `slot_floats` floats after slot i - 1's); the per-slot statistics (Cw,4,90,256),
    // the stored words, the shared positional table, 16 words of -1 (the warm pass's `which`) and the live step's per-stream slots.
    // None of these moves the generation on its own: creating the bank does, storing into it does not.
    struct CvaeBank {
        int Cw = 0;
        size_t slot_floats = 0;
        std::map<std::string, size_t> off;
        DeviceBuffer<float> w, stats, pe;
        DeviceBuffer<int32_t> stored, none, live_slot;
        std::vector<unsigned char> host_stored;            // as the host enqueued them
        std::vector<float> pe_host;
        float* pin = nullptr;                              // pinned staging of one slot's weights and statistics
        hipEvent_t ev = nullptr; bool ev_pending = false;  // the previous store's copies out of `pin`
    } cvb;
    // fp32 GEMMs on the bf16 matrix pipe (gemm_x3.hip): packed three-plane images of the weights, made on first use
    bool gemm_x3 = true;
    bool attn_x3 = true;               // the Generator's attention as plane products on the bf16 pipe (attention_x3.hip)
    std::map<std::tuple<const float*, int, int>, DeviceBuffer<unsigned short>> x3w;
    // fp32 GEMMs on the fp16 matrix pipe with two planes / three passes (gemm_h2.hip; option "gemm_f16x2", default off): packed images and
    // per-row inverse scales of the weights (made on first use), and the PER-WINDOW activation bounds the launches scale by: vectors of
    // AMAX_WIN floats in `amax` (entry w = window w of the chunk), AMAX_SLOTS per workspace set and stage (0 encoder, 1 decoder, 2 to_mot,
    // 3 embedding; a stage zeroes the slots it can take when it starts, so a later stage may read an earlier one's), `amax_ok` = the slot was
    // really written by a launch of that engine or by mocha_absmax (host-side bookkeeping)
    bool gemm_h2 = false;
    struct H2Img { DeviceBuffer<unsigned short> img; DeviceBuffer<float> w_inv; };
    std::map<std::tuple<const float*, int, int>, H2Img> h2w;
    static constexpr int AMAX_SLOTS = 40, AMAX_STAGES = 4;             // stages: 0 encoder, 1 decoder, 2 to_mot, 3 embedding
    static constexpr int AMAX_USED[4] = {2 + 4 * 8, 1 + 3 * 8, 5, 5};      // slots a stage can take (depth <= 8): what its start zeroes
    static constexpr int AMAX_WIN = 4096;                             // windows per chunk the bound vectors cover (larger chunks: the option stays off for them)
    DeviceBuffer<float> amax{BUF_ZEROED};                                          // MAX_SETS x AMAX_STAGES x AMAX_SLOTS vectors of AMAX_WIN floats, then amax_in
    std::vector<char> amax_ok = std::vector<char>(MAX_SETS * AMAX_STAGES * AMAX_SLOTS, 0);
    int amax_stage = 0, amax_next = 0; bool amax_idle = true;
    float* amax_in = nullptr;                                         // constant vector: the bound of an instance-normalised token, (n - 1) / sqrt(n) < 9.5 for 90 tokens
    float emb_l1 = 0.f, emb_bmax = 0.f;                               // largest row L1 norm / bias magnitude of the input 1x1 conv (model.py:44): |conv(x)| <= emb_l1 max|x| + emb_bmax
    bool fold_decoder = true;          // decoder key / value projections folded into the query / output weights
    int upsample_split_min = 256;      // windows from which that conv runs as two 2-tap launches (no zero weight blocks)
    bool fold_upsample = true;         // to_mot: the k=5 temporal conv over the x4-upsampled frames as a 3-tap conv over the SOURCE frames with per-phase summed weights
    bool fold_joint = true;            // embedding joint block: gcn 1x1 conv folded into the k=5 temporal conv (one K = 960 GEMM)
    DeviceBuffer<int> bone_parents;    // device: parents of the (V+1)-bone skeleton with the root bone in front
    DeviceBuffer<double> ingest_rows;  // device: the cubic fit rows of the mocap front end, (15,15) then (31,31) (ensure_ingest_rows)
    // device: the clip ingester's tables (offsets, mirror flags / window counts) and its float64 workspace (mocha_ingest_clips,
    // mocha_clip_windows).  Grow-only; only those two calls read it and neither is captured, so a new allocation does not move the generation.
    DeviceBuffer<double> clip_ws;
    // device: the BVH text parser's tables, report, slow-token list and per-block token counts (mocha_bvh_motion).  Grow-only; only that
    // call reads it and it is never captured, so a new allocation does not move the generation.
    DeviceBuffer<unsigned long long> bvh_ws;
    // device: the BVH text writer's report, clip byte offsets, uploaded tables and per-block byte counts (mocha_bvh_format).  Grow-only;
    // only that call reads it and it is never captured, so a new allocation does not move the generation.
    DeviceBuffer<unsigned long long> bvhw_ws;
    // device: coherent matching's scratch (mocha_match_path, mocha_characterize_path, mocha_characterize_pair_path) - the distance matrix
    // of the characterize forms, the row minima's columns, the continuation bits, the uploaded start lists and the bank starts' bit per
    // row.  Grow-only; batch calls that are never captured read it, so a new allocation does not move the generation.
    DeviceBuffer<float> path_d;
    DeviceBuffer<int32_t> path_m, path_lists;
    DeviceBuffer<unsigned short> path_cont;
    DeviceBuffer<unsigned> path_bits;
    DeviceBuffer<unsigned long long> path_keys;        // the matrix's all-keys scan: one key per entry
    DeviceBuffer<float> path_min;                      // a relative penalty's row minima
    DeviceBuffer<float> pose_norm;     // [x_mean | x_std | y_mean | y_std], (V+1)*C_in each (norm.npz of the reference)
    bool use_tiled = false;            // option "bank_tiled": -4 % on the cold pass for 2 x the bf16 copy's memory (profiles/r04/c_tiled_loader_ab.txt): off
    DeviceBuffer<unsigned long long> topk_keys{BUF_MOVES_GENERATION};      // every row's key of up to 8 queries (mocha_match_topk)
    bool scan16 = true;                // mocha_set_option("scan16", 0) scans the fp32 rows themselves (see Bank::b16f)
    bool match_fold = false;           // option "match_fold": the bf16 coarse pass's last K-slab workgroup per tile sums the slabs; the selection reads one (round 6 experiment)
    bool scan8 = false;                // see Bank::b8
    // many-query matching, round 4 (match_select2.hip): the producer of the centred queries hands over the row statistics of the selection's
    // error bound (match_qstat: ||q - c||^2 and the planes' residual per query), the bf16 coarse pass takes two query planes
    // Used for fp32 banks (demo pair 585 x 585: centre + select 44 us against 68; 128 x 4096: 23 against 30).  bf16 banks stay on
    // mocha_center_bf16 + one plane + mocha_match_select: with ONE query plane the bound admits ~8 rows for the unluckiest query and the
    // LDS-staged kernel re-evaluates them cheaper (128 x 4096: 81 us in all against 103); with TWO planes the selection drops to 15 us but the
    // coarse pass, whose ring then holds a third less of the bank in flight, rises from 39 to 60 us (85 in all; 1024 x 4096: 493 against 360) -
    // mocha_set_option("match_planes", 2) selects that variant (profiles/r04/c_select_ab.txt)
    bool select2 = true;
    int match_planes = 1;              // bf16 query planes of the many-query coarse pass against a bf16 bank
    // round 5: the one-plane coarse pass as mocha_match_pass256 (match_pass.hip: 256-row tiles, bank operands straight into registers) for
    // up to match_pass_max_q queries; 0 = round 4's mocha_match_gemm_bf16_dma.  match_pass_variant: launch_match_pass256's variant bits.
    int match_pass = 0, match_pass_variant = 0, match_pass_max_q = 256;
    // match_pass = 2: the pass reads the bank from Bank::tile32; match_nt: round 4's kernel with non-temporal bank loads
    int match_nt = 1;                  // applied to launches with ONE query tile (Q <= 128): the bank is then read exactly once per launch
    int seg_q = 0;                     // queries per launch of the segmented matcher (mocha_bank_set_segments)

    // captured per-window step (mocha_step_graph): one executable graph, re-captured when its key changes
    struct StepKey {
        const void *x = nullptr, *mean = nullptr, *sd = nullptr; void *y = nullptr, *idx = nullptr; const void* seg = nullptr;
        int windows = 1; bool raw = false;
        // mocha_live_step only: the session buffer, the new frame's arrays, the source's per-frame inputs, the outputs - and the
        // post-processing constants, which the captured launch carries by value
        const void* live[17] = {};
        mocha_post_cfg post{};
        // mocha_live_step_ours only: the state buffer, the four statistics, the caller's noise and the seeded output; the noise mode and seed
        const void* ours[7] = {};
        int noise = 0; unsigned long long seed = 0;
        // the soft steps only: neighbours, temperature, and the (windows, k) outputs idx_k / w_k
        int soft_k = 0; float soft_t = 0.f; const void* soft[2] = {};
        // mocha_live_step_inert only: the inertializer's state buffer and its two constants
        const void* inert = nullptr; double inert_halflife = 0.0, inert_dt = 0.0;
        // mocha_live_step_raw only: the front end's buffer and the raw frame's arrays; its configuration, which the captured launch carries by value
        const void* ingest[3] = {}; mocha_ingest_cfg icfg{};
        // the action-constrained steps only: the masks (read by every replay) and the applied report
        const void* allow[2] = {};
        // mocha_live_step_ours_grouped only: the characters' weight-bank slots (read by every replay)
        const void* cvae_of = nullptr;
        // the mix steps only: components per window, and the weights / normalised-weight pointers (the ids are `seg`, the (windows, J)
        // rows `idx`); ids and weights are read by every replay
        int mix_j = 0; const void* mix[2] = {};
        // the online-path steps only: the path state, the restart words and the dist / continued outputs; the state's rows and the penalty
        const void* path[4] = {}; int path_rows = 0; double path_lambda = 0.0;
        bool operator==(const StepKey& o) const {
            for (int i = 0; i < 4; ++i) if (path[i] != o.path[i]) return false;
            if (path_rows != o.path_rows || path_lambda != o.path_lambda) return false;
            if (mix_j != o.mix_j || mix[0] != o.mix[0] || mix[1] != o.mix[1]) return false;
            if (!(x == o.x && mean == o.mean && sd == o.sd && y == o.y && idx == o.idx && seg == o.seg && windows == o.windows && raw == o.raw))
                return false;
            for (int i = 0; i < 17; ++i) if (live[i] != o.live[i]) return false;
            for (int i = 0; i < 7; ++i) if (ours[i] != o.ours[i]) return false;
            if (noise != o.noise || seed != o.seed) return false;
            if (soft_k != o.soft_k || soft_t != o.soft_t || soft[0] != o.soft[0] || soft[1] != o.soft[1]) return false;
            if (allow[0] != o.allow[0] || allow[1] != o.allow[1]) return false;
            if (cvae_of != o.cvae_of) return false;
            if (inert != o.inert || inert_halflife != o.inert_halflife || inert_dt != o.inert_dt) return false;
            for (int i = 0; i < 3; ++i) if (ingest[i] != o.ingest[i]) return false;
            return same_cfg(icfg, o.icfg) && same_cfg(post, o.post);
        }
    };
    // One captured graph per kind of step: a lane's mocha_step_graph_lane (STEP_LANE + lane, workspace set `lane`), then the steps on
    // workspace set 0, each named after its entry point
    enum StepKind {
        STEP_LANE = 0,
        STEP_SEG = MAX_SETS, STEP_SEG_SOFT, STEP_SEG_MIX, STEP_SEG_ALLOW,                            // mocha_step_graph_[soft_|mix_]segmented[_allow]
        STEP_LIVE, STEP_LIVE_SOFT, STEP_LIVE_INERT,                                                  // mocha_live_step, _soft, _inert (hard or soft)
        STEP_LIVE_RAW, STEP_LIVE_RAW_SOFT, STEP_LIVE_RAW_INERT,                                      // mocha_live_step_raw: hard, soft, inertialized
        STEP_LIVE_ALLOW, STEP_LIVE_RAW_ALLOW, STEP_LIVE_MIX, STEP_LIVE_RAW_MIX,                      // mocha_live_step[_raw]_allow, mocha_live_step[_raw]_mix
        STEP_OURS, STEP_OURS_GROUPED,                                                                // mocha_live_step_ours[_grouped]
        STEP_LIVE_PATH, STEP_LIVE_RAW_PATH,                                                          // mocha_live_step_path, mocha_live_step_raw_path
        STEP_KINDS
    };
    struct StepGraph {
        hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr;
        StepKey key; int64_t generation = -1;
    } steps[STEP_KINDS];
    hipStream_t cap_stream = nullptr;                 // capture happens on this internal stream (the caller's may be the null stream)
    ncclComm_t comm = nullptr; int comm_rank = 0, comm_size = 1;      // mocha_comm_init
    DeviceBuffer<long long> bcast_hdr;                                  // device: {entries, bf16?} header of mocha_bank_broadcast

    // per-launch HIP-event profiling (mocha_profile_start/stop); off in normal operation
    struct ProfRec { std::string kernel, site; hipEvent_t e0, e1; double flops, bytes; };
    bool prof_on = false;
    std::vector<ProfRec> prof;
};

namespace {

// `g` replays for `key` as it is: no capture needed
bool step_holds(const mocha_ctx* c, const mocha_ctx::StepGraph& g, const mocha_ctx::StepKey& key) {
    return g.exec && g.key == key && g.generation == c->generation;
}

int fail(mocha_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                          \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fail((c), MOCHA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

// Room for `need` elements in a context buffer (grow-only, no-op when they fit: DeviceBuffer::reserve); a new allocation moves the
// generation where the buffer's declaration says so
template <class T>
int reserve(mocha_ctx* c, DeviceBuffer<T>& b, size_t need) {
    bool grew = false;
    HIPCHK(c, b.reserve(need, &grew));
    if (grew && (b.policy & BUF_MOVES_GENERATION)) c->generation++;
    return 0;
}

// host -> device copy of one named tensor; a re-load (second load_state_dict on the same context) reuses the
// existing allocation when the size is unchanged and frees it otherwise, so repeated loads do not leak
template <class T>
int upload_to(mocha_ctx* c, std::map<std::string, DeviceBuffer<T>>& tab, const std::string& name, const std::vector<T>& v) {
    DeviceBuffer<T>& d = tab[name];
    if (d.n != v.size()) d.release();
    int rc = reserve(c, d, v.size());
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}
int upload(mocha_ctx* c, const std::string& name, const std::vector<float>& v) { return upload_to(c, c->w, name, v); }

void build_expectations(mocha_ctx* c) {
    const mocha_cfg& g = c->cfg;
    const int64_t d = g.dim, d4 = g.dim / g.patch, cin = g.C_in, V = g.V;
    auto& e = c->expect;
    e["pos_emb"] = {1, (int64_t)c->ntok, d};
    e["mot_embedding.1.weight"] = {d4, cin, 1, 1};
    e["mot_embedding.1.bias"] = {d4};
    e["mot_embedding.2.blk.gcn.conv.weight"] = {3 * d, d4, 1, 1};
    e["mot_embedding.2.blk.gcn.conv.bias"] = {3 * d};
    e["mot_embedding.2.blk.tcn.weight"] = {d, d, 5, 1};
    e["mot_embedding.2.blk.tcn.bias"] = {d};
    e["mot_embedding.5.blk.gcn.conv.weight"] = {2 * d, d, 1, 1};
    e["mot_embedding.5.blk.gcn.conv.bias"] = {2 * d};
    e["mot_embedding.5.blk.tcn.weight"] = {d, d, 3, 1};
    e["mot_embedding.5.blk.tcn.bias"] = {d};
    for (int dec = 0; dec < 2; ++dec) {
        const char* nm = dec ? "decoder" : "encoder";
        const int depth = dec ? g.dec_depth : g.enc_depth;
        const int64_t inner = dec ? (int64_t)g.dec_heads * g.dec_dim_head : (int64_t)g.enc_heads * g.enc_dim_head;
        const int64_t mlp = dec ? g.dec_mlp : g.enc_mlp;
        for (int l = 0; l < depth; ++l) {
            std::string p = std::string(nm) + ".layers." + std::to_string(l);
            if (dec) {
                e[p + ".0.style.2.weight"] = {2 * d, d};
                e[p + ".0.style.2.bias"] = {2 * d};
                e[p + ".0.style.4.weight"] = {2 * d, 2 * d};
                e[p + ".0.style.4.bias"] = {2 * d};
            }
            e[p + ".1.to_q.1.weight"] = {inner, d};
            e[p + ".1.to_k.1.weight"] = {inner, d};
            e[p + ".1.to_v.weight"] = {inner, d};
            e[p + ".1.to_out.0.weight"] = {d, inner};
            e[p + ".1.to_out.0.bias"] = {d};
            e[p + ".2.net.0.weight"] = {mlp, d};
            e[p + ".2.net.0.bias"] = {mlp};
            e[p + ".2.net.3.weight"] = {d, mlp};
            e[p + ".2.net.3.bias"] = {d};
        }
    }
    e["to_mot.1.blk.gcn.conv.weight"] = {2 * d, d, 1, 1};
    e["to_mot.1.blk.gcn.conv.bias"] = {2 * d};
    e["to_mot.1.blk.tcn.weight"] = {d, d, 3, 1};
    e["to_mot.1.blk.tcn.bias"] = {d};
    e["to_mot.4.blk.gcn.conv.weight"] = {3 * d4, d, 1, 1};
    e["to_mot.4.blk.gcn.conv.bias"] = {3 * d4};
    e["to_mot.4.blk.tcn.weight"] = {d4, d4, 5, 1};
    e["to_mot.4.blk.tcn.bias"] = {d4};
    e["to_mot.6.weight"] = {cin, d4, 1, 1};
    e["to_mot.6.bias"] = {cin};
    (void)V;
}

// registered buffers of the reference state_dict: accepted and cross-checked, never used
bool is_graph_buffer(const std::string& n) {
    return n == "mot_embedding.2.A_j" || n == "to_mot.4.A_j" || n == "mot_embedding.5.A_b" || n == "to_mot.1.A_b" ||
           n == "mot_embedding.3.weight" || n == "to_mot.3.weight";
}

int check_graph_buffer(mocha_ctx* c, const std::string& n, const float* host, const int64_t* shape, int ndim) {
    const Skeleton& sk = c->sk;
    const std::vector<double>* ref = nullptr;
    std::vector<int64_t> shp;
    if (n.size() > 3 && n.compare(n.size() - 3, 3, "A_j") == 0) { ref = &sk.A_j; shp = {3, sk.V, sk.V}; }
    else if (n.size() > 3 && n.compare(n.size() - 3, 3, "A_b") == 0) { ref = &sk.A_b; shp = {2, 6, 6}; }
    else if (n == "mot_embedding.3.weight") { ref = &sk.pool; shp = {sk.V, 6}; }
    else { ref = &sk.unpool; shp = {6, sk.V}; }
    if ((int)shp.size() != ndim) return fail(c, MOCHA_ERR_WEIGHT, "%s: rank %d, expected %zu", n.c_str(), ndim, shp.size());
    for (int i = 0; i < ndim; ++i)
        if (shape[i] != shp[i]) return fail(c, MOCHA_ERR_WEIGHT, "%s: dim %d is %lld, expected %lld", n.c_str(), i, (long long)shape[i], (long long)shp[i]);
    for (size_t i = 0; i < ref->size(); ++i)
        if (std::fabs((double)host[i] - (*ref)[i]) > 1e-6)
            return fail(c, MOCHA_ERR_WEIGHT, "%s: graph constant differs from the regenerated one at %zu (%g vs %g)", n.c_str(), i, host[i], (*ref)[i]);
    return 0;
}

const std::vector<float>& W(mocha_ctx* c, const std::string& n) { return c->host_w.at(n).data; }

// [co][tap*Cin + ci] <- conv weight (Cout, Cin, taps, 1)
std::vector<float> repack_tcn(const std::vector<float>& w, int cout, int cin, int taps) {
    std::vector<float> o((size_t)cout * taps * cin);
    for (int co = 0; co < cout; ++co)
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < taps; ++t) o[((size_t)co * taps + t) * cin + ci] = w[((size_t)co * cin + ci) * taps + t];
    return o;
}
// adjacency-first form of SpatialConv (net/blocks.py:57-66): [co][k*Cin + ci] <- conv weight (K*Cout, Cin, 1, 1)
std::vector<float> repack_gcn_adjfirst(const std::vector<float>& w, int K, int cout, int cin) {
    std::vector<float> o((size_t)cout * K * cin);
    for (int k = 0; k < K; ++k)
        for (int co = 0; co < cout; ++co)
            for (int ci = 0; ci < cin; ++ci) o[(size_t)co * K * cin + (size_t)k * cin + ci] = w[((size_t)k * cout + co) * cin + ci];
    return o;
}

int ensure_ws(mocha_ctx* c, int B) {
    const int want = std::min(B, c->max_chunk);
    if (c->chunk >= want && c->chunk > 0) return 0;
    if (c->chunk > 0) HIPCHK(c, hipDeviceSynchronize());      // growing: earlier work may still read the old buffers
    // per-window float counts
    const int V = c->cfg.V;
    const size_t T = 90 * 256;
    const std::pair<const char*, size_t> plan[] = {
        {"hbar", 360 * 192}, {"ybar", 360 * 256}, {"u", 90 * 1280}, {"x5", T}, {"xA", 90 * 512}, {"t1", T}, {"xa", T}, {"xb", T},
        {"qkv", 90 * 3072}, {"ao", 90 * 1024}, {"hff", (size_t)90 * std::max(512, std::max(c->cfg.enc_mlp, c->cfg.dec_mlp))}, {"kin", T}, {"xad", T}, {"qin", T},
        {"smean", 256}, {"s1", 512 * 8}, {"gb", 512 * 8}, {"smean64", 512}, {"s1d", 512 * 8 * 2}, {"qc", T}, {"g", 90 * 192}, {"y2c", (size_t)15 * V * 64},
        {"z", (size_t)60 * V * 64}, {"enc_s", T}, {"enc_c", T}, {"qnm", T}, {"sel", T}, {"dec", T},
        // the decoder attention's pre-split key / value images (attention_kv.hip): 295 KB per window, planned only while option
        // "attention_kv" is on (setting it re-plans the workspaces)
        {"kvimg", c->attn_kv ? (size_t)ATTN_KV_IMG_BYTES / 4 : (size_t)4},
    };
    // free old workspaces
    for (SetScratch& st : c->sets) { st.ws.clear(); st.idx_ws.release(); }
    const bool dual_sets = c->dual_stream && want >= c->dual_min / 2;
    const int nsets = std::max(dual_sets ? 2 : 1, c->lanes);
    for (int set = 0; set < nsets; ++set) {
        // a lane's set serves per-window steps: a handful of windows; dual_stream's second set takes half of every large batch
        const int wset = (set == 0 || (set == 1 && dual_sets)) ? want : std::min(want, 8);
        int rc;
        for (auto& pl : plan)
            if ((rc = reserve(c, c->sets[set].ws[pl.first], pl.second * (size_t)wset))) return rc;
        if ((rc = reserve(c, c->sets[set].idx_ws, (size_t)wset))) return rc;
    }
    c->chunk = want;
    c->dual_ready = dual_sets;
    c->generation++;
    return 0;
}

SetScratch& SET(mocha_ctx* c) { return c->sets[c->cur]; }                // the workspace set the pipelines write to
float* WS(mocha_ctx* c, const char* n) { return SET(c).ws.at(n).p; }
InormExtra IEX(const mocha_ctx* c) { InormExtra e; e.split_max = c->inorm_split_max; return e; }     // the instance norm's extras with this context's launch tuning
float* DW(mocha_ctx* c, const std::string& n) { return c->w.at(n).p; }

// Every kernel launch goes through LAUNCH: error check, and when profiling is on a HIP event
// pair on the launch stream around it, tagged with the kernel symbol and the call site.
int prof_begin(mocha_ctx* c, hipStream_t s, const char* kernel, const char* site, double flops, double bytes) {
    mocha_ctx::ProfRec r{kernel, site, nullptr, nullptr, flops, bytes};
    HIPCHK(c, hipEventCreate(&r.e0));
    HIPCHK(c, hipEventCreate(&r.e1));
    HIPCHK(c, hipEventRecord(r.e0, s));
    c->prof.push_back(r);
    return 0;
}

#define LAUNCH(c, s, kernel, site, flops, bytes, expr)                                                       \
    do {                                                                                                     \
        if ((c)->prof_on) { int rc__ = prof_begin((c), (s), (kernel), (site), (flops), (bytes)); if (rc__) return rc__; } \
        hipError_t e__ = (expr);                                                                             \
        if (e__ != hipSuccess)                                                                               \
            return fail((c), MOCHA_ERR_HIP, "launch %s: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
        if ((c)->prof_on) HIPCHK((c), hipEventRecord((c)->prof.back().e1, (s)));                             \
    } while (0)

// Direction of the next eligible step on stream s (mocha_ctx::walk): 1 = its row blocks from the last to the first.  Launches on the
// internal stream walk upwards and do not count.  same_step: a second launch that produces the same tensor as the one before it
// (emb.front_sums' two clips, mot.tcn_joint's column halves) takes that launch's direction.
int walk_peek(const mocha_ctx* c, hipStream_t s, bool same_step = false) {
    if (c->walk == 0 || (c->aux && s == c->aux)) return 0;
    if (c->walk == 2) return 1;
    return (same_step ? c->walk_ord - 1 : c->walk_ord) & 1;
}
int walk_next(mocha_ctx* c, hipStream_t s, bool same_step = false) {
    const int r = walk_peek(c, s, same_step);
    if (!same_step && !(c->aux && s == c->aux)) c->walk_ord++;
    return r;
}
InormExtra IEXW(mocha_ctx* c, hipStream_t s) { InormExtra e = IEX(c); e.reverse = walk_next(c, s); return e; }     // IEX for a launch that is this call's next step

const char* gemm_kernel_name(const GemmParams& p) {
    if (gemm_is_skinny16(p)) return "mocha_gemm_skinny16";
    if (gemm_is_skinny(p)) return "mocha_gemm_skinny";
    if (gemm_is_small(p)) return "mocha_gemm_f32<64,2,2,1,1>";
    return gemm_is_narrow(p) ? "mocha_gemm_f32<64,4,1,1,2>" : "mocha_gemm_f32<128,2,2,2,2>";
}

// packed weight image of the bf16x3 engine for (W, N, K); made on first use (not while the stream is capturing: the caller
// then takes the exact-f32 kernel), dropped whenever weights are (re-)finalised
int x3_image(mocha_ctx* c, hipStream_t s, const GemmParams& p, const unsigned short** out) {
    *out = nullptr;
    const auto key = std::make_tuple(p.W, p.N, p.K);
    auto it = c->x3w.find(key);
    if (it != c->x3w.end()) { *out = it->second.p; return 0; }
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return 0;
    DeviceBuffer<unsigned short> d;
    int rc = reserve(c, d, gemm_x3_packed_elems(p.N, p.K));
    if (rc) return rc;
    HIPCHK(c, launch_pack_x3(p.W, p.N, p.K, d.p, s));
    HIPCHK(c, hipStreamSynchronize(s));             // once per weight: the image may be read from the other stream of a dual-stream step
    *out = c->x3w.emplace(key, std::move(d)).first->second.p;
    return 0;
}

// A graph captured after warm-up has the image pointers baked into its mocha_gemm_x3 nodes: dropping them is a buffer
// replacement like any other, so the generation moves and every holder re-captures.
void x3_drop_images(mocha_ctx* c) {
    if (!c->x3w.empty()) c->generation++;
    c->x3w.clear();
}

// packed two-plane fp16 image + per-row inverse scales of (W, N, K) for gemm_h2.hip; made on first use like x3_image
int h2_image(mocha_ctx* c, hipStream_t s, const GemmParams& p, const mocha_ctx::H2Img** out) {
    *out = nullptr;
    const auto key = std::make_tuple(p.W, p.N, p.K);
    auto it = c->h2w.find(key);
    if (it != c->h2w.end()) { *out = &it->second; return 0; }
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return 0;
    mocha_ctx::H2Img d;
    int rc = reserve(c, d.img, gemm_h2_packed_elems(p.N, p.K));
    if (!rc) rc = reserve(c, d.w_inv, (size_t)p.N);
    if (rc) return rc;
    HIPCHK(c, launch_pack_h2(p.W, p.N, p.K, d.img.p, d.w_inv.p, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *out = &c->h2w.emplace(key, std::move(d)).first->second;
    c->generation++;            // a step graph captured before this image existed took the three-plane kernels for this weight: its holder re-captures
    return 0;
}
void h2_drop_images(mocha_ctx* c) {
    if (!c->h2w.empty()) c->generation++;
    c->h2w.clear();
}
// activation bounds of the two-plane fp16 engine (see mocha_ctx::amax): a stage's slots are zeroed when the stage starts
int amax_alloc(mocha_ctx* c) {                                       // once, when the option is switched on (never inside a capture)
    if (c->amax.p) return 0;
    const size_t n = (size_t)mocha_ctx::MAX_SETS * mocha_ctx::AMAX_STAGES * mocha_ctx::AMAX_SLOTS;
    int rc = reserve(c, c->amax, (n + 1) * mocha_ctx::AMAX_WIN);       // (zeroed)
    if (rc) return rc;
    c->amax_in = c->amax.p + n * mocha_ctx::AMAX_WIN;
    const std::vector<float> k(mocha_ctx::AMAX_WIN, 9.5f);
    HIPCHK(c, hipMemcpy(c->amax_in, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
// b: windows of this chunk - up to 4 every GEMM of the path runs on the few-rows kernels (gemm_is_skinny), which neither read nor leave
// bounds: the stage then hands out no slots (no memset / absmax launches in the streamed per-window step)
int amax_begin(mocha_ctx* c, int stage, hipStream_t s, int b) {
    c->amax_idle = !c->gemm_h2 || !c->amax.p || b < 5 || b > mocha_ctx::AMAX_WIN;
    if (c->amax_idle) return 0;
    c->amax_stage = stage; c->amax_next = 0;
    const size_t base = ((size_t)c->cur * mocha_ctx::AMAX_STAGES + stage) * mocha_ctx::AMAX_SLOTS;
    std::fill(c->amax_ok.begin() + base, c->amax_ok.begin() + base + mocha_ctx::AMAX_SLOTS, 0);
    // the first b entries of every slot the stage can take: one strided memset
    HIPCHK(c, hipMemset2DAsync(c->amax.p + base * mocha_ctx::AMAX_WIN, mocha_ctx::AMAX_WIN * sizeof(float), 0, (size_t)b * sizeof(float),
                               (size_t)mocha_ctx::AMAX_USED[stage], s));
    return 0;
}
float* amax_slot(mocha_ctx* c) {                                      // a fresh (zero) bound vector of the current stage, or null when the engine is off
    if (c->amax_idle || !c->gemm_h2 || !c->amax.p || c->amax_next >= mocha_ctx::AMAX_USED[c->amax_stage]) return nullptr;
    return c->amax.p + (((size_t)c->cur * mocha_ctx::AMAX_STAGES + c->amax_stage) * mocha_ctx::AMAX_SLOTS + c->amax_next++) * mocha_ctx::AMAX_WIN;
}
ptrdiff_t amax_index(const mocha_ctx* c, const float* slot) {         // slot number inside the arena, or -1 (amax_in / foreign)
    if (!c->amax.p || !slot || slot < c->amax.p) return -1;
    const ptrdiff_t i = (slot - c->amax.p) / mocha_ctx::AMAX_WIN;
    return i < (ptrdiff_t)c->amax_ok.size() ? i : -1;
}
const float* amax_use(const mocha_ctx* c, const float* slot) {        // the bound if a launch wrote it (or it lies outside the arena: the caller checked), else null
    if (!c->gemm_h2 || !slot || !c->amax.p) return nullptr;
    const ptrdiff_t i = amax_index(c, slot);
    if (i >= 0) return c->amax_ok[i] ? slot : nullptr;
    return slot;
}
// *slot[w] = mul * max |window w of x| + add for the chunk's windows of `per` floats each (mocha_absmax)
int amax_measure(mocha_ctx* c, hipStream_t s, const float* x, int nwin, long long per, float** slot, float mul = 1.f, float add = 0.f) {
    *slot = amax_slot(c);
    if (!*slot) return 0;
    LAUNCH(c, s, "mocha_absmax", "h2.absmax", 0.0, 4.0 * nwin * per, launch_absmax(x, nwin, per, *slot, s, mul, add));
    c->amax_ok[amax_index(c, *slot)] = 1;
    return 0;
}

int gemm(mocha_ctx* c, hipStream_t s, const char* site, const GemmParams& p0, bool same_step = false) {
    GemmParams p = p0; p.tile64_below = c->gemm_tile64_below; p.persistent = c->gemm_persistent; p.persistent_max_n = c->gemm_persistent_max_n;
    if (p.rows_per_win <= 0) p.rows_per_win = 90;      // rows of a launch per window: 90 tokens unless the site says otherwise (to_mot's joint rows)
    if (c->gemm_h2 && p.a_amax && gemm_h2_supports(p)) {
        const mocha_ctx::H2Img* img = nullptr;
        int rc = h2_image(c, s, p, &img);
        if (rc) return rc;
        if (img) {
            GemmParams q = p; q.Wh2 = img->img.p; q.w_inv = img->w_inv.p;
            const double fl = 2.0 * p.M * (double)p.N * p.K;
            const double by = 4.0 * ((double)p.M * p.K / (p.gather ? p.ntaps : 1) * (p.R) + (double)p.N * p.K + (double)p.M * p.N + (p.residual ? (double)p.M * p.N : 0.0));
            LAUNCH(c, s, "mocha_gemm_h2", site, fl, by, launch_gemm_h2(q, s));
            { const ptrdiff_t i = amax_index(c, p.c_amax); if (i >= 0) c->amax_ok[i] = 1; }
            return 0;
        }
    }
    const double flops = 2.0 * p.M * (double)p.N * p.K;
    // algorithmic bytes: every operand once - activations, weights, the output, and the residual matrix where the epilogue adds one
    const double bytes = 4.0 * ((double)p.M * p.K / (p.gather ? p.ntaps : 1) * (p.R) + (double)p.N * p.K + (double)p.M * p.N * p.ksplit +
                                (p.residual ? (double)p.M * p.N : 0.0));
    if (c->gemm_x3 && gemm_x3_supports(p)) {
        const unsigned short* img = nullptr;
        int rc = x3_image(c, s, p, &img);
        if (rc) return rc;
        if (img) {
            GemmParams q = p; q.Wsplit = img;
            if (c->gemm_x3r_min_n > 0 && p.N >= c->gemm_x3r_min_n && gemm_x3r_supports(q)) {      // same bits, another schedule (gemm_x3r.hip)
                LAUNCH(c, s, "mocha_gemm_x3r", site, flops, bytes, launch_gemm_x3r(q, s));
                return 0;
            }
            q.reverse = walk_next(c, s, same_step);
            LAUNCH(c, s, "mocha_gemm_x3", site, flops, bytes, launch_gemm_x3(q, s));
            return 0;
        }
    }
    LAUNCH(c, s, gemm_kernel_name(p), site, flops, bytes, launch_gemm(p, s));
    return 0;
}
// the Generator's attention (90 tokens, head dim 128 / 256): plane products on the bf16 pipe unless switched off
const char* attn_kernel_name(const mocha_ctx* c, int DH, long long pairs = 1 << 30) {
    const bool x3 = c->attn_x3 && (DH == 128 || DH == 256);
    if (x3 && DH == 256 && pairs <= c->attn_split_max) return "mocha_attention_x3_split<256>";
    return x3 ? (DH == 128 ? "mocha_attention_x3<128>" : "mocha_attention_x3<256>")
              : (DH == 64 ? "mocha_attention_f32<64>" : DH == 128 ? "mocha_attention_f32<128>" : "mocha_attention_f32<256>");
}
hipError_t attention(mocha_ctx* c, const AttnParams& a0, hipStream_t s) {
    AttnParams a = a0; a.split_max = c->attn_split_max;
    if (!(c->attn_x3 && (a.dh == 128 || a.dh == 256) && a.nq <= 96 && a.nk <= 96)) return launch_attention(a, s);
    // the full-batch instance (more (window, head) pairs than CUs, not the twelve-wave variant) takes the walk direction
    const long long pairs = (long long)a.B * a.heads;
    if (pairs > 256 && !(a.dh == 256 && pairs <= a.split_max)) a.reverse = walk_next(c, s);
    return launch_attention_x3(a, s);
}
#define GEMM(c, s, site, p) do { int rc__ = gemm((c), (s), (site), (p)); if (rc__) return rc__; } while (0)
#define GEMM_SAME(c, s, site, p) do { int rc__ = gemm((c), (s), (site), (p), true); if (rc__) return rc__; } while (0)      // same step as the launch before

GemmParams plain(const float* A, int lda, const float* Wt, float* C, int ldc, int M, int N, int K) {
    GemmParams p;
    p.A = A; p.lda = lda; p.W = Wt; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
    return p;
}

// ---------------------------------------------------------------- stage pipelines on one chunk
// mot_embedding (model.py:42-50) for b windows: X -> tokens (b*90, 256)
// X2 / b2: an optional second clip whose windows follow the first one's in every workspace (pair step: both clips of a
// demo pair share the launches from the gcn conv on, so each launch has twice the tiles)
int run_embed(mocha_ctx* c, const float* X, int b, float* tokens, bool add_pos, hipStream_t s, bool raw = false,
              const float* X2 = nullptr, int b2 = 0) {
    const int V = c->cfg.V;
    const int nn = (V + 1) * c->cfg.C_in;
    if (raw && !c->pose_norm.p) return fail(c, MOCHA_ERR_STATE, "raw input needs mocha_set_pose_norm first");
    // two-plane fp16 engine (z-scored input, fused path): |u| <= |conv1(x)| <= emb_l1 max|x| + emb_bmax (LeakyReLU, the column-normalised
    // adjacency x pool mix and the 4-frame means do not raise a magnitude) - one pass over the poses gives the first launch's bound,
    // every GEMM's epilogue the next one's; the tokens' bound goes on to the encoder
    { int rc = amax_begin(c, 3, s, b + b2); if (rc) return rc; }
    float* u_amax = nullptr;
    SET(c).amax_tok_of = nullptr;
    if (c->gemm_h2 && !c->amax_idle && !raw && c->fold_joint && c->gemm_x3 && c->embed_sums && c->emb_l1 > 0.f && (u_amax = amax_slot(c))) {
        const long long per = 60ll * V * c->cfg.C_in;
        LAUNCH(c, s, "mocha_absmax", "h2.absmax", 0.0, 4.0 * b * per, launch_absmax(X, b, per, u_amax, s, c->emb_l1, c->emb_bmax));
        if (X2 && b2 > 0) LAUNCH(c, s, "mocha_absmax", "h2.absmax", 0.0, 4.0 * b2 * per, launch_absmax(X2, b2, per, u_amax + b, s, c->emb_l1, c->emb_bmax));
        c->amax_ok[amax_index(c, u_amax)] = 1;
    }
    float* x5_amax = nullptr;
    if (c->fold_joint && c->gemm_x3 && c->embed_sums) {
        // conv1 + lrelu + adjacency + joint->part pool, and the 4-frame sums of the five taps, in one kernel: the frame rows stay in LDS
        // the two clips' launches produce one tensor: one step of the walk; downwards, the second clip (the upper rows) is issued first
        const int rev = walk_next(c, s);
        const bool two = X2 && b2 > 0;
        for (int k = 0; k < (two ? 2 : 1); ++k) {
            const bool second = two && (k == 1) != (rev != 0);
            const float* Xk = second ? X2 : X;
            const int bk = second ? b2 : b;
            LAUNCH(c, s, "mocha_embed_sums_x3", "emb.front_sums", bk * 60.0 * V * 64 * (2.0 * 15 + 2.0 * 18) + bk * 90.0 * 960 * 4,
                   bk * 4.0 * (60.0 * V * 15 + 90.0 * 960),
                   launch_embed_sums(Xk, DW(c, "emb.W1"), DW(c, "emb.b1"), DW(c, "AP"), WS(c, "u") + (second ? (size_t)b * 90 * 960 : 0), bk, V, c->cfg.C_in,
                                     raw ? c->pose_norm.p : nullptr, raw ? c->pose_norm.p + nn : nullptr, raw ? 1 : 0, s, c->embed_max_wgs, rev));
        }
        if (two) b += b2;
        GemmParams gf = plain(WS(c, "u"), 960, DW(c, "emb.Wc"), WS(c, "x5"), 256, b * 90, 256, 960);
        gf.rowbias = DW(c, "emb.rbc"); gf.rb_mod = 6;
        gf.a_amax = amax_use(c, u_amax); gf.c_amax = x5_amax = amax_slot(c);
        GEMM(c, s, "emb.joint_block", gf);
    } else {
    // conv1 + lrelu + adjacency + joint->part pool (commuted)                  model.py:44-46
    const char* efk = c->gemm_x3 ? "mocha_embed_front_x3" : "mocha_embed_front";
    LAUNCH(c, s, efk, "emb.front", b * 60.0 * V * 64 * (2.0 * 15 + 2.0 * 18), b * 60.0 * (V * 15 + 6 * 192) * 4,
           launch_embed_front(X, DW(c, "emb.W1"), DW(c, "emb.b1"), DW(c, "AP"), WS(c, "hbar"), b * 60, V, c->cfg.C_in,
                              raw ? c->pose_norm.p : nullptr, raw ? c->pose_norm.p + nn : nullptr, raw ? 1 : 0, s, c->gemm_x3, c->embed_max_wgs));
    if (X2 && b2 > 0) {
        LAUNCH(c, s, efk, "emb.front", b2 * 60.0 * V * 64 * (2.0 * 15 + 2.0 * 18), b2 * 60.0 * (V * 15 + 6 * 192) * 4,
               launch_embed_front(X2, DW(c, "emb.W1"), DW(c, "emb.b1"), DW(c, "AP"), WS(c, "hbar") + (size_t)b * 360 * 192, b2 * 60, V,
                                  c->cfg.C_in, raw ? c->pose_norm.p : nullptr, raw ? c->pose_norm.p + nn : nullptr, raw ? 1 : 0, s, c->gemm_x3, c->embed_max_wgs));
        b += b2;
    }
    if (c->fold_joint) {
        // gcn conv folded into the temporal conv (mocha_finalize_weights: emb.Wc): the 4-frame sums of the five taps are taken on
        // the 192 adjacency-mixed channels and ONE GEMM, K = 5 x 192, does both convolutions and the AvgPool
        LAUNCH(c, s, "mocha_window_sums", "emb.window_sums", b * 90.0 * 960 * 4, b * 4.0 * (360.0 * 192 + 90.0 * 960),
               launch_window_sums(WS(c, "hbar"), WS(c, "u"), b * 90, 192, s));
        GemmParams gf = plain(WS(c, "u"), 960, DW(c, "emb.Wc"), WS(c, "x5"), 256, b * 90, 256, 960);
        gf.rowbias = DW(c, "emb.rbc"); gf.rb_mod = 6;
        GEMM(c, s, "emb.joint_block", gf);
    } else {
    // gcn 1x1 conv on the pooled operand: (b*360, 192) x (256,192)^T + pooled bias
    GemmParams g1 = plain(WS(c, "hbar"), 192, DW(c, "emb.Wg"), WS(c, "ybar"), 256, b * 360, 256, 192);
    g1.rowbias = DW(c, "emb.rbg"); g1.rb_mod = 6;
    GEMM(c, s, "emb.gcn_joint", g1);
    // temporal conv k=5 (reflect) fused with AvgPool2d((4,1)):  (b*90, 5*256) x (256, 1280)^T   blocks.py:112-118, model.py:47
    GemmParams g2 = plain(WS(c, "u"), 1280, DW(c, "emb.Wt"), WS(c, "x5"), 256, b * 90, 256, 1280);
    g2.bias = DW(c, "emb.bt");
    {
        LAUNCH(c, s, "mocha_window_sums", "emb.window_sums", b * 90.0 * 1280 * 4, b * 4.0 * (360.0 * 256 + 90.0 * 1280),
               launch_window_sums(WS(c, "ybar"), WS(c, "u"), b * 90, 256, s));
    }
    GEMM(c, s, "emb.tcn_joint_pool", g2);
    }
    }
    // body block                                                               model.py:48,137-162
    LAUNCH(c, s, "mocha_body_front", "emb.body_front", b * 90.0 * 512 * 12, b * 90.0 * (256 + 512) * 4, launch_body_front(WS(c, "x5"), DW(c, "A_b"), WS(c, "xA"), b * 15, s, walk_next(c, s)));
    GemmParams g3 = plain(WS(c, "xA"), 512, DW(c, "emb.Wgb"), WS(c, "t1"), 256, b * 90, 256, 512);
    g3.rowbias = DW(c, "emb.rbb"); g3.rb_mod = 6;
    g3.a_amax = amax_use(c, x5_amax); g3.c_amax = amax_slot(c);        // body_front: LeakyReLU + a column-normalised mix of x5
    GEMM(c, s, "emb.gcn_body", g3);
    GemmParams g4 = plain(WS(c, "t1"), 256, DW(c, "emb.Wtb"), tokens, 256, b * 90, 256, 768);
    g4.gather = 1; g4.T_out = 15; g4.V = 6; g4.ntaps = 3; g4.pad = 1; g4.stride = 1; g4.R = 1; g4.T_full = 15;
    g4.tshift = 0; g4.Cc = 256; g4.T_src = 15; g4.bias = DW(c, "emb.btb");
    if (add_pos) { g4.rowbias = DW(c, "pos_emb"); g4.rb_mod = 90; }           // model.py:88
    g4.a_amax = amax_use(c, g3.c_amax); g4.c_amax = amax_slot(c);
    GEMM(c, s, "emb.tcn_body", g4);
    if (amax_use(c, g4.c_amax)) { SET(c).amax_tok_of = tokens; SET(c).amax_tok = g4.c_amax; }
    return 0;
}

// one transformer layer's attention output projection + FF (net/transformer.py:91-94), shared by enc/dec
// ao_amax: per-window bounds on |ao| (device vector, two-plane fp16 engine) or null; *out_amax: the slot the last GEMM leaves the output's per-window maxima in
int run_out_ff(mocha_ctx* c, const std::string& p, const float* ao, int inner, const float* resid, int M, int mlp,
               float* out, hipStream_t s, const char* wo = ".Wo", const float* ao_amax = nullptr, float** out_amax = nullptr) {
    GemmParams o = plain(ao, inner, DW(c, p + wo), WS(c, "xb"), 256, M, 256, inner);
    o.bias = DW(c, p + ".bo"); o.residual = resid; o.ldr = 256;
    o.a_amax = amax_use(c, ao_amax); o.c_amax = amax_slot(c);
    GEMM(c, s, "xf.out_proj", o);
    GemmParams f1 = plain(WS(c, "xb"), 256, DW(c, p + ".W1"), WS(c, "hff"), mlp, M, mlp, 256);
    f1.bias = DW(c, p + ".b1"); f1.act = 1;
    f1.a_amax = amax_use(c, o.c_amax); f1.c_amax = amax_slot(c);
    GEMM(c, s, "xf.ff1", f1);
    GemmParams f2 = plain(WS(c, "hff"), mlp, DW(c, p + ".W2"), out, 256, M, 256, mlp);
    f2.bias = DW(c, p + ".b2"); f2.residual = WS(c, "xb"); f2.ldr = 256;
    f2.a_amax = amax_use(c, f1.c_amax); f2.c_amax = amax_slot(c);
    GEMM(c, s, "xf.ff2", f2);
    if (out_amax) *out_amax = f2.c_amax;
    return 0;
}

// encoder (model.py:53-59; net/transformer.py:90-95 with adain=False)
int run_encoder(mocha_ctx* c, const float* tokens, int b, float* encoded, hipStream_t s) {
    const int M = b * 90, H = c->cfg.enc_heads, DH = c->cfg.enc_dim_head, inner = H * DH;
    const float* x = tokens;
    // two-plane fp16 engine: every launch scales its activations by a bound on them - the tokens' largest magnitude is measured, every
    // GEMM's epilogue leaves its output's, and the attention's rows are convex combinations of value rows (a slice of qkv)
    int rc0 = amax_begin(c, 0, s, b); if (rc0) return rc0;
    float* x_amax = nullptr;
    if (c->gemm_h2 && !c->amax_idle) {
        if (tokens == SET(c).amax_tok_of && amax_use(c, SET(c).amax_tok)) x_amax = SET(c).amax_tok;      // the embedding's last GEMM left it
        else { rc0 = amax_measure(c, s, tokens, b, 90ll * 256, &x_amax); if (rc0) return rc0; }
    }
    SET(c).amax_enc_of = nullptr;
    for (int l = 0; l < c->cfg.enc_depth; ++l) {
        const std::string p = "enc" + std::to_string(l);
        GemmParams q = plain(x, 256, DW(c, p + ".Wqkv"), WS(c, "qkv"), 3 * inner, M, 3 * inner, 256);
        q.a_amax = amax_use(c, x_amax); q.c_amax = amax_slot(c);
        GEMM(c, s, "enc.qkv", q);
        AttnParams a{WS(c, "qkv"), WS(c, "qkv") + inner, WS(c, "qkv") + 2 * inner, WS(c, "ao"),
                     3 * inner, 3 * inner, 3 * inner, inner, b, H, DH, 90, 90, (float)std::pow((double)DH, -0.5)};
        LAUNCH(c, s, attn_kernel_name(c, DH), "enc.attn", 4.0 * b * H * 90.0 * 90 * DH,
               4.0 * M * 4 * inner, attention(c, a, s));
        float* out = (l == c->cfg.enc_depth - 1) ? encoded : WS(c, "xa");
        int rc = run_out_ff(c, p, WS(c, "ao"), inner, x, M, c->cfg.enc_mlp, out, s, ".Wo", q.c_amax, &x_amax);
        if (rc) return rc;
        x = out;
    }
    if (amax_use(c, x_amax)) { SET(c).amax_enc_of = encoded; SET(c).amax_enc = x_amax; }
    return 0;
}

// the style MLPs of every decoder layer in float64 (net/transformer.py:102-107): gb (rows, 512 L) = [gamma | beta] per layer, from the
// float64 token means; hidden = rows x 512 L doubles of scratch
// tiled: the tiled kernel whatever the row count (launch_linear_f64): a row's constants then do not depend on how many rows come with it
int run_style_f64(mocha_ctx* c, const double* mean64, double* hidden, float* gb, int rows, hipStream_t s, bool tiled = false) {
    const int L = c->cfg.dec_depth;
    LAUNCH(c, s, "mocha_linear_f64", "dec.style1", 2.0 * rows * 512.0 * L * 256, rows * 8.0 * (256 + 512 * L) + 8.0 * 512 * L * 256,
           launch_linear_f64(mean64, 256, 0, c->w64.at("dec.Ws1_all").p, c->w64.at("dec.bs1_all").p, hidden, nullptr, 512 * L, rows, 512 * L, 256, 1, 2, s,
                             tiled ? 1 : 0));
    LAUNCH(c, s, "mocha_linear_f64", "dec.style2", 2.0 * rows * 512.0 * L * 512, rows * (8.0 + 4.0) * 512 * L + 8.0 * L * 512 * 512,
           launch_linear_f64(hidden, 512 * L, 512, c->w64.at("dec.Ws2_all").p, c->w64.at("dec.bs2_all").p, nullptr, gb, 512 * L, rows, 512, 512, L, 0, s,
                             tiled ? 1 : 0));
    return 0;
}

// style MLPs of every layer at once for the b windows whose token means the instance norm left in the workspace ("smean" fp32,
// "smean64" float64): Linear 256->512, LeakyReLU, Linear 512->512 per layer -> "gb" (b, 512 L)          net/transformer.py:102-107
int run_style(mocha_ctx* c, int b, hipStream_t s) {
    const int L = c->cfg.dec_depth;
    if (c->style_f64)
        return run_style_f64(c, reinterpret_cast<const double*>(WS(c, "smean64")), reinterpret_cast<double*>(WS(c, "s1d")), WS(c, "gb"), b, s);
    GemmParams s1 = plain(WS(c, "smean"), 256, DW(c, "dec.Ws1_all"), WS(c, "s1"), 512 * L, b, 512 * L, 256);
    s1.bias = DW(c, "dec.bs1_all"); s1.act = 2;
    GEMM(c, s, "dec.style1", s1);
    if (b <= 192 || L == 1) {
        // a handful of windows: launch count matters, the block-diagonal matrix's zero half does not
        GemmParams s2 = plain(WS(c, "s1"), 512 * L, DW(c, "dec.Ws2_blk"), WS(c, "gb"), 512 * L, b, 512 * L, 512 * L);
        s2.bias = DW(c, "dec.bs2_all");
        GEMM(c, s, "dec.style2", s2);
    } else {
        for (int l = 0; l < L; ++l) {                     // large batches: layer l's 512 x 512 on its own slice of the hidden activations
            const std::string p = "dec" + std::to_string(l);
            GemmParams s2 = plain(WS(c, "s1") + (size_t)l * 512, 512 * L, DW(c, p + ".Ws2"), WS(c, "gb") + (size_t)l * 512, 512 * L, b, 512, 512);
            s2.bias = DW(c, p + ".bs2");
            GEMM(c, s, "dec.style2", s2);
        }
    }
    return 0;
}

// can the decoder read a bank entry's constants (IN(cha), gamma / beta) in place through frame_index?  (the folded decoder on the plane
// attention kernel; the image variant and the un-folded projections want contiguous per-window copies)
bool dec_cache_ok(const mocha_ctx* c) {
    return c->bank_dec_cache && c->style_f64 && c->fold_decoder && c->cfg.dec_dim_head == 256 && c->attn_x3 && !c->attn_kv;
}

// What the decoder derives from bank entries alone, for rows [0, N) of `enc`: kin = IN(entry) (the folded decoder's keys) and gb = every
// layer's AdaIN gamma / beta (float64 style MLP of the entry's float64 token mean).  mean64 / hidden: scratch for `cap` rows.
// tiled (a resident bank's add): the style MLP's tiled kernel however few rows these are - what a chunk of more than 16 rows gets here
int build_dec_consts(mocha_ctx* c, const float* enc, int64_t N, float* kin, float* gb, double* mean64, double* hidden, int64_t cap, hipStream_t s,
                     bool tiled = false) {
    const size_t D = 90 * 256;
    const int L = c->cfg.dec_depth;
    for (int64_t r0 = 0; r0 < N; r0 += cap) {
        const int rows = (int)std::min<int64_t>(cap, N - r0);
        InormExtra ex = IEXW(c, s); ex.mean64 = mean64;
        LAUNCH(c, s, "mocha_instnorm", "bank.in_cha", 0.0, rows * 90.0 * 256 * 4 * 2,
               launch_instnorm(enc + (size_t)r0 * D, kin + (size_t)r0 * D, nullptr, nullptr, nullptr, nullptr, rows, 90, s, &ex));
        int rc = run_style_f64(c, mean64, hidden, gb + (size_t)r0 * 512 * L, rows, s, tiled);
        if (rc) return rc;
    }
    return 0;
}

// decoder (model.py:62-68; net/transformer.py:90-121 with adain=True)
// gather_table / gather_idx: cha is cha_encoded[frame_index] (test_fullframework.py:298, 465).  With the bank's cached constants
// (kin_table = IN of every entry, gb_table = its gamma / beta: build_dec_consts) the decoder reads everything that depends on the matched
// entry IN PLACE through the indices - no instance norm of cha, no style MLP, no gathered copy; without them the first kernel gathers
// the rows itself, leaves the copy in the "sel" workspace (cha may then be null) and the constants are computed here.
int run_decoder(mocha_ctx* c, const float* src, const float* cha, int b, float* outp, hipStream_t s,
                const float* gather_table = nullptr, const int32_t* gather_idx = nullptr, long long gather_rows = 0,
                const float* kin_table = nullptr, const float* gb_table = nullptr) {
    const int M = b * 90, H = c->cfg.dec_heads, DH = c->cfg.dec_dim_head, inner = H * DH, L = c->cfg.dec_depth;
    const bool cached = gather_table && gather_idx && kin_table && gb_table && dec_cache_ok(c);
    // IN(cha) feeds every layer's keys; mean over tokens of cha feeds every layer's style MLP
    // Folded decoder at batch size: keys IN(cha) and values cha are the same for every head and layer - the instance norm writes them once
    // as pre-split bf16 plane images (InormExtra::kvimg) and every layer's attention reads those (attention_kv.hip); no fp32 copies
    const bool use_kv = c->fold_decoder && DH == 256 && c->attn_x3 && c->attn_kv && H >= 2 && H % 2 == 0 && (long long)b * H > c->attn_split_max;
    // two-plane fp16 engine: the attention's rows are convex combinations of the value rows - the matched bank entries (their largest
    // magnitude is taken at mocha_bank_set) or the character windows this call encoded; the query GEMM's operand is an instance-normalised
    // token (|z| <= (n - 1) / sqrt(n)); without a bound a launch stays on the bf16 planes
    { int rc = amax_begin(c, 1, s, b); if (rc) return rc; }
    const float* v_amax = nullptr;
    if (c->gemm_h2 && !c->amax_idle) {
        const float* vsrc = gather_table ? gather_table : cha;
        // per source window: its matched entry's bound (gathered through the indices), or the same window's character features
        const float* table = nullptr;
        if (vsrc && vsrc == c->bank.enc && c->bank.amax_ok) table = c->bank.amax.p;
        else if (vsrc && vsrc == SET(c).amax_enc_of) table = amax_use(c, SET(c).amax_enc);
        if (table && gather_table) {
            float* slot = amax_slot(c);
            if (slot) {
                LAUNCH(c, s, "mocha_gather_f32", "h2.gather", 0.0, 12.0 * b, launch_gather_f32(table, gather_idx, gather_rows, slot, b, s));
                c->amax_ok[amax_index(c, slot)] = 1;
                v_amax = slot;
            }
        } else if (table) v_amax = table + (cha - vsrc) / (90 * 256);          // cha = rows of the encoder's output: window for window
        else if (cha && !gather_table) {            // caller-supplied character features (mocha_decoder): measured
            float* slot = nullptr;
            int rc = amax_measure(c, s, cha, b, 90ll * 256, &slot); if (rc) return rc;
            v_amax = amax_use(c, slot);
        }
    }
    float* x_amax = nullptr;
    SET(c).amax_dec_of = nullptr;
    if (!cached) {
        InormExtra ex = IEXW(c, s);
        if (gather_table) { ex.table = gather_table; ex.row_idx = gather_idx; ex.table_rows = gather_rows; ex.copy_out = use_kv ? nullptr : WS(c, "sel"); }
        if (use_kv) ex.kvimg = reinterpret_cast<unsigned short*>(WS(c, "kvimg"));
        if (c->style_f64) ex.mean64 = reinterpret_cast<double*>(WS(c, "smean64"));
        const double wr = use_kv ? (double)ATTN_KV_IMG_BYTES * 90.0 / 96.0 : 90.0 * 256 * 4 * (gather_table ? 2 : 1);
        LAUNCH(c, s, "mocha_instnorm", "dec.in_cha", 0.0, b * (90.0 * 256 * 4 + wr),
               launch_instnorm(gather_table ? gather_table : cha, use_kv ? nullptr : WS(c, "kin"), WS(c, "smean"), nullptr, nullptr, nullptr, b, 90, s, &ex));
        if (gather_table) cha = use_kv ? nullptr : WS(c, "sel");
        int rc = run_style(c, b, s);
        if (rc) return rc;
    }
    const float* gbp = cached ? gb_table : WS(c, "gb");
    const float* x = src;
    float* qb = WS(c, "qkv");
    float* kb = qb + (size_t)M * inner;
    float* vb = kb + (size_t)M * inner;
    for (int l = 0; l < c->cfg.dec_depth; ++l) {
        const std::string p = "dec" + std::to_string(l);
        LAUNCH(c, s, "mocha_adain", "dec.adain", 0.0, b * 90.0 * 256 * 4 * 3,
               launch_adain(x, gbp + (size_t)l * 512, 512 * L, WS(c, "xad"), WS(c, "qin"), b, 90, s, c->adain_closed ? 1 : 0,
                            cached ? gather_idx : nullptr, gather_rows, c->inorm_split_max, walk_next(c, s)));
        if (c->fold_decoder && DH == 256) {
            // S_h = IN(x) (Wq_h^T Wk_h) IN(cha)^T and out = sum_h (P_h cha) (Wv_h^T Wo_h^T): with dim_head == dim the key and
            // value projections fold into the query and output weights (exact algebra, net/transformer.py:62-76), so the
            // attention reads IN(cha) / cha directly for every head and two of the four projection GEMMs disappear.
            GemmParams gq = plain(WS(c, "qin"), 256, DW(c, p + ".Wqk"), qb, inner, M, inner, 256);
            gq.a_amax = c->gemm_h2 && !c->amax_idle ? c->amax_in : nullptr;
            GEMM(c, s, "dec.q", gq);
            if (use_kv) {
                AttnKvParams a{qb, WS(c, "ao"), reinterpret_cast<const unsigned short*>(WS(c, "kvimg")), inner, inner, b, H, DH, 90, 90, (float)std::pow((double)DH, -0.5), c->attn_kv_pairs ? 1 : 0};
                LAUNCH(c, s, "mocha_attention_x3_kv<256>", "dec.attn", 4.0 * b * H * 90.0 * 90 * DH, 4.0 * M * 2 * inner + (double)b * ATTN_KV_IMG_BYTES,
                       launch_attention_x3_kv(a, s));
            } else {
            AttnParams a{qb, cached ? kin_table : WS(c, "kin"), cached ? gather_table : cha, WS(c, "ao"), inner, 256, 256, inner, b, H, DH, 90, 90, (float)std::pow((double)DH, -0.5), 0, 0};
            if (cached) { a.kv_idx = gather_idx; a.kv_rows = gather_rows; }      // keys / values of window b = the matched entry's rows, in place
            LAUNCH(c, s, attn_kernel_name(c, DH, (long long)b * H), "dec.attn", 4.0 * b * H * 90.0 * 90 * DH, 4.0 * M * (2 * inner + 2 * 256),
                   attention(c, a, s));
            }
            float* out = (l == c->cfg.dec_depth - 1) ? outp : WS(c, "xa");
            int rc = run_out_ff(c, p, WS(c, "ao"), inner, WS(c, "xad"), M, c->cfg.dec_mlp, out, s, ".Wvo", use_kv ? nullptr : v_amax, &x_amax);
            if (rc) return rc;
            if (l == c->cfg.dec_depth - 1 && amax_use(c, x_amax)) { SET(c).amax_dec_of = outp; SET(c).amax_dec = x_amax; }
            x = out;
            continue;
        }
        GemmParams gq = plain(WS(c, "qin"), 256, DW(c, p + ".Wq"), qb, inner, M, inner, 256);
        GEMM(c, s, "dec.q", gq);
        GemmParams gk = plain(WS(c, "kin"), 256, DW(c, p + ".Wk"), kb, inner, M, inner, 256);
        GEMM(c, s, "dec.k", gk);
        GemmParams gv = plain(cha, 256, DW(c, p + ".Wv"), vb, inner, M, inner, 256);
        GEMM(c, s, "dec.v", gv);
        AttnParams a{qb, kb, vb, WS(c, "ao"), inner, inner, inner, inner, b, H, DH, 90, 90, (float)std::pow((double)DH, -0.5)};
        LAUNCH(c, s, attn_kernel_name(c, DH, (long long)b * H), "dec.attn", 4.0 * b * H * 90.0 * 90 * DH,
               4.0 * M * 4 * inner, attention(c, a, s));
        float* out = (l == c->cfg.dec_depth - 1) ? outp : WS(c, "xa");
        int rc = run_out_ff(c, p, WS(c, "ao"), inner, WS(c, "xad"), M, c->cfg.dec_mlp, out, s);
        if (rc) return rc;
        x = out;
    }
    return 0;
}

// to_mot (model.py:71-80)
int run_to_mot(mocha_ctx* c, const float* tokens, int b, float* Y, hipStream_t s, bool denorm = false) {
    const int V = c->cfg.V, M = b * 90;
    const int nn = (V + 1) * c->cfg.C_in;
    if (denorm && !c->pose_norm.p) return fail(c, MOCHA_ERR_STATE, "de-normalised output needs mocha_set_pose_norm first");
    // two-plane fp16 engine: LeakyReLU and the column-normalised adjacency mixes (body_front, joint_expand: non-negative coefficients that sum
    // to at most one per output) do not raise the largest magnitude, so each GEMM's bound is its predecessor's output bound
    { int rc = amax_begin(c, 2, s, b); if (rc) return rc; }
    float* t_amax = nullptr;
    if (c->gemm_h2 && !c->amax_idle) {
        if (tokens == SET(c).amax_dec_of && amax_use(c, SET(c).amax_dec)) t_amax = SET(c).amax_dec;
        else { int rc = amax_measure(c, s, tokens, b, 90ll * 256, &t_amax); if (rc) return rc; }
    }
    LAUNCH(c, s, "mocha_body_front", "mot.body_front", b * 90.0 * 512 * 12, b * 90.0 * (256 + 512) * 4, launch_body_front(tokens, DW(c, "A_b"), WS(c, "xA"), b * 15, s, walk_next(c, s)));
    GemmParams g1 = plain(WS(c, "xA"), 512, DW(c, "mot.Wgb"), WS(c, "t1"), 256, M, 256, 512);
    g1.rowbias = DW(c, "mot.rbb"); g1.rb_mod = 6;
    g1.a_amax = amax_use(c, t_amax); g1.c_amax = amax_slot(c);
    GEMM(c, s, "mot.gcn_body", g1);
    GemmParams g2 = plain(WS(c, "t1"), 256, DW(c, "mot.Wtb"), WS(c, "x5"), 256, M, 256, 768);
    g2.gather = 1; g2.T_out = 15; g2.V = 6; g2.ntaps = 3; g2.pad = 1; g2.stride = 1; g2.R = 1; g2.T_full = 15;
    g2.tshift = 0; g2.Cc = 256; g2.T_src = 15; g2.bias = DW(c, "mot.btb");
    g2.a_amax = amax_use(c, g1.c_amax); g2.c_amax = amax_slot(c);
    GEMM(c, s, "mot.tcn_body", g2);
    // joint block gcn conv at body-part resolution (upsample + unpool only copy rows):  lrelu -> 256 -> 3*64
    GemmParams g3 = plain(WS(c, "x5"), 256, DW(c, "mot.Wg2"), WS(c, "g"), 192, M, 192, 256);
    g3.a_lrelu = 1; g3.bias = DW(c, "mot.bg2");
    g3.a_amax = amax_use(c, g2.c_amax); g3.c_amax = amax_slot(c);
    GEMM(c, s, "mot.gcn_joint", g3);
    LAUNCH(c, s, "mocha_joint_expand", "mot.joint_expand", b * 15.0 * V * 64 * 36, b * 15.0 * (6 * 192 + V * 64) * 4, launch_joint_expand(WS(c, "g"), DW(c, "AU"), WS(c, "y2c"), b * 15, V, s, walk_next(c, s)));
    // temporal conv k=5 over the x4-upsampled frames, read through the gather (t >> 2)
    if (c->fold_upsample) {
        // rows (window, source frame s, joint), columns (phase, channel): z[(b, s, v)][phase*64 + c] is the conv's output at frame 4 s + phase
        GemmParams g4 = plain(WS(c, "y2c"), 64, DW(c, "mot.Wt2p"), WS(c, "z"), 256, b * 15 * V, 256, 192);
        g4.gather = 1; g4.T_out = 15; g4.V = V; g4.ntaps = 3; g4.pad = 2; g4.stride = 4; g4.tstep = 4; g4.R = 1; g4.T_full = 60;
        g4.tshift = 2; g4.Cc = 64; g4.T_src = 15; g4.bias = DW(c, "mot.bt2p");
        g4.a_amax = amax_use(c, g3.c_amax); g4.rows_per_win = 15 * V;
        if (b >= c->upsample_split_min) {
            // large batches: two launches of two taps each instead of one with a third of its weight blocks zero
            GemmParams ga = g4; ga.W = DW(c, "mot.Wt2a"); ga.N = 128; ga.K = 128; ga.ntaps = 2;
            GemmParams gb = ga; gb.W = DW(c, "mot.Wt2b"); gb.C = WS(c, "z") + 128; gb.pad = -2; gb.bias = DW(c, "mot.bt2p") + 128;
            // the column halves produce one tensor: one step of the walk, issued in the opposite order when it runs downwards
            const bool rev = walk_peek(c, s) != 0;
            GEMM(c, s, "mot.tcn_joint", rev ? gb : ga);
            GEMM_SAME(c, s, "mot.tcn_joint", rev ? ga : gb);
        } else
        GEMM(c, s, "mot.tcn_joint", g4);
    } else {
    GemmParams g4 = plain(WS(c, "y2c"), 64, DW(c, "mot.Wt2"), WS(c, "z"), 64, b * 60 * V, 64, 320);
    g4.gather = 1; g4.T_out = 60; g4.V = V; g4.ntaps = 5; g4.pad = 2; g4.stride = 1; g4.R = 1; g4.T_full = 60;
    g4.tshift = 2; g4.Cc = 64; g4.T_src = 15; g4.bias = DW(c, "mot.bt2");
    GEMM(c, s, "mot.tcn_joint", g4);
    }
    LAUNCH(c, s, "mocha_final_proj", "mot.final_proj", b * 60.0 * V * 64 * 15 * 2, b * 60.0 * V * (64 + 15) * 4, launch_final_proj(WS(c, "z"), DW(c, "mot.W6"), DW(c, "mot.b6"), Y, b * 60 * V, c->cfg.C_in, V,
                             denorm ? c->pose_norm.p + 2 * nn : nullptr, denorm ? c->pose_norm.p + 3 * nn : nullptr, s, c->fold_upsample ? 1 : 0, walk_next(c, s)));
    return 0;
}

// Run fn(b0, b, stream) over the batch.  Small batches: chunk by chunk on the caller's stream.  Large ones: the two
// halves of the batch go to the caller's stream and to `aux` (forked / joined with events, capture-safe), each with its
// own workspace set, so two independent kernel chains are in flight and fill each other's bubbles.
template <class F>
int for_chunks(mocha_ctx* c, int B, hipStream_t s, F&& fn) {
    // set 1 must be a FULL-size set: with lanes >= 2 it exists at 8 windows whenever dual_sets was false at allocation
    const bool dual = c->dual_stream && B >= c->dual_min && c->dual_ready && !c->sets[1].ws.empty();
    if (!dual) {
        c->cur = c->lane;
        for (int b0 = 0; b0 < B; b0 += c->chunk) { c->walk_ord = 0; int rc = fn(b0, std::min(c->chunk, B - b0), s); if (rc) return rc; }      // (the walk order starts over with every chunk)
        return 0;
    }
    HIPCHK(c, hipEventRecord(c->ev_fork, s));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    const int h = (B + 1) / 2;
    int rc = 0;
    c->cur = 0;
    for (int b0 = 0; b0 < h && !rc; b0 += c->chunk) { c->walk_ord = 0; rc = fn(b0, std::min(c->chunk, h - b0), s); }
    c->cur = 1;
    for (int b0 = h; b0 < B && !rc; b0 += c->chunk) rc = fn(b0, std::min(c->chunk, B - b0), c->aux);
    c->cur = 0;
    // join even when a half failed: the caller's stream must not be left forked (an open capture would be invalidated)
    const hipError_t ej = hipEventRecord(c->ev_join, c->aux);
    const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(s, c->ev_join, 0) : ej;
    if (rc) return rc;
    HIPCHK(c, ew);
    return 0;
}

int ready(mocha_ctx* c, int B, bool entry = true) {
    if (!c) return MOCHA_ERR_ARG;
    if (entry) c->walk_ord = 0;                      // an entry point: the walk order starts over (mocha_ctx::walk)
    if (!c->finalized) return fail(c, MOCHA_ERR_STATE, "weights not finalised: call mocha_finalize_weights first");
    if (B < 0) return fail(c, MOCHA_ERR_ARG, "negative batch");
    HIPCHK(c, hipSetDevice(c->device));
    if (B > 0) return ensure_ws(c, B);
    return 0;
}

// required device pointers of a call with B > 0: a NULL must come back as an error code, not as a GPU fault that takes the host down
#define NEED_PTRS(c, B, what, ...)                                                                     \
    do {                                                                                               \
        if ((B) > 0) { const void* need__[] = {__VA_ARGS__}; for (const void* p__ : need__) if (!p__) return fail((c), MOCHA_ERR_ARG, what ": null argument"); } \
    } while (0)

// Nearest bank entry of every query (BallTree.query(k=1), test_fullframework.py:296,443).
// Precision: the rows of one character's bank sit close together far from the origin (||b||^2 ~ 1e5, gaps between the
// best candidates ~ 1e-2), so ||b||^2 - 2 q.b in fp32 cannot rank them.  Few queries: the HBM-bound scan evaluates
// sum (q-b)^2 directly.  Many queries: the GEMM runs on operands centred on the bank centroid c (distances are
// translation invariant; the centred norms are of the size of the distances themselves) and the arg-min re-ranks its
// four best candidates by their exact direct distances.
static constexpr int64_t SCAN16_MIN = 4096;        // rows from which an fp32 bank is scanned through its bf16 copy (few queries)
static constexpr int64_t X3_BANK_MAX = 4096;       // rows: the packed image of a 4096-row bank (BASELINE configs[2]) is 566 MB

// split of the many-query GEMM's K loop over gridDim.z so that a launch has about three tiles per CU
int match_ksplit(int Q, int64_t N) {
    const long long tiles = (long long)((Q + 127) / 128) * ((N + 127) / 128);
    return (int)std::min<long long>(16, std::max<long long>(1, (768 + tiles - 1) / tiles));
}

// windows workspace set `set` holds (ensure_ws): the chunk for set 0 and dual_stream's set 1, a handful for a lane's set
int set_windows(const mocha_ctx* c, int set) {
    return (set == 0 || (set == 1 && c->dual_ready)) ? std::max(c->chunk, 8) : 8;
}

// Scratch of do_match for up to Q queries against N bank rows, in workspace set `set`: centred queries, the streaming
// scan's partial minima, the GEMM's score slabs.  mocha_reserve and mocha_bank_set call it for the workspace chunk, so
// that a steady-state match never allocates (graph-capture safe); do_match itself calls it for exactly its Q.
int ensure_match_scratch(mocha_ctx* c, int set, int Q, const Bank& b, bool every_q_up_to) {
    const size_t D = 90 * 256;
    const int64_t N = b.N;
    SetScratch& st = c->sets[set];
    int rc;
    if ((rc = reserve(c, st.match_qc, (size_t)std::max(Q, 8) * D))) return rc;
    if ((rc = reserve(c, st.best_ws, match_stream_scratch(8, N)))) return rc;
    if (Q > 8) {
        size_t need = 0;
        for (int q = every_q_up_to ? 9 : Q; q <= Q; ++q)
            need = std::max(need, (size_t)std::max(match_ksplit(q, N), match_pass256_ksplit(q, N)) * q * (size_t)N);
        if ((rc = reserve(c, st.match_S, need))) return rc;
        if ((rc = reserve(c, st.match_qstat, (size_t)2 * QSTAT_PARTS * std::max(Q, 256)))) return rc;
        // option "match_fold": a ticket per 128 x 128 score tile of the bf16 coarse pass
        if (c->match_fold && b.is_bf16 && (rc = reserve(c, st.fold_tickets, (size_t)((Q + 127) / 128) * (size_t)((N + 127) / 128)))) return rc;
    }
    if (c->scan16 && !b.is_bf16 && N >= SCAN16_MIN && (rc = reserve(c, st.scan_keys, match_scan16_scratch_words(N)))) return rc;
    return 0;
}

// qc_pre: the queries minus the current bank's centroid, fp32, when the caller's producer already wrote them (mocha_instnorm's zc)
// (fp32; bf16 where the many-query pass against a bf16 bank wants them so: qc_pre_bf16, mocha_instnorm's zc16)
// the round-4 selection (match_select2.hip) serves this many queries against the current bank?
bool use_select2(const mocha_ctx* c, const Bank& b, int Q) { return c->select2 && Q > 8 && (!b.is_bf16 || c->match_planes == 2); }

// qstat_pre: with select2 and Q > 8, the producer also left the row statistics in match_qstat[set] (and, bf16: BOTH query planes in qc_pre)
int do_match(mocha_ctx* c, Bank& b, const float* qnm, int Q, int32_t* idx, float* dist, hipStream_t s, const void* qc_pre_any = nullptr,
             bool qc_pre_bf16 = false, bool qstat_pre = false) {
    if (!b.cnt || b.N <= 0) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    const int D = 90 * 256;
    const int64_t N = b.N;
    const int set = c->cur;
    SetScratch& st = c->sets[set];
    int rc;
    if ((rc = ensure_match_scratch(c, set, Q, b, false))) return rc;
    // centred queries: the bf16 bank holds bf16(b - c) and the GEMMs work on centred operands.  The many-query bf16 pass takes
    // them as bf16 (match_qc holds Q x D bf16 then), everything else as fp32.
    const bool via16 = Q <= 8 && !b.is_bf16 && b.b16f_valid && c->scan16 && st.scan_keys.n >= match_scan16_scratch_words(N);
    const bool need_qc = b.is_bf16 || Q > 8 || via16;
    // the many-query pass against a bf16 bank takes the centred queries as bf16, everything else as fp32: a precomputed copy of the
    // other kind is of no use (mocha_center_bf16 / mocha_sub_rows then make the right one)
    const bool sel2 = use_select2(c, b, Q);                       // many-query path with the round-4 selection: row statistics from the producer
    const float* qc_pre = (qc_pre_any && qc_pre_bf16 == (b.is_bf16 && Q > 8) && (!sel2 || qstat_pre)) ? static_cast<const float*>(qc_pre_any) : nullptr;
    if (need_qc && !qc_pre) {
        if (sel2 && b.is_bf16)
            LAUNCH(c, s, "mocha_center_rows", "match.center", 0.0, 8.0 * Q * D, launch_center_rows(qnm, b.center.p, st.match_qc.p, c->match_planes, nullptr, st.match_qstat.p, Q, D, s, walk_next(c, s)));
        else if (sel2)
            LAUNCH(c, s, "mocha_center_rows", "match.center", 0.0, 8.0 * Q * D, launch_center_rows(qnm, b.center.p, nullptr, 0, st.match_qc.p, st.match_qstat.p, Q, D, s, walk_next(c, s)));
        else if (b.is_bf16 && Q > 8)
            LAUNCH(c, s, "mocha_center_bf16", "match.center", 0.0, 6.0 * Q * D, launch_center_bf16(qnm, b.center.p, st.match_qc.p, Q, D, s));
        else
            LAUNCH(c, s, "mocha_sub_rows", "match.center", 0.0, 8.0 * Q * D, launch_sub_rows(qnm, b.center.p, st.match_qc.p, Q, D, s));
    }
    const float* qc = need_qc ? (qc_pre ? qc_pre : st.match_qc.p) : nullptr;
    if (via16) {
        // fp32 bank through its centred bf16 copy: every row's coarse distance from half the bytes, then the exact fp32 distances of
        // the rows the rounding bound cannot exclude - the result of the fp32 search
        if (c->scan8 && b.b8_valid && Q <= 4) {
            // the adaptive byte stage: 1 B per value while the queries sit close to a few rows, the bf16 scan otherwise (decided on the device)
            LAUNCH(c, s, "mocha_match_scan_adaptive+refine", "match.stream8", 3.0 * Q * N * D, (double)N * D * 1.0 + 4.0 * Q * D + 16.0 * Q * N,
                   launch_match_scan8(b.b8.p, b.b8_scale.p, b.b8_rho.p, b.b16f.p, b.rho.p, b.cnt, qc, qnm, Q, N, D, st.scan_keys.p, idx, dist, s));
            return 0;
        }
        LAUNCH(c, s, "mocha_match_stream<bf16>+refine", "match.stream16", 3.0 * Q * N * D,
               ((Q + 7) / 8) * (double)N * D * 2.0 + 4.0 * Q * D + 16.0 * Q * N,
               launch_match_scan16(b.b16f.p, b.rho.p, b.cnt, qc, qnm, Q, N, D, st.scan_keys.p, idx, dist, s));
        return 0;
    }
    if (Q <= 8) {
        const void* bank = b.is_bf16 ? (const void*)b.bf16.p : (const void*)b.cnt;
        const double passes = (Q + 7) / 8;
        LAUNCH(c, s, b.is_bf16 ? "mocha_match_stream<bf16>" : "mocha_match_stream<f32>", "match.stream", 3.0 * Q * N * D,
               passes * N * D * (b.is_bf16 ? 2.0 : 4.0) + 4.0 * Q * D,
               launch_match_stream(bank, b.is_bf16 ? 1 : 0, b.is_bf16 ? qc : qnm, Q, N, D, st.best_ws.p, idx, dist, s));
        return 0;
    }
    DeviceBuffer<float>& mS = st.match_S;
    if (b.is_bf16) {
        // bf16 bank: one bf16 plane of the centred queries against the centred bf16 bank; the select kernel re-evaluates every
        // row whose coarse score is within the query rounding's error bound of the best one - 2 ||dq|| (||b|| + ||b0||) with the query's
        // measured rounding residual dq, plus 5e-5 (2||q||^2 + ||b||^2 + ||b0||^2) of slack for the pass's fp32 accumulation - exactly
        // (fp32 centred query against the bf16 rows), so the result is the exact search over the rounded bank
        const int npl = sel2 ? c->match_planes : 1;
        const bool pass256 = c->match_pass && !c->use_tiled && Q <= c->match_pass_max_q;
        const int ksplit = pass256 ? match_pass256_ksplit(Q, N) : match_bf16_ksplit(Q, N);
        const void* tiled = nullptr;
        if (c->use_tiled && (size_t)N * D * 2 <= ((size_t)4 << 30)) {          // up to 4 GB of image (N = 93 k rows)
            const size_t need = match_tiled_elems(N, D);
            if (!b.tiled_valid) {
                if ((rc = reserve(c, b.tiled, need))) return rc;
                LAUNCH(c, s, "mocha_tile_bf16", "bank.tile", 0.0, 4.0 * N * D, launch_tile_bf16(b.bf16.p, b.tiled.p, N, D, s));
                b.tiled_valid = true;
            }
            tiled = b.tiled.p;
        }
        if (pass256) {
            const void* t32 = nullptr;
            if (c->match_pass == 2 && (size_t)N * D * 2 <= ((size_t)4 << 30)) {
                const size_t need = match_tile32_elems(N, D);
                if (!b.tile32_valid) {
                    if ((rc = reserve(c, b.tile32, need))) return rc;
                    LAUNCH(c, s, "mocha_tile32_bf16", "bank.tile32", 0.0, 4.0 * N * D, launch_tile32_bf16(b.bf16.p, b.tile32.p, N, D, s));
                    b.tile32_valid = true;
                }
                t32 = b.tile32.p;
            }
            LAUNCH(c, s, "mocha_match_pass256", "match.qk_bf16", 2.0 * npl * Q * (double)N * D, 2.0 * npl * Q * D + 2.0 * N * D + 4.0 * Q * N * ksplit,
                   launch_match_pass256(qc, b.bf16.p, mS.p, Q, N, D, ksplit, s, c->match_pass_variant, npl, t32));
        } else
        {
        unsigned* tk = (c->match_fold && ksplit > 1) ? st.fold_tickets.p : nullptr;      // (sized and zeroed by ensure_match_scratch)
        LAUNCH(c, s, "mocha_match_gemm_bf16", "match.qk_bf16", 2.0 * npl * Q * (double)N * D, 2.0 * npl * Q * D + 2.0 * N * D + 4.0 * Q * N * ksplit,
               launch_match_gemm_bf16(qc, b.bf16.p, mS.p, Q, N, D, ksplit, s, npl, tiled, (c->match_nt && Q <= 128) ? 1 : 0, tk));
        if (tk) {                                        // slab 0 holds the sum: the selection reads one slab
            if (sel2)
                LAUNCH(c, s, "mocha_match_select2", "match.select", 0.0, 4.0 * Q * N + 4.0 * N + 8.0 * Q,
                       launch_match_select2(mS.p, 1, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, nullptr, b.bf16.p,
                                            st.match_qstat.p, 5e-5f, Q, N, D, idx, dist, s));
            else
                LAUNCH(c, s, "mocha_match_select", "match.select", 0.0, 4.0 * Q * N + Q * (8.0 * D + 8 * 2.0 * D),
                       launch_match_select(mS.p, 1, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, nullptr, b.bf16.p, 5e-5f,
                                           Q, N, D, idx, dist, s));
            return 0;
        }
        }
        if (sel2)
            LAUNCH(c, s, "mocha_match_select2", "match.select", 0.0, 4.0 * ksplit * Q * N + 4.0 * N + 8.0 * Q,
                   launch_match_select2(mS.p, ksplit, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, nullptr, b.bf16.p,
                                        st.match_qstat.p, 5e-5f, Q, N, D, idx, dist, s));
        else
        LAUNCH(c, s, "mocha_match_select", "match.select", 0.0, 4.0 * ksplit * Q * N + Q * (8.0 * D + 8 * 2.0 * D),
               launch_match_select(mS.p, ksplit, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, nullptr, b.bf16.p, 5e-5f,
                                   Q, N, D, idx, dist, s));
        return 0;
    }
    const int ksplit = match_ksplit(Q, N);
    GemmParams g = plain(qc, D, b.cnt, mS.p, (int)N, Q, (int)N, D);
    g.ksplit = ksplit; g.slab_stride = (long long)Q * N;
    if (b.x3_valid && c->gemm_x3) {
        // the plane engine wants an even number of K steps in every slab: the largest split <= ksplit that divides 23040 / 32
        int kx = ksplit;
        while (kx > 1 && (D / 32) % kx != 0) --kx;
        g.ksplit = kx;
    }
    if (b.x3_valid && c->gemm_x3 && gemm_x3_supports(g)) {
        g.Wsplit = b.x3.p;                          // the centred bank as planes (bank_set_impl); same coarse-score accuracy as below
        g.persistent = c->gemm_persistent; g.persistent_max_n = c->gemm_persistent_max_n;
        LAUNCH(c, s, "mocha_gemm_x3", "match.qk", 2.0 * Q * (double)N * D, 4.0 * ((double)Q * D + (double)Q * N * g.ksplit) + 6.0 * N * D,
               launch_gemm_x3(g, s));
    } else {
        g.ksplit = ksplit;
        g.wsub = b.center.p;
        GEMM(c, s, "match.qk", g);
    }
    const int nslab = g.ksplit;
    // exact-f32 MFMA on centred operands: a coarse score is accurate to ~4e-7 (||q-c||^2 + ||b-c||^2); candidates within ten
    // times that of the best are re-evaluated in the direct form
    if (sel2)
        LAUNCH(c, s, "mocha_match_select2", "match.select", 0.0, 4.0 * nslab * Q * N + 4.0 * N + 8.0 * Q,
               launch_match_select2(mS.p, nslab, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, b.cnt, nullptr,
                                    st.match_qstat.p, 4e-6f, Q, N, D, idx, dist, s));
    else
    LAUNCH(c, s, "mocha_match_select", "match.select", 0.0, 4.0 * nslab * Q * N + Q * 16.0 * D,
           launch_match_select(mS.p, nslab, (long long)Q * N, (int)N, b.norm.p, qnm, b.center.p, b.cnt, nullptr, 4e-6f,
                               Q, N, D, idx, dist, s));
    return 0;
}

// Scratch of the segmented matcher in workspace set `set` for launches of up to c->seg_q queries against the current table (mocha_bank_set_segments
// sizes it for every set that exists, so that no segmented call allocates).  A resident bank: its two reserved maxima - rows per
// character, slots - stand where the largest segment and the segment count stand
int ensure_seg_scratch(mocha_ctx* c, int set) {
    const int S = c->bank.segments();
    int rc = reserve(c, c->sets[set].seg_partial, match_seg_scratch_words(c->seg_q, c->bank.seg_max_rows));
    if (!rc) rc = reserve(c, c->sets[set].seg_plan, seg_plan_ints(c->seg_q, S));
    if (!rc) rc = reserve(c, c->sets[set].seg_keys, match_seg_keys_words(c->bank.seg_max_rows));
    if (!rc) rc = reserve(c, c->sets[set].mix_partial, match_seg_scratch_words(SEG_MIX_Q * SEG_MIX_MAX_J, c->bank.seg_max_rows));
    if (!rc) rc = reserve(c, c->sets[set].mix_plan, seg_plan_ints(SEG_MIX_Q * SEG_MIX_MAX_J, S));
    if (!rc) rc = reserve(c, c->sets[set].mix_i, seg_mix_scratch_ints());
    if (!rc) rc = reserve(c, c->sets[set].mix_f, seg_mix_scratch_floats());
    if (!rc) rc = reserve(c, c->sets[set].mix_zero, (size_t)SEG_MIX_Q);
    return rc;
}

// The online path's tables of bank `b` (Bank::start_bits, slot_epoch) for N rows in S segments or slots, all zero: no row but a
// character's first starts a clip, every epoch 0.  Called where the bank is set, which moves the generation itself.
int path_tables_zeroed(mocha_ctx* c, Bank& b, int64_t N, int S, hipStream_t s) {
    const size_t words = (size_t)((N + 31) / 32);
    int rc = reserve(c, b.start_bits, words);
    if (!rc) rc = reserve(c, b.slot_epoch, (size_t)S);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(b.start_bits.p, 0, words * sizeof(unsigned), s));
    HIPCHK(c, hipMemsetAsync(b.slot_epoch.p, 0, (size_t)S * sizeof(unsigned), s));
    return 0;
}

// A call that searches or reads the bank's rows as ONE set: a resident bank has free extents and retired rows among them, and none of the
// union's derived data (centroid, norms, images) - it serves the segmented and live calls only
int refuse_resident(mocha_ctx* c, const char* who) {
    if (!c->bank.resident) return 0;
    return fail(c, MOCHA_ERR_STATE, "%s: the current bank is a resident bank (mocha_bank_resident_create), which is searched and read per character only", who);
}

// a segmented matcher finds its scratch missing in workspace set `set`
int no_seg_scratch(mocha_ctx* c, int set) {
    return fail(c, MOCHA_ERR_STATE, "workspace set %d has no segmented-match scratch: call %s after changing the workspaces", set,
                c->bank.resident ? "mocha_reserve" : "mocha_bank_set_segments");
}

// the kernels' view of a constraint: the caller's masks and report with the current bank's label tables
SegAllow seg_allow_of(mocha_ctx* c, const AllowArg& a) {
    return SegAllow{a.allow, c->bank.lab_dev.p, c->bank.lab_any.p, c->bank.lab_gran.p, c->bank.lab_gran_start.p, a.applied};
}

// Exact 1-NN of every query within its own segment (match_segmented.hip), in launches of up to c->seg_q queries.  q: the z-scored queries
// (fp32 bank) or the queries minus the union's centroid (bf16 bank).  idx: local rows (or null), gidx: global rows (or null).
// al: the action constraint (the ALLOW scan), or null
int seg_match(mocha_ctx* c, const float* q, int Q, const int32_t* seg, int32_t* idx, int32_t* gidx, float* dist, hipStream_t s,
              const AllowArg* al = nullptr) {
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (al && !c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    const int set = c->cur, S = c->bank.segments();
    const int D = 90 * 256;
    if (!c->sets[set].seg_partial.p || !c->sets[set].seg_plan.p) return no_seg_scratch(c, set);
    const void* bank = c->bank.is_bf16 ? (const void*)c->bank.bf16.p : (const void*)c->bank.cnt;
    for (int q0 = 0; q0 < Q; q0 += c->seg_q) {
        const int n = std::min(c->seg_q, Q - q0);
        SegAllow sa{};
        if (al) sa = seg_allow_of(c, al->at(q0));
        LAUNCH(c, s, c->bank.is_bf16 ? "mocha_match_seg_scan<bf16>" : "mocha_match_seg_scan<f32>", "match.segmented", 3.0 * n * c->bank.seg_max_rows * D,
               (double)n * c->bank.seg_max_rows * D * (c->bank.is_bf16 ? 2.0 : 4.0) + 4.0 * n * D,
               launch_match_segmented(bank, c->bank.is_bf16 ? 1 : 0, q + (size_t)q0 * D, seg + q0, n, c->bank.seg_dev.p, S, c->bank.seg_max_rows, D,
                                      c->sets[set].seg_partial.p, c->sets[set].seg_plan.p, idx ? idx + q0 : nullptr, gidx ? gidx + q0 : nullptr,
                                      dist ? dist + q0 : nullptr, s, al ? &sa : nullptr, c->bank.resident ? 1 : 0));
    }
    return 0;
}

// The k nearest rows of every query within its own segment, their softmax weights and the blend of their encoded rows (match_seg_topk.hip):
// q as for seg_match; idx0 (Q) / idx_k, dist_k, w_k (Q,k) / out (Q,90,256), each may be null.  One pass over the queries' segments per 16
// queries, through the key buffer of the current workspace set.
int seg_topk(mocha_ctx* c, const float* q, int Q, const int32_t* seg, int k, float temperature, int32_t* idx0, int32_t* idx_k, float* dist_k,
             float* w_k, float* out, hipStream_t s, const AllowArg* al = nullptr) {
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (al && !c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    SegAllow sa{};
    if (al) sa = seg_allow_of(c, *al);
    const int set = c->cur, S = c->bank.segments();
    const int D = 90 * 256;
    if (!c->sets[set].seg_keys.p || !c->sets[set].seg_plan.p) return no_seg_scratch(c, set);
    const bool b16 = c->bank.is_bf16;
    const void* bank = b16 ? (const void*)c->bank.bf16.p : (const void*)c->bank.cnt;
    const double passes = (Q + SEG_TOPK_Q - 1) / SEG_TOPK_Q;
    LAUNCH(c, s, b16 ? "mocha_match_seg_keys<bf16>" : "mocha_match_seg_keys<f32>", "match.soft", 3.0 * Q * c->bank.seg_max_rows * D + 2.0 * Q * k * D,
           passes * c->bank.seg_max_rows * D * (b16 ? 2.0 : 4.0) + 16.0 * Q * c->bank.seg_max_rows + Q * (k * (b16 ? 6.0 : 8.0) + 8.0) * D,
           launch_match_seg_topk(bank, b16 ? 1 : 0, q, seg, Q, c->bank.seg_dev.p, S, c->bank.seg_max_rows, D, c->sets[set].seg_keys.p,
                                 c->sets[set].seg_plan.p, c->bank.enc, k, temperature, idx0, idx_k, dist_k, w_k, out, s, al ? &sa : nullptr,
                                 c->bank.resident ? 1 : 0));
    return 0;
}

// what every online-path call checks of its numbers, nothing launched when they fail
int path_step_check(mocha_ctx* c, const char* who, int streams, int state_rows, double lambda) {
    if (streams < 1 || streams > PATH_STEP_MAX_STREAMS) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= streams <= %d", who, PATH_STEP_MAX_STREAMS);
    if (state_rows < 1 || state_rows > MATCH_PATH_MAX_ROWS) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= state_rows <= %d", who, MATCH_PATH_MAX_ROWS);
    if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(c, MOCHA_ERR_ARG, "%s: the jump penalty must be finite and >= 0", who);
    return 0;
}

// ... and of the bank, for the forms that read one
int path_step_bank(mocha_ctx* c, const char* who, int state_rows) {
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set_segments first");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (c->bank.seg_max_rows > state_rows)
        return fail(c, MOCHA_ERR_STATE, "%s: the bank's largest character has %lld rows, the path state holds %d", who, (long long)c->bank.seg_max_rows, state_rows);
    if (!c->bank.start_bits.p || !c->bank.slot_epoch.p) return fail(c, MOCHA_ERR_STATE, "%s: the bank has no start table", who);
    return 0;
}

// One step of the online path for Q <= 16 streams (match_path_step.hip): the plan and the all-keys scan of the bank's fp32 rows - the
// z-scored queries qnm, whatever the bank's flags - through the key buffer of the current workspace set, then the step kernel on the
// keys.  idx: local rows (or null), gidx: global rows for the decoder (or null).  Nothing allocates, copies from the host or synchronises.
// The caller ran path_step_check and path_step_bank.
int seg_path(mocha_ctx* c, const float* qnm, int Q, const int32_t* seg, const PathStepArg& p, int32_t* idx, int32_t* gidx, hipStream_t s) {
    const int set = c->cur, S = c->bank.segments();
    const int D = 90 * 256;
    if (!c->sets[set].seg_keys.p || !c->sets[set].seg_plan.p) return no_seg_scratch(c, set);
    LAUNCH(c, s, "mocha_match_seg_keys<f32>", "match.path_keys", 3.0 * Q * c->bank.seg_max_rows * D, (double)c->bank.seg_max_rows * D * 4.0 + 8.0 * Q * c->bank.seg_max_rows,
           launch_match_seg_keys(c->bank.cnt, qnm, seg, Q, c->bank.seg_dev.p, S, c->bank.seg_max_rows, D, c->sets[set].seg_keys.p, c->sets[set].seg_plan.p, s,
                                 c->bank.resident ? 1 : 0));
    PathStepArgs a{};
    a.state = p.state; a.streams = Q; a.state_rows = p.state_rows;
    a.ids = seg;
    a.seg_table = c->bank.seg_dev.p; a.S = S; a.pairs = c->bank.resident ? 1 : 0; a.epochs = c->bank.slot_epoch.p;
    a.start_bits = c->bank.start_bits.p; a.n_bits = c->bank.N;
    a.restart = p.restart; a.lambda = p.lambda;
    a.keys = c->sets[set].seg_keys.p; a.kstride = match_seg_key_stride(c->bank.seg_max_rows);
    a.idx = idx; a.gidx = gidx; a.dist_out = p.dist; a.continued = p.continued; a.dist_row = p.dist_row; a.ld_row = p.ld;
    LAUNCH(c, s, "mocha_match_path_step", "match.path_step", 3.0 * Q * c->bank.seg_max_rows, 24.0 * Q * c->bank.seg_max_rows, launch_match_path_step(a, s));
    return 0;
}

// The mixing matcher (match_seg_mix.hip): every window's present components matched in their own characters, the weights normalised per
// body part, and out (Q,90,256, or null) = the part-wise blend of the matched entries' encoded rows.  q as for seg_match.  The windows
// are walked SEG_MIX_Q at a time through the mix scratch of the current workspace set; nothing allocates or synchronises.
int seg_mix(mocha_ctx* c, const float* q, int Q, const MixArg& mx, float* out, hipStream_t s) {
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    const int set = c->cur, S = c->bank.segments();
    const int D = 90 * 256;
    SetScratch& st = c->sets[set];
    if (!st.mix_partial.p || !st.mix_plan.p || !st.mix_i.p || !st.mix_f.p) return no_seg_scratch(c, set);
    const bool b16 = c->bank.is_bf16;
    const void* bank = b16 ? (const void*)c->bank.bf16.p : (const void*)c->bank.cnt;
    for (int q0 = 0; q0 < Q; q0 += SEG_MIX_Q) {
        const int n = std::min(SEG_MIX_Q, Q - q0);
        const MixArg m = mx.at((size_t)q0);
        LAUNCH(c, s, b16 ? "mocha_match_seg_scan_mix<bf16>" : "mocha_match_seg_scan_mix<f32>", "match.mix", 3.0 * n * m.J * c->bank.seg_max_rows * D,
               (double)n * m.J * c->bank.seg_max_rows * D * (b16 ? 2.0 : 4.0) + 4.0 * n * (m.J + 2.0) * D,
               launch_match_seg_mix(bank, b16 ? 1 : 0, q + (size_t)q0 * D, m.ids, m.weights, n, m.J, c->bank.seg_dev.p, S, c->bank.seg_max_rows, D,
                                    st.mix_partial.p, st.mix_plan.p, st.mix_i.p, st.mix_f.p, c->bank.enc, m.gate, m.valid, m.idx, m.dist, m.wnorm,
                                    out ? out + (size_t)q0 * D : nullptr, s, c->bank.resident ? 1 : 0));
    }
    return 0;
}

// fn(q, q0, n) over the Q z-scored queries of a mocha_match_*segmented* call, on workspace set 0, as the matchers above read them: an fp32
// bank takes them as they are, in one piece; the bf16 copy holds bf16(b - centroid of the union), so its queries are centred, as many at
// a time as the centred-query buffer holds
template <class F>
int for_centred_queries(mocha_ctx* c, const float* query_nm, int Q, hipStream_t s, F&& fn) {
    const int D = 90 * 256;
    c->cur = 0;
    if (!c->bank.is_bf16) return fn(query_nm, 0, Q);
    const int per = (int)std::min<size_t>((size_t)c->seg_q, c->sets[0].match_qc.n / D);
    for (int q0 = 0; q0 < Q; q0 += per) {
        const int n = std::min(per, Q - q0);
        LAUNCH(c, s, "mocha_sub_rows", "match.center", 0.0, 8.0 * n * D, launch_sub_rows(query_nm + (size_t)q0 * D, c->bank.center.p, c->sets[0].match_qc.p, n, D, s));
        const int rc = fn(c->sets[0].match_qc.p, q0, n);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

// =========================================================================================== C ABI
extern "C" {

int mocha_abi_version(void) { return 6; }

#define MOCHA_STR2(x) #x
#define MOCHA_STR(x) MOCHA_STR2(x)
const char* mocha_build_info(void) {
    return "hipcc HIP " MOCHA_STR(HIP_VERSION_MAJOR) "." MOCHA_STR(HIP_VERSION_MINOR) "." MOCHA_STR(HIP_VERSION_PATCH) "-" HIP_VERSION_GITHASH " gfx950";
}
int mocha_runtime_version(void) {
    int v = 0;
    return hipRuntimeGetVersion(&v) == hipSuccess ? v : -1;
}

int64_t mocha_generation(const mocha_ctx* c) { return c ? c->generation : 0; }

const char* mocha_last_error(const mocha_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int mocha_create(const mocha_cfg* cfg, int device, mocha_ctx** out) {
    if (!cfg || !out) return fail(nullptr, MOCHA_ERR_ARG, "null argument");
    *out = nullptr;
    // the kernels are specialised for the shipped architecture (configs/config.yaml:13-31)
    if (cfg->T != 60 || cfg->patch != 4 || cfg->dim != 256 || cfg->C_in != 15)
        return fail(nullptr, MOCHA_ERR_ARG, "unsupported T/patch/dim/C_in (%d/%d/%d/%d), need 60/4/256/15", cfg->T, cfg->patch, cfg->dim, cfg->C_in);
    // head dims: 64 (the reference Attention's own default, net/transformer.py:38: exact-f32 MFMA attention), 128 and 256 (also the plane engine)
    for (int dh : {cfg->enc_dim_head, cfg->dec_dim_head})
        if (dh != 64 && dh != 128 && dh != 256) return fail(nullptr, MOCHA_ERR_ARG, "dim_head must be 64, 128 or 256 (got %d)", dh);
    if (cfg->enc_heads * cfg->enc_dim_head > 1024 || cfg->dec_heads * cfg->dec_dim_head > 1024 || cfg->enc_heads < 1 || cfg->dec_heads < 1)
        return fail(nullptr, MOCHA_ERR_ARG, "heads*dim_head must be in [64, 1024]");
    for (int mlp : {cfg->enc_mlp, cfg->dec_mlp})
        if (mlp < 64 || mlp > 2048 || mlp % 64) return fail(nullptr, MOCHA_ERR_ARG, "mlp_dim must be a multiple of 64 in [64, 2048] (got %d)", mlp);
    if (cfg->enc_depth < 1 || cfg->enc_depth > 8 || cfg->dec_depth < 1 || cfg->dec_depth > 8) return fail(nullptr, MOCHA_ERR_ARG, "depth must be in [1, 8]");
    mocha_ctx* c = new mocha_ctx();
    c->cfg = *cfg; c->device = device;
    if (!make_skeleton(cfg->layout, c->sk) || c->sk.V != cfg->V) {
        int v = c->sk.V; delete c;
        return fail(nullptr, MOCHA_ERR_ARG, "layout %d has %d joints, cfg.V = %d (0 = mocha/24, 1 = mixamo/22)", cfg->layout, v, cfg->V);
    }
    build_expectations(c);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = gemm_init();
    if (e == hipSuccess) e = gemm_x3_init();
    if (e == hipSuccess) e = gemm_h2_init();
    if (e == hipSuccess) e = gemm_x3r_init();
    if (e == hipSuccess) e = match_scan8_init();
    if (e == hipSuccess) e = attention_x3_init();
    if (e == hipSuccess) e = match_mfma_init();
    if (e == hipSuccess) e = match_refine_init();
    if (e == hipSuccess) e = featurize_init();
    if (e == hipSuccess) e = live_init();
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
    if (e != hipSuccess) { delete c; return fail(nullptr, MOCHA_ERR_HIP, "device %d init failed: %s", device, hipGetErrorString(e)); }
    *out = c;
    return 0;
}

void mocha_destroy(mocha_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->aux) (void)hipStreamDestroy(c->aux);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    for (auto& g : c->steps) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    if (c->cvb.ev) { (void)hipEventSynchronize(c->cvb.ev); (void)hipEventDestroy(c->cvb.ev); }
    if (c->cvb.pin) (void)hipHostFree(c->cvb.pin);
    (void)mocha_comm_destroy(c);
    delete c;                                             // every device buffer is a DeviceBuffer member: freed here
}

int mocha_load_weight(mocha_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!c || !name || !host || !shape) return fail(c, MOCHA_ERR_ARG, "null argument");
    const std::string n(name);
    if (is_graph_buffer(n)) return check_graph_buffer(c, n, host, shape, ndim);
    auto it = c->expect.find(n);
    if (it == c->expect.end()) return fail(c, MOCHA_ERR_WEIGHT, "unknown weight name '%s'", name);
    if ((int)it->second.size() != ndim) return fail(c, MOCHA_ERR_WEIGHT, "%s: rank %d, expected %zu", name, ndim, it->second.size());
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != it->second[i]) return fail(c, MOCHA_ERR_WEIGHT, "%s: dim %d is %lld, expected %lld", name, i, (long long)shape[i], (long long)it->second[i]);
        cnt *= (size_t)shape[i];
    }
    HostTensor t; t.data.assign(host, host + cnt); t.shape.assign(shape, shape + ndim);
    c->host_w[n] = std::move(t);
    c->finalized = false;
    return 0;
}

int mocha_finalize_weights(mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    for (auto& kv : c->expect)
        if (!c->host_w.count(kv.first)) return fail(c, MOCHA_ERR_STATE, "missing weight '%s'", kv.first.c_str());
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    x3_drop_images(c);                              // re-loaded weights keep their device addresses
    h2_drop_images(c);
    const Skeleton& sk = c->sk;
    const int V = sk.V;
    int rc = 0;
    auto up = [&](const std::string& n, const std::vector<float>& v) { if (!rc) rc = upload(c, n, v); };
    auto f32 = [](const std::vector<double>& v) { return std::vector<float>(v.begin(), v.end()); };

    // ---- graph operators
    // AP[k][v][p] = sum_w A_j[k][v][w] pool[w][p]   (adjacency then joint->part mean, graph.py:463-465)
    std::vector<double> AP((size_t)3 * V * 6, 0.0), APsum(3 * 6, 0.0);
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < V; ++v)
            for (int p = 0; p < 6; ++p) {
                double a = 0;
                for (int w = 0; w < V; ++w) a += (double)(float)sk.A_j[((size_t)k * V + v) * V + w] * sk.pool[(size_t)w * 6 + p];
                AP[((size_t)k * V + v) * 6 + p] = a;
                APsum[k * 6 + p] += a;
            }
    up("AP", f32(AP));
    // AU[k][p][w] = sum_{v in part p} A_j[k][v][w]    (part->joint copy then adjacency, graph.py:606-608)
    std::vector<double> AU((size_t)3 * 6 * V, 0.0);
    for (int k = 0; k < 3; ++k)
        for (int v = 0; v < V; ++v)
            for (int w = 0; w < V; ++w) AU[((size_t)k * 6 + sk.part_of[v]) * V + w] += (double)(float)sk.A_j[((size_t)k * V + v) * V + w];
    up("AU", f32(AU));
    up("A_b", f32(sk.A_b));
    double Absum[2 * 6];
    for (int k = 0; k < 2; ++k)
        for (int w = 0; w < 6; ++w) { double a = 0; for (int v = 0; v < 6; ++v) a += (double)(float)sk.A_b[(k * 6 + v) * 6 + w]; Absum[k * 6 + w] = a; }

    // ---- mot_embedding
    up("pos_emb", W(c, "pos_emb"));
    up("emb.W1", W(c, "mot_embedding.1.weight"));
    up("emb.b1", W(c, "mot_embedding.1.bias"));
    {
        const auto& w1 = W(c, "mot_embedding.1.weight"); const auto& b1 = W(c, "mot_embedding.1.bias");
        const size_t cin = w1.size() / b1.size();
        double l1 = 0, bm = 0;
        for (size_t o = 0; o < b1.size(); ++o) {
            double a = 0;
            for (size_t i = 0; i < cin; ++i) a += std::fabs((double)w1[o * cin + i]);
            l1 = std::max(l1, a); bm = std::max(bm, std::fabs((double)b1[o]));
        }
        c->emb_l1 = (float)(l1 * (1.0 + 1e-6)); c->emb_bmax = (float)(bm * (1.0 + 1e-6));       // rounded up: a bound
    }
    up("emb.Wg", repack_gcn_adjfirst(W(c, "mot_embedding.2.blk.gcn.conv.weight"), 3, 256, 64));
    {
        const auto& bg = W(c, "mot_embedding.2.blk.gcn.conv.bias");
        std::vector<float> rb(6 * 256);
        for (int p = 0; p < 6; ++p)
            for (int co = 0; co < 256; ++co) { double a = 0; for (int k = 0; k < 3; ++k) a += (double)bg[k * 256 + co] * APsum[k * 6 + p]; rb[p * 256 + co] = (float)a; }
        up("emb.rbg", rb);
    }
    up("emb.Wt", repack_tcn(W(c, "mot_embedding.2.blk.tcn.weight"), 256, 256, 5));
    up("emb.bt", W(c, "mot_embedding.2.blk.tcn.bias"));
    {
        // The joint block applies its 1x1 gcn conv and its k=5 temporal conv back to back (net/blocks.py:126-134: norm and
        // activation act on the block's INPUT, nothing sits between gcn and tcn), so the two compose into one linear map on the
        // pooled, adjacency-mixed 3 x 64 channels: per tap  Wc_tap = Wt_tap (256 x 256) · Wg (256 x 192),  K = 5 x 192 = 960
        // instead of a K = 192 GEMM at 4x the rows plus a K = 1280 one.  fp64, rounded once.
        //   Wc[co][tap*192 + j] = sum_c Wt[co][tap*256 + c] Wg[c][j];   rbc[p][co] = bt[co] + sum_tap sum_c Wt[co][tap*256 + c] rbg[p][c]
        // (the gcn bias is constant over frames, so reflect padding and the 4-frame mean leave it a per-part constant)
        const std::vector<float> Wt = repack_tcn(W(c, "mot_embedding.2.blk.tcn.weight"), 256, 256, 5);
        const std::vector<float> Wg = repack_gcn_adjfirst(W(c, "mot_embedding.2.blk.gcn.conv.weight"), 3, 256, 64);
        const auto& bg = W(c, "mot_embedding.2.blk.gcn.conv.bias");
        const auto& bt = W(c, "mot_embedding.2.blk.tcn.bias");
        std::vector<double> Wc((size_t)256 * 960, 0.0), rbc(6 * 256, 0.0), rbg(6 * 256, 0.0);
        for (int p = 0; p < 6; ++p)
            for (int cc = 0; cc < 256; ++cc) { double a = 0; for (int k = 0; k < 3; ++k) a += (double)bg[k * 256 + cc] * APsum[k * 6 + p]; rbg[p * 256 + cc] = a; }
        for (int co = 0; co < 256; ++co)
            for (int tap = 0; tap < 5; ++tap) {
                double* row = &Wc[(size_t)co * 960 + tap * 192];
                for (int cc = 0; cc < 256; ++cc) {
                    const double wt = Wt[(size_t)co * 1280 + tap * 256 + cc];
                    const float* g = &Wg[(size_t)cc * 192];
                    for (int j = 0; j < 192; ++j) row[j] += wt * (double)g[j];
                    for (int p = 0; p < 6; ++p) rbc[p * 256 + co] += wt * rbg[p * 256 + cc];
                }
            }
        for (int p = 0; p < 6; ++p) for (int co = 0; co < 256; ++co) rbc[p * 256 + co] += (double)bt[co];
        up("emb.Wc", f32(Wc)); up("emb.rbc", f32(rbc));
    }
    for (int which = 0; which < 2; ++which) {
        const std::string src = which ? "to_mot.1.blk." : "mot_embedding.5.blk.";
        const std::string dst = which ? "mot." : "emb.";
        up(dst + "Wgb", repack_gcn_adjfirst(W(c, src + "gcn.conv.weight"), 2, 256, 256));
        const auto& bg = W(c, src + "gcn.conv.bias");
        std::vector<float> rb(6 * 256);
        for (int w = 0; w < 6; ++w)
            for (int co = 0; co < 256; ++co) { double a = 0; for (int k = 0; k < 2; ++k) a += (double)bg[k * 256 + co] * Absum[k * 6 + w]; rb[w * 256 + co] = (float)a; }
        up(dst + "rbb", rb);
        up(dst + "Wtb", repack_tcn(W(c, src + "tcn.weight"), 256, 256, 3));
        up(dst + "btb", W(c, src + "tcn.bias"));
    }
    // ---- transformers
    for (int l = 0; l < c->cfg.enc_depth; ++l) {
        const std::string s = "encoder.layers." + std::to_string(l), d = "enc" + std::to_string(l);
        std::vector<float> qkv = W(c, s + ".1.to_q.1.weight");
        const auto& k = W(c, s + ".1.to_k.1.weight"); const auto& v = W(c, s + ".1.to_v.weight");
        qkv.insert(qkv.end(), k.begin(), k.end()); qkv.insert(qkv.end(), v.begin(), v.end());
        up(d + ".Wqkv", qkv);
        up(d + ".Wo", W(c, s + ".1.to_out.0.weight")); up(d + ".bo", W(c, s + ".1.to_out.0.bias"));
        up(d + ".W1", W(c, s + ".2.net.0.weight")); up(d + ".b1", W(c, s + ".2.net.0.bias"));
        up(d + ".W2", W(c, s + ".2.net.3.weight")); up(d + ".b2", W(c, s + ".2.net.3.bias"));
    }
    for (int l = 0; l < c->cfg.dec_depth; ++l) {
        const std::string s = "decoder.layers." + std::to_string(l), d = "dec" + std::to_string(l);
        up(d + ".Ws2", W(c, s + ".0.style.4.weight")); up(d + ".bs2", W(c, s + ".0.style.4.bias"));      // per layer, for large batches
        up(d + ".Wq", W(c, s + ".1.to_q.1.weight")); up(d + ".Wk", W(c, s + ".1.to_k.1.weight")); up(d + ".Wv", W(c, s + ".1.to_v.weight"));
        up(d + ".Wo", W(c, s + ".1.to_out.0.weight")); up(d + ".bo", W(c, s + ".1.to_out.0.bias"));
        up(d + ".W1", W(c, s + ".2.net.0.weight")); up(d + ".b1", W(c, s + ".2.net.0.bias"));
        up(d + ".W2", W(c, s + ".2.net.3.weight")); up(d + ".b2", W(c, s + ".2.net.3.bias"));
        const int H = c->cfg.dec_heads, DH = c->cfg.dec_dim_head, D = 256;
        if (DH == D) {
            // folded projections (see run_decoder), accumulated in fp64 and rounded once:
            //   Wqk[h*D + j][i] = sum_d Wq[h*DH + d][i] * Wk[h*DH + d][j]        q' = IN(x) Wqk^T, keys = IN(cha)
            //   Wvo[c][h*D + j] = sum_d Wo[c][h*DH + d] * Wv[h*DH + d][j]        out = [P_h cha]_h Wvo^T + bo
            const auto& Wq = W(c, s + ".1.to_q.1.weight"); const auto& Wk = W(c, s + ".1.to_k.1.weight");
            const auto& Wv = W(c, s + ".1.to_v.weight");   const auto& Wo = W(c, s + ".1.to_out.0.weight");
            std::vector<double> qk((size_t)H * D * D, 0.0), vo((size_t)D * H * D, 0.0);
            for (int h = 0; h < H; ++h)
                for (int dd = 0; dd < DH; ++dd) {
                    const float* q = &Wq[(size_t)(h * DH + dd) * D];
                    const float* k = &Wk[(size_t)(h * DH + dd) * D];
                    const float* v = &Wv[(size_t)(h * DH + dd) * D];
                    for (int j = 0; j < D; ++j) {
                        double* row = &qk[((size_t)h * D + j) * D];
                        const double kj = k[j];
                        for (int i = 0; i < D; ++i) row[i] += kj * (double)q[i];
                    }
                    for (int co = 0; co < D; ++co) {
                        double* row = &vo[(size_t)co * H * D + (size_t)h * D];
                        const double w = Wo[(size_t)co * H * DH + h * DH + dd];
                        for (int j = 0; j < D; ++j) row[j] += w * (double)v[j];
                    }
                }
            up(d + ".Wqk", f32(qk)); up(d + ".Wvo", f32(vo));
        }
    }
    {
        // the style MLPs of ALL decoder layers read the same input (the token mean of cha): one GEMM for every layer's first linear
        // (weights stacked), one for the second (block-diagonal: layer l's 512 outputs see only layer l's hidden 512) - two launches
        // instead of two per layer
        const int L = c->cfg.dec_depth;
        std::vector<float> w1((size_t)L * 512 * 256), b1v((size_t)L * 512), w2((size_t)L * 512 * L * 512, 0.f), b2v((size_t)L * 512);
        for (int l = 0; l < L; ++l) {
            const std::string sl = "decoder.layers." + std::to_string(l);
            const auto& a1 = W(c, sl + ".0.style.2.weight"); const auto& c1 = W(c, sl + ".0.style.2.bias");
            const auto& a2 = W(c, sl + ".0.style.4.weight"); const auto& c2 = W(c, sl + ".0.style.4.bias");
            std::copy(a1.begin(), a1.end(), w1.begin() + (size_t)l * 512 * 256);
            std::copy(c1.begin(), c1.end(), b1v.begin() + (size_t)l * 512);
            std::copy(c2.begin(), c2.end(), b2v.begin() + (size_t)l * 512);
            for (int o = 0; o < 512; ++o)
                std::copy(a2.begin() + (size_t)o * 512, a2.begin() + (size_t)(o + 1) * 512, w2.begin() + ((size_t)l * 512 + o) * L * 512 + (size_t)l * 512);
        }
        up("dec.Ws1_all", w1); up("dec.bs1_all", b1v); up("dec.Ws2_blk", w2); up("dec.bs2_all", b2v);
        // ... and the same MLP's operands in float64 (mocha_linear_f64; the fp32 values are exact in float64): first linear stacked over the
        // layers, second linear per layer [L][512][512]
        std::vector<double> w2d((size_t)L * 512 * 512);
        for (int l = 0; l < L; ++l) {
            const auto& a2 = W(c, "decoder.layers." + std::to_string(l) + ".0.style.4.weight");
            std::copy(a2.begin(), a2.end(), w2d.begin() + (size_t)l * 512 * 512);
        }
        auto up64 = [&](const std::string& n, const std::vector<double>& v) {
            if (rc) return;
            if (!rc) rc = upload_to(c, c->w64, n, v);
        };
        up64("dec.Ws1_all", std::vector<double>(w1.begin(), w1.end())); up64("dec.bs1_all", std::vector<double>(b1v.begin(), b1v.end()));
        up64("dec.Ws2_all", w2d); up64("dec.bs2_all", std::vector<double>(b2v.begin(), b2v.end()));
        c->bank.dec_valid = false;                          // cached bank constants were made with the previous weights
    }
    // ---- to_mot joint block + head
    up("mot.Wg2", W(c, "to_mot.4.blk.gcn.conv.weight")); up("mot.bg2", W(c, "to_mot.4.blk.gcn.conv.bias"));
    up("mot.Wt2", repack_tcn(W(c, "to_mot.4.blk.tcn.weight"), 64, 64, 5)); up("mot.bt2", W(c, "to_mot.4.blk.tcn.bias"));
    {
        // Output frame t = 4 s + phase of the k = 5 conv over the nearest-x4-upsampled frames (model.py:74, net/blocks.py:112-118) reads
        // upsampled frames t-2 .. t+2 = source frames s-1, s, s+1 only, each several times: the taps that land on one source frame are
        // summed into one weight.  [phase*64 + co][j*64 + ci], j = source frame s-1, s, s+1; a third of the blocks are zero.
        // The reflection at the upsampled ends (frames -2, -1 -> 2, 1; 60, 61 -> 58, 57) stays inside the first / last source frame.
        const std::vector<float>& w = W(c, "to_mot.4.blk.tcn.weight");          // (64, 64, 5, 1)
        static const int JOF[4][5] = {{0, 0, 1, 1, 1}, {0, 1, 1, 1, 1}, {1, 1, 1, 1, 2}, {1, 1, 1, 2, 2}};
        std::vector<double> acc((size_t)256 * 192, 0.0);
        for (int ph = 0; ph < 4; ++ph)
            for (int co = 0; co < 64; ++co)
                for (int ci = 0; ci < 64; ++ci)
                    for (int t = 0; t < 5; ++t) acc[((size_t)ph * 64 + co) * 192 + JOF[ph][t] * 64 + ci] += (double)w[((size_t)co * 64 + ci) * 5 + t];
        std::vector<float> wp(acc.size()), bp(256);
        for (size_t i = 0; i < acc.size(); ++i) wp[i] = (float)acc[i];
        const std::vector<float>& bt = W(c, "to_mot.4.blk.tcn.bias");
        for (int i = 0; i < 256; ++i) bp[i] = bt[i & 63];
        up("mot.Wt2p", wp); up("mot.bt2p", bp);
        // the same without the zero blocks, for large batches: phases 0, 1 read source frames (s-1, s), phases 2, 3 read (s, s+1)
        std::vector<float> wa((size_t)128 * 128), wb((size_t)128 * 128);
        for (int r = 0; r < 128; ++r)
            for (int k = 0; k < 128; ++k) {
                wa[(size_t)r * 128 + k] = wp[(size_t)r * 192 + k];
                wb[(size_t)r * 128 + k] = wp[(size_t)(128 + r) * 192 + 64 + k];
            }
        up("mot.Wt2a", wa); up("mot.Wt2b", wb);
    }
    up("mot.W6", W(c, "to_mot.6.weight")); up("mot.b6", W(c, "to_mot.6.bias"));
    if (rc) return rc;
    c->finalized = true;
    return 0;
}

int mocha_reserve(mocha_ctx* c, int max_batch) {
    if (!c || max_batch < 1) return fail(c, MOCHA_ERR_ARG, "max_batch must be >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    c->max_chunk = max_batch;
    if (c->chunk > max_batch) {           // shrink: drop the larger arena first
        HIPCHK(c, hipDeviceSynchronize());
        c->chunk = 0;
    }
    int rc = ensure_ws(c, max_batch);
    if (rc) return rc;
    if (c->bank.resident) {
        // a resident bank is searched per character only: its scratch is the segmented matcher's, which depends on nothing but the
        // workspace and the bank's two reserved maxima - re-sized here, so that the calls after it still never allocate
        c->seg_q = std::min(SEG_MAX_Q, std::max(set_windows(c, 0), 16));
        for (int set = 0; set < mocha_ctx::MAX_SETS; ++set)
            if ((set == 0 || !c->sets[set].ws.empty()) && (rc = ensure_seg_scratch(c, set))) return rc;
        return 0;
    }
    if (c->bank.N > 0)                                    // ... and the match scratch of the current bank for that many queries
        for (int set = 0; set < mocha_ctx::MAX_SETS; ++set)
            if (!c->sets[set].ws.empty() && (rc = ensure_match_scratch(c, set, set_windows(c, set), c->bank, true))) return rc;
    return 0;
}

int mocha_pos_emb(mocha_ctx* c, const float** dev_ptr) {
    if (!c || !dev_ptr) return MOCHA_ERR_ARG;
    if (!c->finalized) return fail(c, MOCHA_ERR_STATE, "weights not finalised");
    *dev_ptr = DW(c, "pos_emb");
    return 0;
}

int mocha_graph_constants(mocha_ctx* c, float* A_j, float* A_b, float* pool, float* unpool) {
    if (!c) return MOCHA_ERR_ARG;
    const Skeleton& sk = c->sk;
    if (A_j) for (size_t i = 0; i < sk.A_j.size(); ++i) A_j[i] = (float)sk.A_j[i];
    if (A_b) for (size_t i = 0; i < sk.A_b.size(); ++i) A_b[i] = (float)sk.A_b[i];
    if (pool) for (size_t i = 0; i < sk.pool.size(); ++i) pool[i] = (float)sk.pool[i];
    if (unpool) for (size_t i = 0; i < sk.unpool.size(); ++i) unpool[i] = (float)sk.unpool[i];
    return 0;
}

int mocha_embed(mocha_ctx* c, const float* X, int B, float* tokens, int add_pos, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_embed", X, tokens);
    const size_t xs = (size_t)60 * c->cfg.V * c->cfg.C_in, ts = 90 * 256;
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        return run_embed(c, X + b0 * xs, b, tokens + b0 * ts, add_pos != 0, s);
    });
}

int mocha_encoder(mocha_ctx* c, const float* tokens, int B, float* encoded, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_encoder", tokens, encoded);
    const size_t ts = 90 * 256;
    for (int i = 0; i < mocha_ctx::MAX_SETS; ++i) c->sets[i].amax_tok_of = nullptr;      // caller-supplied tokens (the reference adds pos_emb itself): measured, not carried
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        return run_encoder(c, tokens + b0 * ts, b, encoded + b0 * ts, s);
    });
}

int mocha_mvn(mocha_ctx* c, const float* encoded, int B, float* cnt, const float* cnt_mean, const float* cnt_std,
              float* cnt_nm, void* stream) {
    if (!c) return MOCHA_ERR_ARG;                      // needs no weights: usable on a bare context
    if (B == 0) return 0;                              // empty batch: nothing to do, pointers may be null
    if (!encoded || (!cnt && !cnt_nm) || B < 0) return fail(c, MOCHA_ERR_ARG, "bad mvn arguments");
    if (cnt_nm && (!cnt_mean || !cnt_std)) return fail(c, MOCHA_ERR_ARG, "mocha_mvn: cnt_nm needs cnt_mean and cnt_std");
    HIPCHK(c, hipSetDevice(c->device));
    const bool zn = cnt_nm != nullptr;
    hipStream_t s = (hipStream_t)stream;
    const InormExtra iex0 = IEX(c);
    LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, B * 90.0 * 256 * 4 * (1 + (cnt ? 1 : 0) + (zn ? 1 : 0)), launch_instnorm(encoded, cnt, nullptr, zn ? cnt_mean : nullptr, zn ? cnt_std : nullptr, zn ? cnt_nm : nullptr, B, 90, s, &iex0));
    return 0;
}

int mocha_encode(mocha_ctx* c, const float* X, int B, float* encoded, float* cnt, const float* cnt_mean,
                 const float* cnt_std, float* cnt_nm, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_encode", X, encoded);
    const size_t xs = (size_t)60 * c->cfg.V * c->cfg.C_in, ts = 90 * 256;
    if (cnt_nm && (!cnt_mean || !cnt_std)) return fail(c, MOCHA_ERR_ARG, "mocha_encode: cnt_nm needs cnt_mean and cnt_std");
    const bool zn = cnt_nm != nullptr;                      // cnt itself is optional: the z-scored copy alone is a valid request
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r = run_embed(c, X + b0 * xs, b, WS(c, "x5"), true, s);      // x5 is free again once the body block has read it
        if (r) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, encoded + b0 * ts, s))) return r;
        if (cnt || zn) {
            const InormExtra iex0 = IEXW(c, s);
            LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, b * 90.0 * 256 * 4 * (1 + (cnt ? 1 : 0) + (zn ? 1 : 0)),
                   launch_instnorm(encoded + b0 * ts, cnt ? cnt + b0 * ts : nullptr, nullptr, zn ? cnt_mean : nullptr, zn ? cnt_std : nullptr,
                                   zn ? cnt_nm + b0 * ts : nullptr, b, 90, s, &iex0));
        }
        return 0;
    });
}

int mocha_decoder(mocha_ctx* c, const float* src_enc, const float* cha_enc, int B, float* out, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_decoder", src_enc, cha_enc, out);
    const size_t ts = 90 * 256;
    for (int i = 0; i < mocha_ctx::MAX_SETS; ++i) c->sets[i].amax_enc_of = c->sets[i].amax_dec_of = c->sets[i].amax_tok_of = nullptr;     // external activations: no carried bounds
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        return run_decoder(c, src_enc + b0 * ts, cha_enc + b0 * ts, b, out + b0 * ts, s);
    });
}

int mocha_style_constants(mocha_ctx* c, const float* cha_enc, int B, float* gb, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_style_constants", cha_enc, gb);
    const size_t T = 90 * 256, G = (size_t)512 * c->cfg.dec_depth;
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        InormExtra ex = IEXW(c, s);
        if (c->style_f64) ex.mean64 = reinterpret_cast<double*>(WS(c, "smean64"));
        LAUNCH(c, s, "mocha_instnorm", "dec.in_cha", 0.0, b * 90.0 * 256 * 4 * 2,
               launch_instnorm(cha_enc + b0 * T, WS(c, "kin"), WS(c, "smean"), nullptr, nullptr, nullptr, b, 90, s, &ex));
        int r = run_style(c, b, s);
        if (r) return r;
        HIPCHK(c, hipMemcpyAsync(gb + b0 * G, WS(c, "gb"), (size_t)b * G * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    });
}

int mocha_to_mot(mocha_ctx* c, const float* tokens, int B, float* Y, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_to_mot", tokens, Y);
    const size_t ts = 90 * 256, ys = (size_t)60 * c->cfg.V * c->cfg.C_in;
    for (int i = 0; i < mocha_ctx::MAX_SETS; ++i) c->sets[i].amax_enc_of = c->sets[i].amax_dec_of = c->sets[i].amax_tok_of = nullptr;     // external activations: no carried bounds
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        return run_to_mot(c, tokens + b0 * ts, b, Y + b0 * ys, s);
    });
}

int mocha_forward(mocha_ctx* c, const float* src_X, const float* cha_X, int B, float* Y, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_forward", src_X, cha_X, Y);
    const size_t xs = (size_t)60 * c->cfg.V * c->cfg.C_in;
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        if ((r = run_embed(c, src_X + b0 * xs, b, WS(c, "x5"), true, s))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, WS(c, "enc_s"), s))) return r;
        if ((r = run_embed(c, cha_X + b0 * xs, b, WS(c, "x5"), true, s))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, WS(c, "enc_c"), s))) return r;
        if ((r = run_decoder(c, WS(c, "enc_s"), WS(c, "enc_c"), b, WS(c, "dec"), s))) return r;
        return run_to_mot(c, WS(c, "dec"), b, Y + b0 * xs, s);
    });
}

int mocha_forward_features(mocha_ctx* c, const float* src_X, const float* cha_X, int B, float* src_enc, float* cha_enc,
                           float* src_cnt, float* cha_cnt, void* stream) {
    int rc = mocha_encode(c, src_X, B, src_enc, src_cnt, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    return mocha_encode(c, cha_X, B, cha_enc, cha_cnt, nullptr, nullptr, nullptr, stream);
}

// Owned storage for the rows of a bank of N entries (mocha_bank_set without MOCHA_BANK_BORROW, the receiving ranks of mocha_bank_broadcast)
static int bank_own_rows(mocha_ctx* c, Bank& b, int64_t N) {
    const size_t need = (size_t)N * 90 * 256;
    if (b.cnt_own.n >= need && b.enc_own.n >= need) return 0;
    // the current bank may be the copy that is about to be freed: no dangling pointers if an allocation below fails
    if (b.cnt == b.cnt_own.p || b.enc == b.enc_own.p) { b.cnt = nullptr; b.enc = nullptr; b.N = 0; b.resident = false; b.slot.clear(); c->generation++; }
    int rc = reserve(c, b.cnt_own, need);
    return rc ? rc : reserve(c, b.enc_own, need);
}

// Sets bank `b` and derives what matching against it needs.  b = c->bank (mocha_bank_set): it becomes the context's current bank, with every
// derived image and cache.  b = c->pair, the transient bank of mocha_characterize_pair: centroid, row norms and the plane image only, and
// captured graphs stay valid (no generation bump, the current bank's segment table, bounds, copies and decoder cache are not its business)
static int bank_set_impl(mocha_ctx* c, Bank& b, const float* cnt_nm, const float* encoded, int64_t N, int flags, void* stream) {
    int rc = ready(c, 0, &b != &c->pair); if (rc) return rc;      // (the transient bank is set in the middle of a call: its walk order goes on)
    if (!cnt_nm || !encoded || N < 1 || N > (int64_t)1 << 30) return fail(c, MOCHA_ERR_ARG, "bad bank arguments");
    const bool current = &b == &c->bank;
    hipStream_t s = (hipStream_t)stream;
    const size_t D = 90 * 256;
    if (flags & MOCHA_BANK_BORROW) {
        b.cnt = cnt_nm; b.enc = encoded;
    } else {
        if ((rc = bank_own_rows(c, b, N))) return rc;
        HIPCHK(c, hipMemcpyAsync(b.cnt_own.p, cnt_nm, (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(b.enc_own.p, encoded, (size_t)N * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        b.cnt = b.cnt_own.p; b.enc = b.enc_own.p;
    }
    if ((rc = reserve(c, b.norm, (size_t)N))) return rc;
    b.N = N;
    b.is_bf16 = (flags & MOCHA_BANK_BF16) != 0;
    b.seg_start.clear(); b.seg_max_rows = 0;              // a plain bank has no segment table (mocha_bank_set_segments sets it after)
    b.resident = false; b.slot.clear();                   // ... and replaces a resident bank like any other
    b.labelled = false;                                   // ... and no action labels (mocha_bank_set_labels)
    b.tiled_valid = false; b.tile32_valid = false;
    if (current) c->generation++;                         // a captured step has the previous bank's pointers and row count baked in
    // match scratch for every query count the workspace admits: a later match never allocates (capture-safe)
    for (int set = 0; set < mocha_ctx::MAX_SETS; ++set)
        if ((set == 0 || !c->sets[set].ws.empty()) && (rc = ensure_match_scratch(c, set, set_windows(c, set), b, true))) return rc;
    // centroid of the bank: the many-query GEMM and the bf16 copy work on b - centroid (see do_match)
    if ((rc = reserve(c, b.center, D))) return rc;
    if ((rc = reserve(c, c->center_scratch, column_mean_scratch_doubles((int)D)))) return rc;
    LAUNCH(c, s, "mocha_column_mean", "bank.center", 0.0, 4.0 * N * D, launch_column_mean(b.cnt, N, (int)D, b.center.p, c->center_scratch.p, s));
    if (b.is_bf16) {
        if ((rc = reserve(c, b.bf16, (size_t)N * D))) return rc;
        LAUNCH(c, s, "mocha_to_bf16", "bank.to_bf16", 0.0, 6.0 * N * D, launch_to_bf16(b.cnt, b.center.p, (int)D, b.bf16.p, (int64_t)N * D, s));
        LAUNCH(c, s, "mocha_rownorm2_bf16", "bank.norms", 2.0 * N * D, 2.0 * N * D, launch_rownorm2_bf16(b.bf16.p, b.norm.p, N, (int)D, s));
    } else {
        LAUNCH(c, s, "mocha_rownorm2", "bank.norms", 2.0 * N * D, 4.0 * N * D, launch_rownorm2(b.cnt, b.center.p, b.norm.p, N, (int)D, s, walk_next(c, s)));
    }
    b.amax_ok = false; b.b16f_valid = false; b.b8_valid = false; b.dec_valid = false;
    // two-plane fp16 engine: the decoder's attention rows are bounded by the matched entries' largest magnitude, taken once here
    if (current && c->gemm_h2) {
        if ((rc = reserve(c, b.amax, (size_t)N))) return rc;
        HIPCHK(c, hipMemsetAsync(b.amax.p, 0, (size_t)N * sizeof(float), s));
        for (int64_t n0 = 0; n0 < N; n0 += 65535)      // (the kernel's grid.y)
            LAUNCH(c, s, "mocha_absmax", "bank.absmax", 0.0, 4.0 * std::min<int64_t>(65535, N - n0) * D,
                   launch_absmax(b.enc + (size_t)n0 * D, std::min<int64_t>(65535, N - n0), (long long)D, b.amax.p + n0, s));
        b.amax_ok = true;
    }
    // few-query matching against a large fp32 bank scans its centred bf16 copy (half the bytes) and re-ranks exactly
    if (current && !b.is_bf16 && c->scan16 && N >= SCAN16_MIN) {
        if ((rc = reserve(c, b.b16f, (size_t)N * D))) return rc;
        if ((rc = reserve(c, b.rho, (size_t)N))) return rc;
        LAUNCH(c, s, "mocha_to_bf16", "bank.to_bf16", 0.0, 6.0 * N * D, launch_to_bf16(b.cnt, b.center.p, (int)D, b.b16f.p, (int64_t)N * D, s));
        LAUNCH(c, s, "mocha_rowresid", "bank.resid", 3.0 * N * D, 6.0 * N * D, launch_rowresid(b.cnt, b.center.p, b.b16f.p, b.rho.p, N, (int)D, s));
        b.b16f_valid = true;
    }
    if (current && b.b16f_valid && c->scan8) {
        if ((rc = reserve(c, b.b8, (size_t)N * D))) return rc;
        if ((rc = reserve(c, b.b8_scale, (size_t)N))) return rc;
        if ((rc = reserve(c, b.b8_rho, (size_t)N))) return rc;
        LAUNCH(c, s, "mocha_to_i8", "bank.to_i8", 4.0 * N * D, 9.0 * N * D, launch_to_i8(b.cnt, b.center.p, b.b8.p, b.b8_scale.p, b.b8_rho.p, N, (int)D, s));
        // a new bank: the byte stage gets another chance (its mode words, in every workspace set's scratch that exists)
        for (SetScratch& st : c->sets)
            if (st.scan_keys.p) HIPCHK(c, hipMemsetAsync(st.scan_keys.p + match_scan8_mode_word(), 0, sizeof(unsigned long long), s));
        b.b8_valid = true;
    }
    // decoder constants of every entry (round 5): IN(entry) and its AdaIN gamma / beta, read in place through frame_index by the decoder
    if (current && dec_cache_ok(c) && !(flags & MOCHA_BANK_NO_DEC_CACHE)) {
        const int L = c->cfg.dec_depth;
        // + N x (92 KB + 2 KB per decoder layer): about +50 % of the bank's footprint.  If the memory is not there the bank is set all
        // the same and the decoder computes its constants per call (the round-4 flow), instead of failing mocha_bank_set
        if (b.kin.reserve((size_t)N * D) != hipSuccess || b.gb.reserve((size_t)N * 512 * L) != hipSuccess) {
            (void)hipGetLastError();                   // the failed allocation's sticky error
            b.kin.release(); b.gb.release();
        } else {
            const size_t rows = (size_t)std::min<int64_t>(N, 4096);
            if ((rc = reserve(c, c->style_scratch, rows * (256 + (size_t)512 * L)))) return rc;
            if ((rc = build_dec_consts(c, b.enc, N, b.kin.p, b.gb.p, c->style_scratch.p, c->style_scratch.p + rows * 256, (int64_t)rows, s))) return rc;
            b.dec_valid = true;
        }
    }
    // many-query matching against a small fp32 bank runs on the plane engine: centred bank as its packed image (6 B per value)
    b.x3_valid = false;
    if (!b.is_bf16 && c->gemm_x3 && N <= X3_BANK_MAX) {
        if ((rc = reserve(c, b.x3, gemm_x3_packed_elems((int)N, (int)D)))) return rc;
        LAUNCH(c, s, "mocha_pack_x3", "bank.pack_x3", 0.0, 10.0 * N * D, launch_pack_x3(b.cnt, (int)N, (int)D, b.x3.p, s, b.center.p, walk_next(c, s)));
        b.x3_valid = true;
    }
    return 0;
}

int mocha_bank_set(mocha_ctx* c, const float* cnt_nm, const float* encoded, int64_t N, int flags, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    return bank_set_impl(c, c->bank, cnt_nm, encoded, N, flags, stream);
}

int mocha_match(mocha_ctx* c, const float* query_nm, int Q, int32_t* idx, float* dist, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_match"))) return rc;
    if (Q == 0) return 0;
    if (!query_nm || !idx || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad match arguments");
    if (Q == 0) return 0;
    return do_match(c, c->bank, query_nm, Q, idx, dist, (hipStream_t)stream);
}

int mocha_match_topk(mocha_ctx* c, const float* query_nm, int Q, int k, int32_t* idx, float* dist, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_match_topk"))) return rc;
    if (Q == 0) return 0;
    if (!query_nm || !idx || Q < 0 || k < 1 || k > 64) return fail(c, MOCHA_ERR_ARG, "bad top-k arguments (1 <= k <= 64)");
    if (!c->bank.cnt || c->bank.N <= 0) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    hipStream_t s = (hipStream_t)stream;
    const int D = 90 * 256;
    const int64_t N = c->bank.N;
    if ((rc = reserve(c, c->topk_keys, (size_t)8 * N))) return rc;      // not on the per-frame path: allocated on first use
    const float* q = query_nm;
    if (c->bank.is_bf16) {                                  // the bf16 bank holds bf16(b - centroid): centred queries
        if ((rc = reserve(c, c->sets[0].match_qc, (size_t)std::max(Q, 8) * D))) return rc;
        LAUNCH(c, s, "mocha_sub_rows", "match.center", 0.0, 8.0 * Q * D, launch_sub_rows(query_nm, c->bank.center.p, c->sets[0].match_qc.p, Q, D, s));
        q = c->sets[0].match_qc.p;
    }
    const void* bank = c->bank.is_bf16 ? (const void*)c->bank.bf16.p : (const void*)c->bank.cnt;
    LAUNCH(c, s, "mocha_match_topk", "match.topk", 3.0 * Q * N * D, ((Q + 7) / 8) * (double)N * D * (c->bank.is_bf16 ? 2.0 : 4.0),
           launch_match_topk(bank, c->bank.is_bf16 ? 1 : 0, q, Q, N, D, k, c->topk_keys.p, idx, dist, s));
    return 0;
}

int mocha_bank_gather_blend(mocha_ctx* c, const int32_t* idx, const float* dist, float temperature, int Q, int k, float* out, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_bank_gather_blend"))) return rc;
    if (!c->bank.enc) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (Q == 0) return 0;
    if (!idx || !dist || !out || Q < 0 || k < 1 || k > 64 || !(temperature > 0.f)) return fail(c, MOCHA_ERR_ARG, "bad gather_blend arguments");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_gather_blend", "bank.gather_blend", 2.0 * Q * k * 90 * 256, Q * (k + 1.0) * 90 * 256 * 4,
           launch_gather_blend(c->bank.enc, idx, dist, temperature, out, Q, k, 90 * 256, c->bank.N, s));
    return 0;
}

int mocha_bank_gather(mocha_ctx* c, const int32_t* idx, int Q, float* out, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_bank_gather"))) return rc;
    if (!c->bank.enc) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (Q == 0) return 0;
    if (!idx || !out || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad gather arguments");
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_gather_rows", "bank.gather", 0.0, Q * 90.0 * 256 * 8, launch_gather_rows(c->bank.enc, idx, out, Q, 90 * 256, c->bank.N, s));
    return 0;
}

// coherent context matching: what the entry points further down and the pair form share
}  // extern "C"

namespace {
// the host lists of a path call: what they must satisfy, with nothing launched when they do not
struct PathArgs {
    const int32_t* seq_start = nullptr; int n_seq = 0;
    const int32_t* bank_start = nullptr; int n_b = 0;
    double lambda = 0.0;
    bool relative = false;                             // lambda in units of the median over the windows of their nearest distance
    unsigned char* continued = nullptr;
};

int path_check(mocha_ctx* c, const PathArgs& a, int Q, int64_t N, const char* who) {
    if (!(a.lambda >= 0.0) || !std::isfinite(a.lambda)) return fail(c, MOCHA_ERR_ARG, "%s: the jump penalty must be finite and >= 0", who);
    if (N < 1) return fail(c, MOCHA_ERR_ARG, "%s: no bank rows", who);
    if (N > MATCH_PATH_MAX_ROWS) return fail(c, MOCHA_ERR_ARG, "%s: %lld bank rows; a path call serves up to %d", who, (long long)N, MATCH_PATH_MAX_ROWS);
    if (!a.seq_start || a.n_seq < 1 || a.n_seq > Q) return fail(c, MOCHA_ERR_ARG, "%s: sequence starts: 1 .. Q sequences, n_seq + 1 entries", who);
    if (a.seq_start[0] != 0 || a.seq_start[a.n_seq] != Q) return fail(c, MOCHA_ERR_ARG, "%s: sequence starts must begin at 0 and end at Q", who);
    for (int i = 0; i < a.n_seq; ++i)
        if (a.seq_start[i + 1] <= a.seq_start[i]) return fail(c, MOCHA_ERR_ARG, "%s: sequence starts must increase strictly", who);
    if (a.n_b < 0 || (a.n_b > 0 && !a.bank_start)) return fail(c, MOCHA_ERR_ARG, "%s: bank starts: a list or none", who);
    for (int i = 0; i < a.n_b; ++i) {
        if (a.bank_start[i] < 0 || a.bank_start[i] >= N) return fail(c, MOCHA_ERR_ARG, "%s: bank start %d outside the %lld rows", who, (int)a.bank_start[i], (long long)N);
        if (i && a.bank_start[i] <= a.bank_start[i - 1]) return fail(c, MOCHA_ERR_ARG, "%s: bank starts must increase strictly", who);
    }
    return 0;
}

// the path through d (Q x N, leading dimension ld; device) -> path, dist_out, continued (device).  The caller ran path_check.
int path_run(mocha_ctx* c, const float* d, int Q, int N, int64_t ld, const PathArgs& a, int32_t* path, float* dist_out, hipStream_t s) {
    int rc;
    if ((rc = reserve(c, c->path_m, (size_t)Q))) return rc;
    if ((rc = reserve(c, c->path_cont, match_path_cont_words(Q)))) return rc;
    if ((rc = reserve(c, c->path_bits, match_path_bits_words(N)))) return rc;
    if ((rc = reserve(c, c->path_lists, (size_t)a.n_seq + 1 + (size_t)std::max(a.n_b, 1)))) return rc;
    double lambda = a.lambda;
    if (a.relative) {
        // the unit comes from the matrix itself: row minima on the device, their (lower) median on the host - a batch call, the stream
        // is drained here
        if ((rc = reserve(c, c->path_min, (size_t)Q))) return rc;
        LAUNCH(c, s, "mocha_path_rowmin", "match.path_unit", 0.0, 4.0 * Q * N, launch_path_rowmin(d, Q, N, ld, c->path_min.p, s));
        std::vector<float> mins((size_t)Q);
        HIPCHK(c, hipMemcpyAsync(mins.data(), c->path_min.p, (size_t)Q * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        std::nth_element(mins.begin(), mins.begin() + (Q - 1) / 2, mins.end());
        lambda = a.lambda * (double)mins[(size_t)(Q - 1) / 2];
        if (!(lambda >= 0.0) || !std::isfinite(lambda)) return fail(c, MOCHA_ERR_ARG, "relative jump penalty: the distances' median is not finite");
    }
    int32_t* seq_dev = c->path_lists.p;
    int32_t* bank_dev = c->path_lists.p + a.n_seq + 1;
    // (pageable host memory: the copy is staged before the call returns, the caller's lists are free after it)
    HIPCHK(c, hipMemcpyAsync(seq_dev, a.seq_start, ((size_t)a.n_seq + 1) * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (a.n_b > 0) HIPCHK(c, hipMemcpyAsync(bank_dev, a.bank_start, (size_t)a.n_b * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LAUNCH(c, s, "mocha_match_path", "match.path", 4.0 * Q * N, 4.0 * Q * N + 2.0 * match_path_cont_words(Q),
           launch_match_path(d, Q, N, ld, seq_dev, a.n_seq, bank_dev, a.n_b, lambda, c->path_bits.p, c->path_m.p, c->path_cont.p, path, dist_out,
                             a.continued, s));
    return 0;
}

// matrix of Q queries against N fp32 rows into the context's own matrix, then the path through it
int path_match(mocha_ctx* c, const float* rows, int64_t N, const float* q, int Q, const PathArgs& a, int32_t* path, hipStream_t s) {
    int rc;
    const int D = 90 * 256;
    if ((rc = reserve(c, c->path_d, (size_t)Q * N))) return rc;
    if ((rc = reserve(c, c->path_keys, match_dist_keys_words(Q, (int)N)))) return rc;
    LAUNCH(c, s, "mocha_match_dist", "match.dist_matrix", 3.0 * Q * N * D, ((Q + 7) / 8) * (double)N * D * 4.0,
           launch_match_dist(rows, q, Q, (int)N, D, c->path_keys.p, c->path_d.p, N, s));
    return path_run(c, c->path_d.p, Q, (int)N, N, a, path, nullptr, s);
}
}  // namespace

extern "C" {

// The characterize against the bank as ONE set of rows (mocha_characterize, mocha_step_graph)
static int characterize_impl(mocha_ctx* c, const float* src_X, int B, const float* cnt_mean, const float* cnt_std, float* Y,
                             int32_t* idx, void* stream, bool raw) {
    int rc = ready(c, B); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_characterize / mocha_step_graph"))) return rc;
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (B == 0) return 0;
    if (!cnt_mean || !cnt_std || !src_X || !Y) return fail(c, MOCHA_ERR_ARG, "null argument");
    const size_t ys = (size_t)60 * c->cfg.V * c->cfg.C_in;
    const size_t xs = raw ? (size_t)60 * (c->cfg.V + 1) * c->cfg.C_in : ys;
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        int32_t* ix = idx ? idx + b0 : SET(c).idx_ws.p;
        if ((r = run_embed(c, src_X + b0 * xs, b, WS(c, "x5"), true, s, raw))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, WS(c, "enc_s"), s))) return r;
        // cnt, its z-score and - the bank's centroid is known - the matcher's centred queries in one pass
        // (as one bf16 plane where the many-query pass against a bf16 bank will read them: no mocha_center_bf16 launch)
        const bool q16 = c->bank.is_bf16 && b > 8;
        const bool sel2 = use_select2(c, c->bank, b);                   // the selection's row statistics (and the second bf16 plane) come from this pass too
        if (sel2 && (r = ensure_match_scratch(c, c->cur, b, c->bank, false))) return r;
        InormExtra ex = IEXW(c, s); ex.centre = c->bank.center.p;
        if (q16) ex.zc16 = reinterpret_cast<unsigned short*>(WS(c, "qc")); else ex.zc = WS(c, "qc");
        if (sel2) { ex.qstat = SET(c).match_qstat.p; if (q16 && c->match_planes == 2) ex.plane_stride = (long long)b * 90 * 256; }
        LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, b * 90.0 * 256 * 4 * (q16 ? (sel2 ? 3.0 : 2.5) : 3.0), launch_instnorm(WS(c, "enc_s"), nullptr, nullptr, cnt_mean, cnt_std, WS(c, "qnm"), b, 90, s, &ex));
        if ((r = do_match(c, c->bank, WS(c, "qnm"), b, ix, nullptr, s, WS(c, "qc"), q16, sel2))) return r;
        // decoder on cha_encoded[frame_index]: its first kernel gathers the rows itself
        if ((r = run_decoder(c, WS(c, "enc_s"), nullptr, b, WS(c, "dec"), s, c->bank.enc, ix, c->bank.N,
                             c->bank.dec_valid ? c->bank.kin.p : nullptr, c->bank.dec_valid ? c->bank.gb.p : nullptr))) return r;
        return run_to_mot(c, WS(c, "dec"), b, Y + b0 * ys, s, raw);
    });
}

// The segmented characterize, every variant of it: embed -> encoder -> cnt and its z-score (bf16 bank: and the queries centred on the
// union's centroid) -> the window's character feature as `sel` says -> decoder -> to_mot.  Hard: the matcher leaves the global rows in
// the workspace's index buffer and the decoder gathers through them, with the bank's per-entry constants.  Soft and mix: the matcher
// blends into the "sel" workspace and the literal decoder runs on the blend (instance norm and style MLP of the feature per call - the
// per-entry constants do not apply to a blend).  The caller checked k, the temperature and J.
static int characterize_segmented_impl(mocha_ctx* c, const SegWindows& w, const SegSelect& sel, void* stream) {
    int rc = ready(c, w.B); if (rc) return rc;
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (w.B == 0) return 0;
    if (!w.cnt_mean || !w.cnt_std || !w.X || !w.Y || !sel.ids() || (sel.mix && !sel.mix->weights)) return fail(c, MOCHA_ERR_ARG, "null argument");
    const size_t ys = (size_t)60 * c->cfg.V * c->cfg.C_in;
    const size_t xs = w.raw ? (size_t)60 * (c->cfg.V + 1) * c->cfg.C_in : ys;
    const bool b16 = c->bank.is_bf16;
    return for_chunks(c, w.B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        if ((r = run_embed(c, w.X + b0 * xs, b, WS(c, "x5"), true, s, w.raw))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, WS(c, "enc_s"), s))) return r;
        InormExtra ex = IEXW(c, s);
        if (b16) { ex.centre = c->bank.center.p; ex.zc = WS(c, "qc"); }
        LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, b * 90.0 * 256 * 4 * (b16 ? 3.0 : 2.0), launch_instnorm(WS(c, "enc_s"), nullptr, nullptr, w.cnt_mean, w.cnt_std, WS(c, "qnm"), b, 90, s, &ex));
        const float* q = WS(c, b16 ? "qc" : "qnm");
        AllowArg ab;
        if (sel.allow) ab = sel.allow->at(b0);
        const AllowArg* al = sel.allow ? &ab : nullptr;
        int32_t* gx = SET(c).idx_ws.p;
        int32_t* i0 = sel.idx0 ? sel.idx0 + b0 : nullptr;
        if (sel.path) {
            // the online path: window s is stream s of the state, so the call is one chunk; the z-scored queries against the fp32 rows
            // also on a bf16 bank; then the hard decoder route below, through the rows the step left in gx
            if (b != w.B) return fail(c, MOCHA_ERR_STATE, "characterize_segmented_path: the workspace holds fewer windows than the call has streams");
            r = seg_path(c, WS(c, "qnm"), b, sel.seg, *sel.path, i0, gx, s);
        } else if (sel.mix)
            r = seg_mix(c, q, b, sel.mix->at((size_t)b0), WS(c, "sel"), s);
        else if (sel.k > 0)
            r = seg_topk(c, q, b, sel.seg + b0, sel.k, sel.temperature, i0, sel.idx_k ? sel.idx_k + (size_t)b0 * sel.k : nullptr, nullptr,
                         sel.w_k ? sel.w_k + (size_t)b0 * sel.k : nullptr, WS(c, "sel"), s, al);
        else
            r = seg_match(c, q, b, sel.seg + b0, i0, gx, nullptr, s, al);
        if (r) return r;
        if (sel.literal())
            r = run_decoder(c, WS(c, "enc_s"), WS(c, "sel"), b, WS(c, "dec"), s);
        else
            r = run_decoder(c, WS(c, "enc_s"), nullptr, b, WS(c, "dec"), s, c->bank.enc, gx, c->bank.N,
                            c->bank.dec_valid ? c->bank.kin.p : nullptr, c->bank.dec_valid ? c->bank.gb.p : nullptr);
        if (r) return r;
        return run_to_mot(c, WS(c, "dec"), b, w.Y + b0 * ys, s, w.raw);
    });
}

// ... on workspace set 0, as the captured steps run it
static int characterize_segmented_set0(mocha_ctx* c, const SegWindows& w, const SegSelect& sel, hipStream_t s) {
    c->lane = 0;
    const int r = characterize_segmented_impl(c, w, sel, s);
    c->cur = 0;
    return r;
}

int mocha_characterize(mocha_ctx* c, const float* src_X, int B, const float* cnt_mean, const float* cnt_std, float* Y,
                       int32_t* idx, void* stream) {
    return characterize_impl(c, src_X, B, cnt_mean, cnt_std, Y, idx, stream, false);
}

int mocha_characterize_raw(mocha_ctx* c, const float* src_X_raw, int B, const float* cnt_mean, const float* cnt_std, float* Y,
                           int32_t* idx, void* stream) {
    return characterize_impl(c, src_X_raw, B, cnt_mean, cnt_std, Y, idx, stream, true);
}

// Demo pair in one pass (test_fullframework.py:188-194 for both clips, then :293-296, 438-443, 465-467): the character clip
// becomes the bank, the source clip is characterized against it.  Both clips go through mot_embedding / encoder / cnt in the
// same launches (twice the tiles per launch: less tile rounding, fewer prologue / epilogue phases); the bank lives in the
// workspace for the duration of the call and the context's own bank (mocha_bank_set) is left untouched.
static int characterize_pair_impl(mocha_ctx* c, const float* src_X, int B_src, const float* cha_X, int B_cha, const float* cnt_mean,
                                  const float* cnt_std, float* Y, int32_t* idx, float* cha_encoded, float* cha_cnt_nm, void* stream,
                                  bool raw, const PathArgs* path = nullptr) {
    if (!c) return MOCHA_ERR_ARG;
    if (B_src < 0 || B_cha < 1) return fail(c, MOCHA_ERR_ARG, "characterize_pair: needs B_src >= 0 and B_cha >= 1");
    const long long total = (long long)B_src + B_cha;
    if (total > c->max_chunk)
        return fail(c, MOCHA_ERR_ARG, "characterize_pair: %lld windows exceed the workspace limit of %d (raise it with mocha_reserve, or "
                    "use mocha_encode + mocha_bank_set + mocha_characterize)", total, c->max_chunk);
    int rc = ready(c, (int)total); if (rc) return rc;
    if (!cnt_mean || !cnt_std || !cha_X || (B_src > 0 && (!src_X || !Y))) return fail(c, MOCHA_ERR_ARG, "null argument");
    if (path && B_src > 0 && (rc = path_check(c, *path, B_src, B_cha, "mocha_characterize_pair_path"))) return rc;
    hipStream_t s = (hipStream_t)stream;
    c->cur = 0;
    const size_t T = 90 * 256;
    const int B = (int)total;
    // character windows first: rows [0, B_cha) of every buffer are the bank, rows [B_cha, B) the queries
    if ((rc = run_embed(c, cha_X, B_cha, WS(c, "x5"), true, s, raw, src_X, B_src))) return rc;
    if ((rc = run_encoder(c, WS(c, "x5"), B, WS(c, "enc_s"), s))) return rc;
    // The transient bank's decoder constants (IN(entry), gamma / beta of the character windows) depend on the encoder's output alone and
    // are needed by the decoder only: with "pair_overlap" they run on the context's internal stream BESIDE the matching chain (cnt, centroid,
    // norms, plane image, coarse GEMM, selection - small latency-bound launches), forked / joined with events (capture-safe, as for_chunks).
    const float *kin_t = nullptr, *gb_t = nullptr;
    bool forked = false;
    if (B_src > 0 && dec_cache_ok(c)) {
        hipStream_t cs = s;
        if (c->pair_overlap && c->aux) {
            HIPCHK(c, hipEventRecord(c->ev_fork, s));
            HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
            cs = c->aux; forked = true;
        }
        rc = build_dec_consts(c, WS(c, "enc_s"), B_cha, WS(c, "kin"), WS(c, "gb"), reinterpret_cast<double*>(WS(c, "smean64")),
                              reinterpret_cast<double*>(WS(c, "s1d")), B_cha, cs);
        if (forked) {                                     // join even when a launch failed: the caller's stream must not be left forked
            const hipError_t ej = hipEventRecord(c->ev_join, c->aux);
            if (!rc && ej != hipSuccess) rc = fail(c, MOCHA_ERR_HIP, "hipEventRecord: %s", hipGetErrorString(ej));
        }
        if (rc) { if (forked) (void)hipStreamWaitEvent(s, c->ev_join, 0); return rc; }
        kin_t = WS(c, "kin"); gb_t = WS(c, "gb");
    }
    auto join = [&]() -> int { if (forked) { forked = false; HIPCHK(c, hipStreamWaitEvent(s, c->ev_join, 0)); } return 0; };
    // everything between the fork and the join runs in a lambda: an early error return must not skip the join
    rc = [&]() -> int {
        const InormExtra iex0 = IEXW(c, s);
        LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, B * 90.0 * 256 * 4 * 2,
               launch_instnorm(WS(c, "enc_s"), nullptr, nullptr, cnt_mean, cnt_std, WS(c, "qnm"), B, 90, s, &iex0));
        if (cha_encoded) HIPCHK(c, hipMemcpyAsync(cha_encoded, WS(c, "enc_s"), (size_t)B_cha * T * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (cha_cnt_nm) HIPCHK(c, hipMemcpyAsync(cha_cnt_nm, WS(c, "qnm"), (size_t)B_cha * T * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }();
    if (rc) { (void)join(); return rc; }
    if (B_src == 0) return 0;
    // transient bank: c->pair borrows the workspace rows and keeps its own norms, centroid and packed plane image - the user's current
    // bank (c->bank) and what was derived from it are not touched
    int32_t* ix = idx ? idx : c->sets[0].idx_ws.p;
    if (path) {
        // coherent matching needs the rows themselves, none of the transient bank's derived data: the matrix against rows [0, B_cha) of the
        // workspace, then the path
        rc = path_match(c, WS(c, "qnm"), B_cha, WS(c, "qnm") + (size_t)B_cha * T, B_src, *path, ix, s);
    } else {
        rc = bank_set_impl(c, c->pair, WS(c, "qnm"), WS(c, "enc_s"), B_cha, MOCHA_BANK_BORROW, stream);
        if (!rc) rc = do_match(c, c->pair, WS(c, "qnm") + (size_t)B_cha * T, B_src, ix, nullptr, s);
        c->pair.cnt = c->pair.enc = nullptr; c->pair.N = 0;   // the workspace rows were lent for this call only
    }
    { const int rj = join(); if (!rc) rc = rj; }          // the decoder constants are complete (the caller's stream is never left forked)
    if (rc) return rc;
    // decoder on the matched character rows: the transient bank's encoded rows are rows [0, B_cha) of the workspace, their decoder
    // constants (as mocha_bank_set makes them for a user's bank) rows [0, B_cha) of "kin" / "gb"; read in place through the indices
    if ((rc = run_decoder(c, WS(c, "enc_s") + (size_t)B_cha * T, nullptr, B_src, WS(c, "dec"), s, WS(c, "enc_s"), ix, B_cha, kin_t, gb_t))) return rc;
    return run_to_mot(c, WS(c, "dec"), B_src, Y, s, raw);
}

int mocha_characterize_pair(mocha_ctx* c, const float* src_X, int B_src, const float* cha_X, int B_cha, const float* cnt_mean,
                            const float* cnt_std, float* Y, int32_t* idx, float* cha_encoded, float* cha_cnt_nm, void* stream) {
    return characterize_pair_impl(c, src_X, B_src, cha_X, B_cha, cnt_mean, cnt_std, Y, idx, cha_encoded, cha_cnt_nm, stream, false);
}

int mocha_characterize_pair_raw(mocha_ctx* c, const float* src_X_raw, int B_src, const float* cha_X_raw, int B_cha, const float* cnt_mean,
                                const float* cnt_std, float* Y, int32_t* idx, float* cha_encoded, float* cha_cnt_nm, void* stream) {
    return characterize_pair_impl(c, src_X_raw, B_src, cha_X_raw, B_cha, cnt_mean, cnt_std, Y, idx, cha_encoded, cha_cnt_nm, stream, true);
}

// ------------------------------------------------------------------------------------------- coherent context matching
// (include/mocha_hip.h "coherent context matching"; kernels in match_path.hip)
int mocha_match_dist_matrix(mocha_ctx* c, const float* query_nm, int Q, int64_t row0, int64_t rows, float* dist, int64_t ld, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if (Q < 0) return fail(c, MOCHA_ERR_ARG, "mocha_match_dist_matrix: negative query count");
    if (!c->bank.cnt || c->bank.N <= 0) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (rows < 1 || row0 < 0 || row0 > c->bank.N || rows > c->bank.N - row0)
        return fail(c, MOCHA_ERR_ARG, "mocha_match_dist_matrix: rows [%lld, %lld) are not a range of the bank's %lld", (long long)row0,
                    (long long)(row0 + rows), (long long)c->bank.N);
    if (rows > INT32_MAX) return fail(c, MOCHA_ERR_ARG, "mocha_match_dist_matrix: too many rows");
    if (ld < rows) return fail(c, MOCHA_ERR_ARG, "mocha_match_dist_matrix: ld < rows");
    if (Q == 0) return 0;
    if (!query_nm || !dist) return fail(c, MOCHA_ERR_ARG, "mocha_match_dist_matrix: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int D = 90 * 256;
    if ((rc = reserve(c, c->path_keys, match_dist_keys_words(Q, (int)rows)))) return rc;
    LAUNCH(c, s, "mocha_match_dist", "match.dist_matrix", 3.0 * Q * rows * D, ((Q + 7) / 8) * (double)rows * D * 4.0,
           launch_match_dist(c->bank.cnt + (size_t)row0 * D, query_nm, Q, (int)rows, D, c->path_keys.p, dist, ld, s));
    return 0;
}

int mocha_match_path(mocha_ctx* c, const float* dist, int Q, int N, int64_t ld, const int32_t* seq_start, int n_seq, const int32_t* bank_start,
                     int n_b, double lambda, int32_t* path, float* dist_out, unsigned char* continued, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (Q < 0) return fail(c, MOCHA_ERR_ARG, "mocha_match_path: negative window count");
    if (Q == 0) return 0;
    if (!dist || !path) return fail(c, MOCHA_ERR_ARG, "mocha_match_path: null argument");
    if (ld < N) return fail(c, MOCHA_ERR_ARG, "mocha_match_path: ld < N");
    PathArgs a; a.seq_start = seq_start; a.n_seq = n_seq; a.bank_start = bank_start; a.n_b = n_b; a.lambda = lambda; a.continued = continued;
    int rc = path_check(c, a, Q, N, "mocha_match_path"); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return path_run(c, dist, Q, N, ld, a, path, dist_out, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------- coherent matching, the online form
// (include/mocha_hip.h "coherent matching in live sessions"; kernels in match_path_step.hip)
int64_t mocha_path_state_bytes(const mocha_ctx* c, int streams, int state_rows) {
    if (!c || streams < 1 || streams > PATH_STEP_MAX_STREAMS || state_rows < 1 || state_rows > MATCH_PATH_MAX_ROWS) return MOCHA_ERR_ARG;
    return (int64_t)path_step_state_bytes(streams, state_rows);
}

int mocha_path_state_reset(mocha_ctx* c, void* state, int streams, int state_rows, const int32_t* which, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = path_step_check(c, "path_state_reset", streams, state_rows, 0.0); if (rc) return rc;
    if (!state) return fail(c, MOCHA_ERR_ARG, "path_state_reset: null argument");
    if (which && (n < 0 || n > streams)) return fail(c, MOCHA_ERR_ARG, "path_state_reset: n must be 0..streams");
    for (int i = 0; which && i < n; ++i)
        if (which[i] < 0 || which[i] >= streams) return fail(c, MOCHA_ERR_ARG, "path_state_reset: stream %d out of range 0..%d", (int)which[i], streams - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    // the headers alone: a stream that is not running never reads its R
    char* base = static_cast<char*>(state);
    if (!which) { HIPCHK(c, hipMemsetAsync(base, 0, (size_t)PATH_STEP_HDR_BYTES * streams, s)); return 0; }
    for (int i = 0; i < n; ++i) HIPCHK(c, hipMemsetAsync(base + (size_t)PATH_STEP_HDR_BYTES * which[i], 0, PATH_STEP_HDR_BYTES, s));
    return 0;
}

int mocha_match_path_advance(mocha_ctx* c, void* state, int streams, int state_rows, const float* dist, int64_t ld, const int32_t* ids,
                             const int32_t* rows, const uint32_t* start_bits, int64_t n_bits, const int32_t* bit_off, int32_t* restart, double lambda,
                             int32_t* idx, float* dist_out, unsigned char* continued, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = path_step_check(c, "match_path_advance", streams, state_rows, lambda); if (rc) return rc;
    if (!state || !dist || !ids || !rows || !idx) return fail(c, MOCHA_ERR_ARG, "match_path_advance: null argument");
    if (ld < 1) return fail(c, MOCHA_ERR_ARG, "match_path_advance: ld < 1");
    if (n_bits < 0 || (start_bits && n_bits < 1) || (!start_bits && bit_off)) return fail(c, MOCHA_ERR_ARG, "match_path_advance: start bits: a table of n_bits >= 1 bits, or none");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    PathStepArgs a{};
    a.state = state; a.streams = streams; a.state_rows = state_rows;
    a.ids = ids; a.rows = rows;
    a.start_bits = start_bits; a.n_bits = start_bits ? n_bits : 0; a.bit_off = bit_off;
    a.restart = restart; a.lambda = lambda;
    a.dist = dist; a.ld = ld;
    a.idx = idx; a.dist_out = dist_out; a.continued = continued;
    LAUNCH(c, s, "mocha_match_path_step", "match.path_step", 3.0 * streams * state_rows, 28.0 * streams * state_rows, launch_match_path_step(a, s));
    return 0;
}

int mocha_match_path_segmented(mocha_ctx* c, void* state, int streams, int state_rows, const float* query_nm, const int32_t* seg, int32_t* restart,
                               double lambda, int32_t* idx, float* dist, unsigned char* continued, float* dist_row, int64_t ld, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = path_step_check(c, "match_path_segmented", streams, state_rows, lambda); if (rc) return rc;
    if (!state || !query_nm || !seg || !idx) return fail(c, MOCHA_ERR_ARG, "match_path_segmented: null argument");
    if (dist_row && ld < state_rows) return fail(c, MOCHA_ERR_ARG, "match_path_segmented: ld < state_rows");
    if ((rc = ready(c, 0))) return rc;
    if ((rc = path_step_bank(c, "match_path_segmented", state_rows))) return rc;
    PathStepArg p; p.state = state; p.state_rows = state_rows; p.lambda = lambda; p.restart = restart; p.dist = dist; p.continued = continued;
    p.dist_row = dist_row; p.ld = ld;
    c->cur = 0;
    return seg_path(c, query_nm, streams, seg, p, idx, nullptr, (hipStream_t)stream);
}

int mocha_characterize_segmented_path(mocha_ctx* c, const float* src_X, int B, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                                      void* path_state, int state_rows, double lambda, int32_t* restart, float* Y, int32_t* idx, float* dist,
                                      unsigned char* continued, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = path_step_check(c, "characterize_segmented_path", B, state_rows, lambda); if (rc) return rc;
    if (!path_state || !seg) return fail(c, MOCHA_ERR_ARG, "characterize_segmented_path: null argument");
    if (c->bank.cnt && c->bank.segmented() && (rc = path_step_bank(c, "characterize_segmented_path", state_rows))) return rc;
    PathStepArg p; p.state = path_state; p.state_rows = state_rows; p.lambda = lambda; p.restart = restart; p.dist = dist; p.continued = continued;
    SegSelect sel; sel.seg = seg; sel.idx0 = idx; sel.path = &p;
    return characterize_segmented_impl(c, SegWindows{src_X, B, cnt_mean, cnt_std, Y, raw != 0}, sel, stream);
}

int mocha_bank_set_starts(mocha_ctx* c, const int64_t* starts, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    Bank& b = c->bank;
    if (b.resident) return fail(c, MOCHA_ERR_STATE, "bank_set_starts: a resident bank takes its starts per slot (mocha_bank_resident_set_starts)");
    if (!b.cnt || !b.segmented() || !b.start_bits.p) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (n < 0 || (n > 0 && !starts)) return fail(c, MOCHA_ERR_ARG, "bank_set_starts: a list or none");
    for (int i = 0; i < n; ++i) {
        if (starts[i] < 0 || starts[i] >= b.N) return fail(c, MOCHA_ERR_ARG, "bank_set_starts: start %lld outside the %lld rows", (long long)starts[i], (long long)b.N);
        if (i && starts[i] <= starts[i - 1]) return fail(c, MOCHA_ERR_ARG, "bank_set_starts: starts must increase strictly");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> l32(starts, starts + n);
    int rc = reserve(c, b.start_list, (size_t)std::max(n, 1)); if (rc) return rc;
    // (pageable host memory: the copy is staged before the call returns)
    if (n > 0) HIPCHK(c, hipMemcpyAsync(b.start_list.p, l32.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LAUNCH(c, s, "mocha_path_starts", "bank.starts", 0.0, b.N / 8.0 + 4.0 * n, launch_path_starts(b.start_bits.p, b.N, 0, b.N, b.start_list.p, n, nullptr, s));
    return 0;
}

int mocha_bank_resident_set_starts(mocha_ctx* c, int slot, const int32_t* starts, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    Bank& b = c->bank;
    if (!b.resident) return fail(c, MOCHA_ERR_STATE, "bank_resident_set_starts: no resident bank: call mocha_bank_resident_create first");
    if (slot < 0 || slot >= b.segments()) return fail(c, MOCHA_ERR_ARG, "bank_resident_set_starts: slot %d out of range 0 .. %d", slot, b.segments() - 1);
    if (!b.slot[slot].rows) return fail(c, MOCHA_ERR_STATE, "bank_resident_set_starts: slot %d is empty", slot);
    if (n < 0 || (n > 0 && !starts)) return fail(c, MOCHA_ERR_ARG, "bank_resident_set_starts: a list or none");
    const int64_t rows = b.slot[slot].rows;
    for (int i = 0; i < n; ++i) {
        if (starts[i] < 0 || starts[i] >= rows) return fail(c, MOCHA_ERR_ARG, "bank_resident_set_starts: start %d outside the character's %lld rows", (int)starts[i], (long long)rows);
        if (i && starts[i] <= starts[i - 1]) return fail(c, MOCHA_ERR_ARG, "bank_resident_set_starts: starts must increase strictly");
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int rc = reserve(c, b.start_list, (size_t)std::max(n, 1)); if (rc) return rc;
    if (n > 0) HIPCHK(c, hipMemcpyAsync(b.start_list.p, starts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    LAUNCH(c, s, "mocha_path_starts", "bank.starts", 0.0, rows / 8.0 + 4.0 * n,
           launch_path_starts(b.start_bits.p, b.N, b.slot[slot].first, rows, b.start_list.p, n, nullptr, s));
    return 0;
}

// mocha_characterize with the path in the matcher's place.  The path spans the whole batch, so the batch goes through the workspace
// twice: encoder, z-score and matrix rows chunk by chunk, the path, then the decoder and to_mot chunk by chunk (a batch of more than one
// chunk runs its embedding and encoder again for the second pass - the workspace holds one chunk's encoder output).
int mocha_characterize_path(mocha_ctx* c, const float* src_X, int B, const float* cnt_mean, const float* cnt_std, const int32_t* seq_start,
                            int n_seq, const int32_t* bank_start, int n_b, double lambda, int relative, float* Y, int32_t* idx,
                            unsigned char* continued, int raw_, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_characterize_path"))) return rc;
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (B == 0) return 0;
    if (!cnt_mean || !cnt_std || !src_X || !Y) return fail(c, MOCHA_ERR_ARG, "null argument");
    PathArgs a; a.seq_start = seq_start; a.n_seq = n_seq; a.bank_start = bank_start; a.n_b = n_b; a.lambda = lambda; a.continued = continued;
    a.relative = relative != 0;
    const int64_t N = c->bank.N;
    if ((rc = path_check(c, a, B, N, "mocha_characterize_path"))) return rc;
    const bool raw = raw_ != 0;
    const size_t ys = (size_t)60 * c->cfg.V * c->cfg.C_in;
    const size_t xs = raw ? (size_t)60 * (c->cfg.V + 1) * c->cfg.C_in : ys;
    const int D = 90 * 256;
    if ((rc = reserve(c, c->path_d, (size_t)B * N))) return rc;
    if ((rc = reserve(c, c->path_m, (size_t)2 * B))) return rc;      // (Q minima, then the path when the caller wants no indices)
    if ((rc = reserve(c, c->path_keys, match_dist_keys_words(B, (int)N)))) return rc;      // (per chunk its own keys: two chunks may be in flight)
    unsigned long long* keys = c->path_keys.p;
    int chunks = 0;
    auto encode = [&](int b0, int b, hipStream_t s) -> int {
        int r;
        if ((r = run_embed(c, src_X + b0 * xs, b, WS(c, "x5"), true, s, raw))) return r;
        return run_encoder(c, WS(c, "x5"), b, WS(c, "enc_s"), s);
    };
    rc = for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        ++chunks;
        if ((r = encode(b0, b, s))) return r;
        const InormExtra ex = IEXW(c, s);
        LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, b * 90.0 * 256 * 4 * 2.0, launch_instnorm(WS(c, "enc_s"), nullptr, nullptr, cnt_mean, cnt_std, WS(c, "qnm"), b, 90, s, &ex));
        LAUNCH(c, s, "mocha_match_dist", "match.dist_matrix", 3.0 * b * N * D, ((b + 7) / 8) * (double)N * D * 4.0,
               launch_match_dist(c->bank.cnt, WS(c, "qnm"), b, (int)N, D, keys + (size_t)b0 * N, c->path_d.p + (size_t)b0 * N, N, s));
        return 0;
    });
    if (rc) return rc;
    hipStream_t s0 = (hipStream_t)stream;
    int32_t* ix = idx ? idx : c->path_m.p + B;
    if ((rc = path_run(c, c->path_d.p, B, (int)N, N, a, ix, nullptr, s0))) return rc;
    const bool again = chunks > 1;
    return for_chunks(c, B, s0, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        if (again && (r = encode(b0, b, s))) return r;
        if ((r = run_decoder(c, WS(c, "enc_s"), nullptr, b, WS(c, "dec"), s, c->bank.enc, ix + b0, c->bank.N,
                             c->bank.dec_valid ? c->bank.kin.p : nullptr, c->bank.dec_valid ? c->bank.gb.p : nullptr))) return r;
        return run_to_mot(c, WS(c, "dec"), b, Y + b0 * ys, s, raw);
    });
}

int mocha_characterize_pair_path(mocha_ctx* c, const float* src_X, int B_src, const float* cha_X, int B_cha, const float* cnt_mean,
                                 const float* cnt_std, const int32_t* seq_start, int n_seq, const int32_t* bank_start, int n_b, double lambda,
                                 int relative, float* Y, int32_t* idx, unsigned char* continued, float* cha_encoded, float* cha_cnt_nm, int raw,
                                 void* stream) {
    PathArgs a; a.seq_start = seq_start; a.n_seq = n_seq; a.bank_start = bank_start; a.n_b = n_b; a.lambda = lambda; a.continued = continued;
    a.relative = relative != 0;
    return characterize_pair_impl(c, src_X, B_src, cha_X, B_cha, cnt_mean, cnt_std, Y, idx, cha_encoded, cha_cnt_nm, stream, raw != 0, &a);
}

// ------------------------------------------------------------------------------------------- captured per-window step
// BASELINE configs[4]: a clip streamed one 60-frame window per step.  The whole step (mot_embedding, +pos_emb, encoder, cnt,
// z-score, bank scan, gather, decoder, to_mot: test_fullframework.py:438-443, 465-467) is captured once into a HIP graph and
// replayed; the graph is keyed on the buffer pointers and on the context generation, and re-captured when either changes.
}  // extern "C"

namespace {
// Replay `g`, capturing it first when its key or the context generation changed: `body(stream)` enqueues the step's launches on the capture
// stream (mocha_step_graph_lane, mocha_step_graph_segmented).  The caller made sure that nothing inside `body` allocates.
template <class F>
int step_replay(mocha_ctx* c, mocha_ctx::StepGraph& g, const mocha_ctx::StepKey& key, hipStream_t s, F&& body) {
    if (!step_holds(c, g, key)) {
        if (c->prof_on) return fail(c, MOCHA_ERR_STATE, "mocha_step_graph: stop profiling before capturing");
        if (!c->cap_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
        if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
        if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; }
        const int64_t gen0 = c->generation;
        HIPCHK(c, hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeRelaxed));
        int rc = body(c->cap_stream);
        hipGraph_t graph = nullptr;
        const hipError_t ee = hipStreamEndCapture(c->cap_stream, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        if (ee != hipSuccess) return fail(c, MOCHA_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(ee));
        if (c->generation != gen0) { (void)hipGraphDestroy(graph); return fail(c, MOCHA_ERR_STATE, "a buffer was replaced during capture"); }
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (ei != hipSuccess) { (void)hipGraphDestroy(graph); return fail(c, MOCHA_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ei)); }
        g.exec = exec; g.graph = graph; g.key = key; g.generation = c->generation;
    }
    HIPCHK(c, hipGraphLaunch(g.exec, s));
    return 0;
}

// The captured segmented step of up to 16 windows, every variant (`what` names the entry point in its messages): the shared checks, then
// graph `kind` replayed, keyed on `key` (the caller filled the variant's own fields) and the windows' pointers.  outputs_ok: the variant's
// required outputs are there.  Ids, masks and weights are read by the captured kernels on every replay: their contents are not part of
// the key; k, the temperature and J are.
int step_segmented(mocha_ctx* c, const char* what, mocha_ctx::StepKind kind, mocha_ctx::StepKey key, const SegWindows& w, const SegSelect& sel,
                   bool outputs_ok, void* stream) {
    if (w.B < 1 || w.B > 16) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= S_w <= 16 windows", what);
    int rc = ready(c, w.B); if (rc) return rc;
    if (!w.X || !sel.ids() || (sel.mix && !sel.mix->weights) || (sel.allow && !sel.allow->allow) || !w.cnt_mean || !w.cnt_std || !w.Y || !outputs_ok)
        return fail(c, MOCHA_ERR_ARG, "null argument");
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (sel.allow && !c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    key.x = w.X; key.mean = w.cnt_mean; key.sd = w.cnt_std; key.y = w.Y; key.seg = sel.ids(); key.windows = w.B; key.raw = w.raw;
    mocha_ctx::StepGraph& g = c->steps[kind];
    auto body = [&](hipStream_t cs) -> int { return characterize_segmented_set0(c, w, sel, cs); };
    if (sel.literal() && !step_holds(c, g, key)) {
        // Before a capture: the step once, eagerly, so that whatever its kernels make on first use - the plane GEMMs' weight images, the
        // float64 weights of the literal decoder's style MLP - exists; it writes what the replay then writes again.  (The hard step is
        // captured as it comes.)
        if ((rc = body((hipStream_t)stream))) return rc;
    }
    return step_replay(c, g, key, (hipStream_t)stream, body);
}
}  // namespace

extern "C" {

int mocha_step_graph_lane(mocha_ctx* c, int lane, const float* X1, const float* cnt_mean, const float* cnt_std, float* Y1, int32_t* idx,
                          int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (lane < 0 || lane >= c->lanes) return fail(c, MOCHA_ERR_ARG, "lane %d: the context has %d lane(s) (mocha_set_option \"lanes\")", lane, c->lanes);
    int rc = ready(c, 1); if (rc) return rc;
    if (!X1 || !cnt_mean || !cnt_std || !Y1 || !idx) return fail(c, MOCHA_ERR_ARG, "null argument");
    if ((rc = refuse_resident(c, "mocha_step_graph"))) return rc;
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (c->sets[lane].ws.empty()) return fail(c, MOCHA_ERR_STATE, "lane %d has no workspace", lane);
    mocha_ctx::StepKey key; key.x = X1; key.mean = cnt_mean; key.sd = cnt_std; key.y = Y1; key.idx = idx; key.raw = raw != 0;
    mocha_ctx::StepGraph& g = c->steps[mocha_ctx::STEP_LANE + lane];
    if (!step_holds(c, g, key)) {
        // make sure nothing inside the captured region allocates (scratch for one query against the current bank)
        if ((rc = ensure_match_scratch(c, lane, 8, c->bank, true))) return rc;
    }
    return step_replay(c, g, key, (hipStream_t)stream, [&](hipStream_t cs) -> int {
        c->lane = lane;                                   // the step's kernels use this lane's workspace set and match scratch
        const int r = characterize_impl(c, X1, 1, cnt_mean, cnt_std, Y1, idx, cs, raw != 0);
        c->lane = 0; c->cur = 0;
        return r;
    });
}

int mocha_step_graph(mocha_ctx* c, const float* X1, const float* cnt_mean, const float* cnt_std, float* Y1, int32_t* idx,
                     int raw, void* stream) {
    return mocha_step_graph_lane(c, 0, X1, cnt_mean, cnt_std, Y1, idx, raw, stream);
}

// ------------------------------------------------------------------------------------------- multi-character bank
// N characters' banks as N row segments of one bank (rows z-scored with the same global cnt_mean / cnt_std); a batch names, per window,
// the segment it is matched against (device data).  Encoding, z-score, gather, decoder and to_mot are those of mocha_characterize; only
// the matcher is segmented (match_segmented.hip).
int mocha_bank_set_segments(mocha_ctx* c, const float* cnt_nm, const float* encoded, int64_t N, const int64_t* seg_start, int S, int flags,
                            void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (!seg_start || S < 1) return fail(c, MOCHA_ERR_ARG, "bank_set_segments: needs S >= 1 segments and seg_start (S + 1 entries)");
    if (seg_start[0] != 0 || seg_start[S] != N) return fail(c, MOCHA_ERR_ARG, "bank_set_segments: seg_start must run from 0 to N = %lld", (long long)N);
    for (int i = 0; i < S; ++i)
        if (seg_start[i + 1] <= seg_start[i]) return fail(c, MOCHA_ERR_ARG, "bank_set_segments: segment %d is empty or seg_start decreases", i);
    int rc = bank_set_impl(c, c->bank, cnt_nm, encoded, N, flags, stream);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = [&]() -> int {
        int64_t mx = 0;
        std::vector<int> dev32(S + 1);
        for (int i = 0; i <= S; ++i) dev32[i] = (int)seg_start[i];
        for (int i = 0; i < S; ++i) mx = std::max<int64_t>(mx, seg_start[i + 1] - seg_start[i]);
        { int r = reserve(c, c->bank.seg_dev, (size_t)S + 1); if (r) return r; }
        HIPCHK(c, hipMemcpyAsync(c->bank.seg_dev.p, dev32.data(), sizeof(int) * (S + 1), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));                  // (the host vector goes out of scope)
        c->bank.seg_start.assign(seg_start, seg_start + S + 1);
        c->bank.seg_max_rows = mx;
        // launches of up to seg_q queries: the workspace's windows, and at least the 16 windows of mocha_step_graph_segmented
        c->seg_q = std::min(SEG_MAX_Q, std::max(set_windows(c, 0), 16));
        for (int set = 0; set < mocha_ctx::MAX_SETS; ++set) {
            int r;
            if ((set == 0 || !c->sets[set].ws.empty()) && (r = ensure_seg_scratch(c, set))) return r;
        }
        return path_tables_zeroed(c, c->bank, N, S, s);
    }();
    if (rc) { c->bank.seg_start.clear(); c->bank.seg_max_rows = 0; }
    return rc;
}

int mocha_match_segmented(mocha_ctx* c, const float* query_nm, int Q, const int32_t* seg, int32_t* idx, float* dist, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if (!query_nm || !seg || !idx || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad match_segmented arguments");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (Q == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    return for_centred_queries(c, query_nm, Q, s, [&](const float* q, int q0, int n) -> int {
        return seg_match(c, q, n, seg + q0, idx + q0, nullptr, dist ? dist + q0 : nullptr, s);
    });
}

int mocha_characterize_segmented(mocha_ctx* c, const float* src_X, int B, const int32_t* seg, const float* cnt_mean, const float* cnt_std,
                                 float* Y, int32_t* idx, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (B > 0 && !seg) return fail(c, MOCHA_ERR_ARG, "characterize_segmented: null argument");
    SegSelect sel; sel.seg = seg; sel.idx0 = idx;
    return characterize_segmented_impl(c, SegWindows{src_X, B, cnt_mean, cnt_std, Y, raw != 0}, sel, stream);
}

int mocha_step_graph_segmented(mocha_ctx* c, const float* X, int S_w, const int32_t* seg, const float* cnt_mean, const float* cnt_std, float* Y,
                               int32_t* idx, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    SegSelect sel; sel.seg = seg; sel.idx0 = idx;
    mocha_ctx::StepKey key; key.idx = idx;
    return step_segmented(c, "step_graph_segmented", mocha_ctx::STEP_SEG, key, SegWindows{X, S_w, cnt_mean, cnt_std, Y, raw != 0}, sel,
                          idx != nullptr, stream);
}

// ------------------------------------------------------------------------------------------- soft matching, multi-character bank
// The decoder's character feature as the softmax-weighted blend of the k nearest entries of the window's own segment instead of the one
// nearest entry: nothing trained, and no pop when two entries are nearly equidistant.  The matcher is match_seg_topk.hip; the decoder runs
// on the blended feature itself (characterize_segmented_impl with k >= 1).
static_assert(MOCHA_SOFT_MAX_K == SEG_TOPK_MAX_K, "the header's k limit is the kernel's");
static int soft_args(mocha_ctx* c, const char* what, int k, float temperature) {
    if (k < 1 || k > MOCHA_SOFT_MAX_K) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= k <= %d neighbours", what, MOCHA_SOFT_MAX_K);
    if (!(temperature > 0.f)) return fail(c, MOCHA_ERR_ARG, "%s: temperature must be positive", what);
    return 0;
}

int mocha_match_topk_segmented(mocha_ctx* c, const float* query_nm, int Q, const int32_t* seg, int k, int32_t* idx, float* dist, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = soft_args(c, "match_topk_segmented", k, 1.f); if (rc) return rc;
    if ((rc = ready(c, 0))) return rc;
    if (!query_nm || !seg || !idx || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad match_topk_segmented arguments");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (Q == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    return for_centred_queries(c, query_nm, Q, s, [&](const float* q, int q0, int n) -> int {
        return seg_topk(c, q, n, seg + q0, k, 1.f, nullptr, idx + (size_t)q0 * k, dist ? dist + (size_t)q0 * k : nullptr, nullptr, nullptr, s);
    });
}

int mocha_characterize_soft_segmented(mocha_ctx* c, const float* src_X, int B, const int32_t* seg, int k, float temperature, const float* cnt_mean,
                                      const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = soft_args(c, "characterize_soft_segmented", k, temperature); if (rc) return rc;
    if (B > 0 && !seg) return fail(c, MOCHA_ERR_ARG, "characterize_soft_segmented: null argument");
    SegSelect sel; sel.seg = seg; sel.k = k; sel.temperature = temperature; sel.idx_k = idx_k; sel.w_k = w_k;
    return characterize_segmented_impl(c, SegWindows{src_X, B, cnt_mean, cnt_std, Y, raw != 0}, sel, stream);
}

int mocha_step_graph_soft_segmented(mocha_ctx* c, const float* X, int S_w, const int32_t* seg, int k, float temperature, const float* cnt_mean,
                                    const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = soft_args(c, "step_graph_soft_segmented", k, temperature); if (rc) return rc;
    SegSelect sel; sel.seg = seg; sel.k = k; sel.temperature = temperature; sel.idx_k = idx_k; sel.w_k = w_k;
    mocha_ctx::StepKey key; key.soft_k = k; key.soft_t = temperature; key.soft[0] = idx_k; key.soft[1] = w_k;
    return step_segmented(c, "step_graph_soft_segmented", mocha_ctx::STEP_SEG_SOFT, key, SegWindows{X, S_w, cnt_mean, cnt_std, Y, raw != 0}, sel,
                          idx_k && w_k, stream);
}

// ------------------------------------------------------------------------------------------- character mixing, multi-character bank
// A window characterized by up to MOCHA_MIX_MAX (character, six body-part weights) components: each present component is matched exactly in
// its own character, and the decoder runs on the part-wise weighted blend of the matched entries (characterize_segmented_impl with a MixArg).
// The matcher is match_seg_mix.hip; ids and weights are device data every launch and replay reads.
static_assert(MOCHA_MIX_MAX == SEG_MIX_MAX_J, "the header's component limit is the kernel's");
static int mix_args(mocha_ctx* c, const char* what, int J) {
    if (J < 1 || J > MOCHA_MIX_MAX) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= J <= %d components", what, MOCHA_MIX_MAX);
    return 0;
}

int mocha_match_mix_segmented(mocha_ctx* c, const float* query_nm, int Q, const int32_t* ids, const float* weights, int J, int32_t* idx,
                              float* dist, float* wnorm, float* out, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = mix_args(c, "match_mix_segmented", J); if (rc) return rc;
    if ((rc = ready(c, 0))) return rc;
    if (!query_nm || !ids || !weights || !idx || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad match_mix_segmented arguments");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (Q == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const MixArg mx{ids, weights, J, idx, dist, wnorm, nullptr, nullptr};
    return for_centred_queries(c, query_nm, Q, s, [&](const float* q, int q0, int n) -> int {
        return seg_mix(c, q, n, mx.at((size_t)q0), out ? out + (size_t)q0 * 90 * 256 : nullptr, s);
    });
}

int mocha_characterize_mix_segmented(mocha_ctx* c, const float* src_X, int B, const int32_t* ids, const float* weights, int J,
                                     const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx, float* wnorm, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = mix_args(c, "characterize_mix_segmented", J); if (rc) return rc;
    if (B > 0 && (!ids || !weights)) return fail(c, MOCHA_ERR_ARG, "characterize_mix_segmented: null argument");
    const MixArg mx{ids, weights, J, idx, nullptr, wnorm, nullptr, nullptr};
    SegSelect sel; sel.mix = &mx;
    return characterize_segmented_impl(c, SegWindows{src_X, B, cnt_mean, cnt_std, Y, raw != 0}, sel, stream);
}

int mocha_step_graph_mix_segmented(mocha_ctx* c, const float* X, int S_w, const int32_t* ids, const float* weights, int J, const float* cnt_mean,
                                   const float* cnt_std, float* Y, int32_t* idx, float* wnorm, int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = mix_args(c, "step_graph_mix_segmented", J); if (rc) return rc;
    const MixArg mx{ids, weights, J, idx, nullptr, wnorm, nullptr, nullptr};
    SegSelect sel; sel.mix = &mx;
    mocha_ctx::StepKey key; key.idx = idx; key.mix_j = J; key.mix[0] = weights; key.mix[1] = wnorm;
    return step_segmented(c, "step_graph_mix_segmented", mocha_ctx::STEP_SEG_MIX, key, SegWindows{X, S_w, cnt_mean, cnt_std, Y, raw != 0}, sel,
                          idx && wnorm, stream);
}

// ------------------------------------------------------------------------------------------- action-constrained matching
// Every row of a multi-character bank carries an action label 0..63 (mocha_bank_set_labels), every query a 64-bit allow mask: the match is
// the exact nearest neighbour(s) among the rows of the query's segment whose label is allowed; a zero mask, or one that names no label the
// segment holds, takes the plain answer (match_seg_body.h, the ALLOW scans).  The calls below are the segmented ones with an AllowArg.
int mocha_bank_set_labels(mocha_ctx* c, const int32_t* labels, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (c->bank.resident) return fail(c, MOCHA_ERR_STATE, "bank_set_labels: a resident bank takes its labels with mocha_bank_resident_add");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    HIPCHK(c, hipSetDevice(c->device));
    if (!labels) { c->bank.labelled = false; c->generation++; return 0; }
    const int S = c->bank.segments();
    const int64_t N = c->bank.N;
    for (int64_t i = 0; i < N; ++i)
        if (labels[i] < 0 || labels[i] > 63) return fail(c, MOCHA_ERR_ARG, "bank_set_labels: label %d of row %lld is outside 0..63", (int)labels[i], (long long)i);
    std::vector<unsigned char> lab((size_t)N);
    std::vector<unsigned long long> any((size_t)S, 0ull), gran;
    std::vector<int> gstart((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) {
        const int64_t lo = c->bank.seg_start[s], n = c->bank.seg_start[s + 1] - lo;
        gstart[s + 1] = gstart[s] + (int)((n + SEG_GRANULE_ROWS - 1) / SEG_GRANULE_ROWS);
        gran.resize((size_t)gstart[s + 1], 0ull);
        for (int64_t r = 0; r < n; ++r) {
            const unsigned long long bit = 1ull << labels[lo + r];
            lab[(size_t)(lo + r)] = (unsigned char)labels[lo + r];
            any[s] |= bit;
            gran[(size_t)gstart[s] + (size_t)(r / SEG_GRANULE_ROWS)] |= bit;
        }
    }
    // everything a constrained call reads exists from here on: none of them allocates (their scratch is the segmented matcher's)
    c->bank.labelled = false;
    int rc = reserve(c, c->bank.lab_dev, lab.size());
    if (!rc) rc = reserve(c, c->bank.lab_any, any.size());
    if (!rc) rc = reserve(c, c->bank.lab_gran, gran.size());
    if (!rc) rc = reserve(c, c->bank.lab_gran_start, gstart.size());
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipMemcpyAsync(c->bank.lab_dev.p, lab.data(), lab.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->bank.lab_any.p, any.data(), any.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->bank.lab_gran.p, gran.data(), gran.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->bank.lab_gran_start.p, gstart.data(), gstart.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));                  // (the host vectors go out of scope)
    c->bank.labelled = true;
    c->generation++;                                     // a captured constrained step has the previous tables baked in
    return 0;
}

int mocha_match_segmented_allow(mocha_ctx* c, const float* query_nm, int Q, const int32_t* seg, const uint64_t* allow, int k, int32_t* idx,
                                float* dist, int32_t* applied, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (k < 1 || k > MOCHA_SOFT_MAX_K) return fail(c, MOCHA_ERR_ARG, "match_segmented_allow: 1 <= k <= %d neighbours", MOCHA_SOFT_MAX_K);
    int rc = ready(c, 0); if (rc) return rc;
    if (!query_nm || !seg || !allow || !idx || Q < 0) return fail(c, MOCHA_ERR_ARG, "bad match_segmented_allow arguments");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    if (!c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    if (Q == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const AllowArg al{reinterpret_cast<const unsigned long long*>(allow), applied};
    // k = 1: the hard matcher; k >= 2: the top-k matcher
    return for_centred_queries(c, query_nm, Q, s, [&](const float* q, int q0, int n) -> int {
        const AllowArg a = al.at(q0);
        if (k == 1) return seg_match(c, q, n, seg + q0, idx + q0, nullptr, dist ? dist + q0 : nullptr, s, &a);
        return seg_topk(c, q, n, seg + q0, k, 1.f, nullptr, idx + (size_t)q0 * k, dist ? dist + (size_t)q0 * k : nullptr, nullptr, nullptr, s, &a);
    });
}

int mocha_characterize_segmented_allow(mocha_ctx* c, const float* src_X, int B, const int32_t* seg, const uint64_t* allow, int k, float temperature,
                                       const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int32_t* applied,
                                       int raw, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (k != 0) { int rc = soft_args(c, "characterize_segmented_allow", k, temperature); if (rc) return rc; }
    if (B > 0 && (!seg || !allow)) return fail(c, MOCHA_ERR_ARG, "characterize_segmented_allow: null argument");
    if (c->bank.segmented() && !c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    const AllowArg al{reinterpret_cast<const unsigned long long*>(allow), applied};
    SegSelect sel; sel.seg = seg; sel.allow = &al; sel.k = k; sel.temperature = temperature; sel.w_k = w_k;
    if (k == 0) sel.idx0 = idx_k; else sel.idx_k = idx_k;      // k = 0: the hard characterize, idx_k holds one entry per window and w_k is unused
    return characterize_segmented_impl(c, SegWindows{src_X, B, cnt_mean, cnt_std, Y, raw != 0}, sel, stream);
}

int mocha_step_graph_segmented_allow(mocha_ctx* c, const float* X, int S_w, const int32_t* seg, const uint64_t* allow, int k, float temperature,
                                     const float* cnt_mean, const float* cnt_std, float* Y, int32_t* idx_k, float* w_k, int32_t* applied, int raw,
                                     void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (k != 0) { int rc = soft_args(c, "step_graph_segmented_allow", k, temperature); if (rc) return rc; }
    const AllowArg al{reinterpret_cast<const unsigned long long*>(allow), applied};
    mocha_ctx::StepKey key;
    key.soft_k = k; key.soft_t = k > 0 ? temperature : 0.f; key.soft[0] = idx_k; key.soft[1] = k > 0 ? w_k : nullptr;
    key.allow[0] = allow; key.allow[1] = applied;
    SegSelect sel; sel.seg = seg; sel.allow = &al; sel.k = k; sel.temperature = temperature; sel.w_k = w_k;
    if (k == 0) sel.idx0 = idx_k; else sel.idx_k = idx_k;      // k = 0: the hard characterize, idx_k holds one entry per window and w_k is unused
    return step_segmented(c, "step_graph_segmented_allow", mocha_ctx::STEP_SEG_ALLOW, key, SegWindows{X, S_w, cnt_mean, cnt_std, Y, raw != 0}, sel,
                          idx_k && (k == 0 || w_k), stream);
}

// ------------------------------------------------------------------------------------------- resident multi-character bank
// A multi-character bank whose storage, tables and scratch are reserved ONCE: characters are added to and retired from it by calls that
// only enqueue work on the caller's stream.  On an fp32 bank a row's distance depends on no other row, the decoder constants are per
// entry and the label tables per row / 16 rows / character: what ties the characters of mocha_bank_set_segments together is only its
// contiguous seg_start table and the host values baked into launches.  Here the kernels read a slot table ({first row, rows} per slot,
// device data; match_seg_body.h, PAIRS) and the launches are shaped by the two reserved maxima, so the captured graphs of the segmented
// and live steps keep replaying across add / retire: the generation does not move.
static int64_t granule_units(int64_t rows) { return (rows + SEG_GRANULE_ROWS - 1) / SEG_GRANULE_ROWS; }

int mocha_bank_resident_create(mocha_ctx* c, int64_t capacity_rows, int max_characters, int64_t max_rows_per_character, int flags, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if (flags & (MOCHA_BANK_BF16 | MOCHA_BANK_BORROW))
        return fail(c, MOCHA_ERR_ARG, "bank_resident_create: a resident bank is fp32 and owns its rows (no MOCHA_BANK_BF16, no MOCHA_BANK_BORROW)");
    if (capacity_rows < 1 || capacity_rows > (int64_t)1 << 30 || max_characters < 1 || max_characters > 1 << 20 || max_rows_per_character < 1 ||
        max_rows_per_character > capacity_rows)
        return fail(c, MOCHA_ERR_ARG, "bank_resident_create: needs 1 <= max_rows_per_character <= capacity_rows <= 2^30 and 1 <= max_characters <= 2^20");
    const int64_t cap = granule_units(capacity_rows) * SEG_GRANULE_ROWS;
    const size_t D = 90 * 256;
    const int L = c->cfg.dec_depth;
    hipStream_t s = (hipStream_t)stream;
    Bank& b = c->bank;
    // from here on the previous bank is gone; a failure below leaves the context without a current bank
    b.cnt = nullptr; b.enc = nullptr; b.N = 0;
    b.seg_start.clear(); b.seg_max_rows = 0; b.labelled = false; b.resident = false; b.slot.clear();
    b.is_bf16 = false;
    b.tiled_valid = false; b.tile32_valid = false; b.x3_valid = false; b.b16f_valid = false; b.b8_valid = false; b.dec_valid = false; b.amax_ok = false;
    c->generation++;                                      // a captured step has the previous bank's pointers and shapes baked in
    if ((rc = bank_own_rows(c, b, cap))) return rc;
    HIPCHK(c, hipMemsetAsync(b.cnt_own.p, 0, (size_t)cap * D * sizeof(float), s));
    HIPCHK(c, hipMemsetAsync(b.enc_own.p, 0, (size_t)cap * D * sizeof(float), s));
    // the decoder constants of every row the bank can hold; without the memory the decoder computes them per call, as for any bank
    if (dec_cache_ok(c) && !(flags & MOCHA_BANK_NO_DEC_CACHE)) {
        if (b.kin.reserve((size_t)cap * D) != hipSuccess || b.gb.reserve((size_t)cap * 512 * L) != hipSuccess) {
            (void)hipGetLastError();                      // the failed allocation's sticky error
            b.kin.release(); b.gb.release();
        } else {
            const size_t rows = (size_t)std::min<int64_t>(max_rows_per_character, 4096);
            if ((rc = reserve(c, c->style_scratch, rows * (256 + (size_t)512 * L)))) return rc;
            HIPCHK(c, hipMemsetAsync(b.kin.p, 0, (size_t)cap * D * sizeof(float), s));
            HIPCHK(c, hipMemsetAsync(b.gb.p, 0, (size_t)cap * 512 * L * sizeof(float), s));
            b.dec_valid = true;
        }
    }
    if (c->gemm_h2) {
        if ((rc = reserve(c, b.amax, (size_t)cap))) return rc;
        HIPCHK(c, hipMemsetAsync(b.amax.p, 0, (size_t)cap * sizeof(float), s));
        b.amax_ok = true;
    }
    // label bytes, granule words (one per 16 rows of the BANK: a character's words start at first row / 16), per-slot any and gran_start,
    // and the slot table - all zero: every slot empty
    const size_t S = (size_t)max_characters, G = (size_t)(cap / SEG_GRANULE_ROWS);
    if ((rc = reserve(c, b.lab_dev, (size_t)cap))) return rc;
    if ((rc = reserve(c, b.lab_any, S))) return rc;
    if ((rc = reserve(c, b.lab_gran, G))) return rc;
    if ((rc = reserve(c, b.lab_gran_start, S + 1))) return rc;
    if ((rc = reserve(c, b.seg_dev, 2 * S))) return rc;
    HIPCHK(c, hipMemsetAsync(b.lab_dev.p, 0, (size_t)cap, s));
    HIPCHK(c, hipMemsetAsync(b.lab_any.p, 0, S * sizeof(unsigned long long), s));
    HIPCHK(c, hipMemsetAsync(b.lab_gran.p, 0, G * sizeof(unsigned long long), s));
    HIPCHK(c, hipMemsetAsync(b.lab_gran_start.p, 0, (S + 1) * sizeof(int), s));
    HIPCHK(c, hipMemsetAsync(b.seg_dev.p, 0, 2 * S * sizeof(int), s));
    if ((rc = path_tables_zeroed(c, b, cap, (int)S, s))) return rc;
    b.slot.assign(S, Bank::Slot{});
    b.extents.reset(cap / SEG_GRANULE_ROWS);
    b.seg_max_rows = max_rows_per_character;
    b.resident = true;
    // the segmented matcher's scratch of every workspace set, for the two reserved maxima
    c->seg_q = std::min(SEG_MAX_Q, std::max(set_windows(c, 0), 16));
    for (int set = 0; set < mocha_ctx::MAX_SETS; ++set)
        if ((set == 0 || !c->sets[set].ws.empty()) && (rc = ensure_seg_scratch(c, set))) { b.resident = false; b.slot.clear(); b.seg_max_rows = 0; return rc; }
    b.cnt = b.cnt_own.p; b.enc = b.enc_own.p; b.N = cap;
    b.labelled = true;
    return 0;
}

int mocha_bank_resident_add(mocha_ctx* c, int slot, const float* cnt_nm, const float* encoded, int64_t n, const int32_t* labels, int32_t* slot_out,
                            void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    Bank& b = c->bank;
    if (!b.resident) return fail(c, MOCHA_ERR_STATE, "bank_resident_add: no resident bank: call mocha_bank_resident_create first");
    if (!cnt_nm || !encoded) return fail(c, MOCHA_ERR_ARG, "bank_resident_add: null argument");
    const int S = b.segments();
    if (slot < -1 || slot >= S) return fail(c, MOCHA_ERR_ARG, "bank_resident_add: slot %d out of range 0 .. %d (-1: the lowest empty one)", slot, S - 1);
    if (n < 1 || n > b.seg_max_rows)
        return fail(c, MOCHA_ERR_ARG, "bank_resident_add: %lld rows: a character of this bank has 1 .. %lld", (long long)n, (long long)b.seg_max_rows);
    if (slot >= 0 && b.slot[slot].rows) return fail(c, MOCHA_ERR_STATE, "bank_resident_add: slot %d is occupied: retire it first", slot);
    for (int i = 0; slot < 0 && i < S; ++i)
        if (!b.slot[i].rows) slot = i;
    if (slot < 0) return fail(c, MOCHA_ERR_STATE, "bank_resident_add: all %d slots are occupied", S);
    const int64_t units = granule_units(n);
    const int64_t unit0 = b.extents.take(units);
    if (unit0 < 0)
        return fail(c, MOCHA_ERR_STATE, "bank_resident_add: no free extent of %lld rows: the largest is %lld rows (%lld rows free in all; extents do not move)",
                    (long long)n, (long long)(b.extents.largest() * SEG_GRANULE_ROWS), (long long)(b.extents.free_units() * SEG_GRANULE_ROWS));
    const int64_t first = unit0 * SEG_GRANULE_ROWS;
    const size_t D = 90 * 256;
    const int L = c->cfg.dec_depth;
    hipStream_t s = (hipStream_t)stream;
    // rows -> their decoder constants (and bounds) -> their label tables -> the slot, published last
    rc = [&]() -> int {
        HIPCHK(c, hipMemcpyAsync(b.cnt_own.p + (size_t)first * D, cnt_nm, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        HIPCHK(c, hipMemcpyAsync(b.enc_own.p + (size_t)first * D, encoded, (size_t)n * D * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (b.dec_valid) {
            const size_t rows = (size_t)std::min<int64_t>(b.seg_max_rows, 4096);        // what mocha_bank_resident_create reserved
            int r = build_dec_consts(c, b.enc_own.p + (size_t)first * D, n, b.kin.p + (size_t)first * D, b.gb.p + (size_t)first * 512 * L, c->style_scratch.p,
                                     c->style_scratch.p + rows * 256, (int64_t)rows, s, true);
            if (r) return r;
        }
        if (b.amax_ok) {
            HIPCHK(c, hipMemsetAsync(b.amax.p + first, 0, (size_t)n * sizeof(float), s));
            for (int64_t n0 = 0; n0 < n; n0 += 65535)     // (the kernel's grid.y)
                LAUNCH(c, s, "mocha_absmax", "bank.absmax", 0.0, 4.0 * std::min<int64_t>(65535, n - n0) * D,
                       launch_absmax(b.enc_own.p + (size_t)(first + n0) * D, std::min<int64_t>(65535, n - n0), (long long)D, b.amax.p + first + n0, s));
        }
        LAUNCH(c, s, "mocha_resident_labels", "bank.labels", 0.0, 5.0 * n,
               launch_resident_labels(labels, n, first, b.N, b.lab_dev.p, b.lab_gran.p, b.lab_any.p + slot, s));
        // the online path's tables: no row of the new character starts a clip yet (mocha_bank_resident_set_starts), and the slot's epoch
        // moves, so that a stream on this slot restarts even when the new character has the old one's extent
        LAUNCH(c, s, "mocha_path_starts_clear", "bank.starts", 0.0, n / 8.0 + 8.0,
               launch_path_starts(b.start_bits.p, b.N, first, n, nullptr, 0, b.slot_epoch.p + slot, s));
        LAUNCH(c, s, "mocha_resident_publish", "bank.publish", 0.0, 12.0,
               launch_resident_publish(b.seg_dev.p, b.lab_gran_start.p, slot, S, first, n, b.N, s));
        return 0;
    }();
    if (rc) { (void)b.extents.release(unit0, units); return rc; }      // (the slot was not published: its rows are nobody's)
    b.slot[slot].first = first; b.slot[slot].rows = n;
    if (slot_out) *slot_out = slot;
    return 0;
}

int mocha_bank_resident_retire(mocha_ctx* c, int slot, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    Bank& b = c->bank;
    if (!b.resident) return fail(c, MOCHA_ERR_STATE, "bank_resident_retire: no resident bank: call mocha_bank_resident_create first");
    const int S = b.segments();
    if (slot < 0 || slot >= S) return fail(c, MOCHA_ERR_ARG, "bank_resident_retire: slot %d out of range 0 .. %d", slot, S - 1);
    if (!b.slot[slot].rows) return fail(c, MOCHA_ERR_STATE, "bank_resident_retire: slot %d is empty", slot);
    hipStream_t s = (hipStream_t)stream;
    // row count 0: the slot's id is now an id outside the table; its rows stay as they are and are never read
    LAUNCH(c, s, "mocha_resident_publish", "bank.publish", 0.0, 12.0, launch_resident_publish(b.seg_dev.p, b.lab_gran_start.p, slot, S, 0, 0, b.N, s));
    LAUNCH(c, s, "mocha_path_starts_clear", "bank.starts", 0.0, b.slot[slot].rows / 8.0 + 8.0,
           launch_path_starts(b.start_bits.p, b.N, b.slot[slot].first, b.slot[slot].rows, nullptr, 0, b.slot_epoch.p + slot, s));
    (void)b.extents.release(b.slot[slot].first / SEG_GRANULE_ROWS, granule_units(b.slot[slot].rows));
    b.slot[slot] = Bank::Slot{};
    return 0;
}

int mocha_bank_resident_info(const mocha_ctx* c, int slot, int64_t* first_row, int64_t* rows, int64_t* free_rows, int64_t* largest_free) {
    if (!c) return MOCHA_ERR_ARG;
    const Bank& b = c->bank;
    if (!b.resident) return MOCHA_ERR_STATE;
    if (slot < -1 || slot >= b.segments()) return MOCHA_ERR_ARG;
    if (first_row) *first_row = slot >= 0 ? b.slot[slot].first : 0;
    if (rows) *rows = slot >= 0 ? b.slot[slot].rows : 0;
    if (free_rows) *free_rows = b.extents.free_units() * SEG_GRANULE_ROWS;
    if (largest_free) *largest_free = b.extents.largest() * SEG_GRANULE_ROWS;
    return 0;
}

// ------------------------------------------------------------------------------------------- RCCL (multi-GPU set-up)
// One process per GPU; the only exchange on the path is the one-time broadcast of the character bank.
// RCCL is resolved at run time (dlopen of librccl.so.1) so that single-GPU users never load it.
namespace {
struct Rccl {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*GetVersion)(int*) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
std::string g_rccl_path;          // mocha_set_rccl_library: a process that already holds an RCCL (PyTorch ships its own) should use that one

int rccl_load(mocha_ctx* c) {
    if (g_rccl.h) return 0;
    void* h = nullptr;
    if (!g_rccl_path.empty()) {
        h = dlopen(g_rccl_path.c_str(), RTLD_NOW | RTLD_LOCAL);
        if (!h) return fail(c, MOCHA_ERR_STATE, "cannot load RCCL from '%s': %s", g_rccl_path.c_str(), dlerror());
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(c, MOCHA_ERR_STATE, "cannot load RCCL (librccl.so.1): %s", dlerror());
    Rccl r; r.h = h;
    bool ok = true;
    auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) ok = false; return p; };
    r.GetUniqueId = (decltype(r.GetUniqueId))sym("ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))sym("ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.CommCount = (decltype(r.CommCount))sym("ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))sym("ncclCommUserRank");
    r.Broadcast = (decltype(r.Broadcast))sym("ncclBroadcast");
    r.AllGather = (decltype(r.AllGather))sym("ncclAllGather");
    r.Send = (decltype(r.Send))sym("ncclSend");
    r.Recv = (decltype(r.Recv))sym("ncclRecv");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.GetVersion = (decltype(r.GetVersion))sym("ncclGetVersion");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    if (!ok) { dlclose(h); return fail(c, MOCHA_ERR_STATE, "librccl lacks an expected entry point"); }
    g_rccl = r;
    return 0;
}
#define NCCLCHK(c, expr)                                                                                                  \
    do {                                                                                                                  \
        ncclResult_t r__ = (expr);                                                                                        \
        if (r__ != ncclSuccess) return fail((c), MOCHA_ERR_HIP, "%s failed: %s", #expr, g_rccl.GetErrorString(r__));    \
    } while (0)

// Broadcast `count` floats from `root` so that every xGMI link of the root carries traffic: the root sends chunk r to
// rank r (grouped point-to-point = scatter), then an in-place all-gather completes every rank's copy.  A flat
// ncclBroadcast is a ring through the root's neighbours and bound by one link (~153 GB/s); scatter + all-gather moves
// 1/world of the data per link and step.  The count % world tail (a few floats) goes through one small ncclBroadcast.
// the plan of one chunked broadcast: rank r owns floats [r * chunk, (r + 1) * chunk), the last `tail` floats are broadcast whole
struct BcastPlan { size_t chunk, tail, tail_off; };
BcastPlan bcast_plan(size_t count, int world) {
    BcastPlan p;
    p.chunk = count / (size_t)world;
    p.tail_off = p.chunk * (size_t)world;
    p.tail = count - p.tail_off;
    return p;
}

int bcast_chunked(mocha_ctx* c, ncclComm_t comm, int world, int rank, int root, float* buf, size_t count, hipStream_t s) {
    if (world == 1 || count == 0) return 0;
    const BcastPlan pl = bcast_plan(count, world);
    if (pl.chunk > 0) {
        // inside a group no call may return early: a group left open would swallow every later RCCL call of this thread.
        // The first error is kept, the group is always closed.
        ncclResult_t first = ncclSuccess;
        const char* what = "";
        auto keep = [&](ncclResult_t r, const char* w) { if (r != ncclSuccess && first == ncclSuccess) { first = r; what = w; } };
        NCCLCHK(c, g_rccl.GroupStart());
        if (rank == root) {
            for (int r = 0; r < world && first == ncclSuccess; ++r)
                if (r != root) keep(g_rccl.Send(buf + pl.chunk * (size_t)r, pl.chunk, ncclFloat32, r, comm, s), "ncclSend");
        } else {
            keep(g_rccl.Recv(buf + pl.chunk * (size_t)rank, pl.chunk, ncclFloat32, root, comm, s), "ncclRecv");
        }
        keep(g_rccl.GroupEnd(), "ncclGroupEnd");
        if (first != ncclSuccess) return fail(c, MOCHA_ERR_HIP, "%s failed in the bank scatter: %s", what, g_rccl.GetErrorString(first));
        NCCLCHK(c, g_rccl.AllGather(buf + pl.chunk * (size_t)rank, buf, pl.chunk, ncclFloat32, comm, s));
    }
    if (pl.tail > 0) NCCLCHK(c, g_rccl.Broadcast(buf + pl.tail_off, buf + pl.tail_off, pl.tail, ncclFloat32, root, comm, s));
    return 0;
}
}  // namespace

int mocha_bcast_plan(int64_t count, int world, int rank, int64_t out[4]) {
    if (count < 0 || world < 1 || rank < 0 || rank >= world || !out) return MOCHA_ERR_ARG;
    const BcastPlan p = bcast_plan((size_t)count, world);
    out[0] = (int64_t)(p.chunk * (size_t)rank); out[1] = (int64_t)p.chunk; out[2] = (int64_t)p.tail_off; out[3] = (int64_t)p.tail;
    return 0;
}

int mocha_set_rccl_library(const char* path) {
    if (g_rccl.h) return MOCHA_ERR_STATE;              // already resolved: too late to switch
    g_rccl_path = path ? path : "";
    return 0;
}

int mocha_comm_unique_id(mocha_ctx* c, void* id128) {
    if (!c || !id128) return fail(c, MOCHA_ERR_ARG, "null argument");
    int rc = rccl_load(c); if (rc) return rc;
    ncclUniqueId id;
    NCCLCHK(c, g_rccl.GetUniqueId(&id));
    memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return 0;
}

int mocha_comm_init(mocha_ctx* c, const void* id128, int nranks, int rank) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, MOCHA_ERR_ARG, "bad communicator arguments");
    int rc = rccl_load(c); if (rc) return rc;
    if (c->comm) return fail(c, MOCHA_ERR_STATE, "communicator already initialised");
    HIPCHK(c, hipSetDevice(c->device));
    ncclUniqueId id;
    memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    NCCLCHK(c, g_rccl.CommInitRank(&c->comm, nranks, id, rank));
    c->comm_rank = rank; c->comm_size = nranks;
    return 0;
}

int mocha_comm_info(mocha_ctx* c, mocha_comm_info_t* out) {
    if (!c || !out) return fail(c, MOCHA_ERR_ARG, "null argument");
    if (!c->comm || !g_rccl.h) return fail(c, MOCHA_ERR_STATE, "no communicator: call mocha_comm_init first");
    memset(out, 0, sizeof *out);
    NCCLCHK(c, g_rccl.CommCount(c->comm, &out->nranks));
    NCCLCHK(c, g_rccl.CommUserRank(c->comm, &out->rank));
    NCCLCHK(c, g_rccl.GetVersion(&out->rccl_version));
    out->device = c->device;
    HIPCHK(c, hipDeviceGetPCIBusId(out->pci_bus_id, (int)sizeof out->pci_bus_id, c->device));
    Dl_info di;
    if (dladdr(reinterpret_cast<const void*>(g_rccl.CommInitRank), &di) && di.dli_fname) {
        char real[4096];
        const char* path = realpath(di.dli_fname, real) ? real : di.dli_fname;
        snprintf(out->library, sizeof out->library, "%s", path);
    }
    return 0;
}

int mocha_comm_destroy(mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    if (c->comm && g_rccl.h) { (void)g_rccl.CommDestroy(c->comm); }
    c->comm = nullptr; c->comm_rank = 0; c->comm_size = 1;
    return 0;
}

int mocha_bank_broadcast(mocha_ctx* c, void* comm_, int root, int64_t N, int flags, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = rccl_load(c))) return rc;
    ncclComm_t comm = comm_ ? (ncclComm_t)comm_ : c->comm;
    if (!comm) return fail(c, MOCHA_ERR_STATE, "no communicator: call mocha_comm_init first or pass one");
    int world = 1, rank = 0;
    NCCLCHK(c, g_rccl.CommCount(comm, &world));
    NCCLCHK(c, g_rccl.CommUserRank(comm, &rank));
    if (root < 0 || root >= world || N < 1 || N > (int64_t)1 << 30) return fail(c, MOCHA_ERR_ARG, "bad bank_broadcast arguments");
    // A resident bank has no union to send.  A root that is alone refuses at once, as the other union calls do; among several ranks it
    // must not leave the others inside the header exchange, so it announces "no such bank" below - every rank then fails - and names the
    // reason in its own message
    if (rank == root && world == 1 && (rc = refuse_resident(c, "mocha_bank_broadcast"))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t D = 90 * 256;
    const bool want_bf16 = (flags & MOCHA_BANK_BF16) != 0;
    // Header first: EVERY rank contributes {entries, bf16?} as it understands the call - the root from the bank it is about to send
    // (-1 entries: it has none of the size the call names), the others from their arguments - the headers are all-gathered, and
    // every rank checks all of them before any payload moves.  All ranks see the same headers, so a disagreement fails loudly on
    // ALL ranks instead of leaving some of them inside a collective the others never enter.
    if (world > 4096) return fail(c, MOCHA_ERR_ARG, "bank_broadcast: %d ranks", world);
    if ((rc = reserve(c, c->bcast_hdr, 2 * 4096))) return rc;
    std::vector<long long> hdr((size_t)2 * world, 0);
    long long mine[2] = {(long long)N, want_bf16 ? 1 : 0};
    if (rank == root) { mine[0] = (c->bank.cnt && c->bank.N == N && !c->bank.resident) ? (long long)N : -1; mine[1] = c->bank.is_bf16 ? 1 : 0; }
    HIPCHK(c, hipMemcpyAsync(c->bcast_hdr.p + 2 * rank, mine, sizeof mine, hipMemcpyHostToDevice, s));
    if (world > 1) NCCLCHK(c, g_rccl.AllGather(c->bcast_hdr.p + 2 * rank, c->bcast_hdr.p, 2, ncclInt64, comm, s));
    HIPCHK(c, hipMemcpyAsync(hdr.data(), c->bcast_hdr.p, hdr.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (hdr[2 * root] != (long long)N || hdr[2 * root] < 0) {
        if (rank == root && (rc = refuse_resident(c, "mocha_bank_broadcast"))) return rc;
        if (hdr[2 * root] < 0)
            return fail(c, MOCHA_ERR_STATE, "bank_broadcast: the root (rank %d) has no current bank of the number of entries it was called with", root);
        return fail(c, MOCHA_ERR_STATE, "bank_broadcast: the root (rank %d) has no current bank of %lld entries (it announced %lld)", root,
                    (long long)N, hdr[2 * root]);
    }
    for (int r = 0; r < world; ++r) {
        if (hdr[2 * r] != hdr[2 * root])
            return fail(c, MOCHA_ERR_ARG, "bank_broadcast: rank %d asks for %lld entries, the root (rank %d) sends %lld: every rank must name the same bank",
                        r, hdr[2 * r], root, hdr[2 * root]);
        if (hdr[2 * r + 1] != hdr[2 * root + 1])
            return fail(c, MOCHA_ERR_ARG, "bank_broadcast: the root's bank was set %s MOCHA_BANK_BF16 but rank %d asks for the opposite: every "
                        "rank must match against the same bank", hdr[2 * root + 1] ? "with" : "without", r);
    }
    if (rank != root && (rc = bank_own_rows(c, c->bank, N))) return rc;
    // the root's own chunks are rewritten in place with identical values by the all-gather (a borrowed bank stays unchanged)
    float* cnt = rank == root ? const_cast<float*>(c->bank.cnt) : c->bank.cnt_own.p;
    float* enc = rank == root ? const_cast<float*>(c->bank.enc) : c->bank.enc_own.p;
    if ((rc = bcast_chunked(c, comm, world, rank, root, cnt, (size_t)N * D, s))) return rc;
    if ((rc = bcast_chunked(c, comm, world, rank, root, enc, (size_t)N * D, s))) return rc;
    if (rank == root) return 0;
    // derived data (centroid, norms, bf16 copy) is recomputed locally: deterministic kernels, same result on every rank
    return bank_set_impl(c, c->bank, c->bank.cnt_own.p, c->bank.enc_own.p, N, (flags & MOCHA_BANK_BF16) | MOCHA_BANK_BORROW, stream);
}

int mocha_set_pose_norm(mocha_ctx* c, const float* x_mean, const float* x_std, const float* y_mean, const float* y_std) {
    if (!c || !x_mean || !x_std || !y_mean || !y_std) return fail(c, MOCHA_ERR_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nn = (size_t)(c->cfg.V + 1) * c->cfg.C_in;
    for (size_t i = 0; i < nn; ++i)
        if (!(x_std[i] != 0.f)) return fail(c, MOCHA_ERR_ARG, "x_std[%zu] is zero", i);
    { int rc = reserve(c, c->pose_norm, 4 * nn); if (rc) return rc; }
    const float* src[4] = {x_mean, x_std, y_mean, y_std};
    for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpy(c->pose_norm.p + k * nn, src[k], nn * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

int mocha_encode_raw(mocha_ctx* c, const float* X_raw, int B, float* encoded, float* cnt, const float* cnt_mean,
                     const float* cnt_std, float* cnt_nm, void* stream) {
    int rc = ready(c, B); if (rc) return rc;
    NEED_PTRS(c, B, "mocha_encode_raw", X_raw, encoded);
    const size_t xs = (size_t)60 * (c->cfg.V + 1) * c->cfg.C_in, ts = 90 * 256;
    if (cnt_nm && (!cnt_mean || !cnt_std)) return fail(c, MOCHA_ERR_ARG, "mocha_encode_raw: cnt_nm needs cnt_mean and cnt_std");
    const bool zn = cnt_nm != nullptr;
    return for_chunks(c, B, (hipStream_t)stream, [&](int b0, int b, hipStream_t s) -> int {
        int r;
        if ((r = run_embed(c, X_raw + b0 * xs, b, WS(c, "x5"), true, s, true))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), b, encoded + b0 * ts, s))) return r;
        if (cnt || zn) {
            const InormExtra iex0 = IEXW(c, s);
            LAUNCH(c, s, "mocha_instnorm", "mvn", 0.0, b * 90.0 * 256 * 4 * (1 + (cnt ? 1 : 0) + (zn ? 1 : 0)),
                   launch_instnorm(encoded + b0 * ts, cnt ? cnt + b0 * ts : nullptr, nullptr, zn ? cnt_mean : nullptr, zn ? cnt_std : nullptr,
                                   zn ? cnt_nm + b0 * ts : nullptr, b, 90, s, &iex0));
        }
        return 0;
    });
}

// ------------------------------------------------------------------------------------------- CVAE sampler
static void cvae_expectations(mocha_ctx* c) {
    if (!c->cvae_expect.empty()) return;
    auto& e = c->cvae_expect;
    const int64_t d = 256, ff = 512;
    e["prior_net.mu_token"] = {1, 1, d};
    e["prior_net.logvar_token"] = {1, 1, d};
    auto attn = [&](const std::string& p) {
        e[p + ".in_proj_weight"] = {3 * d, d}; e[p + ".in_proj_bias"] = {3 * d};
        e[p + ".out_proj.weight"] = {d, d}; e[p + ".out_proj.bias"] = {d};
    };
    auto ffn = [&](const std::string& p, int norms) {
        e[p + ".linear1.weight"] = {ff, d}; e[p + ".linear1.bias"] = {ff};
        e[p + ".linear2.weight"] = {d, ff}; e[p + ".linear2.bias"] = {d};
        for (int n = 1; n <= norms; ++n) { e[p + ".norm" + std::to_string(n) + ".weight"] = {d}; e[p + ".norm" + std::to_string(n) + ".bias"] = {d}; }
    };
    for (int l = 0; l < c->cvae_depth; ++l) {
        const std::string p = "prior_net.encoder.layers." + std::to_string(l);
        attn(p + ".self_attn"); ffn(p, 2);
        const std::string q = "decoder.decoder.layers." + std::to_string(l);
        attn(q + ".self_attn"); attn(q + ".multihead_attn"); ffn(q, 3);
    }
}

int mocha_cvae_load_weight(mocha_ctx* c, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!c || !name || !host || !shape) return fail(c, MOCHA_ERR_ARG, "null argument");
    cvae_expectations(c);
    const std::string n(name);
    // training-only posterior encoder and the regenerated positional-encoding buffers are accepted and ignored
    if (n.rfind("encoder.", 0) == 0) return 0;
    if (n.size() > 15 && n.compare(n.size() - 15, 15, ".pos_encoder.pe") == 0) {
        // registered buffer (1, max_len, 256): keep its first 192 rows so the table is bit-identical to the checkpoint's
        if (ndim == 3 && shape[0] == 1 && shape[1] >= 192 && shape[2] == 256) {
            HostTensor t; t.data.assign(host, host + 192 * 256); t.shape = {192, 256};
            c->cvae_host["pe"] = std::move(t);
            c->cvae_ready = false;
        }
        return 0;
    }
    auto it = c->cvae_expect.find(n);
    if (it == c->cvae_expect.end()) return fail(c, MOCHA_ERR_WEIGHT, "unknown CVAE weight name '%s'", name);
    if ((int)it->second.size() != ndim) return fail(c, MOCHA_ERR_WEIGHT, "%s: rank %d, expected %zu", name, ndim, it->second.size());
    size_t cnt = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] != it->second[i]) return fail(c, MOCHA_ERR_WEIGHT, "%s: dim %d is %lld, expected %lld", name, i, (long long)shape[i], (long long)it->second[i]);
        cnt *= (size_t)shape[i];
    }
    HostTensor t; t.data.assign(host, host + cnt); t.shape.assign(shape, shape + ndim);
    c->cvae_host[n] = std::move(t);
    c->cvae_ready = false;
    return 0;
}

int mocha_cvae_finalize(mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    cvae_expectations(c);
    for (auto& kv : c->cvae_expect)
        if (!c->cvae_host.count(kv.first)) return fail(c, MOCHA_ERR_STATE, "missing CVAE weight '%s'", kv.first.c_str());
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    x3_drop_images(c);
    h2_drop_images(c);
    for (auto& kv : c->cvae_host) {
        int rc = upload_to(c, c->cw, kv.first, kv.second.data); if (rc) return rc;
    }
    if (c->cw.count("pe")) { c->cvae_ready = true; return 0; }     // table came with the state_dict (pos_encoder.pe)
    // sin/cos positional encoding rows 0..191 (model_CVAE.py:168-178), float32 arithmetic like torch
    std::vector<float> pe(192 * 256);
    for (int i = 0; i < 128; ++i) {
        const float div = expf((float)(2 * i) * (float)(-std::log(10000.0) / 256.0));
        for (int t = 0; t < 192; ++t) {
            const float a = (float)t * div;
            pe[t * 256 + 2 * i] = sinf(a);
            pe[t * 256 + 2 * i + 1] = cosf(a);
        }
    }
    int rc = upload_to(c, c->cw, "pe", pe); if (rc) return rc;
    c->cvae_ready = true;
    return 0;
}

static int cvae_ws(mocha_ctx* c, int B) {
    if (c->cvae_B >= B) return 0;
    if (c->cvae_B > 0) HIPCHK(c, hipDeviceSynchronize());
    c->cws.clear();
    c->generation++;
    const std::pair<const char*, size_t> plan[] = {{"t0", 182 * 256}, {"t1", 182 * 256}, {"t2", 182 * 256}, {"qkv", 182 * 768},
                                                   {"hff", 182 * 512}, {"mem", 181 * 256}, {"kv", 181 * 512}};
    for (auto& pl : plan) { int rc = reserve(c, c->cws[pl.first], pl.second * (size_t)B); if (rc) return rc; }
    c->cvae_B = B;
    return 0;
}

// The sampler's weights come from the context's own CVAE (c->cw) or, for a GROUPED pass - `which` non-null: device, one weight-bank slot
// per clip of the batch - from the weight bank: cvae_w then returns slot 0's tensor and the grouped launches step by the slot stride.
static const float* cvae_w(mocha_ctx* c, const std::string& n, const int32_t* which) {
    return which ? c->cvb.w.p + c->cvb.off.at(n) : c->cw.at(n).p;
}
// one GEMM of the sampler over B clips of m rows each: launch_gemm, or the grouped kernel with the clip's slot
static int cvae_gemm(mocha_ctx* c, hipStream_t s, const char* site, const GemmParams& g, int m, const int32_t* which) {
    if (!which) { GEMM(c, s, site, g); return 0; }
    GroupedGemmParams q;
    q.A = g.A; q.W = g.W; q.bias = g.bias; q.which = which; q.stored = c->cvb.stored.p; q.C = g.C; q.residual = g.residual;
    q.G = g.M / m; q.m = m; q.N = g.N; q.K = g.K; q.Cw = c->cvb.Cw; q.lda = g.lda; q.ldc = g.ldc; q.ldr = g.ldr;
    q.w_stride = q.b_stride = (long long)c->cvb.slot_floats; q.act = g.act;
    // bytes: the activations and the output once, a group's weights once per 16 rows
    LAUNCH(c, s, "mocha_gemm_grouped", site, 2.0 * g.M * (double)g.N * g.K,
           4.0 * ((double)g.M * g.K + (double)q.G * ((m + 15) / 16) * (double)g.N * g.K + (double)g.M * g.N * (g.residual ? 2 : 1)),
           launch_gemm_grouped(q, s));
    return 0;
}
static int cvae_norm(mocha_ctx* c, hipStream_t s, const float* x, const std::string& norm, float* y, int B, int n, const int32_t* which) {
    const float* w = cvae_w(c, norm + ".weight", which); const float* b = cvae_w(c, norm + ".bias", which);
    if (which)
        LAUNCH(c, s, "mocha_layernorm256_grouped", "cvae.norm", 0.0, B * n * 256.0 * 8,
               launch_layernorm256_grouped(x, w, b, (long long)c->cvb.slot_floats, which, c->cvb.stored.p, c->cvb.Cw, y, B, n, s));
    else
        LAUNCH(c, s, "mocha_layernorm256", "cvae.norm", 0.0, B * n * 256.0 * 8, launch_layernorm256(x, w, b, y, B * n, s));
    return 0;
}

// post-norm transformer sub-blocks shared by PriorNet and Decoder (nn.TransformerEncoderLayer / DecoderLayer defaults)
static int cvae_attn_block(mocha_ctx* c, hipStream_t s, const std::string& p, const std::string& norm, float* x /*in/out*/, int nq,
                           const float* kvsrc /*nullptr: self*/, int nk, int B, const int32_t* which = nullptr) {
    int rc;
    float* qkv = c->cws.at("qkv").p; float* t1 = c->cws.at("t1").p; float* t2 = c->cws.at("t2").p; float* kvb = c->cws.at("kv").p;
    const float* Win = cvae_w(c, p + ".in_proj_weight", which); const float* bin = cvae_w(c, p + ".in_proj_bias", which);
    const int H = c->cvae_heads, DH = 256 / H;
    AttnParams a{};
    if (!kvsrc) {
        GemmParams g = plain(x, 256, Win, qkv, 768, B * nq, 768, 256); g.bias = bin;
        if ((rc = cvae_gemm(c, s, "cvae.in_proj", g, nq, which))) return rc;
        a = AttnParams{qkv, qkv + 256, qkv + 512, t1, 768, 768, 768, 256, B, H, DH, nq, nq, (float)std::pow((double)DH, -0.5)};
    } else {
        GemmParams gq = plain(x, 256, Win, qkv, 256, B * nq, 256, 256); gq.bias = bin;
        if ((rc = cvae_gemm(c, s, "cvae.q_proj", gq, nq, which))) return rc;
        GemmParams gk = plain(kvsrc, 256, Win + 256 * 256, kvb, 512, B * nk, 512, 256); gk.bias = bin + 256;
        if ((rc = cvae_gemm(c, s, "cvae.kv_proj", gk, nk, which))) return rc;
        a = AttnParams{qkv, kvb, kvb + 256, t1, 256, 512, 512, 256, B, H, DH, nq, nk, (float)std::pow((double)DH, -0.5)};
    }
    LAUNCH(c, s, "mocha_attention_f32<64>", "cvae.attn", 4.0 * B * H * (double)a.nq * a.nk * DH, 4.0 * B * (a.nq + 2.0 * a.nk) * 256,
           launch_attention(a, s));
    GemmParams o = plain(t1, 256, cvae_w(c, p + ".out_proj.weight", which), t2, 256, B * nq, 256, 256);
    o.bias = cvae_w(c, p + ".out_proj.bias", which); o.residual = x; o.ldr = 256;
    if ((rc = cvae_gemm(c, s, "cvae.out_proj", o, nq, which))) return rc;
    return cvae_norm(c, s, t2, norm, x, B, nq, which);
}

static int cvae_ff_block(mocha_ctx* c, hipStream_t s, const std::string& p, const std::string& norm, float* x, float* out, int n, int B,
                         const int32_t* which = nullptr) {
    int rc;
    float* hff = c->cws.at("hff").p; float* t2 = c->cws.at("t2").p;
    GemmParams f1 = plain(x, 256, cvae_w(c, p + ".linear1.weight", which), hff, 512, B * n, 512, 256);
    f1.bias = cvae_w(c, p + ".linear1.bias", which); f1.act = 3;
    if ((rc = cvae_gemm(c, s, "cvae.ff1", f1, n, which))) return rc;
    GemmParams f2 = plain(hff, 512, cvae_w(c, p + ".linear2.weight", which), t2, 256, B * n, 256, 512);
    f2.bias = cvae_w(c, p + ".linear2.bias", which); f2.residual = x; f2.ldr = 256;
    if ((rc = cvae_gemm(c, s, "cvae.ff2", f2, n, which))) return rc;
    return cvae_norm(c, s, t2, norm, out, B, n, which);
}

// CVAE.sample for B conditions on stream s: the body of mocha_cvae_sample and of the live step's CVAE branch.  The caller checked the
// arguments, the weights (cvae_ready, or the weight bank for a grouped pass) and the workspace (cvae_ws(c, B)).
// which non-null: the GROUPED pass - clip b on slot which[b] (device) of the weight bank; a clip with an invalid slot reads no weight and
// its out / mu / logvar are zeros (the attention and the latent kernel read no weights and run on the zero rows the grouped launches leave).
static int cvae_sample_impl(mocha_ctx* c, const float* cond, int B, float* out, float* mu, float* logvar, const float* eps, hipStream_t s,
                            const int32_t* which = nullptr) {
    int rc;
    const int nc = c->cvae_nc, nq = c->cvae_nq, ntok = nc + 2;
    float* t0 = c->cws.at("t0").p; float* mem = c->cws.at("mem").p;
    const float* pe = which ? c->cvb.pe.p : c->cw.at("pe").p;
    // PriorNet.encode (model_CVAE.py:69-79)
    if (which)
        LAUNCH(c, s, "mocha_cvae_prior_tokens_grouped", "cvae.tokens", 0.0, B * ntok * 256.0 * 8,
               launch_cvae_prior_tokens_grouped(cond, cvae_w(c, "prior_net.mu_token", which), cvae_w(c, "prior_net.logvar_token", which),
                                                (long long)c->cvb.slot_floats, which, c->cvb.stored.p, c->cvb.Cw, pe, t0, B, nc, s));
    else
        LAUNCH(c, s, "mocha_cvae_prior_tokens", "cvae.tokens", 0.0, B * ntok * 256.0 * 8,
               launch_cvae_prior_tokens(cond, c->cw.at("prior_net.mu_token").p, c->cw.at("prior_net.logvar_token").p, pe, t0, B, nc, s));
    for (int l = 0; l < c->cvae_depth; ++l) {
        const std::string p = "prior_net.encoder.layers." + std::to_string(l);
        if ((rc = cvae_attn_block(c, s, p + ".self_attn", p + ".norm1", t0, ntok, nullptr, ntok, B, which))) return rc;
        if ((rc = cvae_ff_block(c, s, p, p + ".norm2", t0, t0, ntok, B, which))) return rc;
    }
    // reparameterize + Decoder inputs (model_CVAE.py:81-87, 158-163); the decoder state reuses t1's sibling t0 after this
    float* xq = c->cws.at("t1").p;     // free until the first attention writes it: use hff as query buffer instead
    xq = c->cws.at("hff").p;           // (B, nq, 256) fits in (B, 182, 512)
    LAUNCH(c, s, "mocha_cvae_latent", "cvae.latent", 0.0, B * (nc + nq + 2) * 256.0 * 4,
           launch_cvae_latent(t0, ntok, eps, cond, nc, pe, nq, mem, xq, mu, logvar, B, s));
    HIPCHK(c, hipMemcpyAsync(t0, xq, (size_t)B * nq * 256 * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int l = 0; l < c->cvae_depth; ++l) {
        const std::string p = "decoder.decoder.layers." + std::to_string(l);
        if ((rc = cvae_attn_block(c, s, p + ".self_attn", p + ".norm1", t0, nq, nullptr, nq, B, which))) return rc;
        if ((rc = cvae_attn_block(c, s, p + ".multihead_attn", p + ".norm2", t0, nq, mem, nc + 1, B, which))) return rc;
        const bool last = l == c->cvae_depth - 1;
        if ((rc = cvae_ff_block(c, s, p, p + ".norm3", t0, last ? out : t0, nq, B, which))) return rc;
    }
    return 0;
}

int mocha_cvae_sample(mocha_ctx* c, const float* cond, int B, float* out, float* mu, float* logvar, const float* eps, void* stream) {
    if (c && B == 0) return 0;
    if (!c || !cond || !out || B < 0) return fail(c, MOCHA_ERR_ARG, "bad CVAE arguments");
    if (!c->cvae_ready) return fail(c, MOCHA_ERR_STATE, "CVAE weights not finalised: call mocha_cvae_finalize first");
    if (B == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = cvae_ws(c, B); if (rc) return rc;
    return cvae_sample_impl(c, cond, B, out, mu, logvar, eps, (hipStream_t)stream);
}

// ---- CVAE weight bank: one CVAE per slot, the slot of a row / stream chosen by device data (cvae_grouped.hip)
int mocha_cvae_bank_create(mocha_ctx* c, int max_cvaes) {
    if (!c) return MOCHA_ERR_ARG;
    if (max_cvaes < 1 || max_cvaes > 4096) return fail(c, MOCHA_ERR_ARG, "cvae_bank_create: 1 <= max_cvaes <= 4096 (got %d)", max_cvaes);
    cvae_expectations(c);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());                    // a previous bank may still be read
    auto& b = c->cvb;
    b.Cw = 0; b.off.clear(); b.slot_floats = 0; b.host_stored.clear();
    c->generation++;                                      // a captured grouped step has the previous bank's pointers baked in
    size_t off = 0;
    for (auto& kv : c->cvae_expect) {
        size_t cnt = 1;
        for (int64_t d : kv.second) cnt *= (size_t)d;
        b.off[kv.first] = off;
        off += (cnt + 3) / 4 * 4;                         // every tensor 16-byte aligned inside its slot
    }
    const size_t T = 90 * 256, Cw = (size_t)max_cvaes;
    b.w.release(); b.stats.release(); b.stored.release();
    int rc;
    if ((rc = reserve(c, b.w, Cw * off))) return rc;
    if ((rc = reserve(c, b.stats, Cw * 4 * T))) return rc;
    if ((rc = reserve(c, b.stored, Cw))) return rc;
    if ((rc = reserve(c, b.pe, (size_t)192 * 256))) return rc;
    if ((rc = reserve(c, b.none, 16))) return rc;
    if ((rc = reserve(c, b.live_slot, 16))) return rc;
    HIPCHK(c, hipMemset(b.w.p, 0, Cw * off * sizeof(float)));
    HIPCHK(c, hipMemset(b.stats.p, 0, Cw * 4 * T * sizeof(float)));
    HIPCHK(c, hipMemset(b.stored.p, 0, Cw * sizeof(int32_t)));
    HIPCHK(c, hipMemset(b.none.p, 0xFF, 16 * sizeof(int32_t)));
    HIPCHK(c, hipMemset(b.live_slot.p, 0xFF, 16 * sizeof(int32_t)));
    // the shared table: sin/cos positional encoding rows 0..191 (model_CVAE.py:168-178), float32 arithmetic like torch - mocha_cvae_finalize's
    b.pe_host.assign((size_t)192 * 256, 0.f);
    for (int i = 0; i < 128; ++i) {
        const float div = expf((float)(2 * i) * (float)(-std::log(10000.0) / 256.0));
        for (int t = 0; t < 192; ++t) {
            const float a = (float)t * div;
            b.pe_host[t * 256 + 2 * i] = sinf(a);
            b.pe_host[t * 256 + 2 * i + 1] = cosf(a);
        }
    }
    HIPCHK(c, hipMemcpy(b.pe.p, b.pe_host.data(), b.pe_host.size() * sizeof(float), hipMemcpyHostToDevice));
    if (b.pin) { (void)hipHostFree(b.pin); b.pin = nullptr; }
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&b.pin), (off + 4 * T + (size_t)192 * 256) * sizeof(float), hipHostMallocDefault));
    if (!b.ev) HIPCHK(c, hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
    b.ev_pending = false;
    b.slot_floats = off;
    b.host_stored.assign(Cw, 0);
    b.Cw = max_cvaes;
    return 0;
}

int mocha_cvae_bank_store(mocha_ctx* c, int slot, const float* src_cnt_mean, const float* src_cnt_std, const float* cha_encoded_mean,
                          const float* cha_encoded_std, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    auto& b = c->cvb;
    if (!b.Cw) return fail(c, MOCHA_ERR_STATE, "cvae_bank_store: no CVAE weight bank: call mocha_cvae_bank_create first");
    if (slot < 0 || slot >= b.Cw) return fail(c, MOCHA_ERR_ARG, "cvae_bank_store: slot %d out of range 0 .. %d", slot, b.Cw - 1);
    if (!src_cnt_mean || !src_cnt_std || !cha_encoded_mean || !cha_encoded_std) return fail(c, MOCHA_ERR_ARG, "cvae_bank_store: null statistic");
    for (auto& kv : c->cvae_expect)
        if (!c->cvae_host.count(kv.first)) return fail(c, MOCHA_ERR_STATE, "cvae_bank_store: missing CVAE weight '%s'", kv.first.c_str());
    // One positional table per bank: the sin / cos table of mocha_cvae_bank_create until a store brings a pos_encoder.pe while NO slot is
    // stored - that table becomes the bank's (a checkpoint's registered buffer, bit for bit); from then on a staged table must equal it.
    auto pe = c->cvae_host.find("pe");
    bool adopt_pe = false;
    if (pe != c->cvae_host.end() && memcmp(pe->second.data.data(), b.pe_host.data(), b.pe_host.size() * sizeof(float)) != 0) {
        if (std::find(b.host_stored.begin(), b.host_stored.end(), 1) != b.host_stored.end()) {
            size_t i = 0;
            while (pe->second.data[i] == b.pe_host[i]) ++i;
            return fail(c, MOCHA_ERR_ARG, "cvae_bank_store: the staged pos_encoder.pe differs from the bank's table at %zu (%.9g vs %.9g): one table per bank",
                        i, pe->second.data[i], b.pe_host[i]);
        }
        adopt_pe = true;
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (b.ev_pending) HIPCHK(c, hipEventSynchronize(b.ev));      // the previous store's copies read the same pinned buffer
    b.ev_pending = false;
    const size_t T = 90 * 256;
    for (auto& kv : b.off) {
        const std::vector<float>& v = c->cvae_host.at(kv.first).data;
        memcpy(b.pin + kv.second, v.data(), v.size() * sizeof(float));
    }
    const float* st[4] = {src_cnt_mean, src_cnt_std, cha_encoded_mean, cha_encoded_std};
    for (int i = 0; i < 4; ++i) memcpy(b.pin + b.slot_floats + i * T, st[i], T * sizeof(float));
    if (adopt_pe) {
        b.pe_host = pe->second.data;
        memcpy(b.pin + b.slot_floats + 4 * T, b.pe_host.data(), b.pe_host.size() * sizeof(float));
        HIPCHK(c, hipMemcpyAsync(b.pe.p, b.pin + b.slot_floats + 4 * T, b.pe_host.size() * sizeof(float), hipMemcpyHostToDevice, s));
    }
    // weights and statistics, then the slot's stored word, LAST: a launch that sees it set sees the whole slot
    HIPCHK(c, hipMemcpyAsync(b.w.p + (size_t)slot * b.slot_floats, b.pin, b.slot_floats * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(b.stats.p + (size_t)slot * 4 * T, b.pin + b.slot_floats, 4 * T * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(b.ev, s));
    b.ev_pending = true;
    LAUNCH(c, s, "mocha_cvae_bank_publish", "cvae.publish", 0.0, 4.0, launch_cvae_bank_publish(b.stored.p, slot, b.Cw, 1, s));
    b.host_stored[slot] = 1;
    return 0;
}

int mocha_cvae_bank_clear(mocha_ctx* c, int slot, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    auto& b = c->cvb;
    if (!b.Cw) return fail(c, MOCHA_ERR_STATE, "cvae_bank_clear: no CVAE weight bank: call mocha_cvae_bank_create first");
    if (slot < 0 || slot >= b.Cw) return fail(c, MOCHA_ERR_ARG, "cvae_bank_clear: slot %d out of range 0 .. %d", slot, b.Cw - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_cvae_bank_publish", "cvae.publish", 0.0, 4.0, launch_cvae_bank_publish(b.stored.p, slot, b.Cw, 0, s));
    b.host_stored[slot] = 0;
    return 0;
}

int mocha_cvae_bank_info(const mocha_ctx* c, int* capacity, unsigned char* stored) {
    if (!c) return MOCHA_ERR_ARG;
    if (!c->cvb.Cw) return MOCHA_ERR_STATE;
    if (capacity) *capacity = c->cvb.Cw;
    if (stored) memcpy(stored, c->cvb.host_stored.data(), (size_t)c->cvb.Cw);
    return 0;
}

int mocha_cvae_sample_grouped(mocha_ctx* c, const float* cond, int B, const int32_t* which, float* out, float* mu, float* logvar,
                              const float* eps, void* stream) {
    if (c && B == 0) return 0;
    if (!c || !cond || !which || !out || B < 0) return fail(c, MOCHA_ERR_ARG, "bad grouped CVAE arguments");
    if (!c->cvb.Cw) return fail(c, MOCHA_ERR_STATE, "cvae_sample_grouped: no CVAE weight bank: call mocha_cvae_bank_create first");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = cvae_ws(c, B); if (rc) return rc;
    return cvae_sample_impl(c, cond, B, out, mu, logvar, eps, (hipStream_t)stream, which);
}

int mocha_cvae_condition(mocha_ctx* c, const float* src_cnt, const float* src_mean, const float* src_std, const float* prev_cha,
                         const float* cha_mean, const float* cha_std, int B, float* cond, void* stream) {
    if (c && B == 0) return 0;
    if (!c || !src_cnt || !src_mean || !src_std || !prev_cha || !cha_mean || !cha_std || !cond || B < 0) return fail(c, MOCHA_ERR_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_cvae_condition", "cvae.condition", 0.0, B * 180.0 * 256 * 8,
           launch_cvae_condition(src_cnt, src_mean, src_std, prev_cha, cha_mean, cha_std, cond, B, 90, s));
    return 0;
}

int mocha_scale_shift(mocha_ctx* c, const float* x, const float* mean, const float* std_, int B, float* out, void* stream) {
    if (c && B == 0) return 0;
    if (!c || !x || !mean || !std_ || !out || B < 0) return fail(c, MOCHA_ERR_ARG, "bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_scale_shift", "cvae.denorm", 0.0, B * 90.0 * 256 * 8, launch_scale_shift(x, mean, std_, out, B, 90, s));
    return 0;
}

// the (V+1)-bone skeleton's parents on the device, uploaded once (mocha_featurize, mocha_live_step)
static int ensure_bone_parents(mocha_ctx* c) {
    if (c->bone_parents.p) return 0;
    const int J = c->cfg.V + 1;
    std::vector<int> par(J);                        // parents = [-1] + (joint parents + 1), test_fullframework.py:101-102
    par[0] = -1;
    for (int i = 0; i < c->cfg.V; ++i) par[i + 1] = c->sk.parents[i] + 1;
    int rc = reserve(c, c->bone_parents, (size_t)J); if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->bone_parents.p, par.data(), sizeof(int) * J, hipMemcpyHostToDevice));
    return 0;
}

int mocha_featurize(mocha_ctx* c, const float* Yrot, const float* Ypos, const float* Yvel, const float* Yang, int B, float* X_raw,
                    void* stream) {
    if (c && B == 0) return 0;
    if (!c || !Yrot || !Ypos || !Yvel || !Yang || !X_raw || B < 0) return fail(c, MOCHA_ERR_ARG, "bad featurize arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const int J = c->cfg.V + 1;
    { int rc = ensure_bone_parents(c); if (rc) return rc; }
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_featurize", "featurize", B * 60.0 * J * 150, B * 60.0 * J * (13 + 15) * 4,
           launch_featurize(Yrot, Ypos, Yvel, Yang, c->bone_parents.p, X_raw, B, c->cfg.T, J, s));
    return 0;
}

int mocha_pose_heads(mocha_ctx* c, const float* Y, int B, float* heads, float* speed, void* stream) {
    if (c && B == 0) return 0;
    if (!c || !Y || !heads || !speed || B < 0) return fail(c, MOCHA_ERR_ARG, "bad pose_heads arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_pose_heads", "post.heads", 0.0, B * (60.0 * 12 + c->cfg.V * 28.0 * 4),
           launch_pose_heads(Y, heads, speed, B, c->cfg.T, c->cfg.V, s));
    return 0;
}

void mocha_post_cfg_default(mocha_post_cfg* cfg) {
    if (!cfg) return;
    *cfg = mocha_post_cfg{};
    cfg->dt = 1.0 / 60.0;                   // test_fullframework.py:105
    cfg->ik_max_length_buffer = 0.015;      // :109-114
    cfg->ik_foot_height = 0.02;
    cfg->ik_unlock_radius = 0.2;
    cfg->ik_blending_halflife = 0.1;
    cfg->ik_enabled = 1;
    cfg->blend_enabled = 1;
    cfg->n_contact = 2;                     // :104
    cfg->contact_bones[0] = 5;
    cfg->contact_bones[1] = 24;
}

// The skeleton and the constants of a post-processing launch from cfg (NULL = the demo's), validated: what mocha_postprocess,
// mocha_postprocess_step and mocha_live_step share.  The caller adds the arrays and the clip / frame counts.
static int post_params(mocha_ctx* c, const mocha_post_cfg* cfg, PostParams& p) {
    mocha_post_cfg d;
    if (!cfg) { mocha_post_cfg_default(&d); cfg = &d; }
    const int J = c->cfg.V + 1;
    if (J > MOCHA_MAX_BONES) return fail(c, MOCHA_ERR_ARG, "postprocess: too many bones");
    if (cfg->n_contact < 0 || cfg->n_contact > MOCHA_MAX_CONTACT) return fail(c, MOCHA_ERR_ARG, "postprocess: n_contact must be 0..4");
    if (!(cfg->dt > 0.0)) return fail(c, MOCHA_ERR_ARG, "postprocess: dt must be positive");
    p.V = c->cfg.V; p.n_contact = cfg->n_contact; p.ik_enabled = cfg->ik_enabled;
    p.blend_enabled = cfg->blend_enabled;
    p.parents[0] = -1;                       // parents = [-1] + (joint parents + 1), test_fullframework.py:101-102
    for (int i = 0; i < c->cfg.V; ++i) p.parents[i + 1] = c->sk.parents[i] + 1;
    for (int i = 0; i < cfg->n_contact; ++i) {
        const int toe = cfg->contact_bones[i];
        if (toe < 1 || toe >= J) return fail(c, MOCHA_ERR_ARG, "postprocess: contact bone out of range");
        int depth = 0;
        for (int b = toe; b != -1; b = p.parents[b]) ++depth;
        if (depth < 5 || depth > MOCHA_MAX_CHAIN) return fail(c, MOCHA_ERR_ARG, "postprocess: contact bone needs 4..7 ancestors");
        p.contact_bones[i] = toe;
    }
    p.dt = cfg->dt; p.max_length_buffer = cfg->ik_max_length_buffer; p.foot_height = cfg->ik_foot_height;
    p.unlock_radius = cfg->ik_unlock_radius; p.halflife = cfg->ik_blending_halflife;
    return 0;
}

int mocha_postprocess(mocha_ctx* c, const mocha_post_cfg* cfg, const float* heads, const float* speed, const float* src_rvel,
                      const float* src_rang, const float* src_speed, const unsigned char* contact, int n_clips, int n_frames,
                      double* pos, double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, void* stream) {
    if (c && (n_clips == 0 || n_frames == 0)) return 0;
    if (!c || !heads || !speed || !src_rvel || !src_rang || !src_speed || !contact || !pos || !rot || !ik_rot || n_clips < 0 ||
        n_frames < 0 || (!bvh_pos) != (!bvh_euler))
        return fail(c, MOCHA_ERR_ARG, "bad postprocess arguments");
    PostParams p{};
    { int rc = post_params(c, cfg, p); if (rc) return rc; }
    p.heads = heads; p.speed = speed; p.src_rvel = src_rvel; p.src_rang = src_rang; p.src_speed = src_speed; p.contact = contact;
    p.pos = pos; p.rot = rot; p.ik_rot = ik_rot; p.bvh_pos = bvh_pos; p.bvh_euler = bvh_euler;
    p.n_clips = n_clips; p.n_frames = n_frames;
    const int J = c->cfg.V + 1;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_post_clip", "post.clip", 0.0, (double)n_clips * n_frames * (c->cfg.V * 13.0 * 4 + J * 11.0 * 8),
           launch_post_clip(p, s));
    return 0;
}

// ------------------------------------------------------------------------------------------- resumable post-processing, live sessions
int64_t mocha_post_state_bytes(const mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    return (int64_t)POST_STATE_DOUBLES * (int64_t)sizeof(double);
}

int mocha_postprocess_step(mocha_ctx* c, const mocha_post_cfg* cfg, void* state, const float* heads, const float* speed, const float* src_rvel,
                           const float* src_rang, const float* src_speed, const unsigned char* contact, int n_clips, double* pos, double* rot,
                           double* ik_rot, double* bvh_pos, double* bvh_euler, void* stream) {
    if (c && n_clips == 0) return 0;
    if (!c || !state || !heads || !speed || !src_rvel || !src_rang || !src_speed || !contact || !pos || !rot || !ik_rot || n_clips < 0 ||
        (!bvh_pos) != (!bvh_euler))
        return fail(c, MOCHA_ERR_ARG, "bad postprocess_step arguments: null argument");
    PostParams p{};
    { int rc = post_params(c, cfg, p); if (rc) return rc; }
    p.heads = heads; p.speed = speed; p.src_rvel = src_rvel; p.src_rang = src_rang; p.src_speed = src_speed; p.contact = contact;
    p.pos = pos; p.rot = rot; p.ik_rot = ik_rot; p.bvh_pos = bvh_pos; p.bvh_euler = bvh_euler;
    p.n_clips = n_clips; p.n_frames = 1; p.state = static_cast<double*>(state);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_post_clip", "post.step", 0.0, (double)n_clips * (c->cfg.V * 13.0 * 4 + (c->cfg.V + 1) * 11.0 * 8 + 2.0 * POST_STATE_DOUBLES * 8),
           launch_post_step(p, s));
    return 0;
}

}  // extern "C"

namespace {
// A live session's buffer (caller-owned device memory, private layout): per stream the ring counters, the post state, the ring and the
// step's staging.  Every section starts on a 256-byte boundary.
struct LiveLayout {
    size_t counters, post, rot, pos, vel, ang, xraw, y, heads, speed, eff, bytes;
};
LiveLayout live_layout(const mocha_ctx* c, int S) {
    const size_t J = (size_t)c->cfg.V + 1, V = (size_t)c->cfg.V, T = LIVE_WINDOW, n = (size_t)S;
    LiveLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.counters = take(n * 2 * sizeof(int32_t));
    l.post = take(n * POST_STATE_DOUBLES * sizeof(double));
    l.rot = take(n * T * J * 4 * sizeof(float));
    l.pos = take(n * T * J * 3 * sizeof(float));
    l.vel = take(n * T * J * 3 * sizeof(float));
    l.ang = take(n * T * J * 3 * sizeof(float));
    l.xraw = take(n * T * J * (size_t)c->cfg.C_in * sizeof(float));
    l.y = take(n * T * V * (size_t)c->cfg.C_in * sizeof(float));
    l.heads = take(n * V * 13 * sizeof(float));
    l.speed = take(n * sizeof(float));
    l.eff = take(n * sizeof(int32_t));
    l.bytes = off;
    return l;
}

// The arguments of the live steps, in the groups that travel together.  The session: the post configuration (NULL: the demo's), the
// session buffer, the streams' character ids (a mix step: its component ids) and the z-score
struct LiveCall {
    const mocha_post_cfg* cfg = nullptr; void* live = nullptr; int streams = 0; const int32_t* seg = nullptr;
    const float *cnt_mean = nullptr, *cnt_std = nullptr; void* stream = nullptr;
};
// ... the featurised frame of every stream (the raw steps: the front end's staging) ...
struct LiveFrame {
    const float *Yrot = nullptr, *Ypos = nullptr, *Yvel = nullptr, *Yang = nullptr, *src_rvel = nullptr, *src_rang = nullptr, *src_speed = nullptr;
    const unsigned char* contact = nullptr;
};
// ... the posed frame and the match the step writes (bvh_pos / bvh_euler: both or neither) ...
struct LiveOut {
    double *pos = nullptr, *rot = nullptr, *ik_rot = nullptr, *bvh_pos = nullptr, *bvh_euler = nullptr;
    int32_t *idx = nullptr, *valid = nullptr;
};
// ... and the optional stages of mocha_live_step's family, each checked by its entry point: the soft matcher (k >= 1; a mix step: w_k is
// its wnorm), the inertializer, the mocap front end in front of the push, the action constraint, the mix
struct LiveStages {
    int k = 0; float temperature = 0.f; int32_t* idx_k = nullptr; float* w_k = nullptr;
    void* inert = nullptr; mocha_inert_cfg icfg{};
    const IngestParams* ingest = nullptr; const mocha_ingest_cfg* ingest_cfg = nullptr;
    const AllowArg* allow = nullptr;
    const MixArg* mix = nullptr;
    const PathStepArg* path = nullptr;                 // the online path in the hard matcher's place (alone: no soft, inert, allow or mix)
};

// A live session's buffer as the steps use it, with what mocha_live_step and mocha_live_step_ours make of their common arguments: the
// post configuration in force, the post-processing launch's parameters and the key fields every live step has
struct LiveView {
    LiveRing ring;
    float *xraw = nullptr, *ystage = nullptr, *heads = nullptr, *speed = nullptr;
    int32_t* eff = nullptr;
    PostParams post{};
    mocha_ctx::StepKey key;
};

// the argument checks the live steps share (`who` names the step in the messages) ...
int live_args(mocha_ctx* c, const char* who, const LiveCall& a, const LiveFrame& f, const LiveOut& o) {
    if (a.streams < 1 || a.streams > 16) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= streams <= 16", who);
    if (!a.live || !f.Yrot || !f.Ypos || !f.Yvel || !f.Yang || !f.src_rvel || !f.src_rang || !f.src_speed || !f.contact || !a.seg || !a.cnt_mean ||
        !a.cnt_std || !o.pos || !o.rot || !o.ik_rot || !o.idx || !o.valid || (!o.bvh_pos) != (!o.bvh_euler))
        return fail(c, MOCHA_ERR_ARG, "%s: null argument", who);
    return 0;
}
// ... the state checks ...
int live_state(mocha_ctx* c, const char* who) {
    if (!c->finalized) return fail(c, MOCHA_ERR_STATE, "weights not finalised: call mocha_finalize_weights first");
    if (!c->pose_norm.p) return fail(c, MOCHA_ERR_STATE, "%s: no pose norm: call mocha_set_pose_norm first", who);
    if (!c->bank.cnt) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set_segments first");
    if (!c->bank.segmented()) return fail(c, MOCHA_ERR_STATE, "no segment table: call mocha_bank_set_segments first");
    return 0;
}
// ... and the view: everything the captured region needs exists when it returns (the workspaces, the skeleton's parents; the segmented
// matcher's scratch was sized by mocha_bank_set_segments)
int live_view(mocha_ctx* c, const LiveCall& a, const LiveFrame& f, const LiveOut& o, LiveView& v) {
    mocha_post_cfg d;
    const mocha_post_cfg* cfg = a.cfg;
    if (!cfg) { mocha_post_cfg_default(&d); cfg = &d; }
    int rc = post_params(c, cfg, v.post); if (rc) return rc;
    if ((rc = ready(c, a.streams))) return rc;
    if ((rc = ensure_bone_parents(c))) return rc;
    const LiveLayout l = live_layout(c, a.streams);
    char* base = static_cast<char*>(a.live);
    auto f32 = [&](size_t at) { return reinterpret_cast<float*>(base + at); };
    v.ring.counters = reinterpret_cast<int32_t*>(base + l.counters);
    v.ring.rot = f32(l.rot); v.ring.pos = f32(l.pos); v.ring.vel = f32(l.vel); v.ring.ang = f32(l.ang);
    v.xraw = f32(l.xraw); v.ystage = f32(l.y); v.heads = f32(l.heads); v.speed = f32(l.speed);
    v.eff = reinterpret_cast<int32_t*>(base + l.eff);
    PostParams& p = v.post;
    p.heads = v.heads; p.speed = v.speed; p.src_rvel = f.src_rvel; p.src_rang = f.src_rang; p.src_speed = f.src_speed; p.contact = f.contact;
    p.pos = o.pos; p.rot = o.rot; p.ik_rot = o.ik_rot; p.bvh_pos = o.bvh_pos; p.bvh_euler = o.bvh_euler;
    p.n_clips = a.streams; p.n_frames = 1; p.state = reinterpret_cast<double*>(base + l.post); p.valid = o.valid;
    mocha_ctx::StepKey& key = v.key;
    key.x = a.live; key.mean = a.cnt_mean; key.sd = a.cnt_std; key.idx = o.idx; key.seg = a.seg; key.windows = a.streams; key.raw = true;
    const void* ptrs[14] = {f.Yrot, f.Ypos, f.Yvel, f.Yang, f.src_rvel, f.src_rang, f.src_speed, f.contact, o.pos, o.rot, o.ik_rot, o.bvh_pos, o.bvh_euler, o.valid};
    for (int i = 0; i < 14; ++i) key.live[i] = ptrs[i];
    key.post = *cfg;
    return 0;
}
}  // namespace

extern "C" {

int64_t mocha_live_state_bytes(const mocha_ctx* c, int streams) {
    if (!c || streams < 1 || streams > 16) return MOCHA_ERR_ARG;
    return (int64_t)live_layout(c, streams).bytes;
}

int mocha_live_reset(mocha_ctx* c, void* live, int streams, const int32_t* which, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (streams < 1 || streams > 16) return fail(c, MOCHA_ERR_ARG, "live_reset: 1 <= streams <= 16");
    if (!live) return fail(c, MOCHA_ERR_ARG, "live_reset: null argument");
    if (which && (n < 0 || n > streams)) return fail(c, MOCHA_ERR_ARG, "live_reset: n must be 0..streams");
    for (int i = 0; which && i < n; ++i)
        if (which[i] < 0 || which[i] >= streams) return fail(c, MOCHA_ERR_ARG, "live_reset: stream %d out of range 0..%d", (int)which[i], streams - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const LiveLayout l = live_layout(c, streams);
    char* base = static_cast<char*>(live);
    const size_t pb = POST_STATE_DOUBLES * sizeof(double), cb = 2 * sizeof(int32_t);
    if (!which) {
        HIPCHK(c, hipMemsetAsync(base + l.counters, 0, cb * streams, s));
        HIPCHK(c, hipMemsetAsync(base + l.post, 0, pb * streams, s));
        return 0;
    }
    for (int i = 0; i < n; ++i) {
        HIPCHK(c, hipMemsetAsync(base + l.counters + cb * which[i], 0, cb, s));
        HIPCHK(c, hipMemsetAsync(base + l.post + pb * which[i], 0, pb, s));
    }
    return 0;
}

// The graph of a step of mocha_live_step's family: mix and allow steps have one each per input form (featurised / raw); the others one
// per input form for the hard, the soft and the inertialized (hard or soft) step
static mocha_ctx::StepKind live_step_kind(bool mix, bool allow, bool ingest, bool inert, bool soft, bool path = false) {
    if (path) return ingest ? mocha_ctx::STEP_LIVE_RAW_PATH : mocha_ctx::STEP_LIVE_PATH;
    if (mix) return ingest ? mocha_ctx::STEP_LIVE_RAW_MIX : mocha_ctx::STEP_LIVE_MIX;
    if (allow) return ingest ? mocha_ctx::STEP_LIVE_RAW_ALLOW : mocha_ctx::STEP_LIVE_ALLOW;
    if (ingest) return inert ? mocha_ctx::STEP_LIVE_RAW_INERT : soft ? mocha_ctx::STEP_LIVE_RAW_SOFT : mocha_ctx::STEP_LIVE_RAW;
    return inert ? mocha_ctx::STEP_LIVE_INERT : soft ? mocha_ctx::STEP_LIVE_SOFT : mocha_ctx::STEP_LIVE;
}

// The body of mocha_live_step and of every step of its family (`st`: which optional stages run; the entry points checked them)
static int live_step_impl(mocha_ctx* c, const LiveCall& a, const LiveFrame& f, const LiveOut& o, const LiveStages& st) {
    int rc = live_args(c, "live_step", a, f, o); if (rc) return rc;
    if ((rc = live_state(c, "live_step"))) return rc;
    const AllowArg* al = st.allow;
    const MixArg* mx = st.mix;
    const IngestParams* ing = st.ingest;
    if (al && !c->bank.labelled) return fail(c, MOCHA_ERR_STATE, "no action labels: call mocha_bank_set_labels first");
    if (mx && !c->sets[0].mix_zero.p) return no_seg_scratch(c, 0);
    if (st.path && (rc = path_step_bank(c, "live_step_path", st.path->state_rows))) return rc;
    LiveView v;
    if ((rc = live_view(c, a, f, o, v))) return rc;
    const int streams = a.streams, J = c->cfg.V + 1, V = c->cfg.V;
    const SegWindows win{v.xraw, streams, a.cnt_mean, a.cnt_std, v.ystage, true};

    // The segmented characterize of the S staging windows with the ids in eff: hard, or soft with column 0 of idx_k in idx.  A mix step:
    // the mix characterize, gated by the push (eff >= 0: the ring is full and a frame came); with the step's outputs (ix non-null) the
    // matcher also rewrites valid - a stream none of whose components is present sits the step out
    auto characterize = [&](int32_t* ix, int32_t* ixk, float* wk, hipStream_t cs) -> int {
        MixArg m;
        SegSelect sel; sel.seg = v.eff; sel.k = st.k; sel.temperature = st.temperature; sel.allow = al; sel.idx0 = ix; sel.idx_k = ixk; sel.w_k = wk;
        if (mx) { m = MixArg{mx->ids, mx->weights, mx->J, ix, nullptr, wk, v.eff, ix ? o.valid : nullptr}; sel.mix = &m; }
        // (the characterize before a capture, ix null, is the plain hard one: it must not move the path state, and the path adds no
        // kernel that makes anything on first use)
        if (st.path && ix) sel.path = st.path;
        return characterize_segmented_set0(c, win, sel, cs);
    };
    // ring push + featurize -> segmented characterize of the S windows with the effective ids -> pose heads -> one post-processing frame
    auto body = [&](hipStream_t cs) -> int {
        // mocha_live_step_raw: the front end writes the frame the push reads (`f` is its staging) and says which streams have one
        if (ing)
            LAUNCH(c, cs, "mocha_live_ingest", "live.ingest", 0.0, (double)streams * (V * 7.0 * 4 + J * 13.0 * 4 + 40.0 * 4 * 8 + J * 16.0 * 13 * 8),
                   launch_live_ingest(*ing, streams, cs));
        LAUNCH(c, cs, "mocha_live_push", "live.push", streams * 60.0 * J * 150, streams * (60.0 * J * (13 + 15) + J * 26.0) * 4,
               launch_live_push(v.ring, f.Yrot, f.Ypos, f.Yvel, f.Yang, mx ? c->sets[0].mix_zero.p : a.seg, c->bone_parents.p, v.xraw, v.eff, o.valid,
                                streams, J, cs, ing ? ing->have : nullptr, c->bank.resident && !mx ? c->bank.seg_dev.p : nullptr,
                                c->bank.resident && !mx ? c->bank.segments() : 0));
        // (a mix step's push takes zero ids and no slot table: its eff is the gate alone; which characters are loaded is the matcher's to read)
        const int r = characterize(o.idx, st.idx_k, st.w_k, cs);
        if (r) return r;
        LAUNCH(c, cs, "mocha_pose_heads", "live.heads", 0.0, streams * (60.0 * 12 + V * 28.0 * 4), launch_pose_heads(v.ystage, v.heads, v.speed, streams, c->cfg.T, V, cs));
        // mocha_live_step_inert: the staged heads inertialized in place, on the step's effective ids and its valid flags
        if (st.inert)
            LAUNCH(c, cs, "mocha_inertialize", "live.inert", 0.0, (double)streams * (V * 26.0 * 4 + 2.0 * INERT_STATE_DOUBLES * 8),
                   launch_inertialize(static_cast<double*>(st.inert), v.heads, v.heads, v.eff, nullptr, o.valid, streams, V, st.icfg.halflife,
                                      st.icfg.dt, cs));
        LAUNCH(c, cs, "mocha_post_clip", "live.post", 0.0, (double)streams * (V * 13.0 * 4 + J * 11.0 * 8 + 2.0 * POST_STATE_DOUBLES * 8),
               launch_post_step(v.post, cs));
        return 0;
    };
    hipStream_t s = (hipStream_t)a.stream;
    // while profiling (mocha_profile_start) the step runs eagerly, launch by launch, so that every kernel of it is timed
    if (c->prof_on) return body(s);

    mocha_ctx::StepKey& key = v.key;
    key.soft_k = st.k; key.soft_t = st.k > 0 ? st.temperature : 0.f; key.soft[0] = st.k > 0 ? st.idx_k : nullptr; key.soft[1] = st.k > 0 ? st.w_k : nullptr;
    if (st.inert) { key.inert = st.inert; key.inert_halflife = st.icfg.halflife; key.inert_dt = st.icfg.dt; }
    if (ing) { key.ingest[0] = ing->state; key.ingest[1] = ing->rot; key.ingest[2] = ing->pos; key.icfg = *st.ingest_cfg; }
    if (al) { key.allow[0] = al->allow; key.allow[1] = al->applied; }
    if (mx) { key.mix_j = mx->J; key.mix[0] = mx->weights; key.mix[1] = st.w_k; }
    if (st.path) {
        key.path[0] = st.path->state; key.path[1] = st.path->restart; key.path[2] = st.path->dist; key.path[3] = st.path->continued;
        key.path_rows = st.path->state_rows; key.path_lambda = st.path->lambda;
    }
    mocha_ctx::StepGraph& g = c->steps[live_step_kind(mx, al, ing, st.inert, st.k > 0, st.path != nullptr)];
    if (!step_holds(c, g, key)) {
        // Before a capture: one eager characterize of the staging windows with every id -1 (no bank row is matched, no state of the
        // session moves), so that whatever the kernels of the step make on first use - the plane GEMMs' weight images, for the soft step
        // the float64 weights of the literal decoder's style MLP - exists and the captured step takes the kernels every later step takes.
        HIPCHK(c, hipMemsetAsync(v.xraw, 0, (size_t)streams * 60 * J * c->cfg.C_in * sizeof(float), s));
        HIPCHK(c, hipMemsetAsync(v.eff, 0xFF, (size_t)streams * sizeof(int32_t), s));
        if ((rc = characterize(nullptr, nullptr, nullptr, s))) return rc;
    }
    return step_replay(c, g, key, s, body);
}

int mocha_live_step(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                    const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                    const int32_t* seg, const float* cnt_mean, const float* cnt_std, double* pos, double* rot, double* ik_rot, double* bvh_pos,
                    double* bvh_euler, int32_t* idx, int32_t* valid, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_impl(c, a, f, o, LiveStages{});
}

int mocha_live_step_soft(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                         const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                         const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k, float temperature, double* pos, double* rot,
                         double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* idx_k, float* w_k, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = soft_args(c, "live_step_soft", k, temperature); if (rc) return rc;
    if (!idx_k || !w_k) return fail(c, MOCHA_ERR_ARG, "live_step_soft: null argument");
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    LiveStages st; st.k = k; st.temperature = temperature; st.idx_k = idx_k; st.w_k = w_k;
    return live_step_impl(c, a, f, o, st);
}

// the soft stage of the steps that take k = 0 for the hard matcher, as the caller gave it: checked, and cleared when k = 0
static int live_soft_check(mocha_ctx* c, const char* who, LiveStages& st) {
    if (st.k == 0) { st.temperature = 0.f; st.idx_k = nullptr; if (!st.mix) st.w_k = nullptr; return 0; }
    int rc = soft_args(c, who, st.k, st.temperature); if (rc) return rc;
    if (!st.idx_k || !st.w_k) return fail(c, MOCHA_ERR_ARG, "%s: null argument", who);
    return 0;
}

// cfg (NULL = half-life 0.1 s at 60 frames per second) checked and copied into `out`
static int inert_cfg(mocha_ctx* c, const char* who, const mocha_inert_cfg* cfg, mocha_inert_cfg& out) {
    out = cfg ? *cfg : mocha_inert_cfg{0.1, 1.0 / 60.0};
    if (!std::isfinite(out.halflife) || !std::isfinite(out.dt) || out.halflife < 0.0 || !(out.dt > 0.0))
        return fail(c, MOCHA_ERR_ARG, "%s: halflife must be finite and >= 0, dt finite and > 0", who);
    return 0;
}

int64_t mocha_inert_state_bytes(const mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    return (int64_t)INERT_STATE_DOUBLES * (int64_t)sizeof(double);
}

int mocha_inertialize_step(mocha_ctx* c, const mocha_inert_cfg* cfg, void* state, const float* heads_in, float* heads_out, const int32_t* ids,
                           const int32_t* trigger, const int32_t* valid, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    mocha_inert_cfg ic;
    int rc = inert_cfg(c, "inertialize_step", cfg, ic); if (rc) return rc;
    if (n < 0) return fail(c, MOCHA_ERR_ARG, "inertialize_step: n must not be negative");
    if (n == 0) return 0;
    if (!state || !heads_in || !heads_out) return fail(c, MOCHA_ERR_ARG, "inertialize_step: null argument");
    if (c->cfg.V + 1 > MOCHA_MAX_BONES) return fail(c, MOCHA_ERR_ARG, "inertialize_step: too many bones");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_inertialize", "post.inert", 0.0, (double)n * (c->cfg.V * 26.0 * 4 + 2.0 * INERT_STATE_DOUBLES * 8),
           launch_inertialize(static_cast<double*>(state), heads_in, heads_out, ids, trigger, valid, n, c->cfg.V, ic.halflife, ic.dt, s));
    return 0;
}

int mocha_live_step_inert(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                          const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                          const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k, float temperature, double* pos, double* rot,
                          double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* idx_k, float* w_k, void* stream,
                          void* inert, const mocha_inert_cfg* icfg) {
    if (!c) return MOCHA_ERR_ARG;
    LiveStages st; st.k = k; st.temperature = temperature; st.idx_k = idx_k; st.w_k = w_k; st.inert = inert;
    int rc = live_soft_check(c, "live_step_inert", st); if (rc) return rc;
    if (!inert) return fail(c, MOCHA_ERR_ARG, "live_step_inert: null inertializer state");
    if ((rc = inert_cfg(c, "live_step_inert", icfg, st.icfg))) return rc;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_impl(c, a, f, o, st);
}

// mocha_live_step_inert's arguments (inert may be NULL: no inertializer; k = 0: the hard matcher) with the streams' allow masks: the
// characterize of the step is the action-constrained one.  A warming stream has the id -1 and so applied 0.
int mocha_live_step_allow(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                          const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                          const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k, float temperature, double* pos, double* rot,
                          double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* idx_k, float* w_k, void* stream,
                          void* inert, const mocha_inert_cfg* icfg, const uint64_t* allow, int32_t* applied) {
    if (!c) return MOCHA_ERR_ARG;
    LiveStages st; st.k = k; st.temperature = temperature; st.idx_k = idx_k; st.w_k = w_k; st.inert = inert;
    int rc = live_soft_check(c, "live_step_allow", st); if (rc) return rc;
    if (!allow) return fail(c, MOCHA_ERR_ARG, "live_step_allow: null allow masks");
    if (inert && (rc = inert_cfg(c, "live_step_allow", icfg, st.icfg))) return rc;
    const AllowArg al{reinterpret_cast<const unsigned long long*>(allow), applied};
    st.allow = &al;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_impl(c, a, f, o, st);
}

}  // extern "C"

namespace {
// The mocap front end's buffer (caller-owned device memory, private layout): per stream the kernel's state row, then the staging
// mocha_live_step_raw hands to the live step.  Every section starts on a 256-byte boundary.
struct IngestLayout {
    size_t state, rot, pos, vel, ang, rvel, rang, speed, contact, have, bytes;
};
IngestLayout ingest_layout(const mocha_ctx* c, int S) {
    const size_t J = (size_t)c->cfg.V + 1, n = (size_t)S;
    IngestLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.state = take(n * INGEST_STATE_DOUBLES * sizeof(double));
    l.rot = take(n * J * 4 * sizeof(float));
    l.pos = take(n * J * 3 * sizeof(float));
    l.vel = take(n * J * 3 * sizeof(float));
    l.ang = take(n * J * 3 * sizeof(float));
    l.rvel = take(n * 3 * sizeof(float));
    l.rang = take(n * 3 * sizeof(float));
    l.speed = take(n * sizeof(float));
    l.contact = take(n * MOCHA_MAX_CONTACT);
    l.have = take(n * sizeof(int32_t));
    l.bytes = off;
    return l;
}

// rows of A (A^T A)^-1 A^T for the cubic Vandermonde matrix on the centred abscissae of a W-sample window, in long double
void fit_rows(int W, double* out) {
    std::vector<long double> A((size_t)W * 4);
    for (int r = 0; r < W; ++r) {
        const long double x = (long double)r - (long double)(W - 1) / 2;
        A[r * 4] = 1; A[r * 4 + 1] = x; A[r * 4 + 2] = x * x; A[r * 4 + 3] = x * x * x;
    }
    long double M[4][8] = {};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 4; ++j)
            for (int r = 0; r < W; ++r) M[i][j] += A[r * 4 + i] * A[r * 4 + j];
        M[i][4 + i] = 1;
    }
    for (int col = 0; col < 4; ++col) {                      // Gauss-Jordan with partial pivoting
        int piv = col;
        for (int r = col + 1; r < 4; ++r) if (std::fabs(M[r][col]) > std::fabs(M[piv][col])) piv = r;
        for (int j = 0; j < 8; ++j) std::swap(M[col][j], M[piv][j]);
        const long double d = M[col][col];
        for (int j = 0; j < 8; ++j) M[col][j] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const long double f = M[r][col];
            for (int j = 0; j < 8; ++j) M[r][j] -= f * M[col][j];
        }
    }
    for (int r = 0; r < W; ++r)
        for (int q = 0; q < W; ++q) {
            long double acc = 0;
            for (int i = 0; i < 4; ++i) {
                long double t = 0;
                for (int j = 0; j < 4; ++j) t += M[i][4 + j] * A[q * 4 + j];
                acc += A[r * 4 + i] * t;
            }
            out[(size_t)r * W + q] = (double)acc;
        }
}

// the fit rows on the device, uploaded once: before any capture
int ensure_ingest_rows(mocha_ctx* c) {
    if (c->ingest_rows.p) return 0;
    std::vector<double> rows(15 * 15 + 31 * 31);
    fit_rows(15, rows.data());
    fit_rows(31, rows.data() + 15 * 15);
    int rc = reserve(c, c->ingest_rows, rows.size()); if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->ingest_rows.p, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    return 0;
}

// cfg and the toes of `post` (NULL = the demo's) checked and copied into the kernel's parameters; the caller adds the pointers
int ingest_params(mocha_ctx* c, const char* who, const mocha_ingest_cfg* cfg, const mocha_post_cfg* post, IngestParams& p) {
    if (!cfg) return fail(c, MOCHA_ERR_ARG, "%s: null ingest configuration", who);
    mocha_post_cfg d;
    if (!post) { mocha_post_cfg_default(&d); post = &d; }
    PostParams pp{};
    int rc = post_params(c, post, pp); if (rc) return rc;      // bone count, n_contact, the toes and their chains
    const int V = c->cfg.V;
    if (cfg->lookahead < 0 || cfg->lookahead > INGEST_MAX_LOOKAHEAD) return fail(c, MOCHA_ERR_ARG, "%s: lookahead must be 0..%d", who, INGEST_MAX_LOOKAHEAD);
    if (cfg->rot_format < 0 || cfg->rot_format > 1) return fail(c, MOCHA_ERR_ARG, "%s: rot_format must be 0 (quaternions) or 1 (Euler degrees)", who);
    int seen = 0;
    for (int i = 0; i < 3; ++i) {
        if (cfg->euler_order[i] < 0 || cfg->euler_order[i] > 2) return fail(c, MOCHA_ERR_ARG, "%s: euler_order must name the axes 0..2", who);
        seen |= 1 << cfg->euler_order[i];
    }
    if (seen != 7) return fail(c, MOCHA_ERR_ARG, "%s: euler_order must be a permutation of 0..2", who);
    if (!std::isfinite(cfg->unit_scale) || !std::isfinite(cfg->fps) || !std::isfinite(cfg->contact_velocity_threshold) || !(cfg->fps > 0.0))
        return fail(c, MOCHA_ERR_ARG, "%s: unit_scale, fps and contact_velocity_threshold must be finite, fps positive", who);
    const int roles[5] = {cfg->spine, cfg->shoulder_l, cfg->shoulder_r, cfg->upleg_l, cfg->upleg_r};
    for (int i = 0; i < 5; ++i)
        if (roles[i] < 0 || roles[i] >= V) return fail(c, MOCHA_ERR_ARG, "%s: role joint %d out of range 0..%d", who, roles[i], V - 1);
    if (c->sk.parents[0] != -1) return fail(c, MOCHA_ERR_ARG, "%s: joint 0 must be the hips (no parent)", who);
    for (int v = 1; v < V; ++v)
        if (c->sk.parents[v] < 0 || c->sk.parents[v] >= v) return fail(c, MOCHA_ERR_ARG, "%s: joint %d does not follow its parent", who, v);
    p.V = V; p.lookahead = cfg->lookahead; p.euler = cfg->rot_format;
    for (int i = 0; i < 3; ++i) p.order[i] = cfg->euler_order[i];
    for (int i = 0; i < 5; ++i) p.roles[i] = roles[i];
    p.n_contact = pp.n_contact;
    for (int i = 0; i < pp.n_contact; ++i) p.contact_bones[i] = pp.contact_bones[i];
    for (int v = 0; v < V; ++v) p.parents[v] = c->sk.parents[v];
    p.scale = cfg->unit_scale; p.fps = cfg->fps; p.threshold = cfg->contact_velocity_threshold;
    return 0;
}
}  // namespace

extern "C" {

void mocha_ingest_cfg_default(mocha_ingest_cfg* cfg, int layout) {
    if (!cfg) return;
    *cfg = mocha_ingest_cfg{};
    cfg->lookahead = 0;
    cfg->rot_format = 1;                                       // a BVH file's channels: Euler degrees, 'zyx'
    cfg->euler_order[0] = 2; cfg->euler_order[1] = 1; cfg->euler_order[2] = 0;
    cfg->unit_scale = 0.01;                                    // generate_database.py:91
    cfg->fps = 60.0;                                           // :140
    cfg->contact_velocity_threshold = 0.5;                     // :162
    if (layout == 1) { cfg->spine = 3; cfg->shoulder_l = 6; cfg->shoulder_r = 10; cfg->upleg_l = 18; cfg->upleg_r = 14; }
    else { cfg->spine = 7; cfg->shoulder_l = 9; cfg->shoulder_r = 16; cfg->upleg_l = 1; cfg->upleg_r = 20; }   // :102, :109-111
}

int64_t mocha_ingest_state_bytes(const mocha_ctx* c, int streams) {
    if (!c || streams < 1 || streams > 16) return MOCHA_ERR_ARG;
    return (int64_t)ingest_layout(c, streams).bytes;
}

int mocha_ingest_reset(mocha_ctx* c, void* ingest, int streams, const int32_t* which, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (streams < 1 || streams > 16) return fail(c, MOCHA_ERR_ARG, "ingest_reset: 1 <= streams <= 16");
    if (!ingest) return fail(c, MOCHA_ERR_ARG, "ingest_reset: null argument");
    if (which && (n < 0 || n > streams)) return fail(c, MOCHA_ERR_ARG, "ingest_reset: n must be 0..streams");
    for (int i = 0; which && i < n; ++i)
        if (which[i] < 0 || which[i] >= streams) return fail(c, MOCHA_ERR_ARG, "ingest_reset: stream %d out of range 0..%d", (int)which[i], streams - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ingest) + ingest_layout(c, streams).state;
    const size_t row = INGEST_STATE_DOUBLES * sizeof(double);
    if (!which) { HIPCHK(c, hipMemsetAsync(base, 0, row * streams, s)); return 0; }
    for (int i = 0; i < n; ++i) HIPCHK(c, hipMemsetAsync(base + row * which[i], 0, row, s));
    return 0;
}

int mocha_live_ingest_step(mocha_ctx* c, const mocha_ingest_cfg* cfg, const mocha_post_cfg* post, void* ingest, int streams, const float* rot,
                           const float* pos, float* Yrot, float* Ypos, float* Yvel, float* Yang, float* src_rvel, float* src_rang,
                           float* src_speed, unsigned char* contact, int32_t* have, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (streams < 1 || streams > 16) return fail(c, MOCHA_ERR_ARG, "live_ingest_step: 1 <= streams <= 16");
    if (!ingest || !rot || !pos || !Yrot || !Ypos || !Yvel || !Yang || !src_rvel || !src_rang || !src_speed || !contact || !have)
        return fail(c, MOCHA_ERR_ARG, "live_ingest_step: null argument");
    IngestParams p{};
    int rc = ingest_params(c, "live_ingest_step", cfg, post, p); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_ingest_rows(c))) return rc;
    p.state = reinterpret_cast<double*>(static_cast<char*>(ingest) + ingest_layout(c, streams).state);
    p.rows15 = c->ingest_rows.p; p.rows31 = c->ingest_rows.p + 15 * 15;
    p.rot = rot; p.pos = pos; p.Yrot = Yrot; p.Ypos = Ypos; p.Yvel = Yvel; p.Yang = Yang; p.src_rvel = src_rvel; p.src_rang = src_rang;
    p.src_speed = src_speed; p.contact = contact; p.have = have;
    hipStream_t s = (hipStream_t)stream;
    const int V = c->cfg.V, J = V + 1;
    LAUNCH(c, s, "mocha_live_ingest", "ingest.step", 0.0, (double)streams * (V * 7.0 * 4 + J * 13.0 * 4 + 40.0 * 4 * 8 + J * 16.0 * 13 * 8),
           launch_live_ingest(p, streams, s));
    return 0;
}

// The raw steps (`who`): the front end's parameters from icfg_in and the raw frame, its staging in `ingest` as the live step's frame.
// st: the soft stage and the inertializer's state as the caller gave them (icfg: its configuration, NULL = the default), checked here
static int live_step_raw_impl(mocha_ctx* c, const char* who, const LiveCall& a, const mocha_ingest_cfg* icfg_in, void* ingest, const float* rot,
                              const float* pos, const LiveOut& o, LiveStages st, const mocha_inert_cfg* icfg) {
    if (!c) return MOCHA_ERR_ARG;
    if (a.streams < 1 || a.streams > 16) return fail(c, MOCHA_ERR_ARG, "%s: 1 <= streams <= 16", who);
    if (!ingest || !rot || !pos) return fail(c, MOCHA_ERR_ARG, "%s: null argument", who);
    int rc = live_soft_check(c, who, st); if (rc) return rc;
    if (st.inert && (rc = inert_cfg(c, who, icfg, st.icfg))) return rc;
    IngestParams p{};
    if ((rc = ingest_params(c, who, icfg_in, a.cfg, p))) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_ingest_rows(c))) return rc;
    const IngestLayout l = ingest_layout(c, a.streams);
    char* base = static_cast<char*>(ingest);
    auto f32 = [&](size_t at) { return reinterpret_cast<float*>(base + at); };
    p.state = reinterpret_cast<double*>(base + l.state);
    p.rows15 = c->ingest_rows.p; p.rows31 = c->ingest_rows.p + 15 * 15;
    p.rot = rot; p.pos = pos; p.Yrot = f32(l.rot); p.Ypos = f32(l.pos); p.Yvel = f32(l.vel); p.Yang = f32(l.ang);
    p.src_rvel = f32(l.rvel); p.src_rang = f32(l.rang); p.src_speed = f32(l.speed);
    p.contact = reinterpret_cast<unsigned char*>(base + l.contact); p.have = reinterpret_cast<int32_t*>(base + l.have);
    LiveFrame f; f.Yrot = p.Yrot; f.Ypos = p.Ypos; f.Yvel = p.Yvel; f.Yang = p.Yang; f.src_rvel = p.src_rvel; f.src_rang = p.src_rang; f.src_speed = p.src_speed; f.contact = p.contact;
    st.ingest = &p; st.ingest_cfg = icfg_in;
    return live_step_impl(c, a, f, o, st);
}

int mocha_live_step_raw(mocha_ctx* c, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                        const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                        float temperature, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                        int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert, const mocha_inert_cfg* icfg) {
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveOut o; o.pos = pos_out; o.rot = rot_out; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    LiveStages st; st.k = k; st.temperature = temperature; st.idx_k = idx_k; st.w_k = w_k; st.inert = inert;
    return live_step_raw_impl(c, "live_step_raw", a, icfg_in, ingest, rot, pos, o, st, icfg);
}

int mocha_live_step_raw_allow(mocha_ctx* c, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                              const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std, int k,
                              float temperature, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx,
                              int32_t* valid, int32_t* idx_k, float* w_k, void* stream, void* inert, const mocha_inert_cfg* icfg,
                              const uint64_t* allow, int32_t* applied) {
    if (!c) return MOCHA_ERR_ARG;
    if (!allow) return fail(c, MOCHA_ERR_ARG, "live_step_raw_allow: null allow masks");
    const AllowArg al{reinterpret_cast<const unsigned long long*>(allow), applied};
    LiveStages st; st.k = k; st.temperature = temperature; st.idx_k = idx_k; st.w_k = w_k; st.inert = inert; st.allow = &al;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveOut o; o.pos = pos_out; o.rot = rot_out; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_raw_impl(c, "live_step_raw_allow", a, icfg_in, ingest, rot, pos, o, st, icfg);
}

// The live step with the online path in the hard matcher's place: stream s of the session is stream s of the path state.  A stream that is
// warming, has no frame or names no loaded character has the effective id -1 and sits the path step out.
static int live_path_arg(mocha_ctx* c, const char* who, int streams, void* path_state, int state_rows, double lambda, int32_t* restart, float* dist,
                         unsigned char* continued, PathStepArg& p) {
    int rc = path_step_check(c, who, streams, state_rows, lambda); if (rc) return rc;
    if (!path_state || !dist || !continued) return fail(c, MOCHA_ERR_ARG, "%s: null argument", who);
    p.state = path_state; p.state_rows = state_rows; p.lambda = lambda; p.restart = restart; p.dist = dist; p.continued = continued;
    return 0;
}

int mocha_live_step_path(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                         const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                         const int32_t* seg, const float* cnt_mean, const float* cnt_std, double* pos, double* rot, double* ik_rot, double* bvh_pos,
                         double* bvh_euler, int32_t* idx, int32_t* valid, void* stream, void* path_state, int state_rows, double lambda,
                         int32_t* restart, float* dist, unsigned char* continued) {
    if (!c) return MOCHA_ERR_ARG;
    PathStepArg p;
    int rc = live_path_arg(c, "live_step_path", streams, path_state, state_rows, lambda, restart, dist, continued, p); if (rc) return rc;
    LiveStages st; st.path = &p;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_impl(c, a, f, o, st);
}

int mocha_live_step_raw_path(mocha_ctx* c, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                             const float* rot, const float* pos, const int32_t* seg, const float* cnt_mean, const float* cnt_std, double* pos_out,
                             double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, void* stream,
                             void* path_state, int state_rows, double lambda, int32_t* restart, float* dist, unsigned char* continued) {
    if (!c) return MOCHA_ERR_ARG;
    PathStepArg p;
    int rc = live_path_arg(c, "live_step_raw_path", streams, path_state, state_rows, lambda, restart, dist, continued, p); if (rc) return rc;
    LiveStages st; st.path = &p;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveOut o; o.pos = pos_out; o.rot = rot_out; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_raw_impl(c, "live_step_raw_path", a, icfg_in, ingest, rot, pos, o, st, nullptr);
}

// The live step with the mix characterize in the place of the hard one (ids (S,J), weights (S,J,6): device data every replay reads; idx
// (S,J), wnorm (S,J,6)).  mocha_live_step_mix: frames already featurised; mocha_live_step_raw_mix: raw mocap frames through the front end.
int mocha_live_step_mix(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                        const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                        const int32_t* ids, const float* weights, int J, const float* cnt_mean, const float* cnt_std, double* pos, double* rot,
                        double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, float* wnorm, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = mix_args(c, "live_step_mix", J); if (rc) return rc;
    if (!ids || !weights || !idx || !wnorm) return fail(c, MOCHA_ERR_ARG, "live_step_mix: null argument");
    const MixArg mx{ids, weights, J, idx, nullptr, wnorm, nullptr, nullptr};
    LiveStages st; st.mix = &mx; st.w_k = wnorm;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = ids; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_impl(c, a, f, o, st);
}

int mocha_live_step_raw_mix(mocha_ctx* c, const mocha_post_cfg* cfg, const mocha_ingest_cfg* icfg_in, void* live, void* ingest, int streams,
                            const float* rot, const float* pos, const int32_t* ids, const float* weights, int J, const float* cnt_mean,
                            const float* cnt_std, double* pos_out, double* rot_out, double* ik_rot, double* bvh_pos, double* bvh_euler,
                            int32_t* idx, int32_t* valid, float* wnorm, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = mix_args(c, "live_step_raw_mix", J); if (rc) return rc;
    if (!ids || !weights || !idx || !wnorm) return fail(c, MOCHA_ERR_ARG, "live_step_raw_mix: null argument");
    const MixArg mx{ids, weights, J, idx, nullptr, wnorm, nullptr, nullptr};
    LiveStages st; st.mix = &mx; st.w_k = wnorm;
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = ids; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveOut o; o.pos = pos_out; o.rot = rot_out; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_raw_impl(c, "live_step_raw_mix", a, icfg_in, ingest, rot, pos, o, st, nullptr);
}

}  // extern "C"

namespace {
// clip_offsets of the clip calls: offsets[0] = 0, strictly increasing, every clip at least min_len frames
int clip_offsets_check(mocha_ctx* c, const char* who, const int32_t* off, int n_clips, int min_len) {
    if (!off) return fail(c, MOCHA_ERR_ARG, "%s: null argument", who);
    if (n_clips < 1) return fail(c, MOCHA_ERR_ARG, "%s: n_clips must be at least 1", who);
    if (off[0] != 0) return fail(c, MOCHA_ERR_ARG, "%s: clip_offsets[0] must be 0", who);
    for (int i = 0; i < n_clips; ++i) {
        if (off[i + 1] <= off[i]) return fail(c, MOCHA_ERR_ARG, "%s: clip_offsets must increase (clip %d)", who, i);
        if (off[i + 1] - off[i] < min_len)
            return fail(c, MOCHA_ERR_ARG, "%s: clip %d has %d frames, fewer than %d", who, i, (int)(off[i + 1] - off[i]), min_len);
    }
    return 0;
}

// windows divide_clip(divide=True) cuts from a clip of n frames: j = 0, step, 2 step, ... < n - window / 4 (generate_database.py:67)
int64_t clip_window_count(int64_t n, int window, int step) {
    const int64_t span = n - window / 4;
    return span <= 0 ? 0 : (span + step - 1) / step;
}

// the tables of a clip call at the head of the context's clip buffer, then `doubles` float64 words; the tables are on the device when
// this returns (the stream is waited for once: the host arrays are the caller's)
int clip_tables(mocha_ctx* c, hipStream_t s, const std::vector<int>& tab, size_t doubles, int** tab_dev, double** ws) {
    const size_t head = (tab.size() * sizeof(int) + 255) / 256 * 32;        // doubles, a multiple of 256 bytes
    int rc = reserve(c, c->clip_ws, head + doubles); if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->clip_ws.p, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *tab_dev = reinterpret_cast<int*>(c->clip_ws.p);
    *ws = c->clip_ws.p + head;
    return 0;
}
}  // namespace

extern "C" {

int mocha_mirror_map_default(int layout, int32_t* map) {
    if (!map || layout < 0 || layout > 1) return MOCHA_ERR_ARG;
    // 'mocha': Left* / Right* of the 24 joint names (legs 1-4 / 20-23, arms 9-12 / 16-19); 'mixamo': arms 6-9 / 10-13, legs 14-17 / 18-21
    const int V = layout == 1 ? 22 : 24;
    for (int v = 0; v < V; ++v) map[v] = v;
    auto swap_run = [&](int a, int b, int n) { for (int k = 0; k < n; ++k) { map[a + k] = b + k; map[b + k] = a + k; } };
    if (layout == 1) { swap_run(6, 10, 4); swap_run(14, 18, 4); }
    else { swap_run(1, 20, 4); swap_run(9, 16, 4); }
    return 0;
}

int mocha_clip_window_count(const int32_t* offsets, int n_clips, int window, int step, int64_t* counts) {
    if (!offsets || !counts || n_clips < 1 || window < 4 || step < 1) return MOCHA_ERR_ARG;
    for (int i = 0; i < n_clips; ++i) {
        if (offsets[i + 1] <= offsets[i]) return MOCHA_ERR_ARG;
        counts[i] = clip_window_count((int64_t)offsets[i + 1] - offsets[i], window, step);
    }
    return 0;
}

int mocha_ingest_clips(mocha_ctx* c, const mocha_ingest_cfg* cfg, const mocha_post_cfg* post, const float* rot, const float* pos,
                       const int32_t* clip_offsets, int n_clips, const int32_t* mirror_map, const unsigned char* mirror_flags,
                       float* out_pos, float* out_vel, float* out_rot, float* out_ang, unsigned char* out_contact, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (!cfg) return fail(c, MOCHA_ERR_ARG, "ingest_clips: null ingest configuration");
    if (!rot || !pos || !out_pos || !out_vel || !out_rot || !out_ang || !out_contact) return fail(c, MOCHA_ERR_ARG, "ingest_clips: null argument");
    mocha_ingest_cfg whole = *cfg;
    whole.lookahead = 0;                                       // a whole clip has no lookahead: the field is ignored
    IngestParams ip{};
    int rc = ingest_params(c, "ingest_clips", &whole, post, ip); if (rc) return rc;
    if ((rc = clip_offsets_check(c, "ingest_clips", clip_offsets, n_clips, INGEST_FIRST))) return rc;
    const int V = c->cfg.V, J = V + 1, F = clip_offsets[n_clips];
    bool mirrored = false;
    double mirrored_share = 0.0;                               // of the frames: what the two launches for mirrored clips touch
    for (int i = 0; mirror_flags && i < n_clips; ++i)
        if (mirror_flags[i]) { mirrored = true; mirrored_share += (double)(clip_offsets[i + 1] - clip_offsets[i]) / F; }
    if (mirrored && !mirror_map) return fail(c, MOCHA_ERR_ARG, "ingest_clips: mirror_flags set without a mirror_map");
    ClipParams p{};
    if (mirror_map) {
        for (int v = 0; v < V; ++v)
            if (mirror_map[v] < 0 || mirror_map[v] >= V || mirror_map[mirror_map[v]] != v)
                return fail(c, MOCHA_ERR_ARG, "ingest_clips: mirror_map is no involution at joint %d", v);
        if (mirror_map[0] != 0) return fail(c, MOCHA_ERR_ARG, "ingest_clips: mirror_map must keep the hips");
        for (int v = 1; v < V; ++v)
            if (c->sk.parents[mirror_map[v]] != mirror_map[c->sk.parents[v]])
                return fail(c, MOCHA_ERR_ARG, "ingest_clips: mirror_map does not commute with the parents at joint %d", v);
        for (int v = 0; v < V; ++v) p.map[v] = mirror_map[v];
    }
    HIPCHK(c, hipSetDevice(c->device));
    if ((rc = ensure_ingest_rows(c))) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> tab(clip_offsets, clip_offsets + n_clips + 1);
    for (int i = 0; i < n_clips; ++i) tab.push_back(mirror_flags && mirror_flags[i] ? 1 : 0);
    const size_t nF = (size_t)F, nq = nF * V * 4, np_ = nF * V * 3;
    const size_t doubles = 2 * nq + np_ + nF * 4 + nF * CLIP_ROOT_DOUBLES + (nF * MOCHA_MAX_CONTACT + 7) / 8;
    int* tab_dev = nullptr; double* ws = nullptr;
    if ((rc = clip_tables(c, s, tab, doubles, &tab_dev, &ws))) return rc;
    p.rot = rot; p.pos = pos; p.offsets = tab_dev; p.flags = tab_dev + n_clips + 1;
    p.rows15 = c->ingest_rows.p; p.rows31 = c->ingest_rows.p + 15 * 15;
    p.qraw = ws; p.q = p.qraw + nq; p.p = p.q + nq; p.series = p.p + np_; p.root = p.series + nF * 4;
    p.below = reinterpret_cast<unsigned char*>(p.root + nF * CLIP_ROOT_DOUBLES);
    p.out_pos = out_pos; p.out_vel = out_vel; p.out_rot = out_rot; p.out_ang = out_ang; p.out_contact = out_contact;
    p.F = F; p.C = n_clips; p.V = V; p.euler = ip.euler; p.n_contact = ip.n_contact;
    for (int i = 0; i < 3; ++i) p.order[i] = ip.order[i];
    for (int i = 0; i < 5; ++i) p.roles[i] = ip.roles[i];
    for (int i = 0; i < ip.n_contact; ++i) p.contact_bones[i] = ip.contact_bones[i];
    for (int v = 0; v < V; ++v) {
        p.parents[v] = ip.parents[v];
        p.depth[v] = v == 0 ? 0 : p.depth[ip.parents[v]] + 1;
        p.max_depth = std::max(p.max_depth, p.depth[v]);
    }
    p.scale = ip.scale; p.fps = ip.fps; p.threshold = ip.threshold;
    // bytes per launch: what it reads and writes once (the fit windows and the neighbours of a difference come from cache)
    const double fq = (double)nq * 8, fp = (double)np_ * 8, fr = (double)nF * CLIP_ROOT_DOUBLES * 8, fin = (double)nF * V * (ip.euler ? 6 : 7) * 4;
    LAUNCH(c, s, "mocha_clip_quat", "clip.quat", 0.0, fin + fq + fp, launch_clip_ingest(p, 0, s));
    LAUNCH(c, s, "mocha_clip_unroll", "clip.unroll", 0.0, 2 * fq, launch_clip_ingest(p, 1, s));
    if (mirrored) {
        LAUNCH(c, s, "mocha_clip_mirror", "clip.mirror", 0.0, mirrored_share * 2 * (fq + fp), launch_clip_ingest(p, 2, s));
        LAUNCH(c, s, "mocha_clip_unroll", "clip.unroll_mirrored", 0.0, mirrored_share * 2 * fq, launch_clip_ingest(p, 3, s));
    }
    LAUNCH(c, s, "mocha_clip_series", "clip.series", 0.0, fq + fp + (double)nF * 32, launch_clip_ingest(p, 4, s));
    LAUNCH(c, s, "mocha_clip_root", "clip.root", 0.0, (double)nF * 32 + fr + (double)nF * 56, launch_clip_ingest(p, 5, s));
    LAUNCH(c, s, "mocha_clip_vel", "clip.vel", 0.0, fq + fp + fr + (double)nF * J * 13 * 4 + (double)nF * 4, launch_clip_ingest(p, 6, s));
    LAUNCH(c, s, "mocha_clip_vote", "clip.vote", 0.0, (double)nF * (4 + ip.n_contact), launch_clip_ingest(p, 7, s));
    return 0;
}

int mocha_clip_windows(mocha_ctx* c, const float* pos, const float* vel, const float* rot, const float* ang, const unsigned char* contact,
                       int n_contact, const int32_t* clip_offsets, int n_clips, int window, int step, float* Yrot, float* Ypos, float* Yvel,
                       float* Yang, unsigned char* Ycontact, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (window < 4 || step < 1) return fail(c, MOCHA_ERR_ARG, "clip_windows: window must be at least 4 and step at least 1");
    if (n_contact < 0 || n_contact > MOCHA_MAX_CONTACT) return fail(c, MOCHA_ERR_ARG, "clip_windows: n_contact must be 0..4");
    int rc = clip_offsets_check(c, "clip_windows", clip_offsets, n_clips, 1); if (rc) return rc;
    std::vector<int> tab(clip_offsets, clip_offsets + n_clips + 1);
    int64_t B = 0;
    tab.push_back(0);
    for (int i = 0; i < n_clips; ++i) {
        B += clip_window_count((int64_t)clip_offsets[i + 1] - clip_offsets[i], window, step);
        if (B > 0x7fffffff) return fail(c, MOCHA_ERR_ARG, "clip_windows: more than 2^31 - 1 windows");
        tab.push_back((int)B);
    }
    if (B == 0) return 0;
    if (!pos || !vel || !rot || !ang || !Yrot || !Ypos || !Yvel || !Yang || (n_contact > 0 && (!contact || !Ycontact)))
        return fail(c, MOCHA_ERR_ARG, "clip_windows: null argument");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    int* tab_dev = nullptr; double* ws = nullptr;
    if ((rc = clip_tables(c, s, tab, 0, &tab_dev, &ws))) return rc;
    ClipWindowParams p{};
    p.pos = pos; p.vel = vel; p.rot = rot; p.ang = ang; p.contact = contact; p.offsets = tab_dev; p.wcum = tab_dev + n_clips + 1;
    p.Yrot = Yrot; p.Ypos = Ypos; p.Yvel = Yvel; p.Yang = Yang; p.Ycontact = Ycontact;
    p.C = n_clips; p.J = c->cfg.V + 1; p.nc = n_contact; p.window = window; p.step = step; p.B = B;
    LAUNCH(c, s, "mocha_clip_windows_k", "clip.windows", 0.0, 2.0 * (double)B * window * (p.J * 13.0 * 4 + n_contact),
           launch_clip_windows(p, s));
    return 0;
}

}  // extern "C"

namespace {
// outputs of a clip of n source frames at a step of num / den source frames: floor((n-1) den / num) + 1
int64_t resample_count(int64_t n, int num, int den) { return (n - 1) * den / num + 1; }

bool resample_terms_ok(int num, int den) { return num >= 1 && num <= RESAMPLE_MAX_TERM && den >= 1 && den <= RESAMPLE_MAX_TERM; }

// rot_format 0 quaternions / 1 Euler degrees in euler_order, as mocha_ingest_cfg names them
int resample_format(mocha_ctx* c, const char* who, int rot_format, const int* euler_order, int order[3]) {
    if (rot_format != 0 && rot_format != 1) return fail(c, MOCHA_ERR_ARG, "%s: rot_format must be 0 (quaternions) or 1 (Euler degrees)", who);
    order[0] = 2; order[1] = 1; order[2] = 0;
    if (rot_format == 0) return 0;
    if (!euler_order) return fail(c, MOCHA_ERR_ARG, "%s: null euler_order", who);
    int seen = 0;
    for (int i = 0; i < 3; ++i) {
        if (euler_order[i] < 0 || euler_order[i] > 2) return fail(c, MOCHA_ERR_ARG, "%s: euler_order must name the axes 0..2", who);
        seen |= 1 << euler_order[i];
        order[i] = euler_order[i];
    }
    if (seen != 7) return fail(c, MOCHA_ERR_ARG, "%s: euler_order must be a permutation of 0..2", who);
    return 0;
}
}  // namespace

extern "C" {

int64_t mocha_resample_frames(int64_t n, int num, int den) {
    if (n < 1 || n > 0x7fffffffll || !resample_terms_ok(num, den)) return MOCHA_ERR_ARG;
    return resample_count(n, num, den);
}

int mocha_resample_clips(mocha_ctx* c, int rot_format, const int* euler_order, const float* rot, const float* pos, const int32_t* offsets_in,
                         const int32_t* num, const int32_t* den, int n_clips, const int32_t* offsets_out, float* rot_out, float* pos_out,
                         void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (!rot || !pos || !num || !den || !offsets_out || !rot_out || !pos_out) return fail(c, MOCHA_ERR_ARG, "resample_clips: null argument");
    int order[3];
    int rc = resample_format(c, "resample_clips", rot_format, euler_order, order); if (rc) return rc;
    if ((rc = clip_offsets_check(c, "resample_clips", offsets_in, n_clips, 1))) return rc;
    if (offsets_out[0] != 0) return fail(c, MOCHA_ERR_ARG, "resample_clips: offsets_out[0] must be 0");
    for (int i = 0; i < n_clips; ++i) {
        if (!resample_terms_ok(num[i], den[i]))
            return fail(c, MOCHA_ERR_ARG, "resample_clips: clip %d: num and den must be 1..%d", i, RESAMPLE_MAX_TERM);
        const int64_t m = resample_count((int64_t)offsets_in[i + 1] - offsets_in[i], num[i], den[i]);
        if ((int64_t)offsets_out[i] + m > 0x7fffffffll) return fail(c, MOCHA_ERR_ARG, "resample_clips: 2^31 output frames or more");
        if ((int64_t)offsets_out[i + 1] != (int64_t)offsets_out[i] + m)
            return fail(c, MOCHA_ERR_ARG, "resample_clips: offsets_out[%d] must be offsets_out[%d] + %lld (mocha_resample_frames)", i + 1, i,
                        (long long)m);
    }
    const int V = c->cfg.V, F = offsets_in[n_clips];
    if (V + 1 > MOCHA_MAX_BONES) return fail(c, MOCHA_ERR_ARG, "resample_clips: at most %d joints", MOCHA_MAX_BONES - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    std::vector<int> tab(offsets_in, offsets_in + n_clips + 1);
    tab.insert(tab.end(), offsets_out, offsets_out + n_clips + 1);
    tab.insert(tab.end(), num, num + n_clips);
    tab.insert(tab.end(), den, den + n_clips);
    const size_t nF = (size_t)F, nq = nF * V * 4, np_ = nF * V * 3;
    int* tab_dev = nullptr; double* ws = nullptr;
    if ((rc = clip_tables(c, s, tab, 2 * nq + np_, &tab_dev, &ws))) return rc;
    ClipParams p{};                                            // launches 0 and 1 of the clip ingester, positions unscaled
    p.rot = rot; p.pos = pos; p.offsets = tab_dev; p.qraw = ws; p.q = ws + nq; p.p = ws + 2 * nq;
    p.F = F; p.C = n_clips; p.V = V; p.euler = rot_format; p.scale = 1.0;
    for (int i = 0; i < 3; ++i) p.order[i] = order[i];
    ClipResampleParams r{};
    r.q = p.q; r.p = p.p; r.in_off = tab_dev; r.out_off = tab_dev + n_clips + 1; r.num = r.out_off + n_clips + 1; r.den = r.num + n_clips;
    r.rot_out = rot_out; r.pos_out = pos_out; r.C = n_clips; r.V = V; r.F_out = offsets_out[n_clips];
    const double fq = (double)nq * 8, fp = (double)np_ * 8, fin = (double)nF * V * (rot_format ? 6 : 7) * 4;
    LAUNCH(c, s, "mocha_clip_quat", "resample.quat", 0.0, fin + fq + fp, launch_clip_ingest(p, 0, s));
    LAUNCH(c, s, "mocha_clip_unroll", "resample.unroll", 0.0, 2 * fq, launch_clip_ingest(p, 1, s));
    // bytes: an output on a source frame reads that frame, any other its two neighbours, no frame more than once from memory (56 bytes
    // per joint: quaternion and position in float64); 28 bytes per output joint written
    double touched = 0.0;
    for (int i = 0; i < n_clips; ++i) {
        const int64_t n = (int64_t)offsets_in[i + 1] - offsets_in[i], m = (int64_t)offsets_out[i + 1] - offsets_out[i];
        const int64_t on_frame = (m - 1) / den[i] + 1;       // k num / den is whole for every den-th output (num / den reduced)
        touched += (double)std::min(n, on_frame + 2 * (m - on_frame));
    }
    LAUNCH(c, s, "mocha_clip_resample", "resample.clips", 0.0, (touched * 56.0 + (double)r.F_out * 28.0) * V, launch_clip_resample(r, s));
    return 0;
}

int64_t mocha_resample_state_bytes(const mocha_ctx* c, int streams) {
    if (!c || streams < 1 || streams > 16) return MOCHA_ERR_ARG;
    return (int64_t)streams * RESAMPLE_STATE_DOUBLES * (int64_t)sizeof(double);
}

int mocha_resample_reset(mocha_ctx* c, void* state, int streams, const int32_t* which, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (streams < 1 || streams > 16) return fail(c, MOCHA_ERR_ARG, "resample_reset: 1 <= streams <= 16");
    if (!state) return fail(c, MOCHA_ERR_ARG, "resample_reset: null argument");
    if (which && (n < 0 || n > streams)) return fail(c, MOCHA_ERR_ARG, "resample_reset: n must be 0..streams");
    for (int i = 0; which && i < n; ++i)
        if (which[i] < 0 || which[i] >= streams)
            return fail(c, MOCHA_ERR_ARG, "resample_reset: stream %d out of range 0..%d", (int)which[i], streams - 1);
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(state);
    const size_t row = RESAMPLE_STATE_DOUBLES * sizeof(double);
    if (!which) { HIPCHK(c, hipMemsetAsync(base, 0, row * streams, s)); return 0; }
    for (int i = 0; i < n; ++i) HIPCHK(c, hipMemsetAsync(base + row * which[i], 0, row, s));
    return 0;
}

int mocha_resample_step(mocha_ctx* c, int rot_format, const int* euler_order, void* state, int streams, const float* rot, const float* pos,
                        int num, int den, int64_t push_index, float* rot_out, float* pos_out, int32_t* n_out, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (streams < 1 || streams > 16) return fail(c, MOCHA_ERR_ARG, "resample_step: 1 <= streams <= 16");
    if (!state || !rot || !pos || !rot_out || !pos_out || !n_out) return fail(c, MOCHA_ERR_ARG, "resample_step: null argument");
    ResampleStepParams p{};
    int rc = resample_format(c, "resample_step", rot_format, euler_order, p.order); if (rc) return rc;
    if (!resample_terms_ok(num, den)) return fail(c, MOCHA_ERR_ARG, "resample_step: num and den must be 1..%d", RESAMPLE_MAX_TERM);
    if (den > RESAMPLE_MAX_OUT * num)
        return fail(c, MOCHA_ERR_ARG, "resample_step: more than %d outputs per source frame (den / num = %d / %d)", RESAMPLE_MAX_OUT, den, num);
    if (push_index < 0 || push_index > ((int64_t)1 << 48)) return fail(c, MOCHA_ERR_ARG, "resample_step: push_index must be 0..2^48");
    if (c->cfg.V + 1 > MOCHA_MAX_BONES) return fail(c, MOCHA_ERR_ARG, "resample_step: at most %d joints", MOCHA_MAX_BONES - 1);
    // push j brings source frame j: the outputs k with floor((j-1) den / num) < k <= floor(j den / num) - integers alone, so the host knows
    // the count without asking the device
    const int64_t last = push_index * den / num, first = push_index == 0 ? 0 : (push_index - 1) * den / num + 1;
    p.state = static_cast<double*>(state); p.rot = rot; p.pos = pos; p.rot_out = rot_out; p.pos_out = pos_out;
    p.V = c->cfg.V; p.euler = rot_format; p.num = num; p.den = den; p.count = (int)(last - first + 1); p.k_first = first;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const double V = p.V;
    LAUNCH(c, s, "mocha_resample_step_k", "resample.step", 0.0,
           (double)streams * (V * (rot_format ? 6 : 7) * 4 + 2 * V * RESAMPLE_JOINT_DOUBLES * 8 + p.count * V * 28.0), launch_resample_step(p, streams, s));
    *n_out = p.count;
    return 0;
}

// ------------------------------------------------------------------------------------------- world-space poses, skinning palettes
// anc[b] of the (V+1)-bone skeleton (parents = [-1] + (joint parents + 1), test_fullframework.py:101-102: what post_params gives
// mocha_postprocess): bit a set for b and each of its ancestors
static int world_ancestors(mocha_ctx* c, const char* who, unsigned* anc) {
    const int J = c->cfg.V + 1;
    if (J > MOCHA_MAX_BONES) return fail(c, MOCHA_ERR_ARG, "%s: at most %d joints", who, MOCHA_MAX_BONES - 1);
    anc[0] = 1u;
    for (int b = 1; b < J; ++b) {
        const int pa = c->sk.parents[b - 1] + 1;
        if (pa < 0 || pa >= b) return fail(c, MOCHA_ERR_STATE, "%s: bone %d has parent %d: parents must precede their children", who, b, pa);
        anc[b] = anc[pa] | (1u << b);
    }
    return 0;
}

int64_t mocha_world_bind_bytes(const mocha_ctx* c) {
    if (!c || c->cfg.V + 1 > MOCHA_MAX_BONES) return MOCHA_ERR_ARG;
    return (int64_t)WORLD_BIND_DOUBLES(c->cfg.V) * (int64_t)sizeof(double);
}

int mocha_world_bind(mocha_ctx* c, const double* rest_rot, const double* rest_pos, const double* pre, void* bind, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (!rest_pos || !bind) return fail(c, MOCHA_ERR_ARG, "world_bind: null argument");
    if (reinterpret_cast<uintptr_t>(bind) % 8) return fail(c, MOCHA_ERR_ARG, "world_bind: bind must be 8-byte aligned");
    WorldBindParams p{};
    static const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) {
        p.pre[k] = pre ? pre[k] : eye[k];
        if (!std::isfinite(p.pre[k])) return fail(c, MOCHA_ERR_ARG, "world_bind: pre[%d] is not finite", k);
    }
    int rc = world_ancestors(c, "world_bind", p.anc); if (rc) return rc;
    p.rest_rot = rest_rot; p.rest_pos = rest_pos; p.bind = static_cast<double*>(bind); p.V = c->cfg.V;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_world_bind_k", "world.bind", 0.0, (p.V + 1) * (rest_rot ? 56.0 : 24.0) + WORLD_BIND_DOUBLES(p.V) * 8.0, launch_world_bind(p, s));
    return 0;
}

int mocha_world_pose(mocha_ctx* c, const void* rot, const void* pos, int in_f32, int64_t n, const int32_t* valid, const void* bind, double* gpos,
                     double* grot, float* palette, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (n == 0) return 0;
    if (n < 0 || (in_f32 != 0 && in_f32 != 1)) return fail(c, MOCHA_ERR_ARG, "world_pose: n must be >= 0 and in_f32 0 or 1");
    if (!rot || !pos) return fail(c, MOCHA_ERR_ARG, "world_pose: null argument");
    if (!gpos && !grot && !palette) return fail(c, MOCHA_ERR_ARG, "world_pose: no output asked for");
    if (palette && !bind) return fail(c, MOCHA_ERR_ARG, "world_pose: a palette needs a bind (mocha_world_bind)");
    if (reinterpret_cast<uintptr_t>(rot) % 16 || reinterpret_cast<uintptr_t>(grot) % 16 || reinterpret_cast<uintptr_t>(palette) % 16 ||
        reinterpret_cast<uintptr_t>(pos) % (in_f32 ? 4 : 8) || reinterpret_cast<uintptr_t>(gpos) % 8 || reinterpret_cast<uintptr_t>(bind) % 8)
        return fail(c, MOCHA_ERR_ARG, "world_pose: rot, grot and palette must be 16-byte aligned, the other arrays to their element");
    if (n > (int64_t)0x7fffffff * WORLD_FPB) return fail(c, MOCHA_ERR_ARG, "world_pose: at most %lld frames a call", (long long)0x7fffffff * WORLD_FPB);
    WorldPoseParams p{};
    int rc = world_ancestors(c, "world_pose", p.anc); if (rc) return rc;
    p.rot = rot; p.pos = pos; p.valid = valid; p.bind = palette ? static_cast<const double*>(bind) : nullptr;
    p.gpos = gpos; p.grot = grot; p.palette = palette; p.n = n; p.V = c->cfg.V; p.in_f32 = in_f32;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const double J = p.V + 1;
    LAUNCH(c, s, "mocha_world_pose_k", "world.pose", 0.0,
           (double)n * (J * 7 * (in_f32 ? 4.0 : 8.0) + (valid ? 4.0 : 0.0) + (gpos ? J * 24 : 0.0) + (grot ? J * 32 : 0.0) + (palette ? p.V * 48.0 : 0.0)) +
               (palette ? (double)((n + WORLD_FPB - 1) / WORLD_FPB) * WORLD_BIND_DOUBLES(p.V) * 8.0 : 0.0),      // every workgroup reads the bind
           launch_world_pose(p, s));
    return 0;
}

int mocha_bvh_motion(mocha_ctx* c, const char* text_dev, int64_t nbytes, const char* text_host, const int64_t* clip_text_begin,
                     const int64_t* clip_text_end, const int32_t* clip_offsets, int n_clips, int n_joints, int channels,
                     const int32_t* joint_map, int v_out, const float* offsets_out, float* rot, float* pos, mocha_bvh_report* report,
                     void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (report) *report = mocha_bvh_report{0, 0, -1};
    if (!text_dev || !clip_text_begin || !clip_text_end || !rot || !pos) return fail(c, MOCHA_ERR_ARG, "bvh_motion: null argument");
    if (n_joints < 1 || n_joints > MOCHA_BVH_MAX_JOINTS) return fail(c, MOCHA_ERR_ARG, "bvh_motion: n_joints must be 1..%d", MOCHA_BVH_MAX_JOINTS);
    if (channels != 3 && channels != 6) return fail(c, MOCHA_ERR_ARG, "bvh_motion: channels must be 3 or 6");
    int rc = clip_offsets_check(c, "bvh_motion", clip_offsets, n_clips, 1); if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(text_dev) % 16) return fail(c, MOCHA_ERR_ARG, "bvh_motion: text_dev must be 16-byte aligned");
    if (nbytes <= 0 || nbytes % MOCHA_BVH_ALIGN || nbytes >= (int64_t)1 << 31)
        return fail(c, MOCHA_ERR_ARG, "bvh_motion: nbytes must be a positive multiple of %d below 2^31", MOCHA_BVH_ALIGN);
    for (int i = 0; i < n_clips; ++i) {
        if (clip_text_begin[i] % MOCHA_BVH_ALIGN || (i == 0 && clip_text_begin[0] != 0))
            return fail(c, MOCHA_ERR_ARG, "bvh_motion: clip %d begins at byte %lld: clip 0 at 0, every clip at a multiple of %d", i,
                        (long long)clip_text_begin[i], MOCHA_BVH_ALIGN);
        const int64_t limit = i + 1 < n_clips ? clip_text_begin[i + 1] : nbytes;
        if (clip_text_end[i] <= clip_text_begin[i] || clip_text_end[i] > limit)
            return fail(c, MOCHA_ERR_ARG, "bvh_motion: the text of clip %d is empty or runs into the next clip", i);
    }
    if (!joint_map) {
        if (v_out != n_joints) return fail(c, MOCHA_ERR_ARG, "bvh_motion: without a joint_map v_out must be n_joints");
    } else {
        if (v_out < 1 || v_out > n_joints) return fail(c, MOCHA_ERR_ARG, "bvh_motion: v_out must be 1..n_joints");
        std::vector<char> seen(v_out, 0);
        int kept = 0;
        for (int j = 0; j < n_joints; ++j) {
            if (joint_map[j] < -1 || joint_map[j] >= v_out || (joint_map[j] >= 0 && seen[joint_map[j]]++))
                return fail(c, MOCHA_ERR_ARG, "bvh_motion: joint_map[%d] = %d: -1 or an output joint, each once", j, joint_map[j]);
            kept += joint_map[j] >= 0;
        }
        if (kept != v_out) return fail(c, MOCHA_ERR_ARG, "bvh_motion: joint_map leaves an output joint unwritten");
    }
    if (channels == 3 && !offsets_out) return fail(c, MOCHA_ERR_ARG, "bvh_motion: channels == 3 needs offsets_out");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;

    // the buffer, in 8-byte words: report | clip begins | clip ends | frame offsets | joint map | offsets_out  (uploaded)  | slow list |
    // block counts | prefix
    typedef unsigned long long W;
    const size_t nC = (size_t)n_clips, nblocks = (size_t)(nbytes / BVH_BLOCK);
    const size_t w_begin = 2, w_end = w_begin + nC, w_off = w_end + nC, w_map = w_off + (nC + 2) / 2, w_out = w_map + ((size_t)n_joints + 1) / 2,
                 w_slow = w_out + ((size_t)v_out * 3 + 1) / 2, w_counts = w_slow + (size_t)BVH_MAX_SLOW * 2, w_prefix = w_counts + (nblocks + 1) / 2,
                 words = w_prefix + (nblocks + 2) / 2;
    std::vector<W> tab(w_slow, 0);
    BvhReport fresh{~0ull, 0u, 0u};
    memcpy(&tab[0], &fresh, sizeof fresh);
    for (size_t i = 0; i < nC; ++i) { tab[w_begin + i] = (W)clip_text_begin[i]; tab[w_end + i] = (W)clip_text_end[i]; }
    memcpy(&tab[w_off], clip_offsets, (nC + 1) * sizeof(int32_t));
    int32_t* map_host = reinterpret_cast<int32_t*>(&tab[w_map]);
    for (int j = 0; j < n_joints; ++j) map_host[j] = joint_map ? joint_map[j] : j;
    if (offsets_out) memcpy(&tab[w_out], offsets_out, (size_t)v_out * 3 * sizeof(float));
    if ((rc = reserve(c, c->bvh_ws, words))) return rc;
    W* ws = c->bvh_ws.p;
    HIPCHK(c, hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(W), hipMemcpyHostToDevice, s));

    BvhParams p{};
    p.text = reinterpret_cast<const unsigned char*>(text_dev); p.nbytes = nbytes; p.nblocks = (unsigned)nblocks;
    p.report = reinterpret_cast<BvhReport*>(ws);
    p.begin = reinterpret_cast<const long long*>(ws + w_begin); p.end = reinterpret_cast<const long long*>(ws + w_end);
    p.offsets = reinterpret_cast<const int*>(ws + w_off); p.map = reinterpret_cast<const int*>(ws + w_map);
    p.off_out = offsets_out ? reinterpret_cast<const float*>(ws + w_out) : nullptr;
    p.slow = reinterpret_cast<BvhSlow*>(ws + w_slow);
    p.counts = reinterpret_cast<unsigned*>(ws + w_counts); p.prefix = reinterpret_cast<unsigned*>(ws + w_prefix);
    p.rot = rot; p.pos = pos;
    p.C = n_clips; p.n_joints = n_joints; p.channels = channels; p.v_out = v_out;
    p.per_frame = channels == 3 ? 3 + 3 * n_joints : 6 * n_joints;
    p.root_out = map_host[0];
    p.F = clip_offsets[n_clips];
    const double out_bytes = (double)p.F * v_out * 6 * sizeof(float);
    LAUNCH(c, s, "mocha_bvh_count", "bvh.count", 0.0, (double)nbytes + nblocks * 4.0, launch_bvh_parse(p, 0, s));
    LAUNCH(c, s, "mocha_bvh_scan", "bvh.scan", 0.0, nblocks * 12.0, launch_bvh_parse(p, 1, s));
    LAUNCH(c, s, "mocha_bvh_parse", "bvh.parse", 0.0, (double)nbytes + nblocks * 4.0 + out_bytes, launch_bvh_parse(p, 2, s));
    LAUNCH(c, s, "mocha_bvh_finish", "bvh.finish", 0.0, channels == 3 ? out_bytes / 2 : nC * 24.0, launch_bvh_parse(p, 3, s));
    BvhReport got{};
    HIPCHK(c, hipMemcpyAsync(&got, p.report, sizeof got, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));               // the one wait: the report decides what the call returns (and `tab` may go)
    const int64_t bad = got.first_bad == ~0ull ? -1 : (int64_t)got.first_bad;
    if (report) *report = mocha_bvh_report{(int64_t)got.tokens, (int64_t)got.slow, bad};
    if (bad >= 0) return fail(c, MOCHA_ERR_STATE, "bvh_motion: the text breaks the frame layout or the number grammar at byte %lld", (long long)bad);
    if (got.slow == 0) return 0;
    if (got.slow > (unsigned)BVH_MAX_SLOW)
        return fail(c, MOCHA_ERR_STATE, "bvh_motion: %u tokens need the host's conversion, more than %d", got.slow, BVH_MAX_SLOW);
    if (!text_host) return fail(c, MOCHA_ERR_STATE, "bvh_motion: %u tokens need the host's conversion and there is no text_host", got.slow);
    std::vector<BvhSlow> slow(got.slow);
    HIPCHK(c, hipMemcpyAsync(slow.data(), p.slow, slow.size() * sizeof(BvhSlow), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (BvhSlow& e : slow) {
        char buf[BVH_MAX_TOKEN + 1];
        int len = 0;
        for (int64_t at = (int64_t)e.at; len < BVH_MAX_TOKEN && at + len < nbytes; ++len) {
            const char ch = text_host[at + len];
            if (ch == ' ' || ch == '\t' || ch == '\r' || ch == '\n') break;
            buf[len] = ch;
        }
        buf[len] = 0;
        const float v = (float)strtod(buf, nullptr);      // the device has checked the grammar: strtod reads the whole token
        unsigned bits; memcpy(&bits, &v, sizeof bits);
        e.at = bits;
    }
    HIPCHK(c, hipMemcpyAsync(p.slow, slow.data(), slow.size() * sizeof(BvhSlow), hipMemcpyHostToDevice, s));
    p.n_patch = (int)slow.size();
    LAUNCH(c, s, "mocha_bvh_patch", "bvh.patch", 0.0, slow.size() * 20.0, launch_bvh_parse(p, 4, s));
    HIPCHK(c, hipStreamSynchronize(s));               // `slow` is the copy's source
    return 0;
}

int64_t mocha_bvh_text_bound(int64_t frames, int n_joints, int save_positions) {
    if (frames < 0 || n_joints < 1) return -1;
    const int64_t C = save_positions ? 6 * (int64_t)n_joints : 3 + 3 * (int64_t)n_joints;
    return frames * (C * MOCHA_BVHW_MAX_TOKEN + 1);
}

int mocha_bvh_format(mocha_ctx* c, const double* bvh_pos, const double* bvh_euler, const int32_t* clip_offsets, int n_clips, int n_joints,
                     const int32_t* visit, const int32_t axes[3], int save_positions, char* text_dev, int64_t capacity,
                     int64_t* clip_text_begin, mocha_bvhw_report* report, void* stream) {
    // the arguments are judged before the context is looked at: every refusal below needs neither a context nor a device
    if (report) *report = mocha_bvhw_report{0, 0, -1};
    if (!bvh_pos || !bvh_euler || !visit || !axes || !text_dev || !clip_text_begin) return fail(c, MOCHA_ERR_ARG, "bvh_format: null argument");
    if (n_joints < 1 || n_joints > MOCHA_BVH_MAX_JOINTS) return fail(c, MOCHA_ERR_ARG, "bvh_format: n_joints must be 1..%d", MOCHA_BVH_MAX_JOINTS);
    {
        char seen[MOCHA_BVH_MAX_JOINTS] = {0};
        for (int i = 0; i < n_joints; ++i)
            if (visit[i] < 0 || visit[i] >= n_joints || seen[visit[i]]++)
                return fail(c, MOCHA_ERR_ARG, "bvh_format: visit[%d] = %d: visit must be a permutation of the joints", i, visit[i]);
        int axis_seen = 0;
        for (int k = 0; k < 3; ++k) {
            if (axes[k] < 0 || axes[k] > 2 || (axis_seen >> axes[k] & 1)) return fail(c, MOCHA_ERR_ARG, "bvh_format: axes must be a permutation of 0, 1, 2");
            axis_seen |= 1 << axes[k];
        }
    }
    int rc = clip_offsets_check(c, "bvh_format", clip_offsets, n_clips, 1); if (rc) return rc;
    if (capacity < 0) return fail(c, MOCHA_ERR_ARG, "bvh_format: negative capacity");
    const int64_t F = clip_offsets[n_clips], per_frame = save_positions ? 6 * (int64_t)n_joints : 3 + 3 * (int64_t)n_joints;
    if (mocha_bvh_text_bound(F, n_joints, save_positions) >= (int64_t)1 << 31)
        return fail(c, MOCHA_ERR_ARG, "bvh_format: %lld frames of %lld numbers may take 2^31 bytes or more: split the call", (long long)F,
                    (long long)per_frame);
    if (!c) return fail(nullptr, MOCHA_ERR_ARG, "bvh_format: null context");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;

    // the buffer, in 8-byte words: report | clip byte offsets (read back together) | frame offsets | visit  (uploaded)  | block counts | prefix
    typedef unsigned long long W;
    const size_t nC = (size_t)n_clips, T = (size_t)(F * per_frame), nblocks = (T + BVHW_BLOCK - 1) / BVHW_BLOCK;
    const size_t w_begin = 2, w_off = w_begin + nC + 1, w_visit = w_off + (nC + 2) / 2, w_counts = w_visit + ((size_t)n_joints + 1) / 2,
                 w_prefix = w_counts + (nblocks + 1) / 2, words = w_prefix + (nblocks + 2) / 2;
    std::vector<W> tab(w_counts, 0);
    BvhwReport fresh{~0ull, 0ull};
    memcpy(&tab[0], &fresh, sizeof fresh);
    memcpy(&tab[w_off], clip_offsets, (nC + 1) * sizeof(int32_t));
    memcpy(&tab[w_visit], visit, (size_t)n_joints * sizeof(int32_t));
    if ((rc = reserve(c, c->bvhw_ws, words))) return rc;
    W* ws = c->bvhw_ws.p;
    HIPCHK(c, hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(W), hipMemcpyHostToDevice, s));

    BvhwParams p{};
    p.pos = bvh_pos; p.euler = bvh_euler;
    p.report = reinterpret_cast<BvhwReport*>(ws);
    p.clip_begin = reinterpret_cast<long long*>(ws + w_begin);
    p.offsets = reinterpret_cast<const int*>(ws + w_off); p.visit = reinterpret_cast<const int*>(ws + w_visit);
    p.counts = reinterpret_cast<unsigned*>(ws + w_counts); p.prefix = reinterpret_cast<unsigned*>(ws + w_prefix);
    p.text = reinterpret_cast<unsigned char*>(text_dev);
    for (int k = 0; k < 3; ++k) p.ax[k] = axes[k];
    p.V = n_joints; p.C = (int)per_frame; p.save_positions = save_positions ? 1 : 0; p.n_clips = n_clips;
    p.T = (unsigned)T; p.nblocks = (unsigned)nblocks;
    LAUNCH(c, s, "mocha_bvhw_count", "bvhw.count", 0.0, T * 8.0 + nblocks * 4.0, launch_bvh_format(p, 0, s));
    LAUNCH(c, s, "mocha_bvhw_scan", "bvhw.scan", 0.0, nblocks * 12.0, launch_bvh_format(p, 1, s));
    std::vector<W> got(w_off);
    HIPCHK(c, hipMemcpyAsync(got.data(), ws, got.size() * sizeof(W), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));               // the one wait: the totals decide what the call returns (and `tab` may go)
    const int64_t bad = got[0] == ~0ull ? -1 : (int64_t)got[0], bytes = (int64_t)got[1];
    if (report) *report = mocha_bvhw_report{(int64_t)T, bytes, bad};
    if (bad >= 0)
        return fail(c, MOCHA_ERR_STATE, "bvh_format: token %lld (frame %lld, column %lld) is NaN, infinite or at least 1e12 in magnitude", (long long)bad,
                    (long long)(bad / per_frame), (long long)(bad % per_frame));
    for (size_t i = 0; i <= nC; ++i) clip_text_begin[i] = (int64_t)got[w_begin + i];
    if (capacity < bytes) return fail(c, MOCHA_ERR_ARG, "bvh_format: the text takes %lld bytes, capacity is %lld", (long long)bytes, (long long)capacity);
    LAUNCH(c, s, "mocha_bvhw_write", "bvhw.write", 0.0, T * 8.0 + (double)bytes, launch_bvh_format(p, 2, s));
    return 0;
}

}  // extern "C"

namespace {
// The state of the CVAE branch of a live session (caller-owned device memory, layout documented in mocha_hip.h): per stream the counters
// {chain, last id, mode}, the character feature `prev`, and the branch's staging.  Every section starts on a 256-byte boundary.
struct OursLayout {
    size_t counters, prev, cnt, cond, vae, eps, mu, logvar, bytes;
};
OursLayout ours_layout(int S) {
    const size_t n = (size_t)S, T = 90 * 256 * sizeof(float);
    OursLayout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) / 256 * 256; return at; };
    l.counters = take(n * 3 * sizeof(int32_t));
    l.prev = take(n * T);
    l.cnt = take(n * T);
    l.cond = take(n * 2 * T);
    l.vae = take(n * T);
    l.eps = take(n * 256 * sizeof(float));
    l.mu = take(n * 256 * sizeof(float));
    l.logvar = take(n * 256 * sizeof(float));
    l.bytes = off;
    return l;
}
}  // namespace

extern "C" {

int64_t mocha_live_ours_state_bytes(const mocha_ctx* c, int streams) {
    if (!c || streams < 1 || streams > 16) return MOCHA_ERR_ARG;
    return (int64_t)ours_layout(streams).bytes;
}

int mocha_live_ours_reset(mocha_ctx* c, void* live, void* ours, int streams, const int32_t* which, int n, void* stream) {
    if (!c) return MOCHA_ERR_ARG;
    if (!ours) return fail(c, MOCHA_ERR_ARG, "live_ours_reset: null argument");
    int rc = mocha_live_reset(c, live, streams, which, n, stream); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* base = static_cast<char*>(ours) + ours_layout(streams).counters;
    const size_t cb = 3 * sizeof(int32_t);
    if (!which) { HIPCHK(c, hipMemsetAsync(base, 0, cb * streams, s)); return 0; }
    for (int i = 0; i < n; ++i) HIPCHK(c, hipMemsetAsync(base + cb * which[i], 0, cb, s));
    return 0;
}

// The body of mocha_live_step_ours and of mocha_live_step_ours_grouped (cvae_of non-null: the device table of the characters' weight-bank
// slots; the weights and statistics then come from the weight bank and the step has its own captured graph).
static int live_step_ours_impl(mocha_ctx* c, const LiveCall& a, const LiveFrame& f, const LiveOut& o, void* ours, const mocha_ours_cfg* ocfg,
                               int32_t* seeded, bool grouped, const int32_t* cvae_of) {
    if (!c) return MOCHA_ERR_ARG;
    int rc = live_args(c, "live_step_ours", a, f, o); if (rc) return rc;
    if (!seeded) return fail(c, MOCHA_ERR_ARG, "live_step_ours: null argument");
    if (!ours || !ocfg) return fail(c, MOCHA_ERR_ARG, "live_step_ours: null state buffer or configuration");
    if (grouped && !cvae_of) return fail(c, MOCHA_ERR_ARG, "live_step_ours_grouped: null cvae_of");
    if (!grouped && (!ocfg->src_cnt_mean || !ocfg->src_cnt_std || !ocfg->cha_encoded_mean || !ocfg->cha_encoded_std))
        return fail(c, MOCHA_ERR_ARG, "live_step_ours: null statistic");
    if (ocfg->noise < 0 || ocfg->noise > 2) return fail(c, MOCHA_ERR_ARG, "live_step_ours: noise must be 0 (none), 1 (given) or 2 (device)");
    if (ocfg->noise == 1 && !ocfg->eps) return fail(c, MOCHA_ERR_ARG, "live_step_ours: noise 1 needs eps");
    const int S = a.streams;
    // the branch's stages run on all the streams in one piece (the sampler needs the whole batch between the encoder and the decoder), so
    // the workspace must hold them: mocha_live_step walks a smaller workspace chunk by chunk, this step refuses
    if (S > c->max_chunk)
        return fail(c, MOCHA_ERR_ARG, "live_step_ours: %d streams exceed the workspace limit of %d windows (raise it with mocha_reserve)", S, c->max_chunk);
    if (!c->finalized) return fail(c, MOCHA_ERR_STATE, "weights not finalised: call mocha_finalize_weights first");
    if (grouped && !c->cvb.Cw) return fail(c, MOCHA_ERR_STATE, "live_step_ours_grouped: no CVAE weight bank: call mocha_cvae_bank_create first");
    if (!grouped && !c->cvae_ready) return fail(c, MOCHA_ERR_STATE, "live_step_ours: no CVAE on this context: call mocha_cvae_load_weight and mocha_cvae_finalize first");
    if ((rc = live_state(c, "live_step_ours"))) return rc;
    LiveView v;
    if ((rc = live_view(c, a, f, o, v))) return rc;
    if ((rc = cvae_ws(c, S))) return rc;                    // ... and the sampler's workspace: nothing in the captured region allocates

    const OursLayout ol = ours_layout(S);
    char* ob = static_cast<char*>(ours);
    auto of32 = [&](size_t at) { return reinterpret_cast<float*>(ob + at); };
    int32_t* ocnt = reinterpret_cast<int32_t*>(ob + ol.counters);
    float *prev = of32(ol.prev), *cnt_o = of32(ol.cnt), *cond = of32(ol.cond), *vae = of32(ol.vae), *eps_o = of32(ol.eps), *mu = of32(ol.mu),
          *logvar = of32(ol.logvar);
    mocha_ours_cfg oc = *ocfg;
    if (grouped) oc.src_cnt_mean = oc.src_cnt_std = oc.cha_encoded_mean = oc.cha_encoded_std = nullptr;      // ignored: the slot's statistics serve
    const int J = c->cfg.V + 1, V = c->cfg.V;
    const int nseg = c->bank.segments();
    // grouped: the condition kernel leaves every stream's slot in live_slot, the `which` of the sampler's grouped launches
    const OursGroup grp{cvae_of, c->cvb.stored.p, c->cvb.stats.p, c->cvb.Cw, c->cvb.live_slot.p};
    const OursGroup* gp = grouped ? &grp : nullptr;

    // sampler -> literal decoder on `cha` -> to_mot (de-normalised) into the staging: the tail of the step, and of the warm pass
    auto tail = [&](const float* cha, hipStream_t cs) -> int {
        int r = run_decoder(c, WS(c, "enc_s"), cha, S, WS(c, "dec"), cs);
        if (r) return r;
        return run_to_mot(c, WS(c, "dec"), S, v.ystage, cs, true);
    };
    // ring push + featurize -> embed, encoder, cnt and the z-scored query -> segmented match -> condition (mode per stream, noise) -> CVAE
    // sampler -> state update -> decoder on the streams' character features -> to_mot -> pose heads -> one post-processing frame.  Not
    // the segmented characterize: the launches are not steps of the walk order (IEX), the instance norm also writes cnt into the state,
    // and the sampler sits between the encoder and the decoder
    auto body = [&](hipStream_t cs) -> int {
        LAUNCH(c, cs, "mocha_live_push", "live.push", S * 60.0 * J * 150, S * (60.0 * J * (13 + 15) + J * 26.0) * 4,
               launch_live_push(v.ring, f.Yrot, f.Ypos, f.Yvel, f.Yang, a.seg, c->bone_parents.p, v.xraw, v.eff, o.valid, S, J, cs, nullptr,
                                c->bank.resident ? c->bank.seg_dev.p : nullptr, c->bank.resident ? c->bank.segments() : 0));
        c->lane = 0; c->cur = 0;
        int r;
        if ((r = run_embed(c, v.xraw, S, WS(c, "x5"), true, cs, true))) return r;
        if ((r = run_encoder(c, WS(c, "x5"), S, WS(c, "enc_s"), cs))) return r;
        InormExtra ex = IEX(c);
        if (c->bank.is_bf16) { ex.centre = c->bank.center.p; ex.zc = WS(c, "qc"); }
        LAUNCH(c, cs, "mocha_instnorm", "mvn", 0.0, S * 90.0 * 256 * 4 * (c->bank.is_bf16 ? 4.0 : 3.0),
               launch_instnorm(WS(c, "enc_s"), cnt_o, nullptr, a.cnt_mean, a.cnt_std, WS(c, "qnm"), S, 90, cs, &ex));
        int32_t* gx = SET(c).idx_ws.p;
        if ((r = seg_match(c, WS(c, c->bank.is_bf16 ? "qc" : "qnm"), S, v.eff, o.idx, gx, nullptr, cs))) return r;
        LAUNCH(c, cs, "mocha_live_ours_condition", "ours.condition", 0.0, S * 180.0 * 256 * 8,
               launch_live_ours_condition(ocnt, v.eff, nseg, cnt_o, prev, oc.src_cnt_mean, oc.src_cnt_std, oc.cha_encoded_mean, oc.cha_encoded_std,
                                          cond, oc.noise, oc.eps, oc.seed, eps_o, S, cs, gp));
        if ((r = cvae_sample_impl(c, cond, S, vae, mu, logvar, oc.noise ? eps_o : nullptr, cs, grouped ? grp.slot : nullptr))) return r;
        LAUNCH(c, cs, "mocha_live_ours_update", "ours.update", 0.0, S * 90.0 * 256 * 12,
               launch_live_ours_update(ocnt, v.eff, vae, oc.cha_encoded_mean, oc.cha_encoded_std, c->bank.enc, gx, c->bank.N, prev, seeded, S, cs, gp));
        if ((r = tail(prev, cs))) return r;
        LAUNCH(c, cs, "mocha_pose_heads", "live.heads", 0.0, S * (60.0 * 12 + V * 28.0 * 4), launch_pose_heads(v.ystage, v.heads, v.speed, S, c->cfg.T, V, cs));
        LAUNCH(c, cs, "mocha_post_clip", "live.post", 0.0, (double)S * (V * 13.0 * 4 + J * 11.0 * 8 + 2.0 * POST_STATE_DOUBLES * 8),
               launch_post_step(v.post, cs));
        return 0;
    };
    hipStream_t s = (hipStream_t)a.stream;
    if (c->prof_on) return body(s);

    mocha_ctx::StepKey& key = v.key;
    const void* optrs[7] = {ours, oc.src_cnt_mean, oc.src_cnt_std, oc.cha_encoded_mean, oc.cha_encoded_std, oc.noise == 1 ? oc.eps : nullptr, seeded};
    for (int i = 0; i < 7; ++i) key.ours[i] = optrs[i];
    key.noise = oc.noise; key.seed = oc.noise == 2 ? oc.seed : 0;
    key.cvae_of = cvae_of;
    mocha_ctx::StepGraph& g = c->steps[grouped ? mocha_ctx::STEP_OURS_GROUPED : mocha_ctx::STEP_OURS];
    if (!step_holds(c, g, key)) {
        // Before a capture: one eager pass over staging alone - mocha_live_step's characterize of zeroed windows with every id -1, then the
        // sampler on a zeroed condition and the literal decoder on its sample - so that whatever the kernels of the step make on first
        // use (the plane GEMMs' weight images, the style MLP's float64 weights) exists.  No counter, ring, `prev` or post state moves.
        // (grouped: the grouped sampler with every slot -1 - no weight is read, the sample is zeros.)
        HIPCHK(c, hipMemsetAsync(v.xraw, 0, (size_t)S * 60 * J * c->cfg.C_in * sizeof(float), s));
        HIPCHK(c, hipMemsetAsync(v.eff, 0xFF, (size_t)S * sizeof(int32_t), s));
        HIPCHK(c, hipMemsetAsync(cond, 0, (size_t)S * 180 * 256 * sizeof(float), s));
        SegSelect hard; hard.seg = v.eff;
        if ((rc = characterize_segmented_set0(c, SegWindows{v.xraw, S, a.cnt_mean, a.cnt_std, v.ystage, true}, hard, s))) return rc;
        if ((rc = cvae_sample_impl(c, cond, S, vae, mu, logvar, nullptr, s, grouped ? c->cvb.none.p : nullptr))) return rc;
        if ((rc = tail(vae, s))) return rc;
    }
    return step_replay(c, g, key, s, body);
}

int mocha_live_step_ours(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos, const float* Yvel,
                         const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed, const unsigned char* contact,
                         const int32_t* seg, const float* cnt_mean, const float* cnt_std, void* ours, const mocha_ours_cfg* ocfg, double* pos,
                         double* rot, double* ik_rot, double* bvh_pos, double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* seeded,
                         void* stream) {
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_ours_impl(c, a, f, o, ours, ocfg, seeded, false, nullptr);
}

int mocha_live_step_ours_grouped(mocha_ctx* c, const mocha_post_cfg* cfg, void* live, int streams, const float* Yrot, const float* Ypos,
                                 const float* Yvel, const float* Yang, const float* src_rvel, const float* src_rang, const float* src_speed,
                                 const unsigned char* contact, const int32_t* seg, const float* cnt_mean, const float* cnt_std, void* ours,
                                 const mocha_ours_cfg* ocfg, const int32_t* cvae_of, double* pos, double* rot, double* ik_rot, double* bvh_pos,
                                 double* bvh_euler, int32_t* idx, int32_t* valid, int32_t* seeded, void* stream) {
    LiveCall a; a.cfg = cfg; a.live = live; a.streams = streams; a.seg = seg; a.cnt_mean = cnt_mean; a.cnt_std = cnt_std; a.stream = stream;
    LiveFrame f; f.Yrot = Yrot; f.Ypos = Ypos; f.Yvel = Yvel; f.Yang = Yang; f.src_rvel = src_rvel; f.src_rang = src_rang; f.src_speed = src_speed; f.contact = contact;
    LiveOut o; o.pos = pos; o.rot = rot; o.ik_rot = ik_rot; o.bvh_pos = bvh_pos; o.bvh_euler = bvh_euler; o.idx = idx; o.valid = valid;
    return live_step_ours_impl(c, a, f, o, ours, ocfg, seeded, true, cvae_of);
}

int mocha_column_stats(mocha_ctx* c, const float* x, int64_t N, float* mean, float* std_, void* stream) {
    if (!c || !x || !mean || !std_ || N < 1) return fail(c, MOCHA_ERR_ARG, "bad column_stats arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(c, s, "mocha_column_stats", "bank.stats", 0.0, 8.0 * N * 23040, launch_column_stats(x, N, 90 * 256, mean, std_, s));
    return 0;
}

int mocha_set_option(mocha_ctx* c, const char* name, int value) {
    if (!c || !name) return MOCHA_ERR_ARG;
    const std::string n(name);
    if (n == "dual_stream") {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        c->dual_stream = value != 0;
        c->chunk = 0;                              // workspaces are re-planned (one or two sets) on the next call
        return 0;
    }
    if (n == "lanes") {
        if (value < 1 || value > mocha_ctx::MAX_SETS) return fail(c, MOCHA_ERR_ARG, "lanes must be 1..%d", mocha_ctx::MAX_SETS);
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        c->lanes = value;
        c->chunk = 0;                              // workspace sets are re-planned on the next call (generation moves)
        return 0;
    }
    if (n == "dual_min") {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        c->dual_min = value < 2 ? 2 : value;
        c->chunk = 0;                              // whether set 1 is a full-size set depends on it: re-planned on the next call
        return 0;
    }
    // Path-selecting options change which kernels a step launches: a captured step graph (mocha_step_graph_lane, OursSession)
    // replays the old path until it is re-captured, so every one of them moves the generation.
    if (n == "fold_decoder") { c->fold_decoder = value != 0; c->generation++; return 0; }
    if (n == "upsample_split_min") { c->upsample_split_min = value; c->generation++; return 0; }
    if (n == "fold_upsample") { c->fold_upsample = value != 0; c->generation++; return 0; }
    if (n == "fold_joint") { c->fold_joint = value != 0; c->generation++; return 0; }
    if (n == "match_fold") { c->match_fold = value != 0; c->generation++; return 0; }
    if (n == "scan8") { c->scan8 = value != 0; if (!value) c->bank.b8_valid = false; c->generation++; return 0; }     // the image is built at the next mocha_bank_set
    if (n == "scan16") { c->scan16 = value != 0; c->generation++; return 0; }             // bank side takes effect at the next mocha_bank_set
    if (n == "attention_split_max") { c->attn_split_max = value < 0 ? 0 : value; c->generation++; return 0; }      // this context only
    if (n == "gemm_persistent_max_n") { c->gemm_persistent_max_n = value < 128 ? 128 : value; c->generation++; return 0; }
    if (n == "gemm_x3r_min_n") { c->gemm_x3r_min_n = value < 0 ? 0 : value; c->generation++; return 0; }
    if (n == "gemm_tile64_below") { c->gemm_tile64_below = value < 0 ? 0 : value; c->generation++; return 0; }
    if (n == "gemm_persistent") { c->gemm_persistent = value < 0 ? 0 : (value + 7) / 8 * 8; c->generation++; return 0; }
    if (n == "embed_sums") { c->embed_sums = value != 0; c->generation++; return 0; }
    if (n == "embed_front_max_wgs") { c->embed_max_wgs = value; c->generation++; return 0; }
    if (n == "inorm_split_max") { c->inorm_split_max = value < 0 ? 0 : value; c->generation++; return 0; }
    if (n == "pair_overlap") { c->pair_overlap = value != 0; c->generation++; return 0; }
    if (n == "walk") { if (value < 0 || value > 2) return fail(c, MOCHA_ERR_ARG, "walk must be 0, 1 or 2"); c->walk = value; c->generation++; return 0; }
    if (n == "adain_closed_form") { c->adain_closed = value != 0; c->generation++; return 0; }
    if (n == "style_f64") { c->style_f64 = value != 0; c->bank.dec_valid = false; c->generation++; return 0; }     // cached bank constants: rebuilt at the next mocha_bank_set
    if (n == "bank_dec_cache") { c->bank_dec_cache = value != 0; if (!value) c->bank.dec_valid = false; c->generation++; return 0; }     // takes effect at the next mocha_bank_set
    if (n == "bank_tiled") { c->use_tiled = value != 0; c->generation++; return 0; }
    if (n == "match_planes") { if (value != 1 && value != 2) return fail(c, MOCHA_ERR_ARG, "match_planes must be 1 or 2"); c->match_planes = value; c->generation++; return 0; }
    if (n == "select2") { c->select2 = value != 0; c->generation++; return 0; }
    if (n == "match_pass") { if (value < 0 || value > 2) return fail(c, MOCHA_ERR_ARG, "match_pass must be 0, 1 or 2"); c->match_pass = value; c->generation++; return 0; }
    if (n == "match_nt") { c->match_nt = value != 0; c->generation++; return 0; }
    if (n == "match_pass_variant") { c->match_pass_variant = value & 31; c->generation++; return 0; }      // prefetch depth + non-temporal bit; the fill-only floor kernel (bit 256: no multiplies) is tools/match_pass_probe's, never the library's
    if (n == "match_pass_max_q") { c->match_pass_max_q = value; c->generation++; return 0; }
    if (n == "attention_kv") {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipDeviceSynchronize());
        c->attn_kv = value != 0;
        c->chunk = 0;                              // the key / value image workspace exists only while the option is on: re-planned on the next call
        return 0;
    }
    if (n == "attention_kv_pairs") { c->attn_kv_pairs = value != 0; c->generation++; return 0; }
    if (n == "gemm_bf16x3") { c->gemm_x3 = value != 0; c->generation++; return 0; }
    if (n == "gemm_f16x2") {                        // encoder / decoder / to_mot GEMMs on two fp16 planes, three passes (gemm_h2.hip); the bank's bound: next mocha_bank_set
        HIPCHK(c, hipSetDevice(c->device));
        if (value) { int rc = amax_alloc(c); if (rc) return rc; }
        c->gemm_h2 = value != 0; c->bank.amax_ok = false;
        for (int i = 0; i < mocha_ctx::MAX_SETS; ++i) c->sets[i].amax_enc_of = c->sets[i].amax_dec_of = c->sets[i].amax_tok_of = nullptr;
        c->generation++; return 0;
    }
    if (n == "attention_bf16x3") { c->attn_x3 = value != 0; c->generation++; return 0; }
    return fail(c, MOCHA_ERR_ARG, "unknown option '%s'", name);
}

int mocha_linear(mocha_ctx* c, const float* x, const float* w, const float* bias, float* y, int64_t M, int N, int K, int engine,
                 void* stream) {
    if (!c || !x || !w || !y) return fail(c, MOCHA_ERR_ARG, "null argument");
    if (M < 0 || N < 1 || K < 32 || K % 32 != 0 || M > (1ll << 30) || engine < 0 || engine > 3)
        return fail(c, MOCHA_ERR_ARG, "mocha_linear: M=%lld N=%d K=%d engine=%d (K %% 32 == 0, engine 0..3)", (long long)M, N, K, engine);
    if (M == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    GemmParams p = plain(x, K, w, y, N, (int)M, N, K);
    p.bias = bias;
    if (engine == 3) {                              // two fp16 planes, three passes: the activation bound is measured here (mocha_absmax)
        p.rows_per_win = 1024;
        if (!gemm_h2_supports(p)) return fail(c, MOCHA_ERR_ARG, "mocha_linear: M=%lld N=%d K=%d is outside the f16x2 engine", (long long)M, N, K);
        DeviceBuffer<unsigned short> img; DeviceBuffer<float> auxb;       // aux: [N] inverse weight scales, then the activation bounds of the "windows" (blocks of 1 024 rows here)
        HIPCHK(c, img.reserve(gemm_h2_packed_elems(N, K)));
        const size_t n4 = ((size_t)N + 3) / 4 * 4;
        const int rpw = 1024; const long long nwin = (M + rpw - 1) / rpw;
        hipError_t e = auxb.reserve(n4 + (size_t)nwin);
        float* aux = auxb.p;
        if (e == hipSuccess) e = hipMemsetAsync(aux + n4, 0, (size_t)nwin * sizeof(float), s);
        if (e == hipSuccess) e = launch_pack_h2(w, N, K, img.p, aux, s);
        for (long long w0 = 0; w0 < nwin && e == hipSuccess; w0 += 65535) {
            const long long nw = std::min<long long>(65535, nwin - w0);
            // the last block may be short: measured on its own
            const long long full = (w0 + nw == nwin && M % rpw) ? nw - 1 : nw;
            if (full > 0) e = launch_absmax(x + (size_t)w0 * rpw * K, full, (long long)rpw * K, aux + n4 + w0, s);
            if (e == hipSuccess && full < nw) e = launch_absmax(x + (size_t)(w0 + full) * rpw * K, 1, (long long)(M % rpw) * K, aux + n4 + w0 + full, s);
        }
        p.Wh2 = img.p; p.w_inv = aux; p.a_amax = aux + n4; p.rows_per_win = rpw;
        if (e == hipSuccess) e = launch_gemm_h2(p, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(c, MOCHA_ERR_HIP, "mocha_linear: %s", hipGetErrorString(e));
        return 0;
    }
    const bool x3 = engine == 2 || (engine == 0 && c->gemm_x3 && gemm_x3_supports(p));
    if (!x3) {
        const double flops = 2.0 * M * (double)N * K;
        LAUNCH(c, s, gemm_kernel_name(p), "linear", flops, 4.0 * ((double)M * K + (double)N * K + (double)M * N), launch_gemm(p, s));
        return 0;
    }
    if (!gemm_x3_supports(p)) return fail(c, MOCHA_ERR_ARG, "mocha_linear: M=%lld N=%d K=%d is outside the bf16x3 engine", (long long)M, N, K);
    DeviceBuffer<unsigned short> img;
    HIPCHK(c, img.reserve(gemm_x3_packed_elems(N, K)));
    hipError_t e = launch_pack_x3(w, N, K, img.p, s);
    p.Wsplit = img.p; p.persistent = c->gemm_persistent; p.persistent_max_n = c->gemm_persistent_max_n;
    if (e == hipSuccess) e = (c->gemm_x3r_min_n > 0 && N >= c->gemm_x3r_min_n && gemm_x3r_supports(p)) ? launch_gemm_x3r(p, s) : launch_gemm_x3(p, s);      // option "gemm_x3r_min_n": same bits
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(c, MOCHA_ERR_HIP, "mocha_linear: %s", hipGetErrorString(e));
    return 0;
}

int mocha_linear_grouped(mocha_ctx* c, const float* x, const float* w_bank, const float* bias_bank, const int32_t* which, const int32_t* stored,
                         float* y, int ldc, int G, int m, int N, int K, int Cw, int act, const float* residual, int ldr, void* stream) {
    if (!c || !x || !w_bank || !which || !stored || !y) return fail(c, MOCHA_ERR_ARG, "mocha_linear_grouped: null argument");
    if (G < 0 || m < 1 || N < 16 || K < 16 || N % 16 != 0 || K % 16 != 0 || Cw < 1 || (act != 0 && act != 3) || ldc < N || ldc % 4 != 0 ||
        (residual && (ldr < N || ldr % 4 != 0)) || (long long)G * m > (1ll << 30))
        return fail(c, MOCHA_ERR_ARG, "mocha_linear_grouped: G=%d m=%d N=%d K=%d Cw=%d act=%d ldc=%d ldr=%d (m >= 1, N %% 16 == 0, K %% 16 == 0, act 0 or 3, "
                    "ldc / ldr >= N and multiples of 4)", G, m, N, K, Cw, act, ldc, ldr);
    if (G == 0) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    GroupedGemmParams p;
    p.A = x; p.W = w_bank; p.bias = bias_bank; p.which = which; p.stored = stored; p.C = y; p.residual = residual;
    p.G = G; p.m = m; p.N = N; p.K = K; p.Cw = Cw; p.lda = K; p.ldc = ldc; p.ldr = residual ? ldr : 0;
    p.w_stride = (long long)N * K; p.b_stride = N; p.act = act;
    const double M = (double)G * m;
    LAUNCH(c, s, "mocha_gemm_grouped", "linear_grouped", 2.0 * M * N * K, 4.0 * (M * K + (double)G * ((m + 15) / 16) * N * K + M * N * (residual ? 2 : 1)),
           launch_gemm_grouped(p, s));
    return 0;
}

int mocha_scan_byte_state(mocha_ctx* c, int set, int32_t* state, void* stream) {
    if (!c || !state || set < 0 || set >= mocha_ctx::MAX_SETS) return fail(c, MOCHA_ERR_ARG, "mocha_scan_byte_state: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    state[0] = c->scan8 && c->bank.b8_valid ? 1 : 0;
    state[1] = -1;
    if (c->sets[set].scan_keys.p) {
        unsigned w[2] = {0, 0};
        (void)stream;
        HIPCHK(c, hipDeviceSynchronize());                     // introspection: whatever stream the calls ran on
        HIPCHK(c, hipMemcpy(w, c->sets[set].scan_keys.p + match_scan8_mode_word(), sizeof(w), hipMemcpyDeviceToHost));
        state[1] = (int32_t)w[1];
    }
    return 0;
}

int mocha_bank_view(mocha_ctx* c, const float** cnt_nm, const float** encoded, const float** centroid, const float** row_norm2,
                    const void** cnt_bf16, int64_t* N) {
    if (!c) return MOCHA_ERR_ARG;
    if (int rc = refuse_resident(c, "mocha_bank_view")) return rc;
    if (!c->bank.cnt || c->bank.N <= 0) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set first");
    if (cnt_nm) *cnt_nm = c->bank.cnt;
    if (encoded) *encoded = c->bank.enc;
    if (centroid) *centroid = c->bank.center.p;
    if (row_norm2) *row_norm2 = c->bank.norm.p;
    if (cnt_bf16) *cnt_bf16 = c->bank.is_bf16 ? c->bank.bf16.p : nullptr;
    if (N) *N = c->bank.N;
    return 0;
}

int mocha_bank_export(mocha_ctx* c, float* cnt_nm, float* encoded, void* stream) {
    int rc = ready(c, 0); if (rc) return rc;
    if ((rc = refuse_resident(c, "mocha_bank_export"))) return rc;
    if (!c->bank.cnt || !c->bank.enc || c->bank.N <= 0) return fail(c, MOCHA_ERR_STATE, "no bank: call mocha_bank_set or mocha_bank_broadcast first");
    const size_t bytes = (size_t)c->bank.N * 90 * 256 * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (cnt_nm) HIPCHK(c, hipMemcpyAsync(cnt_nm, c->bank.cnt, bytes, hipMemcpyDeviceToDevice, s));
    if (encoded) HIPCHK(c, hipMemcpyAsync(encoded, c->bank.enc, bytes, hipMemcpyDeviceToDevice, s));
    return 0;
}

int mocha_profile_start(mocha_ctx* c) {
    if (!c) return MOCHA_ERR_ARG;
    for (auto& r : c->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    c->prof.clear();
    c->prof_on = true;
    return 0;
}

int mocha_profile_stop(mocha_ctx* c, char* json, int64_t cap) {
    if (!c || !json || cap < 64) return fail(c, MOCHA_ERR_ARG, "bad profile buffer");
    c->prof_on = false;
    HIPCHK(c, hipSetDevice(c->device));
    struct Agg { long n = 0; double ms = 0, flops = 0, bytes = 0; };
    std::map<std::string, Agg> byk, bys;
    for (auto& r : c->prof) {
        HIPCHK(c, hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, r.e0, r.e1));
        for (auto* m : {&byk, &bys}) {
            Agg& a = (*m)[m == &byk ? r.kernel : r.site + "|" + r.kernel];
            a.n++; a.ms += ms; a.flops += r.flops; a.bytes += r.bytes;
        }
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    c->prof.clear();
    std::string o = "{";
    for (int pass = 0; pass < 2; ++pass) {
        o += pass ? ",\"sites\":{" : "\"kernels\":{";
        bool first = true;
        for (auto& kv : (pass ? bys : byk)) {
            char buf[384];
            snprintf(buf, sizeof buf, "%s\"%s\":{\"launches\":%ld,\"ms\":%.6f,\"flops\":%.6e,\"bytes\":%.6e}", first ? "" : ",",
                     kv.first.c_str(), kv.second.n, kv.second.ms, kv.second.flops, kv.second.bytes);
            o += buf; first = false;
        }
        o += "}";
    }
    o += "}";
    if ((int64_t)o.size() + 1 > cap) return fail(c, MOCHA_ERR_ARG, "profile buffer too small (%zu needed)", o.size() + 1);
    memcpy(json, o.c_str(), o.size() + 1);
    return 0;
}

}  // extern "C"
