// mocha_bvh_header: the HIERARCHY block and the Frames: / Frame Time: lines of a BVH file (motion/bvh.py:36-104), on the host.
// Plain C++17, no HIP header: g++ alone compiles this unit (tests/bvh_header_main.cpp runs it under the address sanitizer).
// The text is NOT NUL-terminated; every read below is of a byte inside [text, text + nbytes).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/mocha_hip.h"

namespace {

struct Tok { int64_t b, e; };      // [b, e) of the text

struct Parser {
    const char* t;
    int64_t n;
    mocha_bvh_hdr* h;
    int64_t line = 0;               // first byte of the line being read

    bool space(char c) const { return c == ' ' || c == '\t' || c == '\r'; }
    bool is(const Tok& k, const char* w) const {
        const int64_t len = (int64_t)strlen(w);
        return k.e - k.b == len && memcmp(t + k.b, w, (size_t)len) == 0;
    }
    int refuse(const char* fmt, ...) {
        va_list ap; va_start(ap, fmt); vsnprintf(h->error, sizeof h->error, fmt, ap); va_end(ap);
        h->error_offset = line;
        return MOCHA_ERR_ARG;
    }
    // the tokens of the line that starts at `at` (at most `cap` are kept, all are counted); returns the first byte of the next line
    int64_t split(int64_t at, Tok* toks, int cap, int* count) const {
        int m = 0;
        int64_t i = at;
        while (i < n && t[i] != '\n') {
            if (space(t[i])) { ++i; continue; }
            const int64_t b = i;
            while (i < n && t[i] != '\n' && !space(t[i])) ++i;
            if (m < cap) toks[m] = Tok{b, i};
            ++m;
        }
        *count = m;
        return i < n ? i + 1 : n;
    }
    // a decimal number that fills the whole token: copied into a terminated buffer first, strtod never sees the text itself
    bool number(const Tok& k, double* v) const {
        char buf[72];
        const int64_t len = k.e - k.b;
        if (len < 1 || len > 64) return false;
        for (int64_t i = 0; i < len; ++i) {
            const char c = t[k.b + i];
            if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return false;
            buf[i] = c;
        }
        buf[len] = 0;
        char* end = nullptr;
        *v = strtod(buf, &end);
        return end == buf + len;
    }
    bool integer(const Tok& k, int64_t* v) const {
        if (k.e - k.b < 1 || k.e - k.b > 10) return false;
        int64_t r = 0;
        for (int64_t i = k.b; i < k.e; ++i) {
            if (t[i] < '0' || t[i] > '9') return false;
            r = r * 10 + (t[i] - '0');
        }
        *v = r;
        return true;
    }
    int axis(const Tok& k, const char* suffix) const {      // Xrotation -> 0 ...; -1 when the token is no such channel
        if (k.e - k.b != 1 + (int64_t)strlen(suffix) || memcmp(t + k.b + 1, suffix, strlen(suffix)) != 0) return -1;
        const char c = t[k.b];
        return c == 'X' ? 0 : c == 'Y' ? 1 : c == 'Z' ? 2 : -1;
    }

    int run() {
        enum { MAXTOK = 12 };
        Tok k[MAXTOK];
        int m = 0, depth = 0, active = -1, pending = 0;      // pending: a ROOT / JOINT / End Site line waits for its '{'
        bool end_site = false, in_end_site = false, have_order = false, seen_motion = false;
        int chan_of[MOCHA_BVH_MAX_JOINTS];
        int64_t at = 0;
        while (at < n && !seen_motion) {
            line = at;
            at = split(at, k, MAXTOK, &m);
            if (m == 0 || is(k[0], "HIERARCHY")) continue;
            const bool root = is(k[0], "ROOT"), joint = is(k[0], "JOINT");
            if (root || joint) {
                if (pending) return refuse("a joint line where '{' belongs");
                if (m != 2) return refuse("%s takes one name", root ? "ROOT" : "JOINT");
                if (root && h->n_joints > 0) return refuse("a second ROOT");
                if (joint && (active < 0 || in_end_site)) return refuse("JOINT outside a joint's block");
                if (h->n_joints >= MOCHA_BVH_MAX_JOINTS) return refuse("more than %d joints", MOCHA_BVH_MAX_JOINTS);
                const int j = h->n_joints++;
                h->parents[j] = active;
                h->name_offset[j] = k[1].b; h->name_length[j] = (int32_t)(k[1].e - k[1].b);
                h->offsets[j][0] = h->offsets[j][1] = h->offsets[j][2] = 0.0;
                chan_of[j] = 0;
                active = j; pending = 1;
            } else if (is(k[0], "End")) {
                if (m != 2 || !is(k[1], "Site")) return refuse("End without Site");
                if (pending || active < 0 || in_end_site) return refuse("End Site outside a joint's block");
                end_site = true; pending = 1;
            } else if (is(k[0], "{")) {
                if (m != 1 || !pending) return refuse("'{' without a joint line before it");
                pending = 0; ++depth;
                if (end_site) { in_end_site = true; end_site = false; }
            } else if (is(k[0], "}")) {
                if (m != 1 || pending || depth == 0) return refuse("unbalanced '}'");
                --depth;
                if (in_end_site) in_end_site = false;      // bvh.py:55-56
                else active = h->parents[active];          // :58
            } else if (is(k[0], "OFFSET")) {
                if (pending || depth == 0) return refuse("OFFSET outside a block");
                double v[3];
                if (m != 4 || !number(k[1], &v[0]) || !number(k[2], &v[1]) || !number(k[3], &v[2])) return refuse("OFFSET takes three numbers");
                if (!in_end_site) for (int a = 0; a < 3; ++a) h->offsets[active][a] = v[a];      // :63-64: End Site offsets are ignored
            } else if (is(k[0], "CHANNELS")) {
                if (pending || depth == 0 || in_end_site) return refuse("CHANNELS outside a joint's block");
                int64_t c = 0;
                if (m < 2 || !integer(k[1], &c)) return refuse("CHANNELS takes a count");
                if (c != 3 && c != 6) return refuse("%d-channel joints are not supported (3 or 6)", (int)c);
                if (m != 2 + (int)c) return refuse("CHANNELS %d with %d names", (int)c, m - 2);
                if (chan_of[active]) return refuse("a second CHANNELS line of one joint");
                if (active == 0 && c != 6) return refuse("the root needs 6 channels");
                if (c == 6)
                    for (int a = 0; a < 3; ++a)
                        if (axis(k[2 + a], "position") != a) return refuse("position channels must be Xposition Yposition Zposition");
                int ord[3];
                for (int a = 0; a < 3; ++a)
                    if ((ord[a] = axis(k[2 + (int)c - 3 + a], "rotation")) < 0) return refuse("a rotation channel expected");
                if (ord[0] == ord[1] || ord[0] == ord[2] || ord[1] == ord[2]) return refuse("a rotation axis twice");
                if (have_order && (ord[0] != h->order[0] || ord[1] != h->order[1] || ord[2] != h->order[2]))
                    return refuse("joints disagree on the rotation order");
                for (int a = 0; a < 3; ++a) h->order[a] = ord[a];
                have_order = true;
                if (active > 0) {
                    if (h->channels && h->channels != (int)c) return refuse("joints disagree on the channel count");
                    h->channels = (int)c;
                }
                chan_of[active] = (int)c;
            } else if (is(k[0], "MOTION")) {
                if (m != 1) return refuse("MOTION stands alone");
                if (pending || depth != 0) return refuse("unbalanced braces at MOTION");
                if (h->n_joints == 0) return refuse("MOTION without a hierarchy");
                seen_motion = true;
            } else {
                return refuse("not a hierarchy line");
            }
        }
        line = n;
        if (!seen_motion) return refuse(depth || pending ? "the text ends inside the hierarchy" : "no MOTION");
        for (int j = 0; j < h->n_joints; ++j) {
            line = h->name_offset[j];
            if (!chan_of[j]) return refuse("a joint without CHANNELS");
        }
        if (!h->channels) h->channels = 6;      // the root alone: its six channels are the frame
        int stage = 0;                          // 0: Frames: expected, 1: Frame Time:, 2: done
        while (at < n && stage < 2) {
            line = at;
            at = split(at, k, MAXTOK, &m);
            if (m == 0) continue;
            if (stage == 0) {
                if (m != 2 || !is(k[0], "Frames:") || !integer(k[1], &h->frames)) return refuse("Frames: <count> expected");
                if (h->frames > 0x7fffffff) return refuse("more than 2^31 - 1 frames");
            } else {
                if (m != 3 || !is(k[0], "Frame") || !is(k[1], "Time:") || !number(k[2], &h->frame_time)) return refuse("Frame Time: <seconds> expected");
            }
            ++stage;
        }
        line = n;
        if (stage < 2) return refuse(stage == 0 ? "no Frames:" : "no Frame Time:");
        h->motion_begin = at; h->motion_end = n;
        return MOCHA_OK;
    }
};

}  // namespace

extern "C" int mocha_bvh_header(const char* text, int64_t nbytes, mocha_bvh_hdr* hdr) {
    if (!hdr) return MOCHA_ERR_ARG;
    memset(hdr, 0, sizeof *hdr);
    hdr->error_offset = -1;
    if (!text || nbytes < 0) {
        snprintf(hdr->error, sizeof hdr->error, "null text");
        hdr->error_offset = 0;
        return MOCHA_ERR_ARG;
    }
    Parser p{text, nbytes, hdr};
    const int rc = p.run();
    if (rc) { hdr->motion_begin = hdr->motion_end = 0; }
    return rc;
}
