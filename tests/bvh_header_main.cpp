// Stand-alone driver of mocha_bvh_header for the sanitizer run of tests/test_bvh_header.py: compiled together with
// mocha_sigasia2023_amd/csrc/bvh_header.cpp by g++ with -fsanitize=address,undefined.  For every file named on the command line it calls the
// parser on the whole file (which must succeed) and on EVERY byte-length prefix of the file's header region, each prefix copied into a
// heap buffer of exactly that size, so that a read at or past nbytes is a heap-buffer-overflow.  Every call must return MOCHA_OK or
// MOCHA_ERR_ARG.  Prints one line per file; exit status 0 when all is well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/mocha_hip.h"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s file.bvh ...\n", argv[0]); return 2; }
    mocha_bvh_hdr* hdr = static_cast<mocha_bvh_hdr*>(malloc(sizeof(mocha_bvh_hdr)));
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<char> text;
        char chunk[4096];
        for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) text.insert(text.end(), chunk, chunk + n);
        fclose(f);
        char* whole = static_cast<char*>(malloc(text.size()));
        memcpy(whole, text.data(), text.size());
        int rc = mocha_bvh_header(whole, (int64_t)text.size(), hdr);
        free(whole);
        if (rc != MOCHA_OK) { fprintf(stderr, "%s: refused: %s (byte %lld)\n", argv[a], hdr->error, (long long)hdr->error_offset); return 1; }
        const int64_t header_bytes = hdr->motion_begin;
        long ok = 0, refused = 0;
        for (int64_t len = 0; len <= header_bytes; ++len) {
            char* prefix = static_cast<char*>(malloc((size_t)len));      // exactly len bytes: malloc(0) is a valid, unreadable block
            if (len) memcpy(prefix, text.data(), (size_t)len);
            rc = mocha_bvh_header(prefix, len, hdr);
            free(prefix);
            if (rc == MOCHA_OK) {
                if (hdr->motion_begin > len || hdr->motion_end != len) { fprintf(stderr, "%s: prefix %lld: numeric range outside the text\n", argv[a], (long long)len); return 1; }
                ++ok;
            } else if (rc == MOCHA_ERR_ARG) {
                if (hdr->error_offset < 0 || hdr->error_offset > len) { fprintf(stderr, "%s: prefix %lld: error offset outside the text\n", argv[a], (long long)len); return 1; }
                ++refused;
            } else {
                fprintf(stderr, "%s: prefix %lld: status %d\n", argv[a], (long long)len, rc);
                return 1;
            }
        }
        printf("%s: %lld header bytes, %ld prefixes accepted, %ld refused\n", argv[a], (long long)header_bytes, ok, refused);
    }
    free(hdr);
    return 0;
}
