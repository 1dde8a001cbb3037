// Driver of tests/test_extent_alloc.py: replays a file of operations on ExtentAlloc (csrc/extent_alloc.h) and prints every answer.  Its own
// main, host only: the test compiles it with g++ under the address and undefined-behaviour sanitizers.
//   line "u N"        reset to N units            -> "u"
//   line "t N"        take(N)                     -> "t <first or -1> <free units> <largest>"
//   line "r FIRST N"  release(FIRST, N)           -> "r <1 accepted / 0 refused> <free units> <largest>"
#include <cinttypes>
#include <cstdio>

#include "../mocha_sigasia2023_amd/csrc/extent_alloc.h"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s OPS\n", argv[0]); return 2; }
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    mocha::ExtentAlloc a;
    char op;
    long long x = 0, y = 0, done = 0;
    while (std::fscanf(f, " %c", &op) == 1) {
        if (op == 'u' && std::fscanf(f, "%lld", &x) == 1) {
            a.reset(x);
            std::printf("u\n");
        } else if (op == 't' && std::fscanf(f, "%lld", &x) == 1) {
            const long long first = a.take(x);
            std::printf("t %lld %lld %lld\n", first, (long long)a.free_units(), (long long)a.largest());
        } else if (op == 'r' && std::fscanf(f, "%lld %lld", &x, &y) == 2) {
            const int ok = a.release(x, y) ? 1 : 0;
            std::printf("r %d %lld %lld\n", ok, (long long)a.free_units(), (long long)a.largest());
        } else {
            std::fprintf(stderr, "bad operation after %lld\n", done);
            std::fclose(f);
            return 2;
        }
        ++done;
    }
    std::fclose(f);
    std::printf("replayed %lld operations\n", done);
    return 0;
}
