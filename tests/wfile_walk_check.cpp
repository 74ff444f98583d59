// wfile_walk_check.cpp -- the walks of csrc/alz_zfile.h (alz_wframe) in a stand-alone program, for a build with -fsanitize=address,undefined.
// usage: wfile_walk_check CORPUS | wfile_walk_check --keystream N.  The corpus is written by tests/test_wfile_cpu.py: u32 count, then per record u32 kind, u32 big, u32 len, the
// file's bytes, i32 rc, u32 n_parts, u32 stated, u32 flags, i32 is_match, n_parts x 4 u32 -- what the library answered for that file.  Every file
// is copied into a heap block of exactly its length, so that a read outside it is the sanitizer's to report; the answers are compared too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alz_zfile.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--keystream")) {                // the first N words of SSZL's keystream, one per line
        alz_wframe::SszlTwister mt;
        for (long k = atol(argv[2]); k > 0; k--) printf("%u\n", mt.next());
        return 0;
    }
    if (argc != 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint32_t count = 0, bad = 0;
    if (!rd(f, &count, 4)) return 2;
    for (uint32_t i = 0; i < count; i++) {
        uint32_t kind, big, len, np, stated, flags; int32_t rc, match;
        if (!rd(f, &kind, 4) || !rd(f, &big, 4) || !rd(f, &len, 4)) return 2;
        uint8_t* src = (uint8_t*)malloc(len ? len : 1);                 // exactly `len` bytes (one for an empty file, never read)
        if (!rd(f, src, len) || !rd(f, &rc, 4) || !rd(f, &np, 4) || !rd(f, &stated, 4) || !rd(f, &flags, 4) || !rd(f, &match, 4)) return 2;
        std::vector<alz_wfile_part> want(np);
        if (!rd(f, want.data(), (size_t)np * sizeof(alz_wfile_part))) return 2;
        alz_container_options opt; memset(&opt, 0, sizeof(opt)); opt.big_endian = big;
        uint32_t n = 0, st = 0, fl = 0, size = 0;
        int got = alz_wframe::walk(kind, &opt, src, len, nullptr, 0, &n, &st, &fl);
        std::vector<alz_wfile_part> parts(n ? n : 1);
        if (got == ALZ_E_INVALID && n) got = alz_wframe::walk(kind, &opt, src, len, parts.data(), n, &n, &st, &fl);
        bool ok = got == rc && n == np && st == stated && fl == flags && alz_wframe::is_match(kind, src, len) == match;
        for (uint32_t k = 0; ok && k < n; k++) {
            ok = !memcmp(&parts[k], &want[k], sizeof(alz_wfile_part)) && (uint64_t)parts[k].src_off + parts[k].src_len <= len;
        }
        (void)alz_wframe::decompressed_size(kind, &opt, src, len, &size);
        if (!ok) { bad++; fprintf(stderr, "record %u (kind %u, %u bytes): walk %d / %u parts, the library said %d / %u\n", i, kind, len, got, n, rc, np); }
        free(src);
    }
    fclose(f);
    printf("%u records, %u differ\n", count, bad);
    return bad ? 1 : 0;
}
