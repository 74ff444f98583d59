// deflate_plan_dump.cpp -- alz_deflate_plan_block (csrc/alz_inflate.h, the source lane 0 of alz_deflate_find_kernel runs) as a filter: what
// the Python twin of tests/deflate_find_ref.py is pinned to.  Reads records from stdin, each
//     final stored_only fixed_only raw_len ntok  <286 literal/length counts>  <30 distance counts>
// (whitespace separated; the literal/length counts hold the end-of-block's 1) and prints one line per record:
//     type bits bytes hdr_bits size1 size2 | <288 literal/length code lengths> | <32 distance code lengths> | <the header's bytes in hex, or ->
// Built by tests/test_deflate_find_cpu.py as tests/test_deflate_cpu.py builds deflate_codes_check.cpp.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "alz_inflate.h"

static alz_deflate_work g_work;

int main() {
    uint32_t lit[ALZ_DEFLATE_NLIT + 2], dist[ALZ_DEFLATE_NDIST + 2];
    unsigned final, stored_only, fixed_only, raw_len, ntok;
    int records = 0;
    while (scanf("%u %u %u %u %u", &final, &stored_only, &fixed_only, &raw_len, &ntok) == 5) {
        memset(lit, 0, sizeof(lit)); memset(dist, 0, sizeof(dist));
        for (uint32_t i = 0; i < ALZ_DEFLATE_NLIT; i++) if (scanf("%u", &lit[i]) != 1) { fprintf(stderr, "record %d: short literal/length counts\n", records); return 1; }
        for (uint32_t i = 0; i < ALZ_DEFLATE_NDIST; i++) if (scanf("%u", &dist[i]) != 1) { fprintf(stderr, "record %d: short distance counts\n", records); return 1; }
        alz_deflate_plan p; memset(&p, 0, sizeof(p));          // (`p` is zeroed by the caller)
        uint32_t size[3];
        alz_deflate_plan_block(lit, dist, raw_len, ntok, final != 0, stored_only != 0, fixed_only != 0, &g_work, &p, size);
        printf("%u %u %u %u %u %u |", p.type, p.bits, p.bytes, p.hdr_bits, size[1], size[2]);
        for (uint32_t i = 0; i < 288; i++) printf(" %u", p.lit_len[i]);
        printf(" |");
        for (uint32_t i = 0; i < 32; i++) printf(" %u", p.dist_len[i]);
        printf(" | ");
        const uint32_t nb = (p.hdr_bits + 7u) / 8u;
        if (!nb) printf("-");
        for (uint32_t i = 0; i < nb; i++) printf("%02x", p.hdr[i]);
        for (uint32_t i = nb; i < ALZ_DEFLATE_HDR_BYTES; i++) if (p.hdr[i]) { fprintf(stderr, "record %d: a byte behind the header is set\n", records); return 1; }
        printf("\n");
        records++;
    }
    if (!feof(stdin)) { fprintf(stderr, "record %d: not a number\n", records); return 1; }
    return 0;
}
