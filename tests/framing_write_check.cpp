// framing_write_check.cpp -- the writers' rules of csrc/alz_framing.h on their own, without the single-file layer, the batch layer or a GPU:
// prints what they produce for fixed inputs, one line each; tests/test_framing_compress_cpu.py holds the lines against the byte-wise Python
// model of tests/framing_cases.py.  Block results, slot bytes and source bytes are made up here by rules the test restates.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alz_framing.h"

using namespace alz_framing;

static void hex(const char* tag, const uint8_t* p, size_t n) { printf("%s ", tag); for (size_t i = 0; i < n; i++) printf("%02x", p[i]); printf("\n"); }

static uint8_t src_byte(size_t i) { return (uint8_t)(i * 7 + 3); }
static uint8_t slot_byte(size_t block, size_t j) { return (uint8_t)(block * 31 + j * 5 + 1); }

// a sink that writes the file and checks that the pieces come in file order without a gap
struct Sink {
    std::vector<uint8_t> out; size_t end = 0; bool gap = false;
    void put(size_t at, size_t k) { if (at != end) gap = true; end = at + k; if (out.size() < end) out.resize(end); }
    void bytes(size_t at, const uint8_t* p, size_t k) { put(at, k); memcpy(out.data() + at, p, k); }
    void slot(size_t at, size_t i, size_t k) { put(at, k); for (size_t j = 0; j < k; j++) out[at + j] = slot_byte(i, j); }
    void source(size_t at, size_t off, size_t k) { put(at, k); for (size_t j = 0; j < k; j++) out[at + j] = src_byte(off + j); }
};

static alz_result res(uint32_t dst_len, int32_t status = ALZ_ST_OK) { alz_result r; memset(&r, 0, sizeof(r)); r.dst_len = dst_len; r.status = status; return r; }

int main() {
    for (uint32_t opt : {0u, 0x10000u, 0x40000u, 0x100000u, 0x400000u, 0x20000u, 1u}) {
        uint32_t block = 0; uint8_t d[7] = {0};
        const uint8_t bd = lz4_frame_bd(opt, &block);
        if (bd) lz4_frame_descriptor(d, bd);
        printf("descriptor %x %x %x ", opt, bd, block); hex("", d, bd ? 7 : 0);
    }
    printf("word %08x %08x %08x %02x\n", lz4_block_word(1234, false), lz4_block_word(0x10000, true), kLz4EndMark, kLz4LegacyEof);
    { uint8_t h[8]; snappy_chunk_header(h, false, 300, 0xE3069283u); hex("chunk", h, 8); snappy_chunk_header(h, true, 0x10000, 0x12345678u); hex("chunk", h, 8); }
    printf("errors %d %d %d %d\n", lz4_block_error(ALZ_ST_OUTPUT_CAPACITY), lz4_block_error(ALZ_ST_BAD_TOKEN), snappy_block_error(ALZ_ST_OUTPUT_CAPACITY), snappy_block_error(ALZ_ST_BAD_TOKEN));
    printf("slot %zu %zu\n", write_slot_bytes(0x10000), write_slot_bytes(0x800000));
    // what is refused before anything is encoded: capacity floors, an unknown block size, a last block of 1 to 4 bytes
    {
        Lz4Writer w;
        printf("open %d %d %d %d %d %d %d %d %d\n", lz4_write_open(false, 0x10000, 100, 15, w), lz4_write_open(false, 0x20000, 100, 15, w), lz4_write_open(false, 0x20000, 100, 16, w),
               lz4_write_open(false, 0x10000, 0x10004, 1 << 20, w), lz4_write_open(false, 0x10000, 0x10005, 1 << 20, w), lz4_write_open(false, 0x40000, 0x10004, 1 << 20, w),
               lz4_write_open(true, 7, 4, 1 << 20, w), snappy_write_open(9), snappy_write_open(10));
    }
    // a frame of 64 KiB blocks over 2 x 65 536 + 100 bytes: the first block does not shrink (stored), the other two do
    const size_t n = 2 * 65536 + 100;
    const alz_result rs[3] = {res(70000), res(500), res(60)};
    {
        Lz4Writer w; size_t len = 0;
        int rc = lz4_write_open(false, 0x10000, n, 1 << 20, w);
        Sink s; rc = rc ? rc : lz4_write_blocks(w, n, rs, 1 << 20, s, &len);
        printf("frame %d %zu %d\n", rc, len, (int)s.gap); hex("frame_bytes", s.out.data(), len);
        Sink t; size_t l2 = 0;
        printf("frame_caps %d %d\n", lz4_write_blocks(w, n, rs, len, t, &l2), lz4_write_blocks(w, n, rs, len - 1, t, &l2));
        const alz_result bad[3] = {res(70000), res(0, ALZ_ST_OUTPUT_CAPACITY), res(60)}, worse[3] = {res(0, ALZ_ST_BAD_TOKEN), res(500), res(60)};
        printf("frame_errors %d %d\n", lz4_write_blocks(w, n, bad, 1 << 20, t, &l2), lz4_write_blocks(w, n, worse, 1 << 20, t, &l2));
    }
    {   // legacy: one block of 8 MiB at most, never stored
        Lz4Writer w; size_t len = 0;
        int rc = lz4_write_open(true, 0, n, 1 << 20, w);
        const alz_result one[1] = {res(777)};
        Sink s; rc = rc ? rc : lz4_write_blocks(w, n, one, 1 << 20, s, &len);
        printf("legacy %d %zu %d %x\n", rc, len, (int)s.gap, w.block); hex("legacy_bytes", s.out.data(), len);
        Sink t; size_t l2 = 0;
        printf("legacy_caps %d %d\n", lz4_write_blocks(w, n, one, len, t, &l2), lz4_write_blocks(w, n, one, len - 1, t, &l2));
    }
    {   // Snappy: the first chunk stored (its output as long as the chunk), the second compressed, the short last one stored at its own length
        const alz_result cr[3] = {res(65536), res(500), res(100)};
        Sink s; size_t len = 0;
        const int rc = snappy_write_chunks(n, cr, 1 << 20, s, [](size_t i) { return 0x01010101u * (uint32_t)(i + 1); }, &len);
        printf("snappy %d %zu %d\n", rc, len, (int)s.gap); hex("snappy_bytes", s.out.data(), len);
        Sink t; size_t l2 = 0;
        printf("snappy_caps %d %d\n", snappy_write_chunks(n, cr, len, t, [](size_t) { return 0u; }, &l2), snappy_write_chunks(n, cr, len - 1, t, [](size_t) { return 0u; }, &l2));
        Sink e; size_t l0 = 0;
        const int rc0 = snappy_write_chunks(0, cr, 10, e, [](size_t) { return 0u; }, &l0);
        printf("snappy_empty %d %zu\n", rc0, l0);
    }
    return 0;
}
