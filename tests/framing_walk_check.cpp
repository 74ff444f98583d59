// framing_walk_check -- the LZ4 / Snappy framing readers of csrc/alz_framing.h on untrusted bytes, stand-alone (built with AddressSanitizer +
// UndefinedBehaviorSanitizer by `make -C oracle framing_walk_check`; tests/test_framing_walk_cpu.py).  stdin: one input per line,
// "<lz4|legacy|snappy> <hex>".  Each input is copied into a heap buffer of exactly its size and read to the end the way alz_container_measure
// collects a file: frame after frame with chained magics, every frame kept and all blocks in one list, or chunk after chunk at the declared
// positions.  stdout: one line per input,
//   lz4 / legacy:  <container> <len> then per frame  " | <kind> <flg> <nominal> <content> <truncated> <fault> <end>" and " <off>:<len>:<raw>:<next>" per block
//   snappy:        snappy <len> <id 0|1>   then per chunk  " | <kind> <hdr> <body> <len> <stored> <next>"
// Checked here: every block and every stored chunk lies inside the file, no position is behind the end of the file, positions never step back,
// and what the collection holds in the end (frames and blocks, reserved room included) stays linear in the file however many frames it has.
// A violation is printed ("VIOLATION ...") and makes the exit status 1.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "alz_framing.h"

using namespace alz_framing;

static bool g_bad = false;
static void require(bool ok, const char* what, size_t line) {
    if (!ok) { g_bad = true; printf(" VIOLATION(%s, input %zu)", what, line); }
}

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

static void walk_lz4(const uint8_t* src, size_t len, size_t line) {
    static const char* const kinds[] = { "none", "legacy", "frame", "skippable" };
    std::vector<Lz4Frame> frames; std::vector<Lz4Block> blocks; size_t pos = 0; uint32_t magic = 0;
    while (magic != 0 || pos < len) {
        frames.emplace_back(); Lz4Frame& f = frames.back();
        lz4_read_frame(src, len, pos, magic, f, blocks);
        printf(" | %s %u %u %llu %d %d %zu", kinds[f.kind], f.flg, f.nominal, (unsigned long long)f.content, (int)f.truncated, f.fault, f.end);
        size_t at = pos;
        require(f.first + f.count == blocks.size(), "block range", line);
        for (size_t i = f.first; i < blocks.size(); i++) {
            const Lz4Block& b = blocks[i];
            const size_t next = f.behind(b);
            printf(" %zu:%u:%d:%zu", b.off, b.len, (int)b.raw, next);
            require(b.off >= at, "block steps back", line);
            require(b.off <= len && b.len <= len - b.off, "block outside the file", line);
            require(next >= b.off + b.len && next <= len, "position behind a block", line);
            at = next;
        }
        require(f.end >= at && f.end <= len, "end of the read", line);
        require(!(f.truncated && f.fault != ALZ_OK), "truncated and faulted", line);
        pos = f.end; magic = f.next_magic;
        if (f.fault != ALZ_OK || f.truncated || f.ends_file) break;
        if (f.flg & 4) { if (pos + 4 > len) break; pos += 4; }
    }
    // a frame is at least 4 bytes of the file and a block at least 4 (legacy: its size word) -- and one reservation of 2^16 blocks at most
    require(frames.capacity() <= len / 2 + 2 && blocks.capacity() <= len / 2 + (1u << 16), "memory not linear in the file", line);
}

static void walk_snappy(const uint8_t* src, size_t len, size_t line) {
    static const char* const kinds[] = { "compressed", "stored", "skipped", "reserved", "truncated" };
    const bool id = len >= 10 && !memcmp(src, kSnappyId, 10);
    printf(" %d", (int)id);
    for (size_t pos = 10; id && pos < len;) {
        const SnappyChunk c = snappy_read_chunk(src, len, pos);
        printf(" | %s %zu %zu %u %u %zu", kinds[c.kind], c.hdr, c.body, c.len, c.stored, c.next);
        require(c.hdr == pos && c.body >= c.hdr && c.body <= len && c.next >= c.hdr && c.next <= len, "chunk positions", line);
        if (c.kind == SnappyChunk::TRUNCATED || c.kind == SnappyChunk::RESERVED) break;
        require(c.next > pos, "no progress", line);
        if (c.kind == SnappyChunk::STORED) require(c.stored <= len - c.body && c.body + c.stored == c.next, "stored chunk outside the file", line);
        if (c.kind == SnappyChunk::COMPRESSED) { size_t used = 0; (void)snappy_varint(src + c.body, len - c.body, &used); require(used <= len - c.body, "varint outside the file", line); }
        pos = c.next;
    }
}

int main() {
    std::string text; size_t line = 0;
    while (std::getline(std::cin, text)) {
        line++;
        const size_t sp = text.find(' ');
        const std::string container = text.substr(0, sp), hex = sp == std::string::npos ? std::string() : text.substr(sp + 1);
        const bool snappy = container == "snappy";
        if ((!snappy && container != "lz4" && container != "legacy") || hex.size() % 2) { fprintf(stderr, "input %zu: not \"<lz4|legacy|snappy> <hex>\"\n", line); return 2; }
        const size_t len = hex.size() / 2;
        std::unique_ptr<uint8_t[]> buf(new uint8_t[len]);                            // exactly the input: one byte past it is a report
        for (size_t i = 0; i < len; i++) {
            const int h = nibble(hex[2 * i]), l = nibble(hex[2 * i + 1]);
            if (h < 0 || l < 0) { fprintf(stderr, "input %zu: not hex\n", line); return 2; }
            buf[i] = (uint8_t)(h << 4 | l);
        }
        printf("%s %zu", container.c_str(), len);
        if (snappy) walk_snappy(buf.get(), len, line); else walk_lz4(buf.get(), len, line);
        printf("\n");
    }
    return g_bad ? 1 : 0;
}
