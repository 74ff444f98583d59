// framing_replay_check -- what csrc/alz_framing.h makes of a file once the results of its bodies are known, stand-alone: the functions that the
// single-file measure, the single-file Snappy decode and the two batched file calls share, with results from the CPU oracle where the library
// has the GPU's (built with AddressSanitizer + UndefinedBehaviorSanitizer by `make -C oracle framing_replay_check`;
// tests/test_framing_replay_cpu.py).  stdin: one input per line,
//   <lz4|legacy> <capacity> <hex of the file> <hex of the decoded bytes> [<status>:<dst_len>:<src_used>]...
//       one result per compressed block in file order, measured without a bound.  The decoded bytes stand where a decoder has its output: the
//       content checksums are verified over them, the first wrong one in file order deciding in front of anything behind it, as in the batch.
//   snappy <capacity> <hex of the file> [<body offset>:<dst_cap>:<status>:<dst_len>:<src_used>]...
//       what the body at that offset, given the rest of the file, returns in a destination of dst_cap bytes (4294967040: no bound)
// A hex field of "-" stands for no bytes; as the file, "=" stands for the file of the line before.
// stdout: one line per input, "<rc> <status> <dst_len> <src_used>" -- for a Snappy file twice, first as a measure reads it (collected at the
// declared places, replayed, collected again where a chunk ends elsewhere), then as a decoder does (layout, judge, and in order from the
// chunk that decodes to more than it declares).  A result that is asked for and not in the list ends the program with status 3.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "alz_framing.h"

using namespace alz_framing;

static int nibble(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

// exactly the bytes: one byte past them is a report
static std::unique_ptr<uint8_t[]> unhex(const std::string& hex, size_t* len, size_t line) {
    if (hex == "-") { *len = 0; return std::unique_ptr<uint8_t[]>(new uint8_t[0]); }
    if (hex.size() % 2) { fprintf(stderr, "input %zu: not hex\n", line); exit(2); }
    *len = hex.size() / 2;
    std::unique_ptr<uint8_t[]> buf(new uint8_t[*len]);
    for (size_t i = 0; i < *len; i++) {
        const int h = nibble(hex[2 * i]), l = nibble(hex[2 * i + 1]);
        if (h < 0 || l < 0) { fprintf(stderr, "input %zu: not hex\n", line); exit(2); }
        buf[i] = (uint8_t)(h << 4 | l);
    }
    return buf;
}

static void print(const Outcome& o) {
    const bool delivered = o.rc == ALZ_OK || o.rc == ALZ_E_STREAM;
    printf("%d %d %llu %zu", o.rc, delivered ? o.status : 0, delivered ? (unsigned long long)o.out : 0ull, delivered ? o.pos : (size_t)0);
}

// a size query's visitor that verifies the content checksums as well, over the bytes it was given
struct Lz4Checked : Lz4Sizes {
    const uint8_t* src; const uint8_t* decoded; size_t decoded_len; bool wrong = false;
    void content_checksum(uint64_t frame_start, uint64_t out, size_t pos) {
        if (out > decoded_len || le32(src + pos) != xxh32(decoded + frame_start, (size_t)(out - frame_start), 0)) wrong = true;
    }
};

static void replay_lz4(const uint8_t* src, size_t len, uint64_t cap, std::istringstream& rest, size_t line) {
    std::string hex, word;
    rest >> hex;
    size_t decoded_len = 0;
    const std::unique_ptr<uint8_t[]> decoded = unhex(hex, &decoded_len, line);
    std::vector<alz_result> rs;
    while (rest >> word) {
        alz_result r = {};
        if (sscanf(word.c_str(), "%d:%u:%u", &r.status, &r.dst_len, &r.src_used) != 3) { fprintf(stderr, "input %zu: not a result: %s\n", line, word.c_str()); exit(2); }
        rs.push_back(r);
    }
    Lz4File w; size_t bodies = 0;
    lz4_collect(src, len, w, [&](const Lz4Block&) { bodies++; });
    if (bodies != rs.size()) { printf("MISSING: %zu results for %zu compressed blocks (input %zu)\n", rs.size(), bodies, line); exit(3); }
    Lz4Checked v; v.src = src; v.decoded = decoded.get(); v.decoded_len = decoded_len;
    const Outcome o = lz4_replay(w, len, cap, rs.data(), v);
    print(v.wrong ? refused(ALZ_E_CHECKSUM) : o);
}

typedef std::map<std::pair<uint64_t, uint32_t>, alz_result> Results;                  // (body offset, dst_cap) -> result
static const alz_result& lookup(const Results& known, uint64_t off, uint32_t cap, size_t line) {
    const Results::const_iterator it = known.find(std::make_pair(off, cap));
    if (it == known.end()) { printf("MISSING: body %llu with dst_cap %u (input %zu)\n", (unsigned long long)off, cap, line); exit(3); }
    return it->second;
}
struct NoSink { void stored(size_t, uint64_t, uint32_t) {} };

static void replay_snappy(const uint8_t* src, size_t len, uint64_t cap, std::istringstream& rest, size_t line) {
    Results known; std::string word;
    while (rest >> word) {
        unsigned long long off; uint32_t dst_cap; alz_result r = {};
        if (sscanf(word.c_str(), "%llu:%u:%d:%u:%u", &off, &dst_cap, &r.status, &r.dst_len, &r.src_used) != 5) { fprintf(stderr, "input %zu: not a result: %s\n", line, word.c_str()); exit(2); }
        known[std::make_pair((uint64_t)off, dst_cap)] = r;
    }
    if (!snappy_has_id(src, len)) { print(refused(ALZ_E_FORMAT)); printf(" "); print(refused(ALZ_E_FORMAT)); return; }
    Outcome o;
    {   // a measure: alz_container_measure.cpp
        SnappyReader r = { 10, 0, 0 };
        std::vector<alz_stream> ss; std::vector<alz_result> rs;
        do {
            ss.clear(); rs.clear();
            snappy_measure_collect(src, len, r.pos, [&](size_t off) { ss.push_back(body(ALZ_FMT_SNAPPY_RAW, off, len - off, 0, kNoBound, 0)); });
            for (const alz_stream& s : ss) rs.push_back(lookup(known, s.src_off, kNoBound, line));
        } while (!snappy_measure_replay(src, len, cap, r, 0, ss.data(), ss.size(), rs.data(), o));
        print(o);
    }
    printf(" ");
    {   // a decode: alz_container.cpp
        SnappyLayout w; NoSink sink;
        snappy_layout(src, len, cap, w, sink);
        std::vector<alz_result> rs;
        for (const SnappyPiece& p : w.pieces) if (!p.stored) rs.push_back(lookup(known, p.off, p.cap, line));
        SnappyReader r;
        if (!snappy_judge(w, cap, [&](size_t k) -> const alz_result& { return rs[k]; }, r, o)) {
            alz_result got; bool have = false;
            while (!snappy_read_on(src, len, cap, r, have ? &got : nullptr, sink, o)) {
                got = lookup(known, r.pos, clamp32((size_t)(r.out < cap ? cap - r.out : 0)), line);
                have = true;
            }
        }
        print(o);
    }
}

int main() {
    std::string text; size_t line = 0, len = 0;
    std::unique_ptr<uint8_t[]> buf;
    while (std::getline(std::cin, text)) {
        line++;
        std::istringstream rest(text);
        std::string container, hex; unsigned long long cap = 0;
        rest >> container >> cap >> hex;
        const bool snappy = container == "snappy";
        if ((!snappy && container != "lz4" && container != "legacy") || !rest) { fprintf(stderr, "input %zu: not \"<lz4|legacy|snappy> <capacity> <hex> ...\"\n", line); return 2; }
        if (hex != "=" || !buf) buf = unhex(hex, &len, line);
        if (snappy) replay_snappy(buf.get(), len, cap, rest, line); else replay_lz4(buf.get(), len, cap, rest, line);
        printf("\n");
    }
    return 0;
}
