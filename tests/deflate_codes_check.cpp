// deflate_codes_check.cpp -- the code builder of the DEFLATE encoder (csrc/alz_inflate.h: host and device code) on the CPU: adversarial
// and random histograms through the length-limited code lengths, the canonical codes, the run-length form, the dynamic header and the
// three block sizes, against RFC 1951's tables and a serial reader / writer written here.  Prints "ok <histograms>" and exits 0, or says
// what failed and exits 1.  Built by tests/test_deflate_cpu.py, plain and with sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "alz_inflate.h"

static int g_checked = 0;
#define REQUIRE(c, ...) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

// RFC 1951 3.2.5, written out
static const int kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
static const int kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const int kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct Token { uint32_t lit_sym, len_extra, dist_sym, dist_extra; };   // lit_sym < 256: a literal; else a match

struct Bits {                                                          // the serial writer and reader of this program
    std::vector<uint8_t> b; size_t n = 0, at = 0;
    void put(uint32_t v, uint32_t k) { for (uint32_t i = 0; i < k; i++, n++) { if (n / 8 >= b.size()) b.push_back(0); b[n / 8] |= ((v >> i) & 1u) << (n % 8); } }
    void put_code(uint32_t code_msb_first, uint32_t len) { for (uint32_t i = len; i-- > 0;) put((code_msb_first >> i) & 1u, 1); }
    uint32_t get(uint32_t k) { uint32_t v = 0; for (uint32_t i = 0; i < k; i++, at++) { REQUIRE(at < n, "read past the end"); v |= (uint32_t)((b[at / 8] >> (at % 8)) & 1u) << i; } return v; }
};

static uint32_t unreverse(uint32_t r, uint32_t len) { uint32_t c = 0; for (uint32_t i = 0; i < len; i++) c = (c << 1) | ((r >> i) & 1u); return c; }

// lengths in 1..limit for used symbols, 0 for unused; Kraft sum exactly 1, or a single 1-bit code; canonical codes prefix-free
static void check_code_set(const uint32_t* freq, const uint8_t* lens, const uint16_t* codes, uint32_t n, uint32_t limit, const char* what) {
    uint64_t kraft = 0; uint32_t used = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (!freq[i]) { REQUIRE(lens[i] == 0, "%s: unused symbol %u has length %u", what, i, lens[i]); continue; }
        REQUIRE(lens[i] >= 1 && lens[i] <= limit, "%s: symbol %u has length %u (limit %u)", what, i, lens[i], limit);
        kraft += 1ull << (limit - lens[i]); used++;
    }
    if (used == 0) return;
    if (used == 1) { REQUIRE(limit == 15 && kraft == 1ull << (limit - 1), "%s: a single symbol takes the 1-bit code (and the code-length code is never one)", what); }
    else REQUIRE(kraft == 1ull << limit, "%s: Kraft sum %llu / %llu with %u symbols", what, (unsigned long long)kraft, 1ull << limit, used);
    std::vector<int> trie(1, 0), child;                                // node: 0 open, 1 a leaf; children at 2 * node + {1, 2} in `child`
    child.assign(2, -1);
    for (uint32_t i = 0; i < n; i++) {
        if (!lens[i]) continue;
        const uint32_t code = unreverse(codes[i], lens[i]);
        int node = 0;
        for (uint32_t k = lens[i]; k-- > 0;) {
            REQUIRE(trie[node] == 0, "%s: the code of symbol %u runs through another code", what, i);
            const int bit = (code >> k) & 1;
            if (child[2 * node + bit] < 0) { child[2 * node + bit] = (int)trie.size(); trie.push_back(0); child.push_back(-1); child.push_back(-1); }
            node = child[2 * node + bit];
        }
        REQUIRE(trie[node] == 0 && child[2 * node] < 0 && child[2 * node + 1] < 0, "%s: the code of symbol %u is a prefix of another", what, i);
        trie[node] = 1;
    }
    for (uint32_t i = 1; i < n; i++)                                   // canonical: among equal lengths the codes rise with the symbol
        for (uint32_t j = i; j-- > 0;)
            if (lens[j] && lens[j] == lens[i]) { REQUIRE(unreverse(codes[j], lens[j]) + 1 == unreverse(codes[i], lens[i]), "%s: not canonical at %u", what, i); break; }
}

// a decoder of one symbol from canonical lengths (slow, explicit)
static uint32_t read_sym(Bits& in, const uint8_t* lens, const uint16_t* codes, uint32_t n) {
    uint32_t code = 0;
    for (uint32_t len = 1; len <= 15; len++) {
        code = (code << 1) | in.get(1);
        for (uint32_t s = 0; s < n; s++) if (lens[s] == len && unreverse(codes[s], len) == code) return s;
    }
    REQUIRE(false, "no code matches");
    return 0;
}

static alz_deflate_work g_work;

static void check_hist(const uint32_t* lit_in, const uint32_t* dist_freq, const std::vector<Token>* tokens, uint32_t raw_len) {
    g_checked++;
    uint32_t lit_freq[ALZ_DEFLATE_NLIT];
    memcpy(lit_freq, lit_in, sizeof(lit_freq));
    if (!lit_freq[256]) lit_freq[256] = 1;                              // a block always holds its end
    alz_deflate_work* k = &g_work;
    for (int final = 0; final < 2; final++) for (int fixed_only = 0; fixed_only < 2; fixed_only++) {
        alz_deflate_plan p; memset(&p, 0, sizeof(p));
        uint32_t size[3];
        alz_deflate_plan_block(lit_freq, dist_freq, raw_len, tokens ? (uint32_t)tokens->size() : 0u, final != 0, false, fixed_only != 0, k, &p, size);
        uint16_t lit_code[288], dist_code[32], blc[16];
        if (final == 0 && fixed_only == 0) {                           // (the codes do not depend on the two switches: checked once)
        alz_deflate_codes(p.lit_len, ALZ_DEFLATE_NLIT, lit_code, blc);
        check_code_set(lit_freq, p.lit_len, lit_code, ALZ_DEFLATE_NLIT, 15, "literal/length");
        alz_deflate_codes(p.dist_len, ALZ_DEFLATE_NDIST, dist_code, blc);
        check_code_set(dist_freq, p.dist_len, dist_code, ALZ_DEFLATE_NDIST, 15, "distance");
        REQUIRE(p.lit_len[286] == 0 && p.lit_len[287] == 0 && p.dist_len[30] == 0 && p.dist_len[31] == 0, "lengths behind the alphabets");
        check_code_set(k->cl_freq, k->cl_len, k->cl_code, ALZ_DEFLATE_NCL, 7, "code-length");
        // the run-length form expands back to the lengths and never repeats across nothing
        REQUIRE(k->hlit >= 257 && k->hlit <= 286 && k->hdist >= 1 && k->hdist <= 30 && k->hclen >= 4 && k->hclen <= 19, "header counts");
        for (uint32_t i = k->hlit; i < ALZ_DEFLATE_NLIT; i++) REQUIRE(p.lit_len[i] == 0, "HLIT cuts a used symbol");
        for (uint32_t i = k->hdist; i < ALZ_DEFLATE_NDIST; i++) REQUIRE(p.dist_len[i] == 0, "HDIST cuts a used symbol");
        std::vector<uint8_t> expanded;
        for (uint32_t i = 0; i < k->rl_n; i++) {
            const uint32_t s = k->rl_sym[i], e = k->rl_extra[i];
            if (s < 16) { REQUIRE(e == 0, "extra bits on a plain length"); expanded.push_back((uint8_t)s); }
            else if (s == 16) { REQUIRE(!expanded.empty(), "repeat 16 with nothing in front of it"); REQUIRE(e <= 3, "16: extra"); expanded.insert(expanded.end(), 3 + e, expanded.back()); }
            else if (s == 17) { REQUIRE(e <= 7, "17: extra"); expanded.insert(expanded.end(), 3 + e, 0); }
            else { REQUIRE(s == 18 && e <= 127, "18: extra"); expanded.insert(expanded.end(), 11 + e, 0); }
        }
        REQUIRE(expanded.size() == k->hlit + k->hdist, "the run-length form expands to %zu of %u lengths", expanded.size(), k->hlit + k->hdist);
        for (uint32_t i = 0; i < k->hlit; i++) REQUIRE(expanded[i] == p.lit_len[i], "literal/length %u expands wrong", i);
        for (uint32_t i = 0; i < k->hdist; i++) REQUIRE(expanded[k->hlit + i] == p.dist_len[i], "distance length %u expands wrong", i);
        // the header, read back by this program's reader
        REQUIRE(p.hdr_bits <= 8 * ALZ_DEFLATE_HDR_BYTES, "header of %u bits", p.hdr_bits);
        for (uint32_t bit = p.hdr_bits; bit < 8 * ALZ_DEFLATE_HDR_BYTES; bit++) REQUIRE(!((p.hdr[bit / 8] >> (bit % 8)) & 1), "a bit behind the header is set");
        Bits in; in.b.assign(p.hdr, p.hdr + ALZ_DEFLATE_HDR_BYTES); in.n = p.hdr_bits;
        const uint32_t hlit = in.get(5) + 257, hdist = in.get(5) + 1, hclen = in.get(4) + 4;
        REQUIRE(hlit == k->hlit && hdist == k->hdist && hclen == k->hclen, "header counts read back");
        uint8_t cl[19] = {0}; uint16_t clc[19];
        for (uint32_t i = 0; i < hclen; i++) cl[kClOrder[i]] = (uint8_t)in.get(3);
        alz_deflate_codes(cl, 19, clc, blc);
        std::vector<uint8_t> got;
        while (got.size() < hlit + hdist) {
            const uint32_t s = read_sym(in, cl, clc, 19);
            if (s < 16) got.push_back((uint8_t)s);
            else if (s == 16) { REQUIRE(!got.empty(), "16 first"); got.insert(got.end(), 3 + in.get(2), got.back()); }
            else if (s == 17) got.insert(got.end(), 3 + in.get(3), 0);
            else got.insert(got.end(), 11 + in.get(7), 0);
        }
        REQUIRE(got == expanded && in.at == p.hdr_bits, "the header reads back to other lengths, or to another end (%zu of %u bits)", in.at, p.hdr_bits);
        }
        // the three sizes against the serial writer
        REQUIRE(size[0] == 8 * (5 + raw_len), "stored size");
        if (tokens) {
            for (int form = 1; form <= 2; form++) {
                Bits w; w.put((uint32_t)final | (uint32_t)form << 1, 3);
                uint8_t ll[288], dl[32]; uint16_t lc[288], dc[32];
                if (form == 1) { for (uint32_t s = 0; s < 288; s++) ll[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8; for (uint32_t s = 0; s < 32; s++) dl[s] = 5; }
                else { memcpy(ll, p.lit_len, 288); memcpy(dl, p.dist_len, 32); for (uint32_t bit = 0; bit < p.hdr_bits; bit++) w.put((p.hdr[bit / 8] >> (bit % 8)) & 1u, 1); }
                alz_deflate_codes(ll, 288, lc, blc); alz_deflate_codes(dl, 32, dc, blc);
                for (const Token& t : *tokens) {
                    w.put_code(unreverse(lc[t.lit_sym], ll[t.lit_sym]), ll[t.lit_sym]);
                    if (t.lit_sym < 256) continue;
                    w.put(t.len_extra, kLenExtra[t.lit_sym - 257]);
                    w.put_code(unreverse(dc[t.dist_sym], dl[t.dist_sym]), dl[t.dist_sym]);
                    w.put(t.dist_extra, kDistExtra[t.dist_sym]);
                }
                w.put_code(unreverse(lc[256], ll[256]), ll[256]);
                REQUIRE(w.n == size[form], "form %d: the builder says %u bits, the writer made %zu", form, size[form], w.n);
            }
            // the choice: the smallest in bytes, the joining counted; never the dynamic form when only fixed is allowed
            uint32_t bytes[3] = {5 + raw_len, final ? (size[1] + 7) / 8 : (size[1] + 3 + 7) / 8 + 4, final ? (size[2] + 7) / 8 : (size[2] + 3 + 7) / 8 + 4};
            if (fixed_only) bytes[2] = 0xFFFFFFFFu;
            REQUIRE(p.type <= 2 && p.bytes == bytes[p.type] && p.bits == size[p.type], "plan: type %u, %u bytes", p.type, p.bytes);
            for (int f = 0; f < 3; f++) REQUIRE(p.bytes <= bytes[f], "form %d is smaller (%u < %u)", f, bytes[f], p.bytes);
        }
    }
}

static void hist_of(const std::vector<Token>& t, uint32_t* lit, uint32_t* dist) {
    memset(lit, 0, 4 * ALZ_DEFLATE_NLIT); memset(dist, 0, 4 * ALZ_DEFLATE_NDIST);
    for (const Token& x : t) { lit[x.lit_sym]++; if (x.lit_sym >= 256) dist[x.dist_sym]++; }
    lit[256] = 1;
}
// tokens whose histograms are the given ones (the length symbols and the distance symbols must be equally many)
static bool tokens_of(const uint32_t* lit, const uint32_t* dist, std::vector<Token>& out) {
    uint64_t nl = 0, nd = 0;
    for (int s = 257; s < ALZ_DEFLATE_NLIT; s++) nl += lit[s];
    for (int s = 0; s < ALZ_DEFLATE_NDIST; s++) nd += dist[s];
    if (nl != nd || (lit[256] != 0 && lit[256] != 1)) return false;
    out.clear();
    for (uint32_t s = 0; s < 256; s++) for (uint32_t c = 0; c < lit[s]; c++) out.push_back(Token{s, 0, 0, 0});
    uint32_t d = 0, dc = 0;
    for (uint32_t s = 257; s < ALZ_DEFLATE_NLIT; s++) for (uint32_t c = 0; c < lit[s]; c++) {
        while (dc == dist[d]) { d++; dc = 0; }
        out.push_back(Token{s, (1u << kLenExtra[s - 257]) - 1u, d, (c * 2654435761u) & ((1u << kDistExtra[d]) - 1u)}); dc++;
    }
    return true;
}
static void check_both(const uint32_t* lit, const uint32_t* dist) {
    std::vector<Token> t;
    uint64_t total = 0;
    for (int s = 0; s < ALZ_DEFLATE_NLIT; s++) total += lit[s];
    if (total <= 200000 && tokens_of(lit, dist, t)) {
        uint64_t raw = 0;
        for (const Token& x : t) raw += x.lit_sym < 256 ? 1 : kLenBase[x.lit_sym - 257];
        check_hist(lit, dist, &t, (uint32_t)(raw > 32768 ? 32768 : raw));
    } else check_hist(lit, dist, nullptr, 1000);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (uint32_t)(g_rng >> 32); }

int main() {
    // ---- the symbol tables: every length and every distance, there and back
    for (uint32_t len = 3; len <= 258; len++) {
        uint32_t eb, ev; const uint32_t s = alz_deflate_len_sym(len, &eb, &ev);
        int want = 28; while (kLenBase[want] > (int)len) want--;
        if (len == 258) want = 28; else if (want == 28) want = 27;
        REQUIRE(s == 257u + want && eb == (uint32_t)kLenExtra[want] && ev == len - kLenBase[want] && ev < (1u << eb) + (eb == 0), "length %u -> symbol %u, %u extra bits of value %u", len, s, eb, ev);
        REQUIRE(alz_deflate_len_base(s) == (uint32_t)kLenBase[want] && alz_deflate_len_extra(s) == eb && alz_deflate_len_base(s) + ev == len, "length %u back", len);
    }
    for (uint32_t dist = 1; dist <= 32768; dist++) {
        uint32_t eb, ev; const uint32_t s = alz_deflate_dist_sym(dist, &eb, &ev);
        int want = 29; while (kDistBase[want] > (int)dist) want--;
        REQUIRE(s == (uint32_t)want && eb == (uint32_t)kDistExtra[want] && ev == dist - kDistBase[want] && (eb == 0 ? ev == 0 : ev < (1u << eb)), "distance %u -> symbol %u", dist, s);
        REQUIRE(alz_deflate_dist_base(s) == (uint32_t)kDistBase[want] && alz_deflate_dist_extra(s) == eb && alz_deflate_dist_base(s) + ev == dist, "distance %u back", dist);
    }
    for (uint32_t i = 0; i < 19; i++) REQUIRE(alz_deflate_cl_order(i) == (uint32_t)kClOrder[i], "code-length order %u", i);
    for (uint32_t s = 0; s < 288; s++) REQUIRE(alz_deflate_fixed_len(s) == (s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u), "fixed length %u", s);

    // ---- adversarial histograms
    uint32_t lit[ALZ_DEFLATE_NLIT], dist[ALZ_DEFLATE_NDIST];
    auto clear = [&]() { memset(lit, 0, sizeof(lit)); memset(dist, 0, sizeof(dist)); };
    clear(); check_both(lit, dist);                                    // one used symbol: the end-of-block alone; an empty distance alphabet
    clear(); lit[65] = 100; check_both(lit, dist);                     // two used symbols
    clear(); lit[256] = 1; lit[260] = 7; dist[5] = 7; check_both(lit, dist);                 // a distance alphabet with a single symbol
    clear(); lit[256] = 1; lit[0] = 3; lit[285] = 2; dist[0] = 1; dist[29] = 1; check_both(lit, dist);
    clear(); for (uint32_t& f : lit) f = 1; for (uint32_t& f : dist) f = 1; check_both(lit, dist);   // all 286 equal (29 length symbols against 30 distances: codes only)
    clear(); for (uint32_t& f : lit) f = 30; lit[256] = 1; for (uint32_t& f : dist) f = 29; check_both(lit, dist);   // ... and as tokens
    for (uint32_t n : {20u, 40u}) {                                    // Fibonacci counts: the unlimited tree is n - 1 deep
        clear();
        uint32_t a = 1, b = 1;
        for (uint32_t i = 0; i < n; i++) { lit[i * 6] = a; const uint32_t c = a + b; a = b; b = c; }
        check_both(lit, dist);
        clear(); a = b = 1;
        for (uint32_t i = 0; i < (n < 30 ? n : 30); i++) { dist[i] = a; const uint32_t c = a + b; a = b; b = c; }
        uint64_t total = 0; for (uint32_t f : dist) total += f;
        lit[257] = (uint32_t)total; lit[256] = 1; check_both(lit, dist);
    }
    {                                                                  // the code-length code: Fibonacci counts over its 19 symbols, deeper than 7
        uint32_t f[19], a = 1, b = 1; uint8_t lens[19]; uint16_t codes[19], blc[16];
        for (uint32_t i = 0; i < 19; i++) { f[i] = a; const uint32_t c = a + b; a = b; b = c; }
        alz_deflate_build_lengths(f, 19, 7, lens, &g_work);
        alz_deflate_codes(lens, 19, codes, blc);
        check_code_set(f, lens, codes, 19, 7, "Fibonacci code-length");
        g_checked++;
    }
    clear(); for (uint32_t& f : lit) f = 1; lit[101] = 30000; lit[256] = 1; for (uint32_t i = 0; i < 29; i++) dist[i] = 1; check_both(lit, dist);   // one huge count with 285 ones
    clear(); for (uint32_t s = 0; s < 256; s++) lit[s] = 16; check_both(lit, dist);          // flat literals, no match

    // ---- 20 000 random histograms, as token lists
    std::vector<Token> t;
    for (int round = 0; round < 20000; round++) {
        const uint32_t ntok = 1 + rnd() % (round % 200 == 0 ? 6000u : 250u), nsyms = 1 + rnd() % 256, skew = rnd() % 4, match_per = rnd() % 101;
        const uint32_t dist_span = 1 + rnd() % 30, len_span = 1 + rnd() % 29;
        t.clear();
        uint64_t raw = 0;
        for (uint32_t i = 0; i < ntok; i++) {
            uint32_t r = rnd();
            for (uint32_t s = 0; s < skew; s++) r = r < rnd() ? r : rnd() & r;                // lower values more often
            if (rnd() % 100 < match_per) {
                const uint32_t ls = 257 + (r % len_span), ds = (rnd() >> (skew * 3)) % dist_span;
                t.push_back(Token{ls, rnd() & ((1u << kLenExtra[ls - 257]) - 1u), ds, rnd() & ((1u << kDistExtra[ds]) - 1u)});
                raw += kLenBase[ls - 257];
            } else { t.push_back(Token{(r >> 8) % nsyms, 0, 0, 0}); raw++; }
        }
        hist_of(t, lit, dist);
        check_hist(lit, dist, &t, (uint32_t)(raw > 32768 ? 32768 : raw));
    }
    printf("ok %d\n", g_checked);
    return 0;
}
