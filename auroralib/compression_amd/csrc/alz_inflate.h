// alz_inflate.h -- DEFLATE (RFC 1951) as zlib's inflate implements it: the launchers of alz_inflate.hip for the host TU.
// Not part of the ABI (include/auroralz.h: alz_inflate_decode_batch / alz_inflate_measure_batch and their _device forms).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "auroralz.h"

#define ALZ_INFLATE_WINDOW 0x8000u   /* the largest distance a distance symbol can name (symbol 29, 13 extra bits: 24577 + 8191) */

// enqueue the decode kernel over `count` streams (index list selects them; NULL = 0..count-1).  There is ONE decode kernel: every context
// mode runs it.
hipError_t alz_launch_inflate_decode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams,
                                     const uint32_t* d_index, uint32_t count, alz_result* d_results);
// the same parser on a counting sink: writes nothing but the results
hipError_t alz_launch_inflate_measure(hipStream_t stream, const void* d_src, const alz_stream* d_streams,
                                      const uint32_t* d_index, uint32_t count, alz_result* d_results);

// ================================================================================================ the other direction: the encoder
// (include/auroralz.h: alz_deflate_*).  A stream is cut into blocks of ALZ_DEFLATE_BLOCK input bytes; every kernel's unit of work is a
// block.  Three launches over all blocks of all streams and one over the streams:
//   find    one wavefront per block: hash chains over the 32 KiB in front of the block and the block itself, a greedy or lazy parse,
//           tokens to scratch, the two histograms, and -- by the code builder below -- the block's plan: stored, fixed or dynamic, its
//           code lengths, its dynamic header and its size in bytes
//   place   one lane per stream: the byte offsets of its blocks, the verdict against dst_cap, the result
//   emit    one wavefront per block: the bits of the block, packed lane-parallel in LDS, stored at its byte offset
// A block that is not the last of its stream and is not stored ends with an EMPTY STORED BLOCK (3 header bits, padding to the byte
// boundary, 00 00 FF FF), so that every block starts on a byte boundary and can be written without knowing the bits in front of it.
#define ALZ_DEFLATE_BLOCK 32704u     /* input bytes per block: a multiple of 64, <= 65535 (a stored block holds one), and with a low byte that is
                                        not 0 -- ZLib.IsMatchStatic (ZLib.cs:70) takes LEN of a stored first block from the header byte and LEN's
                                        low byte and refuses 0, which a first block of 32 768 stored bytes would give it */
#define ALZ_DEFLATE_NLIT 286
#define ALZ_DEFLATE_NDIST 30
#define ALZ_DEFLATE_NCL 19
#define ALZ_DEFLATE_HDR_BYTES 576u   /* a dynamic header behind the 3 block bits: 14 + 19 * 3 + 316 * 14 bits at the very most */
#define ALZ_DEFLATE_STORED 0u
#define ALZ_DEFLATE_FIXEDB 1u
#define ALZ_DEFLATE_DYNAMIC 2u

#ifdef __HIPCC__
#define ALZ_HD __host__ __device__ inline
#else
#define ALZ_HD inline
#endif

// what find leaves for place and emit, per block
struct alz_deflate_plan {
    uint32_t type;       // ALZ_DEFLATE_STORED / FIXEDB / DYNAMIC
    uint32_t ntok;       // tokens of the block (the end-of-block symbol is not one)
    uint32_t bits;       // the 3 block bits, the header, the symbols and the end-of-block -- without the joining
    uint32_t hdr_bits;   // of a dynamic block: the bits of its header behind the 3 block bits
    uint32_t bytes;      // what the block takes in the stream, the joining included
    uint32_t dst_at;     // where, from the stream's dst_off (place)
    uint8_t lit_len[288], dist_len[32];
    uint8_t hdr[ALZ_DEFLATE_HDR_BYTES];
};
// a block of the batch: block `k` of stream `sid`; its tokens start at tokens[tok_at]
struct alz_deflate_blk { uint32_t sid, k; uint64_t tok_at; };
// the builder's arrays (LDS on the device: nothing here lives in private memory)
struct alz_deflate_work {
    uint32_t w[2 * ALZ_DEFLATE_NLIT];
    uint16_t par[2 * ALZ_DEFLATE_NLIT];
    uint16_t ord[ALZ_DEFLATE_NLIT];
    uint16_t blc[16];
    uint32_t cl_freq[ALZ_DEFLATE_NCL];
    uint16_t cl_code[ALZ_DEFLATE_NCL];
    uint8_t cl_len[ALZ_DEFLATE_NCL];
    uint8_t all[ALZ_DEFLATE_NLIT + ALZ_DEFLATE_NDIST];       // the two sets of lengths as the header lists them
    uint8_t rl_sym[ALZ_DEFLATE_NLIT + ALZ_DEFLATE_NDIST];    // their run-length form: symbol 0..18 ...
    uint8_t rl_extra[ALZ_DEFLATE_NLIT + ALZ_DEFLATE_NDIST];  // ... and the value of its extra bits
    uint32_t rl_n, hlit, hdist, hclen;
};

// ---- the symbol tables of RFC 1951 3.2.5, as arithmetic
ALZ_HD uint32_t alz_deflate_log2(uint32_t v) { uint32_t k = 0; while (v >>= 1) k++; return k; }
// length 3..258 -> symbol 257..285, the count and the value of its extra bits
ALZ_HD uint32_t alz_deflate_len_sym(uint32_t len, uint32_t* eb, uint32_t* ev) {
    const uint32_t l = len - 3u;
    if (l < 8u) { *eb = 0; *ev = 0; return 257u + l; }
    if (len == 258u) { *eb = 0; *ev = 0; return 285u; }
    const uint32_t e = alz_deflate_log2(l) - 2u;
    *eb = e; *ev = l & ((1u << e) - 1u);
    return 261u + 4u * e + ((l >> e) & 3u);
}
ALZ_HD uint32_t alz_deflate_len_extra(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
ALZ_HD uint32_t alz_deflate_len_base(uint32_t sym) {
    if (sym < 265u) return sym - 254u;
    if (sym == 285u) return 258u;
    const uint32_t e = (sym - 261u) >> 2;
    return 3u + ((4u + ((sym - 261u) & 3u)) << e);
}
// distance 1..32768 -> symbol 0..29
ALZ_HD uint32_t alz_deflate_dist_sym(uint32_t dist, uint32_t* eb, uint32_t* ev) {
    const uint32_t d = dist - 1u;
    if (d < 4u) { *eb = 0; *ev = 0; return d; }
    const uint32_t k = alz_deflate_log2(d), e = k - 1u;
    *eb = e; *ev = d & ((1u << e) - 1u);
    return 2u * k + ((d >> e) & 1u);
}
ALZ_HD uint32_t alz_deflate_dist_extra(uint32_t sym) { return sym < 4u ? 0u : (sym >> 1) - 1u; }
ALZ_HD uint32_t alz_deflate_dist_base(uint32_t sym) { return sym < 4u ? sym + 1u : 1u + ((2u + (sym & 1u)) << ((sym >> 1) - 1u)); }
ALZ_HD uint32_t alz_deflate_fixed_len(uint32_t sym) { return sym < 144u ? 8u : sym < 256u ? 9u : sym < 280u ? 7u : 8u; }

// ---- code lengths of at most `limit` bits for the `n` counts `freq`: a Huffman tree over the used symbols (sorted by count, then
// symbol: ties never depend on anything else), depths cut at `limit`, and the Kraft sum put back to exactly 1 by lengthening the
// deepest leaves above the limit row (zlib's step).  The longest lengths go to the
// rarest symbols.  One used symbol gets the single 1-bit code; none leaves every length 0.
ALZ_HD void alz_deflate_build_lengths(const uint32_t* freq, uint32_t n, uint32_t limit, uint8_t* lens, alz_deflate_work* k) {
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; i++) {
        lens[i] = 0;
        if (!freq[i]) continue;
        uint32_t j = m++;
        while (j > 0 && freq[k->ord[j - 1]] > freq[i]) { k->ord[j] = k->ord[j - 1]; j--; }
        k->ord[j] = (uint16_t)i;
    }
    if (m == 0) return;
    if (m == 1) { lens[k->ord[0]] = 1; return; }
    for (uint32_t j = 0; j < m; j++) k->w[j] = freq[k->ord[j]];
    uint32_t a = 0, b = m;                                   // the next leaf, the next inner node: both queues are sorted
    for (uint32_t t = m; t < 2 * m - 1; t++) {
        uint32_t sum = 0;
        for (int two = 0; two < 2; two++) {
            const uint32_t x = (a < m && (b >= t || k->w[a] <= k->w[b])) ? a++ : b++;
            sum += k->w[x]; k->par[x] = (uint16_t)t;
        }
        k->w[t] = sum;
    }
    const uint32_t root = 2 * m - 2;
    k->par[root] = 0;                                        // par[] turns into depths from the root down (a parent lies behind its children)
    for (uint32_t i = root; i-- > 0;) k->par[i] = (uint16_t)(k->par[k->par[i]] + 1u);
    for (uint32_t d = 0; d < 16; d++) k->blc[d] = 0;
    for (uint32_t j = 0; j < m; j++) { const uint32_t d = k->par[j]; k->blc[d > limit ? limit : d]++; }
    uint32_t kraft = 0;                                      // in units of 2^-limit
    for (uint32_t d = 1; d <= limit; d++) kraft += (uint32_t)k->blc[d] << (limit - d);
    const uint32_t one = 1u << limit;
    while (kraft > one) {                                    // zlib's step: a leaf of the deepest row above the limit row goes one down and takes a
        uint32_t d = limit - 1;                              // leaf of the limit row as its sibling -- exactly one unit less.  Every cut leaf adds
        while (!k->blc[d]) d--;                              // less than one unit, so the limit row never runs out.
        k->blc[d]--; k->blc[d + 1] += 2; k->blc[limit]--; kraft--;
    }
    uint32_t j = 0;
    for (uint32_t d = limit; d >= 1; d--)
        for (uint32_t c = k->blc[d]; c > 0; c--) lens[k->ord[j++]] = (uint8_t)d;
}

// ---- canonical codes (RFC 1951 3.2.2) of the lengths, BIT-REVERSED: ready to be written LSB first
ALZ_HD void alz_deflate_codes(const uint8_t* lens, uint32_t n, uint16_t* codes, uint16_t* blc /* [16] */) {
    for (uint32_t d = 0; d < 16; d++) blc[d] = 0;
    for (uint32_t i = 0; i < n; i++) blc[lens[i]]++;
    uint32_t code = 0; blc[0] = 0;
    for (uint32_t d = 1; d < 16; d++) { const uint32_t cnt = blc[d]; code <<= 1; blc[d] = (uint16_t)code; code += cnt; }   // blc[d]: the next code of length d
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t d = lens[i];
        if (!d) { codes[i] = 0; continue; }
        uint32_t c = blc[d]++, r = 0;
        for (uint32_t q = 0; q < d; q++) { r = (r << 1) | (c & 1u); c >>= 1; }
        codes[i] = (uint16_t)r;
    }
}

// ---- a serial bit writer over zeroed bytes (LSB first), for the dynamic header
ALZ_HD void alz_deflate_put(uint8_t* buf, uint32_t* pos, uint32_t v, uint32_t n) {
    while (n) {
        const uint32_t off = *pos & 7u, take = 8u - off < n ? 8u - off : n;
        buf[*pos >> 3] = (uint8_t)(buf[*pos >> 3] | ((v & ((1u << take) - 1u)) << off));
        v >>= take; n -= take; *pos += take;
    }
}

// ---- the run-length form (RFC 1951 3.2.7) of the HLIT + HDIST lengths, as one list: a repeat may run from one set into the other
// (zlib's inflate reads them so), a repeat of the previous length (16) never stands first.  Fills all / rl_* / hlit / hdist.
ALZ_HD void alz_deflate_run_lengths(const uint8_t* lit_len, const uint8_t* dist_len, alz_deflate_work* k) {
    uint32_t hlit = ALZ_DEFLATE_NLIT, hdist = ALZ_DEFLATE_NDIST;
    while (hlit > 257u && !lit_len[hlit - 1]) hlit--;
    while (hdist > 1u && !dist_len[hdist - 1]) hdist--;
    k->hlit = hlit; k->hdist = hdist;
    const uint32_t total = hlit + hdist;
    for (uint32_t i = 0; i < hlit; i++) k->all[i] = lit_len[i];
    for (uint32_t i = 0; i < hdist; i++) k->all[hlit + i] = dist_len[i];
    uint32_t r = 0;
    for (uint32_t i = 0; i < total;) {
        const uint32_t v = k->all[i];
        uint32_t run = 1;
        while (i + run < total && k->all[i + run] == v) run++;
        i += run;
        if (v == 0) {
            while (run >= 11u) { const uint32_t c = run < 138u ? run : 138u; k->rl_sym[r] = 18; k->rl_extra[r++] = (uint8_t)(c - 11u); run -= c; }
            if (run >= 3u) { k->rl_sym[r] = 17; k->rl_extra[r++] = (uint8_t)(run - 3u); run = 0; }
        } else {
            k->rl_sym[r] = (uint8_t)v; k->rl_extra[r++] = 0; run--;
            while (run >= 3u) { const uint32_t c = run < 6u ? run : 6u; k->rl_sym[r] = 16; k->rl_extra[r++] = (uint8_t)(c - 3u); run -= c; }
        }
        for (; run; run--) { k->rl_sym[r] = (uint8_t)v; k->rl_extra[r++] = 0; }
    }
    k->rl_n = r;
}
ALZ_HD uint32_t alz_deflate_cl_order(uint32_t i) {           // the order the header lists the code-length code's lengths in
    return i < 3u ? 16u + i : i == 3u ? 0u : (i & 1u) ? 7u - ((i - 5u) >> 1) : 8u + ((i - 4u) >> 1);   // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
}

// ---- the dynamic header behind the 3 block bits, into the zeroed `hdr`; returns its bits.  Builds the code-length code (7 bits at most).
ALZ_HD uint32_t alz_deflate_header(const uint8_t* lit_len, const uint8_t* dist_len, alz_deflate_work* k, uint8_t* hdr) {
    alz_deflate_run_lengths(lit_len, dist_len, k);
    for (uint32_t i = 0; i < ALZ_DEFLATE_NCL; i++) k->cl_freq[i] = 0;
    for (uint32_t i = 0; i < k->rl_n; i++) k->cl_freq[k->rl_sym[i]]++;
    alz_deflate_build_lengths(k->cl_freq, ALZ_DEFLATE_NCL, 7u, k->cl_len, k);
    alz_deflate_codes(k->cl_len, ALZ_DEFLATE_NCL, k->cl_code, k->blc);
    uint32_t hclen = ALZ_DEFLATE_NCL;
    while (hclen > 4u && !k->cl_len[alz_deflate_cl_order(hclen - 1u)]) hclen--;
    k->hclen = hclen;
    uint32_t pos = 0;
    alz_deflate_put(hdr, &pos, k->hlit - 257u, 5); alz_deflate_put(hdr, &pos, k->hdist - 1u, 5); alz_deflate_put(hdr, &pos, hclen - 4u, 4);
    for (uint32_t i = 0; i < hclen; i++) alz_deflate_put(hdr, &pos, k->cl_len[alz_deflate_cl_order(i)], 3);
    for (uint32_t i = 0; i < k->rl_n; i++) {
        const uint32_t s = k->rl_sym[i];
        alz_deflate_put(hdr, &pos, k->cl_code[s], k->cl_len[s]);
        if (s >= 16u) alz_deflate_put(hdr, &pos, k->rl_extra[i], s == 16u ? 2u : s == 17u ? 3u : 7u);
    }
    return pos;
}

// ---- bytes of a block in its stream: a stored block is its 5 bytes and the data; any other block ends at the byte boundary when it
// is the stream's last, and with the empty stored block (3 bits, padding, 00 00 FF FF) otherwise
ALZ_HD uint32_t alz_deflate_block_bytes_of(uint32_t bits, bool final) { return final ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u; }

// ---- the plan of a block from its histograms (lit_freq holds the end-of-block's 1): code lengths, the dynamic header, the three sizes
// in bits -- size[0] stored (8 * (5 + raw_len)), size[1] fixed, size[2] dynamic -- and the smallest in bytes; ties go to the simpler
// form.  `stored_only`: level 0.  `fixed_only`: ALZ_DEFLATE_FIXED.  `p` is zeroed by the caller.
ALZ_HD void alz_deflate_plan_block(const uint32_t* lit_freq, const uint32_t* dist_freq, uint32_t raw_len, uint32_t ntok, bool final, bool stored_only,
                                   bool fixed_only, alz_deflate_work* k, alz_deflate_plan* p, uint32_t* size) {
    p->ntok = ntok;
    size[0] = 8u * (5u + raw_len); size[1] = size[2] = 0xFFFFFFFFu;
    p->type = ALZ_DEFLATE_STORED; p->bits = size[0]; p->bytes = 5u + raw_len; p->hdr_bits = 0;
    if (stored_only) return;
    alz_deflate_build_lengths(lit_freq, ALZ_DEFLATE_NLIT, 15u, p->lit_len, k);
    alz_deflate_build_lengths(dist_freq, ALZ_DEFLATE_NDIST, 15u, p->dist_len, k);
    p->hdr_bits = alz_deflate_header(p->lit_len, p->dist_len, k, p->hdr);
    uint32_t fixed = 3u, dyn = 3u + p->hdr_bits;
    for (uint32_t s = 0; s < ALZ_DEFLATE_NLIT; s++) {
        const uint32_t f = lit_freq[s], e = s > 256u ? alz_deflate_len_extra(s) : 0u;
        fixed += f * (alz_deflate_fixed_len(s) + e); dyn += f * (p->lit_len[s] + e);
    }
    for (uint32_t s = 0; s < ALZ_DEFLATE_NDIST; s++) {
        const uint32_t f = dist_freq[s], e = alz_deflate_dist_extra(s);
        fixed += f * (5u + e); dyn += f * (p->dist_len[s] + e);
    }
    size[1] = fixed; size[2] = dyn;
    if (alz_deflate_block_bytes_of(fixed, final) < p->bytes) { p->type = ALZ_DEFLATE_FIXEDB; p->bits = fixed; p->bytes = alz_deflate_block_bytes_of(fixed, final); }
    if (!fixed_only && alz_deflate_block_bytes_of(dyn, final) < p->bytes) { p->type = ALZ_DEFLATE_DYNAMIC; p->bits = dyn; p->bytes = alz_deflate_block_bytes_of(dyn, final); }
}

// ---- search effort per level 1..9 (include/auroralz.h holds the table): candidates walked per position, a match of that length ends the
// walk, and whether a longer match one byte on turns this position into a literal
ALZ_HD uint32_t alz_deflate_level_chain(int level) { return level <= 1 ? 4u : level == 2 ? 8u : level <= 4 ? 16u : level == 5 ? 32u : level == 6 ? 64u : level == 7 ? 128u : level == 8 ? 256u : 1024u; }
ALZ_HD uint32_t alz_deflate_level_nice(int level) { return level <= 1 ? 32u : level == 2 ? 64u : level <= 4 ? 128u : 258u; }
ALZ_HD bool alz_deflate_level_lazy(int level) { return level >= 4; }

// enqueue the three block launches and the stream launch of one encode batch.  d_blocks: nblocks entries, the blocks of a stream in
// order and together; d_first: per stream (by its index in d_streams) its first block, n + 1 entries; d_tokens: one word per input byte
// of all blocks; d_plans: nblocks entries.  Every stream of d_streams is encoded (the batch has one kind).
hipError_t alz_launch_deflate_encode(hipStream_t stream, const void* d_src, void* d_dst, const alz_stream* d_streams, uint32_t n,
                                     const alz_deflate_blk* d_blocks, uint32_t nblocks, const uint32_t* d_first, uint32_t* d_tokens,
                                     alz_deflate_plan* d_plans, int level, uint32_t flags, alz_result* d_results);
