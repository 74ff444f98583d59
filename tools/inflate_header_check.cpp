// inflate_header_check.cpp -- a stand-alone host-safety check of the header walks of csrc/alz_inflate_file.cpp (no GPU, no context).
// Build on the CPU with sanitizers and run:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/inflate_header_check.cpp \
//       auroralib/compression_amd/csrc/alz_inflate_file.cpp -o /tmp/inflate_header_check && /tmp/inflate_header_check
// Every input lives in a heap block of exactly its size, so a read past its end is caught.  The walks are reachable with a NULL context: a
// header that is accepted ends in ALZ_E_INVALID where the body would start; the two batch entry points are stubs that must never be reached.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "auroralz.h"

extern "C" int alz_inflate_decode_batch(alz_ctx*, uint32_t, const uint8_t*, size_t, const alz_stream*, uint8_t*, size_t, alz_result*) { abort(); }
extern "C" int alz_inflate_measure_batch(alz_ctx*, uint32_t, const uint8_t*, size_t, const alz_stream*, alz_result*) { abort(); }

static int checks = 0;

static void feed(const std::vector<uint8_t>& v, int want_zlib, int want_gzip) {
    uint8_t* p = (uint8_t*)malloc(v.size() ? v.size() : 1);                     // exactly the input: nothing readable behind it
    if (!v.empty()) memcpy(p, v.data(), v.size());
    size_t a = 0, b = 0; int32_t st = 0;
    const int rz = alz_zlib_decompress(nullptr, p, v.size(), nullptr, 0, &a, &b, &st);
    const int rzm = alz_zlib_measure(nullptr, p, v.size(), 100, &a, &b, &st);
    const int rg = alz_gzip_decompress(nullptr, p, v.size(), nullptr, 0, &a, &b, &st);
    const int rgm = alz_gzip_measure(nullptr, p, v.size(), 100, &a, &b, &st);
    (void)alz_zlib_is_match(p, v.size());
    (void)alz_gzip_is_match(p, v.size());
    if ((want_zlib != 1 && (rz != want_zlib || rzm != want_zlib)) || (want_gzip != 1 && (rg != want_gzip || rgm != want_gzip)) || rz != rzm || rg != rgm) {
        fprintf(stderr, "input of %zu bytes: zlib %d / %d (want %d), gzip %d / %d (want %d)\n", v.size(), rz, rzm, want_zlib, rg, rgm, want_gzip);
        exit(1);
    }
    checks++;
    free(p);
}

int main() {
    const int ANY = 1;
    // gzip: a header with FEXTRA (5 bytes), FNAME, FCOMMENT; every prefix is either no gzip at all or truncated
    std::vector<uint8_t> h = {0x1F, 0x8B, 8, 0x1C, 0, 0, 0, 0, 0, 3, 5, 0, 'e', 'x', 't', 'r', 'a', 'n', 'a', 'm', 'e', 0, 'c', 'o', 'm', 0};
    for (size_t n = 0; n <= h.size(); n++) {
        std::vector<uint8_t> v(h.begin(), h.begin() + n);
        feed(v, ALZ_E_FORMAT, n < 2 ? ALZ_E_FORMAT : (n < h.size() ? ALZ_E_STREAM : ALZ_E_INVALID));
    }
    // FHCRC on top: cut inside it, wrong, and behind a lying XLEN
    std::vector<uint8_t> c = h; c[3] = 0x1E;
    c.push_back(0);
    feed(c, ALZ_E_FORMAT, ALZ_E_STREAM);
    c.push_back(0);
    feed(c, ALZ_E_FORMAT, ANY);                                                 // (ALZ_E_CHECKSUM unless the CRC happens to be 0)
    std::vector<uint8_t> x = h; x[10] = 0xFF; x[11] = 0xFF;
    feed(x, ALZ_E_FORMAT, ALZ_E_STREAM);
    x.resize(12);
    feed(x, ALZ_E_FORMAT, ALZ_E_STREAM);
    x.resize(11);
    feed(x, ALZ_E_FORMAT, ALZ_E_STREAM);
    // names without an end, reserved flag bits, wrong CM, a second magic byte that is wrong
    for (uint8_t flg : {0x08, 0x10, 0x18}) feed({0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3, 'a', 'b', 'c'}, ALZ_E_FORMAT, ALZ_E_STREAM);
    for (uint8_t flg : {0x20, 0x40, 0x80, 0xFF}) feed({0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 3, 0, 0}, ALZ_E_FORMAT, ALZ_E_FORMAT);
    feed({0x1F, 0x8B, 7, 0, 0, 0, 0, 0, 0, 3}, ALZ_E_FORMAT, ALZ_E_FORMAT);
    feed({0x1F, 0x8C, 8, 0, 0, 0, 0, 0, 0, 3}, ALZ_E_FORMAT, ALZ_E_FORMAT);
    // zlib: every 2-byte header with a valid FCHECK or not, alone and with one byte behind it
    for (int cmf = 0; cmf < 256; cmf++)
        for (int flg = 0; flg < 256; flg += 1) {
            const bool ok = (cmf & 15) == 8 && (cmf >> 4) <= 7 && (cmf * 256 + flg) % 31 == 0;
            const int want = !ok ? ALZ_E_FORMAT : ((flg & 0x20) ? ALZ_E_UNSUPPORTED : ALZ_E_INVALID);
            if (ok || (cmf % 16 == 8 && flg % 16 == 0)) {
                feed({(uint8_t)cmf, (uint8_t)flg}, want, ALZ_E_FORMAT);
                feed({(uint8_t)cmf, (uint8_t)flg, 0x01}, want, ALZ_E_FORMAT);
            }
        }
    feed({0x78}, ALZ_E_FORMAT, ALZ_E_FORMAT);
    // is_match on every length up to 9 of both magics
    for (size_t n = 0; n <= 9; n++) {
        std::vector<uint8_t> z = {0x78, 0x9C, 0x01, 0x00, 0x00, 0xFF, 0xFF, 0, 0}, g = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0};
        z.resize(n); g.resize(n);
        feed(z, ANY, ANY);
        feed(g, ANY, ANY);
    }
    printf("inflate_header_check: %d inputs ok\n", checks);
    return 0;
}
