// AddressSanitizer / UndefinedBehaviorSanitizer harness for the host rules of the device Huffman coder (csrc/image_io.cpp:
// fh_jpeg_write_header, fh_jpeg_scan_bits), the way a caller uses them: every buffer is a heap array of EXACTLY the size the contract
// names, so that one byte written at or behind out + cap, one entry written past the scan's blocks or one coefficient read past
// coef_count is a report.
//   g++ -fsanitize=address,undefined ... (tests/test_jpeg_huff_cpu.py builds and runs it)
//
//   jpeg_huff_sanitize
// Seeded coefficient planes of every size 1..40 in both axes (a seeded subset of the pairs), all four layouts; the header at EVERY cap
// from 0 to its size, held to the front of fh_jpeg_write's file; the bits per block held to the file's entropy-coded size; coefficients
// at and beyond the limits of the baseline tables; and hostile hand-made descriptors, which must be refused before anything is read or
// written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../include/facehip.h"

namespace fh {
static std::string g_last;
void set_error(const std::string& msg) { g_last = msg; }
}  // namespace fh

static uint32_t rng_state = 24680;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int planes = 0, caps = 0, refused = 0;

// kind: 0 sparse small values, 1 dense within the limits, 2 all zero, 3 one coefficient beyond the limits (must be refused)
static int one(int w, int h, int gray, int sub, int kind) {
    char what[96];
    snprintf(what, sizeof(what), "%dx%d gray=%d sub=%d kind=%d", w, h, gray, sub, kind);
    fh_jpeg_desc d;
    if (fh_jpeg_enc_desc(w, h, gray, sub, 90, &d) != 0) { fprintf(stderr, "%s: descriptor: %s\n", what, fh::g_last.c_str()); return 1; }
    const size_t n = (size_t)d.coef_count;
    size_t blocks = 0;
    for (int i = 0; i < d.ncomp; ++i) blocks += (size_t)d.comp[i].wblocks * d.comp[i].hblocks;
    const std::unique_ptr<int16_t[]> coef(new int16_t[n]);
    for (size_t k = 0; k < n; ++k) {
        int v = 0;
        if (kind == 0) v = rnd() % 6 == 0 ? (int)(rnd() % 31) - 15 : 0;
        else if (kind == 1 || kind == 3) v = k % 64 == 0 ? (int)(rnd() % 1001) - 500 : (int)(rnd() % 2047) - 1023;   // DC differences stay within +-1000
        coef[k] = (int16_t)v;
    }
    if (kind == 3) {
        const size_t at = rnd() % n;
        coef[at] = (int16_t)(at % 64 == 0 ? (rnd() & 1 ? 32767 : -32768) : (rnd() & 1 ? 1024 : -32768));
    }
    const std::unique_ptr<uint32_t[]> bits(new uint32_t[blocks]);              // exactly the scan's blocks
    if (blocks > 1 && fh_jpeg_scan_bits(&d, coef.get(), bits.get(), blocks - 1) == 0) { fprintf(stderr, "%s: fh_jpeg_scan_bits accepted cap = blocks - 1\n", what); return 1; }
    const int rc = fh_jpeg_scan_bits(&d, coef.get(), bits.get(), blocks);
    size_t need = 0;
    const std::unique_ptr<unsigned char[]> none(new unsigned char[1]);
    const int wrc = fh_jpeg_write(&d, coef.get(), none.get(), 0, &need);
    if (kind == 3) {
        ++refused;
        if (rc == 0 || need != 0 || wrc == 0) { fprintf(stderr, "%s: a coefficient without a code was accepted\n", what); return 1; }
        return 0;
    }
    if (rc != 0 || need == 0) { fprintf(stderr, "%s: fh_jpeg_scan_bits: %s\n", what, fh::g_last.c_str()); return 1; }
    const std::unique_ptr<unsigned char[]> file(new unsigned char[need]);
    size_t written = 0;
    if (fh_jpeg_write(&d, coef.get(), file.get(), need, &written) != 0 || written != need) { fprintf(stderr, "%s: fh_jpeg_write: %s\n", what, fh::g_last.c_str()); return 1; }
    // the header: sized by a call with cap 0, written into exactly that many bytes, the front of the file; every smaller cap is refused
    size_t hdr = 0;
    if (fh_jpeg_write_header(&d, none.get(), 0, &hdr) == 0 || hdr == 0 || hdr >= need) { fprintf(stderr, "%s: header sizing call: %zu\n", what, hdr); return 1; }
    const std::unique_ptr<unsigned char[]> head(new unsigned char[hdr]);
    if (fh_jpeg_write_header(&d, head.get(), hdr, &written) != 0 || written != hdr || memcmp(head.get(), file.get(), hdr) != 0) {
        fprintf(stderr, "%s: the header is not the front of the file\n", what);
        return 1;
    }
    for (size_t cap = 0; cap < hdr; ++cap) {
        const std::unique_ptr<unsigned char[]> part(new unsigned char[cap ? cap : 1]);
        size_t wr = 0;
        if (fh_jpeg_write_header(&d, part.get(), cap, &wr) == 0 || wr != hdr || memcmp(part.get(), file.get(), cap) != 0) { fprintf(stderr, "%s: header cap %zu of %zu\n", what, cap, hdr); return 1; }
        ++caps;
    }
    // the bits add up to the entropy-coded bytes of the file (stuffed zeros taken out)
    unsigned long long total = 0;
    for (size_t b = 0; b < blocks; ++b) {
        if (bits[b] < 4 || bits[b] > 1660) { fprintf(stderr, "%s: block %zu has %u bits\n", what, b, bits[b]); return 1; }
        total += bits[b];
    }
    size_t stuffed = 0;
    for (size_t k = hdr; k + 3 < need; ++k) stuffed += file[k] == 0xFF && file[k + 1] == 0;
    if ((total + 7) / 8 != need - hdr - 2 - stuffed) { fprintf(stderr, "%s: %llu bits against %zu stream bytes\n", what, total, need - hdr - 2 - stuffed); return 1; }
    ++planes;
    return 0;
}

// A descriptor nobody should accept: both entry points refuse it and touch none of the (one-element) buffers.
static int hostile(fh_jpeg_desc d, const char* what) {
    const std::unique_ptr<int16_t[]> coef(new int16_t[1]);
    const std::unique_ptr<unsigned char[]> out(new unsigned char[1]);
    const std::unique_ptr<uint32_t[]> bits(new uint32_t[1]);
    size_t written = 5;
    int bad = 0;
    if (fh_jpeg_write_header(&d, out.get(), (size_t)1 << 40, &written) == 0 || written != 0) bad = 1;
    if (fh_jpeg_scan_bits(&d, coef.get(), bits.get(), (size_t)1 << 40) == 0) bad = 1;
    if (bad) fprintf(stderr, "hostile descriptor accepted: %s\n", what);
    return bad;
}

int main() {
    int bad = 0, hostiles = 0;
    for (int gray = 0; gray < 2; ++gray)
        for (int sub = 0; sub < (gray ? 1 : 3); ++sub)
            for (int w = 1; w <= 40; ++w)
                for (int h = 1; h <= 40; ++h) {
                    const bool small = w <= 9 && h <= 9;
                    if (!small && rnd() % 8 != 0 && !(w == 40 || h == 40 || w == 17 || h == 23)) continue;
                    bad += one(w, h, gray, sub, (int)(rnd() % 4));
                }
    fh_jpeg_desc base;
    if (fh_jpeg_enc_desc(40, 24, 0, 2, 75, &base) != 0) { fprintf(stderr, "base descriptor\n"); return 2; }
    size_t written = 5;
    if (fh_jpeg_write_header(nullptr, nullptr, 0, &written) == 0 || written != 0 || fh_jpeg_write_header(&base, nullptr, 8, &written) == 0 ||
        fh_jpeg_scan_bits(&base, nullptr, nullptr, 0) == 0) { fprintf(stderr, "null arguments accepted\n"); ++bad; }
    auto with = [&](void (*edit)(fh_jpeg_desc&), const char* what) { fh_jpeg_desc d = base; edit(d); bad += hostile(d, what); ++hostiles; };
    with([](fh_jpeg_desc& d) { d.width = 1 << 20; }, "width without its grids");
    with([](fh_jpeg_desc& d) { d.comp[0].wblocks = 1 << 20; }, "wblocks");
    with([](fh_jpeg_desc& d) { d.comp[1].hblocks = 0; }, "hblocks 0");
    with([](fh_jpeg_desc& d) { d.comp[2].coef_off = -64; }, "negative coef_off");
    with([](fh_jpeg_desc& d) { d.comp[2].coef_off = (int64_t)1 << 50; }, "coef_off far away");
    with([](fh_jpeg_desc& d) { d.coef_count = 64; }, "coef_count short");
    with([](fh_jpeg_desc& d) { d.comp[0].h = 4; d.hmax = 4; }, "4:1:1");
    with([](fh_jpeg_desc& d) { d.comp[1].h = 0; }, "h 0");
    with([](fh_jpeg_desc& d) { d.ncomp = 4; }, "ncomp 4");
    with([](fh_jpeg_desc& d) { d.orientation = 8; d.rows = d.width; d.cols = d.height; }, "orientation 8");
    with([](fh_jpeg_desc& d) { d.color = 2; }, "RGB");
    with([](fh_jpeg_desc& d) { d.comp[0].quant[0] = 0; }, "quantiser 0");
    with([](fh_jpeg_desc& d) { d.comp[2].quant[63] = 256; }, "quantiser 256");
    with([](fh_jpeg_desc& d) { d.height = -1; }, "negative height");
    printf("jpeg_huff_sanitize: %d planes, %d capped headers, %d refused planes, %d hostile descriptors, %d failures\n", planes, caps, refused, hostiles, bad);
    return bad ? 1 : (planes >= 300 && caps >= 100000 && refused >= 50 && hostiles >= 14 ? 0 : 3);
}
