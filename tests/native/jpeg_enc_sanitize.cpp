// AddressSanitizer / UndefinedBehaviorSanitizer harness for the host half of the JPEG encoder (csrc/image_io.cpp: fh_jpeg_enc_desc,
// fh_jpeg_enc_check, fh_jpeg_forward, fh_jpeg_write, fh_jpeg_write_bound), the way a caller uses it: every buffer is a heap array of
// EXACTLY the size the contract names, so that one byte read past the last pixel row, one element written past coef_count or one byte
// written at or behind out + cap is a report.
//   g++ -fsanitize=address,undefined ... (tests/test_jpeg_enc_sanitize.py builds and runs it)
//
//   jpeg_enc_sanitize
// Seeded pictures of every size 1..40 in both axes (a seeded subset of the pairs), all four layouts, unaligned pixel bases, pitches with
// slack, extreme pixel values (the checkerboard of 0 / 255 at quality 100 gives the largest coefficients: signed overflow in the
// transform would be a report), the writer at every cap from 0 to the bound for small pictures, the round trip through fh_jpeg_entropy,
// and hostile hand-made descriptors, which must be refused before anything is read or written.
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

static uint32_t rng_state = 9876;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int encodes = 0, caps = 0;

// One picture through the whole host path.  kind: 0 noise, 1 all 0, 2 all 255, 3 checkerboard 0 / 255, 4 ramp.  Returns the failures.
static int encode_one(int w, int h, int gray, int sub, int quality, int kind, bool every_cap) {
    char what[96];
    snprintf(what, sizeof(what), "%dx%d gray=%d sub=%d q=%d kind=%d", w, h, gray, sub, quality, kind);
    fh_jpeg_desc d;
    if (fh_jpeg_enc_desc(w, h, gray, sub, quality, &d) != 0 || fh_jpeg_enc_check(&d) != 0) { fprintf(stderr, "%s: descriptor: %s\n", what, fh::g_last.c_str()); return 1; }
    const int step = w * 3 + (int)(rnd() % 7), shift = (int)(rnd() % 4);
    const size_t px_bytes = (size_t)(h - 1) * step + (size_t)w * 3;                               // the last row ends after cols * 3 bytes
    const std::unique_ptr<unsigned char[]> mem(new unsigned char[px_bytes + shift]);
    unsigned char* const px = mem.get() + shift;                                                   // an unaligned base
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < step && (size_t)y * step + x < px_bytes; ++x) {
            unsigned char v = 0;
            if (x < w * 3) {
                const int col = x / 3;
                v = kind == 0 ? (unsigned char)rnd() : kind == 1 ? 0 : kind == 2 ? 255 : kind == 3 ? (((col + y) & 1) ? 255 : 0) : (unsigned char)((col * 5 + y * 3) & 255);
            } else {
                v = 0xEE;
            }
            px[(size_t)y * step + x] = v;
        }
    const size_t n = (size_t)d.coef_count;
    const std::unique_ptr<int16_t[]> coef(new int16_t[n]);
    if (n > 1 && fh_jpeg_forward(&d, px, step, coef.get(), n - 1) == 0) { fprintf(stderr, "%s: fh_jpeg_forward accepted cap = coef_count - 1\n", what); return 1; }
    if (fh_jpeg_forward(&d, px, step, coef.get(), n) != 0) { fprintf(stderr, "%s: fh_jpeg_forward: %s\n", what, fh::g_last.c_str()); return 1; }
    const size_t bound = fh_jpeg_write_bound(&d);
    size_t need = 0;
    {
        const std::unique_ptr<unsigned char[]> none(new unsigned char[1]);
        if (fh_jpeg_write(&d, coef.get(), none.get(), 0, &need) == 0 || need == 0 || need > bound) { fprintf(stderr, "%s: sizing call: need %zu, bound %zu\n", what, need, bound); return 1; }
    }
    const std::unique_ptr<unsigned char[]> file(new unsigned char[need]);                          // exactly the size the sizing call named
    size_t written = 0;
    if (fh_jpeg_write(&d, coef.get(), file.get(), need, &written) != 0 || written != need) { fprintf(stderr, "%s: fh_jpeg_write: %s\n", what, fh::g_last.c_str()); return 1; }
    ++encodes;
    if (every_cap) {
        for (size_t cap = 0; cap < need; cap += (need > 2000 ? 37 : 1)) {
            const std::unique_ptr<unsigned char[]> part(new unsigned char[cap ? cap : 1]);
            size_t wr = 0;
            if (fh_jpeg_write(&d, coef.get(), part.get(), cap, &wr) == 0 || wr != need || memcmp(part.get(), file.get(), cap) != 0) {
                fprintf(stderr, "%s: cap %zu of %zu\n", what, cap, need);
                return 1;
            }
            ++caps;
        }
    }
    // back through the parser: the same coefficients
    fh_jpeg_desc rd;
    const std::unique_ptr<int16_t[]> back(new int16_t[n]);
    if (fh_jpeg_entropy(file.get(), need, &rd, back.get(), n) != 0 || rd.coef_count != d.coef_count || memcmp(back.get(), coef.get(), n * sizeof(int16_t)) != 0) {
        fprintf(stderr, "%s: fh_jpeg_entropy does not return what fh_jpeg_write was given: %s\n", what, fh::g_last.c_str());
        return 1;
    }
    return 0;
}

// A descriptor nobody should accept: every entry point refuses it and touches none of the (one-element) buffers.
static int hostile(fh_jpeg_desc d, const char* what) {
    const std::unique_ptr<unsigned char[]> px(new unsigned char[1]);
    const std::unique_ptr<int16_t[]> coef(new int16_t[1]);
    const std::unique_ptr<unsigned char[]> out(new unsigned char[1]);
    size_t written = 5;
    int bad = 0;
    if (fh_jpeg_enc_check(&d) == 0) bad = 1;
    if (fh_jpeg_forward(&d, px.get(), 1 << 24, coef.get(), (size_t)1 << 40) == 0) bad = 1;
    if (fh_jpeg_write(&d, coef.get(), out.get(), (size_t)1 << 40, &written) == 0 || written != 0) bad = 1;
    if (fh_jpeg_write_bound(&d) != 0) bad = 1;
    if (bad) fprintf(stderr, "hostile descriptor accepted: %s\n", what);
    return bad;
}

int main() {
    int bad = 0, hostiles = 0;
    for (int gray = 0; gray < 2; ++gray)
        for (int sub = 0; sub < (gray ? 1 : 3); ++sub) {
            for (int w = 1; w <= 40; ++w)
                for (int h = 1; h <= 40; ++h) {
                    const bool small = w <= 9 && h <= 9;
                    if (!small && rnd() % 8 != 0 && !(w == 40 || h == 40 || w == 17 || h == 23)) continue;
                    const int quality = (int)(rnd() % 100) + 1;
                    bad += encode_one(w, h, gray, sub, quality, (int)(rnd() % 5), small && (w + h) % 3 == 0);
                }
            for (int kind = 1; kind <= 3; ++kind) bad += encode_one(33, 31, gray, sub, 100, kind, false);   // the extremes at the finest tables
        }
    fh_jpeg_desc base;
    if (fh_jpeg_enc_desc(40, 24, 0, 2, 75, &base) != 0) { fprintf(stderr, "base descriptor\n"); return 2; }
    auto with = [&](void (*edit)(fh_jpeg_desc&), const char* what) { fh_jpeg_desc d = base; edit(d); bad += hostile(d, what); ++hostiles; };
    with([](fh_jpeg_desc& d) { d.width = 1 << 20; }, "width without its grids");
    with([](fh_jpeg_desc& d) { d.comp[0].wblocks = 1 << 20; }, "wblocks");
    with([](fh_jpeg_desc& d) { d.comp[1].hblocks = 0; }, "hblocks 0");
    with([](fh_jpeg_desc& d) { d.comp[2].coef_off = -64; }, "negative coef_off");
    with([](fh_jpeg_desc& d) { d.comp[2].coef_off = (int64_t)1 << 50; }, "coef_off far away");
    with([](fh_jpeg_desc& d) { d.coef_count = 64; }, "coef_count short");
    with([](fh_jpeg_desc& d) { d.comp[0].dw = 1 << 20; }, "dw");
    with([](fh_jpeg_desc& d) { d.comp[1].dh = 0; }, "dh 0");
    with([](fh_jpeg_desc& d) { d.comp[0].h = 4; d.hmax = 4; }, "4:1:1");
    with([](fh_jpeg_desc& d) { d.comp[1].h = 0; }, "h 0");
    with([](fh_jpeg_desc& d) { d.ncomp = 4; }, "ncomp 4");
    with([](fh_jpeg_desc& d) { d.orientation = 8; d.rows = d.width; d.cols = d.height; }, "orientation 8");
    with([](fh_jpeg_desc& d) { d.color = 2; }, "RGB");
    with([](fh_jpeg_desc& d) { d.comp[0].quant[0] = 0; }, "quantiser 0");
    with([](fh_jpeg_desc& d) { d.comp[2].quant[63] = 256; }, "quantiser 256");
    with([](fh_jpeg_desc& d) { d.rows = 1 << 20; }, "rows");
    with([](fh_jpeg_desc& d) { d.height = -1; }, "negative height");
    printf("jpeg_enc_sanitize: %d pictures, %d capped writes, %d hostile descriptors, %d failures\n", encodes, caps, hostiles, bad);
    return bad ? 1 : (encodes >= 400 && caps >= 1000 && hostiles >= 15 ? 0 : 3);
}
