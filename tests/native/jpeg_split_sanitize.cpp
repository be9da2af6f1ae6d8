// AddressSanitizer / UndefinedBehaviorSanitizer harness for the host half of the JPEG split (csrc/image_io.cpp: fh_jpeg_header,
// fh_jpeg_entropy, fh_jpeg_reconstruct, fh_jpeg_desc_check), the way a caller of the device path uses it: the header sizes the buffers,
// which are heap arrays of EXACTLY that size, so that one element written past coef_count or one byte past the last pixel row is a report.
//   g++ -fsanitize=address,undefined ... (tests/test_jpeg_split_sanitize.py builds and runs it)
//
//   jpeg_split_sanitize <golden dir>
// Every JPEG fixture goes through as it is (must succeed, and must equal fh_image_decode), then as a few hundred damaged variants —
// truncations, byte flips, 16-byte splats at seeded positions — each of which must come back as an error or a picture.  A variant whose
// later markers disagree with its frame header must not move the coefficient bounds: the header call of the SAME bytes sizes the buffer.
#include <dirent.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/facehip.h"

namespace fh {
static std::string g_last;
void set_error(const std::string& msg) { g_last = msg; }
}  // namespace fh

static std::vector<unsigned char> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static std::vector<std::string> list(const std::string& dir, const char* suffix) {
    std::vector<std::string> out;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > strlen(suffix) && n.compare(n.size() - strlen(suffix), strlen(suffix), suffix) == 0) out.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(out.begin(), out.end());
    return out;
}
static uint32_t rng_state = 4321;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static int pictures = 0;

// header -> exactly sized buffers -> entropy -> reconstruct.  Returns the number of failures (0 or 1).
static int split_decode(const std::vector<unsigned char>& b, bool must_succeed, const std::string& what) {
    const std::unique_ptr<unsigned char[]> bytes(new unsigned char[b.size() ? b.size() : 1]);    // (exactly sized too: reads past the file are reports)
    if (!b.empty()) memcpy(bytes.get(), b.data(), b.size());
    auto complain = [&](const char* stage) {
        if (must_succeed) fprintf(stderr, "%s: %s failed: %s\n", what.c_str(), stage, fh::g_last.c_str());
        return must_succeed ? 1 : 0;
    };
    fh_jpeg_desc hd;
    if (fh_jpeg_header(bytes.get(), b.size(), &hd) != 0) return complain("fh_jpeg_header");
    if (hd.coef_count <= 0 || hd.coef_count > (1ll << 31)) { fprintf(stderr, "%s: bogus coef_count %lld\n", what.c_str(), (long long)hd.coef_count); return 1; }
    const size_t cap = (size_t)hd.coef_count;
    const std::unique_ptr<int16_t[]> coef(new int16_t[cap]);
    fh_jpeg_desc d;
    if (fh_jpeg_entropy(bytes.get(), b.size(), &d, coef.get(), cap) != 0) return complain("fh_jpeg_entropy");
    if (d.coef_count != hd.coef_count || (long long)d.rows * d.cols != (long long)hd.rows * hd.cols) {
        fprintf(stderr, "%s: the completed descriptor disagrees with the header\n", what.c_str());
        return 1;
    }
    if (fh_jpeg_desc_check(&d) != 0) { fprintf(stderr, "%s: the parser's own descriptor is refused: %s\n", what.c_str(), fh::g_last.c_str()); return 1; }
    const int step = d.cols * 3 + (int)(rnd() % 3);
    const size_t size = (size_t)(d.rows - 1) * step + (size_t)d.cols * 3;                         // the last row ends after cols * 3 bytes
    const std::unique_ptr<unsigned char[]> px(new unsigned char[size]);
    if (fh_jpeg_reconstruct(&d, coef.get(), px.get(), step) != 0) return complain("fh_jpeg_reconstruct");
    ++pictures;
    // fh_image_decode is the same two calls: same pixels (or, for a file it refuses, nothing to compare)
    unsigned char* whole = nullptr; int rows = 0, cols = 0;
    if (fh_image_decode(bytes.get(), b.size(), &whole, &rows, &cols) != 0) { fprintf(stderr, "%s: fh_image_decode refuses what the split decodes\n", what.c_str()); return 1; }
    int bad = rows != d.rows || cols != d.cols;
    for (int y = 0; !bad && y < rows; ++y) bad = memcmp(whole + (size_t)y * cols * 3, px.get() + (size_t)y * step, (size_t)cols * 3) != 0;
    fh_image_free(whole);
    if (bad) fprintf(stderr, "%s: the split path and fh_image_decode differ\n", what.c_str());
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: jpeg_split_sanitize <tests/golden>\n"); return 2; }
    int bad = 0, images = 0, variants = 0;
    for (const std::string& p : list(std::string(argv[1]) + "/images", ".jpg")) {
        const std::vector<unsigned char> b = slurp(p);
        const bool big = b.size() > 50000;                                 // the 640 x 640 photograph: fewer variants, it is 100x the work
        ++images;
        bad += split_decode(b, true, p);
        for (int t = 0; t < (big ? 16 : 48); ++t) {                        // truncations: dense near the header, sparse over the body
            const size_t n = t < 24 && !big ? (size_t)t * 7 : (size_t)((double)b.size() * (t % 24 + 1) / 25.0);
            if (n >= b.size()) continue;
            bad += split_decode(std::vector<unsigned char>(b.begin(), b.begin() + n), false, p + " truncated"); ++variants;
        }
        for (int t = 0; t < (big ? 24 : 160); ++t) {                       // byte flips, biased towards the first kilobyte (headers, tables)
            std::vector<unsigned char> c = b;
            const size_t pos = (t & 1) ? rnd() % std::min<size_t>(c.size(), 1024) : rnd() % c.size();
            c[pos] ^= (unsigned char)(1u << (rnd() % 8));
            if (t % 3 == 0) c[pos] = (unsigned char)rnd();
            bad += split_decode(c, false, p + " flipped"); ++variants;
        }
        for (int t = 0; t < (big ? 8 : 48); ++t) {                         // splats
            std::vector<unsigned char> c = b;
            const size_t pos = rnd() % c.size();
            for (size_t i = pos; i < std::min(c.size(), pos + 16); ++i) c[i] = (t & 1) ? 0xFF : 0x00;
            bad += split_decode(c, false, p + " splat"); ++variants;
        }
    }
    // a second frame header that claims a larger picture, spliced in front of the first scan: an error, never a larger write
    for (const std::string& p : list(std::string(argv[1]) + "/images", "420_q75_odd.jpg")) {
        const std::vector<unsigned char> b = slurp(p);
        size_t sof = 0, sos = 0;
        for (size_t i = 2; i + 1 < b.size() && !sos; ++i) {
            if (b[i] == 0xFF && b[i + 1] == 0xC0 && !sof) sof = i;
            if (b[i] == 0xFF && b[i + 1] == 0xDA) sos = i;
        }
        if (!sof || !sos) { fprintf(stderr, "%s: no SOF0 / SOS found\n", p.c_str()); ++bad; continue; }
        const size_t len = 2 + ((size_t)b[sof + 2] << 8 | b[sof + 3]);
        std::vector<unsigned char> second(b.begin() + sof, b.begin() + sof + len);
        second[5] = 0x04; second[7] = 0x04;                                // 1024+ rows and columns
        std::vector<unsigned char> c(b.begin(), b.begin() + sos);
        c.insert(c.end(), second.begin(), second.end());
        c.insert(c.end(), b.begin() + sos, b.end());
        fh_jpeg_desc d;
        const std::unique_ptr<int16_t[]> coef(new int16_t[1 << 16]);
        if (fh_jpeg_header(c.data(), c.size(), &d) != 0 || d.coef_count > (1 << 16)) { fprintf(stderr, "spliced: header\n"); ++bad; continue; }
        if (fh_jpeg_entropy(c.data(), c.size(), &d, coef.get(), (size_t)d.coef_count) == 0) { fprintf(stderr, "spliced: a second frame header was accepted\n"); ++bad; }
        ++variants;
    }
    printf("jpeg_split_sanitize: %d images, %d damaged variants, %d pictures, %d failures\n", images, variants, pictures, bad);
    return bad ? 1 : (images >= 20 && variants >= 4000 && pictures > images ? 0 : 3);
}
