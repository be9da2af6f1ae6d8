// image_io.cpp — file -> BGR u8 image, the step in front of the hot path.
//
// What it replaces: `cv::imread(path)` in the reference's callers (src/main.cpp:42,71-72,140-141), i.e.
// OpenCV's default IMREAD_COLOR decode: 8-bit, 3 channels, B-G-R order, alpha dropped, grey replicated,
// 16-bit samples reduced to their high byte, EXIF orientation applied to JPEGs.  OpenCV delegates JPEG to
// libjpeg(-turbo) with its defaults (integer "islow" IDCT, "fancy" triangle chroma up-sampling, 16-bit
// fixed-point YCbCr->RGB); those three published algorithms are restated here so that the pixels are the
// ones the reference's detector would have seen.  Pinned by tests/test_image_io.py against Pillow (which
// wraps the same libjpeg-turbo / zlib) on files written by tests/golden/make_images.py.
//
// Formats: JPEG (baseline, extended-sequential and progressive Huffman, 8-bit, grey / YCbCr / RGB, any
// sampling factors libjpeg up-samples with h2v1 / h2v2 / h1v2 "fancy" or integer replication, restart
// intervals), PNG (all colour types, 1..16 bit, Adam7; inflate from zlib), BMP (24/32-bit BI_RGB),
// binary PPM / PGM.  Host code: runs on the CPU exactly as the reference's imread does.
//
// The JPEG decoder comes in two halves (include/facehip.h, "JPEG in two halves"): the parse up to dense int16 coefficient planes
// (fh_jpeg_header / fh_jpeg_entropy, struct Jpeg) and the reconstruction from them (fh_jpeg_reconstruct, struct Recon), which
// csrc/jpeg_dev.hip restates for the device and is held to, bit for bit.  fh_image_decode of a JPEG is the first followed by the second.
// The way out is here too (include/facehip.h, "JPEG out"): fh_jpeg_enc_desc / fh_jpeg_forward / fh_jpeg_write / fh_imwrite_jpeg, libjpeg's
// forward path and a baseline writer; csrc/jpeg_enc.hip restates fh_jpeg_forward for the device and is held to it, bit for bit.
// This file stays plain C++: no HIP headers, no threads (tests/test_host_sanitize.py builds it with g++ alone).
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/facehip.h"

namespace fh {
void set_error(const std::string& msg);      // api.cpp
}

namespace {

struct Image {
    int rows = 0, cols = 0;
    std::vector<uint8_t> bgr;
};

struct DecodeError {
    std::string msg;
};
[[noreturn]] void fail(const std::string& m) { throw DecodeError{m}; }

// Header sanity: a corrupt file must not make the decoder allocate gigabytes (OpenCV: CV_IO_MAX_IMAGE_PIXELS = 2^30).
constexpr long long kMaxPixels = 1LL << 28;
void check_size(long long w, long long h, const char* fmt) {
    if (w <= 0 || h <= 0 || w > (1 << 20) || h > (1 << 20) || w * h > kMaxPixels) fail(std::string(fmt) + ": unreasonable image size");
}

// =====================================================================================================
// JPEG
// =====================================================================================================
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool present = false;
    uint8_t bits[17] = {0};
    uint8_t vals[256] = {0};
    // canonical decode tables (ITU T.81 F.2.2.3)
    int mincode[17], maxcode[18], valptr[17];
    void build() {
        int code = 0, k = 0;
        for (int l = 1; l <= 16; ++l) {
            valptr[l] = k;
            mincode[l] = code;
            code += bits[l];
            k += bits[l];
            maxcode[l] = bits[l] ? code - 1 : -1;
            code <<= 1;
        }
        maxcode[17] = 0x7fffffff;
        present = true;
    }
};

struct Component {
    int id = 0, h = 1, v = 1, tq = 0;
    int wblocks = 0, hblocks = 0;            // allocated block grid (padded to whole MCUs)
    int dw = 0, dh = 0;                      // "downsampled" real sample dimensions
    int16_t* coef = nullptr;                 // [hblocks][wblocks][64], natural order: the caller's memory (fh_jpeg_entropy), at coef_off
    long long coef_off = 0;
    uint16_t quant[64] = {0};
    bool quant_latched = false;
};

struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint32_t acc = 0;
    int nbits = 0;
    bool hit_marker = false;
    void reset() { acc = 0; nbits = 0; hit_marker = false; }
    void fill() {
        while (nbits <= 24) {
            int b = 0;
            if (!hit_marker && p < end) {
                b = *p;
                if (b == 0xFF) {
                    if (p + 1 < end && p[1] == 0x00) { p += 2; }
                    else { hit_marker = true; b = 0; }          // a marker: feed zeros, leave it in place
                } else {
                    ++p;
                }
            }
            acc |= (uint32_t)b << (24 - nbits);
            nbits += 8;
        }
    }
    int get(int n) {
        if (n == 0) return 0;
        if (nbits < n) fill();
        const int v = (int)(acc >> (32 - n));
        acc <<= n;
        nbits -= n;
        return v;
    }
    int bit() { return get(1); }
};

inline int extend(int v, int n) { return v < (1 << (n - 1)) ? v - (1 << n) + 1 : v; }

int decode_symbol(BitReader& br, const Huff& h) {
    int code = 0;
    for (int l = 1; l <= 16; ++l) {
        code = (code << 1) | br.bit();
        if (h.maxcode[l] >= 0 && code <= h.maxcode[l] && code >= h.mincode[l]) return h.vals[h.valptr[l] + code - h.mincode[l]];
    }
    fail("JPEG: bad Huffman code");
}

struct Jpeg {
    const uint8_t* d;
    size_t n;
    int width = 0, height = 0, ncomp = 0;
    bool progressive = false;
    int hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    Component comp[4];
    uint16_t qt[4][64];
    bool qt_present[4] = {false, false, false, false};
    Huff dc[4], ac[4];
    int restart_interval = 0;
    bool adobe = false;
    int adobe_transform = 0;
    int orientation = 1;
    // where the coefficients go: `cap` int16 elements at coef_mem (fh_jpeg_entropy), or nowhere (fh_jpeg_header stops at the frame header)
    int16_t* coef_mem = nullptr;
    size_t cap = 0;
    bool header_only = false;
    long long coef_count = 0;

    static int u16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

    void parse_exif(const uint8_t* p, int len) {
        if (len < 14 || memcmp(p, "Exif\0\0", 6) != 0) return;
        const uint8_t* t = p + 6;
        const int tl = len - 6;
        const bool le = t[0] == 'I' && t[1] == 'I';
        if (!le && !(t[0] == 'M' && t[1] == 'M')) return;
        auto r16 = [&](int o) { return le ? t[o] | (t[o + 1] << 8) : (t[o] << 8) | t[o + 1]; };
        auto r32 = [&](int o) {
            return le ? (uint32_t)t[o] | ((uint32_t)t[o + 1] << 8) | ((uint32_t)t[o + 2] << 16) | ((uint32_t)t[o + 3] << 24)
                      : ((uint32_t)t[o] << 24) | ((uint32_t)t[o + 1] << 16) | ((uint32_t)t[o + 2] << 8) | (uint32_t)t[o + 3];
        };
        if (r16(2) != 42) return;
        const uint32_t ifd = r32(4);
        if (ifd + 2 > (uint32_t)tl) return;
        const int cnt = r16((int)ifd);
        for (int i = 0; i < cnt; ++i) {
            const int e = (int)ifd + 2 + 12 * i;
            if (e + 12 > tl) return;
            if (r16(e) == 0x0112) {
                const int v = r16(e + 8);
                if (v >= 1 && v <= 8) orientation = v;
                return;
            }
        }
    }

    void read_sof(const uint8_t* p, int len) {
        if (len < 6) fail("JPEG: short SOF");
        if (p[0] != 8) fail("JPEG: only 8-bit precision is supported");
        height = u16(p + 1); width = u16(p + 3); ncomp = p[5];
        if (width <= 0 || height <= 0) fail("JPEG: empty image");
        check_size(width, height, "JPEG");
        if (ncomp != 1 && ncomp != 3) fail("JPEG: only 1- and 3-component images are supported");
        if (len < 6 + 3 * ncomp) fail("JPEG: short SOF");
        for (int i = 0; i < ncomp; ++i) {
            Component& c = comp[i];
            c.id = p[6 + 3 * i]; c.h = p[7 + 3 * i] >> 4; c.v = p[7 + 3 * i] & 15; c.tq = p[8 + 3 * i] & 3;
            if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4) fail("JPEG: bad sampling factor");
            hmax = std::max(hmax, c.h); vmax = std::max(vmax, c.v);
        }
        mcux = (width + 8 * hmax - 1) / (8 * hmax);
        mcuy = (height + 8 * vmax - 1) / (8 * vmax);
        for (int i = 0; i < ncomp; ++i) {
            Component& c = comp[i];
            c.wblocks = mcux * c.h; c.hblocks = mcuy * c.v;
            c.dw = (int)(((long)width * c.h + hmax - 1) / hmax);
            c.dh = (int)(((long)height * c.v + vmax - 1) / vmax);
            if (hmax % c.h || vmax % c.v) fail("JPEG: fractional sampling ratio");
            c.coef_off = coef_count;
            coef_count += (long long)c.wblocks * c.hblocks * 64;
        }
        if (header_only) return;
        // the one place that decides where coefficients may land: the geometry is fixed here (a second frame header is an error), every
        // block index of a scan stays inside its component's grid, so nothing at or behind coef_mem + coef_count is written
        if ((unsigned long long)coef_count > cap) fail("JPEG: the coefficient buffer is too small for this frame");
        memset(coef_mem, 0, (size_t)coef_count * sizeof(int16_t));
        for (int i = 0; i < ncomp; ++i) comp[i].coef = coef_mem + comp[i].coef_off;
    }

    // ---- one scan ------------------------------------------------------------------------------
    int eobrun = 0;

    void decode_block_baseline(BitReader& br, int16_t* blk, const Huff& hd, const Huff& ha, int& pred) {
        const int t = decode_symbol(br, hd);
        if (t > 15) fail("JPEG: bad DC category");              // (a damaged DHT can hold any byte as a symbol; 8-bit files use 0..11)
        const int diff = t ? extend(br.get(t), t) : 0;
        pred += diff;
        blk[0] = (int16_t)pred;
        for (int k = 1; k < 64;) {
            const int rs = decode_symbol(br, ha);
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                if (r != 15) break;
                k += 16;
            } else {
                k += r;
                if (k > 63) fail("JPEG: coefficient index out of range");
                blk[kZigzag[k]] = (int16_t)extend(br.get(s), s);
                ++k;
            }
        }
    }
    void decode_dc_first(BitReader& br, int16_t* blk, const Huff& hd, int& pred, int al) {
        const int t = decode_symbol(br, hd);
        if (t > 15) fail("JPEG: bad DC category");
        const int diff = t ? extend(br.get(t), t) : 0;
        pred += diff;
        blk[0] = (int16_t)(pred * (1 << al));
    }
    void decode_dc_refine(BitReader& br, int16_t* blk, int al) {
        if (br.bit()) blk[0] |= (int16_t)(1 << al);
    }
    void decode_ac_first(BitReader& br, int16_t* blk, const Huff& ha, int ss, int se, int al) {
        if (eobrun > 0) { --eobrun; return; }
        for (int k = ss; k <= se;) {
            const int rs = decode_symbol(br, ha);
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
                if (r < 15) {
                    eobrun = (1 << r) - 1;
                    if (r) eobrun += br.get(r);
                    break;
                }
                k += 16;
            } else {
                k += r;
                if (k > 63) fail("JPEG: coefficient index out of range");
                blk[kZigzag[k]] = (int16_t)(extend(br.get(s), s) * (1 << al));
                ++k;
            }
        }
    }
    void decode_ac_refine(BitReader& br, int16_t* blk, const Huff& ha, int ss, int se, int al) {
        const int p1 = 1 << al, m1 = -(1 << al);
        int k = ss;
        if (eobrun == 0) {
            for (; k <= se;) {
                const int rs = decode_symbol(br, ha);
                int r = rs >> 4;
                const int s = rs & 15;
                int val = 0;
                if (s == 0) {
                    if (r < 15) {
                        eobrun = 1 << r;
                        if (r) eobrun += br.get(r);
                        break;
                    }
                } else {
                    if (s != 1) fail("JPEG: bad refinement symbol");
                    val = br.bit() ? p1 : m1;
                }
                // skip r zero-history coefficients, correcting the non-zero ones on the way
                for (; k <= se; ++k) {
                    int16_t& c = blk[kZigzag[k]];
                    if (c != 0) {
                        if (br.bit() && (c & p1) == 0) c = (int16_t)(c >= 0 ? c + p1 : c + m1);
                    } else {
                        if (r == 0) break;
                        --r;
                    }
                }
                if (val && k <= se) blk[kZigzag[k]] = (int16_t)val;
                ++k;
            }
        }
        if (eobrun > 0) {
            for (; k <= se; ++k) {
                int16_t& c = blk[kZigzag[k]];
                if (c != 0 && br.bit() && (c & p1) == 0) c = (int16_t)(c >= 0 ? c + p1 : c + m1);
            }
            --eobrun;
        }
    }

    // returns the position after the scan's entropy-coded data
    size_t read_scan(size_t pos, int len) {
        const uint8_t* p = d + pos;
        if (len < 1) fail("JPEG: short SOS");
        const int ns = p[0];
        if (ns < 1 || ns > ncomp || len < 1 + 2 * ns + 3) fail("JPEG: bad SOS");
        int ci[4], td[4], ta[4];
        for (int i = 0; i < ns; ++i) {
            const int id = p[1 + 2 * i];
            ci[i] = -1;
            for (int c = 0; c < ncomp; ++c)
                if (comp[c].id == id) ci[i] = c;
            if (ci[i] < 0) fail("JPEG: scan names an unknown component");
            td[i] = p[2 + 2 * i] >> 4; ta[i] = p[2 + 2 * i] & 15;
            if (td[i] > 3 || ta[i] > 3) fail("JPEG: bad table selector");
            Component& c = comp[ci[i]];
            if (!c.quant_latched) {                               // libjpeg latches the table at a component's first scan
                if (!qt_present[c.tq]) fail("JPEG: missing quantisation table");
                memcpy(c.quant, qt[c.tq], sizeof(c.quant));
                c.quant_latched = true;
            }
        }
        const int ss = p[1 + 2 * ns], se = p[2 + 2 * ns], ah = p[3 + 2 * ns] >> 4, al = p[3 + 2 * ns] & 15;
        if (progressive) {
            if (ss > se || se > 63 || (ss == 0 && se != 0) || (ss > 0 && ns != 1) || al > 13) fail("JPEG: bad progressive scan");
        }
        for (int i = 0; i < ns; ++i) {
            const bool need_dc = !progressive || ss == 0, need_ac = !progressive || ss > 0;
            if (need_dc && !(progressive && ah > 0) && !dc[td[i]].present) fail("JPEG: missing DC Huffman table");
            if (need_ac && !ac[ta[i]].present) fail("JPEG: missing AC Huffman table");
        }

        BitReader br{d + pos + len, d + n};
        int pred[4] = {0, 0, 0, 0};
        eobrun = 0;
        int restarts_left = restart_interval, next_rst = 0;
        auto handle_restart = [&]() {
            if (!restart_interval) return;
            if (restarts_left == 0) {
                // expect RSTn at br.p (byte aligned)
                br.reset();
                const uint8_t* q = br.p;
                while (q + 1 < br.end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) {
                    if (q[0] == 0xFF && q[1] != 0 && q[1] != 0xFF) break;      // some other marker: give up resync
                    ++q;
                }
                if (q + 1 < br.end && q[0] == 0xFF && q[1] == 0xD0 + next_rst) q += 2;
                br.p = q;
                next_rst = (next_rst + 1) & 7;
                restarts_left = restart_interval;
                pred[0] = pred[1] = pred[2] = pred[3] = 0;
                eobrun = 0;
            }
            --restarts_left;
        };

        auto do_block = [&](int i, int bx, int by) {
            Component& c = comp[ci[i]];
            int16_t* blk = c.coef + ((size_t)by * c.wblocks + bx) * 64;
            if (!progressive) decode_block_baseline(br, blk, dc[td[i]], ac[ta[i]], pred[i]);
            else if (ss == 0) { if (ah == 0) decode_dc_first(br, blk, dc[td[i]], pred[i], al); else decode_dc_refine(br, blk, al); }
            else { if (ah == 0) decode_ac_first(br, blk, ac[ta[i]], ss, se, al); else decode_ac_refine(br, blk, ac[ta[i]], ss, se, al); }
        };

        if (ns == 1) {                                            // non-interleaved: the component's own block raster
            Component& c = comp[ci[0]];
            const int bw = (c.dw + 7) / 8, bh = (c.dh + 7) / 8;
            for (int by = 0; by < bh; ++by)
                for (int bx = 0; bx < bw; ++bx) {
                    handle_restart();
                    do_block(0, bx, by);
                }
        } else {
            for (int my = 0; my < mcuy; ++my)
                for (int mx = 0; mx < mcux; ++mx) {
                    handle_restart();
                    for (int i = 0; i < ns; ++i) {
                        const Component& c = comp[ci[i]];
                        for (int y = 0; y < c.v; ++y)
                            for (int x = 0; x < c.h; ++x) do_block(i, mx * c.h + x, my * c.v + y);
                    }
                }
        }
        // continue after the entropy-coded segment: scan forward to the next real marker
        const uint8_t* q = br.p;
        while (q + 1 < d + n) {
            if (q[0] == 0xFF && q[1] != 0x00 && q[1] != 0xFF && !(q[1] >= 0xD0 && q[1] <= 0xD7)) break;
            ++q;
        }
        return (size_t)(q - d);
    }

    // ---- the marker loop: everything (fh_jpeg_entropy) or up to the frame header (fh_jpeg_header) ----
    void parse() {
        if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) fail("JPEG: no SOI");
        size_t pos = 2;
        bool have_sof = false, done = false;
        while (!done) {
            while (pos < n && d[pos] != 0xFF) ++pos;
            while (pos < n && d[pos] == 0xFF) ++pos;
            if (pos >= n) break;
            const int m = d[pos++];
            if (m == 0xD9) break;
            if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
            if (pos + 2 > n) fail("JPEG: truncated marker");
            const int len = u16(d + pos) - 2;
            const uint8_t* p = d + pos + 2;
            if (len < 0 || pos + 2 + (size_t)len > n) fail("JPEG: truncated segment");
            switch (m) {
                case 0xC0: case 0xC1: case 0xC2:
                    if (have_sof) fail("JPEG: more than one frame");
                    progressive = m == 0xC2;
                    read_sof(p, len);
                    have_sof = true;
                    if (header_only) return;
                    break;
                case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB: case 0xCD: case 0xCE: case 0xCF:
                    fail("JPEG: lossless / hierarchical / arithmetic-coded files are not supported");
                case 0xC4: {
                    int o = 0;
                    while (o + 17 <= len) {
                        const int tc = p[o] >> 4, th = p[o] & 15;
                        if (tc > 1 || th > 3) fail("JPEG: bad DHT");
                        Huff& h = tc ? ac[th] : dc[th];
                        int total = 0;
                        h.bits[0] = 0;
                        for (int i = 1; i <= 16; ++i) { h.bits[i] = p[o + i]; total += h.bits[i]; }
                        if (total > 256 || o + 17 + total > len) fail("JPEG: bad DHT");
                        memset(h.vals, 0, sizeof(h.vals));
                        memcpy(h.vals, p + o + 17, total);
                        h.build();
                        o += 17 + total;
                    }
                    break;
                }
                case 0xDB: {
                    int o = 0;
                    while (o < len) {
                        const int pq = p[o] >> 4, tq = p[o] & 15;
                        if (tq > 3 || pq > 1 || o + 1 + 64 * (pq + 1) > len) fail("JPEG: bad DQT");
                        for (int i = 0; i < 64; ++i) qt[tq][kZigzag[i]] = pq ? (uint16_t)u16(p + o + 1 + 2 * i) : p[o + 1 + i];
                        qt_present[tq] = true;
                        o += 1 + 64 * (pq + 1);
                    }
                    break;
                }
                case 0xDD:
                    if (len < 2) fail("JPEG: bad DRI");
                    restart_interval = u16(p);
                    break;
                case 0xE1: parse_exif(p, len); break;
                case 0xEE:
                    if (len >= 12 && memcmp(p, "Adobe", 5) == 0) { adobe = true; adobe_transform = p[11]; }
                    break;
                case 0xDA:
                    if (!have_sof) fail("JPEG: scan before frame header");
                    pos = read_scan(pos + 2, len);
                    continue;
                default: break;
            }
            pos += 2 + (size_t)len;
        }
        if (!have_sof) fail("JPEG: no frame header");
        for (int i = 0; i < ncomp; ++i)
            if (!comp[i].quant_latched) fail("JPEG: component without a scan");
    }

    // what reconstruction needs (fh_jpeg_desc, include/facehip.h); after a header-only parse the quantisers are still zero
    void fill_desc(fh_jpeg_desc* o) const {
        memset(o, 0, sizeof(*o));
        o->width = width; o->height = height;
        o->orientation = orientation;
        o->rows = orientation >= 5 ? width : height; o->cols = orientation >= 5 ? height : width;
        o->ncomp = ncomp; o->hmax = hmax; o->vmax = vmax;
        const bool rgb = ncomp == 3 && (adobe ? adobe_transform == 0 : (comp[0].id == 'R' && comp[1].id == 'G' && comp[2].id == 'B'));
        o->color = ncomp == 1 ? 0 : rgb ? 2 : 1;
        o->coef_count = coef_count;
        for (int i = 0; i < ncomp; ++i) {
            const Component& c = comp[i];
            fh_jpeg_comp& oc = o->comp[i];
            oc.h = c.h; oc.v = c.v; oc.wblocks = c.wblocks; oc.hblocks = c.hblocks; oc.dw = c.dw; oc.dh = c.dh;
            oc.coef_off = c.coef_off;
            memcpy(oc.quant, c.quant, sizeof(oc.quant));
        }
    }
};

// fh_jpeg_desc_check's body: null when the descriptor is one the parser could have produced, else the complaint.  Everything both
// reconstructions index with is pinned here: the block grids and sample sizes follow from width / height and the sampling factors, the
// coefficient ranges lie inside [0, coef_count) and apart from each other.
const char* bad_desc(const fh_jpeg_desc* o) {
    if (!o) return "null descriptor";
    if (o->ncomp != 1 && o->ncomp != 3) return "ncomp must be 1 or 3";
    if (o->width <= 0 || o->height <= 0 || o->width > (1 << 20) || o->height > (1 << 20) || (long long)o->width * o->height > kMaxPixels)
        return "unreasonable image size";
    if (o->orientation < 1 || o->orientation > 8) return "orientation outside 1..8";
    const bool swap = o->orientation >= 5;
    if (o->rows != (swap ? o->width : o->height) || o->cols != (swap ? o->height : o->width)) return "rows / cols do not follow from width / height and the orientation";
    if (o->color < 0 || o->color > 2 || (o->ncomp == 1) != (o->color == 0)) return "color must be 0 for one component and 1 or 2 for three";
    if (o->hmax < 1 || o->hmax > 4 || o->vmax < 1 || o->vmax > 4) return "hmax / vmax outside 1..4";
    int hm = 0, vm = 0;
    for (int i = 0; i < o->ncomp; ++i) {
        const fh_jpeg_comp& c = o->comp[i];
        if (c.h < 1 || c.h > 4 || c.v < 1 || c.v > 4) return "a sampling factor outside 1..4";
        if (o->hmax % c.h || o->vmax % c.v) return "fractional sampling ratio";
        hm = std::max(hm, c.h); vm = std::max(vm, c.v);
    }
    if (hm != o->hmax || vm != o->vmax) return "hmax / vmax are not the largest sampling factors";
    const int mcux = (o->width + 8 * o->hmax - 1) / (8 * o->hmax), mcuy = (o->height + 8 * o->vmax - 1) / (8 * o->vmax);
    if (o->coef_count < 0) return "negative coef_count";
    for (int i = 0; i < o->ncomp; ++i) {
        const fh_jpeg_comp& c = o->comp[i];
        if (c.wblocks != mcux * c.h || c.hblocks != mcuy * c.v) return "a block grid does not match width / height";
        if (c.dw != (int)(((long long)o->width * c.h + o->hmax - 1) / o->hmax) || c.dh != (int)(((long long)o->height * c.v + o->vmax - 1) / o->vmax))
            return "dw / dh do not match width / height";
        const long long len = (long long)c.wblocks * c.hblocks * 64;
        if (c.coef_off < 0 || c.coef_off > o->coef_count || len > o->coef_count - c.coef_off) return "a coef_off range exceeds coef_count";
        for (int j = 0; j < i; ++j) {
            const fh_jpeg_comp& e = o->comp[j];
            const long long elen = (long long)e.wblocks * e.hblocks * 64;
            if (c.coef_off < e.coef_off + elen && e.coef_off < c.coef_off + len) return "coef_off ranges overlap";
        }
    }
    return nullptr;
}

// fh_jpeg_reconstruct's working state: the components' IDCT output planes, then up-sampling and colour conversion to an Image
struct Recon {
    struct RComp {
        int h, v, wblocks, hblocks, dw, dh;
        std::vector<uint8_t> plane;              // IDCT output, (hblocks*8) x (wblocks*8)
    };
    int width = 0, height = 0, ncomp = 0, hmax = 1, vmax = 1;
    RComp comp[3];

    // ---- inverse DCT: jidctint.c "islow" (13-bit constants, 2 extra bits between the passes) ----
    static inline uint8_t range_limit(int x) {                 // libjpeg's centred range-limit table, index & 1023
        const int i = x & 1023;
        if (i < 128) return (uint8_t)(i + 128);
        if (i < 512) return 255;
        if (i < 896) return 0;
        return (uint8_t)(i - 896);
    }
    static void idct_islow(const int16_t* in, const uint16_t* q, uint8_t* out, int stride) {
        constexpr int CB = 13, P1 = 2;
        constexpr long F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                       F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
        long ws[64];
        auto descale = [](long x, int nb) { return (x + (1L << (nb - 1))) >> nb; };
        for (int c = 0; c < 8; ++c) {
            auto v = [&](int r) { return (long)in[r * 8 + c] * q[r * 8 + c]; };
            long z2 = v(2), z3 = v(6);
            long z1 = (z2 + z3) * F0_541;
            long tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
            z2 = v(0); z3 = v(4);
            long tmp0 = (z2 + z3) * (1L << CB), tmp1 = (z2 - z3) * (1L << CB);
            const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
            tmp0 = v(7); tmp1 = v(5); tmp2 = v(3); tmp3 = v(1);
            z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
            long z4 = tmp1 + tmp3;
            const long z5 = (z3 + z4) * F1_175;
            tmp0 *= F0_298; tmp1 *= F2_053; tmp2 *= F3_072; tmp3 *= F1_501;
            z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
            z3 += z5; z4 += z5;
            tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
            ws[0 * 8 + c] = descale(tmp10 + tmp3, CB - P1); ws[7 * 8 + c] = descale(tmp10 - tmp3, CB - P1);
            ws[1 * 8 + c] = descale(tmp11 + tmp2, CB - P1); ws[6 * 8 + c] = descale(tmp11 - tmp2, CB - P1);
            ws[2 * 8 + c] = descale(tmp12 + tmp1, CB - P1); ws[5 * 8 + c] = descale(tmp12 - tmp1, CB - P1);
            ws[3 * 8 + c] = descale(tmp13 + tmp0, CB - P1); ws[4 * 8 + c] = descale(tmp13 - tmp0, CB - P1);
        }
        for (int r = 0; r < 8; ++r) {
            const long* w = ws + r * 8;
            uint8_t* o = out + (size_t)r * stride;
            long z2 = w[2], z3 = w[6];
            long z1 = (z2 + z3) * F0_541;
            long tmp2 = z1 + z3 * (-F1_847), tmp3 = z1 + z2 * F0_765;
            long tmp0 = (w[0] + w[4]) * (1L << CB), tmp1 = (w[0] - w[4]) * (1L << CB);
            const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
            tmp0 = w[7]; tmp1 = w[5]; tmp2 = w[3]; tmp3 = w[1];
            z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
            long z4 = tmp1 + tmp3;
            const long z5 = (z3 + z4) * F1_175;
            tmp0 *= F0_298; tmp1 *= F2_053; tmp2 *= F3_072; tmp3 *= F1_501;
            z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
            z3 += z5; z4 += z5;
            tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
            constexpr int SH = CB + P1 + 3;
            o[0] = range_limit((int)descale(tmp10 + tmp3, SH)); o[7] = range_limit((int)descale(tmp10 - tmp3, SH));
            o[1] = range_limit((int)descale(tmp11 + tmp2, SH)); o[6] = range_limit((int)descale(tmp11 - tmp2, SH));
            o[2] = range_limit((int)descale(tmp12 + tmp1, SH)); o[5] = range_limit((int)descale(tmp12 - tmp1, SH));
            o[3] = range_limit((int)descale(tmp13 + tmp0, SH)); o[4] = range_limit((int)descale(tmp13 - tmp0, SH));
        }
    }

    // ---- chroma up-sampling to full resolution: jdsample.c --------------------------------------
    // src: c.plane (stride sw) with real size dw x dh; result: width x height samples
    std::vector<uint8_t> upsample(const RComp& c) const {
        const int sw = c.wblocks * 8;
        const uint8_t* src = c.plane.data();
        std::vector<uint8_t> out((size_t)width * height);
        const int hx = hmax / c.h, vx = vmax / c.v;
        if (hmax % c.h || vmax % c.v) fail("JPEG: fractional sampling ratio");
        const int dw = c.dw, dh = c.dh;
        auto row = [&](int y) { return src + (size_t)std::min(std::max(y, 0), dh - 1) * sw; };    // edge rows replicate
        if (hx == 1 && vx == 1) {
            for (int y = 0; y < height; ++y) memcpy(&out[(size_t)y * width], row(y), width);
        } else if (hx == 2 && vx == 1 && dw > 2) {                // h2v1_fancy_upsample
            std::vector<uint8_t> line((size_t)2 * dw);
            for (int y = 0; y < height; ++y) {
                const uint8_t* in = row(y);
                line[0] = in[0];
                line[1] = (uint8_t)((in[0] * 3 + in[1] + 2) >> 2);
                for (int i = 1; i < dw - 1; ++i) {
                    const int v = in[i] * 3;
                    line[2 * i] = (uint8_t)((v + in[i - 1] + 1) >> 2);
                    line[2 * i + 1] = (uint8_t)((v + in[i + 1] + 2) >> 2);
                }
                line[2 * dw - 2] = (uint8_t)((in[dw - 1] * 3 + in[dw - 2] + 1) >> 2);
                line[2 * dw - 1] = in[dw - 1];
                memcpy(&out[(size_t)y * width], line.data(), width);
            }
        } else if (hx == 2 && vx == 2 && dw > 2) {                // h2v2_fancy_upsample
            std::vector<uint8_t> line((size_t)2 * dw);
            for (int y = 0; y < height; ++y) {
                const int sy = y >> 1;
                const uint8_t* in0 = row(sy);
                const uint8_t* in1 = row((y & 1) ? sy + 1 : sy - 1);
                int thiscol = in0[0] * 3 + in1[0], nextcol = in0[1] * 3 + in1[1], lastcol;
                line[0] = (uint8_t)((thiscol * 4 + 8) >> 4);
                line[1] = (uint8_t)((thiscol * 3 + nextcol + 7) >> 4);
                lastcol = thiscol; thiscol = nextcol;
                for (int i = 1; i < dw - 1; ++i) {
                    nextcol = in0[i + 1] * 3 + in1[i + 1];
                    line[2 * i] = (uint8_t)((thiscol * 3 + lastcol + 8) >> 4);
                    line[2 * i + 1] = (uint8_t)((thiscol * 3 + nextcol + 7) >> 4);
                    lastcol = thiscol; thiscol = nextcol;
                }
                line[2 * dw - 2] = (uint8_t)((thiscol * 3 + lastcol + 8) >> 4);
                line[2 * dw - 1] = (uint8_t)((thiscol * 4 + 7) >> 4);
                memcpy(&out[(size_t)y * width], line.data(), width);
            }
        } else if (hx == 1 && vx == 2) {                          // h1v2_fancy_upsample (libjpeg-turbo)
            for (int y = 0; y < height; ++y) {
                const int sy = y >> 1;
                const uint8_t* in0 = row(sy);
                const uint8_t* in1 = row((y & 1) ? sy + 1 : sy - 1);
                const int bias = (y & 1) ? 2 : 1;
                for (int x = 0; x < width; ++x) out[(size_t)y * width + x] = (uint8_t)((in0[x] * 3 + in1[x] + bias) >> 2);
            }
        } else {                                                  // int_upsample / h2v1 / h2v2 box replication
            for (int y = 0; y < height; ++y) {
                const uint8_t* in = row(y / vx);
                for (int x = 0; x < width; ++x) out[(size_t)y * width + x] = in[x / hx];
            }
        }
        return out;
    }

    // de-quantise + IDCT every block, up-sample, convert: the picture as coded (the orientation comes after)
    Image run(const fh_jpeg_desc& o, const int16_t* coef) {
        width = o.width; height = o.height; ncomp = o.ncomp; hmax = o.hmax; vmax = o.vmax;
        for (int i = 0; i < ncomp; ++i) {
            const fh_jpeg_comp& oc = o.comp[i];
            RComp& c = comp[i];
            c.h = oc.h; c.v = oc.v; c.wblocks = oc.wblocks; c.hblocks = oc.hblocks; c.dw = oc.dw; c.dh = oc.dh;
            c.plane.assign((size_t)c.wblocks * 8 * c.hblocks * 8, 0);
            const int stride = c.wblocks * 8;
            const int16_t* cc = coef + oc.coef_off;
            for (int by = 0; by < c.hblocks; ++by)
                for (int bx = 0; bx < c.wblocks; ++bx)
                    idct_islow(&cc[((size_t)by * c.wblocks + bx) * 64], oc.quant, &c.plane[(size_t)by * 8 * stride + bx * 8], stride);
        }
        Image img;
        img.rows = height; img.cols = width;
        img.bgr.resize((size_t)width * height * 3);
        if (ncomp == 1) {
            const std::vector<uint8_t> y = upsample(comp[0]);
            for (size_t i = 0; i < y.size(); ++i) img.bgr[3 * i] = img.bgr[3 * i + 1] = img.bgr[3 * i + 2] = y[i];
        } else {
            const std::vector<uint8_t> p0 = upsample(comp[0]), p1 = upsample(comp[1]), p2 = upsample(comp[2]);
            if (o.color == 2) {
                for (size_t i = 0; i < p0.size(); ++i) { img.bgr[3 * i] = p2[i]; img.bgr[3 * i + 1] = p1[i]; img.bgr[3 * i + 2] = p0[i]; }
            } else {                                              // jdcolor.c ycc_rgb_convert, SCALEBITS = 16
                int cr_r[256], cb_b[256];
                long cr_g[256], cb_g[256];
                auto fix = [](double x) { return (long)(x * 65536.0 + 0.5); };
                for (int i = 0; i < 256; ++i) {
                    const long x = i - 128;
                    cr_r[i] = (int)((fix(1.40200) * x + 32768) >> 16);
                    cb_b[i] = (int)((fix(1.77200) * x + 32768) >> 16);
                    cr_g[i] = -fix(0.71414) * x;
                    cb_g[i] = -fix(0.34414) * x + 32768;
                }
                auto clamp = [](int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
                for (size_t i = 0; i < p0.size(); ++i) {
                    const int y = p0[i], cb = p1[i], cr = p2[i];
                    img.bgr[3 * i + 2] = clamp(y + cr_r[cr]);
                    img.bgr[3 * i + 1] = clamp(y + (int)((cb_g[cb] + cr_g[cr]) >> 16));
                    img.bgr[3 * i] = clamp(y + cb_b[cb]);
                }
            }
        }
        return img;
    }
};

Image apply_orientation(Image in, int o) {
    if (o <= 1 || o > 8) return in;
    const int R = in.rows, C = in.cols;
    Image out;
    const bool swap = o >= 5;
    out.rows = swap ? C : R; out.cols = swap ? R : C;
    out.bgr.resize(in.bgr.size());
    for (int y = 0; y < out.rows; ++y)
        for (int x = 0; x < out.cols; ++x) {
            int sy, sx;
            switch (o) {
                case 2: sy = y; sx = C - 1 - x; break;               // mirror horizontal
                case 3: sy = R - 1 - y; sx = C - 1 - x; break;       // rotate 180
                case 4: sy = R - 1 - y; sx = x; break;               // mirror vertical
                case 5: sy = x; sx = y; break;                       // transpose
                case 6: sy = R - 1 - x; sx = y; break;               // rotate 90 clockwise
                case 7: sy = R - 1 - x; sx = C - 1 - y; break;       // transverse
                default: sy = x; sx = C - 1 - y; break;              // 8: rotate 270 clockwise
            }
            memcpy(&out.bgr[((size_t)y * out.cols + x) * 3], &in.bgr[((size_t)sy * C + sx) * 3], 3);
        }
    return out;
}

// =====================================================================================================
// PNG
// =====================================================================================================
uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

void png_unfilter(uint8_t* cur, const uint8_t* prev, int ft, size_t rowbytes, int bpp) {
    switch (ft) {
        case 0: break;
        case 1:
            for (size_t i = bpp; i < rowbytes; ++i) cur[i] = (uint8_t)(cur[i] + cur[i - bpp]);
            break;
        case 2:
            if (prev) for (size_t i = 0; i < rowbytes; ++i) cur[i] = (uint8_t)(cur[i] + prev[i]);
            break;
        case 3:
            for (size_t i = 0; i < rowbytes; ++i) {
                const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0;
                cur[i] = (uint8_t)(cur[i] + ((a + b) >> 1));
            }
            break;
        case 4:
            for (size_t i = 0; i < rowbytes; ++i) {
                const int a = i >= (size_t)bpp ? cur[i - bpp] : 0, b = prev ? prev[i] : 0, c = (prev && i >= (size_t)bpp) ? prev[i - bpp] : 0;
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                cur[i] = (uint8_t)(cur[i] + (pa <= pb && pa <= pc ? a : pb <= pc ? b : c));
            }
            break;
        default: fail("PNG: bad filter type");
    }
}

Image decode_png(const uint8_t* d, size_t n) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (n < 8 || memcmp(d, sig, 8) != 0) fail("PNG: bad signature");
    size_t pos = 8;
    int W = 0, H = 0, depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> idat, plte;
    bool have_hdr = false;
    while (pos + 12 <= n) {
        const uint32_t len = be32(d + pos);
        const uint8_t* type = d + pos + 4;
        const uint8_t* body = d + pos + 8;
        if (pos + 12 + (size_t)len > n) fail("PNG: truncated chunk");
        if (!memcmp(type, "IHDR", 4)) {
            if (len < 13) fail("PNG: bad IHDR");
            W = (int)be32(body); H = (int)be32(body + 4); depth = body[8]; ctype = body[9]; interlace = body[12];
            if (W <= 0 || H <= 0 || body[10] != 0 || body[11] != 0 || interlace > 1) fail("PNG: unsupported header");
            check_size(W, H, "PNG");
            have_hdr = true;
        } else if (!memcmp(type, "PLTE", 4)) {
            plte.assign(body, body + len);
        } else if (!memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), body, body + len);
        } else if (!memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + (size_t)len;
    }
    if (!have_hdr) fail("PNG: no IHDR");
    int ch;
    switch (ctype) {
        case 0: ch = 1; break;
        case 2: ch = 3; break;
        case 3: ch = 1; break;
        case 4: ch = 2; break;
        case 6: ch = 4; break;
        default: fail("PNG: bad colour type");
    }
    const bool depth_ok = (ctype == 0 && (depth == 1 || depth == 2 || depth == 4 || depth == 8 || depth == 16)) ||
                          (ctype == 3 && (depth == 1 || depth == 2 || depth == 4 || depth == 8)) ||
                          ((ctype == 2 || ctype == 4 || ctype == 6) && (depth == 8 || depth == 16));
    if (!depth_ok) fail("PNG: bad bit depth");
    if (ctype == 3 && plte.size() < 3) fail("PNG: palette image without PLTE");
    const int bits_pp = ch * depth, bpp = std::max(1, bits_pp / 8);
    auto rowbytes = [&](int w) { return ((size_t)w * bits_pp + 7) / 8; };

    // pass geometry (Adam7 or the single full pass)
    static const int xs[7] = {0, 4, 0, 2, 0, 1, 0}, ys[7] = {0, 0, 4, 0, 2, 0, 1}, dx[7] = {8, 8, 4, 4, 2, 2, 1}, dy[7] = {8, 8, 8, 4, 4, 2, 2};
    const int npass = interlace ? 7 : 1;
    size_t raw_size = 0;
    for (int p = 0; p < npass; ++p) {
        const int pw = interlace ? (W - xs[p] + dx[p] - 1) / dx[p] : W, ph = interlace ? (H - ys[p] + dy[p] - 1) / dy[p] : H;
        if (pw > 0 && ph > 0) raw_size += (rowbytes(pw) + 1) * (size_t)ph;
    }
    std::vector<uint8_t> raw(raw_size);
    {
        z_stream zs;
        memset(&zs, 0, sizeof(zs));
        if (inflateInit(&zs) != Z_OK) fail("PNG: zlib init failed");
        zs.next_in = idat.data(); zs.avail_in = (uInt)idat.size();
        zs.next_out = raw.data(); zs.avail_out = (uInt)raw.size();
        const int rc = inflate(&zs, Z_FINISH);
        const size_t got = raw.size() - zs.avail_out;
        inflateEnd(&zs);
        if ((rc != Z_STREAM_END && rc != Z_OK && rc != Z_BUF_ERROR) || got != raw.size()) fail("PNG: corrupt image data");
    }

    Image img;
    img.rows = H; img.cols = W;
    img.bgr.assign((size_t)W * H * 3, 0);
    auto put = [&](int x, int y, const uint8_t* row, int i) {       // pixel i of an unfiltered row -> BGR
        uint8_t r, g, b;
        auto sample = [&](int s) -> int {                           // s-th sample of pixel i, reduced to 8 bits
            if (depth == 8) return row[(size_t)i * ch + s];
            if (depth == 16) return row[((size_t)i * ch + s) * 2];  // high byte (png_set_strip_16)
            const int per = 8 / depth, v = (row[i / per] >> (8 - depth * (i % per + 1))) & ((1 << depth) - 1);
            return v;
        };
        if (ctype == 3) {
            const int idx = sample(0);
            if ((size_t)idx * 3 + 2 < plte.size()) { r = plte[idx * 3]; g = plte[idx * 3 + 1]; b = plte[idx * 3 + 2]; }
            else { r = g = b = 0; }
        } else if (ctype == 0 || ctype == 4) {
            int v = sample(0);
            if (depth < 8) v = v * 255 / ((1 << depth) - 1);        // png_set_expand_gray_1_2_4_to_8
            r = g = b = (uint8_t)v;
        } else {
            r = (uint8_t)sample(0); g = (uint8_t)sample(1); b = (uint8_t)sample(2);
        }
        uint8_t* o = &img.bgr[((size_t)y * W + x) * 3];
        o[0] = b; o[1] = g; o[2] = r;
    };
    size_t off = 0;
    for (int p = 0; p < npass; ++p) {
        const int pw = interlace ? (W - xs[p] + dx[p] - 1) / dx[p] : W, ph = interlace ? (H - ys[p] + dy[p] - 1) / dy[p] : H;
        if (pw <= 0 || ph <= 0) continue;
        const size_t rb = rowbytes(pw);
        const uint8_t* prev = nullptr;
        for (int y = 0; y < ph; ++y) {
            uint8_t* line = &raw[off];
            png_unfilter(line + 1, prev, line[0], rb, bpp);
            prev = line + 1;
            for (int x = 0; x < pw; ++x) put(interlace ? xs[p] + x * dx[p] : x, interlace ? ys[p] + y * dy[p] : y, line + 1, x);
            off += rb + 1;
        }
    }
    return img;
}

// =====================================================================================================
// BMP, PPM / PGM
// =====================================================================================================
Image decode_bmp(const uint8_t* d, size_t n) {
    if (n < 54) fail("BMP: truncated header");
    auto le32 = [&](size_t o) { return (int32_t)((uint32_t)d[o] | ((uint32_t)d[o + 1] << 8) | ((uint32_t)d[o + 2] << 16) | ((uint32_t)d[o + 3] << 24)); };
    auto le16 = [&](size_t o) { return d[o] | (d[o + 1] << 8); };
    const size_t data_off = (uint32_t)le32(10);
    const int W = le32(18), Hs = le32(22), bpp = le16(28), comp = le32(30);
    if (le16(26) != 1 || (bpp != 24 && bpp != 32) || (comp != 0 && !(comp == 3 && bpp == 32)) || W <= 0 || Hs == 0) fail("BMP: only uncompressed 24/32-bit files are supported");
    const int H = abs(Hs);
    check_size(W, H, "BMP");
    const size_t stride = ((size_t)W * (bpp / 8) + 3) & ~(size_t)3;
    if (data_off + stride * H > n) fail("BMP: truncated pixel data");
    Image img;
    img.rows = H; img.cols = W;
    img.bgr.resize((size_t)W * H * 3);
    for (int y = 0; y < H; ++y) {
        const uint8_t* src = d + data_off + stride * (size_t)(Hs > 0 ? H - 1 - y : y);
        for (int x = 0; x < W; ++x) memcpy(&img.bgr[((size_t)y * W + x) * 3], src + (size_t)x * (bpp / 8), 3);
    }
    return img;
}

Image decode_pnm(const uint8_t* d, size_t n) {
    size_t pos = 2;
    auto next_int = [&]() {
        for (;;) {
            while (pos < n && isspace(d[pos])) ++pos;
            if (pos < n && d[pos] == '#') { while (pos < n && d[pos] != '\n') ++pos; continue; }
            break;
        }
        if (pos >= n || !isdigit(d[pos])) fail("PNM: bad header");
        long v = 0;
        while (pos < n && isdigit(d[pos])) { v = v * 10 + (d[pos++] - '0'); if (v > (1 << 30)) fail("PNM: bad header"); }
        return (int)v;
    };
    const int ch = d[1] == '6' ? 3 : 1;
    const int W = next_int(), H = next_int(), maxv = next_int();
    if (W <= 0 || H <= 0 || maxv <= 0 || maxv > 255) fail("PNM: only 8-bit binary files are supported");
    check_size(W, H, "PNM");
    ++pos;                                                        // the single whitespace byte after maxval
    if (pos + (size_t)W * H * ch > n) fail("PNM: truncated pixel data");
    Image img;
    img.rows = H; img.cols = W;
    img.bgr.resize((size_t)W * H * 3);
    for (size_t i = 0; i < (size_t)W * H; ++i) {
        const uint8_t* s = d + pos + i * ch;
        if (ch == 3) { img.bgr[3 * i] = s[2]; img.bgr[3 * i + 1] = s[1]; img.bgr[3 * i + 2] = s[0]; }
        else { img.bgr[3 * i] = img.bgr[3 * i + 1] = img.bgr[3 * i + 2] = s[0]; }
    }
    return img;
}

Image decode_any(const uint8_t* d, size_t n) {
    if (n >= 8 && d[0] == 0x89 && d[1] == 'P') return decode_png(d, n);
    if (n >= 2 && d[0] == 'B' && d[1] == 'M') return decode_bmp(d, n);
    if (n >= 2 && d[0] == 'P' && (d[1] == '6' || d[1] == '5')) return decode_pnm(d, n);
    fail("unrecognised image format (JPEG, PNG, BMP, PPM/PGM are supported)");
}

bool is_jpeg(const uint8_t* d, size_t n) { return n >= 3 && d[0] == 0xFF && d[1] == 0xD8; }

// The two halves of the JPEG decoder (fh_jpeg_header / fh_jpeg_entropy, fh_jpeg_reconstruct); both throw DecodeError.
void jpeg_parse(const uint8_t* d, size_t n, fh_jpeg_desc* desc, int16_t* coef, size_t cap, bool header_only) {
    Jpeg j;
    j.d = d; j.n = n;
    j.coef_mem = coef; j.cap = cap; j.header_only = header_only;
    j.parse();
    j.fill_desc(desc);
}
void jpeg_reconstruct(const fh_jpeg_desc& o, const int16_t* coef, uint8_t* bgr, size_t step) {
    if (const char* bad = bad_desc(&o)) fail(std::string("JPEG descriptor: ") + bad);
    Recon rc;
    const Image img = apply_orientation(rc.run(o, coef), o.orientation);
    const size_t row = (size_t)img.cols * 3;
    for (int y = 0; y < img.rows; ++y) memcpy(bgr + (size_t)y * step, &img.bgr[(size_t)y * row], row);
}

// set_error + the C ABI's return value around a throwing body
template <class F>
int jpeg_call(const char* fn, F&& f) {
    try {
        f();
        return 0;
    } catch (const DecodeError& e) {
        fh::set_error(e.msg);
    } catch (const std::exception& e) {
        fh::set_error(std::string(fn) + ": " + e.what());
    }
    return -1;
}

// =====================================================================================================
// JPEG out (include/facehip.h, "JPEG out"): libjpeg's forward path restated — jccolor.c, jcsample.c (no smoothing), jfdctint.c "islow",
// jcdctmgr.c's quantiser, jccoefct.c's dummy blocks — and a baseline writer with the Annex K Huffman tables (jchuff.c without `optimize`).
// fh_jpeg_forward is the oracle csrc/jpeg_enc.hip is held to, bit for bit.
// =====================================================================================================
const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
                               14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// ITU T.81 Annex K.3: bits[1..16] and the symbols, DC / AC, luminance / chrominance
struct StdHuff { uint8_t bits[17]; int nvals; const uint8_t* vals; };
const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const StdHuff kStdHuff[4] = {                                              // index = class * 2 + table: DC0, DC1, AC0, AC1
    {{0, 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, kDcVals},
    {{0, 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, kDcVals},
    {{0, 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, 162, kAcLumaVals},
    {{0, 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}, 162, kAcChromaVals},
};

// code and length of every symbol (jchuff.c jpeg_make_c_derived_tbl); built once, on first use
struct EncHuff {
    uint16_t code[4][256];
    uint8_t len[4][256];
    EncHuff() {
        memset(code, 0, sizeof(code)); memset(len, 0, sizeof(len));
        for (int t = 0; t < 4; ++t) {
            int c = 0, k = 0;
            for (int l = 1; l <= 16; ++l) {
                for (int i = 0; i < kStdHuff[t].bits[l]; ++i, ++k) { code[t][kStdHuff[t].vals[k]] = (uint16_t)c++; len[t][kStdHuff[t].vals[k]] = (uint8_t)l; }
                c <<= 1;
            }
        }
    }
};
const EncHuff& enc_huff() { static const EncHuff h; return h; }

// fh_jpeg_enc_check's body: bad_desc plus what the forward path and the writer rely on
const char* bad_enc_desc(const fh_jpeg_desc* o) {
    if (const char* bad = bad_desc(o)) return bad;
    if (o->width > 65535 || o->height > 65535) return "width / height above 65535 do not fit a frame header";
    if (o->orientation != 1) return "the encoder writes orientation 1 only";
    if (o->color != 0 && o->color != 1) return "the encoder writes grey (color 0) or YCbCr (color 1) only";
    if (o->ncomp == 1 && (o->comp[0].h != 1 || o->comp[0].v != 1)) return "a grey picture's sampling factors must be 1 x 1";
    if (o->ncomp == 3) {
        const fh_jpeg_comp& y = o->comp[0];
        if (o->comp[1].h != 1 || o->comp[1].v != 1 || o->comp[2].h != 1 || o->comp[2].v != 1) return "chroma sampling factors must be 1 x 1";
        if (!((y.h == 1 && y.v == 1) || (y.h == 2 && y.v == 1) || (y.h == 2 && y.v == 2))) return "luma sampling factors must be 1 x 1 (4:4:4), 2 x 1 (4:2:2) or 2 x 2 (4:2:0)";
    }
    for (int i = 0; i < o->ncomp; ++i)
        for (int k = 0; k < 64; ++k)
            if (o->comp[i].quant[k] < 1 || o->comp[i].quant[k] > 255) return "a quantiser outside 1..255 (baseline)";
    return nullptr;
}

// jfdctint.c on one 8x8 block of centred samples (s - 128), in place: the result is 8 x the DCT.  int suffices: |sample| <= 128, the row
// pass's largest term is below 8 * 128 * 25172 * 2 < 2^27, its outputs are below 2^13 (8 * 128 * 4 on the DC path), the column pass's
// largest term is below 8 * 2^13 * 25172 * 2 < 2^31 (libjpeg's own claim for 8-bit samples: its INT32 is 32 bits wide).
inline int fdct_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
template <int PASS>                                                          // 0: rows (stride 1), 1: columns (stride 8)
inline void fdct_1d(int* d) {
    constexpr int S = PASS ? 8 : 1;
    constexpr int F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299, F1_847 = 15137,
                  F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
    constexpr int N = PASS ? 15 : 11;                                      // CONST_BITS + PASS1_BITS / CONST_BITS - PASS1_BITS
    int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S], tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
    int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S], tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (PASS == 0) { d[0] = (tmp10 + tmp11) * 4; d[4 * S] = (tmp10 - tmp11) * 4; }
    else { d[0] = fdct_descale(tmp10 + tmp11, 2); d[4 * S] = fdct_descale(tmp10 - tmp11, 2); }
    int z1 = (tmp12 + tmp13) * F0_541;
    d[2 * S] = fdct_descale(z1 + tmp13 * F0_765, N);
    d[6 * S] = fdct_descale(z1 + tmp12 * (-F1_847), N);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F1_175;
    tmp4 *= F0_298; tmp5 *= F2_053; tmp6 *= F3_072; tmp7 *= F1_501;
    z1 *= -F0_899; z2 *= -F2_562; z3 *= -F1_961; z4 *= -F0_390;
    z3 += z5; z4 += z5;
    d[7 * S] = fdct_descale(tmp4 + z1 + z3, N);
    d[5 * S] = fdct_descale(tmp5 + z2 + z4, N);
    d[3 * S] = fdct_descale(tmp6 + z2 + z3, N);
    d[S] = fdct_descale(tmp7 + z1 + z4, N);
}
// jcdctmgr.c's quantiser on a coefficient scaled by 8: qv = 8 q, round half away from zero
inline int16_t fdct_quant(int c, int q) {
    const int qv = q * 8, t = (c < 0 ? -c : c) + (qv >> 1);
    return (int16_t)(c < 0 ? -(t / qv) : t / qv);
}

// jccolor.c rgb_ycc_convert, SCALEBITS = 16: component ci (0 Y, 1 Cb, 2 Cr) of a B, G, R pixel
inline int ycc_of(const uint8_t* p, int ci) {
    const int b = p[0], g = p[1], r = p[2];
    if (ci == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (ci == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// fh_jpeg_forward's body; the descriptor passed bad_enc_desc
void jpeg_forward(const fh_jpeg_desc& o, const uint8_t* bgr, size_t step, int16_t* coef) {
    const int W = o.width, H = o.height;
    for (int ci = 0; ci < o.ncomp; ++ci) {
        const fh_jpeg_comp& c = o.comp[ci];
        const int hx = o.hmax / c.h, vx = o.vmax / c.v;                      // 1 or 2; vx == 2 only with hx == 2
        const int bw = (c.dw + 7) / 8, bh = (c.dh + 7) / 8;                  // the real blocks
        // the component's sample plane over the real blocks.  Columns: the last picture column repeats (clamped index).  Rows: the last
        // picture row repeats up to a multiple of vmax, then the last DOWN-SAMPLED row repeats (jcprepct.c): sample row min(sy, dh - 1).
        std::vector<uint8_t> plane((size_t)bw * 8 * bh * 8);
        auto px = [&](int x, int y) { return ycc_of(bgr + (size_t)std::min(y, H - 1) * step + (size_t)std::min(x, W - 1) * 3, ci); };
        for (int sy = 0; sy < bh * 8; ++sy) {
            const int y = std::min(sy, c.dh - 1);
            uint8_t* row = &plane[(size_t)sy * bw * 8];
            for (int sx = 0; sx < bw * 8; ++sx) {
                int v;
                if (hx == 1) v = px(sx, y);
                else if (vx == 1) v = (px(2 * sx, y) + px(2 * sx + 1, y) + (sx & 1)) >> 1;                                  // h2v1_downsample
                else v = (px(2 * sx, 2 * y) + px(2 * sx + 1, 2 * y) + px(2 * sx, 2 * y + 1) + px(2 * sx + 1, 2 * y + 1) + 1 + (sx & 1)) >> 2;   // h2v2
                row[sx] = (uint8_t)v;
            }
        }
        int16_t* out = coef + c.coef_off;
        for (int by = 0; by < bh; ++by)
            for (int bx = 0; bx < bw; ++bx) {
                int d[64];
                for (int r = 0; r < 8; ++r)
                    for (int k = 0; k < 8; ++k) d[r * 8 + k] = (int)plane[((size_t)by * 8 + r) * bw * 8 + (size_t)bx * 8 + k] - 128;
                for (int r = 0; r < 8; ++r) fdct_1d<0>(d + r * 8);
                for (int k = 0; k < 8; ++k) fdct_1d<1>(d + k);
                int16_t* blk = out + ((size_t)by * c.wblocks + bx) * 64;
                for (int k = 0; k < 64; ++k) blk[k] = fdct_quant(d[k], c.quant[k]);
            }
        // jccoefct.c's dummy blocks: AC zero; right of the real ones DC = the block to the left; below them DC = the last block of the
        // row above in the same MCU column
        for (int by = 0; by < c.hblocks; ++by)
            for (int bx = 0; bx < c.wblocks; ++bx) {
                if (by < bh && bx < bw) continue;
                const int sy = std::min(by, bh - 1), sx = std::min(by < bh ? bx : bx / c.h * c.h + c.h - 1, bw - 1);
                int16_t* blk = out + ((size_t)by * c.wblocks + bx) * 64;
                memset(blk, 0, 64 * sizeof(int16_t));
                blk[0] = out[((size_t)sy * c.wblocks + sx) * 64];
            }
    }
}

// The writer's sink: counts every byte, stores those in front of `cap`.  Entropy-coded bits gather in a 64-bit word and leave four bytes
// at a time; a word without a 0xFF byte that fits in front of `cap` is stored whole, any other goes byte by byte (0xFF is followed by a
// stuffed zero).
struct ByteSink {
    uint8_t* out;
    size_t cap, pos = 0;
    uint64_t acc = 0;
    int nbits = 0;                                                         // valid low bits of acc; below 32 between calls
    void byte(int b) { if (pos < cap) out[pos] = (uint8_t)b; ++pos; }
    void u16(int v) { byte(v >> 8); byte(v & 255); }
    void marker(int m) { byte(0xFF); byte(m); }
    void data_byte(int b) { byte(b); if (b == 0xFF) byte(0); }
    void bits(unsigned code, int n) {                                      // n <= 27 per call
        acc = (acc << n) | code; nbits += n;
        if (nbits < 32) return;
        nbits -= 32;
        const uint32_t w = (uint32_t)(acc >> nbits);
        if (pos + 4 <= cap && ((~w - 0x01010101u) & w & 0x80808080u) == 0) {
            out[pos] = (uint8_t)(w >> 24); out[pos + 1] = (uint8_t)(w >> 16); out[pos + 2] = (uint8_t)(w >> 8); out[pos + 3] = (uint8_t)w;
            pos += 4;
        } else {
            data_byte((int)(w >> 24)); data_byte((int)((w >> 16) & 255)); data_byte((int)((w >> 8) & 255)); data_byte((int)(w & 255));
        }
    }
    void flush() {                                                         // pad the last byte with ones
        if (nbits & 7) { const int pad = 8 - (nbits & 7); acc = (acc << pad) | ((1u << pad) - 1); nbits += pad; }
        for (; nbits > 0; nbits -= 8) data_byte((int)((acc >> (nbits - 8)) & 255));
    }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// fh_jpeg_scan_bits's sink: the bits encode_block emits, counted
struct BitCount {
    uint32_t n = 0;
    void bits(unsigned, int k) { n += (uint32_t)k; }
};

// jchuff.c encode_one_block into a ByteSink or a BitCount; false for a DC difference outside +-2047 or an AC value outside +-1023
template <class Sink>
bool encode_block(Sink& s, const EncHuff& h, const int16_t* blk, int& pred, int dc_tbl, int ac_tbl) {
    const int diff = blk[0] - pred;
    pred = blk[0];
    int t = diff < 0 ? -diff : diff, t2 = diff < 0 ? diff - 1 : diff;
    int n = bit_length((unsigned)t);
    if (n > 11) return false;
    s.bits(((unsigned)h.code[dc_tbl][n] << n) | ((unsigned)t2 & ((1u << n) - 1)), h.len[dc_tbl][n] + n);
    uint64_t nz = 0;                                                       // bit k: the coefficient at zigzag position k is not zero
    for (int k = 1; k < 64; ++k) nz |= (uint64_t)(blk[kZigzag[k]] != 0) << k;
    int prev = 0;
    for (; nz; nz &= nz - 1) {
        const int k = __builtin_ctzll(nz), v = blk[kZigzag[k]];
        int run = k - prev - 1;
        prev = k;
        for (; run > 15; run -= 16) s.bits(h.code[ac_tbl][0xF0], h.len[ac_tbl][0xF0]);
        t = v < 0 ? -v : v; t2 = v < 0 ? v - 1 : v;
        n = bit_length((unsigned)t);
        if (n > 10) return false;
        const int sym = (run << 4) | n;
        s.bits(((unsigned)h.code[ac_tbl][sym] << n) | ((unsigned)t2 & ((1u << n) - 1)), h.len[ac_tbl][sym] + n);
    }
    if (prev != 63) s.bits(h.code[ac_tbl][0], h.len[ac_tbl][0]);           // EOB unless the last coefficient was coded
    return true;
}

// fh_jpeg_write_header's body and the front of jpeg_write: SOI .. the SOS header, everything in front of the first entropy-coded byte
void jpeg_write_header(const fh_jpeg_desc& o, ByteSink& s) {
    const int nc = o.ncomp;
    int tq[3] = {0, 1, 1};                                                 // libjpeg's assignment; a third table only where Cr's differs from Cb's
    if (nc == 3 && memcmp(o.comp[2].quant, o.comp[1].quant, sizeof(o.comp[1].quant)) != 0) tq[2] = 2;
    s.marker(0xD8);
    s.marker(0xE0); s.u16(16);
    for (const char* p = "JFIF"; *p; ++p) s.byte(*p);
    s.byte(0); s.byte(1); s.byte(1); s.byte(0); s.u16(1); s.u16(1); s.byte(0); s.byte(0);
    for (int i = 0; i < nc; ++i) {
        if (i == 2 && tq[2] == 1) continue;
        s.marker(0xDB); s.u16(67); s.byte(tq[i]);
        for (int k = 0; k < 64; ++k) s.byte(o.comp[i].quant[kZigzag[k]]);
    }
    s.marker(0xC0); s.u16(8 + 3 * nc); s.byte(8); s.u16(o.height); s.u16(o.width); s.byte(nc);
    for (int i = 0; i < nc; ++i) { s.byte(i + 1); s.byte((o.comp[i].h << 4) | o.comp[i].v); s.byte(tq[i]); }
    for (int t = 0; t < 4; ++t) {                                          // DC0, AC0 (, DC1, AC1): libjpeg's order
        const int idx = (t & 1) * 2 + (t >> 1);
        if (nc == 1 && (t >> 1)) continue;
        const StdHuff& h = kStdHuff[idx];
        s.marker(0xC4); s.u16(2 + 1 + 16 + h.nvals); s.byte(((t & 1) << 4) | (t >> 1));
        for (int l = 1; l <= 16; ++l) s.byte(h.bits[l]);
        for (int k = 0; k < h.nvals; ++k) s.byte(h.vals[k]);
    }
    s.marker(0xDA); s.u16(6 + 2 * nc); s.byte(nc);
    for (int i = 0; i < nc; ++i) { s.byte(i + 1); s.byte(i ? 0x11 : 0x00); }
    s.byte(0); s.byte(63); s.byte(0);
}

// fh_jpeg_write's body (the descriptor passed bad_enc_desc): false for a coefficient the baseline tables cannot code.  s.pos = the size.
bool jpeg_write(const fh_jpeg_desc& o, const int16_t* coef, ByteSink& s) {
    const int nc = o.ncomp;
    jpeg_write_header(o, s);
    int pred[3] = {0, 0, 0};
    const EncHuff& huff = enc_huff();
    const int mcux = o.comp[0].wblocks / o.comp[0].h, mcuy = o.comp[0].hblocks / o.comp[0].v;
    for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx)
            for (int i = 0; i < nc; ++i) {
                const fh_jpeg_comp& c = o.comp[i];
                for (int y = 0; y < c.v; ++y)
                    for (int x = 0; x < c.h; ++x) {
                        const int16_t* blk = coef + c.coef_off + ((size_t)(my * c.v + y) * c.wblocks + (size_t)(mx * c.h + x)) * 64;
                        if (!encode_block(s, huff, blk, pred[i], i ? 1 : 0, i ? 3 : 2)) return false;
                    }
            }
    s.flush();
    s.marker(0xD9);
    return true;
}

// fh_jpeg_scan_bits's body: jpeg_write's walk over the blocks with the counting sink; false as jpeg_write
bool jpeg_scan_bits(const fh_jpeg_desc& o, const int16_t* coef, uint32_t* bits) {
    int pred[3] = {0, 0, 0};
    const EncHuff& huff = enc_huff();
    const int mcux = o.comp[0].wblocks / o.comp[0].h, mcuy = o.comp[0].hblocks / o.comp[0].v;
    for (int my = 0; my < mcuy; ++my)
        for (int mx = 0; mx < mcux; ++mx)
            for (int i = 0; i < o.ncomp; ++i) {
                const fh_jpeg_comp& c = o.comp[i];
                for (int y = 0; y < c.v; ++y)
                    for (int x = 0; x < c.h; ++x) {
                        const int16_t* blk = coef + c.coef_off + ((size_t)(my * c.v + y) * c.wblocks + (size_t)(mx * c.h + x)) * 64;
                        BitCount n;
                        if (!encode_block(n, huff, blk, pred[i], i ? 1 : 0, i ? 3 : 2)) return false;
                        *bits++ = n.n;
                    }
            }
    return true;
}

// the blocks of the interleaved scan: every component's padded grid
size_t jpeg_scan_blocks(const fh_jpeg_desc& o) {
    size_t blocks = 0;
    for (int i = 0; i < o.ncomp; ++i) blocks += (size_t)o.comp[i].wblocks * o.comp[i].hblocks;
    return blocks;
}

// headers (at most 2 + 18 + 3 * 69 + 19 + 2 * 33 + 2 * 183 + 14 + 2 < 1024 bytes) + per block the longest codes: DC 11 + 11 bits,
// 63 AC values of 16 + 10 bits = 1660 bits < 208 bytes, every one of them stuffed
size_t jpeg_write_bound(const fh_jpeg_desc& o) {
    return 1024 + jpeg_scan_blocks(o) * 416;
}

}  // namespace

namespace fh {
// The writer's code tables for the device coder (jpeg_huff.hip): entry [t * 256 + symbol] = length << 16 | code, t = DC0, DC1, AC0, AC1
// as kStdHuff; 0 for a symbol without a code.
void jpeg_huff_codes(uint32_t* tab) {
    const EncHuff& h = enc_huff();
    for (int t = 0; t < 4; ++t)
        for (int k = 0; k < 256; ++k) tab[t * 256 + k] = (uint32_t)h.len[t][k] << 16 | h.code[t][k];
}
}  // namespace fh

extern "C" {

int fh_jpeg_quant_tables(int quality, uint16_t* luma, uint16_t* chroma) {
    if (!luma || !chroma) { fh::set_error("fh_jpeg_quant_tables: null argument"); return FH_ERR_ARG; }
    const int q = quality < 1 ? 1 : quality > 100 ? 100 : quality;         // jpeg_quality_scaling
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; ++k) {
        const int l = (kBaseLuma[k] * scale + 50) / 100, c = (kBaseChroma[k] * scale + 50) / 100;
        luma[k] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[k] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return 0;
}

int fh_jpeg_enc_desc(int width, int height, int gray, int subsampling, int quality, fh_jpeg_desc* d) {
    if (!d) { fh::set_error("fh_jpeg_enc_desc: null descriptor"); return FH_ERR_ARG; }
    if (width < 1 || height < 1 || width > 65535 || height > 65535) { fh::set_error("fh_jpeg_enc_desc: need 1 <= width, height <= 65535"); return FH_ERR_ARG; }
    if (!gray && (subsampling < 0 || subsampling > 2)) { fh::set_error("fh_jpeg_enc_desc: subsampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0)"); return FH_ERR_ARG; }
    uint16_t luma[64], chroma[64];
    fh_jpeg_quant_tables(quality, luma, chroma);
    memset(d, 0, sizeof(*d));
    d->width = d->cols = width; d->height = d->rows = height;
    d->ncomp = gray ? 1 : 3; d->color = gray ? 0 : 1; d->orientation = 1;
    d->hmax = !gray && subsampling >= 1 ? 2 : 1; d->vmax = !gray && subsampling == 2 ? 2 : 1;
    const int mcux = (width + 8 * d->hmax - 1) / (8 * d->hmax), mcuy = (height + 8 * d->vmax - 1) / (8 * d->vmax);
    for (int i = 0; i < d->ncomp; ++i) {
        fh_jpeg_comp& c = d->comp[i];
        c.h = i ? 1 : d->hmax; c.v = i ? 1 : d->vmax;
        c.wblocks = mcux * c.h; c.hblocks = mcuy * c.v;
        c.dw = (width * c.h + d->hmax - 1) / d->hmax; c.dh = (height * c.v + d->vmax - 1) / d->vmax;
        c.coef_off = d->coef_count;
        d->coef_count += (int64_t)c.wblocks * c.hblocks * 64;
        memcpy(c.quant, i ? chroma : luma, sizeof(c.quant));
    }
    return 0;
}

int fh_jpeg_enc_check(const fh_jpeg_desc* desc) {
    if (const char* bad = bad_enc_desc(desc)) { fh::set_error(std::string("fh_jpeg_enc_check: ") + bad); return FH_ERR_ARG; }
    return 0;
}

int fh_jpeg_forward(const fh_jpeg_desc* desc, const unsigned char* bgr, int step, int16_t* coef, size_t cap) {
    if (!desc || !bgr || !coef) { fh::set_error("fh_jpeg_forward: null argument"); return FH_ERR_ARG; }
    if (const char* bad = bad_enc_desc(desc)) { fh::set_error(std::string("fh_jpeg_forward: ") + bad); return FH_ERR_ARG; }
    if ((long long)step < (long long)desc->cols * 3) { fh::set_error("fh_jpeg_forward: step is smaller than cols * 3"); return FH_ERR_ARG; }
    if ((unsigned long long)desc->coef_count > cap) { fh::set_error("fh_jpeg_forward: the coefficient buffer is too small for this descriptor"); return FH_ERR_ARG; }
    return jpeg_call("fh_jpeg_forward", [&] { jpeg_forward(*desc, bgr, (size_t)step, coef); });
}

size_t fh_jpeg_write_bound(const fh_jpeg_desc* desc) {
    if (bad_enc_desc(desc)) return 0;
    return jpeg_write_bound(*desc);
}

int fh_jpeg_write(const fh_jpeg_desc* desc, const int16_t* coef, unsigned char* out, size_t cap, size_t* written) {
    if (written) *written = 0;
    if (!desc || !coef || !written || (!out && cap)) { fh::set_error("fh_jpeg_write: null argument"); return FH_ERR_ARG; }
    if (const char* bad = bad_enc_desc(desc)) { fh::set_error(std::string("fh_jpeg_write: ") + bad); return FH_ERR_ARG; }
    ByteSink s{out, cap};
    if (!jpeg_write(*desc, coef, s)) {
        fh::set_error("fh_jpeg_write: a DC difference outside +-2047 or an AC coefficient outside +-1023 has no baseline code");
        return FH_ERR_ARG;
    }
    *written = s.pos;
    if (s.pos > cap) { fh::set_error("fh_jpeg_write: the output buffer is too small (see *written)"); return FH_ERR_ARG; }
    return 0;
}

int fh_jpeg_write_header(const fh_jpeg_desc* desc, unsigned char* out, size_t cap, size_t* written) {
    if (written) *written = 0;
    if (!desc || !written || (!out && cap)) { fh::set_error("fh_jpeg_write_header: null argument"); return FH_ERR_ARG; }
    if (const char* bad = bad_enc_desc(desc)) { fh::set_error(std::string("fh_jpeg_write_header: ") + bad); return FH_ERR_ARG; }
    ByteSink s{out, cap};
    jpeg_write_header(*desc, s);
    *written = s.pos;
    if (s.pos > cap) { fh::set_error("fh_jpeg_write_header: the output buffer is too small (see *written)"); return FH_ERR_ARG; }
    return 0;
}

int fh_jpeg_scan_bits(const fh_jpeg_desc* desc, const int16_t* coef, uint32_t* bits, size_t cap) {
    if (!desc || !coef || (!bits && cap)) { fh::set_error("fh_jpeg_scan_bits: null argument"); return FH_ERR_ARG; }
    if (const char* bad = bad_enc_desc(desc)) { fh::set_error(std::string("fh_jpeg_scan_bits: ") + bad); return FH_ERR_ARG; }
    if (jpeg_scan_blocks(*desc) > cap) { fh::set_error("fh_jpeg_scan_bits: the output holds fewer entries than the scan has blocks"); return FH_ERR_ARG; }
    if (!jpeg_scan_bits(*desc, coef, bits)) {
        fh::set_error("fh_jpeg_scan_bits: a DC difference outside +-2047 or an AC coefficient outside +-1023 has no baseline code");
        return FH_ERR_ARG;
    }
    return 0;
}

int fh_imwrite_jpeg(const char* path, const unsigned char* bgr, int rows, int cols, int step, int quality, int subsampling) {
    if (!path || !bgr) { fh::set_error("fh_imwrite_jpeg: null argument"); return FH_ERR_ARG; }
    fh_jpeg_desc d;
    if (rows < 1 || cols < 1 || fh_jpeg_enc_desc(cols, rows, 0, subsampling, quality, &d) != 0) {
        if (rows < 1 || cols < 1) fh::set_error("fh_imwrite_jpeg: empty image");
        return FH_ERR_ARG;
    }
    if ((long long)step < (long long)cols * 3) { fh::set_error("fh_imwrite_jpeg: step is smaller than cols * 3"); return FH_ERR_ARG; }
    size_t n = 0;
    std::vector<unsigned char> bytes;
    const int rc = jpeg_call("fh_imwrite_jpeg", [&] {
        std::vector<int16_t> coef((size_t)d.coef_count);
        jpeg_forward(d, bgr, (size_t)step, coef.data());
        bytes.resize(jpeg_write_bound(d));
        ByteSink s{bytes.data(), bytes.size()};
        if (!jpeg_write(d, coef.data(), s) || s.pos > bytes.size()) fail("fh_imwrite_jpeg: the coefficients have no baseline code");
        n = s.pos;
    });
    if (rc != 0) return rc;
    FILE* f = fopen(path, "wb");
    if (!f) { fh::set_error(std::string("fh_imwrite_jpeg: cannot open ") + path); return -1; }
    const bool ok = fwrite(bytes.data(), 1, n, f) == n;
    if (fclose(f) != 0 || !ok) { fh::set_error(std::string("fh_imwrite_jpeg: cannot write ") + path); return -1; }
    return 0;
}

int fh_jpeg_header(const unsigned char* bytes, size_t n, fh_jpeg_desc* desc) {
    if (!bytes || !desc) { fh::set_error("fh_jpeg_header: null argument"); return -1; }
    return jpeg_call("fh_jpeg_header", [&] {
        if (!is_jpeg(bytes, n)) fail("JPEG: no SOI");
        jpeg_parse(bytes, n, desc, nullptr, 0, true);
    });
}

int fh_jpeg_entropy(const unsigned char* bytes, size_t n, fh_jpeg_desc* desc, int16_t* coef, size_t cap) {
    if (!bytes || !desc || !coef) { fh::set_error("fh_jpeg_entropy: null argument"); return -1; }
    return jpeg_call("fh_jpeg_entropy", [&] {
        if (!is_jpeg(bytes, n)) fail("JPEG: no SOI");
        jpeg_parse(bytes, n, desc, coef, cap, false);
    });
}

int fh_jpeg_desc_check(const fh_jpeg_desc* desc) {
    if (const char* bad = bad_desc(desc)) { fh::set_error(std::string("fh_jpeg_desc_check: ") + bad); return FH_ERR_ARG; }
    return 0;
}

int fh_jpeg_reconstruct(const fh_jpeg_desc* desc, const int16_t* coef, unsigned char* bgr, int step) {
    if (!desc || !coef || !bgr) { fh::set_error("fh_jpeg_reconstruct: null argument"); return FH_ERR_ARG; }
    if (const char* bad = bad_desc(desc)) { fh::set_error(std::string("fh_jpeg_reconstruct: ") + bad); return FH_ERR_ARG; }
    if ((long long)step < (long long)desc->cols * 3) { fh::set_error("fh_jpeg_reconstruct: step is smaller than cols * 3"); return FH_ERR_ARG; }
    return jpeg_call("fh_jpeg_reconstruct", [&] { jpeg_reconstruct(*desc, coef, bgr, (size_t)step); });
}

int fh_image_decode(const unsigned char* bytes, size_t n, unsigned char** bgr, int* rows, int* cols) {
    if (!bytes || !bgr || !rows || !cols) { fh::set_error("fh_image_decode: null argument"); return -1; }
    *bgr = nullptr; *rows = *cols = 0;
    if (is_jpeg(bytes, n)) {                                      // fh_jpeg_entropy, then fh_jpeg_reconstruct
        unsigned char* out = nullptr;
        const int rc = jpeg_call("fh_image_decode", [&] {
            fh_jpeg_desc o;
            jpeg_parse(bytes, n, &o, nullptr, 0, true);
            const std::unique_ptr<int16_t[]> coef(new int16_t[(size_t)o.coef_count]);
            jpeg_parse(bytes, n, &o, coef.get(), (size_t)o.coef_count, false);
            const size_t size = (size_t)o.rows * o.cols * 3;
            out = static_cast<unsigned char*>(malloc(size ? size : 1));
            if (!out) fail("fh_image_decode: out of memory");
            jpeg_reconstruct(o, coef.get(), out, (size_t)o.cols * 3);
            *rows = o.rows; *cols = o.cols;
        });
        if (rc != 0) { free(out); *rows = *cols = 0; return -1; }
        *bgr = out;
        return 0;
    }
    try {
        Image img = decode_any(bytes, n);
        unsigned char* out = static_cast<unsigned char*>(malloc(img.bgr.size() ? img.bgr.size() : 1));
        if (!out) { fh::set_error("fh_image_decode: out of memory"); return -1; }
        memcpy(out, img.bgr.data(), img.bgr.size());
        *bgr = out; *rows = img.rows; *cols = img.cols;
        return 0;
    } catch (const DecodeError& e) {
        fh::set_error(e.msg);
    } catch (const std::exception& e) {
        fh::set_error(std::string("fh_image_decode: ") + e.what());
    }
    return -1;
}

int fh_imread(const char* path, unsigned char** bgr, int* rows, int* cols) {
    if (!path || !bgr || !rows || !cols) { fh::set_error("fh_imread: null argument"); return -1; }
    *bgr = nullptr; *rows = *cols = 0;
    FILE* f = fopen(path, "rb");
    if (!f) { fh::set_error(std::string("fh_imread: cannot open ") + path); return -1; }
    std::vector<unsigned char> buf;
    unsigned char tmp[65536];
    size_t got;
    while ((got = fread(tmp, 1, sizeof(tmp), f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
    fclose(f);
    return fh_image_decode(buf.data(), buf.size(), bgr, rows, cols);
}

void fh_image_free(unsigned char* bgr) { free(bgr); }

}  // extern "C"
