// Host half of the JPEG decoder: marker parsing and Huffman (entropy) decoding of baseline streams into quantised DCT
// coefficients.  Plain C++17, no HIP, no globals, re-entrant: jpeg.hip wraps it as ssd_jpeg_info / ssd_jpeg_entropy_decode, and
// tools_dev/jpeg_host_check.cpp compiles it alone under the host sanitizers.  include/ssd_hip.h states what is served, what is
// refused and the record layout; the numpy twin is tests/jpeg_oracle.py.
//
// Every read goes through a length check against n; every coefficient write is inside the ncoef elements checked against the
// caller's capacity before the scan is touched.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace ssd_jpeg {

enum { OK = 0, ERR_VALUE = -2, ERR_WORKSPACE = -3, ERR_UNSUPPORTED = -5 };          // = SSD_OK, SSD_ERR_* of ssd_hip.h
enum { REC_WIDTH = 0, REC_HEIGHT = 1, REC_NCOMP = 2, REC_KIND = 3, REC_BLOCKS_W = 4, REC_BLOCKS_H = 7, REC_NCOEF = 10,
       REC_RESTART = 11, REC_COEF_OFF = 12, REC_QT = 16, REC_WORDS = 208 };         // = SSD_JPEG_* of ssd_hip.h
enum { KIND_GREY = 0, KIND_444 = 1, KIND_422 = 2, KIND_420 = 3 };

static const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Huff {
    bool present;
    uint16_t fast[512];          // 9-bit prefix -> (length << 8) | symbol, 0 = longer than 9 bits or no such code
    int32_t maxcode[18];         // largest code of each length, -1 = none
    int32_t valoff[17];          // index of the first symbol of a length minus its first code
    uint8_t vals[256];
};

struct Frame {
    int width, height, ncomp, kind, restart;
    int hs[3], vs[3], tq[3], td[3], ta[3];
    int blocks_w[3], blocks_h[3], mcus_x, mcus_y;
    long long coef_off[3], ncoef;
    bool have_qt[4];
    uint16_t qt[4][64];          // natural order
    Huff dc[4], ac[4];
    size_t scan;                 // offset of the first entropy-coded byte
};

// Build the decoding tables of one DHT entry (counts[1..16], symbols).  false: over-subscribed code.
static inline bool build_huff(Huff& h, const uint8_t* counts, const uint8_t* symbols, int total) {
    memset(&h, 0, sizeof(h));
    memcpy(h.vals, symbols, (size_t)total);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int cnt = counts[len - 1];
        h.valoff[len] = k - code;
        if (cnt) {
            if (code + cnt > (1 << len)) return false;
            if (len <= 9)
                for (int i = 0; i < cnt; ++i) {
                    const int first = (code + i) << (9 - len);
                    for (int j = 0; j < (1 << (9 - len)); ++j) h.fast[first + j] = (uint16_t)((len << 8) | symbols[k + i]);
                }
            code += cnt;
            k += cnt;
            h.maxcode[len] = code - 1;
        } else {
            h.maxcode[len] = -1;
        }
        code <<= 1;
    }
    h.maxcode[17] = 0x7fffffff;
    h.present = true;
    return true;
}

static inline int be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Markers up to and including the scan header.  Fills f; coef_off relative to the image's first coefficient.
static inline int parse(const uint8_t* d, size_t n, Frame& f) {
    memset(&f, 0, sizeof(f));
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return ERR_VALUE;
    size_t p = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int adobe_transform = 0, ids[3] = {0, 0, 0};
    for (;;) {
        if (p + 2 > n) return ERR_VALUE;                       // ran out before a scan
        if (d[p] != 0xFF) return ERR_VALUE;
        while (p + 1 < n && d[p + 1] == 0xFF) ++p;             // fill bytes
        if (p + 2 > n) return ERR_VALUE;
        const int m = d[p + 1];
        p += 2;
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // parameterless
        if (m == 0xD9) return ERR_VALUE;                       // EOI before any scan
        if (p + 2 > n) return ERR_VALUE;
        const int len = be16(d + p);
        if (len < 2 || p + (size_t)len > n) return ERR_VALUE;  // segment length past the end
        const uint8_t* s = d + p + 2;
        const int sl = len - 2;
        if (m == 0xC0) {
            if (have_sof || sl < 6) return ERR_VALUE;
            if (s[0] != 8) return ERR_UNSUPPORTED;
            f.height = be16(s + 1);
            f.width = be16(s + 3);
            f.ncomp = s[5];
            if (f.ncomp != 1 && f.ncomp != 3) return f.ncomp == 0 ? ERR_VALUE : ERR_UNSUPPORTED;
            if (sl < 6 + 3 * f.ncomp) return ERR_VALUE;
            if (f.width == 0 || f.height == 0) return ERR_VALUE;
            for (int c = 0; c < f.ncomp; ++c) {
                ids[c] = s[6 + 3 * c];
                f.hs[c] = s[7 + 3 * c] >> 4;
                f.vs[c] = s[7 + 3 * c] & 15;
                f.tq[c] = s[8 + 3 * c];
                if (f.hs[c] < 1 || f.hs[c] > 4 || f.vs[c] < 1 || f.vs[c] > 4 || f.tq[c] > 3) return ERR_VALUE;
            }
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8)) {
            return ERR_UNSUPPORTED;                            // extended / progressive / lossless / arithmetic frames, DAC
        } else if (m == 0xC4) {
            int q = 0;
            while (q < sl) {
                if (q + 17 > sl) return ERR_VALUE;
                const int tc = s[q] >> 4, th = s[q] & 15;
                if (tc > 1 || th > 3) return ERR_VALUE;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
                if (total > 256 || q + 17 + total > sl) return ERR_VALUE;
                if (!build_huff(tc ? f.ac[th] : f.dc[th], s + q + 1, s + q + 17, total)) return ERR_VALUE;
                q += 17 + total;
            }
        } else if (m == 0xDB) {
            int q = 0;
            while (q < sl) {
                const int pq = s[q] >> 4, tq = s[q] & 15;
                if (tq > 3 || pq > 1) return ERR_VALUE;
                if (pq == 1) return ERR_UNSUPPORTED;           // 16-bit table
                if (q + 65 > sl) return ERR_VALUE;
                for (int i = 0; i < 64; ++i) f.qt[tq][ZIGZAG[i]] = s[q + 1 + i];
                f.have_qt[tq] = true;
                q += 65;
            }
        } else if (m == 0xDD) {
            if (sl < 2) return ERR_VALUE;
            f.restart = be16(s);
        } else if (m == 0xE0) {
            if (sl >= 5 && memcmp(s, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (sl >= 12 && memcmp(s, "Adobe", 5) == 0) { adobe = true; adobe_transform = s[11]; }
        } else if (m == 0xDA) {
            if (!have_sof) return ERR_VALUE;
            if (sl < 1) return ERR_VALUE;
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl < 4 + 2 * ns) return ERR_VALUE;
            if (ns != f.ncomp) return ERR_UNSUPPORTED;         // one scan that holds every component, or nothing
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != ids[c]) return ERR_UNSUPPORTED;
                f.td[c] = s[2 + 2 * c] >> 4;
                f.ta[c] = s[2 + 2 * c] & 15;
                if (f.td[c] > 3 || f.ta[c] > 3) return ERR_VALUE;
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return ERR_VALUE;   // Ss, Se, Ah/Al of baseline
            p += (size_t)len;
            break;
        } else if (m == 0xDC) {
            return ERR_UNSUPPORTED;                            // DNL: the height arrives behind the scan
        }                                                      // APPn, COM and everything else with a length: skipped
        p += (size_t)len;
    }
    f.scan = p;
    if (f.ncomp == 1) {
        f.kind = KIND_GREY;
        f.hs[0] = f.vs[0] = 1;                                 // a single component is never interleaved
    } else {
        if (f.hs[1] != 1 || f.vs[1] != 1 || f.hs[2] != 1 || f.vs[2] != 1) return ERR_UNSUPPORTED;
        if (f.hs[0] == 1 && f.vs[0] == 1) f.kind = KIND_444;
        else if (f.hs[0] == 2 && f.vs[0] == 1) f.kind = KIND_422;
        else if (f.hs[0] == 2 && f.vs[0] == 2) f.kind = KIND_420;
        else return ERR_UNSUPPORTED;
        // libjpeg's colour-space rule: JFIF means YCbCr; else Adobe's transform flag; else the component ids
        bool rgb = false;
        if (jfif) rgb = false;
        else if (adobe) rgb = adobe_transform == 0;
        else rgb = ids[0] == 'R' && ids[1] == 'G' && ids[2] == 'B';
        if (rgb) return ERR_UNSUPPORTED;
    }
    f.mcus_x = (f.width + 8 * f.hs[0] - 1) / (8 * f.hs[0]);
    f.mcus_y = (f.height + 8 * f.vs[0] - 1) / (8 * f.vs[0]);
    f.ncoef = 0;
    for (int c = 0; c < f.ncomp; ++c) {
        if (!f.have_qt[f.tq[c]] || !f.dc[f.td[c]].present || !f.ac[f.ta[c]].present) return ERR_VALUE;
        f.blocks_w[c] = f.mcus_x * f.hs[c];
        f.blocks_h[c] = f.mcus_y * f.vs[c];
        f.coef_off[c] = f.ncoef;
        f.ncoef += 64LL * f.blocks_w[c] * f.blocks_h[c];
    }
    if (f.ncoef > 0x7fffffffLL) return ERR_UNSUPPORTED;
    return OK;
}

static inline void fill_record(const Frame& f, int32_t* rec) {
    memset(rec, 0, sizeof(int32_t) * REC_WORDS);
    rec[REC_WIDTH] = f.width;
    rec[REC_HEIGHT] = f.height;
    rec[REC_NCOMP] = f.ncomp;
    rec[REC_KIND] = f.kind;
    rec[REC_NCOEF] = (int32_t)f.ncoef;
    rec[REC_RESTART] = f.restart;
    for (int c = 0; c < f.ncomp; ++c) {
        rec[REC_BLOCKS_W + c] = f.blocks_w[c];
        rec[REC_BLOCKS_H + c] = f.blocks_h[c];
        rec[REC_COEF_OFF + c] = (int32_t)f.coef_off[c];
        for (int i = 0; i < 64; ++i) rec[REC_QT + 64 * c + i] = f.qt[f.tq[c]][i];
    }
}

// MSB-first bit reader over the entropy-coded segment.  Real bytes are taken up to the next marker (FF followed by anything
// but 00 / FF) or the end of the data; past that point zero bytes are supplied and counted in `fake`, and a consumer that has
// eaten into them (cnt < fake) has run past the data.
struct Bits {
    const uint8_t* d;
    size_t p, n;
    uint64_t acc;
    int cnt, fake;
    bool marker;                 // p stands on the FF of a marker

    void reset(size_t at) { p = at; acc = 0; cnt = 0; fake = 0; marker = false; }
    void fill() {
        while (cnt <= 56) {
            if (!marker && p < n) {
                const uint8_t b = d[p];
                if (b != 0xFF) { acc = (acc << 8) | b; cnt += 8; ++p; continue; }
                if (p + 1 >= n) { p = n; continue; }                           // a lone FF at the very end: the data is over
                if (d[p + 1] == 0x00) { acc = (acc << 8) | 0xFF; cnt += 8; p += 2; continue; }
                if (d[p + 1] == 0xFF) { ++p; continue; }                       // fill byte
                marker = true;
                continue;
            }
            acc <<= 8;
            cnt += 8;
            fake += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)((acc >> (cnt - k)) & ((1u << k) - 1u)); }
    void skip(int k) { cnt -= k; }
    bool overrun() const { return cnt < fake; }
};

// One Huffman symbol, or -1 for a code that is not in the table.  Needs cnt >= 16.
static inline int decode_symbol(Bits& b, const Huff& h) {
    const unsigned e = h.fast[b.peek(9)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255u); }
    const int look = (int)b.peek(16);
    for (int len = 10; len <= 16; ++len) {
        const int code = look >> (16 - len);
        if (code <= h.maxcode[len]) { b.skip(len); return h.vals[(code + h.valoff[len]) & 255]; }
    }
    return -1;
}

static inline int extend(Bits& b, int s) {                       // s in 1..15; needs cnt >= s
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

static inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, uint32_t& pred, int16_t* out) {
    if (b.cnt < 32) b.fill();
    int s = decode_symbol(b, dc);
    if (s < 0 || s > 15) return ERR_VALUE;
    if (s) pred += (uint32_t)extend(b, s);
    out[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        if (b.cnt < 32) b.fill();
        const int rs = decode_symbol(b, ac);
        if (rs < 0) return ERR_VALUE;
        const int r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (r != 15) break;                                  // EOB
            k += 16;
            if (k > 64) return ERR_VALUE;
            continue;
        }
        k += r;
        if (k > 63) return ERR_VALUE;                            // coefficient index past 63
        out[ZIGZAG[k]] = (int16_t)extend(b, s);
        ++k;
    }
    return b.overrun() ? ERR_VALUE : OK;
}

// The scan of a parsed frame -> coef[0 .. f.ncoef).  The caller has checked the capacity.
static inline int decode_scan(const uint8_t* d, size_t n, const Frame& f, int16_t* coef) {
    memset(coef, 0, sizeof(int16_t) * (size_t)f.ncoef);
    Bits b;
    b.d = d;
    b.n = n;
    b.reset(f.scan);
    uint32_t pred[3] = {0, 0, 0};
    const long long mcus = (long long)f.mcus_x * f.mcus_y;
    long long done = 0;
    int next_rst = 0;
    for (int my = 0; my < f.mcus_y; ++my)
        for (int mx = 0; mx < f.mcus_x; ++mx) {
            for (int c = 0; c < f.ncomp; ++c)
                for (int v = 0; v < f.vs[c]; ++v)
                    for (int h = 0; h < f.hs[c]; ++h) {
                        const long long blk = (long long)(my * f.vs[c] + v) * f.blocks_w[c] + (mx * f.hs[c] + h);
                        const int rc = decode_block(b, f.dc[f.td[c]], f.ac[f.ta[c]], pred[c], coef + f.coef_off[c] + 64 * blk);
                        if (rc != OK) return rc;
                    }
            ++done;
            if (f.restart && done % f.restart == 0 && done < mcus) {
                b.fill();                                        // to the marker: at most 7 padding bits may be left
                if (!b.marker || b.overrun() || b.cnt - b.fake >= 8) return ERR_VALUE;
                if (b.p + 1 >= n || d[b.p + 1] != 0xD0 + next_rst) return ERR_VALUE;
                next_rst = (next_rst + 1) & 7;
                b.reset(b.p + 2);
                pred[0] = pred[1] = pred[2] = 0;
            }
        }
    b.fill();
    if (b.overrun()) return ERR_VALUE;
    size_t q = b.p;                                              // the first marker behind the last MCU must be EOI
    while (q + 1 < n) {                                          // (b.marker: q stands on it, q + 1 < n was checked in fill)
        if (d[q] == 0xFF && d[q + 1] != 0x00 && d[q + 1] != 0xFF) return d[q + 1] == 0xD9 ? OK : ERR_VALUE;
        q += (d[q] == 0xFF && d[q + 1] == 0x00) ? 2 : 1;
    }
    return ERR_VALUE;
}

static inline int info(const void* data, size_t n, int32_t* rec) {
    if (!data || !rec) return ERR_VALUE;
    Frame f;
    const int rc = parse(static_cast<const uint8_t*>(data), n, f);
    if (rc == OK) fill_record(f, rec);
    return rc;
}

static inline int entropy_decode(const void* data, size_t n, int16_t* coef, size_t capacity, int32_t* rec) {
    if (!data || !coef) return ERR_VALUE;
    Frame f;
    int rc = parse(static_cast<const uint8_t*>(data), n, f);
    if (rc != OK) return rc;
    if ((unsigned long long)f.ncoef > (unsigned long long)capacity) return ERR_WORKSPACE;
    rc = decode_scan(static_cast<const uint8_t*>(data), n, f, coef);
    if (rc == OK && rec) fill_record(f, rec);
    return rc;
}

}  // namespace ssd_jpeg
