// Stand-alone check of csrc/jpeg_host.h under the host sanitizers (no HIP, no Python):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I ssd-object-detection_amd/csrc \
//       tools_dev/jpeg_host_check.cpp -o jpeg_host_check && ./jpeg_host_check tests/golden/jpeg/*.jpg
// Every file is decoded from a heap copy of exactly its length into a heap buffer of exactly the coefficient count, so a read
// or write one byte outside either is the sanitizer's to report.  Then the corrupted variants: the stream cut at (nearly)
// every length, bytes inverted one at a time, restart markers renumbered, and a capacity one short.  Prints one line per file:
//   <file> status <s> ncoef <n> variants <v> ok <a> value <b> unsupported <c>
// Exit status 1 if a variant returns anything but OK, VALUE or UNSUPPORTED, or a short capacity anything but WORKSPACE.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_host.h"

namespace {

struct Tally { long ok = 0, value = 0, unsupported = 0, other = 0; };

int decode_exact(const std::vector<unsigned char>& bytes, size_t n, Tally* tally) {
    unsigned char* data = static_cast<unsigned char*>(std::malloc(n ? n : 1));      // exactly n bytes (1 for the empty stream)
    if (n) std::memcpy(data, bytes.data(), n);
    int32_t rec[ssd_jpeg::REC_WORDS];
    int rc = ssd_jpeg::info(data, n, rec);
    if (rc == ssd_jpeg::OK) {
        const size_t ncoef = (size_t)rec[ssd_jpeg::REC_NCOEF];
        int16_t* coef = static_cast<int16_t*>(std::malloc(ncoef * sizeof(int16_t)));
        int32_t rec2[ssd_jpeg::REC_WORDS];
        rc = ssd_jpeg::entropy_decode(data, n, coef, ncoef, rec2);
        if (rc == ssd_jpeg::OK && std::memcmp(rec, rec2, sizeof(rec)) != 0) rc = 99;   // the two entry points must agree
        std::free(coef);
    }
    std::free(data);
    if (tally) {
        if (rc == ssd_jpeg::OK) ++tally->ok;
        else if (rc == ssd_jpeg::ERR_VALUE) ++tally->value;
        else if (rc == ssd_jpeg::ERR_UNSUPPORTED) ++tally->unsupported;
        else ++tally->other;
    }
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    int failures = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) { std::printf("%s: cannot open\n", argv[a]); return 2; }
        std::vector<unsigned char> bytes;
        unsigned char chunk[4096];
        size_t got;
        while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + got);
        std::fclose(f);
        const size_t n = bytes.size();
        const int status = decode_exact(bytes, n, nullptr);
        int32_t rec[ssd_jpeg::REC_WORDS] = {0};
        long ncoef = 0;
        if (status == ssd_jpeg::OK) {
            ssd_jpeg::info(bytes.data(), n, rec);
            ncoef = rec[ssd_jpeg::REC_NCOEF];
            std::vector<int16_t> small((size_t)ncoef);                       // capacity one short: refused, nothing written
            if (ssd_jpeg::entropy_decode(bytes.data(), n, small.data(), (size_t)ncoef - 1, nullptr) != ssd_jpeg::ERR_WORKSPACE) ++failures;
        }
        Tally t;
        long variants = 0;
        const size_t step = n <= 2048 ? 1 : 7;
        for (size_t cut = 0; cut < n; cut += step, ++variants) decode_exact(bytes, cut, &t);          // truncations
        for (size_t i = 0; i < n; i += step, ++variants) {                                            // one inverted byte
            std::vector<unsigned char> v(bytes);
            v[i] ^= 0xFF;
            decode_exact(v, n, &t);
        }
        for (size_t i = 0; i + 1 < n; ++i)                                                            // a wrong restart marker
            if (bytes[i] == 0xFF && bytes[i + 1] >= 0xD0 && bytes[i + 1] <= 0xD7) {
                std::vector<unsigned char> v(bytes);
                v[i + 1] = (unsigned char)(0xD0 + ((bytes[i + 1] - 0xD0 + 3) & 7));
                decode_exact(v, n, &t);
                ++variants;
            }
        std::printf("%s status %d ncoef %ld variants %ld ok %ld value %ld unsupported %ld\n", argv[a], status, ncoef, variants, t.ok,
                    t.value, t.unsupported);
        if (t.other) ++failures;
    }
    return failures ? 1 : 0;
}
