// RIFF/WAVE reader (wspr_read_wav_file): the recordings of a receiver farm, one two-minute slot of 12 000 Hz 16-bit mono
// audio per file.  The file is untrusted: every length is read from the file and checked against what the file really
// holds; nothing is allocated from a length field, and nothing is written past `cap` samples.
#include "wspr_wav.h"

#include <cstdio>
#include <cstring>

namespace wspr {
namespace {
uint32_t le32(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
uint32_t le16(const unsigned char* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

// skips n bytes of a stream that need not be seekable to its end: false if the file ends first
bool skip_bytes(FILE* fd, uint64_t n) {
    unsigned char buf[4096];
    while (n > 0) {
        const size_t want = n < sizeof buf ? (size_t)n : sizeof buf;
        const size_t got = fread(buf, 1, want, fd);
        if (got == 0) return false;
        n -= got;
    }
    return true;
}

size_t read_chunks(FILE* fd, int16_t* pcm, size_t cap) {
    unsigned char hd[12];
    if (fread(hd, 1, 12, fd) != 12 || memcmp(hd, "RIFF", 4) != 0 || memcmp(hd + 8, "WAVE", 4) != 0) return 0;
    bool have_fmt = false;
    for (;;) {                                                  // the chunks in file order; the RIFF size field is not trusted
        unsigned char ck[8];
        if (fread(ck, 1, 8, fd) != 8) return 0;                 // the file ended without a data chunk
        const uint32_t size = le32(ck + 4);
        if (memcmp(ck, "fmt ", 4) == 0) {
            unsigned char f[16];
            if (size < 16 || fread(f, 1, 16, fd) != 16) return 0;
            const bool ok = le16(f) == 1 && le16(f + 2) == 1 && le32(f + 4) == 12000 && le16(f + 12) == 2 && le16(f + 14) == 16;
            if (!ok) return 0;
            have_fmt = true;
            if (!skip_bytes(fd, (uint64_t)(size - 16) + (size & 1))) return 0;      // an extension, the pad byte
        } else if (memcmp(ck, "data", 4) == 0) {
            if (!have_fmt) return 0;                            // samples of an unknown format
            size_t want = (size_t)(size / 2);
            if (want > cap) want = cap;
            size_t got = 0;
            unsigned char buf[4096];
            while (got < want) {                                // a short data chunk yields what the file holds
                const size_t n = (want - got) * 2 < sizeof buf ? (want - got) * 2 : sizeof buf;
                const size_t r = fread(buf, 1, n, fd);
                for (size_t i = 0; i + 1 < r; i += 2) pcm[got++] = (int16_t)(uint16_t)le16(buf + i);
                if (r < n) break;
            }
            return got;
        } else {
            if (!skip_bytes(fd, (uint64_t)size + (size & 1))) return 0;             // LIST and the like; odd sizes are padded
        }
    }
}
}  // namespace

size_t read_wav_file(const char* filename, int16_t* pcm, size_t cap) {
    if (!filename || (!pcm && cap)) return 0;
    FILE* fd = fopen(filename, "rb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    const size_t n = read_chunks(fd, pcm, cap);
    fclose(fd);
    return n;
}
}  // namespace wspr
