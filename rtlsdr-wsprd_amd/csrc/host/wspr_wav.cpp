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

// The canonical 44-byte header (RIFF, "fmt " of 16 bytes, data) and the samples, little-endian whatever the host is.
int write_wav_file(const char* filename, const int16_t* pcm, size_t nsamp) {
    if (!filename || (!pcm && nsamp) || nsamp > (0xffffffffu - 36u) / 2u) return -1;   // the size fields are 32 bits
    FILE* fd = fopen(filename, "wb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return -1; }
    const uint32_t data = (uint32_t)(nsamp * 2), rate = 12000;
    unsigned char hd[44];
    auto put32 = [&](int at, uint32_t v) { for (int b = 0; b < 4; ++b) hd[at + b] = (unsigned char)(v >> (8 * b)); };
    auto put16 = [&](int at, uint32_t v) { hd[at] = (unsigned char)v; hd[at + 1] = (unsigned char)(v >> 8); };
    memcpy(hd, "RIFF", 4);      put32(4, 36u + data);
    memcpy(hd + 8, "WAVEfmt ", 8);  put32(16, 16);
    put16(20, 1);               put16(22, 1);               // PCM, one channel
    put32(24, rate);            put32(28, rate * 2);        // samples and bytes per second
    put16(32, 2);               put16(34, 16);              // bytes per frame, bits per sample
    memcpy(hd + 36, "data", 4); put32(40, data);
    bool ok = fwrite(hd, 1, sizeof hd, fd) == sizeof hd;
    unsigned char buf[4096];
    for (size_t done = 0; ok && done < nsamp;) {
        const size_t n = nsamp - done < sizeof buf / 2 ? nsamp - done : sizeof buf / 2;
        for (size_t i = 0; i < n; ++i) {
            const uint16_t v = (uint16_t)pcm[done + i];
            buf[2 * i] = (unsigned char)v;
            buf[2 * i + 1] = (unsigned char)(v >> 8);
        }
        ok = fwrite(buf, 2, n, fd) == n;
        done += n;
    }
    if (fclose(fd) != 0) ok = false;
    return ok ? 0 : -1;
}
}  // namespace wspr
