// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): recorded-file formats, the frame time
// and the spot / report texts.  Host code only.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "wspr_pipeline.h"
#include "wspr_wav.h"

namespace {
// RFC 3986 unreserved characters pass, everything else is %XX (what curl_easy_escape does)
std::string url_escape(const char* s) {
    static const char hex[] = "0123456789ABCDEF";
    std::string o;
    for (const unsigned char* p = reinterpret_cast<const unsigned char*>(s); *p; ++p) {
        if (isalnum(*p) || *p == '-' || *p == '.' || *p == '_' || *p == '~') o.push_back((char)*p);
        else { o.push_back('%'); o.push_back(hex[*p >> 4]); o.push_back(hex[*p & 15]); }
    }
    return o;
}

// max-abs normalisation to 0.5 of the first n samples, as every reader of the reference does
// (rtlsdr_wsprd.c:574-589, :649-664)
void normalise_host(float* I, float* Q, int n) {
    float peak = 1e-24f;
    for (int i = 0; i < n; ++i) {
        const float a = fabsf(I[i]), b = fabsf(Q[i]);
        if (a > peak) peak = a;
        if (b > peak) peak = b;
    }
    const float scale = (float)(0.5 / (double)peak);
    for (int i = 0; i < n; ++i) { I[i] *= scale; Q[i] *= scale; }
}
int load_interleaved(FILE* fd, float* I, float* Q) {
    std::vector<float> buf(2 * (size_t)wspr::kMaxSamples);
    const int nread = (int)fread(buf.data(), sizeof(float), buf.size(), fd);
    const int n = nread / 2;
    for (int i = 0; i < n; ++i) { I[i] = buf[2 * i]; Q[i] = -buf[2 * i + 1]; }   // Q sign: wsprsim convention
    normalise_host(I, Q, n);
    return n;
}
}  // namespace

extern "C" {

void wspr_frame_time(long unixtime_now, int* year, int* month, int* day, int* hour, int* minute) {   // :307-310
    time_t t = (time_t)unixtime_now - 120 + 1;
    struct tm g;
    gmtime_r(&t, &g);
    if (year) *year = g.tm_year + 1900;
    if (month) *month = g.tm_mon + 1;
    if (day) *day = g.tm_mday;
    if (hour) *hour = g.tm_hour;
    if (minute) *minute = g.tm_min;
}

// readRawIQfile(), rtlsdr_wsprd.c:555-592: interleaved float32 I/Q, Q negated, normalised.
// I/Q must hold 45000 floats; returns the number of complex samples read (0 on error).
int wspr_read_iq_file(const char* filename, float* I, float* Q) {
    FILE* fd = fopen(filename, "rb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    const int n = load_interleaved(fd, I, Q);
    fclose(fd);
    return n;
}

// readC2file(), rtlsdr_wsprd.c:620-667: 14-byte name, int type, double dial frequency, then the
// same interleaved payload.  *dial_hz receives the header frequency (the reference stores it in
// rx_options.dialfreq, :637).
int wspr_read_c2_file(const char* filename, float* I, float* Q, double* dial_hz) {
    FILE* fd = fopen(filename, "rb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    char name[15];
    int type = 0;
    double frequency = 0.0;
    size_t got = fread(name, sizeof(char), 14, fd);
    got += fread(&type, sizeof(int), 1, fd);
    got += fread(&frequency, sizeof(double), 1, fd);
    (void)got;
    if (dial_hz) *dial_hz = frequency;
    const int n = load_interleaved(fd, I, Q);
    fclose(fd);
    return n;
}

// One slot of 12 000 Hz 16-bit mono audio (the parser, plain C++: wspr_wav.cpp)
size_t wspr_read_wav_file(const char* filename, int16_t* pcm, size_t cap) { return wspr::read_wav_file(filename, pcm, cap); }
int wspr_write_wav_file(const char* filename, const int16_t* pcm, size_t nsamp) { return wspr::write_wav_file(filename, pcm, nsamp); }

// writeRawIQfile(), rtlsdr_wsprd.c:595-617: always 45000 complex samples, Q negated.
int wspr_write_iq_file(const char* filename, const float* I, const float* Q) {
    FILE* fd = fopen(filename, "wb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    std::vector<float> buf(2 * (size_t)wspr::kMaxSamples);
    for (int i = 0; i < wspr::kMaxSamples; ++i) { buf[2 * i] = I[i]; buf[2 * i + 1] = -Q[i]; }
    const size_t nw = fwrite(buf.data(), sizeof(float), buf.size(), fd);
    fclose(fd);
    if (nw != buf.size()) { fprintf(stderr, "Cannot write all the data!\n"); return 0; }
    return wspr::kMaxSamples;
}

// What wspr_read_c2_file() reads (readC2file(), rtlsdr_wsprd.c:620-667; the reference has no writer for it): the file's base
// name in 14 bytes (cut or padded with zeros), int type 2, the dial frequency as a double, then writeRawIQfile()'s payload.
int wspr_write_c2_file(const char* filename, const float* I, const float* Q, double dial_hz) {
    if (!filename || !I || !Q) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    FILE* fd = fopen(filename, "wb");
    if (!fd) { fprintf(stderr, "Cannot open data file...\n"); return 0; }
    const char* base = strrchr(filename, '/');
    base = base ? base + 1 : filename;
    char name[14] = {0};
    memcpy(name, base, std::min<size_t>(strlen(base), sizeof name));
    const int type = 2;
    std::vector<float> buf(2 * (size_t)wspr::kMaxSamples);
    for (int i = 0; i < wspr::kMaxSamples; ++i) { buf[2 * i] = I[i]; buf[2 * i + 1] = -Q[i]; }
    size_t nw = fwrite(name, sizeof(char), sizeof name, fd);
    nw += fwrite(&type, sizeof(int), 1, fd);
    nw += fwrite(&dial_hz, sizeof(double), 1, fd);
    nw += fwrite(buf.data(), sizeof(float), buf.size(), fd);
    const bool closed = fclose(fd) == 0;
    if (nw != sizeof name + 2 + buf.size() || !closed) { fprintf(stderr, "Cannot write all the data!\n"); return 0; }
    return wspr::kMaxSamples;
}

// The -r playback spot line, rtlsdr_wsprd.c:691-701 (without the trailing newline).
int wspr_format_spot(const struct decoder_results* r, char* out, size_t cap) {
    return snprintf(out, cap, "Spot : %6.2f %6.2f %10.6f %2d %7s %6s %2s", r->snr, r->dt, r->freq, (int)r->drift,
                    r->call, r->loc, r->pwr);
}

// The same line followed by pass, stage, block, nhard, dist and metric of the spot's record (wspr_last_spot_details()).
int wspr_format_spot_extended(const struct decoder_results* r, const wspr_spot_detail* d, char* out, size_t cap) {
    return snprintf(out, cap, "Spot : %6.2f %6.2f %10.6f %2d %7s %6s %2s %1d %1d %1d %3d %5d %6d", r->snr, r->dt, r->freq,
                    (int)r->drift, r->call, r->loc, r->pwr, (int)d->pass, (int)d->stage, (int)d->block, (int)d->nhard,
                    (int)d->dist, (int)d->metric);
}

// ---- live-receiver output formats (formatting only, no network) ------
// printSpots(), rtlsdr_wsprd.c:447-474: the daemon's stdout line with the UTC frame time.
int wspr_format_spot_timestamped(const struct decoder_results* r, int year, int month, int day, int hour, int minute,
                                 char* out, size_t cap) {
    return snprintf(out, cap, "Spot :  %04d-%02d-%02d %02d:%02dz %6.2f %6.2f %10.6f %2d %7s %6s %2s", year, month, day,
                    hour, minute, r->snr, r->dt, r->freq, (int)r->drift, r->call, r->loc, r->pwr);
}

// The wsprnet.org report URL of postSpots(), rtlsdr_wsprd.c:414-429 (spot) and :390-397 (empty
// report when r == NULL).  Only the text is produced; nothing is sent.
int wspr_format_wsprnet_url(const struct decoder_results* r, const struct decoder_options* opt, double dial_hz,
                            int year, int month, int day, int hour, int minute, const char* app_version,
                            char* out, size_t cap) {
    const std::string rcall = url_escape(opt->rcall), rloc = url_escape(opt->rloc);
    if (!r)
        return snprintf(out, cap,
                        "https://wsprnet.org/post?function=wsprstat&rcall=%s&rgrid=%s&rqrg=%.6f&tpct=%.2f&tqrg=%.6f&dbm=%d&version=%s&mode=2",
                        rcall.c_str(), rloc.c_str(), dial_hz / 1e6, 0.0f, dial_hz / 1e6, 0, app_version);
    return snprintf(out, cap,
                    "https://wsprnet.org/post?function=wspr&rcall=%s&rgrid=%s&rqrg=%.6f&date=%02d%02d%02d&time=%02d%02d&sig=%.0f&dt=%.1f&tqrg=%.6f&tcall=%s&tgrid=%s&dbm=%s&version=%s&mode=2",
                    rcall.c_str(), rloc.c_str(), r->freq, year % 100, month, day, hour, minute, r->snr, r->dt, r->freq,
                    r->call, r->loc, r->pwr, app_version);
}

}  // extern "C"
