// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the waterfall of a segment (K20; the definition in
// kernels/waterfall.h), its palettes and the two file writers that make the byte image something to look at.  The
// parameters are arguments, not state: no decode call, setting or timing slot is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <exception>
#include <vector>

#include "wspr_capi_impl.h"
#include "wspr_stage_args.h"

using wspr::Context;
using namespace wspr::capi;
namespace args = wspr::args;
namespace waterfall = wspr::waterfall;

static_assert(sizeof(wspr_waterfall_params) == sizeof(waterfall::Params) && sizeof(wspr_waterfall_info) == sizeof(waterfall::Info),
              "the public records are the kernel's");
static_assert(WSPR_WF_REF_ABSOLUTE == waterfall::kRefAbsolute && WSPR_WF_REF_FLOOR == waterfall::kRefFloor &&
              WSPR_WF_WRITTEN == waterfall::kWritten && WSPR_WF_NO_REF == waterfall::kNoRef && WSPR_WF_NONFINITE == waterfall::kNonFinite,
              "the public constants are the definition's");

namespace {
// ---- PNG: the few lines of it an uncompressed 8-bit image needs ---------------------------------------------------------
uint32_t crc32_of(const uint8_t* p, size_t n, uint32_t crc) {        // ISO 3309, as the PNG specification's sample code
    static uint32_t table[256];
    static const bool built = [] {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        return true;
    }();
    (void)built;
    crc = ~crc;
    for (size_t i = 0; i < n; ++i) crc = table[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}
void put_be32(std::vector<uint8_t>& v, uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) v.push_back((uint8_t)(x >> s));
}
// length, type, data, CRC over type and data
void put_chunk(std::vector<uint8_t>& file, const char* type, const std::vector<uint8_t>& data) {
    put_be32(file, (uint32_t)data.size());
    const size_t start = file.size();
    file.insert(file.end(), type, type + 4);
    file.insert(file.end(), data.begin(), data.end());
    put_be32(file, crc32_of(file.data() + start, file.size() - start, 0u));
}
int write_whole_file(const char* filename, const uint8_t* p, size_t n) {
    FILE* fd = fopen(filename, "wb");
    if (!fd) return -1;
    const size_t nw = fwrite(p, 1, n, fd);
    const bool closed = fclose(fd) == 0;
    return (nw == n && closed) ? 0 : -1;
}
bool picture_ok(const char* filename, const uint8_t* img, int width, int height) {
    return filename && img && width >= 1 && height >= 1 && ((long long)width + 1) * (long long)height < (1ll << 31);
}
}  // namespace

extern "C" {

void wspr_waterfall_default_params(wspr_waterfall_params* p) {
    if (!p) return;
    const waterfall::Params d = waterfall::default_params();
    std::memcpy(p, &d, sizeof d);
}

int wspr_waterfall_shape(int samples, const wspr_waterfall_params* p, int* nrows, int* ncols) {
    static const char* where = "wspr_waterfall_shape";
    waterfall::Params use;
    int unused = 0;
    if (const int bad = args::waterfall_args_bad(where, 0, samples, p, &unused, &use)) return bad;
    if (nrows) *nrows = waterfall::rows_of(samples, use.hop, use.tavg);
    if (ncols) *ncols = waterfall::cols_of(use.j0, use.j1);
    return 0;
}

int wspr_waterfall_batch_device(const void* d_idat, const void* d_qdat, int nseg, int samples, size_t seg_stride,
                                const wspr_waterfall_params* p, void* d_img, size_t img_stride, wspr_waterfall_info* info) {
    static const char* where = "wspr_waterfall_batch_device";
    LaneTurn lane_turn;
    try {
        waterfall::Params use;
        if (const int bad = args::waterfall_batch(where, d_idat, d_qdat, nseg, samples, seg_stride, p, d_img, img_stride, info, &use))
            return bad;
        if (nseg == 0) return 0;
        return Context::get().waterfall_device(static_cast<const float*>(d_idat), static_cast<const float*>(d_qdat), nseg, samples,
                                               seg_stride, use, static_cast<uint8_t*>(d_img), img_stride,
                                               reinterpret_cast<waterfall::Info*>(info));
    } catch (const std::exception& e) { return fail(where, e); }
}

int wspr_waterfall(const float* I, const float* Q, int samples, const wspr_waterfall_params* p, uint8_t* img,
                   wspr_waterfall_info* info) {
    static const char* where = "wspr_waterfall";
    LaneTurn lane_turn;
    try {
        waterfall::Params use;
        if (const int bad = args::waterfall_host(where, I, Q, samples, p, img, info, &use)) return bad;
        Context& c = Context::get();
        float* wi = c.work_i(1);
        float* wq = c.work_q(1);
        rows_up(wi, wq, I, Q, (size_t)samples);
        const size_t bytes = (size_t)waterfall::rows_of(samples, use.hop, use.tavg) * (size_t)waterfall::cols_of(use.j0, use.j1);
        const size_t img_stride = (bytes + 15) & ~(size_t)15;
        uint8_t* d_img = c.waterfall_image(img_stride);
        waterfall::Info one;
        std::vector<uint8_t> down(bytes);                    // the whole result arrives before any of it is handed over
        const int rc = c.waterfall_device(wi, wq, 1, samples, (size_t)wspr::kIqStride, use, d_img, img_stride, &one);
        if (rc) return rc;
        if (bytes) HIP_TRY(hipMemcpy(down.data(), d_img, bytes, hipMemcpyDeviceToHost));
        if (bytes) std::memcpy(img, down.data(), bytes);
        std::memcpy(info, &one, sizeof one);
        return 0;
    } catch (const std::exception& e) { return fail(where, e); }
}

// the formula of include/wspr_mi355x.h
void wspr_waterfall_palette(int which, uint8_t rgb[768]) {
    if (!rgb) return;
    for (int v = 0; v < 256; ++v) {
        int r = v, g = v, b = v;
        if (which != 0) {
            const int k = v / 51 < 4 ? v / 51 : 4, t = 5 * (v - 51 * k);
            switch (k) {
                case 0: r = 0; g = 0; b = t; break;
                case 1: r = 0; g = t; b = 255; break;
                case 2: r = t; g = 255; b = 255 - t; break;
                case 3: r = 255; g = 255 - t; b = 0; break;
                default: r = 255; g = t; b = t; break;
            }
        }
        rgb[3 * v] = (uint8_t)r;
        rgb[3 * v + 1] = (uint8_t)g;
        rgb[3 * v + 2] = (uint8_t)b;
    }
}

int wspr_write_pgm_file(const char* filename, const uint8_t* img, int width, int height) {
    if (!picture_ok(filename, img, width, height)) return -1;
    char head[64];
    const int n = snprintf(head, sizeof head, "P5\n%d %d\n255\n", width, height);
    std::vector<uint8_t> file(head, head + n);
    file.insert(file.end(), img, img + (size_t)width * (size_t)height);
    return write_whole_file(filename, file.data(), file.size());
}

int wspr_write_png_file(const char* filename, const uint8_t* img, int width, int height, const uint8_t* rgb768) {
    if (!picture_ok(filename, img, width, height)) return -1;
    static const uint8_t signature[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<uint8_t> file(signature, signature + 8), data;
    put_be32(data, (uint32_t)width);
    put_be32(data, (uint32_t)height);
    const uint8_t rest[5] = {8, (uint8_t)(rgb768 ? 3 : 0), 0, 0, 0};     // bit depth, colour type, deflate, adaptive filtering, no interlace
    data.insert(data.end(), rest, rest + 5);
    put_chunk(file, "IHDR", data);
    if (rgb768) put_chunk(file, "PLTE", std::vector<uint8_t>(rgb768, rgb768 + 768));
    // the scan lines, each behind its filter byte 0 ...
    std::vector<uint8_t> raw;
    raw.reserve(((size_t)width + 1) * (size_t)height);
    for (int y = 0; y < height; ++y) {
        raw.push_back(0);
        raw.insert(raw.end(), img + (size_t)y * (size_t)width, img + ((size_t)y + 1) * (size_t)width);
    }
    // ... as one zlib stream: header (deflate, 32 K window, no dictionary, check bits), stored blocks of at most 65 535
    // bytes (final bit, LEN, ~LEN, little-endian), Adler-32 of the raw bytes, big-endian
    data.assign({0x78, 0x01});
    uint32_t a = 1, b = 0;
    for (size_t at = 0; at < raw.size(); at += 65535) {
        const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
        data.push_back(at + n == raw.size() ? 1 : 0);
        data.push_back((uint8_t)(n & 0xff));
        data.push_back((uint8_t)(n >> 8));
        data.push_back((uint8_t)(~n & 0xff));
        data.push_back((uint8_t)((~n >> 8) & 0xff));
        data.insert(data.end(), raw.begin() + (long)at, raw.begin() + (long)(at + n));
        for (size_t i = at; i < at + n; ++i) {
            a = (a + raw[i]) % 65521u;
            b = (b + a) % 65521u;
        }
    }
    put_be32(data, (b << 16) | a);
    put_chunk(file, "IDAT", data);
    put_chunk(file, "IEND", std::vector<uint8_t>());
    return write_whole_file(filename, file.data(), file.size());
}

}  // extern "C"
