// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the reference's message-layer functions and data
// symbols under the reference's names.  Host code only.
#include <cstdint>
#include <cstring>

#include "wspr_message.h"
#include "wspr_metric_tables.h"
#include "wspr_pipeline.h"

extern "C" {

// ---- message layer under the reference's names ---------------------------------
char get_locator_character_code(char ch) { return wspr::locator_code(ch); }
char get_callsign_character_code(char ch) { return wspr::callsign_code(ch); }
long unsigned int pack_grid4_power(char const* grid4, int power) { return wspr::pack_grid_power(grid4, power); }
long unsigned int pack_call(char const* callsign) { return wspr::pack_callsign(callsign); }
void pack_prefix(char* callsign, int32_t* n, int32_t* m, int32_t* nadd) { wspr::pack_compound(callsign, n, m, nadd); }
void interleave(unsigned char* sym) { wspr::interleave162(sym); }
void deinterleave(unsigned char* sym) { wspr::deinterleave162(sym); }
int get_wspr_channel_symbols(char* message, char* hashtab, char* loctab, unsigned char* symbols) {
    return wspr::channel_symbols(message, hashtab, loctab, symbols);
}
void unpack50(signed char* dat, int32_t* n1, int32_t* n2) { wspr::unpack_50bits(dat, n1, n2); }
int unpackcall(int32_t ncall, char* call) { return wspr::unpack_callsign(ncall, call); }
int unpackgrid(int32_t ngrid, char* grid) { return wspr::unpack_grid(ngrid, grid); }
int unpackpfx(int32_t nprefix, char* call) { return wspr::unpack_prefix(nprefix, call); }
int unpk_(signed char* message, char* hashtab, char* loctab, char* call_loc_pow, char* call, char* loc, char* pwr,
          char* callsign) {
    return wspr::unpack_message(message, hashtab, loctab, call_loc_pow, call, loc, pwr, callsign);
}
int fano(unsigned int* metric, unsigned int* cycles, unsigned int* maxnp, unsigned char* data,
         unsigned char* symbols, unsigned int nbits, int mettab[2][256], int delta, unsigned int maxcycles) {
    return wspr::fano_decode(metric, cycles, maxnp, data, symbols, nbits, mettab, delta, maxcycles);
}
int encode(unsigned char* symbols, unsigned char* data, unsigned int nbytes) {
    return wspr::conv_encode(symbols, data, nbytes);
}
uint32_t nhash(const void* key, size_t length, uint32_t initval) { return wspr::nhash15(key, length, initval); }
void wspr_fano_metric_table(int mettab[2][256]) {
    memcpy(mettab, wspr::default_metrics().tab, sizeof(int) * 512);
}
int doublecomp(const void* a, const void* b) {
    const double x = *(const double*)a, y = *(const double*)b;
    return x < y ? -1 : (x > y);
}
int floatcomp(const void* a, const void* b) {
    const float x = *(const float*)a, y = *(const float*)b;
    return x < y ? -1 : (x > y);
}
// metric_tables (reference wsprd/metric_tables.h:8): a writable data symbol like the reference's, filled from the
// bit patterns before anything else runs
float metric_tables[5][256];
__attribute__((constructor)) static void metric_tables_init(void) {
    static_assert(sizeof(metric_tables) == sizeof(kMetricTableBits), "table shape");
    memcpy(metric_tables, kMetricTableBits, sizeof(metric_tables));
}
// 8-bit parity table (reference wsprd/tab.c:7), generated
unsigned char Partab[256];
__attribute__((constructor)) static void partab_init(void) {
    for (int i = 0; i < 256; ++i) Partab[i] = (unsigned char)__builtin_parity((unsigned)i);
}

}  // extern "C"
