// The message list of the list-decoding stage: see wspr_msglist.h and kernels/listmatch.h.
#include "wspr_msglist.h"

#include <atomic>
#include <cstring>
#include <mutex>
#include <unordered_set>

#include "../kernels/listmatch.h"
#include "wspr_message.h"

namespace wspr {
namespace {

// an empty hash memory that counts what is asked of it: an entry must unpack without a look-up
struct EmptyCounting : HashTable {
    int lookups = 0;
    const char* call_at(int) override { ++lookups; return ""; }
    const char* peek(int) override { ++lookups; return ""; }
    void put(int, const char*, const char*) override {}
};

// One text -> (canonical text, decdata, symbols); false if it does not qualify (listmatch.h: "entry").
bool make_entry(const char* msg, char text[23], unsigned char decdata[11], unsigned char symbols[kNSym]) {
    if (!msg || std::strlen(msg) > 22 || std::strchr(msg, '<')) return false;
    EmptyCounting tab;
    if (!channel_symbols(msg, tab, symbols)) return false;
    // the noise-free code word through the decoder proper: decdata exactly as a Fano decode leaves it
    unsigned char soft[kNSym];
    for (int i = 0; i < kNSym; ++i) soft[i] = (unsigned char)(255 * (symbols[i] >> 1));
    deinterleave162(soft);
    unsigned metric, cycles, maxnp;
    std::memset(decdata, 0, 11);
    if (fano_decode(&metric, &cycles, &maxnp, decdata, soft, kNBits, default_metrics().tab, 60, 10000u) != 0) return false;
    signed char m[12] = {0};
    for (int k = 0; k < 11; ++k) m[k] = (signed char)decdata[k];
    char call[13] = {0}, loc[7] = {0}, pwr[3] = {0}, callsign[13] = {0};
    std::memset(text, 0, 23);
    tab.lookups = 0;
    if (unpack_message(m, tab, text, call, loc, pwr, callsign) != 0 || tab.lookups != 0 || text[0] == '\0') return false;
    unsigned char again[kNSym];
    tab.lookups = 0;
    if (!channel_symbols(text, tab, again) || tab.lookups != 0) return false;
    return std::memcmp(again, symbols, kNSym) == 0;
}

std::mutex g_list_mutex;
std::shared_ptr<const MessageList> g_list;
std::atomic<uint64_t> g_generation{0};

}  // namespace

std::shared_ptr<const MessageList> build_message_list(const char* const* messages, int n, int zmin16, int* bad) {
    using namespace listmatch;
    *bad = -1;
    if (!messages || n <= 0 || n > kMaxEntries || zmin16 < kZminLo || zmin16 > kZminHi) return nullptr;
    auto list = std::make_shared<MessageList>();
    list->zmin16 = zmin16;
    list->text.reserve((size_t)n * 23);
    list->decdata.reserve((size_t)n * 11);
    list->symbols.reserve((size_t)n * kNSym);
    std::unordered_set<uint64_t> seen;
    for (int i = 0; i < n; ++i) {
        char text[23];
        unsigned char dec[11], sym[kNSym];
        if (!make_entry(messages[i], text, dec, sym)) { *bad = i; return nullptr; }
        uint64_t bits = 0;                                    // the 50 message bits
        for (int k = 0; k < 7; ++k) bits = (bits << 8) | (k == 6 ? dec[k] & 0xC0u : dec[k]);
        if (!seen.insert(bits).second) continue;              // a repeat: the first occurrence stays
        list->text.insert(list->text.end(), text, text + 23);
        list->decdata.insert(list->decdata.end(), dec, dec + 11);
        list->symbols.insert(list->symbols.end(), sym, sym + kNSym);
        list->n++;
    }
    const int m = list->n, mpad = padded(m);
    list->table.assign((size_t)kWords * mpad, 0);
    list->bias.assign((size_t)mpad, 0);
    for (int e = 0; e < m; ++e) {
        const unsigned char* sym = list->symbols.data() + (size_t)e * kNSym;
        int b = 0;
        for (int i = 0; i < kN; ++i) {
            const int c = chip(sym[i]);
            b += c;
            list->table[(size_t)(i >> 2) * mpad + e] |= (int32_t)(((uint32_t)c & 0xFFu) << (8 * (i & 3)));
        }
        list->bias[e] = b;
    }
    list->generation = ++g_generation;
    return list;
}

std::shared_ptr<const MessageList> message_list_setting() {
    std::lock_guard<std::mutex> g(g_list_mutex);
    return g_list;
}

void set_message_list_setting(std::shared_ptr<const MessageList> list) {
    std::lock_guard<std::mutex> g(g_list_mutex);
    g_list = std::move(list);
}

}  // namespace wspr
