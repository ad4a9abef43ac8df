// Stand-alone check of csrc/host/wspr_fano_walk.h (tests/test_fano_walk.py builds and runs it): the walk is driven with a
// scripted "search" -- a table of (ret, cycles, data) per attempt, generated from seeds, some entries marked "decodes
// only with the full budget" -- in both placements, serially and on a real pool of 4 and of 16 threads with shuffled
// completion, and compared with the serial walk written out below.
#include <cstdint>
#include <cstdio>
#include <set>
#include <thread>

#include "../../rtlsdr-wsprd_amd/csrc/host/wspr_fano_walk.h"

using wspr::FanoWalk;

static uint64_t mix(uint64_t x) {                            // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

struct Entry { bool gated, decodes, slow; unsigned cycles; unsigned char data[11]; };   // slow: times out at the fast budget
struct Script {
    int na, per;
    bool fast;
    std::vector<Entry> e;                                     // [a * per + q]
    static int off_of(int a, int q, int per) { return (a * per + q) * 3 + 1; }   // where "the vector lies": opaque to the walk
    int search(int off, unsigned* cycles, unsigned char* data11, bool dawdle) const {
        const Entry& x = e[(size_t)(off - 1) / 3];
        const bool ok = x.decodes && !(fast && x.slow);
        // a success returns at once, a time-out takes its time: completion order is not task order
        if (dawdle) for (unsigned k = ok ? 0 : 3 + x.cycles % 8; k > 0; --k) std::this_thread::yield();
        *cycles = ok ? x.cycles : (fast ? 81u * 300u : 81u * 10000u);
        memcpy(data11, x.data, 11);
        return ok ? 0 : -1;
    }
};

static Script make_script(int na, int per, int density_pct, bool fast, uint64_t seed) {
    Script s{na, per, fast, std::vector<Entry>((size_t)na * per)};
    for (size_t i = 0; i < s.e.size(); ++i) {
        const uint64_t h = mix(seed * 1000003u + i);
        Entry& x = s.e[i];
        x.gated = (int)(h % 100) < density_pct;
        x.decodes = (h >> 8) % 100 < (per > 2 ? 4 : 40);      // long walks: few rungs decode, so winners lie at every depth
        x.slow = (h >> 16) % 3 == 0;
        x.cycles = 81 + (unsigned)((h >> 24) % 5000);
        for (int k = 0; k < 11; ++k) x.data[k] = (unsigned char)(mix(h + k) & 0xFF);
    }
    return s;
}

struct Outcome {
    std::vector<int> win, attempts, calls;
    std::vector<unsigned> cycles;
    std::vector<std::vector<unsigned char>> data;
    std::set<int> pending;                                    // offsets
    long n_fano = 0, n_cycles = 0, n_timeout = 0;             // of the attempts that gave a final answer
    bool same_result(const Outcome& o) const {
        return win == o.win && attempts == o.attempts && calls == o.calls && cycles == o.cycles && data == o.data && pending == o.pending;
    }
};

// the serial walk: each candidate tries its gated vectors in rank order and stops at the first that decodes
static Outcome serial_walk(const Script& s) {
    Outcome o;
    for (int a = 0; a < s.na; ++a) {
        int win = s.per, calls = 0;
        unsigned cyc = 0;
        unsigned char d[11] = {0};
        for (int q = 0; q < s.per && win == s.per; ++q) {
            if (!s.e[(size_t)a * s.per + q].gated) continue;
            const int ret = s.search(Script::off_of(a, q, s.per), &cyc, d, false);
            ++calls;
            if (ret == 0) { win = q; break; }
            if (s.fast) { o.pending.insert(Script::off_of(a, q, s.per)); continue; }
            o.n_fano++; o.n_cycles += cyc; o.n_timeout++;
        }
        if (win < s.per) { o.n_fano++; o.n_cycles += cyc; }
        o.win.push_back(win); o.attempts.push_back(std::min(win, s.per - 1) + 1); o.calls.push_back(calls);
        o.cycles.push_back(win < s.per ? cyc : 0);
        o.data.push_back(win < s.per ? std::vector<unsigned char>(d, d + 11) : std::vector<unsigned char>());
    }
    return o;
}

struct Totals { long n_fano = 0, n_cycles = 0, n_timeout = 0; };
static Totals total(const FanoWalk& fw, bool (FanoWalk::*rule)(int) const) {
    Totals t;
    for (int k = 0; k < (int)fw.att.size(); ++k)
        if (!rule || (fw.*rule)(k)) { t.n_fano++; t.n_cycles += fw.res[k].cycles; if (fw.res[k].ret) t.n_timeout++; }
    return t;
}

// threads <= 0: the device placement (one batch search); 1: the host placement on the calling thread; else on a pool
static FanoWalk run_walk(const Script& s, int threads) {
    FanoWalk fw(s.na, s.per);
    for (int a = 0; a < s.na; ++a)
        for (int q = 0; q < s.per; ++q)
            if (s.e[(size_t)a * s.per + q].gated) fw.add(a, q, Script::off_of(a, q, s.per));
    if (threads <= 0) {
        fw.run_device([&](const int* off, int n, int* ret, unsigned* cyc, unsigned char* d10) {
            for (int k = 0; k < n; ++k) {
                unsigned char d11[11];
                ret[k] = s.search(off[k], &cyc[k], d11, false);
                memcpy(d10 + (size_t)k * 10, d11, 10);
            }
        });
        return fw;
    }
    fw.run_host([&](int n, const std::function<void(int)>& task) {
        if (threads == 1) { for (int i = 0; i < n; ++i) task(i); return; }
        std::atomic<int> next{0};                             // one task per grab
        std::vector<std::thread> th;
        for (int t = 0; t < threads; ++t)
            th.emplace_back([&] { for (int i; (i = next.fetch_add(1)) < n;) task(i); });
        for (auto& t : th) t.join();
    }, [&](int off, unsigned* cyc, unsigned char* d11) { return s.search(off, cyc, d11, threads > 1); }, s.fast);
    return fw;
}

static Outcome outcome_of(const FanoWalk& fw, bool device) {
    Outcome o;
    for (int a = 0; a < fw.na; ++a) {
        o.win.push_back(fw.win[a]); o.attempts.push_back(fw.walked(a)); o.calls.push_back(fw.calls[a]);
        o.cycles.push_back(fw.at[a] >= 0 ? fw.res[fw.at[a]].cycles : 0);
        std::vector<unsigned char> d;
        if (fw.at[a] >= 0) { d.assign(fw.res[fw.at[a]].data, fw.res[fw.at[a]].data + 11); if (device) d[10] = 0; }
        o.data.push_back(d);
    }
    for (int k = 0; k < (int)fw.att.size(); ++k)
        if (fw.left_pending(k)) o.pending.insert(fw.att[k].off);
    return o;
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++failures < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

int main() {
    int cases = 0;
    for (int per : {1, 2, 43, 86})
        for (int na : {1, 3, 300})
            for (int density : {0, 7, 50, 100})
                for (int fast = 0; fast < 2; ++fast)
                    for (int threads : {0, 1, 4, 16}) {
                        if (threads == 0 && fast) continue;                   // the device search has one budget
                        const uint64_t seed = mix(((uint64_t)per << 32) ^ (na << 16) ^ (density << 4) ^ fast);
                        const Script s = make_script(na, per, density, fast != 0, seed);
                        Outcome want = serial_walk(s);
                        if (threads == 0) for (auto& d : want.data) if (!d.empty()) d[10] = 0;   // ten bytes come down
                        const FanoWalk fw = run_walk(s, threads);
                        const Outcome got = outcome_of(fw, threads == 0);
                        CHECK(got.same_result(want), "per %d na %d density %d fast %d threads %d", per, na, density, fast, threads);
                        // the counters: the serial rule is the serial walk's totals (full budget), the as-run rule lies
                        // between them and every gated attempt
                        const Totals ser = total(fw, &FanoWalk::serial), run = total(fw, &FanoWalk::as_run), all = total(fw, nullptr);
                        if (!fast)
                            CHECK(ser.n_fano == want.n_fano && ser.n_cycles == want.n_cycles && ser.n_timeout == want.n_timeout,
                                  "serial rule: per %d na %d density %d threads %d: %ld %ld %ld against %ld %ld %ld", per, na, density,
                                  threads, ser.n_fano, ser.n_cycles, ser.n_timeout, want.n_fano, want.n_cycles, want.n_timeout);
                        CHECK(run.n_fano >= want.n_fano && run.n_cycles >= want.n_cycles && run.n_timeout >= want.n_timeout &&
                              run.n_fano <= all.n_fano && run.n_cycles <= all.n_cycles && run.n_timeout <= all.n_timeout,
                              "as-run rule: per %d na %d density %d fast %d threads %d: %ld %ld %ld", per, na, density, fast, threads,
                              run.n_fano, run.n_cycles, run.n_timeout);
                        if (threads == 1 && !fast)                            // nothing is cancelled late on one thread
                            CHECK(run.n_fano == want.n_fano && run.n_cycles == want.n_cycles, "one thread runs the serial walk");
                        // no attempt of a rank above the winner changes anything: rewrite them all and walk again
                        Script t = s;
                        for (int a = 0; a < na; ++a)
                            for (int q = want.win[a] + 1; q < per; ++q) {
                                Entry& x = t.e[(size_t)a * per + q];
                                x.decodes = !x.decodes; x.slow = !x.slow; x.cycles += 7; x.data[0] ^= 0xFF;
                            }
                        CHECK(outcome_of(run_walk(t, threads), threads == 0).same_result(want),
                              "ranks above the winner: per %d na %d density %d fast %d threads %d", per, na, density, fast, threads);
                        ++cases;
                    }
    printf("%s: %d cases, %d failures\n", failures ? "FAILED" : "ok", cases, failures);
    return failures ? 1 : 0;
}
