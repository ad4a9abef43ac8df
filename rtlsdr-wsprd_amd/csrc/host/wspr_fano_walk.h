// The one statement of "search every gated vector, keep the first success in walk order" (the jitter ladder, wsprd.c:
// 739-766, and every stage built like it).  A candidate walks its vectors in a fixed order and stops at the first one the
// Fano search decodes; the attempts are independent, so all listed ones may be searched at once and the pick made
// afterwards from their results.  Host C++ without HIP: the caller supplies "search this vector" and "run these tasks".
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <vector>

namespace wspr {

struct FanoWalk {
    struct Attempt { int a, q, off; };           // candidate, rank in its walk order (0 <= q < per), where the vector lies
    struct Result {
        int ret = -1;                            // the search's return value (0: decoded); -1 where it never ran
        unsigned cycles = 0;
        bool ran = false, pending = false;       // pending: timed out at the fast budget, decides nothing yet
        unsigned char data[11] = {0};
    };
    using Search = std::function<int(int off, unsigned* cycles, unsigned char* data11)>;
    using BatchSearch = std::function<void(const int* off, int n, int* ret, unsigned* cycles, unsigned char* data10)>;
    using RunTasks = std::function<void(int n, const std::function<void(int)>& task)>;

    const int na, per;
    std::vector<Attempt> att;                    // in: the gated attempts only, candidate-major and rank-ascending
    std::vector<Result> res;                     // out, per attempt
    std::vector<int> win, at, calls;             // out, per candidate: winning rank (per: none), its attempt (-1: none),
                                                 // and the searches the serial walk makes (listed attempts up to the winner)
    FanoWalk(int candidates, int ranks) : na(candidates), per(ranks) {}
    void add(int a, int q, int off) { att.push_back(Attempt{a, q, off}); }

    // Device placement: one batch search over all attempts.
    void run_device(const BatchSearch& search) {
        const int nv = (int)att.size();
        std::vector<int> off(nv), ret(nv);
        std::vector<unsigned> cyc(nv);
        std::vector<unsigned char> d10((size_t)nv * 10);
        for (int k = 0; k < nv; ++k) off[k] = att[k].off;
        search(off.data(), nv, ret.data(), cyc.data(), d10.data());
        res.assign(nv, Result{});
        for (int k = 0; k < nv; ++k) {
            res[k].ret = ret[k]; res[k].cycles = cyc[k]; res[k].ran = true;
            memcpy(res[k].data, d10.data() + (size_t)k * 10, 10);
        }
        pick();
    }

    // Host placement: rank-major task order and one task per grab -- a time-out costs ~810 000 decoder cycles
    // (milliseconds) while a success costs microseconds, so costs are heavy-tailed; low ranks finish first and cancel the
    // higher ranks of the same candidate.  fast: a time-out is at the fast budget and leaves the attempt pending.
    void run_host(const RunTasks& run, const Search& search, bool fast) {
        const int nv = (int)att.size();
        res.assign(nv, Result{});
        std::vector<int> order(nv);
        for (int k = 0; k < nv; ++k) order[k] = k;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return att[x].q < att[y].q; });
        std::vector<std::atomic<int>> first(na);
        for (auto& f : first) f.store(per);
        run(nv, [&](int task) {
            const int k = order[task];
            const Attempt& t = att[k];
            if (t.q > first[t.a].load()) return;             // an earlier rank already decoded
            Result& r = res[k];
            r.ret = search(t.off, &r.cycles, r.data);
            r.pending = r.ret != 0 && fast;
            r.ran = true;
            if (r.ret == 0) {
                int cur = first[t.a].load();
                while (t.q < cur && !first[t.a].compare_exchange_weak(cur, t.q)) {}
            }
        });
        pick();
    }

    // The two counter rules (Impl::count_fano at the call sites): what the serial walk would have run, and what actually
    // ran to a final answer (late-cancelled attempts included).
    bool serial(int k) const { return att[k].q <= win[att[k].a]; }
    bool as_run(int k) const { return res[k].ran && !res[k].pending; }
    // an unfinished attempt BEFORE the accepted one decides nothing yet: it goes to PendingFano
    bool left_pending(int k) const { return res[k].pending && att[k].q < win[att[k].a]; }
    // ranks the serial walk visits, gated or not
    int walked(int a) const { return std::min(win[a], per - 1) + 1; }

private:
    // no attempt above the winner takes part: a rank above it is only ever a later success or a result nobody reads
    void pick() {
        win.assign(na, per); at.assign(na, -1); calls.assign(na, 0);
        for (int k = 0; k < (int)att.size(); ++k)
            if (res[k].ret == 0 && att[k].q < win[att[k].a]) { win[att[k].a] = att[k].q; at[att[k].a] = k; }
        for (int k = 0; k < (int)att.size(); ++k) calls[att[k].a] += serial(k) ? 1 : 0;
    }
};

}  // namespace wspr
