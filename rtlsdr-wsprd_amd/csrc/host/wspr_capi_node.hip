// C ABI of libwspr_mi355x.so (declared in include/wspr_mi355x.h): the node-level calls -- one host process, every GPU
// of the node.  They reach the decode through the exported batch entry points only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <vector>

#include "wspr_pipeline.h"

using wspr::Context;

// The CPU share of a node-level call lasts as long as the call: raised on entry (to the largest share any call in
// flight asks for), back to 1 when the last such call returns -- so that later single-device calls size their slots
// and pick their Fano placement for the whole host again.  (Pools of contexts CREATED during the call keep the
// share they were sized for.)
namespace {
struct NodeShareGuard {
    // live shares and the published maximum change together under one mutex: a guard that ends while another call
    // begins can no longer publish a share of 1 over the newcomer's (advisor, round 4)
    static std::mutex& mu() { static std::mutex m; return m; }
    static std::vector<int>& live() { static std::vector<int> v; return v; }
    static void publish() {
        int share = 1;
        for (int n : live()) share = std::max(share, n);
        wspr::node_share().store(share);
    }
    int mine;
    explicit NodeShareGuard(int ndevices) : mine(ndevices) {
        std::lock_guard<std::mutex> g(mu());
        live().push_back(mine);
        publish();
    }
    ~NodeShareGuard() {
        std::lock_guard<std::mutex> g(mu());
        auto& v = live();
        for (size_t i = 0; i < v.size(); ++i) if (v[i] == mine) { v.erase(v.begin() + (long)i); break; }
        publish();
    }
};
}  // namespace

extern "C" {

void wspr_shard_range(int nseg, int shard, int nshards, int* lo, int* hi) {
    if (nshards < 1) nshards = 1;
    const int base = nseg / nshards, rem = nseg % nshards;
    const int a = shard * base + (shard < rem ? shard : rem);
    if (lo) *lo = a;
    if (hi) *hi = a + base + (shard < rem ? 1 : 0);
}

// One host process, every GPU of the node: contiguous blocks of segments, one host thread per device,
// each block through wspr_decode_batch() on its device (H2D of the block, decode, spots straight into the caller's
// arrays).  No collective: the segments are independent (wsprd.c:478-479).
int wspr_decode_batch_node(float* idat, float* qdat, int nseg, int samples, size_t seg_stride,
                           struct decoder_options options, struct decoder_results* decodes, int max_results,
                           int* n_results, int ndevices) {
    wspr::NoSpreadRecord no_record;
    const int count = wspr_device_count();
    if (count <= 0) {
        fprintf(stderr, "libwspr_mi355x: wspr_decode_batch_node: no HIP device visible (there is no CPU fallback)\n");
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return -1;
    }
    if (ndevices <= 0) ndevices = count;
    const char* virt = wspr::lab_env("WSPR_NODE_VIRTUAL"); // test hook (lab build only): more shards than devices, folded onto lanes
    const int per_dev = (ndevices + count - 1) / count;
    if ((ndevices > count && !(virt && atoi(virt))) || ndevices > Context::kMaxDevices ||
        Context::lane() + per_dev > Context::kUserLanes) {
        fprintf(stderr, "libwspr_mi355x: wspr_decode_batch_node: %d devices asked for, %d visible\n", ndevices, count);
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return -1;
    }
    if (options.usehashtable && nseg > 1)                // ordered by definition: nothing to spread
        return wspr_decode_batch(idat, qdat, nseg, samples, seg_stride, options, decodes, max_results, n_results, 0);
    NodeShareGuard share(ndevices);
    wspr::CallScope call_scope;
    const wspr::CallSettings settings = wspr::call_settings();
    const int lane0 = Context::lane();
    int home = 0;
    (void)hipGetDevice(&home);
    std::vector<int> rcs(ndevices, 0);
    std::vector<std::thread> th;
    for (int k = 0; k < ndevices; ++k) {
        int lo = 0, hi = 0;
        wspr_shard_range(nseg, k, ndevices, &lo, &hi);
        if (hi <= lo) continue;
        th.emplace_back([=, &rcs] {
            wspr::CallScope worker_scope(settings);
            if (hipSetDevice(k % count) != hipSuccess) {
                rcs[k] = -1;
                for (int s = lo; s < hi; ++s) n_results[s] = 0;
                return;
            }
            Context::bind_lane(lane0 + k / count);
            rcs[k] = wspr_decode_batch(idat + (size_t)lo * seg_stride, qdat + (size_t)lo * seg_stride, hi - lo, samples,
                                       seg_stride, options, decodes + (size_t)lo * max_results, max_results,
                                       n_results + lo, 0);
        });
    }
    for (auto& t : th) t.join();
    (void)hipSetDevice(home);
    int rc = 0;
    for (int k = 0; k < ndevices; ++k) if (rcs[k] < rc) rc = rcs[k];
    if (rc < 0) for (int s = 0; s < nseg; ++s) n_results[s] = 0;      // as the _device variant: a failed call reports no spots
    return rc;
}

// The same fan-out for input that is already RESIDENT on one device (e.g. the front end's output on the GPU a
// receiver bank feeds): every other device pulls its block of rows over xGMI with a peer copy (one process: a peer
// DMA is what an ncclSend/ncclRecv pair between two devices of the same process comes down to), decodes it, and the
// spots land in the caller's arrays.  SURVEY 8e: "for real inputs ... (scatter) of 360 000 B per segment".
int wspr_decode_batch_node_device(const void* d_idat, const void* d_qdat, int src_device, int nseg, int samples,
                                  size_t seg_stride, struct decoder_options options, struct decoder_results* decodes,
                                  int max_results, int* n_results, int ndevices) {
    wspr::NoSpreadRecord no_record;
    const int count = wspr_device_count();
    if (count <= 0 || src_device < 0 || src_device >= count) {
        fprintf(stderr, "libwspr_mi355x: wspr_decode_batch_node_device: no such source device %d (%d visible)\n", src_device, count);
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return -1;
    }
    if (ndevices <= 0) ndevices = count;
    const char* virt = wspr::lab_env("WSPR_NODE_VIRTUAL");
    const int per_dev = (ndevices + count - 1) / count;
    if ((ndevices > count && !(virt && atoi(virt))) || ndevices > Context::kMaxDevices ||
        Context::lane() + per_dev > Context::kUserLanes) {
        fprintf(stderr, "libwspr_mi355x: wspr_decode_batch_node_device: %d devices asked for, %d visible\n", ndevices, count);
        for (int s = 0; s < nseg; ++s) n_results[s] = 0;
        return -1;
    }
    int home = 0;
    (void)hipGetDevice(&home);
    const float* si = static_cast<const float*>(d_idat);
    const float* sq = static_cast<const float*>(d_qdat);
    if (options.usehashtable && nseg > 1) {              // ordered by definition: decoded where the data is
        (void)hipSetDevice(src_device);
        const int rc = wspr_decode_batch_device(si, sq, nseg, samples, seg_stride, options, decodes, max_results, n_results);
        (void)hipSetDevice(home);
        return rc;
    }
    NodeShareGuard share(ndevices);
    wspr::CallScope call_scope;
    const wspr::CallSettings settings = wspr::call_settings();
    const int lane0 = Context::lane();
    std::vector<int> rcs(ndevices, 0);
    std::vector<std::thread> th;
    for (int k = 0; k < ndevices; ++k) {
        int lo = 0, hi = 0;
        wspr_shard_range(nseg, k, ndevices, &lo, &hi);
        if (hi <= lo) continue;
        th.emplace_back([=, &rcs] {
            wspr::CallScope worker_scope(settings);
            const int dev = k % count;
            if (hipSetDevice(dev) != hipSuccess) { rcs[k] = -1; return; }
            Context::bind_lane(lane0 + k / count);
            const size_t off = (size_t)lo * seg_stride, floats = (size_t)(hi - lo) * seg_stride;
            const float *pi = si + off, *pq = sq + off;
            void *ti = nullptr, *tq = nullptr;
            // (under the test hook every block but the first takes the copy path, also on the source device itself)
            // fault injection (lab build only): WSPR_NODE_FAIL_PEER=1 makes every peer copy report failure (the staged copy
            // must take over), WSPR_NODE_FAIL_SHARD=k fails shard k outright (the whole call must fail, no spots reported)
            const char* fail_peer = wspr::lab_env("WSPR_NODE_FAIL_PEER");
            const char* fail_shard = wspr::lab_env("WSPR_NODE_FAIL_SHARD");
            if (fail_shard && atoi(fail_shard) == k) {
                fprintf(stderr, "libwspr_mi355x: shard %d (segments %d..%d, device %d) failed [injected]\n", k, lo, hi, dev);
                rcs[k] = -1;
                return;
            }
            if (dev != src_device || (virt && atoi(virt) && k > 0)) {     // pull the block over xGMI
                bool peer_ok = true;
                if (dev != src_device) {
                    // refused peer access (no link, IOMMU policy, ...) is not an error: hipMemcpyPeer then goes through
                    // the host by itself, and if it reports failure all the same the block is staged here explicitly
                    const hipError_t e = hipDeviceEnablePeerAccess(src_device, 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) peer_ok = false;
                    (void)hipGetLastError();
                }
                bool ok = hipMalloc(&ti, floats * 4) == hipSuccess && hipMalloc(&tq, floats * 4) == hipSuccess;
                bool copied = ok && !(fail_peer && atoi(fail_peer)) &&
                              hipMemcpyPeer(ti, dev, pi, src_device, floats * 4) == hipSuccess &&
                              hipMemcpyPeer(tq, dev, pq, src_device, floats * 4) == hipSuccess &&
                              // a device-to-device copy may return before it has run, and the library's streams are
                              // non-blocking (they do not wait for the null stream): wait here
                              hipStreamSynchronize(nullptr) == hipSuccess;
                if (ok && !copied) {
                    // staged copy: source device -> pinned host -> this device (what the peer copy does without a link)
                    (void)hipGetLastError();
                    void* hp = nullptr;
                    copied = hipHostMalloc(&hp, floats * 4, hipHostMallocDefault) == hipSuccess;
                    for (int rail = 0; copied && rail < 2; ++rail) {
                        copied = hipSetDevice(src_device) == hipSuccess &&
                                 hipMemcpy(hp, rail ? pq : pi, floats * 4, hipMemcpyDeviceToHost) == hipSuccess &&
                                 hipSetDevice(dev) == hipSuccess &&
                                 hipMemcpy(rail ? tq : ti, hp, floats * 4, hipMemcpyHostToDevice) == hipSuccess;
                    }
                    (void)hipSetDevice(dev);
                    if (hp) (void)hipHostFree(hp);
                    if (copied)
                        fprintf(stderr, "libwspr_mi355x: segments %d..%d reached device %d through the host (peer %s)\n", lo, hi,
                                dev, peer_ok ? "copy failed" : "access refused");
                }
                if (!copied) {
                    fprintf(stderr, "libwspr_mi355x: copy of segments %d..%d to device %d failed\n", lo, hi, dev);
                    if (ti) (void)hipFree(ti);
                    if (tq) (void)hipFree(tq);
                    rcs[k] = -1;
                    return;
                }
                pi = static_cast<const float*>(ti); pq = static_cast<const float*>(tq);
            }
            rcs[k] = wspr_decode_batch_device(pi, pq, hi - lo, samples, seg_stride, options,
                                              decodes + (size_t)lo * max_results, max_results, n_results + lo);
            if (ti) (void)hipFree(ti);
            if (tq) (void)hipFree(tq);
        });
    }
    for (auto& t : th) t.join();
    (void)hipSetDevice(home);
    int rc = 0;
    for (int k = 0; k < ndevices; ++k) if (rcs[k] < rc) rc = rcs[k];
    if (rc < 0) for (int s = 0; s < nseg; ++s) n_results[s] = 0;
    return rc;
}

}  // extern "C"
