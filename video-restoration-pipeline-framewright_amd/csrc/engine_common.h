// Host-side scaffolding shared by the six network sequencers (rrdbnet, nafnet, ifnet, restormer, srvgg, aesrgan .hip): device
// buffers, the workspace and the hipGraph cache.  The lifetime and ordering rules of the library's host layer live here, once.
// The status / last-error mapping of the C-ABI (fail, guarded) is fw_status.h, which the frame-stage files share through
// stage_common.h and the op files (restormer_ops, ifnet_ops .hip) include directly.  nafnet.hip holds fw_nafnet_* only: the C
// entries of the frame ops (crop, tile blend, temporal average, resizes, ...) sit with their launchers in frame_ops.hip.  No device code.
#pragma once
#include <array>
#include <string>
#include <vector>
#include "fw_status.h"

namespace fw {

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

inline void upload(DevBuf& b, const void* src, size_t bytes) {
    b.release();
    FW_HIP_CHECK(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    FW_HIP_CHECK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
}

// bump allocator over an engine's workspace; `plan` = dry run of the sequencing that only measures the peak
struct Arena {
    char* base = nullptr;
    size_t top = 0, peak = 0;
    bool plan = false;
    void* take(size_t bytes) {
        const size_t at = top;
        top += (bytes + 255) / 256 * 256;
        if (top > peak) peak = top;
        return base + at;   // plan mode: base == nullptr, the pointer is never dereferenced or launched on
    }
};

// ---- hipGraph replay of a forward -----------------------------------------------------------------------------------------------
// One executable graph per key.  The key is everything a captured launch sequence bakes in - frame size, sample format, scalar
// arguments, buffer addresses - as 64-bit words (unused words zero).  The graphs also hold the addresses of the workspace and of
// the weights: whoever frees or replaces either calls clear() first (after a device synchronise when replays may be in flight).
// Whether a given forward is graphed at all is the engine's policy; an engine's first forward must run eagerly, because one-time
// initialisations inside the launchers must not land in a capture.
struct GraphCache {
    using Key = std::array<uint64_t, 7>;
    struct Entry {
        Key key;
        hipGraph_t graph;
        hipGraphExec_t exec;
    };
    std::vector<Entry> entries;

    bool empty() const { return entries.empty(); }

    void clear() {
        for (auto& e : entries) {
            if (e.exec) (void)hipGraphExecDestroy(e.exec);
            if (e.graph) (void)hipGraphDestroy(e.graph);
        }
        entries.clear();
    }

    // Replays on `st` what `record(capture_stream)` enqueues, capturing it at the first use of `key`.
    template <typename Record>
    void launch(const Key& key, hipStream_t st, Record&& record) {
        Entry* hit = nullptr;
        for (auto& e : entries)
            if (e.key == key) hit = &e;
        if (!hit) {
            if (entries.size() >= 16) clear();   // callers that never reuse their buffers: do not grow without bound
            (void)conv_zero_page();              // its first use allocates: not inside a capture
            // capture on a stream of our own: the caller's stream may be the legacy default stream, which cannot capture
            hipStream_t cs = nullptr;
            FW_HIP_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
            Entry e{key, nullptr, nullptr};
            hipError_t err = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
            if (err == hipSuccess) {
                try {
                    record(cs);
                } catch (...) {
                    hipGraph_t junk = nullptr;
                    (void)hipStreamEndCapture(cs, &junk);
                    if (junk) (void)hipGraphDestroy(junk);
                    (void)hipStreamDestroy(cs);
                    throw;
                }
                err = hipStreamEndCapture(cs, &e.graph);
            }
            if (err == hipSuccess) err = hipGraphInstantiate(&e.exec, e.graph, nullptr, nullptr, 0);
            (void)hipStreamDestroy(cs);
            if (err != hipSuccess) {
                if (e.graph) (void)hipGraphDestroy(e.graph);
                FW_HIP_CHECK(err);
            }
            entries.push_back(e);
            hit = &entries.back();
        }
        FW_HIP_CHECK(hipGraphLaunch(hit->exec, st));
    }
};

// Grows an engine's workspace to `need` bytes.  The previous workspace may still be in use by work queued on some stream, hence
// the device synchronise before it is freed; the engine's captured graphs hold its addresses and go with it.  After a failed
// allocation the buffer reads as empty.
inline void ensure_workspace(DevBuf& ws, size_t need, GraphCache* graphs = nullptr) {
    if (ws.bytes >= need) return;
    FW_HIP_CHECK(hipDeviceSynchronize());
    if (graphs) graphs->clear();
    ws.release();
    FW_HIP_CHECK(hipMalloc(&ws.p, need));
    ws.bytes = need;
}

}  // namespace fw
