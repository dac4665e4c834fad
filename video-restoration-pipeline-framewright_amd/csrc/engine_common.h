// Host-side scaffolding shared by the six network sequencers (rrdbnet, nafnet, ifnet, restormer, srvgg, aesrgan .hip): owning
// device buffers, the workspace, the hipGraph cache, and the base of every engine handle with its call scope and its destruction.
// The lifetime and ordering rules of the library's host layer live here, once: device memory enters an engine only through
// upload() and reserve_workspace(), and leaves it in the destructors that destroy_engine() runs.
// The status / last-error mapping of the C-ABI (fail, guarded) is fw_status.h, which the frame-stage files share through
// stage_common.h and the op files (restormer_ops, ifnet_ops .hip) include directly.  nafnet.hip holds fw_nafnet_* only: the C
// entries of the frame ops (crop, tile blend, temporal average, resizes, ...) sit with their launchers in frame_ops.hip.  No device code.
#pragma once
#include <array>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>
#include "fw_status.h"

namespace fw {

// A device allocation and its owner: freed with the buffer, on the device that is current then (destroy_engine sees to that).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            bytes = o.bytes;
            o.p = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf has one owner");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value, "containers of DevBufs move them when they grow");

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

    GraphCache() = default;
    GraphCache(const GraphCache&) = delete;
    GraphCache& operator=(const GraphCache&) = delete;
    ~GraphCache() { clear(); }

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

// ---- the engine handle --------------------------------------------------------------------------------------------------------
// What every struct fw_<engine> is before it is a network: its device, the mutex that serialises the enqueue, the device-side
// ordering of forwards enqueued on different streams (fw_internal.h), the workspace and the captured forwards (an engine
// that never captures keeps the cache empty).
struct EngineBase {
    int device = 0;
    std::mutex mu;
    StreamOrder order;
    DevBuf ws;
    GraphCache graphs;
};

// The scope of an entry that enqueues work on `stream`: the handle's lock, its device, its place in the order of forwards -
// taken in that order, given up in reverse.
struct EngineCall {
    std::lock_guard<std::mutex> lk;
    DevGuard dg;
    hipStream_t st;
    StreamOrder::Scope in_order;
    EngineCall(EngineBase* n, void* stream) : lk(n->mu), dg(n->device), st((hipStream_t)stream), in_order(n->order, st) {}
};

inline void reserve_workspace(EngineBase* n, size_t bytes) { ensure_workspace(n->ws, bytes, &n->graphs); }

// fw_<engine>_destroy.  A call in flight on another thread finishes first; calling INTO a destroyed handle remains the caller's
// bug (the Python engine counts its calls in flight and destroys only when there are none).  The graphs hold the addresses of
// the workspace and of the weights and go before either; every buffer is then freed by the handle's destructors, with the
// handle's device current.
template <typename Engine>
int destroy_engine(Engine* n) {
    if (!n) return FW_OK;
    { std::lock_guard<std::mutex> lk(n->mu); }
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(n->device);
    (void)hipDeviceSynchronize();
    n->graphs.clear();
    n->order.destroy();
    delete n;
    if (prev >= 0) (void)hipSetDevice(prev);
    return FW_OK;
}

}  // namespace fw
