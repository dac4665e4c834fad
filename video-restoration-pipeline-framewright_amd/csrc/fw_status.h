// The C-ABI's status and last-error mapping, once: a code for the caller, the message for fw_last_error().  Included by
// engine_common.h (the six network sequencers), stage_common.h (the frame-stage files, and frame_ops.hip with the C entries of its
// frame ops) and the op files restormer_ops.hip and ifnet_ops.hip; host code only.
#pragma once
#include <new>
#include <string>
#include "fw_internal.h"
#include "../../include/framewright_hip.h"

namespace fw {

inline int fail(int code, const std::string& msg) {
    last_error_ref() = msg;
    return code;
}

// "<fn>: <msg>", FW_ERR_INVALID: the refusal of an argument check
inline int invalid(const char* fn, const std::string& msg) { return fail(FW_ERR_INVALID, std::string(fn) + ": " + msg); }

// FW_OK for hipSuccess; else the sticky error is cleared and "<fn>: HIP error: ..." is left
inline int hip_status(const char* fn, hipError_t e) {
    if (e == hipSuccess) return FW_OK;
    (void)hipGetLastError();
    return fail(FW_ERR_HIP, std::string(fn) + ": HIP error: " + hipGetErrorString(e));
}

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return FW_OK;
    } catch (const Error& e) {
        return fail(e.code, e.what());
    } catch (const std::bad_alloc&) {
        return fail(FW_ERR_OOM, "host out of memory");
    } catch (const std::exception& e) {
        return fail(FW_ERR_INTERNAL, e.what());
    }
}

}  // namespace fw
