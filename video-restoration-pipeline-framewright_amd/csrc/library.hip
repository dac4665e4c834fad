// What belongs to the library as a whole and to none of its engines, stages or kernels: the thread-local message behind
// fw_last_error(), the ABI version and the device count.  No device code.
#include "fw_status.h"

namespace fw {
std::string& last_error_ref() {
    thread_local std::string msg;
    return msg;
}
}  // namespace fw

extern "C" {

const char* fw_last_error(void) { return fw::last_error_ref().c_str(); }

int fw_abi_version(void) { return 4; }  // 2: + upscale_u16, resize_lanczos4, grain_addback, attention (softmax rows, transposed pack, MFMA Gram)
                                         // 3 (round 2, additive): + fw_ifnet_*, fw_restormer_*, fw_srvgg_*, fw_unsharp_mask_u8, fw_preserve_edges_*, fw_attn_proj_pack
                                         // 4 (additive): + fw_pack_conv3x3_wino, fw_conv3x3_split_nhwc, fw_conv3x3_wino_nhwc, fw_conv3x3_wino_check_fields
                                         // still 4 (additive entries no longer bump it): + the single-step test hooks fw_nafnet_run_block, fw_restormer_run_block /
                                         // run_step, fw_rrdbnet_run_rrdbs / run_head / run_tail and their *_paths

int fw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
