"""Invalid calls of every C-ABI entry of the nine frame-stage files (scene_cuts, dedup_hash, optical_flow, nlmeans, temporal_chain,
flicker, color_lut, deinterlace, vhs .hip), shared by tools/gen_stage_errors_golden.py (which records what the library answers) and
tests/test_stage_errors_gpu.py (which replays them against tests/golden/stage_errors.json).

Every call is refused by an argument check that runs before the first HIP call, so no device is touched: "device" pointers are
made-up addresses that nothing dereferences, frame-pointer tables and the shift list (which the entries do read) are real host
arrays.  A case is (entry, label, args); the label names the one thing that is wrong with the call.
"""
from __future__ import annotations

import ctypes as C

_KEEP: list = []      # the host arrays the argument lists point into


def dev(k: int) -> int:
    """A made-up device address: 256 MiB apart, so that frames of the sizes used below never overlap by accident."""
    return 0x7F0000000000 + (k << 28)


def table(*addrs):
    t = (C.c_void_p * max(1, len(addrs)))(*addrs)
    _KEEP.append(t)
    return t


def ints(*vals):
    t = (C.c_int32 * len(vals))(*vals)
    _KEEP.append(t)
    return t


def cases() -> list:
    A, B, D, E, F = (dev(k) for k in range(1, 6))
    st = None                      # the stream: never reached
    out: list = []

    def add(entry, label, *args):
        out.append((entry, label, list(args)))

    # ---- scene_cuts.hip
    add("fw_scene_ssim_workspace_bytes", "height 6", 1, 6, 64)
    add("fw_scene_ssim_u8", "null frames_a", None, B, 0, 1, 16, 16, D, E, st)
    add("fw_scene_ssim_u8", "pairs 0", A, B, 0, 0, 16, 16, D, E, st)
    add("fw_scene_ssim_u8", "height 6", A, B, 0, 1, 6, 16, D, E, st)
    add("fw_scene_ssim_u8", "2^31 pixels", A, B, 0, 1, 65536, 32768, D, E, st)
    add("fw_scene_ssim_u8", "stride 0 with two pairs", A, B, 0, 2, 16, 16, D, E, st)
    add("fw_hist64x3_u8", "null hist", A, 1, 16, 16, None, st)
    add("fw_hist64x3_u8", "count 65536", A, 65536, 16, 16, D, st)
    add("fw_hist64x3_u8", "width 0", A, 1, 16, 0, D, st)
    # ---- dedup_hash.hip
    add("fw_pil_lanczos_taps", "out_size 0", 16, 0, None, None, None, 0)
    add("fw_pil_thumb_workspace_bytes", "thumbnail of 66", 1, 16, 16, 66, 8, 1)
    add("fw_pil_thumb_u8", "null workspace", A, 0, 1, 16, 16, 9, 8, 1, D, None, st)
    add("fw_pil_thumb_u8", "side 16385", A, 0, 1, 16385, 16, 9, 8, 1, D, E, st)
    add("fw_pil_thumb_u8", "negative stride", A, -1, 1, 16, 16, 9, 8, 1, D, E, st)
    add("fw_dhash_pack_u8", "null bits", A, 1, 8, None, st)
    add("fw_dhash_pack_u8", "hash size 1", A, 1, 1, D, st)
    # ---- optical_flow.hip
    add("fw_farneback_scratch_bytes", "height 0", 0, 16, 3)
    flow = lambda **kw: [kw.get("prev", A), B, kw.get("channels", 1), kw.get("height", 16), 16, kw.get("pyr_scale", 0.5),  # noqa: E731
                         kw.get("levels", 3), kw.get("winsize", 15), 3, kw.get("poly_n", 5), kw.get("poly_sigma", 1.2),
                         kw.get("flags", 0), D, E, F, st]
    add("fw_farneback_flow_u8", "null prev", *flow(prev=None))
    add("fw_farneback_flow_u8", "2 channels", *flow(channels=2))
    add("fw_farneback_flow_u8", "height 0", *flow(height=0))
    add("fw_farneback_flow_u8", "poly_n 7", *flow(poly_n=7))
    add("fw_farneback_flow_u8", "flags 4", *flow(flags=4))
    add("fw_farneback_flow_u8", "winsize 4", *flow(winsize=4))
    add("fw_farneback_flow_u8", "levels 17", *flow(levels=17))
    add("fw_farneback_flow_u8", "pyr_scale 1", *flow(pyr_scale=1.0))
    add("fw_farneback_flow_u8", "poly_sigma 101", *flow(poly_sigma=101.0))
    add("fw_flow_stats_f32", "null variance", A, B, 16, 16, D, None, st)
    add("fw_flow_confidence_f32", "nothing asked for", A, B, None, None, 16, 16, None, None, st)
    add("fw_flow_confidence_f32", "weight map without magnitude", A, B, None, None, 16, 16, D, E, st)
    # ---- nlmeans.hip
    add("fw_nlmeans_scratch_bytes", "even search window", 16, 16, 20)
    add("fw_nlmeans_u8", "null dst", A, 1, 16, 16, 3.0, 7, 21, None, None, st)
    add("fw_nlmeans_u8", "dst equals src", A, 1, 16, 16, 3.0, 7, 21, None, A, st)
    add("fw_nlmeans_u8", "4 channels", A, 4, 16, 16, 3.0, 7, 21, None, B, st)
    add("fw_nlmeans_u8", "height 1", A, 1, 1, 16, 3.0, 7, 21, None, B, st)
    add("fw_nlmeans_u8", "h 0", A, 1, 16, 16, 0.0, 7, 21, None, B, st)
    add("fw_nlmeans_u8", "template window 9", A, 1, 16, 16, 3.0, 9, 21, None, B, st)
    add("fw_nlmeans_u8", "search window 20", A, 1, 16, 16, 3.0, 7, 20, None, B, st)
    add("fw_nlmeans_colored_u8", "null scratch", A, 16, 16, 3.0, 3.0, 7, 21, None, B, st)
    add("fw_nlmeans_colored_u8", "h_color 0", A, 16, 16, 3.0, 0.0, 7, 21, D, B, st)
    add("fw_nlmeans_colored_u8", "2^31 pixels", A, 65536, 32768, 3.0, 3.0, 7, 21, D, B, st)
    add("fw_nlmeans_weight_table", "h 0", 0.0, 1, 7, 21, None, 0)
    add("fw_nlmeans_weight_table", "even template window", 3.0, 1, 6, 21, None, 0)
    add("fw_nlmeans_lab_tables", "which 4", 4, None, 0)
    # ---- temporal_chain.hip
    add("fw_frame_stats_u8", "null hist", A, 1, 16, 16, None, D, st)
    add("fw_frame_stats_u8", "count 0", A, 0, 16, 16, B, D, st)
    add("fw_frame_stats_u8", "height 0", A, 1, 0, 16, B, D, st)
    add("fw_flow_accumulate_affine_u8", "flow_x without flow_y", A, B, None, None, 1.0, 0.0, 0, 16, 16, D, E, st)
    add("fw_flow_accumulate_affine_u8", "null accumulated", A, None, None, None, 1.0, 0.0, 0, 16, 16, None, E, st)
    add("fw_add_weighted_u8", "null b", A, 0.5, None, 0.5, 16, D, st)
    add("fw_add_weighted_u8", "alpha inf", A, float("inf"), B, 0.5, 16, D, st)
    # ---- flicker.hip
    add("fw_bgr_to_lab_u8", "null dst", A, 16, None, st)
    add("fw_bgr_to_lab_u8", "0 pixels", A, 0, B, st)
    add("fw_lab_to_bgr_u8", "null src", None, 16, B, st)
    add("fw_lab_to_bgr_u8", "2^30 + 1 pixels", A, (1 << 30) + 1, B, st)
    add("fw_lab_l_sums_u8", "null sums", A, 1, 16, 16, None, st)
    add("fw_lab_l_sums_u8", "count 0", A, 0, 16, 16, B, st)
    add("fw_lab_l_sums_u8", "width 0", A, 1, 16, 0, B, st)
    add("fw_deflicker_lab_u8", "null luts", A, 1, 16, 16, None, B, st)
    add("fw_deflicker_lab_u8", "count 65536", A, 65536, 16, 16, D, B, st)
    add("fw_deflicker_lab_u8", "2^31 pixels", A, 1, 65536, 32768, D, B, st)
    add("fw_gamma_lab_tables", "which 3", 3, None, 0)
    add("fw_gamma_lab_tables", "capacity 1", 0, ints(0), 1)
    # ---- color_lut.hip
    for fn, bad_addr in (("fw_lut3d_apply_u8", None), ("fw_lut3d_apply_u16", A + 1)):
        add(fn, "null src", None, 0, 1, 16, 16, D, 33, 1, B, 0, st)
        add(fn, "n 0", A, 0, 0, 16, 16, D, 33, 1, B, 0, st)
        add(fn, "side 16385", A, 0, 1, 16, 16385, D, 33, 1, B, 0, st)
        add(fn, "stride 0 with two frames", A, 0, 2, 16, 16, D, 33, 1, B, 0, st)
        add(fn, "null table", A, 0, 1, 16, 16, None, 33, 1, B, 0, st)
        add(fn, "table size 66", A, 0, 1, 16, 16, D, 66, 1, B, 0, st)
        if bad_addr is not None:
            add(fn, "odd address", bad_addr, 0, 1, 16, 16, D, 33, 1, B, 0, st)
    add("fw_table3_apply_u8", "null dst", A, 0, 1, 16, 16, D, None, 0, st)
    add("fw_table3_apply_u8", "height 0", A, 0, 1, 0, 16, D, B, 0, st)
    add("fw_table3_apply_u8", "negative stride", A, 0, 1, 16, 16, D, B, -4, st)
    add("fw_table3_apply_u8", "null tables", A, 0, 1, 16, 16, None, B, 0, st)
    # ---- deinterlace.hip (modes: 0 YADIF, 1 BWDIF, 2 BOB)
    add("fw_deinterlace_u8", "null cur", None, None, None, B, 16, 48, 0, 1, st)
    add("fw_deinterlace_u8", "BWDIF without prev", A, None, D, B, 16, 48, 1, 1, st)
    add("fw_deinterlace_u8", "rows 0", A, None, None, B, 0, 48, 0, 1, st)
    add("fw_deinterlace_u8", "row_bytes 65537", A, None, None, B, 16, 65537, 0, 1, st)
    add("fw_deinterlace_u8", "mode 3", A, None, None, B, 16, 48, 3, 1, st)
    add("fw_deinterlace_u8", "parity 2", A, None, None, B, 16, 48, 0, 2, st)
    add("fw_deinterlace_u8", "BOB of one row", A, None, None, B, 1, 48, 2, 0, st)
    add("fw_deinterlace_u8", "dst equals cur", A, None, None, A, 16, 48, 0, 1, st)
    add("fw_deinterlace_u8", "dst inside next", A, D, E, E + 100, 16, 48, 1, 1, st)
    add("fw_deinterlace_batch_u8", "null table", None, 1, 16, 48, 0, 1, st)
    add("fw_deinterlace_batch_u8", "n 0", table(A, 0, 0, B), 0, 16, 48, 0, 1, st)
    add("fw_deinterlace_batch_u8", "null dst of the second frame", table(A, 0, 0, B, D, 0, 0, 0), 2, 16, 48, 0, 1, st)
    add("fw_deinterlace_batch_u8", "dst of one frame is cur of another", table(A, 0, 0, B, B, 0, 0, D), 2, 16, 48, 0, 1, st)
    add("fw_interlace_stats_u8", "null table", None, 1, 16, 16, 3, D, st)
    add("fw_interlace_stats_u8", "null stats", table(A), 1, 16, 16, 3, None, st)
    add("fw_interlace_stats_u8", "n 0", table(A), 0, 16, 16, 3, D, st)
    add("fw_interlace_stats_u8", "height 0", table(A), 1, 0, 16, 3, D, st)
    add("fw_interlace_stats_u8", "width 16385", table(A), 1, 16, 16385, 3, D, st)
    add("fw_interlace_stats_u8", "2 channels", table(A), 1, 16, 16, 2, D, st)
    add("fw_interlace_stats_u8", "null second frame", table(A, 0), 2, 16, 16, 3, D, st)
    add("fw_frame_absdiff_sum_u8", "null b", table(A), None, 1, 16, 16, 3, D, st)
    add("fw_frame_absdiff_sum_u8", "n 0", table(A), table(B), 0, 16, 16, 3, D, st)
    add("fw_frame_absdiff_sum_u8", "height 16385", table(A), table(B), 1, 16385, 16, 3, D, st)
    add("fw_frame_absdiff_sum_u8", "2 channels", table(A), table(B), 1, 16, 16, 2, D, st)
    add("fw_frame_absdiff_sum_u8", "null frame of b", table(A), table(0), 1, 16, 16, 3, D, st)
    # ---- vhs.hip
    gs = lambda **kw: [kw.get("frames", table(A)), kw.get("n", 1), kw.get("height", 32), 16, kw.get("channels", 3),  # noqa: E731
                       kw.get("min_len", 4), kw.get("sums", D), kw.get("bottom", None), kw.get("runs", None), kw.get("cap", 0),
                       kw.get("count", None), st]
    add("fw_vhs_gray_stats_u8", "height 0", *gs(height=0))
    add("fw_vhs_gray_stats_u8", "2 channels", *gs(channels=2))
    add("fw_vhs_gray_stats_u8", "null table", *gs(frames=None))
    add("fw_vhs_gray_stats_u8", "n 0", *gs(n=0))
    add("fw_vhs_gray_stats_u8", "null frame", *gs(frames=table(0)))
    add("fw_vhs_gray_stats_u8", "nothing asked for", *gs(sums=None))
    add("fw_vhs_gray_stats_u8", "bottom rows of a 29-row frame", *gs(height=29, bottom=E))
    add("fw_vhs_gray_stats_u8", "runs without a counter", *gs(runs=E, cap=16))
    add("fw_vhs_blend_rows_u8", "rows 0", table(A), table(B), 1, 0, 48, D, E, 1, st)
    add("fw_vhs_blend_rows_u8", "null spec", table(A), table(B), 1, 16, 48, None, E, 1, st)
    add("fw_vhs_blend_rows_u8", "m 0", table(A), table(B), 1, 16, 48, D, E, 0, st)
    add("fw_vhs_blend_rows_u8", "null src table", None, table(B), 1, 16, 48, D, E, 1, st)
    add("fw_vhs_blend_rows_u8", "n 33", table(*[dev(10 + i) for i in range(33)]), table(*[dev(50 + i) for i in range(33)]), 33, 16, 48,
        D, E, 1, st)
    add("fw_vhs_blend_rows_u8", "null dst frame", table(A), table(0), 1, 16, 48, D, E, 1, st)
    add("fw_vhs_blend_rows_u8", "dst equals src", table(A), table(A), 1, 16, 48, D, E, 1, st)
    add("fw_vhs_blend_rows_u8", "two dst frames overlap", table(A, B), table(F, F + 100), 2, 16, 48, D, E, 1, st)
    add("fw_vhs_rainbow_u8", "width 16385", table(A), table(B), 1, 16, 16385, 0.5, 0.5, st)
    add("fw_vhs_rainbow_u8", "n 0", table(A), table(B), 0, 16, 16, 0.5, 0.5, st)
    add("fw_vhs_rainbow_u8", "dst inside src", table(A), table(A + 3), 1, 16, 16, 0.5, 0.5, st)
    add("fw_vhs_box_gray_sums_u8", "2 channels", table(A), 1, 16, 16, 2, D, 1, E, st)
    add("fw_vhs_box_gray_sums_u8", "n 65", table(*[dev(10 + i) for i in range(65)]), 65, 16, 16, 3, D, 1, E, st)
    add("fw_vhs_box_gray_sums_u8", "null tasks", table(A), 1, 16, 16, 3, None, 1, E, st)
    add("fw_vhs_box_gray_sums_u8", "m 0", table(A), 1, 16, 16, 3, D, 0, E, st)
    rp = lambda **kw: [kw.get("sources", table(A)), kw.get("ns", 1), kw.get("results", table(B)), kw.get("nr", 1),  # noqa: E731
                       kw.get("height", 16), 16, 3, kw.get("boxes", D), kw.get("m", 1), kw.get("strength", 0.5), st]
    add("fw_vhs_dropout_repair_u8", "height 0", *rp(height=0))
    add("fw_vhs_dropout_repair_u8", "null sources", *rp(sources=None))
    add("fw_vhs_dropout_repair_u8", "33 results", *rp(results=table(*[dev(50 + i) for i in range(33)]), nr=33))
    add("fw_vhs_dropout_repair_u8", "null boxes", *rp(boxes=None))
    add("fw_vhs_dropout_repair_u8", "m 0", *rp(m=0))
    add("fw_vhs_dropout_repair_u8", "strength 0", *rp(strength=0.0))
    add("fw_vhs_dropout_repair_u8", "result equals source", *rp(results=table(A)))
    add("fw_vhs_dropout_repair_u8", "two results overlap", *rp(results=table(B, B + 8), nr=2))
    add("fw_vhs_edge_counts_u8", "width 0", table(A), 1, 16, 0, D, st)
    add("fw_vhs_edge_counts_u8", "null counts", table(A), 1, 16, 16, None, st)
    add("fw_vhs_edge_counts_u8", "n 0", table(A), 0, 16, 16, D, st)
    add("fw_vhs_edge_counts_u8", "null frame", table(A, 0), 2, 16, 16, D, st)
    add("fw_vhs_chroma_samples_u8", "height 16385", table(A), 1, 16385, 16, D, 1, E, st)
    add("fw_vhs_chroma_samples_u8", "n 0", table(A), 0, 16, 16, D, 1, E, st)
    add("fw_vhs_chroma_samples_u8", "null offsets", table(A), 1, 16, 16, D, 1, None, st)
    add("fw_vhs_chroma_samples_u8", "6401 samples", table(A), 1, 16, 16, D, 6401, E, st)
    add("fw_vhs_chroma_shift_u8", "height 0", table(A), table(B), ints(1), 1, 0, 16, st)
    add("fw_vhs_chroma_shift_u8", "null shifts", table(A), table(B), None, 1, 16, 16, st)
    add("fw_vhs_chroma_shift_u8", "dst equals src", table(A), table(A), ints(1), 1, 16, 16, st)
    add("fw_vhs_chroma_shift_u8", "shift 3", table(A), table(B), ints(3), 1, 16, 16, st)
    add("fw_vhs_column_sums_u8", "height 0", A, 0, 16, D, st)
    add("fw_vhs_column_sums_u8", "null sums", A, 16, 16, None, st)
    add("fw_vhs_column_sums_u8", "one column", A, 16, 1, D, st)
    add("fw_vhs_jitter_shifts_u8", "2 channels", A, 16, 16, 2, D, st)
    add("fw_vhs_jitter_shifts_u8", "null frame", None, 16, 16, 3, D, st)
    add("fw_vhs_jitter_shifts_u8", "two rows", A, 2, 16, 3, D, st)
    add("fw_vhs_saturation_f64", "width 0", A, 16, 0, D, st)
    add("fw_vhs_saturation_f64", "null out", A, 16, 16, None, st)
    return out


def _arg(a):
    return C.cast(a, C.c_void_p) if isinstance(a, C.Array) else a


def replay(lib, case) -> dict:
    """One call: what it returns and, when it refuses, the message it leaves for fw_last_error()."""
    entry, label, args = case
    ret = int(getattr(lib, entry)(*[_arg(a) for a in args]))
    sets_message = ret != 0 or entry.endswith("_tables") or entry.endswith("_weight_table")
    return {"entry": entry, "args": label, "status": ret,
            "message": lib.fw_last_error().decode("utf-8") if sets_message else None}
