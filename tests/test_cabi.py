"""C-ABI surface: the library builds for gfx950, loads without a GPU, and exports every symbol that
include/framewright_hip.h declares.  No compute call is made here."""
import ctypes as C
import re

import numpy as np
import pytest

from framewright_amd import _lib


def _header_symbols():
    text = (_lib.PKG_DIR.parent / "include" / "framewright_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fw_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _header_symbols() == sorted(_lib.EXPORTS)


I32, I64, F32, F64, SZ, VP = C.c_int, C.c_long, C.c_float, C.c_double, C.c_size_t, C.c_void_p
_NET = "typedef struct fw_net fw_net;\n"
# one literal header per mapping rule of _lib._read_header: (text, host-array table, [(name, restype, argtypes)])
READER_CASES = {
    "scalars": ("int fw_a(int a, long b, float c, double d, size_t e, unsigned f, int64_t g, uint64_t h);\n"
                "size_t fw_b(void);\ndouble fw_c();\nlong fw_d(const int n);", {},
                [("fw_a", I32, [I32, I64, F32, F64, SZ, C.c_uint, C.c_int64, C.c_uint64]), ("fw_b", SZ, []), ("fw_c", F64, []),
                 ("fw_d", I64, [I32])]),
    "const_char": ("const char* fw_a(const char* key, const char *other);", {}, [("fw_a", C.c_char_p, [C.c_char_p, C.c_char_p])]),
    "int_long_pointers": ("int fw_a(int* a, const int* b, long* c, const long* d);", {},
                          [("fw_a", I32, [C.POINTER(I32), C.POINTER(I32), C.POINTER(I64), C.POINTER(I64)])]),
    "pointer_to_pointer": (_NET + "int fw_a(fw_net** out, const uint8_t* const* frames, float** rows);", {},
                           [("fw_a", I32, [C.POINTER(VP)] * 3)]),
    "other_pointers": (_NET + "typedef struct fw_p {\n    float m[9];\n    int32_t a, b; /* fw_x(1) */\n} fw_p;\n"
                       "int fw_a(fw_net* h, const fw_net* g, void* a, void** b, const void* const* c, const uint8_t* d, uint16_t* e,\n"
                       "         const int32_t* f, float* p, const double* q, const fw_p* r, char* buf, int64_t* s);", {},
                       [("fw_a", I32, [VP] * 13)]),
    "host_array_table": ("int fw_a(const float* weights, const float* other, double* total);\nint fw_b(const float* weights);",
                         {("fw_a", "weights"): C.POINTER(F32), ("fw_a", "total"): C.POINTER(F64)},
                         [("fw_a", I32, [C.POINTER(F32), VP, C.POINTER(F64)]), ("fw_b", I32, [VP])]),
    "three_lines": ("int fw_a(int dtype,\n         const void* x,   /* device */\n         long stride);\nint\nfw_b\n(void);", {},
                    [("fw_a", I32, [I32, VP, I64]), ("fw_b", I32, [])]),
    "comments": ("/* call fw_x(1) first;\n * then fw_y(2, 3); */\n// or int fw_w(int a);\nint fw_z(void); /* int fw_v(void); */", {},
                 [("fw_z", I32, [])]),
    "preprocessor": ('#ifndef FW_H\n#define FW_H\n#include <stddef.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n#define FW_A 3\n'
                     "int fw_a(void);\n  #define FW_CALL(x) fw_x(x)\n#ifdef __cplusplus\n}\n#endif\n#endif", {}, [("fw_a", I32, [])]),
}


@pytest.mark.parametrize("case", sorted(READER_CASES))
def test_reader_maps_each_rule(case):
    text, table, want = READER_CASES[case]
    got = _lib._read_header(text, table)
    assert [g[0] for g in got] == [w[0] for w in want]
    for (name, restype, argtypes), (_, want_res, want_args) in zip(got, want):
        assert restype is want_res, name
        assert len(argtypes) == len(want_args) and all(a is b for a, b in zip(argtypes, want_args)), (name, argtypes)


@pytest.mark.parametrize("text,names", [
    ("int fw_ok(int a);\nint fw_bad(flaot x);", ("fw_bad", "flaot")),              # an unknown scalar
    ("int fw_bad(flaot* x);", ("fw_bad", "flaot")),                                # an unknown pointee is not a void* either
    ("int fw_bad(unsigned int x);", ("fw_bad", "unsigned int x")),                 # two-word types are not guessed at
    ("void fw_bad(int x);", ("fw_bad", "void")),
    ("int fw_bad(int*** x);", ("fw_bad", "x")),
    ("int fw_bad(float m[9]);", ("fw_bad", "m[9]")),
    ("int fw_bad(int (*cb)(int));", ("fw_bad",)),
    ("int fw_bad(int);", ("fw_bad",)),                                             # a parameter without a name
    ("int fw_ok(void);\nint fw_bad;", ("fw_bad", "not a prototype")),
])
def test_reader_refuses_what_it_does_not_know(text, names):
    with pytest.raises(_lib.FramewrightHipError) as e:
        _lib._read_header(text, {})
    assert e.value.code == _lib.FW_ERR_INTERNAL
    assert all(n in str(e.value) for n in names)


@pytest.mark.parametrize("key", [("fw_a", "wieghts"), ("fw_missing", "weights")])
def test_reader_refuses_a_table_key_the_header_lacks(key):
    with pytest.raises(_lib.FramewrightHipError) as e:
        _lib._read_header("int fw_a(const float* weights);", {key: C.POINTER(F32)})
    assert e.value.code == _lib.FW_ERR_INTERNAL and key[0] in str(e.value) and key[1] in str(e.value)


def test_constants_are_the_headers_defines():
    assert (_lib.FW_OK, _lib.FW_ERR_INVALID, _lib.FW_ERR_OOM, _lib.FW_ERR_HIP, _lib.FW_ERR_INTERNAL) == (0, 1, 2, 3, 4)
    assert (_lib.FW_HOST, _lib.FW_DEVICE, _lib.FW_DTYPE_BF16, _lib.FW_DTYPE_F16) == (0, 1, 0, 1)
    assert (_lib.FW_NAF_PATH_FRONT, _lib.FW_NAF_PATH_TAIL128, _lib.FW_NAF_PATH_TAIL64, _lib.FW_NAF_PATH_GEMM,
            _lib.FW_NAF_PATH_FUSE_LN) == (1, 2, 4, 8, 16)
    assert (_lib.FW_REST_PATH_FRONT_QKV, _lib.FW_REST_PATH_FRONT_FFN, _lib.FW_REST_PATH_QK_DIRECT, _lib.FW_REST_PATH_MERGE_PROJ,
            _lib.FW_REST_PATH_GEMM16) == (1, 2, 4, 8, 16)
    assert (_lib.FW_RRDB_PATH_PAIR12, _lib.FW_RRDB_PATH_PAIR34, _lib.FW_RRDB_PATH_SPLIT_TRUNK, _lib.FW_RRDB_PATH_RRDB_LO,
            _lib.FW_RRDB_PATH_C5_WINO_RDB12, _lib.FW_RRDB_PATH_C5_WINO_RDB3) == (1, 2, 4, 8, 16, 32)
    assert (_lib.FW_RRDB_TAIL_UP_PHASE, _lib.FW_RRDB_TAIL_FUSED, _lib.FW_RRDB_TAIL_HR_WINO) == (1, 2, 4)


# full signatures written out by hand from the header's prototypes, not derived by the reader
PINNED = {
    "fw_last_error": (C.c_char_p, []),
    "fw_rrdbnet_create": (I32, [I32, I32, I32, I32, C.POINTER(VP)]),
    "fw_rrdbnet_workspace_bytes": (SZ, [VP, I32, I32]),
    "fw_rrdbnet_profile_read": (I32, [VP, C.POINTER(I32), C.POINTER(F64), C.POINTER(F64)]),
    "fw_rrdbnet_run_rrdbs": (I32, [VP, I32, I32, VP, I32, I32, VP, VP, VP]),
    "fw_rrdbnet_block_paths": (I32, [VP, C.POINTER(I32)]),
    "fw_rrdbnet_run_head": (I32, [VP, VP, I32, I32, I32, VP, VP, VP]),
    "fw_rrdbnet_run_tail": (I32, [VP, VP, VP, I32, I32, I32, I32, I32, VP, VP, VP]),
    "fw_rrdbnet_tail_paths": (I32, [VP, I32, I32, C.POINTER(I32)]),
    "fw_conv3x3_nhwc": (I32, [I32, VP, I32, I64, I32, I32, I32, VP, VP, I32, I32, I32, VP, F32, VP, F32, VP, I32, I64, I32, VP, VP]),
    "fw_conv3x3_split_nhwc": (I32, [I32, I32, VP, I32, I64, I32, I32, I32, VP, VP, F32, F32, I32, C.POINTER(I64), C.POINTER(F32), I32,
                                    VP, VP, I32, I64, I32, VP]),
    "fw_temporal_average_u8": (I32, [C.POINTER(VP), C.POINTER(F32), I32, SZ, VP, VP]),
    "fw_hdr_convert": (I32, [VP, VP, I32, I32, I32, I32, VP, VP, VP, VP, VP, VP]),
    "fw_qp_artifacts_u8": (I32, [VP, VP, I32, I32, I32, I32, VP, VP, VP, F64, I32, I32, VP, VP, C.c_uint64, VP, VP]),
    "fw_unsharp_mask_u8": (I32, [VP, I32, I32, I32, I32, C.c_uint, C.c_uint, I32, I32, I32, VP, VP, VP, VP]),
}


def test_pinned_signatures():
    table = {name: (restype, argtypes) for name, restype, argtypes in _lib._SIGNATURES}
    assert len(table) == len(_lib.EXPORTS)      # no name twice
    for name, (restype, argtypes) in PINNED.items():
        got_res, got_args = table[name]
        assert got_res is restype, name
        assert len(got_args) == len(argtypes) and all(a is b for a, b in zip(got_args, argtypes)), (name, got_args)


def test_loaded_library_carries_the_readers_signatures(hip_lib):
    for name, restype, argtypes in _lib._SIGNATURES:
        fn = getattr(hip_lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_library_exports_every_declared_symbol(hip_lib):
    for name in _header_symbols():
        assert hasattr(hip_lib, name), f"{name} declared in the header but not exported"


def test_abi_version_and_error_string(hip_lib):
    assert hip_lib.fw_abi_version() == 4
    assert isinstance(hip_lib.fw_last_error(), bytes)


def test_invalid_arguments_are_reported_not_crashed(hip_lib):
    h = C.c_void_p()
    assert hip_lib.fw_rrdbnet_create(0, 0, 4, 0, C.byref(h)) == _lib.FW_ERR_INVALID
    assert b"num_block" in hip_lib.fw_last_error()
    assert hip_lib.fw_rrdbnet_create(0, 23, 3, 0, C.byref(h)) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_rrdbnet_create(0, 23, 4, 7, C.byref(h)) == _lib.FW_ERR_INVALID
    assert hip_lib.fw_rrdbnet_destroy(None) == _lib.FW_OK
    assert hip_lib.fw_rrdbnet_workspace_bytes(None, 10, 10) == 0


def _pack_ref(w, dtype, cout_tiles, cin_chunks):
    """numpy restatement of the MFMA A-fragment order documented in csrc/conv3x3_mfma.hip."""
    import torch
    cout, cin = w.shape[:2]
    wp = np.zeros((32 * cout_tiles, 32 * cin_chunks, 3, 3), np.float32)
    wp[:cout, :cin] = w
    t = torch.from_numpy(wp).to(torch.bfloat16 if dtype == _lib.FW_DTYPE_BF16 else torch.float16)
    bits = t.view(torch.int16).numpy().view(np.uint16)
    # [chunk][tap][16-channel cout tile][lane][j]: v_mfma_f32_16x16x32 A operand, row = lane & 15, k = 8*(lane >> 4) + j
    out = np.empty((cin_chunks, 9, 2 * cout_tiles, 64, 8), np.uint16)
    lane = np.arange(64)
    for c in range(cin_chunks):
        for tap in range(9):
            for wt in range(2 * cout_tiles):
                co = 16 * wt + (lane & 15)
                for j in range(8):
                    ci = 32 * c + 8 * (lane >> 4) + j
                    out[c, tap, wt, :, j] = bits[co, ci, tap // 3, tap % 3]
    return out.reshape(-1)


@pytest.mark.parametrize("dtype", [_lib.FW_DTYPE_BF16, _lib.FW_DTYPE_F16])
@pytest.mark.parametrize("cout,cin,ct,ch", [(32, 64, 1, 2), (64, 192, 2, 6), (3, 64, 1, 2), (64, 12, 2, 1)])
def test_weight_packing_matches_fragment_map(hip_lib, dtype, cout, cin, ct, ch):
    rng = np.random.default_rng(cout * 1000 + cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
    n = hip_lib.fw_pack_conv3x3(dtype, None, cout, cin, ct, ch, None)
    assert n == ch * 9 * 2 * ct * 64 * 8
    dst = np.zeros(n, np.uint16)
    assert hip_lib.fw_pack_conv3x3(dtype, C.c_void_p(w.ctypes.data), cout, cin, ct, ch,
                                   C.c_void_p(dst.ctypes.data)) == n
    np.testing.assert_array_equal(dst, _pack_ref(w, dtype, ct, ch))


def test_pack_rejects_bad_shapes(hip_lib):
    assert hip_lib.fw_pack_conv3x3(0, None, 65, 64, 2, 2, None) == 0
    assert hip_lib.fw_pack_conv3x3(0, None, 64, 65, 2, 2, None) == 0


@pytest.mark.parametrize("dtype", [_lib.FW_DTYPE_BF16, _lib.FW_DTYPE_F16])
def test_phase_weight_packing_matches_its_fragment_map(hip_lib, dtype):
    """fw_pack_conv_up2x_phase: [row phase a][chunk c][step (tx, r, b) in use order][16-channel tile][lane][j] of the summed
    2x2 phase kernels of nearest-x2 + conv3x3 (csrc/conv_up2x_phase.hip), sums in fp64, rounded once."""
    from conv_pair_ref import rnd64, to_bits
    rng = np.random.default_rng(7)
    w = rng.standard_normal((64, 64, 3, 3)).astype(np.float32)
    n = hip_lib.fw_pack_conv_up2x_phase(dtype, None, None)
    assert n == 2 * 2 * 32 * 64 * 8
    dst = np.zeros(n, np.uint16)
    assert hip_lib.fw_pack_conv_up2x_phase(dtype, C.c_void_p(w.ctypes.data), C.c_void_p(dst.ctypes.data)) == n
    assert hip_lib.fw_pack_conv_up2x_phase(7, None, None) == 0
    fold = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    steps = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1), (2, 0, 1), (2, 1, 1)]   # (tx, r, b); column tap = tx - b
    want = np.empty((2, 2, 8, 4, 64, 8), np.uint16)
    lane = np.arange(64)
    name = "bf16" if dtype == _lib.FW_DTYPE_BF16 else "f16"
    for a in range(2):
        for si, (tx, r, b) in enumerate(steps):
            ws = w.astype(np.float64)[:, :, fold[a][r]][:, :, :, fold[b][tx - b]].sum(axis=(2, 3))
            # ONE rounding of the fp64 sum (through fp32 first, as this test once did, a sum that fp32 puts on a tie goes the wrong way)
            bits = to_bits(rnd64(ws, name), name).reshape(64, 64)
            for c in range(2):
                for wt in range(4):
                    co = 16 * wt + (lane & 15)
                    for j in range(8):
                        want[a, c, si, wt, :, j] = bits[co, 32 * c + 8 * (lane >> 4) + j]
    np.testing.assert_array_equal(dst, want.reshape(-1))
