"""The lifetime of a native engine handle, for each of the six network engines at its smallest configuration: every device buffer a
handle acquires - weights set once or again, the forms built at finalize, a workspace that grows - is given back at destroy, and
none of it changes a byte of the output.  The frames are 16 x 16 (24 x 40 where the workspace has to grow), the weights come
from synth.py, every comparison is byte for byte against a fresh handle of the same configuration.

What tests/test_engine_misuse_gpu.py already pins is not repeated here: close twice, a forward after close, the forwards before
any weight, and the Python owners' own answer to a state dict with one key missing (which never reaches finalize).
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE = (16, 16), (24, 40)   # both multiples of 8 (Restormer); IFNet pads to 32 itself


class Kind:
    """One engine configuration: how to make it, its weights, how to set one tensor on the bare handle, and its device forward."""

    def __init__(self, name, make, state, forward, first_missing, twice, tensors=None):
        self.name, self.make, self._state, self.forward = name, make, state, forward
        self._tensors = tensors or (lambda st: dict(st[0]))   # what the owner sets, by key, from the arguments of load_state_dict
        self.first_missing = first_missing   # (keys set) -> what finalize says of a handle that has only those
        self.twice = twice                   # the keys of the set-twice case
        self._cached = None

    def state(self):
        if self._cached is None:
            self._cached = self._state()
        return self._cached

    def keys(self):
        """What the owner sets, in its order: tensors, or RRDBNet's layers (a weight and a bias each)."""
        sd = self._tensors(self.state())
        return [k[:-7] for k in sd if k.endswith(".weight")] if self.name.startswith("rrdbnet") else list(sd)

    def loaded(self):
        eng = self.make()
        eng.load_state_dict(*self.state())
        return eng

    def set_raw(self, eng, key, scale=1.0):
        """One tensor (RRDBNet: one layer) through the C entry itself, its values times ``scale``."""
        from framewright_amd import _lib
        sd = self._tensors(self.state())
        if self.name.startswith("rrdbnet"):
            w = np.ascontiguousarray(sd[key + ".weight"] * np.float32(scale))
            b = np.ascontiguousarray(sd[key + ".bias"] * np.float32(scale))
            _lib.check(eng._lib.fw_rrdbnet_set_conv(eng._h, key.encode(), C.c_void_p(w.ctypes.data), C.c_void_p(b.ctypes.data), w.shape[0], w.shape[1]))
            return
        a = np.ascontiguousarray(sd[key] * np.float32(scale)).reshape(-1)
        set_tensor = getattr(eng._lib, f"fw_{self.name.split('-')[0]}_set_tensor")
        _lib.check(set_tensor(eng._h, key.encode(), C.c_void_p(a.ctypes.data), a.size))

    def finalize(self, eng):
        from framewright_amd import _lib
        _lib.check(getattr(eng._lib, f"fw_{self.name.split('-')[0]}_finalize")(eng._h))


def _frame(size, float_rgb=False, seed=31):
    import torch
    from framewright_amd.synth import synthetic_frames
    t = torch.from_numpy(synthetic_frames(2, size[0], size[1], seed=seed)).cuda()
    return (t[0].flip(2).float() / 255.0).contiguous() if float_rgb else t


def _kinds():
    import nafblock_ref
    import restormer_block_ref
    from framewright_amd import aesrgan as A
    from framewright_amd import realesrgan as R
    from framewright_amd import restormer as RS
    from framewright_amd import rife as RF
    from framewright_amd import srvgg as SV
    from framewright_amd import tap_denoise as T
    from framewright_amd.synth import synthetic_attention_state, synthetic_ifnet_state, synthetic_nafnet_state, synthetic_rrdbnet_state

    naf = nafblock_ref.engine_args(32, 2)          # one block at level 0 (32 channels), one in the middle (128: both fused halves)
    rest = restormer_block_ref.ENGINE_ARGS         # one block per level, no refinement
    out = []
    for scale in (4, 2):
        for dtype in ("f16", "bf16"):
            out.append(Kind(f"rrdbnet-x{scale}-{dtype}", lambda scale=scale, dtype=dtype: R.RRDBNetEngine(num_block=1, scale=scale, dtype=dtype),
                            lambda scale=scale: (synthetic_rrdbnet_state(1, scale, seed=3),),
                            lambda e, size: e.upscale_device(_frame(size)[0]),
                            # the six single layers in the order of the network, then the body
                            lambda kind, have: "fw_rrdbnet_finalize: missing " + [k for k in ("conv_first", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last") if k not in have][0],
                            # phase form, pointwise form, f16: Winograd form (conv_hr and a dense block's conv5)
                            ["conv_up1", "conv_last", "conv_hr", "body.0.rdb2.conv5"]))
    out.append(Kind("srvgg", lambda: SV.SRVGGNetEngine(num_conv=1, scale=4), lambda: (SV.synthetic_srvgg_state(1, 4, seed=9),),
                    lambda e, size: e.upscale_device(_frame(size)[0]),
                    lambda kind, have: "fw_srvgg_finalize: missing tensors of body.2", ["body.2.weight"]))
    out.append(Kind("nafnet", lambda: T.NAFNetEngine(dtype="f16", **naf), lambda: (synthetic_nafnet_state(seed=7, **naf),),
                    lambda e, size: e.denoise_device(_frame(size)[0]),
                    lambda kind, have: "fw_nafnet_finalize: missing downs.0", ["middle_blks.0.conv1.weight"]))
    out.append(Kind("restormer", lambda: RS.RestormerEngine(dtype="f16", **rest), lambda: (RS.synthetic_restormer_state(seed=5, **rest),),
                    lambda e, size: e.denoise_device(_frame(size)[0]),
                    # (restormer.hip and aesrgan.hip walk a std::map of the expected keys: byte order, sorted() for these ASCII names)
                    lambda kind, have: "fw_restormer_finalize: missing " + sorted(k for k in kind.keys() if k not in have)[0],
                    ["encoder_level1.0.attn.qkv.weight"]))
    out.append(Kind("ifnet", lambda: RF.IFNetEngine("f16"), lambda: (synthetic_ifnet_state(),),
                    lambda e, size: e.interpolate_device(*_frame(size)),
                    lambda kind, have: "fw_ifnet_finalize: block2 is missing tensors", ["block3.convblock.0.conv.weight"]))
    out.append(Kind("aesrgan", lambda: A.AESRGANEngine(num_block=1, scale=2, num_attention=1),
                    lambda: (synthetic_rrdbnet_state(1, 4, seed=3), synthetic_attention_state(1, 1, seed=4)),
                    lambda e, size: e.forward_rgb(_frame(size, float_rgb=True)),
                    lambda kind, have: "fw_aesrgan_finalize: missing " + sorted(k for k in kind.keys() if k not in have)[0],
                    ["conv_hr.weight"],
                    # every conv of the x2 net, which has no conv_up2, and the attention block
                    tensors=lambda st: {**{k: v for k, v in st[0].items() if not k.startswith("conv_up2")}, **st[1]}))
    return out


NAMES = ["rrdbnet-x4-f16", "rrdbnet-x4-bf16", "rrdbnet-x2-f16", "rrdbnet-x2-bf16", "srvgg", "nafnet", "restormer", "ifnet", "aesrgan"]
TWICE = [(n, i) for n in NAMES for i in range(4 if n.startswith("rrdbnet") else 1)]


@pytest.fixture(scope="module")
def kinds(hip_lib):
    ks = {k.name: k for k in _kinds()}
    assert list(ks) == NAMES
    return ks


def _bytes(t):
    return t.cpu().numpy().tobytes()   # (the copy waits for the forward)


def _fresh(kind, size):
    """The forward of a handle that lives for this one call."""
    eng = kind.loaded()
    try:
        return _bytes(kind.forward(eng, size))
    finally:
        eng.close()


@pytest.fixture(scope="module")
def fresh(kinds):
    """The output of a fresh handle by (kind, size), computed once."""
    cache = {}

    def get(name, size):
        if (name, size) not in cache:
            cache[name, size] = _fresh(kinds[name], size)
        return cache[name, size]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_second_handle_in_the_same_process_gives_the_same_bytes(kinds, fresh, name):
    first = fresh(name, SMALL)
    assert len(first) > 0 and first != bytes(len(first))
    assert _fresh(kinds[name], SMALL) == first


@pytest.mark.parametrize("name", NAMES)
def test_destroy_a_loaded_handle_that_never_ran(kinds, name):
    eng = kinds[name].loaded()      # weights on the device, no workspace yet
    eng.close()
    assert not eng._h


@pytest.mark.parametrize("name", NAMES)
def test_destroy_a_handle_with_only_some_weights(kinds, name):
    from framewright_amd import _lib
    kind = kinds[name]
    eng = kind.make()
    try:
        keys = kind.keys()
        have = keys[:len(keys) // 2]
        for k in have:
            kind.set_raw(eng, k)
        with pytest.raises(_lib.FramewrightHipError) as e:
            kind.finalize(eng)
        assert e.value.code == _lib.FW_ERR_INVALID
        assert str(e.value) == kind.first_missing(kind, set(have))
    finally:
        eng.close()


@pytest.mark.parametrize("name,index", TWICE, ids=[f"{n}-{i}" for n, i in TWICE])
def test_a_weight_set_twice_is_the_weight_set_last(kinds, fresh, name, index):
    kind = kinds[name]
    key = kind.twice[index]
    eng = kind.make()
    try:
        once = fresh(name, SMALL)
        # on a new handle, then behind a forward: the second time the forms built at finalize (IFNet, Restormer, SRVGG, AESRGAN;
        # NAFNet's fused blocks) are on the device already and are built again
        for _ in range(2):
            kind.set_raw(eng, key, scale=0.5)      # other values first: their buffers go when the tensor is set again
            eng.load_state_dict(*kind.state())
            assert _bytes(kind.forward(eng, SMALL)) == once
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_workspace_that_grows_changes_no_byte(kinds, fresh, name):
    kind = kinds[name]
    eng = kind.loaded()
    try:
        assert _bytes(kind.forward(eng, SMALL)) == fresh(name, SMALL)
        assert _bytes(kind.forward(eng, LARGE)) == fresh(name, LARGE)
        assert _bytes(kind.forward(eng, SMALL)) == fresh(name, SMALL)    # the larger workspace serves the smaller frame
    finally:
        eng.close()
