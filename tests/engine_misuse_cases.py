"""Misuse of the six network engines (NAFNet, RRDBNet, IFNet, Restormer, SRVGG, AESRGAN) and the frames they produce, shared by
tools/gen_engine_misuse_golden.py (which records what the package answers) and tests/test_engine_misuse_gpu.py (which replays them
against tests/golden/engine_misuse.json and tests/golden/engine_outputs.json).

Every engine is built at the smallest configuration the suite uses, frames are 40 x 56.  A misuse case is
``(engine, label, call, literal)``: ``call(ctx)`` makes the one wrong call and its answer is the exception's class name, ``str(e)``
and ``e.code`` where it has one, or a description of the value returned.  ``literal`` is ``None`` for a case whose answer is the
recording; the few cases that carry a literal answer are deliberate differences from the recording, written out here.
An output case is ``(label, call)``: ``call(ctx)`` returns the frames whose bytes are digested.
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch

from framewright_amd import _lib
from framewright_amd import aesrgan as A
from framewright_amd import realesrgan as R
from framewright_amd import restormer as RS
from framewright_amd import rife as RF
from framewright_amd import srvgg as SV
from framewright_amd import tap_denoise as T
from framewright_amd.synth import (synthetic_attention_state, synthetic_frames, synthetic_ifnet_state, synthetic_nafnet_state,
                                   synthetic_rrdbnet_state)

H, W = 40, 56
NAF = dict(width=32, middle_blk_num=1, enc_blk_nums=(1, 1), dec_blk_nums=(1, 1))
REST = dict(dim=48, num_blocks=(1, 1, 1, 1), num_refinement_blocks=1)
DTYPE_MESSAGE = f"dtype must be one of {sorted(_lib.DTYPES)}"


class Kind:
    """One engine kind: how to build it, its weights, and its device and host forwards."""

    def __init__(self, name, make, state, device, host, scale=1, device_dtype=torch.uint8, checks_out=True, has_clone=False):
        self.name, self.make, self._state, self.device, self.host = name, make, state, device, host
        # checks_out: the device forward takes ``out`` / ``out_rgb_f32`` and refuses a wrong one.  NAFNet and Restormer hand them to
        # the library unchecked, where a buffer that is too small would be written past its end: no such call is listed for them
        self.scale, self.device_dtype, self.checks_out, self.has_clone = scale, device_dtype, checks_out, has_clone
        self._cached = None

    def state(self) -> tuple:
        """The arguments of ``load_state_dict``, generated once."""
        if self._cached is None:
            self._cached = self._state()
        return self._cached

    def loaded(self):
        eng = self.make()
        eng.load_state_dict(*self.state())
        return eng


KINDS = {k.name: k for k in (
    Kind("NAFNetEngine", lambda dtype="f16", **kw: T.NAFNetEngine(dtype=dtype, **{**NAF, **kw}),
         lambda: (synthetic_nafnet_state(seed=7, **NAF),),
         lambda e, t, **kw: e.denoise_device(t, **kw), lambda e, a: e.denoise(a), checks_out=False, has_clone=True),
    Kind("RRDBNetEngine", lambda dtype="f16", **kw: R.RRDBNetEngine(**{**dict(num_block=2, scale=2), **kw}, dtype=dtype),
         lambda: (synthetic_rrdbnet_state(2, 2, seed=3),),
         lambda e, t, **kw: e.upscale_device(t, **kw), lambda e, a: e.upscale(a), scale=2),
    Kind("IFNetEngine", lambda dtype="f16": RF.IFNetEngine(dtype),
         lambda: (synthetic_ifnet_state(),),
         lambda e, t, **kw: e.interpolate_device(t, t.flip(0).contiguous() if t.dim() == 3 and t.is_contiguous() else t, **kw),
         lambda e, a: e.interpolate(a, a[::-1]), has_clone=True),
    Kind("RestormerEngine", lambda dtype="f16", **kw: RS.RestormerEngine(dtype=dtype, **{**REST, **kw}),
         lambda: (RS.synthetic_restormer_state(seed=5, **REST),),
         lambda e, t, **kw: e.denoise_device(t, **kw), lambda e, a: e.denoise(a), checks_out=False, has_clone=True),
    Kind("SRVGGNetEngine", lambda dtype="f16", **kw: SV.SRVGGNetEngine(**{**dict(num_conv=16, scale=4), **kw}, dtype=dtype),
         lambda: (SV.synthetic_srvgg_state(16, 4, seed=9),),
         lambda e, t, **kw: e.upscale_device(t, **kw), lambda e, a: e.upscale(a), scale=4),
    Kind("AESRGANEngine", lambda dtype="f16", **kw: A.AESRGANEngine(**{**dict(num_block=2, scale=2, num_attention=1), **kw}, dtype=dtype),
         lambda: (synthetic_rrdbnet_state(2, 4, seed=3), synthetic_attention_state(2, 1, seed=4)),
         lambda e, t, **kw: e.forward_rgb(t, **kw), lambda e, a: e.enhance(a), scale=2, device_dtype=torch.float32, checks_out=False),
)}


class Context:
    """What the cases share: one loaded engine per kind (never closed by a case) and the test frames."""

    def __init__(self):
        self._loaded = {}
        self.frames = synthetic_frames(6, H, W, seed=21)

    def loaded(self, name):
        if name not in self._loaded:
            self._loaded[name] = KINDS[name].loaded()
        return self._loaded[name]

    def frame(self, name, i=0):
        """Frame ``i`` as the device forward of ``name`` takes it (uint8 BGR; float32 RGB in [0, 1] for AESRGAN)."""
        t = torch.from_numpy(self.frames[i]).cuda()
        return t if KINDS[name].device_dtype == torch.uint8 else t.flip(2).float() / 255.0

    def close(self):
        for e in self._loaded.values():
            e.close()
        self._loaded = {}


def describe(v) -> str:
    if isinstance(v, torch.Tensor):
        return f"tensor {v.dtype} {tuple(v.shape)} {v.device.type}"
    if isinstance(v, np.ndarray):
        return f"array {v.dtype} {v.shape}"
    return repr(v)


def answer(call, ctx) -> dict:
    try:
        v = call(ctx)
    except Exception as e:  # noqa: BLE001 - the exception is the answer
        r = {"raises": type(e).__name__, "message": str(e)}
        if hasattr(e, "code"):
            r["code"] = e.code
        return r
    return {"returns": describe(v)}


def _without_one_key(state: tuple) -> tuple:
    first = dict(state[0])
    del first[sorted(first)[len(first) // 2]]
    return (first,) + state[1:]


def _one_wrong_shape(state: tuple) -> tuple:
    first = dict(state[0])
    key = sorted(first)[len(first) // 2]
    first[key] = np.zeros(tuple(first[key].shape) + (2,), np.float32)
    return (first,) + state[1:]


def _closed(kind):
    eng = kind.loaded()
    eng.close()
    return eng


def misuse_cases() -> list:
    out: list = []

    def add(engine, label, call, literal=None):
        out.append((engine, label, call, literal))

    # ---- structural arguments of the constructors
    add("NAFNetEngine", "enc and dec of different length", lambda c: KINDS["NAFNetEngine"].make(enc_blk_nums=(1,)))
    add("NAFNetEngine", "width 48", lambda c: KINDS["NAFNetEngine"].make(width=48))
    add("RRDBNetEngine", "scale 3", lambda c: KINDS["RRDBNetEngine"].make(scale=3))
    add("RestormerEngine", "dim 64", lambda c: KINDS["RestormerEngine"].make(dim=64))
    add("RestormerEngine", "24 channels per head", lambda c: KINDS["RestormerEngine"].make(heads=(2, 2, 4, 8)))
    add("SRVGGNetEngine", "scale 5", lambda c: KINDS["SRVGGNetEngine"].make(scale=5))
    add("AESRGANEngine", "scale 3", lambda c: KINDS["AESRGANEngine"].make(scale=3))
    add("AESRGANEngine", "more attention blocks than RRDBs", lambda c: KINDS["AESRGANEngine"].make(num_attention=3))
    # ---- deliberate differences from the recording ("Engine owners (Python)"): literal answers
    add("NAFNetEngine", "unknown dtype", lambda c: KINDS["NAFNetEngine"].make("f8"), {"raises": "ValueError", "message": DTYPE_MESSAGE})
    add("SRVGGNetEngine", "has __del__", lambda c: hasattr(SV.SRVGGNetEngine, "__del__"), {"returns": "True"})
    add("AESRGANEngine", "has __del__", lambda c: hasattr(A.AESRGANEngine, "__del__"), {"returns": "True"})

    for name, k in KINDS.items():
        def dev(c, t, k=k, name=name, **kw):
            return k.device(c.loaded(name), t, **kw)

        if name != "NAFNetEngine":
            add(name, "unknown dtype", lambda c, k=k: k.make("f8"))
        add(name, "load_state_dict with one key missing", lambda c, k=k: k.make().load_state_dict(*_without_one_key(k.state())))
        add(name, "load_state_dict with one tensor of the wrong shape", lambda c, k=k: k.make().load_state_dict(*_one_wrong_shape(k.state())))
        add(name, "device forward before weights", lambda c, k=k, name=name: k.device(k.make(), c.frame(name)))
        add(name, "host forward before weights", lambda c, k=k: k.host(k.make(), c.frames[0]))
        wrong = torch.float32 if k.device_dtype == torch.uint8 else torch.uint8
        add(name, f"device forward with a {str(wrong).split('.')[1]} tensor", lambda c, name=name, dev=dev, wrong=wrong: dev(c, c.frame(name).to(wrong)))
        add(name, "device forward with a non-contiguous view", lambda c, name=name, dev=dev: dev(c, c.frame(name)[:, ::2]))
        add(name, "device forward with a 2-D tensor", lambda c, name=name, dev=dev: dev(c, c.frame(name)[:, :, 0].contiguous()))
        add(name, "device forward with 4 channels",
            lambda c, name=name, dev=dev: dev(c, torch.cat([c.frame(name), c.frame(name)[:, :, :1]], dim=2).contiguous()))
        add(name, "device forward with a host tensor", lambda c, name=name, dev=dev: dev(c, c.frame(name).cpu()))
        if k.checks_out:
            s = k.scale
            add(name, "out of the wrong shape",
                lambda c, name=name, dev=dev, s=s: dev(c, c.frame(name), out=torch.empty((H * s, W * s + 1, 3), dtype=torch.uint8, device="cuda")))
            add(name, "out_rgb_f32 of the wrong dtype",
                lambda c, name=name, dev=dev, s=s: dev(c, c.frame(name), out_rgb_f32=torch.empty((H * s, W * s, 3), dtype=torch.float16, device="cuda")))
        add(name, "host forward with a float array", lambda c, k=k, name=name: k.host(c.loaded(name), c.frames[0].astype(np.float32)))
        add(name, "host forward with a 2-D array", lambda c, k=k, name=name: k.host(c.loaded(name), c.frames[0][:, :, 0]))
        if k.has_clone:
            add(name, "clone before weights", lambda c, k=k: k.make().clone())
        add(name, "device forward after close", lambda c, k=k, name=name: k.device(_closed(k), c.frame(name)))
        add(name, "host forward after close", lambda c, k=k: k.host(_closed(k), c.frames[0]))
        if name not in ("RestormerEngine", "AESRGANEngine"):     # the two without flops()
            add(name, "flops after close", lambda c, k=k: _closed(k).flops(H, W))
        add(name, "close twice", lambda c, k=k: _closed(k).close())
    add("RestormerEngine", "device forward at 40 x 60",
        lambda c: KINDS["RestormerEngine"].device(c.loaded("RestormerEngine"), torch.zeros((40, 60, 3), dtype=torch.uint8, device="cuda")))
    add("RestormerEngine", "host forward at 40 x 60",
        lambda c: KINDS["RestormerEngine"].host(c.loaded("RestormerEngine"), np.zeros((40, 60, 3), np.uint8)))
    add("IFNetEngine", "frames of two sizes",
        lambda c: c.loaded("IFNetEngine").interpolate_device(c.frame("IFNetEngine"), c.frame("IFNetEngine")[:32].contiguous()))
    return out


# ---- frames -------------------------------------------------------------------------------------------------------------------------
def digest(frames) -> str:
    """sha256 over the bytes of the frames (tensors or arrays), in order, each preceded by its dtype and shape."""
    h = hashlib.sha256()
    for f in (frames if isinstance(frames, (list, tuple)) else [frames]):
        a = np.ascontiguousarray(f.cpu().numpy() if isinstance(f, torch.Tensor) else f)
        h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _tap(ctx, **config):
    return T.TAPDenoiser(T.TAPDenoiseConfig(model="nafnet", **config), engine=KINDS["NAFNetEngine"].loaded())


def _pairs(c):
    eng = KINDS["IFNetEngine"].loaded()
    try:
        fr = [torch.from_numpy(f).cuda() for f in c.frames]
        outs = eng.interpolate_pairs_device([(fr[i], fr[i + 1]) for i in range(5)])
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]
    finally:
        eng.close()


def _frames_fan_out(c):
    dn = _tap(c, tile_size=0)
    try:
        outs = dn.denoise_only_device([torch.from_numpy(f).cuda() for f in c.frames[:5]])
        torch.cuda.synchronize()
        return [o.cpu() for o in outs]
    finally:
        dn.clear_cache()


def _tiled(c):
    dn = _tap(c, tile_size=32, tile_overlap=8)
    try:
        out = dn._denoise_frame_tiled_device(torch.from_numpy(synthetic_frames(1, 72, 88, seed=22)[0]).cuda())
        torch.cuda.synchronize()
        return out.cpu()
    finally:
        dn.clear_cache()


def output_cases() -> list:
    out: list = []
    for name, k in KINDS.items():
        out.append((f"{name} device forward", lambda c, k=k, name=name: k.device(c.loaded(name), c.frame(name))))
        out.append((f"{name} host forward", lambda c, k=k, name=name: k.host(c.loaded(name), c.frames[0])))
    out.append(("interpolate_pairs_device on 5 pairs", _pairs))
    out.append(("denoise_only_device on 5 whole frames", _frames_fan_out))
    out.append(("_denoise_frame_tiled_device on 72 x 88 with 32-pixel tiles", _tiled))
    return out


def record_outputs(ctx) -> dict:
    got = {}
    for label, call in output_cases():
        v = call(ctx)
        torch.cuda.synchronize()
        got[label] = digest(v)
    return got
