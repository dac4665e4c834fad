"""Compression-artifact removal on the device, the classical path (kernel set K21, csrc/qp_artifacts.hip).

The reference's `processors/qp_artifact_removal.py` cleans codec damage between frame extraction and the TAP denoise (step 5c).  What
it executes on any machine without the unpublished ARCNN / DnCNN weights is its `opencv` backend: a bilateral filter and a
block-boundary blend against blocking, a Canny-guided local smoothing against ringing, a masked dither against banding, each scaled by
a strength that follows the quantisation parameter.  `DeviceQPArtifactRemover` runs that path on uint8 BGR frames that are already on
the GPU (`fw_qp_artifacts_u8`); tests/qp_artifact_ref.py is the contract, byte for byte.

The tables a transcendental function goes into (the bilateral's colour and space weights, the 15-tap Gaussian, the normal quantiles of
the dither) are built here on the host in float64, once per strength, and uploaded.

Dither noise.  The reference draws it from numpy's global generator, so its output is not reproducible as it stands.  Here the noise
is an input: an explicit float32 plane per frame, or - the default - a counter-based generator keyed by (`QPArtifactConfig.seed`, frame
index, pixel, channel) that is bit-reproducible on host and device.  Its 65536-entry quantile table ends at +-4.32 sigma.

Not built: the ARCNN / DnCNN engines and `neural_untrained` (`use_neural` is accepted and ignored: there are no published weights, and
the reference's own fallback runs a randomly initialised net); 16-bit and gray frames; effective strengths above 1, where the
reference's ringing blend is no longer convex and casts negative floats to uint8 - the config is accepted as the reference accepts
it, the frame call refuses the (qp, multiplier) pair.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import shutil
import subprocess
import time
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from statistics import NormalDist
from typing import Callable, Iterable, Iterator, List, Optional

import numpy as np

from . import _lib
from ._stage import Stage, check_frame_list, check_no_overlap, check_out, contiguous, fetch, upload

logger = logging.getLogger(__name__)

MAX_SIDE = 16384
DEFAULT_QP = 28                                  # the reference's "default assumption for web video"
TYPE_BITS = {"blocking": 1, "ringing": 2, "banding": 4}
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


class ArtifactType(Enum):
    BLOCKING = "blocking"
    RINGING = "ringing"
    BANDING = "banding"
    MOSQUITO = "mosquito"
    ALL = "all"


class CompressionLevel(Enum):
    LIGHT = "light"          # QP < 23
    MODERATE = "moderate"    # QP 23-32
    HEAVY = "heavy"          # QP 32-40
    SEVERE = "severe"        # QP > 40


@dataclass
class QPArtifactConfig:
    """The reference's fields, defaults and validation, plus ``seed`` for the counter-based dither.  ``use_neural`` is accepted and
    ignored (see the module docstring); ``preserve_edges`` and ``preserve_texture`` play no part in the frame path (they do not in the
    reference either)."""
    auto_detect_qp: bool = True
    manual_qp: Optional[int] = None
    strength_multiplier: float = 1.0
    artifact_types: List[ArtifactType] = field(default_factory=lambda: [ArtifactType.ALL])
    block_size: int = 8
    preserve_edges: bool = True
    preserve_texture: bool = True
    gpu_id: int = 0
    use_neural: bool = True
    seed: int = 0

    def __post_init__(self) -> None:
        if not 0.1 <= self.strength_multiplier <= 3.0:
            raise ValueError(f"strength_multiplier must be 0.1-3.0, got {self.strength_multiplier}")
        if self.block_size not in [4, 8, 16, 32]:
            raise ValueError(f"block_size must be 4, 8, 16, or 32, got {self.block_size}")
        if self.manual_qp is not None and not 0 <= self.manual_qp <= 51:
            raise ValueError(f"manual_qp must be 0-51, got {self.manual_qp}")


@dataclass
class QPArtifactResult:
    frames_processed: int = 0
    frames_failed: int = 0
    output_dir: Optional[Path] = None
    detected_qp: Optional[int] = None
    compression_level: Optional[CompressionLevel] = None
    processing_time_seconds: float = 0.0
    artifacts_removed: List[str] = field(default_factory=list)


# ---- host tables ----------------------------------------------------------------------------------------------------------------------
def blocking_params(strength):
    """(d, sigma_color, sigma_space) of `_remove_blocking_opencv`."""
    return int(5 + strength * 10), 30 + strength * 70, 30 + strength * 70


def bilateral_tables(d: int, sigma_color: float, sigma_space: float):
    """(colour float32 [768], space float32 [2r+1][2r+1]) of cv2.bilateralFilter, computed in float64; r = max(d // 2, 1)."""
    r = max(int(d) // 2, 1)
    k = np.arange(768, dtype=np.float64)
    color = np.exp(k * k * (-0.5 / (np.float64(sigma_color) * np.float64(sigma_color)))).astype(np.float32)
    i = np.arange(-r, r + 1, dtype=np.float64)
    rr = i[:, None] ** 2 + i[None, :] ** 2
    space = np.where(rr <= r * r, np.exp(rr * (-0.5 / (np.float64(sigma_space) * np.float64(sigma_space)))), 0.0).astype(np.float32)
    return color, space


def gaussian15_coeffs() -> np.ndarray:
    """cv2.getGaussianKernel(15, 0) as float32: sigma 0.3 * ((15 - 1) * 0.5 - 1) + 0.8 = 2.6."""
    sigma = 0.3 * ((15 - 1) * 0.5 - 1) + 0.8
    x = np.arange(15, dtype=np.float64) - 7.0
    c = np.exp(-0.5 / (sigma * sigma) * x * x)
    return (c * (1.0 / c.sum())).astype(np.float32)


_QUANTILES: Optional[np.ndarray] = None


def normal_quantiles() -> np.ndarray:
    """float64 [65536]: the standard-normal quantile at (k + 0.5) / 65536 (built once a process)."""
    global _QUANTILES
    if _QUANTILES is None:
        nd = NormalDist()
        _QUANTILES = np.array([nd.inv_cdf((k + 0.5) / 65536.0) for k in range(65536)], dtype=np.float64)
    return _QUANTILES


def noise_table(strength) -> np.ndarray:
    """float32 [65536]: the quantiles times the reference's standard deviation 1 + strength * 2."""
    return (normal_quantiles() * (1 + np.float64(strength) * 2)).astype(np.float32)


def frame_key(seed: int, frame_index: int) -> int:
    """The 64-bit key of one frame's dither: mix64(seed * golden + frame index), modulo 2^64 (the splitmix64 finaliser)."""
    z = ((int(seed) & _M64) * _GOLDEN + (int(frame_index) & _M64)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def type_mask(artifact_types) -> int:
    names = [getattr(t, "value", t) for t in artifact_types]
    if "all" in names:
        return 7
    return sum(bit for name, bit in TYPE_BITS.items() if name in names)


# ---- image files (the directory driver's defaults) ------------------------------------------------------------------------------------
def _read_image(path: Path) -> Optional[np.ndarray]:
    """`cv2.imread(path)` where cv2 is present, else 8-bit BGR through Pillow; None for what cannot be read."""
    try:
        import cv2
        return cv2.imread(str(path))
    except ImportError:
        from PIL import Image
        try:
            with Image.open(str(path)) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])
        except Exception:  # noqa: BLE001 - cv2.imread returns None for what it cannot read
            return None


def _write_image(path: Path, frame: np.ndarray) -> None:
    try:
        import cv2
        cv2.imwrite(str(path), frame)
    except ImportError:
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(frame[:, :, ::-1])).save(str(path))


class DeviceQPArtifactRemover(Stage):
    """The reference's `QPArtifactRemover` frame path (backend 'opencv') on uint8 BGR CUDA frames of one GPU; the results are new
    tensors and the inputs are left as they are.  Work is queued on torch's current stream of the frames' device; with the ringing
    step every frame waits once for that stream (the Canny hysteresis reads its round flags on the host)."""

    def __init__(self, config: Optional[QPArtifactConfig] = None, gpu_id: Optional[int] = None):
        self.config = config or QPArtifactConfig()
        self.gpu_id = int(self.config.gpu_id if gpu_id is None else gpu_id)
        super().__init__(self.gpu_id, needs_gpu=False)       # the host methods (QP detection, the level ladder) need no GPU
        self._tables = {}                                    # float(strength) -> (d, colour, space, noise table) on the device
        self._gauss15 = gaussian15_coeffs()
        self._wrong = "qp_artifacts: uint8 CUDA tensors H x W x 3 (BGR) expected"
        self._wrong_noise = "qp_artifacts: noise as float32 CUDA tensors H x W x 3 on the frames' device expected, one per frame"
        self._closed = False

    def is_available(self) -> bool:
        return not self._closed

    def close(self) -> None:
        """Releases the tables and the scratch; frame calls that arrive afterwards raise."""
        self._closed = True
        self._tables, self._scratch = {}, None

    def clear_cache(self) -> None:
        self._tables, self._scratch = {}, None

    # ---- the reference's host methods ------------------------------------------------------------------------------------------
    def compression_level(self, qp: int) -> CompressionLevel:
        if qp < 23:
            return CompressionLevel.LIGHT
        if qp < 32:
            return CompressionLevel.MODERATE
        if qp < 40:
            return CompressionLevel.HEAVY
        return CompressionLevel.SEVERE

    def strength_for_qp(self, qp: int):
        """`_get_strength_for_qp`: a numpy.float64, as it comes out of np.clip."""
        base_strength = (qp - 15) / 35.0
        base_strength = np.clip(base_strength, 0.1, 1.0)
        return base_strength * self.config.strength_multiplier

    def resolve_qp(self, qp: Optional[int]) -> int:
        if qp is None:
            qp = self.config.manual_qp
        if qp is None:
            qp = DEFAULT_QP
        return qp

    def detect_qp_from_video(self, video_path, run: Callable = subprocess.run) -> Optional[int]:
        """The reference's two ffprobe queries: the mean QP of the first 50 frames, else an estimate from the bits per pixel at an
        assumed 30 fps; None where both fail.  ``run`` replaces subprocess.run."""
        video_path = Path(video_path)
        if not video_path.exists():
            logger.warning(f"Video file not found: {video_path}")
            return None
        try:
            cmd = ["ffprobe", "-v", "quiet", "-select_streams", "v:0", "-show_entries", "frame=pict_type,qp", "-of", "json",
                   "-read_intervals", "%+#50", str(video_path)]
            result = run(cmd, capture_output=True, text=True, timeout=30)
            if result.returncode == 0:
                data = json.loads(result.stdout)
                qp_values = [int(f["qp"]) for f in data.get("frames", []) if f.get("qp") is not None]
                if qp_values:
                    avg_qp = int(np.mean(qp_values))
                    logger.info(f"Detected average QP: {avg_qp} (from {len(qp_values)} frames)")
                    return avg_qp
            cmd = ["ffprobe", "-v", "quiet", "-select_streams", "v:0", "-show_entries", "stream=bit_rate,width,height", "-of", "json",
                   str(video_path)]
            result = run(cmd, capture_output=True, text=True, timeout=30)
            if result.returncode == 0:
                streams = json.loads(result.stdout).get("streams", [])
                if streams:
                    stream = streams[0]
                    bitrate = int(stream.get("bit_rate", 0))
                    width, height = int(stream.get("width", 1920)), int(stream.get("height", 1080))
                    if bitrate > 0:
                        bpp = bitrate / (width * height * 30)
                        estimated_qp = 18 if bpp > 0.5 else 23 if bpp > 0.2 else 28 if bpp > 0.1 else 34 if bpp > 0.05 else 40
                        logger.info(f"Estimated QP from bitrate: {estimated_qp} (bpp: {bpp:.3f})")
                        return estimated_qp
        except subprocess.TimeoutExpired:
            logger.warning("FFprobe timed out during QP detection")
        except Exception as e:  # noqa: BLE001 - the reference logs and returns None
            logger.warning(f"Failed to detect QP: {e}")
        return None

    # ---- frames ----------------------------------------------------------------------------------------------------------------
    def _strength(self, qp: int):
        strength = self.strength_for_qp(qp)
        if not strength <= 1.0:
            raise ValueError(f"qp_artifacts: strength {float(strength):.4g} (qp {qp} x multiplier {self.config.strength_multiplier}) is above 1: "
                             "the reference's ringing blend leaves 0 .. 255 there")
        return strength

    def _tables_for(self, strength, dev):
        key = (float(strength), str(dev))
        if key not in self._tables:
            d, sigma_color, sigma_space = blocking_params(strength)
            color, space = bilateral_tables(d, sigma_color, sigma_space)
            self._tables[key] = (d, upload(color, dev), upload(space, dev), upload(noise_table(strength), dev))
        return self._tables[key]

    @_lib.on_tensor_device
    def process_device(self, frames, qp: Optional[int] = None, noise=None, first_index: int = 0, out=None) -> list:
        """A list of uint8 H x W x 3 BGR CUDA tensors of one shape -> a list of new tensors (or ``out``: as many contiguous uint8
        tensors of that shape, none of which overlaps a frame).  ``qp`` falls back to `manual_qp`, then 28.  ``noise``: one float32
        H x W x 3 CUDA tensor per frame for the dither of the banding step; None draws it from the counter generator with the
        config's seed and the frame index ``first_index + i``."""
        import torch
        if self._closed:
            raise ValueError("qp_artifacts: the remover is closed")
        frames = list(frames)
        if not frames:
            return []
        dev = self.gpu_device()
        h, w, _ = check_frame_list(frames, self._wrong, [(1, MAX_SIDE, 1, MAX_SIDE, "qp_artifacts: frames of 1 .. 16384 pixels a side expected")],
                                   dev=dev, wrong_device=f"qp_artifacts: frames on cuda:{self.gpu_id}, the remover's device, expected")
        if frames[0].dim() != 3:
            raise ValueError(self._wrong)
        qp = self.resolve_qp(qp)
        strength = self._strength(qp)
        mask = type_mask(self.config.artifact_types)
        if noise is not None:
            noise = list(noise) if isinstance(noise, (list, tuple)) else [noise]
            if len(noise) != len(frames):
                raise ValueError(self._wrong_noise)
            for t in noise:
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != (h, w, 3):
                    raise ValueError(self._wrong_noise)
            noise = contiguous(noise)
        frames = contiguous(frames)
        if out is None:
            outs = _lib.empty_like_many(frames)              # one allocation for a clip
        else:
            outs = list(out)
            if len(outs) != len(frames):
                raise ValueError("qp_artifacts: one destination per frame expected")
            for o in outs:
                check_out(o, "qp_artifacts: contiguous uint8 destinations of the frames' shape on their device expected", torch.uint8, dev,
                          shape=frames[0].shape)
            check_no_overlap(outs, frames, "qp_artifacts")
        d, color, space, table = self._tables_for(strength, dev)
        scratch = self.scratch(int(self._lib.fw_qp_artifacts_scratch_bytes(h, w)), dev)
        st = _lib.stream_ptr(dev)
        g15 = self._gauss15.ctypes.data_as(C.c_void_p)
        for i, (f, o) in enumerate(zip(frames, outs)):
            plane = noise[i] if noise is not None else None
            _lib.check(self._lib.fw_qp_artifacts_u8(_lib.ptr(f), _lib.ptr(o), h, w, 3, d, _lib.ptr(color), _lib.ptr(space), g15, float(strength),
                                                    int(self.config.block_size), mask, _lib.ptr(plane), _lib.ptr(table),
                                                    frame_key(self.config.seed, first_index + i), _lib.ptr(scratch), st))
        return outs

    def process_frame(self, frame, qp: Optional[int] = None, noise=None, index: int = 0):
        return self.process_device([frame], qp, None if noise is None else [noise], index)[0]

    def stream(self, frames: Iterable, qp: Optional[int] = None) -> Iterator:
        """Yields the cleaned frame of every frame of an iterator, in order, with no lookahead; the position in the stream is the
        frame index of the dither, so the frames equal `process_device` on the whole clip."""
        for i, f in enumerate(frames):
            yield self.process_device([f], qp, None, i)[0]

    def process(self, frames, qp: Optional[int] = None, noise=None, first_index: int = 0) -> List[np.ndarray]:
        """Host in, host out: uint8 H x W x 3 arrays (and float32 noise planes, if any) -> uint8 arrays."""
        frames = [np.ascontiguousarray(f) for f in frames]
        for a in frames:
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("qp_artifacts: uint8 arrays H x W x 3 (BGR) expected")
        if not frames:
            return []
        with self.host() as dev:
            planes = None if noise is None else [upload(np.asarray(p), dev) for p in noise]
            outs = self.process_device([upload(a, dev) for a in frames], qp, planes, first_index)
            got = fetch(dev, *outs)
            return [got] if len(outs) == 1 else list(got)

    # ---- the primitives alone (what tests/test_qp_artifacts_gpu.py holds to tests/qp_artifact_ref.py) ----------------------------
    def _one_frame(self, frame):
        if self._closed:
            raise ValueError("qp_artifacts: the remover is closed")
        dev = self.gpu_device()
        h, w, _ = check_frame_list([frame], self._wrong, [(1, MAX_SIDE, 1, MAX_SIDE, "qp_artifacts: frames of 1 .. 16384 pixels a side expected")],
                                   dev=dev, wrong_device=f"qp_artifacts: frames on cuda:{self.gpu_id}, the remover's device, expected")
        if frame.dim() != 3:
            raise ValueError(self._wrong)
        return frame.contiguous(), h, w, dev

    @_lib.on_tensor_device
    def bilateral(self, frame, d: int, sigma_color: float, sigma_space: float):
        """cv2.bilateralFilter(frame, d, sigma_color, sigma_space) as tests/qp_artifact_ref.py states it; d 2 .. 15."""
        import torch
        frame, h, w, dev = self._one_frame(frame)
        color, space = bilateral_tables(d, sigma_color, sigma_space)
        color, space = upload(color, dev), upload(space, dev)
        out = torch.empty_like(frame)
        _lib.check(self._lib.fw_bilateral_u8c3(_lib.ptr(frame), _lib.ptr(out), h, w, 3, int(d), _lib.ptr(color), _lib.ptr(space), _lib.stream_ptr(dev)))
        return out

    @_lib.on_tensor_device
    def gaussian5(self, frame):
        """cv2.GaussianBlur(frame, (5, 5), 0) on uint8 BGR: exact fixed point."""
        import torch
        frame, h, w, dev = self._one_frame(frame)
        out = torch.empty_like(frame)
        _lib.check(self._lib.fw_gaussian5_u8(_lib.ptr(frame), _lib.ptr(out), h, w, 3, _lib.stream_ptr(dev)))
        return out

    # ---- the reference's directory driver --------------------------------------------------------------------------------------
    def remove_artifacts(self, input_dir, output_dir, detected_qp: Optional[int] = None,
                         progress_callback: Optional[Callable[[float], None]] = None, read: Optional[Callable] = None,
                         write: Optional[Callable] = None) -> QPArtifactResult:
        """`QPArtifactRemover.remove_artifacts`: every `*.png` of ``input_dir`` (else every `*.jpg`), sorted, is read, cleaned and
        written under its own name into ``output_dir``.  A frame that cannot be read counts as failed; one whose processing or writing
        raises counts as failed and is copied as it is.  ``read(path) -> array or None`` and ``write(path, array)`` replace cv2's
        imread and imwrite.  The position in the sorted list is the frame index of the dither."""
        result = QPArtifactResult()
        start_time = time.time()
        if not self.is_available():
            logger.error("QP artifact removal not available")
            return result
        qp = detected_qp
        if qp is None:
            qp = self.config.manual_qp
        if qp is None:
            qp = DEFAULT_QP
            logger.warning(f"No QP detected, using default: {qp}")
        result.detected_qp = qp
        result.compression_level = self.compression_level(qp)
        output_dir = Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        result.output_dir = output_dir
        input_dir = Path(input_dir)
        read, write = read or _read_image, write or _write_image
        frame_files = sorted(input_dir.glob("*.png"))
        if not frame_files:
            frame_files = sorted(input_dir.glob("*.jpg"))
        if not frame_files:
            logger.warning(f"No frames found in {input_dir}")
            return result
        total_frames = len(frame_files)
        logger.info(f"QP artifact removal: {total_frames} frames, QP={qp} ({result.compression_level.value}), "
                    f"strength={self.strength_for_qp(qp):.2f}")
        for i, frame_file in enumerate(frame_files):
            try:
                frame = read(frame_file)
                if frame is None:
                    logger.warning(f"Failed to read frame: {frame_file}")
                    result.frames_failed += 1
                    continue
                processed = self.process([frame], qp=qp, first_index=i)[0]
                write(output_dir / frame_file.name, processed)
                result.frames_processed += 1
            except Exception as e:  # noqa: BLE001 - the reference copies the frame and goes on
                logger.error(f"Failed to process {frame_file}: {e}")
                result.frames_failed += 1
                try:
                    shutil.copy2(frame_file, output_dir / frame_file.name)
                except Exception:  # noqa: BLE001
                    pass
            if progress_callback:
                progress_callback((i + 1) / total_frames)
        result.processing_time_seconds = time.time() - start_time
        result.artifacts_removed = [at.value for at in self.config.artifact_types]
        logger.info(f"QP artifact removal complete: {result.frames_processed}/{total_frames} frames, "
                    f"time: {result.processing_time_seconds:.1f}s")
        return result


def create_qp_artifact_remover(auto_detect: bool = True, strength: float = 1.0, use_neural: bool = True,
                               gpu_id: int = 0) -> DeviceQPArtifactRemover:
    config = QPArtifactConfig(auto_detect_qp=auto_detect, strength_multiplier=strength, use_neural=use_neural, gpu_id=gpu_id)
    return DeviceQPArtifactRemover(config)
