"""Frame deduplication on the device (kernel set K14, csrc/dedup_hash.hip).

The reference removes the repeated frames of a padded source (18 fps film in a 25 fps container) in front of its enhance step
(src/framewright/processors/deduplication.py; core/restorer.py step 5b): every frame gets a hash, a frame whose hash is close
enough to the last unique frame's is a duplicate, only unique frames are enhanced, and the sequence is rebuilt by repetition.  Its
hashes are Pillow thumbnails - a 17 x 16 gray Lanczos reduction compared column against column (dHash, when `imagehash` imports), or
the MD5 of every fourth byte of a 64 x 64 one (the pixel hash, otherwise) - computed per file on one host core.

`DeviceFrameDeduplicator` forms the same thumbnails on uint8 BGR frames that are already on the GPU (`fw_pil_thumb_u8`, Pillow's
integer resampler byte for byte; tests/dedup_ref.py is the contract) and downloads 32 or 4096 bytes per frame.  The decision loop
is `analyze_hashes`, the one place the comparison lives.  The dHash bit and hex conventions are restated from imagehash's
definition (imagehash parity unpinned).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import logging
import shutil
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._stage import Stage, check_stack, fetch, upload

logger = logging.getLogger(__name__)

PIXEL_THUMB = 64          # the pixel hash's thumbnail is 64 x 64 whatever the configuration


def _imagehash_importable() -> bool:
    try:
        import imagehash  # noqa: F401
        from PIL import Image  # noqa: F401
        return True
    except ImportError:
        return False


@dataclass
class DeduplicationResult:
    """What an analysis found: counts, the frame rate they suggest, and for every frame the unique frame that stands for it."""
    total_frames: int = 0
    unique_frames: int = 0
    duplicate_frames: int = 0
    detected_source_fps: float = 0.0
    target_fps: float = 25.0
    frame_mapping: Dict[int, int] = field(default_factory=dict)      # frame index -> index of its unique frame
    unique_indices: List[int] = field(default_factory=list)

    @property
    def duplication_ratio(self) -> float:
        return self.duplicate_frames / self.total_frames if self.total_frames else 0.0

    @property
    def estimated_original_fps(self) -> float:
        if self.unique_frames == 0 or self.total_frames == 0:
            return self.target_fps
        return self.target_fps * (self.unique_frames / self.total_frames)

    def summary(self) -> str:
        return (f"Frames: {self.unique_frames}/{self.total_frames} unique "
                f"({self.duplicate_frames} duplicates, {self.duplication_ratio:.1%} reduction)\n"
                f"Estimated original FPS: {self.estimated_original_fps:.1f} (target: {self.target_fps}fps)")


@dataclass
class DeduplicationConfig:
    similarity_threshold: float = 0.98      # a frame at least this similar to the last unique frame is a duplicate
    use_perceptual_hash: bool = True        # dHash when imagehash is there; else the pixel hash
    hash_size: int = 16
    pixel_sample_rate: int = 4              # the pixel hash takes every n-th byte of its thumbnail
    min_unique_ratio: float = 0.3           # below it the analysis warns
    expected_source_fps: Optional[float] = None


def hash_similarity(h1: str, h2: str, perceptual: bool, hash_size: int = 16) -> float:
    """1.0 for equal strings; for dHashes 1 - hamming / hash_size^2; for pixel hashes 0.0."""
    if h1 == h2:
        return 1.0
    if perceptual:
        try:
            return 1.0 - bin(int(h1, 16) ^ int(h2, 16)).count("1") / (hash_size * hash_size)
        except ValueError:
            pass
    return 0.0


def analyze_hashes(hashes: Sequence[str], config: Optional[DeduplicationConfig] = None, target_fps: float = 25.0,
                   perceptual: bool = True) -> DeduplicationResult:
    """The decision loop on a clip's hashes: frame 0 is unique; frame i is a duplicate of the LAST UNIQUE frame iff its similarity
    to it reaches the threshold, else it becomes the last unique frame."""
    config = config or DeduplicationConfig()
    total = len(hashes)
    if total == 0:
        return DeduplicationResult()
    result = DeduplicationResult(total_frames=total, target_fps=target_fps)
    unique, mapping = [0], {0: 0}
    last_hash, last_idx = hashes[0], 0
    for i in range(1, total):
        if hash_similarity(last_hash, hashes[i], perceptual, config.hash_size) >= config.similarity_threshold:
            mapping[i] = last_idx
        else:
            unique.append(i)
            mapping[i] = i
            last_hash, last_idx = hashes[i], i
    result.unique_frames = len(unique)
    result.duplicate_frames = total - len(unique)
    result.unique_indices = unique
    result.frame_mapping = mapping
    result.detected_source_fps = result.estimated_original_fps
    return result


def _bits_to_hex(row: bytes, hash_size: int) -> str:
    return format(int.from_bytes(row, "big"), "0%dx" % ((hash_size * hash_size + 3) // 4))


class DeviceFrameDeduplicator(Stage):
    """The reference's `FrameDeduplicator` with the hashes formed on one GPU.  ``imagehash_available`` selects the hash the
    reference would take: None probes the import as the reference does."""

    def __init__(self, config: Optional[DeduplicationConfig] = None, gpu_id: int = 0, imagehash_available: Optional[bool] = None):
        self.config = config or DeduplicationConfig()
        self.gpu_id = int(gpu_id)
        self.imagehash_available = _imagehash_importable() if imagehash_available is None else bool(imagehash_available)
        self._hash_cache: Dict[Path, str] = {}
        super().__init__(self.gpu_id, needs_gpu=False)     # the directory methods that only copy files need no GPU; the hashes do

    @property
    def perceptual(self) -> bool:
        return bool(self.imagehash_available and self.config.use_perceptual_hash)

    # ---- hashes ------------------------------------------------------------------------------------------------------------------
    def _thumbs(self, ptr: int, stride: int, n: int, h: int, w: int, out_w: int, out_h: int, gray_first: bool, dev):
        """Enqueue the thumbnails of n frames on torch's current stream of `dev`; returns the n x out_h x out_w device tensor."""
        import torch
        self.gpu_device()                      # the refusal of a machine without a GPU, put off by the constructor
        thumbs = torch.empty((n, out_h, out_w), dtype=torch.uint8, device=dev)
        ws = torch.empty(max(1, self._lib.fw_pil_thumb_workspace_bytes(n, h, w, out_w, out_h, int(gray_first))), dtype=torch.uint8, device=dev)
        _lib.check(self._lib.fw_pil_thumb_u8(C.c_void_p(ptr), stride, n, h, w, out_w, out_h, int(gray_first), _lib.ptr(thumbs),
                                             _lib.ptr(ws), _lib.stream_ptr(dev)))
        return thumbs

    def _hashes_of_clip(self, clip) -> List[str]:
        import torch
        n, h, w = (int(v) for v in clip.shape[:3])
        dev = clip.device
        if self.perceptual:
            hs = int(self.config.hash_size)
            thumbs = self._thumbs(clip.data_ptr(), h * w * 3, n, h, w, hs + 1, hs, True, dev)
            bits = torch.empty((n, (hs * hs + 7) // 8), dtype=torch.uint8, device=dev)
            _lib.check(self._lib.fw_dhash_pack_u8(_lib.ptr(thumbs), n, hs, _lib.ptr(bits), _lib.stream_ptr(dev)))
            return [_bits_to_hex(row.tobytes(), hs) for row in fetch(dev, bits)]
        thumbs = self._thumbs(clip.data_ptr(), h * w * 3, n, h, w, PIXEL_THUMB, PIXEL_THUMB, False, dev)
        rate = int(self.config.pixel_sample_rate)
        return [hashlib.md5(t.reshape(-1)[::rate].tobytes()).hexdigest() for t in fetch(dev, thumbs)]

    @_lib.on_tensor_device
    def hashes_device(self, frames) -> List[str]:
        """Hex hashes of a uint8 n x H x W x 3 CUDA tensor, or of a list of H x W x 3 CUDA tensors (stacked when they agree in size,
        else hashed one by one): one launch for the thumbnails, one more for the dHash bits, 32 or 4096 bytes per frame downloaded.
        The MD5 of the pixel hash is computed on the host."""
        import torch
        if isinstance(frames, torch.Tensor):
            check_stack(frames, 4, "hashes_device expects a uint8 CUDA tensor n x H x W x 3")
            return self._hashes_of_clip(frames.contiguous()) if frames.shape[0] else []
        frames = list(frames)
        for f in frames:
            check_stack(f, 3, "hashes_device expects uint8 CUDA tensors H x W x 3")
        if not frames:
            return []
        if all(f.shape == frames[0].shape and f.device == frames[0].device for f in frames):
            return self._hashes_of_clip(torch.stack(frames))
        return [self._hashes_of_clip(f.contiguous().unsqueeze(0))[0] for f in frames]

    def analyze_clip_device(self, frames, target_fps: float = 25.0) -> DeduplicationResult:
        return analyze_hashes(self.hashes_device(frames), self.config, target_fps, self.perceptual)

    def _hash_on_host(self, path: Path) -> str:
        """A file that is not 8-bit three-channel (L, P, RGBA, 16-bit): the reference's own Pillow lines, on the file."""
        from PIL import Image
        img = Image.open(path)
        if self.perceptual:
            hs = int(self.config.hash_size)
            px = np.asarray(img.convert("L").resize((hs + 1, hs), Image.Resampling.LANCZOS))
            bits = (px[:, 1:] > px[:, :-1]).reshape(-1)
            return _bits_to_hex(np.packbits(np.concatenate([np.zeros((-bits.size) % 8, bool), bits])).tobytes(), hs)
        px = np.asarray(img.resize((PIXEL_THUMB, PIXEL_THUMB), Image.Resampling.LANCZOS).convert("L")).reshape(-1)
        return hashlib.md5(px[::int(self.config.pixel_sample_rate)].tobytes()).hexdigest()

    # ---- directories -------------------------------------------------------------------------------------------------------------
    def analyze_frames(self, frames_dir: Path, target_fps: float = 25.0, progress_callback: Optional[Callable[[float], None]] = None,
                       block: int = 16) -> DeduplicationResult:
        """`frame_*.png` of a directory, sorted: each file is decoded once, 8-bit RGB frames are uploaded and hashed `block` at a
        time, anything else is hashed on the host.  Hashes are kept by path, so a second call decodes nothing."""
        from PIL import Image
        frames_dir = Path(frames_dir)
        files = sorted(frames_dir.glob("frame_*.png"))
        total = len(files)
        if total == 0:
            logger.warning(f"No frames found in {frames_dir}")
            return DeduplicationResult()
        logger.info(f"Analyzing {total} frames for duplicates...")
        pending: List[Tuple[Path, np.ndarray]] = []

        def flush():
            # frames of one size go up as one clip; a directory of mixed sizes falls apart into runs
            while pending:
                shape = pending[0][1].shape
                run = [p for p in pending if p[1].shape == shape]
                clip = upload(np.stack([a for _, a in run]), self._dev)
                for (path, _), h in zip(run, self.hashes_device(clip)):
                    self._hash_cache[path] = h
                pending[:] = [p for p in pending if p[1].shape != shape]

        for i, path in enumerate(files):
            if progress_callback and i and i % 100 == 0:
                progress_callback(i / total)
            if path in self._hash_cache:
                continue
            try:
                with Image.open(path) as img:
                    rgb = np.asarray(img) if img.mode == "RGB" else None
                if rgb is not None and rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3:
                    pending.append((path, np.ascontiguousarray(rgb[:, :, ::-1])))
                    if len(pending) >= max(1, int(block)):
                        flush()
                else:
                    self._hash_cache[path] = self._hash_on_host(path)
            except _lib.FramewrightHipError:
                raise
            except Exception as e:  # noqa: BLE001 - an unreadable file is a frame of its own, as in the reference
                logger.warning(f"Could not hash {path}: {e}")
                self._hash_cache[path] = hashlib.md5(str(path).encode()).hexdigest()
        flush()
        result = analyze_hashes([self._hash_cache[p] for p in files], self.config, target_fps, self.perceptual)
        if progress_callback:
            progress_callback(1.0)
        logger.info(result.summary())
        if result.unique_frames / total < self.config.min_unique_ratio:
            logger.warning(f"Very few unique frames detected ({result.unique_frames}/{total}). "
                           f"This may indicate incorrect threshold or non-duplicated content.")
        return result

    def extract_unique_frames(self, frames_dir: Path, output_dir: Path, result: Optional[DeduplicationResult] = None,
                              target_fps: float = 25.0,
                              progress_callback: Optional[Callable[[float], None]] = None) -> Tuple[Path, DeduplicationResult]:
        """Copies the unique frames to `output_dir` under their own names (the frame number is what the rebuild goes by)."""
        frames_dir, output_dir = Path(frames_dir), Path(output_dir)
        if result is None:
            result = self.analyze_frames(frames_dir, target_fps, progress_callback)
        if result.unique_frames == 0:
            raise ValueError("No unique frames detected")
        output_dir.mkdir(parents=True, exist_ok=True)
        files = sorted(frames_dir.glob("frame_*.png"))
        for i, idx in enumerate(result.unique_indices):
            if progress_callback and i % 50 == 0:
                progress_callback(i / len(result.unique_indices))
            shutil.copy2(files[idx], output_dir / files[idx].name)
        if progress_callback:
            progress_callback(1.0)
        return output_dir, result

    def reconstruct_sequence(self, enhanced_dir: Path, output_dir: Path, result: DeduplicationResult,
                             progress_callback: Optional[Callable[[float], None]] = None) -> Path:
        """The full sequence from enhanced unique frames: frame i is a copy of the enhanced file whose number is its unique frame's,
        or of the nearest number when that file is missing."""
        enhanced_dir, output_dir = Path(enhanced_dir), Path(output_dir)
        output_dir.mkdir(parents=True, exist_ok=True)
        enhanced = {int(f.stem.split("_")[-1]): f for f in enhanced_dir.glob("frame_*.png")}
        for i in range(result.total_frames):
            if progress_callback and i % 100 == 0:
                progress_callback(i / result.total_frames)
            key = result.frame_mapping.get(i, i)
            if key not in enhanced:
                key = min(enhanced.keys(), key=lambda k: abs(k - key))
            shutil.copy2(enhanced[key], output_dir / f"frame_{i:08d}.png")
        if progress_callback:
            progress_callback(1.0)
        return output_dir

    @staticmethod
    def reconstruct_device(enhanced: Sequence, result: DeduplicationResult) -> List:
        """The full sequence from the enhanced unique frames of a device clip (`enhanced[k]` belongs to `result.unique_indices[k]`):
        a duplicate's entry IS its unique frame's tensor - no copy is made."""
        if len(enhanced) != len(result.unique_indices):
            raise ValueError(f"{len(result.unique_indices)} enhanced frames expected, got {len(enhanced)}")
        by_index = dict(zip(result.unique_indices, enhanced))
        return [by_index[result.frame_mapping.get(i, i)] for i in range(result.total_frames)]


def detect_duplicate_frames(frames_dir: Path, target_fps: float = 25.0, similarity_threshold: float = 0.98) -> DeduplicationResult:
    return DeviceFrameDeduplicator(DeduplicationConfig(similarity_threshold=similarity_threshold)).analyze_frames(Path(frames_dir), target_fps)


def deduplicate_and_enhance(frames_dir: Path, unique_dir: Path, target_fps: float = 25.0,
                            similarity_threshold: float = 0.98) -> Tuple[Path, DeduplicationResult]:
    """Analyses `frames_dir` and leaves its unique frames in `unique_dir`, ready for the enhance step."""
    dd = DeviceFrameDeduplicator(DeduplicationConfig(similarity_threshold=similarity_threshold))
    return dd.extract_unique_frames(Path(frames_dir), Path(unique_dir), target_fps=target_fps)
