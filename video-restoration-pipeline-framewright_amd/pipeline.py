"""Device-resident hand-off between the three stages of the hot path.

The reference chains `tap_denoise -> enhance -> interpolate` through three PNG directories
(core/restorer.py:3217-3329: each stage reads every frame back from disk, decodes it, uploads it, downloads the result and
encodes it again).  Here a clip stays in HBM from the first upload to the last download: the stages exchange uint8 CUDA
tensors, and every stage is exactly the engine call its directory driver makes, so the result is bit-identical to running
the three drivers one after the other.
"""
from __future__ import annotations

from typing import Iterable, Iterator, List, Optional, Sequence

import numpy as np

from . import _lib, policy


class DeviceRestorationPipeline:
    """denoise (TAPDenoiser) -> upscale (RRDBNetEngine / SRVGGNetEngine) -> interpolate (IFNetEngine), any stage optional.

    ``interp_passes`` x2 passes of frame interpolation (1 -> 2n-1 frames, 2 -> 4n-3, ...), as
    `FrameInterpolator.interpolate` runs them for a fps ratio (`policy.interpolation_exponent`).

    ``deduplicator`` (a `dedup.DeviceFrameDeduplicator`; opt-in) analyses the clip that enters the upscale stage, as the reference
    deduplicates what its enhancer reads: only unique frames are upscaled, the sequence is rebuilt by repetition before the
    interpolation, and the analysis is kept as ``last_dedup_result``.  `run_device` / `run` only.

    ``color_grader`` (a `color_grade.DeviceColorGrader`; opt-in) grades every output frame behind the interpolation, where the
    reference has its seasonal grade (step 7c), into new tensors; it is elementwise, so the streaming forms have it too.

    ``deinterlacer`` (a `deinterlace.DeviceDeinterlacer`; opt-in) deinterlaces the input frames in front of every other stage with
    its configured method and field order (BOB doubles the frame count downstream).  The streaming forms keep one frame of
    lookahead for BWDIF and refuse `FieldOrder.AUTO` (a stream has no "first 20 frames"); with an explicit order they equal
    `run_device`.

    ``vhs_processor`` (a `vhs.DeviceVHSProcessor`; opt-in) runs its `process` on the input frames behind the deinterlacer and in front
    of every other stage; the streaming forms use its `stream`, which keeps `temporal_radius` frames on both sides for the dropout
    repair and equals `run_device`.

    ``aspect_handler`` (an `aspect.DeviceAspectHandler`; opt-in) with ``crop_bars`` crops letterbox and pillarbox bars off the input
    frames (`crop_letterbox`: the analysis of the first 20 frames decides for the clip) behind the deinterlacer and the VHS processor -
    an odd crop offset in front of the deinterlacer would swap the field parity, and the VHS analysis reads the bottom rows of the full
    frame - and in front of every other stage, so the networks never see the bars.  With ``aspect_target`` (a ratio as the
    reference's `convert_aspect` takes it) the output frames are converted with the handler's configured method and fill behind the
    colour grade, so the padding is not graded.  The streaming forms hold back the first min(20, n) frames for the analysis
    (`DeviceAspectHandler.stream`) and equal `run_device`.

    ``input_quality_scorer`` and ``quality_scorer`` (each a `quality.DeviceFrameQualityScorer`; opt-in) score the frames as they enter,
    in front of the deinterlacer, and the final frames, behind the aspect conversion; the frames themselves pass through as they are.
    The reports are kept as ``last_input_quality_report`` and ``last_quality_report`` (timestamps from ``quality_fps``; 0 gives the
    reference's timestamp 0).  The streaming forms score each frame as it passes (`DeviceFrameQualityScorer.stream`: a few kilobytes of
    integers a frame are kept, never the frame) and build each report when its stream ends; a generator that is abandoned leaves None.

    ``hdr_converter`` (an `hdr.DeviceHDRConverter`; opt-in) is the last step: behind the colour grade, the aspect conversion and
    ``quality_scorer``, which scores the 8-bit frames, every output frame is converted to a new uint16 PQ / HLG tensor.  It is
    elementwise apart from the frame's own CLAHE histograms, so the streaming forms have it too, and `run_stream`'s pinned ring
    takes the frames' type.  `close` releases it, and every other stage that has a `close`.

    ``artifact_remover`` (a `qp_artifacts.DeviceQPArtifactRemover`; opt-in) removes compression artifacts from the input frames behind
    the bar crop and in front of the denoiser, where the reference has its step 5c in front of 5d, with the quantisation parameter
    ``artifact_qp`` (None: the remover's `manual_qp`, then 28).  It works frame by frame and its dither is keyed by the frame's position
    in the clip, so the streaming forms (`DeviceQPArtifactRemover.stream`) equal `run_device`.

    ``frame_generator`` (a `frame_generation.DeviceMissingFrameGenerator`; opt-in) fills the gaps in the frame numbering behind the
    denoiser and in front of the upscale and its deduplicator, where the reference has its step 5f, when the call names the frames'
    numbers (``frame_numbers``; ``expected_frames`` adds the gap behind the last frame).  The numbers are those of the frames that
    reach the generator, so a stage in front that changes the frame count (BOB deinterlacing) does not go with them.  Without
    ``frame_numbers`` nothing is filled.  The streaming forms take the numbers as a parallel iterable, hold back one frame
    (`DeviceMissingFrameGenerator.stream`) and equal `run_device`.

    ``temporal_consistency`` (a `temporal_consistency.DeviceTemporalConsistencyProcessor`; opt-in) de-flickers the final frames behind
    the interpolation and in front of the colour grade, where the reference has its step 7b: `apply_device` on the clip, which lists
    the scene cuts (one wait) and passes the frames around a cut through as they are.  The streaming forms use its `stream`, which
    is `attention_window // 2 + 1` frames behind its input and equals `run_device`.

    ``perceptual_tuner`` (a `perceptual.DevicePerceptualTuner`; opt-in) applies the perceptual look (denoise, unsharp mask,
    saturation, CLAHE detail, grain) to the final frames behind the temporal-consistency pass and in front of the colour grade, into
    new tensors.  Every step reads one frame, so the streaming forms have it too and hold nothing back.
    """

    def __init__(self, denoiser=None, upscaler=None, interpolator=None, interp_passes: int = 1, deduplicator=None, color_grader=None,
                 deinterlacer=None, vhs_processor=None, aspect_handler=None, aspect_target=None, crop_bars: bool = True,
                 quality_scorer=None, input_quality_scorer=None, quality_fps: float = 0.0, hdr_converter=None, artifact_remover=None,
                 artifact_qp=None, frame_generator=None, expected_frames=None, temporal_consistency=None, perceptual_tuner=None):
        self.denoiser, self.upscaler, self.interpolator = denoiser, upscaler, interpolator
        self.interp_passes = int(interp_passes)
        self.deduplicator = deduplicator
        self.last_dedup_result = None
        self.color_grader = color_grader
        self.deinterlacer = deinterlacer
        self.vhs_processor = vhs_processor
        self.aspect_handler, self.aspect_target, self.crop_bars = aspect_handler, aspect_target, bool(crop_bars)
        self.quality_scorer, self.input_quality_scorer, self.quality_fps = quality_scorer, input_quality_scorer, float(quality_fps)
        self.last_quality_report = self.last_input_quality_report = None
        self.hdr_converter = hdr_converter
        self.artifact_remover, self.artifact_qp = artifact_remover, artifact_qp
        self.frame_generator, self.expected_frames = frame_generator, expected_frames
        self.temporal_consistency = temporal_consistency
        self.perceptual_tuner = perceptual_tuner

    def _stages(self) -> tuple:
        """Every configured stage slot, in the order `_device` asks them: a new stage adds its name here."""
        return (self.interpolator, self.upscaler, self.denoiser, self.color_grader, self.deinterlacer, self.vhs_processor,
                self.aspect_handler, self.quality_scorer, self.input_quality_scorer, self.hdr_converter, self.artifact_remover, self.frame_generator,
                self.temporal_consistency, self.perceptual_tuner)

    def close(self) -> None:
        """Closes every stage that can be closed (the engines free their native handles, the HDR converter its tables)."""
        for stage in self._stages():
            if stage is not None and callable(getattr(stage, "close", None)):
                stage.close()

    def _keep_report(self, name: str):
        return lambda report: setattr(self, name, report)

    @classmethod
    def for_fps(cls, denoiser, upscaler, interpolator, source_fps: float, target_fps: float) -> "DeviceRestorationPipeline":
        return cls(denoiser, upscaler, interpolator, policy.interpolation_exponent(target_fps / source_fps))

    def run_device(self, frames: Sequence, frame_numbers: Optional[Sequence[int]] = None) -> List:
        """frames: uint8 BGR H x W x 3, numpy arrays or CUDA tensors.  Returns uint8 CUDA tensors (still on the device; the
        work is queued on torch's current stream).  ``frame_numbers``: the frames' numbers, for the ``frame_generator``."""
        import torch
        dev = self._device()

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a.contiguous()

        self.last_quality_report = self.last_input_quality_report = None
        with torch.cuda.device(dev):
            cur = [up(f) for f in frames]
            if self.input_quality_scorer is not None:
                self.last_input_quality_report = self.input_quality_scorer.analyze_frames(cur, self.quality_fps)
            if self.deinterlacer is not None:
                cur = list(self.deinterlacer.deinterlace(cur))
            if self.vhs_processor is not None:
                cur = list(self.vhs_processor.process(cur))
            if self.aspect_handler is not None and self.crop_bars:
                cur = list(self.aspect_handler.crop_letterbox(cur))
            if self.artifact_remover is not None:
                cur = self.artifact_remover.process_device(cur, self.artifact_qp)
            if self.denoiser is not None:
                cur = self.denoiser.denoise_clip_device(cur)
            if self.frame_generator is not None and frame_numbers is not None:
                cur = self.frame_generator.fill_device(cur, frame_numbers, self.expected_frames)[0]
            if self.upscaler is not None and self.deduplicator is not None and cur:
                self.last_dedup_result = res = self.deduplicator.analyze_clip_device(cur)
                cur = self.deduplicator.reconstruct_device([self.upscaler.upscale_device(cur[i]) for i in res.unique_indices], res)
            elif self.upscaler is not None:
                cur = [self.upscaler.upscale_device(f) for f in cur]
            if self.interpolator is not None:
                for _ in range(self.interp_passes):
                    nxt = []
                    for i, f in enumerate(cur):
                        nxt.append(f)
                        if i + 1 < len(cur):
                            nxt.append(self.interpolator.interpolate_device(f, cur[i + 1]))
                    cur = nxt
            if self.temporal_consistency is not None:
                cur = self.temporal_consistency.apply_device(cur)
            if self.perceptual_tuner is not None:
                cur = self.perceptual_tuner.apply_device(cur)  # new tensors: a repeated frame may be one tensor several times
            if self.color_grader is not None:
                cur = self.color_grader.apply_device(cur)      # new tensors: a repeated frame may be one tensor several times
            if self.aspect_handler is not None and self.aspect_target is not None:
                cur = list(self.aspect_handler.convert_aspect(cur, self.aspect_target))
            if self.quality_scorer is not None:
                self.last_quality_report = self.quality_scorer.analyze_frames(cur, self.quality_fps)
            if self.hdr_converter is not None:
                cur = self.hdr_converter.convert_device(cur)   # new uint16 tensors: a repeated frame may be one tensor several times
        return cur

    def run(self, frames: Sequence, frame_numbers: Optional[Sequence[int]] = None) -> List[np.ndarray]:
        import torch
        out = self.run_device(frames, frame_numbers)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    # ---- streaming form: the codec edge (codec.py) ---------------------------------------------------------------------------
    def _device(self):
        """The device the stages live on, for `run_device` and the streaming path alike: the interpolator's, else the upscaler's
        (the two never sit on different devices; where both are set the later stage names it, as `run_device` always had it), else
        the first of denoiser, colour grader, deinterlacer, VHS processor, aspect handler, the two quality scorers, the HDR converter, the
        artifact remover, the frame generator, the temporal-consistency processor, the perceptual tuner.
        Every stage answers through `_lib.owner_device`: a new stage adds its name to `_stages`."""
        for stage in self._stages():
            dev = _lib.owner_device(stage)
            if dev is not None:
                return dev
        raise ValueError("DeviceRestorationPipeline: no stage configured")

    def _gen_denoise(self, frames: Iterator, block: int):
        """The temporal-window stage over a stream: every frame goes through the network once (`denoise_only_device`), and a block's
        windows are formed as soon as the `window // 2` frames behind it have been denoised too - the neighbours of a block are
        handed to `denoise_clip_device` as already-denoised halos, exactly what the multi-GPU block partition does between ranks
        (sharding.py), so the frames equal the whole-clip call bit for bit and the stage holds `block + window` frames, not the clip."""
        half = self.denoiser.config.temporal_window // 2
        tail: List = []                      # the last `half` denoised frames in front of the block
        raw: List = []
        den: List = []
        eof = False
        it = iter(frames)
        while True:
            while not eof and len(raw) < block + half:
                chunk = []
                for f in it:
                    chunk.append(f)
                    if len(raw) + len(chunk) >= block + half:
                        break
                else:
                    eof = True
                if chunk:
                    den += self.denoiser.denoise_only_device(chunk)
                    raw += chunk
            if not raw:
                return
            n_out = len(raw) if eof else block
            yield from self.denoiser.denoise_clip_device(raw[:n_out], halo_before=tail, halo_after=den[n_out:n_out + half], denoised=den[:n_out])
            tail = (tail + den[:n_out])[-half:] if half else []
            raw, den = raw[n_out:], den[n_out:]

    def _gen_interp(self, frames: Iterator):
        prev = None
        for f in frames:
            if prev is not None:
                yield prev
                yield self.interpolator.interpolate_device(prev, f)
            prev = f
        if prev is not None:
            yield prev

    def stream_device(self, frames: Iterable, block: int = 8, frame_numbers: Optional[Iterable[int]] = None):
        """Generator form of `run_device` for clips that do not fit (or have not arrived) in memory: ``frames`` is any iterator of
        uint8 BGR frames (numpy - e.g. `codec.RawVideoReader` - or CUDA tensors); yields the output frames, uint8 CUDA tensors, in
        order, as soon as their inputs allow.  Identical frames to `run_device` on the whole clip - without a ``deduplicator``:
        deduplication needs the clip's hashes in front of the upscale stage and is not part of the streaming form, which upscales
        every frame.  ``frame_numbers``: the frames' numbers, in step with ``frames``, for the ``frame_generator``."""
        import torch
        dev = self._device()
        if block < 1:
            raise ValueError("block must be >= 1")
        if self.deinterlacer is not None and self.deinterlacer.config.field_order.value == "auto":
            raise ValueError("FieldOrder.AUTO needs the clip's first 20 frames: give the streaming forms an explicit field order")
        upload = torch.cuda.Stream(device=dev)

        def gen_up():
            for a in frames:
                if isinstance(a, np.ndarray):
                    # on a stream of its own and waited for on the host (a 6 MB copy): the reader reuses its slot two frames later,
                    # while the compute stream may still be tens of frames behind the host
                    with torch.cuda.stream(upload):
                        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(upload)
                    ev.synchronize()
                    t.record_stream(torch.cuda.current_stream(dev))
                    yield t
                else:
                    yield a.contiguous()

        self.last_quality_report = self.last_input_quality_report = None
        with torch.cuda.device(dev):
            g = gen_up()
            if self.input_quality_scorer is not None:
                g = self.input_quality_scorer.stream(g, self.quality_fps, self._keep_report("last_input_quality_report"))
            if self.deinterlacer is not None:
                g = self.deinterlacer.stream(g, block=block)
            if self.vhs_processor is not None:
                g = self.vhs_processor.stream(g, block=block)
            if self.aspect_handler is not None and self.crop_bars:
                g = self.aspect_handler.stream(g, block=block)
            if self.artifact_remover is not None:
                g = self.artifact_remover.stream(g, self.artifact_qp)
            if self.denoiser is not None:
                g = self._gen_denoise(g, block)
            if self.frame_generator is not None and frame_numbers is not None:
                g = (f for _, f in self.frame_generator.stream(zip(frame_numbers, g), self.expected_frames))
            if self.upscaler is not None:
                g = (self.upscaler.upscale_device(f) for f in g)
            if self.interpolator is not None:
                for _ in range(self.interp_passes):
                    g = self._gen_interp(g)
            if self.temporal_consistency is not None:
                g = self.temporal_consistency.stream(g)
            if self.perceptual_tuner is not None:
                g = self.perceptual_tuner.stream(g)
            if self.color_grader is not None:
                g = (self.color_grader.apply_device([f])[0] for f in g)
            if self.aspect_handler is not None and self.aspect_target is not None:
                g = (self.aspect_handler.convert_aspect([f], self.aspect_target)[0] for f in g)
            if self.quality_scorer is not None:
                g = self.quality_scorer.stream(g, self.quality_fps, self._keep_report("last_quality_report"))
            if self.hdr_converter is not None:
                g = self.hdr_converter.stream(g)
            yield from g

    def run_stream(self, frames: Iterable, writer, block: int = 8, slots: int = 3, frame_numbers: Optional[Iterable[int]] = None) -> int:
        """``frames`` (e.g. a `codec.RawVideoReader` on the decoder's pipe) through the stages into ``writer`` (a
        `codec.RawVideoWriter` on the encoder's pipe): decode, GPU stages, download and encode overlap - the reader thread runs
        ahead of this thread, finished frames leave through a ring of ``slots`` pinned buffers on a download stream, and the writer
        thread waits for each download before it writes.  The writer's bounded queue is the back-pressure.  Returns the number of
        frames written (the caller closes reader and writer)."""
        import queue as _queue

        import torch
        dev = self._device()
        down = torch.cuda.Stream(device=dev)
        pins: Optional[list] = None
        free: "_queue.Queue[int]" = _queue.Queue()
        n = 0
        with torch.cuda.device(dev):
            for t in self.stream_device(frames, block, frame_numbers):
                if pins is None:
                    pins = [torch.empty(tuple(t.shape), dtype=t.dtype).pin_memory() for _ in range(max(2, int(slots)))]
                    for k in range(len(pins)):
                        free.put(k)
                k = free.get()                       # every slot with the writer: wait for it (back-pressure)
                ev_c = torch.cuda.Event()
                ev_c.record(torch.cuda.current_stream(dev))
                with torch.cuda.stream(down):
                    down.wait_event(ev_c)
                    pins[k].copy_(t, non_blocking=True)
                    ev_d = torch.cuda.Event()
                    ev_d.record(down)
                t.record_stream(down)
                writer.write(pins[k].numpy(), ready=ev_d.synchronize, release=lambda k=k: free.put(k))
                n += 1
        return n
