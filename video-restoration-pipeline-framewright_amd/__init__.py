"""framewright_amd — MI355X-native engine for FrameWright's per-frame conv-net hot path.

Host code is Python (the reference is Python); all arithmetic runs in hand-written gfx950 HIP kernels reached
through the C-ABI of ``lib/libframewright_hip.so`` (``include/framewright_hip.h``).  There is no CPU fallback:
importing the operator modules works anywhere, but creating an engine without the library or without a GPU
raises ``FramewrightHipError``.
"""
__version__ = "0.1.0"

from .dedup import (DeduplicationConfig, DeduplicationResult, DeviceFrameDeduplicator, analyze_hashes,  # noqa: E402,F401
                    deduplicate_and_enhance, detect_duplicate_frames)
from .color_grade import (LUT, DeviceColorGrader, LUTType, combine_luts, create_contrast_lut,  # noqa: E402,F401
                          create_film_emulation_lut, create_identity_lut, create_seasonal_lut, read_cube, write_cube)
from .quality import DeviceFrameQualityScorer, FrameScore, QualityIssue, QualityReport  # noqa: E402,F401
from .hdr import (ColorSpace, DeviceHDRConverter, HDRConfig, HDRConversionResult, HDRFormat, ToneMapping,  # noqa: E402,F401
                  create_hdr_converter)
from .qp_artifacts import (ArtifactType, CompressionLevel, DeviceQPArtifactRemover, QPArtifactConfig, QPArtifactResult,  # noqa: E402,F401
                           create_qp_artifact_remover)
from .frame_generation import (DeviceMissingFrameGenerator, FrameGenerationConfig, FrameGenerationResult, GapInfo,  # noqa: E402,F401
                               GenerationModel, create_frame_generator)
from .temporal_consistency import (CrossAttentionConfig, DeviceTemporalConsistencyProcessor, TemporalConsistencyResult,  # noqa: E402,F401
                                   TemporalMethod, create_temporal_processor)
from .perceptual import (DevicePerceptualTuner, PerceptualConfig, PerceptualMode, PerceptualProfile,  # noqa: E402,F401
                         create_perceptual_tuner, get_perceptual_profile)
