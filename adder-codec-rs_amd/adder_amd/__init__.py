"""adder_amd -- Python plumbing over the MI355X framed->ADDER C-ABI (libadder_hip.so).

The compute path is the HIP library; this package only moves pointers around
(ctypes, torch device memory, torch.distributed) so that tests and bench.py can
drive it.  The C++ mirror of the reference's Source/Video/Encoder surface lives in
../host/.
"""
from ._native import (  # noqa: F401
    AdderHipError, AdderHipParams, AdderFramerParams, AdderCompressedParams, EVENT_DTYPE, SPARSE_STEP_DTYPE, FRAMER_FEATURE_DTYPE, LIB_PATH,
    TIME_DELTA_T, TIME_ABSOLUTE_T, TIME_MIXED, MULTI_NORMAL, MULTI_COLLAPSE,
    CONTENT_STATIC, CONTENT_NOISE, CONTENT_SCENE, D_EMPTY, D_ZERO_INTEGRATION, D_MAX, C_NONE,
    KERNEL_LEAN, KERNEL_GENERIC, KERNEL_CONTINUOUS, KERNEL_BOUNDED, KERNEL_CONSTANT_RUNS, KERNEL_RUN_RECORDS, KERNEL_LEAN_RUNS, KERNEL_LEAN_RUNS_PACKED,
    KERNEL_NAMES, VIEW_INTENSITY, VIEW_D, VIEW_DELTA_T, VIEW_SAE, SHOW_FEATURES_OFF, SHOW_FEATURES_INSTANT, SHOW_FEATURES_HOLD,
    OK, E_BAD_PARAMS, E_HIP, E_NO_DEVICE, E_OUT_CAPACITY, E_ARENA_DEPTH, E_TIMEOUT, E_POISONED,
)
from .video import CRF, crf_feature_radius, practical_d_max_exact, HipVideo, raw_header, raw_events, raw_eof, synth_clip_device  # noqa: F401
from .framer import HipFramer, contiguous_run_segments, FRAMED_U8, DVS, FRAME_U8, FRAME_U16, FRAME_U32  # noqa: F401
from .compressed import CompressedEncoder, compressed_decode  # noqa: F401
from .quality import calculate_quality_metrics, calculate_mse, calculate_psnr, HipQuality  # noqa: F401
from . import quality as _quality
from . import dvs as _dvs
from .dvs import HipDvs, adder_to_dvs_file, DVS_EVENT_DTYPE, DAT_DTYPE  # noqa: F401
from . import prophesee as _prophesee
from .prophesee import HipProphesee, prophesee_to_adder_file  # noqa: F401
from . import stream_tools as _stream_tools
from .stream_tools import HipStreamMigrator, HipStreamInfo, migrate_file, adder_info_file  # noqa: F401
from . import player as _player
from .player import HipPlayer, play_file  # noqa: F401
from . import viz_player as _viz_player
from .viz_player import HipVizPlayer, viz_play_file  # noqa: F401
from . import color as _color
from .color import to_gray_device, to_gray_host  # noqa: F401
from . import davis as _davis
from .davis import HipDavis, davis_to_adder, davis_to_adder_file, DAVIS_EVENT_DTYPE  # noqa: F401
from . import fast_eval as _fast_eval
from .fast_eval import HipFastEval  # noqa: F401
from . import compressed_model as _compressed_model
from .compressed_model import HipCompressedModel, compress_events_device  # noqa: F401


def load():
    """Loads libadder_hip.so and binds every symbol include/adder_hip.h, adder_framer.h, adder_compressed.h,
    adder_dvs.h, adder_quality.h, adder_prophesee.h, adder_stream.h, adder_player.h, adder_viz_player.h, adder_color.h, adder_davis.h and adder_fast.h declare;
    raises if one is missing."""
    L = _native.load()
    _dvs.load()
    _prophesee.load()
    _quality.load()
    _stream_tools.load()
    _player.load()
    _viz_player.load()
    _color.load()
    _davis.load()
    _fast_eval.load()
    _compressed_model.load()
    return L
