"""bark.cpp_amd - MI355X-native Bark engine: HIP/C++ library (csrc/ -> lib/libbark.so) + this thin
ctypes mirror of its C API.

The directory name contains a dot, so import it through `load_package()` of the repo-root helper
`bark_amd_loader.py`, or put the directory itself on sys.path and `import api`.
"""
from . import voice  # noqa: F401
from .api import (BarkContext, Batcher, BarkContextParams, BarkHipAudioFormat, BarkHipAudioRender, BarkHipJoinParams, BarkHipLongParams, BarkHipLoudnessInfo,  # noqa: F401
                  BarkHipLoudnessParams, BarkHipStats, BarkHipVoicePrompt, audio_format, audio_render, build_library, default_params, flac_max_bytes, join_params, library_path,
                  load_library, loudness_params, speed_permille)
from .voice import VoicePrompt  # noqa: F401
