"""ctypes mirror of libbark.so (include/bark.h + include/bark_mi355x.h).

Names, argument meaning and error behaviour follow the reference C API
(/root/reference/bark.h:148-240): `BarkContext.load_model` <-> bark_load_model,
`generate_audio` <-> bark_generate_audio, `audio_data` <-> bark_get_audio_data[_size], ...
There is NO fallback: if the HIP library is missing or no GPU is present, loading raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

PROGRESS_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p)


class BarkContextParams(C.Structure):
    """struct bark_context_params (bark.h:81-141) - field order is ABI."""
    _fields_ = [
        ("verbosity", C.c_int), ("temp", C.c_float), ("fine_temp", C.c_float), ("min_eos_p", C.c_float),
        ("sliding_window_size", C.c_int32), ("max_coarse_history", C.c_int32), ("sample_rate", C.c_int32),
        ("target_bandwidth", C.c_int32), ("cls_token_id", C.c_int32), ("sep_token_id", C.c_int32),
        ("n_steps_text_encoder", C.c_int32), ("text_pad_token", C.c_int32), ("text_encoding_offset", C.c_int32),
        ("semantic_rate_hz", C.c_float), ("semantic_pad_token", C.c_int32), ("semantic_vocab_size", C.c_int32),
        ("semantic_infer_token", C.c_int32), ("coarse_rate_hz", C.c_float), ("coarse_infer_token", C.c_int32),
        ("coarse_semantic_pad_token", C.c_int32), ("n_coarse_codebooks", C.c_int32), ("n_fine_codebooks", C.c_int32),
        ("codebook_size", C.c_int32), ("progress_callback", PROGRESS_CB), ("progress_callback_user_data", C.c_void_p),
    ]


class BarkHipRequestParams(C.Structure):
    """struct bark_hip_request_params (bark_mi355x.h): what an utterance of a lock-step job may set for itself."""
    _fields_ = [("temp", C.c_float), ("fine_temp", C.c_float), ("min_eos_p", C.c_float), ("n_steps_text_encoder", C.c_int32), ("seed", C.c_uint32)]


class BarkHipSamplingFilter(C.Structure):
    """struct bark_hip_sampling_filter (bark_mi355x.h): top-k / nucleus filter of the semantic and coarse samples (rule C8n); {0, 1.0}: off."""
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float)]


class BarkHipSampleCall(C.Structure):
    """struct bark_hip_sample_call (bark_mi355x.h): per-call settings of the sampler hook bark_hip_sample_rows_state."""
    _fields_ = [("mode", C.c_int32), ("eos_token", C.c_int32), ("token_base", C.c_int32), ("prescaled", C.c_int32), ("n_past_add", C.c_int32),
                ("per_row", C.c_int32)]


class BarkHipVoicePrompt(C.Structure):
    """struct bark_hip_voice_prompt (bark_mi355x.h): speaker history of the three stages (rule C10v), time-major arrays."""
    _fields_ = [("semantic", C.c_void_p), ("n_semantic", C.c_int32), ("coarse_Tx2", C.c_void_p), ("n_coarse_frames", C.c_int32),
                ("fine_Tx8", C.c_void_p), ("n_fine_frames", C.c_int32)]


class BarkHipAudioFormat(C.Structure):
    """struct bark_hip_audio_format (bark_mi355x.h): output rate and sample format of an answer (rule C14r); {24000, SAMPLE_F32}: what the engine makes."""
    _fields_ = [("sample_rate", C.c_int32), ("sample_format", C.c_int32)]


class BarkHipJoinParams(C.Structure):
    """struct bark_hip_join_params (bark_mi355x.h): gaps, fade and trim of the long-form join (rule C15j); {6000, 0, 0.0, 0}: the defaults."""
    _fields_ = [("gap_samples", C.c_int32), ("fade_samples", C.c_int32), ("trim_threshold", C.c_float), ("trim_pad_frames", C.c_int32)]


class BarkHipLongParams(C.Structure):
    """struct bark_hip_long_params (bark_mi355x.h): the splitter's budget (rule C15s), chaining and the join of bark_hip_generate_long."""
    _fields_ = [("max_tokens", C.c_int32), ("chain", C.c_int32), ("join", BarkHipJoinParams)]


def join_params(gap_samples: int = 6000, fade_samples: int = 0, trim_threshold: float = 0.0, trim_pad_frames: int = 0) -> BarkHipJoinParams:
    return BarkHipJoinParams(int(gap_samples), int(fade_samples), float(trim_threshold), int(trim_pad_frames))


SPLIT_MAX_CHUNKS = 64
SAMPLE_F32, SAMPLE_S16, SAMPLE_MULAW, SAMPLE_FLAC = 0, 1, 2, 3          # enum bark_hip_sample_format
SAMPLE_FORMATS = {"f32": SAMPLE_F32, "s16": SAMPLE_S16, "mulaw": SAMPLE_MULAW}
CONTAINER_FORMATS = {"flac": SAMPLE_FLAC}                                # enum bark_hip_container_format: a stream over the s16 samples (rule C18f)
SAMPLE_DTYPES = {SAMPLE_F32: np.float32, SAMPLE_S16: np.int16, SAMPLE_MULAW: np.uint8, SAMPLE_FLAC: np.uint8}       # "flac": the bytes of a complete stream (rule C18f)
FLAC_BLOCK = 4096                                                        # samples per frame


def audio_format(rate: int = 24000, fmt="f32") -> BarkHipAudioFormat:
    """fmt: "f32" | "s16" | "mulaw" | "flac" (the routes that render a held result and the collector; rule C18f), or the enum's value"""
    return BarkHipAudioFormat(int(rate), (CONTAINER_FORMATS[fmt] if fmt in CONTAINER_FORMATS else SAMPLE_FORMATS[fmt]) if isinstance(fmt, str) else int(fmt))


def flac_max_bytes(n: int) -> int:
    """The size no FLAC stream of n samples exceeds (bark_hip_flac_max_bytes), or -1 for n outside 1 .. 2^26."""
    return int(load_library().bark_hip_flac_max_bytes(int(n)))


def speed_permille(speed) -> int:
    """A speaking rate as the C interface takes it: lround(1000 speed), as bark_batch_server converts its "speed" field."""
    return int(math.floor(1000.0 * float(speed) + 0.5))


class BarkHipLoudnessParams(C.Structure):
    """struct bark_hip_loudness_params (bark_mi355x.h): the target in hundredths of a LUFS (0: off), the peak ceiling and the gain cap (rule C17l)."""
    _fields_ = [("target_centilufs", C.c_int32), ("peak_ceiling", C.c_float), ("max_gain", C.c_float)]


class BarkHipLoudnessInfo(C.Structure):
    """struct bark_hip_loudness_info (bark_mi355x.h): what the device measured of a recording and the gain it applied."""
    _fields_ = [("mean_square", C.c_double), ("lufs", C.c_double), ("peak", C.c_float), ("gain", C.c_float), ("n_blocks", C.c_int32), ("n_abs", C.c_int32),
                ("n_gated", C.c_int32), ("flags", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BarkHipAudioRender(C.Structure):
    """struct bark_hip_audio_render (bark_mi355x.h): rate and format, speaking rate, levelling of a held result."""
    _fields_ = [("fmt", BarkHipAudioFormat), ("speed_permille", C.c_int32), ("loudness", BarkHipLoudnessParams)]


LOUDNESS_UNMEASURABLE, LOUDNESS_CAP_BOUND, LOUDNESS_CEILING_BOUND = 1, 2, 4          # flags of bark_hip_loudness_info
LOUDNESS_PEAK_CEILING, LOUDNESS_MAX_GAIN = 1.0, 10.0                                  # the defaults, bark_batch_server's too: full scale, +20 dB


def loudness_params(lufs=None, peak_ceiling: float = LOUDNESS_PEAK_CEILING, max_gain: float = LOUDNESS_MAX_GAIN) -> BarkHipLoudnessParams:
    """A target in LUFS (-40 .. -5) as the C interface takes it: lround(100 lufs), as bark_batch_server converts its "loudness" field; None: off."""
    if lufs is None:
        return BarkHipLoudnessParams(0, 0.0, 0.0)
    return BarkHipLoudnessParams(int(math.floor(100.0 * float(lufs) + 0.5)), float(peak_ceiling), float(max_gain))


def audio_render(rate: int = 24000, fmt="f32", speed: float = 1.0, loudness=None, peak_ceiling: float = LOUDNESS_PEAK_CEILING,
                 max_gain: float = LOUDNESS_MAX_GAIN) -> BarkHipAudioRender:
    lp = loudness if isinstance(loudness, BarkHipLoudnessParams) else loudness_params(loudness, peak_ceiling, max_gain)
    return BarkHipAudioRender(audio_format(rate, fmt), speed_permille(speed), lp)


def _voice_struct(voice):
    """(struct, arrays that must stay alive while it is used) for a voice.VoicePrompt or any object with semantic / coarse [T][2] / fine [T][8]."""
    sem = np.ascontiguousarray(voice.semantic, dtype=np.int32).reshape(-1)
    co = np.ascontiguousarray(voice.coarse, dtype=np.int32).reshape(-1, 2)
    fi = np.ascontiguousarray(voice.fine, dtype=np.int32).reshape(-1, 8)
    return BarkHipVoicePrompt(sem.ctypes.data, len(sem), co.ctypes.data, len(co), fi.ctypes.data, len(fi)), (sem, co, fi)


class BarkHipStats(C.Structure):
    _fields_ = [
        ("t_load_us", C.c_int64), ("t_eval_us", C.c_int64), ("t_semantic_us", C.c_int64), ("t_coarse_us", C.c_int64),
        ("t_fine_us", C.c_int64), ("t_codec_us", C.c_int64), ("n_sample_semantic", C.c_int64), ("n_sample_coarse", C.c_int64),
        ("n_sample_fine", C.c_int64), ("n_semantic", C.c_int32), ("n_frames", C.c_int32), ("n_samples", C.c_int32),
        ("n_near_tie", C.c_int32), ("graph_replays", C.c_int32), ("n_prefix_rows_reused", C.c_int32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def library_path() -> str:
    # BARK_HIP_LIBRARY: another build of the same library (e.g. a host-AddressSanitizer build used while debugging)
    return os.environ.get("BARK_HIP_LIBRARY") or os.path.join(_HERE, "lib", "libbark.so")


def build_library(force: bool = False) -> str:
    """Compile csrc/ for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["rm", "-rf", os.path.join(_HERE, "lib", "obj")])
    subprocess.check_call([os.path.join(_HERE, "build.sh")])
    return library_path()


_LIB = None
VOICE_AUDIO_MAX_SAMPLES = 480000          # BARK_HIP_VOICE_AUDIO_MAX_SAMPLES (include/bark_mi355x.h)

EXPORTS = [
    # bark.h
    "bark_context_default_params", "bark_load_model", "bark_generate_audio", "bark_get_audio_data", "bark_get_audio_data_size",
    "bark_get_load_time", "bark_get_eval_time", "bark_reset_statistics", "bark_model_quantize", "bark_free",
    # ggml.h shim
    "ggml_time_init", "ggml_time_us", "ggml_time_ms", "ggml_init", "ggml_free",
    # bark_mi355x.h
    "bark_hip_hparams", "bark_hip_set_params", "bark_hip_tokenize", "bark_hip_bert_tokenize", "bark_hip_gpt_eval",
    "bark_hip_fine_eval", "bark_hip_semantic", "bark_hip_coarse", "bark_hip_fine", "bark_hip_fine_many", "bark_hip_codec_decode", "bark_hip_codec_tap",
    "bark_hip_clone_context", "bark_hip_generate_audio_batch", "bark_hip_generate_batch", "bark_hip_generate_batch_seeded", "bark_hip_generate_batch_ex", "bark_hip_reserve_batch", "bark_hip_profile_lock_step", "bark_hip_batch_audio", "bark_hip_batch_tokens", "bark_hip_get_semantic_tokens", "bark_hip_get_coarse_tokens", "bark_hip_get_fine_tokens", "bark_hip_get_stats",
    "bark_hip_time_decode_step", "bark_hip_time_gemv", "bark_hip_time_slots", "bark_hip_time_fine_pass", "bark_hip_time_fine_passes", "bark_hip_describe", "bark_hip_set_fine_order", "bark_hip_load_model_on_device", "bark_hip_batcher_create_multi",
    "bark_hip_batcher_create", "bark_hip_batcher_create_ex", "bark_hip_batcher_submit", "bark_hip_batcher_submit_ex", "bark_hip_batcher_wait", "bark_hip_batcher_stats", "bark_hip_batcher_admitted", "bark_hip_batcher_free",
    "bark_hip_set_sampling_filter", "bark_hip_generate_batch_filtered", "bark_hip_batcher_submit_filtered", "bark_hip_sample_rows_filtered", "bark_hip_time_sample_filter",
    "bark_hip_sample_rows_state",
    "bark_hip_set_voice_prompt", "bark_hip_generate_batch_voiced", "bark_hip_batcher_submit_voiced", "bark_hip_pick_rows",
    "bark_hip_has_codec_encoder", "bark_hip_codec_encode", "bark_hip_codec_encode_many", "bark_hip_codec_encode_tap", "bark_hip_rvq_encode", "bark_hip_codec_encode_latents", "bark_hip_codec_encode_device_us",
    "bark_hip_load_semantic_encoder", "bark_hip_has_semantic_encoder", "bark_hip_semantic_encode", "bark_hip_semantic_encode_tap", "bark_hip_semantic_head", "bark_hip_semantic_encode_device_us",
    "bark_hip_resample_taps", "bark_hip_resample_24k_to_16k", "bark_hip_voice_from_audio", "bark_hip_set_voice_from_audio", "bark_hip_time_resample",
    "bark_hip_batch_lock_steps",
    "bark_hip_resample_out_len", "bark_hip_resample_table", "bark_hip_resample", "bark_hip_resample_many", "bark_hip_get_audio_as", "bark_hip_batch_audio_as",
    "bark_hip_batcher_submit_as", "bark_hip_batcher_wait_bytes", "bark_hip_time_resample_pair",
    "bark_hip_split_text", "bark_hip_generate_long", "bark_hip_long_audio_as", "bark_hip_long_chunks", "bark_hip_long_chunk_audio", "bark_hip_long_chunk_tokens",
    "bark_hip_join_many", "bark_hip_time_join", "bark_hip_batcher_submit_long", "bark_hip_batcher_ticket_chunks", "bark_hip_time_join_activity",
    "bark_hip_tempo_out_len", "bark_hip_tempo_window", "bark_hip_tempo", "bark_hip_tempo_many", "bark_hip_tempo_positions", "bark_hip_get_audio_at",
    "bark_hip_batch_audio_at", "bark_hip_long_audio_at", "bark_hip_batcher_submit_at", "bark_hip_batcher_submit_long_at", "bark_hip_time_tempo",
    "bark_hip_loudness_constants", "bark_hip_loudness_target_ms", "bark_hip_loudness_many", "bark_hip_loudness_hops", "bark_hip_level_many", "bark_hip_get_audio_with",
    "bark_hip_batch_audio_with", "bark_hip_long_audio_with", "bark_hip_batcher_submit_with", "bark_hip_batcher_submit_long_with", "bark_hip_time_loudness",
    "bark_hip_codec_decode_many",
    "bark_hip_flac_max_bytes", "bark_hip_flac_encode_many", "bark_hip_flac_frames", "bark_hip_time_flac", "bark_hip_time_flac_launch",
]


def load_library() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing - run bark.cpp_amd/build.sh (there is no fallback path)")
    lib = C.CDLL(path)
    vp, ip, fp = C.c_void_p, C.c_void_p, C.c_void_p
    lib.bark_context_default_params.restype = BarkContextParams
    lib.bark_context_default_params.argtypes = []
    lib.bark_load_model.restype = vp
    lib.bark_load_model.argtypes = [C.c_char_p, BarkContextParams, C.c_uint32]
    lib.bark_generate_audio.restype = C.c_bool
    lib.bark_generate_audio.argtypes = [vp, C.c_char_p, C.c_int]
    lib.bark_get_audio_data.restype = C.POINTER(C.c_float)
    lib.bark_get_audio_data.argtypes = [vp]
    lib.bark_get_audio_data_size.restype = C.c_int
    lib.bark_get_audio_data_size.argtypes = [vp]
    lib.bark_get_load_time.restype = C.c_int64
    lib.bark_get_load_time.argtypes = [vp]
    lib.bark_get_eval_time.restype = C.c_int64
    lib.bark_get_eval_time.argtypes = [vp]
    lib.bark_reset_statistics.argtypes = [vp]
    lib.bark_model_quantize.restype = C.c_bool
    lib.bark_model_quantize.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    lib.bark_free.argtypes = [vp]
    lib.ggml_time_us.restype = C.c_int64
    lib.bark_hip_hparams.argtypes = [vp, C.c_int, ip]
    lib.bark_hip_set_params.argtypes = [vp, BarkContextParams]
    lib.bark_hip_tokenize.argtypes = [vp, C.c_char_p, ip]
    lib.bark_hip_bert_tokenize.argtypes = [vp, C.c_char_p, ip, C.c_int]
    lib.bark_hip_gpt_eval.argtypes = [vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, fp]
    lib.bark_hip_fine_eval.argtypes = [vp, ip, C.c_int, fp]
    lib.bark_hip_semantic.argtypes = [vp, ip, ip, C.c_int, fp]
    lib.bark_hip_coarse.argtypes = [vp, ip, C.c_int, ip, C.c_int]
    lib.bark_hip_fine.argtypes = [vp, ip, C.c_int, ip, C.c_int]
    lib.bark_hip_fine_many.argtypes = [vp, ip, ip, C.c_int, ip, C.c_int]
    lib.bark_hip_codec_decode.argtypes = [vp, ip, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_codec_decode_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_codec_tap.argtypes = [vp, ip, C.c_int, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_has_codec_encoder.argtypes = [vp]
    lib.bark_hip_codec_encode.argtypes = [vp, fp, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_codec_encode_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_codec_encode_tap.argtypes = [vp, fp, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_rvq_encode.argtypes = [vp, fp, C.c_int, C.c_int, ip]
    lib.bark_hip_codec_encode_latents.argtypes = [vp, fp, C.c_int]
    lib.bark_hip_codec_encode_device_us.restype = C.c_double
    lib.bark_hip_codec_encode_device_us.argtypes = [vp]
    lib.bark_hip_load_semantic_encoder.argtypes = [vp, C.c_char_p]
    lib.bark_hip_has_semantic_encoder.argtypes = [vp]
    lib.bark_hip_semantic_encode.argtypes = [vp, fp, C.c_int, ip, C.c_int]
    lib.bark_hip_semantic_encode_tap.argtypes = [vp, fp, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_semantic_head.argtypes = [vp, fp, C.c_int, ip, fp]
    lib.bark_hip_semantic_encode_device_us.restype = C.c_double
    lib.bark_hip_semantic_encode_device_us.argtypes = [vp]
    lib.bark_hip_resample_taps.argtypes = [fp]
    lib.bark_hip_resample_24k_to_16k.argtypes = [vp, fp, C.c_int, fp, C.c_int]
    lib.bark_hip_voice_from_audio.argtypes = [vp, fp, C.c_int, ip, C.c_int, ip, ip, C.c_int, ip, ip]
    lib.bark_hip_set_voice_from_audio.argtypes = [vp, fp, C.c_int]
    lib.bark_hip_time_resample.restype = C.c_double
    lib.bark_hip_time_resample.argtypes = [vp, C.c_int, C.c_int]
    lib.bark_hip_resample_out_len.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.bark_hip_resample_table.argtypes = [C.c_int, C.c_int, fp, C.c_int, ip]
    lib.bark_hip_resample.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_resample_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.c_int, C.POINTER(BarkHipAudioFormat), vp, C.c_int, ip]
    lib.bark_hip_get_audio_as.argtypes = [vp, C.POINTER(BarkHipAudioFormat), vp, C.c_int]
    lib.bark_hip_batch_audio_as.argtypes = [vp, C.c_int, C.POINTER(BarkHipAudioFormat), vp, C.c_int]
    lib.bark_hip_time_resample_pair.restype = C.c_double
    lib.bark_hip_time_resample_pair.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_batcher_submit_as.restype = C.c_int64
    lib.bark_hip_batcher_submit_as.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter), C.POINTER(BarkHipVoicePrompt),
                                               C.POINTER(BarkHipAudioFormat)]
    lib.bark_hip_batcher_wait_bytes.argtypes = [vp, C.c_int64, vp, C.c_int]
    lib.bark_hip_batcher_submit_long.restype = C.c_int64
    lib.bark_hip_batcher_submit_long.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipLongParams), C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter),
                                                 C.POINTER(BarkHipVoicePrompt), C.POINTER(BarkHipAudioFormat)]
    lib.bark_hip_batcher_ticket_chunks.argtypes = [vp, C.c_int64]
    lib.bark_hip_time_join_activity.restype = C.c_double
    lib.bark_hip_time_join_activity.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_split_text.argtypes = [vp, C.c_char_p, C.c_int, ip, C.c_int]
    lib.bark_hip_generate_long.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipLongParams), C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter),
                                           C.POINTER(BarkHipVoicePrompt)]
    lib.bark_hip_long_audio_as.argtypes = [vp, C.POINTER(BarkHipAudioFormat), vp, C.c_int]
    lib.bark_hip_long_chunks.argtypes = [vp, ip, C.c_int]
    lib.bark_hip_long_chunk_audio.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_float))]
    lib.bark_hip_long_chunk_tokens.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_join_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.POINTER(BarkHipJoinParams), C.POINTER(BarkHipAudioFormat), vp, C.c_int, ip]
    lib.bark_hip_tempo_out_len.argtypes = [C.c_int, C.c_int]
    lib.bark_hip_tempo_window.argtypes = [fp]
    lib.bark_hip_tempo.argtypes = [vp, fp, C.c_int, C.c_int, fp, C.c_int]
    lib.bark_hip_tempo_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, ip, C.POINTER(BarkHipAudioFormat), vp, C.c_int, ip]
    lib.bark_hip_tempo_positions.argtypes = [vp, fp, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_get_audio_at.argtypes = [vp, C.POINTER(BarkHipAudioFormat), C.c_int, vp, C.c_int]
    lib.bark_hip_batch_audio_at.argtypes = [vp, C.c_int, C.POINTER(BarkHipAudioFormat), C.c_int, vp, C.c_int]
    lib.bark_hip_long_audio_at.argtypes = [vp, C.POINTER(BarkHipAudioFormat), C.c_int, vp, C.c_int]
    lib.bark_hip_batcher_submit_at.restype = C.c_int64
    lib.bark_hip_batcher_submit_at.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter), C.POINTER(BarkHipVoicePrompt),
                                               C.POINTER(BarkHipAudioFormat), C.c_int]
    lib.bark_hip_batcher_submit_long_at.restype = C.c_int64
    lib.bark_hip_batcher_submit_long_at.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipLongParams), C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter),
                                                    C.POINTER(BarkHipVoicePrompt), C.POINTER(BarkHipAudioFormat), C.c_int]
    lib.bark_hip_time_tempo.restype = C.c_double
    lib.bark_hip_time_tempo.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_loudness_constants.argtypes = [C.POINTER(C.c_double)]
    lib.bark_hip_loudness_target_ms.restype = C.c_double
    lib.bark_hip_loudness_target_ms.argtypes = [C.c_int]
    lib.bark_hip_loudness_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.POINTER(BarkHipLoudnessParams), C.POINTER(BarkHipLoudnessInfo)]
    lib.bark_hip_loudness_hops.argtypes = [vp, fp, C.c_int, C.POINTER(C.c_double), C.c_int]
    lib.bark_hip_level_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.POINTER(BarkHipLoudnessParams), ip, C.POINTER(BarkHipAudioFormat), vp, C.c_int, ip,
                                        C.POINTER(BarkHipLoudnessInfo)]
    lib.bark_hip_get_audio_with.argtypes = [vp, C.POINTER(BarkHipAudioRender), vp, C.c_int, C.POINTER(BarkHipLoudnessInfo)]
    lib.bark_hip_batch_audio_with.argtypes = [vp, C.c_int, C.POINTER(BarkHipAudioRender), vp, C.c_int, C.POINTER(BarkHipLoudnessInfo)]
    lib.bark_hip_long_audio_with.argtypes = [vp, C.POINTER(BarkHipAudioRender), vp, C.c_int, C.POINTER(BarkHipLoudnessInfo), C.c_int]
    lib.bark_hip_batcher_submit_with.restype = C.c_int64
    lib.bark_hip_batcher_submit_with.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter), C.POINTER(BarkHipVoicePrompt),
                                                 C.POINTER(BarkHipAudioRender)]
    lib.bark_hip_batcher_submit_long_with.restype = C.c_int64
    lib.bark_hip_batcher_submit_long_with.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipLongParams), C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter),
                                                      C.POINTER(BarkHipVoicePrompt), C.POINTER(BarkHipAudioRender)]
    lib.bark_hip_time_loudness.restype = C.c_double
    lib.bark_hip_time_loudness.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_flac_max_bytes.argtypes = [C.c_int]
    lib.bark_hip_flac_encode_many.argtypes = [vp, C.POINTER(C.c_void_p), ip, C.c_int, C.c_int, vp, C.c_int, ip]
    lib.bark_hip_flac_frames.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_time_flac.restype = C.c_double
    lib.bark_hip_time_flac.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_time_flac_launch.restype = C.c_double
    lib.bark_hip_time_flac_launch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_time_join.restype = C.c_double
    lib.bark_hip_time_join.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_generate_batch.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int]
    lib.bark_hip_generate_batch_seeded.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint32)]
    lib.bark_hip_generate_batch_ex.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(BarkHipRequestParams)]
    lib.bark_hip_reserve_batch.argtypes = [vp, C.c_int]
    lib.bark_hip_set_fine_order.argtypes = [vp, C.c_int]
    lib.bark_hip_profile_lock_step.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int]
    lib.bark_hip_batch_audio.argtypes = [vp, C.c_int, C.POINTER(C.POINTER(C.c_float))]
    lib.bark_hip_batch_tokens.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int]
    lib.bark_hip_batch_lock_steps.restype = C.c_int
    lib.bark_hip_batch_lock_steps.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.bark_hip_clone_context.restype = vp
    lib.bark_hip_clone_context.argtypes = [vp, C.c_uint32]
    lib.bark_hip_generate_audio_batch.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_char_p), C.c_int]
    lib.bark_hip_get_semantic_tokens.argtypes = [vp, ip, C.c_int]
    lib.bark_hip_get_coarse_tokens.argtypes = [vp, ip, C.c_int]
    lib.bark_hip_get_fine_tokens.argtypes = [vp, ip, C.c_int]
    lib.bark_hip_get_stats.argtypes = [vp, C.POINTER(BarkHipStats)]
    lib.bark_hip_time_decode_step.restype = C.c_double
    lib.bark_hip_time_decode_step.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.bark_hip_time_gemv.restype = C.c_double
    lib.bark_hip_time_gemv.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.bark_hip_time_slots.restype = C.c_double
    lib.bark_hip_time_slots.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_time_fine_pass.restype = C.c_double
    lib.bark_hip_time_fine_pass.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    lib.bark_hip_batcher_create.restype = vp
    lib.bark_hip_batcher_create.argtypes = [vp, C.c_int, C.c_int]
    lib.bark_hip_batcher_create_ex.restype = vp
    lib.bark_hip_batcher_create_ex.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    lib.bark_hip_load_model_on_device.restype = vp
    lib.bark_hip_load_model_on_device.argtypes = [C.c_char_p, BarkContextParams, C.c_uint32, C.c_int]
    lib.bark_hip_batcher_create_multi.restype = vp
    lib.bark_hip_batcher_create_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int]
    lib.bark_hip_batcher_submit.restype = C.c_int64
    lib.bark_hip_batcher_submit.argtypes = [vp, C.c_char_p, C.c_uint32]
    lib.bark_hip_batcher_submit_ex.restype = C.c_int64
    lib.bark_hip_batcher_submit_ex.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams)]
    lib.bark_hip_batcher_submit_filtered.restype = C.c_int64
    lib.bark_hip_batcher_submit_filtered.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter)]
    lib.bark_hip_set_sampling_filter.argtypes = [vp, C.c_int32, C.c_float]
    lib.bark_hip_generate_batch_filtered.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter)]
    lib.bark_hip_sample_rows_filtered.argtypes = [vp, fp, C.c_int, C.c_int, fp, fp, fp, fp, fp, fp]
    lib.bark_hip_sample_rows_state.argtypes = [vp, fp, C.c_int, C.c_int, fp, ip, fp, fp, fp, C.POINTER(BarkHipSampleCall), ip, ip, fp]
    lib.bark_hip_time_sample_filter.restype = C.c_double
    lib.bark_hip_time_sample_filter.argtypes = [vp, C.c_int, C.c_int, C.c_int32, C.c_float, C.c_int, C.c_int]
    lib.bark_hip_set_voice_prompt.argtypes = [vp, C.POINTER(BarkHipVoicePrompt)]
    lib.bark_hip_generate_batch_voiced.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter),
                                                   C.POINTER(C.POINTER(BarkHipVoicePrompt))]
    lib.bark_hip_batcher_submit_voiced.restype = C.c_int64
    lib.bark_hip_batcher_submit_voiced.argtypes = [vp, C.c_char_p, C.POINTER(BarkHipRequestParams), C.POINTER(BarkHipSamplingFilter), C.POINTER(BarkHipVoicePrompt)]
    lib.bark_hip_pick_rows.argtypes = [vp, fp, C.c_int, C.c_int, C.c_float, fp, ip, ip, ip]
    lib.bark_hip_batcher_wait.argtypes = [vp, C.c_int64, fp, C.c_int]
    lib.bark_hip_batcher_stats.restype = None
    lib.bark_hip_batcher_stats.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    lib.bark_hip_batcher_admitted.argtypes = [vp]
    lib.bark_hip_batcher_free.restype = None
    lib.bark_hip_batcher_free.argtypes = [vp]
    lib.bark_hip_time_fine_passes.restype = C.c_double
    lib.bark_hip_time_fine_passes.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    lib.bark_hip_describe.restype = C.c_char_p
    lib.bark_hip_describe.argtypes = [vp]
    _LIB = lib
    return lib


def default_params(**overrides) -> BarkContextParams:
    p = load_library().bark_context_default_params()
    for k, v in overrides.items():
        setattr(p, k, v)
    return p


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class BarkContext:
    """Owner of a `struct bark_context *`."""

    def __init__(self, handle, lib):
        self._h = handle
        self._lib = lib
        self._cb = None
        self._params = None

    # ---- bark.h ---------------------------------------------------------------------------------
    @classmethod
    def load_model(cls, model_path: str, params: BarkContextParams | None = None, seed: int = 0, device: int | None = None) -> "BarkContext":
        """device None: bark_load_model (BARK_HIP_DEVICE / the current device); an ordinal: bark_hip_load_model_on_device (one process, several GPUs)"""
        lib = load_library()
        params = params if params is not None else default_params()
        if device is None:
            h = lib.bark_load_model(os.fsencode(model_path), params, seed)
        else:
            h = lib.bark_hip_load_model_on_device(os.fsencode(model_path), params, seed, int(device))
        if not h:
            raise RuntimeError(f"bark_load_model failed for {model_path}")
        ctx = cls(h, lib)
        ctx._cb = params.progress_callback      # keep the callback object alive
        ctx._params = params
        return ctx

    def generate_audio(self, text: str, n_threads: int = 4) -> bool:
        return bool(self._lib.bark_generate_audio(self._h, text.encode("utf-8"), n_threads))

    def audio_data(self) -> np.ndarray:
        n = self._lib.bark_get_audio_data_size(self._h)
        p = self._lib.bark_get_audio_data(self._h)
        if n <= 0 or not p:
            return np.zeros(0, np.float32)
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    def load_time_us(self) -> int:
        return int(self._lib.bark_get_load_time(self._h))

    def eval_time_us(self) -> int:
        return int(self._lib.bark_get_eval_time(self._h))

    def reset_statistics(self):
        self._lib.bark_reset_statistics(self._h)

    def free(self):
        if self._h:
            self._lib.bark_free(self._h)
            self._h = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    # ---- bark_mi355x.h --------------------------------------------------------------------------
    def describe(self) -> str:
        return self._lib.bark_hip_describe(self._h).decode()

    def hparams(self, which: int) -> dict:
        out = np.zeros(10, np.int32)
        if self._lib.bark_hip_hparams(self._h, which, out.ctypes.data) != 0:
            raise RuntimeError("bark_hip_hparams failed")
        keys = ["n_layer", "n_head", "n_embd", "block_size", "bias", "n_in", "n_out", "n_lm_heads", "n_wtes", "ftype"]
        return dict(zip(keys, (int(v) for v in out)))

    def set_params(self, params: BarkContextParams):
        self._cb = params.progress_callback
        self._params = params
        self._lib.bark_hip_set_params(self._h, params)

    def tokenize(self, text: str) -> np.ndarray:
        out = np.zeros(513, np.int32)
        n = self._lib.bark_hip_tokenize(self._h, text.encode("utf-8"), out.ctypes.data)
        if n != 513:
            raise RuntimeError("bark_hip_tokenize failed")
        return out

    def bert_tokenize(self, text: str, n_max: int = 256) -> np.ndarray:
        out = np.zeros(n_max, np.int32)
        n = self._lib.bark_hip_bert_tokenize(self._h, text.encode("utf-8"), out.ctypes.data, n_max)
        if n < 0:
            raise RuntimeError("bark_hip_bert_tokenize failed")
        return out[:n]

    def gpt_eval(self, which: int, tokens, n_past: int, merge_ctx: bool):
        tokens = _i32(tokens)
        logits = np.zeros(self.hparams(which)["n_out"], np.float32)
        r = self._lib.bark_hip_gpt_eval(self._h, which, tokens.ctypes.data, len(tokens), n_past, int(merge_ctx), logits.ctypes.data)
        if r < 0:
            raise RuntimeError("bark_hip_gpt_eval failed")
        return logits, r

    def fine_eval(self, tokens_8x1024, nn: int) -> np.ndarray:
        tokens = _i32(tokens_8x1024).reshape(8, 1024)
        logits = np.zeros((1024, self.hparams(2)["n_out"]), np.float32)
        if self._lib.bark_hip_fine_eval(self._h, tokens.ctypes.data, nn, logits.ctypes.data) != 0:
            raise RuntimeError("bark_hip_fine_eval failed")
        return logits

    def semantic(self, prompt513, want_eos_trace: bool = False):
        prompt = _i32(prompt513)
        assert prompt.shape == (513,)
        out = np.zeros(1024, np.int32)
        tr = np.zeros(1025, np.float32)
        n = self._lib.bark_hip_semantic(self._h, prompt.ctypes.data, out.ctypes.data, 1024, tr.ctypes.data if want_eos_trace else None)
        if n < 0:
            raise RuntimeError("bark_hip_semantic failed")
        return (out[:n].copy(), tr) if want_eos_trace else out[:n].copy()

    def coarse(self, semantic) -> np.ndarray:
        sem = _i32(semantic)
        p = self._params if self._params is not None else default_params()      # T = floor(n_sem * coarse_rate / semantic_rate) with the context's own rates
        cap = int(len(sem) * max(p.coarse_rate_hz, 1e-3) / max(p.semantic_rate_hz, 1e-3)) + 8
        out = np.zeros((cap, 2), np.int32)
        T = self._lib.bark_hip_coarse(self._h, sem.ctypes.data, len(sem), out.ctypes.data, cap)
        if T < 0:
            raise RuntimeError("bark_hip_coarse failed")
        return out[:T].copy()

    def fine(self, coarse_Tx2) -> np.ndarray:
        co = _i32(coarse_Tx2).reshape(-1, 2)
        out = np.zeros((max(len(co), 1), 8), np.int32)
        T = self._lib.bark_hip_fine(self._h, co.ctypes.data, len(co), out.ctypes.data, len(out))
        if T < 0:
            raise RuntimeError("bark_hip_fine failed")
        return out[:T].copy()

    def fine_many(self, coarse_list) -> list:
        """The fine stage of several utterances, their windows side by side in every forward pass (bark_hip_fine_many)."""
        cos = [_i32(x).reshape(-1, 2) for x in coarse_list]
        T = _i32([len(x) for x in cos])
        cat = np.ascontiguousarray(np.concatenate(cos, axis=0))
        out = np.zeros((len(cat), 8), np.int32)
        n = self._lib.bark_hip_fine_many(self._h, cat.ctypes.data, T.ctypes.data, len(cos), out.ctypes.data, len(out))
        if n < 0:
            raise RuntimeError("bark_hip_fine_many failed")
        res, off = [], 0
        for t in T:
            res.append(out[off:off + int(t)].copy()); off += int(t)
        return res

    def codec_decode(self, codes_qxT) -> np.ndarray:
        codes = _i32(codes_qxT)
        n_q, T = codes.shape
        pcm = np.zeros(T * 320, np.float32)
        n = self._lib.bark_hip_codec_decode(self._h, codes.ctypes.data, n_q, T, pcm.ctypes.data, pcm.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_decode failed")
        return pcm[:n].copy()

    def codec_decode_many(self, codes_list) -> list:
        """n <= 32 utterances in one pass, as a lock-step job decodes them (bark_hip_codec_decode_many): one [n_q][T_i] matrix each, all of one n_q;
        one array of 320 T_i samples per utterance."""
        cs = [_i32(x) for x in codes_list]
        assert cs and all(x.ndim == 2 and x.shape[0] == cs[0].shape[0] for x in cs)
        n_q = cs[0].shape[0]
        T = _i32([x.shape[1] for x in cs])
        ptrs = (C.c_void_p * len(cs))(*[x.ctypes.data for x in cs])
        out = np.zeros(320 * max(int(T.sum()), 1), np.float32)
        n = self._lib.bark_hip_codec_decode_many(self._h, ptrs, T.ctypes.data, len(cs), n_q, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_decode_many failed")
        assert n == 320 * int(T.sum())
        res, off = [], 0
        for t in T:
            res.append(out[off:off + 320 * int(t)].copy()); off += 320 * int(t)
        return res

    def codec_tap(self, codes_qxT, stage: int) -> np.ndarray:
        codes = _i32(codes_qxT)
        n_q, T = codes.shape
        out = np.zeros(T * 320 * 64, np.float32)
        n = self._lib.bark_hip_codec_tap(self._h, codes.ctypes.data, n_q, T, stage, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_tap failed")
        return out[:n].copy()

    def has_codec_encoder(self) -> bool:
        return bool(self._lib.bark_hip_has_codec_encoder(self._h))

    def codec_encode(self, pcm, n_q: int = 8) -> np.ndarray:
        """EnCodec encode (bark_hip_codec_encode): 24 kHz mono float samples -> codes [n_q][T], T = ceil(n / 320)."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        T = (len(x) + 319) // 320
        codes = np.zeros((max(n_q, 1), max(T, 1)), np.int32)
        n = self._lib.bark_hip_codec_encode(self._h, x.ctypes.data, len(x), n_q, codes.ctypes.data, codes.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_encode failed")
        return codes[:, :n].copy()

    def codec_encode_many(self, pcm_list, n_q: int = 8) -> list:
        """n <= 32 recordings in one pass (bark_hip_codec_encode_many): one [n_q][T_i] array per recording."""
        xs = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in pcm_list]
        ns = _i32([len(x) for x in xs])
        Ts = [(len(x) + 319) // 320 for x in xs]
        ptrs = (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
        out = np.zeros(max(n_q, 1) * max(sum(Ts), 1), np.int32)
        n = self._lib.bark_hip_codec_encode_many(self._h, ptrs, ns.ctypes.data, len(xs), n_q, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_encode_many failed")
        res, off = [], 0
        for t in Ts:
            res.append(out[off:off + n_q * t].reshape(n_q, t).copy()); off += n_q * t
        return res

    def codec_encode_tap(self, pcm, stage: int) -> np.ndarray:
        """Parity tap of the encoder (bark_hip_codec_encode_tap), channel-major [C][T']: stage 0 first conv, 1..4 down-sampling convs, 5 LSTM + skip, 6 latent."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        out = np.zeros(max(len(x), 1) * 64 + 4096, np.float32)
        n = self._lib.bark_hip_codec_encode_tap(self._h, x.ctypes.data, len(x), stage, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_codec_encode_tap failed")
        rows = len(x)
        for s in (2, 4, 5, 8)[:min(max(stage, 0), 4)]:
            rows = (rows + s - 1) // s
        return out[:n].copy().reshape(-1, rows)

    def codec_encode_latents(self, n_frames: int, hidden_dim: int = 128) -> np.ndarray:
        """The latents [sum T_i][hidden_dim] the last codec_encode / codec_encode_many call quantised (bark_hip_codec_encode_latents); n_frames = sum T_i."""
        out = np.zeros((n_frames, hidden_dim), np.float32)
        if self._lib.bark_hip_codec_encode_latents(self._h, out.ctypes.data, out.size) != n_frames:
            raise RuntimeError("bark_hip_codec_encode_latents failed")
        return out

    def codec_encode_device_us(self) -> float:
        """hipEvent time between the first and the last kernel of the last codec_encode / codec_encode_many call (bark_hip_codec_encode_device_us)."""
        return float(self._lib.bark_hip_codec_encode_device_us(self._h))

    def rvq_encode(self, latents_TxH, n_q: int = 8) -> np.ndarray:
        """Kernel-level hook (bark_hip_rvq_encode): latents [T][hidden_dim] -> codes [n_q][T] by the RVQ kernel alone (rule C11q)."""
        z = np.ascontiguousarray(latents_TxH, dtype=np.float32)
        assert z.ndim == 2
        codes = np.zeros((max(n_q, 1), len(z)), np.int32)
        if self._lib.bark_hip_rvq_encode(self._h, z.ctypes.data, len(z), n_q, codes.ctypes.data) < 0:
            raise RuntimeError("bark_hip_rvq_encode failed")
        return codes

    # ---- semantic tokens from audio (rule C12h): HuBERT + token head, weights from a file of their own (tools/convert_hubert.py) ----
    def load_semantic_encoder(self, path: str):
        """bark_hip_load_semantic_encoder: this context and the clones made afterwards share the encoder.  Raises on a file the loader refuses."""
        if self._lib.bark_hip_load_semantic_encoder(self._h, os.fsencode(path)) != 0:
            raise RuntimeError(f"bark_hip_load_semantic_encoder failed for {path}")
        with open(path, "rb") as f:
            hp = np.frombuffer(f.read(48), dtype="<i4")[1:]
        self._hub_hp = dict(zip(("C", "H", "n_head", "F", "n_layer_stored", "output_layer", "pos_kernel", "pos_groups", "D", "n_classes", "ftype"), (int(v) for v in hp)))

    def has_semantic_encoder(self) -> bool:
        return bool(self._lib.bark_hip_has_semantic_encoder(self._h))

    def semantic_encode(self, pcm16k) -> np.ndarray:
        """16 kHz mono float samples -> semantic ids [T], T = (n - 400) // 320 + 1 (bark_hip_semantic_encode)."""
        x = np.ascontiguousarray(pcm16k, dtype=np.float32).reshape(-1)
        ids = np.zeros(max((len(x) - 400) // 320 + 1, 1), np.int32)
        n = self._lib.bark_hip_semantic_encode(self._h, x.ctypes.data, len(x), ids.ctypes.data, ids.size)
        if n < 0:
            raise RuntimeError("bark_hip_semantic_encode failed")
        return ids[:n].copy()

    def semantic_encode_tap(self, pcm16k, stage: int) -> np.ndarray:
        """Parity tap (bark_hip_semantic_encode_tap), time-major rows: 0 conv 0 + norm + GELU [T0][C], 1 conv stack [T][C], 2 projection [T][H],
        3 hidden_states[0], 4 hidden_states[output_layer], 5 logits [T][n_classes]."""
        x = np.ascontiguousarray(pcm16k, dtype=np.float32).reshape(-1)
        hp = getattr(self, "_hub_hp", None) or {"C": 512, "H": 768, "n_classes": 10000}
        rows = max((len(x) - 10) // 5 + 1 if stage == 0 else (len(x) - 400) // 320 + 1, 1)
        out = np.zeros(rows * max(hp["C"], hp["H"], hp["n_classes"]), np.float32)
        n = self._lib.bark_hip_semantic_encode_tap(self._h, x.ctypes.data, len(x), stage, out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_semantic_encode_tap failed")
        return out[:n].copy().reshape(rows, -1)

    def semantic_head(self, feats_TxH, want_logits: bool = False):
        """Kernel-level hook (bark_hip_semantic_head): the token head on rows [T][H] -> ids [T] (and logits [T][n_classes])."""
        z = np.ascontiguousarray(feats_TxH, dtype=np.float32)
        assert z.ndim == 2
        ids = np.zeros(max(len(z), 1), np.int32)
        logits = np.zeros((max(len(z), 1), self._hub_hp["n_classes"]), np.float32) if want_logits else None
        if self._lib.bark_hip_semantic_head(self._h, z.ctypes.data, len(z), ids.ctypes.data, logits.ctypes.data if want_logits else None) < 0:
            raise RuntimeError("bark_hip_semantic_head failed")
        return (ids[:len(z)], logits) if want_logits else ids[:len(z)]

    def semantic_encode_device_us(self) -> float:
        return float(self._lib.bark_hip_semantic_encode_device_us(self._h))

    # ---- voice prompts from a recording (rule C13r): the device resampler and the three streams in one native call ----
    def resample_24k_to_16k(self, pcm) -> np.ndarray:
        """24 kHz mono float samples -> (2 n + 2) // 3 samples at 16 kHz (bark_hip_resample_24k_to_16k: f32, one fmaf chain per output)."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        out = np.zeros(max((2 * len(x) + 2) // 3, 1), np.float32)
        n = self._lib.bark_hip_resample_24k_to_16k(self._h, x.ctypes.data, len(x), out.ctypes.data, out.size)
        if n < 0:
            raise RuntimeError("bark_hip_resample_24k_to_16k failed")
        return out[:n].copy()

    def voice_from_audio(self, pcm):
        """A recording of the speaker (24 kHz mono; its last 480 000 samples are used) -> (semantic [n], coarse [T][2], fine [T][8]) by bark_hip_voice_from_audio."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        used = min(len(x), VOICE_AUDIO_MAX_SAMPLES)
        sem = np.zeros(max(((2 * used + 2) // 3 - 400) // 320 + 1, 1), np.int32)
        rows = max((used + 319) // 320, 1)
        coarse, fine = np.zeros((rows, 2), np.int32), np.zeros((rows, 8), np.int32)
        n_sem, n_frames = C.c_int32(0), C.c_int32(0)
        if self._lib.bark_hip_voice_from_audio(self._h, x.ctypes.data, len(x), sem.ctypes.data, sem.size, coarse.ctypes.data, fine.ctypes.data, rows,
                                               C.addressof(n_sem), C.addressof(n_frames)) != 0:
            raise ValueError("bark_hip_voice_from_audio refused the recording (no encoder, too short, non-finite samples, or a voice prompt the engine refuses)")
        return sem[:n_sem.value].copy(), coarse[:n_frames.value].copy(), fine[:n_frames.value].copy()

    def set_voice_from_audio(self, pcm):
        """bark_hip_set_voice_from_audio: the voice prompt of the recording becomes the context's."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        if self._lib.bark_hip_set_voice_from_audio(self._h, x.ctypes.data, len(x)) != 0:
            raise ValueError("bark_hip_set_voice_from_audio refused the recording")

    def time_resample(self, n: int, iters: int) -> float:
        us = self._lib.bark_hip_time_resample(self._h, int(n), int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_resample failed")
        return us

    # ---- output rate and sample format (rule C14r): the rational resampler and the formats f32 / s16 / mu-law ----
    def resample(self, pcm, rate_in: int, rate_out: int) -> np.ndarray:
        """One recording in f32 (bark_hip_resample): n samples at rate_in -> ceil(n rate_out / rate_in) at rate_out; 24000 on at least one side."""
        x = np.ascontiguousarray(pcm, dtype=np.float32).reshape(-1)
        cap = self._lib.bark_hip_resample_out_len(len(x), int(rate_in), int(rate_out))
        if cap < 0:
            raise ValueError(f"bark_hip_resample: unsupported pair {rate_in} -> {rate_out}")
        out = np.zeros(max(cap, 1), np.float32)
        n = self._lib.bark_hip_resample(self._h, x.ctypes.data, len(x), int(rate_in), int(rate_out), out.ctypes.data, out.size)
        if n < 0:
            raise ValueError("bark_hip_resample refused the recording (empty, longer than 1 310 720 samples, or a sample that is not finite)")
        return out[:n].copy()

    def resample_many(self, pcm_list, rate_in: int, rate_out: int, fmt="f32") -> list:
        """Up to 64 segments in one launch (bark_hip_resample_many): one array per segment in the format's dtype (float32 / int16 / uint8)."""
        xs = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in pcm_list]
        to = audio_format(rate_out, fmt)
        ns = _i32([len(x) for x in xs])
        ptrs = (C.c_void_p * len(xs))(*[x.ctypes.data for x in xs])
        dt = np.dtype(SAMPLE_DTYPES[to.sample_format])
        cap = sum(max(self._lib.bark_hip_resample_out_len(len(x), int(rate_in), int(rate_out)), 0) for x in xs) * dt.itemsize
        out = np.zeros(max(cap, 1), np.uint8)
        n_out = np.zeros(max(len(xs), 1), np.int32)
        got = self._lib.bark_hip_resample_many(self._h, ptrs, ns.ctypes.data, len(xs), int(rate_in), C.byref(to), out.ctypes.data, cap, n_out.ctypes.data)
        if got < 0:
            raise ValueError("bark_hip_resample_many refused the call (segment count or length, a sample that is not finite, the pair or the format)")
        res, off = [], 0
        for k in n_out[:len(xs)]:
            res.append(out[off:off + int(k) * dt.itemsize].view(dt).copy()); off += int(k) * dt.itemsize
        return res

    def _audio_as(self, call, to) -> np.ndarray:
        n = call(None, 0)                                   # probe: -(2 + bytes)
        if n > -2:
            raise RuntimeError("no audio held, or an unsupported rate / format")
        buf = np.zeros(-n - 2, np.uint8)
        n = call(buf.ctypes.data, buf.size)
        if n < 0:
            raise RuntimeError("the conversion failed")
        return buf[:n].view(SAMPLE_DTYPES[to.sample_format]).copy()

    def audio_as(self, rate: int = 24000, fmt="f32") -> np.ndarray:
        """The last generate_audio result at `rate` in `fmt` (bark_hip_get_audio_as); audio_data() stays 24 kHz f32."""
        to = audio_format(rate, fmt)
        return self._audio_as(lambda p, cap: self._lib.bark_hip_get_audio_as(self._h, C.byref(to), p, cap), to)

    def batch_audio_as(self, i: int, rate: int = 24000, fmt="f32") -> np.ndarray:
        """Utterance i of the last job at `rate` in `fmt` (bark_hip_batch_audio_as)."""
        to = audio_format(rate, fmt)
        return self._audio_as(lambda p, cap: self._lib.bark_hip_batch_audio_as(self._h, int(i), C.byref(to), p, cap), to)

    def time_resample_pair(self, n: int, rate_in: int, rate_out: int, fmt="f32", iters: int = 20) -> float:
        us = self._lib.bark_hip_time_resample_pair(self._h, int(n), int(rate_in), int(rate_out), audio_format(rate_out, fmt).sample_format, int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_resample_pair failed")
        return us

    # ---- long-form text (rules C15s, C15j): the splitter, the chunks as one lock-step job, the join on the device ----
    def split_text(self, text, max_tokens: int = 0) -> list:
        """The chunks of a text as byte spans [(begin, end)] into its UTF-8 bytes (bark_hip_split_text); max_tokens 0: one sentence per chunk."""
        raw = text if isinstance(text, bytes) else text.encode("utf-8")
        spans = np.zeros(2 * SPLIT_MAX_CHUNKS, np.int32)
        n = self._lib.bark_hip_split_text(self._h, raw, int(max_tokens), spans.ctypes.data, SPLIT_MAX_CHUNKS)
        if n < 0:
            raise ValueError("bark_hip_split_text refused the text (max_tokens outside 0 .. 255, or more than 64 chunks)")
        return [(int(spans[2 * i]), int(spans[2 * i + 1])) for i in range(n)]

    def generate_long(self, text, max_tokens: int = 0, chain: bool = False, join: "BarkHipJoinParams | None" = None, params: "BarkHipRequestParams | None" = None,
                      top_k: "int | None" = None, top_p: "float | None" = None, voice=None) -> list:
        """A text of any length (bark_hip_generate_long): split, one lock-step job over the chunks (chain: a job per chunk, each continuing the one before
        it), results held by the context for long_audio_as / long_chunks.  Returns one dict per chunk: pcm (untrimmed, 24 kHz) and the three token streams."""
        raw = text if isinstance(text, bytes) else text.encode("utf-8")
        lp = BarkHipLongParams(int(max_tokens), int(bool(chain)), join if join is not None else join_params())
        flt = None if top_k is None and top_p is None else BarkHipSamplingFilter(int(top_k or 0), float(1.0 if top_p is None else top_p))
        keep = None if voice is None else _voice_struct(voice)
        n = self._lib.bark_hip_generate_long(self._h, raw, C.byref(lp), None if params is None else C.byref(params), None if flt is None else C.byref(flt),
                                             None if keep is None else C.byref(keep[0]))
        if n < 0:
            raise RuntimeError("bark_hip_generate_long failed")
        out = []
        for i in range(n):
            p = C.POINTER(C.c_float)()
            ns = self._lib.bark_hip_long_chunk_audio(self._h, i, C.byref(p))
            d = {"pcm": np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns > 0 else np.zeros(0, np.float32)}
            for stage, (name, w) in enumerate((("semantic", 1), ("coarse", 2), ("fine", 8))):
                buf = np.zeros(65536, np.int32)
                k = self._lib.bark_hip_long_chunk_tokens(self._h, i, stage, buf.ctypes.data, buf.size)
                d[name] = buf[:max(k, 0)].copy().reshape(-1, w) if w > 1 else buf[:max(k, 0)].copy()
            out.append(d)
        return out

    def long_audio_as(self, rate: int = 24000, fmt="f32") -> np.ndarray:
        """The joined audio of the last generate_long at `rate` in `fmt` (bark_hip_long_audio_as)."""
        to = audio_format(rate, fmt)
        n = self._lib.bark_hip_long_audio_as(self._h, C.byref(to), None, 0)
        if n == -1:
            raise RuntimeError("no long result held, or an unsupported rate / format")
        buf = np.zeros(max(-n - 2, 1), np.uint8)
        if n < -1:
            n = self._lib.bark_hip_long_audio_as(self._h, C.byref(to), buf.ctypes.data, buf.size)
            if n < 0:
                raise RuntimeError("bark_hip_long_audio_as failed")
        return buf[:n].view(SAMPLE_DTYPES[to.sample_format]).copy()

    def long_chunks(self) -> list:
        """[(text begin, text end, first sample in the joined 24 kHz signal, kept samples)] per chunk of the last generate_long (bark_hip_long_chunks)."""
        out = np.zeros(4 * SPLIT_MAX_CHUNKS, np.int32)
        n = self._lib.bark_hip_long_chunks(self._h, out.ctypes.data, SPLIT_MAX_CHUNKS)
        if n < 0:
            raise RuntimeError("no long result held")
        return [tuple(int(v) for v in out[4 * i:4 * i + 4]) for i in range(n)]

    def join_many(self, pcm_list, join: "BarkHipJoinParams | None" = None, rate: int = 24000, fmt="f32", want_layout: bool = False):
        """The join alone on caller audio (bark_hip_join_many): up to 64 segments at 24 kHz -> one array at `rate` in `fmt`; want_layout: also
        [(first sample in the joined signal, kept samples)] per segment."""
        xs = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in pcm_list]
        to = audio_format(rate, fmt)
        jp = join if join is not None else join_params()
        ns = _i32([len(x) for x in xs])
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])
        layout = np.zeros(2 * max(len(xs), 1), np.int32)
        call = lambda p, cap: self._lib.bark_hip_join_many(self._h, ptrs, ns.ctypes.data, len(xs), C.byref(jp), C.byref(to), p, cap, layout.ctypes.data)
        n_max = min(sum(len(x) for x in xs) + max(len(xs) - 1, 0) * max(int(jp.gap_samples), 0), 1 << 25)      # nothing trimmed: one call serves
        buf = np.zeros(max(-(-n_max * max(int(rate), 0) // 24000) * np.dtype(SAMPLE_DTYPES[to.sample_format]).itemsize, 1), np.uint8)
        n = call(buf.ctypes.data, buf.size)
        if n < 0:
            raise ValueError("bark_hip_join_many refused the call (segment count or length, a sample that is not finite, the parameters, the rate or the format)")
        res = buf[:n].view(SAMPLE_DTYPES[to.sample_format]).copy()
        return (res, [(int(layout[2 * i]), int(layout[2 * i + 1])) for i in range(len(xs))]) if want_layout else res

    def time_join(self, count: int, n_each: int, rate: int = 24000, fmt="f32", iters: int = 20) -> float:
        us = self._lib.bark_hip_time_join(self._h, int(count), int(n_each), int(rate), audio_format(rate, fmt).sample_format, int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_join failed")
        return us

    def time_join_activity(self, count: int, n_each: int, iters: int = 20) -> float:
        """What a trim threshold adds in front of the join launch, timed apart (bark_hip_time_join_activity): the table's fill and the activity launch."""
        us = self._lib.bark_hip_time_join_activity(self._h, int(count), int(n_each), int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_join_activity failed")
        return us

    # ---- speaking rate (rule C16t): time-scale modification on the device; speed is a factor (1.25: a quarter faster), sent as lround(1000 speed) ----
    def tempo(self, pcm, speed: float) -> np.ndarray:
        """One 24 kHz recording at another speaking rate, same pitch (bark_hip_tempo): n samples -> ceil(1000 n / p), p = speed_permille(speed)."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        p = speed_permille(speed)
        cap = self._lib.bark_hip_tempo_out_len(len(x), p)
        if cap < 0:
            raise ValueError("bark_hip_tempo: 1 .. 1 310 720 samples and a speed of 0.5 .. 2.0")
        out = np.zeros(cap, np.float32)
        n = self._lib.bark_hip_tempo(self._h, x.ctypes.data, len(x), p, out.ctypes.data, out.size)
        if n < 0:
            raise ValueError("bark_hip_tempo refused the recording (a sample that is not finite or not below 65520 in magnitude)")
        return out[:n]

    def tempo_many(self, pcm_list, speeds, rate: int = 24000, fmt="f32") -> list:
        """Up to 64 recordings, a speed each, in one tempo launch, then `rate` / `fmt` (bark_hip_tempo_many): one array per recording in the format's dtype."""
        xs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in pcm_list]
        sp = np.asarray([speed_permille(v) for v in speeds], np.int32)
        if len(sp) != len(xs):
            raise ValueError("one speed per recording")
        to = audio_format(rate, fmt)
        dt = np.dtype(SAMPLE_DTYPES[to.sample_format])
        lens = [self._lib.bark_hip_resample_out_len(max(self._lib.bark_hip_tempo_out_len(len(x), int(p)), 0), 24000, int(rate)) for x, p in zip(xs, sp)]
        cap = sum(max(v, 0) for v in lens) * dt.itemsize
        out = np.zeros(max(cap, 1), np.uint8)
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])
        ns = np.asarray([len(x) for x in xs], np.int32)
        n_out = np.zeros(max(len(xs), 1), np.int32)
        got = self._lib.bark_hip_tempo_many(self._h, ptrs, ns.ctypes.data, len(xs), sp.ctypes.data, C.byref(to), out.ctypes.data, cap, n_out.ctypes.data)
        if got < 0:
            raise ValueError("bark_hip_tempo_many refused the call (segment count or length, a speed, a sample out of range, the rate or the format)")
        res, off = [], 0
        for k in n_out[:len(xs)]:
            res.append(out[off:off + int(k) * dt.itemsize].view(dt).copy()); off += int(k) * dt.itemsize
        return res

    def tempo_positions(self, pcm, speed: float) -> np.ndarray:
        """The positions the search chose, one per frame of 360 outputs (bark_hip_tempo_positions)."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        p = speed_permille(speed)
        cap = self._lib.bark_hip_tempo_out_len(len(x), p)
        if cap < 0:
            raise ValueError("bark_hip_tempo_positions: 1 .. 1 310 720 samples and a speed of 0.5 .. 2.0")
        pos = np.zeros((cap + 359) // 360, np.int32)
        k = self._lib.bark_hip_tempo_positions(self._h, x.ctypes.data, len(x), p, pos.ctypes.data, pos.size)
        if k < 0:
            raise ValueError("bark_hip_tempo_positions refused the recording")
        return pos[:k]

    def audio_at(self, speed: float, rate: int = 24000, fmt="f32") -> np.ndarray:
        """The last generate_audio result at `speed`, then at `rate` in `fmt` (bark_hip_get_audio_at)."""
        to, p = audio_format(rate, fmt), speed_permille(speed)
        return self._audio_as(lambda o, cap: self._lib.bark_hip_get_audio_at(self._h, C.byref(to), p, o, cap), to)

    def batch_audio_at(self, i: int, speed: float, rate: int = 24000, fmt="f32") -> np.ndarray:
        """Utterance i of the last job at `speed`, then at `rate` in `fmt` (bark_hip_batch_audio_at)."""
        to, p = audio_format(rate, fmt), speed_permille(speed)
        return self._audio_as(lambda o, cap: self._lib.bark_hip_batch_audio_at(self._h, int(i), C.byref(to), p, o, cap), to)

    def long_audio_at(self, speed: float, rate: int = 24000, fmt="f32") -> np.ndarray:
        """The join of the last generate_long's chunks, each at `speed`, at `rate` in `fmt` (bark_hip_long_audio_at)."""
        to, p = audio_format(rate, fmt), speed_permille(speed)
        n = self._lib.bark_hip_long_audio_at(self._h, C.byref(to), p, None, 0)
        if n == -1:
            raise RuntimeError("no long result held, or an unsupported speed / rate / format")
        buf = np.zeros(max(-n - 2, 1), np.uint8)
        if n < -1:
            n = self._lib.bark_hip_long_audio_at(self._h, C.byref(to), p, buf.ctypes.data, buf.size)
            if n < 0:
                raise RuntimeError("bark_hip_long_audio_at failed")
        return buf[:n].view(SAMPLE_DTYPES[to.sample_format]).copy()

    def time_tempo(self, count: int, n_each: int, speed: float, iters: int = 20) -> float:
        us = self._lib.bark_hip_time_tempo(self._h, int(count), int(n_each), speed_permille(speed), int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_tempo failed")
        return us

    # ---- loudness (rule C17l): gated BS.1770 measure and the gain to a target on the device; a target is in LUFS (-16.0), sent as lround(100 lufs) ----
    def loudness_many(self, pcm_list, lufs=None, peak_ceiling: float = LOUDNESS_PEAK_CEILING, max_gain: float = LOUDNESS_MAX_GAIN) -> list:
        """Measures up to 64 recordings in two launches (bark_hip_loudness_many): one dict per recording - mean_square, lufs, peak, gain (what levelling to
        `lufs` would apply; 1 without a target), n_blocks, n_abs, n_gated, flags."""
        xs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in pcm_list]
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])
        ns = np.asarray([len(x) for x in xs], np.int32)
        par = (BarkHipLoudnessParams * max(len(xs), 1))(*[loudness_params(lufs, peak_ceiling, max_gain) for _ in xs])
        info = (BarkHipLoudnessInfo * max(len(xs), 1))()
        if self._lib.bark_hip_loudness_many(self._h, ptrs, ns.ctypes.data, len(xs), None if lufs is None else par, info) != len(xs) or not xs:
            raise ValueError("bark_hip_loudness_many refused the call (segment count or length, a sample out of range, the target, the ceiling or the cap)")
        return [info[i].as_dict() for i in range(len(xs))]

    def loudness(self, pcm, lufs=None, peak_ceiling: float = LOUDNESS_PEAK_CEILING, max_gain: float = LOUDNESS_MAX_GAIN) -> dict:
        """One recording measured (see loudness_many)."""
        return self.loudness_many([pcm], lufs, peak_ceiling, max_gain)[0]

    def loudness_hops(self, pcm) -> np.ndarray:
        """The z table of one recording: the K-weighted sum of squares of every 100 ms hop, f64 (bark_hip_loudness_hops)."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        z = np.zeros(max(len(x) // 2400, 1), np.float64)
        k = self._lib.bark_hip_loudness_hops(self._h, x.ctypes.data, len(x), z.ctypes.data_as(C.POINTER(C.c_double)), z.size)
        if k < 0:
            raise ValueError("bark_hip_loudness_hops refused the recording")
        return z[:k]

    def level_many(self, pcm_list, lufs, speeds=None, rate: int = 24000, fmt="f32", peak_ceiling: float = LOUDNESS_PEAK_CEILING, max_gain: float = LOUDNESS_MAX_GAIN,
                   want_info: bool = False):
        """Up to 64 recordings levelled to `lufs` (one target, or one per recording; None: that one is not levelled), then at `speeds` (None: 1.0), `rate`
        and `fmt` in one call (bark_hip_level_many): one array per recording in the format's dtype; want_info: (arrays, dicts as loudness_many gives)."""
        xs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in pcm_list]
        targets = list(lufs) if isinstance(lufs, (list, tuple, np.ndarray)) else [lufs] * len(xs)
        sp = np.asarray([speed_permille(v) for v in (speeds if speeds is not None else [1.0] * len(xs))], np.int32)
        if len(sp) != len(xs) or len(targets) != len(xs):
            raise ValueError("one target and one speed per recording")
        to = audio_format(rate, fmt)
        dt = np.dtype(SAMPLE_DTYPES[to.sample_format])
        lens = [self._lib.bark_hip_resample_out_len(max(self._lib.bark_hip_tempo_out_len(len(x), int(p)), 0), 24000, int(rate)) for x, p in zip(xs, sp)]
        cap = sum(max(v, 0) for v in lens) * dt.itemsize
        out = np.zeros(max(cap, 1), np.uint8)
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])
        ns = np.asarray([len(x) for x in xs], np.int32)
        n_out = np.zeros(max(len(xs), 1), np.int32)
        par = (BarkHipLoudnessParams * max(len(xs), 1))(*[loudness_params(t, peak_ceiling, max_gain) for t in targets])
        info = (BarkHipLoudnessInfo * max(len(xs), 1))()
        got = self._lib.bark_hip_level_many(self._h, ptrs, ns.ctypes.data, len(xs), par, sp.ctypes.data, C.byref(to), out.ctypes.data, cap, n_out.ctypes.data, info)
        if got < 0:
            raise ValueError("bark_hip_level_many refused the call (segment count or length, a target, ceiling, cap or speed, a sample out of range, the rate or the format)")
        res, off = [], 0
        for k in n_out[:len(xs)]:
            res.append(out[off:off + int(k) * dt.itemsize].view(dt).copy()); off += int(k) * dt.itemsize
        return (res, [info[i].as_dict() for i in range(len(xs))]) if want_info else res

    def audio_with(self, rate: int = 24000, fmt="f32", speed: float = 1.0, loudness=None, want_info: bool = False, **limits):
        """The last generate_audio result levelled to `loudness` LUFS (None: not), at `speed`, `rate` and `fmt` (bark_hip_get_audio_with)."""
        how, info = audio_render(rate, fmt, speed, loudness, **limits), BarkHipLoudnessInfo()
        out = self._audio_as(lambda o, cap: self._lib.bark_hip_get_audio_with(self._h, C.byref(how), o, cap, C.byref(info)), how.fmt)
        return (out, info.as_dict()) if want_info else out

    def batch_audio_with(self, i: int, rate: int = 24000, fmt="f32", speed: float = 1.0, loudness=None, want_info: bool = False, **limits):
        """Utterance i of the last job levelled to `loudness` LUFS (None: not), at `speed`, `rate` and `fmt` (bark_hip_batch_audio_with)."""
        how, info = audio_render(rate, fmt, speed, loudness, **limits), BarkHipLoudnessInfo()
        out = self._audio_as(lambda o, cap: self._lib.bark_hip_batch_audio_with(self._h, int(i), C.byref(how), o, cap, C.byref(info)), how.fmt)
        return (out, info.as_dict()) if want_info else out

    def long_audio_with(self, rate: int = 24000, fmt="f32", speed: float = 1.0, loudness=None, want_info: bool = False, **limits):
        """The join of the last generate_long's chunks, each levelled to `loudness` LUFS on its own and at `speed`, at `rate` in `fmt` (bark_hip_long_audio_with);
        want_info: (audio, one dict per chunk)."""
        how = audio_render(rate, fmt, speed, loudness, **limits)
        info = (BarkHipLoudnessInfo * SPLIT_MAX_CHUNKS)()
        n_chunks = len(self.long_chunks()) if want_info else 0
        n = self._lib.bark_hip_long_audio_with(self._h, C.byref(how), None, 0, info, SPLIT_MAX_CHUNKS)
        if n == -1:
            raise RuntimeError("no long result held, or an unsupported loudness / speed / rate / format")
        buf = np.zeros(max(-n - 2, 1), np.uint8)
        if n < -1:
            n = self._lib.bark_hip_long_audio_with(self._h, C.byref(how), buf.ctypes.data, buf.size, info, SPLIT_MAX_CHUNKS)
            if n < 0:
                raise RuntimeError("bark_hip_long_audio_with failed")
        out = buf[:n].view(SAMPLE_DTYPES[how.fmt.sample_format]).copy()
        return (out, [info[i].as_dict() for i in range(n_chunks)]) if want_info else out

    def time_loudness(self, count: int, n_each: int, level: bool = False, iters: int = 20) -> float:
        us = self._lib.bark_hip_time_loudness(self._h, int(count), int(n_each), int(bool(level)), int(iters))
        if us < 0:
            raise RuntimeError("bark_hip_time_loudness failed")
        return us

    # ---- FLAC (rule C18f): the lossless encoder of the output path; the routes take it as fmt="flac", these calls take caller audio ----
    def flac_encode_many(self, pcm_list, rate: int = 24000) -> list:
        """Up to 64 recordings of int16 samples at `rate` -> one complete FLAC stream (bytes) each, in two launches (bark_hip_flac_encode_many)."""
        xs = [np.ascontiguousarray(x, np.int16).reshape(-1) for x in pcm_list]
        ptrs = (C.c_void_p * max(len(xs), 1))(*[x.ctypes.data for x in xs])
        ns = np.asarray([len(x) for x in xs], np.int32)
        cap = sum(max(self._lib.bark_hip_flac_max_bytes(len(x)), 0) for x in xs)
        out = np.zeros(max(cap, 1), np.uint8)
        lengths = np.zeros(max(len(xs), 1), np.int32)
        got = self._lib.bark_hip_flac_encode_many(self._h, ptrs, ns.ctypes.data, len(xs), int(rate), out.ctypes.data, cap, lengths.ctypes.data)
        if got < 0:
            raise ValueError("bark_hip_flac_encode_many refused the call (recording count or length, the rate)")
        res, off = [], 0
        for k in lengths[:len(xs)]:
            res.append(out[off:off + int(k)].tobytes()); off += int(k)
        return res

    def flac_encode(self, pcm, rate: int = 24000) -> bytes:
        """One recording of int16 samples as a FLAC stream (see flac_encode_many)."""
        return self.flac_encode_many([pcm], rate)[0]

    def flac_frames(self, pcm, rate: int = 24000) -> np.ndarray:
        """[frames][4]: subframe code (0 CONSTANT, 1 VERBATIM, 8 + o FIXED of order o), partition order, byte length and CRC-16 of every frame the device
        makes of one recording (bark_hip_flac_frames)."""
        x = np.ascontiguousarray(pcm, np.int16).reshape(-1)
        out = np.zeros((max((len(x) + FLAC_BLOCK - 1) // FLAC_BLOCK, 1), 4), np.int32)
        k = self._lib.bark_hip_flac_frames(self._h, x.ctypes.data, len(x), int(rate), out.ctypes.data, len(out))
        if k < 0:
            raise ValueError("bark_hip_flac_frames refused the recording")
        return out[:k]

    def time_flac(self, count: int, n_each: int, iters: int = 20, which: int = 0) -> float:
        """Device time (us) of the encoder's two launches (which 0), the frames launch (1) or the pack launch (2)."""
        us = (self._lib.bark_hip_time_flac(self._h, int(count), int(n_each), int(iters)) if which == 0
              else self._lib.bark_hip_time_flac_launch(self._h, int(count), int(n_each), int(which), int(iters)))
        if us < 0:
            raise RuntimeError("bark_hip_time_flac failed")
        return us

    def request_params(self, **over) -> BarkHipRequestParams:
        """The context's own values of the per-utterance parameters, with overrides (temp, fine_temp, min_eos_p, n_steps_text_encoder, seed)."""
        p = self._params if self._params is not None else default_params()
        r = BarkHipRequestParams(p.temp, p.fine_temp, p.min_eos_p, p.n_steps_text_encoder, 0)
        known = {name for name, _ in BarkHipRequestParams._fields_}
        for k, v in over.items():
            if k not in known:             # setattr on a ctypes.Structure accepts any name silently: a typo would run with the context's value
                raise TypeError(f"request_params: unknown parameter {k!r} (one of {sorted(known)})")
            setattr(r, k, v)
        return r

    def reserve_batch(self, slots: int):
        if self._lib.bark_hip_reserve_batch(self._h, slots) != 0:
            raise RuntimeError("bark_hip_reserve_batch failed")

    def generate_batch(self, texts, seeds=None, params=None, filters=None, voices=None) -> list:
        """In-engine batching (bark_hip_generate_batch[_seeded|_ex|_filtered|_voiced]): returns one dict per utterance (or None if it failed).
        params: one BarkHipRequestParams per utterance (request_params(...)); filters: one (top_k, top_p) pair or BarkHipSamplingFilter per
        utterance (bark_hip_generate_batch_filtered; None: the context's filter); voices: one voice.VoicePrompt or None (the context's voice)
        per utterance (bark_hip_generate_batch_voiced)."""
        n = len(texts)
        ts = (C.c_char_p * n)(*[t.encode("utf-8") for t in texts])
        if voices is not None:
            assert len(voices) == n and seeds is None
            keep = [None if v is None else _voice_struct(v) for v in voices]
            vs = (C.POINTER(BarkHipVoicePrompt) * n)(*[C.POINTER(BarkHipVoicePrompt)() if k is None else C.pointer(k[0]) for k in keep])
            fl = None
            if filters is not None:
                fl = (BarkHipSamplingFilter * n)(*[f if isinstance(f, BarkHipSamplingFilter) else BarkHipSamplingFilter(int(f[0]), float(f[1])) for f in filters])
            ps = (BarkHipRequestParams * n)(*params) if params is not None else None
            good = self._lib.bark_hip_generate_batch_voiced(self._h, ts, n, ps, fl, vs)
        elif filters is not None:
            assert len(filters) == n and seeds is None
            fl = (BarkHipSamplingFilter * n)(*[f if isinstance(f, BarkHipSamplingFilter) else BarkHipSamplingFilter(int(f[0]), float(f[1])) for f in filters])
            ps = (BarkHipRequestParams * n)(*params) if params is not None else None
            good = self._lib.bark_hip_generate_batch_filtered(self._h, ts, n, ps, fl)
        elif params is not None:
            assert len(params) == n and seeds is None
            good = self._lib.bark_hip_generate_batch_ex(self._h, ts, n, (BarkHipRequestParams * n)(*params))
        elif seeds is None:
            good = self._lib.bark_hip_generate_batch(self._h, ts, n)
        else:
            assert len(seeds) == n
            good = self._lib.bark_hip_generate_batch_seeded(self._h, ts, n, (C.c_uint32 * n)(*[int(v) for v in seeds]))
        if good < 0:
            raise RuntimeError("bark_hip_generate_batch failed")
        out = []
        for i in range(n):
            p = C.POINTER(C.c_float)()
            ns = self._lib.bark_hip_batch_audio(self._h, i, C.byref(p))
            if ns < 0:
                out.append(None)
                continue
            d = {"pcm": np.ctypeslib.as_array(p, shape=(ns,)).copy() if ns else np.zeros(0, np.float32)}
            for stage, (name, w) in enumerate((("semantic", 1), ("coarse", 2), ("fine", 8))):
                buf = np.zeros(65536, np.int32)
                k = self._lib.bark_hip_batch_tokens(self._h, i, stage, buf.ctypes.data, buf.size)
                d[name] = buf[:max(k, 0)].copy().reshape(-1, w) if w > 1 else buf[:max(k, 0)].copy()
            out.append(d)
        return out

    def batch_lock_steps(self):
        """(semantic, coarse) lock steps of the context's last job (bark_hip_batch_lock_steps); (0, 0): the sequential fallback served it; None: no job yet."""
        out = (C.c_int32 * 2)()
        if self._lib.bark_hip_batch_lock_steps(self._h, out) != 0:
            return None
        return int(out[0]), int(out[1])

    def clone(self, seed: int = 0) -> "BarkContext":
        h = self._lib.bark_hip_clone_context(self._h, seed)
        if not h:
            raise RuntimeError("bark_hip_clone_context failed")
        ctx = BarkContext(h, self._lib)
        ctx._cb = self._cb                              # the clone copies the parameters (and the callback pointer) of its source
        ctx._params = self._params
        return ctx

    @staticmethod
    def generate_audio_batch(ctxs, texts) -> int:
        lib = load_library()
        n = len(ctxs)
        assert n == len(texts) and n > 0
        hs = (C.c_void_p * n)(*[c._h for c in ctxs])
        ts = (C.c_char_p * n)(*[t.encode("utf-8") for t in texts])
        return int(lib.bark_hip_generate_audio_batch(hs, ts, n))

    def semantic_tokens(self) -> np.ndarray:
        out = np.zeros(1024, np.int32)
        n = self._lib.bark_hip_get_semantic_tokens(self._h, out.ctypes.data, 1024)
        return out[:max(n, 0)].copy()

    def coarse_tokens(self) -> np.ndarray:
        out = np.zeros((8192, 2), np.int32)            # engine_fine accepts up to 8192 frames
        n = self._lib.bark_hip_get_coarse_tokens(self._h, out.ctypes.data, 8192)
        return out[:max(n, 0)].copy()

    def fine_tokens(self) -> np.ndarray:
        out = np.zeros((8192, 8), np.int32)
        n = self._lib.bark_hip_get_fine_tokens(self._h, out.ctypes.data, 8192)
        return out[:max(n, 0)].copy()

    def stats(self) -> dict:
        s = BarkHipStats()
        self._lib.bark_hip_get_stats(self._h, C.byref(s))
        return s.as_dict()

    def set_sampling_filter(self, top_k: int = 0, top_p: float = 1.0):
        """Top-k / nucleus filter of the semantic and coarse samples (rule C8n; top_k 0 and top_p 1.0: off).  Greedy stages are not filtered."""
        if self._lib.bark_hip_set_sampling_filter(self._h, int(top_k), float(top_p)) != 0:
            raise ValueError(f"bark_hip_set_sampling_filter rejected top_k={top_k}, top_p={top_p} (top_k >= 0, 0 < top_p <= 1)")

    def set_voice_prompt(self, voice=None):
        """The context's voice prompt (rule C10v): a voice.VoicePrompt (semantic [n], coarse [T][2], fine [T][8]); None clears it."""
        if voice is None:
            rc = self._lib.bark_hip_set_voice_prompt(self._h, None)
        else:
            st, keep = _voice_struct(voice)
            rc = self._lib.bark_hip_set_voice_prompt(self._h, C.byref(st))
        if rc != 0:
            raise ValueError("bark_hip_set_voice_prompt rejected the voice prompt (ids out of range, empty trimmed history, or a history too long for the coarse context)")

    def pick_rows(self, logits, rel, tokens, temp: float = 0.0, u=None):
        """Kernel-level hook (bark_hip_pick_rows): the fine stage's pick kernels on logits [n_windows * 1024, n_cols]; row z * 1024 + j of the token
        plane `tokens` receives its pick when j >= rel[z].  Returns (plane int32 [n_windows * 1024], picks settled by the exact path)."""
        lg = np.ascontiguousarray(logits, np.float32)
        rl = _i32(rel).reshape(-1)
        assert lg.shape[0] == 1024 * len(rl)
        tok = _i32(tokens).reshape(-1).copy()
        assert tok.size == lg.shape[0]
        uu = None if u is None else np.ascontiguousarray(u, np.float64).reshape(-1)
        nt = C.c_int32(0)
        if self._lib.bark_hip_pick_rows(self._h, lg.ctypes.data, len(rl), lg.shape[1], float(temp), None if uu is None else uu.ctypes.data, rl.ctypes.data,
                                        tok.ctypes.data, C.addressof(nt)) != 0:
            raise RuntimeError("bark_hip_pick_rows failed")
        return tok, int(nt.value)

    def sample_rows_filtered(self, logits, temp, top_k, top_p, u):
        """Kernel-level hook (bark_hip_sample_rows_filtered): rows of logits [n_rows, n] through the decode loop's filter + sampler launches;
        per-row temp / top_k / top_p / uniform draw u.  Returns (ids int32 [n_rows], eos_p float32 [n_rows])."""
        lg = np.ascontiguousarray(logits, np.float32)
        nr, n = lg.shape
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temp, np.float32), (nr,)))
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, np.int32), (nr,)))
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(top_p, np.float32), (nr,)))
        uu = np.ascontiguousarray(np.broadcast_to(np.asarray(u, np.float64), (nr,)))
        ids = np.zeros(nr, np.int32)
        eos = np.zeros(nr, np.float32)
        if self._lib.bark_hip_sample_rows_filtered(self._h, lg.ctypes.data, nr, n, t.ctypes.data, k.ctypes.data, p.ctypes.data, uu.ctypes.data,
                                                   ids.ctypes.data, eos.ctypes.data) != 0:
            raise RuntimeError("bark_hip_sample_rows_filtered failed")
        return ids, eos

    STATE_FIELDS = ("n_past", "cur_token", "step", "eos_step", "near_tie", "n_out", "last_eos_p", "fault")      # struct StepState, eight 32-bit words

    def sample_rows_state(self, logits, temp, top_k, top_p, u, min_eos_p, state, mode=0, eos_token=-1, token_base=0, prescaled=0, n_past_add=1,
                          per_row=False):
        """Kernel-level hook (bark_hip_sample_rows_state): rows of logits [n_rows, n] through the decode loop's filter + sampler launches with
        per-row temp (0: greedy) / top_k / top_p / u / min_eos_p and the rows' stage states `state` int32 [n_rows, 8] (STATE_FIELDS; last_eos_p
        as float bits) before the launch; per_row: one single-slot launch per row, as bark_generate_audio makes them.
        Returns (ids int32 [n_rows], eos_p float32 [n_rows], state after the launch int32 [n_rows, 8])."""
        lg = np.ascontiguousarray(logits, np.float32)
        nr, n = lg.shape
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(temp, np.float32), (nr,)))
        k = np.ascontiguousarray(np.broadcast_to(np.asarray(top_k, np.int32), (nr,)))
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(top_p, np.float32), (nr,)))
        uu = np.ascontiguousarray(np.broadcast_to(np.asarray(u, np.float64), (nr,)))
        me = np.ascontiguousarray(np.broadcast_to(np.asarray(min_eos_p, np.float32), (nr,)))
        st = np.array(np.broadcast_to(np.asarray(state, np.int32), (nr, 8)), np.int32, order="C")
        call = BarkHipSampleCall(int(mode), int(eos_token), int(token_base), int(prescaled), int(n_past_add), 1 if per_row else 0)
        ids = np.zeros(nr, np.int32)
        eos = np.zeros(nr, np.float32)
        if self._lib.bark_hip_sample_rows_state(self._h, lg.ctypes.data, nr, n, t.ctypes.data, k.ctypes.data, p.ctypes.data, uu.ctypes.data,
                                                me.ctypes.data, C.byref(call), st.ctypes.data, ids.ctypes.data, eos.ctypes.data) != 0:
            raise RuntimeError("bark_hip_sample_rows_state failed")
        return ids, eos, st

    def time_sample_filter(self, n: int, n_slots: int, top_k: int, top_p: float, peaked: bool, iters: int) -> float:
        us = self._lib.bark_hip_time_sample_filter(self._h, n, n_slots, int(top_k), float(top_p), 1 if peaked else 0, iters)
        if us < 0:
            raise RuntimeError("bark_hip_time_sample_filter failed")
        return us

    def set_fine_order(self, order: int):
        """0: default policy (C1 for generate_audio / stage calls, C1m inside lock-step jobs and fine_many); 1: C1 everywhere; 2: C1m everywhere."""
        if self._lib.bark_hip_set_fine_order(self._h, int(order)) != 0:
            raise RuntimeError("bark_hip_set_fine_order failed")

    def time_decode_step(self, which: int, ctx: int, iters: int):
        b = C.c_double(0)
        us = self._lib.bark_hip_time_decode_step(self._h, which, ctx, iters, C.byref(b))
        if us < 0:
            raise RuntimeError("bark_hip_time_decode_step failed")
        return us, b.value

    def time_gemv(self, which: int, op: int, iters: int):
        b = C.c_double(0)
        us = self._lib.bark_hip_time_gemv(self._h, which, op, iters, C.byref(b))
        if us < 0:
            raise RuntimeError("bark_hip_time_gemv failed")
        return us, b.value

    def time_slots(self, which: int, op: int, n_slots: int, kind: int, ctx: int, iters: int) -> float:
        us = self._lib.bark_hip_time_slots(self._h, which, op, n_slots, kind, ctx, iters)
        if us < 0:
            raise RuntimeError("bark_hip_time_slots failed")
        return us

    def profile_lock_step(self, which: int, n_slots: int, ctx: int, reps: int = 20) -> list:
        """[{"site", "us"}] per launch site of one lock step in launch order (kernel + the gap in front), closed by the graph-replayed step."""
        import json
        buf = C.create_string_buffer(1 << 16)
        n = self._lib.bark_hip_profile_lock_step(self._h, which, n_slots, ctx, reps, buf, len(buf))
        if n < 0:
            raise RuntimeError("bark_hip_profile_lock_step failed")
        return json.loads(buf.value.decode())

    def time_fine_pass(self, iters: int, n_windows: int = 1):
        """us per forward pass of the fine model over n_windows windows side by side, flops of that pass"""
        f = C.c_double(0)
        if n_windows > 1:
            us = self._lib.bark_hip_time_fine_passes(self._h, n_windows, iters, C.byref(f))
        else:
            us = self._lib.bark_hip_time_fine_pass(self._h, iters, C.byref(f))
        if us < 0:
            raise RuntimeError("bark_hip_time_fine_pass failed")
        return us, f.value


class Batcher:
    """bark_hip_batcher: thread-safe submit / wait in front of the context's lock-step batches (the context is owned by the batcher's
    worker thread while it lives)."""

    def __init__(self, ctx, max_batch: int = 32, max_wait_ms: int = 2, streams: int = 1):
        """ctx: one BarkContext (streams > 1: further workers on clones of it, same GPU), or a list of contexts - one worker each, typically one per GPU
        (bark_hip_batcher_create_multi)."""
        ctxs = list(ctx) if isinstance(ctx, (list, tuple)) else [ctx]
        self._lib = ctxs[0]._lib
        self._ctx = ctxs                                # the worker threads run on these contexts: they must outlive the batcher
        self._formats = {}                              # ticket -> sample format of the requests submitted with audio_format (wait_bytes picks the dtype)
        if len(ctxs) > 1:
            arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
            self._b = self._lib.bark_hip_batcher_create_multi(arr, len(ctxs), max_batch, max_wait_ms)
        else:
            self._b = self._lib.bark_hip_batcher_create_ex(ctxs[0]._h, max_batch, max_wait_ms, streams)     # streams > 1: further workers on clones of ctx
        if not self._b:
            raise RuntimeError("bark_hip_batcher_create failed")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def submit(self, text: str, seed: int = 0, params: "BarkHipRequestParams | None" = None, top_k: "int | None" = None, top_p: "float | None" = None,
               voice=None, audio_format: "BarkHipAudioFormat | None" = None, long=None, speed: "float | None" = None, loudness=None) -> int:
        """audio_format: the rate / sample format of the answer (api.audio_format(rate, "s16"); bark_hip_batcher_submit_as) - fetch it with wait_bytes().
        top_k / top_p: the request's own top-k / nucleus filter (bark_hip_batcher_submit_filtered; an omitted one of the two is off);
        neither given: the context's filter.  Without params the request takes the context's parameters with `seed`, as the plain submit does.
        voice: the request's own voice.VoicePrompt (bark_hip_batcher_submit_voiced; None: the context's).
        long: True or a BarkHipLongParams - a text of any length as one ticket (bark_hip_batcher_submit_long): its parts travel as ordinary requests, the
        answer is their joined audio.
        speed: the speaking rate of the answer, 0.5 .. 2.0 (bark_hip_batcher_submit_at / _submit_long_at, rule C16t) - fetch it with wait_bytes().
        loudness: the level of the answer in LUFS, -40 .. -5, or a BarkHipLoudnessParams (bark_hip_batcher_submit_with / _submit_long_with, rule C17l; the
        ceiling 1.0 and the cap 10 unless the struct says otherwise) - fetch it with wait_bytes()."""
        if loudness is not None:
            fmt = audio_format if audio_format is not None else BarkHipAudioFormat(24000, 0)
            lp_loud = loudness if isinstance(loudness, BarkHipLoudnessParams) else loudness_params(loudness)
            how = BarkHipAudioRender(fmt, speed_permille(1.0 if speed is None else speed), lp_loud)
            flt = None
            if top_k is not None or top_p is not None:
                flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            st, keep = _voice_struct(voice) if voice is not None else (None, None)
            common = (C.byref(params), None if flt is None else C.byref(flt), None if st is None else C.byref(st), C.byref(how))
            if long is not None and long is not False:
                lp = long if isinstance(long, BarkHipLongParams) else BarkHipLongParams(0, 0, join_params())
                t = self._lib.bark_hip_batcher_submit_long_with(self._b, text.encode("utf-8"), C.byref(lp), *common)
            else:
                t = self._lib.bark_hip_batcher_submit_with(self._b, text.encode("utf-8"), *common)
            if t > 0:
                self._formats[t] = int(fmt.sample_format)
        elif speed is not None:
            fmt = audio_format if audio_format is not None else BarkHipAudioFormat(24000, 0)
            flt = None
            if top_k is not None or top_p is not None:
                flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            st, keep = _voice_struct(voice) if voice is not None else (None, None)
            common = (C.byref(params), None if flt is None else C.byref(flt), None if st is None else C.byref(st), C.byref(fmt), speed_permille(speed))
            if long is not None and long is not False:
                lp = long if isinstance(long, BarkHipLongParams) else BarkHipLongParams(0, 0, join_params())
                t = self._lib.bark_hip_batcher_submit_long_at(self._b, text.encode("utf-8"), C.byref(lp), *common)
            else:
                t = self._lib.bark_hip_batcher_submit_at(self._b, text.encode("utf-8"), *common)
            if t > 0:
                self._formats[t] = int(fmt.sample_format)
        elif long is not None and long is not False:
            lp = long if isinstance(long, BarkHipLongParams) else BarkHipLongParams(0, 0, join_params())
            flt = None
            if top_k is not None or top_p is not None:
                flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            st, keep = _voice_struct(voice) if voice is not None else (None, None)
            t = self._lib.bark_hip_batcher_submit_long(self._b, text.encode("utf-8"), C.byref(lp), C.byref(params), None if flt is None else C.byref(flt),
                                                       None if st is None else C.byref(st), None if audio_format is None else C.byref(audio_format))
            if t > 0 and audio_format is not None:
                self._formats[t] = int(audio_format.sample_format)
        elif audio_format is not None:
            flt = None
            if top_k is not None or top_p is not None:
                flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            st, keep = _voice_struct(voice) if voice is not None else (None, None)
            t = self._lib.bark_hip_batcher_submit_as(self._b, text.encode("utf-8"), C.byref(params), None if flt is None else C.byref(flt),
                                                     None if st is None else C.byref(st), C.byref(audio_format))
            if t > 0:
                self._formats[t] = int(audio_format.sample_format)
        elif voice is not None:
            flt = None
            if top_k is not None or top_p is not None:
                flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            st, keep = _voice_struct(voice)
            t = self._lib.bark_hip_batcher_submit_voiced(self._b, text.encode("utf-8"), C.byref(params), None if flt is None else C.byref(flt), C.byref(st))
        elif top_k is not None or top_p is not None:
            flt = BarkHipSamplingFilter(0 if top_k is None else int(top_k), 1.0 if top_p is None else float(top_p))
            if params is None:
                params = self._ctx[0].request_params(seed=int(seed))
            t = self._lib.bark_hip_batcher_submit_filtered(self._b, text.encode("utf-8"), C.byref(params), C.byref(flt))
        elif params is not None:
            t = self._lib.bark_hip_batcher_submit_ex(self._b, text.encode("utf-8"), C.byref(params))
        else:
            t = self._lib.bark_hip_batcher_submit(self._b, text.encode("utf-8"), seed)
        if t <= 0:
            raise RuntimeError("bark_hip_batcher_submit failed")
        return t

    def wait(self, ticket: int) -> np.ndarray:
        n = self._lib.bark_hip_batcher_wait(self._b, ticket, None, 0)          # probe: -(2 + samples)
        if n > -2:
            raise RuntimeError("generation failed")
        pcm = np.zeros(max(-n - 2, 1), np.float32)                             # (a long text trimmed away entirely is 0 samples: the buffer still exists)
        n = self._lib.bark_hip_batcher_wait(self._b, ticket, pcm.ctypes.data, pcm.size)
        if n < 0:
            raise RuntimeError("bark_hip_batcher_wait failed")
        return pcm[:n]

    def wait_bytes(self, ticket: int) -> np.ndarray:
        """The answer of any request in its own format (bark_hip_batcher_wait_bytes): float32 / int16 / uint8 samples (a request without audio_format: float32)."""
        n = self._lib.bark_hip_batcher_wait_bytes(self._b, ticket, None, 0)    # probe: -(2 + bytes)
        if n > -2:
            raise RuntimeError("generation failed")
        buf = np.zeros(max(-n - 2, 1), np.uint8)                               # (0 bytes is a legal answer of a long text: the buffer still exists)
        n = self._lib.bark_hip_batcher_wait_bytes(self._b, ticket, buf.ctypes.data, buf.size)
        if n < 0:
            raise RuntimeError("bark_hip_batcher_wait_bytes failed")
        return buf[:n].view(SAMPLE_DTYPES[self._formats.pop(ticket, SAMPLE_F32)]).copy()

    def stats(self) -> dict:
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._lib.bark_hip_batcher_stats(self._b, C.byref(a), C.byref(b), C.byref(c))
        return {"n_batches": a.value, "n_requests": b.value, "largest_batch": c.value, "n_admitted": int(self._lib.bark_hip_batcher_admitted(self._b))}

    def free(self):
        if self._b:
            self._lib.bark_hip_batcher_free(self._b)
            self._b = None
        self._ctx = None
