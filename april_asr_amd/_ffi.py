"""ctypes view of libaprilasr.so (the MI355X build).

Struct layouts and enum values are the reference ABI's (include/april_api.h;
reference april_api.h:82-174, bindings/python/april_asr/_april_c_ffi.py:9-37):
AprilToken 32 bytes {0,8,12,16,24}, AprilConfig 40 bytes {0,16,24,32}.
The library is loaded from this package directory (built in-tree by
csrc/Makefile); there is no CPU fallback -- if it is missing, importing fails.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("APRIL_ASR_LIB") or os.path.join(_HERE, "libaprilasr.so")


class AprilSpeakerID(C.Structure):
    _fields_ = [("data", C.c_uint8 * 16)]


class AprilToken(C.Structure):
    _fields_ = [("token", C.c_char_p), ("logprob", C.c_float), ("flags", C.c_int),
                ("time_ms", C.c_size_t), ("reserved", C.c_void_p)]


HANDLER = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(AprilToken))


class AprilConfig(C.Structure):
    _fields_ = [("speaker", AprilSpeakerID), ("handler", HANDLER), ("userdata", C.c_void_p), ("flags", C.c_int)]


class AprilxDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_layers", "d_model", "hidden", "ffn", "joiner", "vocab", "mel", "seg",
                                         "seg_step", "context", "fft_size", "frame_shift", "sample_rate", "blank_id",
                                         "n_devices", "precision", "d_model_file")] + [("param_count", C.c_int64)]


class AprilxStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("ticks", "steps", "chunks", "rounds", "frames", "max_batch_seen")] + \
               [("kernel_ms", C.c_double * 6), ("kernel_launches", C.c_uint64 * 6), ("host_ms", C.c_double * 8),
                ("flights", C.c_uint64), ("replay_mismatch", C.c_uint64), ("kernels_per_step", C.c_uint64),
                ("lm_steps", C.c_uint64), ("lm_chunks", C.c_uint64),
                ("wave_steps", C.c_uint64), ("wave_chunks", C.c_uint64),
                ("gates_clock_ms", C.c_double), ("gates_clock_launches", C.c_uint64), ("gates_clock_rows", C.c_uint64),
                ("gates_clock_ms_by_n", C.c_double * 4), ("gates_clock_launches_by_n", C.c_uint64 * 4),
                ("resample_ms", C.c_double), ("resample_launches", C.c_uint64), ("confidence_records", C.c_uint64)]


class AprilxTokenInfo(C.Structure):
    _fields_ = [("size", C.c_uint32), ("n_alt", C.c_uint32), ("eval_index", C.c_uint64), ("lse", C.c_float),
                ("token_logprob", C.c_float), ("blank_logprob", C.c_float), ("reserved0", C.c_float),
                ("alt_id", C.c_int32 * 8), ("alt_logit", C.c_float * 8)]


class AprilxSearchOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("endpoint_silence_ms", C.c_uint32), ("max_utterance_ms", C.c_uint32), ("blank_penalty", C.c_float)]


class AprilxLoadInfo(C.Structure):
    _fields_ = [("broadcast_ms", C.c_double), ("comm_init_ms", C.c_double), ("broadcast_bytes", C.c_uint64),
                ("ranks", C.c_int32), ("used_rccl", C.c_int32)]


class AprilxVadOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("band_lo_hz", C.c_float), ("band_hi_hz", C.c_float), ("onset_db", C.c_float), ("offset_db", C.c_float),
                ("onset_ms", C.c_uint32), ("hangover_ms", C.c_uint32), ("min_energy", C.c_float), ("flags", C.c_uint32)]


class AprilxVadInfo(C.Structure):
    _fields_ = [("b0", C.c_int32), ("b1", C.c_int32), ("onset_frames", C.c_int32), ("hangover_frames", C.c_int32),
                ("frames_seen", C.c_uint64), ("speech_frames", C.c_uint64), ("in_speech", C.c_uint32), ("segments", C.c_uint32)]


class AprilxVadPlan(C.Structure):
    _fields_ = [("b0", C.c_int32), ("b1", C.c_int32), ("inv_nb", C.c_float), ("thr_on", C.c_float), ("thr_off", C.c_float),
                ("min_energy", C.c_float), ("onset_frames", C.c_int32), ("hangover_frames", C.c_int32)]


class AprilxVadState(C.Structure):
    _fields_ = [("s", C.c_float), ("cur", C.c_float), ("hist", C.c_float * 8), ("cnt", C.c_int32), ("pos", C.c_int32), ("st", C.c_int32),
                ("run", C.c_int32), ("first", C.c_int32), ("reserved", C.c_int32)]


VAD_HANDLER = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint64)


class AprilxDtmfOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("min_level_dbfs", C.c_float), ("twist_hi_db", C.c_float), ("twist_lo_db", C.c_float), ("rel_peak_db", C.c_float),
                ("min_share", C.c_float), ("min_tone_ms", C.c_uint32), ("min_pause_ms", C.c_uint32), ("flags", C.c_uint32)]


class AprilxDtmfInfo(C.Structure):
    _fields_ = [("Wd", C.c_int32), ("on_frames", C.c_int32), ("off_frames", C.c_int32), ("held", C.c_uint32),
                ("frames_seen", C.c_uint64), ("tone_frames", C.c_uint64), ("digits", C.c_uint64)]


class AprilxDtmfPlan(C.Structure):
    _fields_ = [("Wd", C.c_int32), ("half_w", C.c_float), ("min_power", C.c_float), ("twist_hi", C.c_float), ("twist_lo", C.c_float),
                ("rel_peak", C.c_float), ("min_share", C.c_float), ("on_frames", C.c_int32), ("off_frames", C.c_int32), ("reserved", C.c_int32)]


class AprilxDtmfMachine(C.Structure):
    _fields_ = [("held", C.c_int32), ("cand", C.c_int32), ("run", C.c_int32)]


DTMF_HANDLER = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char, C.c_uint64)


class AprilxToneOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("min_level_dbfs", C.c_float), ("second_db", C.c_float), ("min_share", C.c_float), ("tol_hz", C.c_uint32),
                ("min_tone_ms", C.c_uint32), ("min_pause_ms", C.c_uint32), ("flags", C.c_uint32)]


class AprilxToneInfo(C.Structure):
    _fields_ = [("W", C.c_int32), ("k_lo", C.c_int32), ("F", C.c_int32), ("on_frames", C.c_int32), ("off_frames", C.c_int32),
                ("held_f1", C.c_uint32), ("held_f2", C.c_uint32), ("reserved", C.c_uint32),
                ("frames_seen", C.c_uint64), ("tonal_frames", C.c_uint64), ("tones", C.c_uint64)]


class AprilxTonePlan(C.Structure):
    _fields_ = [("W", C.c_int32), ("k_lo", C.c_int32), ("F", C.c_int32), ("half_w", C.c_float), ("min_power", C.c_float), ("second_ratio", C.c_float),
                ("min_share", C.c_float), ("bin_hz", C.c_float), ("tol_hz", C.c_int32), ("on_frames", C.c_int32), ("off_frames", C.c_int32),
                ("reserved", C.c_int32)]


class AprilxToneMachine(C.Structure):
    _fields_ = [("held", C.c_int32), ("h1", C.c_int32), ("h2", C.c_int32), ("c1", C.c_int32), ("c2", C.c_int32), ("run", C.c_int32)]


TONE_HANDLER = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64)


class AprilxQualityOptions(C.Structure):
    _fields_ = [("size", C.c_uint32), ("flags", C.c_uint32), ("clip_level", C.c_uint32), ("clip_run_min", C.c_uint32), ("clip_hold_ms", C.c_uint32),
                ("dropout_ms", C.c_uint32), ("report_ms", C.c_uint32)]


class AprilxQualityEvent(C.Structure):
    _fields_ = [("kind", C.c_int32), ("frames", C.c_uint32), ("time_ms", C.c_uint64), ("sum", C.c_int64), ("sumsq", C.c_uint64), ("min", C.c_int32), ("max", C.c_int32),
                ("clip_samples", C.c_uint64), ("clipped_frames", C.c_uint32), ("dead_frames", C.c_uint32), ("quiet_sumsq", C.c_uint64), ("loud_sumsq", C.c_uint64),
                ("hop", C.c_uint32), ("reserved", C.c_uint32)]


class AprilxQualityInfo(C.Structure):
    _fields_ = [("hop", C.c_int32), ("hold_frames", C.c_int32), ("dropout_frames", C.c_int32), ("report_frames", C.c_int32), ("clipping", C.c_uint32), ("dropout", C.c_uint32),
                ("frames_seen", C.c_uint64), ("frames", C.c_uint64), ("clipped_frames", C.c_uint64), ("dead_frames", C.c_uint64), ("clip_samples", C.c_uint64),
                ("reports", C.c_uint64)]


class AprilxQualityPlan(C.Structure):
    _fields_ = [("hop", C.c_int32), ("clip_level", C.c_int32), ("clip_run_min", C.c_int32), ("hold_frames", C.c_int32), ("dropout_frames", C.c_int32),
                ("report_frames", C.c_int32)]


class AprilxQualityMachine(C.Structure):
    _fields_ = [("clipping", C.c_int32), ("dropout", C.c_int32), ("quiet_run", C.c_int32), ("dead_run", C.c_int32), ("frames", C.c_uint32), ("have_live", C.c_int32),
                ("first_frame", C.c_uint64), ("sum", C.c_int64), ("sumsq", C.c_uint64), ("min", C.c_int32), ("max", C.c_int32), ("clip_samples", C.c_uint64),
                ("clipped_frames", C.c_uint32), ("dead_frames", C.c_uint32), ("quiet_sumsq", C.c_uint64), ("loud_sumsq", C.c_uint64)]


QUALITY_HANDLER = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(AprilxQualityEvent))


class AprilxInputFormat(C.Structure):
    _fields_ = [("size", C.c_uint32), ("encoding", C.c_uint32), ("channels", C.c_uint32), ("channel", C.c_int32)]


class AprilxSnapshotInfo(C.Structure):
    _fields_ = ([("size", C.c_uint32), ("version", C.c_uint32), ("blob_size", C.c_uint64), ("params_hash", C.c_uint64), ("token_hash", C.c_uint64),
                 ("bias_hash", C.c_uint64), ("bias_edges", C.c_int64), ("chunks", C.c_uint64), ("frames_seen", C.c_uint64), ("now_ms", C.c_uint64),
                 ("rows_written", C.c_uint64)]
                + [(n, C.c_int32) for n in ("n_layers", "d_model", "hidden", "ffn", "joiner", "vocab", "mel", "segment_size", "segment_step", "sample_rate",
                                            "frame_shift_ms", "blank_id")]
                + [(n, C.c_uint32) for n in ("precision", "f16_tile", "input_rate", "confidence_k", "has_format", "has_search_options", "has_vad", "has_dtmf",
                                             "has_tones", "has_bias", "bias_flags")]
                + [("bias_states", C.c_int32), ("ring_rows", C.c_uint32), ("reserved", C.c_uint32), ("format", AprilxInputFormat), ("search", AprilxSearchOptions),
                   ("vad", AprilxVadOptions), ("dtmf", AprilxDtmfOptions), ("tones", AprilxToneOptions), ("name", C.c_char * 64), ("description", C.c_char * 128)])


EXPORTED_REFERENCE_SYMBOLS = [
    "aam_api_init", "aam_create_model", "aam_get_name", "aam_get_description", "aam_get_language",
    "aam_get_sample_rate", "aam_free", "aas_create_session", "aas_feed_pcm16", "aas_flush",
    "aas_realtime_get_speedup", "aas_free",
]
EXPORTED_ENGINE_SYMBOLS = [
    "aprilx_model_dims", "aprilx_model_token", "aprilx_model_blob_size", "aprilx_model_export_blob",
    "aprilx_model_from_blob", "aprilx_model_save_blob", "aprilx_model_save_blob_f16", "aprilx_model_load_blob",
    "aprilx_broadcast_get_id", "aprilx_model_broadcast", "aprilx_model_load_info", "aprilx_feed_many", "aprilx_flush_many", "aprilx_session_drain", "aprilx_feed_many_pipelined", "aprilx_drain_many",
    "aprilx_run_encoder", "aprilx_run_decoder", "aprilx_run_joiner", "aprilx_run_fbank", "aprilx_run_decide", "aprilx_plan_gemm", "aprilx_gemm_plan_debug", "aprilx_run_gemm", "aprilx_stream_form", "aprilx_run_conv_front", "aprilx_conv_front_geometry",
    "aprilx_session_trace_logits", "aprilx_session_chunks", "aprilx_session_read_frames", "aprilx_session_context", "aprilx_model_stats", "aprilx_model_profile", "aprilx_model_feed_latency",
    "aprilx_greedy_create", "aprilx_greedy_step", "aprilx_greedy_finish", "aprilx_greedy_free", "aprilx_probe_file", "aprilx_model_load_host", "aprilx_model_fbank_tables", "aprilx_counting_handler",
    "aprilx_session_set_input_rate", "aprilx_session_input_rate", "aprilx_resampler_taps", "aprilx_resample",
    "aprilx_session_set_confidence", "aprilx_session_confidence", "aprilx_run_confidence",
    "aprilx_bias_create", "aprilx_bias_free", "aprilx_bias_info", "aprilx_bias_edges", "aprilx_session_set_bias", "aprilx_session_bias_state",
    "aprilx_run_decide_biased", "aprilx_greedy_set_bias", "aprilx_greedy_bias_state",
    "aprilx_bias_create_ex", "aprilx_bias_flags", "aprilx_run_confidence_biased",
    "aprilx_session_set_search_options", "aprilx_session_search_options", "aprilx_run_decide_opts", "aprilx_greedy_set_search_options",
    "aprilx_ramp_window", "aprilx_model_ramp_stats", "aprilx_model_ramp_stats2",
    "aprilx_session_set_input_format", "aprilx_session_input_format", "aprilx_session_feed_bytes", "aprilx_feed_many_bytes",
    "aprilx_decode_host", "aprilx_decode", "aprilx_model_decode_stats",
    "aprilx_session_set_vad", "aprilx_session_vad", "aprilx_vad_plan_tables", "aprilx_vad_host", "aprilx_vad_events_host", "aprilx_run_vad",
    "aprilx_model_vad_stats",
    "aprilx_session_set_dtmf", "aprilx_session_dtmf", "aprilx_dtmf_plan", "aprilx_dtmf_tables", "aprilx_dtmf_host", "aprilx_dtmf_decide_host",
    "aprilx_dtmf_events_host", "aprilx_run_dtmf", "aprilx_run_dtmf_decide", "aprilx_model_dtmf_stats",
    "aprilx_session_set_tones", "aprilx_session_tones", "aprilx_tone_plan", "aprilx_tone_tables", "aprilx_tone_host", "aprilx_tone_decide_host",
    "aprilx_tone_events_host", "aprilx_tone_name", "aprilx_run_tones", "aprilx_run_tone_decide", "aprilx_model_tone_stats",
    "aprilx_session_set_quality", "aprilx_session_quality", "aprilx_quality_plan", "aprilx_quality_host", "aprilx_quality_events_host", "aprilx_run_quality",
    "aprilx_model_quality_stats",
    "aprilx_session_snapshot", "aprilx_session_restore", "aprilx_snapshot_info", "aprilx_snapshot_many", "aprilx_restore_many", "aprilx_model_snapshot_stats",
    "aprilx_lm_create", "aprilx_lm_free", "aprilx_lm_info", "aprilx_lm_arrays", "aprilx_lm_score_host", "aprilx_session_set_lm", "aprilx_session_lm_state",
    "aprilx_greedy_set_lm", "aprilx_greedy_lm_state", "aprilx_model_lm_stats", "aprilx_run_decide_lm", "aprilx_run_confidence_lm",
]

_lib = None
_inited = False


def lib():
    """Load the shared library and declare prototypes (no GPU needed for this)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("libaprilasr.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C april_asr_amd/csrc` (hipcc, gfx950). There is no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, sz = C.c_void_p, C.c_size_t
    L.aam_api_init.argtypes = [C.c_int]; L.aam_api_init.restype = None
    L.aam_create_model.argtypes = [C.c_char_p]; L.aam_create_model.restype = vp
    for f in ("aam_get_name", "aam_get_description", "aam_get_language"):
        getattr(L, f).argtypes = [vp]; getattr(L, f).restype = C.c_char_p
    L.aam_get_sample_rate.argtypes = [vp]; L.aam_get_sample_rate.restype = sz
    L.aam_free.argtypes = [vp]; L.aam_free.restype = None
    L.aas_create_session.argtypes = [vp, AprilConfig]; L.aas_create_session.restype = vp
    L.aas_feed_pcm16.argtypes = [vp, vp, sz]; L.aas_feed_pcm16.restype = None
    L.aas_flush.argtypes = [vp]; L.aas_flush.restype = None
    L.aas_realtime_get_speedup.argtypes = [vp]; L.aas_realtime_get_speedup.restype = C.c_float
    L.aas_free.argtypes = [vp]; L.aas_free.restype = None
    L.aprilx_model_dims.argtypes = [vp, C.POINTER(AprilxDims)]; L.aprilx_model_dims.restype = C.c_int
    L.aprilx_model_token.argtypes = [vp, C.c_int32]; L.aprilx_model_token.restype = C.c_char_p
    L.aprilx_model_blob_size.argtypes = [vp]; L.aprilx_model_blob_size.restype = sz
    L.aprilx_model_export_blob.argtypes = [vp, vp, sz]; L.aprilx_model_export_blob.restype = C.c_int
    L.aprilx_model_from_blob.argtypes = [vp, sz, C.c_int]; L.aprilx_model_from_blob.restype = vp
    L.aprilx_model_save_blob.argtypes = [vp, C.c_char_p]; L.aprilx_model_save_blob.restype = C.c_int
    L.aprilx_model_save_blob_f16.argtypes = [vp, C.c_char_p]; L.aprilx_model_save_blob_f16.restype = C.c_int
    L.aprilx_model_load_blob.argtypes = [C.c_char_p]; L.aprilx_model_load_blob.restype = vp
    L.aprilx_broadcast_get_id.argtypes = [vp, sz]; L.aprilx_broadcast_get_id.restype = C.c_int
    L.aprilx_model_broadcast.argtypes = [vp, C.c_int, C.c_int, vp]; L.aprilx_model_broadcast.restype = vp
    L.aprilx_model_load_info.argtypes = [vp, C.POINTER(AprilxLoadInfo)]; L.aprilx_model_load_info.restype = C.c_int
    L.aprilx_feed_many.argtypes = [sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz)]; L.aprilx_feed_many.restype = None
    L.aprilx_flush_many.argtypes = [sz, C.POINTER(vp)]; L.aprilx_flush_many.restype = None
    L.aprilx_session_drain.argtypes = [vp]; L.aprilx_session_drain.restype = None
    L.aprilx_feed_many_pipelined.argtypes = [sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int]; L.aprilx_feed_many_pipelined.restype = None
    L.aprilx_drain_many.argtypes = [sz, C.POINTER(vp)]; L.aprilx_drain_many.restype = None
    L.aprilx_run_encoder.argtypes = [vp, C.c_int] + [vp] * 6; L.aprilx_run_encoder.restype = C.c_int
    L.aprilx_run_decoder.argtypes = [vp, C.c_int, vp, vp]; L.aprilx_run_decoder.restype = C.c_int
    L.aprilx_run_joiner.argtypes = [vp, C.c_int, vp, vp, vp]; L.aprilx_run_joiner.restype = C.c_int
    L.aprilx_run_fbank.argtypes = [vp, C.c_int, vp, vp]; L.aprilx_run_fbank.restype = C.c_int
    L.aprilx_plan_gemm.argtypes = [C.c_int] * 6 + [vp]; L.aprilx_plan_gemm.restype = C.c_int
    L.aprilx_gemm_plan_debug.argtypes = [vp, vp]; L.aprilx_gemm_plan_debug.restype = C.c_int
    L.aprilx_run_gemm.argtypes = [vp] * 5; L.aprilx_run_gemm.restype = C.c_int
    L.aprilx_run_conv_front.argtypes = [vp] * 4; L.aprilx_run_conv_front.restype = C.c_int
    L.aprilx_conv_front_geometry.argtypes = [vp] * 2; L.aprilx_conv_front_geometry.restype = C.c_int
    L.aprilx_ramp_window.argtypes = [C.c_int] * 3 + [vp, C.c_int]; L.aprilx_ramp_window.restype = C.c_int
    L.aprilx_model_ramp_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]; L.aprilx_model_ramp_stats.restype = C.c_int
    L.aprilx_model_ramp_stats2.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64)]; L.aprilx_model_ramp_stats2.restype = C.c_int
    L.aprilx_stream_form.argtypes = [C.c_int] * 6; L.aprilx_stream_form.restype = C.c_int
    L.aprilx_run_decide.argtypes = [vp, C.c_int, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp]; L.aprilx_run_decide.restype = C.c_int
    L.aprilx_session_trace_logits.argtypes = [vp, vp, sz, C.POINTER(sz)]; L.aprilx_session_trace_logits.restype = None
    L.aprilx_session_chunks.argtypes = [vp]; L.aprilx_session_chunks.restype = C.c_uint64
    L.aprilx_session_read_frames.argtypes = [vp, C.c_uint64, C.c_int, C.c_void_p]; L.aprilx_session_read_frames.restype = C.c_uint64
    L.aprilx_session_context.argtypes = [vp, vp, vp]; L.aprilx_session_context.restype = None
    L.aprilx_model_stats.argtypes = [vp, C.c_int, C.POINTER(AprilxStats)]; L.aprilx_model_stats.restype = None
    L.aprilx_model_feed_latency.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]; L.aprilx_model_feed_latency.restype = C.c_int
    L.aprilx_model_profile.argtypes = [vp, C.c_int]; L.aprilx_model_profile.restype = None
    L.aprilx_greedy_create.argtypes = [vp, HANDLER, vp]; L.aprilx_greedy_create.restype = vp
    L.aprilx_greedy_step.argtypes = [vp, C.c_int32, C.c_float, C.c_float, C.c_float, sz, C.POINTER(C.c_int32)]
    L.aprilx_greedy_step.restype = C.c_int
    L.aprilx_greedy_finish.argtypes = [vp]; L.aprilx_greedy_finish.restype = None
    L.aprilx_greedy_free.argtypes = [vp]; L.aprilx_greedy_free.restype = None
    L.aprilx_model_load_host.argtypes = [C.c_char_p]; L.aprilx_model_load_host.restype = vp
    L.aprilx_model_fbank_tables.argtypes = [vp, vp, vp]; L.aprilx_model_fbank_tables.restype = C.c_int
    L.aprilx_probe_file.argtypes = [C.c_char_p, C.c_char_p, sz]; L.aprilx_probe_file.restype = C.c_int
    L.aprilx_session_set_input_rate.argtypes = [vp, C.c_uint32]; L.aprilx_session_set_input_rate.restype = C.c_int
    L.aprilx_session_input_rate.argtypes = [vp]; L.aprilx_session_input_rate.restype = C.c_uint32
    L.aprilx_resampler_taps.argtypes = [C.c_uint32, C.c_uint32, vp, vp, sz]; L.aprilx_resampler_taps.restype = C.c_int
    L.aprilx_resample.argtypes = [vp, C.c_uint32, vp, sz, vp, sz]; L.aprilx_resample.restype = C.c_int64
    L.aprilx_session_set_confidence.argtypes = [vp, C.c_int]; L.aprilx_session_set_confidence.restype = C.c_int
    L.aprilx_session_confidence.argtypes = [vp]; L.aprilx_session_confidence.restype = C.c_int
    L.aprilx_run_confidence.argtypes = [vp, C.c_int, vp, C.c_int, vp]; L.aprilx_run_confidence.restype = C.c_int
    L.aprilx_bias_create.argtypes = [vp, sz, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_char_p, sz]; L.aprilx_bias_create.restype = vp
    L.aprilx_bias_create_ex.argtypes = [vp, sz, C.POINTER(C.c_char_p), C.POINTER(C.c_float), C.c_uint32, C.c_char_p, sz]; L.aprilx_bias_create_ex.restype = vp
    L.aprilx_bias_flags.argtypes = [vp]; L.aprilx_bias_flags.restype = C.c_int
    L.aprilx_run_confidence_biased.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp]; L.aprilx_run_confidence_biased.restype = C.c_int
    L.aprilx_bias_free.argtypes = [vp]; L.aprilx_bias_free.restype = None
    L.aprilx_lm_create.argtypes = [vp, vp, sz, C.c_int, C.c_char_p, sz]; L.aprilx_lm_create.restype = vp
    L.aprilx_lm_free.argtypes = [vp]; L.aprilx_lm_free.restype = None
    L.aprilx_lm_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]; L.aprilx_lm_info.restype = C.c_int
    L.aprilx_lm_arrays.argtypes = [vp] * 7 + [C.POINTER(C.c_float), sz, sz]; L.aprilx_lm_arrays.restype = C.c_int
    L.aprilx_lm_score_host.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]; L.aprilx_lm_score_host.restype = C.c_int
    L.aprilx_session_set_lm.argtypes = [vp, vp, C.c_float, C.c_float]; L.aprilx_session_set_lm.restype = C.c_int
    L.aprilx_session_lm_state.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]; L.aprilx_session_lm_state.restype = C.c_int
    L.aprilx_greedy_set_lm.argtypes = [vp, vp, C.c_float, C.c_float]; L.aprilx_greedy_set_lm.restype = C.c_int
    L.aprilx_greedy_lm_state.argtypes = [vp]; L.aprilx_greedy_lm_state.restype = C.c_int
    L.aprilx_model_lm_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]; L.aprilx_model_lm_stats.restype = C.c_int
    L.aprilx_run_decide_lm.argtypes = [vp, C.c_int, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float]; L.aprilx_run_decide_lm.restype = C.c_int
    L.aprilx_run_confidence_lm.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_float, C.c_float, vp]; L.aprilx_run_confidence_lm.restype = C.c_int
    L.aprilx_bias_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]; L.aprilx_bias_info.restype = C.c_int
    L.aprilx_bias_edges.argtypes = [vp, C.c_int32, vp, vp, vp, sz]; L.aprilx_bias_edges.restype = C.c_int
    L.aprilx_session_set_bias.argtypes = [vp, vp]; L.aprilx_session_set_bias.restype = C.c_int
    L.aprilx_session_bias_state.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]; L.aprilx_session_bias_state.restype = C.c_int
    L.aprilx_run_decide_biased.argtypes = [vp, C.c_int, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp, vp, vp]; L.aprilx_run_decide_biased.restype = C.c_int
    L.aprilx_greedy_set_bias.argtypes = [vp, vp]; L.aprilx_greedy_set_bias.restype = C.c_int
    L.aprilx_greedy_bias_state.argtypes = [vp]; L.aprilx_greedy_bias_state.restype = C.c_int
    L.aprilx_session_set_search_options.argtypes = [vp, C.POINTER(AprilxSearchOptions)]; L.aprilx_session_set_search_options.restype = C.c_int
    L.aprilx_session_search_options.argtypes = [vp, C.POINTER(AprilxSearchOptions)]; L.aprilx_session_search_options.restype = C.c_int
    L.aprilx_run_decide_opts.argtypes = [vp, C.c_int, C.c_int, vp, C.c_float, vp, C.c_int, vp, vp, vp, vp, vp]; L.aprilx_run_decide_opts.restype = C.c_int
    L.aprilx_greedy_set_search_options.argtypes = [vp, C.POINTER(AprilxSearchOptions)]; L.aprilx_greedy_set_search_options.restype = C.c_int
    L.aprilx_session_set_input_format.argtypes = [vp, C.POINTER(AprilxInputFormat)]; L.aprilx_session_set_input_format.restype = C.c_int
    L.aprilx_session_input_format.argtypes = [vp, C.POINTER(AprilxInputFormat)]; L.aprilx_session_input_format.restype = C.c_int
    L.aprilx_session_feed_bytes.argtypes = [vp, vp, sz]; L.aprilx_session_feed_bytes.restype = C.c_int
    L.aprilx_feed_many_bytes.argtypes = [sz, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.c_int]; L.aprilx_feed_many_bytes.restype = C.c_int
    L.aprilx_decode_host.argtypes = [C.POINTER(AprilxInputFormat), vp, sz, vp, sz]; L.aprilx_decode_host.restype = C.c_int64
    L.aprilx_decode.argtypes = [vp, C.POINTER(AprilxInputFormat), vp, sz, vp, sz]; L.aprilx_decode.restype = C.c_int64
    L.aprilx_model_decode_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]; L.aprilx_model_decode_stats.restype = C.c_int
    L.aprilx_session_set_vad.argtypes = [vp, C.POINTER(AprilxVadOptions), VAD_HANDLER, vp]; L.aprilx_session_set_vad.restype = C.c_int
    L.aprilx_session_vad.argtypes = [vp, C.POINTER(AprilxVadOptions), C.POINTER(AprilxVadInfo)]; L.aprilx_session_vad.restype = C.c_int
    L.aprilx_vad_plan_tables.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(AprilxVadOptions), C.POINTER(AprilxVadPlan)]; L.aprilx_vad_plan_tables.restype = C.c_int
    L.aprilx_vad_host.argtypes = [C.POINTER(AprilxVadPlan), C.c_int, C.c_int, vp, C.POINTER(AprilxVadState), vp, vp]; L.aprilx_vad_host.restype = C.c_int
    L.aprilx_vad_events_host.argtypes = [C.POINTER(AprilxVadPlan), C.c_int, C.c_uint64, vp, sz, C.POINTER(C.c_int32), vp, vp, C.c_int]; L.aprilx_vad_events_host.restype = C.c_int
    L.aprilx_run_vad.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp]; L.aprilx_run_vad.restype = C.c_int
    L.aprilx_model_vad_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]; L.aprilx_model_vad_stats.restype = C.c_int
    L.aprilx_session_set_dtmf.argtypes = [vp, C.POINTER(AprilxDtmfOptions), DTMF_HANDLER, vp]; L.aprilx_session_set_dtmf.restype = C.c_int
    L.aprilx_session_dtmf.argtypes = [vp, C.POINTER(AprilxDtmfOptions), C.POINTER(AprilxDtmfInfo)]; L.aprilx_session_dtmf.restype = C.c_int
    L.aprilx_dtmf_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(AprilxDtmfOptions), C.POINTER(AprilxDtmfPlan)]; L.aprilx_dtmf_plan.restype = C.c_int
    L.aprilx_dtmf_tables.argtypes = [C.c_int, C.c_int, vp, sz]; L.aprilx_dtmf_tables.restype = C.c_int
    L.aprilx_dtmf_host.argtypes = [C.POINTER(AprilxDtmfPlan), vp, C.c_int, vp, sz, vp, vp]; L.aprilx_dtmf_host.restype = C.c_int
    L.aprilx_dtmf_decide_host.argtypes = [C.POINTER(AprilxDtmfPlan), vp]; L.aprilx_dtmf_decide_host.restype = C.c_int
    L.aprilx_dtmf_events_host.argtypes = [C.POINTER(AprilxDtmfPlan), C.c_int, C.c_uint64, vp, sz, C.c_int, C.POINTER(AprilxDtmfMachine), vp, vp, vp, C.c_int]
    L.aprilx_dtmf_events_host.restype = C.c_int
    L.aprilx_run_dtmf.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]; L.aprilx_run_dtmf.restype = C.c_int
    L.aprilx_run_dtmf_decide.argtypes = [vp, C.POINTER(AprilxDtmfOptions), C.c_int, vp, vp]; L.aprilx_run_dtmf_decide.restype = C.c_int
    L.aprilx_model_dtmf_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]; L.aprilx_model_dtmf_stats.restype = C.c_int
    L.aprilx_session_set_tones.argtypes = [vp, C.POINTER(AprilxToneOptions), TONE_HANDLER, vp]; L.aprilx_session_set_tones.restype = C.c_int
    L.aprilx_session_tones.argtypes = [vp, C.POINTER(AprilxToneOptions), C.POINTER(AprilxToneInfo)]; L.aprilx_session_tones.restype = C.c_int
    L.aprilx_tone_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(AprilxToneOptions), C.POINTER(AprilxTonePlan)]; L.aprilx_tone_plan.restype = C.c_int
    L.aprilx_tone_tables.argtypes = [C.c_int, C.c_int, vp, sz]; L.aprilx_tone_tables.restype = C.c_int
    L.aprilx_tone_host.argtypes = [C.POINTER(AprilxTonePlan), vp, C.c_int, vp, sz, vp, vp]; L.aprilx_tone_host.restype = C.c_int
    L.aprilx_tone_decide_host.argtypes = [C.POINTER(AprilxTonePlan), vp]; L.aprilx_tone_decide_host.restype = C.c_int64
    L.aprilx_tone_events_host.argtypes = [C.POINTER(AprilxTonePlan), C.c_int, C.c_uint64, vp, sz, C.c_int, C.POINTER(AprilxToneMachine), vp, vp, vp, vp, C.c_int]
    L.aprilx_tone_events_host.restype = C.c_int
    L.aprilx_tone_name.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]; L.aprilx_tone_name.restype = C.c_char_p
    L.aprilx_run_tones.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp]; L.aprilx_run_tones.restype = C.c_int
    L.aprilx_run_tone_decide.argtypes = [vp, C.POINTER(AprilxToneOptions), C.c_int, vp, vp]; L.aprilx_run_tone_decide.restype = C.c_int
    L.aprilx_model_tone_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]; L.aprilx_model_tone_stats.restype = C.c_int
    L.aprilx_session_snapshot.argtypes = [vp, vp, sz]; L.aprilx_session_snapshot.restype = C.c_int64
    L.aprilx_session_restore.argtypes = [vp, vp, sz, vp, sz]; L.aprilx_session_restore.restype = C.c_int
    L.aprilx_snapshot_info.argtypes = [vp, sz, C.POINTER(AprilxSnapshotInfo)]; L.aprilx_snapshot_info.restype = C.c_int
    L.aprilx_snapshot_many.argtypes = [sz, vp, vp, vp, vp]; L.aprilx_snapshot_many.restype = C.c_int
    L.aprilx_restore_many.argtypes = [sz, vp, vp, vp, vp]; L.aprilx_restore_many.restype = C.c_int
    L.aprilx_model_snapshot_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.aprilx_model_snapshot_stats.restype = C.c_int
    L.aprilx_session_set_quality.argtypes = [vp, C.POINTER(AprilxQualityOptions), QUALITY_HANDLER, vp]; L.aprilx_session_set_quality.restype = C.c_int
    L.aprilx_session_quality.argtypes = [vp, C.POINTER(AprilxQualityOptions), C.POINTER(AprilxQualityInfo)]; L.aprilx_session_quality.restype = C.c_int
    L.aprilx_quality_plan.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(AprilxQualityOptions), C.POINTER(AprilxQualityPlan)]; L.aprilx_quality_plan.restype = C.c_int
    L.aprilx_quality_host.argtypes = [C.c_int, C.c_int, C.c_int, vp, sz, vp]; L.aprilx_quality_host.restype = C.c_int
    L.aprilx_quality_events_host.argtypes = [C.POINTER(AprilxQualityPlan), C.c_int, C.c_uint64, vp, sz, C.c_int, C.POINTER(AprilxQualityMachine), vp, C.c_int]
    L.aprilx_quality_events_host.restype = C.c_int
    L.aprilx_run_quality.argtypes = [vp, vp, C.c_int, vp, vp, vp]; L.aprilx_run_quality.restype = C.c_int
    L.aprilx_model_quality_stats.argtypes = [vp, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]; L.aprilx_model_quality_stats.restype = C.c_int
    _lib = L
    return L


def init():
    """aam_api_init(APRIL_VERSION) once per process (reference binding does this at import)."""
    global _inited
    L = lib()
    if not _inited:
        L.aam_api_init(1)
        _inited = True
    return L
