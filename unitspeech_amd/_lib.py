"""ctypes binding of libunitspeech_hip.so (the C ABI of include/unitspeech_hip.h).

There is deliberately no fallback: if the library is missing it is built with hipcc, and if that fails
(or a call returns an error code) a RuntimeError is raised."""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import _build

US_OK = 0
US_CREATE_EXACT_FP32 = 1
US_RANGE_ACT, US_RANGE_WEIGHT = 1, 2
US_BACKWARD_GRADS_ZEROED, US_BACKWARD_KEEP_TAPE = 1, 2
(US_DEBUG_BLOCK, US_DEBUG_RESNET, US_DEBUG_ATTENTION, US_DEBUG_DOWN, US_DEBUG_UP, US_DEBUG_TEMB, US_DEBUG_FIRST,
 US_DEBUG_FINAL) = range(8)          # us_debug_block's kinds
US_ENCODER_CONV_FWD, US_ENCODER_CONV_WGRAD, US_ENCODER_CONV_DGRAD = 0, 1, 2
US_ENCODER_CONV_MASK_IN, US_ENCODER_CONV_RELU, US_ENCODER_CONV_MASK_OUT = 1, 2, 4
ERRORS = {-1: "EINVAL", -2: "ENOKEY", -3: "ESHAPE", -4: "EWEIGHTS", -5: "EWORKSPACE", -6: "EHIP"}


class us_config(C.Structure):
    _fields_ = [("n_feats", C.c_int32), ("dim", C.c_int32), ("n_mults", C.c_int32), ("dim_mults", C.c_int32 * 6),
                ("spk_emb_dim", C.c_int32), ("beta_min", C.c_float), ("beta_max", C.c_float), ("pe_scale", C.c_float)]


class us_encoder_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_vocab", "n_feats", "n_channels", "filter_channels", "n_heads", "n_layers", "kernel_size",
                                         "window_size")]


class us_duration_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_channels", "filter_channels", "kernel_size", "spk_emb_dim")]


class us_vocoder_config(C.Structure):
    _fields_ = [("num_mels", C.c_int32), ("upsample_initial_channel", C.c_int32), ("resblock", C.c_int32), ("n_up", C.c_int32),
                ("upsample_rates", C.c_int32 * 8), ("upsample_kernel_sizes", C.c_int32 * 8), ("n_kernels", C.c_int32),
                ("resblock_kernel_sizes", C.c_int32 * 4), ("resblock_dilation_sizes", (C.c_int32 * 3) * 4), ("activation", C.c_int32),
                ("snake_logscale", C.c_int32)]


US_VOCODER_SNAKE, US_VOCODER_SNAKEBETA = 0, 1
US_SPEAKER_ACT_NONE, US_SPEAKER_ACT_RELU, US_SPEAKER_ACT_TANH = 0, 1, 2


class us_speaker_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("feat_dim", "channels", "emb_dim", "n_layers", "global_context_att")]


class us_mel_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_fft", "hop", "win", "num_mels")]


class us_resample_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("orig_freq", "new_freq", "width")]


US_CTC_WHOLE, US_CTC_FORWARD, US_CTC_BACKWARD = 0, 1, 2
US_LEVEL_F32, US_LEVEL_I16 = 0, 1
US_HUBERT_MAX_CONV = 8
US_HUBERT_NORM_GROUP, US_HUBERT_NORM_LAYER = 0, 1


class us_hubert_config(C.Structure):
    _fields_ = ([("n_conv", C.c_int32)] + [(n, C.c_int32 * US_HUBERT_MAX_CONV) for n in ("conv_dim", "conv_kernel", "conv_stride")] +
                [(n, C.c_int32) for n in ("hidden_size", "n_heads", "intermediate_size", "n_layers", "pos_conv_kernel", "pos_conv_groups",
                                          "feat_extract_norm", "do_stable_layer_norm")] + [("layer_norm_eps", C.c_float)])


class us_wavlm_config(C.Structure):
    _fields_ = us_hubert_config._fields_ + [(n, C.c_int32) for n in ("conv_bias", "num_buckets", "max_bucket_distance")]


class us_whisper_config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "d_model", "encoder_layers", "encoder_heads", "encoder_ffn", "decoder_layers", "decoder_heads",
                                         "decoder_ffn", "max_source_positions", "max_target_positions", "vocab_size")]


class us_whisper_decode_options(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("eos", "no_timestamps", "max_initial_timestamp_index", "no_speech", "sot_index", "max_new")]


class us_whisper_history(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_sampled", "last", "penultimate", "last_timestamp", "done")]


# symbol -> (restype, argtypes); must list every function declared in include/unitspeech_hip.h
SIGNATURES = {
    "us_decoder_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_config)]),
    "us_decoder_create_ex": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_config), C.c_uint]),
    "us_decoder_destroy": (C.c_int, [C.c_void_p]),
    "us_range_status": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint), C.c_int, C.c_void_p]),
    "us_range_status_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "us_decoder_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    "us_decoder_flush_weights": (C.c_int, [C.c_void_p, C.c_void_p]),
    "us_decoder_set_training": (C.c_int, [C.c_void_p, C.c_int]),
    "us_decoder_stale_inference_forms": (C.c_int, [C.c_void_p]),
    "us_decoder_num_weights": (C.c_int, [C.c_void_p]),
    "us_decoder_num_loaded": (C.c_int, [C.c_void_p]),
    "us_decoder_weight_key": (C.c_char_p, [C.c_void_p, C.c_int]),
    "us_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_sampler_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "us_estimator_forward": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_reverse_diffusion": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5 + [C.c_uint64, C.c_int64, C.c_int, C.c_int, C.c_int,
                                                                          C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p,
                                                                          C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_step_coefficients": (C.c_int, [C.c_int, C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "us_fill_normal": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p]),
    "us_estimator_flops": (C.c_double, [C.c_void_p, C.c_int]),
    "us_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_estimator_forward_train": (C.c_int, [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                                                               C.POINTER(C.c_uint64), C.c_void_p]),
    "us_estimator_backward": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                                        C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "us_tape_release": (C.c_int, [C.c_void_p, C.c_uint64]),
    "us_grad_is_overwritten": (C.c_int, [C.c_void_p, C.c_char_p]),
    "us_forward_diffusion": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p]),
    "us_diffusion_loss_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "us_diffusion_loss": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_scale": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_pow2_scale": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]),
    "us_mul_mask": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "us_finetune_segment": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 5 + [C.c_void_p]),
    "us_tts_durations": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "us_tts_align": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_void_p]),
    "us_vc_align": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "us_encoder_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_encoder_config)]),
    "us_encoder_create_contentvec": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_encoder_config), C.c_int32]),
    "us_encoder_forward_features": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_forward_features_train": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_size_t,
                                                                      C.c_void_p]),
    "us_encoder_backward_features": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.c_int,
                                                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_duration_predictor_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_duration_config)]),
    "us_encoder_forward": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_encoder_forward_train": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_size_t,
                                                             C.c_void_p]),
    "us_encoder_backward": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.c_int,
                                                        C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_dropout_mask": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "us_encoder_tape_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "us_encoder_debug_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_encoder_debug_conv": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int] + [C.c_void_p] * 5 + [C.c_float, C.c_uint, C.c_int, C.c_float, C.c_uint64]
                              + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_debug_ln_bwd": (C.c_int, [C.c_void_p, C.c_char_p] + [C.c_void_p] * 3 + [C.c_float] + [C.c_void_p] * 3
                                + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_debug_attention": (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_float, C.c_uint64] + [C.c_void_p] * 9
                                   + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_encoder_debug_embed_grad": (C.c_int, [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    "us_finetune_segment_backward": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]),
    "us_prior_loss": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p]),
    "us_mas_log_prior": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p]),
    "us_maximum_path_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "us_maximum_path": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_duration_loss": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 2 + [C.c_void_p]),
    "us_duration_predictor_forward": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_duration_predictor_train_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_duration_predictor_forward_train": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_void_p, C.c_size_t,
                                                                        C.c_void_p]),
    "us_duration_predictor_backward": (C.c_int, [C.c_void_p] * 2 + [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.c_int,
                                                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_duration_predictor_dropout_mask": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "us_duration_predictor_tape_release": (C.c_int, [C.c_void_p, C.c_void_p]),
    "us_duration_predictor_mse_loss": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]),
    "us_vocoder_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_vocoder_config)]),
    "us_vocoder_forward": (C.c_int, [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_vocoder_debug_layer": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_int,
                                         C.c_void_p]),
    "us_vocoder_forward_lengths": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    "us_vocoder_debug_layer_lengths": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int,
                                                 C.c_int, C.POINTER(C.c_int64), C.c_void_p]),
    "us_speaker_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_speaker_config)]),
    "us_speaker_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_speaker_forward_lengths": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_void_p, C.c_int, C.c_void_p,
                                             C.c_size_t, C.c_void_p]),
    "us_speaker_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "us_speaker_debug_conv": (C.c_int, [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_int, C.c_int, C.c_void_p]),
    "us_mel_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_mel_config)]),
    "us_mel_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "us_mel_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_mel_minmax": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "us_resample_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_resample_config)]),
    "us_resample_out_length": (C.c_int64, [C.c_void_p, C.c_int64]),
    "us_resample_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "us_hubert_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_hubert_config)]),
    "us_hubert_frames": (C.c_int, [C.c_void_p, C.c_int64]),
    "us_hubert_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_wavlm_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_wavlm_config)]),
    "us_wavlm_frames": (C.c_int, [C.c_void_p, C.c_int64]),
    "us_wavlm_position_bucket": (C.c_int, [C.c_void_p, C.c_int64]),
    "us_wavlm_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(us_whisper_config)]),
    "us_whisper_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int]),
    "us_whisper_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_decoder_logits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_size_t, C.c_void_p]),
    "us_whisper_generate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int, C.POINTER(us_whisper_decode_options),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_select_scratch_bytes": (C.c_size_t, [C.c_int]),
    "us_whisper_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(us_whisper_history), C.POINTER(us_whisper_decode_options), C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_beam_workspace_bytes": (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]),
    "us_whisper_decode_beam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int64), C.c_int,
                                         C.POINTER(us_whisper_decode_options), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_whisper_beam_select_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_whisper_beam_select": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(us_whisper_history), C.POINTER(C.c_double),
                                         C.POINTER(us_whisper_decode_options), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_units_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_units_pack_centers": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_units_workspace_bytes": (C.c_size_t, [C.c_int] * 5),
    "us_units_quantize": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_units_dedup": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                 C.c_void_p]),
    "us_units_process": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_units_encode": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t,
                                                                                         C.c_void_p]),
    "us_units_fit_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "us_units_fit_state_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_units_fit_state_clear": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]),
    "us_units_fit_accumulate": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    "us_units_fit_update": (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "us_units_fit_seed_step": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_double] + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "us_ctc_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_ctc_pack_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_ctc_logits": (C.c_int, [C.c_void_p] * 3 + [C.c_int] * 4 + [C.c_void_p] * 4),
    "us_ctc_collapse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "us_edit_distance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "us_ctc_loss_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "us_ctc_loss": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                              C.c_void_p]),
    "us_ctc_head_backward_workspace_bytes": (C.c_size_t, [C.c_int] * 4),
    "us_ctc_head_backward": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "us_ctc_align_workspace_bytes": (C.c_size_t, [C.c_int] * 3),
    "us_ctc_forced_align": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_int64] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]),
    "us_mos_packed_bytes": (C.c_size_t, [C.c_int] * 3),
    "us_mos_pack_head": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_mos_unpack_head": (C.c_int, [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5),
    "us_mos_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_mos_score": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p]),
    "us_level_chunk": (C.c_int, []),
    "us_level_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "us_level_measure": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "us_level_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_debug_block": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_size_t, C.c_void_p]),
    "us_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "us_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int]),
    "us_profile_read_f16": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "us_clip_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_float, C.c_void_p, C.c_void_p]),
    "us_last_error": (C.c_char_p, [C.c_void_p]),
}
# what the eight weight-table handles (csrc/handle.h) share; us_whisper_workspace_bytes takes the batch alone and stands above
for _p in ("frontend", "vocoder", "speaker", "mel", "resample", "hubert", "wavlm", "whisper"):
    SIGNATURES.update({
        f"us_{_p}_destroy": (C.c_int, [C.c_void_p]),
        f"us_{_p}_load_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
        f"us_{_p}_num_weights": (C.c_int, [C.c_void_p]),
        f"us_{_p}_weight_key": (C.c_char_p, [C.c_void_p, C.c_int]),
        f"us_{_p}_last_error": (C.c_char_p, [C.c_void_p]),
    })
    SIGNATURES.setdefault(f"us_{_p}_workspace_bytes", (C.c_size_t, [C.c_void_p, C.c_int, C.c_int]))

_lock = threading.Lock()
_lib = None


def load(build_if_missing: bool = True) -> C.CDLL:
    """dlopen the in-tree library, building it first when absent or older than any of its sources (a cheap mtime check; with
    no hipcc on the machine an existing library is used as it is)."""
    global _lib
    if _lib is not None:                 # every call of a plain function comes through here: no lock once the library is loaded
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = _build.LIB
        alt = os.environ.get("UNITSPEECH_AMD_LIB")          # experiments only: another build of the same ABI (A/B runs on one GPU box)
        if alt:
            if not os.path.exists(alt):
                raise RuntimeError(f"UNITSPEECH_AMD_LIB={alt} does not exist")
            path, build_if_missing = alt, False
        if build_if_missing:
            try:
                path = _build.build_library(force=os.environ.get("UNITSPEECH_AMD_REBUILD") == "1")
            except RuntimeError:
                if not os.path.exists(path) or _build.have_hipcc():
                    raise
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found and could not be built: the HIP decoder has no CPU fallback")
        lib = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)      # AttributeError here == missing export
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


def check(rc: int, handle=None, what: str = "") -> None:
    if rc == US_OK:
        return
    lib = load()
    msg = lib.us_last_error(handle)
    raise RuntimeError(f"libunitspeech_hip: {what} failed with {ERRORS.get(rc, rc)}: {msg.decode() if msg else ''}")
