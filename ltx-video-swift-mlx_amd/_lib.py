"""ctypes binding of libltxhip.so (include/ltxhip.h).

The shared library is the product; this module only declares its C ABI to Python so that tests, bench.py and the
host-side mirror of the reference's `LTXPipeline` can call it. There is deliberately no fallback: if the library
has not been built (``__graft_entry__.build()`` / ``make -C csrc``) importing this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LTX_LIB selects another build of the same ABI (tools/ and the `experiments`-marked tests use csrc/build_exp/libltxhip_exp.so)
SO_PATH = os.environ.get("LTX_LIB") or os.path.join(_HERE, "csrc", "build", "libltxhip.so")


class LTXError(RuntimeError):
    """Mirror of the reference's ``LTXError`` cases (LTXVideo.swift:66-141) keyed by C status code."""

    NAMES = {
        1: "modelNotLoaded", 2: "invalidConfiguration", 3: "insufficientMemory", 4: "weightLoadingFailed",
        5: "generationFailed", 6: "generationCancelled", 7: "invalidFrameCount", 8: "invalidDimensions",
        9: "fileNotFound", 10: "invalidLoRA", 11: "hipError",
    }

    def __init__(self, code, message):
        self.code = int(code)
        self.case = self.NAMES.get(self.code, "unknown")
        super().__init__(f"LTXError.{self.case}: {message}")


class DenoiseOptions(C.Structure):
    """``ltx_denoise_options``: the sampling knobs of ``LTXVideoGenerationConfig`` (LTXConfig.swift:216-300)."""

    _fields_ = [("struct_size", C.c_uint32), ("cfg_scale", C.c_float), ("guidance_rescale", C.c_float), ("stg_scale", C.c_float),
                ("stg_blocks", C.POINTER(C.c_int)), ("n_stg_blocks", C.c_int), ("ge_gamma", C.c_float),
                ("cond_latent", C.c_void_p), ("image_cond_noise_scale", C.c_float), ("cond_noise", C.c_void_p),
                ("shard", C.c_int), ("step_stats", C.c_void_p)]


PROGRESS_CB = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_float, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long)  # ltx_allgather_fn
SHARD_NONE, SHARD_CFG, SHARD_SEQUENCE = 0, 1, 2
DIST_ID_BYTES = 128


class ConnectorConfig(C.Structure):
    """``ltx_connector_config`` / reference ``VideoGemmaTextEncoderModel`` defaults (LTXTextEncoder.swift:18-45)."""

    _fields_ = [("dim", C.c_int), ("heads", C.c_int), ("layers", C.c_int), ("registers", C.c_int), ("states", C.c_int),
                ("theta", C.c_float), ("max_pos", C.c_int)]


class VaeModsJob(C.Structure):
    """``ltx_vae_mods_job``: one modulation table of ``ltx_op_vae_make_mods_batch``."""

    _fields_ = [("table", C.c_void_p), ("te", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int), ("C", C.c_int)]


class GemmaConfig(C.Structure):
    """``ltx_gemma_config`` / reference ``Gemma3Config`` defaults (Gemma3Config.swift:42-60)."""

    _fields_ = [("hidden_size", C.c_int), ("num_hidden_layers", C.c_int), ("intermediate_size", C.c_int), ("num_attention_heads", C.c_int),
                ("head_dim", C.c_int), ("num_key_value_heads", C.c_int), ("vocab_size", C.c_int), ("rms_norm_eps", C.c_float),
                ("rope_theta", C.c_float), ("rope_local_base_freq", C.c_float), ("query_pre_attn_scalar", C.c_float),
                ("sliding_window", C.c_int), ("sliding_window_pattern", C.c_int)]


class LmParams(C.Structure):
    """``ltx_lm_params``: the generate loop's settings; ``ltx_lm_params_default`` fills the reference's (Gemma3Model.swift:390-398)."""

    _fields_ = [("struct_size", C.c_uint32), ("max_new_tokens", C.c_int), ("temperature", C.c_float), ("top_p", C.c_float),
                ("repetition_penalty", C.c_float), ("repetition_context", C.c_int), ("seed", C.c_uint64), ("n_eos", C.c_int),
                ("eos_ids", C.c_int32 * 8)]


class TransformerConfig(C.Structure):
    """``ltx_transformer_config`` / reference ``LTXTransformerConfig`` (LTXConfig.swift:83-177)."""

    _fields_ = [
        ("num_layers", C.c_int), ("num_attention_heads", C.c_int), ("attention_head_dim", C.c_int),
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("cross_attention_dim", C.c_int),
        ("caption_channels", C.c_int), ("rope_theta", C.c_float), ("max_pos", C.c_int * 3),
        ("timestep_scale_multiplier", C.c_float), ("norm_eps", C.c_float),
    ]


class DualBlockConfig(C.Structure):
    """``ltx_dual_block_config``: the dual video + audio block stack (LTX2TransformerBlock.swift:98-170, LTXConfig.swift:83-177)."""

    _fields_ = [("num_layers", C.c_int), ("video_heads", C.c_int), ("video_dim", C.c_int), ("audio_heads", C.c_int), ("audio_dim", C.c_int),
                ("video_context_dim", C.c_int), ("audio_context_dim", C.c_int), ("rope_theta", C.c_float), ("max_pos", C.c_int * 3),
                ("audio_max_pos", C.c_int), ("fps", C.c_float), ("norm_eps", C.c_float)]


class DualForwardArgs(C.Structure):
    """``ltx_dual_forward_args``: what LTX2Transformer.callAsFunction hands its blocks (LTX2TransformerBlock.swift:174-177)."""

    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int), ("F", C.c_int), ("H", C.c_int), ("W", C.c_int), ("T_a", C.c_int), ("S", C.c_int),
                ("x_video", C.c_void_p), ("x_audio", C.c_void_p), ("context_video", C.c_void_p), ("context_audio", C.c_void_p),
                ("key_bias_video", C.c_void_p), ("key_bias_audio", C.c_void_p), ("temb_video", C.c_void_p), ("temb_audio", C.c_void_p),
                ("cross_video_ss", C.c_void_p), ("cross_audio_ss", C.c_void_p), ("phase_mask", C.c_uint32), ("n_groups", C.c_int),
                ("video_row_map", C.c_void_p)]


class GemvJob(C.Structure):
    """``ltx_gemv_job``: one job of ``ltx_op_gemv_group`` (the operands of ``ltx_op_gemv_f32`` without M)."""

    _fields_ = [("a", C.c_void_p), ("lda", C.c_long), ("W", C.c_void_p), ("ldw", C.c_long), ("bias", C.c_void_p), ("out", C.c_void_p),
                ("ldo", C.c_long), ("N", C.c_int), ("K", C.c_int), ("in_act", C.c_int)]


class GemvJobQ(C.Structure):
    """``ltx_gemv_job_q``: one job of ``ltx_op_gemv_group_q`` (``ltx_gemv_job`` with W as affine-quantised codes, group 64 along K)."""

    _fields_ = [("a", C.c_void_p), ("lda", C.c_long), ("codes", C.c_void_p), ("scales", C.c_void_p), ("biases", C.c_void_p),
                ("bias", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_long), ("N", C.c_int), ("K", C.c_int), ("in_act", C.c_int)]


class GemmTileLaunch(C.Structure):
    """``ltx_gemm_tile_launch``: one launch of the 192 x 256 / 384 x 256 GEMM kernel with any epilogue it has (``ltx_op_gemm_tile``)."""

    _fields_ = [("struct_size", C.c_uint32), ("tile_cfg", C.c_int), ("A", C.c_void_p), ("lda", C.c_long), ("B", C.c_void_p), ("ldb", C.c_long),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("split_k", C.c_int), ("split_bf16", C.c_int), ("act", C.c_int),
                ("round_bf16", C.c_int), ("resid", C.c_int), ("bias_n", C.c_void_p), ("bias_m", C.c_void_p), ("out_f32", C.c_void_p),
                ("ld_f32", C.c_long), ("out_bf16", C.c_void_p), ("ld_bf16", C.c_long), ("resid_src", C.c_void_p), ("ld_resid", C.c_long),
                ("gate", C.c_void_p), ("gate_bstride", C.c_long), ("gate_rowmap", C.c_void_p), ("rows_per_batch", C.c_int),
                ("gate_scalar", C.c_float)]


class DualModelConfig(C.Structure):
    """``ltx_dual_model_config``: the block config plus the top-level widths of LTX2Transformer (LTXConfig.swift:83-177)."""

    _fields_ = [("blocks", DualBlockConfig), ("in_channels", C.c_int), ("out_channels", C.c_int), ("audio_in_channels", C.c_int),
                ("audio_out_channels", C.c_int), ("caption_channels", C.c_int), ("timestep_scale_multiplier", C.c_float)]


class DualModelForwardArgs(C.Structure):
    """``ltx_dual_model_forward_args``: the arguments of LTX2Transformer.callAsFunction (LTX2Transformer.swift:254-265)."""

    _fields_ = [("struct_size", C.c_uint32), ("B", C.c_int), ("F", C.c_int), ("H", C.c_int), ("W", C.c_int), ("T_a", C.c_int), ("S", C.c_int),
                ("video_latent", C.c_void_p), ("audio_latent", C.c_void_p), ("video_context", C.c_void_p), ("audio_context", C.c_void_p),
                ("video_timesteps", C.c_void_p), ("audio_timesteps", C.c_void_p), ("video_mask", C.c_void_p), ("audio_mask", C.c_void_p),
                ("video_velocity", C.c_void_p), ("audio_velocity", C.c_void_p), ("ungrouped", C.c_int), ("text_cache", C.c_int)]


class NormMod2Job(C.Structure):
    """``ltx_norm_mod2_job``: one job of ``ltx_op_norm_mod2``."""

    _fields_ = [("x", C.c_void_p), ("ldx", C.c_long), ("scale0", C.c_void_p), ("shift0", C.c_void_p), ("scale1", C.c_void_p),
                ("shift1", C.c_void_p), ("mod_bstride", C.c_long), ("rows_per_batch", C.c_int), ("out0", C.c_void_p), ("out1", C.c_void_p),
                ("ldo", C.c_long), ("rows", C.c_int), ("D", C.c_int), ("row_map", C.c_void_p)]


class DualStepJob(C.Structure):
    """``ltx_dual_step_job``: one job of ``ltx_op_dual_step``."""

    _fields_ = [("latent", C.c_void_p), ("v_cond", C.c_void_p), ("v_uncond", C.c_void_p), ("cfg_scale", C.c_float), ("form", C.c_int),
                ("tokens", C.c_void_p), ("copies", C.c_int), ("v_out", C.c_void_p), ("n", C.c_long), ("n_keep", C.c_long),
                ("keep_src", C.c_void_p), ("keep_noise", C.c_void_p), ("keep_scale", C.c_float)]


class DualDenoiseArgs(C.Structure):
    """``ltx_dual_denoise_args``: the joint video + audio loop of generateVideoWithAudio (LTXPipeline.swift:1276-1417)."""

    _fields_ = [("struct_size", C.c_uint32), ("F", C.c_int), ("H", C.c_int), ("W", C.c_int), ("T_a", C.c_int), ("S", C.c_int),
                ("video_latent", C.c_void_p), ("audio_latent", C.c_void_p), ("sigmas", C.POINTER(C.c_float)), ("n_sigmas", C.c_int),
                ("video_context", C.c_void_p), ("audio_context", C.c_void_p), ("mask", C.c_void_p), ("cfg_scale", C.c_float),
                ("guidance_rescale", C.c_float), ("text_cache", C.c_int), ("step_stats", C.c_void_p), ("cond_latent", C.c_void_p),
                ("image_cond_noise_scale", C.c_float), ("cond_noise", C.c_void_p)]


class DualRestageJob(C.Structure):
    """``ltx_dual_restage_job``: one job of ``ltx_op_dual_restage``."""

    _fields_ = [("x", C.c_void_p), ("latent", C.c_void_p), ("tokens", C.c_void_p), ("C", C.c_int), ("T", C.c_long), ("noise", C.c_void_p),
                ("noise_scale", C.c_float), ("renoise", C.c_int), ("stats", C.c_void_p), ("stats_ref", C.c_void_p), ("ref", C.c_void_p),
                ("T_ref", C.c_long), ("stats_out", C.c_void_p), ("HW", C.c_long), ("cond", C.c_void_p), ("cond_noise", C.c_void_p),
                ("cond_scale", C.c_float), ("cond_sigma2", C.c_float)]


class DualTwoStageArgs(C.Structure):
    """``ltx_dual_two_stage_args``: the two loops of generateVideoWithAudioTwoStage and the bridge between them (LTXPipeline.swift:1613-1817)."""

    _fields_ = [("struct_size", C.c_uint32), ("F", C.c_int), ("H", C.c_int), ("W", C.c_int), ("T_a", C.c_int), ("S", C.c_int),
                ("video_latent_in", C.c_void_p), ("video_latent_out", C.c_void_p), ("audio_latent", C.c_void_p),
                ("sigmas1", C.POINTER(C.c_float)), ("n_sigmas1", C.c_int), ("sigmas2", C.POINTER(C.c_float)), ("n_sigmas2", C.c_int),
                ("video_noise2", C.c_void_p), ("audio_noise2", C.c_void_p), ("video_context", C.c_void_p), ("audio_context", C.c_void_p),
                ("mask", C.c_void_p), ("stage1_out", C.c_void_p), ("cond_latent1", C.c_void_p), ("cond_latent2", C.c_void_p),
                ("image_cond_noise_scale", C.c_float), ("cond_noise1", C.c_void_p), ("cond_noise2", C.c_void_p)]


class NoiseJob(C.Structure):
    """``ltx_noise_job``: one draw of ``ltx_op_mlx_normal_group``."""

    _fields_ = [("key", C.c_uint32 * 2), ("dst", C.c_void_p), ("n", C.c_long), ("scale", C.c_float), ("raw_bits", C.c_int)]


class NoiseDraw(C.Structure):
    """``ltx_noise_draw``: one draw of a generation's plan (``ltx_dual_noise_plan``)."""

    _fields_ = [("draw_index", C.c_int), ("role", C.c_int), ("step", C.c_int), ("numel", C.c_long), ("offset", C.c_long), ("scale", C.c_float)]


class DualGenerateArgs(C.Structure):
    """``ltx_dual_generate_args``: generateVideoWithAudio(TwoStage) from a seed to the final latents (LTXPipeline.swift:1222-1417, :1570-1817)."""

    _fields_ = [("struct_size", C.c_uint32), ("two_stage", C.c_int), ("seed", C.c_uint64), ("channels", C.c_int), ("F", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("T_a", C.c_int), ("S", C.c_int), ("video_latent", C.c_void_p), ("audio_latent", C.c_void_p),
                ("sigmas1", C.POINTER(C.c_float)), ("n_sigmas1", C.c_int), ("sigmas2", C.POINTER(C.c_float)), ("n_sigmas2", C.c_int),
                ("video_context", C.c_void_p), ("audio_context", C.c_void_p), ("mask", C.c_void_p), ("cfg_scale", C.c_float),
                ("guidance_rescale", C.c_float), ("cond_latent1", C.c_void_p), ("cond_latent2", C.c_void_p), ("image_cond_noise_scale", C.c_float),
                ("noise_workspace", C.c_void_p), ("stage1_out", C.c_void_p)]


NOISE_VIDEO1, NOISE_AUDIO1, NOISE_COND1, NOISE_VIDEO2, NOISE_AUDIO2, NOISE_COND2 = range(6)


def _load():
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"libltxhip.so not found at {SO_PATH}; build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the HIP path)")
    return C.CDLL(SO_PATH, mode=C.RTLD_GLOBAL)


lib = _load()

_vp, _i, _f, _l, _u64 = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_uint64
_ip = C.POINTER(C.c_int)

# name -> (restype, argtypes); every symbol declared in include/ltxhip.h must appear here (tests check both ways)
SIGNATURES = {
    "ltx_version": (C.c_char_p, []),
    "ltx_abi_version": (_i, []),
    "ltx_ctx_set_option": (_i, [_vp, C.c_char_p, _i]),
    "ltx_ctx_get_option": (_i, [_vp, C.c_char_p, C.POINTER(C.c_int)]),
    "ltx_option_info": (_i, [_i, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                             C.POINTER(C.c_char_p)]),
    "ltx_build_info": (C.c_char_p, []),
    "ltx_transformer_config_default": (None, [C.POINTER(TransformerConfig)]),
    "ltx_ctx_create": (_i, [_i, C.POINTER(_vp)]),
    "ltx_ctx_destroy": (None, [_vp]),
    "ltx_last_error": (C.c_char_p, [_vp]),
    "ltx_ctx_set_stream": (_i, [_vp, _vp]),
    "ltx_ctx_synchronize": (_i, [_vp]),
    "ltx_load_report": (_i, [_vp, _ip, _ip, _ip]),
    "ltx_validate_generation_config": (_i, [_i, _i, _i, _i, _f, _i, C.c_char_p, _i]),
    "ltx_latent_shape": (_i, [_i, _i, _i, _ip, _ip, _ip]),
    "ltx_sigmas": (_i, [_i, _i, _i, C.POINTER(C.c_float), _i]),
    "ltx_stage2_sigmas": (_i, [C.POINTER(C.c_float), _i]),
    "ltx_rope_tables": (_i, [C.POINTER(TransformerConfig), _i, _i, _i, _vp, _vp]),
    "ltx_vae_tile_plan": (_i, [_i, _i, _i, _ip, _ip, _i, _ip]),
    "ltx_map_transformer_key": (_i, [C.c_char_p, C.c_char_p, _i]),
    "ltx_map_vae_key": (_i, [C.c_char_p, C.c_char_p, _i]),
    "ltx_map_lora_key": (_i, [C.c_char_p, C.c_char_p, _i]),
    "ltx_st_info": (_i, [C.c_char_p, C.c_char_p, C.POINTER(C.c_long)]),
    "ltx_st_read": (_l, [C.c_char_p, C.c_char_p, _i, _vp, _l]),
    "ltx_dit_load": (_i, [_vp, C.c_char_p, C.POINTER(TransformerConfig), _i, _i]),
    "ltx_dit_init_synthetic": (_i, [_vp, C.POINTER(TransformerConfig), _u64]),
    "ltx_dit_unload": (_i, [_vp]),
    "ltx_dit_quantize": (_i, [_vp, _i, _i]),
    "ltx_dit_fuse_lora": (_i, [_vp, C.c_char_p, _f, _ip]),
    "ltx_dit_export_param": (_l, [_vp, C.c_char_p, _vp, _l]),
    "ltx_dist_unique_id": (_i, [_vp]),
    "ltx_dist_init": (_i, [_vp, _i, _i, _vp]),
    "ltx_dist_set_transport": (_i, [_vp, _i, _i, _vp, _vp]),
    "ltx_dist_shutdown": (_i, [_vp]),
    "ltx_dist_info": (_i, [_vp, _ip, _ip, _ip, C.POINTER(C.c_long)]),
    "ltx_dist_allgather_dev": (_i, [_vp, _vp, _vp, _l]),
    "ltx_dist_broadcast_dev": (_i, [_vp, _vp, _l, _i]),
    "ltx_vae_decode_tile_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _i, _vp, _l, _ip]),
    "ltx_dit_memory_info": (_i, [_vp, C.POINTER(_l), C.POINTER(_l), C.POINTER(_l), C.POINTER(_l)]),
    "ltx_op_gemm_q8": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _l]),
    "ltx_vae_res_block_dev": (_i, [_vp, _i, _i, _vp, _i, _i, _i]),
    "ltx_vae_upsample_dev": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "ltx_vae_blend_tiles_dev": (_i, [_vp, C.POINTER(_vp), _ip, _i, _i, _i, _i, _vp, _l, _ip]),
    "ltx_vae_decode_sharded_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _vp, _l, _ip]),
    "ltx_vae_decode_gathered_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _i, _vp, _l, _ip]),
    "ltx_dit_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "ltx_dit_forward_tokens": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "ltx_dit_forward_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _u64, _vp]),
    "ltx_dit_forward_sp_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _u64, _i, _i, _vp, _vp, _vp]),
    "ltx_dit_set_cross_attn_scale": (_i, [_vp, _f, _i, _i]),
    "ltx_dit_set_stg": (_i, [_vp, _ip, _i, _i, _i]),
    "ltx_dit_clear_stg": (_i, [_vp]),
    "ltx_vae_load": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "ltx_vae_init_synthetic": (_i, [_vp, _u64, _i]),
    "ltx_vae_unload": (_i, [_vp]),
    "ltx_vae_timestep_conditioning": (_i, [_vp]),
    "ltx_vae_decode": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _vp, _l, _ip]),
    "ltx_vae_decode_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp, _i, _i, _vp, _l, _ip]),
    "ltx_op_conv3d": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "ltx_connector_config_default": (None, [C.POINTER(ConnectorConfig)]),
    "ltx_connector_load": (_i, [_vp, C.c_char_p, C.POINTER(ConnectorConfig)]),
    "ltx_connector_init_synthetic": (_i, [_vp, C.POINTER(ConnectorConfig), C.c_ulong]),
    "ltx_connector_unload": (_i, [_vp]),
    "ltx_connector_encode_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ltx_connector_encode": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "ltx_connector_encode_taps_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "ltx_map_text_encoder_key": (_i, [C.c_char_p, C.c_char_p, _i]),
    "ltx_rope_tables_1d": (_i, [_i, _i, _f, _i, _vp, _vp]),
    "ltx_vae_encoder_load": (_i, [_vp, C.c_char_p, _i]),
    "ltx_vae_encoder_init_synthetic": (_i, [_vp, _i, C.c_ulong]),
    "ltx_vae_encoder_unload": (_i, [_vp]),
    "ltx_vae_encode": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ltx_vae_encode_dev": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ltx_vae_encoder_latent_frames": (_i, [_i]),
    "ltx_map_vae_encoder_key": (_i, [C.c_char_p, C.c_char_p, _i]),
    "ltx_frames_to_u8": (_i, [_vp, _l, _vp]),
    "ltx_mlx_random_normal": (_i, [_u64, _i, _vp, _l]),
    "ltx_threefry2x32": (None, [_vp, _vp, _vp]),
    "ltx_mlx_draw_key": (_i, [_u64, _i, C.POINTER(C.c_uint32)]),
    "ltx_op_mlx_normal_group": (_i, [_vp, C.POINTER(NoiseJob), _i]),
    "ltx_mlx_random_normal_dev": (_i, [_vp, _u64, _i, _vp, _l, _f]),
    "ltx_dual_noise_plan": (_i, [C.POINTER(DualGenerateArgs), C.POINTER(NoiseDraw), _i, C.POINTER(_l)]),
    "ltx_dual_generate_dev": (_i, [_vp, C.POINTER(DualGenerateArgs), PROGRESS_CB, _vp]),
    "ltx_dual_generate": (_i, [_vp, C.POINTER(DualGenerateArgs), PROGRESS_CB, _vp]),
    "ltx_connector_encode_av_dev": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ltx_connector_encode_av": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "ltx_connector_has_audio": (_i, [_vp]),
    "ltx_text_av_encode_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ltx_text_av_encode": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "ltx_write_png": (_i, [C.c_char_p, _vp, _i, _i]),
    "ltx_upscaler_load": (_i, [_vp, C.c_char_p]),
    "ltx_upscaler_unload": (_i, [_vp]),
    "ltx_upscale_latent": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ltx_upscale_latent_dev": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ltx_adain_filter_latent": (_i, [_vp, _vp, _l, _vp, _l, _i, _f]),
    "ltx_adain_filter_latent_dev": (_i, [_vp, _vp, _l, _vp, _l, _i, _f]),
    "ltx_renoise_dev": (_i, [_vp, _vp, _vp, _f, _l]),
    "ltx_denoise": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_float), _i, _vp, _vp, _i, C.POINTER(DenoiseOptions), PROGRESS_CB, _vp]),
    "ltx_denoise_dev": (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_float), _i, _vp, _vp, _i, _i, _u64, C.POINTER(DenoiseOptions), PROGRESS_CB, _vp]),
    "ltx_prof_enable": (_i, [_vp, _i]),
    "ltx_prof_collect": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_double), _i]),
    "ltx_op_gemm_bf16": (_i, [_vp, _vp, _l, _vp, _l, _vp, _i, _i, _i, _i, _i, _vp, _l, _vp, _l]),
    "ltx_op_value_projection_t": (_i, [_vp, _vp, _l, _i, _vp, _vp, _i, _i, _vp, _l]),
    "ltx_op_qkv_projection": (_i, [_vp, _vp, _l, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _l, _vp, _l, _i]),
    "ltx_op_gemm_bf16_gated_residual": (_i, [_vp, _vp, _l, _vp, _l, _vp, _vp, _f, _i, _i, _i, _vp, _l, _vp, _l]),
    "ltx_op_gemm_bf16_gated_residual_norm": (_i, [_vp, _vp, _l, _vp, _l, _vp, _vp, _f, _i, _i, _i, _vp, _l, _vp, _vp, _f, _vp, _l, _i]),
    "ltx_op_gemv_f32": (_i, [_vp, _vp, _l, _vp, _l, _vp, _vp, _l, _i, _i, _i, _i]),
    "ltx_op_attention": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _f, _vp]),
    "ltx_attention_key_splits": (_i, [_i, _i, _i, _i]),
    "ltx_op_norm_mod": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "ltx_op_qknorm_rope": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "ltx_op_norm_mod_ex": (_i, [_vp, _vp, _l, _vp, _vp, _l, _i, _vp, _i, _i, _i, _f, _i, _vp, _l]),
    "ltx_op_qknorm_rope_pair": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _l, _l, _vp, _vp, _i, _i, _i, _f, _f, _i]),
    "ltx_conv_takes_d2s_pn": (_i, [_i, _i, _i, _i]),
    "ltx_gemm_dense_tile_cfg": (_i, [_i, _i, _i, _i, _i, _i]),
    "ltx_audio_vae_load": (_i, [_vp, C.c_char_p]),
    "ltx_audio_vae_init_synthetic": (_i, [_vp, _i, _u64]),
    "ltx_audio_vae_unload": (_i, [_vp]),
    "ltx_vocoder_load": (_i, [_vp, C.c_char_p]),
    "ltx_vocoder_init_synthetic": (_i, [_vp, _i, _u64]),
    "ltx_vocoder_unload": (_i, [_vp]),
    "ltx_audio_vae_decode": (_i, [_vp, _vp, _i, _vp]),
    "ltx_audio_vae_decode_dev": (_i, [_vp, _vp, _i, _vp]),
    "ltx_vocoder_forward": (_i, [_vp, _vp, _i, _vp]),
    "ltx_vocoder_forward_dev": (_i, [_vp, _vp, _i, _vp]),
    "ltx_audio_decode": (_i, [_vp, _vp, _i, _vp]),
    "ltx_audio_decode_dev": (_i, [_vp, _vp, _i, _vp]),
    "ltx_audio_latent_frames": (_i, [_i, _f]),
    "ltx_audio_mel_frames": (_i, [_i]),
    "ltx_audio_sample_count": (_l, [_i]),
    "ltx_audio_sample_rate": (_i, []),
    "ltx_write_wav": (_i, [C.c_char_p, _vp, _l, _i, _f]),
    "ltx_audio_positions": (_i, [_i, _vp]),
    "ltx_video_temporal_positions": (_i, [_i, _i, _i, _f, _vp]),
    "ltx_rope_tables_positions": (_i, [_vp, _i, _i, _f, _i, _vp, _vp]),
    "ltx_attn_module_init_synthetic": (_i, [_vp, _i, _i, _i, _i, _u64]),
    "ltx_attn_module_load": (_i, [_vp, _i, C.c_char_p, C.c_char_p, _i]),
    "ltx_attn_module_unload": (_i, [_vp, _i]),
    "ltx_attn_module_export_param": (_l, [_vp, _i, C.c_char_p, _vp, _l]),
    "ltx_attn_module_forward_dev": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp]),
    "ltx_dual_block_config_default": (None, [C.POINTER(DualBlockConfig)]),
    "ltx_dual_blocks_init_synthetic": (_i, [_vp, C.POINTER(DualBlockConfig), _u64]),
    "ltx_dual_blocks_load": (_i, [_vp, C.c_char_p, C.POINTER(DualBlockConfig), _i, _i]),
    "ltx_dual_blocks_unload": (_i, [_vp]),
    "ltx_dual_blocks_export_param": (_l, [_vp, C.c_char_p, _vp, _l]),
    "ltx_dual_blocks_forward_dev": (_i, [_vp, C.POINTER(DualForwardArgs)]),
    "ltx_op_norm_mod2": (_i, [_vp, C.POINTER(NormMod2Job), C.POINTER(NormMod2Job), _f]),
    "ltx_op_gemv_group": (_i, [_vp, C.POINTER(GemvJob), _i, _i]),
    "ltx_op_gemv_group_q": (_i, [_vp, C.POINTER(GemvJobQ), _i, _i, _i]),
    "ltx_op_gemm_tile": (_i, [_vp, C.POINTER(GemmTileLaunch)]),
    "ltx_dual_model_config_default": (None, [C.POINTER(DualModelConfig)]),
    "ltx_dual_model_init_synthetic": (_i, [_vp, C.POINTER(DualModelConfig), _u64]),
    "ltx_dual_model_load": (_i, [_vp, C.c_char_p, C.POINTER(DualModelConfig)]),
    "ltx_dual_model_unload": (_i, [_vp]),
    "ltx_dual_model_export_param": (_l, [_vp, C.c_char_p, _vp, _l]),
    "ltx_dual_model_quantize": (_i, [_vp, _i, _i]),
    "ltx_dual_model_memory_info": (_i, [_vp, C.POINTER(_l), C.POINTER(_l), C.POINTER(_l), C.POINTER(_l)]),
    "ltx_dual_model_forward_dev": (_i, [_vp, C.POINTER(DualModelForwardArgs)]),
    "ltx_dual_model_forward_groups_dev": (_i, [_vp, C.POINTER(DualModelForwardArgs), _i, _vp]),
    "ltx_dual_model_embed_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ltx_dual_model_prepare_text_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i]),
    "ltx_dual_model_text_cache_info": (_i, [_vp, _ip, _ip, C.POINTER(_l), C.POINTER(_l)]),
    "ltx_op_dual_step": (_i, [_vp, C.POINTER(DualStepJob), C.POINTER(DualStepJob), _f, _f]),
    "ltx_dual_denoise_dev": (_i, [_vp, C.POINTER(DualDenoiseArgs), PROGRESS_CB, _vp]),
    "ltx_dual_denoise": (_i, [_vp, C.POINTER(DualDenoiseArgs), PROGRESS_CB, _vp]),
    "ltx_op_dual_restage": (_i, [_vp, C.POINTER(DualRestageJob), C.POINTER(DualRestageJob)]),
    "ltx_dual_two_stage_dev": (_i, [_vp, C.POINTER(DualTwoStageArgs), PROGRESS_CB, _vp]),
    "ltx_dual_two_stage": (_i, [_vp, C.POINTER(DualTwoStageArgs), PROGRESS_CB, _vp]),
    "ltx_op_attention_hd": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "ltx_attention_hd_workgroup_queries": (_i, [_i, _i, _i, _i]),
    "ltx_op_qknorm_rope_hd": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _vp]),
    "ltx_op_conv1d": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _i, _f, _vp]),
    "ltx_op_conv_transpose1d": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _f, _vp]),
    "ltx_op_conv2d_causal": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _i, _vp, _i, _vp, _vp]),
    "ltx_gemma_config_default": (None, [C.POINTER(GemmaConfig)]),
    "ltx_gemma_load": (_i, [_vp, C.POINTER(C.c_char_p), _i, C.POINTER(GemmaConfig)]),
    "ltx_gemma_init_synthetic": (_i, [_vp, C.POINTER(GemmaConfig), C.c_ulong]),
    "ltx_gemma_unload": (_i, [_vp]),
    "ltx_gemma_memory_info": (_i, [_vp, C.POINTER(_l), C.POINTER(_l)]),
    "ltx_gemma_encode_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "ltx_gemma_encode": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "ltx_text_encode_dev": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ltx_text_encode": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "ltx_op_attention_causal": (_i, [_vp, _vp, _vp, _vp, _l, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "ltx_op_attention_causal_ld": (_i, [_vp, _vp, _l, _l, _vp, _l, _l, _vp, _l, _l, _vp, _i, _i, _i, _i, _i, _f, _vp, _l, _l]),
    "ltx_op_gemma_norm": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp]),
    "ltx_op_gemma_qknorm_rope": (_i, [_vp, _vp, _l, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _f]),
    "ltx_op_gemma_rope_tables": (_i, [_vp, _i, _f, _vp, _vp]),
    "ltx_op_geglu": (_i, [_vp, _vp, _i, _i, _vp]),
    "ltx_op_gemma_embed": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp]),
    "ltx_lm_params_default": (None, [C.POINTER(LmParams)]),
    "ltx_lm_begin": (_i, [_vp, _i]),
    "ltx_lm_end": (_i, [_vp, C.POINTER(_l)]),
    "ltx_lm_memory_info": (_i, [_vp, C.POINTER(_l), C.POINTER(_l)]),
    "ltx_lm_prefill_dev": (_i, [_vp, _vp, _i, _vp]),
    "ltx_lm_prefill": (_i, [_vp, _vp, _i, _vp]),
    "ltx_lm_step_dev": (_i, [_vp, _vp, _vp]),
    "ltx_lm_step": (_i, [_vp, C.c_int32, _vp]),
    "ltx_lm_last_state": (_i, [_vp, _vp]),
    "ltx_lm_cache_k": (_i, [_vp, _i, _i, _vp]),
    "ltx_lm_cache_vt": (_i, [_vp, _i, _i, _vp]),
    "ltx_lm_generate": (_i, [_vp, _vp, _i, C.POINTER(LmParams), _vp, C.POINTER(C.c_int)]),
    "ltx_lm_sample_host": (_i, [_vp, _i, _vp, _i, _i, _f, _f, _f, _u64, _i, C.POINTER(C.c_int32)]),
    "ltx_op_gemv_bf16": (_i, [_vp, _vp, _vp, _l, _i, _i, _i, _i, _vp, _l, _vp]),
    "ltx_gemv_bf16_rows_per_workgroup": (_i, [_i, _i]),
    "ltx_op_attention_decode": (_i, [_vp, _vp, _vp, _l, _vp, _l, _i, _i, _i, _f, _vp]),
    "ltx_op_lm_pick": (_i, [_vp, _vp, _i, _vp, _i, _i, _f, _vp]),
    "ltx_op_mean_var": (_i, [_vp, _vp, _l, _i, _vp]),
    "ltx_op_guidance_rescale": (_i, [_vp, _vp, _vp, _vp, _f, _l, _i]),
    "ltx_op_adain": (_i, [_vp, _vp, _vp, _vp, _f, _l, _i]),
    "ltx_op_groupnorm_stats": (_i, [_vp, _vp, _l, _i, _i, _f, _vp]),
    "ltx_op_groupnorm_apply": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _l, _i, _i]),
    "ltx_op_pixelnorm_silu": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i]),
    "ltx_op_vae_prepare": (_i, [_vp, _vp, _l, _vp, _f, _vp, _vp, _vp, _i, _l]),
    "ltx_op_upscaler_finish": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i]),
    "ltx_op_blend_frames": (_i, [_vp, _vp, _vp, _i, _l]),
    "ltx_op_patchify_bf16": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "ltx_op_unpatchify_f32": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "ltx_op_euler_step": (_i, [_vp, _vp, _vp, _f, _f, _l, _i, _i]),
    "ltx_op_set_frame0": (_i, [_vp, _vp, _vp, _vp, _f, _f, _i, _i, _i]),
    "ltx_op_make_mod": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i]),
    "ltx_fe_stats_partials_floats": (_l, [_i, _i, _i, _i]),
    "ltx_op_fe_stats": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "ltx_op_fe_norm_concat": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "ltx_op_cfg_combine": (_i, [_vp, _vp, _vp, _f, _vp, _l]),
    "ltx_op_lincomb": (_i, [_vp, _vp, _vp, _f, _f, _vp, _l]),
    "ltx_op_axpby": (_i, [_vp, _vp, _vp, _f, _f, _vp, _l]),
    "ltx_op_ge": (_i, [_vp, _vp, _vp, _f, _vp, _l]),
    "ltx_op_scale_inplace": (_i, [_vp, _vp, _f, _l]),
    "ltx_op_clip01": (_i, [_vp, _vp, _l]),
    "ltx_op_mask_to_bias": (_i, [_vp, _vp, _vp, _l]),
    "ltx_op_cast_f32_bf16": (_i, [_vp, _vp, _vp, _l]),
    "ltx_op_cast_bf16_f32": (_i, [_vp, _vp, _vp, _l]),
    "ltx_op_timestep_embedding": (_i, [_vp, _vp, _f, _vp, _i, _i]),
    "ltx_vae_mods_max_jobs": (_i, []),
    "ltx_op_vae_make_mods_batch": (_i, [_vp, C.POINTER(VaeModsJob), _i]),
    "ltx_op_sp_vt_interleave": (_i, [_vp, _vp, _vp, _i, _i, _i, _l]),
    "ltx_op_register_plan": (_i, [_vp, _vp, _i, _i, _vp]),
    "ltx_op_register_gather": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ltx_op_enc_patchify": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "ltx_op_enc_s2d_residual": (_i, [_vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "ltx_op_enc_finish": (_i, [_vp, _vp, _l, _vp, _vp, _vp, _i, _l]),
    "ltx_op_i2v_rowmap": (_i, [_vp, _vp, _i, _i, _i, _i]),
    "ltx_op_i2v_timesteps": (_i, [_vp, _vp, _i, _i, _f]),
    "ltx_op_fill_const_i32": (_i, [_vp, _vp, _l, _i]),
    "ltx_op_gemma_mask_scan": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "ltx_op_audio_pn_pad": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "ltx_op_audio_upsample_pad": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "ltx_op_audio_denorm_pad": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "ltx_op_audio_mel_pack": (_i, [_vp, _vp, _i, _i, _vp]),
    "ltx_op_audio_mean3_act": (_i, [_vp, _vp, _vp, _vp, _l, _i, _f, _vp, _l]),
    "ltx_op_fill_normal_bf16": (_i, [_vp, _vp, _l, _u64, _f, _f]),
    "ltx_op_fill_normal_f32": (_i, [_vp, _vp, _l, _u64, _f, _f]),
}

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)  # AttributeError here = header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args

HAS_EXPERIMENTS = b"experiments=1" in lib.ltx_build_info()
