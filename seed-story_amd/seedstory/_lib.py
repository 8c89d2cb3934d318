"""ctypes binding of ``libseedstory_hip.so`` (the C ABI declared in ``include/seedstory_hip.h``).

There is deliberately NO fallback: if the shared library is missing or a call fails, an
exception is raised.  The product path never computes on the CPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SEEDSTORY_HIP_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libseedstory_hip.so"))

SS_F32, SS_BF16, SS_F16 = 0, 1, 2
SS_FILTER_BILINEAR, SS_FILTER_BICUBIC = 0, 1
EPI_NONE, EPI_BIAS, EPI_GELU, EPI_RESIDUAL, EPI_SILU_MUL, EPI_GEGLU_PAIR = 0, 1, 2, 4, 8, 16

vp, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
i32p = C.POINTER(C.c_int32)


class SSError(RuntimeError):
    pass


class LlamaConfig(C.Structure):
    _fields_ = [("hidden", i32), ("n_heads", i32), ("n_layers", i32), ("inter", i32), ("vocab", i32),
                ("max_pos", i32), ("rms_eps", f32), ("dtype", i32), ("cache_cap", i32), ("max_new", i32),
                ("n_img_ids", i32), ("eos_id", i32), ("n_seq", i32)]


class LlamaLayerWeights(C.Structure):
    _fields_ = [("wqkv", vp), ("wo", vp), ("wgu", vp), ("wdown", vp), ("ln1", vp), ("ln2", vp)]


class LlamaLayerW8(C.Structure):
    _fields_ = [("wqkv", vp), ("wo", vp), ("wgu", vp), ("wdown", vp), ("s_qkv", vp), ("s_o", vp), ("s_gu", vp), ("s_down", vp)]


class LlamaLayerMx4(C.Structure):       # four code planes, four e8m0 scale planes
    _fields_ = [("wqkv", vp), ("wo", vp), ("wgu", vp), ("wdown", vp), ("s_qkv", vp), ("s_o", vp), ("s_gu", vp), ("s_down", vp)]


class Sampling(C.Structure):
    _fields_ = [("temperature", f32), ("top_p", f32), ("top_k", i32), ("seed", C.c_uint64)]


class LogitsRules(C.Structure):
    _fields_ = [("repetition_penalty", f32), ("no_repeat_ngram", i32), ("min_new_tokens", i32), ("spare_img_ids", i32)]


class BeamParams(C.Structure):
    _fields_ = [("num_beams", i32), ("length_penalty", f32), ("early_stopping", i32)]


BEAM_MAX = 8


class SpecParams(C.Structure):
    """``ss_spec_params``: rows, max n-gram, draft source, the given drafts (device int32) and their count."""
    _fields_ = [("rows", i32), ("max_ngram", i32), ("source", i32), ("given_len", i32), ("given_ids", vp)]


SPEC_LOOKUP, SPEC_GIVEN, SPEC_MAX_ROWS = 0, 1, 8


class BeamState(C.Structure):
    """``ss_beam_state``: the head of a beam-search workspace."""
    _fields_ = [("n", i32), ("K", i32), ("n_stop", i32), ("stop_ids", i32 * 2), ("limit", i32), ("max_new", i32),
                ("early_stopping", i32), ("length_penalty", f32), ("kv0", i32), ("hist0", i32), ("step", i32), ("unsat", i32),
                ("ended", i32), ("pad", i32 * 2), ("run_score", f32 * BEAM_MAX), ("run_live", i32 * BEAM_MAX),
                ("fin_score", f32 * BEAM_MAX), ("fin_len", i32 * BEAM_MAX), ("fin_flag", i32 * BEAM_MAX),
                ("parent", i32 * BEAM_MAX), ("token", i32 * BEAM_MAX)]


class LlamaWeights(C.Structure):
    _fields_ = [("embed", vp), ("lm_head", vp), ("final_norm", vp), ("rope_cos", vp), ("rope_sin", vp),
                ("layers", C.POINTER(LlamaLayerWeights))]


class ResamplerWeights(C.Structure):
    _fields_ = [("q_in", vp), ("pos_kv", vp), ("kv_proj", vp), ("ln_kv_w", vp), ("ln_kv_b", vp), ("in_w", vp),
                ("in_b", vp), ("out_w", vp), ("out_b", vp), ("nq", i32), ("embed", i32), ("n_heads", i32),
                ("kv_dim", i32), ("l_kv", i32), ("ln_eps", f32)]


class VitLayerWeights(C.Structure):
    _fields_ = [(n, vp) for n in ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "in_w", "in_b", "out_w", "out_b", "fc_w",
                                  "fc_b", "proj_w", "proj_b")]


class VitWeights(C.Structure):
    _fields_ = [("conv_w", vp), ("pos", vp), ("ln_pre_w", vp), ("ln_pre_b", vp),
                ("layers", C.POINTER(VitLayerWeights)), ("width", i32), ("n_layers", i32), ("n_heads", i32),
                ("mlp_width", i32), ("patch", i32), ("image", i32), ("kpad", i32), ("ln_eps", f32)]


# name -> (restype, argtypes); every symbol declared in include/seedstory_hip.h
PROTOTYPES = {
    "ss_last_error": (C.c_char_p, []),
    "ss_abi_version": (C.c_int, []),
    "ss_device_info": (C.c_int, [i32p]),
    "ss_rowstats": (C.c_int, [vp, i64, i64, i64, f32, vp, vp, C.c_int, vp]),
    "ss_gemm_lnfold": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, vp, vp, vp, C.c_int, C.c_int, vp]),
    "ss_gemm_rowstat": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, i64, C.c_int, vp, C.c_int, vp]),
    "ss_gemm_rowpart_strips": (i64, [i64, i64, i64, C.c_int]),
    "ss_gemm_rowpart": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, i64, C.c_int, vp, C.c_int, vp]),
    "ss_gemm_lnfold_part": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, vp, i64, i64, f32, vp, vp, C.c_int, C.c_int, vp]),
    "ss_rowstat_finalize": (C.c_int, [vp, i64, i64, f32, vp, vp, vp]),
    "ss_gemm_splitk_workspace_bytes": (C.c_size_t, [i64, i64, i64]),
    "ss_gemm_splitk": (C.c_int, [vp, vp, vp, i64, i64, i64, vp, vp, vp, C.c_size_t, C.c_int, vp]),
    "ss_quantize_rows_fp8": (C.c_int, [vp, i64, i64, i64, vp, vp, vp, vp, f32, C.c_int, vp]),
    "ss_quantize_rows_mxfp4": (C.c_int, [vp, i64, i64, i64, vp, vp, C.c_int, vp]),
    "ss_gemm_fp8": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, i64, i64, vp, vp, i64, C.c_int, vp]),
    "ss_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "ss_context_info": (C.c_int, [vp, C.POINTER(i64)]),
    "ss_destroy": (None, [vp]),
    "ss_rccl_unique_id": (C.c_int, [vp]),
    "ss_rccl_init": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(vp)]),
    "ss_rccl_destroy": (None, [vp]),
    "ss_rccl_send": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
    "ss_rccl_recv": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
    "ss_rccl_bcast": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
    "ss_set_tuning": (C.c_int, [C.c_char_p, C.c_int]),
    "ss_get_tuning": (C.c_int, [C.c_char_p, C.c_int]),
    "ss_rmsnorm": (C.c_int, [vp, vp, vp, i64, i64, f32, C.c_int, vp]),
    "ss_layernorm": (C.c_int, [vp, vp, vp, vp, i64, i64, f32, C.c_int, vp]),
    "ss_add_bcast": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, C.c_int, vp]),
    "ss_silu_mul": (C.c_int, [vp, vp, i64, i64, C.c_int, vp]),
    "ss_gather_rows": (C.c_int, [vp, vp, vp, i64, i64, C.c_int, vp]),
    "ss_scatter_rows": (C.c_int, [vp, vp, vp, i64, i64, C.c_int, vp]),
    "ss_im2col_patch": (C.c_int, [vp, vp, i64, i64, i64, i64, C.c_int, vp]),
    "ss_l2normalize_dim1": (C.c_int, [vp, vp, i64, i64, i64, C.c_int, vp]),
    "ss_rope_kv_append": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i64, C.c_int, vp]),
    "ss_attention": (C.c_int, [vp, vp, vp, vp] + [i64] * 17 + [f32, C.c_int, C.c_int, vp]),
    "ss_attention_ragged": (C.c_int, [vp, vp, vp, vp] + [i64] * 3 + [vp] + [i64] * 13 + [f32, C.c_int, C.c_int, vp]),
    "ss_attn_decode_workspace_bytes": (sz, [i64, i64]),
    "ss_attn_decode": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, i64, C.c_int, vp]),
    "ss_kv_quantize_fp8": (C.c_int, [vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, C.c_int, vp]),
    "ss_attn_decode_kv8": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, C.c_int, vp]),
    "ss_attn_decode_step": (C.c_int, [vp] * 8 + [i64] * 9 + [C.c_int, vp]),
    "ss_attn_decode_kv8_step": (C.c_int, [vp] * 12 + [i64] * 9 + [C.c_int, vp]),
    "ss_attn_scores": (C.c_int, [vp, i64, vp, i64, vp, i64, i64, i64, i64, C.c_int, C.c_int, vp]),
    "ss_gemm": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, i64, C.c_int, C.c_int, vp]),
    "ss_gemm_tune_workspace_bytes": (sz, [i64, i64, i64, C.c_int]),
    "ss_gemm_tune": (C.c_int, [i64, i64, i64, C.c_int, C.c_int, vp, sz, vp, C.POINTER(f32)]),
    "ss_conv3x3_tune_workspace_bytes": (sz, [i64, i64, i64, i64, i64, i64, i64, C.c_int]),
    "ss_conv3x3_tune": (C.c_int, [i64, i64, i64, i64, i64, i64, i64, C.c_int, vp, sz, vp, C.POINTER(f32)]),
    "ss_tune_lookup": (C.c_int, [i64, i64, i64, i64, i64, i64, i64, i64, C.c_int, i32p]),
    "ss_tune_export": (i64, [i32p, i64]),
    "ss_tune_import": (C.c_int, [i32p, i64]),
    "ss_tune_clear": (C.c_int, []),
    "ss_gemv": (C.c_int, [vp, vp, vp, i64, i64, vp, f32, vp, vp, C.c_int, C.c_int, vp]),
    "ss_gemv_batched": (C.c_int, [vp, vp, vp, i64, i64, i64, vp, f32, vp, vp, C.c_int, C.c_int, vp]),
    "ss_gemv_plan": (C.c_int, [i64, i64, i64, C.c_int, C.c_int, C.c_int, C.c_int, i32p, i64]),
    "ss_gemv_w8": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, f32, vp, vp, C.c_int, C.c_int, vp]),
    "ss_gemv_w8_plan": (C.c_int, [i64, i64, i64, C.c_int, C.c_int, C.c_int, i32p, i64]),
    "ss_gemv_mx4": (C.c_int, [vp, vp, vp, vp, i64, i64, i64, vp, f32, vp, vp, C.c_int, C.c_int, vp]),
    "ss_gemv_mx4_plan": (C.c_int, [i64, i64, i64, C.c_int, C.c_int, C.c_int, i32p, i64]),
    "ss_imgproc_argmax": (C.c_int, [vp, i64, vp, vp, i64, vp, C.c_int, vp]),
    "ss_sample_logits": (C.c_int, [vp, i64, i64, i64, C.POINTER(Sampling), vp, C.c_uint32, vp, vp, i64, vp, vp, C.c_int, vp]),
    "ss_process_logits": (C.c_int, [vp, i64, i64, i64, C.POINTER(LogitsRules), vp, i64, vp, vp, i32, vp, i64, C.c_int, vp]),
    "ss_token_logprobs": (C.c_int, [vp, i64, i64, i64, vp, C.POINTER(Sampling), i32, vp, vp, vp, C.c_int, vp]),
    "ss_beam_step": (C.c_int, [vp, i64, i64, i64, vp, i32, i32p, vp, vp, vp, C.c_int, vp]),
    "ss_llama_workspace_bytes": (sz, [C.POINTER(LlamaConfig), i64]),
    "ss_llama_create": (C.c_int, [C.POINTER(LlamaConfig), C.POINTER(LlamaWeights), vp, sz, i64, i32p,
                                  C.POINTER(vp)]),
    "ss_llama_destroy": (None, [vp]),
    "ss_llama_select": (C.c_int, [vp, i32]),
    "ss_llama_set_stop_id": (C.c_int, [vp, i32]),
    "ss_llama_set_attn_capture": (C.c_int, [vp, vp, i64, i64, i64, i32, i32]),
    "ss_llama_set_decode_w8": (C.c_int, [vp, C.POINTER(LlamaLayerW8), vp, vp]),
    "ss_llama_set_decode_mx4": (C.c_int, [vp, C.POINTER(LlamaLayerMx4), vp, vp]),
    "ss_llama_kv8_bytes": (C.c_int, [C.POINTER(LlamaConfig), C.POINTER(sz), C.POINTER(sz)]),
    "ss_llama_set_kv8": (C.c_int, [vp, vp, vp, vp, vp]),
    "ss_llama_kv8_invalidate": (C.c_int, [vp, i64]),
    "ss_llama_set_sampling": (C.c_int, [vp, i32, C.POINTER(Sampling)]),
    "ss_llama_set_logits_rules": (C.c_int, [vp, i32, C.POINTER(LogitsRules)]),
    "ss_llama_set_logprobs": (C.c_int, [vp, i32, vp, vp, vp, vp, i32]),
    "ss_llama_set_history": (C.c_int, [vp, i32, i32p, i64, i32]),
    "ss_llama_buffer": (vp, [vp, C.c_int]),
    "ss_llama_set_lengths": (C.c_int, [vp, i64, i64, vp]),
    "ss_llama_get_lengths": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
    "ss_llama_kv_gather": (C.c_int, [vp, vp, i64, vp]),
    "ss_llama_fork": (C.c_int, [vp, i32, i32p, i32, vp]),
    "ss_llama_beam_bytes": (sz, [C.POINTER(LlamaConfig), i32]),
    "ss_llama_beam_seq_offset": (sz, []),
    "ss_llama_beam_search": (C.c_int, [vp, C.POINTER(BeamParams), vp, i64, i32, vp]),
    "ss_llama_beam_permute": (C.c_int, [vp, vp, i32p, i32, i64, i64, vp]),
    "ss_llama_spec_bytes": (C.c_int, [C.POINTER(LlamaConfig), i32, C.POINTER(sz)]),
    "ss_llama_set_speculation": (C.c_int, [vp, C.POINTER(SpecParams), vp]),
    "ss_llama_spec_stats": (C.c_int, [vp, i32, C.POINTER(i64)]),
    "ss_attn_decode_spec": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, i64, C.c_int, vp]),
    "ss_spec_draft": (C.c_int, [vp, i64, i32, i32, i32, i32p, vp, vp, vp]),
    "ss_llama_prefill": (C.c_int, [vp, vp, i64, vp, vp, vp]),
    "ss_llama_prefill_batch": (C.c_int, [vp, vp, C.POINTER(i64), vp, vp]),
    "ss_llama_generate": (C.c_int, [vp, i64, i32, i32p, i64, C.POINTER(i64), vp]),
    "ss_llama_generate_batch": (C.c_int, [vp, i64, i32p, i32p, i64, C.POINTER(i64), i32p, C.POINTER(i64), vp]),
    "ss_llama_profile_decode": (C.c_int, [vp, i64, C.POINTER(f32), C.POINTER(C.c_double), vp]),
    "ss_resampler_workspace_bytes": (sz, [C.POINTER(ResamplerWeights), i64, C.c_int]),
    "ss_resampler_forward": (C.c_int, [C.POINTER(ResamplerWeights), vp, vp, i64, vp, sz, C.c_int, vp]),
    "ss_vit_workspace_bytes": (sz, [C.POINTER(VitWeights), i64, C.c_int]),
    "ss_vit_forward": (C.c_int, [C.POINTER(VitWeights), vp, vp, i64, vp, sz, C.c_int, vp]),
    "ss_vit_blocks": (C.c_int, [C.POINTER(VitWeights), vp, i64, i64, i64, i64, vp, sz, C.c_int, vp]),
    "ss_conv3x3": (C.c_int, [vp, vp, vp, i64, i64, i64, i64, i64, i64, i64, vp, vp, i64, vp, C.c_int, vp]),
    "ss_loss_workspace_bytes": (C.c_size_t, [i64]),
    "ss_cross_entropy_rows": (C.c_int, [vp, i64, vp, i64, i64, i64, vp, vp, C.c_int, vp]),
    "ss_cosine_rows": (C.c_int, [vp, vp, i64, i64, vp, C.c_int, vp]),
    "ss_masked_mean": (C.c_int, [vp, vp, i64, vp, vp, vp]),
    "ss_mse": (C.c_int, [vp, vp, i64, vp, vp, C.c_int, vp]),
    "ss_groupnorm_workspace_bytes": (C.c_size_t, [i64, i64, i64, i64, C.c_int]),
    "ss_groupnorm": (C.c_int, [vp, vp, vp, vp, vp, i64, i64, i64, i64, f32, C.c_int, C.c_int, vp]),
    "ss_geglu": (C.c_int, [vp, vp, i64, i64, C.c_int, vp]),
    "ss_unary": (C.c_int, [vp, vp, i64, C.c_int, C.c_int, vp]),
    "ss_softmax_rows": (C.c_int, [vp, i64, i64, f32, C.c_int, vp]),
    "ss_transpose": (C.c_int, [vp, vp, i64, i64, C.c_int, vp]),
    "ss_concat_channels": (C.c_int, [vp, vp, vp, i64, i64, i64, C.c_int, vp]),
    "ss_layout_nchw_nhwc": (C.c_int, [vp, vp, i64, i64, i64, i64, C.c_int, C.c_int, vp]),
    "ss_euler_scale_dup": (C.c_int, [vp, vp, i64, f32, C.c_int, vp]),
    "ss_euler_cfg_step": (C.c_int, [vp, vp, i64, f32, f32, f32, C.c_int, vp]),
    "ss_multistep_cfg_step": (C.c_int, [vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, f32, C.c_int, vp]),
    "ss_multistep_step": (C.c_int, [vp, vp, vp, vp, i64, C.c_int, C.c_int, f32, f32, f32, f32, f32, f32, C.c_int, vp]),
    "ss_randn_philox": (C.c_int, [vp, vp, i64, i64, C.c_int, C.c_int, vp]),
    "ss_multistep_noise_step": (C.c_int, [vp, vp, vp, vp, i64, C.c_int, C.c_int, f32, f32, f32, f32, f32, f32, f32, vp, i64, C.c_int,
                                          C.c_int, vp]),
    "ss_euler_step": (C.c_int, [vp, vp, i64, f32, f32, C.c_int, vp]),
    "ss_euler_scale": (C.c_int, [vp, vp, i64, C.c_int, f32, C.c_int, vp]),
    "ss_resample_ksize": (C.c_int, [i64, i64, C.c_int]),
    "ss_resample_coeffs": (C.c_int, [i64, i64, C.c_int, i32p, i32p]),
    "ss_image_preprocess": (C.c_int, [vp, i64, i64, vp, vp, i64, i64, i64, i64, i64, i64, vp, vp, C.c_int, vp, vp, C.c_int,
                                      i64, i64, vp, C.POINTER(f32), C.POINTER(f32), C.c_int, vp]),
    "ss_image_to_u8": (C.c_int, [vp, vp, i64, i64, C.c_int, vp]),
    "ss_debug_tr_probe": (C.c_int, [vp, vp, vp, vp]),
}

_lib = None


def lib():
    """The loaded library; raises if it was not built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SSError("libseedstory_hip.so not found at %s — build it first (seed-story_amd/csrc/Makefile); "
                          "there is no CPU fallback" % LIB_PATH)
        # torch ships its own libamdhip64.so.7 (+ HSA runtime); it must be the copy this process binds
        # to, or the two runtimes disagree about the device ("no ROCm-capable device").  Import torch
        # first so the library's DT_NEEDED libamdhip64.so.7 resolves to the already-loaded one.
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(l, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if l.ss_abi_version() != 1:
            raise SSError("ABI version mismatch")
        _lib = l
        from . import tune
        tune.load_default_table()
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().ss_last_error()
        raise SSError("%s failed (%d): %s" % (what or "seedstory call", rc, msg.decode() if msg else "?"))


_tuning_gen = 0     # bumped by every set_tuning: captured hipGraphs replay the arithmetic / kernels chosen at capture time


def set_tuning(key: str, value: int):
    global _tuning_gen
    check(lib().ss_set_tuning(key.encode(), int(value)), "ss_set_tuning")
    _tuning_gen += 1


def tuning_generation() -> int:
    """Counter of ``set_tuning`` calls: part of the key of every captured graph on the Python side (toggling
    ``gemm_f32_split`` / ``attn_ver`` after a first render used to replay the old arithmetic)."""
    return _tuning_gen


def get_tuning(key: str, default: int = 0) -> int:
    return int(lib().ss_get_tuning(key.encode(), int(default)))
