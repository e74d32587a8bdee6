"""ctypes binding of libdalm_hip.so (the C ABI in include/dalm_hip.h).

This module is the only place that touches the shared object.  There is NO CPU
fallback: if the library is missing, or a tensor is not on a HIP device, the
call raises.  torch is used for device memory and the current stream only.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path
from typing import Callable, Dict, Optional, TypeVar

import torch

_LIB_PATH = Path(__file__).resolve().parent / "csrc" / "libdalm_hip.so"
_lib: Optional[C.CDLL] = None

F32, BF16 = 0, 1
_i64, _f32, _int, _vp, _sz = C.c_int64, C.c_float, C.c_int, C.c_void_p, C.c_size_t

# name -> (restype, argtypes); mirrors include/dalm_hip.h one to one
SIGNATURES = {
    "dalm_version": (_int, []),
    "dalm_last_error_string": (C.c_char_p, []),
    "dalm_pool_l2norm_fwd": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "dalm_pool_l2norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _int, _vp, _int, _vp]),
    "dalm_sim_matmul": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _vp, _i64, _vp]),
    "dalm_gemm_f32": (_int, [_int, _int, _i64, _i64, _i64, _f32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "dalm_sim_rowstats_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_rowstats": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "dalm_sim_rowstats_f32": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "dalm_sim_rowstats_bf16x3_supported": (_int, [_i64, _i64, _i64]),
    "dalm_sim_rowstats_bf16x3_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_rowstats_bf16x3": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _sz, _vp]),
    "dalm_sim_grad_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_grad": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_nt_xent_fwd": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "dalm_nt_xent_bwd": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _int, _vp]),
    "dalm_marg_ce_prep": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "dalm_marg_ce_fwd": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_marg_ce_bwd": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_scale_inplace": (_int, [_vp, _int, _i64, _vp, _vp]),
    "dalm_marg_ce_finalize": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "dalm_marg_ce_finalize_topk": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_marg_ce_bwd_weighted": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_doc_scores_topk_fwd": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _vp, _vp, _vp]),
    "dalm_doc_scores_topk_bwd": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_doc_logprob_fwd": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "dalm_doc_logprob_bwd": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _int, _vp]),
    "dalm_gather_nll": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "dalm_marginalize_rows": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "dalm_marginalize_rows_dev": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "dalm_contrastive_finalize": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
    "dalm_pool_l2norm_fwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dalm_pool_l2norm_fwd_ws": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_sim_small_supported": (_int, [_i64, _i64, _i64]),
    "dalm_sim_small_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dalm_sim_small_fwd": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_sim_small_fwd1_preferred": (_int, [_i64, _i64, _i64]),
    "dalm_sim_small_fwd1_workspace_bytes": (_sz, [_i64, _i64, _i64, _int]),
    "dalm_sim_small_fwd1_ticket_words": (_sz, [_i64, _i64]),
    "dalm_sim_small_fwd1": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "dalm_sim_small_bwd": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_sim_small_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _int]),
    "dalm_sim_small_bwd1_workspace_bytes": (_sz, [_i64, _i64, _i64, _int, _int]),
    "dalm_sim_small_bwd1_ticket_words": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_small_bwd1": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "dalm_sim_small_bwd_ws": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_rag_loss_finalize": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "dalm_sim_topk_supported": (_int, [_i64, _i64]),
    "dalm_sim_topk_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "dalm_sim_topk": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_pool_l2norm_packed_fwd": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "dalm_pool_last_packed_fwd": (_int, [_vp, _int, _vp, _i64, _i64, _i64, _i64, _int, _vp, _i64, _vp, _vp]),
    "dalm_pool_last_packed_bwd": (_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _int, _vp, _int, _vp]),
    "dalm_sim_gold_score": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp]),
    "dalm_sim_gold_rank_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_gold_rank": (_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _f32, _vp, _vp, _vp, _sz, _vp]),
    "dalm_lm_head_lse_workspace_bytes": (_sz, [_i64, _i64]),
    "dalm_lm_head_lse_fwd": (_int, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "dalm_comm_unique_id": (_int, [_vp]),
    "dalm_comm_init": (_int, [C.POINTER(_vp), _vp, _int, _int, _int]),
    "dalm_comm_destroy": (_int, [_vp]),
    "dalm_comm_rank": (_int, [_vp]),
    "dalm_comm_world": (_int, [_vp]),
    "dalm_comm_wait_stream": (_int, [_vp, _vp]),
    "dalm_comm_stream_wait": (_int, [_vp, _vp]),
    "dalm_comm_allgather": (_int, [_vp, _vp, _vp, _sz]),
    "dalm_comm_allreduce_sum_f32": (_int, [_vp, _vp, _sz]),
    "dalm_comm_allgather_on": (_int, [_vp, _vp, _vp, _sz, _vp]),
    "dalm_comm_allreduce_sum_f32_on": (_int, [_vp, _vp, _sz, _vp]),
    "dalm_nf4_packed_bytes": (_sz, [_i64]),
    "dalm_nf4_absmax_count": (_sz, [_i64]),
    "dalm_nf4_quantize": (_int, [_vp, _int, _i64, _vp, _vp, _vp]),
    "dalm_nf4_dequantize": (_int, [_vp, _vp, _i64, _int, _vp, _vp]),
    "dalm_rope_qk": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp]),
    "dalm_swiglu_fwd": (_int, [_vp, _vp, _vp, _int, _i64, _vp]),
    "dalm_swiglu_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _vp]),
    "dalm_swiglu_fwd_2d": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp]),
    "dalm_swiglu_bwd_2d": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp]),
    "dalm_rms_norm_fwd": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "dalm_rms_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "dalm_layer_norm_fwd": (_int, [_vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "dalm_layer_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "dalm_gelu_fwd": (_int, [_vp, _vp, _i64, _vp]),
    "dalm_gelu_bwd": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "dalm_add3": (_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "dalm_bert_add_norm_fwd": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _i64, _f32, _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_bert_add_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp]),
    "dalm_attn_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _f32, _vp, C.c_uint32, _vp, _vp, _vp]),
    "dalm_attn_mask_bits": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "dalm_attn_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _i64, _i64,
                             _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_attn_mask_bits_packed": (_int, [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp, _vp]),
    "dalm_attn_fwd_packed": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _f32, _vp, C.c_uint32, _vp, _vp, _vp]),
    "dalm_attn_bwd_packed": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _i64,
                                    _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_attn_rel_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _i64, _i64, _f32, _vp, C.c_uint32,
                                 _vp, _vp, _vp]),
    "dalm_attn_rel_fwd_packed": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _i64, _i64, _vp, _f32,
                                        _vp, C.c_uint32, _vp, _vp, _vp]),
    "dalm_attn_rel_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _i64, _i64,
                                 _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_attn_rel_bwd_packed": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _f32, _vp, _vp,
                                        _i64, _i64, _vp, _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_attn_gqa_fwd": (_int,[_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "dalm_attn_gqa_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _f32, _vp, _vp, _vp,
                                 _i64, _i64, _i64, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "dalm_attn_gqa_bwd_splits": (_i64, [_i64, _i64, _i64, _i64]),
    "dalm_attn_gqa_bwd_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "dalm_lora_rowdot": (_int, [_vp, _int, _vp, _int, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32, _vp, _vp]),
    "dalm_lora_rankupd": (_int, [_vp, _int, _vp, _vp, _int, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32, _vp]),
    "dalm_lora_colacc_workspace_bytes": (_sz, [_i64, _i64, _int]),
    "dalm_lora_colacc": (_int, [_vp, _int, _vp, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32, _vp, _int, _vp, _sz, _vp]),
    "dalm_lora2_rowdot": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32, C.c_uint32,
                                 _int, _vp]),
    "dalm_lora2_rankupd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp]),
    "dalm_lora2_colacc_workspace_bytes": (_sz, [_i64, _i64, _int, _int]),
    "dalm_lora2_colacc_ticket_words": (_sz, [_i64, _int]),
    "dalm_sim_grad_bf16x3_supported": (_int, [_i64, _i64, _i64]),
    "dalm_sim_grad_bf16x3_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "dalm_sim_grad_bf16x3": (_int, [_vp, _vp, _i64, _i64, _i64, _f32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dalm_lm_head_dlogits": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dalm_lm_head_logits": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dalm_lm_head_dhidden": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _int, _vp]),
    "dalm_transpose_bf16": (_int, [_vp, _i64, _i64, _i64, _vp, _i64, _vp]),
    "dalm_f32_to_bf16": (_int, [_vp, _vp, _i64, _vp]),
    "dalm_lora2_colacc": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp, _sz, _vp, _vp]),
    # the row-wise kernels with a row-liveness vector (one `row_live` pointer in front of the stream; NULL = the plain form)
    "dalm_rope_qk_live": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _int, _vp,
                                 _vp]),
    "dalm_swiglu_fwd_live": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "dalm_swiglu_bwd_live": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "dalm_swiglu_fwd_2d_live": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "dalm_swiglu_bwd_2d_live": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "dalm_rms_norm_fwd_live": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_rms_norm_bwd_live": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp, _vp]),
    # Qwen3's q_norm / k_norm + rotary embedding (forward) and the norm's backward, q and k in one launch each
    "dalm_head_norm_rope_fwd": (_int, [_vp, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_head_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _vp]),
    # Gemma: GeGLU and the (1 + w) RMSNorm, one entry point per direction (row liveness is an argument)
    "dalm_geglu_fwd": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "dalm_geglu_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "dalm_gemma_norm_fwd": (_int, [_vp, _vp, _vp, _int, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_gemma_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _int, _i64, _i64, _vp, _vp, _vp]),
    # Arcee: ReLU^2 (ArceeMLP's activation), one entry point per direction (row liveness is an argument)
    "dalm_relu2_fwd": (_int, [_vp, _vp, _int, _i64, _i64, _i64, _i64, _vp, _vp]),
    "dalm_relu2_bwd": (_int, [_vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    # OLMo-2: norm-then-add (the post-norm of its decoder layer) and q_norm / k_norm over the whole projection width + rotary
    "dalm_norm_add_fwd": (_int, [_vp, _vp, _vp, _int, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    "dalm_norm_add_bwd": (_int, [_vp, _vp, _vp, _vp, _int, _int, _i64, _i64, _vp, _vp, _vp]),
    "dalm_row_norm_rope_fwd": (_int, [_vp, _vp, _vp, _vp, _int, _f32, _f32, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "dalm_row_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _vp, _vp, _vp, _vp]),
    # Granite: the scaled residual add, with the RMSNorm behind it (forward, backward) and alone
    "dalm_rms_norm_scaled_fwd": (_int, [_vp, _vp, _f32, _vp, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_rms_norm_scaled_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _f32, _int, _i64, _i64, _vp, _vp, _vp, _vp]),
    "dalm_scale_add": (_int, [_vp, _vp, _f32, _vp, _int, _i64, _i64, _vp, _vp]),
    # Cohere: the interleaved f32 rotary embedding of q and k, the bias-free f32 LayerNorm (forward, backward), residual + attn + mlp
    "dalm_rope_il_qk": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _int,
                               _vp, _vp]),
    "dalm_cohere_norm_fwd": (_int, [_vp, _vp, _int, _int, _i64, _i64, _f32, _vp, _vp, _vp, _vp, _vp]),
    "dalm_cohere_norm_bwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _int, _i64, _i64, _vp, _vp, _vp]),
    "dalm_add3_live": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _i64, _vp, _vp]),
    # Phi-3: the partial rotary embedding of q and k (the first `rot` elements of a head rotate, the rest pass through)
    "dalm_rope_partial_qk": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                    _int, _vp, _vp]),
    "dalm_bert_add_norm_fwd_live": (_int, [_vp, _vp, _vp, _vp, _int, _i64, _i64, _f32, _f32, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                           _vp, _vp]),
    "dalm_bert_add_norm_bwd_live": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _vp, _vp, _vp, _i64, _i64, _f32, _vp, _vp, _vp, _vp]),
    # RoBERTa-family embeddings: positions from ids + three table rows + LayerNorm + dropout, forward only
    "dalm_embed_norm_fwd": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _i64, _i64, _i64, _f32, _f32,
                                   _vp, C.c_uint32, _vp, _vp, _vp, _vp]),
    "dalm_lora2_rowdot_live": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32,
                                      C.c_uint32, _int, _vp, _vp]),
    "dalm_lora2_rankupd_live": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp, _vp]),
    "dalm_lora2_colacc_live": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp, _sz, _vp, _vp, _vp]),
    # the same with a row stride `ld` (elements) for the bf16 activation operand, in front of the stream
    "dalm_lora2_rowdot_ld": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _f32, _vp, C.c_uint32,
                                    C.c_uint32, _int, _vp, _i64, _vp]),
    "dalm_lora2_rankupd_ld": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp, _i64, _vp]),
    "dalm_lora2_colacc_ld": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _f32, _int, _vp, _sz, _vp, _vp, _i64,
                                    _vp]),
    # host-only queries of the launch geometry (csrc/lora2_plan.hpp)
    "dalm_lora2_rankupd_rows_per_wg": (_int, [_i64, _i64, _int]),
    "dalm_lora2_colacc_rows_per_split": (_int, [_i64, _i64, _int, _int]),
    # padded step: stable partition of the row-liveness vector and the frozen-projection GEMM over the live rows
    "dalm_row_partition": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "dalm_linear_live": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _int, _vp]),
    # the frozen SwiGLU MLP node: SwiGLU inside the epilogue of the gate | up forward
    "dalm_linear_live_swiglu_prepare": (_int, [_vp]),
    "dalm_linear_live_swiglu": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    # the frozen ReLU^2 MLP node: relu(y)^2 inside the epilogue of the up forward
    "dalm_linear_live_relu2": (_int, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
}


def library_path() -> Path:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load (once) and return the shared library; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise RuntimeError(
            f"{_LIB_PATH} is missing: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m dalm_amd._build` (needs hipcc, targets gfx950)."
        )
    lib = C.CDLL(str(_LIB_PATH))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here == header/library drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class DalmHipError(RuntimeError):
    pass


def _check(rc: int, name: str) -> None:
    if rc == 0:
        return
    msg = load().dalm_last_error_string().decode("utf-8", "replace")
    if rc < 0:
        raise ValueError(f"{name} rejected its arguments (code {rc}): {msg}")
    raise DalmHipError(f"{name} failed with hipError {rc}: {msg}")


def call(name: str, *args) -> None:
    _check(getattr(load(), name)(*args), name)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


_capture_info = None


def capture_id(stream_handle: int) -> int:
    """Id of the hipGraph capture in progress on a stream, 0 when it is not capturing.  Graphs captured one after another on the
    SAME stream (torch.cuda.make_graphed_callables captures every graph on one shared stream) may replay concurrently on
    different streams, so device state cached per stream must be cached per capture while one is in progress."""
    global _capture_info
    if _capture_info is None:
        fn = load().hipStreamGetCaptureInfo     # the HIP runtime the library launches with (dlsym searches its dependencies)
        fn.restype = C.c_int
        fn.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong)]
        _capture_info = fn
    status, cid = C.c_int(0), C.c_ulonglong(0)
    rc = _capture_info(stream_handle, C.byref(status), C.byref(cid))
    if rc != 0:
        raise DalmHipError(f"hipStreamGetCaptureInfo failed with hipError {rc}")
    return int(cid.value) if status.value == 1 else 0     # hipStreamCaptureStatusActive


T = TypeVar("T")


def capture_scratch(cache: Dict[tuple, T], device: torch.device, make: Callable[[], T],
                    keep: Callable[[T], bool] = lambda _: True) -> T:
    """Device state owned by (device, current stream, capture id), held in its caller's `cache`: what `make()` built for that
    owner, built again when `keep` rejects the cached value.  Calls that share it are ordered by that stream.  The capture id is
    part of the key because graphs captured one after another on the SAME stream (torch.cuda.make_graphed_callables captures
    every graph on one shared stream: the tower graphs of training/graphed.py) may replay concurrently on different streams -
    the retriever towers on their own stream beside the generator's.  With state shared between two such graphs their kernels'
    arrivals mixed and the reductions summed incomplete partial tiles (NaN losses in bf16 with tower graphs).  So device state a
    graph reads is owned by the capture that recorded it, never shared with an eager region or another capture.  Kept for the
    life of the process."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = torch.cuda.current_stream(idx).cuda_stream
    key = (idx, s, capture_id(s))
    val = cache.get(key)
    if val is None or not keep(val):
        val = cache[key] = make()
    return val


def require_gpu(*tensors: torch.Tensor) -> torch.device:
    """All tensors must live on the same HIP device; returns it."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "dalm_amd: tensor is on %s; the loss path runs only as HIP kernels on an MI355X "
                "(there is no CPU implementation in this package)" % t.device
            )
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError(f"dalm_amd: tensors on different devices ({dev} vs {t.device})")
    if dev is None:
        raise RuntimeError("dalm_amd: no tensor arguments")
    return dev


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"dalm_amd: unsupported dtype {t.dtype} (float32 or bfloat16 expected)")


def as_i64(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dtype == torch.int64 and t.is_contiguous()) else t.to(torch.int64).contiguous()


def as_f32c(t: torch.Tensor) -> torch.Tensor:
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()
