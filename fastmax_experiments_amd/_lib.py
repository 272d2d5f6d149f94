"""ctypes binding of the C ABI declared in the public headers under include/ (HEADERS): one table, ABI, set on one handle.

Fails loudly: if libfastmax_hip.so is absent or a symbol is missing, importing the operator
raises -- there is no eager/PyTorch/CPU fallback for the hot path.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# FASTMAX_LIB_PATH: A/B runs of tools/ against another build of the same library (never a different implementation)
LIB_PATH = os.environ.get("FASTMAX_LIB_PATH") or os.path.join(HERE, "libfastmax_hip.so")

F32, BF16, F16, F64 = 0, 1, 2, 3          # F64: the operator's entry points only, float64 in and out
PATH_AUTO, PATH_QUADRATIC, PATH_RECURRENT, PATH_MFMA, PATH_QUADRATIC_MFMA = 0, 1, 2, 3, 4
PATH_NAMES = {PATH_AUTO: "auto", PATH_QUADRATIC: "quadratic", PATH_RECURRENT: "recurrent", PATH_MFMA: "mfma", PATH_QUADRATIC_MFMA: "quadratic_mfma"}
ABI_VERSION = 9
OK, E_BAD_P, E_BAD_SHAPE, E_BAD_DTYPE, E_WORKSPACE, E_ALIGNMENT, E_NULL = 0, -1, -2, -3, -4, -5, -6      # enum fastmax_error


class Problem(ctypes.Structure):
    _fields_ = [("B", ctypes.c_int), ("H", ctypes.c_int), ("Nq", ctypes.c_int), ("Nk", ctypes.c_int),
                ("D", ctypes.c_int), ("in_dtype", ctypes.c_int), ("out_dtype", ctypes.c_int), ("p", ctypes.c_int),
                ("causal", ctypes.c_int), ("a", ctypes.c_float), ("b", ctypes.c_float), ("g0", ctypes.c_float),
                ("path", ctypes.c_int)]


class Plan(ctypes.Structure):
    """struct fastmax_plan: what fastmax_hip_plan reports"""
    _fields_ = [("rc", ctypes.c_int), ("path", ctypes.c_int), ("fwd_kernel", ctypes.c_int), ("bwd_kernel", ctypes.c_int),
                ("nseg", ctypes.c_int), ("state_bytes", ctypes.c_size_t)]


# enum fastmax_fwd_kernel / fastmax_bwd_kernel, by number
FWD_KERNELS = ["FWD_QUADRATIC", "FWD_RECURRENT", "FWD_UNMASKED_LIN", "FWD_SCAN_V2", "FWD_SCAN_D128_2P", "FWD_SCAN_BF16", "FWD_SCAN_GEN",
               "FWD_QUAD32", "FWD_QUAD_MFMA", "FWD_F64"]
BWD_KERNELS = ["BWD_QUADRATIC", "BWD_UNMASKED_LIN", "BWD_LIN", "BWD_SCAN", "BWD_QUAD32", "BWD_QUAD_MFMA", "BWD_F64"]

vp, sz, ci, i64, cf, cs = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_char_p
i64p, pp, planp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(Problem), ctypes.POINTER(Plan)
QKV = [vp, i64p, vp, i64p, vp, i64p]          # q, q_strides, k, k_strides, v, v_strides
BWD = [pp] + QKV + [vp, vp, vp, i64p]         # ..., o, g, grad_o, go_strides
NF4 = [vp, i64, vp, vp, vp, vp, vp, vp, i64, ci, ci, ci, ci, vp]
ACT_SILU, ACT_GELU = 0, 1                       # enum fastmax_gated_act (include/fastmax_hip_block.h)
# the public headers under include/: one library, one FASTMAX_ABI_VERSION.  A new header goes at the end, with its rows at the
# end of ABI.
HEADERS = ("fastmax_hip.h", "fastmax_hip_generate.h", "fastmax_hip_linearmax_decode.h", "fastmax_hip_block.h", "fastmax_hip_optim.h",
           "fastmax_hip_next_token.h", "fastmax_hip_neox.h", "fastmax_hip_cursor.h", "fastmax_hip_nucleus.h", "fastmax_hip_moe.h",
           "fastmax_hip_moe_decode.h", "fastmax_hip_head.h", "fastmax_hip_adapter.h", "fastmax_hip_kv_decode.h")
NEOX_ACT_GELU = 0                               # enum fastmax_neox_act (include/fastmax_hip_neox.h)
CURSOR_POS, CURSOR_NEXT, CURSOR_DRAW_BASE, CURSOR_SEED, CURSOR_OVERFLOW = range(5)          # enum fastmax_cursor_word
NUCLEUS_MAX_V = 1 << 22                         # the largest V the fixed-point mass of top-p sampling admits
MOE_MAX_EXPERTS, MOE_MAX_PER_TOKEN = 64, 8      # FASTMAX_MOE_MAX_EXPERTS, FASTMAX_MOE_MAX_PER_TOKEN
MOE_DECODE_MAX_ROWS = 16                        # FASTMAX_MOE_DECODE_MAX_ROWS
ADAPTER_ROWS_PER_BLOCK = 64                     # FASTMAX_ADAPTER_ROWS_PER_BLOCK
KV_CHUNK, KV_SLICE, KV_MAX_D = 128, 8, 256      # FASTMAX_KV_CHUNK, FASTMAX_KV_SLICE, FASTMAX_KV_MAX_D
KV_LEN, KV_OVERFLOW, KV_HEADER_WORDS = 0, 1, 16  # enum fastmax_kv_word
# every function the HEADERS declare, in their order and in each header's own order: name -> (restype, argtypes).
# tests/test_binding_cpu.py checks each row against the prototype.
ABI = {
    # fastmax_hip.h
    "fastmax_hip_tune": (ci, [cs, ci]),
    "fastmax_hip_tune_get": (ci, [cs]),
    "fastmax_hip_build_flags": (ci, []),
    "fastmax_hip_forward_workspace": (sz, [pp]),
    "fastmax_hip_forward": (ci, [pp] + QKV + [vp, vp, vp, sz, vp]),
    "fastmax_hip_backward_workspace": (sz, [pp]),
    "fastmax_hip_backward": (ci, BWD + [vp, vp, vp, vp, sz, vp]),
    "fastmax_hip_forward_state_bytes": (sz, [pp] + QKV + [vp]),
    "fastmax_hip_backward_with_states": (ci, BWD + [vp, vp, vp, vp, sz, vp, sz, vp]),
    "fastmax_hip_plan": (ci, [pp] + QKV + [vp, vp, i64p, vp, vp, vp, planp]),
    "fastmax_hip_normalize_workspace": (sz, [ci, ci]),
    "fastmax_hip_normalize": (ci, [vp, i64p, ci, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_stats": (ci, [vp, i64p, ci, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_stats2_workspace": (sz, [ci, ci, ci]),
    "fastmax_hip_normalize_stats2": (ci, [vp, i64p, vp, i64p, ci, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_cast": (ci, [vp, i64p, ci, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_backward_workspace": (sz, [ci, ci, ci]),
    "fastmax_hip_normalize_backward": (ci, [vp, i64p, ci, vp, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_cast_expand": (ci, [vp, i64p, ci, vp, vp, ci, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_normalize_backward_expand": (ci, [vp, i64p, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_linearmax_forward": (ci, [pp] + QKV + [vp, vp, vp, vp, vp, sz, vp]),
    "fastmax_hip_linearmax_forward_auto_workspace": (sz, [pp]),
    "fastmax_hip_linearmax_forward_auto": (ci, [pp] + QKV + [vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "fastmax_hip_linearmax_train_supported": (ci, [pp]),
    "fastmax_hip_linearmax_backward": (ci, BWD + [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, sz, ci, vp]),
    "fastmax_hip_rope_qkv_split": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_rope_qkv_split_backward": (ci, [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_cross_entropy_forward": (ci, [vp, i64, vp, vp, vp, i64, ci, i64, ci, vp]),
    "fastmax_hip_cross_entropy_backward": (ci, [vp, i64, vp, vp, vp, cf, vp, i64, i64, ci, i64, ci, vp]),
    "fastmax_hip_decode_state_bytes": (sz, [ci, ci, ci]),
    "fastmax_hip_p1_prefill_state": (ci, [pp, vp, i64p, vp, i64p, vp, vp]),
    "fastmax_hip_p1_decode_step": (ci, QKV + [vp, vp, ci, ci, ci, ci, ci, cf, i64, vp]),
    "fastmax_hip_p2_decode_state_bytes": (sz, [ci, ci, ci]),
    "fastmax_hip_p2_prefill_state": (ci, [pp, vp, i64p, vp, i64p, vp, vp]),
    "fastmax_hip_p2_decode_step": (ci, QKV + [vp, vp, ci, ci, ci, ci, ci, ci, cf, vp]),
    "fastmax_hip_p2_extend_workspace": (sz, [ci, ci, ci, ci, ci]),
    "fastmax_hip_p2_extend": (ci, [pp, ci] + QKV + [vp, vp, vp, sz, vp]),
    "fastmax_hip_nf4_linear_forward": (ci, NF4),
    "fastmax_hip_nf4_linear_backward_input": (ci, [vp, i64, vp, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_nf4_dequantize": (ci, [vp, vp, vp, i64, ci, vp]),
    "fastmax_hip_nf4_linear_forward_s": (ci, NF4),
    "fastmax_hip_nf4_linear_backward_input_s": (ci, [vp, i64, vp, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_nf4_dequantize_s": (ci, [vp, vp, vp, i64, ci, vp]),
    "fastmax_hip_qlora_gemm": (ci, [vp, i64, vp, ci, vp, vp, vp, vp, ci, vp, i64, ci, ci, ci, vp]),
    "fastmax_hip_qlora_gemm_rope": (ci, [vp, i64, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_nf4_dequantize_transposed": (ci, [vp, vp, vp, ci, ci, vp]),
    "fastmax_hip_lora_down": (ci, [vp, i64, vp, i64, vp, i64, vp, i64, ci, ci, ci, vp]),
    "fastmax_hip_lora_tn_workspace": (i64, [ci, ci, ci]),
    "fastmax_hip_lora_tn": (ci, [vp, i64, vp, i64, vp, ci, ci, ci, vp, ci, ci, ci, vp]),
    "fastmax_hip_lora_up": (ci, [vp, i64, vp, i64, vp, i64, ci, vp, ci, ci, ci, vp]),
    "fastmax_hip_lora_down_dropout": (ci, [vp, i64, vp, i64, vp, i64, vp, i64, ci, ci, ci, vp, cf, vp]),
    "fastmax_hip_lora_tn_dropout": (ci, [vp, i64, vp, i64, vp, ci, ci, ci, vp, ci, ci, ci, vp, cf, vp]),
    "fastmax_hip_lora_up_dropout": (ci, [vp, i64, vp, i64, vp, i64, ci, vp, ci, ci, ci, vp, cf, vp]),
    "fastmax_hip_lora_dropout_mask": (ci, [vp, ci, ci, vp, cf, vp]),
    "fastmax_hip_lora_scatter": (ci, [vp, ci, ci, vp, ci, cf, vp, i64, ci, ci, vp]),
    "fastmax_hip_lora_scatter_backward": (ci, [vp, ci, i64, vp, vp, cf, vp, ci, ci, ci, vp]),
    "fastmax_hip_abi_version": (ci, []),
    "fastmax_hip_select_path": (ci, [pp]),
    "fastmax_hip_error_string": (cs, [ci]),
    # fastmax_hip_generate.h: generation through the attention block
    "fastmax_hip_p2_decode_step_qkv_supported": (ci, [ci, ci, ci, ci, ci]),
    "fastmax_hip_p2_decode_step_qkv": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp]),
    # fastmax_hip_linearmax_decode.h: the first-order linearmax decode state cache
    "fastmax_hip_linearmax_decode_state_bytes": (sz, [ci, ci, ci, ci]),
    "fastmax_hip_linearmax_decode_advance": (ci, QKV + [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    # fastmax_hip_block.h: the decoder block's neighbours of the attention sub-layer (RMSNorm with the residual add, the gated
    # activation of the MLP, and their backward passes)
    "fastmax_hip_rmsnorm_forward": (ci, [vp, i64, vp, i64, vp, vp, i64, vp, i64, vp, ci, ci, cf, ci, ci, ci, vp]),
    "fastmax_hip_rmsnorm_backward_workspace": (sz, [ci, ci, ci, ci]),
    "fastmax_hip_rmsnorm_backward": (ci, [vp, i64, vp, i64, vp, vp, vp, i64, vp, i64, vp, ci, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_gated_act_forward": (ci, [vp, i64, vp, i64, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_gated_act_backward": (ci, [vp, i64, vp, i64, vp, i64, vp, i64, vp, i64, ci, ci, ci, ci, vp]),
    # fastmax_hip_optim.h: the fused AdamW over the flat gradient bucket
    "fastmax_hip_adamw_workspace": (sz, [i64]),
    "fastmax_hip_adamw_chunk": (ci, []),
    "fastmax_hip_adamw_norm": (ci, [vp, ci, i64, cf, vp, sz, vp]),
    "fastmax_hip_adamw_update": (ci, [vp, ci, i64, vp, vp, vp, i64, vp, i64, vp, i64, cf, vp, cf, cf, cf, cf, cf, cf, cf, cf,
                                      ci, ci, ci, vp, sz, vp]),
    # fastmax_hip_next_token.h: last-row logits, exact top-k, seeded sampling
    "fastmax_hip_last_logits": (ci, [vp, i64, vp, i64, vp, i64, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_sample": (ci, [vp, i64, vp, ci, ci, ci, cf, i64, i64, vp]),
    "fastmax_hip_topk_mask": (ci, [vp, i64, vp, i64, ci, ci, ci, vp]),
    # fastmax_hip_neox.h: the NeoX (pythia) block's LayerNorm pair with the three-way residual add, the ungated GELU, their
    # backward passes
    "fastmax_hip_layernorm_forward": (ci, [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, vp, ci, ci, cf,
                                           ci, ci, vp]),
    "fastmax_hip_layernorm_backward_workspace": (sz, [ci, ci, ci, ci, ci]),
    "fastmax_hip_layernorm_backward": (ci, [vp, i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, ci, ci, ci,
                                            ci, vp, sz, vp]),
    "fastmax_hip_act_forward": (ci, [vp, i64, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_act_backward": (ci, [vp, i64, vp, i64, vp, i64, ci, ci, ci, ci, vp]),
    # fastmax_hip_cursor.h: position, draw number and output column of a generation loop in device memory (the feed at the
    # start of a step, the sampler at its end)
    "fastmax_hip_cursor_bytes": (sz, []),
    "fastmax_hip_cursor_feed": (ci, [vp, vp, vp, i64, i64, vp, i64, ci, ci, ci, vp, vp, i64, i64, vp, vp, ci, ci, vp]),
    "fastmax_hip_sample_cursor": (ci, [vp, i64, vp, vp, vp, i64, i64, vp, i64, ci, ci, ci, cf, vp]),
    # fastmax_hip_nucleus.h: the top-p filter behind the top-k in both samplers, and the mask that exposes its kept set
    "fastmax_hip_sample_nucleus": (ci, [vp, i64, vp, ci, ci, ci, cf, cf, i64, i64, vp]),
    "fastmax_hip_nucleus_mask": (ci, [vp, i64, vp, i64, ci, ci, ci, cf, cf, vp]),
    "fastmax_hip_sample_cursor_nucleus": (ci, [vp, i64, vp, vp, vp, i64, i64, vp, i64, ci, ci, ci, cf, cf, vp]),
    # fastmax_hip_moe.h: top-k routing with the stable dispatch, gather, combine and their backward passes
    "fastmax_hip_moe_route_workspace": (sz, [ci, ci]),
    "fastmax_hip_moe_route": (ci, [vp, i64, vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    "fastmax_hip_moe_gather": (ci, [vp, i64, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_moe_combine": (ci, [vp, i64, vp, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_moe_combine_backward": (ci, [vp, i64, vp, i64, vp, vp, vp, i64, vp, ci, ci, ci, ci, vp]),
    "fastmax_hip_moe_gather_backward": (ci, [vp, i64, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_moe_route_backward": (ci, [vp, vp, vp, vp, i64, ci, ci, ci, ci, vp]),
    # fastmax_hip_moe_decode.h: the experts' gated MLPs at M <= 16 tokens on the route kernel's device-side row counts, their
    # NF4 operands from a device table
    "fastmax_hip_moe_expert_entry_bytes": (sz, []),
    "fastmax_hip_moe_experts_up": (ci, [vp, i64, vp, vp, vp, vp, i64, ci, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_moe_experts_down": (ci, [vp, i64, vp, vp, vp, i64, ci, ci, ci, ci, ci, ci, vp]),
    # fastmax_hip_head.h: the last-row logits with an lm_head bias, and on packed NF4 codes
    "fastmax_hip_last_logits_bias": (ci, [vp, i64, vp, i64, vp, vp, i64, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_last_logits_nf4": (ci, [vp, i64, vp, vp, vp, vp, i64, ci, ci, ci, ci, ci, vp]),
    # fastmax_hip_adapter.h: adapter-v2 fine-tuning's per-column scale and bias behind a linear, forward and backward
    "fastmax_hip_adapter_forward": (ci, [vp, i64, vp, vp, vp, i64, ci, ci, ci, ci, vp]),
    "fastmax_hip_adapter_backward_workspace": (sz, [ci, ci, ci, ci]),
    "fastmax_hip_adapter_backward": (ci, [vp, i64, vp, i64, vp, vp, vp, i64, vp, vp, ci, ci, ci, ci, vp, sz, vp]),
    # fastmax_hip_kv_decode.h: the KV-cache decode route of fastmax blocks (csrc/fastmax_kv_decode.hip)
    "fastmax_hip_kv_decode_state_bytes": (sz, [ci, ci, ci, ci, ci]),
    "fastmax_hip_kv_decode_workspace": (sz, [ci, ci, ci, ci, ci, ci]),
    "fastmax_hip_kv_decode_load": (ci, [vp, i64p, vp, i64p, vp, ci, ci, ci, ci, ci, ci, vp]),
    "fastmax_hip_kv_decode_append_attend": (ci, QKV + [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, cf, vp, sz, vp]),
    "fastmax_hip_kv_decode_set_len": (ci, [vp, ci, ci, vp]),
}
SYMBOLS = list(ABI)

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m fastmax_experiments_amd.build` "
            "(hipcc, --offload-arch=gfx950). The fastmax operator has no fallback path.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        if not hasattr(L, name):
            raise RuntimeError(f"libfastmax_hip.so does not export {name}")
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.fastmax_hip_abi_version() != ABI_VERSION:
        raise RuntimeError("libfastmax_hip.so ABI version mismatch")
    _lib = L
    return L


def error_string(code):
    return lib().fastmax_hip_error_string(int(code)).decode()


def check(code, what):
    if code == OK:
        return
    if code == E_BAD_P:
        raise ValueError(f"{what}: {error_string(code)}")
    raise RuntimeError(f"{what} failed: rc={code} ({error_string(code)})")
