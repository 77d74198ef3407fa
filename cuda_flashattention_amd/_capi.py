"""ctypes binding of libfa2_mi355x.so -- the reference-side stub a maintainer would write to
call the C ABI of include/fa2_mi355x.h.

The library is built in-tree (cuda_flashattention_amd/lib/) by cuda_flashattention_amd/csrc/
Makefile.  There is NO fallback: if the shared object is missing or a symbol cannot be
resolved, importing this module raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FA2_LIB_PATH: load another build of the SAME library (A/B runs of kernel variants); never a fallback.
LIB_PATH = os.environ.get("FA2_LIB_PATH") or os.path.join(_HERE, "lib", "libfa2_mi355x.so")
RING_LIB_PATH = os.path.join(_HERE, "lib", "libfa2_ring_mi355x.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_mi355x.h")
KVCACHE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_kvcache_mi355x.h")
ROPE_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_rope_mi355x.h")
EXTEND_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_extend_mi355x.h")
EXTEND_RAGGED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_extend_ragged_mi355x.h")
ROPE_RAGGED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_rope_ragged_mi355x.h")
ROPE_NORM_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "fa2_rope_norm_mi355x.h")

FA2_OK = 0
FA2_DTYPE_BF16 = 0
FA2_DTYPE_F32 = 1
FA2_DTYPE_FP8_E4M3 = 2

_vp = ctypes.c_void_p
_i = ctypes.c_int
_f = ctypes.c_float
_sz = ctypes.c_size_t
_ll = ctypes.c_longlong

# name -> (restype, argtypes); mirrors include/fa2_mi355x.h declaration by declaration.
SIGNATURES = {
    "fa2_version": (ctypes.c_char_p, []),
    "fa2_status_string": (ctypes.c_char_p, [_i]),
    "flash_attention": (_i, [_vp] * 6 + [_i, _i, _i, _i]),
    "flash_attention_2_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f]),
    "flash_attention_2_backward": (_i, [_vp] * 9 + [_i, _i, _f]),
    "fa2_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "fa2_forward_fp8_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fa2_forward_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "fa2_forward_fp8_scaled": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _f, _f, _f, _i, _vp, _sz, _vp]),
    "fa2_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "fa2_backward": (_i, [_vp] * 9 + [_i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp]),
    "fa2_backward_plan": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_char_p)]),
    "fa2_backward_status": (_i, [_vp, _sz, _i, _i, _i, _i, _i, _vp]),
    "fa2_backward_phases": (_i, [_vp] * 9 + [_i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_forward_gqa": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "fa2_backward_gqa_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "fa2_backward_gqa": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_backward_gqa_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_char_p)]),
    "fa2_varlen_plan_bytes": (_sz, [_i, _i]),
    "fa2_varlen_plan_build": (_i, [_vp, _i, _vp, _sz]),
    "fa2_forward_varlen": (_i, [_vp] * 5 + [_i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp]),
    "fa2_backward_varlen_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "fa2_backward_varlen": (_i, [_vp] * 9 + [_i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "fa2_forward_qk": (_i, [_vp] * 5 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "fa2_backward_qk_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "fa2_backward_qk": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_varlen_plan_bytes_qk": (_sz, [_i, _i, _i]),
    "fa2_varlen_plan_build_qk": (_i, [_vp, _vp, _i, _vp, _sz]),
    "fa2_forward_varlen_qk": (_i, [_vp] * 5 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp]),
    "fa2_backward_varlen_qk_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "fa2_backward_varlen_qk": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "fa2_forward_sink": (_i, [_vp] * 6 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _vp]),
    "fa2_backward_sink_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "fa2_backward_sink": (_i, [_vp] * 11 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_forward_varlen_sink": (_i, [_vp] * 6 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp]),
    "fa2_backward_varlen_sink_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "fa2_backward_varlen_sink": (_i, [_vp] * 11 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "fa2_backward_lse": (_i, [_vp] * 12 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_backward_varlen_lse": (_i, [_vp] * 12 + [_i, _i, _i, _i, _i, _f, _i, _i, _vp, _vp, _sz, _vp, _sz, _vp]),
    "fa2_merge_states": (_i, [_vp, _vp, _i, _vp, _vp, _sz, _i, _i, _vp]),
    "fa2_merge_states_backward": (_i, [_vp] * 8 + [_i, _sz, _i, _i, _vp]),
    "fa2_decode_num_splits": (_i, [_i, _i, _i, _i]),
    "fa2_decode_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "fa2_forward_decode": (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _sz, _vp]),
    "fa2_forward_decode_paged": (_i, [_vp] * 8 + [_i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _vp, _sz, _vp]),
    "fa2_forward_decode_fp8kv": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp]),
    "fa2_forward_decode_paged_fp8kv": (_i, [_vp] * 10 + [_i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp]),
    "fa2_decode_window_num_splits": (_i, [_i, _i, _i, _i, _i, _i]),
    "fa2_forward_decode_window": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_forward_decode_paged_window": (_i, [_vp] * 10 + [_i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_backward_fused_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "fa2_backward_fused": (_i, [_vp] * 9 + [_i, _i, _i, _i, _f, _i, _vp, _sz, _vp]),
    "fa2_backward_block": (_i, [_vp] * 9 + [_i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_forward_step": (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _f, _i, _i, _i, _vp]),
    "fa2_forward_step_strided": (_i, [_vp] * 7 + [_i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "fa2_forward_state_finalize": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _vp]),
    "fa2_accumulate_bf16": (_i, [_vp, _vp, _sz, _i, _vp]),
    "fa2_accumulate_bf16_2d": (_i, [_vp, _vp, _sz, _sz, _sz, _i, _vp]),
    "fa2_read_clocks": (_i, [_vp, _vp]),
    "fa2_mfma_probe": (_i, [_vp, _vp, _i, _i, _vp]),
    "fa2_fill_f32": (_i, [_vp, _sz, _f, _vp]),
    "fa2_convert_f32_to_bf16": (_i, [_vp, _vp, _sz, _vp]),
    "fa2_convert_bf16_to_f32": (_i, [_vp, _vp, _sz, _vp]),
}

# include/fa2_kvcache_mi355x.h, the same library: a table of its own because SIGNATURES is pinned to fa2_mi355x.h (the C ABI is
# also linked against stub launchers, which have no kernels of this header's).
KVCACHE_SIGNATURES = {
    "fa2_kv_append": (_i, [_vp] * 7 + [_i] * 5 + [_ll] * 3 + [_i, _i, _vp]),
    "fa2_kv_append_paged": (_i, [_vp] * 8 + [_i] * 7 + [_ll] * 3 + [_i, _i, _vp]),
}

# include/fa2_rope_mi355x.h, the same library: the append with rotary embedding in front and the step's queries beside it.
ROPE_SIGNATURES = {
    "fa2_rope_kv_append": (_i, [_vp] * 11 + [_i] * 9 + [_ll] * 6 + [_i, _i, _vp]),
    "fa2_rope_kv_append_paged": (_i, [_vp] * 12 + [_i] * 11 + [_ll] * 6 + [_i, _i, _vp]),
}

# include/fa2_extend_mi355x.h, the same library: the decode calls for any number of query rows per K/V head (the arguments of
# fa2_forward_decode_window / _paged_window in their order).
EXTEND_SIGNATURES = {
    "fa2_extend_num_splits": (_i, [_i] * 7),
    "fa2_extend_workspace_bytes": (_sz, [_i] * 8),
    "fa2_forward_extend": SIGNATURES["fa2_forward_decode_window"],
    "fa2_forward_extend_paged": SIGNATURES["fa2_forward_decode_paged_window"],
}

# include/fa2_extend_ragged_mi355x.h, the same library: the extend calls with a q_len per sequence and token-major rows (the
# siblings' argument lists with total_q for q_len, q_token_stride behind Q, and plan, plan_bytes behind the caches or the table).
EXTEND_RAGGED_SIGNATURES = {
    "fa2_extend_ragged_max_blocks": (_ll, [_i] * 4),
    "fa2_extend_ragged_plan_bytes": (_sz, [_i] * 4),
    "fa2_extend_ragged_plan": (_i, [_vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "fa2_extend_ragged_num_splits": (_i, [_i] * 7),
    "fa2_extend_ragged_workspace_bytes": (_sz, [_i] * 8),
    "fa2_forward_extend_ragged": (_i, [_vp, _ll, _vp, _vp, _vp, _sz] + [_vp] * 6 + [_i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
    "fa2_forward_extend_ragged_paged": (_i, [_vp, _ll, _vp, _vp, _vp, _vp, _sz] + [_vp] * 6
                                        + [_i, _i, _i, _i, _i, _i, _i, _i, _f, _i, _i, _i, _i, _vp, _sz, _vp, _i]),
}

# include/fa2_rope_ragged_mi355x.h, the same library: the rotary append with an n_new per sequence and token-major tensors (the
# siblings' argument lists with plan, plan_bytes before seqlens_k, total_q for n_new, and two strides per source for three).
ROPE_RAGGED_SIGNATURES = {
    "fa2_rope_kv_append_ragged": (_i, [_vp] * 9 + [_sz] + [_vp] * 3 + [_i] * 9 + [_ll] * 4 + [_i, _i, _vp]),
    "fa2_rope_kv_append_ragged_paged": (_i, [_vp] * 10 + [_sz] + [_vp] * 3 + [_i] * 11 + [_ll] * 4 + [_i, _i, _vp]),
}

# include/fa2_rope_norm_mi355x.h, the same library: the ragged rotary append with a per-head RMSNorm of Q and K in front of the
# rotation (the siblings' argument lists with q_weight, k_weight, eps behind sin_table).
ROPE_NORM_SIGNATURES = {
    "fa2_norm_rope_kv_append_ragged": (_i, [_vp] * 10 + [_f, _vp, _sz] + [_vp] * 3 + [_i] * 9 + [_ll] * 4 + [_i, _i, _vp]),
    "fa2_norm_rope_kv_append_ragged_paged": (_i, [_vp] * 11 + [_f, _vp, _sz] + [_vp] * 3 + [_i] * 11 + [_ll] * 4 + [_i, _i, _vp]),
}


class FA2Error(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        try:
            msg = lib().fa2_status_string(status).decode()
        except Exception:  # pragma: no cover
            msg = "?"
        super().__init__(f"{where}: status {status} ({msg})")


_lib = None


def lib():
    """The loaded library.  import torch first in a torch process so that the HIP runtime the
    library binds (libamdhip64.so.7 by SONAME) is the one torch already loaded."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C cuda_flashattention_amd/csrc` "
                "(or python -c 'import __graft_entry__ as g; g.build()'). There is no fallback path.")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in (list(SIGNATURES.items()) + list(KVCACHE_SIGNATURES.items()) + list(ROPE_SIGNATURES.items())
                                  + list(EXTEND_SIGNATURES.items()) + list(EXTEND_RAGGED_SIGNATURES.items())
                                  + list(ROPE_RAGGED_SIGNATURES.items()) + list(ROPE_NORM_SIGNATURES.items())):
            fn = getattr(handle, name)   # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status, where):
    if status != FA2_OK:
        raise FA2Error(status, where)
