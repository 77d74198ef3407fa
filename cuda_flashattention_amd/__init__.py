"""MI355X-native FlashAttention-2 hot path (fwd / bwd / ring) behind the reference's own
host-wrapper interface.  HIP kernels + C ABI live in csrc/ (libfa2_mi355x.so); this package
is the thin host-side mirror used by tests and bench.py.  No CPU fallback exists."""
from . import _capi  # noqa: F401
from .ops import flash_attention_2_forward, flash_attention_2_backward, forward_step, attention  # noqa: F401
from .ops import VarlenPlan, flash_attention_2_varlen_forward, flash_attention_2_varlen_backward, attention_varlen  # noqa: F401
from .ops import flash_attention_2_qk_forward, flash_attention_2_qk_backward, attention_qk  # noqa: F401
from .ops import flash_attention_2_decode, decode_num_splits, decode_workspace  # noqa: F401
from .ops import flash_attention_2_decode_paged  # noqa: F401
from .ops import flash_attention_2_extend, flash_attention_2_extend_paged, extend_num_splits, extend_workspace  # noqa: F401
from .ops import flash_attention_2_extend_ragged, flash_attention_2_extend_ragged_paged  # noqa: F401
from .ops import ExtendRaggedPlan, extend_ragged_plan, extend_ragged_num_splits, extend_ragged_workspace  # noqa: F401
from .ops import kv_cache_append, kv_cache_append_paged  # noqa: F401
from .ops import rope_kv_cache_append, rope_kv_cache_append_paged  # noqa: F401
from .ops import rope_kv_cache_append_ragged, rope_kv_cache_append_ragged_paged  # noqa: F401
from .ops import norm_rope_kv_cache_append_ragged, norm_rope_kv_cache_append_ragged_paged  # noqa: F401
from .ops import kv_cache_append_ragged, kv_cache_append_ragged_paged  # noqa: F401
from .ops import merge_states_forward,merge_states_backward, merge_attention_states, attention_segments  # noqa: F401
