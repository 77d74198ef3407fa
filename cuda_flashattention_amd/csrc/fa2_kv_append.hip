// fa2_kv_append.hip -- the KV-cache append (fa2_kv_append, fa2_kv_append_paged; include/fa2_kvcache_mi355x.h): writes the
// n_new newest tokens' K and V of every sequence into the caches the decode kernels of fa2_decode.hip read, contiguous
// [B][H_kv][N_cap][d] or a pool of pages [n_pages][H_kv][page_size][d] behind a block table, in bf16 (the source bits) or OCP e4m3
// (clamp(x / descale[h], +-448), round to nearest even).  ONE launch covers K and V.
//
// WORK SPLIT.  A row of d elements is d / 8 lanes of 16 source bytes, so a wave holds 64 / (d / 8) rows (4 at d = 128, 8 at
// d = 64) per pass and makes kKvPasses passes per unit.  A unit is (sequence b, K/V head h, a group of kKvPasses x rows tokens):
// b and h are WAVE-UNIFORM, so seqlens_k[b], k_descale[h] and v_descale[h] are scalar loads, once per unit; a row's table entry
// is one load per row (its lanes read one address).  Units are dealt to the waves of a grid that depends on host values only
// and is capped (kKvMaxBlocks); a wave strides over the rest.  Plain compiler code: no LDS, no atomics, no inline assembly, no
// communication between workgroups; every byte written is a function of the inputs alone.
// ADDRESSES.  A destination is formed by fa2_kv_append_addr.h and nothing else: a token is written iff its row passes
// 0 <= pos < capacity (and, paged, its table entry lies inside the pool); every other token is skipped, source load included.
// No loop bound comes from device memory.  Source rows are read only for t < n_new, through the caller's three strides.
// E4M3.  The quantiser is fa2_kv_quantise.h's, shared with fa2_rope_append.hip.
#include "fa2_common.h"
#include "fa2_kv_append_addr.h"
#include "fa2_kv_quantise.h"
#include "fa2_kvcache_mi355x.h"
#include "fa2_launch.h"

#include <algorithm>

namespace fa2 {

namespace {

constexpr int kKvPasses = 2;           // rows of a lane per unit: both passes' loads are issued before the first store
constexpr int kKvMaxBlocks = 2048;     // 256 CUs x 8 workgroups of 4 waves: a memory-bound grid is capped and strides
// what a wave reads once per unit, at a wave-uniform address: the constant address space makes these scalar loads
typedef __attribute__((address_space(4))) int kv_const_int;
typedef __attribute__((address_space(4))) float kv_const_float;

struct KvAppendArgs {
    const void* Knew; const void* Vnew; void* K; void* V;
    const int* seqlens; const int* block_table; const float* k_descale; const float* v_descale;
    int B, Hkv, n_new, Ncap;                     // Ncap: kv_capacity, or max_pages x page_size
    int n_pages, page_size, max_pages;           // paged only
    long long sb, sh, st;                        // the source's element strides: batch, head, token
};

template <int D, bool FP8, bool PAGED>
__global__ __launch_bounds__(256) void fa2_kv_append_kernel(const KvAppendArgs a)
{
    constexpr int LPR = D / 8;                  // lanes of a row
    constexpr int ROWS = 64 / LPR;              // rows of a wave's pass
    constexpr int TPU = ROWS * kKvPasses;       // tokens of a unit
    const int lane = threadIdx.x & 63;
    const int r = lane / LPR, c = lane % LPR;
    const unsigned groups = ((unsigned)a.n_new + TPU - 1) / TPU;
    const unsigned long long units = (unsigned long long)a.B * a.Hkv * groups;      // host values: below 2^31 (kv_append_check)
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const unsigned long long step = (unsigned long long)gridDim.x * 4u;
    for (unsigned long long u64 = wave; u64 < units; u64 += step) {
        const unsigned u = (unsigned)u64;
        const int g = (int)(u % groups), bh = (int)(u / groups);
        const int h = bh % a.Hkv, b = bh / a.Hkv;
        const int len = ((const kv_const_int*)a.seqlens)[b];
        float kd = 1.0f, vd = 1.0f;
        if constexpr (FP8) {
            if (a.k_descale) kd = ((const kv_const_float*)a.k_descale)[h];
            if (a.v_descale) vd = ((const kv_const_float*)a.v_descale)[h];
        }
        long long dst[kKvPasses];
        u32x4 k[kKvPasses], v[kKvPasses];
#pragma unroll
        for (int p = 0; p < kKvPasses; ++p) {
            const unsigned t = (unsigned)g * TPU + p * ROWS + r;      // unsigned: the last group may pass n_new, up to INT_MAX, by TPU - 1
            dst[p] = kKvAppendDropped;
            if (t < (unsigned)a.n_new) {
                const int pos = kv_append_pos(len, a.n_new, (int)t, a.Ncap);
                if constexpr (PAGED) {
                    if (pos >= 0) {
                        const int entry = a.block_table[(long long)b * a.max_pages + kv_append_table_index(pos, a.page_size)];
                        dst[p] = kv_append_offset_paged(pos, entry, a.n_pages, h, a.Hkv, a.page_size, D);
                    }
                } else {
                    dst[p] = kv_append_offset(pos, b, h, a.Hkv, a.Ncap, D);
                }
            }
            if (dst[p] >= 0) {
                const long long src = (long long)b * a.sb + (long long)h * a.sh + (long long)t * a.st + 8 * c;
                k[p] = *reinterpret_cast<const u32x4*>((const __bf16*)a.Knew + src);
                v[p] = *reinterpret_cast<const u32x4*>((const __bf16*)a.Vnew + src);
            }
        }
#pragma unroll
        for (int p = 0; p < kKvPasses; ++p) {
            if (dst[p] < 0) continue;
            const long long at = dst[p] + 8 * c;
            if constexpr (FP8) {
                *reinterpret_cast<u32x2*>((uint8_t*)a.K + at) = kv_quantise8(k[p], kd);
                *reinterpret_cast<u32x2*>((uint8_t*)a.V + at) = kv_quantise8(v[p], vd);
            } else {
                *reinterpret_cast<u32x4*>((__bf16*)a.K + at) = k[p];
                *reinterpret_cast<u32x4*>((__bf16*)a.V + at) = v[p];
            }
        }
    }
}

template <int D, bool FP8, bool PAGED>
hipError_t kv_append_launch(const KvAppendArgs& a, hipStream_t stream)
{
    constexpr int TPU = 64 / (D / 8) * kKvPasses;
    const long long units = (long long)a.B * a.Hkv * (((long long)a.n_new + TPU - 1) / TPU);
    const unsigned grid = (unsigned)std::min<long long>((units + 3) / 4, kKvMaxBlocks);
    hipLaunchKernelGGL((fa2_kv_append_kernel<D, FP8, PAGED>), dim3(grid), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <bool PAGED>
hipError_t kv_append_dispatch(const KvAppendArgs& a, int d, bool fp8, hipStream_t stream)
{
    if (d == 128) return fp8 ? kv_append_launch<128, true, PAGED>(a, stream) : kv_append_launch<128, false, PAGED>(a, stream);
    if (d == 64) return fp8 ? kv_append_launch<64, true, PAGED>(a, stream) : kv_append_launch<64, false, PAGED>(a, stream);
    return hipErrorInvalidValue;
}

inline int kv_hip_status(hipError_t e) { return e == hipSuccess ? FA2_OK : FA2_ERR_HIP_BASE - (int)e; }

inline bool kv_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// Everything both entry points check after their NULL pointers and their own capacity rules, in the header's order.
int kv_append_check(const void* K_new, const void* V_new, const void* K, const void* V, const float* k_descale,
                    const float* v_descale, int B, int H_kv, int n_new, int head_dim, long long sb, long long sh, long long st,
                    int dtype, int kv_dtype)
{
    const long long heads = (long long)B * H_kv;                                           // the units are counted in 32 bits
    if (heads > 0x7fffffffLL || heads * n_new > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (sb < 0 || sh < 0 || st < 0 || sb % 8 || sh % 8 || st % 8) return FA2_ERR_INVALID_SHAPE;
    if (kv_misaligned(K_new) || kv_misaligned(V_new) || kv_misaligned(K) || kv_misaligned(V)) return FA2_ERR_INVALID_SHAPE;
    if (head_dim != 64 && head_dim != 128) return FA2_ERR_UNSUPPORTED_HEAD_DIM;
    if (dtype != FA2_DTYPE_BF16) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype != FA2_DTYPE_BF16 && kv_dtype != FA2_DTYPE_FP8_E4M3) return FA2_ERR_UNSUPPORTED_DTYPE;
    if (kv_dtype == FA2_DTYPE_BF16 && (k_descale || v_descale)) return FA2_ERR_UNSUPPORTED;
    return FA2_OK;
}

}  // namespace

}  // namespace fa2

extern "C" {

int fa2_kv_append(const void* K_new, const void* V_new, void* K_cache, void* V_cache,
                  const int* seqlens_k, const float* k_descale, const float* v_descale,
                  int B, int H_kv, int n_new, int kv_capacity, int head_dim,
                  long long new_stride_b, long long new_stride_h, long long new_stride_t,
                  int dtype, int kv_dtype, void* stream)
{
    if (!K_new || !V_new || !K_cache || !V_cache || !seqlens_k) return FA2_ERR_NULL_POINTER;
    if (B <= 0 || H_kv <= 0 || n_new <= 0 || kv_capacity <= 0 || head_dim <= 0) return FA2_ERR_INVALID_SHAPE;
    // the decode calls' (b, head) slab limit: 2 bytes per element, 1 in an e4m3 cache
    if ((long long)kv_capacity * head_dim * (kv_dtype == FA2_DTYPE_FP8_E4M3 ? 1 : 2) > 0x7fffffffLL) return FA2_ERR_INVALID_SHAPE;
    if (const int st = fa2::kv_append_check(K_new, V_new, K_cache, V_cache, k_descale, v_descale, B, H_kv, n_new, head_dim,
                                            new_stride_b, new_stride_h, new_stride_t, dtype, kv_dtype))
        return st;
    fa2::KvAppendArgs a{};
    a.Knew = K_new; a.Vnew = V_new; a.K = K_cache; a.V = V_cache; a.seqlens = seqlens_k;
    a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hkv = H_kv; a.n_new = n_new; a.Ncap = kv_capacity;
    a.sb = new_stride_b; a.sh = new_stride_h; a.st = new_stride_t;
    return fa2::kv_hip_status(fa2::kv_append_dispatch<false>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, (hipStream_t)stream));
}

int fa2_kv_append_paged(const void* K_new, const void* V_new, void* K_pages, void* V_pages,
                        const int* block_table, const int* seqlens_k,
                        const float* k_descale, const float* v_descale,
                        int B, int H_kv, int n_new, int n_pages, int page_size,
                        int max_pages_per_seq, int head_dim,
                        long long new_stride_b, long long new_stride_h, long long new_stride_t,
                        int dtype, int kv_dtype, void* stream)
{
    if (!K_new || !V_new || !K_pages || !V_pages || !seqlens_k || !block_table) return FA2_ERR_NULL_POINTER;
    if (B <= 0 || H_kv <= 0 || n_new <= 0 || n_pages <= 0 || page_size <= 0 || max_pages_per_seq <= 0 || head_dim <= 0)
        return FA2_ERR_INVALID_SHAPE;
    if (page_size % fa2::kDecodeTile) return FA2_ERR_INVALID_SHAPE;
    // the paged decode's capacity limit: what this call writes, that call must be able to read
    if ((long long)max_pages_per_seq * page_size > 0x7fffffffLL - (fa2::kDecodeMaxSplits + 2) * fa2::kDecodeKB) return FA2_ERR_INVALID_SHAPE;
    if (const int st = fa2::kv_append_check(K_new, V_new, K_pages, V_pages, k_descale, v_descale, B, H_kv, n_new, head_dim,
                                            new_stride_b, new_stride_h, new_stride_t, dtype, kv_dtype))
        return st;
    fa2::KvAppendArgs a{};
    a.Knew = K_new; a.Vnew = V_new; a.K = K_pages; a.V = V_pages; a.seqlens = seqlens_k; a.block_table = block_table;
    a.k_descale = k_descale; a.v_descale = v_descale;
    a.B = B; a.Hkv = H_kv; a.n_new = n_new; a.Ncap = max_pages_per_seq * page_size;
    a.n_pages = n_pages; a.page_size = page_size; a.max_pages = max_pages_per_seq;
    a.sb = new_stride_b; a.sh = new_stride_h; a.st = new_stride_t;
    return fa2::kv_hip_status(fa2::kv_append_dispatch<true>(a, head_dim, kv_dtype == FA2_DTYPE_FP8_E4M3, (hipStream_t)stream));
}

}  // extern "C"
