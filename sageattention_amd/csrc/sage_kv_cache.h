// sage_kv_cache.h -- what the appendable cache's two translation units share: the parameter block of its launches and the row range of an append
// (sage_kv_cache.hip: the contiguous cache and the commit launch; sage_kv_paged.hip: the paged pool's append and its C entry points -- a unit of
// its own because kernels added to sage_kv_cache.hip changed the register numbering of the D = 64 kernels already there).
#pragma once
#include "sage_common.h"
#include "sage_kernels.h"

namespace sage {

struct KvCacheParams {
    int8_t *k_int8;             // [B,H,cap,D]
    float *k_scale;             // [B,H,cap/64*4]
    unsigned char *v_image;     // [B,H,cap/64,D,64]
    float *v_scale;             // [B,H,D]
    const float *v_amax;        // [B,H,D]
    const uint16_t *k_mean;     // nullable [B,H,D]
    uint16_t *k_tail, *v_tail;  // [B,H,64,D]
    int32_t *lens;              // [B]
    const uint16_t *k_new, *v_new;   // [B,H,T,D], strides below
    const int32_t *new_lens;    // nullable [B]
    int B, H, cap, T, D;
    long k_sb, k_sh, k_sl;
    long v_sb, v_sh, v_sl;
    float scale_max;            // 448 (e4m3)
};

// rows sample b holds (clamped to [0, cap]) and rows this call gives it: clamped to [0, T], then to what still fits
__device__ __forceinline__ void append_range(const KvCacheParams &p, int b, int &len0, int &t)
{
    const int l = p.lens[b];
    len0 = l < 0 ? 0 : (l > p.cap ? p.cap : l);
    int n = p.new_lens != nullptr ? p.new_lens[b] : p.T;
    n = n < 0 ? 0 : (n > p.T ? p.T : n);
    t = n < p.cap - len0 ? n : p.cap - len0;
}

// launch 2 of an append (sage_kv_cache.hip): the tails and the lengths, per sample -- the same launch for the contiguous cache and the paged pool
hipError_t launch_kvcache_commit(const KvCacheParams &p, hipStream_t s);

}  // namespace sage
