// sage_mla_cache.hip -- the appendable quantised latent of the absorbed MLA decode route (include/sage_mlacache_gfx950.h),
// gfx950: rows appended in place to the operands of sage_mla_attn / sage_mlasplit_attn, with the K mean and the V abs-max frozen at seeding
// time.
//
// Replaces in the reference: nothing.
//
// With frozen statistics a row's INT8 bytes depend on its 64-key tile alone (the per-thread scale groups are local to a tile) and its e4m3 bytes
// on the row alone, so an append re-forms the tiles that receive a row and nothing else.  Only the OPEN tile -- the one a sample's next row
// goes to -- holds rows from an earlier append; its group abs-maxima run over valid rows only and change as it grows, so its raw rows are kept
// (tail [B, 64, 576]) and it is re-quantised from them each time.  The arithmetic is the pre-pass's own text (sage_mla_block.h).
//
//   mlacache_append_kernel   grid (ceil((63 + T) / 64), B), 256 threads.  Workgroup (j, b) owns tile lens[b] / 64 + j and leaves if the tile
//                            receives no row.  Row r of the tile comes from the tail if it lies in front of lens[b] (only j = 0 has such rows)
//                            and from kv_new otherwise, by 16-byte loads.  K: thread = (row, quarter) holds 144 channels in registers, the row
//                            abs-max by two __shfl_xor, the four group scales through LDS, nine 16-byte stores per thread.  V: e4m3 bytes
//                            scattered into the 32-KiB image in LDS, zeros behind the last valid token, copied out in 16-byte stores.  j = 0
//                            writes v_scale = v_amax / 448 on every call, rows or none.
//   mlacache_commit_kernel   grid (B).  The rows of the NEW open tile that came from kv_new go to the tail; behind a __syncthreads() one thread
//                            stores lens[b].
//   mlacache_stats_kernel, mlacache_fold_kernel   the pre-pass's statistics launch and its fold on a prompt, publishing the 512 FP32 maxima.
//
// Ordering.  Launch 1 reads lens and the tail and writes the images, k_scale and v_scale; no two of its workgroups own the same tile, so no two
// write the same byte.  Launch 2 alone writes the tail and lens; workgroup b alone touches sample b's, every thread of it has read lens[b]
// before the barrier in front of the one store to it, and stream order puts the launch behind every read of launch 1 and in front of the next
// call's.  No atomics, no host read: the grids follow from B, T and the capacity.
#include "../../include/sage_mlacache_gfx950.h"
#include "sage_mla.h"
#include "sage_mla_block.h"
#include "sage_host_checks.h"

namespace sage {

struct MlaCacheParams {
    const uint16_t *kv_new;         // [B, T, 576] behind element strides
    const int32_t *new_lens;        // nullable: every sample takes T rows
    int32_t *lens;                  // [B]
    uint16_t *tail;                 // [B, 64, 576]: the raw rows of the open tile
    const uint16_t *k_mean;         // [B, 576], input dtype
    const float *v_amax;            // [B, 512]
    unsigned char *k_img, *v_img;
    float *k_scale, *v_scale;
    long kvn_sb, kvn_sl;
    int B, T, cap, ntile, smooth_k;
};

// sample b's rows before the call and the rows it takes: new_lens clamped to [0, T], then to what the capacity leaves
__device__ __forceinline__ void mlacache_range(const MlaCacheParams &p, int b, int &len0, int &t)
{
    len0 = mla_kv_len(p.lens, b, p.cap);
    t = p.new_lens != nullptr ? p.new_lens[b] : p.T;
    t = t < 0 ? 0 : (t > p.T ? p.T : t);
    t = t > p.cap - len0 ? p.cap - len0 : t;
}

template <int DT>
__global__ void __launch_bounds__(256) mlacache_append_kernel(const MlaCacheParams p)
{
    __shared__ MlaTileLds s;
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    int len0, t;
    mlacache_range(p, b, len0, t);
    const float *v_amax = p.v_amax + (long)b * MLA_DV;
    // the scales of the frozen abs-max (every call: the same bytes; a sample that never gets a row has them too)
    if (j == 0)
        for (int d = tid; d < MLA_DV; d += 256) p.v_scale[(long)b * MLA_DV + d] = v_amax[d] / 448.0f;
    const int len1 = len0 + t;                          // <= cap
    const int tile = len0 / BLKK + j, row0 = tile * BLKK;
    if (t == 0 || row0 >= len1) return;                 // (workgroup-uniform) no new row for this tile; row0 < len1 <= cap: the tile exists
    const int old = len0 - row0;                        // rows r < old of the tile are the tail's (j = 0 only), the rest kv_new's
    const uint16_t *tail = p.tail + (long)b * BLKK * MLA_DQK;
    const uint16_t *fresh = p.kv_new + (long)b * p.kvn_sb + (long)(row0 - len0) * p.kvn_sl;      // row r of the tile, r >= old
    const long kvn_sl = p.kvn_sl;
    auto row_of = [=](int r) { return r < old ? tail + r * MLA_DQK : fresh + (long)r * kvn_sl; };
    const long bt = (long)b * p.ntile + tile;
    mla_tile_constants<DT>(s, p.k_mean + (long)b * MLA_DQK, v_amax, tid);
    __syncthreads();
    mla_quant_k_tile<DT>(s, row_of, len1 - row0, p.smooth_k != 0, p.k_img + bt * MLA_K_TILE_BYTES, p.k_scale + bt * 4, tid);
    mla_quant_v_tile<DT, true>(s, row_of, len1 - row0, p.v_img + bt * MLA_V_TILE_BYTES, tid);
}

// launch 2: the raw rows of the tile the NEXT append opens, then the new length
__global__ void __launch_bounds__(256) mlacache_commit_kernel(const MlaCacheParams p)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    int len0, t;
    mlacache_range(p, b, len0, t);
    const int len1 = len0 + t;
    const int open0 = len1 / BLKK * BLKK;               // first row of the open tile
    const int lo = len0 > open0 ? len0 : open0;         // its rows lo .. len1 - 1 are new; those in front of lo (same tile as before) are in the tail
    const int n = len1 - lo;                            // 0 .. 63
    const uint16_t *src = p.kv_new + (long)b * p.kvn_sb + (long)(lo - len0) * p.kvn_sl;
    uint16_t *dst = p.tail + ((long)b * BLKK + (lo - open0)) * MLA_DQK;
    for (int piece = tid; piece < n * (MLA_DQK / 8); piece += 256) {
        const int r = piece / (MLA_DQK / 8), c8 = (piece % (MLA_DQK / 8)) * 8;
        *reinterpret_cast<v4u *>(dst + r * MLA_DQK + c8) = *reinterpret_cast<const v4u *>(src + (long)r * p.kvn_sl + c8);
    }
    __syncthreads();                                    // every thread has read lens[b]
    if (tid == 0) p.lens[b] = len1;
}

template <int DT>
__global__ void __launch_bounds__(MLA_STATS_THREADS) mlacache_stats_kernel(const MlaPrepParams p)
{
    __shared__ float red_k[MLA_STATS_RG][MLA_DQK], red_v[MLA_STATS_RG][MLA_DV];
    mla_stats_chunk<DT>(p, blockIdx.x, blockIdx.y, threadIdx.x, red_k, red_v);
}

// the fold, with the maxima themselves published (p.v_scale carries v_amax here)
template <int DT>
__global__ void __launch_bounds__(MLA_DQK) mlacache_fold_kernel(const MlaPrepParams p)
{
    const int b = blockIdx.x, tid = threadIdx.x;        // thread = channel
    const float a = mla_fold_channel<DT>(p, b, tid);
    if (tid < MLA_DV) p.v_scale[(long)b * MLA_DV + tid] = a;
}

static hipError_t launch_mlacache_stats(const MlaPrepParams &p, int dtype, hipStream_t stream)
{
    const dim3 g1(p.nchunk, p.B), g2(p.B);
    if (dtype == DT_F16) {
        hipLaunchKernelGGL(mlacache_stats_kernel<DT_F16>, g1, dim3(MLA_STATS_THREADS), 0, stream, p);
        hipLaunchKernelGGL(mlacache_fold_kernel<DT_F16>, g2, dim3(MLA_DQK), 0, stream, p);
    } else {
        hipLaunchKernelGGL(mlacache_stats_kernel<DT_BF16>, g1, dim3(MLA_STATS_THREADS), 0, stream, p);
        hipLaunchKernelGGL(mlacache_fold_kernel<DT_BF16>, g2, dim3(MLA_DQK), 0, stream, p);
    }
    return hipGetLastError();
}

static hipError_t launch_mlacache_append(const MlaCacheParams &p, int dtype, hipStream_t stream)
{
    const dim3 grid((63 + p.T + BLKK - 1) / BLKK, p.B);
    if (dtype == DT_F16) hipLaunchKernelGGL(mlacache_append_kernel<DT_F16>, grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(mlacache_append_kernel<DT_BF16>, grid, dim3(256), 0, stream, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(mlacache_commit_kernel, dim3(p.B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

static bool aligned2(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 1u) == 0; }

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_MLACACHE_API int sage_mlacache_abi_version(void) { return SAGE_MLACACHE_ABI_VERSION; }

SAGE_MLACACHE_API int sage_mlacache_stats(const void *kv, const int32_t *kv_lens, void *k_mean, float *v_amax, float *ws, int64_t ws_floats,
                                          int B, int Lk, int64_t kv_sb, int64_t kv_sl, int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_mlacache_stats";
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && Lk >= 1, "%s: empty problem (B %d, Lk %d)", e, B, Lk);
    SAGE_REQUIRE(kv && k_mean && v_amax && ws, "%s: null pointer (only kv_lens may be null)", e);
    SAGE_REQUIRE(aligned16_strides(kv, 8, kv_sb, kv_sl) && kv_sb >= 0 && kv_sl >= MLA_DQK,
                 "%s: kv must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 576", e);
    SAGE_REQUIRE(aligned4(v_amax) && aligned4(ws) && aligned4(kv_lens) && aligned2(k_mean),
                 "%s: v_amax, ws and kv_lens must be 4-byte aligned, k_mean 2-byte", e);
    const int64_t need = (int64_t)B * mla_ws_per_sample((Lk + MLA_CHUNK - 1) / MLA_CHUNK);
    SAGE_REQUIRE(ws_floats >= need, "%s: ws holds %lld floats, sage_mla_ws_floats(B, Lk) = %lld", e, (long long)ws_floats, (long long)need);
    SAGE_REQUIRE(B <= 65535, "%s: B must be at most 65535 (got %d)", e, B);
    MlaPrepParams p{};
    p.kv = kv; p.kv_lens = kv_lens; p.k_mean = k_mean; p.v_scale = v_amax; p.ws = ws;
    p.kv_sb = kv_sb; p.kv_sl = kv_sl;
    p.B = B; p.Lk = Lk; p.ntile = (Lk + BLKK - 1) / BLKK; p.nchunk = (Lk + MLA_CHUNK - 1) / MLA_CHUNK; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_mlacache_stats(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

SAGE_MLACACHE_API int sage_mlacache_append(const void *kv_new, const int32_t *new_lens, int32_t *lens, void *tail, const void *k_mean,
                                           const float *v_amax, void *k_image, float *k_scale, void *v_image, float *v_scale, int B, int T,
                                           int capacity, int64_t kvn_sb, int64_t kvn_sl, int smooth_k, int dtype, void *stream)
{
    const char *const e = "sage_mlacache_append";
    SAGE_REQUIRE(dtype == DT_F16 || dtype == DT_BF16, "%s: dtype must be SAGE_DTYPE_F16 (0) or SAGE_DTYPE_BF16 (1) (got %d)", e, dtype);
    SAGE_REQUIRE(B >= 1 && T >= 1 && capacity >= 1, "%s: empty problem (B %d, T %d, capacity %d)", e, B, T, capacity);
    SAGE_REQUIRE(kv_new && lens && tail && k_mean && v_amax && k_image && k_scale && v_image && v_scale,
                 "%s: null pointer (only new_lens may be null)", e);
    SAGE_REQUIRE(aligned16_strides(kv_new, 8, kvn_sb, kvn_sl) && kvn_sb >= 0 && kvn_sl >= MLA_DQK,
                 "%s: kv_new must be 16-byte aligned with non-negative strides in multiples of 8 elements and a token stride of at least 576", e);
    SAGE_REQUIRE(aligned16(tail) && aligned16(k_image) && aligned16(v_image) && aligned4(k_scale) && aligned4(v_scale) && aligned4(v_amax) &&
                     aligned4(lens) && aligned4(new_lens) && aligned2(k_mean),
                 "%s: tail and the images must be 16-byte aligned, k_scale, v_scale, v_amax, lens and new_lens 4-byte, k_mean 2-byte", e);
    SAGE_REQUIRE(B <= 65535 && T <= (1 << 30) && capacity <= (1 << 30),
                 "%s: B must be at most 65535, T and capacity at most 2^30 (got %d, %d and %d)", e, B, T, capacity);
    MlaCacheParams p{};
    p.kv_new = static_cast<const uint16_t *>(kv_new); p.new_lens = new_lens; p.lens = lens;
    p.tail = static_cast<uint16_t *>(tail); p.k_mean = static_cast<const uint16_t *>(k_mean); p.v_amax = v_amax;
    p.k_img = static_cast<unsigned char *>(k_image); p.v_img = static_cast<unsigned char *>(v_image);
    p.k_scale = k_scale; p.v_scale = v_scale;
    p.kvn_sb = kvn_sb; p.kvn_sl = kvn_sl;
    p.B = B; p.T = T; p.cap = capacity; p.ntile = (capacity + BLKK - 1) / BLKK; p.smooth_k = smooth_k != 0;
    const hipError_t err = launch_mlacache_append(p, dtype, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
