// sage_kv_fork.hip -- the fork of sequences of the paged quantised KV cache (include/sage_kvfork_gfx950.h): the child's table names the
// parent's closed pages, the parent's open page is copied into a page of the child's own, the child takes the parent's per-slot state.  A unit
// of its own (kernels added to sage_kv_cache.hip / sage_kv_paged.hip renumber the registers of the ones there); copies only, no arithmetic.
//
// Replaces in the reference: nothing (no KV cache there).
//
// One launch, grid (tiles per page + 1, Hkv, n), 256 threads.  Workgroup (j, h, i) with j < tiles per page copies tile j of head h of the open
// page, if the prefix reaches it; the last j copies head h's per-slot state and, for h == 0, the table row and the length.  No workgroup depends
// on another: what a workgroup reads (the source's length, table row, state and pages) no workgroup of a call that keeps the contract writes,
// and each writes bytes no other workgroup touches.  Every id read from memory is checked before it forms an address.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvfork_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_kv_cache.h"

namespace sage {

struct KvForkParams {
    int8_t *k_int8;             // the pool: [num_pages,H,ps,D]
    float *k_scale;             // [num_pages,H,ps/64*4]
    unsigned char *v_image;     // [num_pages,H,ps/64,D,64]
    float *v_scale, *v_amax;    // [B,H,D]
    uint16_t *k_mean;           // nullable [B,H,D]
    uint16_t *k_tail, *v_tail;  // [B,H,64,D]
    int32_t *lens;              // [B]
    int32_t *block_table;       // [B,max_pages], row stride bt_stride
    long bt_stride;
    int page_shift, num_pages, max_pages;
    int B, H, cap;              // cap = max_pages * (64 << page_shift)
    const int32_t *src_slots, *dst_slots, *new_pages;   // [n]
    const int32_t *prefix_lens; // nullable [n]
};

// `chunks` 16-byte pieces from src to dst (both 16-byte aligned), spread over the workgroup
__device__ __forceinline__ void copy16(void *dst, const void *src, int chunks, int tid)
{
    const v4u *s = static_cast<const v4u *>(src);
    v4u *d = static_cast<v4u *>(dst);
    for (int c = tid; c < chunks; c += 256) d[c] = s[c];
}

template <int D>
__global__ void __launch_bounds__(256)
kvpaged_fork_kernel(const KvForkParams p)
{
    const int tid = threadIdx.x;
    const int j = blockIdx.x, h = blockIdx.y, i = blockIdx.z;
    const int tiles = 1 << p.page_shift;        // 64-key tiles per page (= gridDim.x - 1)
    // (wave-uniform addresses: scalar loads, as p.lens[b] in sage_kv_append_body.h)
    const int s = p.src_slots[i], d = p.dst_slots[i];
    if (s < 0 || s >= p.B || d < 0 || d >= p.B || s == d) return;          // the fork is skipped entirely
    const int l = p.lens[s];
    const int L = l < 0 ? 0 : (l > p.cap ? p.cap : l);
    int P = L;
    if (p.prefix_lens != nullptr) {
        const int w = p.prefix_lens[i];
        P = w < 0 ? 0 : (w > L ? L : w);
        if (P < L) P &= ~(BLKK - 1);            // a prefix shorter than the parent ends on a block boundary
    }
    const int np = P >> (6 + p.page_shift);     // whole pages shared
    const int r = P & ((BLKK << p.page_shift) - 1);     // keys in the open page; r > 0 implies np * ps < P <= cap: np < max_pages
    const int pg = p.new_pages[i];

    if (j < tiles) {
        // ---- copy-on-write: tile j of head h of the open page
        if (j * BLKK >= r) return;
        const int sp = p.block_table[(long)s * p.bt_stride + np];
        if (sp < 0 || sp >= p.num_pages || pg < 0 || pg >= p.num_pages) return;       // not pages of the pool: nothing of the pool is written
        const long src = (((long)sp * p.H + h) << p.page_shift) + j;     // the tile's index among the 64-row blocks of the pool
        const long dst = (((long)pg * p.H + h) << p.page_shift) + j;
        copy16(p.k_int8 + dst * (BLKK * D), p.k_int8 + src * (BLKK * D), BLKK * D / 16, tid);
        copy16(p.v_image + dst * (D * 64), p.v_image + src * (D * 64), D * 64 / 16, tid);
        copy16(p.k_scale + dst * 4, p.k_scale + src * 4, 1, tid);
        return;
    }

    // ---- the per-slot state of head h
    const long from = ((long)s * p.H + h) * D, to = ((long)d * p.H + h) * D;
    if (tid < D) {
        p.v_scale[to + tid] = p.v_scale[from + tid];
        p.v_amax[to + tid] = p.v_amax[from + tid];
    }
    if (p.k_mean != nullptr) copy16(p.k_mean + to, p.k_mean + from, D / 8, tid);
    const int open = P & (BLKK - 1);            // raw rows of the open block
    copy16(p.k_tail + to * BLKK, p.k_tail + from * BLKK, open * (D / 8), tid);
    copy16(p.v_tail + to * BLKK, p.v_tail + from * BLKK, open * (D / 8), tid);
    if (h != 0) return;
    // ---- the table row and the length
    const int32_t *row_s = p.block_table + (long)s * p.bt_stride;
    int32_t *row_d = p.block_table + (long)d * p.bt_stride;
    for (int e = tid; e < np; e += 256) row_d[e] = row_s[e];               // (np <= max_pages)
    if (tid == 0) {
        if (np < p.max_pages) row_d[np] = pg;   // the child's first own page, as given
        p.lens[d] = P;
    }
}

static hipError_t launch_kvpaged_fork(const KvForkParams &p, int D, int n, hipStream_t s)
{
    const dim3 grid((1 << p.page_shift) + 1, p.H, n);
    if (D == 128) hipLaunchKernelGGL((kvpaged_fork_kernel<128>), grid, dim3(256), 0, s, p);
    else if (D == 64) hipLaunchKernelGGL((kvpaged_fork_kernel<64>), grid, dim3(256), 0, s, p);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace sage

extern "C" {

SAGE_KVFORK_API int sage_kvfork_abi_version(void) { return SAGE_KVFORK_ABI_VERSION; }

SAGE_KVFORK_API int sage_kvfork(int8_t *k_int8, float *k_scale, void *v_image, float *v_scale, float *v_amax, void *k_mean,
                                void *k_tail, void *v_tail, int32_t *lens,
                                int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                int B, int Hkv, int head_dim, int dtype,
                                const int32_t *src_slots, const int32_t *dst_slots, const int32_t *new_pages, const int32_t *prefix_lens,
                                int n, void *stream)
{
    using namespace sage;
    const char *const e = "sage_kvfork";
    PagedArgs g;
    SAGE_REQUIRE(k_int8 && k_scale && v_image && v_scale && v_amax && k_tail && v_tail && lens, "%s: null cache pointer (only k_mean may be null)", e);
    SAGE_REQUIRE(src_slots && dst_slots && new_pages, "%s: null src_slots / dst_slots / new_pages pointer (only prefix_lens may be null)", e);
    if (const int rc = paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = kv_check_batch(e, B, Hkv)) return rc;
    SAGE_REQUIRE(head_dim == 64 || head_dim == 128, "%s: head_dim must be 64 or 128 (got %d)", e, head_dim);
    SAGE_REQUIRE(dtype == SAGE_DTYPE_F16 || dtype == SAGE_DTYPE_BF16, "%s: bad dtype %d", e, dtype);
    SAGE_REQUIRE(aligned16(k_int8) && aligned16(k_scale) && aligned16(v_image) && aligned16(k_tail) && aligned16(v_tail) && (!k_mean || aligned16(k_mean)),
                 "%s: k_int8 / k_scale / v_image / k_mean / k_tail / v_tail must be 16-byte aligned", e);
    if (const int rc = paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE(aligned4(src_slots) && aligned4(dst_slots) && aligned4(new_pages) && aligned4(prefix_lens) && aligned4(v_scale) && aligned4(v_amax) &&
                 aligned4(lens), "%s: src_slots / dst_slots / new_pages / prefix_lens / v_scale / v_amax / lens must be 4-byte aligned", e);
    SAGE_REQUIRE(n >= 1 && n <= 65535, "%s: n must be in [1, 65535] (got %d)", e, n);
    const KvForkParams p{k_int8, k_scale, static_cast<unsigned char *>(v_image), v_scale, v_amax, static_cast<uint16_t *>(k_mean),
                         static_cast<uint16_t *>(k_tail), static_cast<uint16_t *>(v_tail), lens, block_table, g.bt_stride, g.page_shift, g.num_pages,
                         g.max_pages, B, Hkv, max_pages_per_seq * page_size, src_slots, dst_slots, new_pages, prefix_lens};
    const hipError_t err = launch_kvpaged_fork(p, head_dim, n, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // extern "C"
