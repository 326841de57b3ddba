// sage_kv_pool.hip -- the page pool of the paged quantised KV cache (include/sage_kvpool_gfx950.h): a free stack, reference
// counts and the block table kept on the device, so that a captured reserve -> append -> attend step grows its sequences across page boundaries
// without the host.  The arithmetic -- clamps, needs, the order of the pops and the pushes, the header -- is csrc/sage_page_pool.h's (the host
// runs the same functions: sage_kvpool_*_host); this file holds the parallel walks and the C entries.  A unit of its own, as sage_kv_fork.hip is.
//
// Replaces in the reference: nothing (no KV cache there).
//
// Every kernel is ONE workgroup of 1024 threads: reserve and fork_prepare take a slot / a fork per thread (B, n <= kVarlenPlanMaxSeq) and grant by
// one inclusive Hillis-Steele scan in LDS; release strides over the listed slots' entries with atomicSub, marks the pages whose last reference it
// took, and compacts the marks over the ids after a barrier -- the pushes do not depend on which thread saw the last reference.  No host read;
// the grids follow from nothing at all.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvpool_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_kv_cache.h"
#include "sage_page_pool.h"

namespace sage {

constexpr int kPoolThreads = 1024;
static_assert(kVarlenPlanMaxSeq <= kPoolThreads, "a slot per thread");

struct KvPoolParams {
    PoolView v;
    PoolTable t;
    int32_t *lens;                   // [B]: read by reserve / fork_prepare, zeroed by release
    const int32_t *new_lens;         // reserve, dense: [B], with T
    const int32_t *cu;               // reserve, packed: [B + 1], with total and max_new
    int T, total, max_new;
    int32_t *granted;                // reserve: [B]
    const int32_t *src, *dst, *prefix_lens, *slots;     // fork_prepare: [n] (prefix_lens nullable); release: slots [n]
    int n;
    int32_t *new_pages, *dst_eff;    // fork_prepare: [n]
};

// inclusive scan of one value per thread over the workgroup (values of threads >= count are 0); every thread returns its own sum, `all` the last
__device__ __forceinline__ long long pool_scan(long long (*sq)[kPoolThreads], int i, long long x, long long &all)
{
    sq[0][i] = x;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < kPoolThreads; d <<= 1) {
        sq[cur ^ 1][i] = sq[cur][i] + (i >= d ? sq[cur][i - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    all = sq[cur][kPoolThreads - 1];
    return sq[cur][i];
}

__global__ void __launch_bounds__(kPoolThreads) kv_pool_init_kernel(int *ws, int N, int B)
{
    const long long words = pool_ws_words(N, B);
    for (long long i = (long long)blockIdx.x * kPoolThreads + threadIdx.x; i < words; i += (long long)gridDim.x * kPoolThreads) ws[i] = pool_init_word(N, B, i);
}

__global__ void __launch_bounds__(kPoolThreads) kv_pool_reserve_kernel(const KvPoolParams p)
{
    __shared__ long long sq[2][kPoolThreads];
    __shared__ int popped_s, refused_s;
    const int b = threadIdx.x;
    const int nf = pool_n_free(p.v);                     // (read by every thread in front of the scan's barriers, written behind them)
    if (b == 0) { popped_s = 0; refused_s = 0; }
    int n = 0, own = 0, want = 0, need = 0;
    if (b < p.v.B) {
        n = p.new_lens != nullptr ? pool_rows_dense(p.new_lens[b], p.T) : pool_rows_packed(p.cu[b], p.cu[b + 1], p.total, p.max_new);
        need = pool_need(p.lens[b], n, p.v.owned[b], p.t, own, want);
    }
    long long asked;
    const long long upto = pool_scan(sq, b, need, asked);
    if (b < p.v.B) {
        if (need == 0) p.granted[b] = n;
        else if (upto > nf) { p.granted[b] = 0; atomicAdd(&refused_s, 1); }
        else {
            pool_take(p.v, p.t, b, nf, (int)upto - need, own, want);
            atomicMax(&popped_s, (int)upto);
            p.granted[b] = n;
        }
    }
    __syncthreads();
    if (b == 0) pool_close_call(p.v, nf, popped_s, refused_s, asked);
}

__global__ void __launch_bounds__(kPoolThreads) kv_pool_fork_prepare_kernel(const KvPoolParams p)
{
    __shared__ long long sq[2][kPoolThreads];
    __shared__ int popped_s, refused_s;
    const int i = threadIdx.x;
    const int nf = pool_n_free(p.v);
    if (i == 0) { popped_s = 0; refused_s = 0; }
    int s = -1, d = -1, np = 0, need = -1;
    if (i < p.n) {
        s = p.src[i]; d = p.dst[i];
        need = pool_fork_need(p.v, p.t, p.lens, s, d, p.prefix_lens != nullptr ? p.prefix_lens + i : nullptr, np);      // (reads n_owned[d]: in front of the barriers)
    }
    long long asked;
    const long long upto = pool_scan(sq, i, need > 0 ? need : 0, asked);
    const bool take = i < p.n && need >= 0 && (need == 0 || upto <= nf);
    if (take) {
        const int *row = p.t.table + (long)s * p.t.stride;
        for (int e = 0; e < np; e++) {                   // one source may fork to many destinations in one call
            const int id = row[e];
            if (id >= 0 && id < p.v.N) atomicAdd(&p.v.refc[id], 1);
        }
    }
    __syncthreads();                                     // the popped pages' counts are stored behind every addition
    if (i < p.n) {
        if (take) {
            int pg;
            pool_fork_take(p.v, p.t, d, np, need, nf, (int)upto - need, pg);
            if (need > 0) atomicMax(&popped_s, (int)upto);
            p.new_pages[i] = pg;
            p.dst_eff[i] = d;
        } else {
            p.new_pages[i] = -1;
            p.dst_eff[i] = -1;
            atomicAdd(&refused_s, 1);
        }
    }
    __syncthreads();
    if (i == 0) pool_close_call(p.v, nf, popped_s, refused_s, asked);
}

__global__ void __launch_bounds__(kPoolThreads) kv_pool_release_kernel(const KvPoolParams p)
{
    __shared__ long long sq[2][kPoolThreads];
    const int tid = threadIdx.x, N = p.v.N;
    const int nf = pool_n_free(p.v);
    // ---- one reference less for every entry the listed slots own; the thread that takes a page's last one marks it
    const long long entries = (long long)p.n * p.t.mp;
    for (long long idx = tid; idx < entries; idx += kPoolThreads) {
        const int b = p.slots[idx / p.t.mp], e = (int)(idx % p.t.mp);
        if (b < 0 || b >= p.v.B || e >= pool_clamp(p.v.owned[b], 0, p.t.mp)) continue;
        int *word = p.t.table + (long)b * p.t.stride + e;
        const int id = *word;
        if (id >= 0 && id < N && atomicSub(&p.v.refc[id], 1) == 1) atomicExch(&p.v.refc[id], kPoolFreed);
        *word = -1;
    }
    __syncthreads();                                     // every n_owned word has been read, every decrement has been made
    for (int i = tid; i < p.n; i += kPoolThreads) {
        const int b = p.slots[i];
        if (b >= 0 && b < p.v.B) { p.v.owned[b] = 0; p.lens[b] = 0; }
    }
    // ---- the compaction over the ids: thread 0 holds the highest ids, so that a page's place is nf + the marked pages of a higher id
    const int per = (N + kPoolThreads - 1) / kPoolThreads;
    const long long top = (long long)N - 1 - (long long)tid * per;          // this thread's ids: top, top - 1 .. top - per + 1, those >= 0
    int mine = 0;
    for (int k = 0; k < per && top - k >= 0; k++)
        mine += __hip_atomic_load(&p.v.refc[top - k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kPoolFreed ? 1 : 0;
    long long freed;
    long long at = nf + pool_scan(sq, tid, mine, freed) - mine;
    for (int k = 0; k < per && top - k >= 0; k++) {
        const int pg = (int)(top - k);
        if (__hip_atomic_load(&p.v.refc[pg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kPoolFreed) continue;
        p.v.refc[pg] = 0;
        if (at < N) p.v.stack[at] = pg;                  // (more marks than the stack has room for: a workspace init never wrote)
        at++;
    }
    if (tid == 0) p.v.hdr[0] = nf + freed < N ? (int)(nf + freed) : N;
}

static hipError_t launch_kv_pool_init(int *ws, int N, int B, hipStream_t s)
{
    const long long blocks = (pool_ws_words(N, B) + kPoolThreads - 1) / kPoolThreads;
    hipLaunchKernelGGL(kv_pool_init_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kPoolThreads), 0, s, ws, N, B);
    return hipGetLastError();
}
static hipError_t launch_kv_pool(void (*kernel)(const KvPoolParams), const KvPoolParams &p, hipStream_t s)
{
    if (p.v.B <= 0 || p.v.B > kVarlenPlanMaxSeq || p.n > kVarlenPlanMaxSeq || p.v.hdr == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(1), dim3(kPoolThreads), 0, s, p);
    return hipGetLastError();
}

// ---- host side: the checks every entry and its _host twin share, in the header's order ------------------------------------------------------
static int pool_ws_check(const char *e, const int32_t *ws, int64_t ws_bytes, int num_pages, int B)
{
    const long long need = 4 * pool_ws_words(num_pages, B);
    SAGE_REQUIRE(ws_bytes >= need, "%s: pool_ws holds %lld bytes, sage_kvpool_ws_bytes(num_pages, B) = %lld", e, (long long)ws_bytes, need);
    return SAGE_OK;
}
static int pool_check_B(const char *e, int B)
{
    SAGE_REQUIRE(B >= 1 && B <= kVarlenPlanMaxSeq, "%s: B must be in 1 .. %d (got %d)", e, kVarlenPlanMaxSeq, B);
    return SAGE_OK;
}
static int pool_check_n(const char *e, int n)
{
    SAGE_REQUIRE(n >= 1 && n <= kVarlenPlanMaxSeq, "%s: n must be in 1 .. %d (got %d)", e, kVarlenPlanMaxSeq, n);
    return SAGE_OK;
}
static bool pool_aligned4(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr, const void *f = nullptr, const void *g = nullptr)
{
    return aligned4(a) && aligned4(b) && aligned4(c) && aligned4(d) && aligned4(f) && aligned4(g);
}

static int pool_init_args(const char *e, int32_t *ws, int64_t ws_bytes, int num_pages, int B)
{
    SAGE_REQUIRE(num_pages >= 1, "%s: num_pages must be at least 1 (got %d)", e, num_pages);
    SAGE_REQUIRE(ws, "%s: null pool_ws", e);
    SAGE_REQUIRE(pool_aligned4(ws), "%s: pool_ws must be 4-byte aligned", e);
    if (const int rc = pool_check_B(e, B)) return rc;
    return pool_ws_check(e, ws, ws_bytes, num_pages, B);
}

static int pool_reserve_args(const char *e, int32_t *ws, int64_t ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                             int B, const int32_t *lens, const int32_t *new_lens, int T, const int32_t *cu_seqlens, int total, int max_new, int32_t *granted, KvPoolParams &p)
{
    PagedArgs g;
    if (const int rc = paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    SAGE_REQUIRE(ws && lens && granted, "%s: null pool_ws, lens or granted", e);
    SAGE_REQUIRE((new_lens != nullptr) != (cu_seqlens != nullptr), "%s: pass exactly one of new_lens (with T) and cu_seqlens (with total and max_new)", e);
    SAGE_REQUIRE(pool_aligned4(ws, block_table, lens, new_lens, cu_seqlens, granted), "%s: pool_ws, block_table, lens, new_lens, cu_seqlens and granted must be 4-byte aligned", e);
    if (const int rc = pool_check_B(e, B)) return rc;
    if (new_lens != nullptr) SAGE_REQUIRE(T >= 1, "%s: T must be at least 1 (got %d)", e, T);
    else SAGE_REQUIRE(total >= 1 && max_new >= 1, "%s: total and max_new must be at least 1 (got %d, %d)", e, total, max_new);
    if (const int rc = pool_ws_check(e, ws, ws_bytes, num_pages, B)) return rc;
    p = KvPoolParams{};
    p.v = pool_view(ws, num_pages, B);
    p.t = PoolTable{block_table, g.bt_stride, g.max_pages, g.page_shift};
    p.lens = const_cast<int32_t *>(lens); p.new_lens = new_lens; p.T = T; p.cu = cu_seqlens; p.total = total; p.max_new = max_new; p.granted = granted;
    return SAGE_OK;
}

static int pool_release_args(const char *e, int32_t *ws, int64_t ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                             int B, int32_t *lens, const int32_t *slots, int n, KvPoolParams &p)
{
    PagedArgs g;
    if (const int rc = paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    SAGE_REQUIRE(ws && lens && slots, "%s: null pool_ws, lens or slots", e);
    SAGE_REQUIRE(pool_aligned4(ws, block_table, lens, slots), "%s: pool_ws, block_table, lens and slots must be 4-byte aligned", e);
    if (const int rc = pool_check_B(e, B)) return rc;
    if (const int rc = pool_check_n(e, n)) return rc;
    if (const int rc = pool_ws_check(e, ws, ws_bytes, num_pages, B)) return rc;
    p = KvPoolParams{};
    p.v = pool_view(ws, num_pages, B);
    p.t = PoolTable{block_table, g.bt_stride, g.max_pages, g.page_shift};
    p.lens = lens; p.slots = slots; p.n = n;
    return SAGE_OK;
}

static int pool_fork_args(const char *e, int32_t *ws, int64_t ws_bytes, const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                          int B, const int32_t *lens, const int32_t *src_slots, const int32_t *dst_slots, const int32_t *prefix_lens, int n,
                          int32_t *new_pages, int32_t *dst_eff, KvPoolParams &p)
{
    PagedArgs g;
    if (const int rc = paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    SAGE_REQUIRE(ws && lens && src_slots && dst_slots && new_pages && dst_eff, "%s: null pool_ws, lens, src_slots, dst_slots, new_pages or dst_eff (only prefix_lens may be null)", e);
    SAGE_REQUIRE(pool_aligned4(ws, block_table, lens, src_slots, dst_slots, prefix_lens) && pool_aligned4(new_pages, dst_eff),
                 "%s: pool_ws, block_table, lens, src_slots, dst_slots, prefix_lens, new_pages and dst_eff must be 4-byte aligned", e);
    if (const int rc = pool_check_B(e, B)) return rc;
    if (const int rc = pool_check_n(e, n)) return rc;
    if (const int rc = pool_ws_check(e, ws, ws_bytes, num_pages, B)) return rc;
    p = KvPoolParams{};
    p.v = pool_view(ws, num_pages, B);
    p.t = PoolTable{const_cast<int32_t *>(block_table), g.bt_stride, g.max_pages, g.page_shift};      // (fork_prepare reads the table)
    p.lens = const_cast<int32_t *>(lens); p.src = src_slots; p.dst = dst_slots; p.prefix_lens = prefix_lens; p.n = n; p.new_pages = new_pages; p.dst_eff = dst_eff;
    return SAGE_OK;
}

static int pool_launched(const char *e, hipError_t err)
{
    if (err != hipSuccess) return set_last_error(SAGE_ELAUNCH, "%s launch: %s", e, hipGetErrorString(err));
    return SAGE_OK;
}

}  // namespace sage

extern "C" {

using namespace sage;

SAGE_KVPOOL_API int sage_kvpool_abi_version(void) { return SAGE_KVPOOL_ABI_VERSION; }

SAGE_KVPOOL_API int64_t sage_kvpool_ws_bytes(int num_pages, int B)
{
    if (num_pages < 1 || B < 1) return set_last_error(SAGE_EINVAL, "sage_kvpool_ws_bytes: num_pages and B must be at least 1 (got %d, %d)", num_pages, B);
    return 4 * pool_ws_words(num_pages, B);
}

SAGE_KVPOOL_API int sage_kvpool_init(int32_t *pool_ws, int64_t pool_ws_bytes, int num_pages, int B, void *stream)
{
    const char *const e = "sage_kvpool_init";
    if (const int rc = pool_init_args(e, pool_ws, pool_ws_bytes, num_pages, B)) return rc;
    return pool_launched(e, launch_kv_pool_init(pool_ws, num_pages, B, static_cast<hipStream_t>(stream)));
}

SAGE_KVPOOL_API int sage_kvpool_init_host(int32_t *pool_ws, int64_t pool_ws_bytes, int num_pages, int B)
{
    if (const int rc = pool_init_args("sage_kvpool_init_host", pool_ws, pool_ws_bytes, num_pages, B)) return rc;
    for (long long i = 0; i < pool_ws_words(num_pages, B); i++) pool_ws[i] = pool_init_word(num_pages, B, i);
    return SAGE_OK;
}

SAGE_KVPOOL_API int sage_kvpool_reserve(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                        int max_pages_per_seq, int B, const int32_t *lens, const int32_t *new_lens, int T,
                                        const int32_t *cu_seqlens, int total, int max_new, int32_t *granted, void *stream)
{
    const char *const e = "sage_kvpool_reserve";
    KvPoolParams p;
    if (const int rc = pool_reserve_args(e, pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, new_lens, T, cu_seqlens, total,
                                         max_new, granted, p)) return rc;
    return pool_launched(e, launch_kv_pool(kv_pool_reserve_kernel, p, static_cast<hipStream_t>(stream)));
}

SAGE_KVPOOL_API int sage_kvpool_reserve_host(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, const int32_t *lens, const int32_t *new_lens, int T,
                                             const int32_t *cu_seqlens, int total, int max_new, int32_t *granted)
{
    KvPoolParams p;
    if (const int rc = pool_reserve_args("sage_kvpool_reserve_host", pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, new_lens,
                                         T, cu_seqlens, total, max_new, granted, p)) return rc;
    pool_reserve_serial(p.v, p.t, p.lens, p.new_lens, p.T, p.cu, p.total, p.max_new, p.granted);
    return SAGE_OK;
}

SAGE_KVPOOL_API int sage_kvpool_release(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                        int max_pages_per_seq, int B, int32_t *lens, const int32_t *slots, int n, void *stream)
{
    const char *const e = "sage_kvpool_release";
    KvPoolParams p;
    if (const int rc = pool_release_args(e, pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, slots, n, p)) return rc;
    return pool_launched(e, launch_kv_pool(kv_pool_release_kernel, p, static_cast<hipStream_t>(stream)));
}

SAGE_KVPOOL_API int sage_kvpool_release_host(int32_t *pool_ws, int64_t pool_ws_bytes, int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, int32_t *lens, const int32_t *slots, int n)
{
    KvPoolParams p;
    if (const int rc = pool_release_args("sage_kvpool_release_host", pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, slots, n, p))
        return rc;
    pool_release_serial(p.v, p.t, p.lens, p.slots, p.n);
    return SAGE_OK;
}

SAGE_KVPOOL_API int sage_kvpool_fork_prepare(int32_t *pool_ws, int64_t pool_ws_bytes, const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                             int max_pages_per_seq, int B, const int32_t *lens, const int32_t *src_slots, const int32_t *dst_slots,
                                             const int32_t *prefix_lens, int n, int32_t *new_pages, int32_t *dst_eff, void *stream)
{
    const char *const e = "sage_kvpool_fork_prepare";
    KvPoolParams p;
    if (const int rc = pool_fork_args(e, pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, src_slots, dst_slots, prefix_lens, n,
                                      new_pages, dst_eff, p)) return rc;
    return pool_launched(e, launch_kv_pool(kv_pool_fork_prepare_kernel, p, static_cast<hipStream_t>(stream)));
}

SAGE_KVPOOL_API int sage_kvpool_fork_prepare_host(int32_t *pool_ws, int64_t pool_ws_bytes, const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size,
                                                  int max_pages_per_seq, int B, const int32_t *lens, const int32_t *src_slots, const int32_t *dst_slots,
                                                  const int32_t *prefix_lens, int n, int32_t *new_pages, int32_t *dst_eff)
{
    KvPoolParams p;
    if (const int rc = pool_fork_args("sage_kvpool_fork_prepare_host", pool_ws, pool_ws_bytes, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, B, lens, src_slots,
                                      dst_slots, prefix_lens, n, new_pages, dst_eff, p)) return rc;
    pool_fork_prepare_serial(p.v, p.t, p.lens, p.src, p.dst, p.prefix_lens, p.n, p.new_pages, p.dst_eff);
    return SAGE_OK;
}

}  // extern "C"
