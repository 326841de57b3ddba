// sage_cabi.hip -- extern "C" entry points declared in include/sage_gfx950.h.
// Validates arguments, fills the kernel parameter blocks, launches on the caller's stream.
#include "../../include/sage_gfx950.h"
#include "../../include/sage_kvpaged_gfx950.h"
#include "../../include/sage_kvpsplit_gfx950.h"
#include "../../include/sage_kvpvarlen_gfx950.h"
#include "../../include/sage_kvstep_gfx950.h"
#include "../../include/sage_kvlist_gfx950.h"
#include "../../include/sage_kvlsplit_gfx950.h"
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_work_order.h"
#include "sage_step_list.h"
#include "sage_host_checks.h"
#include "sage_kv_cache.h"

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static thread_local char g_err[512] = "";

int sage::set_last_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

using sage::aligned16, sage::aligned16_strides, sage::multiples_of, sage::k_tile_fits_int;    // (sage_host_checks.h, with SAGE_REQUIRE)

int check_launch(hipError_t e, const char *what)
{
    if (e != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
    return SAGE_OK;
}

// the argument checks that come back in every entry point
#define SAGE_REQUIRE_HEAD_DIM(D, hint) SAGE_REQUIRE((D) == 64 || (D) == 128, "head_dim must be 64 or 128 (got %d)" hint, D)
#define SAGE_REQUIRE_DTYPE(t, name) SAGE_REQUIRE((t) == SAGE_DTYPE_F16 || (t) == SAGE_DTYPE_BF16, "bad " name " %d", t)
inline int64_t stats_slabs(int64_t L) { return (L + sage::kStatsSlab - 1) / sage::kStatsSlab; }       // 512-token slabs of a sequence of L tokens

struct Strides { int64_t sb, sh, sl; };         // element strides of a [batch, head, row, D] view (packed tensors: sb = 0)
inline bool multiples_of(int n, const Strides &s) { return multiples_of(n, s.sb, s.sh, s.sl); }
struct MaskArg { const void *ptr; int kind; int64_t sb, sh, sq, sk; };

// SageLaunchAttr (nullable) -> the launch workspace and the launcher's options; the attributes are arguments of THIS call, nothing is kept
struct LaunchAttr {
    unsigned *ws; sage::AttnLaunchOpts opts; unsigned *trace; int trace_wgs; const int32_t *q_start; int window; bool bottom_right, gqa_pack;
    // SAGE_ATTR_KV_SPLIT: the bit, the chunk count of flags bits 16-23, and launch_ws / launch_ws_bytes as the split workspace (ws stays null then)
    bool kv_split_flag; int kv_split; void *split_ws; int64_t split_ws_bytes;
};
// the refusal every entry point but sage_attn_fused_q_pv_f8_kvlens gives the split's bit and its count bits
#define SAGE_REFUSE_KV_SPLIT(la) SAGE_REQUIRE(!(la).kv_split_flag && (la).kv_split == 0, \
    "SAGE_ATTR_KV_SPLIT (and the chunk count in flags bits 16-23): sage_attn_fused_q_pv_f8_kvlens with Lq <= 128 and the exact score form only")
int read_attr(const SageLaunchAttr *attr, void *stream, bool takes_ws, LaunchAttr &out)
{
    out.ws = nullptr;
    out.opts = sage::AttnLaunchOpts{static_cast<hipStream_t>(stream), false, false, nullptr};
    out.trace = nullptr;
    out.trace_wgs = 0;
    out.q_start = nullptr;
    out.window = 0;
    out.bottom_right = false;
    out.gqa_pack = false;
    out.kv_split_flag = false;
    out.kv_split = 0;
    out.split_ws = nullptr;
    out.split_ws_bytes = 0;
    if (attr == nullptr) return SAGE_OK;
    SageLaunchAttr a{};
    // struct_bytes is what the CALLER's struct holds: fewer bytes than ours (an older caller) are read as far as they go, more (a newer
    // caller) are ignored beyond what this library knows; 0 -- a caller that never set it -- is refused rather than guessed at
    SAGE_REQUIRE(attr->struct_bytes >= 8, "SageLaunchAttr.struct_bytes = %u: set it to sizeof(SageLaunchAttr) (at least the 8-byte header)", attr->struct_bytes);
    const size_t n = attr->struct_bytes > sizeof(SageLaunchAttr) ? sizeof(SageLaunchAttr) : attr->struct_bytes;
    memcpy(&a, attr, n);
    if (n < offsetof(SageLaunchAttr, q_start) + sizeof(a.q_start)) a.q_start = nullptr;      // (a struct that ends inside the field does not have it)
    if (n < offsetof(SageLaunchAttr, window) + sizeof(a.window)) a.window = 0;
    SAGE_REQUIRE(a.window >= 0, "SageLaunchAttr.window = %d: the number of keys a row sees up to its diagonal, 0 = unbounded", a.window);
    SAGE_REQUIRE((a.flags & ~(SAGE_ATTR_FP8_EXACT_SCORES | SAGE_ATTR_FP8_FOLDED_SCORES | SAGE_ATTR_FORCE_PERSISTENT | SAGE_ATTR_CAUSAL_BOTTOM_RIGHT | SAGE_ATTR_GQA_PACK |
                              SAGE_ATTR_KV_SPLIT | (0xffu << SAGE_ATTR_KV_SPLIT_SHIFT))) == 0, "unknown SageLaunchAttr.flags 0x%x", a.flags);
    const bool kv_split = (a.flags & SAGE_ATTR_KV_SPLIT) != 0;      // (launch_ws is then the split workspace, checked against the shapes by the entry that honours the bit)
    SAGE_REQUIRE((a.flags & (SAGE_ATTR_FP8_EXACT_SCORES | SAGE_ATTR_FP8_FOLDED_SCORES)) != (SAGE_ATTR_FP8_EXACT_SCORES | SAGE_ATTR_FP8_FOLDED_SCORES),
                 "SageLaunchAttr.flags asks for both FP8 score forms");
    SAGE_REQUIRE(kv_split || a.launch_ws == nullptr || (a.launch_ws_bytes >= sage::kAttnSchedBytes && (reinterpret_cast<uintptr_t>(a.launch_ws) & 127u) == 0),
                 "the launch workspace is %d bytes, 128-byte aligned, zeroed (got %lld bytes at %p)", sage::kAttnSchedBytes,
                 (long long)a.launch_ws_bytes, a.launch_ws);
    SAGE_REQUIRE(!(a.flags & SAGE_ATTR_FORCE_PERSISTENT) || (a.launch_ws != nullptr && !kv_split),
                 "SAGE_ATTR_FORCE_PERSISTENT needs a launch workspace (with SAGE_ATTR_KV_SPLIT there is none: launch_ws is the split workspace)");
    out.ws = takes_ws && !kv_split ? static_cast<unsigned *>(a.launch_ws) : nullptr;
    out.kv_split_flag = kv_split;
    out.kv_split = (int)((a.flags >> SAGE_ATTR_KV_SPLIT_SHIFT) & 0xffu);
    if (kv_split) { out.split_ws = a.launch_ws; out.split_ws_bytes = a.launch_ws_bytes; }
    out.opts.fp8_folded = (a.flags & SAGE_ATTR_FP8_FOLDED_SCORES) != 0;
    out.opts.force_persistent = takes_ws && (a.flags & SAGE_ATTR_FORCE_PERSISTENT) != 0;
    out.opts.grid_out = a.grid_out;
    out.trace = a.trace;
    out.trace_wgs = a.trace != nullptr ? a.trace_wgs : 0;
    out.q_start = a.q_start;
    out.window = a.window;
    out.bottom_right = (a.flags & SAGE_ATTR_CAUSAL_BOTTOM_RIGHT) != 0;
    out.gqa_pack = (a.flags & SAGE_ATTR_GQA_PACK) != 0;
    return SAGE_OK;
}

// What an attention entry point received: it sets the fields it has by name, the rest stays zero / null.
enum QForm {
    Q_INT8,             // INT8 q with q_scale, groups by qk_quant_gran / q_warp; scores scaled by sm_scale_log2
    Q_FUSED_THREAD,     // fp16 / bf16 q (q_dtype), quantised per thread group in the kernel prologue; per-thread k scales; dense
    Q_FUSED_BLOCK,      // fp16 / bf16 q, multiplied by q_premul and quantised per 128-row block in the prologue; per-block k scales
};
struct AttnCall {
    QForm q_form;
    bool pv_fp8;                     // the PV format: FP8 (v_scale) or FP16
    const void *q; const int8_t *k; const void *v; void *o; float *lse;
    const float *q_scale, *k_scale, *v_scale, *v_mean;
    int B, Hq, Hkv, Lq, Lk, D;       // varlen: B = nseq, Lq = max_seqlen_q, no Lk
    Strides qs, ks, os;
    const Strides *v_rows;           // `v` is the caller's fp16 value tensor itself (rows of these strides), read in place; null: the tile image
    const MaskArg *mask;
    bool varlen;                     // packed batch: the prefix arrays, and either the work list or (nullable) seq_order
    const int32_t *cu_q, *cu_k, *cu_qs, *cu_ks, *seq_order, *work_items, *work_hdr;
    int items_bound;
    int64_t lse_sh;                  // varlen lse [Hq, sum Lq]: its head stride
    const int32_t *kv_lens;          // per-sample key lengths [B] of a dense, right-padded batch.  Also the mark of the ONE entry point
                                     // (sage_attn_fused_q_pv_f8_kvlens) that takes per-sample query offsets: those arrive in the attributes
                                     // (SageLaunchAttr::q_start, read by attn_run), so they have no field here
    int kv_split;                    // > 1: the (inexact) split, the chunks folded into Hq / Hkv by the entry point
    const sage::PagedArgs *paged;    // sage_kvpaged_attn: k / v / k_scale are a pool of pages behind a block table (with kv_lens; Lk = the logical capacity)
    const sage::RaggedArgs *ragged;  // sage_kvpvarlen_attn (with paged): q / o packed [total_q, Hq, D] behind cu_seqlens_q, lse [Hq, total_q]; Lq = max_seqlen_q, qs.sb = os.sb = 0
    bool paged_split;                // sage_kvpsplit_attn (with paged): the exact split on that pool -- SAGE_ATTR_KV_SPLIT is required instead of refused
    bool step;                       // sage_kvstep_attn (with ragged): two launches behind band filters, the decode rows packed by GQA group
    bool list; int32_t *list_ws;     // sage_kvlist_attn (with step): the work lists' workspace -- a plan launch in front, the list kernels
    int64_t list_ws_bytes;
    bool lsplit;                     // sage_kvlsplit_attn (with list): the decode sequences as S chunks -- SAGE_ATTR_KV_SPLIT is required instead of refused
    int is_causal, gran, q_warp, pv_accum, q_dtype, out_dtype;
    float sm_scale_log2, q_premul;
    void *stream; const SageLaunchAttr *attr;
};

// What differs per Q form: the scale groups of q and k (p.q_gran, p.qs_per_blk, p.ks_shift; kthread: four k scales per 64 keys) and where
// sm_scale * log2(e) goes
int set_q_form(const AttnCall &c, sage::AttnParams &p, bool &kthread)
{
    kthread = c.q_form == Q_FUSED_THREAD;
    p.sm_scale_log2 = c.sm_scale_log2;
    if (c.q_form == Q_FUSED_THREAD) { p.q_gran = sage::QG_PER_THREAD; p.qs_per_blk = 32; }
    if (c.q_form == Q_FUSED_BLOCK) {
        p.q_gran = sage::QG_PER_BLOCK; p.qs_per_blk = 1;
        p.sm_scale_log2 = 1.0f;                 // sm_scale * log2(e) is folded into the quantised q (q_premul), as the reference's quantiser does
        p.q_premul = c.q_premul;
    }
    if (c.q_form != Q_INT8) return SAGE_OK;
    const bool k128 = (c.gran & SAGE_GRAN_KBLK128) != 0;       // k scale groups of 128 keys (sm90 configuration)
    const int gran = c.gran & ~SAGE_GRAN_KBLK128;
    SAGE_REQUIRE(gran >= SAGE_GRAN_PER_BLOCK && gran <= SAGE_GRAN_PER_THREAD, "bad qk_quant_gran %d", gran);
    SAGE_REQUIRE(!k128 || (!c.varlen && c.mask == nullptr), "128-key k scale groups: dense, unmasked attention only");
    SAGE_REQUIRE(!c.varlen || gran == SAGE_GRAN_PER_BLOCK, "varlen supports per_block scales only");
    p.ks_shift = k128 ? 1 : 0;
    if (gran == SAGE_GRAN_PER_BLOCK) { p.q_gran = sage::QG_PER_BLOCK; p.qs_per_blk = 1; }
    else if (gran == SAGE_GRAN_PER_WARP) {
        SAGE_REQUIRE(c.q_warp == 32 || c.q_warp == 16, "per_warp q_warp must be 32 or 16 (got %d)", c.q_warp);
        p.q_gran = c.q_warp == 32 ? sage::QG_PER_WARP32 : sage::QG_PER_WARP16;
        p.qs_per_blk = sage::BLKQ / c.q_warp;
    } else {
        SAGE_REQUIRE(c.q_warp == 32 || c.q_warp == 16, "per_thread q_warp must be 32 or 16 (got %d)", c.q_warp);
        p.q_gran = c.q_warp == 32 ? sage::QG_PER_THREAD : sage::QG_PER_THREAD16;
        p.qs_per_blk = (sage::BLKQ / c.q_warp) * 8; kthread = true;
    }
    return SAGE_OK;
}

// the geometry of a call (after set_q_form): tensors, shape, strides, scale slots
void fill_geometry(const AttnCall &c, bool kthread, sage::AttnParams &p)
{
    p.q = c.q; p.k = c.k; p.v = c.v; p.o = c.o; p.lse = c.lse;
    p.q_scale = c.q_scale; p.k_scale = c.k_scale; p.v_scale = c.v_scale; p.v_mean = c.v_mean;
    p.cu_q = c.cu_q; p.cu_k = c.cu_k; p.cu_qs = c.cu_qs; p.cu_ks = c.cu_ks; p.seq_order = c.seq_order;
    p.work_items = c.work_items; p.work_hdr = c.work_hdr; p.items_bound = c.items_bound;
    p.B = c.B; p.Hq = c.Hq; p.Hkv = c.Hkv; p.group = c.Hq / c.Hkv;
    p.Lq = c.Lq; p.Lk = c.Lk;
    p.nqblk = (c.Lq + sage::BLKQ - 1) / sage::BLKQ;
    p.q_sb = c.qs.sb; p.q_sh = c.qs.sh; p.q_sl = c.qs.sl;
    p.k_sb = c.ks.sb; p.k_sh = c.ks.sh; p.k_sl = c.ks.sl;
    p.o_sb = c.os.sb; p.o_sh = c.os.sh; p.o_sl = c.os.sl;
    p.nqs = p.nqblk * p.qs_per_blk;
    p.nks = ((c.Lk + (sage::BLKK << p.ks_shift) - 1) / (sage::BLKK << p.ks_shift)) * (kthread ? 4 : 1);
    p.out_dtype = c.out_dtype;
    p.lse_sh = c.lse_sh;
    p.kv_split = c.kv_split;
    if (c.v_rows != nullptr) { p.v_rows = 1; p.v_sb = c.v_rows->sb; p.v_sh = c.v_rows->sh; p.v_sl = c.v_rows->sl; }
}

// SAGE_ATTR_KV_SPLIT: bytes of the split workspace -- chunk_max, lse_part [B, Hkv, S, group, Lq] and o_part [.., D], fp32, each segment rounded up to 128 bytes
inline int64_t r128(int64_t x) { return (x + 127) / 128 * 128; }
inline int64_t kv_split_ws_bytes(int64_t B, int64_t Hq, int64_t Lq, int64_t D, int64_t S) { return 2 * r128(4 * B * Hq * S * Lq) + r128(4 * B * Hq * S * Lq * D); }

// the split workspace of a call of S chunks (`who`: the prefix of the message, the flag or the entry that requires it)
int kv_split_ws_check(const char *who, const void *ws, int64_t ws_bytes, int64_t B, int64_t Hq, int64_t Lq, int64_t D, int64_t S)
{
    const int64_t need = kv_split_ws_bytes(B, Hq, Lq, D, S);
    SAGE_REQUIRE(ws != nullptr && (reinterpret_cast<uintptr_t>(ws) & 127u) == 0 && ws_bytes >= need,
                 "%s: launch_ws is the split workspace, %lld bytes of device memory, 128-byte aligned (got %lld bytes at %p)",
                 who, (long long)need, (long long)ws_bytes, ws);
    return SAGE_OK;
}

// The kv_lens family's exact split (sage_attn_fused_q_pv_f8_kvlens with SAGE_ATTR_KV_SPLIT; the call is validated -- v_mean null --, p / v describe
// the unsplit launch): pass 1 (the chunk maxima), pass 2 (the chunks folded into the kv heads, seeded, FP32 partials) and the merge, on the call's stream.
// (sage_kvpsplit_attn, c.paged set: the same three launches, pass 1 and pass 2 through the block table; Lk is the logical capacity)
int kv_split_run(const AttnCall &c, const LaunchAttr &la, const sage::AttnParams &p0, const sage::AttnVariant &v0)
{
    const int S = la.kv_split, tiles = ((c.Lk + 63) / 64 + S - 1) / S;      // T = ceil(ceil(Lk / 64) / S), from the padded Lk
    if (const int rc = kv_split_ws_check(c.paged != nullptr ? "sage_kvpsplit_attn: SAGE_ATTR_KV_SPLIT" : "SAGE_ATTR_KV_SPLIT", la.split_ws, la.split_ws_bytes,
                                         c.B, c.Hq, c.Lq, c.D, S)) return rc;
    SAGE_REQUIRE((int64_t)c.B * c.Hq * S < ((int64_t)1 << 31), "SAGE_ATTR_KV_SPLIT: grid too large");
    const int64_t rows = (int64_t)c.B * c.Hq * S * c.Lq;
    float *chunk_max = static_cast<float *>(la.split_ws);
    float *lse_part = reinterpret_cast<float *>(static_cast<char *>(la.split_ws) + r128(4 * rows));
    float *o_part = reinterpret_cast<float *>(static_cast<char *>(la.split_ws) + 2 * r128(4 * rows));
    const hipStream_t stream = static_cast<hipStream_t>(c.stream);

    sage::ChunkMaxLensParams m{};
    m.q = c.q; m.k = c.k; m.k_scale = c.k_scale; m.out = chunk_max; m.kv_lens = c.kv_lens; m.q_start = la.q_start;
    m.B = c.B; m.Hq = c.Hq; m.Hkv = c.Hkv; m.group = c.Hq / c.Hkv; m.Lq = c.Lq; m.Lk = c.Lk; m.D = c.D;
    m.S = S; m.tiles = tiles; m.nks = p0.nks;
    m.q_sb = c.qs.sb; m.q_sh = c.qs.sh; m.q_sl = c.qs.sl; m.k_sb = c.ks.sb; m.k_sh = c.ks.sh; m.k_sl = c.ks.sl;
    m.sm_scale_log2 = c.sm_scale_log2; m.q_dtype = c.q_dtype; m.causal = c.is_causal != 0;
    if (c.paged != nullptr) {
        if (const int rc = check_launch(sage::launch_chunk_max_lens_paged(m, *c.paged, stream), "sage_kvpsplit_attn pass 1 launch")) return rc;
    } else
    if (const int rc = check_launch(sage::launch_chunk_max_lens(m, stream), "sage_attn_fused_q_pv_f8_kvlens (SAGE_ATTR_KV_SPLIT) pass 1 launch")) return rc;

    // pass 2: the unsplit call's operands read in place, the chunks folded into the kv-head dimension (kv head hk0 * S + chunk); FP32 partials
    // [B, Hq * S, Lq, D] = [B, Hkv, S, group, Lq, D], LSEs [B, Hq * S, Lq]
    sage::AttnParams p = p0;
    sage::AttnVariant v = v0;
    p.Hq = c.Hq * S; p.Hkv = c.Hkv * S; p.kv_split = S; p.kv_base = 64 * tiles;
    p.o = o_part; p.lse = lse_part;
    p.o_sb = (int64_t)p.Hq * c.Lq * c.D; p.o_sh = (int64_t)c.Lq * c.D; p.o_sl = c.D;
    p.seed_max = chunk_max; p.seed_chunks = S; p.seed_first = 0;
    p.sched = nullptr;
    v.seeded = true;
    if (const int rc = check_launch(sage::launch_attention(p, v, la.opts), c.paged != nullptr ? "sage_kvpsplit_attn pass 2 launch" :
                                    "sage_attn_fused_q_pv_f8_kvlens (SAGE_ATTR_KV_SPLIT) pass 2 launch")) return rc;

    sage::SplitMergeParams g{};
    g.o_part = o_part; g.lse_part = lse_part; g.o_tail = nullptr; g.lse_tail = nullptr; g.o_out = c.o; g.lse_out = c.lse;
    g.B = c.B; g.S = S; g.H = c.Hq; g.L = c.Lq; g.D = c.D; g.group = c.Hq / c.Hkv;
    g.o_sb = c.os.sb; g.o_sh = c.os.sh; g.o_sl = c.os.sl; g.dtype = c.out_dtype;
    return check_launch(sage::launch_merge_split_f32(g, stream), c.paged != nullptr ? "sage_kvpsplit_attn merge launch" :
                        "sage_attn_fused_q_pv_f8_kvlens (SAGE_ATTR_KV_SPLIT) merge launch");
}

// The split step call (sage_kvlsplit_attn) behind the listed call's checks (c, p / v describe the listed call, lp its plan launch):
// the entry's own checks in the header's order -- the flag, S, no window, the split workspace -- then plan, pass 1, pass 2, merge and the listed
// chunk launch on the call's stream, no host read in between.  The decode sequences' partials go to the dense workspace of Lq_ws =
// min(max_seqlen_q, 32) rows per (sequence, head); pass 2 carries that stride in AttnParams::lse_sh, free in a seeded launch.
int kv_lsplit_run(const AttnCall &c, const LaunchAttr &la, const sage::AttnParams &p0, const sage::AttnVariant &v0, const sage::KvListPlanParams &lp)
{
    const char *const e = "sage_kvlsplit_attn";
    const int S = la.kv_split;
    SAGE_REQUIRE(la.kv_split_flag, "%s: attr must carry SAGE_ATTR_KV_SPLIT (the unsplit step call is sage_kvlist_attn)", e);
    SAGE_REQUIRE(S >= 2 && S <= 255, "%s: a chunk count of 2 .. 255 in flags bits 16-23 (got %d)", e, S);
    SAGE_REQUIRE(la.window == 0, "%s: no window with a split (got %d)", e, la.window);
    const int lq_ws = sage::step_split_ws_rows(c.Lq), group = c.Hq / c.Hkv;
    if (const int rc = kv_split_ws_check("sage_kvlsplit_attn: SAGE_ATTR_KV_SPLIT", la.split_ws, la.split_ws_bytes, c.B, c.Hq, lq_ws, c.D, S)) return rc;
    const long long bound = lp.items_cap;
    SAGE_REQUIRE(sage::step_split_grid(c.B, S, c.Hkv, group) < (1LL << 31), "%s: grid too large", e);
    const int tiles = sage::step_split_tiles(c.Lk, S);
    const int64_t rows = (int64_t)c.B * c.Hq * S * lq_ws;
    float *chunk_max = static_cast<float *>(la.split_ws);
    float *lse_part = reinterpret_cast<float *>(static_cast<char *>(la.split_ws) + r128(4 * rows));
    float *o_part = reinterpret_cast<float *>(static_cast<char *>(la.split_ws) + 2 * r128(4 * rows));
    const hipStream_t stream = static_cast<hipStream_t>(c.stream);
    if (la.opts.grid_out != nullptr) *la.opts.grid_out = 0;
    if (const int rc = check_launch(sage::launch_kv_list_plan(lp, stream), "sage_kvlsplit_attn plan launch")) return rc;

    sage::ChunkMaxLensParams m{};
    m.q = c.q; m.k = c.k; m.k_scale = c.k_scale; m.out = chunk_max; m.kv_lens = c.kv_lens; m.q_start = la.q_start;
    m.B = c.B; m.Hq = c.Hq; m.Hkv = c.Hkv; m.group = group; m.Lq = c.Lq; m.Lk = c.Lk; m.D = c.D;
    m.S = S; m.tiles = tiles; m.nks = p0.nks;
    m.q_sb = 0; m.q_sh = c.qs.sh; m.q_sl = c.qs.sl; m.k_sb = c.ks.sb; m.k_sh = c.ks.sh; m.k_sl = c.ks.sl;
    m.sm_scale_log2 = c.sm_scale_log2; m.q_dtype = c.q_dtype; m.causal = 1;
    if (const int rc = check_launch(sage::launch_chunk_max_lens_ragged(m, *c.paged, *c.ragged, lq_ws, stream), "sage_kvlsplit_attn pass 1 launch")) return rc;

    // pass 2: the listed decode launch over the seeded form, the chunks folded into the kv-head dimension (kv head hk0 * S + chunk); FP32 partials
    // [B, Hq * S, Lq_ws, D] = [B, Hkv, S, group, Lq_ws, D], LSEs [B, Hq * S, Lq_ws]
    int grid_d = 0, grid_c = 0;
    sage::AttnLaunchOpts o = la.opts;
    const sage::BandArgs decode{0, sage::kStepDecodeRows}, chunk{sage::kStepDecodeRows, c.Lq};
    {
        sage::AttnParams p = p0;
        sage::AttnVariant v = v0;
        p.Hq = c.Hq * S; p.Hkv = c.Hkv * S; p.kv_split = S; p.kv_base = 64 * tiles;
        p.o = o_part; p.lse = lse_part; p.lse_sh = lq_ws;
        p.o_sb = (int64_t)p.Hq * lq_ws * c.D; p.o_sh = (int64_t)lq_ws * c.D; p.o_sl = c.D;
        p.seed_max = chunk_max; p.seed_chunks = S; p.seed_first = 0;
        p.sched = nullptr;
        p.work_hdr = c.list_ws; p.work_items = c.list_ws + sage::kStepHdrWords; p.items_bound = 0;
        v.seeded = true; v.list = true; v.gqa_pack = true; v.band = &decode; o.grid_out = &grid_d;
        if (const int rc = check_launch(sage::launch_attention(p, v, o), "sage_kvlsplit_attn pass 2 launch")) return rc;
    }
    sage::SplitMergeParams g{};
    g.o_part = o_part; g.lse_part = lse_part; g.o_tail = nullptr; g.lse_tail = nullptr; g.o_out = c.o; g.lse_out = c.lse;
    g.B = c.B; g.S = S; g.H = c.Hq; g.L = lq_ws; g.D = c.D; g.group = group;
    g.o_sb = 0; g.o_sh = c.os.sh; g.o_sl = c.os.sl; g.dtype = c.out_dtype;
    if (const int rc = check_launch(sage::launch_merge_split_ragged(g, *c.ragged, c.Lq, (long)c.lse_sh, stream), "sage_kvlsplit_attn merge launch")) return rc;

    if (c.Lq > sage::kStepDecodeRows && bound > 0) {
        // the listed call's chunk launch as that call makes it (hdr + 1: {n_chunk_items, group, fold, left})
        sage::AttnParams pl = p0;
        sage::AttnVariant vs = v0;
        vs.list = true; vs.gqa_pack = false; vs.band = &chunk; o.grid_out = &grid_c;
        pl.work_hdr = c.list_ws + 1; pl.work_items = c.list_ws + sage::kStepHdrWords + c.B; pl.items_bound = (int)bound;
        if (const int rc = check_launch(sage::launch_attention(pl, vs, o), "sage_kvlsplit_attn chunk launch")) return rc;
    }
    if (la.opts.grid_out != nullptr) *la.opts.grid_out = grid_d + grid_c;
    return SAGE_OK;
}

// validates the call, fills the kernel parameter block, launches
int attn_run(const AttnCall &c)
{
    const bool int8q = c.q_form == Q_INT8, per_thread = c.q_form == Q_FUSED_THREAD, per_block = c.q_form == Q_FUSED_BLOCK;
    const bool fp8 = c.pv_fp8, varlen = c.varlen, split = c.kv_split > 1;
    LaunchAttr la;
    // (a pool of pages: what it does not take is refused by name, in front of everything else about the attributes)
    if (c.paged != nullptr && c.paged_split) {
        // sage_kvpsplit_attn: what the split needs of the attributes, by the entry's name and in front of everything else about them -- the flag,
        // S, one query block, no window, the exact score form, the ordinary dispatch, the workspace (the shapes it is sized by are checked below)
        const char *const e = "sage_kvpsplit_attn";
        SageLaunchAttr a{};
        if (c.attr != nullptr && c.attr->struct_bytes >= 8) memcpy(&a, c.attr, c.attr->struct_bytes > sizeof(a) ? sizeof(a) : c.attr->struct_bytes);
        if (c.attr != nullptr && c.attr->struct_bytes < offsetof(SageLaunchAttr, window) + sizeof(a.window)) a.window = 0;
        const int S = (int)((a.flags >> SAGE_ATTR_KV_SPLIT_SHIFT) & 0xffu);
        SAGE_REQUIRE(c.attr != nullptr && c.attr->struct_bytes >= 8 && (a.flags & SAGE_ATTR_KV_SPLIT) != 0,
                     "%s: attr must carry SAGE_ATTR_KV_SPLIT (the unsplit call on a paged cache is sage_kvpaged_attn)", e);
        SAGE_REQUIRE(S >= 2 && S <= 255, "%s: a chunk count of 2 .. 255 in flags bits 16-23 (got %d)", e, S);
        SAGE_REQUIRE(c.Lq <= 128, "%s: Lq <= 128, one query block (got %d)", e, c.Lq);
        SAGE_REQUIRE(a.window == 0, "%s: no window with a split (got %d)", e, a.window);
        SAGE_REQUIRE(!(a.flags & SAGE_ATTR_FP8_FOLDED_SCORES), "%s: SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache (the exact score form only)", e);
        SAGE_REQUIRE(!(a.flags & SAGE_ATTR_FORCE_PERSISTENT), "%s: SAGE_ATTR_FORCE_PERSISTENT is not supported (the split takes the ordinary dispatch only)", e);
        if (const int rc = kv_split_ws_check("sage_kvpsplit_attn: SAGE_ATTR_KV_SPLIT", a.launch_ws, a.launch_ws_bytes, c.B, c.Hq > 0 ? c.Hq : 0, c.Lq > 0 ? c.Lq : 0,
                                             c.D > 0 ? c.D : 0, S)) return rc;
    } else
    if (c.paged != nullptr && c.attr != nullptr && c.attr->struct_bytes >= 8) {
        const char *const e = c.lsplit ? "sage_kvlsplit_attn" : c.list ? "sage_kvlist_attn" : c.step ? "sage_kvstep_attn" : c.ragged != nullptr ? "sage_kvpvarlen_attn" : "sage_kvpaged_attn";
        const unsigned f = c.attr->flags;
        SAGE_REQUIRE(c.lsplit || !(f & (SAGE_ATTR_KV_SPLIT | (0xffu << SAGE_ATTR_KV_SPLIT_SHIFT))),
                     "%s: SAGE_ATTR_KV_SPLIT is not supported on a paged cache (pass 1 and the split's kernels do not look pages up)", e);
        SAGE_REQUIRE(!(f & SAGE_ATTR_FP8_FOLDED_SCORES), "%s: SAGE_ATTR_FP8_FOLDED_SCORES is not supported on a paged cache (the exact score form only)", e);
        SAGE_REQUIRE(!(f & SAGE_ATTR_FORCE_PERSISTENT), "%s: SAGE_ATTR_FORCE_PERSISTENT is not supported on a paged cache (the ordinary dispatch only)", e);
        SAGE_REQUIRE(c.ragged == nullptr || c.step || !(f & SAGE_ATTR_GQA_PACK), "%s: SAGE_ATTR_GQA_PACK is not supported on packed query rows (one workgroup per query head)", e);
        SAGE_REQUIRE(!c.step || !(f & SAGE_ATTR_GQA_PACK), "%s: SAGE_ATTR_GQA_PACK is not taken (the entry packs the decode rows of a GQA group on its own)", e);
    }
    if (const int rc = read_attr(c.attr, c.stream, c.mask == nullptr && !split && c.paged == nullptr, la)) return rc;     // (masked, split and paged launches take no launch workspace)
    // (packed query rows: the offsets place every sample's rows, so they are required -- the bottom-right ones are the caller's kv_lens[b] - Lq_b)
    SAGE_REQUIRE(c.ragged == nullptr || la.q_start != nullptr, "%s: SageLaunchAttr.q_start is required (int32 [B]: the key position of each sample's row 0)",
                 c.lsplit ? "sage_kvlsplit_attn" : c.list ? "sage_kvlist_attn" : c.step ? "sage_kvstep_attn" : "sage_kvpvarlen_attn");
    // ---- the routes a Q form admits
    if (c.kv_lens == nullptr) SAGE_REFUSE_KV_SPLIT(la);
    // (sage_kvlsplit_attn checks the bit, the count and the window by its own name behind the listed call's checks, below)
    SAGE_REQUIRE(c.lsplit || la.kv_split_flag || la.kv_split == 0, "SAGE_ATTR_KV_SPLIT: a chunk count (%d in flags bits 16-23) without the bit", la.kv_split);
    SAGE_REQUIRE(c.lsplit || !la.kv_split_flag || (la.kv_split >= 2 && c.Lq <= 128 && la.window == 0 && !la.opts.fp8_folded),
                 "SAGE_ATTR_KV_SPLIT: a chunk count of 2 .. 255 in flags bits 16-23 (got %d), Lq <= 128 (got %d), no window (got %d) and the exact score form only",
                 la.kv_split, c.Lq, la.window);
    // (pass 2 would add the mean to every chunk's partial, and a row without a visible key would merge to 0 where the unsplit kernel gives the mean)
    SAGE_REQUIRE(!la.kv_split_flag || c.v_mean == nullptr, "SAGE_ATTR_KV_SPLIT: v_mean must be null (the split's partials carry no V mean)");
    SAGE_REQUIRE(!(fp8 && varlen && la.opts.fp8_folded), "packed (varlen) FP8 attention has the exact score form only (SAGE_ATTR_FP8_FOLDED_SCORES)");
    // (per-sample query offsets travel in the attributes; kv_lens marks the one entry point that takes them)
    SAGE_REQUIRE(la.q_start == nullptr || (c.kv_lens != nullptr && c.is_causal && !la.opts.fp8_folded),
                 "SageLaunchAttr.q_start: sage_attn_fused_q_pv_f8_kvlens with is_causal = 1 and the exact score form only");
    // (so does the window, which may come without offsets)
    // (... or, on the packed entry, only together with the bottom-right flag and everything that flag needs)
    SAGE_REQUIRE(la.window == 0 || (c.is_causal && !la.opts.fp8_folded &&
                                    (c.kv_lens != nullptr || (la.bottom_right && per_block && fp8 && varlen && c.pv_accum == SAGE_PV_ACCUM_TWO_LEVEL))),
                 "SageLaunchAttr.window: sage_attn_fused_q_pv_f8_kvlens with is_causal = 1 and the exact score form, or "
                 "sage_attn_fused_qblock_pv_f8_varlen with SAGE_ATTR_CAUSAL_BOTTOM_RIGHT, is_causal = 1 and SAGE_PV_ACCUM_TWO_LEVEL, only");
    // (bottom-right alignment of a packed batch: the one entry point with FP8 PV, the per-block Q quantiser and cu_seqlens)
    SAGE_REQUIRE(!la.bottom_right || (per_block && fp8 && varlen && c.is_causal && c.pv_accum == SAGE_PV_ACCUM_TWO_LEVEL),
                 "SAGE_ATTR_CAUSAL_BOTTOM_RIGHT: sage_attn_fused_qblock_pv_f8_varlen with is_causal = 1 and SAGE_PV_ACCUM_TWO_LEVEL only");
    // (packed GQA groups: the kv_lens entry, decode-shaped, a group to pack)
    SAGE_REQUIRE(!la.gqa_pack || (c.kv_lens != nullptr && !la.opts.fp8_folded && c.Lq <= 32 && c.Hkv > 0 && c.Hq % c.Hkv == 0 && c.Hq / c.Hkv >= 2),
                 "SAGE_ATTR_GQA_PACK: sage_attn_fused_q_pv_f8_kvlens with Lq <= 32, Hq / Hkv >= 2 and the exact score form only");
    SAGE_REQUIRE(c.kv_lens == nullptr || (per_thread && fp8 && !split && c.v_rows == nullptr && !la.opts.fp8_folded),
                 "kv_lens: FP8 PV, the exact score form (SAGE_ATTR_FP8_FOLDED_SCORES), no split");
    SAGE_REQUIRE(!(per_block && varlen) || c.cu_q != nullptr, "varlen needs cu_seqlens_q");
    SAGE_REQUIRE(!(per_block && fp8) || (varlen && c.v_rows == nullptr), "FP8 PV with the per-block Q quantiser: packed (varlen) batches only");
    SAGE_REQUIRE(c.kv_split >= 0 && (!split || (per_thread && c.Hkv % c.kv_split == 0)), "kv_split (%d) must divide the folded kv-head count (%d)", c.kv_split, c.Hkv);
    if (c.v_rows != nullptr) {
        // (no entry point can violate the first line -- every *_vrows entry is dense, unmasked, FP16 PV, fp16 q, without a split: it guards
        // against a misuse inside this file)
        SAGE_REQUIRE(!fp8 && !varlen && c.mask == nullptr && !split && (int8q || c.q_dtype == SAGE_DTYPE_F16),
                     "V rows in place: dense, unmasked FP16-PV calls on fp16 inputs, no split");
        SAGE_REQUIRE(multiples_of(8, *c.v_rows) && c.v_rows->sl >= c.D, "v strides must be multiples of 8 elements (16-byte rows)");
        SAGE_REQUIRE(((int64_t)(c.Lk - 1) * c.v_rows->sl + c.D) * 2 < (int64_t)1 << 31, "one head of v must span less than 2 GiB");
    }
    // ---- the same checks for every Q form; where the forms worded a message differently, each keeps its wording
    SAGE_REQUIRE(c.q && c.k && c.v && c.o && c.k_scale && (!int8q || c.q_scale), "null tensor pointer");
    SAGE_REQUIRE(!fp8 || c.v_scale, per_thread ? "null tensor pointer" : "fp8 PV needs v_scale");
    SAGE_REQUIRE_HEAD_DIM(c.D, "; pad on the host as core.py:260-271 does");
    SAGE_REQUIRE(c.B > 0 && c.Hq > 0 && c.Hkv > 0 && c.Lq > 0 && (int8q || varlen || c.Lk > 0),
                 int8q ? "empty problem (B=%d Hq=%d Hkv=%d Lq=%d)" : "empty problem (B=%d Hq=%d Hkv=%d Lq=%d Lk=%d)", c.B, c.Hq, c.Hkv, c.Lq, c.Lk);
    SAGE_REQUIRE(varlen || c.Lk > 0, "kv_len must be positive");
    SAGE_REQUIRE(c.Hq % c.Hkv == 0, "num_qo_heads (%d) must be divisible by num_kv_heads (%d)", c.Hq, c.Hkv);
    if (!int8q) SAGE_REQUIRE_DTYPE(c.q_dtype, "q_dtype");
    SAGE_REQUIRE_DTYPE(c.out_dtype, "out_dtype");
    SAGE_REQUIRE(aligned16(c.q) && aligned16(c.k) && aligned16(c.v) && aligned16(c.o), "q/k/v/o must be 16-byte aligned");
    // q strides: 16 bytes of INT8, or 8 elements of fp16 / bf16
    SAGE_REQUIRE(multiples_of(int8q ? 16 : 8, c.qs), int8q ? "int8 q/k strides must be multiples of 16" : "q strides must be multiples of 8 elements");
    SAGE_REQUIRE(multiples_of(16, c.ks), int8q ? "int8 q/k strides must be multiples of 16" : "int8 k strides must be multiples of 16");
    SAGE_REQUIRE(k_tile_fits_int(c.ks.sl, c.D), "one 64-key tile of k must span less than 2 GiB (row stride %lld): the kernel addresses a tile's rows with 32-bit offsets",
                 (long long)c.ks.sl);
    SAGE_REQUIRE(multiples_of(8, c.os), "output strides must be multiples of 8 elements");
    SAGE_REQUIRE(c.pv_accum >= SAGE_PV_ACCUM_SINGLE && c.pv_accum <= SAGE_PV_ACCUM_TRITON && (!fp8 || c.pv_accum != SAGE_PV_ACCUM_TRITON),
                 "bad pv_accum %d", c.pv_accum);
    if (varlen) {
        SAGE_REQUIRE(!int8q || (c.cu_q && c.cu_k && c.cu_qs && c.cu_ks), "varlen needs cu_seqlens arrays");
        SAGE_REQUIRE(c.cu_k && c.cu_ks, "varlen needs cu_seqlens_k and the k scale prefix array");
        SAGE_REQUIRE(fp8 || c.lse == nullptr, "varlen FP16 PV returns no lse");
        SAGE_REQUIRE(c.lse == nullptr || c.lse_sh > 0, "varlen lse [Hq, sum Lq]: its head stride lse_sh must be positive (got %lld)", (long long)c.lse_sh);
    }
    SAGE_REQUIRE((c.work_items == nullptr) == (c.work_hdr == nullptr) && (c.work_items == nullptr || (varlen && c.items_bound > 0)),
                 "the work list comes as (work_items, work_hdr, items_bound > 0), varlen only");
    if (c.mask != nullptr) {
        SAGE_REQUIRE(c.mask->ptr, "null attn_mask pointer");
        SAGE_REQUIRE(c.mask->kind >= SAGE_MASK_BOOL && c.mask->kind <= SAGE_MASK_BF16, "bad mask_kind %d", c.mask->kind);
        SAGE_REQUIRE(!c.is_causal, "Mask should be None for causal attention.");           // core.py:310
    }

    sage::AttnParams p{};
    sage::AttnVariant v{};
    if (const int rc = set_q_form(c, p, v.kthread)) return rc;
    fill_geometry(c, v.kthread, p);
    p.sched = la.ws; p.trace = la.trace; p.trace_wgs = la.trace_wgs;
    if (c.mask != nullptr) { p.mask = c.mask->ptr; p.m_sb = c.mask->sb; p.m_sh = c.mask->sh; p.m_sq = c.mask->sq; p.m_sk = c.mask->sk; v.mask_kind = c.mask->kind; }
    if (c.kv_lens != nullptr) { p.cu_k = c.kv_lens; v.kv_lens = true; }
    if (c.paged != nullptr) { v.paged = c.paged; p.nks = 4 << c.paged->page_shift; }      // (the scale slots of ONE page; p.Lk is the logical capacity)
    v.ragged = c.ragged;
    if (la.q_start != nullptr) { p.cu_qs = la.q_start; v.q_start = true; }
    p.window = v.window = la.window;
    v.bottom_right = la.bottom_right;
    v.gqa_pack = la.gqa_pack;
    v.head_dim = c.D; v.pv_fp8 = fp8; v.causal = c.is_causal != 0;
    // FP16 PV: the kernel's TWO_LEVEL parameter selects the Triton kernel form (true) or the CUDA kernel form (false)
    v.two_level = fp8 ? c.pv_accum == SAGE_PV_ACCUM_TWO_LEVEL : c.pv_accum == SAGE_PV_ACCUM_TRITON;
    v.qf = int8q ? 0 : sage::attn_qf(per_block, c.q_dtype);
    if (la.kv_split_flag && !c.lsplit) return kv_split_run(c, la, p, v);
    if (c.list) {
        // the listed step call: the step call's two launches behind a plan launch, their items from its lists (sage_step_list.h) -- the workspace
        // checks first, the last of the entry's; then plan, decode, chunk on the call's stream, no host read in between
        const char *const e = c.lsplit ? "sage_kvlsplit_attn" : "sage_kvlist_attn";
        const int total_q = c.ragged->total_q;
        const long long need = 4 * sage::step_ws_words(c.B, total_q, c.Lq), bound = sage::step_chunk_bound(c.B, total_q, c.Lq);
        SAGE_REQUIRE(c.list_ws != nullptr && (reinterpret_cast<uintptr_t>(c.list_ws) & 3u) == 0, "%s: list_ws must be int32 device memory, 4-byte aligned (got %p)", e, (void *)c.list_ws);
        SAGE_REQUIRE(c.list_ws_bytes >= need, "%s: list_ws holds %lld bytes, sage_kvlist_ws_bytes(B, total_q, max_seqlen_q) = %lld are needed", e, (long long)c.list_ws_bytes, need);
        SAGE_REQUIRE(c.B <= sage::kVarlenPlanMaxSeq, "%s: B must be at most %d, the sequences one plan launch takes (got %d)", e, sage::kVarlenPlanMaxSeq, c.B);
        SAGE_REQUIRE(sage::step_decode_grid(c.B, c.Hkv, c.Hq / c.Hkv) < (1LL << 31) && sage::step_chunk_grid(c.Hq, bound) < (1LL << 31), "%s: grid too large", e);
        sage::KvListPlanParams lp{};
        lp.cu_q = c.ragged->cu_q; lp.kv_lens = c.kv_lens; lp.q_start = la.q_start;
        lp.B = c.B; lp.total_q = total_q; lp.max_seqlen_q = c.Lq; lp.Lk = c.Lk; lp.window = la.window;
        lp.Hq = c.Hq; lp.Hkv = c.Hkv; lp.head_dim = c.D; lp.items_cap = (int)bound; lp.ws = c.list_ws;
        if (c.lsplit) return kv_lsplit_run(c, la, p, v, lp);
        if (la.opts.grid_out != nullptr) *la.opts.grid_out = 0;
        if (const int rc = check_launch(sage::launch_kv_list_plan(lp, static_cast<hipStream_t>(c.stream)), "sage_kvlist_attn plan launch")) return rc;
        int grid_d = 0, grid_c = 0;
        sage::AttnLaunchOpts o = la.opts;
        const sage::BandArgs decode{0, sage::kStepDecodeRows}, chunk{sage::kStepDecodeRows, c.Lq};
        sage::AttnVariant vs = v;
        sage::AttnParams pl = p;
        vs.list = true;
        vs.gqa_pack = true; vs.band = &decode; o.grid_out = &grid_d;
        pl.work_hdr = c.list_ws; pl.work_items = c.list_ws + sage::kStepHdrWords; pl.items_bound = 0;
        if (const int rc = check_launch(sage::launch_attention(pl, vs, o), "sage_kvlist_attn decode launch")) return rc;
        if (c.Lq > sage::kStepDecodeRows && bound > 0) {
            // (hdr + 1: {n_chunk_items, group, fold, left}, the four words the packed route's header starts with)
            vs.gqa_pack = false; vs.band = &chunk; o.grid_out = &grid_c;
            pl.work_hdr = c.list_ws + 1; pl.work_items = c.list_ws + sage::kStepHdrWords + c.B; pl.items_bound = (int)bound;
            if (const int rc = check_launch(sage::launch_attention(pl, vs, o), "sage_kvlist_attn chunk launch")) return rc;
        }
        if (la.opts.grid_out != nullptr) *la.opts.grid_out = grid_d + grid_c;
        return SAGE_OK;
    }
    if (c.step) {
        // the step call: the decode launch -- the samples of 1 .. 32 rows, GPACK's work item -- always, then the chunk launch -- the samples of more
        // rows, the ragged launch's grid -- only if max_seqlen_q admits such a sample (host-known: a pure decode step is one launch).  Both on the
        // call's stream, no host read in between; p.Lq = max_seqlen_q in both, the row bound ragged_band clamps to
        int grid_d = 0, grid_c = 0;
        sage::AttnLaunchOpts o = la.opts;
        if (la.opts.grid_out != nullptr) *la.opts.grid_out = 0;
        const sage::BandArgs decode{0, 32}, chunk{32, c.Lq};
        sage::AttnVariant vs = v;
        vs.gqa_pack = true; vs.band = &decode; o.grid_out = &grid_d;
        if (const int rc = check_launch(sage::launch_attention(p, vs, o), "sage_kvstep_attn decode launch")) return rc;
        if (c.Lq > 32) {
            vs.gqa_pack = false; vs.band = &chunk; o.grid_out = &grid_c;
            if (const int rc = check_launch(sage::launch_attention(p, vs, o), "sage_kvstep_attn chunk launch")) return rc;
        }
        if (la.opts.grid_out != nullptr) *la.opts.grid_out = grid_d + grid_c;
        return SAGE_OK;
    }
    return check_launch(sage::launch_attention(p, v, la.opts), int8q ? "sage_attn launch" : per_block ? "sage_attn_fused_qblock launch" :
                        c.ragged != nullptr ? "sage_kvpvarlen_attn launch" : c.paged != nullptr ? "sage_kvpaged_attn launch" : c.kv_lens != nullptr ? "sage_attn_fused_q_pv_f8_kvlens launch" : "sage_attn_fused_q launch");
}

}  // namespace

extern "C" {

SAGE_API int sage_abi_version(void) { return SAGE_ABI_VERSION; }
SAGE_API const char *sage_last_error(void) { return g_err; }
// host-side views of sage_work_order.h (the code the kernels and launchers run), for tests without a GPU
SAGE_API int sage_debug_work_order_plan(int nheads, int nqblk, int64_t kv_len, int head_dim, int pv_fp8, int forced, int *group, int *fold, int *left)
{
    if (nheads <= 0 || nqblk <= 0 || group == nullptr || fold == nullptr || left == nullptr) return sage::set_last_error(SAGE_EINVAL, "sage_debug_work_order_plan: bad argument");
    sage::WorkOrder w;
    const int grid = sage::plan_work_order(w, nheads, nqblk, (long)kv_len, head_dim, pv_fp8 != 0, forced);
    *group = w.group; *fold = w.fold; *left = w.left;
    return grid;
}
SAGE_API int sage_debug_work_item(int bid, int nwg, int nheads, int nqblk, int group, int fold, int left, int *head, int *qrank)
{
    if (head == nullptr || qrank == nullptr || nwg <= 0 || bid < 0 || bid >= nwg || nheads <= 0 || nqblk <= 0 || group < 0 || fold < 0 || fold > 1 ||
        left < 0 || left >= 8 || left > nheads)
        return sage::set_last_error(SAGE_EINVAL, "sage_debug_work_item: bad argument");
    const sage::WorkOrder w = {group, fold, left};
    return sage::work_item(w, bid, nwg, nheads, nqblk, *head, *qrank) ? 1 : 0;
}
SAGE_API int sage_work_order(void) { return sage::work_order(); }
SAGE_API void sage_set_work_order(int group) { sage::set_work_order_mode(group < -1 ? -1 : group); }

SAGE_API int64_t sage_v_image_bytes(int head_dim, int fp8, int64_t n_kv_tiles_total)
{
    return n_kv_tiles_total * (int64_t)head_dim * (fp8 ? 64 : 128);
}

static int quant_common(const void *x, const void *mean, int8_t *out, float *scale,
                        int B, int H, int L, int D,
                        int64_t x_sb, int64_t x_sh, int64_t x_sl,
                        int64_t o_sb, int64_t o_sh, int64_t o_sl,
                        int64_t mean_sb, int64_t mean_sh,
                        int blk, int warp, int gran, int is_key, int style,
                        float pre_scale, int dtype, void *stream, const int32_t *kv_lens)
{
    SAGE_REQUIRE(x && out && scale, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(blk == 64 || blk == 128, "blk must be 64 or 128 (got %d)", blk);
    SAGE_REQUIRE(B > 0 && H > 0 && L > 0, "empty tensor");
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(style >= 0 && style <= 2, "bad style %d", style);
    SAGE_REQUIRE(aligned16(x) && aligned16(out) && (!mean || aligned16(mean)), "x/out/mean must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, x_sl, x_sh, x_sb), "input strides must be multiples of 8 elements");
    SAGE_REQUIRE(multiples_of(16, o_sl, o_sh, o_sb), "int8 output strides must be multiples of 16");
    SAGE_REQUIRE(!mean || multiples_of(8, mean_sb, mean_sh), "mean strides must be multiples of 8 elements");
    sage::QuantParams p{};
    p.x = x; p.mean = mean; p.out = out; p.scale = scale; p.cu = nullptr; p.cu_scale = nullptr;
    p.B = B; p.H = H; p.L = L; p.D = D;
    p.x_sb = x_sb; p.x_sh = x_sh; p.x_sl = x_sl; p.o_sb = o_sb; p.o_sh = o_sh; p.o_sl = o_sl;
    p.mean_sb = mean_sb; p.mean_sh = mean_sh;
    p.blk = blk; p.warp = warp; p.style = style; p.dtype = dtype; p.pre_scale = pre_scale;
    int slots = 1;
    if (gran == SAGE_GRAN_PER_BLOCK) { p.gran = sage::GR_BLOCK; p.warp = blk; }
    else if (gran == SAGE_GRAN_PER_WARP) {
        SAGE_REQUIRE(warp > 0 && blk % warp == 0 && blk / warp <= 32, "bad warp block %d for blk %d", warp, blk);
        p.gran = sage::GR_WARP; slots = blk / warp;
    } else if (gran == SAGE_GRAN_PER_THREAD) {
        SAGE_REQUIRE(warp > 0 && blk % warp == 0 && warp % 8 == 0, "bad warp block %d for blk %d", warp, blk);
        p.gran = is_key ? sage::GR_THREAD_K : sage::GR_THREAD_Q;
        slots = (blk / warp) * (is_key ? 4 : 8);
        SAGE_REQUIRE(slots <= 64, "too many scale groups per block (%d)", slots);
    } else return sage::set_last_error(SAGE_EINVAL, "bad qk_quant_gran %d", gran);
    p.nscale = ((L + blk - 1) / blk) * slots;
    p.kv_lens = kv_lens;
    return check_launch(sage::launch_quant_int8(p, static_cast<hipStream_t>(stream)), "sage_quant_qk_int8 launch");
}

SAGE_API int sage_quant_qk_int8(const void *x, const void *mean, int8_t *out, float *scale,
                       int B, int H, int L, int D,
                       int64_t x_sb, int64_t x_sh, int64_t x_sl,
                       int64_t o_sb, int64_t o_sh, int64_t o_sl,
                       int64_t mean_sb, int64_t mean_sh,
                       int blk, int warp, int gran, int is_key, int style,
                       float pre_scale, int dtype, void *stream)
{
    return quant_common(x, mean, out, scale, B, H, L, D, x_sb, x_sh, x_sl, o_sb, o_sh, o_sl, mean_sb, mean_sh, blk, warp, gran, is_key, style,
                        pre_scale, dtype, stream, nullptr);
}

// keys of a dense, right-padded batch with a length per sample: per-thread groups of 64-key blocks (the FP8 entry point's K convention), the
// mean (nullable) subtracted first.  Rows >= clamp(kv_lens[b], 0, L) are neither read nor written and take no part in any abs-max; the scale
// slots [B, H, ceil(L / 64) * 4] of blocks wholly past the length stay unwritten.  No host read of kv_lens.
SAGE_API int sage_quant_qk_int8_kvlens(const void *x, const void *mean, int8_t *out, float *scale, const int32_t *kv_lens,
                                       int B, int H, int L, int D,
                                       int64_t x_sb, int64_t x_sh, int64_t x_sl,
                                       int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                       int64_t mean_sb, int64_t mean_sh, int dtype, void *stream)
{
    SAGE_REQUIRE(kv_lens, "sage_quant_qk_int8_kvlens: null kv_lens");
    return quant_common(x, mean, out, scale, B, H, L, D, x_sb, x_sh, x_sl, o_sb, o_sh, o_sl, mean_sb, mean_sh, 64, 64, SAGE_GRAN_PER_THREAD, 1,
                        sage::QS_TRITON_THREAD, 1.0f, dtype, stream, kv_lens);
}

SAGE_API int sage_quant_qk_int8_varlen(const void *x, const void *mean, int8_t *out, float *scale,
                              const int32_t *cu_seqlens, const int32_t *cu_scale,
                              int nseq, int max_seqlen, int H, int D,
                              int64_t x_sl, int64_t x_sh, int64_t o_sl, int64_t o_sh, int64_t mean_sh,
                              int blk, float pre_scale, int dtype, void *stream)
{
    SAGE_REQUIRE(x && out && scale && cu_seqlens && cu_scale, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(blk == 64 || blk == 128, "blk must be 64 or 128 (got %d)", blk);
    SAGE_REQUIRE(nseq > 0 && H > 0 && max_seqlen > 0, "empty batch");
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16(x) && aligned16(out) && (!mean || aligned16(mean)), "x/out/mean must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, x_sl, x_sh) && multiples_of(16, o_sl, o_sh), "bad strides");
    sage::QuantParams p{};
    p.x = x; p.mean = mean; p.out = out; p.scale = scale; p.cu = cu_seqlens; p.cu_scale = cu_scale;
    p.B = nseq; p.H = H; p.L = max_seqlen; p.D = D;
    p.x_sb = 0; p.x_sh = x_sh; p.x_sl = x_sl; p.o_sb = 0; p.o_sh = o_sh; p.o_sl = o_sl;
    p.mean_sb = 0; p.mean_sh = mean_sh;
    p.blk = blk; p.warp = blk; p.gran = sage::GR_BLOCK; p.style = sage::QS_TRITON; p.dtype = dtype;
    p.pre_scale = pre_scale; p.nscale = 0;
    return check_launch(sage::launch_quant_int8(p, static_cast<hipStream_t>(stream)), "sage_quant_qk_int8_varlen launch");
}

SAGE_API int sage_varlen_plan_max_seqs(void) { return sage::kVarlenPlanMaxSeq; }
SAGE_API int sage_varlen_plan(const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, int nseq, int total_k, int blkq, int blkk,
                              int is_causal, int Hq, int Hkv, int head_dim, int pv_fp8,
                              int32_t *cu_q_scale, int32_t *cu_k_scale, int32_t *seq_order,
                              int32_t *work_items, int work_items_cap, int32_t *slab_first, int32_t *slab_seq, int slab_seq_cap,
                              int32_t *hdr, void *stream)
{
    SAGE_REQUIRE((work_items == nullptr || work_items_cap > 0) && (slab_seq == nullptr || slab_seq_cap > 0),
                 "work_items / slab_seq come with their capacities (got %d, %d)", work_items_cap, slab_seq_cap);
    SAGE_REQUIRE(cu_seqlens_q && cu_seqlens_k && cu_k_scale, "null tensor pointer");
    SAGE_REQUIRE(nseq > 0 && nseq <= sage::kVarlenPlanMaxSeq, "nseq must be in 1 .. %d (got %d)", sage::kVarlenPlanMaxSeq, nseq);
    SAGE_REQUIRE(blkq > 0 && blkk > 0, "block sizes must be positive");
    SAGE_REQUIRE(work_items == nullptr || (hdr != nullptr && blkq == sage::BLKQ && blkk == sage::BLKK),
                 "the work list needs hdr and the attention kernel's blocks (%d query rows, %d keys)", sage::BLKQ, sage::BLKK);
    SAGE_REQUIRE(hdr == nullptr || (Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && (head_dim == 64 || head_dim == 128)),
                 "the launch plan needs Hq %% Hkv == 0 and head_dim 64 / 128 (got %d, %d, %d)", Hq, Hkv, head_dim);
    SAGE_REQUIRE((slab_seq == nullptr) == (slab_first == nullptr) && (slab_seq == nullptr || hdr != nullptr), "slab_seq, slab_first and hdr come together");
    sage::VarlenPlanParams p{};
    SAGE_REQUIRE(slab_seq == nullptr || total_k > 0, "the slab map needs total_k, the row count of the packed k / v tensors");
    p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k; p.nseq = nseq; p.blkq = blkq; p.blkk = blkk; p.total_k = total_k;
    p.causal = is_causal == 2 ? 2 : (is_causal ? 1 : 0); p.Hq = Hq > 0 ? Hq : 1; p.Hkv = Hkv > 0 ? Hkv : 1; p.head_dim = head_dim; p.pv_fp8 = pv_fp8 ? 1 : 0;
    p.cu_qs = cu_q_scale; p.cu_ks = cu_k_scale; p.order = seq_order; p.items = work_items;
    p.slab_first = slab_first; p.slab_seq = slab_seq; p.hdr = hdr;
    p.items_cap = work_items_cap; p.slab_cap = slab_seq_cap;
    p.forced_group = sage::work_order() > 0 ? sage::work_order() : -1;
    return check_launch(sage::launch_varlen_plan(p, static_cast<hipStream_t>(stream)), "sage_varlen_plan launch");
}
// host-side view of the work list (csrc/sage_work_order.h, the functions varlen_plan_kernel runs; no GPU needed): lq / lk are HOST arrays of
// the nseq sequence lengths; items_out receives 2 * nitems ints ((sequence, query block), heaviest first), hdr_out {nitems, group, fold, left};
// returns the grid size of the launch, or a negative status
SAGE_API int sage_debug_varlen_items(const int32_t *lq, const int32_t *lk, int nseq, int is_causal, int Hq, int Hkv, int head_dim, int pv_fp8,
                                     int32_t *items_out, int items_cap, int32_t *hdr_out)
{
    if (lq == nullptr || lk == nullptr || items_out == nullptr || hdr_out == nullptr || nseq <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv != 0 ||
        (head_dim != 64 && head_dim != 128))
        return sage::set_last_error(SAGE_EINVAL, "sage_debug_varlen_items: bad argument");
    int nitems = 0, max_lk = 0;
    for (int s = 0; s < nseq; s++) {
        if (lq[s] < 0 || lk[s] < 0) return sage::set_last_error(SAGE_EINVAL, "sage_debug_varlen_items: negative length");
        nitems += (lq[s] + 127) / 128;
        max_lk = lk[s] > max_lk ? lk[s] : max_lk;
    }
    if (nitems > items_cap) return sage::set_last_error(SAGE_EINVAL, "sage_debug_varlen_items: %d items do not fit %d", nitems, items_cap);
    for (int s = 0; s < nseq; s++)
        for (int j = 0; j < (lq[s] + 127) / 128; j++) {
            const int r = sage::varlen_item_rank(lq, lk, nseq, s, j, is_causal == 2 ? 2 : (is_causal ? 1 : 0));
            if (r < 0 || r >= nitems) return sage::set_last_error(SAGE_ELAUNCH, "sage_debug_varlen_items: rank %d out of range", r);
            items_out[2 * r] = s; items_out[2 * r + 1] = j;
        }
    sage::WorkOrder w;
    const int grid = sage::plan_varlen_order(w, Hq, Hq / Hkv, nitems, (long)max_lk, head_dim, pv_fp8 != 0);
    hdr_out[0] = nitems; hdr_out[1] = w.group; hdr_out[2] = w.fold; hdr_out[3] = w.left;
    return grid;
}

static int stats_common(const void *x, void *mean_out, float *ws, float *stats, int B, int H, int L, int D,
                        int64_t x_sb, int64_t x_sh, int64_t x_sl, int dtype, void *stream, const char *what, const int32_t *kv_lens = nullptr)
{
    SAGE_REQUIRE(x && ws, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(B > 0 && H > 0 && L > 0, "empty tensor");
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16(x), "input must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, x_sl, x_sh, x_sb), "strides must be multiples of 8 elements");
    sage::StatsParams p{};
    p.x = x; p.ws = ws; p.stats = stats; p.mean_out = mean_out;
    p.B = B; p.H = H; p.L = L; p.D = D; p.nslab = stats_slabs(L);
    p.x_sb = x_sb; p.x_sh = x_sh; p.x_sl = x_sl; p.dtype = dtype;
    p.kv_lens = kv_lens;
    return check_launch(sage::launch_stats(p, static_cast<hipStream_t>(stream)), what);
}

static int prep_v_common(const void *v, void *v_image, float *v_scale, float *v_mean_out, const float *v_mean_in,
                         const float *stats, const int32_t *cu, const int32_t *cu_tiles, int B, int H, int L, int D,
                         int64_t v_sb, int64_t v_sh, int64_t v_sl, float scale_max, int dtype, int fp8, void *stream, const int32_t *kv_lens = nullptr)
{
    SAGE_REQUIRE(v && v_image, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(B > 0 && H > 0 && L > 0, "empty tensor");
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16(v) && aligned16(v_image), "v / v_image must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, v_sl, v_sh, v_sb), "v strides must be multiples of 8 elements");
    sage::PrepVParams p{};
    p.v = v; p.out = v_image; p.stats = stats; p.mean_in = v_mean_in; p.v_scale = v_scale; p.v_mean = v_mean_out;
    p.cu = cu; p.cu_tiles = cu_tiles;
    p.B = B; p.H = H; p.L = L; p.D = D; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.dtype = dtype; p.fp8 = fp8; p.scale_max = scale_max;
    p.kv_lens = kv_lens;
    return check_launch(sage::launch_prep_v(p, static_cast<hipStream_t>(stream)), "sage_prep_v launch");
}

SAGE_API int64_t sage_stats_ws_floats(int B, int H, int L, int D)
{
    const int64_t nslab = stats_slabs(L);
    return (int64_t)B * H * (nslab + 1) * 3 * D;
}

SAGE_API int sage_channel_mean(const void *x, void *mean_out, float *ws, int B, int H, int L, int D,
                               int64_t x_sb, int64_t x_sh, int64_t x_sl, int dtype, void *stream)
{
    SAGE_REQUIRE(mean_out, "null output pointer");
    return stats_common(x, mean_out, ws, nullptr, B, H, L, D, x_sb, x_sh, x_sl, dtype, stream, "sage_channel_mean launch");
}

// the mean of sample b over rows < clamp(kv_lens[b], 0, L) (0 for a sample without rows): the slabs and the order of sage_channel_mean, so it
// is that entry's result on the first kv_lens[b] rows, bit for bit.  ws: sage_stats_ws_floats(B, H, L, D).  No host read of kv_lens.
SAGE_API int sage_channel_mean_kvlens(const void *x, void *mean_out, float *ws, const int32_t *kv_lens, int B, int H, int L, int D,
                                      int64_t x_sb, int64_t x_sh, int64_t x_sl, int dtype, void *stream)
{
    SAGE_REQUIRE(mean_out && kv_lens, "sage_channel_mean_kvlens: null output or kv_lens pointer");
    return stats_common(x, mean_out, ws, nullptr, B, H, L, D, x_sb, x_sh, x_sl, dtype, stream, "sage_channel_mean_kvlens launch", kv_lens);
}

SAGE_API int sage_channel_mean_varlen(const void *x, void *mean_out, float *ws, const int32_t *cu_seqlens, const int32_t *slab_first,
                                      const int32_t *slab_seq, const int32_t *hdr, int nseq, int total_tokens, int nslab_bound, int H, int D,
                                      int64_t x_sl, int64_t x_sh, int dtype, void *stream)
{
    SAGE_REQUIRE(x && ws && mean_out && cu_seqlens && slab_first && slab_seq && hdr && nseq > 0, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(H > 0 && total_tokens > 0 && nslab_bound >= stats_slabs(total_tokens), "empty tensor or nslab_bound too small");
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16_strides(x, 8, x_sl, x_sh), "input must be 16-byte aligned with strides in multiples of 8 elements");
    sage::StatsParams p{};
    p.x = x; p.ws = ws; p.stats = nullptr; p.mean_out = mean_out;
    p.B = 1; p.H = H; p.L = total_tokens; p.D = D; p.nslab = nslab_bound;
    p.x_sb = 0; p.x_sh = x_sh; p.x_sl = x_sl; p.dtype = dtype;
    p.cu = cu_seqlens; p.slab_first = slab_first; p.slab_seq = slab_seq; p.hdr = hdr; p.nseq = nseq;
    return check_launch(sage::launch_stats(p, static_cast<hipStream_t>(stream)), "sage_channel_mean_varlen launch");
}

// the dense FP8 V pre-pass: statistics, then scales and image; kv_lens (nullable): over the valid tokens of each sample only
static int prep_v_fp8_dense(const void *v, void *v_image, float *v_scale, float *v_mean, float *ws, const int32_t *kv_lens,
                            int B, int H, int L, int D, int64_t v_sb, int64_t v_sh, int64_t v_sl, float scale_max, int dtype, void *stream)
{
    SAGE_REQUIRE(scale_max > 0.0f, "scale_max must be positive");
    float *stats = ws + (int64_t)B * H * stats_slabs(L) * 3 * D;      // final block lives behind the partials
    if (const int rc = stats_common(v, nullptr, ws, stats, B, H, L, D, v_sb, v_sh, v_sl, dtype, stream,
                                    kv_lens ? "sage_v_stats_kvlens launch" : "sage_v_stats launch", kv_lens)) return rc;
    return prep_v_common(v, v_image, v_scale, v_mean, nullptr, stats, nullptr, nullptr, B, H, L, D, v_sb, v_sh, v_sl,
                         scale_max, dtype, 1, stream, kv_lens);
}

SAGE_API int sage_prep_v_fp8(const void *v, void *v_image, float *v_scale, float *v_mean, float *ws,
                    int B, int H, int L, int D, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                    float scale_max, int dtype, void *stream)
{
    SAGE_REQUIRE(v_scale && ws, "fp8 V pre-pass needs v_scale and the statistics workspace");
    return prep_v_fp8_dense(v, v_image, v_scale, v_mean, ws, nullptr, B, H, L, D, v_sb, v_sh, v_sl, scale_max, dtype, stream);
}

// FP8 V image of a dense, right-padded batch with a length per sample: statistics and scales over tokens < clamp(kv_lens[b], 0, L), the image
// laid out as sage_prep_v_fp8's for L tokens ([B, H, ceil(L / 64)] tiles); in the tile that holds a sample's last token the positions past it
// are zero, the tiles behind it stay unwritten, a sample without tokens gets scales of 0.  No smooth_v.  ws: sage_stats_ws_floats(B, H, L, D).
SAGE_API int sage_prep_v_fp8_kvlens(const void *v, void *v_image, float *v_scale, float *ws, const int32_t *kv_lens,
                                    int B, int H, int L, int D, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                                    float scale_max, int dtype, void *stream)
{
    SAGE_REQUIRE(v_scale && ws && kv_lens, "sage_prep_v_fp8_kvlens needs v_scale, the statistics workspace and kv_lens");
    return prep_v_fp8_dense(v, v_image, v_scale, nullptr, ws, kv_lens, B, H, L, D, v_sb, v_sh, v_sl, scale_max, dtype, stream);
}

// per-sequence V statistics of a packed batch: the stage-1 partials (the slab map's layout [1,H,nslab_bound], or nslab_bound = 0: without a
// map, [nseq,H,ceil(max_seqlen/512)]), then the final block [nseq,H,3,D]
static int64_t prep_v_varlen_partials(int nseq, int H, int max_seqlen, int nslab_bound, int D)
{
    if (nslab_bound > 0) return (int64_t)H * nslab_bound * 3 * D;
    return (int64_t)nseq * H * stats_slabs(max_seqlen) * 3 * D;
}

SAGE_API int64_t sage_prep_v_fp8_varlen_ws_floats(int nseq, int H, int max_seqlen, int nslab_bound, int D)
{
    if (nseq < 1 || H < 1 || max_seqlen < 1 || nslab_bound < 0 || D < 1) return 0;
    return prep_v_varlen_partials(nseq, H, max_seqlen, nslab_bound, D) + (int64_t)nseq * H * 3 * D;
}

SAGE_API int sage_prep_v_fp8_varlen(const void *v, void *v_image, float *v_scale, float *ws, const int32_t *cu_seqlens, const int32_t *cu_tiles,
                                    const int32_t *slab_first, const int32_t *slab_seq, const int32_t *hdr,
                                    int nseq, int total_tokens, int max_seqlen, int nslab_bound, int H, int D, int64_t v_sl, int64_t v_sh,
                                    float scale_max, int dtype, void *stream)
{
    SAGE_REQUIRE(v && v_image && v_scale && ws && cu_seqlens && cu_tiles, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(nseq >= 1 && H > 0 && total_tokens > 0 && max_seqlen > 0, "empty problem (nseq=%d H=%d total_tokens=%d max_seqlen=%d)",
                 nseq, H, total_tokens, max_seqlen);
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16(v) && aligned16(v_image), "v / v_image must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, v_sl, v_sh), "v strides must be multiples of 8 elements");
    SAGE_REQUIRE(scale_max > 0.0f, "scale_max must be positive");
    const bool map = slab_seq != nullptr;
    SAGE_REQUIRE((slab_first != nullptr) == map && (hdr != nullptr) == map, "the slab map comes as (slab_first, slab_seq, hdr) together");
    SAGE_REQUIRE(!map || (nseq <= sage::kVarlenPlanMaxSeq && nslab_bound >= stats_slabs(total_tokens)),
                 "slab map: nseq <= %d and nslab_bound >= ceil(total_tokens / %d) (got nseq=%d nslab_bound=%d)", sage::kVarlenPlanMaxSeq,
                 sage::kStatsSlab, nseq, nslab_bound);
    SAGE_REQUIRE(map || nslab_bound == 0, "nslab_bound is the slab map's (0 without one)");
    sage::StatsParams st{};
    st.x = v; st.ws = ws; st.stats = ws + prep_v_varlen_partials(nseq, H, max_seqlen, nslab_bound, D); st.mean_out = nullptr;
    st.B = nseq; st.H = H; st.L = total_tokens; st.D = D;
    st.nslab = map ? nslab_bound : stats_slabs(max_seqlen);
    st.x_sb = 0; st.x_sh = v_sh; st.x_sl = v_sl; st.dtype = dtype;
    st.cu = cu_seqlens; st.slab_first = slab_first; st.slab_seq = slab_seq; st.hdr = hdr; st.nseq = nseq; st.seq_stats = 1;
    if (const int rc = check_launch(sage::launch_stats(st, static_cast<hipStream_t>(stream)), "sage_v_stats_varlen launch")) return rc;
    return prep_v_common(v, v_image, v_scale, nullptr, nullptr, st.stats, cu_seqlens, cu_tiles, nseq, H, max_seqlen, D, 0, v_sh, v_sl,
                         scale_max, dtype, 1, stream);
}

SAGE_API int64_t sage_prepass_ws_floats(int B, int H, int L, int D)
{
    const int64_t nslab = stats_slabs(L);
    return 2 * (int64_t)B * H * nslab * 3 * D;
}

SAGE_API int64_t sage_prepass_sync_words(int B, int H) { return 2 * (int64_t)B * H * sage::kPrepassSyncStride; }

// Longest head the in-launch barrier takes on the current device: at most kPrepassMaxSlabs slabs, and never more than one per
// compute unit of the device (or partition) the caller runs on -- every slab of a head must be able to be resident while its
// head-mates arrive, with room left for the workgroups of the heads before it (2 resident workgroups per CU at D = 128).
static int g_prepass_debug_fail = 0;
SAGE_API void sage_debug_prepass_fail(int on) { g_prepass_debug_fail = on ? 1 : 0; }

// compute units a launch on `stream` can use: the stream's CU mask if it has one (hipExtStreamCreateWithCUMask), else the device's
static int stream_cu_count(hipStream_t stream, int dev)
{
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    uint32_t mask[16] = {0};
    if (hipExtStreamGetCUMask(stream, 16, mask) == hipSuccess) {
        int bits = 0;
        for (int i = 0; i < 16; i++) bits += __builtin_popcount(mask[i]);
        if (bits > 0 && bits < cus) cus = bits;
    }
    (void)hipGetLastError();
    return cus;
}
// the slabs that wait for each other inside a fused pre-pass launch must be co-resident: the compute units its stream may use
static int prepass_stream_cus(void *stream, int &cus)
{
    int dev = 0;
    SAGE_REQUIRE(hipGetDevice(&dev) == hipSuccess, "no current device");
    cus = stream_cu_count(static_cast<hipStream_t>(stream), dev);
    return SAGE_OK;
}
static int prepass_max_seqlen_of(int cus) { return (cus < sage::kPrepassMaxSlabs ? cus : sage::kPrepassMaxSlabs) * sage::kStatsSlab; }

SAGE_API int sage_prepass_max_seqlen(void)
{
    static thread_local int cached_dev = -1, cached_len = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (dev != cached_dev) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        cached_len = prepass_max_seqlen_of(cus);
        cached_dev = dev;
    }
    return cached_len;
}

// one device-visible word of pinned host memory for the `host_flag` argument below (owned by the caller: the library keeps no handle)
SAGE_API int sage_host_word_alloc(void **host_ptr, void **device_ptr)
{
    SAGE_REQUIRE(host_ptr && device_ptr, "null output pointer");
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocPortable);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) { if (h) (void)hipHostFree(h); return sage::set_last_error(SAGE_ELAUNCH, "sage_host_word_alloc: %s", hipGetErrorString(e)); }
    *static_cast<volatile uint32_t *>(h) = 0u;
    *host_ptr = h; *device_ptr = d;
    return SAGE_OK;
}
SAGE_API int sage_host_word_free(void *host_ptr)
{
    if (host_ptr == nullptr) return SAGE_OK;
    const hipError_t e = hipHostFree(host_ptr);
    return e == hipSuccess ? SAGE_OK : sage::set_last_error(SAGE_ELAUNCH, "sage_host_word_free: %s", hipGetErrorString(e));
}

SAGE_API int sage_prepass_max_seqlen_stream(void *stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    return prepass_max_seqlen_of(stream_cu_count(static_cast<hipStream_t>(stream), dev));
}

SAGE_API int sage_prepass_failed_heads(const uint32_t *sync, int B, int H, void *stream)
{
    if (!sync || B <= 0 || H <= 0) return sage::set_last_error(SAGE_EINVAL, "bad arguments");
    const size_t words = (size_t)2 * B * H * sage::kPrepassSyncStride;
    uint32_t *host = static_cast<uint32_t *>(malloc(words * sizeof(uint32_t)));
    if (!host) return sage::set_last_error(SAGE_ELAUNCH, "out of host memory");
    hipError_t e = hipMemcpyAsync(host, sync, words * sizeof(uint32_t), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    int n = 0;
    if (e == hipSuccess)
        for (size_t i = 0; i < (size_t)2 * B * H; i++) n += host[i * sage::kPrepassSyncStride + 2] != 0;
    free(host);
    if (e != hipSuccess) return sage::set_last_error(SAGE_ELAUNCH, "sage_prepass_failed_heads: %s", hipGetErrorString(e));
    return n;
}

SAGE_API int sage_prepass_kv(const void *k, const void *v, void *k_mean, int8_t *k_int8, float *k_scale,
                    void *v_image, float *v_scale, float *v_mean, float *ws, uint32_t *sync,
                    int B, int H, int L, int D,
                    int64_t k_sb, int64_t k_sh, int64_t k_sl, int64_t v_sb, int64_t v_sh, int64_t v_sl,
                    int64_t ko_sb, int64_t ko_sh, int64_t ko_sl,
                    int k_blk, int qk_quant_gran, int k_style, float scale_max, int v_fp16, int dtype, uint32_t *host_flag, void *stream)
{
    SAGE_REQUIRE(k || v, "nothing to do: both k and v are null");
    SAGE_REQUIRE(ws && sync, "the fused pre-pass needs its workspace and its sync buffer");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(B > 0 && H > 0 && L > 0, "empty tensor");
    SAGE_REQUIRE(B <= 32767 && H <= 65535, "batch / head count too large for one launch (%d, %d)", B, H);
    SAGE_REQUIRE(L <= sage_prepass_max_seqlen(), "sequence too long for the in-launch head barrier (%d > %d): use the "
                 "sage_channel_mean / sage_quant_qk_int8 / sage_prep_v_fp8 sequence", L, sage_prepass_max_seqlen());
    int cus = 0;            // the slabs of a head must be co-resident: a stream restricted to a CU mask has fewer compute units than the device
    if (const int rc = prepass_stream_cus(stream, cus)) return rc;
    SAGE_REQUIRE(stats_slabs(L) <= cus, "a head of %d slabs cannot be co-resident on the %d compute units this stream may use: use the "
                 "sage_channel_mean / sage_quant_qk_int8 / sage_prep_v_fp8 sequence", (int)stats_slabs(L), cus);
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    // rows of the last slab past L are read through the buffer range check: their 32-bit byte offsets must not wrap either
    const int64_t lpad = stats_slabs(L) * sage::kStatsSlab;
    sage::PrepassParams p{};
    p.parts = (k ? 1 : 0) | (v ? 2 : 0);
    if (k) {
        SAGE_REQUIRE(k_int8 && k_scale, "K part needs k_int8 and k_scale");
        SAGE_REQUIRE(aligned16(k) && aligned16(k_int8), "k / k_int8 must be 16-byte aligned");
        SAGE_REQUIRE(multiples_of(8, k_sl, k_sh, k_sb), "input strides must be multiples of 8 elements");
        SAGE_REQUIRE(multiples_of(16, ko_sl, ko_sh, ko_sb), "int8 output strides must be multiples of 16");
        SAGE_REQUIRE(((lpad - 1) * k_sl + D) * 2 < (int64_t)1 << 32 && (lpad - 1) * ko_sl + D < (int64_t)1 << 32,
                     "one head of k (rounded up to whole 512-row slabs) spans 4 GiB or more: the kernel addresses a head with 32-bit buffer offsets");
        SAGE_REQUIRE(k_blk == 64 || k_blk == 128, "k_blk must be 64 or 128 (got %d)", k_blk);
        SAGE_REQUIRE(k_style == sage::QS_CUDA || k_style == sage::QS_TRITON_THREAD || k_style == sage::QS_TRITON,
                     "k_style must be the Triton per-block (0), the CUDA (1) or the per-thread Triton (2) convention (got %d)", k_style);
        SAGE_REQUIRE(k_style != sage::QS_TRITON || qk_quant_gran == SAGE_GRAN_PER_BLOCK, "the Triton per-block convention goes with per-block scales");
        if (qk_quant_gran == SAGE_GRAN_PER_BLOCK) p.k_gran = sage::GR_BLOCK;
        else if (qk_quant_gran == SAGE_GRAN_PER_THREAD) p.k_gran = sage::GR_THREAD_K;
        else return sage::set_last_error(SAGE_EINVAL, "bad k granularity %d (per-block or per-thread)", qk_quant_gran);
    }
    if (v) {
        SAGE_REQUIRE(v_image && (v_scale || v_fp16), "V part needs v_image (and v_scale for the FP8 image)");
        SAGE_REQUIRE(aligned16(v) && aligned16(v_image), "v / v_image must be 16-byte aligned");
        SAGE_REQUIRE(multiples_of(8, v_sl, v_sh, v_sb), "input strides must be multiples of 8 elements");
        SAGE_REQUIRE(((lpad - 1) * v_sl + D) * 2 < (int64_t)1 << 32,
                     "one head of v (rounded up to whole 512-row slabs) spans 4 GiB or more: the kernel addresses a head with 32-bit buffer offsets");
        SAGE_REQUIRE(v_fp16 || scale_max > 0.0f, "scale_max must be positive");
        SAGE_REQUIRE(!(v_fp16 && v_mean), "the fp16 image has no smooth_v (use sage_prep_v_f16 with a mean for sub_mean)");
    }
    p.k = k; p.v = v; p.k_mean = k_mean; p.k_out = k_int8; p.k_scale = k_scale;
    p.v_image = v_image; p.v_scale = v_scale; p.v_mean = v_mean; p.ws = ws; p.sync = sync;
    p.B = B; p.H = H; p.L = L; p.D = D; p.nslab = stats_slabs(L);
    p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = v_sb; p.v_sh = v_sh; p.v_sl = v_sl;
    p.ko_sb = ko_sb; p.ko_sh = ko_sh; p.ko_sl = ko_sl;
    p.k_blk = k_blk; p.k_warp = k_blk; p.k_style = k_style; p.dtype = dtype; p.scale_max = scale_max; p.v_fp16 = v_fp16 ? 1 : 0;
    p.debug_fail = g_prepass_debug_fail;
    p.host_flag = host_flag;
    // the per-head counters and give-up flags start from zero in every launch (a launch that gave up leaves them dirty); launch_prepass_kv
    // zeroes them with a small kernel of its own (a hipMemsetAsync node replayed wrongly inside a captured HIP graph on ROCm 7.0)
    return check_launch(sage::launch_prepass_kv(p, static_cast<hipStream_t>(stream)), "sage_prepass_kv launch");
}

// packed (varlen) batches: K mean over all packed tokens + per-sequence INT8 K (Triton per-block rounding) + fp16 V tile image, one launch
SAGE_API int sage_prepass_kv_varlen(const void *k, const void *v, void *k_mean, int8_t *k_int8, float *k_scale, void *v_image,
                                    float *ws, uint32_t *sync, const int32_t *cu_seqlens_k, const int32_t *cu_k_scale,
                                    const int32_t *slab_first, const int32_t *slab_seq, const int32_t *hdr,
                                    int nseq, int total_tokens, int max_seqlen_k, int nslab_bound, int H, int D,
                                    int64_t k_sl, int64_t k_sh, int64_t v_sl, int64_t v_sh, int64_t ko_sl, int64_t ko_sh,
                                    int dtype, uint32_t *host_flag, void *stream)
{
    SAGE_REQUIRE(k && k_int8 && k_scale, "the varlen pre-pass needs k, k_int8 and k_scale");
    SAGE_REQUIRE(!v || v_image, "V part needs v_image");
    SAGE_REQUIRE(ws && sync, "the fused pre-pass needs its workspace and its sync buffer");
    SAGE_REQUIRE(cu_seqlens_k && cu_k_scale && slab_first && slab_seq && hdr, "the varlen pre-pass needs the index arrays of sage_varlen_plan");
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE(nseq > 0 && H > 0 && total_tokens > 0 && max_seqlen_k > 0 && nslab_bound > 0, "empty batch");
    SAGE_REQUIRE(H <= 65535, "head count too large for one launch (%d)", H);
    SAGE_REQUIRE(nslab_bound >= stats_slabs(total_tokens), "nslab_bound (%d) is below ceil(total_tokens / %d)", nslab_bound, sage::kStatsSlab);
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    int cus = 0;            // every slab of a head (all sequences) waits for the others when the K mean is asked for: they must be co-resident
    if (const int rc = prepass_stream_cus(stream, cus)) return rc;
    SAGE_REQUIRE(k_mean == nullptr || (nslab_bound <= sage::kPrepassMaxSlabs && nslab_bound <= cus),
                 "up to %d slabs per head cannot wait for each other inside one launch (limit %d, %d compute units on this stream): use the "
                 "sage_channel_mean / sage_quant_qk_int8_varlen / sage_prep_v_f16_varlen sequence", nslab_bound, sage::kPrepassMaxSlabs, cus);
    const int64_t lpad = stats_slabs(max_seqlen_k) * sage::kStatsSlab;
    SAGE_REQUIRE(aligned16(k) && aligned16(k_int8) && (!v || (aligned16(v) && aligned16(v_image))), "k / k_int8 / v / v_image must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, k_sl, k_sh) && (!v || multiples_of(8, v_sl, v_sh)), "input strides must be multiples of 8 elements");
    SAGE_REQUIRE(multiples_of(16, ko_sl, ko_sh), "int8 output strides must be multiples of 16");
    SAGE_REQUIRE(((lpad - 1) * k_sl + D) * 2 < (int64_t)1 << 32 && (lpad - 1) * ko_sl + D < (int64_t)1 << 32 &&
                 (!v || ((lpad - 1) * v_sl + D) * 2 < (int64_t)1 << 32),
                 "one sequence of one head (rounded up to whole 512-row slabs) spans 4 GiB or more: the kernel addresses it with 32-bit buffer offsets");
    sage::PrepassParams p{};
    p.parts = 1 | (v ? 2 : 0);
    p.k = k; p.v = v; p.k_mean = k_mean; p.k_out = k_int8; p.k_scale = k_scale;
    p.v_image = v_image; p.v_scale = nullptr; p.v_mean = nullptr; p.ws = ws; p.sync = sync;
    p.B = 1; p.H = H; p.L = total_tokens; p.D = D; p.nslab = nslab_bound;
    p.k_sb = 0; p.k_sh = k_sh; p.k_sl = k_sl; p.v_sb = 0; p.v_sh = v_sh; p.v_sl = v_sl;
    p.ko_sb = 0; p.ko_sh = ko_sh; p.ko_sl = ko_sl;
    p.k_blk = 64; p.k_warp = 64; p.k_gran = sage::GR_BLOCK; p.k_style = sage::QS_TRITON;      // quant_per_block_varlen.py:21-58
    p.dtype = dtype; p.scale_max = 448.0f; p.v_fp16 = 1;
    p.debug_fail = g_prepass_debug_fail;
    p.host_flag = host_flag;
    p.cu = cu_seqlens_k; p.cu_tiles = cu_k_scale; p.slab_seq = slab_seq; p.slab_first = slab_first; p.hdr = hdr; p.nseq = nseq;
    return check_launch(sage::launch_prepass_kv(p, static_cast<hipStream_t>(stream)), "sage_prepass_kv_varlen launch");
}

// test hook: `nwg` workgroups of 1024 threads that spin for `ms` milliseconds (two of them fill a compute unit's wave slots)
SAGE_API int sage_debug_spin(int ms, int nwg, void *stream)
{
    SAGE_REQUIRE(ms > 0 && ms <= 10000 && nwg > 0 && nwg <= 4096, "sage_debug_spin: bad argument");
    return check_launch(sage::launch_debug_spin(ms, nwg, static_cast<hipStream_t>(stream)), "sage_debug_spin launch");
}

SAGE_API int sage_prep_v_f16(const void *v, void *v_image, const float *v_mean, int B, int H, int L, int D,
                    int64_t v_sb, int64_t v_sh, int64_t v_sl, int dtype, void *stream)
{
    return prep_v_common(v, v_image, nullptr, nullptr, v_mean, nullptr, nullptr, nullptr, B, H, L, D, v_sb, v_sh, v_sl,
                         0.0f, dtype, 0, stream);
}

SAGE_API int sage_prep_v_f16_varlen(const void *v, void *v_image, const int32_t *cu_seqlens, const int32_t *cu_tiles,
                           int nseq, int max_seqlen, int H, int D, int64_t v_sl, int64_t v_sh, int dtype, void *stream)
{
    SAGE_REQUIRE(cu_seqlens && cu_tiles, "varlen needs cu_seqlens and cu_tiles");
    return prep_v_common(v, v_image, nullptr, nullptr, nullptr, nullptr, cu_seqlens, cu_tiles, nseq, H, max_seqlen, D, 0, v_sh, v_sl,
                         0.0f, dtype, 0, stream);
}

SAGE_API int64_t sage_attn_launch_ws_bytes(void) { return sage::kAttnSchedBytes; }

// ---- INT8 q with its scales
SAGE_API int sage_attn_qk_int8_pv_f8(const int8_t *q, const int8_t *k, const void *v_image, void *o, float *lse,
                            const float *q_scale, const float *k_scale, const float *v_scale, const float *v_mean,
                            int B, int Hq, int Hkv, int Lq, int Lk, int D,
                            int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                            int64_t o_sb, int64_t o_sh, int64_t o_sl,
                            int is_causal, int qk_quant_gran, int q_warp,
                            float sm_scale_log2, int pv_accum, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = true;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.q_scale = q_scale; c.k_scale = k_scale; c.v_scale = v_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.gran = qk_quant_gran; c.q_warp = q_warp; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = pv_accum;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_qk_int8_pv_f16(const int8_t *q, const int8_t *k, const void *v_image, void *o, float *lse,
                             const float *q_scale, const float *k_scale, const float *v_mean,
                             int B, int Hq, int Hkv, int Lq, int Lk, int D,
                             int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                             int64_t o_sb, int64_t o_sh, int64_t o_sl,
                             int is_causal, int qk_quant_gran, int q_warp,
                             float sm_scale_log2, int pv_accum, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = false;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.q_scale = q_scale; c.k_scale = k_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.gran = qk_quant_gran; c.q_warp = q_warp; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = pv_accum;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_qk_int8_pv_f16_vrows(const int8_t *q, const int8_t *k, const void *v, void *o, float *lse,
                                   const float *q_scale, const float *k_scale, const float *v_mean,
                                   int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                   int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                   int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                   int is_causal, int qk_quant_gran, int q_warp,
                                   float sm_scale_log2, int pv_accum, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const Strides vs = {v_sb, v_sh, v_sl};
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = false;
    c.q = q; c.k = k; c.v = v; c.v_rows = &vs; c.o = o; c.lse = lse; c.q_scale = q_scale; c.k_scale = k_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.gran = qk_quant_gran; c.q_warp = q_warp; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = pv_accum;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_qk_int8_pv_f16_masked(const int8_t *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                    const float *q_scale, const float *k_scale, const void *mask, int mask_kind,
                                    int64_t m_sb, int64_t m_sh, int64_t m_sq, int64_t m_sk,
                                    int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                    int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                    int64_t o_sb, int64_t o_sh, int64_t o_sl, float sm_scale_log2, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const MaskArg m{mask, mask_kind, m_sb, m_sh, m_sq, m_sk};
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = false;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.q_scale = q_scale; c.k_scale = k_scale; c.mask = &m;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = 0; c.gran = SAGE_GRAN_PER_BLOCK; c.q_warp = 128; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = SAGE_PV_ACCUM_TRITON;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_qk_int8_pv_f16_varlen(const int8_t *q, const int8_t *k, const void *v_image, void *o,
                                    const float *q_scale, const float *k_scale,
                                    const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                                    const int32_t *cu_q_scale, const int32_t *cu_k_scale, const int32_t *seq_order,
                                    const int32_t *work_items, const int32_t *work_hdr, int items_bound,
                                    int nseq, int max_seqlen_q, int Hq, int Hkv, int D,
                                    int64_t q_sl, int64_t q_sh, int64_t k_sl, int64_t k_sh, int64_t o_sl, int64_t o_sh,
                                    int is_causal, float sm_scale_log2, int pv_accum, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = false;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.q_scale = q_scale; c.k_scale = k_scale;
    c.varlen = true; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.cu_qs = cu_q_scale; c.cu_ks = cu_k_scale; c.seq_order = seq_order;
    c.work_items = work_items; c.work_hdr = work_hdr; c.items_bound = items_bound;
    c.B = nseq; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {0, k_sh, k_sl}; c.os = {0, o_sh, o_sl};
    c.is_causal = is_causal; c.gran = SAGE_GRAN_PER_BLOCK; c.q_warp = 128; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = pv_accum;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_qk_int8_pv_f8_varlen(const int8_t *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                            const float *q_scale, const float *k_scale, const float *v_scale,
                                            const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k,
                                            const int32_t *cu_q_scale, const int32_t *cu_k_scale, const int32_t *seq_order,
                                            const int32_t *work_items, const int32_t *work_hdr, int items_bound,
                                            int nseq, int max_seqlen_q, int Hq, int Hkv, int D,
                                            int64_t q_sl, int64_t q_sh, int64_t k_sl, int64_t k_sh, int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                            int is_causal, float sm_scale_log2, int pv_accum, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_INT8; c.pv_fp8 = true;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.lse_sh = lse_sh; c.q_scale = q_scale; c.k_scale = k_scale; c.v_scale = v_scale;
    c.varlen = true; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.cu_qs = cu_q_scale; c.cu_ks = cu_k_scale; c.seq_order = seq_order;
    c.work_items = work_items; c.work_hdr = work_hdr; c.items_bound = items_bound;
    c.B = nseq; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {0, k_sh, k_sl}; c.os = {0, o_sh, o_sl};
    c.is_causal = is_causal; c.gran = SAGE_GRAN_PER_BLOCK; c.q_warp = 128; c.sm_scale_log2 = sm_scale_log2; c.pv_accum = pv_accum;
    c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// ---- q in fp16 / bf16, quantised per thread group in the kernel prologue; dense.  FP8 PV: two-level accumulation; FP16 PV: straight FP32
// accumulation, the CUDA kernel form
SAGE_API int sage_attn_fused_q_pv_f8(const void *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const float *v_mean,
                                     int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                     int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_q_pv_f8_kvlens(const void *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                            const float *k_scale, const float *v_scale, const float *v_mean, const int32_t *kv_lens,
                                            int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                            int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                            int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                            int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    SAGE_REQUIRE(kv_lens, "sage_attn_fused_q_pv_f8_kvlens: null kv_lens");
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.v_mean = v_mean; c.kv_lens = kv_lens;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_attn_fused_q_pv_f8_kvlens on a pool of pages (include/sage_kvpaged_gfx950.h): the same call, Lk = the logical capacity, the paged kernels
SAGE_KVPAGED_API int sage_kvpaged_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                       const float *k_scale, const float *v_scale, const int32_t *kv_lens,
                                       const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                       int B, int Hq, int Hkv, int Lq, int D,
                                       int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                       int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                       int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "sage_kvpaged_attn: null tensor pointer (only lse may be null)");
    SAGE_REQUIRE(kv_lens, "sage_kvpaged_attn: null kv_lens");
    const char *const e = "sage_kvpaged_attn";
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_kvpaged_attn over packed query rows (include/sage_kvpvarlen_gfx950.h): the ragged paged kernels, Lq = max_seqlen_q sizing the dense grid
SAGE_KVPVARLEN_API int sage_kvpvarlen_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                           const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                           const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                           int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                           int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                           int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                           int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const char *const e = "sage_kvpvarlen_attn";
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "%s: null tensor pointer (only lse may be null)", e);
    SAGE_REQUIRE(kv_lens, "%s: null kv_lens", e);
    SAGE_REQUIRE(cu_seqlens_q, "%s: null cu_seqlens_q", e);
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(cu_seqlens_q) & 3u) == 0, "%s: cu_seqlens_q must be 4-byte aligned", e);
    SAGE_REQUIRE(total_q >= 1 && max_seqlen_q >= 1, "%s: total_q and max_seqlen_q must be at least 1 (got %d, %d)", e, total_q, max_seqlen_q);
    SAGE_REQUIRE(is_causal == 1, "%s: is_causal must be 1 (packed query rows are placed by their offsets; got %d)", e, is_causal);
    SAGE_REQUIRE(Hq >= 1 && (int64_t)B * Hq * ((max_seqlen_q + 127) / 128) < ((int64_t)1 << 31), "%s: B * Hq * ceil(max_seqlen_q / 128) must be in [1, 2^31) (got %d, %d, %d)",
                 e, B, Hq, max_seqlen_q);
    SAGE_REQUIRE(lse == nullptr || lse_sh >= total_q, "%s: lse is [Hq, total_q]: its head stride lse_sh must be at least total_q (got %lld)", e, (long long)lse_sh);
    const sage::RaggedArgs r{cu_seqlens_q, total_q};
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g; c.ragged = &r;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {0, o_sh, o_sl}; c.lse_sh = lse_sh;
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_kvpvarlen_attn as one call per engine step (include/sage_kvstep_gfx950.h): the same operands, the decode rows of a GQA
// group packed four heads to a workgroup, the longer samples on the 128-row kernel -- sorted on the device by a band filter, two launches
SAGE_KVSTEP_API int sage_kvstep_abi_version(void) { return SAGE_KVSTEP_ABI_VERSION; }

SAGE_KVSTEP_API int sage_kvstep_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                     const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                     int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                     int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const char *const e = "sage_kvstep_attn";
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "%s: null tensor pointer (only lse may be null)", e);
    SAGE_REQUIRE(kv_lens, "%s: null kv_lens", e);
    SAGE_REQUIRE(cu_seqlens_q, "%s: null cu_seqlens_q", e);
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(cu_seqlens_q) & 3u) == 0, "%s: cu_seqlens_q must be 4-byte aligned", e);
    SAGE_REQUIRE(total_q >= 1 && max_seqlen_q >= 1, "%s: total_q and max_seqlen_q must be at least 1 (got %d, %d)", e, total_q, max_seqlen_q);
    SAGE_REQUIRE(is_causal == 1, "%s: is_causal must be 1 (packed query rows are placed by their offsets; got %d)", e, is_causal);
    SAGE_REQUIRE(Hq >= 1 && (int64_t)B * Hq * ((max_seqlen_q + 127) / 128) < ((int64_t)1 << 31), "%s: B * Hq * ceil(max_seqlen_q / 128) must be in [1, 2^31) (got %d, %d, %d)",
                 e, B, Hq, max_seqlen_q);
    SAGE_REQUIRE(lse == nullptr || lse_sh >= total_q, "%s: lse is [Hq, total_q]: its head stride lse_sh must be at least total_q (got %lld)", e, (long long)lse_sh);
    SAGE_REQUIRE(Hq / Hkv >= 2, "%s: Hq / Hkv must be at least 2, no GQA group to pack (got Hq %d, Hkv %d; sage_kvpvarlen_attn takes such a call)", e, Hq, Hkv);
    const sage::RaggedArgs r{cu_seqlens_q, total_q};
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g; c.ragged = &r;
    c.step = true;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {0, o_sh, o_sl}; c.lse_sh = lse_sh;
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_kvstep_attn with its launches over device-built work lists, heaviest first (include/sage_kvlist_gfx950.h)
SAGE_KVLIST_API int sage_kvlist_abi_version(void) { return SAGE_KVLIST_ABI_VERSION; }

SAGE_KVLIST_API int64_t sage_kvlist_ws_bytes(int B, int total_q, int max_seqlen_q)
{
    if (B < 1 || total_q < 1 || max_seqlen_q < 1) return sage::set_last_error(SAGE_EINVAL, "sage_kvlist_ws_bytes: B, total_q and max_seqlen_q must be at least 1 (got %d, %d, %d)", B, total_q, max_seqlen_q);
    return 4 * sage::step_ws_words(B, total_q, max_seqlen_q);
}

// the checks sage_kvlist_plan and sage_kvlist_plan_host share (`e`: the entry's name); fills the plan's parameters
static int kvlist_plan_args(const char *e, const int32_t *cu_seqlens_q, const int32_t *kv_lens, const int32_t *q_start, int B, int total_q, int max_seqlen_q,
                            int capacity, int window, int Hq, int Hkv, int D, int32_t *list_ws, int64_t list_ws_bytes, sage::KvListPlanParams &lp)
{
    SAGE_REQUIRE(cu_seqlens_q && kv_lens && q_start, "%s: null cu_seqlens_q, kv_lens or q_start", e);
    SAGE_REQUIRE(((reinterpret_cast<uintptr_t>(cu_seqlens_q) | reinterpret_cast<uintptr_t>(kv_lens) | reinterpret_cast<uintptr_t>(q_start)) & 3u) == 0,
                 "%s: cu_seqlens_q, kv_lens and q_start must be 4-byte aligned", e);
    SAGE_REQUIRE(B >= 1 && B <= sage::kVarlenPlanMaxSeq, "%s: B must be in 1 .. %d (got %d)", e, sage::kVarlenPlanMaxSeq, B);
    SAGE_REQUIRE(total_q >= 1 && max_seqlen_q >= 1 && capacity >= 1, "%s: total_q, max_seqlen_q and capacity must be at least 1 (got %d, %d, %d)", e, total_q, max_seqlen_q, capacity);
    SAGE_REQUIRE(window >= 0, "%s: window = %d: the number of keys a row sees up to its diagonal, 0 = unbounded", e, window);
    SAGE_REQUIRE(Hq >= 1 && Hkv >= 1 && Hq % Hkv == 0, "%s: Hq (%d) must be divisible by Hkv (%d)", e, Hq, Hkv);
    SAGE_REQUIRE_HEAD_DIM(D, "");
    SAGE_REQUIRE((int64_t)B * Hq * ((max_seqlen_q + 127) / 128) < ((int64_t)1 << 31), "%s: B * Hq * ceil(max_seqlen_q / 128) must be below 2^31 (got %d, %d, %d)", e, B, Hq, max_seqlen_q);
    const long long need = 4 * sage::step_ws_words(B, total_q, max_seqlen_q);
    SAGE_REQUIRE(list_ws != nullptr && (reinterpret_cast<uintptr_t>(list_ws) & 3u) == 0 && list_ws_bytes >= need,
                 "%s: list_ws is %lld bytes of int32 memory, 4-byte aligned (got %lld bytes at %p)", e, need, (long long)list_ws_bytes, (void *)list_ws);
    lp = sage::KvListPlanParams{};
    lp.cu_q = cu_seqlens_q; lp.kv_lens = kv_lens; lp.q_start = q_start;
    lp.B = B; lp.total_q = total_q; lp.max_seqlen_q = max_seqlen_q; lp.Lk = capacity; lp.window = window;
    lp.Hq = Hq; lp.Hkv = Hkv; lp.head_dim = D; lp.items_cap = (int)sage::step_chunk_bound(B, total_q, max_seqlen_q); lp.ws = list_ws;
    return SAGE_OK;
}

SAGE_KVLIST_API int sage_kvlist_plan(const int32_t *cu_seqlens_q, const int32_t *kv_lens, const int32_t *q_start,
                                     int B, int total_q, int max_seqlen_q, int capacity, int window, int Hq, int Hkv, int D,
                                     int32_t *list_ws, int64_t list_ws_bytes, void *stream)
{
    sage::KvListPlanParams lp;
    if (const int rc = kvlist_plan_args("sage_kvlist_plan", cu_seqlens_q, kv_lens, q_start, B, total_q, max_seqlen_q, capacity, window, Hq, Hkv, D, list_ws, list_ws_bytes, lp)) return rc;
    return check_launch(sage::launch_kv_list_plan(lp, static_cast<hipStream_t>(stream)), "sage_kvlist_plan launch");
}

SAGE_KVLIST_API int sage_kvlist_plan_host(const int32_t *cu_seqlens_q, const int32_t *kv_lens, const int32_t *q_start,
                                          int B, int total_q, int max_seqlen_q, int capacity, int window, int Hq, int Hkv, int D,
                                          int32_t *list_ws, int64_t list_ws_bytes, int *decode_grid, int *chunk_grid)
{
    sage::KvListPlanParams lp;
    if (const int rc = kvlist_plan_args("sage_kvlist_plan_host", cu_seqlens_q, kv_lens, q_start, B, total_q, max_seqlen_q, capacity, window, Hq, Hkv, D, list_ws, list_ws_bytes, lp)) return rc;
    int scratch[3 * sage::kVarlenPlanMaxSeq];
    sage::step_plan_serial(cu_seqlens_q, kv_lens, q_start, B, total_q, max_seqlen_q, capacity, window, Hq, Hkv, D, lp.items_cap,
                           scratch, scratch + sage::kVarlenPlanMaxSeq, scratch + 2 * sage::kVarlenPlanMaxSeq, list_ws);
    if (decode_grid != nullptr) *decode_grid = (int)sage::step_decode_grid(B, Hkv, Hq / Hkv);
    if (chunk_grid != nullptr) *chunk_grid = max_seqlen_q > sage::kStepDecodeRows ? (int)sage::step_chunk_grid(Hq, lp.items_cap) : 0;
    return SAGE_OK;
}

SAGE_KVLIST_API int sage_kvlist_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                     const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                     int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                     int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr,
                                     int32_t *list_ws, int64_t list_ws_bytes)
{
    const char *const e = "sage_kvlist_attn";
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "%s: null tensor pointer (only lse may be null)", e);
    SAGE_REQUIRE(kv_lens, "%s: null kv_lens", e);
    SAGE_REQUIRE(cu_seqlens_q, "%s: null cu_seqlens_q", e);
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(cu_seqlens_q) & 3u) == 0, "%s: cu_seqlens_q must be 4-byte aligned", e);
    SAGE_REQUIRE(total_q >= 1 && max_seqlen_q >= 1, "%s: total_q and max_seqlen_q must be at least 1 (got %d, %d)", e, total_q, max_seqlen_q);
    SAGE_REQUIRE(is_causal == 1, "%s: is_causal must be 1 (packed query rows are placed by their offsets; got %d)", e, is_causal);
    SAGE_REQUIRE(Hq >= 1 && (int64_t)B * Hq * ((max_seqlen_q + 127) / 128) < ((int64_t)1 << 31), "%s: B * Hq * ceil(max_seqlen_q / 128) must be in [1, 2^31) (got %d, %d, %d)",
                 e, B, Hq, max_seqlen_q);
    SAGE_REQUIRE(lse == nullptr || lse_sh >= total_q, "%s: lse is [Hq, total_q]: its head stride lse_sh must be at least total_q (got %lld)", e, (long long)lse_sh);
    SAGE_REQUIRE(Hq / Hkv >= 2, "%s: Hq / Hkv must be at least 2, no GQA group to pack (got Hq %d, Hkv %d; sage_kvpvarlen_attn takes such a call)", e, Hq, Hkv);
    const sage::RaggedArgs r{cu_seqlens_q, total_q};
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g; c.ragged = &r;
    c.step = true; c.list = true; c.list_ws = list_ws; c.list_ws_bytes = list_ws_bytes;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {0, o_sh, o_sl}; c.lse_sh = lse_sh;
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_kvlist_attn with every decode sequence as S key-range chunks, exactly (include/sage_kvlsplit_gfx950.h)
SAGE_KVLSPLIT_API int sage_kvlsplit_abi_version(void) { return SAGE_KVLSPLIT_ABI_VERSION; }

SAGE_KVLSPLIT_API int64_t sage_kvlsplit_ws_bytes(int B, int Hq, int max_seqlen_q, int D, int S)
{
    if (B < 1 || Hq < 1 || max_seqlen_q < 1 || (D != 64 && D != 128) || S < 2 || S > 255)
        return sage::set_last_error(SAGE_EINVAL, "sage_kvlsplit_ws_bytes: B, Hq and max_seqlen_q at least 1, D 64 or 128, S in 2 .. 255 (got %d, %d, %d, %d, %d)", B, Hq, max_seqlen_q, D, S);
    return kv_split_ws_bytes(B, Hq, sage::step_split_ws_rows(max_seqlen_q), D, S);
}

SAGE_KVLSPLIT_API int sage_kvlsplit_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                     const float *k_scale, const float *v_scale, const int32_t *kv_lens, const int32_t *cu_seqlens_q,
                                     const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                     int B, int Hq, int Hkv, int total_q, int max_seqlen_q, int D,
                                     int64_t q_sl, int64_t q_sh, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                     int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                     int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr,
                                     int32_t *list_ws, int64_t list_ws_bytes)
{
    const char *const e = "sage_kvlsplit_attn";
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "%s: null tensor pointer (only lse may be null)", e);
    SAGE_REQUIRE(kv_lens, "%s: null kv_lens", e);
    SAGE_REQUIRE(cu_seqlens_q, "%s: null cu_seqlens_q", e);
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    SAGE_REQUIRE((reinterpret_cast<uintptr_t>(cu_seqlens_q) & 3u) == 0, "%s: cu_seqlens_q must be 4-byte aligned", e);
    SAGE_REQUIRE(total_q >= 1 && max_seqlen_q >= 1, "%s: total_q and max_seqlen_q must be at least 1 (got %d, %d)", e, total_q, max_seqlen_q);
    SAGE_REQUIRE(is_causal == 1, "%s: is_causal must be 1 (packed query rows are placed by their offsets; got %d)", e, is_causal);
    SAGE_REQUIRE(Hq >= 1 && (int64_t)B * Hq * ((max_seqlen_q + 127) / 128) < ((int64_t)1 << 31), "%s: B * Hq * ceil(max_seqlen_q / 128) must be in [1, 2^31) (got %d, %d, %d)",
                 e, B, Hq, max_seqlen_q);
    SAGE_REQUIRE(lse == nullptr || lse_sh >= total_q, "%s: lse is [Hq, total_q]: its head stride lse_sh must be at least total_q (got %lld)", e, (long long)lse_sh);
    SAGE_REQUIRE(Hq / Hkv >= 2, "%s: Hq / Hkv must be at least 2, no GQA group to pack (got Hq %d, Hkv %d; sage_kvpvarlen_attn takes such a call)", e, Hq, Hkv);
    const sage::RaggedArgs r{cu_seqlens_q, total_q};
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g; c.ragged = &r;
    c.step = true; c.list = true; c.lsplit = true; c.list_ws = list_ws; c.list_ws_bytes = list_ws_bytes;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {0, o_sh, o_sl}; c.lse_sh = lse_sh;
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// sage_kvpaged_attn as the exact split (include/sage_kvpsplit_gfx950.h): SAGE_ATTR_KV_SPLIT required, pass 1 / pass 2 / merge through the table
SAGE_KVPSPLIT_API int sage_kvpsplit_abi_version(void) { return SAGE_KVPSPLIT_ABI_VERSION; }

SAGE_KVPSPLIT_API int sage_kvpsplit_attn(const void *q, const int8_t *k_int8, const void *v_image, void *o, float *lse,
                                         const float *k_scale, const float *v_scale, const int32_t *kv_lens,
                                         const int32_t *block_table, int64_t bt_stride, int num_pages, int page_size, int max_pages_per_seq,
                                         int B, int Hq, int Hkv, int Lq, int D,
                                         int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                         int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                         int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    SAGE_REQUIRE(q && k_int8 && v_image && o && k_scale && v_scale, "sage_kvpsplit_attn: null tensor pointer (only lse may be null)");
    SAGE_REQUIRE(kv_lens, "sage_kvpsplit_attn: null kv_lens");
    const char *const e = "sage_kvpsplit_attn";
    sage::PagedArgs g;
    if (const int rc = sage::paged_args(e, block_table, bt_stride, num_pages, page_size, max_pages_per_seq, g)) return rc;
    if (const int rc = sage::kv_check_batch(e, B, Hkv)) return rc;
    if (const int rc = sage::paged_check_table_aligned(e, block_table)) return rc;
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k_int8; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_scale = v_scale; c.kv_lens = kv_lens; c.paged = &g;
    c.paged_split = true;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = max_pages_per_seq * page_size; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_q_pv_f16(const void *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                      const float *k_scale, const float *v_mean,
                                      int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                      int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                      int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                      int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_SINGLE;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_q_pv_f16_vrows(const void *q, const int8_t *k, const void *v, void *o, float *lse, const float *k_scale,
                                            int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                            int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                            int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                            int is_causal, float sm_scale_log2, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const Strides vs = {v_sb, v_sh, v_sl};
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_SINGLE;
    c.q = q; c.k = k; c.v = v; c.v_rows = &vs; c.o = o; c.lse = lse; c.k_scale = k_scale;       // fp16 q / k / v tensors of one call
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = SAGE_DTYPE_F16; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// the (inexact) split: kv_split >= 2 chunks of Lk_chunk keys each, folded into the kv-head dimension; partial outputs and LSEs per chunk
static int split_check(int kv_split, const void *o_part, const float *lse_part, int Lk_chunk)
{
    SAGE_REQUIRE(kv_split >= 2, "kv_split must be at least 2 (got %d)", kv_split);
    SAGE_REQUIRE(o_part && lse_part, "split-KV needs the partial output and log-sum-exp buffers");
    SAGE_REQUIRE(Lk_chunk % 64 == 0, "split-KV chunks are whole numbers of 64-key tiles (got %d keys)", Lk_chunk);
    return SAGE_OK;
}

SAGE_API int sage_attn_fused_q_pv_f8_split(const void *q, const int8_t *k, const void *v_image, void *o_part, float *lse_part,
                                           const float *k_scale, const float *v_scale, const float *v_mean,
                                           int B, int Hq, int Hkv, int kv_split, int Lq, int Lk_chunk, int D,
                                           int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                           int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                           int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    if (const int rc = split_check(kv_split, o_part, lse_part, Lk_chunk)) return rc;
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true; c.pv_accum = SAGE_PV_ACCUM_TWO_LEVEL;
    c.q = q; c.k = k; c.v = v_image; c.o = o_part; c.lse = lse_part; c.k_scale = k_scale; c.v_scale = v_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq * kv_split; c.Hkv = Hkv * kv_split; c.kv_split = kv_split; c.Lq = Lq; c.Lk = Lk_chunk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_q_pv_f16_split(const void *q, const int8_t *k, const void *v_image, void *o_part, float *lse_part,
                                            const float *k_scale, const float *v_mean,
                                            int B, int Hq, int Hkv, int kv_split, int Lq, int Lk_chunk, int D,
                                            int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                            int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                            int is_causal, float sm_scale_log2, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    if (const int rc = split_check(kv_split, o_part, lse_part, Lk_chunk)) return rc;
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_SINGLE;
    c.q = q; c.k = k; c.v = v_image; c.o = o_part; c.lse = lse_part; c.k_scale = k_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq * kv_split; c.Hkv = Hkv * kv_split; c.kv_split = kv_split; c.Lq = Lq; c.Lk = Lk_chunk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.sm_scale_log2 = sm_scale_log2; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// ---- q in fp16 / bf16, quantised per 128-row block in the kernel prologue.  FP16 PV in the Triton kernel form, dense or packed; FP8 PV (ABI 22):
// packed batches only, v_scale [nseq,Hkv,D], pv_accum single / two-level, lse nullable [Hq, lse_sh] by packed row
SAGE_API int sage_attn_fused_qblock_pv_f16(const void *q, const int8_t *k, const void *v_image, void *o, float *lse, const float *k_scale,
                                           int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                           int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                           int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                           int is_causal, float q_premul, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_FUSED_BLOCK; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_TRITON;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.k_scale = k_scale;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.q_premul = q_premul; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_qblock_pv_f16_vrows(const void *q, const int8_t *k, const void *v, void *o, float *lse, const float *k_scale,
                                                 int B, int Hq, int Hkv, int Lq, int Lk, int D,
                                                 int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                                 int64_t v_sb, int64_t v_sh, int64_t v_sl, int64_t o_sb, int64_t o_sh, int64_t o_sl,
                                                 int is_causal, float q_premul, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    const Strides vs = {v_sb, v_sh, v_sl};
    AttnCall c{};
    c.q_form = Q_FUSED_BLOCK; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_TRITON;
    c.q = q; c.k = k; c.v = v; c.v_rows = &vs; c.o = o; c.lse = lse; c.k_scale = k_scale;
    c.B = B; c.Hq = Hq; c.Hkv = Hkv; c.Lq = Lq; c.Lk = Lk; c.D = D;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl}; c.os = {o_sb, o_sh, o_sl};
    c.is_causal = is_causal; c.q_premul = q_premul; c.q_dtype = SAGE_DTYPE_F16; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_qblock_pv_f16_varlen(const void *q, const int8_t *k, const void *v_image, void *o, const float *k_scale,
                                                  const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, const int32_t *cu_k_scale,
                                                  const int32_t *seq_order, const int32_t *work_items, const int32_t *work_hdr, int items_bound,
                                                  int nseq, int max_seqlen_q, int Hq, int Hkv, int D,
                                                  int64_t q_sl, int64_t q_sh, int64_t k_sl, int64_t k_sh, int64_t o_sl, int64_t o_sh,
                                                  int is_causal, float q_premul, int q_dtype, int out_dtype, void *stream, const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_FUSED_BLOCK; c.pv_fp8 = false; c.pv_accum = SAGE_PV_ACCUM_TRITON;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.k_scale = k_scale;
    c.varlen = true; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.cu_ks = cu_k_scale; c.seq_order = seq_order;
    c.work_items = work_items; c.work_hdr = work_hdr; c.items_bound = items_bound;
    c.B = nseq; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {0, k_sh, k_sl}; c.os = {0, o_sh, o_sl};
    c.is_causal = is_causal; c.q_premul = q_premul; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

SAGE_API int sage_attn_fused_qblock_pv_f8_varlen(const void *q, const int8_t *k, const void *v_image, void *o, float *lse,
                                                 const float *k_scale, const float *v_scale,
                                                 const int32_t *cu_seqlens_q, const int32_t *cu_seqlens_k, const int32_t *cu_k_scale,
                                                 const int32_t *seq_order, const int32_t *work_items, const int32_t *work_hdr, int items_bound,
                                                 int nseq, int max_seqlen_q, int Hq, int Hkv, int D,
                                                 int64_t q_sl, int64_t q_sh, int64_t k_sl, int64_t k_sh, int64_t o_sl, int64_t o_sh, int64_t lse_sh,
                                                 int is_causal, float q_premul, int pv_accum, int q_dtype, int out_dtype, void *stream,
                                                 const SageLaunchAttr *attr)
{
    AttnCall c{};
    c.q_form = Q_FUSED_BLOCK; c.pv_fp8 = true; c.pv_accum = pv_accum;
    c.q = q; c.k = k; c.v = v_image; c.o = o; c.lse = lse; c.lse_sh = lse_sh; c.k_scale = k_scale; c.v_scale = v_scale;
    c.varlen = true; c.cu_q = cu_seqlens_q; c.cu_k = cu_seqlens_k; c.cu_ks = cu_k_scale; c.seq_order = seq_order;
    c.work_items = work_items; c.work_hdr = work_hdr; c.items_bound = items_bound;
    c.B = nseq; c.Hq = Hq; c.Hkv = Hkv; c.Lq = max_seqlen_q; c.D = D;
    c.qs = {0, q_sh, q_sl}; c.ks = {0, k_sh, k_sl}; c.os = {0, o_sh, o_sl};
    c.is_causal = is_causal; c.q_premul = q_premul; c.q_dtype = q_dtype; c.out_dtype = out_dtype; c.stream = stream; c.attr = attr;
    return attn_run(c);
}

// the exact split (pass 1 / pass 2): the checks the two entries share
static int split_exact_check(const void *q, const int8_t *k, const float *k_scale, int B, int Hq, int Hkv, int kv_split, int Lq, int Lk, int D,
                             int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl, int q_dtype)
{
    SAGE_REQUIRE(q && k && k_scale, "null tensor pointer");
    SAGE_REQUIRE_HEAD_DIM(D, "; pad on the host as core.py:260-271 does");
    SAGE_REQUIRE(B > 0 && Hq > 0 && Hkv > 0 && Lq > 0 && Lk > 0, "empty problem (B=%d Hq=%d Hkv=%d Lq=%d Lk=%d)", B, Hq, Hkv, Lq, Lk);
    SAGE_REQUIRE(Hq % Hkv == 0, "num_qo_heads (%d) must be divisible by num_kv_heads (%d)", Hq, Hkv);
    SAGE_REQUIRE(kv_split >= 1 && Lk / 64 >= kv_split && (Lk / 64) % kv_split == 0,
                 "kv_split (%d) must divide the number of whole 64-key tiles (%d keys: %d tiles)", kv_split, Lk, Lk / 64);
    SAGE_REQUIRE((int64_t)B * Hq * kv_split * ((Lq + 127) / 128) < ((int64_t)1 << 31), "grid too large");
    SAGE_REQUIRE_DTYPE(q_dtype, "q_dtype");
    SAGE_REQUIRE(aligned16(q) && aligned16(k), "q/k must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, q_sl, q_sh, q_sb), "q strides must be multiples of 8 elements");
    SAGE_REQUIRE(multiples_of(16, k_sl, k_sh, k_sb), "int8 k strides must be multiples of 16");
    SAGE_REQUIRE(k_tile_fits_int(k_sl, D), "one 64-key tile of k must span less than 2 GiB (row stride %lld): the kernel addresses a tile's rows with 32-bit offsets",
                 (long long)k_sl);
    return SAGE_OK;
}

SAGE_API int sage_split_exact_chunk_max(const void *q, const int8_t *k, const float *k_scale, float *chunk_max,
                                        int B, int Hq, int Hkv, int kv_split, int Lq, int Lk, int D,
                                        int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                        int is_causal, float sm_scale_log2, int q_dtype, void *stream)
{
    if (const int rc = split_exact_check(q, k, k_scale, B, Hq, Hkv, kv_split, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, q_dtype)) return rc;
    SAGE_REQUIRE(chunk_max != nullptr, "null chunk_max buffer");
    sage::ChunkMaxParams p{};
    p.q = q; p.k = k; p.k_scale = k_scale; p.out = chunk_max;
    p.B = B; p.Hq = Hq; p.Hkv = Hkv; p.group = Hq / Hkv; p.Lq = Lq; p.Lk = Lk; p.D = D;
    p.S = kv_split; p.tiles = (Lk / 64) / kv_split;
    p.nks = ((Lk + 63) / 64) * 4;
    p.q_sb = q_sb; p.q_sh = q_sh; p.q_sl = q_sl; p.k_sb = k_sb; p.k_sh = k_sh; p.k_sl = k_sl;
    p.sm_scale_log2 = sm_scale_log2; p.q_dtype = q_dtype; p.causal = is_causal != 0;
    return check_launch(sage::launch_chunk_max(p, reinterpret_cast<hipStream_t>(stream)), "sage_split_exact_chunk_max launch");
}

SAGE_API int sage_attn_fused_q_pv_f8_split_exact(const void *q, const int8_t *k, const void *v_image, float *o_part, float *lse_part,
                                                 const float *k_scale, const float *v_scale, const float *v_mean, const float *chunk_max,
                                                 int B, int Hq, int Hkv, int kv_split, int tail, int Lq, int Lk, int D,
                                                 int64_t q_sb, int64_t q_sh, int64_t q_sl, int64_t k_sb, int64_t k_sh, int64_t k_sl,
                                                 int is_causal, float sm_scale_log2, int q_dtype, void *stream, const SageLaunchAttr *attr)
{
    LaunchAttr la;
    if (const int rc = read_attr(attr, stream, false, la)) return rc;
    SAGE_REQUIRE(!la.opts.fp8_folded, "the exact split takes the exact score form only (SAGE_ATTR_FP8_FOLDED_SCORES given)");
    SAGE_REQUIRE(la.q_start == nullptr, "SageLaunchAttr.q_start: sage_attn_fused_q_pv_f8_kvlens with is_causal = 1 and the exact score form only");
    SAGE_REQUIRE(la.window == 0, "SageLaunchAttr.window: sage_attn_fused_q_pv_f8_kvlens with is_causal = 1 and the exact score form only");
    SAGE_REQUIRE(!la.bottom_right, "SAGE_ATTR_CAUSAL_BOTTOM_RIGHT: sage_attn_fused_qblock_pv_f8_varlen with is_causal = 1 and SAGE_PV_ACCUM_TWO_LEVEL only");
    SAGE_REQUIRE(!la.gqa_pack, "SAGE_ATTR_GQA_PACK: sage_attn_fused_q_pv_f8_kvlens with Lq <= 32, Hq / Hkv >= 2 and the exact score form only");
    SAGE_REFUSE_KV_SPLIT(la);
    if (const int rc = split_exact_check(q, k, k_scale, B, Hq, Hkv, kv_split, Lq, Lk, D, q_sb, q_sh, q_sl, k_sb, k_sh, k_sl, q_dtype)) return rc;
    SAGE_REQUIRE(v_image && v_scale && o_part && lse_part && chunk_max, "null tensor pointer");
    SAGE_REQUIRE(tail == 0 || tail == 1, "tail must be 0 (the whole chunks) or 1 (the ragged tail), got %d", tail);
    SAGE_REQUIRE(tail == 0 || Lk % 64 != 0, "tail = 1 needs a ragged key range (Lk = %d is a multiple of 64)", Lk);
    SAGE_REQUIRE(aligned16(v_image) && aligned16(o_part), "v_image / o_part must be 16-byte aligned");
    const int nch = tail ? 1 : kv_split;                // chunks of this launch, folded into the kv-head dimension
    AttnCall c{};
    c.q_form = Q_FUSED_THREAD; c.pv_fp8 = true;
    c.q = q; c.k = k; c.v = v_image; c.o = o_part; c.lse = lse_part; c.k_scale = k_scale; c.v_scale = v_scale; c.v_mean = v_mean;
    c.B = B; c.Hq = Hq * nch; c.Hkv = Hkv * nch; c.kv_split = nch; c.Lq = Lq; c.D = D;
    c.Lk = tail ? Lk % 64 : (Lk / 64 / kv_split) * 64;
    c.qs = {q_sb, q_sh, q_sl}; c.ks = {k_sb, k_sh, k_sl};
    c.os = {(int64_t)c.Hq * Lq * D, (int64_t)Lq * D, D};      // FP32 partials [B, Hq * nch, Lq, D], contiguous
    c.sm_scale_log2 = sm_scale_log2; c.out_dtype = SAGE_DTYPE_F16;        // (unused: FP32 partials)
    sage::AttnParams p{};
    sage::AttnVariant v{};
    if (const int rc = set_q_form(c, p, v.kthread)) return rc;
    fill_geometry(c, v.kthread, p);       // (also sets p.nqs, which only kernels with q scales -- INT8 q -- read)
    p.nks = ((Lk + 63) / 64) * 4;        // the chunks read the unsplit operands in place: k scale slots per head of the unsplit call
    p.kv_base = tail ? (Lk / 64) * 64 : 0;
    p.seed_max = chunk_max; p.seed_chunks = kv_split; p.seed_first = tail ? kv_split : 0;
    v.head_dim = D; v.pv_fp8 = true; v.causal = is_causal != 0; v.two_level = true; v.qf = sage::attn_qf(false, q_dtype); v.seeded = true;
    return check_launch(sage::launch_attention(p, v, la.opts), "sage_attn_fused_q_pv_f8_split_exact launch");
}

SAGE_API int sage_merge_states(float *o_acc, float *lse_acc, const void *o_new, const float *lse_new, void *o_out,
                               int B, int H, int L, int D, int64_t n_sb, int64_t n_sh, int64_t n_sl,
                               int64_t o_sb, int64_t o_sh, int64_t o_sl, int dtype, int first, void *stream)
{
    SAGE_REQUIRE(o_acc && lse_acc && o_new && lse_new, "null tensor pointer");
    SAGE_REQUIRE(B > 0 && H > 0 && L > 0, "empty problem (B=%d H=%d L=%d)", B, H, L);
    SAGE_REQUIRE(D > 0 && D % 8 == 0 && D <= 512, "head_dim must be a positive multiple of 8, at most 512 (got %d)", D);
    SAGE_REQUIRE_DTYPE(dtype, "dtype");
    SAGE_REQUIRE(aligned16(o_acc) && aligned16(o_new) && (o_out == nullptr || aligned16(o_out)), "o tensors must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, n_sb, n_sh, n_sl), "o_new strides must be multiples of 8 elements");
    SAGE_REQUIRE(o_out == nullptr || multiples_of(8, o_sb, o_sh, o_sl), "o_out strides must be multiples of 8 elements");
    sage::MergeParams p{};
    p.o_acc = o_acc; p.lse_acc = lse_acc; p.o_new = o_new; p.lse_new = lse_new; p.o_out = o_out;
    p.B = B; p.H = H; p.L = L; p.D = D;
    p.n_sb = n_sb; p.n_sh = n_sh; p.n_sl = n_sl; p.o_sb = o_sb; p.o_sh = o_sh; p.o_sl = o_sl;
    p.dtype = dtype; p.first = first != 0;
    return check_launch(sage::launch_merge_states(p, reinterpret_cast<hipStream_t>(stream)), "sage_merge_states launch");
}

// the split-KV merge over fp16 partials (sage_merge_split) or over the exact split's FP32 partials (sage_merge_split_f32)
static int merge_split_common(bool f32, const void *o_part, const float *lse_part, const void *o_tail, const float *lse_tail,
                              void *o_out, float *lse_out, int B, int S, int H, int group, int L, int D,
                              int64_t o_sb, int64_t o_sh, int64_t o_sl, int out_dtype, void *stream)
{
    SAGE_REQUIRE(group > 0 && H % group == 0, "num heads (%d) must be divisible by the GQA group size (%d)", H, group);
    SAGE_REQUIRE(o_part && lse_part && o_out, "null tensor pointer");
    SAGE_REQUIRE((o_tail == nullptr) == (lse_tail == nullptr), "o_tail and lse_tail come together");
    SAGE_REQUIRE(B > 0 && S > 0 && H > 0 && L > 0, "empty problem (B=%d S=%d H=%d L=%d)", B, S, H, L);
    SAGE_REQUIRE(D > 0 && D % 8 == 0 && D <= 512, "head_dim must be a positive multiple of 8, at most 512 (got %d)", D);
    SAGE_REQUIRE_DTYPE(out_dtype, "out_dtype");
    SAGE_REQUIRE(aligned16(o_part) && aligned16(o_out) && (o_tail == nullptr || aligned16(o_tail)), "o tensors must be 16-byte aligned");
    SAGE_REQUIRE(multiples_of(8, o_sb, o_sh, o_sl), "o_out strides must be multiples of 8 elements");
    sage::SplitMergeParams p{};
    p.o_part = o_part; p.lse_part = lse_part; p.o_tail = o_tail; p.lse_tail = lse_tail; p.o_out = o_out; p.lse_out = lse_out;
    p.B = B; p.S = S; p.H = H; p.L = L; p.D = D; p.group = group; p.o_sb = o_sb; p.o_sh = o_sh; p.o_sl = o_sl; p.dtype = out_dtype;
    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return f32 ? check_launch(sage::launch_merge_split_f32(p, s), "sage_merge_split_f32 launch") : check_launch(sage::launch_merge_split(p, s), "sage_merge_split launch");
}

SAGE_API int sage_merge_split(const void *o_part, const float *lse_part, const void *o_tail, const float *lse_tail,
                              void *o_out, float *lse_out, int B, int S, int H, int group, int L, int D,
                              int64_t o_sb, int64_t o_sh, int64_t o_sl, int out_dtype, void *stream)
{
    return merge_split_common(false, o_part, lse_part, o_tail, lse_tail, o_out, lse_out, B, S, H, group, L, D, o_sb, o_sh, o_sl, out_dtype, stream);
}

SAGE_API int sage_merge_split_f32(const float *o_part, const float *lse_part, const float *o_tail, const float *lse_tail,
                                  void *o_out, float *lse_out, int B, int S, int H, int group, int L, int D,
                                  int64_t o_sb, int64_t o_sh, int64_t o_sl, int out_dtype, void *stream)
{
    return merge_split_common(true, o_part, lse_part, o_tail, lse_tail, o_out, lse_out, B, S, H, group, L, D, o_sb, o_sh, o_sl, out_dtype, stream);
}

}  // extern "C"
