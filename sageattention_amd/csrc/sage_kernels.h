// sage_kernels.h -- internal launch interface between the C ABI (sage_cabi.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sage {

// query-scale granularity as seen by the attention kernel (slots per 128-row block)
enum : int { QG_PER_BLOCK = 1, QG_PER_WARP32 = 2, QG_PER_THREAD = 3, QG_PER_WARP16 = 4, QG_PER_THREAD16 = 5 };

constexpr int kAttnSchedBytes = 32 * 128;   // 32 ticket queues (8 XCDs x 4), one counter per 128-byte line
constexpr int kAttnSchedDoneWord = 16;      // (word 16 of line 0) workgroups that have left a persistent launch: the last one returns every word to zero

struct AttnParams {
    const void *q;            // int8 (or fp16 / bf16 for the fused-Q kernels), strides below (elements)
    const int8_t *k;
    const void *v;            // gfx950 tiled V^T image (see sage_prep_v.hip) -- or, v_rows != 0, the caller's fp16 V itself (rows of D halves)
    long v_sb, v_sh, v_sl;    // v_rows: element strides of that tensor (batch, kv-head, token)
    int v_rows;
    void *o;                  // fp16 / bf16
    float *lse;               // nullable, [B,Hq,Lq] log2 units
    const float *q_scale;
    const float *k_scale;
    const float *v_scale;     // [B,Hkv,D] (fp8 PV) or null
    const float *v_mean;      // [B,Hkv,D] or null
    const void *mask;         // attn_mask (bool bytes or fp16/bf16 additive), element strides below; null = none
    long m_sb, m_sh, m_sq, m_sk;
    const int32_t *cu_q;      // varlen only (null => dense)
    const int32_t *cu_k;      // (AttnVariant::kv_lens: the per-sample key lengths [B] instead, clamped to [0, Lk] by the kernel)
    const int32_t *cu_qs;     // prefix sums of ceil(Lq_i/128)  (dense AttnVariant::q_start: the per-sample query offsets [B] instead)
    const int32_t *cu_ks;     // prefix sums of ceil(Lk_i/64)
    const int32_t *seq_order; // varlen, nullable: permutation of sequence indices in processing order (legacy unit order, no work list)
    const int32_t *work_items;// varlen, nullable: the device-built work list of sage_varlen_plan ((sequence, query block), heaviest first)
    const int32_t *work_hdr;  // with work_items: {nitems, group, fold, left, ...} (kVarlenHdrWords)
    int items_bound;          // with work_items: host-known upper bound of nitems (sizes the grid)
    unsigned *sched;          // persistent launch (nullable): kAttnSchedBytes of ticket counters, ZERO on entry, zero again when the launch ends
    int nwg;                  // with sched: the logical grid (workgroup indices 0 .. nwg - 1 are dealt as tickets; the launch has fewer workgroups)
    int B, Hq, Hkv, group;    // group = Hq / Hkv
    int Lq, Lk;               // dense lengths; varlen: max lengths (grid sizing only)
    int nqblk;                // ceil(max Lq / 128)
    long q_sb, q_sh, q_sl;
    long k_sb, k_sh, k_sl;
    long o_sb, o_sh, o_sl;
    int nqs, nks;             // scale slots per (b,h) for q / k (dense)
    int qs_per_blk;           // q scale slots per 128-row block
    int q_gran;               // QG_*
    int kv_split;             // > 1: split-KV, the key range of a head is folded into the kv-head dimension (dense, fused-Q kernels)
    int ks_shift;             // k scale groups span 64 << ks_shift keys (1: the sm90 kernels' 128-key groups, core.py:964-970)
    int out_dtype;            // DT_F16 / DT_BF16
    long lse_sh;              // varlen lse head stride (unused for dense)
    float sm_scale_log2;      // multiplier taking dequantised scores to the log2 domain
    float q_premul;           // fused per-block Q quantisation (AttnVariant::qf 3 / 4): q is multiplied by this before its abs-max
    int order_group;          // set by the launcher (sage_attn.hip plan_grid): causal dense work order, heads per group; 0 = head-major
    int order_fold;           // 1: single-round grid, pair the i-th longest with the i-th shortest block on a CU
    int order_left;           // (B * Hq) % 8 heads whose query blocks are dealt to all eight XCDs
    unsigned *trace;          // -DSAGE_ATTN_TRACE=1 builds (tools/attn_trace.py): 16 words per logical workgroup, nullable; ignored otherwise
    int trace_wgs;
    // the exact split's pass 2 (AttnVariant::seeded; zero / null for every other launch): kv_split chunks of Lk keys from key kv_base on,
    // folded into the kv-head dimension as above but reading the unsplit operands in place (nks: k scale slots per head of the unsplit call);
    // seed_max: pass 1's chunk maxima [B, Hkv, seed_chunks, group, Lq], seed_first: the pass-1 chunks in front of this launch's chunk 0
    // (AttnVariant::seeded with kv_lens, the kv_lens family's split: kv_split chunks of kv_base = 64 T keys each from key 0 on, clipped per sample
    // to its length; Lk stays the padded length of the tensors, seed_chunks = kv_split, seed_first = 0)
    const float *seed_max;
    int seed_chunks, seed_first;
    int kv_base;
    int window;               // AttnVariant::window: keys a row sees up to and including its diagonal (the WINDOW kernels; in the block's tail padding:
                              // its size and the offsets of the hidden arguments behind it are what they were)
};

// The operands of a PAGED launch (AttnVariant::paged; sage_attn_paged_kernel): a second kernel argument behind the parameter block, whose size
// and offsets stay what they are.  k / v / k_scale of AttnParams are then a pool of num_pages pages of 64 << page_shift keys, laid out as the
// tensors of a call with B = num_pages and Lk = the page size (k_sb: the page stride, nks: the scale slots of one page), and p.Lk is the logical
// capacity max_pages * (64 << page_shift).  Logical 64-key tile t of sample b lies in page block_table[b * bt_stride + (t >> page_shift)], at
// tile t & ((1 << page_shift) - 1) of it; an id is clamped to [0, num_pages - 1] by the kernel before it forms an address.
struct PagedArgs {
    const int32_t *block_table;   // int32 [B, max_pages] in device memory, row stride bt_stride (elements)
    long bt_stride;
    int page_shift;               // page size = 64 << page_shift keys
    int num_pages;                // >= 1
    int max_pages;                // table entries per sample
};
constexpr long kPagedArgsOffset = (long)((sizeof(AttnParams) + alignof(PagedArgs) - 1) / alignof(PagedArgs) * alignof(PagedArgs));      // of the second argument in the kernarg segment

// The operands of a RAGGED paged launch (sage_attn_paged_varlen_kernel): a third kernel argument behind PagedArgs, whose size and
// offset stay what they are.  q / o are then packed [total_q, Hq, D] (q_sl / o_sl: the row strides, q_sb / o_sb unused), lse is [Hq, total_q]
// with head stride AttnParams::lse_sh, sample b's rows are cu_q[b] .. cu_q[b + 1] - 1 -- both words clamped by the kernel (ragged_rows,
// sage_ragged.h) before they form an address -- and AttnParams::Lq is max_seqlen_q: it sizes the grid and bounds the rows a sample gets.
struct RaggedArgs {
    const int32_t *cu_q;          // int32 [B + 1] in device memory
    int total_q;                  // rows of q / o / lse
};
constexpr long kRaggedArgsOffset = (long)((kPagedArgsOffset + sizeof(PagedArgs) + alignof(RaggedArgs) - 1) / alignof(RaggedArgs) * alignof(RaggedArgs));

// The band of a STEP launch (sage_attn_paged_step_kernel): a fourth kernel argument behind RaggedArgs, whose size and offset stay
// what they are.  A work item whose sample has `rows` query rows (ragged_rows' clamped count) runs iff lo < rows <= hi and leaves otherwise
// (ragged_band, sage_ragged.h): the step call's decode launch carries (0, 32], its chunk launch (32, max_seqlen_q].
struct BandArgs {
    int lo, hi;
};
constexpr long kBandArgsOffset = (long)((kRaggedArgsOffset + sizeof(RaggedArgs) + alignof(BandArgs) - 1) / alignof(BandArgs) * alignof(BandArgs));

// launch attributes of an attention call that are not kernel parameters (the C ABI's SageLaunchAttr, include/sage_gfx950.h)
struct AttnLaunchOpts {
    hipStream_t stream;
    bool fp8_folded;         // FP8 PV: the folded score form (opt-in variant) instead of the exact one
    bool force_persistent;   // take the ticket queues whatever the number of rounds (tests; AttnParams::sched must be set)
    int *grid_out;           // nullable (host): receives the number of workgroups launched
};
// Which member of the kernel family a launch takes: the instantiation unit (head_dim, pv_fp8, AttnLaunchOpts::fp8_folded, seeded, kv_lens, q_start, window, gqa_pack; the
// per-block fused Q quantiser with FP8 PV has units of its own) and everything else the template arguments of sage_attn_kernel encode.
//   INT8 q (qf 0)            every field below; a mask: FP16 PV, per-block scales, non-causal, the Triton kernel form
//   fused per-thread Q (1/2) dense; kthread, two_level = pv_fp8 (FP16 PV: straight FP32 accumulation)
//   fused per-block Q (3/4)  per-block k scales after the multiplication by AttnParams::q_premul; FP16 PV in the Triton kernel form, dense or
//                            varlen (AttnParams::cu_q); FP8 PV varlen only, the exact score form, two_level or single accumulation
struct AttnVariant {
    int head_dim;       // 64 / 128
    bool pv_fp8;
    bool causal;
    bool kthread;       // per-thread k scale groups (4 per 64 keys)
    bool two_level;     // FP8 PV: tile product from a zero accumulator; FP16 PV: the Triton kernel form (SAGE_PV_ACCUM_TRITON)
    int mask_kind;      // 0 none, 1 bool, 2 additive fp16, 3 additive bf16
    int qf;             // 0: INT8 q + q_scale; attn_qf(): fp16 / bf16 q quantised in the prologue per thread group (1 / 2) or per 128-row block (3 / 4)
    bool seeded;        // the exact split's pass 2 (fused per-thread Q, FP8 PV two-level, exact score form): the running maximum is seeded from
                        // AttnParams::seed_max, p.o takes FP32 partial outputs and p.lse log2-domain LSEs per chunk; p.kv_split >= 1 chunks of p.Lk
                        // keys from p.kv_base; head-major grid, no launch workspace
    bool kv_lens;       // per-sample key lengths (same kernels otherwise, dense): AttnParams::cu_k = int32 lengths [B] in device memory, sample b
                        // attends to keys 0 .. clamp(cu_k[b], 0, p.Lk) - 1 of the padded tensors; k / its scales / the V image from
                        // sage_quant_qk_int8_kvlens / sage_prep_v_fp8_kvlens
    bool q_start;       // per-sample query offsets (kv_lens and causal): AttnParams::cu_qs = int32 offsets [B] in device memory, row i of sample b
                        // attends to key j iff j <= clamp(cu_qs[b], -p.Lq, p.Lk) + i and j < its length
    int window;         // > 0: a sliding window on the causal kv_lens kernels (AttnParams::window = this): row i sees key j iff additionally
                        // j > s_b + i - window, s_b = cu_qs[b] (0 without q_start); 0: none
    bool bottom_right;  // a packed causal launch (FP8 PV, per-block Q, two-level, the exact score form): row i of sequence b attends to key j iff
                        // j <= i + Lk_b - Lq_b, the lengths from cu_q / cu_k -- no operand of its own (SAGE_ATTR_CAUSAL_BOTTOM_RIGHT)
    bool gqa_pack;      // a decode-shaped kv_lens launch (p.Lq <= 32, p.group >= 2; with or without q_start / window) whose work item is (batch, kv head,
                        // block of four query heads of the group), one wave per head over one shared K / V ring: B * Hkv * ceil(group / 4) workgroups,
                        // the bits of the launch without it (SAGE_ATTR_GQA_PACK); no operand, AttnParams is what it is without
    const PagedArgs *paged; // non-null (host memory, read by the launcher): a kv_lens launch (no split) whose K / V image / K scales are a pool of pages
                        // reached through a block table -- the paged kernel of the same form, same grid, ordinary dispatch (never the ticket route)
    const RaggedArgs *ragged; // non-null (host memory, with paged, q_start and causal; no gqa_pack, no split): packed query rows with a prefix array --
                        // the ragged paged kernel of the same form over the dense grid of B * Hq * ceil(AttnParams::Lq / 128) items
    const BandArgs *band;   // non-null (host memory, with ragged): one launch of the step call -- the step kernel of the same form, which runs the
                        // samples inside the band alone.  With gqa_pack it is the decode launch: B * Hkv * ceil(group / 4) items whatever
                        // AttnParams::Lq = max_seqlen_q is (the band's hi <= 32 bounds the rows instead)
    bool list;          // (with band) a launch of the LISTED step call (sage_kvlist_attn): the list kernel of the same form, its items from
                        // AttnParams::work_hdr / work_items (device memory, written by launch_kv_list_plan).  With gqa_pack the decode list, grid
                        // 8 * ceil(B * Hkv / 8) * ceil(group / 4); without, the chunk list, the packed route's grid over AttnParams::items_bound
};
constexpr int attn_qf(bool per_block, int q_dtype) { return (per_block ? 3 : 1) + (q_dtype == 0 ? 0 : 1); }   // q_dtype: DT_F16 (0) / DT_BF16
// the one attention launcher: plans the work order, checks that the route exists (hipErrorInvalidValue) and launches the variant's kernel.
// V rows in place (AttnParams::v_rows): FP16 PV, qf 0 / 1 / 3, dense, unmasked, no split
hipError_t launch_attention(const AttnParams &p, const AttnVariant &v, const AttnLaunchOpts &o);

// causal dense work order of the 128-row kernels: -1 grouped / folded by grid size, 0 head-major, n groups of n heads (SAGE_ORDER_GROUP)
int work_order();
void set_work_order_mode(int group);

// ---- INT8 quantisation of Q / K ----------------------------------------------------------------
enum : int { QS_TRITON = 0, QS_CUDA = 1, QS_TRITON_THREAD = 2 };          // rounding / epsilon style
enum : int { GR_BLOCK = 1, GR_WARP = 2, GR_THREAD_Q = 3, GR_THREAD_K = 5 };  // row -> scale group map

struct QuantParams {
    const void *x;            // fp16 / bf16
    const void *mean;         // nullable [B,H,D] (strides mean_sb, mean_sh)
    int8_t *out;
    float *scale;
    const int32_t *cu;        // varlen: cu_seqlens (null => dense)
    const int32_t *cu_scale;  // varlen: prefix of blocks
    int B, H, L, D;
    long x_sb, x_sh, x_sl;
    long o_sb, o_sh, o_sl;
    long mean_sb, mean_sh;
    int nscale;               // dense: scale slots per (b,h)
    int blk;                  // rows per workgroup: 128 (Q) / 64 (K)
    int warp;                 // sub-group rows for GR_WARP / GR_THREAD_* (32, 16, 64)
    int gran, style, dtype;
    float pre_scale;
    const int32_t *kv_lens;   // dense, nullable [B]: rows >= clamp(kv_lens[b], 0, L) of sample b are neither read nor written, their scale groups not formed
};
hipError_t launch_quant_int8(const QuantParams &p, hipStream_t stream);
// packed batches: every index array of a varlen call from one launch (sage_varlen_plan.hip), nseq <= kVarlenPlanMaxSeq
constexpr int kVarlenPlanMaxSeq = 1024;
constexpr int kVarlenHdrWords = 8;       // hdr: nitems, group, fold, left, nslab (K / V pre-pass slabs), max Lk, sum Lk, 0
struct VarlenPlanParams {
    const int32_t *cu_q, *cu_k;          // [nseq + 1]
    int nseq, blkq, blkk;
    int total_k;                         // rows of the packed k / v tensors (>= cu_k[nseq]): rows outside every sequence still count in the K mean
    int causal, Hq, Hkv, head_dim, pv_fp8;   // for the launch plan (hdr) only
    int32_t *cu_qs;                      // nullable [nseq + 1]
    int32_t *cu_ks;                      // [nseq + 1]
    int32_t *order;                      // nullable [nseq]
    int32_t *items;                      // nullable [2 * nitems]: (sequence, query block), heaviest first
    int32_t *slab_first;                 // nullable [nseq + 3]: prefix sums of the slab counts of the nseq sequences, then of two "gap" segments
                                         // (index nseq: rows cu_k[nseq] .. total_k, index nseq + 1: rows 0 .. cu_k[0]) that only the K mean reads
    int32_t *slab_seq;                   // nullable [nslab]: slab -> segment (sequence, or nseq / nseq + 1 for the gaps)
    int32_t *hdr;                        // nullable [kVarlenHdrWords]
    int forced_group;                    // work_order() when > 0 (experiments: heads per XCD group of the attention launch's plan), else -1
    int items_cap, slab_cap;             // (sequence, query block) pairs `items` holds, entries of `slab_seq`: counts derived from cu_seqlens on the
                                         // device are clamped to them (hdr reports the clamped counts), so an inconsistent cu_seqlens cannot write past
};
hipError_t launch_varlen_plan(const VarlenPlanParams &p, hipStream_t stream);

// the listed step call's work lists from one small launch (sage_kv_list_plan.hip; the arithmetic is sage_step_list.h's), B <= kVarlenPlanMaxSeq
constexpr int kStepListHdrWords = 16;    // hdr: n_decode, n_chunk_items, group, fold, left, chunk items before the clamp, max key count of a chunk sequence, 0 ...
struct KvListPlanParams {
    const int32_t *cu_q;                 // [B + 1] the packed query rows' prefix array
    const int32_t *kv_lens, *q_start;    // [B]
    int B, total_q, max_seqlen_q;
    int Lk, window;                      // the logical capacity; SageLaunchAttr.window (0: none)
    int Hq, Hkv, head_dim;               // for the chunk launch's plan (hdr) only
    int items_cap;                       // (sequence, query block) pairs the chunk list holds: step_chunk_bound()
    int32_t *ws;                         // hdr[kStepListHdrWords], decode_list[B], chunk_items[2 * items_cap]
};
hipError_t launch_kv_list_plan(const KvListPlanParams &p, hipStream_t stream);

// ---- per-channel statistics over the sequence (K mean, V amax / mean) -----------------------------
#ifndef SAGE_STATS_SLAB
#define SAGE_STATS_SLAB 512
#endif
constexpr int kStatsSlab = SAGE_STATS_SLAB;   // tokens per stage-1 workgroup
struct StatsParams {
    const void *x;            // fp16 / bf16 [.., L, D] with strides
    float *ws;                // [B,H,nslab,3,D] partial (max, min, sum)
    float *stats;             // nullable [B,H,3,D] final (max, min, sum)
    void *mean_out;           // nullable [B,H,D] mean in the input dtype
    int B, H, L, D, nslab;
    long x_sb, x_sh, x_sl;
    int dtype;
    // packed batches (nullable, together): slabs per segment as sage_varlen_plan lays them out; nslab = host-known bound, L = rows of x
    const int32_t *cu, *slab_first, *slab_seq, *hdr;
    int nseq;
    // seq_stats != 0 (packed batches, cu set; B = nseq): stage 2 per SEQUENCE, stats [nseq,H,3,D] (the V scales of sage_prep_v_fp8_varlen).
    // With the slab map above stage 1 is the map's launch (ws [1,H,nslab,3,D]); without it stage 1 runs over (slab of a sequence, head,
    // sequence), nslab = ceil(max L / 512) slabs per sequence (ws [nseq,H,nslab,3,D])
    int seq_stats;
    // dense, nullable [B]: the statistics of sample b run over rows < clamp(kv_lens[b], 0, L) only (same slabs from row 0, same order: what a
    // call on the first kv_lens[b] rows gives, bit for bit); the mean of a sample without rows is 0, its (max, min, sum) (-inf, +inf, 0)
    const int32_t *kv_lens;
};
hipError_t launch_stats(const StatsParams &p, hipStream_t stream);

// ---- V pre-pass -------------------------------------------------------------------------------
struct PrepVParams {
    const void *v;            // fp16 / bf16 [.., L, D] with strides
    void *out;                // tiled V^T image, fp8 or fp16
    const float *stats;       // fp8: [B,H,3,D] (max, min, sum) from launch_stats
    const float *mean_in;     // fp16 path: nullable [B,H,D] mean to subtract (smooth_v)
    float *v_scale;           // [B,H,D] out (fp8)
    float *v_mean;            // fp8: nullable [B,H,D] out; non-null = smooth_v (subtract the mean)
    const int32_t *cu;        // varlen
    const int32_t *cu_tiles;  // varlen: prefix of ceil(L_i/64)
    int B, H, L, D;
    long v_sb, v_sh, v_sl;
    int dtype;
    int fp8;                  // 1: e4m3 output, 0: fp16 output
    float scale_max;
    const int32_t *kv_lens;   // dense fp8, nullable [B]: tokens >= clamp(kv_lens[b], 0, L) are zero in the tile that holds the last valid token, the
                              // tiles behind it are not written; the scales of a sample without tokens are 0 (image layout as for L tokens)
};
hipError_t launch_prep_v(const PrepVParams &p, hipStream_t stream);

// ---- fused K / V pre-pass: one launch, one read of K and V (sage_prepass.hip) -----------------------------------------
constexpr int kPrepassMaxSlabs = 65536 / kStatsSlab;   // slabs of one head that wait for each other inside the launch (L <= 65536):
                                                       // 16 per XCD against 64 resident workgroup slots per XCD
constexpr int kPrepassSyncStride = 32;  // uint32 words per (part, head): arrival + departure counter on their own 128-B line
struct PrepassParams {
    const void *k;            // fp16 / bf16 [.., L, D] with strides (parts & 1)
    const void *v;            // same shape (parts & 2)
    void *k_mean;             // nullable [B,H,D] out, input dtype; non-null = smooth_k (subtract it before quantising)
    int8_t *k_out;            // INT8 K, strides ko_*
    float *k_scale;           // [B,H,ceil(L/k_blk)*groups]
    void *v_image;            // tile image [B,H,ceil(L/64),D,64], fp8 or fp16 (v_fp16)
    float *v_scale;           // [B,H,D] out
    float *v_mean;            // nullable [B,H,D] out; non-null = smooth_v
    float *ws;                // [2,B,H,nslab,3,D] slab partials
    unsigned *sync;           // [2,B,H,kPrepassSyncStride] per head: arrival counter, departure counter, give-up flag.  ZERO on entry (the
                              // caller zeroes the buffer once); the kernel returns both counters to zero before it ends
    int B, H, L, D, nslab;
    long k_sb, k_sh, k_sl;
    long v_sb, v_sh, v_sl;
    long ko_sb, ko_sh, ko_sl;
    int parts;                // 1: K only, 2: V only, 3: both
    int v_fp16;               // V half: 0 = per-channel FP8 image (statistics + scales), 1 = fp16 image (`v.to(float16)`, no statistics)
    int k_blk;                // keys per scale block: 64 / 128
    int k_warp;               // == k_blk (one thread-group map per block)
    int k_gran;               // GR_BLOCK / GR_THREAD_K
    int k_style;              // QS_*
    int dtype;
    float scale_max;          // 448 for e4m3
    int debug_fail;           // test hook (sage_debug_prepass_fail): wait for one slab more than exists and give up after 2^10 polls
    unsigned *host_flag;      // nullable: device-visible pinned HOST word that a workgroup which gives up sets to 1 (system-scope store), so
                              // the caller can learn of a poisoned launch at its next call without a synchronisation
    // packed (varlen) batches: k / v are [sum L, H, D]; a slab is 512 tokens of ONE sequence, the head barrier and the K mean span all
    // sequences (core.py:432-434).  B = 1, L = sum L (the mean's divisor), nslab = host-known bound of the slab count (grid, workspace)
    const int32_t *cu;        // null => dense.  cu_seqlens_k [nseq + 1]
    const int32_t *cu_tiles;  // prefix sums of ceil(L_i / 64): k scale block / V tile index of a sequence's first block
    const int32_t *slab_seq;  // slab -> segment: a sequence, or a gap (nseq: rows cu[nseq] .. L, nseq + 1: rows 0 .. cu[0]; statistics only)
    const int32_t *slab_first;// prefix sums of the segments' slab counts
    const int32_t *hdr;       // sage_varlen_plan's header: hdr[4] = number of slabs that exist
    int nseq;                 // number of sequences (segments >= nseq are gaps)
};
hipError_t launch_prepass_kv(const PrepassParams &p, hipStream_t stream);
hipError_t launch_debug_spin(int ms, int nwg, hipStream_t stream);

// ---- LSE merge of partial attention states (sequence-parallel callers) -----------------------------
struct MergeParams {
    float *o_acc;             // [B,H,L,D] fp32 running output, contiguous
    float *lse_acc;           // [B,H,L] fp32 running log-sum-exp (natural log), contiguous
    const void *o_new;        // fp16 / bf16 partial output, element strides below
    const float *lse_new;     // [B,H,L] contiguous
    void *o_out;              // nullable: also write the merged output in the dtype of o_new (last step)
    int B, H, L, D;
    long n_sb, n_sh, n_sl;    // o_new strides
    long o_sb, o_sh, o_sl;    // o_out strides
    int dtype;
    int first;                // 1: initialise the running state from (o_new, lse_new)
    int cpr_pad;              // set by launch_merge_states: lanes per row (power of two >= D/8, <= 64)
};
hipError_t launch_merge_states(const MergeParams &p, hipStream_t stream);

// ---- split-KV merge (one attention call computed as S (+1) key-range chunks) -------------------------------------------
struct SplitMergeParams {
    const void *o_part;       // fp16 [B, Hkv, S, group, L, D] contiguous (H = Hkv * group)
    const float *lse_part;    // [B, Hkv, S, group, L] log2-domain log-sum-exp of each chunk (-inf: no visible key)
    const void *o_tail;       // nullable fp16 [B, H, L, D]: one more chunk (ragged tail of the key range)
    const float *lse_tail;    // [B, H, L]
    void *o_out;              // fp16 / bf16, element strides below
    float *lse_out;           // nullable [B, H, L] log2 domain
    int B, S, H, L, D, group;
    long o_sb, o_sh, o_sl;
    int dtype;                // of o_out
    int cpr_pad;              // set by the launcher
};
hipError_t launch_merge_split(const SplitMergeParams &p, hipStream_t stream);
// the same merge over FP32 partials (o_part, o_tail: float; the exact split's pass 2 writes them)
hipError_t launch_merge_split_f32(const SplitMergeParams &p, hipStream_t stream);
// ... for the decode sequences of a step alone (the split step call): FP32 partials [B, Hkv, S, group, L] with L = min(max_seqlen_q, 32),
// the results packed behind r -- o_out [total_q, H, D] (o_sl / o_sh), lse_out [H, total_q] (lse_sh); other sequences and rows are not touched
hipError_t launch_merge_split_ragged(const SplitMergeParams &p, const RaggedArgs &r, int max_seqlen_q, long lse_sh, hipStream_t stream);

// ---- the exact split's pass 1: per (batch, query head, query row, chunk) the row maximum the attention kernel forms over the chunk's keys ---------
struct ChunkMaxParams {
    const void *q;            // fp16 / bf16 [B, Hq, Lq, D] (element strides), quantised per thread group exactly as the fused-Q kernels do
    const int8_t *k;          // INT8 K of the unsplit call (strides in bytes = elements), per-thread k scales [B, Hkv, nks]
    const float *k_scale;
    float *out;               // [B, Hkv, S, group, Lq]: fma(max raw score, c, -log2(448)) over the chunk's visible keys, -inf where none is
    int B, Hq, Hkv, group, Lq, Lk, D;
    int S, tiles;             // chunks, 64-key tiles per chunk (chunk c: tiles c * tiles .. + tiles - 1)
    int nqblk, nks;
    long q_sb, q_sh, q_sl;
    long k_sb, k_sh, k_sl;
    float sm_scale_log2;
    int q_dtype, causal;
};
hipError_t launch_chunk_max(const ChunkMaxParams &p, hipStream_t stream);

// ---- the same for the kv_lens family's split (num_splits=): a call of one query block (Lq <= 128) whose sample b attends to keys j < len_b and,
// causal, j <= s_b + i; chunk c holds the tiles c * tiles .. + tiles - 1 of the padded tensor, clipped to ceil(len_b / 64) per sample
struct ChunkMaxLensParams {
    const void *q;            // as ChunkMaxParams
    const int8_t *k;
    const float *k_scale;
    float *out;               // [B, Hkv, S, group, Lq]; every element is written (-inf: the chunk holds no visible key of the row)
    const int32_t *kv_lens;   // [B], clamped to [0, Lk] as the KVLEN kernels clamp it
    const int32_t *q_start;   // causal: nullable [B] (null: offsets 0), clamped to [-Lq, Lk] as the QSTART kernels clamp it
    int B, Hq, Hkv, group, Lq, Lk, D;
    int S, tiles;
    int nks;
    long q_sb, q_sh, q_sl;
    long k_sb, k_sh, k_sl;
    float sm_scale_log2;
    int q_dtype, causal;
};
hipError_t launch_chunk_max_lens(const ChunkMaxLensParams &p, hipStream_t stream);
// ... over a paged cache (sage_split_paged.hip): k / k_scale / k_sb / Hkv / nks describe the pool of pages, Lk is the logical capacity, g the table
hipError_t launch_chunk_max_lens_paged(const ChunkMaxLensParams &p, const PagedArgs &g, hipStream_t stream);
// ... for the decode sequences of a step (sage_split_ragged.hip): Lq = max_seqlen_q, q packed behind r (q_sl the row stride), causal; out is
// [B, Hkv, S, group, lq_ws] with lq_ws = min(max_seqlen_q, 32), written for the rows of the sequences of 1 .. 32 rows alone
hipError_t launch_chunk_max_lens_ragged(const ChunkMaxLensParams &p, const PagedArgs &g, const RaggedArgs &r, int lq_ws, hipStream_t stream);

// ---- the C ABI's error channel for entry points defined outside sage_cabi.hip (sage_kv_cache.hip): stores the thread-local message that
// sage_last_error() returns and hands `code` back
int set_last_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// page_size = 64 * 2^k -> k, or -1 (sage_kv_paged.hip)
int paged_shift(int page_size);

}  // namespace sage
