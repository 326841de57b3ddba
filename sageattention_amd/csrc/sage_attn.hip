// sage_attn.hip -- host-side dispatch of the attention launches: the work order of a launch (sage_work_order.h) and the choice of the
// instantiation unit (sage_attn_form.h, sage_attn_parts.h; the kernels themselves are in sage_attn_kernel.h, compiled by sage_attn_d*_*.hip).
#include "sage_common.h"
#include "sage_kernels.h"
#include "sage_attn_parts.h"
#include "sage_work_order.h"
#include "sage_step_list.h"
#include <cstdlib>

#ifndef SAGE_ORDER_DEFAULT   // causal work order: -1 = grouped / folded (plan_grid), 0 = head-major heavy-first, n = groups of n heads
#define SAGE_ORDER_DEFAULT -1
#endif

namespace sage {

// Causal dense grids: which (head, query block) item a workgroup takes -- sage_work_order.h (mapping, group-size rule, measurements).
// Split-KV chunks (weights depend on the chunk), masked and varlen calls keep the head-major heavy-first order over contiguous runs.
// SAGE_ORDER_GROUP / sage_set_work_order: 0 restores the head-major order, n > 0 forces the group size (experiments).
static int g_work_order = -2;         // -2: not read yet
int work_order()
{
    if (g_work_order == -2) {
        const char *e = getenv("SAGE_ORDER_GROUP");
        g_work_order = (e != nullptr && e[0] != 0) ? atoi(e) : SAGE_ORDER_DEFAULT;
    }
    return g_work_order;
}
void set_work_order_mode(int group) { g_work_order = group; }

// the work order of a launch (q.order_*); returns its grid size
static int plan_grid(AttnParams &q, const AttnVariant &v)
{
    q.order_group = 0;
    q.order_fold = 0;
    q.order_left = 0;
    const int nheads = q.B * q.Hq;
    // a launch of the listed step call (sage_step_list.h): whole octets of (decode sequence, kv head) units, or the packed route's grid over the
    // host-known bound of the chunk list
    if (v.list) return (int)(v.gqa_pack ? step_decode_grid(q.B, q.Hkv, q.group) : step_chunk_grid(q.Hq, q.items_bound));
    // packed GQA groups (decode-shaped, one query block): (batch, kv head, block of four query heads) in head-major order
    if (v.gqa_pack) return q.B * q.Hkv * ((q.group + 3) / 4);
    if (q.cu_q != nullptr && q.work_items != nullptr)             // varlen, device-built work list: bound of the dense-style grid over it
        return 8 * ((q.Hq & 7) * ((q.items_bound + 7) / 8) + (q.Hq >> 3) * q.items_bound);
    if (q.cu_q != nullptr) return ((q.B * q.Hkv + 7) / 8) * 8 * q.group * q.nqblk;   // varlen: whole rounds of 8 (sequence, kv-head) units
    const int forced = work_order();
    // the exact split's pass 2 (one chunk included): (batch, folded head, query block) in head-major order, like the inexact split's
    if (!v.causal || v.mask_kind != 0 || v.seeded || q.kv_split > 1 || q.nqblk <= 1 || forced == 0) return nheads * q.nqblk;
    // (per-sample key lengths: planned for the padded q.Lk -- the order is a permutation of the items whatever the lengths are, and nothing on the
    // host depends on their values)
    WorkOrder w;
    const int grid = plan_work_order(w, nheads, q.nqblk, q.Lk, v.head_dim, v.pv_fp8, forced);
    q.order_group = w.group;
    q.order_fold = w.fold;
    q.order_left = w.left;
    return grid;
}

// the routes that exist: what a variant asks of the parameter block and of its own fields beyond what its form (attn_form, sage_attn_form.h) says
static bool route_exists(const AttnParams &p, const AttnVariant &v, const AttnLaunchOpts &o)
{
    const bool varlen = p.cu_q != nullptr, per_thread = v.qf == 1 || v.qf == 2, per_block = v.qf == 3 || v.qf == 4;
    if ((v.head_dim != 64 && v.head_dim != 128) || v.qf < 0 || v.qf > 4 || v.mask_kind < 0 || v.mask_kind > 3) return false;
    // a mask: INT8 q, FP16 PV, per-block scales, non-causal, the Triton kernel form
    if (v.mask_kind != 0 && (v.qf != 0 || v.pv_fp8 || v.causal || v.kthread || !v.two_level)) return false;
    if (per_thread && (varlen || !v.kthread || v.two_level != v.pv_fp8)) return false;
    // per-block Q: per-block k scales; FP16 PV in the Triton kernel form; FP8 PV over packed batches only, the exact score form
    if (per_block && (v.kthread || (v.pv_fp8 ? (!varlen || o.fp8_folded) : !v.two_level))) return false;
    if (p.v_rows != 0 && (v.pv_fp8 || v.mask_kind != 0 || varlen || p.kv_split > 1 || v.qf == 2 || v.qf == 4)) return false;     // (fp16 q only)
    if ((v.seeded || v.kv_lens) && (!per_thread || !v.pv_fp8 || o.fp8_folded)) return false;
    if (v.seeded != (p.seed_max != nullptr) || (v.seeded && p.kv_split < 1)) return false;
    if (v.kv_lens && (p.cu_k == nullptr || (p.kv_split > 1 && !v.seeded))) return false;
    // the kv_lens family's split (seeded with kv_lens): one query block, chunks of whole tiles folded into the kv heads, no window
    // (the split step call's pass 2 -- a listed decode launch, below: p.Lq = max_seqlen_q sizes nothing there, the band bounds the rows)
    if (v.seeded && v.kv_lens && ((v.list && v.band != nullptr ? v.band->hi > 32 : p.nqblk != 1) || p.kv_split < 2 || p.kv_base <= 0 || (p.kv_base & 63) != 0 || p.Hkv % p.kv_split != 0 ||
                                  p.seed_chunks != p.kv_split || p.seed_first != 0 || v.window != 0 || p.sched != nullptr)) return false;
    if (v.q_start != (!varlen && p.cu_qs != nullptr) || (v.q_start && (!v.kv_lens || !v.causal))) return false;
    // a window: the causal kv_lens kernels (offsets optional), or -- without kv_lens -- a packed bottom-right launch (the next line's conditions);
    // shapes whose sums stay inside the kernel's int arithmetic (a packed launch has no Lk of its own: p.Lk = 0, the caller bounds the sum)
    if (v.window < 0 || v.window != p.window ||
        (v.window > 0 && (!v.causal || (long)p.Lq + p.Lk > (1L << 29) || (!v.kv_lens && !(varlen && v.bottom_right))))) return false;
    // bottom-right alignment of a packed batch: causal, FP8 PV, per-block Q, two-level, the exact score form
    if (v.bottom_right && (!varlen || !v.causal || !v.pv_fp8 || !per_block || !v.two_level || o.fp8_folded)) return false;
    // packed GQA groups: the kv_lens family (above: fused per-thread Q, FP8 PV, the exact score form, dense, no split), a group to pack and
    // no more query rows than one wave's slab holds
    // (a step launch's decode half: p.Lq = max_seqlen_q sizes nothing there, the band bounds the rows a sample may have)
    if (v.gqa_pack && (!v.kv_lens || p.group < 2 || (v.band != nullptr ? v.band->hi > 32 : (p.Lq > 32 || p.nqblk != 1)))) return false;
    // a pool of pages behind a block table: the kv_lens family, or its split's pass 2 (seeded with kv_lens, checked above: the chunks folded into
    // p.Hkv, the pool's heads p.Hkv / p.kv_split); whole pages of 64 << page_shift keys, p.Lk the logical capacity
    if (v.paged != nullptr && (!v.kv_lens || (v.seeded ? (p.kv_split < 2 || p.Hkv % p.kv_split != 0) : p.kv_split > 1) ||
                               v.paged->block_table == nullptr || v.paged->page_shift < 0 ||
                               v.paged->page_shift > 20 || v.paged->num_pages < 1 || v.paged->max_pages < 1 ||
                               (long)p.Lk != ((long)v.paged->max_pages << (6 + v.paged->page_shift)) || p.nks != (4 << v.paged->page_shift))) return false;
    // packed query rows on that pool: the paged q_start / window kernels (no packed GQA groups, no split); the prefix array is the third kernel
    // argument, p.cu_q stays null -- the dense grid and the dense branches of the kernel -- and the packed lse needs its head stride
    if (v.ragged != nullptr && (v.paged == nullptr || !v.q_start || !v.causal || (v.gqa_pack && v.band == nullptr) || (v.seeded && !(v.list && v.gqa_pack && v.kv_lens)) || varlen ||
                                v.ragged->cu_q == nullptr || v.ragged->total_q < 1 ||
                                // (the split step call's pass 2: the partials are dense -- p.lse is lse_part, p.lse_sh the rows per (sequence, head) of the workspace)
                                (v.seeded ? (p.lse == nullptr || p.lse_sh < 1 || p.lse_sh > 32) : (p.lse != nullptr && p.lse_sh < v.ragged->total_q)))) return false;
    // one launch of the step call: packed query rows behind a band (lo, hi] of row counts, 0 <= lo <= hi; with packed GQA groups hi <= 32 (above)
    if (v.band != nullptr && (v.ragged == nullptr || v.band->lo < 0 || v.band->hi < v.band->lo)) return false;
    // ... of the listed step call: the lists in the two members a paged launch leaves free (the chunk list with the bound its grid is sized by)
    if (v.list && (v.band == nullptr || p.work_hdr == nullptr || p.work_items == nullptr || (!v.gqa_pack && p.items_bound < 1))) return false;
    return true;
}

hipError_t launch_attention(const AttnParams &p_in, const AttnVariant &v, const AttnLaunchOpts &o)
{
    AttnParams p = p_in;
    const int nwork = plan_grid(p, v);
    if (o.grid_out != nullptr) *o.grid_out = 0;
    if (nwork <= 0) return hipSuccess;
    if (!route_exists(p, v, o)) return hipErrorInvalidValue;
    // the form the launch needs and the unit that holds it (sage_attn_form.h): one launcher per (unit, head size)
    typedef hipError_t (*unit_launcher)(uint32_t, const AttnParams &, int, const AttnLaunchOpts &);
#define SAGE_UNIT_ROW(U) {launch_attn_unit<UNIT_##U, 64>, launch_attn_unit<UNIT_##U, 128>},
    static const unit_launcher launchers[UNIT_COUNT][2] = {SAGE_ATTN_UNITS(SAGE_UNIT_ROW)};
#undef SAGE_UNIT_ROW
    const AttnForm f = attn_form(p, v, o);
    if (v.paged != nullptr) {     // the paged kernel of the same form: same grid, the ordinary dispatch
        p.sched = nullptr;
        if (v.list && f.seed)         // pass 2 of the split step call: the list kernel of the seeded packed-group form (route_exists: gqa_pack with kv_lens)
            return (f.D == 128 ? launch_attn_lsplit_units<128, SAGE_STEP_KS_UNITS> : launch_attn_lsplit_units<64, SAGE_STEP_KS_UNITS>)(pack(f), p, *v.paged, *v.ragged, *v.band, nwork, o);
        if (v.list)                   // a launch of the listed step call: the list kernel of the form, from the same lists of forms as the step call's
            return f.gpack ? (f.D == 128 ? launch_attn_list_units<128, SAGE_STEP_G_UNITS> : launch_attn_list_units<64, SAGE_STEP_G_UNITS>)(pack(f), p, *v.paged, *v.ragged, *v.band, nwork, o)
                           : (f.D == 128 ? launch_attn_list_units<128, SAGE_STEP_UNITS> : launch_attn_list_units<64, SAGE_STEP_UNITS>)(pack(f), p, *v.paged, *v.ragged, *v.band, nwork, o);
        if (v.band != nullptr)        // a launch of the step call: the step kernel of the form, from the packed-group list (decode) or the ragged units' lists (chunks)
            return f.gpack ? (f.D == 128 ? launch_attn_step_units<128, SAGE_STEP_G_UNITS> : launch_attn_step_units<64, SAGE_STEP_G_UNITS>)(pack(f), p, *v.paged, *v.ragged, *v.band, nwork, o)
                           : (f.D == 128 ? launch_attn_step_units<128, SAGE_STEP_UNITS> : launch_attn_step_units<64, SAGE_STEP_UNITS>)(pack(f), p, *v.paged, *v.ragged, *v.band, nwork, o);
        if (v.ragged != nullptr)      // packed query rows: the ragged paged kernel of the form (the q_start / window forms, route_exists)
            return (f.D == 128 ? launch_attn_ragged_units<128, SAGE_RAGGED_UNITS> : launch_attn_ragged_units<64, SAGE_RAGGED_UNITS>)(pack(f), p, *v.paged, *v.ragged, nwork, o);
        if (f.seed) return (f.D == 128 ? launch_attn_paged_units<128, SAGE_PAGED_KS_UNITS> : launch_attn_paged_units<64, SAGE_PAGED_KS_UNITS>)(pack(f), p, *v.paged, nwork, o);
        return f.gpack ? (f.D == 128 ? launch_attn_paged_units<128, SAGE_PAGED_G_UNITS> : launch_attn_paged_units<64, SAGE_PAGED_G_UNITS>)(pack(f), p, *v.paged, nwork, o)
                       : (f.D == 128 ? launch_attn_paged_units<128, SAGE_PAGED_UNITS> : launch_attn_paged_units<64, SAGE_PAGED_UNITS>)(pack(f), p, *v.paged, nwork, o);
    }
    return launchers[unit_of(f)][f.D == 128](pack(f), p, nwork, o);
}

}  // namespace sage
