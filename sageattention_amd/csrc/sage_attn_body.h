// sage_attn_body.h -- the body of sage_attn_kernel<FORM>, of sage_attn_paged_kernel<FORM>, of sage_attn_paged_varlen_kernel<FORM> and of
// sage_attn_paged_step_kernel<FORM> (sage_attn_kernel.h, which documents the flags): a code fragment, included INSIDE the four kernel functions
// with SAGE_ATTN_BODY_PAGED defined as false / true / true / true, SAGE_ATTN_BODY_RAGGED as false / false / true / true and SAGE_ATTN_BODY_BAND as
// false / false / false / true -- and of sage_attn_paged_list_kernel<FORM> (sage_attn_list_kernel.h), the fifth entry: all three true and
// SAGE_ATTN_BODY_LIST defined as true (a SEED form under that entry is pass 2 of the split step call).  Not a header of its own: no
// include guard, no declarations.
    static constexpr bool PAGED = SAGE_ATTN_BODY_PAGED;
    static constexpr bool RAGGED = SAGE_ATTN_BODY_RAGGED;
    static constexpr bool BAND = SAGE_ATTN_BODY_BAND;
#ifndef SAGE_ATTN_BODY_LIST      // (the four entries of sage_attn_kernel.h leave it undefined: false; sage_attn_list_kernel.h defines it true)
#define SAGE_ATTN_BODY_LIST false
#define SAGE_ATTN_BODY_LIST_DEFAULTED
#endif
    // LIST (sage_attn_paged_list_kernel, sage_attn_list_kernel.h): a step launch whose work items come from the device-built lists
    // of sage_kv_list_plan.hip -- p.work_hdr / p.work_items, free in a paged launch -- instead of the dense grid.  Only the work-item site differs.
    static constexpr bool LIST = SAGE_ATTN_BODY_LIST;
    static_assert(!LIST || BAND, "the listed step launch: a band launch over a work list");
    // The form's fields under the names the body uses.  (static: the body's lambdas capture by reference, and a plain constexpr local that one of
    // them passes on by reference becomes a captured stack slot -- folded away later, but sixteen D = 128 FP16-PV kernels then allocate their
    // registers differently, 217 - 229 VGPRs where these give 219 - 226.)
    static constexpr AttnForm F = unpack(FORM);
    static_assert(pack(F) == FORM && valid(F), "not a form of the family: form_error() in sage_attn_form.h names the rule it breaks");
    static constexpr int D = F.D;
    static constexpr bool PV_FP8 = F.pv_fp8;
    static constexpr bool CAUSAL = F.causal;
    static constexpr bool KTHREAD = F.kthread;
    static constexpr bool TWO_LEVEL = F.two_level;
    static constexpr int NH = 1;                            // 64-key images per iteration: every member of the family runs 64-key iterations
    static constexpr int MASK = F.mask;
    static constexpr int QF = F.qf;
    static constexpr bool GPACK = F.gpack;
    static constexpr bool SFOLD = F.sfold;
    // (F.cpers has no alias: its one reader is ticket_loop(F), PERS_OK below)
    static constexpr bool VROWS = F.vrows;
    static constexpr bool SEED = F.seed;
    static constexpr bool WINDOW = F.window;
    static constexpr bool QSTART = F.qstart;
    static constexpr bool KVLEN = F.kvlen;
    static_assert(!PAGED || (KVLEN && PV_FP8), "paged tiles: the kv_lens family, its split (SEED with KVLEN) included");
    // LSPLIT: pass 2 of the split step call -- the list entry over a SEED form: the decode list's sequences as p.kv_split key-range chunks each,
    // Q from the packed rows, the FP32 partials into the dense split workspace whose rows per (sequence, head) are p.lse_sh (min(max_seqlen_q, 32))
    static constexpr bool LSPLIT = LIST && SEED;
    static_assert(!LSPLIT || (GPACK && KVLEN && !WINDOW), "the split step launch: the seeded packed-group forms with offsets, no window");
    static_assert(!RAGGED || (PAGED && CAUSAL && QSTART && (LSPLIT || !SEED) && (BAND || !GPACK)), "packed query rows: the paged q_start / window kernels (a step launch: their packed-group forms too; the split step launch: the seeded ones)");
    static_assert(!BAND || RAGGED, "the band filter: a ragged launch of the step call");
    // The parameter block is read through the kernarg segment pointer, and inside the persistent loop through a copy of that pointer the
    // compiler cannot see through (an empty asm): otherwise every scalar load of a parameter is hoisted out of the loop and stays live in
    // SGPRs across it (128 SGPRs and 16-400 VGPRs spilled in every instantiation).  AttnParams is the kernel's only explicit argument.
    typedef const __attribute__((address_space(4))) AttnParams *kparams_t;
    const kparams_t kp0 = (kparams_t)__builtin_amdgcn_kernarg_segment_ptr();
    const __attribute__((address_space(4))) AttnParams &p = *kp0;
    (void)p_arg;
#if SAGE_KARG_PREFETCH
    // The parameter block spans seven 64-byte lines and the prologue reads it in ten dependent rounds of scalar loads (branches in between): in a
    // launch's first round of workgroups every first touch of a line is a miss of the scalar cache, three or four of them in series.  One load per
    // line here, waited for together: one miss time instead, the rounds below hit.  (Values unused; each load has its own destination.)
    static_assert(sizeof(AttnParams) > 0x180, "prefetch offsets lie inside the parameter block");
    {
        unsigned t0, t1, t2, t3, t4, t5, t6;
        asm volatile("s_load_dword %0, %7, 0x0\n\ts_load_dword %1, %7, 0x40\n\ts_load_dword %2, %7, 0x80\n\ts_load_dword %3, %7, 0xc0\n\t"
                     "s_load_dword %4, %7, 0x100\n\ts_load_dword %5, %7, 0x140\n\ts_load_dword %6, %7, 0x180\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(t0), "=&s"(t1), "=&s"(t2), "=&s"(t3), "=&s"(t4), "=&s"(t5), "=&s"(t6) : "s"(kp0) : "memory");
    }
#endif
    using C = TileCfg<D, PV_FP8, NH>;
    constexpr int KT = C::KT;
    constexpr int NS = 2 * NH;                       // 32-key S^T sub-tiles per iteration
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    // (wave index in an SGPR, lane index from v_mbcnt wherever it is needed: nothing derived from threadIdx.x has to stay in a VGPR across
    //  the persistent loop below)
    const int wave_s = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
#if SAGE_ATTN_TRACE
    __shared__ unsigned ttrace[16];
#endif
    // ---- persistent launch (p.sched != null; non-causal, unmasked instantiations only): gridDim.x workgroups -- as many as the device holds at
    //      once -- work through the logical grid of p.nwg workgroup indices.  The indices are dealt into 32 queues: index i belongs to XCD i & 7
    //      (the work order's L2 locality, sage_work_order.h) and there to sub-queue (i >> 3) & 3, i.e. i = 32 k + 8 s + x.  A workgroup starts with
    //      its own blockIdx.x (the hardware deals blockIdx.x to XCD blockIdx.x & 7) and then takes tickets k from the counter of its queue -- the
    //      ticket is requested behind the last tile of the item in hand and read after its output rows are on their way.  When that queue is empty
    //      it looks at all 32 counters once and takes a ticket from the fullest queue, its own XCD's first (the XCDs of a device run a few per cent
    //      apart: profiles/r4_run_p_attention_phase_trace.txt).  One counter per 128-byte line, zeroed by the caller: agent-scope atomics on one
    //      address serialise at ~200 ns each, and the 64 workgroups of an XCD finish equal items together.
    //      Causal launches keep the hardware's dispatch: their work order pairs a long and a short block on a CU through the order in which
    //      freed slots are refilled, and tickets lose that (measured: +2.6 % at C3, +7 % at C2).
    // (round 5: the packed / varlen route's CAUSAL launches over the device-built work list take the route too -- +2.2 ... 2.9 % at C4 -- through
    //  instantiations of their own (CPERS); dense causal launches lose 0.1 ... 7.5 % with tickets and the loop's mere presence costs the dense
    //  Triton-API causal kernel 1.3 %, so their instantiations stay without it: profiles/r5_pers_causal_probe.txt, r5_run_c_qf_pers_ab.txt)
    constexpr bool PERS_OK = ticket_loop(F);
    const bool pers = PERS_OK && p.sched != nullptr;
    __shared__ int s_ticket[2];                 // (two slots, alternating: a wave may still be reading the previous ticket when wave 0 posts the next)
    int tpar = 0;
    int bid = blockIdx.x;
    unsigned next_k_v = 0;                       // (lane 0 of wave 0) the ticket requested ahead
    bool have_next = false, own_empty = false;   // wave-uniform
    // this workgroup's queue: 4 * XCD (HW_REG_XCC_ID[3:0]) + sub-queue.  Everything the ticket code needs besides the three words above is
    // re-derived where it is used (a register read, a scalar load), so that nothing of it is live across the key loop: two SGPRs more
    // spilled to a VGPR cost the D = 64 per-thread instantiation its last register under the three-waves limit.
    // (parameters through a pointer the compiler cannot see through, as in the item loop below: else their scalar loads are hoisted and stay live)
    auto kpl = [&]() -> kparams_t { kparams_t k = kp0; asm volatile("" : "+s"(k)); return k; };
    auto my_queue = [&]() -> int { return 4 * (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u) + (int)((blockIdx.x >> 3) & 3u); };
    // the logical grid
    auto logical_grid = [&]() -> int {
        const __attribute__((address_space(4))) AttnParams &pl = *kpl();
        int n = pl.nwg;
        if (pl.cu_q != nullptr && pl.work_items != nullptr) {
            typedef const __attribute__((address_space(4))) int *cint_p;
            const cint_p hdr = (cint_p)pl.work_hdr;
            n = 8 * (hdr[3] * ((hdr[0] + 7) >> 3) + (pl.Hq >> 3) * hdr[0]);
        }
        return n;
    };
    // wave 0: the next logical workgroup index, or -1 when every queue is empty
    auto resolve_ticket = [&]() -> int {
        const int nwg_l = logical_grid();
        const int sched_first = gridDim.x >> 5;      // tickets of every queue that the first round (blockIdx.x) covers
        const int my_q = my_queue(), my_xcd = my_q >> 2;
        unsigned *const sched = kpl()->sched;
        if (have_next) {
            have_next = false;
            const int i = 32 * ((int)__builtin_amdgcn_readfirstlane(next_k_v) + sched_first) + 8 * (my_q & 3) + my_xcd;
            if (i < nwg_l) return i;
            own_empty = true;
        }
        int lane_o = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+v"(lane_o));         // (or the per-lane queue addresses below are computed once, outside the item loop, and stay live)
        for (int attempt = 0; attempt < 4; attempt++) {
            // lane q < 32 looks at queue q; the fullest queue wins, queues of the own XCD before the others
            const int q = lane_o & 31, x = q >> 2, s8x = 8 * (q & 3) + x;
            const unsigned c = lane_o < 32 ? __hip_atomic_load(sched + 32 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
            const int cnt = nwg_l > s8x ? (nwg_l - s8x + 31) >> 5 : 0;
            int left = cnt - sched_first - (int)c;
            left = left < (1 << 24) ? left : (1 << 24) - 1;
            unsigned key = (lane_o < 32 && left > 0) ? ((x == my_xcd ? 1u : 0u) << 30) | ((unsigned)left << 5) | (unsigned)q : 0u;
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) { const unsigned o = __shfl_xor(key, m); key = o > key ? o : key; }
            key = __builtin_amdgcn_readfirstlane(key);
            if (key == 0u) return -1;
            const int bq = (int)(key & 31u);
            unsigned kv = 0;
            if (lane_o == 0) kv = __hip_atomic_fetch_add(sched + 32 * bq, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int i = 32 * ((int)__builtin_amdgcn_readfirstlane(kv) + sched_first) + 8 * (bq & 3) + (bq >> 2);
            if (i < nwg_l) return i;
        }
        return -1;
    };
    while (bid >= 0) {
    next_k_v = 0;                                // (defined at the top of every pass: not carried round the loop in a VGPR)
    do {
    kparams_t kp = kp0;
    if constexpr (PERS_OK) asm volatile("" : "+s"(kp));
    const __attribute__((address_space(4))) AttnParams &p = *kp;
    // (the same for everything derived from the thread index: hoisted out of the loop, the prologue's and the epilogue's per-lane
    //  offsets would stay live through the key loop -- 13-32 VGPRs spilled in every instantiation)
    int lane_v = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    if constexpr (PERS_OK) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_v));     // (per item: the builtin's value is hoisted out of the loop and lives through it)
    const int lane = lane_v;
    const int wave = wave_s;
    [[maybe_unused]] const int tid = wave * 64 + lane;
    int n = lane & 31;            // query row inside the wave's 32-row tile
    int g = lane >> 5;            // k-group (operand half)
    SAGE_TSTAMP(0);
    // Inside the key loop the conversions of P saturate to the largest finite value instead of overflowing (MODE.FP16_OVFL = 1; back to 0 in front
    // of the epilogue, whose output conversion overflows to inf as the reference's does).  FP8 PV: the reference converts P with
    // cvt.rn.satfinite.e4m3x2.f32 (numeric_conversion.cuh:46-61) and v_cvt_pk_fp8_f32 without the mode bit returns NaN above 464.  With the exact
    // score form P exceeds 448 = 2^8.807 only by the rounding of m (scores of millions); the folded form's m + bias c' is rounded at a magnitude
    // of bias c', so from c = sm_scale log2(e) q_scale k_scale ~ 0.1 (|q|, |k| ~ 100) on a row's largest P can pass 464 -- NaN rows without this.
    // FP16 PV: the folded bias of the pipelined loops likewise, at c ~ 50, against fp16's 65504.
    __builtin_amdgcn_s_setreg(kHwregModeFp16Ovfl, 1);

    // ---- work item: XCD-aware, heavy-first --------------------------------------------------
    const int nqblk = p.nqblk;
    int b, h, hk, qblk;
    [[maybe_unused]] bool idle = false;       // (GPACK) wave-uniform: this wave's head lies past the group's last one
    if constexpr (LSPLIT) {
        // the decode list again, every sequence as p.kv_split chunks: units (list rank, chunk, kv head) dealt as the arm below deals (list rank, kv head)
        // -- step_split_item, sage_step_list.h -- with the chunk folded into the kv heads as the dense split folds it (hk = hk0 * S + chunk, p.Hkv =
        // Hkv * S).  Every word of the list is clamped before anything is formed from it
        typedef const __attribute__((address_space(4))) int *cint_p;          // wave-uniform: scalar loads
        const int nd_raw = ((cint_p)p.work_hdr)[0];
        const int nd = nd_raw < 0 ? 0 : (nd_raw < p.B ? nd_raw : p.B);
        int r, ck, hk0, gb;
        if (!step_split_item(bid, nd, p.kv_split, p.Hkv / p.kv_split, p.group, r, ck, hk0, gb)) break;
        const int bl = ((cint_p)p.work_items)[r];
        b = bl < 0 ? 0 : (bl < p.B ? bl : p.B - 1);
        hk = hk0 * p.kv_split + ck;
        const int hw = 4 * gb + wave_s;
        idle = hw >= p.group;
        h = hk * p.group + (idle ? 0 : hw);
        qblk = 0;
    } else if constexpr (LIST && GPACK) {
        // the decode list (hdr[0] sequences, heaviest first): units (list rank, kv head) dealt to the XCDs round-robin, the blocks of a unit on
        // one XCD.  Every word of the list is clamped before anything is formed from it: a workspace the plan never wrote stays inside the operands
        typedef const __attribute__((address_space(4))) int *cint_p;          // wave-uniform: scalar loads
        const int nd_raw = ((cint_p)p.work_hdr)[0];
        const int nd = nd_raw < 0 ? 0 : (nd_raw < p.B ? nd_raw : p.B);
        const int ngb = (p.group + 3) >> 2;
        const int xcd = bid & 7, idx = bid >> 3;
        const int uj = idx / ngb, gb = idx - uj * ngb;
        const int unit = uj * 8 + xcd;
        if (unit >= nd * p.Hkv) break;
        const int r = unit / p.Hkv;
        const int bl = ((cint_p)p.work_items)[r];
        b = bl < 0 ? 0 : (bl < p.B ? bl : p.B - 1);
        hk = unit - r * p.Hkv;
        const int hw = 4 * gb + wave_s;
        idle = hw >= p.group;
        h = hk * p.group + (idle ? 0 : hw);
        qblk = 0;
    } else if constexpr (LIST) {
        // the chunk list: the statements of the packed route's arm below over hdr {nitems, group, fold, left} and the (sequence, query block)
        // pairs, with every word clamped -- the count to the host-known bound the grid is sized by, the order to one work_item() deals in full
        typedef const __attribute__((address_space(4))) int *cint_p;          // wave-uniform: scalar loads
        const cint_p hdr = (cint_p)p.work_hdr;
        const int ni_raw = hdr[0], g_raw = hdr[1], hpx = p.Hq >> 3;
        const int nitems = ni_raw < 0 ? 0 : (ni_raw < p.items_bound ? ni_raw : p.items_bound);
        const WorkOrder wo = {g_raw < 1 || hpx < 1 ? 1 : (g_raw < hpx ? g_raw : hpx), hdr[2] != 0 ? 1 : 0, p.Hq & 7};
        const int nwg = 8 * (wo.left * ((nitems + 7) >> 3) + hpx * nitems);
        int qrank;
        if (bid >= nwg || !work_item(wo, bid, nwg, p.Hq, nitems, h, qrank)) break;
        qrank = qrank < 0 ? 0 : (qrank < nitems ? qrank : nitems - 1);
        h = h < 0 ? 0 : (h < p.Hq ? h : p.Hq - 1);
        const cint_p items = (cint_p)p.work_items;
        const int bl = items[2 * qrank], ql = items[2 * qrank + 1];
        b = bl < 0 ? 0 : (bl < p.B ? bl : p.B - 1);
        qblk = ql < 0 ? 0 : (ql < nqblk ? ql : nqblk - 1);
        hk = h / p.group;
    } else if constexpr (GPACK) {
        // the grid is B * Hkv * ceil(group / 4) items in head-major order, one contiguous run per XCD as below: the blocks of a kv head -- and
        // the kv heads of a sample -- stream K / V through one L2
        const int ngb = (p.group + 3) >> 2;
        int u, qrank;
        const WorkOrder wo = {0, 0, 0};
        if (!work_item(wo, bid, (int)gridDim.x, p.B * p.Hkv * ngb, 1, u, qrank)) break;
        const int bk = u / ngb, hw = 4 * (u - bk * ngb) + wave_s;
        b = bk / p.Hkv;
        hk = bk - b * p.Hkv;
        idle = hw >= p.group;
        h = hk * p.group + (idle ? 0 : hw);
        qblk = 0;
    } else if (p.cu_q != nullptr && p.work_items != nullptr) {
        // varlen with the device-built work list (sage_varlen_plan): the query blocks of all sequences are one item list per query head,
        // heaviest first, and the launch is a dense launch over Hq heads of `nitems` items each (sage_work_order.h) -- whole GQA groups
        // stay on one XCD, every workgroup has an item (the grid is sized by a host-known bound of nitems; the few past it exit here)
        typedef const __attribute__((address_space(4))) int *cint_p;          // wave-uniform: scalar loads
        const cint_p hdr = (cint_p)p.work_hdr;
        const int nitems = hdr[0];
        const WorkOrder wo = {hdr[1], hdr[2], hdr[3]};
        const int nwg = 8 * (wo.left * ((nitems + 7) >> 3) + (p.Hq >> 3) * nitems);
        int qrank;
        if (bid >= nwg || !work_item(wo, bid, nwg, p.Hq, nitems, h, qrank)) break;
        const cint_p items = (cint_p)p.work_items;
        b = items[2 * qrank];
        qblk = items[2 * qrank + 1];
        hk = h / p.group;
    } else if (p.cu_q != nullptr) {
        // varlen without a work list (more sequences than sage_varlen_plan takes): sequences differ in length, so a contiguous run
        // per XCD would hand one XCD the longest sequence
        // (measured 3.5x slower on lengths 256..16384).  XCDs take (sequence, kv-head) units round-robin instead;
        // inside a unit the `group` query heads that share the K/V stream run heavy-first, interleaved.
        const int xcd = bid & 7, idx = bid >> 3;
        const int per_unit = nqblk * p.group;
        const int j = idx / per_unit, within = idx - j * per_unit;
        const int u = j * 8 + xcd;
        if (u >= p.B * p.Hkv) break;
        const int r = within / p.group, hg = within - r * p.group;
        qblk = nqblk - 1 - r;
        const int bs = u / p.Hkv;
        hk = u - bs * p.Hkv;
        b = p.seq_order != nullptr ? p.seq_order[bs] : bs;      // caller's processing order (longest first)
        h = hk * p.group + hg;
    } else {
        // workgroups bid, bid+8, bid+16.. share an XCD (bid % 8); each XCD takes one contiguous run of work items,
        // so the q-blocks of one head -- and the query heads of one GQA group -- stream K/V through one L2, and the
        // longest (causal) blocks of a head are dispatched first.  Measured alternatives (profiles/r1_run28_xcd_map.txt,
        // DESIGN.md 3.1): heads dealt to XCDs in rounds of 8 is 6-14 % slower where it spreads a head's K/V over all
        // eight L2s; shortest-first order -5 %, alternating long/short -21 %.
        int bh, qrank;
        const WorkOrder wo = {CAUSAL ? p.order_group : 0, p.order_fold, p.order_left};      // causal work order: sage_work_order.h
        if (!work_item(wo, bid, pers ? p.nwg : (int)gridDim.x, p.B * p.Hq, nqblk, bh, qrank)) break;
        qblk = nqblk - 1 - qrank;
        b = bh / p.Hq;
        h = bh - b * p.Hq;
        hk = h / p.group;
    }

    // ---- per-sequence geometry ---------------------------------------------------------------
    int Lq = p.Lq, Lk = p.Lk;
    [[maybe_unused]] int qstart = 0;      // (QSTART) the position of the sample's query row 0 on the key axis
    [[maybe_unused]] int wwin = 0, kc0w = 0;      // (WINDOW) keys a row sees up to and including its diagonal; the work item's first key (a multiple of 64)
    long q_off, k_off, o_off;
    long v_tile0, v_tstride;              // V image index = v_tile0 + t * v_tstride
    const float *qs_ptr, *ks_ptr;
    int qs_stride, ks_tstride;
    // (PAGED) the item's first logical tile (a window's kc0w / 64)
    [[maybe_unused]] int pt0 = 0;
    // (PAGED with SEED) the chunk is folded into the kv heads, the pool is not: the unsplit kv head hk0 and the pool's heads per page, p.Hkv / S
    [[maybe_unused]] int phk = 0, pnh = 0;
    if (p.cu_q != nullptr) {              // varlen: packed [sum L, H, D]
        // the prefix arrays are read-only here and the sequence index is wave-uniform: scalar loads, requested together (as vector loads they
        // were a memory round trip of their own behind the work list's; measured neutral at C4, profiles/r4_run_p_attention_phase_trace.txt)
        typedef const __attribute__((address_space(4))) int *cint_p;
        const int bu = __builtin_amdgcn_readfirstlane(b);
        const int q0 = ((cint_p)p.cu_q)[bu], k0 = ((cint_p)p.cu_k)[bu], q1 = ((cint_p)p.cu_q)[bu + 1], k1 = ((cint_p)p.cu_k)[bu + 1];
        const int ks0 = ((cint_p)p.cu_ks)[bu];
        Lq = q1 - q0;
        Lk = k1 - k0;
        if (qblk * BLKQ >= Lq) break;
        if constexpr (QSTART && !KVLEN) qstart = Lk - Lq;      // (packed, bottom-right: in [-Lq, Lk] by construction, wave-uniform, from the words just loaded)
        q_off = (long)q0 * p.q_sl + (long)h * p.q_sh;
        k_off = (long)k0 * p.k_sl + (long)hk * p.k_sh;
        o_off = (long)q0 * p.o_sl + (long)h * p.o_sh;
        v_tile0 = (long)ks0 * p.Hkv + hk;
        v_tstride = p.Hkv;
        qs_ptr = QF == 0 ? p.q_scale + ((long)((cint_p)p.cu_qs)[bu] + qblk) * p.Hq + h : nullptr;    // [sum nblk, Hq] (fused Q: no stored scales)
        qs_stride = 0;
        ks_ptr = p.k_scale + (long)ks0 * p.Hkv + hk;                  // [sum nblk, Hkv]
        ks_tstride = p.Hkv;
        if constexpr (WINDOW && QSTART && !KVLEN) {
            // the packed window: W from p.window, clamped as in the dense branch; the offset needs no clamp (above).  The item's first key as
            // there -- a0 <= Lk - W < Lk for a block that exists, so a shifted item keeps at least one key -- but in the PACKED layouts: V images
            // and the per-block k scales are one per 64-key tile with stride Hkv
            const int w = p.window;
            wwin = w < 1 ? 1 : (w < (1 << 30) ? w : (1 << 30));
            const int a0 = (qstart - wwin) + qblk * BLKQ + 1;
            kc0w = a0 > 0 ? (a0 & ~(BLKK - 1)) : 0;
            k_off += (long)kc0w * p.k_sl;
            v_tile0 += (long)(kc0w >> 6) * p.Hkv;
            ks_ptr += (long)(kc0w >> 6) * p.Hkv;
            Lk = Lk > kc0w ? Lk - kc0w : 0;
        }
    } else if constexpr (SEED && KVLEN) {
        // the kv_lens split (pass 2): chunk hk - hk0 * S of kv head hk0 holds keys [kc0, kc0 + p.kv_base) of the sample's first len_b, in whole
        // 64-key tiles of the UNSPLIT call's operands.  The length and the offset are formed as the KVLEN / QSTART kernels form them and shifted
        // into the chunk's coordinates; k_off, v_tile0 and ks_ptr move as the WINDOW branch moves them.  A chunk from len_b on keeps Lk = 0:
        // no tile is requested and nothing is formed from its pointers.
        typedef const __attribute__((address_space(4))) int *cint_p;
        const int hk0 = hk / p.kv_split, kc0 = (hk - hk0 * p.kv_split) * p.kv_base;
        const long bh0 = (long)b * (p.Hkv / p.kv_split) + hk0;
        const int bu = __builtin_amdgcn_readfirstlane(b);
        const int len = ((cint_p)p.cu_k)[bu];
        const int lenb = len < 0 ? 0 : (len < p.Lk ? len : p.Lk);
        // (RAGGED: the split step launch) the sample's rows of the packed q, by the band arm's statements below: Lq is the sample's own row count
        // from here on, as in the dense split call of that many rows; a sample outside the band leaves.  (ragged_band_rows: ragged_band itself
        // under the name of this second site, sage_ragged.h)
        [[maybe_unused]] int rq0 = 0;
        if constexpr (RAGGED) {
            typedef const __attribute__((address_space(4))) RaggedArgs *kragged_t;
            typedef const __attribute__((address_space(4))) BandArgs *kband_t;
            const kragged_t r = (kragged_t)((const __attribute__((address_space(4))) char *)kp + kRaggedArgsOffset);
            const kband_t bd = (kband_t)((const __attribute__((address_space(4))) char *)kp + kBandArgsOffset);
            ragged_band_rows(((cint_p)r->cu_q)[bu], ((cint_p)r->cu_q)[bu + 1], r->total_q, p.Lq, bd->lo, bd->hi, rq0, Lq);
            if (qblk * BLKQ >= Lq) break;
        }
        if constexpr (QSTART) {            // (p.cu_qs may be null: offsets 0, the top-left mask)
            const int s = p.cu_qs != nullptr ? ((cint_p)p.cu_qs)[bu] : 0;
            if constexpr (RAGGED) qstart = s < -Lq ? -Lq : (s < p.Lk ? s : p.Lk);         // (the sample's own row count where the dense kernel has the call's)
            else
            qstart = s < -p.Lq ? -p.Lq : (s < p.Lk ? s : p.Lk);
        }
        kc0w = kc0;
        const int left = lenb - kc0;
        Lk = left < 0 ? 0 : (left < p.kv_base ? left : p.kv_base);
        if constexpr (RAGGED) q_off = (long)rq0 * p.q_sl + (long)(hk0 * p.group + (h - hk * p.group)) * p.q_sh;
        else
        q_off = (long)b * p.q_sb + (long)(hk0 * p.group + (h - hk * p.group)) * p.q_sh;
        if constexpr (PAGED) k_off = (long)hk0 * p.k_sh;             // (the page's p.k_sb and the tile inside it come per tile: k_tile, through pt0)
        else
        k_off = (long)b * p.k_sb + (long)hk0 * p.k_sh + (long)kc0 * p.k_sl;
        o_off = (long)b * p.o_sb + (long)h * p.o_sh;
        v_tile0 = bh0 * (p.nks >> 2) + (kc0 >> 6);      // (per-thread k scales: four per 64-key tile, so nks / 4 tiles per head of the tensor)
        v_tstride = 1;
        qs_ptr = nullptr;
        qs_stride = 0;
        if constexpr (PAGED) ks_ptr = p.k_scale;                     // (the slots of (page, kv head hk0): ks_slot)
        else
        ks_ptr = p.k_scale + bh0 * p.nks + (kc0 >> 6) * 4;
        ks_tstride = 4;
        if constexpr (PAGED) {
            // a chunk need not start on a page boundary: its tile t is logical tile pt0 + t, as a window's
            pt0 = kc0 >> 6;
            phk = hk0;
            pnh = p.Hkv / p.kv_split;
        }
    } else if constexpr (SEED) {
        // exact split (pass 2): chunk `chunk` of kv head hk0 starts at key kc0; q, k, its scales and the V image are the unsplit call's
        const int hk0 = hk / p.kv_split, kc0 = p.kv_base + (hk - hk0 * p.kv_split) * Lk;
        const long bh0 = (long)b * (p.Hkv / p.kv_split) + hk0;
        q_off = (long)b * p.q_sb + (long)(hk0 * p.group + (h - hk * p.group)) * p.q_sh;
        k_off = (long)b * p.k_sb + (long)hk0 * p.k_sh + (long)kc0 * p.k_sl;
        o_off = (long)b * p.o_sb + (long)h * p.o_sh;
        v_tile0 = bh0 * (p.nks >> 2) + (kc0 >> 6);      // (per-thread k scales: four per 64-key tile, so nks / 4 tiles per head)
        v_tstride = 1;
        qs_ptr = nullptr;
        qs_stride = 0;
        ks_ptr = p.k_scale + bh0 * p.nks + (kc0 >> 6) * 4;
        ks_tstride = 4;
    } else {
        // split-KV (p.kv_split = S > 1): the key range is folded into the kv-head dimension, kv head hk = hk0 * S + chunk and query
        // head h = hk * group + g; the query rows are those of head hk0 * group + g (read in place, no per-chunk copy of Q)
        const int hq = p.kv_split > 1 ? (hk / p.kv_split) * p.group + (h - hk * p.group) : h;
        // (RAGGED) the sample's rows of the packed q / o / lse: the two prefix words through scalar loads (wave-uniform index), clamped before
        // anything is formed from them (ragged_rows: 0 <= rq0 <= rq0 + Lq <= total_q, Lq <= p.Lq = max_seqlen_q); a query block past the
        // sample's last row leaves as the packed route's does
        [[maybe_unused]] int rq0 = 0;
        if constexpr (RAGGED) {
            typedef const __attribute__((address_space(4))) int *cint_p;
            typedef const __attribute__((address_space(4))) RaggedArgs *kragged_t;
            const kragged_t r = (kragged_t)((const __attribute__((address_space(4))) char *)kp + kRaggedArgsOffset);
            const int bu = __builtin_amdgcn_readfirstlane(b);
            if constexpr (BAND) {
                // (a step launch: the sample's rows only if their count lies in the launch's band -- two more words behind the ragged ones, scalar
                //  loads; a sample outside the band has Lq = 0 here and its items leave with the blocks past a sample's last row, just below)
                typedef const __attribute__((address_space(4))) BandArgs *kband_t;
                const kband_t bd = (kband_t)((const __attribute__((address_space(4))) char *)kp + kBandArgsOffset);
                ragged_band(((cint_p)r->cu_q)[bu], ((cint_p)r->cu_q)[bu + 1], r->total_q, p.Lq, bd->lo, bd->hi, rq0, Lq);
            } else
            ragged_rows(((cint_p)r->cu_q)[bu], ((cint_p)r->cu_q)[bu + 1], r->total_q, p.Lq, rq0, Lq);
            if (qblk * BLKQ >= Lq) break;
        }
        if constexpr (KVLEN) {             // the sample's key count: wave-uniform index, one scalar load (as the packed route's prefix arrays)
            typedef const __attribute__((address_space(4))) int *cint_p;
            const int len = ((cint_p)p.cu_k)[__builtin_amdgcn_readfirstlane(b)];
            Lk = len < 0 ? 0 : (len < p.Lk ? len : p.Lk);
            if constexpr (QSTART) {        // the sample's query offset, requested with the length: p.cu_qs is as free in a dense launch as p.cu_k
                if constexpr (WINDOW) {
                    const int w = p.window, s = p.cu_qs != nullptr ? ((cint_p)p.cu_qs)[__builtin_amdgcn_readfirstlane(b)] : 0;
                    wwin = w < 1 ? 1 : (w < (1 << 30) ? w : (1 << 30));
                    int sl;
                    if constexpr (RAGGED) sl = s < -Lq ? -Lq : s;         // (the sample's own row count where the dense kernel has the call's)
                    else
                    sl = s < -p.Lq ? -p.Lq : s;                 // (the lower clamp first: sl - p.Lk cannot overflow)
                    qstart = sl - p.Lk > wwin ? p.Lk + wwin : sl;       // (above p.Lk + W no row sees a key either way)
                } else {
                const int s = ((cint_p)p.cu_qs)[__builtin_amdgcn_readfirstlane(b)];
                if constexpr (RAGGED) qstart = s < -Lq ? -Lq : (s < p.Lk ? s : p.Lk);
                else
                qstart = s < -p.Lq ? -p.Lq : (s < p.Lk ? s : p.Lk);
                }
            }
        }
        if constexpr (RAGGED) q_off = (long)rq0 * p.q_sl + (long)hq * p.q_sh;
        else
        q_off = (long)b * p.q_sb + (long)hq * p.q_sh;
        if constexpr (PAGED) k_off = (long)hk * p.k_sh;              // (the page's p.k_sb comes per tile: k_tile)
        else
        k_off = (long)b * p.k_sb + (long)hk * p.k_sh;
        if constexpr (RAGGED) o_off = (long)rq0 * p.o_sl + (long)h * p.o_sh;
        else
        o_off = (long)b * p.o_sb + (long)h * p.o_sh;
        const int ntk = ((KVLEN ? p.Lk : Lk) + BLKK - 1) / BLKK;      // (images per head of the tensor)
        v_tile0 = ((long)b * p.Hkv + hk) * ntk;
        v_tstride = 1;
        qs_ptr = p.q_scale + ((long)b * p.Hq + h) * p.nqs + (long)qblk * p.qs_per_blk;
        qs_stride = 1;
        if constexpr (PAGED) ks_ptr = p.k_scale;                     // (the slots of (page, kv head): ks_slot)
        else
        ks_ptr = p.k_scale + ((long)b * p.Hkv + hk) * p.nks;
        ks_tstride = KTHREAD ? 4 : 1;
        if constexpr (PAGED) {
            if constexpr (WINDOW) {
                const int a0 = (qstart - wwin) + qblk * BLKQ + 1;
                kc0w = a0 > 0 ? (a0 & ~(BLKK - 1)) : 0;
                pt0 = kc0w >> 6;
                Lk = Lk > kc0w ? Lk - kc0w : 0;
            }
        } else
        if constexpr (WINDOW) {
            // the first key any row of the block sees, a0 = max(0, s + 128 qblk - W + 1), and the tile it lies in: the item's key 0 from here on
            const int a0 = (qstart - wwin) + qblk * BLKQ + 1;
            kc0w = a0 > 0 ? (a0 & ~(BLKK - 1)) : 0;
            k_off += (long)kc0w * p.k_sl;
            v_tile0 += kc0w >> 6;
            ks_ptr += (kc0w >> 6) * 4;
            Lk = Lk > kc0w ? Lk - kc0w : 0;
        }
    }

    SAGE_TSTAMP(1);
    const int row0 = GPACK ? 0 : qblk * BLKQ + wave * 32;        // first query row of this wave (GPACK: every wave holds rows 0 .. of its own head)
    int Lq_w = Lq;                                   // the rows this wave loads and stores: Lq, but (GPACK) none in an idle wave
    if constexpr (GPACK) Lq_w = idle ? 0 : Lq;
    int my_row = row0 + n;                           // (re-derived behind the pipelined loops, see there)
    // causal mask in the chunk's key coordinates (split-KV: this workgroup sees keys kchunk0 .. kchunk0 + Lk - 1 as 0 .. Lk - 1):
    // key <= row  <=>  local key <= row - kchunk0
    // (QSTART: row i sees key <= i + qstart -- the same shift with kchunk0 = -qstart, in [-p.Lk, p.Lq].  Every bound below is formed from
    //  it in signed arithmetic: a division that truncates a negative numerator towards zero yields a value the following clamp to 0 replaces)
    const int kchunk0 = QSTART ? kc0w - qstart
                      : SEED ? (CAUSAL ? p.kv_base + (hk % p.kv_split) * Lk : 0)
                             : ((CAUSAL && p.kv_split > 1 && p.cu_q == nullptr) ? (hk % p.kv_split) * Lk : 0);
    const int crow0 = row0 - kchunk0;
    int cmy_row = my_row - kchunk0;
    const int ntk_all = (Lk + BLKK - 1) / BLKK;      // 64-key images that exist
    int n_iters = (Lk + KT - 1) / KT;
    if (CAUSAL) {
        int lim = (qblk * BLKQ + BLKQ - kchunk0 + KT - 1) / KT;      // <= 0: the whole chunk lies behind the diagonal
        lim = lim > 0 ? lim : 0;
        n_iters = lim < n_iters ? lim : n_iters;
    }
    // (WINDOW) head tiles: the block's last row that exists sees keys from x on (the item's coordinates), so tiles 0 .. ceil(x / 64) - 1 cut some row
    // on the left
    [[maybe_unused]] int nh = 0;
    if constexpr (WINDOW) {
        int rlast = qblk * BLKQ + BLKQ - 1;
        rlast = rlast < Lq ? rlast : Lq - 1;
        const int x = rlast - kchunk0 + 1 - wwin;
        nh = x > 0 ? (x + BLKK - 1) >> 6 : 0;
        nh = nh < n_iters ? nh : n_iters;
    }
    int n_lim = n_iters;                  // tiles of the run in hand: all of them, or (WINDOW) the head tiles first
    if constexpr (WINDOW) n_lim = nh > 0 ? nh : n_iters;

    // ---- Q fragments (B operand of S^T = K Q^T), resident in VGPRs ---------------------------
    v4i qf[C::KSTEPS];
    float qsc;
    // ---- tile staging ------------------------------------------------------------------------
    const unsigned char *kbase = reinterpret_cast<const unsigned char *>(p.k) + k_off;
    static_assert(!VROWS || (!PV_FP8 && MASK == 0), "V rows in place: FP16 PV, unmasked, dense launches");
    // (VROWS: the (batch, kv-head)'s first row; else the image array, indexed by v_tile0 + t * v_tstride)
    const unsigned char *vbase = reinterpret_cast<const unsigned char *>(p.v) + (VROWS ? 2 * ((long)b * p.v_sb + (long)hk * p.v_sh) : 0L);
    constexpr int CPR = D / 16;                                   // 16-B chunks per K row
    // LDS-DMA: every wave-instruction moves 64 x 16 B = 1 KiB; the LDS destination is lane-linear
    // (M0 base + lane*16), so the XOR swizzle of the K image goes on the per-lane SOURCE address.
    // Key rows past Lk are clamped to the last valid row, V images past the last one to the last
    // image (their probabilities are exactly zero: masked scores).
    constexpr int KP = C::K_TILE_BYTES / 1024, VP = C::V_IMG_BYTES / 1024;   // 1-KiB pieces
    // per-lane source offsets are loop-invariant: tile base pointers advance in SGPRs, so a full
    // tile costs no VALU address arithmetic per iteration
    unsigned koff[KP / 4];
#pragma unroll
    for (int i = 0; i < KP / 4; i++) {
        const int e = (wave * (KP / 4) + i) * 64 + lane;       // 16-B slot index inside the tile
        const int row = e / CPR, phys = e % CPR;
        koff[i] = (unsigned)(row * (int)p.k_sl + swz_chunk<D>(row, phys) * 16);
    }
    // VROWS: the tile in LDS is [64 tokens][D halves], at D = 128 with the 64-byte segments of a row XOR-ed by (token & 3) -- the four rows a
    // 32-lane half of a transposing read touches then lie in different banks (unswizzled: 1.5x the read time at two workgroups per CU; D = 64
    // measured no different).  A 1-KiB piece of the DMA is RPP whole rows; the lane's slot inside it is (row l / CPRV, chunk l % CPRV), and
    // since RPP is a multiple of 4 the swizzle is the same for every piece: ONE per-lane source offset, piece bases in SGPRs.
    constexpr int CPRV = D / 8;                                   // 16-B chunks per V row
    constexpr int RPP = 64 / CPRV;                                // rows per 1-KiB piece
    [[maybe_unused]] unsigned voffr = 0;                          // (VROWS) per-lane source offset inside a piece: row * row stride + logical chunk * 16
    if constexpr (VROWS) {
        const int row = lane / CPRV, phys = lane % CPRV;
        const int logical = D == 128 ? (phys ^ ((row & 3) << 2)) : phys;
        voffr = (unsigned)(row * (int)p.v_sl * 2 + logical * 16);
    }
    // the A operand of v_mfma_f32_32x32x16_f16 for channels 32 dt .. + 31 and tokens 16 c .. + 15 of the tile at LDS address `vs`: from the
    // image one ds_read_b128 (lane = channel row of the image); from rows two transposing reads -- the lane ADDRESSES the 8-byte chunk
    // (token 16 c + 8 half + 4 g + (s >> 2), channels 32 dt + 16 hgrp + 4 (s & 3) .. + 3), s = lane & 15, hgrp = (lane >> 4) & 1, and RECEIVES
    // tokens 16 c + 8 half + 4 g + 0 .. 3 of channel 32 dt + (lane & 31): elements 4 half .. 4 half + 3 of the operand, the order P is in
    // (the lane's part of the address is loop-invariant -- one offset per 32-channel tile at D = 128, where the segment swizzle depends on dt -- and
    //  the (c, half) part an immediate: one address add per channel tile and 64-key tile, in the LDS address space so that the offsets fold)
    typedef __attribute__((address_space(3))) unsigned char *lds_bytes;
    [[maybe_unused]] int vr_off[C::DT];
    if constexpr (VROWS) {
        const int s16 = lane & 15, hgrp = (lane >> 4) & 1;
#pragma unroll
        for (int dt = 0; dt < C::DT; dt++)
            vr_off[dt] = (4 * g + (s16 >> 2)) * (D * 2) + (D == 128 ? (dt ^ (s16 >> 2)) : dt) * 64 + 32 * hgrp + 8 * (s16 & 3);
    }
    auto v_frag = [&](const unsigned char *vs, int dt, int c) -> v4i {
        if constexpr (VROWS) {
            typedef short v4s __attribute__((ext_vector_type(4)));
            typedef short v8s __attribute__((ext_vector_type(8)));
            typedef __attribute__((address_space(3))) v4s *lds_v4s;
            const lds_bytes a0 = (lds_bytes)vs + vr_off[dt];
            const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(a0 + 16 * c * (D * 2)));
            const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(a0 + (16 * c + 8) * (D * 2)));
            return __builtin_bit_cast(v4i, (v8s)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        } else {
            const int drow = dt * 32 + n;
            return *reinterpret_cast<const v4i *>(vs + drow * 128 + swz_chunk<128>(drow, 4 * g + c) * 16);
        }
    };
    // ---- (PAGED) where 64-key tile t of the item lies, `pg` being page_of(t), looked up once per tile by the caller: the three address functions
    //      every tile address of a paged kernel goes through.  (The unpaged kernels keep their expressions where they stood: routed through
    //      lambdas of their own they came out with other scalar register numbers and operand orders, and their listings are held identical.)
    // (the second kernel argument is read as the first is, through the kernarg segment, and through a pointer the compiler cannot see through each
    //  time: the table's base, stride and geometry are then scalar loads next to their use -- kept in SGPRs across the key loop they cost the D = 64
    //  kernels one or two VGPRs more than three waves leave)
    typedef const __attribute__((address_space(4))) PagedArgs *kpaged_t;
    [[maybe_unused]] auto paged_args = [&]() -> kpaged_t {
        kparams_t k2 = kp;
        asm volatile("" : "+s"(k2));
        return (kpaged_t)((const __attribute__((address_space(4))) char *)k2 + kPagedArgsOffset);
    };
    [[maybe_unused]] auto page_of = [&]([[maybe_unused]] int t) -> int {
        if constexpr (PAGED) {
            typedef const __attribute__((address_space(4))) int *ctable_p;
            const kpaged_t g = paged_args();
            const int pg = ((ctable_p)g->block_table)[(long)__builtin_amdgcn_readfirstlane(b) * g->bt_stride + ((pt0 + t) >> g->page_shift)];
            const int last = g->num_pages - 1;
            return pg < 0 ? 0 : (pg < last ? pg : last);            // (clamped on the scalar unit before it forms an address)
        } else return 0;
    };
    [[maybe_unused]] auto tile_in_page = [&]([[maybe_unused]] int t) -> int {
        if constexpr (PAGED) return (pt0 + t) & ((p.nks >> 2) - 1);   // (p.nks: four scale slots per tile of ONE page, a power of two)
        else return 0;
    };
    [[maybe_unused]] auto k_tile = [&]([[maybe_unused]] int t, [[maybe_unused]] int pg) -> const unsigned char * {
        if constexpr (PAGED) return kbase + (long)pg * p.k_sb + (long)tile_in_page(t) * KT * p.k_sl;
        else return nullptr;
    };
    [[maybe_unused]] auto v_tile = [&]([[maybe_unused]] int t, [[maybe_unused]] int pg) -> long {     // the V image's index
        if constexpr (PAGED) {
            if constexpr (SEED) return ((long)pg * pnh + phk) * (p.nks >> 2) + tile_in_page(t);
            else
            return ((long)pg * p.Hkv + hk) * (p.nks >> 2) + tile_in_page(t);
        }
        else return 0;
    };
    [[maybe_unused]] auto ks_slot = [&]([[maybe_unused]] int t, [[maybe_unused]] int pg) -> long {    // the tile's first K scale slot
        if constexpr (PAGED) {
            if constexpr (SEED) return ((long)pg * pnh + phk) * p.nks + tile_in_page(t) * 4;
            else
            return ((long)pg * p.Hkv + hk) * p.nks + tile_in_page(t) * 4;
        }
        else return 0;
    };
    int lane_g = lane;                      // the lane index as the ragged tile loads see it (laundered behind the pipelined loops, see there)
    auto issue_loads = [&](int it, int buf) {
        unsigned char *ks = smem + buf * C::STAGE_BYTES;
        unsigned char *vs = ks + C::K_TILE_BYTES;
        // (`if constexpr`, not a conditional expression: a paged-only name in a live expression is captured by the lambda, and the closure's
        //  layout is visible in the unpaged D = 128 kernels' register allocation)
        const unsigned char *kt;
        [[maybe_unused]] long vti = 0;
        if constexpr (PAGED) {
            const int pg = page_of(it);      // (every caller requests a tile that exists, it < ntk_all: K and the V image of one page)
            kt = k_tile(it, pg);
            vti = v_tile(it, pg);
        } else
        kt = kbase + (long)it * KT * p.k_sl;
        if (it * KT + KT <= Lk) {
#pragma unroll
            for (int i = 0; i < KP / 4; i++) {
                const int pc = wave * (KP / 4) + i;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(kt + koff[i]),
                                                 (__attribute__((address_space(3))) void *)(ks + pc * 1024), 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < KP / 4; i++) {
                const int pc = wave * (KP / 4) + i;
                const int e = pc * 64 + lane_g;
                const int row = e / CPR, phys = e % CPR;
                int key = it * KT + row;
                key = key < Lk ? key : Lk - 1;
                const unsigned char *src;
                if constexpr (PAGED) src = kt + (long)(key - it * KT) * p.k_sl + swz_chunk<D>(row, phys) * 16;
                else
                src = kbase + (long)key * p.k_sl + swz_chunk<D>(row, phys) * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                 (__attribute__((address_space(3))) void *)(ks + pc * 1024), 16, 0, 0);
            }
        }
#pragma unroll
        for (int hh = 0; hh < NH; hh++) {
            int tv = it * NH + hh;
            tv = tv < ntk_all ? tv : ntk_all - 1;
            if constexpr (VROWS) {          // rows 64 tv .. of the head; rows past Lk are clamped to the last one (their probabilities are exactly zero)
#pragma unroll
                for (int i = 0; i < VP / 4; i++) {
                    const int pc = wave * (VP / 4) + i;
                    int tok = tv * BLKK + pc * RPP + lane_g / CPRV;
                    tok = tok < Lk ? tok : Lk - 1;
                    const int row = pc * RPP + lane_g / CPRV, phys = lane_g % CPRV;
                    const int logical = D == 128 ? (phys ^ ((row & 3) << 2)) : phys;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vbase + (long)tok * p.v_sl * 2 + logical * 16),
                                                     (__attribute__((address_space(3))) void *)(vs + hh * C::V_IMG_BYTES + pc * 1024), 16, 0, 0);
                }
            } else {
            const unsigned char *vt;
            if constexpr (PAGED) vt = vbase + vti * (long)C::V_IMG_BYTES;      // (tv == it here, see above)
            else
            vt = vbase + (v_tile0 + (long)tv * v_tstride) * (long)C::V_IMG_BYTES;
#pragma unroll
            for (int i = 0; i < VP / 4; i++) {
                const int pc = wave * (VP / 4) + i;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(vt + pc * 1024 + lane_g * 16),
                                                 (__attribute__((address_space(3))) void *)(vs + hh * C::V_IMG_BYTES + pc * 1024), 16, 0, 0);
            }
            }
        }
    };

    // ---- running state -------------------------------------------------------------------------
    v16f o[C::DT];
#pragma unroll
    for (int dt = 0; dt < C::DT; dt++)
#pragma unroll
        for (int i = 0; i < 16; i++) o[dt][i] = 0.0f;
    float m_run = kNegBig, l_run = 0.0f;
    constexpr float OFF = PV_FP8 ? kFp8Offset : 0.0f;

    // K scales of an iteration are fetched one iteration ahead with SCALAR loads (constant address
    // space, wave-uniform index -> s_load, tracked by lgkmcnt).  An ordinary VMEM load here would be
    // fatal for the pipeline: with LDS-DMA in flight hipcc waits vmcnt(0) at the first use of any
    // VGPR-destination load, draining the in-flight tiles every iteration.
    typedef const __attribute__((address_space(4))) float *cfloat_p;
    const cfloat_p ks_c = (cfloat_p)(ks_ptr);
    float ksc[NH][2];
    auto load_kscales = [&](int it, float (&dst)[NH][2]) {
#pragma unroll
        for (int hh = 0; hh < NH; hh++) {
            int tk = it * NH + hh;
            tk = tk < ntk_all ? tk : ntk_all - 1;
            long tb;
            if constexpr (PAGED) tb = ks_slot(tk, page_of(tk));
            else
            tb = (long)(tk >> p.ks_shift) * ks_tstride;
            if (KTHREAD) {      // 4 key scales per 64 keys: token%8/2 (quant_per_thread.py:75-83); lane half g uses 2g, 2g+1
                const float s0 = ks_c[tb], s1 = ks_c[tb + 1], s2 = ks_c[tb + 2], s3 = ks_c[tb + 3];
                dst[hh][0] = g ? s2 : s0;
                dst[hh][1] = g ? s3 : s1;
            } else {
                dst[hh][0] = dst[hh][1] = ks_c[tb];
            }
        }
    };
    // LDS ring.  NSTAGE == 3: tiles it+1 and it+2 are in flight while tile it is consumed; a wave waits
    // only for ITS OWN older DMA group with a counted s_waitcnt vmcnt(N) (N = DMA instructions of the
    // younger group) and then meets the others at a raw s_barrier -- __syncthreads() would drain
    // vmcnt(0) and expose the full L2/HBM latency every iteration (cdna_hip_programming.md T3+T4).
    constexpr int NSTAGE = C::NSTAGE;
    constexpr int DMA_PER_TILE = KP / 4 + NH * (VP / 4);          // per wave
    auto ring_wait = [&](bool younger_in_flight) {
        if (younger_in_flight) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_TILE) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };
    if (n_lim > 0) {
        load_kscales(0, ksc);
        issue_loads(0, 0);
    }
    if (n_lim > 1) issue_loads(1, 1);
    // The Q fragments are fetched AFTER the first tiles' LDS-DMA has been issued: hipcc waits vmcnt(0) at the first use of an
    // ordinary VGPR load, and with the Q loads in front it did so after the first DMA instruction -- the Q round trip and the
    // tiles' round trip ran one after the other in every workgroup's prologue.
    if constexpr (QF == 0) {
        const int8_t *qrow = reinterpret_cast<const int8_t *>(p.q) + q_off + (long)my_row * p.q_sl;
        const bool ok = my_row < Lq_w;
#pragma unroll
        for (int ks = 0; ks < C::KSTEPS; ks++) {
            v4i z = {0, 0, 0, 0};
            qf[ks] = ok ? *reinterpret_cast<const v4i *>(qrow + 32 * ks + 16 * g) : z;
        }
        // this lane's query-row scale (per-block / per-warp / per-thread granularity)
        int slot;
        const int rin = wave * 32 + n;               // row inside the 128-row block
        if (p.q_gran == QG_PER_BLOCK) slot = 0;
        else if (p.q_gran == QG_PER_WARP32) slot = rin >> 5;
        else if (p.q_gran == QG_PER_WARP16) slot = rin >> 4;
        else if (p.q_gran == QG_PER_THREAD16) slot = (rin >> 4) * 8 + (rin & 7);   // per-thread, WARPQ = 16 (core.py:604,969)
        else slot = (rin >> 5) * 8 + (rin & 7);      // per-thread: quant_per_thread.py:27-37
        qsc = qs_ptr[slot * qs_stride];
    } else {
        // Fused Q quantisation.  (The per-thread form has two restatements that must stay bit-equal: chunk_max_kernel's
        // prologue in sage_split_exact.hip and cm_quant_q in sage_chunk_max.h.)  The lane holds channels [32 ks + 16 g, +16) of its row for every ks -- the layout of
        // the MFMA B operand -- so it quantises exactly the bytes it needs.  A per-thread group is the rows
        // r, r+8, r+16, r+24 of the wave's 32-row tile, all 128 channels: lanes n = r (mod 8), both halves g.
        constexpr int QDT = (QF == 1 || QF == 3) ? DT_F16 : DT_BF16;
        constexpr bool QBLOCK = QF >= 3;
        const float premul = QBLOCK ? p.q_premul : 1.0f;
        const uint16_t *qrow = reinterpret_cast<const uint16_t *>(p.q) + q_off + (long)my_row * p.q_sl;
        const bool ok = my_row < Lq_w;
        float x[C::KSTEPS][16];
        float amax = 0.0f;
#pragma unroll
        for (int ks = 0; ks < C::KSTEPS; ks++) {
            v4u raw[2] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
            if (ok) {
                raw[0] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g);
                raw[1] = *reinterpret_cast<const v4u *>(qrow + 32 * ks + 16 * g + 8);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const unsigned w = raw[j >> 3][(j & 7) >> 1];
                float f = ld16<QDT>((uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu)));
                if constexpr (QBLOCK) f *= premul;          // x.to(float32) * sm_scale before the abs-max (quant_per_block.py:35-37)
                x[ks][j] = f;
                amax = fmaxf(amax, fabsf(f));
            }
        }
        if constexpr (QBLOCK) {
            // one scale for the workgroup's 128 rows: the wave's maximum, then the four waves' through 16 bytes of LDS (the K / V ring
            // is receiving its first tiles meanwhile; only this word is waited for)
            amax = fmaxf(amax, __shfl_xor(amax, 1));
            amax = fmaxf(amax, __shfl_xor(amax, 2));
            amax = fmaxf(amax, __shfl_xor(amax, 4));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 8));
        amax = fmaxf(amax, __shfl_xor(amax, 16));
        amax = fmaxf(amax, __shfl_xor(amax, 32));
        if constexpr (QBLOCK) {
            __shared__ float q_amax[4];
            if (lane == 0) q_amax[wave] = amax;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            amax = fmaxf(fmaxf(q_amax[0], q_amax[1]), fmaxf(q_amax[2], q_amax[3]));
        }
        const float sc = quant_scale(amax, QBLOCK ? QS_TRITON : QS_TRITON_THREAD);
        const float y = quant_recip(sc);
        qsc = sc;
#pragma unroll
        for (int ks = 0; ks < C::KSTEPS; ks++) {
            int q8[16];
#pragma unroll
            for (int j = 0; j < 16; j++) q8[j] = QBLOCK ? quant_round_triton(x[ks][j], sc, y) : quant_round_triton_nz(x[ks][j], sc, y);
#pragma unroll
            for (int w = 0; w < 4; w++) qf[ks][w] = (int)pack_int8x4(q8[4 * w], q8[4 * w + 1], q8[4 * w + 2], q8[4 * w + 3]);
        }
    }

    if constexpr (SEED && KVLEN) {
        // as below, for this wave's head (GPACK: an idle wave reads its group's first head and stores nothing); up to 254 chunks stand in
        // front, so the values are requested four at a time instead of one memory round trip each
        // (RAGGED: the split step launch -- the workspace's rows per (sequence, head) are p.lse_sh, a quantity of its own; Lq is the sample's)
        if (my_row < Lq) {
            const int hk0 = hk / p.kv_split;
            long gl;
            const float *sm;
            if constexpr (RAGGED) {
                gl = (long)p.group * p.lse_sh;
                sm = p.seed_max + ((long)b * (p.Hkv / p.kv_split) + hk0) * p.seed_chunks * gl + (long)(h - hk * p.group) * p.lse_sh + my_row;
            } else {
            gl = (long)p.group * Lq;
            sm = p.seed_max + ((long)b * (p.Hkv / p.kv_split) + hk0) * p.seed_chunks * gl + (long)(h - hk * p.group) * Lq + my_row;
            }
            const int c_end = hk - hk0 * p.kv_split;
            int c = 0;
            for (; c + 4 <= c_end; c += 4) {
                const float a0 = sm[c * gl], a1 = sm[(c + 1) * gl], a2 = sm[(c + 2) * gl], a3 = sm[(c + 3) * gl];
                m_run = fmaxf(fmaxf(m_run, fmaxf(a0, a1)), fmaxf(a2, a3));
            }
            for (; c < c_end; c++) m_run = fmaxf(m_run, sm[c * gl]);
        }
    } else if constexpr (SEED) {
        // the running maximum the unsplit call holds in front of this chunk: the maximum of pass 1's values for the chunks before it
        // ([B, Hkv, seed_chunks, group, Lq]; seed_first: the number of pass-1 chunks in front of this launch's chunk 0)
        if (my_row < Lq) {
            const int hk0 = hk / p.kv_split;
            const long gl = (long)p.group * Lq;
            const float *sm = p.seed_max + ((long)b * (p.Hkv / p.kv_split) + hk0) * p.seed_chunks * gl + (long)(h - hk * p.group) * Lq + my_row;
            const int c_end = p.seed_first + (hk - hk0 * p.kv_split);
            for (int c = 0; c < c_end; c++) m_run = fmaxf(m_run, sm[c * gl]);
        }
    }
    SAGE_TSTAMP(2);
    ring_wait(n_lim > 1);
    SAGE_TSTAMP(3);

    int cur = 0;
    // One K/V tile in the general form: masked, ragged, or one of a workgroup's last two (the whole, unmasked tiles in front of them run the
    // software-pipelined loops below).
    auto tile_iter = [&](const int it) {
        const bool more = (it + 1) < n_lim;
        const bool more2 = (it + 2) < n_lim;
        const int nxt = (cur + 1 == NSTAGE) ? 0 : cur + 1;
        float ksc_next[NH][2];
        if (more) load_kscales(it + 1, ksc_next);
        if (more2) issue_loads(it + 2, (nxt + 1 == NSTAGE) ? 0 : nxt + 1);

        // number of 64-key halves with at least one key this wave may attend to (wave-uniform)
        int nact = 0;
#pragma unroll
        for (int hh = 0; hh < NH; hh++) {
            const int key0 = it * KT + hh * BLKK;
            if (key0 < Lk && (!CAUSAL || key0 <= crow0 + 31) && (!WINDOW || key0 + BLKK - 1 > crow0 - wwin)) nact = hh + 1;     // (WINDOW: not wholly in front of the wave's first row's window)
        }
        // ---- attn_mask (Triton-named API only; attn_qk_int8_per_block.py:31-51): additive term per
        //      score in the log2 domain.  bool: 0 / -1e6, and a tile whose whole 128x64 mask block is
        //      False is skipped; float: the mask value itself; out-of-range positions count as False / -1e6.
        float mk[MASK ? NS : 1][16];
        bool skip_tile = false;
        if constexpr (MASK != 0) {
            const unsigned char *mbase = reinterpret_cast<const unsigned char *>(p.mask);
            const long mrow = (long)b * p.m_sb + (long)h * p.m_sh + (long)my_row * p.m_sq;
            int anytrue = 0;
#pragma unroll
            for (int sb = 0; sb < NS; sb++)
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const int key = it * KT + sb * 32 + crow(i, g);
                    const bool inb = (my_row < Lq) && (key < Lk);
                    float add = -1.0e6f;
                    if (inb) {
                        const long idx = mrow + (long)key * p.m_sk;
                        if (MASK == 1) { const bool t = mbase[idx] != 0; add = t ? 0.0f : -1.0e6f; anytrue |= (int)t; }
                        else if (MASK == 2) add = f16_to_f32(reinterpret_cast<const uint16_t *>(mbase)[idx]);
                        else add = bf16_to_f32(reinterpret_cast<const uint16_t *>(mbase)[idx]);
                    }
                    mk[sb][i] = add;
                }
            if (MASK == 1) skip_tile = !__syncthreads_or(anytrue);
        }
        if (nact > 0 && !skip_tile) {
            const unsigned char *ks = smem + cur * C::STAGE_BYTES;
            const unsigned char *vs = ks + C::K_TILE_BYTES;
            const int last_key = it * KT + nact * BLKK - 1;
            const bool full = (MASK == 0) && (nact == NH) && !(CAUSAL && last_key > crow0) && (last_key < Lk) && !(WINDOW && it < nh);

            // ---- S^T = K Q^T (int8 -> int32), NS sub-tiles of 32 keys ----
            v16i s[NS];
#pragma unroll
            for (int sb = 0; sb < NS; sb++) {
#pragma unroll
                for (int i = 0; i < 16; i++) s[sb][i] = 0;        // sub-tiles past the wave's last key are masked below
                if (sb < 2 * nact) {
                    const int krow = sb * 32 + n;
#pragma unroll
                    for (int kk = 0; kk < C::KSTEPS; kk++) {
                        const v4i a = *reinterpret_cast<const v4i *>(ks + krow * D + swz_chunk<D>(krow, 2 * kk + g) * 16);
                        s[sb] = kk == 0 ? mfma_i8_first(a, qf[kk]) : __builtin_amdgcn_mfma_i32_32x32x32_i8(a, qf[kk], s[sb], 0, 0, 0);
                    }
                }
            }

            // ---- scales: c multiplies the raw int32 score into the log2 domain, formed in the reference's order
            //      sm_scale*log2e * (q_scale * k_scale)  (qk_int_sv_f8_cuda_sm89.cuh:263-266,334-335) ----
            float cs[NH][2];
#pragma unroll
            for (int hh = 0; hh < NH; hh++) {
                cs[hh][0] = __builtin_ldexpf(p.sm_scale_log2 * (qsc * ksc[hh][0]), kSUnitLog2);
                cs[hh][1] = KTHREAD ? __builtin_ldexpf(p.sm_scale_log2 * (qsc * ksc[hh][1]), kSUnitLog2) : cs[hh][0];
            }

            // ---- online softmax over the iteration's keys ----
            // The row max is taken on the raw int32 scores (c >= 0, so max commutes with the scale);
            // only the per-(half, scale) maxima are converted.  exp2 / row sum / low-precision pack
            // are fused per 8-register chunk so no float copy of S stays live.
            float m_new;
            if (full) {
                float mxc = -INFINITY;
#pragma unroll
                for (int hh = 0; hh < NH; hh++) {
                    int mx0 = INT_MIN, mx1 = INT_MIN;
#pragma unroll
                    for (int u = 0; u < 2; u++)
#pragma unroll
                        for (int i = 0; i < 16; i++) {
                            if (KTHREAD && (i & 2)) mx1 = max(mx1, s[2 * hh + u][i]);
                            else mx0 = max(mx0, s[2 * hh + u][i]);
                        }
                    // m_temp = fma(max raw score, scale, -offset)  (attn_utils.cuh:372-384)
                    mxc = fmaxf(mxc, __builtin_fmaf(sfl(mx0), cs[hh][0], -OFF));
                    if (KTHREAD) mxc = fmaxf(mxc, __builtin_fmaf(sfl(mx1), cs[hh][1], -OFF));
                }
                m_new = fmaxf(m_run, pair_max(mxc));
            } else {
                float mx = -INFINITY;
#pragma unroll
                for (int sb = 0; sb < NS; sb++)
#pragma unroll
                    for (int i = 0; i < 16; i++) {
                        if (sb < 2 * nact) {
                            const float cc = cs[sb >> 1][(KTHREAD && (i & 2)) ? 1 : 0];
                            const int key = it * KT + sb * 32 + crow(i, g);
                            const bool ok = (key < Lk) && (!CAUSAL || key <= cmy_row) && (!WINDOW || key > cmy_row - wwin);
                            if constexpr (MASK != 0) mx = fmaxf(mx, (ok ? sfl(s[sb][i]) * cc : 0.0f) + mk[sb][i] - OFF);
                            else mx = fmaxf(mx, ok ? __builtin_fmaf(sfl(s[sb][i]), cc, -OFF) : -INFINITY);
                        }
                    }
                m_new = fmaxf(m_run, pair_max(mx));
            }
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
            m_run = m_new;
            if (!TWO_LEVEL) {
#pragma unroll
                for (int dt = 0; dt < C::DT; dt++)
#pragma unroll
                    for (int i = 0; i < 16; i++) o[dt][i] *= alpha;
            }

            // P for chunk c (16 keys) of half hh = registers 8u..8u+7 of S^T tile 2hh + (c>>1):
            // exactly the order of the PV B operand (sage_common.h)
            // Row sum.  The reference's FP16-PV CUDA kernels sum the fp16-ROUNDED probabilities (RS_32_to_16, then the tensor-core
            // row sum mma::rowsum_f16f16f32: qk_int_sv_f16_cuda_sm80.cu:313-320, attn_utils.cuh:529-545, DenominatorAccumUnit =
            // kTensorCore in every instantiation); its Triton kernels and FP8 kernels sum the un-rounded ones
            // (attn_qk_int8_per_block.py:57-60, qk_int_sv_f8_cuda_sm90.cu:317-318).  For FP16 PV the C ABI maps the two forms onto
            // the TWO_LEVEL parameter: false = the CUDA kernels' form (SAGE_PV_ACCUM_SINGLE / _TWO_LEVEL: gfx950 accumulates P.V
            // in FP32 whatever tile buffer the reference would use), true = the Triton kernels' form
            // (SAGE_PV_ACCUM_TRITON: tile product folded into the FP32 output, un-rounded denominator).
            constexpr bool sum_rounded = !PV_FP8 && !TWO_LEVEL;
            // FP8 PV, folded score form (SFOLD): as in the pipelined loop, the scale FMA reads the accumulator's bit pattern and subtracts
            // m + bias * c, rounded once per (row, tile, k scale) -- every tile of a launch uses ONE form, which the oracle mirrors
            constexpr bool GFOLD = PV_FP8 && SFOLD && MASK == 0;
            float rs = 0.0f;
            auto p_chunk = [&](auto masked, auto rnd, int hh, int c, float (&e)[8]) {
                const int sb = 2 * hh + (c >> 1), r0 = (c & 1) * 8;
                // (formed per chunk: two FMAs, and nothing more stays live across the chunks -- kept in registers over the whole tile the
                //  pair tipped two D = 64 instantiations one VGPR over their three-waves budget)
                [[maybe_unused]] const float mbf0 = GFOLD ? __builtin_fmaf(__int_as_float(0x3E22F983), cs[hh][0], m_new) : 0.0f;
                [[maybe_unused]] const float mbf1 = (GFOLD && KTHREAD) ? __builtin_fmaf(__int_as_float(0x3E22F983), cs[hh][1], m_new) : mbf0;
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int i = r0 + j;
                    const float cc = cs[hh][(KTHREAD && (i & 2)) ? 1 : 0];
                    float v;
                    if constexpr (MASK != 0) {
                        const int key = it * KT + sb * 32 + crow(i, g);
                        v = __builtin_amdgcn_exp2f(((key < Lk) ? sfl(s[sb][i]) * cc : 0.0f) + mk[sb][i] - m_new);
                    } else {
                        if constexpr (GFOLD) v = __builtin_amdgcn_exp2f(__builtin_fmaf(__int_as_float(s[sb][i]), cc, -((KTHREAD && (i & 2)) ? mbf1 : mbf0)));
                        else v = __builtin_amdgcn_exp2f(__builtin_fmaf(sfl(s[sb][i]), cc, -m_new));
                        if constexpr (decltype(masked)::value) {
                            const int key = it * KT + sb * 32 + crow(i, g);
                            const bool ok = (sb < 2 * nact) && (key < Lk) && (!CAUSAL || key <= cmy_row) && (!WINDOW || key > cmy_row - wwin);
                            v = ok ? v : 0.0f;
                        }
                    }
                    e[j] = v;
                    if constexpr (decltype(rnd)::value) rs += (float)(_Float16)v;
                    else rs += v;
                }
            };

            if constexpr (PV_FP8) {
                int pw[NH][8];                   // 32 fp8 per 64-key half = B operand of one K=64 MFMA
                auto build_p = [&](auto masked) {
#pragma unroll
                    for (int hh = 0; hh < NH; hh++)
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            float e[8];
                            p_chunk(masked, std::false_type{}, hh, c, e);
                            int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], __float_as_int(e[0]), false);   // high half is overwritten next
                            w0 = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], w0, true);
                            int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[4], e[5], __float_as_int(e[4]), false);
                            w1 = __builtin_amdgcn_cvt_pk_fp8_f32(e[6], e[7], w1, true);
                            pw[hh][2 * c] = w0;
                            pw[hh][2 * c + 1] = w1;
                        }
                };
                if (full) build_p(std::false_type{});
                else build_p(std::true_type{});
                l_run = l_run * alpha + rs;      // lane-partial; the pair is summed in the epilogue
                auto pv = [&](auto fold_tag) {
                    constexpr bool FOLD = decltype(fold_tag)::value;     // tile product from zero, then O = O * alpha + T
#pragma unroll
                    for (int dt = 0; dt < C::DT; dt++) {
                        const int drow = dt * 32 + n;
                        v16f acc;
                        if (FOLD) {
#pragma unroll
                            for (int i = 0; i < 16; i++) acc[i] = 0.0f;
                        } else acc = o[dt];
#pragma unroll
                        for (int hh = 0; hh < NH; hh++) {
                            if (hh < nact) {
                                const unsigned char *vr = vs + hh * C::V_IMG_BYTES + drow * 64;
                                const v4u va = *reinterpret_cast<const v4u *>(vr + swz_chunk<64>(drow, 2 * g) * 16);
                                const v4u vb = *reinterpret_cast<const v4u *>(vr + swz_chunk<64>(drow, 2 * g + 1) * 16);
                                // one K = 64 FP8 MFMA (the plain form: no block scales)
                                const v8i av = {(int)va[0], (int)va[1], (int)va[2], (int)va[3], (int)vb[0], (int)vb[1], (int)vb[2], (int)vb[3]};
                                const v8i bv = {pw[hh][0], pw[hh][1], pw[hh][2], pw[hh][3], pw[hh][4], pw[hh][5], pw[hh][6], pw[hh][7]};
                                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, acc, 0, 0, 0, 0, 0, 0);    // (zero scale operands: hipcc selects the plain v_mfma_f32_32x32x64_f8f6f4, no scale VGPRs)
                            }
                        }
                        if (FOLD) {
#pragma unroll
                            for (int i = 0; i < 16; i++) o[dt][i] = __builtin_fmaf(o[dt][i], alpha, acc[i]);
                        } else o[dt] = acc;
                    }
                };
                if constexpr (!TWO_LEVEL) pv(std::false_type{});
                else pv(std::true_type{});
            } else {
                v8h pb[NH][4];
                auto build_p = [&](auto masked, auto rnd) {
#pragma unroll
                    for (int hh = 0; hh < NH; hh++)
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            float e[8];
                            p_chunk(masked, rnd, hh, c, e);
#pragma unroll
                            for (int j = 0; j < 8; j++) pb[hh][c][j] = (_Float16)e[j];
                        }
                };
                if (full) build_p(std::false_type{}, std::integral_constant<bool, sum_rounded>{});
                else build_p(std::true_type{}, std::integral_constant<bool, sum_rounded>{});
                l_run = l_run * alpha + rs;
                auto pv = [&](auto fold_tag) {
                    constexpr bool FOLD = decltype(fold_tag)::value;
#pragma unroll
                    for (int dt = 0; dt < C::DT; dt++) {
                        v16f acc;
                        if (FOLD) {
#pragma unroll
                            for (int i = 0; i < 16; i++) acc[i] = 0.0f;
                        } else acc = o[dt];
#pragma unroll
                        for (int hh = 0; hh < NH; hh++) {
                            if (hh < nact) {
#pragma unroll
                                for (int c = 0; c < 4; c++) {
                                    const v8h a = __builtin_bit_cast(v8h, v_frag(vs + hh * C::V_IMG_BYTES, dt, c));
                                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pb[hh][c], acc, 0, 0, 0);
                                }
                            }
                        }
                        if (FOLD) {
#pragma unroll
                            for (int i = 0; i < 16; i++) o[dt][i] = __builtin_fmaf(o[dt][i], alpha, acc[i]);
                        } else o[dt] = acc;
                    }
                };
                if constexpr (!TWO_LEVEL) pv(std::false_type{});
                else pv(std::true_type{});
            }
        }

        if (more) {
#pragma unroll
            for (int hh = 0; hh < NH; hh++) { ksc[hh][0] = ksc_next[hh][0]; ksc[hh][1] = ksc_next[hh][1]; }
        }
        ring_wait(more2);
        cur = nxt;
    };

    int it = 0;
    if constexpr (WINDOW) {
        // the head tiles, then the ring again from slot 0 for what follows (the pipelined loop enters with its first tile there): the last head
        // tile ended behind vmcnt(0) and a barrier, so every wave is past its reads of all three slots
        if (nh > 0) {
#pragma nounroll
            for (; it < nh; it++) tile_iter(it);
            n_lim = n_iters;
            cur = 0;
            if (it < n_iters) {
                load_kscales(it, ksc);
                issue_loads(it, 0);
                if (it + 1 < n_iters) issue_loads(it + 1, 1);
                ring_wait(it + 1 < n_iters);
            }
        }
    }
    if constexpr (MASK == 0) {
        static_assert(NH == 1 && NSTAGE == 3, "the pipelined loops are written for 64-key iterations on the 3-slot ring");
        constexpr bool SIX_BODIES = D == 128 || PV_FP8;         // the pipelined loops' ring slot as a compile-time constant (see the FP8 loop; not D = 64 FP16 PV)
        // whole tiles: it < Lk/64; unmasked for wave 0 (hence all waves): 64 it + 63 <= 128 qblk; two whole tiles follow
        int n_steady = Lk / KT - 2;
        n_steady = n_steady < n_iters - 2 ? n_steady : n_iters - 2;
        if (CAUSAL) {                                  // unmasked for wave 0 (hence all waves): 64 it + 63 <= 128 qblk - kchunk0
            int nd = (qblk * BLKQ - kchunk0) / KT;
            nd = nd > 0 ? nd : 0;
            n_steady = n_steady < nd ? n_steady : nd;
        }
        // DIAG_PIPE (causal): when exactly two tiles follow the steady ones and both are whole, they run through the pipelined body as well (masked
        // there) instead of as general iterations -- also when there is no steady tile at all (the first query block)
        // (FP16 PV: only behind at least one steady tile -- its first body is a form of its own -- and at D = 128: the D = 64 instantiations spill
        //  5-10 VGPRs under their three-waves limit with the two extra bodies)
        constexpr bool DIAG_PIPE = CAUSAL && SAGE_DIAG_PIPE && (PV_FP8 || D == 128);
        // (QSTART: with an offset that is no multiple of 64 the diagonal crosses three tiles of a query block and rows in front of key 0 see
        //  nothing at all -- which the last-tile bodies, whose masked scores still set a row maximum, do not provide for: general iterations.
        //  With a multiple of 64 every row of a block that runs these bodies sees key 0: they need n_iters >= 2, i.e. 128 qblk + 128 - kchunk0 > 64,
        //  so crow0 of wave 0 is > -64, hence >= 0; the one negative case, crow0 = -64, has lim = 1 and runs no pipelined body)
        // (WINDOW: and neither of the two is a head tile -- every row then sees its diagonal key in them, and whole rows of the first)
        bool diag_ok = DIAG_PIPE && (!QSTART || (kchunk0 & (KT - 1)) == 0) && (n_steady > 0 ? n_iters - n_steady == 2 : (PV_FP8 && n_iters == 2 && Lk >= 2 * KT));
        if constexpr (WINDOW) diag_ok = diag_ok && nh <= (n_steady > 0 ? n_steady : 0);
        // TAIL_PIPE (non-causal FP8 PV): the two whole tiles the steady loop leaves (it looks two tiles ahead) and a ragged last one behind them take the
        // pipelined body as well -- keys past Lk masked like keys behind the diagonal, the ragged tile requested in the general (clamped) form
        // (FP16 PV, D = 128: the two whole tiles of a call whose Lk is a multiple of 64, behind at least one steady tile -- kinds 1 and 2 as they are)
        constexpr bool TAIL_PIPE = !CAUSAL && SAGE_TAIL_PIPE && (PV_FP8 || D == 128);
        const bool tail_ok = TAIL_PIPE && n_steady == Lk / KT - 2 &&
                             (PV_FP8 ? (n_steady >= 0 && n_iters - n_steady <= (SAGE_TAIL_PIPE == 2 ? 2 : 3)) : (n_steady > 0 && n_iters - n_steady == 2));

        if constexpr (PV_FP8) {
#include "sage_attn_loop_f8.h"          // (the FP8-PV pipelined loop, its last-tile bodies and its drain: a fragment of this function)
        } else {
#include "sage_attn_loop_f16.h"         // (the FP16-PV pipelined loop)
        }
    }
    if constexpr (MASK == 0) {
        // the general iterations' and the epilogue's per-lane values (LDS offsets, the lane's row) are re-derived here from a lane index the
        // compiler cannot see through: formed before the pipelined loops they stay live across them, and the D = 64 instantiations, which
        // have no register to spare under their three-waves limit, spill them
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_g));
        n = lane_g & 31;
        g = lane_g >> 5;
        my_row = row0 + n;
        cmy_row = my_row - kchunk0;
    }
#pragma nounroll
    for (; it < n_iters; it++) tile_iter(it);
    SAGE_TSTAMP(4);
    __syncthreads();      // (raw barriers above do not order the epilogue's LDS reuse against stray waits)
    SAGE_TSTAMP(5);
    // persistent launch: the next ticket is requested here, behind the last tile, and read after the output rows are on their way
    if (pers && !own_empty) {
        if (wave == 0 && lane_g == 0) next_k_v = __hip_atomic_fetch_add(kpl()->sched + 32 * my_queue(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        have_next = true;
    }

    // ---- epilogue: normalise, (x v_scale, + v_mean), cast, transpose through LDS, store rows ----
    __builtin_amdgcn_s_setreg(kHwregModeFp16Ovfl, 0);
    const float l_tot = pair_sum(l_run);
    const float inv = l_tot > 0.0f ? __builtin_amdgcn_rcpf(l_tot) : 0.0f;
    if (p.lse != nullptr && g == 0 && my_row < Lq_w) {
        long lidx;
        if constexpr (RAGGED && SEED) lidx = ((long)b * p.Hq + h) * p.lse_sh + my_row;      // (the split step launch: lse_part [B, Hq * S, p.lse_sh], dense)
        else
        if constexpr (RAGGED) {
            // the packed index, from the clamped first row: the two words are read and clamped again here (a pointer the compiler cannot see
            // through) instead of a value kept in an SGPR across the key loop
            typedef const __attribute__((address_space(4))) int *cint_p;
            typedef const __attribute__((address_space(4))) RaggedArgs *kragged_t;
            kparams_t k3 = kp;
            asm volatile("" : "+s"(k3));
            const kragged_t r = (kragged_t)((const __attribute__((address_space(4))) char *)k3 + kRaggedArgsOffset);
            const int bu = __builtin_amdgcn_readfirstlane(b);
            int q0e, lqe;
            ragged_rows(((cint_p)r->cu_q)[bu], ((cint_p)r->cu_q)[bu + 1], r->total_q, p.Lq, q0e, lqe);
            lidx = (long)h * p.lse_sh + q0e + my_row;
        } else
        lidx = (p.cu_q != nullptr) ? ((long)h * p.lse_sh + p.cu_q[b] + my_row)
                                        : ((long)b * p.Hq + h) * (long)p.Lq + my_row;
        p.lse[lidx] = __builtin_amdgcn_logf(l_tot) + m_run;   // v_log_f32 is log2
    }
    // all waves are past the last tile barrier: the staging LDS is free
    unsigned char *obuf = smem + wave * (32 * D * 2);
    // per-channel epilogue factors, fetched per 32-wide d tile as straight-line batches of 16-byte
    // vectors (a per-element "load if non-null" makes hipcc branch around every load and wait
    // vmcnt(0) each time: 128 serial L2 round trips per workgroup)
    const long vbh = SEED ? (long)b * (p.Hkv / p.kv_split) + hk / p.kv_split : (long)b * p.Hkv + hk;      // (the seeded split: the unsplit kv head)
    const float *vsc = PV_FP8 ? p.v_scale + vbh * D : nullptr;
    const float *vmn = (p.v_mean != nullptr) ? p.v_mean + vbh * D : nullptr;
    // every factor of the tile is requested before the first one is used: one exposed memory latency per workgroup
    // instead of one per 32-channel tile (the slot is idle for the co-resident workgroup's sake until this one retires)
    v4f sc4[C::DT][4], mn4[C::DT][4];
    // (KVLEN) all ones, or zero for a sample without keys: a bit mask the compiler cannot see through -- as a select on Lk it moved the factor
    // loads below behind a branch, 0.6 us per work item (profiles/kv_lens_trace_wan.txt)
    // (a packed bottom-right launch -- QSTART without KVLEN -- likewise: a sequence without keys has no V scales of its own)
    constexpr bool KEEP = KVLEN || QSTART;
    [[maybe_unused]] unsigned keep = (!KEEP || Lk > 0) ? ~0u : 0u;
    if constexpr (KEEP) asm volatile("" : "+v"(keep));
#pragma unroll
    for (int dt = 0; dt < C::DT; dt++) {
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const v4f one = {1.0f, 1.0f, 1.0f, 1.0f};
            sc4[dt][r4] = PV_FP8 ? *reinterpret_cast<const v4f *>(vsc + dt * 32 + 8 * r4 + 4 * g) : one;
        }
        if (vmn != nullptr) {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) mn4[dt][r4] = *reinterpret_cast<const v4f *>(vmn + dt * 32 + 8 * r4 + 4 * g);
        } else {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) { const v4f z = {0.0f, 0.0f, 0.0f, 0.0f}; mn4[dt][r4] = z; }
        }
    }
#pragma unroll
    for (int dt = 0; dt < C::DT; dt++) {
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) {
            const int d0 = dt * 32 + 8 * r4 + 4 * g;           // 4 consecutive d: regs 4*r4 .. 4*r4+3
            float x[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                x[j] = o[dt][4 * r4 + j] * inv;
                if (PV_FP8) x[j] *= sc4[dt][r4][j];
                if constexpr (KEEP) x[j] = __uint_as_float(__float_as_uint(x[j]) & keep);      // (a sample without keys: +0 whatever its scale slots hold)
                x[j] += mn4[dt][r4][j];
            }
            if constexpr (SEED) {      // FP32 partial rows straight from the registers: four channels per lane
                if (my_row < Lq_w) *reinterpret_cast<v4f *>(reinterpret_cast<float *>(p.o) + o_off + (long)my_row * p.o_sl + d0) = v4f{x[0], x[1], x[2], x[3]};
                continue;
            }
            v2u pk;
            if (p.out_dtype == DT_F16) {
                pk[0] = (unsigned)f32_to_f16_rne(x[0]) | ((unsigned)f32_to_f16_rne(x[1]) << 16);
                pk[1] = (unsigned)f32_to_f16_rne(x[2]) | ((unsigned)f32_to_f16_rne(x[3]) << 16);
            } else {
                pk[0] = (unsigned)f32_to_bf16_rne(x[0]) | ((unsigned)f32_to_bf16_rne(x[1]) << 16);
                pk[1] = (unsigned)f32_to_bf16_rne(x[2]) | ((unsigned)f32_to_bf16_rne(x[3]) << 16);
            }
            const int q8 = d0 >> 2;                             // 8-byte chunk index in the row
            const int Q = (q8 >> 1) ^ (n & 7);                 // 16-B chunk, XOR-swizzled by row
            *reinterpret_cast<v2u *>(obuf + n * (D * 2) + Q * 16 + (q8 & 1) * 8) = pk;
        }
    }
    // each wave transposes through its OWN 32-row region: its ds_writes and ds_reads execute in order, no workgroup barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if constexpr (!SEED) {
        constexpr int LPR = D * 2 / 16;          // lanes per row (16 B each)
        constexpr int RPP = 64 / LPR;            // rows per pass
        unsigned char *obase = reinterpret_cast<unsigned char *>(p.o) + 2 * o_off;
#pragma unroll
        for (int pass = 0; pass < 32 / RPP; pass++) {
            const int r = pass * RPP + lane_g / LPR, Q = lane_g % LPR;
            const v4u val = *reinterpret_cast<const v4u *>(obuf + r * (D * 2) + (Q ^ (r & 7)) * 16);
            const int grow = row0 + r;
            if (grow < Lq_w) *reinterpret_cast<v4u *>(obase + 2 * ((long)grow * p.o_sl) + Q * 16) = val;
        }
    }
#if SAGE_ATTN_TRACE
    SAGE_TSTAMP(6);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    SAGE_TSTAMP(7);
    if (wave == 0 && p.trace != nullptr && bid < p.trace_wgs) {
        if (lane < 8 || lane == 8 || lane >= 13) p.trace[16 * bid + lane] = ttrace[lane];
        if (lane == 9) p.trace[16 * bid + 9] = __builtin_amdgcn_s_getreg((31 << 11) | 4);      // HW_REG_HW_ID
        if (lane == 10) p.trace[16 * bid + 10] = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
        if (lane == 11) p.trace[16 * bid + 11] = blockIdx.x;
        if (lane == 12) p.trace[16 * bid + 12] = (unsigned)qblk;
    }
#endif
    } while (0);
    if (!pers) break;
    // (the barrier also separates this item's LDS transposes from the next item's first tiles)
    if (wave_s == 0) { const int t = resolve_ticket(); if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) s_ticket[tpar] = t; }
    __syncthreads();
    bid = __builtin_amdgcn_readfirstlane(s_ticket[tpar]);      // (wave-uniform: everything derived from it stays in SGPRs)
    tpar ^= 1;
    }
    // A persistent launch leaves its counter block as it found it: every workgroup checks out once it has no ticket left (all its ticket
    // atomics have returned by then -- their values were consumed), and the last one to leave writes the zeros, so the caller can hand the
    // same block to the next launch of the stream without a memset in between (round 6; the Python layer keeps one block per stream).
    if constexpr (PERS_OK) {
        if (pers && wave_s == 0) {
            unsigned *const sched = kpl()->sched;
            const int lane_x = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
            unsigned gone = 0;
            if (lane_x == 0) gone = __hip_atomic_fetch_add(sched + kAttnSchedDoneWord, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if ((unsigned)__builtin_amdgcn_readfirstlane(gone) + 1u == gridDim.x) {
                if (lane_x < 32) __hip_atomic_store(sched + 32 * lane_x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (lane_x == 32) __hip_atomic_store(sched + kAttnSchedDoneWord, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
#ifdef SAGE_ATTN_BODY_LIST_DEFAULTED
#undef SAGE_ATTN_BODY_LIST_DEFAULTED
#undef SAGE_ATTN_BODY_LIST
#endif
