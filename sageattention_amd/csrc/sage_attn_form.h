// sage_attn_form.h -- the identity of a member of the attention kernel family as one value: which flags of sage_attn_kernel.h are on (AttnForm),
// its packing into the kernel's single template argument, the rules that follow from a form alone (which forms exist, waves per SIMD, ticket
// loop, persist_ok), the form a launch needs (attn_form) and the forms each instantiation unit holds (unit_forms / Forms<...>).  Host-side
// constant expressions only: no device code, and not the kernel header -- the kernel, the launch header, the dispatcher and the units include it.
#pragma once
#include "sage_kernels.h"
#include <cstdint>
#include <utility>

namespace sage {

// What each flag MEANS is documented above sage_attn_kernel (sage_attn_kernel.h); AttnVariant (sage_kernels.h) is the launch's view of it.
struct AttnForm {
    int D = 128;                                             // head size, 64 / 128
    bool pv_fp8 = false, causal = false, kthread = false;    // FP8 PV (else FP16 PV); per-thread k scale groups
    bool two_level = false;                                  // FP8 PV: two-level accumulation; FP16 PV: the Triton kernel form
    int mask = 0, qf = 0;                                    // attn_mask kind 0 .. 3; q: 0 INT8, 1 / 2 fp16 / bf16 quantised per thread group, 3 / 4 per block
    bool gpack = false;
    bool sfold = true;                                       // the folded FP8 score form (FP16 PV has one form and says true)
    bool cpers = false, vrows = false, seed = false, window = false, qstart = false, kvlen = false;
};

// The canonical packing: field positions inside the kernel's template argument (POS = lowest bit, LEN = bits).  tools/kernel_form.py reads these
// lines to decode a kernel's name.  A new flag takes the next free bit (14 are left) and a place in SAGE_FORM_FIELDS.
enum : uint32_t {
    FORM_D128_POS = 0,       FORM_D128_LEN = 1,       // D == 128 (else 64)
    FORM_PV_FP8_POS = 1,     FORM_PV_FP8_LEN = 1,
    FORM_CAUSAL_POS = 2,     FORM_CAUSAL_LEN = 1,
    FORM_KTHREAD_POS = 3,    FORM_KTHREAD_LEN = 1,
    FORM_TWO_LEVEL_POS = 4,  FORM_TWO_LEVEL_LEN = 1,
    FORM_MASK_POS = 5,       FORM_MASK_LEN = 2,
    FORM_QF_POS = 7,         FORM_QF_LEN = 3,
    FORM_GPACK_POS = 10,     FORM_GPACK_LEN = 1,
    FORM_SFOLD_POS = 11,     FORM_SFOLD_LEN = 1,
    FORM_CPERS_POS = 12,     FORM_CPERS_LEN = 1,
    FORM_VROWS_POS = 13,     FORM_VROWS_LEN = 1,
    FORM_SEED_POS = 14,      FORM_SEED_LEN = 1,
    FORM_WINDOW_POS = 15,    FORM_WINDOW_LEN = 1,
    FORM_QSTART_POS = 16,    FORM_QSTART_LEN = 1,
    FORM_KVLEN_POS = 17,     FORM_KVLEN_LEN = 1,
    FORM_BITS = 18
};
#define SAGE_FORM_FIELDS(X) /* every field but D */                                                                                  \
    X(pv_fp8, PV_FP8) X(causal, CAUSAL) X(kthread, KTHREAD) X(two_level, TWO_LEVEL) X(mask, MASK) X(qf, QF) X(gpack, GPACK) X(sfold, SFOLD) \
    X(cpers, CPERS) X(vrows, VROWS) X(seed, SEED) X(window, WINDOW) X(qstart, QSTART) X(kvlen, KVLEN)

constexpr uint32_t pack(const AttnForm &f)
{
    uint32_t w = (uint32_t)(f.D == 128) << FORM_D128_POS;
#define SAGE_FORM_PACK(field, NAME) w |= (uint32_t)f.field << FORM_##NAME##_POS;
    SAGE_FORM_FIELDS(SAGE_FORM_PACK)
#undef SAGE_FORM_PACK
    return w;
}
constexpr AttnForm unpack(uint32_t w)
{
    AttnForm f;
    f.D = (w >> FORM_D128_POS & 1u) ? 128 : 64;
#define SAGE_FORM_UNPACK(field, NAME) f.field = w >> FORM_##NAME##_POS & ((1u << FORM_##NAME##_LEN) - 1u);
    SAGE_FORM_FIELDS(SAGE_FORM_UNPACK)
#undef SAGE_FORM_UNPACK
    return f;
}

// Which flags may meet: the rule a form breaks, or null.  pack() is one-to-one on the forms this admits (D and qf are the only fields whose
// range is smaller than their bits), so a form gives one instantiation however it was written.
constexpr const char *form_error(const AttnForm &f)
{
    const bool fused_f8 = f.pv_fp8 && f.kthread && f.two_level && !f.sfold && f.mask == 0 && (f.qf == 1 || f.qf == 2) && !f.cpers && !f.vrows;
    const bool packed_f8 = f.pv_fp8 && !f.kthread && f.two_level && !f.sfold && f.mask == 0 && f.qf >= 3 && !f.vrows && !f.seed;
    if ((f.D != 64 && f.D != 128) || f.mask < 0 || f.mask > 3 || f.qf < 0 || f.qf > 4) return "D is 64 or 128, mask 0 .. 3, qf 0 .. 4";
    if (!f.pv_fp8 && !f.sfold) return "FP16 PV has one score form";
    if (f.cpers && !f.causal) return "the ticket loop as a flag: causal kernels (non-causal unmasked ones always carry it)";
    if (f.vrows && (f.pv_fp8 || f.mask != 0)) return "V rows in place: FP16 PV, unmasked, dense launches";
    if (f.seed && !fused_f8) return "the seeded split: FP8 PV, fused per-thread Q, exact score form, dense";
    if (f.kvlen && !fused_f8) return "per-sample key lengths: FP8 PV, fused per-thread Q, exact score form, dense";
    if (f.seed && f.kvlen && (f.window || f.qstart != f.causal)) return "the kv_lens split: no window, and its causal kernels are the offset kernels";
    if (f.qstart && !(f.causal && (f.kvlen || packed_f8)))
        return "query offsets: the causal kv_lens kernels (dense, p.cu_qs), or a packed launch's bottom-right alignment (FP8 PV, per-block Q, two-level; with or without a window)";
    if (f.window && !f.qstart) return "the sliding window: the q_start kernels";
    if (f.gpack && !f.kvlen) return "packed GQA groups: the kv_lens kernels (dense, p.Lq <= 32)";
    return nullptr;
}
constexpr bool valid(const AttnForm &f) { return form_error(f) == nullptr; }

// ---- what follows from a form alone, for the kernel and for its launch --------------------------------------------------------------------
// __launch_bounds__ waves / SIMD the register allocator must allow: the software-pipelined loops carry two score tiles, which at D = 128 is
// 2 waves (248 VGPRs); D = 64 fits 3 (167); the attn_mask variants 2.  The packed window's ticket kernel at D = 64 -- the general iteration
// instantiated twice next to the ticket loop's state -- needs 4 VGPRs more than three waves leave, 172 against 168: it is built for 2 waves
// rather than with scratch.
constexpr int min_waves(const AttnForm &f)
{
    const bool packed_window_tickets = f.window && f.qstart && !f.kvlen && f.cpers;
    return (f.mask != 0 || (packed_window_tickets && f.D == 64)) ? 2 : (f.D == 64 ? 3 : 2);
}
// the ticket loop is compiled into the kernel (its PERS_OK): non-causal unmasked kernels and CPERS ones; packed GQA groups and the kv_lens split
// take the ordinary launch alone
constexpr bool ticket_loop(const AttnForm &f) { return (!f.causal || f.cpers) && f.mask == 0 && !f.gpack && !(f.seed && f.kvlen); }
// ... and launch_kernel may take it (its persist_ok): every split launch keeps the hardware's dispatch, the exact split's non-causal kernels too
// although they carry the loop
constexpr bool persist_ok(const AttnForm &f) { return ticket_loop(f) && !f.seed; }

// ---- instantiations name only what is on: form(D).fp8().causal(c).kthread().two_level().qf(f).kvlen() ---------------------------------------
struct FormBuilder {
    AttnForm f;
    constexpr operator AttnForm() const { return f; }
    constexpr FormBuilder fp8() const { FormBuilder b = *this; b.f.pv_fp8 = true; b.f.sfold = false; return b; }      // FP8 PV, the exact score form
    constexpr FormBuilder folded() const { return sfold(); }
#define SAGE_FORM_SET(field, NAME) constexpr FormBuilder field(int on = 1) const { FormBuilder b = *this; b.f.field = on; return b; }
    SAGE_FORM_FIELDS(SAGE_FORM_SET)
#undef SAGE_FORM_SET
};
constexpr FormBuilder form(int D) { FormBuilder b{}; b.f.D = D; return b; }      // FP16 PV, INT8 q, everything off

// ---- the form a launch needs (after route_exists() of sage_attn.hip, which checks the parameter block against the variant) --------------------
inline AttnForm attn_form(const AttnParams &p, const AttnVariant &v, const AttnLaunchOpts &o)
{
    // kthread / two_level as the variant says: fused per-thread Q comes with kthread and two_level = pv_fp8 (FP16 PV accumulates straight in
    // FP32), fused per-block Q with per-block k scales and, FP16 PV, the Triton form -- route_exists() has checked that, a form no unit holds is refused
    FormBuilder b = form(v.head_dim).pv_fp8(v.pv_fp8).causal(v.causal).kthread(v.kthread).two_level(v.two_level).mask(v.mask_kind).qf(v.qf);
    b = b.sfold(!v.pv_fp8 || o.fp8_folded).vrows(p.v_rows != 0).seed(v.seeded).kvlen(v.kv_lens).gpack(v.gqa_pack).window(v.window > 0);
    // causal launches take the ticket route only over a packed batch's work list (items of very different lengths, heaviest first: +2.9 % at
    // C4), in instantiations of their own: the fused per-block Q kernels; dense causal launches keep the hardware's dispatch, which their work
    // order is built on
    b = b.cpers(v.causal && v.qf >= 3 && p.cu_q != nullptr && p.work_items != nullptr);
    // offsets of their own (q_start), a window (p.cu_qs nullable), a packed launch's bottom-right alignment, the kv_lens split's causal kernels
    return b.qstart(v.q_start || v.window > 0 || v.bottom_right || (v.seeded && v.kv_lens && v.causal));
}

// ---- the instantiation units sage_attn_d{128,64}_<unit>.hip (the split exists for build time only: they compile in parallel) -------------------
#define SAGE_ATTN_UNITS(X) X(F8) X(F8F) X(F16) X(F8V) X(F8VB) X(F8VBW) X(F8S) X(F8K) X(F8Q) X(F8W) X(F8G) X(F8KS)
#define SAGE_UNIT_ENUM(U) UNIT_##U,
enum AttnUnit : int { SAGE_ATTN_UNITS(SAGE_UNIT_ENUM) UNIT_COUNT };
#undef SAGE_UNIT_ENUM

// which unit holds a form
constexpr AttnUnit unit_of(const AttnForm &f)
{
    if (f.seed) return f.kvlen ? UNIT_F8KS : UNIT_F8S;                           // pass 2 of the exact splits
    if (f.gpack) return UNIT_F8G;                                                // the kv_lens family for decode-shaped calls
    if (f.kvlen) return f.window ? UNIT_F8W : f.qstart ? UNIT_F8Q : UNIT_F8K;    // the kv_lens family
    if (f.qstart) return f.window ? UNIT_F8VBW : UNIT_F8VB;                      // packed batches, bottom-right
    if (f.pv_fp8 && f.qf >= 3) return UNIT_F8V;                                  // packed batches, FP8 PV with the per-block Q quantiser
    return !f.pv_fp8 ? UNIT_F16 : f.sfold ? UNIT_F8F : UNIT_F8;                  // one head size, PV format and FP8 score form each
}

// the forms a unit holds
struct FormList {
    uint32_t v[40] = {};
    int n = 0;
    constexpr void add(const AttnForm &f) { v[n++] = pack(f); }
};
constexpr FormList unit_forms(AttnUnit u, int D)
{
    FormList l;
    const FormBuilder f8 = form(D).fp8();
    const FormBuilder base = u == UNIT_F16 ? form(D) : u == UNIT_F8F ? f8.folded() : f8;      // (F8 / F8F / F16)
    const FormBuilder fused = f8.kthread().two_level();      // the fused per-thread Q quantiser, FP8 PV two-level, exact: the kv_lens family, the splits
    const FormBuilder packed = f8.causal().two_level();      // packed bottom-right: per-block Q, FP8 PV two-level, exact
    for (int c = 0; c < 2; c++)                              // causal
        for (int h = 0; h < 2; h++)                          // fp16 / bf16 q where q is quantised in the prologue (h = 0 alone: what has no such axis)
            switch (u) {
            case UNIT_F8: case UNIT_F8F: case UNIT_F16:
                // INT8 q: causal x k-scale groups x accumulation; the fused per-thread Q quantiser (FP16 PV: straight FP32 accumulation)
                if (h == 0)
                    for (int k = 0; k < 2; k++)
                        for (int t = 0; t < 2; t++) l.add(base.causal(c).kthread(k).two_level(t));
                l.add(base.causal(c).kthread().two_level(u != UNIT_F16).qf(1 + h));
                if (u != UNIT_F16) break;
                // FP16 PV alone: the fused per-block Q quantiser (the Triton-named API, dense or packed; causal over a work list with the ticket loop) ...
                l.add(base.causal(c).two_level().qf(3 + h));
                if (c) l.add(base.causal().two_level().qf(3 + h).cpers());
                // ... and V rows in place (fp16 q): INT8 q in every grouping and both forms, q quantised per thread group or per block
                if (h == 0) {
                    for (int k = 0; k < 2; k++)
                        for (int t = 0; t < 2; t++) l.add(base.causal(c).kthread(k).two_level(t).vrows());
                    l.add(base.causal(c).kthread().qf(1).vrows());
                    l.add(base.causal(c).two_level().qf(3).vrows());
                }
                break;
            case UNIT_F8V:      // packed batches: per-block Q, two-level or single accumulation; causal over a work list with the ticket loop
                for (int t = 0; t < 2; t++) {
                    l.add(f8.causal(c).two_level(t).qf(3 + h));
                    if (c) l.add(f8.causal().two_level(t).qf(3 + h).cpers());
                }
                break;
            case UNIT_F8VB:  l.add(packed.qf(3 + h).cpers(c).qstart()); break;                 // (c: with and without the ticket loop)
            case UNIT_F8VBW: l.add(packed.qf(3 + h).cpers(c).qstart().window()); break;
            case UNIT_F8S:   l.add(fused.causal(c).qf(1 + h).seed()); break;
            case UNIT_F8K:   l.add(fused.causal(c).qf(1 + h).kvlen()); break;
            case UNIT_F8Q:   if (c) l.add(fused.causal().qf(1 + h).kvlen().qstart()); break;
            case UNIT_F8W:   if (c) l.add(fused.causal().qf(1 + h).kvlen().qstart().window()); break;
            case UNIT_F8G:      // the four members of the kv_lens family: lengths non-causal and causal, query offsets, a window on top
                l.add(fused.causal(c).qf(1 + h).gpack().kvlen());
                if (c) l.add(fused.causal().qf(1 + h).gpack().kvlen().qstart());
                if (c) l.add(fused.causal().qf(1 + h).gpack().kvlen().qstart().window());
                break;
            case UNIT_F8KS:     // non-causal with lengths or causal with offsets, each unpacked and with packed GQA groups
                for (int g = 0; g < 2; g++) l.add(fused.causal(c).qf(1 + h).gpack(g).seed().kvlen().qstart(c));
                break;
            default: break;
            }
    if (u == UNIT_F16)      // the attn_mask kernels: INT8 q, per-block scales, non-causal, the Triton form
        for (int m = 1; m <= 3; m++) l.add(base.two_level().mask(m));
    return l;
}

// every listed form is valid, stands in the unit unit_of() names -- so in one list only -- and stands there once
constexpr bool unit_ok(AttnUnit u, int D)
{
    const FormList l = unit_forms(u, D);
    for (int i = 0; i < l.n; i++) {
        const AttnForm f = unpack(l.v[i]);
        if (!valid(f) || f.D != D || unit_of(f) != u) return false;
        for (int j = 0; j < i; j++)
            if (l.v[j] == l.v[i]) return false;
    }
    return l.n > 0;
}
#define SAGE_UNIT_CHECK(U) static_assert(unit_ok(UNIT_##U, 128) && unit_ok(UNIT_##U, 64), "unit " #U ": an invalid form, one of another unit, or one listed twice");
SAGE_ATTN_UNITS(SAGE_UNIT_CHECK)
#undef SAGE_UNIT_CHECK

// the same lists as types: Forms<F...>, what the launcher folds over (sage_attn_launch.h)
template <uint32_t... F> struct Forms {};
template <AttnUnit U, int D> struct UnitForms {
    static constexpr FormList list = unit_forms(U, D);
    template <int... I> static Forms<list.v[I]...> pick(std::integer_sequence<int, I...>);
    using type = decltype(pick(std::make_integer_sequence<int, list.n>{}));
};

}  // namespace sage
