// sage_attn_parts.h -- interface between the host-side dispatch of the attention launches (sage_attn.hip) and the instantiation units
// sage_attn_d{128,64}_{f8,f8f,f16}.hip, each of which compiles the kernel family of sage_attn_kernel.h for one head size, one PV format and
// (FP8) one score form, sage_attn_d{128,64}_f8v.hip (the packed FP8 route's fused-Q kernels) and sage_attn_d{128,64}_f8s.hip (the exact
// split's seeded kernels) and sage_attn_d{128,64}_f8k.hip (the kv_lens route's kernels) and sage_attn_d{128,64}_f8q.hip (the same with a query offset per sample) and sage_attn_d{128,64}_f8w.hip (the same with a sliding window) and sage_attn_d{128,64}_f8g.hip (that family for decode-shaped calls, a GQA group's query heads four to a workgroup) and sage_attn_d{128,64}_f8ks.hip (that family's exact split: its kernels over one key-range chunk each, seeded).  The split exists for build time only: the units are independent and compile in parallel.
#pragma once
#include "sage_kernels.h"

namespace sage {

// D in {64, 128}; PV_FP8; SFOLD: the FP8 score form (true = folded bias, false = exact subtraction; FP16 PV has one form: true)
template <int D, bool PV_FP8, bool SFOLD>
hipError_t launch_attn_part(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);

extern template hipError_t launch_attn_part<128, true, true>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_part<128, true, false>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_part<128, false, true>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_part<64, true, true>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_part<64, true, false>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_part<64, false, true>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// FP8 PV over a packed batch, per-block Q quantised in the prologue (qf 3 / 4), exact score form: units sage_attn_d{128,64}_f8v.hip
template <int D>
hipError_t launch_attn_f8_varlen(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_varlen<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_varlen<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// the exact split's pass 2: the fused per-thread Q FP8 kernels with a seeded running maximum and FP32 partials: units sage_attn_d{128,64}_f8s.hip
template <int D>
hipError_t launch_attn_f8_seeded(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_seeded<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_seeded<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// per-sample key lengths (AttnParams::cu_k = the [B] lengths): the fused per-thread Q FP8 kernels, dense: units sage_attn_d{128,64}_f8k.hip
template <int D>
hipError_t launch_attn_f8_kvlens(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_kvlens<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_kvlens<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// per-sample query offsets on top of the key lengths (AttnParams::cu_qs = the [B] offsets; causal): units sage_attn_d{128,64}_f8q.hip
template <int D>
hipError_t launch_attn_f8_qstart(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_qstart<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_qstart<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// a sliding window on top of the offsets (AttnParams::window keys per row; AttnParams::cu_qs nullable): units sage_attn_d{128,64}_f8w.hip
template <int D>
hipError_t launch_attn_f8_window(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_window<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_window<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// the packed FP8-PV route with bottom-right causal alignment (offset Lk - Lq per sequence, from cu_seqlens): units sage_attn_d{128,64}_f8vb.hip
template <int D>
hipError_t launch_attn_f8_varlen_br(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_varlen_br<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_varlen_br<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// ... and with a sliding window (SageLaunchAttr.window together with the flag): units sage_attn_d{128,64}_f8vbw.hip
template <int D>
hipError_t launch_attn_f8_varlen_br_window(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_varlen_br_window<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_varlen_br_window<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// decode-shaped calls with a GQA group's query heads packed four to a workgroup (AttnVariant::gqa_pack; the kv_lens family): units sage_attn_d{128,64}_f8g.hip
template <int D>
hipError_t launch_attn_f8_gpack(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_gpack<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_gpack<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

// pass 2 of the kv_lens family's exact split (AttnVariant::seeded with kv_lens; unpacked or gqa_pack): units sage_attn_d{128,64}_f8ks.hip
template <int D>
hipError_t launch_attn_f8_kvsplit(const AttnParams &p, const AttnVariant &v, int nwork, const AttnLaunchOpts &l);
extern template hipError_t launch_attn_f8_kvsplit<128>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);
extern template hipError_t launch_attn_f8_kvsplit<64>(const AttnParams &, const AttnVariant &, int, const AttnLaunchOpts &);

}  // namespace sage
