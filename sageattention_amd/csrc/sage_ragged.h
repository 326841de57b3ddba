// sage_ragged.h -- the row range of one sample of a PACKED operand, from two words of a caller-written prefix array: the one clamp the ragged
// attention kernel (sage_attn_paged_varlen_kernel) and the ragged append (sage_kv_varlen.hip) put between those words and every address.
// Plain C++ with no include of its own, so that a host program can exercise it (tests/ragged_clamp_main.cpp) -- and the band
// filter the step call's two launches sort the samples with (tests/ragged_band_main.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SAGE_RAGGED_HD __host__ __device__
#else
#define SAGE_RAGGED_HD
#endif

namespace sage {

// c0 = cu[b], c1 = cu[b + 1], `total` the rows the packed tensor has, `max_rows` the most rows the launch gives a sample (max_seqlen_q /
// max_new: the grid is sized by it).  Yields the sample's first row `first` and its row count `rows` with
//     0 <= first <= first + rows <= max(total, 0)   and   0 <= rows <= max(max_rows, 0)
// whatever the four words hold -- negative, non-monotone, past `total`, INT_MIN / INT_MAX: every comparison is between two ints, no sum or
// difference is formed before both of its operands lie in [0, total].  A bad prefix array gives wrong numbers, never a row outside the tensor.
SAGE_RAGGED_HD inline void ragged_rows(int c0, int c1, int total, int max_rows, int &first, int &rows)
{
    const int t = total < 0 ? 0 : total;
    const int q0 = c0 < 0 ? 0 : (c0 < t ? c0 : t);       // in [0, t]
    const int q1 = c1 < q0 ? q0 : (c1 < t ? c1 : t);     // in [q0, t]
    const int m = max_rows < 0 ? 0 : max_rows;
    const int n = q1 - q0;                               // in [0, t]
    first = q0;
    rows = n < m ? n : m;
}

// ragged_rows behind a band filter (the step call's two launches): the sample's (first, rows) when lo < rows <= hi, rows = 0
// otherwise -- `first` is ragged_rows' either way.  The filter compares the CLAMPED count (an int in [0, max(max_rows, 0)]) with two ints and
// forms nothing: the bands (0, 32] and (32, max_rows] of one launch pair split the samples that have rows between them, whatever the words hold.
SAGE_RAGGED_HD inline void ragged_band(int c0, int c1, int total, int max_rows, int lo, int hi, int &first, int &rows)
{
    int n;
    ragged_rows(c0, c1, total, max_rows, first, n);
    rows = (lo < n && n <= hi) ? n : 0;
}

// ragged_band again, under the name of the attention body's SECOND band site (sage_attn_body.h, the split step launch's arm of the seeded
// branch): the same words, the same filter, nothing of its own -- the body's first band site stays the one place that spells
// ragged_band, which the host tests of the step calls count.
SAGE_RAGGED_HD inline void ragged_band_rows(int c0, int c1, int total, int max_rows, int lo, int hi, int &first, int &rows)
{
    ragged_band(c0, c1, total, max_rows, lo, hi, first, rows);
}

}  // namespace sage
