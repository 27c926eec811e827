// ewk_topdb_shift.h -- the top_db shift rule of the float32 scorer (ewk_mfcc.hip), as plain
// host/device formulas (tests/test_topdb_shift_model.py compiles them on the host).
//
// A tile stored clamped at its speculative clamp r holds two kinds of entries: the clamped
// ones, all equal to r, and the unclamped ones, all above r.  When the clamp rises to r' and no
// unclamped entry lies in (r, r'), only the clamped entries move, all by delta = r' - r.  The
// DCT is linear, so with m = D . mask (mask: the 0/1 vector of a frame's clamped bands) the
// frame's coefficients move by delta m and nothing has to be recomputed.  Per coefficient the
// shifted sums s1 = sum d, s2 = sum d^2 (d = c - cref) of the frames seen so far follow from
// three more sums over those frames:
//     A = sum m,  B = sum d m,  C = sum m^2
//     s1 += delta A,  s2 += 2 delta B + delta^2 C,  B += delta C        (shift_rise)
// after which every earlier clamped entry sits at r'.  A tile that does hold an unclamped entry
// below the final threshold (its minimum above the clamp < theta: shift_flags) is recomputed,
// and the columns taken out of the sums are its stored ones as shifted so far (shift_replace).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define EWK_SHIFT_HD __host__ __device__ inline
#else
#define EWK_SHIFT_HD inline
#endif

namespace ewk {

// One frame column joins the sums: d = c - cref at the column's clamp, m its mask DCT.
template <typename TA, typename TB>
EWK_SHIFT_HD void shift_add(TA d, TA m, TA& A, TB& B, TA& C) {
    A += m;
    B += (TB)(d * m);
    C += m * m;
}

// The clamp of every column in (A, B, C) rises by delta.
template <typename TA, typename TB>
EWK_SHIFT_HD void shift_rise(double delta, TA A, TB& B, TA C, double& s1, double& s2) {
    s1 += delta * (double)A;
    s2 += delta * (2.0 * (double)B + delta * (double)C);
    B = (TB)((double)B + delta * (double)C);
}

// A tile may stay shifted only while no unclamped stored value lies below the threshold.
template <typename T>
EWK_SHIFT_HD bool shift_flags(T min_above_clamp, T theta) { return min_above_clamp < theta; }

// A recomputed column: out goes the stored one as the rises have moved it (co + delta m,
// delta = theta - its own clamp), in comes cn (the column clamped at theta).
EWK_SHIFT_HD void shift_replace(double cn, double co, double m, double delta, double cref, double& s1, double& s2) {
    const double dn = cn - cref, dd = (co - cref) + delta * m;
    s1 += dn - dd;
    s2 += dn * dn - dd * dd;
}

}  // namespace ewk
