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

// Which tiles get a mask at all.  A tile's mask is used only if a tile processed after it raises
// the clamp.  The tiles are processed in descending scout energy e, so the loudest tile still to
// come is the next one: the tile at position k gets a mask only if tile k + 1 is "near" the
// loudest by the scout (e >= ratio e_max; NaN already mapped to 0), that is if k + 1 < K with K
// the number of near tiles.  The last tile never needs one (theta equals its clamp).  A zero or
// all-equal scout makes every tile near: all but the last are masked.  Only a cost heuristic: a
// tile left without a mask is stored and recorded like a tile without clamped entries -- the
// record of a pass that holds one is the clamp itself -- so a later rise flags exactly those
// passes (shift_flags) and they are recomputed and swapped as plain columns, which never joined
// A, B, C.
#ifndef EWK_MASK_NEAR_RATIO
#define EWK_MASK_NEAR_RATIO 0.1f   // 10^(-X / 10), X = 10 dB (profiles/r08_v1_scout_sim_mask_rule.txt)
#endif
EWK_SHIFT_HD bool mask_near(float e, float e_max, float ratio = EWK_MASK_NEAR_RATIO) { return e >= ratio * e_max; }
EWK_SHIFT_HD bool mask_wanted(int k, int near_tiles) { return k + 1 < near_tiles; }

// A recomputed column: out goes the stored one as the rises have moved it (co + delta m,
// delta = theta - its own clamp), in comes cn (the column clamped at theta).
EWK_SHIFT_HD void shift_replace(double cn, double co, double m, double delta, double cref, double& s1, double& s2) {
    const double dn = cn - cref, dd = (co - cref) + delta * m;
    s1 += dn - dd;
    s2 += dn * dn - dd * dd;
}

}  // namespace ewk
