// l2c_slots.h -- the TWO-LEVEL slot order of the one-product operands (pack.hip writes it, l2c_topk.hip's one-step loop relies
// on it, local_seeds.hip reads components and the norm slot through it), as functions the host and the device share:
// tests/test_two_level_cpu.py compiles this header for the host.
//
// The plain order is [hi_0 .. hi_{g-1} | nh | nl | ey] (pack.hip).  The two-level order puts everything the score needs
// apart from the last g - 28 components into the FIRST step of 32 slots, with a bound on what those components can
// contribute in their place:
//   step 0 (slots 0..31):   hi_0 .. hi_27 | tail | nh | nl | ey
//   step 1 (slots 32..63):  hi_28 .. hi_{g-1} | tail' | 0 ..
// references: tail = tail' = ty,  ty  = f16 >= ||hi_y[28..g)||;   targets: tail = -2 tx2, tail' = +2 tx2,
// tx2 = f16 >= ||hi_x[28..g)|| (both rounded like ey / tx: a factor 1 + 2^-9 before rounding to nearest, never below 2^-13).
// After step 0 the accumulator holds   ||rep_y||^2 - 2 hi_x[0..28).hi_y[0..28) - 2 tx2 ty - tx ey,   by Cauchy-Schwarz a lower
// bound of the full one-product score; step 1 adds  -2 hi_x[28..g).hi_y[28..g) + 2 tx2 ty  and the two tail products (each
// an exact f16 x f16 product) cancel: the full score.  Needs 28 < g and g + 5 <= 64.
#pragma once

#if defined(__HIPCC__)
#define NABO_SLOT_HD __host__ __device__
#else
#define NABO_SLOT_HD
#endif

namespace nabo {

constexpr int L2C_HEAD = 28;                 // components of step 0
constexpr int L2C_SLOT_TAIL = 28, L2C_SLOT_NH = 29, L2C_SLOT_NL = 30, L2C_SLOT_EY = 31;
// what a slot holds (l2c_slot_holds): a component index >= 0, or one of these
constexpr int L2C_IS_TAIL = -1, L2C_IS_NH = -2, L2C_IS_NL = -3, L2C_IS_EY = -4, L2C_IS_TAIL2 = -5, L2C_IS_ZERO = -6;

NABO_SLOT_HD inline bool l2c_slots_fit(int g) { return g > L2C_HEAD && g + 5 <= 64; }
NABO_SLOT_HD inline int l2c_slot_of_comp(int e) { return e < L2C_HEAD ? e : 32 + (e - L2C_HEAD); }
NABO_SLOT_HD inline int l2c_slot_tail2(int g) { return 32 + (g - L2C_HEAD); }

NABO_SLOT_HD inline int l2c_slot_holds(int g, int p)
{
    if (p < L2C_HEAD) return p;
    if (p < 32) return p == L2C_SLOT_TAIL ? L2C_IS_TAIL : p == L2C_SLOT_NH ? L2C_IS_NH : p == L2C_SLOT_NL ? L2C_IS_NL : L2C_IS_EY;
    const int e = L2C_HEAD + (p - 32);
    return e < g ? e : e == g ? L2C_IS_TAIL2 : L2C_IS_ZERO;
}

// Slot of the high norm word / what slot p holds, in either order (two_level = false: the plain order of g + 3 slots)
NABO_SLOT_HD inline int l2c_norm_slot(int g, bool two_level) { return two_level ? L2C_SLOT_NH : g; }
NABO_SLOT_HD inline bool l2c_slot_is_comp(int g, int p, bool two_level) { return two_level ? l2c_slot_holds(g, p) >= 0 : p < g; }

// An upper bound of a norm that survives the rounding to f16: what ey, tx, ty and tx2 all go through (as a float; the
// caller converts it to f16, round to nearest).  2^-13: f16 subnormals round with an absolute error.
NABO_SLOT_HD inline float l2c_round_up(double v) { const float f = (float)(v * 1.001953125); return f > 1.220703125e-4f ? f : 1.220703125e-4f; }

}  // namespace nabo
