// The two-level slot order of the one-product operands (nabo_amd/csrc/l2c_slots.h) compiled for the host: what pack.hip,
// l2c_topk.hip and local_seeds.hip share, callable from tests/test_two_level_cpu.py.
#include "l2c_slots.h"

using namespace nabo;

extern "C" int l2c_slots_fit_host(int g) { return l2c_slots_fit(g) ? 1 : 0; }
extern "C" int l2c_slot_of_comp_host(int e) { return l2c_slot_of_comp(e); }
extern "C" int l2c_slot_tail2_host(int g) { return l2c_slot_tail2(g); }
extern "C" int l2c_slot_holds_host(int g, int p) { return l2c_slot_holds(g, p); }
extern "C" int l2c_norm_slot_host(int g, int two_level) { return l2c_norm_slot(g, two_level != 0); }
extern "C" int l2c_slot_is_comp_host(int g, int p, int two_level) { return l2c_slot_is_comp(g, p, two_level != 0) ? 1 : 0; }
extern "C" float l2c_round_up_host(double v) { return l2c_round_up(v); }
