// lgh_switches.hip — the environment switches (lgh_common.hpp Switches): the parsers and read_switches, the one place of the
// library that asks the environment (but for the two properties of the shared-memory transport, lgh_comm_transport.hip).
#include <cstdlib>

#include "lgh_common.hpp"

namespace lgh
{

// a flag: '0...' is 0, '1...' is 1, anything else (and no variable) is `unset`
static int env_flag(const char *name, const int unset)
{
   const char *e = getenv(name);
   return (e && (e[0] == '0' || e[0] == '1')) ? e[0] - '0' : unset;
}
// a number; a variable that does not start with one counts as not set
static long env_long(const char *name, const long unset)
{
   const char *e = getenv(name);
   char *end = nullptr;
   const long v = e ? strtol(e, &end, 10) : 0;
   return (e && end != e) ? v : unset;
}
static double env_double(const char *name, const double unset)
{
   const char *e = getenv(name);
   char *end = nullptr;
   const double v = e ? strtod(e, &end) : 0.0;
   return (e && end != e) ? v : unset;
}
static std::string env_string(const char *name)
{
   const char *e = getenv(name);
   return e ? e : "";
}
// the variable exists, whatever it holds
static bool env_present(const char *name) { return getenv(name) != nullptr; }

Switches read_switches()
{
   Switches s;
   s.vcg_variant = (int)env_long("LGH_VCG_VARIANT", -1);
   s.slab_wide = env_flag("LGH_SLAB_WIDE", 1);
   s.slab_exact = env_flag("LGH_SLAB_EXACT", 1);
   s.slab_merge = env_flag("LGH_SLAB_MERGE", 1);
   s.slab_defer = env_flag("LGH_SLAB_DEFER", 1);
   s.slab_ye_wide = env_flag("LGH_SLAB_YE_WIDE", 0);
   s.slab_dyn = env_flag("LGH_SLAB_DYN", -1);
   s.rz_limbs = env_flag("LGH_RZ_LIMBS", 1);
   s.kron_neb = env_flag("LGH_KRON_NEB", 1);
   s.fused_init = env_flag("LGH_FUSED_INIT", 1);
   s.k2p = env_flag("LGH_K2P", 1);
   s.k2_skip = env_flag("LGH_K2_SKIP", 1);
   s.k2_grid = (int)env_long("LGH_K2_GRID", 0);
   s.k2_node_weight = env_long("LGH_K2_NODE_WEIGHT", 5);
   s.order = env_flag("LGH_ORDER", 1);
   s.order_multi = env_flag("LGH_ORDER_MULTI", 1);
   s.comm2 = env_flag("LGH_COMM2", -1);
   s.force_multi = env_flag("LGH_FORCE_MULTI", 0);
   s.halo_piggyback = env_flag("LGH_HALO_PIGGYBACK", 1);
   s.halo_fused_pack = env_flag("LGH_HALO_FUSED_PACK", 1);
   s.overlap = env_flag("LGH_OVERLAP", 1);
   s.energy_lockstep = env_flag("LGH_ENERGY_LOCKSTEP", 1);
   s.spin = env_flag("LGH_SPIN", 1);
   s.mass_sep = env_flag("LGH_MASS_SEP", 1);
   s.mass_kron = env_flag("LGH_MASS_KRON", 1);
   s.mass_rank1 = env_flag("LGH_MASS_RANK1", 1);
   s.mass_rank1_tol = env_double("LGH_MASS_RANK1_TOL", kMassRank1Tol);
   s.l2_neb = env_flag("LGH_L2_NEB", 1);
   s.l2_plane = env_flag("LGH_L2_PLANE", 1);
   s.l2_fused = env_flag("LGH_L2_FUSED", 1);
   s.q_form = env_flag("LGH_Q_FORM", 1);
   s.q_ppt = env_flag("LGH_Q_PPT", 0);
   s.q_swz = (int)env_long("LGH_Q_SWZ", -1);
   s.q_occ4 = env_flag("LGH_Q_OCC4", -1);
   s.q_discard = (int)env_long("LGH_Q_DISCARD", 1);
   s.q_tiny_grad = env_double("LGH_Q_TINY_GRAD", 1e-30); // 0: exact zeros only; -1: off
   s.fused_ftv = env_flag("LGH_FUSED_FTV", 1);
   s.fused_f1 = env_flag("LGH_FUSED_F1", 1);
   s.b_sym = env_flag("LGH_B_SYM", 1);
   s.jac0_compact = env_flag("LGH_JAC0_COMPACT", 1);
   // (a tolerance above 1e-10 would turn curved zones into affine ones: clamped - round-5 advisor)
   s.jac0_tol = std::min(std::max(env_double("LGH_JAC0_TOL", kJac0Tol), 0.0), 1e-10);
   s.profile_fold = (int)std::max(0L, env_long("LGH_PROFILE_FOLD", 8));
   s.map_fold = (int)std::min(std::max(0L, env_long("LGH_MAP_FOLD", 8)), 64L); // (a wavefront has 64 lanes: no more cells than that)
   s.roctx = env_flag("LGH_ROCTX", 0);
   s.vcg_trace = env_string("LGH_VCG_TRACE");
   s.vcg_trace_phases = env_present("LGH_VCG_TRACE_PHASES");
   s.q_trace = env_string("LGH_Q_TRACE");
   s.q_trace_call = (int)env_long("LGH_Q_TRACE_CALL", 40);
   return s;
}

} // namespace lgh
