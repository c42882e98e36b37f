// mfg_obs_g.hip — the single-wave dense render with the window geometry of pomdp_r 1, 2, 3 folded at compile time
// (k_obs / k_obs_list <2R + 2, OT, MM, 0, DIRT, R>, see build_obs and ObsGeo in mfg_kernels.h), three-word cell and
// layer records (specs with more than 16 agents, mfg_variant.obs_wide_records); mfg_obs_h.hip: the one-word records.
#define MFG_OBS_UNIT
#include "mfg_kernels.h"

MFG_DEFINE_LAUNCH_OBS_GEO
MFG_INSTANTIATE_OBS_GEO(1, false)
MFG_INSTANTIATE_OBS_GEO(2, false)
MFG_INSTANTIATE_OBS_GEO(3, false)
