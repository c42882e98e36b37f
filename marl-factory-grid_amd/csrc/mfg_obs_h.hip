// mfg_obs_h.hip — the folded-geometry dense render of pomdp_r 1, 2, 3 (mfg_obs_g.hip) with one-word cell and layer
// records (k_obs / k_obs_list <2R + 2, OT, MM, 0, DIRT, R, true>, see build_obs, NARROW, in mfg_kernels.h): the render
// of specs with at most 16 agents. -DMFG_OBS_NARROW=0 (given to this unit and to mfg_engine) compiles none of them.
#define MFG_OBS_UNIT
#include "mfg_kernels.h"

#if MFG_OBS_NARROW
MFG_DEFINE_LAUNCH_OBS_GEO
MFG_INSTANTIATE_OBS_GEO(1, true)
MFG_INSTANTIATE_OBS_GEO(2, true)
MFG_INSTANTIATE_OBS_GEO(3, true)
#endif
