#!/bin/bash
# Variant libraries for A/B timing (tools/ab_run.sh): build/ablate/libmfg_hip_NAME.so from "NAME=FLAGS" arguments, e.g.
#   tools/build_variant.sh RPV7=-DMFG_RPV=7 OVL0=-DMFG_RESET_OVERLAP=0
# usage: [UNITS="mfg_engine"] tools/build_variant.sh NAME=FLAGS ...
# Every unit is compiled with FLAGS unless UNITS names the ones that are (__graft_entry__.build_hip holds the unit list
# and does the work); the other units link from build/obj, refreshed with the default flags first. So
#   UNITS=mfg_engine  a variant of the host unit only (k_logic, k_replay*, resets) reuses the render objects;
#   UNITS=mfg_obs_a   a render variant: mfg_obs_a holds ray lengths 4-8 (C2/C3), mfg_obs_b C4's 10-point rays,
#                     mfg_obs_c C5's 18; mfg_obs_g the dense renders with pomdp_r 1-3's window geometry folded
#                     (-DMFG_OBS_GEO_ALIGN=0, -DMFG_OBS_GEO_LANE_OPAQUE=0, -DMFG_OBS_GEO_WPE=8), mfg_obs_h the same with
#                     one-word records (C2/C3 dense obs run these; wider specs run mfg_obs_g's).
#   UNITS="mfg_engine mfg_obs_h" with -DMFG_OBS_NARROW=0: C2/C3 back on mfg_obs_g's three-word records.
# One variant at a time: each build is already one compile per unit in parallel.
set -e
cd "$(dirname "$0")/.."
for arg in "$@"; do
  python3 -c 'import sys, __graft_entry__ as g
name, flags = sys.argv[1].split("=", 1)
print(g.build_hip(out=f"build/ablate/libmfg_hip_{name}.so", extra=flags.split(), units=sys.argv[2].split() or None))' \
    "$arg" "$UNITS"
done
