// lk_ovrun.hip - the run-resident kernel of lk_batch_replay_overlay_runs_dev: lk_ovscan.hip's kernel template instantiated with RUN (and ov_run_launch, which
// launches it), a translation unit of its own for the build time - two more instantiations of a kernel that takes as long to compile as the overlay unit.
#define LK_OVSCAN_RUNS 1
#include "lk_ovscan.hip"
