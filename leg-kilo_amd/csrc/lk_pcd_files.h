// lk_pcd_files.h - which registered points go into which map file: the counting of PcdSaver::workerLoop (common/pcd_saver.hpp:91-112) over the tables of
// the run replays.  A run is one mapping session: its frames (scans) are appended in order, a file is cut after every frames_per_file frames and once
// more at the run's end for the remainder; a frame without points is skipped and not counted (pcd_saver.hpp:101); frames_per_file <= 0 means 100
// (pcd_saver.hpp:32).  The frames of a run are contiguous in d_world_out, so a file is one range of records - what lk_downsample_clouds_dev takes.
// Plain C++ without HIP: legkilo_host.hpp uses it, tests/pcd_files_main.cc runs it under the host sanitizers on its own.
#pragma once
#include <cstddef>
#include <cstdint>

// run r = the scans run_off[r] .. run_off[r+1), scan s = the records scan_off[s] .. scan_off[s+1).  Writes file_off[0 .. n_files] (file f = the records
// file_off[f] .. file_off[f+1); file_off[0] = the first scan's first record) and file_run[0 .. n_files) (the run a file belongs to) and returns n_files.
// Either array may be null (a null file_off: the call only counts); n_files is at most the number of scans, so run_off[n_runs] + 1 and run_off[n_runs]
// entries are always enough.
static inline size_t pcd_file_offsets(const uint32_t* run_off, size_t n_runs, const uint64_t* scan_off, int frames_per_file, uint64_t* file_off,
                                      uint32_t* file_run) {
    if (frames_per_file <= 0) frames_per_file = 100;
    size_t n_files = 0;
    if (file_off && n_runs) file_off[0] = scan_off[run_off[0]];
    for (size_t r = 0; r < n_runs; ++r) {
        int frames_in_buffer = 0;
        for (uint32_t s = run_off[r]; s < run_off[r + 1]; ++s) {
            if (scan_off[s + 1] == scan_off[s]) continue;   // an empty cloud is never queued
            if (++frames_in_buffer >= frames_per_file) {
                if (file_off) file_off[n_files + 1] = scan_off[s + 1];
                if (file_run) file_run[n_files] = (uint32_t)r;
                ++n_files, frames_in_buffer = 0;
            }
        }
        if (frames_in_buffer) {   // the remainder, written when the session ends
            if (file_off) file_off[n_files + 1] = scan_off[run_off[r + 1]];
            if (file_run) file_run[n_files] = (uint32_t)r;
            ++n_files;
        }
    }
    return n_files;   // (empty frames between two files hold no records: a file starts where the one before it ends)
}
