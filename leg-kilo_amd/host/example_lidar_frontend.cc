// Minimal use of the LidarProcessing mirror: the PointCloud2 payloads of a recorded run (here three small synthetic Velodyne-layout
// messages) go to HBM once and come back as decoded, voxel-grid filtered, time-sorted scans - still in HBM - with their offsets and
// begin / end times.  Needs a gfx950 device to RUN (exit code 3 otherwise); tests/test_lidar_frontend.py only checks that it compiles and links.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "legkilo_host.hpp"

using namespace legkilo;

int main() {
    lk_config cfg{};
    cfg.max_voxel_size = 0.5, cfg.max_layer = 2, cfg.max_points_num = 50, cfg.gravity = 9.81;
    for (int i = 0; i < 5; ++i) cfg.layer_init_num[i] = 5;
    cfg.ext_R[0] = cfg.ext_R[4] = cfg.ext_R[8] = 1.0;
    cfg.n_slots = 1, cfg.max_roots = 1u << 12, cfg.max_nodes = 1u << 13, cfg.max_point_blocks = 1u << 12, cfg.max_scan_points = 1u << 12;
    std::shared_ptr<Device> dev;
    try {
        dev = std::make_shared<Device>(cfg);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "no device: %s\n", e.what());
        return 3;
    }
    LidarProcessing::Config lc;
    lc.blind_ = 1.5f, lc.filter_num_ = 3, lc.lidar_type_ = 1, lc.time_scale_ = 1.0;
    lc.layout.point_step = 22, lc.layout.off_x = 0, lc.layout.off_y = 4, lc.layout.off_z = 8, lc.layout.off_time = 16;   // x y z intensity time ring
    LidarProcessing lidar(lc, dev);
    // three messages of 3 000 / 2 000 / 2 500 points on a 10 m circle, 0.1 s sweeps, 10 Hz stamps, laid back to back
    const uint32_t sizes[3] = {3000, 2000, 2500};
    std::vector<unsigned char> bag;
    std::vector<uint64_t> msg_off;
    std::vector<uint32_t> n_points;
    std::vector<double> stamps;
    for (int s = 0; s < 3; ++s) {
        msg_off.push_back(bag.size());
        n_points.push_back(sizes[s]);
        stamps.push_back(100.0 + 0.1 * s);
        for (uint32_t i = 0; i < sizes[s]; ++i) {
            unsigned char pt[22] = {0};
            const float a = 6.2831853f * (float)i / (float)sizes[s];
            const float xyz[3] = {10.0f * std::cos(a), 10.0f * std::sin(a), 0.1f * (float)(i % 16)}, t = 0.1f * (float)i / (float)sizes[s];
            std::memcpy(pt, xyz, 12), std::memcpy(pt + 16, &t, 4);
            bag.insert(bag.end(), pt, pt + 22);
        }
    }
    void* d_bag = nullptr;
    dev->check(lk_device_malloc(dev->h(), &d_bag, bag.size()));
    dev->check(lk_memcpy_h2d(dev->h(), d_bag, bag.data(), bag.size()));
    {
        LidarProcessing::DeviceScans scans = lidar.processRun(d_bag, msg_off, n_points, stamps, 0.3f);
        for (size_t s = 0; s < scans.size(); ++s)
            std::printf("scan %zu: %llu points, %.3f .. %.3f s\n", s, (unsigned long long)(scans.scan_off[s + 1] - scans.scan_off[s]), scans.t_begin[s],
                        scans.t_end[s]);
    }
    lk_device_free(dev->h(), d_bag);
    return 0;
}
