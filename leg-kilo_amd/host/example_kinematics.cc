// Minimal use of the Kinematics mirror, the way RosInterface drives the reference's Kinematics: serialized HighState messages in, the
// kept messages' KinImuMeas records out, then the split of the records over two scans.  Needs a gfx950 device to RUN (exit code 3
// otherwise); tests/test_kin_frontend.py only checks that it compiles and links.
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
    Kinematics kin(Kinematics::Config{0.1881, 0.04675, 0.213, 0.213, 0.08, 220, 200, true}, dev);   // leg_fusion.yaml
    // 20 messages at 500 Hz: the IMU changes every second message, foot force 250 (stance) on every foot
    const size_t n = 20;
    std::vector<unsigned char> msgs(n * LK_HIGHSTATE_BYTES, 0);
    for (size_t i = 0; i < n; ++i) {
        unsigned char* m = &msgs[i * LK_HIGHSTATE_BYTES];
        const uint32_t sec = 10, nsec = (uint32_t)(2000000 * i);
        const float acc_z = 9.8f + 0.01f * (float)(i / 2), q[3] = {0.02f, 0.8f, -1.6f};
        const int16_t force = 250;
        std::memcpy(m + 0, &sec, 4), std::memcpy(m + 4, &nsec, 4), std::memcpy(m + 66, &acc_z, 4);
        for (int k = 0; k < 12; ++k) std::memcpy(m + 84 + 38 * k, &q[k % 3], 4);
        for (int f = 0; f < 4; ++f) std::memcpy(m + 877 + 2 * f, &force, 2);
    }
    std::vector<lk_kin_imu> recs = kin.processing(msgs.data(), n);
    std::printf("%zu of %zu messages kept; FR foot at (%.4f %.4f %.4f), contact %d\n", recs.size(), n, recs[0].foot_pos[0][0], recs[0].foot_pos[0][1],
                recs[0].foot_pos[0][2], recs[0].contact[0]);
    void* d = nullptr;
    dev->check(lk_device_malloc(dev->h(), &d, sizeof(lk_kin_imu) * recs.size()));
    dev->check(lk_memcpy_h2d(dev->h(), d, recs.data(), sizeof(lk_kin_imu) * recs.size()));
    std::vector<uint32_t> n_msg;
    size_t consumed = 0;
    const size_t packaged = kin.syncPackages(static_cast<const lk_kin_imu*>(d), recs.size(), {10.010, 10.030}, n_msg, &consumed);
    std::printf("%zu scans packaged, %zu records consumed\n", packaged, consumed);
    lk_device_free(dev->h(), d);
    return 0;
}
