// The start of an IMU-only run (only_imu_use: true) from message bytes, the way RosInterface + KILO::process start one: the first cloud is
// decoded, the serialized sensor_msgs/Imu messages become lk_imu records, the IMU branch of syncPackage hands them to the scans, the first
// package starts the run (state initialisation + first-frame map), and the second scan is replayed against that map - clouds and records
// staying in HBM.  Needs a gfx950 device to RUN (exit code 3 otherwise); tests/test_imu_frontend.py only checks that it compiles and links.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "legkilo_host.hpp"

using namespace legkilo;

// a floor 1 m below the sensor and a wall 6 m ahead, 0.1 s sweep, Velodyne layout (x y z intensity time ring: 22 bytes)
static std::vector<unsigned char> cloud_message(uint32_t n) {
    std::vector<unsigned char> msg;
    for (uint32_t i = 0; i < n; ++i) {
        unsigned char pt[22] = {0};
        const float u = (float)(i % 100) * 0.08f - 4.0f, v = (float)(i / 100) * 0.08f;
        const bool floor = (i & 1) == 0;
        const float xyz[3] = {floor ? 2.0f + v : 6.0f, u, floor ? -1.0f : -1.0f + 0.5f * v}, t = 0.1f * (float)i / (float)n;
        std::memcpy(pt, xyz, 12), std::memcpy(pt + 16, &t, 4);
        msg.insert(msg.end(), pt, pt + 22);
    }
    return msg;
}

int main() {
    ESKF::Config ec{20, 500, 1000, 20, 0.001, 0.001, 0.001, 0.1, 1.0, 0.01, 0.1, 0.1, 0.001, 10};
    VoxelMapConfig vc;
    DeviceCaps caps;
    caps.max_roots = 1u << 12, caps.max_nodes = 1u << 13, caps.max_point_blocks = 1u << 12, caps.max_scan_points = 1u << 14;
    std::unique_ptr<KiloPath> kilo;
    try {
        kilo = std::make_unique<KiloPath>(ec, vc, Mat3D::Identity(), Vec3D{0, 0, 0}, 9.81, caps);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "no device: %s\n", e.what());
        return 3;
    }
    Device& dev = kilo->device();
    auto to_device = [&](const void* src, size_t bytes) {
        void* d = nullptr;
        dev.check(lk_device_malloc(dev.h(), &d, bytes));
        dev.check(lk_memcpy_h2d(dev.h(), d, src, bytes));
        return d;
    };

    // two clouds stamped 10.0 and 10.1 s
    const uint32_t n_pts = 6000;
    const std::vector<unsigned char> cloud = cloud_message(n_pts);
    lk_cloud_layout layout{22, 0, 4, 8, 16, 1};
    void* d_cloud = to_device(cloud.data(), cloud.size());
    void *d_raw = nullptr, *d_scan = nullptr;
    dev.check(lk_device_malloc(dev.h(), &d_raw, sizeof(lk_point) * n_pts));
    dev.check(lk_device_malloc(dev.h(), &d_scan, sizeof(lk_point) * n_pts));
    size_t n_raw = 0;
    double begin0 = 0, end0 = 0;
    dev.check(lk_decode_scan_dev(dev.h(), d_cloud, n_pts, &layout, 1.0, 3, 1.5f, 10.0, static_cast<lk_point*>(d_raw), &n_raw, &begin0, &end0));
    const uint64_t cloud_off[1] = {0};
    const double stamp1[1] = {10.1};
    uint64_t scan_off[2] = {0, 0};
    double begin1 = 0, end1 = 0;
    dev.check(lk_decode_scans_dev(dev.h(), d_cloud, 1, cloud_off, &n_pts, stamp1, &layout, 1.0, 3, 1.5f, 0.3f, static_cast<lk_point*>(d_scan), scan_off,
                                  &begin1, &end1));

    // 200 Hz Imu messages from 10.0 to 10.25 s, the sensor at rest; the frame_id changes length, so no field is aligned
    std::vector<unsigned char> bag;
    std::vector<uint64_t> msg_off;
    for (uint32_t i = 0; i < 50; ++i) {
        const char* frame = (i % 3 == 0) ? "imu" : (i % 3 == 1) ? "imu_link" : "base/imu_frame";
        const uint32_t L = (uint32_t)std::strlen(frame), head[4] = {i, 10u, 5000000u * i + 2500000u, L};
        const double gyr[3] = {0.001, -0.002, 0.0005 + 1e-6 * i}, acc[3] = {0.02, -0.01, 9.81 + 1e-4 * i};
        msg_off.push_back(bag.size());
        std::vector<unsigned char> m(LK_IMU_MSG_FIXED_BYTES + L, 0);
        std::memcpy(&m[0], head, 16), std::memcpy(&m[16], frame, L);
        std::memcpy(&m[120 + L], gyr, 24), std::memcpy(&m[216 + L], acc, 24);
        bag.insert(bag.end(), m.begin(), m.end());
    }
    msg_off.push_back(bag.size());
    void* d_bag = to_device(bag.data(), bag.size());
    void* d_imus = nullptr;
    dev.check(lk_device_malloc(dev.h(), &d_imus, sizeof(lk_imu) * 50));
    ImuFrontend imu(true, kilo->device_ptr());
    const size_t kept = imu.processingDev(d_bag, msg_off, static_cast<lk_imu*>(d_imus));
    std::vector<uint32_t> n_msg;
    size_t consumed = 0;
    const size_t packaged = imu.syncPackages(static_cast<const lk_imu*>(d_imus), kept, {end0, end1}, n_msg, &consumed);
    std::printf("%zu of 50 Imu messages kept, %zu scans packaged with %u + %u records\n", kept, packaged, n_msg[0], n_msg[1]);

    // package 0 starts the run; package 1 is replayed from the state the first frame left
    kilo->firstFrameDev(static_cast<const lk_point*>(d_raw), n_raw, end0, 1, d_imus, n_msg[0]);
    const Vec3D g = kilo->eskf().state().grav_;
    std::printf("first frame: acc_norm %.4f, grav (%.4f %.4f %.4f)\n", kilo->accNorm(), g[0], g[1], g[2]);
    const std::vector<lk_pose> poses = kilo->replayRecordedRunImuDev(static_cast<const lk_point*>(d_scan), {scan_off[0], scan_off[1]}, {begin1}, {n_msg[1]},
                                                                     static_cast<const lk_imu*>(d_imus) + n_msg[0]);
    std::printf("scan 1: %u buckets, %llu matched points, pos (%.4f %.4f %.4f)\n", poses[0].n_buckets, (unsigned long long)poses[0].n_effect, poses[0].pos[0],
                poses[0].pos[1], poses[0].pos[2]);
    for (void* d : {d_cloud, d_raw, d_scan, d_bag, d_imus}) lk_device_free(dev.h(), d);
    return 0;
}
