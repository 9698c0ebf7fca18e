// A recorded IMU-only run (only_imu_use: true) LIVE from message bytes, the way RosInterface + KILO::process run one: the PointCloud2 payloads
// become decoded, voxel-filtered, time-sorted scans (lk_decode_scans_dev), the serialized sensor_msgs/Imu messages become lk_imu records
// (lk_decode_imu_dev) that the IMU branch of syncPackage hands to the scans (lk_imu_split_dev), the first package starts the run
// (lk_first_frame_dev: state initialisation + first-frame map), and every later scan is processed against the growing map in ONE call
// (lk_run_scans_dev) - clouds, records and the registered cloud staying in HBM.  Prints the trajectory as TUM lines (`stamp x y z qx qy qz qw`).
// Needs a gfx950 device to RUN (exit code 3 otherwise); tests/test_live_run.py only checks that it compiles and links.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "legkilo_host.hpp"

using namespace legkilo;

// a floor 1 m below the sensor and a wall 6 m ahead seen from x = dx, 0.1 s sweep, Velodyne layout (x y z intensity time ring: 22 bytes)
static void cloud_message(uint32_t n, float dx, std::vector<unsigned char>& bag) {
    for (uint32_t i = 0; i < n; ++i) {
        unsigned char pt[22] = {0};
        const float u = (float)(i % 100) * 0.08f - 4.0f, v = (float)(i / 100) * 0.08f;
        const bool floor = (i & 1) == 0;
        const float xyz[3] = {(floor ? 2.0f + v : 6.0f) - dx, u, floor ? -1.0f : -1.0f + 0.5f * v}, t = 0.1f * (float)i / (float)n;
        std::memcpy(pt, xyz, 12), std::memcpy(pt + 16, &t, 4);
        bag.insert(bag.end(), pt, pt + 22);
    }
}

// Eigen::Quaterniond(Matrix3d) (trajectory_saver.hpp:43-50 writes it as x y z w)
static void rot_to_quat(const double* R, double* q) {
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t, t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t, q[1] = (R[2] - R[6]) * t, q[2] = (R[3] - R[1]) * t;
        return;
    }
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[4 * i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    t = std::sqrt(R[4 * i] - R[4 * j] - R[4 * k] + 1.0);
    q[i] = 0.5 * t, t = 0.5 / t;
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t, q[j] = (R[3 * j + i] + R[3 * i + j]) * t, q[k] = (R[3 * k + i] + R[3 * i + k]) * t;
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
    auto device_room = [&](size_t bytes) {
        void* d = nullptr;
        dev.check(lk_device_malloc(dev.h(), &d, bytes));
        return d;
    };
    auto to_device = [&](const void* src, size_t bytes) {
        void* d = device_room(bytes);
        dev.check(lk_memcpy_h2d(dev.h(), d, src, bytes));
        return d;
    };

    // five clouds stamped 10.0 .. 10.4 s, the sensor creeping forward 1 cm per scan
    const uint32_t S = 5, n_pts = 6000;
    std::vector<unsigned char> clouds;
    std::vector<uint64_t> cloud_off;
    std::vector<uint32_t> cloud_n(S, n_pts);
    std::vector<double> stamp;
    for (uint32_t s = 0; s < S; ++s) {
        cloud_off.push_back(clouds.size());
        cloud_message(n_pts, 0.01f * (float)s, clouds);
        stamp.push_back(10.0 + 0.1 * s);
    }
    void* d_clouds = to_device(clouds.data(), clouds.size());
    LidarProcessing::Config lc;
    lc.blind_ = 1.5f, lc.filter_num_ = 3, lc.lidar_type_ = 1, lc.time_scale_ = 1.0, lc.layout = lk_cloud_layout{22, 0, 4, 8, 16, 1};
    LidarProcessing lidar(lc, kilo->device_ptr());
    const LidarProcessing::DeviceScans scans = lidar.processRun(d_clouds, cloud_off, cloud_n, stamp, 0.3f);
    // the first frame takes the RAW first cloud (KILO.cc:336-339), not the voxel-filtered one
    void* d_raw = device_room(sizeof(lk_point) * n_pts);
    size_t n_raw = 0;
    double begin0 = 0, end0 = 0;
    dev.check(lk_decode_scan_dev(dev.h(), d_clouds, n_pts, &lc.layout, 1.0, 3, 1.5f, stamp[0], static_cast<lk_point*>(d_raw), &n_raw, &begin0, &end0));

    // 200 Hz Imu messages from 10.0 to 10.55 s, the sensor (almost) at rest; the frame_id changes length, so no field is aligned
    const uint32_t n_imu = 110;
    std::vector<unsigned char> bag;
    std::vector<uint64_t> msg_off;
    for (uint32_t i = 0; i < n_imu; ++i) {
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
    lk_imu* d_imus = static_cast<lk_imu*>(device_room(sizeof(lk_imu) * n_imu));
    ImuFrontend imu(true, kilo->device_ptr());
    const size_t kept = imu.processingDev(d_bag, msg_off, d_imus);
    std::vector<uint32_t> n_msg;
    size_t consumed = 0;
    const size_t packaged = imu.syncPackages(d_imus, kept, scans.t_end, n_msg, &consumed);
    std::fprintf(stderr, "%zu of %u Imu messages kept, %zu of %u scans packaged\n", kept, n_imu, packaged, S);

    // package 0 starts the run; packages 1 .. are the live run: the front ends' tables shifted by one
    kilo->firstFrameDev(static_cast<const lk_point*>(d_raw), n_raw, end0, 1, d_imus, n_msg[0]);
    const std::vector<uint64_t> run_off(scans.scan_off.begin() + 1, scans.scan_off.begin() + 1 + packaged);
    const std::vector<double> run_begin(scans.t_begin.begin() + 1, scans.t_begin.begin() + packaged);
    const std::vector<uint32_t> run_msg(n_msg.begin() + 1, n_msg.begin() + packaged);
    float* d_world = static_cast<float*>(device_room(16 * scans.scan_off[S]));   // the run's registered cloud, index-aligned with the scans
    const lk_run_options slide{8.0, 100, 0};
    uint32_t n_slides = 0;
    const std::vector<lk_pose> poses = kilo->runScans(scans.data(), run_off, run_begin, 1, run_msg, d_imus + n_msg[0], &slide, d_world, &n_slides);
    for (size_t s = 0; s < poses.size(); ++s) {
        double q[4];
        rot_to_quat(poses[s].rot, q);
        std::printf("%.9f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n", scans.t_end[s + 1], poses[s].pos[0], poses[s].pos[1], poses[s].pos[2], q[0], q[1], q[2], q[3]);
    }
    std::fprintf(stderr, "%zu scans, %u map slides\n", poses.size(), n_slides);
    for (void* d : {d_clouds, d_raw, d_bag, static_cast<void*>(d_imus), static_cast<void*>(d_world)}) lk_device_free(dev.h(), d);
    return 0;
}
