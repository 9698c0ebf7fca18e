// legkilo_host.hpp — C++ mirror of the reference class surface that KILO consumes, implemented purely on
// the C-ABI of include/legkilo_hip.h (no HIP, no torch, no Eigen in this header).
//
//   legkilo::ESKF              <- legkilo/src/core/slam/eskf.h:46-109
//   legkilo::VoxelMapManager   <- legkilo/src/core/slam/voxel_map.h:180-244 (live members)
//   legkilo::KiloPath          <- KILO::predictUpdatePoint / predictUpdateImu / predictUpdateKinImu and the
//                                 bucket loop of KILO::process (KILO.cc:108-399)
//   legkilo::Kinematics        <- legkilo/src/preprocess/kinematics.h (Kinematics::processing for a batch of serialized HighState
//                                 messages, with kinematicImuCallBack's redundancy filter) + the kin branch of syncPackage
//   legkilo::ImuFrontend       <- RosInterface::imuCallBack for a batch of serialized sensor_msgs/Imu messages + the IMU branch of syncPackage
//   legkilo::LidarProcessing   <- legkilo/src/preprocess/lidar_processing.h (LidarProcessing::processing for a recorded run's
//                                 PointCloud2 messages in HBM, with the voxel grid and time sort of KILO.cc:356-370)
//
// Same method names, argument meaning and (void / bool) error behaviour as the reference.  Differences forced
// by the state living in HBM: state()/cov()/Q() return COPIES (use setState/setCov/setQ to write back), and
// build_single_residual takes the voxel KEY where the reference takes a VoxelOctoTree* (a batch of points per call; a bucket of the path
// goes through BuildResidualList(), which never leaves the GPU).
// Configuration errors throw std::runtime_error like YamlHelper does (yaml_helper.hpp:42,50).
#pragma once
#include <algorithm>
#include <array>
#include <cstddef>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "legkilo_hip.h"
#include "../csrc/lk_pcd_files.h"   // pcd_file_offsets: PcdSaver::workerLoop's counting over the run replays' tables (plain C++)

// The mirror lives in namespace legkilo, like the classes it stands in for.  Inside the reference's own tree that namespace already
// holds the Eigen typedefs of common/eigen_types.hpp (Vec3D, Mat3D, ...): there legkilo_host_eigen.hpp includes this header under
// another name (LEGKILO_HOST_NAMESPACE = legkilo_hip) and puts Eigen-typed classes with the reference's names on top of it.
#ifndef LEGKILO_HOST_NAMESPACE
#define LEGKILO_HOST_NAMESPACE legkilo
#endif

namespace LEGKILO_HOST_NAMESPACE {

constexpr int DIM_STATE = LK_DIM_STATE;
using Vec3D = std::array<double, 3>;
struct Mat3D {
    double m[9];  // row-major
    double& operator()(int i, int j) { return m[3 * i + j]; }
    double operator()(int i, int j) const { return m[3 * i + j]; }
    static Mat3D Identity() { return Mat3D{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; }
};
using StateVec = std::array<double, DIM_STATE>;
struct StateCov {
    std::vector<double> d = std::vector<double>(DIM_STATE * DIM_STATE, 0.0);  // row-major
    double& operator()(int i, int j) { return d[i * DIM_STATE + j]; }
    double operator()(int i, int j) const { return d[i * DIM_STATE + j]; }
    Mat3D block3(int o) const {
        Mat3D b;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) b(i, j) = (*this)(o + i, o + j);
        return b;
    }
};
using StateF = StateCov;
using StateQ = StateCov;

// eskf.h:15-32
struct State {
    Mat3D rot_ = Mat3D::Identity();
    Vec3D pos_{}, vel_{}, ba_{}, bw_{}, grav_{{0.0, 0.0, -9.81}}, imu_a_{}, imu_w_{}, bv_{}, contact_{};
    void to_x36(double* x) const {
        std::memcpy(x, rot_.m, sizeof(rot_.m));
        const Vec3D* v[9] = {&pos_, &vel_, &ba_, &bw_, &grav_, &imu_a_, &imu_w_, &bv_, &contact_};
        for (int k = 0; k < 9; ++k)
            for (int c = 0; c < 3; ++c) x[9 + 3 * k + c] = (*v[k])[c];
    }
    void from_x36(const double* x) {
        std::memcpy(rot_.m, x, sizeof(rot_.m));
        Vec3D* v[9] = {&pos_, &vel_, &ba_, &bw_, &grav_, &imu_a_, &imu_w_, &bv_, &contact_};
        for (int k = 0; k < 9; ++k)
            for (int c = 0; c < 3; ++c) (*v[k])[c] = x[9 + 3 * k + c];
    }
};

// eskf.h:34-44; pt_h is N x 6 and ki_h is M x 30, both row-major
struct ObsShared {
    std::vector<double> pt_z, pt_h, pt_R, ki_z, ki_h, ki_R;
};

// voxel_map.h:41-57
struct VoxelMapConfig {
    double max_voxel_size_ = 0.5;
    int max_layer_ = 2;
    int max_iterations_ = 0;
    std::vector<int> layer_init_num_{5, 5, 5, 5, 5};
    int max_points_num_ = 50;
    double planner_threshold_ = 0.01, beam_err_ = 0.2, dept_err_ = 0.04, sigma_num_ = 3;
    bool is_pub_plane_map_ = false;
    double sliding_thresh = 8;      // loaded, never consulted by the reference (KILO.cc:68-70)
    bool map_sliding_en = false;
    int half_map_size = 100;
};

// voxel_map.h:59-78: the two fields UpdateVoxelMap reads
struct pointWithVar {
    Vec3D point_w{};
    Mat3D var{};
};

// PointToPlane (voxel_map.h:80-94): what build_single_residual writes into it and KILO.cc:160-210 reads of it
struct PointToPlane {
    Vec3D point_w_{}, normal_{}, center_{};
    int layer_ = -1;
    double d_ = 0.0;
    float dis_to_plane_ = 0.0f;
};

// PointType (pcl_types.h:11) fields the path touches
struct PointType {
    float x = 0, y = 0, z = 0, intensity = 0, curvature = 0;
};
using PointCloudType = std::vector<PointType>;

struct DeviceCaps {
    int device_id = 0;
    uint32_t n_slots = 1, max_roots = 1u << 18, max_nodes = 1u << 19, max_point_blocks = 1u << 18, max_scan_points = 1u << 17;
};

// One lk_handle shared by the ESKF and VoxelMapManager mirrors (they are two views of the same device state).
class Device {
   public:
    Device(const lk_config& cfg) {
        if (lk_create(&cfg, &h_) != LK_OK) throw std::runtime_error(std::string("lk_create: ") + lk_last_error(nullptr));
        cfg_ = cfg;
    }
    ~Device() { lk_destroy(h_); }
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    lk_handle* h() const { return h_; }
    const lk_config& cfg() const { return cfg_; }
    void check(int rc) const {
        if (rc != LK_OK) throw std::runtime_error(std::string("liblegkilo_hip: ") + lk_last_error(h_));
    }

   private:
    lk_handle* h_ = nullptr;
    lk_config cfg_;
};

class ESKF {
   public:
    // eskf.h:49-65
    struct Config {
        double vel_process_cov, imu_acc_process_cov, imu_gyr_process_cov, contact_process_cov, acc_bias_process_cov,
            gyr_bias_process_cov, kin_bias_process_cov;
        double imu_acc_meas_noise, imu_acc_z_meas_noise, imu_gyr_meas_noise, kin_meas_noise, chd_meas_noise,
            contact_meas_noise, lidar_point_meas_ratio;
    };
    ESKF(const Config& config, std::shared_ptr<Device> dev) : config_(config), dev_(std::move(dev)) {}

    State state() const {
        double x[LK_STATE_DOUBLES];
        dev_->check(lk_get_state(dev_->h(), 0, x, nullptr));
        State s;
        s.from_x36(x);
        return s;
    }
    void setState(const State& s) {
        double x[LK_STATE_DOUBLES];
        s.to_x36(x);
        dev_->check(lk_set_state(dev_->h(), 0, x, nullptr));
    }
    Mat3D getRot() const { return state().rot_; }
    Vec3D getPos() const { return state().pos_; }
    Vec3D getVel() const { return state().vel_; }
    Mat3D getRotCov() const { return cov().block3(0); }
    Mat3D getPosCov() const { return cov().block3(3); }
    Mat3D getVelCov() const { return cov().block3(6); }
    StateQ Q() const {
        StateQ q;
        dev_->check(lk_get_Q(dev_->h(), q.d.data()));
        return q;
    }
    void setQ(const StateQ& q) { dev_->check(lk_set_Q(dev_->h(), q.d.data())); }
    StateCov cov() const {
        StateCov c;
        dev_->check(lk_get_state(dev_->h(), 0, nullptr, c.d.data()));
        return c;
    }
    void setCov(const StateCov& c) { dev_->check(lk_set_state(dev_->h(), 0, nullptr, c.d.data())); }
    const Config& config() const { return config_; }

    void initProcessCovQ() { dev_->check(lk_init_process_cov_q(dev_->h())); }
    StateVec getFunctionf(double dt) {
        StateVec f;
        dev_->check(lk_get_function_f(dev_->h(), 0, dt, f.data()));
        return f;
    }
    StateF getFx(double dt) {
        StateF F;
        dev_->check(lk_get_fx(dev_->h(), 0, dt, F.d.data()));
        return F;
    }
    void predict(double dt, bool prop_state, bool prop_cov) { dev_->check(lk_predict(dev_->h(), 0, dt, prop_state, prop_cov)); }
    void updateByPoints(ObsShared& o) {
        dev_->check(lk_update_by_points(dev_->h(), 0, o.pt_h.data(), o.pt_z.data(), o.pt_R.data(), o.pt_z.size()));
    }
    void updateByImu(ObsShared& o) { dev_->check(lk_update_by_imu(dev_->h(), 0, o.ki_z.data(), o.ki_R.data())); }
    void updateByKinImu(ObsShared& o) {
        dev_->check(lk_update_by_kin_imu(dev_->h(), 0, o.ki_h.data(), o.ki_z.data(), o.ki_R.data(), o.ki_z.size()));
    }

   private:
    Config config_;
    std::shared_ptr<Device> dev_;
};

class VoxelMapManager {
   public:
    VoxelMapManager(VoxelMapConfig& config_setting, std::shared_ptr<Device> dev) : config_setting_(config_setting), dev_(std::move(dev)) {}
    VoxelMapConfig config_setting_;
    Mat3D extR_ = Mat3D::Identity();
    Vec3D extT_{};
    std::shared_ptr<PointCloudType> feats_down_body_, feats_down_world_;

    // voxel_map.cc:287-334.  rot / rot_cov / pos_cov are those of the filter (KILO.cc:339) and already live on
    // the device; the arguments are kept for source compatibility.
    void BuildVoxelMap(const Mat3D&, const Mat3D&, const Mat3D&) {
        if (!feats_down_body_ || !feats_down_world_ || feats_down_body_->size() != feats_down_world_->size())
            throw std::runtime_error("BuildVoxelMap: feats_down_body_/feats_down_world_ not set");
        std::vector<float> w, b;
        for (size_t i = 0; i < feats_down_world_->size(); ++i) {
            const PointType &pw = (*feats_down_world_)[i], &pb = (*feats_down_body_)[i];
            w.insert(w.end(), {pw.x, pw.y, pw.z});
            b.insert(b.end(), {pb.x, pb.y, pb.z});
        }
        dev_->check(lk_map_build(dev_->h(), w.data(), b.data(), feats_down_world_->size()));
    }
    // voxel_map.cc:336-361
    void UpdateVoxelMap(const std::vector<pointWithVar>& input_points) {
        std::vector<double> pw, var;
        for (const auto& p : input_points) {
            pw.insert(pw.end(), p.point_w.begin(), p.point_w.end());
            var.insert(var.end(), p.var.m, p.var.m + 9);
        }
        dev_->check(lk_map_update(dev_->h(), pw.data(), var.data(), input_points.size()));
    }
    // voxel_map.cc:552-569.  position_last_ is the public member the caller sets (voxel_map.h:199); last_slide_position
    // (voxel_map.h:201) lives in the device handle.
    Vec3D position_last_{};
    bool mapSliding() {
        int32_t slid = 0;
        dev_->check(lk_map_slide(dev_->h(), position_last_.data(), config_setting_.sliding_thresh, config_setting_.half_map_size, &slid, nullptr));
        return slid != 0;
    }
    // voxel_map.cc:571-594
    void clearMemOutOfMap(const int& x_max, const int& x_min, const int& y_max, const int& y_min, const int& z_max, const int& z_min) {
        dev_->check(lk_map_clear_outside(dev_->h(), x_max, x_min, y_max, y_min, z_max, z_min, nullptr));
    }
    // voxel_map.cc:363-427 for points the caller holds as pointWithVar, each started on the root voxel at keys[i] with
    // is_success = false, prob = 0 (KILO.cc:149-155).  found[i]: the find of KILO.cc:149 hit.  The reference's argument
    // `const VoxelOctoTree* current_octo` has no host-side counterpart (the octrees live in HBM): the key stands in for it.
    void build_single_residual(const std::vector<pointWithVar>& pv, const std::vector<std::array<int32_t, 3>>& keys, std::vector<uint8_t>& found,
                               std::vector<uint8_t>& is_success, std::vector<double>& prob, std::vector<PointToPlane>& single_ptpl) {
        const size_t n = pv.size();
        if (keys.size() != n) throw std::runtime_error("build_single_residual: one key per point");
        std::vector<int32_t> k(3 * n);
        std::vector<double> pw(3 * n), var(9 * n), nrm(3 * n), ctr(3 * n), d(n);
        std::vector<float> dis(n);
        std::vector<int32_t> layer(n);
        for (size_t i = 0; i < n; ++i) {
            std::copy(keys[i].begin(), keys[i].end(), k.begin() + 3 * i);
            std::copy(pv[i].point_w.begin(), pv[i].point_w.end(), pw.begin() + 3 * i);
            std::copy(pv[i].var.m, pv[i].var.m + 9, var.begin() + 9 * i);
        }
        found.assign(n, 0), is_success.assign(n, 0), prob.assign(n, 0.0), single_ptpl.assign(n, PointToPlane());
        dev_->check(lk_match_points(dev_->h(), n, k.data(), pw.data(), var.data(), found.data(), is_success.data(), prob.data(), nrm.data(), ctr.data(),
                                    d.data(), dis.data(), layer.data()));
        for (size_t i = 0; i < n; ++i) {
            PointToPlane& t = single_ptpl[i];
            t.point_w_ = pv[i].point_w;
            for (int c = 0; c < 3; ++c) t.normal_[c] = nrm[3 * i + c], t.center_[c] = ctr[3 * i + c];
            t.layer_ = layer[i], t.d_ = d[i], t.dis_to_plane_ = dis[i];
        }
    }
    // Residual build of KILO.cc:122-210 for a whole bucket (replaces the per-point build_single_residual calls).
    void BuildResidualList(const PointCloudType& body, size_t i0, size_t i1, ObsShared& obs, std::vector<uint8_t>& valid) {
        size_t n = i1 - i0;
        std::vector<float> b;
        for (size_t i = i0; i < i1; ++i) b.insert(b.end(), {body[i].x, body[i].y, body[i].z});
        std::vector<double> h(6 * n), z(n), R(n);
        valid.assign(n, 0);
        dev_->check(lk_residuals(dev_->h(), b.data(), n, h.data(), z.data(), R.data(), valid.data()));
        obs.pt_h.clear(), obs.pt_z.clear(), obs.pt_R.clear();
        for (size_t k = 0; k < n; ++k)
            if (valid[k]) {
                obs.pt_h.insert(obs.pt_h.end(), h.begin() + 6 * k, h.begin() + 6 * k + 6);
                obs.pt_z.push_back(z[k]);
                obs.pt_R.push_back(R[k]);
            }
    }

   private:
    std::shared_ptr<Device> dev_;
};

// The path of KILO (KILO.cc:108-399) with the reference's private method names.
class KiloPath {
   public:
    KiloPath(const ESKF::Config& ec, VoxelMapConfig& vc, const Mat3D& ext_rot, const Vec3D& ext_t, double gravity,
             const DeviceCaps& caps = DeviceCaps()) {
        lk_config c;
        std::memset(&c, 0, sizeof(c));
        std::memcpy(&c.vel_process_cov, &ec, sizeof(ec));  // same 14 doubles, same order (eskf.h:49-65)
        c.max_voxel_size = vc.max_voxel_size_;
        c.planner_threshold = vc.planner_threshold_;
        c.beam_err = vc.beam_err_;
        c.dept_err = vc.dept_err_;
        c.sigma_num = vc.sigma_num_;
        c.max_layer = vc.max_layer_;
        c.max_iterations = vc.max_iterations_;
        if (vc.layer_init_num_.size() < 5) throw std::runtime_error("layer_init_num needs 5 entries");
        for (int i = 0; i < 5; ++i) c.layer_init_num[i] = vc.layer_init_num_[i];
        c.max_points_num = vc.max_points_num_;
        std::memcpy(c.ext_R, ext_rot.m, sizeof(c.ext_R));
        for (int i = 0; i < 3; ++i) c.ext_T[i] = ext_t[i];
        c.gravity = gravity;
        c.device_id = caps.device_id;
        c.n_slots = caps.n_slots;
        c.max_roots = caps.max_roots;
        c.max_nodes = caps.max_nodes;
        c.max_point_blocks = caps.max_point_blocks;
        c.max_scan_points = caps.max_scan_points;
        dev_ = std::make_shared<Device>(c);
        eskf_ = std::make_unique<ESKF>(ec, dev_);
        map_manager_ = std::make_unique<VoxelMapManager>(vc, dev_);
        map_manager_->extR_ = ext_rot;
        map_manager_->extT_ = ext_t;
    }
    ESKF& eskf() { return *eskf_; }
    VoxelMapManager& map_manager() { return *map_manager_; }
    Device& device() { return *dev_; }   // the lk_handle behind both mirrors (multi-GPU helpers: legkilo_rccl.hpp)
    std::shared_ptr<Device> device_ptr() { return dev_; }   // ... shared with the front-end mirrors (Kinematics, ImuFrontend, LidarProcessing)
    void setTimes(double last_predict, double last_update) { dev_->check(lk_set_times(dev_->h(), 0, last_predict, last_update)); }
    void setAccNorm(double a) { dev_->check(lk_set_acc_norm(dev_->h(), a)); }
    double accNorm() const {
        double a = 0.0;
        dev_->check(lk_get_acc_norm(dev_->h(), &a));
        return a;
    }

    // The first frame of KILO::process (KILO.cc:332-352) as one call (lk_first_frame): state initialisation from the first package's
    // messages (state_initial.hpp), cloudLidarToWorld on the RAW cloud, BuildVoxelMap, acc_norm_ and both time stamps = end_time.
    // Exactly one of the two message vectors is non-empty (only_imu_use: imus).
    void firstFrame(const std::vector<lk_point>& cloud_raw, double end_time, const std::vector<lk_imu>& imus, const std::vector<lk_kin_imu>& kins = {}) {
        if (imus.empty() == kins.empty()) throw std::runtime_error("firstFrame: IMU messages or kinematic + IMU messages, one of the two");
        const bool imu_mode = !imus.empty();
        dev_->check(lk_first_frame(dev_->h(), cloud_raw.data(), cloud_raw.size(), end_time, imu_mode ? 1 : 2,
                                   imu_mode ? static_cast<const void*>(imus.data()) : static_cast<const void*>(kins.data()), imu_mode ? imus.size() : kins.size()));
    }
    // the same with the decoded cloud (lk_decode_scan_dev) and the decoded records (msg_kind 1: lk_imu, 2: lk_kin_imu) where they lie in HBM
    void firstFrameDev(const lk_point* d_cloud_raw, size_t n, double end_time, int msg_kind, const void* d_msgs, size_t n_msg) {
        dev_->check(lk_first_frame_dev(dev_->h(), d_cloud_raw, n, end_time, msg_kind, d_msgs, n_msg));
    }
    // lk_batch_replay_scans_imu_dev: recorded scans and their IMU records, both in HBM (ImuFrontend::syncPackages says how many per scan)
    std::vector<lk_pose> replayRecordedRunImuDev(const lk_point* d_pts, const std::vector<uint64_t>& scan_off, const std::vector<double>& t_begin,
                                                 const std::vector<uint32_t>& n_msg, const lk_imu* d_imus) {
        const size_t S = t_begin.size();
        if (scan_off.size() != S + 1 || n_msg.size() != S) throw std::runtime_error("replayRecordedRunImuDev: table sizes differ");
        std::vector<lk_pose> out(S);
        dev_->check(lk_batch_replay_scans_imu_dev(dev_->h(), d_pts, S, scan_off.data(), t_begin.data(), n_msg.data(), d_imus, out.data()));
        return out;
    }
    // lk_batch_replay_overlay_runs_dev: whole recorded runs WITH the map insert, run r = the scans run_off[r] .. run_off[r+1) on filter slot r, each
    // scan one KILO::process - state, covariance, times and the slot's copy-on-write overlay carried across the scan boundaries, the map itself
    // untouched.  Scans and message records (msg_kind 0 none, 1 lk_imu, 2 lk_kin_imu; n_msg[s] per scan) lie in HBM, as the front ends leave
    // them.  Priors: lk_batch_set_priors.  Returns one pose per SCAN, its counters that scan's alone.
    // d_world_out / bucket_poses (lk_batch_replay_overlay_runs_cloud_dev; both optional): the scans registered into the world frame, one 16-byte x y z
    // intensity record per point of d_pts under the state after the point's time bucket (cloud_down_world_out of KILO::process), and the state after
    // every bucket - scan s owns (*scan_bucket_off)[s] .. [s+1] of *bucket_poses.  Without them this is lk_batch_replay_overlay_runs_dev.
    std::vector<lk_pose> replayRunsWithInsertDev(const lk_point* d_pts, const std::vector<uint32_t>& run_off, const std::vector<uint64_t>& scan_off,
                                                 const std::vector<double>& t_begin, int msg_kind, const std::vector<uint32_t>& n_msg, const void* d_msgs,
                                                 float* d_world_out = nullptr, std::vector<lk_bucket_pose>* bucket_poses = nullptr,
                                                 std::vector<uint32_t>* scan_bucket_off = nullptr) {
        const size_t S = t_begin.size();
        if (run_off.size() < 2 || run_off.back() != S || scan_off.size() != S + 1 || (msg_kind && n_msg.size() != S))
            throw std::runtime_error("replayRunsWithInsertDev: table sizes differ");
        std::vector<lk_pose> out(S);
        std::vector<uint32_t> sbo(bucket_poses || scan_bucket_off ? S + 1 : 0);
        dev_->check(lk_batch_replay_overlay_runs_cloud_dev(dev_->h(), d_pts, run_off.size() - 1, run_off.data(), scan_off.data(), t_begin.data(), msg_kind,
                                                           msg_kind ? n_msg.data() : nullptr, d_msgs, out.data(), d_world_out, sbo.empty() ? nullptr : sbo.data()));
        fetchBucketPoses(sbo, bucket_poses, scan_bucket_off);
        return out;
    }
    // what the two run replays share behind a _cloud call: the whole bucket table (lk_runs_bucket_poses) and the scans' ranges in it
    void fetchBucketPoses(std::vector<uint32_t>& sbo, std::vector<lk_bucket_pose>* bucket_poses, std::vector<uint32_t>* scan_bucket_off) {
        if (bucket_poses) {
            bucket_poses->resize(sbo.back());
            dev_->check(lk_runs_bucket_poses(dev_->h(), 0, bucket_poses->size(), bucket_poses->data()));
        }
        if (scan_bucket_off) scan_bucket_off->swap(sbo);
    }
    // lk_runs_ate_dev: every run of the last _cloud replay scored against ground truth where its bucket table lies - nearest stamp within max_dt,
    // align: the best rigid motion removed first (tum.py's associate + ate).  Run r = the records run_bucket_off[r] .. [r+1]) of the table
    // (scan_bucket_off[run_off[r]]); ground truth in HBM, sample k gt_stride bytes behind d_gt_t / d_gt_pos, trajectory r the samples gt_off[r] ..
    // [r+1]).  One lk_ate per run: "choose a slot" is the run with the smallest rmse among those with status 0 and n_pairs > 0.
    std::vector<lk_ate> runsAteDev(const std::vector<uint64_t>& run_bucket_off, const double* d_gt_t, const double* d_gt_pos, size_t gt_stride,
                                   const std::vector<uint64_t>& gt_off, double max_dt, bool align = false) {
        if (run_bucket_off.size() < 2 || gt_off.size() != run_bucket_off.size()) throw std::runtime_error("runsAteDev: table sizes differ");
        std::vector<lk_ate> out(run_bucket_off.size() - 1);
        dev_->check(lk_runs_ate_dev(dev_->h(), out.size(), run_bucket_off.data(), d_gt_t, d_gt_pos, gt_stride, gt_off.data(), max_dt,
                                    align ? LK_ATE_ALIGN : 0u, out.data()));
        return out;
    }
    // lk_traj_ate_dev: the same over trajectories the caller holds in HBM (strided tables on both sides)
    std::vector<lk_ate> trajAteDev(const double* d_est_t, const double* d_est_pos, size_t est_stride, const std::vector<uint64_t>& est_off,
                                   const double* d_gt_t, const double* d_gt_pos, size_t gt_stride, const std::vector<uint64_t>& gt_off, double max_dt,
                                   bool align = false) {
        if (est_off.size() < 2 || gt_off.size() != est_off.size()) throw std::runtime_error("trajAteDev: table sizes differ");
        std::vector<lk_ate> out(est_off.size() - 1);
        dev_->check(lk_traj_ate_dev(dev_->h(), out.size(), d_est_t, d_est_pos, est_stride, est_off.data(), d_gt_t, d_gt_pos, gt_stride, gt_off.data(),
                                    max_dt, align ? LK_ATE_ALIGN : 0u, out.data()));
        return out;
    }
    // lk_runs_rpe_dev: every run of the last _cloud replay scored by its drift per step, translation and rotation, where its bucket table lies (t, pos
    // AND rot of the records; tum.py's rpe).  A step reaches from bucket i to the first later one at least `delta` seconds on (by_index: `delta`
    // buckets on) and counts when both ends find a ground-truth partner within max_dt; d_gt_rot: nine row-major doubles per sample, body -> world.
    // One lk_rpe per run; worst_trans / worst_rot name the first bucket of the worst step.
    std::vector<lk_rpe> runsRpeDev(const std::vector<uint64_t>& run_bucket_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot,
                                   size_t gt_stride, const std::vector<uint64_t>& gt_off, double max_dt, double delta, bool by_index = false) {
        if (run_bucket_off.size() < 2 || gt_off.size() != run_bucket_off.size()) throw std::runtime_error("runsRpeDev: table sizes differ");
        std::vector<lk_rpe> out(run_bucket_off.size() - 1);
        dev_->check(lk_runs_rpe_dev(dev_->h(), out.size(), run_bucket_off.data(), d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off.data(), max_dt, delta,
                                    by_index ? LK_RPE_INDEX : 0u, out.data()));
        return out;
    }
    // lk_traj_rpe_dev: the same over trajectories the caller holds in HBM (strided tables on both sides)
    std::vector<lk_rpe> trajRpeDev(const double* d_est_t, const double* d_est_pos, const double* d_est_rot, size_t est_stride,
                                   const std::vector<uint64_t>& est_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot,
                                   size_t gt_stride, const std::vector<uint64_t>& gt_off, double max_dt, double delta, bool by_index = false) {
        if (est_off.size() < 2 || gt_off.size() != est_off.size()) throw std::runtime_error("trajRpeDev: table sizes differ");
        std::vector<lk_rpe> out(est_off.size() - 1);
        dev_->check(lk_traj_rpe_dev(dev_->h(), out.size(), d_est_t, d_est_pos, d_est_rot, est_stride, est_off.data(), d_gt_t, d_gt_pos, d_gt_rot,
                                    gt_stride, gt_off.data(), max_dt, delta, by_index ? LK_RPE_INDEX : 0u, out.data()));
        return out;
    }
    // lk_clouds_c2c_dev: map clouds scored against a reference cloud where they lie - cloud c of a side = the 16-byte x y z w records
    // off[c] .. off[c + 1]) at its device pointer (a replay's d_world_out, downsampleCloudsDev's output and offsets; both sides may be one buffer),
    // pairs[k] = (query cloud, reference cloud).  A query point is matched when its nearest reference point lies within max_dist; thr (up to four,
    // each <= max_dist) are counted in n_within.  One lk_c2c per pair.  d_nn_idx / d_nn_d2 (both or neither) take the neighbour and the squared
    // distance per pair and query point, pair k's from entry (*nn_off)[k] on.  (No Eigen mirror: the reference has no type this would fit.)
    std::vector<lk_c2c> cloudsC2cDev(const float* d_query, const std::vector<uint64_t>& q_off, const float* d_ref, const std::vector<uint64_t>& r_off,
                                     const std::vector<std::pair<uint32_t, uint32_t>>& pairs, double max_dist, const std::vector<double>& thr = {},
                                     uint32_t* d_nn_idx = nullptr, double* d_nn_d2 = nullptr, std::vector<uint64_t>* nn_off = nullptr) {
        if (q_off.size() < 2 || r_off.size() < 2 || pairs.empty()) throw std::runtime_error("cloudsC2cDev: an offset table or the pairs are empty");
        std::vector<uint32_t> pq(pairs.size()), pr(pairs.size());
        for (size_t k = 0; k < pairs.size(); ++k) pq[k] = pairs[k].first, pr[k] = pairs[k].second;
        std::vector<lk_c2c> out(pairs.size());
        std::vector<uint64_t> off(pairs.size() + 1);
        dev_->check(lk_clouds_c2c_dev(dev_->h(), d_query, q_off.size() - 1, q_off.data(), d_ref, r_off.size() - 1, r_off.data(), pairs.size(), pq.data(),
                                      pr.data(), max_dist, thr.empty() ? nullptr : thr.data(), (uint32_t)thr.size(), out.data(), d_nn_idx, d_nn_d2, off.data()));
        if (nn_off) *nn_off = off;
        return out;
    }
    // lk_clouds_align_dev: map clouds aligned to a reference cloud where they lie (point-to-point ICP, the loop on the device) - cloudsC2cDev's
    // clouds, tables and pairs; T0 = 12 doubles per pair, R row-major then t with r ~ R q + t (empty: the identity; lk_runs_ate_dev with LK_ATE_ALIGN
    // gives a run's rot / trans), up to max_iter solves until one moves by no more than eps_rot (radians) and eps_trans (metres).  One lk_align per
    // pair; c2c_out takes the lk_c2c records of the final search, the nn outputs its neighbours.
    std::vector<lk_align> cloudsAlignDev(const float* d_query, const std::vector<uint64_t>& q_off, const float* d_ref, const std::vector<uint64_t>& r_off,
                                         const std::vector<std::pair<uint32_t, uint32_t>>& pairs, double max_dist, const std::vector<double>& T0 = {},
                                         uint32_t max_iter = 30, double eps_rot = 1e-6, double eps_trans = 1e-6, std::vector<lk_c2c>* c2c_out = nullptr,
                                         const std::vector<double>& thr = {}, uint32_t* d_nn_idx = nullptr, double* d_nn_d2 = nullptr,
                                         std::vector<uint64_t>* nn_off = nullptr) {
        if (q_off.size() < 2 || r_off.size() < 2 || pairs.empty()) throw std::runtime_error("cloudsAlignDev: an offset table or the pairs are empty");
        if (!T0.empty() && T0.size() != 12 * pairs.size()) throw std::runtime_error("cloudsAlignDev: T0 holds 12 doubles per pair");
        std::vector<uint32_t> pq(pairs.size()), pr(pairs.size());
        for (size_t k = 0; k < pairs.size(); ++k) pq[k] = pairs[k].first, pr[k] = pairs[k].second;
        std::vector<lk_align> out(pairs.size());
        std::vector<lk_c2c> c2c(pairs.size());
        std::vector<uint64_t> off(pairs.size() + 1);
        dev_->check(lk_clouds_align_dev(dev_->h(), d_query, q_off.size() - 1, q_off.data(), d_ref, r_off.size() - 1, r_off.data(), pairs.size(), pq.data(),
                                        pr.data(), max_dist, thr.empty() ? nullptr : thr.data(), (uint32_t)thr.size(), T0.empty() ? nullptr : T0.data(), max_iter,
                                        eps_rot, eps_trans, out.data(), c2c.data(), d_nn_idx, d_nn_d2, off.data()));
        if (c2c_out) *c2c_out = c2c;
        if (nn_off) *nn_off = off;
        return out;
    }
    // lk_clouds_align_plane_dev: cloudsAlignDev with the point-to-plane solve against d_ref_normals (one nx ny nz w record per reference record, at
    // d_ref's index; cloudsNormalsDev writes them).  pl_out takes the lk_align_plane records; LK_ALIGN_DEGENERATE marks a pair whose used normals
    // leave a direction unobserved.
    std::vector<lk_align> cloudsAlignPlaneDev(const float* d_query, const std::vector<uint64_t>& q_off, const float* d_ref, const std::vector<uint64_t>& r_off,
                                              const float* d_ref_normals, const std::vector<std::pair<uint32_t, uint32_t>>& pairs, double max_dist,
                                              const std::vector<double>& T0 = {}, uint32_t max_iter = 30, double eps_rot = 1e-6, double eps_trans = 1e-6,
                                              std::vector<lk_align_plane>* pl_out = nullptr, std::vector<lk_c2c>* c2c_out = nullptr, const std::vector<double>& thr = {},
                                              uint32_t* d_nn_idx = nullptr, double* d_nn_d2 = nullptr, std::vector<uint64_t>* nn_off = nullptr) {
        if (q_off.size() < 2 || r_off.size() < 2 || pairs.empty()) throw std::runtime_error("cloudsAlignPlaneDev: an offset table or the pairs are empty");
        if (!T0.empty() && T0.size() != 12 * pairs.size()) throw std::runtime_error("cloudsAlignPlaneDev: T0 holds 12 doubles per pair");
        std::vector<uint32_t> pq(pairs.size()), pr(pairs.size());
        for (size_t k = 0; k < pairs.size(); ++k) pq[k] = pairs[k].first, pr[k] = pairs[k].second;
        std::vector<lk_align> out(pairs.size());
        std::vector<lk_align_plane> pl(pairs.size());
        std::vector<lk_c2c> c2c(pairs.size());
        std::vector<uint64_t> off(pairs.size() + 1);
        dev_->check(lk_clouds_align_plane_dev(dev_->h(), d_query, q_off.size() - 1, q_off.data(), d_ref, r_off.size() - 1, r_off.data(), pairs.size(), pq.data(),
                                              pr.data(), max_dist, thr.empty() ? nullptr : thr.data(), (uint32_t)thr.size(), T0.empty() ? nullptr : T0.data(),
                                              max_iter, eps_rot, eps_trans, d_ref_normals, out.data(), pl.data(), c2c.data(), d_nn_idx, d_nn_d2, off.data()));
        if (pl_out) *pl_out = pl;
        if (c2c_out) *c2c_out = c2c;
        if (nn_off) *nn_off = off;
        return out;
    }
    // lk_clouds_normals_dev: per-point normals where the clouds lie - cloudsMmeDev's clouds, table and neighbourhoods; record off[c] + i gets
    // (nx, ny, nz, planarity) at entry off[c] - off[0] + i of d_normals, NaN in nx ny nz below min_pts (>= 3) neighbours or min_planarity.
    std::vector<lk_normals> cloudsNormalsDev(const float* d_clouds, const std::vector<uint64_t>& off, double radius, float* d_normals, uint32_t min_pts = 5,
                                             double min_planarity = 0.0) {
        if (off.size() < 2) throw std::runtime_error("cloudsNormalsDev: the offset table is empty");
        std::vector<lk_normals> out(off.size() - 1);
        dev_->check(lk_clouds_normals_dev(dev_->h(), d_clouds, off.size() - 1, off.data(), radius, min_pts, min_planarity, out.data(), d_normals));
        return out;
    }
    // lk_clouds_transform_dev: the moved clouds - record off[c] + i of d_in to entry off[c] - off[0] + i of d_out under T[c] (12 doubles a cloud),
    // rounded once to float32, w copied; d_out may be d_in + 4 * off[0] (in place).  What cloudsC2cDev / cloudsMmeDev take after an alignment.
    void cloudsTransformDev(const float* d_in, const std::vector<uint64_t>& off, const std::vector<double>& T, float* d_out) {
        if (off.size() < 2 || T.size() != 12 * (off.size() - 1)) throw std::runtime_error("cloudsTransformDev: the offset table is empty or T does not hold 12 doubles per cloud");
        dev_->check(lk_clouds_transform_dev(dev_->h(), d_in, off.size() - 1, off.data(), T.data(), d_out));
    }
    // lk_clouds_mme_dev: map clouds scored WITHOUT a reference where they lie - mean map entropy and mean plane variance, both lower for a crisper
    // map.  Cloud c = the 16-byte x y z w records off[c] .. off[c + 1]) at d_clouds (a replay's d_world_out, downsampleCloudsDev's output and
    // offsets).  A point's neighbourhood is every record of its cloud within `radius`, itself included; min_pts (>= 4) of them make it dense.  One
    // lk_mme per cloud.  d_n / d_h / d_lmin (each optional) take n_i, h_i and lmin_i per record, entry off[c] - off[0] + i.
    std::vector<lk_mme> cloudsMmeDev(const float* d_clouds, const std::vector<uint64_t>& off, double radius, uint32_t min_pts = 5, uint32_t* d_n = nullptr,
                                     double* d_h = nullptr, double* d_lmin = nullptr) {
        if (off.size() < 2) throw std::runtime_error("cloudsMmeDev: the offset table is empty");
        std::vector<lk_mme> out(off.size() - 1);
        dev_->check(lk_clouds_mme_dev(dev_->h(), d_clouds, off.size() - 1, off.data(), radius, min_pts, out.data(), d_n, d_h, d_lmin));
        return out;
    }
    // lk_clouds_sor_dev: outliers removed from map clouds where they lie - cloudsMmeDev's clouds and table.  A point with fewer than k (1 .. 32)
    // other records within `reach` is isolated; the others are kept when the mean distance to their k nearest is at most mu + n_sigma * sigma of
    // their cloud (n_sigma = infinity: the radius criterion alone).  d_out (room for off.back() - off.front() records) takes the kept records in
    // input order, cloud c at (*out_off)[c] .. (*out_off)[c + 1]) - what cloudsC2cDev, cloudsMmeDev, cloudsNormalsDev and the align entries take
    // as they are; d_src_idx their indices within their input clouds; d_keep / d_cnt / d_dbar (each optional) one entry per input record.
    std::vector<lk_sor> cloudsSorDev(const float* d_clouds, const std::vector<uint64_t>& off, uint32_t k, double reach, double n_sigma, float* d_out = nullptr,
                                     std::vector<uint64_t>* out_off = nullptr, uint32_t* d_src_idx = nullptr, uint8_t* d_keep = nullptr, uint32_t* d_cnt = nullptr,
                                     double* d_dbar = nullptr) {
        if (off.size() < 2) throw std::runtime_error("cloudsSorDev: the offset table is empty");
        if ((d_out || d_src_idx) && !out_off) throw std::runtime_error("cloudsSorDev: d_out and d_src_idx need out_off");
        std::vector<lk_sor> out(off.size() - 1);
        std::vector<uint64_t> oo(off.size());
        dev_->check(lk_clouds_sor_dev(dev_->h(), d_clouds, off.size() - 1, off.data(), k, reach, n_sigma, out.data(), d_out, out_off ? oo.data() : nullptr, d_src_idx,
                                      d_keep, d_cnt, d_dbar));
        if (out_off) *out_off = oo;
        return out;
    }
    // lk_clouds_cluster_dev: map clouds clustered where they lie (DBSCAN; min_pts = 1: the connected components within `reach`) - cloudsMmeDev's
    // clouds and table.  A point with min_pts records within `reach`, itself among them, is core; core points within reach of each other share a
    // cluster; another point joins the cluster of its nearest core point or is noise.  The arrays of ClusterOut (each optional, device memory) take a
    // label, a kind and n_i per input record, a size and a first core index per cluster - cluster k of cloud c at (*cl_off)[c] + k - and the points
    // of the clusters with min_size <= size <= max_size (flags LK_CLUSTER_KEEP_LARGEST: of the largest of them) in input order, cloud c at
    // (*out_off)[c] .. (*out_off)[c + 1]), what cloudsSorDev, cloudsMmeDev, cloudsC2cDev and the align entries take as they are.
    struct ClusterOut {   // (value-initialised: every pointer null)
        uint32_t* d_label;
        uint8_t* d_kind;
        uint32_t *d_n, *d_cl_size, *d_cl_first;
        std::vector<uint64_t>* cl_off;
        float* d_out;
        std::vector<uint64_t>* out_off;
        uint32_t* d_src_idx;
    };
    std::vector<lk_cluster> cloudsClusterDev(const float* d_clouds, const std::vector<uint64_t>& off, double reach, uint32_t min_pts = 1, uint32_t min_size = 0,
                                             uint32_t max_size = 0xffffffffu, uint32_t flags = 0, const ClusterOut& o = ClusterOut()) {
        if (off.size() < 2) throw std::runtime_error("cloudsClusterDev: the offset table is empty");
        if ((o.d_cl_size || o.d_cl_first) && !o.cl_off) throw std::runtime_error("cloudsClusterDev: d_cl_size and d_cl_first need cl_off");
        if ((o.d_out || o.d_src_idx) && !o.out_off) throw std::runtime_error("cloudsClusterDev: d_out and d_src_idx need out_off");
        std::vector<lk_cluster> out(off.size() - 1);
        std::vector<uint64_t> co(off.size()), oo(off.size());
        dev_->check(lk_clouds_cluster_dev(dev_->h(), d_clouds, off.size() - 1, off.data(), reach, min_pts, min_size, max_size, flags, out.data(), o.d_label, o.d_kind, o.d_n,
                                          o.d_cl_size, o.d_cl_first, o.cl_off ? co.data() : nullptr, o.d_out, o.out_off ? oo.data() : nullptr, o.d_src_idx));
        if (o.cl_off) *o.cl_off = co;
        if (o.out_off) *o.out_off = oo;
        return out;
    }
    // lk_clouds_planes_dev: the dominant planes peeled off map clouds where they lie (RANSAC; PCL's SACSegmentation with SACMODEL_PLANE, with an axis
    // SACMODEL_PERPENDICULAR_PLANE, repeated on what is left) - cloudsMmeDev's clouds and table.  Per round n_hyp planes through three sampled
    // records of the remainder; the one with the most records within `dist` wins, its records become plane r; up to max_planes rounds while a
    // winner holds min_inliers.  The arrays of PlanesOut (each optional, device memory) take a label per input record and the remainder (flags
    // LK_PLANES_KEEP_PLANES: the points on planes) in input order, cloud c at (*out_off)[c] .. (*out_off)[c + 1]) - ground and wall removal in
    // front of cloudsClusterDev.  *planes (optional) takes plane r of cloud c at c * max_planes + r.
    struct PlanesOut {   // (value-initialised: every pointer null)
        std::vector<lk_plane>* planes;
        uint32_t* d_label;
        float* d_out;
        std::vector<uint64_t>* out_off;
        uint32_t* d_src_idx;
    };
    std::vector<lk_planes> cloudsPlanesDev(const float* d_clouds, const std::vector<uint64_t>& off, double dist, uint32_t n_hyp = 256, uint32_t max_planes = 4,
                                           uint32_t min_inliers = 100, const double* axis = nullptr, double cos_max_angle = 0.0, uint64_t seed = 0, uint32_t flags = 0,
                                           const PlanesOut& o = PlanesOut()) {
        if (off.size() < 2) throw std::runtime_error("cloudsPlanesDev: the offset table is empty");
        if ((o.d_out || o.d_src_idx) && !o.out_off) throw std::runtime_error("cloudsPlanesDev: d_out and d_src_idx need out_off");
        std::vector<lk_planes> out(off.size() - 1);
        std::vector<lk_plane> pl((off.size() - 1) * (size_t)(max_planes ? max_planes : 1));
        std::vector<uint64_t> oo(off.size());
        dev_->check(lk_clouds_planes_dev(dev_->h(), d_clouds, off.size() - 1, off.data(), dist, n_hyp, max_planes, min_inliers, axis, cos_max_angle, seed, flags, out.data(),
                                         pl.data(), o.d_label, o.d_out, o.out_off ? oo.data() : nullptr, o.d_src_idx));
        if (o.planes) *o.planes = pl;
        if (o.out_off) *o.out_off = oo;
        return out;
    }
    // lk_overlay_commit: run (slot) `slot`'s overlay of the last replay with insert becomes part of the handle's map, in HBM - the map KILO::process
    // of that run would have left on a private copy; the other slots' overlays are stale afterwards.  adopt_filter (LK_COMMIT_ADOPT_FILTER): the
    // slot's whole filter record goes to slot 0, so that the live entries go on from the committed map.  Windowed mapping: replay a window with
    // insert on all slots, commit the chosen one, arm the next window's priors from lk_batch_get_states_dev.
    void commitOverlay(uint32_t slot, bool adopt_filter = false) {
        dev_->check(lk_overlay_commit(dev_->h(), slot, adopt_filter ? LK_COMMIT_ADOPT_FILTER : 0u));
    }
    // lk_batch_replay_runs_dev: the same runs on the FROZEN map (localisation against a finished map: no insert, no overlay, the map untouched) -
    // state, covariance and both time stamps carried across the scan boundaries.  cont (LK_RUNS_CONTINUE): the slots go on from what they hold, so
    // a run may be fed in chunks of scans, the first chunk with cont = false; the caller has not used the slots in between.  Tables as above.
    // d_world_out / bucket_poses / scan_bucket_off: as for replayRunsWithInsertDev (lk_batch_replay_runs_cloud_dev); a continued call records its chunk.
    std::vector<lk_pose> replayRunsDev(const lk_point* d_pts, const std::vector<uint32_t>& run_off, const std::vector<uint64_t>& scan_off,
                                       const std::vector<double>& t_begin, int msg_kind, const std::vector<uint32_t>& n_msg, const void* d_msgs,
                                       bool cont = false, float* d_world_out = nullptr, std::vector<lk_bucket_pose>* bucket_poses = nullptr,
                                       std::vector<uint32_t>* scan_bucket_off = nullptr) {
        const size_t S = t_begin.size();
        if (run_off.size() < 2 || run_off.back() != S || scan_off.size() != S + 1 || (msg_kind && n_msg.size() != S))
            throw std::runtime_error("replayRunsDev: table sizes differ");
        std::vector<lk_pose> out(S);
        std::vector<uint32_t> sbo(bucket_poses || scan_bucket_off ? S + 1 : 0);
        dev_->check(lk_batch_replay_runs_cloud_dev(dev_->h(), d_pts, run_off.size() - 1, run_off.data(), scan_off.data(), t_begin.data(), msg_kind,
                                                   msg_kind ? n_msg.data() : nullptr, d_msgs, cont ? LK_RUNS_CONTINUE : 0u, out.data(), d_world_out,
                                                   sbo.empty() ? nullptr : sbo.data()));
        fetchBucketPoses(sbo, bucket_poses, scan_bucket_off);
        return out;
    }
    // lk_downsample_clouds_dev behind a run replay's d_world_out: what PcdSaver (pcd_saver.hpp, defaults 100 frames per file, leaf 0.1 m) makes of the
    // registered frames up to the file container - a file after every frames_per_file non-empty scans of a run and at each run's end, pcl::VoxelGrid at
    // `leaf` per file.  d_out: room for scan_off.back() - scan_off[run_off[0]] records.  File f's cloud is d_out[(*out_off)[f] .. (*out_off)[f+1]) and
    // belongs to run (*file_run)[f]; (*unfiltered)[f] = 1 where the grid would overflow an int and the file is its input.  Returns the number of files.
    size_t downsampleCloudsDev(const float* d_world, const std::vector<uint32_t>& run_off, const std::vector<uint64_t>& scan_off, float* d_out,
                               std::vector<uint64_t>* out_off, std::vector<uint32_t>* file_run = nullptr, std::vector<uint8_t>* unfiltered = nullptr,
                               int frames_per_file = 100, float leaf = 0.1f) {
        if (run_off.size() < 2 || scan_off.size() != (size_t)run_off.back() + 1) throw std::runtime_error("downsampleCloudsDev: table sizes differ");
        const size_t R = run_off.size() - 1;
        std::vector<uint64_t> file_off(scan_off.size()), off(scan_off.size());
        std::vector<uint32_t> runs(scan_off.size());
        const size_t F = pcd_file_offsets(run_off.data(), R, scan_off.data(), frames_per_file, file_off.data(), runs.data());
        std::vector<uint8_t> unf(F);
        if (F) dev_->check(lk_downsample_clouds_dev(dev_->h(), d_world, F, file_off.data(), leaf, d_out, off.data(), unf.data()));
        off.resize(F + 1), runs.resize(F);
        if (out_off) out_off->swap(off);
        if (file_run) file_run->swap(runs);
        if (unfiltered) unfiltered->swap(unf);
        return F;
    }
    // lk_run_scans_dev: a recorded run LIVE on the handle's map (KILO::process scan after scan, the map growing), from scans and message records
    // that lie in HBM - msg_kind 0 none, 1 lk_imu, 2 lk_kin_imu; n_msg[s] records per scan at d_msgs.  slide: mapSliding after every scan
    // (lk_run_options), or null.  d_world_out: one 16-byte record per point of d_pts (cloud_down_world), or null.  Returns the poses of the scans
    // that went through; an error of scan k throws with k of them in *done (when given).
    std::vector<lk_pose> runScans(const lk_point* d_pts, const std::vector<uint64_t>& scan_off, const std::vector<double>& t_begin, int msg_kind,
                                  const std::vector<uint32_t>& n_msg, const void* d_msgs, const lk_run_options* slide = nullptr, float* d_world_out = nullptr,
                                  uint32_t* n_slides = nullptr, std::vector<lk_pose>* done = nullptr) {
        const size_t S = t_begin.size();
        if (scan_off.size() != S + 1 || (msg_kind && n_msg.size() != S)) throw std::runtime_error("runScans: table sizes differ");
        std::vector<lk_pose> out(std::max<size_t>(S, 1));
        size_t n_done = 0;
        const int rc = lk_run_scans_dev(dev_->h(), d_pts, S, scan_off.data(), t_begin.data(), msg_kind, msg_kind ? n_msg.data() : nullptr, d_msgs, slide,
                                        d_world_out, out.data(), &n_done, n_slides);
        out.resize(n_done);
        if (done) *done = out;
        dev_->check(rc);
        return out;
    }

    // KILO.cc:108-233
    bool predictUpdatePoint(double current_time, size_t idx_i, size_t idx_j, const PointCloudType& cloud_down_body,
                            PointCloudType& cloud_down_world, size_t& success_pts_size_out) {
        size_t n = idx_j - idx_i;
        std::vector<float> b, w(3 * n), inten(n);
        for (size_t i = idx_i; i < idx_j; ++i) b.insert(b.end(), {cloud_down_body[i].x, cloud_down_body[i].y, cloud_down_body[i].z});
        size_t before = success_pts_size_out;
        dev_->check(lk_update_points(dev_->h(), current_time, b.data(), n, w.data(), inten.data(), &success_pts_size_out));
        for (size_t i = 0; i < n; ++i) {
            PointType& p = cloud_down_world[idx_i + i];
            p.x = w[3 * i], p.y = w[3 * i + 1], p.z = w[3 * i + 2], p.intensity = inten[i];
        }
        return success_pts_size_out > before;
    }
    bool predictUpdateImu(const lk_imu& imu) {  // KILO.cc:235-258
        dev_->check(lk_update_imu(dev_->h(), &imu));
        return true;
    }
    bool predictUpdateKinImu(const lk_kin_imu& kin) {  // KILO.cc:260-314
        dev_->check(lk_update_kin_imu(dev_->h(), &kin));
        return true;
    }
    // bucket loop of KILO::process (KILO.cc:367-396), fused on the device stream: one call per scan
    bool processSorted(const PointCloudType& sorted_body, double begin_time, const std::vector<lk_imu>& imus,
                       const std::vector<lk_kin_imu>& kins, PointCloudType* world_out, lk_pose* pose) {
        std::vector<lk_point> pts(sorted_body.size());
        for (size_t i = 0; i < pts.size(); ++i) pts[i] = lk_point{sorted_body[i].x, sorted_body[i].y, sorted_body[i].z, sorted_body[i].curvature};
        std::vector<float> w(world_out ? 3 * pts.size() : 0);
        dev_->check(lk_process_scan(dev_->h(), pts.data(), pts.size(), begin_time, imus.data(), imus.size(), kins.data(), kins.size(),
                                    world_out ? w.data() : nullptr, pose));
        if (world_out) {
            world_out->resize(pts.size());
            for (size_t i = 0; i < pts.size(); ++i) (*world_out)[i].x = w[3 * i], (*world_out)[i].y = w[3 * i + 1], (*world_out)[i].z = w[3 * i + 2];
        }
        return true;
    }

    // Many recorded scans at once against the CURRENT map, frozen (lk_batch_replay_scans_dev): scan s runs the bucket
    // loop of KILO::process (KILO.cc:375-395) on filter slot s from its own prior; buckets are the runs of equal curvature
    // of each time-sorted scan (KILO.cc:376-378), t_begin[s] its start time; `imus` (optional, one time-sorted vector per
    // scan) are applied between the buckets as in only_imu_use mode (KILO.cc:379-383), `kins` as in the default leg-fusion
    // mode (KILO.cc:384-390); at most one of the two.  n scans need DeviceCaps::n_slots >= n.
    std::vector<lk_pose> replayRecordedRun(const std::vector<PointCloudType>& sorted_scans, const std::vector<double>& t_begin,
                                           const std::vector<State>& prior_states, const std::vector<StateCov>& prior_covs,
                                           const std::vector<std::vector<lk_imu>>* imus = nullptr,
                                           const std::vector<std::vector<lk_kin_imu>>* kins = nullptr) {
        const size_t S = sorted_scans.size();
        if (t_begin.size() != S || prior_states.size() != S || prior_covs.size() != S || (imus && imus->size() != S) ||
            (kins && kins->size() != S))
            throw std::runtime_error("replayRecordedRun: one start time, prior state and prior covariance per scan");
        if (imus && kins) throw std::runtime_error("replayRecordedRun: IMU messages or kinematic + IMU messages, not both");
        std::vector<lk_kin_imu> kin_flat;
        // the scans go to HBM back to back; their time buckets (runs of equal curvature, KILO.cc:375-378) are found on the device
        std::vector<lk_point> pts;
        std::vector<uint64_t> scan_off(1, 0);
        std::vector<uint32_t> n_msg;
        std::vector<double> x36(S * LK_STATE_DOUBLES), P900(S * DIM_STATE * DIM_STATE);
        std::vector<lk_imu> imu_flat;
        for (size_t s = 0; s < S; ++s) {
            const PointCloudType& sc = sorted_scans[s];
            for (size_t i = 0; i < sc.size(); ++i) pts.push_back(lk_point{sc[i].x, sc[i].y, sc[i].z, sc[i].curvature});
            scan_off.push_back(pts.size());
            prior_states[s].to_x36(&x36[s * LK_STATE_DOUBLES]);
            std::memcpy(&P900[s * DIM_STATE * DIM_STATE], prior_covs[s].d.data(), sizeof(double) * DIM_STATE * DIM_STATE);
            if (imus) {
                n_msg.push_back((uint32_t)(*imus)[s].size());
                imu_flat.insert(imu_flat.end(), (*imus)[s].begin(), (*imus)[s].end());
            }
            if (kins) {
                n_msg.push_back((uint32_t)(*kins)[s].size());
                kin_flat.insert(kin_flat.end(), (*kins)[s].begin(), (*kins)[s].end());
            }
        }
        void* d_pts = nullptr;
        dev_->check(lk_device_malloc(dev_->h(), &d_pts, sizeof(lk_point) * std::max<size_t>(pts.size(), 1)));
        std::vector<lk_pose> out(S);
        int rc = lk_memcpy_h2d(dev_->h(), d_pts, pts.data(), sizeof(lk_point) * pts.size());
        if (!rc) rc = lk_batch_set_priors(dev_->h(), x36.data(), P900.data(), S);
        if (!rc)
            rc = lk_batch_replay_scans_dev(dev_->h(), static_cast<const lk_point*>(d_pts), S, scan_off.data(), t_begin.data(), kins ? 2 : (imus ? 1 : 0),
                                           (imus || kins) ? n_msg.data() : nullptr,
                                           kins ? static_cast<const void*>(kin_flat.data()) : static_cast<const void*>(imu_flat.data()), out.data());
        lk_device_free(dev_->h(), d_pts);
        dev_->check(rc);
        return out;
    }

    // Many equally shaped scans at once WITH the map insert of KILO::process (KILO.cc:216-233 after every bucket): scan s runs the whole
    // bucket loop on filter slot s from its own prior and inserts into its OWN copy-on-write overlay of the current map
    // (lk_batch_replay_overlay_dev); the map itself is not changed.  All scans share their bucket bounds (runs of equal curvature of
    // scan 0, KILO.cc:375-378) and start time.  Per scan the result equals processSorted() on a private copy of the map.
    std::vector<lk_pose> replayWithInsert(const std::vector<PointCloudType>& sorted_scans, double t_begin, const std::vector<State>& prior_states,
                                          const std::vector<StateCov>& prior_covs) {
        const size_t S = sorted_scans.size();
        if (S == 0 || prior_states.size() != S || prior_covs.size() != S) throw std::runtime_error("replayWithInsert: one prior state and covariance per scan");
        const size_t n = sorted_scans[0].size();
        std::vector<uint32_t> off(1, 0);
        std::vector<double> dt;
        for (size_t i = 0; i < n;) {
            size_t j = i + 1;
            while (j < n && sorted_scans[0][i].curvature == sorted_scans[0][j].curvature) ++j;
            dt.push_back((double)sorted_scans[0][i].curvature);
            off.push_back((uint32_t)j);
            i = j;
        }
        std::vector<lk_point> pts;
        pts.reserve(S * n);
        std::vector<double> x36(S * LK_STATE_DOUBLES), P900(S * DIM_STATE * DIM_STATE);
        for (size_t s = 0; s < S; ++s) {
            const PointCloudType& sc = sorted_scans[s];
            if (sc.size() != n) throw std::runtime_error("replayWithInsert: the scans of a batch have one size");
            for (size_t b = 0; b + 1 < off.size(); ++b)
                if (sc[off[b]].curvature != sorted_scans[0][off[b]].curvature || sc[off[b + 1] - 1].curvature != sc[off[b]].curvature)
                    throw std::runtime_error("replayWithInsert: the scans of a batch share their time buckets");
            for (size_t i = 0; i < n; ++i) pts.push_back(lk_point{sc[i].x, sc[i].y, sc[i].z, sc[i].curvature});
            prior_states[s].to_x36(&x36[s * LK_STATE_DOUBLES]);
            std::memcpy(&P900[s * DIM_STATE * DIM_STATE], prior_covs[s].d.data(), sizeof(double) * DIM_STATE * DIM_STATE);
        }
        void* d_pts = nullptr;
        dev_->check(lk_device_malloc(dev_->h(), &d_pts, sizeof(lk_point) * std::max<size_t>(pts.size(), 1)));
        std::vector<lk_pose> out(S);
        int rc = lk_memcpy_h2d(dev_->h(), d_pts, pts.data(), sizeof(lk_point) * pts.size());
        if (!rc) rc = lk_batch_set_priors(dev_->h(), x36.data(), P900.data(), S);
        if (!rc) rc = lk_batch_replay_overlay_dev(dev_->h(), static_cast<const lk_point*>(d_pts), S, n, t_begin, off.data(), dt.data(), dt.size(), out.data());
        lk_device_free(dev_->h(), d_pts);
        dev_->check(rc);
        return out;
    }

    // A recorded run's scans WITH the map insert (lk_batch_replay_overlay_ragged_dev): every scan its own size, its own time buckets (runs of
    // equal curvature, KILO.cc:375-378), its own start time and - optionally - its own IMU (only_imu_use, KILO.cc:379-383) or kinematic + IMU
    // (leg fusion, KILO.cc:384-390) messages between the buckets; each scan inserts into its own copy-on-write overlay of the current map,
    // the map itself is not changed.  Per scan the result equals processSorted() on a private copy of the map.
    std::vector<lk_pose> replayRecordedRunWithInsert(const std::vector<PointCloudType>& sorted_scans, const std::vector<double>& t_begin,
                                                     const std::vector<State>& prior_states, const std::vector<StateCov>& prior_covs,
                                                     const std::vector<std::vector<lk_imu>>* imus = nullptr,
                                                     const std::vector<std::vector<lk_kin_imu>>* kins = nullptr) {
        const size_t S = sorted_scans.size();
        if (S == 0 || t_begin.size() != S || prior_states.size() != S || prior_covs.size() != S || (imus && imus->size() != S) || (kins && kins->size() != S))
            throw std::runtime_error("replayRecordedRunWithInsert: one start time, prior state and prior covariance per scan");
        if (imus && kins) throw std::runtime_error("replayRecordedRunWithInsert: IMU messages or kinematic + IMU messages, not both");
        std::vector<lk_point> pts;
        std::vector<uint64_t> scan_off(1, 0);
        std::vector<uint32_t> n_buckets, bucket_off, n_msg;
        std::vector<double> bucket_dt, x36(S * LK_STATE_DOUBLES), P900(S * DIM_STATE * DIM_STATE);
        std::vector<lk_imu> imu_flat;
        std::vector<lk_kin_imu> kin_flat;
        for (size_t s = 0; s < S; ++s) {
            const PointCloudType& sc = sorted_scans[s];
            if (sc.size() == 0) throw std::runtime_error("replayRecordedRunWithInsert: empty scan");
            uint32_t nb = 0;
            bucket_off.push_back(0);
            for (size_t i = 0; i < sc.size();) {   // KILO.cc:375-378
                size_t j = i + 1;
                while (j < sc.size() && sc[i].curvature == sc[j].curvature) ++j;
                bucket_dt.push_back((double)sc[i].curvature);
                bucket_off.push_back((uint32_t)j);
                ++nb;
                i = j;
            }
            n_buckets.push_back(nb);
            for (size_t i = 0; i < sc.size(); ++i) pts.push_back(lk_point{sc[i].x, sc[i].y, sc[i].z, sc[i].curvature});
            scan_off.push_back(pts.size());
            prior_states[s].to_x36(&x36[s * LK_STATE_DOUBLES]);
            std::memcpy(&P900[s * DIM_STATE * DIM_STATE], prior_covs[s].d.data(), sizeof(double) * DIM_STATE * DIM_STATE);
            if (imus) n_msg.push_back((uint32_t)(*imus)[s].size()), imu_flat.insert(imu_flat.end(), (*imus)[s].begin(), (*imus)[s].end());
            if (kins) n_msg.push_back((uint32_t)(*kins)[s].size()), kin_flat.insert(kin_flat.end(), (*kins)[s].begin(), (*kins)[s].end());
        }
        void* d_pts = nullptr;
        dev_->check(lk_device_malloc(dev_->h(), &d_pts, sizeof(lk_point) * std::max<size_t>(pts.size(), 1)));
        std::vector<lk_pose> out(S);
        int rc = lk_memcpy_h2d(dev_->h(), d_pts, pts.data(), sizeof(lk_point) * pts.size());
        if (!rc) rc = lk_batch_set_priors(dev_->h(), x36.data(), P900.data(), S);
        if (!rc)
            rc = lk_batch_replay_overlay_ragged_dev(dev_->h(), static_cast<const lk_point*>(d_pts), S, scan_off.data(), n_buckets.data(), bucket_off.data(), bucket_dt.data(),
                                                    t_begin.data(), (imus || kins) ? n_msg.data() : nullptr,
                                                    kins ? static_cast<const void*>(kin_flat.data()) : static_cast<const void*>(imu_flat.data()), kins ? 2 : (imus ? 1 : 0),
                                                    out.data());
        lk_device_free(dev_->h(), d_pts);
        dev_->check(rc);
        return out;
    }

   private:
    std::shared_ptr<Device> dev_;
    std::unique_ptr<ESKF> eskf_;
    std::unique_ptr<VoxelMapManager> map_manager_;
};

// Kinematics::Config (kinematics.h) + the callback's `redundancy` flag.  processing() takes serialized unitree_legged_msgs/HighState
// messages (ROS1 serialisation, LK_HIGHSTATE_BYTES each, e.g. the bytes of a recorded /high_state topic) instead of one deserialised
// message, and returns the records of the kept ones (a dropped one yields none): what kinematicImuCallBack pushes into kin_imu_cache_.
// State carried across calls: the four ContactDetectors, the previous message, the last kept stamp (frontend() / setFrontend()).
class Kinematics {
   public:
    struct Config {
        double leg_offset_x;
        double leg_offset_y;
        double leg_calf_length;
        double leg_thigh_length;
        double leg_thigh_offset;
        double contact_force_threshold_up;
        double contact_force_threshold_down;
        bool redundancy = true;
    };

    Kinematics(const Config& config, std::shared_ptr<Device> dev) : dev_(std::move(dev)) {
        lk_kin_config c{config.leg_offset_x, config.leg_offset_y, config.leg_calf_length, config.leg_thigh_length, config.leg_thigh_offset,
                        config.contact_force_threshold_up, config.contact_force_threshold_down, config.redundancy ? 1 : 0, 0};
        dev_->check(lk_kin_configure(dev_->h(), &c));
    }
    std::vector<lk_kin_imu> processing(const void* msgs, size_t n_msgs) {
        std::vector<lk_kin_imu> out(std::max<size_t>(n_msgs, 1));
        size_t n_out = 0;
        dev_->check(lk_decode_highstate(dev_->h(), msgs, n_msgs, out.data(), &n_out));
        out.resize(n_out);
        return out;
    }
    lk_kin_frontend_state frontend() const {
        lk_kin_frontend_state st;
        dev_->check(lk_kin_get_frontend(dev_->h(), &st));
        return st;
    }
    void setFrontend(const lk_kin_frontend_state& st) { dev_->check(lk_kin_set_frontend(dev_->h(), &st)); }
    // syncPackage's kin branch (ros_interface.cc:303-328) over records already in HBM; n_msg[s] = records of packaged scan s
    size_t syncPackages(const lk_kin_imu* d_kins, size_t n_kins, const std::vector<double>& scan_end, std::vector<uint32_t>& n_msg,
                        size_t* n_consumed) {
        n_msg.assign(std::max<size_t>(scan_end.size(), 1), 0);
        size_t n_packaged = 0, consumed = 0;
        dev_->check(lk_kin_split_dev(dev_->h(), d_kins, n_kins, scan_end.data(), scan_end.size(), n_msg.data(), &n_packaged, &consumed));
        n_msg.resize(scan_end.size());
        if (n_consumed) *n_consumed = consumed;
        return n_packaged;
    }

   private:
    std::shared_ptr<Device> dev_;
};

// RosInterface::imuCallBack (ros_interface.cc:194-219) for a batch of serialized sensor_msgs/Imu messages (ROS1 serialisation, message i =
// the bytes [msg_off[i], msg_off[i+1]) of the buffer, e.g. a recorded /imu topic): the records of the kept ones - what the callback pushes
// into imu_cache_.  State carried across calls: the previous message's z values, the last kept stamp (frontend() / setFrontend()).
class ImuFrontend {
   public:
    ImuFrontend(bool redundancy, std::shared_ptr<Device> dev) : dev_(std::move(dev)) { dev_->check(lk_imu_configure(dev_->h(), redundancy ? 1 : 0)); }
    std::vector<lk_imu> processing(const void* msgs, const std::vector<uint64_t>& msg_off) {
        const size_t n = msg_off.empty() ? 0 : msg_off.size() - 1;
        std::vector<lk_imu> out(std::max<size_t>(n, 1));
        size_t n_out = 0;
        dev_->check(lk_decode_imu(dev_->h(), msgs, n, msg_off.data(), out.data(), &n_out));
        out.resize(n_out);
        return out;
    }
    // bytes and records in HBM (d_out: room for one record per message); returns the number kept
    size_t processingDev(const void* d_msgs, const std::vector<uint64_t>& msg_off, lk_imu* d_out) {
        size_t n_out = 0;
        dev_->check(lk_decode_imu_dev(dev_->h(), d_msgs, msg_off.empty() ? 0 : msg_off.size() - 1, msg_off.data(), d_out, &n_out));
        return n_out;
    }
    lk_imu_frontend_state frontend() const {
        lk_imu_frontend_state st;
        dev_->check(lk_imu_get_frontend(dev_->h(), &st));
        return st;
    }
    void setFrontend(const lk_imu_frontend_state& st) { dev_->check(lk_imu_set_frontend(dev_->h(), &st)); }
    // syncPackage's IMU branch (ros_interface.cc:277-301) over records already in HBM; n_msg[s] = records of packaged scan s
    size_t syncPackages(const lk_imu* d_imus, size_t n_imus, const std::vector<double>& scan_end, std::vector<uint32_t>& n_msg, size_t* n_consumed) {
        n_msg.assign(std::max<size_t>(scan_end.size(), 1), 0);
        size_t n_packaged = 0, consumed = 0;
        dev_->check(lk_imu_split_dev(dev_->h(), d_imus, n_imus, scan_end.data(), scan_end.size(), n_msg.data(), &n_packaged, &consumed));
        n_msg.resize(scan_end.size());
        if (n_consumed) *n_consumed = consumed;
        return n_packaged;
    }

   private:
    std::shared_ptr<Device> dev_;
};

// LidarProcessing::Config (lidar_processing.h) + the PointCloud2 point layout its handler reads.  processRun() is the lidar half of a recorded
// run: the payloads of n sensor_msgs/PointCloud2 messages, already in HBM, become what lidarCallBack + LidarProcessing::processing +
// the voxel grid and time sort of KILO.cc:356-370 make of each message - the scans stay in HBM, with the tables
// lk_batch_replay_scans(_kin)_dev and lk_kin_split_dev take.  Refusals (lk_decode_scans_dev) throw, naming the offending message.
class LidarProcessing {
   public:
    struct Config {
        float blind_ = 1.0f;
        int filter_num_ = 1;
        int lidar_type_ = 1;      // common::LidarType: 1 Velodyne, 2 Ouster, 3 Hesai
        double time_scale_ = 1.0;
        lk_cloud_layout layout{}; // point_step and field offsets of the messages (layout.lidar_type is set from lidar_type_)
    };
    // the decoded scans of a run: scan s = data()[scan_off[s], scan_off[s+1]) in HBM, owned (lk_device_free on destruction)
    class DeviceScans {
       public:
        DeviceScans(std::shared_ptr<Device> dev, size_t n_points) : dev_(std::move(dev)) {
            void* p = nullptr;
            dev_->check(lk_device_malloc(dev_->h(), &p, sizeof(lk_point) * std::max<size_t>(n_points, 1)));
            d_ = static_cast<lk_point*>(p);
        }
        ~DeviceScans() {
            if (d_) lk_device_free(dev_->h(), d_);
        }
        DeviceScans(DeviceScans&& o) noexcept
            : scan_off(std::move(o.scan_off)), t_begin(std::move(o.t_begin)), t_end(std::move(o.t_end)), dev_(std::move(o.dev_)), d_(o.d_) {
            o.d_ = nullptr;
        }
        DeviceScans(const DeviceScans&) = delete;
        DeviceScans& operator=(const DeviceScans&) = delete;
        DeviceScans& operator=(DeviceScans&&) = delete;
        lk_point* data() const { return d_; }
        size_t size() const { return scan_off.empty() ? 0 : scan_off.size() - 1; }
        std::vector<uint64_t> scan_off;   // n + 1 entries, first 0
        std::vector<double> t_begin;      // LidarScan::lidar_begin_time_
        std::vector<double> t_end;        // LidarScan::lidar_end_time_ (syncPackage's scan end)

       private:
        std::shared_ptr<Device> dev_;
        lk_point* d_ = nullptr;
    };

    LidarProcessing(const Config& config, std::shared_ptr<Device> dev) : cfg_(config), dev_(std::move(dev)) { cfg_.layout.lidar_type = cfg_.lidar_type_; }
    // message s: n_points[s] points at d_msgs + msg_off[s], header stamp header_stamp[s] (non-decreasing); leaf = voxel_grid_resolution
    DeviceScans processRun(const void* d_msgs, const std::vector<uint64_t>& msg_off, const std::vector<uint32_t>& n_points,
                           const std::vector<double>& header_stamp, float leaf) {
        if (msg_off.size() != n_points.size() || header_stamp.size() != n_points.size()) throw std::invalid_argument("processRun: table sizes differ");
        size_t total = 0;
        for (uint32_t n : n_points) total += n;
        DeviceScans out(dev_, total);
        const size_t n = n_points.size();
        out.scan_off.resize(n + 1), out.t_begin.resize(n), out.t_end.resize(n);
        dev_->check(lk_decode_scans_dev(dev_->h(), d_msgs, n, msg_off.data(), n_points.data(), header_stamp.data(), &cfg_.layout, cfg_.time_scale_,
                                        cfg_.filter_num_, cfg_.blind_, leaf, out.data(), out.scan_off.data(), out.t_begin.data(), out.t_end.data()));
        return out;
    }

   private:
    Config cfg_;
    std::shared_ptr<Device> dev_;
};

}  // namespace LEGKILO_HOST_NAMESPACE
