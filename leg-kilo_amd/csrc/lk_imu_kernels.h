// lk_imu_kernels.h - kernels of the IMU front end (lk_kin.hip): serialised sensor_msgs/Imu messages -> lk_imu records.
//
// Reference: RosInterface::imuCallBack (ros_interface.cc:194-219: the redundancy filter and the time check).  The one piece of sequential
// state - which messages are kept - is a flag per message (linear_acceleration.z and angular_velocity.z against message i - 1), compacted
// by an exclusive sum; the scan split of the IMU branch of syncPackage is lk_kin_kernels.h's, shared.
// ROS1 serialisation of sensor_msgs/Imu, L = frame_id length: seq 0 | stamp.sec 4 | stamp.nsec 8 | L 12 | frame_id 16 | orientation 16+L |
// its covariance 48+L | angular_velocity 120+L | its covariance 144+L | linear_acceleration 216+L | its covariance 240+L | end 312+L.
// One thread per message: a message is ~340 B of which 60 B are read, but every 128-B line of the stream holds a field that is read, so
// each pass is one read of the stream whatever the lanes pick from it; nothing is staged through LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/legkilo_hip.h"

#define LK_IMU_SEC 4
#define LK_IMU_NSEC 8
#define LK_IMU_LEN 12
#define LK_IMU_GYR 120   // + L
#define LK_IMU_ACC 216   // + L

static_assert(sizeof(lk_imu) == 56, "IMU record must be 56 B");

// what the last pass leaves for the host (one read-back per call)
struct LkImuStatus {
    unsigned int n_out;
    unsigned int err;          // 1: a kept stamp is older than the kept one before it
    unsigned int bad;          // n - (index of the first message whose length is not 312 + L); 0: none
    unsigned int pad_;
    double acc_z, gyr_z;       // the last message's, kept or not
    double last_stamp;         // the last kept stamp (the carried one when nothing was kept)
};

// Little-endian fields at any byte address, assembled from the aligned 32-bit words that hold them.  The words reach at most 3 bytes
// before and behind the field; every field read here has at least 4 bytes of its own message on either side (seq in front of sec, a
// covariance behind linear_acceleration), so no word leaves the message.
__device__ __forceinline__ unsigned int lk_ldw_u32(const unsigned char* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned int sh = (unsigned int)(a & 3u) * 8u;
    const unsigned int* w = reinterpret_cast<const unsigned int*>(a - (a & 3u));
    const unsigned int lo = w[0];
    if (sh == 0) return lo;
    return (lo >> sh) | (w[1] << (32u - sh));
}
__device__ __forceinline__ double lk_ldw_f64(const unsigned char* p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned int sh = (unsigned int)(a & 3u) * 8u;
    const unsigned int* w = reinterpret_cast<const unsigned int*>(a - (a & 3u));
    unsigned int lo = w[0], hi = w[1];
    if (sh) {
        const unsigned int top = w[2];
        lo = (lo >> sh) | (hi << (32u - sh));
        hi = (hi >> sh) | (top << (32u - sh));
    }
    return __hiloint2double((int)hi, (int)lo);
}

// Message i lies at msgs + off[i], off[i + 1] - off[i] >= 312 bytes long (checked on the host).  Its frame_id length is read from bytes
// 12 .. 15; the message is valid when its length is 312 + L in 64 bits - only then is anything behind byte 16 looked at.
__device__ __forceinline__ bool lk_imu_msg_valid(const unsigned char* __restrict__ msgs, const unsigned long long* __restrict__ off, unsigned int i,
                                                 const unsigned char** body) {
    const unsigned long long o = off[i];
    const unsigned long long L = lk_ldw_u32(msgs + o + LK_IMU_LEN);
    *body = msgs + o + L;   // field at body + its offset for L = 0 (only dereferenced when valid)
    return off[i + 1] - o == (unsigned long long)LK_IMU_MSG_FIXED_BYTES + L;
}

// Pass 1: the keep flag (imuCallBack's redundancy test, fp64 == against message i - 1 whether that one was kept or not; message 0 against the
// carried values).  A message whose length disagrees with its L is reported (st->bad) and not kept, so the later passes never read it.
__global__ void __launch_bounds__(256)
    lk_imu_fe_flags_kernel(const unsigned char* __restrict__ msgs, const unsigned long long* __restrict__ off, unsigned int n, double prev_acc_z,
                           double prev_gyr_z, int redundancy, unsigned int* __restrict__ keep, LkImuStatus* __restrict__ st) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char* m;
    if (!lk_imu_msg_valid(msgs, off, i, &m)) {
        atomicMax(&st->bad, n - i);
        keep[i] = 0u;
        return;
    }
    bool k = true;
    if (redundancy) {
        double pa = prev_acc_z, pg = prev_gyr_z;
        bool have_prev = true;
        if (i > 0) {
            const unsigned char* q;
            have_prev = lk_imu_msg_valid(msgs, off, i - 1, &q);   // (an invalid neighbour fails the call: this flag is then never used)
            if (have_prev) pa = lk_ldw_f64(q + LK_IMU_ACC + 16), pg = lk_ldw_f64(q + LK_IMU_GYR + 16);
        }
        if (have_prev) k = !(lk_ldw_f64(m + LK_IMU_ACC + 16) == pa && lk_ldw_f64(m + LK_IMU_GYR + 16) == pg);
    }
    keep[i] = k ? 1u : 0u;
}

// Pass 2: a kept message's record at its compacted index: stamp (ros::Time::toSec), acc = linear_acceleration, gyr = angular_velocity.
__global__ void __launch_bounds__(256)
    lk_imu_fe_scatter_kernel(const unsigned char* __restrict__ msgs, const unsigned long long* __restrict__ off, unsigned int n,
                             const unsigned int* __restrict__ keep, const unsigned int* __restrict__ rank, lk_imu* __restrict__ out) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const unsigned long long o = off[i];
    const unsigned char* m = msgs + o + (off[i + 1] - o - LK_IMU_MSG_FIXED_BYTES);   // kept: valid, so the length says L
    lk_imu r;
    r.stamp = (double)lk_ldw_u32(msgs + o + LK_IMU_SEC) + 1e-9 * (double)lk_ldw_u32(msgs + o + LK_IMU_NSEC);
    for (int k = 0; k < 3; ++k) {
        r.acc[k] = lk_ldw_f64(m + LK_IMU_ACC + 8 * k);
        r.gyr[k] = lk_ldw_f64(m + LK_IMU_GYR + 8 * k);
    }
    out[rank[i]] = r;
}

// Pass 3: the kept stamps must not go backwards (the reference's callback clears its cache there, ros_interface.cc:209-212: refused here),
// within the call and against the carried last stamp; block 0 / thread 0 also fills the status the host reads back.
__global__ void __launch_bounds__(256)
    lk_imu_fe_finish_kernel(const unsigned char* __restrict__ msgs, const unsigned long long* __restrict__ off, unsigned int n, double last_stamp,
                            const unsigned int* __restrict__ keep, const unsigned int* __restrict__ rank, const lk_imu* __restrict__ out,
                            LkImuStatus* __restrict__ st) {
    const unsigned int n_out = rank[n - 1] + keep[n - 1];
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_out) {
        const double prev = k ? out[k - 1].stamp : last_stamp;
        if (out[k].stamp < prev) atomicOr(&st->err, 1u);
    }
    if (k == 0) {
        st->n_out = n_out;
        const unsigned char* m;
        const bool ok = lk_imu_msg_valid(msgs, off, n - 1, &m);
        st->acc_z = ok ? lk_ldw_f64(m + LK_IMU_ACC + 16) : 0.0;
        st->gyr_z = ok ? lk_ldw_f64(m + LK_IMU_GYR + 16) : 0.0;
        st->last_stamp = n_out ? out[n_out - 1].stamp : last_stamp;
    }
}
