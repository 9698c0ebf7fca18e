// lk_kin_kernels.h - kernels of the leg kinematics front end (lk_kin.hip): unitree_legged_msgs/HighState messages -> lk_kin_imu records.
//
// Reference: RosInterface::kinematicImuCallBack (ros_interface.cc:221-248: the redundancy filter and the time check), Kinematics::processing
// (kinematics.cc:5-90: leg reorder, ContactDetector of kinematics.h, forward kinematics + Jacobian foot velocity) and the kin branch of
// RosInterface::syncPackage (ros_interface.cc:303-328).  Both sequential pieces of state become scans:
//   - which messages are kept: a flag per message (acc z and gyr z against message i-1), compacted by an exclusive sum;
//   - the contact detector of each leg: a transition map {0,1} -> {0,1} per message (identity for a dropped one), composed by an inclusive scan
//     (lk_prim_compose_scan); the scanned map applied to the carried state is the leg's contact after that message.
// HighState's ROS1 serialisation has a fixed size (every array has a fixed length); the byte offsets read here follow the field order of
// unitree_legged_msgs/msg/{HighState,IMU,MotorState,BmsState}.msg: stamp 0 | head 8 | levelFlag 10 | frameReserve 11 | SN 12 | version 20 |
// bandWidth 28 | imu 30 (quaternion 30, gyroscope 46, accelerometer 58, rpy 70, temperature 82) | motorState[20] 83 (38 B each: mode, q +1,
// dq +5, ...) | bms 843 (34 B) | footForce 877 | ... | crc 1091.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/legkilo_hip.h"

#define LK_HS_SEC 0
#define LK_HS_NSEC 4
#define LK_HS_GYR 46
#define LK_HS_ACC 58
#define LK_HS_Q0 84       // motorState[k].q at LK_HS_Q0 + LK_HS_MOTOR * k, dq 4 bytes behind
#define LK_HS_MOTOR 38
#define LK_HS_FORCE 877
#define LK_KIN_IDENTITY 0xAAu   // the identity map of all four legs (state 0 -> 0, 1 -> 1)
#define LK_KIN_MSGS_PER_BLOCK 32   // messages one scatter workgroup stages into LDS (4 lanes each: 128 threads, 35 KB)

static_assert(LK_HIGHSTATE_BYTES == 1095, "HighState serialisation size");
static_assert(sizeof(lk_kin_imu) == 264, "kinematic record must be 264 B");

// what the last pass leaves for the host (one read-back per call)
struct LkKinStatus {
    unsigned int n_out;
    unsigned int err;          // 1: a kept stamp is older than the kept one before it
    int contact[4];            // detector state after the last message
    float acc_z, gyr_z;        // the last message's, kept or not
    double last_stamp;         // the last kept stamp (the carried one when nothing was kept)
};

// little-endian fields at any byte address (global memory or LDS)
__device__ __forceinline__ unsigned int lk_ld_u32(const unsigned char* p) {
    return (unsigned int)p[0] | ((unsigned int)p[1] << 8) | ((unsigned int)p[2] << 16) | ((unsigned int)p[3] << 24);
}
__device__ __forceinline__ float lk_ld_f32(const unsigned char* p) { return __uint_as_float(lk_ld_u32(p)); }
__device__ __forceinline__ int lk_ld_i16(const unsigned char* p) { return (int)(short)((unsigned int)p[0] | ((unsigned int)p[1] << 8)); }

// ContactDetector::update (kinematics.h) as a map: state 0 -> (f > T_on), state 1 -> !(f < T_off); bits 2j / 2j+1 of leg j.
// Project leg j (FR FL RR RL) reads Unitree foot j ^ 1 (FL FR RL RR): kinematics.cc:20-23.
__device__ __forceinline__ unsigned int lk_contact_maps(const unsigned char* msg, double t_on, double t_off) {
    unsigned int m = 0;
    for (int j = 0; j < 4; ++j) {
        const double f = (double)lk_ld_i16(msg + LK_HS_FORCE + 2 * (j ^ 1));
        m |= (unsigned int)(f > t_on) << (2 * j);
        m |= (unsigned int)!(f < t_off) << (2 * j + 1);
    }
    return m;
}

// Pass 1, one thread per message: keep flag (kinematicImuCallBack's redundancy test, float == against message i - 1 whether that one was kept
// or not; message 0 against the carried values) and the four detectors' transition maps (identity for a dropped message).
__global__ void __launch_bounds__(256)
    lk_kin_flags_kernel(const unsigned char* __restrict__ msgs, unsigned int n, float prev_acc_z, float prev_gyr_z, int redundancy, double t_on,
                        double t_off, unsigned int* __restrict__ keep, unsigned char* __restrict__ maps) {
    const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned char* m = msgs + (size_t)i * LK_HIGHSTATE_BYTES;
    bool k = true;
    if (redundancy) {
        const float az = lk_ld_f32(m + LK_HS_ACC + 8), gz = lk_ld_f32(m + LK_HS_GYR + 8);
        float pa = prev_acc_z, pg = prev_gyr_z;
        if (i > 0) {
            pa = lk_ld_f32(m - LK_HIGHSTATE_BYTES + LK_HS_ACC + 8);
            pg = lk_ld_f32(m - LK_HIGHSTATE_BYTES + LK_HS_GYR + 8);
        }
        k = !(az == pa && gz == pg);
    }
    keep[i] = k ? 1u : 0u;
    maps[i] = (unsigned char)(k ? lk_contact_maps(m, t_on, t_off) : LK_KIN_IDENTITY);
}

// Kinematics::caculateFootPosVel (kinematics.cc:54-90) for project leg j, fp64, the reference's operation order
__device__ __forceinline__ void lk_foot_pos_vel(int j, const double q[3], const double dq[3], const lk_kin_config& c, double pos[3], double vel[3]) {
    const int lfoot = (j == 0 || j == 2) ? 1 : -1, ffoot = j < 2 ? 1 : -1;
    const double lt = c.leg_thigh_length, lc = c.leg_calf_length, d = c.leg_thigh_offset, ox = c.leg_offset_x, oy = c.leg_offset_y;
    const double s1 = sin(q[0]), s2 = sin(q[1]), s23 = sin(q[1] + q[2]);
    const double c1 = cos(q[0]), c2 = cos(q[1]), c23 = cos(q[1] + q[2]);
    pos[0] = -lt * s2 - lc * s23 + ffoot * ox;
    pos[1] = lfoot * d * c1 + lc * s1 * c23 + lt * c2 * s1 + lfoot * oy;
    pos[2] = lfoot * d * s1 - lc * c1 * c23 - lt * c1 * c2;
    const double j01 = -lc * c23 - lt * c2, j02 = -lc * c23;
    const double j10 = lt * c1 * c2 - lfoot * d * s1 + lc * c1 * c23, j11 = -s1 * (lc * s23 + lt * s2), j12 = -lc * s23 * s1;
    const double j20 = lt * c2 * s1 + lfoot * d * c1 + lc * s1 * c23, j21 = c1 * (lc * s23 + lt * s2), j22 = lc * s23 * c1;
    vel[0] = j01 * dq[1] + j02 * dq[2];
    vel[1] = j10 * dq[0] + j11 * dq[1] + j12 * dq[2];
    vel[2] = j20 * dq[0] + j21 * dq[1] + j22 * dq[2];
}

// Pass 2: a workgroup stages the contiguous bytes of LK_KIN_MSGS_PER_BLOCK messages into LDS with 16-byte loads (the 1095-byte stride leaves
// every field unaligned; only bytes of these messages are read: a ragged head and tail go byte by byte), then 4 lanes per message - one per
// leg - write the kept message's record at its compacted index: stamp (ros::Time::toSec), acc / gyr, contact = scanned map applied to the
// carried state, foot position / velocity.
__global__ void __launch_bounds__(4 * LK_KIN_MSGS_PER_BLOCK)
    lk_kin_scatter_kernel(const unsigned char* __restrict__ msgs, unsigned int n, lk_kin_config cfg, int4 contact0, const unsigned int* __restrict__ keep,
                          const unsigned int* __restrict__ rank, const unsigned char* __restrict__ cmaps, lk_kin_imu* __restrict__ out) {
    __shared__ uint4 lds4[(LK_KIN_MSGS_PER_BLOCK * LK_HIGHSTATE_BYTES + 16 + 15) / 16];
    unsigned char* lds = reinterpret_cast<unsigned char*>(lds4);
    const unsigned int m0 = blockIdx.x * LK_KIN_MSGS_PER_BLOCK;
    const unsigned int nm = min((unsigned int)LK_KIN_MSGS_PER_BLOCK, n - m0);
    const unsigned char* g0 = msgs + (size_t)m0 * LK_HIGHSTATE_BYTES;
    const unsigned int len = nm * LK_HIGHSTATE_BYTES;
    // lds[sh + k] = g0[k]; 16-byte chunk c of LDS = bytes [al + 16c, al + 16c + 16) of global memory, loaded whole only when inside [g0, g0 + len)
    const unsigned int sh = (unsigned int)(reinterpret_cast<uintptr_t>(g0) & 15u);
    const uint4* al = reinterpret_cast<const uint4*>(g0 - sh);
    const unsigned int c0 = sh ? 1u : 0u, c1 = (sh + len) / 16u;
    const unsigned int head_end = min(len, 16u * c0 - sh);
    const unsigned int tail_start = c1 > c0 ? max(head_end, 16u * c1 - sh) : head_end;
    for (unsigned int c = c0 + threadIdx.x; c < c1; c += blockDim.x) lds4[c] = al[c];
    for (unsigned int k = threadIdx.x; k < head_end; k += blockDim.x) lds[sh + k] = g0[k];
    for (unsigned int k = tail_start + threadIdx.x; k < len; k += blockDim.x) lds[sh + k] = g0[k];
    __syncthreads();
    const unsigned int ml = threadIdx.x >> 2, j = threadIdx.x & 3u;
    if (ml >= nm) return;
    const unsigned int i = m0 + ml;
    if (!keep[i]) return;
    const unsigned char* m = lds + sh + ml * LK_HIGHSTATE_BYTES;
    lk_kin_imu* r = out + rank[i];
    const int u = (int)(j ^ 1u);   // Unitree leg of project leg j: motors 3u .. 3u + 2 (kinematics.cc:28-37)
    double q[3], dq[3];
    for (int k = 0; k < 3; ++k) {
        q[k] = (double)lk_ld_f32(m + LK_HS_Q0 + LK_HS_MOTOR * (3 * u + k));
        dq[k] = (double)lk_ld_f32(m + LK_HS_Q0 + 4 + LK_HS_MOTOR * (3 * u + k));
    }
    double pos[3], vel[3];
    lk_foot_pos_vel((int)j, q, dq, cfg, pos, vel);
    for (int k = 0; k < 3; ++k) {
        r->foot_pos[j][k] = pos[k];
        r->foot_vel[j][k] = vel[k];
    }
    const int c_in = j == 0 ? contact0.x : j == 1 ? contact0.y : j == 2 ? contact0.z : contact0.w;
    r->contact[j] = (int32_t)((cmaps[i] >> (2 * j + (c_in ? 1 : 0))) & 1u);
    if (j == 0) {
        r->time_stamp = (double)lk_ld_u32(m + LK_HS_SEC) + 1e-9 * (double)lk_ld_u32(m + LK_HS_NSEC);
        for (int k = 0; k < 3; ++k) {
            r->acc[k] = (double)lk_ld_f32(m + LK_HS_ACC + 4 * k);
            r->gyr[k] = (double)lk_ld_f32(m + LK_HS_GYR + 4 * k);
        }
    }
}

// Pass 3: the kept stamps must not go backwards (the reference's callback clears its cache there, ros_interface.cc:232-235: refused here),
// within the call and against the carried last stamp; block 0 / thread 0 also fills the status the host reads back.
__global__ void __launch_bounds__(256)
    lk_kin_finish_kernel(const unsigned char* __restrict__ msgs, unsigned int n, double last_stamp, int4 contact0, const unsigned int* __restrict__ keep,
                         const unsigned int* __restrict__ rank, const unsigned char* __restrict__ cmaps, const lk_kin_imu* __restrict__ out,
                         LkKinStatus* __restrict__ st) {
    const unsigned int n_out = rank[n - 1] + keep[n - 1];
    const unsigned int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n_out) {
        const double prev = k ? out[k - 1].time_stamp : last_stamp;
        if (out[k].time_stamp < prev) atomicOr(&st->err, 1u);
    }
    if (k == 0) {
        st->n_out = n_out;
        const unsigned int cm = cmaps[n - 1];
        const int c[4] = {contact0.x, contact0.y, contact0.z, contact0.w};
        for (int j = 0; j < 4; ++j) st->contact[j] = (int)((cm >> (2 * j + (c[j] ? 1 : 0))) & 1u);
        const unsigned char* m = msgs + (size_t)(n - 1) * LK_HIGHSTATE_BYTES;
        st->acc_z = lk_ld_f32(m + LK_HS_ACC + 8);
        st->gyr_z = lk_ld_f32(m + LK_HS_GYR + 8);
        st->last_stamp = n_out ? out[n_out - 1].time_stamp : last_stamp;
    }
}

// ---- scan split (syncPackage: the kin branch, ros_interface.cc:303-328, and the IMU branch, :277-301 - one rule) ----
// One thread per scan: lb[s] = first record stamped >= scan_end[s] (n when none), eq[s] = that record is stamped exactly scan_end[s].
// A record is `stride` bytes and starts with its stamp (lk_kin_imu::time_stamp, lk_imu::stamp).
__device__ __forceinline__ double lk_rec_stamp(const unsigned char* __restrict__ recs, unsigned int stride, unsigned int i) {
    return *reinterpret_cast<const double*>(recs + (size_t)i * stride);
}
__global__ void __launch_bounds__(256)
    lk_kin_lb_kernel(const unsigned char* __restrict__ recs, unsigned int stride, unsigned int n, const double* __restrict__ ends, unsigned int S,
                     unsigned int* __restrict__ lb, unsigned char* __restrict__ eq) {
    const unsigned int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    const double e = ends[s];
    unsigned int lo = 0, hi = n;
    while (lo < hi) {
        const unsigned int mid = (lo + hi) >> 1;
        if (lk_rec_stamp(recs, stride, mid) < e) lo = mid + 1;
        else hi = mid;
    }
    lb[s] = lo;
    eq[s] = (unsigned char)(lo < n && lk_rec_stamp(recs, stride, lo) == e);
}

// One wave carries the cursor over all scans: cursor_s = cursor_{s-1} < lb_s ? lb_s + eq_s : cursor_{s-1}.  With d_s = cursor_s - lb_s (always 0 or
// 1) and delta_s = lb_s - lb_{s-1} the step is a map of d on {0, 1} - delta >= 2: d -> eq; delta 1: 0 -> eq, 1 -> 0; delta 0: d -> d - so 64 scans
// at a time go through a wave-wide scan of 2-bit maps (the contact detectors' trick again).  A scan is packaged while lb_s < n (the newest record
// is >= its end time) and cursor_{s-1} < n (syncPackage returns false on an empty cache); packaging stops at the first scan that is not.
// out: n_msg[s] for the packaged scans; st[0] = packaged scans, st[1] = consumed records.
__global__ void __launch_bounds__(LK_WAVE)
    lk_kin_split_kernel(const unsigned int* __restrict__ lb, const unsigned char* __restrict__ eq, unsigned int S, unsigned int n,
                        unsigned int* __restrict__ n_msg, unsigned int* __restrict__ st) {
    const int lane = threadIdx.x;
    unsigned int d_carry = 0, lb_carry = 0;   // d and lb of the scan before the chunk (cursor 0 before the first scan)
    unsigned int packaged = S, consumed = 0;
    for (unsigned int base = 0; base < S; base += LK_WAVE) {
        const unsigned int s = base + lane;
        const bool live = s < S;
        const unsigned int l = live ? lb[s] : n;
        const unsigned int e = live ? eq[s] : 0u;
        unsigned int l_prev = __shfl_up(l, 1);
        if (lane == 0) l_prev = lb_carry;
        const unsigned int delta = l - l_prev;
        unsigned int f = delta >= 2 ? (e | (e << 1)) : delta == 1 ? e : 2u;   // bit0 = image of 0, bit1 = image of 1
        for (int off = 1; off < LK_WAVE; off <<= 1) {   // inclusive scan: f = f_s o ... o f_base
            const unsigned int g = __shfl_up(f, off);
            if (lane >= off) f = (((f >> (g & 1u)) & 1u)) | (((f >> ((g >> 1) & 1u)) & 1u) << 1);
        }
        const unsigned int d = (f >> d_carry) & 1u;
        const unsigned int cur = l + d;
        unsigned int cur_prev = __shfl_up(cur, 1);
        if (lane == 0) cur_prev = lb_carry + d_carry;
        const bool pk = live && l < n && cur_prev < n;
        const unsigned long long stop = __ballot(!pk);
        const int first = stop ? __ffsll((long long)stop) - 1 : LK_WAVE;
        if (pk && lane < first) n_msg[s] = cur - cur_prev;
        if (stop) {
            packaged = base + (unsigned int)first;
            const unsigned int c_first = __shfl(cur_prev, first);   // cursor after the last packaged scan
            consumed = c_first;
            break;
        }
        d_carry = __shfl(d, LK_WAVE - 1);
        lb_carry = __shfl(l, LK_WAVE - 1);
        consumed = lb_carry + d_carry;
    }
    if (lane == 0) {
        st[0] = packaged;
        st[1] = packaged ? consumed : 0u;
    }
}
