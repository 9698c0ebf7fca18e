// lk_kin.hip - the message front-end unit of liblegkilo_hip.so (see lk_internal.h): unitree_legged_msgs/HighState messages -> lk_kin_imu records
// (lk_kin_kernels.h) and sensor_msgs/Imu messages -> lk_imu records (lk_imu_kernels.h) on the device, the branch of syncPackage that hands either
// kind to the scans, and the C-ABI entries around them.
#define LK_TU_KIN 1
#include "lk_internal.h"
#include "lk_kin_kernels.h"
#include "lk_imu_kernels.h"

static_assert(sizeof(lk_kin_config) == 64, "lk_kin_config must be 64 B");
static_assert(sizeof(lk_kin_frontend_state) == 32, "lk_kin_frontend_state must be 32 B");
static_assert(sizeof(lk_imu_frontend_state) == 24, "lk_imu_frontend_state must be 24 B");
static_assert(offsetof(lk_kin_imu, time_stamp) == 0 && offsetof(lk_imu, stamp) == 0, "the scan split reads a record's first double as its stamp");

// flags -> two scans -> scatter -> check; the carried state moves only when the call succeeds
static int kin_decode(lk_handle* h, const unsigned char* d_msgs, size_t n_sz, lk_kin_imu* d_out, size_t* n_out) {
    const unsigned int n = (unsigned int)n_sz;
    unsigned int *keep = nullptr, *rank = nullptr;
    unsigned char *maps = nullptr, *cmaps = nullptr;   // transition maps, their scan
    LkKinStatus* st = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        keep = c.take<unsigned int>(n_sz), rank = c.take<unsigned int>(n_sz);
        maps = c.take<unsigned char>(n_sz), cmaps = c.take<unsigned char>(n_sz);
        st = c.take<LkKinStatus>(1);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->kin, bytes, bytes / 4));
    carve(h->kin.p);
    size_t b0 = 0, b1 = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, b0, keep, rank, n_sz, h->stream));
    HIPCHK(h, lk_prim_compose_scan(nullptr, b1, maps, cmaps, n_sz, h->stream));
    size_t tb = std::max(b0, b1);
    LKCHK(reserve(h, h->prim_tmp, tb));
    const lk_kin_config& c = h->kin_cfg;
    const lk_kin_frontend_state& fe = h->kin_fe;
    const int4 c0 = make_int4(fe.contact[0], fe.contact[1], fe.contact[2], fe.contact[3]);
    HIPCHK(h, hipMemsetAsync(st, 0, sizeof(LkKinStatus), h->stream));
    const unsigned int nb = (n + 255) / 256;
    LAUNCH(h, "kin_flags", hipLaunchKernelGGL(lk_kin_flags_kernel, dim3(nb), dim3(256), 0, h->stream, d_msgs, n, fe.last_acc_z, fe.last_gyr_z,
                                              c.redundancy ? 1 : 0, c.contact_force_threshold_up, c.contact_force_threshold_down, keep, maps));
    size_t t0 = tb, t1 = tb;
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, t0, keep, rank, n_sz, h->stream));
    HIPCHK(h, lk_prim_compose_scan(h->prim_tmp.p, t1, maps, cmaps, n_sz, h->stream));
    const unsigned int ns = (n + LK_KIN_MSGS_PER_BLOCK - 1) / LK_KIN_MSGS_PER_BLOCK;
    LAUNCH(h, "kin_scatter", hipLaunchKernelGGL(lk_kin_scatter_kernel, dim3(ns), dim3(4 * LK_KIN_MSGS_PER_BLOCK), 0, h->stream, d_msgs, n, c, c0, keep,
                                                rank, cmaps, d_out));
    LAUNCH(h, "kin_finish", hipLaunchKernelGGL(lk_kin_finish_kernel, dim3(nb), dim3(256), 0, h->stream, d_msgs, n, fe.last_stamp, c0, keep, rank,
                                               cmaps, d_out, st));
    LkKinStatus hs;
    HIPCHK(h, hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hs.err) return fail(h, LK_ERR_INVALID, "HighState stamps go backwards (a kept message is older than the kept one before it); the front end keeps its state");
    for (int j = 0; j < 4; ++j) h->kin_fe.contact[j] = hs.contact[j];
    h->kin_fe.last_acc_z = hs.acc_z;
    h->kin_fe.last_gyr_z = hs.gyr_z;
    h->kin_fe.last_stamp = hs.last_stamp;
    *n_out = hs.n_out;
    return LK_OK;
}

// syncPackage's message branch over time-sorted records of `stride` bytes that start with their stamp: lk_kin_split_dev, lk_imu_split_dev
static int split_records(lk_handle* h, const void* d_recs, size_t stride, size_t n_recs, const double* scan_end, size_t n_scans, uint32_t* n_msg,
                         size_t* n_packaged, size_t* n_consumed) {
    if (!n_packaged || !n_consumed || (n_scans && (!scan_end || !n_msg)) || (n_recs && !d_recs)) return fail(h, LK_ERR_INVALID, "null argument");
    if (n_recs >= ((size_t)1 << 31) || n_scans >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "more than 2^31 records or scans");
    for (size_t s = 0; s < n_scans; ++s) {
        if (scan_end[s] != scan_end[s]) return fail(h, LK_ERR_INVALID, "scan end time is NaN");
        if (s && scan_end[s] < scan_end[s - 1]) return fail(h, LK_ERR_INVALID, "scan end times must be non-decreasing");
    }
    *n_packaged = 0;
    *n_consumed = 0;
    for (size_t s = 0; s < n_scans; ++s) n_msg[s] = 0;
    if (n_scans == 0 || n_recs == 0) return LK_OK;   // an empty cache packages nothing (ros_interface.cc:307)
    const unsigned int S = (unsigned int)n_scans, n = (unsigned int)n_recs;
    double* ends = nullptr;
    unsigned int *lb = nullptr, *nm = nullptr, *st = nullptr;
    unsigned char* eq = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        ends = c.take<double>(n_scans);
        lb = c.take<unsigned int>(n_scans), nm = c.take<unsigned int>(n_scans);   // lower bounds, messages per scan
        eq = c.take<unsigned char>(n_scans);
        st = c.take<unsigned int>(2);   // scans packaged, records consumed
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->kin, bytes, bytes / 4));
    carve(h->kin.p);
    HIPCHK(h, hipMemcpyAsync(ends, scan_end, 8 * n_scans, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "kin_lb", hipLaunchKernelGGL(lk_kin_lb_kernel, dim3((S + 255) / 256), dim3(256), 0, h->stream, static_cast<const unsigned char*>(d_recs), (unsigned int)stride, n, ends, S, lb, eq));
    LAUNCH(h, "kin_split", hipLaunchKernelGGL(lk_kin_split_kernel, dim3(1), dim3(LK_WAVE), 0, h->stream, lb, eq, S, n, nm, st));
    unsigned int hs[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(hs, st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (hs[0]) {
        HIPCHK(h, hipMemcpyAsync(n_msg, nm, 4 * (size_t)hs[0], hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    *n_packaged = hs[0];
    *n_consumed = hs[1];
    return LK_OK;
}

// flags -> scan -> scatter -> check, as kin_decode; d_first = byte msg_off[0] of the caller's buffer, the offsets go to the device relative to it
static int imu_decode(lk_handle* h, const unsigned char* d_first, size_t n_sz, const uint64_t* msg_off, lk_imu* d_out, size_t* n_out) {
    const unsigned int n = (unsigned int)n_sz;
    unsigned long long* off = nullptr;
    unsigned int *keep = nullptr, *rank = nullptr;
    LkImuStatus* st = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        off = c.take<unsigned long long>(n_sz + 1);
        keep = c.take<unsigned int>(n_sz), rank = c.take<unsigned int>(n_sz);
        st = c.take<LkImuStatus>(1);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->imu, bytes, bytes / 4));
    carve(h->imu.p);
    size_t tb = 0;
    HIPCHK(h, lk_prim_exclusive_scan(nullptr, tb, keep, rank, n_sz, h->stream));
    LKCHK(reserve(h, h->prim_tmp, tb));
    std::vector<unsigned long long> rel(n_sz + 1);
    for (size_t i = 0; i <= n_sz; ++i) rel[i] = msg_off[i] - msg_off[0];
    HIPCHK(h, hipMemcpyAsync(off, rel.data(), 8 * (n_sz + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(st, 0, sizeof(LkImuStatus), h->stream));
    const lk_imu_frontend_state& fe = h->imu_fe;
    const unsigned int nb = (n + 255) / 256;
    LAUNCH(h, "imu_fe_flags", hipLaunchKernelGGL(lk_imu_fe_flags_kernel, dim3(nb), dim3(256), 0, h->stream, d_first, off, n, fe.last_acc_z, fe.last_gyr_z,
                                                 h->imu_redundancy ? 1 : 0, keep, st));
    HIPCHK(h, lk_prim_exclusive_scan(h->prim_tmp.p, tb, keep, rank, n_sz, h->stream));
    LAUNCH(h, "imu_fe_scatter", hipLaunchKernelGGL(lk_imu_fe_scatter_kernel, dim3(nb), dim3(256), 0, h->stream, d_first, off, n, keep, rank, d_out));
    LAUNCH(h, "imu_fe_finish", hipLaunchKernelGGL(lk_imu_fe_finish_kernel, dim3(nb), dim3(256), 0, h->stream, d_first, off, n, fe.last_stamp, keep, rank,
                                                  d_out, st));
    LkImuStatus hs;
    HIPCHK(h, hipMemcpyAsync(&hs, st, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (`rel` has been read by now)
    if (hs.bad) {
        const size_t i = n_sz - hs.bad;
        return fail(h, LK_ERR_INVALID, "Imu message " + std::to_string(i) + ": its length of " + std::to_string(msg_off[i + 1] - msg_off[i]) +
                                           " bytes is not 312 + its frame_id length; the front end keeps its state");
    }
    if (hs.err) return fail(h, LK_ERR_INVALID, "Imu stamps go backwards (a kept message is older than the kept one before it); the front end keeps its state");
    h->imu_fe.last_acc_z = hs.acc_z;
    h->imu_fe.last_gyr_z = hs.gyr_z;
    h->imu_fe.last_stamp = hs.last_stamp;
    *n_out = hs.n_out;
    return LK_OK;
}

// what both Imu decode entries refuse before anything runs; *n_out = 0
static int imu_decode_check(lk_handle* h, const void* msgs, size_t n, const uint64_t* msg_off, const void* out, size_t* n_out) {
    if (!n_out || (n && (!msgs || !out || !msg_off))) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->imu_configured) return fail(h, LK_ERR_STATE, "the IMU front end is not configured (lk_imu_configure)");
    if (n >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "more than 2^31 messages in one call");
    *n_out = 0;
    for (size_t i = 0; i < n; ++i) {
        if (msg_off[i + 1] < msg_off[i]) return fail(h, LK_ERR_INVALID, "Imu message " + std::to_string(i) + ": msg_off decreases");
        if (msg_off[i + 1] - msg_off[i] < (uint64_t)LK_IMU_MSG_FIXED_BYTES)
            return fail(h, LK_ERR_INVALID, "Imu message " + std::to_string(i) + ": shorter than the 312 fixed bytes of a sensor_msgs/Imu");
    }
    return LK_OK;
}

static void kin_reset_frontend(lk_handle* h) {
    for (int j = 0; j < 4; ++j) h->kin_fe.contact[j] = 1;   // ContactDetector::in_contact_{true}
    h->kin_fe.last_acc_z = 0.0f;                            // the callback's zero-initialised static message
    h->kin_fe.last_gyr_z = 0.0f;
    h->kin_fe.last_stamp = -HUGE_VAL;
}

extern "C" {

int lk_kin_configure(lk_handle* h, const lk_kin_config* cfg) {
    CHECK_H(h);
    if (!cfg) return fail(h, LK_ERR_INVALID, "null argument");
    h->kin_cfg = *cfg;
    h->kin_cfg.pad_ = 0;
    h->kin_configured = true;
    kin_reset_frontend(h);
    return LK_OK;
}

int lk_kin_get_frontend(lk_handle* h, lk_kin_frontend_state* st) {
    CHECK_H(h);
    if (!st) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->kin_configured) return fail(h, LK_ERR_STATE, "the kinematics front end is not configured (lk_kin_configure)");
    *st = h->kin_fe;
    return LK_OK;
}

int lk_kin_set_frontend(lk_handle* h, const lk_kin_frontend_state* st) {
    CHECK_H(h);
    if (!st) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->kin_configured) return fail(h, LK_ERR_STATE, "the kinematics front end is not configured (lk_kin_configure)");
    for (int j = 0; j < 4; ++j)
        if (st->contact[j] != 0 && st->contact[j] != 1) return fail(h, LK_ERR_INVALID, "contact states must be 0 or 1");
    h->kin_fe = *st;
    return LK_OK;
}

int lk_decode_highstate_dev(lk_handle* h, const void* d_msgs, size_t n, lk_kin_imu* d_out, size_t* n_out) {
    CHECK_H(h);
    if (!n_out || (n && (!d_msgs || !d_out))) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->kin_configured) return fail(h, LK_ERR_STATE, "the kinematics front end is not configured (lk_kin_configure)");
    if (n >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "more than 2^31 messages in one call");
    *n_out = 0;
    if (n == 0) return LK_OK;
    return kin_decode(h, static_cast<const unsigned char*>(d_msgs), n, d_out, n_out);
}

int lk_decode_highstate(lk_handle* h, const void* msgs, size_t n, lk_kin_imu* out, size_t* n_out) {
    CHECK_H(h);
    if (!n_out || (n && (!msgs || !out))) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->kin_configured) return fail(h, LK_ERR_STATE, "the kinematics front end is not configured (lk_kin_configure)");
    if (n >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "more than 2^31 messages in one call");
    *n_out = 0;
    if (n == 0) return LK_OK;
    DevTemps tmp;
    unsigned char* d_msgs = nullptr;
    lk_kin_imu* d_out = nullptr;
    HIPCHK(h, tmp.alloc(&d_msgs, n * (size_t)LK_HIGHSTATE_BYTES));
    HIPCHK(h, tmp.alloc(&d_out, n * sizeof(lk_kin_imu)));
    HIPCHK(h, hipMemcpyAsync(d_msgs, msgs, n * (size_t)LK_HIGHSTATE_BYTES, hipMemcpyHostToDevice, h->stream));
    size_t cnt = 0;
    const int rc = kin_decode(h, d_msgs, n, d_out, &cnt);
    if (rc != LK_OK) {
        hipStreamSynchronize(h->stream);   // (the temporaries are freed on return)
        return rc;
    }
    if (cnt) HIPCHK(h, hipMemcpyAsync(out, d_out, cnt * sizeof(lk_kin_imu), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_out = cnt;
    return LK_OK;
}

int lk_kin_split_dev(lk_handle* h, const lk_kin_imu* d_kins, size_t n_kins, const double* scan_end, size_t n_scans, uint32_t* n_msg,
                     size_t* n_packaged, size_t* n_consumed) {
    CHECK_H(h);
    return split_records(h, d_kins, sizeof(lk_kin_imu), n_kins, scan_end, n_scans, n_msg, n_packaged, n_consumed);
}

int lk_imu_configure(lk_handle* h, int redundancy) {
    CHECK_H(h);
    h->imu_redundancy = redundancy != 0;
    h->imu_configured = true;
    h->imu_fe.last_acc_z = 0.0;   // the callback's zero-initialised static message
    h->imu_fe.last_gyr_z = 0.0;
    h->imu_fe.last_stamp = -HUGE_VAL;
    return LK_OK;
}

int lk_imu_get_frontend(lk_handle* h, lk_imu_frontend_state* st) {
    CHECK_H(h);
    if (!st) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->imu_configured) return fail(h, LK_ERR_STATE, "the IMU front end is not configured (lk_imu_configure)");
    *st = h->imu_fe;
    return LK_OK;
}

int lk_imu_set_frontend(lk_handle* h, const lk_imu_frontend_state* st) {
    CHECK_H(h);
    if (!st) return fail(h, LK_ERR_INVALID, "null argument");
    if (!h->imu_configured) return fail(h, LK_ERR_STATE, "the IMU front end is not configured (lk_imu_configure)");
    h->imu_fe = *st;
    return LK_OK;
}

int lk_decode_imu_dev(lk_handle* h, const void* d_msgs, size_t n, const uint64_t* msg_off, lk_imu* d_out, size_t* n_out) {
    CHECK_H(h);
    LKCHK(imu_decode_check(h, d_msgs, n, msg_off, d_out, n_out));
    if (n == 0) return LK_OK;
    return imu_decode(h, static_cast<const unsigned char*>(d_msgs) + msg_off[0], n, msg_off, d_out, n_out);
}

int lk_decode_imu(lk_handle* h, const void* msgs, size_t n, const uint64_t* msg_off, lk_imu* out, size_t* n_out) {
    CHECK_H(h);
    LKCHK(imu_decode_check(h, msgs, n, msg_off, out, n_out));
    if (n == 0) return LK_OK;
    const size_t len = (size_t)(msg_off[n] - msg_off[0]);
    DevTemps tmp;
    unsigned char* d_msgs = nullptr;
    lk_imu* d_out = nullptr;
    HIPCHK(h, tmp.alloc(&d_msgs, len));
    HIPCHK(h, tmp.alloc(&d_out, n * sizeof(lk_imu)));
    HIPCHK(h, hipMemcpyAsync(d_msgs, static_cast<const unsigned char*>(msgs) + msg_off[0], len, hipMemcpyHostToDevice, h->stream));
    size_t cnt = 0;
    const int rc = imu_decode(h, d_msgs, n, msg_off, d_out, &cnt);
    if (rc != LK_OK) {
        hipStreamSynchronize(h->stream);   // (the temporaries are freed on return)
        return rc;
    }
    if (cnt) HIPCHK(h, hipMemcpyAsync(out, d_out, cnt * sizeof(lk_imu), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    *n_out = cnt;
    return LK_OK;
}

int lk_imu_split_dev(lk_handle* h, const lk_imu* d_imus, size_t n_imus, const double* scan_end, size_t n_scans, uint32_t* n_msg,
                     size_t* n_packaged, size_t* n_consumed) {
    CHECK_H(h);
    return split_records(h, d_imus, sizeof(lk_imu), n_imus, scan_end, n_scans, n_msg, n_packaged, n_consumed);
}

}  // extern "C"
