// lk_traj.hip - the trajectory error unit of liblegkilo_hip.so (see lk_internal.h): absolute trajectory error of many trajectories against ground
// truth in one launch (lk_traj_kernels.h) and the two C-ABI entries around it - lk_traj_ate_dev over strided tables the caller owns, lk_runs_ate_dev
// over the bucket table of the handle's last _cloud run replay - and the relative pose error beside it, the same way: lk_traj_rpe_dev, lk_runs_rpe_dev.
#define LK_TU_TRAJ 1
#include "lk_internal.h"
#include "lk_traj_kernels.h"

static_assert(sizeof(lk_ate) == 136, "lk_ate must be 136 B");
static_assert(sizeof(lk_rpe) == 80, "lk_rpe must be 80 B");
static_assert(offsetof(lk_bucket_pose, rot) == 0 && sizeof(lk_bucket_pose) == 144, "lk_runs_rpe_dev reads the bucket table's rotations through this offset");
static_assert(offsetof(lk_bucket_pose, t) == 120 && offsetof(lk_bucket_pose, pos) == 72, "lk_runs_ate_dev reads the bucket table through these offsets");

// one side's table: pointers, stride and offsets as the header asks for them
static int traj_side_check(lk_handle* h, const char* side, size_t n_traj, const double* d_t, const double* d_pos, size_t stride, const uint64_t* off) {
    const std::string s(side);
    if (!d_t || !d_pos || !off) return fail(h, LK_ERR_INVALID, "null argument (" + s + ")");
    if (((uintptr_t)d_t | (uintptr_t)d_pos) & 7) return fail(h, LK_ERR_INVALID, s + " pointers must be 8-byte aligned");
    if (stride % 8 || stride < 24) return fail(h, LK_ERR_INVALID, s + " stride of " + std::to_string(stride) + " bytes: a multiple of 8, at least 24 with positions, is required");
    for (size_t r = 0; r < n_traj; ++r) {
        if (off[r + 1] < off[r]) return fail(h, LK_ERR_INVALID, s + " offsets decrease at trajectory " + std::to_string(r));
        if (off[r + 1] - off[r] >= 0xffffffffull) return fail(h, LK_ERR_INVALID, s + " of trajectory " + std::to_string(r) + " holds 2^32 - 1 samples or more");
    }
    return LK_OK;
}

// both entries behind their checks of the estimate's side
static int traj_ate(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, size_t est_stride, const uint64_t* est_off,
                    const double* d_gt_t, const double* d_gt_pos, size_t gt_stride, const uint64_t* gt_off, double max_dt, uint32_t flags, lk_ate* out) {
    LKCHK(traj_side_check(h, "ground truth", n_traj, d_gt_t, d_gt_pos, gt_stride, gt_off));
    if (!out) return fail(h, LK_ERR_INVALID, "null argument (out)");
    if (!(max_dt >= 0.0) || !std::isfinite(max_dt)) return fail(h, LK_ERR_INVALID, "max_dt must be finite and not negative");
    if (flags & ~LK_ATE_ALIGN) return fail(h, LK_ERR_INVALID, "unknown flag bits");
    const size_t n_est = (size_t)(est_off[n_traj] - est_off[0]);
    LkTraj a = {};
    unsigned long long *eoff = nullptr, *goff = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        eoff = c.take<unsigned long long>(n_traj + 1), goff = c.take<unsigned long long>(n_traj + 1);
        a.partner = c.take<unsigned int>(n_est);
        a.out = c.take<lk_ate>(n_traj);
        a.bad = c.take<unsigned int>(1);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->traj, bytes, bytes / 4));
    carve(h->traj.p);
    a.est_t = reinterpret_cast<const unsigned char*>(d_est_t), a.est_p = reinterpret_cast<const unsigned char*>(d_est_pos);
    a.gt_t = reinterpret_cast<const unsigned char*>(d_gt_t), a.gt_p = reinterpret_cast<const unsigned char*>(d_gt_pos);
    a.est_stride = est_stride, a.gt_stride = gt_stride;
    a.est_off = eoff, a.gt_off = goff;
    a.part_base = est_off[0];
    a.max_dt = max_dt, a.flags = flags;
    HIPCHK(h, hipMemcpyAsync(eoff, est_off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(goff, gt_off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(a.bad, 0xff, sizeof(unsigned int), h->stream));
    LAUNCH(h, "traj_ate", hipLaunchKernelGGL(lk_traj_ate_kernel, dim3((unsigned int)n_traj), dim3(LK_WAVE), 0, h->stream, a));
    unsigned int bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, a.bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, a.out, sizeof(lk_ate) * n_traj, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != 0xffffffffu)
        return fail(h, LK_ERR_INVALID, "trajectory " + std::to_string(bad >> 1) + ": the " + ((bad & 1) ? "ground truth" : "estimate") +
                                           " stamps decrease or are not finite");
    return LK_OK;
}

// the rotations of one side, beside traj_side_check of its stamps and positions
static int traj_rot_check(lk_handle* h, const char* side, const double* d_rot, size_t stride) {
    const std::string s(side);
    if (!d_rot) return fail(h, LK_ERR_INVALID, "null argument (" + s + " rotations)");
    if ((uintptr_t)d_rot & 7) return fail(h, LK_ERR_INVALID, s + " rotation pointer must be 8-byte aligned");
    if (stride < 72) return fail(h, LK_ERR_INVALID, s + " stride of " + std::to_string(stride) + " bytes: a multiple of 8, at least 72 with rotations, is required");
    return LK_OK;
}

// both entries behind their checks of the estimate's side
static int traj_rpe(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, const double* d_est_rot, size_t est_stride,
                    const uint64_t* est_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot, size_t gt_stride, const uint64_t* gt_off,
                    double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    LKCHK(traj_side_check(h, "ground truth", n_traj, d_gt_t, d_gt_pos, gt_stride, gt_off));
    LKCHK(traj_rot_check(h, "ground truth", d_gt_rot, gt_stride));
    if (!out) return fail(h, LK_ERR_INVALID, "null argument (out)");
    if (!(max_dt >= 0.0) || !std::isfinite(max_dt)) return fail(h, LK_ERR_INVALID, "max_dt must be finite and not negative");
    if (flags & ~LK_RPE_INDEX) return fail(h, LK_ERR_INVALID, "unknown flag bits");
    if (!(delta > 0.0) || !std::isfinite(delta)) return fail(h, LK_ERR_INVALID, "delta must be finite and above 0");
    if ((flags & LK_RPE_INDEX) && (delta != std::floor(delta) || delta > 4294967294.0))
        return fail(h, LK_ERR_INVALID, "delta must be a whole number in 1 .. 2^32 - 2 with LK_RPE_INDEX");
    const size_t n_est = (size_t)(est_off[n_traj] - est_off[0]);
    LkTrajRpe a = {};
    unsigned long long *eoff = nullptr, *goff = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        eoff = c.take<unsigned long long>(n_traj + 1), goff = c.take<unsigned long long>(n_traj + 1);
        a.partner = c.take<unsigned int>(n_est);
        a.out = c.take<lk_rpe>(n_traj);
        a.bad = c.take<unsigned int>(1);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->traj, bytes, bytes / 4));
    carve(h->traj.p);
    a.est_t = reinterpret_cast<const unsigned char*>(d_est_t), a.est_p = reinterpret_cast<const unsigned char*>(d_est_pos);
    a.est_r = reinterpret_cast<const unsigned char*>(d_est_rot);
    a.gt_t = reinterpret_cast<const unsigned char*>(d_gt_t), a.gt_p = reinterpret_cast<const unsigned char*>(d_gt_pos);
    a.gt_r = reinterpret_cast<const unsigned char*>(d_gt_rot);
    a.est_stride = est_stride, a.gt_stride = gt_stride;
    a.est_off = eoff, a.gt_off = goff;
    a.part_base = est_off[0];
    a.max_dt = max_dt, a.delta = delta, a.flags = flags;
    a.step = (flags & LK_RPE_INDEX) ? (unsigned long long)delta : 0ull;
    HIPCHK(h, hipMemcpyAsync(eoff, est_off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(goff, gt_off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(a.bad, 0xff, sizeof(unsigned int), h->stream));
    LAUNCH(h, "traj_rpe", hipLaunchKernelGGL(lk_traj_rpe_kernel, dim3((unsigned int)n_traj), dim3(LK_WAVE), 0, h->stream, a));
    unsigned int bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, a.bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, a.out, sizeof(lk_rpe) * n_traj, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != 0xffffffffu)
        return fail(h, LK_ERR_INVALID, "trajectory " + std::to_string(bad >> 1) + ": the " + ((bad & 1) ? "ground truth" : "estimate") +
                                           " stamps decrease or are not finite");
    return LK_OK;
}

extern "C" {

int lk_traj_ate_dev(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, size_t est_stride, const uint64_t* est_off,
                    const double* d_gt_t, const double* d_gt_pos, size_t gt_stride, const uint64_t* gt_off, double max_dt, uint32_t flags, lk_ate* out) {
    CHECK_H(h);
    if (n_traj == 0 || n_traj >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "n_traj must be 1 .. 2^31 - 1");
    LKCHK(traj_side_check(h, "estimate", n_traj, d_est_t, d_est_pos, est_stride, est_off));
    return traj_ate(h, n_traj, d_est_t, d_est_pos, est_stride, est_off, d_gt_t, d_gt_pos, gt_stride, gt_off, max_dt, flags, out);
}

int lk_runs_ate_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off, const double* d_gt_t, const double* d_gt_pos, size_t gt_stride,
                    const uint64_t* gt_off, double max_dt, uint32_t flags, lk_ate* out) {
    CHECK_H(h);
    if (!h->bucket_n) return fail(h, LK_ERR_STATE, "the handle's last batch replay recorded no bucket poses (lk_batch_replay_runs_cloud_dev / lk_batch_replay_overlay_runs_cloud_dev do)");
    if (n_runs == 0 || n_runs >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "n_runs must be 1 .. 2^31 - 1");
    const lk_bucket_pose* tab = static_cast<const lk_bucket_pose*>(h->bucket_tab.p);
    LKCHK(traj_side_check(h, "estimate", n_runs, &tab->t, &tab->pos[0], sizeof(lk_bucket_pose), run_bucket_off));
    if (run_bucket_off[n_runs] > h->bucket_n) return fail(h, LK_ERR_INVALID, "bucket range ends past the " + std::to_string(h->bucket_n) + " records of the table");
    return traj_ate(h, n_runs, &tab->t, &tab->pos[0], sizeof(lk_bucket_pose), run_bucket_off, d_gt_t, d_gt_pos, gt_stride, gt_off, max_dt, flags, out);
}

int lk_traj_rpe_dev(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, const double* d_est_rot, size_t est_stride,
                    const uint64_t* est_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot, size_t gt_stride, const uint64_t* gt_off,
                    double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    CHECK_H(h);
    if (n_traj == 0 || n_traj >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "n_traj must be 1 .. 2^31 - 1");
    LKCHK(traj_side_check(h, "estimate", n_traj, d_est_t, d_est_pos, est_stride, est_off));
    LKCHK(traj_rot_check(h, "estimate", d_est_rot, est_stride));
    return traj_rpe(h, n_traj, d_est_t, d_est_pos, d_est_rot, est_stride, est_off, d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off, max_dt, delta, flags, out);
}

int lk_runs_rpe_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot,
                    size_t gt_stride, const uint64_t* gt_off, double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    CHECK_H(h);
    if (!h->bucket_n) return fail(h, LK_ERR_STATE, "the handle's last batch replay recorded no bucket poses (lk_batch_replay_runs_cloud_dev / lk_batch_replay_overlay_runs_cloud_dev do)");
    if (n_runs == 0 || n_runs >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, "n_runs must be 1 .. 2^31 - 1");
    const lk_bucket_pose* tab = static_cast<const lk_bucket_pose*>(h->bucket_tab.p);
    LKCHK(traj_side_check(h, "estimate", n_runs, &tab->t, &tab->pos[0], sizeof(lk_bucket_pose), run_bucket_off));
    if (run_bucket_off[n_runs] > h->bucket_n) return fail(h, LK_ERR_INVALID, "bucket range ends past the " + std::to_string(h->bucket_n) + " records of the table");
    return traj_rpe(h, n_runs, &tab->t, &tab->pos[0], &tab->rot[0], sizeof(lk_bucket_pose), run_bucket_off, d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off,
                    max_dt, delta, flags, out);
}

}  // extern "C"
