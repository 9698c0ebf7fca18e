// lk_traj.hip - the trajectory error unit of liblegkilo_hip.so (see lk_internal.h): absolute trajectory error of many trajectories against ground
// truth in one launch (lk_traj_kernels.h) and the two C-ABI entries around it - lk_traj_ate_dev over strided tables the caller owns, lk_runs_ate_dev
// over the bucket table of the handle's last _cloud run replay - and the relative pose error beside it, the same way: lk_traj_rpe_dev, lk_runs_rpe_dev.
// One host path for both families (traj_call: scratch, uploads, launch, fetch, refusal) behind traj_ate / traj_rpe, which keep their own checks and
// members; traj_bucket_side turns the handle's bucket table into the estimate side of either lk_runs_ entry.
#define LK_TU_TRAJ 1
#include "lk_internal.h"
#include "lk_traj_kernels.h"

static_assert(sizeof(lk_ate) == 136, "lk_ate must be 136 B");
static_assert(sizeof(lk_rpe) == 80, "lk_rpe must be 80 B");
static_assert(offsetof(lk_bucket_pose, rot) == 0 && sizeof(lk_bucket_pose) == 144, "lk_runs_rpe_dev reads the bucket table's rotations through this offset");
static_assert(offsetof(lk_bucket_pose, t) == 120 && offsetof(lk_bucket_pose, pos) == 72, "lk_runs_ate_dev reads the bucket table through these offsets");

namespace {
struct TrajSide {   // one side's table as the caller gave it (rot: the RPE entries only)
    const double *t, *pos, *rot;
    size_t stride;
    const uint64_t* off;
};
}  // namespace

// one side's table: pointers, stride and offsets as the header asks for them
static int traj_side_check(lk_handle* h, const char* side, size_t n_traj, const TrajSide& t) {
    const std::string s(side);
    if (!t.t || !t.pos || !t.off) return fail(h, LK_ERR_INVALID, "null argument (" + s + ")");
    if (((uintptr_t)t.t | (uintptr_t)t.pos) & 7) return fail(h, LK_ERR_INVALID, s + " pointers must be 8-byte aligned");
    if (t.stride % 8 || t.stride < 24)
        return fail(h, LK_ERR_INVALID, s + " stride of " + std::to_string(t.stride) + " bytes: a multiple of 8, at least 24 with positions, is required");
    for (size_t r = 0; r < n_traj; ++r) {
        if (t.off[r + 1] < t.off[r]) return fail(h, LK_ERR_INVALID, s + " offsets decrease at trajectory " + std::to_string(r));
        if (t.off[r + 1] - t.off[r] >= 0xffffffffull) return fail(h, LK_ERR_INVALID, s + " of trajectory " + std::to_string(r) + " holds 2^32 - 1 samples or more");
    }
    return LK_OK;
}

// the rotations of one side, beside traj_side_check of its stamps and positions
static int traj_rot_check(lk_handle* h, const char* side, const TrajSide& t) {
    const std::string s(side);
    if (!t.rot) return fail(h, LK_ERR_INVALID, "null argument (" + s + " rotations)");
    if ((uintptr_t)t.rot & 7) return fail(h, LK_ERR_INVALID, s + " rotation pointer must be 8-byte aligned");
    if (t.stride < 72) return fail(h, LK_ERR_INVALID, s + " stride of " + std::to_string(t.stride) + " bytes: a multiple of 8, at least 72 with rotations, is required");
    return LK_OK;
}

// what both families ask of the arguments behind the tables
static int traj_out_check(lk_handle* h, const void* out, double max_dt) {
    if (!out) return fail(h, LK_ERR_INVALID, "null argument (out)");
    if (!(max_dt >= 0.0) || !std::isfinite(max_dt)) return fail(h, LK_ERR_INVALID, "max_dt must be finite and not negative");
    return LK_OK;
}

static int traj_count_check(lk_handle* h, const char* what, size_t n) {
    if (n == 0 || n >= ((size_t)1 << 31)) return fail(h, LK_ERR_INVALID, std::string(what) + " must be 1 .. 2^31 - 1");
    return LK_OK;
}

// the estimate side of both lk_runs_ entries: the bucket table of the handle's last _cloud run replay, checked against run_bucket_off
static int traj_bucket_side(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off, TrajSide* est) {
    if (!h->bucket_n) return fail(h, LK_ERR_STATE, "the handle's last batch replay recorded no bucket poses (lk_batch_replay_runs_cloud_dev / lk_batch_replay_overlay_runs_cloud_dev do)");
    LKCHK(traj_count_check(h, "n_runs", n_runs));
    const lk_bucket_pose* tab = static_cast<const lk_bucket_pose*>(h->bucket_tab.p);
    *est = {&tab->t, &tab->pos[0], &tab->rot[0], sizeof(lk_bucket_pose), run_bucket_off};
    LKCHK(traj_side_check(h, "estimate", n_runs, *est));
    if (run_bucket_off[n_runs] > h->bucket_n) return fail(h, LK_ERR_INVALID, "bucket range ends past the " + std::to_string(h->bucket_n) + " records of the table");
    return LK_OK;
}

// One call of either family behind its checks: `a` arrives with the family's own members filled and gets the shared table here - scratch carved and
// reserved, both offset tables uploaded, the refusal word set - then one wave per trajectory of `kernel` under the profiler name `name`, the word and
// the records back in one synchronisation
template <typename Args, typename Rec>
static int traj_call(lk_handle* h, const char* name, void (*kernel)(Args), Args a, size_t n_traj, const TrajSide& est, const TrajSide& gt, double max_dt, Rec* out) {
    const size_t n_est = (size_t)(est.off[n_traj] - est.off[0]);
    LkTrajTab& t = a.t;
    unsigned long long *eoff = nullptr, *goff = nullptr;
    auto carve = [&](void* base) {
        LkCarve c(base);
        eoff = c.take<unsigned long long>(n_traj + 1), goff = c.take<unsigned long long>(n_traj + 1);
        t.partner = c.take<unsigned int>(n_est);
        a.out = c.take<Rec>(n_traj);
        t.bad = c.take<unsigned int>(1);
        return c.total();
    };
    const size_t bytes = carve(nullptr);
    LKCHK(reserve(h, h->traj, bytes, bytes / 4));
    carve(h->traj.p);
    t.est_t = reinterpret_cast<const unsigned char*>(est.t), t.est_p = reinterpret_cast<const unsigned char*>(est.pos);
    t.gt_t = reinterpret_cast<const unsigned char*>(gt.t), t.gt_p = reinterpret_cast<const unsigned char*>(gt.pos);
    t.est_stride = est.stride, t.gt_stride = gt.stride;
    t.est_off = eoff, t.gt_off = goff;
    t.part_base = est.off[0];
    t.max_dt = max_dt;
    HIPCHK(h, hipMemcpyAsync(eoff, est.off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(goff, gt.off, 8 * (n_traj + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(t.bad, 0xff, sizeof(unsigned int), h->stream));
    LAUNCH(h, name, hipLaunchKernelGGL(kernel, dim3((unsigned int)n_traj), dim3(LK_WAVE), 0, h->stream, a));
    unsigned int bad = 0;
    HIPCHK(h, hipMemcpyAsync(&bad, t.bad, sizeof(bad), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(out, a.out, sizeof(Rec) * n_traj, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (bad != 0xffffffffu)
        return fail(h, LK_ERR_INVALID, "trajectory " + std::to_string(bad >> 1) + ": the " + ((bad & 1) ? "ground truth" : "estimate") +
                                           " stamps decrease or are not finite");
    return LK_OK;
}

// both ATE entries behind their checks of the estimate's side
static int traj_ate(lk_handle* h, size_t n_traj, const TrajSide& est, const TrajSide& gt, double max_dt, uint32_t flags, lk_ate* out) {
    LKCHK(traj_side_check(h, "ground truth", n_traj, gt));
    LKCHK(traj_out_check(h, out, max_dt));
    if (flags & ~LK_ATE_ALIGN) return fail(h, LK_ERR_INVALID, "unknown flag bits");
    LkTraj a = {};
    a.flags = flags;
    return traj_call(h, "traj_ate", lk_traj_ate_kernel, a, n_traj, est, gt, max_dt, out);
}

// both RPE entries behind their checks of the estimate's side
static int traj_rpe(lk_handle* h, size_t n_traj, const TrajSide& est, const TrajSide& gt, double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    LKCHK(traj_side_check(h, "ground truth", n_traj, gt));
    LKCHK(traj_rot_check(h, "ground truth", gt));
    LKCHK(traj_out_check(h, out, max_dt));
    if (flags & ~LK_RPE_INDEX) return fail(h, LK_ERR_INVALID, "unknown flag bits");
    if (!(delta > 0.0) || !std::isfinite(delta)) return fail(h, LK_ERR_INVALID, "delta must be finite and above 0");
    if ((flags & LK_RPE_INDEX) && (delta != std::floor(delta) || delta > 4294967294.0))
        return fail(h, LK_ERR_INVALID, "delta must be a whole number in 1 .. 2^32 - 2 with LK_RPE_INDEX");
    LkTrajRpe a = {};
    a.est_r = reinterpret_cast<const unsigned char*>(est.rot), a.gt_r = reinterpret_cast<const unsigned char*>(gt.rot);
    a.delta = delta, a.flags = flags;
    a.step = (flags & LK_RPE_INDEX) ? (unsigned long long)delta : 0ull;
    return traj_call(h, "traj_rpe", lk_traj_rpe_kernel, a, n_traj, est, gt, max_dt, out);
}

extern "C" {

int lk_traj_ate_dev(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, size_t est_stride, const uint64_t* est_off,
                    const double* d_gt_t, const double* d_gt_pos, size_t gt_stride, const uint64_t* gt_off, double max_dt, uint32_t flags, lk_ate* out) {
    CHECK_H(h);
    LKCHK(traj_count_check(h, "n_traj", n_traj));
    const TrajSide est = {d_est_t, d_est_pos, nullptr, est_stride, est_off};
    LKCHK(traj_side_check(h, "estimate", n_traj, est));
    return traj_ate(h, n_traj, est, {d_gt_t, d_gt_pos, nullptr, gt_stride, gt_off}, max_dt, flags, out);
}

int lk_runs_ate_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off, const double* d_gt_t, const double* d_gt_pos, size_t gt_stride,
                    const uint64_t* gt_off, double max_dt, uint32_t flags, lk_ate* out) {
    CHECK_H(h);
    TrajSide est;
    LKCHK(traj_bucket_side(h, n_runs, run_bucket_off, &est));
    return traj_ate(h, n_runs, est, {d_gt_t, d_gt_pos, nullptr, gt_stride, gt_off}, max_dt, flags, out);
}

int lk_traj_rpe_dev(lk_handle* h, size_t n_traj, const double* d_est_t, const double* d_est_pos, const double* d_est_rot, size_t est_stride,
                    const uint64_t* est_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot, size_t gt_stride, const uint64_t* gt_off,
                    double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    CHECK_H(h);
    LKCHK(traj_count_check(h, "n_traj", n_traj));
    const TrajSide est = {d_est_t, d_est_pos, d_est_rot, est_stride, est_off};
    LKCHK(traj_side_check(h, "estimate", n_traj, est));
    LKCHK(traj_rot_check(h, "estimate", est));
    return traj_rpe(h, n_traj, est, {d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off}, max_dt, delta, flags, out);
}

int lk_runs_rpe_dev(lk_handle* h, size_t n_runs, const uint64_t* run_bucket_off, const double* d_gt_t, const double* d_gt_pos, const double* d_gt_rot,
                    size_t gt_stride, const uint64_t* gt_off, double max_dt, double delta, uint32_t flags, lk_rpe* out) {
    CHECK_H(h);
    TrajSide est;
    LKCHK(traj_bucket_side(h, n_runs, run_bucket_off, &est));
    return traj_rpe(h, n_runs, est, {d_gt_t, d_gt_pos, d_gt_rot, gt_stride, gt_off}, max_dt, delta, flags, out);
}

}  // extern "C"
