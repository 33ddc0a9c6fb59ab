// flyhip_abi.hip — the extern "C" surface declared in include/flyhip.h.
// Argument checking, handle lifetime and error strings live here; the kernels and their launchers
// (flyhip_launch_*) live in the other .hip files of this directory and are declared, once, in
// launch.h.  Nothing here synchronises the host or allocates caller tensors.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <new>
#include "flyhip.h"
#include "obs_norm.h"
#include "domain_rand.h"
#include "launch.h"
#include <math.h>

struct FlyEnv {
    FlyConfig host;
    FlyConfig* dev;
    float* poses;           // fly_set_pose_record (device [T][FLY_POSE_FLOATS], NULL = off)
    const float* obs_norm;  // fly_set_obs_norm (device [FLY_OBS_NORM_TABLE], NULL = off); also in dev's slot (obs_norm.h)
    float* dr_table;        // fly_set_randomization (device [N][FLY_DR_ROW], NULL = off); with the ranges in dev's slot (domain_rand.h)
};

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    return fail(FLY_E_HIP, "%s: %s", what, hipGetErrorString(e));
}

int check_buffers(const FlyBuffers* b, int phases)
{
    if (!b) return fail(FLY_E_ARG, "FlyBuffers is null");
    const bool need_root = phases & (PH_RESET | PH_INTEGRATE | PH_OBS | PH_REWARD);
    const bool need_dof = phases & (PH_RESET | PH_INTEGRATE | PH_OBS);
    const bool need_tgt = phases & (PH_SCALE | PH_INTEGRATE | PH_OBS | PH_REWARD);
    const bool need_con = phases & (PH_INTEGRATE | PH_OBS | PH_REWARD);
    const bool need_pot = phases & (PH_RESET | PH_OBS | PH_REWARD);
    const bool need_obs = phases & (PH_OBS | PH_REWARD);
    const bool need_flags = phases & (PH_RESET | PH_REWARD | PH_PROGRESS);
    if (need_root && !b->root) return fail(FLY_E_ARG, "root is null");
    if (need_dof && !b->dof_state) return fail(FLY_E_ARG, "dof_state is null");
    if (need_tgt && !b->targets) return fail(FLY_E_ARG, "targets is null");
    if (need_con && !b->contact) return fail(FLY_E_ARG, "contact is null");
    if (need_pot && (!b->pot || !b->prev_pot)) return fail(FLY_E_ARG, "pot/prev_pot is null");
    if (need_obs && !b->obs) return fail(FLY_E_ARG, "obs is null");
    if (need_obs && ((uintptr_t)b->obs & 3)) return fail(FLY_E_ARG, "obs must be 4-byte aligned");
    if ((phases & PH_REWARD) && !b->reward) return fail(FLY_E_ARG, "reward is null");
    if (need_flags && (!b->reset || !b->progress)) return fail(FLY_E_ARG, "reset/progress is null");
    return FLY_OK;
}

int launch(FlyHandle h, int phases, const float* actions, const FlyBuffers* b, void* stream)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if ((phases & PH_SCALE) && !actions) return fail(FLY_E_ARG, "actions is null");
    int rc = check_buffers(b, phases);
    if (rc) return rc;
    hipError_t e = flyhip_launch_env(phases, h->dev, h->host.num_envs, actions, b, stream, h->dr_table != nullptr);
    if (e != hipSuccess) return hip_fail(e, "fly env kernel launch");
    return FLY_OK;
}
}  // namespace

extern "C" {

const char* fly_last_error(void) { return g_err; }
int fly_abi_version(void) { return FLY_ABI_VERSION; }

int fly_create(const FlyConfig* cfg, FlyHandle* out)
{
    if (!cfg || !out) return fail(FLY_E_ARG, "fly_create: null argument");
    if (cfg->num_envs <= 0) return fail(FLY_E_CONFIG, "num_envs must be > 0 (got %d)", cfg->num_envs);
    if (cfg->substeps <= 0 || cfg->substeps > 1024) return fail(FLY_E_CONFIG, "substeps out of range (%d)", cfg->substeps);
    if (!(cfg->dt > 0.0f)) return fail(FLY_E_CONFIG, "dt must be > 0");
    if (!(cfg->mass > 0.0f) || !(cfg->joint_inertia > 0.0f)) return fail(FLY_E_CONFIG, "mass / joint_inertia must be > 0");
    for (int i = 0; i < 3; ++i)
        if (!(cfg->inertia[i] > 0.0f)) return fail(FLY_E_CONFIG, "inertia[%d] must be > 0", i);
    for (int j = 0; j < FLY_NUM_DOF; ++j)
        if (!(cfg->dof_hi[j] > cfg->dof_lo[j])) return fail(FLY_E_CONFIG, "dof limits of joint %d are not ordered", j);
    if (cfg->reward_mode != 0 && cfg->reward_mode != 1) return fail(FLY_E_CONFIG, "reward_mode must be 0 or 1");
    FlyEnv* h = new (std::nothrow) FlyEnv;
    if (!h) return fail(FLY_E_ARG, "out of host memory");
    h->host = *cfg;
    h->dev = nullptr;
    h->poses = nullptr;
    h->obs_norm = nullptr;
    h->dr_table = nullptr;
    hipError_t e = hipMalloc((void**)&h->dev, DR_CONFIG_BYTES);    // FlyConfig + the obs-norm table slot + the randomisation slot
    if (e != hipSuccess) { delete h; return hip_fail(e, "hipMalloc(FlyConfig)"); }
    e = hipMemcpy(h->dev, cfg, sizeof(FlyConfig), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(reinterpret_cast<char*>(h->dev) + OBS_NORM_SLOT, 0, DR_CONFIG_BYTES - OBS_NORM_SLOT);
    if (e != hipSuccess) { (void)hipFree(h->dev); delete h; return hip_fail(e, "hipMemcpy(FlyConfig)"); }
    *out = h;
    return FLY_OK;
}

int fly_destroy(FlyHandle h)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    hipError_t e = hipFree(h->dev);
    delete h;
    if (e != hipSuccess) return hip_fail(e, "hipFree(FlyConfig)");
    return FLY_OK;
}

int fly_step(FlyHandle h, const float* actions, const FlyBuffers* b, void* stream)
{
    return launch(h, PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD, actions, b, stream);
}

int ppo_rollout_step(FlyHandle h, const FlyBuffers* b, const float* params, const float* params_frag, const float* x,
                     const float* eps, const float* var, int32_t var_steps, float var_decay, float var_min,
                     float* act_out, float* logp_out, float* v_out, const uint16_t* params_b3,
                     const int32_t* var_steps_base, void* stream)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (!params || !params_frag || !x || !eps || !var || !act_out || !logp_out)
        return fail(FLY_E_ARG, "ppo_rollout_step: null pointer");
    if (var_steps < 0 || var_steps > (1 << 20)) return fail(FLY_E_ARG, "ppo_rollout_step: var_steps out of range");
    int rc = check_buffers(b, PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD);
    if (rc) return rc;
    hipError_t e = flyhip_launch_rollout_step(h->dev, b, params, params_frag, x, h->host.num_envs, eps, var, var_steps,
                                              var_decay, var_min, act_out, logp_out, v_out, params_b3, var_steps_base, stream,
                                              h->obs_norm != nullptr, h->dr_table != nullptr);
    if (e != hipSuccess) return hip_fail(e, "ppo_rollout_step launch");
    return FLY_OK;
}

static int rollout_all_impl(FlyHandle h, const FlyBuffers* b, const float* params, const float* params_frag, float* obs_ring,
                            const float* eps_all, const float* var, float var_decay, float var_min, float* act_all,
                            float* logp_all, float* v_ring, float* reward_all, int32_t T, const int32_t* rows_applied,
                            const uint16_t* params_b3, int64_t* reset_rows, int64_t* progress_rows, void* stream,
                            unsigned long long* stamps)
{
    if ((reset_rows != nullptr) != (progress_rows != nullptr)) return fail(FLY_E_ARG, "ppo_rollout_all: reset_rows and progress_rows go together");
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (!params || !params_frag || !obs_ring || !eps_all || !var || !act_all || !logp_all || !v_ring || !reward_all)
        return fail(FLY_E_ARG, "ppo_rollout_all: null pointer");
    if (T <= 0 || T > (1 << 20)) return fail(FLY_E_ARG, "ppo_rollout_all: T out of range");
    if (!b) return fail(FLY_E_ARG, "ppo_rollout_all: buffers are null");
    FlyBuffers bb = *b;
    bb.obs = obs_ring; bb.reward = reward_all;              // checked as present; the kernel walks the rows itself
    int rc = check_buffers(&bb, PH_SCALE | PH_RESET | PH_INTEGRATE | PH_OBS | PH_PROGRESS | PH_REWARD);
    if (rc) return rc;
    if (stamps && h->obs_norm) return fail(FLY_E_ARG, "the stamped rollout does not normalise observations (fly_set_obs_norm)");
    if (stamps && h->dr_table) return fail(FLY_E_ARG, "the stamped rollout does not randomise the physics (fly_set_randomization)");
    hipError_t e = flyhip_launch_rollout_all(h->dev, &bb, params, params_frag, obs_ring, h->host.num_envs, eps_all, var,
                                             var_decay, var_min, act_all, logp_all, v_ring, reward_all, T, rows_applied,
                                             params_b3, reset_rows, progress_rows, stream, stamps, stamps ? nullptr : h->poses,
                                             h->obs_norm != nullptr, h->dr_table != nullptr);
    if (e != hipSuccess) return hip_fail(e, "ppo_rollout_all launch");
    return FLY_OK;
}

int ppo_rollout_all(FlyHandle h, const FlyBuffers* b, const float* params, const float* params_frag, float* obs_ring,
                    const float* eps_all, const float* var, float var_decay, float var_min, float* act_all,
                    float* logp_all, float* v_ring, float* reward_all, int32_t T, const int32_t* rows_applied,
                    const uint16_t* params_b3, int64_t* reset_rows, int64_t* progress_rows, void* stream)
{
    return rollout_all_impl(h, b, params, params_frag, obs_ring, eps_all, var, var_decay, var_min, act_all, logp_all, v_ring,
                            reward_all, T, rows_applied, params_b3, reset_rows, progress_rows, stream, nullptr);
}

// diagnostic: the same launch through the stamped instantiation of rollout_all_fs_kernel (bench.py's policy / env split of a
// rollout step, tools/ab_rollout.py); stamps u64 [tiles][T + 1][8].  Not part of the ABI header.
extern "C" int flyhip_debug_rollout_all_stamped(FlyHandle h, const FlyBuffers* b, const float* params, const float* params_frag,
                                                float* obs_ring, const float* eps_all, const float* var, float var_decay,
                                                float var_min, float* act_all, float* logp_all, float* v_ring, float* reward_all,
                                                int32_t T, const uint16_t* params_b3, int64_t* reset_rows, int64_t* progress_rows,
                                                unsigned long long* stamps, void* stream)
{
    if (!stamps) return fail(FLY_E_ARG, "stamps is null");
    return rollout_all_impl(h, b, params, params_frag, obs_ring, eps_all, var, var_decay, var_min, act_all, logp_all, v_ring,
                            reward_all, T, nullptr, params_b3, reset_rows, progress_rows, stream, stamps);
}

int fly_set_pose_record(FlyHandle h, float* poses)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (reinterpret_cast<uintptr_t>(poses) & 3) return fail(FLY_E_ARG, "fly_set_pose_record: poses is not 4-byte aligned");
    h->poses = poses;
    return FLY_OK;
}

int fly_set_obs_norm(FlyHandle h, const float* table)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (reinterpret_cast<uintptr_t>(table) & 3) return fail(FLY_E_ARG, "fly_set_obs_norm: table is not 4-byte aligned");
    // synchronous: the slot holds the new pointer before any later launch on any stream reads it
    hipError_t e = hipMemcpy(reinterpret_cast<char*>(h->dev) + OBS_NORM_SLOT, &table, sizeof(table), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "fly_set_obs_norm");
    h->obs_norm = table;
    return FLY_OK;
}

int fly_set_randomization(FlyHandle h, const FlyRandomization* r, float* env_params, void* stream)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (!r) {               // off: the plain kernels again; the slot and the table are left as they are
        h->dr_table = nullptr;
        return FLY_OK;
    }
    static const char* const names[FLY_DR_PARAMS] = {"kp", "kd", "effort", "mass", "mu", "gravity"};
    for (int j = 0; j < FLY_DR_PARAMS; ++j) {
        const float lo = r->lo[j], hi = r->hi[j];
        if (!isfinite(lo) || !isfinite(hi)) return fail(FLY_E_ARG, "fly_set_randomization: %s bounds are not finite", names[j]);
        if (!(lo > 0.0f)) return fail(FLY_E_ARG, "fly_set_randomization: %s lower bound must be > 0 (got %g)", names[j], (double)lo);
        if (lo > hi) return fail(FLY_E_ARG, "fly_set_randomization: %s range is not ordered (%g > %g)", names[j], (double)lo, (double)hi);
    }
    if (!env_params) return fail(FLY_E_ARG, "fly_set_randomization: env_params is null");
    if (reinterpret_cast<uintptr_t>(env_params) & 15) return fail(FLY_E_ARG, "fly_set_randomization: env_params is not 16-byte aligned");
    DrSlot slot;
    slot.table = env_params;
    slot.r = *r;
    // synchronous: the slot holds the new table and ranges before the registration draw and any later launch read them
    hipError_t e = hipMemcpy(reinterpret_cast<char*>(h->dev) + DR_SLOT, &slot, sizeof(slot), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "fly_set_randomization");
    e = flyhip_launch_dr_register(h->dev, h->host.num_envs, stream);
    if (e != hipSuccess) return hip_fail(e, "fly_set_randomization launch");
    h->dr_table = env_params;
    return FLY_OK;
}

int ppo_obs_norm_pass(const float* ring, int64_t rows, int64_t count_from, const float* table, float* out, double* sets,
                      void* stream)
{
    if (!ring || !table || !out || !sets) return fail(FLY_E_ARG, "ppo_obs_norm_pass: null pointer");
    if (rows <= 0 || count_from < 0 || count_from > rows) return fail(FLY_E_ARG, "ppo_obs_norm_pass: bad row range");
    if (ring == out) return fail(FLY_E_ARG, "ppo_obs_norm_pass: out must not alias the ring");
    hipError_t e = flyhip_launch_obs_norm_pass(ring, rows, count_from, table, out, sets, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_obs_norm_pass launch");
    return FLY_OK;
}

int ppo_obs_norm_merge(double* stats, float* table, const double* sets, int64_t k, float clip, void* stream)
{
    if (!stats || !table || !sets) return fail(FLY_E_ARG, "ppo_obs_norm_merge: null pointer");
    if (k <= 0 || !(clip > 0.0f)) return fail(FLY_E_ARG, "ppo_obs_norm_merge: bad argument");
    hipError_t e = flyhip_launch_obs_norm_merge(stats, table, sets, k, clip, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_obs_norm_merge launch");
    return FLY_OK;
}

int ppo_td_gae_vnorm(const float* reward, const float* v, const float* v_next, const float* done, const float* table,
                     float gamma, float lambda, int64_t T, int64_t N, float* target_out, float* adv_out, double* sets,
                     int mode_flags, void* stream)
{
    if (!reward || !v || !v_next || !done || !table || !target_out || !adv_out || !sets)
        return fail(FLY_E_ARG, "ppo_td_gae_vnorm: null pointer");
    if (T <= 0 || N <= 0) return fail(FLY_E_ARG, "ppo_td_gae_vnorm: T and N must be > 0");
    if (reinterpret_cast<uintptr_t>(sets) & 7) return fail(FLY_E_ARG, "ppo_td_gae_vnorm: sets is not 8-byte aligned");
    if ((mode_flags & PPO_GAE_SCAN) && (mode_flags & PPO_GAE_MASK_RECURRENCE))
        return fail(FLY_E_ARG, "ppo_td_gae_vnorm: PPO_GAE_SCAN does not implement the masked recurrence");
    hipError_t e = flyhip_launch_td_gae_vnorm(reward, v, v_next, done, table, gamma, lambda, T, N, target_out, adv_out, sets,
                                              mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_td_gae_vnorm launch");
    return FLY_OK;
}

int ppo_value_norm_merge(const double* stats_in, const double* sets, int64_t k, double* stats_out, float* table_out, void* stream)
{
    if (!stats_in || !sets || !stats_out || !table_out) return fail(FLY_E_ARG, "ppo_value_norm_merge: null pointer");
    if (k <= 0) return fail(FLY_E_ARG, "ppo_value_norm_merge: k must be > 0");
    if ((reinterpret_cast<uintptr_t>(stats_in) | reinterpret_cast<uintptr_t>(sets) | reinterpret_cast<uintptr_t>(stats_out)) & 7)
        return fail(FLY_E_ARG, "ppo_value_norm_merge: a float64 buffer is not 8-byte aligned");
    if (stats_in < stats_out + FLY_VALUE_NORM_SET && stats_out < stats_in + FLY_VALUE_NORM_SET)
        return fail(FLY_E_ARG, "ppo_value_norm_merge: stats_out must not overlap stats_in");
    hipError_t e = flyhip_launch_value_norm_merge(stats_in, sets, k, stats_out, table_out, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_value_norm_merge launch");
    return FLY_OK;
}

int ppo_value_norm_apply(const float* target, int64_t n, const float* table, float* out, void* stream)
{
    if (!target || !table || !out) return fail(FLY_E_ARG, "ppo_value_norm_apply: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "ppo_value_norm_apply: n must be > 0");
    if (target < out + n && out < target + n) return fail(FLY_E_ARG, "ppo_value_norm_apply: out must not alias the targets");
    hipError_t e = flyhip_launch_value_norm_apply(target, n, table, out, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_value_norm_apply launch");
    return FLY_OK;
}

int ppo_lambda_targets(const float* adv, const float* v, const float* table, int64_t n, float* target_out, double* sets,
                       void* stream)
{
    if (!adv || !v || !target_out) return fail(FLY_E_ARG, "ppo_lambda_targets: null pointer");
    if (n < 0) return fail(FLY_E_ARG, "ppo_lambda_targets: n must be >= 0");
    if ((reinterpret_cast<uintptr_t>(adv) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(table) |
         reinterpret_cast<uintptr_t>(target_out)) & 3)
        return fail(FLY_E_ARG, "ppo_lambda_targets: a float32 buffer is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sets) & 7) return fail(FLY_E_ARG, "ppo_lambda_targets: sets is not 8-byte aligned");
    if ((target_out < adv + n && adv < target_out + n) || (target_out < v + n && v < target_out + n))
        return fail(FLY_E_ARG, "ppo_lambda_targets: target_out must not alias the inputs");
    if (n == 0 && !sets) return FLY_OK;                     // nothing to write at all
    hipError_t e = flyhip_launch_lambda_targets(adv, v, table, n, target_out, sets, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_lambda_targets launch");
    return FLY_OK;
}

// the checks the two episodic entry points share; `what` names the caller in the message
static int check_episodic(const char* what, bool any_null, int64_t max_episode_length, int64_t T, int64_t N, int mode_flags)
{
    if (any_null) return fail(FLY_E_ARG, "%s: null pointer", what);
    if (T <= 0 || N <= 0) return fail(FLY_E_ARG, "%s: T and N must be > 0", what);
    if (max_episode_length <= 0) return fail(FLY_E_ARG, "%s: max_episode_length must be > 0", what);
    if (mode_flags != 0 && mode_flags != PPO_GAE_SCAN)
        return fail(FLY_E_ARG, "%s: mode_flags must be 0 or PPO_GAE_SCAN (got %d)", what, mode_flags);
    return FLY_OK;
}

int ppo_td_gae_episodic(const float* reward, const float* v, const float* v_next, const int64_t* reset, const int64_t* progress,
                        const int64_t* ended_prev, int64_t max_episode_length, float gamma, float lambda, int64_t T, int64_t N,
                        float* target_out, float* adv_out, int mode_flags, void* stream)
{
    int rc = check_episodic("ppo_td_gae_episodic",
                            !reward || !v || !v_next || !reset || !progress || !ended_prev || !target_out || !adv_out,
                            max_episode_length, T, N, mode_flags);
    if (rc) return rc;
    hipError_t e = flyhip_launch_td_gae_episodic(reward, v, v_next, reset, progress, ended_prev, max_episode_length, gamma, lambda,
                                                 T, N, target_out, adv_out, mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_td_gae_episodic launch");
    return FLY_OK;
}

int ppo_td_gae_episodic_vnorm(const float* reward, const float* v, const float* v_next, const int64_t* reset,
                              const int64_t* progress, const int64_t* ended_prev, int64_t max_episode_length, const float* table,
                              float gamma, float lambda, int64_t T, int64_t N, float* target_out, float* adv_out, double* sets,
                              int mode_flags, void* stream)
{
    int rc = check_episodic("ppo_td_gae_episodic_vnorm",
                            !reward || !v || !v_next || !reset || !progress || !ended_prev || !table || !target_out || !adv_out || !sets,
                            max_episode_length, T, N, mode_flags);
    if (rc) return rc;
    if (reinterpret_cast<uintptr_t>(sets) & 7) return fail(FLY_E_ARG, "ppo_td_gae_episodic_vnorm: sets is not 8-byte aligned");
    hipError_t e = flyhip_launch_td_gae_episodic_vnorm(reward, v, v_next, reset, progress, ended_prev, max_episode_length, table,
                                                       gamma, lambda, T, N, target_out, adv_out, sets, mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_td_gae_episodic_vnorm launch");
    return FLY_OK;
}

int ppo_episode_stats(const float* reward, const int64_t* reset, const int64_t* progress, int64_t max_episode_length, int64_t T,
                      int64_t N, double* carry_ret, int64_t* carry_len, double* sets, int mode_flags, void* stream)
{
    int rc = check_episodic("ppo_episode_stats", !reward || !reset || !progress || !carry_ret || !carry_len || !sets,
                            max_episode_length, T, N, mode_flags);
    if (rc) return rc;
    if (T > (INT64_MAX >> 3) / N) return fail(FLY_E_ARG, "ppo_episode_stats: T * N int64 rows overflow a byte offset");
    if (reinterpret_cast<uintptr_t>(reward) & 3) return fail(FLY_E_ARG, "ppo_episode_stats: reward is not 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(reset) | reinterpret_cast<uintptr_t>(progress) | reinterpret_cast<uintptr_t>(carry_ret) |
         reinterpret_cast<uintptr_t>(carry_len) | reinterpret_cast<uintptr_t>(sets)) & 7)
        return fail(FLY_E_ARG, "ppo_episode_stats: an int64 / float64 buffer is not 8-byte aligned");
    hipError_t e = flyhip_launch_episode_stats(reward, reset, progress, max_episode_length, T, N, carry_ret, carry_len, sets,
                                               mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_episode_stats launch");
    return FLY_OK;
}

int ppo_episode_stats_merge(const double* sets, int64_t nsets, double* window, double* total, void* stream)
{
    if (!sets || !window || !total) return fail(FLY_E_ARG, "ppo_episode_stats_merge: null pointer");
    if (nsets <= 0) return fail(FLY_E_ARG, "ppo_episode_stats_merge: nsets must be > 0");
    if (nsets > INT64_MAX / (FLY_EPISODE_SET * (int64_t)sizeof(double)))
        return fail(FLY_E_ARG, "ppo_episode_stats_merge: nsets * FLY_EPISODE_SET overflows int64");
    if ((reinterpret_cast<uintptr_t>(sets) | reinterpret_cast<uintptr_t>(window) | reinterpret_cast<uintptr_t>(total)) & 7)
        return fail(FLY_E_ARG, "ppo_episode_stats_merge: a float64 buffer is not 8-byte aligned");
    if (window < total + FLY_EPISODE_SET && total < window + FLY_EPISODE_SET)
        return fail(FLY_E_ARG, "ppo_episode_stats_merge: window must not overlap total");
    hipError_t e = flyhip_launch_episode_stats_merge(sets, nsets, window, total, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_episode_stats_merge launch");
    return FLY_OK;
}

int ppo_reward_returns(const float* reward, const int64_t* reset, float gamma, int64_t T, int64_t N, const double* carry_in,
                       double* carry_out, double* sets, int mode_flags, void* stream)
{
    if (!reward || !reset || !carry_in || !carry_out || !sets) return fail(FLY_E_ARG, "ppo_reward_returns: null pointer");
    if (T < 1 || N < 1) return fail(FLY_E_ARG, "ppo_reward_returns: T and N must be > 0");
    if (mode_flags != 0 && mode_flags != PPO_GAE_SCAN)
        return fail(FLY_E_ARG, "ppo_reward_returns: mode_flags must be 0 or PPO_GAE_SCAN (got %d)", mode_flags);
    if (T > (INT64_MAX >> 3) / N) return fail(FLY_E_ARG, "ppo_reward_returns: T * N int64 rows overflow a byte offset");
    if (reinterpret_cast<uintptr_t>(reward) & 3) return fail(FLY_E_ARG, "ppo_reward_returns: reward is not 4-byte aligned");
    if ((reinterpret_cast<uintptr_t>(reset) | reinterpret_cast<uintptr_t>(carry_in) | reinterpret_cast<uintptr_t>(carry_out) |
         reinterpret_cast<uintptr_t>(sets)) & 7)
        return fail(FLY_E_ARG, "ppo_reward_returns: an int64 / float64 buffer is not 8-byte aligned");
    if (carry_in != carry_out && carry_in < carry_out + N && carry_out < carry_in + N)
        return fail(FLY_E_ARG, "ppo_reward_returns: carry_out must be carry_in or not overlap it");
    hipError_t e = flyhip_launch_reward_returns(reward, reset, gamma, T, N, carry_in, carry_out, sets, mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_reward_returns launch");
    return FLY_OK;
}

int ppo_reward_scale(const float* reward, int64_t n, const float* table, float clip, float* out, void* stream)
{
    if (!reward || !table || !out) return fail(FLY_E_ARG, "ppo_reward_scale: null pointer");
    if (n < 1) return fail(FLY_E_ARG, "ppo_reward_scale: n must be > 0");
    if (!(clip > 0.0f)) return fail(FLY_E_ARG, "ppo_reward_scale: clip must be > 0");
    if ((reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(table) | reinterpret_cast<uintptr_t>(out)) & 3)
        return fail(FLY_E_ARG, "ppo_reward_scale: a float32 buffer is not 4-byte aligned");
    if (reward != out && reward < out + n && out < reward + n)
        return fail(FLY_E_ARG, "ppo_reward_scale: out must be the reward buffer or not overlap it");
    hipError_t e = flyhip_launch_reward_scale(reward, n, table, clip, out, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_reward_scale launch");
    return FLY_OK;
}

int ppo_update_stats(const float* mu, const float* action, const float* old_logp, const float* adv, const float* v,
                     const float* target, const float* var, float clip, int64_t R, double* sets, void* stream)
{
    if (!mu || !action || !old_logp || !adv || !v || !target || !var || !sets) return fail(FLY_E_ARG, "ppo_update_stats: null pointer");
    if (R < 1) return fail(FLY_E_ARG, "ppo_update_stats: R must be > 0");
    if (!(clip > 0.0f && clip < 1.0f)) return fail(FLY_E_ARG, "ppo_update_stats: clip must be in (0, 1) (got %g)", (double)clip);   // NaN too
    if (R > (INT64_MAX >> 2) / 18) return fail(FLY_E_ARG, "ppo_update_stats: R * 18 floats overflow a byte offset");
    if ((reinterpret_cast<uintptr_t>(mu) | reinterpret_cast<uintptr_t>(action) | reinterpret_cast<uintptr_t>(old_logp) |
         reinterpret_cast<uintptr_t>(adv) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(target) |
         reinterpret_cast<uintptr_t>(var)) & 3)
        return fail(FLY_E_ARG, "ppo_update_stats: a float32 buffer is not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(sets) & 7) return fail(FLY_E_ARG, "ppo_update_stats: sets is not 8-byte aligned");
    hipError_t e = flyhip_launch_update_stats(mu, action, old_logp, adv, v, target, var, clip, R, sets, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_update_stats launch");
    return FLY_OK;
}

int ppo_update_stats_merge(const double* sets, int64_t nsets, double* last, double* window, double* total, void* stream)
{
    if (!sets || !last || !window || !total) return fail(FLY_E_ARG, "ppo_update_stats_merge: null pointer");
    if (nsets < 1) return fail(FLY_E_ARG, "ppo_update_stats_merge: nsets must be > 0");
    if (nsets > INT64_MAX / (FLY_UPDATE_STATS_SET * (int64_t)sizeof(double)))
        return fail(FLY_E_ARG, "ppo_update_stats_merge: nsets * FLY_UPDATE_STATS_SET overflows int64");
    if ((reinterpret_cast<uintptr_t>(sets) | reinterpret_cast<uintptr_t>(last) | reinterpret_cast<uintptr_t>(window) |
         reinterpret_cast<uintptr_t>(total)) & 7)
        return fail(FLY_E_ARG, "ppo_update_stats_merge: a float64 buffer is not 8-byte aligned");
    const double* p[3] = {last, window, total};
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j)
            if (p[i] < p[j] + FLY_UPDATE_STATS_SET && p[j] < p[i] + FLY_UPDATE_STATS_SET)
                return fail(FLY_E_ARG, "ppo_update_stats_merge: last, window and total must not overlap");
    hipError_t e = flyhip_launch_update_stats_merge(sets, nsets, last, window, total, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_update_stats_merge launch");
    return FLY_OK;
}

int ppo_minibatch_gather(const float* obs, const float* act, const float* logp, const float* adv, const float* target, int64_t R,
                         uint32_t seed, uint32_t epoch_key, int64_t first, int64_t n, float* obs_out, float* act_out,
                         float* logp_out, float* adv_out, float* target_out, int32_t* index_out, void* stream)
{
    if (!obs || !act || !logp || !adv || !target || !obs_out || !act_out || !logp_out || !adv_out || !target_out)
        return fail(FLY_E_ARG, "ppo_minibatch_gather: null pointer");
    if (R < 1 || R >= (int64_t)1 << 31) return fail(FLY_E_ARG, "ppo_minibatch_gather: R must be in [1, 2^31)");
    if (n < 1 || first < 0 || first > R - n) return fail(FLY_E_ARG, "ppo_minibatch_gather: [first, first + n) is not a window of [0, R)");
    if ((reinterpret_cast<uintptr_t>(obs_out) | reinterpret_cast<uintptr_t>(act_out)) & 15)
        return fail(FLY_E_ARG, "ppo_minibatch_gather: obs_out and act_out must be 16-byte aligned");
    // an output range that overlaps a source range (what can be seen from here; aliasing is forbidden altogether)
    const char* src[5] = {(const char*)obs, (const char*)act, (const char*)logp, (const char*)adv, (const char*)target};
    const char* dst[5] = {(const char*)obs_out, (const char*)act_out, (const char*)logp_out, (const char*)adv_out, (const char*)target_out};
    const int64_t width[5] = {73 * 4, 18 * 4, 4, 4, 4};
    for (int d = 0; d < 5; ++d)
        for (int s = 0; s < 5; ++s)
            if (dst[d] < src[s] + R * width[s] && src[s] < dst[d] + n * width[d])
                return fail(FLY_E_ARG, "ppo_minibatch_gather: an output overlaps a source");
    hipError_t e = flyhip_launch_minibatch_gather(obs, act, logp, adv, target, R, seed, epoch_key, first, n, obs_out, act_out, logp_out,
                                                  adv_out, target_out, index_out, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_minibatch_gather launch");
    return FLY_OK;
}

int ppo_noise_ar1(float* eps, float* carry, int64_t T, int64_t C, float rho, void* stream)
{
    if (!eps || !carry) return fail(FLY_E_ARG, "ppo_noise_ar1: null pointer");
    if (T <= 0 || C <= 0) return fail(FLY_E_ARG, "ppo_noise_ar1: T and C must be > 0");
    if (!(rho > 0.0f && rho < 1.0f)) return fail(FLY_E_ARG, "ppo_noise_ar1: rho must be in (0, 1) (got %g)", (double)rho);   // NaN too
    hipError_t e = flyhip_launch_noise_ar1(eps, carry, T, C, rho, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_noise_ar1 launch");
    return FLY_OK;
}

int fly_render(FlyHandle h, const float* poses, int32_t frames, const FlyRenderConfig* rc, uint32_t* rgba_out,
               uint8_t* id_out, void* stream)
{
    if (!h) return fail(FLY_E_ARG, "handle is null");
    if (!poses || !rc || !rgba_out) return fail(FLY_E_ARG, "fly_render: null pointer");
    if (frames < 1 || frames > 65535) return fail(FLY_E_ARG, "fly_render: frames out of range (%d)", frames);
    if (rc->width < 1 || rc->width > 4096 || rc->height < 1 || rc->height > 4096)
        return fail(FLY_E_ARG, "fly_render: image size out of range (%d x %d)", rc->width, rc->height);
    if (!(rc->fov_y_deg > 0.0f && rc->fov_y_deg < 180.0f)) return fail(FLY_E_ARG, "fly_render: fov_y_deg out of range");
    if (!(rc->cam_offset[0] != 0.0f || rc->cam_offset[1] != 0.0f))
        return fail(FLY_E_ARG, "fly_render: the camera must not look straight along z (cam_offset x, y both 0)");
    if ((reinterpret_cast<uintptr_t>(poses) | reinterpret_cast<uintptr_t>(rgba_out)) & 3)
        return fail(FLY_E_ARG, "fly_render: misaligned buffer");
    hipError_t e = flyhip_launch_render(h->dev, poses, frames, rc, rgba_out, id_out, stream);
    if (e != hipSuccess) return hip_fail(e, "fly_render launch");
    return FLY_OK;
}

int fly_scale_actions(FlyHandle h, const float* actions, float* targets, void* stream)
{
    FlyBuffers b = {};
    b.targets = targets;
    return launch(h, PH_SCALE, actions, &b, stream);
}

int fly_reset_masked(FlyHandle h, const FlyBuffers* b, void* stream) { return launch(h, PH_RESET, nullptr, b, stream); }
int fly_integrate(FlyHandle h, const FlyBuffers* b, void* stream) { return launch(h, PH_INTEGRATE, nullptr, b, stream); }
int fly_pack_obs(FlyHandle h, const FlyBuffers* b, void* stream) { return launch(h, PH_OBS, nullptr, b, stream); }
int fly_pack_reward(FlyHandle h, const FlyBuffers* b, int add_progress, void* stream)
{
    return launch(h, add_progress ? (PH_REWARD | PH_PROGRESS) : PH_REWARD, nullptr, b, stream);
}

int ppo_sample_logprob(const float* mu, const float* var, const float* eps, float* act_out,
                       float* logp_out, int64_t n, void* stream)
{
    if (!mu || !var || !eps || !act_out || !logp_out) return fail(FLY_E_ARG, "ppo_sample_logprob: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "ppo_sample_logprob: n must be > 0");
    hipError_t e = flyhip_launch_sample_logprob(mu, var, eps, act_out, logp_out, n, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_sample_logprob launch");
    return FLY_OK;
}

int ppo_td_gae(const float* reward, const float* v, const float* v_next, const float* done,
               float gamma, float lambda, int64_t T, int64_t N, float* target_out, float* adv_out,
               int mode_flags, void* stream)
{
    if (!reward || !v || !v_next || !done || !target_out || !adv_out) return fail(FLY_E_ARG, "ppo_td_gae: null pointer");
    if (T <= 0 || N <= 0) return fail(FLY_E_ARG, "ppo_td_gae: T and N must be > 0");
    if ((mode_flags & PPO_GAE_SCAN) && (mode_flags & PPO_GAE_MASK_RECURRENCE))
        return fail(FLY_E_ARG, "ppo_td_gae: PPO_GAE_SCAN does not implement the masked recurrence");
    hipError_t e = flyhip_launch_td_gae(reward, v, v_next, done, gamma, lambda, T, N, target_out, adv_out, mode_flags, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_td_gae launch");
    return FLY_OK;
}

int ppo_adv_stats(const float* adv, int64_t n, float* stats, void* stream)
{
    if (!adv || !stats || n <= 1) return fail(FLY_E_ARG, "ppo_adv_stats: bad argument");
    if (reinterpret_cast<uintptr_t>(stats) & 7) return fail(FLY_E_ARG, "ppo_adv_stats: stats is not 8-byte aligned");
    hipError_t e = flyhip_launch_adv_stats(adv, n, stats, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_adv_stats launch");
    return FLY_OK;
}

int ppo_adv_apply(float* adv, int64_t n, const float* totals, float count, float eps, void* stream)
{
    if (!adv || !totals || n <= 0 || !(count > 1.0f)) return fail(FLY_E_ARG, "ppo_adv_apply: bad argument");
    hipError_t e = flyhip_launch_adv_apply(adv, n, totals, count, eps, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_adv_apply launch");
    return FLY_OK;
}

int ppo_rollout_bookkeeping(const float* reward, int64_t rows, int64_t n, float* terms, float* score_acc,
                            float score_scale, float* action_var, int32_t nvar, float var_decay,
                            float var_min, int32_t* rows_applied, void* stream)
{
    if (!reward || !terms || !score_acc || !action_var) return fail(FLY_E_ARG, "ppo_rollout_bookkeeping: null pointer");
    if (rows < 0 || n <= 0 || nvar < 0 || nvar > 63) return fail(FLY_E_ARG, "ppo_rollout_bookkeeping: bad size");
    if (rows == 0) return FLY_OK;
    hipError_t e = flyhip_launch_rollout_bookkeeping(reward, rows, n, terms, score_acc, score_scale, action_var, nvar,
                                                     var_decay, var_min, rows_applied, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_rollout_bookkeeping launch");
    return FLY_OK;
}

int ppo_step_bookkeeping(const float* reward, int64_t n, float* score_acc, float score_scale,
                         float* action_var, int32_t nvar, float var_decay, float var_min, void* stream)
{
    if (!reward || !score_acc || !action_var) return fail(FLY_E_ARG, "ppo_step_bookkeeping: null pointer");
    if (n <= 0 || nvar < 0 || nvar > 256) return fail(FLY_E_ARG, "ppo_step_bookkeeping: bad size");
    hipError_t e = flyhip_launch_bookkeeping(reward, n, score_acc, score_scale, action_var, nvar, var_decay, var_min, stream);
    if (e != hipSuccess) return hip_fail(e, "ppo_step_bookkeeping launch");
    return FLY_OK;
}

int mlp_forward(const float* params, const float* params_frag, const float* x, int64_t n, float* mu_out, float* v_out,
                float* out_save, float* h1_save, float* h2_save, float* h3_save, const uint16_t* params_b3, void* stream)
{
    if (((uintptr_t)params_b3 & 15)) return fail(FLY_E_ARG, "mlp_forward: params_b3 must be 16-byte aligned");
    if (!params || !params_frag || !x) return fail(FLY_E_ARG, "mlp_forward: null params/x");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_forward: n must be > 0");
    if (((uintptr_t)params_frag & 15)) return fail(FLY_E_ARG, "mlp_forward: params_frag must be 16-byte aligned");
    hipError_t e = flyhip_launch_mlp_forward(params, params_frag, x, n, mu_out, v_out, out_save, h1_save, h2_save, h3_save,
                                             params_b3, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_forward launch");
    return FLY_OK;
}

int mlp_forward_sample(const float* params, const float* params_frag, const float* x, int64_t n,
                       const float* eps, const float* var, int32_t var_steps, float var_decay,
                       float var_min, float* act_out, float* logp_out, float* mu_out, float* v_out,
                       const uint16_t* params_b3, const int32_t* var_steps_base, void* stream)
{
    if (!params || !params_frag || !x || !eps || !var || !act_out || !logp_out)
        return fail(FLY_E_ARG, "mlp_forward_sample: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_forward_sample: n must be > 0");
    if (var_steps < 0 || var_steps > (1 << 20)) return fail(FLY_E_ARG, "mlp_forward_sample: var_steps out of range");
    hipError_t e = flyhip_launch_mlp_forward_sample(params, params_frag, x, n, eps, var, var_steps, var_decay, var_min, act_out, logp_out,
                                                    mu_out, v_out, params_b3, var_steps_base, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_forward_sample launch");
    return FLY_OK;
}

int64_t mlp_grad_workspace_floats(void) { return flyhip_mlp_grad_workspace_floats(); }

int mlp_backward_dx(const float* params_t, const float* out_saved, const float* h1_saved,
                    const float* h2_saved, const float* h3_saved, const float* action,
                    const float* old_logp, const float* adv, const float* target, const float* var,
                    int64_t n, float inv_batch, float clip, float* dz4, float* dz3, float* dz2,
                    float* dz1, float* loss_part, const uint16_t* params_t_b3, void* stream)
{
    if (!params_t || !out_saved || !h1_saved || !h2_saved || !h3_saved || !action || !old_logp || !adv ||
        !target || !var || !dz4 || !dz3 || !dz2 || !dz1)
        return fail(FLY_E_ARG, "mlp_backward_dx: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_backward_dx: n must be > 0");
    hipError_t e = flyhip_launch_mlp_backward_dx(params_t, out_saved, h1_saved, h2_saved, h3_saved, action, old_logp,
                                                 adv, target, var, n, inv_batch, clip, dz4, dz3, dz2, dz1, loss_part,
                                                 params_t_b3, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_backward_dx launch");
    return FLY_OK;
}

int mlp_forward_backward(const float* params, const float* params_frag, const float* params_t_frag,
                         const float* x, int64_t n, float* out_save, float* h1_save, float* h2_save,
                         float* h3_save, const float* action, const float* old_logp, const float* adv,
                         const float* target, const float* var, float inv_batch, float clip,
                         float* dz4, float* dz3, float* dz2, float* dz1, float* loss_part,
                         int32_t* flags, int32_t epoch, int32_t* err, const uint16_t* params_b3,
                         const uint16_t* params_t_b3, int32_t coherent, void* stream)
{
    if ((params_b3 == nullptr) != (params_t_b3 == nullptr))
        return fail(FLY_E_ARG, "mlp_forward_backward: params_b3 and params_t_b3 go together");
    if (!params || !params_frag || !params_t_frag || !x || !out_save || !h1_save || !h2_save || !h3_save || !action ||
        !old_logp || !adv || !target || !var || !dz4 || !dz3 || !dz2 || !dz1 || !flags || !err)
        return fail(FLY_E_ARG, "mlp_forward_backward: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_forward_backward: n must be > 0");
    if (epoch <= 0 || epoch >= (1 << 27)) return fail(FLY_E_ARG, "mlp_forward_backward: epoch must be in [1, 2^27)");
    hipError_t e = flyhip_launch_mlp_fwd_bwd(params, params_frag, params_t_frag, x, n, out_save, h1_save, h2_save, h3_save,
                                             action, old_logp, adv, target, var, inv_batch, clip, dz4, dz3, dz2, dz1,
                                             loss_part, flags, epoch, err, params_b3, params_t_b3, coherent, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_forward_backward launch");
    return FLY_OK;
}

int mlp_grad_w(const float* x, const float* h1_saved, const float* h2_saved, const float* h3_saved,
               const float* dz1, const float* dz2, const float* dz3, const float* dz4, int64_t n,
               float* workspace, float* grad, const float* norm_mask, float* norm_ws, int32_t* norm_step,
               const int32_t* err, int32_t gemm_b3, void* stream)
{
    if ((norm_ws != nullptr) != (norm_mask != nullptr) || (norm_ws != nullptr) != (norm_step != nullptr))
        return fail(FLY_E_ARG, "mlp_grad_w: norm_mask, norm_ws and norm_step go together");
    if (!x || !h1_saved || !h2_saved || !h3_saved || !dz1 || !dz2 || !dz3 || !dz4 || !workspace || !grad)
        return fail(FLY_E_ARG, "mlp_grad_w: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_grad_w: n must be > 0");
    hipError_t e = flyhip_launch_mlp_grad_w(x, h1_saved, h2_saved, h3_saved, dz1, dz2, dz3, dz4, n, workspace, grad, norm_mask,
                                            norm_ws, norm_step, err, gemm_b3, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_grad_w launch");
    return FLY_OK;
}

int64_t mlp_fused_workspace_floats(void) { return flyhip_mlp_fused_workspace_floats(); }

int mlp_fused_grad(const float* params, const uint16_t* params_b3, const uint16_t* params_t_b3, const float* x, int64_t n,
                   const float* action, const float* old_logp, const float* adv, const float* target, const float* var,
                   float inv_batch, float clip, float* workspace, float* grad, const float* norm_mask, float* norm_ws,
                   int32_t* norm_step, float* loss_part, float* const* debug_dump, void* stream)
{
    if ((norm_ws != nullptr) != (norm_mask != nullptr) || (norm_ws != nullptr) != (norm_step != nullptr))
        return fail(FLY_E_ARG, "mlp_fused_grad: norm_mask, norm_ws and norm_step go together");
    if (!params || !params_b3 || !params_t_b3) return fail(FLY_E_ARG, "mlp_fused_grad: needs params and both bf16x3 plane buffers");
    if (!x || !action || !old_logp || !adv || !target || !var || !workspace || !grad)
        return fail(FLY_E_ARG, "mlp_fused_grad: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_fused_grad: n must be > 0");
    if (debug_dump) {
        if (!debug_dump[0]) return fail(FLY_E_ARG, "mlp_fused_grad: debug_dump[0] is null");
        if (debug_dump[1])      // the chain dump: all eight; {stamps, NULL}: the diagnostic stamp build (tools/stamp_fused.py)
            for (int i = 2; i < 8; ++i)
                if (!debug_dump[i]) return fail(FLY_E_ARG, "mlp_fused_grad: debug_dump[%d] is null", i);
    }
    hipError_t e = flyhip_launch_mlp_fused_grad(params, params_b3, params_t_b3, x, n, action, old_logp, adv, target, var, inv_batch,
                                                clip, workspace, grad, norm_mask, norm_ws, norm_step, loss_part, debug_dump, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_fused_grad launch");
    return FLY_OK;
}

int64_t mlp_fused_h2_workspace_floats(void) { return flyhip_mlp_fused_h2_workspace_floats(); }

int mlp_h2_rescale(const float* params, const int32_t* idx_b3, const int32_t* idx_t_b3, uint16_t* params_h2, uint16_t* params_t_h2,
                   float* h2_scales, void* stream)
{
    if (!params || !idx_b3 || !idx_t_b3 || !params_h2 || !params_t_h2 || !h2_scales) return fail(FLY_E_ARG, "mlp_h2_rescale: null pointer");
    hipError_t e = flyhip_launch_mlp_h2_rescale(params, idx_b3, idx_t_b3, params_h2, params_t_h2, h2_scales, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_h2_rescale launch");
    return FLY_OK;
}

int mlp_fused_grad_h2(const float* params, const uint16_t* params_h2, const uint16_t* params_t_h2, float* h2_scales,
                      int32_t* h2_overflow, int32_t freeze, const float* x, int64_t n, const float* action,
                      const float* old_logp, const float* adv, const float* target, const float* var, float inv_batch,
                      float clip, float* workspace, float* grad, const float* norm_mask, float* norm_ws, int32_t* norm_step,
                      float* loss_part, float* const* debug_dump, void* stream)
{
    if ((norm_ws != nullptr) != (norm_mask != nullptr) || (norm_ws != nullptr) != (norm_step != nullptr))
        return fail(FLY_E_ARG, "mlp_fused_grad_h2: norm_mask, norm_ws and norm_step go together");
    if (!params || !params_h2 || !params_t_h2 || !h2_scales || !h2_overflow)
        return fail(FLY_E_ARG, "mlp_fused_grad_h2: needs params, both fp16x2 plane buffers, the scale table and the overflow word");
    if (!x || !action || !old_logp || !adv || !target || !var || !workspace || !grad)
        return fail(FLY_E_ARG, "mlp_fused_grad_h2: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "mlp_fused_grad_h2: n must be > 0");
    if (debug_dump) {
        if (!debug_dump[0]) return fail(FLY_E_ARG, "mlp_fused_grad_h2: debug_dump[0] is null");
        if (debug_dump[1])
            for (int i = 2; i < 8; ++i)
                if (!debug_dump[i]) return fail(FLY_E_ARG, "mlp_fused_grad_h2: debug_dump[%d] is null", i);
    }
    hipError_t e = flyhip_launch_mlp_fused_grad_h2(params, params_h2, params_t_h2, h2_scales, h2_overflow, freeze, x, n, action, old_logp,
                                                   adv, target, var, inv_batch, clip, workspace, grad, norm_mask, norm_ws, norm_step,
                                                   loss_part, debug_dump, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_fused_grad_h2 launch");
    return FLY_OK;
}

int mlp_adam_step(float* params, float* params_frag, float* params_t_frag, const int32_t* idx_frag,
                  const int32_t* idx_t_frag, const float* grad, const float* mask, float* exp_avg,
                  float* exp_avg_sq, int32_t* step, float lr, float beta1, float beta2, float eps,
                  float max_norm, float grad_scale, float* norm_ws, int32_t norm_ready, uint16_t* params_b3,
                  uint16_t* params_t_b3, const int32_t* idx_b3, const int32_t* idx_t_b3, int32_t* step_out,
                  const int32_t* grad_invalid, uint16_t* params_h2, uint16_t* params_t_h2, float* h2_scales, int32_t h2_period,
                  void* stream)
{
    if (params_b3 && (!params_t_b3 || !idx_b3 || !idx_t_b3))
        return fail(FLY_E_ARG, "mlp_adam_step: params_b3 needs params_t_b3, idx_b3 and idx_t_b3");
    if (params_h2 && (!params_t_h2 || !h2_scales || !params_b3))
        return fail(FLY_E_ARG, "mlp_adam_step: params_h2 needs params_t_h2, h2_scales and the bf16x3 planes with their index maps");
    if (!params || !params_frag || !params_t_frag || !idx_frag || !idx_t_frag || !grad || !mask || !exp_avg ||
        !exp_avg_sq || !step || !norm_ws)
        return fail(FLY_E_ARG, "mlp_adam_step: null pointer");
    hipError_t e = flyhip_launch_mlp_adam(params, params_frag, params_t_frag, idx_frag, idx_t_frag, grad, mask, exp_avg, exp_avg_sq, step, lr, beta1, beta2,
                                          eps, max_norm, grad_scale, norm_ws, norm_ready, params_b3, params_t_b3, idx_b3, idx_t_b3,
                                          step_out, grad_invalid, params_h2, params_t_h2, h2_scales, h2_period, stream);
    if (e != hipSuccess) return hip_fail(e, "mlp_adam_step launch");
    return FLY_OK;
}

int dqn_eps_greedy(const float* q, const float* coin_u, const float* rand_u, float epsilon, int32_t A,
                   float* act_out, int64_t n, void* stream)
{
    if (!q || !coin_u || !rand_u || !act_out) return fail(FLY_E_ARG, "dqn_eps_greedy: null pointer");
    if (n <= 0 || A < 2) return fail(FLY_E_ARG, "dqn_eps_greedy: need n > 0 and A >= 2");
    hipError_t e = flyhip_launch_dqn_eps_greedy(q, coin_u, rand_u, epsilon, A, act_out, n, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_eps_greedy launch");
    return FLY_OK;
}

int dqn_huber_td(const float* q_table, const float* act, const float* reward, const float* q_next,
                 const float* done, float discount, int32_t A, int64_t B, float* dq, float* loss_part,
                 void* stream)
{
    if (!q_table || !act || !reward || !q_next || !done || !dq || !loss_part)
        return fail(FLY_E_ARG, "dqn_huber_td: null pointer");
    if (B <= 0 || A < 2) return fail(FLY_E_ARG, "dqn_huber_td: need B > 0 and A >= 2");
    hipError_t e = flyhip_launch_dqn_huber_td(q_table, act, reward, q_next, done, discount, A, B, dq, loss_part, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_huber_td launch");
    return FLY_OK;
}

int dqn_forward(const float* params, const float* params_frag, const float* x, int64_t n, float* q_out, void* stream)
{
    if (!params || !params_frag || !x || !q_out) return fail(FLY_E_ARG, "dqn_forward: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "dqn_forward: n must be > 0");
    hipError_t e = flyhip_launch_dqn_forward(params, params_frag, x, n, q_out, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_forward launch");
    return FLY_OK;
}

int dqn_act(const float* params, const float* params_frag, const float* x, int64_t n, const float* coin_u,
            const float* rand_u, float epsilon, float* act_out, float* q_out, void* stream)
{
    if (!params || !params_frag || !x || !coin_u || !rand_u || !act_out) return fail(FLY_E_ARG, "dqn_act: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "dqn_act: n must be > 0");
    hipError_t e = flyhip_launch_dqn_act(params, params_frag, x, n, coin_u, rand_u, epsilon, act_out, q_out, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_act launch");
    return FLY_OK;
}

int dqn_td_step(const float* params, const float* params_frag, const float* params_t_frag,
                const float* target_params, const float* target_params_frag, const float* obs,
                const float* next_obs, const float* act, const float* reward, const float* done, int64_t n,
                float discount, float inv_B, float* h1, float* h2, float* dz3, float* dz2, float* dz1,
                float* loss_part, void* stream)
{
    if (!params || !params_frag || !params_t_frag || !target_params || !target_params_frag || !obs || !next_obs || !act ||
        !reward || !done || !h1 || !h2 || !dz3 || !dz2 || !dz1 || !loss_part)
        return fail(FLY_E_ARG, "dqn_td_step: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "dqn_td_step: n must be > 0");
    hipError_t e = flyhip_launch_dqn_td(params, params_frag, params_t_frag, target_params, target_params_frag, obs, next_obs,
                                        act, reward, done, n, discount, inv_B, h1, h2, dz3, dz2, dz1, loss_part, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_td_step launch");
    return FLY_OK;
}

int64_t dqn_grad_workspace_floats(void) { return flyhip_dqn_grad_workspace_floats(); }

int dqn_grad_w(const float* x, const float* h1, const float* h2, const float* dz1, const float* dz2,
               const float* dz3, int64_t n, float* workspace, float* grad, int32_t accumulate, void* stream)
{
    if (!x || !h1 || !h2 || !dz1 || !dz2 || !dz3 || !workspace || !grad) return fail(FLY_E_ARG, "dqn_grad_w: null pointer");
    if (n <= 0) return fail(FLY_E_ARG, "dqn_grad_w: n must be > 0");
    hipError_t e = flyhip_launch_dqn_grad_w(x, h1, h2, dz1, dz2, dz3, n, workspace, grad, accumulate, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_grad_w launch");
    return FLY_OK;
}

int dqn_adam_soft_update(float* params, float* params_frag, float* params_t_frag, float* target_params,
                         float* target_params_frag, const int32_t* idx_frag, const int32_t* idx_t_frag,
                         const float* grad, const float* mask, float* exp_avg, float* exp_avg_sq, int32_t* step,
                         float lr, float beta1, float beta2, float eps, float tau, uint16_t* params_b3, uint16_t* params_t_b3,
                         uint16_t* target_params_b3, const int32_t* idx_b3, const int32_t* idx_t_b3, const int32_t* grad_invalid,
                         void* stream)
{
    if (!params || !params_frag || !params_t_frag || !target_params || !target_params_frag || !idx_frag || !idx_t_frag ||
        !grad || !mask || !exp_avg || !exp_avg_sq || !step)
        return fail(FLY_E_ARG, "dqn_adam_soft_update: null pointer");
    if (params_b3 && (!params_t_b3 || !target_params_b3 || !idx_b3 || !idx_t_b3))
        return fail(FLY_E_ARG, "dqn_adam_soft_update: params_b3 needs params_t_b3, target_params_b3, idx_b3 and idx_t_b3");
    hipError_t e = flyhip_launch_dqn_adam(params, params_frag, params_t_frag, target_params, target_params_frag, idx_frag,
                                          idx_t_frag, grad, mask, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, tau,
                                          params_b3, params_t_b3, target_params_b3, idx_b3, idx_t_b3, grad_invalid, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_adam_soft_update launch");
    return FLY_OK;
}

int64_t dqn_fused_workspace_floats(void) { return flyhip_dqn_fused_workspace_floats(); }
int64_t dqn_fused_image_halves(int64_t rows) { return flyhip_dqn_fused_image_halves(rows); }

int dqn_fused_update(const float* params, const uint16_t* params_b3, const uint16_t* params_t_b3, const float* target_params,
                     const uint16_t* target_params_b3, const void* chunks, int32_t num_chunks, int64_t n, float discount, float inv_B,
                     uint16_t* images, float* workspace, float* grad, float* loss_part, int32_t rows_aligned16, void* stream)
{
    if (!params || !params_b3 || !params_t_b3 || !target_params || !target_params_b3 || !chunks || !images || !workspace || !grad ||
        !loss_part)
        return fail(FLY_E_ARG, "dqn_fused_update: null pointer");
    if (num_chunks <= 0 || n <= 0 || (n % 32) != 0)
        return fail(FLY_E_ARG, "dqn_fused_update: needs num_chunks > 0 and n a positive multiple of 32 (whole tiles; use dqn_td_step + dqn_grad_w otherwise)");
    hipError_t e = flyhip_launch_dqn_fused_update(params, params_b3, params_t_b3, target_params, target_params_b3, chunks, num_chunks, n,
                                                  discount, inv_B, images, workspace, grad, loss_part, rows_aligned16 ? 1 : 0, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_fused_update launch");
    return FLY_OK;
}

int64_t dqn_fused_h2_workspace_floats(void) { return flyhip_dqn_fused_h2_workspace_floats(); }
int64_t dqn_fused_h2_image_halves(int64_t rows) { return flyhip_dqn_fused_h2_image_halves(rows); }

int dqn_fused_update_h2(const float* params, uint16_t* params_h2, uint16_t* params_t_h2, const float* target_params,
                        uint16_t* target_params_h2, const int32_t* idx_b3, const int32_t* idx_t_b3, float* h2_scales,
                        int32_t* h2_overflow, const void* chunks, int32_t num_chunks, int64_t n, float discount, float inv_B,
                        uint16_t* images, float* workspace, float* grad, float* loss_part, int32_t rows_aligned16, int32_t flags,
                        void* stream)
{
    if (!params || !params_h2 || !params_t_h2 || !target_params || !target_params_h2 || !idx_b3 || !idx_t_b3 || !h2_scales ||
        !h2_overflow || !chunks || !images || !workspace || !grad || !loss_part)
        return fail(FLY_E_ARG, "dqn_fused_update_h2: null pointer");
    if (num_chunks <= 0 || n <= 0 || (n % 32) != 0)
        return fail(FLY_E_ARG, "dqn_fused_update_h2: needs num_chunks > 0 and n a positive multiple of 32 (whole tiles; use dqn_td_step + dqn_grad_w otherwise)");
    if (!(inv_B > 0.0f) || !(inv_B < 1.0e30f)) return fail(FLY_E_ARG, "dqn_fused_update_h2: inv_B must be a positive finite number");
    hipError_t e = flyhip_launch_dqn_fused_update_h2(params, params_h2, params_t_h2, target_params, target_params_h2, idx_b3, idx_t_b3,
                                                     h2_scales, h2_overflow, chunks, num_chunks, n, discount, inv_B, images, workspace, grad,
                                                     loss_part, rows_aligned16 ? 1 : 0, flags & 7, stream);
    if (e != hipSuccess) return hip_fail(e, "dqn_fused_update_h2 launch");
    return FLY_OK;
}

int dp_p2p_alloc(int64_t n_floats, void** window_out)
{
    if (!window_out || n_floats <= 0 || (n_floats & 3)) return fail(FLY_E_ARG, "dp_p2p_alloc: need a pointer and n_floats a positive multiple of 4");
    hipError_t e = flyhip_p2p_alloc(n_floats, window_out);
    if (e != hipSuccess) return hip_fail(e, "dp_p2p_alloc");
    return FLY_OK;
}

int dp_p2p_free(void* window)
{
    if (!window) return FLY_OK;
    hipError_t e = hipFree(window);
    if (e != hipSuccess) return hip_fail(e, "dp_p2p_free");
    return FLY_OK;
}

int dp_ipc_export(const void* window, uint8_t handle_out[64])
{
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    if (!window || !handle_out) return fail(FLY_E_ARG, "dp_ipc_export: null pointer");
    hipIpcMemHandle_t h;
    hipError_t e = hipIpcGetMemHandle(&h, const_cast<void*>(window));
    if (e != hipSuccess) return hip_fail(e, "hipIpcGetMemHandle");
    memcpy(handle_out, &h, 64);
    return FLY_OK;
}

int dp_ipc_import(const uint8_t handle[64], void** window_out)
{
    if (!handle || !window_out) return fail(FLY_E_ARG, "dp_ipc_import: null pointer");
    hipIpcMemHandle_t h;
    memcpy(&h, handle, 64);
    hipError_t e = hipIpcOpenMemHandle(window_out, h, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) return hip_fail(e, "hipIpcOpenMemHandle");
    return FLY_OK;
}

int dp_ipc_close(void* window)
{
    if (!window) return FLY_OK;
    hipError_t e = hipIpcCloseMemHandle(window);
    if (e != hipSuccess) return hip_fail(e, "hipIpcCloseMemHandle");
    return FLY_OK;
}

int dp_allreduce_p2p(float* grad, int64_t n_floats, void* const* windows, int32_t rank, int32_t world, uint32_t epoch,
                     int32_t* err, int64_t fail_slot, void* stream)
{
    if (fail_slot >= n_floats) return fail(FLY_E_ARG, "dp_allreduce_p2p: fail_slot outside the buffer");
    if (!grad || !windows || !err) return fail(FLY_E_ARG, "dp_allreduce_p2p: null pointer");
    if (world < 1 || world > 16 || rank < 0 || rank >= world) return fail(FLY_E_ARG, "dp_allreduce_p2p: bad rank / world (max 16)");
    if (n_floats <= 0 || (n_floats & 3)) return fail(FLY_E_ARG, "dp_allreduce_p2p: n_floats must be a positive multiple of 4");
    if (n_floats / 4 > 1024L * 256) return fail(FLY_E_ARG, "dp_allreduce_p2p: buffer too large for a co-resident grid");
    if (epoch == 0) return fail(FLY_E_ARG, "dp_allreduce_p2p: epochs start at 1");
    for (int r = 0; r < world; ++r)
        if (!windows[r]) return fail(FLY_E_ARG, "dp_allreduce_p2p: window %d is null", r);
    hipError_t e = flyhip_launch_p2p_allreduce(grad, n_floats, windows, rank, world, epoch, err, fail_slot, stream);
    if (e != hipSuccess) return hip_fail(e, "dp_allreduce_p2p launch");
    return FLY_OK;
}

}  // extern "C"
