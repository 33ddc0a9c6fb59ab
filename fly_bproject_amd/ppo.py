"""`Net` and `PPO`: the reference's agent (ppo.py:10-285) on the MI355X-native environment.

Same classes, attributes and methods as the reference (`PPO(args)`, `.run() -> bool`, `.update()`,
`.make_data()`, `.save(suffix)`, `.net.pi/.v`, state-dict keys `shared_net.{0,2}`,
`to_mean.{0,2}`, `to_value.{0,2}`), same hyper-parameters and the same quirks,
each named where it is reproduced.

What changed underneath (MI355X-first, not a translation):
  * rollout rows live in one ring `[T+1, N, 73]`; `all_obs = ring[:T]`, `all_next_obs = ring[1:]`
    are views (next_obs[t] is obs[t+1] by construction, ppo.py:210/:228), and the env kernel
    writes each observation row straight into the ring (`Fly.bind_obs`), so the two 2.4 MB
    row copies per step are gone;
  * the policy forward, sampling, log-prob and clip are ONE launch writing the action / log-prob rows
    of the rollout in place (`mlp_forward_sample`);
  * TD target + GAE is one kernel (`ppo_td_gae`) instead of a T-long Python loop, and the two
    critic passes over the rollout collapse into one pass over the ring;
  * no per-step host sync: the score accumulates on the device and is read every
    `num_eval_freq` steps, when it is printed;
  * the update runs on the MFMA kernels of csrc/mlp_mfma.hip (forward, loss + dX chain, dW, clip +
    Adam) over contiguous minibatch slices of the rollout;
  * data-parallel training: one packed-gradient all-reduce over RCCL per optimizer step.
"""
import ctypes as C
import collections
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, options, train_state
from .fly import Fly
from .params import NUM_DOF



class Net(nn.Module):
    """ppo.py:10-102: shared 73-256-128 (ELU); actor 128-64-18 with ELU after BOTH layers;
    critic 128-64-1.  `pi` and `v` each run the shared trunk."""

    def __init__(self, num_obs, num_act):
        super().__init__()
        self.shared_net = nn.Sequential(nn.Linear(num_obs, 256), nn.ELU(), nn.Linear(256, 128), nn.ELU())
        self.to_mean = nn.Sequential(nn.Linear(128, 64), nn.ELU(), nn.Linear(64, num_act), nn.ELU())
        self.to_value = nn.Sequential(nn.Linear(128, 64), nn.ELU(), nn.Linear(64, 1))

    _policy = None      # PackedPolicy, attached by PPO: inference then runs on the MFMA kernel

    def pi(self, x):
        if self._policy is not None and not torch.is_grad_enabled():
            return self._policy.forward(x, want_mu=True, want_v=False)[0]
        return self.to_mean(self.shared_net(x))

    def v(self, x):
        if self._policy is not None and not torch.is_grad_enabled():
            return self._policy.forward(x, want_mu=False, want_v=True)[1]
        return self.to_value(self.shared_net(x))


def diag_gauss_logprob(mu, action, var):
    """log N(action; mu, diag(var)) exactly as MultivariateNormal(mu, scale_tril=cholesky(diag(var)))
    evaluates it (ppo.py:185-189): -0.5 (k log 2pi + |L^-1 (a-mu)|^2) - sum log L_jj."""
    L = torch.sqrt(var)
    x = (action - mu) / L
    M = (x * x).sum(-1)
    half_log_det = torch.log(L).sum(-1)
    return -0.5 * (mu.shape[-1] * 1.8378770664093453 + M) - half_log_det


OBS_RMS_KEYS = ("obs_rms.mean", "obs_rms.var", "obs_rms.count")
VALUE_RMS_KEYS = ("value_rms.mean", "value_rms.var", "value_rms.count")
REWARD_RMS_KEYS = ("reward_rms.mean", "reward_rms.var", "reward_rms.count")


def _split_rms(state_dict, keys, on, what, flag):
    """Remove the `what` statistics (`keys`, one prefix) from a loaded state dict, in place, and return them: the rest then
    loads strictly into Net (a reference checkpoint has none).  Statistics while the option is not `on` are an error."""
    prefix = keys[0].split(".")[0] + "."
    rms = {k: state_dict.pop(k) for k in list(state_dict) if k.startswith(prefix)}
    if rms and not on:
        raise ValueError("this checkpoint was trained with %s normalisation (it holds %s): run with --%s"
                         % (what, ", ".join(sorted(rms)), flag))
    if rms and sorted(rms) != sorted(keys):
        raise ValueError("incomplete %s statistics in the checkpoint: %s (want %s)" % (what, sorted(rms), list(keys)))
    return rms


def split_obs_rms(state_dict, normalize_obs):
    """The observation statistics (obs_rms.*) out of a loaded state dict.  Without `normalize_obs` they are an error: the
    network was trained on normalised inputs."""
    return _split_rms(state_dict, OBS_RMS_KEYS, normalize_obs, "observation", "normalize_obs")


def split_value_rms(state_dict, normalize_value):
    """The value statistics (value_rms.*) out of a loaded state dict.  Without `normalize_value` they are an error: the critic
    was trained on normalised targets, its outputs are not in reward units."""
    return _split_rms(state_dict, VALUE_RMS_KEYS, normalize_value, "value", "normalize_value")


def split_reward_rms(state_dict, normalize_reward):
    """The return statistics (reward_rms.*) out of a loaded state dict.  Without `normalize_reward` they are an error: the
    critic was trained on scaled rewards, its outputs are not in reward units."""
    return _split_rms(state_dict, REWARD_RMS_KEYS, normalize_reward, "reward", "normalize_reward")


def value_norm_table(stats):
    """The table the value-normalisation kernels read, from S_v = count | mean | var (float64): m = (float) mean,
    s = (float) sqrt(var + 1e-5), r = (float) (1 / sqrt(var + 1e-5)), 0 -- each rounded once from float64 (what
    ppo_value_norm_merge writes)."""
    mean, sd = stats[1].double(), torch.sqrt(stats[2].double() + 1e-5)
    return torch.stack((mean.float(), sd.float(), (1.0 / sd).float(), torch.zeros((), dtype=torch.float32, device=stats.device)))


def obs_norm_table(stats, clip):
    """The table the kernels read, from S = count | mean[k] | var[k] (float64): m = (float) mean, r = (float) (1 / sqrt(var +
    1e-5)), clip -- each rounded once from float64 (what ppo_obs_norm_merge writes)."""
    k = (stats.numel() - 1) // 2
    mean, var = stats[1:1 + k].double(), stats[1 + k:].double()
    return torch.cat((mean.float(), (1.0 / torch.sqrt(var + 1e-5)).float(),
                      torch.full((1,), clip, dtype=torch.float32, device=stats.device)))


def normalize_obs_ref(x, table):
    """torch's statement of the kernels' normalisation: ((x - m) * r).clamp(-clip, clip), NaN passing through."""
    k = (table.numel() - 1) // 2
    clip = float(table[2 * k])
    return ((x - table[:k]) * table[k:2 * k]).clamp(-clip, clip)


def update_stats_entries(s):
    """One set of update statistics (FLY_UPDATE_STATS_SET numbers, include/flyhip_update_stats.h) as agent.update_stats()
    reports it: Python numbers; means are over the finite rows, and without one everything but the two counts is nan."""
    rows, bad = int(s[0]), int(s[14])
    n = rows - bad
    nan = float("nan")
    if n <= 0:
        out = dict.fromkeys(("approx_kl", "kl_k1", "clip_fraction", "ratio_min", "ratio_max", "policy_loss", "value_loss", "loss",
                             "explained_variance", "target_mean", "target_std", "adv_absmax", "target_absmax"), nan)
        return dict(out, rows=rows, nonfinite=bad)
    pol, hub, m2 = float(s[6]) / n, float(s[7]) / n, float(s[10])
    return {"rows": rows, "nonfinite": bad, "approx_kl": float(s[2]) / n, "kl_k1": float(s[1]) / n,
            "clip_fraction": float(s[3]) / n, "ratio_min": float(s[4]), "ratio_max": float(s[5]), "policy_loss": pol,
            "value_loss": hub, "loss": pol + hub, "explained_variance": 1.0 - float(s[13]) / m2 if m2 > 0.0 else nan,
            "target_mean": float(s[9]), "target_std": (max(m2, 0.0) / n) ** 0.5, "adv_absmax": float(s[15]),
            "target_absmax": float(s[16])}


def update_stats_suffix(w):
    """' | KL ... | Clip ...% | EV ... | Loss ...' of the score line from a set's numbers; ' | KL n/a' for a set without rows."""
    if int(w[0]) == 0:
        return " | KL n/a"
    e = update_stats_entries(w)
    text = " | KL {:.5f} | Clip {:.1f}% | EV {:.3f} | Loss {:.4f}".format(e["approx_kl"], 100.0 * e["clip_fraction"],
                                                                        e["explained_variance"], e["loss"])
    return text + (" | Nonfinite {}".format(e["nonfinite"]) if e["nonfinite"] > 0 else "")


def update_stats_empty():
    """The empty set of update statistics."""
    inf = float("inf")
    return torch.tensor([0.0, 0.0, 0.0, 0.0, inf, -inf] + [0.0] * 11, dtype=torch.float64)


def combine_adv_stats(ranks, count):
    """The all-rank (sum, M2) of the advantages from every rank's ppo_adv_stats pair: `ranks` [world][2] holds
    (sum_r, M2_r) over `count` elements each, M2 the centred second moment.  M2 = sum_r M2_r + count (mean_r - mean)^2
    (Chan et al.'s update for equal counts), in float64 on the device, rounded once: what ppo_adv_apply takes as totals."""
    r = ranks.to(torch.float64)
    total = r[:, 0].sum()
    mean = total / (count * r.shape[0])
    m2 = r[:, 1].sum() + count * ((r[:, 0] / count - mean) ** 2).sum()
    return torch.stack((total, m2)).to(torch.float32)


class PPO:
    def __init__(self, args, env=None):
        self.args = args
        self._book_terms = None                                     # nothing to flush until _prepare_step_args
        # every option, resolved and validated once and first (options.py): a bad value must not leave an env behind.  Only what
        # callers flip on a live agent is read from `args` later, when it is used: testing, save, save_path, save_freq,
        # save_state, load_path.
        opts = self.options = options.resolve(args, os.environ)
        self.gae, self.minibatch = opts.gae, opts.minibatch
        self.action_noise, self.noise_rho = opts.action_noise, opts.noise_rho
        # opt-in (`resume`, trainer.py --resume_path): the run continues the one that wrote `resume_path` with `save_state`, bit
        # for bit.  The state file is read and its meta held against these args HERE, before the env exists: a
        # state of another shape or option must not leave an env behind either.  load_training_state() applies it.
        self._resume_state = None
        if opts.resume:
            self._resume_state = train_state.read_state_file(self.training_state_path(opts.resume_path, opts.rank))
            train_state.check_meta(self._resume_state.get("meta"), args)
            train_state.check_meta_ext(self._resume_state.get("meta_ext"), args)
            train_state.check_reward_norm(self._resume_state, opts.normalize_reward)
        self.env = env if env is not None else Fly(args)           # ppo.py:110
        self.num_acts = self.env.num_act
        self.num_obs = self.env.num_obs
        self.epoch = 5
        self.lr = 0.001
        self.gamma = 0.99
        self.lmbda = 0.95
        self.clip = 0.2
        self.mini_batch_size = options.MINI_BATCH_SIZE
        self.chuck_number = options.CHUNK_NUMBER
        n = opts.num_envs
        self.mini_chunk_size = opts.mini_chunk_size                 # ppo.py:120 (Q9: 0 for N > 40960, refused by the resolver)
        print("mini_chunk_size: ", self.mini_chunk_size)
        self.rollout_size = opts.rollout_size
        print("rollout_size: ", self.rollout_size)
        self.num_eval_freq = 100
        self.mini_batch_number = 0

        dev = self.device = self.env.device
        T = self.rollout_size
        # ppo.py:132-138, with all_obs / all_next_obs as two views of one ring
        self._obs_ring = torch.zeros((T + 1, n, self.num_obs), device=dev)
        self.all_obs = self._obs_ring[:T]
        self.all_next_obs = self._obs_ring[1:]
        # v(obs_t) falls out of the rollout's policy launch (same kernel, same weights, same rows as the
        # critic pass of ppo.py:158-159), so make_data only has to evaluate the last next_obs
        self._v_ring = torch.zeros((T + 1, n, 1), device=dev)
        self._v_have, self._v_version = 0, -1
        self.reuse_rollout_values = opts.reuse_rollout_values
        self.all_acts = torch.zeros((T, n, self.num_acts), device=dev)
        self.all_reward = torch.zeros((T, n, 1), device=dev)
        self._all_done = None                                        # see the all_done property (Q1)
        self.all_log_prob = torch.zeros((T, n), device=dev)
        self.all_advantage = torch.zeros((T, n, 1), device=dev)
        self._target = torch.zeros((T, n, 1), device=dev)
        self._eps_all = torch.zeros((T, n, self.num_acts), device=dev)   # one normal_() per rollout
        self._mu = torch.zeros((n, self.num_acts), device=dev)
        self.normalize_advantage = opts.normalize_advantage
        self._adv_stats = torch.zeros(514, device=dev)
        # opt-in (`normalize_obs`, rl_games' normalize_input): the policy sees clamp((obs - mean) * rsqrt(var + 1e-5), +-obs_clip)
        # under running statistics of the observations.  The ring keeps the raw rows; see _setup_obs_norm.
        self.normalize_obs, self.obs_clip = opts.normalize_obs, opts.obs_clip
        # opt-in (`normalize_value`, rl_games' normalize_value): the critic regresses on TD targets kept at zero mean / unit
        # variance by running statistics, and make_data maps its outputs back to reward units
        self.normalize_value = opts.normalize_value
        # opt-in (`lambda_returns`, rl_games' / SB3's `returns`): the critic regresses on the lambda-return A_t + V(s_t) of the
        # estimator in use, made by one launch behind the unchanged GAE kernel.  NOT the reference's critic
        # target (the one-step TD target, ppo.py:160).
        self.lambda_returns = opts.lambda_returns
        # opt-in (`gae="episodic"`): per-step end flags, a recurrence that stops at episode ends, a bootstrap through time-outs
        # and no training signal from the step that performs a reset.  NOT the reference's estimator (Q1/Q2).
        # (self.gae, above)
        self.use_graph = opts.graph
        # one launch per ROLLOUT (ppo_rollout_all): each workgroup loops over the T steps of its own 32 envs.  The device then
        # runs ahead of the host's step count inside a rollout, but everything `run()` reads per step is a ROW the launch wrote
        # for that step: observation / reward / action / log-prob rows as always, and `env.reset_buf` / `env.progress_buf`
        # (fly.py:175-177) are re-pointed at row t of per-step [T, N] tensors -- so it is the default whenever one launch stays
        # short (T <= 4096 steps; the reference's 16-env shape, T = 40 960, steps launch by launch).  `persistent_rollout=False`
        # (or its environment variable at 0, options.py) keeps one launch per step; the env's STATE tensors (root_tensor,
        # dof_states, ...) show the rollout's end while the host is still counting through it.
        self.persistent_rollout = opts.persistent_rollout
        self._reset_rows = self._progress_rows = self._ended_prev = None
        if self.gae == "episodic":
            # the end flags the env carries into the first rollout: its initial reset_buf (every env resets in its first step)
            self._flag_rows()
            self._ended_prev = self.env.reset_buf.clone()
        # opt-in (`episode_stats`): return and length of the episodes that finish, from the reward and flag rows at the end of
        # every rollout, on the score line and through episode_stats().  It observes: nothing the rollout or
        # the update reads is written.
        self._episode_stats = opts.episode_stats
        if self._episode_stats:
            self._setup_episode_stats()
        # opt-in (`update_stats`): how far the finished update moved the policy, how much of the surrogate was clipped and how
        # well the critic fits its targets, from one forward of the updated network over the rollout's rows and one reduction
        # behind every update, on the score line and through update_stats().  It observes, as episode_stats.
        self._update_stats = opts.update_stats
        if self._update_stats:
            self._setup_update_stats()
        # opt-in (`normalize_reward`, gymnasium's NormalizeReward / SB3's norm_reward): the GAE pass reads the rewards divided by
        # the running standard deviation of the discounted return, clamped to +-reward_clip.  all_reward keeps
        # the raw rows: score line, episode statistics and recorder read what they always did.  See _setup_reward_norm.
        self.normalize_reward, self.reward_clip = opts.normalize_reward, opts.reward_clip
        # opt-in (`minibatch="shuffled"`): every epoch draws its 15 minibatches from a fresh keyed permutation of ALL T * N rows
        # of the rollout, gathered into one staging set in front of the unchanged optimizer-step kernels.  NOT
        # the reference's contiguous-in-time slices (Q3).  Nothing of it goes into the weights file; `--save_state` carries it
        # (the count of updates, and with it the epoch keys).
        self._mb_stage = self._mb_index = None
        if self.minibatch == "shuffled":
            self._setup_minibatch()
        # opt-in (`action_noise="ar1"`): the rollout's noise is an AR(1) process along time with unit stationary variance, made
        # by one filter launch over `_eps_all` right behind the white draw.  NOT the reference's sampling.  The
        # carry [N, 18] is the process' last row: drawn once before the first rollout (`_draw_noise`), then handed from rollout
        # to rollout by the launch.  Nothing of it goes into the weights file (`--save_state` carries it) or to another rank.
        self._noise_carry, self._noise_carry_drawn = None, False
        if self.action_noise == "ar1":
            self._noise_carry = torch.zeros((n, self.num_acts), device=dev)
        self._graphs = {}
        self._graphs_form = getattr(self.env, "launch_form", 0)     # the env's kernel selection the captured graphs hold
        self._fwd_args = None
        self._score_acc = torch.zeros((), device=dev)
        # The reference prints its score line from a host read of device values (ppo.py:257-260).  A blocking read in the middle
        # of a rollout that runs as ONE launch stalls the host until the launch ends, and the device then idles while the host
        # walks the rest of the rollout's run() calls (measured: 150-270 us per iteration).  So log lines go through an ordered
        # queue: a score line is an asynchronous copy into pinned memory plus an event, and lines are written, in order, as soon
        # as the head of the queue is ready -- at the latest by flush_log() / exit() / the next blocking point.  The text and the
        # order of the lines are the reference's; only the moment they appear moves.  `async_log=False` reads and prints at once.
        self._async_log = opts.async_log and dev.type == "cuda"
        self._log_q = collections.deque()
        # opt-in (`--log_throughput`): the score line also carries env-steps/s (all ranks) over the steps since the previous score
        # line, by the host's clock.  Off by default: stdout then is the reference's lines (ppo.py:257-260), character for character.
        self.log_throughput = opts.log_throughput
        self._rate_mark = None                                      # (perf_counter, run_step) of the previous score line
        self._pending_step = None                                   # deferred check of the device step counter (_update_hip)
        self._in_run_tail = False                                   # True inside run()'s periodic save (save_training_state)
        self.env.bind_obs(self._obs_ring[0])                        # first policy input: zeros (Q8)

        self.score = 0
        self.run_step = 0
        self.optim_step = 0

        self.net = Net(self.env.num_obs, self.env.num_act).to(dev)
        loaded_rms, loaded_value_rms, loaded_reward_rms = {}, {}, {}
        if opts.resume or opts.load:                                # ppo.py:147-149; a resumed run's weights file goes in alike
            said, path = ("resuming from: ", opts.resume_path) if opts.resume else ("loaded from: ", self.args.load_path)
            print(said, str(path))
            sd = torch.load(path, map_location=dev, weights_only=True)
            loaded_rms = split_obs_rms(sd, self.normalize_obs)
            loaded_value_rms = split_value_rms(sd, self.normalize_value)
            loaded_reward_rms = split_reward_rms(sd, self.normalize_reward)
            self.net.load_state_dict(sd)
        self._loaded = opts.load
        from .policy import PackedPolicy
        self.policy = PackedPolicy(self.net, dev)                   # parameters become views of one packed buffer
        self.net._policy = self.policy
        # "hip": MFMA forward/backward + fused clip/Adam kernels; "torch": torch-ROCm autograd (A/B reference)
        self.update_backend = opts.update_backend
        self.policy.init_training(self.mini_chunk_size * n, lr=self.lr)
        action_var = 0.01 if self.args.testing else 0.2             # ppo.py:152
        # ppo.py:236-237 decays the variance after every env step and ppo.py:233 adds the step's mean
        # reward to the score.  Both are applied to the device tensors LAZILY, for a run of steps at
        # once (`_flush_bookkeeping`): when the score is printed, before an update, and whenever
        # `action_var` is read; in between the policy launch derives the step's variance from the
        # tensor and the number of pending decays.  Bit for bit the per-step result.
        self._action_var = torch.full((self.env.num_act,), action_var, device=dev)
        self._book_from = 0            # first rollout row whose bookkeeping is still pending
        self._rows_done = 0            # rollout rows stepped so far in this rollout
        self.optim = torch.optim.Adam(self.net.parameters(), lr=self.lr)

        self._lib = _lib.load()
        self._obs_norm_ring = None
        if self.normalize_obs:
            self._setup_obs_norm(loaded_rms)
        if self.normalize_value:
            self._setup_value_norm(loaded_value_rms)
        if self.normalize_reward:
            self._setup_reward_norm(loaded_reward_rms)
        self._gen = torch.Generator(device=dev)
        self._gen.manual_seed(opts.seed + 1000003 * opts.rank)
        self.world_size = opts.world_size
        # "grad_allreduce" (default): one packed-gradient all-reduce per optimizer step = the reference's
        # update on the global minibatch.  "param_average": one exchange per PPO update (non-parity).
        self.dp_mode = opts.dp_mode
        # the per-step gradient exchange: "rccl" = torch.distributed.all_reduce (RCCL over xGMI; the default and the
        # fallback) or "p2p" = the one-shot peer-to-peer kernel of csrc/dp_p2p.hip (one node, <= 16 ranks)
        # "auto" = p2p if its start-up self-test against the collective passes on this node, else rccl.
        self.dp_allreduce = opts.dp_allreduce
        self._p2p = None
        self._flat_grad = None
        if self.world_size > 1:
            from .dist import FlatGradAllReduce
            self._flat_grad = FlatGradAllReduce(self.net.parameters(), self.world_size)

    def _say_no_statistics(self, option, what):
        """The line for a loaded weights file without the statistics that `option` keeps (none for a new network)."""
        if self._loaded:
            print("%s: %s holds no %s; starting from mean 0, var 1" % (option, str(self.args.load_path), what))

    def _all_rank_sets(self, sets, keep):
        """The moment sets of every rank, in rank order, on the device (one rank: `sets` itself).  A gloo group gathers on the
        CPU; the gathered tensor is held in the attribute `keep` until the stream has consumed it."""
        if self.world_size == 1:
            return sets
        import torch.distributed as dist
        src = sets.cpu() if dist.get_backend() == "gloo" else sets
        parts = [torch.empty_like(src) for _ in range(self.world_size)]
        dist.all_gather(parts, src)
        sets = torch.cat(parts).to(self.device)
        setattr(self, keep, sets)
        return sets

    # ------------------------------------------------------------------------------------------
    # observation normalisation (opt-in)
    def _setup_obs_norm(self, loaded_rms):
        """The running statistics S (f64: count | mean[73] | var[73], initially 0 | 0 | 1), the table the kernels read (f32:
        m[73] | r[73] | clip, derived from S), the normalised copy of the ring, the pass's moment sets; the table is registered
        with the env handle, so every rollout launch from here on normalises its policy input.  The table's address never
        changes: the merge rewrites it in place (captured graphs stay valid)."""
        dev, k = self.device, self.num_obs
        self._obs_stats = torch.zeros(_lib.OBS_NORM_SET, dtype=torch.float64, device=dev)
        self._obs_stats[1 + k:] = 1.0
        if loaded_rms:
            self._obs_stats[0] = loaded_rms["obs_rms.count"].to(dev, torch.float64).reshape(())
            self._obs_stats[1:1 + k] = loaded_rms["obs_rms.mean"].to(dev, torch.float64)
            self._obs_stats[1 + k:] = loaded_rms["obs_rms.var"].to(dev, torch.float64)
        else:
            self._say_no_statistics("normalize_obs", "observation statistics (obs_rms.*)")
        self._obs_table = torch.empty(_lib.OBS_NORM_SET, dtype=torch.float32, device=dev)
        self._obs_table.copy_(obs_norm_table(self._obs_stats, self.obs_clip))
        self._obs_norm_ring = torch.empty_like(self._obs_ring)
        self._obs_sets = torch.zeros((_lib.OBS_NORM_SETS, _lib.OBS_NORM_SET), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)                                 # the table is in place before any launch reads it
        _lib.api().fly_set_obs_norm(self.env._handle, self._obs_table)

    @property
    def obs_mean(self):
        """Running mean of the observations (f64 [73], a copy), or None when normalisation is off."""
        return self._obs_stats[1:1 + self.num_obs].clone() if self.normalize_obs else None

    @property
    def obs_var(self):
        """Running population variance of the observations (f64 [73], a copy), or None when normalisation is off."""
        return self._obs_stats[1 + self.num_obs:].clone() if self.normalize_obs else None

    @property
    def obs_count(self):
        """Rows the running statistics are taken over (f64 scalar, a copy), or None when normalisation is off."""
        return self._obs_stats[0].clone() if self.normalize_obs else None

    def _obs_norm_pass(self):
        """ppo_obs_norm_pass over the whole ring: rows 0..T normalised under the current table into _obs_norm_ring, and the
        float64 moments of rows 1..T (the observations this rollout produced; row 0 is the previous rollout's row T) into
        _obs_sets.  Idempotent until the next merge."""
        T, n = self.rollout_size, int(self.args.num_envs)
        _lib.api().ppo_obs_norm_pass(self._obs_ring, (T + 1) * n, n, self._obs_table, self._obs_norm_ring, self._obs_sets,
                                    _lib.stream_ptr())

    def _merge_obs_stats(self):
        """Fold the moments of the last pass into S (all ranks' sets, in rank order) and rewrite the table: S_k -> S_k+1."""
        sets = self._all_rank_sets(self._obs_sets, "_keep_sets")
        _lib.api().ppo_obs_norm_merge(self._obs_stats, self._obs_table, sets, sets.shape[0], self.obs_clip, _lib.stream_ptr())

    # ------------------------------------------------------------------------------------------
    # value normalisation (opt-in)
    def _setup_value_norm(self, loaded_rms):
        """The running statistics S_v of the TD targets (f64: count | mean | var, initially 0 | 0 | 1) and their table (f32:
        m | s | r | 0): the COMMITTED pair, under which make_data denormalises the critic's outputs.  Beside it the scratch
        pair make_data's merge writes (S_v with this rollout's targets folded in), the normalised copy of the targets and the
        GAE pass's moment sets.  update() commits scratch -> committed by two device copies into these fixed addresses."""
        dev = self.device
        self._value_stats = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        if loaded_rms:
            for i, k in enumerate(("value_rms.count", "value_rms.mean", "value_rms.var")):
                self._value_stats[i] = loaded_rms[k].to(dev, torch.float64).reshape(())
        else:
            self._say_no_statistics("normalize_value", "value statistics (value_rms.*)")
        self._value_table = value_norm_table(self._value_stats).contiguous()
        self._value_stats_next = self._value_stats.clone()
        self._value_table_next = self._value_table.clone()
        self._target_norm = torch.zeros_like(self._target)
        self._value_sets = torch.zeros((_lib.VALUE_NORM_SETS, _lib.VALUE_NORM_SET), dtype=torch.float64, device=dev)

    @property
    def value_mean(self):
        """Running mean of the TD targets, reward units (f64 scalar, a copy), or None when value normalisation is off."""
        return self._value_stats[1].clone() if self.normalize_value else None

    @property
    def value_var(self):
        """Running population variance of the TD targets (f64 scalar, a copy), or None when value normalisation is off."""
        return self._value_stats[2].clone() if self.normalize_value else None

    @property
    def value_count(self):
        """Targets the running statistics are taken over (f64 scalar, a copy), or None when value normalisation is off."""
        return self._value_stats[0].clone() if self.normalize_value else None

    def denormalize_value(self, v):
        """A critic output in reward units: v * s + m under the committed table in float32 (what make_data's GAE pass does);
        `v` itself when value normalisation is off."""
        if not self.normalize_value:
            return v
        return v * self._value_table[1] + self._value_table[0]

    def _td_gae_vnorm(self, reward, values, done_f, mode):
        """make_data's GAE pass with value normalisation: raw targets and advantages under the COMMITTED table plus the targets'
        moments (ppo_td_gae_vnorm; with gae='episodic' ppo_td_gae_episodic_vnorm, which reads the flag rows, not `done_f`), S_v
        with them folded in and its table into the scratch pair (ppo_value_norm_merge; all ranks' sets in rank order), and the
        targets normalised under the scratch table (ppo_value_norm_apply).  With `lambda_returns` the targets and their moments
        are overwritten by the lambda-returns' right behind the GAE kernel, so everything after it is theirs.  Nothing committed
        is written, so it is idempotent on a finished rollout.  `reward` is all_reward, or its scaled copy (normalize_reward)."""
        T, n = self.rollout_size, int(self.args.num_envs)
        if self.gae == "episodic":
            _lib.api().ppo_td_gae_episodic_vnorm(
                reward, values[:T], values[1:], self._reset_rows, self._progress_rows, self._ended_prev,
                self.env.max_episode_length, self._value_table, self.gamma, self.lmbda, T, n, self._target, self.all_advantage,
                self._value_sets, mode, _lib.stream_ptr())
        else:
            _lib.api().ppo_td_gae_vnorm(
                reward, values[:T], values[1:], done_f, self._value_table, self.gamma, self.lmbda, T, n, self._target,
                self.all_advantage, self._value_sets, mode, _lib.stream_ptr())
        if self.lambda_returns:
            self._lambda_targets(values, self._value_table, self._value_sets)      # the targets AND their moments: S_v is theirs
        sets = self._all_rank_sets(self._value_sets, "_keep_value_sets")
        _lib.api().ppo_value_norm_merge(self._value_stats, sets, sets.shape[0], self._value_stats_next, self._value_table_next,
                                       _lib.stream_ptr())
        _lib.api().ppo_value_norm_apply(self._target, T * n, self._value_table_next, self._target_norm, _lib.stream_ptr())

    def _lambda_targets(self, values, table, sets):
        """Opt-in (`lambda_returns`): _target <- all_advantage + v(obs_t) in reward units (ppo_lambda_targets: one launch, no
        host sync), from the advantages the GAE kernel has just written -- raw, so before _normalize_advantage -- and the critic
        outputs it read.  `table` / `sets` (value normalisation) or None: denormalise v under the committed table, and write
        the float64 moment sets of the new targets over the TD targets'."""
        T, n = self.rollout_size, int(self.args.num_envs)
        _lib.api().ppo_lambda_targets(self.all_advantage, values[:T], table, T * n, self._target, sets, _lib.stream_ptr())

    def _commit_value_stats(self):
        """S_v <- scratch, table <- scratch table: the next make_data denormalises under the table this update trained on."""
        self._value_stats.copy_(self._value_stats_next)
        self._value_table.copy_(self._value_table_next)

    # ------------------------------------------------------------------------------------------
    # reward scaling (opt-in)
    def _setup_reward_norm(self, loaded_rms):
        """The running statistics S_r of the discounted returns (f64: count | mean | var, initially 0 | 0 | 1; the mean is
        tracked, only the variance scales), their table (f32: m | s | r | 0) and the per-env carries G (f64 [N], the discounted
        return of each env's open episode): the COMMITTED set, as the last update left it.  Beside it the scratch set that
        make_data's pass writes (S_r with this rollout's returns folded in, its table, the carries at the rollout's end), the
        launch's moment sets and the scaled copy of the rewards the GAE launches read.  update() commits scratch -> committed
        by device copies into these fixed addresses."""
        dev, T, n = self.device, self.rollout_size, int(self.args.num_envs)
        self._flag_rows()
        self._rnorm_stats = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64, device=dev)
        if loaded_rms:
            for i, k in enumerate(("reward_rms.count", "reward_rms.mean", "reward_rms.var")):
                self._rnorm_stats[i] = loaded_rms[k].to(dev, torch.float64).reshape(())
        else:
            self._say_no_statistics("normalize_reward", "return statistics (reward_rms.*)")
        self._rnorm_table = value_norm_table(self._rnorm_stats).contiguous()
        self._rnorm_stats_next = self._rnorm_stats.clone()
        self._rnorm_table_next = self._rnorm_table.clone()
        self._rnorm_carry = torch.zeros(n, dtype=torch.float64, device=dev)
        self._rnorm_carry_next = torch.zeros(n, dtype=torch.float64, device=dev)
        self._rnorm_sets = torch.zeros((_lib.VALUE_NORM_SETS, _lib.VALUE_NORM_SET), dtype=torch.float64, device=dev)
        self._rnorm_scaled = torch.zeros((T, n, 1), device=dev)

    @property
    def reward_var(self):
        """Running population variance of the discounted returns (f64 scalar, a copy), or None when reward scaling is off."""
        return self._rnorm_stats[2].clone() if self.normalize_reward else None

    @property
    def reward_count(self):
        """Returns the running statistics are taken over (f64 scalar, a copy), or None when reward scaling is off."""
        return self._rnorm_stats[0].clone() if self.normalize_reward else None

    @property
    def reward_scale(self):
        """The committed factor r = (float)(1 / sqrt(var + 1e-5)) (f32 scalar, a copy), or None when reward scaling is off."""
        return self._rnorm_table[2].clone() if self.normalize_reward else None

    def _reward_norm_pass(self):
        """make_data's first pass with reward scaling: the finished rollout's discounted returns from the COMMITTED carries,
        their moments and the carries at its end (ppo_reward_returns), S_r with the moments folded in and its table into the
        scratch pair (ppo_value_norm_merge; all ranks' sets in rank order), and the rewards scaled under the scratch table
        (ppo_reward_scale): update, then normalise, gymnasium's and SB3's order.  Nothing committed is written, so it is
        idempotent on a finished rollout.  Returns the buffer the GAE launch reads in place of all_reward."""
        T, n = self.rollout_size, int(self.args.num_envs)
        mode = 4 if n < 512 and T >= 1024 else 0                    # PPO_GAE_SCAN: make_data's rule
        _lib.ext().ppo_reward_returns(self.all_reward, self._reset_rows, self.gamma, T, n, self._rnorm_carry,
                                     self._rnorm_carry_next, self._rnorm_sets, mode, _lib.stream_ptr())
        sets = self._all_rank_sets(self._rnorm_sets, "_keep_rnorm_sets")
        _lib.api().ppo_value_norm_merge(self._rnorm_stats, sets, sets.shape[0], self._rnorm_stats_next, self._rnorm_table_next,
                                       _lib.stream_ptr())
        _lib.ext().ppo_reward_scale(self.all_reward, T * n, self._rnorm_table_next, self.reward_clip, self._rnorm_scaled,
                                   _lib.stream_ptr())
        return self._rnorm_scaled

    def _commit_rnorm_stats(self):
        """S_r, table and carries <- scratch: the next rollout's returns go on from where this one's ended."""
        self._rnorm_stats.copy_(self._rnorm_stats_next)
        self._rnorm_table.copy_(self._rnorm_table_next)
        self._rnorm_carry.copy_(self._rnorm_carry_next)

    # ------------------------------------------------------------------------------------------
    # shuffled minibatches (opt-in)
    def _setup_minibatch(self):
        """The one staging minibatch (obs | action | log-prob | target | advantage rows, 376 B per row: 15.4 MB at the default
        shape; stream order makes one set enough), this rank's seed (options.py: `minibatch_seed`, default `seed`, offset by
        the rank as domain randomisation's) and the count of update() calls the epoch keys are derived from.  Nothing of it
        goes into the weights file; `--save_state` carries it."""
        dev, rows = self.device, self.mini_chunk_size * int(self.args.num_envs)
        self._mb_seed = self.options.minibatch_seed
        self._mb_update = 0
        self._mb_stage = (torch.zeros((rows, self.num_obs), device=dev), torch.zeros((rows, self.num_acts), device=dev),
                          torch.zeros(rows, device=dev), torch.zeros((rows, 1), device=dev), torch.zeros((rows, 1), device=dev))

    def _gather_minibatch(self, epoch_key, first, rows, obs, action, old_log_prob, target, advantage):
        """The staged minibatch of positions [first, first + rows) of the permutation (seed, epoch_key) over all T * N rows of
        what make_data returned: obs [rows, 73], action [rows, 18], old log-prob [rows], target [rows, 1], advantage [rows, 1]
        -- views of the ONE staging set, valid until the next call (ppo_minibatch_gather, one launch, no host sync).  A pure
        function of its arguments: a redone optimizer step sees its minibatch again bit for bit.  `_mb_index` (optional int32
        [rows], tests) receives the source rows."""
        T, n = self.rollout_size, int(self.args.num_envs)
        so, sa, sl, st, sv = self._mb_stage
        _lib.api().ppo_minibatch_gather(obs, action, old_log_prob, advantage, target, T * n, self._mb_seed, epoch_key & 0xFFFFFFFF,
                                       first, rows, so, sa, sl, sv, st, self._mb_index, _lib.stream_ptr())
        return so, sa, sl, st, sv

    def _minibatches(self):
        """The optimizer steps of one update, in order.  reference: (k, j), the rollout's step slices [k, j) of ppo.py:179-181
        (Q3: the 16th chunk is never visited).  shuffled: (epoch key, window), the same number of steps; epoch e of update u
        has key u * epoch + e and window w is positions [w * rows, (w + 1) * rows) of its permutation, so each epoch leaves a
        random sixteenth of the rows out."""
        mc = self.mini_chunk_size
        cuts = range(mc, self.rollout_size, mc)
        if self.minibatch == "shuffled":
            return [(self._mb_update * self.epoch + e, w) for e in range(self.epoch) for w in range(len(cuts))]
        return [(j - mc, j) for _ in range(self.epoch) for j in cuts]   # 5 x 15 (Q3)

    def _minibatch(self, item, data):
        """One entry of _minibatches() as the five tensors of an optimizer step ([mc, N, ..] slices, or the staged rows)."""
        if self.minibatch == "shuffled":
            rows = self.mini_chunk_size * int(self.args.num_envs)
            return self._gather_minibatch(item[0], item[1] * rows, rows, *data)
        k, j = item
        return tuple(x[k:j] for x in data)

    # ppo.py:230 replaces the whole [T,N,1] buffer by the LAST step's [N,1] mask after every step
    # (Q1).  reset_buf only changes inside env.step, so deriving the mask on demand is the same
    # thing without two tiny launches per step; an explicit assignment (tests) overrides it.
    @property
    def all_done(self):
        if self._all_done is not None:
            return self._all_done
        return (1 - self.env.reset_buf).unsqueeze(-1)

    @all_done.setter
    def all_done(self, value):
        if self.gae == "episodic":
            raise ValueError("all_done has no meaning with gae='episodic': the estimator reads the per-step reset / progress "
                             "rows the rollout wrote, not a done mask")
        self._all_done = value

    def _flag_rows(self):
        """The per-step [T, N] int64 rows of the env's reset / progress flags: row t holds them as step t left them."""
        if self._reset_rows is None:
            T, n = self.rollout_size, int(self.args.num_envs)
            self._reset_rows = torch.zeros((T, n), dtype=torch.long, device=self.device)
            self._progress_rows = torch.zeros((T, n), dtype=torch.long, device=self.device)

    def _td_gae_episodic(self, reward, values, mode):
        """make_data's GAE pass with gae='episodic' (ppo_td_gae_episodic): straight from the int64 flag rows, no conversions."""
        T, n = self.rollout_size, int(self.args.num_envs)
        _lib.api().ppo_td_gae_episodic(
            reward, values[:T], values[1:], self._reset_rows, self._progress_rows, self._ended_prev,
            self.env.max_episode_length, self.gamma, self.lmbda, T, n, self._target, self.all_advantage, mode, _lib.stream_ptr())

    # ------------------------------------------------------------------------------------------
    # episode statistics (opt-in)
    def _setup_episode_stats(self):
        """The per-env carries of the open episodes (float64 return, int64 length), the sets one ppo_episode_stats launch
        writes, and the two persistent sets: `window` (episodes closed since the last score line) and `total` (since the start
        of the run), both the empty set with rows = 0."""
        dev, n = self.device, int(self.args.num_envs)
        self._flag_rows()
        self._ep_carry_ret = torch.zeros(n, dtype=torch.float64, device=dev)
        self._ep_carry_len = torch.zeros(n, dtype=torch.long, device=dev)
        self._ep_sets = torch.zeros((_lib.EPISODE_SETS, _lib.EPISODE_SET), dtype=torch.float64, device=dev)
        inf = float("inf")
        self._ep_empty = torch.tensor([0.0, 0.0, 0.0, inf, -inf, 0.0, inf, 0.0, 0.0, 0.0], dtype=torch.float64, device=dev)
        self._ep_window, self._ep_total = self._ep_empty.clone(), self._ep_empty.clone()

    def _episode_stats_pass(self):
        """The finished rollout's rows through ppo_episode_stats (the carries go on into the next rollout), all ranks' sets in
        rank order into `window` and `total` (ppo_episode_stats_merge): every rank holds the same two sets.  On the stream, no
        host sync."""
        T, n = self.rollout_size, int(self.args.num_envs)
        mode = 4 if n < 512 and T >= 1024 else 0                    # PPO_GAE_SCAN: make_data's rule
        _lib.api().ppo_episode_stats(self.all_reward, self._reset_rows, self._progress_rows, self.env.max_episode_length, T, n,
                                    self._ep_carry_ret, self._ep_carry_len, self._ep_sets, mode, _lib.stream_ptr())
        sets = self._all_rank_sets(self._ep_sets, "_keep_ep_sets")
        _lib.api().ppo_episode_stats_merge(sets, sets.shape[0], self._ep_window, self._ep_total, _lib.stream_ptr())

    @staticmethod
    def _episode_suffix(w):
        """' | Episodes ...' of the score line from a set's ten numbers."""
        n = int(w[0])
        if n == 0:
            return " | Episodes 0"
        return " | Episodes {} | Return {:.4f} [{:.4f}, {:.4f}] | Length {:.1f} | Timeouts {:.1f}%".format(
            n, float(w[1]), float(w[3]), float(w[4]), float(w[5]) / n, 100.0 * float(w[8]) / n)

    def episode_stats(self):
        """{"window": {...}, "total": {...}}: the episodes closed since the last score line and since the start of the run, as
        Python numbers (episodes, return_mean, return_std -- the population's --, return_min, return_max, length_mean,
        length_min, length_max, timeouts; without an episode everything but the two counts is nan).  Host-synchronising.
        None when `episode_stats` is off."""
        if not self._episode_stats:
            return None

        def entries(s):
            n = int(s[0])
            if n == 0:
                nan = float("nan")
                return {"episodes": 0, "return_mean": nan, "return_std": nan, "return_min": nan, "return_max": nan,
                        "length_mean": nan, "length_min": nan, "length_max": nan, "timeouts": 0}
            return {"episodes": n, "return_mean": s[1], "return_std": (max(s[2], 0.0) / n) ** 0.5 if s[2] == s[2] else s[2],
                    "return_min": s[3], "return_max": s[4], "length_mean": s[5] / n, "length_min": int(s[6]),
                    "length_max": int(s[7]), "timeouts": int(s[8])}
        return {"window": entries(self._ep_window.tolist()), "total": entries(self._ep_total.tolist())}

    # ------------------------------------------------------------------------------------------
    # update diagnostics (opt-in)
    def _setup_update_stats(self):
        """The sets one ppo_update_stats launch writes and the three persistent sets, all the empty set: `last` (the latest
        update), `window` (the updates since the last score line) and `total` (since the start of the run)."""
        dev = self.device
        self._us_sets = torch.zeros((_lib.UPDATE_STATS_SETS, _lib.UPDATE_STATS_SET), dtype=torch.float64, device=dev)
        self._us_empty = update_stats_empty().to(dev)
        self._us_last, self._us_window, self._us_total = (self._us_empty.clone() for _ in range(3))
        self._us_mu = self._us_v = None                             # the probe's forward of the latest update

    def _update_stats_probe(self, obs, action, old_log_prob, target, advantage):
        """Behind the finished update: the UPDATED network over ALL T * N rows the update was handed (the normalised rows under
        normalize_obs; the 16th chunk too, which the reference's minibatches never train on, Q3), through the unchanged
        mlp_forward, one ppo_update_stats over them against the targets the update regressed on, and all ranks' sets in rank
        order into `last`, `window` and `total`: every rank holds the same three sets.  On the stream, no host sync; nothing a
        rollout or an update reads is written."""
        api = _lib.update_stats_api()
        with torch.no_grad():
            self._us_mu, self._us_v = self.policy.forward(obs, want_mu=True, want_v=True)
            rows = self._us_v.numel()
            api.ppo_update_stats(self._us_mu, action, old_log_prob, advantage, self._us_v, target, self._action_var, self.clip, rows,
                                 self._us_sets, _lib.stream_ptr())
            sets = self._all_rank_sets(self._us_sets, "_keep_us_sets")
            api.ppo_update_stats_merge(sets, sets.shape[0], self._us_last, self._us_window, self._us_total, _lib.stream_ptr())

    def update_stats(self):
        """{"last": {...}, "window": {...}, "total": {...}}: the latest update, the updates since the last score line and since
        the start of the run, as Python numbers (update_stats_entries: rows, nonfinite, approx_kl -- Schulman's k3 --, kl_k1,
        clip_fraction, ratio_min, ratio_max, policy_loss, value_loss, loss, explained_variance -- of the UPDATED critic on the
        targets it just regressed on, in their units --, target_mean, target_std, adv_absmax, target_absmax).
        Host-synchronising.  None when `update_stats` is off."""
        if not self._update_stats:
            return None
        return {k: update_stats_entries(getattr(self, "_us_" + k).tolist()) for k in ("last", "window", "total")}

    # ------------------------------------------------------------------------------------------
    @property
    def action_var(self):
        self._flush_bookkeeping()
        return self._action_var

    @action_var.setter
    def action_var(self, value):
        """The reference rebinds this attribute (ppo.py:237); here the rollout launches hold a POINTER to
        the variance tensor, so an assignment first applies the decays still pending on the old value and
        then writes the new one in place -- every later launch (sampling, log-prob, loss) sees it."""
        if getattr(self, "_action_var", None) is None:
            self._action_var = value
            return
        if getattr(self, "persistent_rollout", False) and 0 < getattr(self, "_rows_done", 0) < self.rollout_size:
            # one launch per rollout: the steps of the rollout in progress have already been sampled on the device
            import warnings
            warnings.warn("action_var assigned inside a rollout that was launched as ONE kernel: the new value takes effect at the "
                          "next rollout (PPO(..., persistent_rollout=False) launches step by step and applies it at once)")
        if getattr(self, "_book_terms", None) is not None:
            self._flush_bookkeeping()
        with torch.no_grad():
            v = torch.as_tensor(value, dtype=torch.float32, device=self._action_var.device)
            self._action_var.copy_(v.expand_as(self._action_var))

    def _flush_bookkeeping(self):
        """Apply the score terms and variance decays of rollout rows [_book_from, _rows_done); there are none before the first
        step has built the launch arguments (`_book_terms`, _prepare_step_args)."""
        if self._book_terms is None:
            return
        rows = self._rows_done - self._book_from
        if rows <= 0:
            return
        n = int(self.args.num_envs)
        _lib.api().ppo_rollout_bookkeeping(
            self.all_reward[self._book_from], rows, n, self._book_terms, self._score_acc, 1.0 / self.num_eval_freq,
            self._action_var, self.num_acts, self._var_decay, self._var_min, self._rows_applied, _lib.stream_ptr())
        self._book_from = self._rows_done

    def make_data(self):
        """ppo.py:157-171: TD target and GAE.  `all_done` is the [N,1] mask of the LAST step,
        broadcast over T (Q1), and the recurrence never resets at episode ends (Q2).  With gae='episodic' the estimator of
        DESIGN.md 3.3d instead, from the per-step flag rows.  With lambda_returns the critic's target is the advantage plus
        v(obs_t) instead of the TD target; the advantages are the same either way."""
        T, n = self.rollout_size, self.args.num_envs
        with torch.no_grad():
            reward = self._reward_norm_pass() if self.normalize_reward else self.all_reward
            ring = self._obs_ring
            if self.normalize_obs:
                self._obs_norm_pass()                               # the rows the rollout's policy saw, under the same table
                ring = self._obs_norm_ring
            if self.reuse_rollout_values and self._v_have == T and self._v_version == self.policy.version:
                self._v_ring[T].copy_(self.net.v(ring[T]))
                values = self._v_ring                               # rows 0..T-1 were written by the rollout launches
            else:
                values = self.net.v(ring)                           # [T+1, N, 1]: v(obs) and v(next_obs) in one pass
            self._v_have = 0
            mode = 4 if n < 512 and T >= 1024 else 0                # PPO_GAE_SCAN: few envs x long rollout
            if self.gae == "episodic":
                if self.normalize_value:
                    self._td_gae_vnorm(reward, values, None, mode)
                else:
                    self._td_gae_episodic(reward, values, mode)
                self._keep = (values,)
            else:
                done = self.all_done
                if done.dim() == 3 and done.shape[0] == T and done.shape[1] == n:
                    mode |= 1                                       # per-step mask; the reference path is [N,1]
                done_f = done.to(torch.float32).contiguous()
                if self.normalize_value:
                    self._td_gae_vnorm(reward, values, done_f, mode)        # `values` are normalised-unit outputs: denormalised there
                else:
                    _lib.api().ppo_td_gae(reward, values[:T], values[1:], done_f, self.gamma, self.lmbda, T, n,
                                         self._target, self.all_advantage, mode, _lib.stream_ptr())
                self._keep = (values, done_f)                       # alive until the stream has consumed them
            if self.lambda_returns and not self.normalize_value:
                self._lambda_targets(values, None, None)            # (with normalize_value: inside _td_gae_vnorm)
            if self.normalize_advantage:
                self._normalize_advantage()
        obs = self._obs_norm_ring[:T] if self.normalize_obs else self.all_obs
        target = self._target_norm if self.normalize_value else self._target
        return obs, self.all_acts, self.all_log_prob, target, self.all_advantage

    def _normalize_advantage(self):
        """Opt-in (`normalize_advantage`): adv <- (adv - mean) / (std + 1e-8) over the whole rollout of
        ALL ranks.  Not in the reference (ppo.py:171 uses raw advantages); named by BASELINE's north_star."""
        import torch.distributed as dist
        cnt = self.all_advantage.numel()
        _lib.api().ppo_adv_stats(self.all_advantage, cnt, self._adv_stats, _lib.stream_ptr())
        if self.world_size > 1:
            mine = self._adv_stats[:2].clone()
            parts = [torch.empty_like(mine) for _ in range(self.world_size)]
            dist.all_gather(parts, mine)                            # every rank combines the same pairs in rank order
            self._adv_stats[:2].copy_(combine_adv_stats(torch.stack(parts), cnt))
        _lib.api().ppo_adv_apply(self.all_advantage, cnt, self._adv_stats, float(cnt * self.world_size), 1e-8, _lib.stream_ptr())

    def minibatch_loss(self, obs_mc, action_mc, old_log_prob_mc, target_mc, advantage_mc):
        """ppo.py:184-194.  Old log-prob is of the unclipped sample, the new one of the stored
        clipped action under the current (decayed) variance (Q6); the Huber term is a scalar
        mean added to every element (Q7)."""
        mu = self.net.pi(obs_mc)
        log_prob = diag_gauss_logprob(mu, action_mc, self._action_var)
        ratio = torch.exp(log_prob - old_log_prob_mc).unsqueeze(-1)
        surr1 = ratio * advantage_mc
        surr2 = torch.clamp(ratio, 1 - self.clip, 1 + self.clip) * advantage_mc
        loss = -torch.min(surr1, surr2) + F.smooth_l1_loss(self.net.v(obs_mc), target_mc)
        return loss.mean()

    def update(self):
        """ppo.py:173-202: 5 epochs x 15 contiguous-in-T minibatches; the 16th chunk is never
        visited (Q3).  With world_size > 1 the flat gradient is all-reduced (mean) before the clip.
        minibatch='shuffled': the same 75 steps on windows of a fresh permutation of all rows per epoch."""
        self._flush_bookkeeping()                                   # the loss uses the variance after this rollout's decays
        obs, action, old_log_prob, target, advantage = self.make_data()
        if self.update_backend == "hip":
            self._update_hip(obs, action, old_log_prob, target, advantage)
        else:
            self._update_torch(obs, action, old_log_prob, target, advantage)
        if self._update_stats:
            self._update_stats_probe(obs, action, old_log_prob, target, advantage)
        if self.minibatch == "shuffled":
            self._mb_update += 1                                    # the next update's epoch keys
        if self.normalize_obs:
            self._merge_obs_stats()                                 # after update k: the statistics of rollout k + 1
        if self.normalize_value:
            self._commit_value_stats()                              # after update k: the table make_data k + 1 denormalises with
        if self.normalize_reward:
            self._commit_rnorm_stats()                             # after update k: S_r and the carries rollout k + 1 goes on from

    def _update_torch(self, obs, action, old_log_prob, target, advantage):
        data = (obs, action, old_log_prob, target, advantage)
        for item in self._minibatches():
            loss = self.minibatch_loss(*self._minibatch(item, data))
            if self._flat_grad is not None:
                self._flat_grad.zero()                              # grads are views of the flat buffer
            else:
                self.optim.zero_grad()
            loss.backward()
            if self._flat_grad is not None:
                self._flat_grad.allreduce_mean()
            nn.utils.clip_grad_norm_(self.net.parameters(), 1.0)
            self.optim.step()
            self.optim_step += 1
        self.policy.refresh()       # torch wrote the master weights: rebuild the fragment-ordered copies

    def _optimizer_step(self, obs, action, old_log_prob, advantage, target, sync_grads):
        """One optimizer step of `_update_hip` on this rank's rows (flat: obs [rows, 73], action [rows, 18], the rest [rows]):
        the gradient launch, with `sync_grads` the exchange of the packed gradient, and the clip + Adam launch.  Each rank
        divides by ITS row count and the launch scales the summed gradient by 1 / world_size: the mean over the global
        minibatch, which the clip then sees (tests/test_dist_step_gpu.py holds two ranks of this to float64)."""
        pol = self.policy
        pol.minibatch_grad(obs, action, old_log_prob, advantage, target, self._action_var, self.clip, fuse_norm=not sync_grads)
        if sync_grads:
            if self._p2p is not None:
                self._p2p.allreduce_(pol.G)                 # one launch, one xGMI hop, sum in rank order
            else:
                import torch.distributed as dist
                dist.all_reduce(pol.G, op=dist.ReduceOp.SUM)    # 297 KB, latency-bound on xGMI
        # either way ONE optimizer launch per step; it reads the exchange's err word itself and refuses a gradient
        # that ANY workgroup of the exchange left un-reduced (fail closed, on the device)
        pol.adam_step(grad_scale=1.0 / self.world_size if sync_grads else 1.0, norm_ready=not sync_grads,
                      self_norm=sync_grads, grad_invalid=self._p2p.err if (sync_grads and self._p2p is not None) else None)

    def _update_hip(self, obs, action, old_log_prob, target, advantage):
        """ppo.py:179-202 on the MFMA kernels: per minibatch one fused forward, the loss gradient +
        dX chain, the split-row dW, (world_size > 1: ONE all-reduce of the packed gradient), and
        the fused clip + Adam step.  Minibatches are contiguous slices of the rollout, so no
        gather/copy happens -- except with minibatch='shuffled', where one gather launch stages each step's rows."""
        import torch.distributed as dist
        rows = self.mini_chunk_size * int(self.args.num_envs)
        pol = self.policy
        sync_grads = self.world_size > 1 and self.dp_mode == "grad_allreduce"
        slices = self._minibatches()     # reference: 5 x 15 (k, j) step slices (Q3); shuffled: 5 x 15 (epoch key, window)
        data = (obs, action, old_log_prob, target, advantage)
        self.prepare()                   # idempotent; callers that time the update call it themselves before warm-up

        def run(todo):
            for item in todo:
                # shuffled: the rows are staged again from (epoch key, window), so a redone step sees its minibatch bit for bit
                o, a, lp, tg, adv = self._minibatch(item, data)
                self._optimizer_step(o.view(rows, self.num_obs), a.view(rows, self.num_acts), lp.view(rows), adv.view(rows),
                                     tg.view(rows), sync_grads)

        self._check_step_counter()       # the previous update's counter, copied while this rollout ran
        cal_failed = False
        if pol.h2_live() and pol.fused_step and not pol.h2_calibrated:
            # fp16x2 step: the per-class scales are measured on the first minibatch before anything depends on them (a new
            # network, or an update whose values outgrew the scales: a few discarded launches, host-synchronising, rare)
            o, a, lp, tg, adv = self._minibatch(slices[0], data)
            failed = None
            try:
                pol.calibrate_h2(o.view(rows, self.num_obs), a.view(rows, self.num_acts), lp.view(rows), adv.view(rows),
                                 tg.view(rows), self._action_var, self.clip)
            except _lib.FlyHipError as e:
                if not sync_grads:
                    raise                # one rank, or param_average (no exchange inside the update for a peer to wait in)
                failed = e
            if sync_grads:
                # The ranks calibrate on their own rows, so one of them may fail to settle where its peers succeed -- and a rank
                # that raised here would leave them waiting in the update's first all-reduce.  So the verdict is the ranks'
                # together: ONE status word (MAX) over the process group, exchanged only when a calibration was attempted --
                # which every rank decides alike (`h2_calibrated` starts False everywhere and flips only on refusals every rank
                # sees).  If any rank failed, EVERY rank runs this update on bf16x3 and calibrates again at the next one.
                word = torch.tensor([0 if failed is None else 1], dtype=torch.int32, device=self.device)
                dist.all_reduce(word, op=dist.ReduceOp.MAX)
                if int(word.item()) != 0:
                    if failed is not None:
                        print("rank %d: %s; every rank runs this update on bf16x3" % (self.options.rank, failed))
                    pol.h2_suspended = cal_failed = True        # cleared at the end of this update, below
                    pol.h2_calibrated = False
                    pol.h2_calibration_failures += 1
        run(slices)
        if self._p2p is not None and not self._p2p.check():
            # FIRST, before anything looks at the step counter: a bounded wait of the peer-to-peer exchange expired on this
            # rank.  Its optimizer launches have refused the un-reduced gradients (fail closed) and the counter is behind, but
            # redoing steps is no remedy here -- no peer is at those epochs.  Fatal by design (dist.py: "the caller must stop").
            raise _lib.FlyHipError("dp_allreduce_p2p: a rank never published its gradient (bounded wait expired; "
                                   "FLY_P2P_POLL_LOG2 raises the budget, --dp_allreduce rccl avoids the kernel)")
        if not pol.update_can_be_refused():
            # No launch of this update path can leave an invalid gradient (the fused optimizer step hands nothing from workgroup to
            # workgroup), so the device counter only CONFIRMS the count.
            if self._p2p is None and self._async_log:
                # copied asynchronously and compared when the next update begins (or at exit) -- the host goes straight on to the
                # next rollout instead of draining the queue here (measured: ~120 us of launch-bound idle per iteration behind a
                # blocking read)
                host = torch.empty(1, dtype=pol.step.dtype, pin_memory=True)
                host.copy_(pol.step, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                self._pending_step = (ev, host, pol.steps_issued)
            else:
                got = int(pol.step.item())
                if got != pol.steps_issued:
                    raise _lib.FlyHipError("update: the device step counter says %d optimizer steps, %d were issued"
                                           % (got, pol.steps_issued))
                self._drain_log(block=True)
            if cal_failed:
                pol.h2_suspended = False
            self.optim_step += len(slices)
            self._finish_update(sync_grads)
            return
        # ONE host sync per update.  A fused forward+backward launch whose backward could not get a tile
        # leaves an invalid gradient; the optimizer kernels refuse such a step ON THE DEVICE (on every
        # rank: the flag rides inside the all-reduced gradient), and every later step of this update too.
        # So the device step counter says how many minibatches really happened: redo the rest through the
        # two-launch path -- bit for bit what an undisturbed update leaves.  (Only this path -- the tile
        # hand-off of mlp_forward_backward -- is ever redone.)
        h2 = pol.h2_live() and pol.fused_step
        for attempt in range(3):
            short = pol.steps_issued - int(pol.step.item())
            if (pol.fuse_fwd_bwd and not h2) or short:
                pol.check_fused_launch()
            if short == 0:
                break
            if short < 0 or short > len(slices) or attempt == 2:
                raise _lib.FlyHipError("update: device step counter is %d steps behind the %d issued" % (short, pol.steps_issued))
            pol.steps_issued -= short
            if h2 and not pol.h2_suspended:
                # a value of some launch did not fit fp16 under the scales its predecessor left (mlp_fused_h2.inc): that step and
                # every later one were refused on the device (the sticky word), on every rank.  Redo them, in order, on the bf16x3
                # kernel -- bit for bit what an undisturbed bf16x3 step leaves -- and measure the scales afresh before the next update.
                pol.h2_overflow.zero_()
                pol.h2_suspended = True
                pol.h2_calibrated = False
                pol.h2_overflows += 1
            else:
                pol.fuse_fwd_bwd = False
                print("mlp_forward_backward: %d of %d optimizer steps were refused on the device (a backward workgroup "
                      "could not get its tile); redoing them with two launches" % (short, len(slices)))
            run(slices[len(slices) - short:])
            if self._p2p is not None and not self._p2p.check():
                raise _lib.FlyHipError("dp_allreduce_p2p: a rank never published its gradient while refused steps were redone")
        pol.h2_suspended = False
        self.optim_step += len(slices)
        self._drain_log(block=True)                     # the queue is drained anyway: pending log lines cost nothing here
        self._finish_update(sync_grads)

    def _finish_update(self, sync_grads):
        import torch.distributed as dist
        pol = self.policy
        if self.world_size > 1 and not sync_grads:
            # dp_mode "param_average": ONE exchange per PPO update (BASELINE's north_star wording) --
            # ranks take their 75 optimizer steps locally, then parameters and Adam moments are
            # averaged.  NOT the reference algorithm on a larger batch (that is the default mode).
            for buf in (pol.P, pol.exp_avg, pol.exp_avg_sq):
                dist.all_reduce(buf, op=dist.ReduceOp.SUM)
                buf.div_(self.world_size)
            pol.refresh()

    def prepare(self):
        """Everything an update needs that is not part of an update: with data-parallel ranks and `dp_allreduce` "p2p" or
        "auto", open the peer windows and self-test the one-shot exchange against the collective.  A COLLECTIVE call (every
        rank makes it, in the same place); idempotent.  `bench.py` calls it before the warm-up so that none of it lands in a
        timed region; `_update_hip` calls it too, so a plain `run()` loop needs nothing extra."""
        if getattr(self, "_prepared", False):
            return
        self._prepared = True
        self.p2p_selftest = None
        sync_grads = self.world_size > 1 and self.dp_mode == "grad_allreduce"
        if sync_grads and self.update_backend == "hip" and self.dp_allreduce in ("p2p", "auto"):
            self._p2p = self._open_p2p(self.policy.G.numel())

    def _open_p2p(self, n):
        """Open the peer windows and hold the one-shot kernel to the collective on random data (3 epochs, both
        parities).  Every rank takes the same decision at every stage (`P2PAllReduce` votes inside its constructor, the
        self-test verdicts are all-reduced): on any failure -- no IPC between these devices, a wrong sum, a rank that
        never publishes -- "auto" falls back to RCCL on every rank together, "p2p" raises on every rank together."""
        import torch.distributed as dist
        from .dist import P2PAllReduce, P2PUnavailable
        from .policy import ERR_SLOT
        p2p, why = None, ""
        try:
            p2p = P2PAllReduce(n, self.device, fail_slot=ERR_SLOT)          # raises on ALL ranks or on none
        except P2PUnavailable as e:
            why = str(e)[:300]
        good = p2p is not None
        if good:
            flag = torch.ones(1, device=self.device, dtype=torch.int32)
            gen = torch.Generator(device=self.device)
            gen.manual_seed(7 + self.options.rank)
            for _ in range(3):
                a = torch.randn(n, device=self.device, generator=gen)
                a[ERR_SLOT] = 0.0
                b = a.clone()
                p2p.allreduce_(a)
                dist.all_reduce(b, op=dist.ReduceOp.SUM)
                mine = p2p.check() and torch.allclose(a, b, rtol=1e-5, atol=1e-5)
                flag.fill_(1 if mine else 0)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if int(flag.item()) != 1:
                    good, why = False, "self-test against the collective failed"
                    break
        self.p2p_selftest = "passed" if good else ("failed: " + (why or "a peer failed"))
        if good:
            self.dp_allreduce = "p2p"
            return p2p
        if p2p is not None:
            p2p.close()
        if self.dp_allreduce == "p2p":
            raise _lib.FlyHipError("dp_allreduce=p2p is not usable on this node: %s" % (why or "a peer failed"))
        if self.options.rank == 0:
            print("dp_allreduce auto: peer-to-peer all-reduce unavailable (%s); using the RCCL collective" % (why or "a peer failed"))
        self.dp_allreduce = "rccl"
        return None

    # ------------------------------------------------------------------------------------------
    def _prepare_step_args(self):
        """Every pointer of step t is a fixed row of a preallocated rollout tensor, so the ctypes
        argument tuples of the three launches are built ONCE per t: a step then costs three foreign
        calls and two attribute stores on the host (the rollout was host-bound at ~50 us/step
        against ~35 us of GPU work)."""
        T, n = self.rollout_size, int(self.args.num_envs)
        P = C.c_void_p
        pol = self.policy
        self._obs_rows = [self._obs_ring[t] for t in range(T + 1)]
        self._reward_rows = [self.all_reward[t].view(-1) for t in range(T)]
        self._act_rows = [self.all_acts[t] for t in range(T)]
        fwd, bufs, step = [], [], []
        self._var_decay = 0.0 if self.args.testing else 0.00001     # ppo.py:236
        self._var_min = C.c_float(0.01)
        self._book_terms = torch.zeros(T, device=self.device)       # scratch of ppo_rollout_bookkeeping
        # The policy launch of row t derives its variance from the tensor and the decays still pending:
        # t - (rows of this rollout already applied).  The second term lives in a DEVICE word that
        # ppo_rollout_bookkeeping advances, so the launch arguments of row t never change -- the same tuple
        # serves every rollout, eager or replayed from a captured hipGraph.
        self._rows_applied = torch.zeros(1, dtype=torch.int32, device=self.device)
        base_ptr = P(self._rows_applied.data_ptr())
        var_ptr = P(self._action_var.data_ptr())
        for t in range(T):
            fwd.append((P(pol.P.data_ptr()), P(pol.PF.data_ptr()), P(self._obs_rows[t].data_ptr()), C.c_int64(n),
                        P(self._eps_all[t].data_ptr()), var_ptr, C.c_int(t), C.c_float(self._var_decay), self._var_min,
                        P(self._act_rows[t].data_ptr()), P(self.all_log_prob[t].data_ptr()), None,
                        P(self._v_ring[t].data_ptr()), pol.infer_pb_ptr(), base_ptr))
            step.append((P(pol.P.data_ptr()), P(pol.PF.data_ptr()), P(self._obs_rows[t].data_ptr()),
                         P(self._eps_all[t].data_ptr()), var_ptr, C.c_int(t), C.c_float(self._var_decay), self._var_min,
                         P(self._act_rows[t].data_ptr()), P(self.all_log_prob[t].data_ptr()), P(self._v_ring[t].data_ptr()),
                         pol.infer_pb_ptr(), base_ptr))
            bufs.append((self._obs_rows[t + 1].data_ptr(), self._reward_rows[t].data_ptr()))
        self._fwd_args, self._buf_ptrs, self._step_args = fwd, bufs, step
        self._graphs = {}                                            # captured steps hold the old pointers
        # one launch per env step (policy + sampling + env step), eager or captured; FLY_FUSE_ROLLOUT_STEP=0 keeps the
        # two-launch form (mlp_forward_sample + fly_step) for the A/B test
        self.fuse_rollout_step = os.environ.get("FLY_FUSE_ROLLOUT_STEP", "1") != "0"
        self._args_infer_gemm = pol.gemm_infer
        if self.normalize_obs and not self.fuse_rollout_step and not self.persistent_rollout:
            raise _lib.FlyHipError("normalize_obs: the two-launch rollout step (FLY_FUSE_ROLLOUT_STEP=0, mlp_forward_sample) does not "
                                   "normalise observations; use the one-launch step")

    def _draw_noise(self):
        """The noise of a whole rollout into `_eps_all` [T, N, 18], on the current stream (captured with the rollout in a graph).
        white: one normal_() and nothing else.  ar1: the same draw, then ppo_noise_ar1 filters it in place along time from the
        carry, so `_eps_all` holds what the rollout uses; the carry is drawn from the stationary law immediately before the
        first rollout's draw (the first rollout always runs eagerly) and left to the launches after that."""
        if self.action_noise == "ar1" and not self._noise_carry_drawn:
            self._noise_carry.normal_(generator=self._gen)
            self._noise_carry_drawn = True
        self._eps_all.normal_(generator=self._gen)
        if self.action_noise == "ar1":
            T, n = self.rollout_size, int(self.args.num_envs)
            _lib.api().ppo_noise_ar1(self._eps_all, self._noise_carry, T, n * self.num_acts, self.noise_rho, _lib.stream_ptr())

    def _launch_step(self, t):
        """The device work of one env step (ppo.py:213-237): ONE launch (`ppo_rollout_step`), no host logic.  Rows of
        the rollout are written in place (obs row t+1, action/log-prob/reward rows t); the score and
        variance bookkeeping of the step is deferred (`_flush_bookkeeping`)."""
        lib, env = self._lib, self.env
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if t == 0:
            self._draw_noise()                                      # the eps of MultivariateNormal.sample, whole rollout
            self._rows_applied.zero_()                              # a new rollout: no row's bookkeeping applied yet
        env.obs_buf, env.reward_buf = self._obs_rows[t + 1], self._reward_rows[t]      # ppo.py:228-229
        env._bufs.obs, env._bufs.reward = self._buf_ptrs[t]
        if t == 0 and self.gae == "episodic":
            self._ended_prev.copy_(env.reset_buf)                   # the flags the env carries into this rollout
        if self.fuse_rollout_step:
            # policy + sampling + env step of every 32-env tile in ONE launch (ppo.py:214-229)
            rc = lib.ppo_rollout_step(env._handle, C.byref(env._bufs), *self._step_args[t], st)
        else:
            rc = lib.mlp_forward_sample(*self._fwd_args[t], st)     # ppo.py:214-220, :227 (policy + sampling fused)
            rc |= lib.fly_step(env._handle, C.c_void_p(self._act_rows[t].data_ptr()), C.byref(env._bufs), st)  # ppo.py:223
        if rc:
            _lib.check(rc, "rollout step")
        if self.gae == "episodic" or self._episode_stats or self.normalize_reward:
            # row t of the flag rows, as the one-launch rollout writes them itself (captured with the step in a graph)
            self._reset_rows[t].copy_(env.reset_buf)
            self._progress_rows[t].copy_(env.progress_buf)
        self._after_step(t)
        if env.recorder is not None:
            env.recorder.capture(t)                                 # env 0's pose after this step (captured with it in a graph)
        env.render_count += 1

    def _launch_rollout(self):
        """The device work of a WHOLE rollout in one launch (`ppo_rollout_all`): eps draw, then every workgroup runs
        the T steps of its own 32 envs with the env state in registers.  Bit for bit what T `_launch_step` calls leave."""
        pol, env, T = self.policy, self.env, self.rollout_size
        self._draw_noise()
        self._rows_applied.zero_()
        self._flag_rows()
        if self.gae == "episodic":
            # env.reset_buf is the env's own tensor before the first rollout and row T-1 of the previous rollout after it:
            # copied before this launch overwrites that row
            self._ended_prev.copy_(env.reset_buf)
        rec = env.recorder
        if rec is not None:
            # the launch writes env 0's pose of step t to row t of the record: frames of rows the host has not reached are
            # rendered first (none unless a rollout was cut short), then the record is (re)registered
            rec.buffer(T)
            rec.flush()
            _lib.api().fly_set_pose_record(env._handle, rec.poses)
        # env._bufs.reset / .progress point at the CURRENT flags (the env's own tensors, or the last row of the previous
        # rollout): the launch reads them once, then writes step t's flags to row t
        _lib.api().ppo_rollout_all(
            env._handle, C.byref(env._bufs), pol.P, pol.PF, self._obs_ring, self._eps_all, self._action_var, self._var_decay,
            self._var_min, self.all_acts, self.all_log_prob, self._v_ring, self.all_reward, T, self._rows_applied,
            pol.infer_pb_ptr(), self._reset_rows, self._progress_rows, _lib.stream_ptr())

    def _after_step(self, t):
        """Host-side state of a step that has been issued (launched or replayed): rows whose score / variance
        bookkeeping is pending (ppo.py:233, :236-237, applied by _flush_bookkeeping) and how many rows of
        v(obs_t) the rollout's policy launches have left for make_data."""
        if t == 0:
            self._book_from = 0
            self._v_have, self._v_version = 1, self.policy.version
        elif self._v_have == t:
            self._v_have = t + 1
        self._rows_done = t + 1

    SCORE_LINE = 'Steps: {:04d} | Opt Step: {:04d} | Reward {:.04f} | Action Var {:.04f}'

    def _emit(self, text):
        """A log line, behind whatever is still pending (see `_async_log`)."""
        self._log_q.append(text)
        self._drain_log()

    def _throughput_suffix(self):
        """' | Env-steps/s ...' for the score line when `log_throughput` is on: env steps of all ranks since the previous score
        line over the host's wall clock (inside a rollout that runs as ONE launch the host counts ahead of the device, so a
        window is exact only from rollout boundary to rollout boundary; over several windows it is the loop's rate)."""
        if not self.log_throughput:
            return ""
        import time
        now, mark = time.perf_counter(), self._rate_mark
        self._rate_mark = (now, self.run_step)
        if mark is None or now <= mark[0]:
            return " | Env-steps/s n/a"
        steps = (self.run_step - mark[1]) * int(self.args.num_envs) * self.world_size
        return " | Env-steps/s {:.4g}".format(steps / (now - mark[0]))

    def _emit_score(self):
        """ppo.py:257-260: the score line of this step.  Values are read from the device asynchronously (pinned memory + event);
        the accumulator is cleared on the stream, behind the copy."""
        rank0 = self.options.rank == 0
        suffix = self._throughput_suffix()
        if not self._async_log:
            self._drain_log(block=True)
            score = float(self._score_acc.item())
            self._score_acc.zero_()
            if self._episode_stats:
                suffix += self._episode_suffix(self._ep_window.tolist())
                self._ep_window.copy_(self._ep_empty)
            if self._update_stats:
                suffix += update_stats_suffix(self._us_window.tolist())
                self._us_window.copy_(self._us_empty)
            if rank0:
                print(self.SCORE_LINE.format(self.run_step, self.optim_step, score, self._action_var[0].item()) + suffix)
            return
        dev_vals = torch.stack((self._score_acc.reshape(()), self._action_var[0]))
        host = torch.empty(2, dtype=torch.float32, pin_memory=True)
        host.copy_(dev_vals, non_blocking=True)
        window = None
        if self._episode_stats:
            # the window's ten float64 numbers by the same route; the window starts anew on the stream, behind the copy
            window = torch.empty(_lib.EPISODE_SET, dtype=torch.float64, pin_memory=True)
            window.copy_(self._ep_window, non_blocking=True)
            self._ep_window.copy_(self._ep_empty)
        us_window = None
        if self._update_stats:
            us_window = torch.empty(_lib.UPDATE_STATS_SET, dtype=torch.float64, pin_memory=True)
            us_window.copy_(self._us_window, non_blocking=True)
            self._us_window.copy_(self._us_empty)
        ev = torch.cuda.Event()
        ev.record()
        self._score_acc.zero_()
        self._log_q.append((ev, host, dev_vals, self.run_step, self.optim_step, rank0, suffix, window, us_window))
        self._drain_log()

    def _drain_log(self, block=False):
        """Write the queued lines whose values have arrived, in order; block=True waits for all of them."""
        q = self._log_q
        while q:
            head = q[0]
            if isinstance(head, str):
                print(head)
            else:
                ev, host, _keep, run_step, optim_step, rank0, suffix, window, us_window = head
                if block:
                    ev.synchronize()
                elif not ev.query():
                    return
                if window is not None:
                    suffix += self._episode_suffix(window.tolist())
                if us_window is not None:
                    suffix += update_stats_suffix(us_window.tolist())
                if rank0:
                    print(self.SCORE_LINE.format(run_step, optim_step, float(host[0]), float(host[1])) + suffix)
            q.popleft()

    def flush_log(self):
        """Blocks until every queued log line has been written (a host sync when one is pending)."""
        self._drain_log(block=True)

    def _check_step_counter(self):
        """The deferred half of _update_hip's step check: the device counter copied at the end of the previous update."""
        if self._pending_step is None:
            return
        ev, host, expect = self._pending_step
        self._pending_step = None
        ev.synchronize()
        if int(host[0]) != expect:
            raise _lib.FlyHipError("update: the device step counter says %d optimizer steps, %d were issued"
                                   % (int(host[0]), expect))

    def run(self):
        """ppo.py:204-264: one env step of the rollout (and an update when the rollout is full).
        `graph=True` replays the device work of a whole rollout from ONE captured hipGraph (the first
        rollout runs eagerly, the second captures)."""
        t = self.mini_batch_number
        end = self.env.end
        if self._fwd_args is None or self._args_infer_gemm != self.policy.gemm_infer:
            self._prepare_step_args()                               # (re)built when the inference arithmetic changes
        if self._graphs_form != getattr(self.env, "launch_form", 0):
            self._graphs = {}                                       # randomisation turned on / off: captured kernels are stale
            self._graphs_form = self.env.launch_form
        rec = self.env.recorder
        step_s = self.env.render_count                              # the env step this call runs (record.py)
        if rec is not None:
            rec.buffer(self.rollout_size)
        with torch.no_grad():
            if self.persistent_rollout:
                if t == 0:
                    self._launch_rollout()
                env = self.env
                env.obs_buf, env.reward_buf = self._obs_rows[t + 1], self._reward_rows[t]
                env._bufs.obs, env._bufs.reward = self._buf_ptrs[t]
                env.reset_buf, env.progress_buf = self._reset_rows[t], self._progress_rows[t]      # this step's flags (fly.py:175-177)
                env._bufs.reset, env._bufs.progress = env.reset_buf.data_ptr(), env.progress_buf.data_ptr()
                self._after_step(t)
                env.render_count += 1
            elif not self.use_graph or self.run_step < self.rollout_size:
                self._launch_step(t)
            else:
                # graph=True: the device work of a WHOLE rollout (eps draw + T one-launch env steps) is one
                # captured hipGraph, replayed when the rollout's first step is asked for; the later run() calls of
                # the rollout only advance the host-side counters.  (A graph per step cannot win: the step is
                # GPU-bound and every replay pays a graph launch of its own -- tools/graph_vs_eager.py.)  The
                # deferred bookkeeping makes this exact: row t's launch carries the frozen row index, the
                # device word `_rows_applied` is zeroed inside the graph, and a flush only ever covers the rows
                # the HOST has counted as done.
                if t == 0:
                    key = bool(self.args.testing)
                    g = self._graphs.get(key)
                    if g is None:
                        g = torch.cuda.CUDAGraph()
                        g.register_generator_state(self._gen)
                        torch.cuda.synchronize(self.device)
                        count = self.env.render_count               # capturing runs no env step
                        with torch.cuda.graph(g):
                            for tt in range(self.rollout_size):
                                self._launch_step(tt)
                        self.env.render_count = count
                        self._graphs[key] = g
                    g.replay()
                self.env.obs_buf, self.env.reward_buf = self._obs_rows[t + 1], self._reward_rows[t]
                self.env._bufs.obs, self.env._bufs.reward = self._buf_ptrs[t]
                self._after_step(t)
                self.env.render_count += 1
            if rec is not None:
                rec.reached(t, step_s)
                if t + 1 == self.rollout_size:
                    rec.flush()                                     # before the next rollout overwrites the record

        if t + 1 == self.rollout_size:                              # ppo.py:240-252
            if self._episode_stats:
                with torch.no_grad():
                    self._episode_stats_pass()                      # the rollout's rows are complete; in testing too
            self._flush_bookkeeping()                               # the update reads the decayed variance
            if not self.args.testing:
                self._emit("Training")
                self.update()
            self.mini_batch_number = 0
            with torch.no_grad():
                self._obs_ring[0].copy_(self._obs_ring[self.rollout_size])
            self.env.bind_obs(self._obs_ring[0])
            if getattr(self.args, "save", False) and self.optim_step % self.args.save_freq == 0 and self.optim_step != 0:
                self._emit("saving...")
                self._in_run_tail = True                            # this call's `run_step += 1` is still to come (save_training_state)
                try:
                    self.save(str(self.optim_step))
                finally:
                    self._in_run_tail = False
                self._emit("saved!")
        else:
            self.mini_batch_number += 1

        if self.run_step % self.num_eval_freq == 0:                 # ppo.py:257-260
            self._flush_bookkeeping()
            self._emit_score()
            self.score = 0
        elif self._log_q:
            self._drain_log()

        self.run_step += 1
        return end

    def save(self, endofname=""):
        """ppo.py:266-273: state_dict only, reference key names, written by rank 0.  With `save_state` EVERY rank also writes
        its training state beside it (save_training_state) -- at a rollout boundary; inside a rollout only the weights."""
        if not getattr(self.args, "save", False):
            return
        self._check_step_counter()
        rank = self.options.rank
        path = self.args.save_path + endofname + ".pth"
        if rank == 0:
            # parameters are views of the packed buffer: save compact, contiguous copies
            sd = {k: v.detach().clone().contiguous() for k, v in self.net.state_dict().items()}
            if self.normalize_obs:                                  # only then: otherwise the file is the reference's
                sd["obs_rms.mean"], sd["obs_rms.var"], sd["obs_rms.count"] = self.obs_mean, self.obs_var, self.obs_count
            if self.normalize_value:
                sd["value_rms.mean"], sd["value_rms.var"], sd["value_rms.count"] = self.value_mean, self.value_var, self.value_count
            if self.normalize_reward:
                sd["reward_rms.mean"], sd["reward_rms.var"], sd["reward_rms.count"] = (
                    self._rnorm_stats[1].clone(), self.reward_var, self.reward_count)
            torch.save(sd, path)
        if not getattr(self.args, "save_state", False):
            return
        if self.mini_batch_number != 0:
            # with one launch per rollout the device is a whole rollout ahead of the host: there is no state "at step t"
            if rank == 0:
                self._emit("save_state: step %d of %d of a rollout: %s holds the weights only, no training state; the last periodic "
                           "save is the one to resume from" % (self.mini_batch_number, self.rollout_size, path))
                self.flush_log()
            return
        self.save_training_state(self.training_state_path(path, rank))

    # ------------------------------------------------------------------------------------------
    # exact resume (opt-in: `save_state`, `resume`)
    training_state_path = staticmethod(train_state.training_state_path)

    def _training_state_meta(self):
        """The meta block of THIS run: the args' (train_state.expected_meta), with what the live objects report in place of
        what the args predict."""
        meta = train_state.expected_meta(self.args)
        meta.update(rollout_size=int(self.rollout_size), gemm=self.policy.gemm, step_gemm=self.policy.step_gemm,
                    persistent_rollout=bool(self.persistent_rollout), dp_mode=self.dp_mode)
        return meta

    def save_training_state(self, path):
        """Everything between the kernels and the public interface that the next rollout and update read, into `path`
        (train_state.py has the format): with the weights file beside it, a new process continues this run bit for bit.
        Only at a ROLLOUT BOUNDARY (mini_batch_number == 0: after the update, after ring[0] <- ring[T]); ValueError inside a
        rollout.  Host-synchronising; the log queue is drained first.  Not restored, so not stored: the recorder, the
        peer-to-peer windows (prepare() reopens them), and the torch backend's optimizer (ValueError)."""
        if self.mini_batch_number != 0:
            raise ValueError("save_training_state: step %d of %d of a rollout; a training state exists only at a rollout boundary"
                             % (self.mini_batch_number, self.rollout_size))
        if self.update_backend != "hip":
            raise ValueError("save_training_state: update_backend=%r keeps its optimizer state in torch.optim.Adam, which is not "
                             "part of a training state" % (self.update_backend,))
        self._flush_bookkeeping()
        self._check_step_counter()
        self.flush_log()
        run_step = self.run_step
        if self._in_run_tail:
            # run()'s periodic save: the call still has its score check and `run_step += 1` ahead.  No score line is due there
            # (rollout_size is a multiple of 16, so run_step is odd), so the state is the one after the call.
            assert run_step % self.num_eval_freq != 0
            run_step += 1
        pack = train_state.pack
        agent = {"run_step": int(run_step), "optim_step": int(self.optim_step), "action_var": pack(self._action_var),
                 "score_acc": pack(self._score_acc), "generator": pack(self._gen.get_state()), "obs_row0": pack(self._obs_ring[0])}
        if self.action_noise == "ar1":
            agent["noise_carry"], agent["noise_carry_drawn"] = pack(self._noise_carry), bool(self._noise_carry_drawn)
        if self.minibatch == "shuffled":
            agent["mb_update"] = int(self._mb_update)
        if self.gae == "episodic":
            agent["ended_prev"] = pack(self._ended_prev)
        if self.normalize_obs:
            agent["obs_stats"], agent["obs_table"] = pack(self._obs_stats), pack(self._obs_table)
        if self.normalize_value:
            for k in ("value_stats", "value_table", "value_stats_next", "value_table_next"):
                agent[k] = pack(getattr(self, "_" + k))
        if self.normalize_reward:
            agent["reward_norm"] = {k: pack(getattr(self, "_rnorm_" + k)) for k in train_state.REWARD_NORM_KEYS}
        if self._episode_stats:
            agent["episode_stats"] = {k: pack(getattr(self, "_ep_" + k)) for k in ("carry_ret", "carry_len", "window", "total")}
        if self._update_stats:
            agent["update_stats"] = {k: pack(getattr(self, "_us_" + k)) for k in ("last", "window", "total")}
        state = {"format": train_state.FORMAT, "meta": self._training_state_meta(),
                 "meta_ext": train_state.expected_meta_ext(self.args), "policy": self.policy.training_state(),
                 "agent": agent, "env": self.env.training_state()}
        tmp = path + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, path)                                       # a run cut off in the middle of a save leaves the previous file whole

    def load_training_state(self, path=None):
        """save_training_state() back into this agent, in place; `path` defaults to the state file beside `args.resume_path`
        (already read and checked by the constructor).  Call it LAST: after a gemm selection and after broadcast_policy, which
        rebuild the planes and clear the fp16x2 calibration.  The meta is held against the live objects once more (a gemm set
        after construction), and the float64 statistics the weights file carried must be the state file's."""
        if path is None and self._resume_state is not None:
            state = self._resume_state
        else:
            if path is None:
                if self.options.resume_path is None:
                    raise ValueError("load_training_state: no path given and no args.resume_path")
                path = self.training_state_path(self.options.resume_path, self.options.rank)
            state = train_state.read_state_file(path)
        self._resume_state = None
        if self.mini_batch_number != 0:
            raise ValueError("load_training_state: step %d of %d of a rollout; a training state goes in only at a rollout boundary"
                             % (self.mini_batch_number, self.rollout_size))
        if self.update_backend != "hip":
            raise ValueError("load_training_state: update_backend=%r is not part of a training state" % (self.update_backend,))
        train_state.compare_meta(state.get("meta"), self._training_state_meta())
        train_state.check_meta_ext(state.get("meta_ext"), self.args)
        train_state.check_reward_norm(state, self.normalize_reward)
        agent = train_state.block(state, "agent")
        restore, value = train_state.restore, train_state.value
        for mine, blk, key, on in ((getattr(self, "_obs_stats", None), agent, "obs_stats", self.normalize_obs),
                                   (getattr(self, "_value_stats", None), agent, "value_stats", self.normalize_value),
                                   (getattr(self, "_rnorm_stats", None), agent.get("reward_norm"), "stats", self.normalize_reward)):
            if on and torch.is_tensor(blk.get(key)) and not torch.equal(mine.cpu(), blk[key]):
                what = key if blk is agent else "reward_norm." + key
                raise ValueError("training state: %s of the weights file %s and of the state file disagree; they are not of the same "
                                 "save" % (what, mine.cpu().tolist()[:3]))
        self._check_step_counter()
        self.flush_log()
        self.policy.load_training_state(train_state.block(state, "policy"))
        self.env.load_training_state(train_state.block(state, "env"))
        self.run_step, self.optim_step = value(agent, "agent", "run_step", int), value(agent, "agent", "optim_step", int)
        self._flush_bookkeeping()                                   # (an agent that has run: nothing pending on the old variance)
        restore(self._action_var, agent, "agent", "action_var")
        restore(self._score_acc, agent, "agent", "score_acc")
        gen = self._gen.get_state()
        restore(gen, agent, "agent", "generator")
        self._gen.set_state(gen)
        restore(self._obs_ring[0], agent, "agent", "obs_row0")
        self._v_have = 0
        if self.action_noise == "ar1":
            restore(self._noise_carry, agent, "agent", "noise_carry")
            self._noise_carry_drawn = value(agent, "agent", "noise_carry_drawn", bool)
        if self.minibatch == "shuffled":
            self._mb_update = value(agent, "agent", "mb_update", int)
        if self.gae == "episodic":
            restore(self._ended_prev, agent, "agent", "ended_prev")
        if self.normalize_obs:
            restore(self._obs_stats, agent, "agent", "obs_stats")
            restore(self._obs_table, agent, "agent", "obs_table")
        if self.normalize_value:
            for k in ("value_stats", "value_table", "value_stats_next", "value_table_next"):
                restore(getattr(self, "_" + k), agent, "agent", k)
        if self.normalize_reward:
            for k in train_state.REWARD_NORM_KEYS:
                restore(getattr(self, "_rnorm_" + k), agent["reward_norm"], "agent.reward_norm", k)
        if self._episode_stats:
            if isinstance(agent.get("episode_stats"), dict):
                for k in ("carry_ret", "carry_len", "window", "total"):
                    restore(getattr(self, "_ep_" + k), agent["episode_stats"], "agent.episode_stats", k)
            else:
                # a state saved without the flag: the env's step count is the open episodes' length (an env whose end flag is
                # up has no open episode: its count is reset in the step to come), their return so far is gone
                with torch.no_grad():
                    self._ep_carry_len.copy_(self.env.progress_buf * (self.env.reset_buf == 0))
                    self._ep_carry_ret.zero_()
                    self._ep_window.copy_(self._ep_empty)
                    self._ep_total.copy_(self._ep_empty)
                print("episode_stats: the training state holds no episode statistics; each env's first closed return after "
                      "the resume is partial (its length is whole)")
        if self._update_stats:
            if isinstance(agent.get("update_stats"), dict):
                for k in ("last", "window", "total"):
                    restore(getattr(self, "_us_" + k), agent["update_stats"], "agent.update_stats", k)
            else:
                with torch.no_grad():
                    for k in ("last", "window", "total"):
                        getattr(self, "_us_" + k).copy_(self._us_empty)
                print("update_stats: the training state holds no update statistics; the totals start at this resume")
        self._rate_mark = None
        torch.cuda.synchronize(self.device)

    def generate_video(self):
        return self.env.generate_video()

    def exit(self):
        self._check_step_counter()
        self.flush_log()
        if self._p2p is not None:
            self._p2p.close()
            self._p2p = None
        self.env.exit()
