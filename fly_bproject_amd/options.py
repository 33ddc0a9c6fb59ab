"""The options of a run, written down once: the table of names, defaults, choices and environment variables, the constants of
the reference's rollout shape, and the resolver that turns `args` (an argparse namespace, or any object with some of the
attributes) and the environment into one immutable record of resolved and validated values.

`trainer.parse_args` takes its defaults and choices from the table, `Fly.__init__` reads the env's options through
`resolve_env`, `PPO.__init__` resolves the whole record before anything exists that a bad value could leave behind, and
`train_state.expected_meta` is a projection of that record.  Nothing here touches a GPU or imports the agent.
"""
import collections
import dataclasses

MINI_BATCH_SIZE, CHUNK_NUMBER = 40960, 16           # ppo.py:118-121: rollout_size = (40960 // num_envs) * 16
MAX_PERSISTENT_ROLLOUT = 4096                       # one launch per rollout up to this many steps (PPO.persistent_rollout)
RANK_SEED_STRIDE = 0x9E3779B9                       # rank r of a data-parallel run draws with seed + r * this (mod 2^32)

# per-env physics domain randomisation (include/flyhip.h, fly_set_randomization): multipliers of these FlyConfig values, in
# this order; `mass` scales the inertia too
DR_NAMES = ("kp", "kd", "effort", "mass", "mu", "gravity")
# trainer.py's starting ranges (--dr_*): not tuned
DR_DEFAULT_RANGES = {"kp": (0.8, 1.2), "kd": (0.8, 1.2), "effort": (1.0, 1.0), "mass": (0.8, 1.2), "mu": (0.5, 1.5),
                     "gravity": (1.0, 1.0)}

# `default` is what a run gets when neither the args nor `env` name a value.  An option with an `env` is open while its
# attribute is None (the flag's default, see flag_default): the variable then decides, and the default after it.
Option = collections.namedtuple("Option", "name default choices env", defaults=(None, None))

OPTIONS = (
    Option("sim_device", "cuda:0"), Option("rl_device", None), Option("compute_device_id", 0), Option("graphics_device_id", 0),
    Option("num_envs", 1000), Option("headless", False), Option("rank", 0), Option("world_size", 1), Option("seed", 0),
    Option("max_steps", 0), Option("testing", False),
    Option("save", False), Option("save_path", None), Option("save_freq", 100), Option("save_state", False),
    Option("load", False), Option("load_path", None), Option("resume", False), Option("resume_path", None),
    Option("record", False), Option("record_dir_name", None), Option("time_steps_per_recorded_frame", 2),
    Option("variant", "bigGrav", ("bigGrav", "lowGrav")), Option("reward", "standing", ("standing", "walking")),
    Option("randomize", False), Option("dr_seed", None),
    *(Option("dr_" + name, DR_DEFAULT_RANGES[name]) for name in DR_NAMES),
    Option("gae", "reference", ("reference", "episodic")),
    Option("minibatch", "reference", ("reference", "shuffled")), Option("minibatch_seed", None),
    Option("action_noise", "white", ("white", "ar1")), Option("noise_rho", 0.5),
    Option("normalize_obs", False), Option("obs_clip", 5.0), Option("normalize_value", False),
    Option("normalize_advantage", False), Option("lambda_returns", False), Option("episode_stats", False),
    Option("normalize_reward", False), Option("reward_clip", 10.0), Option("update_stats", False),
    Option("graph", False), Option("reuse_rollout_values", True), Option("log_throughput", False),
    Option("persistent_rollout", True, env="FLY_PERSISTENT_ROLLOUT"), Option("async_log", True, env="FLY_ASYNC_LOG"),
    Option("update_backend", "hip"), Option("dp_mode", "grad_allreduce", ("grad_allreduce", "param_average")),
    Option("dp_allreduce", "rccl", ("rccl", "p2p", "auto"), "FLY_DP_ALLREDUCE"),
    # gemm names EVERY GEMM ("f16x2": bf16x3 + the fp16x2 optimizer step); step_gemm has no flag, its variable names the
    # arithmetic of the fused optimizer-step gradient alone (bf16x3 | f16x2, held by PackedPolicy), under a gemm that the
    # args leave open (resolve_gemm)
    Option("gemm", "f16x2", ("f32", "bf16x3", "f16x2"), "FLY_GEMM"), Option("step_gemm", None, env="FLY_STEP_GEMM"),
)
BY_NAME = {o.name: o for o in OPTIONS}


def flag_default(name):
    """The default of the command-line flag: the table's, or None (open) where an environment variable comes first."""
    return None if BY_NAME[name].env else BY_NAME[name].default


def choices(name):
    return list(BY_NAME[name].choices)


def _get(args, name):
    return getattr(args, name, BY_NAME[name].default)


def _wanted(args, environ, name):
    """args.<name>; left open there (None, or an empty string), the option's environment variable; without it, the default."""
    opt = BY_NAME[name]
    v = getattr(args, name, None)
    if v is not None and v != "":
        return v
    if isinstance(opt.default, bool):
        return environ.get(opt.env, "1") != "0"
    return environ.get(opt.env, opt.default)


def _choice(name, v):
    c = BY_NAME[name].choices
    if v not in c:
        raise ValueError("%s must be %s or %s (got %r)" % (name, ", ".join(c[:-1]), c[-1], v))
    return v


def dr_args(args):
    """(ranges, seed) of `args.randomize`: the --dr_* ranges (defaults DR_DEFAULT_RANGES), and --dr_seed (default --seed)
    offset by the rank, so that the ranks of a data-parallel run draw different constants."""
    ranges = {}
    for name in DR_NAMES:
        v = getattr(args, "dr_" + name, None)
        ranges[name] = tuple(v) if v is not None else DR_DEFAULT_RANGES[name]
    seed = _get(args, "dr_seed")
    if seed is None:
        seed = _get(args, "seed") or 0
    return ranges, (int(seed) + RANK_SEED_STRIDE * int(_get(args, "rank") or 0)) % (1 << 32)


def wanted_gemm(args):
    """--gemm as resolve_gemm takes it: the value, validated, or None while the args leave it open."""
    want = getattr(args, "gemm", None) or None
    return want if want is None else _choice("gemm", want)


def resolve_gemm(want, environ):
    """(gemm, step_gemm) as `policy.gemm` / `policy.step_gemm` report them once a run is set up.  `want` (--gemm, or None)
    names every GEMM, the optimizer step included; left open, the two environment variables decide, and f16x2 after them.
    "f16x2" is bf16x3 everywhere with the fused optimizer step in fp16x2; under f32 the step is f32 too."""
    if want:
        gemm, step = want, None
    else:
        gemm, step = environ.get(BY_NAME["gemm"].env, BY_NAME["gemm"].default), environ.get(BY_NAME["step_gemm"].env)
    if gemm == "f16x2":
        gemm, step = "bf16x3", step or "f16x2"
    return gemm, ((step or "bf16x3") if gemm == "bf16x3" else gemm)


@dataclasses.dataclass(frozen=True)
class EnvOptions:
    """What `Fly` takes from the args."""
    num_envs: int
    rank: int
    variant: str
    reward: str
    randomize: bool
    dr_ranges: tuple                # (lo, hi) per DR_NAMES entry, as dr_args gives them
    dr_seed: int                    # this rank's
    record: bool                    # rank 0 only
    record_dir_name: str
    time_steps_per_recorded_frame: int


@dataclasses.dataclass(frozen=True)
class Options(EnvOptions):
    """What `PPO` takes from the args and the environment, with what follows from it."""
    world_size: int
    seed: int
    resume: bool
    resume_path: object
    load: bool
    gae: str
    minibatch: str
    minibatch_seed: int             # this rank's (`minibatch_seed`, default `seed`, + rank * RANK_SEED_STRIDE, wrapping)
    action_noise: str
    noise_rho: float
    normalize_obs: bool
    obs_clip: float
    normalize_value: bool
    normalize_advantage: bool
    lambda_returns: bool
    episode_stats: bool             # observes only: not part of a training state's meta (projection)
    normalize_reward: bool          # not in the meta either: a training state says it by holding agent["reward_norm"]
    reward_clip: float              # a launch argument, not state: a resume may change it
    update_stats: bool              # observes only, like episode_stats: not in the meta
    graph: bool
    reuse_rollout_values: bool
    log_throughput: bool
    async_log: bool                 # wanted: the agent logs asynchronously only on a GPU
    update_backend: str
    dp_mode: str
    dp_allreduce: str
    gemm: str
    step_gemm: str
    mini_chunk_size: int
    rollout_size: int
    persistent_rollout: bool


def _env_fields(args):
    rank = int(_get(args, "rank") or 0)
    ranges, dr_seed = dr_args(args)
    return dict(num_envs=int(args.num_envs), rank=rank, variant=_choice("variant", _get(args, "variant")),
                reward=_choice("reward", _get(args, "reward")), randomize=bool(_get(args, "randomize")),
                dr_ranges=tuple(ranges[k] for k in DR_NAMES), dr_seed=dr_seed, record=bool(_get(args, "record")) and rank == 0,
                record_dir_name=_get(args, "record_dir_name") or "recording",
                time_steps_per_recorded_frame=_get(args, "time_steps_per_recorded_frame"))


def resolve_env(args):
    """The env's part of the record: a `Fly` stands on its own, at any num_envs."""
    return EnvOptions(**_env_fields(args))


def resolve(args, environ):
    """The record of the run that `args` and `environ` describe, or ValueError for a value no run can have."""
    gae = _choice("gae", _get(args, "gae"))
    minibatch = _choice("minibatch", _get(args, "minibatch"))
    action_noise = _choice("action_noise", _get(args, "action_noise"))
    noise_rho = float(_get(args, "noise_rho"))
    if not 0.0 < noise_rho < 1.0:
        raise ValueError("noise_rho must be in (0, 1) (got %r)" % (noise_rho,))
    resume, load, resume_path = bool(_get(args, "resume")), bool(_get(args, "load")), _get(args, "resume_path")
    if resume:
        if load:
            raise ValueError("resume and load exclude each other: resume_path names the weights file too")
        if _get(args, "testing"):
            raise ValueError("resume continues a training run: it has no meaning with testing")
        if resume_path is None:
            raise ValueError("resume needs resume_path: a weights file written by a save_state run")
    n = int(args.num_envs)
    mini_chunk_size = MINI_BATCH_SIZE // n                          # ppo.py:120 (Q9: 0 for N > 40960)
    if mini_chunk_size < 1:
        raise ValueError("num_envs=%d gives mini_chunk_size 0 (ppo.py:120); use num_envs <= 40960" % n)
    rollout_size = mini_chunk_size * CHUNK_NUMBER
    normalize_obs, obs_clip = bool(_get(args, "normalize_obs")), float(_get(args, "obs_clip"))
    if normalize_obs and not obs_clip > 0.0:
        raise ValueError("obs_clip must be > 0 (got %r)" % obs_clip)
    normalize_reward, reward_clip = bool(_get(args, "normalize_reward")), float(_get(args, "reward_clip"))
    if normalize_reward and not reward_clip > 0.0:
        raise ValueError("reward_clip must be > 0 (got %r)" % reward_clip)
    dp_mode = _get(args, "dp_mode")
    if dp_mode not in BY_NAME["dp_mode"].choices:
        raise ValueError("dp_mode must be grad_allreduce or param_average")
    dp_allreduce = _wanted(args, environ, "dp_allreduce")
    if dp_allreduce not in BY_NAME["dp_allreduce"].choices:
        raise ValueError("dp_allreduce must be rccl, p2p or auto")
    gemm, step_gemm = resolve_gemm(wanted_gemm(args), environ)
    env = _env_fields(args)
    seed, graph = int(_get(args, "seed") or 0), bool(_get(args, "graph"))
    mb_seed = _get(args, "minibatch_seed")
    return Options(
        **env, world_size=int(_get(args, "world_size")), seed=seed, resume=resume, resume_path=resume_path, load=load, gae=gae,
        minibatch=minibatch, minibatch_seed=(int(seed if mb_seed is None else mb_seed) + env["rank"] * RANK_SEED_STRIDE) & 0xFFFFFFFF,
        action_noise=action_noise, noise_rho=noise_rho, normalize_obs=normalize_obs, obs_clip=obs_clip,
        normalize_value=bool(_get(args, "normalize_value")), normalize_advantage=bool(_get(args, "normalize_advantage")),
        lambda_returns=bool(_get(args, "lambda_returns")), episode_stats=bool(_get(args, "episode_stats")),
        normalize_reward=normalize_reward, reward_clip=reward_clip, update_stats=bool(_get(args, "update_stats")),
        graph=graph, reuse_rollout_values=bool(_get(args, "reuse_rollout_values")), log_throughput=bool(_get(args, "log_throughput")),
        async_log=bool(_wanted(args, environ, "async_log")), update_backend=_get(args, "update_backend"), dp_mode=dp_mode,
        dp_allreduce=dp_allreduce, gemm=gemm, step_gemm=step_gemm, mini_chunk_size=mini_chunk_size, rollout_size=rollout_size,
        persistent_rollout=bool(_wanted(args, environ, "persistent_rollout")) and rollout_size <= MAX_PERSISTENT_ROLLOUT and not graph)


def projection(o):
    """The record's statement of what a training state depends on (train_state.META_FIELDS and META_EXT_FIELDS).  An option
    that is off stores None for its dependent values (`noise_rho` without ar1, `obs_clip` without normalize_obs, the seeds and
    ranges of features that are off): they mean nothing then, and must not block a resume."""
    return {
        "num_envs": o.num_envs, "rollout_size": o.rollout_size, "variant": o.variant, "reward": o.reward,
        "world_size": o.world_size, "rank": o.rank, "gae": o.gae, "minibatch": o.minibatch,
        "minibatch_seed": o.minibatch_seed if o.minibatch == "shuffled" else None,
        "action_noise": o.action_noise, "noise_rho": o.noise_rho if o.action_noise == "ar1" else None,
        "normalize_obs": o.normalize_obs, "obs_clip": o.obs_clip if o.normalize_obs else None,
        "normalize_value": o.normalize_value, "normalize_advantage": o.normalize_advantage, "randomize": o.randomize,
        "dr_ranges": [[float(lo), float(hi)] for lo, hi in o.dr_ranges] if o.randomize else None,
        "dr_seed": o.dr_seed if o.randomize else None, "gemm": o.gemm, "step_gemm": o.step_gemm,
        "persistent_rollout": o.persistent_rollout, "dp_mode": o.dp_mode, "lambda_returns": o.lambda_returns,
    }
