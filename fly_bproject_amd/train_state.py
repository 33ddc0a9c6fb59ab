"""The pure half of exact training resume (`--save_state` / `--resume_path`): the state file's name, its
`meta` block and the strict check of it, and the helpers that move a tensor between a live object and the file's dict.

A state file is ONE dict written by torch.save with every tensor on the CPU -- tensors, numbers, strings, lists and dicts only,
so it loads with `torch.load(..., weights_only=True)`:

    {"format": 1, "meta": {...}, "policy": {...}, "agent": {...}, "env": {...}}

`meta` names everything the MEANING of the three state blocks depends on: the shapes (num_envs, rollout_size), which rank's
envs and draws these are, and every option that decides which state exists or how the next rollout and update read it.  A run
resumes a state only under exactly these values; to change one, start from the weights alone (`--load_path`).  Nothing here
touches a GPU: `check_meta` runs in `PPO.__init__` before the env exists.
"""
import os

import torch

FORMAT = 1
MINI_BATCH_SIZE, CHUNK_NUMBER = 40960, 16           # ppo.py:118-121: rollout_size = (40960 // num_envs) * 16
MAX_PERSISTENT_ROLLOUT = 4096                       # one launch per rollout up to this many steps (PPO.persistent_rollout)

META_FIELDS = ("num_envs", "rollout_size", "variant", "reward", "world_size", "rank", "gae", "minibatch", "minibatch_seed",
               "action_noise", "noise_rho", "normalize_obs", "obs_clip", "normalize_value", "normalize_advantage", "randomize",
               "dr_ranges", "dr_seed", "gemm", "step_gemm", "persistent_rollout", "dp_mode")


def training_state_path(weights_path, rank):
    """The state file that goes with a weights file: "a/b_300.pth", 1 -> "a/b_300.state.r1.pth"."""
    path = str(weights_path)
    base = path[:-len(".pth")] if path.endswith(".pth") else path
    return "%s.state.r%d.pth" % (base, int(rank))


def resolve_gemm(args):
    """(gemm, step_gemm) as PackedPolicy starts with them ($FLY_GEMM, $FLY_STEP_GEMM) and `trainer.main` then sets them from
    `--gemm`: what `policy.gemm` / `policy.step_gemm` report once the run is set up."""
    env_gemm = os.environ.get("FLY_GEMM")
    gemm = "bf16x3" if env_gemm in (None, "f16x2") else env_gemm
    step = os.environ.get("FLY_STEP_GEMM", "f16x2" if env_gemm in (None, "f16x2") else "bf16x3")
    want = getattr(args, "gemm", None)
    if want == "f16x2":
        gemm, step = "bf16x3", "f16x2"
    elif want:
        gemm, step = want, "bf16x3"
    return gemm, (step if gemm == "bf16x3" else gemm)


def expected_meta(args):
    """The meta block of the run that `args` describes, from the args (and the environment variables the options default to)
    alone.  An option that is off stores None for its dependent values (`noise_rho` without ar1, `obs_clip` without
    normalize_obs, the seeds and ranges of features that are off): they mean nothing then, and must not block a resume."""
    from .fly import DR_NAMES, dr_args
    n = int(args.num_envs)
    rank = int(getattr(args, "rank", 0) or 0)
    T = (MINI_BATCH_SIZE // n) * CHUNK_NUMBER
    minibatch = getattr(args, "minibatch", "reference")
    mb_seed = None
    if minibatch == "shuffled":
        mb_seed = getattr(args, "minibatch_seed", None)
        if mb_seed is None:
            mb_seed = getattr(args, "seed", 0)
        mb_seed = (int(mb_seed) + rank * 0x9E3779B9) & 0xFFFFFFFF
    action_noise = getattr(args, "action_noise", "white")
    normalize_obs = bool(getattr(args, "normalize_obs", False))
    randomize = bool(getattr(args, "randomize", False))
    dr_ranges = dr_seed = None
    if randomize:
        ranges, dr_seed = dr_args(args)
        dr_ranges = [[float(ranges[k][0]), float(ranges[k][1])] for k in DR_NAMES]
    want = getattr(args, "persistent_rollout", None)
    if want is None:
        want = os.environ.get("FLY_PERSISTENT_ROLLOUT", "1") != "0"
    gemm, step_gemm = resolve_gemm(args)
    return {
        "num_envs": n, "rollout_size": T, "variant": getattr(args, "variant", "bigGrav"),
        "reward": getattr(args, "reward", "standing"), "world_size": int(getattr(args, "world_size", 1)), "rank": rank,
        "gae": getattr(args, "gae", "reference"), "minibatch": minibatch, "minibatch_seed": mb_seed,
        "action_noise": action_noise, "noise_rho": float(getattr(args, "noise_rho", 0.5)) if action_noise == "ar1" else None,
        "normalize_obs": normalize_obs, "obs_clip": float(getattr(args, "obs_clip", 5.0)) if normalize_obs else None,
        "normalize_value": bool(getattr(args, "normalize_value", False)),
        "normalize_advantage": bool(getattr(args, "normalize_advantage", False)),
        "randomize": randomize, "dr_ranges": dr_ranges, "dr_seed": dr_seed, "gemm": gemm, "step_gemm": step_gemm,
        "persistent_rollout": bool(want) and T <= MAX_PERSISTENT_ROLLOUT and not bool(getattr(args, "graph", False)),
        "dp_mode": getattr(args, "dp_mode", "grad_allreduce"),
    }


def compare_meta(file_meta, run_meta):
    """Strict: every field of META_FIELDS is in the file and equals the run's, else ValueError naming the first field that is
    not, with both values."""
    if not isinstance(file_meta, dict):
        raise ValueError("training state: no meta block")
    for field in META_FIELDS:
        if field not in file_meta:
            raise ValueError("training state: the meta block lacks %s" % field)
        if file_meta[field] != run_meta[field] or type(file_meta[field]) is not type(run_meta[field]):
            raise ValueError("training state: %s is %r in the state file and %r in this run; a state resumes only under the "
                             "options it was saved with (--load_path takes the weights alone)"
                             % (field, file_meta[field], run_meta[field]))


def check_meta(file_meta, args):
    """The meta check: the file's meta and the resuming run's args go in, it returns or raises ValueError."""
    compare_meta(file_meta, expected_meta(args))


def check_format(state):
    """ValueError unless `state` is a state dict of a format this build reads."""
    if not isinstance(state, dict) or "format" not in state:
        raise ValueError("not a training state file (no format number): was it written by --save_state?")
    if state["format"] != FORMAT:
        raise ValueError("training state of unknown format %r (this build reads format %d)" % (state["format"], FORMAT))


def read_state_file(path):
    """The dict of a state file, tensors on the CPU, its format checked.  A missing file is an error of its own."""
    if not os.path.isfile(path):
        raise FileNotFoundError("no training state file %s (a weights file resumes only beside the state files its --save_state "
                                "run wrote, one per rank)" % path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    check_format(state)
    return state


def block(state, name):
    if not isinstance(state.get(name), dict):
        raise ValueError("training state: the %s block is missing" % name)
    return state[name]


def value(blk, where, key, kind):
    """A number / flag of a state block, of exactly the type `kind`."""
    if key not in blk:
        raise ValueError("training state: %s.%s is missing" % (where, key))
    if type(blk[key]) is not kind:
        raise ValueError("training state: %s.%s is %r, not %s" % (where, key, blk[key], kind.__name__))
    return blk[key]


def pack(t):
    """A tensor as it goes into the file: a contiguous CPU copy."""
    return t.detach().to("cpu", copy=True).contiguous()


def restore(dst, blk, where, key):
    """dst <- blk[key], IN PLACE (launch arguments, registered tables and parameter views hold dst's address).  The file's
    tensor must have dst's shape and dtype exactly."""
    if key not in blk:
        raise ValueError("training state: %s.%s is missing" % (where, key))
    src = blk[key]
    if not torch.is_tensor(src) or tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        got = "%s %s" % (tuple(src.shape), src.dtype) if torch.is_tensor(src) else type(src).__name__
        raise ValueError("training state: %s.%s is %s, this run holds %s %s" % (where, key, got, tuple(dst.shape), dst.dtype))
    with torch.no_grad():
        dst.copy_(src)
