"""The pure half of exact training resume (`--save_state` / `--resume_path`): the state file's name, its
`meta` block and the strict check of it, and the helpers that move a tensor between a live object and the file's dict.

A state file is ONE dict written by torch.save with every tensor on the CPU -- tensors, numbers, strings, lists and dicts only,
so it loads with `torch.load(..., weights_only=True)`:

    {"format": 1, "meta": {...}, "meta_ext": {...}, "policy": {...}, "agent": {...}, "env": {...}}

`meta` names everything the MEANING of the three state blocks depends on: the shapes (num_envs, rollout_size), which rank's
envs and draws these are, and every option that decides which state exists or how the next rollout and update read it.  A run
resumes a state only under exactly these values; to change one, start from the weights alone (`--load_path`).  `meta_ext`
holds the options that came after format 1 (`lambda_returns`), under the same rule; a file written before them has no such
block and resumes as a run with those options at their defaults -- so the format number did not have to move.  Nothing here
touches a GPU: `check_meta` runs in `PPO.__init__` before the env exists.
"""
import os

import torch

from . import options

FORMAT = 1

META_FIELDS = ("num_envs", "rollout_size", "variant", "reward", "world_size", "rank", "gae", "minibatch", "minibatch_seed",
               "action_noise", "noise_rho", "normalize_obs", "obs_clip", "normalize_value", "normalize_advantage", "randomize",
               "dr_ranges", "dr_seed", "gemm", "step_gemm", "persistent_rollout", "dp_mode")
# Options added after format 1 was fixed: their own top-level block of the file, "meta_ext", checked as strictly as `meta`.  A
# file without the block (or without a field) was written before the option existed, so it holds the option's default.
META_EXT_FIELDS = ("lambda_returns",)


def training_state_path(weights_path, rank):
    """The state file that goes with a weights file: "a/b_300.pth", 1 -> "a/b_300.state.r1.pth"."""
    path = str(weights_path)
    base = path[:-len(".pth")] if path.endswith(".pth") else path
    return "%s.state.r%d.pth" % (base, int(rank))


def resolve_gemm(args):
    """(gemm, step_gemm) as `policy.gemm` / `policy.step_gemm` report them once the run that `args` describes is set up
    (options.resolve_gemm has the rule)."""
    return options.resolve_gemm(options.wanted_gemm(args), os.environ)


def expected_meta(args):
    """The meta block of the run that `args` describes, from the args (and the environment variables the options default to)
    alone: the resolved record (options.resolve), projected onto META_FIELDS."""
    meta = options.projection(options.resolve(args, os.environ))
    return {field: meta[field] for field in META_FIELDS}


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


def expected_meta_ext(args):
    """The meta_ext block of the run that `args` describes: the resolved record, projected onto META_EXT_FIELDS."""
    meta = options.projection(options.resolve(args, os.environ))
    return {field: meta[field] for field in META_EXT_FIELDS}


def check_meta_ext(file_ext, args):
    """The meta_ext check, strict as compare_meta: `file_ext` is the file's meta_ext block, or None for a file that has none,
    `args` the resuming run's.  Every field of META_EXT_FIELDS must equal the run's -- a field the file lacks reads as the
    option's default -- else ValueError naming the first that does not, with both values."""
    if file_ext is not None and not isinstance(file_ext, dict):
        raise ValueError("training state: meta_ext is no block")
    run_ext = expected_meta_ext(args)
    for field in META_EXT_FIELDS:
        held = (file_ext or {}).get(field, options.BY_NAME[field].default)
        if held != run_ext[field] or type(held) is not type(run_ext[field]):
            raise ValueError("training state: %s is %r in the state file and %r in this run; a state resumes only under the "
                             "options it was saved with (--load_path takes the weights alone)" % (field, held, run_ext[field]))


REWARD_NORM_KEYS = ("stats", "table", "stats_next", "table_next", "carry", "carry_next")


def check_reward_norm(state, normalize_reward):
    """`normalize_reward` is named by neither meta block (their fields are fixed), so the PRESENCE of agent["reward_norm"] says
    whether the state was saved under it: a state with the block resumes only under the flag -- its critic is in scaled
    units -- and one without it only without the flag.  ValueError otherwise."""
    agent = state.get("agent") if isinstance(state, dict) else None
    has = isinstance(agent, dict) and "reward_norm" in agent
    if has and not isinstance(agent["reward_norm"], dict):
        raise ValueError("training state: agent.reward_norm is no block")
    if has and not normalize_reward:
        raise ValueError("training state: it was saved with normalize_reward (it holds agent.reward_norm); this run is "
                         "without it: run with --normalize_reward")
    if normalize_reward and not has:
        raise ValueError("training state: it was saved without normalize_reward (it holds no agent.reward_norm); this run is "
                         "with it: run without --normalize_reward")


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
