"""ctypes binding of libflyhip.so (include/flyhip.h, and include/flyhip_ext.h and include/flyhip_update_stats.h for what was added
after its prototype list was fixed).  Fails loudly: no library, no product."""
import ctypes as C
import os

from .params import FlyParams

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLYHIP_LIB") or os.path.join(_HERE, "libflyhip.so")
_lib = None
_api = None
_ext = None
_update_stats = None


class FlyHipError(RuntimeError):
    pass


class FlyBuffers(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("root", "dof_state", "targets", "contact", "pot", "prev_pot",
                                          "obs", "reward", "reset", "progress", "ep_return", "ep_length",
                                          "done_return", "done_length", "done_count")]


class FlyRenderConfig(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fov_y_deg", C.c_float), ("cam_offset", C.c_float * 3),
                ("look_z", C.c_float)]


class FlyRandomization(C.Structure):
    _fields_ = [("lo", C.c_float * 6), ("hi", C.c_float * 6), ("seed", C.c_uint32), ("reserved", C.c_int32)]


POSE_FLOATS = 25        # FLY_POSE_FLOATS: root pos xyz | quat xyzw | 18 joint angles
OBS_NORM_SET = 147      # FLY_OBS_NORM_SET / FLY_OBS_NORM_TABLE: count | mean[73] | var or M2[73] (f64); m[73] | r[73] | clip (f32)
OBS_NORM_SETS = 256     # FLY_OBS_NORM_SETS: moment sets one ppo_obs_norm_pass writes
VALUE_NORM_SET = 3      # FLY_VALUE_NORM_SET: count | mean | var or M2 (f64)
VALUE_NORM_TABLE = 4    # FLY_VALUE_NORM_TABLE: m | s | r | 0 (f32)
VALUE_NORM_SETS = 256   # FLY_VALUE_NORM_SETS: moment sets one ppo_td_gae_vnorm writes
EPISODE_SET = 10        # FLY_EPISODE_SET: n | ret_mean | ret_M2 | ret_min | ret_max | len_sum | len_min | len_max | timeouts | rows (f64)
EPISODE_SETS = 256      # FLY_EPISODE_SETS: sets one ppo_episode_stats writes
UPDATE_STATS_SET = 17   # FLY_UPDATE_STATS_SET: one set of update statistics (f64), include/flyhip_update_stats.h has the table
UPDATE_STATS_SETS = 256 # FLY_UPDATE_STATS_SETS: sets one ppo_update_stats writes
DR_PARAMS = 6           # FLY_DR_PARAMS: kp, kd, effort, mass (+ inertia), mu, gravity multipliers
DR_ROW = 8              # FLY_DR_ROW: a randomisation table row, f32 m[6] | draw count (int32 bits) | 0
ABI_VERSION = 13        # include/flyhip.h as this package binds it (fly_abi_version(): argument lists changed between versions)
# name -> argtypes; every entry point returns int except fly_last_error
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SYMBOLS = {
    "fly_abi_version": [],
    "fly_create": [C.POINTER(FlyParams), C.POINTER(_P)],
    "fly_destroy": [_P],
    "fly_step": [_P, _P, C.POINTER(FlyBuffers), _P],
    "fly_scale_actions": [_P, _P, _P, _P],
    "fly_reset_masked": [_P, C.POINTER(FlyBuffers), _P],
    "fly_integrate": [_P, C.POINTER(FlyBuffers), _P],
    "fly_pack_obs": [_P, C.POINTER(FlyBuffers), _P],
    "fly_pack_reward": [_P, C.POINTER(FlyBuffers), _I, _P],
    "fly_set_pose_record": [_P, _P],
    "fly_set_obs_norm": [_P, _P],
    "fly_set_randomization": [_P, C.POINTER(FlyRandomization), _P, _P],
    "fly_render": [_P, _P, _I, C.POINTER(FlyRenderConfig), _P, _P, _P],
    "ppo_sample_logprob": [_P, _P, _P, _P, _P, _L, _P],
    "ppo_td_gae": [_P, _P, _P, _P, _F, _F, _L, _L, _P, _P, _I, _P],
    "ppo_adv_stats": [_P, _L, _P, _P],
    "ppo_adv_apply": [_P, _L, _P, _F, _F, _P],
    "ppo_obs_norm_pass": [_P, _L, _L, _P, _P, _P, _P],
    "ppo_obs_norm_merge": [_P, _P, _P, _L, _F, _P],
    "ppo_td_gae_vnorm": [_P, _P, _P, _P, _P, _F, _F, _L, _L, _P, _P, _P, _I, _P],
    "ppo_value_norm_merge": [_P, _P, _L, _P, _P, _P],
    "ppo_value_norm_apply": [_P, _L, _P, _P, _P],
    "ppo_lambda_targets": [_P, _P, _P, _L, _P, _P, _P],
    "ppo_td_gae_episodic": [_P, _P, _P, _P, _P, _P, _L, _F, _F, _L, _L, _P, _P, _I, _P],
    "ppo_td_gae_episodic_vnorm": [_P, _P, _P, _P, _P, _P, _L, _P, _F, _F, _L, _L, _P, _P, _P, _I, _P],
    "ppo_episode_stats": [_P, _P, _P, _L, _L, _L, _P, _P, _P, _I, _P],
    "ppo_episode_stats_merge": [_P, _L, _P, _P, _P],
    "ppo_minibatch_gather": [_P] * 5 + [_L, C.c_uint32, C.c_uint32, _L, _L] + [_P] * 6 + [_P],
    "ppo_noise_ar1": [_P, _P, _L, _L, _F, _P],
    "ppo_step_bookkeeping": [_P, _L, _P, _F, _P, _I, _F, _F, _P],
    "ppo_rollout_step": [_P, C.POINTER(FlyBuffers), _P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _P, _P, _P],
    "ppo_rollout_all": [_P, C.POINTER(FlyBuffers), _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P],
    "ppo_rollout_bookkeeping": [_P, _L, _L, _P, _P, _F, _P, _I, _F, _F, _P, _P],
    "mlp_forward": [_P, _P, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P],
    "mlp_forward_sample": [_P, _P, _P, _L, _P, _P, _I, _F, _F, _P, _P, _P, _P, _P, _P, _P],
    "mlp_grad_workspace_floats": [],
    "mlp_backward_dx": [_P] * 10 + [_L, _F, _F, _P, _P, _P, _P, _P, _P, _P],
    "mlp_forward_backward": [_P] * 4 + [_L] + [_P] * 9 + [_F, _F] + [_P] * 6 + [_I, _P, _P, _P, _I, _P],
    "mlp_grad_w": [_P] * 8 + [_L, _P, _P, _P, _P, _P, _P, _I, _P],
    "mlp_fused_workspace_floats": [],
    "mlp_fused_grad": [_P] * 3 + [_P, _L] + [_P] * 5 + [_F, _F] + [_P] * 6 + [C.POINTER(_P), _P],
    "mlp_fused_h2_workspace_floats": [],
    "mlp_fused_grad_h2": [_P] * 5 + [_I, _P, _L] + [_P] * 5 + [_F, _F] + [_P] * 6 + [C.POINTER(_P), _P],
    "mlp_h2_rescale": [_P] * 7,
    "mlp_adam_step": [_P] * 10 + [_F, _F, _F, _F, _F, _F, _P, _I, _P, _P, _P, _P, _P, _P] + [_P] * 3 + [_I, _P],
    "dqn_eps_greedy": [_P, _P, _P, _F, _I, _P, _L, _P],
    "dqn_huber_td": [_P, _P, _P, _P, _P, _F, _I, _L, _P, _P, _P],
    "dqn_forward": [_P, _P, _P, _L, _P, _P],
    "dqn_act": [_P, _P, _P, _L, _P, _P, _F, _P, _P, _P],
    "dqn_td_step": [_P] * 10 + [_L, _F, _F] + [_P] * 7,
    "dqn_grad_workspace_floats": [],
    "dqn_grad_w": [_P] * 6 + [_L, _P, _P, _I, _P],
    "dqn_fused_workspace_floats": [],
    "dqn_fused_image_halves": [_L],
    "dqn_fused_update": [_P] * 6 + [_I, _L, _F, _F, _P, _P, _P, _P, _I, _P],
    "dqn_fused_h2_workspace_floats": [],
    "dqn_fused_h2_image_halves": [_L],
    "dqn_fused_update_h2": [_P] * 10 + [_I, _L, _F, _F, _P, _P, _P, _P, _I, _I, _P],
    "dqn_adam_soft_update": [_P] * 12 + [_F, _F, _F, _F, _F, _P, _P, _P, _P, _P, _P, _P],
    "dp_p2p_alloc": [_L, C.POINTER(_P)],
    "dp_p2p_free": [_P],
    "dp_ipc_export": [_P, _P],
    "dp_ipc_import": [_P, C.POINTER(_P)],
    "dp_ipc_close": [_P],
    "dp_allreduce_p2p": [_P, _L, C.POINTER(_P), _I, _I, C.c_uint32, _P, _L, _P],
}
# include/flyhip_ext.h: the entry points added since flyhip.h's prototype list was fixed -- a table and a binding object of
# their own (ext()), so that SYMBOLS and api() stay the statement of flyhip.h
SYMBOLS_EXT = {
    "ppo_reward_returns": [_P, _P, _F, _L, _L, _P, _P, _P, _I, _P],
    "ppo_reward_scale": [_P, _L, _P, _F, _P, _P],
}
# include/flyhip_update_stats.h: the update diagnostics (PPO --update_stats), bound the same way on update_stats_api()
SYMBOLS_UPDATE_STATS = {
    "ppo_update_stats": [_P, _P, _P, _P, _P, _P, _P, _F, _L, _P, _P],
    "ppo_update_stats_merge": [_P, _L, _P, _P, _P, _P],
}


def build(verbose=False):
    """Compile libflyhip.so in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    import subprocess
    cmd = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


def load():
    global _lib, _api, _ext, _update_stats
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FlyHipError(
            "libflyhip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C fly_bproject_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.fly_last_error.restype = C.c_char_p
    lib.fly_last_error.argtypes = []
    for name, argtypes in list(SYMBOLS.items()) + list(SYMBOLS_EXT.items()) + list(SYMBOLS_UPDATE_STATS.items()):
        fn = getattr(lib, name)          # AttributeError if the library lacks a declared symbol
        fn.argtypes = argtypes
        fn.restype = C.c_int64 if name.endswith(("_workspace_floats", "_image_halves")) else C.c_int
    if lib.fly_abi_version() != ABI_VERSION:
        raise FlyHipError("stale libflyhip.so (ABI %d, this package was written for %d): rebuild it "
                          "(`make -C fly_bproject_amd/csrc`)" % (lib.fly_abi_version(), ABI_VERSION))
    _api = _Api()
    for name in SYMBOLS:
        setattr(_api, name, _checked(name, getattr(lib, name), lib.fly_last_error))
    _ext = _Api()
    for name in SYMBOLS_EXT:
        setattr(_ext, name, _checked(name, getattr(lib, name), lib.fly_last_error))
    _update_stats = _Api()
    for name in SYMBOLS_UPDATE_STATS:
        setattr(_update_stats, name, _checked(name, getattr(lib, name), lib.fly_last_error))
    _lib = lib
    return lib


class _Api:
    """One checked callable per SYMBOLS entry (api()), per SYMBOLS_EXT entry (ext()) or per SYMBOLS_UPDATE_STATS entry
    (update_stats_api())."""


def _checked(name, fn, last_error):
    """`fn` as the product calls it: an argument with a `data_ptr` method (a tensor) goes as that address, everything else as
    ctypes takes it under fn.argtypes (None, Python numbers, ctypes instances, byref(...), c_void_p arrays).  An int entry point
    returns None or raises FlyHipError under its own name; a size query (int64_t) and fly_abi_version return their value."""
    if fn.restype is not C.c_int or name == "fly_abi_version":      # a value, not a status (and no pointer among the arguments)
        return fn
    nargs = len(fn.argtypes)
    slots = tuple(i for i, t in enumerate(fn.argtypes) if t is C.c_void_p)   # where a tensor can stand: decided once, here

    def call(*args):
        if len(args) != nargs:
            raise TypeError("%s takes %d arguments (%d given)" % (name, nargs, len(args)))
        args = list(args)
        for i in slots:
            data_ptr = getattr(args[i], "data_ptr", None)
            if data_ptr is not None:
                args[i] = data_ptr()
        rc = fn(*args)
        if rc != 0:
            msg = last_error()
            raise FlyHipError("%s failed (%d): %s" % (name, rc, msg.decode() if msg else "?"))
    call.__name__ = call.__qualname__ = name
    return call


def api():
    """The checked binding: api().f(...) is lib.f(...) with tensors passed as they are and the return code checked.  The stream
    stays the caller's explicit last argument."""
    if _api is None:
        load()
    return _api


def ext():
    """api() for the entry points of include/flyhip_ext.h (SYMBOLS_EXT): the same checked callables, on an object of their own."""
    if _ext is None:
        load()
    return _ext


def update_stats_api():
    """api() for the entry points of include/flyhip_update_stats.h (SYMBOLS_UPDATE_STATS), on an object of their own."""
    if _update_stats is None:
        load()
    return _update_stats


def check(rc, what):
    if rc != 0:
        msg = load().fly_last_error()
        raise FlyHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """The device address of a tensor, as the C ABI takes it."""
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
