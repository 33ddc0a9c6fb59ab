"""`Fly`: the reference's vectorised environment class (fly.py:11-681), MI355X-native.

Same constructor argument (`args` with `.sim_device`, `.num_envs`, `.headless`, ...), same public
attributes (`num_obs`, `num_act`, `obs_buf`, `reward_buf`, `reset_buf`, `progress_buf`, `end`,
`root_tensor`, `dof_states`, `dof_pos`, `dof_vel`, `force_tensor`, `potentials`, ...) and methods
(`step`, `reset`, `get_obs`, `get_reward`, `simulate`, `render`, `generate_video`, `exit`).  What
was a chain of torch ops plus Isaac Gym calls per step is ONE kernel launch through the C ABI
(`fly_step`, include/flyhip.h); the unfused methods launch the matching single-phase kernels.
With `args.record`, rank 0 records env 0 (record.py).  With `args.randomize`, every env runs FlyDyn on its own
multiplied constants, redrawn at each of its resets (`set_randomization`).

No Isaac Gym, no PhysX, no CPU path: the rigid-body model behind `simulate()` is the
build-defined FlyDyn because the reference's physics is a closed binary.
"""
import ctypes as C
import math

import torch

from . import _lib
from .options import DR_DEFAULT_RANGES, DR_NAMES, dr_args, resolve_env  # noqa: F401  (the randomisation's names live there)
from .params import NUM_CONTACT, NUM_DOF, NUM_OBS, ROOT_DIM, default_params


def dr_bounds(ranges):
    """{name: (lo, hi)} -> (lo[6], hi[6]) as fp32, a missing name = (1, 1).  The ABI's rules, checked here first so that bad
    input fails before any GPU call: finite bounds, lo > 0, lo <= hi (after rounding to fp32)."""
    unknown = set(ranges) - set(DR_NAMES)
    if unknown:
        raise ValueError("unknown randomisation parameter(s) %s; expected some of %s" % (sorted(unknown), list(DR_NAMES)))
    lo, hi = [], []
    for name in DR_NAMES:
        pair = ranges.get(name, (1.0, 1.0))
        if len(pair) != 2:
            raise ValueError("randomisation range of %s must be (lo, hi), got %r" % (name, pair))
        a, b = (C.c_float(float(v)).value for v in pair)
        if not (math.isfinite(a) and math.isfinite(b)):
            raise ValueError("randomisation range of %s is not finite: %r" % (name, pair))
        if not a > 0.0:
            raise ValueError("randomisation lower bound of %s must be > 0, got %r" % (name, pair[0]))
        if a > b:
            raise ValueError("randomisation range of %s is not ordered: %r > %r" % (name, pair[0], pair[1]))
        lo.append(a)
        hi.append(b)
    return lo, hi


class Fly:
    def __init__(self, args, params=None):
        self.args = args
        opts = resolve_env(args)
        self.end = False                                  # fly.py:15
        self.up_axis_idx = 2
        n = opts.num_envs
        self.params = params if params is not None else default_params(n, opts.variant, opts.reward)
        if self.params.num_envs != n:
            raise ValueError("params.num_envs (%d) != args.num_envs (%d)" % (self.params.num_envs, n))
        self.dt = float(self.params.dt)                   # fly.py:16
        self.num_act = NUM_DOF                            # fly.py:31
        self.num_obs = 19 + 3 * self.num_act              # fly.py:32
        self.max_episode_length = int(self.params.max_episode_length)
        self.render_count = 0

        self.device = torch.device(args.sim_device)
        if self.device.type != "cuda":
            raise _lib.FlyHipError(
                "Fly runs on an MI355X (sim_device=%r). This build has no CPU path; the CPU restatement "
                "under oracle/ is test infrastructure only." % (args.sim_device,))
        if not torch.cuda.is_available():
            raise _lib.FlyHipError("no GPU visible: Fly needs an MI355X")
        self._lib = _lib.load()
        torch.cuda.set_device(self.device)
        self._handle = C.c_void_p()
        _lib.api().fly_create(C.byref(self.params), C.byref(self._handle))

        dev = self.device
        f32 = dict(dtype=torch.float32, device=dev)
        # fly.py:169-179
        self.obs_buf = torch.zeros((n, NUM_OBS), **f32)
        self.reward_buf = torch.zeros(n, **f32)
        self.reset_buf = torch.ones(n, device=dev, dtype=torch.long)
        self.progress_buf = torch.zeros(n, device=dev, dtype=torch.long)
        # fly.py:378-395, :89-100 (shapes and aliasing views as Isaac Gym exposed them)
        self.root_tensor = torch.zeros((n, ROOT_DIM), **f32)
        self.dof_states = torch.zeros((n, NUM_DOF * 2), **f32)
        self.force_tensor = torch.zeros((n * NUM_CONTACT, 3), **f32)
        self.num_dof = NUM_DOF
        self.dof_pos = self.dof_states.view(n, NUM_DOF, 2)[..., 0]
        self.dof_vel = self.dof_states.view(n, NUM_DOF, 2)[..., 1]
        self.root_positions = self.root_tensor[:, 0:3]
        self.root_orientations = self.root_tensor[:, 3:7]
        self.root_linvels = self.root_tensor[:, 7:10]
        self.root_angvels = self.root_tensor[:, 10:13]
        # fly.py:636: the scaled actions, [N*18, 1] (allocated up front; upstream creates it in the first step)
        self.actions = torch.zeros((n * NUM_DOF, 1), **f32)
        # fly.py:121-135
        self.potentials = torch.full((n,), -1000.0 / self.dt, **f32)
        self.prev_potentials = self.potentials.clone()
        self.targets = torch.tensor(list(self.params.target), **f32).repeat((n, 1))
        self.dof_limits_lower = torch.tensor(list(self.params.dof_lo), **f32)
        self.dof_limits_upper = torch.tensor(list(self.params.dof_hi), **f32)
        base = torch.arange(n, device=dev, dtype=torch.long).view(n, 1) * NUM_CONTACT
        self.index_abdomen_sim = (base + torch.arange(0, 5, device=dev)).reshape(-1)     # fly.py:311-314
        self.index_legs_tip = (base + torch.arange(5, 11, device=dev)).reshape(-1)
        # episode statistics kept by the step kernel (not in the reference): running return/length of
        # the current episode and per-env totals over finished ones
        self.episode_return_buf = torch.zeros(n, **f32)
        self.episode_length_buf = torch.zeros(n, **f32)
        self.finished_return_sum = torch.zeros(n, **f32)
        self.finished_length_sum = torch.zeros(n, **f32)
        self.finished_count = torch.zeros(n, **f32)
        self._bufs = _lib.FlyBuffers()
        self._refresh_pointers()
        # per-env physics domain randomisation (opt-in): the [N, FLY_DR_ROW] table the kernels read and redraw; kept once made,
        # so turning randomisation off and on again continues each env's draw count
        self._dr_table = None
        self._dr_on = False
        # bumped whenever the kernels a launch selects change (randomisation on / off): captured graphs hold the old ones
        self.launch_form = 0
        if opts.randomize:
            self.set_randomization(dict(zip(DR_NAMES, opts.dr_ranges)), opts.dr_seed)
        # recording (fly.py:592-610): env 0, rank 0 only (record.py)
        self.recorder = None
        if opts.record:
            from .record import Recorder
            self.recorder = Recorder(self, opts.record_dir_name, opts.time_steps_per_recorded_frame)

    # ------------------------------------------------------------------------------------------
    def _refresh_pointers(self):
        b = self._bufs
        b.root, b.dof_state = self.root_tensor.data_ptr(), self.dof_states.data_ptr()
        b.targets, b.contact = self.actions.data_ptr(), self.force_tensor.data_ptr()
        b.pot, b.prev_pot = self.potentials.data_ptr(), self.prev_potentials.data_ptr()
        b.obs, b.reward = self.obs_buf.data_ptr(), self.reward_buf.data_ptr()
        b.reset, b.progress = self.reset_buf.data_ptr(), self.progress_buf.data_ptr()
        b.ep_return, b.ep_length = self.episode_return_buf.data_ptr(), self.episode_length_buf.data_ptr()
        b.done_return, b.done_length = self.finished_return_sum.data_ptr(), self.finished_length_sum.data_ptr()
        b.done_count = self.finished_count.data_ptr()

    def bind_obs(self, rows):
        """Make `rows` (f32 [N,73], contiguous) the observation buffer: the
        step kernel then writes observation rows straight into the caller's rollout storage."""
        if rows.shape != self.obs_buf.shape or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise ValueError("bind_obs needs a contiguous f32 [%d,%d] tensor" % tuple(self.obs_buf.shape))
        if rows.device != self.obs_buf.device:
            raise ValueError("bind_obs: rows live on %s, env on %s" % (rows.device, self.obs_buf.device))
        self.obs_buf = rows
        self._bufs.obs = rows.data_ptr()

    def bind_reward(self, row):
        """Make `row` (f32 [N], contiguous) the reward buffer (a row of the caller's rollout)."""
        if row.numel() != self.reward_buf.numel() or row.dtype != torch.float32 or not row.is_contiguous():
            raise ValueError("bind_reward needs a contiguous f32 tensor of %d elements" % self.reward_buf.numel())
        if row.device != self.reward_buf.device:
            raise ValueError("bind_reward: wrong device")
        self.reward_buf = row.view(-1)
        self._bufs.reward = row.data_ptr()

    def _check_actions(self, actions):
        n = self.args.num_envs
        if actions.shape != (n, NUM_DOF) or actions.dtype != torch.float32 or actions.device != self.device:
            raise ValueError("actions must be f32 [%d,%d] on %s" % (n, NUM_DOF, self.device))
        return actions if actions.is_contiguous() else actions.contiguous()

    # ------------------------------------------------------------------------------------------
    def set_randomization(self, ranges, seed=0):
        """Per-env physics domain randomisation.  `ranges`: {name: (lo, hi)} over DR_NAMES, multipliers of the config's kp, kd,
        effort, mass (and inertia), mu and gravity; a missing name is (1, 1).  Turning it on draws every env's multipliers once;
        every reset the kernels perform then draws that env's next set.  `None` turns it off: the plain kernels run again and
        the table is left as it is."""
        if ranges is None:
            _lib.api().fly_set_randomization(self._handle, None, None, _lib.stream_ptr())
            self._dr_on = False
            self.launch_form += 1
            return
        lo, hi = dr_bounds(ranges)
        if self._dr_table is None:
            self._dr_table = torch.zeros((self.args.num_envs, _lib.DR_ROW), dtype=torch.float32, device=self.device)
        r = _lib.FlyRandomization()
        r.lo[:], r.hi[:] = lo, hi
        r.seed = int(seed) % (1 << 32)
        _lib.api().fly_set_randomization(self._handle, C.byref(r), self._dr_table, _lib.stream_ptr())
        self._dr_on = True
        self.launch_form += 1

    @property
    def randomized(self):
        return self._dr_on

    @property
    def env_params(self):
        """[N, 6] float32 view of each env's current multipliers (DR_NAMES order), or None when randomisation is off."""
        return self._dr_table[:, :_lib.DR_PARAMS] if self._dr_on else None

    @property
    def env_param_draws(self):
        """[N] int32 view of each env's draw count (None if randomisation was never on)."""
        return None if self._dr_table is None else self._dr_table[:, _lib.DR_PARAMS].view(torch.int32)

    # ---- exact resume (train_state.py) ------------------------------------------
    # every tensor FlyBuffers points at except obs and reward, which are rows of the caller's rollout
    _STATE_TENSORS = ("root_tensor", "dof_states", "actions", "force_tensor", "potentials", "prev_potentials", "reset_buf",
                      "progress_buf", "episode_return_buf", "episode_length_buf", "finished_return_sum", "finished_length_sum",
                      "finished_count")

    def training_state(self):
        """The env's state between two steps, tensors on the CPU: the simulation state, the CURRENT reset / progress flags
        (`reset_buf` / `progress_buf` may be rows of the caller's per-step flag tensors: their values are what counts), the
        episode statistics, the step count, and with randomisation the whole table (multipliers and draw counts).  The
        recorder is not part of it.  A host sync."""
        from .train_state import pack
        state = {k: pack(getattr(self, k)) for k in self._STATE_TENSORS}
        state["render_count"] = int(self.render_count)
        if self._dr_on:
            state["dr_table"] = pack(self._dr_table)
        return state

    def load_training_state(self, state):
        """training_state() back, in place: the flags go into whatever `reset_buf` / `progress_buf` are now (the env's own
        tensors in a new process), the table into the one the handle already points at, over the constructor's first draw."""
        from .train_state import restore, value
        for k in self._STATE_TENSORS:
            restore(getattr(self, k), state, "env", k)
        self.render_count = value(state, "env", "render_count", int)
        if self._dr_on:
            restore(self._dr_table, state, "env", "dr_table")

    def step(self, actions):
        """fly.py:624-681 in one launch."""
        a = self._check_actions(actions)
        rec = self.recorder
        row = rec.next_ring_row() if rec is not None else 0
        _lib.api().fly_step(self._handle, a, C.byref(self._bufs), _lib.stream_ptr())
        if rec is not None:
            rec.capture(row)
            rec.reached(row, self.render_count)
        self.render_count += 1

    def set_actions(self, actions):
        """fly.py:626-657 alone: scale to joint ranges and hand the targets to the sim."""
        a = self._check_actions(actions)
        _lib.api().fly_scale_actions(self._handle, a, self.actions, _lib.stream_ptr())

    def reset(self):
        """fly.py:446-480.  Returns whether any env was flagged (one host sync, as upstream)."""
        any_flag = bool(self.reset_buf.any().item())
        if not any_flag:
            return False
        _lib.api().fly_reset_masked(self._handle, C.byref(self._bufs), _lib.stream_ptr())
        return True

    def reset_async(self):
        """fly.py:446-480 without the host sync of the boolean return value."""
        _lib.api().fly_reset_masked(self._handle, C.byref(self._bufs), _lib.stream_ptr())

    def simulate(self):
        """fly.py:482-485."""
        _lib.api().fly_integrate(self._handle, C.byref(self._bufs), _lib.stream_ptr())

    def get_obs(self):
        """fly.py:397-411."""
        _lib.api().fly_pack_obs(self._handle, C.byref(self._bufs), _lib.stream_ptr())

    def get_reward(self):
        """fly.py:413-443."""
        _lib.api().fly_pack_reward(self._handle, C.byref(self._bufs), 0, _lib.stream_ptr())

    compute_observations = get_obs      # names used by BASELINE.json's north_star
    compute_reward = get_reward

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _quat_rotate(q, v):
        qw = q[:, 3:4]
        qv = q[:, :3]
        a = v * (2.0 * qw ** 2 - 1.0)
        b = torch.cross(qv, v, dim=-1) * qw * 2.0
        c = qv * (qv * v).sum(-1, keepdim=True) * 2.0
        return a + b + c

    @property
    def up_vec(self):
        """fly.py:405 output of compute_heading_and_up, derived on demand."""
        z = torch.tensor([0.0, 0.0, 1.0], device=self.device).expand(self.args.num_envs, 3)
        return self._quat_rotate(self.root_orientations, z)

    @property
    def heading_vec(self):
        x = torch.tensor([1.0, 0.0, 0.0], device=self.device).expand(self.args.num_envs, 3)
        return self._quat_rotate(self.root_orientations, x)

    def episode_stats(self, reset=False):
        """(mean return, mean length, count) over the episodes finished since the last reset of the
        statistics.  One host sync; call it when logging, not per step."""
        cnt = float(self.finished_count.sum().item())
        if cnt == 0:
            out = (float("nan"), float("nan"), 0)
        else:
            out = (float(self.finished_return_sum.sum().item()) / cnt, float(self.finished_length_sum.sum().item()) / cnt, int(cnt))
        if reset:
            self.finished_return_sum.zero_(); self.finished_length_sum.zero_(); self.finished_count.zero_()
        return out

    def reward_terms(self):
        """The per-term reward dump behind the reference viewer's P key (fly.py:504-546), as a dict
        of [N] tensors computed from the current buffers (diagnostics; not on the hot path)."""
        n, p = self.args.num_envs, self.params
        obs = self.obs_buf
        acts = self.actions.view(n, -1)
        hw, uw = float(p.heading_weight), float(p.up_weight)
        heading = torch.where(obs[:, 11] > 0.8, torch.full_like(obs[:, 11], hw), hw * obs[:, 11] / 0.8)
        up = torch.where(obs[:, 0] > 1.4, torch.full_like(heading, uw), torch.zeros_like(heading))      # fly.py:512-513
        q = self.root_orientations
        orient = torch.where(q[:, 2] ** 2 + q[:, 3] ** 2 > 0.92, torch.full_like(up, uw), torch.zeros_like(up))   # fly.py:518
        start = 12 + 2 * self.num_act
        stored = obs[:, start:start + self.num_act]
        elec = (acts - stored).abs().sum(-1)
        lim = ((stored > self.dof_limits_upper * 0.9).sum(-1) + (stored < self.dof_limits_lower * 0.9).sum(-1))
        legs = (self.force_tensor[self.index_legs_tip].sum(1).view(n, -1) > 0).long().sum(1) * 0.1
        return {"heading_reward": heading, "alive_reward": torch.full_like(heading, 0.5), "up_reward": up,
                "orient_reward": orient, "actions_cost": (acts ** 2).sum(-1), "electricity_cost": elec,
                "dof_at_limit_cost": lim * float(p.joints_at_limit_cost_scale),
                "progress_reward": self.potentials - self.prev_potentials, "leg_reward": legs}

    def render(self):
        """fly.py:487-562: there is no viewer in this build.  Not recording: None.  Recording: the recorded view of env 0's
        current state, uint8 [H, W, 3] (one synchronous fly_render)."""
        if self.recorder is None:
            return None
        return self.recorder.render_now()

    def generate_video(self):
        """fly.py:592-610: finish the recorded frames (record.py); an .mp4 when ffmpeg is on PATH."""
        if self.recorder is not None:
            return self.recorder.generate_video()
        return None

    def exit(self):
        """fly.py:617-621."""
        if self.recorder is not None:
            self.recorder.close()
        if self._handle:
            torch.cuda.synchronize(self.device)
            _lib.api().fly_destroy(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            if getattr(self, "_handle", None):
                self._lib.fly_destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass
