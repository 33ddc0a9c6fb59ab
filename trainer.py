"""Entry point, the reference's trainer.py (trainer.py:1-50) on the MI355X-native Fly/PPO.

Same flags (`--sim_device --compute_device_id --graphics_device_id --num_envs --headless --save
--save_path --save_freq --load --load_path --record --record_dir_name
--time_steps_per_recorded_frame --testing`), same seeding and the same run loop.  Additions:
`--rl_device` (accepted alias; the reference uses sim_device for both), `--variant`
(bigGrav = fly.py, lowGrav = flyLowGrav.py), `--reward` (standing | walking), `--max_steps`
(bounded runs; the reference loops until the viewer's E key), `--seed` and `--log_throughput` (env-steps/s on the score line).
`--normalize_obs` (running mean / std normalisation of the policy input, rl_games' normalize_input; off by default) with
`--obs_clip` (the bound of a normalised input, default 5.0): the statistics are saved with the checkpoint as obs_rms.* and
loaded with it; such a checkpoint needs `--normalize_obs` to load.
`--normalize_value` (running mean / std normalisation of the critic's regression targets; off by default): the critic's
outputs are mapped back to reward units wherever they meet rewards; the statistics are saved with the checkpoint as
value_rms.* and loaded with it; such a checkpoint needs `--normalize_value` to load.
`--lambda_returns` (the critic regresses on the lambda-return A_t + V(s_t) of the advantage estimator in use, DESIGN.md 3.3g;
off by default: the reference's one-step TD target r + gamma v(s')).  The policy's advantages are untouched; with
`--normalize_value` the running statistics are those of the lambda-returns.  Meant for `--gae episodic`: the reference
estimator's quirks pass through, and its done mask makes whole columns of lambda-returns strongly negative.  One seed of
evidence (profiles/lambda_returns_curve.txt): under the reference's hyper-parameters it does not train the standing task.
Nothing of it goes into the weights file;
`--save_state` records the option, and a state resumes only under the value it was saved with.
`--episode_stats` (return and length of the episodes that finished; off by default): the score line also
carries ` | Episodes n | Return mean [min, max] | Length mean | Timeouts pct%` over the episodes closed since the previous
score line, every step of an episode counted, the one that performs the reset too.  It observes and steers nothing: weights
and rollouts are the same bits with and without it.  `--save_state` carries the open episodes and the totals, and a state
saved with or without the flag resumes with or without it.
`--normalize_reward` (the GAE pass reads rewards divided by the running standard deviation of the discounted return, DESIGN.md
3.3i; off by default) with `--reward_clip` (the bound of a scaled reward, default 10.0).  Score line, `--episode_stats` and the
recorder keep the raw rewards.  The statistics are saved with the checkpoint as reward_rms.* and loaded with it; such a
checkpoint needs `--normalize_reward` to load, and a `--save_state` state resumes only under the flag it was saved with.
`--update_stats` (PPO update diagnostics; off by default): behind every finished update one forward of the
updated network over all rows of the rollout and one reduction; the score line also carries
` | KL k3 | Clip pct% | EV ev | Loss loss` over the updates since the previous score line (` | KL n/a` without one, as under
`--testing`; ` | Nonfinite n` when rows were non-finite).  The explained variance is that of the UPDATED critic on the targets
it just regressed on (SB3 prints the pre-update critic's: this number one update later).  It observes and steers nothing;
`--save_state` carries the sets, and a state saved with or without the flag resumes with or without it.
`--gae episodic` (episode-aware advantage estimate with time-limit bootstrapping; the default `reference` is
the reference's estimator with its quirks).
`--minibatch shuffled` (every epoch draws its 15 minibatches from a fresh permutation of ALL rows of the rollout, DESIGN.md
3.3e; the default `reference` is the reference's 15 contiguous-in-time slices, the same in every epoch, the 16th chunk never
visited) with `--minibatch_seed` (default `--seed`; rank r adds r * 0x9E3779B9).  The permutation is a pure function of the seed,
the count of updates and the epoch: nothing of it goes into the weights file; `--save_state` carries the count.
`--action_noise ar1` (temporally correlated exploration noise, DESIGN.md 3.2b: the rollout's noise is an AR(1) process along
time with unit stationary variance and lag-1 correlation `--noise_rho`, default 0.5; the default `white` is the reference's
independent draw at every step).  Each step's noise is still N(0, 1), so the stored log-probs stay the densities of the actions.
The process runs on from rollout to rollout and is not restarted at episode ends; nothing of it goes into the weights file;
`--save_state` carries it.
`--randomize` (per-env physics domain randomisation, off by default): each env runs on its own multipliers of kp, kd, effort,
mass (and inertia), mu and gravity, drawn from `--dr_<name> LO HI` at every reset of that env with seed `--dr_seed` (default
`--seed`; rank r adds r * 0x9E3779B9).  A property of the env: nothing of it goes into the weights file; `--save_state` carries it.
`--save_state` (with `--save_path`) and `--resume_path FILE` (exact resume).  The weights file stays the
reference's; with `--save_state` every save made at a rollout boundary (all periodic ones) also writes, on EVERY rank,
`<save_path><suffix>.state.r<rank>.pth`: Adam's moments and counter, the fp16x2 scales and planes, the step counts and the
action variance, the generator, the env's state and episode statistics, the normalisation statistics, the noise carry, the
minibatch update count and the randomisation table.  `--resume_path FILE` names a weights file of such a run: the weights load
as `--load_path` loads them, each rank's state comes from the file beside it, and the run goes on bit for bit as if it had
never stopped -- under exactly the options it was saved with (any difference is an error naming the option; `--load_path`
takes the weights alone).  A save inside a rollout (the end-of-run save after a `--max_steps` that is no multiple of the
rollout) writes the weights only and says so.  Not restored: the recorder's frame numbering; `--resume_path` excludes
`--load_path` and `--testing`.
Recording (`--record True` or `--record_dir_name DIR`): rank 0 renders env 0 on the GPU every
`--time_steps_per_recorded_frame` env steps to DIR/frame_%06d.png (fly_bproject_amd/record.py) and, when ffmpeg is on
PATH, assembles DIR.mp4 at the end.  Unlike the reference, which records only with its viewer open, recording does not
depend on `--headless`: this build has no viewer.
Multi-GPU: launch with `python -m torch.distributed.run --nproc-per-node N trainer.py ...`;
each rank owns `--num_envs` envs on its own GPU.
"""
import argparse
import random

import torch


def parse_args(argv=None):
    from fly_bproject_amd import options as O
    parser = argparse.ArgumentParser()

    def flag(name, **kw):
        """--<name>, its default and choices from the one table of options."""
        opt = O.BY_NAME[name]
        if opt.choices:
            kw['choices'] = list(opt.choices)
        if kw.get('action') != 'store_true':
            default = O.flag_default(name)
            kw['default'] = list(default) if isinstance(default, tuple) else default
        parser.add_argument('--' + name, **kw)

    flag('sim_device', type=str, help='Physics Device in PyTorch-like syntax')
    flag('rl_device', type=str, help='accepted for compatibility; sim_device is used')
    flag('compute_device_id', type=int)
    flag('graphics_device_id', type=int, help='Graphics Device ID')
    flag('num_envs', type=int)
    flag('headless')
    flag('save', type=bool)
    flag('save_path', type=str)
    flag('save_freq', type=int)
    flag('load', type=bool)
    flag('load_path', type=str)
    flag('record', type=bool)
    flag('record_dir_name', type=str)
    flag('time_steps_per_recorded_frame', type=int)
    flag('testing', type=bool)
    flag('variant', type=str)
    flag('reward', type=str)
    flag('max_steps', type=int, help='stop after this many env steps (0 = run until env.end)')
    flag('seed', type=int)
    flag('gemm', type=str,
         help='arithmetic of the MLP GEMMs: f16x2 (default) = bf16x3 for the rollout policy and the critic pass, the '
              'optimizer-step gradient in the two-term fp16 split with three product terms and per-class '
              'power-of-two scales (DESIGN.md 3.4c; a step whose values do not fit fp16 is refused on the device '
              'and redone in bf16x3); bf16x3 = fp32 operands split exactly into three bf16 terms on the bf16 matrix '
              'pipe, fp32 accumulate, for EVERY GEMM (DESIGN.md 3.4); f32 = v_mfma_f32_32x32x2_f32.  All are held to '
              'the reference goldens at the fp32 tolerances.  Default: $FLY_GEMM or f16x2')
    flag('log_throughput', action='store_true',
         help='append env-steps/s (all ranks, host clock, since the previous score line) to the score line '
              '(ppo.py:257-260 prints the score only; off by default so that stdout stays the reference\'s)')
    flag('dp_mode', type=str,
         help='multi-GPU: all-reduce the gradient every optimizer step (reference algorithm on the global '
              'batch) or average parameters once per PPO update (non-parity)')
    flag('normalize_advantage', action='store_true',
         help='normalise advantages over the rollout (not in the reference; off by default)')
    flag('normalize_obs', action='store_true',
         help='normalise the policy input by running mean / std of the observations, clamped to +-obs_clip '
              '(rl_games normalize_input; not in the reference; off by default)')
    flag('normalize_value', action='store_true',
         help='the critic regresses on TD targets normalised by their running mean / std, and its outputs are '
              'mapped back to reward units for the TD target and GAE (rl_games normalize_value, without its clamp; '
              'not in the reference; off by default)')
    flag('lambda_returns', action='store_true',
         help='the critic regresses on the lambda-return A_t + V(s_t) (the GAE advantage, before any normalisation, plus the '
              'critic\'s own value in reward units: rl_games / SB3 / cleanrl `returns`) instead of the one-step TD target '
              'r + gamma v(s\') of ppo.py:160; with --normalize_value the running statistics are those of the lambda-returns.  '
              'NOT the reference\'s critic target; off by default.  Meant for --gae episodic (the reference estimator\'s '
              'done-mask quirk passes through and is amplified); on one seed it did not train the standing task under the '
              'reference\'s hyper-parameters (DESIGN.md 3.3g)')
    flag('episode_stats', action='store_true',
         help='the score line also carries the count, mean / min / max return, mean length and time-out share of the '
              'episodes that finished since the previous score line (every step of an episode counts, the one that '
              'performs the reset too: rl_games current_rewards); one kernel over the reward and flag rows at the end of a '
              'rollout, no host sync; changes nothing the rollout or the update reads (DESIGN.md 3.3h); off by default')
    flag('update_stats', action='store_true',
         help='the score line also carries the approximate KL (Schulman k3), the clip fraction, the explained variance of the '
              'updated critic on its targets and the loss over all rows of the rollout, from one forward of the updated network '
              'and one reduction behind every update; no host sync; changes nothing the rollout or the update reads '
              '(DESIGN.md 3.3j); off by default')
    flag('normalize_reward', action='store_true',
         help='the GAE pass reads rewards divided by the running standard deviation of the discounted return, clamped to '
              '+-reward_clip (gymnasium NormalizeReward, SB3 VecNormalize(norm_reward=True); no mean-centring).  The score '
              'line, --episode_stats and the recorder keep the raw rewards; the critic then lives in scaled units, so the '
              'statistics are saved with the checkpoint as reward_rms.* (DESIGN.md 3.3i; not in the reference; off by default)')
    flag('reward_clip', type=float, help='bound of a scaled reward under --normalize_reward, > 0')
    flag('gae', type=str,
         help='advantage estimator: reference = ppo.py:157-171 as it stands (the done mask of the last step over the '
              'whole rollout, no reset of the recurrence at episode ends); episodic = per-step end flags, the '
              'recurrence stops at every episode end, time-outs bootstrap from the value of the next observation '
              '(rl_games value_bootstrap / time_outs) and the step that performs a reset trains nothing.  episodic '
              'is NOT the reference\'s estimator; off by default')
    flag('minibatch', type=str,
         help='minibatches of the update: reference = ppo.py:173-202 as it stands (15 contiguous-in-time slices of the '
              'rollout, the same in every epoch; the 16th chunk trains nothing); shuffled = every epoch cuts its 15 '
              'minibatches from a fresh keyed permutation of all rows of the rollout (still 75 optimizer steps per '
              'update; each epoch leaves a random sixteenth out).  shuffled is NOT the reference\'s update; off by default')
    flag('minibatch_seed', type=int, help='seed of the minibatch permutations (default: --seed)')
    flag('action_noise', type=str,
         help='exploration noise of the rollout: white = ppo.py:215-220 as it stands (an independent N(0, 1) draw per '
              'step and joint); ar1 = the draws of a rollout are filtered along time into an AR(1) process with unit '
              'stationary variance (each step still N(0, 1), corr(t, t + k) = rho^k; continuous across rollouts, not '
              'restarted at episode ends).  ar1 is NOT the reference\'s sampling; off by default')
    flag('noise_rho', type=float,
         help='lag-1 correlation of --action_noise ar1, 0 < rho < 1 (0.5: between white and pink noise, a starting '
              'choice, not a measurement)')
    flag('obs_clip', type=float, help='bound of a normalised observation (with --normalize_obs)')
    flag('randomize', action='store_true',
         help='per-env physics domain randomisation, redrawn at every reset of the env (Isaac Gym actor-property '
              'randomisation; not in the reference; off by default)')
    for name in O.DR_NAMES:
        flag('dr_' + name, type=float, nargs=2, metavar=('LO', 'HI'),
             help='range of the %s multiplier (with --randomize; mass scales the inertia too)' % name)
    flag('dr_seed', type=int, help='seed of the randomisation draws (default: --seed)')
    flag('save_state', action='store_true',
         help='with --save_path: every save at a rollout boundary also writes <save_path><suffix>.state.r<rank>.pth, '
              'the full training state of each rank, for --resume_path (off by default: the weights file alone)')
    flag('resume_path', type=str,
         help='a weights file written by a --save_state run: continue that run bit for bit from it and the state '
              'files beside it, under the same options (excludes --load_path and --testing)')
    args = parser.parse_args(argv)
    if args.save_path is not None:          # trainer.py:27-34
        args.save = True
    if args.load_path is not None:
        args.load = True
    if args.record_dir_name is not None:
        args.record = True
    args.resume = args.resume_path is not None
    if args.resume and args.load:
        parser.error("--resume_path and --load_path exclude each other (--resume_path names the weights file too)")
    if args.resume and args.testing:
        parser.error("--resume_path continues a training run: it has no meaning with --testing")
    if args.save_state and args.save_path is None:
        parser.error("--save_state needs --save_path")
    return args


def main(argv=None):
    args = parse_args(argv)
    from fly_bproject_amd.dist import broadcast_policy, init_from_env
    from fly_bproject_amd.ppo import PPO

    rank, local_rank, world = init_from_env("cuda")
    args.rank, args.world_size = rank, world
    if world > 1:
        args.sim_device = "cuda:%d" % local_rank
    torch.manual_seed(args.seed)            # trainer.py:24-25
    random.seed(args.seed)
    if args.testing:
        print("## Careful you are in testing mode, no Training will take place ##")
    policy = PPO(args)                      # trainer.py:39
    if args.gemm:
        policy.policy.gemm = args.gemm
    broadcast_policy(policy)
    if args.resume:
        policy.load_training_state()        # last: the two calls above rebuild planes and clear the fp16x2 calibration
    end = False                             # trainer.py:41-44
    while not end:
        end = policy.run()
        if args.max_steps and policy.run_step >= args.max_steps:
            end = True
    policy.save()                           # trainer.py:48-50
    policy.generate_video()
    policy.exit()
    return policy


if __name__ == '__main__':
    main()
