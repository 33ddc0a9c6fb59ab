"""GPU (-m gpu): PPO.make_data and update()'s commits with the opt-in features composed, over THREE iterations, against an
independent reference of the whole chain (tests/make_data_ref.py; the capture and the checks are tests/make_data_capture.py).

Per iteration k = 0, 1, 2 of every case:
  (a) every stage equals its float32 reference applied to the agent's own inputs of that stage, bit for bit in the lane forms
      (the scan forms of `all_300` within the existing scan bounds; statistics within the existing statistics bounds);
  (b) every named output equals chain64 -- fed iteration k's raw rows and ITS OWN state from iteration k - 1, never the
      agent's -- within 4 x the chain32-against-chain64 figure of that output on these same rows;
  (c) what update() commits is what make_data left in the scratch set, bit for bit, and what the chain commits;
  (d) optimizer steps 0, 14, 15 and 74 of updates 0 and 2 are fed minibatch_ref.gather_ref of what make_data returned (the
      slices update() documents with contiguous minibatches), bit for bit;
  (e) the rollouts are not tame: an episode ends in the last row of a rollout that has a successor and one in the first row of
      a rollout that has a predecessor, open episodes cross every boundary, some env never falls and some do, the committed value table is not the identity, the reward factor is off 1 by more than 10 %, and at most 1 % of
      the scaled rewards sit at the clip.
(a) isolates a kernel, (b) the wiring between them.  The worst error / bar per output is printed; the figures of the run
that made this test are in profiles/make_data_chain_error.txt."""
import numpy as np
import pytest

from tests import make_data_capture as K

pytestmark = pytest.mark.gpu

ALL = dict(normalize_obs=True, normalize_value=True, normalize_reward=True, lambda_returns=True, normalize_advantage=True,
           gae="episodic", minibatch="shuffled", action_noise="ar1", randomize=True, episode_stats=True, update_stats=True)
CASES = {
    "all_4096": (4096, 160, ALL),                                            # the lane kernels, one launch per rollout
    "all_4096_stepwise": (4096, 160, dict(ALL, persistent_rollout=False)),
    # PPO_GAE_SCAN forms, a ragged last tile of 12 envs.  Three rollouts are 6528 steps here, about 180 episodes per env, and at
    # the default termination height (1.1) every one of the 300 envs falls in one of them (measured: 18769 falls): no env
    # "never falls".  At 0.8 falls are rare (measured: 322 in 54307 episode ends) and 109 envs never fall.
    "all_300": (300, 2176, ALL, dict(termination_height=0.8)),
    "ref_gae_4096": (4096, 160, dict(gae="reference", normalize_reward=True, normalize_value=True, lambda_returns=True,
                                     normalize_advantage=True)),             # the reference estimator's vnorm path
    "no_vnorm_4096": (4096, 160, dict(normalize_reward=True, lambda_returns=True, gae="episodic",
                                      normalize_advantage=True)),            # lambda-targets without a table
}


@pytest.mark.parametrize("case", list(CASES))
def test_three_iterations_against_the_chain(case):
    n, T, kw = CASES[case][:3]
    info, its = K.run_agent(n, 3, env_params=CASES[case][3] if len(CASES[case]) > 3 else None, **kw)
    assert (info["T"], info["N"]) == (T, n) and info["persistent"] == kw.get("persistent_rollout", True)
    assert info["scan"] == (case == "all_300") and info["reward_clip"] == 10.0
    K.check_coverage(info, its)
    seeds = dict(minibatch_seeds=[info["mb_seed"]], minibatch_rows=info["mb_rows"])
    c64, c32 = K.chain_pair(info, **seeds)
    outs64, outs32, states = [], [], []
    for it in its:
        outs64.append(c64.step(it["raw"]))
        outs32.append(c32.step(it["raw"]))
        c64.commit()
        c32.commit()
        states.append(c64.state())
        # the reference alone stays inside the clip too
        assert (np.abs(outs64[-1]["reward_scaled"]) >= info["reward_clip"]).mean() <= 0.01
    worst = K.check_rank(info, its, outs64, outs32, states)
    print("make_data chain %s: worst error / bar per output: %s"
          % (case, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0
