"""GPU (-m gpu): a constructed agent stands on the resolved record (fly_bproject_amd/options.py).  Construction only, no
rollout: every public option attribute of the agent is the record's field, and the meta block the live agent reports is the
one train_state.expected_meta predicts from the args before an env exists."""
import os

import pytest

from fly_bproject_amd import options, train_state
from tests.hip_helpers import make_args
from tests.test_resume_gpu import OPT_IN

pytestmark = pytest.mark.gpu

# the agent's attribute -> the record's field, where the names differ
RENAMED = {"use_graph": "graph", "_async_log": "async_log", "_loaded": "load"}
ATTRIBUTES = ("gae", "minibatch", "action_noise", "noise_rho", "normalize_obs", "obs_clip", "normalize_value",
              "normalize_advantage", "reuse_rollout_values", "log_throughput", "update_backend", "world_size", "dp_mode",
              "dp_allreduce", "mini_chunk_size", "rollout_size", "persistent_rollout", "use_graph", "_async_log", "_loaded")


@pytest.mark.parametrize("kw", [{}, OPT_IN], ids=["defaults", "all_opt_in"])
def test_a_constructed_agent_holds_the_record(monkeypatch, kw):
    from fly_bproject_amd.ppo import PPO
    for o in options.OPTIONS:
        if o.env:
            monkeypatch.delenv(o.env, raising=False)
    args = make_args(4096, **kw)
    record = options.resolve(args, os.environ)
    agent = PPO(args)
    try:
        assert agent.options == record
        for name in ATTRIBUTES:
            got, want = getattr(agent, name), getattr(record, RENAMED.get(name, name))
            assert got == want and type(got) is type(want), name
        assert (agent.mini_batch_size, agent.chuck_number) == (options.MINI_BATCH_SIZE, options.CHUNK_NUMBER)
        assert (agent.policy.gemm, agent.policy.step_gemm) == (record.gemm, record.step_gemm)
        assert agent.env.randomized == record.randomize and (agent.env.recorder is not None) == record.record
        if record.minibatch == "shuffled":
            assert agent._mb_seed == record.minibatch_seed
        else:
            assert not hasattr(agent, "_mb_seed")
        agent.gae = agent.gae                               # plain, assignable attributes
        assert agent._training_state_meta() == train_state.expected_meta(args)
    finally:
        agent.exit()
