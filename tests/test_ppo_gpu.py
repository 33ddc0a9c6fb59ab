"""GPU (-m gpu): the PPO loop end to end on the native env — shapes of log.txt (75 optimizer
steps per update), finiteness over several iterations, checkpoint wire format."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests.hip_helpers import make_args

pytestmark = pytest.mark.gpu


def _run(agent, steps):
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(steps):
            agent.run()


def test_two_iterations_stay_finite(tmp_path):
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    args = make_args(4096, save=True, save_path=str(tmp_path / "ck_"), save_freq=75)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(args)
    assert agent.mini_chunk_size == 10 and agent.rollout_size == 160      # ppo.py:120-122
    for it in range(2):
        _run(agent, agent.rollout_size)
        torch.cuda.synchronize()
        assert agent.optim_step == 75 * (it + 1)                          # log.txt:48-49
        assert torch.isfinite(agent._obs_ring).all(), "non-finite observation in the rollout"
        assert torch.isfinite(agent.all_reward).all() and torch.isfinite(agent.all_advantage).all()
        assert torch.isfinite(agent.all_log_prob).all()
        for k, p in agent.net.state_dict().items():
            assert torch.isfinite(p).all(), k
    # checkpoint: reference key names, loadable into a fresh agent (ppo.py:147-149, :266-273)
    sd = torch.load(str(tmp_path / "ck_150.pth"), weights_only=True)
    assert sorted(sd) == sorted(["shared_net.0.weight", "shared_net.0.bias", "shared_net.2.weight", "shared_net.2.bias",
                                 "to_mean.0.weight", "to_mean.0.bias", "to_mean.2.weight", "to_mean.2.bias",
                                 "to_value.0.weight", "to_value.0.bias", "to_value.2.weight", "to_value.2.bias"])
    assert sum(v.numel() for v in sd.values()) == 69587
    args2 = make_args(4096, load=True, load_path=str(tmp_path / "ck_150.pth"), testing=True)
    with contextlib.redirect_stdout(io.StringIO()):
        agent2 = PPO(args2)
    for k, p in agent2.net.state_dict().items():
        assert torch.equal(p.cpu(), sd[k].cpu())
    assert float(agent2.action_var[0]) == pytest.approx(0.01)             # ppo.py:152
    _run(agent2, 5)
    assert agent2.optim_step == 0                                         # testing: no updates (ppo.py:241)
    agent.exit(); agent2.exit()


def test_action_var_schedule_and_done_mask():
    from fly_bproject_amd.ppo import PPO
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(4096))
    _run(agent, 7)
    np.testing.assert_allclose(float(agent.action_var[0]), 0.2 - 7e-5, rtol=1e-5)   # ppo.py:237
    assert agent.all_done.shape == (4096, 1)                              # Q1: replaced by the last step's mask
    assert torch.equal(agent.all_done[:, 0], 1 - agent.env.reset_buf)
    # the default is ONE launch per rollout: the device has run all 160 steps, but what run() exposes per step are that step's
    # rows -- env.reset_buf / progress_buf (fly.py:175-177) included
    assert agent.persistent_rollout and agent.env.progress_buf.data_ptr() == agent._progress_rows[6].data_ptr()
    assert int(agent.env.progress_buf.max()) == 7 and torch.equal(agent.env.obs_buf, agent._obs_ring[7])
    assert torch.equal(agent.all_obs[1], agent.all_next_obs[0])           # ring aliasing
    agent.exit()


GEMMS = ["f32", "bf16x3"]     # both arithmetics of the MLP GEMMs are held to the reference's golden vectors at the SAME tolerance


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("n", [1, 31, 32, 33, 8192, 40960 + 7])
def test_mfma_forward_matches_torch_and_oracle(golden, n, gemm):
    """mlp_forward (fp32 MFMA, and the bf16x3 operand-split arithmetic) vs torch fp32 on the same weights; tolerance
    2e-5 rel/abs (k-order and fma chaining differ from a BLAS dot product, nothing else), and vs the reference's own
    Net.pi/.v outputs recorded in g4."""
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    g = golden("g4_net")
    net = Net(73, 18).to("cuda:0")
    net.load_state_dict({k: torch.from_numpy(g[k]) for k in g.files if "." in k})
    ref = Net(73, 18).to("cuda:0")
    ref.load_state_dict(net.state_dict())
    pol = PackedPolicy(net, "cuda:0")
    pol.gemm = gemm
    net._policy = pol
    gen = torch.Generator(device="cuda:0").manual_seed(n)
    x = torch.randn(n, 73, device="cuda:0", generator=gen) * 1.5
    with torch.no_grad():
        mu, v = net.pi(x), net.v(x)                       # MFMA path (no grad)
        mu_t, v_t = ref.to_mean(ref.shared_net(x)), ref.to_value(ref.shared_net(x))
    torch.testing.assert_close(mu, mu_t, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(v, v_t, rtol=2e-5, atol=2e-5)
    if n == 8192:
        xg = torch.from_numpy(g["x"]).to("cuda:0")
        with torch.no_grad():
            np.testing.assert_allclose(net.pi(xg).cpu().numpy(), g["pi"], rtol=2e-5, atol=2e-5)
            np.testing.assert_allclose(net.v(xg).cpu().numpy(), g["v"], rtol=2e-5, atol=2e-5)
        saves = {"out": torch.empty(n, 32, device="cuda:0"), "h1": torch.empty(n, 256, device="cuda:0"),
                 "h2": torch.empty(n, 128, device="cuda:0"), "h3": torch.empty(n, 128, device="cuda:0")}
        pol.forward(x, saves=saves)      # saves given: the UPDATE's forward arithmetic (pol.gemm)
        with torch.no_grad():
            h1 = ref.shared_net[1](ref.shared_net[0](x)); h2 = ref.shared_net(x)
            h3 = torch.cat([ref.to_mean[1](ref.to_mean[0](h2)), ref.to_value[1](ref.to_value[0](h2))], dim=1)
        from fly_bproject_amd.policy import untile          # saved tensors are in tile-fragment order
        torch.testing.assert_close(untile(saves["h1"], n, 256), h1, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(untile(saves["h2"], n, 128), h2, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(untile(saves["h3"], n, 128), h3, rtol=2e-5, atol=2e-5)
        out_rows = untile(saves["out"], n, 32)
        torch.testing.assert_close(out_rows[:, :18], mu_t, rtol=2e-5, atol=2e-5)
        assert torch.all(out_rows[:, 19:] == 0)
        # determinism
        mu2 = net.pi(x) if not torch.is_grad_enabled() else None
        with torch.no_grad():
            assert torch.equal(net.pi(x), mu)


def test_rollout_values_equal_the_critic_pass():
    """make_data with v(obs_t) captured from the rollout's policy launches == make_data with the
    reference's separate critic pass over all stored observations (ppo.py:158-159), bit for bit;
    a weight change between rollout and make_data invalidates the captured values."""
    from fly_bproject_amd.ppo import PPO
    res = {}
    for reuse in (True, False):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(4096, reuse_rollout_values=reuse, persistent_rollout=False))   # steps launched one by one below
            _run(agent, agent.rollout_size - 1)
            agent._launch_step(agent.rollout_size - 1)           # last step without the update
        assert agent._v_have == (agent.rollout_size)
        _, _, _, target, adv = agent.make_data()
        torch.cuda.synchronize()
        res[reuse] = (target.clone(), adv.clone())
        if reuse:
            with torch.no_grad():
                full = agent.net.v(agent._obs_ring)
            assert torch.equal(full, agent._v_ring)
            agent._v_have = agent.rollout_size                   # pretend the rollout is still cached ...
            agent.policy.P.mul_(1.001); agent.policy.refresh()   # ... but the weights moved
            _, _, _, t2, _ = agent.make_data()
            assert not torch.equal(t2, res[True][0])
        agent.exit()
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


def test_graph_replay_matches_eager_rollout():
    """graph=True (and persistent_rollout=True: one launch per rollout) replays the device work of a whole rollout from ONE captured hipGraph (the captured normal_
    advances the Philox offset like the eager call).  After whole rollouts everything equals the eager run bit for
    bit -- also when the score print's mid-rollout bookkeeping flush falls inside a replayed rollout (run_step 200,
    300 below).  Mid-rollout the DEVICE is ahead of the host's step count (documented in PPO.run): the rows the
    host has stepped through are final, env.reset_buf / progress_buf already hold the rollout's end state."""
    from fly_bproject_amd.ppo import PPO
    res = {}
    for graph in (False, True, "persistent"):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(4096, graph=graph is True, persistent_rollout=graph == "persistent", testing=True))
            T = agent.rollout_size
            _run(agent, 3 * T)                           # rollout 1 eager, rollout 2 captures + replays, rollout 3 replays
        torch.cuda.synchronize()
        if graph is True:
            assert len(agent._graphs) == 1
        res[graph] = (agent._obs_ring.clone(), agent.all_acts.clone(), agent.all_reward.clone(),
                      agent.all_log_prob.clone(), agent.env.progress_buf.clone(), float(agent.action_var[0]), agent._score_acc.clone())
        # rows the host has stepped through are final mid-rollout too: 7 more steps, compare those rows
        with contextlib.redirect_stdout(io.StringIO()):
            _run(agent, 7)
        torch.cuda.synchronize()
        res[graph] += (agent.all_acts[:7].clone(), agent.all_log_prob[:7].clone(), agent._obs_ring[:8].clone(),
                       float(agent.action_var[0]), agent.env.obs_buf.clone())
        agent.exit()
    for mode in (True, "persistent"):       # "persistent": ONE launch per rollout (ppo_rollout_all), env state in registers
        for i, (a, b) in enumerate(zip(res[False], res[mode])):
            if torch.is_tensor(a):
                assert torch.equal(a, b), (mode, i)
            else:
                assert a == b, (mode, i)


@pytest.mark.parametrize("n,fs", [(4096, None), (8192, None), (16384, None), (300, None), (4096, "0"), (8192, "0")])
def test_one_launch_per_rollout_in_training_mode(n, fs, monkeypatch):
    """`persistent_rollout` (ppo_rollout_all) with the variance DECAYING (training mode, 1e-5 per step) over two whole
    iterations, updates included, with the score print (and its bookkeeping flush) landing inside rollouts while the device
    has run ahead: rollout tensors, per-step reset / progress rows, action_var and every parameter equal the eager run bit for
    bit.  8192 envs = one workgroup per CU = the bench configuration (rollout_all_fs_kernel); 16384 envs walks two tiles per
    workgroup; 300 envs has a ragged last tile (rollout_all_kernel<true> with its HBM hand-offs for that tile);
    FLY_ROLLOUT_FS=0 forces rollout_all_kernel<true> (LDS hand-offs x_tile_lds / act_tile_lds, resident biases) at whole tiles."""
    from fly_bproject_amd.ppo import PPO
    if fs is not None:
        monkeypatch.setenv("FLY_ROLLOUT_FS", fs)
    res = {}
    for persistent in (False, True):
        torch.manual_seed(0)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            agent = PPO(make_args(n, persistent_rollout=persistent))
            assert agent.persistent_rollout == persistent
            T = agent.rollout_size                      # 4096 envs: 160 -- the prints at run_step 100, 200, 300 fall inside rollouts
            iters = 2 if T <= 160 else 1
            extra = 37 if T > 37 else T // 2            # steps into the next rollout: only rows the HOST has stepped through compare
            flags = []
            for i in range(iters * T + extra):
                agent.run()
                if i >= iters * T:                      # the flags run() shows for THIS step (fly.py:175-177)
                    flags.append((agent.env.reset_buf.clone(), agent.env.progress_buf.clone()))
            agent.flush_log()
        torch.cuda.synchronize()
        assert agent.optim_step == 75 * iters
        res[persistent] = (agent._obs_ring[:extra + 1].clone(), agent.all_acts[:extra].clone(), agent.all_reward[:extra].clone(),
                           agent.all_log_prob[:extra].clone(), agent._v_ring[:extra].clone(), float(agent.action_var[0]),
                           agent.policy.P.clone(), agent.policy.exp_avg_sq.clone(), agent.all_advantage.clone(),
                           [ln for ln in buf.getvalue().splitlines() if ln.startswith("Steps:")],
                           torch.stack([f[0] for f in flags]), torch.stack([f[1] for f in flags]))
        agent.exit()
    assert abs(res[False][5] - (0.2 - (iters * T + extra) * 1e-5)) < 1e-6 + 2e-9 * (iters * T + extra)    # fp32 running subtraction
    for i, (a, b) in enumerate(zip(res[False], res[True])):
        if torch.is_tensor(a):
            assert torch.equal(a, b), i
        else:
            assert a == b, (i, a, b)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("n", [33, 8192])
def test_fused_forward_sample_matches_separate_kernels(n, gemm):
    """mlp_forward_sample (policy + sampling in one launch) == mlp_forward then ppo_sample_logprob (the kernel
    tests/test_hip_parity.py pins to g5); actions also bit-exact against the oracle's restatement of ppo.py:215-220."""
    import ctypes as C
    from fly_bproject_amd import _lib
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    from oracle import oracle as O
    torch.manual_seed(n)
    net = Net(73, 18).to("cuda:0")
    pol = PackedPolicy(net, "cuda:0")
    pol.gemm = gemm
    lib = _lib.load()
    x = torch.randn(n, 73, device="cuda:0")
    eps = torch.randn(n, 18, device="cuda:0")
    var = torch.rand(18, device="cuda:0") * 0.19 + 0.01
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    mu, v1 = pol.forward(x, want_mu=True, want_v=True)
    act1 = torch.empty(n, 18, device="cuda:0"); lp1 = torch.empty(n, device="cuda:0")
    _lib.check(lib.ppo_sample_logprob(p(mu), p(var), p(eps), p(act1), p(lp1), n, None), "sample")
    act2 = torch.empty(n, 18, device="cuda:0"); lp2 = torch.empty(n, device="cuda:0"); mu2 = torch.empty(n, 18, device="cuda:0")
    v2 = torch.empty(n, device="cuda:0")
    _lib.check(lib.mlp_forward_sample(p(pol.P), p(pol.PF), p(x), n, p(eps), p(var), 0, 0.0, 0.0, p(act2), p(lp2), p(mu2), p(v2), pol.infer_pb_ptr(), None, None), "fused")
    torch.cuda.synchronize()
    assert torch.equal(mu, mu2) and torch.equal(act1, act2) and torch.equal(v1.view(-1), v2)
    torch.testing.assert_close(lp1, lp2, rtol=2e-6, atol=1e-5)
    a_o, lp_o = O.sample_logprob(mu.cpu().numpy(), var.cpu().numpy(), eps.cpu().numpy())
    assert np.array_equal(act2.cpu().numpy(), a_o)
    np.testing.assert_allclose(lp2.cpu().numpy(), lp_o, rtol=2e-6, atol=1e-5)


@pytest.mark.parametrize("gemm", GEMMS)
@pytest.mark.parametrize("tag", ["v02", "v001", "vmix"])
def test_fused_forward_sample_vs_reference_goldens(golden, gemm, tag):
    """The fused policy + sampling launch against the reference's OWN outputs: g4's weights and observations give g4's
    Net.pi (ppo.py:30), g5's recorded eps / variance then give action = clip(pi + sqrt(var) eps) and its log-prob
    (ppo.py:215-220) -- evaluated here in float64 numpy from the golden pi, compared at the suite's 2e-5."""
    import ctypes as C
    from fly_bproject_amd import _lib
    from fly_bproject_amd.policy import PackedPolicy
    from fly_bproject_amd.ppo import Net
    g4, g5 = golden("g4_net"), golden("g5_sample")
    net = Net(73, 18).to("cuda:0")
    net.load_state_dict({k: torch.from_numpy(g4[k]) for k in g4.files if "." in k})
    pol = PackedPolicy(net, "cuda:0")
    pol.gemm = gemm
    x = torch.from_numpy(g4["x"]).to("cuda:0")
    n = x.shape[0]
    eps, var = torch.from_numpy(g5[tag + "_eps"]).to("cuda:0"), torch.from_numpy(g5[tag + "_var"]).to("cuda:0")
    act = torch.empty(n, 18, device="cuda:0"); lp = torch.empty(n, device="cuda:0"); mu = torch.empty(n, 18, device="cuda:0")
    v = torch.empty(n, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    _lib.check(_lib.load().mlp_forward_sample(p(pol.P), p(pol.PF), p(x), n, p(eps), p(var), 0, 0.0, 0.0, p(act), p(lp), p(mu),
                                              p(v), pol.infer_pb_ptr(), None, None), "fused")
    torch.cuda.synchronize()
    np.testing.assert_allclose(mu.cpu().numpy(), g4["pi"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(v.cpu().numpy(), g4["v"][:, 0], rtol=2e-5, atol=2e-5)
    L = np.sqrt(g5[tag + "_var"].astype(np.float64))
    a64 = g4["pi"].astype(np.float64) + L * g5[tag + "_eps"].astype(np.float64)
    np.testing.assert_allclose(act.cpu().numpy(), np.clip(a64, -1, 1), rtol=2e-5, atol=2e-5)
    # the log-prob is of the UNCLIPPED sample: -0.5 (18 log 2pi + |eps|^2) - sum log L  (mu cancels)
    lp64 = -0.5 * (18 * np.log(2 * np.pi) + (g5[tag + "_eps"].astype(np.float64) ** 2).sum(1)) - np.log(L).sum()
    np.testing.assert_allclose(lp.cpu().numpy(), lp64, rtol=2e-5, atol=2e-5)


def test_trainer_entry_point(tmp_path, capsys):
    """trainer.py (reference trainer.py:1-50): bounded run, final save under the reference's key names."""
    import trainer
    policy = trainer.main(["--num_envs", "4096", "--headless", "True", "--max_steps", "165",
                           "--save_path", str(tmp_path / "final_"), "--save_freq", "1000000"])
    out = capsys.readouterr().out
    assert "mini_chunk_size:  10" in out and "rollout_size:  160" in out and "Training" in out
    assert "Steps: 0100 | Opt Step: 0000" in out                      # the reference's log line format
    assert policy.optim_step == 75 and policy.run_step == 165
    sd = torch.load(str(tmp_path / "final_.pth"), weights_only=True)  # policy.save() at exit (trainer.py:48)
    assert "to_mean.2.weight" in sd and sd["shared_net.0.weight"].shape == (256, 73)


def test_reference_default_env_count():
    """trainer.py's default --num_envs 1000: rows per minibatch (40 000) and per step (1000) are not
    multiples of the kernels' 16/32-row tiles; one full iteration stays finite and counts 75 steps."""
    from fly_bproject_amd.ppo import PPO
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = PPO(make_args(1000))
    assert agent.mini_chunk_size == 40 and agent.rollout_size == 640
    _run(agent, agent.rollout_size)
    torch.cuda.synchronize()
    assert agent.optim_step == 75
    assert torch.isfinite(agent._obs_ring).all() and torch.isfinite(agent.policy.P).all()
    assert torch.all(agent.policy.W1[:, 73:] == 0)
    agent.exit()


def test_rollout_bookkeeping_equals_per_step_calls():
    """ppo_rollout_bookkeeping over a block of rows == ppo_step_bookkeeping row by row, bit for bit
    (score terms added in row order, variance decayed once per row, clamp included) -- also at env counts
    that are no multiple of 4, where every other row starts off a 16-byte boundary, and below one float4."""
    import ctypes as C
    from fly_bproject_amd import _lib
    lib = _lib.load()
    torch.manual_seed(5)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    for n in (8192, 4099, 5):
        rows = 37
        reward = torch.randn(rows, n, device="cuda:0")
        for dec, v0 in ((1e-5, 0.2), (1e-3, 0.02), (0.0, 0.2)):
            s1 = torch.full((), 0.25, device="cuda:0"); v1 = torch.full((18,), v0, device="cuda:0")
            for r in range(rows):
                _lib.check(lib.ppo_step_bookkeeping(p(reward[r]), n, p(s1), C.c_float(0.01), p(v1), 18, C.c_float(dec),
                                                    C.c_float(0.01), None), "step")
            s2 = torch.full((), 0.25, device="cuda:0"); v2 = torch.full((18,), v0, device="cuda:0")
            terms = torch.zeros(rows, device="cuda:0")
            applied = torch.full((1,), 5, dtype=torch.int32, device="cuda:0")
            _lib.check(lib.ppo_rollout_bookkeeping(p(reward), rows, n, p(terms), p(s2), C.c_float(0.01), p(v2), 18,
                                                   C.c_float(dec), C.c_float(0.01), p(applied), None), "rollout")
            torch.cuda.synchronize()
            assert torch.equal(s1, s2) and torch.equal(v1, v2)
            assert int(applied) == 5 + rows                      # the word the policy launches subtract from their row index
        assert float(v2[0]) == float(np.float32(0.2))            # dec = 0: untouched


@pytest.mark.parametrize("n", [33, 8192])
def test_bf16x3_forward_is_fp32_accurate(n):
    """The bf16x3 GEMM path (three-term bf16 split of both operands, six MFMA terms, fp32 accumulate)
    against an fp64 evaluation of the same network: its error must stay within the fp32 tolerance of
    this suite (2e-5) and within 2x of the error of the fp32-MFMA path on the same inputs."""
    from fly_bproject_amd.policy import PackedPolicy, untile
    from fly_bproject_amd.ppo import Net
    torch.manual_seed(n + 1)
    net = Net(73, 18).to("cuda:0")
    pol = PackedPolicy(net, "cuda:0")
    pol.init_training(n)
    x = torch.randn(n, 73, device="cuda:0") * 2.0
    ref = Net(73, 18).to("cuda:0").double()
    ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
    with torch.no_grad():
        t = ref.shared_net(x.double())
        mu64, v64 = ref.to_mean(t), ref.to_value(t)
        h1_64 = torch.nn.functional.elu(ref.shared_net[0](x.double()))
    err = {}
    for mode in ("f32", "bf16x3"):
        pol.gemm = mode
        with torch.no_grad():
            mu, v = pol.forward(x, saves=pol.saves)
        torch.cuda.synchronize()
        err[mode] = (float((mu.double() - mu64).abs().max()), float((v.double() - v64).abs().max()),
                     float((untile(pol.saves["h1"], n, 256).double() - h1_64).abs().max()))
        assert torch.isfinite(mu).all() and torch.isfinite(v).all()
    for a, b in zip(err["bf16x3"], err["f32"]):
        assert a <= 2e-5 and a <= 2.0 * b + 1e-7, err


@pytest.mark.parametrize("n", [4096, 1000])
def test_one_launch_rollout_step_equals_two_launches(n):
    """ppo_rollout_step (policy + sampling + env step of each 32-env tile in one launch) leaves bit for
    bit what mlp_forward_sample followed by fly_step leave, over a whole rollout plus the next one
    (1000 envs: the trainer's default, a ragged last tile)."""
    from fly_bproject_amd.ppo import PPO
    res = {}
    for fuse in (True, False):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(n, testing=True, persistent_rollout=False))     # one launch per STEP is what is compared here
            agent.run()
            assert agent.fuse_rollout_step
            agent.fuse_rollout_step = fuse
            _run(agent, agent.rollout_size + 6)
        torch.cuda.synchronize()
        res[fuse] = (agent._obs_ring.clone(), agent.all_acts.clone(), agent.all_reward.clone(), agent.all_log_prob.clone(),
                     agent._v_ring.clone(), agent.env.progress_buf.clone(), agent.env.reset_buf.clone(),
                     agent.env.root_tensor.clone(), agent.env.dof_states.clone())
        agent.exit()
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


def test_asynchronous_log_queue_writes_the_same_lines_in_the_same_order():
    """The score line (ppo.py:257-260) read asynchronously and written when its values have arrived (the default) against
    read-and-print-at-once (`async_log=False`): the same stdout, line for line -- 'Training' and the score lines in the reference's
    order --, and the same parameters after two updates; nothing is pending once flush_log() has returned, and a line queued by the
    LAST run() call is not lost."""
    from fly_bproject_amd.ppo import PPO
    res = {}
    for async_log in (False, True):
        torch.manual_seed(0)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            agent = PPO(make_args(4096, async_log=async_log))
            assert agent._async_log == async_log
            T = agent.rollout_size                      # 160: score lines at run_step 0, 100, 200, 300 -- two of them inside rollouts
            for _ in range(2 * T - 20 + 1):             # ends ON run_step 300: its line is queued by the last call
                agent.run()
            agent.flush_log()
            assert not agent._log_q
        torch.cuda.synchronize()
        lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Steps:") or ln == "Training"]
        res[async_log] = (lines, agent.policy.P.clone(), agent.optim_step)
        agent.exit()
    assert res[True][0] == res[False][0] and len(res[True][0]) == 5 and res[True][0].count("Training") == 1
    assert res[True][0][-1].startswith("Steps: 0300 | Opt Step: 0075")
    assert res[True][2] == res[False][2] == 75 and torch.equal(res[True][1], res[False][1])


def test_log_throughput_flag_extends_the_score_line_only_when_asked():
    """`log_throughput` (trainer.py --log_throughput): every score line (ppo.py:257-260) gets ' | Env-steps/s <rate>' appended
    (the first one 'n/a': no earlier line to measure from); without the flag stdout is the reference's text.  Same training."""
    import re
    from fly_bproject_amd.ppo import PPO
    res = {}
    for flag in (False, True):
        torch.manual_seed(0)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            agent = PPO(make_args(2048, log_throughput=flag))
            for _ in range(agent.rollout_size + 5):
                agent.run()
            agent.flush_log()
        torch.cuda.synchronize()
        res[flag] = ([ln for ln in buf.getvalue().splitlines() if ln.startswith("Steps:")], agent.policy.P.clone())
        agent.exit()
    plain, timed = res[False][0], res[True][0]
    assert len(plain) == len(timed) >= 3
    assert all("Env-steps/s" not in ln for ln in plain)
    assert timed[0].endswith(" | Env-steps/s n/a")
    for a, b in zip(plain, timed):
        assert b.startswith(a + " | Env-steps/s ")
    rates = [float(re.search(r"Env-steps/s ([0-9.e+]+)$", ln).group(1)) for ln in timed[1:]]
    assert all(r > 1e5 for r in rates), rates
    assert torch.equal(res[False][1], res[True][1])


@pytest.mark.parametrize("n", [8192, 16384])
def test_one_launch_rollout_is_deterministic_run_to_run(n):
    """`ppo_rollout_all` twice on identical inputs (same seed -> same weights, same reset state, same eps): every row it writes --
    observations, actions, log-probs, values, rewards, per-step reset / progress flags -- must be bit-equal run to run, over a WHOLE
    rollout and the first steps of the next one (after an update: changed weights).  8192 envs = rollout_all_fs_kernel<false, false>
    at one tile per CU (T = 80), 16384 = its persistent-over-tiles instantiation (T = 32).  The kernel runs the fused step's chain
    GEMMs as inline-asm MFMAs (policy_tile_fs): an operand hazard there shows as run-to-run differences in the last bits INSIDE every
    parity tolerance -- the defect class round 4's b6e3caf fixed in the DQN kernel, which only a determinism test can see
    (tools/check_mfma_hazard.py is the static half of this check)."""
    from fly_bproject_amd.ppo import PPO
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            agent = PPO(make_args(n))
            assert agent.persistent_rollout and agent.policy.gemm_infer == "bf16x3"
            T = agent.rollout_size
            assert T == 16 * (40960 // n)
            for _ in range(T):
                agent.run()
            torch.cuda.synchronize()
            first = [t.clone() for t in (agent._obs_ring, agent.all_acts, agent.all_log_prob, agent._v_ring[:T], agent.all_reward,
                                         agent._reset_rows, agent._progress_rows)]
            assert agent.optim_step == 75
            for _ in range(T // 2):                         # into the next rollout: the launch has run all T steps on the NEW weights
                agent.run()
            torch.cuda.synchronize()
            second = [t.clone() for t in (agent._obs_ring, agent.all_acts, agent.all_log_prob, agent._v_ring[:T], agent.all_reward,
                                          agent._reset_rows, agent._progress_rows, agent.policy.P)]
        runs.append(first + second)
        agent.exit()
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.isfinite(a.float()).all(), i
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))
    assert int(runs[0][5].sum()) > 0                        # episodes ended inside the rollout: the reset path ran too


def test_checked_binding_launches_what_the_raw_call_launches():
    """ppo_td_gae through `_lib.api()` with tensors and plain numbers, and through the raw function with explicit ctypes
    wrappers: bitwise the same targets and advantages.  T = 3 carries the recurrence, N = 65 leaves a ragged last block."""
    import ctypes as C
    from fly_bproject_amd import _lib
    lib, api, p = _lib.load(), _lib.api(), _lib.ptr
    T, N = 3, 65
    g = torch.Generator(device="cuda").manual_seed(11)
    reward, v, v_next = (torch.randn((T, N), device="cuda", generator=g) for _ in range(3))
    done = (torch.rand(N, device="cuda", generator=g) > 0.25).float()
    out = [torch.full((T, N), float("nan"), device="cuda") for _ in range(4)]
    api.ppo_td_gae(reward, v, v_next, done, 0.99, 0.95, T, N, out[0], out[1], 0, _lib.stream_ptr())
    _lib.check(lib.ppo_td_gae(p(reward), p(v), p(v_next), p(done), C.c_float(0.99), C.c_float(0.95), C.c_int64(T), C.c_int64(N),
                              p(out[2]), p(out[3]), C.c_int(0), _lib.stream_ptr()), "ppo_td_gae")
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and float(out[1].abs().max()) > 0
    assert torch.equal(out[0].view(torch.int32), out[2].view(torch.int32)), "targets differ"
    assert torch.equal(out[1].view(torch.int32), out[3].view(torch.int32)), "advantages differ"
