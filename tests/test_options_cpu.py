"""The one table of a run's options and its resolver (fly_bproject_amd/options.py), no GPU: the defaults of trainer.py and of
a sparse namespace agree, choices are enforced by argparse and by the resolver, every bad value is refused before an env
exists, the environment variables are read at resolve time, the derived values are their definitions, and
train_state.expected_meta is a projection of the record."""
import dataclasses
import os
import types

import pytest

from fly_bproject_amd import options, train_state
from tests.test_resume_cpu import FULL, _args as resume_args

ENV_VARS = ("FLY_PERSISTENT_ROLLOUT", "FLY_ASYNC_LOG", "FLY_DP_ALLREDUCE", "FLY_GEMM", "FLY_STEP_GEMM")


@pytest.fixture(autouse=True)
def clean_environment(monkeypatch):
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)


def ns(**kw):
    return types.SimpleNamespace(**dict(dict(num_envs=1000), **kw))


def resolve(**kw):
    return options.resolve(ns(**kw), os.environ)


def test_the_table_names_the_five_environment_variables():
    assert sorted(o.env for o in options.OPTIONS if o.env) == sorted(ENV_VARS)
    assert (options.MINI_BATCH_SIZE, options.CHUNK_NUMBER, options.MAX_PERSISTENT_ROLLOUT) == (40960, 16, 4096)


def test_defaults_agree():
    import trainer
    a, b = options.resolve(trainer.parse_args([]), os.environ), resolve()
    for f in dataclasses.fields(a):
        assert getattr(a, f.name) == getattr(b, f.name), f.name
        assert type(getattr(a, f.name)) is type(getattr(b, f.name)), f.name
    assert a == b
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.gae = "episodic"
    # every flag of the parser is an entry of the table, with the table's default (None where a variable comes first)
    for name, value in vars(trainer.parse_args([])).items():
        want = options.flag_default(name)
        assert value == (list(want) if isinstance(want, tuple) else want), name


WITH_CHOICES = [o.name for o in options.OPTIONS if o.choices]


def test_the_options_with_choices():
    assert sorted(WITH_CHOICES) == ["action_noise", "dp_allreduce", "dp_mode", "gae", "gemm", "minibatch", "reward", "variant"]


@pytest.mark.parametrize("name", WITH_CHOICES)
def test_choices_are_enforced_in_both_places(name, capsys):
    import trainer
    if name != "dp_allreduce":                              # (the one option with choices and no flag)
        with pytest.raises(SystemExit):
            trainer.parse_args(["--" + name, "no_such_value"])
        assert name in capsys.readouterr().err
    with pytest.raises(ValueError, match=name):
        resolve(**{name: "no_such_value"})
    for good in options.BY_NAME[name].choices:
        resolve(**{name: good})
        if name != "dp_allreduce":
            assert getattr(trainer.parse_args(["--" + name, good]), name) == good


# the checks of section "validation", in their order: (args, what the message must hold)
BAD = [
    (dict(gae="lambda"), r"gae must be reference or episodic \(got 'lambda'\)"),
    (dict(minibatch="random"), r"minibatch must be reference or shuffled \(got 'random'\)"),
    (dict(action_noise="pink"), r"action_noise must be white or ar1 \(got 'pink'\)"),
    (dict(noise_rho=1.0), r"noise_rho must be in \(0, 1\) \(got 1.0\)"),
    (dict(noise_rho=float("nan"), action_noise="ar1"), r"noise_rho must be in \(0, 1\)"),
    (dict(resume=True, load=True, resume_path="x.pth"), "resume and load exclude each other"),
    (dict(resume=True, testing=True, resume_path="x.pth"), "resume continues a training run: it has no meaning with testing"),
    (dict(resume=True), "resume needs resume_path"),
    (dict(num_envs=40961), r"num_envs=40961 gives mini_chunk_size 0 \(ppo.py:120\); use num_envs <= 40960"),
    (dict(normalize_obs=True, obs_clip=0.0), r"obs_clip must be > 0 \(got 0.0\)"),
    (dict(normalize_obs=True, obs_clip=-1.0), "obs_clip must be > 0"),
    (dict(normalize_obs=True, obs_clip=float("nan")), "obs_clip must be > 0"),
    (dict(dp_mode="ring"), "dp_mode must be grad_allreduce or param_average"),
    (dict(dp_allreduce="mpi"), "dp_allreduce must be rccl, p2p or auto"),
]
GOOD = [dict(), dict(gae="episodic", minibatch="shuffled", action_noise="ar1", noise_rho=0.9),
        dict(normalize_obs=True, obs_clip=0.5), dict(obs_clip=0.0),            # (the clip means nothing without normalize_obs)
        dict(dp_mode="param_average", dp_allreduce="auto"), dict(num_envs=40960), dict(num_envs=16)]


def test_validation_comes_before_the_env(monkeypatch):
    from fly_bproject_amd import ppo

    def no_env(args):
        raise AssertionError("the env was built before the argument was validated")

    monkeypatch.setattr(ppo, "Fly", no_env)
    for kw, message in BAD:
        with pytest.raises(ValueError, match=message):
            ppo.PPO(ns(**kw))
    for kw in GOOD:
        with pytest.raises(AssertionError, match="before the argument"):     # a good value gets as far as the env
            ppo.PPO(ns(**kw))


def test_the_order_of_the_checks():
    """Each bad value in front of all the later ones: the earlier check is the one that raises."""
    firsts = [BAD[i] for i in (0, 1, 2, 3, 7, 8, 9, 12, 13)]
    for i, (kw, message) in enumerate(firsts):
        later = {}
        for other, _ in reversed(firsts[i + 1:]):
            later.update(other)
        with pytest.raises(ValueError, match=message):
            resolve(**dict(later, **kw))


def test_environment_variables_are_read_at_resolve_time(monkeypatch):
    base = resolve()
    assert (base.persistent_rollout, base.async_log, base.dp_allreduce, base.gemm, base.step_gemm) == \
        (True, True, "rccl", "bf16x3", "f16x2")
    cases = [("FLY_PERSISTENT_ROLLOUT", "0", dict(persistent_rollout=False), dict(persistent_rollout=True)),
             ("FLY_ASYNC_LOG", "0", dict(async_log=False), dict(async_log=True)),
             ("FLY_DP_ALLREDUCE", "p2p", dict(dp_allreduce="p2p"), dict(dp_allreduce="auto")),
             ("FLY_GEMM", "f32", dict(gemm="f32", step_gemm="f32"), dict(gemm="bf16x3")),
             ("FLY_STEP_GEMM", "bf16x3", dict(step_gemm="bf16x3"), dict(gemm="f16x2"))]
    for var, value, changed, explicit in cases:
        with monkeypatch.context() as m:
            m.setenv(var, value)
            assert resolve() == dataclasses.replace(base, **changed), var          # exactly its field(s)
            got = resolve(**explicit)                                               # an explicit arg wins
            want = dict(explicit, **({"gemm": "bf16x3", "step_gemm": "f16x2"} if explicit.get("gemm") == "f16x2" else
                                     {"step_gemm": "bf16x3"} if "gemm" in explicit else {}))
            assert got == dataclasses.replace(base, **want), var
        assert resolve() == base                                                    # and nothing is cached
    monkeypatch.setenv("FLY_GEMM", "f16x2")
    assert resolve() == base


def test_resolve_gemm_is_the_rule_of_the_policy_and_the_trainer():
    """(gemm, step_gemm) as PackedPolicy starts and as `policy.gemm = --gemm` leaves them, over every combination."""
    R = options.resolve_gemm
    assert R(None, {}) == ("bf16x3", "f16x2")
    assert R(None, {"FLY_GEMM": "f16x2"}) == ("bf16x3", "f16x2")
    assert R(None, {"FLY_GEMM": "bf16x3"}) == ("bf16x3", "bf16x3")
    assert R(None, {"FLY_GEMM": "f32"}) == ("f32", "f32")
    assert R(None, {"FLY_STEP_GEMM": "bf16x3"}) == ("bf16x3", "bf16x3")
    assert R(None, {"FLY_GEMM": "f16x2", "FLY_STEP_GEMM": "bf16x3"}) == ("bf16x3", "bf16x3")
    assert R(None, {"FLY_GEMM": "bf16x3", "FLY_STEP_GEMM": "f16x2"}) == ("bf16x3", "f16x2")
    assert R(None, {"FLY_GEMM": "f32", "FLY_STEP_GEMM": "f16x2"}) == ("f32", "f32")
    for environ in ({}, {"FLY_GEMM": "f32", "FLY_STEP_GEMM": "bf16x3"}, {"FLY_STEP_GEMM": "f16x2"}):
        assert R("f16x2", environ) == ("bf16x3", "f16x2")
        assert R("bf16x3", environ) == ("bf16x3", "bf16x3")
        assert R("f32", environ) == ("f32", "f32")
    assert train_state.resolve_gemm(ns(gemm="f32")) == ("f32", "f32") and train_state.resolve_gemm(ns()) == ("bf16x3", "f16x2")


@pytest.mark.parametrize("n", [16, 1000, 4096, 40960, 40961])
def test_derived_values_match_their_definitions(n):
    if n == 40961:
        with pytest.raises(ValueError, match="mini_chunk_size 0"):
            resolve(num_envs=n)
        return
    T = (40960 // n) * 16
    for graph in (False, True):
        for want in (None, True, False):
            o = resolve(num_envs=n, graph=graph, persistent_rollout=want)
            assert (o.num_envs, o.mini_chunk_size, o.rollout_size, o.graph) == (n, 40960 // n, T, graph)
            assert o.persistent_rollout == (want is not False and T <= 4096 and not graph)


def test_the_seeds_of_rank_3():
    o = resolve(rank=3, seed=11)
    assert o.minibatch_seed == (11 + 3 * 0x9E3779B9) & 0xFFFFFFFF == (11 + 3 * 0x9E3779B9) % 2 ** 32 == o.dr_seed
    assert (o.rank, o.seed) == (3, 11) and 3 * 0x9E3779B9 > 2 ** 32            # (it wraps)
    o = resolve(rank=3, seed=11, minibatch_seed=0xF0000000, dr_seed=0xE0000000)
    assert o.minibatch_seed == (0xF0000000 + 3 * 0x9E3779B9) % 2 ** 32
    assert o.dr_seed == (0xE0000000 + 3 * 0x9E3779B9) % 2 ** 32
    assert (o.dr_ranges, o.dr_seed) == (tuple(options.dr_args(ns(rank=3, dr_seed=0xE0000000))[0][k] for k in options.DR_NAMES),
                                        options.dr_args(ns(rank=3, dr_seed=0xE0000000))[1])
    o = resolve(rank=None, seed=None)                       # what a launcher that sets neither leaves
    assert (o.rank, o.seed, o.minibatch_seed, o.dr_seed) == (0, 0, 0, 0)
    from fly_bproject_amd import fly
    assert fly.dr_args is options.dr_args and fly.DR_NAMES is options.DR_NAMES


@pytest.mark.parametrize("kw", [{}, FULL], ids=["default", "full"])
def test_expected_meta_is_a_projection(kw):
    args = resume_args(**kw)
    record = options.resolve(args, os.environ)
    meta = train_state.expected_meta(args)
    assert meta == {f: options.projection(record)[f] for f in train_state.META_FIELDS}
    assert list(meta) == list(train_state.META_FIELDS)
    dependents = ("minibatch_seed", "noise_rho", "obs_clip", "dr_ranges", "dr_seed")
    if kw:
        assert all(meta[f] is not None for f in dependents)
        assert meta["dr_ranges"] == [list(options.DR_DEFAULT_RANGES[k]) for k in options.DR_NAMES]
        assert (meta["noise_rho"], meta["obs_clip"], meta["minibatch_seed"], meta["dr_seed"]) == (0.5, 5.0, 0, 0)
    else:
        assert all(meta[f] is None for f in dependents)


def test_the_env_resolves_its_own_part_at_any_size():
    """`Fly(args)` stands on its own: a sparse namespace, and more envs than an agent's rollout allows."""
    e = options.resolve_env(types.SimpleNamespace(num_envs=65536))
    assert (e.num_envs, e.variant, e.reward, e.randomize, e.record, e.record_dir_name, e.time_steps_per_recorded_frame) == \
        (65536, "bigGrav", "standing", False, False, "recording", 2)
    assert not options.resolve_env(ns(record=True, rank=1)).record and options.resolve_env(ns(record=True)).record
    o = resolve(record=True, record_dir_name="clip", variant="lowGrav", randomize=True, dr_mass=[0.5, 2.0])
    for f in dataclasses.fields(options.EnvOptions):
        assert getattr(o, f.name) == getattr(options.resolve_env(ns(record=True, record_dir_name="clip", variant="lowGrav",
                                                                    randomize=True, dr_mass=[0.5, 2.0])), f.name)
    assert o.dr_ranges[options.DR_NAMES.index("mass")] == (0.5, 2.0)
