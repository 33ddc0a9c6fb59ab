"""CPU: the composed make_data reference (tests/make_data_ref.py) holds itself, and the bar it sets tells a right chain from
a wrong one.

  * with every option off it IS the existing references (bit for bit), and with one option on it is that option's reference
    called directly;
  * chain32 against chain64 over three iterations, per named output, as max |difference| relative to the output's largest
    |value|: the float32 rounding floor of the chain, measured here (printed; recorded in profiles/make_data_chain_error.txt).
    4 x these figures is the bar the GPU tests hold the agent to;
  * every wrong wiring of make_data_ref.WIRING_CHOICES, flipped one at a time, moves chain64 on some output of iteration 2 or
    3 by at least 100 x that bar."""
import numpy as np
import pytest

from tests import gae_episodic_ref as E
from tests import make_data_cases as C
from tests import make_data_ref as M
from tests import obs_norm_ref as O
from tests import reward_norm_ref as RN
from tests import rollout_ref as R
from tests import value_norm_ref as V
from tests import value_target_ref as VT

f32 = np.float32
FACTOR, CAUGHT = 4.0, 100.0          # the GPU bar is FACTOR x the floor; a wrong wiring must move an output by CAUGHT x the bar


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.fixture(scope="module", params=C.SHAPES, ids=lambda s: "T%d_N%d" % s)
def seq(request):
    T, N = request.param
    return T, N, C.sequence(T, N)


@pytest.fixture(scope="module")
def floors(seq):
    """chain64, chain32 with every option on over the three rollouts: ([out64], [out32], [{name: rel_err}])."""
    T, N, rollouts = seq
    kw = dict(minibatch_seeds=[0], minibatch_rows=(T // 16) * N)
    c64, c32 = C.chains(C.ALL_ON, T, N, **kw)
    o64, o32 = C.run(c64, rollouts), C.run(c32, rollouts)
    return o64, o32, [M.compare(a, b) for a, b in zip(o32, o64)]


def test_every_option_off_is_the_existing_reference(seq):
    T, N, rollouts = seq
    raw = rollouts[1]
    out = M.Chain({}, T, N, C.MAXLEN, precision="32").step(raw)
    tg, adv = V.td_gae(raw["reward"], raw["values"][:T], raw["values"][1:], raw["done"], M.IDENTITY)
    assert np.array_equal(_bits(out["target"]), _bits(tg)) and np.array_equal(_bits(out["advantage"]), _bits(adv))
    assert out["obs"] is not None and np.array_equal(out["obs"], raw["ring"][:T])
    ref = R.td_gae64(raw["reward"], raw["values"][:T], raw["values"][1:], raw["done"], *R.gamma_gl32(), 0)
    assert (np.abs(adv - ref.adv) <= ref.bound * 1.001 + 1e-30).all()       # and that is rollout_ref's estimator
    out64 = M.Chain({}, T, N, C.MAXLEN, precision="64").step(raw)
    assert np.array_equal(out64["advantage"], ref.adv) and np.array_equal(out64["target"], ref.target)
    for name in ("S_r_next", "obs_norm", "target_norm", "adv_totals", "epoch_keys"):
        assert name not in out


def test_one_option_on_is_that_options_reference(seq):
    T, N, rollouts = seq
    a, b = rollouts[0], rollouts[1]
    v = b["values"]
    # normalize_reward: two iterations, the second from the first one's carries and S_r
    ch = M.Chain(dict(normalize_reward=True), T, N, C.MAXLEN, precision="32")
    ch.step(a)
    ch.commit()
    out = ch.step(b)
    w1 = RN.walk(a["reward"], a["reset"], 0.99)
    w2 = RN.walk(b["reward"], b["reset"], 0.99, w1.carry)
    assert np.array_equal(_bits(out["carry_next"]), _bits(w2.carry))
    S = RN.merge(RN.merge((0.0, 0.0, 1.0), w1.G), w2.G)
    np.testing.assert_allclose(out["S_r_next"], S, rtol=1e-13)
    scaled = RN.scale(b["reward"], out["rnorm_table_next"][2], 10.0)
    assert np.array_equal(_bits(out["reward_scaled"]), _bits(scaled))
    tg, adv = V.td_gae(scaled, v[:T], v[1:], b["done"], M.IDENTITY)
    assert np.array_equal(_bits(out["advantage"]), _bits(adv)) and np.array_equal(_bits(out["target"]), _bits(tg))
    # normalize_obs
    ch = M.Chain(dict(normalize_obs=True), T, N, C.MAXLEN, precision="32")
    ch.step(a)
    ch.commit()
    out = ch.step(b)
    S = O.merge(O.initial(), a["ring"][1:])
    assert np.array_equal(_bits(out["obs_norm"]), _bits(O.normalize(b["ring"], O.table(S))))
    S2 = O.merge(S, b["ring"][1:])
    np.testing.assert_allclose(out["obs_stats_next"][1:], np.concatenate(S2[1:]), rtol=1e-12, atol=1e-13)
    # gae="episodic"
    out = M.Chain(dict(gae="episodic"), T, N, C.MAXLEN, precision="32").step(b)
    tg, adv = E.episodic32(b["reward"], v[:T], v[1:], b["reset"], b["progress"], b["reset_start"], C.MAXLEN)
    assert np.array_equal(_bits(out["target"]), _bits(tg)) and np.array_equal(_bits(out["advantage"]), _bits(adv))
    # normalize_value (under a table that is not the identity: second iteration)
    ch = M.Chain(dict(normalize_value=True), T, N, C.MAXLEN, precision="32")
    first = ch.step(a)
    ch.commit()
    out = ch.step(b)
    tab = V.table(V.merge(V.initial(), first["target_raw"]))
    assert tab[1] != 1.0 and np.array_equal(_bits(tab), _bits(first["value_table_next"]))
    tg, adv = V.td_gae(b["reward"], v[:T], v[1:], b["done"], tab)
    assert np.array_equal(_bits(out["target_raw"]), _bits(tg)) and np.array_equal(_bits(out["advantage"]), _bits(adv))
    tab2 = V.table(V.merge(V.merge(V.initial(), first["target_raw"]), tg))
    assert np.array_equal(_bits(out["target"]), _bits(V.normalize(tg, tab2)))
    # lambda_returns
    out = M.Chain(dict(lambda_returns=True), T, N, C.MAXLEN, precision="32").step(b)
    tg, adv = V.td_gae(b["reward"], v[:T], v[1:], b["done"], M.IDENTITY)
    assert np.array_equal(_bits(out["target"]), _bits(VT.lambda_targets(adv, v[:T])))
    # normalize_advantage
    out = M.Chain(dict(normalize_advantage=True), T, N, C.MAXLEN, precision="32").step(b)
    want = R.adv_normalise64(adv)[0]
    np.testing.assert_allclose(out["advantage"], want, rtol=2e-6, atol=2e-6)
    # two ranks: the statistics are those of both ranks' rows, the advantages are normalised by all 2 T N of them
    other = C.sequence(T, N, 1, rank=1)[0]
    o0, o1 = M.Chain(dict(C.ALL_ON, world_size=2), T, N, C.MAXLEN).step([a, other])
    both = np.concatenate([o0["advantage"].reshape(-1), o1["advantage"].reshape(-1)])
    assert abs(both.mean()) < 1e-6 and abs(both.std(ddof=1) - 1.0) < 1e-6
    assert o0["S_v_next"][0] == 2 * T * N and np.array_equal(o0["S_v_next"], o1["S_v_next"])
    np.testing.assert_allclose(o0["S_r_next"][1:], RN.moments(np.concatenate([o0["returns"], o1["returns"]]))[1:], rtol=1e-12)


def test_float32_floor_of_the_chain(seq, floors):
    """The figures: printed, finite, and small -- a float32 chain of this depth that is 1e-4 of the output's scale away from
    float64 would be a reference that is wrong, not rounding."""
    T, N, _ = seq
    _, _, figs = floors
    for k, fig in enumerate(figs):
        for name, x in fig.items():
            print("floor T=%d N=%d iteration %d %-18s %.3e" % (T, N, k, name, x))
            assert np.isfinite(x) and x < 1e-4, (k, name, x)
    for name in ("reward_scaled", "obs_norm", "target_raw", "advantage_raw", "target_norm", "advantage"):
        assert all(fig[name] > 0 for fig in figs), name              # float32 rounds: a floor of 0 here means nothing was compared
    # the tables of iteration 1 are not the identity, and rewards are not at the clip
    o64 = floors[0]
    assert abs(float(o64[0]["rnorm_table_next"][2]) - 1.0) > 0.1 and abs(float(o64[0]["value_table_next"][1]) - 1.0) > 0.01
    assert (np.abs(o64[2]["reward_scaled"]) >= 10.0).mean() <= 0.01


def test_the_cases_have_the_episode_structure(seq):
    T, N, rollouts = seq
    for k, raw in enumerate(rollouts):
        ended = raw["reset"] != 0
        timeout = ended & (raw["progress"] >= C.MAXLEN - 1)
        assert ended[T - 1].any() and ended[0].any()
        assert not (ended & ~timeout)[:, :2].any() and (ended & ~timeout)[:, 4:].any()      # some never fall, some fall
        assert timeout.any()
        assert (raw["reset_start"] == (1 if k == 0 else rollouts[k - 1]["reset"][T - 1])).all()
        if k:
            assert np.array_equal(raw["ring"][0], rollouts[k - 1]["ring"][T])
    # an open episode crosses each boundary
    assert (rollouts[0]["reset"][T - 1] == 0).any() and (rollouts[1]["reset"][T - 1] == 0).any()


# A wrong wiring has to show in the ROWS the optimizer is fed or a later stage reads, whose floor is float32 rounding.  The
# float64 statistics have floors of 1e-10 and less (rounding errors of the rows average out in them): any change at all is
# many times such a bar, so a ratio formed there would say nothing about the cases.
ROWS = ("reward_scaled", "obs_norm", "target_raw", "advantage_raw", "target_norm", "advantage", "mb0_target")

FLIPS = [(name, wrong, {}) for name, (_, wrong) in M.WIRING_CHOICES.items()]
# lambda-targets from normalised advantages is its own mistake only where make_data does not normalise them: there too
FLIPS.append(("lambda_reads", "normalised", dict(normalize_advantage=False)))


@pytest.mark.parametrize("name,wrong,options", FLIPS, ids=["%s=%s%s" % (n, w, "_no_advnorm" if o else "") for n, w, o in FLIPS])
def test_wrong_wirings_are_caught(seq, floors, name, wrong, options):
    T, N, rollouts = seq
    kw = dict(minibatch_seeds=[0], minibatch_rows=(T // 16) * N)
    if options:
        opts = dict(C.ALL_ON, **options)
        c64, c32 = C.chains(opts, T, N, **kw)
        right, o32 = C.run(c64, rollouts), C.run(c32, rollouts)
        figs = [M.compare(a, b) for a, b in zip(o32, right)]
    else:
        opts, (right, _, figs) = C.ALL_ON, floors
    bad = C.run(M.Chain(opts, T, N, C.MAXLEN, wiring={name: wrong}, **kw), rollouts)
    best = (0.0, None, None)
    for k in (1, 2):
        moved = M.compare(bad[k], right[k])
        for out, d in moved.items():
            if out not in ROWS:
                continue
            bar = FACTOR * figs[k][out]
            # where the two references agree to the last bit (float64 statistics, gathered rows) the floor is 0 and the GPU
            # test holds the output to its own bound instead; a ratio is only formed against a bar that exists
            if bar > 0 and d / bar > best[0]:
                best = (d / bar, out, k)
        if name == "epoch_keys":
            # the keys feed nothing but the permutation: the witness is step 0's gathered targets, held bit for bit on the GPU
            d = moved["mb0_target"]
            assert d > 0.1 and not np.array_equal(bad[k]["epoch_keys"], right[k]["epoch_keys"])
            best = max(best, (d / (FACTOR * max(figs[k]["target_norm"], 1e-300)), "mb0_target", k))
    print("wrong wiring %s=%s T=%d N=%d: %s of iteration %d moves by %.3g x its bar" % (name, wrong, T, N, best[1], best[2], best[0]))
    assert best[0] >= CAUGHT, best


# ------------------------------------------------------------------------- the GPU tests' checks, checked without a GPU
def _checks(T, N, rollouts, options, wiring=None):
    """tests/make_data_capture.py's checks of one rank on a float32 chain that poses as the agent."""
    from tests import make_data_capture as K
    info, its = C.pose_as_agent(M.Chain(options, T, N, C.MAXLEN, precision="32", wiring=wiring), rollouts)
    K.check_coverage(info, its)
    c64, c32 = K.chain_pair(info, minibatch_seeds=[0], minibatch_rows=info["mb_rows"])
    outs64, outs32, states = [], [], []
    for it in its:
        outs64.append(c64.step(it["raw"]))
        outs32.append(c32.step(it["raw"]))
        c64.commit()
        c32.commit()
        states.append(c64.state())
    return K.check_rank(info, its, outs64, outs32, states)


OPTION_SETS = {"all": C.ALL_ON,
               "ref_gae": dict(gae="reference", normalize_reward=True, normalize_value=True, lambda_returns=True,
                               normalize_advantage=True),
               "no_vnorm": dict(normalize_reward=True, lambda_returns=True, gae="episodic", normalize_advantage=True)}


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_the_gpu_checks_pass_on_a_right_chain(seq, name):
    T, N, rollouts = seq
    worst = _checks(T, N, rollouts, OPTION_SETS[name])
    print("float32 chain as the agent, %s: worst error / bar %s" % (name, worst))
    assert 0 < max(worst.values()) <= 0.2501                     # chain32 against chain64 is the floor itself: 1 / FACTOR


@pytest.mark.parametrize("name,wrong", [(n, w[1]) for n, w in M.WIRING_CHOICES.items()])
def test_the_gpu_checks_fail_on_every_wrong_wiring(seq, name, wrong):
    T, N, rollouts = seq
    with pytest.raises(AssertionError):
        _checks(T, N, rollouts, C.ALL_ON, {name: wrong})
