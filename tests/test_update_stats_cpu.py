"""CPU: PPO update diagnostics (PPO --update_stats) without a GPU -- the numpy reference's identities and its
merge, the condition on the seeded cases, the option table and the flag, the new header against its binding table, the refusals
of the two entry points (they return before any HIP call), the score-line suffix and the reader's dict from given sets, and the
state block."""
import math
import os
import types

import numpy as np
import pytest
import torch

from fly_bproject_amd import options, train_state
from tests import update_stats_cases as cases
from tests import update_stats_ref as R


def _set(c, **kw):
    c = c._replace(**kw)
    return R.set_of(c.mu, c.action, c.old_logp, c.adv, c.v, c.target, c.var, c.clip)


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def test_reference_by_hand():
    """var = 1 in every column (hld = 0) and a = mu except one column: M = 0.25, logp = -0.5 (C + 0.25)."""
    mu = np.zeros((2, 18), np.float32)
    action = np.zeros((2, 18), np.float32)
    action[:, 5] = 0.5
    var = np.ones(18, np.float32)
    logp = -0.5 * (R.LOG_2PI_18 + 0.25)
    old = np.array([logp, logp - math.log(2.0)], np.float32)         # ratios 1 and 2 (to fp32 rounding of old_logp)
    t = R.row_terms(mu, action, old, [1.0, -1.0], [0.5, 3.0], [0.0, 0.0], var, 0.2)
    assert t.M.tolist() == [0.25, 0.25] and t.finite.all() and t.clipped.tolist() == [False, True]
    assert abs(t.ratio[0] - 1) < 1e-6 and abs(t.ratio[1] - 2) < 1e-6
    assert abs(t.pol[0] + 1) < 1e-6 and abs(t.pol[1] - 2) < 1e-6      # -min(1 * 1, 1 * 1);  -min(2 * -1, 1.2 * -1) = 2
    assert t.hub.tolist() == [0.125, 2.5]
    s = R.set_from_terms(t, [1.0, -1.0], [0.5, 3.0], [0.0, 0.0])
    assert s[[R.ROWS, R.CLIPPED, R.NONFINITE, R.AMAX, R.TMAX, R.TN, R.TMEAN, R.TM2]].tolist() == [2, 1, 0, 1, 0, 2, 0, 0]
    assert (s[R.EN], s[R.EMEAN], s[R.EM2]) == (2.0, -1.75, 3.125)
    assert R.empty_set().tolist() == [0, 0, 0, 0, np.inf, -np.inf] + [0] * 11
    assert R.clip_edges(0.2) == (float(np.float32(1) - np.float32(0.2)), float(np.float32(1) + np.float32(0.2)))
    assert R.K == 22 and R.U == 2.0 ** -24 and R.LOG_2PI_18 == float(np.float32(33.08178959434617))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_reference_identities(seed):
    c = cases.case(300, seed)
    t = R.row_terms(*c[:8])
    assert t.finite.all() and (t.k3 >= 0).all()                       # k3 = r - 1 - ln r >= 0
    assert t.clipped.any() and not t.clipped.all()
    assert (t.ratio[t.clipped] < t.lo).any() and (t.ratio[t.clipped] > t.hi).any()
    # an identical policy: old_logp is the new log-prob -> KL 0, nothing clipped (to the fp32 rounding of old_logp)
    logp = -0.5 * (R.LOG_2PI_18 + t.M) - np.log(np.sqrt(c.var.astype(np.float64))).sum()
    s = _set(c, old_logp=logp.astype(np.float32))
    assert s[R.CLIPPED] == 0 and abs(s[R.K1]) / 300 < 1e-5 and 0 <= s[R.K3] / 300 < 1e-10
    assert abs(s[R.RMIN] - 1) < 1e-5 and abs(s[R.RMAX] - 1) < 1e-5
    # a perfect critic, and one that predicts the mean of its targets
    s = _set(c, v=c.target.copy())
    assert s[R.EM2] == 0 and s[R.HUB] == 0 and 1 - s[R.EM2] / s[R.TM2] == 1.0
    s = _set(c, v=np.full(300, c.target.astype(np.float64).mean()).astype(np.float32))
    assert abs(1 - s[R.EM2] / s[R.TM2]) < 1e-6                        # EV 0 (the mean is rounded to fp32)


def test_the_nonfinite_rule():
    c = cases.case(64, 3, bad=True)
    t = R.row_terms(*c[:8])
    assert sorted(np.flatnonzero(~t.finite).tolist()) == sorted(c.bad_rows) and len(set(c.bad_rows)) == 3
    s = _set(c)
    assert s[R.ROWS] == 64 and s[R.NONFINITE] == 3 and s[R.TN] == 61 and s[R.EN] == 61 and np.isfinite(s).all()
    keep = t.finite
    clean = R.set_of(c.mu[keep], c.action[keep], c.old_logp[keep], c.adv[keep], c.v[keep], c.target[keep], c.var, c.clip)
    clean[R.ROWS], clean[R.NONFINITE] = 64, 3
    assert np.array_equal(s, clean)                                   # a non-finite row counts in rows and nonfinite, nothing else
    # a bad var makes every row non-finite
    for bad in (0.0, -1.0, np.nan):
        var = c.var.copy()
        var[7] = bad
        s = _set(c, var=var)
        assert s[R.ROWS] == 64 == s[R.NONFINITE] and np.array_equal(s[1:14], R.empty_set()[1:14]) and s[R.AMAX] == s[R.TMAX] == 0


def test_merge_of_splits_is_the_set_of_the_whole():
    c = cases.case(1027, 7, bad=True)
    whole = _set(c)
    cuts = [0, 1, 64, 64, 300, 1000, 1027]                             # one empty part among them
    parts = [R.set_of(c.mu[a:b], c.action[a:b], c.old_logp[a:b], c.adv[a:b], c.v[a:b], c.target[a:b], c.var, c.clip)
             if b > a else R.empty_set() for a, b in zip(cuts[:-1], cuts[1:])]
    pooled = R.merge_all(parts)
    exact = list(R.EXACT) + [R.RMIN, R.RMAX]
    assert np.array_equal(pooled[exact], whole[exact])
    for k in R.SUMS:
        assert math.isclose(pooled[k], whole[k], rel_tol=1e-12, abs_tol=1e-12)
    for k in (R.TMEAN, R.TM2, R.EMEAN, R.EM2):
        assert math.isclose(pooled[k], whole[k], rel_tol=1e-10, abs_tol=1e-12)
    assert np.array_equal(R.merge(R.empty_set(), whole), whole) and np.array_equal(R.merge(whole, R.empty_set()), whole)


@pytest.mark.parametrize("R_,seed,bad", cases.GPU_CASES)
def test_the_condition_on_the_cases(R_, seed, bad):
    """Every case the GPU tests use: no finite row's ratio within its margin of a clip edge; and what the docstring promises."""
    c = cases.case(R_, seed, bad)
    t = R.row_terms(*c[:8])
    assert R.clip_margin_ok(t)
    assert int((~t.finite).sum()) == (3 if bad else 0)
    assert len(set(c.var.tolist())) == 18
    if R_ >= 63:
        f = t.finite
        assert (t.ratio[f] < t.lo).any() and (t.ratio[f] > t.hi).any() and ((t.ratio[f] > t.lo) & (t.ratio[f] < t.hi)).any()
        assert (c.adv > 0).any() and (c.adv < 0).any() and (c.adv == 0).any()
        dv = np.abs(c.v.astype(np.float64) - c.target.astype(np.float64))[f]
        assert (dv < 1).any() and (dv == 1).any() and (dv > 1).any()
        assert t.b[f].max() < 1e-3                                    # the margin is rounding, not a tolerance


# ---- option, flag ----------------------------------------------------------------------------------------------------------------
def test_option_flag_and_an_untouched_state_meta():
    import trainer
    opt = options.BY_NAME["update_stats"]
    assert opt.default is False and opt.choices is None and opt.env is None
    assert trainer.parse_args([]).update_stats is False and trainer.parse_args(["--update_stats"]).update_stats is True
    for args, want in ((trainer.parse_args([]), False), (trainer.parse_args(["--update_stats"]), True),
                       (types.SimpleNamespace(num_envs=1000), False), (types.SimpleNamespace(num_envs=1000, update_stats=1), True)):
        rec = options.resolve(args, os.environ)
        assert rec.update_stats is want and "update_stats" not in options.projection(rec)
        assert "update_stats" not in train_state.expected_meta(args) and "update_stats" not in train_state.expected_meta_ext(args)
    assert "--update_stats" in trainer.__doc__ and "DESIGN.md 3.3j" in trainer.__doc__
    assert train_state.FORMAT == 1 and len(train_state.META_FIELDS) == 22 and train_state.META_EXT_FIELDS == ("lambda_returns",)
    on, off = types.SimpleNamespace(num_envs=1000, update_stats=True), types.SimpleNamespace(num_envs=1000)
    train_state.check_meta(train_state.expected_meta(off), on)
    train_state.check_meta_ext(train_state.expected_meta_ext(on), off)


def test_flag_help(capsys):
    import trainer
    with pytest.raises(SystemExit):
        trainer.parse_args(["--help"])
    out = " ".join(capsys.readouterr().out.split())
    assert "--update_stats" in out and "approximate KL" in out and "explained variance" in out


# ---- header, binding, refusals ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fly_bproject_amd import _lib
    _lib.build()
    return _lib.load()


def test_the_header_and_its_binding_table(lib, monkeypatch, tmp_path):
    """include/flyhip_update_stats.h (which flyhip.h includes at its end, behind flyhip_ext.h) against _lib.SYMBOLS_UPDATE_STATS,
    prototype by prototype; the two constants against a host program that includes flyhip.h; and nothing of it in SYMBOLS,
    SYMBOLS_EXT, api() or ext(), whose version stays 13."""
    from fly_bproject_amd import _lib
    from tests import abi_header
    from tests.test_abi_cpu import _host_program_values
    main = open(abi_header.HEADER).read()
    assert main.count('#include "flyhip_update_stats.h"') == 1
    assert main.index('#include "flyhip_ext.h"') < main.index('#include "flyhip_update_stats.h"')
    assert "ppo_update_stats" not in abi_header.header_text().replace('#include "flyhip_update_stats.h"', "")
    assert len(abi_header.prototypes()) == 66                         # flyhip.h's own list did not move
    monkeypatch.setattr(abi_header, "HEADER", os.path.join(abi_header.REPO, "include", "flyhip_update_stats.h"))
    protos = abi_header.prototypes()
    assert protos == {
        "ppo_update_stats": ("int", ["const float*"] * 7 + ["float", "int64_t", "double*", "void*"]),
        "ppo_update_stats_merge": ("int", ["const double*", "int64_t", "double*", "double*", "double*", "void*"])}
    assert set(protos) == set(_lib.SYMBOLS_UPDATE_STATS)
    assert not set(protos) & set(_lib.SYMBOLS) and not set(protos) & set(_lib.SYMBOLS_EXT)
    for name, (ret, params) in protos.items():
        want = [abi_header.ctype_of(t, {}) for t in params]
        fn = getattr(lib, name)
        assert _lib.SYMBOLS_UPDATE_STATS[name] == want == list(fn.argtypes) and fn.restype is abi_header.RETURNS[ret], name
    us = _lib.update_stats_api()
    assert us is _lib.update_stats_api() and set(vars(us)) == set(_lib.SYMBOLS_UPDATE_STATS)
    assert not set(vars(us)) & set(vars(_lib.api())) and not set(vars(us)) & set(vars(_lib.ext()))
    assert set(_lib.SYMBOLS_EXT) == {"ppo_reward_returns", "ppo_reward_scale"} and len(_lib.SYMBOLS) == 65
    with pytest.raises(_lib.FlyHipError, match=r"ppo_update_stats_merge failed \(-1\): ppo_update_stats_merge: null pointer"):
        us.ppo_update_stats_merge(None, 4, None, None, None, None)
    got = _host_program_values(tmp_path, "update_stats_macros", ("flyhip.h",),
                               {"FLY_UPDATE_STATS_SET": "FLY_UPDATE_STATS_SET", "FLY_UPDATE_STATS_SETS": "FLY_UPDATE_STATS_SETS"})
    assert got == {"FLY_UPDATE_STATS_SET": _lib.UPDATE_STATS_SET, "FLY_UPDATE_STATS_SETS": _lib.UPDATE_STATS_SETS}
    assert (_lib.UPDATE_STATS_SET, _lib.UPDATE_STATS_SETS) == (R.SET, R.SETS) == (17, 256)
    assert _lib.ABI_VERSION == 13 == lib.fly_abi_version()


def test_stats_refusals(lib):
    """Fake addresses: every refusal returns before any HIP call (a launch on them would fault, and no GPU is needed)."""
    f = lib.ppo_update_stats
    ptrs = [0x10000 * (k + 1) for k in range(7)]
    sets = 0x90000
    good = ptrs + [0.2, 64, sets, None]
    for i in list(range(7)) + [9]:
        args = list(good)
        args[i] = None
        assert f(*args) == -1 and b"null pointer" in lib.fly_last_error(), i
    for R_ in (0, -1):
        assert f(*(ptrs + [0.2, R_, sets, None])) == -1 and b"R must be > 0" in lib.fly_last_error()
    for clip in (0.0, 1.0, -0.2, 1.5, float("nan"), float("inf")):
        assert f(*(ptrs + [clip, 64, sets, None])) == -1 and b"clip must be in (0, 1)" in lib.fly_last_error()
    assert f(*(ptrs + [0.2, 1 << 60, sets, None])) == -1 and b"overflow" in lib.fly_last_error()
    for i in range(7):
        for off in (1, 2, 3):
            args = list(good)
            args[i] += off
            assert f(*args) == -1 and b"4-byte aligned" in lib.fly_last_error(), (i, off)
    assert f(*(ptrs + [0.2, 64, sets + 4, None])) == -1 and b"8-byte aligned" in lib.fly_last_error()


def test_merge_refusals(lib):
    g = lib.ppo_update_stats_merge
    sets, last, window, total = 0x10000, 0x20000, 0x30000, 0x40000
    good = [sets, 256, last, window, total, None]
    for i in (0, 2, 3, 4):
        args = list(good)
        args[i] = None
        assert g(*args) == -1 and b"null pointer" in lib.fly_last_error(), i
    for n in (0, -4):
        assert g(sets, n, last, window, total, None) == -1 and b"nsets must be > 0" in lib.fly_last_error()
    assert g(sets, 1 << 60, last, window, total, None) == -1 and b"overflows" in lib.fly_last_error()
    for i in (0, 2, 3, 4):
        args = list(good)
        args[i] += 4
        assert g(*args) == -1 and b"8-byte aligned" in lib.fly_last_error(), i
    for a, b, c in ((last, last, total), (last, window, last + 8 * 16), (last, window, window - 8), (total, window, total)):
        assert g(sets, 256, a, b, c, None) == -1 and b"must not overlap" in lib.fly_last_error()


# ---- suffix and reader ------------------------------------------------------------------------------------------------------------------
def test_suffix_and_reader_from_given_sets():
    from fly_bproject_amd import ppo
    empty = ppo.update_stats_empty()
    assert empty.dtype == torch.float64 and empty.tolist() == R.empty_set().tolist()
    assert ppo.update_stats_suffix(empty.tolist()) == " | KL n/a"
    e = ppo.update_stats_entries(empty.tolist())
    assert e["rows"] == 0 and e["nonfinite"] == 0 and all(math.isnan(v) for k, v in e.items() if k not in ("rows", "nonfinite"))
    s = [100, 0.49, 0.294, 7, 0.5, 1.75, -2.94, 11.76, 98, 1.0, 50.0, 98, 0.0, 5.0, 2, 3.0, 4.0]
    e = ppo.update_stats_entries(s)
    assert e == {"rows": 100, "nonfinite": 2, "approx_kl": 0.294 / 98, "kl_k1": 0.49 / 98, "clip_fraction": 7 / 98, "ratio_min": 0.5,
                 "ratio_max": 1.75, "policy_loss": -2.94 / 98, "value_loss": 11.76 / 98, "loss": -2.94 / 98 + 11.76 / 98,
                 "explained_variance": 1 - 5.0 / 50.0, "target_mean": 1.0, "target_std": (50.0 / 98) ** 0.5, "adv_absmax": 3.0,
                 "target_absmax": 4.0}
    assert type(e["rows"]) is int and type(e["nonfinite"]) is int and all(type(v) is float for k, v in e.items() if k not in ("rows", "nonfinite"))
    assert ppo.update_stats_suffix(s) == " | KL 0.00300 | Clip 7.1% | EV 0.900 | Loss 0.0900 | Nonfinite 2"
    s[14], s[8], s[11] = 0, 100, 100
    assert ppo.update_stats_suffix(s) == " | KL 0.00294 | Clip 7.0% | EV 0.900 | Loss 0.0882"
    s[10] = 0.0                                                         # constant targets: no explained variance
    assert math.isnan(ppo.update_stats_entries(s)["explained_variance"]) and " | EV nan | " in ppo.update_stats_suffix(s)
    bad = R.empty_set()
    bad[R.ROWS] = bad[R.NONFINITE] = 64                                 # every row non-finite
    e = ppo.update_stats_entries(bad.tolist())
    assert (e["rows"], e["nonfinite"]) == (64, 64) and all(math.isnan(v) for k, v in e.items() if k not in ("rows", "nonfinite"))
    assert ppo.update_stats_suffix(bad.tolist()) == " | KL nan | Clip nan% | EV nan | Loss nan | Nonfinite 64"


# ---- state block ---------------------------------------------------------------------------------------------------------------------------
def test_state_block_pack_and_restore():
    from fly_bproject_amd import ppo
    live = {k: ppo.update_stats_empty() for k in ("last", "window", "total")}
    live["total"][:] = torch.arange(17, dtype=torch.float64)
    block = {k: train_state.pack(v) for k, v in live.items()}
    assert all(b.dtype == torch.float64 and b.shape == (17,) and b.data_ptr() != live[k].data_ptr() for k, b in block.items())
    back = {k: torch.zeros(17, dtype=torch.float64) for k in live}
    for k in back:
        train_state.restore(back[k], block, "agent.update_stats", k)
        assert torch.equal(back[k], live[k])
    with pytest.raises(ValueError, match=r"agent.update_stats.window is missing"):
        train_state.restore(back["window"], {"last": block["last"]}, "agent.update_stats", "window")
    with pytest.raises(ValueError, match=r"agent.update_stats.last is \(10,\) torch.float64"):
        train_state.restore(back["last"], {"last": torch.zeros(10, dtype=torch.float64)}, "agent.update_stats", "last")
