"""PPO.make_data and update()'s commits as ONE reference: the per-stage references of tests/ composed in the kernels' order,
fed only what a rollout leaves behind, carrying its own committed state from iteration to iteration.  numpy; nothing here
imports the agent or a kernel.

    chain = Chain(options, T, N)            # options: a dict of make_data's switches, see OPTIONS
    out = chain.step(raw)                   # every intermediate and output of this iteration, by name (one rank: a dict)
    chain.commit()                          # what update() commits behind the optimizer steps

`raw` (a dict; a list of them, one per rank in rank order, with world_size > 1) holds the rollout's rows before make_data:
    ring     f32 [T+1][N][73]   the raw observation ring
    reward   f32 [T][N]         all_reward
    values   f32 [T+1][N]       the critic's outputs on the ring (normalised units with normalize_value): an input here
    reset, progress  int64 [T][N]   the flag rows
    reset_start      int64 [N]      the env's reset_buf when the rollout began (checked against the chain's own ended_prev)
    done     f32 [N]            gae="reference" only: the last step's mask

The stages, in order:
    returns G from the committed carries -> S_r with them folded in -> its table -> reward_scaled under the NEW table
    obs_norm: the ring under the COMMITTED obs table; the moments of rows 1..T go into the obs statistics at the commit
    GAE on reward_scaled and the critic outputs denormalised under the COMMITTED value table -> TD targets, raw advantages
    lambda-targets = raw advantage + denormalised v (overwrite the targets; S_v takes THEIR moments)
    S_v with the targets' moments folded in -> its table -> target_norm under the NEW table
    advantages normalised by the moments of all ranks' rows
    the epoch keys update * 5 + e of the shuffled minibatches
Statistics of several ranks are moment sets combined in rank order (Chan et al.), then folded into S.

Two evaluations of the same wiring:
    precision="64"   everything in float64 from the float32 inputs; only the TABLES are rounded to float32, where the product
                     rounds them (S -> table, the advantage totals): a table is data the next stage reads
    precision="32"   the float32 references of tests/ in the kernels' order (reward_norm_ref.scale, obs_norm_ref.normalize,
                     gae_episodic_ref.episodic32 / value_norm_ref.td_gae, value_target_ref.lambda_targets,
                     value_norm_ref.normalize), float64 moments of what they give

WIRING names every choice the Python around the kernels makes; `Chain(..., wiring={"gae_reads": "raw"})` evaluates a WRONG
chain (tests/test_make_data_chain_cpu.py shows that each one is seen)."""
import numpy as np

from tests import gae_episodic_ref as E
from tests import minibatch_ref as MB
from tests import obs_norm_ref as O
from tests import reward_norm_ref as RN
from tests import rollout_ref as R
from tests import value_norm_ref as V
from tests import value_target_ref as VT

f32 = np.float32
EPOCHS = 5
IDENTITY = np.array([0.0, 1.0, 1.0, 0.0], f32)

OPTIONS = dict(normalize_reward=False, normalize_obs=False, normalize_value=False, lambda_returns=False,
               normalize_advantage=False, gae="reference", minibatch="reference", world_size=1)

# choice -> (the product's, the wrong one)
WIRING_CHOICES = {
    "denorm_table": ("committed", "scratch"),        # scratch: v denormalised under THIS iteration's new value table
    "sv_from": ("final_targets", "td_targets"),      # td_targets: S_v takes the TD targets' moments though lambda replaced them
    "adv_norm_at": ("after_lambda", "before_lambda"),  # before_lambda: advantages normalised first, everything after reads them
    "lambda_reads": ("raw", "normalised"),           # normalised: the lambda-targets alone are formed from normalised advantages
    "gae_reads": ("scaled", "raw"),                  # raw: GAE reads all_reward though normalize_reward made a scaled copy
    "commit_carries": (True, False),                 # False: S_r commits, the return carries stay where they were
    "ended_prev": ("rollout_start", "stale"),        # stale: the flags of the first rollout's start, never refreshed
    "epoch_keys": ("advance", "stuck"),              # stuck: the update count behind the epoch keys never moves
}
WIRING = {k: v[0] for k, v in WIRING_CHOICES.items()}


def rel_err(got, want):
    """max |got - want| relative to the largest |want| (0 / 0 = 0): the figure every comparison of chains is made in."""
    got, want = np.asarray(got), np.asarray(want)
    if want.size == 0:
        return 0.0
    d = np.subtract(got, want, dtype=np.float64)
    np.abs(d, out=d)
    d, m = float(d.max()), max(float(want.max()), -float(want.min()))
    return d / m if m > 0 else d


def cached(raw, name, key, make):
    """raw[name] = (key, value), made once per key: the chains and the tests' stage checks share what is float64 either way
    (the ring's moments) or the same float32 reference under the same table, at 48 M elements a second each."""
    if name not in raw or raw[name][0] != key:
        raw[name] = (key, make())
    return raw[name][1]


def obs_normalize32(raw, tab):
    return cached(raw, "_obs_norm32", tab.tobytes(), lambda: O.normalize(raw["ring"], tab))


def ring_moments(raw):
    return cached(raw, "_obs_moments", None, lambda: obs_moments3(raw["ring"][1:]))


def moments3(x):
    """(count, mean, M2) of all elements of x in float64, two passes."""
    return VT.moments(x)


def fold(S, sets):
    """S = (count, mean, var) with the moment sets [(count, mean, M2)] combined in order and folded in."""
    nb, mb, qb = VT.combine(sets)
    c, mu, var = S
    if not nb > 0:
        return S
    n = c + nb
    d = mb - mu
    return n, mu + d * (nb / n), (var * c + qb + d * d * (c * nb / n)) / n


def obs_moments3(rows):
    x = np.asarray(rows, np.float64).reshape(-1, np.shape(rows)[-1])
    mean = x.mean(axis=0)
    return float(x.shape[0]), mean, ((x - mean) ** 2).sum(axis=0)


def obs_fold(S, sets):
    """fold() per column: S = (count, mean[k], var[k]), sets = [(count, mean[k], M2[k])] in rank order."""
    n, mean, m2 = sets[0]
    for nb, mb, qb in sets[1:]:
        t, d = n + nb, mb - mean
        mean = mean + d * (nb / t)
        m2 = m2 + qb + d * d * (n * nb / t)
        n = t
    c, mu, var = S
    tot = c + n
    d = mean - mu
    return tot, mu + d * (n / tot), (var * c + m2 + d * d * (c * n / tot)) / tot


def adv_totals32(sets):
    """The float32 pair (sum, M2) ppo_adv_apply reads: all ranks' float64 moments combined in rank order, rounded once."""
    n, mean, m2 = VT.combine(sets)
    return np.array([n * mean, max(m2, 0.0)], np.float64).astype(f32), n


def adv_apply(adv, totals, count, precision):
    """(adv - mean) / (std + 1e-8), std with ddof = 1, from the float32 totals, in float64; precision "32" rounds the result
    once (ppo_adv_apply's arithmetic)."""
    mean = float(totals[0]) / count
    var = max(float(totals[1]) / (count - 1.0), 0.0)
    inv = 1.0 / (np.sqrt(var) + float(f32(1e-8)))
    out = (np.asarray(adv, np.float64) - mean) * inv
    return out.astype(f32) if precision == "32" else out


class Chain:
    def __init__(self, options, T, N, max_episode_length=37, gamma=0.99, lam=0.95, reward_clip=10.0, obs_clip=5.0,
                 precision="64", wiring=None, minibatch_seeds=None, minibatch_rows=None):
        unknown = set(options) - set(OPTIONS)
        assert not unknown, unknown
        self.opt = dict(OPTIONS, **options)
        assert self.opt["gae"] in ("reference", "episodic") and precision in ("64", "32")
        self.wiring = dict(WIRING, **(wiring or {}))
        assert all(self.wiring[k] in WIRING_CHOICES[k] for k in self.wiring) and set(self.wiring) == set(WIRING)
        self.T, self.N, self.W = T, N, int(self.opt["world_size"])
        self.maxlen, self.gamma, self.lam = max_episode_length, gamma, lam
        self.g32, self.gl32 = R.gamma_gl32(gamma, lam)
        self.reward_clip, self.obs_clip, self.precision = reward_clip, obs_clip, precision
        self.mb_seeds, self.mb_rows = minibatch_seeds, minibatch_rows
        # the committed state
        self.S_r, self.rnorm_table = (0.0, 0.0, 1.0), RN.table((0.0, 0.0, 1.0))
        self.carry = [np.zeros(N) for _ in range(self.W)]
        self.S_v, self.value_table = V.initial(), V.table(V.initial())
        self.S_obs = O.initial()
        self.obs_table = O.table(self.S_obs, obs_clip)
        self.ended_prev = [None] * self.W                # set from the first rollout's reset_start
        self.update = 0
        self._next = None

    # ------------------------------------------------------------------------------------------------------ the stages
    def _scale(self, reward, r):
        if self.precision == "32":
            return RN.scale(reward, r, self.reward_clip)
        c = float(f32(self.reward_clip))
        return np.clip(reward.astype(np.float64) * float(f32(r)), -c, c)

    def _obs_normalize(self, raw, tab):
        if self.precision == "32":
            return obs_normalize32(raw, tab)
        k = (tab.size - 1) // 2
        t = tab.astype(np.float64)
        x = raw["ring"].astype(np.float64)
        x -= t[:k]
        x *= t[k:2 * k]
        return np.clip(x, -t[2 * k], t[2 * k], out=x)

    def _gae(self, reward, raw, ended_prev, tab):
        """(TD targets, raw advantages) [T][N] of the estimator in use, v denormalised under `tab` (None: as it is)."""
        T, v = self.T, raw["values"]
        if self.opt["gae"] == "episodic":
            flags = (raw["reset"], raw["progress"], ended_prev, self.maxlen)
            if self.precision == "32":
                return E.episodic32(reward, v[:T], v[1:], *flags, table=tab, gamma=self.gamma, lam=self.lam)
            ref = E.episodic64(reward, v[:T], v[1:], *flags, self.g32, self.gl32, tab)
            return ref.target, ref.adv
        done = np.asarray(raw["done"], f32).reshape(-1)
        if self.precision == "32":
            return V.td_gae(reward, v[:T], v[1:], done, IDENTITY if tab is None else tab, self.gamma, self.lam, 0)
        vd = v.astype(np.float64) if tab is None else v.astype(np.float64) * float(tab[1]) + float(tab[0])
        ref = R.td_gae64(reward, vd[:T], vd[1:], done, self.g32, self.gl32, 0)
        return ref.target, ref.adv

    def _lambda(self, adv, v, tab):
        return VT.lambda_targets(adv, v, tab) if self.precision == "32" else VT.lambda_targets64(adv, v, tab)

    def _vnormalize(self, tg, tab):
        if self.precision == "32":
            return V.normalize(tg, tab)
        return (np.asarray(tg, np.float64) - float(tab[0])) * float(tab[2])

    def _normalise_all(self, advs):
        totals, n = adv_totals32([moments3(a) for a in advs])
        return [adv_apply(a, totals, n, self.precision) for a in advs], totals

    def _targets(self, raws, rewards, prevs, tab):
        """GAE and, with lambda_returns, the lambda-targets of every rank under the denormalisation table `tab`:
        -> per rank (targets, TD targets, raw advantages, the advantages make_data goes on with)."""
        opt, w, T = self.opt, self.wiring, self.T
        td, adv_raw = zip(*[self._gae(rewards[i], raws[i], prevs[i], tab) for i in range(self.W)])
        adv = list(adv_raw)
        if opt["normalize_advantage"] and w["adv_norm_at"] == "before_lambda":
            adv = self._normalise_all(adv)[0]
        reads = adv
        if w["lambda_reads"] == "normalised":
            reads = self._normalise_all(list(adv_raw))[0]
        tg = list(td)
        if opt["lambda_returns"]:
            tg = [self._lambda(reads[i], raws[i]["values"][:T], tab) for i in range(self.W)]
        return tg, list(td), list(adv_raw), adv

    # --------------------------------------------------------------------------------------------------- one iteration
    def step(self, raw):
        single = isinstance(raw, dict)
        raws = [raw] if single else list(raw)
        opt, w, T, N, W = self.opt, self.wiring, self.T, self.N, self.W
        assert len(raws) == W
        outs = [dict() for _ in range(W)]
        nxt = {}
        for i, r in enumerate(raws):
            assert r["reward"].shape == (T, N) and r["values"].shape == (T + 1, N) and r["reward"].dtype == f32
            if self.ended_prev[i] is None:
                self.ended_prev[i] = np.asarray(r["reset_start"]).copy()
        prevs = [p for p in self.ended_prev]
        # reward scaling
        rewards = [r["reward"] for r in raws]
        if opt["normalize_reward"]:
            walks = [RN.walk(r["reward"], r["reset"], self.gamma, self.carry[i]) for i, r in enumerate(raws)]
            nxt["S_r"] = fold(self.S_r, [moments3(x.G) for x in walks])
            nxt["rnorm_table"] = RN.table(nxt["S_r"])
            nxt["carry"] = [x.carry for x in walks]
            for i, o in enumerate(outs):
                o["returns"], o["carry_next"], o["return_smax"] = walks[i].G, walks[i].carry, walks[i].smax
                o["S_r_next"], o["rnorm_table_next"] = np.array(nxt["S_r"]), nxt["rnorm_table"]
                o["reward_scaled"] = self._scale(raws[i]["reward"], nxt["rnorm_table"][2])
            if w["gae_reads"] == "scaled":
                rewards = [o["reward_scaled"] for o in outs]
        # observation normalisation: the committed table normalises, the moments wait for the commit
        if opt["normalize_obs"]:
            sets = []
            for i, o in enumerate(outs):
                o["obs_norm"] = self._obs_normalize(raws[i], self.obs_table)
                sets.append(ring_moments(raws[i]))               # float64 either way: shared by the two precisions
            nxt["S_obs"] = obs_fold(self.S_obs, sets)
            nxt["obs_table"] = O.table(nxt["S_obs"], self.obs_clip)
            for o in outs:
                o["obs_stats_next"] = np.concatenate([[nxt["S_obs"][0]], nxt["S_obs"][1], nxt["S_obs"][2]])
                o["obs_table_next"] = nxt["obs_table"]
        # GAE, lambda-targets, value normalisation
        tab = self.value_table if opt["normalize_value"] else None
        tg, td, adv_raw, adv = self._targets(raws, rewards, prevs, tab)
        if opt["normalize_value"]:
            if w["denorm_table"] == "scratch":
                first = V.table(fold(self.S_v, [moments3(x) for x in tg]))
                tg, td, adv_raw, adv = self._targets(raws, rewards, prevs, first)
            sets = [moments3(x) for x in (td if w["sv_from"] == "td_targets" else tg)]
            nxt["S_v"] = fold(self.S_v, sets)
            nxt["value_table"] = V.table(nxt["S_v"])
            for i, o in enumerate(outs):
                n, mean, m2 = sets[i]
                o["value_moments"] = np.array([n, mean, m2 / n])
                o["S_v_next"], o["value_table_next"] = np.array(nxt["S_v"]), nxt["value_table"]
                o["target_norm"] = self._vnormalize(tg[i], nxt["value_table"])
        for i, o in enumerate(outs):
            o["target_raw"], o["advantage_raw"] = tg[i], adv_raw[i]
        if opt["normalize_advantage"] and w["adv_norm_at"] == "after_lambda":
            adv, totals = self._normalise_all(adv)
            for o in outs:
                o["adv_totals"] = totals
        # what make_data returns
        for i, o in enumerate(outs):
            o["advantage"] = adv[i]
            o["target"] = o["target_norm"] if opt["normalize_value"] else o["target_raw"]
            o["obs"] = o["obs_norm"][:T] if opt["normalize_obs"] else raws[i]["ring"][:T]
            o["ended_prev"] = prevs[i]
            o["ended_prev_next"] = np.asarray(raws[i]["reset"][T - 1]).copy()
        # shuffled minibatches: the epoch keys of this update, and step 0's rows of the targets as a witness
        if opt["minibatch"] == "shuffled":
            keys = [MB.epoch_key(self.update, EPOCHS, e) for e in range(EPOCHS)]
            for i, o in enumerate(outs):
                o["epoch_keys"] = np.array(keys, np.int64)
                if self.mb_seeds is not None:
                    idx = MB.perm_index(T * N, self.mb_seeds[i], keys[0], np.arange(self.mb_rows))
                    o["mb0_index"] = idx
                    o["mb0_target"] = np.asarray(o["target"]).reshape(-1)[idx]
        nxt["ended_prev"] = [o["ended_prev_next"] for o in outs]
        self._next = nxt
        return outs[0] if single else outs

    def commit(self):
        """What update() leaves behind the optimizer steps: scratch -> committed."""
        nxt, w = self._next, self.wiring
        assert nxt is not None, "commit() without a step()"
        if "S_r" in nxt:
            self.S_r, self.rnorm_table = nxt["S_r"], nxt["rnorm_table"]
            if w["commit_carries"]:
                self.carry = nxt["carry"]
        if "S_obs" in nxt:
            self.S_obs, self.obs_table = nxt["S_obs"], nxt["obs_table"]
        if "S_v" in nxt:
            self.S_v, self.value_table = nxt["S_v"], nxt["value_table"]
        if w["ended_prev"] == "rollout_start":
            self.ended_prev = nxt["ended_prev"]
        if self.opt["minibatch"] == "shuffled" and w["epoch_keys"] == "advance":
            self.update += 1
        self._next = None

    def state(self):
        """The committed state by the names the agent's attributes go by."""
        s = {"update": self.update, "ended_prev": self.ended_prev}
        if self.opt["normalize_reward"]:
            s.update(S_r=np.array(self.S_r), rnorm_table=self.rnorm_table, carry=self.carry)
        if self.opt["normalize_value"]:
            s.update(S_v=np.array(self.S_v), value_table=self.value_table)
        if self.opt["normalize_obs"]:
            s.update(S_obs=np.concatenate([[self.S_obs[0]], self.S_obs[1], self.S_obs[2]]), obs_table=self.obs_table)
        return s


# the outputs two chains are compared in (whatever of them the options produce)
COMPARED = ("S_r_next", "rnorm_table_next", "carry_next", "reward_scaled", "obs_norm", "obs_stats_next", "obs_table_next",
            "target_raw", "advantage_raw", "value_moments", "S_v_next", "value_table_next", "target_norm", "advantage",
            "mb0_target")


def compare(got, want, names=COMPARED):
    """{name: rel_err} over the outputs both dicts hold."""
    return {k: rel_err(got[k], want[k]) for k in names if k in got and k in want}
