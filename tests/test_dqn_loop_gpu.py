"""GPU (-m gpu): the DQN training loop (`DQN.run()` / `DQN.update()`; reference UselessFiles/dqn.py:64-126) held to float64 on the
rows it actually trains on -- real `Fly` observations, rewards and done == 0 rows, fp16x2 scales that lag one update behind the data,
chunks that are views of replay-ring slots in sampled order -- where every other float64 test of the update runs on `torch.randn`
rows the scales were calibrated on, and the loop around it is only smoke-tested (tests/test_dqn.py::test_dqn_runs_end_to_end).

A `DQN` is built as that test builds it and `run()` is called with recorders wrapped around INSTANCE attributes (`act`, `env.step`,
`replay.sample_slots`, `_fused_launch_h2`, `update`: fly_bproject_amd/dqn.py is not touched).  The transcript is then held to
tests/dqn_loop_ref.py (itself held to torch in tests/test_dqn_loop_ref_cpu.py):
  * the ring against the transcript, bit for bit (`check_transcript`), and the stored action against the eps-greedy of the float64
    Q values under the weights in front of the step (rows any fp32 arithmetic may decide either way left out: at most 2 % of a case);
  * every update against float64, restarted from the device's own state in front of it (the idiom of test_fused_step_vs_oracle_resynced):
    the returned loss, `packed.G` per tensor (_kink_reference / _beyond of tests/test_dqn_h2_gpu.py under the scales recorded in
    front of that launch), the optimizer's buffers and copies (check_dqn_adam_soft of tests/test_adam_step_gpu.py); a refused update
    left everything bit-identical and its redo is a record of its own (none occurs at these seeds: one more run of case b has a
    lagged scale pushed 2^14 too high, as tests/test_dqn_h2_gpu.py does it, and is held the same way through the refusal);
  * negative controls: the reference fed the neighbouring slots, done = 1 everywhere, or the following step's obs for next_obs misses.

Cases (the smallest at which each path can still go wrong):
    a  96 envs, 5 sampled of 7 stored steps, 24 steps   fused update, three tiles per slot, the ring wraps three times
    b  32 envs, 3 of 4, 14 steps                        fused update, one tile per slot, the smallest ring
    c  40 envs, 3 of 5, 14 steps                        n % 32 != 0: `dqn_td_step` / `dqn_grad_w` on a ragged tile
Every env starts flagged, so the first step resets them all and clears `progress_buf`: the time-limit envs (one per later step) are
set in front of the run as tests/test_hip_parity.py sets progress[3] = 1497, and again after that first step.

Bars: loss 2e-6 |loss| + 1e-9 and 2e-5 of a tensor's scale are the project's (tests/test_dqn_h2_gpu.py); the fused error <= twice the
per-step fp32-MFMA path's + 2e-6 is test_h2_gradient_error_against_float64_beside_bf16x3's rule, and so is the cap on ambiguous
pairs: at most 1e-4 of an update's (row, unit) pairs, held for every applied update (the count over a case is printed beside it).
The tables the tests print are profiles/dqn_loop_float64.txt."""
import contextlib
import io
import re
import types

import numpy as np
import pytest
import torch

from tests import dqn_loop_ref as LR
from tests.test_adam_step_gpu import check_dqn_adam_soft
from tests.test_dqn import _bare_dqn
from tests.test_dqn_h2_gpu import KINK_K, _beyond, _kink_reference

pytestmark = pytest.mark.gpu

CASES = {"a": dict(envs=96, mbs=5, cap=7, steps=24), "b": dict(envs=32, mbs=3, cap=4, steps=14), "c": dict(envs=40, mbs=3, cap=5, steps=14)}
PARAMS = [("a", "f16x2"), ("a", "bf16x3"), ("b", "f16x2"), ("b", "bf16x3"), ("c", None)]
BAR, LOSS_RTOL, LOSS_ATOL = 2e-5, 2e-6, 1e-9
NO_SCALE = 2.0 ** 40        # "no scales" for _kink_reference: the sign-loss term 2^-25 / (0.01 s) vanishes, the GEMM term is left
EVAL_FREQ = 4               # the score line every 4th step (an instance attribute: the loop's default of 100 lies past these runs)
GRADS = ("dW1", "db1", "dW2", "db2", "dW3", "db3")
SNAP = ("P", "P_tgt", "exp_avg", "exp_avg_sq", "step", "PF", "PT", "PF_tgt", "QB", "QTB", "QB_tgt")
assert KINK_K == LR.KINK_K
_RECORDED = {}            # (case, gemm, push_at) -> the recorded run: each loop runs once per module, its agent is closed at the end


def _np(t):
    return t.detach().cpu().numpy().copy()


def _record(case, gemm, push_at=None):
    key = (case, gemm, push_at)
    if key not in _RECORDED:
        _RECORDED[key] = _run_recorded(case, gemm, push_at)
    return _RECORDED[key]


def _run_recorded(case, gemm, push_at):
    """Run the loop of one case with the recorders on.  -> namespace(agent, transcript, updates, arith, final).
    push_at: in front of that step the lagged scale of class X is pushed 2^14 too high (as tests/test_dqn_h2_gpu.py does it), so that
    the step's fp16x2 update does not fit and is refused on the device."""
    from fly_bproject_amd.dqn import DQN
    from tests.hip_helpers import make_args
    c = CASES[case]
    torch.manual_seed(0)
    kw = {} if gemm is None else {"dqn_gemm": gemm}
    with contextlib.redirect_stdout(io.StringIO()):
        agent = DQN(make_args(c["envs"], dqn_mini_batch_size=c["mbs"], replay_steps=c["cap"], **kw))
    agent.num_eval_freq = EVAL_FREQ
    pk, rb, env = agent.packed, agent.replay, agent.env
    assert rb.capacity == c["cap"]
    fused = agent.fused_update and c["envs"] % 32 == 0
    arith = (agent.update_gemm if fused else "f32")
    cur, stack, updates = {}, [], []
    snap = lambda: {k: getattr(pk, k).clone() for k in SNAP}   # noqa: E731

    orig_act, orig_step, orig_sample, orig_h2, orig_update = agent.act, env.step, rb.sample_slots, agent._fused_launch_h2, agent.update

    def act(obs, epsilon=0.0):
        cur["w"] = [p_.detach().clone() for p_ in agent.q.parameters()]
        cur["act_obs"] = obs.clone()
        a = orig_act(obs, epsilon)
        cur.update(eps=epsilon, coin=agent._coin.clone(), rand=agent._rand.clone(), action=a.clone())
        return a

    def step(actions):
        orig_step(actions)
        cur.update(step_obs=env.obs_buf.clone(), step_reward=env.reward_buf.clone(), step_reset=env.reset_buf.clone())

    def sample_slots(k):
        s = list(orig_sample(k))
        stack[-1]["slots"] = s
        if len(stack) == 1:
            cur["slot_lists"].append(s)
        return s

    def fused_launch_h2(dev, S, n, aligned, inv_B, flags):
        if flags in (0, 1):
            stack[-1]["scales"] = pk.h2_scales.clone()           # the scales THIS launch runs under
        return orig_h2(dev, S, n, aligned, inv_B, flags)

    def update(chunks=None):
        rec = {"run_step": cur["run_step"], "depth": len(stack), "pre": snap(), "ring": {k: getattr(rb, k).clone() for k in LR.FIELDS},
               "head": rb.head, "count": rb.count, "slots": None, "scales": None, "b3": bool(agent._h2_use_b3)}
        stack.append(rec)
        loss = orig_update(chunks)
        torch.cuda.synchronize()
        stack.pop()
        rec.update(post=snap(), G=pk.G.clone(), overflow=int(pk.h2_overflow), loss=float(loss), loss_tensor=loss)
        rec["index"] = len(updates)
        updates.append(rec)                                      # an update _h2_poll made inside another completes first
        for outer in stack:                                      # ... and moved the state the outer one really starts from
            outer["pre"] = snap()
        if not stack:
            cur["ring_before_update"], cur["update"] = rec["ring"], rec
        return loss

    agent.act, env.step, rb.sample_slots, agent._fused_launch_h2, agent.update = act, step, sample_slots, fused_launch_h2, update
    steps = []
    for t in range(1, c["steps"] + 1):
        if t <= 2:      # env 3 + 2 j reaches the time limit at step 2 + j (a reset clears progress, and step 1 resets every env)
            j = torch.arange(c["steps"] - 1, device=env.device)
            env.progress_buf[3 + 2 * j] = env.max_episode_length - 2 - j
        if t == push_at:
            with torch.no_grad():
                pk.h2_scales[0] *= 2.0 ** 14
                pk.h2_scales[16] /= 2.0 ** 14
        cur.clear()
        cur.update(run_step=agent.run_step, obs_before=env.obs_buf.clone(), slot_lists=[])
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            agent.run()
        torch.cuda.synchronize()
        h = (t - 1) % c["cap"]
        cur["row"] = tuple(x[h].clone() for x in (rb.obs, rb.action, rb.reward, rb.next_obs, rb.done))
        cur.update(head=rb.head, count=rb.count, size=rb.size(), last_loss=agent.last_loss, printed=out.getvalue())
        steps.append(dict(cur))
    cur.clear()
    cur.update(run_step=None, slot_lists=[])                     # (updates the closing poll makes belong to no step)
    with contextlib.redirect_stdout(io.StringIO()):
        agent._h2_poll(block=True)
    torch.cuda.synchronize()
    final = dict(step=int(pk.step), issued=agent._updates_issued, overflows=agent.h2_overflows, overflow_word=int(pk.h2_overflow))
    agent.act, env.step, rb.sample_slots, agent._fused_launch_h2, agent.update = orig_act, orig_step, orig_sample, orig_h2, orig_update
    tr = {"capacity": c["cap"], "mini_batch_size": c["mbs"], "steps": steps}
    return types.SimpleNamespace(agent=agent, transcript=tr, updates=updates, arith=arith, final=final, case=c)


@pytest.fixture(scope="module", autouse=True)
def _close_the_recorded_agents():
    yield
    for rec in _RECORDED.values():
        rec.agent.exit()
    _RECORDED.clear()


def _host(v):
    if isinstance(v, torch.Tensor):
        return _np(v)
    if isinstance(v, (tuple, list)) and v and isinstance(v[0], torch.Tensor):
        return tuple(_np(x) for x in v)
    if isinstance(v, dict) and v and all(isinstance(x, torch.Tensor) for x in v.values()):
        return {k: _np(x) for k, x in v.items()}
    return v


def _refused(rec):
    return int(rec["post"]["step"]) == int(rec["pre"]["step"])


def _done0_rows(rec):
    return int(sum(int((rec["ring"]["done"][s] == 0).sum()) for s in rec["slots"]))


def _check_ring(rec):
    """The recorded transcript on the host, through tests/dqn_loop_ref.check_transcript.  -> (host transcript, its statistics)."""
    tr = rec.transcript
    keep = lambda s: {k: _host(v) for k, v in s.items() if k not in ("w", "update", "last_loss")}   # noqa: E731
    host = {"capacity": tr["capacity"], "mini_batch_size": tr["mini_batch_size"], "steps": [keep(s) for s in tr["steps"]]}
    return host, LR.check_transcript(host)


@pytest.mark.parametrize("case,gemm", PARAMS)
def test_ring_follows_the_transcript(case, gemm):
    """Section by section of `run()`: the slot a step is recorded in holds the env's observation in front of the step, the action `act`
    returned, the reward and observation the step left BEFORE the reset, done = 1 - reset_buf of that step; head / count / size()
    follow commit(); every env carries next_obs into the next step's obs -- the ones that reset too: `Fly`'s reset, like the reference's
    (fly.py:446-480), restores the simulation state and leaves the observation buffer to the next step, so next_obs stored before or
    after the reset is the same row here, and tests/test_dqn_loop_ref_cpu.py shows the checker telling the two apart for an env whose
    reset does repack observations; at least one env resets; updates begin exactly
    when size() > mini_batch_size, one per step, each on mini_batch_size distinct slots below count; every slot in front of an update
    is what its last writer left; epsilon follows the schedule.  The stored action is the float64 eps-greedy's; `last_loss` and the
    score line are those of the update the step just made."""
    rec = _record(case, gemm)
    c, tr = rec.case, rec.transcript
    host, stats = _check_ring(rec)
    assert stats["updates"] == c["steps"] - c["mbs"]
    # at least one sampled slot of at least one update holds a done == 0 row
    sampled_done0 = [_done0_rows(u) for u in rec.updates]
    assert max(sampled_done0) > 0, sampled_done0
    # the stored action
    left_out = rows = ties = edges = explored = 0
    for s, hs in zip(tr["steps"], host["steps"]):
        w = [_np(x) for x in s["w"]]
        want, out, cnt = LR.expected_actions(w, hs["act_obs"], hs["coin"], hs["rand"], hs["eps"])
        keep = ~out
        assert np.array_equal(hs["action"][keep].view(np.int32), want[keep].view(np.int32)), ("step", hs["run_step"], "eps-greedy action")
        left_out += int(out.sum()); rows += out.size; ties += cnt["tie"]; edges += cnt["edge"]; explored += cnt["explore"]
    print("\ncase %s %s: %d steps x %d envs, %d rows reset, %d done == 0 rows in sampled slots; actions: %d explored, %d greedy, "
          "left out %d of %d (%d ties, %d on the coin edge)" % (case, rec.arith, c["steps"], c["envs"], stats["reset_envs"],
                                                               sum(sampled_done0), explored, rows - explored, left_out, rows, ties, edges))
    assert left_out <= 0.02 * rows, (left_out, rows)
    assert 0 < explored < rows                                   # both branches of the mix occurred
    # the loss the loop keeps and prints is the one of the update the step just made; the score is the mean reward of the update steps
    acc, lines = 0.0, 0
    for s, hs in zip(tr["steps"], host["steps"]):
        u = s.get("update")
        if u is None:
            assert s["last_loss"] is None and s["printed"] == ""
            continue
        assert s["last_loss"] is u["loss_tensor"] and u["depth"] == 0 and u["slots"] == s["slot_lists"][0]
        acc += float(hs["row"][2].astype(np.float64).mean()) / EVAL_FREQ
        m = re.search(r"Steps: (\d+) \| Reward (-?[\d.]+) \| TD Loss (-?[\d.]+) Epsilon ([\d.]+) Buffer (\d+)", s["printed"])
        assert (m is not None) == (hs["run_step"] % EVAL_FREQ == 0), (hs["run_step"], s["printed"])
        if m:
            lines += 1
            assert int(m.group(1)) == hs["run_step"] and int(m.group(5)) == hs["size"]
            assert abs(float(m.group(3)) - u["loss"]) <= 5.1e-5 + 1e-6 * abs(u["loss"]), (m.group(0), u["loss"])     # (four printed decimals)
            assert abs(float(m.group(2)) - acc) <= 5.1e-5 + 1e-5 * abs(acc), (m.group(0), acc)
            acc = 0.0
    assert lines >= 2
    # every step past the threshold has had its update, refused ones redone
    assert rec.final["step"] == rec.final["issued"] == c["steps"] - c["mbs"] and rec.final["overflow_word"] == 0, rec.final


def _shadow(rec, u, d):
    """`d` (a bare per-step fp32-MFMA DQN) with the networks as they were in front of update `u`."""
    for k in ("P", "P_tgt", "exp_avg", "exp_avg_sq", "step"):
        getattr(d.packed, k).copy_(u["pre"][k])
    d.packed.refresh()
    return d


def _reference(rec, u, d):
    """float64 of update `u` on the device's own state in front of it: (loss64, numpy gradient, the batch, w, wt)."""
    ring = {k: _np(v) for k, v in u["ring"].items()}
    b = LR.batch(ring, u["slots"])
    w = [_np(p_) for p_ in d.q.parameters()]
    wt = [_np(p_) for p_ in d.q_target.parameters()]
    loss64, g64, _ = LR.loss_and_grad(w, wt, b)
    return loss64, g64, b, w, wt, ring


def _check_updates(rec, case):
    """Every recorded update of `rec` against float64 (the two tests below); prints the table.  -> {"refused", "redone"}."""
    c = rec.case
    pk = rec.agent.packed
    d = _bare_dqn(rows=c["envs"], fused=False)
    mask = _np(pk.grad_mask)
    cls = np.where(mask == 1, "bulk", "masked").astype(object)
    applied = [u for u in rec.updates if not _refused(u)]
    rerun = {applied[0]["index"], applied[len(applied) // 2]["index"], applied[-1]["index"]} if case == "a" else set()
    figures, failures, table = [], [], []
    amb_all = pairs_all = refused = 0
    worst = [0.0] * 6
    for u in rec.updates:
        tag = "case %s %s update %d" % (case, rec.arith, u["index"])
        if _refused(u):
            refused += 1
            assert u["overflow"] != 0, (tag, "a refused update must have set the overflow word")
            for k in SNAP:
                assert torch.equal(u["post"][k], u["pre"][k]), (tag, k, "a refused update wrote")
            table.append("%3d %4d refused (class maxima %s)" % (u["index"], u["run_step"], ["%.3g" % x for x in _np(u["scales"])[32:48]]))
            continue
        assert int(u["post"]["step"]) == int(u["pre"]["step"]) + 1, tag
        arith = "bf16x3" if (u["b3"] and rec.arith == "f16x2") else rec.arith
        assert (u["scales"] is not None) == (arith == "f16x2"), tag
        _shadow(rec, u, d)
        loss64, g64, b, w, wt, ring = _reference(rec, u, d)
        loss_err = abs(u["loss"] - loss64)
        if not loss_err <= LOSS_RTOL * abs(loss64) + LOSS_ATOL:
            failures.append((tag, "loss", u["loss"], loss64))
        sc = _np(u["scales"]) if u["scales"] is not None else None
        s_h1, s_h2 = (float(sc[1]), float(sc[2])) if sc is not None else (NO_SCALE, NO_SCALE)
        chunks = LR.chunks(u["ring"], u["slots"])
        want, eff, n_amb, pairs, _ = _kink_reference(d, chunks, s_h1, s_h2)
        for a, g in zip(want, g64):                              # (the CPU-held reference and the suite's are one gradient)
            assert float(np.abs(_np(a) - g).max()) <= 1e-8 * float(np.abs(g).max()), tag
        errs, flipped = _beyond(u["G"], want, eff)
        amb_all += n_amb; pairs_all += pairs
        assert n_amb <= 1e-4 * pairs, (tag, "ambiguous pairs", n_amb, pairs)
        worst = [max(a, e) for a, e in zip(worst, errs)]
        line = "%3d %4d %-6s slots %-16s done0 %3d  amb %2d flip %2d |" % (u["index"], u["run_step"], arith, u["slots"], int((b[4] == 0).sum()), n_amb, flipped)
        line += " ".join("%.2e" % e for e in errs)
        for name, e in zip(GRADS, errs):
            if not e <= BAR:
                failures.append((tag, name, "error %.3e of its scale > %g" % (e, BAR)))
        if u["index"] in rerun:
            d.update(chunks)                                     # the same rows and weights through dqn_td_step / dqn_grad_w
            torch.cuda.synchronize()
            e32, _ = _beyond(d.packed.G.clone(), want, eff)
            line += " | f32 " + " ".join("%.2e" % e for e in e32)
            for name, e, f in zip(GRADS, errs, e32):
                if not e <= 2 * f + 2e-6:
                    failures.append((tag, name, "error %.3e > 2 x fp32-MFMA's %.3e + 2e-6" % (e, f)))
        line += " | loss %.1e of %.4f applied" % (loss_err / max(abs(loss64), 1e-30), loss64)
        table.append(line)
        # the optimizer on the device's own gradient and state
        inp = {"P": _np(u["pre"]["P"]), "G": _np(u["G"]), "m": _np(u["pre"]["exp_avg"]), "v": _np(u["pre"]["exp_avg_sq"]), "mask": mask}
        after = types.SimpleNamespace(idx_f=pk.idx_f, idx_t=pk.idx_t, idx_fb=pk.idx_fb, idx_tb=pk.idx_tb, **u["post"])
        with contextlib.redirect_stdout(io.StringIO()):
            check_dqn_adam_soft(tag, after, inp, _np(u["pre"]["P_tgt"]).astype(np.float64), int(u["pre"]["step"]), cls, figures)
    print("\n==== case %s (%d envs, %d of %d slots, %d steps), %s: every update against float64, max |g - g64| / max |g64| per tensor (%s) ===="
          % (case, c["envs"], c["mbs"], c["cap"], c["steps"], rec.arith, " ".join(GRADS)))
    print("  u step arith  ...")
    for ln in table:
        print(ln)
    print("worst per tensor: %s; ambiguous pairs %d of %d (%.2e); refused updates: %d (h2_overflows %d)"
          % (" ".join("%.2e" % e for e in worst), amb_all, pairs_all, amb_all / max(pairs_all, 1), refused, rec.final["overflows"]))
    print("optimizer: %d applied updates checked element by element; the last one:" % len(applied))
    for ln in figures[-2:]:
        print(ln)
    assert amb_all <= 1e-4 * pairs_all, (amb_all, pairs_all)
    assert not failures, failures
    assert len(applied) == c["steps"] - c["mbs"]
    assert refused == 0 or rec.arith == "f16x2"
    return {"refused": refused, "redone": sum(1 for u in applied if u["b3"])}


@pytest.mark.parametrize("case,gemm", PARAMS)
def test_every_update_against_float64_resynchronised(case, gemm):
    """Every update the loop made: applied (step + 1; loss, gradient, optimizer buffers and copies against float64 from the device's
    own state in front of it) or refused (the overflow word set, every buffer and the step word bit-identical).  Case a: the first, a
    middle and the last update also through the per-step fp32-MFMA launches on the same rows and weights; the fused error is held to
    twice that + 2e-6.  For these seeds no refusal is expected; a count that is not zero is printed with the class maxima behind it."""
    st = _check_updates(_record(case, gemm), case)
    assert st["redone"] == st["refused"]


def test_a_refused_update_hides_nothing():
    """Case b, f16x2, with the lagged scale of class X pushed 2^14 too high in front of step 8 (the disturbance of
    test_h2_overflow_in_the_training_loop_is_refused_on_the_device_and_settled_later): that step's update is refused on the device --
    the overflow word set, every buffer and the step word bit-identical -- and `_h2_poll` forms it again in bf16x3 from inside the
    next step's update.  The redo is a record of its own, completed before the update it ran inside, and is held to float64 at the
    same bars; the ring keeps its rules through it; at the end every step past the threshold has had its update."""
    rec = _record("b", "f16x2", 8)
    c = rec.case
    _check_ring(rec)
    st = _check_updates(rec, "b")
    assert st["refused"] >= 1 and st["redone"] == st["refused"] and rec.final["overflows"] >= st["refused"], (st, rec.final)
    first = next(u for u in rec.updates if _refused(u))
    assert first["run_step"] == 8 and first["depth"] == 0
    redo = [u for u in rec.updates if u["b3"]]
    assert all(u["depth"] == 1 and u["scales"] is None for u in redo)
    outer = rec.updates[redo[-1]["index"] + 1]                   # the update the redo ran inside completes after it, in fp16x2 again
    assert outer["depth"] == 0 and outer["run_step"] == redo[-1]["run_step"] and outer["scales"] is not None and not _refused(outer)
    assert torch.equal(outer["pre"]["P"], redo[-1]["post"]["P"])  # ... and starts from what the redo left
    assert rec.final["step"] == rec.final["issued"] == c["steps"] - c["mbs"] and rec.final["overflow_word"] == 0, rec.final


def test_negative_controls_miss_their_bars():
    """Case a, f16x2, one update whose batch holds a done == 0 row (and the ring's newest slot: the following step's obs differs from
    next_obs only on rows that reset -- whose bootstrap term done == 0 masks, which is why the ring is held bit for bit above -- and in
    the newest slot, whose successor is the OLDEST step).  The reference fed the slots (s + 1) % capacity misses the gradient bar;
    fed done = 1 everywhere it misses the loss bar; fed the following step's obs for next_obs it misses the loss bar."""
    rec = _record("a", "f16x2")
    cap = rec.case["cap"]
    pick = [u for u in rec.updates if not _refused(u) and u["scales"] is not None and _done0_rows(u) > 0 and u["count"] == cap
            and (u["head"] - 1) % cap in u["slots"]]
    assert pick, "no update of case a holds a done == 0 row and the newest slot"
    u = pick[len(pick) // 2]
    d = _shadow(rec, u, _bare_dqn(rows=rec.case["envs"], fused=False))
    loss64, g64, b, w, wt, ring = _reference(rec, u, d)
    bar = LOSS_RTOL * abs(loss64) + LOSS_ATOL
    assert abs(u["loss"] - loss64) <= bar
    sc = _np(u["scales"])
    shifted = [(s + 1) % cap for s in u["slots"]]
    want, eff, _, _, _ = _kink_reference(d, LR.chunks(u["ring"], shifted), float(sc[1]), float(sc[2]))
    errs, _ = _beyond(u["G"], want, eff)
    obs, act, rew, nxt, done = b
    loss_done1, _, _ = LR.loss_and_grad(w, wt, (obs, act, rew, nxt, np.ones_like(done)))
    nxt_following = np.concatenate([ring["obs"][s] for s in shifted])
    loss_nxt, _, _ = LR.loss_and_grad(w, wt, (obs, act, rew, nxt_following, done))
    print("\nnegative controls on update %d (slots %s, %d done == 0 rows, loss %.6f, bar %.1e): neighbouring slots -> gradient off by %s; "
          "done = 1 -> loss off by %.2e; next_obs = the following step's obs -> loss off by %.2e"
          % (u["index"], u["slots"], int((done == 0).sum()), loss64, bar, ["%.1e" % e for e in errs], abs(u["loss"] - loss_done1), abs(u["loss"] - loss_nxt)))
    assert max(errs) > BAR, errs
    assert abs(u["loss"] - loss_done1) > LOSS_RTOL * abs(loss_done1) + LOSS_ATOL
    assert abs(u["loss"] - loss_nxt) > LOSS_RTOL * abs(loss_nxt) + LOSS_ATOL
