"""The float64 reference of the data-parallel optimizer step (tests/test_dist_step_ref_cpu.py pins it on the CPU,
tests/test_dist_step_gpu.py holds the kernels to it).

Plain torch and nothing else: a `Net(73, 18)` in float64, the project's loss (`PPO.minibatch_loss` on a bare agent), autograd,
`clip_grad_norm_(…, 1.0)` and `torch.optim.Adam(lr=1e-3)` on the WHOLE batch of 2 n rows.  No kernel, no packed layout, no
all-reduce: what two data-parallel ranks of n rows each have to reproduce is this single-process step.  Rank r owns rows
[r n, (r + 1) n).

The batch has the distributions of `_setup` in tests/test_mlp_train_gpu.py (one generator seed), drawn on the CPU in fp32 so that
every process -- the CPU test, the GPU test's parent and its ranks -- holds the same bits; the reference widens those bits to
float64, it does not draw its own."""
import functools

import torch

STEPS = 3               # the ping-pong step counter of `self_norm` goes through both parities
BOOST_STEP = 1          # the step whose advantages are multiplied by BOOST: the clip bites there and nowhere else
BOOST = 50.0
CLIP = 0.2
MAX_NORM = 1.0
LR = 1e-3
SEED = 5


def _bare_agent(net, var):
    from fly_bproject_amd.ppo import PPO
    p = PPO.__new__(PPO)
    p.net, p.action_var, p.clip = net, var, CLIP
    return p


@functools.lru_cache(maxsize=None)
def problem(n, seed=SEED):
    """(state_dict, batch) for n rows PER RANK: the initial fp32 weights of `Net(73, 18)` under `torch.manual_seed(seed)` and the
    fp32 batch (x [2n, 73], action [2n, 18], old_logp [2n], adv [2n], target [2n], var [18]) of 2 n rows.  Cached: treat as
    read-only."""
    from fly_bproject_amd.ppo import Net, diag_gauss_logprob
    rows = 2 * n
    state = torch.get_rng_state()
    try:
        torch.manual_seed(seed)
        net = Net(73, 18)
    finally:
        torch.set_rng_state(state)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, 73, generator=g)
    var = torch.full((18,), 0.15)
    with torch.no_grad():
        mu = net.to_mean(net.shared_net(x))
        action = (mu + 0.4 * torch.randn(rows, 18, generator=g)).clamp(-1, 1)
        old_logp = diag_gauss_logprob(mu, action, var) + 0.3 * torch.randn(rows, generator=g)
    adv = torch.randn(rows, generator=g)
    target = torch.randn(rows, generator=g) * 1.5
    return sd, (x, action, old_logp, adv, target, var)


def rank_rows(batch, rank, n):
    """Rank `rank`'s rows [rank n, (rank + 1) n) of a batch of `problem` (the variance is shared)."""
    x, action, old_logp, adv, target, var = batch
    s = slice(rank * n, (rank + 1) * n)
    return x[s], action[s], old_logp[s], adv[s], target[s], var


def step_advantage(adv, it):
    """The advantages of step `it`: times BOOST at BOOST_STEP."""
    return adv * BOOST if it == BOOST_STEP else adv


def make_net(sd, dtype):
    from fly_bproject_amd.ppo import Net
    net = Net(73, 18).to(dtype)
    net.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return net


def loss_and_grads(net, rows, it, dtype):
    """(loss, {name: gradient}) of the project's loss over `rows` (a batch or a rank's part of one) at step `it`, in `dtype`."""
    x, action, old_logp, adv, target, var = (t.to(dtype) for t in rows)
    agent = _bare_agent(net, var)
    for p in net.parameters():
        p.grad = None
    loss = agent.minibatch_loss(x, action, old_logp, target.unsqueeze(-1), step_advantage(adv, it).unsqueeze(-1))
    loss.backward()
    return loss.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


def run_steps(n, dtype=torch.float64, seed=SEED):
    """STEPS optimizer steps on the whole batch of 2 n rows in `dtype`.  One dict per step: `loss`, `grads` (per parameter, before
    the clip), `norm` (the pre-clip norm), `clipped`, and `params`, `exp_avg`, `exp_avg_sq` (per parameter, after the step)."""
    sd, batch = problem(n, seed)
    net = make_net(sd, dtype)
    opt = torch.optim.Adam(net.parameters(), lr=LR)
    out = []
    for it in range(STEPS):
        loss, grads = loss_and_grads(net, batch, it, dtype)         # leaves the gradients in .grad
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), MAX_NORM)
        opt.step()
        named = dict(net.named_parameters())
        out.append({"loss": float(loss), "grads": grads, "norm": float(norm), "clipped": float(norm) > MAX_NORM,
                    "params": {k: p.detach().clone() for k, p in named.items()},
                    "exp_avg": {k: opt.state[p]["exp_avg"].clone() for k, p in named.items()},
                    "exp_avg_sq": {k: opt.state[p]["exp_avg_sq"].clone() for k, p in named.items()}})
    return out


@functools.lru_cache(maxsize=None)
def reference(n, seed=SEED):
    """`run_steps` in float64, computed once per size and shared.  Treat as read-only."""
    return run_steps(n, torch.float64, seed)
