"""CPU: the float64 reference of the data-parallel optimizer step (tests/dist_step_ref.py) pinned without a GPU, so that a
disagreement in tests/test_dist_step_gpu.py is the kernels' and not the reference's.

  * the gradient (and the loss) of the whole batch is the mean of the gradients (losses) of its two halves -- the identity the
    data-parallel update rests on: each rank divides by ITS row count, the all-reduced sum is scaled by 1 / world;
  * the float64 computation agrees with the same computation in fp32 torch within the suite's autograd bar;
  * the clip branch is taken in the step with the boosted advantages and in no other."""
import pytest
import torch

from tests import dist_step_ref as R

N = 33                  # rows per rank: the smaller size of the GPU test


def test_whole_batch_gradient_is_the_mean_of_the_halves():
    sd, batch = R.problem(N)
    net = R.make_net(sd, torch.float64)
    for it in (0, R.BOOST_STEP):
        loss, whole = R.loss_and_grads(net, batch, it, torch.float64)
        halves = [R.loss_and_grads(net, R.rank_rows(batch, r, N), it, torch.float64) for r in range(2)]
        assert abs(float(loss) - 0.5 * (float(halves[0][0]) + float(halves[1][0]))) <= 1e-12 * abs(float(loss))
        for k, want in whole.items():
            got = 0.5 * (halves[0][1][k] + halves[1][1][k])
            assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (it, k)
        # the halves are different problems: the identity is not trivially true
        assert not torch.allclose(halves[0][1]["shared_net.0.weight"], halves[1][1]["shared_net.0.weight"])


@pytest.mark.parametrize("n", [N])
def test_float64_reference_agrees_with_fp32_torch(n):
    ref, f32 = R.reference(n), R.run_steps(n, torch.float32)
    for it, (a, b) in enumerate(zip(ref, f32)):
        assert abs(a["loss"] - b["loss"]) <= 2e-5 * max(1.0, abs(a["loss"]))
        assert abs(a["norm"] - b["norm"]) <= 2e-4 * a["norm"]
        assert a["clipped"] == b["clipped"]
        for k, want in a["grads"].items():
            scale = float(want.abs().max()) + 1e-12
            err = float((b["grads"][k].double() - want).abs().max())
            assert err <= 2e-4 * scale + 1e-9, (k, err, scale)
    # the steps themselves, at the bar of test_adam_clip_step_matches_torch: Adam's first steps move a weight by ~lr sign(g), so
    # an element whose gradient is at rounding level may land anywhere within lr per step
    for it, (a, b) in enumerate(zip(ref, f32)):
        for k, q in a["params"].items():
            err = (b["params"][k].double() - q).abs()
            assert float(err.max()) <= 1.05e-3 * (it + 1), (it, k, float(err.max()))


def test_both_clip_branches_occur():
    for n in (33, 2049):
        ref = R.reference(n)
        print("n = %d: pre-clip norms %s" % (n, ["%.4f" % s["norm"] for s in ref]))
        # the boosted step clips, and some step does not.  (At 2 x 33 rows the first step clips as well: the gradient of 66 rows
        # is noisier than that of 4098, norm 3.93 against 0.57 -- so there the moments of step 0 carry the clip coefficient.)
        assert ref[R.BOOST_STEP]["clipped"] and not all(s["clipped"] for s in ref), [s["norm"] for s in ref]
        assert not ref[R.STEPS - 1]["clipped"]
        # the GPU test holds the kernels' norm to rtol 2e-4: no step may sit so close to the threshold that a norm inside that
        # bar takes the other branch
        assert all(abs(s["norm"] - R.MAX_NORM) > 1e-2 for s in ref), [s["norm"] for s in ref]


def test_reference_moments_after_the_first_step_are_the_clipped_gradient():
    """From zero moments, exp_avg = (1 - beta1) c g and exp_avg_sq = (1 - beta2) (c g)^2 with c the clip coefficient: what the
    GPU test's first-step bars on the moments (gradient bar + norm bar, once for m and twice for v) are derived from."""
    s = R.reference(N)[0]
    c = min(1.0, R.MAX_NORM / (s["norm"] + 1e-6))
    for k, g in s["grads"].items():
        torch.testing.assert_close(s["exp_avg"][k], 0.1 * c * g, rtol=1e-12, atol=0)
        torch.testing.assert_close(s["exp_avg_sq"][k], 0.001 * (c * g) ** 2, rtol=1e-9, atol=0)
