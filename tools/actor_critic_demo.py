#!/usr/bin/env python3
"""An actor-critic loop built from the library's five launches per iteration, on 256 solvable 4x4 levels; prints the share of
episodes won per iteration.

    python tools/actor_critic_demo.py [--shared] [--fused-loss] [--fused-optim] [--curriculum] [--score-every K] [--iterations 60] [--steps 32] [--hidden 32] [--lr 1e-2] [--log FILE]

The critic is a second PolicyNet whose output column 0 is read as V(s) ("a critic without a new kernel"):

    rollout_policy (actor, sample)          -> start, cells, actions, flags        one launch
    trajectory_logits(critic, out)[..., 0]  -> values, read in place (stride 4)    one launch
    trajectory_logits(critic)[0, :, 0]      -> last_value, on the boards as they stand after the rollout    one launch
    trajectory_returns(gamma, lam)          -> adv, ret, mask                       one launch
    trajectory_logits(actor, out)           -> log-probabilities of the played actions; both losses' backward: one launch each

With --shared the actor and the critic are ONE ActorCriticNet: the hidden layer feeds four logits and a
value head of its own, and an iteration is

    rollout_policy (net.policy(), sample)   -> start, cells, actions, flags        one launch
    trajectory_outputs(net, out)            -> logits and values                    one launch
    trajectory_outputs(net)[1][0]           -> last_value                           one launch
    trajectory_returns(gamma, lam)          -> adv, ret, mask                       one launch
    both losses' backward                                                           one launch

The losses are plain torch on [K, N] floats: -(adv * logp(a)) and (v - ret)^2, both over the steps that played a transition.
With --fused-loss they are ONE trajectory_loss() instead (four launches for the loss and its gradient, no
float atomics), with the same hyper-parameters.  The torch path subtracts the advantages' mean; the fused loss has
normalize_adv, which also divides by their standard deviation - so the curve of --fused-loss is NOT comparable line for line
with the one of the torch path.  The torch path stays the default.
With --fused-optim the optimiser is FusedAdam instead of torch.optim.Adam (the update and the zeroing of
the gradients in ONE launch, the step count on the device); it may be combined with --shared --fused-loss.  The last line then
reports the steps it applied and skipped.
With --curriculum the episodes do not start where the levels say: the distance table of the 256 levels is
built once, every board is put on a placement one move from the win (place_at_distance, band [1, 1], set_initial=True, so that
the auto-reset inside a rollout returns there), and before every later iteration the boards that are done get a fresh placement
(only_done=True).  The upper end of the band rises by one whenever the share of episodes won in the last rollout passes 0.8, up to
the median over the levels of their deepest distance.  The share of episodes won is then a share at the CURRENT band: it is not
comparable with the curves that start from the levels' own cells.
With --score-every K the current network is scored every K iterations, before the iteration's rollout, and once after the last
(DESIGN.md section 24): build_policy_table(actor) and score_policy() against the distance table of the 256 levels - the greedy
play of the network from EVERY placement of every level, exactly.  solved, optimal and agreement are shares of the solvable
placements; they depend on neither the start distribution nor the auto-reset nor the step limit of the line they stand on, so
they are comparable between runs and flags.  They score GREEDY play; the rollouts of the loop sample.
No number here is asserted by a test; with --log profiles/actor_critic_demo.log a run is kept.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--gamma", type=float, default=0.97)
    ap.add_argument("--lam", type=float, default=0.9)
    ap.add_argument("--shared", action="store_true", help="one ActorCriticNet with a shared trunk instead of two PolicyNets")
    ap.add_argument("--fused-loss", action="store_true", help="trajectory_loss() instead of the plain-torch losses (normalize_adv for the mean subtraction)")
    ap.add_argument("--fused-optim", action="store_true", help="FusedAdam instead of torch.optim.Adam: update and zero_grad in one launch")
    ap.add_argument("--curriculum", action="store_true", help="start the episodes a band of moves from the win (place_at_distance); the band widens as the win rate passes 0.8")
    ap.add_argument("--score-every", type=int, default=0, metavar="K", help="every K iterations: solved, optimal and agreement shares of the network's greedy play over all placements")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    from tiler_slider_amd import ActorCriticNet, FusedAdam, PolicyNet, RewardWeights, TilerSliderEnvFactory

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.log:
            os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
            open(args.log, "w").write("\n".join(lines) + "\n")

    dev = torch.device("cuda", 0)
    seeds = TilerSliderEnvFactory.solvable_seeds(256, size=4, num_tiles=2, num_obstacles=2, device=dev)
    env = TilerSliderEnvFactory.create_vec_env_from_seeds(seeds, size=4, num_tiles=2, num_obstacles=2, device=dev, max_steps=16, auto_reset=True,
                                                          obs_dtype=None)
    env.reset()
    D = env.onehot_channels * 16
    gen = torch.Generator(device=dev).manual_seed(0)
    Adam = FusedAdam if args.fused_optim else torch.optim.Adam
    if args.shared:
        actor = critic = ActorCriticNet(D, args.hidden, dev, generator=gen)
        opt = Adam(actor.parameters(), lr=args.lr)
    else:
        actor, critic = PolicyNet(D, args.hidden, dev, generator=gen), PolicyNet(D, args.hidden, dev, generator=gen)
        opt = Adam(list(actor.parameters()) + list(critic.parameters()), lr=args.lr)
    weights = RewardWeights(step=-0.01, win=1.0)
    say(f"{'one ActorCriticNet (shared trunk)' if args.shared else 'two PolicyNets'}: 256 solvable 4x4 levels, {args.steps} steps per iteration, H = {args.hidden}, Adam {args.lr}, gamma {args.gamma}, lambda {args.lam}, "
        f"reward {tuple(weights)}{', fused loss (normalize_adv)' if args.fused_loss else ''}{', FusedAdam' if args.fused_optim else ''}")
    # FusedAdam leaves the gradients at zero itself: the first backward creates them, every later one adds to zeros
    zero_grad = (lambda: None) if args.fused_optim else opt.zero_grad
    step = (lambda: opt.step(zero_grad=True)) if args.fused_optim else opt.step
    hi = hi_max = 1
    table = env.build_table() if args.curriculum or args.score_every else None

    def say_score(it):
        score = env.score_policy(env.build_policy_table(actor), table)    # three launches; no state is touched
        say(f"before iteration {it:3d}: over all {int(score.solvable.sum())} solvable placements of the 256 levels, greedy play solves "
            f"{float(score.solved_share):6.3f}, in the least number of moves {float(score.optimal_share):6.3f}, and its move is one of the expert's on "
            f"{float(score.agreement):6.3f}; {int(score.excess.sum())} moves too many in all")

    if args.curriculum:
        start = env.place_at_distance(table, 1, hi, seed=0xC0DE, step_index=0)
        hi_max = max(1, int(start.deepest[start.deepest != 255].float().median()))
        say(f"curriculum: band [1, 1] to start with, {int(start.placed.sum())} of 256 boards placed, its upper end rises up to {hi_max} (the median deepest distance)")
    for it in range(args.iterations):
        if args.score_every and it % args.score_every == 0:
            say_score(it)
        if args.curriculum and it:
            env.place_at_distance(table, 1, hi, seed=0xC0DE, step_index=it, only_done=True)     # fresh starts for the boards that finished
        out = env.rollout_policy(args.steps, actor.policy(), select="sample", seed=it, log=("start", "pos", "act", "flags"))
        if args.shared:
            logits, v = env.trajectory_outputs(actor, out)                      # [K, N, 4] and [K, N], one launch
            with torch.no_grad():
                last = env.trajectory_outputs(actor)[1][0]                      # the boards as they stand after the rollout
        else:
            v = env.trajectory_logits(critic, out)[..., 0]                      # [K, N], strides (4 N, 4): read in place below
            with torch.no_grad():
                last = env.trajectory_logits(critic)[0, :, 0].contiguous()      # the boards as they stand after the rollout
        tr = env.trajectory_returns(out, args.gamma, args.lam, values=v, last_value=last, reward=weights)
        if args.fused_loss:
            info = env.trajectory_loss(logits if args.shared else env.trajectory_logits(actor, out), out, tr, values=v.contiguous(),
                                       value_coef=0.5, normalize_adv=True)
            actor_loss, critic_loss = info.policy, info.value
            zero_grad()
            info.loss.backward()
        else:
            live = tr.mask.float()
            count = live.sum().clamp(min=1)
            adv = (tr.adv - (tr.adv * live).sum() / count) * live
            logp = torch.log_softmax(logits if args.shared else env.trajectory_logits(actor, out), dim=2)
            played = logp.gather(2, out.act_log.clamp(max=3).long().unsqueeze(2)).squeeze(2)
            actor_loss = -(adv * played).sum() / count
            critic_loss = (((v - tr.ret) ** 2) * live).sum() / count
            zero_grad()
            (actor_loss + 0.5 * critic_loss).backward()
        step()
        share = float(out.wins.sum()) / max(1.0, float(out.finished.sum()))
        say(f"iteration {it:3d}: episodes won {share:6.3f} ({int(out.wins.sum())} of {int(out.finished.sum())}), actor loss {float(actor_loss):8.4f}, "
            f"critic loss {float(critic_loss):8.4f}" + (f", band [1, {hi}]" if args.curriculum else ""))
        if args.curriculum and share > 0.8 and hi < hi_max:
            hi += 1
    if args.score_every:
        say_score(args.iterations)
    if args.fused_optim:
        say(f"FusedAdam: {int(opt.steps_applied)} steps applied, {int(opt.steps_skipped)} skipped, last gradient norm {float(opt.grad_norm):.4f}")


if __name__ == "__main__":
    main()
