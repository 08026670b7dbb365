"""PPO self-play with everything between the env and the optimiser on the device.

    python -m splendor_gym.scripts.ppo_device --num-envs 65536 --num-steps 128 --total-timesteps 100000000

The loop of the reference's ppo_splendor.py with its argument names where they apply: rollouts of
DualStepVectorEnv against an OpponentPool (current policy with --p-current, else one of --pool-size
snapshots, drawn per episode), the agent's forward fused (FusedActorCritic), the trajectory in a
PPORolloutStore, GAE on the device, the update in torch (splendor_gym.ppo; --fused-loss: its loss head
as one device call; --device-adam: the norm clip, the Adam step and the target-KL stop as one device call
per minibatch, so that an update reads the device once; --device-nets: the two networks' forward and
backward passes as device calls too, a minibatch then being four device calls; --tiled-nets on | auto: those
passes by the LDS-tiled matrix-core kernels built for minibatches of tens of thousands of rows, always or
from DeviceNets.TILED_MIN_ROWS rows upward, with the same bytes either way; --net-operands bf16: those
passes with bf16 operands on the matrix cores at every minibatch size, float32 accumulation and master
weights, which is another run: its numbers differ; --device-permutation: each epoch's permutation drawn on the
device by splendor_gym.ppo.DevicePermutation seeded with --seed instead of torch.randperm, another permutation and
so another run; --graph-update: the whole update, every epoch's draw and every minibatch, captured once and
replayed as one hipGraph, which implies --device-permutation, --device-adam and --device-nets and gives the
numbers of those three without it).  After each update the
fused agent and the pool re-pack the new weights; every --snapshot-every-updates updates the pool takes
a snapshot.  --eval-every-updates N evaluates before training and every N updates, --eval-games games
against each of random, greedy_v1, basic, the agent itself and greedy_v2 in one batch on the device
(splendor_gym.evaluation.DeviceEvaluator), one line per opponent.  Logging to tensorboard and plots are
the reference scripts' business.
"""
import argparse
import time


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--total-timesteps", type=int, default=1_000_000)
    p.add_argument("--num-envs", type=int, default=4096)
    p.add_argument("--num-steps", type=int, default=128)
    p.add_argument("--gamma", type=float, default=0.999)
    p.add_argument("--gae-lambda", type=float, default=0.95)
    p.add_argument("--lr", type=float, default=2.5e-4)
    p.add_argument("--ent-coef", type=float, default=0.03)
    p.add_argument("--ent-coef-final", type=float, default=0.01)
    p.add_argument("--vf-coef", type=float, default=0.5)
    p.add_argument("--clip-coef", type=float, default=0.2)
    p.add_argument("--vclip", type=float, default=0.2)
    p.add_argument("--update-epochs", type=int, default=4)
    p.add_argument("--minibatch-size", type=int, default=256)
    p.add_argument("--target-kl", type=float, default=0.02)
    p.add_argument("--lr-anneal", action="store_true")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--pool-size", type=int, default=12)
    p.add_argument("--snapshot-every-updates", type=int, default=10)
    p.add_argument("--p-current", type=float, default=0.25)
    p.add_argument("--save-path", type=str, default="")
    p.add_argument("--load-path", type=str, default="", help="a state_dict (.pt) or .safetensors to start from")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--entropy-bonus", action="store_true",
                   help="subtract the entropy term (the usual PPO bonus); default: the reference's sign (ppo_update)")
    p.add_argument("--fused-loss", action="store_true",
                   help="the update's loss head as one device call (PPORolloutStore.loss) instead of torch elementwise ops")
    p.add_argument("--device-adam", action="store_true",
                   help="the optimiser on the device (splendor_gym.ppo.DeviceAdam) instead of torch.optim.Adam: no per-minibatch "
                        "read-back; a minibatch behind the target-KL crossing is computed and then skipped")
    p.add_argument("--device-nets", action="store_true",
                   help="the two networks' forward and backward passes of the update as device calls "
                        "(splendor_gym.ppo.DeviceNets) instead of torch autograd; implies --fused-loss")
    p.add_argument("--tiled-nets", choices=("off", "auto", "on"), default="off",
                   help="DeviceNets' passes on the tiled matrix-core kernels: on always, auto from DeviceNets.TILED_MIN_ROWS "
                        "rows a minibatch upward; the same bytes as off; auto and on imply --device-nets")
    p.add_argument("--net-operands", choices=("f32", "bf16"), default="f32",
                   help="DeviceNets' matrix products: f32, or bf16 operands with float32 accumulation and float32 master "
                        "weights (mixed precision: the numbers of the run change); bf16 implies --device-nets")
    p.add_argument("--device-permutation", action="store_true",
                   help="draw each epoch's permutation on the device (splendor_gym.ppo.DevicePermutation, seeded with --seed) "
                        "instead of torch.randperm: another permutation, so another run")
    p.add_argument("--graph-update", action="store_true",
                   help="capture one whole update (every epoch's permutation and every minibatch) as one hipGraph and replay "
                        "it; implies --device-permutation, --device-adam and --device-nets; --no-graph runs it eagerly")
    p.add_argument("--no-graph", action="store_true",
                   help="run every rollout (and with --graph-update every update) eagerly instead of replaying a hipGraph")
    p.add_argument("--eval-every-updates", type=int, default=0,
                   help="evaluate before training and every N updates (0: never), as ppo_splendor.py does")
    p.add_argument("--eval-games", type=int, default=400, help="games per opponent kind of one evaluation")
    args = p.parse_args(argv)
    args.device_nets = args.device_nets or args.tiled_nets != "off" or args.net_operands != "f32" or args.graph_update
    args.device_adam = args.device_adam or args.graph_update
    args.device_permutation = args.device_permutation or args.graph_update

    import torch
    from ..fused_policy import FusedActorCritic, OpponentPool
    from ..policy import ActorCritic
    from ..ppo import DeviceAdam, DeviceNets, DevicePermutation, PPORolloutStore, collect, ppo_update
    from ..selfplay import DualStepVectorEnv

    dev = torch.device(args.device)
    torch.cuda.set_device(dev)
    torch.manual_seed(args.seed)
    agent = ActorCritic().to(dev)
    if args.load_path.endswith(".safetensors"):
        from safetensors.torch import load_file
        agent.load_state_dict(load_file(args.load_path, device=str(dev)))
    elif args.load_path:
        agent.load_state_dict(torch.load(args.load_path, map_location=dev))
    if args.device_adam:
        optimizer = DeviceAdam(agent.parameters(), lr=args.lr, eps=1e-5, target_kl=args.target_kl)
    else:
        optimizer = torch.optim.Adam(agent.parameters(), lr=args.lr, eps=1e-5)
    nets = DeviceNets(agent, tiled={"off": False, "auto": "auto", "on": True}[args.tiled_nets],
                      operands=args.net_operands) if args.device_nets else False
    agent_k = FusedActorCritic(agent)
    pool =OpponentPool(agent, pool_size=args.pool_size, p_current=args.p_current, seed=args.seed)
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    env = DualStepVectorEnv(args.num_envs, device=dev, opponent=pool, opponent_obs=False, step_counter=counter,
                            agent_obs_u8=True)
    store = PPORolloutStore(args.num_steps, args.num_envs, dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    perm = DevicePermutation(args.num_steps * args.num_envs, args.minibatch_size, dev, seed=args.seed) \
        if args.device_permutation else None
    obs, info = env.reset(seed=args.seed)
    mask = info["action_mask"]
    batch = args.num_envs * args.num_steps
    num_updates = max(1, args.total_timesteps // batch)
    evaluator = None
    if args.eval_every_updates > 0:
        from ..evaluation import DeviceEvaluator
        # run_evaluation_suite's opponents in its order (group g plays seed + g), greedy_v2 after them
        evaluator = DeviceEvaluator(args.eval_games, opponents=("random", "greedy_v1", "basic", "self_play", "greedy_v2"),
                                    device=dev, policy_seed=args.seed, graph=not args.no_graph)

    def evaluate(update_seed, steps):
        print(f"evaluation at step {steps} ({args.eval_games} games per opponent)", flush=True)
        for name, r in evaluator.run(agent_k, seed=update_seed).items():
            print(f"  eval vs {name}: win_rate {r['win_rate']:.3f} +- {r['win_rate_ci95']:.3f} "
                  f"avg_turns {r['avg_turns']:.1f} avg_prestige {r['avg_prestige']:.2f} "
                  f"illegal_action_rate {r['illegal_action_rate']:.4f}", flush=True)

    if evaluator is not None:
        evaluate(0, 0)  # ppo_splendor.py:195-197
    t0 = time.time()
    for update in range(num_updates):
        if args.lr_anneal and args.device_adam:
            optimizer.set_lr(args.lr * (1.0 - update / num_updates))
        elif args.lr_anneal:
            optimizer.param_groups[0]["lr"] = args.lr * (1.0 - update / num_updates)
        obs, mask = collect(env, agent_k, store, obs, mask, seed=args.seed, graph=not args.no_graph)
        store.compute_gae(gamma=args.gamma, gae_lambda=args.gae_lambda)
        progress = update / max(1, num_updates - 1)
        res = ppo_update(agent, optimizer, store, clip_coef=args.clip_coef, vclip=args.vclip,
                         ent_coef=args.ent_coef + (args.ent_coef_final - args.ent_coef) * progress,
                         vf_coef=args.vf_coef, update_epochs=args.update_epochs, minibatch_size=args.minibatch_size,
                         target_kl=args.target_kl, generator=gen, entropy_bonus=args.entropy_bonus,
                         fused_loss=args.fused_loss, device_nets=nets, permutation=perm,
                         graph=args.graph_update and not args.no_graph)
        agent_k.refresh()
        pool.refresh()
        if (update + 1) % max(1, args.snapshot_every_updates) == 0:
            pool.add_snapshot()
        if args.save_path:
            torch.save(agent.state_dict(), args.save_path)
        steps = (update + 1) * batch
        print(f"update {update + 1}/{num_updates} steps {steps} sps {steps / (time.time() - t0):.0f} "
              f"reward/step {float(store.reward.mean()):+.5f} episodes {int(store.done.sum())} "
              f"pl {res['policy_loss']:+.4f} vl {res['value_loss']:.4f} ent {res['entropy']:.3f} "
              f"kl {res['approx_kl']:+.5f} opt-steps {res['optimizer_steps']}", flush=True)
        if evaluator is not None and (update + 1) % args.eval_every_updates == 0:
            evaluate(update, steps)  # ppo_splendor.py:382-388, on the refreshed agent_k
    if evaluator is not None:
        evaluator.close()
    env.close()


if __name__ == "__main__":
    main()
