"""Timings of the PPO rollout store (splendor_gym/ppo.py) at the size the engine exists for.

    python tools/bench_ppo.py [--tables 65536] [--steps 128] [--repeats 7] [--loss-json FILE] [--adam-json FILE] [--adam-only]
                                [--nets-json FILE] [--nets-only] [--graph-json FILE] [--graph-only]

Prints one JSON line with five comparisons, each arm timed with device events, the arms alternating,
medians reported:
  1. record: a hipGraph of `steps` config-5 dual steps (tools/bench_selfplay.py's loop: fused fp32 actor,
     opponent pool of 12 trained snapshots) without and with the store's record launches and with the
     actor writing straight into the store's rows; and the record launches alone.
  2. gae: spl_ppo_gae beside the same recurrence as a torch loop over [T] rows on the device (the
     loop's result is compared bit for bit with the kernel's); back to back over the same planes, and once
     per window after 1 GiB of other stores.
  3. gather: spl_ppo_gather at B = 256 and B = 65 536 beside index_select plus the torch expansion.
  4. loss: PPORolloutStore.loss (spl_ppo_loss) beside the torch loss head of ppo_update, forward and backward
     from leaf logits / value tensors, at B = 256 and B = 65 536.
  5. adam: DeviceAdam.step (spl_ppo_adam) beside clip_grad_norm_ + torch.optim.Adam.step + zero_grad (torch's
     default and, where the installed torch takes it, fused=True) on the trained agent with one real minibatch's
     gradients; and one whole ppo_update(fused_loss=True, target_kl=0.02) with either optimiser, timed with
     the host clock, at the reference's shape (128 steps x 16 tables, minibatch 256, 4 epochs) and at 128 x
     4 096 with minibatch 65 536.  It builds its own small stores; --adam-only runs nothing else.
  6. nets (--nets-only, not part of the default run): DeviceNets.forward + backward (spl_ppo_net_forward /
     spl_ppo_net_backward), DeviceNets(tiled=True) (spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled)
     and DeviceNets(operands="bf16") (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16, other numbers)
     beside store.gather + the two torch networks + torch.autograd.backward for fixed dlogits / dvalue, at
     B = 256, 4 096, 16 384 and 65 536; and one whole ppo_update(fused_loss=True, target_kl=0.02) with
     DeviceAdam without device_nets, with them, with the tiled ones and with the bf16 ones, at the same two
     shapes as in 5 (--nets-json profiles/ppo/bench_ppo_nets_bf16.json keeps the section).
  7. graph (--graph-only, not part of the default run): one whole ppo_update with DeviceAdam and DeviceNets, target
     KL 0.02, 4 epochs, eager with torch.randperm, eager with a DevicePermutation and as the replayed graph
     (ppo_update(graph=True)), at 128 x 16 with minibatch 256 (the 8-row f32 passes) and at 128 x 4 096 with
     minibatch 65 536 (tiled="auto", and again with operands="bf16"), host clock; and spl_ppo_permute alone at
     n = 2 048, 524 288 and 8 388 608 (--graph-json profiles/ppo/bench_ppo_graph.json keeps the section).
Bytes are the algorithmic bytes each kernel has to move, computed from the shapes below.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "splendor-gym_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pool-size", type=int, default=12)
    ap.add_argument("--loss-json", default="", help="also write the loss section to this file (profiles/ppo/bench_ppo_loss.json)")
    ap.add_argument("--adam-json", default="", help="also write the optimiser section to this file (profiles/ppo/bench_ppo_adam.json)")
    ap.add_argument("--adam-only", action="store_true", help="run the optimiser section alone")
    ap.add_argument("--nets-json", default="", help="also write the network section to this file (profiles/ppo/bench_ppo_nets_bf16.json)")
    ap.add_argument("--nets-only", action="store_true", help="run the network-pass section alone")
    ap.add_argument("--graph-json", default="", help="also write the graph section to this file (profiles/ppo/bench_ppo_graph.json)")
    ap.add_argument("--graph-only", action="store_true", help="run the whole-update-as-one-graph section alone")
    args = ap.parse_args()

    import torch
    from safetensors.torch import load_file
    from splendor_gym.fused_policy import FusedActorCritic, OpponentPool
    from splendor_gym.policy import ActorCritic
    from splendor_gym.ppo import PPORolloutStore
    from splendor_gym.selfplay import DualStepVectorEnv

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    T, K = args.tables, args.steps
    ckpt = os.path.join(REPO, "tests", "golden", "ppo_splendor_latest.safetensors")

    def net():
        m = ActorCritic().to(dev).eval()
        m.load_state_dict(load_file(ckpt, device=str(dev)))
        return m

    def timed(arms, inner=1, repeats=args.repeats, before=None, spread=None):
        """median milliseconds per call of each arm (`inner` back-to-back calls per timed window), the arms
        alternating; one untimed call of each first; `before` runs ahead of every timed window; `spread`, a
        dictionary, takes each arm's (fastest, slowest) window"""
        for fn in arms.values():
            fn()
        torch.cuda.synchronize(dev)
        ms = {name: [] for name in arms}
        for _ in range(repeats):
            for name, fn in arms.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if before is not None:
                    before()
                a.record()
                for _ in range(inner):
                    fn()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b) / inner)
        if spread is not None:
            spread.update({name: (min(v), max(v)) for name, v in ms.items()})
        return {name: statistics.median(v) for name, v in ms.items()}

    # ---- 5. the optimiser step (defined here, run last; --adam-only runs nothing else) --------------
    def adam_section():
        import copy
        import time
        from splendor_gym.ppo import DeviceAdam, collect, ppo_update

        def collected(tables, steps):
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
            e = DualStepVectorEnv(tables, device=dev, opponent="random", policy_seed=3, opponent_obs=False,
                                  step_counter=counter, agent_obs_u8=True)
            obs, info = e.reset(seed=40)
            s = PPORolloutStore(steps, tables, dev)
            collect(e, FusedActorCritic(trained), s, obs, info["action_mask"], seed=5)
            s.compute_gae()
            e.close()
            return s

        trained = net()
        # (1) the step alone, on the gradients of one real minibatch of 256 positions
        big = collected(4096, 128)
        idx = next(iter(big.minibatches(256, torch.Generator(device=dev).manual_seed(0))))
        obs = big.gather(idx)["obs"]
        probe = copy.deepcopy(trained)
        big.loss(idx, probe.actor(obs), probe.critic(obs))[0].backward()
        grads = [p.grad.clone() for p in probe.parameters()]
        arms, notes = {}, {}

        def torch_arm(**kw):
            a = copy.deepcopy(trained)
            params = list(a.parameters())
            opt = torch.optim.Adam(params, lr=2.5e-4, eps=1e-5, **kw)
            own = [g.clone() for g in grads]

            def run():
                for p, g in zip(params, own):
                    p.grad = g
                torch.nn.utils.clip_grad_norm_(params, 0.5)
                opt.step()
                opt.zero_grad()
            return run

        arms["torch"] = torch_arm()
        try:
            fused = torch_arm(fused=True)
            fused()
            arms["torch_fused"] = fused
        except Exception as exc:  # the installed torch does not take fused=True on this device
            notes["torch_fused"] = f"not accepted: {type(exc).__name__}: {exc}"
        a_dev = copy.deepcopy(trained)
        p_dev = list(a_dev.parameters())
        dev_opt = DeviceAdam(p_dev, lr=2.5e-4, eps=1e-5, max_grad_norm=0.5)

        def device_arm():
            for p, g in zip(p_dev, grads):
                p.grad = g
            dev_opt.step()

        arms["device"] = device_arm
        ms = timed(arms, inner=100)
        floats = sum(p.numel() for p in p_dev)
        step = {f"{name}_us": round(v * 1e3, 2) for name, v in ms.items()}
        step.update(notes)
        step.update({"floats": floats, "tensors": len(p_dev), "bytes_device": floats * 4 * (1 + 4 + 3),
                     "ratio_torch_over_device": round(ms["torch"] / ms["device"], 2),
                     "note": "clip_grad_norm_(0.5) + Adam.step + zero_grad() beside DeviceAdam.step (spl_ppo_adam: two launches), "
                             "the agent's 12 tensors, gradients of one minibatch of 256; device events around 100 back-to-back "
                             "calls, arms alternating, medians; bytes_device: the gradients once for the norm, then parameters, "
                             "gradients and both moments in, parameters and both moments out"})
        if "torch_fused" in ms:
            step["ratio_torch_fused_over_device"] = round(ms["torch_fused"] / ms["device"], 2)

        # (2) one whole ppo_update(fused_loss=True), host clock around it and a synchronise, target_kl 0.02
        def update_arms(store, minibatch):
            out = {}

            def arm(device_adam):
                def run():
                    a = copy.deepcopy(trained)
                    make = DeviceAdam if device_adam else torch.optim.Adam
                    opt = make(list(a.parameters()), lr=2.5e-4, eps=1e-5)
                    gen = torch.Generator(device=dev).manual_seed(0)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    res = ppo_update(a, opt, store, update_epochs=4, minibatch_size=minibatch, target_kl=0.02, generator=gen,
                                     fused_loss=True)
                    torch.cuda.synchronize(dev)
                    return (time.perf_counter() - t0) * 1e3, res
                return run

            runs = {"torch_adam": arm(False), "device_adam": arm(True)}
            for fn in runs.values():
                fn()
            times, last = {k: [] for k in runs}, {}
            for _ in range(args.repeats):
                for name, fn in runs.items():
                    t, last[name] = fn()
                    times[name].append(t)
            total = store.num_steps * store.num_envs
            per_epoch = -(-total // minibatch)
            for name in runs:
                out[f"{name}_ms"] = round(statistics.median(times[name]), 3)
                out[f"{name}_optimizer_steps"] = last[name]["optimizer_steps"]
            out.update({"ratio_torch_over_device": round(out["torch_adam_ms"] / out["device_adam_ms"], 3),
                        "minibatches_run_torch_adam": "stops each epoch at the crossing",
                        "minibatches_run_device_adam": 4 * per_epoch, "gated": last["device_adam"]["gated"],
                        "K": store.num_steps, "T": store.num_envs, "minibatch": minibatch, "epochs": 4})
            return out

        updates = {"reference_shape": update_arms(collected(16, 128), 256), "large": update_arms(big, 65536)}
        updates["note"] = ("one ppo_update(fused_loss=True, target_kl=0.02) from the trained checkpoint, host clock from the call to "
                           "a device synchronise behind it, arms alternating, medians; torch_adam: clip_grad_norm_, "
                           "torch.optim.Adam and a KL read-back per minibatch (the path before DeviceAdam, unchanged); device_adam: "
                           "DeviceAdam.step per minibatch, one read-back per update, every minibatch computed")
        section = {"step": step, "ppo_update": updates}
        if args.adam_json:
            with open(args.adam_json, "w") as f:
                json.dump({"metric": "PPO optimiser step (spl_ppo_adam) and whole updates, one MI355X", "repeats": args.repeats,
                           "adam": section}, f, indent=1)
                f.write("\n")
        return section

    # ---- 6. the network passes (--nets-only runs nothing else) --------------------------------------
    def nets_section():
        import copy
        import time
        from splendor_gym.ppo import DeviceAdam, DeviceNets, collect, ppo_update

        trained = net()

        def collected(tables, steps):
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
            e = DualStepVectorEnv(tables, device=dev, opponent="random", policy_seed=3, opponent_obs=False,
                                  step_counter=counter, agent_obs_u8=True)
            obs, info = e.reset(seed=40)
            s = PPORolloutStore(steps, tables, dev)
            collect(e, FusedActorCritic(trained), s, obs, info["action_mask"], seed=5)
            s.compute_gae()
            e.close()
            return s

        big = collected(4096, 128)
        gen = torch.Generator(device=dev).manual_seed(0)
        passes = {}
        for B in (256, 4096, 16384, 65536):
            idx = torch.randperm(big.num_steps * big.num_envs, device=dev, generator=gen)[:B].contiguous()
            dlogits = torch.randn(B, 45, device=dev, generator=gen) / B
            dvalue = torch.randn(B, device=dev, generator=gen) / B
            a_dev, a_ref, a_tiled, a_bf16 = (copy.deepcopy(trained) for _ in range(4))
            nets, tiled, bf16 = DeviceNets(a_dev), DeviceNets(a_tiled, tiled=True), DeviceNets(a_bf16, operands="bf16")
            ref_params = list(a_ref.parameters())

            def device_arm():
                nets.forward(big, idx)
                nets.backward(big, idx, dlogits, dvalue)

            def tiled_arm():
                tiled.forward(big, idx)
                tiled.backward(big, idx, dlogits, dvalue)

            def bf16_arm():
                bf16.forward(big, idx)
                bf16.backward(big, idx, dlogits, dvalue)

            def torch_arm():
                for p in ref_params:
                    p.grad = None
                obs = big.gather(idx)["obs"]
                torch.autograd.backward([a_ref.actor(obs), a_ref.critic(obs)], [dlogits, dvalue.view(B, 1)])

            spread = {}
            ms = timed({"device": device_arm, "torch": torch_arm, "tiled": tiled_arm, "bf16": bf16_arm}, inner=100, spread=spread)
            rel = lambda xs, ys: float(torch.sqrt(sum(((x.grad - y.grad).double() ** 2).sum() for x, y in zip(xs, ys)) /
                                                  sum((y.grad.double() ** 2).sum() for y in ys)))
            same = all(torch.equal(p.grad.view(torch.int32), q.grad.view(torch.int32))
                       for p, q in zip(a_dev.parameters(), a_tiled.parameters()))
            diff = max(float((p.grad - q.grad).abs().max()) for p, q in zip(a_dev.parameters(), ref_params))
            scale = max(float(q.grad.abs().max()) for q in ref_params)
            passes[f"B{B}"] = {"device_us": round(ms["device"] * 1e3, 1), "torch_us": round(ms["torch"] * 1e3, 1),
                               "tiled_us": round(ms["tiled"] * 1e3, 1), "bf16_us": round(ms["bf16"] * 1e3, 1),
                               "tiled_us_fastest_slowest": [round(x * 1e3, 1) for x in spread["tiled"]],
                               "bf16_us_fastest_slowest": [round(x * 1e3, 1) for x in spread["bf16"]],
                               "ratio_tiled_over_bf16": round(ms["tiled"] / ms["bf16"], 2),
                               "bf16_gradients_relative_l2_to_tiled": rel(list(a_bf16.parameters()), list(a_tiled.parameters())),
                               "ratio_torch_over_device": round(ms["torch"] / ms["device"], 2),
                               "ratio_torch_over_tiled": round(ms["torch"] / ms["tiled"], 2),
                               "ratio_device_over_tiled": round(ms["device"] / ms["tiled"], 2),
                               "faster": min(ms, key=ms.get), "tiled_gradients_equal_device_bytes": same,
                               "max_abs_gradient_difference_to_torch": diff, "max_abs_gradient": scale}
        passes["note"] = ("forward and backward of both networks for B store positions, fixed dlogits / dvalue: DeviceNets.forward + "
                          "backward (spl_ppo_net_forward: 1 launch, spl_ppo_net_backward: 3) and the same with tiled=True "
                          "(spl_ppo_net_forward_tiled: 3 launches, spl_ppo_net_backward_tiled: 4) "
                          "and DeviceNets(operands=\"bf16\") (spl_ppo_net_forward_bf16: 3 launches, spl_ppo_net_backward_bf16: 4; "
                          "bf16 operands on the matrix cores, other numbers) beside store.gather + actor + critic + "
                          "torch.autograd.backward from cleared gradients; device events around 100 back-to-back iterations, arms "
                          "alternating, medians")

        def update_arms(store, minibatch):
            def arm(device_nets):
                def run():
                    a = copy.deepcopy(trained)
                    opt = DeviceAdam(list(a.parameters()), lr=2.5e-4, eps=1e-5)
                    nets = False
                    if device_nets:
                        nets = DeviceNets(a, tiled=device_nets == "tiled", operands="bf16" if device_nets == "bf16" else "f32")
                    g = torch.Generator(device=dev).manual_seed(0)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    res = ppo_update(a, opt, store, update_epochs=4, minibatch_size=minibatch, target_kl=0.02, generator=g,
                                     fused_loss=True, device_nets=nets)
                    torch.cuda.synchronize(dev)
                    return (time.perf_counter() - t0) * 1e3, res
                return run

            runs = {"torch_nets": arm(False), "device_nets": arm(True), "tiled_nets": arm("tiled"), "bf16_nets": arm("bf16")}
            for fn in runs.values():
                fn()
            times, last = {k: [] for k in runs}, {}
            for _ in range(args.repeats):
                for name, fn in runs.items():
                    t, last[name] = fn()
                    times[name].append(t)
            out = {}
            for name in runs:
                out[f"{name}_ms"] = round(statistics.median(times[name]), 3)
                out[f"{name}_ms_fastest_slowest"] = [round(min(times[name]), 3), round(max(times[name]), 3)]
                out[f"{name}_optimizer_steps"] = last[name]["optimizer_steps"]
            total = store.num_steps * store.num_envs
            out.update({"ratio_torch_over_device": round(out["torch_nets_ms"] / out["device_nets_ms"], 3),
                        "ratio_torch_over_tiled": round(out["torch_nets_ms"] / out["tiled_nets_ms"], 3),
                        "ratio_tiled_over_bf16": round(out["tiled_nets_ms"] / out["bf16_nets_ms"], 3),
                        "faster": min(runs, key=lambda name: out[f"{name}_ms"]),
                        "minibatches_run": 4 * -(-total // minibatch), "K": store.num_steps, "T": store.num_envs,
                        "minibatch": minibatch, "epochs": 4})
            return out

        updates = {"reference_shape": update_arms(collected(16, 128), 256), "large": update_arms(big, 65536)}
        updates["note"] = ("one ppo_update(fused_loss=True, target_kl=0.02) with DeviceAdam from the trained checkpoint, without "
                           "device_nets, with them, with DeviceNets(tiled=True) and with DeviceNets(operands=\"bf16\") (a DeviceNets built outside the clock, as the optimiser is), host clock from the call to "
                           "a device synchronise behind it, arms alternating, medians")
        section = {"passes": passes, "ppo_update": updates}
        if args.nets_json:
            with open(args.nets_json, "w") as f:
                json.dump({"metric": "PPO network passes (spl_ppo_net_forward / spl_ppo_net_backward, their _tiled and their _bf16 forms) and whole updates, one MI355X",
                           "repeats": args.repeats, "nets": section}, f, indent=1)
                f.write("\n")
        return section

    # ---- 7. one update as one replayed graph (--graph-only runs nothing else) ------------------------
    def graph_section():
        import copy
        import time
        from splendor_gym.ppo import DeviceAdam, DeviceNets, DevicePermutation, collect, ppo_update

        trained = net()

        def collected(tables, steps):
            counter = torch.zeros(1, dtype=torch.int64, device=dev)
            e = DualStepVectorEnv(tables, device=dev, opponent="random", policy_seed=3, opponent_obs=False,
                                  step_counter=counter, agent_obs_u8=True)
            obs, info = e.reset(seed=40)
            s = PPORolloutStore(steps, tables, dev)
            collect(e, FusedActorCritic(trained), s, obs, info["action_mask"], seed=5)
            s.compute_gae()
            e.close()
            return s

        def update_arms(store, minibatch, **nets_kw):
            total = store.num_steps * store.num_envs

            def arm(permutation, graph):
                # the objects live from update to update, as a training run's do; every timed update starts from the
                # checkpoint, zero moments and draw counter 0, restored outside the clock, so that every window of an
                # arm does the same work and the two device-permutation arms the same arithmetic
                a = copy.deepcopy(trained)
                opt = DeviceAdam(list(a.parameters()), lr=2.5e-4, eps=1e-5)
                nets = DeviceNets(a, **nets_kw)
                perm = DevicePermutation(total, minibatch, dev, seed=0) if permutation else None

                def run():
                    with torch.no_grad():
                        for p, q in zip(a.parameters(), trained.parameters()):
                            p.copy_(q)
                    opt._exp_avg.zero_()
                    opt._exp_avg_sq.zero_()
                    opt._set("step", 0, integer=True)
                    if perm is not None:
                        perm.set_counter(0)
                    g = torch.Generator(device=dev).manual_seed(0)
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    res = ppo_update(a, opt, store, update_epochs=4, minibatch_size=minibatch, target_kl=0.02, generator=g,
                                     device_nets=nets, permutation=perm, graph=graph)
                    torch.cuda.synchronize(dev)
                    return (time.perf_counter() - t0) * 1e3, res
                return run

            runs = {"eager_randperm": arm(False, False), "eager_device_permutation": arm(True, False),
                    "graph": arm(True, True)}
            for fn in runs.values():  # the graph arm's first call is its eager run and the capture
                fn()
            times, last = {k: [] for k in runs}, {}
            for _ in range(args.repeats):
                for name, fn in runs.items():
                    t, last[name] = fn()
                    times[name].append(t)
            out = {}
            for name in runs:
                out[f"{name}_ms"] = round(statistics.median(times[name]), 3)
                out[f"{name}_ms_fastest_slowest"] = [round(min(times[name]), 3), round(max(times[name]), 3)]
                out[f"{name}_optimizer_steps"] = last[name]["optimizer_steps"]
                out[f"{name}_gated"] = last[name]["gated"]
            same = all(last["graph"][k] == last["eager_device_permutation"][k] for k in last["graph"])
            out.update({"ratio_eager_randperm_over_graph": round(out["eager_randperm_ms"] / out["graph_ms"], 3),
                        "ratio_eager_device_permutation_over_graph": round(out["eager_device_permutation_ms"] / out["graph_ms"], 3),
                        "faster": min(runs, key=lambda name: out[f"{name}_ms"]), "graph_result_equals_eager_device_permutation": same,
                        "replays": store._update_replays, "minibatches_run": 4 * -(-total // minibatch),
                        "K": store.num_steps, "T": store.num_envs, "minibatch": minibatch, "epochs": 4,
                        "nets": {"tiled": nets_kw.get("tiled", False), "operands": nets_kw.get("operands", "f32")}})
            return out

        big = collected(4096, 128)
        updates = {"reference_shape": update_arms(collected(16, 128), 256),
                   "large": update_arms(big, 65536, tiled="auto"),
                   "large_bf16": update_arms(big, 65536, tiled="auto", operands="bf16")}
        updates["note"] = ("one ppo_update(device_nets=DeviceNets, target_kl=0.02, 4 epochs) with DeviceAdam from the trained checkpoint: "
                           "eager over torch.randperm, eager over a DevicePermutation, and ppo_update(graph=True) replaying its "
                           "capture; the objects are built once per arm and every timed update starts from the checkpoint with zero "
                           "moments, restored outside the clock; host clock from the call to a device synchronise behind it (the "
                           "result dictionary's read-back included), arms alternating in one process, medians")
        permute = {}
        for n, B in ((2048, 256), (524288, 65536), (8388608, 65536)):
            perm = DevicePermutation(n, B, dev, seed=0)
            spread = {}
            ms = timed({"permute": perm.draw}, inner=100 if n <= 524288 else 20, spread=spread)
            permute[f"n{n}"] = {"us": round(ms["permute"] * 1e3, 2), "us_fastest_slowest": [round(x * 1e3, 2) for x in spread["permute"]],
                                "B": B, "bytes": perm.rows * perm.stride * 8,
                                "GBps": round(perm.rows * perm.stride * 8 / (ms["permute"] * 1e-3) / 1e9, 1)}
        permute["note"] = ("DevicePermutation.draw (spl_ppo_permute: the permutation's launch and the one-thread launch that advances "
                           "the counter), device events around back-to-back eager calls, medians; bytes: the int64 words written")
        section = {"ppo_update": updates, "permute": permute}
        if args.graph_json:
            with open(args.graph_json, "w") as f:
                json.dump({"metric": "one PPO update as one replayed graph (ppo_update(graph=True)) beside the eager update, and "
                                     "spl_ppo_permute, one MI355X", "repeats": args.repeats, "graph": section}, f, indent=1)
                f.write("\n")
        return section

    if args.graph_only:
        print(json.dumps({"metric": "one PPO update as one replayed graph, one MI355X", "repeats": args.repeats,
                          "graph": graph_section()}))
        return

    if args.nets_only:
        print(json.dumps({"metric": "PPO network passes, one MI355X", "repeats": args.repeats, "nets": nets_section()}))
        return

    if args.adam_only:
        print(json.dumps({"metric": "PPO optimiser step, one MI355X", "repeats": args.repeats, "adam": adam_section()}))
        return

    # ---- 1. the dual step without and with recording ---------------------------------------------
    agent = net()
    agent_k = FusedActorCritic(agent)
    pool = OpponentPool(agent, pool_size=args.pool_size, p_current=0.25, seed=99)
    for _ in range(args.pool_size):
        pool.add_snapshot(net())
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    env = DualStepVectorEnv(T, device=dev, opponent=pool, opponent_obs=False, step_counter=counter, agent_obs_u8=True)
    _, info = env.reset(seed=0)
    mask = info["action_mask"]
    store = PPORolloutStore(K, T, dev)
    plain_out = {"action": torch.empty(T, dtype=torch.int32, device=dev), "logprob": torch.empty(T, device=dev),
                 "entropy": torch.empty(T, device=dev), "value": torch.empty(T, 1, device=dev)}

    def rollout(record):
        m = mask
        for k in range(K):
            if record:
                store.record_pre(k, env.agent_obs_u8, m)
            a = agent_k.act(env.agent_obs_u8, m, seed=1234, ply_base=counter, out=store.row(k) if record else plain_out)[0]
            _, reward, _, _, done, inf = env.dual_step(a)
            m = inf["action_mask"]
            if record:
                store.record_post(k, reward, done)

    def record_only():
        for k in range(K):
            store.record_pre(k, env.agent_obs_u8, mask)
            store.record_post(k, env.agent_reward, env.done)

    with torch.no_grad():
        for _ in range(16):  # eager warm-up of every launch (and the games leave their openings)
            a = agent_k.act(env.agent_obs_u8, mask, seed=1234, ply_base=counter, out=plain_out)[0]
            env.dual_step(a)
        record_only()
        graphs = {}
        for name, record in (("plain", False), ("recorded", True)):
            torch.cuda.synchronize(dev)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                rollout(record)
            graphs[name] = g
        ms = timed({"plain": graphs["plain"].replay, "recorded": graphs["recorded"].replay, "record_only": record_only})
    record_bytes = T * (2 * 300 + 45 + 8 + 2 * 4 + 2 * 1)
    rec = {"ms_per_dual_step_plain": round(ms["plain"] / K, 5), "ms_per_dual_step_recorded": round(ms["recorded"] / K, 5),
           "ratio_recorded_over_plain": round(ms["recorded"] / ms["plain"], 4),
           "record_launches_us_per_step": round(ms["record_only"] / K * 1e3, 2), "record_bytes_per_step": record_bytes,
           "record_GBps": round(record_bytes / (ms["record_only"] / K * 1e-3) / 1e9, 1),
           "note": "hipGraph replays of `steps` dual steps; record_launches: the two spl_ppo_record launches of a step, "
                   "eager, back to back"}

    # ---- 2. GAE ----------------------------------------------------------------------------------
    last_value = agent_k.get_value(env.eng.obs).view(-1).clone()
    gamma, lam = 0.999, 0.95
    t_adv, t_ret = torch.empty_like(store.adv), torch.empty_like(store.ret)

    def torch_gae():
        last = torch.zeros(T, dtype=torch.float64, device=dev)
        g32 = torch.tensor(gamma, dtype=torch.float32, device=dev)
        gl = gamma * lam
        for t in reversed(range(K)):
            nnt = 1.0 - store.done[t].double()
            v_next = last_value if t == K - 1 else store.value[t + 1]
            v = store.value[t].double()
            delta = store.reward[t].double() + (g32 * v_next).double() * nnt - v
            last = delta + (gl * nnt) * last
            t_adv[t] = last.float()
            t_ret[t] = (last + v).float()

    ms = timed({"kernel": lambda: store.compute_gae(last_value, gamma, lam), "torch": torch_gae}, inner=4)
    # the same launch after 1 GiB of other stores has gone through the 256 MB Infinity Cache
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    cold = timed({"kernel": lambda: store.compute_gae(last_value, gamma, lam)}, before=flush.zero_)
    del flush
    gae_bytes = K * T * (4 + 4 + 1 + 4 + 4) + 4 * T
    gae = {"kernel_us": round(ms["kernel"] * 1e3, 1), "torch_loop_us": round(ms["torch"] * 1e3, 1),
           "ratio_torch_over_kernel": round(ms["torch"] / ms["kernel"], 2), "bytes": gae_bytes,
           "kernel_GBps": round(gae_bytes / (ms["kernel"] * 1e-3) / 1e9, 1),
           "kernel_after_flush_us": round(cold["kernel"] * 1e3, 1),
           "kernel_after_flush_GBps": round(gae_bytes / (cold["kernel"] * 1e-3) / 1e9, 1),
           "torch_loop_bit_equal": bool(torch.equal(t_adv.view(torch.int32), store.adv.view(torch.int32))
                                        and torch.equal(t_ret.view(torch.int32), store.ret.view(torch.int32))),
           "stats": store.stats()}

    # ---- 3. gather -------------------------------------------------------------------------------
    total = K * T
    rows_u8, bits = store.obs_u8.view(total, 300), store.mask_bits.view(total)
    shifts = torch.arange(45, device=dev)
    flat = {n: getattr(store, n).view(total) for n in ("action", "logprob", "value", "adv", "ret")}

    def torch_gather(idx):
        r = rows_u8.index_select(0, idx)
        obs = r[:, :297].float()
        obs[:, 295] += 256.0 * r[:, 297].float()
        m = ((bits.index_select(0, idx).unsqueeze(1) >> shifts) & 1).float()
        adv = (flat["adv"].index_select(0, idx) - store.mean32) / (store.std32 + 1e-8)
        return (obs, m, flat["action"].index_select(0, idx).long(), flat["logprob"].index_select(0, idx),
                flat["value"].index_select(0, idx), adv, flat["ret"].index_select(0, idx))

    gather = {}
    gen = torch.Generator(device=dev).manual_seed(0)
    for B in (256, 65536):
        idx = torch.randperm(total, device=dev, generator=gen)[:B].contiguous()
        out = store.gather(idx)
        ref = torch_gather(idx)
        same = all(torch.equal(out[n], r) for n, r in zip(("obs", "mask", "action", "logprob", "value", "adv", "ret"), ref))
        ms = timed({"kernel": lambda: store.gather(idx, out=out), "torch": lambda: torch_gather(idx)},
                   inner=200 if B <= 4096 else 20)
        nbytes = B * (8 + 300 + 8 + 5 * 4) + B * (297 * 4 + 45 * 4 + 8 + 4 * 4)
        gather[f"B{B}"] = {"kernel_us": round(ms["kernel"] * 1e3, 1), "torch_us": round(ms["torch"] * 1e3, 1),
                           "ratio_torch_over_kernel": round(ms["torch"] / ms["kernel"], 2), "bytes": nbytes,
                           "kernel_GBps": round(nbytes / (ms["kernel"] * 1e-3) / 1e9, 1), "equal_to_torch": bool(same)}
    assert int(store.errors.item()) == 0

    # ---- 4. loss head ----------------------------------------------------------------------------
    # the store as a rollout leaves it (the timing loops above ended on record_only, whose masks do not
    # belong to the recorded actions)
    from splendor_gym.policy import masked_categorical
    graphs["recorded"].replay()
    store.compute_gae(last_value, gamma, lam)
    clip_coef, vclip, vf_coef, ent_coef = 0.2, 0.2, 0.5, 0.03
    loss_head = {}
    for B in (256, 65536):
        idx = torch.randperm(total, device=dev, generator=gen)[:B].contiguous()
        mb = store.gather(idx)
        with torch.no_grad():
            logits0, value0 = agent.actor(mb["obs"]), agent.critic(mb["obs"])
        leaves = {arm: (logits0.clone().requires_grad_(), value0.clone().requires_grad_()) for arm in ("kernel", "torch")}

        def torch_head():
            logits, value = leaves["torch"]
            logits.grad = value.grad = None
            probs = masked_categorical(logits, mb["mask"])
            new_logprob, entropy = probs.log_prob(mb["action"]), probs.entropy().mean()
            ratio = (new_logprob - mb["logprob"]).exp()
            clip_adv = torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef) * mb["adv"]
            policy_loss = -torch.min(ratio * mb["adv"], clip_adv).mean()
            v_pred = value.squeeze(-1)
            v_clipped = mb["value"] + torch.clamp(v_pred - mb["value"], -vclip, vclip)
            value_loss = 0.5 * torch.max((v_pred - mb["ret"]).pow(2), (v_clipped - mb["ret"]).pow(2)).mean()
            (policy_loss + vf_coef * value_loss + ent_coef * entropy).backward()

        def kernel_head():
            logits, value = leaves["kernel"]
            logits.grad = value.grad = None
            store.loss(idx, logits, value, clip_coef, vclip, vf_coef, ent_coef)[0].backward()

        def launches_only():  # spl_ppo_loss's two launches, without autograd's copies of the gradients
            store.loss(idx, logits0, value0, clip_coef, vclip, vf_coef, ent_coef)

        ms = timed({"kernel": kernel_head, "torch": torch_head, "launches": launches_only}, inner=200 if B <= 4096 else 20)
        bad = int(store.loss(idx, logits0, value0)[1].bad)
        scale = float(leaves["torch"][0].grad.abs().max())
        diff = max(float((leaves["kernel"][0].grad - leaves["torch"][0].grad).abs().max()),
                   float((leaves["kernel"][1].grad - leaves["torch"][1].grad).abs().max()))
        # idx, mask word, action, four float planes, logits and value in; both gradients out; the partial sums
        nbytes = B * (8 + 8 + 4 + 4 * 4 + 45 * 4 + 4 + 45 * 4 + 4) + 2 * 48 * ((B + 255) // 256) + 56
        loss_head[f"B{B}"] = {"kernel_fwd_bwd_us": round(ms["kernel"] * 1e3, 1), "torch_fwd_bwd_us": round(ms["torch"] * 1e3, 1),
                              "ratio_torch_over_kernel": round(ms["torch"] / ms["kernel"], 2),
                              "launches_only_us": round(ms["launches"] * 1e3, 1), "bytes": nbytes,
                              "launches_only_GBps": round(nbytes / (ms["launches"] * 1e-3) / 1e9, 1),
                              "launches_only_fraction_of_8TBps": round(nbytes / (ms["launches"] * 1e-3) / 8e12, 4),
                              "bad_rows": bad, "max_abs_gradient_difference_to_torch": diff, "max_abs_gradient": scale}
    loss_head["note"] = ("forward and backward of the loss head from leaf logits / value tensors, fp32: PPORolloutStore.loss "
                         "(spl_ppo_loss, then autograd's grad_output * gradient) beside the torch expression of ppo_update; "
                         "launches_only: spl_ppo_loss alone")
    if args.loss_json:
        with open(args.loss_json, "w") as f:
            json.dump({"metric": f"PPO loss head, store of {T} tables x {K} steps, one MI355X", "repeats": args.repeats,
                       "loss": loss_head}, f, indent=1)
            f.write("\n")

    print(json.dumps({"metric": f"PPO rollout store, {T} tables x {K} steps, one MI355X", "tables": T, "steps": K,
                      "repeats": args.repeats, "timing": "device events around back-to-back eager calls (graphs: one replay), arms alternating, medians; "
                                "calls of a few microseconds are bound by the host's launch path",
                      "store_bytes": sum(getattr(store, n).numel() * getattr(store, n).element_size() for n in
                                         ("obs_u8", "mask_bits", "action", "logprob", "value", "reward", "done", "adv", "ret")),
                      "record": rec, "gae": gae, "gather": gather, "loss": loss_head, "adam": adam_section()}))
    env.close()


if __name__ == "__main__":
    main()
