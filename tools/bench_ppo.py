"""Timings of the PPO rollout store (splendor_gym/ppo.py) at the size the engine exists for.

    python tools/bench_ppo.py [--tables 65536] [--steps 128] [--repeats 7] [--loss-json FILE]

Prints one JSON line with four comparisons, each arm timed with device events, the arms alternating,
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

    def timed(arms, inner=1, repeats=args.repeats, before=None):
        """median milliseconds per call of each arm (`inner` back-to-back calls per timed window), the arms
        alternating; one untimed call of each first; `before` runs ahead of every timed window"""
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
        return {name: statistics.median(v) for name, v in ms.items()}

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
                      "record": rec, "gae": gae, "gather": gather, "loss": loss_head}))
    env.close()


if __name__ == "__main__":
    main()
