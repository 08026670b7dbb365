"""The PPO rollout store on the device (splendor_gym/ppo.py, include/splendor_ppo.h): spl_ppo_record and
spl_ppo_gather against numpy / torch restatements, the store filled around real dual steps against
clones of what the env returned, collect() against the loop driven by hand (eager and as a replayed
hipGraph), and one ppo_update."""
import os

import numpy as np
import pytest

from test_ppo_host import gae_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BITS = np.uint64(1) << np.arange(45, dtype=np.uint64)


def trained():
    """An ActorCritic with the reference checkpoint (tests/golden/ppo_splendor_latest.safetensors)."""
    from safetensors.torch import load_file
    from splendor_gym.policy import ActorCritic
    m = ActorCritic().to(DEV)
    m.load_state_dict(load_file(os.path.join(os.path.dirname(__file__), "golden", "ppo_splendor_latest.safetensors"),
                                device=DEV))
    return m


def compact(obs):
    """numpy int32 [n, 297] -> the uint8 [n, 300] rows of spl_step_args_t.obs_u8."""
    u8 = np.zeros((obs.shape[0], 300), dtype=np.uint8)
    u8[:, :297] = (obs & 0xFF).astype(np.uint8)
    u8[:, 297] = ((obs[:, 295] >> 8) & 0xFF).astype(np.uint8)
    return u8


def expand(u8):
    """torch uint8 [n, 300] -> the int32 [n, 297] observation it stands for."""
    obs = u8[:, :297].int()
    obs[:, 295] += 256 * u8[:, 297].int()
    return obs


# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 65, 200])
def test_record(T):
    import torch
    from splendor_gym.ppo import PPORolloutStore
    rng = np.random.default_rng(T)
    store = PPORolloutStore(3, T, DEV)
    for shift in range(6):
        obs = rng.integers(0, 256, size=(T, 297)).astype(np.int32)
        obs[:, 295] = rng.integers(256, 2000, size=T)  # move_count >= 256: byte 297 is in use
        mask = np.zeros((T, 45), dtype=np.int8)
        for i in range(T):
            kind = (i + shift) % 6
            if kind == 0:
                mask[i, 0] = 1
            elif kind == 1:
                mask[i, 44] = 1
            elif kind == 2:
                mask[i] = 1
            elif kind == 4:  # legal entries of every nonzero flavour
                mask[i] = rng.choice(np.array([0, 1, -1, 2, -128, 127], dtype=np.int8), size=45)
            elif kind == 5:
                mask[i] = rng.integers(0, 2, size=45)
        reward = rng.normal(size=T).astype(np.float32)
        done = rng.random(T) < 0.5
        for p in (store.obs_u8, store.mask_bits, store.done):
            p.fill_(0x5A)
        store.reward.fill_(-77.0)
        store.record_pre(1, torch.from_numpy(compact(obs)).to(DEV), torch.from_numpy(mask).to(DEV))
        store.record_post(1, torch.from_numpy(reward).to(DEV), torch.from_numpy(done).to(DEV))
        assert np.array_equal(store.obs_u8[1].cpu().numpy(), compact(obs))
        want = ((mask != 0).astype(np.uint64) * BITS).sum(axis=1).astype(np.uint64)
        assert np.array_equal(store.mask_bits[1].cpu().numpy().view(np.uint64), want)
        assert np.array_equal(store.reward[1].cpu().numpy(), reward)
        assert np.array_equal(store.done[1].cpu().numpy(), done.astype(np.uint8))
        for k in (0, 2):  # the neighbouring rows are untouched
            assert (store.obs_u8[k] == 0x5A).all() and (store.done[k] == 0x5A).all()
            assert (store.mask_bits[k] == 0x5A).all() and (store.reward[k] == -77.0).all()
    with pytest.raises(ValueError):
        store.record_pre(1, torch.zeros(T + 1, 300, dtype=torch.uint8, device=DEV),
                         torch.zeros(T + 1, 45, dtype=torch.int8, device=DEV))


def test_record_unaligned_rows_take_the_dword_path():
    """A store row is 300 * T bytes from the last: only 4-byte aligned for odd T, and a 4-byte aligned
    source is as good as a 16-byte one."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    T = 67
    store = PPORolloutStore(3, T, DEV)
    assert store.obs_u8[1].data_ptr() % 16 != 0
    rows = torch.randint(0, 256, (T + 1, 300), dtype=torch.uint8, device=DEV)
    src = rows.view(-1)[4:4 + T * 300].view(T, 300)  # 4 bytes past a 16-byte boundary
    store.record_pre(1, src, torch.ones(T, 45, dtype=torch.int8, device=DEV))
    assert torch.equal(store.obs_u8[1], src) and (store.obs_u8[0] == 0).all() and (store.obs_u8[2] == 0).all()
    assert (store.mask_bits[1] == (1 << 45) - 1).all()


# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filled():
    """A 3 x 50 store with random planes and the GAE of them; nothing below writes to it."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    K, T = 3, 50
    g = torch.Generator().manual_seed(11)
    store = PPORolloutStore(K, T, DEV)
    u8 = torch.randint(0, 256, (K, T, 300), dtype=torch.uint8, generator=g)
    u8[:, :, 297] = torch.randint(1, 8, (K, T), generator=g).to(torch.uint8)  # column 295 above 255
    u8[:, :, 298:] = 0
    store.obs_u8.copy_(u8)
    store.mask_bits.copy_(torch.randint(0, 1 << 45, (K, T), dtype=torch.int64, generator=g))
    store.mask_bits[0, 0], store.mask_bits[0, 1] = 1, 1 << 44
    store.action.copy_(torch.randint(0, 45, (K, T), dtype=torch.int32, generator=g))
    for p in (store.logprob, store.value, store.reward):
        p.copy_(torch.randn(K, T, generator=g))
    store.done.copy_((torch.rand(K, T, generator=g) < 0.2).to(torch.uint8))
    store.compute_gae(torch.randn(T, generator=g).to(DEV))
    return store


def gather_cases(total):
    rng = np.random.default_rng(5)
    yield [0]
    yield [total - 1]
    for B in (63, 257):
        idx = [0, total - 1, 7, 7, total - 1] + rng.integers(0, total, size=B - 5).tolist()
        yield idx


@pytest.mark.parametrize("normalize", [True, False])
def test_gather(filled, normalize):
    import torch
    s = filled
    total = s.num_steps * s.num_envs
    mean32, std32 = s.mean32.cpu(), s.std32.cpu()
    assert mean32.dtype == std32.dtype == torch.float32 and torch.isfinite(std32).all()
    flat = lambda p: p.reshape(total, *p.shape[2:]).cpu()
    obs_i32, bits = expand(flat(s.obs_u8)), flat(s.mask_bits)
    assert int(obs_i32[:, 295].min()) > 255
    mask_f = ((bits.unsqueeze(1) >> torch.arange(45)) & 1).float()
    adv = flat(s.adv)
    adv_want = (adv - mean32) / (std32 + 1e-8) if normalize else adv  # float32 operations on the CPU
    assert adv_want.dtype == torch.float32
    errors = int(s.errors.item())
    for case in gather_cases(total):
        idx = torch.tensor(case, dtype=torch.int64)
        got = {k: v.cpu() for k, v in s.gather(idx.to(DEV), normalize=normalize).items()}
        assert got["obs"].dtype == torch.float32 and tuple(got["obs"].shape) == (len(case), 297)
        assert torch.equal(got["obs"], obs_i32[idx].float())
        assert torch.equal(got["mask"], mask_f[idx])
        assert got["action"].dtype == torch.int64 and torch.equal(got["action"], flat(s.action)[idx].long())
        for name in ("logprob", "value", "ret"):
            assert torch.equal(got[name], flat(getattr(s, name))[idx]), name
        assert torch.equal(got["adv"].view(torch.int32), adv_want[idx].view(torch.int32))
    assert int(s.errors.item()) == errors


def test_gather_bad_positions_write_nothing(filled):
    import torch
    s = filled
    total = s.num_steps * s.num_envs
    B = 63
    idx = torch.arange(B, dtype=torch.int64)
    idx[5], idx[40] = total, -1  # one past the end, one negative
    out = {"obs": torch.full((B, 297), -5.0), "mask": torch.full((B, 45), -5.0),
           "action": torch.full((B,), -5, dtype=torch.int64), **{k: torch.full((B,), -5.0) for k in
                                                                  ("logprob", "value", "adv", "ret")}}
    out = {k: v.to(DEV) for k, v in out.items()}
    before = int(s.errors.item())
    s.gather(idx.to(DEV), out=out)
    assert int(s.errors.item()) - before == 2
    good = torch.ones(B, dtype=torch.bool)
    good[5] = good[40] = False
    for name, v in out.items():
        v = v.cpu()
        assert (v[~good] == -5).all(), name
        assert not (v[good].reshape(int(good.sum()), -1) == -5).all(dim=1).any(), name
    with pytest.raises(ValueError):
        s.gather(idx.to(DEV).int())


# ---------------------------------------------------------------------------------------------------
T_E2E, K_E2E = 256, 8


def make_env(opponent, agent):
    """A reset 256-table dual-step env against the "random" device opponent or a two-snapshot pool."""
    import torch
    from splendor_gym.fused_policy import OpponentPool
    from splendor_gym.policy import ActorCritic
    from splendor_gym.selfplay import DualStepVectorEnv
    if opponent == "pool":
        opponent = OpponentPool(agent, pool_size=2, p_current=0.25, seed=99)
        for seed in (21, 22):
            torch.manual_seed(seed)
            opponent.add_snapshot(ActorCritic().to(DEV))
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    env = DualStepVectorEnv(T_E2E, device=DEV, opponent=opponent, policy_seed=3, opponent_obs=False,
                            step_counter=counter, agent_obs_u8=True)
    obs, info = env.reset(seed=40)
    return env, obs, info["action_mask"]


def hand_loop(env, agent_k, store, mask, seed):
    """The config-5 loop of tools/bench_selfplay.py with the store's calls around it; clones of what the
    env returned."""
    import torch
    seen = {"obs": [], "mask": [], "reward": [], "done": []}
    obs = env.eng.obs
    for k in range(store.num_steps):
        seen["obs"].append(obs.clone())
        seen["mask"].append(mask.clone())
        store.record_pre(k, env.agent_obs_u8, mask)
        action = agent_k.act(env.agent_obs_u8, mask, seed=seed, table0=0, ply_base=env._step_counter,
                             out=store.row(k))[0]
        assert action.data_ptr() == store.action[k].data_ptr()
        obs, reward, _, _, done, info = env.dual_step(action)
        mask = info["action_mask"]
        seen["reward"].append(reward.clone())
        seen["done"].append(done.clone())
        store.record_post(k, reward, done)
    agent_k.get_value(obs, out=store.last_value.view(-1, 1))
    return {k: torch.stack(v) for k, v in seen.items()}


PLANES = ("obs_u8", "mask_bits", "action", "logprob", "value", "reward", "done", "last_value")


def snapshot(store):
    return {name: getattr(store, name).cpu().numpy().tobytes() for name in PLANES}


@pytest.mark.parametrize("opponent", ["random", "pool"])
def test_store_around_real_dual_steps(opponent):
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore
    K, T = K_E2E, T_E2E
    agent = trained()
    agent_k = FusedActorCritic(agent)
    env, obs, mask = make_env(opponent, agent)
    store = PPORolloutStore(K, T, DEV)
    seen = hand_loop(env, agent_k, store, mask, seed=1234)
    got = store.gather(torch.arange(K * T, dtype=torch.int64, device=DEV), normalize=False)
    assert torch.equal(got["obs"], seen["obs"].reshape(K * T, 297).float())
    assert torch.equal(got["mask"], (seen["mask"].reshape(K * T, 45) != 0).float())
    assert torch.equal(store.reward, seen["reward"]) and torch.equal(store.done, seen["done"].to(torch.uint8))
    assert (store.mask_bits > 0).any() and int(store.errors.item()) == 0
    # the stored log-probabilities and values are the torch module's on the gathered rows
    with torch.no_grad():
        _, logprob, _, value = agent.get_action_and_value(got["obs"], got["mask"], got["action"])
    assert torch.allclose(got["logprob"], logprob, atol=1e-5, rtol=1e-5)
    value = value.squeeze(-1)
    assert ((got["value"] - value).abs() <= 1e-5 * (value.abs() + 1)).all()
    # GAE on the store == the oracle on the downloaded planes
    store.compute_gae()
    want_adv, want_ret = gae_oracle(store.reward.cpu().numpy(), store.value.cpu().numpy(), store.done.cpu().numpy(),
                                    store.last_value.cpu().numpy(), 0.999, 0.95)
    assert np.array_equal(store.adv.cpu().numpy().view(np.uint32), want_adv.view(np.uint32))
    assert np.array_equal(store.ret.cpu().numpy().view(np.uint32), want_ret.view(np.uint32))
    env.close()


@pytest.mark.parametrize("opponent", ["random", "pool"])
def test_collect_equals_the_hand_loop(opponent):
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect
    agent = trained()
    agent_k = FusedActorCritic(agent)
    want, got = PPORolloutStore(K_E2E, T_E2E, DEV), PPORolloutStore(K_E2E, T_E2E, DEV)
    env_a, _, mask_a = make_env(opponent, agent)
    hand_loop(env_a, agent_k, want, mask_a, seed=1234)
    env_b, obs_b, mask_b = make_env(opponent, agent)
    obs_b, mask_b = collect(env_b, agent_k, got, obs_b, mask_b, seed=1234, table0=0)
    assert snapshot(got) == snapshot(want)
    assert obs_b.data_ptr() == env_b.eng.obs.data_ptr() and mask_b.data_ptr() == env_b.eng.mask.data_ptr()
    # and a second rollout continues where the first ended
    hand_loop(env_a, agent_k, want, mask_a, seed=1234)
    collect(env_b, agent_k, got, obs_b, mask_b, seed=1234, table0=0)
    assert snapshot(got) == snapshot(want)
    if opponent == "random":
        with pytest.raises(ValueError, match="network opponent"):
            collect(env_b, agent_k, got, obs_b, mask_b, seed=1234, graph=True)
    env_a.close()
    env_b.close()


def test_collect_graph_replays_equal_eager_calls():
    """Three rollouts from the same reset state: collect(graph=True) (the first call runs eagerly and
    captures, the next two replay) against three eager calls.  A failed capture raises: nothing here
    falls back to eager."""
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect
    agent = trained()
    agent_k = FusedActorCritic(agent)
    want, got = PPORolloutStore(K_E2E, T_E2E, DEV), PPORolloutStore(K_E2E, T_E2E, DEV)
    env_a, obs_a, mask_a = make_env("pool", agent)
    env_b, obs_b, mask_b = make_env("pool", agent)
    for call in range(3):
        obs_a, mask_a = collect(env_a, agent_k, want, obs_a, mask_a, seed=77)
        obs_b, mask_b = collect(env_b, agent_k, got, obs_b, mask_b, seed=77, graph=True)
        assert snapshot(got) == snapshot(want), call
        assert int(env_b._step_counter.item()) == int(env_a._step_counter.item()) == (call + 1) * K_E2E
    assert got._graph is not None and got._replays == 2
    env_a.close()
    env_b.close()


def test_ppo_update():
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect, ppo_update
    agent = trained()
    agent_k = FusedActorCritic(agent)
    env, obs, mask = make_env("pool", agent)
    store = PPORolloutStore(K_E2E, T_E2E, DEV)
    obs, mask = collect(env, agent_k, store, obs, mask, seed=5)
    store.compute_gae()
    fixed_obs, fixed_mask = obs.clone(), mask.clone()
    logits_before = agent_k.act(fixed_obs, fixed_mask, want_logits=True)[4].clone()
    params_before = [p.detach().clone() for p in agent.parameters()]
    optimizer = torch.optim.Adam(agent.parameters(), lr=2.5e-4, eps=1e-5)
    gen = torch.Generator(device=DEV).manual_seed(0)
    res = ppo_update(agent, optimizer, store, update_epochs=1, minibatch_size=512, generator=gen)
    # the first minibatch is evaluated with the weights that collected it: its KL estimate is rounding
    assert abs(res["first_approx_kl"]) <= 1e-5 * (1 + float(store.logprob.abs().max()))
    assert all(np.isfinite(res[k]) for k in ("policy_loss", "value_loss", "entropy", "approx_kl"))
    assert 1 <= res["optimizer_steps"] <= K_E2E * T_E2E // 512
    assert any(not torch.equal(a, b.detach()) for a, b in zip(params_before, agent.parameters()))
    # the packed image still holds the old weights until refresh()
    assert torch.equal(agent_k.act(fixed_obs, fixed_mask, want_logits=True)[4], logits_before)
    agent_k.refresh()
    logits_after = agent_k.act(fixed_obs, fixed_mask, want_logits=True)[4]
    assert not torch.equal(logits_after, logits_before)
    with torch.no_grad():
        ref = agent.actor(fixed_obs.float())
    assert ((logits_after - ref).abs() <= 1e-5 * (ref.abs() + 1)).all()
    assert int(store.errors.item()) == 0
    env.close()


def test_cli_trains_a_few_updates(capsys):
    """splendor_gym.scripts.ppo_device end to end at a toy size: four updates, a snapshot after each
    (so the replayed rollout graph is re-captured while the pool grows), every printed loss finite."""
    import re
    from splendor_gym.scripts import ppo_device
    ppo_device.main(["--num-envs", "256", "--num-steps", "8", "--total-timesteps", str(4 * 256 * 8),
                     "--minibatch-size", "512", "--update-epochs", "1", "--pool-size", "2",
                     "--snapshot-every-updates", "1", "--load-path",
                     os.path.join(os.path.dirname(__file__), "golden", "ppo_splendor_latest.safetensors")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 4 and lines[-1].startswith("update 4/4 steps 8192 ")
    for ln in lines:
        nums = re.findall(r"(?:pl|vl|ent|kl) ([-+0-9.einfa]+)", ln)
        assert len(nums) == 4 and all(np.isfinite(float(x)) for x in nums), ln
