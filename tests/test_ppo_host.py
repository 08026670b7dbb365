"""The PPO rollout store without a GPU (include/splendor_ppo.h): every spl_ppo_* entry point refuses
bad arguments on the host, before any device work, and the numpy GAE oracle the GPU tests compare
against (ppo_splendor.py:304-314 with every dtype explicit) is checked against a case worked by hand
and against the reference's own expression."""
import ctypes

import numpy as np
import pytest


def gae_oracle(reward, value, done, last_value, gamma, lam):
    """adv, ret float32 [K, T] of include/splendor_ppo.h's recurrence: np.float32(gamma) * v_next in
    float32, everything else float64, gamma * lam multiplied once, `last` carried unrounded."""
    reward, value, last_value = (np.asarray(x, dtype=np.float32) for x in (reward, value, last_value))
    done = np.asarray(done)
    K, T = reward.shape
    adv = np.zeros((K, T), dtype=np.float32)
    ret = np.zeros((K, T), dtype=np.float32)
    last = np.zeros(T, dtype=np.float64)
    gl = float(gamma) * float(lam)
    with np.errstate(all="ignore"):
        for t in reversed(range(K)):
            nnt = np.where(done[t] != 0, np.float64(0.0), np.float64(1.0))
            v_next = last_value if t == K - 1 else value[t + 1]
            gv = np.float32(gamma) * v_next
            assert gv.dtype == np.float32
            v = value[t].astype(np.float64)
            delta = (reward[t].astype(np.float64) + gv.astype(np.float64) * nnt) - v
            last = delta + (np.float64(gl) * nnt) * last
            adv[t] = last.astype(np.float32)
            ret[t] = (last + v).astype(np.float32)
    return adv, ret


def reference_loop(rewards, values, terms, last_values, gamma, gae_lambda):
    """ppo_splendor.py:304-314 as written there: rewards float64 (np.array of Python floats), values
    float32 (downloaded tensors), terminals bool, lastgaelam float64."""
    num_steps, num_envs = rewards.shape
    advantages = np.zeros_like(rewards)
    lastgaelam = np.zeros(num_envs)
    for t in reversed(range(num_steps)):
        nextnonterminal = 1.0 - terms[t]
        nextvalues = last_values if t == num_steps - 1 else values[t + 1]
        delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
        advantages[t] = lastgaelam = delta + gamma * gae_lambda * nextnonterminal * lastgaelam
    return advantages, advantages + values


def test_oracle_three_steps_by_hand():
    """gamma = lam = 0.5, one table, every operand a dyadic rational, so each step is exact:
      t=2: gv = 0.5*2 = 1;        delta = -1 + 1 - 1 = -1;          last = -1;                 ret = -1 + 1 = 0
      t=1 (done): nnt = 0;        delta = 2 + 0 - 0.25 = 1.75;      last = 1.75 + 0*(-1);      ret = 2
      t=0: gv = 0.5*0.25 = 0.125; delta = 1 + 0.125 - 0.5 = 0.625;  last = 0.625 + 0.25*1.75;  ret = 1.0625 + 0.5"""
    adv, ret = gae_oracle([[1.0], [2.0], [-1.0]], [[0.5], [0.25], [1.0]], [[0], [1], [0]], [2.0], 0.5, 0.5)
    assert adv.dtype == ret.dtype == np.float32
    assert adv[:, 0].tolist() == [1.0625, 1.75, -1.0]
    assert ret[:, 0].tolist() == [1.5625, 2.0, 0.0]


def test_oracle_rounds_gamma_times_value_to_float32():
    """The one float32 operation: gamma * v_next is fp32(fp32(0.999) * 3), not the float64 product
    0.999 * 3; with K = 1 the advantage is that product minus v."""
    g32 = np.float32(0.999) * np.float32(3.0)
    assert float(g32) != 0.999 * 3.0
    adv, ret = gae_oracle([[0.0]], [[-2.997]], [[0]], [3.0], 0.999, 0.95)
    v = float(np.float32(-2.997))
    assert adv[0, 0] == np.float32(float(g32) - v) and ret[0, 0] == np.float32((float(g32) - v) + v)


def test_oracle_equals_the_reference_expression():
    rng = np.random.default_rng(7)
    K, T = 9, 33
    values = rng.normal(size=(K, T)).astype(np.float32) * np.float32(3.0)
    rewards32 = rng.choice(np.array([0.0, -0.01, 1.0, -1.0, -0.1], dtype=np.float32), size=(K, T))
    terms = rng.random((K, T)) < 0.2
    last_values = rng.normal(size=T).astype(np.float32)
    want_adv, want_ret = reference_loop(rewards32.astype(np.float64), values, terms, last_values, 0.999, 0.95)
    adv, ret = gae_oracle(rewards32, values, terms.astype(np.uint8), last_values, 0.999, 0.95)
    assert np.array_equal(adv, want_adv.astype(np.float32))
    assert np.array_equal(ret, want_ret.astype(np.float32))


# --------------------------------------------------------------------------------------------
P = 0x10000  # a plausible, aligned, never-dereferenced device address: every case below is refused first


def _lib():
    from splendor_gym import _native
    return _native, _native.load_library()  # dlopen only: no GPU needed


def _refused(lib, code, word):
    assert code < 0, code
    msg = lib.spl_last_error()
    assert msg and word.encode() in msg, msg


def test_abi_constant_and_struct_sizes():
    import os
    import re
    native, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splendor_ppo.h")).read()
    assert re.search(r"#define SPL_PPO_ABI 1\b", src)
    assert ctypes.sizeof(native.PpoStats) == 48 and ctypes.sizeof(native.PpoRecord) == 64
    assert ctypes.sizeof(native.PpoGae) == 80 and ctypes.sizeof(native.PpoGather) == 16 + 17 * 8
    assert lib.spl_abi_version() == 9


def test_record_refusals():
    native, lib = _lib()
    full = dict(obs_u8=P, dst_obs_u8=P, mask=P, dst_mask_bits=P, reward=P, dst_reward=P, done=P, dst_done=P)
    rec = lambda **kw: ctypes.byref(native.PpoRecord(**kw))
    _refused(lib, lib.spl_ppo_record(4, None, None), "null")
    _refused(lib, lib.spl_ppo_record(0, rec(**full), None), "positive")
    _refused(lib, lib.spl_ppo_record(4, rec(), None), "null")  # nothing to record
    for name in full:  # a group with one side missing
        _refused(lib, lib.spl_ppo_record(4, rec(**{k: v for k, v in full.items() if k != name}), None), "null")
    for name in ("obs_u8", "dst_obs_u8"):
        for off in (1, 2, 3):
            _refused(lib, lib.spl_ppo_record(4, rec(**{**full, name: P + off}), None), "aligned")
    _refused(lib, lib.spl_ppo_record(4, rec(**{**full, "dst_mask_bits": P + 4}), None), "aligned")
    _refused(lib, lib.spl_ppo_record(4, rec(**{**full, "reward": P + 2}), None), "aligned")


def test_gae_refusals():
    native, lib = _lib()
    full = dict(reward=P, value=P, done=P, last_value=P, adv=P, ret=P, gamma=0.999, lam=0.95, stats=P, scratch=P)
    gae = lambda **kw: ctypes.byref(native.PpoGae(**kw))
    _refused(lib, lib.spl_ppo_gae(4, 4, None, None), "null")
    for K, T in ((0, 4), (4, 0), (-1, 4), (4, -3)):
        _refused(lib, lib.spl_ppo_gae(K, T, gae(**full), None), "positive")
    for name in ("reward", "value", "done", "last_value", "adv", "ret", "stats", "scratch"):
        _refused(lib, lib.spl_ppo_gae(4, 4, gae(**{**full, name: None}), None), "null")
    for name in ("gamma", "lam"):
        for bad in (-0.001, 1.001, float("nan"), float("inf")):
            _refused(lib, lib.spl_ppo_gae(4, 4, gae(**{**full, name: bad}), None), "[0, 1]")
    _refused(lib, lib.spl_ppo_gae(4, 4, gae(**{**full, "value": P + 2}), None), "aligned")
    assert lib.spl_ppo_gae_scratch_bytes(0) < 0 and b"positive" in lib.spl_last_error()
    assert lib.spl_ppo_gae_scratch_bytes(1) == 16 and lib.spl_ppo_gae_scratch_bytes(257) == 32


def test_gather_refusals():
    native, lib = _lib()
    ptrs = ("idx", "obs_u8", "mask_bits", "action", "logprob", "value", "adv", "ret", "stats", "out_obs", "out_mask",
            "out_action", "out_logprob", "out_value", "out_adv", "out_ret", "errors")
    full = dict(K=4, T=4, normalize=1, reserved=0, **{k: P for k in ptrs})
    gat = lambda **kw: ctypes.byref(native.PpoGather(**kw))
    _refused(lib, lib.spl_ppo_gather(4, None, None), "null")
    _refused(lib, lib.spl_ppo_gather(0, gat(**full), None), "positive")
    _refused(lib, lib.spl_ppo_gather(4, gat(**{**full, "K": 0}), None), "positive")
    _refused(lib, lib.spl_ppo_gather(4, gat(**{**full, "T": 0}), None), "positive")
    for name in ptrs:
        _refused(lib, lib.spl_ppo_gather(4, gat(**{**full, name: None}), None), "null")
    for off in (1, 2, 3):
        _refused(lib, lib.spl_ppo_gather(4, gat(**{**full, "obs_u8": P + off}), None), "aligned")
    _refused(lib, lib.spl_ppo_gather(4, gat(**{**full, "idx": P + 4}), None), "aligned")


# --------------------------------------------------------------------------------------------
class StubStore:
    """What ppo_update's torch head with a torch.optim optimiser needs of a store, on the CPU: .torch, .minibatches
    and .gather over K x T planes drawn from a seeded generator (the recorded action is always legal; the recorded
    log-probability is that of a uniform choice among the legal moves, jittered)."""
    K, T = 2, 16

    def __init__(self, seed):
        import torch
        from splendor_gym.ppo import NUM_ACTIONS, OBS_DIM
        self.torch = torch
        rng, n = np.random.default_rng(seed), self.K * self.T
        action = rng.integers(0, NUM_ACTIONS, size=n)
        mask = (rng.random((n, NUM_ACTIONS)) < 0.5).astype(np.float32)
        mask[np.arange(n), action] = 1.0
        logprob = -np.log(mask.sum(axis=1)) + 0.05 * rng.normal(size=n)
        planes = {"obs": rng.integers(0, 5, size=(n, OBS_DIM)).astype(np.float32), "mask": mask, "action": action.astype(np.int64),
                  "logprob": logprob.astype(np.float32), "value": rng.normal(size=n).astype(np.float32),
                  "adv": rng.normal(size=n).astype(np.float32), "ret": rng.normal(size=n).astype(np.float32)}
        self.planes = {k: torch.from_numpy(v) for k, v in planes.items()}

    def minibatches(self, batch_size, generator=None):
        perm = self.torch.randperm(self.K * self.T, generator=generator)
        for start in range(0, self.K * self.T, batch_size):
            yield perm[start:start + batch_size]

    def gather(self, idx, normalize=True):
        return {k: v[idx] for k, v in self.planes.items()}


def _fresh_agent():
    import torch
    from splendor_gym.policy import ActorCritic
    torch.manual_seed(3)
    return ActorCritic()


def _straight_line_update(store, epochs, minibatch, target_kl):
    """The loop ppo_update must be, written out: float32, default coefficients, clip_grad_norm_ + torch.optim.Adam,
    the reference's `break`.  Returns the parameters, (epoch, KL) of every minibatch that ran and the last
    minibatch's statistics."""
    import torch
    a = _fresh_agent()
    opt = torch.optim.Adam(a.parameters(), lr=2.5e-4, eps=1e-5)
    gen = torch.Generator().manual_seed(0)
    ran, last = [], None
    for epoch in range(epochs):
        for idx in store.minibatches(minibatch, gen):
            mb = store.gather(idx)
            _, new_logprob, entropy, new_value = a.get_action_and_value(mb["obs"], mb["mask"], mb["action"])
            ratio = (new_logprob - mb["logprob"]).exp()
            clip_adv = torch.clamp(ratio, 1 - 0.2, 1 + 0.2) * mb["adv"]
            policy_loss = -torch.min(ratio * mb["adv"], clip_adv).mean()
            v_pred = new_value.squeeze(-1)
            v_clipped = mb["value"] + torch.clamp(v_pred - mb["value"], -0.2, 0.2)
            value_loss = 0.5 * torch.max((v_pred - mb["ret"]).pow(2), (v_clipped - mb["ret"]).pow(2)).mean()
            loss = policy_loss + 0.5 * value_loss + 0.03 * entropy.mean()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(a.parameters(), 0.5)
            opt.step()
            kl = float((mb["logprob"] - new_logprob).mean().detach())
            ran.append((epoch, kl))
            last = {"policy_loss": float(policy_loss.detach()), "value_loss": float(value_loss.detach()),
                    "entropy": float(entropy.mean().detach()), "approx_kl": kl}
            if target_kl > 0 and kl > target_kl:
                break
    return list(a.parameters()), ran, last


def test_ppo_update_is_the_straight_line_loop():
    """ppo_update's torch head with torch.optim.Adam on a CPU stub store against the loop written out above, bit for
    bit: without a gate, and with a target between two neighbouring KLs of the ungated run that the first epoch
    crosses before its last minibatch.  The `break` ends that epoch only: the second one still runs."""
    import torch
    from splendor_gym.ppo import ppo_update
    store = StubStore(5)
    _, ungated, _ = _straight_line_update(store, 2, 8, 0.0)
    assert [e for e, _ in ungated] == [0] * 4 + [1] * 4
    early = sorted(kl for _, kl in ungated[:3])
    target = (early[-2] + early[-1]) / 2  # the largest of the first three minibatches' KLs crosses it, the others do not
    assert target > 0 and early[-2] < target < early[-1]
    for target_kl in (0.0, target):
        want, ran, last = _straight_line_update(store, 2, 8, target_kl)
        agent = _fresh_agent()
        opt = torch.optim.Adam(agent.parameters(), lr=2.5e-4, eps=1e-5)
        res = ppo_update(agent, opt, store, update_epochs=2, minibatch_size=8, target_kl=target_kl,
                         generator=torch.Generator().manual_seed(0))
        assert set(res) == {"policy_loss", "value_loss", "entropy", "approx_kl", "first_approx_kl", "optimizer_steps"}
        assert res["optimizer_steps"] == len(ran) and res["first_approx_kl"] == ran[0][1]
        assert {k: res[k] for k in last} == last
        assert all(torch.equal(p.detach(), w.detach()) for p, w in zip(agent.parameters(), want))
        first, second = ([kl for e, kl in ran if e == epoch] for epoch in (0, 1))
        if target_kl:
            assert len(first) < 4 and first[-1] > target_kl and all(kl <= target_kl for kl in first[:-1])
            assert len(second) >= 1  # the break ended the first epoch, not the update
        else:
            assert len(first) == len(second) == 4
    with pytest.raises(ValueError, match="update_epochs must be at least 1"):
        ppo_update(agent, opt, store, update_epochs=0)
