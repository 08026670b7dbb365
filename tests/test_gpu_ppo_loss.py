"""The PPO loss head on the device (spl_ppo_loss, PPORolloutStore.loss): rows whose branches are fixed by
construction against the float64 oracle of test_ppo_loss_host.py, bad rows, determinism, the parameter
gradients through autograd on a collected store, ppo_update(fused_loss=True) and ppo_device --fused-loss.

Tolerances are not constants.  The kernel and torch's float32 head evaluate one formula and differ only
in summation order and in their exp / log, so the kernel may be as far from the float64 oracle as
max(4 x torch's float32 error on the same inputs, 64 x 2^-24 x the scale of the quantity)."""
import copy
import os

import numpy as np
import pytest

from test_ppo_loss_host import COEF, NA, STATS, case_idx, case_rows, loss_oracle, make_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K, T = 3, 70
P = K * T
ULPS = 64 * 2.0 ** -24


def allowed(e_torch, scale):
    return max(4.0 * e_torch, ULPS * scale)


def store_of(case):
    """A K x T store whose planes hold make_case's (the advantage statistics are not set)."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    s = PPORolloutStore(case["K"], case["T"], DEV)
    for name in ("mask_bits", "action", "logprob", "value", "adv", "ret"):
        getattr(s, name).copy_(torch.from_numpy(case[name]).view(case["K"], case["T"]))
    return s


def torch_head(rows, sign=1.0, dtype=None, divisor=None):
    """The loss head of ppo_update on the GPU from leaf logits / value tensors (dtype: torch.float32 by
    default).  divisor None: the literal expression with its .mean()s; a number: the sums over the given
    rows divided by it (the minibatch had bad rows, which are not in `rows`).  Returns the gradients as
    float64 numpy and the statistics as floats."""
    import torch
    from splendor_gym.policy import masked_categorical
    dtype = dtype or torch.float32
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    n = len(rows["action"])
    logits, value = dev(rows["logits"]).to(dtype).requires_grad_(), dev(rows["value"]).to(dtype).view(n, 1).requires_grad_()
    mask = dev(((rows["mask_bits"][:, None] >> np.arange(NA)) & 1).astype(np.float32))
    mb = {k: dev(rows[k]).to(dtype) for k in ("lp_old", "v_old", "adv", "ret")}
    clip_coef, vclip, vf_coef, ent_coef = (rows[k] for k in ("clip_coef", "vclip", "vf_coef", "ent_coef"))
    mean = (lambda x: x.mean()) if divisor is None else (lambda x: x.sum() / divisor)
    probs = masked_categorical(logits, mask)
    new_logprob, entropy = probs.log_prob(dev(rows["action"]).long()), mean(probs.entropy())
    ratio = (new_logprob - mb["lp_old"]).exp()
    clip_adv = torch.clamp(ratio, 1 - clip_coef, 1 + clip_coef) * mb["adv"]
    policy_loss = -mean(torch.min(ratio * mb["adv"], clip_adv))
    v_pred = value.squeeze(-1)
    v_clipped = mb["v_old"] + torch.clamp(v_pred - mb["v_old"], -vclip, vclip)
    value_loss = 0.5 * mean(torch.max((v_pred - mb["ret"]).pow(2), (v_clipped - mb["ret"]).pow(2)))
    loss = policy_loss + vf_coef * value_loss + sign * ent_coef * entropy
    loss.backward()
    stats = {"loss": loss, "policy_loss": policy_loss, "value_loss": value_loss, "entropy": entropy,
             "approx_kl": mean(mb["lp_old"] - new_logprob), "clipfrac": mean(((ratio - 1).abs() > clip_coef).to(dtype))}
    return {"dlogits": logits.grad.double().cpu().numpy(), "dvalue": value.grad.double().cpu().numpy().reshape(n),
            **{k: float(v.detach()) for k, v in stats.items()}}


def run_loss(store, case, idx, normalize=False, entropy_bonus=False, value_2d=False):
    """store.loss on rows idx of the case's logits and values, the store's gradient buffers pre-filled
    with a sentinel; backward() with the default grad_output of 1.  Everything on the host."""
    import torch
    B = len(idx)
    bufs = store._loss_buffers(B)
    bufs["dlogits"].fill_(-77.0)
    bufs["dvalue"].fill_(-77.0)
    safe = np.where((idx >= 0) & (idx < P), idx, 0)
    logits = torch.from_numpy(case["logits"][safe]).to(DEV).requires_grad_()
    value = torch.from_numpy(case["v"][safe]).to(DEV)
    value = (value.view(B, 1) if value_2d else value).requires_grad_()
    loss, out = store.loss(torch.from_numpy(idx).to(DEV), logits, value, entropy_bonus=entropy_bonus, normalize=normalize, **COEF)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    loss.backward()
    assert value.grad.shape == value.shape
    assert torch.equal(logits.grad, bufs["dlogits"]) and torch.equal(value.grad.view(B), bufs["dvalue"])
    got = {"dlogits": logits.grad.double().cpu().numpy(), "dvalue": value.grad.double().cpu().numpy().reshape(B),
           "bad": int(out.bad), "loss32": float(out.loss32), "loss_tensor": float(loss.detach()),
           **{name: float(getattr(out, name)) for name in STATS}}
    assert got["loss_tensor"] == got["loss32"] == float(np.float32(got["loss"]))
    return got


def compare(got, want, ref, B, label):
    """The tolerance rule of the module docstring on B * gradient and on each statistic; prints every
    figure first."""
    scale = max(np.abs(B * want["dlogits"]).max(), np.abs(B * want["dvalue"]).max())
    err = lambda o: max(np.abs(B * o["dlogits"] - B * want["dlogits"]).max(), np.abs(B * o["dvalue"] - B * want["dvalue"]).max())
    e_kernel, e_torch = err(got), err(ref)
    print(f"{label} B={B} gradients: e_kernel {e_kernel:.3e} e_torch {e_torch:.3e} scale {scale:.3e}")
    figures = [("gradients", e_kernel, e_torch, scale)]
    for name in STATS:
        figures.append((name, abs(got[name] - want[name]), abs(ref[name] - want[name]), abs(want[name])))
        print(f"{label} B={B} {name}: e_kernel {figures[-1][1]:.3e} e_torch {figures[-1][2]:.3e} oracle {want[name]:+.6e}")
    for name, e_k, e_t, s in figures:
        assert e_k <= allowed(e_t, s), (name, e_k, e_t, s)


@pytest.fixture(scope="module")
def case():
    return make_case(K, T, 1)


@pytest.fixture(scope="module")
def filled(case):
    """The store of the case; the tests below only read its planes."""
    return store_of(case)


@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_rows_against_the_oracle(filled, case, B):
    """One row, the last lane of a wave, one wave, one row into the second wave, one row into the second
    workgroup; duplicates in idx; no row is excluded.  Measured on an MI355X (B * gradient, scale ~ 3):
    see DESIGN.md's table."""
    idx = case_idx(P, B, B)
    bonus = B % 2 == 0
    rows = case_rows(case, idx)
    sign = -1.0 if bonus else 1.0
    want = loss_oracle(**{**rows, "ent_coef": sign * COEF["ent_coef"]})
    assert want["bad"] == 0
    before = int(filled.errors.item())
    got = run_loss(filled, case, idx, entropy_bonus=bonus, value_2d=B % 2 == 1)
    assert not (got["dlogits"] == -77.0).any() and not (got["dvalue"] == -77.0).any()  # every row written
    compare(got, want, torch_head(rows, sign), B, "rows")
    bits = rows["mask_bits"]
    illegal = (bits[:, None] != 0) & (((bits[:, None] >> np.arange(NA)) & 1) == 0)
    assert (got["dlogits"][illegal] == 0).all()
    assert got["bad"] == 0 and int(filled.errors.item()) == before


def test_normalize_uses_the_gathers_advantage(case):
    """normalize=1: the advantage is the one spl_ppo_gather hands out, from the store's own statistics."""
    import torch
    store = store_of(case)
    g = torch.Generator().manual_seed(3)
    store.reward.copy_(torch.randn(K, T, generator=g))
    store.done.copy_((torch.rand(K, T, generator=g) < 0.2).to(torch.uint8))
    store.compute_gae(torch.randn(T, generator=g).to(DEV))
    store.ret.copy_(torch.from_numpy(case["ret"]).view(K, T))  # keep the value branches where the case put them
    B = 65
    idx = case_idx(P, B, 5)
    adv = store.gather(torch.from_numpy(idx).to(DEV), normalize=True)["adv"].cpu().numpy()
    assert not np.array_equal(adv, store.adv.view(-1).cpu().numpy()[idx])
    rows = {**case_rows(case, idx), "adv": adv}
    got = run_loss(store, case, idx, normalize=True)
    compare(got, loss_oracle(**rows), torch_head(rows), B, "normalize")
    assert got["bad"] == 0


def bad_case(case):
    """The case with one recorded action outside its mask (position 1 allows action 44 only), and a
    minibatch that holds it and three positions outside the store."""
    broken = {**case, "action": case["action"].copy()}
    assert broken["mask_bits"][1] == 1 << 44
    broken["action"][1] = 3
    idx = case_idx(P, 257, 9)
    idx[[4, 70, 200, 256]] = (-1, P, 2 ** 40, 1)  # position 1 may occur elsewhere too: every occurrence is bad
    return broken, idx


def test_bad_rows(case):
    broken, idx = bad_case(case)
    store = store_of(broken)
    B = len(idx)
    outside = (idx < 0) | (idx >= P)
    safe = np.where(outside, 0, idx)
    rows = case_rows(broken, safe)
    want = loss_oracle(**rows, bad=outside)
    n_bad = int(outside.sum() + (idx == 1).sum())
    assert want["bad"] == n_bad >= 4
    before = int(store.errors.item())
    got = run_loss(store, broken, idx)
    assert got["bad"] == n_bad and int(store.errors.item()) - before == n_bad
    drop = outside | (idx == 1)
    assert not got["dlogits"][drop].any() and not got["dvalue"][drop].any()
    kept = {k: (v[~drop] if isinstance(v, np.ndarray) else v) for k, v in rows.items()}
    ref = torch_head(kept, divisor=B)
    full = {**ref, "dlogits": np.zeros((B, NA)), "dvalue": np.zeros(B)}
    full["dlogits"][~drop], full["dvalue"][~drop] = ref["dlogits"], ref["dvalue"]
    compare(got, want, full, B, "bad rows")


def test_two_calls_give_the_same_bits(case):
    import torch
    broken, idx = bad_case(case)
    store = store_of(broken)
    safe = np.where((idx >= 0) & (idx < P), idx, 0)
    logits, value = torch.from_numpy(case["logits"][safe]).to(DEV), torch.from_numpy(case["v"][safe]).to(DEV)
    seen = []
    for _ in range(2):
        bufs = store._loss_buffers(len(idx))
        bufs["dlogits"].fill_(-77.0)
        bufs["dvalue"].fill_(-77.0)
        bufs["out"].buf.fill_(-77.0)
        store.loss(torch.from_numpy(idx).to(DEV), logits, value, **COEF, normalize=False)
        seen.append([bufs[k].view(torch.int32).clone() for k in ("dlogits", "dvalue")] + [bufs["out"].buf.view(torch.int64).clone()])
    assert all(torch.equal(a, b) for a, b in zip(*seen))


def test_refuses_what_own_refuses(filled, case):
    import torch
    idx = torch.arange(8, dtype=torch.int64, device=DEV)
    logits, value = torch.zeros(8, NA, device=DEV), torch.zeros(8, device=DEV)
    for bad in ((idx.int(), logits, value), (idx, logits.double(), value), (idx, logits[:, :44], value),
                (idx, logits, value[:7]), (idx, logits.t().contiguous().t(), value), (idx, logits.cpu(), value),
                (idx, logits, torch.zeros(8, 2, device=DEV))):
        with pytest.raises(ValueError):
            filled.loss(*bad)
    # a backward() after a later call with the same B has lost its gradients
    first, _ = filled.loss(idx, logits.clone().requires_grad_(), value, normalize=False)
    filled.loss(idx, logits, value, normalize=False)
    with pytest.raises(RuntimeError, match="later loss"):
        first.backward()


# ---------------------------------------------------------------------------------------------------
def trained():
    from safetensors.torch import load_file
    from splendor_gym.policy import ActorCritic
    m = ActorCritic().to(DEV)
    m.load_state_dict(load_file(os.path.join(os.path.dirname(__file__), "golden", "ppo_splendor_latest.safetensors"), device=DEV))
    return m


@pytest.fixture(scope="module")
def collected():
    """The committed checkpoint, and a 4 x 64 store it collected against the random opponent, with GAE."""
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect
    from splendor_gym.selfplay import DualStepVectorEnv
    agent = trained()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    env = DualStepVectorEnv(64, device=DEV, opponent="random", policy_seed=3, opponent_obs=False, step_counter=counter,
                            agent_obs_u8=True)
    obs, info = env.reset(seed=40)
    store = PPORolloutStore(4, 64, DEV)
    collect(env, FusedActorCritic(agent), store, obs, info["action_mask"], seed=5)
    store.compute_gae()
    env.close()
    return agent, store


def head_gradients(agent, mb, dtype):
    """Parameter gradients of ppo_update's expression (default coefficients) as one float64 vector."""
    import torch
    agent = copy.deepcopy(agent).to(dtype)
    f = lambda x: x.to(dtype)
    _, new_logprob, entropy, new_value = agent.get_action_and_value(f(mb["obs"]), mb["mask"], mb["action"])
    ratio = (new_logprob - f(mb["logprob"])).exp()
    clip_adv = torch.clamp(ratio, 1 - 0.2, 1 + 0.2) * f(mb["adv"])
    policy_loss = -torch.min(ratio * f(mb["adv"]), clip_adv).mean()
    v_pred = new_value.squeeze(-1)
    v_clipped = f(mb["value"]) + torch.clamp(v_pred - f(mb["value"]), -0.2, 0.2)
    value_loss = 0.5 * torch.max((v_pred - f(mb["ret"])).pow(2), (v_clipped - f(mb["ret"])).pow(2)).mean()
    (policy_loss + 0.5 * value_loss + 0.03 * entropy.mean()).backward()
    return torch.cat([p.grad.double().reshape(-1) for p in agent.parameters()]), (f(mb["logprob"]) - new_logprob).mean().detach()


def test_parameter_gradients_through_autograd(collected):
    """All 256 positions as one minibatch, before any optimiser step (every ratio ~ 1, every value inside
    its clamp): the parameter gradients of store.loss against a float64 copy of the agent, beside those of
    the float32 torch expression."""
    import torch
    agent, store = collected
    idx = torch.arange(256, dtype=torch.int64, device=DEV)
    mb = store.gather(idx, normalize=True)
    fused = copy.deepcopy(agent)
    loss, out = store.loss(idx, fused.actor(mb["obs"]), fused.critic(mb["obs"]))
    loss.backward()
    g_fused = torch.cat([p.grad.double().reshape(-1) for p in fused.parameters()])
    g_32, _ = head_gradients(agent, mb, torch.float32)
    g_64, _ = head_gradients(agent, mb, torch.float64)
    e_fused, e_torch, norm = float((g_fused - g_64).norm()), float((g_32 - g_64).norm()), float(g_64.norm())
    print(f"parameter gradients: |fused - f64| {e_fused:.3e} |torch32 - f64| {e_torch:.3e} |f64| {norm:.3e}")
    assert int(out.bad) == 0 and float(out.clipfrac) == 0.0 and norm > 0
    assert e_fused <= allowed(e_torch, norm)


def test_ppo_update_fused(collected):
    import torch
    from splendor_gym.ppo import ppo_update
    agent, store = collected
    res = {}
    for fused in (False, True):
        a = copy.deepcopy(agent)
        opt = torch.optim.Adam(a.parameters(), lr=2.5e-4, eps=1e-5)
        gen = torch.Generator(device=DEV).manual_seed(0)
        res[fused] = ppo_update(a, opt, store, update_epochs=1, minibatch_size=128, target_kl=1e9, generator=gen,
                                fused_loss=fused)
    assert "clipfrac" not in res[False] and 0.0 <= res[True]["clipfrac"] <= 1.0
    assert res[True]["optimizer_steps"] == res[False]["optimizer_steps"] == 2
    assert all(np.isfinite(v) for v in res[True].values())
    # the first minibatch's KL, evaluated before any step: both paths against a float64 copy of the agent
    gen = torch.Generator(device=DEV).manual_seed(0)
    idx = next(iter(store.minibatches(128, gen)))
    kl_64 = float(head_gradients(agent, store.gather(idx, normalize=True), torch.float64)[1])
    e_fused, e_torch = abs(res[True]["first_approx_kl"] - kl_64), abs(res[False]["first_approx_kl"] - kl_64)
    print(f"first_approx_kl: fused {res[True]['first_approx_kl']:+.3e} torch {res[False]['first_approx_kl']:+.3e} "
          f"f64 {kl_64:+.3e} e_fused {e_fused:.3e} e_torch {e_torch:.3e}")
    assert e_fused <= allowed(e_torch, abs(kl_64))
    assert int(store.errors.item()) == 0


def test_cli_fused_loss(capsys):
    """splendor_gym.scripts.ppo_device --fused-loss at a toy size: two updates, every printed figure finite."""
    import re
    from splendor_gym.scripts import ppo_device
    ppo_device.main(["--num-envs", "64", "--num-steps", "4", "--total-timesteps", str(2 * 64 * 4), "--minibatch-size", "128",
                     "--update-epochs", "1", "--pool-size", "2", "--fused-loss", "--load-path",
                     os.path.join(os.path.dirname(__file__), "golden", "ppo_splendor_latest.safetensors")])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("update ")]
    assert len(lines) == 2 and lines[-1].startswith("update 2/2 steps 512 ")
    for ln in lines:
        nums = re.findall(r"(?:pl|vl|ent|kl) ([-+0-9.einfa]+)", ln)
        assert len(nums) == 4 and all(np.isfinite(float(x)) for x in nums), ln
