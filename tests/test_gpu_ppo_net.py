"""The PPO network passes on the device (spl_ppo_net_forward / spl_ppo_net_backward, splendor_gym.ppo.DeviceNets):
rows against the float64 oracle of test_ppo_net_host.py, the rebuilt column 295, bad rows, overwrite and
determinism, the real loss head against autograd, one minibatch as a captured single-stream graph,
ppo_update(device_nets=True) with both optimisers and ppo_device --device-nets.

Tolerances are not constants.  The kernels and torch's float32 path evaluate one formula and differ in
summation order and in their tanh, so against the float64 oracle a kernel result may be off by at most
max(4 x torch's float32 error on the same inputs, 64 x 2^-24 x the largest magnitude of the oracle's tensor),
per tensor: logits, value and B x each of the twelve gradients.  Measured on an MI355X: DESIGN.md's table."""
import copy

import numpy as np
import pytest

from test_gpu_ppo_adam import (EPS, LR, bits, choose_target_kl, compare, finite_figures, reference_update,  # noqa: F401
                               run_cli, run_update)
from test_gpu_ppo_loss import DEV, allowed, collected, head_gradients, trained  # noqa: F401  (collected: a module fixture)
from test_ppo_net_host import FIELDS, NA, NETS, expand, net_oracle, params_of, quantities, tensors_of, torch_passes

pytestmark = pytest.mark.gpu

K, T = 3, 70
P = K * T
CRAFTED = (5, 77, 209)  # positions whose move count is 256 or more
SENTINEL = -77.0
COEF = (0.2, 0.2, 0.5, 0.03)


def constants():
    from splendor_gym import _native
    return _native.PPO_NET_FWD_ROWS, _native.PPO_NET_BWD_ROWS


@pytest.fixture(scope="module")
def store(collected):
    """A 3 x 70 store whose observation rows are the first 210 the checkpoint collected, three of them with a
    move count of 256 or more.  The tests only read it."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    _, real = collected
    s = PPORolloutStore(K, T, DEV)
    s.obs_u8.view(P, 300).copy_(real.obs_u8.view(-1, 300)[:P])
    for i, q in enumerate(CRAFTED):
        s.obs_u8.view(P, 300)[q, 297] = 1 + i
    torch.cuda.synchronize()
    return s


@pytest.fixture(scope="module")
def agents():
    import torch
    from splendor_gym.policy import ActorCritic
    torch.manual_seed(11)
    return {"trained": trained(), "fresh": ActorCritic().to(DEV)}


def in_arena(agent):
    """A copy of the agent whose twelve gradients lie in one arena filled with SENTINEL, each segment on a
    16-byte boundary with at least four sentinel floats before and after it.  Returns (agent, arena, views)."""
    import torch
    a = copy.deepcopy(agent)
    ps = tensors_of(a)
    at, total = [], 4
    for p in ps:
        at.append(total)
        total += (p.numel() + 3) // 4 * 4 + 4
    arena = torch.full((total,), SENTINEL, dtype=torch.float32, device=DEV)
    views = [arena[o:o + p.numel()].view(p.shape) for o, p in zip(at, ps)]
    for p, v in zip(ps, views):
        p.grad = v
    return a, arena, views


def gaps_untouched(arena, views):
    import torch
    keep = torch.ones_like(arena, dtype=torch.bool)
    base = arena.data_ptr()
    for v in views:
        o = (v.data_ptr() - base) // 4
        keep[o:o + v.numel()] = False
    return bool((arena[keep] == SENTINEL).all()) and int(keep.sum()) >= 4 * (len(views) + 1)


def gradients(dlogits_seed, B):
    rng = np.random.default_rng(dlogits_seed)
    return (rng.normal(size=(B, NA)) / B).astype(np.float32), (rng.normal(size=B) / B).astype(np.float32)


def run_device(agent, store, idx, dlogits, dvalue):
    """DeviceNets.forward and backward with every output pre-filled with SENTINEL.  Everything on the host as
    float64, in net_oracle's layout, plus the objects."""
    import torch
    from splendor_gym.ppo import DeviceNets
    a, arena, views = in_arena(agent)
    nets = DeviceNets(a)
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(tensors_of(a), views))  # taken in place
    B = len(idx)
    bufs = nets._buffers(B)
    for name in ("logits", "value", "act", "scratch"):
        bufs[name].fill_(SENTINEL)
    d_idx = torch.from_numpy(idx).to(DEV)
    logits, value = nets.forward(store, d_idx)
    assert logits.shape == (B, NA) and value.shape == (B,) and not logits.requires_grad and not value.requires_grad
    nets.backward(store, d_idx, torch.from_numpy(dlogits).to(DEV), torch.from_numpy(dvalue).to(DEV))
    torch.cuda.synchronize()
    assert gaps_untouched(arena, views)
    got = {"logits": logits.double().cpu().numpy(), "value": value.double().cpu().numpy(),
           "grads": {net: [v.double().cpu().numpy() for v in views[6 * i:6 * i + 6]] for i, net in enumerate(NETS)}}
    return got, nets, a, arena


def torch32(agent, rows, dlogits, dvalue):
    import torch
    x = torch.from_numpy(expand(rows).astype(np.float32)).to(DEV)
    return torch_passes(copy.deepcopy(agent), x, torch.from_numpy(dlogits).to(DEV), torch.from_numpy(dvalue).to(DEV))


def check(label, got, ref, want, B):
    """The rule of the module docstring on every tensor; prints every figure first."""
    figures = []
    for (name, g), (_, r), (_, w) in zip(quantities(got, B), quantities(ref, B), quantities(want, B)):
        e_k, e_t, scale = float(np.abs(g - w).max()), float(np.abs(r - w).max()), float(np.abs(w).max())
        figures.append((name, e_k, e_t, scale))
        print(f"{label} B={B} {name}: e_kernel {e_k:.3e} e_torch {e_t:.3e} scale {scale:.3e} allowed {allowed(e_t, scale):.3e}")
    for name, e_k, e_t, scale in figures:
        assert e_k <= allowed(e_t, scale), (label, name, e_k, e_t, scale)


def rows_of(store, idx):
    safe = np.where((idx >= 0) & (idx < P), idx, 0)
    return store.obs_u8.view(P, 300).cpu().numpy()[safe]


def batch_sizes():
    R, S = constants()
    return sorted({1, R - 1, R, R + 1, S + 1, 2 * S + 1})


def make_idx(B, seed):
    """B positions with duplicates; the crafted positions when there is room."""
    idx = np.random.default_rng(seed).integers(0, P, size=B).astype(np.int64)
    if B >= 7:
        idx[:5] = (CRAFTED[0], P - 1, CRAFTED[1], CRAFTED[0], CRAFTED[2])
    elif B >= 2:
        idx[-1] = idx[0]
    return idx


@pytest.mark.parametrize("kind", ["trained", "fresh"])
@pytest.mark.parametrize("B", batch_sizes())
def test_rows_against_the_oracle(store, agents, kind, B):
    """One row; one short of, exactly and one past a forward tile; one past one and two chunks of the sums
    over rows.  Every word of every output is written; the gaps between the gradients are not."""
    agent = agents[kind]
    idx = make_idx(B, B)
    dlogits, dvalue = gradients(B, B)
    rows = rows_of(store, idx)
    before = int(store.errors.item())
    got, _, _, arena = run_device(agent, store, idx, dlogits, dvalue)
    assert not (got["logits"] == SENTINEL).any() and not (got["value"] == SENTINEL).any()
    for net in NETS:
        assert not any((g == SENTINEL).any() for g in got["grads"][net])
    want = net_oracle(params_of(agent), rows, dlogits, dvalue)
    check(f"rows {kind}", got, torch32(agent, rows, dlogits, dvalue), want, B)
    assert int(store.errors.item()) == before


def test_column_295_is_rebuilt(store, agents):
    import torch
    from splendor_gym.ppo import DeviceNets, PPORolloutStore
    agent = agents["trained"]
    idx = np.array(CRAFTED + (CRAFTED[0],), dtype=np.int64)
    B = len(idx)
    dlogits, dvalue = gradients(3, B)
    got, _, _, _ = run_device(agent, store, idx, dlogits, dvalue)
    rows = rows_of(store, idx)
    assert (rows[:, 297] > 0).all()
    check("column 295", got, torch32(agent, rows, dlogits, dvalue), net_oracle(params_of(agent), rows, dlogits, dvalue), B)
    cleared = PPORolloutStore(K, T, DEV)
    cleared.obs_u8.copy_(store.obs_u8)
    cleared.obs_u8[:, :, 297] = 0
    low, _ = DeviceNets(copy.deepcopy(agent)).forward(cleared, torch.from_numpy(idx).to(DEV))
    low = low.double().cpu().numpy()
    assert all(not np.array_equal(low[r], got["logits"][r]) for r in range(B))


def test_bad_rows(store, agents):
    agent = agents["trained"]
    B = 65
    idx = make_idx(B, 9)
    idx[[3, 8, 64]] = (-1, P, 2 ** 40)
    bad = (idx < 0) | (idx >= P)
    assert bad.sum() == 3
    dlogits, dvalue = gradients(9, B)
    rows = rows_of(store, idx)
    planes = store.obs_u8.clone()
    before = int(store.errors.item())
    got, _, _, _ = run_device(agent, store, idx, dlogits, dvalue)
    assert int(store.errors.item()) - before == 3  # the forward call counts, the backward call does not
    assert not got["logits"][bad].any() and not got["value"][bad].any()  # exact zeros
    want = net_oracle(params_of(agent), rows, dlogits, dvalue, bad=bad)
    kept = torch32(agent, rows[~bad], dlogits[~bad], dvalue[~bad])  # the good rows alone
    ref = {"logits": np.zeros((B, NA)), "value": np.zeros(B), "grads": kept["grads"]}
    ref["logits"][~bad], ref["value"][~bad] = kept["logits"], kept["value"]
    check("bad rows", got, ref, want, B)
    assert bool((store.obs_u8 == planes).all())


def test_overwrite_and_determinism(store, agents):
    import torch
    from splendor_gym.ppo import DeviceNets
    agent = agents["fresh"]
    _, S = constants()
    B = 2 * S + 1
    idx = make_idx(B, 4)
    idx[10] = -1
    dlogits, dvalue = gradients(4, B)
    got, nets, a, arena = run_device(agent, store, idx, dlogits, dvalue)
    first = arena.view(torch.int32).clone()
    d = lambda x: torch.from_numpy(x).to(DEV)
    nets.backward(store, d(idx), d(dlogits), d(dvalue))  # on top of the first call's gradients
    assert torch.equal(arena.view(torch.int32), first)
    # fresh buffers, another fill
    b, arena2, _ = in_arena(agent)
    nets2 = DeviceNets(b)
    for name in ("logits", "value", "act", "scratch"):
        nets2._buffers(B)[name].fill_(123.0)
    nets2.forward(store, d(idx))
    nets2.backward(store, d(idx), d(dlogits), d(dvalue))
    assert torch.equal(arena2.view(torch.int32), first)
    assert torch.equal(nets2._buffers(B)["logits"], nets._buffers(B)["logits"])
    assert torch.equal(nets2._buffers(B)["value"], nets._buffers(B)["value"])


def test_refusals_on_the_device(store, agents):
    import torch
    from splendor_gym import _native
    from splendor_gym.ppo import DeviceNets
    from splendor_gym.policy import ActorCritic
    with pytest.raises(ValueError, match="GPU"):
        DeviceNets(ActorCritic())
    nets = DeviceNets(copy.deepcopy(agents["fresh"]))
    idx = torch.arange(8, dtype=torch.int64, device=DEV)
    for bad in (idx.int(), idx.cpu(), idx[:0], idx.view(2, 4), torch.arange(16, device=DEV)[::2]):
        with pytest.raises(ValueError, match="idx"):
            nets.forward(store, bad)
    with pytest.raises(ValueError, match=str(_native.PPO_NET_MAX_ROWS)):
        nets.forward(store, torch.zeros(_native.PPO_NET_MAX_ROWS + 1, dtype=torch.int64, device=DEV))
    ok_l, ok_v = torch.zeros(8, NA, device=DEV), torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="forward"):
        nets.backward(store, idx, ok_l, ok_v)
    nets.forward(store, idx)
    for dl, dv in ((ok_l.double(), ok_v), (ok_l[:, :44], ok_v), (ok_l, ok_v[:7]), (ok_l.cpu(), ok_v), (ok_l, torch.zeros(8, 2, device=DEV))):
        with pytest.raises(ValueError, match="dlogits|dvalue"):
            nets.backward(store, idx, dl, dv)
    nets.backward(store, idx, ok_l, ok_v.view(8, 1))
    # an index tensor that starts off a 16-byte boundary is taken (copied), with the same result
    odd = torch.arange(9, dtype=torch.int64, device=DEV)[1:]
    assert odd.data_ptr() % 16 == 8
    a = nets.forward(store, odd)[0].clone()
    assert torch.equal(a, nets.forward(store, odd.clone())[0])


# ---------------------------------------------------------------------------------------------------
def split(vector, agent):
    out, at = [], 0
    for p in agent.parameters():
        out.append(vector[at:at + p.numel()].cpu().numpy())
        at += p.numel()
    return out


def test_against_autograd_through_the_real_head(collected):
    """forward -> the loss launch -> backward on all 256 collected positions, against store.loss + loss.backward()
    in float32 and against a float64 copy of the agent: B x each parameter's gradient, per tensor."""
    import torch
    from splendor_gym.ppo import DeviceNets
    agent, store = collected
    B = 256
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    mb = store.gather(idx, normalize=True)
    dev = copy.deepcopy(agent)
    nets = DeviceNets(dev)
    logits, value = nets.forward(store, idx)
    bufs = store._launch_loss(idx, logits, value, COEF, True)
    nets.backward(store, idx, bufs["dlogits"], bufs["dvalue"])
    g_dev = torch.cat([p.grad.double().reshape(-1) for p in dev.parameters()])
    kl_dev = float(bufs["out"].approx_kl)
    fused = copy.deepcopy(agent)
    loss, out = store.loss(idx, fused.actor(mb["obs"]), fused.critic(mb["obs"]))
    loss.backward()
    g_32 = torch.cat([p.grad.double().reshape(-1) for p in fused.parameters()])
    g_64, kl_64 = head_gradients(agent, mb, torch.float64)
    assert int(out.bad) == 0 and int(store.errors.item()) == 0
    print(f"real head approx_kl: device nets {kl_dev:+.3e} float64 {float(kl_64):+.3e}")
    names = [n for n, _ in agent.named_parameters()]
    figures = []
    for name, a, b, w in zip(names, split(g_dev, agent), split(g_32, agent), split(g_64, agent)):
        e_k, e_t, scale = float(np.abs(B * (a - w)).max()), float(np.abs(B * (b - w)).max()), float(np.abs(B * w).max())
        figures.append((name, e_k, e_t, scale))
        print(f"real head {name}: e_kernel {e_k:.3e} e_torch {e_t:.3e} scale {scale:.3e} allowed {allowed(e_t, scale):.3e}")
    for name, e_k, e_t, scale in figures:
        assert scale > 0 and e_k <= allowed(e_t, scale), (name, e_k, e_t, scale)


def minibatch(nets, store, opt, idx):
    logits, value = nets.forward(store, idx)
    bufs = store._launch_loss(idx, logits, value, COEF, True)
    nets.backward(store, idx, bufs["dlogits"], bufs["dvalue"])
    opt.step(loss_out=bufs["out"])


def test_one_minibatch_is_one_linear_graph(collected):
    """forward, loss, backward and DeviceAdam.step captured after an eager first run, the way collect(graph=True)
    does, replayed twice with set_lr between: bit-equal to the same three minibatches eager.  Every call of the
    capture is issued on the capture's one stream and nothing forks from it, so the graph is a single chain."""
    import torch
    from splendor_gym.ppo import DeviceAdam, DeviceNets
    agent, store = collected
    idx = torch.arange(64, 192, dtype=torch.int64, device=DEV)
    rates = (LR, LR, 1e-3)

    def make():
        a = copy.deepcopy(agent)
        return a, DeviceNets(a), DeviceAdam(list(a.parameters()), lr=LR, eps=EPS)

    a_e, nets_e, opt_e = make()
    for k, lr in enumerate(rates):
        if k == 2:
            opt_e.set_lr(lr)
        minibatch(nets_e, store, opt_e, idx)
    a_g, nets_g, opt_g = make()
    minibatch(nets_g, store, opt_g, idx)  # eager: loads every kernel, sizes every buffer
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    streams = set()
    with torch.cuda.graph(graph):
        capture = torch.cuda.current_stream().cuda_stream
        minibatch(nets_g, store, opt_g, idx)
        streams.update((nets_g._stream().value, store._stream().value, opt_g._stream().value,
                        torch.cuda.current_stream().cuda_stream))
    assert streams == {capture}  # one stream from the first call to the last: no branch to join
    assert opt_g.read_state()["step"] == 1  # capturing ran nothing
    graph.replay()
    opt_g.set_lr(rates[2])
    graph.replay()
    torch.cuda.synchronize()
    s_e, s_g = opt_e.read_state(), opt_g.read_state()
    assert s_e == s_g and s_g["step"] == 3 and s_g["lr"] == rates[2]
    assert torch.equal(opt_e._state.view(torch.int64), opt_g._state.view(torch.int64))
    want = bits(a_e.parameters()) + bits([opt_e._exp_avg, opt_e._exp_avg_sq])
    got = bits(a_g.parameters()) + bits([opt_g._exp_avg, opt_g._exp_avg_sq])
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    assert not torch.equal(bits(a_g.parameters())[0], bits(agent.parameters())[0])  # and the steps were taken


# ---------------------------------------------------------------------------------------------------
def test_ppo_update_with_device_nets(collected, reference_update):
    agent, store = collected
    want, kls, steps = reference_update
    assert steps == 8
    want = [x.detach().cpu().numpy() for x in want]
    p_ref, res_ref, _ = run_update(agent, store, False, 0.0)      # the existing fused path, torch.optim.Adam
    p_ref_dev, res_ref_dev, _ = run_update(agent, store, True, 0.0)  # the existing fused path, DeviceAdam
    for device_adam, existing in ((True, res_ref_dev), (False, res_ref)):
        label = f"ppo_update(device_nets) {'DeviceAdam' if device_adam else 'torch.optim.Adam'}"
        p, res, opt = run_update(agent, store, device_adam, 0.0, device_nets=True)
        assert res["optimizer_steps"] == existing["optimizer_steps"] == 8
        assert set(res) == set(existing)
        compare(label, p, p_ref, want, 8)
        for name in ("policy_loss", "value_loss", "entropy", "approx_kl", "first_approx_kl", "clipfrac"):
            print(f"{label} {name}: {res[name]:+.6e} existing path {existing[name]:+.6e}")
            assert np.isfinite(res[name])
        for name, w in (("approx_kl", kls[-1]), ("first_approx_kl", kls[0])):
            assert abs(res[name] - w) <= allowed(abs(res_ref[name] - w), abs(w)), name
    assert int(store.errors.item()) == 0


def test_ppo_update_with_device_nets_stops_where_the_float64_loop_stops(collected, reference_update):
    """target_kl between two of the run's minibatch KLs, chosen as test_gpu_ppo_adam.py chooses it."""
    agent, store = collected
    _, kls, _ = reference_update
    want_steps, target, _ = choose_target_kl(agent, store, kls)
    _, res_dev, opt = run_update(agent, store, True, target, device_nets=True)
    _, res_opt, _ = run_update(agent, store, False, target, device_nets=True)
    assert res_dev["optimizer_steps"] == res_opt["optimizer_steps"] == want_steps
    assert res_dev["gated"] == 8 - want_steps and opt.target_kl == target


def test_ppo_update_refuses_nets_of_another_agent(collected):
    import torch
    from splendor_gym.ppo import DeviceNets, ppo_update
    agent, store = collected
    a = copy.deepcopy(agent)
    with pytest.raises(ValueError, match="another agent"):
        ppo_update(a, torch.optim.Adam(a.parameters()), store, device_nets=DeviceNets(copy.deepcopy(agent)))


def test_cli_device_nets():
    """ppo_device --device-nets at the smallest shape: one update, every printed figure finite."""
    finite_figures(run_cli("--update-epochs", "1", "--device-nets", "--device-adam", updates=1)[0], 2)
