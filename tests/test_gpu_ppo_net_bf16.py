"""The bf16 PPO network passes on the device (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16,
DeviceNets(operands="bf16")): every product against float64 with a DERIVED bound, layer by layer from the
planes the kernel itself saved; the exact inputs; every word written; bad rows; determinism; one minibatch as
a linear graph; the end-to-end deviation from full precision against the numpy emulator's; ppo_update and the CLI.

The bound (bf16_nets.product): both operands of a matrix-core product are bf16, so every product is exact in
float32 and the only error is that of the n float32 additions, in whatever order: gamma_n * SUM |a_k b_k| with
gamma_n = n u / (1 - n u), n the number of summed terms (the bias or the combination of the partial sums
included) and u = 2^-23, twice float32's unit round-off, so that a truncating adder inside the instruction is
covered.  Behind a tanh 4 ulp of the result are added (tanh_acc's documented limit); behind (1 - H^2) the bound
is multiplied by that factor and 2 ulp are added.  The VALU products take the same formula on unrounded operands.
Each layer is rebuilt from the operands the kernel read (its own saved float32 planes, rounded by to_bf16), so a
rounding flip in one layer does not leak into the next layer's check.

Largest error / bound per product, measured on an MI355X over the sixteen cases of test_layer_by_layer: H1 0.001,
H2 0.001, logits 0.007, dZ2 0.024, dZ1 0.008, dW1 0.014, dW2 0.014, dW3 0.006, value 0.004, the critic's dZ2 0.498
(three float32 roundings, about 1.5 ulp, against gamma_1 |s| (1 - h^2) + 2 ulp, about 3 ulp), db1 0.030, db2 0.011, db3 0.003.

The end-to-end test's yardstick is bf16_nets.emulate on the host (float64 sums of rounded operands) against the
float64 full-precision network on the same 4 097 rows: relative L2 per tensor, the kernel may deviate from full
precision by at most twice the emulator's figure.  The emulator's figures (numpy on the host; the golden
checkpoint on the collected store's rows): logits 5.38e-4, value 4.20e-3, actor w1 3.86e-3, b1 3.54e-3, w2 3.81e-3,
b2 2.75e-3, w3 2.19e-3, critic w1 2.74e-3, b1 2.58e-3, w2 2.41e-3, b2 8.55e-4, w3 2.31e-3; the kernel's were
0.999 to 1.001 of them."""
import copy
import functools

import numpy as np
import pytest

import bf16_nets
from bf16_nets import product, to_bf16, ulp32
from crafted_nets import forward64
from test_gpu_ppo_adam import EPS, LR, bits, finite_figures, run_cli
from test_gpu_ppo_loss import DEV, collected, trained  # noqa: F401  (collected: a module fixture)
from test_gpu_ppo_net import CRAFTED, K, P, T, agents, gradients, make_idx, minibatch, rows_of, store  # noqa: F401
from test_gpu_ppo_net_tiled import Counting, every_word_written, passes as net_passes
from test_ppo_net_host import FIELDS, NA, NETS, net_oracle, params_of

pytestmark = pytest.mark.gpu

H = 256
SIZES = (1, 63, 64, 65, 129, 257, 4097, 4225)
# what the sums over rows add beyond their rows: up to SPL_PPO_NET_BWD_PARTS partial sums combined in order, the
# fold of position 297 into column 295, and the four quarter sums of a stage's rows in db3
N_COMBINE = 32 + 1 + 4


# test_gpu_ppo_net_tiled.passes on DeviceNets(operands="bf16"), with the float32 host copies under "f"
passes = functools.partial(net_passes, floats=True, operands="bf16")


def params32(agent):
    return {net: [p.astype(np.float32) for p in ps] for net, ps in params_of(agent).items()}


def layer_ratios(params, rows, bad, dlogits, dvalue, f):
    """{product: largest |kernel - float64| / bound} over both networks, every layer rebuilt from the operands the
    kernel read.  f: passes()["f"]."""
    B = len(rows)
    bf = lambda v: to_bf16(np.asarray(v, dtype=np.float32)).astype(np.float64)
    x = bf16_nets.split_inputs(rows)
    x[bad] = 0.0
    ones = np.ones((B, 1))
    ratios = {}

    def note(name, got, want, bound):
        err = np.abs(np.asarray(got, dtype=np.float64) - want)
        assert err.shape == bound.shape == want.shape, name
        r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, np.finfo(np.float64).tiny))
        ratios[name] = max(ratios.get(name, 0.0), float(r.max()))

    for i, net in enumerate(NETS):
        w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params[net])
        h1, h2 = f["act"][i, 0].astype(np.float64), f["act"][i, 1].astype(np.float64)
        dz2, dz1 = f["dz"][i, 0].astype(np.float64), f["dz"][i, 1].astype(np.float64)
        d = np.asarray(dlogits if net == "actor" else dvalue, dtype=np.float64).reshape(B, -1).copy()
        d[bad] = 0.0
        # forward
        z, bound = product(x, bf16_nets.split_weights(bf(w1)).T, start=b1)
        note("H1", h1, np.tanh(z), bound + 4 * ulp32(np.tanh(z)))
        z, bound = product(bf(h1), bf(w2).T, start=b2)
        note("H2", h2, np.tanh(z), bound + 4 * ulp32(np.tanh(z)))
        if net == "actor":
            y, bound = product(bf(h2), bf(w3).T, start=b3)
        else:
            y, bound = product(h2, w3.T, start=b3)  # VALU: unrounded
        y[bad], bound[bad] = 0.0, 0.0  # exact zeros
        note("logits" if net == "actor" else "value (VALU)", f["logits"] if net == "actor" else f["value"].reshape(B, 1), y, bound)
        # backward
        fac2, fac1 = 1.0 - h2 * h2, 1.0 - h1 * h1
        s, bound = product(bf(d), bf(w3)) if net == "actor" else product(d, w3)
        note("dZ2" if net == "actor" else "dZ2 critic (VALU)", dz2, s * fac2, bound * np.abs(fac2) + 2 * ulp32(s * fac2))
        s, bound = product(bf(dz2), bf(w2))
        note("dZ1", dz1, s * fac1, bound * np.abs(fac1) + 2 * ulp32(s * fac1))
        g = f["grads"][net]
        y, bound = product(bf(dz1).T, x, n_extra=N_COMBINE)
        note("dW1", g[0], bf16_nets.fold_columns(y), bf16_nets.fold_columns(bound))
        y, bound = product(bf(dz2).T, bf(h1), n_extra=N_COMBINE)
        note("dW2", g[2], y, bound)
        y, bound = product(bf(d).T, bf(h2), n_extra=N_COMBINE)
        note("dW3", g[4], y, bound)
        for name, got, plane in (("db1 (VALU)", g[1], dz1), ("db2 (VALU)", g[3], dz2), ("db3 (VALU)", g[5], d)):
            y, bound = product(plane.T, ones, n_extra=N_COMBINE)
            note(name, got.reshape(-1, 1), y, bound)
    return ratios


def report(label, ratios):
    for name, r in ratios.items():
        print(f"{label} {name}: error / bound {r:.3f}")
    for name, r in ratios.items():
        assert r <= 1.0, (label, name, r)


@pytest.mark.parametrize("kind", ["trained", "fresh"])
@pytest.mark.parametrize("B", SIZES)
def test_layer_by_layer(store, agents, kind, B):
    """One row; one short of, exactly and one past a row tile; one and two chunks of the sums over rows; 33 chunks
    (partial 0 gets a second chunk, of one row) and 34 (a whole second chunk and a ragged one).  Every word of every
    output is written, the gaps between the gradients are not, and no row counts as bad."""
    idx = make_idx(B, B)
    dlogits, dvalue = gradients(B, B)
    out = passes(agents[kind], store, idx, dlogits, dvalue)
    every_word_written(out, B)
    assert out["errors"] == (0, 0)
    report(f"bf16 {kind} B={B}", layer_ratios(params32(agents[kind]), rows_of(store, idx), np.zeros(B, dtype=bool), dlogits, dvalue,
                                              out["f"]))


def test_inputs_are_exact(store, agents):
    """Rows whose move count is 256 or more and odd (so that column 295 is NO bf16), a network whose layer-1
    weights are zero except column 295 and small enough to keep tanh near its linear part: H1 is tanh of the
    float64 pre-activation within the bound, where a rounded column 295 would be up to 2^-9 off; dW1's column 295
    likewise."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    s = PPORolloutStore(K, T, DEV)
    s.obs_u8.copy_(store.obs_u8)
    flat = s.obs_u8.view(P, 300)
    for j, q in enumerate(CRAFTED):
        flat[q, 295] = (77, 201, 255)[j]
        flat[q, 297] = (1, 2, 3)[j]
    agent = copy.deepcopy(agents["fresh"])
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for net in NETS:
            w = np.zeros((H, 297), dtype=np.float32)
            w[:, 295] = rng.uniform(-2.5e-4, 2.5e-4, size=H)
            getattr(agent, net)[0].weight.copy_(torch.from_numpy(w).to(DEV))
    B = 65
    idx = make_idx(B, 3)
    idx[5:5 + 3 * 8] = np.tile(CRAFTED, 8)
    rows = rows_of(s, idx)
    x295 = rows[:, 295].astype(np.float64) + 256.0 * rows[:, 297]
    inexact = to_bf16(x295.astype(np.float32)) != x295
    assert inexact.sum() >= 24 and x295.max() == 3 * 256 + 255
    dlogits, dvalue = gradients(3, B)
    out = passes(agent, s, idx, dlogits, dvalue)
    params = params32(agent)
    bad = np.zeros(B, dtype=bool)
    report("exact inputs", layer_ratios(params, rows, bad, dlogits, dvalue, out["f"]))
    # and directly, with the sensitivity of the check: the rounded column is far outside the bound
    for i, net in enumerate(NETS):
        w = to_bf16(params[net][0][:, 295]).astype(np.float64)
        b1 = params[net][1].astype(np.float64)
        z = x295[:, None] * w[None, :] + b1
        bound = bf16_nets.gamma(3) * (np.abs(x295[:, None] * w[None, :]) + np.abs(b1)) + 4 * ulp32(np.tanh(z))
        h1 = out["f"]["act"][i, 0].astype(np.float64)
        assert (np.abs(h1 - np.tanh(z)) <= bound).all(), net
        z_rounded = to_bf16(x295.astype(np.float32)).astype(np.float64)[:, None] * w[None, :] + b1
        off = np.abs(np.tanh(z_rounded) - np.tanh(z))[inexact]
        assert (off > bound[inexact]).mean() > 0.9, net  # nearly every unit of every such row would show it
        dz1 = to_bf16(out["f"]["dz"][i, 1]).astype(np.float64)
        want = dz1.T @ x295
        bound = bf16_nets.gamma(B + N_COMBINE) * (np.abs(dz1).T @ x295)
        got = out["f"]["grads"][net][0][:, 295].astype(np.float64)
        assert (np.abs(got - want) <= bound).all(), net
        rounded = dz1.T @ to_bf16(x295.astype(np.float32)).astype(np.float64)
        assert (np.abs(rounded - want) > bound).mean() > 0.5, net


def test_bad_rows(store, agents):
    """Positions -1, K * T and 2^40 as the batch's last three rows: exact-zero logits and value, store.errors up
    by three in the forward call alone, and the gradients' bytes those of the same call without them (the rows
    that remain keep their order and their chunks)."""
    import torch
    B, n_bad = 4225, 3
    idx = make_idx(B, 17)
    idx[-n_bad:] = (-1, P, 2 ** 40)
    dlogits, dvalue = gradients(17, B)
    planes = store.obs_u8.clone()
    got = passes(agents["trained"], store, idx, dlogits, dvalue)
    every_word_written(got, B)
    assert got["errors"] == (n_bad, 0)
    f = got["f"]
    assert not f["logits"].view(np.int32)[-n_bad:].any() and not f["value"].view(np.int32)[-n_bad:].any()  # +0.0 in every word
    assert f["logits"][:-n_bad].any(axis=1).all() and f["value"][:-n_bad].all()
    assert not f["dz"][:, :, -n_bad:].any()
    assert bool((store.obs_u8 == planes).all())
    kept = passes(agents["trained"], store, idx[:-n_bad], dlogits[:-n_bad], dvalue[:-n_bad])
    assert kept["errors"] == (0, 0)
    assert all(torch.equal(x, y) for x, y in zip(got["views"], kept["views"]))
    assert np.array_equal(f["logits"][:-n_bad].view(np.int32), kept["f"]["logits"].view(np.int32))
    bad = np.zeros(B, dtype=bool)
    bad[-n_bad:] = True
    report("bad rows", layer_ratios(params32(agents["trained"]), rows_of(store, idx), bad, dlogits, dvalue, f))
    # bad rows in the middle of a row tile and of a chunk: zeros, counted, and the bounds hold
    B = 129
    idx = make_idx(B, 9)
    idx[[3, 63, 64, 128]] = (-1, P, 2 ** 40, -5)
    bad = (idx < 0) | (idx >= P)
    dlogits, dvalue = gradients(9, B)
    got = passes(agents["fresh"], store, idx, dlogits, dvalue)
    assert got["errors"] == (4, 0)
    assert not got["f"]["logits"].view(np.int32)[bad].any() and not got["f"]["value"].view(np.int32)[bad].any()
    report("bad rows inside", layer_ratios(params32(agents["fresh"]), rows_of(store, idx), bad, dlogits, dvalue, got["f"]))


def test_same_bytes_twice(store, agents):
    import torch
    B = 4225
    idx = make_idx(B, 4)
    idx[10] = -1
    dlogits, dvalue = gradients(4, B)
    first = passes(agents["fresh"], store, idx, dlogits, dvalue)
    again = passes(agents["fresh"], store, idx, dlogits, dvalue, fill=123.0)
    for name in ("logits", "value", "act"):
        assert torch.equal(first[name], again[name]), name
    assert torch.equal(first["scratch"][:4 * B * H], again["scratch"][:4 * B * H])
    assert all(torch.equal(x, y) for x, y in zip(first["views"], again["views"]))


def test_tiled_is_not_consulted(store, agents):
    import torch
    from splendor_gym.ppo import DeviceNets
    for tiled in (False, True, "auto"):
        nets = DeviceNets(copy.deepcopy(agents["fresh"]), tiled=tiled, operands="bf16")
        nets.lib = lib = Counting(nets.lib)
        for B in (1, DeviceNets.TILED_MIN_ROWS):
            lib.calls.clear()
            idx = torch.from_numpy(make_idx(B, 1)).to(DEV)
            nets.forward(store, idx)
            nets.backward(store, idx, torch.zeros(B, NA, device=DEV), torch.zeros(B, device=DEV))
            called = {k: v for k, v in lib.calls.items() if k.endswith(("forward", "backward", "_tiled", "_bf16"))}
            assert called == {"spl_ppo_net_forward_bf16": 1, "spl_ppo_net_backward_bf16": 1}, (tiled, B)
    torch.cuda.synchronize()


def test_one_bf16_minibatch_is_one_linear_graph(collected):
    """forward_bf16 -> spl_ppo_loss -> backward_bf16 -> spl_ppo_adam captured on one stream after an eager first
    run, replayed twice with set_lr between: the parameters and moments are byte-equal to the same three
    minibatches eager."""
    import torch
    from splendor_gym.ppo import DeviceAdam, DeviceNets
    agent, store = collected
    idx = torch.arange(64, 192, dtype=torch.int64, device=DEV)
    rates = (LR, LR, 1e-3)

    def make():
        a = copy.deepcopy(agent)
        return a, DeviceNets(a, operands="bf16"), DeviceAdam(list(a.parameters()), lr=LR, eps=EPS)

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
    # and it is another run than the f32 one
    a_f = copy.deepcopy(agent)
    minibatch(DeviceNets(a_f), store, DeviceAdam(list(a_f.parameters()), lr=LR, eps=EPS), idx)
    a_b = copy.deepcopy(agent)
    minibatch(DeviceNets(a_b, operands="bf16"), store, DeviceAdam(list(a_b.parameters()), lr=LR, eps=EPS), idx)
    assert not all(torch.equal(x, y) for x, y in zip(bits(a_f.parameters()), bits(a_b.parameters())))


def test_end_to_end_against_full_precision(collected):
    """The golden checkpoint on 4 097 positions of the collected store: logits, value and the twelve gradients
    against the float64 full-precision network (crafted_nets.forward64; its backward is test_ppo_net_host.net_oracle,
    the same formulas), relative L2 per tensor.  MEASURED, not derived: the yardstick is the numpy emulator's own
    deviation on the same inputs, which is what bf16 operands cost by construction, and the kernel may deviate by
    at most twice that: a rounding flip between emulator and kernel moves an operand by 2^-8 relative.  The
    emulator's figures are printed; the module docstring and DESIGN.md section 4.9 list them."""
    import torch
    agent, store = collected
    B = 4097
    n = store.num_steps * store.num_envs
    idx = np.random.default_rng(7).integers(0, n, size=B).astype(np.int64)
    dlogits, dvalue = gradients(7, B)
    out = passes(agent, store, idx, dlogits, dvalue)
    assert out["errors"] == (0, 0)
    rows = store.obs_u8.view(n, 300).cpu().numpy()[idx]
    params = params_of(agent)
    want = net_oracle(params, rows, dlogits, dvalue)
    fwd = forward64(params, bf16_nets.fold_columns(bf16_nets.split_inputs(rows)))
    assert np.allclose(want["logits"], fwd["actor"]["y"], rtol=1e-12, atol=1e-12) and \
        np.allclose(want["value"], fwd["critic"]["y"][:, 0], rtol=1e-12, atol=1e-12)
    emu = bf16_nets.emulate(params32(agent), rows, dlogits, dvalue)
    f = out["f"]
    figures = [("logits", f["logits"], emu["logits"], want["logits"]), ("value", f["value"], emu["value"], want["value"])]
    for net in NETS:
        for field, g, e, w in zip(FIELDS, f["grads"][net], emu["grads"][net], want["grads"][net]):
            figures.append((f"{net}.{field}", g, e, w))
    rel = [(name, bf16_nets.rel_l2(g, w), bf16_nets.rel_l2(e, w)) for name, g, e, w in figures]
    for name, kernel, emulator in rel:
        print(f"end to end {name}: kernel {kernel:.3e} emulator {emulator:.3e} ratio {kernel / emulator if emulator else float('nan'):.3f}")
    # db3 takes no rounded operand (a plain float32 sum of dOut down the rows), so the float64 emulator is exact
    # there and twice its figure would ask a float32 result for all of float64's digits: that tensor alone gets
    # the derived bound of a float32 sum instead, gamma_n * SUM |dOut|, as a relative L2 figure
    floor = {f"{net}.b3": float(np.linalg.norm(bf16_nets.gamma(B + N_COMBINE) * np.abs(d).reshape(B, -1).sum(0)) /
                                np.linalg.norm(want["grads"][net][5])) for net, d in zip(NETS, (dlogits, dvalue))}
    for name, kernel, emulator in rel:
        if name in floor:
            assert emulator <= 1e-12 and kernel <= floor[name], (name, kernel, emulator, floor[name])
        else:
            assert kernel <= 2 * emulator, (name, kernel, emulator)


@pytest.fixture(scope="module")
def long_store():
    """The committed checkpoint and a 128 x 16 store it collected against the random opponent, with GAE."""
    import torch
    from splendor_gym.fused_policy import FusedActorCritic
    from splendor_gym.ppo import PPORolloutStore, collect
    from splendor_gym.selfplay import DualStepVectorEnv
    agent = trained()
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    env = DualStepVectorEnv(16, device=DEV, opponent="random", policy_seed=3, opponent_obs=False, step_counter=counter,
                            agent_obs_u8=True)
    obs, info = env.reset(seed=41)
    s = PPORolloutStore(128, 16, DEV)
    collect(env, FusedActorCritic(agent), s, obs, info["action_mask"], seed=5)
    s.compute_gae()
    env.close()
    return agent, s


def test_ppo_update_with_bf16_nets(long_store):
    import torch
    from splendor_gym.ppo import DeviceAdam, DeviceNets, ppo_update
    agent, s = long_store
    a = copy.deepcopy(agent)
    opt = DeviceAdam(list(a.parameters()), lr=LR, eps=EPS)
    gen = torch.Generator(device=DEV).manual_seed(0)
    res = ppo_update(a, opt, s, update_epochs=4, minibatch_size=256, target_kl=0.0, generator=gen,
                     device_nets=DeviceNets(a, operands="bf16"))
    assert res["optimizer_steps"] == 32 and res["gated"] == 0
    for name in ("policy_loss", "value_loss", "entropy", "approx_kl", "first_approx_kl", "clipfrac", "grad_norm"):
        print(f"ppo_update(bf16 nets) {name}: {res[name]:+.6e}")
        assert np.isfinite(res[name]), name
    assert all(not torch.equal(x, y) for x, y in zip(bits(a.parameters()), bits(agent.parameters())))
    assert all(bool(torch.isfinite(p).all()) for p in a.parameters())
    assert int(s.errors.item()) == 0


def test_cli_net_operands_bf16():
    """python -m splendor_gym.scripts.ppo_device --net-operands bf16 (which implies --device-nets) at the smallest
    shape: two updates, every printed figure finite."""
    for line in run_cli("--update-epochs", "1", "--device-adam", "--net-operands", "bf16", updates=2):
        finite_figures(line, 2)
