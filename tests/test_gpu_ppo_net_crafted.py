"""The PPO network passes (spl_ppo_net_forward / backward and the tiled pair, DeviceNets(tiled=False | True)) on
the crafted networks of crafted_nets.py: the tanh probes (saturated units, H = +-1 and a factor 1 - H^2 of exactly
0, and near-zero ones), the range networks and store rows of all-0 and all-255 bytes with byte 297 in {0, 1, 255}.

Outputs of the probes: 4 ulp (layer-2 probe) and 9 ulp (layer-1 probe) of the float64 oracle, as for the policy
kernels' tanh_acc, of which spl_ppo_net_common.h keeps a copy.  Everything else, gradients included: the rule of
test_gpu_ppo_net.py against test_ppo_net_host.net_oracle, max(4 x torch's float32 error on the same inputs,
64 x 2^-24 x the tensor's largest magnitude).  Every word the tiled pair writes equals the 8-row pair's."""
import numpy as np
import pytest

import crafted_nets as cn
from test_gpu_ppo_loss import DEV
from test_gpu_ppo_net import check, gradients, torch32
from test_gpu_ppo_net_tiled import passes, same_bytes
from test_ppo_net_host import NA, NETS, net_oracle, params_of, tensors_of

pytestmark = pytest.mark.gpu

K, T = 2, 80
P = K * T
B = 150
BAD = (9, 140)  # rows of the minibatch whose position is outside the store


@pytest.fixture(scope="module")
def store():
    """A 2 x 80 store: the 145 compact rows of crafted_nets (all bytes 0; bytes 0..296 all 255 with byte 297 = 0, 1,
    255; real rows with those high bytes) and 15 more real rows.  The tests only read it."""
    import torch
    from splendor_gym.ppo import PPORolloutStore
    s = PPORolloutStore(K, T, DEV)
    s.obs_u8.view(P, 300).copy_(torch.from_numpy(store_rows()).to(DEV))
    torch.cuda.synchronize()
    return s


def store_rows():
    return np.concatenate([cn.compact_rows("ppo"), cn.compact(cn.real_rows(P - cn.SWEEP_N, first=300))])


def minibatch():
    """150 positions: the crafted rows first, duplicates, and two positions outside the store."""
    idx = np.random.default_rng(3).permutation(P)[:B].astype(np.int64)
    idx[:8] = np.arange(8)          # all-0, the all-255 rows, the real rows with a high byte
    idx[20:23] = (1, 3, 3)          # duplicates
    idx[list(BAD)] = (-1, P)
    return idx


def both(label, agent, store):
    """The 8-row pair and the tiled pair on the minibatch: the same bytes everywhere; returns the 8-row pair's
    outputs as float64 in net_oracle's layout, the oracle, torch's float32 results, and the rows."""
    import torch
    agent = agent.to(DEV)
    idx = minibatch()
    dlogits, dvalue = gradients(5, B)
    want = passes(agent, store, idx, dlogits, dvalue, tiled=False)
    got = passes(agent, store, idx, dlogits, dvalue, tiled=True)
    same_bytes(label, got, want)
    assert want["errors"] == (len(BAD), 0)
    f = lambda w, shape: w.view(torch.float32).double().cpu().numpy().reshape(shape)
    shapes = [tuple(p.shape) for p in tensors_of(agent)]
    res = {"logits": f(want["logits"], (B, NA)), "value": f(want["value"], (B,)),
           "grads": {net: [f(v, s) for v, s in zip(want["views"][6 * i:6 * i + 6], shapes[6 * i:6 * i + 6])] for i, net in enumerate(NETS)}}
    bad = (idx < 0) | (idx >= P)
    rows = store_rows()[np.where(bad, 0, idx)]
    oracle = net_oracle(params_of(agent), rows, dlogits, dvalue, bad=bad)
    kept = torch32(agent, rows[~bad], dlogits[~bad], dvalue[~bad])
    ref = {"logits": np.zeros((B, NA)), "value": np.zeros(B), "grads": kept["grads"]}
    ref["logits"][~bad], ref["value"][~bad] = kept["logits"], kept["value"]
    assert not res["logits"][bad].any() and not res["value"][bad].any()
    return res, oracle, ref, bad


@pytest.mark.parametrize("layer", [2, 1])
@pytest.mark.parametrize("image", range(cn.PROBE_IMAGES))
def test_tanh_probes(store, layer, image):
    agent = cn.probe_agent(layer, image)
    res, oracle, ref, bad = both(f"probe layer {layer} image {image}", agent, store)
    arg, want = cn.probe_expected(layer, image)
    got = np.column_stack([res["logits"], res["value"]])[~bad]
    assert (got == got[0]).all()
    u = cn.ulps(got[0], want)
    below = np.abs(arg) < float(cn.BRANCH)
    print(f"tanh_acc ppo layer-{layer} probe image {image}: below 0.625 {u[below].max():.3f} ulp, from 0.625 {u[~below].max():.3f} ulp, "
          f"critic {u[NA]:.3f} ulp")
    assert (u <= cn.PROBE_ULPS[layer]).all(), (arg[u > cn.PROBE_ULPS[layer]], u.max())
    # a saturated unit (|argument| >= 20: H is exactly +-1 in any fp32 evaluation) adds exactly nothing
    w_at, b_at = (2, 3) if layer == 2 else (0, 1)
    for net, sweep in zip(NETS, cn.probe_biases(image)):
        sat = np.abs(sweep.astype(np.float64)) >= cn.SATURATED
        assert sat.sum() >= 14
        g = res["grads"][net]
        assert not g[w_at][sat].any() and not g[b_at][sat].any(), net
        assert np.abs(g[b_at][~sat]).max() > 0 or net == "critic"
    check(f"probe layer {layer} image {image}", res, ref, oracle, B)


def range_agents():
    obs = cn.expand(store_rows())
    return {"hidden": lambda: cn.range_agent("hidden", cn.range_obs()), "out": lambda: cn.range_agent("out", cn.range_obs()),
            "bytes": lambda: cn.sweep_agent(obs)}


@pytest.mark.parametrize("kind", list(range_agents()))
def test_range_networks_and_store_rows(store, kind):
    """The range networks, and ("bytes") a network whose W1 columns are divided by the store's largest value of the
    column, so that the all-255 rows and column 295 = 65 535 stay unsaturated."""
    agent = range_agents()[kind]()
    res, oracle, ref, bad = both(f"range {kind}", agent, store)
    check(f"range {kind}", res, ref, oracle, B)
